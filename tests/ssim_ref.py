"""Checker for the image metrics: the reference's ``img2ssim`` (run_nerf_helpers.py:151-197) restated with numpy only, and the seeded test images.

The reference filters with ``scipy.signal.convolve2d(..., mode='valid')``, columns first and rows second (:170-175); a 'valid' convolution
with a T-tap filter is a sum of T shifted slices, which is what ``_filter_axis`` adds up.  ``dtype`` selects the arithmetic: float64 is the
yardstick, float32 shows what the same formulas cost in straightforward single precision (the bound of tests/test_metrics_gpu.py).
"""
import numpy as np

KINDS = ('noise', 'smooth', 'flat', 'anti')
FIXTURE_SHAPES = ((12, 17), (43, 75))


def filter_taps(filter_size=11, filter_sigma=1.5):
    """:163-167 — T taps one pixel apart, centred on zero (an even T: half a tap off the grid), Gaussian, normalised; float64."""
    centre = filter_size // 2 - (2 * (filter_size // 2) - filter_size + 1) / 2
    expo = ((np.arange(filter_size) - centre) / filter_sigma) ** 2
    w = np.exp(-0.5 * expo)
    return w / np.sum(w)


def _filter_axis(z, w, axis):
    """'valid' convolution of z with w along one axis: out[i] = sum_k w[k] z[i + T - 1 - k]  (:170-171)."""
    T = len(w)
    n = z.shape[axis] - T + 1
    out = np.zeros_like(np.take(z, range(n), axis=axis))
    for k in range(T):
        out = out + w[k] * np.take(z, range(T - 1 - k, T - 1 - k + n), axis=axis)
    return out


def img2ssim_ref(img0, img1, max_val=1, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False, dtype=np.float64, input_products=False):
    """``input_products``: form a^2, b^2 and ab in the precision of the INPUT before they are filtered, as the reference's ``img0**2`` and
    ``img0 * img1`` do (:181-183: fp32 products of fp32 images, then a float64 convolution) — what its own numbers contain.  Off, every
    operation runs in ``dtype``: with float64 the exact value of the formulas, the yardstick for an implementation."""
    assert img0.ndim == 3 and img0.shape[-1] == 3 and img0.shape == img1.shape          # :158-160
    a, b = np.asarray(img0, dtype=dtype), np.asarray(img1, dtype=dtype)
    aa, bb, ab = ((img0 * img0).astype(dtype), (img1 * img1).astype(dtype), (img0 * img1).astype(dtype)) if input_products else (a * a, b * b, a * b)
    w = filter_taps(filter_size, filter_sigma).astype(dtype)
    blur = lambda z: _filter_axis(_filter_axis(z, w, 0), w, 1)                          # :173-175, the channels together
    mu0, mu1 = blur(a), blur(b)                                                         # :176-177
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1                                  # :178-180
    s00 = np.maximum(dtype(0), blur(aa) - mu00)                                         # :181, 187
    s11 = np.maximum(dtype(0), blur(bb) - mu11)                                         # :182, 188
    s01 = blur(ab) - mu01                                                              # :183
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))                    # :189-190
    c1, c2 = dtype((k1 * max_val) ** 2), dtype((k2 * max_val) ** 2)                     # :191-192
    ssim_map = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))   # :193-195
    assert ssim_map.dtype == dtype
    return ssim_map if return_map else np.mean(ssim_map, dtype=np.float64)              # :196-197


def make_pair(kind, H, W, seed=0):
    """Two float32 [H,W,3] images.  noise: uniform and itself + N(0, 0.05); smooth: sinusoids and themselves + N(0, 0.01); flat: 0.7 + N(0, 1e-3)
    twice (E[x^2] - mu^2 cancels to 1e-6 of its terms); anti: b = 1 - a (negative covariance: the sign / min branch)."""
    rs = np.random.RandomState(1000 * seed + 97 * H + W + 7 * KINDS.index(kind))
    if kind == 'noise':
        a = rs.uniform(0, 1, (H, W, 3))
        b = a + 0.05 * rs.randn(H, W, 3)
    elif kind == 'smooth':
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (x / (9.0 + 4 * c) + y / (13.0 - 3 * c)) + c) for c in range(3)], -1)
        b = a + 0.01 * rs.randn(H, W, 3)
    elif kind == 'flat':
        a = 0.7 + 1e-3 * rs.randn(H, W, 3)
        b = 0.7 + 1e-3 * rs.randn(H, W, 3)
    elif kind == 'anti':
        a = rs.uniform(0, 1, (H, W, 3))
        b = 1 - a
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)
