"""Checker for the SSIM loss: ``img2ssim`` (run_nerf_helpers.py:151-197, as tests/ssim_ref.py restates it) for batches of patches in torch, so
that autograd differentiates it, and the distance of every window to the two kinks of its formula.

The arithmetic follows tests/ssim_ref.py line for line — columns filtered first, rows second, the clamp as ``torch.maximum``, the limiter as
``torch.sign * torch.minimum`` — in the dtype of the inputs: float64 is the yardstick, float32 on the CPU shows what the same formulas and
their autograd cost in straightforward single precision (the bound of tests/test_ssim_loss_gpu.py).
"""
import numpy as np
import torch

import ssim_ref


def _filter_axis(z, w, axis):
    """'valid' convolution along one axis: out[i] = sum_k w[k] z[i + T - 1 - k]."""
    T = w.shape[0]
    n = z.shape[axis] - T + 1
    out = torch.zeros_like(z.narrow(axis, 0, n))
    for k in range(T):
        out = out + w[k] * z.narrow(axis, T - 1 - k, n)
    return out


def _moments(pred, gt, filter_size, filter_sigma, products=None):
    assert pred.dim() == 4 and pred.shape[-1] == 3 and pred.shape == gt.shape and pred.dtype == gt.dtype
    w = torch.tensor(ssim_ref.filter_taps(filter_size, filter_sigma), dtype=pred.dtype)
    blur = lambda z: _filter_axis(_filter_axis(z, w, 1), w, 2)
    mu0, mu1 = blur(pred), blur(gt)
    aa, bb, ab = (pred * pred, gt * gt, pred * gt) if products is None else products
    return mu0, mu1, blur(aa) - mu0 * mu0, blur(bb) - mu1 * mu1, blur(ab) - mu0 * mu1


def ssim_map(pred, gt, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, products=None):
    """[B,H,W,3] x 2 -> the SSIM map [B,H-T+1,W-T+1,3], differentiable.  ``products``: (pred^2, gt^2, pred gt) formed elsewhere — in the
    input's float32, as the reference forms them before its float64 filter (``input_products`` of tests/ssim_ref.py)."""
    mu0, mu1, r00, r11, r01 = _moments(pred, gt, filter_size, filter_sigma, products)
    zero = torch.zeros((), dtype=pred.dtype)
    s00, s11 = torch.maximum(zero, r00), torch.maximum(zero, r11)
    s01 = torch.sign(r01) * torch.minimum(torch.sqrt(s00 * s11), torch.abs(r01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return ((2 * mu0 * mu1 + c1) * (2 * s01 + c2)) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))


def ssim_mean(pred, gt, **kw):
    return ssim_map(pred, gt, **kw).mean()


def value_and_grad(pred, gt, dtype=torch.float64, **kw):
    """numpy / tensors [B,H,W,3] -> (mean SSIM as a float, d mean / d pred as a ``dtype`` tensor), by autograd in ``dtype`` on the CPU."""
    p = torch.as_tensor(np.asarray(pred)).to(dtype).clone().requires_grad_(True)
    g = torch.as_tensor(np.asarray(gt)).to(dtype)
    m = ssim_mean(p, g, **kw)
    m.backward()
    return float(m.detach()), p.grad


def kink_distances(pred, gt, filter_size=11, filter_sigma=1.5):
    """Per window and channel, the relative distances to the two kinks, in float64: (|s00| / F[x^2], | |s01| - sqrt(v0 v1) | / sqrt(v0 v1)).
    The first is the prediction's variance over the window against its filtered second moment — the two terms whose difference the clamp
    sees —, 0 on the clamp's kink; the second is 0 where the limiter switches.  A window is within r of a kink when either is below r."""
    p, g = torch.as_tensor(np.asarray(pred)).double(), torch.as_tensor(np.asarray(gt)).double()
    mu0, mu1, r00, r11, r01 = _moments(p, g, filter_size, filter_sigma)
    scale = r00 + mu0 * mu0                                   # the filtered E[x^2] of the window
    lim = torch.sqrt(torch.clamp(r00, min=0) * torch.clamp(r11, min=0))
    return r00.abs() / scale, (torch.abs(r01) - lim).abs() / lim


def make_inputs(H, W, B=1, mix=0.6, seed=0):
    """gt: the seeded 'noise' images of tests/ssim_ref.py (their first member), one per patch; pred = mix gt + (1 - mix) independent seeded noise.
    float32 [B,H,W,3] each.  Cauchy-Schwarz has slack (the correlation is about mix / sqrt(mix^2 + (1 - mix)^2)) and both variances are those
    of uniform noise, far from 0."""
    gt = np.stack([ssim_ref.make_pair('noise', H, W, seed=seed + b)[0] for b in range(B)])
    noise = np.random.RandomState(4242 + 31 * seed + 97 * H + W).uniform(0, 1, gt.shape)
    return (mix * gt + (1 - mix) * noise).astype(np.float32), gt.astype(np.float32)
