"""CPU: the checker of the image metrics against the reference's own numbers (tests/golden/ssim_cases.npz, written by tools/gen_ssim_golden.py
from the reference's img2ssim), the filter helper, the argument checks of the three frame-tail entry points and the reference-named face."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(kind, H, W) for H, W in ssim_ref.FIXTURE_SHAPES for kind in ssim_ref.KINDS]


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'ssim_cases.npz')))


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('kind,H,W', CASES)
def test_restatement_reproduces_the_reference(golden, kind, H, W):
    """The numpy restatement, with the products formed in the input's precision as the reference forms them (fp32 squares of fp32 images,
    run_nerf_helpers.py:181-183), against the reference's mean: within 1e-6 (measured: 0).  The fixture's images are the seeded generator's.
    In pure float64 — the yardstick of the GPU tests — the restatement differs from the reference by those fp32 squares alone: up to 2.4e-6
    on the mean (flat, 12 x 17: E[x^2] - mu^2 cancels to 1e-6 of its terms there), below 2.1e-7 in the seven other cases; printed."""
    key = f'{kind}_{H}x{W}'
    a, b = golden[key + '_a'], golden[key + '_b']
    ga, gb = ssim_ref.make_pair(kind, H, W)
    assert a.dtype == np.float32 and np.array_equal(a, ga) and np.array_equal(b, gb)
    want = float(golden[key + '_ssim'])
    got = ssim_ref.img2ssim_ref(a, b, input_products=True)
    pure = ssim_ref.img2ssim_ref(a, b)
    print(f'\n[ssim restatement] {key}: reference {want:.12f}, restatement - reference {got - want:.3e}, in pure float64 {pure - want:.3e}')
    assert abs(got - want) <= 1e-6
    assert abs(pure - want) <= 1e-5
    if key + '_map' in golden:
        m = ssim_ref.img2ssim_ref(a, b, return_map=True, input_products=True)
        assert m.shape == (H - 10, W - 10, 3) == golden[key + '_map'].shape
        assert np.abs(m - golden[key + '_map']).max() <= 1e-6


def test_filter_sizes_of_the_restatement(golden):
    a, b = golden['noise_43x75_a'], golden['noise_43x75_b']
    for T in (7, 8, 11):
        assert abs(ssim_ref.img2ssim_ref(a, b, filter_size=T, input_products=True) - float(golden[f'ssim_noise_43x75_T{T}'])) <= 1e-6


@pytest.mark.parametrize('T', [7, 8, 11])
def test_filter_helper_is_the_reference_filter(golden, T):
    """ops.ssim_filter (what the kernel is handed, rounded to fp32) and the checker's filter_taps against the 1-D filter the reference gave
    scipy: exact in float64, the even size with its half-tap shift included."""
    from pronerf_amd import ops
    want = golden[f'taps_{T}']
    assert want.dtype == np.float64 and want.shape == (T,)
    assert np.array_equal(ops.ssim_filter(T, 1.5), want)
    assert np.array_equal(ssim_ref.filter_taps(T, 1.5), want)
    assert np.array_equal(want, want[::-1]) and abs(want.sum() - 1) < 1e-15


def test_frame_tail_argument_errors(lib):
    """Each refusal returns PNRF_E_ARG before any device work (no GPU here) and names its entry point."""
    host = (C.c_double * 64)()                      # stands for device memory: never touched by a refused call
    p = C.c_void_p(C.addressof(host))
    taps = (C.c_float * 16)(*([1 / 11] * 11))

    def metrics(pred=p, sp=3, gt=p, sg=3, H=20, W=20, taps_=taps, T=11, out=p, ws=p, ws_bytes=512):
        return lib.pnrf_image_metrics_fwd(pred, sp, gt, sg, H, W, taps_, T, 1.0, 0.01, 0.03, out, None, ws, ws_bytes, None)

    bad = [dict(pred=None), dict(gt=None), dict(taps_=None), dict(out=None), dict(ws=None), dict(H=10), dict(W=10), dict(H=0, W=0), dict(T=0), dict(T=17),
           dict(sp=2), dict(sg=2), dict(ws_bytes=8)]
    for kw in bad:
        assert metrics(**kw) == -1, kw
        assert b'pnrf_image_metrics_fwd' in lib.pnrf_last_error(), kw
    assert lib.pnrf_image_metrics_workspace_bytes(20, 20, 11) == 3 * 16 and lib.pnrf_image_metrics_workspace_bytes(756, 1008, 11) == 24 * 32 * 3 * 16
    for H, W, T in ((10, 20, 11), (20, 10, 11), (20, 20, 0), (20, 20, 17), (0, 0, 1)):
        assert lib.pnrf_image_metrics_workspace_bytes(H, W, T) == 0

    def to8b(rgb=p, sr=4, depth=p, sd=4, n=5, rgb8=p, depth8=p, ws=p, ws_bytes=4096):
        return lib.pnrf_frame_to8b_fwd(rgb, sr, depth, sd, n, rgb8, depth8, ws, ws_bytes, None)

    for kw in (dict(rgb8=None, depth8=None), dict(rgb=None), dict(depth=None), dict(sr=2), dict(sd=0), dict(n=-1), dict(ws=None), dict(ws_bytes=100)):
        assert to8b(**kw) == -1, kw
        assert b'pnrf_frame_to8b_fwd' in lib.pnrf_last_error(), kw
    assert to8b(n=0) == 0                           # an empty frame is a no-op, like the other operators


def test_img2ssim_has_the_reference_signature():
    from pronerf_amd import run_nerf_helpers as h
    params = inspect.signature(h.img2ssim).parameters
    assert [(k, v.default) for k, v in params.items()] == [('img0', inspect.Parameter.empty), ('img1', inspect.Parameter.empty), ('max_val', 1),
                                                           ('filter_size', 11), ('filter_sigma', 1.5), ('k1', 0.01), ('k2', 0.03), ('return_map', False)]
    x = np.linspace(0.01, 1, 7)
    assert h.img2mse_np(x, x * 0.5) == np.mean((x * 0.5) ** 2) and h.mse2psnr_np(0.01) == 20.0
