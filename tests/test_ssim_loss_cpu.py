"""CPU: the checker of the SSIM loss (tests/ssim_loss_ref.py) against the numpy restatement and the reference's own numbers, its autograd
gradient against central differences, and the argument checks of pnrf_ssim_loss_fwd / pnrf_ssim_loss_workspace_bytes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ssim_loss_ref as R
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
def test_torch_restatement_is_the_numpy_restatement_and_the_reference(golden, kind, H, W):
    """float64, to 1e-12: against ssim_ref.img2ssim_ref on the fixture's images (mean and map), and — with the squares formed in the input's
    precision, as the reference forms them — against the reference's own mean and map in ssim_cases.npz."""
    key = f'{kind}_{H}x{W}'
    a, b = golden[key + '_a'], golden[key + '_b']
    ta, tb = torch.tensor(a).double()[None], torch.tensor(b).double()[None]
    m = R.ssim_map(ta, tb)[0].numpy()
    want = ssim_ref.img2ssim_ref(a, b, return_map=True)
    assert m.shape == want.shape and np.abs(m - want).max() <= 1e-12
    assert abs(float(R.ssim_mean(ta, tb)) - ssim_ref.img2ssim_ref(a, b)) <= 1e-12
    prod = tuple((x * y).double()[None] for x, y in ((torch.tensor(a), torch.tensor(a)), (torch.tensor(b), torch.tensor(b)), (torch.tensor(a), torch.tensor(b))))
    mp = R.ssim_map(ta, tb, products=prod)                                                  # the reference's own numbers
    assert abs(float(mp.mean()) - float(golden[key + '_ssim'])) <= 1e-12
    if key + '_map' in golden:
        assert np.abs(mp[0].numpy() - golden[key + '_map']).max() <= 1e-12
    two = R.ssim_map(torch.cat([ta, tb]), torch.cat([tb, ta]))                              # a batch is its patches
    assert np.abs(two[0].numpy() - want).max() <= 1e-12 and np.abs(two[1].numpy() - ssim_ref.img2ssim_ref(b, a, return_map=True)).max() <= 1e-12


@pytest.mark.parametrize('T', [7, 8, 11])
def test_filter_sizes_of_the_torch_restatement(golden, T):
    a, b = golden['noise_43x75_a'], golden['noise_43x75_b']
    got = float(R.ssim_mean(torch.tensor(a).double()[None], torch.tensor(b).double()[None], filter_size=T))
    assert abs(got - ssim_ref.img2ssim_ref(a, b, filter_size=T)) <= 1e-12


def test_autograd_gradient_against_central_differences():
    """One 12 x 13 patch, T = 5, float64: every element of d mean / d pred against (f(x + h) - f(x - h)) / 2h, h = 1e-6.  The inputs are the GPU
    test's mix, away from both kinks (asserted), so the formula is smooth over the step: truncation ~h^2 f''' and round-off ~1e-16 / h."""
    pred, gt = R.make_inputs(12, 13)
    d0, d1 = R.kink_distances(pred, gt, filter_size=5)
    assert float(d0.min()) > 1e-3 and float(d1.min()) > 1e-3
    val, grad = R.value_and_grad(pred, gt, filter_size=5)
    p, g = torch.tensor(pred).double(), torch.tensor(gt).double()
    h = 1e-6
    num = torch.zeros_like(p)
    flat, nflat = p.view(-1), num.view(-1)
    for i in range(flat.numel()):
        x = float(flat[i])
        flat[i] = x + h
        up = float(R.ssim_mean(p, g, filter_size=5))
        flat[i] = x - h
        dn = float(R.ssim_mean(p, g, filter_size=5))
        flat[i] = x
        nflat[i] = (up - dn) / (2 * h)
    err = float((num - grad).abs().max())
    print(f'\n[ssim loss ref] 12x13 T=5: mean {val:.9f}, |grad| max {float(grad.abs().max()):.3e}, autograd vs central differences {err:.2e}')
    assert float(grad.abs().max()) > 1e-4 and err <= 1e-8


def test_float32_run_of_the_restatement_is_close():
    """The bound of the GPU test is built on this run: it must be a sane fp32 evaluation (relative L2 error of the gradient below 1e-4)."""
    pred, gt = R.make_inputs(33, 37)
    _, g64 = R.value_and_grad(pred, gt)
    _, g32 = R.value_and_grad(pred, gt, dtype=torch.float32)
    assert g32.dtype == torch.float32
    assert float((g32.double() - g64).norm() / g64.norm()) < 1e-4


def test_ssim_loss_argument_errors(lib):
    """Each refusal returns PNRF_E_ARG before any device work (no GPU here), names its entry point and the limit."""
    host = (C.c_double * 64)()                      # stands for device memory: never touched by a refused call
    p = C.c_void_p(C.addressof(host))
    taps = (C.c_float * 16)(*([1 / 11] * 11))

    def loss(pred=p, sp=3, pp=1200, gt=p, sg=3, pg=1200, B=2, H=20, W=20, taps_=taps, T=11, out=p, d=p, ws=p, ws_bytes=1 << 20):
        return lib.pnrf_ssim_loss_fwd(pred, sp, pp, gt, sg, pg, B, H, W, taps_, T, 1.0, 0.01, 0.03, out, d, ws, ws_bytes, None)

    bad = [(dict(pred=None), b'null pointer'), (dict(gt=None), b'null pointer'), (dict(taps_=None), b'null pointer'), (dict(out=None), b'null pointer'),
           (dict(d=None), b'null pointer'), (dict(ws=None), b'null pointer'), (dict(H=10), b'has no 11 x 11 window'), (dict(W=10), b'has no 11 x 11 window'),
           (dict(T=0), b'outside 1 .. 16'), (dict(T=17), b'outside 1 .. 16'), (dict(B=0), b'outside 1 .. 21845'), (dict(B=21846), b'outside 1 .. 21845'),
           (dict(sp=2), b'need >= 3 floats'), (dict(sg=2), b'need >= 3 floats'), (dict(pp=-1), b'need >= 0 floats'), (dict(pg=-1), b'need >= 0 floats'),
           (dict(ws_bytes=8), b'workspace of')]
    for kw, text in bad:
        assert loss(**kw) == -1, kw
        msg = lib.pnrf_last_error()
        assert b'pnrf_ssim_loss_fwd' in msg and text in msg, (kw, msg)
    # workspace: per patch one fp64 partial sum per 32 x 32 tile of windows and channel + three fp32 planes of windows per channel
    wb = lib.pnrf_ssim_loss_workspace_bytes
    assert wb(1, 20, 20, 11) == 3 * 8 + 9 * 10 * 10 * 4
    assert wb(4, 43, 75, 11) == 4 * (2 * 3 * 3 * 8 + 9 * 33 * 65 * 4)
    assert wb(3, 5, 7, 1) == 3 * (3 * 8 + 9 * 5 * 7 * 4)
    for B, H, W, T in ((1, 10, 20, 11), (1, 20, 10, 11), (1, 20, 20, 0), (1, 20, 20, 17), (0, 20, 20, 11), (21846, 20, 20, 11), (1, 0, 0, 1)):
        assert wb(B, H, W, T) == 0, (B, H, W, T)
    assert loss(ws_bytes=wb(2, 20, 20, 11) - 1) == -1 and str(wb(2, 20, 20, 11)).encode() in lib.pnrf_last_error()


def test_the_two_kernels_do_not_spill(lib):
    """Both passes of pnrf_ssim_loss_fwd in the built library: no scratch, LDS within a workgroup's 64 KB, and the metrics instance beside them."""
    from pronerf_amd import build
    k = build.device_kernels()
    names = ['void image_ssim_kernel<true>(MetricsArgs)', 'ssim_grad_gather_kernel(SsimGradArgs)', 'void image_ssim_kernel<false>(MetricsArgs)']
    for n in names:
        assert n in k, [x for x in k if 'ssim' in x]
        assert k[n]['scratch'] == 0 and 0 < k[n]['vgpr'] <= 128 and k[n]['lds'] <= 65536, (n, k[n])


def test_patch_indices_on_the_host_device():
    """The index arithmetic is torch's, so it can be checked where there is no GPU: patch-major, row-major inside, every crop inside one view."""
    from pronerf_amd import ops
    nv, H, W, patch, count = 5, 9, 12, 4, 200
    g = ops.patch_indices(nv, H, W, patch, count, generator=torch.Generator().manual_seed(1)).reshape(count, patch, patch)
    assert g.dtype == torch.int64
    v, y, x = g // (H * W), g % (H * W) // W, g % W
    k = torch.arange(patch)
    assert bool((v == v[:, :1, :1]).all()) and bool((y == y[:, :1, :1] + k[None, :, None]).all()) and bool((x == x[:, :1, :1] + k[None, None, :]).all())
    assert int(g.min()) >= 0 and int(v.max()) < nv and int(y.max()) < H and int(x.max()) < W
    corners = {(int(a), int(b), int(c)) for a, b, c in zip(v[:, 0, 0], y[:, 0, 0], x[:, 0, 0])}
    assert {c[0] for c in corners} == set(range(nv)) and {c[1] for c in corners} == set(range(H - patch + 1)) and {c[2] for c in corners} == set(range(W - patch + 1))


def test_patch_indices_and_ssim_loss_refuse_bad_arguments(lib):
    from pronerf_amd import autograd, ops
    from pronerf_amd._lib import PnrfError
    for kw in (dict(patch=0), dict(patch=9), dict(count=0), dict(nv=0)):
        a = dict(nv=3, H=8, W=12, patch=4, count=2)
        a.update(kw)
        with pytest.raises(PnrfError, match='patch_indices'):
            ops.patch_indices(**a)
    with pytest.raises(PnrfError, match='ssim_loss'):
        ops.ssim_loss(torch.zeros(12, 12), torch.zeros(12, 12))
    with pytest.raises(PnrfError, match='filter_size 11 must be 1 .. 16 and fit'):
        ops.ssim_loss(torch.zeros(2, 10, 12, 3), torch.zeros(2, 10, 12, 3))
    with pytest.raises(PnrfError, match='expected a GPU tensor'):
        autograd.ssim(torch.zeros(2, 12, 12, 3), torch.zeros(2, 12, 12, 3))
