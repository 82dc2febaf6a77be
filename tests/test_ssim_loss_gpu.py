"""GPU: the SSIM loss — pnrf_ssim_loss_fwd through ops.ssim_loss and autograd.ssim, ops.patch_indices and the stage-2 driver's patch_size.

Both kernels work on 32 x 32 tiles (windows in the first pass, pixels in the second; one workgroup per tile, patch and channel), so the shapes
are, per filter size T: 11 — 11 x 11 (one window), 12 x 11, 33 x 37 (23 x 27 windows, two pixel tiles in both directions with ragged edges),
64 x 64 (54 x 54 windows: two window tiles in both directions); 1 — 5 x 7; 8 — 20 x 9 (even filter); 16 — 16 x 47 (the largest filter, one row
of windows).  B is 1 and 3, the pixel strides 3 and 4, and the patches lie further apart than a patch is long.

Gradient bound, per case (the protocol of test_custom_loss_gpu.py): relative L2 error against float64 autograd of tests/ssim_loss_ref.py
<= 4 x the error of the same restatement run in float32 on the CPU + 2e-5.  The inputs (ssim_loss_ref.make_inputs) keep every window away
from the two kinks of the formula, which the test asserts on the CPU before it looks at the kernel.  With T = 1 that cannot be done: a
one-tap window has exactly zero variance, so EVERY window sits on both kinks whatever the images are, and float64 autograd returns NaN there
(the derivative of sqrt at 0).  The 5 x 7 / T = 1 shape therefore runs in the value, determinism and finiteness tests, not in the comparison
with autograd."""
import functools

import numpy as np
import pytest
import torch

import ssim_loss_ref as R
import ssim_ref

pytestmark = pytest.mark.gpu

SHAPES = [(11, 11, 11), (11, 12, 11), (11, 33, 37), (11, 64, 64), (1, 5, 7), (8, 20, 9), (16, 16, 47)]      # (T, H, W)
SMOOTH = [s for s in SHAPES if s[0] > 1]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case(T, H, W, B):
    """(pred, gt, float64 mean, float64 gradient, relative L2 error of the float32 CPU run's gradient, smallest distance to a kink) — computed
    once per case, shared, never written to."""
    pred, gt = R.make_inputs(H, W, B)
    d0, d1 = R.kink_distances(pred, gt, filter_size=T)
    if T == 1:
        return pred, gt, float(R.ssim_mean(torch.tensor(pred).double(), torch.tensor(gt).double(), filter_size=1)), None, None, float(d0.max())
    v64, g64 = R.value_and_grad(pred, gt, filter_size=T)
    _, g32 = R.value_and_grad(pred, gt, dtype=torch.float32, filter_size=T)
    return pred, gt, v64, g64, rel(g32, g64), min(float(d0.min()), float(d1.min()))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def _place(x, dev, stride):
    """Device view [B,H,W,3] of x with ``stride`` floats per pixel and five pixels of filler between the patches: nothing is contiguous but a pixel."""
    B, H, W, _ = x.shape
    big = torch.full((B, H * W + 5, stride), 7.0, device=dev)
    big[:, :H * W, :3] = torch.as_tensor(x, device=dev).reshape(B, H * W, 3)
    v = torch.as_strided(big, (B, H, W, 3), ((H * W + 5) * stride, W * stride, stride, 1))
    assert v.data_ptr() == big.data_ptr() and torch.equal(v, torch.as_tensor(x, device=dev))
    return v


# ------------------------------------------------------------------------------------------------ value
@pytest.mark.parametrize('T,H,W', SHAPES)
def test_one_patch_has_the_bits_of_image_metrics(dev, T, H, W):
    """The test inputs and the four image kinds of tests/ssim_ref.py ('flat': the clamp at work, 'anti': the limiter's negative branch)."""
    from pronerf_amd import ops
    pairs = [tuple(x[0] for x in _case(T, H, W, 1)[:2])] + [ssim_ref.make_pair(kind, H, W) for kind in ssim_ref.KINDS]
    for a, b in pairs:
        want = ops.image_metrics(torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev), filter_size=T)[3]
        for stride in (3, 4):
            mean, d = ops.ssim_loss(_place(a[None], dev, stride), _place(b[None], dev, 7 - stride), filter_size=T)
            assert mean.dtype == torch.float64 and mean.dim() == 0 and d.dtype == torch.float32 and d.shape == (1, H, W, 3) and d.is_contiguous()
            assert torch.equal(mean, want), (float(mean), float(want))
        mean3, d3 = ops.ssim_loss(torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev), filter_size=T)           # [H,W,3] in, [H,W,3] out
        assert torch.equal(mean3, want) and d3.shape == (H, W, 3) and torch.equal(d3, d[0])


@pytest.mark.parametrize('T,H,W', SHAPES)
def test_three_patches_sum_their_single_sums(dev, T, H, W):
    """The sum over the batch (mean x N: one more rounding, 2^-53 relative) within N 2^-52 relative of the fp64 sum of the three patches' own sums,
    and the gradient of a batch is that of its patches over 3 — the same products, one more rounding of the scale."""
    from pronerf_amd import ops
    pred, gt = _case(T, H, W, 3)[:2]
    n = 3 * (H - T + 1) * (W - T + 1) * 3
    for stride in (3, 4):
        p, g = _place(pred, dev, stride), _place(gt, dev, stride)
        mean, d = ops.ssim_loss(p, g, filter_size=T)
        singles = [ops.ssim_loss(p[i:i + 1], g[i:i + 1], filter_size=T) for i in range(3)]
        sums = [float(ops.image_metrics(torch.as_tensor(pred[i], device=dev), torch.as_tensor(gt[i], device=dev), filter_size=T)[2]) for i in range(3)]
        want = sums[0] + sums[1] + sums[2]
        assert abs(float(mean) * n - want) <= n * 2.0 ** -52 * abs(want), (float(mean) * n, want)
        assert abs(float(mean) - _case(T, H, W, 3)[2]) <= 1e-5
        for i in range(3):
            assert float((d[i] * 3 - singles[i][1][0]).abs().max()) <= 2.0 ** -22 * float(singles[i][1].abs().max())


# ------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T,H,W', SMOOTH)
def test_gradient_against_float64_autograd(dev, T, H, W, B):
    from pronerf_amd import ops
    pred, gt, v64, g64, e32, kink = _case(T, H, W, B)
    assert kink > 1e-6, f'a window within 1e-6 of a kink ({kink:.2e}): change the mix of ssim_loss_ref.make_inputs'
    for stride in (3, 4):
        mean, d = ops.ssim_loss(_place(pred, dev, stride), _place(gt, dev, stride), filter_size=T)
        e = rel(d, g64)
        print(f'\n[ssim loss] T {T} {H}x{W} B {B} stride {stride}: mean {float(mean):.9f} (float64 {v64:.9f}), gradient error {e:.2e} '
              f'(fp32 CPU autograd {e32:.2e}, ratio {e / e32:.2f}); nearest kink {kink:.1e}')
        assert abs(float(mean) - v64) <= 1e-5
        assert e <= 4 * e32 + 2e-5, (e, e32)


def test_one_tap_filter_sits_on_the_kinks_and_stays_finite(dev):
    """T = 1 (module docstring): every window has zero variance — asserted on the reference —, the kernel takes its stated branches there."""
    from pronerf_amd import ops
    for B in (1, 3):
        pred, gt, v64, _, _, kink = _case(1, 5, 7, B)
        assert kink == 0.0
        mean, d = ops.ssim_loss(_place(pred, dev, 4), _place(gt, dev, 3), filter_size=1)
        assert abs(float(mean) - v64) <= 1e-5 and bool(torch.isfinite(d).all())


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_identical_and_constant_patches(dev):
    from pronerf_amd import ops
    gt = torch.as_tensor(_case(11, 33, 37, 3)[1], device=dev)
    for name, x in (('pred == gt', gt), ('constant', torch.full((3, 33, 37, 3), 0.7, device=dev))):
        mean, d = ops.ssim_loss(x.clone(), x, filter_size=11)
        print(f'\n[ssim loss] {name}: mean - 1 = {float(mean) - 1:.2e}, |gradient| max {float(d.abs().max()):.2e}')
        assert abs(float(mean) - 1) <= 1e-6, name
        assert bool(torch.isfinite(d).all()), name


def test_a_nan_pixel_stays_in_its_windows(dev):
    """64 x 64, T = 11, the NaN at (35, 30) of patch 1: its windows span both window tiles and all four pixel tiles.  NaN exactly on the
    pixels that share a window with it; every other element — the other patches too — has the clean run's bits."""
    from pronerf_amd import ops
    T, H, W = 11, 64, 64
    pred, gt = (torch.as_tensor(x, device=dev) for x in _case(T, H, W, 3)[:2])
    _, clean = ops.ssim_loss(pred, gt, filter_size=T)
    bad = pred.clone()
    qy, qx = 35, 30
    bad[1, qy, qx, :] = float('nan')
    mean, d = ops.ssim_loss(bad, gt, filter_size=T)
    span = lambda q, n: (max(0, q - T + 1), min(n - T, q) + T)              # pixels of the windows that hold q
    mask = torch.zeros(3, H, W, 3, dtype=torch.bool, device=dev)
    (y0, y1), (x0, x1) = span(qy, H), span(qx, W)
    mask[1, y0:y1, x0:x1, :] = True
    assert bool(torch.isnan(mean)) and int(mask.sum()) == 21 * 21 * 3
    assert torch.equal(torch.isnan(d), mask)
    assert torch.equal(d[~mask], clean[~mask])
    bad_gt = gt.clone()
    bad_gt[1, qy, qx, 1] = float('nan')                                      # in the ground truth, one channel
    _, d = ops.ssim_loss(pred, bad_gt, filter_size=T)
    mask[:] = False
    mask[1, y0:y1, x0:x1, 1] = True
    assert torch.equal(torch.isnan(d), mask) and torch.equal(d[~mask], clean[~mask])


# ------------------------------------------------------------------------------------------------ determinism
def test_two_streams_give_the_same_bits(dev):
    from pronerf_amd import ops
    for T, H, W in ((11, 64, 64), (1, 5, 7)):
        pred, gt = (_place(x, dev, 4) for x in _case(T, H, W, 3)[:2])
        m0, d0 = ops.ssim_loss(pred, gt, filter_size=T)
        torch.cuda.synchronize()
        got = []
        for s in (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)):
            with torch.cuda.stream(s):
                got.append(ops.ssim_loss(pred, gt, filter_size=T))
        torch.cuda.synchronize()
        for m, d in got:
            assert torch.equal(m, m0) and torch.equal(d, d0)


# ------------------------------------------------------------------------------------------------ autograd.ssim
def test_autograd_ssim_is_the_kernel_gradient_times_the_incoming_one(dev):
    from pronerf_amd import autograd, ops
    pred, gt = (torch.as_tensor(x, device=dev) for x in _case(8, 20, 9, 3)[:2])
    mean, d = ops.ssim_loss(pred, gt, filter_size=8)
    p = pred.clone().requires_grad_(True)
    g = gt.clone().requires_grad_(True)
    s = autograd.ssim(p, g, filter_size=8)
    assert s.dtype == torch.float32 and s.dim() == 0 and torch.equal(s, mean.float())
    (1 - s).backward()
    assert torch.equal(p.grad, -d) and g.grad is None
    # a weighted sum with an mse term: the two gradients, summed
    lam = 0.2
    p1 = pred.clone().requires_grad_(True)
    (((p1 - gt) ** 2).mean() + lam * (1 - autograd.ssim(p1, gt, filter_size=8))).backward()
    p2 = pred.clone().requires_grad_(True)
    ((p2 - gt) ** 2).mean().backward()
    assert torch.equal(p1.grad, p2.grad + torch.tensor(-lam, device=dev) * d)
    # the prediction as the trainer leaves it: rows of an [n, 3] map, reshaped by the loss
    rows = pred.reshape(-1, 3).clone().requires_grad_(True)
    (1 - autograd.ssim(rows.reshape(3, 20, 9, 3), gt, filter_size=8)).backward()
    assert torch.equal(rows.grad, -d.reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ patches
def _small_set(dev, nv=6, H=10, W=14):
    from pronerf_amd import ops
    rs = np.random.RandomState(3)
    poses = np.concatenate([np.tile(np.eye(3, dtype=np.float32), (nv, 1, 1)), rs.uniform(-1, 1, (nv, 3, 1)).astype(np.float32)], 2)
    images = rs.rand(nv, H, W, 3).astype(np.float32)
    f = 1.3 * W
    K = np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1]], dtype=np.float32)
    return images, ops.TrainSet(ops.Scene.from_views(poses, images, K, device=dev), 512, near=0., far=1.)


def test_patch_indices_are_crops_of_single_views(dev):
    from pronerf_amd import ops
    nv, H, W, patch, count = 6, 10, 14, 4, 32
    images, tset = _small_set(dev, nv, H, W)
    gen = torch.Generator(device=dev).manual_seed(5)
    idx = ops.patch_indices(nv, H, W, patch, count, generator=gen)
    assert idx.dtype == torch.int64 and idx.device == dev and idx.shape == (count * patch * patch,)
    g = idx.reshape(count, patch, patch).cpu()
    v, y, x = g // (H * W), g % (H * W) // W, g % W
    assert bool((v == v[:, :1, :1]).all()) and 0 <= int(v.min()) and int(v.max()) < nv                     # one view per patch
    k = torch.arange(patch)
    assert bool((y == y[:, :1, :1] + k[None, :, None]).all()) and bool((x == x[:, :1, :1] + k[None, None, :]).all())      # row-major inside
    assert int(y.max()) < H and int(x.max()) < W and int(y[:, 0, 0].max()) <= H - patch and int(x[:, 0, 0].max()) <= W - patch
    assert len({(int(a), int(b), int(c)) for a, b, c in zip(v[:, 0, 0], y[:, 0, 0], x[:, 0, 0])}) > count // 2      # placed, not repeated
    gen.manual_seed(5)
    assert torch.equal(ops.patch_indices(nv, H, W, patch, count, generator=gen), idx)
    assert ops.patch_indices(nv, H, W, H, 3, device=dev).shape == (3 * H * H,)                              # a patch as tall as the view
    target = tset.batch(idx, (0, 1, 2, 3))[2].reshape(count, patch, patch, 3).cpu().numpy()
    for i in range(count):
        vi, yi, xi = int(v[i, 0, 0]), int(y[i, 0, 0]), int(x[i, 0, 0])
        assert np.array_equal(target[i], images[vi, yi:yi + patch, xi:xi + patch]), i


# ------------------------------------------------------------------------------------------------ driver
def test_driver_trains_on_patches_with_mse_and_ssim(dev, tmp_path, monkeypatch):
    import test_custom_loss_gpu as CL
    from pronerf_amd import autograd, ops
    from pronerf_amd import run_S_eS_eN_alter_base_refine2 as s2
    from pronerf_amd._lib import PnrfError
    cfg = CL._driver_setup(tmp_path, 'scene')
    lam, patch, T = 0.2, 8, 7
    seen, cots = [], []

    def loss_fn(maps, target, step):
        assert tuple(maps['rgb_map1'].shape) == (512, 3) and tuple(target.shape) == (512, 3)
        pred, gt = maps['rgb_map1'].reshape(-1, patch, patch, 3), target.reshape(-1, patch, patch, 3)
        if step == 1:
            seen.append((maps['rgb_map1'].detach().clone(), target.clone()))
        return ((maps['rgb_map1'] - target) ** 2).mean() + lam * (1 - autograd.ssim(pred, gt, filter_size=T))

    backward = ops.Trainer.backward

    def spy(self, **cot):
        cots.append({k: v.clone() for k, v in cot.items()})
        return backward(self, **cot)
    monkeypatch.setattr(ops.Trainer, 'backward', spy)
    CL._seed()
    tr, log = s2.train(['--config', cfg('patches'), '--max_steps', '3', '--device_batches', 'all', '--i_print', '1'], device=dev, loss_fn=loss_fn,
                       patch_size=patch)
    assert len(cots) == 3 and [e[0] for e in log] == [1, 2, 3] and all(np.isfinite(e[1]) and np.isfinite(e[2]) for e in log)
    assert all(bool(torch.isfinite(t).all()) for i in range(26) for t in tr.read('param', i))
    # the first iteration's cotangent: the mse gradient as autograd forms it + (-lam) x the kernel's gradient
    rgb, target = seen[0]
    assert sorted(cots[0]) == ['rgb_map1']
    r = rgb.clone().requires_grad_(True)
    ((r - target) ** 2).mean().backward()
    _, d = ops.ssim_loss(rgb.reshape(-1, patch, patch, 3), target.reshape(-1, patch, patch, 3), filter_size=T)
    assert torch.equal(cots[0]['rgb_map1'], r.grad + torch.tensor(-lam, device=dev) * d.reshape(-1, 3))
    assert float(d.abs().max()) > 0
    # what patch batches need
    for argv, kw in ((['--device_batches', 'off'], dict(patch_size=8)), (['--device_batches', 'all'], dict(patch_size=7)),
                     (['--device_batches', 'rays'], dict(patch_size=-1))):
        with pytest.raises(PnrfError, match='patch_size'):
            s2.train(['--config', cfg('refused'), '--max_steps', '1'] + argv, device=dev, loss_fn=loss_fn, **kw)
