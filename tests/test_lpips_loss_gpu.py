"""GPU: the LPIPS loss — pnrf_lpips_loss_fwd, pnrf_lpips_layer_bwd and pnrf_lpips_tap_bwd through ops.Lpips, autograd.lpips and the stage-2 driver's
--a_p.

The data-gradient kernel works on tiles of 64 pixels x 64 channels, 32 channels of one filter tap per step, so the layer shapes are those of
tests/test_lpips_gpu.py: output 1 x 1, 7 x 19 (133 pixels per image: full tiles and a partial one, an odd width) and 5 x 1, for 1 and 3 images; the
pooling inputs have one row and column more than the windows cover.

Bound of every comparison with float64 autograd of tests/lpips_loss_ref.py, per case: the relative L2 error e32 of the SAME formulas in float32 on
the CPU; the kernels may err 4 e32 + 2e-5 — their sums run in another order.  The whole-gradient cases are the admissible ones of
lpips_loss_ref.CASES (tests/test_lpips_loss_cpu.py asserts their margins; the test below asserts them again before it looks at the device).

Measured on the MI355X: DESIGN §7.4."""
import functools

import numpy as np
import pytest
import torch

import lpips_loss_ref as L
import lpips_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_handles = {}


@functools.lru_cache(maxsize=None)
def _int_net(net):
    return R.make_int_net(net)


def _lp(net, kind='seeded'):
    from pronerf_amd import ops
    if (net, kind) not in _handles:
        _handles[net, kind] = ops.Lpips(net, *R.state_dicts(net, _int_net(net) if kind == 'int' else R.cached_net(net)))
    return _handles[net, kind]


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


# ---- 1. exact layer gradients ---------------------------------------------------------------------------------------------------------------------
_same = lambda n: n
_pool2 = lambda n: 2 * n + 1                       # 2 / 2 windows and a dropped row / column
_pool3 = lambda n: 2 * n + 2                       # 3 / 2 windows (overlapping) and a dropped row / column
# (net, layer, pool in front, input size for an output of n pixels along one axis)
GEOMETRIES = [('alex', 0, False, lambda n: 4 * (n - 1) + 8), ('alex', 1, False, _same), ('alex', 1, True, _pool3), ('alex', 2, False, _same), ('alex', 2, True, _pool3),
              ('alex', 3, False, _same), ('alex', 4, False, _same),
              ('vgg', 0, False, _same), ('vgg', 1, False, _same), ('vgg', 2, True, _pool2), ('vgg', 3, False, _same), ('vgg', 4, True, _pool2), ('vgg', 5, False, _same),
              ('vgg', 7, True, _pool2), ('vgg', 8, False, _same), ('vgg', 10, True, _pool2)]


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('oh,ow', [(1, 1), (7, 19), (5, 1)])
@pytest.mark.parametrize('net,layer,pool,size', GEOMETRIES, ids=[f'{g[0]}{g[1]}{"p" if g[2] else ""}' for g in GEOMETRIES])
def test_layer_gradients_are_exact_on_integers(dev, net, layer, pool, size, oh, ow, n):
    """Integer weights in [-2, 2], inputs and output gradients in [-3, 3]: every sum of the backward stays below 2^24 (asserted), so fp32 is exact
    and dx must equal float64 autograd bit for bit — which pins the ReLU rule at 0, the pooling's tie rule (integer inputs tie at positive values)
    and window order (alex's windows overlap) and the zeros of the dropped rows and columns."""
    w = _int_net(net)
    ci, co, k = R.TABLES[net][layer][:3]
    H, W = size(oh), size(ow)
    g = torch.Generator().manual_seed(7000 + 100 * layer + 10 * oh + ow + n)
    x = torch.randint(-3, 4, (n, H, W, ci), generator=g).float()
    dy = torch.randint(-3, 4, (n, oh, ow, co), generator=g).float()
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = R.layer_ref(net, layer, x64, w['W'][layer], w['b'][layer], pool)
    assert tuple(y.shape) == (n, co, oh, ow) and float(y.detach().max()) > 0 and float(y.detach().min()) == 0
    y.backward(dy.double().permute(0, 3, 1, 2))
    want = x64.grad.permute(0, 2, 3, 1)
    # every partial sum: |w| <= 2, |dz| <= 3, k k c_out terms per window position, at most four overlapping windows on one pooling input
    assert 4 * k * k * co * 2 * 3 < 2 ** 24 and float(want.abs().max()) < 2 ** 24 and float(y.detach().max()) < 2 ** 24 and float(want.abs().max()) > 0
    if pool:
        assert float(want[:, -1].abs().max()) == 0 and float(want[:, :, -1].abs().max()) == 0        # the dropped row and column
    lp = _lp(net, 'int')
    args = (layer, x.to(dev), y.detach().permute(0, 2, 3, 1).float().contiguous().to(dev), dy.to(dev))
    dx = lp.layer_bwd(*args, pool_first=pool)
    assert tuple(dx.shape) == (n, H, W, ci)
    assert torch.equal(dx.cpu().double(), want)
    if layer > 0:                                                       # the mask of the layer below, fused into the kernel that writes dx
        dx = lp.layer_bwd(*args, pool_first=pool, relu_in=True)
        assert torch.equal(dx.cpu().double(), want * (x > 0))


# ---- 2. tap backward ------------------------------------------------------------------------------------------------------------------------------
def _tap_ref(z, fg, lin, dtype):
    z = z.to(dtype).requires_grad_(True)
    f, fg = torch.relu(z), fg.to(dtype)
    na = f / (torch.sqrt((f ** 2).sum(-1, keepdim=True)) + R.dtype_eps(dtype))
    nb = fg / (torch.sqrt((fg ** 2).sum(-1, keepdim=True)) + R.dtype_eps(dtype))
    (lin.to(dtype) * (na - nb) ** 2).sum(-1).mean().backward()
    return z.grad


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('net,tap,C', [('alex', 0, 64), ('alex', 1, 192), ('vgg', 3, 512)])
def test_tap_backward_against_float64(dev, net, tap, C, n):
    """The gradient with respect to the pre-activations z (F = relu(z)) of mean over the n x 3 x 5 pixels of m.  Pixel 0 has an all-zero pred feature
    vector (float64 autograd with respect to F: NaN from sqrt'(0), which the closed ReLU behind it turns into 0; the kernel: finite and 0), pixel 1
    has pred == gt (exactly 0)."""
    g = torch.Generator().manual_seed(40 + 3 * tap + n)
    P = n * 15
    z = torch.randn(P, C, generator=g)
    fg = torch.relu(torch.randn(P, C, generator=g))
    z[0] = -z[0].abs() - 0.1
    fg[1] = torch.relu(z[1])
    lin = R.cached_net(net)['lin'][tap]
    g64, g32 = _tap_ref(z, fg, lin, torch.float64), _tap_ref(z, fg, lin, torch.float32)
    assert float(g64[:2].abs().max()) == 0 and bool(torch.isfinite(g64).all())
    d = _lp(net).tap_bwd(tap, torch.relu(z).to(dev), fg.to(dev)).cpu()
    assert float(d[0].abs().max()) == 0 and float(d[1].abs().max()) == 0
    e, e32 = rel(d[2:], g64[2:]), rel(g32[2:], g64[2:])
    print(f'\n[lpips tap bwd] {net} tap {tap} C {C} n {n}: error {e:.2e} (float32 CPU {e32:.2e})')
    assert e <= 4 * e32 + 2e-5, (e, e32)
    assert torch.equal(d == 0, (z <= 0) | (torch.arange(P)[:, None] == 1))                # the mask of the tap layer's own ReLU, nothing else


# ---- 3. the whole gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('net,H,W,seeds', L.CASES, ids=[f'{c[0]}-{c[1]}x{c[2]}' for c in L.CASES])
def test_gradient_against_float64_autograd(dev, net, H, W, seeds, B):
    pred, gt, m = L.case(net, H, W, L.batch_seeds(seeds, B))
    assert L.admissible(m), m                                               # on the CPU, before any device comparison
    for stride in (3, 4):
        v, d = _lp(net).loss(_place(pred, dev, stride), _place(gt, dev, 7 - stride))
        assert v.dtype == torch.float64 and v.dim() == 0 and d.dtype == torch.float32 and d.shape == (B, H, W, 3) and d.is_contiguous()
        e, ev = rel(d, m['g64']), abs(float(v) - m['v64']) / m['v64']
        print(f'\n[lpips loss] {net} {H}x{W} B {B} stride {stride}: value {float(v):.9g} (float64 {m["v64"]:.9g}, rel. error {ev:.2e}), gradient error {e:.2e} '
              f'(float32 CPU {m["e32"]:.2e}); margins ReLU {m["relu"]:.1f} pooling {m["pool"]:.1f}')
        assert e <= 4 * m['e32'] + 2e-5, (e, m['e32'])
        assert ev <= 4 * m['e32'] + 2e-5, (ev, m['e32'])


def test_gradient_without_normalize(dev):
    net, H, W, seeds = L.NO_NORMALIZE
    pred, gt, m = L.case(net, H, W, seeds, False)
    assert L.admissible(m), m
    v, d = _lp(net).loss(torch.as_tensor(pred[0], device=dev), torch.as_tensor(gt[0], device=dev), normalize=False)          # [H,W,3] in, [H,W,3] out
    assert d.shape == (H, W, 3)
    e, ev = rel(d, m['g64']), abs(float(v) - m['v64']) / m['v64']
    print(f'\n[lpips loss] {net} {H}x{W} normalize=False: value rel. error {ev:.2e}, gradient error {e:.2e} (float32 CPU {m["e32"]:.2e})')
    assert e <= 4 * m['e32'] + 2e-5 and ev <= 4 * m['e32'] + 2e-5
    _, dn = _lp(net).loss(torch.as_tensor(pred, device=dev), torch.as_tensor(gt, device=dev))
    assert not torch.equal(dn[0], d)


# ---- 4. the value against the metric --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W,seeds', [L.CASES[0], L.CASES[1], L.CASES[3], L.CASES[5]], ids=lambda v: str(v))
def test_value_has_the_bits_of_the_metric(dev, net, H, W, seeds):
    lp = _lp(net)
    pred, gt = (torch.as_tensor(t, device=dev) for t in L.make_batch(H, W, L.batch_seeds(seeds, 3)))
    singles = []
    for i in range(3):
        d, layers = lp(pred[i], gt[i], return_layers=True)
        v, _, vl = lp.loss(pred[i:i + 1], gt[i:i + 1], return_layers=True)
        assert torch.equal(v, d) and torch.equal(vl, layers) and float(d) > 0
        singles.append(float(d))
    v, _ = lp.loss(pred, gt)
    want = (singles[0] + singles[1] + singles[2]) / 3
    assert abs(float(v) - want) <= 1e-9 * want, (float(v), want)


# ---- 5. zero --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W', [('alex', 35, 47), ('vgg', 18, 31)])
def test_identical_patches_give_exactly_zero(dev, net, H, W):
    x = torch.as_tensor(L.make_batch(H, W, (0, 1))[0], device=dev)
    v, d = _lp(net).loss(x, x.clone())
    assert float(v) == 0.0 and torch.equal(d, torch.zeros_like(d))


# ---- 6. patch independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W', [('alex', 31, 39), ('vgg', 16, 16)])
def test_a_nan_stays_in_its_patch(dev, net, H, W):
    """A NaN in patch 1 of pred: the value and patch 1's gradient are NaN, patches 0 and 2 keep the clean run's bits.  Inside the patch the NaN
    spreads as in torch (a NaN activation passes its gradient, a pooling window gives its gradient to the NaN): through vgg's thirteen 3 x 3
    layers to every element at 16 x 16; behind alex's stride-4 first layer the float32 CPU restatement leaves 5 % of the elements finite (those
    whose every path runs through a closed ReLU), so there the test asks for the pixel itself and most of the patch."""
    pred, gt = (torch.as_tensor(t, device=dev) for t in L.make_batch(H, W, (0, 1, 2)))
    lp = _lp(net)
    v0, clean = lp.loss(pred, gt)
    bad = pred.clone()
    bad[1, H // 2, W // 2, 1] = float('nan')
    v, d = lp.loss(bad, gt)
    assert bool(torch.isfinite(v0)) and bool(torch.isfinite(clean).all())
    assert torch.equal(d[0], clean[0]) and torch.equal(d[2], clean[2])
    assert bool(torch.isnan(v)) and bool(torch.isnan(d[1, H // 2, W // 2]).all())
    assert float(torch.isnan(d[1]).float().mean()) > (0.9 if net == 'alex' else 0.999999)


# ---- 7. determinism -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W', [('alex', 47, 35), ('vgg', 33, 20)])
def test_results_are_bit_identical_across_calls_streams_and_graph_replays(dev, net, H, W):
    pred, gt = (_place(t, dev, 4) for t in L.make_batch(H, W, (0, 1, 2)))
    lp = _lp(net)
    v0, d0 = lp.loss(pred, gt)
    v1, d1 = lp.loss(pred, gt)
    assert torch.equal(v0, v1) and torch.equal(d0, d1) and float(d0.abs().max()) > 0
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    got = []
    for s in streams:
        with torch.cuda.stream(s):
            got.append(lp.loss(pred, gt))                              # separate workspaces: the cache is keyed by the stream
    torch.cuda.synchronize()
    assert all(torch.equal(v, v0) and torch.equal(d, d0) for v, d in got)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=streams[0]):
        cv, cd = lp.loss(pred, gt)
    for _ in range(2):
        cv.zero_(); cd.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cv, v0) and torch.equal(cd, d0)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_what_the_call_refuses_leaves_the_outputs_alone(dev):
    from pronerf_amd import _lib
    lib = _lib.load()
    x = torch.zeros(3 * 64 * 64 * 3, device=dev)
    out = torch.full((6,), 5.0, device=dev, dtype=torch.float64)
    d = torch.full((3 * 64 * 64 * 3,), 5.0, device=dev)
    ws = torch.zeros(1 << 25, device=dev)
    wb = ws.numel() * 4
    for net, lo in (('alex', 31), ('vgg', 16)):
        h = _lp(net)._h
        call = lambda B, H, W, sp=3, sg=3, pp=0, pg=0, p=x.data_ptr(), g=x.data_ptr(), o=out.data_ptr(), dp=d.data_ptr(), w=ws.data_ptr(), nb=wb: \
            lib.pnrf_lpips_loss_fwd(h, p, sp, pp, g, sg, pg, B, H, W, 1, o, dp, w, nb, None)
        for B, H, W in ((1, lo - 1, lo), (1, lo, lo - 1), (2, 4097, lo), (2, lo, 4097), (0, lo, lo), (-1, lo, lo), (1 << 20, 4096, 4096)):
            assert lib.pnrf_lpips_loss_workspace_bytes(h, B, H, W) == 0 and call(B, H, W) == -1, (net, B, H, W)
        nb = lib.pnrf_lpips_loss_workspace_bytes(h, 3, 40, 40)
        assert 0 < nb <= wb and lib.pnrf_lpips_loss_workspace_bytes(None, 3, 40, 40) == 0
        assert call(3, 40, 40, sp=2) == -1 and call(3, 40, 40, sg=2) == -1 and call(3, 40, 40, pp=-1) == -1
        for null in ('p', 'g', 'o', 'dp', 'w'):
            assert call(3, 40, 40, **{null: None}) == -1, null
        assert call(3, 40, 40, nb=nb - 1) == -1
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()) and bool((d == 5.0).all())
        assert call(3, 40, 40, nb=nb) == 0                                   # patch stride 0: one patch three times
        torch.cuda.synchronize()
        assert float(out[0]) == 0.0 and bool((d[:3 * 40 * 40 * 3] == 0).all()) and bool((d[3 * 40 * 40 * 3:] == 5.0).all())
        out.fill_(5.0); d.fill_(5.0)


# ---- 9. autograd.lpips ----------------------------------------------------------------------------------------------------------------------------
def test_autograd_lpips_is_the_kernel_gradient_times_the_incoming_one(dev):
    from pronerf_amd import autograd
    lp = _lp('vgg')
    pred, gt = (torch.as_tensor(t, device=dev) for t in L.make_batch(16, 16, (0, 1, 7)))
    v, d = lp.loss(pred, gt)
    p = pred.clone().requires_grad_(True)
    g = gt.clone().requires_grad_(True)
    s = autograd.lpips(p, g, lp)
    assert s.dtype == torch.float32 and s.dim() == 0 and torch.equal(s, v.float())
    (3 * s).backward()
    assert torch.equal(p.grad, 3 * d) and g.grad is None
    # the prediction as the trainer leaves it: the rgb columns of an [n, 4] map, read in place and reshaped by the loss
    rows = torch.zeros(3 * 256, 4, device=dev)
    rows[:, :3] = pred.reshape(-1, 3)
    rows.requires_grad_(True)
    view = rows[:, :3].reshape(3, 16, 16, 3)
    assert view.data_ptr() == rows.data_ptr()
    (3 * autograd.lpips(view, gt, lp)).backward()
    assert torch.equal(rows.grad[:, :3], 3 * d.reshape(-1, 3)) and float(rows.grad[:, 3].abs().max()) == 0


# ---- 10. the stage-2 driver's --a_p ---------------------------------------------------------------------------------------------------------------
def _driver_setup(tmp_path, H, W, n_rand):
    """test_custom_loss_gpu._driver_setup with the size of the views and N_rand as arguments (alex needs 32 x 32 patches)."""
    import llff_synth
    from oracle import synth
    root = llff_synth.make_dataset(str(tmp_path / 'scene'), seed=2, n=10, H=H, W=W, factor=4)
    sds = synth.state_dicts(synth.make_weights(0, 'trained'))
    pre = str(tmp_path / 'stage1.tar')
    torch.save({'global_step': 7, 'network_fn_state_dict': synth.nerfcls_state_dict(synth.make_nerfcls_weights(0, head_scale=0.3)),
                'mmr_network_fn_state_dict': sds['sampler'], 'refine_net_state_dict': sds['refine']}, pre)

    def cfg(exp):
        p = tmp_path / f'{exp}.txt'
        p.write_text(f'expname = {exp}\nbasedir = {tmp_path}/logs\ndatadir = {root}\npretrain_path = {pre}\nfactor = 4\nllffhold = 8\nN_rand = {n_rand}\nN_samples = 8\n'
                     'N_point_ray_enc = 48\nmmnetdepth = 6\nmmnetskips = [10000]\nnum_neighbor = 4\nuse_viewdirs = True\nraw_noise_std = 1e0\nlrate = 5e-4\n'
                     'weight_decay = 5e-8\ni_print = 1\ni_weights = 1000\n')
        return str(p)
    return cfg


@pytest.mark.parametrize('net,patch,H,W,n_rand', [('vgg', 16, 24, 32, 512), ('alex', 32, 40, 48, 2048)])
def test_driver_trains_with_the_perceptual_term(dev, tmp_path, monkeypatch, net, patch, H, W, n_rand):
    import test_custom_loss_gpu as CL
    from pronerf_amd import ops
    from pronerf_amd import run_S_eS_eN_alter_base_refine2 as s2
    from pronerf_amd._lib import PnrfError
    cfg = _driver_setup(tmp_path, H, W, n_rand)
    backbone, lin = R.state_dicts(net, R.cached_net(net))
    fb, fl = str(tmp_path / 'backbone.pth'), str(tmp_path / 'lin.pth')
    torch.save(backbone, fb); torch.save(lin, fl)
    weights = ['--lpips_net', net, '--lpips_backbone', fb, '--lpips_lin', fl]
    calls = []
    loss = ops.Lpips.loss

    def spy(self, pred, gt, normalize=True, **kw):
        out = loss(self, pred, gt, normalize=normalize, **kw)
        calls.append((pred.detach().clone(), gt.clone(), out[0].clone(), normalize))
        return out
    monkeypatch.setattr(ops.Lpips, 'loss', spy)
    CL._seed()
    tr, log = s2.train(['--config', cfg('perceptual'), '--max_steps', '3', '--device_batches', 'all', '--a_p', '0.1'] + weights, device=dev, patch_size=patch)
    assert len(calls) == 3 and [e[0] for e in log] == [1, 2, 3] and all(np.isfinite(e[1]) and np.isfinite(e[2]) for e in log)
    assert all(bool(torch.isfinite(t).all()) for i in range(26) for t in tr.read('param', i))
    pred, gt, value, normalize = calls[0]
    assert tuple(pred.shape) == (n_rand // patch ** 2, patch, patch, 3) and pred.shape == gt.shape and normalize and float(value) > 0
    want = float(((pred - gt) ** 2).mean()) + 0.1 * float(value)
    assert abs(log[0][1] - want) <= 4 * 2.0 ** -23 * want, (log[0][1], want)             # the sum and the product in fp32: a few roundings
    # what the perceptual term needs, said before any iteration
    n_calls = len(calls)
    base = ['--config', cfg('refused'), '--max_steps', '1', '--device_batches', 'all', '--a_p', '0.1']
    with pytest.raises(PnrfError, match='patch_size'):
        s2.train(base + weights, device=dev)
    with pytest.raises(PnrfError, match='patch_size'):
        s2.train(base + weights, device=dev, patch_size=8)
    with pytest.raises(PnrfError, match='lpips_backbone'):
        s2.train(base + ['--lpips_net', net], device=dev, patch_size=patch)
    with pytest.raises(PnrfError, match='lpips_lin'):
        s2.train(base + ['--lpips_net', net, '--lpips_backbone', fb, '--lpips_lin', str(tmp_path / 'nothing.pth')], device=dev, patch_size=patch)
    with pytest.raises(PnrfError, match='lpips_net'):
        s2.train(base + ['--lpips_net', 'squeeze', '--lpips_backbone', fb, '--lpips_lin', fl], device=dev, patch_size=patch)
    assert len(calls) == n_calls
