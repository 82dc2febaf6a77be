"""GPU: LPIPS on the device — pnrf_lpips_layer_fwd and pnrf_lpips_fwd through ops.Lpips, the reference-named rgb_lpips and render_path's pnrf_lpips.

The convolution kernel works on tiles of 64 output pixels (of both images together) x 64 channels, 32 channels of one filter tap per step, so the
layer shapes are: output 1 x 1 (two pixels: one partial tile), 7 x 19 (266 pixels: four full tiles and a partial one, an odd width) and 5 x 1.

Bound of every comparison with the float64 restatement (tests/lpips_ref.py), per case: what the SAME formulas cost in float32 on the CPU is
e32; the kernels may err 4 e32 + 2e-5 (relative L2 error of each m_k plane, relative error of d) — their sums run in another order.

Measured on the MI355X: relative error of d 8e-9 .. 1.2e-7 (e32 2.5e-9 .. 6.6e-7) and worst plane 7e-7 .. 1.1e-5 (e32 5e-7 .. 2.9e-5) on every
case but 'flat' (two images 1e-3 apart, d = 1.8e-7): d 2.2e-6 (e32 5.6e-6), worst plane 1.2e-4 (e32 2.9e-4).  The table is in DESIGN §4.8.1."""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _weights(net, kind):
    return R.make_int_net(net) if kind == 'int' else R.cached_net(net, 4096.0 if kind == 'big' else 1.0)


_handles = {}


def _lp(net, kind='seeded'):
    """One ops.Lpips per (net, weights), built through the loader from torchvision-style state dicts."""
    from pronerf_amd import ops
    if (net, kind) not in _handles:
        _handles[net, kind] = ops.Lpips(net, *R.state_dicts(net, _weights(net, kind)))
    return _handles[net, kind]


# ---- 5. exact layers ------------------------------------------------------------------------------------------------------------------------------
# (net, layer, pool in front, input size for an output of n pixels along one axis)
GEOMETRIES = [('alex', 0, False, lambda n: 4 * (n - 1) + 7), ('alex', 1, True, lambda n: 2 * (n - 1) + 3), ('alex', 2, True, lambda n: 2 * (n - 1) + 3),
              ('vgg', 0, False, lambda n: n), ('vgg', 2, True, lambda n: 2 * n + (n > 1)), ('vgg', 12, False, lambda n: n)]


@pytest.mark.parametrize('oh,ow', [(1, 1), (7, 19), (5, 1)])
@pytest.mark.parametrize('net,layer,pool,size', GEOMETRIES, ids=[f'{g[0]}{g[1]}' for g in GEOMETRIES])
def test_layers_are_exact_on_integers(dev, net, layer, pool, size, oh, ow):
    """Integer weights in [-2, 2], biases in [-8, 8], inputs in [-3, 3]: every partial sum is below 2^15, so fp32 products and sums are exact and the
    layer must equal the float64 CPU layer bit for bit."""
    w = _weights(net, 'int')
    ci, co = R.TABLES[net][layer][:2]
    H, W = size(oh), size(ow)
    g = torch.Generator().manual_seed(1000 * layer + 10 * oh + ow)
    x = torch.randint(-3, 4, (2, H, W, ci), generator=g).float()
    want = R.layer_ref(net, layer, x.permute(0, 3, 1, 2), w['W'][layer], w['b'][layer], pool)
    assert tuple(want.shape) == (2, co, oh, ow) and float(want.abs().max()) < 2 ** 15 and float(want.max()) > 0
    y = _lp(net, 'int').layer(layer, x.to(dev), pool_first=pool)
    assert tuple(y.shape) == (2, oh, ow, co)
    assert torch.equal(y.cpu().double().permute(0, 3, 1, 2), want)


# ---- 6., 7. the metric against float64 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(net, kind, H, W, normalize=True, weights='seeded'):
    """(a, b, d64, maps64, e32 of d, [e32 of each plane]) — computed once per case, shared, never written to."""
    a, b = R.make_pair(kind, H, W)
    w = _weights(net, weights)
    d64, m64 = R.lpips_ref(net, w, a, b, normalize)
    d32, m32 = R.lpips_ref(net, w, a, b, normalize, dtype=torch.float32)
    e_maps = [float((x.double() - y).norm() / y.norm()) for x, y in zip(m32, m64)]
    return a, b, d64, m64, abs(d32 - d64) / abs(d64), e_maps


def _check(dev, net, kind, H, W, normalize=True, weights='seeded', stride_a=3):
    a, b, d64, m64, e_d, e_maps = _case(net, kind, H, W, normalize, weights)
    ta, tb = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    if stride_a == 4:                                                   # a in the rgb columns of [n, 4] rows, as the renderer leaves a frame
        rgbd = torch.full((H * W, 4), 7.0, device=dev)
        rgbd[:, :3] = ta.reshape(-1, 3)
        ta = rgbd[:, :3].reshape(H, W, 3)
        assert ta.data_ptr() == rgbd.data_ptr() and ta.stride() == (4 * W, 4, 1)
    d, layers, maps = _lp(net, weights)(ta, tb, normalize=normalize, return_layers=True, return_maps=True)
    assert d.dtype == torch.float64 and d.dim() == 0 and d.is_cuda and layers.shape == (5,)
    assert [tuple(m.shape) for m in maps] == R.tap_dims(net, H, W)
    got_d, got = float(d), [m.cpu().double() for m in maps]
    errs = [float((x - y).norm() / y.norm()) for x, y in zip(got, m64)]
    err_d = abs(got_d - d64) / abs(d64)
    print(f'lpips {net} {kind} {H}x{W} normalize={normalize} weights={weights}: d {got_d:.9g} (float64 {d64:.9g}) rel. error {err_d:.2e} (float32 CPU {e_d:.2e}); '
          f'planes {" ".join(f"{e:.2e}" for e in errs)} (float32 CPU {" ".join(f"{e:.2e}" for e in e_maps)})')
    assert abs(float(layers.sum()) - got_d) <= 1e-14 * max(1.0, abs(got_d))
    for k in range(5):
        assert abs(float(layers[k]) - float(got[k].mean())) <= 1e-12 * max(1e-30, abs(float(got[k].mean())))
        assert errs[k] <= 4 * e_maps[k] + 2e-5, (k, errs[k], e_maps[k])
    assert err_d <= 4 * e_d + 2e-5, (err_d, e_d)


CASES = [('alex', 'noise', 31, 31), ('alex', 'smooth', 31, 39), ('alex', 'mix', 64, 80), ('vgg', 'anti', 16, 16), ('vgg', 'flat', 17, 23), ('vgg', 'mix', 48, 40)]


@pytest.mark.parametrize('net,kind,H,W', CASES)
def test_metric_against_float64(dev, net, kind, H, W):
    _check(dev, net, kind, H, W)


def test_metric_with_a_pixel_stride_of_four_and_without_normalize(dev):
    _check(dev, 'alex', 'mix', 31, 39, stride_a=4)
    _check(dev, 'vgg', 'noise', 17, 23, normalize=False)


@pytest.mark.parametrize('net,H,W', [('alex', 31, 39), ('vgg', 17, 23)])
def test_metric_with_large_activations(dev, net, H, W):
    """Layer 0's weights and bias x 4096: activations of thousands behind the first layer; the same bound."""
    _check(dev, net, 'mix', H, W, weights='big')


# ---- 8., 9. identity, symmetry, determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W', [('alex', 35, 47), ('vgg', 18, 31)])
def test_identity_is_exactly_zero_and_the_metric_is_symmetric_to_the_bit(dev, net, H, W):
    a, b = (torch.tensor(t, device=dev) for t in R.make_pair('mix', H, W))
    lp = _lp(net)
    d, layers, maps = lp(a, a.clone(), return_layers=True, return_maps=True)
    assert float(d) == 0.0 and float(layers.abs().max()) == 0.0 and all(float(m.abs().max()) == 0.0 for m in maps)
    (d1, l1, m1), (d2, l2, m2) = lp(a, b, return_layers=True, return_maps=True), lp(b, a, return_layers=True, return_maps=True)
    assert float(d1) > 0 and torch.equal(d1, d2) and torch.equal(l1, l2) and all(torch.equal(x, y) for x, y in zip(m1, m2))


@pytest.mark.parametrize('net,H,W', [('alex', 64, 80), ('vgg', 48, 40)])
def test_results_are_bit_identical_across_calls_streams_and_graph_replays(dev, net, H, W):
    a, b = (torch.tensor(t, device=dev) for t in R.make_pair('noise', H, W))
    lp = _lp(net)
    run = lambda: lp(a, b, return_layers=True, return_maps=True)
    flat = lambda r: torch.cat([r[0].reshape(1).view(torch.int64), r[1].view(torch.int64)] + [m.reshape(-1).view(torch.int32).long() for m in r[2]])
    first = flat(run())
    assert torch.equal(first, flat(run()))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        second = flat(run())                                            # its own workspace: the cache is keyed by the stream
    s.synchronize()
    assert torch.equal(first, second)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    for _ in range(2):
        captured[0].zero_(); captured[1].zero_()
        for m in captured[2]:
            m.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(first, flat(captured))


def test_workspace_size_is_zero_exactly_where_the_call_refuses(dev):
    """With a handle: pnrf_lpips_workspace_bytes == 0 <=> pnrf_lpips_fwd returns PNRF_E_ARG for the size (checked before any launch)."""
    from pronerf_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64 * 64 * 3, device=dev)
    out = torch.zeros(6, device=dev, dtype=torch.float64)
    ws = torch.zeros(1 << 22, device=dev)
    for net, lo in (('alex', 31), ('vgg', 16)):
        h = _lp(net)._h
        for H, W in ((lo, lo), (lo - 1, lo), (lo, lo - 1), (lo + 1, lo), (0, lo), (lo, 4097), (4097, lo)):
            nb = lib.pnrf_lpips_workspace_bytes(h, H, W)
            rc = lib.pnrf_lpips_fwd(h, x.data_ptr(), 3, x.data_ptr(), 3, H, W, 1, out.data_ptr(), None, ws.data_ptr(), ws.numel() * 4, None)
            assert (nb == 0) == (rc == -1) and (nb > 0) == (H >= lo and W >= lo and H <= 4096 and W <= 4096), (net, H, W, nb, rc)
        nb = lib.pnrf_lpips_workspace_bytes(h, 40, 40)
        assert lib.pnrf_lpips_fwd(h, x.data_ptr(), 3, x.data_ptr(), 3, 40, 40, 1, out.data_ptr(), None, ws.data_ptr(), nb - 1, None) == -1
        assert lib.pnrf_lpips_fwd(h, x.data_ptr(), 2, x.data_ptr(), 3, 40, 40, 1, out.data_ptr(), None, ws.data_ptr(), nb, None) == -1
    torch.cuda.synchronize()


# ---- 10. the reference's names and render_path ----------------------------------------------------------------------------------------------------
def test_rgb_lpips_by_its_reference_name(dev):
    from pronerf_amd import run_nerf_helpers as h
    a, b = R.make_pair('mix', 35, 47)
    h.__LPIPS__.clear()
    h.LPIPS_WEIGHTS['alex'] = R.state_dicts('alex', _weights('alex', 'seeded'))
    try:
        v = h.rgb_lpips(a, b, 'alex', dev)
        v0 = h.rgb_lpips(a, b, 'alex', dev, normalize=False)
    finally:
        h.__LPIPS__.clear(); h.LPIPS_WEIGHTS.clear()
    lp = _lp('alex')
    assert isinstance(v, float) and v == float(lp(torch.tensor(a, device=dev), torch.tensor(b, device=dev))) and v > 0
    assert v0 == float(lp(torch.tensor(a, device=dev), torch.tensor(b, device=dev), normalize=False)) != v


def test_render_path_takes_lpips_of_every_pose(dev):
    from types import SimpleNamespace

    from oracle import synth
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    args = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256, mmnetskips=[10000],
                           N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)
    kw, _ = trt.create_nerf(args, device=dev)
    sd = synth.state_dicts(synth.make_weights(0, 'trained'))
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    H, W = 32, 40
    scene = synth.make_scene(0, H=H, W=W, n_views=6)
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
    lp = _lp('alex')
    kw['pnrf_lpips'] = lp
    targets = [scene['c2w'], scene['poses'][0]]
    gt = [scene['images'][0], np.random.RandomState(1).uniform(0, 1, (H, W, 3)).astype(np.float32)]
    out = trt.render_path(targets, (H, W, scene['focal']), scene['K'], None, kw, gt_imgs=gt, savedir=None, n_timing_reps=1, verbose=False)
    assert len(kw['lpips']) == 2 and all(isinstance(v, float) and v > 0 for v in kw['lpips'])
    for i in range(2):
        assert kw['lpips'][i] == float(lp(torch.tensor(gt[i], device=dev), torch.tensor(out[1][i], device=dev)))
    without = {k: v for k, v in kw.items() if k not in ('pnrf_lpips', 'lpips')}
    trt.render_path(targets[:1], (H, W, scene['focal']), scene['K'], None, without, gt_imgs=gt[:1], savedir=None, n_timing_reps=1, verbose=False)
    assert 'lpips' not in without
