"""GPU: the frame tail on the device — pnrf_image_metrics_fwd (img2mse + img2ssim) and pnrf_frame_to8b_fwd — through ops, the reference-named
img2ssim and render_path's two opt-in switches.

The SSIM kernel works on 32 x 32 output tiles (TILE below; one workgroup per tile and channel), so with the 11-tap filter the shapes are:
11 x 11 (one window), 12 x 17, 43 x 75 (33 x 65 windows: one more than a tile / two tiles), 75 x 107 (65 x 97 windows: one more than two /
three tiles, more than one workgroup in both directions); with 7 and 8 taps 43 x 75 gives 37 x 69 and 36 x 68 windows.

Bound of every SSIM comparison, per case: the error of the SAME formulas evaluated in fp32 numpy (tests/ssim_ref.py with dtype float32)
against their float64 value is what straightforward single precision costs; the kernel may err twice that (its sums run in another
order), with floors of 1e-6 on the mean and 1e-5 on the map."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ssim_ref
from oracle import pronerf_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu

TILE = 32
SHAPES = [(11, 11), (12, 17), (43, 75), (2 * TILE + 11, 3 * TILE + 11)]
to8b_np = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssim_cases.npz')))


@functools.lru_cache(maxsize=None)
def _case(kind, H, W, T=11):
    """(a, b, float64 mean, float64 map, bound on the mean, bound on the map) — computed once per case, shared, never written to."""
    key = f'{kind}_{H}x{W}'
    a, b = (_golden()[key + '_a'], _golden()[key + '_b']) if key + '_a' in _golden() else ssim_ref.make_pair(kind, H, W)
    m64 = ssim_ref.img2ssim_ref(a, b, filter_size=T, return_map=True)
    m32 = ssim_ref.img2ssim_ref(a, b, filter_size=T, return_map=True, dtype=np.float32)
    e_mean, e_map = abs(float(m32.mean(dtype=np.float64)) - float(m64.mean())), float(np.abs(m32 - m64).max())
    return a, b, float(m64.mean()), m64, max(2 * e_mean, 1e-6), max(2 * e_map, 1e-5)


def _run(dev, a, b, T=11, stride_a=3):
    """ops.image_metrics on device copies of a, b; stride_a = 4 places a in the rgb columns of an [n, 4] tensor, as the renderer leaves it."""
    from pronerf_amd import ops
    H, W = a.shape[:2]
    ta, tb = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    if stride_a == 4:
        rgbd = torch.full((H * W, 4), 7.0, device=dev)
        rgbd[:, :3] = ta.reshape(-1, 3)
        ta = rgbd[:, :3].reshape(H, W, 3)
        assert ta.data_ptr() == rgbd.data_ptr() and ta.stride() == (4 * W, 4, 1)
    out, smap = ops.image_metrics(ta, tb, filter_size=T, return_map=True)
    assert out.dtype == torch.float64 and out.shape == (4,) and smap.shape == (H - T + 1, W - T + 1, 3)
    return out.cpu().numpy(), smap.cpu().numpy()


@pytest.mark.parametrize('kind', ssim_ref.KINDS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_ssim_against_the_float64_restatement(dev, H, W, kind):
    a, b, mean64, map64, tol_mean, tol_map = _case(kind, H, W)
    out4, map4 = _run(dev, a, b, stride_a=4)
    out3, map3 = _run(dev, a, b, stride_a=3)
    assert out4.tobytes() == out3.tobytes() and map4.tobytes() == map3.tobytes()          # the pixel stride changes no bit
    n_win = (H - 10) * (W - 10) * 3
    assert out3[3] == out3[2] / n_win and abs(out3[2] - map3.astype(np.float64).sum()) <= 1e-12 * n_win
    e_mean, e_map = abs(out3[3] - mean64), float(np.abs(map3 - map64).max())
    print(f'\n[ssim] {kind} {H}x{W}: ssim {out3[3]:.9f}; kernel error mean {e_mean:.2e} (bound {tol_mean:.2e}), map {e_map:.2e} (bound {tol_map:.2e})')
    assert e_mean <= tol_mean and e_map <= tol_map
    key = f'{kind}_{H}x{W}'
    if key + '_ssim' in _golden():                                                        # the reference's own numbers, same bound
        assert abs(out3[3] - float(_golden()[key + '_ssim'])) <= tol_mean
        if key + '_map' in _golden():
            assert np.abs(map3 - _golden()[key + '_map']).max() <= tol_map


@pytest.mark.parametrize('T', [7, 8])
def test_ssim_other_filter_sizes(dev, T):
    for kind in ssim_ref.KINDS:
        a, b, mean64, map64, tol_mean, tol_map = _case(kind, 43, 75, T)
        out, smap = _run(dev, a, b, T=T)
        e_mean, e_map = abs(out[3] - mean64), float(np.abs(smap - map64).max())
        print(f'\n[ssim] {kind} 43x75 T={T}: kernel error mean {e_mean:.2e} (bound {tol_mean:.2e}), map {e_map:.2e} (bound {tol_map:.2e})')
        assert e_mean <= tol_mean and e_map <= tol_map
    assert abs(_run(dev, *_case('noise', 43, 75, T)[:2], T=T)[0][3] - float(_golden()[f'ssim_noise_43x75_T{T}'])) <= _case('noise', 43, 75, T)[4]


@pytest.mark.parametrize('H,W', SHAPES)
def test_sse_mse_and_psnr(dev, H, W):
    from pronerf_amd import run_nerf_helpers as h
    for kind in ssim_ref.KINDS:
        a, b = _case(kind, H, W)[:2]
        out, _ = _run(dev, a, b, stride_a=4)
        ta, tb = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
        sse = float(((ta - tb).double() ** 2).sum())
        assert abs(out[0] - sse) <= 1e-6 * sse and abs(out[1] - sse / (H * W * 3)) <= 1e-6 * sse / (H * W * 3)
        psnr = float(h.mse2psnr(h.img2mse(ta, tb)))
        assert abs(-10 * np.log10(out[1]) - psnr) <= 1e-4, (kind, -10 * np.log10(out[1]), psnr)


def test_img2ssim_by_its_reference_name(dev):
    from pronerf_amd import run_nerf_helpers as h
    a, b, mean64, map64, tol_mean, tol_map = _case('smooth', 43, 75)
    s = h.img2ssim(a, b)
    assert isinstance(s, float) and abs(s - mean64) <= tol_mean
    m = h.img2ssim(a, b, return_map=True)
    assert isinstance(m, np.ndarray) and m.shape == (33, 65, 3) and np.abs(m - map64).max() <= tol_map
    mt = h.img2ssim(torch.tensor(a, device=dev), torch.tensor(b), return_map=True)          # tensors in (one of them on the host): tensor out
    assert isinstance(mt, torch.Tensor) and mt.is_cuda and np.array_equal(mt.cpu().numpy(), m)
    assert h.img2ssim(a, b, filter_size=8, k1=0.02) != s
    with pytest.raises(AssertionError):
        h.img2ssim(a, b[:, :, :2])


def test_metrics_are_deterministic_across_streams_and_graph_replays(dev):
    from pronerf_amd import ops
    a, b = _case('noise', *SHAPES[3])[:2]
    ta, tb = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    out0, map0 = ops.image_metrics(ta, tb, return_map=True)
    torch.cuda.synchronize()
    want = (out0.cpu().numpy().tobytes(), map0.cpu().numpy().tobytes())
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    got = []
    for i in range(20):
        with torch.cuda.stream(streams[i % 2]):
            got.append(ops.image_metrics(ta, tb, return_map=True))
    torch.cuda.synchronize()
    for o, m in got:
        assert (o.cpu().numpy().tobytes(), m.cpu().numpy().tobytes()) == want
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, mg = ops.image_metrics(ta, tb, return_map=True)
    for _ in range(3):
        og.zero_(); mg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert (og.cpu().numpy().tobytes(), mg.cpu().numpy().tobytes()) == want


def _to8b_inputs(n):
    """rgb [n,3]: every k / 255 with its two fp32 neighbours and the values outside [0, 1], repeated from a rotating start; depth [n]: 1000 random
    positive values repeated, the largest of the plane neither first nor last (n >= 3)."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    special = np.concatenate([np.array([-0.0, -1e-3, 1.0, np.nextafter(np.float32(1), np.float32(2)), 7.5, 1e30], np.float32),
                              k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))]).astype(np.float32)
    rgb = np.resize(np.roll(special, -(n % 5)), (n, 3)).astype(np.float32)
    d = np.resize(np.random.RandomState(5).uniform(0.05, 9.0, 1000).astype(np.float32), n).copy()
    if n >= 3:
        d[n // 2] = np.float32(9.5)
        assert 0 < int(np.argmax(d)) < n - 1
    return special, rgb, d


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000, 1024 * 256 + 3])       # the maximum's first kernel runs at most 1024 workgroups of 256: the last n is past that grid
def test_frame_to8b_is_numpy_bit_for_bit(dev, n):
    from pronerf_amd import ops
    special, rgb, d = _to8b_inputs(n)
    if n * 3 >= special.size:
        assert set(special.tolist()) <= set(rgb.reshape(-1).tolist())
    want_rgb, want_d = to8b_np(rgb), to8b_np(d / np.max(d))
    rgbd = torch.from_numpy(np.concatenate([rgb, d[:, None]], 1)).to(dev)
    r8, d8 = ops.frame_to8b(rgbd=rgbd)                                         # the renderer's rows: strides 4
    assert r8.dtype == torch.uint8 and r8.shape == (n, 3) and d8.shape == (n,)
    assert np.array_equal(r8.cpu().numpy(), want_rgb) and np.array_equal(d8.cpu().numpy(), want_d)
    r8, none = ops.frame_to8b(rgb=torch.from_numpy(rgb).to(dev))               # each output NULL in turn, contiguous inputs
    assert none is None and np.array_equal(r8.cpu().numpy(), want_rgb)
    none, d8 = ops.frame_to8b(depth=torch.from_numpy(d).to(dev))
    assert none is None and np.array_equal(d8.cpu().numpy(), want_d)


def test_frame_to8b_not_finite_input(dev):
    """Documented in include/pronerf_hip.h: NaN -> 0, +Inf -> 255, -Inf -> 0; the maximum skips NaN depths."""
    from pronerf_amd import ops
    _, rgb, d = _to8b_inputs(1000)
    rgb[3, 1], rgb[500, 0], rgb[999, 2] = np.nan, np.inf, -np.inf
    d[7] = np.nan
    r8, d8 = ops.frame_to8b(rgb=torch.from_numpy(rgb).to(dev), depth=torch.from_numpy(d).to(dev))
    torch.cuda.synchronize()
    want = to8b_np(np.nan_to_num(rgb, nan=0.0, posinf=2.0, neginf=-1.0))
    assert np.array_equal(r8.cpu().numpy(), want) and want[3, 1] == 0 and want[500, 0] == 255 and want[999, 2] == 0
    wd = to8b_np(np.nan_to_num(d / np.nanmax(d), nan=0.0))
    assert np.array_equal(d8.cpu().numpy(), wd) and wd[7] == 0


def _args():
    return SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256,
                           mmnetskips=[10000], N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)


def test_render_path_with_the_frame_tail_on_the_device(dev, tmp_path):
    """render_path on the small synthetic data set of tests/test_mirror_gpu.py, default against pnrf_metrics + pnrf_device_to8b."""
    from pronerf_amd import run_nerf_helpers as h
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    kw, _ = trt.create_nerf(_args(), device=dev)
    sd = synth.state_dicts(synth.make_weights(0, 'trained'))
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    scene = synth.make_scene(0, H=24, W=32, n_views=6)
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
    targets = [scene['c2w'], scene['poses'][0]]
    fr = orc.frame_setup({**scene, 'c2w': scene['c2w']}, num_neighbor=4)
    ref = orc.render_rays_infer(synth.make_weights(0, 'trained'), fr['rays'], fr['or_rays'], fr['images'], fr['proj'])
    gt = [ref['rgb'].reshape(24, 32, 3).numpy(), np.random.RandomState(1).uniform(0, 1, (24, 32, 3)).astype(np.float32)]
    runs = {}
    for name, opts in (('host', {}), ('device', {'pnrf_metrics': True, 'pnrf_device_to8b': True})):
        k = {**kw, **opts}
        out = trt.render_path(targets, (24, 32, scene['focal']), scene['K'], None, k, gt_imgs=gt, savedir=str(tmp_path / name), n_timing_reps=1, verbose=False)
        runs[name] = (out, k)
    (o0, k0), (o1, k1) = runs['host'], runs['device']
    for x, y in zip(o0, o1):
        assert x.dtype == np.float32 and x.tobytes() == y.tobytes()
    assert 'ssims' not in k0 and len(k1['ssims']) == len(k1['psnrs']) == 2
    assert max(abs(p - q) for p, q in zip(k0['psnrs'], k1['psnrs'])) <= 1e-4
    for i in range(2):
        assert k1['ssims'][i] == h.img2ssim(o1[1][i], gt[i])
    assert all(-1 <= v <= 1 for v in k1['ssims']) and k1['ssims'][0] > k1['ssims'][1]       # the oracle's frame of the same pose / noise
    files = sorted(os.listdir(tmp_path / 'host'))
    assert files == sorted(os.listdir(tmp_path / 'device')) == ['000.png', '001.png', 'depth_000.png', 'depth_001.png']
    for f in files:
        assert (tmp_path / 'host' / f).read_bytes() == (tmp_path / 'device' / f).read_bytes(), f
