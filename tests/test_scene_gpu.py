"""GPU: the device-resident scene (pnrf_scene_*, pnrf_frame_rays_dev_fwd, pnrf_render_pose_fwd; ops.Scene, Renderer.set_scene / render_pose /
capture_pose, render_path's pnrf_scene_cache).  Everything a target pose needs is derived on the device from its twelve floats and must equal what
the host path computes: neighbour indices and texels bit for bit, rays bit for bit, projection matrices bit for bit against the float64
restatement of tests/scene_ref.py (and within the derived bound of the host's fp32 matmul), the rendered rows bit for bit against
``render_rays`` fed with the same intermediates — and the frame within the project's bar of the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import pronerf_oracle as orc
from oracle import synth
from scene_ref import proj_exact_and_bound, proj_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rand_poses(rs, nv, sig=1.0):
    poses = np.tile(np.eye(3, 4, dtype=np.float32), (nv, 1, 1))
    poses[:, :, 3] = (rs.randn(nv, 3) * sig).astype(np.float32)
    return poses


# ---------------------------------------------------------------------------------------------- 1. ingest + gather
@pytest.mark.parametrize('source', ['f32_stride3', 'f32_stride4', 'u8_to_f32', 'u8_to_u8'])
@pytest.mark.parametrize('size', [(1, 1), (5, 7), (24, 32)])
def test_ingest_and_gather_equal_images_pack_of_the_selected_views(dev, size, source):
    from pronerf_amd import ops
    from pronerf_amd.render import select_neighbors
    Hf, Wf = size
    rs = np.random.RandomState(Hf * 100 + Wf)
    for nv, nb in ((6, 1), (6, 4), (8, 8)):
        poses = _rand_poses(rs, nv)
        c2w = _rand_poses(rs, 1)[0]
        if source.startswith('u8'):
            src = np.stack([((np.arange(Hf * Wf * 3) * 37 + 11 * v) % 256).astype(np.uint8).reshape(Hf, Wf, 3) for v in range(nv)])
            want_imgs = (src / 255.).astype(np.float32)                    # load_llff.py: the floats an 8-bit image is loaded as
            given = src
        else:
            want_imgs = rs.rand(nv, Hf, Wf, 3).astype(np.float32)
            want_imgs.reshape(-1)[:4] = [0.0, 1.0, np.float32(1e-42), -0.0]          # end points, a subnormal, a signed zero: a copy keeps them
            given = want_imgs if source == 'f32_stride3' else np.concatenate([want_imgs, rs.rand(nv, Hf, Wf, 1).astype(np.float32) + 5], -1)
        scene = ops.Scene.from_views(poses, given, np.eye(3, dtype=np.float32), cache='u8' if source == 'u8_to_u8' else 'f32', device=dev)
        ref_nos, proj, img4 = scene.select(torch.from_numpy(c2w).to(dev), nb)
        want_ref = select_neighbors(c2w, poses, nb)
        np.testing.assert_array_equal(ref_nos.cpu().numpy(), want_ref)
        sel = want_imgs[want_ref]
        if source.startswith('u8') and Hf * Wf * 3 >= 256:
            assert len(np.unique(src[want_ref])) == 256                     # every byte value went through the expansion
        want = ops.images_pack(torch.from_numpy(sel).permute(0, 3, 1, 2).contiguous().to(dev))
        assert img4.shape == (nb, Hf, Wf, 4) and torch.equal(_bits(img4), _bits(want))
        assert bool((_bits(img4)[..., 3] == 0).all())                       # w == +0.0
    with pytest.raises(ops.PnrfError):                                       # fp32 pixels are never quantised into an RGBA8 cache
        ops.Scene.from_views(poses, rs.rand(nv, Hf, Wf, 3).astype(np.float32), np.eye(3, dtype=np.float32), cache='u8', device=dev)


# ---------------------------------------------------------------------------------------------- 2. selection
def _dyadic_scene(nv, rs):
    """Camera centres on the grid of multiples of 0.25 in [-8, 8]: every difference, square and sum of the distance is exact in fp32, so equal
    distances are EXACT ties.  From three views on: view 1 and view 2 mirrored about the target (tie: the lower index first), the last view at the
    target itself (distance 0)."""
    grid = lambda n: (rs.randint(-32, 33, (n, 3)) * 0.25).astype(np.float32)
    target = np.array([0.5, -1.25, 2.0], np.float32)
    t = grid(nv)
    if nv >= 3:
        off = np.array([0.75, -0.5, 0.25], np.float32)
        t[1], t[2], t[nv - 1] = target - off, target + off, target
    poses = np.tile(np.eye(3, 4, dtype=np.float32), (nv, 1, 1))
    poses[:, :, 3] = t
    c2w = np.eye(3, 4, dtype=np.float32)
    c2w[:, 3] = target
    return c2w, poses


@pytest.mark.parametrize('nv', [1, 4, 6, 20, 300])
def test_selection_equals_select_neighbors_index_for_index(dev, nv):
    from pronerf_amd import ops
    from pronerf_amd.render import select_neighbors
    cases = [_dyadic_scene(nv, np.random.RandomState(nv))]
    for seed in range(4):
        s = synth.make_scene(seed, H=2, W=2, n_views=nv)
        cases.append((s['c2w'], s['poses']))
    imgs = np.zeros((nv, 2, 2, 3), np.uint8)
    for i, (c2w, poses) in enumerate(cases):
        scene = ops.Scene.from_views(poses, imgs, np.eye(3, dtype=np.float32), cache='u8', device=dev)
        for nb in sorted({1, min(4, nv), min(8, nv)}):
            ref_nos, _, _ = scene.select(torch.from_numpy(np.ascontiguousarray(c2w[:3, :4])).to(dev), nb)
            assert ref_nos.dtype == torch.int32
            want = select_neighbors(c2w, poses, nb)
            np.testing.assert_array_equal(ref_nos.cpu().numpy(), want, err_msg=f'case {i}, nb {nb}')
        if i == 0 and nv >= 4:
            got = ref_nos.cpu().numpy().tolist()
            assert got[0] == nv - 1 and got.index(1) + 1 == got.index(2)          # the view at the target first; the mirrored pair in index order
    if nv >= 4:                                                                  # a target that is not finite: every distance NaN, ranked by index
        bad = np.full((3, 4), np.nan, np.float32)
        ref_nos, _, _ = scene.select(torch.from_numpy(bad).to(dev), 4)
        np.testing.assert_array_equal(ref_nos.cpu().numpy(), select_neighbors(bad, poses, 4))
        with pytest.raises(ops.PnrfError):
            scene.select(torch.from_numpy(bad).to(dev), nv + 1 if nv < 8 else 9)


# ---------------------------------------------------------------------------------------------- 3. projection
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_projection_matrices_equal_the_float64_restatement(dev, seed):
    from pronerf_amd import ops
    from pronerf_amd.render import projection_matrices, select_neighbors
    s = synth.make_scene(seed, H=2, W=2, n_views=6, rotate=True, sigma_t=0.05 if seed < 2 else 0.7)
    ref_K = s['K'].copy()
    ref_K[0, 0] *= 1.25; ref_K[1, 1] *= 0.8; ref_K[0, 1] = 0.37; ref_K[0, 2] += 3.5           # not the target's intrinsics: ref_K is the one that counts
    scene = ops.Scene.from_views(s['poses'], s['images'], s['K'], ref_K, device=dev)
    for nb in (1, 4, 6):
        ref_nos, proj, _ = scene.select(torch.from_numpy(s['c2w']).to(dev), nb)
        want_ref = select_neighbors(s['c2w'], s['poses'], nb)
        np.testing.assert_array_equal(ref_nos.cpu().numpy(), want_ref)
        got = proj.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.int32), proj_f64(ref_K, s['poses'][want_ref]).view(np.int32))
        exact, bound = proj_exact_and_bound(ref_K, s['poses'][want_ref])
        assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
        host = projection_matrices(ref_K, s['poses'][want_ref])
        assert (np.abs(got.astype(np.float64) - host.astype(np.float64)) <= bound).all()          # ... and of the host's fp32 matmul


# ---------------------------------------------------------------------------------------------- 4. rays from a camera in device memory
@pytest.mark.parametrize('size', [(5, 7), (24, 32)])
def test_frame_rays_dev_is_bit_identical_to_frame_rays(dev, size):
    from pronerf_amd import ops
    from pronerf_amd.render import RayPartition
    H, W = size
    s = synth.make_scene(1, H=H, W=W, rotate=True)
    Kd, cd = torch.from_numpy(s['K']).to(dev), torch.from_numpy(s['c2w']).to(dev)
    cases = [{}, {'first': 3, 'count': H * W - 8}, {'first': H * W - 1, 'count': 1}]
    if (H, W) == (24, 32):
        part = RayPartition(H * W, 3)
        assert part.kind == 'cyclic' and sum(part.counts) == H * W
        cases += [part.frame_rays_args(r) for r in range(3)]
    for kw in cases:
        a, b = ops.frame_rays(s['K'], s['c2w'], H, W, near=0.0, far=1.0, or_near=1.0, or_far=10.0, device=dev, **kw)
        c, d = ops.frame_rays_dev(Kd, cd, H, W, near=0.0, far=1.0, or_near=1.0, or_far=10.0, **kw)
        assert c.shape == a.shape and a.shape[0] > 0
        assert torch.equal(_bits(a), _bits(c)) and torch.equal(_bits(b), _bits(d)), kw
    a, b = ops.frame_rays(s['K'], s['c2w'], H, W, near=0.25, far=0.75, or_near=2.0, or_far=7.0, device=dev)
    c, d = ops.frame_rays_dev(Kd, cd, H, W, near=0.25, far=0.75, or_near=2.0, or_far=7.0)
    assert torch.equal(_bits(a), _bits(c)) and torch.equal(_bits(b), _bits(d))


# ---------------------------------------------------------------------------------------------- 5. pose -> frame
@pytest.fixture(scope='module')
def weights():
    return synth.make_weights(0, 'trained')


def _quantised(images):
    q = np.round(images * 255.).astype(np.uint8)
    return q, (q / 255.).astype(np.float32)


@pytest.mark.parametrize('case', ['f32', 'f32_other_source_size', 'u8'])
def test_render_pose_equals_render_rays_on_its_own_intermediates_and_meets_the_oracle_bar(dev, weights, case):
    from pronerf_amd import ops
    from pronerf_amd.render import Renderer
    if case == 'f32_other_source_size':
        H, W = 20, 28
        scene = synth.make_scene(0, H=H, W=W, Hf=48, Wf=64, n_views=6)
    else:
        H, W = 24, 32
        scene = synth.make_scene(0, H=H, W=W, n_views=6)
    given = scene['images']
    if case == 'u8':
        given, as_float = _quantised(scene['images'])
        scene = {**scene, 'images': as_float}                               # the oracle renders from the same 8-bit images
    rend = Renderer(weights, max_rays=H * W, device=dev)
    sc = rend.set_scene(scene['poses'], given, scene['K'], cache='u8' if case == 'u8' else 'f32')
    assert (sc.Hf, sc.Wf) == scene['images'].shape[1:3]
    c2w_d = torch.from_numpy(scene['c2w']).to(dev)
    rgbd = rend.render_pose(c2w_d, H, W).clone()
    assert rgbd.shape == (H * W, 4)
    # the same rows from render_rays fed with the scene's own intermediates
    ref_nos, proj, img4 = sc.select(c2w_d, rend.num_neighbor)
    rays, or_rays = ops.frame_rays_dev(sc.K, c2w_d, H, W)
    want, _ = rend.ctx.render_rays(rays, or_rays, img4, proj)
    assert torch.equal(_bits(rgbd), _bits(want))
    # a host pose goes through the renderer's own device buffer: same rows; a sub-range renders its rows of the frame
    assert torch.equal(_bits(rend.render_pose(scene['c2w'], H, W)), _bits(want))
    part = rend.render_pose(c2w_d, H, W, first=37, count=101)
    assert torch.equal(_bits(part), _bits(want[37:138]))
    # the project's bar against the oracle (tests/test_mirror_gpu.py)
    fr = orc.frame_setup(scene, num_neighbor=4)
    np.testing.assert_array_equal(ref_nos.cpu().numpy(), fr['ref_nos'].numpy())
    ref = orc.render_rays_infer(weights, fr['rays'], fr['or_rays'], fr['images'], fr['proj'])
    ps = orc.psnr(rgbd[:, :3].cpu(), ref['rgb'])
    print(f'render_pose[{case}]: rgb PSNR vs oracle {ps:.2f} dB, max depth err {float((rgbd[:, 3].cpu() - ref["depth"]).abs().max()):.3e}')
    assert ps > 46.4
    np.testing.assert_allclose(rgbd[:, 3].cpu().numpy(), ref['depth'].numpy(), rtol=0, atol=2e-2)


# ---------------------------------------------------------------------------------------------- 6. one graph, many poses
def test_one_captured_graph_replays_any_pose(dev, weights):
    from pronerf_amd.render import Renderer, select_neighbors
    H, W = 24, 32
    scene = synth.make_scene(0, H=H, W=W, n_views=6, sigma_t=0.3)
    rend = Renderer(weights, max_rays=H * W, device=dev)
    rend.set_scene(scene['poses'], scene['images'], scene['K'])
    targets, seen = [], []
    for c2w in [scene['c2w']] + [p for p in scene['poses']]:
        nbrs = sorted(select_neighbors(c2w, scene['poses'], 4).tolist())
        if nbrs not in seen:
            seen.append(nbrs); targets.append(np.ascontiguousarray(c2w[:3, :4]))
    assert len(targets) >= 3, seen                                           # three poses whose neighbour sets differ
    targets = targets[:3]
    eager = [rend.render_pose(torch.from_numpy(t).to(dev), H, W).clone() for t in targets]
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    g = rend.capture_pose(H, W)
    for order in ((0, 1, 2), (2, 0, 1)):
        for i in order:
            out = g.replay(targets[i])
            assert out is g.rgbd
            assert torch.equal(_bits(out), _bits(eager[i])), i
    assert torch.equal(_bits(g.replay(torch.from_numpy(targets[1]).to(dev))), _bits(eager[1]))      # a pose that already lives on the device


# ---------------------------------------------------------------------------------------------- 7. the inference driver
def _models(dev):
    from types import SimpleNamespace
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    args = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256, mmnetskips=[10000],
                           N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)
    kw, _ = trt.create_nerf(args, device=dev)
    sd = synth.state_dicts(synth.make_weights(0, 'trained'))
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    return trt, kw


@pytest.mark.parametrize('cache', ['f32', 'u8'])
def test_render_path_with_a_scene_cache(dev, tmp_path, cache):
    """The set-up of tests/test_mirror_gpu.py::test_render_path_frame_loop with render_kwargs['pnrf_scene_cache']."""
    trt, kw = _models(dev)
    scene = synth.make_scene(0, H=24, W=32, n_views=6)
    if cache == 'u8':
        scene = {**scene, 'images': _quantised(scene['images'])[1]}
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'], pnrf_scene_cache=cache)
    targets = [scene['c2w'], scene['poses'][0]]
    fr = orc.frame_setup({**scene, 'c2w': scene['c2w']}, num_neighbor=4)
    ref = orc.render_rays_infer(synth.make_weights(0, 'trained'), fr['rays'], fr['or_rays'], fr['images'], fr['proj'])
    gt = [ref['rgb'].reshape(24, 32, 3).numpy(), np.zeros((24, 32, 3), np.float32)]
    rgbs0, rgbs1, depths, _ = trt.render_path(targets, (24, 32, scene['focal']), scene['K'], None, kw, gt_imgs=gt, savedir=str(tmp_path),
                                              n_timing_reps=2, verbose=False)
    assert rgbs0.shape == (2, 24, 32, 3) and rgbs1.shape == (2, 24, 32, 3) and depths.shape == (2, 24, 32)
    assert kw['psnrs'][0] > 46.4                      # frame 0 vs the oracle's image of the same pose
    assert len(kw['render_ms']) == 2 and all(len(t) == 2 and min(t) > 0 for t in kw['render_ms'])
    assert not np.array_equal(rgbs1[0], rgbs1[1])     # the second pose is another frame, not the buffer of the first
    for name in ('000.png', 'depth_000.png', '001.png', 'depth_001.png'):
        assert open(os.path.join(str(tmp_path), name), 'rb').read()[:8] == b'\x89PNG\r\n\x1a\n'
    if cache == 'f32':                                 # the same kwargs without the entry: today's statements, after a scene run in the same process
        kw.pop('pnrf_scene_cache')
        _, host1, hostd, _ = trt.render_path(targets, (24, 32, scene['focal']), scene['K'], None, kw, gt_imgs=gt, savedir=None, n_timing_reps=1, verbose=False)
        assert host1.shape == rgbs1.shape and hostd.shape == depths.shape and kw['psnrs'][0] > 46.4


def test_render_path_refuses_a_u8_cache_for_images_that_are_not_8_bit(dev, tmp_path):
    from pronerf_amd.ops import PnrfError
    trt, kw = _models(dev)
    scene = synth.make_scene(0, H=24, W=32, n_views=6)
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'], pnrf_scene_cache='u8')
    with pytest.raises(PnrfError, match='8-bit'):
        trt.render_path([scene['c2w']], (24, 32, scene['focal']), scene['K'], None, kw, n_timing_reps=1, verbose=False)
    kw['pnrf_scene_cache'] = 'f16'
    with pytest.raises(PnrfError):
        trt.render_path([scene['c2w']], (24, 32, scene['focal']), scene['K'], None, kw, n_timing_reps=1, verbose=False)
