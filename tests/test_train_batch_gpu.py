"""GPU: the device-resident training set (pnrf_scene_arrays, pnrf_scene_rank_table_fwd, pnrf_train_batch_fwd; ops.Scene.arrays / rank_table,
ops.TrainSet, --device_batches of the two training drivers).  A batch assembled on the device from ray indices must be the batch the drivers assemble
on the host today: rays, targets and neighbour views bit for bit, hence the trainer's loss and gradients bit for bit, hence a training run's
parameters bit for bit; the draws of the device generator must be the float64 restatement of tests/batch_ref.py within the derived bound."""
import random

import numpy as np
import pytest
import torch

import batch_ref as R
from oracle import pronerf_oracle as orc
from oracle import synth
from test_scene_gpu import _dyadic_scene, _rand_poses

pytestmark = pytest.mark.gpu

SCENES = [(5, 1, 1), (6, 5, 7), (9, 24, 32)]
NS = [1, 63, 64, 65, 257, 1000]
NEARS = [0.0, 1e-6]                                    # stage 2, stage 1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _K(Hf, Wf):
    f = 1.3 * max(Hf, Wf) + 0.37
    return np.array([[f, 0, 0.5 * Wf], [0, f, 0.5 * Hf], [0, 0, 1]], dtype=np.float32)


_CASES = {}


def _case(dev, shape):
    """One scene per shape, its host-side reference computed once: per-pixel rays of every view (ops.frame_rays, both drivers' near), targets, owner
    views and the rank table of the stage-2 driver."""
    if shape not in _CASES:
        from pronerf_amd import ops
        from pronerf_amd.run_S_eS_eN_alter_base_refine2 import neighbor_rank_table
        nv, Hf, Wf = shape
        rs = np.random.RandomState(nv * 1000 + Hf * 10 + Wf)
        poses = _rand_poses(rs, nv)
        images = rs.rand(nv, Hf, Wf, 3).astype(np.float32)
        images[0].reshape(-1)[:3] = [0.0, 1.0, np.float32(1e-42)]                  # end points and a subnormal in pixel 0 of view 0 ...
        images[1].reshape(-1)[0] = -0.0                                            # ... a signed zero in pixel 0 of view 1: a copy keeps them
        K = _K(Hf, Wf)
        scene = ops.Scene.from_views(poses, images, K, device=dev)
        ref = {}
        for near in NEARS:
            pr = [ops.frame_rays(K, poses[v], Hf, Wf, near=near, far=1., device=dev) for v in range(nv)]
            ref[near] = (torch.cat([p[0] for p in pr], 0), torch.cat([p[1] for p in pr], 0))
        _CASES[shape] = dict(nv=nv, Hf=Hf, Wf=Wf, plane=Hf * Wf, poses=poses, images=images, K=K, scene=scene, ref=ref,
                             target=torch.from_numpy(images.reshape(-1, 3)).to(dev), own=torch.arange(nv, device=dev).repeat_interleave(Hf * Wf),
                             rank=torch.from_numpy(neighbor_rank_table(poses)).to(dev),
                             sets={near: ops.TrainSet(scene, max(NS), near=near, far=1., max_cols=8) for near in NEARS})
    return _CASES[shape]


def _idx(c, n, seed=0):
    """n ray indices: first and last pixel of the first and last view, the pixels with the special texels, duplicates, then random ones."""
    plane, nv = c['plane'], c['nv']
    special = [0, plane - 1, (nv - 1) * plane, nv * plane - 1, plane, nv * plane - 1, 0, min(1, plane - 1)]
    rs = np.random.RandomState(n + seed)
    pool = special + rs.randint(0, nv * plane, max(n, 8)).tolist()
    got = pool[:n] if n >= 8 else special[3:3 + n]
    return np.asarray(got, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- 1. rank table, scene arrays
@pytest.mark.parametrize('nv', [5, 6, 20, 300])
def test_rank_table_equals_neighbor_rank_table(dev, nv):
    from pronerf_amd import ops
    from pronerf_amd.run_S_eS_eN_alter_base_refine2 import neighbor_rank_table
    rs = np.random.RandomState(nv)
    dy = _dyadic_scene(nv, rs)[1]                       # exact ties (views 1 and 2 mirrored about the last one) ...
    dy[3, :, 3] = dy[0, :, 3]                           # ... and two views at the same position
    cases = [dy, _rand_poses(rs, nv), _rand_poses(rs, nv, 0.01), synth.make_scene(nv, H=2, W=2, n_views=nv)['poses']]
    imgs = np.zeros((nv, 2, 2, 3), np.float32)
    for i, poses in enumerate(cases):
        scene = ops.Scene.from_views(poses, imgs, np.eye(3, dtype=np.float32), device=dev)
        got = scene.rank_table()
        assert got.dtype == torch.int32 and got.shape == (nv, nv)
        want = neighbor_rank_table(poses)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'case {i}')
        if i == 0:
            g = got.cpu().numpy()
            assert g[0, 0] == 0 and g[0, 1] == 3 and g[3, 0] == 0 and g[3, 1] == 3          # the coincident pair: lower index first, in both rows
            row = g[nv - 1].tolist()
            assert row.index(1) + 1 == row.index(2)                                         # the mirrored pair in index order


@pytest.mark.parametrize('shape', SCENES)
def test_scene_arrays_are_what_the_trainer_takes(dev, shape):
    from pronerf_amd import ops
    c = _case(dev, shape)
    img4, poses, Kt, Kr = c['scene'].arrays()
    want = ops.images_pack(torch.from_numpy(c['images']).permute(0, 3, 1, 2).contiguous().to(dev))
    assert img4.shape == want.shape and torch.equal(_bits(img4), _bits(want))
    assert torch.equal(poses.cpu(), torch.from_numpy(c['poses'])) and torch.equal(Kt.cpu(), torch.from_numpy(c['K'])) and torch.equal(Kr.cpu(), Kt.cpu())
    u8 = ops.Scene.from_views(c['poses'], np.zeros((c['nv'], 2, 2, 3), np.uint8), c['K'], cache='u8', device=dev)
    with pytest.raises(ops.PnrfError, match='PNRF_SCENE_F32'):
        u8.arrays()
    part = ops.Scene(c['nv'], 2, 2, device=dev).set_intrinsics(c['K'])
    part.set_view(0, np.zeros((2, 2, 3), np.float32), c['poses'][0])
    with pytest.raises(ops.PnrfError, match='not complete'):
        part.arrays()
    with pytest.raises(ops.PnrfError, match='not complete'):
        part.rank_table()


# ---------------------------------------------------------------------------------------------- 2. rays, target, ref_nos
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('shape', SCENES)
def test_batch_rows_equal_the_host_assembled_batch(dev, shape, n):
    c = _case(dev, shape)
    nv = c['nv']
    idx = torch.from_numpy(_idx(c, n)).to(dev)
    rs = np.random.RandomState(n)
    orders = [(0, 1, 2, 3), tuple(range(nv - 5, nv - 1)), tuple(sorted(rs.choice(nv - 1, 4, replace=False).tolist()))]
    for near in NEARS:
        ts = c['sets'][near]
        before = ts.bad_rows()
        for order in orders:
            rays, or_rays, target, img4, poses, K, ref_nos = ts.batch(idx, order)
            want_r, want_o = c['ref'][near]
            assert rays.shape == (n, 11) and or_rays.shape == (n, 11) and target.shape == (n, 3) and ref_nos.shape == (n, 4) and ref_nos.dtype == torch.int64
            assert torch.equal(_bits(rays), _bits(want_r[idx])) and torch.equal(_bits(or_rays), _bits(want_o[idx])), (near, order)
            assert torch.equal(_bits(target), _bits(c['target'][idx]))
            want_ref = c['rank'][c['own'][idx]][:, 1:][:, torch.as_tensor(order, device=dev)]          # today's statement
            assert torch.equal(ref_nos, want_ref), (near, order)
            assert img4.data_ptr() == ts.img4.data_ptr() and float(rays[0, 6]) == np.float32(near) and float(rays[0, 7]) == 1.0
        assert ts.bad_rows() == before
    if n >= 8:                                                                      # the special texels went through
        t = _bits(c['sets'][0.0].batch(idx, orders[0])[2]).cpu().numpy()
        assert t[0].tolist() == [0, 0x3f800000, int(np.float32(1e-42).view(np.int32))] and t[4, 0] == np.int32(-2 ** 31)


# ---------------------------------------------------------------------------------------------- 3. bad indices, argument errors
@pytest.mark.parametrize('shape', SCENES)
def test_bad_indices_get_nan_rows_and_are_counted(dev, shape):
    from pronerf_amd import ops
    c = _case(dev, shape)
    n = 257
    good = _idx(c, n, seed=1)
    bad = good.copy()
    where = [0, 5, 64, 255, 256]
    bad[where] = [-1, c['nv'] * c['plane'], -2 ** 40, 2 ** 62, c['nv'] * c['plane']]
    ts = ops.TrainSet(c['scene'], n, near=0., far=1.)
    order = (0, 1, 2, 3)
    clean = [t.clone() for t in ts.batch(torch.from_numpy(good).to(dev), order)]
    assert ts.bad_rows() == 0
    got = ts.batch(torch.from_numpy(bad).to(dev), order)
    assert ts.bad_rows() == len(where)
    keep = np.setdiff1d(np.arange(n), where)
    for k in (0, 1, 2):
        assert bool(torch.isnan(got[k][where]).all())
        assert torch.equal(_bits(got[k][keep]), _bits(clean[k][keep]))
    assert bool((got[6][where] == 0).all()) and torch.equal(got[6][keep], clean[6][keep])
    ts.batch(torch.from_numpy(bad).to(dev), order)
    assert ts.bad_rows() == 2 * len(where)


def test_argument_errors_raise_before_any_launch(dev):
    import ctypes as C
    from pronerf_amd import _lib, ops
    c = _case(dev, (6, 5, 7))
    ts = ops.TrainSet(c['scene'], 64, near=0., far=1., max_cols=8)
    idx = torch.from_numpy(_idx(c, 64)).to(dev)
    ts.batch(idx, (0, 1, 2, 3), step=1, jitter_cols=8, noise_cols=8, noise_std=1.)
    for t in (ts._rays, ts._or_rays, ts._target, ts._jitter, ts._noise):
        t.fill_(7.0)
    ts._ref_nos.fill_(7)
    bad_calls = [dict(order=(0, 1, 2, 5)), dict(order=(-1, 1, 2, 3)), dict(order=(0, 1, 2)), dict(order=(0, 1, 2, 3), step=1, jitter_cols=6),
                 dict(order=(0, 1, 2, 3), step=1, noise_cols=12), dict(order=(0, 1, 2, 3), jitter_cols=8), dict(order=(0, 1, 2, 3), row0=-1)]
    for kw in bad_calls:
        with pytest.raises(ops.PnrfError):
            ts.batch(idx, **kw)
    with pytest.raises(ops.PnrfError):
        ts.batch(torch.cat([idx, idx]), (0, 1, 2, 3))                                # more rays than the set was sized for
    with pytest.raises(ops.PnrfError):
        ts.batch(idx.to(torch.int32), (0, 1, 2, 3))
    lib = _lib.load()
    order = (C.c_int * 4)(0, 1, 2, 3)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda n, rays, cj, cn: lib.pnrf_train_batch_fwd(ts.scene.handle, p(ts.rank), p(idx), n, order, 0., 1., 1., 10., rays, p(ts._or_rays), p(ts._target),
                                                           p(ts._ref_nos), None, 0, 1, 0, p(ts._jitter), cj, 0.99, p(ts._noise), cn, 1., None)
    assert call(-1, p(ts._rays), 8, 8) == -1 and call(64, None, 8, 8) == -1 and call(64, p(ts._rays), 260, 8) == -1 and call(64, p(ts._rays), 8, 2) == -1
    four = ops.Scene.from_views(c['poses'][:4], c['images'][:4], c['K'], device=dev)          # nv < 5: no four neighbours besides the view itself
    with pytest.raises(ops.PnrfError, match='nv - 1'):
        ops.TrainSet(four, 64, near=0., far=1.).batch(idx, (0, 1, 2, 2))
    torch.cuda.synchronize()
    for t in (ts._rays, ts._or_rays, ts._target, ts._jitter, ts._noise):
        assert bool((t == 7.0).all())                                                # nothing was launched by any refused call
    assert bool((ts._ref_nos == 7).all()) and ts.bad_rows() == 0


# ---------------------------------------------------------------------------------------------- 4. draws
@pytest.fixture(scope='module')
def draw_set(dev):
    from pronerf_amd import ops
    return ops.TrainSet(_case(dev, (5, 1, 1))['scene'], 257, near=0., far=1., max_cols=256)


@pytest.mark.parametrize('Cj', [8, 16, 256])
def test_draws_equal_the_float64_restatement(dev, draw_set, Cj):
    """The normals behind ``noise`` (std 1) against float64.  u0 >= 2^-24 gives |z| <= sqrt(48 ln 2) = 5.77; an angle error of 2 pi 2^-24 plus four
    fp32 ulps of function error (logf, sqrt, sincospi, the product) scale with it: 5.77 (3.7e-7 + 2.4e-7) = 3.6e-6 < 4e-6 absolute.  The jitter is
    a fifth of that plus half an ulp of the quotient: 1e-6."""
    n, Cn, seed, step = 257, 8, 20240611, 7
    idx = torch.zeros(n, dtype=torch.int64, device=dev)
    for row0 in (0, 2 ** 31):                                                        # row0 2^31 with 64 quads per row: the quad index needs the counter's second word
        for cap in (np.float32(1 - 2e-6), np.float32(0.99), np.float32(0.1)):
            out = draw_set.batch(idx, (0, 1, 2, 3), step=step, seed=seed, row0=row0, jitter_cols=Cj, jitter_cap=float(cap), noise_cols=Cn, noise_std=1.0)
            jit, noi = out[7].cpu().numpy(), out[8].cpu().numpy()
            assert jit.shape == (n, Cj) and noi.shape == (n, Cn)
            zn = R.normals(n, Cn, seed, step, R.STREAM_NOISE, row0)
            zj = R.normals(n, Cj, seed, step, R.STREAM_JITTER, row0)
            e_n = float(np.abs(noi.astype(np.float64) - zn).max())
            e_j = float(np.abs(jit.astype(np.float64) - np.minimum(np.abs(zj) / 5, float(cap))).max())
            print(f'draws Cj={Cj} row0={row0} cap={cap}: max |noise - ref| {e_n:.3e} (bound 4e-6), max |jitter - ref| {e_j:.3e} (bound 1e-6)')
            assert e_n <= 4e-6 and e_j <= 1e-6
            assert bool((jit <= cap).all()) and bool((jit >= 0).all())
            if cap == np.float32(0.1):
                assert bool((jit == cap).any())                                      # the cap was exercised


def test_draws_are_deterministic_split_invariant_and_keyed(dev, draw_set):
    n = 100
    idx = torch.zeros(n, dtype=torch.int64, device=dev)
    kw = dict(step=3, seed=5, jitter_cols=16, jitter_cap=0.99, noise_cols=8, noise_std=1.0)
    draw = lambda m=n, **over: [t.clone() for t in draw_set.batch(idx[:m], (0, 1, 2, 3), **{**kw, **over})[7:]]
    a, b = draw(), draw()
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = draw()
    side.synchronize()
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, s))
    tail = draw(40, row0=60)
    assert all(torch.equal(_bits(x[60:]), _bits(y)) for x, y in zip(a, tail))
    for over in (dict(seed=6), dict(seed=5 + 2 ** 32), dict(step=4)):
        o = draw(**over)
        assert not torch.equal(a[0], o[0]) and not torch.equal(a[1], o[1]), over
    j8 = draw(jitter_cols=8, jitter_cap=1e9)[0]                                      # stream 0 against stream 1 at the same width: other normals
    assert not torch.equal(j8, a[1].abs() / 5)


# ---------------------------------------------------------------------------------------------- 5. one trainer iteration
def _host_batch(dev, scene, near, idx, order):
    """Today's statements of the drivers (run_S_eS_eN_alter_base_refine2.py / ..._base.py train())."""
    from pronerf_amd import ops
    from pronerf_amd import run_S_eS_eN_alter_base_refine2 as s2
    images, poses, K = scene['images'], scene['poses'], scene['K']
    H, W = images.shape[1:3]
    pr = [ops.frame_rays(K, poses[i], H, W, near=near, far=1., device=dev) for i in range(len(poses))]
    rays_all = torch.cat([p[0] for p in pr], 0); or_rays_all = torch.cat([p[1] for p in pr], 0)
    target_all = torch.as_tensor(images, dtype=torch.float32).reshape(-1, 3).to(dev)
    own_all = torch.arange(len(poses), device=dev).repeat_interleave(H * W)
    img4, poses_t, K_t, rank = s2._train_views(images, poses, K, dev)
    order = torch.as_tensor(order, device=dev)
    ref_nos = rank[own_all[idx]][:, 1:][:, order].contiguous()
    return rays_all[idx], or_rays_all[idx], target_all[idx], img4, poses_t, K_t, ref_nos


def _grads(tr):
    return [tuple(_bits(t).clone() for t in tr.read('grad', i)) for i in range(26)]


@pytest.mark.parametrize('kind', ['stage2', 'explore'])
def test_trainer_iteration_is_bit_identical_from_either_batch(dev, kind):
    from pronerf_amd import ops
    H, W, nv, n = 24, 32, 9, 257
    scene = synth.make_scene(1, H=H, W=W, n_views=nv, sigma_t=0.2, rotate=True)
    w = synth.make_weights(1, 'trained'); w['nerfcls'] = synth.make_nerfcls_weights(1, head_scale=0.3)
    layers = orc.trainer_layers(w)
    n_mult = 2
    S = 8 if kind == 'stage2' else 8 * n_mult
    near = 0. if kind == 'stage2' else 1e-6
    tr = ops.Trainer([W_ for W_, _ in layers], [b for _, b in layers], max_rays=n, device=dev, max_samples=S)
    g = torch.Generator(device=dev).manual_seed(3)
    idx = torch.randperm(nv * H * W, device=dev, generator=g)[:n]
    order = [1, 3, 4, 7]
    jitter = torch.abs(torch.normal(0.0, 1.0, size=(n, S), device=dev, generator=g) / 5).clamp(max=1 - 2e-6 if kind == 'stage2' else 0.99)
    noise = torch.randn(n, S, device=dev, generator=g)
    ts = ops.TrainSet(ops.Scene.from_views(scene['poses'], scene['images'], scene['K'], device=dev), n, near=near, far=1.)

    def run(head):
        if kind == 'stage2':
            L, _ = tr.fwd_bwd(*head, jitter=jitter, jitter_dir=-1, raw_noise=noise, a_mmrgb=0.0, want_rgb=False)
        else:
            L, _ = tr.explore_fwd_bwd(*head, n_mult=n_mult, dir1=-1, jitter=jitter, dir2=1, raw_noise=noise, want_rgb=False)
        return _bits(L).clone(), _grads(tr)
    L_host, g_host = run(_host_batch(dev, scene, near, idx, order))
    for li in range(26):                                   # poison the gradients: the second run has to write them all again (NeRF layers on 'explore')
        tr.write('grad', li, torch.full(layers[li][0].shape, 3.0).to(dev), torch.full(layers[li][1].shape, 3.0).to(dev))
    L_dev, g_dev = run(ts.batch(idx, order))
    assert L_host.shape == (4,) and torch.equal(L_host, L_dev) and bool(torch.isfinite(L_dev.view(torch.float32)).all())
    for li in (range(26) if kind == 'stage2' else range(14, 26)):
        assert torch.equal(g_host[li][0], g_dev[li][0]) and torch.equal(g_host[li][1], g_dev[li][1]), li
    assert any(bool((gw.view(torch.float32) != 0).any()) for gw, _ in g_dev[14:])


# ---------------------------------------------------------------------------------------------- 6. the drivers
def _params(tr):
    return [tuple(_bits(t).cpu() for t in tr.read('param', i)) for i in range(26)]


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize('stage', [2, 1])
def test_drivers_with_device_batches(dev, tmp_path, stage, monkeypatch):
    import llff_synth
    from pronerf_amd import ops
    from pronerf_amd import run_S_eS_eN_alter_base as s1
    from pronerf_amd import run_S_eS_eN_alter_base_refine2 as s2
    root = llff_synth.make_dataset(str(tmp_path / 'scene'), seed=2, n=10, H=24, W=32, factor=4)
    common = (f'basedir = {tmp_path}/logs\ndatadir = {root}\nfactor = 4\nllffhold = 8\nN_rand = 512\nN_samples = 8\nN_point_ray_enc = 48\nmmnetdepth = 6\n'
              'mmnetskips = [10000]\nnum_neighbor = 4\nuse_viewdirs = True\nraw_noise_std = 1e0\nlrate = 5e-4\nweight_decay = 5e-8\ni_print = 2\ni_weights = 1000\n')
    if stage == 2:
        w = synth.make_weights(0, 'trained'); wc = synth.make_nerfcls_weights(0, head_scale=0.3)
        sds = synth.state_dicts(w)
        pre = str(tmp_path / 'stage1.tar')
        torch.save({'global_step': 7, 'network_fn_state_dict': synth.nerfcls_state_dict(wc), 'mmr_network_fn_state_dict': sds['sampler'],
                    'refine_net_state_dict': sds['refine']}, pre)
        common += f'pretrain_path = {pre}\n'
    cfg = tmp_path / 'train.txt'
    cfg.write_text(common)
    mod, steps, entry = (s2, 6, 'fwd_bwd') if stage == 2 else (s1, 8, 'explore_fwd_bwd')
    first = {}
    orig = getattr(ops.Trainer, entry)

    def spy(self, *a, **kw):                                # the jitter of a run's first iteration (stage 1: iteration 1 is an exploration)
        if 'jitter' not in first:
            first['jitter'] = kw['jitter'].clone()
        return orig(self, *a, **kw)
    monkeypatch.setattr(ops.Trainer, entry, spy)

    def run(name, *extra):
        first.clear()
        random.seed(11); np.random.seed(11); torch.manual_seed(11); torch.cuda.manual_seed_all(11)
        tr, log = mod.train(['--config', str(cfg), '--expname', name, '--max_steps', str(steps)] + list(extra), device=dev)
        losses = [e[1] for e in log if e[1] != 'test_psnr']
        assert len(losses) == steps // 2 and all(np.isfinite(x) for x in losses), log
        return _params(tr), first['jitter']
    off_a, j_off = run('off_a')
    off_b, _ = run('off_b', '--device_batches', 'off')
    assert _same(off_a, off_b), 'two runs of today\'s statements with the same seeds do not agree bit for bit'
    rays, j_rays = run('rays', '--device_batches', 'rays')
    assert torch.equal(j_off, j_rays)                        # torch's draws, in the same call order
    assert _same(off_a, rays)
    all_a, j_a = run('all_a', '--device_batches', 'all', '--batch_seed', '77')
    all_b, j_b = run('all_b', '--device_batches', 'all', '--batch_seed', '77')
    assert _same(all_a, all_b) and torch.equal(_bits(j_a), _bits(j_b))
    assert not _same(all_a, off_a)
    all_c, j_c = run('all_c', '--device_batches', 'all', '--batch_seed', '78')
    assert not torch.equal(j_a, j_c) and not _same(all_a, all_c)
    # the first batch's jitter straight from a training set (the draws do not depend on the scene): step 1, row0 0
    Cj = j_a.shape[1]
    assert j_a.shape[0] == 512 and Cj % 8 == 0 and (Cj == 8 or stage == 1)
    ts = ops.TrainSet(_case(dev, (5, 1, 1))['scene'], 512, near=0., far=1., max_cols=64)
    want = ts.batch(torch.zeros(512, dtype=torch.int64, device=dev), (0, 1, 2, 3), step=1, seed=77, jitter_cols=Cj,
                    jitter_cap=1 - 2e-6 if stage == 2 else 0.99)[7]
    assert torch.equal(_bits(j_a), _bits(want))
