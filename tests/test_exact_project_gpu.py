"""GPU: neighbour-view projection and colour fetch — warp_trt_kernel, warp_train_kernel, refine_input_kernel, refine_input_train_kernel and
images_pack_kernel — bit for bit against the float32 replay of tests/exact_project.py on every input set, and against float64.

Exact assertions (``assert_array_equal``):
  * every kernel on its exact sets (images 5 x 9 and 9 x 17; tests/test_exact_project_cpu.py certifies the replay there and the edges the
    sets hold) against the replay, and against the float64 run rounded to fp32 (the training forms' run rounds the certified
    |c2.z| + 1e-8f to fp32 as the kernels do; the mean-fill columns, one division by fl(cnt + 1e-6f), within 2 ulp);
  * refine_input at nb = 1 .. 8 and 1 / 63 / 64 / 65 / 257 rays (the 64-ray tile, waves k and k + 4), refine_input_train in both layouts
    at 1 / 7 / 8 / 9 / 257 rays (the 32-lane groups of a ragged block), the warps at B = 1, 3, shared and per-view rays, 1 / 255 / 256 / 257
    pixels; one call of each past the 4096-block cap against the tiling of the small result;
  * the general sets (random poses, textured 13 x 19 images) against the replay, bit for bit;
  * a NaN depth and an infinite direction: zeros in their own (view, sample) colours, every other output bit for bit as without them;
  * the fused head (pnrf_refine_project_fwd) on integer nets: torch.equal to pnrf_refine_fwd on the reference's refine_in, for every
    (num_neighbor, depth) of exact_nets.REFINE_CONFIGS, default / bf16 / refine_16x16, wide and narrow, two nets with skip connections,
    refusals asserted.  Half of the set's rays move across the image with the sample's depth, so the sample order, eps, the B half
    of view_ray and the fetch pipeline's slots are held too.  v_rcp_f32 is assumed good to 1 ulp only (the CPU certificate); (a) held
    bit for bit on the first run.
Bounded assertions: every output element on the general sets within the derived per-element bound of float64 (exact_project's docstring;
the worst error / bound per kernel is printed at the end of the module).
"""
import functools

import numpy as np
import pytest
import torch

import exact_project as P

pytestmark = pytest.mark.gpu

WORST = {}
KERNELS = ('refine_input', 'refine_input_train', 'warp_trt', 'warp_train')


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    if WORST:
        print('\n[exact_project] worst error / bound: ' + '   '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def launch(kernel, inp, dev, nb=None, layout=0):
    """One kernel through pronerf_amd.ops on an input set -> the output tensor (on the device)."""
    from pronerf_amd import ops
    t = lambda k: cu(inp[k], dev)
    if kernel == 'refine_input':
        nb = inp['proj'].shape[0] if nb is None else nb
        return ops.refine_input(t('rays'), t('or_rays'), t('depth'), ops.images_pack(cu(inp['img'][:nb], dev)), cu(inp['proj'][:nb], dev), eps=inp['eps'])
    if kernel == 'refine_input_train':
        return ops.refine_input_train(t('rays'), t('or_rays'), t('depth'), ops.images_pack(t('img')), t('poses'), t('K'), t('ref_nos'), eps=inp['eps'],
                                      layout=layout)
    if kernel == 'warp_trt':
        return ops.warp_trt(t('img'), t('depth'), t('ro1'), t('rd1'), t('w2c'))
    return ops.warp_train(t('img'), t('depth'), t('ro1'), t('rd1'), t('c2w2'), t('K'))


def run(kernel, inp, dev, **kw):
    return launch(kernel, inp, dev, **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def exact_set(kernel, size):
    if kernel == 'refine_input':
        return P.exact_inference(size)
    if kernel == 'refine_input_train':
        return P.exact_training(size)
    return P.exact_warp(kernel[5:], size)


@functools.lru_cache(maxsize=None)
def general_set(kernel):
    if kernel == 'refine_input':
        return P.general_inference()
    if kernel == 'refine_input_train':
        return P.general_training()
    return P.general_warp(kernel[5:])


def check_float64(kernel, got, inp, exact, **kw):
    """Against the float64 run: rounded to fp32 it is the answer on the exact sets (mean-fill columns: 2 ulp); within the bound elsewhere."""
    if exact:
        ref = P.run64(kernel, inp, absorb=True, **kw)[0].astype(np.float32)
        fill = P.filled_columns(inp, kw['layout']) if kernel == 'refine_input_train' else np.zeros(got.shape, bool)
        np.testing.assert_array_equal(got[~fill], ref[~fill], err_msg=f'{kernel} {kw} float64')
        assert (P.ulp_distance(got, ref)[fill] <= 2).all(), (kernel, kw)       # the mean fill's division by fl(cnt + 1e-6f)
        return
    ref, mag, _ = P.run64(kernel, inp, **kw)
    r = P.worst_ratio(got, ref, P.bound(P.D[kernel], mag))
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    assert r <= 1, (kernel, kw, r)


def test_images_pack(dev):
    """[nv,3,Hf,Wf] -> [nv,Hf,Wf,4]: the three channels bit for bit, w == 0."""
    from pronerf_amd import ops
    for img in (P.exact_images(8, 9, 17), P.exact_images(1, 5, 9), P.general_images(np.random.RandomState(1), 6)):
        out = ops.images_pack(cu(img, dev)).cpu().numpy()
        assert out.shape == (img.shape[0],) + img.shape[2:] + (4,)
        np.testing.assert_array_equal(out[..., :3], img.transpose(0, 2, 3, 1))
        np.testing.assert_array_equal(out[..., 3], 0.0)


@pytest.mark.parametrize('nb', P.NBS)
def test_refine_input_exact(dev, nb):
    """refine_input on the exact and the general set at nb views: every call bit for bit the replay; float64 at the full size."""
    for exact, inp in [(True, exact_set('refine_input', s)) for s in (0, 1)] + [(False, general_set('refine_input'))]:
        exp = P.emulate('refine_input', inp, nb=nb)
        for n in P.NS_INPUT:
            got = run('refine_input', P.head(inp, n), dev, nb=nb)
            np.testing.assert_array_equal(got, exp[:n], err_msg=f'nb={nb} n={n} exact={exact}')
        check_float64('refine_input', got, inp, exact, nb=nb)


@pytest.mark.parametrize('layout', [0, 1])
def test_refine_input_train_exact(dev, layout):
    """refine_input_train in one layout: every call bit for bit the replay (the mean fill's division included); float64 as check_float64 says."""
    for exact, inp in [(True, exact_set('refine_input_train', s)) for s in (0, 1)] + [(False, general_set('refine_input_train'))]:
        exp = P.emulate('refine_input_train', inp, layout=layout)
        for n in P.NS_TRAIN:
            got = run('refine_input_train', P.head(inp, n), dev, layout=layout)
            np.testing.assert_array_equal(got, exp[:n], err_msg=f'layout={layout} n={n} exact={exact}')
        check_float64('refine_input_train', got, inp, exact, layout=layout)
    # the two layouts hold the same values in their two orders
    a = run('refine_input_train', inp, dev, layout=layout)[:, 48:]
    b = run('refine_input_train', inp, dev, layout=1 - layout)[:, 48:]
    first, second = ((4, 8), (8, 4)) if layout == 0 else ((8, 4), (4, 8))
    np.testing.assert_array_equal(a.reshape(-1, *first, 3).transpose(0, 2, 1, 3), b.reshape(-1, *second, 3))


@pytest.mark.parametrize('kind', ['trt', 'train'])
def test_warp_exact(dev, kind):
    """warp_trt / warp_train at B = 1, 3, with one shared copy of the rays (ray_bstride = 0) and with rays per view, 1 .. 257 pixels."""
    kernel = 'warp_' + kind
    for exact, full in [(True, exact_set(kernel, s)) for s in (0, 1)] + [(False, general_set(kernel))]:
        for B in P.BS_WARP:
            for shared in (True, False):
                inp = P.warp_head(full, B, P.N_SET, shared)
                exp = P.emulate(kernel, inp)
                for n in P.NS_WARP:
                    got = run(kernel, P.warp_head(full, B, n, shared), dev)
                    np.testing.assert_array_equal(got, exp[:, :, :n], err_msg=f'{kernel} B={B} shared={shared} n={n} exact={exact}')
                check_float64(kernel, got, inp, exact)


def _equal_tiled(big, small, axis):
    idx = torch.arange(big.shape[axis], device=big.device) % small.shape[axis]
    return torch.equal(big, small.index_select(axis, idx))


def test_refine_input_past_the_block_cap(dev):
    """262 209 rays at nb = 5: 4097 tiles on 4096 blocks, so block 0 takes a second, ragged tile (65 rays of the last 128).  The tiled
    exact set gives the tiling of the 257-ray result, which is the replay."""
    inp = exact_set('refine_input', 1)
    small = launch('refine_input', inp, dev, nb=5)
    np.testing.assert_array_equal(small.cpu().numpy(), P.emulate('refine_input', inp, nb=5))
    big = launch('refine_input', P.tile(inp, P.N_INPUT_CAP), dev, nb=5)
    assert big.shape == (P.N_INPUT_CAP, 48 + 24 * 5) and _equal_tiled(big, small, 0)


@pytest.mark.parametrize('layout', [0, 1])
def test_refine_input_train_past_the_block_cap(dev, layout):
    """32 777 rays: 1 048 864 lanes on 4096 blocks of 256 — a second round in which only the first 288 lanes are live, the others
    shuffling with their groups all the same."""
    inp = exact_set('refine_input_train', 1)
    small = launch('refine_input_train', inp, dev, layout=layout)
    np.testing.assert_array_equal(small.cpu().numpy(), P.emulate('refine_input_train', inp, layout=layout))
    big = launch('refine_input_train', P.tile(inp, P.N_TRAIN_CAP), dev, layout=layout)
    assert big.shape == (P.N_TRAIN_CAP, 144) and _equal_tiled(big, small, 0)


@pytest.mark.parametrize('kind', ['trt', 'train'])
def test_warp_past_the_block_cap(dev, kind):
    """B n = 1 048 593 pixels on 4096 blocks of 256 threads: 17 threads take a second pixel."""
    kernel = 'warp_' + kind
    inp = P.warp_head(exact_set(kernel, 1), 3, P.N_SET, False)
    small = launch(kernel, inp, dev)
    np.testing.assert_array_equal(small.cpu().numpy(), P.emulate(kernel, inp))
    big = launch(kernel, P.warp_tile(inp, P.N_WARP_CAP), dev)
    assert big.shape == (3, 3, P.N_WARP_CAP) and _equal_tiled(big, small, 2)


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize('kernel', ['refine_input', 'refine_input_train'])
def test_non_finite_coordinates_stay_in_their_sample(dev, kernel):
    """A NaN depth at (ray 70, sample 3) and an infinite direction on ray 135 of the general set: the colours of (ray 70, every view,
    sample 3) and of ray 135 are zeros, the Pluecker columns of the NaN depth are NaN, and every other output keeps the bits of the
    clean call — which is what the replay says."""
    clean = general_set(kernel)
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    inp['depth'][70, 3] = np.nan
    inp['or_rays'][135, 3] = np.inf
    kw = dict(nb=8) if kernel == 'refine_input' else dict(layout=0)
    nbv = 8 if kernel == 'refine_input' else 4
    got, base = run(kernel, inp, dev, **kw), run(kernel, clean, dev, **kw)
    col = got[:, 48:].reshape(-1, nbv, 8, 3)
    np.testing.assert_array_equal(col[70, :, 3], 0.0)
    np.testing.assert_array_equal(col[135], 0.0)
    assert np.isnan(got[70, 3 * 6 + 3:3 * 6 + 6]).all()
    t = np.zeros(col.shape, bool)
    t[70, :, 3] = True
    t[135] = True
    touched = np.concatenate([np.zeros((got.shape[0], 48), bool), t.reshape(got.shape[0], -1)], 1)
    touched[70, 18:24] = True
    np.testing.assert_array_equal(_bits(got)[~touched], _bits(base)[~touched])
    np.testing.assert_array_equal(got, P.emulate(kernel, inp, **kw))


# ------------------------------------------------------------------------------------------------ the fused head (pnrf_refine_project_fwd)
def _head_refusal(nb, variant, skips):
    """What pnrf_refine_project_fwd must refuse, as a pattern of the error: the bf16 stage projects at most 4 views; a net with skip
    connections runs the default variant only."""
    if skips:
        return None if variant == 'default' else 'skip'
    return 'num_neighbor' if variant == 'bf16' and nb > 4 else None


def _head_runs(dev, net, pack, lim, nb, counts, variants, shapes, skips, what):
    """(a) refine_project_fwd == refine_fwd on the reference's refine_in, bit for bit; (b) both within the stage's tolerances of
    refine_reference — for every variant, shape and ray count; refusals asserted."""
    from pronerf_amd import ops
    import exact_nets as E
    import test_exact_stages_gpu as ST
    n_set = max(counts)
    inp = P.head_set(nb, n_set)
    x = P.head_refine_in(inp).astype(np.float32)
    if n_set > 257:
        cert = max(E.refine_counts(E.CU_CERT, big=True))
        if n_set > cert:                                           # a larger device than the CPU test certified for: certify here
            P.head_certificate(inp)
    y = pack['exact'](net, x, lim)
    ref = E.refine_reference(y, inp['rays'], inp['depth'])
    g = lambda a: cu(np.asarray(a, np.float32), dev)
    rays, orr, ds, xg, proj = g(inp['rays']), g(inp['or_rays']), g(inp['depth']), g(x), g(inp['proj'])
    img4 = ops.images_pack(g(inp['img']))
    for variant in variants:
        for shape in shapes:
            refusal = _head_refusal(nb, variant, skips)
            if refusal and skips:                                  # refused when the handle is made, or at the latest by the call
                with pytest.raises(ops.PnrfError, match=refusal):
                    m = pack['mlp'](net, variant)
                    m.set_shape(shape)
                    ops.refine_project_fwd(m, rays[:1], orr[:1], ds[:1], img4, proj, eps=inp['eps'])
                continue
            if skips and shape == 'wide' and nb > 4:               # no wide skip kernel beyond two views per lane half
                with pytest.raises(ops.PnrfError, match='WIDE'):
                    pack['mlp'](net, variant).set_shape(shape)
                continue
            mlp = pack['mlp'](net, variant)
            mlp.set_shape(shape)
            for n in counts:
                tag = f'{what} nb={nb} {variant} {shape} n={n}'
                if refusal:
                    with pytest.raises(ops.PnrfError, match=refusal):
                        ops.refine_project_fwd(mlp, rays[:n], orr[:n], ds[:n], img4, proj, eps=inp['eps'])
                    continue
                a = ops.refine_project_fwd(mlp, rays[:n], orr[:n], ds[:n], img4, proj, eps=inp['eps'])
                b = ops.refine_fwd(mlp, xg[:n], rays[:n], ds[:n])
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag + ': the head and the rows from memory differ'
                ST._check_refine(a, ref, n, tag + ' (head)')
                ST._check_refine(b, ref, n, tag + ' (rows)')


@pytest.mark.parametrize('nb,depth', __import__('exact_nets').REFINE_CONFIGS)
def test_fused_head_exact(dev, nb, depth):
    """pnrf_refine_project_fwd on the integer net of every (num_neighbor, depth), variants default / bf16 / refine_16x16, wide and
    narrow: the projecting head feeds the net the reference's integer colours (per sample, on the moving rays) and Pluecker columns,
    so z and pts equal those of pnrf_refine_fwd on refine_in from memory bit for bit (tests/test_exact_project_cpu.py certifies the
    set, +-1 ulp of both v_rcp_f32 results and of the coordinates included)."""
    from pronerf_amd import ops
    import exact_nets as E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = E.refine_counts(cus, big=(nb, depth) == E.REFINE_BIG)
    Wp, bp = E.refine_pack_weights(E.refine_net(nb, depth))
    pack = dict(mlp=lambda net, variant: ops.PackedMLP(ops.NET_REFINE, Wp, bp, variant=variant), exact=lambda net, x, lim: E.elu_reference(net, x))
    _head_runs(dev, E.refine_net(nb, depth), pack, E.LIM['bf16'], nb, counts, ('default', 'bf16', 'refine_16x16'), ('wide', 'narrow'), False, f'D={depth}')


@pytest.mark.parametrize('nb', [4, 6])
def test_fused_head_exact_with_skips(dev, nb):
    """A net with skip connections (mmnetskips) for two views per lane half (nb = 4) and for three (nb = 6: the shallower fetch
    pipeline, narrow only); every other variant is refused."""
    from pronerf_amd import ops
    import exact_nets as E
    import mmskips_ref as ms
    net = ms.refine_net(nb, 4, [1])
    Wp, bp = ms.refine_pack_weights(net)
    pack = dict(mlp=lambda net, variant: ops.PackedMLP(ops.NET_REFINE, Wp, bp, variant=variant), exact=ms.exact_forward)
    _head_runs(dev, net, pack, E.LIM['f16'], nb, E.refine_counts(0, big=False), ('default', 'bf16', 'refine_16x16'), ('wide', 'narrow'), True, 'skips [1]')
