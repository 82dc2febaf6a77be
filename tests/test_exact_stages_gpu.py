"""GPU: every MLP engine of the render path on integer nets (tests/exact_nets.py), where the answer is exact.

The stage tests elsewhere hold the reduced-precision engines to loose bounds against the fp32 oracle, and to each other; a packing slip
that all kernels reading a stream share (a K tail, a bias slot of one column block) could hide under those bounds.  Here every operand
is an integer representable in the operand type and every partial sum stays below 2^24, so the MLP output must equal the oracle's
float64 forward bit for bit (``assert_array_equal``), in every variant and workgroup shape, at the ray counts where batching changes.
Downstream arithmetic (compositing, sigmoid / tanh heads, interval refinement) is compared within stated fp32 bounds.  A mutation check
per engine re-packs the weights with one entry changed by +1 and asserts that the same comparison then fails.

Bounds (2^-24 = one rounding of a value in [0.5, 1)):
  * refine z: sigmoid_fast (v_exp, add, v_rcp: <= 3 roundings relative) scaled by an interval width <= 0.25, plus five roundings of
    values <= 1 (two midpoints, the width, the product, the sum): < 4 x 2^-24; TOL_Z = 2^-20 keeps a factor 4.
  * refine pts = o + d z + 0.01 tanh(offset) with |o|, |d| <= 1, |pts| < 4: |d| TOL_Z + three roundings at ulp(4) / 2 = 2^-22 + tanh_fast's
    few 2^-24 times 0.01: < 2^-19; TOL_PTS = 2^-18.
  * rgb0 = sigmoid(y) through expf and an IEEE division: <= 3 roundings of a value < 1: TOL_RGB0 = 2^-21.
  * rgbd (compositing of the exact raw): per sample sigmoid_fast (3 roundings), alpha = (1 - exp) * relu(mul) (4), 1 - alpha + 1e-10
    (2), the transmittance as a product of up to 7 such factors (2 each), the weight and its product with the colour / depth (2), and a
    tree sum of 8 terms (3): about 30 roundings per sample of values <= 1.5, 8 samples of weights summing to <= 1: the first-order
    bound stays under 64 x 2^-24 = 2^-18; TOL_RGBD = 2^-17.
"""
import numpy as np
import pytest
import torch

import exact_nets as E

pytestmark = pytest.mark.gpu

TOL_Z, TOL_PTS, TOL_RGB0, TOL_RGBD = E.TOL_Z, 2.0 ** -18, 2.0 ** -21, 2.0 ** -17
SHAPES = ('wide', 'narrow', 'auto')


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ----------------------------------------------------------------------------------------------- NeRF stage
def _nerf_pack(kind, w, variant='default', shape=None):
    from pronerf_amd import ops
    if kind == 'nerf':
        m = ops.PackedMLP(ops.NET_NERF, w['W'], w['b'], variant=variant)
    else:
        Ws, bs = E.nerfcls_pack_order(w)
        m = ops.PackedMLP(ops.NET_NERFCLS, Ws, bs, variant=variant)
    if shape is not None:
        m.set_shape(shape)
    return m


def _nerf_case(kind, w, n, cus, dev, live=None, S=8):
    """Inputs (on the device), exact raw and fp64 compositing of the first n rays of the certified set."""
    inp = E.nerf_inputs(max(n, max(E.nerf_counts(E.CU_CERT))) if S == 8 else n, live=live, n_samples=S)
    if cus > E.CU_CERT and S == 8:               # a device larger than the CPU test certified for: certify here
        raw = E.certify_nerf(kind, w, inp)
    else:
        raw = E.nerf_reference(kind, w, inp)
    assert np.all(raw == np.round(raw)) and np.abs(raw).max() < E.ACC_MAX
    from oracle import pronerf_oracle as orc
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    rgb, _, _, _, depth = orc.raw2outputs(t(raw), t(inp['z']), t(inp['rays'][:, 3:6]), t(inp['add']), t(inp['mul']))
    ref_rgbd = np.concatenate([rgb.numpy(), depth.numpy()[:, None]], 1)
    g = {k: _g(v, dev) for k, v in inp.items()}
    return g, raw.astype(np.float32), ref_rgbd


def _check_nerf(mlp, g, raw, ref_rgbd, n, what):
    from pronerf_amd import ops
    rgbd, got = ops.nerf_fwd(mlp, g['pts'][:n], g['rays'][:n], g['z'][:n], g['add'][:n], g['mul'][:n], want_raw=True)
    np.testing.assert_array_equal(got.cpu().numpy(), raw[:n], err_msg=what)
    err = np.abs(rgbd.cpu().numpy().astype(np.float64) - ref_rgbd[:n]).max()
    assert err <= TOL_RGBD, f'{what}: rgbd off by {err:.3g} > {TOL_RGBD:.3g}'


def _nerf_runs(kind, depth):
    """(variant, shape) pairs: the two-shape engines in wide / narrow / auto, the single-shape ones once."""
    runs = [(v, s) for v in ('default', 'f16') for s in SHAPES] + [('nerf_4x64', None)]
    if kind == 'nerfcls' or depth == 8:
        runs.append(('bf16_32x32', None))
    return runs


@pytest.mark.parametrize('kind,depth', [('nerf', d) for d in E.NERF_DEPTHS] + [('nerfcls', 8)])
def test_nerf_stage_exact(dev, cus, kind, depth):
    """pnrf_nerf_fwd, want_raw: raw bit for bit at every boundary ray count, every variant and shape; rgbd within TOL_RGBD."""
    w = E.nerf_net(depth) if kind == 'nerf' else E.nerfcls_net()
    counts = E.nerf_counts(cus)
    g, raw, ref_rgbd = _nerf_case(kind, w, max(counts), cus, dev)
    for variant, shape in _nerf_runs(kind, depth):
        mlp = _nerf_pack(kind, w, variant, shape)
        for n in counts:
            _check_nerf(mlp, g, raw, ref_rgbd, n, f'{kind} D={depth} {variant} {shape} n={n}')


@pytest.mark.parametrize('live', [0, 1, 2])
def test_nerf_stage_exact_sincos(dev, cus, live):
    """The sin / cos columns of one coordinate carry weight; that coordinate is 0 in every sample and view direction (sin 0 = 0, cos 0 = 1)."""
    counts = [1, 33, 16 * cus + 1]
    for kind, depth in (('nerf', 8), ('nerf', 3 + live), ('nerfcls', 8)):
        w = E.nerf_net(depth, live=live) if kind == 'nerf' else E.nerfcls_net(live=live)
        g, raw, ref_rgbd = _nerf_case(kind, w, max(counts), cus, dev, live=live)
        for variant, shape in [('default', 'wide'), ('default', 'narrow'), ('f16', 'wide'), ('f16', 'narrow'), ('nerf_4x64', None)]:
            mlp = _nerf_pack(kind, w, variant, shape)
            for n in counts:
                _check_nerf(mlp, g, raw, ref_rgbd, n, f'{kind} D={depth} live={live} {variant} {shape} n={n}')


@pytest.mark.parametrize('S', [8, 16, 64])
@pytest.mark.parametrize('kind', ['nerf', 'nerfcls'])
def test_nerf_train_stage_exact(dev, cus, kind, S):
    """pnrf_nerf_train_fwd: S = 8 fused (raw and rgbd), S = 16 / 64 raw only."""
    from pronerf_amd import ops
    w = E.nerf_net(8) if kind == 'nerf' else E.nerfcls_net()
    n = 33
    g, raw, ref_rgbd = _nerf_case(kind, w, n, cus, dev, S=S)
    for variant, shape in [('default', 'wide'), ('default', 'narrow'), ('f16', 'auto'), ('nerf_4x64', None)]:
        mlp = _nerf_pack(kind, w, variant, shape)
        for m in (1, 17, 33):
            rgbd, got = ops.nerf_train_fwd(mlp, g['pts'][:m], g['rays'][:m], g['z'][:m], g['add'][:m], g['mul'][:m], want_raw=True)
            what = f'{kind} S={S} {variant} {shape} n={m}'
            np.testing.assert_array_equal(got.cpu().numpy(), raw[:m], err_msg=what)
            if S == 8:
                err = np.abs(rgbd.cpu().numpy().astype(np.float64) - ref_rgbd[:m]).max()
                assert err <= TOL_RGBD, f'{what}: rgbd off by {err:.3g}'
            else:
                assert rgbd is None


# ----------------------------------------------------------------------------------------------- refine stage
def _refine_pack(net, variant='default', shape=None):
    from pronerf_amd import ops
    Wp, bp = E.refine_pack_weights(net)
    m = ops.PackedMLP(ops.NET_REFINE, Wp, bp, variant=variant)
    if shape is not None:
        m.set_shape(shape)
    return m


def _refine_case(nb, depth, n, dev):
    net = E.refine_net(nb, depth)
    x = E.elu_inputs(n, 48 + 24 * nb)
    y = E.elu_reference(net, x)
    assert np.all(y == np.round(y))
    rays, ds = E.refine_rays(n)
    z, pts, rgb0 = E.refine_reference(y, rays, ds)
    return net, (_g(x, dev), _g(rays, dev), _g(ds, dev)), (z, pts, rgb0)


def _check_refine(out, ref, n, what):
    for name, got, want, tol in zip(('z', 'pts', 'rgb0'), out, ref, (TOL_Z, TOL_PTS, TOL_RGB0)):
        if got is None:
            continue
        err = np.abs(got.cpu().numpy().astype(np.float64) - want[:n]).max()
        assert err <= tol, f'{what}: {name} off by {err:.3g} > {tol:.3g}'


@pytest.mark.parametrize('nb,depth', E.REFINE_CONFIGS)
def test_refine_stage_exact(dev, cus, nb, depth):
    """pnrf_refine_fwd: z, pts against interval_refine(sigmoid(exact logits)) in fp64, every variant and shape."""
    from pronerf_amd import ops
    big = (nb, depth) == E.REFINE_BIG
    counts = E.refine_counts(cus, big=big)
    n_set = max(E.refine_counts(E.CU_CERT, big=big))
    if max(counts) > n_set:                      # a device larger than the CPU test certified for: certify here
        n_set = max(counts)
        E.certify_elu(E.refine_net(nb, depth), E.elu_inputs(n_set, 48 + 24 * nb), E.LIM['bf16'])
    net, (x, rays, ds), ref = _refine_case(nb, depth, n_set, dev)
    for variant in ('default', 'bf16', 'refine_16x16'):
        for shape in SHAPES:
            mlp = _refine_pack(net, variant, shape)
            for n in counts:
                _check_refine(ops.refine_fwd(mlp, x[:n], rays[:n], ds[:n]), ref, n, f'refine nb={nb} D={depth} {variant} {shape} n={n}')


def test_refine_train_stage_exact(dev, cus):
    """pnrf_refine_train_fwd without jitter (num_neighbor 4, its only width): z, pts and the rgb0 head."""
    from pronerf_amd import ops
    nb, depth = E.REFINE_BIG
    n_set = max(E.refine_counts(E.CU_CERT, big=False))
    net, (x, rays, ds), ref = _refine_case(nb, depth, n_set, dev)
    for variant in ('default', 'bf16'):
        for shape in SHAPES:
            mlp = _refine_pack(net, variant, shape)
            for n in E.refine_counts(cus, big=False):
                _check_refine(ops.refine_train_fwd(mlp, x[:n], rays[:n], ds[:n], jitter=None), ref, n, f'refine_train {variant} {shape} n={n}')


# ----------------------------------------------------------------------------------------------- module level (pnrf_mlp_fwd)
def test_mlp_fwd_exact(dev):
    """pnrf_mlp_fwd, head_act = 0: the sampler (exact fp32), refine nb 1..8 (fp16, bf16), the NeRF class and DoNeRFTRT, bit for bit."""
    from pronerf_amd import ops
    m_max = max(E.MLP_COUNTS)
    net = E.sampler_net()
    x = E.elu_inputs(m_max, 288)
    y = E.elu_reference(net, x).astype(np.float32)
    mlp = ops.PackedMLP(ops.NET_SAMPLER, [np.float32(W) for W in net['W']], [np.float32(b) for b in net['b']])
    xg = _g(x, dev)
    for m in E.MLP_COUNTS:
        np.testing.assert_array_equal(mlp.forward(xg[:m]).cpu().numpy(), y[:m], err_msg=f'sampler m={m}')
    for nb, depth in E.REFINE_CONFIGS:
        net = E.refine_net(nb, depth)
        x = E.elu_inputs(m_max, 48 + 24 * nb)
        y = E.elu_reference(net, x).astype(np.float32)
        xg = _g(x, dev)
        for variant in ('default', 'bf16'):
            mlp = _refine_pack(net, variant)
            for m in E.MLP_COUNTS:
                np.testing.assert_array_equal(mlp.forward(xg[:m]).cpu().numpy(), y[:m], err_msg=f'refine nb={nb} D={depth} {variant} m={m}')
    inp = E.nerf_inputs(m_max, n_samples=1)
    e, ev = (_g(t.numpy(), dev) for t in E.nerf_embed(inp))
    for kind, w in (('nerf', E.nerf_net(8)), ('nerfcls', E.nerfcls_net())):
        raw = E.nerf_reference(kind, w, inp).reshape(m_max, 4).astype(np.float32)
        mlp = _nerf_pack(kind, w)
        for m in E.MLP_COUNTS:
            np.testing.assert_array_equal(mlp.forward(e[:m], ev[:m]).cpu().numpy(), raw[:m], err_msg=f'{kind} m={m}')


# ----------------------------------------------------------------------------------------------- mutation self-check
def _visible_mutation(w_list, layer, changes):
    """The first +1 mutation of ``layer`` (E.mutate, seeds 0, 1, ...) whose effect reaches the compared outputs in the fp64 reference (an
    entry that only meets zero operands, or a unit ReLU switches off, changes nothing there)."""
    for seed in range(32):
        Wm, where = E.mutate(w_list, layer, seed)
        if changes(Wm):
            return Wm
    raise AssertionError(f'no visible +1 mutation in layer {layer}')


def _mutated_nerf(kind, w, layer, inp):
    def build(Ws):
        if kind == 'nerf':
            return {'W': Ws, 'b': w['b']}
        bs = E.nerfcls_pack_order(w)[1]
        out = {'pts_linears': list(zip(Ws[:8], bs[:8]))}
        for i, k in enumerate(('feature_linear', 'alpha_linear', 'views_linears', 'rgb_linear')):
            out[k] = [(Ws[8 + i], bs[8 + i])] if k == 'views_linears' else (Ws[8 + i], bs[8 + i])
        return out
    Ws = w['W'] if kind == 'nerf' else E.nerfcls_pack_order(w)[0]
    ref = E.nerf_reference(kind, w, inp)
    return build(_visible_mutation(Ws, layer, lambda Wm: not np.array_equal(E.nerf_reference(kind, build(Wm), inp), ref)))


@pytest.mark.parametrize('kind,variant,shape,layer', [
    ('nerf', 'default', 'wide', 3), ('nerf', 'default', 'narrow', 0), ('nerf', 'f16', 'wide', 7), ('nerf', 'nerf_4x64', None, 5),
    ('nerf', 'bf16_32x32', None, 2), ('nerfcls', 'default', 'wide', 5), ('nerfcls', 'f16', 'narrow', 10), ('nerfcls', 'nerf_4x64', None, 9),
    ('nerfcls', 'bf16_32x32', None, 8)])
def test_mutation_nerf(dev, cus, kind, variant, shape, layer):
    """One weight +1, re-packed: the unchanged exact reference must no longer match (the comparison can fail)."""
    w = E.nerf_net(8) if kind == 'nerf' else E.nerfcls_net()
    g, raw, ref_rgbd = _nerf_case(kind, w, 33, cus, dev)
    _check_nerf(_nerf_pack(kind, w, variant, shape), g, raw, ref_rgbd, 33, 'unmutated')
    inp = {k: v[:33] for k, v in E.nerf_inputs(max(E.nerf_counts(E.CU_CERT))).items()}
    with pytest.raises(AssertionError):
        _check_nerf(_nerf_pack(kind, _mutated_nerf(kind, w, layer, inp), variant, shape), g, raw, ref_rgbd, 33, 'mutated')


@pytest.mark.parametrize('variant,shape,layer,api', [
    ('default', 'wide', 0, 'fwd'), ('bf16', 'narrow', 3, 'fwd'), ('refine_16x16', 'wide', 6, 'fwd'), ('refine_16x16', 'narrow', 1, 'fwd'),
    ('default', 'wide', 2, 'train'), ('default', None, 4, 'mlp'), ('bf16', None, 6, 'mlp')])
def test_mutation_refine(dev, variant, shape, layer, api):
    from pronerf_amd import ops
    nb, depth = E.REFINE_BIG
    n = 257
    net, (x, rays, ds), ref = _refine_case(nb, depth, n, dev)
    y = E.elu_reference(net, E.elu_inputs(n, 48 + 24 * nb)).astype(np.float32)
    # the logits the compared outputs are sensitive to: z / pts read y[0:32] within ranges where a slip of 1 exceeds the bounds (rgb0's
    # logits read every unit and mostly saturate the sigmoid: a slip there is only certain to show in the module-level output)
    cols = slice(0, 35) if api == 'mlp' else slice(0, 32)
    xs = E.elu_inputs(n, 48 + 24 * nb)
    Wm = _visible_mutation(net['W'], layer, lambda Wm: not np.array_equal(E.elu_reference({'W': Wm, 'b': net['b']}, xs)[:, cols], y[:, cols]))
    bad = {'W': Wm, 'b': net['b']}

    def check(mlp):
        if api == 'fwd':
            _check_refine(ops.refine_fwd(mlp, x, rays, ds), ref, n, 'refine_fwd')
        elif api == 'train':
            _check_refine(ops.refine_train_fwd(mlp, x, rays, ds, jitter=None), ref, n, 'refine_train_fwd')
        else:
            np.testing.assert_array_equal(mlp.forward(x).cpu().numpy(), y)
    check(_refine_pack(net, variant, shape))
    with pytest.raises(AssertionError):
        check(_refine_pack(bad, variant, shape))


def test_mutation_sampler(dev):
    from pronerf_amd import ops
    net = E.sampler_net()
    x = E.elu_inputs(129, 288)
    y = E.elu_reference(net, x).astype(np.float32)
    Wm = _visible_mutation(net['W'], 2, lambda Wm: not np.array_equal(E.elu_reference({'W': Wm, 'b': net['b']}, x), y))
    xg = _g(x, dev)
    good = ops.PackedMLP(ops.NET_SAMPLER, [np.float32(W) for W in net['W']], [np.float32(b) for b in net['b']])
    np.testing.assert_array_equal(good.forward(xg).cpu().numpy(), y)
    bad = ops.PackedMLP(ops.NET_SAMPLER, [np.float32(W) for W in Wm], [np.float32(b) for b in net['b']])
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(bad.forward(xg).cpu().numpy(), y)
