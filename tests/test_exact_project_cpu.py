"""CPU: the input sets of tests/exact_project.py — the exact sets tests/test_exact_project_gpu.py runs certify (no step of a replay
rounds, the one absorbed 1e-8f and the mean fill's division apart), the float32 replay equals the certificate there and the float64 run
of the same formulas rounds to the same bits (mean-fill columns: within 2 ulp), the float64 run agrees with the oracle, the sets hold
the edges they claim, and every slipped replay in ``MUTATIONS`` changes a bit of an exact answer — so the GPU comparisons can fail.
The fused head's set: integer refine_in, the +-1 ulp certificate, the nets' certificates, and each slip moving a depth."""
from fractions import Fraction

import numpy as np
import pytest

import exact_project as P

SIZES = (0, 1)


def exact_cases(size):
    """(kernel, input set, replay options) of every exact call the GPU test makes at full size."""
    inf, trn = P.exact_inference(size), P.exact_training(size)
    for nb in P.NBS:
        yield 'refine_input', inf, dict(nb=nb)
    for layout in (0, 1):
        yield 'refine_input_train', trn, dict(layout=layout)
    for kind in ('trt', 'train'):
        full = P.exact_warp(kind, size)
        for B in P.BS_WARP:
            for shared in (False, True):
                yield 'warp_' + kind, P.warp_head(full, B, P.N_SET, shared), {}


@pytest.mark.parametrize('size', SIZES)
def test_exact_sets_certify(size):
    """Every output element of every exact call is untainted, the float32 replay gives the certificate's bits, and the float64 run (with
    the certified absorption of 1e-8f in the training forms' denominator) rounds to the same bits — the mean-fill columns apart, whose
    one division by fl(cnt + 1e-6f) lies within 2 ulp of float64's."""
    for kernel, inp, kw in exact_cases(size):
        exp, bad = P.certify(kernel, inp, **kw)
        em = P.emulate(kernel, inp, **kw)
        np.testing.assert_array_equal(em, exp, err_msg=f'{kernel} {kw}')
        ref = P.run64(kernel, inp, absorb=True, **kw)[0].astype(np.float32)
        fill = P.filled_columns(inp, kw['layout']) if kernel == 'refine_input_train' else np.zeros(em.shape, bool)
        np.testing.assert_array_equal(ref[~fill], em[~fill], err_msg=f'{kernel} {kw} float64')
        assert fill.any() == (kernel == 'refine_input_train') and (P.ulp_distance(ref, em)[fill] <= 2).all(), (kernel, kw)
        assert (em != 0).mean() > 0.15, (kernel, kw)


def _axis_edges(c, size_1, fin):
    """The coordinate classes of one axis (size_1 = Wf - 1 or Hf - 1), each present among the finite samples."""
    c = np.where(fin, c, np.nan)
    with np.errstate(invalid='ignore'):
        return {'integer inside': ((c == np.floor(c)) & (c > 0) & (c < size_1)).any(), 'fraction inside': ((c != np.floor(c)) & (c > 0) & (c < size_1)).any(),
                '== 0': (c == 0).any(), '== size - 1': (c == size_1).any(), 'partial low': ((c > -1) & (c < 0)).any(),
                'partial high': ((c > size_1) & (c < size_1 + 1)).any(), '== -1': (c == -1).any(), '== size': (c == size_1 + 1).any(),
                'outside low': (c < -1).any(), 'outside high': (c > size_1 + 1).any()}


def _corners(X, Y, Hf, Wf, fin):
    return {(cx, cy): (fin & (X == cx) & (Y == cy)).any() for cx in (0, Wf - 1) for cy in (0, Hf - 1)}


@pytest.mark.parametrize('size', SIZES)
def test_inference_set_holds_the_edges(size):
    Hf, Wf = P.SIZES[size]
    inp = P.exact_inference(size)
    a = P.intermediates('refine_input', inp)
    fin = a['fin']
    for name, c, s1 in (('X', a['X'], Wf - 1), ('Y', a['Y'], Hf - 1)):
        e = _axis_edges(c, s1, fin)
        assert all(e.values()), (name, e)
        assert (np.where(fin, c, 0) * 4 == np.round(np.where(fin, c, 0) * 4)).all()          # quarter pixels
    assert all(_corners(a['X'], a['Y'], Hf, Wf, fin).values())
    assert (a['p2'] < 0).any() and (a['p2'] == 0).any() and (a['p2'] > 0).any()
    assert (a['diff'] == 0).any() and (a['diff'] < 0).any()
    assert set(np.unique(a['diff'][a['diff'] > 0])) == {2.0 ** -j for j in range(10)}             # z3d = 2^0 .. 2^9
    assert (~fin).any() and fin.mean() > 0.8
    # non-finite coordinates: zeros for that (view, sample), and only where the set says so (p[2] == 0 or 1 - dn - eps == 0)
    out = P.emulate('refine_input', inp)[:, 48:].reshape(-1, 8, 8, 3)
    assert (out[~fin] == 0).all()
    assert ((~fin) == ((a['p2'] == 0) | (a['diff'] == 0))).all()
    # the first 63 rays (the smallest multi-ray call) already hold partial taps, both signs of p[2] and a non-finite sample
    assert (~fin[:63]).any() and (a['p2'][:63] < 0).any() and ((a['X'][:63] > -1) & (a['X'][:63] < 0)).any()


@pytest.mark.parametrize('size', SIZES)
def test_training_set_holds_the_edges(size):
    Hf, Wf = P.SIZES[size]
    inp = P.exact_training(size)
    a = P.intermediates('refine_input_train', inp)
    fin, inside = a['fin'], a['inside']
    for name, c, s1 in (('X', a['X'], Wf - 1), ('Y', a['Y'], Hf - 1)):
        e = _axis_edges(c, s1, fin)
        assert all(e.values()), (name, e)
    assert all(_corners(a['X'], a['Y'], Hf, Wf, fin & inside).values())
    for c in (a['xn'], a['yn']):                                  # the mask's own boundary: inside
        assert (inside & (c == 1)).any() and (inside & (c == -1)).any()
    with np.errstate(invalid='ignore'):                             # partial taps are masked out in this form
        partial = fin & (((a['X'] > -1) & (a['X'] < 0)) | ((a['X'] > Wf - 1) & (a['X'] < Wf)))
    assert partial.any() and not inside[partial].any()
    out = P.emulate('refine_input_train', inp)
    assert (a['c2z'] < 0).any() and (a['c2z'] > 0).any() and (np.abs(a['c2z'][np.isfinite(a['c2z'])]) >= 0.25).all()
    assert (a['diff'] == 0).any() and (a['diff'] < 0).any()
    ref = inp['ref_nos']
    assert (ref < 0).any() and (ref >= P.NV_TRAIN).any() and (np.sort(ref, 1)[:, 1:] == np.sort(ref, 1)[:, :-1]).any()
    assert set(np.unique(a['cnt'])) == {0.0, 1.0, 2.0, 3.0, 4.0}                                   # samples with 0 .. 4 valid neighbours
    view = np.broadcast_to(P.clamp_views(ref, P.NV_TRAIN)[:, :, None], inside.shape)
    black = inside & fin & (view == P.ZERO_VIEW)
    assert black.any() and (a['vsum'][black] == 0).all() and (a['valid'][black] == 0).all()       # inside, colours sum to exactly 0
    assert (a['valid'][inside & fin & (view != P.ZERO_VIEW)] == 1).all()
    # a filled entry holds the mean: it differs from the sample's own (zero) colour wherever a neighbour is valid
    filled = (a['valid'] == 0) & (a['cnt'] > 0)
    assert filled.any() and (out[:, 48:].reshape(-1, 4, 8, 3)[filled].sum(-1) > 0).all()
    assert (out[:, 48:].reshape(-1, 4, 8, 3)[(a['valid'] == 0) & (a['cnt'] == 0)] == 0).all()


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('kind', ['trt', 'train'])
def test_warp_sets_hold_the_edges(size, kind):
    Hf, Wf = P.SIZES[size]
    full = P.exact_warp(kind, size)
    for shared in (False, True):
        inp = P.warp_head(full, 3, P.N_SET, shared)
        a = P.intermediates('warp_' + kind, inp)
        fin = a['fin']
        for c, s1 in ((a['X'], Wf - 1), (a['Y'], Hf - 1)):
            e = _axis_edges(c, s1, fin)
            assert all(e.values()), e
        assert all(_corners(a['X'], a['Y'], Hf, Wf, fin & a['inside'] if kind == 'train' else fin).values())
        assert (~fin).any() and (P.emulate('warp_' + kind, inp).transpose(0, 2, 1)[~fin] == 0).all()
        if kind == 'train':
            for c in (a['xn'], a['yn']):
                assert (a['inside'] & (c == 1)).any() and (a['inside'] & (c == -1)).any()
            assert (a['c2z'] < 0).any()
        else:
            assert (a['p2'] < 0).any() and (a['p2'] == 0).any()


def general_cases():
    yield 'refine_input', P.general_inference(), {}
    trn = P.general_training()
    for layout in (0, 1):
        yield 'refine_input_train', trn, dict(layout=layout)
    for kind in ('trt', 'train'):
        full = P.general_warp(kind)
        for shared in (False, True):
            yield 'warp_' + kind, P.warp_head(full, 3, P.N_SET, shared), {}


def test_general_sets_within_bound():
    """The float32 replay lies within the per-element bound of the float64 run on the general sets, every element; the float64 run is the
    oracle's statement of the operation to float64 round-off; no normalised coordinate of a training form is within 2^-12 of the mask's
    boundary, and every coordinate is finite (so the bound's first-order model holds)."""
    for kernel, inp, kw in general_cases():
        ref, mag, aux = P.run64(kernel, inp, **kw)
        em = P.emulate(kernel, inp, **kw)
        assert np.isfinite(ref).all() and aux['fin'].all()
        r = P.worst_ratio(em, ref, P.bound(P.D[kernel], mag))
        assert r <= 1, (kernel, kw, r)
        assert 0.2 < (em != 0).mean()
        if kernel in ('refine_input_train', 'warp_train'):
            assert P.margin_ok(aux).all()
            assert aux['inside'].any() and not aux['inside'].all()
        if kernel.startswith('refine') and kw.get('layout', 0) == 0:
            o = P.oracle(kernel, inp)
            assert np.abs(o - ref[:, 48:]).max() <= 1e-11 * np.abs(ref).max(), kernel
        if kernel == 'warp_train' and inp['ro1'].ndim == 2:
            assert np.abs(P.oracle(kernel, inp) - ref).max() <= 1e-11 * np.abs(ref).max()
    inp = P.general_inference()                                    # at Wf = 19 the coordinate round trip is not the identity in fp32
    a = P.intermediates('refine_input', inp)
    assert (a['ix'] != a['X']).any()


@pytest.mark.parametrize('size', SIZES)
def test_oracle_on_the_exact_sets(size):
    """The oracle's project_trt / project_train / warp_train in float64 on the exact sets: the certified answers (inference), within the
    bound (training forms)."""
    inp = P.exact_inference(size)
    np.testing.assert_array_equal(P.oracle('refine_input', inp).astype(np.float32), P.emulate('refine_input', inp)[:, 48:])
    inp = P.exact_training(size)
    ref, mag, _ = P.run64('refine_input_train', inp)
    assert np.abs(P.oracle('refine_input_train', inp) - ref[:, 48:]).max() <= 1e-9 * np.abs(ref).max()
    inp = P.warp_head(P.exact_warp('train', size), 3, P.N_SET, True)
    ref, mag, _ = P.run64('warp_train', inp)
    assert np.abs(P.oracle('warp_train', inp) - ref).max() <= 1e-9 * np.abs(ref).max()


def _nearest_f32(x):
    """The float32 nearest to a Fraction (ties to even), found among the neighbours of its double rounding by exact comparison."""
    r = np.float32(float(x))
    cands = [r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))]
    even = lambda c: (np.float32(c).view(np.uint32) & 1) == 0
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), not even(c)))


def test_fma32_rounds_once():
    """exact_composite.fma32 (the replay's fused multiply-add of unit_dir and cross_rn) against exact rational arithmetic: random
    operands, cancelling operands, and the two cases where the float64 sum hides the bit that decides an fp32 tie."""
    from exact_composite import fma32
    one = np.float32(1 + 2.0 ** -12)
    up, down = fma32(one, one, np.float32(2.0 ** -60)), fma32(one, one, np.float32(-2.0 ** -60))      # 1 + 2^-11 + 2^-24 +- 2^-60
    assert float(up) == 1 + 2.0 ** -11 + 2.0 ** -23 and float(down) == 1 + 2.0 ** -11
    rs = np.random.RandomState(5)
    a, b = rs.randn(400).astype(np.float32), rs.randn(400).astype(np.float32)
    c = np.where(rs.rand(400) < 0.5, -(a.astype(np.float64) * b).astype(np.float32), rs.randn(400) * 2.0 ** rs.randint(-30, 30, 400)).astype(np.float32)
    got = fma32(a, b, c)
    for i in range(400):
        want = _nearest_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (a[i], b[i], c[i], got[i], want)


def test_bound_constants():
    """d of each kernel is the chain count of the module docstring."""
    z3d, w, blend = 3, 2, 6                                        # weight, tap weight, product, three sums
    setup = 2 + 2                                                  # xn (2 X exact, a division, a difference), ix (a sum, a product; / 2 exact)
    assert P.D['refine_input'] == z3d + w + 4 + 1 + setup + blend
    assert P.D['warp_trt'] == w + 4 + 1 + setup + blend
    assert P.D['warp_train'] == w + 4 + 1 + 1 + 3 + setup + blend
    assert P.D['refine_input_train'] == z3d + w + 4 + 1 + 1 + 3 + setup + blend + 4 + 1 + 1
    assert np.isclose(P.bound(8, 1.0), 8 * 2.0 ** -24 * (1 + 2.0 ** -10), rtol=1e-12, atol=1e-30)


# slips the general set cannot see: it keeps off the mask's boundary, its views all face the scene (c2.z > 0), its texels are positive in
# every channel, and its eps = 1e-5 moves a depth of 2 .. 10 by less than the bound allows (the exact sets' eps = 2^-10 is half of their smallest 1 - dn - eps)
EXACT_ONLY = ('inside_strict', 'z_without_abs', 'valid_one_channel', 'eps_dropped')


def _caught(kernel, mutation):
    """Which comparisons of the GPU test a slipped replay fails: 'exact' (a bit of an exact-set answer) and / or 'bound' (the general set)."""
    caught = set()
    for size in SIZES:
        for k, inp, kw in exact_cases(size):
            if k == kernel and not np.array_equal(P.emulate(k, inp, **kw), P.emulate(k, inp, mutation=mutation, **kw)):
                caught.add('exact')
    for k, inp, kw in general_cases():
        if k == kernel:
            ref, mag, _ = P.run64(k, inp, **kw)
            if P.worst_ratio(P.emulate(k, inp, mutation=mutation, **kw), ref, P.bound(P.D[k], mag)) > 1:
                caught.add('bound')
    return caught


@pytest.mark.parametrize('kernel,mutation', [(k, m) for k in P.APPLIES for m in P.APPLIES[k]])
def test_mutation_changes_an_exact_answer(kernel, mutation):
    caught = _caught(kernel, mutation)
    assert 'exact' in caught, (kernel, mutation, caught)
    if mutation not in EXACT_ONLY:
        assert 'bound' in caught, (kernel, mutation, caught)     # the others also exceed the bound on the general set


def test_every_mutation_applies_somewhere():
    assert set(m for ms in P.APPLIES.values() for m in ms) | set(P.HEAD_MUTATIONS) == set(P.MUTATIONS) and len(P.MUTATIONS) == 17
    for kernel in P.APPLIES:
        assert not _caught(kernel, None)


def test_generators_are_deterministic_and_nested():
    for f in (P.exact_inference, P.exact_training, P.general_inference, P.general_training, lambda: P.exact_warp('trt'), lambda: P.general_warp('train')):
        a, b = f(), f()
        assert all(np.array_equal(a[k], b[k]) for k in a)
    a = P.head(P.exact_training(), 9)
    assert a['rays'].shape == (9, 11) and a['ref_nos'].shape == (9, 4) and a['img'].shape[0] == P.NV_TRAIN
    t = P.tile(P.exact_inference(), P.N_INPUT_CAP)
    assert t['depth'].shape == (P.N_INPUT_CAP, 8) and np.array_equal(t['depth'][257:514], P.exact_inference()['depth'])
    w = P.warp_tile(P.warp_head(P.exact_warp('trt'), 3, P.N_SET, False), P.N_WARP_CAP)
    assert w['depth'].shape == (3, P.N_WARP_CAP) and w['ro1'].shape == (3, 4, P.N_WARP_CAP) and 3 * P.N_WARP_CAP > 4096 * 256
    assert P.N_INPUT_CAP > 4096 * 64 and P.N_TRAIN_CAP * 32 > 4096 * 256


# ------------------------------------------------------------------------------------------------ the fused head's set
def _head_case(nb, depth, n):
    import exact_nets as E
    inp = P.head_set(nb, n)
    x = P.head_refine_in(inp)
    assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 2          # refine_in lies in the nets' certified box
    return inp, x.astype(np.float32), E.refine_net(nb, depth)


@pytest.mark.parametrize('nb,depth', __import__('exact_nets').REFINE_CONFIGS)
def test_head_set_certifies(nb, depth):
    """The fused-head set of every net configuration, at the largest count the GPU test runs on a device of up to CU_CERT compute units:
    refine_in of the float64 reference is integer in [0, 2] (Pluecker columns included) and the float32 replay rounds to it; every
    colour survives +-1 ulp on both reciprocals and on both coordinates after rounding to fp16 and to bf16; the net certifies on it (certify_elu)
    and a logit slip moves some depth by more than MARGIN * TOL_Z (refine_margin)."""
    import exact_nets as E
    n = max(E.refine_counts(E.CU_CERT, big=(nb, depth) == E.REFINE_BIG))
    inp, x, net = _head_case(nb, depth, n)
    em = P.emulate('refine_input', inp)                                                 # a moving ray's 2 (w00 + .. + w11) rounds in fp32
    assert np.array_equal(np.round(em), x) and np.abs(em - x).max() <= 2.0 ** -20
    col = P.head_certificate(inp)
    assert set(np.unique(col)) == {0.0, 1.0, 2.0} and set(np.unique(x[:, :48])) == {0.0, 1.0, 2.0}
    # moving rays: a third of the set at least; their colours change along the ray, and not symmetrically under s -> 7 - s, within
    # the first 127 rays already (the smallest count with more than one ray)
    moving = inp['or_rays'][:, 5] != 0
    varies, skew = (col != col[:, :, :1]).any((1, 2, 3)), (col != col[:, :, ::-1]).any((1, 2, 3))
    assert moving.mean() > 0.33 and not varies[~moving].any() and varies.mean() > 0.15 and skew.mean() > 0.15
    assert skew[:127].sum() >= 8
    for k, view in enumerate(P.HEAD_VIEWS[:nb]):
        assert (col[:, k] != col[:, k, :1]).any() == bool(view[5])                         # every view that sees w_z shows it
    a = P.intermediates('refine_input', inp)
    assert (a['X'] != np.floor(a['X'])).any() and (a['Y'] != np.floor(a['Y'])).any() and (a['X'] < 0).any() and (a['X'] > P.HEAD_SIZE[1] - 1).any()
    assert set(np.unique(a['p2'])) == {v[4] for v in P.HEAD_VIEWS[:nb]}                 # the reciprocals the head takes: of powers of two
    y = E.certify_elu(net, x, E.LIM['bf16'])
    E.assert_refine_margin(y, inp['rays'], inp['depth'])


@pytest.mark.parametrize('mutation', P.HEAD_MUTATIONS)
def test_head_mutation_moves_a_depth(mutation):
    """Each slip, applied to the reference's refine_in of the fused-head set, moves some z by more than MARGIN * TOL_Z on at least one
    net configuration (head_padding_weight: on every odd nb, where a lane half holds a padding view; sample_reversed: on both
    configurations the skip nets share their sets with, nb = 4 and 6)."""
    import exact_nets as E
    moved = {}
    for nb, depth in E.REFINE_CONFIGS:
        if mutation == 'head_padding_weight' and nb % 2 == 0:
            continue
        inp, x, net = _head_case(nb, depth, 257)
        z = E.refine_reference(E.elu_reference(net, x), inp['rays'], inp['depth'])[0]
        zm = E.refine_reference(E.elu_reference(net, P.head_refine_in(inp, mutation)), inp['rays'], inp['depth'])[0]
        moved[nb] = float(np.abs(zm - z).max())
    lim = E.MARGIN * E.TOL_Z
    assert max(moved.values()) > lim, (mutation, moved)
    if mutation == 'head_padding_weight':
        assert min(moved.values()) > lim, (mutation, moved)
    if mutation == 'sample_reversed':
        assert moved[4] > lim and moved[6] > lim, (mutation, moved)
