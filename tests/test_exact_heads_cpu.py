"""CPU: the input sets of tests/exact_heads.py — the exact sets tests/test_exact_heads_gpu.py runs certify (no step of a replay rounds),
the float32 replay equals the certificate there, the float64 oracle lies within the per-element bounds of the float32 replay on the general
sets, the sets hold the edges they claim, and every slipped replay in ``MUTATIONS`` both changes a bit of an exact answer and exceeds the
bound on a general set — so the GPU comparisons can fail."""
import numpy as np
import pytest

import exact_heads as H


@pytest.fixture(scope='module')
def sets():
    e, f, r = H.exact_inputs(), H.exact_inputs(free=True), H.random_inputs()
    return dict(exact=(e, H.forward_state(e)), free=(f, H.forward_state(f)), random=(r, H.forward_state(r)))


def _x0(inp, a):
    """The elements of a posenc output [rows, 3 m] that belong to an x == 0."""
    return np.broadcast_to((inp['x'] == 0)[:, None, :], (a.shape[0], a.shape[1] // 3, 3)).reshape(a.shape)


def test_exact_sets_certify(sets):
    """No output of any head kernel is tainted on the dyadic set, in every option set (pts apart: 0.01f tanh rounds into o + d z; its
    answer is the float32 replay, which the forward's ieee_* operations make exact), and the float32 replay gives the same bits."""
    inp, st = sets['exact']
    for kernel, kw in H.head_cases():
        kwf = dict(kw, **H.saved(kernel, st))
        exp, bad = H.certify(kernel, inp, taint_ok=('pts',), **kwf)
        em = H.emulate(kernel, inp, **kwf)
        for k in exp:
            if k == 'pts':
                assert not bad[k][np.broadcast_to((inp['y35'][:, 8:32] == 0).reshape(-1, 8, 3), bad[k].shape)].any()    # tanh = 0: exact
                np.testing.assert_array_equal(em[k][~bad[k]], exp[k][~bad[k]])
            else:
                np.testing.assert_array_equal(em[k], exp[k], err_msg=f'{kernel} {kw} {k}')
        if kernel == 'sampler_bwd' and not kw['d_rgb']:
            assert (exp['dy'][:, 24:27] == 0).all()
        if kernel == 'refine_bwd' and not kw['d_rgb0']:
            assert (exp['dy'][:, 32:35] == 0).all()


@pytest.mark.parametrize('n_freq', H.PE_FREQS)
def test_posenc_exact_set_certifies_at_zero(n_freq):
    """Every output element of an x == 0 is untainted (sin 0 = 0, cos 0 = 1, the gradient dE[c] + sum 2^k dE[sin_k] exact), the x columns
    of the forward are copies, and the float32 replay agrees on all of them."""
    inp = H.posenc_inputs(n_freq=n_freq, exact=True)
    for kernel in ('posenc_fwd', 'posenc_bwd'):
        k = H.KEYS[kernel][0]
        exp, bad = H.certify(kernel, inp, taint_ok=(k,))
        em = H.emulate(kernel, inp)
        z = _x0(inp, exp[k])
        assert z.mean() > 0.25 and not bad[k][z].any()
        np.testing.assert_array_equal(em[k][~bad[k]], exp[k][~bad[k]])
        if kernel == 'posenc_fwd':
            assert not bad[k][:, :3].any()
            want = np.tile(np.array([0, 1], np.float32), n_freq)                                 # sin_k, cos_k of this coordinate
            assert all((exp[k][r, 3:].reshape(-1, 3)[:, c] == want).all() for r, c in zip(*np.nonzero(inp['x'] == 0)))
        elif n_freq:
            sin_cols = np.stack([inp['dE'][:, 3 + 6 * q:6 + 6 * q] * 2.0 ** q for q in range(n_freq)]).sum(0) + inp['dE'][:, :3]
            np.testing.assert_array_equal(exp[k][z], sin_cols[z].astype(np.float32))


def _u(z, rays):
    near, far = rays[:, 6:7], rays[:, 7:8]
    return z - np.concatenate([z[:, 1:], far], 1), z - np.concatenate([near, z[:, :-1]], 1)      # dir > 0, dir < 0


@pytest.mark.parametrize('which', ['exact', 'free', 'random'])
def test_sets_hold_the_edges(sets, which):
    inp, st = sets[which]
    near, far = inp['rays'][:, 6], inp['rays'][:, 7]
    assert set(np.unique(near)) == {0.0, 0.5, 2.0} and set(np.unique(far - near)) == {1.0, 4.0}
    D = inp['D']
    unsorted = (np.diff(D, axis=1) < 0).any(1)
    assert 0.2 < unsorted.mean() < 0.6
    assert (np.diff(D, axis=1) == 0).any() and (D == near[:, None]).any() and (D == far[:, None]).any()
    for u in _u(st['z_pre'], inp['rays']):                       # both signs and ties, for each jitter direction, with a jitter != 0
        for sel in (u > 0, u < 0, u == 0):
            assert (sel & (inp['jitter'] != 0)).any() and (sel & (inp['jitter'] == 0)).any()
    assert (u[:, 0] == 0).any() and (_u(st['z_pre'], inp['rays'])[0][:, 7] == 0).any()          # ties with near and with far themselves
    assert 0.2 < (inp['jitter'] == 0).mean() < 0.6
    depth = H.emulate('sampler_fwd', inp)['depth']
    tied = (np.diff(depth, axis=1) == 0).any(1)
    assert tied.any() and (st['idx'] != np.arange(8)).any()
    for i in np.flatnonzero(tied)[:20]:                          # tied sort indices: ascending within a run of equal depths (stable)
        for s in range(7):
            assert depth[i, s] < depth[i, s + 1] or st['idx'][i, s] < st['idx'][i, s + 1]
    assert (np.sort(st['idx'], 1) == np.arange(8)).all()
    if which != 'random':
        for y in (inp['y27'][:, :8], inp['y27'][:, 24:], inp['y35']):
            assert set(np.unique(y)) == {-200.0, 0.0, 200.0} and 0.4 < (y == 0).mean() < 0.6
    else:
        for y in (inp['y27'][:, :8], inp['y35']):
            assert (np.abs(y) == 200).any() and (y == 0).any()
        assert H._robust(inp).all()
    # the prefixes the GPU test runs keep the edges from 63 rays on
    for n in (63,):
        assert (u[:n] == 0).any() and unsorted[:n].any() and tied[:n].any()


def test_general_sets_within_bound(sets):
    """The float64 oracle (autograd included) lies within bound_* of the float32 replay on the general set, every element; the replay in
    float64 is the oracle to float64 round-off.  The forward kernels' free set too (its transcendentals are exact: tighter still)."""
    for which, kernels in (('random', None), ('free', ('sampler_fwd', 'refine_fwd'))):
        inp, st = sets[which]
        for kernel, kw in H.head_cases():
            if kernels and kernel not in kernels:
                continue
            kwf = dict(kw, **H.saved(kernel, st))
            ref = H.reference(kernel, inp, **kw)
            val, mag = H.magnitudes(kernel, inp, **kwf)
            for k in ref:
                if k != 'idx':                                   # pts and dy hold the kernels' 0.01f, 0.37 * 2^-24 from the oracle's 0.01
                    tol = 2.0 ** -25 if k in ('pts', 'dy') else 2.0 ** -40
                    assert (np.abs(val[k] - ref[k]) <= tol * mag[k] + 1e-80).all(), (which, kernel, kw, k)
            r = H.ratios(kernel, H.emulate(kernel, inp, **kwf), ref, mag, inp)
            assert max(r.values()) <= 1, (which, kernel, kw, r)


@pytest.mark.parametrize('n_freq', H.PE_FREQS)
def test_posenc_within_bound(n_freq):
    for exact in (True, False):
        inp = H.posenc_inputs(n_freq=n_freq, exact=exact)
        assert np.abs(inp['x']).max() == 1.5 and (inp['x'] == 0).any()
        ref = H.reference_posenc(inp)
        for kernel in ('posenc_fwd', 'posenc_bwd'):
            val, mag = H.magnitudes(kernel, inp)
            k = H.KEYS[kernel][0]
            assert (np.abs(val[k] - ref[k]) <= 2.0 ** -40 * mag[k] + 1e-80).all()
            r = H.ratios(kernel, H.emulate(kernel, inp), ref, mag, inp)
            assert max(r.values()) <= 1, (n_freq, exact, kernel, r)


def test_bound_constants():
    """The ulp assumptions are no larger than the OpenCL full-profile figures (sin, cos 4 ulp; tanh 5 ulp) and expf's 2 ulp of
    exact_composite: in roundings of 2^-24, 8 / 8 / 10 / 4, and the d of each kernel is the chain count of the module docstring."""
    sig, tanh, trig = 4 + 2, 10, 8
    assert H.D_SAMPLER_FWD == sig + 2 and H.D_SAMPLER_BWD == max(2, sig) + 2
    assert H.D_REFINE_FWD == max(max(2, sig) + 2 + 3 + 2, tanh + 1) + 1
    assert H.D_REFINE_BWD == max(tanh + 3, 7 + 3, 7 + 1 + 4)
    assert H.D_POSENC_FWD == trig and H.bound_posenc_bwd(1.0, 16) == H.bound(trig + 2 + 16, 1.0)
    assert H.bound_of('refine_bwd', None, 1.0) == H.bound(H.D_REFINE_BWD, 1.0) and H.bound_of('posenc_bwd', dict(n_freq=4), 1.0) == H.bound(14, 1.0)
    assert np.isclose(H.bound(8, 1.0), 8 * 2.0 ** -24 * (1 + 2.0 ** -10), rtol=1e-12, atol=1e-30)


def _mutated(sets, mutation):
    """('exact' | 'bound', kernel, options) of every comparison of the GPU test that a slipped replay fails."""
    caught = []
    for which in ('exact', 'free', 'random'):
        inp, st = sets[which]
        for kernel, kw in H.head_cases():
            if which == 'free' and kernel not in ('sampler_fwd', 'refine_fwd'):
                continue
            kwf = dict(kw, **H.saved(kernel, st))
            good, em = H.emulate(kernel, inp, **kwf), H.emulate(kernel, inp, mutation=mutation, **kwf)
            if which != 'random':
                if any(not np.array_equal(good[k], em[k]) for k in good):
                    caught.append(('exact', kernel, tuple(kw.items())))
            else:
                _, mag = H.magnitudes(kernel, inp, **kwf)
                if max(H.ratios(kernel, em, H.reference(kernel, inp, **kw), mag, inp).values()) > 1:
                    caught.append(('bound', kernel, tuple(kw.items())))
    for n_freq in (4, 10):
        for exact in (True, False):
            inp = H.posenc_inputs(n_freq=n_freq, exact=exact)
            ref = H.reference_posenc(inp)
            for kernel in ('posenc_fwd', 'posenc_bwd'):
                k = H.KEYS[kernel][0]
                good, em = H.emulate(kernel, inp)[k], H.emulate(kernel, inp, mutation=mutation)[k]
                z = _x0(inp, good)
                if exact and not np.array_equal(good[z], em[z]):
                    caught.append(('exact', kernel, n_freq))
                _, mag = H.magnitudes(kernel, inp)
                if H.ratios(kernel, {k: em}, ref, mag, inp)[k] > 1:
                    caught.append(('bound', kernel, n_freq))
    return caught


@pytest.mark.parametrize('mutation', H.MUTATIONS)
def test_mutation_fails_both_ways(sets, mutation):
    caught = _mutated(sets, mutation)
    assert any(c[0] == 'exact' for c in caught), (mutation, caught)
    assert any(c[0] == 'bound' for c in caught), (mutation, caught)


def test_no_mutation_passes(sets):
    assert not _mutated(sets, None)


def test_generators_are_deterministic_and_nested():
    for f in (H.exact_inputs, H.random_inputs, lambda: H.exact_inputs(free=True), H.posenc_inputs):
        a, b = f(), f()
        assert all(np.array_equal(a[k], b[k]) for k in a)
    a = H.head(H.exact_inputs(), 65)
    assert all(v.shape[0] == 65 for v in a.values())
    t = H.tile(H.exact_inputs(), H.N_CAP)
    assert t['y35'].shape == (H.N_CAP, 35) and np.array_equal(t['y35'][257:514], H.exact_inputs()['y35'])
