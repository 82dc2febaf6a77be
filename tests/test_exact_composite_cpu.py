"""CPU: the compositing input sets of tests/exact_composite.py — every exact-regime set tests/test_exact_composite_gpu.py runs certifies
(the replay of both kernels is exact at every step), the replay computes the oracle's raw2outputs and its autograd, the general regime's
per-element bound holds for a float32 emulation of the kernels, and each slipped emulation in ``MUTATIONS`` fails the exact comparison,
the bound, or both — so the GPU assertions can fail."""
import numpy as np
import pytest

import exact_composite as X


def _equal(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize('S', sorted(set(X.S_BWD) | set(X.S_THREAD)))
def test_exact_sets_certify(S):
    for oi in range(len(X.OPTS)):
        inp = X.exact_case(S, oi)
        exp = X.certify(inp)
        em = X.emulate(inp)                                      # the float32 emulation agrees (the mutations below start from it)
        assert _equal(exp, em), (S, oi, [k for k in exp if not np.array_equal(exp[k], em[k], equal_nan=True)])


@pytest.mark.parametrize('S', [1, 9, 72, 136, 256])
def test_exact_answers_are_the_oracles(S):
    """The certified answers are raw2outputs and its autograd, up to the float64 oracle's own 1e-10 (which fp32 absorbs) and
    exp(-200) != 0.  A ray that composites nothing (acc = 0) has disp = NaN in the oracle (torch.max passes 0 / 0 on)."""
    for oi in range(len(X.OPTS)):
        inp = X.exact_case(S, oi)
        exp, ref = X.certify(inp), X.reference(inp)
        for k in ref:
            assert np.array_equal(np.isnan(exp[k]), np.isnan(ref[k])), (S, oi, k)
            e, r = np.nan_to_num(exp[k].astype(np.float64)), np.nan_to_num(ref[k])
            assert np.abs(e - r).max() <= 1e-7 * max(1.0, np.abs(r).max()), (S, oi, k)


def test_exact_sets_reach_the_edges():
    """sigma == 0, sigma < 0, mul == 0, mul < 0, |raw| == clamp and past it, empty intervals with sigma > 0 on both sides of every chunk
    boundary and before the last sample, d z != 0 there, rays with acc = 0 and rays with several alphas != 0."""
    for S in (72, 136, 256):
        for oi, (am, nz, cl, wh) in enumerate(X.OPTS):
            inp = X.exact_case(S, oi)
            exp = X.certify(inp)
            r3 = np.clip(inp['raw'][..., 3], -cl, cl) if cl else inp['raw'][..., 3]
            sg = r3 + (inp['noise'] if nz else 0) + (inp['add'] if am else 0)
            assert (sg == 0).any() and (sg < 0).any() and (sg > 0).any()
            if am:
                assert (inp['mul'] == 0).any() and (inp['mul'] < 0).any() and (exp['d_mul'] != 0).any()
            if cl:
                assert (np.abs(inp['raw']) == cl).any() and (np.abs(inp['raw']) > cl).any()
            for s in [b for b in range(64, S, 64)] + [S - 1]:
                assert (inp['z'][:, s] == inp['z'][:, s - 1]).all() and (sg[:, s - 1] > 0).all()
                assert (exp['d_z'][:, s] != 0).any(), (S, oi, s)
            for b in range(64, S - 1, 64):
                assert (inp['z'][:, b + 1] == inp['z'][:, b]).all() and (exp['d_z'][:, b + 1] != 0).any()
            assert (exp['acc'] == 0).any() or am
            assert ((exp['w'] != 0).sum(1) >= 2).any() or not am              # without mul alpha = 1: only on the last sample


@pytest.mark.parametrize('S', [1, 2, 8, 65, 72, 200, 256])
def test_replay_is_the_oracle_and_the_bound_holds(S):
    """General regime: the replay in float64 is raw2outputs and its autograd (to float64 round-off), and the float32 emulation of the
    kernels stays within the per-element bound of BOUND_DOC."""
    for oi in range(len(X.OPTS)):
        inp = X.random_case(S, oi)
        ref = X.reference(inp)
        val, mag = X.magnitudes(inp)
        for k in ref:
            assert np.array_equal(np.isnan(val[k]), np.isnan(ref[k])), (S, oi, k)                  # disp of a ray with acc = 0
            ok = np.isnan(ref[k]) | (np.abs(val[k] - ref[k]) <= 2.0 ** -40 * mag[k] * (S + 9) + 1e-300)
            assert ok.all(), (S, oi, k)
        assert not X.check_bound(X.emulate(inp), ref, mag, S, list(ref)), (S, oi)


def test_bound_constants():
    """c = 2, k = 9 of BOUND_DOC: the backward's longest chain is 2 S + E + 14 roundings with E = 4 (expf assumed <= 2 ulp)."""
    E = 4
    for S in X.S_BWD:
        assert 2 * S + E + 14 <= 2 * (S + 9) and S + 13 + E <= 2 * (S + 9)
    assert np.isclose(X.bound(10, 1.0), 2 * 19 * X.U * (1 + 2.0 ** -10), rtol=1e-12, atol=1e-30)


_MUT_S = (72, 136)


@pytest.fixture(scope='module')
def mut_sets():
    out = []
    for S in _MUT_S:
        for oi in range(len(X.OPTS)):
            e, r = X.exact_case(S, oi), X.random_case(S, oi)
            _, mag = X.magnitudes(r)
            out.append((S, oi, e, X.certify(e), r, X.reference(r), mag))
    return out


@pytest.mark.parametrize('mutation', X.MUTATIONS)
def test_mutation_fails(mut_sets, mutation):
    caught = []
    for S, oi, e, exp, r, ref, mag in mut_sets:
        if not _equal(exp, X.emulate(e, mutation)):
            caught.append(('exact', S, oi))
        if X.check_bound(X.emulate(r, mutation), ref, mag, S, list(ref)):
            caught.append(('bound', S, oi))
    assert caught, mutation
    if mutation in ('t_restart', 'q_reset', 'dd_next_dropped', 'partial_stale', 'relu_sigma_at_0', 'last_interval_z', 'd_stride'):
        assert any(c[0] == 'exact' for c in caught), (mutation, caught)       # these the exact comparison catches on its own


def test_generators_are_deterministic():
    for f in (X.exact_case, X.random_case):
        a, b = f(72, 1), f(72, 1)
        assert all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
