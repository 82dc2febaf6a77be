"""CPU: certificate of what tests/test_exact_sampler_gpu.py runs (tests/exact_sampler.py) — no kernel runs here.

1. Exactness: every net x input population passes the layer walk of ``exact_sampler.exact_forward`` (integers representable in the planes that carry them,
   ELU pre-activations >= 0, sums of |terms| < 2^24, pass 1's scaled skip layers < 2^24 / 2^11, equal to the oracle's float64 forward), and the families
   do what they are for: x_big inputs have lo planes of both signs, hid_big activations need theirs in every layer.
2. Tolerance: B (the unmutated replay against the integers, plus an fp32 ulp of the output) is what exact_sampler.B_TABLE records; T = 4 B <= 1/8.
3. Mutations: every applicable one-slip variant of the replay moves some add / mul of some ray by >= 1 - T on the family built to catch it, and by nothing
   (P_lo slips: exactly 0; the others: the pre-images' residuals, < 1e-4, so that the mutated replay still passes) on the integer sets the suite had
   before (mmskips_ref.sampler_scaled_net on sampler_rays): the gap these tests close.
4. Flags: twopass_ref's always-flagged mask of the pass-2 list test is the chosen subset, nobody else is flagged at kappa = 0; on every other ray set
   pass 1 flags nobody at any kappa (the depth rows carry no weights: M = 0).
"""
import numpy as np
import pytest

import exact_nets as en
import exact_sampler as xs
import mmskips_ref as ms
import twopass_ref as tp

CONFIGS = [(D, ()) for D in xs.DEPTHS] + list(xs.SKIP_NETS)
CASES = [(f, D, sk) for f in xs.FAMILIES for D, sk in CONFIGS]


@pytest.mark.parametrize('family,D,skips', CASES)
def test_exactness(family, D, skips):
    net = xs.net_for(D, skips, family)
    assert ms.skips_of(net['W']) == list(skips) and net['W'][0].shape == (256, 288)
    rays = xs.population(family)
    x6 = xs.x6_of(rays)
    np.testing.assert_array_equal(tp.pluecker32(rays), x6)                  # the kernels' fp32 Pluecker vector is these integers
    y = xs.exact_forward(net, x6, xs.KERNELS[family])
    assert np.array_equal(np.argsort(y[0, :8], kind='stable'), xs.order_of(net)) and np.all(y[:, :8] == y[0, :8]) and np.abs(y[:, :8]).max() <= 4
    assert np.all((net['W'][-1][8:24] != 0).sum(0) == 1) and np.all(net['W'][-1][:8] == 0)      # every last-layer unit read once by add / mul; M = 0
    # exact_rows (what the GPU tests index) draws every ray's answer from this population
    big = xs.rays_for(family, 300, seed=1)
    pop = {tuple(r): i for i, r in enumerate(x6)}
    np.testing.assert_array_equal(xs.exact_rows(net, big), y[[pop[tuple(r)] for r in xs.x6_of(big)]])
    lo_in = xs._split(x6)[1]
    if family == 'x_big':
        assert {-2048.0, 0.0, 2048.0} == set(np.unique(lo_in[:, 3])) == set(np.unique(lo_in[:, 4]))
        assert any(abs(w) > 2048 for w in np.unique(net['W'][0]))          # a first-layer weight whose own lo plane is +-2048
    else:
        assert not lo_in.any()
    if family == 'hid_big':                                                # every hidden layer has units in [2048, 4096] whose lo plane is not 0
        h = np.tile(x6, (1, xs.P))
        for l in range(D):
            a = h @ net['W'][l].T + net['b'][l]
            bigs = a[:, a.min(0) >= 2048]
            assert bigs.shape[1] >= 64 and bigs.max() <= 4096 + xs.WIDTH_CAP + 2 and np.count_nonzero(xs._split(bigs)[1]) > 0, (l, bigs.shape)
            h = np.concatenate([np.tile(x6, (1, xs.P)), a], 1) if l in skips else a


def test_tolerance_table():
    """B per net, family and replay, printed; the recorded table is the measured one; T <= 1/8."""
    keys = set()
    for family, D, skips in CASES:
        net = xs.net_for(D, skips, family)
        for kind in xs.KERNELS[family]:
            B = xs.measure_bound(net, kind)
            key = (family, kind, D, tuple(skips))
            keys.add(key)
            print(f'\n[exact_sampler] {family:8s} {kind:3s} D {D} skips {list(skips)}: B = {B:.3g}, T = {4 * B:.3g}', end='')
            assert xs.B_TABLE[key] == xs.up2(B), (key, B)
            assert xs.tol(*key) <= xs.T_MAX
    assert keys == set(xs.B_TABLE)


@pytest.mark.parametrize('family,D,skips', [c for c in CASES if c[0] != 'small'])
def test_mutations_are_caught(family, D, skips):
    """x_big catches the P_lo mutations (both replays), hid_big the X_lo' mutations (the split kernel's replay); the 2^-10 slip is caught by both."""
    net = xs.net_for(D, skips, family)
    rays = xs.population(family)
    Wp, bp = xs.pack_scaled(net)
    for kind in xs.KERNELS[family]:
        base = xs.replay(kind, Wp, bp, rays)
        T = xs.tol(family, kind, D, skips)
        for mut in xs.MUTATIONS:
            mine = (mut in xs.PLO_MUTATIONS) if family == 'x_big' else (mut.startswith('Xlo_') or mut == 'lo_scale')
            if not (mine and xs.applies(mut, kind, D, skips)):
                continue
            moved = float(np.abs(xs.replay(kind, Wp, bp, rays, mut)[:, 8:24] - base[:, 8:24]).max())
            assert moved >= 1 - T, (family, kind, D, skips, mut, moved)


@pytest.mark.parametrize('D,skips', [(D, tuple(sk)) for D, sets in ms.SKIP_SETS.items() for sk in sets])
def test_mutations_are_invisible_on_the_earlier_sets(D, skips):
    """The integer sets of tests/test_mmskips_gpu.py (inputs in [0, 2], activations below 2048): every lo plane of an input or an activation is 0, so no
    mutation moves anything — what those tests could not see.  The replay itself agrees with the bound those tests hold the kernels to."""
    net = ms.sampler_scaled_net(D, list(skips))
    Wp, bp = ms.sampler_pack_weights(net)
    rays = ms.sampler_rays(257, seed=D)
    y = ms.exact_forward(net, ms.sampler_inputs(rays, 1), en.LIM['f16'])
    for kind in ('p1', 'h16'):
        base = xs.replay(kind, Wp, bp, rays)
        assert np.abs(base[:, 8:24] - y[:, 8:24]).max() <= ms.SCALED_TOL and np.array_equal(base[:, :8], y[:, :8])
        for mut in xs.MUTATIONS:
            if xs.applies(mut, kind, D, skips):
                got = xs.replay(kind, Wp, bp, rays, mut)
                # what a slip can move there is the pre-images' residuals (integer + 1e-6 has a lo plane of 2e-3): the mutated replay passes those tests
                assert np.abs(got - base).max() < 1e-4, (kind, mut)
                assert np.abs(got[:, 8:24] - y[:, 8:24]).max() <= ms.SCALED_TOL and np.array_equal(got[:, :8], y[:, :8]), (kind, mut)
                if mut.startswith('Plo') and mut != 'Plo_in_Wlo' or mut == 'skip_Plo_drop':
                    assert np.array_equal(got, base), (kind, mut)                  # P_lo is exactly 0


def test_flags():
    net = xs.net_for(6, (), 'x_big')
    Wp, bp = xs.pack_scaled(net)
    for size in xs.LIST_SIZES:
        sub = xs.flag_subset(size)
        assert len(sub) == size == len(set(sub.tolist())) and (size == 0 or (0 <= sub.min() and sub.max() < xs.LIST_N))
        rays = xs.rays_for('x_big', xs.LIST_N, same=sub)
        ck = tp.emulated(Wp, bp, (), rays)[3]
        mask = np.zeros(xs.LIST_N, bool); mask[sub] = True
        assert np.array_equal(ck['always'], mask) and np.all(ck['kappa'][~mask] > 0), size
    subs = [set(xs.flag_subset(s).tolist()) for s in xs.LIST_SIZES]
    assert any(0 in s for s in subs) and any(xs.LIST_N - 1 in s for s in subs) and any(0 not in s for s in subs[1:])
    for family, D, skips in CASES:                 # every other set: nobody is flagged at any kappa, so the default call's rows are pass 1's
        if 'p1' in xs.KERNELS[family]:
            ck = tp.emulated(*xs.pack_scaled(xs.net_for(D, skips, family)), tuple(skips), xs.population(family))[3]
            assert not ck['always'].any() and np.all(ck['kappa'] == np.inf), (family, D, skips)
