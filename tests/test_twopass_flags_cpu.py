"""CPU: the restatement of the two-pass sampler's per-ray decision (tests/twopass_ref.py) held to the older CPU model, its own rounding measured, and the
teeth of the GPU comparison (tests/test_twopass_flags_gpu.py) shown on one-slip mutations of it.

Tolerance.  kappa* of every ray of every case in float64 and in float32 arithmetic (same code, same depths): worst relative difference inside the
scanned range 3.19e-5 (d6_x4; 7e-6 .. 1.1e-5 on the other sets) -> DELTA = 4 x that, rounded up = 1.4e-4.  The factor 4: the kernel sums in a third order and
forms its first layer from split fp16 planes (2^-22 per product against 2^-24 of a float32 sum), so a few more fp16 roundings of activations flip; each
flip moves one of 256 terms of one S_l by 2^-11.  DELTA is 0.014 %, far below the 0.5 % at which the restatement would be too loose to use.

Grid.  The scan's step G = 2^(1/2048) - 1 = 3.4e-4.  A step of 2^(1/128) (5.4e-3) would be too coarse for two mutations: a missing last-layer term moves
kappa* by 0.17 % (depth 9) .. 0.5 % on the deep signal-preserving nets, where C_l = 2.3 per layer makes the early layers' terms 2.3^L times the last one's,
and per-depth M_k by 0.55 .. 1.5 % (the eight rows' largest weights are within 3 % of each other).  Smallest move at the 10 % quantile: 0.166 % against
2 (DELTA + G) = 0.096 %.

Against tools/sampler_twopass_model.py.  That model works at true scale, the kernel on the log2(e) scale: every fp16 rounding of an activation falls
differently (each <= 2^-11, zero mean), which moves S_l by up to 7e-4 and s by up to 1.7e-4 (measured on the five sets) — the two cannot agree to
float64 noise.  Held to 5e-4: s_new / s_old = sqrt(max M / M_k) per depth row, i.e. never below, and equal with the per-depth-M mutation.

`>=` in place of `>` changes the flag only where a gap EQUALS its threshold.  That is constructible for gap = threshold = 0 alone (tied logits on a ray
with near = far), and there the comparison is not finite either, so the kernel's combined flag cannot separate the two; the mutation is pinned at the
level of the gap rule (twopass_ref's 'gap' reason), and the GPU test requires those rays flagged.
"""
import os
import sys

import numpy as np
import pytest
import torch

import twopass_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MEASURED = 3.19e-5      # worst |kappa*_f32 / kappa*_f64 - 1| inside the scanned range, all cases
DELTA = R.DELTA         # 1.4e-4 = 4 x MEASURED, rounded up
SCAN_CASES = [c for c in R.CASES if c not in R.OUT_OF_RANGE]


def test_delta_is_four_times_the_reference_rounding():
    worst = {}
    for name in R.CASES:
        W, b, skips, rays = R.case(name)
        p1, z, idx, ck = R.emulated(W, b, skips, rays)
        c32 = R.critical_kappa(W, b, skips, rays, z, idx, dtype=np.float32)
        inr = R.in_range(ck)
        np.testing.assert_array_equal(c32['always'], ck['always'])
        worst[name] = float(np.abs(c32['kappa'][inr] / ck['kappa'][inr] - 1).max()) if inr.any() else 0.0
    print('\n[twopass_ref] worst |kappa*_f32 / kappa*_f64 - 1| per case: ' + '  '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert 4 * max(worst.values()) <= DELTA <= 5e-3
    assert max(worst.values()) >= 0.25 * MEASURED                                         # the docstring's figure is this measurement
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'δ = 1.4e-4' in design and '2^(1/2048)' in design


@pytest.mark.parametrize('name', SCAN_CASES)
def test_every_mutation_moves_kappa_by_more_than_the_scan_tolerates(name):
    W, b, skips, rays = R.case(name)
    p1, z, idx, ck = R.emulated(W, b, skips, rays)
    inr = R.in_range(ck)
    tol = 2 * (DELTA + R.G)
    share = {}
    for mut in R.MUTATIONS:
        if mut in R.EDGE_MUTATIONS or not R.applies(mut, skips):
            continue
        km = R.critical_kappa(W, b, skips, rays, z, idx, mut=mut, p1=p1)['kappa']
        share[mut] = float((np.abs(km[inr] / ck['kappa'][inr] - 1) > tol).mean())
    print(f'\n[twopass_ref] {name}: share of in-range rays moved by more than {tol:.2e}: ' + '  '.join(f'{k} {v:.0%}' for k, v in share.items()))
    assert len(share) == len(R.MUTATIONS) - len(R.EDGE_MUTATIONS) - (0 if skips else 2)
    assert min(share.values()) >= 0.10, share


def test_edge_mutations_on_rays_built_for_them():
    # the allowance: logits TIE_EPS apart -> 0 < gap <= 2e-6 span; without the allowance those rays are not flagged at kappa = 0
    W, b, skips, rays = R.edge_case('near')
    p1, z, idx, ck = R.emulated(W, b, skips, rays)
    gap = (z[:, 1:] - z[:, :-1]).min(1)
    span = rays[:, 7] - rays[:, 6]
    inside = (gap > 0) & (gap <= np.float32(2e-6) * span)
    assert inside.mean() > 0.9 and bool(ck['always'].all())
    mut = R.critical_kappa(W, b, skips, rays, z, idx, mut='no_allow', p1=p1)
    assert not mut['always'][inside].any()
    # the comparison: tied logits -> gap == 0 exactly, flagged; with near = far the gap equals the threshold and only `>` flags by the gap rule
    W, b, skips, rays = R.edge_case('tie')
    p1, z, idx, ck = R.emulated(W, b, skips, rays)
    gap = (z[:, 1:] - z[:, :-1]).min(1)
    flat = rays[:, 7] == rays[:, 6]
    assert bool((gap == 0).all()) and flat.sum() == R.N_RAYS // 16 and bool(ck['gap'].all()) and bool(ck['always'].all())
    mut = R.critical_kappa(W, b, skips, rays, z, idx, mut='ge', p1=p1)
    assert not mut['gap'][flat].any() and bool(mut['gap'][~flat].all())
    assert bool(ck['nonfinite'][flat].all()) and not ck['nonfinite'][~flat].any()              # (what keeps them flagged under either comparison)


def test_the_edges_are_in_the_input_sets():
    below_cases = 0
    for name in R.CASES:
        W, b, skips, rays = R.case(name)
        ck = R.emulated(W, b, skips, rays)[3]
        inr = R.in_range(ck)
        below = (ck['kappa'] < R.KAPPA_LO) | ck['always']
        above = (ck['kappa'] > R.KAPPA_HI) & ~ck['always']
        assert rays.shape == (R.N_RAYS, 11)
        if name in R.OUT_OF_RANGE:                                                             # (twopass_ref.CASES says why)
            assert bool((ck['ovf'] if R.OUT_OF_RANGE[name] == 'always' else above).all()), name
            continue
        assert inr.mean() >= 0.25 and above.sum() > 0, (name, inr.mean(), above.sum())
        below_cases += int(below.sum() > 0)
        pairs = {(float(a), float(f)) for a, f in rays[inr][:, 6:8]}
        assert len(pairs) >= 4 and any(a != 0 for a, _ in pairs) and any(f - a != 1 for a, f in pairs), (name, pairs)
    assert below_cases >= len(SCAN_CASES) // 2
    for which, both in (('x300', False), ('x70', True)):
        W, b, skips, rays = R.saturating_case(which)
        norm = R.pass1(W, b, skips, rays)['S'].max((0, 1)) / R.OVF2
        assert (np.abs(norm - 1) <= R.SAT_BAND).mean() <= 0.02
        hi, lo = (norm > 1 + R.SAT_BAND).mean(), (norm < 1 - R.SAT_BAND).mean()
        assert (hi > 0.2 and lo > 0.2) if both else hi == 1.0, (which, hi, lo)


@pytest.mark.parametrize('seed,kind', [(0, 'trained'), (1, 'default'), (2, 'spread'), (0, 'optimizer'), (0, 'x4')])
def test_restatement_against_the_older_model(seed, kind):
    import sampler_twopass_model as M
    from oracle import pronerf_oracle as orc
    from oracle import synth
    H, Wd, focal, n = 756, 1008, 815.13, 1024
    scene = synth.make_scene(seed, H=H, W=Wd, focal=focal, rotate=True)
    w = synth.weight_set(seed, kind)['sampler']
    ro, rd = orc.get_rays(H, Wd, scene['K'], scene['c2w'])
    o, d = orc.ndc_rays(H, Wd, float(scene['K'][0, 0]), 1.0, ro, rd)
    sel = torch.linspace(0, H * Wd - 1, n).long()
    o, d = o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel]
    with torch.no_grad():
        _, S = M.pass1(w, o, d)
    old = M.model_std(w, S).numpy()                                                            # [n, 8], per-depth M_k
    rays = np.concatenate([o.numpy(), d.numpy(), np.zeros((n, 1)), np.ones((n, 1)), np.zeros((n, 3))], 1).astype(np.float32)
    Ws = [np.asarray(x, np.float32) for x in w['W']]; bs = [np.asarray(x, np.float32) for x in w['b']]
    p1 = R.pass1(Ws, bs, (), rays)
    sd, _ = R.sd_bound(p1, Ws, ())
    sdk, _ = R.sd_bound(p1, Ws, (), mut='M_k')
    Mk = (np.asarray(Ws[-1], np.float64)[:8] ** 2).max(1)
    assert np.abs(sd[:, None] / old / np.sqrt(Mk.max() / Mk)[None, :] - 1).max() <= 5e-4      # never below: max M >= M_k
    assert np.abs(sdk / old - 1).max() <= 5e-4
