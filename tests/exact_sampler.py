"""Exact answers for the fused sampler stage at its real shapes, and a replay of its two plane arithmetics (a plain helper module of the suite).

What tests/test_exact_sampler_{cpu,gpu}.py run.  The integer nets are made as in tests/mmskips_ref.py (``_int_stack``: interval bounds per unit, bias lifted
to the lower bound, ELU on its identity branch), with their own generator and seeds, at the shapes the frame path runs: 288 = 6 x 48 input columns,
depths 2, 5, 6, 8 without skips (the kernels without the ``_skip`` suffix), and two skip nets.  Every first-layer-like weight sits in ONE randomly chosen
6-column block of the 288, so the packer's fold over the 48 ray points returns the weight itself and a fold that misses or doubles a block moves a unit
by >= 1.  The same integer net serves both scales: ``pack_true`` hands the integers to the exact-fp32 kernels, ``pack_scaled`` hands pre-images (stored
hi planes = the integers) to the log2(e)-scaled streams of pass 1 and of the split-fp16 kernel.

Three input / net families:
  * ``small``: rays of mmskips_ref.sampler_rays (moment components in [0, 2]): every lo plane of every operand is exactly 0;
  * ``x_big``: moment components in {2048 .. 2051}: fp16 hi 2048, 2048, 2050, 2052, lo' 0, +2048, 0, -2048, so the W_hi P_lo product of layer 0 and of
    the skip layers' x k-step carries an integer that the answer needs.  A few first-layer rows also carry an odd weight above 2048 on the constant
    column, whose own lo plane is +-2048: the W_lo P_hi term carries an integer too;
  * ``hid_big`` (split kernel and exact kernels only: pass 1 holds activations in one fp16 plane): a third of the units of every hidden layer have their
    bias lifted by 2048 + r, so their activations are integers in [2048, 4096] that need the lo plane X_lo' of ``store_piece``.

``replay`` restates the plane arithmetic of ``sampler_h16_body`` ('h16': split_h16, layer_h16x2's three-term product, store_piece) and of
``sampler_p1_body`` ('p1': the split layer 0 and skip k-steps, one fp16 plane elsewhere) on the packer's planes (pnrf_pack_rules.h split_h16: the weight
times its scale in double, hi = RN fp16, lo' = RN fp16 of the remainder x 2^11), products in float64, every accumulator rounded to fp32 once.
``MUTATIONS`` are one-slip variants of it, in the manner of twopass_ref.MUTATIONS.

Tolerance.  B = the unmutated replay's largest |add, mul - exact integer| per net and family (the pre-images' lo-plane residuals, <= 2^-24 relative, times
operands up to 2^11 .. 2^12; fp32 ulp of the combined value); the GPU tests hold the kernels to T = 4 B (the factor mmskips_ref.SCALED_TOL keeps over its
derivation), and T <= 1/8 while every mutation moves an output by >= 1 - T.  As tests/test_exact_sampler_cpu.py measures them (B; T = 4 B):

    family   replay  D 2              D 5              D 6              D 8              D 6 skips [0, 4]  D 3 skips [0, 1]
    small    p1      2.0e-6; 8.0e-6   2.0e-6; 8.0e-6   3.9e-6; 1.6e-5   7.7e-6; 3.1e-5   7.7e-6; 3.1e-5    2.0e-6; 8.0e-6
    small    h16     2.9e-6; 1.2e-5   3.9e-6; 1.6e-5   7.7e-6; 3.1e-5   1.2e-5; 4.8e-5   1.2e-5; 4.8e-5    3.0e-6; 1.2e-5
    x_big    p1      2.0e-5; 8.0e-5   3.9e-6; 1.6e-5   7.7e-6; 3.1e-5   7.7e-6; 3.1e-5   3.9e-6; 1.6e-5    1.6e-5; 6.4e-5
    x_big    h16     1.0e-4; 4.0e-4   1.3e-4; 5.2e-4   3.1e-4; 1.3e-3   2.5e-4; 1.0e-3   1.8e-4; 7.2e-4    9.3e-5; 3.8e-4
    hid_big  h16     3.0e-4; 1.2e-3   2.1e-4; 8.4e-4   1.8e-4; 7.2e-4   3.3e-4; 1.4e-3   1.0e-4; 4.0e-4    1.8e-4; 7.2e-4

(``B_TABLE`` holds B; test_exact_sampler_cpu.py::test_tolerance_table asserts that it is what the replay gives.  Pass 1 packs its activations to fp16, which
returns every hidden activation but a zero to its integer: its B is an fp32 ulp of the largest output plus what a chain of zero units lets through.)
"""
from __future__ import annotations

import math

import numpy as np
import torch

import exact_nets as en
import mmskips_ref as ms
import twopass_ref as tp

LOG2E = en.LOG2E
P = 48
IN_CH = 6 * P
DEPTHS = (2, 5, 6, 8)
SKIP_NETS = ((6, (0, 4)), (3, (0, 1)))
PERM = ms.SAMPLER_PERM
FAMILIES = ('small', 'x_big', 'hid_big')
BIG_X = (2048, 2049, 2050, 2051)
WIDTH_CAP = 64          # a unit's interval is kept at most this wide: activations of the plain units stay far below 2048
T_MAX = 0.125

# B per (family, kernel, D, skips): the unmutated replay's largest deviation from the integers, as test_tolerance_table measured it (rounded up to two
# digits); T = 4 B.  KERNELS[family] = the replays (and scaled GPU variants) that run the family.
KERNELS = {'small': ('p1', 'h16'), 'x_big': ('p1', 'h16'), 'hid_big': ('h16',)}
B_TABLE = {
    ('small', 'p1', 2, ()): 2e-06, ('small', 'h16', 2, ()): 2.9e-06, ('small', 'p1', 5, ()): 2e-06, ('small', 'h16', 5, ()): 3.9e-06,
    ('small', 'p1', 6, ()): 3.9e-06, ('small', 'h16', 6, ()): 7.7e-06, ('small', 'p1', 8, ()): 7.7e-06, ('small', 'h16', 8, ()): 1.2e-05,
    ('small', 'p1', 6, (0, 4)): 7.7e-06, ('small', 'h16', 6, (0, 4)): 1.2e-05, ('small', 'p1', 3, (0, 1)): 2e-06, ('small', 'h16', 3, (0, 1)): 3e-06,
    ('x_big', 'p1', 2, ()): 2e-05, ('x_big', 'h16', 2, ()): 0.0001, ('x_big', 'p1', 5, ()): 3.9e-06, ('x_big', 'h16', 5, ()): 0.00013,
    ('x_big', 'p1', 6, ()): 7.7e-06, ('x_big', 'h16', 6, ()): 0.00031, ('x_big', 'p1', 8, ()): 7.7e-06, ('x_big', 'h16', 8, ()): 0.00025,
    ('x_big', 'p1', 6, (0, 4)): 3.9e-06, ('x_big', 'h16', 6, (0, 4)): 0.00018, ('x_big', 'p1', 3, (0, 1)): 1.6e-05, ('x_big', 'h16', 3, (0, 1)): 9.3e-05,
    ('hid_big', 'h16', 2, ()): 0.0003, ('hid_big', 'h16', 5, ()): 0.00021, ('hid_big', 'h16', 6, ()): 0.00018, ('hid_big', 'h16', 8, ()): 0.00033,
    ('hid_big', 'h16', 6, (0, 4)): 0.0001, ('hid_big', 'h16', 3, (0, 1)): 0.00018,
}


def up2(x):
    """x rounded up to two significant digits (how B_TABLE records a measured bound)."""
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f'{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.2g}')


def measure_bound(net, kind):
    """B of one net and replay: the replay's largest |add, mul - exact integer| over the family's population, plus one fp32 ulp of the largest
    |add, mul| (the replay rounds every accumulator once; the kernels' MFMA chains round in their own order, an ulp of the result apart)."""
    rays = population(net['family'])
    y = exact_forward(net, x6_of(rays), KERNELS[net['family']])
    r = replay(kind, *pack_scaled(net), rays)
    return float(np.abs(r[:, 8:24] - y[:, 8:24]).max()) + float(np.spacing(np.float32(np.abs(y[:, 8:24]).max())))


def tol(family, kind, D, skips=()):
    return 4.0 * B_TABLE[(family, kind, D, tuple(skips))]


# ----------------------------------------------------------------------------------------------- nets
def _lift(b):
    """The smallest integer >= b whose float32 pre-image exists for both spellings of the bias scale (``bias_pre_image``)."""
    while bias_pre_image(b) is None:
        b += 1
    return b


def bias_pre_image(k):
    """float32 v with fp32(double(v) log2e) == k (the pass-1 bias table, pnrf_pack_rules.h bias_val) AND fp32(v fp32(log2e)) == k (the split kernel scales
    the shared true-scale table itself, in fp32); None if no float32 does both."""
    w = np.float32(k / LOG2E)
    cands = [w]
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        c = w
        for _ in range(3):
            c = np.nextafter(c, toward)
            cands.append(c)
    for v in cands:
        if np.float32(np.float64(v) * LOG2E) == k and np.float32(v * np.float32(LOG2E)) == k:
            return v
    return None


def _place(rs, W, r, comp, val):
    """Weight ``val`` of row r on Pluecker component comp, in one randomly chosen block of the 48."""
    W[r, 6 * rs.randint(P) + comp] += val


def _fold(Wx):
    return np.asarray(Wx, np.float64).reshape(Wx.shape[0], -1, 6).sum(1)


def make_net(D, skips=(), family='small', seed=0):
    """Integer sampler net 288 -> D x 256 -> 27 for the rays of ``rays_for(family)`` (module docstring).  {'W', 'b'}: float64 integers; 'family', 'D', 'skips':
    what it was made for."""
    assert family in FAMILIES
    rs = np.random.RandomState(7919 + 101 * D + 17 * sum(2 ** s for s in skips) + 1009 * FAMILIES.index(family) + seed)
    big_x, big_h = family == 'x_big', family == 'hid_big'
    lo_x = np.array([0, 0, 1, 2048 if big_x else 0, 2048 if big_x else 0, 0], np.float64)
    hi_x = np.array([0, 0, 1, 2051 if big_x else 2, 2051 if big_x else 2, 0], np.float64)
    Ws, bs = [], []
    lo = hi = None
    for l in range(D):
        skip = l >= 1 and (l - 1) in skips
        W = np.zeros((256, (IN_CH if l == 0 or skip else 0) + (256 if l else 0)))
        off = W.shape[1] - (256 if l else 0)
        if l == 0:
            comp = rs.permutation(np.tile([2, 3, 4], 86))[:256]
            for r in range(256):
                _place(rs, W, r, comp[r], rs.choice((1, 1, 2, 3, -1, -2)))
                if rs.rand() < 0.5:
                    _place(rs, W, r, rs.choice([c for c in (2, 3, 4) if c != comp[r]]), rs.choice((-1, 1)))
                if big_x and r % 16 == 5 and not W[r, 2::6].any():      # an odd weight above 2048 on the constant column: W_lo' = +-2048
                    _place(rs, W, r, 2, rs.choice((2049, 2051, 2053, -2049)))
        else:
            perm = rs.permutation(256)
            for r in range(256):
                W[r, off + perm[r]] += 1
                if rs.rand() < 0.5:
                    c = rs.choice(np.delete(np.arange(256), perm[r]))
                    if (hi[perm[r]] - lo[perm[r]]) + (hi[c] - lo[c]) <= WIDTH_CAP:
                        W[r, off + c] -= 1
                if skip and r % 4 == 0:                # x[c] - x[d] on the two moment components (+ 2 x[2] on some): sums stay below 2^13 (pass 1: x 2^11)
                    c, d = rs.permutation([3, 4])
                    _place(rs, W, r, c, 1); _place(rs, W, r, d, -1)
                    if rs.rand() < 0.5:
                        _place(rs, W, r, 2, 2)
        Wf = np.concatenate([_fold(W[:, :off]), W[:, off:]], 1) if off else W
        lo_in = np.concatenate([lo_x, lo]) if (off and l) else (lo_x if l == 0 else lo)
        hi_in = np.concatenate([hi_x, hi]) if (off and l) else (hi_x if l == 0 else hi)
        l0 = np.where(Wf > 0, Wf * lo_in, Wf * hi_in).sum(1); h0 = np.where(Wf > 0, Wf * hi_in, Wf * lo_in).sum(1)
        b = -l0 + rs.randint(0, 3, 256)
        if big_h:
            up = rs.rand(256) < 1 / 3
            b = b + up * (2048 + rs.randint(0, 1980, 256))
        b = np.array([_lift(v) for v in b], np.float64)
        Ws.append(W); bs.append(b)
        lo, hi = l0 + b, h0 + b
    # head: depth rows a spread, permuted bias only (M = 0: pass 1 flags nobody by its bound); add / mul read every last-layer unit once with +-1, centred by their bias
    W = np.zeros((27, 256)); b = np.zeros(27)
    b[:8] = (np.arange(8) - 4.0)[PERM]
    W[8:24] = en._dense(rs, 16, 256, (-1, 1))
    l0 = np.where(W > 0, W * lo, W * hi).sum(1); h0 = np.where(W > 0, W * hi, W * lo).sum(1)
    b[8:24] = (-np.floor((l0 + h0) / 2) + rs.randint(-5, 6, 27))[8:24]
    assert max(np.abs(l0 + b).max(), np.abs(h0 + b).max()) < 2 ** 12
    Ws.append(W); bs.append(b)
    return {'W': Ws, 'b': bs, 'family': family, 'D': D, 'skips': tuple(skips)}


_NETS = {}


def net_for(D, skips=(), family='small'):
    key = (D, tuple(skips), family)
    if key not in _NETS:
        _NETS[key] = make_net(D, skips, family)
    return _NETS[key]


def pack_true(net):
    """fp32 weights for the exact-fp32 kernels (true scale): the integers themselves."""
    return [np.asarray(W, np.float32) for W in net['W']], [np.asarray(b, np.float32) for b in net['b']]


def pack_scaled(net, W=None):
    """fp32 weights for pnrf_mlp_pack whose log2(e)-scaled streams hold the integers of ``net`` (W: other integer weights, for the mutation self-check) in
    their hi planes: first-layer-like weights and ELU biases / log2(e), output weights x log2(e), as pre-images (exact_nets._pre_image, bias_pre_image)."""
    Ws = net['W'] if W is None else W
    L = len(Ws)
    outW, outb = [], []
    for l in range(L):
        Wl = np.asarray(Ws[l], np.float64)
        if l == 0:
            Wl = en._pre_image(Wl, LOG2E)
        elif l == L - 1:
            Wl = en._pre_image(Wl, 1.0 / LOG2E)
        elif Wl.shape[1] > 256:
            Wl = np.concatenate([en._pre_image(Wl[:, :IN_CH], LOG2E), Wl[:, IN_CH:].astype(np.float32)], 1)
        b = np.asarray(net['b'][l], np.float32) if l == L - 1 else np.array([bias_pre_image(v) for v in net['b'][l]], np.float32)
        outW.append(np.asarray(Wl, np.float32)); outb.append(b)
    return outW, outb


# ----------------------------------------------------------------------------------------------- rays
def rays_for(family, n, seed=0, same=None):
    """rays [n, 11] float32: o = (a, b, c), d = (0, 0, 1), near 0, far 1: unit direction (0, 0, 1), moment (b, -a, 0) exactly.  small / hid_big:
    mmskips_ref.sampler_rays; x_big: b and -a run through the 16 combinations of {2048 .. 2051} (ray r takes combination r % 16 of a seeded order).
    same: indices of rays that get near == far = 0.5 (flagged by pass 1 at every kappa; their depths are all 0.5, the stable sort leaves the order)."""
    if family == 'x_big':
        rs = np.random.RandomState(1913 + seed)
        comb = rs.permutation(16)[np.arange(n) % 16]
        o = np.stack([-(2048.0 + comb % 4), 2048.0 + comb // 4, rs.randint(-2, 3, n)], 1)
        d = np.tile([0.0, 0.0, 1.0], (n, 1))
        rays = np.concatenate([o, d, np.zeros((n, 1)), np.ones((n, 1)), d], 1).astype(np.float32)
    else:
        rays = ms.sampler_rays(n, seed)
    if same is not None:
        rays[np.asarray(same, np.int64), 6:8] = 0.5
    return rays


LIST_N = 257
LIST_SIZES = (0, 1, 63, 64, 65, 127, 128, 129)


def flag_subset(size, n=LIST_N):
    """Sorted ray numbers of the subset of ``size`` rays that get near == far: a seeded draw; the odd sizes hold ray 0, the sizes from 64 on ray n - 1."""
    rs = np.random.RandomState(4057 + size)
    must = ([0] if size % 2 else []) + ([n - 1] if size >= 64 else [])
    rest = rs.permutation(np.setdiff1d(np.arange(n), must))[:size - len(must)] if size else np.zeros(0, np.int64)
    return np.sort(np.concatenate([np.asarray(must[:size], np.int64), rest]).astype(np.int64))


def population(family):
    """One ray per distinct input of the family (16 resp. 9 moment pairs): certifying these covers every ray count."""
    if family == 'x_big':
        return rays_for('x_big', 16)
    r = ms.sampler_rays(9)
    r[:, 0] = -(np.arange(9) % 3); r[:, 1] = np.arange(9) // 3
    return r


def x6_of(rays):
    o = np.asarray(rays, np.float64)[:, :3]
    z = 0 * o[:, 0]
    return np.stack([z, z, 1 + z, o[:, 1], -o[:, 0], z], 1)


def exact_rows(net, rays):
    """y [n, 27] (float64) of the integer net per ray, through the distinct inputs (``exact_forward`` on them)."""
    x6 = x6_of(rays)
    u, inv = np.unique(x6, axis=0, return_inverse=True)
    return exact_forward(net, u)[inv.reshape(-1)]


def order_of(net):
    return np.argsort(net['b'][-1][:8], kind='stable')


# ----------------------------------------------------------------------------------------------- certificate
def _two_planes(v):
    return en.split_exact(v)


def exact_forward(net, x6, kinds=()):
    """The exact answer y [n, 27] of the net on Pluecker vectors x6 [n, 6] (tiled over the 48 ray points), every layer walked in the manner of
    exact_nets.check_layer: operands that meet a nonzero weight are integers; pre-activations >= 0; sums of |terms| < 2^24; the walk equals the
    oracle's float64 forward (mmskips_ref.skip_backbone = orc.mlp_elu_backbone without skips).  kinds: also what the planes of these replays need —
    'h16': first-layer-like weights, inputs and every activation survive the split into hi + 2^-11 lo'; 'p1': the same for the weights and inputs of
    layer 0 and of the skip k-step, every hidden activation and weight an fp16 integer (<= 2048), and the sums of a skip layer, which runs at
    scale 2^11, below 2^13 (x 2^11: multiples of 2^11 below 2^24)."""
    x6 = np.asarray(x6, np.float64)
    x = np.tile(x6, (1, P))
    Ws, bs = net['W'], net['b']
    L = len(Ws)
    sk = ms.skips_of(Ws)
    h = x
    for l in range(L):
        W, b = np.asarray(Ws[l], np.float64), np.asarray(bs[l], np.float64)
        what = f'D {net["D"]} skips {net["skips"]} {net["family"]} layer {l}'
        y = en.check_layer(h, W, b, en.LIM['f32'], what, elu=l < L - 1)
        has_x = l == 0 or (l - 1) in sk
        Wx, Wh = (W[:, :IN_CH], W[:, IN_CH:]) if has_x else (W[:, :0], W)
        hh = h[:, IN_CH:] if has_x else h
        if kinds:
            if has_x:
                Wf = _fold(Wx)
                assert np.array_equal(np.abs(Wf).sum(1), np.abs(Wx).sum(1)), f'{what}: two weights of a row share a component (the fold would add them)'
                assert _two_planes(Wf) and _two_planes(x6[:, np.any(Wf != 0, 0)]), f'{what}: x-part not representable in two planes'
            live = hh[:, np.any(Wh != 0, 0)] if Wh.size else np.zeros((1, 0))
            assert np.abs(Wh).max(initial=0) <= en.LIM['f16']
            if 'h16' in kinds:
                assert _two_planes(live) and np.abs(live).max(initial=0) < 65504, f'{what}: activation not representable in two planes'
            if 'p1' in kinds:
                assert np.abs(live).max(initial=0) <= en.LIM['f16'], f'{what}: activation beyond the fp16 integers'
                if has_x and l:
                    bound = np.abs(h) @ np.abs(W).T + np.abs(b)
                    assert bound.max() * 2048 < en.ACC_MAX, f'{what}: sums of |terms| x 2^11 up to {bound.max() * 2048} >= 2^24'
            assert all(bias_pre_image(v) is not None for v in b) or l == L - 1, f'{what}: a bias without a float32 pre-image'
        h = y if l not in sk else np.concatenate([x, y], 1)
    ref = ms.skip_backbone(torch.from_numpy(x), [torch.from_numpy(np.asarray(W, np.float64)) for W in Ws],
                           [torch.from_numpy(np.asarray(b, np.float64)) for b in bs]).numpy()
    np.testing.assert_array_equal(h, ref)
    assert np.abs(ref[:, 8:24]).max() < 2 ** 12
    return ref


# ----------------------------------------------------------------------------------------------- replay of the plane arithmetic
# name -> what slips.  'Xlo_*' exist in the split kernel only (pass 1 has one activation plane); 'skip_*' in nets with skips only.
MUTATIONS = {
    'Plo_drop': 'P_lo of the folded input missing (layer 0 and the skip k-step)',
    'Plo_swap': 'the two moment components of P_lo exchanged',
    'Plo_in_Wlo': 'P_lo in place of P_hi in the W_lo term',
    'lo_scale': '2^-10 in place of 2^-11 where the cross accumulator joins the main one',
    'skip_Plo_drop': "the lo operand of a skip layer's x k-step (the ninth of the split kernel) missing; layer 0 keeps its own",
    'Xlo_ks_next': "X_lo' of k-step tp read from tp + 1 (32 features on)",
    'Xlo_ks_prev': "X_lo' of k-step tp read from tp - 1",
    'Xlo_pair': "the two halves of every packed X_lo' pair exchanged (v_fma_mixlo / mixhi)",
}
MUTATIONS.update({f'Xlo_drop_{l}': f"X_lo' of layer {l}'s activations missing" for l in range(max(DEPTHS))})
PLO_MUTATIONS = ('Plo_drop', 'Plo_swap', 'Plo_in_Wlo', 'lo_scale', 'skip_Plo_drop')


def applies(mut, kind, D, skips):
    if mut.startswith('skip_'):
        return len(skips) > 0
    if mut.startswith('Xlo_drop_'):
        return kind == 'h16' and int(mut[9:]) < D
    if mut.startswith('Xlo_'):
        return kind == 'h16'
    return True


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _h(x):
    """Round to nearest fp16, saturating at +-65 504 (MODE.FP16_OVFL; the packer's values are far below)."""
    return np.clip(np.asarray(x, np.float64), -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def _split(v):
    """hi = RN fp16 (v), lo' = RN fp16 ((v - hi) 2^11): pnrf_pack_rules.h split_h16 on a double, the kernels' split_h16 / store_piece on an fp32 value
    (v - hi and the product with 2^11 are exact there)."""
    hi = _h(v)
    return hi, _h((np.asarray(v, np.float64) - hi) * 2048.0)


def _elu(y):
    with np.errstate(over='ignore'):
        return _r32(np.where(y > 0, y, LOG2E * np.exp2(np.minimum(y, 0)) - LOG2E))


def planes(Wp, bp):
    """The packer's streams of fp32 pack weights (pnrf_pack.hip pack_sampler, scale_for_elu): per layer dict(xh, xl: planes of the folded x-part times
    log2(e); wh, wl: planes of the h-columns (the output layer's over log2(e)); w1: their single fp16 plane of pass 1; b_p1, b_h16: the bias as each
    kernel sees it)."""
    L = len(Wp)
    out = []
    for l in range(L):
        W = np.asarray(Wp[l], np.float32)
        has_x = l == 0 or W.shape[1] > 256
        d = {}
        if has_x:
            xf = tp._fold(W[:, :W.shape[1] - (256 if l else 0)], (W.shape[1] - (256 if l else 0)) // 6).astype(np.float64) * LOG2E
            d['xh'], d['xl'] = _split(xf)
        if l:
            wd = W[:, -256:].astype(np.float64) * (1.0 / LOG2E if l == L - 1 else 1.0)
            d['wh'], d['wl'] = _split(wd)
            d['w1'] = _h(wd)
        b = np.asarray(bp[l], np.float32)
        d['b_p1'] = b.astype(np.float64) if l == L - 1 else _r32(b.astype(np.float64) * LOG2E)
        d['b_h16'] = b.astype(np.float64) if l == L - 1 else (b * np.float32(LOG2E)).astype(np.float64)
        out.append(d)
    return out


def replay(kind, Wp, bp, rays, mut=None):
    """y [n, 27] (float64 holding fp32 values, unsorted) of the split kernel ('h16') or of pass 1 ('p1') on rays [n, 11], from the fp32 weights handed to
    the packer.  Products in float64 (exact for these operands), each accumulator rounded to fp32 once, the cross accumulator joined by one fma."""
    pl = planes(Wp, bp)
    L = len(pl)
    x6 = tp.pluecker32(rays)
    Ph, Pl = _split(x6)
    if mut == 'Plo_drop':
        Pl = 0 * Pl
    elif mut == 'Plo_swap':
        Pl = Pl[:, [0, 1, 2, 4, 3, 5]]
    inv = 2.0 ** -10 if mut == 'lo_scale' else 2.0 ** -11
    Pw = Pl if mut == 'Plo_in_Wlo' else Ph              # the operand of the W_lo term

    def xpart(d, skip_layer):
        plo = 0 * Pl if (skip_layer and mut == 'skip_Plo_drop') else Pl
        return Ph @ d['xh'].T, plo @ d['xh'].T + Pw @ d['xl'].T

    bk = 'b_h16' if kind == 'h16' else 'b_p1'
    mn, cr = xpart(pl[0], False)
    a = _elu(_r32(_r32(cr) * inv + _r32(mn + pl[0][bk])))
    for l in range(1, L):
        d = pl[l]
        last = l == L - 1
        if kind == 'h16':
            Xh, Xl = _split(a)
            if mut == f'Xlo_drop_{l - 1}':
                Xl = 0 * Xl
            elif mut == 'Xlo_ks_next':
                Xl = np.roll(Xl, -32, 1)
            elif mut == 'Xlo_ks_prev':
                Xl = np.roll(Xl, 32, 1)
            elif mut == 'Xlo_pair':
                Xl = Xl.reshape(len(Xl), 128, 2)[:, :, ::-1].reshape(len(Xl), 256)
            mn = Xh @ d['wh'].T + d[bk]
            cr = Xl @ d['wh'].T + Xh @ d['wl'].T
            if 'xh' in d:
                m2, c2 = xpart(d, True)
                mn, cr = mn + m2, cr + c2
            pre = _r32(_r32(cr) * inv + _r32(mn))
        else:
            B = _h(a)
            if 'xh' in d:                               # the layer runs at scale 2^11 in ONE accumulator (PK_F16_SKIP: W 2^11, W_hi 2^11 | W_hi | W_lo 2^11)
                m2, c2 = xpart(d, True)
                pre = _r32(_r32(2048.0 * (B @ d['w1'].T + m2 + d[bk]) + c2 * (2048.0 * inv)) / 2048.0)
            else:
                pre = _r32(B @ d['w1'].T + d[bk])
        a = pre if last else _elu(pre)
    return a


def answers(y, order):
    """(add, mul) [n, 8] of rows y [n, 27] in the sorted order."""
    return y[:, 8:16][:, order], y[:, 16:24][:, order]
