"""The two-pass sampler's per-ray decision, restated once: what tests/test_twopass_flags_{cpu,gpu}.py compare the kernel with.

``sampler_p1_kernel`` / ``sampler_p1_skip_kernel`` (pnrf_mlp_kernels.hip, ``sampler_p1_body``) flag ray r at threshold kappa when, on its SORTED
pass-1 depths z_0 <= .. <= z_7 (fp32, written by the kernel), some adjacent gap is not above the bound

    thr_i = kappa (sdev_i + sdev_{i+1}) + 2e-6 span,        sdev_i = (z_i - near)(1 - u_i) sd,   u_i = (z_i - near) / span,   span = far - near,
    sd    = sqrt(p1c[0] U),   U = U^0 + U^1,   U^h = 2c S^h_L + V^h_L,   V^h_{l+1} = p1c[1 + l] (2c S^h_l + V^h_l),   V^h_0 = 0,   2c = 2 x (2^-22 / 3) in fp32,

or when the comparison is not finite, or when some S^h_l >= 65504^2.  With everything the kernel carries:

  * S^h_l is the sum of a^2 over HALF h of layer l's 256 activations (l = 0 .. L, L = number of 256 -> 256 layers): the activations ``a = log2(e) x`` are
    on the packer's log2(e) scale (``scale_for_elu``) and are squared UNROUNDED (fp32), before the fp16 pack.  A half is what one lane of the
    32x32 MFMA accumulator holds: features f with (f % 8) < 4 (half 0) resp. >= 4 (half 1) (``acc_row``, pnrf_engine.h) — 16 of every 32.  The
    recurrence is linear, so the two halves run side by side and only U is summed; the fp16-range test however is on each half's partial sum
    (an activation at the saturation limit 65 504 puts its own half's sum at >= 65504^2, which is all the test is for).
  * p1c[1 + l] = fp32(C_{l+1} (1 + 1e-6)), C_l = max_j sum_i W_l[i, j]^2 over the 256 h-columns of Linear l (for a skip layer, cat([x, h]): columns
    in_ch .. in_ch + 255); p1c[0] = fp32(M / log2(e)^2 (1 + 1e-6)), M = max_{k < 8, j} W_out[k, j]^2: the log2(e)^2 of the S_l cancels there.
  * the net: layer 0 fp32-grade on the folded Pluecker input (fold = fp64 sum over the P ray points, rounded to fp32, x log2(e)); Linear l >= 1 with
    fp16-rounded weights (RN) and fp16-packed activations (RN, saturating at 65 504: MODE.FP16_OVFL), fp32 bias x log2(e); the x-part of a skip layer
    fp32-grade like layer 0; ELU on the log2(e) scale, ``elu(y) = y > 0 ? y : log2(e) (2^y - 1)``.

``critical_kappa`` returns, per ray, kappa* = min_i (gap_i - 2e-6 span) / (sdev_i + sdev_{i+1}) — the ray is flagged exactly when kappa >= kappa* — and the
mask of rays flagged at every kappa >= 0 (a gap <= 2e-6 span, a non-finite comparison, a half-layer norm at the fp16 limit).  The same code runs in
float64 (the reference) and in float32 (``dtype=``), which measures how far the arithmetic's own rounding moves kappa* (the tolerance of the tests).

``MUTATIONS`` are one-slip variants of the restatement; the CPU test shows that each moves kappa* (or the mask) by more than the GPU test tolerates.
"""
from __future__ import annotations

import numpy as np

LOG2E = 1.4426950408889634
C2_F32 = float(np.float32(2.0) * np.float32(7.947285970052083e-08))      # 2 c as the kernel spells it
ALLOW_F32 = float(np.float32(2e-6))
F16_MAX = 65504.0
OVF2 = float(np.float32(65504.0) * np.float32(65504.0))
PACK_MARGIN = 1.0 + 1e-6

# name -> what slips.  'skip_*' apply to nets with skip connections only; 'no_allow' and 'ge' move the edge of the gap rule, not kappa* (see the CPU test).
MUTATIONS = {
    'C_shift': 'C_l read one slot early: p1c[l] in place of p1c[1 + l] (layer 0 gets the output constant)',
    'tile_next': 'the last 32-column tile of every layer credited to the next layer\'s S',
    'tile_drop': 'the last 32-column tile of every layer missing from S',
    'half1': 'the rows of half 1 missing from U',
    'no_last': '2c S_L of the last layer missing from U',
    'c_not_2c': 'c in place of 2c',
    'M_log2e': 'M not divided by log2(e)^2',
    'M_k': 'per-depth M_k in place of the max over the 8 depth rows',
    'no_1mu': 'sdev without the (1 - u) factor',
    'span2': 'sdev with span applied twice',
    'single': 'sdev_i alone in place of sdev_i + sdev_{i+1}',
    'no_allow': 'the 2e-6 span allowance dropped',
    'ge': '>= in place of >',
    'skip_C_all': 'C_l of a skip layer over all 262 packed columns [h | folded x]',
    'skip_C_off1': 'C_l of a skip layer over packed columns 1 .. 256 (h-columns offset by one)',
}
EDGE_MUTATIONS = ('no_allow', 'ge')


def applies(mut, skips):
    return not mut.startswith('skip_') or len(skips) > 0


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def pluecker32(rays):
    """The kernel's folded input (unit_dir + moment at t = 0, pnrf_geom.h) in its fp32 operations: [n, 6] float64 holding fp32 values."""
    r = np.asarray(rays, np.float32).astype(np.float64)
    o, d = r[:, 0:3], r[:, 3:6]
    n2 = _r32(d[:, 2] * d[:, 2] + _r32(d[:, 1] * d[:, 1] + _r32(d[:, 0] * d[:, 0])))
    den = np.maximum(_r32(np.sqrt(n2)), 1e-12)
    h = _r32(d / den[:, None])
    cr = lambda a1, b2, a2, b1: _r32(a1 * b2 - _r32(a2 * b1))              # fma(a1, b2, -(a2 b1))
    m = np.stack([cr(o[:, 1], h[:, 2], o[:, 2], h[:, 1]), cr(o[:, 2], h[:, 0], o[:, 0], h[:, 2]), cr(o[:, 0], h[:, 1], o[:, 1], h[:, 0])], 1)
    return np.concatenate([h, m], 1)


def _f16(x):
    with np.errstate(over='ignore'):
        return np.asarray(x).astype(np.float16)


def _pack16(a, T):
    """v_cvt_pk_f16_f32 under MODE.FP16_OVFL: round to nearest even, saturate at +-65 504."""
    return _f16(np.clip(a, -F16_MAX, F16_MAX)).astype(T)


def _elu_scaled(y, T):
    with np.errstate(over='ignore'):
        return np.where(y > 0, y, (T(LOG2E) * (np.exp2(np.minimum(y, 0)) - T(1))).astype(T)).astype(T)


def _fold(Wx, P):
    return np.asarray(Wx, np.float64).reshape(Wx.shape[0], P, 6).sum(1).astype(np.float32)


def constants(W, skips, mut=None):
    """The packer's p1c block (pnrf_pack.hip): fp32 values [M / log2e^2, C_1 .. C_L] and, for the 'M_k' mutation, the per-row M_k [8]."""
    L = len(W) - 2
    in_ch = W[0].shape[1]
    C = []
    for l in range(1, L + 1):
        Wl = np.asarray(W[l], np.float64)
        if (l - 1) in skips:
            packed = np.concatenate([Wl[:, in_ch:], _fold(W[l][:, :in_ch], in_ch // 6).astype(np.float64)], 1)      # [h | folded x], as the packer lays it out
            cols = packed if mut == 'skip_C_all' else packed[:, 1:257] if mut == 'skip_C_off1' else packed[:, :256]
        else:
            cols = Wl
        C.append(np.float32((cols ** 2).sum(0).max() * PACK_MARGIN))
    Mk = (np.asarray(W[-1], np.float64)[:8] ** 2).max(1)
    div = 1.0 if mut == 'M_log2e' else LOG2E * LOG2E
    m_out = np.float32(Mk.max() / div * PACK_MARGIN)
    return m_out, C, np.asarray([np.float32(m / div * PACK_MARGIN) for m in Mk])


def pass1(W, b, skips, rays, dtype=np.float64, square_rounded=False):
    """Pass 1 of the sampler on rays [n, 11] in ``dtype`` arithmetic -> dict(S [L + 1, 2, n] half-layer norms on the log2(e) scale, T [L + 1, 2, n] the
    part of S in the last 32-column tile, logits [n, 8] of the depth rows).  square_rounded: square the fp16-packed activations (what
    tools/sampler_twopass_model.py does; the kernel squares the unrounded ones)."""
    T = np.dtype(dtype).type
    L = len(W) - 2
    in_ch = W[0].shape[1]
    x6 = pluecker32(rays).astype(T)
    half = (np.arange(256) % 8) >= 4
    last = np.arange(256) >= 224
    sc = lambda v: (np.asarray(v, np.float64) * LOG2E)
    bias = lambda l: sc(b[l]).astype(np.float32).astype(T)
    a = _elu_scaled(x6 @ sc(_fold(W[0], in_ch // 6)).astype(T).T + bias(0), T)
    S, Tl = [], []

    def norms(a):
        q = (_pack16(a, T) if square_rounded else a) ** 2
        S.append(np.stack([q[:, ~half].sum(1, dtype=T), q[:, half].sum(1, dtype=T)]))
        Tl.append(np.stack([q[:, ~half & last].sum(1, dtype=T), q[:, half & last].sum(1, dtype=T)]))
    norms(a)
    for l in range(1, L + 1):
        Wl = np.asarray(W[l], np.float32)
        if (l - 1) in skips:                       # the layer runs at scale 2^11 (same significands); its x-part as layer 0's product
            Wh = (_f16(Wl[:, in_ch:] * np.float32(2048.0)).astype(np.float64) / 2048.0).astype(T)
            pre = _pack16(a, T) @ Wh.T + x6 @ sc(_fold(Wl[:, :in_ch], in_ch // 6)).astype(T).T + bias(l)
        else:
            pre = _pack16(a, T) @ _f16(Wl).astype(T).T + bias(l)
        a = _elu_scaled(pre.astype(T), T)
        norms(a)
    Wo = _f16((np.asarray(W[-1], np.float64)[:8] / LOG2E).astype(np.float32)).astype(T)
    logits = _pack16(a, T) @ Wo.T + np.asarray(b[-1], np.float32)[:8].astype(T)
    return dict(S=np.stack(S), T=np.stack(Tl), logits=logits.astype(T))


def sorted_depths(logits, rays):
    """The kernel's epilogue on depth logits (fp32 operations): sigmoid, z = d span + near, stable ascending sort -> (z [n, 8] float32, idx [n, 8])."""
    r = np.asarray(rays, np.float32)
    near, far = r[:, 6:7], r[:, 7:8]
    with np.errstate(over='ignore'):
        d = (1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))).astype(np.float32)
    z = (d * (far - near)).astype(np.float32) + near
    idx = np.argsort(z, axis=1, kind='stable')
    return np.take_along_axis(z, idx, 1), idx


def sd_bound(p1, W, skips, dtype=np.float64, mut=None):
    """sd = sqrt(p1c[0] U) per ray [n] (for 'M_k': per depth row [n, 8]) from the half-layer norms of ``pass1``, and the fp16-range mask [n]."""
    T = np.dtype(dtype).type
    m_out, C, Mk = constants(W, skips, mut)
    S, Tl = p1['S'].astype(T), p1['T'].astype(T)
    L = S.shape[0] - 1
    if mut == 'tile_drop':
        S = S - Tl
    elif mut == 'tile_next':
        S = S - Tl
        S[1:] = S[1:] + Tl[:-1]
    c2 = T(C2_F32 / 2 if mut == 'c_not_2c' else C2_F32)
    coef = [T(m_out)] + [T(c) for c in C]                       # p1c
    V = np.zeros_like(S[0])
    for l in range(L):
        V = coef[l if mut == 'C_shift' else 1 + l] * (c2 * S[l] + V)
    U = V if mut == 'no_last' else c2 * S[L] + V
    U = U[0] if mut == 'half1' else U[0] + U[1]
    ovf = (p1['S'].astype(T) >= T(OVF2)).any((0, 1))
    if mut == 'M_k':
        return np.sqrt(Mk.astype(T)[None, :] * U[:, None]), ovf
    return np.sqrt(T(m_out) * U), ovf


def critical_kappa(W, b, skips, rays, z_sorted, sort_idx=None, dtype=np.float64, mut=None, p1=None):
    """-> dict(kappa [n]: the smallest threshold at which the kernel flags the ray (<= 0 or NaN: at every one), always [n] bool: flagged at every
    kappa >= 0, gap / nonfinite / ovf [n] bool: the three reasons, norm [n]: the largest half-layer norm, sd [n]).  z_sorted [n, 8]: the pass-1
    sorted depths as the kernel wrote them (fp32); sort_idx [n, 8] is needed by the 'M_k' mutation only."""
    T = np.dtype(dtype).type
    if p1 is None:
        p1 = pass1(W, b, skips, rays, dtype)
    sd, ovf = sd_bound(p1, W, skips, dtype, mut)
    r = np.asarray(rays, np.float32)
    near, far = r[:, 6:7].astype(T), r[:, 7:8].astype(T)
    z = np.asarray(z_sorted, np.float32).astype(T)
    with np.errstate(all='ignore'):
        span = far - near
        inv = T(1) / span
        u = (z - near) * inv
        sdk = np.take_along_axis(sd, np.asarray(sort_idx), 1) if mut == 'M_k' else sd[:, None]
        sdev = (z - near) * (T(1) if mut == 'no_1mu' else (T(1) - u)) * sdk
        if mut == 'span2':
            sdev = sdev * span
        pair = sdev[:, :-1] if mut == 'single' else sdev[:, :-1] + sdev[:, 1:]
        allow = np.zeros_like(span) if mut == 'no_allow' else T(ALLOW_F32) * span
        gap = z[:, 1:] - z[:, :-1]
        ratio = (gap - allow) / pair
        nonfinite = ~(np.isfinite(gap) & np.isfinite(pair) & np.isfinite(allow)).all(1)
        above = (gap >= allow) if mut == 'ge' else (gap > allow)                     # the comparison at kappa = 0
        gap_rule = ~above.all(1)
        kappa = np.where(np.isnan(ratio), -np.inf, ratio).min(1)
    return dict(kappa=kappa, always=gap_rule | nonfinite | ovf, gap=gap_rule, nonfinite=nonfinite, ovf=ovf, norm=p1['S'].max((0, 1)), sd=sd)


# ----------------------------------------------------------------------------------------------- the cases of the CPU and GPU tests
# name -> (seed, kind, mmnetdepth, mmnetskips).  Depths 3 / 4 / 9: 2 / 3 / 8 hidden 256 -> 256 layers (even and odd counts, the shortest nets).
# Two of the sets have no ray inside the scanned range, by construction of the weights: 'spread' at depth 8 (module-default hidden layers, C_l = 1/3:
# kappa* = 370 .. 640, the kernel must flag nobody up to 16) and 'x4' at depth 8 (4^8 = 65 536 x the activations: every ray is at the fp16 limit and
# flagged at every kappa).  'd6_x4' is the x4 kind where it stays inside the fp16 range (4^6).
CASES = {
    'd8_trained': (0, 'trained', 8, ()),
    'd8_spread': (1, 'spread', 8, ()),
    'd8_x4': (0, 'x4', 8, ()),
    'd6_x4': (0, 'x4', 6, ()),
    'd3': (1, 'trained', 3, ()),
    'd4': (2, 'trained', 4, ()),
    'd9': (0, 'trained', 9, ()),
    'd8_s4': (0, 'trained', 8, (4,)),
    'd6_s04': (1, 'trained', 6, (0, 4)),
}
OUT_OF_RANGE = {'d8_spread': 'above', 'd8_x4': 'always'}
CASE_SHAPES = [('d8_trained', 'narrow'), ('d8_trained', 'wide'), ('d8_spread', 'wide'), ('d8_x4', 'narrow'), ('d6_x4', 'wide'), ('d3', 'narrow'), ('d3', 'wide'),
               ('d4', 'wide'), ('d4', 'narrow'), ('d9', 'narrow'), ('d8_s4', 'narrow'), ('d8_s4', 'wide'), ('d6_s04', 'wide'), ('d6_s04', 'narrow')]
NEAR_FAR = [(0.0, 1.0), (0.0, 1.0), (0.0, 1.0), (0.0, 1.0), (0.25, 1.0), (0.0, 2.0), (0.5, 0.625), (1.0, 3.0)]      # ray i of the frame takes pair i % 8
KAPPA_LO, KAPPA_HI = 0.125, 16.0
GRID_PER_OCTAVE = 2048                             # 128 per octave is too coarse for two of the mutations (test_twopass_flags_cpu.py: grid)
G = 2.0 ** (1.0 / GRID_PER_OCTAVE) - 1.0           # the scan's step: kappa_{j+1} = kappa_j (1 + G)
N_RAYS = 1024
DELTA = 1.4e-4          # relative tolerance on kappa*: 4 x the float32 / float64 difference of this restatement (test_twopass_flags_cpu.py measures it)


def kappa_grid():
    return KAPPA_LO * 2.0 ** (np.arange(7 * GRID_PER_OCTAVE + 1) / GRID_PER_OCTAVE)


def scene_rays(seed, H=64, W=64):
    """H x W rays [n, 11] (float32 numpy) of synth.make_scene, columns 6 / 7 rewritten to NEAR_FAR[i % 8]."""
    from oracle import pronerf_oracle as orc
    from oracle import synth
    rays = orc.frame_setup(synth.make_scene(seed, H=H, W=W, rotate=True))['rays'].numpy().astype(np.float32).copy()
    nf = np.asarray(NEAR_FAR, np.float32)[np.arange(rays.shape[0]) % len(NEAR_FAR)]
    rays[:, 6], rays[:, 7] = nf[:, 0], nf[:, 1]
    return rays


def emulated(W, b, skips, rays):
    """The float64 reference on its own pass-1 depths (what the CPU test has in place of the kernel's) -> (p1, z_sorted, sort_idx, critical_kappa's dict)."""
    p1 = pass1(W, b, skips, rays)
    z, idx = sorted_depths(p1['logits'], rays)
    return p1, z, idx, critical_kappa(W, b, skips, rays, z, idx, p1=p1)


def in_range(ck):
    return (ck['kappa'] >= KAPPA_LO) & (ck['kappa'] <= KAPPA_HI) & ~ck['always']


_CACHE = {}


def case(name):
    """-> (W, b, skips, rays): the sampler's weights (float32 numpy lists) and N_RAYS rays of a 64 x 64 frame.  The short nets have most of their rays
    above the scanned range, so the rays are chosen on the reference's own kappa* (emulated depths): up to 384 rays outside the range, the rest
    inside as far as the frame has them, in frame order."""
    if name not in _CACHE:
        from oracle import synth
        seed, kind, D, skips = CASES[name]
        w = synth.make_weights(seed, kind, mmnetdepth=D, mmnetskips=skips)['sampler']
        pool = scene_rays(seed)
        inr = in_range(emulated(w['W'], w['b'], tuple(skips), pool)[3])
        out, ins = np.flatnonzero(~inr), np.flatnonzero(inr)
        n_out = max(min(len(out), 384), N_RAYS - len(ins))
        pick = np.sort(np.concatenate([out[:n_out], ins[:N_RAYS - n_out]]))
        _CACHE[name] = (w['W'], w['b'], tuple(skips), pool[pick])
    return _CACHE[name]


TIE_EPS = 2e-6          # logit distance of the 'near' set: a depth gap of span d (1 - d) eps <= 5e-7 span, inside the 2e-6 span allowance


def edge_case(which):
    """Weights whose rays sit on the edge of the gap rule, on d8_trained's rays.  'tie': depth rows 0 and 1 of the output layer equal, with equal
    biases — the two logits are the same number in every kernel, the gap is exactly 0; every 16th ray has near = far (span 0: gap = allowance = 0,
    and a comparison that is not finite).  'near': the biases TIE_EPS apart — 0 < gap <= 2e-6 span."""
    W, b, skips, rays = case('d8_trained')
    W = [x.copy() for x in W]; b = [x.copy() for x in b]; rays = rays.copy()
    W[-1][1] = W[-1][0]
    b[-1][1] = b[-1][0] + (np.float32(TIE_EPS) if which == 'near' else np.float32(0))
    if which == 'tie':
        rays[::16, 6] = 0.5; rays[::16, 7] = 0.5
    return W, b, skips, rays


SAT_GAINS = {'x300': 300.0, 'x70': 70.0}      # x300: test_sampler_fp16_range_is_defined's net, every ray beyond the limit; x70: the limit runs through the frame
SAT_BAND = 1e-3


def saturating_case(which, n=N_RAYS):
    """The sampler of test_sampler_fp16_range_is_defined (two hidden layers x gain, the output layer / gain^2) on n rays of a 40 x 52 frame, chosen on the
    reference's own norms so that as few as possible lie within SAT_BAND of the fp16 limit -> (W, b, skips, rays)."""
    key = ('sat', which, n)
    if key not in _CACHE:
        from oracle import synth
        gain = SAT_GAINS[which]
        w = synth.make_weights(0, 'trained')['sampler']
        W = [x.copy() for x in w['W']]; b = [x.copy() for x in w['b']]
        W[2] = W[2] * np.float32(gain); W[3] = W[3] * np.float32(gain); W[-1] = W[-1] / np.float32(gain * gain)
        rays = scene_rays(0, 40, 52)
        norm = pass1(W, b, (), rays)['S'].max((0, 1))
        order = np.argsort(np.abs(norm / OVF2 - 1.0) <= SAT_BAND, kind='stable')[:n]      # rays outside the band first, in frame order
        _CACHE[key] = (W, b, (), rays[np.sort(order)])
    return _CACHE[key]


