"""Integer networks with exact answers, for the MLP engines of the render path (a plain helper module of the suite).

A net whose weights, biases and inputs are small integers has an answer that every engine must reproduce EXACTLY: every operand is
exactly representable in the engine's operand type (bf16: integers up to 256; fp16: up to 2048) and every partial sum stays below 2^24,
so fp32 accumulation is exact in any order.  A kernel that reads one weight from the wrong row, column, K chunk or bias slot then
produces a wrong integer, however small the slip.  ``certify_*`` assert these conditions for a given input set; the reference values
are the oracle's own forward (``orc.nerf_forward``, ``orc.nerfcls_forward``, ``orc.mlp_elu_backbone``) in float64.

How the pieces are made exact:
  * NeRF nets (ReLU): integer ``pts``; at layer 0 and at the NeRF class's skip re-entry only the raw x, y, z columns carry weight, so
    the non-integer sin / cos columns meet zero weights.  With ``live = c`` coordinate c is held at 0 in every sample and in every view
    direction, and its sin / cos columns carry weight too: sin(0) = 0 and cos(0) = 1 exactly (nerf16_kernel's ``pe_sincos_scaled`` takes
    v_sin / v_cos of fract(0) = 0, and its double-angle step gives 2 * 0 * 1 = 0 and (1 - 0) (1 + 0) = 1).  View directions are
    +-axis unit vectors (the kernel reads them from rays[:, 8:11]).  The NeRF class's feature_linear is folded into its view layer by
    the packer (pnrf_pack.hip, E89: Wv[:, :256] @ Wf, bv + Wv[:, :256] @ bf); the folded matrix is an operand and is certified too.
  * ELU nets (refine, sampler): every hidden pre-activation is >= 0, so ELU is the identity.  The generator guarantees it for every
    input in the box the inputs are drawn from (interval bounds per unit, bias lifted to the lower bound); the certificate checks it
    on the actual values.
  * Refine nets: the packer stores a refine net for activations on the log2(e) scale (pnrf_pack.hip ``scale_for_elu``: first-layer
    weights and every ELU layer's bias times log2(e), output-layer weights over log2(e), in double, then rounded to the stream's type).
    An integer refine net ``{'W', 'b'}`` here is the net the kernels evaluate on that scale; ``refine_pack_weights`` gives the fp32
    weights that the packer turns into exactly these integers.  On the ELU identity region both describe the same function.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import pronerf_oracle as orc
from pronerf_amd import synthetic as synth

LOG2E = 1.4426950408889634074          # LOG2E_D of pnrf_engine.h (the packer's scale of the refine streams)
LIM = {'bf16': 256, 'f16': 2048, 'f32': 2 ** 24}
ACC_MAX = 2 ** 24                      # |partial sum| < 2^24: fp32 accumulation exact in any order
S = synth.N_SAMPLES
MULTIRES, MULTIRES_V = synth.MULTIRES, synth.MULTIRES_VIEWS
# refine-stage comparisons (z, pts, rgb0 against fp64): stated and derived in tests/test_exact_stages_gpu.py
TOL_Z = 2.0 ** -20
MARGIN = 50.0                          # a logit off by +-1 must move some z by more than MARGIN * TOL_Z
LOGIT_MAX, OFFSET_MAX = 6, 2           # |y[0:8]| <= 6, |y[8:32]| <= 2 (tanh(2) - tanh(1) = 0.2: offsets stay sensitive too)

# ---- what tests/test_exact_stages_gpu.py runs (tests/test_exact_nets_cpu.py certifies the same sets)
NERF_DEPTHS = (3, 4, 5, 6, 7, 8)
REFINE_CONFIGS = ((1, 2), (2, 32), (3, 3), (4, 6), (5, 2), (6, 3), (7, 6), (8, 32))     # (num_neighbor, mmnetdepth)
REFINE_BIG = (4, 6)                    # the configuration that also runs the AUTO switch and the multi-batch count
CU_CERT = 256                          # the CPU test certifies the input sets of a device with up to this many CUs


def nerf_counts(cus):
    """Ray counts of the NeRF stage: around the 16-ray (wide: 32-ray) batch edges, the AUTO switch +-1 (narrow while 8 n <= 128 CUs) and
    one count with more wide batches (256 rows) than workgroups."""
    sw = 16 * cus
    return [1, 15, 16, 17, 31, 32, 33, sw - 1, sw, sw + 1, 32 * cus + 5]


def refine_counts(cus, big=True):
    """Ray counts of the refine stage: around the 128 / 256-ray batch edges; big: the AUTO switch +-1 (narrow while n <= 128 CUs) and
    one count with more wide batches (256 rays) than workgroups."""
    small = [1, 127, 128, 129, 255, 256, 257]
    sw = 128 * cus
    return small + [sw - 1, sw, sw + 1, 256 * cus + 3] if big else small


MLP_COUNTS = (1, 127, 128, 129, 333)


def pe_cols(c, n_freq):
    """Columns of coordinate c's sin / cos in [x, sin(2^k x), cos(2^k x)]_k (orc.posenc)."""
    return [3 + 6 * k + c for k in range(n_freq)] + [3 + 6 * k + 3 + c for k in range(n_freq)]


def _rows(rs, fo, cols, nnz, vals):
    """[fo, max(cols) + 1] with ``nnz`` distinct nonzero columns per row drawn from ``cols``, values from ``vals``."""
    cols = np.asarray(cols)
    W = np.zeros((fo, int(cols.max()) + 1))
    for r in range(fo):
        k = min(nnz, len(cols))
        W[r, rs.choice(cols, k, replace=False)] = rs.choice(vals, k)
    return W


def _pad(W, fi):
    out = np.zeros((W.shape[0], fi))
    out[:, :W.shape[1]] = W
    return out


# ----------------------------------------------------------------------------------------------- NeRF nets (ReLU)
def _first(rs, fo, fi, live, vals=(-2, -1, 1, 2, 3)):
    """Layer-0 weights over the raw x, y, z columns (all three, small integers), plus coordinate ``live``'s sin / cos columns."""
    W = np.zeros((fo, fi))
    W[:, :3] = rs.choice(vals, (fo, 3)) * (rs.rand(fo, 3) < 0.8)
    if live is not None:
        W[:, :63] += _pad(_rows(rs, fo, pe_cols(live, MULTIRES), 2, (-1, 1, 2)), 63)
    return W


def _hidden(rs, fo, fi, col0=0):
    """+1 on one unit, -1 on another, +1 on a third for some rows: sparse, asymmetric, activations stay small.  The +1 sources run
    through a permutation, so that every unit of the layer below is read."""
    W = np.zeros((fo, fi))
    perm = rs.permutation(np.tile(np.arange(fi - col0), fo // (fi - col0) + 1))
    for r in range(fo):
        a = perm[r] + col0
        b, c = rs.choice(np.delete(np.arange(col0, fi), a - col0), 2, replace=False)
        W[r, a] += 1; W[r, b] -= 1
        if rs.rand() < 0.3:
            W[r, c] += 1
    return W


def _dense(rs, fo, fi, vals):
    """Every input unit read by exactly one of the fo rows, with a weight from vals."""
    W = np.zeros((fo, fi))
    W[rs.randint(0, fo, fi), np.arange(fi)] = rs.choice(vals, fi)
    return W


def _views(rs, fo, col0, live):
    """Weights on the 27 view-embedding columns starting at col0: the raw direction (all three), plus ``live``'s sin / cos."""
    W = np.zeros((fo, col0 + 27))
    W[:, col0:col0 + 3] = rs.randint(-2, 3, (fo, 3))
    if live is not None:
        W[:, col0:] += _pad(_rows(rs, fo, pe_cols(live, MULTIRES_V), 2, (-1, 1, 2)), 27)
    return W


def _bias(rs, fo, lo=-1, hi=2):
    return rs.randint(lo, hi + 1, fo).astype(np.float64)


def nerf_net(netdepth, seed=0, live=None):
    """DoNeRFTRT(D = netdepth) with integer weights: {'W': [...], 'b': [...]} in float64, layer dims of synthetic.nerf_layer_dims."""
    rs = np.random.RandomState(9001 * netdepth + 17 * seed + (0 if live is None else 1 + live))
    dims = synth.nerf_layer_dims(netdepth)
    Ws, bs = [], []
    for i, (fi, fo) in enumerate(dims):
        if i == 0:
            W = _first(rs, fo, fi, live)
        elif i < len(dims) - 1:
            W = _hidden(rs, fo, fi)
        else:
            W = _pad(_dense(rs, fo, 256, (-1, 1, 2)), fi) + _views(rs, fo, 256, live)
        Ws.append(W); bs.append(_bias(rs, fo))
    return {'W': Ws, 'b': bs}


def nerfcls_net(seed=0, live=None):
    """The NeRF class (D = 8, skips = [4], use_viewdirs) with integer weights, by name as synthetic.make_nerfcls_weights."""
    rs = np.random.RandomState(7717 + 17 * seed + (0 if live is None else 1 + live))
    t = synth.nerfcls_layer_dims()
    pts = []
    for i, (fi, fo) in enumerate(t['pts_linears']):
        if i == 0:
            W = _first(rs, fo, fi, live)
        elif fi == 256 + 63:                    # skip re-entry: cat[pts(63), h(256)]
            W = _hidden(rs, fo, fi, col0=63) + _first(rs, fo, fi, live, vals=(-1, 1, 2))
        else:
            W = _hidden(rs, fo, fi)
        pts.append((W, _bias(rs, fo)))
    Wf = _pad(_rows(rs, 256, np.arange(256), 2, (-1, 1)), 256)
    Wa = _pad(_rows(rs, 1, np.arange(256), 64, (-1, 1, 2)), 256)
    Wv = _pad(_rows(rs, 128, np.arange(256), 2, (-1, 1)), 256 + 27) + _views(rs, 128, 256, live)
    Wr = _dense(rs, 3, 128, (-1, 1, 2))
    return {'pts_linears': pts, 'feature_linear': (Wf, _bias(rs, 256, -2, 2)), 'alpha_linear': (Wa, _bias(rs, 1)),
            'views_linears': [(Wv, _bias(rs, 128))], 'rgb_linear': (Wr, _bias(rs, 3))}


def nerfcls_pack_order(w):
    """NeRF-class weights as the 12 layers pnrf_mlp_pack takes (pts0..7, feature, alpha, views, rgb)."""
    L = list(w['pts_linears']) + [w['feature_linear'], w['alpha_linear'], w['views_linears'][0], w['rgb_linear']]
    return [W for W, _ in L], [b for _, b in L]


def nerf_inputs(n, seed=0, live=None, n_samples=S):
    """pts [n, S, 3] (integers in [-4, 4]; coordinate ``live`` = 0), rays [n, 11] (o, d in [-1, 1]; near 0, far 1; view direction a
    +-axis unit vector, never along ``live``), z [n, S] ascending in (0, 1), add in [-1, 1], mul in [0, 1.5] — float32 numpy."""
    rs = np.random.RandomState(31337 + 101 * seed + (0 if live is None else 1 + live))
    pts = rs.randint(-4, 5, (n, n_samples, 3)).astype(np.float32)
    axes = [a for a in range(3) if a != live]
    view = np.zeros((n, 3), np.float32)
    view[np.arange(n), rs.choice(axes, n)] = rs.choice((-1.0, 1.0), n)
    if live is not None:
        pts[..., live] = 0.0
    rays = np.concatenate([rs.uniform(-1, 1, (n, 6)), np.zeros((n, 1)), np.ones((n, 1)), view], 1).astype(np.float32)
    z = np.sort(rs.uniform(0.02, 0.98, (n, n_samples)), 1).astype(np.float32)
    add = rs.uniform(-1, 1, (n, n_samples)).astype(np.float32)
    mul = rs.uniform(0, 1.5, (n, n_samples)).astype(np.float32)
    return {'pts': pts, 'rays': rays, 'z': z, 'add': add, 'mul': mul}


def nerf_embed(inp):
    """(emb_pts [n S, 63], emb_dirs [n S, 27]) in float64, as the oracle builds them (orc.posenc)."""
    n, s = inp['pts'].shape[:2]
    p = torch.from_numpy(inp['pts'].reshape(-1, 3)).double()
    v = torch.from_numpy(inp['rays'][:, 8:11]).double()[:, None, :].expand(-1, s, -1).reshape(-1, 3)
    return orc.posenc(p, MULTIRES), orc.posenc(v, MULTIRES_V)


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def nerf_reference(kind, w, inp):
    """raw [n, S, 4] in float64: orc.nerf_forward (kind 'nerf') or orc.nerfcls_forward (kind 'nerfcls') on float64 tensors."""
    n, s = inp['pts'].shape[:2]
    e, ev = nerf_embed(inp)
    if kind == 'nerf':
        out = orc.nerf_forward({'W': [_t64(W) for W in w['W']], 'b': [_t64(b) for b in w['b']]}, e, ev)
    else:
        t = lambda p: (_t64(p[0]), _t64(p[1]))
        w64 = {'pts_linears': [t(p) for p in w['pts_linears']], 'views_linears': [t(w['views_linears'][0])],
               **{k: t(w[k]) for k in ('feature_linear', 'alpha_linear', 'rgb_linear')}}
        out = orc.nerfcls_forward(w64, torch.cat([e, ev], -1))
    return out.numpy().reshape(n, s, 4)


# ----------------------------------------------------------------------------------------------- certificate
def _is_int(a):
    return bool(np.all(np.isfinite(a)) and np.all(a == np.round(a)))


def check_layer(x, W, b, lim, what, elu=False):
    """One product y = x W^T + b of an engine: asserts that every operand meeting a nonzero weight is an integer of magnitude <= lim,
    that W and b are integers (|W| <= lim), that every partial sum, in any order, stays below 2^24, and (elu) that every pre-activation
    is >= 0.  Returns y (float64)."""
    x = np.asarray(x, np.float64); W = np.asarray(W, np.float64); b = np.asarray(b, np.float64)
    live = np.any(W != 0, axis=0)
    xs, Ws = x[:, live], W[:, live]
    assert _is_int(xs), f'{what}: a non-integer operand meets a nonzero weight'
    assert np.abs(xs).max(initial=0) <= lim, f'{what}: operand {np.abs(xs).max()} > {lim}'
    assert _is_int(W) and np.abs(W).max(initial=0) <= lim, f'{what}: weights not integers within {lim}'
    assert _is_int(b), f'{what}: bias not integer'
    bound = np.abs(xs) @ np.abs(Ws).T + np.abs(b)
    assert bound.max(initial=0) < ACC_MAX, f'{what}: partial sums up to {bound.max()} >= 2^24'
    y = x @ W.T + b
    if elu:
        assert y.min(initial=0) >= 0, f'{what}: pre-activation {y.min()} < 0 (ELU is the identity only on >= 0)'
    return y


def certify_nerf(kind, w, inp, lim=LIM['bf16']):
    """Walks the engine's layer sequence (NeRF class: with the packer's feature fold) checking every product; asserts that the walk
    reproduces the oracle's float64 raw and returns that raw [n, S, 4]."""
    n, s = inp['pts'].shape[:2]
    e, ev = (t.numpy() for t in nerf_embed(inp))
    if kind == 'nerf':
        h = e
        for i, (W, b) in enumerate(zip(w['W'], w['b'])):
            last = i == len(w['W']) - 1
            if last:
                h = np.concatenate([h, ev], 1)
            h = check_layer(h, W, b, lim, f'layer {i}')
            if not last:
                h = np.maximum(h, 0)
        raw = h
    else:
        h = e
        for i, (W, b) in enumerate(w['pts_linears']):
            h = np.maximum(check_layer(h, W, b, lim, f'pts_linears.{i}'), 0)
            if i == 4:
                h = np.concatenate([e, h], 1)
        (Wf, bf), (Wa, ba), (Wv, bv), (Wr, br) = w['feature_linear'], w['alpha_linear'], w['views_linears'][0], w['rgb_linear']
        Wc = np.concatenate([Wv[:, :256] @ Wf, Wv[:, 256:]], 1)                      # the packer's fold (pnrf_pack.hip E89)
        bc = bv + Wv[:, :256] @ bf
        alpha = check_layer(h, Wa, ba, lim, 'alpha_linear')
        hv = np.maximum(check_layer(np.concatenate([h, ev], 1), Wc, bc, lim, 'views_linears.0 (feature folded)'), 0)
        raw = np.concatenate([check_layer(hv, Wr, br, lim, 'rgb_linear'), alpha], 1)
    raw = raw.reshape(n, s, 4)
    ref = nerf_reference(kind, w, inp)
    np.testing.assert_array_equal(raw, ref)
    assert _is_int(ref) and np.abs(ref).max() < ACC_MAX
    return ref


# ----------------------------------------------------------------------------------------------- ELU nets (refine, sampler)
def _elu_net(rs, dims, in_lo, in_hi, lim, head, scaled=False):
    """Integer ELU net (dims = [in, hidden..., out]) whose hidden pre-activations are >= 0 for EVERY input in [in_lo, in_hi]^in.
    Interval bounds are carried per unit: a row draws a few +-1 / +2 weights, its bias is lifted to the row's lower bound (plus 0..2),
    rows whose upper bound passes cap are redrawn or fall back to copying one unit.  A quarter of the units are 'narrow' (upper - lower
    <= 4, built from narrow units only), so the output rows can be centred into small ranges.  head(rs, lo, hi, narrow) -> (W, b) of
    the output layer."""
    cap = min(lim, 200)
    lo = np.full(dims[0], float(in_lo)); hi = np.full(dims[0], float(in_hi))
    narrow = np.ones(dims[0], bool)                          # the inputs span 2: narrow
    Ws, bs = [], []
    for fi, fo in zip(dims[:-2], dims[1:-1]):
        W = np.zeros((fo, fi)); b = np.zeros(fo); nlo = np.zeros(fo); nhi = np.zeros(fo)
        nar = rs.rand(fo) < 0.25
        pool_n = np.flatnonzero(narrow)
        perm = rs.permutation(np.tile(np.arange(fi), fo // fi + 1))
        for r in range(fo):
            pool = pool_n if nar[r] else np.arange(fi)
            wcap = 4 if nar[r] else cap
            for attempt in range(8):
                k = rs.randint(1, 4) if not nar[r] else rs.randint(1, 3)
                cols = rs.choice(pool, min(k, len(pool)), replace=False)
                if not nar[r] and perm[r] not in cols:
                    cols[0] = perm[r]                              # every unit below is read by some wide row
                vals = rs.choice((-1, 1, 1, 2), len(cols)) if not nar[r] else rs.choice((-1, 1), len(cols))
                l0 = np.sum(np.where(vals > 0, vals * lo[cols], vals * hi[cols]))
                h0 = np.sum(np.where(vals > 0, vals * hi[cols], vals * lo[cols]))
                bias = -l0 + rs.randint(0, 3)
                if h0 + bias <= cap and h0 - l0 <= wcap:
                    break
            else:
                cols = rs.choice(pool, 1); vals = np.array([1.0]); l0, h0 = lo[cols[0]], hi[cols[0]]; bias = 0.0
            while scaled and not _has_pre_image(bias, LOG2E):     # (a bias that no float32 / log2(e) reproduces: lift it by one)
                bias += 1
            W[r, cols] = vals; b[r] = bias; nlo[r] = l0 + bias; nhi[r] = h0 + bias
        assert nlo.min() >= 0 and nhi.max() <= lim
        Ws.append(W); bs.append(b)
        lo, hi, narrow = nlo, nhi, (nhi - nlo) <= 4
    W, b = head(rs, lo, hi, narrow)
    Ws.append(W); bs.append(b)
    return {'W': Ws, 'b': bs, 'in_box': (in_lo, in_hi)}


def _centred(rs, lo, hi, narrow, n_units, half_width):
    """One output row on up to n_units narrow units, weights +-1, bias centring it: every value in [-half_width, half_width]."""
    fi = len(lo)
    pool = np.flatnonzero(narrow & ((hi - lo) <= 2 * half_width))
    w = np.zeros(fi)
    if len(pool):
        for c in rs.choice(pool, min(n_units, len(pool)), replace=False):
            s = rs.choice((-1.0, 1.0))
            if np.sum(np.abs(w) * (hi - lo)) + (hi[c] - lo[c]) <= 2 * half_width:
                w[c] = s
    l0 = np.sum(np.where(w > 0, w * lo, w * hi)); h0 = np.sum(np.where(w > 0, w * hi, w * lo))
    bias = -np.floor((l0 + h0) / 2)
    assert l0 + bias >= -half_width and h0 + bias <= half_width
    return w, bias


def _refine_head(rs, lo, hi, narrow):
    fi = len(lo)
    W = np.zeros((35, fi)); b = np.zeros(35)
    for o in range(35):
        if o < 8:
            W[o], b[o] = _centred(rs, lo, hi, narrow, 3, LOGIT_MAX)
        elif o < 32:
            W[o], b[o] = _centred(rs, lo, hi, narrow, 1, OFFSET_MAX)
    W[32:35] = _dense(rs, 3, fi, (-1, 1))                  # rgb0 logits read every unit of the last hidden layer
    return W, b


def refine_net(nb, mmnetdepth, seed=0):
    """Integer refine net (MinMaxRayEpiSamplerTRT_Net: 48 + 24 nb -> mmnetdepth x 256 ELU -> 35) on the kernels' log2(e) scale (module
    docstring); inputs in [0, 2].  Output logits: y[0:8] in [-6, 6], y[8:32] in [-2, 2] for every input in the box; y[32:35] (the rgb0 head) reads every last hidden unit."""
    rs = np.random.RandomState(5003 * nb + 61 * mmnetdepth + seed)
    dims = [6 * S + 3 * nb * S] + [256] * mmnetdepth + [4 * S + 3]
    return _elu_net(rs, dims, 0, 2, LIM['bf16'], _refine_head, scaled=True)


def sampler_net(mmnetdepth=synth.MMNETDEPTH, seed=0):
    """Integer sampler net (MinMaxRay_Net: 288 -> mmnetdepth x 256 ELU -> 27) for the exact-fp32 module-level kernel; inputs in [0, 2]."""
    rs = np.random.RandomState(4001 + 61 * mmnetdepth + seed)
    dims = [6 * synth.N_POINT_RAY_ENC] + [256] * mmnetdepth + [3 * S + 3]

    def head(rs, lo, hi, narrow):
        W = _hidden(rs, 27, len(lo)) * rs.choice((1, 2, 3), (27, 1))
        return W, _bias(rs, 27, -5, 5)
    return _elu_net(rs, dims, 0, 2, LIM['f32'], head)


def _has_pre_image(k, scale):
    w = np.float32(k / scale)
    return any(np.float32(np.float64(v) * scale) == k for v in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf))))


def _pre_image(k, scale):
    """float32 w with float32(float64(w) * scale) == k exactly, elementwise (the packer's (float)((double) W * wscale))."""
    k = np.asarray(k, np.float64)
    w = (k / scale).astype(np.float32)
    img = lambda v: (v.astype(np.float64) * scale).astype(np.float32)
    ok = img(w) == k
    for step in (1, -1, 2, -2, 3, -3):
        cand = w.copy()
        toward = np.float32(np.inf) if step > 0 else np.float32(-np.inf)
        for _ in range(abs(step)):
            cand = np.nextafter(cand, toward)
        hit = ~ok & (img(cand) == k)
        w = np.where(hit, cand, w); ok |= hit
    assert ok.all(), 'no float32 pre-image for some integer'
    return w


def refine_pack_weights(net):
    """fp32 weights / biases to hand pnrf_mlp_pack so that the stored refine streams hold exactly the integers of ``net``: first-layer
    W and ELU biases / log2(e), output-layer W * log2(e) (inverting pnrf_pack.hip scale_for_elu), hidden W and the output bias as they are."""
    Ws, bs, L = net['W'], net['b'], len(net['W'])
    outW, outb = [], []
    for l in range(L):
        W, b = Ws[l], bs[l]
        if l == 0:
            W = _pre_image(W, LOG2E)
        elif l == L - 1:
            W = _pre_image(W, 1.0 / LOG2E)
        if l < L - 1:
            b = _pre_image(b, LOG2E)
        outW.append(np.asarray(W, np.float32)); outb.append(np.asarray(b, np.float32))
    return outW, outb


def elu_inputs(n, in_dim, seed=0):
    """Integer inputs in the box [0, 2] of the ELU nets, float32 [n, in_dim]."""
    return np.random.RandomState(271 + seed + 7 * in_dim).randint(0, 3, (n, in_dim)).astype(np.float32)


def elu_reference(net, x):
    """orc.mlp_elu_backbone in float64: y [n, out]."""
    return orc.mlp_elu_backbone(torch.from_numpy(np.asarray(x, np.float64)), [_t64(W) for W in net['W']], [_t64(b) for b in net['b']]).numpy()


def certify_elu(net, x, lim):
    """Checks every product of an ELU net on inputs x (integers, pre-activations >= 0, representable, sums < 2^24); asserts that the walk
    equals the oracle's float64 forward and returns it."""
    h = np.asarray(x, np.float64)
    L = len(net['W'])
    for l in range(L):
        h = check_layer(h, net['W'][l], net['b'][l], lim, f'layer {l}', elu=l < L - 1)
    ref = elu_reference(net, x)
    np.testing.assert_array_equal(h, ref)
    return ref


def refine_rays(n, seed=0):
    """rays [n, 11] (o, d in [-1, 1], near 0, far 1) and well-separated depth_sorted [n, 8] ((k + 0.5) / 8 +- 0.02), float32."""
    rs = np.random.RandomState(8191 + seed)
    rays = np.concatenate([rs.uniform(-1, 1, (n, 6)), np.zeros((n, 1)), np.ones((n, 1)), rs.uniform(-1, 1, (n, 3))], 1).astype(np.float32)
    ds = ((np.arange(S) + 0.5) / S + rs.uniform(-0.02, 0.02, (n, S))).astype(np.float32)
    return rays, ds


def _sig(x):
    return np.exp(-np.logaddexp(0.0, -x))


def refine_reference(y, rays, ds):
    """z [n, 8], pts [n, 8, 3], rgb0 [n, 3] in float64 from the exact logits y: orc.interval_refine(sigmoid(y[0:8])), o + d z + 0.01 tanh."""
    y = np.asarray(y, np.float64); r = np.asarray(rays, np.float64)
    n = y.shape[0]
    z = orc.interval_refine(torch.from_numpy(np.asarray(ds, np.float64)), torch.from_numpy(_sig(y[:, :S])),
                            torch.from_numpy(r[:, 6:7]), torch.from_numpy(r[:, 7:8])).numpy()
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., None] + 1e-2 * np.tanh(y[:, S:4 * S]).reshape(n, S, 3)
    return z, pts, _sig(y[:, 4 * S:])


def refine_margin(y, rays, ds):
    """Smallest |z(y +- 1) - z(y)| over every ray, sample and sign (float64): how far the smallest slip of a logit moves a depth."""
    z0 = refine_reference(y, rays, ds)[0]
    m = np.inf
    for d in (1.0, -1.0):
        y1 = np.array(y, np.float64); y1[:, :S] += d
        m = min(m, float(np.abs(refine_reference(y1, rays, ds)[0] - z0).min()))
    return m


def assert_refine_margin(y, rays, ds):
    y = np.asarray(y)
    assert np.abs(y[:, :S]).max() <= LOGIT_MAX and np.abs(y[:, S:4 * S]).max() <= OFFSET_MAX
    m = refine_margin(y, rays, ds)
    assert m > MARGIN * TOL_Z, f'a logit slip of 1 moves z by only {m:.3g} (<= {MARGIN} x {TOL_Z:.3g})'
    return m


def mutate(w_list, layer, seed=0):
    """Copy of a weight list with one entry of ``layer`` changed by +1: a nonzero-column entry of a row, so that it meets live operands."""
    rs = np.random.RandomState(123 + seed)
    out = [np.array(W, np.float64, copy=True) for W in w_list]
    W = out[layer]
    r, c = np.argwhere(W != 0)[rs.randint(np.count_nonzero(W))]
    W[r, c] += 1
    return out, (layer, int(r), int(c))
