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


# ----------------------------------------------------------------------------------------------- training nets (pnrf_trainer_net_fwd_bwd)
# What tests/test_exact_train_gpu.py runs (tests/test_exact_train_cpu.py certifies the same sets).  The trainer holds the three nets as plain
# integer nets: its ELU is expm1f on the pre-activation (no log2(e) scale), so the refine net is refine_net's {'W', 'b'} as they are.
TRAIN_LIVE = 1                         # the fine net's live coordinate (0 in every sample and view direction)
TRAIN_MAX_RAYS, TRAIN_BIG = 12800, (1024, 256)          # the two trainers: (max_rays, max_samples 8) and (max_rays, max_samples)
ELU_COUNTS = (1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 12800)
NERF_S8 = (1023, 1024, 1025, 1287, 4096, 4097, 8192, 8193)             # rays at S = 8: 8184 .. 65 544 rows
NERF_BIG = ((64, 127), (64, 129), (64, 512), (256, 128), (256, 256), (256, 257))   # (S, rays) on the large trainer: 8128 .. 65 792 rows
NERF_ONEHOT = (8, 4101)                # S, rays of the one-hot case: 32 808 rows (past 32 768)
E_SIN = 2.0 ** -22                     # |sinf / cosf - sin / cos| of the embedding kernel (<= 2 ulp of a value <= 1), with a factor 2
DY_NNZ = 384                           # nonzero rows of an output gradient over many rows: the weight-gradient sums stay below 2^24


def nerf_cu_rays(cus):
    """Rays at S = 8 whose 128-row batches outnumber the CUs, with a ragged last batch: 128 cus + 40 rows."""
    return 16 * cus + 5


def train_nets(live=TRAIN_LIVE):
    """The trainer's 26 (W, b) in float64: sampler_net(), refine_net(4, 6) as plain integers, nerfcls_net(live) in pack order (pts0 .. 7,
    feature, alpha, views, rgb)."""
    s, r = sampler_net(), refine_net(4, synth.MMNETDEPTH)
    Wn, bn = nerfcls_pack_order(nerfcls_net(live=live))
    return list(s['W']) + list(r['W']) + Wn, list(s['b']) + list(r['b']) + bn


def train_dy(rows, width, seed=0, nnz=DY_NNZ, big=(2049, -2051, 3001)):
    """Integer output gradient [rows, width] (float32): every fifth row zero; of the others a quarter mix one large entry (``big``: more than
    the 11 bits of the fp16 hi plane) with +-1 entries, the rest are small integers in [-3, 3].  nnz: only that many nonzero rows (spread over
    the set, the first and the last row among them), so that the weight-gradient sums over many rows stay below 2^24."""
    rs = np.random.RandomState(6007 + 31 * seed + width)
    dy = rs.randint(-3, 4, (rows, width)).astype(np.float64)
    mix = rs.rand(rows) < 0.25
    dy[mix] = rs.choice((-1.0, 0.0, 1.0), (int(mix.sum()), width))
    dy[mix, rs.randint(0, width, int(mix.sum()))] = rs.choice(big, int(mix.sum()))
    dy[::5] = 0.0
    if nnz is not None and nnz < rows:
        keep = np.zeros(rows, bool)
        keep[np.linspace(0, rows - 1, nnz).astype(np.int64)] = True
        dy[~keep] = 0.0
        dy[[0, rows - 1]] = rs.choice((-2.0, -1.0, 1.0, 2.0), (2, width))
    return dy.astype(np.float32)


def onehot_rows(rows):
    """Rows of the one-hot output gradient: the first, the last, and those on each side of a 128-row and a 32 768-row boundary."""
    cand = [0, rows - 1, 127, 128, 32767, 32768]
    return sorted({r for r in cand if 0 <= r < rows})


def hg_scale_for(mx):
    """pnrf_hgemm.h hg_scale_for: the power of two s with s mx in [2^11, 2^12) (mx = 0 or non-finite: 1).  Elementwise."""
    mx = np.asarray(mx, np.float64)
    ok = (mx > 0) & np.isfinite(mx)
    ex = np.frexp(np.where(ok, mx, 1.0))[1]
    return np.where(ok, np.ldexp(1.0, np.clip(12 - ex, -100, 100)), 1.0)


def split_exact(v, scale=1.0):
    """Does every v * scale survive the kernels' split into fp16 hi + 2^-11 fp16 lo exactly?  (hi = fp16(x), lo = fp16((x - hi) 2^11).)"""
    x = (np.asarray(v, np.float64) * scale).astype(np.float32)
    if not np.array_equal(x.astype(np.float64), np.asarray(v, np.float64) * scale):
        return False
    with np.errstate(over='ignore', invalid='ignore'):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
        back = hi.astype(np.float64) + lo.astype(np.float64) / 2048
    return bool(np.all(np.isfinite(back)) and np.array_equal(back, x.astype(np.float64)))


def _assert_split(v, scale, what):
    assert split_exact(v, scale), f'{what}: an operand does not survive the fp16 hi / lo split at scale {np.min(scale):.3g}'


def _pow2_floor(x):
    return np.ldexp(1.0, np.floor(np.log2(x)).astype(np.int64))


def _split_hgemm(dz, what):
    """A gradient operand of hgemm_kernel / dwh_*: one scale from the tensor's recorded maximum; the row-chain kernels take the scale of a
    workgroup's own rows, between that and the scale of each row's own maximum."""
    if not dz.size:
        return
    _assert_split(dz, hg_scale_for(np.abs(dz).max()), what)
    _assert_split(dz, hg_scale_for(np.abs(dz).max(1, keepdims=True)), what + ' (row scale)')


def _check_sums(bound, what):
    assert bound.max(initial=0) < ACC_MAX, f'{what}: sums of |terms| up to {bound.max()} >= 2^24'


# ---- ELU nets
def elu_train_reference(W, b, x, dy):
    """torch autograd in float64: y, [(dW, db)] per layer, and each layer's input X and output gradient dZ (float64 numpy)."""
    h = torch.from_numpy(np.asarray(x, np.float64))
    Wt = [_t64(w).requires_grad_() for w in W]; bt = [_t64(v).requires_grad_() for v in b]
    Xs, Zs = [], []
    for l in range(len(W)):
        Xs.append(h)
        z = torch.nn.functional.linear(h, Wt[l], bt[l])
        z.retain_grad(); Zs.append(z)
        h = torch.nn.functional.elu(z) if l < len(W) - 1 else z
    h.backward(_t64(dy))
    return (h.detach().numpy(), [(w.grad.numpy(), v.grad.numpy()) for w, v in zip(Wt, bt)],
            [X.detach().numpy() for X in Xs], [z.grad.numpy() for z in Zs])


def certify_elu_train(W, b, x, dy, lim=LIM['f32']):
    """Forward as certify_elu (pre-activations >= 0: ELU' = 1), then the backward: every dZ, dX, dW, db an integer; the input-gradient
    products (sum_k |dZ_k| |W_kj| per row) and the weight-gradient reductions over ALL rows (sum_r |dZ_r| |X_r|, db: sum_r |dZ_r|) below 2^24;
    every gradient operand survives the fp16 split at the scales the kernels can choose, every activation operand at scale 1.  Returns the
    reference (y, grads)."""
    h = np.asarray(x, np.float64)
    for l in range(len(W)):
        _assert_split(h, 1.0, f'layer {l} input')
        h = check_layer(h, W[l], b[l], lim, f'layer {l}', elu=l < len(W) - 1)
    y, grads, Xs, dZs = elu_train_reference(W, b, x, dy)
    np.testing.assert_array_equal(h, y)
    for l in range(len(W)):
        dz, X = dZs[l], Xs[l]
        assert _is_int(dz) and _is_int(grads[l][0]) and _is_int(grads[l][1]), f'layer {l}: non-integer gradient'
        _check_sums(np.abs(dz).T @ np.abs(X), f'layer {l} dW')
        _check_sums(np.abs(dz).sum(0), f'layer {l} db')
        if l:
            _check_sums(np.abs(dz) @ np.abs(W[l]), f'layer {l} dX')
        if l < len(W) - 1:                 # the output layer's gradient (dy) meets the exact-fp32 kernels only
            _split_hgemm(dz, f'layer {l} dZ')
    return y, grads


# ---- the fine net (NeRF class, trainer layout)
def _nerf_layers(Ws, bs, e, ev):
    """Trainer-order forward of the NeRF class on float64 tensors: (raw, [X_l], [Z_l]) for the 12 layers (pts0..7, feature, alpha, views, rgb)."""
    Xs, Zs = [None] * 12, [None] * 12

    def lin(l, X):
        Xs[l] = X
        Zs[l] = torch.nn.functional.linear(X, Ws[l], bs[l])
        return Zs[l]
    h = e
    for i in range(8):
        h = torch.relu(lin(i, h))
        if i == 4:
            h = torch.cat([e, h], -1)
    f = lin(8, h)
    a = lin(9, h)
    hv = torch.relu(lin(10, torch.cat([f, ev], -1)))
    rgb = lin(11, hv)
    return torch.cat([rgb, a], -1), Xs, Zs


class NerfTrainRef:
    """The fine net's forward / backward in float64 for one input set (pts [n, S, 3], rays [n, 11]) over its DISTINCT rows (integer points in a
    small box, axis view directions: a few thousand): activations X_l(u), pre-activations and the Jacobians d raw / d Z_l and d raw / d pts per
    distinct row u.  A row's gradients are then dy_r J(u_r) — exact in float64 — and a weight gradient sum_r dZ_r^T X(u_r) = sum_u (sum over
    u's rows of dZ_r)^T X(u): one reference per (net, row count) for any number of output gradients and kernel configurations."""

    def __init__(self, Ws, bs, inp):
        n, S = inp['pts'].shape[:2]
        self.R = n * S
        rows = np.concatenate([inp['pts'].reshape(-1, 3), np.repeat(inp['rays'][:, 8:11], S, 0)], 1).astype(np.float64)
        self.keys, self.inv = np.unique(rows, axis=0, return_inverse=True)
        self.inv = self.inv.reshape(-1)
        p = torch.from_numpy(self.keys[:, :3].copy()).requires_grad_()
        v = torch.from_numpy(self.keys[:, 3:].copy())
        self.W = [np.asarray(W, np.float64) for W in Ws]
        raw, Xs, Zs = _nerf_layers([_t64(W) for W in Ws], [_t64(x) for x in bs], orc.posenc(p, MULTIRES), orc.posenc(v, MULTIRES_V))
        for Z in Zs:
            Z.retain_grad()
        self.J, self.Jp = [[] for _ in range(12)], []
        for o in range(4):
            for Z in Zs:
                Z.grad = None
            p.grad = None
            raw[:, o].sum().backward(retain_graph=o < 3)
            for l in range(12):
                self.J[l].append(Zs[l].grad.numpy().copy())
            self.Jp.append(p.grad.numpy().copy())
        self.J = [np.stack(j) for j in self.J]                 # [4, U, out_l]
        self.Jp = np.stack(self.Jp)                            # [4, U, 3]
        self.X = [X.detach().numpy() for X in Xs]              # [U, in_l]
        self.raw_u = raw.detach().numpy()
        w = {'pts_linears': [(Ws[i], bs[i]) for i in range(8)], 'feature_linear': (Ws[8], bs[8]), 'alpha_linear': (Ws[9], bs[9]),
             'views_linears': [(Ws[10], bs[10])], 'rgb_linear': (Ws[11], bs[11])}
        t = lambda wb: (_t64(wb[0]), _t64(wb[1]))
        w64 = {'pts_linears': [t(x) for x in w['pts_linears']], 'views_linears': [t(w['views_linears'][0])],
               **{k: t(w[k]) for k in ('feature_linear', 'alpha_linear', 'rgb_linear')}}
        e, ev = orc.posenc(p.detach(), MULTIRES), orc.posenc(v, MULTIRES_V)
        np.testing.assert_array_equal(self.raw_u, orc.nerfcls_forward(w64, torch.cat([e, ev], -1)).numpy())   # the trainer layout is the oracle's net

    def raw(self):
        return self.raw_u[self.inv]

    def dz(self, l, dy, rows=None):
        """dZ_l per row [R, out_l] for the output gradient dy [R, 4]; rows: only those rows (dy [len(rows), 4])."""
        inv = self.inv if rows is None else self.inv[rows]
        return np.einsum('ro,oru->ru', np.asarray(dy, np.float64), self.J[l][:, inv])

    def grads(self, dy):
        """[(dW_l, db_l)] for the 12 layers and d_pts [R, 3]."""
        dy = np.asarray(dy, np.float64)
        agg = np.zeros((len(self.keys), 4))
        np.add.at(agg, self.inv, dy)
        out = []
        for l in range(12):
            A = np.einsum('uo,ouj->uj', agg, self.J[l])
            out.append((A.T @ self.X[l], A.sum(0)))
        return out, np.einsum('ro,orc->rc', dy, self.Jp[:, self.inv])

    def exact_cols(self, l):
        """Columns of layer l's weight gradient that are exact: those whose input column holds integers in every row (the raw coordinates,
        sin / cos of a coordinate that is 0, every hidden column); the others meet sin / cos of non-zero coordinates."""
        X = self.X[l]
        return np.all(X == np.round(X), axis=0)


def _tb_cmax(Ws):
    """tchain_norms_body: largest column sum of squares per backward stream layer (views^T feature columns, [feature; alpha]^T, pts7^T ..
    pts1^T, pts5^T over its hidden columns)."""
    W = [np.asarray(w, np.float64) for w in Ws]
    cm = [(W[10][:, :256] ** 2).sum(0).max(), (np.concatenate([W[8], W[9]], 0) ** 2).sum(0).max()]
    for L in (7, 6, 5, 4, 3, 2, 1):
        cm.append(((W[L][:, 63:] if L == 5 else W[L]) ** 2).sum(0).max())
    return cm


def certify_nerf_train(ref, dy, what=''):
    """Certificate of one fine-net call (forward on the distinct rows, backward per row for dy [R, 4]):
      * forward: every product integer, representable, partial sums < 2^24 (check_layer), every activation operand survives the split at scale 1;
      * every dZ_l, dX_l (= dZ_l W_l), dW_l, db_l an integer (dW: on the exact columns), the input-gradient sums sum_k |dZ_k| |W_kj| per row and
        the weight-gradient sums sum_r |dZ_r| |X_r| over ALL R rows (exact columns; db: sum_r |dZ_r|) below 2^24;
      * every gradient operand survives the split: at the tensor-maximum scale (hgemm_kernel, dwh_*) and at the engine backward's per-row scales —
        the row maximum into [2^13, 2^14), then per layer the SMALLEST factor t its norm bound allows (sqrt(n2 cmax) t >= 2^12, one binade below
        the kernel's choice for the fp32 rounding of n2) and the largest (sqrt(n2 cmax) t < 2^14).
    Returns (raw, grads, d_pts) of the reference."""
    Ws = ref.W
    for l in range(12):
        fi = Ws[l].shape[1]
        X = ref.X[l]
        check_layer(X, Ws[l], np.zeros(Ws[l].shape[0]), LIM['f16'], f'{what} fwd layer {l}')
        _assert_split(X[:, np.any(Ws[l] != 0, axis=0)], 1.0, f'{what} fwd layer {l} input')
        assert X.shape[1] == fi
    dy = np.asarray(dy, np.float64)
    assert _is_int(dy)
    grads, dpts = ref.grads(dy)
    cm = _tb_cmax(Ws)
    rows = np.flatnonzero(np.any(dy != 0, 1))          # a row whose dy is 0 has dZ = 0 in every layer: no term, nothing to split
    inv = ref.inv[rows]
    dzs = {}
    for l in range(12):
        dz = ref.dz(l, dy[rows], rows)
        dzs[l] = dz
        assert _is_int(dz), f'{what} layer {l}: non-integer dZ'
        ex = ref.exact_cols(l)
        assert _is_int(grads[l][0][:, ex]) and _is_int(grads[l][1]), f'{what} layer {l}: non-integer dW / db'
        B = np.zeros((len(ref.keys), dz.shape[1]))
        np.add.at(B, inv, np.abs(dz))
        _check_sums((B.T @ np.abs(ref.X[l]))[:, ex], f'{what} layer {l} dW')
        _check_sums(np.abs(dz).sum(0), f'{what} layer {l} db')
        _check_sums(np.abs(dz) @ np.abs(Ws[l]), f'{what} layer {l} dX')
        assert _is_int(dz @ Ws[l])
        if l != 11:                     # rgb's dZ is d raw: it meets the exact-fp32 head kernels only
            _split_hgemm(dz, f'{what} layer {l} dZ')
    assert _is_int(dpts[:, nerf_dpts_exact_cols(Ws, ref)])
    # the engine backward's planes: s0 = dZ of views (128), then d feature, dZ7 .. dZ0 (stream layers s0 .. s8); alpha gradient rides along
    chain = [dzs[10], dzs[8], dzs[7], dzs[6], dzs[5], dzs[4], dzs[3], dzs[2], dzs[1], dzs[0]]
    m = np.abs(chain[0]).max(1)
    s_lo = np.where(m > 0, np.ldexp(1.0, 13 - np.floor(np.log2(np.where(m > 0, m, 1))).astype(np.int64)), 1.0)
    s_hi = s_lo.copy()
    da = np.abs(dy[rows, 3])
    for i, v in enumerate(chain):
        if i:
            sq = (chain[i - 1] ** 2).sum(1) + (da ** 2 if i == 2 else 0.0)     # s1's inputs: d feature and the alpha gradient's plane
            n2_lo, n2_hi = sq * s_lo ** 2, sq * s_hi ** 2
            b_lo, b_hi = np.sqrt(n2_lo * cm[i - 1]), np.sqrt(n2_hi * cm[i - 1])
            t_lo = np.where(b_lo > 0, _pow2_floor(np.where(b_lo > 0, 2.0 ** 12 / np.maximum(b_lo, 1e-300), 1)), 1.0)
            if i == 1:                  # s0's outputs also hold the alpha gradient: its factor is capped by |da| s0 t < 2^14
                cap = np.where(da > 0, _pow2_floor(np.where(da > 0, 2.0 ** 13 / np.maximum(da * s_lo, 1e-300), 1)), np.inf)
                t_lo = np.minimum(t_lo, cap)
            t_hi = np.where(b_hi > 0, 2.0 ** 14 / np.maximum(b_hi, 1e-300), 1.0)
            s_lo, s_hi = s_lo * t_lo, s_hi * _pow2_floor(t_hi)
        _assert_split(v, s_lo[:, None], f'{what} engine plane {i} (smallest scale)')
        if i == 1:
            _assert_split(da, s_lo, f'{what} engine alpha plane (smallest scale)')
        assert np.all(np.abs(v) * s_hi[:, None] < 2.0 ** 14 * 4), f'{what} engine plane {i}: overflow at the largest scale'
    return ref.raw(), grads, dpts


def nerf_dpts_exact_cols(Ws, ref):
    """Coordinates c of d_pts that are exact: c is 0 in every sample, or no weight of pts0 / of the skip layer's embedding columns meets c's
    sin / cos columns (d e / d x_c then carries only the raw column's integer gradient: cos(.) 0 - sin(.) 0 = 0 exactly)."""
    pts = ref.keys[:, :3]
    return np.array([bool(np.all(pts[:, c] == 0) or (np.all(Ws[0][:, pe_cols(c, MULTIRES)] == 0) and np.all(Ws[5][:, pe_cols(c, MULTIRES)] == 0)))
                     for c in range(3)])


def dpts_sums(ref, dy):
    """posenc_bwd's sum of |terms| per row and coordinate [R, 3]: g = sum over pts0's and the skip layer's embedding gradient e of
    e_c + sum_k 2^k (cos(2^k x) e_sin,k - sin(2^k x) e_cos,k).  Where it is below 2^24 d_pts is exact (cos 0 = 1, sin 0 = 0 on the live
    coordinate; zero e on the others); elsewhere fp32 rounds it (d_pts_bound)."""
    dy = np.asarray(dy, np.float64)
    rows = np.flatnonzero(np.any(dy != 0, 1))
    T = np.zeros((ref.R, 3))
    f = np.concatenate([[1.0], np.repeat(2.0 ** np.arange(MULTIRES), 2)])
    for l, cols in ((0, slice(0, 63)), (5, slice(0, 63))):
        e = np.abs(ref.dz(l, dy[rows], rows) @ ref.W[l][:, cols])
        for c in range(3):
            T[rows, c] += e[:, [c] + [3 + 6 * k + c + 3 * h for k in range(MULTIRES) for h in (0, 1)]] @ f
    return T


def dpts_bound(T):
    """|got - ref| of d_pts where its sum of |terms| T reaches 2^24: 2 x 21 terms, each a product and a difference rounded (<= 3 roundings),
    and 42 additions, each rounding by <= 2^-24 of a partial sum <= T: (3 + 42) 2^-24 T, taken as 48 2^-24 T."""
    return np.where(T < ACC_MAX, 0.0, 48.0 * 2.0 ** -24 * T)


def dw_inexact_bound(ref, l, dy, splits=132):
    """Componentwise bound for the weight-gradient columns that meet sin / cos of non-zero coordinates (tests/test_exact_train_gpu.py docstring):
    sum_r |dZ_r| (E_SIN + 2^-23 + (nnz + splits) 2^-24 (|X_r| + E_SIN + 2^-23)), nnz = nonzero rows of dZ in that output; db needs none."""
    rows = np.flatnonzero(np.any(np.asarray(dy) != 0, 1))
    dz = np.abs(ref.dz(l, np.asarray(dy)[rows], rows))
    B = np.zeros((len(ref.keys), dz.shape[1]))
    np.add.at(B, ref.inv[rows], dz)
    nnz = (dz != 0).sum(0)[:, None]
    e = E_SIN + 2.0 ** -23
    return B.sum(0)[:, None] * e + (nnz + splits) * 2.0 ** -24 * (B.T @ (np.abs(ref.X[l]) + e))
