"""Head and positional-encoding inputs with exact answers, per-element error bounds and slipped kernel emulations (a plain helper module).

The five small kernels between the trainer's MLP stages and the compositing — ``sampler_head_fwd_kernel`` / ``sampler_head_bwd_kernel``,
``refine_head_fwd_kernel`` / ``refine_head_bwd_kernel``, ``posenc_bwd_kernel`` (pnrf_train.hip) — and ``posenc_kernel`` (pnrf_ops.hip),
reached through ``pnrf_sampler_head_*``, ``pnrf_refine_head_*``, ``pnrf_posenc_fwd`` / ``pnrf_posenc_bwd``.  This module holds

  * ``replay_*``: each kernel's formulas in the kernel's order, written once over the arithmetic back ends of tests/exact_composite.py
    (``F32``: one IEEE rounding per operation; ``Cert``: float64 with a certificate that no step rounds; ``Mag``: float64 with running
    magnitudes).  The forward heads are written with ieee_* (contraction off), so their ``F32`` replay is the bit-exact answer wherever
    the transcendentals are exact: sigmoid and tanh at y in {-200, 0, 200} (expf(-200) = 0, expf(200) = inf, expf(0) = 1,
    tanhf(+-200) = +-1, tanhf(0) = 0), sin / cos at x = 0 — whatever the origins, directions, depths, near, far and jitter are.  The
    backward kernels are compiled with contraction on; their exact regime is the ``Cert`` certificate: dyadic directions, depths,
    jitter and gradients (d_pts signed powers of two: 0.01f gp must not round) with y in {-200, 0, 200}, every product and sum exact,
    so neither a fused multiply-add nor the order of a sum can change a bit.  (The forward's pts = o + d z + 0.01f tanh rounds even
    there — 0.01f has 24 significant bits —: pts is the one output whose answer is the ``F32`` replay alone.)
  * ``exact_inputs`` (dyadic: certifies forward and backward; ``free=True``: general values around saturated y, for the forward
    kernels), ``random_inputs`` (the general regime), ``posenc_inputs``; ``reference_*``: the oracle in float64 and its autograd.
  * ``bound``, ``bound_*``: the general regime's per-element bounds, below.
  * ``MUTATIONS``: one slip each, applied inside ``replay_*``.

Per-element bound of the general regime:  |got - ref| <= d 2^-24 mag (1 + 2^-10) + d 2^-126, every element, nothing masked.

``mag`` comes from ``Mag`` (exact_composite.BOUND_DOC: inputs m = |v|; sums m_a + m_b; products m_a |b| + |a| m_b; a scaling by a power
of two scales m), run over the same ``replay_*`` as the exact answers; d is the largest number of roundings on any path to an output, in
units of u = 2^-24, a fused multiply-add counting as its two unfused operations (it rounds less, never more).

Transcendental ASSUMPTIONS (nothing in the ROCm device library documents a bound; these are exact_composite's figure for expf and the
OpenCL full-profile figures for the others, in ulp of the exact result, 1 ulp <= 2 u relative):
    expf <= 2 ulp (4 roundings; sigmoid_f = 1 / (1 + expf(-y)) of an input: 6),   sinf, cosf <= 4 ulp (8),   tanhf <= 5 ulp (10).
Their arguments carry no error: y is an input, and x 2^k is exact in fp32.

    sampler_head_fwd   d =  8   depth = sigmoid (6) * span (1) -> 7, + near -> 8; add / mul / idx are copies, mm_rgb is a sigmoid (6)
    sampler_head_bwd   d =  8   scatter (0 + g: 1), * span (1) -> 2, * sg (6) -> 7, * (1 - sg) (7) -> 8
    refine_head_fwd    d = 14   lower, upper 1 (the halving is exact), upper - lower 2, * sigmoid (6) -> 7, + lower -> 8 = z_pre;
                                z - neighbour 9, j |.| 10, z +- 11; d z 12, o + 13; 0.01 tanh (10) -> 11 (the reference's 0.01 is the
                                double: 0.37 u from 0.01f, on a path three roundings short of the longest); sum -> 14
    refine_head_bwd    d = 13   gz = d_z + sum_c gp d_c: 4; jitter factor 1 +- j sg: 2; product 5; two shares summed 7;
                                dy_s = gz (upper - lower) (2) -> 8, rf (6) -> 9, (1 - rf) (7) -> 10;
                                gD: gz (1 - rf) -> 8, halved, up to four terms summed -> 12;  dy_tanh = 0.01 gp (1) (1 - t t) (12) -> 13
    posenc_fwd         d =  8   sin / cos; the x columns are copies
    posenc_bwd         d = n_freq + 10   cos (8) e -> 9, difference 10, 2^k exact; the first term passes n_freq additions

The float64 reference's own error and the second-order terms fit in the factor 1 + 2^-10.  The absolute term covers results below the
normal range (sigmoid_f(y) is 0 in fp32 from y <= -89 on, where float64 keeps e^y).  sign(u) of the jitter's |u| is a branch: the input
sets hold no u within rounding of 0 unless it is exactly 0 in both precisions (a run of four equal depths), see ``random_inputs``; the
same holds for the sort order of the sampler's depths.

Worst observed error / bound on the MI355X (tests/test_exact_heads_gpu.py prints them; every element counted):
    sampler_head_fwd 0.226   sampler_head_bwd 0.088   refine_head_fwd 0.151   refine_head_bwd 0.076   posenc_fwd 0.246   posenc_bwd 0.091
"""
from __future__ import annotations

import numpy as np
import torch

from exact_composite import F32, Cert, Mag, U, head, tile  # noqa: F401  (head / tile: used by the tests through this module)
from oracle import pronerf_oracle as orc

BOUND_DOC = __doc__[__doc__.index('Per-element bound'):]

D_SAMPLER_FWD, D_SAMPLER_BWD, D_REFINE_FWD, D_REFINE_BWD, D_POSENC_FWD = 8, 8, 14, 13, 8
C001 = float(np.float32(1e-2))        # the kernels' 1e-2f

# ---- what tests/test_exact_heads_gpu.py runs (tests/test_exact_heads_cpu.py certifies the same sets)
N_SET = 257                           # one 257-ray set per regime; the smaller runs are its prefixes
NS = (1, 63, 64, 65, 257)             # 64-thread blocks: one ray, one short of a block, a block, one over, five blocks
N_CAP = 262144 + 65                   # past grid_for(n, 64)'s 4096 blocks: every thread loops
# option sets of the refine head: (jitter_dir or 0 for none, d_z given, d_rgb0 given); of the sampler head: d_rgb given
REFINE_OPTS = tuple((j, dz, dr) for j in (0, 1, -1) for dz, dr in ((True, True), (False, False), (True, False), (False, True)))
SAMPLER_OPTS = (True, False)
PE_FREQS = (0, 1, 4, 10, 16)
PE_ROWS = (1, 85, 86, 1000)           # 85 / 86 rows: 255 / 258 scalars, on either side of one 256-thread block
PE_SET = 1000
PE_CAP_ROWS = 349526                  # 1 048 578 scalars: past grid_for(n * 3)'s 4096 blocks of 256


def bound(d, mag):
    """The general regime's per-element bound (module docstring)."""
    return d * U * mag * (1 + 2.0 ** -10) + d * 2.0 ** -126


def bound_sampler_fwd(mag): return bound(D_SAMPLER_FWD, mag)
def bound_sampler_bwd(mag): return bound(D_SAMPLER_BWD, mag)
def bound_refine_fwd(mag): return bound(D_REFINE_FWD, mag)
def bound_refine_bwd(mag): return bound(D_REFINE_BWD, mag)
def bound_posenc_fwd(mag): return bound(D_POSENC_FWD, mag)
def bound_posenc_bwd(mag, n_freq): return bound(n_freq + 10, mag)


def worst_ratio(got, ref, bnd):
    """max over the elements of |got - ref| / bound (inf where got is not finite)."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape == np.shape(bnd), (g.shape, r.shape, np.shape(bnd))
    with np.errstate(invalid='ignore'):
        q = np.abs(g - r) / bnd
    q = np.where(np.isfinite(g) & np.isfinite(q), q, np.inf)
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------------------------------------ the kernels' formulas
MUTATIONS = (
    'first_lower_without_near',   # refine heads: lower_0 = 0.5 D_0 (near dropped)
    'last_upper_without_far',     # refine heads: upper_7 = 0.5 D_7 (far dropped)
    'neighbour_after_jitter',     # refine_head_fwd: the jitter's neighbour read after it was jittered itself (updated in place)
    'edge_neighbour_from_z',      # refine heads: the last (dir > 0) / first (dir < 0) sample's neighbour is z itself, not far / near
    'jitter_dir_flipped',         # refine heads: jitter toward the other neighbour
    'pts_from_z_pre',             # refine_head_fwd: query points on the depths before the jitter
    'abs_grad_always_plus',       # refine_head_bwd: d|u| / du = +1 for u < 0 too
    'abs_grad_at_zero',           # refine_head_bwd: d|u| / du = +1 at u == 0 (torch: 0)
    'neighbour_share_lost',       # refine_head_bwd: the jitter's gradient to the neighbouring depth dropped
    'gd_neighbour_share_lost',    # refine_head_bwd: the lower midpoint's share of gD[s - 1] dropped
    'span_missing',               # sampler_head_bwd: d depth / d sigmoid = 1 instead of far - near
    'scatter_as_gather',          # sampler_head_bwd: dy[q] = g[idx[q]] instead of dy[idx[s]] = g[s]
    'sort_unstable',              # sampler_head_fwd: tied depths in descending index order
    'posenc_identity_lost',       # posenc_bwd: the dE[c] term dropped
    'posenc_octave',              # posenc fwd / bwd: 2^(k+1) for 2^k
    'posenc_sin_cos_swapped',     # posenc_bwd: the sin and cos columns of dE swapped
)


def _cols(A, x):
    return [A.inp(x[:, k]) for k in range(x.shape[1])]


def _pick(A, cols, k):
    """cols[k] per ray (k an int array): the kernels' select chains."""
    r = cols[0]
    for q in range(1, len(cols)):
        r = A.where(k == q, cols[q], r)
    return r


def replay_sampler_fwd(A, inp, mutation=None):
    """sampler_head_fwd_kernel.  inp: y27 [n,27], rays [n,11].  Returns depth [8], add [8], mul [8], rgb [3] as lists of back-end columns,
    and idx [n,8] (int64)."""
    y, rays = inp['y27'], inp['rays']
    near, far = A.inp(rays[:, 6]), A.inp(rays[:, 7])
    span = A.sub(far, near)
    yc = _cols(A, y)
    dep = [A.add(A.mul(A.sigmoid(yc[s]), span), near) for s in range(8)]
    val = np.stack([np.asarray(A.cond(d), np.float64) for d in dep], 1)
    if mutation == 'sort_unstable':
        idx = 7 - np.argsort(val[:, ::-1], axis=1, kind='stable')           # stable on the reversed row: ties in descending index order
    else:
        idx = np.argsort(val, axis=1, kind='stable')
    idx = idx.astype(np.int64)
    return dict(depth=[_pick(A, dep, idx[:, s]) for s in range(8)], add=[_pick(A, yc[8:16], idx[:, s]) for s in range(8)],
                mul=[_pick(A, yc[16:24], idx[:, s]) for s in range(8)], rgb=[A.sigmoid(yc[24 + c]) for c in range(3)], idx=idx)


def replay_sampler_bwd(A, inp, idx, d_rgb=True, mutation=None):
    """sampler_head_bwd_kernel.  inp: y27, rays, s_gd / s_ga / s_gm [n,8], s_gr [n,3]; idx [n,8] from the forward.  Returns dy [27]."""
    y, rays = inp['y27'], inp['rays']
    yc = _cols(A, y)
    span = A.sub(A.inp(rays[:, 7]), A.inp(rays[:, 6]))
    zero = A.const(0.0, span)
    one = A.const(1.0, span)
    g = [zero] * 27
    src = [_cols(A, inp['s_gd']), _cols(A, inp['s_ga']), _cols(A, inp['s_gm'])]
    for q in range(8):
        for b in range(3):
            if mutation == 'scatter_as_gather':
                g[8 * b + q] = A.add(zero, _pick(A, src[b], idx[:, q]))
            else:
                acc = zero
                for s in range(8):
                    acc = A.where(idx[:, s] == q, A.add(acc, src[b][s]), acc)
                g[8 * b + q] = acc
    for s in range(8):
        sg = A.sigmoid(yc[s])
        gs = g[s] if mutation == 'span_missing' else A.mul(g[s], span)
        g[s] = A.mul(A.mul(gs, sg), A.sub(one, sg))
    for c in range(3):
        if d_rgb:
            sg = A.sigmoid(yc[24 + c])
            g[24 + c] = A.mul(A.mul(A.inp(inp['s_gr'][:, c]), sg), A.sub(one, sg))
    return dict(dy=g)


def _lower_upper(A, D, near, far, s, M):
    zero = A.const(0.0, near)
    if s == 0:
        lower = A.scale(A.add(zero if M == 'first_lower_without_near' else near, D[0]), 0.5)
    else:
        lower = A.scale(A.add(D[s], D[s - 1]), 0.5)
    if s == 7:
        upper = A.scale(A.add(zero if M == 'last_upper_without_far' else far, D[7]), 0.5)
    else:
        upper = A.scale(A.add(D[s + 1], D[s]), 0.5)
    return lower, upper


def replay_refine_fwd(A, inp, jdir=0, mutation=None):
    """refine_head_fwd_kernel.  inp: y35 [n,35], rays, D [n,8] (any order), jitter [n,8]; jdir 0: no jitter.  Returns z_pre [8], z [8],
    pts [24] (sample-major), rgb0 [3]."""
    M = mutation
    yc, r, D = _cols(A, inp['y35']), _cols(A, inp['rays']), _cols(A, inp['D'])
    near, far = r[6], r[7]
    zz = []
    for s in range(8):
        lower, upper = _lower_upper(A, D, near, far, s, M)
        zz.append(A.add(lower, A.mul(A.sub(upper, lower), A.sigmoid(yc[s]))))
    z_pre = list(zz)
    if jdir:
        jd = -jdir if M == 'jitter_dir_flipped' else jdir
        j = _cols(A, inp['jitter'])
        zn = list(zz)
        src = zn if M == 'neighbour_after_jitter' else zz
        for s in (range(7, -1, -1) if jd > 0 else range(8)):                 # the order matters to neighbour_after_jitter only
            if jd > 0:
                nb = src[s + 1] if s < 7 else (zz[7] if M == 'edge_neighbour_from_z' else far)
                zn[s] = A.add(zz[s], A.mul(j[s], A.abs(A.sub(zz[s], nb))))
            else:
                nb = src[s - 1] if s > 0 else (zz[0] if M == 'edge_neighbour_from_z' else near)
                zn[s] = A.sub(zz[s], A.mul(j[s], A.abs(A.sub(zz[s], nb))))
        zz = zn
    c001 = A.const(C001, near)
    zp = z_pre if M == 'pts_from_z_pre' else zz
    pts = [A.add(A.add(r[c], A.mul(r[3 + c], zp[s])), A.mul(c001, A.tanh(yc[8 + 3 * s + c]))) for s in range(8) for c in range(3)]
    return dict(z_pre=z_pre, z=zz, pts=pts, rgb0=[A.sigmoid(yc[32 + c]) for c in range(3)])


def replay_refine_bwd(A, inp, z_pre, jdir=0, d_z=True, d_rgb0=True, mutation=None):
    """refine_head_bwd_kernel.  inp: y35, rays, D, jitter, r_gp [n,8,3], r_gz [n,8], r_gr [n,3]; z_pre [n,8] from the forward (an
    input of the kernel: only the sign of z_pre - neighbour is used).  Returns dy [35], dD [8]."""
    M = mutation
    yc, r, D, zp = _cols(A, inp['y35']), _cols(A, inp['rays']), _cols(A, inp['D']), _cols(A, z_pre)
    near, far = r[6], r[7]
    zero, one = A.const(0.0, near), A.const(1.0, near)
    c001 = A.const(C001, near)
    dy = [zero] * 35
    gz = []
    for s in range(8):
        g = A.inp(inp['r_gz'][:, s]) if d_z else zero
        for c in range(3):
            gp = A.inp(inp['r_gp'][:, s, c])
            g = A.add(g, A.mul(gp, r[3 + c]))
            t = A.tanh(yc[8 + 3 * s + c])
            dy[8 + 3 * s + c] = A.mul(A.mul(c001, gp), A.sub(one, A.mul(t, t)))
        gz.append(g)
    if jdir:
        jd = -jdir if M == 'jitter_dir_flipped' else jdir
        j = _cols(A, inp['jitter'])
        gn = [zero] * 8
        for s in range(8):
            if jd > 0:
                nb = zp[s + 1] if s < 7 else (zp[7] if M == 'edge_neighbour_from_z' else far)
            else:
                nb = zp[s - 1] if s > 0 else (zp[0] if M == 'edge_neighbour_from_z' else near)
            u = A.sub(zp[s], nb)
            if M == 'abs_grad_always_plus':
                sg = A.where(A.cond(u) == 0, zero, one)
            elif M == 'abs_grad_at_zero':
                sg = A.where(A.cond(u) == 0, one, A.sign(u))
            else:
                sg = A.sign(u)
            js = A.mul(j[s], sg)
            if jd > 0:
                gn[s] = A.add(gn[s], A.mul(gz[s], A.add(one, js)))
                if s < 7 and M != 'neighbour_share_lost':
                    gn[s + 1] = A.add(gn[s + 1], A.mul(gz[s], A.neg(js)))
            else:
                gn[s] = A.add(gn[s], A.mul(gz[s], A.sub(one, js)))
                if s > 0 and M != 'neighbour_share_lost':
                    gn[s - 1] = A.add(gn[s - 1], A.mul(gz[s], js))
        gz = gn
    gD = [zero] * 8
    for s in range(8):
        lower, upper = _lower_upper(A, D, near, far, s, M)
        rf = A.sigmoid(yc[s])
        dy[s] = A.mul(A.mul(A.mul(gz[s], A.sub(upper, lower)), rf), A.sub(one, rf))
        gl, gu = A.scale(A.mul(gz[s], A.sub(one, rf)), 0.5), A.scale(A.mul(gz[s], rf), 0.5)
        gD[s] = A.add(gD[s], gl)
        if s > 0 and M != 'gd_neighbour_share_lost':
            gD[s - 1] = A.add(gD[s - 1], gl)
        if s < 7:
            gD[s + 1] = A.add(gD[s + 1], gu)
        gD[s] = A.add(gD[s], gu)
    if d_rgb0:
        for c in range(3):
            sg = A.sigmoid(yc[32 + c])
            dy[32 + c] = A.mul(A.mul(A.inp(inp['r_gr'][:, c]), sg), A.sub(one, sg))
    return dict(dy=dy, dD=gD)


def _octave(k, mutation):
    return 2.0 ** (k + 1 if mutation == 'posenc_octave' else k)


def replay_posenc_fwd(A, inp, mutation=None):
    """posenc_kernel.  inp: x [rows,3], n_freq.  Returns out: a list of [rows,3] blocks [x, sin 2^0 x, cos 2^0 x, sin 2^1 x, ...]."""
    x = A.inp(inp['x'])
    out = [x]
    for k in range(inp['n_freq']):
        arg = A.scale(x, _octave(k, mutation))
        out += [A.sin(arg), A.cos(arg)]
    return dict(out=out)


def replay_posenc_bwd(A, inp, mutation=None):
    """posenc_bwd_kernel with one gradient source.  inp: x [rows,3], dE [rows, 3 + 6 n_freq], n_freq.  Returns dx: one [rows,3] block."""
    x, dE = A.inp(inp['x']), inp['dE']
    g = A.const(0.0, x)
    if mutation != 'posenc_identity_lost':
        g = A.add(g, A.inp(dE[:, 0:3]))
    for k in range(inp['n_freq']):
        f = _octave(k, mutation)
        arg = A.scale(x, f)
        es, ec = A.inp(dE[:, 3 + 6 * k:6 + 6 * k]), A.inp(dE[:, 6 + 6 * k:9 + 6 * k])
        if mutation == 'posenc_sin_cos_swapped':
            es, ec = ec, es
        g = A.add(g, A.scale(A.sub(A.mul(A.cos(arg), es), A.mul(A.sin(arg), ec)), f))
    return dict(dx=[g])


SHAPES = dict(pts=(8, 3))


def collect(out, get):
    """Lists of back-end columns (or [rows,3] blocks) -> arrays in the ops' shapes; get(V) picks .v or .t (F32: the array itself)."""
    res = {}
    for k, v in out.items():
        if k == 'idx':
            res[k] = v
            continue
        g = [np.asarray(get(x)) for x in v]
        a = np.concatenate(g, 1) if g[0].ndim == 2 else np.stack(g, 1)
        res[k] = a.reshape((a.shape[0],) + SHAPES[k]) if k in SHAPES else a
    return res


def _run(A, kernel, inp, **kw):
    return {'sampler_fwd': replay_sampler_fwd, 'sampler_bwd': replay_sampler_bwd, 'refine_fwd': replay_refine_fwd,
            'refine_bwd': replay_refine_bwd, 'posenc_fwd': replay_posenc_fwd, 'posenc_bwd': replay_posenc_bwd}[kernel](A, inp, **kw)


def emulate(kernel, inp, **kw):
    """float32 CPU emulation of a kernel (F32 back end): dict of float32 arrays (idx: int64)."""
    with np.errstate(all='ignore'):
        out = collect(_run(F32(), kernel, inp, **kw), lambda x: x)
    return {k: (v if k == 'idx' else np.asarray(v, np.float32)) for k, v in out.items()}


def certify(kernel, inp, taint_ok=(), **kw):
    """The exact regime's certificate: (expected float32 outputs, taint masks).  Raises when an output outside taint_ok is tainted."""
    A = Cert()
    with np.errstate(all='ignore'):
        out = _run(A, kernel, inp, **kw)
        val, bad = collect(out, lambda x: x.v), collect(out, lambda x: x.t)
    for k in val:
        if k == 'idx' or k in taint_ok:
            continue
        assert not bad[k].any(), f'{kernel} {k}: {int(bad[k].sum())} inexact elements ({A.why})'
        assert np.isfinite(val[k]).all(), (kernel, k)
    return {k: (v if k == 'idx' else v.astype(np.float32)) for k, v in val.items()}, bad


def magnitudes(kernel, inp, **kw):
    """General regime: (float64 values of the replay, magnitudes) of every output."""
    A = Mag()
    with np.errstate(all='ignore'):
        out = _run(A, kernel, inp, **kw)
        return collect(out, lambda x: x.v), collect(out, lambda x: x.t)


# ------------------------------------------------------------------------------------------------ the float64 references
def _t(x, rg=False):
    return torch.tensor(np.asarray(x, np.float64), requires_grad=rg)


def reference_sampler(inp, d_rgb=True):
    """orc.sort_gather on sigmoid(y[:, :8]) in float64, and autograd of sum(out * g): depth, idx, add, mul, rgb, dy."""
    y, rays = _t(inp['y27'], True), _t(inp['rays'])
    depth = torch.sigmoid(y[:, :8])
    ds, idx, adds, muls = orc.sort_gather(depth, y[:, 8:16], y[:, 16:24], rays[:, 6:7], rays[:, 7:8])
    rgb = torch.sigmoid(y[:, 24:])
    loss = (ds * _t(inp['s_gd'])).sum() + (adds * _t(inp['s_ga'])).sum() + (muls * _t(inp['s_gm'])).sum()
    if d_rgb:
        loss = loss + (rgb * _t(inp['s_gr'])).sum()
    loss.backward()
    return dict(depth=ds.detach().numpy(), idx=idx.numpy(), add=adds.detach().numpy(), mul=muls.detach().numpy(), rgb=rgb.detach().numpy(),
                dy=y.grad.numpy())


def reference_refine(inp, jdir=0, d_z=True, d_rgb0=True):
    """orc.interval_refine in float64, the jitter and pts as tests/test_train_gpu.py states them, and autograd: z_pre, z, pts, rgb0, dy, dD."""
    n = inp['y35'].shape[0]
    y, rays, D = _t(inp['y35'], True), _t(inp['rays']), _t(inp['D'], True)
    jit = _t(inp['jitter'])
    near, far = rays[:, 6:7], rays[:, 7:8]
    z_pre = z = orc.interval_refine(D, torch.sigmoid(y[:, :8]), near, far)
    if jdir > 0:
        z = z + jit * (z - torch.cat([z[:, 1:], far], 1)).abs()
    elif jdir < 0:
        z = z - jit * (z - torch.cat([near, z[:, :-1]], 1)).abs()
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None] + 1e-2 * torch.tanh(y[:, 8:32]).reshape(n, 8, 3)
    rgb0 = torch.sigmoid(y[:, 32:])
    loss = (pts * _t(inp['r_gp'])).sum()
    if d_z:
        loss = loss + (z * _t(inp['r_gz'])).sum()
    if d_rgb0:
        loss = loss + (rgb0 * _t(inp['r_gr'])).sum()
    loss.backward()
    return dict(z_pre=z_pre.detach().numpy(), z=z.detach().numpy(), pts=pts.detach().numpy(), rgb0=rgb0.detach().numpy(), dy=y.grad.numpy(),
                dD=D.grad.numpy())


def reference_posenc(inp):
    """orc.posenc in float64 and its autograd for d out = dE: out, dx."""
    x = _t(inp['x'], True)
    out = orc.posenc(x, inp['n_freq'])
    out.backward(_t(inp['dE']))
    return dict(out=out.detach().numpy(), dx=x.grad.numpy())


KEYS = dict(sampler_fwd=('depth', 'idx', 'add', 'mul', 'rgb'), sampler_bwd=('dy',), refine_fwd=('z_pre', 'z', 'pts', 'rgb0'), refine_bwd=('dy', 'dD'),
            posenc_fwd=('out',), posenc_bwd=('dx',))


def head_cases():
    """(kernel, options) of the four head kernels: every combination the tests run."""
    yield 'sampler_fwd', {}
    for dr in SAMPLER_OPTS:
        yield 'sampler_bwd', dict(d_rgb=dr)
    for j in (0, 1, -1):
        yield 'refine_fwd', dict(jdir=j)
    for j, dz, dr in REFINE_OPTS:
        yield 'refine_bwd', dict(jdir=j, d_z=dz, d_rgb0=dr)


def saved(kernel, fwd):
    """What a backward kernel takes from its forward (fwd: dict(idx=, z_pre=)): the sort indices / the depths before the jitter."""
    return {'sampler_bwd': dict(idx=fwd['idx']), 'refine_bwd': dict(z_pre=fwd['z_pre'])}.get(kernel, {})


def forward_state(inp):
    """idx and z_pre of the float32 forward replays (the kernels' forwards give the same: asserted on the GPU)."""
    return dict(idx=emulate('sampler_fwd', inp)['idx'], z_pre=emulate('refine_fwd', inp)['z_pre'])


def reference(kernel, inp, **kw):
    """The float64 reference's outputs of one kernel."""
    if kernel.startswith('sampler'):
        ref = reference_sampler(inp, **kw)
    elif kernel.startswith('refine'):
        ref = reference_refine(inp, **kw)
    else:
        ref = reference_posenc(inp)
    return {k: ref[k] for k in KEYS[kernel]}


def bound_of(kernel, inp, mag):
    """bound_<kernel> of a magnitude array."""
    if kernel == 'posenc_bwd':
        return bound_posenc_bwd(mag, inp['n_freq'])
    return dict(sampler_fwd=bound_sampler_fwd, sampler_bwd=bound_sampler_bwd, refine_fwd=bound_refine_fwd, refine_bwd=bound_refine_bwd,
                posenc_fwd=bound_posenc_fwd)[kernel](mag)


def ratios(kernel, got, ref, mag, inp):
    """{output: worst |got - ref| / bound} of one kernel's outputs (idx: 0 when equal, inf otherwise)."""
    out = {}
    for k in KEYS[kernel]:
        if k == 'idx':
            out[k] = 0.0 if np.array_equal(got[k], ref[k]) else np.inf
        else:
            out[k] = worst_ratio(got[k], ref[k], bound_of(kernel, inp, mag[k]))
    return out


# ------------------------------------------------------------------------------------------------ input sets
SAT = np.array([-200, 0, 0, 200], np.float32)                  # y = 0 on half of the entries: sg (1 - sg) = 0.25, 1 - t^2 = 1


def _special_depths(D, near, far, mid):
    """Rays i % 8 == 1: all depths equal; == 2: the last four at far; == 3: the first four at near; == 4: a run of four equal depths
    inside.  A run of four equal depths v makes lower = upper = v for the two samples inside it, so z_pre = v there in every precision
    and u == 0 exactly; at far / near the same holds for the last / first sample against its far / near neighbour."""
    i = np.arange(D.shape[0])
    D[i % 8 == 1] = mid[i % 8 == 1, None]
    D[i % 8 == 2, 4:] = far[i % 8 == 2, None]
    D[i % 8 == 3, :4] = near[i % 8 == 3, None]
    D[i % 8 == 4, 2:6] = D[i % 8 == 4, 2:3]
    return D


def _near_far(rs, n):
    near = rs.choice(np.array([0.0, 0.5, 2.0], np.float32), n)
    return near, near + rs.choice(np.array([1.0, 4.0], np.float32), n)


def exact_inputs(n=N_SET, seed=0, free=False):
    """The exact regime's set for the four head kernels.  y27[:, 0:8], y27[:, 24:27] and all of y35 in {-200, 0, 0, 200}; tied sampler
    depths follow.  free=False: directions and origins in halves, depths near + span k / 8 (sorted on three rays of five, the special
    rays of _special_depths among them), jitter in quarters with half of them 0, gradients in eighths / quarters, d_pts 0 or +-2^k.
    free=True: all of those general floats (the forward kernels' set)."""
    rs = np.random.RandomState(1000 + seed + (500 if free else 0))
    near, far = _near_far(rs, n)
    span = far - near
    rays = rs.randn(n, 11).astype(np.float32)
    if not free:
        rays[:, 0:6] = rs.randint(-4, 5, (n, 6)) / 2.0
    rays[:, 6], rays[:, 7] = near, far
    y27 = rs.randn(n, 27).astype(np.float32)
    y27[:, 0:8] = rs.choice(SAT, (n, 8)); y27[:, 24:27] = rs.choice(SAT, (n, 3))
    y35 = rs.choice(SAT, (n, 35)).astype(np.float32)
    if free:
        D = near[:, None] + span[:, None] * rs.rand(n, 8)
        mid = near + span * rs.rand(n)
        jit = np.minimum(np.abs(rs.randn(n, 8)) / 5, 1 - 2e-6)
        g = lambda *s: rs.randn(n, *s)
        gp = g(8, 3)
    else:
        D = near[:, None] + span[:, None] * rs.randint(0, 9, (n, 8)) / 8.0
        mid = near + span * rs.randint(1, 8, n) / 8.0
        jit = rs.randint(1, 4, (n, 8)) / 4.0
        g = lambda *s: rs.randint(-16, 17, (n,) + s) / 8.0
        gp = rs.choice(np.array([0, 0.5, -0.5, 1, -1, 2, -2]), (n, 8, 3))
    jit = np.where(rs.rand(n, 8) < 0.5, 0.0, jit)
    srt = rs.rand(n) < 0.6
    D = np.where(srt[:, None], np.sort(D, 1), D)
    D = _special_depths(D, near, far, mid)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(y27=y27, y35=y35, rays=rays, D=f(D), jitter=f(jit), s_gd=f(g(8)), s_ga=f(g(8)), s_gm=f(g(8)), s_gr=f(g(3)),
                r_gp=f(gp), r_gz=f(g(8)), r_gr=f(g(3)))


def _robust(inp):
    """Rays of a general set whose discrete decisions agree between fp32 and float64: the sampler's sort order, and the sign of every
    u = z_pre - neighbour the jitter can take (both directions), with no u within 64 roundings of 0 unless it is 0 in both."""
    f = emulate('sampler_fwd', inp)
    ok = (f['idx'] == reference_sampler(inp)['idx']).all(1)
    z32 = emulate('refine_fwd', inp)['z_pre'].astype(np.float64)
    z64 = reference_refine(inp)['z_pre']
    near, far = inp['rays'][:, 6:7].astype(np.float64), inp['rays'][:, 7:8].astype(np.float64)

    def us(z):
        return np.concatenate([z - np.concatenate([z[:, 1:], far], 1), z - np.concatenate([near, z[:, :-1]], 1)], 1)
    u32, u64 = us(z32), us(z64)
    scale = np.abs(z64).max(1, keepdims=True) + np.abs(far)
    ok &= (np.sign(u32) == np.sign(u64)).all(1) & ((u64 == 0) | (np.abs(u64) > 64 * U * scale)).all(1)
    return ok


def random_inputs(n=N_SET, seed=0):
    """The general regime's set for the four head kernels: y ~ 2 N(0, 1) with a tenth of the entries in {-200, 0, 200} and, on rays
    i % 8 == 5, three equal depth logits (tied depths in every precision); rays ~ N(0, 1) with near in {0, 0.5, 2}, far - near in
    {1, 4}; depths uniform in [near, far], sorted on three rays of five, with _special_depths; jitter min(|N| / 5, 1 - 2e-6) with a
    third exactly 0; gradients ~ N(0, 1).  Rays whose sort order or whose sign of u is decided by rounding (_robust) are redrawn."""
    rs = np.random.RandomState(2000 + seed)

    def draw(m, first):
        near, far = _near_far(rs, m)
        span = far - near
        rays = rs.randn(m, 11).astype(np.float32)
        rays[:, 6], rays[:, 7] = near, far
        y27, y35 = (2 * rs.randn(m, 27)).astype(np.float32), (2 * rs.randn(m, 35)).astype(np.float32)
        if first:
            for y in (y27, y35):
                sat = rs.rand(*y.shape) < 0.1
                y[sat] = rs.choice(np.array([-200, 0, 200], np.float32), int(sat.sum()))
            i = np.arange(m)
            y27[i % 8 == 5, 3] = y27[i % 8 == 5, 1]; y27[i % 8 == 5, 5] = y27[i % 8 == 5, 1]
        D = near[:, None] + span[:, None] * rs.rand(m, 8)
        srt = rs.rand(m) < 0.6
        D = np.where(srt[:, None], np.sort(D, 1), D)
        if first:
            D = _special_depths(D, near, far, near + span * rs.rand(m))
        jit = np.minimum(np.abs(rs.randn(m, 8)) / 5, 1 - 2e-6)
        jit[rs.rand(m, 8) < 0.33] = 0
        f = lambda a: np.ascontiguousarray(a, np.float32)
        return dict(y27=y27, y35=y35, rays=rays, D=f(D), jitter=f(jit), s_gd=f(rs.randn(m, 8)), s_ga=f(rs.randn(m, 8)), s_gm=f(rs.randn(m, 8)),
                    s_gr=f(rs.randn(m, 3)), r_gp=f(rs.randn(m, 8, 3)), r_gz=f(rs.randn(m, 8)), r_gr=f(rs.randn(m, 3)))
    inp = draw(n, True)
    for _ in range(8):
        bad = np.flatnonzero(~_robust(inp))
        if not bad.size:
            return inp
        new = draw(bad.size, False)
        for k in inp:
            inp[k][bad] = new[k]
    raise AssertionError('random_inputs: rays with a rounding-decided branch remain')


def posenc_inputs(rows=PE_SET, n_freq=10, seed=0, exact=True):
    """x [rows,3] and dE [rows, 3 + 6 n_freq].  A third of the x are exactly 0 (sin = 0, cos = 1 in every implementation), a tenth are
    +-1.5 (the edge of the range the pipeline produces), the rest uniform in [-1.5, 1.5].  exact=True: dE in eighths within +-2, so
    that dE[c] + sum_k 2^k dE[sin_k] is exact at x = 0 (at most 2^17 in units of 2^-3); exact=False: dE ~ N(0, 1)."""
    rs = np.random.RandomState(3000 + 20 * seed + n_freq + (0 if exact else 10000))
    x = rs.uniform(-1.5, 1.5, (rows, 3)).astype(np.float32)
    pick = rs.rand(rows, 3)
    x[pick < 1 / 3] = 0
    x[pick > 0.9] = rs.choice(np.array([-1.5, 1.5], np.float32), int((pick > 0.9).sum()))
    w = 3 + 6 * n_freq
    dE = (rs.randint(-16, 17, (rows, w)) / 8.0 if exact else rs.randn(rows, w)).astype(np.float32)
    return dict(x=x, dE=dE, n_freq=n_freq)
