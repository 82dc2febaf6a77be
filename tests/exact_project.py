"""Neighbour-view projection and colour fetch: inputs with exact answers, per-element bounds and slipped emulations (a plain helper module).

The four operator kernels of pnrf_ops.hip that map (ray, view, sample) to four texel indices, four weights and an output column —
``warp_trt_kernel``, ``warp_train_kernel``, ``refine_input_kernel``, ``refine_input_train_kernel`` (with pnrf_geom.h), reached through
``ops.warp_trt`` / ``warp_train`` / ``refine_input`` / ``refine_input_train`` — and ``images_pack_kernel``.  The projecting head of the
fused refine stage (pnrf_refine_project_fwd) has its own exact set at the end of the module.  This module holds

  * ``replay_*``: each kernel's sequence stated once over the arithmetic back ends of tests/exact_composite.py: ``project`` (inference:
    metric depth, world point, 3x4 matrix, perspective division), ``project_train`` (R^T (w - t), |c2.z| + 1e-8, y flip, K, the inside
    mask), ``_fetch`` (bilinear_setup's normalise / un-normalise round trip, floor, the four weights and taps, zero padding), the valid-mask
    mean fill, the sample Pluecker columns and the two column layouts.  The kernels use only the one-rounding operations of pnrf_ieee.h,
    so the ``F32`` replay is their complete specification: the GPU test compares bit for bit with it on every input set.  The float64
    run of the same formulas (``reference``) is the reference; tests/test_exact_project_cpu.py cross-checks it against the oracle.
  * the exact sets (``exact_inference``, ``exact_training``, ``exact_warp``), where float64 = ``F32`` replay = ``Cert`` certificate bit for bit:
    images of (Hf, Wf) = (5, 9) and (9, 17) (Wf - 1, Hf - 1 powers of two: the coordinate round trip is the identity on dyadic
    coordinates), eps = 2^-10 and dn = 1 - 2^-10 - 2^-j (z3d = 2^j), dyadic rays and matrices with p[2] / |c2.z| a power of two, so that
    every X, Y is a multiple of 1/4 (1/8 in Y where K couples it to x), and texels that are distinct integers below 2^12 (a fixed
    permutation of (view, channel, y, x)): a blend is a sum of integers times dyadic weights, exact in fp32, and any displaced tap,
    swapped view, channel or sample changes it.  One rounding is allowed and certified: |c2.z| + 1e-8f rounds back to |c2.z|.  The mean
    fill divides an exact sum by fl(cnt + 1e-6f): one correctly rounded division, which the certificate computes.
    The float64 run rounds to the same bits, given the certified absorption: ``run64(absorb=True)`` rounds |c2.z| + 1e-8f to fp32 as
    the kernels do (plain float64 would keep the 1e-8 and shift a coordinate by 1e-8 of itself — times a texel difference of up to
    4092 more than an ulp of a small colour, and enough to flip ``valid`` beside a black texel: hence also the black VIEW of the
    training sets).  The mean-fill columns lie within 2 ulp of it.
  * the general sets (``general_inference``, ``general_training``, ``general_warp``): random poses and depths, textured 13 x 19 images
    (at Wf = 19 the round trip is not the identity); the training sets redraw, on the CPU, every ray whose float64 normalised coordinates
    come within 2^-12 of |xn| = 1 or |yn| = 1 (input selection on the reference: no element is excluded from a comparison).
  * ``MUTATIONS``: one slip each, applied inside the replays.

Per-element bound of the general sets:  |got - ref| <= d 2^-24 mag (1 + 2^-10) + d 2^-126, every element.

``mag`` comes from ``Mag`` (exact_composite.BOUND_DOC) run over the same replays; floor carries no error of its own and a tap's magnitude
is the largest |texel| of the 4x4 neighbourhood of its cell (zero padding included): a coordinate within rounding of an integer may fall
into the next cell in fp32, where bilinear interpolation of the zero-padded image continues the same continuous function.  d counts the
roundings of the longest path (a fused multiply-add as its two operations):
    refine_input        d = 20   z3d 3 (two differences, a division), w 5, p 9 (a product, three sums), X 10, xn 12 (2 X is exact), ix 14,
                                 weight 15, tap weight 16, product 17, three sums 20;  Pluecker columns 10 (|d| 6, h 7, point 2, cross 10)
    warp_trt            d = 17   w 2, p 6, X 7, xn 9, ix 11, weight 12, tap weight 13, product 14, sums 17
    warp_train          d = 21   w 2, c2 6, |z| + 1e-8 7, c 8, X 11, xn 13, ix 15, then 6 more as above
    refine_input_train  d = 30   z3d 3, w 5, c2 9, 10, 11, X 14, xn 16, ix 18, colour 24, the mean's four sums 28, division 29, blend 30
The float64 run's own error, the kernels' 1e-8f / 1e-6f against the oracle's doubles and the second-order terms fit in 1 + 2^-10.

The bound is loose by design (a tap's magnitude is the largest texel of a 4x4 neighbourhood, d counts the longest path): it states what
fp32 may do to the reference, while the bit-for-bit comparison with the replay is what holds the kernels.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from exact_composite import F32, Cert, Mag, V, U
from oracle import pronerf_oracle as orc

BOUND_DOC = __doc__[__doc__.index('Per-element bound'):]

D = dict(refine_input=20, warp_trt=17, warp_train=21, refine_input_train=30)
EPS_EXACT = 2.0 ** -10
EPS_GENERAL = float(np.float32(1e-5))
C1E8 = float(np.float32(1e-8))
C1E6 = float(np.float32(1e-6))
FIN_LIM = 1e9                          # bilinear_setup: |ix|, |iy| < 1e9f, else every tap is outside
SIZES = ((5, 9), (9, 17))              # (Hf, Wf) of the exact sets
GENERAL_SIZE = (13, 19)
NV_TRAIN = 6                           # training views of the exact and general training sets
N_SET = 257

# ---- what tests/test_exact_project_gpu.py runs (tests/test_exact_project_cpu.py certifies the same sets)
NBS = (1, 2, 3, 4, 5, 6, 7, 8)
NS_INPUT = (1, 63, 64, 65, 257)        # refine_input_kernel: 64-ray tiles
N_INPUT_CAP = 4096 * 64 + 65           # past grid_for's 4096 blocks of one tile each
NS_TRAIN = (1, 7, 8, 9, 257)           # refine_input_train_kernel: 8 rays (32 lanes each) per 256-thread block
N_TRAIN_CAP = 32768 + 9                # past 4096 blocks of 8 rays: a ragged second round
NS_WARP = (1, 255, 256, 257)
BS_WARP = (1, 3)
N_WARP_CAP = 349531                    # B = 3: 1 048 593 threads' worth, past 4096 blocks of 256

MUTATIONS = (
    'tap_x1_to_x0',          # the tap at x0 + 1 reads column x0
    'floor_to_round',        # the cell origin by rounding to nearest instead of floor
    'align_corners_off',     # un-normalisation ((x + 1) W - 1) / 2
    'border_padding',        # a tap outside the image reads the clamped texel with its weight (border, not zero padding)
    'xy_swapped',            # X and Y exchanged before the fetch
    'y_flip_missing',        # project_train: c2.y not negated
    'inside_strict',         # project_train: the inside mask with < and > (xn == +-1 falls outside)
    'z_without_abs',         # project_train: division by c2.z + 1e-8 instead of |c2.z| + 1e-8
    'mean_over_all',         # mean fill: every neighbour counted, not the valid ones
    'valid_one_channel',     # mean fill: valid decided by the first channel alone
    'layouts_swapped',       # layout 1 written for layout 0 and the reverse
    'view_next',             # the colours of view k + 1 mod nb in the columns of view k
    'sample_reversed',       # the colours of sample 7 - s in the columns of sample s
    'channel_rotated',       # channel c + 1 mod 3 in the column of channel c
    'ref_nos_wrapped',       # ref_nos taken modulo nv instead of clamped into 0 .. nv - 1
    'eps_dropped',           # z3d = 1 / (1 - dn)
    'head_padding_weight',   # fused head: the last view's colours count twice, as a padding view with non-zero weights could make them
)
APPLIES = dict(
    refine_input=('tap_x1_to_x0', 'floor_to_round', 'align_corners_off', 'border_padding', 'xy_swapped', 'layouts_swapped', 'view_next',
                  'sample_reversed', 'channel_rotated', 'eps_dropped'),
    refine_input_train=('tap_x1_to_x0', 'floor_to_round', 'align_corners_off', 'xy_swapped', 'y_flip_missing', 'inside_strict',
                        'z_without_abs', 'mean_over_all', 'valid_one_channel', 'layouts_swapped', 'view_next', 'sample_reversed',
                        'channel_rotated', 'ref_nos_wrapped', 'eps_dropped'),
    warp_trt=('tap_x1_to_x0', 'floor_to_round', 'align_corners_off', 'border_padding', 'xy_swapped', 'channel_rotated'),
    warp_train=('tap_x1_to_x0', 'floor_to_round', 'align_corners_off', 'xy_swapped', 'y_flip_missing', 'inside_strict',
                'z_without_abs', 'channel_rotated'),
)       # border_padding: not in the training forms — their inside mask leaves a tap outside the image only at X = Wf - 1, with weight 0


def bound(d, mag):
    return d * U * mag * (1 + 2.0 ** -10) + d * 2.0 ** -126


# ------------------------------------------------------------------------------------------------ values of any back end as arrays
def _shape(x):
    return np.shape(x.v) if isinstance(x, V) else np.shape(x)


def _map(x, f):
    """An array function (reshape, transpose, roll, index) applied to a back-end value."""
    return V(f(x.v), f(x.t)) if isinstance(x, V) else f(x)


def _stack(xs, axis=-1):
    shp = np.broadcast_shapes(*[_shape(x) for x in xs])
    if isinstance(xs[0], V):
        return V(np.stack([np.broadcast_to(x.v, shp) for x in xs], axis), np.stack([np.broadcast_to(x.t, shp) for x in xs], axis))
    return np.stack([np.broadcast_to(x, shp) for x in xs], axis)


def _cat(xs, axis=-1):
    if isinstance(xs[0], V):
        return V(np.concatenate([x.v for x in xs], axis), np.concatenate([x.t for x in xs], axis))
    return np.concatenate(xs, axis)


def _finite(A, x):
    v = np.asarray(A.val(x), np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(v) & (np.abs(v) < FIN_LIM)


def _pool(img):
    """max |texel| over the 4x4 neighbourhood (x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2) of the cell with origin (x0, y0), zero padding
    included, for x0 in -2 .. Wf, y0 in -2 .. Hf: [nv, 3, Hf + 3, Wf + 3], indexed at (y0 + 2, x0 + 2)."""
    a = np.pad(np.abs(np.asarray(img, np.float64)), ((0, 0), (0, 0), (3, 3), (3, 3)))
    Hf, Wf = img.shape[2:]
    return np.max([a[:, :, i:i + Hf + 3, j:j + Wf + 3] for i in range(4) for j in range(4)], 0)


# ------------------------------------------------------------------------------------------------ the kernels' formulas
def _fetch(A, img, view, X, Y, M=None, mask=None):
    """bilinear_setup and the four taps (pnrf_geom.h): three colour values shaped like X.  img [nv,3,Hf,Wf] float32; view: integer array
    broadcastable to X; mask: the training form's inside mask (a sample outside it fetches nothing).  A tap outside the image
    contributes an exact 0, and so does every tap of a sample whose coordinates are not finite (or reach 1e9)."""
    Hf, Wf = img.shape[2:]
    if M == 'xy_swapped':
        X, Y = Y, X
    one, two, zero = A.const(1.0, X), A.const(2.0, X), A.const(0.0, X)
    wm, hm = A.const(float(Wf - 1), X), A.const(float(Hf - 1), X)
    xn = A.sub(A.div(A.mul(two, X), wm), one)
    yn = A.sub(A.div(A.mul(two, Y), hm), one)
    if M == 'align_corners_off':
        ix = A.div(A.sub(A.mul(A.add(xn, one), A.const(float(Wf), X)), one), two)
        iy = A.div(A.sub(A.mul(A.add(yn, one), A.const(float(Hf), X)), one), two)
    else:
        ix = A.mul(A.div(A.add(xn, one), two), wm)
        iy = A.mul(A.div(A.add(yn, one), two), hm)
    fin = _finite(A, ix) & _finite(A, iy)
    rnd = A.rint if M == 'floor_to_round' else A.floor
    fx, fy = rnd(ix), rnd(iy)
    wx1, wx0 = A.sub(ix, fx), A.sub(A.add(fx, one), ix)
    wy1, wy0 = A.sub(iy, fy), A.sub(A.add(fy, one), iy)
    with np.errstate(invalid='ignore'):
        x0 = np.where(fin, A.val(fx), -4).astype(np.int64)
        y0 = np.where(fin, A.val(fy), -4).astype(np.int64)
    live = fin if mask is None else fin & mask
    view = np.broadcast_to(view, x0.shape)
    cell_taint = (fx.t | fy.t) if isinstance(A, Cert) else None
    pool = _pool(img) if isinstance(A, Mag) else None
    out = []
    for c in range(3):
        cell_mag = pool[view, c, np.clip(y0, -2, Hf) + 2, np.clip(x0, -2, Wf) + 2] if pool is not None else None
        terms = []
        for dy, dx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
            xx, yy = x0 + dx, y0 + dy
            ok = live if M == 'border_padding' else live & (xx >= 0) & (xx < Wf) & (yy >= 0) & (yy < Hf)
            xr = x0 if (M == 'tap_x1_to_x0' and dx == 1) else xx
            t = A.texel(img[view, c, np.clip(yy, 0, Hf - 1), np.clip(xr, 0, Wf - 1)], cell_taint, cell_mag)
            terms.append(A.where(ok, A.mul(t, A.mul(wx, wy)), zero))
        out.append(A.add(A.add(A.add(terms[0], terms[1]), terms[2]), terms[3]))
    return out, dict(X=X, Y=Y, xn=xn, yn=yn, ix=ix, iy=iy, fin=fin, x0=x0, y0=y0)


def _z3d(A, dn, eps, M=None):
    one = A.const(1.0, dn)
    diff = A.sub(one, dn) if M == 'eps_dropped' else A.sub(A.sub(one, dn), A.const(eps, dn))
    return A.div(one, diff), diff


def project(A, w, Mrow, homogeneous=None):
    """p = M (w, 1) and the perspective division: X, Y, p[2].  w: three back-end values; Mrow(r, c): the matrix entries as back-end
    values; homogeneous: the fourth coordinate where the kernel multiplies by it (warp_trt), None where it is the constant 1."""
    p = []
    for r in range(3):
        last = Mrow(r, 3) if homogeneous is None else A.mul(Mrow(r, 3), homogeneous)
        p.append(A.add(A.add(A.add(A.mul(Mrow(r, 0), w[0]), A.mul(Mrow(r, 1), w[1])), A.mul(Mrow(r, 2), w[2])), last))
    return A.div(p[0], p[2]), A.div(p[1], p[2]), p[2]


def project_train(A, w, P, K, Hf, Wf, M=None):
    """project_train (pnrf_ops.hip): P(r, c) the camera-to-world pose entries, K(i) the nine intrinsics -> X, Y, inside, c2.z."""
    c2 = []
    for i in range(3):
        r0, r1, r2 = P(0, i), P(1, i), P(2, i)
        tt = A.neg(A.add(A.add(A.mul(r0, P(0, 3)), A.mul(r1, P(1, 3))), A.mul(r2, P(2, 3))))
        c2.append(A.add(A.add(A.add(A.mul(r0, w[0]), A.mul(r1, w[1])), A.mul(r2, w[2])), tt))
    z = A.add_const(c2[2] if M == 'z_without_abs' else A.abs(c2[2]), C1E8)
    cx, cy = A.div(c2[0], z), A.div(c2[1], z)
    if M != 'y_flip_missing':
        cy = A.neg(cy)
    X = A.add(A.add(A.mul(K(0), cx), A.mul(K(1), cy)), K(2))
    Y = A.add(A.add(A.mul(K(3), cx), A.mul(K(4), cy)), K(5))
    one, two = A.const(1.0, X), A.const(2.0, X)
    xn = A.sub(A.div(A.mul(two, X), A.const(float(Wf - 1), X)), one)
    yn = A.sub(A.div(A.mul(two, Y), A.const(float(Hf - 1), X)), one)
    mone = A.neg(one)
    if M == 'inside_strict':
        inside = A.lt(xn, one) & A.gt(xn, mone) & A.lt(yn, one) & A.gt(yn, mone)
    else:
        inside = A.le(xn, one) & A.ge(xn, mone) & A.le(yn, one) & A.ge(yn, mone)
    return X, Y, inside, c2[2]


def _plucker(A, rays, dn):
    """The 48 sample Pluecker columns [n, 8, 6]: unit_dir, the sample point o + d dn, cross_rn (pnrf_geom.h)."""
    r = [A.inp(rays[:, c:c + 1]) for c in range(6)]
    n2 = A.fma(r[5], r[5], A.fma(r[4], r[4], A.mul(r[3], r[3])))
    nrm = A.sqrt(n2)
    tiny = A.const(1e-12, nrm)
    den = A.where(A.lt(nrm, tiny), tiny, nrm)
    h = [A.div(r[3 + c], den) for c in range(3)]
    p = [A.add(r[c], A.mul(r[3 + c], dn)) for c in range(3)]
    m = [A.fma(p[1], h[2], A.neg(A.mul(p[2], h[1]))), A.fma(p[2], h[0], A.neg(A.mul(p[0], h[2]))), A.fma(p[0], h[1], A.neg(A.mul(p[1], h[0])))]
    return _stack(h + m, -1)


def _columns(cols, layout, M):
    """Colours [n, nb, 8, 3] -> the epi columns [n, 24 nb]: layout 0 (k*8+s)*3+c, layout 1 s*(3 nb)+k*3+c."""
    if M == 'view_next':
        cols = _map(cols, lambda a: np.roll(a, -1, 1))
    if M == 'sample_reversed':
        cols = _map(cols, lambda a: a[:, :, ::-1])
    if M == 'channel_rotated':
        cols = _map(cols, lambda a: np.roll(a, -1, 3))
    if M == 'layouts_swapped':
        layout = 1 - layout
    if layout == 1:
        cols = _map(cols, lambda a: a.transpose(0, 2, 1, 3))
    return _map(cols, lambda a: a.reshape(a.shape[0], -1))


def replay_refine_input(A, inp, nb=None, mutation=None):
    """refine_input_kernel.  inp: rays, or_rays [n,11], depth [n,8], img [>= nb,3,Hf,Wf], proj [>= nb,3,4], eps.  -> out [n, 48 + 24 nb]."""
    M = mutation
    nb = inp['proj'].shape[0] if nb is None else nb
    img, proj = inp['img'][:nb], inp['proj'][:nb]
    dn = A.inp(inp['depth'])
    z3d, diff = _z3d(A, _map(dn, lambda a: a[:, None, :]), inp['eps'], M)
    orr = inp['or_rays']
    w = [A.add(A.inp(orr[:, c, None, None]), A.mul(A.inp(orr[:, 3 + c, None, None]), z3d)) for c in range(3)]
    X, Y, p2 = project(A, w, lambda r, c: A.inp(proj[None, :, r, c, None]))
    col, aux = _fetch(A, img, np.arange(nb)[None, :, None], X, Y, M)
    out = _cat([_map(_plucker(A, inp['rays'], dn), lambda a: a.reshape(a.shape[0], 48)), _columns(_stack(col, -1), 0, M)], 1)
    return dict(out=out), dict(aux, p2=p2, diff=diff)


def clamp_views(ref_nos, nv, mutation=None):
    return np.mod(ref_nos, nv) if mutation == 'ref_nos_wrapped' else np.clip(ref_nos, 0, nv - 1)


def replay_refine_input_train(A, inp, layout=0, mutation=None):
    """refine_input_train_kernel.  inp: rays, or_rays, depth, img [nv,3,Hf,Wf], poses [nv,3,4], K [3,3], ref_nos [n,4] int64, eps.
    -> out [n, 144]."""
    M = mutation
    img, poses, K = inp['img'], inp['poses'], inp['K']
    nv, _, Hf, Wf = img.shape
    view = clamp_views(inp['ref_nos'], nv, M)[:, :, None]                       # [n,4,1]
    dn = A.inp(inp['depth'])
    z3d, diff = _z3d(A, _map(dn, lambda a: a[:, None, :]), inp['eps'], M)
    orr = inp['or_rays']
    w = [A.add(A.inp(orr[:, c, None, None]), A.mul(A.inp(orr[:, 3 + c, None, None]), z3d)) for c in range(3)]
    X, Y, inside, c2z = project_train(A, w, lambda r, c: A.inp(poses[view, r, c]), lambda i: A.inp(np.full((1, 1, 1), K.reshape(9)[i])), Hf, Wf, M)
    v, aux = _fetch(A, img, view, X, Y, M, mask=inside)                        # three values [n,4,8]
    zero, one = A.const(0.0, v[0]), A.const(1.0, v[0])
    vsum = v[0] if M == 'valid_one_channel' else A.add(A.add(v[0], v[1]), v[2])
    valid = A.where(A.gt(vsum, zero), one, zero)
    k_of = lambda x, k: _map(x, lambda a: a[:, k:k + 1])
    cnt, m = k_of(zero, 0), [k_of(zero, 0)] * 3
    for k in range(4):
        vk = k_of(one if M == 'mean_over_all' else valid, k)
        cnt = A.add(cnt, vk)
        m = [A.add(m[c], A.mul(vk, k_of(v[c], k))) for c in range(3)]
    den = A.round_add(cnt, C1E6)
    col = [A.add(A.mul(v[c], valid), A.mul(A.div(m[c], den), A.sub(one, valid))) for c in range(3)]
    out = _cat([_map(_plucker(A, inp['rays'], dn), lambda a: a.reshape(a.shape[0], 48)), _columns(_stack(col, -1), layout, M)], 1)
    return dict(out=out), dict(aux, inside=inside, c2z=c2z, diff=diff, valid=A.val(valid), vsum=A.val(vsum), cnt=A.val(cnt))


def _warp_rays(A, inp, comps):
    ro, rd = inp['ro1'], inp['rd1']
    if ro.ndim == 2:
        ro, rd = ro[None], rd[None]
    dep = A.inp(inp['depth'])
    return [A.add(A.inp(ro[:, c]), A.mul(A.inp(rd[:, c]), dep)) for c in range(comps)]


def replay_warp_trt(A, inp, mutation=None):
    """warp_trt_kernel.  inp: img [B,3,Hf,Wf], depth [B,n], ro1 / rd1 [4,n] or [B,4,n], w2c [B,3,4].  -> out [B,3,n]."""
    w = _warp_rays(A, inp, 4)
    X, Y, p2 = project(A, w, lambda r, c: A.inp(inp['w2c'][:, r, c, None]), homogeneous=w[3])
    col, aux = _fetch(A, inp['img'], np.arange(inp['img'].shape[0])[:, None], X, Y, mutation)
    out = _stack(col, 1)
    if mutation == 'channel_rotated':
        out = _map(out, lambda a: np.roll(a, -1, 1))
    return dict(out=out), dict(aux, p2=p2)


def replay_warp_train(A, inp, mutation=None):
    """warp_train_kernel.  inp: img, depth [B,n], ro1 / rd1 [3,n] or [B,3,n], c2w2 [B,3,4], K [B,3,3].  -> out [B,3,n]."""
    w = _warp_rays(A, inp, 3)
    Hf, Wf = inp['img'].shape[2:]
    X, Y, inside, c2z = project_train(A, w, lambda r, c: A.inp(inp['c2w2'][:, r, c, None]), lambda i: A.inp(inp['K'].reshape(-1, 9)[:, i, None]),
                                      Hf, Wf, mutation)
    col, aux = _fetch(A, inp['img'], np.arange(inp['img'].shape[0])[:, None], X, Y, mutation, mask=inside)
    out = _stack(col, 1)
    if mutation == 'channel_rotated':
        out = _map(out, lambda a: np.roll(a, -1, 1))
    return dict(out=out), dict(aux, inside=inside, c2z=c2z)


REPLAYS = dict(refine_input=replay_refine_input, refine_input_train=replay_refine_input_train, warp_trt=replay_warp_trt, warp_train=replay_warp_train)


def emulate(kernel, inp, **kw):
    """The F32 replay: the kernel's specification as a float32 array."""
    with np.errstate(all='ignore'):
        return np.asarray(REPLAYS[kernel](F32(), inp, **kw)[0]['out'], np.float32)


def intermediates(kernel, inp, **kw):
    """The F32 replay's intermediates (X, Y, xn, yn, p2 / c2z, diff = 1 - dn - eps, fin, inside, valid, vsum, cnt, x0, y0) as arrays."""
    with np.errstate(all='ignore'):
        return {k: np.asarray(v) for k, v in REPLAYS[kernel](F32(), inp, **kw)[1].items()}


def run64(kernel, inp, absorb=False, **kw):
    """The float64 run of the same formulas: (values, magnitudes, the intermediates' values).  absorb: the denominator |c2.z| + 1e-8f is
    rounded to fp32 — on the exact sets, where the certificate shows that this rounding gives |c2.z| back, the float64 run then divides
    by the same number as the kernels and is their answer to the bit."""
    A = Mag(absorb=absorb)
    with np.errstate(all='ignore'):
        out, aux = REPLAYS[kernel](A, inp, **kw)
    return out['out'].v, out['out'].t, {k: (x.v if isinstance(x, V) else x) for k, x in aux.items()}


def reference(kernel, inp, **kw):
    return run64(kernel, inp, **kw)[0]


def certify(kernel, inp, taint_ok=None, **kw):
    """The exact sets' certificate: (expected float32 output, taint mask).  Raises when an element outside taint_ok (a mask) is inexact
    or a branch was decided on an inexact finite value."""
    A = Cert()
    with np.errstate(all='ignore'):
        out = REPLAYS[kernel](A, inp, **kw)[0]['out']
    bad = out.t if taint_ok is None else out.t & ~taint_ok
    assert 'comparison of an inexact value' not in A.why, (kernel, A.why)
    assert not bad.any(), f'{kernel}: {int(bad.sum())} inexact elements ({A.why})'
    assert np.isfinite(out.v).all(), kernel
    return out.v.astype(np.float32), out.t


def worst_ratio(got, ref, bnd):
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape == np.shape(bnd), (g.shape, r.shape, np.shape(bnd))
    with np.errstate(invalid='ignore'):
        q = np.abs(g - r) / bnd
    q = np.where(np.isfinite(g) & np.isfinite(q), q, np.inf)
    return float(q.max()) if q.size else 0.0


def filled_columns(inp, layout):
    """refine_input_train: the mask [n, 144] of the mean-fill columns (an invalid entry beside at least one valid view)."""
    a = intermediates('refine_input_train', inp, layout=layout)
    f = np.broadcast_to(((a['valid'] == 0) & (a['cnt'] > 0))[..., None], a['valid'].shape + (3,))
    return np.concatenate([np.zeros((f.shape[0], 48), bool), _columns(f, layout, None)], 1)


def ulp_distance(a, b):
    """|a - b| in units in the last place of float32 (a, b float32 arrays of finite values)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ the oracle, in float64
@contextlib.contextmanager
def _float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _t(x):
    return torch.tensor(np.asarray(x, np.float64))


def oracle(kernel, inp, nb=None):
    """oracle.pronerf_oracle's statement of the same operation in float64: the 24 nb colour columns (refine_input: project_trt;
    refine_input_train, layout 0: project_train on the clamped ref_nos) or the warp's [B,3,n] (warp_train)."""
    with _float64():
        if kernel == 'refine_input':
            nb = inp['proj'].shape[0] if nb is None else nb
            return orc.project_trt(_t(inp['img'][:nb]), _t(inp['proj'][:nb]), _t(inp['or_rays'][:, 0:3]), _t(inp['or_rays'][:, 3:6]), _t(inp['depth']),
                                   eps=float(inp['eps'])).numpy()
        if kernel == 'refine_input_train':
            ref = torch.tensor(clamp_views(inp['ref_nos'], inp['img'].shape[0]))
            return orc.project_train(_t(inp['img']), _t(inp['poses']), _t(inp['K']), _t(inp['or_rays'][:, 0:3]), _t(inp['or_rays'][:, 3:6]),
                                     _t(inp['depth']), ref, eps=float(inp['eps']))[0].numpy()
        if kernel == 'warp_train':
            assert inp['ro1'].ndim == 2
            return orc.warp_train(*(_t(inp[k]) for k in ('img', 'depth', 'ro1', 'rd1', 'c2w2', 'K')))[0].numpy()
    raise KeyError(kernel)


# ------------------------------------------------------------------------------------------------ input sets
RAY_KEYS = ('rays', 'or_rays', 'depth', 'ref_nos')


def head(inp, n):
    """The first n rays of a refine_input / refine_input_train set."""
    return {k: (v[:n] if k in RAY_KEYS else v) for k, v in inp.items()}


def tile(inp, n):
    """n rays that repeat the rays of a refine_input / refine_input_train set."""
    idx = np.arange(n) % inp['rays'].shape[0]
    return {k: (v[idx] if k in RAY_KEYS else v) for k, v in inp.items()}


def warp_head(inp, B, n, shared):
    """B views and n pixels of a warp set; shared: one [C,n] copy of the rays for every view (ray_bstride = 0)."""
    out = {k: (v[:B] if k in ('img', 'w2c', 'c2w2', 'K') else v) for k, v in inp.items()}
    out['depth'] = np.ascontiguousarray(inp['depth'][:B, :n])
    for k in ('ro1', 'rd1'):
        out[k] = np.ascontiguousarray(inp[k][0, :, :n] if shared else inp[k][:B, :, :n])
    return out


def warp_tile(inp, n):
    idx = np.arange(n) % inp['depth'].shape[1]
    return dict(inp, depth=np.ascontiguousarray(inp['depth'][:, idx]), ro1=np.ascontiguousarray(inp['ro1'][..., idx]),
                rd1=np.ascontiguousarray(inp['rd1'][..., idx]))


ZERO_VIEW = 4                          # the training sets' black view


def exact_images(nv, Hf, Wf, zero_view=None):
    """Texels that are distinct integers in 1 .. 4093: a fixed permutation (multiplication modulo the prime 4093) of the running index of
    (view, channel, y, x) — not linear in x or y, so that no displaced cell interpolates to the same value.  View 1 carries a 2x2 block
    of zeros (x in 2 .. 3, y in 1 .. 2, every channel).  zero_view (the training sets): one view black everywhere — its inside samples'
    colours sum to exactly 0 in every precision (a black block would do so in fp32 only: float64 does not absorb the 1e-8 of
    |c2.z| + 1e-8, and a sample on the block's edge picks up 1e-8 of the texel next to it, which flips ``valid``)."""
    assert nv * 3 * Hf * Wf < 4093
    img = ((np.arange(nv * 3 * Hf * Wf, dtype=np.int64) * 1663) % 4093 + 1).reshape(nv, 3, Hf, Wf).astype(np.float32)
    if zero_view is not None:
        img[zero_view] = 0
        img[(zero_view + 1) % nv, 0] = 0                           # a view without red: valid through the other channels alone
    elif nv > 1:
        img[1, :, 1:3, 2:4] = 0
    return img


def _exact_rays(rs, n, size, training):
    """or_rays, depth, rays of an exact set (module docstring).  Per ray the samples' j = jb .. jb + 3 and the direction is a small
    integer times 2^-(jb+2), so the world points are quarter multiples within a few texels of the image whatever the depth."""
    Hf, Wf = SIZES[size]
    sc = float(size + 1)
    jb = rs.randint(0, 7, n)
    j = jb[:, None] + rs.randint(0, 4, (n, 8))
    depth = 1.0 - 2.0 ** -10 - 2.0 ** -j.astype(np.float64)
    i = np.arange(n)
    depth[i % 16 == 3, 2] = 1.0 - 2.0 ** -10                     # 1 - dn - eps == 0: z3d = inf
    depth[i % 16 == 5, 6] = 1.0 - 2.0 ** -11                     # 1 - dn - eps == -2^-11: z3d = -2048
    orr = rs.randn(n, 11)
    orr[:, 0] = sc * rs.randint(-8, 9, n) / 4.0
    orr[:, 1] = sc * rs.randint(-4, 5, n) / 4.0
    orr[:, 2] = rs.choice(np.array([1, 1, 1, 0.5, -1, 0.25] if training else [1, 1, 1, 1, 0.5, -1, 0.25, 0]), n)
    orr[:, 3] = sc * rs.randint(-2, 3, n) * 2.0 ** -(jb + 2.0)
    orr[:, 4] = sc * rs.randint(-1, 2, n) * 2.0 ** -(jb + 2.0)
    orr[:, 5] = 0
    if not training and n > 11:                                   # rays 8 .. 11: the four corners of view 0 (X = w_x + cx, Y = w_y + cy, p[2] = 1)
        for q in range(4):
            orr[8 + q, 0:6] = [(Wf - 1) / 2.0 * (1 if q & 1 else -1), (Hf - 1) / 2.0 * (1 if q & 2 else -1), 1, 0, 0, 0]
    rays = rs.randn(n, 11)
    rays[:, 0:3] = rs.randint(-8, 9, (n, 3)) / 4.0
    rays[:, 3:6] = 0
    rays[i, 3 + rs.randint(0, 3, n)] = rs.choice([-1.0, 1.0], n) * 2.0 ** rs.randint(-2, 3, n)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(rays), f(orr), f(depth), jb


def exact_inference(size=0, n=N_SET, seed=0):
    """The exact set of refine_input: eight views whose 3x4 matrices scale, mirror, shear and shift the quarter-multiple world points,
    with p[2] = g o_z + h in {+-1, +-1/2, 1/4, 1/8, 0}."""
    Hf, Wf = SIZES[size]
    rs = np.random.RandomState(4000 + 10 * size + seed)
    rays, orr, depth, _ = _exact_rays(rs, n, size, False)
    cx, cy = (Wf - 1) / 2.0, (Hf - 1) / 2.0
    a = [1, 1, -1, 2, 1, 1, -2, 1]; c = [0, 0, 0, 0, 1, 0, 0, -1]; d = [1, -1, 1, 1, 2, 1, 1, 1]
    bx = [0, 1, -1, 0, 0.25, -2, 0.5, 3]; by = [0, 0.5, 0, -1, 1, 0.25, 0, -0.75]
    g = [1, 1, 1, 0.5, 1, 0, -1, 1]; h = [0, 0, 0, 0, 0, 1, 0, 0]
    proj = np.zeros((8, 3, 4), np.float32)
    for k in range(8):
        proj[k] = [[a[k], c[k], 0, cx + bx[k]], [0, d[k], 0, cy + by[k]], [0, 0, g[k], h[k]]]
    return dict(rays=rays, or_rays=orr, depth=depth, img=exact_images(8, Hf, Wf), proj=proj, eps=EPS_EXACT)


def exact_poses():
    """Six camera-to-world poses: signed permutations of x and y with z kept or mirrored, translations in quarters with t_z = 0 — so
    c2.z = +-o_z, a power of two >= 1/4 (|c2.z| + 1e-8f rounds back to |c2.z|)."""
    R = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, -1, 0], [0, 0, -1]], [[0, 1, 0], [1, 0, 0], [0, 0, 1]],
         [[-1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, -1]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]]]
    t = [[0, 0, 0], [0.25, -0.5, 0], [-1, 0.75, 0], [1.5, 0, 0], [0, 1, 0], [-2.25, -1, 0]]
    return np.concatenate([np.array(R, np.float32), np.array(t, np.float32)[:, :, None]], 2)


def exact_K(size, fx=1.0, skew=0.0):
    Hf, Wf = SIZES[size]
    return np.array([[fx, skew, (Wf - 1) / 2.0], [0.5 * skew, 1, (Hf - 1) / 2.0], [0, 0, 1]], np.float32)


def exact_training(size=0, n=N_SET, seed=0):
    """The exact set of refine_input_train.  ref_nos holds duplicates within a ray, entries below 0 and entries >= nv (clamped)."""
    Hf, Wf = SIZES[size]
    rs = np.random.RandomState(5000 + 10 * size + seed)
    rays, orr, depth, _ = _exact_rays(rs, n, size, True)
    ref = rs.randint(0, NV_TRAIN, (n, 4)).astype(np.int64)
    i = np.arange(n)
    ref[i % 8 == 1, 2] = ref[i % 8 == 1, 0]
    ref[i % 8 == 2, 1] = rs.choice([-1, -3], int((i % 8 == 2).sum()))
    ref[i % 8 == 4, 3] = rs.choice([NV_TRAIN, NV_TRAIN + 3], int((i % 8 == 4).sum()))
    far = i % 8 == 6                                              # rays far from every image: no neighbour valid
    orr[far, 0] = 64.0
    for q in range(4):                                            # rays 8 .. 11: the four corners in view 0 (identity pose; K = exact_K(size, 1, 1))
        a, b = (Wf - 1) / 2.0 * (1 if q & 1 else -1), (Hf - 1) / 2.0 * (1 if q & 2 else -1)
        orr[8 + q, 0:6] = [2 * (a - b), a - 2 * b, 1, 0, 0, 0]
        ref[8 + q, 0] = 0
    return dict(rays=rays, or_rays=orr, depth=depth, img=exact_images(NV_TRAIN, Hf, Wf, zero_view=ZERO_VIEW), poses=exact_poses(), K=exact_K(size, 1.0, 1.0),
                ref_nos=ref, eps=EPS_EXACT)


def exact_warp(kind, size=0, n=N_SET, seed=0):
    """The exact set of a warp operator ('trt' | 'train'): three views; view b's rays are view 0's with mirrored components, so that the
    per-view form ([B,C,n]) and the shared form (view 0's rays for every view: warp_head) both keep the depths 2^j matched to the
    directions' 2^-(jb+2); one depth per 16 pixels is inf."""
    Hf, Wf = SIZES[size]
    rs = np.random.RandomState(6000 + 10 * size + seed + (100 if kind == 'train' else 0))
    B = 3
    _, orr, _, jb = _exact_rays(rs, n, size, kind == 'train')
    if kind == 'train':                                           # pixels 8 .. 11: the four corners of view 0 (as exact_training's rays 8 .. 11)
        for q in range(4):
            a, b = (Wf - 1) / 2.0 * (1 if q & 1 else -1), (Hf - 1) / 2.0 * (1 if q & 2 else -1)
            orr[8 + q, 0:6] = [2 * (a - b), a - 2 * b, 1, 0, 0, 0]
    depth = 2.0 ** (jb[None, :] + rs.randint(0, 4, (B, n)))
    depth[:, 3::16] = np.inf
    C = 4 if kind == 'trt' else 3
    ro1, rd1 = np.zeros((B, C, n), np.float32), np.zeros((B, C, n), np.float32)
    for b, sign in enumerate(((1, 1, 1), (-1, 1, 1), (1, -1, 1))):
        ro1[b, :3], rd1[b, :3] = (orr[:, 0:3] * sign).T, (orr[:, 3:6] * sign).T
    if kind == 'trt':
        ro1[:, 3] = 1
        return dict(img=exact_images(B, Hf, Wf), depth=depth.astype(np.float32), ro1=ro1, rd1=rd1, w2c=exact_inference(size)['proj'][[0, 3, 6]].copy())
    K = np.stack([exact_K(size, 1.0, 1.0), exact_K(size, 2.0, 0.0), exact_K(size, 1.0, 0.0)])
    return dict(img=exact_images(B, Hf, Wf), depth=depth.astype(np.float32), ro1=ro1, rd1=rd1, c2w2=exact_poses()[[0, 2, 4]].copy(), K=K)


def _rot(rs, n, amp):
    """n rotation matrices: Rodrigues of random vectors of length ~ amp (float64)."""
    v = rs.randn(n, 3) * amp
    th = np.linalg.norm(v, axis=1)[:, None, None] + 1e-12
    k = v / th[:, :, 0]
    Kx = np.zeros((n, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def general_images(rs, nv):
    Hf, Wf = GENERAL_SIZE
    return rs.uniform(0.05, 1.0, (nv, 3, Hf, Wf)).astype(np.float32)


def _general_rays(rs, n):
    orr = rs.randn(n, 11)
    orr[:, 0:3] = rs.uniform(-0.3, 0.3, (n, 3))
    orr[:, 3:5] = rs.uniform(-0.6, 0.6, (n, 2))
    orr[:, 5] = rs.uniform(0.8, 1.2, n)
    depth = np.sort(rs.uniform(0.5, 0.9, (n, 8)), 1)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(rs.randn(n, 11)), f(orr), f(depth)


GENERAL_K = np.array([[20, 0.5, 9], [0.25, 20, 6], [0, 0, 1]], np.float32)


def general_inference(n=N_SET, seed=0):
    """The general set of refine_input: eight views K [R | t] with small rotations, points 2 .. 10 in front of them, X in about -3 .. 21."""
    rs = np.random.RandomState(7000 + seed)
    rays, orr, depth = _general_rays(rs, n)
    Rt = np.concatenate([_rot(rs, 8, 0.15), rs.uniform(-0.5, 0.5, (8, 3, 1))], 2)
    proj = (GENERAL_K.astype(np.float64)[None] @ Rt).astype(np.float32)
    return dict(rays=rays, or_rays=orr, depth=depth, img=general_images(rs, 8), proj=proj, eps=EPS_GENERAL)


def margin_ok(aux):
    """Per sample: the float64 normalised coordinates keep 2^-12 from |xn| = 1 and |yn| = 1 (a non-finite coordinate counts as near)."""
    with np.errstate(invalid='ignore'):
        far = (np.abs(np.abs(aux['xn']) - 1) >= 2.0 ** -12) & (np.abs(np.abs(aux['yn']) - 1) >= 2.0 ** -12)
    return far


def general_training(n=N_SET, seed=0):
    """The general set of refine_input_train; rays with a coordinate within 2^-12 of the inside mask's boundary are redrawn."""
    rs = np.random.RandomState(8000 + seed)
    poses = np.concatenate([_rot(rs, NV_TRAIN, 0.15), rs.uniform(-0.5, 0.5, (NV_TRAIN, 3, 1))], 2).astype(np.float32)
    img = general_images(rs, NV_TRAIN)

    def draw(m):
        rays, orr, depth = _general_rays(rs, m)
        ref = rs.randint(-1, NV_TRAIN + 1, (m, 4)).astype(np.int64)
        return dict(rays=rays, or_rays=orr, depth=depth, ref_nos=ref)
    inp = dict(draw(n), img=img, poses=poses, K=GENERAL_K.copy(), eps=EPS_GENERAL)
    for _ in range(8):
        bad = np.flatnonzero(~margin_ok(run64('refine_input_train', inp)[2]).all((1, 2)))
        if not bad.size:
            return inp
        new = draw(bad.size)
        for k in new:
            inp[k][bad] = new[k]
    raise AssertionError('general_training: rays on the mask boundary remain')


def general_warp(kind, n=N_SET, seed=0):
    """The general set of a warp operator: three views, rays per view; the training form redraws pixels on the mask boundary."""
    rs = np.random.RandomState(9000 + seed + (100 if kind == 'train' else 0))
    B = 3
    C = 4 if kind == 'trt' else 3
    Rt = np.concatenate([_rot(rs, B, 0.15), rs.uniform(-0.5, 0.5, (B, 3, 1))], 2)
    img = general_images(rs, B)

    def draw(m):
        _, orr, _ = _general_rays(rs, B * m)
        orr = orr.reshape(B, m, 11)
        ro1, rd1 = np.zeros((B, C, m), np.float32), np.zeros((B, C, m), np.float32)
        ro1[:, :3], rd1[:, :3] = orr[:, :, 0:3].transpose(0, 2, 1), orr[:, :, 3:6].transpose(0, 2, 1)
        if kind == 'trt':
            ro1[:, 3] = 1
        return dict(depth=rs.uniform(2, 10, (B, m)).astype(np.float32), ro1=ro1, rd1=rd1)
    inp = dict(draw(n), img=img)
    if kind == 'trt':
        inp['w2c'] = (GENERAL_K.astype(np.float64)[None] @ Rt).astype(np.float32)
        return inp
    inp['c2w2'] = Rt.astype(np.float32)
    inp['K'] = np.stack([GENERAL_K, GENERAL_K * np.array([[1.25], [1.0], [1.0]], np.float32), GENERAL_K])
    for _ in range(8):
        ok = np.ones(n, bool)
        for shared in (False, True):                              # both ray forms the GPU test runs
            ok &= margin_ok(run64('warp_train', warp_head(inp, B, n, shared))[2]).all(0)
        bad = np.flatnonzero(~ok)
        if not bad.size:
            return inp
        new = draw(bad.size)
        for k in new:
            inp[k][..., bad] = new[k]
    raise AssertionError('general_warp: pixels on the mask boundary remain')


# ------------------------------------------------------------------------------------------------ the fused head (pnrf_refine_project_fwd)
# Its colours are observable only through the net, so it runs on the integer nets of tests/exact_nets.py (input box: the integers 0, 1, 2).
# Images: 17 x 33, constant 4 x 4 blocks of 0 or 2 (a fixed pseudo-random pattern), last row and column 0.  A true colour 0 beside a
# non-zero texel does not survive a 1 ulp slip of a coordinate (1e-6 is a normal fp16 / bf16 number), hence locally constant images;
# the price: a tap displaced by one texel INSIDE a block is invisible — single-texel displacement in the head is held by the half-way
# coordinates alone.  Two kinds of rays:
#   * still rays (direction 0): X, Y on a block's two inner rows / columns (4 i + 1, 4 i + 2) or half-way between two blocks
#     (4 i + 3.5: colour 0, 1 or 2), never half-way in both axes; the same colour at all 8 samples;
#   * moving rays (direction (0, 0, e_z), views with a non-zero M[0][2]): X_s = a ox + m e_z z3d_s + bx walks across the blocks with
#     the sample's depth.  (ox, e_z) are drawn by rejection on the float64 reference — input selection — so that every sample of every
#     such view lies at least 1/4 texel inside a block (four equal taps: colour 0 or 2 after rounding to fp16 / bf16, whatever a few
#     ulp of v_rcp_f32 and the FMAs do to X) or more than 1 1/4 texels outside the image (0), and the samples do not all share a block.
#     They hold the sample index, the order of dn8 / z3d, eps, the B half of view_ray and the fetch pipeline's slots.  eps = 2^-6 here
#     (a free argument of the entry point): dropping the usual 1e-5 would move no coordinate out of its block.
# p.z = g in {1/4, 1/2, 1, 2, 4} whatever the depth.  Rays: axis directions of norm 1/2 or 1, origins 0 / +-1 / +-2 of the sign that
# makes every Pluecker column an integer in [0, 2].
HEAD_SIZE = (17, 33)
HEAD_EPS = 2.0 ** -6
HEAD_VIEWS = ((1, 0, 1, 0, 1.0, 1.0), (-1, 35, 1, 4, 1.0, 0.0), (1, 4, -1, 19, 2.0, 0.0), (1, -8, 1, -4, 0.5, 0.0),   # (a, bx, d, by, g, m):
              (-1, 27, -1, 15, 1.0, 0.0), (1, 8, 1, 4, 4.0, -2.0), (1, -4, 1, 0, 0.25, 0.0), (-1, 31, 1, -8, 1.0, 0.0))  # X = a ox + m w_z + bx,
HEAD_TRIES = 160                                                                                        # Y = d oy + by, p.z = g
HEAD_MUTATIONS = ('tap_x1_to_x0', 'floor_to_round', 'align_corners_off', 'border_padding', 'xy_swapped', 'layouts_swapped', 'view_next',
                  'sample_reversed', 'channel_rotated', 'eps_dropped', 'head_padding_weight')


def head_images(nb):
    Hf, Wf = HEAD_SIZE
    nby, nbx = Hf // 4, Wf // 4
    bits = (((np.arange(nb * 3 * nby * nbx, dtype=np.int64) * 1663) % 4093) >> 3 & 1).reshape(nb, 3, nby, nbx)
    img = np.zeros((nb, 3, Hf, Wf), np.float32)
    img[:, :, :4 * nby, :4 * nbx] = 2.0 * np.repeat(np.repeat(bits, 4, 2), 4, 3)
    return img


def head_robust(X):
    """A float64 X coordinate is safe: >= 1/4 texel inside a constant block's tap range, or > 1 1/4 texels outside the image."""
    Wf = HEAD_SIZE[1]
    inside = (X >= 0) & (X < Wf - 1) & (np.mod(X, 4) >= 0.25) & (np.mod(X, 4) <= 2.75)
    return inside | (X < -1.25) | (X > Wf + 0.25)


def head_set(nb, n, seed=0):
    """rays, or_rays, depth, img, proj, eps of the fused-head exact set for nb views and n rays (depths: exact_nets.refine_rays).
    Every second ray is a moving ray if HEAD_TRIES draws find it an (ox, e_z) that head_robust accepts (else it stays still)."""
    import exact_nets as E
    Hf, Wf = HEAD_SIZE
    rs = np.random.RandomState(9500 + 31 * nb + seed)
    i = np.arange(n)
    rays = rs.uniform(-1, 1, (n, 11))
    rays[:, 6], rays[:, 7] = 0, 1
    axis = i % 3
    rays[:, 0:6] = 0
    rays[i, 3 + axis] = rs.choice([0.5, 1.0], n)
    u, v = rs.randint(0, 3, n), rs.randint(0, 3, n)               # moment (.., u, v) on the two other axes, in cyclic order
    rays[i, (axis + 2) % 3] = u                                   # h = e_a: m[a+1] = o[a+2], m[a+2] = -o[a+1]
    rays[i, (axis + 1) % 3] = -v
    pos = lambda k, lo, hi: 4 * rs.randint(lo, hi, k) + rs.choice([1, 2], k)
    ox, oy = pos(n, -1, 9).astype(np.float64), pos(n, -1, 5).astype(np.float64)
    half = rs.rand(n)
    ox = np.where(half < 0.25, 4 * rs.randint(-1, 9, n) + 3.5, ox)
    oy = np.where(half > 0.75, 4 * rs.randint(-1, 5, n) + 3.5, oy)
    depth = E.refine_rays(n)[1]
    # moving rays: (ox, e_z) by rejection on the float64 coordinates of the views that see w_z
    z3d = 1.0 / (1.0 - depth.astype(np.float64) - HEAD_EPS)
    ez, found = np.zeros(n), np.zeros(n, bool)
    for _ in range(HEAD_TRIES):
        cox = pos(n, -1, 9).astype(np.float64)                    # an inner column: the views that do not see w_z stay on it
        cez = (rs.choice([-1.0, 1.0], n) * 2.0 ** rs.uniform(-6, 0, n)).astype(np.float32).astype(np.float64)
        ok = np.ones(n, bool)
        for k, (a, bx, d, by, g, m) in enumerate(HEAD_VIEWS[:nb]):
            if m:
                X = a * cox[:, None] + m * cez[:, None] * z3d + bx
                ok &= head_robust(X).all(1)
                if k == 0:
                    blk = np.where((X >= 0) & (X < Wf - 1), np.floor(X / 4), -1)
                    ok &= blk.max(1) != blk.min(1)
        take = (i % 2 == 1) & ~found & ok
        ox, ez, found = np.where(take, cox, ox), np.where(take, cez, ez), found | take
    orr = rs.uniform(-1, 1, (n, 11))
    orr[:, 0], orr[:, 1], orr[:, 2], orr[:, 3], orr[:, 4], orr[:, 5] = ox, oy, 0, 0, 0, ez
    proj = np.zeros((nb, 3, 4), np.float32)
    for k, (a, bx, d, by, g, m) in enumerate(HEAD_VIEWS[:nb]):
        proj[k] = [[g * a, 0, g * m, g * bx], [0, g * d, 0, g * by], [0, 0, 0, g]]
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(rays=f(rays), or_rays=f(orr), depth=depth, img=head_images(nb), proj=proj, eps=HEAD_EPS)


def head_refine_in(inp, mutation=None):
    """refine_in [n, 48 + 24 nb] of the float64 reference (replay_refine_input).  Without a mutation it is rounded to the integers it
    stands for (a moving ray's colour is 2 (w00 + w01 + w10 + w11): 2 to float64 round-off), after the assertion that it is within
    2^-40 of them.  head_padding_weight does NOT replay the head's view[vv] mapping (a padding view projects into the last real view
    and meets zero weights): it shows one effect that non-zero weights there would have — the last view's colours counting twice — as
    a check that the nets are sensitive to it."""
    nb = inp['proj'].shape[0]
    x = reference('refine_input', inp, mutation=None if mutation == 'head_padding_weight' else mutation)
    if mutation is None:
        assert np.abs(x - np.round(x)).max() <= 2.0 ** -40
        return np.round(x) + 0.0
    if mutation == 'head_padding_weight':
        x = x.copy()
        x[:, 48 + 24 * (nb - 1):] *= 2
    return x


def _bf16(x):
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def head_colours_fast(inp, dz=0, dr=0, dx=0, dy=0):
    """view_ray + project_taps_fast + blend4 in fp32 for the head set: colours [n, nb, 8, 3], with z3d = rcp(1 - dn - eps) moved by dz
    ulp, the reciprocal of p.z by dr ulp and the resulting X, Y by dx, dy ulp.  A = M (o, 1) is exact here, and so is
    B0 = M[0][2] e_z (a power of two times e_z); B1 = B2 = 0."""
    from exact_composite import fma32
    f32 = np.float32
    step = lambda x, d: x if d == 0 else np.nextafter(x, f32(np.inf if d > 0 else -np.inf)).astype(f32)
    img, proj, orr = inp['img'], inp['proj'].astype(np.float64), inp['or_rays'].astype(np.float64)
    Hf, Wf = img.shape[2:]
    assert not orr[:, 3:5].any() and not proj[:, 1, 2].any() and not proj[:, 2, :3].any()
    A = np.einsum('krc,nc->nkr', proj[:, :, :3], orr[:, 0:3]) + proj[None, :, :, 3]
    B0 = orr[:, 5, None] * proj[None, :, 0, 2]
    assert np.array_equal(A, A.astype(f32)) and np.abs(A).max() < 2 ** 12 and np.array_equal(B0, B0.astype(f32))
    A, B0 = A.astype(f32), B0.astype(f32)
    den = ((f32(1) - inp['depth'].astype(f32)).astype(f32) - f32(inp['eps'])).astype(f32)
    z3d = step((f32(1) / den).astype(f32), dz)[:, None, :]                                        # [n, 1, 8]
    r = step((f32(1) / A[..., 2]).astype(f32), dr)[:, :, None]                                      # [n, nb, 1]
    X = step((fma32(z3d, B0[:, :, None], A[:, :, None, 0]) * r).astype(f32), dx)
    Y = np.broadcast_to(step((A[:, :, None, 1] * r).astype(f32), dy), X.shape)
    fx, fy = np.floor(X), np.floor(Y)
    wx1, wy1 = (X - fx).astype(f32), (Y - fy).astype(f32)
    wx0, wy0 = (f32(1) - wx1).astype(f32), (f32(1) - wy1).astype(f32)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    view = np.arange(img.shape[0])[None, :, None]
    out = []
    for c in range(3):
        acc = None
        for ddy, ddx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
            xx, yy = x0 + ddx, y0 + ddy
            ok = (xx >= 0) & (xx < Wf) & (yy >= 0) & (yy < Hf)
            t = img[view, c, np.clip(yy, 0, Hf - 1), np.clip(xx, 0, Wf - 1)]
            term = (t * np.where(ok, (wx * wy).astype(f32), f32(0))).astype(f32)
            acc = term if acc is None else (acc + term).astype(f32)
        out.append(acc)
    return np.stack(out, -1)


def head_certificate(inp):
    """Every colour of the head set, after rounding to the operand type (fp16; bf16), is the reference's integer whichever way both
    v_rcp_f32 results (of 1 - dn - eps and of p.z) and both coordinates are off by one ulp: the nominal values and the 16 corners
    (a coordinate is monotone in each of the four, and the safe set of a coordinate is an interval).  Returns the colours [n, nb, 8, 3]."""
    nb = inp['proj'].shape[0]
    want = head_refine_in(inp)[:, 48:].reshape(-1, nb, 8, 3)
    assert want.min() >= 0 and want.max() <= 2
    want = want.astype(np.float32)
    combos = [(0, 0, 0, 0)] + [(a, b, c, d) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1) for d in (-1, 1)]
    for combo in combos:
        c = head_colours_fast(inp, *combo)
        assert np.array_equal(c.astype(np.float16).astype(np.float32), want), ('fp16', combo)
        assert np.array_equal(_bf16(c), want), ('bf16', combo)
    return want
