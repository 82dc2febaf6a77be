"""Compositing inputs with exact answers, per-element error bounds and slipped kernel emulations (a plain helper module of the suite).

The per-ray kernels between the MLPs — ``composite_kernel`` / ``composite_thread_kernel`` (pnrf_ops.hip, raw2outputs forward) and
``composite_bwd_kernel`` (pnrf_train.hip, its backward for d rgb_map) — each claim a fixed order of fp32 operations.  This module holds:

  * ``replay``: the kernels' formulas in the kernels' order (the forward's ascending sums, the backward's chunked descending pass with
    ``t_start``, the carried ``Q``, the ``ds_bpermute`` / ``dd_next`` neighbour of ``d_z``), written once over an arithmetic back end:
      - ``F32``: numpy float32, one IEEE rounding per operation — the kernels as a CPU emulation;
      - ``Cert``: float64 with a certificate: every product and sum is checked to be unchanged by rounding to fp32 (products of two
        fp32 values are exact in float64; sums are checked with Knuth's TwoSum), every exp / sigmoid argument is 0 or >= 200 in
        magnitude (so expf returns exactly 1 or 0, sigmoid exactly 0.5, 1 or 0), and ``1 - alpha + 1e-10`` rounds back to ``1 - alpha``
        (or gives 1e-10 itself when alpha = 1).  A value that fails is tainted; a tainted value may only meet an exact 0 in a product
        (x * 0 = 0 for finite x, fused or not).  When no output is tainted every intermediate is the exact real value, so fused
        multiply-adds (``composite_bwd_kernel`` is compiled with contraction on) and the order of the sums cannot change any bit, and the
        replay cast to float32 is the answer the kernels must produce.  The two divisions of ``disp`` are single IEEE divisions of exact
        values (``ieee_div``, contraction off): their correctly rounded result is computed, with the double-rounding case excluded;
      - ``Mag``: float64 values with a running magnitude (see ``BOUND_DOC``), for the per-element bound of the general regime.
  * ``exact_inputs`` / ``random_inputs``: the two regimes' input sets; ``reference``: the oracle's raw2outputs in float64 plus autograd.
  * ``MUTATIONS``: one slip each, applied by ``replay(..., mutation=...)``.

The back ends also carry the operations of the head and positional-encoding kernels (scale, tanh, sin, cos, abs, sign): tests/exact_heads.py,
and those of the projection and texel-fetch kernels (floor, fma, comparisons, texel): tests/exact_project.py.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import pronerf_oracle as orc

U = 2.0 ** -24                       # unit roundoff of fp32
TINY = float(np.float32(1e-10))      # the 1e-10f of 1 - alpha + 1e-10
BIG = float(np.float32(1e10))        # the last interval (1e10f = 9765625 * 2^10: exact in fp32)
CLAMP = 10.0
G = 4096.0                           # exact regime: the length of a non-empty interval
CAP = 4                              # exact regime: at most this many samples with alpha != 0 per ray

# ---- what tests/test_exact_composite_gpu.py runs (tests/test_exact_composite_cpu.py certifies the same exact sets)
S_BWD = (1, 2, 3, 7, 8, 9, 63, 64, 65, 72, 127, 128, 129, 136, 200, 248, 255, 256)
NS = (1, 3, 4, 5, 257)
# option sets: (add/mul, noise, clamp, white_bkgd)
OPTS = ((False, False, 0.0, False), (True, True, CLAMP, False), (True, False, 0.0, True), (False, True, CLAMP, True))
S_THREAD = (1, 2, 3, 5, 8, 64, 65, 72, 129, 256)
N_THREAD = 65536 + 37                # >= 65 536 rays: pnrf_composite_fwd takes composite_thread_kernel


def exact_case(S, oi):
    """The exact-regime input set of the GPU matrix for S and option set OPTS[oi]: 257 rays, run whole and as its first 1, 3, 4, 5 rays."""
    return exact_inputs(max(NS), S, *OPTS[oi], seed=100 * S + oi)


def random_case(S, oi):
    """The general-regime input set of the GPU matrix for S and OPTS[oi]."""
    return random_inputs(max(NS), S, *OPTS[oi], seed=100 * S + oi + 50)


def head(inp, n):
    """The first n rays of an input set."""
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def tile(inp, n):
    """An input set (or a set of outputs) of n rays that repeats the rays of inp (the thread-per-ray kernel's exact inputs)."""
    idx = np.arange(n) % next(v for v in inp.values() if isinstance(v, np.ndarray)).shape[0]
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


# ------------------------------------------------------------------------------------------------ arithmetic back ends
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def fma32(a, b, c):
    """fl32(a b + c) with one rounding, on float32 arrays: the product of two fp32 values is exact in float64; the float64 sum is
    corrected to round-to-odd with TwoSum's error term, so that the final rounding to fp32 sees the exact sum's sticky bit."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


class F32:
    """numpy float32: one IEEE rounding per operation (what the kernels' ieee_* helpers do)."""
    def inp(self, x): return np.asarray(x, np.float32)
    def const(self, c, like): return np.full(np.shape(like), c, np.float32)
    def add(self, a, b): return np.float32(a) + np.float32(b)
    def sub(self, a, b): return np.float32(a) - np.float32(b)
    def mul(self, a, b): return np.float32(a) * np.float32(b)
    def div(self, a, b): return np.float32(a) / np.float32(b)
    def neg(self, a): return -a
    def sqrt(self, a): return np.sqrt(a)
    def relu(self, a): return np.maximum(a, np.float32(0))
    def clamp(self, a, c): return np.minimum(np.maximum(a, np.float32(-c)), np.float32(c))
    def expneg(self, x): return np.exp(-x)
    def sigmoid(self, r): return np.float32(1) / (np.float32(1) + np.exp(-r))
    def add_tiny(self, a): return a + np.float32(TINY)
    def max_nan(self, c, a): return np.where(np.isnan(a), a, np.maximum(np.float32(c), a))       # torch.max: NaN propagates
    def where(self, c, a, b): return np.where(c, a, b).astype(np.float32)
    def cond(self, a): return a
    # ---- what tests/exact_heads.py adds (the heads' and the positional encoding's operations)
    def scale(self, a, p): return np.float32(a) * np.float32(p)                                  # p a power of two: exact
    def tanh(self, a): return np.tanh(np.float32(a))
    def sin(self, a): return np.sin(np.float32(a))
    def cos(self, a): return np.cos(np.float32(a))
    def abs(self, a): return np.abs(a)
    def sign(self, a): return np.sign(a).astype(np.float32)                                      # +1 / -1 / 0 (NaN passes)
    # ---- what tests/exact_project.py adds (projection and texel fetch): floor, a fused multiply-add, comparisons, a constant absorbed
    def val(self, a): return np.asarray(a)                                                       # the plain values (indices, branches)
    def floor(self, a): return np.floor(np.float32(a))
    def rint(self, a): return np.rint(np.float32(a))
    def fma(self, a, b, c): return fma32(a, b, c)
    def add_const(self, a, c): return np.float32(a) + np.float32(c)                              # |c2.z| + 1e-8f
    def round_add(self, a, c): return np.float32(a) + np.float32(c)                              # cnt + 1e-6f
    def le(self, a, b): return np.float32(a) <= np.float32(b)
    def lt(self, a, b): return np.float32(a) < np.float32(b)
    def ge(self, a, b): return np.float32(a) >= np.float32(b)
    def gt(self, a, b): return np.float32(a) > np.float32(b)
    def texel(self, v, cell_taint, cell_mag): return np.asarray(v, np.float32)


class V:
    """A Cert / Mag value: float64 value v and, per element, a taint flag (Cert) or a magnitude (Mag)."""
    __slots__ = ('v', 't')

    def __init__(self, v, t):
        self.v, self.t = np.asarray(v, np.float64), t


class Cert:
    """float64 with exactness checks (module docstring).  ``t`` is the taint mask; ``why`` counts the reasons of taint."""
    def __init__(self):
        self.why = {}

    def _taint(self, what, mask):
        k = int(np.count_nonzero(mask))
        if k:
            self.why[what] = self.why.get(what, 0) + k
        return mask

    def inp(self, x):
        x = np.asarray(x, np.float32).astype(np.float64)
        return V(x, np.zeros(x.shape, bool))

    def const(self, c, like):
        return V(np.full(np.shape(like.v), float(np.float32(c))), np.zeros(np.shape(like.v), bool))

    def _round(self, what, exact, t):
        r = f32(exact)
        bad = (r != exact) | ~np.isfinite(r)
        return V(r, t | self._taint(what, bad & ~t))

    def add(self, a, b, what='add'):
        s = a.v + b.v
        bb = s - a.v
        err = (a.v - (s - bb)) + (b.v - bb)                     # TwoSum: s + err == a + b exactly
        t = a.t | b.t | self._taint(what + ' (float64)', (err != 0) & ~(a.t | b.t))
        return self._round(what, s, t)

    def sub(self, a, b, what='sub'):
        return self.add(a, V(-b.v, b.t), what)

    def mul(self, a, b, what='mul'):
        p = a.v * b.v                                            # exact: two fp32 significands fit in 53 bits
        zero = ((a.v == 0) & ~a.t & np.isfinite(b.v)) | ((b.v == 0) & ~b.t & np.isfinite(a.v))
        r = self._round(what, p, a.t | b.t)
        r.t = r.t & ~zero
        r.v = np.where(zero, 0.0 * p, r.v)
        return r

    def div(self, a, b):
        with np.errstate(divide='ignore', invalid='ignore'):
            q = a.v / b.v
        r = f32(q)
        # double rounding (to float64, then fp32) is harmless unless q lands on an fp32 midpoint
        lo = np.nextafter(r.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
        hi = np.nextafter(r.astype(np.float32), np.float32(np.inf)).astype(np.float64)
        mid = np.isfinite(q) & ((q == (r + lo) / 2) | (q == (r + hi) / 2))
        return V(r, a.t | b.t | self._taint('division on a midpoint', mid))

    def neg(self, a): return V(-a.v, a.t)

    def sqrt(self, a):
        r = f32(np.sqrt(a.v))
        return V(r, a.t | self._taint('sqrt', (r * r != a.v) & ~a.t))

    def relu(self, a): return V(np.maximum(a.v, 0.0), a.t)

    def clamp(self, a, c): return V(np.clip(a.v, -c, c), a.t)

    def expneg(self, x):
        """expf(-x) for x >= 0: exactly 1 at x == 0 and exactly 0 from x >= 200 on (a tainted x must clear 200 with room)."""
        one = (x.v == 0) & ~x.t
        zero = x.v >= np.where(x.t, 200.0 * (1 + 2.0 ** -10), 200.0)
        bad = ~(one | zero)
        self._taint('exp argument neither 0 nor >= 200', bad)
        return V(np.where(one, 1.0, np.where(zero, 0.0, np.exp(-x.v))), bad)

    def sigmoid(self, r):
        one, zero, half = (r.v >= 200) & ~r.t, (r.v <= -200) & ~r.t, (r.v == 0) & ~r.t
        bad = ~(one | zero | half)
        self._taint('sigmoid argument neither 0 nor |.| >= 200', bad)
        return V(np.where(one, 1.0, np.where(zero, 0.0, np.where(half, 0.5, 1.0 / (1.0 + np.exp(-r.v))))), bad)

    def add_tiny(self, a):
        """1 - alpha + 1e-10f: must round back to 1 - alpha (or be 1e-10f itself at alpha = 1)."""
        s = f32(a.v + TINY)
        ok = ((s == a.v) & (a.v != 0)) | (a.v == 0)
        return V(np.where(a.v == 0, TINY, a.v), a.t | self._taint('1 - alpha + 1e-10 not absorbed', ~ok & ~a.t))

    def max_nan(self, c, a):
        return V(np.where(np.isnan(a.v), a.v, np.maximum(float(np.float32(c)), a.v)), a.t)

    def where(self, c, a, b):
        return V(np.where(c, a.v, b.v), np.where(c, a.t, b.t))

    def cond(self, a):
        assert not np.any(a.t), 'a branch depends on a tainted value'
        return a.v

    # ---- what tests/exact_heads.py adds
    def scale(self, a, p):
        """a * p for a power of two p (one rounding, checked like any product)."""
        return self._round('scale', a.v * float(p), a.t)

    def tanh(self, a):
        """tanhf: exactly +-1 from |a| >= 200 on and exactly 0 at 0; anything else taints."""
        one, mone, zero = (a.v >= 200) & ~a.t, (a.v <= -200) & ~a.t, (a.v == 0) & ~a.t
        bad = ~(one | mone | zero)
        self._taint('tanh argument neither 0 nor |.| >= 200', bad)
        return V(np.where(one, 1.0, np.where(mone, -1.0, np.where(zero, 0.0, np.tanh(a.v)))), bad)

    def sin(self, a):
        bad = ~((a.v == 0) & ~a.t)
        self._taint('sin argument not 0', bad)
        return V(np.where(bad, np.sin(a.v), 0.0), bad)

    def cos(self, a):
        bad = ~((a.v == 0) & ~a.t)
        self._taint('cos argument not 0', bad)
        return V(np.where(bad, np.cos(a.v), 1.0), bad)

    def abs(self, a): return V(np.abs(a.v), a.t)
    def sign(self, a): return V(np.sign(a.v), a.t)               # the sign of an exact value; a tainted one taints what it decides

    # ---- what tests/exact_project.py adds
    def val(self, a): return a.v
    def floor(self, a): return V(np.floor(a.v), a.t)
    def rint(self, a): return V(np.rint(a.v), a.t)
    def fma(self, a, b, c): return self.add(self.mul(a, b), c, 'fma')       # product and sum both exact: fused or not, the same bits

    def add_const(self, a, c):
        """a + c for a constant c far below ulp(a): must round back to a (the one rounding the training projection is allowed)."""
        s = f32(a.v + float(np.float32(c)))
        return V(a.v, a.t | self._taint('constant not absorbed', (s != a.v) & ~a.t))

    def round_add(self, a, c):
        """fl32(a + c) of an exact a and a constant: one IEEE addition that no product feeds (nothing to fuse, no order to change) — the
        rounded sum is the value the kernel holds, and counts as exact from here on (the mean fill's cnt + 1e-6f)."""
        return V(f32(a.v + float(np.float32(c))), a.t)

    def _cmp(self, a, b):
        self._taint('comparison of an inexact value', (a.t | b.t) & np.isfinite(a.v) & np.isfinite(b.v))

    def le(self, a, b): self._cmp(a, b); return a.v <= b.v
    def lt(self, a, b): self._cmp(a, b); return a.v < b.v
    def ge(self, a, b): self._cmp(a, b); return a.v >= b.v
    def gt(self, a, b): self._cmp(a, b); return a.v > b.v

    def texel(self, v, cell_taint, cell_mag):
        """A fetched texel: exact, unless the cell it was fetched from was chosen by an inexact coordinate."""
        return V(np.asarray(v, np.float64), np.broadcast_to(cell_taint, np.shape(v)).copy())


BOUND_DOC = """Per-element bound of the general regime:  |got - ref| <= 2 (S + 9) 2^-24 mag (1 + 2^-10) + (S + 9) 2^-126.

``mag`` comes from ``Mag``: the kernels' recurrences in float64 with, next to each value v, a magnitude m such that |fl(v) - v| <= d u m
when d is the largest number of roundings on any path to v (first order in u = 2^-24).  Inputs: m = |v|.  Sums and differences:
m = m_a + m_b (the absolute-value recurrence: covers the cancellation of d_z = ddist_s - ddist_{s+1} and of 1 - exp).  Products:
m = m_a |b| + |a| m_b (first order; m_a m_b would grow like 2^S along the transmittance product).  expf(-x): m = e (1 + m_x) — its
argument's error times e, plus expf's own error, which counts as E roundings: the ROCm device library documents no ulp bound for expf,
so this ASSUMES <= 2 ulp, i.e. 2^-23 relative per ulp: E = 4.  sigmoid(r) of an input r: m = sigmoid(r) (E + 2 roundings).  Division:
m = (m_a + |q| m_b) / |b|.  sqrt: m = m_a / (2 sqrt a).  relu / clamp / max: m passes (they do not increase an error).

Counting roundings (E = 4): dn = sqrt of three squares summed: 3.  sigma = raw + noise + add: 2.  dist = (z' - z) dn: 4.  relu(sigma)
dist: 5.  exp: 5 + E.  a = 1 - exp: 6 + E.  alpha = a relu(mul): 7 + E.  x = 1 - alpha + 1e-10: 9 + E.  T_s = x_0 ... x_{s-1}:
s + 9 + E.  Forward: w_s = alpha T_s, w c, then the running sum — the term of sample s passes S - s additions: S + 11 + E; white
background 2 more, disp 2 more: at most S + 13 + E = S + 17.  Backward: sigmoid E + 2, g c E + 3, dws E + 6 (gsum 2), dws alpha E + 8;
Q_{s-1} = dws alpha + x Q costs two roundings per sample (a product and a sum, fused or not): Q_s <= 2 (S - s) + E + 7; dal = T (dws -
Q) <= 2 S + E + 9; da 2 S + E + 10; ddist = da ee ex dn 2 S + E + 13; d_z = ddist - ddist' 2 S + E + 14 = 2 (S + 9); d_raw colours,
dsg, d_mul below that.  So d <= c (S + k) with c = 2, k = 9 for every output.  The float64 reference's own error (about d 2^-53 mag) and
the second-order terms ((d u)^2 < 2^-28 at S = 256) fit in the factor 1 + 2^-10.  The absolute term covers subnormal results (expf
below 2^-126, products of tiny transmittances), where a relative error bound does not hold."""


class Mag:
    """float64 values with running magnitudes (BOUND_DOC)."""
    def __init__(self, exp_rounds=4, absorb=False):
        self.E = exp_rounds
        self.absorb = absorb            # add_const rounds its sum to fp32 (exact_project's exact sets: the certified absorption of 1e-8f)

    def inp(self, x):
        x = np.asarray(x, np.float32).astype(np.float64)
        return V(x, np.abs(x))

    def const(self, c, like): return V(np.full(np.shape(like.v), float(np.float32(c))), np.full(np.shape(like.v), abs(float(np.float32(c)))))
    def add(self, a, b): return V(a.v + b.v, a.t + b.t)
    def sub(self, a, b): return V(a.v - b.v, a.t + b.t)
    def mul(self, a, b): return V(a.v * b.v, a.t * np.abs(b.v) + np.abs(a.v) * b.t)

    def div(self, a, b):
        with np.errstate(divide='ignore', invalid='ignore'):
            q = a.v / b.v
            return V(q, (a.t + np.abs(q) * b.t) / np.abs(b.v))

    def neg(self, a): return V(-a.v, a.t)

    def sqrt(self, a):
        r = np.sqrt(a.v)
        with np.errstate(divide='ignore', invalid='ignore'):
            return V(r, np.where(r > 0, a.t / (2 * r), 0.0))

    def relu(self, a): return V(np.maximum(a.v, 0.0), a.t)
    def clamp(self, a, c): return V(np.clip(a.v, -c, c), a.t)

    def expneg(self, x):
        e = np.exp(-x.v)
        return V(e, e * (1.0 + x.t))

    def sigmoid(self, r):
        s = 1.0 / (1.0 + np.exp(-r.v))
        return V(s, s)

    def add_tiny(self, a): return V(a.v + TINY, a.t + TINY)
    def max_nan(self, c, a): return V(np.where(np.isnan(a.v), a.v, np.maximum(float(np.float32(c)), a.v)), a.t)
    def where(self, c, a, b): return V(np.where(c, a.v, b.v), np.where(c, a.t, b.t))
    def cond(self, a): return a.v
    # ---- what tests/exact_heads.py adds.  tanh / sin / cos of an argument that carries no error (an input, or an input times 2^k):
    # m = |result|; the function's own error counts as roundings in the bound's d (exact_heads.BOUND_DOC), as sigmoid's does above.
    def scale(self, a, p): return V(a.v * float(p), a.t * abs(float(p)))
    def tanh(self, a): return V(np.tanh(a.v), np.abs(np.tanh(a.v)))
    def sin(self, a): return V(np.sin(a.v), np.abs(np.sin(a.v)))
    def cos(self, a): return V(np.cos(a.v), np.abs(np.cos(a.v)))
    def abs(self, a): return V(np.abs(a.v), a.t)
    def sign(self, a): return V(np.sign(a.v), np.abs(np.sign(a.v)))    # decided alike in both precisions (the input sets see to that)
    # ---- what tests/exact_project.py adds.  floor: the integer carries no error of its own — a coordinate within rounding of an integer
    # may fall into the neighbouring cell in fp32, where bilinear interpolation continues the same function; texel() therefore takes
    # the largest |texel| of the cell's 4x4 neighbourhood as the magnitude of each of its taps.  Comparisons: decided on the values.
    def val(self, a): return a.v
    def floor(self, a): return V(np.floor(a.v), np.zeros(np.shape(a.v)))
    def rint(self, a): return V(np.rint(a.v), np.zeros(np.shape(a.v)))
    def fma(self, a, b, c): return self.add(self.mul(a, b), c)        # counted as its two unfused operations
    def add_const(self, a, c):
        s = a.v + float(np.float32(c))
        return V(f32(s) if self.absorb else s, a.t + abs(float(np.float32(c))))

    def round_add(self, a, c): return V(a.v + float(np.float32(c)), a.t + abs(float(np.float32(c))))
    def le(self, a, b): return a.v <= b.v
    def lt(self, a, b): return a.v < b.v
    def ge(self, a, b): return a.v >= b.v
    def gt(self, a, b): return a.v > b.v
    def texel(self, v, cell_taint, cell_mag): return V(np.asarray(v, np.float64), np.broadcast_to(cell_mag, np.shape(v)).astype(np.float64))


def bound(S, mag):
    """The general regime's per-element bound (BOUND_DOC)."""
    return 2 * (S + 9) * U * mag * (1 + 2.0 ** -10) + (S + 9) * 2.0 ** -126


# ------------------------------------------------------------------------------------------------ the kernels' formulas
MUTATIONS = (
    't_restart',          # composite_bwd_kernel: the transmittance restarts at 1 at a chunk start (t_start dropped)
    'q_reset',            # composite_bwd_kernel: Q not carried across chunks
    'dd_next_dropped',    # composite_bwd_kernel: lane 63's neighbour (dd_next, the next chunk's first ddist) read as 0
    'partial_stale',      # partial chunk: its last lane reads the clamped (stale) sample c0 instead of its own (on = lane < m - 1)
    'clamp_exclusive',    # composite_bwd_kernel: clamp gradient passes only for |raw| < clamp
    'relu_sigma_at_0',    # composite_bwd_kernel: d sigma passes at sigma == 0
    'relu_mul_at_0',      # composite_bwd_kernel: d mul passes at mul == 0
    'last_interval_z',    # both: the last interval taken from z (z_next - z, with the 0 an off lane loads) instead of 1e10
    'd_stride',           # both: directions of a [n, 3] tensor read with a row stride of 11
)


def _dirs(d, mutation):
    if mutation != 'd_stride':
        return d
    flat = np.concatenate([d.reshape(-1), np.zeros(11 * d.shape[0], np.float32)])
    return np.stack([flat[np.arange(d.shape[0]) * 11 + k] for k in range(3)], 1)


def replay(A, inp, mutation=None):
    """Both kernels' formulas in their order over back end A.  inp: dict of float32 arrays raw [n,S,4], z [n,S], d [n,3], g [n,3],
    add / mul / noise [n,S] or None, clamp, white.  Returns (forward, backward): rgb [n,3], disp, acc, w [n,S], depth; d_raw [n,S,4],
    d_z, d_add, d_mul (None without add / mul) — as back-end values."""
    raw, z, add, mul, noise = inp['raw'], inp['z'], inp['add'], inp['mul'], inp['noise']
    clampv, white = float(inp['clamp']), bool(inp['white'])
    n, S = z.shape
    d = _dirs(inp['d'], mutation)
    M = mutation

    def col(x, s):
        return A.inp(x[:, s])

    dx, dy, dz = A.inp(d[:, 0]), A.inp(d[:, 1]), A.inp(d[:, 2])
    dn = A.sqrt(A.add(A.add(A.mul(dx, dx), A.mul(dy, dy)), A.mul(dz, dz)))
    zero = A.const(0.0, dn)
    one = A.const(1.0, dn)

    # the per-sample quantities of both passes (load(): the same operations in the forward and the backward kernels)
    def sample(s, src=None):
        k = s if src is None else src
        r = [A.inp(raw[:, k, c]) for c in range(4)]
        rc = [A.clamp(x, clampv) for x in r] if clampv > 0 else list(r)
        sg = rc[3]
        if noise is not None:
            sg = A.add(sg, col(noise, k))
        if add is not None:
            sg = A.add(sg, col(add, k))
        zc = col(z, k)
        if s + 1 < S:
            dist = A.mul(A.sub(col(z, k + 1), zc), dn)
        elif M == 'last_interval_z':
            dist = A.mul(A.sub(zero, zc), dn)
        else:
            dist = A.mul(A.const(BIG, dn), dn)
        ee = A.relu(sg)
        a = A.sub(one, A.expneg(A.mul(ee, dist)))
        ml = col(mul, k) if mul is not None else None
        al = A.mul(a, A.relu(ml)) if mul is not None else a
        x = A.add_tiny(A.sub(one, al))
        return dict(r=r, rc=rc, sg=sg, zc=zc, dist=dist, ee=ee, a=a, ml=ml, al=al, x=x)

    def src_of(s):
        """partial_stale: the last lane of a partial chunk reads the chunk's first sample."""
        c0 = (s // 64) * 64
        m = min(S - c0, 64)
        return c0 if (M == 'partial_stale' and m < 64 and s == c0 + m - 1) else None

    smp = [sample(s, src_of(s)) for s in range(S)]

    # ---- forward (composite_kernel / composite_thread_kernel)
    T = one
    s0 = s1 = s2 = sd = sa = zero
    w_f = []
    for s in range(S):
        q = smp[s]
        w = A.mul(q['al'], T)
        T = A.mul(T, q['x'])
        cs = [A.sigmoid(q['rc'][c]) for c in range(3)]
        s0 = A.add(s0, A.mul(w, cs[0])); s1 = A.add(s1, A.mul(w, cs[1])); s2 = A.add(s2, A.mul(w, cs[2]))
        sd = A.add(sd, A.mul(w, q['zc'])); sa = A.add(sa, w)
        w_f.append(w)
    if white:
        bg = A.sub(one, sa)
        s0, s1, s2 = A.add(s0, bg), A.add(s1, bg), A.add(s2, bg)
    disp = A.div(one, A.max_nan(1e-10, A.div(sd, sa)))
    fwd = dict(rgb=[s0, s1, s2], disp=disp, acc=sa, w=w_f, depth=sd)

    # ---- backward (composite_bwd_kernel): chunks from the last to the first
    g = [A.inp(inp['g'][:, c]) for c in range(3)]
    gsum = A.add(A.add(g[0], g[1]), g[2]) if white else zero
    nch = (S + 63) // 64
    T_before = [one]                                            # t_start(c): the product over the chunks before c, in sample order
    for c in range(1, nch):
        Tc = T_before[-1]
        for s in range(64 * (c - 1), 64 * c):
            Tc = A.mul(Tc, smp[s]['x'])
        T_before.append(Tc)
    d_raw = [[None] * 4 for _ in range(S)]
    d_z, d_add, d_mul = [None] * S, [None] * S, [None] * S
    Q, dd_next = zero, zero
    for c in range(nch - 1, -1, -1):
        c0, m = 64 * c, min(S - 64 * c, 64)
        Tr = one if M == 't_restart' else T_before[c]
        if M == 'q_reset':
            Q = zero
        Tpre, dws, Ql, ddist = {}, {}, {}, {}
        for j in range(m):
            Tpre[j] = Tr
            Tr = A.mul(Tr, smp[c0 + j]['x'])
        for j in range(m):
            q = smp[c0 + j]
            cs = [A.sigmoid(q['rc'][k]) for k in range(3)]
            q['cs'] = cs
            dws[j] = A.sub(A.add(A.add(A.mul(g[0], cs[0]), A.mul(g[1], cs[1])), A.mul(g[2], cs[2])), gsum)
        for j in range(m - 1, -1, -1):
            Ql[j] = Q
            Q = A.add(A.mul(dws[j], smp[c0 + j]['al']), A.mul(smp[c0 + j]['x'], Q))
        for j in range(m):
            s, q = c0 + j, smp[c0 + j]
            dal = A.mul(Tpre[j], A.sub(dws[j], Ql[j]))
            w = A.mul(q['al'], Tpre[j])
            ex = A.expneg(A.mul(q['ee'], q['dist']))
            da = A.mul(dal, A.relu(q['ml'])) if mul is not None else dal
            sgv = A.cond(q['sg'])
            pos = sgv >= 0 if M == 'relu_sigma_at_0' else sgv > 0
            dsg = A.where(pos, A.mul(A.mul(da, q['dist']), ex), zero)
            has_next = s + 1 < S or M == 'last_interval_z'
            ddist[j] = A.mul(A.mul(A.mul(da, q['ee']), ex), dn) if has_next else zero
            for k in range(3):
                rk = A.cond(q['r'][k])
                inside = np.ones(n, bool) if clampv <= 0 else ((np.abs(rk) < clampv) if M == 'clamp_exclusive' else (np.abs(rk) <= clampv))
                ck = q['cs'][k]
                d_raw[s][k] = A.where(inside, A.mul(A.mul(A.mul(g[k], w), ck), A.sub(one, ck)), zero)
            r3 = A.cond(q['r'][3])
            in3 = np.ones(n, bool) if clampv <= 0 else ((np.abs(r3) < clampv) if M == 'clamp_exclusive' else (np.abs(r3) <= clampv))
            d_raw[s][3] = A.where(in3, dsg, zero)
            if mul is not None:
                mlv = A.cond(q['ml'])
                d_mul[s] = A.where(mlv >= 0 if M == 'relu_mul_at_0' else mlv > 0, A.mul(dal, q['a']), zero)
                d_add[s] = dsg
            q['dal'] = dal
        for j in range(m):
            s = c0 + j
            if j + 1 < m:
                up = ddist[j + 1]
            else:
                up = zero if M == 'dd_next_dropped' else dd_next
            if s + 1 < S:
                d_z[s + 1] = A.sub(ddist[j], up)
            if s == 0:
                d_z[0] = A.neg(ddist[j])
        dd_next = ddist[0]
    bwd = dict(d_raw=d_raw, d_z=d_z, d_add=d_add if mul is not None else None, d_mul=d_mul if mul is not None else None)
    return fwd, bwd


def collect(A, fwd, bwd, get):
    """Back-end values -> float64 arrays in the ops' shapes; get(V) picks .v or .t (F32: the arrays themselves)."""
    out = dict(rgb=np.stack([get(x) for x in fwd['rgb']], 1), disp=get(fwd['disp']), acc=get(fwd['acc']),
               w=np.stack([get(x) for x in fwd['w']], 1), depth=get(fwd['depth']),
               d_raw=np.stack([np.stack([get(x) for x in row], 1) for row in bwd['d_raw']], 1),
               d_z=np.stack([get(x) for x in bwd['d_z']], 1))
    if bwd['d_add'] is not None:
        out['d_add'] = np.stack([get(x) for x in bwd['d_add']], 1)
        out['d_mul'] = np.stack([get(x) for x in bwd['d_mul']], 1)
    return out


FWD_KEYS = ('rgb', 'disp', 'acc', 'w', 'depth')


def emulate(inp, mutation=None):
    """float32 CPU emulation of both kernels (F32 back end)."""
    A = F32()
    with np.errstate(all='ignore'):
        f, b = replay(A, inp, mutation)
        return {k: np.asarray(v, np.float32) for k, v in collect(A, f, b, lambda x: np.asarray(x, np.float64)).items()}


def certify(inp):
    """The exact regime's certificate: returns the expected float32 outputs, or raises with the reasons of taint."""
    A = Cert()
    with np.errstate(all='ignore'):
        f, b = replay(A, inp)
        val = collect(A, f, b, lambda x: x.v)
        bad = collect(A, f, b, lambda x: x.t)
    for k in val:
        if k == 'disp':
            continue                                             # one or two IEEE divisions of exact values: checked separately below
        assert not bad[k].any(), f'{k}: {int(bad[k].sum())} inexact elements ({A.why})'
    assert not bad['disp'].any(), f'disp: a division lands on a midpoint ({A.why})'
    assert all(np.isfinite(v).all() or k == 'disp' for k, v in val.items())
    return {k: v.astype(np.float32) for k, v in val.items()}


def magnitudes(inp):
    """General regime: (float64 values of the replay, magnitudes) of every output."""
    A = Mag()
    with np.errstate(all='ignore'):
        f, b = replay(A, inp)
        return collect(A, f, b, lambda x: x.v), collect(A, f, b, lambda x: x.t)


def reference(inp):
    """The oracle's raw2outputs in float64 and its autograd for d rgb_map = g: the outputs in the ops' order and shapes.

    At S = 1 the oracle's ``dists[..., :1]`` of the empty difference tensor is empty too, so it composites nothing (acc = 0); the
    kernels give the single sample the 1e10 interval, as they give every ray's last sample.  The reference at S = 1 is the oracle on a
    padded ray: a second sample 1e10 behind the first (so the first interval is 1e10 again) that contributes nothing (sigma and mul
    0, colour raw 0); its outputs are dropped, and d z_0 is 0 (the kernels' last interval does not depend on z)."""
    if inp['z'].shape[1] == 1:
        pad = lambda x, v: None if x is None else np.concatenate([x, np.full_like(x[:, :1], v)], 1)
        z2 = np.concatenate([inp['z'].astype(np.float64), inp['z'].astype(np.float64) + 1e10], 1)
        p = dict(inp, raw=pad(inp['raw'], 0), z=z2, add=pad(inp['add'], 0), mul=pad(inp['mul'], 0), noise=pad(inp['noise'], 0))
        p['raw'][:, 1, 3] = -1.0 if not p['clamp'] else -p['clamp']
        out = reference(p)
        out = {k: (v[:, :1] if v.ndim >= 2 and k != 'rgb' else v) for k, v in out.items()}
        out['d_z'] = np.zeros_like(out['d_z'])
        return out
    t = lambda x, rg=False: None if x is None else torch.tensor(np.asarray(x, np.float64), requires_grad=rg)
    raw, z, add, mul = t(inp['raw'], True), t(inp['z'], True), t(inp['add'], True), t(inp['mul'], True)
    rgb, disp, acc, w, depth = orc.raw2outputs(raw, z, t(inp['d']), add, mul, noise=t(inp['noise']), clamp=float(inp['clamp']),
                                               white_bkgd=bool(inp['white']))
    rgb.backward(t(inp['g']))
    out = dict(rgb=rgb, disp=disp, acc=acc, w=w, depth=depth, d_raw=raw.grad, d_z=z.grad)
    if add is not None:
        out['d_add'], out['d_mul'] = add.grad, mul.grad
    return {k: v.detach().numpy() for k, v in out.items()}


def check_bound(got, ref, mag, S, keys):
    """Per-element |got - ref| <= bound; returns the list of (key, worst ratio) that fail (empty: all pass)."""
    bad = []
    for k in keys:
        if k not in ref:
            continue
        g = np.asarray(got[k], np.float64)
        both = np.isnan(g) & np.isnan(ref[k])                   # disp of a ray with acc = 0: NaN in the oracle, NaN required
        with np.errstate(invalid='ignore'):
            r = np.where(both, 0.0, np.abs(g - ref[k]) / bound(S, mag[k]))
        r = np.where(np.isnan(r), np.inf, r)
        if r.size and r.max() > 1:
            bad.append((k, float(r.max())))
    return bad


# ------------------------------------------------------------------------------------------------ input sets
def _boundaries(S):
    """Samples next to every chunk boundary (63 / 64, 127 / 128, ...) and the one-before-last: their intervals are made empty."""
    s = set()
    for b in range(64, S, 64):
        s |= {b - 1, b}
    s.add(S - 2)
    return sorted(x for x in s if 0 <= x <= S - 2)


def exact_inputs(n, S, addmul=False, noise=False, clamp=0.0, white=False, seed=0):
    """An input set of the exact regime (module docstring): intervals empty or G long, sigma terms in quarters (0 and negatives
    included), mul in {-0.5, 0, 0.25, 0.5, 0.75}, colour raws 0 / +-200 (clamp 10: 0 where alpha can be != 0;
    +-10 exactly, +-10.5 and +-200, clamped to +-10 where sigma <= 0, so that sigmoid(+-10) only meets w = 0), axis-aligned power-of-two directions, at most CAP samples with alpha != 0 per ray (none before the last without mul),
    and sigma > 0 on empty intervals on both sides of every chunk boundary and before the last sample."""
    rs = np.random.RandomState(seed)
    # directions: +-2^k along one axis
    d = np.zeros((n, 3), np.float32)
    d[np.arange(n), rs.randint(0, 3, n)] = rs.choice([-1, 1], n) * 2.0 ** rs.randint(-2, 3, n)
    # depths: empty or G-long intervals from a power-of-two-times-G start
    gaps = np.where(rs.rand(n, S) < 0.5, 0.0, G)
    gaps[:, 0] = G * rs.randint(0, 4, n)
    for s in _boundaries(S):
        gaps[:, s + 1] = 0.0
    z = np.cumsum(gaps, 1).astype(np.float32)
    dist = np.concatenate([np.diff(z, axis=1), np.full((n, 1), np.inf)], 1)     # inf: the last interval
    quarters = lambda *v: rs.choice(np.array(v, np.float32), (n, S))
    r3 = quarters(-1, -0.25, 0, 0.25, 0.5, 1, 3)
    if clamp > 0:
        r3 = np.where(rs.rand(n, S) < 0.2, quarters(-200, -10.5, -10, 10, 10.5, 200), r3)
    nz = quarters(-0.5, -0.25, 0, 0, 0.25, 0.5) if noise else None
    ad = quarters(-1, -0.25, 0, 0, 0.25, 1) if addmul else None
    ml = quarters(-0.5, 0, 0.25, 0.5, 0.75) if addmul else None
    # samples next to a chunk boundary: sigma > 0 on an empty interval (the only exact-regime samples with ddist != 0)
    for s in _boundaries(S):
        r3[:, s] = rs.choice(np.array([0.25, 0.5, 1, 3], np.float32), n)     # varied: equal neighbours would cancel in d_z
        if nz is not None:
            nz[:, s] = 0
        if ad is not None:
            ad[:, s] = 0.25
            ml[:, s] = rs.choice(np.array([0.25, 0.5, 0.75, 0], np.float32), n)

    def sigma():
        sg = np.clip(r3.astype(np.float64), -clamp, clamp) if clamp > 0 else r3.astype(np.float64)
        return sg + (0 if nz is None else nz) + (0 if ad is None else ad)
    live = (sigma() > 0) & (dist > 0) & ((ml > 0) if ml is not None else True)
    keep = np.zeros_like(live)
    for i in range(n):
        idx = np.flatnonzero(live[i])
        if ml is None:
            idx = idx[idx == S - 1]                             # alpha = 1: only on the last sample
        keep[i, rs.permutation(idx)[:CAP]] = True
    off = live & ~keep                                          # alpha forced to 0 through sigma <= 0 (0 exactly, or negative)
    r3 = np.where(off, rs.choice(np.array([0, -1], np.float32), (n, S)), r3)
    if nz is not None:
        nz = np.where(off, 0, nz).astype(np.float32)
    if ad is not None:
        ad = np.where(off, 0, ad).astype(np.float32)
    # colour raws: 0 / +-200; the values sigmoid does not give exactly (clamp: +-10, +-10.5) only where sigma <= 0 (alpha = 0, w = 0)
    if clamp > 0:                                               # clamped to 10: sigmoid(+-10) is not exact, so 0 where alpha can be != 0
        dead = (sigma() <= 0)[..., None] & (rs.rand(n, S, 3) < 0.6)
        rgb = np.where(dead, rs.choice(np.array([10, -10, 10.5, -10.5, 200, -200], np.float32), (n, S, 3)), np.float32(0))
    else:
        rgb = rs.choice(np.array([0, 200, -200], np.float32), (n, S, 3))
    raw = np.concatenate([rgb, r3[..., None]], -1).astype(np.float32)
    g = (rs.randint(-16, 17, (n, 3)) / 8.0).astype(np.float32)
    return dict(raw=raw, z=z, d=d, g=g, add=ad, mul=ml, noise=nz, clamp=clamp, white=white)


def random_inputs(n, S, addmul=False, noise=False, clamp=0.0, white=False, seed=0):
    """An input set of the general regime, as the older operator tests draw them, plus: raws exactly at +-clamp, empty intervals,
    mul exactly 0, sigma exactly 0, and no sigma within a few roundings of 0 (the kernels' relu branch must be decided the same way)."""
    rs = np.random.RandomState(seed)
    raw = (rs.randn(n, S, 4) * (4.0 if clamp > 0 else 1.5)).astype(np.float32)
    if clamp > 0:
        raw[rs.rand(n, S, 4) < 0.05] = clamp
        raw[rs.rand(n, S, 4) < 0.05] = -clamp
    z = np.sort(rs.uniform(0.05, 0.95, (n, S)), -1).astype(np.float32)
    rep = rs.rand(n, S) < 0.05
    rep[:, 0] = False
    for s in range(1, S):
        z[:, s] = np.where(rep[:, s], z[:, s - 1], z[:, s])
    d = rs.randn(n, 3).astype(np.float32)
    ad = rs.randn(n, S).astype(np.float32) if addmul else None
    ml = (rs.randn(n, S) + 0.7).astype(np.float32) if addmul else None
    if ml is not None:
        ml[rs.rand(n, S) < 0.05] = 0
    nz = rs.randn(n, S).astype(np.float32) if noise else None
    zero_sg = rs.rand(n, S) < 0.03                              # sigma exactly 0: the relu boundary
    if nz is not None:
        nz = np.where(zero_sg, 0, nz).astype(np.float32)
    if ad is not None:
        ad = np.where(zero_sg, 0, ad).astype(np.float32)
    raw[..., 3] = np.where(zero_sg, 0, raw[..., 3])
    inp = dict(raw=raw, z=z, d=d, g=rs.randn(n, 3).astype(np.float32), add=ad, mul=ml, noise=nz, clamp=clamp, white=white)
    # no sigma within a few roundings of 0 unless exactly 0: nudge the add (or noise, or raw) term
    for _ in range(3):
        r3 = np.clip(raw[..., 3], -clamp, clamp) if clamp > 0 else raw[..., 3]
        terms = [r3.astype(np.float64)] + [x.astype(np.float64) for x in (nz, ad) if x is not None]
        sg, mg = sum(terms), sum(np.abs(t) for t in terms)
        amb = (np.abs(sg) <= 8 * U * mg) & (sg != 0)
        if not amb.any():
            break
        tgt = ad if ad is not None else (nz if nz is not None else None)
        if tgt is not None:
            tgt[amb] += 0.5
        else:
            raw[..., 3][amb] += 0.5
    return inp
