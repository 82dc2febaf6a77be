"""GPU: the per-ray kernels between the MLPs — compositing forward (composite_kernel, composite_thread_kernel), its backward
(composite_bwd_kernel) and stage-1 exploration (explore_kernel) — against answers that are exact, and the sampler head's sort on ties.

Exact assertions (``assert_array_equal``):
  * compositing on the exact-regime sets of tests/exact_composite.py, whose replay tests/test_exact_composite_cpu.py certifies: every
    intermediate is exactly representable, so fused multiply-adds and summation order cannot change a bit;
  * the thread-per-ray forward (>= 65 536 rays) against the wave-per-ray forward on the same rays, and against the exact answers;
  * d_stride = 11 (rays[:, 3:6] of the [n, 11] rays, the trainer's case) against a contiguous copy;
  * exploration against orc.explore_samples in float32: both do the same IEEE operations, and ties cannot change sorted values;
  * the sampler head's indices, add and mul against the oracle's stable sort, on tied depths.
Bounded assertions: compositing forward and backward on general inputs, elementwise within 2 (S + 9) 2^-24 mag of the float64 oracle
(exact_composite.BOUND_DOC derives the constants; expf's error is an assumption stated there).
"""
import functools

import numpy as np
import pytest
import torch

import exact_composite as X
from oracle import pronerf_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def cu(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run(inp, dev, d=None):
    """ops.composite and ops.composite_bwd on an input set -> dict of numpy outputs (d: the directions to pass, default a copy of inp['d'])."""
    from pronerf_amd import ops
    raw, z, d = cu(inp['raw'], dev), cu(inp['z'], dev), cu(inp['d'], dev) if d is None else d
    kw = dict(add=cu(inp['add'], dev), mul=cu(inp['mul'], dev), noise=cu(inp['noise'], dev), clamp=inp['clamp'], white_bkgd=inp['white'])
    rgb, disp, acc, w, depth = ops.composite(raw, z, d, **kw)
    d_raw, d_z, d_add, d_mul = ops.composite_bwd(raw, z, d, cu(inp['g'], dev), **kw)
    out = dict(rgb=rgb, disp=disp, acc=acc, w=w, depth=depth, d_raw=d_raw, d_z=d_z, d_add=d_add, d_mul=d_mul)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


@functools.lru_cache(maxsize=None)
def exact(S, oi):
    inp = X.exact_case(S, oi)
    return inp, X.certify(inp)


def assert_exact(got, exp, what):
    for k in exp:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f'{k} {what}')


@pytest.mark.parametrize('S', X.S_BWD)
def test_composite_exact(dev, S):
    """Forward and backward, every option set, 1 / 3 / 4 / 5 / 257 rays (n mod 4 != 0: idle waves in the last block): bit for bit."""
    for oi in range(len(X.OPTS)):
        inp, exp = exact(S, oi)
        for n in X.NS:
            assert_exact(run(X.head(inp, n), dev), X.head(exp, n), f'S={S} opts={X.OPTS[oi]} n={n}')


@pytest.mark.parametrize('S', X.S_BWD)
def test_composite_bounded(dev, S):
    """General inputs: every output element within the derived bound of the float64 oracle and its autograd."""
    for oi in range(len(X.OPTS)):
        inp = X.random_case(S, oi)
        ref = X.reference(inp)
        _, mag = X.magnitudes(inp)
        for n in X.NS:
            got = run(X.head(inp, n), dev)
            bad = X.check_bound(got, X.head(ref, n), X.head(mag, n), S, list(ref))
            assert not bad, (S, X.OPTS[oi], n, bad)


@pytest.mark.parametrize('S', X.S_THREAD)
def test_thread_kernel(dev, S):
    """65 573 rays take composite_thread_kernel (four samples in flight, an m < 4 tail); the same rays in slices below 65 536 take
    composite_kernel (partial chunks for S = 65, 72, 129).  All five outputs agree bit for bit, on general inputs and on the exact set
    (tiled), which must also give the exact answers."""
    from pronerf_amd import ops
    oi = X.S_THREAD.index(S) % len(X.OPTS)
    inp_e, exp = exact(S, oi)
    sets = [(X.tile(inp_e, X.N_THREAD), X.tile(exp, X.N_THREAD)), (X.random_inputs(X.N_THREAD, S, *X.OPTS[oi], seed=S), None)]
    for inp, want in sets:
        raw, z, d = cu(inp['raw'], dev), cu(inp['z'], dev), cu(inp['d'], dev)
        kw = dict(add=cu(inp['add'], dev), mul=cu(inp['mul'], dev), noise=cu(inp['noise'], dev), clamp=inp['clamp'], white_bkgd=inp['white'])
        whole = [t.cpu().numpy() for t in ops.composite(raw, z, d, **kw)]
        parts = []
        for a, b in ((0, 40000), (40000, 65536), (65536, X.N_THREAD)):
            kwp = {k: (v[a:b].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
            parts.append([t.cpu().numpy() for t in ops.composite(raw[a:b].contiguous(), z[a:b].contiguous(), d[a:b].contiguous(), **kwp)])
        for k, name in enumerate(X.FWD_KEYS):
            np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]), err_msg=f'{name} S={S}')
            if want is not None:
                np.testing.assert_array_equal(whole[k], want[name], err_msg=f'{name} S={S} (exact)')


@pytest.mark.parametrize('S,n', [(8, 257), (72, 5), (136, 257), (256, 3), (8, X.N_THREAD)])
def test_strided_directions(dev, S, n):
    """rays_d as rays[:, 3:6] of an [n, 11] tensor (d_stride = 11, what the trainer passes): bit-identical to a contiguous copy, forward
    (both kernels: n = 65 573 takes the thread-per-ray one) and backward, and exact."""
    oi = 1 if n == X.N_THREAD else 2
    inp, exp = exact(S, oi)
    inp, exp = (X.tile(inp, n), X.tile(exp, n)) if n > 257 else (X.head(inp, n), X.head(exp, n))
    rays = torch.randn(n, 11, generator=torch.Generator().manual_seed(S)).to(dev)
    rays[:, 3:6] = cu(inp['d'], dev)
    view = rays[:, 3:6]
    assert view.stride() == (11, 1)
    got_v, got_c = run(inp, dev, view), run(inp, dev, view.contiguous())
    for k in got_c:
        np.testing.assert_array_equal(got_v[k], got_c[k], err_msg=k)
    assert_exact(got_v, exp, f'S={S} n={n} strided')


def _explore_inputs(n, n_mult, seed):
    """Refined depths with ties: repeated values, values equal to near or far, zero gaps; jitter 0 on a third of the samples."""
    rs = np.random.RandomState(seed)
    rays = rs.randn(n, 11).astype(np.float32)
    near = rs.choice(np.array([0.0, 0.5, 2.0], np.float32), n)
    far = near + rs.choice(np.array([1.0, 4.0], np.float32), n)
    rays[:, 6], rays[:, 7] = near, far
    grid = near[:, None] + (far - near)[:, None] * rs.choice(np.array([0, 0.125, 0.25, 0.25, 0.5, 0.75, 1.0], np.float32), (n, 8))
    free = near[:, None] + (far - near)[:, None] * rs.rand(n, 8).astype(np.float32)
    z8 = np.sort(np.where(rs.rand(n, 8) < 0.6, grid, free).astype(np.float32), 1)
    z8[: n // 4, 3:6] = z8[: n // 4, 3:4]                        # a run of equal depths
    z8[n // 4: n // 2, 0] = near[n // 4: n // 2]                 # first depth at near, last at far
    z8[n // 4: n // 2, 7] = far[n // 4: n // 2]
    z8 = np.sort(z8, 1)
    jit = np.minimum(np.abs(rs.randn(n, 8 * n_mult)) / 5, 0.99).astype(np.float32)
    jit[rs.rand(n, 8 * n_mult) < 0.33] = 0
    return rays, z8, jit


@pytest.mark.parametrize('n_mult', range(1, 33))
def test_explore_exact(dev, n_mult):
    """ops.explore against orc.explore_samples in float32, and pts = o + d z, bit for bit: both signs of dir1 and dir2, 1 / 5 / 4097 rays."""
    from pronerf_amd import ops
    rays, z8, jit = _explore_inputs(4097, n_mult, n_mult)
    assert (np.diff(z8, axis=1) == 0).any() and (z8 == rays[:, 6:7]).any() and (z8 == rays[:, 7:8]).any() and (jit == 0).any()
    rt, zt, jt = torch.from_numpy(rays), torch.from_numpy(z8), torch.from_numpy(jit)
    for dir1 in (1, -1):
        for dir2 in (1, -1):
            zr = orc.explore_samples(zt, rt[:, 6:7], rt[:, 7:8], n_mult, dir1, jt, dir2)
            pr = rt[:, None, 0:3] + rt[:, None, 3:6] * zr[..., None]
            for n in (1, 5, 4097):
                zg, pg = ops.explore(cu(z8[:n], dev), cu(rays[:n], dev), cu(jit[:n], dev), n_mult, dir1, dir2)
                np.testing.assert_array_equal(zg.cpu().numpy(), zr[:n].numpy(), err_msg=f'z n_mult={n_mult} dir={dir1},{dir2} n={n}')
                np.testing.assert_array_equal(pg.cpu().numpy(), pr[:n].numpy(), err_msg=f'pts n_mult={n_mult} dir={dir1},{dir2} n={n}')


def test_sampler_head_ties(dev):
    """Tied depths: saturated y (sigmoid exactly 0, 1; and 0.5 at y = 0) and rays with near == far.  Indices, depths, add and mul equal
    the oracle's stable sort."""
    from pronerf_amd import ops
    rs = np.random.RandomState(11)
    n = 1000
    y = rs.randn(n, 27).astype(np.float32)
    y[:, :8] = rs.choice(np.array([-200, 0, 200], np.float32), (n, 8))
    y[: n // 8, :8] = rs.randn(n // 8, 8)                       # untied depths on some rays, on near == far rays below too
    rays = rs.randn(n, 11).astype(np.float32)
    rays[:, 6] = rs.choice(np.array([0.0, 1.0, 2.0], np.float32), n)
    rays[:, 7] = rays[:, 6] + rs.choice(np.array([0.0, 0.0, 1.0, 2.0], np.float32), n)
    assert (rays[:, 6] == rays[:, 7]).any()
    yt, rt = torch.from_numpy(y), torch.from_numpy(rays)
    depth = torch.sigmoid(yt[:, :8])
    ds, idx, adds, muls = orc.sort_gather(depth, yt[:, 8:16], yt[:, 16:24], rt[:, 6:7], rt[:, 7:8])
    tied = (ds[:, 1:] == ds[:, :-1]).any(1)
    assert float(tied.float().mean()) > 0.5
    D, I, A, M, _ = ops.sampler_head_fwd(cu(y, dev), cu(rays, dev))
    np.testing.assert_array_equal(I.cpu().numpy(), idx.numpy())
    sat = np.ones(n, bool); sat[: n // 8] = False                # sigmoid of a saturated / zero y is exact in both
    np.testing.assert_array_equal(D.cpu().numpy()[sat], ds.numpy()[sat])
    np.testing.assert_array_equal(A.cpu().numpy(), adds.numpy())
    np.testing.assert_array_equal(M.cpu().numpy(), muls.numpy())
