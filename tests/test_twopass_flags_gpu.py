"""GPU: the two-pass sampler's per-ray error bound, its flag and its row bookkeeping (pnrf_sampler_fwd_ws: sampler_p1_kernel /
sampler_p1_skip_kernel, the list, pass 2's and pass 3's scatter) against tests/twopass_ref.py, the float64 restatement of DESIGN.md §4.1.

a. Critical kappa of every ray.  kappa is scanned over a geometric grid 1/8 .. 16 with step G = 2^(1/2048) - 1 (14 337 calls of 1024 rays per case, the
   lists copied on the device, no host wait inside the scan).  Every ray's flag is monotone over the grid (exact).  The first grid point kappa_j at
   which a ray is on the list brackets the kernel's own critical value, kappa_{j-1} < kappa* <= kappa_j, and the reference's — computed from the depths
   the kernel itself wrote at kappa = 0 — must lie in [kappa_{j-1} / (1 + DELTA), kappa_j (1 + DELTA)]; a ray listed at the first point has
   kappa*_ref <= (1/8)(1 + DELTA), one never listed kappa*_ref >= 16 / (1 + DELTA).  No ray is excluded.  DELTA = 1.4e-4 and G come from
   tests/test_twopass_flags_cpu.py, which also shows that every one-slip mutation of the bound moves kappa* by more than 2 (DELTA + G).
   The rays listed at kappa = 0 have had their pass-1 depths overwritten by pass 2, so for them the comparison is one-sided where it has to be:
   a ray NOT listed must not be flagged by the reference (exact: its depths are pass 1's); a ray listed must be flagged by the reference on the
   depths it has now, or have kappa*_ref <= 4 on them (pass 1's depths differ from these by its own error, |e| <= 4 s being 10.8 sigma of the model;
   largest |e| / s ever measured: 1.9) — at most 1 % of the rays may need the second clause.
b. Where every row comes from, at kappa = 2, 0 and 1e29, n = 1 .. 257 in both shapes and past the grid cap: the list has ws[1] distinct in-range
   entries; every listed row is the split kernel's row and every other row the kappa = 0 call's, torch.equal on all six outputs; a second call on the
   same workspace gives the same lists (as sets) and outputs.
c. Saturation (two hidden layers x300 and x70): at kappa = 0 pass 2's list holds every ray whose largest half-layer norm is above 65504^2 (1 + 1e-3)
   and none below 65504^2 (1 - 1e-3) that the reference does not flag otherwise; pass 3's rows are the exact-fp32 variant's bit for bit, the others
   follow b.

Worst share of DELTA used per case (printed by every run; 0 = the reference's kappa* inside the scan's own bracket), MI355X: d8_trained 0.001, d8_spread 0 (never
listed), d8_x4 0 (every ray at the fp16 limit), d6_x4 0, d3 0, d4 0.013, d9 0, d8_s4 0.027, d6_s04 0.000, the same in both shapes; no ray needed the second clause
at kappa = 0.  Against the mutated references of twopass_ref.MUTATIONS the same scan gives 13 .. 53 000 x DELTA (d9, d8_s4, d4).
"""
import functools

import numpy as np
import pytest
import torch

import twopass_ref as R

pytestmark = pytest.mark.gpu

USED = {}
SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    if USED:
        print('\n[twopass_flags] share of DELTA used (worst ray), second-clause rays at kappa = 0: ' + '   '.join(f'{k} {v[0]:.3f} / {v[1]}' for k, v in USED.items()))


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def pack(W, b, shape, variant=None):
    from pronerf_amd import ops
    return ops.PackedMLP(ops.NET_SAMPLER, W, b, variant=variant).set_shape(shape)


def two_pass(mlp, rays, kappa, ws=None):
    """-> (the six outputs, mask [n] of pass 2's list, mask [n] of pass 3's list), the lists checked: ws[1] / ws[5] distinct in-range entries."""
    from pronerf_amd import ops
    out = ops.sampler_fwd(mlp, rays, two_pass=True, want_raw=True, kappa=kappa, want_lists=True, workspace=ws)
    n = rays.shape[0]
    masks = []
    for cnt, lst in ((out[6], out[8]), (out[7], out[9])):
        cnt = int(cnt)
        assert 0 <= cnt <= n
        ent = lst[:cnt].long().cpu()
        assert bool(((ent >= 0) & (ent < n)).all()) and ent.unique().numel() == cnt
        m = torch.zeros(n, dtype=torch.bool)
        m[ent] = True
        masks.append(m)
    return [t.cpu() for t in out[:6]], masks[0], masks[1]


def rows_equal(a, b, rows):
    return all(torch.equal(x[rows], y[rows]) for x, y in zip(a, b))


def reference(W, b, skips, rays_np, outs):
    return R.critical_kappa(W, b, skips, rays_np, outs[0].numpy(), outs[1].numpy())


def check_kappa0(ref, listed):
    """The list of a kappa = 0 call against the reference on that call's depths (module docstring, a) -> number of rays that needed the second clause."""
    assert not ref['always'][~listed].any()
    second = listed & ~ref['always']
    assert bool((ref['kappa'][second] <= 4.0).all()), ref['kappa'][second].max()
    assert second.sum() <= 0.01 * len(listed), int(second.sum())
    return int(second.sum())


# ----------------------------------------------------------------------------------------------- a. critical kappa
def scan(dev, mlp, rays, ws):
    """One call per grid point on workspace ws -> (grid float64 [J] as passed (fp32 values), first [n]: index of the first grid point at which the ray is
    listed, ever [n]: listed at the last point, the last call's depths).  Lists are in range and distinct, every flag monotone over the grid."""
    import ctypes as C
    from pronerf_amd import _lib, ops
    lib = _lib.load()
    n = rays.shape[0]
    grid = R.kappa_grid().astype(np.float32)
    J = len(grid)
    d = torch.empty(n, 8, device=dev); a = torch.empty_like(d); m = torch.empty_like(d)
    rec = torch.empty(J, n + 1, device=dev, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = (mlp.handle, p(rays), n, p(d), p(a), p(m), None, None, None, p(ws), ws.numel() * 4)
    stream = ops._stream()
    for j in range(J):
        ops.check(lib.pnrf_sampler_fwd_ws(*args, float(grid[j]), stream), 'pnrf_sampler_fwd_ws')
        rec[j, 0] = ws[1]
        rec[j, 1:] = ws[16:16 + n]
    cnt, lst = rec[:, :1], rec[:, 1:].long()
    valid = torch.arange(n, device=dev)[None, :] < cnt
    assert not bool((valid & ((lst < 0) | (lst >= n))).any())
    flags = torch.zeros(J, n + 1, device=dev, dtype=torch.bool).scatter_(1, torch.where(valid, lst.clamp(0, n - 1), n), True)[:, :n]
    assert torch.equal(flags.sum(1, dtype=torch.int32), cnt[:, 0])                              # distinct entries
    assert not bool((flags[:-1] & ~flags[1:]).any())                                            # monotone, exact
    return grid.astype(np.float64), flags.to(torch.uint8).argmax(0).cpu().numpy(), flags[-1].cpu().numpy(), d.cpu()


def delta_used(k, grid, first, ever, free):
    """Per ray, how far the reference's kappa* lies outside the bracket the scan gives the kernel's, as a share of DELTA (<= 0: inside the bracket)."""
    at0, never, mid = free & ever & (first == 0), free & ~ever, free & ever & (first > 0)
    used = np.zeros(len(k))
    with np.errstate(all='ignore'):
        used[at0] = k[at0] / grid[0] - 1
        used[never] = grid[-1] / k[never] - 1
        used[mid] = np.maximum(k[mid] / grid[first[mid]] - 1, grid[first[mid] - 1] / k[mid] - 1)
    return used / R.DELTA, (int(at0.sum()), int(mid.sum()), int(never.sum()))


@pytest.mark.parametrize('name,shape', R.CASE_SHAPES)
def test_critical_kappa_of_every_ray(dev, name, shape):
    W, b, skips, rays_np = R.case(name)
    n = rays_np.shape[0]
    rays = cu(rays_np, dev)
    mlp = pack(W, b, shape)
    ws = torch.zeros(16 + 2 * n, device=dev, dtype=torch.int32)
    out0, listed0, _ = two_pass(mlp, rays, 0.0, ws)
    listed0 = listed0.numpy()
    ref = reference(W, b, skips, rays_np, out0)
    second = check_kappa0(ref, listed0)
    grid, first, ever, d = scan(dev, mlp, rays, ws)
    assert bool((first[listed0] == 0).all()) and bool(ever[listed0].all())                      # flagged at no margin: flagged at every margin
    assert torch.equal(d[~torch.from_numpy(ever)], out0[0][~torch.from_numpy(ever)])            # rows never listed: pass 1's, as in the kappa = 0 call
    used, (at0, mid, never) = delta_used(ref['kappa'].astype(np.float64), grid, first, ever, ~listed0)
    worst = max(float(used.max()), 0.0)
    USED[f'{name}/{shape}'] = (worst, second)
    print(f'\n[twopass_flags] {name} {shape}: listed at kappa = 0: {int(listed0.sum())} ({second} by the second clause), at the first grid point {at0}, '
          f'inside {mid}, never {never}; worst share of DELTA used {worst:.3f}')
    assert worst <= 1.0, (worst, int(np.argmax(used)))


# ----------------------------------------------------------------------------------------------- b. where every row comes from
@functools.lru_cache(maxsize=None)
def _row_nets(shape):
    W, b, skips, rays_np = R.case('d8_trained')
    return pack(W, b, shape), pack(W, b, shape, 'sampler_split'), rays_np


def check_rows(dev, mlp, split, rays, kappa, base=None):
    """Rule b on one call -> (outputs, listed mask).  base: the kappa = 0 call's outputs (made here when absent)."""
    from pronerf_amd import ops
    n = rays.shape[0]
    ws = torch.zeros(16 + 2 * n, device=dev, dtype=torch.int32)
    if base is None:
        base = two_pass(mlp, rays, 0.0)[0]
    out, listed, sat = two_pass(mlp, rays, kappa, ws)
    assert not bool(sat.any())
    ref = [t.cpu() for t in ops.sampler_fwd(split, rays, want_raw=True)]
    assert rows_equal(out, ref, listed) and rows_equal(out, base, ~listed)
    again, listed2, sat2 = two_pass(mlp, rays, kappa, ws)                                       # the same workspace, as the call left it
    assert torch.equal(listed2, listed) and torch.equal(sat2, sat) and rows_equal(again, out, slice(None))
    return out, listed, ref


@pytest.mark.parametrize('shape', ['narrow', 'wide'])
@pytest.mark.parametrize('n', SIZES)
def test_rows_come_from_the_split_kernel_or_from_pass_1(dev, n, shape):
    mlp, split, rays_np = _row_nets(shape)
    rays = cu(rays_np[:n], dev)
    base, listed0, _ = check_rows(dev, mlp, split, rays, 0.0)
    out, listed, _ = check_rows(dev, mlp, split, rays, 2.0, base)
    assert bool((listed | ~listed0).all())                                                      # kappa = 0's rays are on every list
    out, listed, ref = check_rows(dev, mlp, split, rays, 1e29, base)
    assert bool(listed.all()) and rows_equal(out, ref, slice(None))                             # a permutation of 0 .. n - 1; the split kernel's output


@pytest.mark.parametrize('shape', ['narrow', 'wide'])
def test_rows_past_the_grid_cap(dev, shape):
    from pronerf_amd import ops
    mlp, split, rays_np = _row_nets(shape)
    n = 2 * torch.cuda.get_device_properties(dev).multi_processor_count * 256 + 37
    small = cu(rays_np, dev)
    per = torch.arange(n) % rays_np.shape[0]
    rays = small[per.to(dev)].contiguous()
    base_s = two_pass(mlp, small, 0.0)[0]
    out_s, listed_s, _ = two_pass(mlp, small, 2.0)
    split_s = [t.cpu() for t in ops.sampler_fwd(split, small, want_raw=True)]
    out, listed, sat = two_pass(mlp, rays, 2.0)
    assert not bool(sat.any()) and torch.equal(listed, listed_s[per])                           # the periodic extension of the small call's set
    assert 0 < int(listed_s.sum()) < rays_np.shape[0]
    for x, sp, ba in zip(out, split_s, base_s):
        assert torch.equal(x[listed], sp[per][listed]) and torch.equal(x[~listed], ba[per][~listed])


# ----------------------------------------------------------------------------------------------- the edge of the gap rule
@pytest.mark.parametrize('which', ['tie', 'near'])
def test_rays_on_the_edge_of_the_gap_rule_are_listed(dev, which):
    """Tied depth logits (gap exactly 0; with near = far the threshold is 0 too and the comparison not finite) and logits 2e-6 apart (0 < gap inside the
    2e-6 span allowance): all of them are listed at kappa = 0, and their rows are the split kernel's."""
    W, b, skips, rays_np = R.edge_case(which)
    rays = cu(rays_np, dev)
    mlp, split = pack(W, b, 'narrow'), pack(W, b, 'narrow', 'sampler_split')
    out, listed, ref = check_rows(dev, mlp, split, rays, 0.0)
    z = out[0].numpy()
    gap = (z[:, 1:] - z[:, :-1]).min(1)
    span = rays_np[:, 7] - rays_np[:, 6]
    if which == 'tie':
        assert bool((gap == 0).all())
    else:
        assert ((gap > 0) & (gap <= np.float32(2e-6) * span)).mean() > 0.9
    assert bool(listed.all())
    assert bool(reference(W, b, skips, rays_np, out)['always'].all())


# ----------------------------------------------------------------------------------------------- c. saturation
@pytest.mark.parametrize('which,shape', [('x300', 'narrow'), ('x300', 'wide'), ('x70', 'wide'), ('x70', 'narrow')])
def test_saturated_rays_go_through_the_exact_pass(dev, which, shape):
    from pronerf_amd import ops
    W, b, skips, rays_np = R.saturating_case(which)
    n = rays_np.shape[0]
    rays = cu(rays_np, dev)
    mlp, split, f32 = pack(W, b, shape), pack(W, b, shape, 'sampler_split'), pack(W, b, shape, 'sampler_f32')
    lone = [t.cpu() for t in ops.sampler_fwd(split, rays, want_raw=True)]                       # saturating arithmetic, no third pass
    exact = [t.cpu() for t in ops.sampler_fwd(f32, rays, want_raw=True)]
    ws = torch.zeros(16 + 2 * n, device=dev, dtype=torch.int32)
    base, listed0, sat0 = two_pass(mlp, rays, 0.0, ws)
    ref = reference(W, b, skips, rays_np, base)
    norm = ref['norm'] / R.OVF2
    band = np.abs(norm - 1) <= R.SAT_BAND
    assert band.mean() <= 0.02
    hi, lo = torch.from_numpy(norm > 1 + R.SAT_BAND), torch.from_numpy(norm < 1 - R.SAT_BAND)
    assert bool(listed0[hi].all())
    rest = ref['gap'] | ref['nonfinite'] | (ref['kappa'] <= 4.0)                                # (module docstring, a: listed rows carry pass 2's depths)
    assert not (listed0 & lo).numpy()[~rest].any()
    assert not (ref['gap'] | ref['nonfinite'])[(~listed0).numpy()].any()
    print(f'\n[twopass_flags] {which} {shape}: norm above / below / in the band {int(hi.sum())} / {int(lo.sum())} / {int(band.sum())}; pass 2 {int(listed0.sum())}, pass 3 {int(sat0.sum())}')
    assert int(hi.sum()) > 0 and (which == 'x300' or int(lo.sum()) > 0)
    assert which != 'x300' or int(sat0.sum()) > 0
    for kappa in (0.0, 2.0):
        out, listed, sat = (base, listed0, sat0) if kappa == 0.0 else two_pass(mlp, rays, kappa, ws)
        assert bool((listed | ~sat).all()) and bool((listed | ~listed0).all())                  # pass 3's rays come from pass 2's list
        assert rows_equal(out, exact, sat) and rows_equal(out, lone, listed & ~sat) and rows_equal(out, base, ~listed)
        for t in out:
            assert bool(torch.isfinite(t.float()).all())
