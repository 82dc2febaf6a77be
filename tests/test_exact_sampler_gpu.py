"""GPU: the fused sampler stage on integer nets with exact answers, at the shapes the frame path runs (tests/exact_sampler.py; certified on the CPU by
tests/test_exact_sampler_cpu.py).  288 = 6 x 48 input columns; depths 2, 5, 6, 8 without skips reach the kernels without the ``_skip`` suffix —
``sampler_p1_kernel<4 | 8>`` and, for listed rays, ``sampler_h16_kernel<4 | 8>`` ('default', two passes), ``sampler_h16_kernel<4 | 8>`` ('sampler_split'),
``sampler_kernel<2>`` ('sampler_f32'), ``sampler_kernel<1>`` ('sampler_f32_full') — at both parities of the hidden-layer count and the shortest chain.

  * the exact-fp32 kernels give the integers bit for bit and the one sort order the head's biases fix;
  * the two kernels on log2(e)-scaled streams give add / mul within T = 4 B of the integers (B, T: exact_sampler's docstring; <= 1.4e-3, where one
    operand, plane, k-step or pair read from the wrong place moves an output by >= 1), the same indices, and depth_raw within 2e-7 of sigmoid;
  * x_big (moment components 2048 .. 2051) puts integers into P_lo and into a first-layer W_lo; hid_big (activations in [2048, 4096]) into the X_lo'
    planes of the split kernel — the operands that the integer nets of tests/test_mmskips_gpu.py multiply by zero.  Both run the skip forms too
    (``sampler_p1_skip_kernel``, ``sampler_h16_skip_kernel``, ``sampler_skip_kernel``), whose x k-step reuses layer 0's P0h / P0l;
  * the pass-2 list path on exact answers: rays with near == far are flagged at every kappa; list, count, rows of both origins, counters re-armed;
  * a +1 on one weight makes the same comparison fail.

Measured on the MI355X (printed by the tests): the exact-fp32 kernels 0 everywhere; pass 1 0 .. 1.7e-5 and the split kernel 9.5e-7 .. 3.2e-4 on the nets
without skips, which is the replay's own deviation to three digits; the split kernel's skip form on x_big 3.5e-4 (T = 3.7e-4, D = 3 skips [0, 1]) and
4.0e-4 (T = 7.2e-4, D = 6 skips [0, 4]): its main accumulator passes through partial sums of 2^11 .. 2^12 in the x k-step while it carries the
fractional parts of zero units, an fp32 ulp there (2.4e-4) that the replay, which rounds an accumulator once, does not have.  Nothing in the kernels or
the packer had to change.  The 24 cases take 3.2 s of test calls (the file alone: 4.8 s).
"""
import numpy as np
import pytest
import torch

import exact_nets as en
import exact_sampler as xs

pytestmark = pytest.mark.gpu

NOSKIP = [(D, ()) for D in xs.DEPTHS]
VARIANTS = (('default', True, 'p1'), ('sampler_split', False, 'h16'), ('sampler_f32', False, None), ('sampler_f32_full', False, None))   # variant, two_pass, replay


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pack(net, variant, W=None):
    from pronerf_amd import ops
    if variant in ('default', 'sampler_split'):
        Wp, bp = xs.pack_scaled(net, W)
    else:
        Wp, bp = xs.pack_true(net if W is None else dict(net, W=W))
    mlp = ops.PackedMLP(ops.NET_SAMPLER, Wp, bp, variant=variant)
    assert mlp.skips == list(net['skips'])
    return mlp


def _check(out, y, order, T, tag, two_pass):
    """One call's outputs against the exact rows y [n, 27]: T None: bit for bit."""
    n = len(y)
    if two_pass:
        assert int(out[6]) == 0 and int(out[7]) == 0, tag                  # no ray went to the second / third pass: these are pass 1's rows
    add, mul = xs.answers(y, order)
    np.testing.assert_array_equal(out[1].cpu().numpy(), np.tile(order, (n, 1)), err_msg=tag)
    got_add, got_mul = out[2].cpu().numpy().astype(np.float64), out[3].cpu().numpy().astype(np.float64)
    if T is None:
        np.testing.assert_array_equal(got_add, add, err_msg='add: ' + tag)
        np.testing.assert_array_equal(got_mul, mul, err_msg='mul: ' + tag)
    else:
        np.testing.assert_allclose(got_add, add, rtol=0, atol=T, err_msg='add: ' + tag)
        np.testing.assert_allclose(got_mul, mul, rtol=0, atol=T, err_msg='mul: ' + tag)
    np.testing.assert_allclose(out[5].cpu().numpy(), 1 / (1 + np.exp(-y[:, :8])), rtol=0, atol=2e-7, err_msg='depth_raw: ' + tag)


def _run_family(dev, family, D, skips, variants, shapes, counts):
    from pronerf_amd import ops
    net = xs.net_for(D, skips, family)
    rays = xs.rays_for(family, max(counts), seed=D)
    y = xs.exact_rows(net, rays)
    order = xs.order_of(net)
    rd = torch.from_numpy(rays).to(dev)
    failed = []
    for variant, two_pass, kind in variants:
        T = None if kind is None else xs.tol(family, kind, D, skips)
        mlp = _pack(net, variant)
        worst = 0.0
        for shp in shapes:
            mlp.set_shape(shp)
            for n in counts:
                out = ops.sampler_fwd(mlp, rd[:n].contiguous(), want_idx=True, want_rgb=True, want_raw=True, two_pass=two_pass)
                add, mul = xs.answers(y[:n], order)
                worst = max(worst, float(np.abs(out[2].cpu().numpy() - add).max()), float(np.abs(out[3].cpu().numpy() - mul).max()))
                try:                                                       # (every figure is printed before the first failure is raised)
                    _check(out, y[:n], order, T, f'{family} {variant} {shp}: D {D} skips {list(skips)} n {n}', two_pass)
                except AssertionError as e:
                    failed.append(str(e)[:600])
        print(f'\n[exact_sampler] {family} D {D} skips {list(skips)} {variant}: largest |add, mul - integer| (in the order the biases fix) {worst:.3g}, T = {T}', end='')
    assert not failed, f'{len(failed)} calls failed, the first:\n{failed[0]}'


@pytest.mark.parametrize('D,skips', NOSKIP)
def test_noskip_small_inputs(dev, cus, D, skips):
    """The default kernels on the [0, 2] inputs: every batch edge, the three shapes; at D = 6 also the narrow / wide switch +-1 and a count at which a
    persistent workgroup takes a second batch and the weight ring wraps."""
    _run_family(dev, 'small', D, skips, VARIANTS, ('narrow', 'wide', 'auto'), en.refine_counts(cus, big=D == 6))


@pytest.mark.parametrize('D,skips', NOSKIP + list(xs.SKIP_NETS))
def test_x_big(dev, D, skips):
    """Large inputs: the W_hi P_lo and W_lo P_hi products of layer 0 (and of the skip layers' x k-step) carry integers of the answer."""
    variants = VARIANTS if not skips else VARIANTS[:3]                    # (the unfolded stream has no skip form)
    _run_family(dev, 'x_big', D, skips, variants, ('narrow', 'wide'), en.refine_counts(0, big=False))


@pytest.mark.parametrize('D,skips', NOSKIP + list(xs.SKIP_NETS))
def test_hid_big(dev, D, skips):
    """Large hidden activations: the X_lo' planes of the split kernel carry integers of the answer in every layer (pass 1 holds one fp16 plane: not run)."""
    _run_family(dev, 'hid_big', D, skips, (VARIANTS[1], VARIANTS[2]), ('narrow', 'wide'), en.refine_counts(0, big=False))


@pytest.mark.parametrize('shape', ['narrow', 'wide'])
def test_pass2_list_on_exact_answers(dev, shape):
    """x_big, D = 6, n = 257, kappa = 0: the rays with near == far (and only they) go through the list to the split kernel; their depths are ``near``, the
    eight ties keep the identity order, add / mul are the integers unpermuted.  Every call runs on the workspace as the call before left it."""
    from pronerf_amd import ops
    net = xs.net_for(6, (), 'x_big')
    mlp = _pack(net, 'default').set_shape(shape)
    n = xs.LIST_N
    order, ident = xs.order_of(net), np.arange(8)
    T1, T2 = xs.tol('x_big', 'p1', 6), xs.tol('x_big', 'h16', 6)
    ws = torch.zeros(16 + 2 * n, device=dev, dtype=torch.int32)
    for size in xs.LIST_SIZES + (1, 0):
        sub = xs.flag_subset(size)
        rays = xs.rays_for('x_big', n, seed=6, same=sub)
        y = xs.exact_rows(net, rays)
        out = ops.sampler_fwd(mlp, torch.from_numpy(rays).to(dev), want_idx=True, want_raw=True, two_pass=True, kappa=0.0, want_lists=True, workspace=ws)
        tag = f'{shape} subset of {size}'
        assert int(out[6]) == size and int(out[7]) == 0, tag
        np.testing.assert_array_equal(np.sort(out[8][:size].cpu().numpy()), sub, err_msg=tag)
        mask = np.zeros(n, bool); mask[sub] = True
        idx, ds = out[1].cpu().numpy(), out[0].cpu().numpy()
        np.testing.assert_array_equal(idx[mask], np.tile(ident, (size, 1)), err_msg=tag)
        np.testing.assert_array_equal(idx[~mask], np.tile(order, (n - size, 1)), err_msg=tag)
        np.testing.assert_array_equal(ds[mask], np.full((size, 8), 0.5, np.float32), err_msg=tag)
        for got, lo in ((out[2].cpu().numpy(), 8), (out[3].cpu().numpy(), 16)):
            np.testing.assert_allclose(got[mask], y[mask, lo:lo + 8], rtol=0, atol=T2, err_msg=tag)
            np.testing.assert_allclose(got[~mask], y[~mask, lo:lo + 8][:, order], rtol=0, atol=T1, err_msg=tag)
        np.testing.assert_allclose(out[5].cpu().numpy(), 1 / (1 + np.exp(-y[:, :8])), rtol=0, atol=2e-7, err_msg=tag)


@pytest.mark.parametrize('layer', [0, 3])
@pytest.mark.parametrize('variant,two_pass,kind', VARIANTS[:3])
def test_mutated_weight_fails(dev, variant, two_pass, kind, layer):
    """Self-check: +1 on one first-layer / hidden weight (exact_nets.mutate), packed anew: the comparison with the unmutated answer fails."""
    from pronerf_amd import ops
    net = xs.net_for(6, (), 'x_big')
    n = 257
    rays = xs.rays_for('x_big', n, seed=6)
    y, order = xs.exact_rows(net, rays), xs.order_of(net)
    T = None if kind is None else xs.tol('x_big', kind, 6)
    rd = torch.from_numpy(rays).to(dev)
    _check(ops.sampler_fwd(_pack(net, variant), rd, want_idx=True, want_raw=True, two_pass=two_pass), y, order, T, 'unmutated', two_pass)
    mlp = None
    for seed in range(8):                     # (a mutated first-layer weight may have no float32 pre-image: the next seed's entry then)
        Wm, where = en.mutate(net['W'], layer, seed=seed)
        try:
            mlp = _pack(net, variant, Wm)
            break
        except AssertionError:
            continue
    assert mlp is not None
    out = ops.sampler_fwd(mlp, rd, want_idx=True, want_raw=True, two_pass=two_pass)
    with pytest.raises(AssertionError):
        _check(out, y, order, T, f'mutated {where}', two_pass)
