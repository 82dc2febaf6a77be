"""CPU: the integer training nets and output gradients of tests/test_exact_train_gpu.py are exact for every input set that file runs — forward
and backward products integer, sums of |terms| below 2^24 (the weight-gradient reductions over all rows included), every split operand
exact at the scales the kernels can choose, exact-zero ReLU pre-activations present — the generators are deterministic, and the split check
rejects a value that loses bits."""
import numpy as np
import pytest

import exact_nets as E

L_N = 14


@pytest.fixture(scope='module')
def nets():
    return E.train_nets()


def _elu(nets, first):
    W, b = nets
    return W[first:first + 7], b[first:first + 7]


@pytest.mark.parametrize('first', [0, 7])
def test_elu_train_certificate(nets, first):
    W, b = _elu(nets, first)
    x = E.elu_inputs(max(E.ELU_COUNTS), W[0].shape[1])
    for n in E.ELU_COUNTS:
        E.certify_elu_train(W, b, x[:n], E.train_dy(n, W[-1].shape[0], seed=n))


def _nerf_sets():
    sets = [(8, n, n) for n in E.NERF_S8] + [(S, n, S + n) for S, n in E.NERF_BIG]
    sets += [(8, E.nerf_cu_rays(cus), 3) for cus in (80, 104, 256)]
    sets += [(8, n, s) for n in (1023, 1025) for s in (11, 5, 21)] + [(8, 4101, 31), (8, 1025, 31)]
    return sets


@pytest.mark.parametrize('S,n,seed', _nerf_sets())
def test_nerf_train_certificate(nets, S, n, seed):
    W, b = nets
    inp = E.nerf_inputs(n, live=E.TRAIN_LIVE, n_samples=S)
    ref = E.NerfTrainRef(W[L_N:], b[L_N:], inp)
    E.certify_nerf_train(ref, E.train_dy(ref.R, 4, seed=seed), f'S={S} n={n}')


def test_nerf_onehot_certificate(nets):
    W, b = nets
    S, n = E.NERF_ONEHOT
    ref = E.NerfTrainRef(W[L_N:], b[L_N:], E.nerf_inputs(n, live=E.TRAIN_LIVE, n_samples=S))
    for r in E.onehot_rows(ref.R):
        dy = np.zeros((ref.R, 4), np.float32)
        dy[r] = (1, -2, 3, 1)
        E.certify_nerf_train(ref, dy, f'one-hot {r}')


def test_relu_zero_preactivations_occur(nets):
    """Exact zeros among the ReLU pre-activations (relu'(0) = 0: torch and the kernels' v > 0 masks must agree there), in every ReLU layer
    of the fine net, and on rows that carry a gradient."""
    W, b = nets
    inp = E.nerf_inputs(1025, live=E.TRAIN_LIVE, n_samples=8)
    ref = E.NerfTrainRef(W[L_N:], b[L_N:], inp)
    for l in list(range(8)) + [10]:
        Z = ref.X[l] @ np.asarray(W[L_N + l]).T + b[L_N + l]
        assert (Z == 0).sum() > 0, f'layer {l}: no pre-activation is exactly 0'


def test_exact_and_inexact_columns(nets):
    """Which weight-gradient columns are exact is derived from the inputs: pts0 and the skip layer's embedding are exact on the raw x, y, z
    and the live coordinate's sin / cos, views_linears.0 on the features and the view embedding's zero coordinates; d_pts everywhere."""
    W, b = nets
    ref = E.NerfTrainRef(W[L_N:], b[L_N:], E.nerf_inputs(1025, live=E.TRAIN_LIVE, n_samples=8))
    live = E.pe_cols(E.TRAIN_LIVE, E.MULTIRES)
    for l in (0, 5):
        ex = ref.exact_cols(l)
        assert ex[:3].all() and ex[live].all() and (l == 0 or ex[63:].all())
        assert not ex[[c for c in range(3, 63) if c not in live]].any()
    ex = ref.exact_cols(10)
    assert ex[:256].all() and ex[256:259].all() and ex[[256 + c for c in E.pe_cols(E.TRAIN_LIVE, E.MULTIRES_V)]].all() and not ex.all()
    for l in (1, 2, 3, 4, 6, 7, 8, 9, 11):
        assert ref.exact_cols(l).all()
    assert E.nerf_dpts_exact_cols(ref.W, ref).all()


def test_split_check_rejects_a_lossy_value():
    """2049 + 2^-12 spans 24 bits: hi = 2050 and (2049 + 2^-12 - 2050) 2^11 = -2047.5 is no fp16 (2049 + 2^-10: -2046, exact).  1 + 2^-11 +
    2^-23 likewise (lo would need 13 bits); 1 + 2^-13 at scale 2^-24 leaves a lo below fp16's range; 70000 overflows hi."""
    assert E.split_exact(np.array([1.0, 2049.0, 4097.0, 65503.0, 2049.0 + 2.0 ** -10]))
    assert not E.split_exact(np.array([2049.0 + 2.0 ** -12]))
    assert not E.split_exact(np.array([1.0 + 2.0 ** -11 + 2.0 ** -23]))
    assert not E.split_exact(np.array([1.0 + 2.0 ** -13]), 2.0 ** -24) and E.split_exact(np.array([3.0]), 2.0 ** -24)
    assert not E.split_exact(np.array([70000.0]))                       # fp16 hi overflows
    assert E.hg_scale_for(0.0) == 1.0 and E.hg_scale_for(2048.0) == 1.0 and E.hg_scale_for(3.0) == 2.0 ** 10


def test_train_generators_deterministic(nets):
    W2, b2 = E.train_nets()
    for u, v in zip(nets[0] + nets[1], W2 + b2):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(E.train_dy(10296, 4, seed=3), E.train_dy(10296, 4, seed=3))
    np.testing.assert_array_equal(E.train_dy(77, 35, seed=1), E.train_dy(77, 35, seed=1))
    dy = E.train_dy(500, 27, seed=2, nnz=None)
    assert np.all(dy[::5] == 0) and np.any(np.abs(dy) > 2048) and np.any(np.abs(dy) == 1)
    dy = E.train_dy(65536, 4)
    assert np.count_nonzero(np.any(dy != 0, 1)) <= E.DY_NNZ + 2 and np.any(dy[-1] != 0) and np.any(dy[0] != 0)
    assert [len(W2), W2[0].shape, W2[7].shape, W2[L_N + 5].shape, W2[L_N + 10].shape] == [26, (256, 288), (256, 144), (256, 319), (128, 283)]
