"""CPU: the integer nets of tests/exact_nets.py are exact for every configuration tests/test_exact_stages_gpu.py runs — integer operands
representable in the operand type, partial sums below 2^24, ELU pre-activations >= 0, the refine packer's log2(e) scaling inverted
exactly, refine logits sensitive enough that a slip of 1 cannot hide under the comparison's tolerance — and the generators are
deterministic."""
import numpy as np
import pytest

import exact_nets as E

N_NERF = max(E.nerf_counts(E.CU_CERT))
N_REFINE_BIG = max(E.refine_counts(E.CU_CERT))
N_REFINE = max(E.refine_counts(E.CU_CERT, big=False))


@pytest.mark.parametrize('depth', E.NERF_DEPTHS)
def test_nerf_certificate(depth):
    E.certify_nerf('nerf', E.nerf_net(depth), E.nerf_inputs(N_NERF))


def test_nerfcls_certificate():
    E.certify_nerf('nerfcls', E.nerfcls_net(), E.nerf_inputs(N_NERF))


@pytest.mark.parametrize('live', [0, 1, 2])
def test_live_sincos_certificate(live):
    """Nets whose sin / cos columns of one coordinate carry weight, on inputs where that coordinate is 0 (the extra GPU calls)."""
    inp = E.nerf_inputs(N_NERF, live=live)
    assert (inp['pts'][..., live] == 0).all() and (inp['rays'][:, 8 + live] == 0).all()
    for kind, w in (('nerf', E.nerf_net(8, live=live)), ('nerf', E.nerf_net(3 + live, live=live)), ('nerfcls', E.nerfcls_net(live=live))):
        W0 = w['W'][0] if kind == 'nerf' else w['pts_linears'][0][0]
        assert np.any(W0[:, E.pe_cols(live, E.MULTIRES)] != 0)          # the sin / cos columns really carry weight
        E.certify_nerf(kind, w, inp)


@pytest.mark.parametrize('S,n', [(8, 33), (16, 33), (64, 33)])
def test_train_inputs_certificate(S, n):
    inp = E.nerf_inputs(n, n_samples=S)
    E.certify_nerf('nerf', E.nerf_net(8), inp)
    E.certify_nerf('nerfcls', E.nerfcls_net(), inp)


@pytest.mark.parametrize('nb,depth', E.REFINE_CONFIGS)
def test_refine_certificate_and_margin(nb, depth):
    n = N_REFINE_BIG if (nb, depth) == E.REFINE_BIG else N_REFINE
    net = E.refine_net(nb, depth)
    x = E.elu_inputs(n, 48 + 24 * nb)
    y = E.certify_elu(net, x, E.LIM['bf16'])
    rays, ds = E.refine_rays(n)
    assert E.assert_refine_margin(y, rays, ds) > E.MARGIN * E.TOL_Z
    # the packer's scaling (first layer and ELU biases x log2(e), output layer / log2(e), double -> float) lands on the integers exactly
    Wp, bp = E.refine_pack_weights(net)
    L = len(Wp)
    for l in range(L):
        ws = E.LOG2E if l == 0 else (1.0 / E.LOG2E if l == L - 1 else 1.0)
        bsc = E.LOG2E if l < L - 1 else 1.0
        np.testing.assert_array_equal((Wp[l].astype(np.float64) * ws).astype(np.float32), net['W'][l])
        np.testing.assert_array_equal((bp[l].astype(np.float64) * bsc).astype(np.float32), net['b'][l])


def test_refine_module_level_counts():
    """pnrf_mlp_fwd on refine nets: every configuration at the module-level row counts."""
    for nb, depth in E.REFINE_CONFIGS:
        E.certify_elu(E.refine_net(nb, depth), E.elu_inputs(max(E.MLP_COUNTS), 48 + 24 * nb), E.LIM['bf16'])


def test_sampler_certificate():
    E.certify_elu(E.sampler_net(), E.elu_inputs(max(E.MLP_COUNTS), 288), E.LIM['f32'])


def test_nerf_module_level_certificate():
    inp = E.nerf_inputs(max(E.MLP_COUNTS), n_samples=1)
    E.certify_nerf('nerf', E.nerf_net(8), inp)
    E.certify_nerf('nerfcls', E.nerfcls_net(), inp)


def test_margin_detects_a_slip():
    """The margin is what a slip of one in a logit does: shifting one logit by 1 moves z by at least the computed margin."""
    net = E.refine_net(4, 6)
    x = E.elu_inputs(64, 144)
    y = E.elu_reference(net, x)
    rays, ds = E.refine_rays(64)
    m = E.refine_margin(y, rays, ds)
    y1 = y.copy(); y1[5, 3] += 1
    dz = np.abs(E.refine_reference(y1, rays, ds)[0] - E.refine_reference(y, rays, ds)[0]).max()
    assert dz >= m > E.MARGIN * E.TOL_Z


def test_generators_deterministic():
    a, b = E.nerf_net(5, live=1), E.nerf_net(5, live=1)
    for x, y in zip(a['W'] + a['b'], b['W'] + b['b']):
        np.testing.assert_array_equal(x, y)
    c1, c2 = E.nerfcls_net(), E.nerfcls_net()
    for W1, W2 in zip(E.nerfcls_pack_order(c1)[0] + E.nerfcls_pack_order(c1)[1], E.nerfcls_pack_order(c2)[0] + E.nerfcls_pack_order(c2)[1]):
        np.testing.assert_array_equal(W1, W2)
    r1, r2 = E.refine_net(3, 3), E.refine_net(3, 3)
    for x, y in zip(r1['W'] + r1['b'], r2['W'] + r2['b']):
        np.testing.assert_array_equal(x, y)
    for k, v in E.nerf_inputs(40, live=2).items():
        np.testing.assert_array_equal(v, E.nerf_inputs(40, live=2)[k])
    np.testing.assert_array_equal(E.elu_inputs(9, 144), E.elu_inputs(9, 144))
    np.testing.assert_array_equal(E.refine_rays(9)[1], E.refine_rays(9)[1])
