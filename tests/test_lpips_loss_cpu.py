"""CPU: the float64 restatement of the LPIPS loss (tests/lpips_loss_ref.py) is held to the metric's restatement and to central differences of its own
value, and every case of tests/test_lpips_loss_gpu.py is checked to lie clear of the gradient's kinks.  These tests qualify the reference, not the
kernels."""
import numpy as np
import pytest
import torch

import lpips_loss_ref as L
import lpips_ref as R

BATCHES = [(net, H, W, L.batch_seeds(seeds, B), True) for net, H, W, seeds in L.CASES for B in (1, 3)] + \
          [(L.NO_NORMALIZE[0], L.NO_NORMALIZE[1], L.NO_NORMALIZE[2], L.NO_NORMALIZE[3], False)]


@pytest.mark.parametrize('net,H,W', [('alex', 31, 39), ('vgg', 17, 23)])
def test_one_patch_has_the_value_of_the_metric_restatement(net, H, W):
    """B = 1: the same formulas on a batch of two images instead of two batches of one: float64 sums of at most 4608 terms in another order at
    the most, 1e-12 relative with a wide margin."""
    w = R.cached_net(net)
    a, b = R.make_pair('mix', H, W, 1)
    want, _ = R.lpips_ref(net, w, a, b)
    got, means, _, _ = L.forward(net, w, torch.tensor(a).double()[None], torch.tensor(b).double()[None])
    assert abs(float(got) - want) <= 1e-12 * want and len(means) == 5
    v3, _, _, _ = L.forward(net, w, torch.tensor(np.stack([a, b, a])).double(), torch.tensor(np.stack([b, a, a])).double())
    assert abs(float(v3) - 2 * want / 3) <= 1e-12 * want                        # the mean over the patches; d(a, a) = 0


@pytest.mark.parametrize('net,H,W,seeds', [('alex', 31, 31, (2, 3)), ('vgg', 16, 16, (0, 1))])
def test_gradient_agrees_with_central_differences(net, H, W, seeds):
    """A handful of coordinates per net; step 1e-6 in float64: the truncation error is O(h^2) = 1e-12 relative to the curvature and the rounding
    error about 1e-16 |value| / h = 1e-10 |value|; the case's margins keep a step of that size on one side of every kink."""
    w = R.cached_net(net)
    pred, gt = L.make_batch(H, W, seeds)
    _, g, _, _ = L.run(net, w, pred, gt)
    gt64 = torch.tensor(gt).double()
    rs = np.random.RandomState(7)
    h = 1e-6
    scale = float(g.abs().max())
    for _ in range(6):
        i = (rs.randint(len(seeds)), rs.randint(H), rs.randint(W), rs.randint(3))
        vals = []
        for sgn in (1, -1):
            p = torch.tensor(pred).double()
            p[i] += sgn * h
            vals.append(float(L.forward(net, w, p, gt64)[0]))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - float(g[i])) <= 1e-6 * scale + 1e-9, (i, fd, float(g[i]))


@pytest.mark.parametrize('net,H,W,seeds,normalize', BATCHES, ids=[f'{b[0]}-{b[1]}x{b[2]}-{"".join(map(str, b[3]))}{"" if b[4] else "-raw"}' for b in BATCHES])
def test_every_gpu_case_is_clear_of_the_kinks(net, H, W, seeds, normalize):
    _, _, m = L.case(net, H, W, seeds, normalize)
    print(f'\n[lpips loss margins] {net} {H}x{W} seeds {seeds} normalize={normalize}: ReLU ratio {m["relu"]:.1f}, pooling ratio {m["pool"]:.1f}, '
          f'masks equal {m["masks"]}, float32 gradient error {m["e32"]:.2e}')
    assert L.admissible(m), m
    assert 0 < m['e32'] < 1e-5
