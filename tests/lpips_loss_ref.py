"""Checker for the LPIPS loss (pnrf_lpips_loss_fwd): the batched definition of include/pronerf_hip.h restated with torch on the CPU on the tables and
nets of tests/lpips_ref.py, differentiable by autograd.  float64 is the yardstick; float32 shows what the same formulas cost in straightforward
single precision (the bound of tests/test_lpips_loss_gpu.py).

The gradient is discontinuous where a pre-activation crosses 0 or two pooling candidates tie, so a (net, shape, seed) is only compared on the
device when ``margins`` says it is admissible (``admissible``): the float32 and float64 runs must sit on the same side of every kink with room
for a third summation order.  CASES is the table of the admissible ones, asserted by tests/test_lpips_loss_cpu.py.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref as R

MARGIN = 8.0
# (net, H, W, seeds of lpips_ref.make_pair('mix', H, W, seed)): B = 1 runs the first seed, B = 3 the first three (cycled where there are fewer).
# Seeds 0 .. 15 were tried in order with this file's restatement (one image at a time, as ``margins`` runs it); the table keeps those that pass both
# conditions with a ratio of 10 or more, at most three per shape.  Not in it, because a ratio is below 8 here: vgg 17 x 23 seed 0 (ReLU 7.5),
# vgg 33 x 20 seed 1 (ReLU 3.7), alex 31 x 31 seeds 0 (pooling 2.9) and 1 (ReLU 4.7), alex 47 x 35 seeds 0 (pooling 7.4) and 2 (ReLU 5.1).
CASES = [('vgg', 16, 16, (0, 1, 7)), ('vgg', 17, 23, (1,)), ('vgg', 33, 20, (3,)),
         ('alex', 31, 31, (2, 3, 5)), ('alex', 31, 39, (0, 2, 3)), ('alex', 47, 35, (1, 3, 4))]
NO_NORMALIZE = ('alex', 31, 31, (0,))                 # the case run with normalize=False (ReLU 151, pooling 163)


def make_batch(H, W, seeds):
    """(pred, gt) [B,H,W,3] float32 arrays: patch i is make_pair('mix', H, W, seeds[i])."""
    pairs = [R.make_pair('mix', H, W, s) for s in seeds]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def batch_seeds(seeds, B):
    return tuple(seeds[i % len(seeds)] for i in range(B))


def forward(net, w, pred, gt, normalize=True, dtype=torch.float64, taps=True):
    """pred, gt: [B,H,W,3] tensors of ``dtype`` (pred may require a gradient).  -> (value: 0-d float64 tensor = sum over the taps of the mean over
    patches and pixels, [five tap means], [pre-activation z_l of the pred half, NCHW], [(window, pooling input of the pred half)])."""
    B = pred.shape[0]
    x = torch.cat([pred, gt], 0)
    if normalize:
        x = 2 * x - 1
    x = ((x - torch.tensor(R.SHIFT, dtype=dtype)) / torch.tensor(R.SCALE, dtype=dtype)).permute(0, 3, 1, 2)
    zs, pools, means = [], [], []
    for i, (_, _, k, stride, pad, pool, tap) in enumerate(R.TABLES[net]):
        if pool:
            pools.append((pool, x[:B]))
            x = F.max_pool2d(x, pool, 2)
        z = F.conv2d(x, w['W'][i].to(dtype), w['b'][i].to(dtype), stride=stride, padding=pad)
        zs.append(z[:B])
        x = F.relu(z)
        if tap >= 0 and taps:
            fa, fb = x[:B], x[B:]
            na = fa / (torch.sqrt((fa ** 2).sum(1, keepdim=True)) + R.dtype_eps(dtype))
            nb = fb / (torch.sqrt((fb ** 2).sum(1, keepdim=True)) + R.dtype_eps(dtype))
            means.append((w['lin'][tap].to(dtype)[None, :, None, None] * (na - nb) ** 2).sum(1).double().mean())
    return sum(means), means, zs, pools


def run(net, w, pred, gt, normalize=True, dtype=torch.float64):
    """-> (value float, gradient [B,H,W,3] tensor of ``dtype``, [z_l], [(window, pooling input)]) of the batch (numpy [B,H,W,3] arrays)."""
    p = torch.as_tensor(np.asarray(pred)).to(dtype).requires_grad_(True)
    value, _, zs, pools = forward(net, w, p, torch.as_tensor(np.asarray(gt)).to(dtype), normalize, dtype)
    value.backward()
    return float(value.detach()), p.grad.detach(), [z.detach() for z in zs], [(k, a.detach()) for k, a in pools]


def activations(net, w, img, normalize=True, dtype=torch.float64):
    """([pre-activation z_l], [(window, pooling input)]) of ONE [H,W,3] image, NCHW with a batch of one, without autograd."""
    with torch.no_grad():
        _, _, zs, pools = forward(net, w, torch.as_tensor(np.asarray(img)).to(dtype)[None], torch.zeros(0, *np.shape(img), dtype=dtype), normalize, dtype, taps=False)
    return zs, pools


def margins(net, w, pred, gt, normalize=True):
    """The margin check of one batch, patch by patch on the pred half.  -> dict: 'relu' = min over patches and layers of
    min |z64| / max |z32 - z64|; 'masks' = the float32 and float64 ReLU masks agree everywhere; 'pool' = min over patches and poolings of (smallest
    gap between the two largest values of a window with a positive maximum) / (max float32 error of that pooling's input) (inf without such a
    window); 'e32' = relative L2 error of the float32 gradient of the batch; v64, g64 = float64 value and gradient."""
    v64, g64, _, _ = run(net, w, pred, gt, normalize, torch.float64)
    _, g32, _, _ = run(net, w, pred, gt, normalize, torch.float32)
    relu, masks, pool = float('inf'), True, float('inf')
    for img in pred:
        z64, p64 = activations(net, w, img, normalize, torch.float64)
        z32, p32 = activations(net, w, img, normalize, torch.float32)
        for a, b in zip(z64, z32):
            err = float((b.double() - a).abs().max())
            relu = min(relu, float(a.abs().min()) / max(err, 1e-300))
            masks = masks and bool(((a > 0) == (b > 0)).all())
        for (k, a), (_, b) in zip(p64, p32):
            err = float((b.double() - a).abs().max())
            top = a.unfold(2, k, 2).unfold(3, k, 2).reshape(*a.shape[:2], -1, k * k).topk(2, dim=-1).values
            live = top[..., 0] > 0
            if bool(live.any()):
                pool = min(pool, float((top[..., 0] - top[..., 1])[live].min()) / max(err, 1e-300))
    e32 = float((g32.double() - g64).norm() / g64.norm())
    return {'relu': relu, 'masks': masks, 'pool': pool, 'e32': e32, 'v64': v64, 'g64': g64}


def admissible(m):
    return m['relu'] >= MARGIN and m['masks'] and m['pool'] > MARGIN


@functools.lru_cache(maxsize=None)
def case(net, H, W, seeds, normalize=True):
    """(pred, gt, margins dict) of one batch with the seeded net 0 — computed once, shared, never written to."""
    pred, gt = make_batch(H, W, seeds)
    return pred, gt, margins(net, R.cached_net(net), pred, gt, normalize)
