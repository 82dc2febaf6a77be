"""Skip connections inside the sampler / refine stacks (``--mmnetskips``): what the tests compare against (a plain helper module of the suite).

* ``skip_backbone`` restates the reference's backbone (run_nerf_helpers.py:1490-1497, 1526-1533 of the reference) in torch: behind backbone layer i of
  the skip set the net input is concatenated back, ``h = cat([x, h])``.  The skip set is read off the weights' shapes.  ``with skip_oracle():`` puts it in
  place of the oracle's no-skip backbone, so the oracle's own stage functions (``render_rays_infer``, ``sampler_forward``, ``refine_forward``) run on it.
* Integer skip nets with exact answers, in the manner of tests/exact_nets.py (whose certificate ``check_layer``, head generator and refine reference
  are used by import): weights, biases and inputs are small integers, every ELU pre-activation is >= 0 for every input in the box (interval bounds,
  bias lifted to the lower bound), every partial sum stays below 2^24.  The x-columns of every skip layer carry non-zero weights, so an x fragment read
  from the wrong place gives a wrong integer.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

import exact_nets as en
from oracle import pronerf_oracle as orc
from oracle import synth

# golden name -> (mmnetskips, what it is); tools/gen_golden_mmskips.py writes them from the reference
CASES = {
    'infer_skip_d8_s4_p48_nb4_16x20': (4,),
    'infer_skip_d3_s01_p8_nb1_16x20': (0, 1),
    'infer_skip_d5_s3_p32_nb7_16x20': (3,),
}
TIE = 1e-6


def skips_of(Ws):
    """Skip set of a stack from its shapes: Linear i + 1 with in_ch + 256 columns = a skip behind backbone layer i."""
    in_ch = Ws[0].shape[1]
    return [i - 1 for i in range(1, len(Ws) - 1) if Ws[i].shape[1] == in_ch + Ws[i].shape[0]]


def skip_backbone(x, Ws, bs):
    sk = skips_of(Ws)
    h = x
    for i, (W, b) in enumerate(zip(Ws[:-1], bs[:-1])):
        h = F.elu(orc._lin(h, W, b))
        if i in sk:
            h = torch.cat([x, h], -1)
    return orc._lin(h, Ws[-1], bs[-1])


@contextlib.contextmanager
def skip_oracle():
    keep = orc.mlp_elu_backbone
    orc.mlp_elu_backbone = skip_backbone
    try:
        yield
    finally:
        orc.mlp_elu_backbone = keep


def case(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name + '.npz')))
    shape = dict(n_pts=int(g['n_pts']), mmnetdepth=int(g['mmnetdepth']), num_neighbor=int(g['num_neighbor']), netdepth=int(g['netdepth']), mmnetskips=CASES[name])
    scene = synth.make_scene(int(g['seed']), H=int(g['H']), W=int(g['W']), Hf=int(g['Hf']), Wf=int(g['Wf']), rotate=bool(g['rotate']),
                             sigma_t=float(g['sigma_t']), n_views=int(g['n_views']))
    return g, shape, scene, synth.make_weights(int(g['seed']), str(g['kind']), **shape)


def render_ref(w, fr, n_pts):
    with skip_oracle(), torch.no_grad():
        return orc.render_rays_infer(w, fr['rays'], fr['or_rays'], fr['images'], fr['proj'], n_pts=n_pts)


# ----------------------------------------------------------------------------------------------- integer skip nets
SKIP_SETS = {2: ([0],), 3: ([0], [1], [0, 1]), 6: ([0], [4], [0, 4], [1, 2])}      # D -> skip sets: [0], [D-2], [0, D-2], [1, 2] where they exist


def _int_stack(rs, in_ch, D, skips, head, live_cols=None, scaled=False):
    """in_ch -> D x 256 (ELU on its identity branch) -> head.  Inputs in [0, 2].  Hidden row r reads unit perm[r] (+1: every unit is read), half of the
    rows minus another unit; rows r % 4 == 0 of a skip layer also read x[c] - x[d] (+ x[e] on some).  Interval bounds per unit; bias = -lower bound + 0..2 (scaled: lifted further to an integer that has a float32 pre-image under the packer's log2(e) scale)."""
    cols = np.arange(in_ch) if live_cols is None else np.asarray(live_cols)
    lo_x, hi_x = np.zeros(in_ch), np.full(in_ch, 2.0)
    Ws, bs = [], []
    lo, hi = lo_x, hi_x
    for l in range(D):
        fi = in_ch if l == 0 else 256
        W = np.zeros((256, fi + (in_ch if (l - 1) in skips and l >= 1 else 0)))
        off = W.shape[1] - fi                      # x-columns come first in a skip layer
        src = cols if l == 0 else np.arange(fi)
        perm = rs.permutation(np.tile(src, 256 // len(src) + 1))[:256]
        for r in range(256):
            W[r, off + perm[r]] += 1
            if l > 0 and rs.rand() < 0.5:
                W[r, off + rs.choice(np.delete(src, np.flatnonzero(src == perm[r])))] -= 1
            if off and r % 4 == 0:
                c, d, e = rs.choice(cols, 3, replace=False)
                W[r, c] += 1; W[r, d] -= 1
                if rs.rand() < 0.5:
                    W[r, e] += 2
        lo_in = np.concatenate([lo_x, lo]) if off else lo
        hi_in = np.concatenate([hi_x, hi]) if off else hi
        l0 = np.where(W > 0, W * lo_in, W * hi_in).sum(1); h0 = np.where(W > 0, W * hi_in, W * lo_in).sum(1)
        b = -l0 + rs.randint(0, 3, 256)
        if scaled:                                 # (a bias that no float32 / log2(e) reproduces: lift it, as exact_nets does)
            for r in range(256):
                while not en._has_pre_image(b[r], en.LOG2E):
                    b[r] += 1
        Ws.append(W); bs.append(b.astype(np.float64))
        lo, hi = l0 + b, h0 + b
    W, b = head(rs, lo, hi, (hi - lo) <= 4)
    Ws.append(W); bs.append(b)
    return {'W': Ws, 'b': bs}


def refine_net(nb, D, skips, seed=0):
    """Integer refine skip net on the kernels' log2(e) scale (exact_nets' module docstring), logits bounded like exact_nets.refine_net's."""
    rs = np.random.RandomState(7001 * nb + 97 * D + 13 * sum(2 ** s for s in skips) + seed)
    return _int_stack(rs, 48 + 24 * nb, D, skips, en._refine_head, scaled=True)


def refine_pack_weights(net):
    """exact_nets.refine_pack_weights, with the x-columns of the skip layers taken through the first layer's pre-image (the packer scales them alike)."""
    W, b = en.refine_pack_weights(net)
    in_ch = net['W'][0].shape[1]
    for i in skips_of(net['W']):
        W[i + 1] = np.concatenate([en._pre_image(net['W'][i + 1][:, :in_ch], en.LOG2E), np.asarray(net['W'][i + 1][:, in_ch:], np.float32)], 1)
    return W, b


SAMPLER_P = 3           # ray points of the integer sampler nets: the fold sums three column blocks
SAMPLER_PERM = np.array([5, 2, 7, 0, 3, 6, 1, 4])


def sampler_net(D, skips, seed=0):
    """Integer sampler skip net for the exact-fp32 kernel (true scale).  Its input is the ray's Pluecker 6-vector repeated over the P ray points; the rays
    of ``sampler_rays`` make that vector (0, 0, 1, b, -a, 0) with integers a <= 0 <= b: columns 2, 3, 4 of every block are live.  The depth rows of the
    head carry no weights and a spread, permuted bias — the sort order is SAMPLER_PERM's for every ray — while add / mul read the last hidden layer."""
    rs = np.random.RandomState(6007 + 89 * D + 11 * sum(2 ** s for s in skips) + seed)
    live = [6 * p + c for p in range(SAMPLER_P) for c in (2, 3, 4)]

    def head(rs, lo, hi, narrow):
        W = np.zeros((27, 256)); b = np.zeros(27)
        b[:8] = (np.arange(8) - 4.0)[SAMPLER_PERM]
        W[8:] = en._hidden(rs, 19, 256) * rs.choice((1, 2, 3), (19, 1)); b[8:] = rs.randint(-5, 6, 19)
        return W, b
    return _int_stack(rs, 6 * SAMPLER_P, D, skips, head, live_cols=live)


def sampler_scaled_net(D, skips, seed=0):
    """Integer sampler skip net ON THE log2(e) SCALE of the split-fp16 and pass-1 streams, for a placement test that survives the scale.  No weight of
    those streams is an integer in general: the packer multiplies first-layer-like weights and ELU biases by log2(e) and splits them into two fp16
    planes.  Here the fp32 weights handed to the packer are PRE-IMAGES (``sampler_pack_weights``): the stored hi plane of every first-layer-like weight,
    every bias and every output weight is exactly the integer of this net, the lo plane holds the pre-image's residual (<= 2^-24 relative).  On integer
    inputs every accumulator is then an integer plus at most a few 1e-6, every fp16-packed activation of pass 1 the integer itself, and add / mul come
    out within 1e-3 of the integers (SCALED_TOL) — while one x fragment, plane or k-step read from the wrong place moves some hidden unit by >= 1, and
    the head (every last-layer unit read by exactly one add / mul row with weight +-1) carries that to an output.  One ray point (the fold over P is
    the packer's, shared by the three streams, and is exercised by ``sampler_net``)."""
    rs = np.random.RandomState(6151 + 83 * D + 7 * sum(2 ** s for s in skips) + seed)

    def head(rs, lo, hi, narrow):
        W = np.zeros((27, 256)); b = np.zeros(27)
        b[:8] = (np.arange(8) - 4.0)[SAMPLER_PERM]
        W[8:24] = en._dense(rs, 16, 256, (-1, 1)); b[8:24] = rs.randint(-5, 6, 16)
        return W, b
    return _int_stack(rs, 6, D, skips, head, live_cols=[2, 3, 4], scaled=True)


SCALED_TOL = 1e-3       # |add, mul - exact integer| on the scaled streams: lo-plane residuals 2^-24 x (|value| <= 2048) x fan-in <= 3 per layer, <= 6 layers: < 4e-4


def sampler_pack_weights(net):
    """fp32 weights for pnrf_mlp_pack whose log2(e)-scaled streams hold exactly the integers of a ``sampler_scaled_net`` in their hi planes."""
    return refine_pack_weights(net)


def sampler_rays(n, seed=0):
    """rays [n, 11]: o = (a, b, c) with integers a in [-2, 0], b in [0, 2], d = (0, 0, 1): unit direction (0, 0, 1), moment (b, -a, 0), exactly."""
    rs = np.random.RandomState(911 + seed)
    o = np.stack([-rs.randint(0, 3, n), rs.randint(0, 3, n), rs.randint(-2, 3, n)], 1)
    d = np.tile([0.0, 0.0, 1.0], (n, 1))
    return np.concatenate([o, d, np.zeros((n, 1)), np.ones((n, 1)), d], 1).astype(np.float32)


def sampler_inputs(rays, n_pts=SAMPLER_P):
    o = rays[:, :3].astype(np.float64)
    x6 = np.stack([0 * o[:, 0], 0 * o[:, 0], 1 + 0 * o[:, 0], o[:, 1], -o[:, 0], 0 * o[:, 0]], 1)
    return np.tile(x6, (1, n_pts))


def exact_forward(net, x, lim):
    """The exact answer y [n, out] (float64) of an integer skip net, every layer certified by exact_nets.check_layer (operands representable below
    ``lim``, ELU pre-activations >= 0, partial sums below 2^24), and equal to ``skip_backbone`` in float64."""
    x = np.asarray(x, np.float64)
    sk = skips_of(net['W'])
    h, L = x, len(net['W'])
    for l in range(L):
        h = en.check_layer(h, net['W'][l], net['b'][l], lim, f'layer {l}', elu=l < L - 1)
        if l in sk:
            h = np.concatenate([x, h], 1)
    ref = skip_backbone(torch.from_numpy(x), [torch.from_numpy(np.asarray(W, np.float64)) for W in net['W']],
                        [torch.from_numpy(np.asarray(b, np.float64)) for b in net['b']]).numpy()
    np.testing.assert_array_equal(h, ref)
    return h
