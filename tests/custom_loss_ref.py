"""References for training with a caller's loss (a plain helper module of the suite): pnrf_composite_bwd_maps, pnrf_train_stage2_fwd / _bwd.

  * ``fold``: the closed-form rule that turns the cotangents of all outputs of raw2outputs into the cotangent of the weights alone, plus a term
    on z — what ``composite_bwd_body<true>`` (pnrf_train.hip) adds in front of the colour-only backward — in numpy float64.
  * ``autograd_ref``: float64 autograd over ``orc.raw2outputs`` for arbitrary cotangents (the arbiter of the operator tests).
  * ``mse_cotangent``: the cotangent losses_kernel hands to the backward pass, ((scale * 2) * (pred - target)) * fp32(1 / numel), every product
    rounded to fp32 — with it the split iteration must reproduce the fused one bit for bit.

The one place where the library deviates from autograd: a ray with acc == 0 has disp = 1 / max(1e-10, 0 / 0) = NaN and autograd propagates
NaN into every gradient of the ray; the kernel gives exact zeros from d_disp there (and on the constant branch depth / acc <= 1e-10, where
autograd gives zeros too).  ``disp_ok`` is that rule's mask; ``autograd_ref`` forms disp on those rays only.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import pronerf_oracle as orc

COT = ('rgb', 'disp', 'acc', 'w', 'depth', 'z_in')         # the six cotangents of pnrf_composite_bwd_maps (ops.composite_bwd_maps: d_rgb, d_disp, ...)


def _pad_s1(inp):
    """S = 1: the oracle composites nothing (its ``dists[..., :1]`` of an empty difference is empty); the kernels give the single sample the 1e10
    interval.  As exact_composite.reference: a second, dead sample 1e10 behind the first."""
    pad = lambda x, v: None if x is None else np.concatenate([x, np.full_like(x[:, :1], v)], 1)
    z2 = np.concatenate([inp['z'].astype(np.float64), inp['z'].astype(np.float64) + 1e10], 1)
    p = dict(inp, raw=pad(inp['raw'], 0), z=z2, add=pad(inp['add'], 0), mul=pad(inp['mul'], 0), noise=pad(inp['noise'], 0))
    p['raw'][:, 1, 3] = -1.0 if not p['clamp'] else -p['clamp']
    return p


def _leaves(inp, dtype):
    t = lambda x, rg=False: None if x is None else torch.tensor(np.asarray(x, np.float64), dtype=dtype, requires_grad=rg)
    return t(inp['raw'], True), t(inp['z'], True), t(inp['add'], True), t(inp['mul'], True), t(inp['d']), t(inp['noise'])


def forward(inp, dtype=torch.float64):
    """The oracle's raw2outputs on an exact_composite input set -> (leaves, outputs) with S = 1 padded (outputs cut back to one sample)."""
    S = inp['z'].shape[1]
    p = _pad_s1(inp) if S == 1 else inp
    raw, z, add, mul, d, noise = _leaves(p, dtype)
    rgb, disp, acc, w, depth = orc.raw2outputs(raw, z, d, add, mul, noise=noise, clamp=float(inp['clamp']), white_bkgd=bool(inp['white']))
    return dict(raw=raw, z=z, add=add, mul=mul), dict(rgb=rgb, disp=disp, acc=acc, w=w[:, :S], depth=depth), S


def disp_ok(depth, acc):
    """Rays on which d_disp counts: r = depth / acc finite and > 1e-10 (float64 arrays)."""
    with np.errstate(all='ignore'):
        r = np.asarray(depth, np.float64) / np.asarray(acc, np.float64)
    return np.isfinite(r) & (r > 1e-10)


def _grads(leaves, S):
    cut = lambda g: g.detach().numpy()[:, :S]
    out = dict(d_raw=cut(leaves['raw'].grad), d_z=cut(leaves['z'].grad))
    if S == 1:      # the kernels' last interval (1e10) does not depend on z: the padded ray's does, through z_1 - z_0 alone, so adding d z_1 removes that path
        out['d_z'] = out['d_z'] + leaves['z'].grad.detach().numpy()[:, 1:2]
    if leaves['add'] is not None:
        out['d_add'], out['d_mul'] = cut(leaves['add'].grad), cut(leaves['mul'].grad)
    return out


def autograd_ref(inp, cot, dtype=torch.float64):
    """Autograd of sum_k <cot_k, out_k> (+ <cot['z_in'], z>) through orc.raw2outputs in ``dtype``; cot: dict over COT of arrays or None.
    disp is formed from depth and acc as raw2outputs forms it, on the rays of ``disp_ok`` only.  -> dict d_raw, d_z [, d_add, d_mul]."""
    leaves, o, S = forward(inp, dtype)
    c = lambda k: None if cot.get(k) is None else torch.tensor(np.asarray(cot[k], np.float64), dtype=dtype)
    obj = 0
    for k in ('rgb', 'acc', 'w', 'depth'):
        if c(k) is not None:
            obj = obj + (c(k) * o[k]).sum()
    if c('z_in') is not None and S > 1:
        obj = obj + (c('z_in') * leaves['z']).sum()
    if c('disp') is not None:
        ok = torch.from_numpy(disp_ok(o['depth'].detach().double().numpy(), o['acc'].detach().double().numpy()))
        r = o['depth'][ok] / o['acc'][ok]
        obj = obj + (c('disp')[ok] * (1.0 / torch.max(1e-10 * torch.ones_like(r), r))).sum()
    obj.backward()
    out = _grads(leaves, S)
    if c('z_in') is not None and S == 1:
        out['d_z'] = out['d_z'] + np.asarray(cot['z_in'], np.float64)
    return out


def fold(fwd, z, cot, white):
    """The closed form (float64 numpy).  fwd: dict of the forward's depth, acc [n] (and w [n, S]); z [n, S]; cot over COT (None = zeros).
    -> (g_rgb [n, 3] unchanged, dws_extra [n, S], dz_extra [n, S]):  the cotangent of w_s is  g_rgb . c_s - [white] sum g_rgb + dws_extra[s],
    and d z_s gains dz_extra[s];  dws_extra = G_depth z_s + G_acc + g_w[s],  dz_extra = w_s G_depth + d_z_in[s]  with
    G_depth = g_depth - g_disp disp^2 / acc,  G_acc = g_acc + g_disp disp^2 depth / acc^2  on the rays of disp_ok, else g_depth, g_acc."""
    z = np.asarray(z, np.float64)
    n, S = z.shape
    g = lambda k, shape: np.zeros(shape) if cot.get(k) is None else np.asarray(cot[k], np.float64)
    depth, acc, w = (np.asarray(fwd[k], np.float64) for k in ('depth', 'acc', 'w'))
    Gd, Ga = g('depth', n).copy(), g('acc', n).copy()
    ok = disp_ok(depth, acc)
    gd = g('disp', n)
    with np.errstate(all='ignore'):
        disp = acc / depth                                       # 1 / r on the rays that count
        k = np.where(ok, gd * disp * disp / acc, 0.0)
        Gd = Gd - k
        Ga = Ga + np.where(ok, k * depth / acc, 0.0)
    dws_extra = Gd[:, None] * z + Ga[:, None] + g('w', (n, S))
    dz_extra = w * Gd[:, None] + g('z_in', (n, S))
    return g('rgb', (n, 3)), dws_extra, dz_extra


def random_cotangents(n, S, seed, names=COT):
    rs = np.random.RandomState(seed)
    shapes = dict(rgb=(n, 3), disp=(n,), acc=(n,), w=(n, S), depth=(n,), z_in=(n, S))
    return {k: (rs.randn(*shapes[k]).astype(np.float32) if k in names else None) for k in COT}


def mask_disp(cot, depth64, acc64, lo=0.05):
    """The test protocol's d_disp: zero on rays where the float64 reference has acc < lo or depth / acc < lo (disp^2 beyond 400 amplifies the
    forward's round-off without bound as acc -> 0).  -> (cot with d_disp masked, fraction of rays left out)."""
    with np.errstate(all='ignore'):
        out = (np.asarray(acc64) < lo) | ~(np.asarray(depth64) / np.asarray(acc64) >= lo)
    c = dict(cot)
    c['disp'] = np.where(out, 0, cot['disp']).astype(np.float32)
    return c, float(out.mean())


def mse_cotangent(pred, target, scale=1.0):
    """losses_kernel's d_pred = scale * 2.f * e * inv (left to right, each product rounded to fp32), e = pred - target, inv = 1.f / (float)numel.
    pred, target: float32 torch tensors (any device) -> float32 tensor on pred's device."""
    inv = np.float32(1.0) / np.float32(pred.numel())
    e = pred - target
    return ((float(np.float32(scale)) * 2.0) * e) * float(inv)
