"""torch.autograd face of the trainer's forward / backward split: train the three networks with a loss written in torch.

``render_train`` runs ``Trainer.forward`` and returns its maps as the outputs of one ``torch.autograd.Function``; ``loss.backward()`` on
anything computed from them runs ``Trainer.backward`` with the cotangents autograd hands over, which leaves the gradients of the 26 layers
in the trainer — ``Trainer.adam_step`` (or ``dist.allreduce_gradients`` first) goes on from there as after ``Trainer.fwd_bwd``.  The
parameters live in the trainer, not in torch, so the graph hangs on ``trainer.anchor``, a zero-dim leaf that only exists to require a
gradient.  No arithmetic happens here: a cotangent is made a contiguous float32 tensor of its map's shape and passed on.

    maps = render_train(tr, rays, or_rays, img4, poses, K, ref_nos, jitter=j, raw_noise=nz)
    loss = ((maps['rgb_map1'] - target) ** 2).mean() + 0.1 * ((1 - maps['acc']) ** 2).mean()
    loss.backward(); tr.adam_step(lr)

One forward is good for one backward (the activations are the trainer's own buffers): a second backward through the same graph, or one
after any other trainer call, raises ``PnrfError`` with the library's PNRF_E_STATE message.  No second-order gradients, and none with
respect to rays or images.

``ssim`` is the mean img2ssim of image patches as a differentiable scalar (``ops.ssim_loss``: value and gradient from one kernel pair), for
a structural term in such a loss when the batch is made of patches (the stage-2 driver's ``patch_size``).  ``lpips`` is the mean LPIPS of such
patches in the same mould (``ops.Lpips.loss``), the perceptual term of the stage-2 driver's ``--a_p``.
"""
from __future__ import annotations

import torch

from ._lib import PnrfError


class _RenderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, trainer, names, args, kwargs):
        maps = trainer.forward(*args, want=names, **kwargs)
        ctx.trainer, ctx.names = trainer, names
        ctx.shapes = [tuple(maps[k].shape) for k in names]
        ctx.set_materialize_grads(False)                 # a map the loss does not use arrives as None, and reaches the library as NULL
        return tuple(maps[k] for k in names)

    @staticmethod
    def backward(ctx, *grads):
        cot = {}
        for k, shape, g in zip(ctx.names, ctx.shapes, grads):
            if g is None:
                continue
            if tuple(g.shape) != shape:
                raise PnrfError(f'render_train: the cotangent of {k} has shape {tuple(g.shape)}, the map {shape}')
            cot[k] = g.detach().to(torch.float32).contiguous()
        if not cot:
            raise PnrfError('render_train: backward without a cotangent for any map')
        ctx.trainer.backward(**cot)
        return None, None, None, None, None              # nothing flows to the anchor or the data; the gradients are in the trainer


class _Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, kwargs):
        from . import ops
        mean, d_pred = ops.ssim_loss(pred, gt, **kwargs)
        ctx.save_for_backward(d_pred)                    # the kernel pair leaves the gradient with the value: backward has nothing to launch but a product
        return mean.to(torch.float32)

    @staticmethod
    def backward(ctx, grad):
        d_pred, = ctx.saved_tensors
        return grad * d_pred, None, None                 # no gradient with respect to gt


def ssim(pred, gt, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """Mean SSIM of [B,H,W,3] or [H,W,3] patches (``ops.ssim_loss``) as a float32 scalar, differentiable with respect to ``pred`` — for a loss
    such as ``mse + lam * (1 - ssim(pred, gt))``.  The gradient is computed with the value and kept; backward is one multiply by the incoming
    gradient, without a host sync.  ``gt`` gets none; no second-order gradients."""
    return _Ssim.apply(pred, gt, dict(max_val=max_val, filter_size=filter_size, filter_sigma=filter_sigma, k1=k1, k2=k2))


class _Lpips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, lp, normalize):
        value, d_pred = lp.loss(pred, gt, normalize=normalize)
        ctx.save_for_backward(d_pred)                    # value and gradient come from one call: backward has nothing to launch but a product
        return value.to(torch.float32)

    @staticmethod
    def backward(ctx, grad):
        d_pred, = ctx.saved_tensors
        return grad * d_pred, None, None, None           # no gradient with respect to gt


def lpips(pred, gt, lp, normalize=True):
    """Mean LPIPS of [B,H,W,3] or [H,W,3] patches under the ``ops.Lpips`` handle ``lp`` (``Lpips.loss``) as a float32 scalar, differentiable
    with respect to ``pred`` — for a loss such as ``mse + a_p * lpips(pred, gt, lp)``.  The gradient is computed with the value and kept;
    backward is one multiply by the incoming gradient, without a host sync.  ``gt`` gets none; no second-order gradients."""
    return _Lpips.apply(pred, gt, lp, bool(normalize))


def render_train(trainer, rays, or_rays, img4, poses, K, ref_nos, jitter=None, jitter_dir=1, raw_noise=None, white_bkgd=False, eps=1e-5, clamp=0.0,
                 layout=0, want=None):
    """``Trainer.forward`` with the same arguments -> the same dict of maps, differentiable: ``backward()`` of a loss formed from them runs
    ``Trainer.backward``."""
    names = tuple(trainer.MAPS) if want is None else tuple(want)
    out = _RenderTrain.apply(trainer.anchor, trainer, names, (rays, or_rays, img4, poses, K, ref_nos),
                             dict(jitter=jitter, jitter_dir=jitter_dir, raw_noise=raw_noise, white_bkgd=white_bkgd, eps=eps, clamp=clamp, layout=layout))
    return dict(zip(names, out))
