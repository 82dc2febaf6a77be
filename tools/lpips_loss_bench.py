#!/usr/bin/env python
"""What an LPIPS term costs the stage-2 iteration at 4096 rays (workloads.TrainWorkload), and pnrf_lpips_loss_fwd alone.

The call alone: ops.Lpips.loss (value + gradient) on 4 x (32 x 32), 16 x (16 x 16) (vgg only) and 1 x (64 x 64) patches, device ms per call from
two events around back-to-back calls; beside it the same definition in float32 eager torch on the same GPU (tests/lpips_loss_ref.forward:
conv2d / max_pool2d, then autograd's backward), twice (`eager_again`: eager against itself).  Seeded weights (tests/lpips_ref.make_net).

Inside the iteration, the protocol of tools/ssim_loss_bench.py — device events around `--iters` back-to-back iterations including Adam behind
`--warm` untimed ones, the variants alternating in ONE process, the median over `--rounds` rounds — per net:

    mse         Trainer.forward -> torch mse(rgb_map1) -> .backward() (Trainer.backward) + adam_step      (the baseline; twice: `mse_again`
                                                                                                            gives the A/A spread)
    eager       ... + a_p x LPIPS in eager torch, float32, with torch's autograd
    kernel      ... + a_p x autograd.lpips(...)

Reported per variant: median and range of the ms per iteration and the kernel launches per iteration (torch.profiler); `added_ms`:
eager - mse and kernel - mse, to be read against `a_a_spread_ms`.  `--call NET BxS`: only back-to-back calls of that shape (for a kernel trace).

    python tools/lpips_loss_bench.py --out profiles/lpips_loss.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--patch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--a_p', type=float, default=0.1)
    ap.add_argument('--call', nargs=2, metavar=('NET', 'BxS'), default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('lpips_loss_bench: needs a GPU (a CPU run measures nothing)')
    import lpips_loss_ref
    import lpips_ref
    from train_split_bench import launches_per_iteration
    from pronerf_amd import autograd, ops
    from pronerf_amd.workloads import TrainWorkload, timed_ms
    dev = torch.device('cuda:0')
    nets = {}
    for net in ('alex', 'vgg'):
        w = lpips_ref.cached_net(net)
        nets[net] = (ops.Lpips(net, *lpips_ref.state_dicts(net, w), device=dev), {k: [t.to(dev) for t in v] for k, v in w.items()})

    def eager(net, pred, gt):
        with torch.device(dev):
            return lpips_loss_ref.forward(net, nets[net][1], pred, gt, True, torch.float32)[0]

    def eager_call(net, a, b):
        def fn():
            p = a.detach().requires_grad_(True)
            eager(net, p, b).backward()
            return p.grad
        return fn

    def pair(B, side):
        g = torch.Generator(device=dev).manual_seed(B)
        return torch.rand(B, side, side, 3, device=dev, generator=g), torch.rand(B, side, side, 3, device=dev, generator=g)

    if args.call:
        net, (B, side) = args.call[0], (int(x) for x in args.call[1].split('x'))
        a, b = pair(B, side)
        ms = timed_ms(lambda: nets[net][0].loss(a, b), 200, 50)[0]
        print(json.dumps({'net': net, 'B': B, 'side': side, 'ms': ms}))
        return

    stat = lambda v: {'ms_median': float(np.median(v)), 'ms_min': float(min(v)), 'ms_max': float(max(v))}
    alone = {}
    for net in ('alex', 'vgg'):
        for B, side in ((4, 32), (16, 16), (1, 64)):
            if side < ops.LPIPS_MIN[net]:
                continue
            a, b = pair(B, side)
            fns = {'kernel': lambda: nets[net][0].loss(a, b), 'eager': eager_call(net, a, b), 'eager_again': eager_call(net, a, b)}
            ms = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    ms[k].append(timed_ms(fn, 100, 20)[0])
            p = a.detach().requires_grad_(True)
            eager(net, p, b).backward()
            got = nets[net][0].loss(a, b)[1]
            alone[f'{net} {B}x{side}x{side}'] = {**{k: stat(v) for k, v in ms.items()}, 'launches': {k: launches_per_iteration(fns[k]) for k in ('kernel', 'eager')},
                                               'gradient_rel_l2_kernel_vs_eager': float((got - p.grad).norm() / p.grad.norm())}

    wl = TrainWorkload(n_rays=args.rays)
    tr = wl.trainer
    head, tail = wl.batch_args()[:2], wl.batch_args()[3:]
    P = args.patch
    if wl.n % (P * P):
        raise SystemExit(f'lpips_loss_bench: {wl.n} rays are not whole {P} x {P} patches')
    shape = (wl.n // (P * P), P, P, 3)
    gt = wl.target.reshape(shape)

    def iteration(extra):
        def fn():
            maps = autograd.render_train(tr, *head, *tail, jitter=wl.jitter, jitter_dir=1, raw_noise=wl.noise, want=('rgb_map1',))
            rgb = maps['rgb_map1']
            loss = ((rgb - wl.target) ** 2).mean()
            if extra is not None:
                loss = loss + args.a_p * extra(rgb.reshape(shape))
            loss.backward()
            tr.adam_step(5e-4, weight_decay=5e-8)
        return fn

    res = {'what': f'stage-2 iteration at {wl.n} rays = {shape[0]} patches of {P} x {P} with loss mse + {args.a_p} LPIPS, device ms per iteration (two events around '
                   f'{args.iters} back-to-back iterations including Adam behind {args.warm} untimed ones), {args.rounds} rounds with the variants alternating in '
                   f'one process; call_alone: value + gradient per call, 100 back-to-back calls behind 20 untimed ones, {args.rounds} rounds',
           'device': torch.cuda.get_device_name(0), 'call_alone': alone, 'iteration': {}}
    for net in ('alex', 'vgg'):
        variants = {'mse': iteration(None), 'mse_again': iteration(None), 'eager': iteration(lambda p: eager(net, p, gt)),
                    'kernel': iteration(lambda p: autograd.lpips(p, gt, nets[net][0]))}
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed_ms(fn, args.iters, args.warm)[0])
        r = {'variants': {k: {**stat(v), 'ms_rounds': [round(x, 4) for x in v]} for k, v in ms.items()}}
        for k, fn in variants.items():
            if k != 'mse_again':
                r['variants'][k]['launches'] = launches_per_iteration(fn)
        med = lambda k: r['variants'][k]['ms_median']
        r['a_a_spread_ms'] = abs(med('mse') - med('mse_again'))
        r['added_ms'] = {k: med(k) - med('mse') for k in ('eager', 'kernel')}
        res['iteration'][net] = r
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == '__main__':
    main()
