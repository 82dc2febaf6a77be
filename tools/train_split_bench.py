#!/usr/bin/env python
"""Stage-2 iteration at 4096 rays (workloads.TrainWorkload): the fused call against the forward / backward split around a torch loss.

    fused:  Trainer.fwd_bwd + adam_step                                   (TrainWorkload.stage2_step)
    split:  Trainer.forward -> torch mse(rgb_map1) cotangent -> Trainer.backward + adam_step

Both variants run in ONE process on one trainer, alternating in rounds (a round = `--iters` back-to-back iterations behind `--warm` untimed
ones, timed with two device events), so that clock drift hits both alike.  Reported per variant: the median and the range over the rounds of
the device milliseconds per iteration, and the number of kernel launches per iteration (counted with torch.profiler's device activity;
null if the profiler is not available).

`--lib PATH --fused-only` times another build's library (e.g. one built from the parent commit): the fused variant twice, as `fused` and
`fused_again`, alternating — the A/A spread a difference between two builds has to be read against.  That library need not export the
split's entry points.

    python tools/train_split_bench.py --out profiles/train_split_loss.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPLIT_SYMBOLS = ('pnrf_composite_bwd_maps', 'pnrf_train_stage2_fwd', 'pnrf_train_stage2_bwd')


def launches_per_iteration(fn, n=3):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        copies = len(prof.events()) - len(kernels)
        return {'kernels': len(kernels) / n, 'copies_and_memsets': copies / n}
    except Exception as e:                                       # noqa: BLE001 — a diagnostic: the timings do not depend on it
        return {'kernels': None, 'error': f'{type(e).__name__}: {e}'}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', default=None, help='time this libpronerf_hip.so instead of the package\'s own')
    ap.add_argument('--fused-only', action='store_true', help='the fused variant twice (A/A); for a library without the split entry points')
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    from pronerf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.fused_only:
        for k in SPLIT_SYMBOLS:
            _lib.SIGNATURES.pop(k, None)
    from pronerf_amd.workloads import TrainWorkload, timed_ms
    wl = TrainWorkload(n_rays=args.rays)
    tr = wl.trainer
    head, tail = wl.batch_args()[:2], wl.batch_args()[3:]
    inv = 2.0 / (3 * wl.n)

    def fused():
        wl.stage2_step()

    def split():
        maps = tr.forward(*head, *tail, jitter=wl.jitter, jitter_dir=1, raw_noise=wl.noise, want=('rgb_map1',))
        tr.backward(rgb_map1=(maps['rgb_map1'] - wl.target) * inv)
        tr.adam_step(5e-4, weight_decay=5e-8)

    def split_all_maps():                                        # every map copied out, a depth + opacity loss: three cotangents
        maps = tr.forward(*head, *tail, jitter=wl.jitter, jitter_dir=1, raw_noise=wl.noise)
        tr.backward(rgb_map1=(maps['rgb_map1'] - wl.target) * inv, acc=(maps['acc'] - 1) * (0.2 / wl.n), depth=torch.full_like(maps['depth'], 0.01 / wl.n))
        tr.adam_step(5e-4, weight_decay=5e-8)
    variants = {'fused': fused, 'fused_again': fused} if args.fused_only else {'fused': fused, 'split': split, 'split_all_maps': split_all_maps}
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed_ms(fn, args.iters, args.warm)[0])
    res = {'what': f'stage-2 iteration at {wl.n} rays, device ms per iteration (two events around {args.iters} back-to-back iterations behind {args.warm} '
                   f'untimed ones), {args.rounds} rounds with the variants alternating in one process',
           'library': _lib.LIB_PATH if args.lib else 'the package\'s own', 'device': torch.cuda.get_device_name(0), 'variants': {}}
    for k, v in ms.items():
        res['variants'][k] = {'ms_median': float(np.median(v)), 'ms_min': float(min(v)), 'ms_max': float(max(v)), 'ms_rounds': [round(x, 4) for x in v]}
    for k, fn in variants.items():
        if k != 'fused_again':
            res['variants'][k]['launches'] = launches_per_iteration(fn)
    if args.fused_only:
        a, b = res['variants']['fused']['ms_median'], res['variants']['fused_again']['ms_median']
        res['a_a_spread_ms'] = abs(a - b)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == '__main__':
    main()
