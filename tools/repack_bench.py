#!/usr/bin/env python
"""Trainer -> renderable nets: today's way round the host against the device repack, in ONE process, the paths alternating, five repeats each.

    (a) host:     state_dicts_from_trainer (26 layers read back) + three ops.PackedMLP(...) (host packer, new handles, uploads);
                  host wall time, a synchronise before and after
    (b) publish:  Trainer.publish into existing handles (pnrf_trainer_publish -> pnrf_mlp_repack); device events and synchronised wall time
    (c) one 756 x 1008 hold-out view through evaluate_views(path='train') and through path='render' (synchronised wall time; the first
        'render' call, which builds the kept Renderer and its scene, is timed apart as render_first)

All raw times go into the JSON; (b) has to lie below (a) in every repeat on the same box.

    python tools/repack_bench.py --out profiles/repack.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--H', type=int, default=756)
    ap.add_argument('--W', type=int, default=1008)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    from pronerf_amd import ops, synthetic
    from pronerf_amd.run_S_eS_eN_alter_base_refine2 import _FINE_KEYS, _MM_KEYS, evaluate_views, state_dicts_from_trainer
    from pronerf_amd.workloads import TrainWorkload
    H, W = args.H, args.W
    wl = TrainWorkload(n_rays=1024, H=H, W=W, n_views=args.views)
    tr = wl.trainer
    for _ in range(2):                                       # the weights have moved off their initial values
        wl.stage2_step()

    def host_path():
        sds = state_dicts_from_trainer(tr)
        return [ops.PackedMLP(net, [sd[k + '.weight'] for k in keys], [sd[k + '.bias'] for k in keys])
                for net, sd, keys in zip((ops.NET_SAMPLER, ops.NET_REFINE, ops.NET_NERFCLS), sds, (_MM_KEYS, _MM_KEYS, _FINE_KEYS))]

    handles = host_path()
    tr.publish(*handles)                                     # the warm call: builds the three plans
    torch.cuda.synchronize()
    same = [h.serialize() for h in handles] == [h.serialize() for h in host_path()]

    scene = synthetic.make_scene(0, H=H, W=W, n_views=args.views, sigma_t=0.2, rotate=True)
    test, train = [0], list(range(1, args.views))
    ev = (tr, 2, scene['poses'][test], scene['images'][test], scene['images'][train], scene['poses'][train], scene['K'], H, W)
    render_first, psnr_render = wall_ms(lambda: evaluate_views(*ev, path='render'))
    _, psnr_train = wall_ms(lambda: evaluate_views(*ev, path='train'))

    rows = []
    for _ in range(args.repeats):
        a, _h = wall_ms(host_path)
        del _h
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(); tr.publish(*handles); e1.record()
        submitted = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        b_wall = (time.perf_counter() - t0) * 1e3
        c_train, _ = wall_ms(lambda: evaluate_views(*ev, path='train'))
        c_render, _ = wall_ms(lambda: evaluate_views(*ev, path='render'))
        rows.append({'host_ms': a, 'publish_device_ms': e0.elapsed_time(e1), 'publish_submit_ms': submitted, 'publish_wall_ms': b_wall,
                     'view_train_ms': c_train, 'view_render_ms': c_render})
    res = {'what': __doc__.split('\n\n')[1], 'device': torch.cuda.get_device_name(0), 'frame': [H, W], 'training_views': len(train), 'repeats': rows,
           'publish_equals_host_pack_bytes': same, 'view_render_first_ms': render_first, 'psnr_train_path': psnr_train, 'psnr_render_path': psnr_render,
           'publish_below_host_in_every_repeat': all(r['publish_wall_ms'] < r['host_ms'] for r in rows),
           'median': {k: float(np.median([r[k] for r in rows])) for k in rows[0]}}
    print(json.dumps(res['median']), 'publish below host in every repeat:', res['publish_below_host_in_every_repeat'])
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    return 0 if res['publish_below_host_in_every_repeat'] and same else 1


if __name__ == '__main__':
    sys.exit(main())
