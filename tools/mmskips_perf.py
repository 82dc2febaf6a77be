#!/usr/bin/env python3
"""Cost of a skip connection inside the sampler / refine stacks (``--mmnetskips``), interleaved in one process (a sibling of tools/perf_ab.py).

    python tools/mmskips_perf.py [--rounds 7] [--frames 10] [--depth 8] [--skips 4] [--out profiles/mmskips_frame.json]

Renders the bench frame (756 x 1008) with ``make_weights(0, 'trained', mmnetdepth=D)`` and with the same nets plus ``mmnetskips`` (the h-columns and every
other array are the same draws), alternating the two every round, through pnrf_render_rays_fwd with the context's per-kernel events; reports median / min
per stage kernel and frame.  For comparison, not as gates: the sampler's skip adds 8 tiles x 1 k-step (x 3 MFMAs where split) to the 128 of a hidden layer,
the refine net's 8 x (3 NV + 3); the stream padding of a skip layer adds 2-4 slot barriers."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pronerf_amd import synthetic    # noqa: E402
from pronerf_amd.render import Renderer         # noqa: E402

H, W = 756, 1008


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--skips', type=int, nargs='*', default=[4])
    ap.add_argument('--num_neighbor', type=int, default=4)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    scene = synthetic.make_scene(0, H=H, W=W, focal=815.13, rotate=True)
    # (name: skips, forced shape of the refine handle).  'no skip, refine narrow' prices the NARROW refine shape on a whole frame: what a skip net with
    # num_neighbor > 4, whose refine stage has no WIDE form, pays under PNRF_SHAPE_AUTO
    cfgs = {'no skip': ((), None), 'no skip, refine narrow': ((), 'narrow'), f'skips {a.skips}': (tuple(a.skips), None)}
    rends = {}
    scene = synthetic.make_scene(0, H=H, W=W, focal=815.13, rotate=True, n_views=a.num_neighbor)
    for name, (sk, shp) in cfgs.items():
        r = Renderer(synthetic.make_weights(0, 'trained', mmnetdepth=a.depth, mmnetskips=sk, num_neighbor=a.num_neighbor), max_rays=H * W, device=dev)
        if shp:
            r.refine.set_shape(shp)
        r.set_views(scene['c2w'], scene['poses'], scene['images'], scene['K'])
        rends[name] = r
    rays, or_rays = next(iter(rends.values())).frame_rays(scene['K'], scene['c2w'], H, W)
    res = {n: {} for n in cfgs}
    for rnd in range(a.rounds + 1):
        for name, rend in rends.items():
            rend.ctx.profile_begin(a.frames)
            for _ in range(a.frames):
                rend.render_rays(rays, or_rays)
            ms, _ = rend.ctx.profile_end()
            torch.cuda.synchronize()
            if rnd:
                for k, v in ms.items():
                    res[name].setdefault(k, []).append(v)
                res[name].setdefault('frame', []).append(sum(ms.values()))
    out = {'frame': [H, W], 'mmnetdepth': a.depth, 'num_neighbor': a.num_neighbor, 'rounds': a.rounds, 'frames_per_round': a.frames, 'unit': 'ms, median / min over the rounds', 'configs': {}}
    for name in cfgs:
        out['configs'][name] = {k: [round(statistics.median(v), 4), round(min(v), 4)] for k, v in res[name].items()}
        out['configs'][name]['second_pass_share'] = round(rends[name].ctx.sampler_stats() / (H * W), 4)
        print(name, ' '.join(f'{k}={m:.3f}/{lo:.3f}' for k, (m, lo) in ((k, v) for k, v in out['configs'][name].items() if isinstance(v, list))),
              f"second pass {out['configs'][name]['second_pass_share']:.1%}")
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
