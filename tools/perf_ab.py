#!/usr/bin/env python3
"""Interleaved A/B timing of library builds and kernel variants in ONE process (cdna guide §5.4 rule 24).

    python tools/perf_ab.py [--rounds 7] [--frames 10] --configs "lib=;lib=head;lib=,sampler=sampler_split;lib=,nerf=bf16_32x32"

A config selects a library build (lib=<name> -> pronerf_amd/lib/libpronerf_hip_<name>.so, empty = the default build; see
`python -m pronerf_amd.build --variant <name> [flags]`) and the kernel variants of its handles (pnrf_mlp_set_variant: sampler=
default (two passes) | sampler_split | sampler_f32 | sampler_f32_full, refine= default (fp16) | bf16 | refine_16x16, nerf= default (fp16) | bf16 | bf16_32x32 | nerf_4x64) — explicit configuration, the library reads no environment.  shape=wide|narrow|single forces the workgroup shape of all three
stages (pnrf_mlp_set_shape).  skip=never|auto|always sets the NeRF stage's compacted-column path (pnrf_ctx_set_nerf_skip; a library without the entry point
takes no skip=).  --weights picks the nets: a kind of synthetic.make_weights or a trained fixture ('pictures' | 'scene3d'), on the same frame.  Naming one
config twice (lib=parent;lib=parent;lib=) gives the A/B's own spread: the difference between two identical configs, printed as 'pair spread'.
Every round renders `--frames` frames per config through pnrf_render_rays_fwd with the context's per-kernel events
(pnrf_ctx_profile_begin / _end); reports median / min over the rounds per stage kernel on the bench workload (one 1008x756 frame).
path=ops times the operator-level sequence instead (sampler, refine_input, refine on refine_in, NeRF: four kernels with the [n,144]
intermediate in HBM), frames back to back with torch events per stage."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pronerf_amd import _lib, ops, synthetic    # noqa: E402
from pronerf_amd.render import Renderer         # noqa: E402

H, W = 756, 1008


def load_lib(name):
    path = _lib.LIB_PATH if not name else os.path.join(os.path.dirname(_lib.LIB_PATH), f'libpronerf_hip_{name}.so')
    lib = C.CDLL(path)
    for fn, (res, args) in _lib.SIGNATURES.items():
        f = getattr(lib, fn, None)            # an older build under comparison may lack the newest entry points
        if f is not None:
            f.restype = res; f.argtypes = args
    if getattr(lib, 'pnrf_mlp_skips', None) is None:      # a build from before skip connections holds no skip nets: report none (ops.PackedMLP asks every handle)
        def no_skips(handle, mask):
            mask._obj.value = 0
            return 0
        lib.pnrf_mlp_skips = no_skips
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--weights', default='trained')
    ap.add_argument('--configs', default='lib=;lib=,sampler=sampler_split;lib=,nerf=bf16_32x32')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    weights = synthetic.load_trained_fixture(a.weights) if a.weights in synthetic.FIXTURES else synthetic.make_weights(0, a.weights)
    scene = synthetic.make_scene(0, H=H, W=W, focal=815.13, rotate=True)
    cfgs = [dict(kv.split('=') for kv in c.split(',') if kv) for c in a.configs.split(';')]
    libs, rends = {}, []
    for c in cfgs:
        n = c.get('lib', '')
        if n not in libs:
            libs[n] = load_lib(n)
        _lib._lib = libs[n]
        var = {k: v for k, v in (('sampler', c.get('sampler', 'default')), ('refine', c.get('refine', 'default')), ('nerf', c.get('nerf', 'default'))) if v != 'default'}
        r = Renderer(weights, max_rays=H * W, device=dev, variants=var, shape=(c.get('shape') or None))
        r.set_views(scene['c2w'], scene['poses'], scene['images'], scene['K'])
        if c.get('skip'):
            r.ctx.set_nerf_skip(c['skip'])
        rends.append(r)
    _lib._lib = libs[cfgs[0].get('lib', '')]
    rays, or_rays = rends[0].frame_rays(scene['K'], scene['c2w'], H, W)
    res = [dict() for _ in cfgs]
    for r in range(a.rounds + 1):
        for i, c in enumerate(cfgs):
            _lib._lib = libs[c.get('lib', '')]
            rend = rends[i]
            if c.get('path') == 'ops':
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(a.frames)]
                for e in ev:
                    e[0].record()
                    depth, _, add, mul, _, _ = ops.sampler_fwd(rend.sampler, rays, want_idx=False, want_rgb=False)
                    e[1].record()
                    rin = ops.refine_input(rays, or_rays, depth, rend.img4, rend.proj)
                    e[2].record()
                    z, pts = ops.refine_fwd(rend.refine, rin, rays, depth)
                    e[3].record()
                    ops.nerf_fwd(rend.nerf, pts, rays, z, add, mul)
                    e[4].record()
                torch.cuda.synchronize()
                names = ('sampler_kernel', 'refine_input_kernel', 'refine_kernel', 'nerf_kernel')
                ms = {k: sum(e[i].elapsed_time(e[i + 1]) for e in ev) / a.frames for i, k in enumerate(names)}
            else:
                rend.ctx.profile_begin(a.frames)
                for _ in range(a.frames):
                    rend.render_rays(rays, or_rays)
                ms, _ = rend.ctx.profile_end()
                torch.cuda.synchronize()
            if r == 0:
                continue
            for k, v in ms.items():
                res[i].setdefault(k, []).append(v)
            res[i].setdefault('frame', []).append(sum(ms.values()))
    for i, c in enumerate(cfgs):
        line = ' '.join(f'{k}={statistics.median(v):.3f}/{min(v):.3f}' for k, v in res[i].items())
        live = ''
        if hasattr(libs[c.get('lib', '')], 'pnrf_ctx_nerf_live'):
            _lib._lib = libs[c.get('lib', '')]
            n_live, list_mode = rends[i].ctx.nerf_live()
            live = f'  live columns {n_live} of {H * W * 8}, list mode {list_mode}'
        print(f'{a.weights} {c}: median/min ms  {line}{live}')
    # identical configs: the spread of the comparison itself (largest difference of their medians and of their per-round values)
    for i, c in enumerate(cfgs):
        for j in range(i + 1, len(cfgs)):
            if cfgs[j] == c:
                for k in ('nerf_kernel', 'frame'):
                    d = [x - y for x, y in zip(res[i][k], res[j][k])]
                    print(f'{a.weights} pair spread {k}: medians differ by {abs(statistics.median(res[i][k]) - statistics.median(res[j][k])):.4f} ms, '
                          f'rounds by {min(d):+.4f} .. {max(d):+.4f} ms')


if __name__ == '__main__':
    main()
