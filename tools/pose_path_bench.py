"""Times the pose-to-frame path at the frame size (756 x 1008, 20 source views, 4 neighbours) on one GPU: the three kernels a target pose costs with a
device-resident scene (neighbour selection, texel gather, rays; device events), and a whole pose — host wall time until the frame is finished, and
device time — three ways: today's ``set_views`` + ``frame_rays`` + ``render_rays``, ``render_pose`` eager, and the replay of one captured graph.
Every pose of a round is a different camera, so nothing is cached between calls.  Writes one JSON document.

    python tools/pose_path_bench.py [--out profiles/pose_path_756x1008.json] [--poses 24] [--reps 200]      (--out: that path by default)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pronerf_amd import ops, synthetic  # noqa: E402
from pronerf_amd.render import Renderer  # noqa: E402

H, W, NV = 756, 1008, 20


def device_ms(fn, reps, warmup=10, windows=5):
    """Mean milliseconds of fn() over ``reps`` back-to-back calls between two events, after a warm-up; ``windows`` windows -> (median, min, max)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return {'median': float(np.median(out)), 'min': min(out), 'max': max(out)}


def stats(v):
    v = [float(x) for x in v]
    return {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'p10': float(np.percentile(v, 10)), 'p90': float(np.percentile(v, 90)), 'n': len(v)}


def per_pose(fn, poses, rounds=3):
    """fn(c2w) renders one pose and returns without synchronising.  Per pose: host wall time from the call to the finished frame (the call + one
    synchronisation) and device time between two events around the call; the first round is the warm-up."""
    wall, devms = [], []
    for r in range(rounds + 1):
        for c2w in poses:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            t0.record()
            fn(c2w)
            t1.record()
            torch.cuda.synchronize()
            if r:
                wall.append((time.perf_counter() - t) * 1e3)
                devms.append(t0.elapsed_time(t1))
    return {'host_wall_ms': stats(wall), 'device_ms': stats(devms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_path_756x1008.json'))
    ap.add_argument('--poses', type=int, default=24)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    scene = synthetic.make_scene(0, H=H, W=W, n_views=NV, sigma_t=0.3)
    rs = np.random.RandomState(1)
    poses = []
    for _ in range(args.poses):                                   # targets spread over the rig: the neighbour sets change from pose to pose
        p = np.eye(3, 4, dtype=np.float32)
        p[:, 3] = (rs.randn(3) * 0.3).astype(np.float32)
        poses.append(p)
    rend = Renderer(synthetic.make_weights(0, 'trained'), max_rays=H * W, device=dev)
    nb = rend.num_neighbor
    res = {'frame': [H, W], 'source_views': NV, 'neighbours': nb, 'device': torch.cuda.get_device_name(0), 'poses': args.poses, 'reps': args.reps}

    t = time.perf_counter()
    sc = rend.set_scene(scene['poses'], scene['images'], scene['K'])
    torch.cuda.synchronize()
    res['scene_upload_ms_once'] = (time.perf_counter() - t) * 1e3
    res['scene_cache_bytes'] = NV * H * W * 16

    # ---- the three kernels of a pose
    c2w_d = torch.from_numpy(poses[0]).to(dev)
    ref = torch.empty(nb, device=dev, dtype=torch.int32); proj = torch.empty(nb, 3, 4, device=dev); img4 = torch.empty(nb, H, W, 4, device=dev)
    rays = torch.empty(H * W, 11, device=dev); orr = torch.empty(H * W, 11, device=dev)
    from pronerf_amd import _lib
    lib = _lib.load()
    st = lambda: torch.cuda.current_stream().cuda_stream
    select = lambda: _lib.check(lib.pnrf_scene_select_fwd(sc.handle, c2w_d.data_ptr(), nb, ref.data_ptr(), proj.data_ptr(), img4.data_ptr(), st()), 'select')
    raysf = lambda: _lib.check(lib.pnrf_frame_rays_dev_fwd(sc.K.data_ptr(), c2w_d.data_ptr(), H, W, 0.0, 1.0, 1.0, 10.0, 0, H * W, 0, H * W, rays.data_ptr(),
                                                           orr.data_ptr(), st()), 'rays')
    one = ops.Scene.from_views(scene['poses'], np.zeros((NV, 2, 2, 3), np.uint8), scene['K'], cache='u8', device=dev)      # same ranking, a 64-byte gather
    img_small = torch.empty(nb, 2, 2, 4, device=dev)
    rank = lambda: _lib.check(lib.pnrf_scene_select_fwd(one.handle, c2w_d.data_ptr(), nb, ref.data_ptr(), proj.data_ptr(), img_small.data_ptr(), st()), 'rank')
    # the gather has no entry point of its own: it is timed as the full-size call minus the same call on 2 x 2-pixel views (same ranking and
    # projection, a 64-byte gather), window by window with the two calls alternating, so the spread of the difference is a measured one
    pairs = [(device_ms(select, args.reps, windows=1)['median'], device_ms(rank, args.reps, windows=1)['median']) for _ in range(7)]
    full, small = [a for a, _ in pairs], [b for _, b in pairs]
    mmm = lambda v: {'median': float(np.median(v)), 'min': min(v), 'max': max(v)}
    res['select_and_gather_ms'] = mmm(full)
    res['ranking_and_projection_ms'] = mmm(small)                          # with its 2 x 2-pixel gather: two launches, the floor of the pair
    res['gather_ms'] = mmm([a - b for a, b in pairs])
    res['gather_bytes'] = 2 * nb * H * W * 16
    res['rays_dev_ms'] = device_ms(raysf, args.reps)
    res['rays_host_pointer_ms'] = device_ms(lambda: ops.frame_rays(scene['K'], poses[0], H, W, device=dev), args.reps)
    res['render_rays_ms'] = device_ms(lambda: rend.ctx.render_rays(rays, orr, img4, proj), max(20, args.reps // 4))

    # ---- a whole pose, three ways
    out = torch.empty(H * W, 4, device=dev)

    def today(c2w):
        rend.set_views(c2w, scene['poses'], scene['images'], scene['K'])
        r, o = rend.frame_rays(scene['K'], c2w, H, W)
        rend.render_rays(r, o, out=out)

    res['today_set_views_frame_rays_render_rays'] = per_pose(today, poses)
    res['render_pose_eager'] = per_pose(lambda c2w: rend.render_pose(c2w, H, W, out=out), poses)
    g = rend.capture_pose(H, W)
    res['graph_replay'] = per_pose(lambda c2w: g.replay(c2w), poses)
    # the frames agree: same pose through the three paths (today's differs by the ulp of the projection matrices)
    today(poses[3]); a = out.clone()
    b = rend.render_pose(poses[3], H, W).clone()
    c = g.replay(poses[3]).clone()
    res['eager_equals_replay_bitwise'] = bool(torch.equal(b, c))
    res['today_vs_render_pose_max_abs_rgb'] = float((a[:, :3] - b[:, :3]).abs().max())
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
