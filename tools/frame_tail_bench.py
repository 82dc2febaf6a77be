"""Times the frame tail at the frame size (756 x 1008) on one GPU: ops.image_metrics and ops.frame_to8b (device events), the same SSIM in
eager torch (conv2d with the separable filter) on the same GPU, the host tail render_path runs per pose by default (three fp32 planes to
the host, PSNR through eager torch, to8b and depth / max in numpy) against the device tail, and the wall time of a 3-pose render_path with
the two switches off and on.  Writes one JSON document.

    python tools/frame_tail_bench.py [--out profiles/<name>.json] [--reps 200] [--no-render-path]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pronerf_amd import ops, synthetic  # noqa: E402
from pronerf_amd import run_nerf_helpers as h  # noqa: E402

H, W = 756, 1008


def device_ms(fn, reps, warmup=10):
    """Mean milliseconds of fn() over ``reps`` back-to-back calls between two events, after a warm-up; three windows -> (median, min, max)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return {'median': sorted(out)[1], 'min': min(out), 'max': max(out)}


def host_ms(fn, reps):
    """Host wall milliseconds of fn() (which ends synchronised), median / min / max over ``reps`` calls after two warm-up calls."""
    fn(); fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {'median': float(np.median(out)), 'min': min(out), 'max': max(out)}


def torch_ssim(a, b, taps, max_val=1.0, k1=0.01, k2=0.03):
    """img2ssim in eager torch on the device: [H,W,3] -> five planes per image pair through two 1-D conv2d passes."""
    T = taps.numel()
    x = torch.stack([a, b, a * a, b * b, a * b], 0).permute(0, 3, 1, 2).reshape(15, 1, a.shape[0], a.shape[1])
    x = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, taps.flip(0).view(1, 1, T, 1)), taps.flip(0).view(1, 1, 1, T)).reshape(5, 3, a.shape[0] - T + 1, -1)
    mu0, mu1 = x[0], x[1]
    s00, s11, s01 = (x[2] - mu0 * mu0).clamp_min(0), (x[3] - mu1 * mu1).clamp_min(0), x[4] - mu0 * mu1
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return (((2 * mu0 * mu1 + c1) * (2 * s01 + c2)) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--no-render-path', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([0.5 + 0.4 * np.sin(xx / (17.0 + 5 * c) + yy / (23.0 - 4 * c)) for c in range(3)], -1).astype(np.float32)
    rgbd = torch.empty(H * W, 4, device=dev)
    rgbd[:, :3] = torch.tensor(np.clip(img + 0.02 * rs.randn(H, W, 3), 0, 1).astype(np.float32), device=dev).reshape(-1, 3)
    rgbd[:, 3] = torch.tensor(rs.uniform(0.1, 1.0, H * W).astype(np.float32), device=dev)
    rgb, depth = rgbd[:, :3].reshape(H, W, 3), rgbd[:, 3].reshape(H, W)
    gt_host = img
    gt = torch.tensor(gt_host, device=dev)
    taps = torch.tensor(ops.ssim_filter(11, 1.5), dtype=torch.float32, device=dev)
    res = {'frame': [H, W], 'device': torch.cuda.get_device_name(0), 'reps': args.reps}

    res['image_metrics_ms'] = device_ms(lambda: ops.image_metrics(rgb, gt), args.reps)
    res['frame_to8b_ms'] = device_ms(lambda: ops.frame_to8b(rgb, depth), args.reps)
    res['torch_ssim_ms'] = device_ms(lambda: torch_ssim(rgb, gt, taps), max(10, args.reps // 10))
    res['torch_psnr_ms'] = device_ms(lambda: h.mse2psnr(h.img2mse(rgb, gt)), args.reps)
    m = ops.image_metrics(rgb, gt).cpu()
    res['ssim_kernel'], res['ssim_torch'], res['psnr_kernel'], res['psnr_torch'] = float(m[3]), float(torch_ssim(rgb, gt, taps)), float(h.mse2psnr(m[1])), float(h.mse2psnr(h.img2mse(rgb, gt)))
    # bytes the two calls have to move at least: both images once (the renderer's rows are 16 bytes per pixel, the ground truth 12), resp. the rows once + 4 bytes per pixel out
    res['image_metrics_min_bytes'], res['frame_to8b_min_bytes'] = H * W * 28, H * W * 20

    def host_tail():       # the default statements of render_path after the timed renders
        a, b, d = rgb.cpu().numpy(), rgb.cpu().numpy(), depth.cpu().numpy()
        p = float(h.mse2psnr(h.img2mse(rgb, torch.as_tensor(gt_host, dtype=torch.float32).to(dev))))
        return h.to8b(b), h.to8b(d / np.max(d)), a, p

    def device_tail():     # the same with pnrf_metrics + pnrf_device_to8b (the float arrays still travel: render_path returns them)
        a, b, d = rgb.cpu().numpy(), rgb.cpu().numpy(), depth.cpu().numpy()
        m = ops.image_metrics(rgb, torch.as_tensor(gt_host, dtype=torch.float32).to(dev)).cpu()
        planes = [torch.empty(t.shape, dtype=torch.uint8).pin_memory().copy_(t, non_blocking=True) for t in ops.frame_to8b(rgb, depth)]
        torch.cuda.current_stream().synchronize()
        return planes[0].numpy(), planes[1].numpy(), a, float(h.mse2psnr(m[1])), float(m[3])

    def host_tail_8bit_only():
        return h.to8b(rgb.cpu().numpy()), h.to8b((lambda d: d / np.max(d))(depth.cpu().numpy()))

    res['host_tail_ms'] = host_ms(host_tail, 20)
    res['device_tail_ms'] = host_ms(device_tail, 20)
    res['host_to8b_with_copies_ms'] = host_ms(host_tail_8bit_only, 20)
    x, y = host_tail(), device_tail()
    res['tails_agree'] = bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and abs(x[3] - y[3]) < 1e-4)

    if not args.no_render_path:
        from types import SimpleNamespace
        from pronerf_amd import run_S_eS_eN_alter_trt as trt
        a = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256, mmnetskips=[10000],
                            N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)
        kw, _ = trt.create_nerf(a, device=dev)
        sd = synthetic.state_dicts(synthetic.make_weights(0, 'trained'))
        kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
        scene = synthetic.make_scene(0, H=H, W=W, n_views=6)
        kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
        targets = [scene['c2w'], scene['poses'][0], scene['poses'][1]]
        gts = [gt_host] * 3
        walls = {'off': [], 'on': []}
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            for rep in range(4):                                  # alternating; the first pair is the warm-up
                for name, opts in (('off', {}), ('on', {'pnrf_metrics': True, 'pnrf_device_to8b': True})):
                    k = {**kw, **opts}
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    trt.render_path(targets, (H, W, scene['focal']), scene['K'], None, k, gt_imgs=gts, savedir=os.path.join(tmp, name), n_timing_reps=1, verbose=False)
                    if rep:
                        walls[name].append((time.perf_counter() - t) * 1e3)
        res['render_path_3_poses_wall_ms'] = {n: {'median': float(np.median(v)), 'min': min(v), 'max': max(v)} for n, v in walls.items()}
        res['render_path_note'] = 'one render per pose, PNGs written (zlib on a worker thread); switches off = the statements of the parent commit'
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
