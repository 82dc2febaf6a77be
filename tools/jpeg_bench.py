"""Measures the JPEG encoder and the Motion-JPEG path and writes profiles/jpeg_encode.json.

    python tools/jpeg_bench.py [--out profiles/jpeg_encode.json] [--cpu-only] [--no-spiral]

Host part (any machine; ``--cpu-only`` refreshes it alone and keeps the device sections of an existing file): on the ``llff_synth.Scene3D`` views
at 189 x 252 and 378 x 504 (RGB and depth) at quality 50 / 75 / 90 / 95 the host twin's file against PIL's (``quality=q, subsampling=0,
optimize=False, restart_marker_rows=1``): sizes, PSNR against the source of PIL's decode of both files, the ratio to the device-PNG file.
``margins``: d = the worst PSNR shortfall against PIL's file in dB (0 if none), m = the worst relative size excess (0 if none); tests/test_jpeg_cpu.py
reads them.

Device part (one GPU) at 756 x 1008 on the planes of a ray-cast Scene3D view, five repeats after a warm-up: device events around
``pnrf_jpeg_encode_fwd``; wall time of ``JpegEncoder.encode_to_host``; PIL's host encode of the same plane in the same repeats; and the 120-pose
spiral of the synthetic scene as frames per second of wall time, ``Renderer.render_video`` against ``render_path`` with ``pnrf_device_png``,
``pnrf_scene_cache='f32'`` and ``n_timing_reps=1``."""
from __future__ import annotations

import argparse
import io
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import png_ref  # noqa: E402
from pronerf_amd import ops  # noqa: E402

REPEATS = 5
QUALITIES = (50, 75, 90, 95)
VIEWS = ((189, 252), (378, 504))


def pil_encode(img, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=quality, subsampling=0, optimize=False, restart_marker_rows=1)
    return b.getvalue()


def pil_psnr(data, img):
    from PIL import Image
    dec = np.asarray(Image.open(io.BytesIO(data))).astype(np.float64)
    mse = np.mean((dec - img) ** 2)
    return float('inf') if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def compare(img, quality):
    """(our bytes, PIL's bytes, our PSNR, PIL's PSNR) of one image: the measurement the margins and the test share."""
    ours, pil = ops.jpeg_encode_host(img, quality), pil_encode(img, quality)
    return ours, pil, pil_psnr(ours, img), pil_psnr(pil, img)


def host_part():
    rows, d, m = [], 0.0, 0.0
    for H, W in VIEWS:
        for name, img in zip(('rgb', 'depth'), png_ref.scene_views(H, W)):
            png = len(ops.png_encode_host(img))
            for q in QUALITIES:
                ours, pil, p_ours, p_pil = compare(img, q)
                d, m = max(d, p_pil - p_ours), max(m, len(ours) / len(pil) - 1)
                rows.append({'view': [H, W], 'plane': name, 'quality': q, 'file_bytes': len(ours), 'pil_file_bytes': len(pil), 'file_over_pil': round(len(ours) / len(pil), 4),
                             'psnr_db': round(p_ours, 4), 'pil_psnr_db': round(p_pil, 4), 'device_png_bytes': png, 'file_over_device_png': round(len(ours) / png, 4)})
    up = lambda x: math.ceil(max(x, 0.0) * 1e4) / 1e4
    return {'d': up(d), 'm': up(m), 'pil': 'quality=q, subsampling=0, optimize=False, restart_marker_rows=1', 'cases': rows}


def device_part(spiral=True):
    import torch
    from pronerf_amd import run_nerf_helpers as h
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    from pronerf_amd import synthetic
    H, W = 756, 1008
    dev = torch.device('cuda:0')
    res = {'frame': [H, W], 'device': torch.cuda.get_device_name(0), 'repeats': REPEATS, 'quality': 90}
    for name, plane_h in zip(('rgb', 'depth'), png_ref.scene_views(H, W)):
        plane = torch.from_numpy(plane_h).to(dev)
        enc = ops.JpegEncoder(H, W, 1 if plane_h.ndim == 2 else 3, dev, 90)
        data = enc.encode_to_host(plane)                      # warm-up of both paths
        pil_encode(plane_h, 90)
        assert data == ops.jpeg_encode_host(plane_h, 90)
        ev, wall, host = [], [], []
        for _ in range(REPEATS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record(); enc.launch(plane); t1.record()
            torch.cuda.synchronize()
            ev.append(t0.elapsed_time(t1))
            t = time.perf_counter(); data = enc.encode_to_host(plane); wall.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); pil = pil_encode(plane_h, 90); host.append((time.perf_counter() - t) * 1e3)
        res[name] = {'encode_fwd_device_ms': ev, 'encode_to_host_wall_ms': wall, 'pil_host_encode_wall_ms': host, 'device_file_bytes': len(data), 'pil_file_bytes': len(pil),
                     'max_bytes': enc.max_bytes, 'device_png_bytes': len(ops.png_encode_host(plane_h)),
                     'device_below_pil_in_every_repeat': bool(all(a < b for a, b in zip(wall, host)))}
    if spiral:
        from types import SimpleNamespace
        a = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256, mmnetskips=[10000],
                            N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)
        kw, _ = trt.create_nerf(a, device=dev)
        sd = synthetic.state_dicts(synthetic.make_weights(0, 'trained'))
        kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
        scene = synthetic.make_scene(0, H=H, W=W, n_views=6)
        kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
        c2w = np.asarray(scene['c2w'], np.float32)[:3, :4]
        poses = []
        for k in range(120):                                  # a small circle around the scene's target pose
            p = c2w.copy()
            p[:, 3] += 0.05 * (math.cos(2 * math.pi * k / 120) * p[:, 0] + math.sin(2 * math.pi * k / 120) * p[:, 1])
            poses.append(p)
        rend = trt._renderer(kw['min_max_ray_net'], kw['refine_net'], kw['network_fine'], H * W, dev)
        fps = {'render_path_device_png': [], 'render_video': []}
        sizes = {}
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            for rep in range(REPEATS + 1):                    # alternating; the first pair is the warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                trt.render_path(poses, (H, W, scene['focal']), scene['K'], None, {**kw, 'pnrf_device_png': True, 'pnrf_scene_cache': 'f32'}, savedir=os.path.join(tmp, 'png'),
                                n_timing_reps=1, verbose=False)
                if rep:
                    fps['render_path_device_png'].append(len(poses) / (time.perf_counter() - t))
                sizes['render_path_device_png'] = sum(os.path.getsize(os.path.join(tmp, 'png', f)) for f in os.listdir(os.path.join(tmp, 'png')))
                torch.cuda.synchronize()
                t = time.perf_counter()
                rend.set_scene(scene['poses'], scene['images'], scene['K'], scene['K'])
                rend.render_video(poses, H, W, os.path.join(tmp, 'video.avi'), depth_path=os.path.join(tmp, 'video_depth.avi'))
                if rep:
                    fps['render_video'].append(len(poses) / (time.perf_counter() - t))
                sizes['render_video'] = os.path.getsize(os.path.join(tmp, 'video.avi')) + os.path.getsize(os.path.join(tmp, 'video_depth.avi'))
                rend.scene = rend._pose_ws = None
        res['spiral_120_poses_frames_per_second'] = fps
        res['spiral_120_poses_bytes_on_disk'] = sizes
        res['spiral_note'] = ('both write RGB and depth of every pose and upload the source views once, inside the time; render_path also reads the float frame '
                              'back and returns it, render_video does not; render, encode, copy and file writes are not separated')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode.json'))
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--no-spiral', action='store_true')
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res['margins'] = host_part()
    if not args.cpu_only:
        import torch
        assert torch.cuda.is_available(), 'the device part needs a GPU (--cpu-only measures the host part alone)'
        res['device'] = device_part(not args.no_spiral)
    line = json.dumps(res, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
