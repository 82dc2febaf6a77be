"""Measures the PNG encoder and writes profiles/png_encode.json.

    python tools/png_bench.py [--out profiles/png_encode.json] [--cpu-only] [--no-render-path]

Host part (any machine): the size margin m of tests/test_png_cpu.py — over the ``llff_synth.Scene3D`` views at 189 x 252 and 378 x 504 (RGB clean,
RGB with sigma = 0.012 noise, depth) the largest (zlib stream of the host twin) / (reference: zlib level 6, Z_RLE, a full flush per segment, on the
same filtered bytes) - 1 — and the file sizes against the parent writer's.

Device part (one GPU), at 756 x 1008 on the RGB and depth planes of a ray-cast Scene3D view, five repeats each after a warm-up:
device events around ``pnrf_png_encode_fwd``; wall time of ``PngEncoder.encode_to_host``, alone and with the file written; in the same process
and repeats ``_write_png`` of the driver on the same planes (the parent's path as it stands: filter 0, zlib level 6, the file written); file
sizes of both; the 3-pose ``render_path`` with files written, ``pnrf_device_png`` off and on.  ``--cpu-only`` keeps the device sections of an
existing file."""
from __future__ import annotations

import argparse
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


def size_margin():
    S = ops.png_segment_rows()
    rng = np.random.RandomState(5)
    rows, worst = [], 0.0
    for H, W in ((189, 252), (378, 504)):
        rgb, depth = png_ref.scene_views(H, W)
        noisy = (255 * np.clip(rgb.astype(np.float32) / 255 + rng.normal(0, 0.012, rgb.shape), 0, 1)).astype(np.uint8)
        for name, img in (('rgb', rgb), ('rgb+noise', noisy), ('depth', depth)):
            data = ops.png_encode_host(img)
            p = png_ref.parse(data)
            ref = png_ref.reference_size(p['filtered'], W * p['channels'] + 1, S)
            parent = len(png_ref.parent_file(img))
            raw = H * W * p['channels']
            worst = max(worst, len(p['zdata']) / ref - 1)
            rows.append({'view': [H, W], 'plane': name, 'file_bytes': len(data), 'zlib_stream_bytes': len(p['zdata']), 'reference_stream_bytes': ref,
                         'stream_over_reference': round(len(p['zdata']) / ref, 4), 'parent_file_bytes': parent, 'file_over_parent': round(len(data) / parent, 4),
                         'file_over_raw_plane': round(len(data) / raw, 4)})
    return {'m': math.ceil(max(worst, 0.0) * 1e4) / 1e4, 'segment_rows': S, 'reference': 'zlib.compressobj(6, DEFLATED, 15, 9, Z_RLE), Z_FULL_FLUSH per segment, same filtered bytes',
            'cases': rows}


def device_part(render_path=True):
    import torch
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    from pronerf_amd import synthetic
    H, W = 756, 1008
    dev = torch.device('cuda:0')
    rgb_h, depth_h = png_ref.scene_views(H, W)
    res = {'frame': [H, W], 'device': torch.cuda.get_device_name(0), 'repeats': REPEATS}
    with tempfile.TemporaryDirectory() as tmp:
        for name, plane_h in (('rgb', rgb_h), ('depth', depth_h)):
            plane = torch.from_numpy(plane_h).to(dev)
            enc = ops.PngEncoder(H, W, 1 if plane_h.ndim == 2 else 3, dev)
            path_d, path_h = os.path.join(tmp, name + '_device.png'), os.path.join(tmp, name + '_host.png')
            data = enc.encode_to_host(plane)                      # warm-up of both paths
            trt._write_png(path_h, plane_h)
            assert np.array_equal(png_ref.decode(data), plane_h)
            ev, wall, wall_file, host = [], [], [], []
            for _ in range(REPEATS):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record(); enc.launch(plane); t1.record()
                torch.cuda.synchronize()
                ev.append(t0.elapsed_time(t1))
                t = time.perf_counter(); data = enc.encode_to_host(plane); wall.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter(); trt._write_bytes(path_d, enc.encode_to_host(plane)); wall_file.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter(); trt._write_png(path_h, plane_h); host.append((time.perf_counter() - t) * 1e3)
            res[name] = {'encode_fwd_device_ms': ev, 'encode_to_host_wall_ms': wall, 'encode_to_host_and_write_wall_ms': wall_file, 'host_write_png_wall_ms': host,
                         'device_file_bytes': len(data), 'host_file_bytes': os.path.getsize(path_h), 'raw_plane_bytes': int(plane_h.size),
                         'device_below_host_in_every_repeat': bool(all(a < b for a, b in zip(wall_file, host)))}
    if render_path:
        from types import SimpleNamespace
        a = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256, mmnetskips=[10000],
                            N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)
        kw, _ = trt.create_nerf(a, device=dev)
        sd = synthetic.state_dicts(synthetic.make_weights(0, 'trained'))
        kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
        scene = synthetic.make_scene(0, H=H, W=W, n_views=6)
        kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
        targets = [scene['c2w'], scene['poses'][0], scene['poses'][1]]
        walls, sizes = {'off': [], 'on': []}, {}
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            for rep in range(REPEATS + 1):                        # alternating; the first pair is the warm-up
                for name, opts in (('off', {}), ('on', {'pnrf_device_png': True})):
                    k = {**kw, **opts}
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    trt.render_path(targets, (H, W, scene['focal']), scene['K'], None, k, savedir=os.path.join(tmp, name), n_timing_reps=1, verbose=False)
                    if rep:
                        walls[name].append((time.perf_counter() - t) * 1e3)
                    sizes[name] = sum(os.path.getsize(os.path.join(tmp, name, f)) for f in os.listdir(os.path.join(tmp, name)))
        res['render_path_3_poses_wall_ms'] = walls
        res['render_path_6_files_bytes'] = sizes
        res['render_path_note'] = 'one render per pose, six PNG files written; off = the statements of the parent commit (zlib on a worker thread)'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode.json'))
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--no-render-path', action='store_true')
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res['size_margin'] = size_margin()
    if not args.cpu_only:
        import torch
        assert torch.cuda.is_available(), 'the device part needs a GPU (--cpu-only measures the sizes alone)'
        res['device'] = device_part(not args.no_render_path)
    line = json.dumps(res, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
