"""Times the training drivers' loop AROUND the trainer's device step, at the Fern training size (756 x 1008 pixels, 17 training views, N_rand as in
configs/llff/fern/fern_refine.txt) on a synthetic LLFF-style scene: host wall time per iteration of the statements train() executes per batch
(batch assembly, draws, fwd_bwd / explore_fwd_bwd, adam_step) for --device_batches off (twice: their difference is the spread), rays and all, for
stage 2 and stage 1; the set-up time and the device memory each mode holds after set-up; and the device time of pnrf_train_batch_fwd alone.
The four configurations are interleaved window by window in one process; a window is 200 iterations, synchronised at both ends; the figure is
the median of 5 windows.  The per-kernel figure repeats ONE call on cached buffers (same indices every time).  Writes one JSON document.

    python tools/train_loop_bench.py [--out profiles/train_batch_loop.json] [--iters 200] [--windows 5]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pronerf_amd import ops, synthetic  # noqa: E402
from pronerf_amd.config import read_config_file  # noqa: E402
from pronerf_amd import run_S_eS_eN_alter_base_refine2 as s2  # noqa: E402

H, W, NV = 756, 1008, 17
MAX_MULT = 8
RAW_NOISE_STD = 1.0


class Loop:
    """One configuration of one stage: the set-up and the per-iteration statements of train() (run_S_eS_eN_alter_base_refine2.py, ..._base.py)."""

    def __init__(self, stage, mode, scene, tr, n_rand, dev):
        self.stage, self.mode, self.tr, self.n_rand, self.dev = stage, mode, tr, n_rand, dev
        near = 0. if stage == 2 else 1e-6
        images, poses, K = scene['images'], scene['poses'], scene['K']
        s2._VIEWS.clear()                                                   # every configuration pays for its own packed views
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m0, t0 = torch.cuda.memory_allocated(), time.perf_counter()
        if mode == 'off':
            pr = [ops.frame_rays(K, poses[i], H, W, near=near, far=1., device=dev) for i in range(NV)]
            self.rays_all = torch.cat([p[0] for p in pr], 0); self.or_rays_all = torch.cat([p[1] for p in pr], 0)
            del pr
            self.target_all = torch.as_tensor(images, dtype=torch.float32).reshape(-1, 3).to(dev)
            self.own_all = torch.arange(NV, device=dev).repeat_interleave(H * W)
            self.img4, self.poses_t, self.K_t, self.rank = s2._train_views(images, poses, K, dev)
        else:
            self.tset = ops.TrainSet(ops.Scene.from_views(poses, images, K, device=dev), n_rand, near=near, far=1., max_cols=8 if stage == 2 else 8 * MAX_MULT)
        torch.cuda.synchronize()
        self.setup_ms = (time.perf_counter() - t0) * 1e3
        self.bytes_after_setup = torch.cuda.memory_allocated() - m0
        # a Scene's device arrays are the library's own allocation, which torch's counter does not see: texel cache, poses, intrinsics (pnrf_scene.hip)
        self.library_bytes = 0 if mode == 'off' else NV * H * W * 16 + 1024 + 256
        self.peak_bytes_during_setup = torch.cuda.max_memory_allocated() - m0
        self.n_total = NV * H * W
        self.perm = torch.randperm(self.n_total, device=dev)
        self.i_batch, self.i = 0, 0

    def step(self):
        dev, tr, mode, nv, N = self.dev, self.tr, self.mode, NV, self.n_rand
        self.i += 1
        i = self.i
        idx = self.perm[self.i_batch:self.i_batch + N]
        self.i_batch += N
        if self.i_batch + N > self.n_total:
            self.perm = torch.randperm(self.n_total, device=dev); self.i_batch = 0
        n = idx.shape[0]
        if mode == 'off':
            order = torch.as_tensor(sorted(random.sample(range(nv - 1), 4)), device=dev)
            ref_nos = self.rank[self.own_all[idx]][:, 1:][:, order].contiguous()
            batch = (self.rays_all[idx], self.or_rays_all[idx], self.target_all[idx], self.img4, self.poses_t, self.K_t, ref_nos)
        else:
            order = sorted(random.sample(range(nv - 1), 4))
            batch = self.tset.batch(idx, order) if mode == 'rays' or (self.stage == 1 and i % 2 == 0) else None
        if self.stage == 2:
            if mode != 'all':
                jitter = torch.abs(torch.normal(0.0, 1.0, size=(n, 8), device=dev) / 5).clamp(max=1 - 2e-6)
                jdir = 1 if random.random() > 0.5 else -1
                noise = torch.randn(n, 8, device=dev) * RAW_NOISE_STD
            else:
                out = self.tset.batch(idx, order, step=i, seed=0, jitter_cols=8, jitter_cap=1 - 2e-6, noise_cols=8, noise_std=RAW_NOISE_STD)
                batch, jitter, noise = out[:7], out[7], out[8]
                jdir = 1 if random.random() > 0.5 else -1
            tr.fwd_bwd(*batch, jitter=jitter, jitter_dir=jdir, raw_noise=noise, a_mmrgb=0.0, want_rgb=False)
            tr.adam_step(3e-4)
        elif i % 2 != 0:
            n_mult = random.randint(1, MAX_MULT)
            dir1 = (1 if random.random() > 0.5 else -1) if n_mult > 1 else 1
            if mode != 'all':
                jitter = torch.abs(torch.normal(0.0, 1.0, size=(n, 8 * n_mult), device=dev) / 5).clamp(max=0.99)
            dir2 = 1 if random.random() > 0.5 else -1
            if mode != 'all':
                noise = torch.randn(n, 8 * n_mult, device=dev) * RAW_NOISE_STD
            else:
                out = self.tset.batch(idx, order, step=i, seed=0, jitter_cols=8 * n_mult, jitter_cap=0.99, noise_cols=8 * n_mult, noise_std=RAW_NOISE_STD)
                batch, jitter, noise = out[:7], out[7], out[8]
            tr.explore_fwd_bwd(*batch, n_mult=n_mult, dir1=dir1, jitter=jitter, dir2=dir2, raw_noise=noise, want_rgb=False)
            tr.adam_step(3e-4, nerf_only=True)
        else:
            tr.fwd_bwd(*batch, eps=1e-6, a_mmrgb=1.0, clamp=10.0, layout=1, want_rgb=False)
            tr.adam_step(3e-4)


def window_ms(loop, iters, seed):
    random.seed(seed)                                     # every configuration draws the same n_mult sequence in a given window
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        loop.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def device_ms(fn, reps, warmup=10, windows=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_batch_loop.json'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--windows', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    n_rand = int(read_config_file(os.path.join(ROOT, 'configs', 'llff', 'fern', 'fern_refine.txt'))['N_rand'])
    scene = synthetic.make_scene(0, H=H, W=W, n_views=NV, sigma_t=0.2, rotate=True)
    sd = synthetic.state_dicts(synthetic.make_weights(0, 'trained'))
    layers = s2.trainer_layer_list(sd['sampler'], sd['refine'], synthetic.nerfcls_state_dict(synthetic.make_nerfcls_weights(0, head_scale=0.3)))
    res = {'frame': [H, W], 'training_views': NV, 'N_rand': n_rand, 'iters_per_window': args.iters, 'windows': args.windows,
           'device': torch.cuda.get_device_name(0), 'raw_noise_std': RAW_NOISE_STD}
    names = ['off', 'off_again', 'rays', 'all']
    for stage in (2, 1):
        tr = ops.Trainer([W_ for W_, _ in layers], [b for _, b in layers], max_rays=n_rand, device=dev, max_samples=8 if stage == 2 else 8 * MAX_MULT)
        loops = {nm: Loop(stage, nm.split('_')[0], scene, tr, n_rand, dev) for nm in names}
        for lp in loops.values():                         # warm-up: allocator, kernels, every n_mult
            window_ms(lp, 40, 0)
        ms = {nm: [] for nm in names}
        for w in range(args.windows):
            for nm in names:
                ms[nm].append(window_ms(loops[nm], args.iters, 1000 + w))
        med = {nm: float(np.median(v)) for nm, v in ms.items()}
        spread = abs(med['off'] - med['off_again'])
        off = 0.5 * (med['off'] + med['off_again'])
        st = {'host_wall_ms_per_iteration': {nm: {'median': med[nm], 'windows': ms[nm]} for nm in names},
              'spread_ms': spread,
              'gain_ms': {'rays': off - med['rays'], 'all': off - med['all']},
              'gain_exceeds_3x_spread': {'rays': bool(off - med['rays'] > 3 * spread), 'all': bool(off - med['all'] > 3 * spread)},
              'setup_ms': {nm: loops[nm].setup_ms for nm in names},
              'torch_bytes_after_setup': {nm: loops[nm].bytes_after_setup for nm in names},
              'library_scene_bytes': {nm: loops[nm].library_bytes for nm in names},
              'bytes_after_setup': {nm: loops[nm].bytes_after_setup + loops[nm].library_bytes for nm in names},
              'peak_bytes_during_setup': {nm: loops[nm].peak_bytes_during_setup for nm in names}}
        # pnrf_train_batch_fwd alone: ONE call repeated on cached buffers (same indices, same outputs)
        ts = loops['all'].tset
        idx = torch.randperm(NV * H * W, device=dev)[:n_rand]
        cols = 8 if stage == 2 else 8 * MAX_MULT
        st['train_batch_fwd_device_ms'] = {
            'rows_only': device_ms(lambda: ts.batch(idx, (0, 3, 7, 11)), 200),
            f'rows_and_draws_{cols}_columns': device_ms(lambda: ts.batch(idx, (0, 3, 7, 11), step=1, jitter_cols=cols, jitter_cap=0.99, noise_cols=cols,
                                                                         noise_std=1.0), 200)}
        assert ts.bad_rows() == 0
        res[f'stage{stage}'] = st
        del loops, tr, ts
        torch.cuda.empty_cache()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
