#!/usr/bin/env python3
"""Index evidence at frame size for the pass-1 error model with skip connections: one 756 x 1008 frame per weight kind of
``synthetic.make_weights`` with ``mmnetdepth 8, mmnetskips [4]``, the two-pass sampler at kappa = 2, 1 and 0.5 against the fp32 restatement of the
backbone with skips (torch on the device, the oracle's sampler and sort).  Prints, per kind and kappa, the rays outside the fp32 tie set (smallest sorted gap
> 4e-6, as tests/test_shapes_gpu.py's full-frame test) whose sort indices differ, and the shares of the second and third pass.

    python tools/mmskips_kappa_scan.py > profiles/mmskips_kappa_scan.txt

A mismatch at kappa >= 1 means the model is wrong (fix the model, do not widen kappa); kappa = 0.5 is below the margin the default (2) is meant to hold."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import pronerf_oracle as orc      # noqa: E402
from pronerf_amd import ops, synthetic        # noqa: E402
import mmskips_ref as ms                      # noqa: E402

H, W, D, SKIPS = 756, 1008, 8, (4,)


def main():
    dev = torch.device('cuda:0')
    torch.backends.cuda.matmul.allow_tf32 = False
    scene = synthetic.make_scene(0, H=H, W=W, focal=815.13, rotate=True)
    rays, _ = ops.frame_rays(scene['K'], scene['c2w'], H, W, device=dev)
    N = H * W
    print(f'frame {H} x {W} ({N} rays), mmnetdepth {D}, mmnetskips {list(SKIPS)}, seed 0; outside ties = smallest sorted gap of the fp32 restatement > 4e-6')
    for kind in ('default', 'spread', 'trained', 'heavy', 'x4'):
        w = synthetic.make_weights(0, kind, mmnetdepth=D, mmnetskips=SKIPS)['sampler']
        wd = {'W': [torch.as_tensor(x).to(dev) for x in w['W']], 'b': [torch.as_tensor(x).to(dev) for x in w['b']]}
        idx, free = [], []
        with ms.skip_oracle(), torch.no_grad():
            for a in range(0, N, 131072):
                r = rays[a:a + 131072]
                _, add, mul, depth = orc.sampler_forward(wd, orc.mm_input_from_rays(r[:, 0:3], r[:, 3:6], synthetic.N_POINT_RAY_ENC))
                ds, ix, _, _ = orc.sort_gather(depth, add, mul, r[:, 6:7], r[:, 7:8])
                idx.append(ix); free.append((ds[:, 1:] - ds[:, :-1]).min(1)[0] > 4e-6)
        idx, free = torch.cat(idx), torch.cat(free)
        mlp = ops.PackedMLP(ops.NET_SAMPLER, w['W'], w['b'])
        for kappa in (2.0, 1.0, 0.5):
            out = ops.sampler_fwd(mlp, rays, want_idx=True, two_pass=True, kappa=kappa)
            mism = int((out[1][free] != idx[free]).any(1).sum())
            print(f'{kind:8s} kappa {kappa:3.1f}: {mism} rays with other indices among {int(free.sum())} outside ties; second pass {int(out[6]) / N:6.1%}, third pass {int(out[7]) / N:6.1%}')


if __name__ == '__main__':
    main()
