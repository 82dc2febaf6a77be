"""TEST INFRASTRUCTURE ONLY — golden vectors of nets with skip connections inside the sampler / refine stacks (``--mmnetskips``).

Runs where the reference lies (CPU, fp32), like ``oracle/gen_golden.py``, whose import recipe, per-frame setup and capture hooks it uses: the
reference's own ``render_rays`` on modules built with ``skips=mmnetskips``, weights from ``synthetic.make_weights(..., mmnetskips=...)`` (so the
fixtures hold no weights), every intermediate captured under the keys of the ``infer_shape_*`` fixtures.  Writes tests/golden/infer_skip_*.npz.

Each case must keep the reference's own fp32 tie set (adjacent sorted depths within 1e-6) at no more than 5 % of the rays: the cap of
tests/test_shapes_gpu.py.  A seed that misses it is replaced, not tolerated.

Usage:  python tools/gen_golden_mmskips.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from oracle import synth  # noqa: E402

TIE, TIE_CAP = 1e-6, 0.05
# (name, seed, kind, H, W, shape, pool of views): (a) the reference's argparse defaults mmnetdepth 8 / mmnetskips [4] on Fern's other values; (b) a skip straight
# behind layer 0, two consecutive skips, the last legal index; (c) four views per lane half, the eighth a padded one
CASES = [
    ('infer_skip_d8_s4_p48_nb4_16x20', 21, 'trained', 16, 20, dict(n_pts=48, mmnetdepth=8, num_neighbor=4, netdepth=8, mmnetskips=(4,)), 5),
    ('infer_skip_d3_s01_p8_nb1_16x20', 22, 'trained', 16, 20, dict(n_pts=8, mmnetdepth=3, num_neighbor=1, netdepth=8, mmnetskips=(0, 1)), 3),
    ('infer_skip_d5_s3_p32_nb7_16x20', 23, 'trained', 16, 20, dict(n_pts=32, mmnetdepth=5, num_neighbor=7, netdepth=8, mmnetskips=(3,)), 8),
]


def build_models(helpers, weights, shape):
    """gen_golden.build_models with the sampler / refine stacks built from --mmnetskips as the reference's create_nerf builds them."""
    S, NB = synth.N_SAMPLES, shape['num_neighbor']
    skips = list(shape.get('mmnetskips', (10000,)))
    sd = synth.state_dicts(weights, skips)
    sampler = helpers.MinMaxRaySamplerTRT_Net(D=shape['mmnetdepth'], W=synth.MMNETWIDTH, input_ch=6 * shape['n_pts'], output_ch=3 * S + 3, skips=skips, N_samples=S)
    refine = helpers.MinMaxRayEpiSamplerTRT_Net(D=shape['mmnetdepth'], W=synth.MMNETWIDTH, input_ch=6 * S + 3 * NB * S, output_ch=4 * S + 3, skips=skips, N_samples=S)
    nerf = helpers.DoNeRFTRT(D=shape['netdepth'], W=synth.NETWIDTH, n_in=synth.POS_CH + synth.DIR_CH, n_out=4, skip='auto')
    sampler.load_state_dict(sd['sampler']); refine.load_state_dict(sd['refine']); nerf.load_state_dict(sd['nerf'])
    return sampler.eval(), refine.eval(), nerf.eval()


def main():
    helpers, iw, trt = gg.load_reference()
    gg.build_models = build_models
    for name, seed, kind, H, W, shape, nv in CASES:
        gg.run_infer_case(helpers, iw, trt, name, seed, kind, H, W, rotate=True, sigma_t=0.1, shape=shape, n_views=nv)
        path = os.path.join(gg.OUT, name + '.npz')
        g = np.load(path)
        ties = float((np.diff(g['depth_sorted'], axis=1).min(axis=1) <= TIE).mean())
        size = os.path.getsize(path)
        print(f'  {name}: skips {list(shape["mmnetskips"])}, fp32 tie set {ties:.1%} of the rays, {size / 1024:.0f} KiB')
        assert ties <= TIE_CAP, f'{name}: the reference ties on {ties:.1%} of the rays (cap {TIE_CAP:.0%}): take another seed'
        assert size <= 900 * 1024, f'{name}: {size} bytes'


if __name__ == '__main__':
    main()
