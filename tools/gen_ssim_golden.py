"""TEST INFRASTRUCTURE ONLY — writes tests/golden/ssim_cases.npz.

Runs where the reference checkout is present: imports its ``run_nerf_helpers`` (CPU; the modules it imports at top level and never uses
on this path — torchvision — are replaced by empty stand-ins, as in oracle/gen_golden.py), feeds its own ``img2ssim`` the seeded images of
tests/ssim_ref.py and stores inputs + results.  Only the arrays travel:

    <kind>_<H>x<W>_a / _b      the two float32 images (four kinds, 12 x 17 and 43 x 75)
    <kind>_<H>x<W>_ssim        what the reference's img2ssim returns for them (float64)
    <kind>_12x17_map           its return_map=True result
    taps_<T>                   the 1-D filter the reference hands to scipy for filter_size 7, 8, 11 (recorded from its convolve2d calls)

Usage:  python tools/gen_ssim_golden.py [reference directory]
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ssim_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ssim_cases.npz')


def load_reference(ref_dir):
    sys.dont_write_bytecode = True
    for m in ('torchvision', 'torchvision.models'):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, ref_dir)
    import run_nerf_helpers as helpers
    return helpers


class _Recorder:
    """Stands in for the reference module's ``signal``: passes convolve2d through to scipy and keeps the filters it was called with."""

    def __init__(self, real):
        self.real, self.filters = real, []

    def convolve2d(self, z, f, mode='full'):
        self.filters.append(np.array(f, copy=True))
        return self.real.convolve2d(z, f, mode=mode)


def main(ref_dir='/root/reference'):
    helpers = load_reference(ref_dir)
    out = {}
    for H, W in ssim_ref.FIXTURE_SHAPES:
        for kind in ssim_ref.KINDS:
            a, b = ssim_ref.make_pair(kind, H, W)
            key = f'{kind}_{H}x{W}'
            out[key + '_a'], out[key + '_b'] = a, b
            out[key + '_ssim'] = np.float64(helpers.img2ssim(a, b))
            if (H, W) == (12, 17):
                out[key + '_map'] = np.asarray(helpers.img2ssim(a, b, return_map=True), dtype=np.float64)
    a, b = ssim_ref.make_pair('noise', 43, 75)
    rec = _Recorder(helpers.signal)
    helpers.signal = rec
    try:
        for T in (7, 8, 11):
            del rec.filters[:]
            out[f'ssim_noise_43x75_T{T}'] = np.float64(helpers.img2ssim(a, b, filter_size=T))
            out[f'taps_{T}'] = np.asarray(rec.filters[0], dtype=np.float64).reshape(-1)
            assert out[f'taps_{T}'].shape == (T,)
    finally:
        helpers.signal = rec.real
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main(*sys.argv[1:2])
