"""CPU: skip connections inside the sampler / refine stacks (``--mmnetskips``) — what can be checked without a GPU.

* the restatement ``mmskips_ref.skip_backbone`` composed with the oracle's stage functions reproduces the REFERENCE's captured intermediates and rgb on
  the three ``infer_skip_*`` goldens (tools/gen_golden_mmskips.py), to the tolerances of tests/test_oracle_golden.py;
* the integer skip nets the GPU tests run are certified exact;
* ``make_weights(mmnetskips=())`` draws what it drew before the argument existed, and the skip draws leave every other array alone;
* the built library's skip kernels: no scratch, at most 256 VGPRs (the 8-wave forms: exactly 256), and the MFMA counts the layer bodies add up to.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import exact_nets as en
import mmskips_ref as ms
from oracle import pronerf_oracle as orc
from oracle import synth


@pytest.mark.parametrize('name', sorted(ms.CASES))
def test_restatement_reproduces_the_reference_goldens(golden_dir, name):
    g, shape, scene, w = ms.case(golden_dir, name)
    assert ms.skips_of(w['sampler']['W']) == list(ms.CASES[name]) == ms.skips_of(w['refine']['W'])
    fr = orc.frame_setup(scene, num_neighbor=shape['num_neighbor'], n_pts=shape['n_pts'])
    np.testing.assert_array_equal(fr['rays'].numpy(), g['rays'])
    r = ms.render_ref(w, fr, shape['n_pts'])
    tie_free = np.diff(g['depth_sorted'], axis=1).min(axis=1) > ms.TIE
    assert (~tie_free).mean() <= 0.05
    np.testing.assert_array_equal(r['sort_idx'].numpy()[tie_free], g['sort_idx'][tie_free])
    np.testing.assert_allclose(r['depth_raw'].numpy(), g['depth_raw'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r['depth_sorted'].numpy(), g['depth_sorted'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r['add_sorted'].numpy()[tie_free], g['add_sorted'][tie_free], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(r['refine_in'].numpy()[:, 48:], g['epi'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r['refine_depth'].numpy(), g['refine_depth'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r['z'].numpy(), g['z'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r['rgb'].numpy()[tie_free], g['rgb'][tie_free], rtol=0, atol=1e-3)
    assert orc.psnr(r['rgb'][torch.from_numpy(tie_free)], torch.from_numpy(g['rgb'][tie_free])) > 60.0


def test_integer_skip_nets_are_certified():
    """Every net / input set of tests/test_mmskips_gpu.py's exact tests: operands representable (fp16: integers up to 2048; fp32: 2^24), partial sums
    below 2^24, ELU pre-activations >= 0, x-columns with non-zero weights, refine logits inside exact_nets' sensitive range."""
    for D, sets in ms.SKIP_SETS.items():
        for skips in sets:
            net = ms.refine_net(4, D, skips)
            x = en.elu_inputs(257, 48 + 24 * 4, seed=D)
            y = ms.exact_forward(net, x, en.LIM['f16'])
            assert np.abs(y[:, :8]).max() <= en.LOGIT_MAX and np.abs(y[:, 8:32]).max() <= en.OFFSET_MAX
            for i in skips:
                assert np.count_nonzero(net['W'][i + 1][:, :144]) >= 128
            W, b = ms.refine_pack_weights(net)
            assert all(a.dtype == np.float32 for a in W + b) and ms.skips_of(W) == skips
            snet = ms.sampler_net(D, skips)
            rays = ms.sampler_rays(257, seed=D)
            ys = ms.exact_forward(snet, ms.sampler_inputs(rays), en.LIM['f32'])
            assert (np.argsort(ys[:, :8], axis=1) == np.argsort(ys[:1, :8], axis=1)).all() and len(np.unique(ys[:, 8:24])) > 8
            for i in skips:
                assert np.count_nonzero(snet['W'][i + 1][:, :6 * ms.SAMPLER_P]) >= 128
            # the net on the log2(e) scale for the split-fp16 / pass-1 placement test: certified at fp16's integer range, every last-layer unit read by
            # exactly one add / mul row with weight +-1 (a hidden unit off by 1 moves an output by 1 >> SCALED_TOL), packer weights exist
            pnet = ms.sampler_scaled_net(D, skips)
            yp = ms.exact_forward(pnet, ms.sampler_inputs(rays, 1), en.LIM['f16'])
            head = pnet['W'][-1][8:24]
            assert (np.count_nonzero(head, axis=0) == 1).all() and set(np.unique(head)) <= {-1.0, 0.0, 1.0} and ms.SCALED_TOL < 0.01
            assert (np.argsort(yp[:, :8], axis=1) == np.argsort(yp[:1, :8], axis=1)).all()
            Wp, bp = ms.sampler_pack_weights(pnet)
            assert ms.skips_of(Wp) == skips and all(a.dtype == np.float32 for a in Wp + bp)
            for i in skips:
                assert np.count_nonzero(pnet['W'][i + 1][:, :6]) >= 128


# sha256 of every array make_weights(seed, kind) returned before it took mmnetskips, for the seeds / kinds / shapes of the skip goldens' no-skip twins
def _digest(w):
    h = hashlib.sha256()
    for n in ('sampler', 'refine', 'nerf'):
        for a in w[n]['W'] + w[n]['b']:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


PARENT_DIGESTS = {
    (21, 'trained', 48, 8, 4): '0c07dfe545363900a8d40efe387762f9df34387461d47758b831f26cc1714f11',
    (22, 'trained', 8, 3, 1): 'fb94ec9266869660a1efb4e6485b6c3b4ce55eea346062943a45dac83484bfb2',
    (23, 'trained', 32, 5, 7): '87217b0247a84b9bc5a13b657dd6a684a6255a4408cd2320c609e432e3bf0b8a',
    (0, 'trained', 48, 6, 4): '31c7ef7f5761c2cf8c77f968a26b3c0e2013eaccee57830f57b37bda24bd1b2d',
    (1, 'default', 48, 6, 4): '106ebeebfb26c76f3aab99bee245a7971d85cb01035525c1a3087c588dd9a527',
}


@pytest.mark.parametrize('key', sorted(PARENT_DIGESTS))
def test_make_weights_without_skips_is_what_it_was(key):
    seed, kind, n_pts, D, nb = key
    base = synth.make_weights(seed, kind, n_pts=n_pts, mmnetdepth=D, num_neighbor=nb)
    assert _digest(base) == PARENT_DIGESTS[key]                     # recorded on the parent commit
    assert _digest(synth.make_weights(seed, kind, n_pts=n_pts, mmnetdepth=D, num_neighbor=nb, mmnetskips=())) == PARENT_DIGESTS[key]
    assert _digest(synth.make_weights(seed, kind, n_pts=n_pts, mmnetdepth=D, num_neighbor=nb, mmnetskips=[10000])) == PARENT_DIGESTS[key]
    sk = synth.make_weights(seed, kind, n_pts=n_pts, mmnetdepth=D, num_neighbor=nb, mmnetskips=[0, D - 2])
    for n in ('sampler', 'refine', 'nerf'):
        for a, b in zip(sk[n]['W'] + sk[n]['b'], base[n]['W'] + base[n]['b']):
            np.testing.assert_array_equal(a[..., -b.shape[-1]:], b)          # the h-columns (and every other array) are the no-skip draws
    assert ms.skips_of(sk['sampler']['W']) == sorted({0, D - 2}) == ms.skips_of(sk['refine']['W'])
    assert np.abs(sk['sampler']['W'][1][:, :6 * n_pts]).min() > 0


def test_skip_kernels_static_figures():
    """No scratch, at most 256 VGPRs, the 8-wave (WIDE) forms exactly 256 — and the MFMA counts.  A kernel's hidden layer is compiled at three call
    sites (the ping-pong pair and the odd layer), and the skip form adds at each of them one more layer body with the x k-steps:
      pass 1    424 + 3 x 8 tiles x (16 + 3: W_hi 2^11, W_hi, W_lo 2^11)                     = 880
      split     1248 + 3 x 8 pairs x (8 + 1) k-steps x 6                                      = 2544
      exact     3264 + 3 x 16 tiles x (16 + 1) fragments x 4                                  = 6528
      refine    the plain kernel's count + 3 x 8 tiles x (16 + 3 NV + 3)                      (NV = 2, projecting head: 472 + 600 = 1072)"""
    from pronerf_amd import build
    lib = build.LIB
    if not os.path.exists(lib):
        build.build(verbose=False)
    k = build.device_kernels(lib)
    skip = {n: v for n, v in k.items() if '_skip_kernel' in n}
    want = {'sampler_skip_kernel(SamplerArgs)': 6528}
    for nw in (4, 8):
        want[f'void sampler_p1_skip_kernel<{nw}>(SamplerArgs)'] = 880
        want[f'void sampler_h16_skip_kernel<{nw}>(SamplerArgs)'] = 2544
    for nv in (1, 2, 3, 4):
        body = 3 * 8 * (16 + 3 * nv + 3)
        want[f'void refine_skip_kernel<4, 0, 0, {nv}>(RefineArgs)'] = k[f'void refine_kernel<1, 4, 0, 0, PrecF16, {nv}>(RefineArgs)']['mfma'] + body
        for nw in ((4, 8) if nv <= 2 else (4,)):          # the WIDE form's parked input fits the LDS up to num_neighbor 4: no instance beyond
            for head in (0, 1):
                want[f'void refine_skip_kernel<{nw}, 1, {head}, {nv}>(RefineArgs)'] = k[f'void refine_kernel<1, {nw}, 1, {head}, PrecF16, {nv}>(RefineArgs)']['mfma'] + body
    assert sorted(skip) == sorted(want)
    assert k['void sampler_p1_kernel<8>(SamplerArgs)']['mfma'] == 424 and k['void refine_kernel<1, 8, 1, 1, PrecF16, 2>(RefineArgs)']['mfma'] == 472
    for n, v in skip.items():
        assert v['scratch'] == 0 and v['vgpr'] <= 256 and v['mfma'] == want[n], (n, v, want[n])
        wide = n.startswith('sampler_skip_kernel') or '_skip_kernel<8' in n
        assert not wide or v['vgpr'] == 256, (n, v)


@pytest.mark.parametrize('driver', ['run_S_eS_eN_alter_base', 'run_S_eS_eN_alter_base_refine2'])
def test_training_drivers_refuse_skips_inside_the_stack(tmp_path, driver):
    """The two training drivers build their sampler / refine stacks without skip connections: an ``mmnetskips`` that names a layer inside the stack is
    refused before anything else happens (no device, no data set needed)."""
    import importlib
    from pronerf_amd.ops import PnrfError
    mod = importlib.import_module('pronerf_amd.' + driver)
    cfg = tmp_path / 'c.txt'
    base = (f'expname = t\nbasedir = {tmp_path}/logs\ndatadir = {tmp_path}/none\ndataset_type = llff\nfactor = 4\nllffhold = 8\nN_samples = 8\n'
            f'N_point_ray_enc = 48\nmmnetdepth = 6\nnum_neighbor = 4\nuse_viewdirs = True\n') + (f'pretrain_path = {tmp_path}/stage1.tar\n' if driver.endswith('refine2') else '')
    cfg.write_text(base + 'mmnetskips = [4]\n')
    with pytest.raises(PnrfError, match='mmnetskips'):
        mod.train(['--config', str(cfg)])
