"""GPU: skip connections inside the sampler / refine stacks (``--mmnetskips``; the reference's argparse default is ``mmnetdepth 8, mmnetskips [4]``).

1. surface: skip nets pack, the mask is reported, what is not built says so and names skips, engine files (format 6) round-trip;
2. integer skip nets with exact answers (tests/mmskips_ref.py): the exact-fp32 sampler kernel and the refine kernel (module-level forward: bit for bit;
   fused stage: z / pts against float64 at exact_nets' derived tolerance), skip sets [0], [D-2], [0, D-2], [1, 2] at D in {2, 3, 6}, ray counts at the
   batch edges.  The split-fp16 and pass-1 sampler kernels run on log2(e)-scaled streams whose first-layer-like weights are split into two planes, so
   no weight is an integer there and bit identity cannot be had; they run an integer net ON that scale whose stored hi planes are exact integers
   (pre-image weights, ``mmskips_ref.sampler_scaled_net``) and must give add / mul within 1e-3 of the integers, where one misplaced x fragment, plane
   or k-step moves an output by >= 1 — same skip sets, same ray counts, both shapes;
3. stages against the fp32 restatement on the shapes of the three reference goldens: the three sampler forms, the refine stage from rows and with the
   projecting head, NARROW and WIDE, at the bars of tests/test_shapes_gpu.py;
4. frames against the REFERENCE's goldens through ``Renderer`` and the driver API;
5. index evidence for the pass-1 error model with skips at kappa 2 and 1;
6. NARROW and WIDE rows are bit-identical; a call under graph capture equals the eager call.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import exact_nets as en
import mmskips_ref as ms
from oracle import pronerf_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def refs(golden_dir):
    """Per golden: (g, shape, scene, weights, frame setup, fp32 restatement of every stage) — computed once, shared, never modified."""
    out = {}
    for name in ms.CASES:
        g, shape, scene, w = ms.case(golden_dir, name)
        fr = orc.frame_setup(scene, num_neighbor=shape['num_neighbor'], n_pts=shape['n_pts'])
        out[name] = (g, shape, scene, w, fr, ms.render_ref(w, fr, shape['n_pts']))
    return out


def _mlp(ops, net, w, **kw):
    return ops.PackedMLP(net, w['W'], w['b'], **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. surface
def test_surface(dev, tmp_path):
    from pronerf_amd import ops
    from pronerf_amd import run_nerf_helpers as h
    s = h.MinMaxRaySamplerTRT_Net(D=8, input_ch=288, output_ch=27, skips=[4]).to(dev)
    r = h.MinMaxRayEpiSamplerTRT_Net(D=8, input_ch=144, output_ch=35, skips=[4]).to(dev)
    ps, pr = s.packed(), r.packed()
    assert ps.skips == [4] and pr.skips == [4]
    import ctypes as C
    from pronerf_amd import _lib
    m = C.c_uint32()
    assert _lib.load().pnrf_mlp_skips(ps.handle, C.byref(m)) == 0 and m.value == 1 << 4
    assert h.MinMaxRaySamplerTRT_Net(D=6, input_ch=288, output_ch=27, skips=[10000]).to(dev).packed().skips == []
    w = synth.make_weights(0, 'trained', mmnetdepth=8, mmnetskips=[4])
    bad = [a.copy() for a in w['sampler']['W']]
    bad[5] = bad[5][:, 1:]                                               # 256 + in_ch - 1 columns
    with pytest.raises(ops.PnrfError, match='skip'):
        ops.PackedMLP(ops.NET_SAMPLER, bad, w['sampler']['b'])
    with pytest.raises(ops.PnrfError):                                   # a skip at D - 1 would feed fc_output
        h.MinMaxRaySamplerTRT_Net(D=8, input_ch=288, output_ch=27, skips=[7]).to(dev).packed()
    last = [a.copy() for a in w['refine']['W']]
    last[-1] = np.concatenate([np.zeros((35, 144), np.float32), last[-1]], 1)
    with pytest.raises(ops.PnrfError, match='skip'):
        ops.PackedMLP(ops.NET_REFINE, last, w['refine']['b'])
    # what is not built for skip nets raises and names skips
    rays = torch.from_numpy(ms.sampler_rays(64)).to(dev)
    for net, wts, variant in ((ops.NET_REFINE, w['refine'], 'refine_16x16'), (ops.NET_REFINE, w['refine'], 'bf16'), (ops.NET_SAMPLER, w['sampler'], 'sampler_f32_full')):
        with pytest.raises(ops.PnrfError, match='skip'):
            _mlp(ops, net, wts, variant=variant)
    with pytest.raises(ops.PnrfError, match='skip'):
        ps.forward(torch.zeros(4, 288, device=dev))                      # module-level sampler forward: the unfolded stream has no skip form
    with pytest.raises(ops.PnrfError, match='skip'):
        ops.refine_train_fwd(pr, torch.zeros(64, 144, device=dev), rays, torch.rand(64, 8, device=dev).sort(1)[0])
    # engine files: format 6 keeps the skips and the outputs
    scene = synth.make_scene(0, H=16, W=20, rotate=True)
    fr = orc.frame_setup(scene)
    r11 = fr['rays'].to(dev)
    for net, wts, packed in ((ops.NET_SAMPLER, w['sampler'], None), (ops.NET_REFINE, w['refine'], None)):
        a = _mlp(ops, net, wts)
        blob = a.serialize()
        assert int.from_bytes(blob[8:12], 'little') == 6
        b = ops.PackedMLP.deserialize(blob, expect_net=net)
        assert b.skips == [4] == a.skips
        if net == ops.NET_SAMPLER:
            oa, ob = ops.sampler_fwd(a, r11, two_pass=True), ops.sampler_fwd(b, r11, two_pass=True)
            assert all(torch.equal(x, y) for x, y in zip(oa[:5], ob[:5]))
        else:
            x = torch.rand(320, 144, device=dev)
            assert torch.equal(a.forward(x), b.forward(x))
        if net == ops.NET_SAMPLER:                                       # a module built without skips refuses the skip engine (and the other way round)
            path = str(tmp_path / 'sampler.pnrf')
            a.save(path)
            s.load_engine(path)
            assert s.packed().skips == [4]
            with pytest.raises(ops.PnrfError, match='mmnetskips'):
                h.MinMaxRaySamplerTRT_Net(D=8, input_ch=288, output_ch=27, skips=[10000]).to(dev).load_engine(path)
        old = bytearray(blob); old[8:12] = (5).to_bytes(4, 'little')
        with pytest.raises(ops.PnrfError):
            ops.PackedMLP.deserialize(bytes(old))


# ------------------------------------------------------------------------------------------------------------------ 2. exact integer nets
EXACT = [(D, tuple(sk)) for D, sets in ms.SKIP_SETS.items() for sk in sets]


@pytest.mark.parametrize('D,skips', EXACT)
def test_exact_refine(dev, D, skips):
    """Module-level forward: the exact integers, bit for bit.  Fused stage (rows from memory), both shapes: z, pts within exact_nets.TOL_Z of float64."""
    from pronerf_amd import ops
    net = ms.refine_net(4, D, list(skips))
    W, b = ms.refine_pack_weights(net)
    mlp = ops.PackedMLP(ops.NET_REFINE, W, b)
    assert mlp.skips == list(skips)
    nmax = 257
    x = en.elu_inputs(nmax, 144, seed=D)
    y = ms.exact_forward(net, x, en.LIM['f16'])
    rays, ds = en.refine_rays(nmax, seed=D)
    en.assert_refine_margin(y, rays, ds)
    z, pts, _ = en.refine_reference(y, rays, ds)
    xd, rd, dd = (torch.from_numpy(a).to(dev) for a in (x, rays, ds))
    for n in en.refine_counts(0, big=False):
        got = mlp.forward(xd[:n].contiguous()).cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(got, y[:n], err_msg=f'D {D} skips {skips} n {n}')
        for shape in ('narrow', 'wide'):
            mlp.set_shape(shape)
            zz, pp = ops.refine_fwd(mlp, xd[:n].contiguous(), rd[:n].contiguous(), dd[:n].contiguous())
            np.testing.assert_allclose(zz.cpu().numpy(), z[:n], rtol=0, atol=en.TOL_Z, err_msg=f'D {D} skips {skips} n {n} {shape}')
            np.testing.assert_allclose(pp.cpu().numpy(), pts[:n], rtol=0, atol=4 * en.TOL_Z)
        mlp.set_shape('auto')


@pytest.mark.parametrize('D,skips', EXACT)
def test_exact_sampler_f32(dev, D, skips):
    """The exact-fp32 kernel (folded stream): add / mul are the exact integers, permuted by the one order the head's depth biases fix."""
    from pronerf_amd import ops
    net = ms.sampler_net(D, list(skips))
    mlp = ops.PackedMLP(ops.NET_SAMPLER, [np.asarray(W, np.float32) for W in net['W']], [np.asarray(b, np.float32) for b in net['b']], variant='sampler_f32')
    rays = ms.sampler_rays(257, seed=D)
    y = ms.exact_forward(net, ms.sampler_inputs(rays), en.LIM['f32'])
    order = np.argsort(y[0, :8], kind='stable')
    rd = torch.from_numpy(rays).to(dev)
    for n in en.refine_counts(0, big=False):
        out = ops.sampler_fwd(mlp, rd[:n].contiguous(), want_idx=True, want_rgb=True, want_raw=True)
        np.testing.assert_array_equal(out[1].cpu().numpy(), np.tile(order, (n, 1)))
        np.testing.assert_array_equal(out[2].cpu().numpy().astype(np.float64), y[:n, 8:16][:, order], err_msg=f'add: D {D} skips {skips} n {n}')
        np.testing.assert_array_equal(out[3].cpu().numpy().astype(np.float64), y[:n, 16:24][:, order], err_msg=f'mul: D {D} skips {skips} n {n}')
        np.testing.assert_allclose(out[5].cpu().numpy(), 1 / (1 + np.exp(-y[:n, :8])), rtol=0, atol=2e-7)


@pytest.mark.parametrize('D,skips', EXACT)
def test_placement_sampler_split_and_pass1(dev, D, skips):
    """The two kernels on log2(e)-scaled streams (module docstring, 2.): pass 1 (the two-pass default: every ray of these nets is decided, so its rows are
    pass 1's; asserted) and the split-fp16 kernel, NARROW and WIDE.  add / mul within mmskips_ref.SCALED_TOL = 1e-3 of the exact integers (derived there:
    lo-plane residuals of the pre-image weights, < 4e-4), the sort order the one the head's biases fix.
    The integer inputs and activations here have lo planes of 0: the products with P_lo and X_lo' are held by tests/test_exact_sampler_gpu.py (x_big, hid_big)."""
    from pronerf_amd import ops
    net = ms.sampler_scaled_net(D, list(skips))
    W, b = ms.sampler_pack_weights(net)
    rays = ms.sampler_rays(257, seed=D)
    y = ms.exact_forward(net, ms.sampler_inputs(rays, 1), en.LIM['f16'])
    order = np.argsort(y[0, :8], kind='stable')
    rd = torch.from_numpy(rays).to(dev)
    for variant, two_pass in (('default', True), ('sampler_split', False)):
        for shp in ('narrow', 'wide'):
            mlp = ops.PackedMLP(ops.NET_SAMPLER, W, b, variant=variant).set_shape(shp)
            assert mlp.skips == list(skips)
            for n in en.refine_counts(0, big=False):
                out = ops.sampler_fwd(mlp, rd[:n].contiguous(), want_idx=True, want_rgb=True, want_raw=True, two_pass=two_pass)
                tag = f'{variant} {shp}: D {D} skips {skips} n {n}'
                if two_pass:
                    assert int(out[6]) == 0 and int(out[7]) == 0, tag          # no ray went to the second / third pass: these are pass 1's rows
                np.testing.assert_array_equal(out[1].cpu().numpy(), np.tile(order, (n, 1)), err_msg=tag)
                np.testing.assert_allclose(out[2].cpu().numpy(), y[:n, 8:16][:, order], rtol=0, atol=ms.SCALED_TOL, err_msg='add: ' + tag)
                np.testing.assert_allclose(out[3].cpu().numpy(), y[:n, 16:24][:, order], rtol=0, atol=ms.SCALED_TOL, err_msg='mul: ' + tag)


# ------------------------------------------------------------------------------------------------------------------ 3. stages vs the fp32 restatement
@pytest.mark.parametrize('name', sorted(ms.CASES))
def test_stages_vs_restatement(dev, refs, name):
    from pronerf_amd import ops
    g, shape, scene, w, fr, ref = refs[name]
    rays, or_rays = fr['rays'].to(dev), fr['or_rays'].to(dev)
    ds_ref = ref['depth_sorted']
    tie = ((ds_ref[:, 1:] - ds_ref[:, :-1]).min(1)[0] <= ms.TIE).numpy()
    for variant, two_pass in (('default', True), ('sampler_split', False), ('sampler_f32', False)):
        for shp in ('narrow', 'wide'):
            mlp = _mlp(ops, ops.NET_SAMPLER, w['sampler'], variant=variant).set_shape(shp)
            out = ops.sampler_fwd(mlp, rays, want_idx=True, want_rgb=True, want_raw=True, two_pass=two_pass)
            tag = f'{name} {variant} {shp}'
            assert int((out[1].cpu().numpy()[~tie] != ref['sort_idx'].numpy()[~tie]).any(1).sum()) == 0, tag
            derr = float((out[5].cpu() - ref['depth_raw']).abs().max())
            print(f'\n[mmskips] {tag}: indices identical on {int((~tie).sum())} of {len(tie)} rays, max depth error {derr:.2e}')
            assert derr <= (2e-3 if two_pass else 2e-6), tag
    img4 = ops.images_pack(fr['images'].to(dev).contiguous())
    proj = fr['proj'].to(dev)
    ds = ds_ref.to(dev)
    rin = ops.refine_input(rays, or_rays, ds, img4, proj)
    for shp in ('narrow', 'wide'):
        if shp == 'wide' and shape['num_neighbor'] > 4:                 # the WIDE refine form with skips is built up to num_neighbor 4: a forced WIDE says so
            with pytest.raises(ops.PnrfError, match='WIDE'):
                _mlp(ops, ops.NET_REFINE, w['refine']).set_shape(shp)
            continue
        mlp = _mlp(ops, ops.NET_REFINE, w['refine']).set_shape(shp)
        for tag, (z, pts) in (('rows', ops.refine_fwd(mlp, rin, rays, ds)), ('head', ops.refine_project_fwd(mlp, rays, or_rays, ds, img4, proj))):
            ez, ep = float((z.cpu() - ref['z']).abs().max()), float((pts.cpu() - ref['pts']).abs().max())
            print(f'[mmskips] {name} refine {tag} {shp}: max z error {ez:.2e}, max pts error {ep:.2e}')
            assert ez <= 2e-3 and ep <= 4e-3, (name, tag, shp)
    y = _mlp(ops, ops.NET_REFINE, w['refine']).forward(ref['refine_in'].to(dev).contiguous(), head_act=True)
    assert float((y[:, :8].cpu() - ref['refine_depth']).abs().max()) <= 4e-3


# ------------------------------------------------------------------------------------------------------------------ 4. frames vs the reference
def _check_against_reference(g, rgbd, idx, tag):
    tie_free = np.diff(g['depth_sorted'], axis=1).min(axis=1) > ms.TIE
    m = torch.from_numpy(tie_free)
    np.testing.assert_array_equal(idx.cpu().numpy()[tie_free], g['sort_idx'][tie_free])
    ps = orc.psnr(rgbd[:, :3].cpu()[m], torch.from_numpy(g['rgb'])[m])
    derr = float((rgbd[:, 3].cpu()[m] - torch.from_numpy(g['depth'])[m]).abs().max())
    print(f'\n[mmskips] {tag}: {int(tie_free.sum())} of {len(tie_free)} rays outside the tie set, indices identical, rgb PSNR vs the reference {ps:.1f} dB, max depth error {derr:.2e}')
    assert ps > 46.4 and derr < 2e-2 and int((~tie_free).sum()) <= 0.05 * len(tie_free)


@pytest.mark.parametrize('name', sorted(ms.CASES))
def test_frames_vs_the_reference(dev, refs, name):
    from pronerf_amd.render import Renderer
    g, shape, scene, w, fr, ref = refs[name]
    H, W = int(g['H']), int(g['W'])
    for preset in ('default', 'quality'):
        rend = Renderer(w, max_rays=H * W, device=dev, preset=preset)
        assert rend.sampler.skips == list(ms.CASES[name]) == rend.refine.skips
        np.testing.assert_array_equal(rend.set_views(scene['c2w'], scene['poses'], scene['images'], scene['K']), g['ref_nos'])
        rays, or_rays = rend.frame_rays(scene['K'], scene['c2w'], H, W)
        np.testing.assert_array_equal(rays.cpu().numpy(), g['rays'])
        rgbd, idx = rend.render_rays(rays, or_rays, want_idx=True)
        _check_against_reference(g, rgbd, idx, f'{name} [{preset}]')


@pytest.mark.parametrize('name', sorted(ms.CASES)[:2])
def test_driver_api_vs_the_reference(dev, refs, name):
    """create_nerf(args) with --mmnetskips, the reference's kwargs -> render()."""
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    g, shape, scene, w, fr, ref = refs[name]
    args = SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=shape['netdepth'], netwidth=256, mmnetdepth=shape['mmnetdepth'], mmnetwidth=256,
                           mmnetskips=list(ms.CASES[name]), N_point_ray_enc=shape['n_pts'], N_samples=8, num_neighbor=shape['num_neighbor'], ft_path=None)
    kw, _ = trt.create_nerf(args, device=dev)
    sd = synth.state_dicts(w, ms.CASES[name])
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    S, NB, Hh, Ww = 8, shape['num_neighbor'], int(g['H']), int(g['W'])
    rays, or_rays = fr['rays'].to(dev), fr['or_rays'].to(dev)
    ref_rgb = fr['images'].to(dev).unsqueeze(1).expand(-1, S, -1, -1, -1).contiguous().view(NB * S, 3, int(g['Hf']), int(g['Wf']))
    ref_pose = fr['proj'].to(dev).unsqueeze(1).expand(-1, S, -1, -1).contiguous().view(NB * S, 3, 4)
    fwd = {k: kw[k] for k in ('network_fn', 'network_query_fn', 'N_samples', 'network_fine', 'min_max_ray_net', 'refine_net', 'N_point_ray_enc',
                              'embed_fn', 'embeddirs_fn', 'num_neighbor', 'use_trt', 'embed_rays')}
    rgb0, rgb1, depth_map, _ = trt.render(rays, or_rays, (Hh, Ww, 3), mm_input=fr['mm_input'].to(dev), ref_rgb=ref_rgb, ref_pose=ref_pose, **fwd)
    tie_free = torch.from_numpy(np.diff(g['depth_sorted'], axis=1).min(axis=1) > ms.TIE)
    assert orc.psnr(rgb1.reshape(-1, 3).cpu()[tie_free], torch.from_numpy(g['rgb'])[tie_free]) > 46.4
    np.testing.assert_allclose(depth_map.reshape(-1).cpu().numpy()[tie_free.numpy()], g['depth'][tie_free.numpy()], rtol=0, atol=2e-2)


# ------------------------------------------------------------------------------------------------------------------ 5. index evidence
@pytest.mark.parametrize('D,skips', [(8, (4,)), (6, (0, 4))])
@pytest.mark.parametrize('kind', ['default', 'spread', 'trained', 'heavy', 'x4'])
def test_index_evidence_for_the_error_model(dev, D, skips, kind):
    """128 x 192 rays per weight kind: at kappa 2 and 1 no ray outside the fp32 tie set may get other sort indices from the two-pass sampler than from the
    fp32 restatement (a mismatch means the pass-1 error model with skips — DESIGN.md 4.1 — is wrong, not that kappa is too small).  "Outside ties" is
    a smallest sorted gap above 4e-6, not the 1e-6 of the reference goldens: the restatement here is torch's fp32 graph, whose summation order differs
    from the kernels' exact-fp32 chain by a few ulp of a depth (tests/test_shapes_gpu.py's full-frame test draws the same line for the same reason)."""
    from pronerf_amd import ops
    w = synth.make_weights(5, kind, mmnetdepth=D, mmnetskips=skips)['sampler']
    scene = synth.make_scene(5, H=128, W=192, rotate=True)
    rays, _ = ops.frame_rays(scene['K'], scene['c2w'], 128, 192, device=dev)
    with ms.skip_oracle(), torch.no_grad():
        _, add, mul, depth = orc.sampler_forward(w, orc.mm_input_from_rays(rays[:, 0:3].cpu(), rays[:, 3:6].cpu(), synth.N_POINT_RAY_ENC))
        ds, idx, _, _ = orc.sort_gather(depth, add, mul, rays[:, 6:7].cpu(), rays[:, 7:8].cpu())
    free = ((ds[:, 1:] - ds[:, :-1]).min(1)[0] > 4e-6).numpy()
    mlp = _mlp(ops, ops.NET_SAMPLER, w)
    for kappa in (2.0, 1.0):
        out = ops.sampler_fwd(mlp, rays, want_idx=True, two_pass=True, kappa=kappa)
        mism = int((out[1].cpu().numpy()[free] != idx.numpy()[free]).any(1).sum())
        print(f'\n[mmskips] D {D} skips {list(skips)} {kind} kappa {kappa}: {mism} mismatches on {int(free.sum())} rays outside ties, second pass {int(out[6]) / len(free):.1%}, third {int(out[7])}')
        assert mism == 0, (D, skips, kind, kappa)


# ------------------------------------------------------------------------------------------------------------------ 6. invariance
def test_narrow_wide_and_graph_capture(dev, refs):
    from pronerf_amd import ops
    g, shape, scene, w, fr, ref = refs['infer_skip_d8_s4_p48_nb4_16x20']
    rays, or_rays = fr['rays'].to(dev), fr['or_rays'].to(dev)
    img4 = ops.images_pack(fr['images'].to(dev).contiguous()); proj = fr['proj'].to(dev); ds = ref['depth_sorted'].to(dev)
    outs = {}
    for shp in ('narrow', 'wide'):
        s = _mlp(ops, ops.NET_SAMPLER, w['sampler']).set_shape(shp)
        r = _mlp(ops, ops.NET_REFINE, w['refine']).set_shape(shp)
        outs[shp] = list(ops.sampler_fwd(s, rays, two_pass=True)[:5]) + list(ops.sampler_fwd(s.set_variant('sampler_split'), rays)[:5]) + \
            list(ops.refine_project_fwd(r, rays, or_rays, ds, img4, proj))
    assert all(torch.equal(a, b) for a, b in zip(outs['narrow'], outs['wide']))
    r = _mlp(ops, ops.NET_REFINE, w['refine'])
    eager = ops.refine_project_fwd(r, rays, or_rays, ds, img4, proj)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            cap = ops.refine_project_fwd(r, rays, or_rays, ds, img4, proj)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1])
