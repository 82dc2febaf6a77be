"""GPU: pnrf_mlp_repack / pnrf_trainer_publish — a handle rewritten in place on the device from device weights holds, byte for byte, the image the
host packer writes for those weights (one statement of the element rules, pnrf_pack_rules.h); refusals leave it untouched; renderers and captured
graphs built on the handles follow; the trainer publishes without a read-back, also between forward and backward, also from a captured graph; the
drivers' hold-out render on the inference path (evaluate_views(path='render')).

Measured on one MI355X: evaluate_views on the 16 x 20 synthetic scene, stage 2, fixture weights: path='render' lies 0.019 and 0.017 dB above
path='train' on the two hold-out views (10.05 / 10.33 dB against 10.03 / 10.32 dB; printed by test_driver_render_path)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

import pack_cases as pc
from oracle import pronerf_oracle as orc
from oracle import synth
from train_golden_util import load_case

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE = -1, -2
SEED_B = 11


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def case_b(name):
    """The case's shape with a second seeded set of weights."""
    if name == 'nerfcls':
        return (pc.NET_NERFCLS,) + pc.cls_stack(synth.make_nerfcls_weights(SEED_B))
    c, n = name.split('-')
    w = synth.make_weights(SEED_B, 'trained', **pc.SHAPES[c][0])[n]
    return pc.NETS[n], w['W'], w['b']


def to_dev(arrs, dev):
    return [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrs]


def image(net, W, b):
    from pronerf_amd import ops
    return ops.PackedMLP.pack_image(net, W, b)


# ------------------------------------------------------------------------------------------------ 1. byte identity
@pytest.mark.parametrize('name', pc.NAMES)
def test_repacked_handle_serializes_to_the_host_packers_image(dev, name):
    from pronerf_amd import ops
    net, WA, bA = pc.case(name)
    _, WB, bB = case_b(name)
    imgA, imgB = image(net, WA, bA), image(net, WB, bB)
    assert imgA != imgB and len(imgA) == len(imgB)
    h = ops.PackedMLP(net, WA, bA)
    assert h.serialize() == imgA
    assert h.repack(to_dev(WB, dev), to_dev(bB, dev)) is h
    assert h.serialize() == imgB                                  # checksum included
    h.repack(to_dev(WA, dev), to_dev(bA, dev))                    # nothing stale in the plan or its scratch
    assert h.serialize() == imgA
    h2 = ops.PackedMLP.deserialize(imgB, expect_net=net)          # a handle that never saw pnrf_mlp_pack: the header's shape fields suffice
    h2.repack(to_dev(WA, dev), to_dev(bA, dev))
    assert h2.serialize() == imgA


# ------------------------------------------------------------------------------------------------ 2. rounding corners
CORNER_CASES = ['smallest-sampler', 'smallest-refine', 'smallest-nerf', 'skip02-sampler', 'skip02-refine', 'nerfcls']
TIES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]
FLT_MAX = float(np.finfo(np.float32).max)
# +-0, fp32 subnormals, beyond the fp16 range (and below its subnormals), the exact fp16 / bf16 round-to-even ties and their negatives
CORNERS = [0.0, -0.0, 1e-40, -1e-42, 1.4e-45, 7e4, -1e5, 65520.0, 65519.996, 1e-8, -2.98e-8, 6e-8] + TIES + [-t for t in TIES]


def planted(W, b, values, seed, once=()):
    """Copies of the matrices with `values` written at seeded places of every matrix and bias vector; `once`: values written once per matrix only."""
    rs = np.random.RandomState(seed)
    W = [np.array(w, dtype=np.float32) for w in W]; b = [np.array(x, dtype=np.float32) for x in b]
    for a in W + b:
        flat = a.reshape(-1)
        reps = max(1, min(8, flat.size // (4 * len(values))))
        at = rs.choice(flat.size, size=min(flat.size, reps * len(values)), replace=False)
        flat[at] = np.resize(np.asarray(values, dtype=np.float32), at.size)
        if once and flat.size > 64:
            flat[rs.choice(flat.size, size=len(once), replace=False)] = np.asarray(once, dtype=np.float32)
    return W, b


# element width of the 14 sections of an image per net kind (file order, EngineHeader): 2 = fp16 / bf16, 4 = fp32, 0 = integer maps
SECTION_COUNTS = ['nslots', 'nslots_fold', 'nslots_h16', 'nslots_b16', 'nbias_b16', 'nbias', 'n_in0', 'n_inx', 'n_out', 'n_tvals', 'nslots_p1', 'nbias_p1', 'n_p1c', 'nslots_f16']
STREAM_WIDTH = {pc.NET_SAMPLER: {'nslots': 4, 'nslots_fold': 4, 'nslots_h16': 2, 'nslots_p1': 2},
                pc.NET_REFINE: {'nslots': 2, 'nslots_fold': 2, 'nslots_b16': 2, 'nslots_f16': 2},
                pc.NET_NERF: {'nslots': 2, 'nslots_b16': 2, 'nslots_f16': 2}, pc.NET_NERFCLS: {'nslots': 2, 'nslots_b16': 2, 'nslots_f16': 2}}


def sections(img, net):
    """-> [(name, element width, payload bytes)] of an engine image"""
    hd = struct.unpack_from('<8s4I5i4I6iIQQI2iI3H', img, 0)
    cnt = dict(zip(SECTION_COUNTS[:10], hd[10:20]))
    cnt.update(nslots_p1=hd[23], nbias_p1=hd[24], n_p1c=hd[25], nslots_f16=hd[26])
    out, off = [], 128
    for s in SECTION_COUNTS:
        stream = s.startswith('nslots')
        size = cnt[s] * (16384 if stream else 4)
        width = STREAM_WIDTH[net].get(s, 0) if stream else (4 if s in ('nbias_b16', 'nbias', 'nbias_p1', 'n_p1c', 'n_tvals') else 0)
        assert not (stream and size and not width), s
        out.append((s, width, img[off:off + size]))
        off += size
    assert off == len(img)
    return out


@pytest.mark.parametrize('name', CORNER_CASES)
def test_rounding_corners_are_byte_identical(dev, name):
    from pronerf_amd import ops
    net, W, b = pc.case(name)
    h = ops.PackedMLP(net, W, b)
    Wc, bc = planted(W, b, CORNERS, 5, once=[FLT_MAX])
    h.repack(to_dev(Wc, dev), to_dev(bc, dev))
    want = image(net, Wc, bc)
    got = h.serialize()
    for (s, _, x), (_, _, y) in zip(sections(want, net), sections(got, net)):
        assert x == y, (s, int((np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8)).sum()))
    assert got == want


@pytest.mark.parametrize('name', CORNER_CASES)
def test_nan_and_inf_land_where_the_host_puts_them(dev, name):
    from pronerf_amd import ops
    net, W, b = pc.case(name)
    h = ops.PackedMLP(net, W, b)
    Wn, bn = planted(W, b, [float('nan'), float('inf'), -float('inf'), 1.0], 6)
    h.repack(to_dev(Wn, dev), to_dev(bn, dev))
    want, got = image(net, Wn, bn), h.serialize()
    assert want[:96] == got[:96] and want[104:128] == got[104:128]           # the header but for the checksum (NaN payloads may differ)
    n_nan = 0
    for (s, width, x), (_, _, y) in zip(sections(want, net), sections(got, net)):
        if width == 0:
            assert x == y, s
            continue
        u = np.uint16 if width == 2 else np.uint32
        x, y = np.frombuffer(x, u), np.frombuffer(y, u)
        if width == 4:
            nx, ny = np.isnan(x.view(np.float32)), np.isnan(y.view(np.float32))
        elif s == 'nslots' or (s == 'nslots_b16' and net != pc.NET_REFINE):     # bf16
            nx, ny = (x & 0x7fff) > 0x7f80, (y & 0x7fff) > 0x7f80
        else:                                                                   # fp16
            nx, ny = (x & 0x7fff) > 0x7c00, (y & 0x7fff) > 0x7c00
        assert np.array_equal(nx, ny), (s, int(nx.sum()), int(ny.sum()))
        assert np.array_equal(x[~nx], y[~nx]), s
        n_nan += int(nx.sum())
    assert n_nan > 0


# ------------------------------------------------------------------------------------------------ 3. refusals
def mm_dims(in0, out, depth, skips=()):
    return [(in0, 256)] + [(256 + in0 if (l - 1) in skips else 256, 256) for l in range(1, depth)] + [(256, out)]


def zeros(dims, dev=None):
    if dev is None:
        return [np.zeros((o, i), np.float32) for i, o in dims], [np.zeros(o, np.float32) for i, o in dims]
    return [torch.zeros(o, i, device=dev) for i, o in dims], [torch.zeros(o, device=dev) for i, o in dims]


def cls_dims():
    return [(63, 256)] + [(256 + 63 if l == 5 else 256, 256) for l in range(1, 8)] + [(256, 256), (256, 1), (256 + 27, 128), (128, 3)]


REFUSALS = {
    'another depth': (pc.NET_SAMPLER, mm_dims(6, 27, 2), mm_dims(6, 27, 3), E_SHAPE),
    'another P': (pc.NET_SAMPLER, mm_dims(6, 27, 2), mm_dims(12, 27, 2), E_SHAPE),
    'another nb': (pc.NET_REFINE, mm_dims(72, 35, 2), mm_dims(96, 35, 2), E_SHAPE),
    'another skip set': (pc.NET_SAMPLER, mm_dims(6, 27, 4, (0, 2)), mm_dims(6, 27, 4, (0, 1)), E_SHAPE),
    'DoNeRFTRT weights into a NeRF-class handle': (pc.NET_NERFCLS, cls_dims(), [(63, 256), (256, 256), (256 + 27, 4)], E_SHAPE),
    'a null pointer': (pc.NET_REFINE, mm_dims(72, 35, 2), None, E_ARG),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals_leave_the_handle_untouched(dev, what):
    from pronerf_amd import _lib, ops
    from pronerf_amd.ops import PnrfError
    net, have, given, code = REFUSALS[what]
    rs = np.random.RandomState(1)
    W0 = [rs.randn(o, i).astype(np.float32) * 0.05 for i, o in have]; b0 = [rs.randn(o).astype(np.float32) * 0.05 for i, o in have]
    h = ops.PackedMLP(net, W0, b0)
    before = h.serialize()
    lib = _lib.load()
    for warm in (False, True):                     # with and without a plan on the handle
        if warm:
            h.repack(to_dev(W0, dev), to_dev(b0, dev))
            assert h.serialize() == before
        W, b = zeros(given if given is not None else have, dev)
        n = len(W)
        Wp = (C.c_void_p * n)(*[w.data_ptr() for w in W]); bp = (C.c_void_p * n)(*[x.data_ptr() for x in b])
        if given is None:
            Wp[1] = None
        ind = (C.c_int * n)(*[w.shape[1] for w in W]); outd = (C.c_int * n)(*[w.shape[0] for w in W])
        rc = lib.pnrf_mlp_repack(h.handle, Wp, bp, ind, outd, n, None)
        msg = lib.pnrf_last_error().decode()
        assert rc == code and len(msg) > 20, (rc, msg)
        if code == E_SHAPE and what != 'DoNeRFTRT weights into a NeRF-class handle':
            assert msg.count('hidden layers') == 2 and 'skip mask' in msg, msg      # both shapes are named
        if given is not None:
            with pytest.raises(PnrfError):
                h.repack(W, b)
        torch.cuda.synchronize()
        assert h.serialize() == before


def test_cpu_tensors_and_arrays_are_refused(dev):
    from pronerf_amd import ops
    from pronerf_amd.ops import PnrfError
    net, W, b = pc.case('smallest-nerf')
    h = ops.PackedMLP(net, W, b)
    before = h.serialize()
    with pytest.raises(PnrfError, match='GPU tensor'):
        h.repack([torch.as_tensor(w) for w in W], [torch.as_tensor(x) for x in b])
    with pytest.raises(PnrfError, match='GPU tensor'):
        h.repack(W, b)
    with pytest.raises(PnrfError, match='float32'):
        h.repack([t.double() for t in to_dev(W, dev)], to_dev(b, dev))
    assert h.serialize() == before


# ------------------------------------------------------------------------------------------------ 4. the renderer follows
def _renderer_weights(seed, kind):
    w = synth.make_weights(seed, 'trained', **({'mmnetskips': [4]} if kind == 'skip' else {}))
    if kind == 'nerfcls':
        Wc, bc = pc.cls_stack(synth.make_nerfcls_weights(seed))
        w = {**w, 'nerf': {'W': Wc, 'b': bc}}
    return {k: w[k] for k in ('sampler', 'refine', 'nerf')}


@pytest.mark.parametrize('kind', ['nerf', 'nerfcls', 'skip'])
def test_renderer_and_its_captured_graph_follow_a_repack(dev, kind):
    from pronerf_amd.render import Renderer
    H, W = 16, 20
    scene = synth.make_scene(0, H=H, W=W, n_views=6)
    A, B = _renderer_weights(3, kind), _renderer_weights(SEED_B, kind)
    rend = Renderer(A, max_rays=H * W, device=dev)
    rend.set_scene(scene['poses'], scene['images'], scene['K'])
    c2w = torch.from_numpy(np.ascontiguousarray(scene['c2w'][:3, :4])).to(dev)
    graph = rend.capture_pose(H, W)
    before = rend.render_pose(c2w, H, W).clone()
    assert torch.equal(graph.replay(c2w), before)
    for net in ('sampler', 'refine', 'nerf'):
        getattr(rend, net).repack(to_dev(B[net]['W'], dev), to_dev(B[net]['b'], dev))
    fresh = Renderer(B, max_rays=H * W, device=dev)
    fresh.set_scene(scene['poses'], scene['images'], scene['K'])
    want = fresh.render_pose(c2w, H, W).clone()
    assert not torch.equal(want, before)
    assert torch.equal(rend.render_pose(c2w, H, W), want)
    assert torch.equal(graph.replay(c2w), want)


# ------------------------------------------------------------------------------------------------ 5. / 6. trainer publish
@pytest.fixture(scope='module')
def fern(golden_dir):
    return load_case(golden_dir, 'stage2_step_12x16')[1]


def cu(t, dev):
    return torch.as_tensor(t).to(dev).contiguous()


def _trainer(b, dev):
    from pronerf_amd import ops
    layers = orc.trainer_layers(b['w'])
    return ops.Trainer([W for W, _ in layers], [x for _, x in layers], max_rays=b['N'], device=dev), layers


def _batch(b, dev):
    from pronerf_amd import ops
    return dict(head=(cu(b['rays'], dev), cu(b['or_rays'], dev)), target=cu(b['target'], dev),
                tail=(ops.images_pack(cu(b['images'], dev)), cu(b['poses'], dev), cu(b['K'], dev), b['ref_nos'].to(dev).contiguous()),
                jitter=cu(b['jitter'], dev), noise=cu(b['noise'], dev))


def _handles(layers):
    from pronerf_amd import ops
    nets = ((ops.NET_SAMPLER, layers[0:7]), (ops.NET_REFINE, layers[7:14]), (ops.NET_NERFCLS, layers[14:26]))
    return [ops.PackedMLP(net, [W for W, _ in ls], [x for _, x in ls]) for net, ls in nets]


def _images_of(tr):
    from pronerf_amd import ops
    from pronerf_amd.run_S_eS_eN_alter_base_refine2 import _FINE_KEYS, _MM_KEYS, state_dicts_from_trainer
    out = []
    for net, sd, keys in zip((ops.NET_SAMPLER, ops.NET_REFINE, ops.NET_NERFCLS), state_dicts_from_trainer(tr), (_MM_KEYS, _MM_KEYS, _FINE_KEYS)):
        out.append(image(net, [sd[k + '.weight'] for k in keys], [sd[k + '.bias'] for k in keys]))
    return out


def test_trainer_publish(dev, fern):
    from pronerf_amd import ops
    from pronerf_amd.ops import PnrfError
    b = fern
    tr, layers = _trainer(b, dev)
    B = _batch(b, dev)
    hs = _handles(layers)
    initial = [h.serialize() for h in hs]
    for _ in range(2):
        tr.fwd_bwd(*B['head'], B['target'], *B['tail'], jitter=B['jitter'], jitter_dir=b['jdir'], raw_noise=B['noise'], white_bkgd=b['white'], a_mmrgb=b['a_mmrgb'])
        tr.adam_step(b['lr'])
    assert tr.publish(*hs) is tr
    want = _images_of(tr)
    got = [h.serialize() for h in hs]
    assert got == want and all(g != i for g, i in zip(got, initial))
    tr.publish(fine=hs[2]); tr.publish(sampler=hs[0]); tr.publish()                    # any of the three may be missing
    assert [h.serialize() for h in hs] == want

    # a DoNeRFTRT handle as the fine net, a sampler where the refine net goes: refused, nothing launched for the others
    w = synth.make_weights(3, 'trained')
    donerf = ops.PackedMLP(ops.NET_NERF, w['nerf']['W'], w['nerf']['b'])
    kept = donerf.serialize()
    tr.write('param', 0, W=torch.as_tensor(np.asarray(layers[0][0])).to(dev) * 0.5)        # the trainer has moved on; a refused publish must not show it
    with pytest.raises(PnrfError, match='net kind'):
        tr.publish(hs[0], hs[1], donerf)
    with pytest.raises(PnrfError):
        tr.publish(hs[0], hs[0], None)
    assert donerf.serialize() == kept and [h.serialize() for h in hs] == want

    # between forward and backward: the pair stays whole, the gradients are those of a run without the publish
    def pair(publish):
        maps = tr.forward(*B['head'], *B['tail'], jitter=B['jitter'], jitter_dir=b['jdir'], raw_noise=B['noise'], white_bkgd=b['white'])
        if publish:
            tr.publish(*hs)
        tr.backward(rgb_map1=2.0 * (maps['rgb_map1'] - B['target']) / maps['rgb_map1'].numel())
        return [t for i in range(26) for t in tr.read('grad', i)]
    plain, with_publish = pair(False), pair(True)
    assert all(torch.equal(x, y) for x, y in zip(plain, with_publish))
    assert [h.serialize() for h in hs] == _images_of(tr)


def test_publish_captured_in_a_graph(dev, fern):
    tr, layers = _trainer(fern, dev)
    hs = _handles(layers)
    tr.publish(*hs)                                                # the warm call: the plans are built outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.publish(*hs)
    rs = np.random.RandomState(2)
    for li in (0, 3, 7, 13, 14, 19, 22, 23, 24, 25):               # every net, the NeRF class's skip layer and all four heads
        Wl, bl = layers[li]
        tr.write('param', li, W=torch.as_tensor(np.asarray(Wl) + rs.randn(*np.shape(Wl)).astype(np.float32) * 0.01).to(dev),
                 b=torch.as_tensor(np.asarray(bl) + rs.randn(*np.shape(bl)).astype(np.float32) * 0.01).to(dev))
    want = _images_of(tr)
    assert [h.serialize() for h in hs] != want
    g.replay()
    torch.cuda.synchronize()
    assert [h.serialize() for h in hs] == want


# ------------------------------------------------------------------------------------------------ 7. the drivers' hold-out render
def test_driver_render_path(dev, fern):
    from pronerf_amd.render import Renderer
    from pronerf_amd.run_S_eS_eN_alter_base_refine2 import _FINE_KEYS, _MM_KEYS, eval_renderer, evaluate_views, state_dicts_from_trainer
    H, W = 16, 20
    scene = synth.make_scene(0, H=H, W=W, n_views=8, sigma_t=0.2, rotate=True)
    test, train = [0, 5], [1, 2, 3, 4, 6, 7]
    poses, images, K = scene['poses'], scene['images'], scene['K']
    tr, _ = _trainer(fern, dev)
    args = (tr, 2, poses[test], images[test], images[train], poses[train], K, H, W)
    train_before = evaluate_views(*args)
    render = evaluate_views(*args, path='render')
    assert evaluate_views(*args, path='train') == train_before == evaluate_views(*args)
    rend = eval_renderer(tr, images[train], poses[train], K, H, W)
    # the weights move: the kept renderer follows, and its frames are those of a renderer built from the state dicts
    tr.write('param', 25, b=torch.tensor([0.3, -0.2, 0.1], device=dev))
    render2 = evaluate_views(*args, path='render')
    assert eval_renderer(tr, images[train], poses[train], K, H, W) is rend and render2 != render
    nets = dict(zip(('sampler', 'refine', 'nerf'), zip(state_dicts_from_trainer(tr), (_MM_KEYS, _MM_KEYS, _FINE_KEYS))))
    fresh = Renderer({n: {'W': [sd[k + '.weight'] for k in keys], 'b': [sd[k + '.bias'] for k in keys]} for n, (sd, keys) in nets.items()}, H * W, device=dev)
    fresh.set_scene(poses[train][:, :3, :4], images[train], K)
    for c2w in poses[test]:
        assert torch.equal(rend.render_pose(c2w[:3, :4], H, W).clone(), fresh.render_pose(c2w[:3, :4], H, W))
    train2 = evaluate_views(*args)
    print('evaluate_views PSNR (dB) train path', train2, 'render path', render2, 'difference', [r - t for r, t in zip(render2, train2)])
    assert all(np.isfinite(render2)) and len(render2) == len(test)
