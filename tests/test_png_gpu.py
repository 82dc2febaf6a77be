"""GPU: the device PNG encoder (pnrf_png_encode_fwd, ops.PngEncoder) held to its host twin byte for byte.

* every image of png_ref.cases (the list of tests/test_png_cpu.py, which checks the twin's files against PIL / zlib): the device file and the length
  in size_dev equal pnrf_png_encode_host's;
* the same bytes from two streams, from a captured graph replayed with the pixels changed in between, and from a second call on a workspace
  that a larger image has used (stale workspace contents must not leak);
* one frame-sized call, 756 x 1008 RGB + gray from ops.frame_to8b of a synthetic frame: decodes to those planes;
* render_path on the small synthetic data set with and without pnrf_device_png: same pixels in the files, the same float arrays, and with the
  switch off the files the parent's writer writes.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import png_ref
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def all_cases():
    from pronerf_amd import ops
    return {name: (img, flt) for name, img, flt in png_ref.cases(ops.png_segment_rows())}


def _names():
    return [n for n, _, _ in png_ref.cases(16)]


def _enc(img, dev):
    from pronerf_amd import ops
    return ops.PngEncoder(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, dev)


@pytest.mark.parametrize('name', _names())
def test_device_file_is_the_host_twins(dev, all_cases, name):
    from pronerf_amd import ops
    img, flt = all_cases[name]
    enc = _enc(img, dev)
    t = torch.from_numpy(img).to(dev)
    for f in ([flt] if flt is not None else ([-1, 0, 1, 2, 3, 4] if img.size <= 64 * 33 * 3 else [-1])):      # the threshold of the CPU list
        want = ops.png_encode_host(img, f)
        enc.out.fill_(0x5a)
        got = enc.encode(t, f)
        assert int(enc.size.item()) == len(want) == got.numel()
        assert got.cpu().numpy().tobytes() == want
        assert enc.encode_to_host(t, f) == want
    if img.shape[0] > 1:                                               # a row pitch larger than the row
        wide = torch.full((img.shape[0], img.shape[1] + 3) + img.shape[2:], 0xa5, dtype=torch.uint8, device=dev)
        wide[:, :img.shape[1]] = t
        assert enc.encode_to_host(wide[:, :img.shape[1]], f) == want


def test_streams_graph_and_a_used_workspace(dev, all_cases):
    from pronerf_amd import ops
    img, _ = all_cases['scene_rgb']
    other, _ = all_cases['noise64x33']
    want = ops.png_encode_host(img)
    t = torch.from_numpy(img).to(dev)
    encs = [_enc(img, dev), _enc(img, dev)]
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for i in range(4):
        with torch.cuda.stream(streams[i % 2]):
            encs[i % 2].launch(t)
    torch.cuda.synchronize()
    for e in encs:
        assert e.out[:int(e.size.item())].cpu().numpy().tobytes() == want
    # a captured graph, replayed with the pixels changed in between
    enc, buf = encs[0], t.clone()
    flipped = np.ascontiguousarray(img[::-1, ::-1])
    want_flipped = ops.png_encode_host(flipped)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.launch(buf)
    for pixels, w in ((img, want), (flipped, want_flipped), (img, want)):
        buf.copy_(torch.from_numpy(pixels).to(dev))
        enc.out.zero_(); enc.size.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert enc.out[:int(enc.size.item())].cpu().numpy().tobytes() == w
    # a smaller image on the workspace and the output buffer the larger one has just used
    small = _enc(other, dev)
    assert small.workspace_bytes <= enc.workspace_bytes and small.max_bytes <= enc.max_bytes
    small.workspace, small.out = enc.workspace, enc.out[:small.max_bytes]
    assert small.encode_to_host(torch.from_numpy(other).to(dev)) == ops.png_encode_host(other)
    enc.workspace.fill_(0xff)
    assert small.encode_to_host(torch.from_numpy(other).to(dev)) == ops.png_encode_host(other)


def test_a_frame_sized_call(dev):
    from pronerf_amd import ops
    H, W = 756, 1008
    yy, xx = np.mgrid[0:H, 0:W]
    rs = np.random.RandomState(0)
    img = np.stack([0.5 + 0.4 * np.sin(xx / (17.0 + 5 * c) + yy / (23.0 - 4 * c)) for c in range(3)], -1)
    rgbd = torch.empty(H * W, 4, device=dev)
    rgbd[:, :3] = torch.tensor(np.clip(img + 0.02 * rs.randn(H, W, 3), 0, 1).astype(np.float32), device=dev).reshape(-1, 3)
    rgbd[:, 3] = torch.tensor((2.0 + np.sin(xx / 90.0) * np.cos(yy / 70.0) + (xx > 400) * 1.5).astype(np.float32), device=dev).reshape(-1)
    rgb8, depth8 = ops.frame_to8b(rgbd[:, :3].reshape(H, W, 3), rgbd[:, 3].reshape(H, W))
    for plane in (rgb8, depth8):
        enc = ops.PngEncoder(H, W, 1 if plane.dim() == 2 else 3, dev)
        data = enc.encode_to_host(plane)
        assert len(data) <= enc.max_bytes
        assert np.array_equal(png_ref.decode(data), plane.cpu().numpy())
        png_ref.parse(data)                                            # every CRC, the Adler-32


def _args():
    return SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256,
                           mmnetskips=[10000], N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)


def test_render_path_with_the_files_encoded_on_the_device(dev, tmp_path):
    from pronerf_amd import run_nerf_helpers as h
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    kw, _ = trt.create_nerf(_args(), device=dev)
    sd = synth.state_dicts(synth.make_weights(0, 'trained'))
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    scene = synth.make_scene(0, H=24, W=32, n_views=6)
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
    targets = [scene['c2w'], scene['poses'][0]]
    runs = {}
    for name, opts in (('off', {}), ('on', {'pnrf_device_png': True})):
        runs[name] = trt.render_path(targets, (24, 32, scene['focal']), scene['K'], None, {**kw, **opts}, savedir=str(tmp_path / name), n_timing_reps=1, verbose=False)
    for x, y in zip(runs['off'], runs['on']):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    files = sorted(os.listdir(tmp_path / 'off'))
    assert files == sorted(os.listdir(tmp_path / 'on')) == ['000.png', '001.png', 'depth_000.png', 'depth_001.png']
    for f in files:
        off, on = (tmp_path / 'off' / f).read_bytes(), (tmp_path / 'on' / f).read_bytes()
        assert np.array_equal(png_ref.decode(off), png_ref.decode(on)), f
        png_ref.parse(on)
    for i in range(2):                                                 # switch off: the parent's files
        assert (tmp_path / 'off' / f'{i:03d}.png').read_bytes() == png_ref.parent_file(h.to8b(runs['off'][1][i]))
        d = runs['off'][2][i]
        assert (tmp_path / 'off' / f'depth_{i:03d}.png').read_bytes() == png_ref.parent_file(h.to8b(d / np.max(d)))
