"""GPU: the device JPEG encoder (pnrf_jpeg_encode_fwd, ops.JpegEncoder) held to its host twin byte for byte, and the Motion-JPEG paths.

* every image of jpeg_ref.cases (the list of tests/test_jpeg_cpu.py, which checks the twin's files against PIL and an independent decoder): the
  device file and the length in size_dev equal pnrf_jpeg_encode_host's;
* the same bytes from two streams, from a captured graph replayed with the pixels changed in between, and from a second call on a workspace and an
  output buffer that a larger image has used (stale contents must not leak);
* one frame-sized call each, 756 x 1008 RGB and gray at quality 90, against the twin;
* render_path on the small synthetic data set with pnrf_video: both AVI files hold one frame per pose, each the twin's encoding of frame_to8b's
  plane of that pose; PNG files and returned arrays are those of a run without the switch;
* Renderer.render_video on the same scene: frames equal to the twin's encoding of the planes of render_pose, the returned sizes those in the file.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_ref
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
    return {name: (img, q) for name, img, q in jpeg_ref.cases()}


def _enc(img, dev, quality=90):
    from pronerf_amd import ops
    return ops.JpegEncoder(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, dev, quality)


@pytest.mark.parametrize('name', jpeg_ref.case_names())
def test_device_file_is_the_host_twins(dev, all_cases, name):
    from pronerf_amd import ops
    img, q = all_cases[name]
    want = ops.jpeg_encode_host(img, q)
    enc = _enc(img, dev, q)
    t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    enc.out.fill_(0x5a)
    got = enc.encode(t)
    assert int(enc.size.item()) == len(want) == got.numel()
    assert got.cpu().numpy().tobytes() == want
    assert (enc.out[len(want):] == 0x5a).all()                         # nothing behind the file
    assert enc.encode_to_host(t) == want
    assert enc.encode_to_host(t, 37) == ops.jpeg_encode_host(img, 37)   # a quality per call
    wide = torch.full((img.shape[0], img.shape[1] + 3) + img.shape[2:], 0xa5, dtype=torch.uint8, device=dev)      # a row pitch larger than the row
    wide[:, :img.shape[1]] = t
    view = wide[:, :img.shape[1]]
    assert img.shape[0] == 1 or not view.is_contiguous()
    assert enc.encode_to_host(view) == want


def test_streams_graph_and_a_used_workspace(dev, all_cases):
    from pronerf_amd import ops
    img, _ = all_cases['scene_rgb']
    other, _ = all_cases['noise_rgb']
    want = ops.jpeg_encode_host(img, 90)
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
    want_flipped = ops.jpeg_encode_host(flipped, 90)
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
    small = _enc(other, dev, 100)
    assert small.workspace_bytes <= enc.workspace_bytes and small.max_bytes <= enc.max_bytes
    small.workspace, small.out = enc.workspace, enc.out[:small.max_bytes]
    assert small.encode_to_host(torch.from_numpy(other).to(dev)) == ops.jpeg_encode_host(other, 100)
    enc.workspace.fill_(0xff)
    assert small.encode_to_host(torch.from_numpy(other).to(dev)) == ops.jpeg_encode_host(other, 100)


def test_frame_sized_calls(dev):
    from pronerf_amd import ops
    H, W = 756, 1008
    yy, xx = np.mgrid[0:H, 0:W]
    rs = np.random.RandomState(0)
    img = np.stack([0.5 + 0.4 * np.sin(xx / (17.0 + 5 * c) + yy / (23.0 - 4 * c)) for c in range(3)], -1)
    rgb = (255 * np.clip(img + 0.02 * rs.randn(H, W, 3), 0, 1)).astype(np.uint8)
    gray = (255 * np.clip((2.0 + np.sin(xx / 90.0) * np.cos(yy / 70.0) + (xx > 400) * 1.5) / 4.5, 0, 1)).astype(np.uint8)
    for plane in (rgb, gray):
        enc = _enc(plane, dev, 90)
        data = enc.encode_to_host(torch.from_numpy(plane).to(dev))
        assert len(data) <= enc.max_bytes and data == ops.jpeg_encode_host(plane, 90)


def _args():
    return SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, mmnetdepth=6, mmnetwidth=256,
                           mmnetskips=[10000], N_point_ray_enc=48, N_samples=8, num_neighbor=4, ft_path=None)


@pytest.fixture(scope='module')
def small_scene(dev):
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    kw, _ = trt.create_nerf(_args(), device=dev)
    sd = synth.state_dicts(synth.make_weights(0, 'trained'))
    kw['min_max_ray_net'].load_state_dict(sd['sampler']); kw['refine_net'].load_state_dict(sd['refine']); kw['network_fine'].load_state_dict(sd['nerf'])
    scene = synth.make_scene(0, H=24, W=32, n_views=6)
    kw.update(poses=scene['poses'], images=scene['images'], ref_K=scene['K'])
    return kw, scene, [scene['c2w'], scene['poses'][0], scene['poses'][1]]


def _frames(path):
    data = open(path, 'rb').read()
    chunks = jpeg_ref.riff_walk(data)
    return [data[body:body + size] for p, _, body, size in chunks if p.endswith('/00dc')]


def test_render_path_with_video(dev, small_scene, tmp_path):
    from pronerf_amd import ops
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    kw, scene, targets = small_scene
    runs = {}
    for name, opts in (('off', {}), ('on', {'pnrf_video': {'fps': 24, 'quality': 85}}), ('default', {'pnrf_video': True, 'pnrf_device_png': True})):
        runs[name] = trt.render_path(targets, (24, 32, scene['focal']), scene['K'], None, {**kw, **opts}, savedir=str(tmp_path / name), n_timing_reps=1, verbose=False)
    pngs = ['000.png', '001.png', '002.png', 'depth_000.png', 'depth_001.png', 'depth_002.png']
    assert sorted(os.listdir(tmp_path / 'off')) == pngs
    assert sorted(os.listdir(tmp_path / 'on')) == sorted(os.listdir(tmp_path / 'default')) == pngs + ['video.avi', 'video_depth.avi']
    for x, y, z in zip(runs['off'], runs['on'], runs['default']):
        assert x.dtype == np.float32 and np.array_equal(x, y) and np.array_equal(x, z)
    for f in pngs:                                                     # the switch leaves the PNG files alone
        assert (tmp_path / 'off' / f).read_bytes() == (tmp_path / 'on' / f).read_bytes()
    for name, quality in (('on', 85), ('default', 90)):
        rgb_frames, depth_frames = _frames(tmp_path / name / 'video.avi'), _frames(tmp_path / name / 'video_depth.avi')
        assert len(rgb_frames) == len(depth_frames) == len(targets)
        for i in range(len(targets)):
            rgb8, depth8 = ops.frame_to8b(torch.from_numpy(runs[name][1][i]).to(dev), torch.from_numpy(runs[name][2][i]).to(dev))
            assert rgb_frames[i] == ops.jpeg_encode_host(rgb8.cpu().numpy(), quality), (name, i)
            assert depth_frames[i] == ops.jpeg_encode_host(depth8.cpu().numpy(), quality), (name, i)


def test_render_video(dev, small_scene, tmp_path):
    from pronerf_amd import ops
    from pronerf_amd import run_S_eS_eN_alter_trt as trt
    from pronerf_amd._lib import PnrfError
    kw, scene, targets = small_scene
    H, W = 24, 32
    rend = trt._renderer(kw['min_max_ray_net'], kw['refine_net'], kw['network_fine'], H * W, dev)
    rend.scene = None
    with pytest.raises(PnrfError):
        rend.render_video(targets, H, W, str(tmp_path / 'v.avi'))
    try:
        rend.set_scene(scene['poses'], scene['images'], scene['K'], scene['K'])
        poses = targets + targets[::-1]                                # five poses: both pinned buffers are reused
        poses = poses[:5]
        sizes = rend.render_video(poses, H, W, str(tmp_path / 'v.avi'), fps=25, quality=80, depth_path=str(tmp_path / 'd.avi'))
        only = rend.render_video(poses[:2], H, W, str(tmp_path / 'w.avi'))
        rgb_frames, depth_frames = _frames(tmp_path / 'v.avi'), _frames(tmp_path / 'd.avi')
        assert [(len(a), len(b)) for a, b in zip(rgb_frames, depth_frames)] == sizes and len(sizes) == len(poses)
        assert [len(f) for f in _frames(tmp_path / 'w.avi')] == only and len(only) == 2
        for i, c2w in enumerate(poses):
            rgbd = rend.render_pose(c2w, H, W)
            rgb8, depth8 = ops.frame_to8b(rgbd[:, 0:3].reshape(H, W, 3), rgbd[:, 3].reshape(H, W))
            assert rgb_frames[i] == ops.jpeg_encode_host(rgb8.cpu().numpy(), 80), i
            assert depth_frames[i] == ops.jpeg_encode_host(depth8.cpu().numpy(), 80), i
            if i < 2:
                assert _frames(tmp_path / 'w.avi')[i] == ops.jpeg_encode_host(rgb8.cpu().numpy(), 90)
    finally:
        rend.scene = rend._pose_ws = None
