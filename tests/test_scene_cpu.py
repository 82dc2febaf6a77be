"""CPU: the device-resident scene's entry points refuse bad arguments before any device work (there is no GPU here: reaching one would fail
differently), and the host restatement of the projection arithmetic that tests/test_scene_gpu.py compares the kernel with is itself within the
derived bound of the exact product — as is the fp32 matmul of render.projection_matrices."""
import ctypes as C

import numpy as np
import pytest

from oracle import synth
from scene_ref import proj_exact_and_bound, proj_f64


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _scene(lib, nv, Hf, Wf, fmt):
    h = C.c_void_p()
    rc = lib.pnrf_scene_create(nv, Hf, Wf, fmt, C.byref(h))
    return rc, h


def test_scene_argument_errors_are_reported_before_any_device_work(lib):
    for nv in (0, 4097, -3):
        rc, h = _scene(lib, nv, 4, 4, 0)
        assert rc == -1 and not h.value and b'pnrf_scene_create' in lib.pnrf_last_error(), nv
    rc, h = _scene(lib, 4, 4, 4, 2)
    assert rc == -1 and not h.value and b'format' in lib.pnrf_last_error()
    assert _scene(lib, 4, 0, 4, 0)[0] == -1
    assert lib.pnrf_scene_create(4, 4, 4, 0, None) == -1
    # creation itself does no device work: both ends of the view range are accepted without a GPU
    pose = (C.c_float * 12)(1, 0, 0, 0.5, 0, 1, 0, 0.25, 0, 0, 1, 0)
    img = (C.c_float * (4 * 4 * 4))()                      # never dereferenced: every call below is refused on the host
    fp = C.POINTER(C.c_float)
    for nv in (1, 4096):
        rc, h = _scene(lib, nv, 4, 4, 0)
        assert rc == 0 and h.value
        assert lib.pnrf_scene_free(h) == 0
    rc, f32 = _scene(lib, 5, 4, 4, 0)
    rc2, u8 = _scene(lib, 5, 4, 4, 1)
    assert rc == 0 and rc2 == 0
    try:
        img_p = C.cast(img, C.c_void_p)
        assert lib.pnrf_scene_set_view(None, 0, img_p, 0, 3, pose, None) == -1
        for stride in (2, 5, 0):
            assert lib.pnrf_scene_set_view(f32, 0, img_p, 0, stride, pose, None) == -1 and b'pix_stride' in lib.pnrf_last_error()
        for v in (-1, 5):
            assert lib.pnrf_scene_set_view(f32, v, img_p, 0, 3, pose, None) == -1
        assert lib.pnrf_scene_set_view(f32, 0, img_p, 2, 3, pose, None) == -1 and b'img_dtype' in lib.pnrf_last_error()
        assert lib.pnrf_scene_set_view(f32, 0, None, 0, 3, pose, None) == -1
        assert lib.pnrf_scene_set_view(f32, 0, img_p, 0, 3, None, None) == -1
        # fp32 pixels into an RGBA8 cache would be quantised: refused, for either pixel stride
        for stride in (3, 4):
            assert lib.pnrf_scene_set_view(u8, 0, img_p, 0, stride, pose, None) == -1 and b'uint8 images only' in lib.pnrf_last_error()
        for bad in (float('nan'), float('inf'), -float('inf')):
            for at in (0, 3, 11):
                p = (C.c_float * 12)(*pose)
                p[at] = bad
                assert lib.pnrf_scene_set_view(f32, 1, img_p, 0, 3, p, None) == -1 and b'not finite' in lib.pnrf_last_error()
        nanK = (C.c_float * 9)(*([1.0] * 8 + [float('nan')]))
        okK = (C.c_float * 9)(*([1.0] * 9))
        assert lib.pnrf_scene_set_intrinsics(f32, nanK, okK) == -1 and lib.pnrf_scene_set_intrinsics(f32, okK, nanK) == -1
        assert lib.pnrf_scene_set_intrinsics(f32, None, okK) == -1
        # selection: the neighbour count is checked against 1 .. 8 and the scene's views before anything else
        one = C.c_void_p(16)                              # non-null stand-ins for device pointers, never dereferenced
        for nb in (0, 9, 6, -1):
            assert lib.pnrf_scene_select_fwd(f32, one, nb, one, one, one, None) == -1 and b'nb must be' in lib.pnrf_last_error(), nb
        assert lib.pnrf_scene_select_fwd(None, one, 4, one, one, one, None) == -1
        assert lib.pnrf_scene_select_fwd(f32, one, 4, one, one, one, None) == -3 and b'not complete' in lib.pnrf_last_error()     # no view set yet
        n = C.c_int64()
        for nb in (0, 9, 6):
            assert lib.pnrf_render_pose_workspace_bytes(f32, nb, 100, C.byref(n)) == -1
        assert lib.pnrf_render_pose_workspace_bytes(f32, 4, 100, C.byref(n)) == 0
        assert n.value >= 8 * 4 + 4 * 12 * 4 + 4 * 4 * 4 * 16 + 2 * 100 * 44 and n.value % 256 == 0
        assert lib.pnrf_render_pose_fwd(None, f32, one, 4, 4, 4, 0, 1, 1, 10, 0, 16, 0, 16, 1e-5, one, 1 << 20, one, None, None) == -1
        # the camera-from-device ray entry point validates like pnrf_frame_rays_blocks_fwd
        assert lib.pnrf_frame_rays_dev_fwd(one, one, 4, 4, 0, 1, 1, 10, 0, 16, 0, 17, one, one, None) == -1      # leaves the frame
        assert lib.pnrf_frame_rays_dev_fwd(one, one, 4, 4, 0, 1, 1, 10, 0, 4, 2, 8, one, one, None) == -1        # blocks overlap
        assert lib.pnrf_frame_rays_dev_fwd(None, one, 4, 4, 0, 1, 1, 10, 0, 16, 0, 16, one, one, None) == -1
        assert lib.pnrf_frame_rays_dev_fwd(one, one, 4, 4, 0, 1, 1, 10, 0, 16, 0, 0, one, one, None) == 0         # empty range: a no-op
    finally:
        lib.pnrf_scene_free(f32); lib.pnrf_scene_free(u8)


def test_python_wrappers_refuse_host_tensors_and_unknown_caches():
    import torch
    from pronerf_amd import ops
    with pytest.raises(ops.PnrfError):
        ops.Scene(4, 4, 4, cache='f16')
    with pytest.raises(ops.PnrfError):
        ops.Scene(4, 4, 4, device='cpu')
    with pytest.raises(ops.PnrfError):
        ops.frame_rays_dev(torch.eye(3), torch.eye(3, 4), 4, 4)


def test_uint8_texels_expand_to_the_loaders_floats():
    """The kernels expand a byte k with ONE correctly rounded fp32 division k / 255; load_llff's images are (k / 255.).astype(float32) (a float64
    quotient rounded to fp32).  The two agree for all 256 values."""
    k = np.arange(256)
    one_rounding = np.float32(k) / np.float32(255)
    assert one_rounding.dtype == np.float32
    np.testing.assert_array_equal(one_rounding, (k / 255.).astype(np.float32))


def _cases():
    out = []
    for seed in range(4):
        s = synth.make_scene(seed, n_views=6, rotate=bool(seed % 2), sigma_t=0.05 if seed < 2 else 0.6)
        out.append((s['K'], s['poses']))
    rs = np.random.RandomState(5)
    K = np.array([[815.13, 0.3, 504.0], [0, 790.2, 378.0], [0, 0, 1]], np.float32)
    out.append((K, (rs.randn(40, 3, 4) * np.array([1, 1, 1, 30.0])).astype(np.float32)))
    return out


def test_projection_restatement_and_host_matmul_lie_within_the_derived_bound():
    from pronerf_amd.render import projection_matrices
    for K, poses in _cases():
        exact, bound = proj_exact_and_bound(K, poses)
        got = proj_f64(K, poses)
        assert got.dtype == np.float32 and got.shape == exact.shape
        assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
        host = projection_matrices(K, poses)
        assert (np.abs(host.astype(np.float64) - exact) <= bound).all()
    # the two are not the same bits: the kernel's product is compared with the restatement, the fp32 matmul only through the bound
    s = synth.make_scene(0)
    assert np.abs(proj_f64(s['K'], s['poses']).astype(np.float64) - projection_matrices(s['K'], s['poses'])).max() < 1e-6


def test_scene_cache_option_reaches_the_driver():
    from pronerf_amd import cli
    from pronerf_amd.config import config_parser
    assert config_parser('trt').parse_args([]).scene_cache is None
    assert config_parser('trt').parse_args(['--scene_cache', 'u8']).scene_cache == 'u8'
    for cmd in ('infer', 'eval'):
        ns = cli.build_parser().parse_args([cmd, '--scene_cache', 'f32'])
        argv = cli.infer_argv(ns)
        assert argv[argv.index('--scene_cache') + 1] == 'f32'
        assert '--scene_cache' not in cli.infer_argv(cli.build_parser().parse_args([cmd]))
