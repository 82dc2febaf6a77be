"""CPU: the packer's host half, pnrf_mlp_pack_image — no GPU is touched.

* byte identity: for every net of tests/pack_cases.py the image (layout tag zeroed: it changes with every edit of the packer) has the sha256 that
  ``pnrf_mlp_serialize(pnrf_mlp_pack(...))`` of the library built from commit 8e43696 — the last whose packer built its streams and uploaded them in one
  function — wrote on an MI355X;
* refusals: the codes and the texts of that commit's pnrf_mlp_pack (pnrf_last_error keeps 511 characters of a message);
* tests/pack_host_check.cpp, the packer under AddressSanitizer + UBSan as a stand-alone host program.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import pack_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# recorded with the library of the parent commit 8e43696: pack -> serialize on the GPU, bytes 16:20 zeroed, sha256
PARENT_DIGESTS = {
    'fern-sampler': '64a73ca97a960531c0efb3e0f0a473bf3d2bcb5d2e38d241ab0dfdfa08407991',
    'fern-refine': '1959fd5655fba9dda5abbf45b2b250317e20d6a52e44864616df3d204fdf637f',
    'fern-nerf': '48ba5af5e389c409d414c99b178d7bd65e9c755aa669a8d9787bad4e439a308e',
    'smallest-sampler': '0f92c3c0e4b43839948e060257a5b1054ff1a83a6ef9db760d29ba8b76db6d8e',
    'smallest-refine': 'ceafea13ca61dcbce508897acb5ab22a09811ed22e6e67e53e0bec28ee590955',
    'smallest-nerf': '953613f1d0b8b03bb30488ae2979e67eceb739e1076890898c56ced642092a56',
    'offfern-sampler': '00baed821f6ee8ffba78fae034e7658f749681413809c30ab678ceb7a4916f4d',
    'offfern-refine': 'f58697a4742486420922d3f9b97e8694f4e0d73d72152f60c7e3704799044132',
    'offfern-nerf': '81c5c7ae9ea98ec76bdb38f92e889b2097cfda5c20b1d89de709a2c73d02e97b',
    'skip4-sampler': 'dcd29370e84cf192296de76c9e27bb641b6534935a36e6f5b883a572f43a778f',
    'skip4-refine': 'abbe9dd1fb31269c5d2ab908b05e25b41ece9cd8a59e1130b37e537abcd2796d',
    'skip02-sampler': '61fec4e3050bd6ac88e9a217865b370ba57cf2ef754ef95c6f6f62f9aabd7bd8',
    'skip02-refine': '8d2b779e9bfa006668dd41fbb121fb33085fa028e13fec5b29e869f7e2418050',
    'deepest-sampler': 'f6c2b21562b13434761ebbf460da4fc263036dab910d0065fc44376db3e9af7c',
    'deepest-refine': '760ff3a4b367bfdf1f6116db8c14462003de57dee4b5f6aadc64c310421e3560',
    'nb2-refine': 'd74c21203310e492b3cac0024cc4c5616f83464e18f6014a9004440690139afb',
    'nb3-refine': '8a18473774886819689efa261d56aa8f0837e202e75921462e77618a9e1cb086',
    'nb4-refine': '1b14b68f16ff4e5fa2616135d4020a38f8a4ed7fb00b7464454a89f77f3738e6',
    'nb5-refine': '226d42324e2ec03d0c6ea2d95c5b97a01fd3ff92ff296073e60acc44f1ba8f17',
    'nb6-refine': '26688c0f486732ff3a4afbbc19d2cbe3adb0a77040e765d6f916da8d0e5e06a4',
    'nb7-refine': '563f73bf40512661df98fb96368bc133e74f37c3db9afef02cfaeb4720b2adf6',
    'nb8-refine': 'f5cc4c96931357deb54d2df48ea29493419c7baea010cfed7d028b598a872eaa',
    'nerfcls': '22e71fce564d1547f142ab3c6feda1933738630f6f4e838f7d1fe28ea83d18ff',
}


def test_every_case_is_pinned():
    assert sorted(PARENT_DIGESTS) == sorted(pc.NAMES)


@pytest.mark.parametrize('name', pc.NAMES)
def test_image_is_byte_identical_to_the_parent_commits(lib, name):
    from pronerf_amd import ops
    img = bytearray(ops.PackedMLP.pack_image(*pc.case(name)))
    assert img[:8] == b'PNRFENG\0'
    img[16:20] = b'\0\0\0\0'
    assert hashlib.sha256(bytes(img)).hexdigest() == PARENT_DIGESTS[name]


# ---- refusals: (code, message) of the parent's pnrf_mlp_pack, from its source
E_ARG, E_SHAPE = -1, -2
SUPPORTED = ('supported: hidden width 256, N_samples 8 (sampler 6*P -> D x 256 -> 27, any P >= 1; refine 48 + 24*nb -> D x 256 -> 35, nb = 1..8; '
             'DoNeRFTRT 63 -> (netdepth - 1) x 256 -> [256 + 27] -> 4 with 3 <= netdepth <= 8; sampler / refine depth 2 <= D <= 32, skip connections (mmnetskips) behind '
             'backbone layers 0 .. D - 2: such a layer has 256 + input width columns; the NeRF class: D = 8, skips = [4])')


def _stack(dims):
    """zero weights of the Linear layers (in, out), ..."""
    return [np.zeros((o, i), np.float32) for i, o in dims], [np.zeros(o, np.float32) for i, o in dims]


def _mm(in0, out, depth=6):
    return [(in0, 256)] + [(256, 256)] * (depth - 1) + [(256, out)]


def _refusals():
    from pronerf_amd import synthetic
    cls = synthetic.nerfcls_layer_dims()
    cls = cls['pts_linears'] + [cls['feature_linear'], cls['alpha_linear'], cls['views_linears'][0], cls['rgb_linear']]
    narrow = _mm(288, 27); narrow[2] = (256, 128)
    skip_deep = _mm(48 + 24 * 7, 35, depth=32); skip_deep[3] = (256 + 48 + 24 * 7, 256)
    return {
        'null layer': (0, _mm(288, 27), 3, E_ARG, 'pnrf_mlp_pack: null weight/bias at layer 3'),
        'width is not 256': (0, narrow, None, E_SHAPE, 'pnrf_mlp_pack: net 0 layer 2 is 128x256 where 256x256 is needed (or 544 input columns for a skip layer, cat([x, h]), '
                             'behind backbone layers 0 .. D - 2); ' + SUPPORTED),
        'sampler input is not a multiple of 6': (0, _mm(100, 27), None, E_SHAPE, 'pnrf_mlp_pack: sampler input width 100 is not 6 * N_point_ray_enc; ' + SUPPORTED),
        'num_neighbor 9': (1, _mm(48 + 24 * 9, 35), None, E_SHAPE, 'pnrf_mlp_pack: refine input width 264 is not 48 + 24 * num_neighbor with 1 <= num_neighbor <= 8; ' + SUPPORTED),
        'DoNeRFTRT with 9 layers': (2, synthetic.nerf_layer_dims(9), None, E_SHAPE, "pnrf_mlp_pack: DoNeRFTRT with netdepth 9: from 9 layers on skip='auto' feeds the view "
                                    'encoding into a hidden layer; ' + SUPPORTED),
        'NeRF class with 11 layers': (3, cls[:11], None, E_SHAPE, 'pnrf_mlp_pack: the NeRF class expects 12 Linear layers (pts0..7, feature, alpha, views, rgb), got 11'),
        'skip refine net beyond the LDS': (1, skip_deep, None, E_SHAPE, 'pnrf_mlp_pack: refine net with skip connections (mmnetskips), 32 layers and 7 neighbour views: its bias '
                                           'table and the parked net input do not fit the LDS beside the weight ring (at most 31 layers with 7 or 8 views); ' + SUPPORTED),
    }


@pytest.mark.parametrize('what', ['null layer', 'width is not 256', 'sampler input is not a multiple of 6', 'num_neighbor 9', 'DoNeRFTRT with 9 layers',
                                  'NeRF class with 11 layers', 'skip refine net beyond the LDS'])
def test_refusals_are_the_parent_commits(lib, what):
    net, dims, null_at, code, text = _refusals()[what]
    Ws, bs = _stack(dims)
    n = len(Ws)
    Wp = (C.c_void_p * n)(*[w.ctypes.data for w in Ws])
    bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
    if null_at is not None:
        Wp[null_at] = None
    ind = (C.c_int * n)(*[w.shape[1] for w in Ws]); outd = (C.c_int * n)(*[w.shape[0] for w in Ws])
    size = C.c_int64(-7)
    buf = (C.c_char * 256)()
    for args in ((None, 0), (buf, 256)):            # the size query refuses like the call that writes, and nothing is written
        assert lib.pnrf_mlp_pack_image(net, Wp, bp, ind, outd, n, args[0], args[1], C.byref(size)) == code
        assert lib.pnrf_last_error().decode() == text[:511]
    assert bytes(buf) == b'\0' * 256
    # ... and pnrf_mlp_pack refuses with the same words before it reaches a device
    h = C.c_void_p()
    assert lib.pnrf_mlp_pack(net, Wp, bp, ind, outd, n, C.byref(h)) == code and lib.pnrf_last_error().decode() == text[:511] and not h.value


def test_size_query_and_short_buffer(lib):
    net, Ws, bs = pc.case('smallest-nerf')
    from pronerf_amd import ops
    img = ops.PackedMLP.pack_image(net, Ws, bs)
    _keep, args = ops.PackedMLP._pack_args(Ws, bs)
    size = C.c_int64()
    assert lib.pnrf_mlp_pack_image(net, *args, None, 0, C.byref(size)) == 0 and size.value == len(img)
    buf = (C.c_char * len(img))()
    assert lib.pnrf_mlp_pack_image(net, *args, buf, len(img) - 1, C.byref(size)) == E_ARG and b'pnrf_mlp_pack_image: buffer of' in lib.pnrf_last_error()
    assert lib.pnrf_mlp_pack_image(net, *args, buf, len(img), None) == E_ARG and lib.pnrf_last_error() == b'pnrf_mlp_pack: null argument'


def test_packer_runs_clean_under_the_sanitizers(tmp_path):
    """tests/pack_host_check.cpp + pnrf_pack.hip as one host program under ASan + UBSan (nothing is loaded into python): every shape of pack_cases through
    pnrf_mlp_pack_image, the size query against the bytes written, the checksum; damaged images into pnrf_mlp_deserialize, refused on the host."""
    from pronerf_amd import build
    exe = str(tmp_path / 'pack_host_check')
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all']
    cmd = [build._hipcc(), '-O1', '-g', '-std=c++17', f'--offload-arch={build.ARCH}', f'-DPNRF_LAYOUT_TAG=0x{build._layout_tag():08x}u', '-I', build.INCLUDE] + san + \
          [os.path.join(build.CSRC, 'pnrf_pack.hip'), '-x', 'hip', os.path.join(ROOT, 'tests', 'pack_host_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'ERROR' not in r.stdout and 'runtime error' not in r.stdout, r.stdout[-4000:]
    assert f'{len(pc.NAMES)} images packed' in r.stdout and 'all damaged images refused' in r.stdout, r.stdout[-2000:]
