"""CPU: the JPEG encoder's host twin, pnrf_jpeg_encode_host (the same rule functions the device kernels run; no GPU is touched), and the Motion-JPEG
writer.

* every image of jpeg_ref.cases: marker order, no marker inside the entropy data but the expected RSTm sequence, every FF followed by 00 or that
  marker, PIL opens the file with the right size and mode, the coefficients jpeg_ref's decoder reads equal the numpy statement exactly, the size is
  at most pnrf_jpeg_max_bytes, a larger row pitch gives the same file, two calls give the same bytes;
* the decoder's event counts show that the list really exercises stuffing, ZRL runs of 1 / 2 / 3, a block without EOB, DC category 11, AC category
  10 and more than 8 intervals;
* the quantisation tables are PIL's for quality 1, 10, 50, 75, 90, 95, 100;
* on the Scene3D views, PSNR and size against PIL's own file within the margins recorded in profiles/jpeg_encode.json;
* every refusal of the argument list, with ``out`` untouched;
* tests/jpeg_host_check.cpp under AddressSanitizer + UBSan as a stand-alone host program;
* the AVI file: chunks inside their parents, even padding, frame counts, index, frames as given, the 2 GiB refusal; config / cli forward the options.
"""
import ctypes as C
import io
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
MARKERS = ['SOI', 'APP0', 'DQT', 'SOF0', 'DHT', 'DRI', 'SOS', 'EOI']


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def all_cases():
    cases = {name: (img, q) for name, img, q in jpeg_ref.cases()}
    assert list(cases) == jpeg_ref.case_names()
    return cases


@pytest.fixture(scope='module')
def decoded(lib, all_cases):
    """name -> (file, jpeg_ref.decode of it): every case is encoded and decoded once for the tests that look at it."""
    from pronerf_amd import ops
    out = {}
    for name, (img, q) in all_cases.items():
        data = ops.jpeg_encode_host(img, q)
        out[name] = (data, jpeg_ref.decode(data))
    return out


def _pil(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _pil_file(img, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=quality, subsampling=0, optimize=False, restart_marker_rows=1)
    return b.getvalue()


@pytest.mark.parametrize('name', jpeg_ref.case_names())
def test_host_twin_writes_a_correct_file(lib, all_cases, decoded, name):
    from pronerf_amd import ops
    img, q = all_cases[name]
    data, d = decoded[name]
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    assert d['markers'] == MARKERS                                                              # decode() asserts the rest of the structure on its way
    assert (d['H'], d['W'], d['channels']) == (H, W, ch) and d['dri'] == -(-W // 8)
    assert sorted(d['dht']) == ([(0, 0), (1, 0)] if ch == 1 else [(0, 0), (0, 1), (1, 0), (1, 1)])
    assert d['header_bytes'] == (330 if ch == 1 else 613)
    for t in range(1 if ch == 1 else 2):
        assert d['qtables'][t] == list(jpeg_ref.qtable(t, q)[jpeg_ref.ZZ])
    want = jpeg_ref.coefficients(img, q)
    assert d['coefficients'].shape == want.shape and np.array_equal(d['coefficients'], want)
    assert len(data) <= ops.jpeg_max_bytes(H, W, ch)
    im = _pil(data)
    assert im.size == (W, H) and im.mode == ('L' if ch == 1 else 'RGB')
    assert ops.jpeg_encode_host(img, q) == data                                                 # deterministic
    wide = np.full((H, W + 5) + img.shape[2:], 0xa5, np.uint8)                                   # a row stride larger than the row: the same file
    view = wide[:, :W]
    view[...] = img
    assert ops.jpeg_encode_host(view, q) == data
    if name.startswith('strided'):
        assert not img.flags['C_CONTIGUOUS'] and ops.jpeg_encode_host(np.ascontiguousarray(img), q) == data


def test_the_cases_reach_every_mechanism(decoded):
    """On the decoder's event counts: a changed case list cannot quietly lose what it is there for."""
    ev = {name: d['events'] for name, (_, d) in decoded.items()}
    for k in ('gray', 'rgb'):
        assert ev[f'noise_{k}']['stuffed'] > 0
        z = ev[f'zrl_{k}']
        assert z['zrl_runs'][1] >= 1 and z['zrl_runs'][2] >= 1 and z['zrl_runs'][3] >= 2 and z['no_eob'] == 1
        assert ev[f'checker_{k}']['max_dc_category'] == 11 and ev[f'checker_{k}']['max_ac_category'] == 10
        assert ev[f'72x16_{k}']['intervals'] == 9 and decoded[f'72x16_{k}'][1]['rst'] == [0, 1, 2, 3, 4, 5, 6, 7]
        assert ev[f'8x2056_{k}']['intervals'] == 1 and decoded[f'8x2056_{k}'][1]['coefficients'].shape[1] == 257
        c = decoded[f'constant_{k}'][1]['coefficients']
        assert not c[..., 1:].any() and not np.diff(c[..., 0], axis=1).any()                 # EOB only, DC difference 0 after the first block
        assert ev[f'noise_{k}']['no_eob'] > 0
    zz = decoded['zrl_gray'][1]['coefficients'][0, :, 0]
    for blk, levels in zip(zz, jpeg_ref.ZRL_BLOCKS):
        assert {int(k): int(blk[k]) for k in np.nonzero(blk)[0]} == levels


@pytest.mark.parametrize('quality', [1, 10, 50, 75, 90, 95, 100])
def test_quantisation_tables_are_pils(lib, all_cases, quality):
    from pronerf_amd import ops
    for name in ('7x9_gray', '7x9_rgb'):
        img = all_cases[name][0]
        ours, pil = _pil(ops.jpeg_encode_host(img, quality)), _pil(_pil_file(img, quality))
        assert {k: list(v) for k, v in ours.quantization.items()} == {k: list(v) for k, v in pil.quantization.items()}
        assert ours.size == pil.size and ours.mode == pil.mode


M_FILE = os.path.join(ROOT, 'profiles', 'jpeg_encode.json')


def test_against_pil_on_the_scene_views(lib):
    """PSNR of PIL's decode of our file >= that of PIL's own file - (d + 0.05 dB), size <= (1 + m + 0.01) x PIL's; d and m as measured on these
    fixtures (tools/jpeg_bench.py --cpu-only) and recorded.  Measured: d = 0, m = 0 — the decoded pixels are those of PIL's file at every quality,
    the files are 16 (RGB) and 4 (gray) bytes shorter (one DQT and one DHT segment instead of one per table)."""
    import png_ref
    from pronerf_amd import ops
    rec = json.load(open(M_FILE))['margins']
    d_allowed, m_allowed = rec['d'] + 0.05, rec['m'] + 0.01
    from PIL import Image
    for H, W in ((189, 252), (378, 504)):
        for plane, img in zip(('rgb', 'depth'), png_ref.scene_views(H, W)):
            for q in (50, 75, 90, 95):
                ours, pil = ops.jpeg_encode_host(img, q), _pil_file(img, q)
                psnr = lambda data: 10 * np.log10(255.0 ** 2 / np.mean((np.asarray(Image.open(io.BytesIO(data))).astype(np.float64) - img) ** 2))
                p_ours, p_pil = psnr(ours), psnr(pil)
                print(f'{H}x{W} {plane} q{q}: {len(ours)} B against {len(pil)} B (x{len(ours) / len(pil):.4f}), PSNR {p_ours:.4f} dB against {p_pil:.4f} dB')
                assert p_ours >= p_pil - d_allowed, (H, W, plane, q)
                assert len(ours) <= (1 + m_allowed) * len(pil), (H, W, plane, q)


def test_refusals(lib):
    img = np.zeros((4, 5, 3), np.uint8)
    cap = int(lib.pnrf_jpeg_max_bytes(4, 5, 3))
    out = np.full(cap, 0x5a, np.uint8)
    size = C.c_int64(-1)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    call = lambda i=ip, stride=15, H=4, W=5, ch=3, q=90, o=op, c=cap, s=C.byref(size): lib.pnrf_jpeg_encode_host(i, stride, H, W, ch, q, o, c, s)
    refused = (dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, c=1 << 40), dict(W=65536, c=1 << 40), dict(ch=2), dict(ch=4), dict(ch=0), dict(q=0), dict(q=101), dict(q=-1),
               dict(stride=14), dict(c=cap - 1), dict(i=None), dict(o=None), dict(s=None))
    for kw in refused:
        assert call(**kw) == E_ARG, kw
        assert size.value == -1 and (out == 0x5a).all(), kw                                  # nothing written
    assert call(c=cap - 1) == E_ARG and b'pnrf_jpeg_max_bytes' in lib.pnrf_last_error()
    assert call() == 0 and 0 < size.value <= cap
    for f in (lib.pnrf_jpeg_max_bytes, lib.pnrf_jpeg_workspace_bytes):
        assert f(0, 5, 3) == 0 and f(4, 0, 1) == 0 and f(4, 5, 2) == 0 and f(65536, 5, 1) == 0 and f(4, 65536, 3) == 0
        assert f(65535, 65535, 3) > 0 and f(1, 1, 1) > 0
    # the closed form: header + intervals x (2 ceil(1660 blocks / 8) + 2) + 2
    for H, W, ch in ((1, 1, 1), (9, 17, 3), (756, 1008, 3), (756, 1008, 1)):
        blocks = -(-W // 8) * ch
        assert lib.pnrf_jpeg_max_bytes(H, W, ch) == (330 if ch == 1 else 613) + -(-H // 8) * (2 * -(-1660 * blocks // 8) + 2) + 2
    # the device entry refuses the same list before it touches a device (no GPU here: a launch would fail otherwise)
    ws = int(lib.pnrf_jpeg_workspace_bytes(4, 5, 3))
    assert ws > 0
    fake = C.c_void_p(1 << 20)
    dev = lambda i=fake, stride=15, H=4, W=5, ch=3, q=90, o=fake, c=cap, s=fake, w=fake, wb=ws: lib.pnrf_jpeg_encode_fwd(i, stride, H, W, ch, q, o, c, s, w, wb, None)
    for kw in (dict(H=0), dict(W=0), dict(H=65536, c=1 << 40, wb=1 << 50), dict(ch=2), dict(q=0), dict(q=101), dict(stride=14), dict(c=cap - 1), dict(wb=ws - 1),
               dict(w=C.c_void_p((1 << 20) + 8)), dict(i=None), dict(o=None), dict(s=None), dict(w=None)):
        assert dev(**kw) == E_ARG, kw
    from pronerf_amd import ops
    from pronerf_amd._lib import PnrfError
    import torch
    with pytest.raises(PnrfError):
        ops.JpegEncoder(4, 5, 3, 'cpu')
    with pytest.raises(PnrfError):
        ops.jpeg_encode_host(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(PnrfError):
        ops.jpeg_encode_host(img, 0)
    with pytest.raises(PnrfError):
        ops.jpeg_encode_host(img, 'best')


def test_encoder_runs_clean_under_the_sanitizers(tmp_path):
    """tests/jpeg_host_check.cpp + the host halves of pnrf_jpeg.hip and pnrf_pack.hip (the error string lives there) as one program under ASan + UBSan;
    nothing is loaded into python."""
    from pronerf_amd import build
    exe = str(tmp_path / 'jpeg_host_check')
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all']
    cmd = [build._hipcc(), '-O1', '-g', '-std=c++17', f'--offload-arch={build.ARCH}', f'-DPNRF_LAYOUT_TAG=0x{build._layout_tag():08x}u', '-I', build.INCLUDE] + san + \
          [os.path.join(build.CSRC, 'pnrf_jpeg.hip'), os.path.join(build.CSRC, 'pnrf_pack.hip'), '-x', 'hip', os.path.join(ROOT, 'tests', 'jpeg_host_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'ERROR' not in r.stdout and 'runtime error' not in r.stdout, r.stdout[-4000:]
    assert 'images encoded' in r.stdout, r.stdout[-2000:]


def _avi_frames(data):
    """(chunks by path, the 00dc frames in order, idx1 entries) of an AVI file."""
    chunks = jpeg_ref.riff_walk(data)
    frames = [(tag_at, data[body:body + size]) for path, tag_at, body, size in chunks if path == 'RIFF:AVI /LIST:movi/00dc']
    by = {path: (tag_at, body, size) for path, tag_at, body, size in chunks if not path.endswith('00dc')}
    _, body, size = by['RIFF:AVI /idx1']
    index = [struct.unpack('<4sIII', data[body + 16 * k:body + 16 * k + 16]) for k in range(size // 16)]
    return by, frames, index


def _check_avi(data, given, W, H, gray, fps):
    by, frames, index = _avi_frames(data)
    assert list(by) == ['RIFF:AVI ', 'RIFF:AVI /LIST:hdrl', 'RIFF:AVI /LIST:hdrl/avih', 'RIFF:AVI /LIST:hdrl/LIST:strl', 'RIFF:AVI /LIST:hdrl/LIST:strl/strh',
                        'RIFF:AVI /LIST:hdrl/LIST:strl/strf', 'RIFF:AVI /LIST:movi', 'RIFF:AVI /idx1']
    assert by['RIFF:AVI '][:2] == (0, 12) and by['RIFF:AVI '][2] + 12 == len(data) and struct.unpack('<I', data[4:8])[0] + 8 == len(data)
    assert [f for _, f in frames] == list(given)
    avih = struct.unpack('<14I', data[by['RIFF:AVI /LIST:hdrl/avih'][1]:][:56])
    assert by['RIFF:AVI /LIST:hdrl/avih'][2] == 56 and avih[4] == len(given) and avih[6] == 1 and avih[8:10] == (W, H) and avih[3] & 0x10
    assert avih[0] == round(1e6 / fps) and avih[7] == max(map(len, given), default=0)
    strh = struct.unpack('<4s4sIHHIIIIIIII4H', data[by['RIFF:AVI /LIST:hdrl/LIST:strl/strh'][1]:][:56])
    assert strh[:2] == (b'vids', b'MJPG') and strh[9] == len(given) and strh[7] / strh[6] == fps
    strf = struct.unpack('<IiiHH4sIiiII', data[by['RIFF:AVI /LIST:hdrl/LIST:strl/strf'][1]:][:40])
    assert by['RIFF:AVI /LIST:hdrl/LIST:strl/strf'][2] == 40 and strf[:6] == (40, W, H, 1, 8 if gray else 24, b'MJPG')
    movi_tag = by['RIFF:AVI /LIST:movi'][1] - 4                                               # where 'movi' stands
    assert data[movi_tag:movi_tag + 4] == b'movi' and len(index) == len(given)
    for (tag_at, frame), (ckid, flags, off, size) in zip(frames, index):
        assert ckid == b'00dc' and flags & 0x10 and movi_tag + off == tag_at and size == len(frame)
        assert tag_at % 2 == 0                                                                  # every chunk starts on an even offset: odd frames are padded


def test_avi_files(lib, all_cases, decoded, tmp_path):
    from pronerf_amd import ops
    from pronerf_amd._lib import PnrfError
    from pronerf_amd.video import MjpegAviWriter
    rgb = [decoded[n][0] for n in ('9x17_rgb',)]
    img = all_cases['9x17_rgb'][0]
    assert img.shape == (9, 17, 3)
    frames = [ops.jpeg_encode_host(np.roll(img, k, 1), q) for k, q in enumerate((90, 91, 92, 93, 94, 95))] + rgb
    assert any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames), [len(f) for f in frames]
    path = str(tmp_path / 'a.avi')
    with MjpegAviWriter(path, 17, 9, 30) as v:
        for f in frames:
            v.add(f)
    _check_avi(open(path, 'rb').read(), frames, 17, 9, False, 30)
    gray = [ops.jpeg_encode_host(np.roll(img[..., 0], k, 0), 80 + k) for k in range(3)]
    v = MjpegAviWriter(path, 17, 9, 12.5, gray=True)
    for f in gray:
        v.add(f)
    v.close(); v.close()
    _check_avi(open(path, 'rb').read(), gray, 17, 9, True, 12.5)
    with pytest.raises(PnrfError):
        v.add(gray[0])                                                                          # closed
    with MjpegAviWriter(path, 17, 9, 30):                                                       # no frames: still a file the walker accepts
        pass
    _check_avi(open(path, 'rb').read(), [], 17, 9, False, 30)
    # the size limit, lowered through the keyword: the frame that would take the closed file past it is refused, the file closed there is valid
    head = len(open(path, 'rb').read())                                                         # headers and an empty index
    room = lambda fs: head + sum(8 + len(f) + len(f) % 2 + 16 for f in fs)
    v = MjpegAviWriter(path, 17, 9, 30, limit=room(frames[:3]))
    for f in frames[:3]:
        v.add(f)
    with pytest.raises(PnrfError):
        v.add(frames[3])
    v.close()
    data = open(path, 'rb').read()
    assert len(data) == room(frames[:3])
    _check_avi(data, frames[:3], 17, 9, False, 30)
    from pronerf_amd import video
    assert video.AVI_LIMIT == 2 ** 31 - 2 ** 20
    for bad in (dict(W=0), dict(H=70000), dict(fps=0)):
        with pytest.raises(PnrfError):
            MjpegAviWriter(path, **{**dict(W=17, H=9, fps=30), **bad})
    with pytest.raises(PnrfError):
        with MjpegAviWriter(path, 17, 9, 30) as v:
            v.add(b'not a jpeg')


def test_config_and_cli_forward_the_options():
    from pronerf_amd import cli, config
    p = config.config_parser('trt')
    a = p.parse_args(['--video', '--video_fps', '24', '--video_quality', '75'])
    assert a.video is True and a.video_fps == 24 and a.video_quality == 75
    a = p.parse_args([])
    assert a.video is False and a.video_fps == 30 and a.video_quality == 90
    for sub in ('infer', 'eval'):
        ns = cli.build_parser().parse_args([sub, '--video', '--video_fps', '24', '--video-quality', '75'])
        argv = cli.infer_argv(ns)
        assert ns.video is True and '--video' in argv
        assert float(argv[argv.index('--video_fps') + 1]) == 24 and int(argv[argv.index('--video_quality') + 1]) == 75
        b = p.parse_args(argv[argv.index('--video'):argv.index('--video') + 5])                  # the driver's parser takes what the cli forwards
        assert b.video is True and b.video_fps == 24 and b.video_quality == 75
        ns = cli.build_parser().parse_args([sub])
        assert ns.video is False and not any(x.startswith('--video') for x in cli.infer_argv(ns))
