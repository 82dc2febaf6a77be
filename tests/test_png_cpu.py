"""CPU: the PNG encoder's host twin, pnrf_png_encode_host (the same rule functions the device kernels run; no GPU is touched).

* every image of png_ref.cases: PIL decodes the file to exactly the input, all CRCs and the Adler-32 are right, the filter bytes are the rule's
  (adaptive and each forced type), larger row strides give the same file, two calls give the same bytes, size <= pnrf_png_max_bytes;
* the stored fallback engages on uniform random bytes; the 15-bit limit on a histogram whose unconstrained Huffman tree is deeper;
* every refusal of the argument list;
* sizes on the Scene3D views: RGB smaller than the parent writer's file, depth at most a quarter of its raw plane, every file at most
  (1 + m) x the reference scheme (zlib level 6, Z_RLE, a full flush per segment, on the same filtered bytes), m + 0.01 with m as measured on these
  fixtures and recorded in profiles/png_encode.json;
* config / cli forward the flag; tests/png_host_check.cpp under AddressSanitizer + UBSan as a stand-alone host program.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def S(lib):
    return int(lib.pnrf_png_segment_rows())


@pytest.fixture(scope='module')
def all_cases(S):
    return {name: (img, flt) for name, img, flt in png_ref.cases(S)}


def _names():
    return [n for n, _, _ in png_ref.cases(16)]      # the names do not depend on the segment length


def _check_file(data, img, flt):
    p = png_ref.parse(data)                                       # CRCs, inflate, Adler-32
    ch = 1 if img.ndim == 2 else 3
    assert (p['H'], p['W'], p['channels']) == (img.shape[0], img.shape[1], ch)
    assert p['filtered'] == png_ref.refilter(img, flt), 'filter bytes / residuals differ from the rule'
    assert np.array_equal(png_ref.decode(data), img)
    return p


@pytest.mark.parametrize('name', _names())
def test_host_twin_writes_a_correct_file(lib, all_cases, name):
    from pronerf_amd import ops
    img, flt = all_cases[name]
    ch = 1 if img.ndim == 2 else 3
    filters = [flt] if flt is not None else ([-1, 0, 1, 2, 3, 4] if img.size <= 64 * 33 * 3 else [-1])
    for f in filters:
        data = ops.png_encode_host(img, f)
        assert len(data) <= ops.png_max_bytes(img.shape[0], img.shape[1], ch)
        p = _check_file(data, img, f)
        assert ops.png_encode_host(img, f) == data                                       # deterministic
        if img.shape[0] * img.shape[1] <= 64 * 33:                                          # our own un-filter agrees with PIL's
            assert np.array_equal(png_ref.unfilter(p['filtered'], p['H'], p['W'], ch).reshape(img.shape), img)
    # a row stride larger than the row: the same file
    wide = np.full((img.shape[0], img.shape[1] + 5) + img.shape[2:], 0xa5, np.uint8)
    view = wide[:, :img.shape[1]]
    view[...] = img
    assert not view.flags['C_CONTIGUOUS'] or img.shape[0] == 1
    assert ops.png_encode_host(view, filters[0]) == ops.png_encode_host(img, filters[0])


def test_stored_fallback_and_bound(lib, all_cases, S):
    from pronerf_amd import ops
    img, flt = all_cases['uniform']
    data = ops.png_encode_host(img, flt)
    raw = img.shape[0] * (img.shape[1] + 1)
    nseg = -(-img.shape[0] // S)
    z = png_ref.parse(data)['zdata']
    assert len(z) <= raw + 5 * nseg + 5 * nseg + 6, (len(z), raw)               # stored: 5 bytes a block, 5 a marker; a Huffman block of noise is larger
    assert len(z) > raw
    for name, (im, _) in all_cases.items():
        ch = 1 if im.ndim == 2 else 3
        r = im.shape[0] * (im.shape[1] * ch + 1)
        bound = ops.png_max_bytes(im.shape[0], im.shape[1], ch)
        assert 0 < bound <= r + r // 8 + 1024 * -(-im.shape[0] // S) + 1024, name


@pytest.mark.parametrize('name', ['depth17', 'depth18', 'depth19', 'depth20', 'bushy17'])
def test_length_limit_engages(lib, all_cases, S, name):
    """filter 0 makes the pixels the symbols; the segment's histogram (with the filter bytes and the end-of-block symbol) has an unconstrained Huffman
    tree of the stated depth, beyond the 15-bit limit — chains that need 1, 3, 7 and 15 repair steps and a bushy tree with four leaves at depth 17
    under two roots — and the block is a dynamic one that zlib inflates to the pixels, with a complete literal / length code of at most 15 bits."""
    from pronerf_amd import ops
    img, flt = all_cases[name]
    counts, depth = png_ref.deep_cases(S)[name]
    assert img.shape[0] == S and flt == 0
    filtered = np.frombuffer(png_ref.refilter(img, 0), np.uint8)
    assert max(len(r) for r in bytes(filtered == np.roll(filtered, 1)).split(b'\x00')) < 2      # no byte repeats twice in a row: no run of 4, no match
    hist = sorted([int(c) for c in np.bincount(filtered, minlength=256) if c] + [1])              # + the end-of-block symbol
    assert hist == sorted(png_ref.deep_segment(counts, S)[1])
    d = png_ref.huffman_depths(hist)
    assert max(d) == depth > 15
    if name == 'bushy17':
        assert sum(x == 17 for x in d) == 4 and sum(x > 15 for x in d) == 4
    data = ops.png_encode_host(img, 0)
    p = _check_file(data, img, 0)
    h = png_ref.first_block_header(p['zdata'])
    assert h['btype'] == 2, 'the segment must go out as a dynamic block'
    used = [l for l in h['ll'] if l]
    assert len(used) == len(hist) and max(used) == 15 and sum(2.0 ** -l for l in used) == 1.0
    assert sum(2.0 ** -l for l in h['cl'] if l) == 1.0 and h['dist'] == [1, 1]


def test_whole_image_histogram_of_the_issue(lib, all_cases):
    img, flt = all_cases['forced_depth']
    from pronerf_amd import ops
    _check_file(ops.png_encode_host(img, 0), img, 0)


def test_code_length_code_limit_engages(lib, all_cases):
    """The histogram of the code-length symbols that write the literal lengths has an unconstrained tree more than 8 deep (the limit is 7); the code
    written is complete, at most 7 bits, and zlib inflates the file."""
    from pronerf_amd import ops
    img, flt = all_cases['cl_deep']
    p = _check_file(ops.png_encode_host(img, flt), img, flt)
    h = png_ref.first_block_header(p['zdata'])
    assert h['btype'] == 2
    freq = [f for f in h['cl_freq'] if f]
    print('code-length symbol counts', sorted(freq), 'unconstrained depth', max(png_ref.huffman_depths(freq)))
    assert max(png_ref.huffman_depths(freq)) > 8
    used = [l for l in h['cl'] if l]
    assert len(used) == len(freq) and max(used) == 7 and sum(2.0 ** -l for l in used) == 1.0


def test_geometric_noise_frame(lib, all_cases):
    """Every dynamic block of a frame-sized image of geometric noise: zlib walks them all when it inflates (the generic case test does that; here
    also that the blocks are dynamic ones, not the stored fallback)."""
    from pronerf_amd import ops
    img, _ = all_cases['geometric_frame']
    data = ops.png_encode_host(img)
    p = png_ref.parse(data)
    assert png_ref.first_block_header(p['zdata'])['btype'] == 2 and len(p['zdata']) < 0.5 * img.size


def test_refusals(lib):
    img = np.zeros((4, 5, 3), np.uint8)
    cap = int(lib.pnrf_png_max_bytes(4, 5, 3))
    out = np.zeros(cap, np.uint8)
    size = C.c_int64(-1)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    call = lambda i=ip, stride=15, H=4, W=5, ch=3, f=-1, o=op, c=cap, s=C.byref(size): lib.pnrf_png_encode_host(i, stride, H, W, ch, f, o, c, s)
    assert call() == 0 and size.value > 0
    assert call(H=0) == E_ARG and call(W=0) == E_ARG and call(H=-3) == E_ARG
    assert call(H=1 << 15, W=(1 << 13) + 1, c=1 << 40) == E_ARG                      # more than 2^28 pixels
    assert call(ch=2) == E_ARG and call(ch=4) == E_ARG and call(ch=0) == E_ARG
    assert call(f=-2) == E_ARG and call(f=5) == E_ARG
    assert call(stride=14) == E_ARG
    assert call(c=cap - 1) == E_ARG and b'pnrf_png_max_bytes' in lib.pnrf_last_error()
    assert call(i=None) == E_ARG and call(o=None) == E_ARG and call(s=None) == E_ARG
    assert lib.pnrf_png_max_bytes(0, 5, 3) == 0 and lib.pnrf_png_max_bytes(4, 5, 2) == 0 and lib.pnrf_png_workspace_bytes(4, 0, 1) == 0
    assert lib.pnrf_png_workspace_bytes(1 << 15, (1 << 13) + 1, 1) == 0
    # the device entry refuses the same list before it touches a device (no GPU here: a launch would fail otherwise)
    ws = int(lib.pnrf_png_workspace_bytes(4, 5, 3))
    assert ws > 0
    fake = C.c_void_p(1 << 20)
    dev = lambda i=fake, stride=15, H=4, W=5, ch=3, f=-1, o=fake, c=cap, s=fake, w=fake, wb=ws: lib.pnrf_png_encode_fwd(i, stride, H, W, ch, f, o, c, s, w, wb, None)
    for kw in (dict(H=0), dict(W=0), dict(H=1 << 15, W=(1 << 13) + 1, c=1 << 40, wb=1 << 40), dict(ch=2), dict(f=5), dict(f=-2), dict(stride=14), dict(c=cap - 1), dict(wb=ws - 1),
               dict(w=C.c_void_p((1 << 20) + 8)), dict(i=None), dict(o=None), dict(s=None), dict(w=None)):
        assert dev(**kw) == E_ARG, kw
    from pronerf_amd import ops
    from pronerf_amd._lib import PnrfError
    import torch
    with pytest.raises(PnrfError):
        ops.PngEncoder(4, 5, 3, 'cpu')
    with pytest.raises(PnrfError):
        ops.png_encode_host(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(PnrfError):
        ops.png_encode_host(img, 'best')


M_FILE = os.path.join(ROOT, 'profiles', 'png_encode.json')


def test_sizes_on_the_scene_views(lib, S):
    from pronerf_amd import ops
    recorded = json.load(open(M_FILE))['size_margin']
    m_allowed = recorded['m'] + 0.01
    rng = np.random.RandomState(5)
    worst = 0.0
    for H, W in ((189, 252), (378, 504)):
        rgb, depth = png_ref.scene_views(H, W)
        noisy = np.clip(rgb.astype(np.float32) / 255 + rng.normal(0, 0.012, rgb.shape), 0, 1)
        planes = [('rgb', rgb), ('rgb+noise', (255 * noisy).astype(np.uint8)), ('depth', depth)]
        for name, img in planes:
            data = ops.png_encode_host(img)
            p = _check_file(data, img, -1) if H == 189 else png_ref.parse(data)
            ch = p['channels']
            ref = png_ref.reference_size(p['filtered'], W * ch + 1, S)
            ratio = len(p['zdata']) / ref
            worst = max(worst, ratio - 1)
            print(f'{H}x{W} {name}: file {len(data)} B, zlib stream {len(p["zdata"])} B, reference {ref} B (x{ratio:.4f}), parent writer {len(png_ref.parent_file(img))} B, '
                  f'raw {H * W * ch} B')
            assert len(p['zdata']) <= ref * (1 + m_allowed), (name, ratio)
            if ch == 3:
                assert len(data) < len(png_ref.parent_file(img)), name
            else:
                assert len(data) <= H * W // 4, name
    print(f'measured m = {worst:.4f} (recorded {recorded["m"]})')


def test_config_and_cli_forward_the_flag():
    from pronerf_amd import cli, config
    p = config.config_parser('trt')
    assert p.parse_args(['--device_png']).device_png is True and p.parse_args([]).device_png is False
    for sub in ('infer', 'eval'):
        for flag in ('--device-png', '--device_png'):
            ns = cli.build_parser().parse_args([sub, flag])
            assert ns.device_png is True and '--device_png' in cli.infer_argv(ns)
        ns = cli.build_parser().parse_args([sub])
        assert ns.device_png is False and '--device_png' not in cli.infer_argv(ns)


def test_encoder_runs_clean_under_the_sanitizers(tmp_path):
    """tests/png_host_check.cpp + the host halves of pnrf_png.hip and pnrf_pack.hip (the error string lives there) as one program under ASan + UBSan;
    nothing is loaded into python."""
    from pronerf_amd import build
    exe = str(tmp_path / 'png_host_check')
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all']
    cmd = [build._hipcc(), '-O1', '-g', '-std=c++17', f'--offload-arch={build.ARCH}', f'-DPNRF_LAYOUT_TAG=0x{build._layout_tag():08x}u', '-I', build.INCLUDE] + san + \
          [os.path.join(build.CSRC, 'pnrf_png.hip'), os.path.join(build.CSRC, 'pnrf_pack.hip'), '-x', 'hip', os.path.join(ROOT, 'tests', 'png_host_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'ERROR' not in r.stdout and 'runtime error' not in r.stdout, r.stdout[-4000:]
    assert 'images encoded' in r.stdout, r.stdout[-2000:]
