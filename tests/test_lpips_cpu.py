"""CPU: LPIPS — the restatement of tests/lpips_ref.py against an independent formulation, the properties of the definition, the argument and shape
checks of every new entry point (all made before any device work, so they are reported without a GPU) and the weight loader."""
import ctypes as C

import numpy as np
import pytest
import torch

import lpips_ref as R


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- 1. the restatement against unfold + matmul, and the tap sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize('net,layer,H,W', [('alex', 0, 31, 39), ('alex', 1, 7, 9), ('alex', 2, 5, 7), ('vgg', 0, 5, 6), ('vgg', 2, 6, 9), ('vgg', 12, 3, 4)])
def test_layer_restatement_against_unfold_matmul(net, layer, H, W):
    ci, co, k, stride, pad, pool, _ = R.TABLES[net][layer]
    g = torch.Generator().manual_seed(layer + 100 * H)
    x = torch.randn(2, ci, H, W, generator=g, dtype=torch.float64)
    Wt, b = (t.double() for t in (R.cached_net(net)['W'][layer], R.cached_net(net)['b'][layer]))
    got = R.layer_ref(net, layer, x, Wt, b, pool != 0)
    # independent: the pooling as a maximum over shifted slices, the convolution as columns x matrix
    if pool:
        ph, pw = (H - pool) // 2 + 1, (W - pool) // 2 + 1
        x = torch.stack([x[:, :, dy:dy + 2 * ph - 1:2, dx:dx + 2 * pw - 1:2] for dy in range(pool) for dx in range(pool)]).max(0).values
    oh, ow = (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1
    cols = torch.nn.functional.unfold(x, k, padding=pad, stride=stride)                 # [2, ci k k, oh ow]
    want = (Wt.reshape(co, -1) @ cols + b[None, :, None]).clamp_min(0).reshape(2, co, oh, ow)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


SIZES = {'alex': [(31, 31), (31, 39), (32, 34), (35, 47), (64, 80), (66, 67), (67, 63), (95, 96), (127, 130)],
         'vgg': [(16, 16), (17, 23), (18, 31), (32, 33), (47, 48), (48, 40), (63, 65)]}


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_tap_dims_match_the_restatement(lib, net):
    for H, W in SIZES[net]:
        hw = (C.c_int * 10)()
        assert lib.pnrf_lpips_tap_dims(net.encode(), H, W, hw) == 0, lib.pnrf_last_error()
        got = [(hw[2 * k], hw[2 * k + 1]) for k in range(5)]
        assert got == R.tap_dims(net, H, W)
    H, W = SIZES[net][1]                                                                # ... and the shapes conv2d / max_pool2d themselves give
    feats = R.features(net, R.cached_net(net), np.zeros((H, W, 3), np.float32), dtype=torch.float32)
    assert [tuple(f.shape[1:]) for f in feats] == R.tap_dims(net, H, W) and [f.shape[0] for f in feats] == R.lin_channels(net)


# ---- 2. properties of the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,H,W', [('alex', 31, 39), ('vgg', 17, 23)])
def test_restatement_identity_and_symmetry(net, H, W):
    a, b = R.make_pair('mix', H, W)
    w = R.cached_net(net)
    d_aa, maps = R.lpips_ref(net, w, a, a)
    assert d_aa == 0.0 and all(float(m.abs().max()) == 0.0 for m in maps)
    d_ab, d_ba = R.lpips_ref(net, w, a, b)[0], R.lpips_ref(net, w, b, a)[0]
    assert d_ab == d_ba and d_ab > 0


# ---- 3. argument and shape errors, all before any device work -----------------------------------------------------------------------------------
def _create(lib, net, shapes, lin_dims, n=None):
    n = len(shapes) if n is None else n
    bufs = [np.zeros(int(np.prod(s)), np.float32) for s in shapes] + [np.zeros(s[0], np.float32) for s in shapes] + [np.zeros(max(c, 1), np.float32) for c in lin_dims]
    ptr = lambda arrs: (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    ns = len(shapes)
    h = C.c_void_p()
    rc = lib.pnrf_lpips_create(net, ptr(bufs[:ns]), ptr(bufs[ns:2 * ns]), (C.c_int * max(4 * ns, 1))(*[d for s in shapes for d in s]), n, ptr(bufs[2 * ns:]),
                               (C.c_int * 5)(*lin_dims), C.byref(h))
    return rc, h, lib.pnrf_last_error()


def test_argument_and_shape_errors_are_reported(lib):
    from pronerf_amd import ops
    good = {net: (ops.LPIPS_CONVS[net], list(ops.LPIPS_LIN[net])) for net in ('alex', 'vgg')}
    rc, h, msg = _create(lib, b'squeeze', *good['alex'])
    assert rc == -1 and not h.value and b'squeeze' in msg and b'pnrf_lpips_create' in msg
    assert lib.pnrf_lpips_create(None, None, None, None, 0, None, None, None) == -1
    for net in ('alex', 'vgg'):
        shapes, lin = good[net]
        bad = list(shapes); bad[2] = (shapes[2][0], shapes[2][1] + 1, 3, 3)
        rc, h, msg = _create(lib, net.encode(), bad, lin)
        assert rc == -2 and not h.value and b'conv 2' in msg and b'Table of' in msg and str(list(shapes[0])).replace(' ', '').encode() in msg, msg
        rc, h, msg = _create(lib, net.encode(), shapes[:-1], lin)                       # a missing layer
        assert rc == -2 and not h.value and b'conv layers' in msg and b'Table of' in msg
        bad_lin = list(lin); bad_lin[4] += 1
        rc, h, msg = _create(lib, net.encode(), shapes, bad_lin)
        assert rc == -2 and not h.value and b'lin 4' in msg
    # tap_dims: the minimum, the maximum, the net
    hw = (C.c_int * 10)()
    for net, lo in (('alex', 31), ('vgg', 16)):
        for H, W, ok in ((lo, lo, True), (lo - 1, lo, False), (lo, lo - 1, False), (4096, lo, True), (4097, lo, False), (lo, 4097, False), (0, 0, False), (-5, 40, False)):
            assert (lib.pnrf_lpips_tap_dims(net.encode(), H, W, hw) == 0) == ok, (net, H, W)
    assert lib.pnrf_lpips_tap_dims(b'squeeze', 64, 64, hw) == -1 and b'squeeze' in lib.pnrf_last_error()
    assert lib.pnrf_lpips_tap_dims(b'vgg', 64, 64, None) == -1
    # without a handle nothing runs and no workspace size is given
    assert lib.pnrf_lpips_workspace_bytes(None, 64, 64) == 0 and lib.pnrf_lpips_layer_workspace_bytes(None, 0, 0, 64, 64) == 0
    assert lib.pnrf_lpips_fwd(None, None, 3, None, 3, 64, 64, 1, None, None, None, 0, None) == -1 and b'pnrf_lpips_fwd' in lib.pnrf_last_error()
    assert lib.pnrf_lpips_layer_fwd(None, 0, 0, None, 64, 64, None, None, 0, None) == -1 and b'pnrf_lpips_layer_fwd' in lib.pnrf_last_error()
    assert lib.pnrf_lpips_free(None) == 0


# ---- 4. the loader ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('style', ['torchvision', 'lpips'])
def test_loader_accepts_both_key_sets(net, style, tmp_path):
    from pronerf_amd import ops
    w = R.make_int_net(net)
    sd, lin = R.state_dicts(net, w, style)
    sd['classifier.1.weight'] = torch.zeros(8, 8)                                       # what a full torchvision checkpoint also holds
    if style == 'lpips':
        sd.update(lin)                                                                  # one file with everything: the lin entries are no conv layers,
        sd.update({k.replace('lin', 'lins.', 1): v.clone() for k, v in lin.items()})    # nor are those of a module list 'lins.<k>.model.1.weight'
        sd['scaling_layer.shift'] = torch.zeros(1, 3, 1, 1)
    W, B, L = ops.lpips_weights(net, sd, lin)
    assert all(torch.equal(x, y) for x, y in zip(W, w['W'])) and all(torch.equal(x, y) for x, y in zip(B, w['b']))
    assert all(torch.equal(x, y) for x, y in zip(L, w['lin'])) and [tuple(x.shape) for x in L] == [(c,) for c in R.lin_channels(net)]
    flat = {f'lin{k}.weight': v.clone() for k, v in enumerate(w['lin'])}                # [C] entries
    assert all(torch.equal(x, y) for x, y in zip(ops.lpips_weights(net, sd, flat)[2], w['lin']))
    if net == 'alex' and style == 'torchvision':                                        # paths: torch.load(weights_only=True)
        pb, pl = str(tmp_path / 'b.pth'), str(tmp_path / 'l.pth')
        torch.save(sd, pb); torch.save(lin, pl)
        assert all(torch.equal(x, y) for x, y in zip(ops.lpips_weights(net, pb, pl)[0], w['W']))


def test_loader_refuses_what_does_not_fit():
    from pronerf_amd import ops, run_nerf_helpers as hp
    from pronerf_amd._lib import PnrfError
    w = R.make_int_net('alex')
    sd, lin = R.state_dicts('alex', w)
    with pytest.raises(PnrfError, match='squeeze'):
        ops.lpips_weights('squeeze', sd, lin)
    bad = dict(sd); bad['features.6.weight'] = torch.zeros(384, 191, 3, 3)
    with pytest.raises(PnrfError, match=r'features\.6\.weight.*\(384, 192, 3, 3\)'):
        ops.lpips_weights('alex', bad, lin)
    missing = {k: v for k, v in sd.items() if not k.startswith('features.8.')}
    with pytest.raises(PnrfError, match='5 conv layers'):
        ops.lpips_weights('alex', missing, lin)
    nobias = {k: v for k, v in sd.items() if k != 'features.3.bias'}
    with pytest.raises(PnrfError, match=r'features\.3\.bias'):
        ops.lpips_weights('alex', nobias, lin)
    bad_lin = dict(lin); bad_lin['lin2.model.1.weight'] = torch.zeros(1, 383, 1, 1)
    with pytest.raises(PnrfError, match=r'lin2\.model\.1\.weight.*384'):
        ops.lpips_weights('alex', sd, bad_lin)
    with pytest.raises(PnrfError, match='lin4'):
        ops.lpips_weights('alex', sd, {k: v for k, v in lin.items() if not k.startswith('lin4')})
    with pytest.raises(PnrfError, match='5 conv layers.*found 13'):                     # a vgg backbone is no alex
        ops.lpips_weights('alex', R.state_dicts('vgg', R.make_int_net('vgg'))[0], lin)
    # nothing is fetched: without weights init_lpips says which two files to bring
    hp.LPIPS_WEIGHTS.clear()
    with pytest.raises(PnrfError, match=r'vgg16.*weights/v0\.1/vgg\.pth'):
        hp.init_lpips('vgg', 'cuda')
    with pytest.raises(PnrfError, match='squeeze'):
        hp.init_lpips('squeeze', 'cuda')


def test_metrics_option_takes_lpips_and_refuses_missing_files(tmp_path):
    from pronerf_amd import cli
    from pronerf_amd._lib import PnrfError
    from pronerf_amd.config import config_parser
    from pronerf_amd.run_S_eS_eN_alter_trt import lpips_from_args
    d = config_parser('trt').parse_args([])
    assert d.metrics == 'psnr' and d.lpips_net == 'vgg' and d.lpips_backbone is None and d.lpips_lin is None
    ns = cli.build_parser().parse_args(['infer', '--metrics', 'psnr,ssim,lpips', '--lpips_net', 'alex', '--lpips_backbone', 'b.pth', '--lpips_lin', 'l.pth'])
    argv = cli.infer_argv(ns)
    a = config_parser('trt').parse_args(argv[2:])                                       # behind '--config <file>'
    assert (a.metrics, a.lpips_net, a.lpips_backbone, a.lpips_lin) == ('psnr,ssim,lpips', 'alex', 'b.pth', 'l.pth')
    assert '--lpips_net' not in cli.infer_argv(cli.build_parser().parse_args(['infer', '--metrics', 'psnr,ssim']))
    with pytest.raises(PnrfError, match='lpips_backbone'):
        lpips_from_args(a, 'cuda')
    (tmp_path / 'b.pth').write_bytes(b'x')
    a.lpips_backbone = str(tmp_path / 'b.pth')
    with pytest.raises(PnrfError, match='lpips_lin'):
        lpips_from_args(a, 'cuda')
