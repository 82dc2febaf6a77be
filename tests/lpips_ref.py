"""Checker for LPIPS: the definition of include/pronerf_hip.h restated with torch on the CPU (``conv2d`` / ``max_pool2d``), line by line, the layer
tables, and a seeded net maker.  ``dtype`` selects the arithmetic: float64 is the yardstick, float32 shows what the same formulas cost in
straightforward single precision (the bound of tests/test_lpips_gpu.py).

No real weights: the operator is held to its definition with seeded ones.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# (c_in, c_out, k, stride, pad, pool window in front of the conv (stride 2; 0 = none), tap index behind it or -1)
ALEX = [(3, 64, 11, 4, 2, 0, 0), (64, 192, 5, 1, 2, 3, 1), (192, 384, 3, 1, 1, 3, 2), (384, 256, 3, 1, 1, 0, 3), (256, 256, 3, 1, 1, 0, 4)]
_VGG_W = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
_VGG_POOL = (2, 4, 7, 10)
_VGG_TAP = {1: 0, 3: 1, 6: 2, 9: 3, 12: 4}
VGG = [(3 if i == 0 else _VGG_W[i - 1], w, 3, 1, 1, 2 if i in _VGG_POOL else 0, _VGG_TAP.get(i, -1)) for i, w in enumerate(_VGG_W)]
TABLES = {'alex': ALEX, 'vgg': VGG}
MIN_SIZE = {'alex': 31, 'vgg': 16}
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# torchvision's indices of the conv layers inside ``features`` (the keys a user's backbone file has)
TV_INDEX = {'alex': [0, 3, 6, 8, 10], 'vgg': [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]}


def lin_channels(net):
    return [c for _, c, *_, tap in TABLES[net] if tap >= 0]


def make_net(net, seed=0, first_scale=1.0):
    """{'W': [out,in,k,k] fp32, 'b': [out] fp32, 'lin': [C] fp32}: conv weights N(0, 2 / fan_in), biases N(0, 0.05^2), lin uniform [0, 1) / C.
    ``first_scale`` multiplies layer 0's weights and bias (activations far above O(1))."""
    g = torch.Generator().manual_seed(1234 + 17 * seed + (0 if net == 'alex' else 1))
    W, b = [], []
    for i, (ci, co, k, *_r) in enumerate(TABLES[net]):
        s = first_scale if i == 0 else 1.0
        W.append((torch.randn(co, ci, k, k, generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5 * s).float())
        b.append((torch.randn(co, generator=g, dtype=torch.float64) * 0.05 * s).float())
    lin = [(torch.rand(c, generator=g, dtype=torch.float64) / c).float() for c in lin_channels(net)]
    return {'W': W, 'b': b, 'lin': lin}


def make_int_net(net, seed=0):
    """Integer weights in [-2, 2] and biases in [-8, 8] (exact layers); lin as make_net."""
    g = torch.Generator().manual_seed(4321 + 17 * seed + (0 if net == 'alex' else 1))
    W = [torch.randint(-2, 3, (co, ci, k, k), generator=g).float() for ci, co, k, *_r in TABLES[net]]
    b = [torch.randint(-8, 9, (co,), generator=g).float() for _, co, *_r in TABLES[net]]
    lin = [(torch.rand(c, generator=g, dtype=torch.float64) / c).float() for c in lin_channels(net)]
    return {'W': W, 'b': b, 'lin': lin}


def state_dicts(net, w, style='torchvision'):
    """(backbone, lin) state dicts with the keys of a torchvision checkpoint (``features.<idx>.*``) or of the lpips package (``net.slice<k>.<idx>.*``;
    ``lin<k>.model.1.weight`` of shape [1,C,1,1])."""
    sd = {}
    for i, idx in enumerate(TV_INDEX[net]):
        taps_before = sum(1 for j in range(i) if TABLES[net][j][6] >= 0)
        pre = f'features.{idx}' if style == 'torchvision' else f'net.slice{1 + taps_before}.{idx}'
        sd[pre + '.weight'], sd[pre + '.bias'] = w['W'][i].clone(), w['b'][i].clone()
    lin = {f'lin{k}.model.1.weight': v.reshape(1, -1, 1, 1).clone() for k, v in enumerate(w['lin'])}
    return sd, lin


def layer_ref(net, layer, x_nchw, W, b, pool_first, dtype=torch.float64):
    """[pool] -> conv -> bias -> ReLU of one layer on an NCHW batch."""
    _, _, k, stride, pad, pool, _ = TABLES[net][layer]
    x = x_nchw.to(dtype)
    if pool_first:
        x = F.max_pool2d(x, pool, 2)                                     # no padding, floor sizes
    return F.relu(F.conv2d(x, W.to(dtype), b.to(dtype), stride=stride, padding=pad))


def tap_dims(net, H, W):
    out, h, w = [], H, W
    for _, _, k, stride, pad, pool, tap in TABLES[net]:
        if pool:
            h, w = (h - pool) // 2 + 1, (w - pool) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        if tap >= 0:
            out.append((h, w))
    return out


def features(net, w, img, normalize=True, dtype=torch.float64):
    """The five taps [C_k, h_k, w_k] of one [H,W,3] image."""
    x = torch.as_tensor(np.asarray(img)).to(dtype)
    if normalize:
        x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    x = x.permute(2, 0, 1)[None]
    taps = []
    for i, spec in enumerate(TABLES[net]):
        x = layer_ref(net, i, x, w['W'][i], w['b'][i], spec[5] != 0, dtype)
        if spec[6] >= 0:
            taps.append(x[0])
    return taps


def lpips_ref(net, w, a, b, normalize=True, dtype=torch.float64):
    """(d, [m_1 .. m_5]) — d a Python float (the means and their sum in float64), m_k [h_k, w_k] tensors of ``dtype``."""
    fa, fb = features(net, w, a, normalize, dtype), features(net, w, b, normalize, dtype)
    maps = []
    for k in range(5):
        na = fa[k] / (torch.sqrt((fa[k] ** 2).sum(0, keepdim=True)) + dtype_eps(dtype))
        nb = fb[k] / (torch.sqrt((fb[k] ** 2).sum(0, keepdim=True)) + dtype_eps(dtype))
        maps.append((w['lin'][k].to(dtype)[:, None, None] * (na - nb) ** 2).sum(0))
    return float(sum(m.double().mean() for m in maps)), maps


def dtype_eps(dtype):
    return torch.tensor(1e-10, dtype=dtype)


def make_pair(kind, H, W, seed=0):
    """tests/ssim_ref.make_pair kinds plus 'mix': pred = 0.6 gt + 0.4 noise."""
    import ssim_ref
    if kind == 'mix':
        rs = np.random.RandomState(5000 + 1000 * seed + 97 * H + W)
        gt, _ = ssim_ref.make_pair('smooth', H, W, seed)
        return (0.6 * gt + 0.4 * rs.uniform(0, 1, (H, W, 3))).astype(np.float32), gt
    return ssim_ref.make_pair(kind, H, W, seed)


@functools.lru_cache(maxsize=None)
def cached_net(net, first_scale=1.0):
    return make_net(net, 0, first_scale)
