"""Thin torch-tensor wrappers over the C ABI (device memory + stream plumbing only).

Every function takes contiguous fp32 CUDA(ROCm) tensors, allocates its outputs with torch and
launches on ``torch.cuda.current_stream()``.  No arithmetic happens on the Python side.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import NET_NERF, NET_NERFCLS, NET_REFINE, NET_SAMPLER, PnrfError, check

f32 = torch.float32


def _ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, shape_tail=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PnrfError(f'{name}: expected a GPU tensor (pronerf_amd has no CPU path)')
    if t.dtype != f32:
        raise PnrfError(f'{name}: expected float32, got {t.dtype}')
    if shape_tail is not None and tuple(t.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise PnrfError(f'{name}: expected trailing shape {shape_tail}, got {tuple(t.shape)}')
    return t.contiguous()


def _chk_rows(t, name, width):
    """[n, width] rows with contiguous columns and any row stride >= width, e.g. rays[:, 3:6] of the [n, 11] rays: (tensor, row stride),
    without a copy.  Any other layout goes through _chk (checked, made contiguous; row stride = width)."""
    if (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == f32 and t.dim() == 2 and t.shape[1] == width and t.stride(1) == 1
            and t.stride(0) >= width):
        return t, t.stride(0)
    return _chk(t, name, (width,)), width


class PackedMLP:
    """Device-resident pre-tiled weights of one network (pnrf_mlp_pack)."""

    def __init__(self, net: int, weights, biases, variant=None):
        """variant: None / 'default', or one of ``_lib.VARIANTS`` ('sampler_f32', 'sampler_f32_full', 'bf16_32x32') — fixed for the
        life of the handle (pnrf_mlp_set_variant); nothing is read from the environment."""
        lib = _lib.load()
        (ws, _bs), args = self._pack_args(weights, biases)
        h = C.c_void_p()
        check(lib.pnrf_mlp_pack(net, *args, C.byref(h)), 'pnrf_mlp_pack')
        self.handle = h
        self.net = net
        self.in_dim = ws[0].shape[1]
        self.out_dim = 4 if net == NET_NERFCLS else ws[-1].shape[0]      # NeRF class: [rgb(3), alpha]
        self.skips = self._read_skips()
        self.variant = 'default'
        if variant not in (None, 'default'):
            self.set_variant(variant)

    @staticmethod
    def _pack_args(weights, biases):
        """-> ((float32 weight arrays, bias arrays): to be kept alive over the call, (W, b, in_dim, out_dim, n_layers) of pnrf_mlp_pack / pnrf_mlp_pack_image)."""
        n = len(weights)
        ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32) for w in weights]
        bs = [np.ascontiguousarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float32) for b in biases]
        Wp = (C.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        return (ws, bs), (Wp, bp, (C.c_int * n)(*[w.shape[1] for w in ws]), (C.c_int * n)(*[w.shape[0] for w in ws]), n)

    @classmethod
    def pack_image(cls, net: int, weights, biases) -> bytes:
        """The engine image of a net packed on the host (pnrf_mlp_pack_image): the bytes ``PackedMLP(net, weights, biases).serialize()`` returns, without a device."""
        lib = _lib.load()
        _keep, args = cls._pack_args(weights, biases)
        size = C.c_int64()
        check(lib.pnrf_mlp_pack_image(net, *args, None, 0, C.byref(size)), 'pnrf_mlp_pack_image')
        buf = (C.c_char * size.value)()
        check(lib.pnrf_mlp_pack_image(net, *args, buf, size.value, C.byref(size)), 'pnrf_mlp_pack_image')
        return bytes(buf)

    def repack(self, weights, biases):
        """Rewrite the handle's weights in place, on the device, from float32 GPU tensors W[out, in] / b[out] of the handle's shape (pnrf_mlp_repack):
        kernels on the current stream write the bytes ``pack_image(net, weights, biases)`` holds into the handle's buffers, at the same addresses, so a
        ``Context``, ``Renderer`` or ``PoseGraph`` built on the handle renders the new weights from its next launch in stream order.  No host
        synchronisation; from the second call on nothing is allocated, and the call can be captured in a graph.  Another shape or net kind raises
        ``PnrfError`` and leaves the handle as it was.  -> self.  (``Renderer.calibrate()`` depends on the weights: call it again if it matters.)"""
        n = len(weights)
        if len(biases) != n:
            raise PnrfError(f'repack: {n} weight matrices, {len(biases)} bias vectors')
        ws = [_chk(w, f'weights[{l}]') for l, w in enumerate(weights)]
        bs = [_chk(b, f'biases[{l}]') for l, b in enumerate(biases)]
        if any(w.dim() != 2 for w in ws) or any(b.dim() != 1 or b.shape[0] != w.shape[0] for w, b in zip(ws, bs)):
            raise PnrfError('repack: expected W[out, in] matrices and b[out] vectors')
        args = ((C.c_void_p * n)(*[w.data_ptr() for w in ws]), (C.c_void_p * n)(*[b.data_ptr() for b in bs]),
                (C.c_int * n)(*[w.shape[1] for w in ws]), (C.c_int * n)(*[w.shape[0] for w in ws]), n)
        check(_lib.load().pnrf_mlp_repack(self.handle, *args, _stream()), 'pnrf_mlp_repack')
        return self

    def set_variant(self, variant):
        """Configuration step (before the handle is used by a context / stream)."""
        if variant not in _lib.VARIANTS:
            raise PnrfError(f'unknown kernel variant {variant!r}; one of {sorted(_lib.VARIANTS)}')
        check(_lib.load().pnrf_mlp_set_variant(self.handle, _lib.VARIANTS[variant]), 'pnrf_mlp_set_variant')
        self.variant = variant
        return self

    def _read_skips(self):
        """Backbone layers of a sampler / refine stack behind which the net input is concatenated back (``--mmnetskips``), from the handle's mask."""
        mask = C.c_uint32()
        check(_lib.load().pnrf_mlp_skips(self.handle, C.byref(mask)), 'pnrf_mlp_skips')
        return [i for i in range(32) if (mask.value >> i) & 1]

    SHAPES = {'auto': 0, 'narrow': 4, 'wide': 8}

    def set_shape(self, shape):
        """Workgroup shape of the fused stages launched from this handle (pnrf_mlp_set_shape): 'auto' (per launch, the default), 'wide',
        'narrow', or the PNRF_SHAPE_* integer — bit-identical results, A/B timing."""
        v = self.SHAPES.get(shape, shape) if isinstance(shape, str) else shape
        if isinstance(v, str):
            raise PnrfError(f'unknown workgroup shape {shape!r}; one of {sorted(self.SHAPES)}')
        check(_lib.load().pnrf_mlp_set_shape(self.handle, int(v)), 'pnrf_mlp_set_shape')
        return self

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().pnrf_mlp_free(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- engine files: the packed stream as bytes (pnrf_mlp_serialize / pnrf_mlp_deserialize)
    def serialize(self) -> bytes:
        lib = _lib.load()
        size = C.c_int64()
        check(lib.pnrf_mlp_serialize(self.handle, None, 0, C.byref(size)), 'pnrf_mlp_serialize')
        buf = (C.c_char * size.value)()
        check(lib.pnrf_mlp_serialize(self.handle, buf, size.value, C.byref(size)), 'pnrf_mlp_serialize')
        return bytes(buf)

    @classmethod
    def deserialize(cls, data: bytes, expect_net=None):
        """New handle on the current device from ``serialize()`` output; ``expect_net`` (NET_*) guards against swapped files."""
        lib = _lib.load()
        data = bytes(data)
        h = C.c_void_p()
        check(lib.pnrf_mlp_deserialize(data, len(data), C.byref(h)), 'pnrf_mlp_deserialize')
        self = cls.__new__(cls)
        self.handle = h
        net, ind, indx, outd = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib.pnrf_mlp_kind(h, C.byref(net), C.byref(ind), C.byref(indx), C.byref(outd)), 'pnrf_mlp_kind')
        self.net, self.in_dim, self.out_dim = net.value, ind.value, outd.value
        self.skips = self._read_skips()
        self.variant = 'default'
        if expect_net is not None and self.net != expect_net:
            raise PnrfError(f'engine holds net kind {self.net}, expected {expect_net}')
        return self

    def save(self, path):
        with open(path, 'wb') as f:
            f.write(self.serialize())

    @classmethod
    def load(cls, path, expect_net=None):
        with open(path, 'rb') as f:
            return cls.deserialize(f.read(), expect_net)

    def forward(self, x, x_views=None, head_act=False):
        """Output of the last Linear, [m, out_dim]; head_act applies the TRT classes' sigmoid/tanh heads."""
        x = _chk(x, 'x', (self.in_dim,))
        m = x.shape[0]
        y = torch.empty(m, self.out_dim, device=x.device, dtype=f32)
        if x_views is not None:
            x_views = _chk(x_views, 'x_views', (27,))
        check(_lib.load().pnrf_mlp_fwd(self.handle, _ptr(x), _ptr(x_views), _ptr(y), m, int(bool(head_act)), _stream()), 'pnrf_mlp_fwd')
        return y


def posenc(x, n_freq):
    x = _chk(x, 'x', (3,))
    lead = x.shape[:-1]
    xf = x.reshape(-1, 3)
    out = torch.empty(xf.shape[0], 3 + 6 * n_freq, device=x.device, dtype=f32)
    check(_lib.load().pnrf_posenc_fwd(_ptr(xf), _ptr(out), xf.shape[0], n_freq, _stream()), 'pnrf_posenc_fwd')
    return out.reshape(*lead, 3 + 6 * n_freq)


def plucker(o, d):
    o = _chk(o, 'rays_o', (3,)); d = _chk(d, 'rays_d', (3,))
    if o.shape != d.shape:
        raise PnrfError(f'plucker: shape mismatch {tuple(o.shape)} vs {tuple(d.shape)}')
    lead = o.shape[:-1]
    of, df = o.reshape(-1, 3), d.reshape(-1, 3)
    out = torch.empty(of.shape[0], 6, device=o.device, dtype=f32)
    check(_lib.load().pnrf_plucker_fwd(_ptr(of), _ptr(df), _ptr(out), of.shape[0], _stream()), 'pnrf_plucker_fwd')
    return out.reshape(*lead, 6)


def ray_encode(rays, n_pts=48):
    rays = _chk(rays, 'rays', (11,))
    out = torch.empty(rays.shape[0], 6 * n_pts, device=rays.device, dtype=f32)
    check(_lib.load().pnrf_ray_encode_fwd(_ptr(rays), _ptr(out), rays.shape[0], n_pts, _stream()), 'pnrf_ray_encode_fwd')
    return out


def frame_rays(K, c2w, H, W, near=0.0, far=1.0, or_near=1.0, or_far=10.0, first=0, count=None, device='cuda', block=None, stride=0):
    """rays[count,11], or_rays[count,11] for flat pixel range [first, first+count); with ``block`` / ``stride``: row q is pixel
    first + (q // block) * stride + q % block (a rank's share of a block-cyclic partition, pnrf_frame_rays_blocks_fwd)."""
    count = H * W - first if count is None else count
    Kh = np.ascontiguousarray(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32).reshape(3, 3))
    Ch = np.ascontiguousarray(np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)[:3, :4])
    rays = torch.empty(count, 11, device=device, dtype=f32)
    orr = torch.empty(count, 11, device=device, dtype=f32)
    fp = C.POINTER(C.c_float)
    if block is None:
        check(_lib.load().pnrf_frame_rays_fwd(Kh.ctypes.data_as(fp), Ch.ctypes.data_as(fp), H, W, near, far, or_near, or_far,
                                              first, count, _ptr(rays), _ptr(orr), _stream()), 'pnrf_frame_rays_fwd')
    else:
        check(_lib.load().pnrf_frame_rays_blocks_fwd(Kh.ctypes.data_as(fp), Ch.ctypes.data_as(fp), H, W, near, far, or_near, or_far,
                                                     first, int(block), int(stride), count, _ptr(rays), _ptr(orr), _stream()), 'pnrf_frame_rays_blocks_fwd')
    return rays, orr


def _dev_mat(t, name, shape):
    """A contiguous fp32 GPU tensor of exactly ``shape`` (a camera matrix in device memory), used in place."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != f32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise PnrfError(f'{name}: expected a contiguous float32 GPU tensor {list(shape)}, got {getattr(t, "dtype", type(t))} '
                        f'{tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')
    return t


def frame_rays_dev(K, c2w, H, W, near=0.0, far=1.0, or_near=1.0, or_far=10.0, first=0, count=None, block=None, stride=0):
    """``frame_rays`` with the camera in device memory (pnrf_frame_rays_dev_fwd): K [3,3] and c2w [3,4] are GPU tensors read by the kernel in stream
    order — no host copy, no synchronisation; bit-identical rows."""
    K = _dev_mat(K, 'K', (3, 3)); c2w = _dev_mat(c2w, 'c2w', (3, 4))
    count = H * W - first if count is None else count
    rays = torch.empty(count, 11, device=c2w.device, dtype=f32)
    orr = torch.empty(count, 11, device=c2w.device, dtype=f32)
    check(_lib.load().pnrf_frame_rays_dev_fwd(_ptr(K), _ptr(c2w), H, W, near, far, or_near, or_far, first, int(max(count, 1) if block is None else block),
                                              int(0 if block is None else stride), count, _ptr(rays), _ptr(orr), _stream()), 'pnrf_frame_rays_dev_fwd')
    return rays, orr


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    rays_o = _chk(rays_o, 'rays_o', (3,)); rays_d = _chk(rays_d, 'rays_d', (3,))
    lead = rays_o.shape
    of, df = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    oo = torch.empty_like(of); od = torch.empty_like(df)
    check(_lib.load().pnrf_ndc_rays_fwd(_ptr(of), _ptr(df), int(H), int(W), float(focal), float(near), _ptr(oo), _ptr(od), of.shape[0], _stream()),
          'pnrf_ndc_rays_fwd')
    return oo.reshape(lead), od.reshape(lead)


def warp_trt(img, depth, ro1, rd1, w2c):
    """img [B,3,Hf,Wf]; depth [B,n]; ro1, rd1 [4,n] (shared) or [B,4,n]; w2c [B,3,4] -> [B,3,n]."""
    img = _chk(img, 'img'); depth = _chk(depth, 'depth'); w2c = _chk(w2c, 'w2c', (3, 4))
    B, _, Hf, Wf = img.shape
    n = depth.shape[-1]
    if ro1.dim() == 3 and ro1.stride(0) == 0:       # the reference's expand(): one copy shared by all B
        ro1, rd1 = ro1[0], rd1[0]
    ro1 = _chk(ro1, 'ro1'); rd1 = _chk(rd1, 'rd1')
    bstride = 4 * n if ro1.dim() == 3 else 0
    out = torch.empty(B, 3, n, device=img.device, dtype=f32)
    check(_lib.load().pnrf_warp_trt_fwd(_ptr(img), _ptr(depth), _ptr(ro1), _ptr(rd1), bstride, _ptr(w2c), _ptr(out), B, Hf, Wf, n, _stream()),
          'pnrf_warp_trt_fwd')
    return out


def warp_train(img, depth, ro1, rd1, c2w2, K):
    """Training warp: img [B,3,Hf,Wf]; depth [B,n]; ro1, rd1 [3,n] (shared) or [B,3,n]; c2w2 [B,3,4]; K [B,3,3] -> [B,3,n]."""
    img = _chk(img, 'img'); depth = _chk(depth, 'depth'); c2w2 = _chk(c2w2, 'c2w2', (3, 4)); K = _chk(K, 'intrinsics', (3, 3))
    B, _, Hf, Wf = img.shape
    n = depth.shape[-1]
    if ro1.dim() == 3 and ro1.stride(0) == 0:
        ro1, rd1 = ro1[0], rd1[0]
    ro1 = _chk(ro1, 'ro1'); rd1 = _chk(rd1, 'rd1')
    bstride = 3 * n if ro1.dim() == 3 else 0
    out = torch.empty(B, 3, n, device=img.device, dtype=f32)
    check(_lib.load().pnrf_warp_train_fwd(_ptr(img), _ptr(depth), _ptr(ro1), _ptr(rd1), bstride, _ptr(c2w2), _ptr(K), _ptr(out), B, Hf, Wf, n, _stream()),
          'pnrf_warp_train_fwd')
    return out


def refine_input_train(rays, or_rays, depth_sorted, img4, poses, K, ref_nos, eps=1e-5, layout=0):
    rays = _chk(rays, 'rays', (11,)); or_rays = _chk(or_rays, 'or_rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    img4 = _chk(img4, 'img4', (4,)); poses = _chk(poses, 'poses', (3, 4)); K = _chk(K, 'K', (3, 3))
    if ref_nos.dtype != torch.int64 or not ref_nos.is_cuda or ref_nos.shape != (rays.shape[0], 4):
        raise PnrfError(f'refine_input_train: ref_nos must be a GPU int64 tensor [n,4], got {ref_nos.dtype} {tuple(ref_nos.shape)}')
    ref_nos = ref_nos.contiguous()
    nv, Hf, Wf, _ = img4.shape
    n = rays.shape[0]
    out = torch.empty(n, 144, device=rays.device, dtype=f32)
    check(_lib.load().pnrf_refine_input_train_fwd(_ptr(rays), _ptr(or_rays), _ptr(depth_sorted), _ptr(img4), _ptr(poses), _ptr(K), _ptr(ref_nos),
                                                  nv, 4, Hf, Wf, eps, int(layout), _ptr(out), n, _stream()), 'pnrf_refine_input_train_fwd')
    return out


def refine_train_fwd(mlp, refine_in, rays, depth_sorted, jitter=None, jitter_dir=1, want_rgb0=True):
    refine_in = _chk(refine_in, 'refine_in', (144,)); rays = _chk(rays, 'rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    jitter = None if jitter is None else _chk(jitter, 'jitter', (8,))
    n, dev = rays.shape[0], rays.device
    z = torch.empty(n, 8, device=dev, dtype=f32); pts = torch.empty(n, 8, 3, device=dev, dtype=f32)
    rgb0 = torch.empty(n, 3, device=dev, dtype=f32) if want_rgb0 else None
    check(_lib.load().pnrf_refine_train_fwd(mlp.handle, _ptr(refine_in), _ptr(rays), _ptr(depth_sorted), _ptr(jitter), int(jitter_dir),
                                            _ptr(z), _ptr(pts), _ptr(rgb0), n, _stream()), 'pnrf_refine_train_fwd')
    return z, pts, rgb0


def nerf_train_fwd(mlp, pts, rays, z=None, add=None, mul=None, noise=None, clamp=0.0, white_bkgd=False, want_raw=False):
    """pts [n,S,3].  S == 8: fused compositing -> (rgbd [n,4], raw|None).  S != 8: -> (None, raw [n,S,4])."""
    pts = _chk(pts, 'pts', (3,)); rays = _chk(rays, 'rays', (11,))
    n, S, dev = rays.shape[0], pts.shape[1], rays.device
    if pts.shape[0] != n:
        raise PnrfError(f'nerf_train_fwd: pts {tuple(pts.shape)} does not match {n} rays')
    z = None if z is None else _chk(z, 'z'); add = None if add is None else _chk(add, 'add'); mul = None if mul is None else _chk(mul, 'mul')
    noise = None if noise is None else _chk(noise, 'noise')
    fused = S == 8
    rgbd = torch.empty(n, 4, device=dev, dtype=f32) if fused else None
    raw = torch.empty(n, S, 4, device=dev, dtype=f32) if (want_raw or not fused) else None
    check(_lib.load().pnrf_nerf_train_fwd(mlp.handle, _ptr(pts), _ptr(rays), _ptr(z), _ptr(add), _ptr(mul), _ptr(noise), float(clamp),
                                          int(bool(white_bkgd)), int(S), _ptr(rgbd), _ptr(raw), n, _stream()), 'pnrf_nerf_train_fwd')
    return rgbd, raw


def explore(z8, rays, jitter, n_mult, dir1, dir2):
    """Stage-1 exploration: z8 [n,8], jitter [n, 8*n_mult] -> (z [n, 8*n_mult], pts [n, 8*n_mult, 3])."""
    z8 = _chk(z8, 'z8', (8,)); rays = _chk(rays, 'rays', (11,)); jitter = _chk(jitter, 'jitter', (8 * n_mult,))
    n, dev = rays.shape[0], rays.device
    z = torch.empty(n, 8 * n_mult, device=dev, dtype=f32); pts = torch.empty(n, 8 * n_mult, 3, device=dev, dtype=f32)
    check(_lib.load().pnrf_explore_fwd(_ptr(z8), _ptr(rays), _ptr(jitter), int(n_mult), int(dir1), int(dir2), _ptr(z), _ptr(pts), n, _stream()),
          'pnrf_explore_fwd')
    return z, pts


def images_pack(img_nchw):
    img = _chk(img_nchw, 'images')
    nv, c, Hf, Wf = img.shape
    if c != 3:
        raise PnrfError(f'images_pack: expected [nv,3,H,W], got {tuple(img.shape)}')
    out = torch.empty(nv, Hf, Wf, 4, device=img.device, dtype=f32)
    check(_lib.load().pnrf_images_pack(_ptr(img), _ptr(out), nv, Hf, Wf, _stream()), 'pnrf_images_pack')
    return out


def refine_input(rays, or_rays, depth_sorted, img4, proj, eps=1e-5):
    rays = _chk(rays, 'rays', (11,)); or_rays = _chk(or_rays, 'or_rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    img4 = _chk(img4, 'img4', (4,)); proj = _chk(proj, 'proj', (3, 4))
    nb, Hf, Wf, _ = img4.shape                   # any 1 .. 8 neighbour views: refine_in is [n, 48 + 24 nb] (nb = 4: 144)
    if proj.shape[0] != nb:
        raise PnrfError(f'refine_input: {nb} packed images but {proj.shape[0]} projection matrices')
    n = rays.shape[0]
    out = torch.empty(n, 48 + 24 * nb, device=rays.device, dtype=f32)
    check(_lib.load().pnrf_refine_input_fwd(_ptr(rays), _ptr(or_rays), _ptr(depth_sorted), _ptr(img4), _ptr(proj), nb, Hf, Wf, eps,
                                            _ptr(out), n, _stream()), 'pnrf_refine_input_fwd')
    return out


def composite(raw, z, rays_d, add=None, mul=None, noise=None, clamp=0.0, white_bkgd=False):
    """raw2outputs -> (rgb, disp, acc, weights, depth).  rays_d may be a row-strided [n, 3] view (rays[:, 3:6] of the [n, 11] rays)."""
    raw = _chk(raw, 'raw', (4,)); z = _chk(z, 'z_vals'); rays_d, d_stride = _chk_rows(rays_d, 'rays_d', 3)
    n, s = z.shape
    add = None if add is None else _chk(add, 'mm_density_add')
    mul = None if mul is None else _chk(mul, 'mm_density_mul')
    noise = None if noise is None else _chk(noise, 'noise')
    dev = raw.device
    rgb = torch.empty(n, 3, device=dev, dtype=f32); disp = torch.empty(n, device=dev, dtype=f32)
    acc = torch.empty(n, device=dev, dtype=f32); w = torch.empty(n, s, device=dev, dtype=f32); depth = torch.empty(n, device=dev, dtype=f32)
    check(_lib.load().pnrf_composite_fwd(_ptr(raw), _ptr(z), _ptr(rays_d), d_stride, _ptr(add), _ptr(mul), _ptr(noise), float(clamp),
                                         int(bool(white_bkgd)), _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(w), _ptr(depth), n, s, _stream()),
          'pnrf_composite_fwd')
    return rgb, disp, acc, w, depth


def sampler_fwd(mlp: PackedMLP, rays, want_idx=True, want_rgb=True, want_raw=False, two_pass=False, kappa=None, want_lists=False, workspace=None):
    """pnrf_sampler_fwd; two_pass=True: pnrf_sampler_fwd_ws (plain-fp16 pass for every ray + split-fp16 pass for the undecided ones, what
    the fused path runs) and the numbers of rays of the second (split fp16) and third (exact fp32: saturated activations) pass as a seventh
    and eighth return value (0-d int32 tensors on the device).  want_lists=True: also the two lists themselves, as views [n] of the workspace
    (int32 ray numbers in no particular order; only the first ``count`` entries of each belong to this call).  workspace: an int32 tensor of
    at least pnrf_sampler_workspace_bytes(n) / 4 words to run on (a fresh one otherwise)."""
    rays = _chk(rays, 'rays', (11,))
    n, dev = rays.shape[0], rays.device
    depth = torch.empty(n, 8, device=dev, dtype=f32); add = torch.empty_like(depth); mul = torch.empty_like(depth)
    idx = torch.empty(n, 8, device=dev, dtype=torch.int64) if want_idx else None
    rgb = torch.empty(n, 3, device=dev, dtype=f32) if want_rgb else None
    draw = torch.empty(n, 8, device=dev, dtype=f32) if want_raw else None
    if two_pass:
        lib = _lib.load()
        nb = int(lib.pnrf_sampler_workspace_bytes(n))
        ws = torch.empty(max(nb, 64) // 4, device=dev, dtype=torch.int32) if workspace is None else workspace
        if ws.dtype != torch.int32 or ws.device != dev or not ws.is_contiguous() or ws.numel() * 4 < nb:
            raise PnrfError(f'sampler_fwd: workspace must be a contiguous int32 tensor of at least {nb // 4} words on {dev}')
        check(lib.pnrf_sampler_fwd_ws(mlp.handle, _ptr(rays), n, _ptr(depth), _ptr(add), _ptr(mul), _ptr(idx), _ptr(rgb), _ptr(draw), _ptr(ws), nb,
                                      -1.0 if kappa is None else float(kappa), _stream()), 'pnrf_sampler_fwd_ws')
        if want_lists:
            return depth, idx, add, mul, rgb, draw, ws[1], ws[5], ws[16:16 + n], ws[16 + n:16 + 2 * n]
        return depth, idx, add, mul, rgb, draw, ws[1], ws[5]
    check(_lib.load().pnrf_sampler_fwd(mlp.handle, _ptr(rays), n, _ptr(depth), _ptr(add), _ptr(mul), _ptr(idx), _ptr(rgb), _ptr(draw), _stream()),
          'pnrf_sampler_fwd')
    return depth, idx, add, mul, rgb, draw


def refine_fwd(mlp: PackedMLP, refine_in, rays, depth_sorted):
    refine_in = _chk(refine_in, 'refine_in', (mlp.in_dim,)); rays = _chk(rays, 'rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    n, dev = rays.shape[0], rays.device
    z = torch.empty(n, 8, device=dev, dtype=f32); pts = torch.empty(n, 8, 3, device=dev, dtype=f32)
    check(_lib.load().pnrf_refine_fwd(mlp.handle, _ptr(refine_in), _ptr(rays), _ptr(depth_sorted), _ptr(z), _ptr(pts), n, _stream()), 'pnrf_refine_fwd')
    return z, pts


def refine_project_fwd(mlp: PackedMLP, rays, or_rays, depth_sorted, img4, proj, eps=1e-5):
    """Projection into the neighbour views + refine MLP + interval refinement in one kernel (pnrf_refine_project_fwd) -> (z [n,8], pts [n,8,3])."""
    rays = _chk(rays, 'rays', (11,)); or_rays = _chk(or_rays, 'or_rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    img4 = _chk(img4, 'img4', (4,)); proj = _chk(proj, 'proj', (3, 4))
    nb, Hf, Wf, _ = img4.shape
    if proj.shape[0] != nb:
        raise PnrfError(f'refine_project_fwd: {nb} packed images but {proj.shape[0]} projection matrices')
    n, dev = rays.shape[0], rays.device
    z = torch.empty(n, 8, device=dev, dtype=f32); pts = torch.empty(n, 8, 3, device=dev, dtype=f32)
    check(_lib.load().pnrf_refine_project_fwd(mlp.handle, _ptr(rays), _ptr(or_rays), _ptr(depth_sorted), _ptr(img4), _ptr(proj), nb, Hf, Wf, eps,
                                              _ptr(z), _ptr(pts), n, _stream()), 'pnrf_refine_project_fwd')
    return z, pts


def nerf_fwd(mlp: PackedMLP, pts, rays, z, add, mul, want_raw=False):
    pts = _chk(pts, 'pts', (8, 3)); rays = _chk(rays, 'rays', (11,)); z = _chk(z, 'z', (8,)); add = _chk(add, 'add', (8,)); mul = _chk(mul, 'mul', (8,))
    n, dev = rays.shape[0], rays.device
    rgbd = torch.empty(n, 4, device=dev, dtype=f32)
    raw = torch.empty(n, 8, 4, device=dev, dtype=f32) if want_raw else None
    check(_lib.load().pnrf_nerf_fwd(mlp.handle, _ptr(pts), _ptr(rays), _ptr(z), _ptr(add), _ptr(mul), _ptr(rgbd), _ptr(raw), n, _stream()), 'pnrf_nerf_fwd')
    return rgbd, raw


class RenderContext:
    """pnrf_ctx: per-ray workspace for the whole inference path (sized once)."""

    def __init__(self, sampler: PackedMLP, refine: PackedMLP, nerf: PackedMLP, max_rays: int):
        self._keep = (sampler, refine, nerf)
        h = C.c_void_p()
        check(_lib.load().pnrf_ctx_create(sampler.handle, refine.handle, nerf.handle, int(max_rays), C.byref(h)), 'pnrf_ctx_create')
        self.handle = h
        self.max_rays = int(max_rays)

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().pnrf_ctx_free(self.handle)
                self.handle = None
        except Exception:
            pass

    STAGES = ('sampler_kernel', 'refine_kernel', 'nerf_kernel')

    def sampler_stats(self):
        """Rays the sampler's second (split-fp16) pass rendered in the most recent render_rays call; waits for the device."""
        v = C.c_int64()
        check(_lib.load().pnrf_ctx_sampler_stats(self.handle, C.byref(v)), 'pnrf_ctx_sampler_stats')
        return int(v.value)

    def sampler_saturated(self):
        """Rays the exact-fp32 third pass rendered in the most recent render_rays call (activations at the fp16 limit); waits for the device."""
        v = C.c_int64()
        check(_lib.load().pnrf_ctx_sampler_saturated(self.handle, C.byref(v)), 'pnrf_ctx_sampler_saturated')
        return int(v.value)

    def set_sampler_kappa(self, kappa):
        """Threshold of the two-pass sampler for this context (pnrf_ctx_set_sampler_kappa): negative = the library default (PNRF_SAMPLER_KAPPA of
        include/pronerf_hip.h; ``sampler_kappa()`` reports it), 0 = only the fp32 round-off allowance; NaN / inf are refused."""
        check(_lib.load().pnrf_ctx_set_sampler_kappa(self.handle, float(kappa)), 'pnrf_ctx_set_sampler_kappa')

    def sampler_kappa(self):
        """The threshold this context's calls run with (pnrf_ctx_get_sampler_kappa)."""
        v = C.c_float()
        check(_lib.load().pnrf_ctx_get_sampler_kappa(self.handle, C.byref(v)), 'pnrf_ctx_get_sampler_kappa')
        return float(v.value)

    NERF_SKIP = {'never': 0, 'auto': 1, 'always': 2}

    def set_nerf_skip(self, mode):
        """NeRF stage of render_rays (pnrf_ctx_set_nerf_skip): 'never' = the fused kernel alone, 'auto' (a new context) = large calls evaluate only the samples
        whose sampler gate is open (mul > 0) when enough are closed, 'always' = that path whatever the call size or share.  Same rgbd bit for bit."""
        check(_lib.load().pnrf_ctx_set_nerf_skip(self.handle, int(self.NERF_SKIP.get(mode, mode))), 'pnrf_ctx_set_nerf_skip')

    def nerf_live(self):
        """-> (live columns, list mode) of the most recent render_rays call (pnrf_ctx_nerf_live): samples with mul > 0 the builder counted (-1 if the call
        did not take the compacted-column path) and whether the MLP ran over the list; waits for the device."""
        v, m = C.c_int64(), C.c_int()
        check(_lib.load().pnrf_ctx_nerf_live(self.handle, C.byref(v), C.byref(m)), 'pnrf_ctx_nerf_live')
        return int(v.value), bool(m.value)

    def profile_begin(self, max_frames=64):
        """Record per-stage events on the next ``max_frames`` render_rays calls (pnrf_ctx_profile_begin)."""
        check(_lib.load().pnrf_ctx_profile_begin(self.handle, int(max_frames)), 'pnrf_ctx_profile_begin')

    def profile_end(self):
        """-> ({stage: mean ms}, frames recorded); waits for the last recorded call."""
        ms = (C.c_float * len(self.STAGES))()
        frames = C.c_int()
        check(_lib.load().pnrf_ctx_profile_end(self.handle, ms, C.byref(frames)), 'pnrf_ctx_profile_end')
        return dict(zip(self.STAGES, (float(v) for v in ms))), frames.value

    def render_rays(self, rays, or_rays, img4, proj, eps=1e-5, want_idx=False, out=None):
        rays = _chk(rays, 'rays', (11,)); or_rays = _chk(or_rays, 'or_rays', (11,))
        img4 = _chk(img4, 'img4', (4,)); proj = _chk(proj, 'proj', (3, 4))
        n = rays.shape[0]
        nb, Hf, Wf, _ = img4.shape
        if proj.shape[0] != nb:
            raise PnrfError(f'render_rays: {nb} packed neighbour images but {proj.shape[0]} projection matrices')
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != rays.device or out.dtype != f32 or tuple(out.shape) != (n, 4) or not out.is_contiguous():
                raise PnrfError(f'render_rays: out must be a contiguous float32 tensor [{n}, 4] on {rays.device}, got '
                                f'{getattr(out, "dtype", type(out))} {tuple(getattr(out, "shape", ()))} on {getattr(out, "device", "?")}')
        rgbd = out if out is not None else torch.empty(n, 4, device=rays.device, dtype=f32)
        idx = torch.empty(n, 8, device=rays.device, dtype=torch.int64) if want_idx else None
        check(_lib.load().pnrf_render_rays_fwd(self.handle, _ptr(rays), _ptr(or_rays), _ptr(img4), _ptr(proj), nb, Hf, Wf, eps,
                                               _ptr(rgbd), _ptr(idx), n, _stream()), 'pnrf_render_rays_fwd')
        return rgbd, idx

    def render_pose(self, scene, c2w, nb, H, W, near=0.0, far=1.0, or_near=1.0, or_far=10.0, first=0, count=None, block=None, stride=0, eps=1e-5,
                    ws=None, out=None, want_idx=False):
        """Pose -> rows of the frame (pnrf_render_pose_fwd): neighbour selection, gather, rays and render_rays on the current stream from the GPU
        tensor c2w [3,4], read in place.  ws: uint8 GPU tensor of ``scene.pose_workspace_bytes(nb, count)`` bytes (None: allocated here)."""
        c2w = _dev_mat(c2w, 'c2w', (3, 4))
        n = H * W - first if count is None else int(count)
        need = scene.pose_workspace_bytes(nb, n)
        if ws is None:
            ws = torch.empty(need, device=c2w.device, dtype=torch.uint8)
        elif not isinstance(ws, torch.Tensor) or ws.device != c2w.device or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
            raise PnrfError(f'render_pose: ws must be a contiguous uint8 tensor of at least {need} bytes on {c2w.device}')
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != c2w.device or out.dtype != f32 or tuple(out.shape) != (n, 4) or not out.is_contiguous():
                raise PnrfError(f'render_pose: out must be a contiguous float32 tensor [{n}, 4] on {c2w.device}')
        rgbd = out if out is not None else torch.empty(n, 4, device=c2w.device, dtype=f32)
        idx = torch.empty(n, 8, device=c2w.device, dtype=torch.int64) if want_idx else None
        check(_lib.load().pnrf_render_pose_fwd(self.handle, scene.handle, _ptr(c2w), int(nb), int(H), int(W), near, far, or_near, or_far, int(first),
                                               int(max(n, 1) if block is None else block), int(0 if block is None else stride), n, eps, _ptr(ws), ws.numel(),
                                               _ptr(rgbd), _ptr(idx), _stream()), 'pnrf_render_pose_fwd')
        return rgbd, idx


class Scene:
    """pnrf_scene: the source views of a scene on the device — texel cache [nv,Hf,Wf,4], poses, intrinsics — uploaded once; ``select`` and
    ``RenderContext.render_pose`` derive everything a target pose needs from it on the device.

    cache: 'f32' (float4 texels, exact for any image) or 'u8' (RGBA8 texels, a quarter of the memory; uint8 images only)."""

    FORMATS = {'f32': 0, 'u8': 1}

    def __init__(self, nv, Hf, Wf, cache='f32', device='cuda:0'):
        if cache not in self.FORMATS:
            raise PnrfError(f"Scene: cache must be 'f32' or 'u8', got {cache!r}")
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise PnrfError('Scene needs a GPU device (pronerf_amd has no CPU path)')
        h = C.c_void_p()
        check(_lib.load().pnrf_scene_create(int(nv), int(Hf), int(Wf), self.FORMATS[cache], C.byref(h)), 'pnrf_scene_create')
        self.handle = h
        self.nv, self.Hf, self.Wf, self.cache = int(nv), int(Hf), int(Wf), cache
        self.K = None                                      # device copy of the target intrinsics (what frame_rays_dev takes)

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().pnrf_scene_free(self.handle)
                self.handle = None
        except Exception:
            pass

    def set_view(self, v, image, pose):
        """image: [Hf,Wf,3|4] float32 or uint8, numpy or torch (host data is copied to the device first; a GPU tensor is read in place);
        pose: host [3,4] camera-to-world."""
        img = torch.as_tensor(image)
        if img.dtype not in (torch.float32, torch.uint8):
            if img.dtype.is_floating_point:
                img = img.to(torch.float32)
            else:
                raise PnrfError(f'Scene.set_view: images must be float32 or uint8, got {img.dtype}')
        if img.dim() != 3 or tuple(img.shape[:2]) != (self.Hf, self.Wf) or img.shape[2] not in (3, 4):
            raise PnrfError(f'Scene.set_view: expected an image [{self.Hf}, {self.Wf}, 3|4], got {tuple(img.shape)}')
        img = img.to(self.device).contiguous()
        ph = np.ascontiguousarray(np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float32)[:3, :4])
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_scene_set_view(self.handle, int(v), _ptr(img), 1 if img.dtype == torch.uint8 else 0, int(img.shape[2]),
                                                  ph.ctypes.data_as(C.POINTER(C.c_float)), _stream()), 'pnrf_scene_set_view')
            img.record_stream(torch.cuda.current_stream())
        return self

    def set_intrinsics(self, K, ref_K=None):
        fp = C.POINTER(C.c_float)
        host = lambda m: np.ascontiguousarray(np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float32).reshape(3, 3))
        Kh = host(K)
        Rh = Kh if ref_K is None else host(ref_K)
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_scene_set_intrinsics(self.handle, Kh.ctypes.data_as(fp), Rh.ctypes.data_as(fp)), 'pnrf_scene_set_intrinsics')
        self.K = torch.from_numpy(Kh).to(self.device)
        return self

    @classmethod
    def from_views(cls, poses, images, K, ref_K=None, cache='f32', device='cuda:0'):
        """poses [nv,3,4]; images [nv,Hf,Wf,3] numpy or torch, float32 or uint8 (one view at a time travels to the device); K, ref_K: the driver's
        target / source intrinsics (ref_K None: K)."""
        nv, Hf, Wf = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
        if len(poses) != nv:
            raise PnrfError(f'Scene.from_views: {nv} images but {len(poses)} poses')
        self = cls(nv, Hf, Wf, cache=cache, device=device)
        self.set_intrinsics(K, ref_K)
        for v in range(nv):
            self.set_view(v, images[v], poses[v])
        return self

    def select(self, c2w, nb):
        """Neighbours of the target pose c2w (GPU tensor [3,4], read in place) -> (ref_nos int32 [nb], proj [nb,3,4], img4 [nb,Hf,Wf,4])
        (pnrf_scene_select_fwd)."""
        c2w = _dev_mat(c2w, 'c2w', (3, 4))
        nb = int(nb)
        with torch.cuda.device(self.device):
            ref = torch.empty(max(nb, 0), device=self.device, dtype=torch.int32)
            proj = torch.empty(max(nb, 0), 3, 4, device=self.device, dtype=f32)
            img4 = torch.empty(max(nb, 0), self.Hf, self.Wf, 4, device=self.device, dtype=f32)
            check(_lib.load().pnrf_scene_select_fwd(self.handle, _ptr(c2w), nb, _ptr(ref), _ptr(proj), _ptr(img4), _stream()), 'pnrf_scene_select_fwd')
        return ref, proj, img4

    def pose_workspace_bytes(self, nb, max_rays):
        v = C.c_int64()
        check(_lib.load().pnrf_render_pose_workspace_bytes(self.handle, int(nb), int(max_rays), C.byref(v)), 'pnrf_render_pose_workspace_bytes')
        return int(v.value)

    def arrays(self):
        """Zero-copy views (img4 [nv,Hf,Wf,4], poses [nv,3,4], K_target [3,3], K_ref [3,3]) of a complete 'f32' scene's device arrays
        (pnrf_scene_arrays): img4 is bit for bit ``images_pack`` of the views, i.e. what ``Trainer.fwd_bwd`` takes."""
        ptrs = [C.c_void_p() for _ in range(4)]
        check(_lib.load().pnrf_scene_arrays(self.handle, *[C.byref(p) for p in ptrs]), 'pnrf_scene_arrays')
        shapes = [(self.nv, self.Hf, self.Wf, 4), (self.nv, 3, 4), (3, 3), (3, 3)]
        return tuple(_dev_view(int(p.value), sh, '<f4', self.device, self) for p, sh in zip(ptrs, shapes))

    def rank_table(self):
        """int32 [nv,nv]: row c = the views in stable ascending order of their distance to view c (pnrf_scene_rank_table_fwd) — the stage-2
        driver's ``neighbor_rank_table`` index for index."""
        with torch.cuda.device(self.device):
            rank = torch.empty(self.nv, self.nv, device=self.device, dtype=torch.int32)
            check(_lib.load().pnrf_scene_rank_table_fwd(self.handle, _ptr(rank), _stream()), 'pnrf_scene_rank_table_fwd')
        return rank


def _dev_view(ptr, shape, typestr, device, owner):
    """torch tensor over device memory the library owns (``__cuda_array_interface__`` v3: no copy); ``owner`` stays alive as long as the view."""
    class _Dev:
        __cuda_array_interface__ = {'shape': tuple(int(x) for x in shape), 'typestr': typestr, 'data': (int(ptr), False), 'version': 3}
    with torch.cuda.device(device):
        t = torch.as_tensor(_Dev(), device=device)
    t._pnrf_owner = owner
    return t


class TrainSet:
    """The training set of a driver on the device: a complete 'f32' ``Scene`` of the training views, its rank table and persistent output buffers
    for one batch of at most ``max_rays`` rays (``max_cols`` jitter / noise columns), so that the pointers the trainer sees are the same in every
    iteration.  ``batch`` turns ray indices (ray g = view g // (Hf Wf), pixel g % (Hf Wf)) into the positional head of ``Trainer.fwd_bwd`` /
    ``Trainer.explore_fwd_bwd`` with at most two launches (pnrf_train_batch_fwd); nothing per-pixel is ever expanded for the whole set."""

    def __init__(self, scene, max_rays, near, far, or_near=1.0, or_far=10.0, max_cols=8):
        if not isinstance(scene, Scene):
            raise PnrfError('TrainSet: expected an ops.Scene')
        max_rays, max_cols = int(max_rays), int(max_cols)
        if max_rays < 1 or max_cols < 4 or max_cols % 4 or max_cols > 256:
            raise PnrfError(f'TrainSet: max_rays >= 1 and max_cols a multiple of 4 in 4 .. 256, got {max_rays}, {max_cols}')
        self.scene, self.device = scene, scene.device
        self.max_rays, self.max_cols = max_rays, max_cols
        self.near, self.far, self.or_near, self.or_far = float(near), float(far), float(or_near), float(or_far)
        self.img4, self.poses, self.K_target, self.K = scene.arrays()          # K: the source cameras' intrinsics (ref_K), the one the trainer projects with
        self.device = self.img4.device                                           # with its index, as every tensor's device has it
        self.rank = scene.rank_table()
        with torch.cuda.device(self.device):
            new = lambda *sh, dt=f32: torch.empty(*sh, device=self.device, dtype=dt)
            self._rays, self._or_rays, self._target = new(max_rays, 11), new(max_rays, 11), new(max_rays, 3)
            self._ref_nos = new(max_rays, 4, dt=torch.int64)
            self._jitter, self._noise = new(max_rays * max_cols), new(max_rays * max_cols)
            self._bad = torch.zeros(1, device=self.device, dtype=torch.int64)

    def batch(self, idx, order, step=None, seed=0, row0=0, jitter_cols=0, jitter_cap=1 - 2e-6, noise_cols=0, noise_std=0.):
        """idx: int64 GPU tensor [n], n <= max_rays; order: four Python ints in 0 .. nv - 2 (rank positions after dropping the view itself).
        -> (rays, or_rays, target, img4, poses, K, ref_nos) [+ jitter [n,jitter_cols]] [+ noise [n,noise_cols]]: views of the persistent buffers,
        valid until the next call.  Draws (jitter_cols / noise_cols > 0) need ``step``; they are a function of (seed, step, row0 + row) alone."""
        if not isinstance(idx, torch.Tensor) or idx.device != self.device or idx.dtype != torch.int64 or idx.dim() != 1:
            raise PnrfError(f'TrainSet.batch: idx must be a 1-D int64 tensor on {self.device}')
        idx = idx.contiguous()
        n = idx.shape[0]
        if n > self.max_rays:
            raise PnrfError(f'TrainSet.batch: {n} rays, the set was sized for {self.max_rays}')
        cj, cn = int(jitter_cols), int(noise_cols)
        if max(cj, cn) > self.max_cols or min(cj, cn) < 0:
            raise PnrfError(f'TrainSet.batch: jitter_cols / noise_cols must be 0 .. max_cols = {self.max_cols}, got {cj}, {cn}')
        if (cj or cn) and step is None:
            raise PnrfError('TrainSet.batch: draws need a step')
        order = [int(o) for o in order]
        if len(order) != 4:
            raise PnrfError(f'TrainSet.batch: order must hold 4 rank positions, got {len(order)}')
        jit = self._jitter[:n * cj].view(n, cj) if cj else None
        noi = self._noise[:n * cn].view(n, cn) if cn else None
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_train_batch_fwd(self.scene.handle, _ptr(self.rank), _ptr(idx), n, (C.c_int * 4)(*order), self.near, self.far, self.or_near,
                                                   self.or_far, _ptr(self._rays), _ptr(self._or_rays), _ptr(self._target), _ptr(self._ref_nos),
                                                   _ptr(self._bad), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step or 0) & 0xFFFFFFFF, int(row0), _ptr(jit), cj,
                                                   float(jitter_cap), _ptr(noi), cn, float(noise_std), _stream()), 'pnrf_train_batch_fwd')
            idx.record_stream(torch.cuda.current_stream())
        out = (self._rays[:n], self._or_rays[:n], self._target[:n], self.img4, self.poses, self.K, self._ref_nos[:n])
        return out + ((jit,) if cj else ()) + ((noi,) if cn else ())

    def bad_rows(self):
        """Rows whose index lay outside the set since construction (they got NaN rays and targets).  Synchronises: tests and debugging."""
        return int(self._bad.item())


def linspace(start, end, n):
    out = (C.c_float * n)()
    check(_lib.load().pnrf_linspace(start, end, n, out), 'pnrf_linspace')
    return np.array(out[:], dtype=np.float32)


# ------------------------------------------------------------------------------------------ frame tail: image metrics, 8-bit output
def ssim_filter(filter_size=11, filter_sigma=1.5):
    """The 1-D Gaussian of img2ssim in float64 (helpers:163-167): ``filter_size`` taps spaced 1 apart and centred on 0 — an even size sits
    half a tap off the pixel grid —, exp(-x^2 / (2 sigma^2)), normalised to sum 1.  The kernel takes it rounded to fp32."""
    half = int(filter_size) // 2
    offset = (2 * half - int(filter_size) + 1) / 2            # 0 for an odd size, 0.5 for an even one
    x = (np.arange(int(filter_size)) - half + offset) / filter_sigma
    g = np.exp(-0.5 * x ** 2)
    return g / g.sum()


def _pixels(t, name, width):
    """A tensor whose last dimension holds ``width`` contiguous floats per pixel (width 0: the tensor's elements are the pixels) and whose
    pixels lie a constant number of floats apart — [H,W,3], [n,3], or such a view into rgbd[n,4] — as (tensor, pixel stride, pixel count)
    without a copy; any other layout is made contiguous."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PnrfError(f'{name}: expected a GPU tensor (pronerf_amd has no CPU path)')
    if t.dtype != f32:
        raise PnrfError(f'{name}: expected float32, got {t.dtype}')
    if width and (t.dim() < 2 or t.shape[-1] != width):
        raise PnrfError(f'{name}: expected trailing shape ({width},), got {tuple(t.shape)}')
    lead = t.shape[:-1] if width else t.shape
    strides = t.stride()[:-1] if width else t.stride()
    n = int(np.prod(lead, dtype=np.int64))
    ok = (not width or t.stride(-1) == 1) and len(lead) >= 1 and strides[-1] >= max(width, 1)
    for d in range(len(lead) - 1):
        ok = ok and (lead[d] == 1 or strides[d] == strides[d + 1] * lead[d + 1])
    if ok:
        return t, int(strides[-1]), n
    return t.contiguous(), max(width, 1), n


def image_metrics(pred, gt, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """img2mse and img2ssim of two [H,W,3] images in one call (pnrf_image_metrics_fwd; helpers:129, 151-197).  ``pred`` / ``gt`` may be
    views with a pixel stride above 3, e.g. ``rgbd[:, :3].reshape(H, W, 3)`` of the renderer's [n,4] rows.  Returns a float64 device tensor
    [4] = (sum of squared differences, mse, sum of the SSIM map, mean SSIM) — nothing is read back — and, with ``return_map``, also the
    [H-T+1, W-T+1, 3] SSIM map."""
    lib = _lib.load()
    if pred.dim() != 3 or pred.shape[-1] != 3 or pred.shape != gt.shape:
        raise PnrfError(f'image_metrics: expected two [H,W,3] images of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}')
    H, W = int(pred.shape[0]), int(pred.shape[1])
    T = int(filter_size)
    if not 1 <= T <= 16 or H < T or W < T:
        raise PnrfError(f'image_metrics: filter_size {T} must be 1 .. 16 and fit the {H} x {W} image')
    pred, sp, _ = _pixels(pred, 'pred', 3)
    gt, sg, _ = _pixels(gt, 'gt', 3)
    if gt.device != pred.device:
        raise PnrfError('image_metrics: pred and gt are on different devices')
    taps = np.ascontiguousarray(ssim_filter(T, filter_sigma), dtype=np.float32)
    with torch.cuda.device(pred.device):
        nb = int(lib.pnrf_image_metrics_workspace_bytes(H, W, T))
        ws = torch.empty(nb // 8, device=pred.device, dtype=torch.float64)
        out = torch.empty(4, device=pred.device, dtype=torch.float64)
        smap = torch.empty(H - T + 1, W - T + 1, 3, device=pred.device, dtype=f32) if return_map else None
        check(lib.pnrf_image_metrics_fwd(_ptr(pred), sp, _ptr(gt), sg, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), T, float(max_val), float(k1),
                                         float(k2), _ptr(out), _ptr(smap), _ptr(ws), nb, _stream()), 'pnrf_image_metrics_fwd')
    return (out, smap) if return_map else out


def _patches(t, name):
    """[B,H,W,3] patches whose pixels hold 3 contiguous floats, lie a constant number of floats apart inside a patch (rows without gaps) and
    whose patches lie any number of floats apart, as (tensor, pixel stride, patch stride) without a copy; any other layout is made contiguous."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PnrfError(f'{name}: expected a GPU tensor (pronerf_amd has no CPU path)')
    if t.dtype != f32:
        raise PnrfError(f'{name}: expected float32, got {t.dtype}')
    B, H, W, _ = t.shape
    sb, sy, sx, sc = t.stride()
    if sc == 1 and sx >= 3 and (H == 1 or sy == W * sx) and (B == 1 or sb >= 0):
        return t, int(sx), int(sb) if B > 1 else 0
    return t.contiguous(), 3, H * W * 3


_ssim_workspaces = {}      # (device index, stream, B, H, W, T) -> workspace: calls on one stream follow each other, so they may share one


def ssim_loss(pred, gt, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """The mean SSIM of B patch pairs and its gradient with respect to ``pred`` (pnrf_ssim_loss_fwd; the arithmetic of ``image_metrics``).
    ``pred`` / ``gt``: [B,H,W,3] or [H,W,3]; views with a pixel stride above 3 and any patch stride are read in place.  Returns (mean SSIM as a
    0-d float64 device tensor, d mean / d pred as a float32 tensor shaped like ``pred``) — nothing is read back.  The loss 1 - mean and its
    weight are the caller's (``autograd.ssim`` makes it differentiable)."""
    lib = _lib.load()
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3 or pred.shape != gt.shape:
        raise PnrfError(f'ssim_loss: expected two [B,H,W,3] or [H,W,3] tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}')
    shape = tuple(pred.shape)
    B, H, W = (1,) * (pred.dim() == 3) + tuple(int(x) for x in shape[:-1])
    T = int(filter_size)
    if not 1 <= T <= 16 or H < T or W < T:
        raise PnrfError(f'ssim_loss: filter_size {T} must be 1 .. 16 and fit the {H} x {W} patches')
    if not 1 <= B <= 21845:
        raise PnrfError(f'ssim_loss: {B} patches, one call takes 1 .. 21845')
    pred, sp, pp = _patches(pred.reshape(B, H, W, 3) if pred.dim() == 3 else pred, 'pred')
    gt, sg, pg = _patches(gt.reshape(B, H, W, 3) if gt.dim() == 3 else gt, 'gt')
    if gt.device != pred.device:
        raise PnrfError('ssim_loss: pred and gt are on different devices')
    taps = np.ascontiguousarray(ssim_filter(T, filter_sigma), dtype=np.float32)
    with torch.cuda.device(pred.device):
        nb = int(lib.pnrf_ssim_loss_workspace_bytes(B, H, W, T))
        key = (pred.device.index, torch.cuda.current_stream().cuda_stream, B, H, W, T)
        ws = _ssim_workspaces.get(key)
        if ws is None:
            if len(_ssim_workspaces) >= 64:
                _ssim_workspaces.clear()
            ws = _ssim_workspaces[key] = torch.empty((nb + 7) // 8, device=pred.device, dtype=torch.float64)
        out = torch.empty(2, device=pred.device, dtype=torch.float64)
        d_pred = torch.empty(shape, device=pred.device, dtype=f32)
        check(lib.pnrf_ssim_loss_fwd(_ptr(pred), sp, pp, _ptr(gt), sg, pg, B, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), T, float(max_val),
                                     float(k1), float(k2), _ptr(out), _ptr(d_pred), _ptr(ws), nb, _stream()), 'pnrf_ssim_loss_fwd')
    return out[1], d_pred


# ------------------------------------------------------------------------------------------ LPIPS
# torch shapes [out, in, kh, kw] of the backbones' conv layers and the channels of the five 'lin' layers (include/pronerf_hip.h)
LPIPS_CONVS = {'alex': [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)],
               'vgg': [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3),
                       (512, 256, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3)]}
LPIPS_LIN = {'alex': (64, 192, 384, 256, 256), 'vgg': (64, 128, 256, 512, 512)}
LPIPS_MIN = {'alex': 31, 'vgg': 16}
LPIPS_MAX_DIM = 4096


def _lpips_state(sd, what):
    """A state dict, or the path of one (loaded on the CPU, tensors only)."""
    if isinstance(sd, (str, bytes)) or hasattr(sd, '__fspath__'):
        sd = torch.load(sd, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict):
        raise PnrfError(f'Lpips: {what} must be a state dict or the path of one, got {type(sd).__name__}')
    return sd


def lpips_weights(net, backbone, lin):
    """(conv weights, conv biases, lin vectors) as contiguous fp32 CPU tensors from a backbone state dict — the 4-D ``….<idx>.weight`` / ``.bias``
    entries in index order: torchvision's ``features.<idx>.*`` or the lpips package's ``net.slice<k>.<idx>.*`` — and a lin state dict — entries
    named ``lin<k>…weight``, k = 0 .. 4 in order, [1,C,1,1] or [C].  Anything else raises a PnrfError that names the key and the expected shape."""
    import re
    if net not in LPIPS_CONVS:
        raise PnrfError(f"Lpips: unknown net {net!r}; the kernels take 'alex' and 'vgg'")
    backbone, lin = _lpips_state(backbone, 'backbone'), _lpips_state(lin, 'lin')
    is_lin = re.compile(r'(^|\.)lin(\d+)(\.|$)')
    any_lin = re.compile(r'(^|\.)lins?\d*(\.|$)')                 # lin<k>.* and the lpips module's lins.<k>.* list: 4-D, but no conv layers of the backbone
    found = []
    for k, v in backbone.items():
        m = re.search(r'(^|\.)(\d+)\.weight$', k)
        if m and isinstance(v, torch.Tensor) and v.dim() == 4 and not any_lin.search(k):
            found.append((int(m.group(2)), k))
    found.sort()
    shapes = LPIPS_CONVS[net]
    if len(found) != len(shapes):
        raise PnrfError(f"Lpips: backbone of {net!r} needs {len(shapes)} conv layers ('<idx>.weight' of shapes {shapes}), found {len(found)}: "
                        f'{[k for _, k in found]}')
    W, B = [], []
    for (_, k), shp in zip(found, shapes):
        if tuple(backbone[k].shape) != shp:
            raise PnrfError(f'Lpips: {k} has shape {tuple(backbone[k].shape)}, expected {shp}')
        kb = k[:-len('weight')] + 'bias'
        if kb not in backbone or tuple(backbone[kb].shape) != (shp[0],):
            raise PnrfError(f'Lpips: {kb} is missing or not of shape {(shp[0],)}')
        W.append(backbone[k].detach().to('cpu', f32).contiguous())
        B.append(backbone[kb].detach().to('cpu', f32).contiguous())
    lins = sorted((int(is_lin.search(k).group(2)), k) for k in lin if is_lin.search(k) and k.endswith('weight'))
    if [i for i, _ in lins] != [0, 1, 2, 3, 4]:
        raise PnrfError(f"Lpips: lin needs the five entries 'lin0…weight' .. 'lin4…weight' of {LPIPS_LIN[net]} channels, found {[k for _, k in lins]}")
    L = []
    for (i, k), c in zip(lins, LPIPS_LIN[net]):
        if tuple(lin[k].shape) not in ((1, c, 1, 1), (c,)):
            raise PnrfError(f'Lpips: {k} has shape {tuple(lin[k].shape)}, expected {(1, c, 1, 1)} or {(c,)}')
        L.append(lin[k].detach().to('cpu', f32).reshape(c).contiguous())
    return W, B, L


def lpips_tap_dims(net, H, W):
    """[(rows, columns)] of the five tap planes of an H x W image (pnrf_lpips_tap_dims; host only)."""
    hw = (C.c_int * 10)()
    check(_lib.load().pnrf_lpips_tap_dims(str(net).encode(), int(H), int(W), hw), 'pnrf_lpips_tap_dims')
    return [(hw[2 * k], hw[2 * k + 1]) for k in range(5)]


_lpips_workspaces = {}     # (handle, device index, stream, H, W) -> workspace: calls on one stream follow each other, so they may share one


class Lpips:
    """LPIPS 0.1 of image pairs on the device (pnrf_lpips_fwd): ``Lpips(net, backbone, lin)`` with net 'alex' | 'vgg', ``backbone`` the
    torchvision state dict of the net (or the lpips package's, keys ``net.slice*``) and ``lin`` the lpips package's ``lin`` state dict — each a dict
    or a path (``lpips_weights``).  The weights are the caller's; nothing is fetched from anywhere."""

    def __init__(self, net, backbone, lin, device=None):
        W, B, L = lpips_weights(net, backbone, lin)
        lib = _lib.load()
        self.net, self.device = net, torch.device('cuda' if device is None else device)
        n = len(W)
        shapes = (C.c_int * (4 * n))(*[d for w in W for d in w.shape])
        dims = (C.c_int * 5)(*[int(l.numel()) for l in L])
        pw, pb, pl = ((C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) for ts in (W, B, L))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.pnrf_lpips_create(net.encode(), pw, pb, shapes, n, pl, dims, C.byref(h)), 'pnrf_lpips_create')
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:                                                    # (at interpreter exit the module's globals may be gone already)
                for k in [k for k in _lpips_workspaces if k[0] == h.value]:
                    del _lpips_workspaces[k]
                _lib.load().pnrf_lpips_free(h)
            except Exception:
                pass

    def _workspace(self, dev, nb, H, W):
        key = (self._h.value, dev.index, torch.cuda.current_stream().cuda_stream, H, W)
        ws = _lpips_workspaces.get(key)
        if ws is None or ws.numel() * 8 < nb:
            if len(_lpips_workspaces) >= 16:
                _lpips_workspaces.clear()
            ws = _lpips_workspaces[key] = torch.empty((nb + 7) // 8, device=dev, dtype=torch.float64)
        return ws

    def __call__(self, a, b, normalize=True, return_layers=False, return_maps=False):
        """d(a, b) of two [H,W,3] fp32 GPU images — or views with a pixel stride above 3, e.g. ``rgbd[:, :3].reshape(H, W, 3)`` — as a 0-d float64
        device tensor; nothing is read back.  ``return_layers``: also the five per-tap means [5]; ``return_maps``: also the five m_k planes."""
        lib = _lib.load()
        if a.dim() != 3 or a.shape[-1] != 3 or a.shape != b.shape:
            raise PnrfError(f'Lpips: expected two [H,W,3] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
        H, W = int(a.shape[0]), int(a.shape[1])
        lo = LPIPS_MIN[self.net]
        if not (lo <= H <= LPIPS_MAX_DIM and lo <= W <= LPIPS_MAX_DIM):
            raise PnrfError(f'Lpips: {self.net!r} takes images of {lo} .. {LPIPS_MAX_DIM} pixels per side, got {H} x {W}')
        a, sa, _ = _pixels(a, 'a', 3)
        b, sb, _ = _pixels(b, 'b', 3)
        if a.device != b.device:
            raise PnrfError('Lpips: a and b are on different devices')
        with torch.cuda.device(a.device):
            nb = int(lib.pnrf_lpips_workspace_bytes(self._h, H, W))
            ws = self._workspace(a.device, nb, H, W)
            out = torch.empty(6, device=a.device, dtype=torch.float64)
            maps, dims = None, None
            if return_maps:
                dims = lpips_tap_dims(self.net, H, W)
                maps = torch.empty(sum(h * w for h, w in dims), device=a.device, dtype=f32)
            check(lib.pnrf_lpips_fwd(self._h, _ptr(a), sa, _ptr(b), sb, H, W, int(bool(normalize)), _ptr(out), _ptr(maps), _ptr(ws), nb, _stream()),
                  'pnrf_lpips_fwd')
        res = [out[0]]
        if return_layers:
            res.append(out[1:])
        if return_maps:
            offs = np.cumsum([0] + [h * w for h, w in dims])
            res.append([maps[offs[k]:offs[k + 1]].view(*dims[k]) for k in range(5)])
        return res[0] if len(res) == 1 else tuple(res)

    def layer(self, layer, x, pool_first=False):
        """Conv layer ``layer`` of the net (with ``pool_first`` its preceding max pooling first), bias and ReLU on a dense NHWC pair
        x [2,H,W,C_in] -> [2,OH,OW,C_out] (pnrf_lpips_layer_fwd: the kernels of the metric, for tests)."""
        lib = _lib.load()
        shapes = LPIPS_CONVS[self.net]
        if not 0 <= layer < len(shapes):
            raise PnrfError(f'Lpips.layer: layer {layer} outside 0 .. {len(shapes) - 1}')
        co, ci, k, _ = shapes[layer]
        x = _chk(x, 'x', (ci,))
        if x.dim() != 4 or x.shape[0] != 2:
            raise PnrfError(f'Lpips.layer: expected x of shape [2,H,W,{ci}], got {tuple(x.shape)}')
        H, W = int(x.shape[1]), int(x.shape[2])
        stride, pad = (4, 2) if k == 11 else (1, k // 2)
        window = {('alex', 1): 3, ('alex', 2): 3}.get((self.net, layer), 2)
        h, w = ((H - window) // 2 + 1, (W - window) // 2 + 1) if pool_first else (H, W)
        oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        with torch.cuda.device(x.device):
            nb = int(lib.pnrf_lpips_layer_workspace_bytes(self._h, layer, int(pool_first), H, W))
            ws = torch.empty(max(nb, 8) // 4, device=x.device, dtype=f32)
            y = torch.empty(2, max(oh, 0), max(ow, 0), co, device=x.device, dtype=f32)
            check(lib.pnrf_lpips_layer_fwd(self._h, layer, int(pool_first), _ptr(x), H, W, _ptr(y), _ptr(ws), nb, _stream()), 'pnrf_lpips_layer_fwd')
        return y

    def loss(self, pred, gt, normalize=True, return_layers=False):
        """The mean d(pred_i, gt_i) of B patch pairs and its gradient with respect to ``pred`` (pnrf_lpips_loss_fwd).  ``pred`` / ``gt``:
        [B,H,W,3] or [H,W,3] fp32 GPU tensors; views with a pixel stride above 3 and any patch stride are read in place.  Returns (mean d as a
        0-d float64 device tensor, d mean / d pred as a float32 tensor shaped like ``pred``) — nothing is read back; ``return_layers``: also
        the five tap means [5].  The weight and the sign are the caller's (``autograd.lpips`` makes it differentiable)."""
        lib = _lib.load()
        if pred.dim() not in (3, 4) or pred.shape[-1] != 3 or pred.shape != gt.shape:
            raise PnrfError(f'Lpips.loss: expected two [B,H,W,3] or [H,W,3] tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}')
        shape = tuple(pred.shape)
        B, H, W = (1,) * (pred.dim() == 3) + tuple(int(x) for x in shape[:-1])
        lo = LPIPS_MIN[self.net]
        if not (lo <= H <= LPIPS_MAX_DIM and lo <= W <= LPIPS_MAX_DIM) or B < 1 or 2 * B * H * W > 2 ** 31 - 1:
            raise PnrfError(f'Lpips.loss: {self.net!r} takes B >= 1 patches of {lo} .. {LPIPS_MAX_DIM} pixels per side with 2 B H W < 2^31, got {B} of {H} x {W}')
        pred, sp, pp = _patches(pred.reshape(B, H, W, 3) if pred.dim() == 3 else pred, 'pred')
        gt, sg, pg = _patches(gt.reshape(B, H, W, 3) if gt.dim() == 3 else gt, 'gt')
        if gt.device != pred.device:
            raise PnrfError('Lpips.loss: pred and gt are on different devices')
        with torch.cuda.device(pred.device):
            nb = int(lib.pnrf_lpips_loss_workspace_bytes(self._h, B, H, W))
            if nb <= 0:
                check(-1, 'pnrf_lpips_loss_workspace_bytes')
            ws = self._workspace(pred.device, nb, ('loss', B, H), W)
            out = torch.empty(6, device=pred.device, dtype=torch.float64)
            d_pred = torch.empty(shape, device=pred.device, dtype=f32)
            check(lib.pnrf_lpips_loss_fwd(self._h, _ptr(pred), sp, pp, _ptr(gt), sg, pg, B, H, W, int(bool(normalize)), _ptr(out), _ptr(d_pred), _ptr(ws), nb,
                                          _stream()), 'pnrf_lpips_loss_fwd')
        return (out[0], d_pred, out[1:]) if return_layers else (out[0], d_pred)

    def _geometry(self, layer, H, W, pool_first):
        co, ci, k, _ = LPIPS_CONVS[self.net][layer]
        stride, pad = (4, 2) if k == 11 else (1, k // 2)
        window = {('alex', 1): 3, ('alex', 2): 3}.get((self.net, layer), 2)
        h, w = ((H - window) // 2 + 1, (W - window) // 2 + 1) if pool_first else (H, W)
        return co, ci, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def layer_bwd(self, layer, x, y, dy, pool_first=False, relu_in=False):
        """The backward of ``layer`` (``Lpips.layer``'s arguments) on n images: x [n,H,W,C_in] the saved input, y [n,OH,OW,C_out] the saved output,
        dy its gradient -> dx [n,H,W,C_in] (pnrf_lpips_layer_bwd: the kernels of the loss, for tests).  ``relu_in``: dx is also multiplied by
        [x > 0], in the kernel that writes it."""
        lib = _lib.load()
        shapes = LPIPS_CONVS[self.net]
        if not 0 <= layer < len(shapes):
            raise PnrfError(f'Lpips.layer_bwd: layer {layer} outside 0 .. {len(shapes) - 1}')
        x = _chk(x, 'x', (shapes[layer][1],))
        if x.dim() != 4:
            raise PnrfError(f'Lpips.layer_bwd: expected x of shape [n,H,W,{shapes[layer][1]}], got {tuple(x.shape)}')
        n, H, W = (int(v) for v in x.shape[:3])
        co, ci, oh, ow = self._geometry(layer, H, W, pool_first)
        y, dy = _chk(y, 'y', (co,)), _chk(dy, 'dy', (co,))
        if tuple(y.shape) != (n, oh, ow, co) or y.shape != dy.shape:
            raise PnrfError(f'Lpips.layer_bwd: expected y and dy of shape {(n, oh, ow, co)}, got {tuple(y.shape)} and {tuple(dy.shape)}')
        with torch.cuda.device(x.device):
            nb = int(lib.pnrf_lpips_layer_bwd_workspace_bytes(self._h, layer, int(pool_first), n, H, W))
            ws = torch.empty(max(nb, 16) // 4, device=x.device, dtype=f32)
            dx = torch.empty_like(x)
            check(lib.pnrf_lpips_layer_bwd(self._h, layer, int(pool_first), int(relu_in), n, _ptr(x), H, W, _ptr(y), _ptr(dy), _ptr(dx), _ptr(ws), nb,
                                           _stream()), 'pnrf_lpips_layer_bwd')
        return dx

    def tap_bwd(self, tap, f_pred, f_gt):
        """dF [F > 0] of tap ``tap`` for features f_pred, f_gt [..., C_tap] of any number of tap pixels P (omega = 1 / P) (pnrf_lpips_tap_bwd: the
        loss's kernel, for tests)."""
        lib = _lib.load()
        c = LPIPS_LIN[self.net][tap]
        f_pred, f_gt = _chk(f_pred, 'f_pred', (c,)), _chk(f_gt, 'f_gt', (c,))
        if f_pred.shape != f_gt.shape:
            raise PnrfError(f'Lpips.tap_bwd: f_pred {tuple(f_pred.shape)} and f_gt {tuple(f_gt.shape)} differ')
        with torch.cuda.device(f_pred.device):
            d = torch.empty_like(f_pred)
            check(lib.pnrf_lpips_tap_bwd(self._h, int(tap), _ptr(f_pred), _ptr(f_gt), f_pred.numel() // c, _ptr(d), _stream()), 'pnrf_lpips_tap_bwd')
        return d


def patch_indices(nv, H, W, patch, count, generator=None, device=None):
    """Ray indices [count patch^2] (int64, on the device) of ``count`` ``patch`` x ``patch`` crops placed uniformly over the views and the
    positions at which a crop lies inside its view: patch-major, row-major inside a patch, in ``TrainSet``'s numbering
    g = view H W + y W + x.  Drawn by torch on the device (``generator``'s, else ``device``, else the current one): no host sync."""
    nv, H, W, patch, count = int(nv), int(H), int(W), int(patch), int(count)
    if nv < 1 or count < 1 or not 1 <= patch <= min(H, W):
        raise PnrfError(f'patch_indices: need nv >= 1, count >= 1 and 1 <= patch <= min(H, W), got nv {nv}, count {count}, patch {patch} in {H} x {W}')
    dev = generator.device if generator is not None else torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    ny, nx = H - patch + 1, W - patch + 1
    place = torch.randint(nv * ny * nx, (count,), device=dev, generator=generator)          # one draw: view, row and column of the crop's corner
    v, rest = place // (ny * nx), place % (ny * nx)
    corner = v * (H * W) + (rest // nx) * W + rest % nx
    k = torch.arange(patch, device=dev)
    return (corner[:, None] + (k[:, None] * W + k[None, :]).reshape(1, -1)).reshape(-1)


def frame_to8b(rgb=None, depth=None, rgbd=None):
    """to8b(rgb) and to8b(depth / max(depth)) as uint8 device tensors (pnrf_frame_to8b_fwd; helpers:135, trt.py:356-360), bit-identical to
    numpy for finite input (NaN -> 0).  ``rgbd`` [n,4] (the renderer's rows), or ``rgb`` [..., 3] and / or ``depth`` [...] — views into
    rgbd are taken as they are.  Returns (rgb8 shaped like rgb, depth8 shaped like depth); an input that is None gives None."""
    lib = _lib.load()
    if rgbd is not None:
        if rgb is not None or depth is not None or rgbd.dim() != 2 or rgbd.shape[-1] != 4:
            raise PnrfError('frame_to8b: rgbd must be [n,4] and excludes rgb / depth')
        rgb, depth = rgbd[:, :3], rgbd[:, 3]
    if rgb is None and depth is None:
        raise PnrfError('frame_to8b: nothing to convert')
    n = None
    if rgb is not None:
        shape_rgb = tuple(rgb.shape)
        rgb, sr, n = _pixels(rgb, 'rgb', 3)
    if depth is not None:
        shape_d = tuple(depth.shape)
        depth, sd, nd = _pixels(depth, 'depth', 0)
        if n is not None and nd != n:
            raise PnrfError(f'frame_to8b: {n} rgb pixels but {nd} depths')
        n = nd
    dev = (rgb if rgb is not None else depth).device
    with torch.cuda.device(dev):
        rgb8 = torch.empty(shape_rgb, device=dev, dtype=torch.uint8) if rgb is not None else None
        depth8 = torch.empty(shape_d, device=dev, dtype=torch.uint8) if depth is not None else None
        ws = torch.empty(1024, device=dev, dtype=f32) if depth is not None else None
        check(lib.pnrf_frame_to8b_fwd(_ptr(rgb), sr if rgb is not None else 0, _ptr(depth), sd if depth is not None else 0, n, _ptr(rgb8), _ptr(depth8),
                                      _ptr(ws), 4096 if ws is not None else 0, _stream()), 'pnrf_frame_to8b_fwd')
    return rgb8, depth8


# ------------------------------------------------------------------------------------------ PNG files of an 8-bit plane
PNG_FILTERS = {'adaptive': -1, 'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4}


def _png_filter(filter):
    f = PNG_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not -1 <= int(f) <= 4:
        raise PnrfError(f'png: filter {filter!r}; one of {sorted(PNG_FILTERS)} or -1 .. 4')
    return int(f)


def png_segment_rows():
    """Rows of filtered bytes per independently coded segment of the encoder's zlib stream (a constant of csrc/pnrf_png_rules.h)."""
    return int(_lib.load().pnrf_png_segment_rows())


def png_max_bytes(H, W, channels):
    """Upper bound of the PNG file of an H x W plane of ``channels`` (1 or 3) bytes per pixel, for any content (pnrf_png_max_bytes)."""
    return int(_lib.load().pnrf_png_max_bytes(int(H), int(W), int(channels)))


def png_encode_host(img, filter='adaptive'):
    """The PNG file (``bytes``) of a uint8 numpy image [H,W] or [H,W,3] from the host twin of the device encoder (pnrf_png_encode_host):
    the same bytes as ``PngEncoder.encode``.  Rows may be strided (a view with a larger row pitch is read as it stands)."""
    lib = _lib.load()
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
        raise PnrfError(f'png_encode_host: expected a uint8 numpy array [H,W] or [H,W,3], got {getattr(img, "dtype", type(img))} {getattr(img, "shape", ())}')
    H, W = int(img.shape[0]), int(img.shape[1])
    ch = 1 if img.ndim == 2 else int(img.shape[2])
    dense = img.strides[-1] == 1 and (img.ndim == 2 or img.strides[1] == ch)      # a row's bytes lie together
    if not (dense and img.strides[0] >= W * ch) or H * W == 0:
        img = np.ascontiguousarray(img)
    stride = int(img.strides[0]) if H * W else W * ch
    cap = max(png_max_bytes(H, W, ch), 64)
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    check(lib.pnrf_png_encode_host(C.c_void_p(img.ctypes.data), stride, H, W, ch, _png_filter(filter), C.c_void_p(out.ctypes.data), cap, C.byref(size)),
          'pnrf_png_encode_host')
    return out[:size.value].tobytes()


class PngEncoder:
    """PNG files of H x W uint8 planes (channels 1: gray, 3: RGB) encoded on the device (pnrf_png_encode_fwd).  Owns the workspace, the output
    buffer of ``png_max_bytes``, a pinned host buffer of the same size and the device cell that receives the file's length; ``encode`` allocates
    nothing and works in stream order, so it can be captured in a graph."""

    def __init__(self, H, W, channels, device):
        lib = _lib.load()
        self.H, self.W, self.channels = int(H), int(W), int(channels)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise PnrfError('PngEncoder: expected a GPU device (pronerf_amd has no CPU path; png_encode_host is the host twin)')
        self.max_bytes = int(lib.pnrf_png_max_bytes(self.H, self.W, self.channels))
        self.workspace_bytes = int(lib.pnrf_png_workspace_bytes(self.H, self.W, self.channels))
        if self.max_bytes <= 0:
            raise PnrfError(f'PngEncoder: {self.H} x {self.W} x {self.channels} is outside what the encoder takes (sides >= 1, H W <= 2^28, 1 or 3 channels)')
        self.out = torch.empty(self.max_bytes, device=self.device, dtype=torch.uint8)
        self.workspace = torch.empty(self.workspace_bytes, device=self.device, dtype=torch.uint8)
        self.size = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.host = torch.empty(self.max_bytes, dtype=torch.uint8).pin_memory()
        self.host_size = torch.zeros(1, dtype=torch.int64).pin_memory()

    def _plane(self, img):
        if not isinstance(img, torch.Tensor) or not img.is_cuda:
            raise PnrfError('PngEncoder: expected a GPU tensor (pronerf_amd has no CPU path)')
        want = (self.H, self.W) if self.channels == 1 else (self.H, self.W, 3)
        if img.dtype != torch.uint8 or tuple(img.shape) != want or img.device != self.device:
            raise PnrfError(f'PngEncoder: expected a uint8 tensor {list(want)} on {self.device}, got {img.dtype} {tuple(img.shape)} on {img.device}')
        st = img.stride()
        if not (st[-1] == 1 and (self.channels == 1 or st[1] == 3) and st[0] >= self.W * self.channels):
            img = img.contiguous()
        return img, int(img.stride(0))

    def launch(self, img, filter='adaptive'):
        """The encoder's launches on the current stream; the file is then in ``self.out``, its length in ``self.size``.  Returns nothing: no sync."""
        img, stride = self._plane(img)
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_png_encode_fwd(_ptr(img), stride, self.H, self.W, self.channels, _png_filter(filter), _ptr(self.out), self.max_bytes, _ptr(self.size),
                                                  _ptr(self.workspace), self.workspace_bytes, _stream()), 'pnrf_png_encode_fwd')

    def encode(self, img, filter='adaptive'):
        """-> uint8 device tensor: a view of the finished file in the encoder's output buffer (valid until the next call).  Reads the length
        back, which synchronises the stream; ``launch`` does not."""
        self.launch(img, filter)
        return self.out[:int(self.size.item())]

    def encode_to_host(self, img, filter='adaptive'):
        """-> ``bytes`` of the file: the launches, one asynchronous copy of ``max_bytes`` and of the length into pinned memory, one sync, a slice."""
        self.launch(img, filter)
        with torch.cuda.device(self.device):
            self.host.copy_(self.out, non_blocking=True)
            self.host_size.copy_(self.size, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return self.host[:int(self.host_size[0])].numpy().tobytes()


# ------------------------------------------------------------------------------------------ JPEG files of an 8-bit plane
def jpeg_max_bytes(H, W, channels):
    """Upper bound of the JPEG file of an H x W plane of ``channels`` (1 or 3) bytes per pixel, for any content and quality (pnrf_jpeg_max_bytes)."""
    return int(_lib.load().pnrf_jpeg_max_bytes(int(H), int(W), int(channels)))


def _jpeg_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise PnrfError(f'jpeg: quality {quality!r}; an integer 1 .. 100')
    return int(quality)


def jpeg_encode_host(img, quality=90):
    """The baseline JPEG file (``bytes``) of a uint8 numpy image [H,W] (gray) or [H,W,3] (RGB, coded as YCbCr 4:4:4) from the host twin of the
    device encoder (pnrf_jpeg_encode_host): the same bytes as ``JpegEncoder.encode``.  Rows may be strided."""
    lib = _lib.load()
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
        raise PnrfError(f'jpeg_encode_host: expected a uint8 numpy array [H,W] or [H,W,3], got {getattr(img, "dtype", type(img))} {getattr(img, "shape", ())}')
    H, W = int(img.shape[0]), int(img.shape[1])
    ch = 1 if img.ndim == 2 else int(img.shape[2])
    dense = img.strides[-1] == 1 and (img.ndim == 2 or img.strides[1] == ch)      # a row's bytes lie together
    if not (dense and img.strides[0] >= W * ch) or H * W == 0:
        img = np.ascontiguousarray(img)
    stride = int(img.strides[0]) if H * W else W * ch
    cap = max(jpeg_max_bytes(H, W, ch), 64)
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    check(lib.pnrf_jpeg_encode_host(C.c_void_p(img.ctypes.data), stride, H, W, ch, _jpeg_quality(quality), C.c_void_p(out.ctypes.data), cap, C.byref(size)),
          'pnrf_jpeg_encode_host')
    return out[:size.value].tobytes()


class JpegEncoder:
    """Baseline JPEG files of H x W uint8 planes (channels 1: gray, 3: RGB as YCbCr 4:4:4) encoded on the device (pnrf_jpeg_encode_fwd).  Owns the
    workspace, the output buffer of ``jpeg_max_bytes``, a pinned host buffer of the same size and the device cell that receives the file's length;
    ``launch`` allocates nothing and works in stream order, so it can be captured in a graph."""

    def __init__(self, H, W, channels, device, quality=90):
        lib = _lib.load()
        self.H, self.W, self.channels, self.quality = int(H), int(W), int(channels), _jpeg_quality(quality)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise PnrfError('JpegEncoder: expected a GPU device (pronerf_amd has no CPU path; jpeg_encode_host is the host twin)')
        self.max_bytes = int(lib.pnrf_jpeg_max_bytes(self.H, self.W, self.channels))
        self.workspace_bytes = int(lib.pnrf_jpeg_workspace_bytes(self.H, self.W, self.channels))
        if self.max_bytes <= 0:
            raise PnrfError(f'JpegEncoder: {self.H} x {self.W} x {self.channels} is outside what the encoder takes (sides 1 .. 65535, 1 or 3 channels)')
        self.out = torch.empty(self.max_bytes, device=self.device, dtype=torch.uint8)
        self.workspace = torch.empty(self.workspace_bytes, device=self.device, dtype=torch.uint8)
        self.size = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.host = torch.empty(self.max_bytes, dtype=torch.uint8).pin_memory()
        self.host_size = torch.zeros(1, dtype=torch.int64).pin_memory()

    def _plane(self, img):
        if not isinstance(img, torch.Tensor) or not img.is_cuda:
            raise PnrfError('JpegEncoder: expected a GPU tensor (pronerf_amd has no CPU path)')
        want = (self.H, self.W) if self.channels == 1 else (self.H, self.W, 3)
        if img.dtype != torch.uint8 or tuple(img.shape) != want or img.device != self.device:
            raise PnrfError(f'JpegEncoder: expected a uint8 tensor {list(want)} on {self.device}, got {img.dtype} {tuple(img.shape)} on {img.device}')
        st = img.stride()
        if not (st[-1] == 1 and (self.channels == 1 or st[1] == 3) and st[0] >= self.W * self.channels):
            img = img.contiguous()
        return img, int(img.stride(0))

    def launch(self, img, quality=None):
        """The encoder's launches on the current stream; the file is then in ``self.out``, its length in ``self.size``.  Returns nothing: no sync."""
        img, stride = self._plane(img)
        q = self.quality if quality is None else _jpeg_quality(quality)
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_jpeg_encode_fwd(_ptr(img), stride, self.H, self.W, self.channels, q, _ptr(self.out), self.max_bytes, _ptr(self.size),
                                                   _ptr(self.workspace), self.workspace_bytes, _stream()), 'pnrf_jpeg_encode_fwd')

    def encode(self, img, quality=None):
        """-> uint8 device tensor: a view of the finished file in the encoder's output buffer (valid until the next call).  Reads the length
        back, which synchronises the stream; ``launch`` does not."""
        self.launch(img, quality)
        return self.out[:int(self.size.item())]

    def encode_to_host(self, img, quality=None):
        """-> ``bytes`` of the file: the launches, one asynchronous copy of ``max_bytes`` and of the length into pinned memory, one sync, a slice."""
        self.launch(img, quality)
        with torch.cuda.device(self.device):
            self.host.copy_(self.out, non_blocking=True)
            self.host_size.copy_(self.size, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return self.host[:int(self.host_size[0])].numpy().tobytes()


# ------------------------------------------------------------------------------------------ stage-2 training step
def composite_bwd(raw, z, rays_d, d_rgb, add=None, mul=None, noise=None, clamp=0.0, white_bkgd=False):
    """raw2outputs backward for d rgb_map -> (d_raw, d_z, d_add, d_mul); d_add / d_mul are None without add / mul.  rays_d may be a
    row-strided [n, 3] view, as in composite."""
    raw = _chk(raw, 'raw', (4,)); z = _chk(z, 'z_vals'); rays_d, d_stride = _chk_rows(rays_d, 'rays_d', 3); d_rgb = _chk(d_rgb, 'd_rgb', (3,))
    n, s = z.shape
    add = None if add is None else _chk(add, 'mm_density_add')
    mul = None if mul is None else _chk(mul, 'mm_density_mul')
    noise = None if noise is None else _chk(noise, 'noise')
    d_raw = torch.empty_like(raw); d_z = torch.empty_like(z)
    d_add = None if add is None else torch.empty_like(z)
    d_mul = None if mul is None else torch.empty_like(z)
    check(_lib.load().pnrf_composite_bwd(_ptr(raw), _ptr(z), _ptr(rays_d), d_stride, _ptr(add), _ptr(mul), _ptr(noise), float(clamp), int(bool(white_bkgd)),
                                         _ptr(d_rgb), _ptr(d_raw), _ptr(d_z), _ptr(d_add), _ptr(d_mul), n, s, _stream()), 'pnrf_composite_bwd')
    return d_raw, d_z, d_add, d_mul


def composite_bwd_maps(raw, z, rays_d, d_rgb=None, d_disp=None, d_acc=None, d_weights=None, d_depth=None, d_z=None, add=None, mul=None, noise=None,
                       clamp=0.0, white_bkgd=False):
    """raw2outputs backward for the cotangents of all its outputs — d_rgb [n, 3], d_disp / d_acc / d_depth [n], d_weights [n, s] — and one that z
    receives from elsewhere (d_z [n, s], added into the returned d_z); None = zeros, not all of them -> (d_raw, d_z, d_add, d_mul) as
    composite_bwd.  A ray with acc == 0 (or depth / acc <= 1e-10) gets exact zeros from d_disp (pnrf_composite_bwd_maps)."""
    raw = _chk(raw, 'raw', (4,)); z = _chk(z, 'z_vals'); rays_d, d_stride = _chk_rows(rays_d, 'rays_d', 3)
    n, s = z.shape
    cot = [None if t is None else _chk(t, name, tail) for t, name, tail in
           ((d_rgb, 'd_rgb', (n, 3)), (d_disp, 'd_disp', (n,)), (d_acc, 'd_acc', (n,)), (d_weights, 'd_weights', (n, s)), (d_depth, 'd_depth', (n,)),
            (d_z, 'd_z', (n, s)))]
    add = None if add is None else _chk(add, 'mm_density_add')
    mul = None if mul is None else _chk(mul, 'mm_density_mul')
    noise = None if noise is None else _chk(noise, 'noise')
    d_raw = torch.empty_like(raw); o_z = torch.empty_like(z)
    d_add = None if add is None else torch.empty_like(z)
    d_mul = None if mul is None else torch.empty_like(z)
    check(_lib.load().pnrf_composite_bwd_maps(_ptr(raw), _ptr(z), _ptr(rays_d), d_stride, _ptr(add), _ptr(mul), _ptr(noise), float(clamp),
                                              int(bool(white_bkgd)), *[_ptr(c) for c in cot], _ptr(d_raw), _ptr(o_z), _ptr(d_add), _ptr(d_mul), n, s,
                                              _stream()), 'pnrf_composite_bwd_maps')
    return d_raw, o_z, d_add, d_mul


def posenc_bwd(x, d_out, n_freq):
    x = _chk(x, 'x', (3,)); d_out = _chk(d_out, 'd_out', (3 + 6 * n_freq,))
    d_x = torch.empty_like(x)
    check(_lib.load().pnrf_posenc_bwd(_ptr(x), _ptr(d_out), _ptr(d_x), x.numel() // 3, n_freq, _stream()), 'pnrf_posenc_bwd')
    return d_x


def sampler_head_fwd(y, rays):
    y = _chk(y, 'y', (27,)); rays = _chk(rays, 'rays', (11,))
    n, dev = y.shape[0], y.device
    depth = torch.empty(n, 8, device=dev, dtype=f32); add = torch.empty_like(depth); mul = torch.empty_like(depth)
    idx = torch.empty(n, 8, device=dev, dtype=torch.int64); rgb = torch.empty(n, 3, device=dev, dtype=f32)
    check(_lib.load().pnrf_sampler_head_fwd(_ptr(y), _ptr(rays), _ptr(depth), _ptr(idx), _ptr(add), _ptr(mul), _ptr(rgb), n, _stream()), 'pnrf_sampler_head_fwd')
    return depth, idx, add, mul, rgb


def sampler_head_bwd(y, rays, idx, d_depth, d_add, d_mul, d_rgb=None):
    y = _chk(y, 'y', (27,)); rays = _chk(rays, 'rays', (11,))
    d_y = torch.empty_like(y)
    check(_lib.load().pnrf_sampler_head_bwd(_ptr(y), _ptr(rays), _ptr(idx.contiguous()), _ptr(_chk(d_depth, 'd_depth', (8,))), _ptr(_chk(d_add, 'd_add', (8,))),
                                            _ptr(_chk(d_mul, 'd_mul', (8,))), _ptr(d_rgb), _ptr(d_y), y.shape[0], _stream()), 'pnrf_sampler_head_bwd')
    return d_y


def refine_head_fwd(y, rays, depth_sorted, jitter=None, jitter_dir=1):
    y = _chk(y, 'y', (35,)); rays = _chk(rays, 'rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    n, dev = y.shape[0], y.device
    z_pre = torch.empty(n, 8, device=dev, dtype=f32); z = torch.empty_like(z_pre)
    pts = torch.empty(n, 8, 3, device=dev, dtype=f32); rgb0 = torch.empty(n, 3, device=dev, dtype=f32)
    jitter = None if jitter is None else _chk(jitter, 'jitter', (8,))
    check(_lib.load().pnrf_refine_head_fwd(_ptr(y), _ptr(rays), _ptr(depth_sorted), _ptr(jitter), int(jitter_dir), _ptr(z_pre), _ptr(z), _ptr(pts), _ptr(rgb0),
                                           n, _stream()), 'pnrf_refine_head_fwd')
    return z_pre, z, pts, rgb0


def refine_head_bwd(y, rays, depth_sorted, z_pre, d_pts, d_z=None, d_rgb0=None, jitter=None, jitter_dir=1):
    y = _chk(y, 'y', (35,)); rays = _chk(rays, 'rays', (11,)); depth_sorted = _chk(depth_sorted, 'depth_sorted', (8,))
    d_y = torch.empty_like(y); d_depth = torch.empty_like(depth_sorted)
    jitter = None if jitter is None else _chk(jitter, 'jitter', (8,))
    check(_lib.load().pnrf_refine_head_bwd(_ptr(y), _ptr(rays), _ptr(depth_sorted), _ptr(_chk(z_pre, 'z_pre', (8,))), _ptr(jitter), int(jitter_dir),
                                           _ptr(_chk(d_pts, 'd_pts', (3,))), _ptr(d_z), _ptr(d_rgb0), _ptr(d_y), _ptr(d_depth), y.shape[0], _stream()),
          'pnrf_refine_head_bwd')
    return d_y, d_depth


TRAINER_LAYERS = 26          # 7 sampler + 7 refine + 12 NeRF class (pts_linears.0..7, feature, alpha, views, rgb)


class Trainer:
    """fp32 parameters, gradients, Adam state and workspaces of the stage-2 training step (pnrf_trainer_*).

    weights / biases: 26 arrays in the order of ``TRAINER_LAYERS`` (torch layout ``W[out, in]``)."""

    def __init__(self, weights, biases, max_rays, device='cuda:0', max_samples=8):
        lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise PnrfError('Trainer needs a GPU device (pronerf_amd has no CPU path)')
        n = len(weights)
        ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32) for w in weights]
        bs = [np.ascontiguousarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float32) for b in biases]
        self.shapes = [w.shape for w in ws]
        Wp = (C.c_void_p * n)(*[w.ctypes.data for w in ws]); bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        ind = (C.c_int * n)(*[w.shape[1] for w in ws]); outd = (C.c_int * n)(*[w.shape[0] for w in ws])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.pnrf_trainer_create(Wp, bp, ind, outd, n, int(max_rays), int(max_samples), C.byref(h)), 'pnrf_trainer_create')
        self.handle = h
        self.max_rays = int(max_rays)
        self.max_samples = int(max_samples)

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().pnrf_trainer_free(self.handle)
                self.handle = None
        except Exception:
            pass

    def read(self, kind, layer):
        """kind: 'param' | 'grad' | 'm' | 'v' (joint Adam) | 'm_nerf' | 'v_nerf' (NeRF-only Adam) -> (W, b) as new device tensors."""
        k = self._KINDS[kind]
        out_d, in_d = self.shapes[layer]
        W = torch.empty(out_d, in_d, device=self.device, dtype=f32); b = torch.empty(out_d, device=self.device, dtype=f32)
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_trainer_read(self.handle, k, layer, _ptr(W), _ptr(b), _stream()), 'pnrf_trainer_read')
        return W, b

    def write(self, kind, layer, W=None, b=None):
        k = self._KINDS[kind]
        W = None if W is None else torch.as_tensor(W, dtype=f32).contiguous()
        b = None if b is None else torch.as_tensor(b, dtype=f32).contiguous()
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_trainer_write(self.handle, k, layer, _ptr(W), _ptr(b), _stream()), 'pnrf_trainer_write')

    _KINDS = {'param': 0, 'grad': 1, 'm': 2, 'v': 3, 'm_nerf': 4, 'v_nerf': 5}

    def publish(self, sampler=None, refine=None, fine=None):
        """Repack ``PackedMLP`` handles in place from the trainer's own device parameters (pnrf_trainer_publish; kernels on the current stream, no host
        synchronisation, no read-back): ``sampler`` from trainer layers 0-6, ``refine`` from 7-13, ``fine`` — a NeRF-class handle — from 14-25.  Any of
        them may be None.  Reads only: allowed between ``forward`` and ``backward``.  A handle of another kind or shape raises ``PnrfError`` before
        anything is launched.  What is built on the handles (``Renderer``, ``RenderContext``, ``PoseGraph``) renders the published weights from its
        next launch in stream order; ``Renderer.calibrate()`` may be called again afterwards, its choice depends on the weights."""
        for name, h in (('sampler', sampler), ('refine', refine), ('fine', fine)):
            if h is not None and not isinstance(h, PackedMLP):
                raise PnrfError(f'Trainer.publish: {name} must be a PackedMLP or None')
        hp = [C.c_void_p(0) if h is None else h.handle for h in (sampler, refine, fine)]
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_trainer_publish(self.handle, *hp, _stream()), 'pnrf_trainer_publish')
        return self

    def flat(self, kind='grad'):
        """Zero-copy torch view [nparam] of one of the trainer's flat device arrays (all layers, trainer order) — e.g. for
        ``torch.distributed.all_reduce`` of the gradients of data-parallel replicas (pronerf_amd.dist.allreduce_gradients)."""
        ptr, n = C.c_void_p(), C.c_int64()
        check(_lib.load().pnrf_trainer_flat(self.handle, self._KINDS[kind], C.byref(ptr), C.byref(n)), 'pnrf_trainer_flat')

        class _Dev:                                      # __cuda_array_interface__ v3: torch wraps the memory without copying
            __cuda_array_interface__ = {'shape': (int(n.value),), 'typestr': '<f4', 'data': (int(ptr.value), False), 'version': 3}
        with torch.cuda.device(self.device):
            t = torch.as_tensor(_Dev(), device=self.device)
        t._pnrf_owner = self                             # keep the trainer alive as long as the view is
        return t

    def set_dw_kernel(self, tile=0, min_rows_128=0):
        """Weight-gradient kernel of the square layers: 0 = by shape and row count, 64 / 128 = forced; 256 / 255 = the grouped gradients' 256 x 128 tiles
        on from ``min_rows_128`` rows / off (pnrf_trainer_set_dw_kernel)."""
        check(_lib.load().pnrf_trainer_set_dw_kernel(self.handle, int(tile), int(min_rows_128)), 'pnrf_trainer_set_dw_kernel')

    def dw_group_info(self):
        """(gradients in the most recent iteration's grouped weight-gradient launch, bit mask of those that ran on 256 x 128 tiles)
        (pnrf_trainer_dw_group_info)."""
        n, m = C.c_int(), C.c_uint()
        check(_lib.load().pnrf_trainer_dw_group_info(self.handle, C.byref(n), C.byref(m)), 'pnrf_trainer_dw_group_info')
        return int(n.value), int(m.value)

    def set_graph(self, enable=True):
        """Replay the iterations as hipGraphs, or (default) launch their kernels one by one (pnrf_trainer_set_graph)."""
        check(_lib.load().pnrf_trainer_set_graph(self.handle, int(bool(enable))), 'pnrf_trainer_set_graph')

    def set_products(self, kind):
        """'f16x2' (default): split-fp16 MFMA layer products (fp32-grade), the fine net's forward as one launch on the fused-MLP engine; 'f32':
        exact-fp32 MFMA products; 'f16x2_unchained': split fp16 with one launch per layer of the fine net's forward; 'f16x2_wchain': with its
        256 -> 256 layers as two 64-row layer chains (bit-identical to 'f16x2_unchained'; pnrf_trainer_set_products)."""
        kinds = {'f16x2': 0, 'f32': 1, 'f16x2_unchained': 2, 'f16x2_wchain': 3}
        if kind not in kinds:
            raise PnrfError(f"Trainer.set_products: kind must be one of {sorted(kinds)} ('f16x2': split-fp16 MFMA products, the default; 'f32': exact-fp32 "
                            f'MFMA products), got {kind!r} (the training drivers read it from PNRF_TRAIN_PRODUCTS)')
        k = kinds[kind]
        check(_lib.load().pnrf_trainer_set_products(self.handle, k), 'pnrf_trainer_set_products')

    def set_step(self, step, step_nerf=0):
        check(_lib.load().pnrf_trainer_set_step(self.handle, int(step), int(step_nerf)), 'pnrf_trainer_set_step')

    def _batch(self, rays, or_rays, target, img4, poses, K, ref_nos, jitter, jitter_dir, raw_noise, white_bkgd, eps, a_mmrgb, clamp, layout, S):
        rays = _chk(rays, 'rays', (11,)); or_rays = _chk(or_rays, 'or_rays', (11,)); target = None if target is None else _chk(target, 'target', (3,))
        img4 = _chk(img4, 'img4', (4,)); poses = _chk(poses, 'poses', (3, 4)); K = _chk(K, 'K', (3, 3))
        if ref_nos.dtype != torch.int64 or not ref_nos.is_cuda or tuple(ref_nos.shape) != (rays.shape[0], 4):
            raise PnrfError('ref_nos: expected an int64 GPU tensor [n, 4]')
        ref_nos = ref_nos.contiguous()
        jitter = None if jitter is None else _chk(jitter, 'jitter', (S,))
        raw_noise = None if raw_noise is None else _chk(raw_noise, 'raw_noise', (S,))
        keep = (rays, or_rays, target, img4, poses, K, ref_nos, jitter, raw_noise)          # alive until the call returns
        bt = _lib.TrainBatch(rays=rays.data_ptr(), or_rays=or_rays.data_ptr(), target=None if target is None else target.data_ptr(), img4=img4.data_ptr(), poses=poses.data_ptr(),
                             K=K.data_ptr(), ref_nos=ref_nos.data_ptr(), jitter=None if jitter is None else jitter.data_ptr(),
                             raw_noise=None if raw_noise is None else raw_noise.data_ptr(), n=rays.shape[0], nv=img4.shape[0], Hf=img4.shape[1],
                             Wf=img4.shape[2], jitter_dir=int(jitter_dir), white_bkgd=int(bool(white_bkgd)), eps=float(eps), a_mmrgb=float(a_mmrgb),
                             clamp=float(clamp), layout=int(layout))
        return bt, keep

    def fwd_bwd(self, rays, or_rays, target, img4, poses, K, ref_nos, jitter=None, jitter_dir=1, raw_noise=None, white_bkgd=False, eps=1e-5,
                a_mmrgb=0.0, want_rgb=True, clamp=0.0, layout=0):
        """One joint forward + backward (stage 2; stage-1 even iterations with clamp=10, layout=1, eps=1e-6, a_mmrgb=1);
        returns (loss[4] device tensor = total, img, rgb0, mm_rgb; rgb_map1 [n,3] or None)."""
        bt, keep = self._batch(rays, or_rays, target, img4, poses, K, ref_nos, jitter, jitter_dir, raw_noise, white_bkgd, eps, a_mmrgb, clamp, layout, 8)
        dev = keep[0].device
        loss = torch.empty(4, device=dev, dtype=f32)
        rgb = torch.empty(keep[0].shape[0], 3, device=dev, dtype=f32) if want_rgb else None
        with torch.cuda.device(dev):
            check(_lib.load().pnrf_train_stage2_fwd_bwd(self.handle, C.byref(bt), _ptr(loss), _ptr(rgb), _stream()), 'pnrf_train_stage2_fwd_bwd')
        return loss, rgb

    # the maps of pnrf_train_maps_t, in the struct's order: name -> trailing shape after the ray count
    MAPS = {'rgb_map1': (3,), 'rgb_map0': (3,), 'mm_rgb': (3,), 'depth': (), 'acc': (), 'disp': (), 'weights': (8,), 'z': (8,)}

    @property
    def anchor(self):
        """A zero-dim leaf with requires_grad: the differentiable input ``autograd.render_train`` hangs the trainer's maps on (the parameters
        live in the trainer, not in torch)."""
        if getattr(self, '_anchor', None) is None:
            self._anchor = torch.zeros((), device=self.device, dtype=f32, requires_grad=True)
        return self._anchor

    def forward(self, rays, or_rays, img4, poses, K, ref_nos, jitter=None, jitter_dir=1, raw_noise=None, white_bkgd=False, eps=1e-5, clamp=0.0,
                layout=0, want=None):
        """Forward half of the joint iteration (pnrf_train_stage2_fwd) -> dict of fresh tensors keyed by ``Trainer.MAPS`` (want: the names to
        return; None = all).  ``backward`` must be the next call on this trainer, on the same stream.  Always kernel by kernel (set_graph does
        not apply)."""
        want = tuple(self.MAPS) if want is None else tuple(want)
        for k in want:
            if k not in self.MAPS:
                raise PnrfError(f'Trainer.forward: unknown map {k!r} (one of {list(self.MAPS)})')
        bt, keep = self._batch(rays, or_rays, None, img4, poses, K, ref_nos, jitter, jitter_dir, raw_noise, white_bkgd, eps, 0.0, clamp, layout, 8)
        n, dev = keep[0].shape[0], keep[0].device
        out = {k: torch.empty((n,) + self.MAPS[k], device=dev, dtype=f32) for k in want}
        maps = _lib.TrainMaps(**{k: out[k].data_ptr() for k in want})
        with torch.cuda.device(dev):
            check(_lib.load().pnrf_train_stage2_fwd(self.handle, C.byref(bt), C.byref(maps), _stream()), 'pnrf_train_stage2_fwd')
        self._split_n = n
        return out

    def backward(self, **cotangents):
        """Backward half (pnrf_train_stage2_bwd) from the cotangents of the maps ``forward`` returned: keyword arguments named as the maps
        (None / absent = zeros).  Leaves the 26 layers' gradients where ``fwd_bwd`` leaves them."""
        n = getattr(self, '_split_n', None)
        ptrs, keep = {}, []
        for k, g in cotangents.items():
            if k not in self.MAPS:
                raise PnrfError(f'Trainer.backward: unknown map {k!r} (one of {list(self.MAPS)})')
            if g is None:
                continue
            if not isinstance(g, torch.Tensor) or not g.is_cuda:
                raise PnrfError(f'Trainer.backward: {k}: expected a GPU tensor (pronerf_amd has no CPU path)')
            if n is not None and tuple(g.shape) != (n,) + self.MAPS[k]:
                raise PnrfError(f'Trainer.backward: {k}: expected shape {(n,) + self.MAPS[k]}, got {tuple(g.shape)}')
            g = g.detach().to(f32).contiguous()
            keep.append(g)
            ptrs['d_' + k] = g.data_ptr()
        cot = _lib.TrainCotangents(**ptrs)
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_train_stage2_bwd(self.handle, C.byref(cot), _stream()), 'pnrf_train_stage2_bwd')

    def explore_fwd_bwd(self, rays, or_rays, target, img4, poses, K, ref_nos, n_mult, dir1, jitter, dir2, raw_noise=None, white_bkgd=False, eps=1e-6,
                        clamp=10.0, layout=1, want_rgb=True):
        """Stage-1 odd iteration: NeRF-only forward + backward on 8*n_mult explored samples per ray (jitter, raw_noise: [n, 8*n_mult])."""
        bt, keep = self._batch(rays, or_rays, target, img4, poses, K, ref_nos, jitter, dir2, raw_noise, white_bkgd, eps, 0.0, clamp, layout, 8 * int(n_mult))
        dev = keep[0].device
        loss = torch.empty(4, device=dev, dtype=f32)
        rgb = torch.empty(keep[0].shape[0], 3, device=dev, dtype=f32) if want_rgb else None
        with torch.cuda.device(dev):
            check(_lib.load().pnrf_train_explore_fwd_bwd(self.handle, C.byref(bt), int(n_mult), int(dir1), _ptr(loss), _ptr(rgb), _stream()),
                  'pnrf_train_explore_fwd_bwd')
        return loss, rgb

    _NETS = {'sampler': (0, 288, 27), 'refine': (1, 144, 35), 'nerf': (2, 3, 4)}

    def net_fwd_bwd(self, net, x, dy, rays=None, S=1, want_dpts=False):
        """y = net(x); y.backward(dy) for one of the three nets through the iterations' dispatch (pnrf_trainer_net_fwd_bwd); overwrites that net's
        gradients only.  net 'sampler': x [n, 288], dy [n, 27]; 'refine': x [n, 144], dy [n, 35]; 'nerf': x = pts [n S, 3], rays [n, 11], dy = d raw
        [n S, 4].  Returns (y, d_pts [n S, 3] or None)."""
        if net not in self._NETS:
            raise PnrfError(f'Trainer.net_fwd_bwd: net must be one of {sorted(self._NETS)}, got {net!r}')
        k, fi, fo = self._NETS[net]
        x = _chk(x, 'x', (fi,)).contiguous(); dy = _chk(dy, 'dy', (fo,)).contiguous()
        rows = x.shape[0]
        if tuple(dy.shape) != (rows, fo):
            raise PnrfError(f'Trainer.net_fwd_bwd: dy must be [{rows}, {fo}], got {tuple(dy.shape)}')
        if k == 2:
            rays = _chk(rays, 'rays', (11,)).contiguous()
            n = rays.shape[0]
            if n * int(S) != rows:
                raise PnrfError(f'Trainer.net_fwd_bwd: pts has {rows} rows, expected n * S = {n} * {S}')
        else:
            n, S, rays = rows, 0, None
        y = torch.empty(rows, fo, device=x.device, dtype=f32)
        d_pts = torch.empty(rows, 3, device=x.device, dtype=f32) if want_dpts else None
        with torch.cuda.device(x.device):
            check(_lib.load().pnrf_trainer_net_fwd_bwd(self.handle, k, _ptr(x), _ptr(rays), int(n), int(S), _ptr(dy), _ptr(y), _ptr(d_pts), _stream()),
                  'pnrf_trainer_net_fwd_bwd')
        return y, d_pts

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, nerf_only=False):
        """optimizer.step(); nerf_only: the stage-1 NeRF-only optimizer (own moments / step count) instead of the joint one."""
        with torch.cuda.device(self.device):
            check(_lib.load().pnrf_trainer_adam_step(self.handle, int(bool(nerf_only)), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                     float(weight_decay), _stream()), 'pnrf_trainer_adam_step')
