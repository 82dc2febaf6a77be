/* pronerf_hip.h — C ABI of libpronerf_hip.so (MI355X / gfx950).
 *
 * The reference (KAIST-VICLab/pronerf) is pure Python over torch; it has no FFI layer.  Its
 * "operator boundary" is the set of Python callables the driver scripts import by name
 * (run_S_eS_eN_alter_trt.py:19,27).  Each entry point below replaces the torch-op sequence of
 * one of those callables (cited per function, paths relative to the reference root) and is
 * what a ctypes binding on the reference side would call.
 *
 * Conventions
 *   - every pointer marked "dev" is device memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); tensors are contiguous, fp32 unless noted; nothing is allocated per call;
 *   - `stream` is a hipStream_t (NULL = default stream); all launches are asynchronous on it,
 *     there is no hidden device synchronisation;
 *   - return 0 = ok, < 0 = argument error (PNRF_E_*), > 0 = hipError_t; the message for the
 *     last non-zero return of the calling thread is available from pnrf_last_error();
 *   - handles are immutable once configured (pack / deserialize [+ pnrf_mlp_set_variant]): entry points are re-entrant across
 *     streams, and no entry point reads the process environment.
 */
#ifndef PRONERF_HIP_H
#define PRONERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNRF_ABI_VERSION 1

#define PNRF_E_ARG (-1)      /* bad argument (null pointer, negative size, wrong dims) */
#define PNRF_E_SHAPE (-2)    /* network shape not supported by the packed kernels */
#define PNRF_E_STATE (-3)    /* handle/context misuse (e.g. more rays than the context was sized for) */

/* network kinds for pnrf_mlp_pack */
#define PNRF_NET_SAMPLER 0   /* MinMaxRaySamplerTRT_Net / MinMaxRay_Net, 288->6x256->27, ELU  (run_nerf_helpers.py:1440-1507) */
#define PNRF_NET_REFINE 1    /* MinMaxRayEpiSamplerTRT_Net, 144->6x256->35, ELU                 (run_nerf_helpers.py:1509-1540) */
#define PNRF_NET_NERF 2      /* DoNeRFTRT(skip='auto'), 63->7x256->[256+27]->4, ReLU            (run_nerf_helpers.py:1186-1343) */
#define PNRF_NET_NERFCLS 3   /* NeRF(D=8,W=256,skips=[4],use_viewdirs=True): the fine net stages 1/2 train and save
                                (run_nerf_helpers.py:792-847).  12 Linear layers in the order pts_linears[0..7],
                                feature_linear, alpha_linear, views_linears[0], rgb_linear; output [rgb(3), alpha]. */

typedef struct pnrf_mlp pnrf_mlp_t;
typedef struct pnrf_ctx pnrf_ctx_t;
typedef struct pnrf_trainer pnrf_trainer_t;
typedef struct pnrf_scene pnrf_scene_t;

int pnrf_abi_version(void);
const char* pnrf_last_error(void);

/* ---- weights ------------------------------------------------------------------------------
 * Pack one network's nn.Linear parameters (HOST pointers, torch layout W[out][in], n_layers
 * matrices) into the device-resident, pre-tiled weight stream consumed by the MFMA kernels.
 * Replaces load_state_dict + .to(device) for the three inference nets
 * (run_S_eS_eN_alter_trt.py:427-458, 468-481).  Synchronous; not on the render path.
 *
 * Shapes (round 6).  The reference sizes its modules from --mmnetdepth, --N_point_ray_enc, --num_neighbor, --netdepth
 * (run_S_eS_eN_alter_trt.py:62-82, 110-118, 427-457); the Fern configs are 6 / 48 / 4 / 8.  Hidden width 256 and 8 samples per ray are fixed; taken are
 *   PNRF_NET_SAMPLER  6 P -> D x 256 (ELU) -> 27      any number of ray points P >= 1 (the fused kernels run the folded first layer, K = 6), 2 <= D <= 32
 *   PNRF_NET_REFINE   48 + 24 nb -> D x 256 -> 35     num_neighbor nb = 1 .. 8, 2 <= D <= 32
 *   PNRF_NET_NERF     63 -> (D - 1) x 256 (ReLU) -> [256 + 27] -> 4     DoNeRFTRT, 3 <= netdepth D <= 8 (from 9 on the reference's skip='auto' moves the
 *                                                                        view input into a hidden layer, run_nerf_helpers.py:1190-1201)
 *   PNRF_NET_NERFCLS  the NeRF class with D = 8, skips = [4], use_viewdirs (12 Linear layers: pts0..7, feature, alpha, views, rgb)
 * Skip connections inside the sampler / refine stacks (--mmnetskips; the reference's default is [4], the Fern configs put it beyond the depth): behind
 * backbone layer i of the set the net input is concatenated back, h = cat([x, h]), so Linear i + 1 has in_dim = 256 + in_dim[0].  pnrf_mlp_pack
 * recognises such a layer by that width for 1 <= i + 1 <= D - 1, i.e. skips in 0 .. D - 2 (a skip at D - 1 would feed the output layer: refused, the
 * reference cannot run it either); pnrf_mlp_skips reports the set as a mask (bit i = skip behind backbone layer i).  A handle with skips runs the
 * default kernels, PNRF_VARIANT_SAMPLER_SPLIT and PNRF_VARIANT_SAMPLER_F32 (pnrf_sampler_fwd[_ws], pnrf_refine_fwd, pnrf_refine_project_fwd,
 * pnrf_mlp_fwd on a refine handle, pnrf_render_rays_fwd); PNRF_VARIANT_REFINE_16X16, PNRF_VARIANT_BF16 on refine, PNRF_VARIANT_SAMPLER_F32_FULL,
 * pnrf_mlp_fwd on a sampler handle and pnrf_refine_train_fwd return PNRF_E_SHAPE with a message that names skips.  The refine stage's PNRF_SHAPE_WIDE form with
 * skips is built for num_neighbor <= 4 (its parked net input must fit the LDS beside the ring): pnrf_mlp_set_shape(WIDE) on another skip net returns
 * PNRF_E_SHAPE, PNRF_SHAPE_AUTO runs it NARROW; a skip refine net with 32 layers and 7 or 8 views is refused by pnrf_mlp_pack.  Everything else returns PNRF_E_SHAPE and
 * the message lists this set.  Three things exist for the Fern values only and say so: the sampler's UNFOLDED first layer (pnrf_mlp_fwd on a sampler handle,
 * PNRF_VARIANT_SAMPLER_F32_FULL: P = 48), PNRF_VARIANT_BF16_32X32 and pnrf_mlp_fwd on a DoNeRFTRT handle (netdepth 8), the training entry points (the
 * trainer's shapes).  pnrf_mlp_kind reports in_dim, from which P = in_dim / 6 resp. nb = (in_dim - 48) / 24 follow. */
int pnrf_mlp_pack(int net, const float* const* W, const float* const* b, const int* in_dim,
                  const int* out_dim, int n_layers, pnrf_mlp_t** out);
int pnrf_mlp_free(pnrf_mlp_t* h);

/* ---- engine files -------------------------------------------------------------------------
 * A packed network as one flat byte image (128-byte header + the weight stream and its maps):
 * the counterpart of the serialized TensorRT engines the reference builds with `export-trt`
 * (pronerf/cli.py:105-157, onnx2trt.get_engine) and deserializes at start-up
 * (run_S_eS_eN_alter_trt.py:490-499, trt_infer_v2.py NeRFEngine/MMEngine/RefineEngine).
 * serialize: buf == NULL only reports the size in *size; otherwise capacity >= *size and the image
 * is written to HOST memory (synchronous device read).  deserialize builds a new handle on the
 * current device from a HOST image; images from another library build (ABI version / stream layout
 * tag), truncated or corrupt images are refused with PNRF_E_STATE / PNRF_E_ARG.
 * pnrf_mlp_kind reports what a handle holds (any out pointer may be NULL); pnrf_mlp_skips the skip mask of a sampler / refine handle (0 for the
 * other kinds).  Engine images are format 6 since they carry that mask; older images are refused like any other build's. */
int pnrf_mlp_serialize(const pnrf_mlp_t* h, void* buf, int64_t capacity, int64_t* size);
int pnrf_mlp_deserialize(const void* buf, int64_t size, pnrf_mlp_t** out);
int pnrf_mlp_kind(const pnrf_mlp_t* h, int* net, int* in_dim, int* in_dim_x, int* out_dim);
/* The packer's host half: the engine image of a net, written to HOST memory without touching a device — byte for byte what
 * pnrf_mlp_serialize(pnrf_mlp_pack(...)) writes.  Arguments, checks, return codes and messages as pnrf_mlp_pack; (buf, capacity, size) as
 * pnrf_mlp_serialize (buf == NULL only reports the size).  pnrf_mlp_pack itself is this followed by the upload pnrf_mlp_deserialize makes. */
int pnrf_mlp_pack_image(int net, const float* const* W, const float* const* b, const int* in_dim,
                        const int* out_dim, int n_layers, void* buf, int64_t capacity, int64_t* size);
int pnrf_mlp_skips(const pnrf_mlp_t* h, uint32_t* mask);
/* Repack a handle in place, on the device, from weights that live on the device: W[l] / b[l] are DEVICE pointers (torch layout W[out, in], layer order
 * of pnrf_mlp_pack); the arrays of pointers and dims are host arrays.  Kernels on `stream` rewrite every weight-dependent buffer of the handle — all its
 * weight streams, the bias tables, the pass-1 constants — at the same device addresses, to the bytes pnrf_mlp_pack_image writes for these weights (the
 * kernels and the host packer share one statement of the element rules; only NaN payloads may differ).  Maps, ray points, variant and shape settings are
 * left alone, so contexts, scenes and captured graphs that hold the handle's buffers stay valid.
 * The weights must have the handle's shape (net kind, hidden layers, ray points, neighbour views, skip mask; a deserialized handle serves as well):
 * PNRF_E_SHAPE otherwise, PNRF_E_ARG for a null pointer, PNRF_E_STATE for a handle of another device than the current one — all decided on the host before
 * anything is launched: a refused call leaves the handle untouched.
 * The call never synchronises with the host.  The first call on a handle allocates and uploads a small plan (the packer's per-layer tables, scratch for
 * the folded matrices), owned by the handle and freed by pnrf_mlp_free; later calls allocate and copy nothing and can be captured in a hipGraph on one
 * stream (the weight pointers are kernel arguments: a captured call reads the addresses it was captured with).
 * ORDERING: the rewrite is ordered against renders that use the handle by stream order alone, and that is the caller's business — run it on the stream
 * the handle's launches run on, or order the streams with events.  The weights are read when the kernels run, not when the call returns. */
int pnrf_mlp_repack(pnrf_mlp_t* h, const float* const* W, const float* const* b, const int* in_dim,
                    const int* out_dim, int n_layers, void* stream);

/* Kernel variant of a packed network.  PNRF_VARIANT_DEFAULT is what pack / deserialize produce and what every product path runs:
 * sampler with the folded first layer in split fp16 (fp32-grade, three v_mfma_f32_16x16x32_f16 per product) — through pnrf_sampler_fwd_ws /
 * pnrf_render_rays_fwd as the second of two passes, see there —, refine stage on v_mfma_f32_32x32x16_f16 (fp16 operands: its refined depths
 * feed 2^9 positional octaves, and with bf16 operands they are the largest error of the frame), NeRF stage on v_mfma_f32_16x16x32_bf16
 * (the "bf16 MLP" of BASELINE.json configs[1]); fp32 accumulation everywhere.  fp16 kernels run with MODE.FP16_OVFL: packed activations
 * saturate at 65 504 instead of overflowing.  The others exist for parity tests and A/B timing (tools/perf_ab.py, tools/variant_psnr.py):
 *   SAMPLER_F32       sampler on the exact fp32 FMA chain (v_mfma_f32_16x16x4_f32), folded first layer;
 *   SAMPLER_F32_FULL  ... with the full K = 288 first layer on the 48 Pluecker points (no fold);
 *   SAMPLER_SPLIT     the split-fp16 kernel for every ray, also where a workspace is given (single pass: the default of round 2);
 *   BF16              refine handles: bf16 operands (8 significand bits; the round-2 default); NeRF handles: same as DEFAULT;
 *   F16               NeRF handles: fp16 operands (11 significand bits, like the FP16 TensorRT engines of the reference's own fast path,
 *                     trt_infer_v2.py: raw output within the authors' 1e-3 tolerance) — same MFMA count, 5 % slower under the power limit;
 *   BF16_32X32        NeRF handles: the v_mfma_f32_32x32x16_bf16 engine;
 *   REFINE_16X16      refine handles: the fused inference stage (pnrf_refine_fwd, pnrf_refine_project_fwd, pnrf_render_rays_fwd) on
 *                     v_mfma_f32_16x16x32_f16 — the NeRF stage's engine shape, four lanes per ray instead of two; same fp16 operands;
 *   NERF_4X64         NeRF handles: bf16, 4 waves of 64 columns per workgroup (one wave per SIMD) instead of 8 waves of 32 — same arithmetic,
 *                     same packed stream, every weight fragment read from LDS feeds four MFMAs instead of two.
 * A variant is part of a handle's configuration, like its weights: set it right after pack / deserialize, before the handle is given to
 * a context or a stream (the call is not synchronised against launches that use the handle).  Nothing in the library reads the process
 * environment to pick kernels.  Returns PNRF_E_ARG for a variant the handle's net kind does not have. */
#define PNRF_VARIANT_DEFAULT 0
#define PNRF_VARIANT_SAMPLER_F32 1
#define PNRF_VARIANT_SAMPLER_F32_FULL 2
#define PNRF_VARIANT_BF16_32X32 3
#define PNRF_VARIANT_NERF_4X64 4
#define PNRF_VARIANT_SAMPLER_SPLIT 5
#define PNRF_VARIANT_BF16 6
#define PNRF_VARIANT_F16 7
#define PNRF_VARIANT_REFINE_16X16 8
int pnrf_mlp_set_variant(pnrf_mlp_t* h, int variant);
/* Workgroup shape of the fused stages (sampler passes, projection + refine, NeRF) launched from this handle — how a launch's columns (rays or
 * ray samples) are cut into batches and spread over the 256 CUs.  The reference renders any ray count through the same modules
 * (run_S_eS_eN_alter_trt.py:223: `chunk` is accepted and unused); here a whole frame and a 1024-ray chunk want different shapes:
 *   WIDE    one 8-wave workgroup per CU (two waves per SIMD) walking batches of 256 columns (128 rays in the split-fp16 sampler kernel):
 *           every weight fragment streamed into the CU feeds 8 waves.  Whole frames, ray shards.
 *   NARROW  one 4-wave workgroup per CU (a SIMD per wave) on batches of half the width: a call of at most one such batch per CU takes the
 *           latency of one batch through the layers, and a wave that has its SIMD to itself gets through them in 0.7 of the time
 *           (a 1024-ray call: 8 / 16 / 8 / 64 workgroups in the four kernels; 0.148 -> 0.114 ms).
 *   AUTO    (what pack / deserialize produce) NARROW when the launch has at most one narrow batch per CU, else WIDE.
 * Every ray's instruction stream is the same in both shapes: results are bit-identical (tests/test_render_gpu.py).  In both shapes a CU
 * holds at most ONE workgroup of these kernels (registers exclude a second wide one, the LDS request a second narrow one), whatever runs on
 * other streams.  Configuration like the variant: set before the handle is used; the single-kernel test variants (SAMPLER_F32*, BF16_32X32,
 * NERF_4X64) have one shape. */
#define PNRF_SHAPE_AUTO 0
#define PNRF_SHAPE_NARROW 4
#define PNRF_SHAPE_WIDE 8
int pnrf_mlp_set_shape(pnrf_mlp_t* h, int shape);

/* Module-level forward y = net(x), [m, out_dim].  head_act = 0: the raw output of the last Linear
 * (MinMaxRay_Net.forward, DoNeRFTRT.forward); head_act = 1: with the head activations of the TRT
 * wrapper classes applied in place of their slicing ops — sampler: sigmoid on y[0:8] and y[24:27];
 * refine: sigmoid on y[0:8] and y[32:35], tanh on y[8:32] (run_nerf_helpers.py:1502-1505, 1536-1538).
 * x: dev [m, in_dim]; x_views: dev [m, 27] (PNRF_NET_NERF / PNRF_NET_NERFCLS: the view embedding; x is then
 * the 63-wide position embedding), else NULL.
 * Replaces <module>.forward (run_nerf_helpers.py:1490-1507, 1526-1540, 1331-1343). */
int pnrf_mlp_fwd(const pnrf_mlp_t* h, const float* x, const float* x_views, float* y, int64_t m,
                 int head_act, void* stream);

/* ---- element-wise operators --------------------------------------------------------------- */
/* Embedder.embed: out[n, 3+6*n_freq] = [x, sin(2^k x), cos(2^k x)]_k  (run_nerf_helpers.py:666-671). */
int pnrf_posenc_fwd(const float* x, float* out, int64_t n, int n_freq, void* stream);
/* Pluecker.forward: out[n,6] = [d/|d|, o x d/|d|]  (run_nerf_helpers.py:629-632). */
int pnrf_plucker_fwd(const float* o, const float* d, float* out, int64_t n, void* stream);
/* Sampler input: mm_input[n, 6*n_pts] = Pluecker of n_pts points o + t d, t = linspace(0,1,n_pts);
 * rays: dev [n, 11] NDC ray batch (run_S_eS_eN_alter_trt.py:274-277, 546-562). */
int pnrf_ray_encode_fwd(const float* rays, float* mm_input, int64_t n, int n_pts, void* stream);
/* Per-frame ray set-up: get_rays + viewdirs + ndc_rays -> rays[H*W,11] = [o',d',near,far,viewdir],
 * or_rays[H*W,11] = [o,d,or_near,or_far,viewdir].  K (3x3) and c2w (3x4) are HOST pointers.
 * (run_S_eS_eN_alter_trt.py:245-271; run_nerf_helpers.py:2705-2714, 2776-2793). */
int pnrf_frame_rays_fwd(const float* K, const float* c2w, int H, int W, float near, float far,
                        float or_near, float or_far, int64_t first, int64_t count,
                        float* rays, float* or_rays, void* stream);
/* The same for the pixels of a block-cyclic ray partition (multi-GPU frames; pronerf_amd.render.RayPartition): output row q is
 * pixel first + (q / block) * stride + q % block — rank r of `world` ranks dealt blocks of `block` consecutive pixels round-robin passes
 * first = r * block, stride = world * block and count = the number of pixels it owns.  stride = 0 with count <= block is the contiguous
 * range of pnrf_frame_rays_fwd.  Blocks that leave the frame or overlap are refused. */
int pnrf_frame_rays_blocks_fwd(const float* K, const float* c2w, int H, int W, float near, float far,
                               float or_near, float or_far, int64_t first, int64_t block, int64_t stride,
                               int64_t count, float* rays, float* or_rays, void* stream);
/* ndc_rays on an arbitrary ray set: rays_o, rays_d dev [n,3] -> out_o, out_d dev [n,3]
 * (run_nerf_helpers.py:2776-2793). */
int pnrf_ndc_rays_fwd(const float* rays_o, const float* rays_d, int H, int W, float focal, float near,
                      float* out_o, float* out_d, int64_t n, void* stream);
/* inverse_warp_rod1_rt2_coords_trt: img dev [B,3,Hf,Wf]; depth dev [B,n]; ro1,rd1 dev [4,n] per
 * batch entry with batch stride ray_bstride floats (0 = shared by all B, the reference's
 * expand()); w2c dev [B,3,4]; out dev [B,3,n].
 * Bilinear, zero padding, align_corners=True (inverse_warp.py:584-619).
 * Pinned bit for bit by tests/test_exact_project_gpu.py (fp32 replay: tests/exact_project.py). */
int pnrf_warp_trt_fwd(const float* img, const float* depth, const float* ro1, const float* rd1,
                      int64_t ray_bstride, const float* w2c, float* out, int B, int Hf, int Wf,
                      int64_t n, void* stream);
/* inverse_warp_rod1_rt2_coords (training variant): c2 = R^T w - R^T t, c2 /= |c2.z|+1e-8, c2.z = 1, c2.y = -c2.y,
 * p = K c2; samples whose normalised X or Y leaves [-1,1] give 0.  img dev [B,3,Hf,Wf]; depth dev [B,n]; ro1, rd1 dev
 * [3,n] per batch entry (batch stride ray_bstride floats, 0 = shared); c2w2 dev [B,3,4]; K dev [B,3,3]; out dev
 * [B,3,n]  (inverse_warp.py:515-581).
 * Pinned bit for bit by tests/test_exact_project_gpu.py, the mask's boundary xn, yn == +-1 (inside) included. */
int pnrf_warp_train_fwd(const float* img, const float* depth, const float* ro1, const float* rd1,
                        int64_t ray_bstride, const float* c2w2, const float* K, float* out, int B, int Hf,
                        int Wf, int64_t n, void* stream);
/* Neighbour images [nv,3,Hf,Wf] -> texel-interleaved [nv,Hf,Wf,4] used by the fused projection
 * (replaces the x8 image replication of run_S_eS_eN_alter_trt.py:296-298).  Texels must be finite (pnrf_geom.h). */
int pnrf_images_pack(const float* img_nchw, float* out_nhwc4, int nv, int Hf, int Wf, void* stream);
/* Projection + sample Pluecker: refine_in[n, 48 + 24 nb] (nb = 4: [n,144]) = [pluecker(8 samples)(48), epi(24 nb)], nb = 1 .. 8, with
 * epi index (k*8+s)*3+c  (run_S_eS_eN_alter_trt.py:637-661).  rays,or_rays dev [n,11];
 * depth_sorted dev [n,8]; img4 dev [nb,Hf,Wf,4]; proj dev [nb,3,4]; eps = 1e-5 (stage 1: 1e-6).
 * Non-finite pixel coordinates (p.z == 0) give zeros in their own three columns.
 * Pinned bit for bit by tests/test_exact_project_gpu.py for nb = 1 .. 8. */
int pnrf_refine_input_fwd(const float* rays, const float* or_rays, const float* depth_sorted,
                          const float* img4, const float* proj, int nb, int Hf, int Wf, float eps,
                          float* refine_in, int64_t n, void* stream);
/* Training-time refine_in[n,144]: like pnrf_refine_input_fwd but with per-ray source views ref_nos dev [n,4] (int64,
 * indices into the nv training views img4 dev [nv,Hf,Wf,4] / poses dev [nv,3,4] camera-to-world), the training
 * projection (pnrf_warp_train_fwd) and the valid-mask mean fill: valid = (sum_c rgb > 0), invalid (view, sample)
 * entries are replaced by the mean over the valid views of that sample.  K dev [3,3].  layout 0: epi index
 * (k*8+s)*3+c (stage 2); 1: s*12+k*3+c (stage 1).
 * (run_S_eS_eN_alter_base_refine2.py:570-634; run_S_eS_eN_alter_base.py:607-673)
 * ref_nos outside 0 .. nv - 1 are clamped.  Pinned bit for bit, both layouts, by tests/test_exact_project_gpu.py. */
int pnrf_refine_input_train_fwd(const float* rays, const float* or_rays, const float* depth_sorted,
                                const float* img4, const float* poses, const float* K, const int64_t* ref_nos,
                                int nv, int nb, int Hf, int Wf, float eps, int layout, float* refine_in,
                                int64_t n, void* stream);
/* raw2outputs (infer variant; clamp/noise/white_bkgd select the training variants):
 * raw dev [n,s,4]; z dev [n,s]; rays_d dev [n,3] with row stride d_stride floats; add,mul dev
 * [n,s] or NULL; noise dev [n,s] or NULL.  Outputs (any may be NULL): rgb[n,3], disp[n],
 * acc[n], weights[n,s], depth[n]  (run_S_eS_eN_alter_trt.py:564-597). */
int pnrf_composite_fwd(const float* raw, const float* z, const float* rays_d, int d_stride,
                       const float* add, const float* mul, const float* noise, float clamp,
                       int white_bkgd, float* rgb, float* disp, float* acc, float* weights,
                       float* depth, int64_t n, int s, void* stream);

/* ---- fused stages ---------------------------------------------------------------------------
 * Sampler: Pluecker ray encoding -> MLP -> sigmoid, depth affine, stable ascending sort of the 8 depths,
 * permutation of add/mul.  Arithmetic of a DEFAULT handle: every layer product in SPLIT fp16 (hi + lo planes, three
 * v_mfma_f32_16x16x32_f16 per product, fp32 accumulation: fp32-grade, 22 significand bits per operand), every ray in one pass —
 * the exact-index form; SAMPLER_F32 / SAMPLER_F32_FULL handles run the exact fp32 FMA chain (v_mfma_f32_16x16x4_f32) instead.
 * (The frame path pnrf_render_rays_fwd runs pnrf_sampler_fwd_ws below: a plain-fp16 first pass + this kernel on the undecided
 * rays.)  rays dev [n,11].  Outputs dev:
 * depth_sorted[n,8], add_sorted[n,8], mul_sorted[n,8]; optional (NULL to skip) sort_idx[n,8]
 * (int64, the "sampler indices"), mm_rgb[n,3], depth_raw[n,8] (sigmoid output before the sort).
 * (run_S_eS_eN_alter_trt.py:628-635) */
int pnrf_sampler_fwd(const pnrf_mlp_t* h, const float* rays, int64_t n, float* depth_sorted,
                     float* add_sorted, float* mul_sorted, int64_t* sort_idx, float* mm_rgb,
                     float* depth_raw, void* stream);
/* The same operator in two passes (what pnrf_render_rays_fwd runs).  The eight depths of a ray are sorted, so the products must be
 * fp32-grade wherever two of them are close — and only there.  Pass 1 renders every ray in plain fp16 (one v_mfma_f32_32x32x16_f16 per
 * product, a third of the split kernel's MFMA work) and carries, per ray, a bound s_k on the standard deviation of its own rounding error
 * in depth k (variance propagation through the layers from |x_l|^2 and the weights' column norms); a ray is "undecided" when
 * some adjacent sorted gap is not larger than kappa (s_i + s_i+1) + 2e-6 (far - near), when a depth is not finite, or when one of its
 * activations reached the fp16 limit.  Pass 2 renders the undecided rays with the split-fp16 kernel of pnrf_sampler_fwd and overwrites
 * their rows.  Pass 3 (a few workgroups that leave at once when there is nothing to do) renders with the exact-fp32 kernel
 * (PNRF_VARIANT_SAMPLER_F32's) the rays of pass 2 in which a hidden activation saturated at 65 504 — fp16 range is DEFINED: every kernel
 * runs with MODE.FP16_OVFL (saturation instead of inf), a saturated ray is detected and re-rendered in fp32, nothing becomes NaN.
 * Guarantee: the depths / add / mul of the rays of passes 2 and 3 are identical to pnrf_sampler_fwd's (split fp16 resp. exact fp32:
 * fp32-grade); those of the other rays are fp16-grade (measured <= 6e-4 (far - near), tested <= 2e-3) and their SORT INDICES equal
 * pnrf_sampler_fwd's under the error model — a statistical bound (fp16 roundings treated as independent zero-mean errors; subnormals and
 * fp32 accumulation error are covered by the 2e-6 allowance), not a proof.  kappa = 2 (round 5; 4 before): the bound s is >= 2.7 sigma of the
 * measured error where it is tightest (largest |error| / s over 524 288 depths: 0.8 .. 1.9 on seven weight sets, tools/sampler_twopass_model.py),
 * so the threshold is >= 7.6 sigma of the difference of two errors; it is 2x the smallest kappa that was ever clean and >= 4x the first that
 * was not (0 index mismatches on 762 048 rays x synthetic, heavy-tailed, x4-scaled and optimizer-trained weights down to kappa = 1; one ray
 * of 3 M at 0.5: tools/kappa_scan.py, tests/test_fullframe_gpu.py; 0 of 45.7 M rays of 60 further weight sets at kappa = 2 and at 1:
 * tools/kappa_population.py).  It halves the second pass (7.5 % of the bench frame's rays instead of
 * 14.6 %).  Where exactness matters more than 0.5 ms per frame, PNRF_VARIANT_SAMPLER_SPLIT renders every ray fp32-grade;
 * pnrf_ctx_set_sampler_kappa restores a wider margin per context.
 * kappa < 0 selects PNRF_SAMPLER_KAPPA; kappa = 0 leaves only the fp32 round-off allowance (tests); NaN and values >= 1e30 are refused.
 * workspace: dev, 16-byte aligned, >= pnrf_sampler_workspace_bytes(n) bytes, contents irrelevant (its counters are reset on the stream
 * by every call); concurrent calls need separate workspaces.  Handles set to SAMPLER_SPLIT run the split kernel for every ray + pass 3;
 * SAMPLER_F32* handles run their single kernel.
 * After the call (in stream order) the workspace stays readable as int32 words until the next call on it: word 1 = rays of pass 2, word 5 = rays of
 * pass 3, words 16 .. 16 + [1] the list of pass 2 and words 16 + n .. 16 + n + [5] the list of pass 3 (ray numbers, distinct, in no particular order;
 * what lies behind the counts is left over from earlier calls).
 * Pinned by tests/test_twopass_flags_gpu.py against tests/twopass_ref.py: the critical kappa of every ray (the bound s with the kernel's constants,
 * DESIGN.md 4.1) to a relative 1.4e-4, the flag's monotony in kappa, the rays flagged at every kappa (gap inside the allowance, not finite, fp16 limit),
 * the lists, and bit for bit which kernel every output row comes from (n = 1 .. 257, past the grid cap, saturated rays, a second call on the same workspace). */
#define PNRF_SAMPLER_KAPPA 2.0f
int64_t pnrf_sampler_workspace_bytes(int64_t n);
int pnrf_sampler_fwd_ws(const pnrf_mlp_t* h, const float* rays, int64_t n, float* depth_sorted, float* add_sorted,
                        float* mul_sorted, int64_t* sort_idx, float* mm_rgb, float* depth_raw, void* workspace,
                        int64_t workspace_bytes, float kappa, void* stream);
/* Refine: MLP on refine_in[n, 48 + 24 nb] (the handle's num_neighbor; Fern: [n,144]) -> sigmoid/tanh -> interval refinement -> query points.  Arithmetic of a DEFAULT handle: fp16
 * operands (v_mfma_f32_32x32x16_f16, 11 significand bits, MODE.FP16_OVFL saturation), fp32 accumulation; a handle set to
 * PNRF_VARIANT_BF16 runs bf16 operands (8 bits; the round-2 default).
 * Outputs dev: z[n,8], pts[n,8,3]  (run_S_eS_eN_alter_trt.py:668-681). */
int pnrf_refine_fwd(const pnrf_mlp_t* h, const float* refine_in, const float* rays,
                    const float* depth_sorted, float* z, float* pts, int64_t n, void* stream);
/* Projection + refine in ONE kernel: what pnrf_refine_input_fwd followed by pnrf_refine_fwd compute, without the refine_in [n,144]
 * round trip through HBM.  NOT bit for bit: the colours go straight into the MFMA operands (fp16 on a DEFAULT handle, bf16 on a PNRF_VARIANT_BF16 one), so the head uses a linearised projection
 * p(z) = A + z B per (ray, view) with FMA contraction and v_rcp_f32 for 1 / (1 - d - eps) and 1 / p.z, and skips grid_sample's normalise /
 * un-normalise round trip: pixel coordinates move by a few fp32 ulps (~1e-4 px), colours by ~1e-4 of the local texel difference, well
 * below the operand rounding applied next (fp16: 5e-4 relative) (tests/test_ops_gpu.py bounds z within 2e-3 of the two-kernel path).  The operator that replays
 * the reference's fp32 projection sequence exactly is pnrf_refine_input_fwd.  Here every workgroup projects the samples of its 256 rays into the four neighbour views, fetches
 * the colours and encodes the sample Pluecker values in the head of its batch, straight into the MFMA operand registers.
 * rays, or_rays dev [n,11]; depth_sorted dev [n,8]; img4 dev [nb,Hf,Wf,4] (pnrf_images_pack); proj dev [nb,3,4]; eps as pnrf_refine_input_fwd;
 * nb must be the handle's num_neighbor (1 .. 8; 4 in the Fern configs: a lane half then projects two views, ceil(nb / 2) in general).
 * This is the refine stage of pnrf_render_rays_fwd.  (run_S_eS_eN_alter_trt.py:637-681; inverse_warp.py:584-619)
 * Pinned by tests/test_exact_project_gpu.py: on integer nets and colours it equals pnrf_refine_fwd on the reference's refine_in. */
int pnrf_refine_project_fwd(const pnrf_mlp_t* h, const float* rays, const float* or_rays, const float* depth_sorted,
                            const float* img4, const float* proj, int nb, int Hf, int Wf, float eps, float* z,
                            float* pts, int64_t n, void* stream);
/* Training-time refine stage (stage 2): as pnrf_refine_fwd, plus the depth jitter of refine2.py:646-662 —
 * jitter dev [n,8] = min(|N(0,1)|/5, 1-2e-6) or NULL, jitter_dir +1 (toward the next refined sample / far) or -1 (toward
 * the previous / near): z += dir * jitter * |z - neighbour| — and the refine rgb head rgb0 dev [n,3] =
 * sigmoid(y[32:35]) (rgb_map0) or NULL.  (run_S_eS_eN_alter_base_refine2.py:635-668) */
int pnrf_refine_train_fwd(const pnrf_mlp_t* h, const float* refine_in, const float* rays,
                          const float* depth_sorted, const float* jitter, int jitter_dir, float* z, float* pts,
                          float* rgb0, int64_t n, void* stream);
/* NeRF: positional encoding of pts/viewdirs -> MLP (DEFAULT handle: bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation;
 * PNRF_VARIANT_F16: fp16 operands) -> alpha compositing with the sampler's
 * density modulation.  pts dev [n,8,3]; rays dev [n,11]; z, add_sorted, mul_sorted dev [n,8].
 * Outputs dev: rgbd[n,4] = (r,g,b,depth); raw[n,8,4] optional (NULL to skip).  h may be a PNRF_NET_NERF or a
 * PNRF_NET_NERFCLS handle (the fine-net class mismatch of the released scripts).
 * (run_S_eS_eN_alter_trt.py:691-694; run_network :195-208) */
int pnrf_nerf_fwd(const pnrf_mlp_t* h, const float* pts, const float* rays, const float* z,
                  const float* add_sorted, const float* mul_sorted, float* rgbd, float* raw,
                  int64_t n, void* stream);

/* Training-time NeRF stage: as pnrf_nerf_fwd, plus noise dev [n,S] (= randn * raw_noise_std, added to sigma before
 * the density modulation) or NULL; clamp > 0 clamps raw to +-clamp first (stage 1: 10); white_bkgd (rgb += 1 - acc);
 * add_sorted/mul_sorted may both be NULL (stage-1 odd steps composite without them); S samples per ray: pts dev
 * [n,S,3].  S == 8: fused compositing into rgbd (raw optional).  S != 8 (stage-1 exploration, 16..256): rgbd must be
 * NULL and raw dev [n,S,4] is written; composite it with pnrf_composite_fwd.
 * (run_S_eS_eN_alter_base_refine2.py:497-520, 669-676; run_S_eS_eN_alter_base.py:523, 731-751) */
int pnrf_nerf_train_fwd(const pnrf_mlp_t* h, const float* pts, const float* rays, const float* z,
                        const float* add_sorted, const float* mul_sorted, const float* noise, float clamp,
                        int white_bkgd, int S, float* rgbd, float* raw, int64_t n, void* stream);
/* Stage-1 exploration of the refined depths (run_S_eS_eN_alter_base.py:689-729): every one of the 8 depths z8 dev
 * [n,8] is replicated n_mult times toward the next (dir1 = +1) or previous (-1) sample with offsets
 * linspace(0, 1-1/n_mult, n_mult)*|gap|, the 8*n_mult values are sorted, then jittered: z += dir2 * jitter * |z -
 * neighbour| with jitter dev [n, 8*n_mult] = min(|N(0,1)|/5, 0.99).  Outputs dev: z_out [n, 8*n_mult] and the query
 * points pts_out [n, 8*n_mult, 3] = o + d*z (no learned offsets on these steps).  n_mult 1..32. */
int pnrf_explore_fwd(const float* z8, const float* rays, const float* jitter, int n_mult, int dir1, int dir2,
                     float* z_out, float* pts_out, int64_t n, void* stream);

/* ---- whole path: render_rays (inference) ----------------------------------------------------
 * A context owns the per-ray workspace for up to max_rays rays (allocated once). */
int pnrf_ctx_create(const pnrf_mlp_t* sampler, const pnrf_mlp_t* refine, const pnrf_mlp_t* nerf,
                    int64_t max_rays, pnrf_ctx_t** out);
int pnrf_ctx_free(pnrf_ctx_t* ctx);
/* render_rays(ray_batch, or_ray_batch, ...) -> rgbd[n,4] = (rgb_map, depth_map); sort_idx
 * optional.  img4 dev [nb,Hf,Wf,4] (pnrf_images_pack), proj dev [nb,3,4].
 * (run_S_eS_eN_alter_trt.py:599-696) */
int pnrf_render_rays_fwd(pnrf_ctx_t* ctx, const float* rays, const float* or_rays,
                         const float* img4, const float* proj, int nb, int Hf, int Wf, float eps,
                         float* rgbd, int64_t* sort_idx, int64_t n, void* stream);
/* Threshold of the two-pass sampler for this context's calls (pnrf_sampler_fwd_ws's kappa): negative = PNRF_SAMPLER_KAPPA (what a new
 * context has), 0 = only the fp32 round-off allowance; NaN and values >= 1e30 are refused.  A larger kappa sends more rays through the
 * fp32-grade second pass; PNRF_VARIANT_SAMPLER_SPLIT on the sampler handle sends all of them (the exact path). */
int pnrf_ctx_set_sampler_kappa(pnrf_ctx_t* ctx, float kappa);
/* The kappa this context's calls run with (PNRF_SAMPLER_KAPPA unless pnrf_ctx_set_sampler_kappa chose another): what bench.py reports. */
int pnrf_ctx_get_sampler_kappa(const pnrf_ctx_t* ctx, float* kappa);
/* Rays the sampler's second pass rendered in the context's most recent pnrf_render_rays_fwd (waits for the device; diagnostics). */
int pnrf_ctx_sampler_stats(pnrf_ctx_t* ctx, int64_t* rays_second_pass);
/* Rays whose hidden activations reached the fp16 limit in the split-fp16 kernel and were therefore rendered by the exact-fp32 kernel (the
 * third pass) in the context's most recent pnrf_render_rays_fwd: 0 for every net whose activations stay below 65 504 / log2(e) (waits for the
 * device; diagnostics). */
int pnrf_ctx_sampler_saturated(pnrf_ctx_t* ctx, int64_t* rays_third_pass);
/* NeRF stage of pnrf_render_rays_fwd: evaluate only the samples whose sampler gate is open.  Compositing multiplies a sample's alpha by relu(mul), and mul
 * is an output of the sampler: where mul <= 0 (or NaN) the sample's weight is exactly 0 and the network's answer for it cannot change the output, as long as
 * that answer is finite.  On this path a small kernel lists the live columns (ray * 8 + s with mul > 0) and decides on the device: if at least
 * PNRF_NERF_SKIP_DEAD_PERCENT percent of the call's samples are dead, the MLP runs over the compacted list and a compositing pass follows (LIST); otherwise the
 * fused kernel runs as ever (DENSE).  rgbd is the same bit for bit either way; the host reads nothing back and the call still captures into a graph.  The
 * path's workspace, 160 bytes per ray of max_rays, is allocated by pnrf_ctx_set_nerf_skip or by the context's first call on the path outside a stream capture;
 * a call inside a capture that finds none, and a call of 2^28 rays or more (the list holds int32 column ids), run the fused kernel alone.
 *   PNRF_NERF_SKIP_NEVER   the fused kernel alone, no extra launch
 *   PNRF_NERF_SKIP_AUTO    (a new context) that path for calls of more than PNRF_NERF_SKIP_MIN_RAYS rays — one wide NeRF batch per CU on 256 CUs; below that
 *                          a call's time is the latency of one batch and two more launches would only add to it
 *   PNRF_NERF_SKIP_ALWAYS  that path and LIST whatever the call size or the dead share (tests, A/B timing)
 * Handles on PNRF_VARIANT_NERF_4X64 / PNRF_VARIANT_BF16_32X32 always run the fused kernel alone. */
#define PNRF_NERF_SKIP_NEVER 0
#define PNRF_NERF_SKIP_AUTO 1
#define PNRF_NERF_SKIP_ALWAYS 2
#define PNRF_NERF_SKIP_MIN_RAYS 8192
#define PNRF_NERF_SKIP_DEAD_PERCENT 2      /* break-even, measured: (list builder 0.019 + compositing pass 0.031 + empty launch 0.005 ms) / dense stage 3.29 ms = 1.7 %, rounded up; DESIGN 4.10 */
int pnrf_ctx_set_nerf_skip(pnrf_ctx_t* ctx, int mode);
/* The most recent pnrf_render_rays_fwd of the context: live columns the builder counted (-1 if the call did not take that path) and whether it chose
 * LIST (1) or DENSE (0) (waits for the device; diagnostics). */
int pnrf_ctx_nerf_live(pnrf_ctx_t* ctx, int64_t* live_columns, int* list_mode);
/* Per-stage device time of pnrf_render_rays_fwd (what the reference gets from line_profiler / the cuda events around
 * render(), run_S_eS_eN_alter_trt.py:327-332, at frame granularity): after _begin, the next max_frames calls on this
 * context record an event before and after each of the three kernels on the caller's stream; _end waits for the last
 * recorded call and returns the mean milliseconds ms[3] = {sampler, projection + refine, NeRF + compositing}
 * over *frames calls.  Recording costs four event records per call and changes no result. */
int pnrf_ctx_profile_begin(pnrf_ctx_t* ctx, int max_frames);
int pnrf_ctx_profile_end(pnrf_ctx_t* ctx, float* ms, int* frames);

/* ---- stage-2 training step --------------------------------------------------
 * fp32 storage and accumulation throughout, like the reference's training.  Every stage is a kernel of this library: the layer
 * products carry bias + activation (forward) and the activation derivative of the layer below (backward) in their epilogues and
 * multiply either in split fp16 (default: both operands as hi + 2^-11 lo fp16 pairs, 22 significand bits, three fp16 MFMAs per
 * block, gradients scaled by a power of two from their recorded maximum) or in exact fp32 on v_mfma_f32_16x16x4_f32
 * (pnrf_trainer_set_products).  From 8192 sample rows on the fine net runs as two launches on the fused-MLP engine of the inference
 * path — forward pts0 .. feature, views with every activation saved once; backward the ten input-gradient products with per-row
 * scaled fp16 planes — and the 256-wide weight gradients of all three nets as one grouped launch per iteration; below that, and
 * for the 4096-row sampler / refine nets, a layer's products are launches or 16-row layer chains.  The 1-4 wide heads, sort,
 * interval refinement, jitter, encodings, compositing, losses and Adam are per-ray / streaming kernels. */

/* Operator-level backward passes (each mirrors what torch.autograd derives for the forward it names). */
/* raw2outputs backward for d rgb_map [n,3]: arguments as pnrf_composite_fwd; outputs d_raw dev [n,s,4], d_z dev [n,s] (NULL to
 * skip), d_add / d_mul dev [n,s] (NULL to skip).  Any s >= 1 (a wave per ray, a lane per sample, two recurrences in sample order).
 * (run_S_eS_eN_alter_base_refine2.py:475-522) */
int pnrf_composite_bwd(const float* raw, const float* z, const float* rays_d, int d_stride, const float* add,
                       const float* mul, const float* noise, float clamp, int white_bkgd, const float* d_rgb,
                       float* d_raw, float* d_z, float* d_add, float* d_mul, int64_t n, int s, void* stream);
/* raw2outputs backward for the cotangents of ALL its outputs and of z itself: d_rgb dev [n,3], d_disp / d_acc / d_depth dev [n],
 * d_weights dev [n,s], d_z_in dev [n,s] (a cotangent z receives from elsewhere; added into d_z, which must then be given).  Each
 * may be NULL (= zeros), not all of them.  Inputs and outputs as pnrf_composite_bwd.  With w_s = alpha_s T_s the cotangent of w_s
 * is  g_rgb . c_s - [white] sum g_rgb + G_depth z_s + G_acc + d_weights[s],  d_z[s] gains  w_s G_depth + d_z_in[s], and
 * disp = 1 / max(1e-10, depth / acc) folds into the ray scalars: with r = depth / acc finite and > 1e-10,
 * G_depth = d_depth - d_disp disp^2 / acc and G_acc = d_acc + d_disp disp^2 depth / acc^2; otherwise (the constant branch of the
 * max, or acc == 0) d_disp contributes exact zeros — a deviation from autograd, which gives NaN at acc == 0.  depth and acc are
 * summed again in pnrf_composite_fwd's order, so the branch is the one the forward took.  With d_rgb alone the call is
 * pnrf_composite_bwd (the same launch: bit-identical).  Any s >= 1. */
int pnrf_composite_bwd_maps(const float* raw, const float* z, const float* rays_d, int d_stride, const float* add,
                            const float* mul, const float* noise, float clamp, int white_bkgd, const float* d_rgb,
                            const float* d_disp, const float* d_acc, const float* d_weights, const float* d_depth,
                            const float* d_z_in, float* d_raw, float* d_z, float* d_add, float* d_mul, int64_t n, int s,
                            void* stream);
/* Embedder.embed backward: d_x[n,3] from d_out[n, 3+6*n_freq] (run_nerf_helpers.py:666-671).  n_freq 0..16; at x = 0 the result
 * is exactly d_out[c] + sum_k 2^k d_out[sin_k] (tests/test_exact_heads_gpu.py pins it there, and forward and backward elsewhere
 * within a per-element bound, past the grid cap included). */
int pnrf_posenc_bwd(const float* x, const float* d_out, float* d_x, int64_t n, int n_freq, void* stream);
/* Sampler head on the raw output y dev [n,27] of MinMaxRay_Net: depth = sigmoid(y[0:8]) (far-near)+near, stable ascending
 * sort, add / mul gathered by the sort indices, mm_rgb = sigmoid(y[24:27]) (NULL to skip)
 * (run_S_eS_eN_alter_base_refine2.py:557-568); the backward scatters through sort_idx.
 * Forward: tied depths keep their index order; a NaN depth still gives a permutation of 0..7 in sort_idx, at an unspecified
 * place, and stays in its ray. */
int pnrf_sampler_head_fwd(const float* y, const float* rays, float* depth_sorted, int64_t* sort_idx, float* add_sorted,
                          float* mul_sorted, float* mm_rgb, int64_t n, void* stream);
/* Backward: sort_idx as the forward wrote it (ties included); d_mm_rgb NULL gives exact zeros in d_y[:, 24:27]. */
int pnrf_sampler_head_bwd(const float* y, const float* rays, const int64_t* sort_idx, const float* d_depth_sorted,
                          const float* d_add_sorted, const float* d_mul_sorted, const float* d_mm_rgb, float* d_y,
                          int64_t n, void* stream);
/* Refine head on the raw output y dev [n,35]: refine = sigmoid(y[0:8]), offsets = tanh(y[8:32]), rgb0 = sigmoid(y[32:35])
 * (NULL to skip); interval refinement, depth jitter (jitter dev [n,8] or NULL, jitter_dir +-1), query points
 * pts dev [n,8,3] = o + d z + 0.01 offsets; z_pre dev [n,8] = depths before the jitter (input of the backward)
 * (run_S_eS_eN_alter_base_refine2.py:635-668).  Backward: d_pts dev [n,8,3], d_z dev [n,8] or NULL, d_rgb0 dev [n,3] or
 * NULL -> d_y dev [n,35], d_depth_sorted dev [n,8].
 * Forward: depth_sorted need not be sorted (the formulas are applied to whatever order it holds); a NaN stays in its ray. */
int pnrf_refine_head_fwd(const float* y, const float* rays, const float* depth_sorted, const float* jitter,
                         int jitter_dir, float* z_pre, float* z, float* pts, float* rgb0, int64_t n, void* stream);
/* Backward: depth_sorted need not be sorted either: |z_pre - neighbour| is differentiated by the sign it has (0 at a tie, as
 * torch's abs); d_z NULL counts as zeros, d_rgb0 NULL gives exact zeros in d_y[:, 32:35]. */
int pnrf_refine_head_bwd(const float* y, const float* rays, const float* depth_sorted, const float* z_pre,
                         const float* jitter, int jitter_dir, const float* d_pts, const float* d_z,
                         const float* d_rgb0, float* d_y, float* d_depth_sorted, int64_t n, void* stream);

/* Trainer: fp32 parameters, gradients, Adam moments and workspaces of the three networks for batches of up to max_rays
 * rays.  26 Linear layers in this order: sampler fc_backbone.0..5, fc_output (MinMaxRay_Net, 288 -> 27); refine net
 * likewise (144 -> 35); fine net of class NeRF: pts_linears.0..7, feature_linear, alpha_linear, views_linears.0, rgb_linear.
 * W[i]: [out_dim[i], in_dim[i]] row-major (torch layout), host or device.  max_samples: samples per ray the NeRF-side
 * workspaces are sized for (8; stage-1 exploration: up to 256).
 * Replaces create_nerf's modules + torch.optim.Adam (run_S_eS_eN_alter_base_refine2.py:337-395). */
int pnrf_trainer_create(const float* const* W, const float* const* b, const int* in_dim, const int* out_dim,
                        int n_layers, int64_t max_rays, int max_samples, pnrf_trainer_t** out);
int pnrf_trainer_free(pnrf_trainer_t* t);
/* Weight-gradient kernel of the square layers: tile 0 = chosen by shape and row count (default), 64 / 128 = forced where the shape allows;
 * min_rows_128 = row count from which the 128 x 128-tile kernel is used (0 = default).  tile 256 / 255 (round 5) leave that choice alone and switch
 * the 256 x 128-tile form of the grouped split-fp16 gradients on from min_rows_128 rows (0: from the first row) / off; default: from 32 768 rows.
 * The two choices are independent: tile 0 / 64 / 128 do not touch the wide-tile threshold either.  Configuration, not on the step path. */
int pnrf_trainer_set_dw_kernel(pnrf_trainer_t* t, int tile, int64_t min_rows_128);
/* Diagnostics of the most recent iteration's grouped weight-gradient launch: number of gradients it held and which of them (bit k = k-th) ran on
 * the 256 x 128 tiles.  Host state; lets a test assert that the tile shape it forced is the one that ran. */
int pnrf_trainer_dw_group_info(const pnrf_trainer_t* t, int* n_jobs, unsigned* wide_mask);

/* kind 0 parameters, 1 gradients, 2 / 3 Adam first / second moment of the joint optimizer, 4 / 5 those of the NeRF-only
 * optimizer; W, b: host or device (NULL to skip). */
int pnrf_trainer_read(const pnrf_trainer_t* t, int kind, int layer, float* W, float* b, void* stream);
int pnrf_trainer_write(pnrf_trainer_t* t, int kind, int layer, const float* W, const float* b, void* stream);
int pnrf_trainer_set_step(pnrf_trainer_t* t, int64_t step, int64_t step_nerf);
/* Device address / element count of a flat array (kind as above): layers contiguous in trainer order, each [W, b] padded to 4
 * floats.  For in-place collectives over data-parallel replicas (RCCL all-reduce of the gradients). */
int pnrf_trainer_flat(pnrf_trainer_t* t, int kind, float** ptr, int64_t* count);
/* Trainer -> renderable nets without leaving the device: pnrf_mlp_repack of each non-NULL handle from the trainer's own parameters (sampler: trainer
 * layers 0-6, refine: 7-13, fine: 14-25 = the NeRF class in pack order pts0..7, feature, alpha, views, rgb), on `stream`.  Reads only: trainer state is
 * not changed, and the call may stand between pnrf_train_stage2_fwd and _bwd.  A handle of another kind or shape (fine: anything but PNRF_NET_NERFCLS)
 * is refused as by pnrf_mlp_repack, before anything is launched for any of the three.  Ordering against training steps and renders: stream order. */
int pnrf_trainer_publish(const pnrf_trainer_t* t, pnrf_mlp_t* sampler, pnrf_mlp_t* refine, pnrf_mlp_t* fine, void* stream);

typedef struct pnrf_train_batch {
  const float* rays;       /* dev [n,11] NDC ray batch (o, d, near, far, viewdir) */
  const float* or_rays;    /* dev [n,11] world-space rays */
  const float* target;     /* dev [n,3] ground-truth colours */
  const float* img4;       /* dev [nv,Hf,Wf,4] training views (pnrf_images_pack) */
  const float* poses;      /* dev [nv,3,4] camera-to-world */
  const float* K;          /* dev [3,3] */
  const int64_t* ref_nos;  /* dev [n,4] source views of each ray (the reference's random neighbour draw, made explicit) */
  const float* jitter;     /* dev [n,8] = min(|N(0,1)|/5, 1-2e-6) or NULL */
  const float* raw_noise;  /* dev [n,8] = randn * raw_noise_std or NULL */
  int64_t n;
  int nv, Hf, Wf;
  int jitter_dir;          /* +1 toward the next sample / far, -1 toward the previous / near */
  int white_bkgd;
  float eps;               /* NDC -> metric epsilon: 1e-5 */
  float a_mmrgb;           /* weight of mse(rgb_map0) + mse(mm_rgb) in the loss (0 in fern_refine.txt; 1 on stage-1 even iterations) */
  float clamp;             /* raw clamp before compositing: 0 = none (stage 2), 10 (stage 1, base.py:523) */
  int layout;              /* epi feature layout: 0 neighbour-major (stage 2), 1 sample-major (stage 1) */
} pnrf_train_batch_t;

/* Joint iteration: render_rays (training) + img2mse [+ a_mmrgb (...)] + loss.backward(): leaves the gradients of all 26
 * layers in the trainer.  loss dev [4] = {total, mse(rgb_map1), mse(rgb_map0), mse(mm_rgb)}; rgb_map1 dev [n,3] or NULL.
 * Stage 2 (run_S_eS_eN_alter_base_refine2.py:525-680, 858-868) and, with layout 1 / eps 1e-6 / clamp 10 / a_mmrgb 1 / no
 * jitter and noise, the even iterations of stage 1 (run_S_eS_eN_alter_base.py:554-761, 941-958). */
int pnrf_train_stage2_fwd_bwd(pnrf_trainer_t* t, const pnrf_train_batch_t* batch, float* loss, float* rgb_map1,
                              void* stream);
/* Odd iterations of stage 1 (run_S_eS_eN_alter_base.py:929-940, exploration :689-729): sampler / refine nets without
 * gradient, refined depths explored into 8 n_mult samples (replicated toward dir1, jittered toward batch->jitter_dir with
 * batch->jitter dev [n, 8 n_mult]), no offsets, compositing without add / mul with batch->raw_noise dev [n, 8 n_mult];
 * loss = img2mse(rgb_map1); gradients for the 12 NeRF layers only. */
int pnrf_train_explore_fwd_bwd(pnrf_trainer_t* t, const pnrf_train_batch_t* batch, int n_mult, int dir1, float* loss,
                               float* rgb_map1, void* stream);
/* The joint iteration in two calls, for a loss of the caller's between them.  Every map is dev fp32; any pointer may be NULL.
 * rgb_map1 / rgb_map0 / mm_rgb [n,3]: composited, refine-head and sampler-head colours; depth / acc / disp [n] and
 * weights [n,8]: the other outputs of raw2outputs; z [n,8]: the refined, jittered sample depths the compositing used. */
typedef struct pnrf_train_maps {
  float *rgb_map1, *rgb_map0, *mm_rgb, *depth, *acc, *disp, *weights, *z;
} pnrf_train_maps_t;
typedef struct pnrf_train_cotangents {
  const float *d_rgb_map1, *d_rgb_map0, *d_mm_rgb, *d_depth, *d_acc, *d_disp, *d_weights, *d_z;
} pnrf_train_cotangents_t;
/* Forward half of pnrf_train_stage2_fwd_bwd: the same launches up to and including the compositing (which here also writes
 * disp, acc and depth), then the requested maps are copied out.  batch->target may be NULL and batch->a_mmrgb is ignored: the
 * loss is the caller's.  Stage-1 even iterations: layout 1, eps 1e-6, clamp 10. */
int pnrf_train_stage2_fwd(pnrf_trainer_t* t, const pnrf_train_batch_t* batch, const pnrf_train_maps_t* out, void* stream);
/* Backward half, from the caller's cotangents of the maps (NULL = zeros; all NULL: PNRF_E_ARG), read in place: compositing
 * backward for every map (pnrf_composite_bwd_maps; d_z enters there), the fine net, the refine head (d_rgb_map0), the refine
 * net, the sampler head (d_mm_rgb), the sampler net.  Leaves the gradients of all 26 layers where the fused call leaves them
 * (pnrf_trainer_read / _flat / _adam_step as after it); with d_rgb_map1 [, d_rgb_map0, d_mm_rgb] alone they are the fused
 * call's, bit for bit.  It reads the batch copy the forward half staged in the trainer.
 * State: valid only as the NEXT trainer call after a pnrf_train_stage2_fwd, on the same stream.  After any other iteration,
 * pnrf_trainer_net_fwd_bwd, _adam_step, _write, _set_products, _set_dw_kernel or a first pnrf_train_stage2_bwd it returns
 * PNRF_E_STATE, decided on the host before anything is launched.
 * Both calls launch kernel by kernel whatever pnrf_trainer_set_graph says (a captured graph would hold the caller's pointers). */
int pnrf_train_stage2_bwd(pnrf_trainer_t* t, const pnrf_train_cotangents_t* cotangents, void* stream);
/* y = net(x); y.backward(dy) for ONE of the trainer's three nets, through the dispatch of the iterations (preparation launch, product kind,
 * weight-gradient tile choice, engine / chain / per-layer path chosen by row count, grouped weight-gradient launch).  Overwrites that net's
 * layer gradients only (kind 1 of pnrf_trainer_read).  Test-facing: the output gradient is the caller's, not the losses'.
 * net 0 sampler: x dev [n,288], dy / y dev [n,27];  net 1 refine: x dev [n,144], dy / y dev [n,35]  (S, rays unused: 0 / NULL; d_pts NULL);
 * net 2 fine net (NeRF class): x = pts dev [n*S,3], rays dev [n,11] (view directions at 8:11, repeated S times), 1 <= S <= max_samples,
 *       dy = d raw dev [n*S,4], y = raw dev [n*S,4], d_pts dev [n*S,3] (n*S <= 8 max_rays) or NULL (the exploration's branch without
 *       position gradient).  n in [1, max_rays] for every net. */
int pnrf_trainer_net_fwd_bwd(pnrf_trainer_t* t, int net, const float* x, const float* rays, int64_t n, int S, const float* dy,
                             float* y, float* d_pts, void* stream);
/* Both iteration entry points copy the batch into buffers of the trainer with one launch; with pnrf_trainer_set_graph(t, 1) they then replay
 * their ~100-kernel launch sequence as a hipGraph (captured from the given stream — the legacy default stream is served through a stream of
 * the trainer's own — the first time a configuration (ray count, views, flags, stream) is seen; up to 8 configurations are kept).  Default
 * 0: the kernels are launched one by one (same results bit for bit; measured slightly faster). */
int pnrf_trainer_set_graph(pnrf_trainer_t* t, int enable);
/* Arithmetic of the layer products X W^T and dZ W.  kind 0 (default): split-fp16 MFMA — both operands as hi + 2^-11 lo fp16 pairs (22
   significand bits), three fp16 MFMAs per product block, fp32 accumulation; gradients are scaled by a power of two taken from their
   recorded maximum before the split.  kind 1: exact-fp32 MFMA products everywhere (the reference trains in fp32; torch's fp32 GEMMs are
   this).  From 8192 rows on kind 0 runs the fine net on the fused-MLP engine of the inference path: forward (pts0 .. pts7, feature_linear,
   views_linear) and backward (their input gradients) as ONE launch each — 128 rows per workgroup stay in registers through the layers, the
   weights stream through LDS once per 128 rows, each activation / gradient is written once, ReLU derivatives travel as bit masks — and the
   weight gradients as one grouped launch (same split-fp16 arithmetic, the engine's contraction order and per-row gradient scales: fp32
   round-off apart from the per-layer products).  kind 2: one product launch per layer; kind 3: pts1-4 and pts6, pts7, feature forward as two
   64-row layer chains (kinds 2 and 3: bit-identical to each other; kept for A/B timing and tests).  The narrow heads (fewer than 64 output
   columns) always use the fp32 kernel. */
int pnrf_trainer_set_products(pnrf_trainer_t* t, int kind);
/* optimizer.step() of torch.optim.Adam (L2 weight decay added to the gradient).  which 0: the joint optimizer over all
 * parameters (run_S_eS_eN_alter_base_refine2.py:394, 869; stage 1 s_optimizer); which 1: the NeRF-only optimizer of stage 1
 * (run_S_eS_eN_alter_base.py:398-421, 940) with its own moments and step count. */
int pnrf_trainer_adam_step(pnrf_trainer_t* t, int which, float lr, float beta1, float beta2, float eps,
                           float weight_decay, void* stream);

/* ---- frame tail: image metrics and 8-bit output ------------------------------------------------
 * What render_path does with a finished frame (run_S_eS_eN_alter_trt.py:350-362: PSNR against the ground truth, to8b, depth / max(depth),
 * PNG) and the SSIM the method is reported with (run_nerf_helpers.py:151-197), on the device: the frame never travels as fp32.
 *
 * img2mse + img2ssim of two H x W x 3 images in one call (run_nerf_helpers.py:129, 151-197).  pred, gt: dev fp32, pixel (y, x) channel c at
 * [(y W + x) stride + c] with the image's own pixel stride in floats (>= 3): 3 reads an [H,W,3] image, 4 the rgbd[n,4] rows of
 * pnrf_render_rays_fwd.  taps: HOST [T], the 1-D filter (run_nerf_helpers.py:163-167 evaluated in float64, rounded to fp32), 1 <= T <= 16,
 * applied as a convolution along y and along x with 'valid' windows (:170-175): the SSIM map has (H - T + 1) x (W - T + 1) x 3 values.
 * Arithmetic of :176-196 in fp32: five filtered moments per channel (of the images minus max_val / 2: variances do not see the shift, the
 * means get it back), variances clamped at 0, covariance limited to sign(s01) min(sqrt(s00 s11), |s01|), c1 = (k1 max_val)^2,
 * c2 = (k2 max_val)^2, the quotient.  One workgroup per 32 x 32 output tile and channel (both input tiles with their halo in LDS, a pass
 * along x into LDS, a pass along y from it), per-workgroup partial sums in fp64 into the workspace, summed in a fixed order by a second
 * small kernel: no atomics, results bit-identical from call to call on any stream.
 * out: dev double[4] = {sum (pred - gt)^2 over the H W 3 values, that / (H W 3) (img2mse), sum of the SSIM map, its mean (img2ssim)}.
 * ssim_map: dev fp32 [H-T+1, W-T+1, 3] or NULL.  workspace: dev, 8-byte aligned, >= pnrf_image_metrics_workspace_bytes(H, W, T) bytes
 * (0 for sizes the call refuses), contents irrelevant; concurrent calls need separate workspaces.  H < T, W < T, T outside 1 .. 16, a
 * null pointer or a stride below 3 return PNRF_E_ARG. */
int64_t pnrf_image_metrics_workspace_bytes(int H, int W, int T);
int pnrf_image_metrics_fwd(const float* pred, int pred_stride, const float* gt, int gt_stride, int H, int W,
                           const float* taps, int T, float max_val, float k1, float k2, double* out,
                           float* ssim_map, void* workspace, int64_t workspace_bytes, void* stream);
/* img2ssim as a training loss: the mean SSIM of B patch pairs of H x W x 3 and its gradient with respect to the prediction, in two launches.
 * pred, gt: dev fp32, patch b pixel (y, x) channel c at [b patch_stride + (y W + x) stride + c]: a pixel stride in floats (>= 3) per operand as
 * above, and a patch stride in floats (>= 0; 0 reads one patch B times) per operand.  taps: HOST [T], 1 <= T <= 16, H >= T, W >= T;
 * 1 <= B <= 21845 (a patch and channel per grid z).  The forward arithmetic is that of pnrf_image_metrics_fwd, one kernel text for both: for
 * B = 1 the mean has the bits of that call's out[3].
 * out: dev double[2] = {sum of the SSIM map over all B (H-T+1) (W-T+1) 3 values, its mean}.  d_pred: dev fp32 [B,H,W,3], dense =
 * d mean / d pred.  The loss 1 - mean, its weight and the sign are the caller's.
 * Gradient: with x' = pred - max_val / 2, y' = gt - max_val / 2 and the window's filter weights w, every window and channel gives
 * w_p (a + 2 b x'_p + e y'_p) to its pixel p:  b = dS/ds00 through the clamp (zero unless s00 > 0);  e = dS/ds01 through the limiter (dS/dc
 * where |s01| <= sqrt(v0 v1); otherwise 0, and b gains sign(s01) 1/2 sqrt(v1 / v0) dS/dc where v0 > 0);  a = dS/dmu0 (direct) - 2 m0 b - m1 e
 * with the means m0, m1 of x', y'.  The first pass (the metrics kernel's tiling) writes a, b, e per window into the workspace; the second is
 * the transposed separable convolution of the three planes as a gather per pixel, 32 x 32 pixels per workgroup, patch and channel:
 * d_pred[p] = (F^T[a] + 2 x'_p F^T[b] + y'_p F^T[e]) / (B (H-T+1) (W-T+1) 3); its first workgroup adds the fp64 partial sums in a fixed order.
 * No atomics: value and gradient are bit-identical from call to call on any stream.
 * Deviation from autograd, exactly ON a kink only: torch.maximum / minimum split the gradient between equal operands; here s00 == 0 takes
 * b = 0 and |s01| == sqrt(v0 v1) counts as the limiter being inactive.  A NaN reaches the windows, and the pixels, that contain it — no others.
 * workspace: dev, 8-byte aligned, >= pnrf_ssim_loss_workspace_bytes(B, H, W, T) bytes (0 for sizes the call refuses), contents irrelevant;
 * concurrent calls need separate workspaces.  Everything outside the limits above returns PNRF_E_ARG before any launch. */
int64_t pnrf_ssim_loss_workspace_bytes(int B, int H, int W, int T);
int pnrf_ssim_loss_fwd(const float* pred, int pred_stride, int64_t pred_patch_stride, const float* gt, int gt_stride,
                       int64_t gt_patch_stride, int B, int H, int W, const float* taps, int T, float max_val, float k1,
                       float k2, double* out, float* d_pred, void* workspace, int64_t workspace_bytes, void* stream);
/* to8b of a frame (run_nerf_helpers.py:135; run_S_eS_eN_alter_trt.py:356, 360): rgb8[n,3] = to8b(rgb), depth8[n] = to8b(depth / max(depth)),
 * uint8, bit-identical to numpy for finite input — 255 * clip(x, 0, 1) is one fp32 product, truncated; the quotient is one correctly
 * rounded fp32 division by the maximum, which a first kernel takes on the device.  rgb: dev, pixel i at [i rgb_stride + c], rgb_stride >= 3;
 * depth: dev, pixel i at [i depth_stride], depth_stride >= 1 (rgbd[n,4]: rgb = rgbd, depth = rgbd + 3, both strides 4).  Either output
 * may be NULL (then its input may be too), not both.  workspace: dev, 4-byte aligned, >= PNRF_TO8B_WORKSPACE_BYTES (needed with depth8).
 * Not finite input: NaN -> 0, +Inf -> 255, -Inf -> 0; the maximum skips NaN depths, and a quotient that is NaN (Inf / Inf, 0 / 0) -> 0. */
#define PNRF_TO8B_WORKSPACE_BYTES 4096
int pnrf_frame_to8b_fwd(const float* rgb, int rgb_stride, const float* depth, int depth_stride, int64_t n,
                        uint8_t* rgb8, uint8_t* depth8, void* workspace, int64_t workspace_bytes, void* stream);
/* An 8-bit plane as the bytes of a PNG file (csrc/pnrf_png_rules.h states the format rules once, for the host twin and the kernels).
 * img: H rows of W pixels of `channels` bytes (1: gray, 3: RGB), row y at img + y row_stride, row_stride in bytes >= W channels: the planes of
 * pnrf_frame_to8b_fwd as they stand.  filter: -1 adaptive (per row the type with the smallest sum of |residual as a signed byte|, ties to the lowest
 * type), 0 .. 4 that type on every row.  The file: signature, IHDR (8 bit, colour type 0 or 2, no interlace), one IDAT, IEND.  The IDAT's zlib stream
 * is coded in independent segments of pnrf_png_segment_rows() rows of filtered bytes: literals and distance-1 matches of 3 .. 258 bytes, one dynamic
 * Huffman block (code lengths from the segment's histogram, at most 15 bits) or stored blocks where those are smaller, and behind every segment but
 * the last an empty stored block (00 00 FF FF after padding).  Adler-32 and CRC-32 are taken per piece and combined.  Deterministic: the same pixels
 * give the same bytes from pnrf_png_encode_host, from pnrf_png_encode_fwd, on any stream.
 * pnrf_png_max_bytes: an upper bound of the file for any content (raw + 5 raw / 65535 + 10 segments + 63 with raw = H (W channels + 1));
 * pnrf_png_workspace_bytes: the device workspace of pnrf_png_encode_fwd; both 0 for sizes the calls refuse.
 * pnrf_png_encode_host: HOST pointers, plain C++: the twin the device bytes are held to.  size: HOST, receives the file's length.
 * pnrf_png_encode_fwd: dev pointers, four launches in stream order, nothing allocated or read back, capturable in a graph.  out receives the
 * file, size_dev (dev int64, 8-byte aligned) its length.  workspace: dev, 16-byte aligned, >= pnrf_png_workspace_bytes, contents irrelevant;
 * concurrent calls need separate workspaces.
 * PNRF_E_ARG before any launch: H or W < 1, H W > 2^28, channels not 1 or 3, filter outside -1 .. 4, row_stride < W channels,
 * capacity < pnrf_png_max_bytes, a workspace that is too small or misaligned, a null pointer. */
int pnrf_png_segment_rows(void);
int64_t pnrf_png_max_bytes(int H, int W, int channels);
int64_t pnrf_png_workspace_bytes(int H, int W, int channels);
int pnrf_png_encode_host(const uint8_t* img_host, int64_t row_stride, int H, int W, int channels, int filter,
                         uint8_t* out_host, int64_t capacity, int64_t* size);
int pnrf_png_encode_fwd(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int filter,
                        uint8_t* out, int64_t capacity, int64_t* size_dev, void* workspace, int64_t workspace_bytes,
                        void* stream);
/* An 8-bit plane as the bytes of a baseline JPEG file (csrc/pnrf_jpeg_rules.h states the format rules once, for the host twin and the kernels).
 * img as for pnrf_png_encode_fwd: 1 channel is coded as one gray component, 3 as Y, Cb, Cr (JFIF full-range BT.601 in 16-bit fixed point) without
 * subsampling, one block of each per MCU.  quality 1 .. 100: the Annex K tables in the IJG library's scaling, entries 1 .. 255.  The file: SOI, APP0
 * (JFIF 1.01), DQT, SOF0, DHT (the Annex K.3 tables as they stand), DRI, SOS, entropy data, EOI.  Right and bottom edges are padded to a multiple of 8
 * by replication; the forward DCT is the 13-bit scaled integer form with 32-bit intermediates; quantisation divides rounding half away from zero.
 * Every MCU row is one restart interval (DRI = ceil(W / 8)), coded on its own: DC predictions start at 0, the last byte is filled with 1-bits, RSTm
 * (m = row mod 8) follows every interval but the last; every FF byte of entropy data is followed by 00.  Deterministic: the same pixels give the same
 * bytes from pnrf_jpeg_encode_host, from pnrf_jpeg_encode_fwd, on any stream.
 * pnrf_jpeg_max_bytes: an upper bound of the file for any content: header (330 gray, 613 colour) + ceil(H / 8) (2 ceil(1660 blocks / 8) + 2) + 2 with
 * blocks = ceil(W / 8) channels a row, 1660 = 22 DC bits + 63 x 26 AC bits, doubled for stuffing, 2 for RSTm;
 * pnrf_jpeg_workspace_bytes: the device workspace of pnrf_jpeg_encode_fwd; both 0 for sizes the calls refuse.
 * pnrf_jpeg_encode_host: HOST pointers, plain C++: the twin the device bytes are held to.  size: HOST, receives the file's length.
 * pnrf_jpeg_encode_fwd: dev pointers, four launches in stream order, nothing allocated or read back, capturable in a graph.  out receives the
 * file, size_dev (dev int64, 8-byte aligned) its length.  workspace: dev, 16-byte aligned, >= pnrf_jpeg_workspace_bytes, contents irrelevant;
 * concurrent calls need separate workspaces.
 * PNRF_E_ARG before any launch: H or W outside 1 .. 65535, channels not 1 or 3, quality outside 1 .. 100, row_stride < W channels,
 * capacity < pnrf_jpeg_max_bytes, a workspace that is too small or misaligned, a null pointer. */
int64_t pnrf_jpeg_max_bytes(int H, int W, int channels);
int64_t pnrf_jpeg_workspace_bytes(int H, int W, int channels);
int pnrf_jpeg_encode_host(const uint8_t* img_host, int64_t row_stride, int H, int W, int channels, int quality,
                          uint8_t* out_host, int64_t capacity, int64_t* size);
int pnrf_jpeg_encode_fwd(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int quality,
                         uint8_t* out, int64_t capacity, int64_t* size_dev, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ---- LPIPS (version 0.1) of an image pair: AlexNet / VGG-16 feature stacks and the metric ---------------------
 * The third number the method is reported with (run_nerf_helpers.py:137-149: rgb_lpips, nets 'alex' and 'vgg').  The weights are the caller's:
 * the backbone's convolutions and the five 1 x 1 'lin' layers; nothing is fetched from anywhere.
 * Definition.  Two H x W x 3 images a, b; with normalize x <- 2 x - 1; then (x - shift) / scale per channel, shift = (-.030, -.088, -.188),
 * scale = (.458, .448, .450).  Five taps F_k (ReLU outputs):
 *   alex: conv(3->64, k 11, stride 4, pad 2) | maxpool(3, 2) conv(64->192, k 5, pad 2) | maxpool(3, 2) conv(192->384, k 3, pad 1) |
 *         conv(384->256, k 3, pad 1) | conv(256->256, k 3, pad 1), a tap behind each;
 *   vgg:  thirteen conv(k 3, pad 1) of widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512, maxpool(2, 2) between the groups, a
 *         tap behind the last layer of each group.
 * Pooling has no padding and floor sizes.  Per tap and pixel n(F) = F / (sqrt(sum_c F_c^2) + 1e-10),
 * m_k[y,x] = sum_c lin_k[c] (n(F_k(a)) - n(F_k(b)))_c^2, and d = sum_k mean_yx m_k.  Sides: alex 31 .. PNRF_LPIPS_MAX_DIM (the second pool needs a
 * 3 x 3 input), vgg 16 .. PNRF_LPIPS_MAX_DIM.
 * Arithmetic: every convolution is an implicit GEMM on the exact-fp32 MFMA (fp32 products and range, sums in (ky, kx, c_in) order), the pair as a
 * batch of two; the tap sums are fp32 per pixel and fp64 over pixels, per-workgroup partial sums added in a fixed order by a last small kernel:
 * no atomics, results bit-identical from call to call on any stream; d(x, x) is exactly 0 and d(a, b) has the bits of d(b, a).
 *
 * pnrf_lpips_create: net "alex" or "vgg" (anything else: PNRF_E_ARG).  conv_w[n_conv], conv_b[n_conv]: pointers to fp32 [out,in,kh,kw] / [out]
 * (torch layout), on the host or on a device; conv_shape: HOST int[n_conv][4] = the shapes of conv_w; lin_w[5]: pointers to fp32 [C_k];
 * lin_dim: HOST int[5].  Every shape is checked against the net's table before any device work (PNRF_E_SHAPE; the message lists the table).  The
 * weights are repacked once, [K][C_out], on the current device. */
#define PNRF_LPIPS_MAX_DIM 4096
typedef struct pnrf_lpips pnrf_lpips_t;
int pnrf_lpips_create(const char* net, const float* const* conv_w, const float* const* conv_b, const int* conv_shape, int n_conv,
                      const float* const* lin_w, const int* lin_dim, pnrf_lpips_t** out);
int pnrf_lpips_free(pnrf_lpips_t* h);
/* Host only: hw = HOST int[5][2], the rows and columns of the five tap planes of an H x W image.  PNRF_E_ARG for an unknown net or a side outside
 * the limits above. */
int pnrf_lpips_tap_dims(const char* net, int H, int W, int* hw);
/* Bytes of workspace pnrf_lpips_fwd needs at H x W: two activation buffers and the partial sums.  0 for sizes the call refuses. */
int64_t pnrf_lpips_workspace_bytes(const pnrf_lpips_t* h, int H, int W);
/* a, b: dev fp32, pixel (y, x) channel c at [(y W + x) stride + c], pixel strides in floats >= 3 as pnrf_image_metrics_fwd (4 reads rgbd rows in
 * place).  out: dev double[6] = {d, mean m_1 .. mean m_5}.  maps: dev fp32, the five m_k planes concatenated (sizes: pnrf_lpips_tap_dims), or NULL.
 * workspace: dev, 16-byte aligned, >= pnrf_lpips_workspace_bytes(h, H, W) bytes, contents irrelevant; concurrent calls need separate workspaces.
 * Nothing is allocated and nothing is read back: the call is capturable in a hipGraph.  A null pointer, a stride below 3 or a size outside the
 * limits return PNRF_E_ARG before any launch. */
int pnrf_lpips_fwd(const pnrf_lpips_t* h, const float* a, int a_stride, const float* b, int b_stride, int H, int W, int normalize,
                   double* out, float* maps, void* workspace, int64_t workspace_bytes, void* stream);
/* For tests: conv layer `layer` of the handle — with pool_first its preceding max pooling, then conv, bias, ReLU — on a dense NHWC pair
 * x: dev fp32 [2,H,W,C_in] -> y: dev fp32 [2,OH,OW,C_out], with the very kernels pnrf_lpips_fwd runs (layer 0: its gather without the input
 * scaling).  pool_first on a layer without a pooling in front, an input smaller than the window / filter, x (hidden layers) or y not 16-byte
 * aligned: PNRF_E_ARG.  workspace: >= pnrf_lpips_layer_workspace_bytes bytes (layer 0: the gathered rows; pool_first: the pooled pair; else 0
 * and the pointer may be NULL). */
int64_t pnrf_lpips_layer_workspace_bytes(const pnrf_lpips_t* h, int layer, int pool_first, int H, int W);
int pnrf_lpips_layer_fwd(const pnrf_lpips_t* h, int layer, int pool_first, const float* x, int H, int W, float* y, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* LPIPS as a training loss: the mean d of B patch pairs of H x W x 3 and its gradient with respect to the prediction.
 * pred, gt: dev fp32, patch b pixel (y, x) channel c at [b patch_stride + (y W + x) stride + c], strides as pnrf_ssim_loss_fwd (pixel stride >= 3
 * floats; patch stride >= 0, 0 reads one patch B times).  Sides as pnrf_lpips_fwd (alex >= 31, vgg >= 16, <= PNRF_LPIPS_MAX_DIM), B >= 1, and
 * 2 B H W <= 2^31 - 1 (the kernels' pixel index).
 * Definition: that of pnrf_lpips_fwd per pair.  The B pairs run as one batch of 2 B images [pred_0 .. pred_{B-1}, gt_0 .. gt_{B-1}];
 * out: dev double[6] = {mean over the patches of d, the five tap means over patches and pixels}.  On numbers the forward arithmetic is that of
 * pnrf_lpips_fwd: for B = 1 the six numbers have that call's bits.  A NaN in a patch is kept (the loss's own conv and pooling kernels: ReLU and
 * maximum as torch takes them), so the value is NaN; the metric's kernels drop it.
 * d_pred: dev fp32 [B,H,W,3], dense = d out[0] / d pred.  The weight and the sign are the caller's.
 * Backward, pred half only, top layer down, with omega_k = 1 / (B h_k w_k), F the pred features of a tap pixel, s = sqrt(sum_c F_c^2),
 * na = F / (s + 1e-10), nb likewise from gt:  r_c = 2 omega_k lin_c (na - nb)_c,  dF_c = (r_c - na_c (sum_j r_j F_j) / s) / (s + 1e-10), sums over the
 * channels as a butterfly over the wave; it is added to the gradient arriving from the layers above.  ReLU: dz = dy [y > 0].  Convolutions with
 * C_in >= 64: dX = dZ * flip(W)^T as an implicit GEMM on the exact-fp32 MFMA, sums in (k-1-ky, k-1-kx, c_out) order — with few pixels (at most 32 workgroups of 64 pixels x 64 channels) one chain per filter tap and the taps' sums
 * added in tap order by a second kernel, a function of the shape alone; first layers: per input value a
 * gather over the outputs whose window covers it, one fmaf chain in (oy, ox, c_out) order, then x 2 / scale_c (normalize) or 1 / scale_c.
 * Max pooling: per input element a gather over the windows that hold it, in row-major order.
 * Kink rules.  ReLU: y == 0 gives 0, as torch.  Tap: at s == 0 the second term of dF is taken as 0 (float64 autograd gives NaN from sqrt'(0)); the
 * ReLU mask zeroes that pixel anyway.  Tie rule of the pooling: the gradient of a window goes to the first element attaining its maximum in
 * (ky, kx) order, as torch's CPU kernel; elements in the rows / columns that the floor sizes drop get exactly 0.
 * No atomics, one writer per element, every sum in a fixed order: value and gradient are bit-identical from call to call on any stream; patches
 * do not see each other (a NaN in one stays in its gradient, and reaches the value).  pred == gt gives exactly 0 and a gradient of exactly 0.
 * workspace: dev, 16-byte aligned, >= pnrf_lpips_loss_workspace_bytes(h, B, H, W) bytes (every conv output of the batch, two gradient buffers, the
 * partial sums), contents irrelevant; concurrent calls need separate workspaces.  The first pnrf_lpips_loss_workspace_bytes (or
 * pnrf_lpips_layer_bwd_workspace_bytes) on a handle packs its weights a second time for the data gradient, [k k C_out][C_in] flipped (one device
 * allocation, waited for): make it outside a stream capture; a handle used for the metric alone never pays it.  pnrf_lpips_loss_fwd itself
 * allocates nothing and reads nothing back: it is capturable in a hipGraph.  Everything outside the limits above, a null pointer or a short
 * workspace return PNRF_E_ARG before any launch, and pnrf_lpips_loss_workspace_bytes returns 0 for such sizes. */
int64_t pnrf_lpips_loss_workspace_bytes(const pnrf_lpips_t* h, int B, int H, int W);
int pnrf_lpips_loss_fwd(const pnrf_lpips_t* h, const float* pred, int pred_stride, int64_t pred_patch_stride, const float* gt, int gt_stride,
                        int64_t gt_patch_stride, int B, int H, int W, int normalize, double* out, float* d_pred, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* For tests: the backward of conv layer `layer` — with pool_first its preceding max pooling in front — on n images, by the kernels the loss runs.
 * x: dev fp32 [n,H,W,C_in] the saved input (the pooling's input with pool_first), y: [n,OH,OW,C_out] the saved output (after ReLU), dy: its
 * gradient, all dense NHWC and 16-byte aligned -> dx [n,H,W,C_in] = pooling gather(data gradient(dy [y > 0])); layer 0: lpips_dgrad0_kernel
 * without the input scaling.  The first mask is a kernel of this entry point alone (in the loss the kernel that writes a gradient applies it);
 * relu_in != 0 (hidden layers): dx is also multiplied by [x > 0] in the data gradient's epilogue / the pooling gather, as the loss does it.
 * workspace: >= pnrf_lpips_layer_bwd_workspace_bytes bytes (0 for what the call refuses). */
int64_t pnrf_lpips_layer_bwd_workspace_bytes(const pnrf_lpips_t* h, int layer, int pool_first, int n, int H, int W);
int pnrf_lpips_layer_bwd(const pnrf_lpips_t* h, int layer, int pool_first, int relu_in, int n, const float* x, int H, int W, const float* y,
                         const float* dy, float* dx, void* workspace, int64_t workspace_bytes, void* stream);
/* For tests: the tap backward alone.  f_pred, f_gt: dev fp32 [P, C_tap] features of P = n h w tap pixels (omega = 1 / P) -> d_f [P, C_tap] =
 * dF [F > 0], F = f_pred: the gradient with respect to the pre-activation, as the loss stores it. */
int pnrf_lpips_tap_bwd(const pnrf_lpips_t* h, int tap, const float* f_pred, const float* f_gt, int64_t P, float* d_f, void* stream);

/* ---- device-resident scene: a frame from a camera pose alone ---------------------------------------
 * What render_path does per pose on the host (run_S_eS_eN_alter_trt.py:245-302: rank the source cameras, fetch / permute / upload the neighbour
 * images, build the projection matrices, build the rays) from a scene that lives on the device.  The source views are fixed, so they are uploaded
 * once; per target pose only O(views) arithmetic and one copy of the nb selected images remain, all of it kernels of this library reading the pose
 * from DEVICE memory: no host read-back, no allocation, capturable in a hipGraph that is replayed with twelve floats changed.
 *
 * A scene holds nv source views of Hf x Wf pixels: the texel cache [nv,Hf,Wf,4] (PNRF_SCENE_F32: float4 texels, exact for any image;
 * PNRF_SCENE_U8: RGBA8 texels, a quarter of the memory, for 8-bit sources), their camera-to-world poses [nv,3,4] and two 3 x 3 intrinsics.
 * 1 <= nv <= 4096.  pnrf_scene_create validates and does NO device work; the device arrays (one allocation) are made on the current device by the
 * first pnrf_scene_set_view / pnrf_scene_set_intrinsics, and the scene then belongs to that device (PNRF_E_STATE from another one).  A scene is
 * configuration like a packed network: set every view and the intrinsics, then use it; the forward calls do not change it. */
#define PNRF_SCENE_F32 0
#define PNRF_SCENE_U8 1
#define PNRF_IMG_F32 0
#define PNRF_IMG_U8 1
int pnrf_scene_create(int nv, int Hf, int Wf, int format, pnrf_scene_t** out);
int pnrf_scene_free(pnrf_scene_t* s);
/* Source view v: img dev [Hf,Wf,pix_stride], fp32 (PNRF_IMG_F32) or uint8 (PNRF_IMG_U8), pix_stride 3 or 4 values per pixel of which the first three
 * are taken (an [H,W,3] image as loaded, no permute) -> the view's texels (r, g, b, 0).  uint8 -> fp32 is one correctly rounded fp32 division k / 255:
 * the 256 values of (k / 255.).astype(float32), what load_llff produces (load_llff.py).  A PNRF_SCENE_U8 cache takes uint8 images only — an fp32 image
 * is refused (PNRF_E_ARG), never quantised silently.  pose_host: HOST [3,4] camera-to-world, 12 finite floats; it travels in the ingest kernel's
 * arguments, so both the image and the pose are read in stream order and the host buffer is free when the call returns.  Arguments are checked
 * before any device work. */
int pnrf_scene_set_view(pnrf_scene_t* s, int v, const void* img, int img_dtype, int pix_stride, const float* pose_host, void* stream);
/* The driver's K (target camera: rays) and ref_K (source cameras: projection), HOST [3,3] each, finite.  Synchronous copy; configuration. */
int pnrf_scene_set_intrinsics(pnrf_scene_t* s, const float* K_target_host, const float* K_ref_host);
/* Neighbour selection for the target pose c2w dev [3,4] (run_S_eS_eN_alter_trt.py:281-296), two launches:
 *   ranking     d_v = sqrt((dx dx + dy dy) + dz dz) of the camera centres in fp32, every operation rounded once; stable ascending rank (ties to the
 *               lower index, NaN last: np.argsort(kind='stable')); ref_nos_out dev int32 [nb] = the nb nearest views — pronerf_amd.render.select_neighbors
 *               index for index.  One workgroup ranks by counting over the distances in LDS (O(nv^2) comparisons: microseconds for tens of views).
 *   projection  proj_out dev [nb,3,4], proj[k] = K_ref . diag(1,-1,-1) . pose[ref_nos[k]]: the fp32 x fp32 products are exact in fp64, each three-term sum
 *               is formed left to right in fp64 and rounded once to fp32 — independent of FMA contraction, reproducible with element-wise float64
 *               numpy.  NOT the bits of an fp32 matmul (render.projection_matrices): both lie within 4 x 2^-24 (|K| . |diag . pose|) of the exact product.
 *   gather      img4_out dev [nb,Hf,Wf,4] (16-byte aligned), img4_out[k] = float4(cache[ref_nos[k]]): what pnrf_images_pack makes of the selected images,
 *               bit for bit; ref_nos is read from device memory.
 * nb 1 .. 8, at most nv (PNRF_E_ARG); every view and the intrinsics must have been set (PNRF_E_STATE). */
int pnrf_scene_select_fwd(const pnrf_scene_t* s, const float* c2w_dev, int nb, int32_t* ref_nos_out, float* proj_out, float* img4_out, void* stream);
/* pnrf_frame_rays_blocks_fwd with the camera in device memory: K_dev dev [3,3], c2w_dev dev [3,4].  Same per-pixel code (csrc/pnrf_frame_rays.h), the
 * double-precision NDC scale evaluated on the device: output bit-identical to the host-pointer entry point. */
int pnrf_frame_rays_dev_fwd(const float* K_dev, const float* c2w_dev, int H, int W, float near, float far, float or_near, float or_far,
                            int64_t first, int64_t block, int64_t stride, int64_t count, float* rays, float* or_rays, void* stream);
/* Pose -> rows of the frame on one stream: pnrf_scene_select_fwd, pnrf_frame_rays_dev_fwd with the scene's K_target, pnrf_render_rays_fwd — three
 * launches (select, gather, rays) in front of that call's own, nothing allocated, nothing read back.  rgbd dev [count,4], sort_idx optional; first / block / stride / count as
 * pnrf_frame_rays_blocks_fwd (a whole frame: 0, H W, 0, H W); count <= the context's max_rays.  ws: dev, 16-byte aligned, ws_bytes >=
 * pnrf_render_pose_workspace_bytes(scene, nb, count) — it holds ref_nos, proj, img4, rays and or_rays of the call; contents irrelevant, concurrent calls
 * need separate workspaces (and contexts). */
int pnrf_render_pose_workspace_bytes(const pnrf_scene_t* s, int nb, int64_t max_rays, int64_t* bytes);
int pnrf_render_pose_fwd(pnrf_ctx_t* ctx, const pnrf_scene_t* s, const float* c2w_dev, int nb, int H, int W, float near, float far, float or_near,
                         float or_far, int64_t first, int64_t block, int64_t stride, int64_t count, float eps, void* ws, int64_t ws_bytes,
                         float* rgbd, int64_t* sort_idx, void* stream);

/* ---- device-resident training set: a batch from ray indices alone ------------------------------------
 * What the training drivers do per iteration on the host side (run_S_eS_eN_alter_base_refine2.py / ..._base.py: three row gathers out of per-pixel
 * arrays of every training view, a fancy-index chain for ref_nos, a host-to-device copy of the neighbour draw, the jitter / noise kernels) from a
 * PNRF_SCENE_F32 scene of the training views.  Ray g of the training set is view g / (Hf Wf), pixel g % (Hf Wf).
 *
 * Device addresses of a COMPLETE PNRF_SCENE_F32 scene (any output may be NULL): img4 [nv,Hf,Wf,4] — bit for bit what pnrf_images_pack makes of the
 * views, so it is pnrf_train_batch_t.img4 as it stands — poses [nv,3,4], K_target [3,3], K_ref [3,3].  Valid until pnrf_scene_free.  PNRF_E_STATE if a
 * view or the intrinsics are missing; PNRF_E_ARG for a PNRF_SCENE_U8 scene (the trainer reads fp32 texels). */
int pnrf_scene_arrays(const pnrf_scene_t* s, const float** img4, const float** poses, const float** K_target, const float** K_ref);
/* rank dev int32 [nv,nv]: row c = the views in stable ascending order of their distance to view c — the ranking of pnrf_scene_select_fwd (one shared
 * device function: same arithmetic, ties to the lower index, NaN last) with view c's camera centre as the target, one workgroup per row; equal to
 * neighbor_rank_table of the stage-2 driver index for index (rank[c][0] is c itself unless another view shares its position). */
int pnrf_scene_rank_table_fwd(const pnrf_scene_t* s, int32_t* rank, void* stream);
/* The batch of the n rays idx dev int64 [n], at most two launches, nothing allocated, nothing read back; all outputs dev, caller-owned:
 *   rays, or_rays [n,11]  the rows pnrf_frame_rays_fwd writes for (K_target, pose of the ray's view, Hf, Wf, near, far, or_near, or_far) at the ray's
 *                         pixel, bit for bit (the shared per-pixel body, csrc/pnrf_frame_rays.h, with a per-row camera)
 *   target [n,3]          the texel's r, g, b, copied
 *   ref_nos int64 [n,4]   rank[view][1 + order[k]]; order: HOST int[4], 0 <= order[k] < nv - 1 (the driver's sorted random.sample; it travels in the
 *                         kernel arguments); rank: the table above (entries are clamped into 0 .. nv - 1 when read)
 *   jitter [n,jitter_cols] = fminf(|z| / 5, jitter_cap), noise [n,noise_cols] = z noise_std, z ~ N(0,1); NULL skips the draw; columns: multiples of
 *                         4 up to 256; 16-byte aligned.
 * An idx outside [0, nv Hf Wf) reads nothing out of range: its row gets NaN rays and target, ref_nos 0, and bad_rows (dev int64, optional) is
 * incremented once per such row (atomicAdd; the caller zeroes it).
 * Draws: Philox4x32-10 (pnrf_philox4x32_10 below), key = (seed low word, seed high word); the quad q = (row0 + row) (C / 4) + k of an array with C
 * columns takes counter (q low, q high, step, stream), stream 0 = jitter, 1 = noise, and fills columns 4k .. 4k + 3 of its row: word x -> u =
 * (2 (x >> 9) + 1) 2^-24 (exact, inside (0, 1)); words (0, 1) and (2, 3) each give r = sqrt(-2 logf(u0)), (r cospi(2 u1), r sinpi(2 u1)), accurate
 * library functions.  row0: the batch row of the caller's first row (a data-parallel replica passes replica n_local: the union of the replicas'
 * draws does not depend on the world size).  Deterministic in (seed, step, row); not torch's stream.
 * Checked before any device work (PNRF_E_ARG): nv < 5, order out of range, n < 0, a null required pointer, bad column counts. */
int pnrf_train_batch_fwd(const pnrf_scene_t* s, const int32_t* rank, const int64_t* idx, int64_t n, const int* order, float near, float far,
                         float or_near, float or_far, float* rays, float* or_rays, float* target, int64_t* ref_nos, int64_t* bad_rows,
                         uint64_t seed, uint32_t step, int64_t row0, float* jitter, int jitter_cols, float jitter_cap, float* noise,
                         int noise_cols, float noise_std, void* stream);
/* Host helper: one Philox4x32-10 block (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), the code the draws above run.
 * counter HOST [4], key HOST [2], out HOST [4].  counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8. */
int pnrf_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* Host helper: torch.linspace(start,end,n) in fp32, as used for the 48 ray points
 * (run_S_eS_eN_alter_trt.py:556-557).  out: HOST [n]. */
int pnrf_linspace(float start, float end, int n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PRONERF_HIP_H */
