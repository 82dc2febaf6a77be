// pnrf_scene.hip — the device-resident scene: the source views of a scene uploaded once (texel cache [nv,Hf,Wf,4], poses, intrinsics), and everything
// that depends on the TARGET pose computed on the device from a [3,4] matrix in device memory: neighbour ranking, projection matrices, the [nb,Hf,Wf,4]
// texel block the refine stage reads, the rays (pnrf_scene_select_fwd, pnrf_frame_rays_dev_fwd) — and pnrf_render_pose_fwd, which chains them in front of
// pnrf_render_rays_fwd on one stream.  No call here reads anything back or allocates on the render path, so a pose-to-frame call captures into a hipGraph
// that is replayed with twelve floats changed.  Streaming kernels, no MFMA; the fused-MLP units are untouched.
#include <math.h>

#include <vector>

#include "pnrf_common.h"
#include "pnrf_frame_rays.h"
#include "pnrf_scene_impl.h"

using namespace pnrf;

namespace {

constexpr int TPB = SCENE_TPB;
constexpr int MAX_VIEWS = SCENE_MAX_VIEWS;           // the ranking kernel keeps one distance per view in LDS (16 KiB)
constexpr int SCENE_MAX_NB = 8;
inline int grid_for(int64_t work) {
  int64_t g = (work + TPB - 1) / TPB;
  const int64_t cap = 256 * 16;           // 256 CUs x 16 blocks, grid-stride the rest
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
inline int64_t texel_bytes(int format) { return format == PNRF_SCENE_U8 ? 4 : 16; }
inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// uint8 -> fp32 as load_llff does it, (k / 255.).astype(float32): one correctly rounded fp32 division gives the same 256 values (tests/test_scene_cpu.py)
__device__ __forceinline__ float u8_to_f32(unsigned k) { return ieee_div((float)k, 255.f); }

struct PoseArg { float p[12]; };

// One source image [Hf,Wf,pix_stride] (fp32 or uint8, 3 or 4 values per pixel, the first three taken) -> the view's texels in the cache; the pose rides in
// the kernel arguments and is written by the first twelve threads: no host copy is in flight after the call returns.
__global__ void scene_ingest_kernel(const void* __restrict__ src, int src_u8, int pix_stride, void* __restrict__ dst, int dst_u8, int64_t plane, PoseArg pose,
                                    float* __restrict__ pose_dst) {
  if (blockIdx.x == 0 && threadIdx.x < 12) {
    float v = pose.p[0];
#pragma unroll
    for (int e = 1; e < 12; ++e) v = (int)threadIdx.x == e ? pose.p[e] : v;
    pose_dst[threadIdx.x] = v;
  }
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < plane; q += (int64_t)gridDim.x * blockDim.x) {
    if (src_u8) {
      const uint8_t* s = (const uint8_t*)src + q * pix_stride;
      const unsigned r = s[0], g = s[1], b = s[2];
      if (dst_u8) ((uchar4*)dst)[q] = make_uchar4((unsigned char)r, (unsigned char)g, (unsigned char)b, 0);
      else ((float4*)dst)[q] = make_float4(u8_to_f32(r), u8_to_f32(g), u8_to_f32(b), 0.f);
    } else {
      const float* s = (const float*)src + q * pix_stride;
      ((float4*)dst)[q] = make_float4(s[0], s[1], s[2], 0.f);
    }
  }
}

// Neighbour ranking + projection matrices of one target pose: ONE workgroup.
//   distances and stable ascending ranks as scene_rank_views states them (pnrf_scene_impl.h; shared with the training set's rank table); the views of
//   rank < nb go to ref_nos[rank].
//   proj[k] = K_ref . diag(1,-1,-1) . pose[ref_nos[k]]: fp32 x fp32 products are exact in fp64, the left-to-right three-term sum is formed in fp64 and
//   rounded once to fp32 — the same bits with or without FMA contraction.
__global__ __launch_bounds__(TPB) void scene_select_kernel(const float* __restrict__ poses, int nv, const float* __restrict__ c2w, const float* __restrict__ Kref,
                                                           int nb, int* __restrict__ ref_nos, float* __restrict__ proj) {
  __shared__ float sd[MAX_VIEWS];
  __shared__ int ssel[SCENE_MAX_NB];
  const int tid = threadIdx.x;
  scene_rank_views(poses, nv, c2w[3], c2w[7], c2w[11], sd, [&](int v, int rank) {
    if (rank < nb) { ssel[rank] = v; ref_nos[rank] = v; }        // the ranks are a permutation of 0 .. nv - 1 and nb <= nv: every slot is written once
  });
  __syncthreads();
  if (tid < nb * 12) {
    const int k = tid / 12, e = tid - k * 12, r = e >> 2, c = e & 3;
    const float* p = poses + (int64_t)ssel[k] * 12;
    const double a0 = (double)Kref[r * 3] * (double)p[c];
    const double a1 = (double)Kref[r * 3 + 1] * (double)(-p[4 + c]);
    const double a2 = (double)Kref[r * 3 + 2] * (double)(-p[8 + c]);
    proj[tid] = (float)((a0 + a1) + a2);
  }
}

// img4_out[k] = float4(cache[ref_nos[k]]): ref_nos is read from device memory (written by scene_select_kernel earlier on the stream), one 16-byte store per
// texel.  F32 cache: a copy; U8 cache: the RGBA8 texel expanded as the ingest would have.
template <bool U8>
__global__ void scene_gather_kernel(const void* __restrict__ cache, const int* __restrict__ ref_nos, int nv, int nb, int64_t plane, float4* __restrict__ out) {
  const int64_t total = (int64_t)nb * plane;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(q / plane);
    const int64_t i = q - (int64_t)k * plane;
    int v = ref_nos[k];
    v = v < 0 ? 0 : (v >= nv ? nv - 1 : v);          // never leaves the cache, whatever the buffer holds
    const int64_t s = (int64_t)v * plane + i;
    if (U8) {
      const uchar4 t = ((const uchar4*)cache)[s];
      out[q] = make_float4(u8_to_f32(t.x), u8_to_f32(t.y), u8_to_f32(t.z), 0.f);
    } else {
      out[q] = ((const float4*)cache)[s];
    }
  }
}

// pnrf_frame_rays_blocks_fwd's kernel with the camera read from device memory: the per-pixel body is the shared one (pnrf_frame_rays.h), the double-precision
// NDC scale is evaluated here instead of on the host (IEEE fp64 division and conversion on both sides: the same bits).
__global__ void frame_rays_dev_kernel(FrameArgs a, const float* __restrict__ K, const float* __restrict__ c2w, float* __restrict__ rays,
                                      float* __restrict__ or_rays) {
  a.K00 = K[0]; a.K02 = K[2]; a.K11 = K[4]; a.K12 = K[5];
  a.sx = ndc_scale(a.W, a.K00); a.sy = ndc_scale(a.H, a.K00);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.R[r * 3 + c] = c2w[r * 4 + c];
    a.T[r] = c2w[r * 4 + 3];
  }
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < a.count; q += (int64_t)gridDim.x * blockDim.x)
    frame_ray_row(a, q, rays, or_rays);
}

bool all_finite(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Device arrays of a scene, allocated by the first call that needs them (pnrf_scene_create itself does no device work).
int ensure_device(pnrf_scene* s) {
  int cur = -1;
  PNRF_HIP(hipGetDevice(&cur));
  if (s->device >= 0) {
    PNRF_REQUIRE(cur == s->device, PNRF_E_STATE, "pnrf_scene: the scene lives on device %d, the calling thread's current device is %d", s->device, cur);
    return 0;
  }
  const size_t cache_bytes = (size_t)s->nv * s->Hf * s->Wf * (size_t)texel_bytes(s->format);
  const size_t pose_bytes = (size_t)up256((int64_t)s->nv * 12 * sizeof(float));
  char* base = nullptr;
  hipError_t e = hipMalloc((void**)&base, (size_t)up256((int64_t)cache_bytes) + pose_bytes + 256);      // one allocation: cache, poses, the two 3 x 3 matrices
  if (e != hipSuccess) {
    if (base) (void)hipFree(base);
    set_error("pnrf_scene: allocating %zu bytes for %d views of %d x %d failed: %s", cache_bytes, s->nv, s->Hf, s->Wf, hipGetErrorString(e));
    return (int)e;
  }
  s->cache = base;
  s->poses = (float*)(base + up256((int64_t)cache_bytes));
  s->K = (float*)(base + up256((int64_t)cache_bytes) + pose_bytes);
  s->device = cur;
  return 0;
}

// Workspace of pnrf_render_pose_fwd: ref_nos | proj | img4 | rays | or_rays, each part on a 256-byte boundary.
struct PoseWs { int64_t ref_nos, proj, img4, rays, or_rays, total; };
PoseWs pose_ws(const pnrf_scene* s, int nb, int64_t max_rays) {
  PoseWs w;
  w.ref_nos = 0;
  w.proj = 256;
  w.img4 = w.proj + 512;                                         // 8 x 12 floats
  w.rays = w.img4 + up256((int64_t)nb * s->Hf * s->Wf * 16);
  w.or_rays = w.rays + up256(max_rays * 11 * (int64_t)sizeof(float));
  w.total = w.or_rays + up256(max_rays * 11 * (int64_t)sizeof(float));
  return w;
}

int check_select(const char* who, const pnrf_scene* s, int nb) {
  PNRF_REQUIRE(s, PNRF_E_ARG, "%s: null scene", who);
  PNRF_REQUIRE(nb >= 1 && nb <= SCENE_MAX_NB && nb <= s->nv, PNRF_E_ARG, "%s: nb must be 1 .. %d and at most the scene's %d views, got %d", who, SCENE_MAX_NB, s->nv, nb);
  PNRF_REQUIRE(s->n_have == s->nv && s->have_K, PNRF_E_STATE, "%s: the scene is not complete (%d of %d views set, intrinsics %s)", who, s->n_have, s->nv,
               s->have_K ? "set" : "missing");
  return 0;
}

int launch_select(const pnrf_scene* s, const float* c2w_dev, int nb, int* ref_nos, float* proj, float* img4, hipStream_t st) {
  hipLaunchKernelGGL(scene_select_kernel, dim3(1), dim3(TPB), 0, st, s->poses, s->nv, c2w_dev, s->K + 9, nb, ref_nos, proj);
  PNRF_LAUNCH_CHECK();
  const int64_t plane = (int64_t)s->Hf * s->Wf;
  if (s->format == PNRF_SCENE_U8)
    hipLaunchKernelGGL(scene_gather_kernel<true>, dim3(grid_for(nb * plane)), dim3(TPB), 0, st, s->cache, ref_nos, s->nv, nb, plane, (float4*)img4);
  else
    hipLaunchKernelGGL(scene_gather_kernel<false>, dim3(grid_for(nb * plane)), dim3(TPB), 0, st, s->cache, ref_nos, s->nv, nb, plane, (float4*)img4);
  PNRF_LAUNCH_CHECK();
  return 0;
}

int launch_rays(const float* K_dev, const float* c2w_dev, int H, int W, float near, float far, float or_near, float or_far, int64_t first, int64_t block,
                int64_t stride, int64_t count, float* rays, float* or_rays, hipStream_t st) {
  FrameArgs a = {};
  a.H = H; a.W = W; a.near = near; a.far = far; a.or_near = or_near; a.or_far = or_far; a.first = first; a.count = count; a.block = block; a.stride = stride;
  hipLaunchKernelGGL(frame_rays_dev_kernel, dim3(grid_for(count)), dim3(TPB), 0, st, a, K_dev, c2w_dev, rays, or_rays);
  PNRF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
extern "C" int pnrf_scene_create(int nv, int Hf, int Wf, int format, pnrf_scene_t** out) {
  PNRF_REQUIRE(out, PNRF_E_ARG, "pnrf_scene_create: null output");
  *out = nullptr;
  PNRF_REQUIRE(nv >= 1 && nv <= MAX_VIEWS, PNRF_E_ARG, "pnrf_scene_create: 1 .. %d source views, got %d", MAX_VIEWS, nv);
  PNRF_REQUIRE(Hf >= 1 && Wf >= 1 && (int64_t)Hf * Wf <= ((int64_t)1 << 31) - 1, PNRF_E_ARG, "pnrf_scene_create: bad image size %d x %d", Hf, Wf);
  PNRF_REQUIRE(format == PNRF_SCENE_F32 || format == PNRF_SCENE_U8, PNRF_E_ARG, "pnrf_scene_create: format must be PNRF_SCENE_F32 or PNRF_SCENE_U8, got %d", format);
  pnrf_scene* s = new pnrf_scene();
  s->nv = nv; s->Hf = Hf; s->Wf = Wf; s->format = format; s->device = -1;
  s->cache = nullptr; s->poses = nullptr; s->K = nullptr;
  s->have.assign((size_t)nv, 0); s->n_have = 0; s->have_K = false;
  *out = s;
  return 0;
}

extern "C" int pnrf_scene_free(pnrf_scene_t* s) {
  if (!s) return 0;
  if (s->cache) (void)hipFree(s->cache);
  delete s;
  return 0;
}

extern "C" int pnrf_scene_set_view(pnrf_scene_t* s, int v, const void* img, int img_dtype, int pix_stride, const float* pose_host, void* stream) {
  PNRF_REQUIRE(s, PNRF_E_ARG, "pnrf_scene_set_view: null scene");
  PNRF_REQUIRE(v >= 0 && v < s->nv, PNRF_E_ARG, "pnrf_scene_set_view: view %d outside 0 .. %d", v, s->nv - 1);
  PNRF_REQUIRE(img_dtype == PNRF_IMG_F32 || img_dtype == PNRF_IMG_U8, PNRF_E_ARG, "pnrf_scene_set_view: img_dtype must be PNRF_IMG_F32 or PNRF_IMG_U8, got %d", img_dtype);
  PNRF_REQUIRE(pix_stride == 3 || pix_stride == 4, PNRF_E_ARG, "pnrf_scene_set_view: pix_stride must be 3 or 4, got %d", pix_stride);
  PNRF_REQUIRE(!(s->format == PNRF_SCENE_U8 && img_dtype != PNRF_IMG_U8), PNRF_E_ARG,
               "pnrf_scene_set_view: a PNRF_SCENE_U8 cache takes uint8 images only (an fp32 image would be quantised; use PNRF_SCENE_F32)");
  PNRF_REQUIRE(img && pose_host, PNRF_E_ARG, "pnrf_scene_set_view: null pointer");
  PNRF_REQUIRE(img_dtype == PNRF_IMG_U8 || ((uintptr_t)img & 3) == 0, PNRF_E_ARG, "pnrf_scene_set_view: an fp32 image must be 4-byte aligned");
  PNRF_REQUIRE(all_finite(pose_host, 12), PNRF_E_ARG, "pnrf_scene_set_view: the pose of view %d is not finite", v);
  int rc = ensure_device(s);
  if (rc) return rc;
  PoseArg pa;
  for (int i = 0; i < 12; ++i) pa.p[i] = pose_host[i];
  const int64_t plane = (int64_t)s->Hf * s->Wf;
  void* dst = (char*)s->cache + (int64_t)v * plane * texel_bytes(s->format);
  hipLaunchKernelGGL(scene_ingest_kernel, dim3(grid_for(plane)), dim3(TPB), 0, (hipStream_t)stream, img, img_dtype == PNRF_IMG_U8 ? 1 : 0, pix_stride, dst,
                     s->format == PNRF_SCENE_U8 ? 1 : 0, plane, pa, s->poses + (int64_t)v * 12);
  PNRF_LAUNCH_CHECK();
  if (!s->have[(size_t)v]) { s->have[(size_t)v] = 1; s->n_have += 1; }
  return 0;
}

extern "C" int pnrf_scene_set_intrinsics(pnrf_scene_t* s, const float* K_target_host, const float* K_ref_host) {
  PNRF_REQUIRE(s && K_target_host && K_ref_host, PNRF_E_ARG, "pnrf_scene_set_intrinsics: null argument");
  PNRF_REQUIRE(all_finite(K_target_host, 9) && all_finite(K_ref_host, 9), PNRF_E_ARG, "pnrf_scene_set_intrinsics: the matrices must be finite");
  int rc = ensure_device(s);
  if (rc) return rc;
  float both[18];
  for (int i = 0; i < 9; ++i) { both[i] = K_target_host[i]; both[9 + i] = K_ref_host[i]; }
  PNRF_HIP(hipMemcpy(s->K, both, sizeof(both), hipMemcpyHostToDevice));       // synchronous: configuration, not on the render path
  s->have_K = true;
  return 0;
}

extern "C" int pnrf_scene_select_fwd(const pnrf_scene_t* s, const float* c2w_dev, int nb, int32_t* ref_nos_out, float* proj_out, float* img4_out, void* stream) {
  int rc = check_select("pnrf_scene_select_fwd", s, nb);
  if (rc) return rc;
  PNRF_REQUIRE(c2w_dev && ref_nos_out && proj_out && img4_out, PNRF_E_ARG, "pnrf_scene_select_fwd: null pointer");
  PNRF_REQUIRE(((uintptr_t)img4_out & 15) == 0, PNRF_E_ARG, "pnrf_scene_select_fwd: img4_out must be 16-byte aligned");
  {
    int cur = -1;
    PNRF_HIP(hipGetDevice(&cur));
    PNRF_REQUIRE(cur == s->device, PNRF_E_STATE, "pnrf_scene_select_fwd: the scene lives on device %d, the calling thread's current device is %d", s->device, cur);
  }
  return launch_select(s, c2w_dev, nb, ref_nos_out, proj_out, img4_out, (hipStream_t)stream);
}

extern "C" int pnrf_frame_rays_dev_fwd(const float* K_dev, const float* c2w_dev, int H, int W, float near, float far, float or_near, float or_far,
                                       int64_t first, int64_t block, int64_t stride, int64_t count, float* rays, float* or_rays, void* stream) {
  int rc = frame_rays_check("pnrf_frame_rays_dev_fwd", H, W, first, block, stride, count);
  if (rc) return rc;
  if (count == 0) return 0;
  PNRF_REQUIRE(K_dev && c2w_dev && rays && or_rays, PNRF_E_ARG, "pnrf_frame_rays_dev_fwd: null pointer");
  return launch_rays(K_dev, c2w_dev, H, W, near, far, or_near, or_far, first, block, stride, count, rays, or_rays, (hipStream_t)stream);
}

extern "C" int pnrf_render_pose_workspace_bytes(const pnrf_scene_t* s, int nb, int64_t max_rays, int64_t* bytes) {
  PNRF_REQUIRE(s && bytes, PNRF_E_ARG, "pnrf_render_pose_workspace_bytes: null argument");
  PNRF_REQUIRE(nb >= 1 && nb <= SCENE_MAX_NB && nb <= s->nv && max_rays >= 0 && max_rays < ((int64_t)1 << 31), PNRF_E_ARG,
               "pnrf_render_pose_workspace_bytes: nb must be 1 .. %d and at most the scene's %d views, max_rays below 2^31 (got %d, %lld)", SCENE_MAX_NB, s->nv, nb,
               (long long)max_rays);
  *bytes = pose_ws(s, nb, max_rays).total;
  return 0;
}

extern "C" int pnrf_render_pose_fwd(pnrf_ctx_t* ctx, const pnrf_scene_t* s, const float* c2w_dev, int nb, int H, int W, float near, float far, float or_near,
                                    float or_far, int64_t first, int64_t block, int64_t stride, int64_t count, float eps, void* ws, int64_t ws_bytes,
                                    float* rgbd, int64_t* sort_idx, void* stream) {
  PNRF_REQUIRE(ctx, PNRF_E_ARG, "pnrf_render_pose_fwd: null context");
  int rc = check_select("pnrf_render_pose_fwd", s, nb);
  if (rc) return rc;
  if ((rc = frame_rays_check("pnrf_render_pose_fwd", H, W, first, block, stride, count))) return rc;
  if (count == 0) return 0;
  PNRF_REQUIRE(count < ((int64_t)1 << 31), PNRF_E_ARG, "pnrf_render_pose_fwd: at most 2^31 - 1 rays per call");
  PNRF_REQUIRE(s->Hf >= 2 && s->Wf >= 2, PNRF_E_ARG, "pnrf_render_pose_fwd: the projection needs source images of at least 2 x 2 pixels (the scene's are %d x %d)", s->Hf, s->Wf);
  PNRF_REQUIRE(c2w_dev && ws && rgbd, PNRF_E_ARG, "pnrf_render_pose_fwd: null pointer");
  const PoseWs w = pose_ws(s, nb, count);
  PNRF_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= w.total, PNRF_E_ARG,
               "pnrf_render_pose_fwd: the workspace must be 16-byte aligned and hold pnrf_render_pose_workspace_bytes(scene, %d, %lld) = %lld bytes (got %lld)", nb,
               (long long)count, (long long)w.total, (long long)ws_bytes);
  {
    int cur = -1;
    PNRF_HIP(hipGetDevice(&cur));
    PNRF_REQUIRE(cur == s->device, PNRF_E_STATE, "pnrf_render_pose_fwd: the scene lives on device %d, the calling thread's current device is %d", s->device, cur);
  }
  char* b = (char*)ws;
  int* ref_nos = (int*)(b + w.ref_nos);
  float* proj = (float*)(b + w.proj);
  float* img4 = (float*)(b + w.img4);
  float* rays = (float*)(b + w.rays);
  float* or_rays = (float*)(b + w.or_rays);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = launch_select(s, c2w_dev, nb, ref_nos, proj, img4, st))) return rc;                                                            // trt.py:281-296
  if ((rc = launch_rays(s->K, c2w_dev, H, W, near, far, or_near, or_far, first, block, stride, count, rays, or_rays, st))) return rc;        // :245-271
  return pnrf_render_rays_fwd(ctx, rays, or_rays, img4, proj, nb, s->Hf, s->Wf, eps, rgbd, sort_idx, count, stream);                       // :599-696
}
