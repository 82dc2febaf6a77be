// pnrf_batch.hip — the device-resident training set: a pnrf_train_batch_t from ray indices alone.  A training driver's batch is a pure function of the
// scene (views, poses, intrinsics) and a slice of the epoch's permutation; this unit computes it from a pnrf_scene_t instead of gathering it from
// per-pixel arrays expanded on the host: the rank table of the training cameras (pnrf_scene_rank_table_fwd, once per scene), then per iteration rays,
// or_rays, target and ref_nos of the indexed pixels in one launch and the jitter / sigma-noise draws of a counter-based generator in a second
// (pnrf_train_batch_fwd).  Nothing is allocated or read back.  Streaming kernels, no MFMA; pnrf_train.hip and the fused-MLP units are untouched.
#include <math.h>

#include "pnrf_common.h"
#include "pnrf_frame_rays.h"
#include "pnrf_philox.h"
#include "pnrf_scene_impl.h"

using namespace pnrf;

namespace {

constexpr int TPB = SCENE_TPB;
constexpr int MAX_DRAW_COLS = 256;
inline int grid_for(int64_t work) {
  int64_t g = (work + TPB - 1) / TPB;
  const int64_t cap = 256 * 16;           // 256 CUs x 16 blocks, grid-stride the rest
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Row c of the table: the views in stable ascending order of their distance to view c (neighbor_rank_table of the stage-2 driver).  One workgroup per row.
__global__ __launch_bounds__(TPB) void scene_rank_table_kernel(const float* __restrict__ poses, int nv, int32_t* __restrict__ rank) {
  __shared__ float sd[SCENE_MAX_VIEWS];
  const int c = blockIdx.x;
  const float* t = poses + (int64_t)c * 12;
  int32_t* row = rank + (int64_t)c * nv;
  scene_rank_views(poses, nv, t[3], t[7], t[11], sd, [&](int v, int r) { row[r] = v; });
}

struct OrderArg { int o[4]; };

// Row q of the batch from ray index g = idx[q]: view g / plane, pixel g % plane.  rays / or_rays: frame_ray_row with that view's pose as the camera (built
// as frame_rays_dev_kernel builds it: the same bits as pnrf_frame_rays_fwd); target: the texel; ref_nos: rank[view][1 + order[k]].  An index outside
// [0, nv plane) reads nothing: NaN rays and target, ref_nos 0, one count.
__global__ __launch_bounds__(TPB) void train_batch_rows_kernel(FrameArgs a, const float* __restrict__ K, const float* __restrict__ poses,
                                                               const float4* __restrict__ cache, const int32_t* __restrict__ rank, int nv, int64_t plane,
                                                               const int64_t* __restrict__ idx, int64_t n, OrderArg order, float* __restrict__ rays,
                                                               float* __restrict__ or_rays, float* __restrict__ target, int64_t* __restrict__ ref_nos,
                                                               unsigned long long* __restrict__ bad) {
  a.K00 = K[0]; a.K02 = K[2]; a.K11 = K[4]; a.K12 = K[5];
  a.sx = ndc_scale(a.W, a.K00); a.sy = ndc_scale(a.H, a.K00);
  a.block = 1; a.stride = 0;                                  // frame_ray_row(a, 0, ...): output row 0 of the pointers it is given, pixel a.first
  const int64_t total = (int64_t)nv * plane;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = idx[q];
    float* r = rays + q * 11;
    float* o = or_rays + q * 11;
    float* t = target + q * 3;
    int64_t* rn = ref_nos + q * 4;
    if (g < 0 || g >= total) {
      const float nan = __builtin_nanf("");
#pragma unroll
      for (int e = 0; e < 11; ++e) { r[e] = nan; o[e] = nan; }
      t[0] = nan; t[1] = nan; t[2] = nan;
      rn[0] = 0; rn[1] = 0; rn[2] = 0; rn[3] = 0;
      if (bad) atomicAdd(bad, 1ull);
      continue;
    }
    const int v = (int)(g / plane);
    a.first = g - (int64_t)v * plane;
    const float* c2w = poses + (int64_t)v * 12;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) a.R[rr * 3 + cc] = c2w[rr * 4 + cc];
      a.T[rr] = c2w[rr * 4 + 3];
    }
    frame_ray_row(a, 0, r, o);
    const float4 tx = cache[g];
    t[0] = tx.x; t[1] = tx.y; t[2] = tx.z;
    const int32_t* row = rank + (int64_t)v * nv + 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int s = row[order.o[k]];
      s = s < 0 ? 0 : (s >= nv ? nv - 1 : s);                 // whatever the caller's table holds, the trainer never leaves the views
      rn[k] = s;
    }
  }
}

struct DrawArgs {
  uint32_t key0, key1, step;
  int64_t row0, n;
  float* jitter; int qj; float cap;          // qj = Cj / 4 quads per row (0: no jitter)
  float* noise; int qn; float std;
};

// One Philox call per thread: four words -> four uniforms in (0, 1) -> two Box-Muller pairs -> columns 4k .. 4k + 3 of one row of the jitter (stream 0) or
// of the noise (stream 1).  The quad's counter depends on the GLOBAL row (row0 + row) alone, so a batch split over replicas draws the same values.
__global__ __launch_bounds__(TPB) void train_batch_draws_kernel(DrawArgs a) {
  const int64_t nj = a.n * a.qj, total = nj + a.n * a.qn;
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
    const bool is_noise = w >= nj;
    const int64_t l = is_noise ? w - nj : w;
    const int qc = is_noise ? a.qn : a.qj;
    const int64_t row = l / qc;
    const int k = (int)(l - row * qc);
    const uint64_t quad = (uint64_t)(a.row0 + row) * (uint64_t)qc + (uint64_t)k;
    uint32_t x[4];
    philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), a.step, is_noise ? 1u : 0u, a.key0, a.key1, x);
    float z[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u0 = philox_unit(x[2 * h]), u1 = philox_unit(x[2 * h + 1]);
      const float rad = ieee_sqrt(ieee_mul(-2.f, logf(u0)));
      float sn, cs;
      sincospif(ieee_mul(2.f, u1), &sn, &cs);
      z[2 * h] = ieee_mul(rad, cs);
      z[2 * h + 1] = ieee_mul(rad, sn);
    }
    float4 out;
    if (is_noise) {
      out = make_float4(ieee_mul(z[0], a.std), ieee_mul(z[1], a.std), ieee_mul(z[2], a.std), ieee_mul(z[3], a.std));
      ((float4*)a.noise)[l] = out;
    } else {
      out = make_float4(fminf(ieee_div(fabsf(z[0]), 5.f), a.cap), fminf(ieee_div(fabsf(z[1]), 5.f), a.cap), fminf(ieee_div(fabsf(z[2]), 5.f), a.cap),
                        fminf(ieee_div(fabsf(z[3]), 5.f), a.cap));
      ((float4*)a.jitter)[l] = out;
    }
  }
}

int check_scene(const char* who, const pnrf_scene* s) {
  PNRF_REQUIRE(s, PNRF_E_ARG, "%s: null scene", who);
  PNRF_REQUIRE(s->format == PNRF_SCENE_F32, PNRF_E_ARG, "%s: a training set is a PNRF_SCENE_F32 scene (the trainer reads fp32 texels)", who);
  PNRF_REQUIRE(s->n_have == s->nv && s->have_K, PNRF_E_STATE, "%s: the scene is not complete (%d of %d views set, intrinsics %s)", who, s->n_have, s->nv,
               s->have_K ? "set" : "missing");
  return 0;
}

int check_device(const char* who, const pnrf_scene* s) {
  int cur = -1;
  PNRF_HIP(hipGetDevice(&cur));
  PNRF_REQUIRE(cur == s->device, PNRF_E_STATE, "%s: the scene lives on device %d, the calling thread's current device is %d", who, s->device, cur);
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
extern "C" int pnrf_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  PNRF_REQUIRE(counter && key && out, PNRF_E_ARG, "pnrf_philox4x32_10: null pointer");
  philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
  return 0;
}

extern "C" int pnrf_scene_arrays(const pnrf_scene_t* s, const float** img4, const float** poses, const float** K_target, const float** K_ref) {
  int rc = check_scene("pnrf_scene_arrays", s);
  if (rc) return rc;
  if (img4) *img4 = (const float*)s->cache;
  if (poses) *poses = s->poses;
  if (K_target) *K_target = s->K;
  if (K_ref) *K_ref = s->K + 9;
  return 0;
}

extern "C" int pnrf_scene_rank_table_fwd(const pnrf_scene_t* s, int32_t* rank, void* stream) {
  int rc = check_scene("pnrf_scene_rank_table_fwd", s);
  if (rc) return rc;
  PNRF_REQUIRE(rank, PNRF_E_ARG, "pnrf_scene_rank_table_fwd: null output");
  if ((rc = check_device("pnrf_scene_rank_table_fwd", s))) return rc;
  hipLaunchKernelGGL(scene_rank_table_kernel, dim3(s->nv), dim3(TPB), 0, (hipStream_t)stream, s->poses, s->nv, rank);
  PNRF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pnrf_train_batch_fwd(const pnrf_scene_t* s, const int32_t* rank, const int64_t* idx, int64_t n, const int* order, float near, float far,
                                    float or_near, float or_far, float* rays, float* or_rays, float* target, int64_t* ref_nos, int64_t* bad_rows,
                                    uint64_t seed, uint32_t step, int64_t row0, float* jitter, int jitter_cols, float jitter_cap, float* noise,
                                    int noise_cols, float noise_std, void* stream) {
  int rc = check_scene("pnrf_train_batch_fwd", s);
  if (rc) return rc;
  PNRF_REQUIRE(s->nv >= 5, PNRF_E_ARG, "pnrf_train_batch_fwd: a batch draws 4 neighbour ranks out of nv - 1 >= 4 views, the scene has %d", s->nv);
  PNRF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PNRF_E_ARG, "pnrf_train_batch_fwd: n must be 0 .. 2^31 - 1, got %lld", (long long)n);
  PNRF_REQUIRE(order, PNRF_E_ARG, "pnrf_train_batch_fwd: null order");
  OrderArg oa;
  for (int k = 0; k < 4; ++k) {
    PNRF_REQUIRE(order[k] >= 0 && order[k] < s->nv - 1, PNRF_E_ARG, "pnrf_train_batch_fwd: order[%d] = %d outside 0 .. %d", k, order[k], s->nv - 2);
    oa.o[k] = order[k];
  }
  PNRF_REQUIRE(rank && idx && rays && or_rays && target && ref_nos, PNRF_E_ARG, "pnrf_train_batch_fwd: null pointer");
  PNRF_REQUIRE(row0 >= 0, PNRF_E_ARG, "pnrf_train_batch_fwd: row0 must not be negative, got %lld", (long long)row0);
  const int cj = jitter ? jitter_cols : 0, cn = noise ? noise_cols : 0;
  PNRF_REQUIRE(cj >= 0 && cj <= MAX_DRAW_COLS && (cj & 3) == 0 && cn >= 0 && cn <= MAX_DRAW_COLS && (cn & 3) == 0, PNRF_E_ARG,
               "pnrf_train_batch_fwd: jitter_cols / noise_cols must be multiples of 4 up to %d, got %d / %d", MAX_DRAW_COLS, jitter_cols, noise_cols);
  PNRF_REQUIRE((!jitter || cj > 0) && (!noise || cn > 0), PNRF_E_ARG, "pnrf_train_batch_fwd: an output of 0 columns (pass NULL to skip the draw)");
  PNRF_REQUIRE((((uintptr_t)jitter | (uintptr_t)noise) & 15) == 0, PNRF_E_ARG, "pnrf_train_batch_fwd: jitter and noise must be 16-byte aligned");
  if ((rc = check_device("pnrf_train_batch_fwd", s))) return rc;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  FrameArgs a = {};
  a.H = s->Hf; a.W = s->Wf; a.near = near; a.far = far; a.or_near = or_near; a.or_far = or_far; a.count = 1;
  hipLaunchKernelGGL(train_batch_rows_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, a, s->K, s->poses, (const float4*)s->cache, rank, s->nv,
                     (int64_t)s->Hf * s->Wf, idx, n, oa, rays, or_rays, target, ref_nos, (unsigned long long*)bad_rows);
  PNRF_LAUNCH_CHECK();
  if (cj + cn > 0) {
    DrawArgs d;
    d.key0 = (uint32_t)seed; d.key1 = (uint32_t)(seed >> 32); d.step = step; d.row0 = row0; d.n = n;
    d.jitter = jitter; d.qj = cj / 4; d.cap = jitter_cap;
    d.noise = noise; d.qn = cn / 4; d.std = noise_std;
    hipLaunchKernelGGL(train_batch_draws_kernel, dim3(grid_for(n * (int64_t)(d.qj + d.qn))), dim3(TPB), 0, st, d);
    PNRF_LAUNCH_CHECK();
  }
  return 0;
}
