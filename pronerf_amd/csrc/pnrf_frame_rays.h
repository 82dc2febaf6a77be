// pnrf_frame_rays.h — per-pixel arithmetic of the frame's ray set-up (get_rays + viewdirs + ndc_rays), shared by the two kernels that run it: frame_rays_kernel
// (pnrf_ops.hip: camera in the kernel arguments, from host pointers) and frame_rays_dev_kernel (pnrf_scene.hip: camera read from device memory).  One body, so the
// two entry points cannot drift apart: their outputs are bit-identical (tests/test_scene_gpu.py).
#pragma once
#include <stdint.h>

#include "pnrf_common.h"
#include "pnrf_ieee.h"

namespace pnrf {

// ---------------------------------------------------------------- frame rays (trt.py:245-271; helpers:2705-2714, 2776-2793)
// The NDC scale factors follow the reference drivers' types: K is a float64 numpy array there (run_S_eS_eN_alter_trt.py:742-747, :798), so
// -1./(W/(2.*focal)) is evaluated in double and rounded to fp32 once, when it meets the fp32 ray tensor (helpers:2781-2786).
__host__ __device__ static inline float ndc_scale(int extent, float focal) { return (float)(-1.0 / ((double)extent / (2.0 * (double)focal))); }

struct FrameArgs {
  float K00, K02, K11, K12;
  float sx, sy;              // ndc_scale(W, K00), ndc_scale(H, K00)
  float R[9], T[3];
  int H, W;
  float near, far, or_near, or_far;
  int64_t first, count;
  int64_t block, stride;     // output row q is pixel first + (q / block) * stride + q % block (one contiguous range: block = count; a rank's blocks of a
                             // block-cyclic partition: first = rank * block, stride = world * block)
};
// The row range of a launch, checked the same way by every entry point that runs the body below: sizes, and that the blocks neither leave the H x W frame
// nor overlap.  0 = ok (count == 0 included), else PNRF_E_ARG with the message set.
static inline int frame_rays_check(const char* who, int H, int W, int64_t first, int64_t block, int64_t stride, int64_t count) {
  PNRF_REQUIRE(H > 0 && W > 0 && first >= 0 && count >= 0 && block >= 1 && stride >= 0, PNRF_E_ARG,
               "%s: bad arguments (H=%d W=%d first=%lld block=%lld stride=%lld count=%lld)", who, H, W, (long long)first, (long long)block, (long long)stride,
               (long long)count);
  if (count == 0) return 0;
  const int64_t last = first + ((count - 1) / block) * stride + (count - 1) % block;          // the largest pixel index addressed
  PNRF_REQUIRE(last < (int64_t)H * W && (stride == 0 ? count <= block : stride >= block), PNRF_E_ARG,
               "%s: the blocks leave the %d x %d frame or overlap (last pixel %lld)", who, H, W, (long long)last);
  return 0;
}

// Output row q of a launch: pixel a.first + (q / a.block) * a.stride + q % a.block.
__device__ __forceinline__ void frame_ray_row(const FrameArgs& a, int64_t q, float* __restrict__ rays, float* __restrict__ or_rays) {
  const int64_t pix = a.first + (q / a.block) * a.stride + q % a.block;
  const int j = (int)(pix / a.W), i = (int)(pix - (int64_t)j * a.W);
  // dirs = ((i-cx)/fx, -(j-cy)/fy, -1);  rays_d[c] = sum_k dirs[k]*R[c][k]  (products, then a 3-term sum)
  const float d0 = ieee_div(ieee_sub((float)i, a.K02), a.K00);
  const float d1 = -ieee_div(ieee_sub((float)j, a.K12), a.K11);
  const float d2 = -1.f;
  float rd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rd[c] = ieee_add(ieee_add(ieee_mul(d0, a.R[c * 3]), ieee_mul(d1, a.R[c * 3 + 1])), ieee_mul(d2, a.R[c * 3 + 2]));
  const float ro[3] = {a.T[0], a.T[1], a.T[2]};
  const float nrm = ieee_sqrt(ieee_fma(rd[2], rd[2], ieee_fma(rd[1], rd[1], ieee_mul(rd[0], rd[0]))));      // torch.norm: an FMA chain (pnrf_geom.h, unit_dir)
  const float v0 = ieee_div(rd[0], nrm), v1 = ieee_div(rd[1], nrm), v2 = ieee_div(rd[2], nrm);
  float* orr = or_rays + q * 11;
  orr[0] = ro[0]; orr[1] = ro[1]; orr[2] = ro[2]; orr[3] = rd[0]; orr[4] = rd[1]; orr[5] = rd[2];
  orr[6] = a.or_near; orr[7] = a.or_far; orr[8] = v0; orr[9] = v1; orr[10] = v2;
  // ndc_rays(H, W, focal=K00, near=1.)
  const float nearp = 1.f;
  const float t = ieee_div(-ieee_add(nearp, ro[2]), rd[2]);
  const float ox = ieee_add(ro[0], ieee_mul(t, rd[0])), oy = ieee_add(ro[1], ieee_mul(t, rd[1])), oz = ieee_add(ro[2], ieee_mul(t, rd[2]));
  const float sx = a.sx, sy = a.sy;
  const float o0 = ieee_div(ieee_mul(sx, ox), oz);
  const float o1 = ieee_div(ieee_mul(sy, oy), oz);
  const float roz = ieee_div(1.f, oz);                               // python scalar / tensor is tensor.reciprocal() * scalar in torch
  const float o2 = ieee_add(1.f, ieee_mul(roz, 2.f * nearp));
  const float e0 = ieee_mul(sx, ieee_sub(ieee_div(rd[0], rd[2]), ieee_div(ox, oz)));
  const float e1 = ieee_mul(sy, ieee_sub(ieee_div(rd[1], rd[2]), ieee_div(oy, oz)));
  const float e2 = ieee_mul(roz, -2.f * nearp);
  float* r = rays + q * 11;
  r[0] = o0; r[1] = o1; r[2] = o2; r[3] = e0; r[4] = e1; r[5] = e2; r[6] = a.near; r[7] = a.far; r[8] = v0; r[9] = v1; r[10] = v2;
}

}  // namespace pnrf
