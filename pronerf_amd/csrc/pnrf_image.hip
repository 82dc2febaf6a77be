// pnrf_image.hip — the frame tail on the device: img2mse + img2ssim of a finished frame against its ground truth (pnrf_image_metrics_fwd)
// and the 8-bit planes the PNG writer takes (pnrf_frame_to8b_fwd); and img2ssim as a training loss: the mean SSIM of B patch pairs with its
// gradient with respect to the prediction (pnrf_ssim_loss_fwd).  Streaming kernels, no MFMA; nothing here is shared with the fused-MLP units.
//
// Gradient of the SSIM.  Per window and channel, with x' = pred - max_val / 2, y' = gt - max_val / 2, the filtered moments
// m0 = F[x'], m1 = F[y'], m00 = F[x'^2], m01 = F[x' y'], s00 = m00 - m0^2, s01 = m01 - m0 m1 and S the window's quotient:
//   b = dS/ds00 through the clamp (zero unless s00 > 0),  e = dS/ds01 through the limiter,  a = dS/dmu0 (direct) - 2 m0 b - m1 e,
// and the window gives w_p (a + 2 b x'_p + e y'_p) to each of its pixels p (w: the separable filter).  Where the limiter is active
// (|s01| > sqrt(v0 v1), c = sign(s01) sqrt(v0 v1)) e is 0 and b gains sign(s01) 1/2 sqrt(v1 / v0) dS/dc where v0 > 0.
// STATED DEVIATION FROM AUTOGRAD: exactly on a kink torch's maximum / minimum split the gradient between their operands; this kernel takes
// one branch — s00 == 0: b = 0;  |s01| == sqrt(v0 v1): the limiter counts as inactive (e = dS/dc).  Off the kinks the two agree.
#include <math.h>

#include "pnrf_common.h"
#include "pnrf_ieee.h"

using namespace pnrf;

namespace {

constexpr int TPB = 256;
constexpr int TILE = 32;                  // output tile of the SSIM kernel: 32 x 32 windows per workgroup and channel (tests/test_metrics_gpu.py names it)
constexpr int MAXT = 16;                  // largest filter
constexpr int IN = TILE + MAXT - 1;       // input tile with its halo: at most 47 x 47 pixels
constexpr int INP = IN + 1;               // ... its row pitch in LDS

struct MetricsArgs {
  const float* a;        // pred
  const float* b;        // gt
  int sa, sb;            // pixel strides in floats
  int H, W, OH, OW, T;
  float taps[MAXT];
  float shift;           // subtracted from both images before the moments are formed (max_val / 2)
  float shift_w;         // shift * sum(taps): what the filtered means get back
  float c1, c2;
  float* map;            // [OH, OW, 3] or NULL
  double* partial;       // [workgroups][2] = {sum of squared differences, sum of SSIM values};  the loss instance: [workgroups] sums of SSIM values
  // the loss instance (GRAD) only: workgroup z works on patch z / 3
  int64_t pa, pb;        // patch strides in floats
  float* coef;           // [3][gridDim.z][OH, OW]: the planes a, b, e of every patch and channel
};

// Sum over the workgroup in a fixed order (a tree over LDS): the same bits whatever the scheduling.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// One workgroup per 32 x 32 output tile and channel.  run_nerf_helpers.py:170-196: the reference filters the columns first and the rows second, in
// float64; here the rows come first (both input tiles are read from LDS once per tap) and the arithmetic is fp32 with fused multiply-adds.
// GRAD: the first pass of pnrf_ssim_loss_fwd — the same windows of patch blockIdx.z / 3, no squared differences, and per window the three
// coefficients of its gradient (top of this file) into p.coef.  The text up to the quotient is one for both instances, so a patch's SSIM sum has
// the bits of pnrf_image_metrics_fwd's; the coefficients use none of the quotient's products again (a product with a second use could be
// fused into another operation than in the metrics instance).
template <bool GRAD>
__global__ __launch_bounds__(TPB) void image_ssim_kernel(MetricsArgs p) {
  __shared__ float s_a[IN * INP], s_b[IN * INP];       // the two input tiles, shifted
  __shared__ float s_h[5][IN * TILE];                  // moments a, b, a^2, b^2, ab after the pass along x
  __shared__ double s_red[TPB];
  __shared__ float s_w[MAXT];
  const int tid = threadIdx.x, ch = blockIdx.z % 3, T = p.T;
  const float* pa = GRAD ? p.a + (int64_t)(blockIdx.z / 3) * p.pa : p.a;
  const float* pb = GRAD ? p.b + (int64_t)(blockIdx.z / 3) * p.pb : p.b;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  const int tw = min(TILE, p.OW - x0), th = min(TILE, p.OH - y0);       // windows of this tile
  const int iw = tw + T - 1, ih = th + T - 1;                           // pixels it reads: x0 + iw <= W, y0 + ih <= H
  // every pixel's squared difference is counted by exactly one tile: the tile whose windows start there, and the last tile of a row / column also its halo
  const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
  if (tid < MAXT) s_w[tid] = tid < T ? p.taps[tid] : 0.f;
  double sse = 0.0;
  for (int i = tid; i < ih * iw; i += TPB) {
    const int r = i / iw, c = i - r * iw;
    const int64_t pix = (int64_t)(y0 + r) * p.W + (x0 + c);
    const float a = pa[pix * p.sa + ch], b = pb[pix * p.sb + ch];
    if (!GRAD && (r < TILE || lasty) && (c < TILE || lastx)) {
      const float d = ieee_sub(a, b);                                  // img2mse: the difference in fp32, as torch forms it; squares and sum in fp64
      sse += (double)d * (double)d;
    }
    s_a[r * INP + c] = a - p.shift;
    s_b[r * INP + c] = b - p.shift;
  }
  __syncthreads();
  // pass along x: out[c] = sum_k taps[k] z[c + T - 1 - k] (a convolution, :170-171)
  for (int i = tid; i < ih * TILE; i += TPB) {
    const int r = i / TILE, c = i % TILE;
    if (c < tw) {
      float m0 = 0.f, m1 = 0.f, m00 = 0.f, m11 = 0.f, m01 = 0.f;
      for (int k = 0; k < T; ++k) {
        const float w = s_w[k];
        const float x = s_a[r * INP + c + T - 1 - k], y = s_b[r * INP + c + T - 1 - k];
        const float wx = w * x, wy = w * y;
        m0 += wx;
        m1 += wy;
        m00 = fmaf(wx, x, m00);
        m11 = fmaf(wy, y, m11);
        m01 = fmaf(wx, y, m01);
      }
      s_h[0][i] = m0; s_h[1][i] = m1; s_h[2][i] = m00; s_h[3][i] = m11; s_h[4][i] = m01;
    }
  }
  __syncthreads();
  // pass along y and the quotient (:176-196)
  double acc = 0.0;
  for (int i = tid; i < th * TILE; i += TPB) {
    const int y = i / TILE, x = i % TILE;
    if (x < tw) {
      float m0 = 0.f, m1 = 0.f, m00 = 0.f, m11 = 0.f, m01 = 0.f;
      for (int k = 0; k < T; ++k) {
        const float w = s_w[k];
        const int j = (y + T - 1 - k) * TILE + x;
        m0 = fmaf(w, s_h[0][j], m0);
        m1 = fmaf(w, s_h[1][j], m1);
        m00 = fmaf(w, s_h[2][j], m00);
        m11 = fmaf(w, s_h[3][j], m11);
        m01 = fmaf(w, s_h[4][j], m01);
      }
      const float mu0 = m0 + p.shift_w, mu1 = m1 + p.shift_w;          // the means of the unshifted images
      const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
      float s00 = m00 - m0 * m0, s11 = m11 - m1 * m1, s01 = m01 - m0 * m1;   // shift-invariant
      s00 = s00 < 0.f ? 0.f : s00;                                     // np.maximum(0., .): NaN stays NaN
      s11 = s11 < 0.f ? 0.f : s11;
      const float r01 = s01, sq = sqrtf(s00 * s11);
      const float lim = fminf(sq, fabsf(s01));
      s01 = s01 > 0.f ? lim : (s01 < 0.f ? -lim : s01);               // np.sign(s01) * min(sqrt(s00 s11), |s01|)
      const float A1 = 2.f * mu01 + p.c1, A2 = 2.f * s01 + p.c2, B1 = mu00 + mu11 + p.c1, B2 = s00 + s11 + p.c2;
      const float numer = A1 * A2;
      const float denom = B1 * B2;
      const float v = numer / denom;
      acc += (double)v;
      if constexpr (GRAD) {
        const float dc = (2.f * A1) / denom;                           // dS/dc, c the limited covariance
        float e = dc, b = 0.f;
        if (s00 > 0.f) b = -v / B2;                                    // dS/dv0 through the clamp; s00 == 0 takes the zero branch
        if (!(fabsf(r01) <= sq)) {                                     // limiter active: c = sign(s01) sqrt(v0 v1); equality counts as inactive
          e = 0.f;
          if (s00 > 0.f) b += (r01 > 0.f ? 0.5f : -0.5f) * (sqrtf(s11) / sqrtf(s00)) * dc;
        }
        const float dmu = (2.f * mu1 * A2) / denom - (2.f * mu0 * v) / B1;
        const int64_t plane = (int64_t)p.OH * p.OW, at = (int64_t)(y0 + y) * p.OW + (x0 + x);
        float* cf = p.coef + (int64_t)blockIdx.z * plane + at;
        cf[0] = dmu - 2.f * m0 * b - m1 * e;                           // a NaN window leaves a NaN here whatever its branches were
        cf[(int64_t)gridDim.z * plane] = b;
        cf[2 * (int64_t)gridDim.z * plane] = e;
      } else {
        if (p.map) p.map[((int64_t)(y0 + y) * p.OW + (x0 + x)) * 3 + ch] = v;
      }
    }
  }
  const double ssum = block_sum(acc, s_red);
  const int64_t bid = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if constexpr (GRAD) {
    if (tid == 0) p.partial[bid] = ssum;
  } else {
    const double esum = block_sum(sse, s_red);
    if (tid == 0) {
      p.partial[2 * bid] = esum;
      p.partial[2 * bid + 1] = ssum;
    }
  }
}

// The partial sums of all workgroups, in index order per thread and then over the tree: one workgroup, fp64.
__global__ __launch_bounds__(TPB) void image_metrics_finish_kernel(const double* partial, int64_t nblocks, double n_values, double n_windows, double* out) {
  __shared__ double s_red[TPB];
  double e = 0.0, s = 0.0;
  for (int64_t j = threadIdx.x; j < nblocks; j += TPB) {
    e += partial[2 * j];
    s += partial[2 * j + 1];
  }
  e = block_sum(e, s_red);
  s = block_sum(s, s_red);
  if (threadIdx.x == 0) {
    out[0] = e;
    out[1] = e / n_values;
    out[2] = s;
    out[3] = s / n_windows;
  }
}

inline int64_t metrics_tiles(int H, int W, int T, dim3* grid) {
  if (T < 1 || T > MAXT || H < T || W < T) return 0;
  const int64_t gx = ((int64_t)W - T + 1 + TILE - 1) / TILE, gy = ((int64_t)H - T + 1 + TILE - 1) / TILE;
  if (gy > 65535) return 0;
  if (grid) *grid = dim3((unsigned)gx, (unsigned)gy, 3);
  return gx * gy * 3;
}

// The window sizes, the filter and the constants of img2ssim, the same for the metrics and for the loss.
inline void ssim_constants(MetricsArgs* p, int H, int W, const float* taps, int T, float max_val, float k1, float k2) {
  p->H = H; p->W = W; p->OH = H - T + 1; p->OW = W - T + 1; p->T = T;
  double wsum = 0.0;
  for (int k = 0; k < MAXT; ++k) {
    p->taps[k] = k < T ? taps[k] : 0.f;
    wsum += (double)p->taps[k];
  }
  p->shift = 0.5f * max_val;
  p->shift_w = (float)((double)p->shift * wsum);
  p->c1 = (float)(((double)k1 * (double)max_val) * ((double)k1 * (double)max_val));      // :191-192, in double like the reference's Python floats
  p->c2 = (float)(((double)k2 * (double)max_val) * ((double)k2 * (double)max_val));
}

// ---- SSIM loss: the second pass, with the sum ------------------------------------------------------------------------------------------------
constexpr int MAX_PATCHES = 65535 / 3;    // a patch and channel per grid z

struct SsimGradArgs {
  const float* coef;     // [3][3 B][OH, OW]: a, b, e of the first pass
  const float* a;        // pred
  const float* b;        // gt
  int sa, sb;            // pixel strides in floats
  int64_t pa, pb;        // patch strides in floats
  int H, W, OH, OW, T;
  float taps[MAXT];
  float shift;
  float inv_n;           // 1 / (B OH OW 3)
  float* d;              // [B, H, W, 3]
  const double* partial; // [nblocks]: the first pass's sums of SSIM values
  int64_t nblocks;
  double n_windows;      // B OH OW 3
  double* out;           // {sum, mean}
};

// d mean / d pred as a gather: pixel p collects w (a + 2 b x'_p + e y'_p) of every window that holds it — the transposed ("full") separable
// convolution of the three planes, F^T[m](py, px) = sum_ij taps[T-1-i] taps[T-1-j] m(py - i, px - j) with zeros outside the planes.  One
// workgroup per 32 x 32 PIXEL tile, patch and channel: the planes' tile with its halo (towards smaller indices) in LDS, a pass along x into
// LDS, a pass along y from it.  Every pixel is written by one thread: no atomics.
__global__ __launch_bounds__(TPB) void ssim_grad_gather_kernel(SsimGradArgs p) {
  __shared__ float s_m[3][IN * INP];                   // a, b, e: plane rows y0 - T + 1 .. y0 + th - 1, columns likewise
  __shared__ float s_h[3][IN * TILE];
  __shared__ double s_red[TPB];
  __shared__ float s_w[MAXT];
  const int tid = threadIdx.x, ch = blockIdx.z % 3, T = p.T;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  const int tw = min(TILE, p.W - x0), th = min(TILE, p.H - y0);         // pixels of this tile
  const int iw = tw + T - 1, ih = th + T - 1;
  const int64_t plane = (int64_t)p.OH * p.OW;
  if (tid < MAXT) s_w[tid] = tid < T ? p.taps[tid] : 0.f;
  for (int i = tid; i < ih * iw; i += TPB) {
    const int r = i / iw, c = i - r * iw;
    const int oy = y0 - (T - 1) + r, ox = x0 - (T - 1) + c;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    if (oy >= 0 && oy < p.OH && ox >= 0 && ox < p.OW) {
      const float* cf = p.coef + (int64_t)blockIdx.z * plane + ((int64_t)oy * p.OW + ox);
      m0 = cf[0]; m1 = cf[(int64_t)gridDim.z * plane]; m2 = cf[2 * (int64_t)gridDim.z * plane];
    }
    s_m[0][r * INP + c] = m0; s_m[1][r * INP + c] = m1; s_m[2][r * INP + c] = m2;
  }
  __syncthreads();
  for (int i = tid; i < ih * TILE; i += TPB) {
    const int r = i / TILE, c = i % TILE;
    if (c < tw) {
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
      for (int j = 0; j < T; ++j) {                                     // window column px - j holds pixel px at its tap T - 1 - j
        const float w = s_w[T - 1 - j];
        const int k = r * INP + c + T - 1 - j;
        g0 = fmaf(w, s_m[0][k], g0);
        g1 = fmaf(w, s_m[1][k], g1);
        g2 = fmaf(w, s_m[2][k], g2);
      }
      s_h[0][i] = g0; s_h[1][i] = g1; s_h[2][i] = g2;
    }
  }
  __syncthreads();
  const int64_t patch = blockIdx.z / 3;
  for (int i = tid; i < th * TILE; i += TPB) {
    const int y = i / TILE, x = i % TILE;
    if (x < tw) {
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
      for (int j = 0; j < T; ++j) {
        const float w = s_w[T - 1 - j];
        const int k = (y + T - 1 - j) * TILE + x;
        g0 = fmaf(w, s_h[0][k], g0);
        g1 = fmaf(w, s_h[1][k], g1);
        g2 = fmaf(w, s_h[2][k], g2);
      }
      const int64_t pix = (int64_t)(y0 + y) * p.W + (x0 + x);
      const float xs = p.a[patch * p.pa + pix * p.sa + ch] - p.shift, ys = p.b[patch * p.pb + pix * p.sb + ch] - p.shift;   // as the first pass shifts them
      p.d[(patch * p.H * p.W + pix) * 3 + ch] = (g0 + 2.f * xs * g1 + ys * g2) * p.inv_n;
    }
  }
  // the first workgroup also adds the first pass's partial sums, in image_metrics_finish_kernel's order: one patch has that call's bits
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    double s = 0.0;
    for (int64_t j = tid; j < p.nblocks; j += TPB) s += p.partial[j];
    s = block_sum(s, s_red);
    if (tid == 0) {
      p.out[0] = s;
      p.out[1] = s / p.n_windows;
    }
  }
}

// ---- to8b ------------------------------------------------------------------------------------------------------------------------------
constexpr int MAX_PARTIAL = PNRF_TO8B_WORKSPACE_BYTES / (int)sizeof(float);      // workgroups of the maximum's first kernel

__device__ __forceinline__ float block_max(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = fmaxf(red[t], red[t + s]);       // fmaxf: a NaN operand is skipped
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(TPB) void depth_max_kernel(const float* depth, int ds, int64_t n, float* partial) {
  __shared__ float s_red[TPB];
  float m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) m = fmaxf(m, depth[i * ds]);
  m = block_max(m, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8): one fp32 product, truncated.  NaN -> 0.
__device__ __forceinline__ unsigned to8(float x) {
  if (!(x == x)) return 0u;
  const float v = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  return (unsigned)ieee_mul(255.f, v);
}

// Four pixels per thread: 12 + 4 output bytes leave as whole dwords where the output pointers allow it (wide = both 4-byte aligned).
__global__ __launch_bounds__(TPB) void frame_to8b_kernel(const float* rgb, int rs, const float* depth, int ds, int64_t n, const float* partial, int npartial,
                                                        uint8_t* rgb8, uint8_t* depth8, int wide) {
  __shared__ float s_red[TPB];
  float mx = 1.f;
  if (depth8) {                                           // every workgroup reduces the (at most 1024) partial maxima itself
    float m = -INFINITY;
    for (int j = threadIdx.x; j < npartial; j += TPB) m = fmaxf(m, partial[j]);
    mx = block_max(m, s_red);
  }
  const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x, i0 = g * 4;
  if (i0 >= n) return;
  const int cnt = (int)(n - i0 < 4 ? n - i0 : 4);
  unsigned q[12], dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + (j < cnt ? j : 0);
    if (rgb8) {
      q[3 * j] = to8(rgb[i * rs]); q[3 * j + 1] = to8(rgb[i * rs + 1]); q[3 * j + 2] = to8(rgb[i * rs + 2]);
    }
    if (depth8) dq[j] = to8(ieee_div(depth[i * ds], mx));          // one correctly rounded division, as numpy's depth / depth.max()
  }
  if (wide && cnt == 4) {
    if (rgb8) {
      uint32_t* o = (uint32_t*)rgb8 + g * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] = q[4 * j] | (q[4 * j + 1] << 8) | (q[4 * j + 2] << 16) | (q[4 * j + 3] << 24);
    }
    if (depth8) ((uint32_t*)depth8)[g] = dq[0] | (dq[1] << 8) | (dq[2] << 16) | (dq[3] << 24);
  } else {
    for (int j = 0; j < cnt; ++j) {
      if (rgb8) {
        rgb8[(i0 + j) * 3] = (uint8_t)q[3 * j]; rgb8[(i0 + j) * 3 + 1] = (uint8_t)q[3 * j + 1]; rgb8[(i0 + j) * 3 + 2] = (uint8_t)q[3 * j + 2];
      }
      if (depth8) depth8[i0 + j] = (uint8_t)dq[j];
    }
  }
}

}  // namespace

extern "C" int64_t pnrf_image_metrics_workspace_bytes(int H, int W, int T) { return metrics_tiles(H, W, T, nullptr) * 2 * (int64_t)sizeof(double); }

extern "C" int pnrf_image_metrics_fwd(const float* pred, int pred_stride, const float* gt, int gt_stride, int H, int W, const float* taps, int T,
                                      float max_val, float k1, float k2, double* out, float* ssim_map, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  PNRF_REQUIRE(pred && gt && taps && out && workspace, PNRF_E_ARG, "pnrf_image_metrics_fwd: null pointer (pred, gt, taps, out and workspace are required)");
  PNRF_REQUIRE(T >= 1 && T <= MAXT, PNRF_E_ARG, "pnrf_image_metrics_fwd: filter size %d outside 1 .. %d", T, MAXT);
  PNRF_REQUIRE(H >= T && W >= T, PNRF_E_ARG, "pnrf_image_metrics_fwd: a %d x %d image has no %d x %d window", H, W, T, T);
  PNRF_REQUIRE(pred_stride >= 3 && gt_stride >= 3, PNRF_E_ARG, "pnrf_image_metrics_fwd: pixel strides %d / %d, need >= 3 floats", pred_stride, gt_stride);
  dim3 grid;
  const int64_t nblocks = metrics_tiles(H, W, T, &grid);
  PNRF_REQUIRE(nblocks > 0, PNRF_E_ARG, "pnrf_image_metrics_fwd: image of %d rows is too tall (at most %d rows of windows)", H, 65535 * TILE);
  PNRF_REQUIRE(workspace_bytes >= pnrf_image_metrics_workspace_bytes(H, W, T) && ((uintptr_t)workspace & 7) == 0, PNRF_E_ARG,
               "pnrf_image_metrics_fwd: workspace of %lld bytes (8-byte aligned) needed, got %lld", (long long)pnrf_image_metrics_workspace_bytes(H, W, T),
               (long long)workspace_bytes);
  MetricsArgs p;
  p.a = pred; p.b = gt; p.sa = pred_stride; p.sb = gt_stride;
  ssim_constants(&p, H, W, taps, T, max_val, k1, k2);
  p.map = ssim_map;
  p.partial = (double*)workspace;
  p.pa = p.pb = 0; p.coef = nullptr;
  hipLaunchKernelGGL(image_ssim_kernel<false>, grid, dim3(TPB), 0, (hipStream_t)stream, p);
  PNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const double*)workspace, nblocks,
                     (double)H * (double)W * 3.0, (double)p.OH * (double)p.OW * 3.0, out);
  PNRF_LAUNCH_CHECK();
  return 0;
}

// Workspace of the loss: one fp64 partial sum per workgroup of the first pass, then the three coefficient planes of every patch and channel.
extern "C" int64_t pnrf_ssim_loss_workspace_bytes(int B, int H, int W, int T) {
  const int64_t tiles = metrics_tiles(H, W, T, nullptr);
  if (tiles == 0 || B < 1 || B > MAX_PATCHES || ((int64_t)H + TILE - 1) / TILE > 65535) return 0;
  return B * (tiles * (int64_t)sizeof(double) + 9 * ((int64_t)H - T + 1) * ((int64_t)W - T + 1) * (int64_t)sizeof(float));
}

extern "C" int pnrf_ssim_loss_fwd(const float* pred, int pred_stride, int64_t pred_patch_stride, const float* gt, int gt_stride, int64_t gt_patch_stride,
                                  int B, int H, int W, const float* taps, int T, float max_val, float k1, float k2, double* out, float* d_pred,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(pred && gt && taps && out && d_pred && workspace, PNRF_E_ARG,
               "pnrf_ssim_loss_fwd: null pointer (pred, gt, taps, out, d_pred and workspace are required)");
  PNRF_REQUIRE(T >= 1 && T <= MAXT, PNRF_E_ARG, "pnrf_ssim_loss_fwd: filter size %d outside 1 .. %d", T, MAXT);
  PNRF_REQUIRE(H >= T && W >= T, PNRF_E_ARG, "pnrf_ssim_loss_fwd: a %d x %d patch has no %d x %d window", H, W, T, T);
  PNRF_REQUIRE(B >= 1 && B <= MAX_PATCHES, PNRF_E_ARG, "pnrf_ssim_loss_fwd: %d patches outside 1 .. %d", B, MAX_PATCHES);
  PNRF_REQUIRE(pred_stride >= 3 && gt_stride >= 3, PNRF_E_ARG, "pnrf_ssim_loss_fwd: pixel strides %d / %d, need >= 3 floats", pred_stride, gt_stride);
  PNRF_REQUIRE(pred_patch_stride >= 0 && gt_patch_stride >= 0, PNRF_E_ARG, "pnrf_ssim_loss_fwd: patch strides %lld / %lld, need >= 0 floats",
               (long long)pred_patch_stride, (long long)gt_patch_stride);
  dim3 grid;
  const int64_t tiles = metrics_tiles(H, W, T, &grid);
  const dim3 grid2((unsigned)((W + TILE - 1) / TILE), (unsigned)(((int64_t)H + TILE - 1) / TILE), (unsigned)(3 * B));
  PNRF_REQUIRE(tiles > 0 && grid2.y <= 65535, PNRF_E_ARG, "pnrf_ssim_loss_fwd: patch of %d rows is too tall (at most %d)", H, 65535 * TILE);
  const int64_t need = pnrf_ssim_loss_workspace_bytes(B, H, W, T);
  PNRF_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, PNRF_E_ARG,
               "pnrf_ssim_loss_fwd: workspace of %lld bytes (8-byte aligned) needed, got %lld", (long long)need, (long long)workspace_bytes);
  grid.z = 3 * B;
  const int64_t nblocks = tiles * B;
  const double n_windows = (double)B * (double)(H - T + 1) * (double)(W - T + 1) * 3.0;
  MetricsArgs p;
  p.a = pred; p.b = gt; p.sa = pred_stride; p.sb = gt_stride; p.pa = pred_patch_stride; p.pb = gt_patch_stride;
  ssim_constants(&p, H, W, taps, T, max_val, k1, k2);
  p.map = nullptr;
  p.partial = (double*)workspace;
  p.coef = (float*)((double*)workspace + nblocks);
  hipLaunchKernelGGL(image_ssim_kernel<true>, grid, dim3(TPB), 0, (hipStream_t)stream, p);
  PNRF_LAUNCH_CHECK();
  SsimGradArgs q;
  q.coef = p.coef; q.a = pred; q.b = gt; q.sa = pred_stride; q.sb = gt_stride; q.pa = pred_patch_stride; q.pb = gt_patch_stride;
  q.H = H; q.W = W; q.OH = p.OH; q.OW = p.OW; q.T = T;
  for (int k = 0; k < MAXT; ++k) q.taps[k] = p.taps[k];
  q.shift = p.shift;
  q.inv_n = (float)(1.0 / n_windows);
  q.d = d_pred;
  q.partial = p.partial; q.nblocks = nblocks; q.n_windows = n_windows; q.out = out;
  hipLaunchKernelGGL(ssim_grad_gather_kernel, grid2, dim3(TPB), 0, (hipStream_t)stream, q);
  PNRF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pnrf_frame_to8b_fwd(const float* rgb, int rgb_stride, const float* depth, int depth_stride, int64_t n, uint8_t* rgb8, uint8_t* depth8,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(rgb8 || depth8, PNRF_E_ARG, "pnrf_frame_to8b_fwd: null pointer for both outputs");
  PNRF_REQUIRE(n >= 0 && n < ((int64_t)1 << 40), PNRF_E_ARG, "pnrf_frame_to8b_fwd: pixel count %lld outside 0 .. 2^40", (long long)n);
  PNRF_REQUIRE(!rgb8 || rgb, PNRF_E_ARG, "pnrf_frame_to8b_fwd: null pointer (rgb8 without rgb)");
  PNRF_REQUIRE(!rgb8 || rgb_stride >= 3, PNRF_E_ARG, "pnrf_frame_to8b_fwd: rgb pixel stride %d, need >= 3 floats", rgb_stride);
  PNRF_REQUIRE(!depth8 || depth, PNRF_E_ARG, "pnrf_frame_to8b_fwd: null pointer (depth8 without depth)");
  PNRF_REQUIRE(!depth8 || depth_stride >= 1, PNRF_E_ARG, "pnrf_frame_to8b_fwd: depth pixel stride %d, need >= 1 float", depth_stride);
  PNRF_REQUIRE(!depth8 || (workspace && workspace_bytes >= PNRF_TO8B_WORKSPACE_BYTES && ((uintptr_t)workspace & 3) == 0), PNRF_E_ARG,
               "pnrf_frame_to8b_fwd: depth8 needs a workspace of %d bytes (4-byte aligned), got %lld", PNRF_TO8B_WORKSPACE_BYTES, (long long)workspace_bytes);
  if (n == 0) return 0;
  int npartial = 0;
  if (depth8) {
    const int64_t want = (n + TPB - 1) / TPB;
    npartial = (int)(want < MAX_PARTIAL ? want : MAX_PARTIAL);
    hipLaunchKernelGGL(depth_max_kernel, dim3(npartial), dim3(TPB), 0, (hipStream_t)stream, depth, depth_stride, n, (float*)workspace);
    PNRF_LAUNCH_CHECK();
  }
  const int wide = (((uintptr_t)rgb8 | (uintptr_t)depth8) & 3) == 0;
  const int64_t groups = (n + 3) / 4;
  hipLaunchKernelGGL(frame_to8b_kernel, dim3((unsigned)((groups + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, rgb, rgb_stride, depth, depth_stride, n,
                     (const float*)workspace, npartial, rgb8, depth8, wide);
  PNRF_LAUNCH_CHECK();
  return 0;
}
