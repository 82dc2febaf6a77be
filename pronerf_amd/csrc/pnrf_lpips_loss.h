// pnrf_lpips_loss.h — LPIPS as a training loss: the mean d of B patch pairs and its gradient with respect to the prediction (pnrf_lpips_loss_fwd;
// DESIGN §7.4).  The second half of pnrf_lpips.hip, which includes it behind the metric: tables, handle, tap and finish kernels are the metric's.
//
// Batch.  B pairs of H x W x 3 run as ONE batch of 2 B images [pred_0 .. pred_{B-1}, gt_0 .. gt_{B-1}]: to the tap kernel that is a pair of tall images
// (P = B h_k w_k).  Every conv output after ReLU stays in the workspace (ReLU mask, pooling input and tap features of the backward); the pooled
// activations and the gathered first-layer rows are temporaries.
// Forward kernels of the loss's own: the patch-strided first-layer gather, and conv / max pooling instances that keep a NaN (the metric's ReLU and
// maximum are v_max / compares that drop one; a loss must not hide a NaN from the optimiser's caller).  On numbers their results have the metric's bits.
// Backward, pred half only, top layer down; the gradient buffer of a layer holds dZ = dY [Y > 0], written by one writer per element:
//   lpips_tap_bwd_kernel     adds the tap's dF to what arrived from above and applies the mask of its own layer in the store;
//   lpips_dgrad_kernel       dX = dZ * flip(W)^T as the forward's implicit GEMM, epilogue x the mask of the layer below (same address); with few
//                            pixels split over the filter taps (grid z) and summed in tap order by lpips_dgrad_reduce_kernel, which then masks;
//   lpips_maxpool_bwd_kernel gather per pooling-input element over the windows that hold it, then the mask of that element;
//   lpips_dgrad0_kernel      the 3-channel first layer down to the image, a gather per input value, then d(input scaling).
// No atomics, every sum in a fixed order: value and gradient are bit-identical from call to call on any stream.
#pragma once

namespace {

// ---- first layer of the batch: lpips_im2col_kernel's gather and arithmetic, image i < B from a + i pa, else from b + (i - B) pb -----------------
struct Im2colPatchArgs {
  const float *a, *b;
  int sa, sb;
  int64_t pa, pb;
  int B, H, W, OH, OW, k, stride, pad, K, Kp;
  int mode;              // as Im2colArgs
  float* out;            // [2 B OH OW][Kp]
  int64_t total;
};

__global__ __launch_bounds__(TPB) void lpips_im2col_patch_kernel(Im2colPatchArgs p) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= p.total) return;
  const int kk = (int)(i % p.Kp);
  const int m = (int)(i / p.Kp);
  float v = 0.f;
  if (kk < p.K) {
    const int t = kk / 3, c = kk - 3 * t;
    const int ky = t / p.k, kx = t - ky * p.k;
    const int img = m / (p.OH * p.OW), r = m - img * (p.OH * p.OW);
    const int oy = r / p.OW, ox = r - oy * p.OW;
    const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
      const bool second = img >= p.B;
      const float* src = second ? p.b + (int64_t)(img - p.B) * p.pb : p.a + (int64_t)img * p.pa;
      v = src[((int64_t)iy * p.W + ix) * (second ? p.sb : p.sa) + c];
      if (p.mode) {
        const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f), scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
        if (p.mode == 2) v = ieee_sub(ieee_mul(2.f, v), 1.f);
        v = ieee_div(ieee_sub(v, shift), scale);
      }
    }
  }
  p.out[i] = v;
}

// ---- implicit GEMM of the loss: lpips_conv_kernel's tiling (64 pixels x 64 channels, K chunks of 32 channels of one tap, v_mfma_f32_16x16x4_f32) -------
// FWD:   y = ReLU(conv(x) + bias), the ReLU keeping a NaN.
// DGRAD: x = dZ [n, H, W, Cin = the layer's C_out], w = the layer's weights flipped and transposed [k k C_out][C_in], stride 1, pad = k - 1 - the
//        layer's pad, y = dX [n, OH, OW, Cout = the layer's C_in]; no bias; with `mask` (the activation that dX is the gradient of, same shape and
//        address as y) the epilogue writes 0 where mask <= 0.
struct GemmArgs {
  const float* x;
  const float* w;
  const float* bias;
  const float* mask;
  float* y;
  int H, W, Cin, OH, OW, Cout, k, stride, pad;
  int M;                 // n OH OW
  float* part;           // DGRAD, split over the filter taps (grid z = tap): the raw sums of tap z go to part[z][M][Cout], the reduce kernel goes on
};

template <bool DGRAD>
__device__ __forceinline__ void lpips_gemm_body(const GemmArgs& p) {
  __shared__ __attribute__((aligned(16))) float sX[CT_M * SX_LD];
  __shared__ __attribute__((aligned(16))) float sW[CT_K * SW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * CT_M, n0 = blockIdx.y * CT_N;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int xc = (tid & 7) * 4, wr = tid >> 4, wc = (tid & 15) * 4;
  int64_t ximg[2];
  int xy[2], xx[2];
  bool xon[2];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int m = m0 + (tid >> 3) + 32 * ps;
    xon[ps] = m < p.M;
    const int mm = xon[ps] ? m : 0;
    const int img = mm / (p.OH * p.OW), r = mm - img * (p.OH * p.OW);
    const int oy = r / p.OW, ox = r - oy * p.OW;
    ximg[ps] = (int64_t)img * p.H * p.W;
    xy[ps] = oy * p.stride - p.pad;
    xx[ps] = ox * p.stride - p.pad;
  }
  const int cchunks = p.Cin / CT_K;
  const bool split = DGRAD && p.part != nullptr;
  const int q0 = split ? (int)blockIdx.z * cchunks : 0, total = split ? q0 + cchunks : p.k * p.k * cchunks;
  lp_f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = lp_f4{0.f, 0.f, 0.f, 0.f};
  lp_f4 rx[2], rw[2];
  auto fetch = [&](int q) {
    const int t = q / cchunks, c0 = (q - t * cchunks) * CT_K;
    const int ky = t / p.k, kx = t - ky * p.k;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int iy = xy[ps] + ky, ix = xx[ps] + kx;
      const bool ok = xon[ps] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      rx[ps] = ok ? *(const lp_f4*)(p.x + (ximg[ps] + (int64_t)iy * p.W + ix) * p.Cin + c0 + xc) : lp_f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) rw[ps] = *(const lp_f4*)(p.w + ((int64_t)q * CT_K + wr + 16 * ps) * p.Cout + n0 + wc);
  };
  fetch(q0);
  for (int q = q0; q < total; ++q) {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      *(lp_f4*)(sX + ((tid >> 3) + 32 * ps) * SX_LD + xc) = rx[ps];
      *(lp_f4*)(sW + (wr + 16 * ps) * SW_LD + wc) = rw[ps];
    }
    __syncthreads();
    if (q + 1 < total) fetch(q + 1);
#pragma unroll
    for (int k4 = 0; k4 < CT_K; k4 += 4) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = sW[(k4 + g) * SW_LD + wn + 16 * i + l16];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = sX[(wm + 16 * j + l16) * SX_LD + k4 + g];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = n0 + wn + 16 * i + 4 * g;
    lp_f4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (!DGRAD) bias4 = *(const lp_f4*)(p.bias + c);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm + 16 * j + l16;
      if (m < p.M) {
        lp_f4 v = acc[i][j];
        if (split) {
          *(lp_f4*)(p.part + ((int64_t)blockIdx.z * p.M + m) * p.Cout + c) = v;
          continue;
        }
        if (DGRAD) {
          if (p.mask) {
            const lp_f4 k4 = *(const lp_f4*)(p.mask + (int64_t)m * p.Cout + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = k4[e] <= 0.f ? 0.f : v[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float z = ieee_add(v[e], bias4[e]);
            v[e] = z <= 0.f ? 0.f : z;                      // a NaN stays
          }
        }
        *(lp_f4*)(p.y + (int64_t)m * p.Cout + c) = v;
      }
    }
  }
}

__global__ __launch_bounds__(TPB) void lpips_loss_conv_kernel(GemmArgs p) { lpips_gemm_body<false>(p); }
__global__ __launch_bounds__(TPB) void lpips_dgrad_kernel(GemmArgs p) { lpips_gemm_body<true>(p); }

// Second step of the split data gradient: dX = sum over the taps, in tap order, of part[tap]; then the mask.  One thread per 4 channels.
struct DgradReduceArgs { const float* part; const float* mask; float* y; int taps; int64_t total4, plane; };     // plane = M Cout floats, total4 = plane / 4

__global__ __launch_bounds__(TPB) void lpips_dgrad_reduce_kernel(DgradReduceArgs p) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= p.total4) return;
  lp_f4 v = *(const lp_f4*)(p.part + 4 * i);
  for (int t = 1; t < p.taps; ++t) {
    const lp_f4 u = *(const lp_f4*)(p.part + t * p.plane + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ieee_add(v[e], u[e]);
  }
  if (p.mask) {
    const lp_f4 k4 = *(const lp_f4*)(p.mask + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k4[e] <= 0.f ? 0.f : v[e];
  }
  *(lp_f4*)(p.y + 4 * i) = v;
}

// ---- max pooling of the loss: lpips_maxpool_kernel with torch's rule for a NaN (it replaces the maximum) ---------------------------------------
__global__ __launch_bounds__(TPB) void lpips_loss_maxpool_kernel(PoolArgs p) {      // total = n PH PW C / 4
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = p.C / 4;
  const int c = (int)(i % c4) * 4;
  const int64_t pix = i / c4;
  const int img = (int)(pix / ((int64_t)p.PH * p.PW)), r = (int)(pix - (int64_t)img * p.PH * p.PW);
  const int py = r / p.PW, px = r - py * p.PW;
  lp_f4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int dy = 0; dy < p.window; ++dy)
    for (int dx = 0; dx < p.window; ++dx) {
      const lp_f4 v = *(const lp_f4*)(p.x + (((int64_t)img * p.H + 2 * py + dy) * p.W + 2 * px + dx) * p.C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];
    }
  *(lp_f4*)(p.y + pix * p.C + c) = m;
}

// ---- max pooling backward: a gather.  One thread per pooling-input element x 4 channels: the windows that hold it in row-major order; a window gives
// its gradient to the FIRST element attaining its maximum in (ky, kx) order (torch's CPU kernel).  Elements of the rows / columns that the floor
// sizes drop belong to no window: 0.  relu: then 0 where the element itself is <= 0. ----------------------------------------------------------------
struct PoolBwdArgs { const float* x; const float* dp; float* dx; int H, W, C, PH, PW, window, relu; int64_t total; };     // total = n H W C / 4

__global__ __launch_bounds__(TPB) void lpips_maxpool_bwd_kernel(PoolBwdArgs p) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = p.C / 4;
  const int c = (int)(i % c4) * 4;
  const int64_t pix = i / c4;
  const int img = (int)(pix / ((int64_t)p.H * p.W)), r = (int)(pix - (int64_t)img * p.H * p.W);
  const int y = r / p.W, x = r - y * p.W;
  const int wdw = p.window;
  const int py0 = y - wdw + 1 > 0 ? (y - wdw + 2) / 2 : 0, py1 = min(p.PH - 1, y / 2);
  const int px0 = x - wdw + 1 > 0 ? (x - wdw + 2) / 2 : 0, px1 = min(p.PW - 1, x / 2);
  lp_f4 sum = {0.f, 0.f, 0.f, 0.f};
  for (int py = py0; py <= py1; ++py)
    for (int px = px0; px <= px1; ++px) {
      lp_f4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int at0 = -1, at1 = -1, at2 = -1, at3 = -1;
      for (int dy = 0; dy < wdw; ++dy)
        for (int dx = 0; dx < wdw; ++dx) {
          const lp_f4 v = *(const lp_f4*)(p.x + (((int64_t)img * p.H + 2 * py + dy) * p.W + 2 * px + dx) * p.C + c);
          const int id = dy * wdw + dx;
          bool t;
          t = v[0] > m[0] || v[0] != v[0]; m[0] = t ? v[0] : m[0]; at0 = t ? id : at0;
          t = v[1] > m[1] || v[1] != v[1]; m[1] = t ? v[1] : m[1]; at1 = t ? id : at1;
          t = v[2] > m[2] || v[2] != v[2]; m[2] = t ? v[2] : m[2]; at2 = t ? id : at2;
          t = v[3] > m[3] || v[3] != v[3]; m[3] = t ? v[3] : m[3]; at3 = t ? id : at3;
        }
      const int mine = (y - 2 * py) * wdw + (x - 2 * px);
      const lp_f4 gq = *(const lp_f4*)(p.dp + (((int64_t)img * p.PH + py) * p.PW + px) * p.C + c);
      if (at0 == mine) sum[0] += gq[0];
      if (at1 == mine) sum[1] += gq[1];
      if (at2 == mine) sum[2] += gq[2];
      if (at3 == mine) sum[3] += gq[3];
    }
  if (p.relu) {
    const lp_f4 own = *(const lp_f4*)(p.x + pix * p.C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) sum[e] = own[e] <= 0.f ? 0.f : sum[e];
  }
  *(lp_f4*)(p.dx + pix * p.C + c) = sum;
}

// ---- tap backward.  One wave per tap pixel (lane l: channels l, l + 64, ...), F the pred features, s = sqrt(sum F^2), na = F / (s + 1e-10), nb from gt:
//   r_c = 2 omega lin_c (na - nb)_c,   dF_c = (r_c - na_c (sum_j r_j F_j) / s) / (s + 1e-10),   the second term 0 at s == 0;
// g <- [F > 0] (g + dF) with acc, [F > 0] dF without: the tap layer's output feeds the tap and the next layer, and the mask is its own ReLU's. -------
struct TapBwdArgs { const float* fa; const float* fb; const float* lin; int C; int64_t P; float omega2; float* g; int acc; };

__global__ __launch_bounds__(TPB) void lpips_tap_bwd_kernel(TapBwdArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nj = p.C / 64;
  float lin[TAP_MAXC / 64];
#pragma unroll
  for (int j = 0; j < TAP_MAXC / 64; ++j) lin[j] = j < nj ? ieee_mul(p.omega2, p.lin[lane + 64 * j]) : 0.f;
  const int64_t nwaves = (int64_t)gridDim.x * (TPB / 64);
  for (int64_t pix = (int64_t)blockIdx.x * (TPB / 64) + wave; pix < p.P; pix += nwaves) {
    const float* fa = p.fa + pix * p.C;
    const float* fb = p.fb + pix * p.C;
    float a[TAP_MAXC / 64], b[TAP_MAXC / 64], r[TAP_MAXC / 64], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < TAP_MAXC / 64; ++j) {
      a[j] = j < nj ? fa[lane + 64 * j] : 0.f;
      b[j] = j < nj ? fb[lane + 64 * j] : 0.f;
      sa = fmaf(a[j], a[j], sa);
      sb = fmaf(b[j], b[j], sb);
    }
    const float s = sqrtf(wave_sum(sa));
    const float na = ieee_add(s, 1e-10f), nb = ieee_add(sqrtf(wave_sum(sb)), 1e-10f);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < TAP_MAXC / 64; ++j) {
      r[j] = ieee_mul(lin[j], ieee_sub(ieee_div(a[j], na), ieee_div(b[j], nb)));
      dot = fmaf(r[j], a[j], dot);
    }
    dot = wave_sum(dot);
    const float t = s > 0.f ? ieee_div(dot, s) : 0.f;
    float* gp = p.g + pix * p.C;
#pragma unroll
    for (int j = 0; j < TAP_MAXC / 64; ++j)
      if (j < nj) {
        const float d = ieee_div(ieee_sub(r[j], ieee_mul(ieee_div(a[j], na), t)), na);
        const float up = p.acc ? gp[lane + 64 * j] : 0.f;
        gp[lane + 64 * j] = a[j] <= 0.f ? 0.f : ieee_add(up, d);
      }
  }
}

// ---- first layer down to the image.  One thread per input value (n, y, x, c): the outputs whose window covers it in (oy, ox, c_out) order, one fmaf
// chain; w = the forward's packed weights [(ky, kx, c)][C_out].  mode 0: dX as it is; 1: / scale_c; 2: x 2 / scale_c (d of the input scaling). -----
struct Dgrad0Args { const float* dz; const float* w; float* dx; int H, W, OH, OW, Cout, k, stride, pad, mode; int64_t total; };     // total = n H W 3

__global__ __launch_bounds__(TPB) void lpips_dgrad0_kernel(Dgrad0Args p) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= p.total) return;
  const int c = (int)(i % 3);
  const int64_t pix = i / 3;
  const int img = (int)(pix / ((int64_t)p.H * p.W)), r = (int)(pix - (int64_t)img * p.H * p.W);
  const int y = r / p.W, x = r - y * p.W;
  const int ny = y + p.pad - p.k + 1, nx = x + p.pad - p.k + 1;
  const int oy0 = ny > 0 ? (ny + p.stride - 1) / p.stride : 0, oy1 = min(p.OH - 1, (y + p.pad) / p.stride);
  const int ox0 = nx > 0 ? (nx + p.stride - 1) / p.stride : 0, ox1 = min(p.OW - 1, (x + p.pad) / p.stride);
  float acc = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const int ky = y + p.pad - oy * p.stride, kx = x + p.pad - ox * p.stride;
      const float* wrow = p.w + (int64_t)((ky * p.k + kx) * 3 + c) * p.Cout;
      const float* zrow = p.dz + (((int64_t)img * p.OH + oy) * p.OW + ox) * p.Cout;
      for (int co = 0; co < p.Cout; co += 4) {
        const lp_f4 z = *(const lp_f4*)(zrow + co), w = *(const lp_f4*)(wrow + co);
        acc = fmaf(z[0], w[0], acc);
        acc = fmaf(z[1], w[1], acc);
        acc = fmaf(z[2], w[2], acc);
        acc = fmaf(z[3], w[3], acc);
      }
    }
  if (p.mode) {
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    acc = ieee_mul(acc, ieee_div(p.mode == 2 ? 2.f : 1.f, scale));
  }
  p.dx[i] = acc;
}

// ---- for pnrf_lpips_layer_bwd only: dz = dy [y > 0].  In the loss this mask is applied by the kernel that writes the gradient (above). ------------
__global__ __launch_bounds__(TPB) void lpips_relu_bwd_kernel(const float* dy, const float* y, float* dz, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i < total) dz[i] = y[i] <= 0.f ? 0.f : dy[i];
}

// ---- the data gradient's weights from the forward's: wt[((k k - 1 - t) C_out + co) C_in + ci] = w[(t C_in + ci) C_out + co] --------------------------
__global__ __launch_bounds__(TPB) void lpips_flip_weights_kernel(const float* w, float* wt, int kk, int cin, int cout, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const int ci = (int)(i % cin);
  const int64_t rest = i / cin;
  const int co = (int)(rest % cout), tf = (int)(rest / cout);
  wt[i] = w[((int64_t)(kk - 1 - tf) * cin + ci) * cout + co];
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + TPB - 1) / TPB); }

// The second packing, once per handle (one allocation; the null stream, waited for): outside any stream capture.
inline int ensure_dgrad_weights(const pnrf_lpips* hc) {
  pnrf_lpips* h = const_cast<pnrf_lpips*>(hc);
  std::lock_guard<std::mutex> lock(h->mu);
  if (h->d_wt_all) return 0;
  int n;
  const LayerSpec* T = net_table(h->net, &n);
  size_t off[13], total = 0;
  for (int l = 1; l < n; ++l) { off[l] = total; total += (size_t)T[l].k * T[l].k * T[l].cin * T[l].cout; }
  float* d = nullptr;
  PNRF_HIP(hipMalloc((void**)&d, total * sizeof(float)));
  for (int l = 1; l < n; ++l) {
    const int64_t cnt = (int64_t)T[l].k * T[l].k * T[l].cin * T[l].cout;
    hipLaunchKernelGGL(lpips_flip_weights_kernel, dim3(blocks_for(cnt)), dim3(TPB), 0, 0, h->d_w[l], d + off[l], T[l].k * T[l].k, T[l].cin, T[l].cout, cnt);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  if (e != hipSuccess) {
    set_error("pnrf_lpips: packing the data-gradient weights failed: %s", hipGetErrorString(e));
    (void)hipFree(d);
    return (int)e;
  }
  h->d_wt[0] = nullptr;
  for (int l = 1; l < n; ++l) h->d_wt[l] = d + off[l];
  h->d_wt_all = d;
  return 0;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------------
// The data gradient of a layer with few pixels is a handful of workgroups walking the whole K (k k C_out / 32 chunks, one after the other): up to
// SPLIT_MAX_WG workgroups it is split over the filter taps, one tap per grid z, and summed in tap order by lpips_dgrad_reduce_kernel.
constexpr int SPLIT_MAX_WG = 32;
inline bool dgrad_is_split(int M, int cin) { return (int64_t)((M + CT_M - 1) / CT_M) * (cin / CT_N) <= SPLIT_MAX_WG; }
inline int64_t dgrad_part_floats(const LayerSpec& L, int M) { return dgrad_is_split(M, L.cin) ? (int64_t)L.k * L.k * M * L.cin : 0; }

inline int launch_gemm(bool dgrad, const GemmArgs& c, hipStream_t st) {
  const dim3 grid((unsigned)((c.M + CT_M - 1) / CT_M), (unsigned)(c.Cout / CT_N), dgrad && c.part ? (unsigned)(c.k * c.k) : 1u);
  if (dgrad) hipLaunchKernelGGL(lpips_dgrad_kernel, grid, dim3(TPB), 0, st, c);
  else hipLaunchKernelGGL(lpips_loss_conv_kernel, grid, dim3(TPB), 0, st, c);
  PNRF_LAUNCH_CHECK();
  return 0;
}

// dX [n, H, W, C_in] of hidden layer L from dZ [n, OH, OW, C_out]; mask: the activation at dX's address or NULL
// part: room for dgrad_part_floats(L, n H W) floats
inline int launch_dgrad(const pnrf_lpips* h, int layer, const LayerSpec& L, const float* dz, int n, int H, int W, int OH, int OW, const float* mask, float* dx,
                        float* part, hipStream_t st) {
  GemmArgs c;
  c.x = dz; c.w = h->d_wt[layer]; c.bias = nullptr; c.mask = mask; c.y = dx;
  c.H = OH; c.W = OW; c.Cin = L.cout; c.OH = H; c.OW = W; c.Cout = L.cin; c.k = L.k; c.stride = 1; c.pad = L.k - 1 - L.pad;
  c.M = n * H * W;
  c.part = dgrad_is_split(c.M, L.cin) ? part : nullptr;
  const int rc = launch_gemm(true, c, st);
  if (rc || !c.part) return rc;
  DgradReduceArgs r;
  r.part = part; r.mask = mask; r.y = dx; r.taps = L.k * L.k; r.plane = (int64_t)c.M * L.cin; r.total4 = r.plane / 4;
  hipLaunchKernelGGL(lpips_dgrad_reduce_kernel, dim3(blocks_for(r.total4)), dim3(TPB), 0, st, r);
  PNRF_LAUNCH_CHECK();
  return 0;
}

inline int launch_dgrad0(const pnrf_lpips* h, const LayerSpec& L, const float* dz, int n, int H, int W, int OH, int OW, int mode, float* dx, hipStream_t st) {
  Dgrad0Args a;
  a.dz = dz; a.w = h->d_w[0]; a.dx = dx; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.Cout = L.cout; a.k = L.k; a.stride = L.stride; a.pad = L.pad; a.mode = mode;
  a.total = (int64_t)n * H * W * 3;
  hipLaunchKernelGGL(lpips_dgrad0_kernel, dim3(blocks_for(a.total)), dim3(TPB), 0, st, a);
  PNRF_LAUNCH_CHECK();
  return 0;
}

inline int launch_pool_bwd(const float* x, const float* dp, float* dx, int n, int H, int W, int C, int window, int relu, hipStream_t st) {
  PoolBwdArgs q;
  q.x = x; q.dp = dp; q.dx = dx; q.H = H; q.W = W; q.C = C; q.PH = pool_out(H, window); q.PW = pool_out(W, window); q.window = window; q.relu = relu;
  q.total = (int64_t)n * H * W * (C / 4);
  hipLaunchKernelGGL(lpips_maxpool_bwd_kernel, dim3(blocks_for(q.total)), dim3(TPB), 0, st, q);
  PNRF_LAUNCH_CHECK();
  return 0;
}

inline int launch_tap_bwd(const float* fa, const float* fb, const float* lin, int C, int64_t P, float* g, int acc, hipStream_t st) {
  TapBwdArgs t;
  t.fa = fa; t.fb = fb; t.lin = lin; t.C = C; t.P = P; t.omega2 = (float)(2.0 / (double)P); t.g = g; t.acc = acc;
  const int64_t want = (P + TPB / 64 - 1) / (TPB / 64);
  hipLaunchKernelGGL(lpips_tap_bwd_kernel, dim3((unsigned)(want < TAP_MAXB ? want : TAP_MAXB)), dim3(TPB), 0, st, t);
  PNRF_LAUNCH_CHECK();
  return 0;
}

// Sizes of a loss call.  Offsets in floats behind the partial sums, every piece a multiple of 64 floats.
struct LossPlan {
  int h[13], w[13];          // output of conv l
  int ph[13], pw[13];        // its input (behind the pooling, if any)
  int64_t y_off[13];         // saved output of conv l, [2 B, h, w, C_out]
  int64_t tmp_off, g_off[2]; // pooled activations / gathered rows of the forward, per-tap sums of a split data gradient; the two gradient buffers (pred half)
  int64_t total;             // floats
};
inline int64_t align64(int64_t n) { return (n + 63) / 64 * 64; }
inline void make_loss_plan(int id, int B, int H, int W, LossPlan* pl) {
  int n;
  const LayerSpec* T = net_table(id, &n);
  int64_t tmp = 0, gmax = 0, off = 0;
  int h = H, w = W;
  for (int l = 0; l < n; ++l) {
    const LayerSpec& L = T[l];
    if (L.pool) {
      h = pool_out(h, L.pool); w = pool_out(w, L.pool);
      tmp = std::max(tmp, (int64_t)2 * B * h * w * L.cin);
      gmax = std::max(gmax, (int64_t)B * h * w * L.cin);
    }
    pl->ph[l] = h; pl->pw[l] = w;
    if (L.cin != 3) tmp = std::max(tmp, dgrad_part_floats(L, B * h * w));
    h = conv_out(h, L); w = conv_out(w, L);
    if (L.cin == 3) tmp = std::max(tmp, (int64_t)2 * B * h * w * k_padded(L));
    pl->h[l] = h; pl->w[l] = w;
    pl->y_off[l] = off; off += align64((int64_t)2 * B * h * w * L.cout);
    gmax = std::max(gmax, (int64_t)B * h * w * L.cout);
  }
  pl->tmp_off = off; off += align64(tmp);
  pl->g_off[0] = off; off += align64(gmax);
  pl->g_off[1] = off; off += align64(gmax);
  pl->total = off;
}
inline bool loss_size_ok(const pnrf_lpips* h, int B, int H, int W) {
  return h && B >= 1 && size_ok(h->net, H, W) && (int64_t)2 * B * H * W <= 0x7fffffffLL;
}

}  // namespace

extern "C" int64_t pnrf_lpips_loss_workspace_bytes(const pnrf_lpips_t* h, int B, int H, int W) {
  if (!loss_size_ok(h, B, H, W) || ensure_dgrad_weights(h)) return 0;
  LossPlan pl;
  make_loss_plan(h->net, B, H, W, &pl);
  return PARTIAL_BYTES + pl.total * (int64_t)sizeof(float);
}

extern "C" int pnrf_lpips_loss_fwd(const pnrf_lpips_t* h, const float* pred, int pred_stride, int64_t pred_patch_stride, const float* gt, int gt_stride,
                                   int64_t gt_patch_stride, int B, int H, int W, int normalize, double* out, float* d_pred, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_lpips_loss_fwd: null handle");
  PNRF_REQUIRE(pred && gt && out && d_pred && workspace, PNRF_E_ARG, "pnrf_lpips_loss_fwd: null pointer (pred, gt, out, d_pred and workspace are required)");
  PNRF_REQUIRE(pred_stride >= 3 && gt_stride >= 3 && pred_patch_stride >= 0 && gt_patch_stride >= 0, PNRF_E_ARG,
               "pnrf_lpips_loss_fwd: pixel strides %d / %d (need >= 3 floats), patch strides %lld / %lld (need >= 0)", pred_stride, gt_stride,
               (long long)pred_patch_stride, (long long)gt_patch_stride);
  PNRF_REQUIRE(B >= 1 && size_ok(h->net, H, W), PNRF_E_ARG, "pnrf_lpips_loss_fwd: %d patches of %d x %d: need B >= 1 and %d .. %d pixels per side for '%s'", B, H, W,
               min_dim(h->net), MAX_DIM, h->net == 0 ? "alex" : "vgg");
  PNRF_REQUIRE(loss_size_ok(h, B, H, W), PNRF_E_ARG, "pnrf_lpips_loss_fwd: 2 x %d x %d x %d pixels do not fit the kernels' 32-bit pixel index", B, H, W);
  const int64_t need = pnrf_lpips_loss_workspace_bytes(h, B, H, W);
  PNRF_REQUIRE(need > 0, PNRF_E_ARG, "pnrf_lpips_loss_fwd: the data-gradient weights of the handle could not be made");
  PNRF_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, PNRF_E_ARG,
               "pnrf_lpips_loss_fwd: workspace of %lld bytes (16-byte aligned) needed, got %lld", (long long)need, (long long)workspace_bytes);
  const hipStream_t st = (hipStream_t)stream;
  LossPlan pl;
  make_loss_plan(h->net, B, H, W, &pl);
  double* partial = (double*)workspace;
  float* base = (float*)((char*)workspace + PARTIAL_BYTES);
  float* tmp = base + pl.tmp_off;
  float* gbuf[2] = {base + pl.g_off[0], base + pl.g_off[1]};
  int n;
  const LayerSpec* T = net_table(h->net, &n);
  // ---- forward: the batch of 2 B images, every conv output kept
  FinishArgs fin;
  fin.partial = partial; fin.out = out;
  const float* x = nullptr;
  int hh = H, ww = W;
  for (int l = 0; l < n; ++l) {
    const LayerSpec& L = T[l];
    float* y = base + pl.y_off[l];
    GemmArgs c;
    c.w = h->d_w[l]; c.bias = h->d_b[l]; c.mask = nullptr; c.part = nullptr; c.y = y; c.OH = pl.h[l]; c.OW = pl.w[l]; c.Cout = L.cout; c.M = 2 * B * pl.h[l] * pl.w[l];
    if (L.cin == 3) {
      Im2colPatchArgs a;
      a.a = pred; a.b = gt; a.sa = pred_stride; a.sb = gt_stride; a.pa = pred_patch_stride; a.pb = gt_patch_stride; a.B = B; a.H = H; a.W = W;
      a.OH = pl.h[l]; a.OW = pl.w[l]; a.k = L.k; a.stride = L.stride; a.pad = L.pad; a.K = L.k * L.k * 3; a.Kp = k_padded(L); a.mode = normalize ? 2 : 1;
      a.out = tmp; a.total = (int64_t)2 * B * a.OH * a.OW * a.Kp;
      hipLaunchKernelGGL(lpips_im2col_patch_kernel, dim3(blocks_for(a.total)), dim3(TPB), 0, st, a);
      PNRF_LAUNCH_CHECK();
      c.x = tmp; c.H = a.OH; c.W = a.OW; c.Cin = a.Kp; c.k = 1; c.stride = 1; c.pad = 0;
    } else {
      if (L.pool) {
        PoolArgs q;
        q.x = x; q.y = tmp; q.H = hh; q.W = ww; q.C = L.cin; q.PH = pl.ph[l]; q.PW = pl.pw[l]; q.window = L.pool;
        q.total = (int64_t)2 * B * q.PH * q.PW * (L.cin / 4);
        hipLaunchKernelGGL(lpips_loss_maxpool_kernel, dim3(blocks_for(q.total)), dim3(TPB), 0, st, q);
        PNRF_LAUNCH_CHECK();
        x = tmp;
      }
      c.x = x; c.H = pl.ph[l]; c.W = pl.pw[l]; c.Cin = L.cin; c.k = L.k; c.stride = L.stride; c.pad = L.pad;
    }
    const int rc = launch_gemm(false, c, st);
    if (rc) return rc;
    x = y; hh = pl.h[l]; ww = pl.w[l];
    if (L.tap >= 0) {
      TapArgs t;
      t.f = y; t.lin = h->d_lin[L.tap]; t.C = L.cout; t.P = (int64_t)B * hh * ww; t.map = nullptr; t.partial = partial + L.tap * TAP_MAXB;
      const int64_t want = (t.P + TPB / 64 - 1) / (TPB / 64);
      const int nb = (int)(want < TAP_MAXB ? want : TAP_MAXB);
      hipLaunchKernelGGL(lpips_tap_kernel, dim3(nb), dim3(TPB), 0, st, t);
      PNRF_LAUNCH_CHECK();
      fin.nb[L.tap] = nb; fin.P[L.tap] = (double)t.P;
    }
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(TPB), 0, st, fin);
  PNRF_LAUNCH_CHECK();
  // ---- backward: the pred half, top layer down; gbuf[cur] = dZ of layer l as far as the layers above have written it
  int cur = 0;
  for (int l = n - 1; l >= 0; --l) {
    const LayerSpec& L = T[l];
    const float* y = base + pl.y_off[l];
    const int64_t P = (int64_t)B * pl.h[l] * pl.w[l];
    int rc = 0;
    if (L.tap >= 0) rc = launch_tap_bwd(y, y + P * L.cout, h->d_lin[L.tap], L.cout, P, gbuf[cur], l < n - 1, st);
    if (rc) return rc;
    if (l == 0) return launch_dgrad0(h, L, gbuf[cur], B, H, W, pl.h[0], pl.w[0], normalize ? 2 : 1, d_pred, st);
    const float* below = base + pl.y_off[l - 1];
    rc = launch_dgrad(h, l, L, gbuf[cur], B, pl.ph[l], pl.pw[l], pl.h[l], pl.w[l], L.pool ? nullptr : below, gbuf[cur ^ 1], tmp, st);
    if (rc) return rc;
    cur ^= 1;
    if (L.pool) {
      rc = launch_pool_bwd(below, gbuf[cur], gbuf[cur ^ 1], B, pl.h[l - 1], pl.w[l - 1], L.cin, L.pool, 1, st);
      if (rc) return rc;
      cur ^= 1;
    }
  }
  return 0;
}

// ---- for tests: one layer's backward, one tap's backward ----------------------------------------------------------------------------------------
namespace {
struct LayerBwdPlan { int ph, pw, oh, ow; int64_t dz, dp, part; };    // floats of the masked gradient / of the gradient behind the pooling / of the per-tap sums
inline bool layer_bwd_plan(const pnrf_lpips* h, int layer, int pool_first, int n, int H, int W, LayerBwdPlan* q) {
  if (!h || layer < 0 || layer >= h->n || n < 1 || H < 1 || W < 1 || H > MAX_DIM || W > MAX_DIM || (int64_t)n * H * W > 0x7fffffffLL) return false;
  int nn;
  const LayerSpec& L = net_table(h->net, &nn)[layer];
  if (pool_first && (!L.pool || H < L.pool || W < L.pool)) return false;
  q->ph = pool_first ? pool_out(H, L.pool) : H; q->pw = pool_first ? pool_out(W, L.pool) : W;
  if (q->ph + 2 * L.pad < L.k || q->pw + 2 * L.pad < L.k) return false;
  q->oh = conv_out(q->ph, L); q->ow = conv_out(q->pw, L);
  q->dz = align64((int64_t)n * q->oh * q->ow * L.cout);
  q->dp = pool_first ? align64((int64_t)n * q->ph * q->pw * L.cin) : 0;
  q->part = L.cin != 3 ? dgrad_part_floats(L, n * q->ph * q->pw) : 0;
  return true;
}
}  // namespace

extern "C" int64_t pnrf_lpips_layer_bwd_workspace_bytes(const pnrf_lpips_t* h, int layer, int pool_first, int n, int H, int W) {
  LayerBwdPlan q;
  if (!layer_bwd_plan(h, layer, pool_first, n, H, W, &q) || ensure_dgrad_weights(h)) return 0;
  return (q.dz + q.dp + q.part) * (int64_t)sizeof(float);
}

extern "C" int pnrf_lpips_layer_bwd(const pnrf_lpips_t* h, int layer, int pool_first, int relu_in, int n, const float* x, int H, int W, const float* y,
                                    const float* dy, float* dx, void* workspace, int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_lpips_layer_bwd: null handle");
  PNRF_REQUIRE(x && y && dy && dx && workspace, PNRF_E_ARG, "pnrf_lpips_layer_bwd: null pointer");
  LayerBwdPlan q;
  PNRF_REQUIRE(layer_bwd_plan(h, layer, pool_first, n, H, W, &q), PNRF_E_ARG,
               "pnrf_lpips_layer_bwd: layer %d (pool_first %d) with %d inputs of %d x %d: no such layer / pooling, or the input is smaller than the window or filter", layer,
               pool_first, n, H, W);
  PNRF_REQUIRE(!(relu_in && layer == 0), PNRF_E_ARG, "pnrf_lpips_layer_bwd: layer 0 reads the image, there is no ReLU below it");
  const int64_t need = pnrf_lpips_layer_bwd_workspace_bytes(h, layer, pool_first, n, H, W);
  PNRF_REQUIRE(need > 0 && workspace_bytes >= need, PNRF_E_ARG, "pnrf_lpips_layer_bwd: workspace of %lld bytes needed, got %lld", (long long)need, (long long)workspace_bytes);
  PNRF_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)workspace) & 15) == 0, PNRF_E_ARG, "pnrf_lpips_layer_bwd: every pointer must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  int nn;
  const LayerSpec& L = net_table(h->net, &nn)[layer];
  float* dz = (float*)workspace;
  float* dp = dz + q.dz;
  float* part = dp + q.dp;
  const int64_t cnt = (int64_t)n * q.oh * q.ow * L.cout;
  hipLaunchKernelGGL(lpips_relu_bwd_kernel, dim3(blocks_for(cnt)), dim3(TPB), 0, st, dy, y, dz, cnt);
  PNRF_LAUNCH_CHECK();
  if (layer == 0) return launch_dgrad0(h, L, dz, n, H, W, q.oh, q.ow, 0, dx, st);
  if (!pool_first) return launch_dgrad(h, layer, L, dz, n, H, W, q.oh, q.ow, relu_in ? x : nullptr, dx, part, st);
  const int rc = launch_dgrad(h, layer, L, dz, n, q.ph, q.pw, q.oh, q.ow, nullptr, dp, part, st);
  if (rc) return rc;
  return launch_pool_bwd(x, dp, dx, n, H, W, L.cin, L.pool, relu_in, st);
}

extern "C" int pnrf_lpips_tap_bwd(const pnrf_lpips_t* h, int tap, const float* f_pred, const float* f_gt, int64_t P, float* d_f, void* stream) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_lpips_tap_bwd: null handle");
  PNRF_REQUIRE(tap >= 0 && tap < 5, PNRF_E_ARG, "pnrf_lpips_tap_bwd: tap %d outside 0 .. 4", tap);
  PNRF_REQUIRE(f_pred && f_gt && d_f, PNRF_E_ARG, "pnrf_lpips_tap_bwd: null pointer");
  PNRF_REQUIRE(P >= 1 && P <= 0x7fffffffLL, PNRF_E_ARG, "pnrf_lpips_tap_bwd: %lld pixels outside 1 .. 2^31 - 1", (long long)P);
  int n, C = 0;
  const LayerSpec* T = net_table(h->net, &n);
  for (int l = 0; l < n; ++l)
    if (T[l].tap == tap) C = T[l].cout;
  return launch_tap_bwd(f_pred, f_gt, h->d_lin[tap], C, P, d_f, 0, (hipStream_t)stream);
}
