// pnrf_lpips.hip — LPIPS (version 0.1, nets 'alex' and 'vgg') of an image pair on the device: the backbone's convolutions as an implicit GEMM on the
// exact-fp32 MFMA, max pooling, and per tap the unit normalisation, the squared difference and the 1 x 1 'lin' layer (pnrf_lpips_fwd).
// Nothing here is shared with the fused-MLP units.
//
// Arithmetic.  Every product is v_mfma_f32_16x16x4_f32: an fp32 fmaf chain in k order, one rounding per product, fp32 range — so a backbone whose
// activations are far above O(1) needs no operand scaling (the split-fp16 scheme of pnrf_hgemm.h would: its planes are fp16).  The price is the fp32
// MFMA rate, 1/16 of the 16-bit one; DESIGN §4.8 has the measured times.
//
// Layout.  The two images run as a batch of two through every kernel.  Activations are dense NHWC fp32 [2, H, W, C]; a filter tap outside the image is
// a predicated load that returns zeros.  Every hidden C_in is a multiple of 32 and every C_out one of 64.  A convolution is C^T = W X^T with
//   M = 2 OH OW output pixels,  N = C_out,  K = (ky, kx, c_in) in that order,
// the weights packed once at handle creation as [K][C_out] (a tile's rows are whole 256-byte segments).  The two 3-channel first layers (K = 27, 363)
// go through an explicit gather (im2col_kernel, fused with the 2x - 1 / shift / scale step) into rows of K padded to 32 / 384, and are then a 1 x 1
// convolution of the same kernel.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "pnrf_common.h"
#include "pnrf_ieee.h"

using namespace pnrf;

struct pnrf_lpips {
  int net;               // 0 alex, 1 vgg
  int n;                 // conv layers
  float* d_all;          // one allocation: packed weights, biases, lin
  float* d_w[13];        // [K padded][C_out]
  float* d_b[13];
  float* d_lin[5];
  int device;
  // the loss: every hidden layer's weights a second time, flipped and transposed for the data gradient, [k k C_out][C_in]; made by the first loss call
  std::mutex mu;
  float* d_wt_all;
  float* d_wt[13];
};

namespace {

typedef float lp_f4 __attribute__((ext_vector_type(4)));

constexpr int MAX_DIM = PNRF_LPIPS_MAX_DIM;
constexpr int TPB = 256;

struct LayerSpec { int cin, cout, k, stride, pad, pool, tap; };     // pool: window of the max pooling (stride 2) in front of the conv, 0 = none; tap: 0 .. 4 or -1
constexpr LayerSpec ALEX[5] = {{3, 64, 11, 4, 2, 0, 0}, {64, 192, 5, 1, 2, 3, 1}, {192, 384, 3, 1, 1, 3, 2}, {384, 256, 3, 1, 1, 0, 3}, {256, 256, 3, 1, 1, 0, 4}};
constexpr LayerSpec VGG[13] = {{3, 64, 3, 1, 1, 0, -1},    {64, 64, 3, 1, 1, 0, 0},    {64, 128, 3, 1, 1, 2, -1},  {128, 128, 3, 1, 1, 0, 1},  {128, 256, 3, 1, 1, 2, -1},
                               {256, 256, 3, 1, 1, 0, -1}, {256, 256, 3, 1, 1, 0, 2},  {256, 512, 3, 1, 1, 2, -1}, {512, 512, 3, 1, 1, 0, -1}, {512, 512, 3, 1, 1, 0, 3},
                               {512, 512, 3, 1, 1, 2, -1}, {512, 512, 3, 1, 1, 0, -1}, {512, 512, 3, 1, 1, 0, 4}};
constexpr int MIN_ALEX = 31, MIN_VGG = 16;
const char* const TABLE_ALEX = "Table of 'alex': conv [64,3,11,11] [192,64,5,5] [384,192,3,3] [256,384,3,3] [256,256,3,3], lin 64 192 384 256 256";
const char* const TABLE_VGG =
    "Table of 'vgg': conv [64,3,3,3] [64,64,3,3] [128,64,3,3] [128,128,3,3] [256,128,3,3] [256,256,3,3] x2 [512,256,3,3] [512,512,3,3] x5, lin 64 128 256 512 512";

inline int net_id(const char* net) {
  if (!net) return -1;
  if (!strcmp(net, "alex")) return 0;
  if (!strcmp(net, "vgg")) return 1;
  return -1;
}
inline const LayerSpec* net_table(int id, int* n) {
  *n = id == 0 ? 5 : 13;
  return id == 0 ? ALEX : VGG;
}
inline int min_dim(int id) { return id == 0 ? MIN_ALEX : MIN_VGG; }
inline bool size_ok(int id, int H, int W) { return H >= min_dim(id) && W >= min_dim(id) && H <= MAX_DIM && W <= MAX_DIM; }
inline int conv_out(int n, const LayerSpec& L) { return (n + 2 * L.pad - L.k) / L.stride + 1; }
inline int pool_out(int n, int window) { return (n - window) / 2 + 1; }
inline int k_padded(const LayerSpec& L) { return L.cin == 3 ? (L.k * L.k * 3 + 31) / 32 * 32 : L.k * L.k * L.cin; }
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// ---- first layer: gather into rows of K = (ky, kx, c) padded with zeros, with the input scaling ----------------------------------------------
struct Im2colArgs {
  const float *a, *b;    // the two images, pixel (y, x) channel c at [(y W + x) stride + c]
  int sa, sb;
  int H, W, OH, OW, k, stride, pad, K, Kp;
  int mode;              // 0: values as they are (pnrf_lpips_layer_fwd); 1: (x - shift) / scale; 2: (2 x - 1 - shift) / scale
  float* out;            // [2 OH OW][Kp]
  int64_t total;         // 2 OH OW Kp
};

__global__ __launch_bounds__(TPB) void lpips_im2col_kernel(Im2colArgs p) {
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
      const float* src = img ? p.b : p.a;
      v = src[((int64_t)iy * p.W + ix) * (img ? p.sb : p.sa) + c];
      if (p.mode) {
        const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f), scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
        if (p.mode == 2) v = ieee_sub(ieee_mul(2.f, v), 1.f);
        v = ieee_div(ieee_sub(v, shift), scale);
      }
    }
  }
  p.out[i] = v;
}

// ---- convolution + bias + ReLU ------------------------------------------------------------------------------------------------------------
// Workgroup = 4 waves on a tile of 64 pixels x 64 channels; wave (wm, wn) owns 32 x 32 of it = 2 x 2 MFMA tiles.  The weight fragment is the
// MFMA's A operand (rows = channels), the activation fragment its B operand (columns = pixels): D register e of lane (l16, g) is
// channel 4 g + e of pixel l16, so a lane stores 16 contiguous bytes of its pixel's NHWC row.
// K loop: chunks of 32 channels of one filter tap.  The next chunk is fetched into registers while the MFMAs of the current one run; one LDS
// buffer, two barriers per chunk.  LDS pitches: [pixel][32 + 4] and [k][64 + 16] floats — the fragment reads of a wave (16 pixels x 4 k, 4 k x 16
// channels) fall on 64 different banks.
constexpr int CT_M = 64, CT_N = 64, CT_K = 32, SX_LD = CT_K + 4, SW_LD = CT_N + 16;

struct ConvArgs {
  const float* x;        // [2, H, W, Cin]
  const float* w;        // [k k Cin][Cout]
  const float* bias;     // [Cout]
  float* y;              // [2, OH, OW, Cout]
  int H, W, Cin, OH, OW, Cout, k, stride, pad;
  int M;                 // 2 OH OW
};

__global__ __launch_bounds__(TPB) void lpips_conv_kernel(ConvArgs p) {
  __shared__ __attribute__((aligned(16))) float sX[CT_M * SX_LD];
  __shared__ __attribute__((aligned(16))) float sW[CT_K * SW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * CT_M, n0 = blockIdx.y * CT_N;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  // loaders: activations — pixels (tid >> 3) and + 32 of the tile, channels 4 (tid & 7) .. + 3 of the chunk; weights — rows (tid >> 4) and + 16, columns 4 (tid & 15) .. + 3
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
  const int cchunks = p.Cin / CT_K, total = p.k * p.k * cchunks;
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
    for (int ps = 0; ps < 2; ++ps) rw[ps] = *(const lp_f4*)(p.w + ((int64_t)q * CT_K + wr + 16 * ps) * p.Cout + n0 + wc);      // row q 32 + r = (tap, channel) in K order
  };
  fetch(0);
  for (int q = 0; q < total; ++q) {
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
    const lp_f4 bias4 = *(const lp_f4*)(p.bias + c);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm + 16 * j + l16;
      if (m < p.M) {
        lp_f4 v = acc[i][j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(ieee_add(v[e], bias4[e]), 0.f);
        *(lp_f4*)(p.y + (int64_t)m * p.Cout + c) = v;
      }
    }
  }
}

// ---- max pooling, window 2 or 3, stride 2, no padding, floor sizes: every window lies inside the image -----------------------------------------
struct PoolArgs { const float* x; float* y; int H, W, C, PH, PW, window; int64_t total; };    // total = 2 PH PW C / 4

__global__ __launch_bounds__(TPB) void lpips_maxpool_kernel(PoolArgs p) {
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
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  *(lp_f4*)(p.y + pix * p.C + c) = m;
}

// ---- tap: m[y, x] = sum_c lin[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 --------------------------------------------------------------
// One wave per pixel (lane l holds channels l, l + 64, ...; C <= 512), sums over the wave as a butterfly — the same bits in every lane and for
// (a, b) as for (b, a).  Every wave adds its pixels' values in fp64, the workgroup's four sums go to the workspace in wave order.
constexpr int TAP_MAXB = 1024;           // workgroups of a tap kernel; the grid is a function of the pixel count alone
constexpr int TAP_MAXC = 512;

struct TapArgs { const float* f; const float* lin; int C; int64_t P; float* map; double* partial; };      // f: [2, P, C]

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(TPB) void lpips_tap_kernel(TapArgs p) {
  __shared__ double s_red[TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nj = p.C / 64;
  float lin[TAP_MAXC / 64];
#pragma unroll
  for (int j = 0; j < TAP_MAXC / 64; ++j) lin[j] = j < nj ? p.lin[lane + 64 * j] : 0.f;
  double sum = 0.0;
  const int64_t nwaves = (int64_t)gridDim.x * (TPB / 64);
  for (int64_t pix = (int64_t)blockIdx.x * (TPB / 64) + wave; pix < p.P; pix += nwaves) {
    const float* fa = p.f + pix * p.C;
    const float* fb = p.f + (p.P + pix) * p.C;
    float a[TAP_MAXC / 64], b[TAP_MAXC / 64], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < TAP_MAXC / 64; ++j) {
      a[j] = j < nj ? fa[lane + 64 * j] : 0.f;
      b[j] = j < nj ? fb[lane + 64 * j] : 0.f;
      sa = fmaf(a[j], a[j], sa);
      sb = fmaf(b[j], b[j], sb);
    }
    const float na = ieee_add(sqrtf(wave_sum(sa)), 1e-10f), nb = ieee_add(sqrtf(wave_sum(sb)), 1e-10f);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < TAP_MAXC / 64; ++j) {
      const float d = ieee_sub(ieee_div(a[j], na), ieee_div(b[j], nb));
      s = ieee_add(s, ieee_mul(lin[j], ieee_mul(d, d)));        // no contraction: d^2 must not depend on the sign of d through a fused product's rounding
    }
    s = wave_sum(s);
    if (lane == 0 && p.map) p.map[pix] = s;
    sum += (double)s;
  }
  if (lane == 0) s_red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

struct FinishArgs { const double* partial; int nb[5]; double P[5]; double* out; };

// One workgroup: per tap the workgroups' partial sums in index order per thread, then a tree over LDS; d = the five means added in tap order.
__global__ __launch_bounds__(TPB) void lpips_finish_kernel(FinishArgs p) {
  __shared__ double s_red[TPB];
  const int t = threadIdx.x;
  double d = 0.0;
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int j = t; j < p.nb[k]; j += TPB) s += p.partial[k * TAP_MAXB + j];
    s_red[t] = s;
    __syncthreads();
    for (int h = TPB / 2; h > 0; h >>= 1) {
      if (t < h) s_red[t] += s_red[t + h];
      __syncthreads();
    }
    const double mean = s_red[0] / p.P[k];
    __syncthreads();
    if (t == 0) p.out[1 + k] = mean;
    d += mean;
  }
  if (t == 0) p.out[0] = d;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------------
inline int launch_conv(const pnrf_lpips* h, int layer, const float* x, int H, int W, int Cin, int k, int stride, int pad, float* y, int OH, int OW, hipStream_t st) {
  int n;
  const LayerSpec& L = net_table(h->net, &n)[layer];
  ConvArgs c;
  c.x = x; c.w = h->d_w[layer]; c.bias = h->d_b[layer]; c.y = y;
  c.H = H; c.W = W; c.Cin = Cin; c.OH = OH; c.OW = OW; c.Cout = L.cout; c.k = k; c.stride = stride; c.pad = pad;
  c.M = 2 * OH * OW;
  hipLaunchKernelGGL(lpips_conv_kernel, dim3((unsigned)((c.M + CT_M - 1) / CT_M), (unsigned)(L.cout / CT_N)), dim3(TPB), 0, st, c);
  PNRF_LAUNCH_CHECK();
  return 0;
}

// One layer from a dense NHWC pair (hidden layers) or from two strided 3-channel images (layer 0): [pool] -> [gather] -> conv + bias + ReLU -> y.
// tmp: room for the pooled activations / the gathered rows.  (OH, OW) of y are returned.
inline int run_layer(const pnrf_lpips* h, int layer, bool pool, const float* x, const float* xb, int sa, int sb, int mode, int H, int W, float* tmp, float* y,
                     int* OH, int* OW, hipStream_t st) {
  int n;
  const LayerSpec& L = net_table(h->net, &n)[layer];
  if (L.cin == 3) {
    const int oh = conv_out(H, L), ow = conv_out(W, L);
    Im2colArgs a;
    a.a = x; a.b = xb; a.sa = sa; a.sb = sb; a.H = H; a.W = W; a.OH = oh; a.OW = ow; a.k = L.k; a.stride = L.stride; a.pad = L.pad;
    a.K = L.k * L.k * 3; a.Kp = k_padded(L); a.mode = mode; a.out = tmp; a.total = (int64_t)2 * oh * ow * a.Kp;
    hipLaunchKernelGGL(lpips_im2col_kernel, dim3((unsigned)((a.total + TPB - 1) / TPB)), dim3(TPB), 0, st, a);
    PNRF_LAUNCH_CHECK();
    *OH = oh; *OW = ow;
    return launch_conv(h, layer, tmp, oh, ow, a.Kp, 1, 1, 0, y, oh, ow, st);
  }
  if (pool) {
    PoolArgs q;
    q.x = x; q.y = tmp; q.H = H; q.W = W; q.C = L.cin; q.PH = pool_out(H, L.pool); q.PW = pool_out(W, L.pool); q.window = L.pool;
    q.total = (int64_t)2 * q.PH * q.PW * (L.cin / 4);
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)((q.total + TPB - 1) / TPB)), dim3(TPB), 0, st, q);
    PNRF_LAUNCH_CHECK();
    x = tmp; H = q.PH; W = q.PW;
  }
  *OH = conv_out(H, L); *OW = conv_out(W, L);
  return launch_conv(h, layer, x, H, W, L.cin, L.k, L.stride, L.pad, y, *OH, *OW, st);
}

// Sizes of a forward call: the tap planes and the largest buffer (in floats) any step writes.
struct Plan { int hw[5][2]; int64_t max_elems; };
inline void make_plan(int id, int H, int W, Plan* pl) {
  int n;
  const LayerSpec* T = net_table(id, &n);
  int64_t mx = 0;
  int h = H, w = W;
  for (int l = 0; l < n; ++l) {
    const LayerSpec& L = T[l];
    if (L.pool) {
      h = pool_out(h, L.pool); w = pool_out(w, L.pool);
      mx = std::max(mx, (int64_t)2 * h * w * L.cin);
    }
    h = conv_out(h, L); w = conv_out(w, L);
    if (L.cin == 3) mx = std::max(mx, (int64_t)2 * h * w * k_padded(L));
    mx = std::max(mx, (int64_t)2 * h * w * L.cout);
    if (L.tap >= 0) { pl->hw[L.tap][0] = h; pl->hw[L.tap][1] = w; }
  }
  pl->max_elems = mx;
}
constexpr int64_t PARTIAL_BYTES = 5 * TAP_MAXB * (int64_t)sizeof(double);

// Copy n floats that lie on the host or on a device to the host.
inline int to_host(float* dst, const float* src, size_t n) {
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, src);
  if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
    (void)hipGetLastError();                     // an unregistered host pointer is reported as an error: not one
    memcpy(dst, src, n * sizeof(float));
    return 0;
  }
  PNRF_HIP(hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int pnrf_lpips_tap_dims(const char* net, int H, int W, int* hw) {
  const int id = net_id(net);
  PNRF_REQUIRE(id >= 0, PNRF_E_ARG, "pnrf_lpips_tap_dims: unknown net '%s' (alex, vgg)", net ? net : "(null)");
  PNRF_REQUIRE(hw, PNRF_E_ARG, "pnrf_lpips_tap_dims: null pointer");
  PNRF_REQUIRE(size_ok(id, H, W), PNRF_E_ARG, "pnrf_lpips_tap_dims: image of %d x %d outside %d .. %d per side for '%s'", H, W, min_dim(id), MAX_DIM, net);
  Plan pl;
  make_plan(id, H, W, &pl);
  for (int k = 0; k < 5; ++k) { hw[2 * k] = pl.hw[k][0]; hw[2 * k + 1] = pl.hw[k][1]; }
  return 0;
}

extern "C" int pnrf_lpips_create(const char* net, const float* const* conv_w, const float* const* conv_b, const int* conv_shape, int n_conv,
                                 const float* const* lin_w, const int* lin_dim, pnrf_lpips_t** out) {
  PNRF_REQUIRE(out, PNRF_E_ARG, "pnrf_lpips_create: null pointer (out)");
  *out = nullptr;
  const int id = net_id(net);
  PNRF_REQUIRE(id >= 0, PNRF_E_ARG, "pnrf_lpips_create: unknown net '%s' (alex, vgg)", net ? net : "(null)");
  PNRF_REQUIRE(conv_w && conv_b && conv_shape && lin_w && lin_dim, PNRF_E_ARG, "pnrf_lpips_create: null pointer");
  int n;
  const LayerSpec* T = net_table(id, &n);
  const char* const TABLE_TEXT = id == 0 ? TABLE_ALEX : TABLE_VGG;
  PNRF_REQUIRE(n_conv == n, PNRF_E_SHAPE, "pnrf_lpips_create: %d conv layers, '%s' has %d.  %s", n_conv, net, n, TABLE_TEXT);
  int tap_c[5] = {0, 0, 0, 0, 0};
  for (int l = 0; l < n; ++l) {
    const int* s = conv_shape + 4 * l;
    PNRF_REQUIRE(s[0] == T[l].cout && s[1] == T[l].cin && s[2] == T[l].k && s[3] == T[l].k, PNRF_E_SHAPE,
                 "pnrf_lpips_create: conv %d of '%s' is [%d,%d,%d,%d], expected [%d,%d,%d,%d].  %s", l, net, s[0], s[1], s[2], s[3], T[l].cout, T[l].cin, T[l].k,
                 T[l].k, TABLE_TEXT);
    PNRF_REQUIRE(conv_w[l] && conv_b[l], PNRF_E_ARG, "pnrf_lpips_create: null pointer (conv %d)", l);
    if (T[l].tap >= 0) tap_c[T[l].tap] = T[l].cout;
  }
  for (int k = 0; k < 5; ++k) {
    PNRF_REQUIRE(lin_dim[k] == tap_c[k], PNRF_E_SHAPE, "pnrf_lpips_create: lin %d of '%s' has %d channels, expected %d.  %s", k, net, lin_dim[k], tap_c[k], TABLE_TEXT);
    PNRF_REQUIRE(lin_w[k], PNRF_E_ARG, "pnrf_lpips_create: null pointer (lin %d)", k);
  }
  // host image of the one allocation: per layer [K padded][C_out] then [C_out]; then the five lin vectors.  Every piece starts on a multiple of 64 floats.
  size_t off_w[13], off_b[13], off_lin[5], total = 0;
  for (int l = 0; l < n; ++l) {
    off_w[l] = total; total += (size_t)k_padded(T[l]) * T[l].cout;
    off_b[l] = total; total += (size_t)T[l].cout;
  }
  for (int k = 0; k < 5; ++k) { off_lin[k] = total; total += (size_t)tap_c[k]; }
  std::vector<float> img(total, 0.f), tmp;
  for (int l = 0; l < n; ++l) {
    const LayerSpec& L = T[l];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    tmp.resize(nw);
    int rc = to_host(tmp.data(), conv_w[l], nw);
    if (rc) return rc;
    for (int o = 0; o < L.cout; ++o)
      for (int c = 0; c < L.cin; ++c)
        for (int t = 0; t < L.k * L.k; ++t) img[off_w[l] + ((size_t)t * L.cin + c) * L.cout + o] = tmp[((size_t)o * L.cin + c) * L.k * L.k + t];
    rc = to_host(img.data() + off_b[l], conv_b[l], (size_t)L.cout);
    if (rc) return rc;
  }
  for (int k = 0; k < 5; ++k) {
    const int rc = to_host(img.data() + off_lin[k], lin_w[k], (size_t)tap_c[k]);
    if (rc) return rc;
  }
  pnrf_lpips* h = new pnrf_lpips();
  h->net = id; h->n = n; h->d_all = nullptr; h->d_wt_all = nullptr;
  hipError_t e = hipGetDevice(&h->device);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_all, total * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(h->d_all, img.data(), total * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("pnrf_lpips_create: device allocation / upload of %zu bytes failed: %s", total * sizeof(float), hipGetErrorString(e));
    if (h->d_all) (void)hipFree(h->d_all);
    delete h;
    return (int)e;
  }
  for (int l = 0; l < n; ++l) { h->d_w[l] = h->d_all + off_w[l]; h->d_b[l] = h->d_all + off_b[l]; }
  for (int k = 0; k < 5; ++k) h->d_lin[k] = h->d_all + off_lin[k];
  *out = h;
  return 0;
}

extern "C" int pnrf_lpips_free(pnrf_lpips_t* h) {
  if (!h) return 0;
  if (h->d_all) (void)hipFree(h->d_all);
  if (h->d_wt_all) (void)hipFree(h->d_wt_all);
  delete h;
  return 0;
}

extern "C" int64_t pnrf_lpips_workspace_bytes(const pnrf_lpips_t* h, int H, int W) {
  if (!h || !size_ok(h->net, H, W)) return 0;
  Plan pl;
  make_plan(h->net, H, W, &pl);
  return PARTIAL_BYTES + 2 * align256(pl.max_elems * (int64_t)sizeof(float));
}

extern "C" int pnrf_lpips_fwd(const pnrf_lpips_t* h, const float* a, int a_stride, const float* b, int b_stride, int H, int W, int normalize, double* out,
                              float* maps, void* workspace, int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_lpips_fwd: null handle");
  PNRF_REQUIRE(a && b && out && workspace, PNRF_E_ARG, "pnrf_lpips_fwd: null pointer (a, b, out and workspace are required)");
  PNRF_REQUIRE(a_stride >= 3 && b_stride >= 3, PNRF_E_ARG, "pnrf_lpips_fwd: pixel strides %d / %d, need >= 3 floats", a_stride, b_stride);
  PNRF_REQUIRE(size_ok(h->net, H, W), PNRF_E_ARG, "pnrf_lpips_fwd: image of %d x %d outside %d .. %d per side for '%s'", H, W, min_dim(h->net), MAX_DIM,
               h->net == 0 ? "alex" : "vgg");
  const int64_t need = pnrf_lpips_workspace_bytes(h, H, W);
  PNRF_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, PNRF_E_ARG, "pnrf_lpips_fwd: workspace of %lld bytes (16-byte aligned) needed, got %lld",
               (long long)need, (long long)workspace_bytes);
  const hipStream_t st = (hipStream_t)stream;
  Plan pl;
  make_plan(h->net, H, W, &pl);
  double* partial = (double*)workspace;
  float* buf[2];
  buf[0] = (float*)((char*)workspace + PARTIAL_BYTES);
  buf[1] = (float*)((char*)buf[0] + align256(pl.max_elems * (int64_t)sizeof(float)));
  int n;
  const LayerSpec* T = net_table(h->net, &n);
  FinishArgs fin;
  fin.partial = partial; fin.out = out;
  // x: where the current activations are; every step writes into the other buffer (a layer with a pool or a gather: tmp = the other one, y = x's own —
  // the conv reads tmp only)
  const float* x = a;
  int cur = 1, hh = H, ww = W;
  int64_t map_off = 0;
  for (int l = 0; l < n; ++l) {
    const LayerSpec& L = T[l];
    const bool two = L.cin == 3 || L.pool != 0;
    float* tmp = two ? buf[cur ^ 1] : nullptr;
    float* y = two ? buf[cur] : buf[cur ^ 1];
    int oh, ow;
    const int rc = run_layer(h, l, L.pool != 0, x, b, a_stride, b_stride, normalize ? 2 : 1, hh, ww, tmp, y, &oh, &ow, st);
    if (rc) return rc;
    if (!two) cur ^= 1;
    x = y; hh = oh; ww = ow;
    if (L.tap >= 0) {
      TapArgs t;
      t.f = y; t.lin = h->d_lin[L.tap]; t.C = L.cout; t.P = (int64_t)oh * ow; t.map = maps ? maps + map_off : nullptr; t.partial = partial + L.tap * TAP_MAXB;
      const int64_t want = (t.P + TPB / 64 - 1) / (TPB / 64);
      const int nb = (int)(want < TAP_MAXB ? want : TAP_MAXB);
      hipLaunchKernelGGL(lpips_tap_kernel, dim3(nb), dim3(TPB), 0, st, t);
      PNRF_LAUNCH_CHECK();
      fin.nb[L.tap] = nb; fin.P[L.tap] = (double)t.P;
      map_off += t.P;
    }
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(TPB), 0, st, fin);
  PNRF_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t pnrf_lpips_layer_workspace_bytes(const pnrf_lpips_t* h, int layer, int pool_first, int H, int W) {
  if (!h || layer < 0 || layer >= h->n || H < 1 || W < 1 || H > MAX_DIM || W > MAX_DIM) return 0;
  int n;
  const LayerSpec& L = net_table(h->net, &n)[layer];
  if (L.cin == 3) {
    const int oh = conv_out(H, L), ow = conv_out(W, L);
    return oh >= 1 && ow >= 1 && H + 2 * L.pad >= L.k && W + 2 * L.pad >= L.k ? (int64_t)2 * oh * ow * k_padded(L) * (int64_t)sizeof(float) : 0;
  }
  if (pool_first && L.pool && H >= L.pool && W >= L.pool) return (int64_t)2 * pool_out(H, L.pool) * pool_out(W, L.pool) * L.cin * (int64_t)sizeof(float);
  return 0;
}

extern "C" int pnrf_lpips_layer_fwd(const pnrf_lpips_t* h, int layer, int pool_first, const float* x, int H, int W, float* y, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_lpips_layer_fwd: null handle");
  PNRF_REQUIRE(layer >= 0 && layer < h->n, PNRF_E_ARG, "pnrf_lpips_layer_fwd: layer %d outside 0 .. %d", layer, h->n - 1);
  PNRF_REQUIRE(x && y, PNRF_E_ARG, "pnrf_lpips_layer_fwd: null pointer (x and y are required)");
  int n;
  const LayerSpec& L = net_table(h->net, &n)[layer];
  PNRF_REQUIRE(!pool_first || L.pool, PNRF_E_ARG, "pnrf_lpips_layer_fwd: layer %d has no max pooling in front of it", layer);
  PNRF_REQUIRE(H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM, PNRF_E_ARG, "pnrf_lpips_layer_fwd: input of %d x %d outside 1 .. %d per side", H, W, MAX_DIM);
  int ch = H, cw = W;
  if (pool_first) {
    PNRF_REQUIRE(H >= L.pool && W >= L.pool, PNRF_E_ARG, "pnrf_lpips_layer_fwd: input of %d x %d has no %d x %d pooling window", H, W, L.pool, L.pool);
    ch = pool_out(H, L.pool); cw = pool_out(W, L.pool);
  }
  PNRF_REQUIRE(ch + 2 * L.pad >= L.k && cw + 2 * L.pad >= L.k, PNRF_E_ARG, "pnrf_lpips_layer_fwd: input of %d x %d is smaller than the %d x %d filter", ch, cw, L.k, L.k);
  PNRF_REQUIRE(((uintptr_t)y & 15) == 0 && (L.cin == 3 || ((uintptr_t)x & 15) == 0), PNRF_E_ARG, "pnrf_lpips_layer_fwd: x (hidden layers) and y must be 16-byte aligned");
  const int64_t need = pnrf_lpips_layer_workspace_bytes(h, layer, pool_first, H, W);
  PNRF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0), PNRF_E_ARG,
               "pnrf_lpips_layer_fwd: workspace of %lld bytes (16-byte aligned) needed, got %lld", (long long)need, (long long)workspace_bytes);
  int oh, ow;
  return run_layer(h, layer, pool_first != 0, x, x + (int64_t)H * W * 3, 3, 3, 0, H, W, (float*)workspace, y, &oh, &ow, (hipStream_t)stream);
}

// ---- the loss: value and gradient (pnrf_lpips_loss_fwd, pnrf_lpips_layer_bwd, pnrf_lpips_tap_bwd) -------------------------------------------------
#include "pnrf_lpips_loss.h"
