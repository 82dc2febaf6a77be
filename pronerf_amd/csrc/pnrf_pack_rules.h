// pnrf_pack_rules.h — THE statement of what every element of a packed net is: the roundings, the scalings, the lane / row / feature indexing of the
// fragment orders, the bias tables and the derived matrices (folded first layers, the NeRF class's Wc = Wv . Wf, the pass-1 constants).
// __host__ __device__ throughout: the host packer (pnrf_pack.hip) loops over these functions, the device repack kernels (pnrf_repack.hip) run one
// lane of them per thread, so the two produce the same bytes by construction.
//
// Arithmetic that has to agree between an x86-64 host and gfx950:
//  * fp64 multiply-add: a * b + c is contracted to an fma by hipcc's device pass (-ffp-contract=fast) and is NOT by the host pass (baseline
//    x86-64 has no fma instruction).  mac_d() switches contraction off in its own body, on both sides: product rounded, then sum rounded;
//  * double -> float, double -> fp16, float -> fp16 are the compilers' conversions: round to nearest even, one rounding each (see d2h); float -> bf16
//    is integer code.  fp32 and fp16 subnormals are kept on both sides (hipcc's default
//    denormal mode of gfx950 kernels is IEEE for all three widths; nothing here is built with -fgpu-flush-denormals-to-zero);
//  * NaN payloads of the fp16 conversion are the one thing the two sides may not share.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pnrf_layout.h"

namespace pnrf {

#define PNRF_RULE __host__ __device__ inline

constexpr int PACK_MAX_LAYERS = MAX_NHID + 2;      // Linear layers of the deepest net (the NeRF class has 12)

// The caller's matrices: W[l] at m[l], b[l] at m[PACK_MAX_LAYERS + l].  A PackSrc names a matrix either as one of them (idx >= 0, plus an element
// offset) or by address (a derived matrix); a device plan keeps PackSrc's, so it holds for whatever pointers a later call brings
struct PackPtrs { const float* m[2 * PACK_MAX_LAYERS]; };
struct PackSrc { const float* abs; int idx, off; };
PNRF_RULE const float* resolve(const PackPtrs& P, const PackSrc& s) { return s.idx >= 0 ? P.m[s.idx] + s.off : s.abs; }

// ---- roundings ---------------------------------------------------------------------------------------------------------------------------------
// fp32 -> bf16, round to nearest even; NaN stays NaN.
PNRF_RULE uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// double / float -> fp16, ONE rounding each.  A value held in double goes to fp16 directly (d2h), not by way of fp32: that is what the packer's images
// have always held — under -ffp-contract=fast the compiler narrows (fp16)(float)x of a double x once — and it is written out here, with contraction off
// in the bodies that narrow, so that neither side depends on that fold.  (gfx950 has no f64 -> f16 instruction; the compiler's expansion rounds exactly.)
PNRF_RULE uint16_t f2h(float f) {
#pragma clang fp contract(off)
  _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u;
}
PNRF_RULE uint16_t d2h(double f) {
#pragma clang fp contract(off)
  _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u;
}
PNRF_RULE float h2f(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }
// acc + a * b in double: two roundings, on the host and on the device
PNRF_RULE double mac_d(double acc, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return acc + p;
}
// split fp16 of a value: hi, and the remainder times 2^11
PNRF_RULE void split_h16(double w, uint16_t* hi, uint16_t* lo) {
#pragma clang fp contract(off)
  *hi = d2h(w); *lo = d2h((w - (double)h2f(*hi)) * H16_LO_SCALE);
}

// ---- one layer of one stream ---------------------------------------------------------------------------------------------------------------------
struct PackLayer {
  const float *W, *b;
  const int *in_map, *out_map;      // as Layer::in_map / out_map of pnrf_pack.hip
  int in_dim, nt, nk, x_from;
  double wscale, bscale, xscale;
  float bpost;                      // != 1: the bias table's entries times this, in fp32 (pass-1 skip layers: P1_SKIP_SCALE)
};
// weight (out, in) on the stream's scale, in double (0 for padding rows / columns)
PNRF_RULE double wdbl(const PackLayer& L, int out, int in) { return (out >= 0 && in >= 0) ? (double)L.W[(size_t)out * L.in_dim + in] * (in >= L.x_from ? L.xscale : L.wscale) : 0.0; }
PNRF_RULE float wval(const PackLayer& L, int out, int in) {
#pragma clang fp contract(off)
  return (float)wdbl(L, out, in);
}

// The fragment orders.  A fragment is FRAG_BYTES = 64 lanes x 16 bytes; pack_lane() gives the 16 bytes of one lane of fragment `frag` of a layer.
enum PackKind {
  PK_BF16_32, PK_F16_32,      // 32x32x16: fragments [tile][k-step]; lane = (row r = lane & 31, half h = lane >> 5), 8 features in_map[ks][h][j]
  PK_F32,                     // 16x16x4: fragments [tile][4 k-steps]; lane = (row i = lane & 15, quarter q = lane >> 4), in_map[4 fr + i][q]
  PK_B16, PK_E16,             // 16x16x32, bf16 / fp16: fragments (tile pair, ks, tile in pair); lane = (row lane & 15, group g = lane >> 4), in_map[ks][g][j]
  PK_H16X2,                   // ... split fp16: two planes per fragment position, hi and lo * 2^11
  PK_L0_F16X2,                // pass 1's split first layer (one k-step): per 32-row tile a W_hi and a W_lo * 2^11 fragment
  PK_F16_SKIP,                // pass 1's skip layer: per tile KS_HID fp16 fragments of the h-columns times 2^11, then of the x-columns W_hi 2^11, W_hi, W_lo 2^11
  PK_BIAS16, PK_BIAS32        // bias tables, 4 floats per lane: [tile][16 rows] in row order / 32-row tiles as [tile][half][16 registers]
};
union PackLane { uint32_t w[4]; uint16_t h[8]; float f[4]; };

PNRF_RULE int pack_frags(int kind, const PackLayer& L) {
  switch (kind) {
    case PK_BF16_32: case PK_F16_32: return L.nt * L.nk;
    case PK_F32: return L.nt * (L.nk / 4);
    case PK_B16: case PK_E16: return (L.nt / 2) * L.nk * 2;
    case PK_H16X2: return (L.nt / 2) * L.nk * 4;
    case PK_L0_F16X2: return L.nt * 2;
    case PK_F16_SKIP: return L.nt * (KS_HID + P1_KS_X);
    case PK_BIAS16: return (L.nt * 16 + 255) / 256;
    default: return (L.nt * 32 + 255) / 256;
  }
}

PNRF_RULE uint16_t round16(bool bf, double w) {
#pragma clang fp contract(off)
  return bf ? f2bf((float)w) : d2h(w);
}
// 32x32x16 fragment of tile `to` whose k-step map is kmap[h * 8 + j]
PNRF_RULE void lane_32(const PackLayer& L, int to, const int* kmap, bool bf, int lane, uint16_t* o) {
  const int out = L.out_map[to * 32 + (lane & 31)];
  for (int j = 0; j < 8; ++j) o[j] = round16(bf, wdbl(L, out, kmap[(lane >> 5) * 8 + j]));
}
// fp16 of an fp32 (or fp16) value times P1_SKIP_SCALE.  The product is formed in double, where it is exact, and rounded to fp16 once — the value of
// f2h(v * 2048.f), whose fp32 product is exact as well.  Not written that way: hipcc fuses an fp32 multiply that feeds an fp16 conversion into
// v_fma_mixlo_f16 v, 2048, +0, and -0 * 2048 + 0 is +0 where the host writes -0
PNRF_RULE uint16_t scaled_h(float v) { return d2h((double)v * (double)P1_SKIP_SCALE); }
// ... a 32x32x16 fragment of the fp32 weights so scaled
PNRF_RULE void lane_32_scaled(const PackLayer& L, int to, const int* kmap, int lane, uint16_t* o) {
  const int out = L.out_map[to * 32 + (lane & 31)];
  for (int j = 0; j < 8; ++j) o[j] = scaled_h(wval(L, out, kmap[(lane >> 5) * 8 + j]));
}
// ... and its split form: plane 0 = hi, 1 = lo * 2^11, 2 = hi * P1_SKIP_SCALE (of the rounded hi, in fp32)
PNRF_RULE void lane_32_split(const PackLayer& L, int to, const int* xmap, int plane, int lane, uint16_t* o) {
  const int out = L.out_map[to * 32 + (lane & 31)];
  for (int j = 0; j < 8; ++j) {
    uint16_t hi, lo;
    split_h16(wdbl(L, out, xmap[(lane >> 5) * 8 + j]), &hi, &lo);
    o[j] = plane == 0 ? hi : plane == 1 ? lo : scaled_h(h2f(hi));
  }
}
PNRF_RULE float bias_val(const PackLayer& L, int out) {
  float v = out >= 0 ? (float)((double)L.b[out] * L.bscale) : 0.f;
  if (L.bpost != 1.f) v *= L.bpost;
  return v;
}

// false: the lane lies behind the end of a bias table (nothing to write)
PNRF_RULE bool pack_lane(int kind, const PackLayer& L, int frag, int lane, PackLane* o) {
  switch (kind) {
    case PK_BF16_32: case PK_F16_32:
      lane_32(L, frag / L.nk, L.in_map + (frag % L.nk) * 16, kind == PK_BF16_32, lane, o->h);
      return true;
    case PK_F32: {
      const int ks4 = L.nk / 4, to = frag / ks4, fr = frag % ks4, r = lane & 15, q = lane >> 4;
      const int out = L.out_map[to * 16 + r];
      for (int i = 0; i < 4; ++i) o->f[i] = wval(L, out, L.in_map[(4 * fr + i) * 4 + q]);
      return true;
    }
    case PK_B16: case PK_E16: case PK_H16X2: {
      const int planes = kind == PK_H16X2 ? 2 : 1, plane = frag % planes, pos = frag / planes;
      const int t = pos & 1, ks = (pos >> 1) % L.nk, tp = (pos >> 1) / L.nk, r = lane & 15, g = lane >> 4;
      const int out = L.out_map[(2 * tp + t) * 16 + r];
      for (int j = 0; j < 8; ++j) {
        const int in = L.in_map[(ks * 4 + g) * 8 + j];
        if (planes == 1) o->h[j] = round16(kind == PK_B16, wdbl(L, out, in));
        else {
          uint16_t hi, lo;
          split_h16(wdbl(L, out, in), &hi, &lo);
          o->h[j] = plane ? lo : hi;
        }
      }
      return true;
    }
    case PK_L0_F16X2:
      lane_32_split(L, frag >> 1, L.in_map, frag & 1, lane, o->h);
      return true;
    case PK_F16_SKIP: {
      const int kt = KS_HID + P1_KS_X, to = frag / kt, i = frag % kt;
      if (i < KS_HID) lane_32_scaled(L, to, L.in_map + i * 16, lane, o->h);
      else lane_32_split(L, to, L.in_map + KS_HID * 16, i == KS_HID ? 2 : i - KS_HID - 1, lane, o->h);
      return true;
    }
    case PK_BIAS16: {
      const int e0 = (frag * 64 + lane) * 4;
      if (e0 >= L.nt * 16) return false;
      for (int i = 0; i < 4; ++i) o->f[i] = bias_val(L, L.out_map[e0 + i]);
      return true;
    }
    default: {
      const int e0 = (frag * 64 + lane) * 4;
      if (e0 >= L.nt * 32) return false;
      for (int i = 0; i < 4; ++i) {
        const int e = e0 + i, to = e >> 5, h = (e >> 4) & 1, g = e & 15;
        o->f[i] = bias_val(L, L.out_map[to * 32 + acc_row(g, h)]);
      }
      return true;
    }
  }
}

// ---- derived matrices --------------------------------------------------------------------------------------------------------------------------
// Every one is a function of the caller's matrices alone (none reads another derived matrix), so all of a net's run side by side.
enum DeriveKind {
  DV_COPY,        // dst[r][c] = a[r][c]
  DV_FOLD6,       // dst[r][j] = sum_p a[r][6 p + j], p < n, j < 6: n column groups of width 6 folded into one (the Pluecker 6-vectors of a ray's points
                  // are ONE vector in exact arithmetic, pnrf_layout.h); fp64 sum over p, rounded once
  DV_WC,          // NeRF class: dst[r][c] = sum_k a[r][k] b[k][c] (Wv . Wf), k < W_HID ascending, fp64 multiply-add of two roundings, rounded to fp32 once
  DV_BC,          // ... dst[r] = c[r] + sum_k a[r][k] b[k] (bv + Wv . bf), likewise
  DV_COLMAX,      // pass-1 constant of a hidden layer: max over columns j < W_HID of sum_i a[i][j]^2 (i < W_HID ascending, fp64), times 1 + 1e-6
  DV_OUTMAX       // ... of the output layer: max over its 8 depth rows of a[k][j]^2, / log2(e)^2, times 1 + 1e-6
};
struct DeriveOp {
  int kind, rows, cols, n;
  float* dst; int ldd;
  PackSrc a, b, c; int lda;
};
PNRF_RULE int derive_elems(const DeriveOp& op) { return op.kind == DV_COLMAX || op.kind == DV_OUTMAX ? 1 : op.rows * op.cols; }

PNRF_RULE float fold6_elem(const float* row, int n, int j) {
  double acc = 0.0;
  for (int p = 0; p < n; ++p) acc += (double)row[6 * p + j];
  return (float)acc;
}
// element e of an elementwise op (every kind but DV_COLMAX / DV_OUTMAX)
PNRF_RULE void derive_elem(const DeriveOp& op, const PackPtrs& P, int e) {
  const int r = e / op.cols, c = e % op.cols;
  const float* A = resolve(P, op.a);
  float* d = op.dst + (size_t)r * op.ldd + c;
  if (op.kind == DV_COPY) *d = A[(size_t)r * op.lda + c];
  else if (op.kind == DV_FOLD6) *d = fold6_elem(A + (size_t)r * op.lda, op.n, c);
  else if (op.kind == DV_WC) {
    const float* B = resolve(P, op.b);
    double acc = 0.0;
    for (int k = 0; k < W_HID; ++k) acc = mac_d(acc, (double)A[(size_t)r * op.lda + k], (double)B[(size_t)k * W_HID + c]);
    *d = (float)acc;
  } else {      // DV_BC
    const float* B = resolve(P, op.b);
    double acc = (double)resolve(P, op.c)[r];
    for (int k = 0; k < W_HID; ++k) acc = mac_d(acc, (double)A[(size_t)r * op.lda + k], (double)B[k]);
    *d = (float)acc;
  }
}
// the pass-1 constants: column norm, the maximum (a NaN never wins: the comparison is false for it), the final scalings
PNRF_RULE double colnorm(const float* W, int ld, int j) {
  double cn = 0.0;
  for (int i = 0; i < W_HID; ++i) { const double w = (double)W[(size_t)i * ld + j]; cn = mac_d(cn, w, w); }
  return cn;
}
PNRF_RULE double max_keep(double v, double vmax) { return v > vmax ? v : vmax; }
PNRF_RULE double sq_d(float w) { return (double)w * (double)w; }
PNRF_RULE float p1c_hidden(double cmax) { return (float)(cmax * (1.0 + 1e-6)); }
PNRF_RULE float p1c_out(double mmax) { return (float)(mmax / (LOG2E_D * LOG2E_D) * (1.0 + 1e-6)); }

// ---- what a device plan holds: per stream (or bias table) the layers' tables, and the derive ops -------------------------------------------------
struct PackEntry {
  PackSrc W, b;
  int in_map, out_map;      // offsets into the plan's map pool
  int in_dim, nt, nk, x_from;
  double wscale, bscale, xscale;
  float bpost;
  int kind, frags;
  uint32_t dst_off;         // bytes from the section's start
};
PNRF_RULE PackLayer entry_layer(const PackEntry& e, const PackPtrs& P, const int* maps) {
  return PackLayer{resolve(P, e.W), resolve(P, e.b), maps + e.in_map, maps + e.out_map, e.in_dim, e.nt, e.nk, e.x_from, e.wscale, e.bscale, e.xscale, e.bpost};
}

}  // namespace pnrf
