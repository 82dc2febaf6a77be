// pnrf_jpeg_rules.h — THE statement of the JPEG encoder's format rules: colour conversion, edge replication, the forward DCT, quantisation and zigzag,
// the quality scaling of the Annex K tables, the fixed Annex K.3 Huffman tables and the symbols of a block, restart intervals, byte stuffing, the
// file's header and the size bound.  __host__ __device__ throughout, integer arithmetic only: the host twin (pnrf_jpeg_encode_host) loops over these
// functions, the kernels of pnrf_jpeg.hip run them per lane, so the two produce the same bytes by construction.
//
// The file: baseline sequential DCT, 8-bit samples.  SOI, APP0 (JFIF 1.01, no units, 1 : 1), one DQT (table 0, and table 1 for colour), SOF0, one DHT
// (DC 0, AC 0, and DC 1, AC 1 for colour), DRI, SOS, the entropy data, EOI.
//  * components: 1 (gray: the plane is Y) or 3 (Y, Cb, Cr from RGB; 1 x 1 sampling each, an MCU is the Y, Cb, Cr block of one 8 x 8 pixel square);
//  * colour: JFIF full-range BT.601 in 16-bit fixed point (jpeg_ycc), then the level shift by -128;
//  * edges: a pixel right of column W - 1 or below row H - 1 is the last column's / row's (jpeg_sample's clamp);
//  * forward DCT: the 13-bit scaled integer form with 32-bit intermediates — Loeffler, Ligtenberg and Moschytz' 12-multiplication flow graph, constants
//    round(c 2^13), rows first and kept with 2 extra bits, then columns; the result is 8 x the orthonormal DCT-II coefficient (jpeg_fdct_1d, jpeg_fdct);
//  * quantisation: sign(c) ((|c| + 4 q) / (8 q)) in integers, q the table entry: division rounding half away from zero (jpeg_quantise);
//  * tables: Annex K.1 / K.2 scaled as the IJG library does, s = 5000 / quality below 50 and 200 - 2 quality from 50, entry (base s + 50) / 100 clamped
//    to 1 .. 255 (jpeg_qtable): the tables PIL writes for the same quality;
//  * entropy coding: the Annex K.3 tables as they stand, DC as the difference to the previous block of the component inside the interval, AC as
//    (run << 4 | size) symbols with F0 for 16 zeros and 00 when the block ends in zeros (jpeg_block_symbols); bits MSB first;
//  * one restart interval per MCU row (DRI = ceil(W / 8)): predictions start at 0, the last byte is filled with 1-bits, FF D0+m follows every interval
//    but the last, m = row mod 8; every FF byte of entropy data (a filled last byte included) is followed by 00.
#pragma once
#include <stdint.h>

namespace pnrf {

#ifndef PNRF_RULE
#define PNRF_RULE __host__ __device__ inline
#endif

constexpr int JPEG_MAX_SIDE = 65535;
constexpr int JPEG_DC_MAX_BITS = 11 + 11;             // the longest DC code (chrominance, category 11) and its 11 value bits
constexpr int JPEG_AC_MAX_BITS = 16 + 10;             // the longest AC code and the 10 value bits of the largest category
constexpr int JPEG_BLOCK_MAX_BITS = JPEG_DC_MAX_BITS + 63 * JPEG_AC_MAX_BITS;      // 1660: every coefficient non-zero, so no ZRL and no EOB on top

// ---- geometry -----------------------------------------------------------------------------------------------------------------------------------
PNRF_RULE int64_t jpeg_mcu_cols(int W) { return ((int64_t)W + 7) / 8; }
PNRF_RULE int64_t jpeg_mcu_rows(int H) { return ((int64_t)H + 7) / 8; }
PNRF_RULE int64_t jpeg_row_blocks(int W, int ch) { return jpeg_mcu_cols(W) * ch; }      // blocks of one MCU row = of one restart interval, in coding order
PNRF_RULE int jpeg_header_bytes(int ch) {
  // SOI, APP0, DQT (65 a table), SOF0, DHT (29 a DC table, 179 an AC table), DRI, SOS
  return 2 + 18 + (4 + 65 * (ch == 3 ? 2 : 1)) + (10 + 3 * ch) + (4 + 208 * (ch == 3 ? 2 : 1)) + 6 + (8 + 2 * ch);
}
// an interval for any content: every block at its worst, every byte an FF and stuffed, the 2 bytes of RSTm
PNRF_RULE int64_t jpeg_interval_max_bytes(int W, int ch) { return 2 * ((jpeg_row_blocks(W, ch) * JPEG_BLOCK_MAX_BITS + 7) / 8) + 2; }
PNRF_RULE int64_t jpeg_max_file_bytes(int H, int W, int ch) { return jpeg_header_bytes(ch) + jpeg_mcu_rows(H) * jpeg_interval_max_bytes(W, ch) + 2; }
// room of an interval's slot in the workspace, in 16-byte granules
PNRF_RULE int64_t jpeg_slot_bytes(int W, int ch) { return (jpeg_interval_max_bytes(W, ch) + 15) / 16 * 16; }

// ---- samples ------------------------------------------------------------------------------------------------------------------------------------
// component c (0: Y, 1: Cb, 2: Cr) of an RGB pixel, 0 .. 255
PNRF_RULE int jpeg_ycc(int c, int r, int g, int b) {
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// the level-shifted sample of component c at (y, x), y and x anywhere in the padded frame
PNRF_RULE int jpeg_sample(const uint8_t* img, int64_t stride, int H, int W, int ch, int c, int y, int x) {
  const uint8_t* p = img + (int64_t)(y < H ? y : H - 1) * stride + (int64_t)(x < W ? x : W - 1) * ch;
  return (ch == 1 ? (int)p[0] : jpeg_ycc(c, p[0], p[1], p[2])) - 128;
}

// ---- transform ----------------------------------------------------------------------------------------------------------------------------------
PNRF_RULE int32_t jpeg_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
// One pass over 8 values d[0], d[s], .. d[7 s], in place.  Even outputs 0 and 4 leave scaled by 2^up (up >= 0) or descaled by -up bits; the others are
// products by 2^13 constants descaled by 13 - up bits.  Rows: up = 2; columns: up = -2.
PNRF_RULE void jpeg_fdct_1d(int32_t* d, int s, int up) {
  const int32_t t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
  const int32_t t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = 13 - up;
  if (up >= 0) { d[0] = (t10 + t11) * (1 << up); d[4 * s] = (t10 - t11) * (1 << up); }
  else { d[0] = jpeg_descale(t10 + t11, -up); d[4 * s] = jpeg_descale(t10 - t11, -up); }
  const int32_t e = (t12 + t13) * 4433;                      // 0.541196100
  d[2 * s] = jpeg_descale(e + t13 * 6270, n);                // 0.765366865
  d[6 * s] = jpeg_descale(e - t12 * 15137, n);               // 1.847759065
  const int32_t z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;      // 1.175875602
  const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;                  // 0.298631336 2.053119869 3.072711026 1.501321110
  const int32_t b1 = -z1 * 7373, b2 = -z2 * 20995, b3 = -z3 * 16069 + z5, b4 = -z4 * 3196 + z5;     // 0.899976223 2.562915447 1.961570560 0.390180644
  d[7 * s] = jpeg_descale(a4 + b1 + b3, n);
  d[5 * s] = jpeg_descale(a5 + b2 + b4, n);
  d[3 * s] = jpeg_descale(a6 + b2 + b3, n);
  d[s] = jpeg_descale(a7 + b1 + b4, n);
}
// 64 level-shifted samples, row-major, to 8 x their DCT coefficients, row-major (vertical frequency first)
PNRF_RULE void jpeg_fdct(int32_t* d) {
#pragma unroll
  for (int r = 0; r < 8; ++r) jpeg_fdct_1d(d + 8 * r, 1, 2);
#pragma unroll
  for (int c = 0; c < 8; ++c) jpeg_fdct_1d(d + c, 8, -2);
}
PNRF_RULE int jpeg_quantise(int32_t c, int q) {
  const int32_t q8 = q << 3, a = c < 0 ? -c : c, v = (a + (q8 >> 1)) / q8;
  return c < 0 ? -v : v;
}
// the row-major index of zigzag position k
PNRF_RULE int jpeg_natural(int k) {
  const uint8_t Z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return Z[k];
}
// entry k (row-major) of quantisation table t (0: luminance, 1: chrominance) at quality 1 .. 100
PNRF_RULE int jpeg_qtable(int t, int k, int quality) {
  const uint8_t L[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                         18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  const uint8_t Cq[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = ((t ? Cq[k] : L[k]) * s + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}

// ---- Huffman tables (Annex K.3) -----------------------------------------------------------------------------------------------------------------
// table id = class << 1 | destination: 0 DC luminance, 1 DC chrominance, 2 AC luminance, 3 AC chrominance
PNRF_RULE int jpeg_huff_count(int id, int len) {      // codes of length len = 1 .. 16
  const uint8_t B[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                            {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
  return B[id][len - 1];
}
PNRF_RULE int jpeg_huff_symbols(int id) { return id < 2 ? 12 : 162; }
PNRF_RULE int jpeg_huff_symbol(int id, int i) {       // the i-th symbol in order of increasing code
  const uint8_t AL[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
      0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  const uint8_t AC[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
      0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  return id < 2 ? i : id == 2 ? AL[i] : AC[i];
}
// code[s] = bits | nbits << 24 of symbol s (0 for a symbol the table does not have): the canonical codes of Annex C
struct JpegHuff { uint32_t code[256]; };
PNRF_RULE void jpeg_huff_build(int id, JpegHuff* h) {
  for (int s = 0; s < 256; ++s) h->code[s] = 0;
  uint32_t code = 0;
  int i = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int k = jpeg_huff_count(id, len); k > 0; --k) h->code[jpeg_huff_symbol(id, i++)] = code++ | (uint32_t)len << 24;
    code <<= 1;
  }
}

// ---- symbols ------------------------------------------------------------------------------------------------------------------------------------
PNRF_RULE int jpeg_category(int v) {      // bits of |v|
  int a = v < 0 ? -v : v, n = 0;
  while (a) { ++n; a >>= 1; }
  return n;
}
// a Huffman code followed by the n value bits of v (v - 1 in n bits for a negative v), as bits | nbits << 27 (at most 26 bits)
PNRF_RULE uint32_t jpeg_coded(uint32_t huff, int v, int n) {
  const uint32_t hb = huff >> 24, val = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
  return ((huff & 0xffffff) << n | val) | (hb + (uint32_t)n) << 27;
}
// The symbols of one block in order: zz its 64 quantised coefficients in zigzag order, pred the DC of the component's previous block in the interval
// (0 for the first).  emit(bits | nbits << 27) is called per symbol with its value bits.
template <class Emit>
PNRF_RULE void jpeg_block_symbols(const int16_t* zz, int pred, const JpegHuff& dc, const JpegHuff& ac, Emit emit) {
  const int diff = zz[0] - pred, s = jpeg_category(diff);
  emit(jpeg_coded(dc.code[s], diff, s));
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = zz[k];
    if (v == 0) { ++run; continue; }
    for (; run >= 16; run -= 16) emit(jpeg_coded(ac.code[0xf0], 0, 0));
    const int n = jpeg_category(v);
    emit(jpeg_coded(ac.code[run << 4 | n], v, n));
    run = 0;
  }
  if (run > 0) emit(jpeg_coded(ac.code[0x00], 0, 0));
}

// ---- the file's header --------------------------------------------------------------------------------------------------------------------------
// writes jpeg_header_bytes(ch) bytes (one lane / the host); the entropy data starts behind them
PNRF_RULE int jpeg_header(uint8_t* out, int H, int W, int ch, int quality) {
  uint8_t* p = out;
  auto put = [&](int v) { *p++ = (uint8_t)v; };
  auto put16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
  const int nt = ch == 3 ? 2 : 1;
  put16(0xffd8);
  put16(0xffe0); put16(16); put('J'); put('F'); put('I'); put('F'); put(0); put16(0x0101); put(0); put16(1); put16(1); put(0); put(0);
  put16(0xffdb); put16(2 + 65 * nt);
  for (int t = 0; t < nt; ++t) {
    put(t);
    for (int k = 0; k < 64; ++k) put(jpeg_qtable(t, jpeg_natural(k), quality));
  }
  put16(0xffc0); put16(8 + 3 * ch); put(8); put16(H); put16(W); put(ch);
  for (int c = 0; c < ch; ++c) { put(c + 1); put(0x11); put(c ? 1 : 0); }
  put16(0xffc4); put16(2 + 208 * nt);
  for (int t = 0; t < nt; ++t)
    for (int cls = 0; cls < 2; ++cls) {
      const int id = cls << 1 | t;
      put(cls << 4 | t);
      for (int len = 1; len <= 16; ++len) put(jpeg_huff_count(id, len));
      for (int i = 0; i < jpeg_huff_symbols(id); ++i) put(jpeg_huff_symbol(id, i));
    }
  put16(0xffdd); put16(4); put16((int)jpeg_mcu_cols(W));
  put16(0xffda); put16(6 + 2 * ch); put(ch);
  for (int c = 0; c < ch; ++c) { put(c + 1); put(c ? 0x11 : 0x00); }
  put(0); put(63); put(0);
  return (int)(p - out);
}

}  // namespace pnrf
