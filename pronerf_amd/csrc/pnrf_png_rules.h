// pnrf_png_rules.h — THE statement of the PNG encoder's format rules: the five row filters and the adaptive choice, the cut of the filtered bytes into
// segments and tiles, which bytes become literals and which distance-1 matches, the length-limited Huffman codes and the code-length header of a
// segment's dynamic block, the stored fallback, and the Adler-32 / CRC-32 pieces with their combination.  __host__ __device__ throughout, integer
// arithmetic only: the host twin (pnrf_png_encode_host) loops over these functions, the kernels of pnrf_png.hip run them per lane (or, for the serial
// code construction, on one lane), so the two produce the same bytes by construction.
//
// The file: signature, IHDR, one IDAT, IEND.  The IDAT's zlib stream: 78 9C, the segments, the Adler-32 of the filtered bytes.
//  * filtered bytes: per row its filter type (0 .. 4) and the residuals.  Adaptive: the type with the smallest sum of |residual as int8|, ties to the lowest;
//  * a segment = PNG_SEGMENT_ROWS rows of filtered bytes (the last one what is left), coded on its own: nothing refers across a segment's start;
//  * inside a segment, tiles of PNG_TILE bytes: a tile's first byte is a literal (a run does not cross a tile's start), so a tile's symbols depend on
//    that tile alone.  A run of R equal bytes is one literal and then, over its R - 1 repeats, matches of distance 1: 258 as often as it goes, then the
//    rest as one match if it has 3 bytes or more, else as literals;
//  * one dynamic block per segment: literal / length lengths from the segment's histogram limited to 15 bits (Huffman depths, then zlib's overflow
//    repair), two distance codes of one bit each (code 0 is distance 1; a complete code, whatever the segment holds), the code-length code limited to 7;
//  * stored block(s) of up to 65535 bytes instead when the segment comes out smaller that way;
//  * every segment but the last is followed by an empty stored block (000, padding, 00 00 FF FF): the next one starts on a byte boundary.
#pragma once
#include <stdint.h>

namespace pnrf {

#ifndef PNRF_RULE
#define PNRF_RULE __host__ __device__ inline
#endif

constexpr int PNG_SEGMENT_ROWS = 16;
constexpr int PNG_TILE = 4096;
constexpr int PNG_NLL = 286;                 // literal / length symbols
constexpr int PNG_MAX_HDR = 352;             // entries of a block header: 4 fields, 19 code-length lengths, at most 288 coded lengths
constexpr int PNG_STORED_MAX = 65535;
constexpr int64_t PNG_MAX_PIXELS = (int64_t)1 << 28;
constexpr uint32_t PNG_ADLER_MOD = 65521u;
constexpr int PNG_FILE_HEAD = 8 + 25 + 8 + 2;      // signature, IHDR chunk, IDAT length and tag, zlib header: where the first segment starts
constexpr int PNG_FILE_TAIL = 4 + 4 + 12;          // Adler-32, IDAT CRC, IEND chunk

// ---- geometry -----------------------------------------------------------------------------------------------------------------------------------
PNRF_RULE int64_t png_row_bytes(int W, int ch) { return (int64_t)W * ch + 1; }
PNRF_RULE int64_t png_raw_bytes(int H, int W, int ch) { return (int64_t)H * png_row_bytes(W, ch); }
PNRF_RULE int64_t png_segments(int H) { return ((int64_t)H + PNG_SEGMENT_ROWS - 1) / PNG_SEGMENT_ROWS; }
PNRF_RULE int64_t png_segment_bytes(int W, int ch) { return png_row_bytes(W, ch) * PNG_SEGMENT_ROWS; }
// a segment of n filtered bytes as stored blocks, with the marker behind it unless it is the last
PNRF_RULE int64_t png_stored_bytes(int64_t n, bool last) { return n + 5 * ((n + PNG_STORED_MAX - 1) / PNG_STORED_MAX) + (last ? 0 : 5); }
// room of a segment's slot in the workspace: the stored form (nothing larger is ever written), whole 32-bit words, 16-byte granules
PNRF_RULE int64_t png_slot_bytes(int W, int ch) { return (png_stored_bytes(png_segment_bytes(W, ch), false) + 8 + 15) / 16 * 16; }
PNRF_RULE int64_t png_max_file_bytes(int H, int W, int ch) {
  const int64_t raw = png_raw_bytes(H, W, ch), ns = png_segments(H);
  return raw + 5 * (raw / PNG_STORED_MAX) + 10 * ns + PNG_FILE_HEAD + PNG_FILE_TAIL;      // every segment stored: 5 (n / 65535 + 1) + 5 each at the most
}

// ---- filters ------------------------------------------------------------------------------------------------------------------------------------
PNRF_RULE int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// residual of byte x under filter t; a = left, b = up, c = up-left (0 where there is none)
PNRF_RULE uint8_t png_residual(int t, int x, int a, int b, int c) {
  const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
  return (uint8_t)(x - pred);
}
PNRF_RULE uint32_t png_cost(uint8_t r) { return r < 128 ? r : 256u - r; }
// adaptive choice from the five sums: the smallest, ties to the lowest type
PNRF_RULE int png_choose(const uint64_t cost[5]) {
  int best = 0;
  for (int t = 1; t < 5; ++t) if (cost[t] < cost[best]) best = t;
  return best;
}

// ---- symbols ------------------------------------------------------------------------------------------------------------------------------------
// The symbol that starts at byte i of a tile, whose run of equal bytes is [s, e) (s <= i < e; s = the tile's first byte or the first byte that
// differs from the one before it, e = the next such byte or the tile's end).  Returns 0: none (inside a match), 1: a literal, L >= 3: a match of L.
PNRF_RULE int png_token(int i, int s, int e) {
  if (i == s) return 1;
  const int off = (i - s - 1) % 258, start = i - off;
  const int len = e - start < 258 ? e - start : 258;
  if (len < 3) return 1;
  return off == 0 ? len : 0;
}
// length 3 .. 258 -> code index 0 .. 28 (symbol 257 + index), extra-bit count and value
PNRF_RULE int png_len_code(int len, int* nextra, int* extra) {
  const int l = len - 3;
  if (len == 258) { *nextra = 0; *extra = 0; return 28; }
  if (l < 8) { *nextra = 0; *extra = 0; return l; }
  int lg = 3;                              // floor(log2 l)
  while ((l >> lg) > 1) ++lg;
  const int nb = lg - 2;
  *nextra = nb; *extra = l & ((1 << nb) - 1);
  return 4 * nb + 4 + ((l >> nb) & 3);
}
PNRF_RULE int png_len_code_extra(int c) { return (c < 8 || c == 28) ? 0 : (c >> 2) - 1; }

// ---- Huffman ------------------------------------------------------------------------------------------------------------------------------------
struct PngScratch {
  uint64_t keys[288];      // (count << 16 | symbol) of the used symbols, ascending
  uint32_t w[576];
  uint16_t par[576], dep[576];
  uint16_t rle[320];       // the coded length sequence: symbol | extra << 5
  uint8_t seq[320];
  int n_used;
};
struct PngCodes {
  uint32_t lit[256];       // bits | nbits << 24 of a literal
  uint32_t len[256];       // ... of a match of length 3 + index: length code, extra bits, the distance code
  uint32_t eob;
  uint32_t hdr[PNG_MAX_HDR];      // the block's header fields in order, same packing
  int nhdr;
  int stored;              // 1: the segment goes out as stored blocks
  uint64_t bits;           // dynamic block, header to end-of-block
  uint8_t ll[288];         // code lengths
};
PNRF_RULE uint32_t png_bitrev(uint32_t c, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) { r = (r << 1) | (c & 1); c >>= 1; }
  return r;
}
// Code lengths of the n >= 2 symbols of keys[] (ascending by count, then symbol) limited to maxbits, into len[symbol].  Returns whether the code is
// complete (Kraft sum exactly 1): always, for n <= 2^maxbits; a caller that sees false writes the segment as stored blocks
PNRF_RULE bool png_huff_lengths(const uint64_t* keys, int n, int maxbits, uint8_t* len, PngScratch* S) {
  uint32_t* w = S->w;
  uint16_t *par = S->par, *dep = S->dep;
  for (int i = 0; i < n; ++i) w[i] = (uint32_t)(keys[i] >> 16);
  int li = 0, ii = n, ni = n;
  for (int k = 0; k < n - 1; ++k) {
    int pick[2];
    for (int j = 0; j < 2; ++j) {
      if (li < n && (ii >= ni || w[li] <= w[ii])) pick[j] = li++;
      else pick[j] = ii++;
    }
    w[ni] = w[pick[0]] + w[pick[1]];
    par[pick[0]] = par[pick[1]] = (uint16_t)ni;
    ++ni;
  }
  dep[2 * n - 2] = 0;
  for (int j = 2 * n - 3; j >= 0; --j) dep[j] = (uint16_t)(dep[par[j]] + 1);
  int count[16];
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int i = 0; i < n; ++i) ++count[dep[i] < maxbits ? dep[i] : maxbits];
  // Leaves deeper than maxbits now sit at maxbits and the code is over-subscribed: its Kraft sum, in units of 2^-maxbits, exceeds 2^maxbits by the
  // number of repair steps it takes.  One step (zlib's gen_bitlen): a leaf of the deepest level above maxbits that has one moves a level down and a
  // leaf of level maxbits becomes its sibling — count[b]--, count[b + 1] += 2, count[maxbits]-- lowers the sum by exactly one unit.  (Counting the
  // overflowing leaves alone does not give the number of steps: a chain 18 deep has 3 of them and needs 3 steps, not 2.)
  int64_t kraft = 0;
  for (int b = 1; b <= maxbits; ++b) kraft += (int64_t)count[b] << (maxbits - b);
  const int64_t one = (int64_t)1 << maxbits;
  while (kraft > one) {
    int bits = maxbits - 1;
    while (bits > 0 && count[bits] == 0) --bits;
    if (bits == 0) break;                                       // more symbols than codes of maxbits bits: not reached for n <= 2^maxbits
    --count[bits]; count[bits + 1] += 2; --count[maxbits];
    --kraft;
  }
  int idx = 0;
  for (int bits = maxbits; bits >= 1; --bits)
    for (int c = 0; c < count[bits] && idx < n; ++c) len[keys[idx++] & 0xffff] = (uint8_t)bits;
  return kraft == one && idx == n;
}
// canonical codes of lengths len[0 .. n), bit-reversed for an LSB-first writer: code[i] = bits | nbits << 24 (0 for an unused symbol)
PNRF_RULE void png_canonical(const uint8_t* len, int n, int maxbits, uint32_t* code) {
  int count[17], next[17];
  for (int b = 0; b <= 16; ++b) count[b] = 0;
  for (int i = 0; i < n; ++i) ++count[len[i]];
  count[0] = 0;
  int c = 0;
  for (int b = 1; b <= maxbits; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
  for (int i = 0; i < n; ++i) code[i] = len[i] ? (png_bitrev((uint32_t)next[len[i]]++, len[i]) | (uint32_t)len[i] << 24) : 0u;
}
PNRF_RULE uint64_t png_sort_key(const uint32_t* hist, int sym) { return (uint64_t)hist[sym] << 16 | (uint64_t)sym; }
// place of a symbol among the used ones (ascending keys), or -1 for an unused one
PNRF_RULE int png_sort_rank(const uint32_t* hist, int n, int sym) {
  if (!hist[sym]) return -1;
  const uint64_t k = png_sort_key(hist, sym);
  int r = 0;
  for (int j = 0; j < n; ++j) r += (hist[j] != 0 && png_sort_key(hist, j) < k) ? 1 : 0;
  return r;
}

// The dynamic block of a segment from its histogram hist[286] (end-of-block counted; S->keys / S->n_used the sorted used symbols): code tables,
// header fields, the block's length in bits, and the choice between it and stored blocks for the segment's n bytes.  Serial.
PNRF_RULE void png_build_block(const uint32_t* hist, int64_t n, bool last, PngCodes* C, PngScratch* S) {
  const int cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t* ll = C->ll;
  for (int i = 0; i < 288; ++i) ll[i] = 0;
  bool complete = png_huff_lengths(S->keys, S->n_used, 15, ll, S);
  int nll = PNG_NLL;
  while (nll > 257 && ll[nll - 1] == 0) --nll;
  // the length sequence: nll literal / length lengths, then the two distance lengths, run-length coded
  uint8_t* seq = S->seq;
  for (int i = 0; i < nll; ++i) seq[i] = ll[i];
  seq[nll] = 1; seq[nll + 1] = 1;
  const int nseq = nll + 2;
  int nr = 0;
  uint32_t clh[19];
  for (int i = 0; i < 19; ++i) clh[i] = 0;
  for (int i = 0; i < nseq;) {
    const int v = seq[i];
    int r = 1;
    while (i + r < nseq && seq[i + r] == v) ++r;
    i += r;
    if (v == 0) {
      while (r > 0) {
        if (r >= 11) { const int c = r < 138 ? r : 138; S->rle[nr++] = (uint16_t)(18 | (c - 11) << 5); ++clh[18]; r -= c; }
        else if (r >= 3) { S->rle[nr++] = (uint16_t)(17 | (r - 3) << 5); ++clh[17]; r = 0; }
        else { S->rle[nr++] = 0; ++clh[0]; --r; }
      }
    } else {
      S->rle[nr++] = (uint16_t)v; ++clh[v]; --r;
      while (r >= 3) { const int c = r < 6 ? r : 6; S->rle[nr++] = (uint16_t)(16 | (c - 3) << 5); ++clh[16]; r -= c; }
      while (r > 0) { S->rle[nr++] = (uint16_t)v; ++clh[v]; --r; }
    }
  }
  // the code-length code: at least two symbols (a complete code), 7 bits at the most
  uint64_t ck[19];
  int nck = 0;
  for (int i = 0; i < 19; ++i) if (clh[i]) ck[nck++] = (uint64_t)clh[i] << 16 | (uint64_t)i;
  if (nck == 1) { const uint64_t other = (ck[0] & 0xffff) == 0 ? 1 : 0; ck[nck++] = other; }
  for (int i = 1; i < nck; ++i) {      // insertion sort, ascending
    const uint64_t k = ck[i];
    int j = i - 1;
    while (j >= 0 && ck[j] > k) { ck[j + 1] = ck[j]; --j; }
    ck[j + 1] = k;
  }
  uint8_t cl[19];
  for (int i = 0; i < 19; ++i) cl[i] = 0;
  complete = png_huff_lengths(ck, nck, 7, cl, S) && complete;
  uint32_t clc[19];
  png_canonical(cl, 19, 7, clc);
  int ncl = 19;
  while (ncl > 4 && cl[cl_order[ncl - 1]] == 0) --ncl;
  // header fields
  int nh = 0;
  uint64_t bits = 0;
  auto put = [&](uint32_t v, int nb) { C->hdr[nh++] = v | (uint32_t)nb << 24; bits += (uint64_t)nb; };
  put((last ? 1u : 0u) | 2u << 1, 3);
  put((uint32_t)(nll - 257), 5);
  put(1u, 5);
  put((uint32_t)(ncl - 4), 4);
  for (int i = 0; i < ncl; ++i) put(cl[cl_order[i]], 3);
  for (int i = 0; i < nr; ++i) {
    const int sym = S->rle[i] & 31, ex = S->rle[i] >> 5;
    const int cb = (int)(clc[sym] >> 24), eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
    put((clc[sym] & 0xffffff) | (uint32_t)ex << cb, cb + eb);
  }
  C->nhdr = nh;
  // symbol tables
  uint32_t* code = S->w;      // the Huffman scratch is free again
  png_canonical(ll, PNG_NLL, 15, code);
  for (int i = 0; i < 256; ++i) { C->lit[i] = code[i]; bits += (uint64_t)hist[i] * ll[i]; }
  C->eob = code[256]; bits += ll[256];
  for (int L = 3; L <= 258; ++L) {
    int nx, ex;
    const int c = png_len_code(L, &nx, &ex);
    const int cb = ll[257 + c];
    C->len[L - 3] = cb ? ((code[257 + c] & 0xffffff) | (uint32_t)ex << cb | (uint32_t)(cb + nx + 1) << 24) : 0u;      // distance code 0: one 0 bit
  }
  for (int c = 0; c < 29; ++c) bits += (uint64_t)hist[257 + c] * (uint64_t)(ll[257 + c] + png_len_code_extra(c) + 1);
  C->bits = bits;
  const int64_t dyn = last ? (int64_t)((bits + 7) / 8) : (int64_t)((bits + 3 + 7) / 8) + 4;
  C->stored = (!complete || png_stored_bytes(n, last) < dyn) ? 1 : 0;      // an incomplete code never goes out
}
// what a segment written as a dynamic block takes, marker included
PNRF_RULE int64_t png_dynamic_bytes(uint64_t bits, bool last) { return last ? (int64_t)((bits + 7) / 8) : (int64_t)((bits + 3 + 7) / 8) + 4; }
// byte o of a segment of n bytes written as stored blocks (src = its filtered bytes)
PNRF_RULE uint8_t png_stored_byte(int64_t o, const uint8_t* src, int64_t n, bool last) {
  const int64_t body = n + 5 * ((n + PNG_STORED_MAX - 1) / PNG_STORED_MAX);
  if (o >= body) { const int64_t k = o - body; return k >= 3 ? 0xff : 0x00; }      // 00 00 00 FF FF
  const int64_t blk = o / (PNG_STORED_MAX + 5), r = o % (PNG_STORED_MAX + 5);
  if (r >= 5) return src[blk * PNG_STORED_MAX + r - 5];
  const int64_t left = n - blk * PNG_STORED_MAX;
  const uint32_t len = (uint32_t)(left < PNG_STORED_MAX ? left : PNG_STORED_MAX);
  const bool final = last && left <= PNG_STORED_MAX;
  return r == 0 ? (final ? 1 : 0) : r == 1 ? (uint8_t)len : r == 2 ? (uint8_t)(len >> 8) : r == 3 ? (uint8_t)~len : (uint8_t)(~len >> 8);
}

// ---- checksums ----------------------------------------------------------------------------------------------------------------------------------
// CRC-32 (reflected 0xEDB88320).  A piece's CRC is the standard one (crc32 of the piece alone); pieces combine as zlib's crc32_combine:
// crc(A B) = crc(A) x^(8 |B|) + crc(B) in GF(2)[x] mod p
PNRF_RULE uint32_t png_crc_byte(uint32_t c, uint8_t b) {
  c ^= b;
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}
PNRF_RULE uint32_t png_crc(const uint8_t* p, int64_t n) {
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < n; ++i) c = png_crc_byte(c, p[i]);
  return n > 0 ? ~c : 0u;
}
PNRF_RULE uint32_t png_multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// x^(8 n) mod p
PNRF_RULE uint32_t png_x8n(uint64_t n) {
  uint32_t p = 1u << 31, q = 1u << 23;      // x^0, x^8
  while (n) {
    if (n & 1) p = png_multmodp(q, p);
    q = png_multmodp(q, q);
    n >>= 1;
  }
  return p;
}
// a piece's CRC moved in front of `after` more bytes; the CRC of the whole is the XOR of every piece's
PNRF_RULE uint32_t png_crc_shift(uint32_t crc, uint64_t after) { return crc ? png_multmodp(png_x8n(after), crc) : 0u; }
// Adler-32 piece sums of n bytes: S = sum b_j, T = sum (n - j) b_j, both mod 65521.  For the whole of N bytes: s1 = 1 + sum S,
// s2 = N + sum (T + S * bytes after the piece), mod 65521
PNRF_RULE void png_adler_piece(const uint8_t* p, int64_t n, uint32_t* S, uint32_t* T) {
  uint64_t s = 0, t = 0;
  for (int64_t j = 0; j < n; ++j) {
    s += p[j]; t += s;
    if ((j & 0xffff) == 0xffff) { s %= PNG_ADLER_MOD; t %= PNG_ADLER_MOD; }
  }
  *S = (uint32_t)(s % PNG_ADLER_MOD); *T = (uint32_t)(t % PNG_ADLER_MOD);
}
PNRF_RULE uint32_t png_adler_s2_term(uint32_t S, uint32_t T, uint64_t after) { return (uint32_t)((T + (uint64_t)S * (after % PNG_ADLER_MOD)) % PNG_ADLER_MOD); }

}  // namespace pnrf
