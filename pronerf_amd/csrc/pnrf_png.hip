// pnrf_png.hip — a finished frame's 8-bit plane as the bytes of a PNG file: pnrf_png_encode_host (plain C++, the twin) and pnrf_png_encode_fwd
// (four launches in stream order).  Every format rule is a function of pnrf_png_rules.h, called from both.
//   png_filter_kernel    one wave per row: the five candidates' costs, the choice, the filtered row into the workspace
//   png_segment_kernel   one workgroup per segment: tiles of the filtered bytes through LDS, run detection and histogram (LDS atomics), the
//                        code construction (sorted in parallel, built on one lane), then the bit packing (prefix sum of the symbols' bit
//                        lengths, OR into LDS words) or the stored form into the segment's slot; the segment's Adler-32 and CRC-32 pieces
//   png_finish_kernel    one workgroup: exclusive scan of the segment sizes, both checksums combined, the file's head and tail, its length
//   png_copy_kernel      each slot to its offset in the file
// Kernel boundaries are the only hand-off between workgroups; nothing is allocated, read back or decided on the host from the file's contents.
#include "pnrf_common.h"
#include "pnrf_png_rules.h"

#include <string.h>

namespace pnrf {
namespace {

struct PngSegMeta { uint32_t size, crc, adler_s, adler_t; };

struct PngLayout { int64_t filt, slots, meta, offs, total, raw, nseg, seg_bytes, slot; };
PngLayout png_layout(int H, int W, int ch) {
  PngLayout L;
  L.raw = png_raw_bytes(H, W, ch); L.nseg = png_segments(H); L.seg_bytes = png_segment_bytes(W, ch); L.slot = png_slot_bytes(W, ch);
  auto up = [](int64_t x) { return (x + 15) / 16 * 16; };
  L.filt = 0;
  L.slots = up(L.raw);
  L.meta = L.slots + L.nseg * L.slot;
  L.offs = L.meta + L.nseg * (int64_t)sizeof(PngSegMeta);
  L.total = up(L.offs + L.nseg * 8);
  return L;
}

__host__ __device__ inline void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// head and tail of the file around zbytes bytes of segments (one lane / the host)
__host__ __device__ inline int64_t png_frame(uint8_t* out, int H, int W, int ch, int64_t zbytes, uint32_t adler, uint32_t crc_segments) {
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  for (int i = 0; i < 8; ++i) out[i] = sig[i];
  uint8_t* p = out + 8;
  put_be32(p, 13); p[4] = 'I'; p[5] = 'H'; p[6] = 'D'; p[7] = 'R';
  put_be32(p + 8, (uint32_t)W); put_be32(p + 12, (uint32_t)H);
  p[16] = 8; p[17] = ch == 3 ? 2 : 0; p[18] = 0; p[19] = 0; p[20] = 0;
  put_be32(p + 21, png_crc(p + 4, 17));
  p = out + 33;
  put_be32(p, (uint32_t)(2 + zbytes + 4)); p[4] = 'I'; p[5] = 'D'; p[6] = 'A'; p[7] = 'T'; p[8] = 0x78; p[9] = 0x9c;
  uint8_t* q = out + PNG_FILE_HEAD + zbytes;
  put_be32(q, adler);
  const uint32_t crc = png_crc_shift(png_crc(p + 4, 6), (uint64_t)zbytes + 4) ^ png_crc_shift(crc_segments, 4) ^ png_crc(q, 4);
  put_be32(q + 4, crc);
  put_be32(q + 8, 0); q[12] = 'I'; q[13] = 'E'; q[14] = 'N'; q[15] = 'D'; q[16] = 0xae; q[17] = 0x42; q[18] = 0x60; q[19] = 0x82;
  return PNG_FILE_HEAD + zbytes + PNG_FILE_TAIL;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------------
struct HostBits {
  std::vector<uint8_t>& out;
  uint64_t acc = 0;
  int n = 0;
  void put(uint32_t packed) { acc |= (uint64_t)(packed & 0xffffff) << n; n += (int)(packed >> 24); while (n >= 8) { out.push_back((uint8_t)acc); acc >>= 8; n -= 8; } }
  void align() { if (n > 0) { out.push_back((uint8_t)acc); acc = 0; n = 0; } }
};

void host_tokens(const uint8_t* src, int64_t n, std::vector<int>& tok) {
  tok.assign((size_t)n, 0);
  for (int64_t base = 0; base < n; base += PNG_TILE) {
    const int nt = (int)(n - base < PNG_TILE ? n - base : PNG_TILE);
    const uint8_t* B = src + base;
    int s = 0;
    while (s < nt) {
      int e = s + 1;
      while (e < nt && B[e] == B[s]) ++e;
      for (int i = s; i < e; ++i) tok[(size_t)(base + i)] = png_token(i, s, e);
      s = e;
    }
  }
}

void host_segment(const uint8_t* src, int64_t n, bool last, std::vector<uint8_t>& seg) {
  std::vector<int> tok;
  host_tokens(src, n, tok);
  uint32_t hist[288] = {0};
  for (int64_t i = 0; i < n; ++i) {
    int nx, ex;
    if (tok[(size_t)i] == 1) ++hist[src[i]];
    else if (tok[(size_t)i] >= 3) ++hist[257 + png_len_code(tok[(size_t)i], &nx, &ex)];
  }
  hist[256] = 1;
  static thread_local PngCodes C;
  static thread_local PngScratch S;
  S.n_used = 0;
  for (int sym = 0; sym < PNG_NLL; ++sym) {
    const int r = png_sort_rank(hist, PNG_NLL, sym);
    if (r >= 0) { S.keys[r] = png_sort_key(hist, sym); ++S.n_used; }
  }
  png_build_block(hist, n, last, &C, &S);
  seg.clear();
  if (C.stored) {
    const int64_t sz = png_stored_bytes(n, last);
    seg.resize((size_t)sz);
    for (int64_t o = 0; o < sz; ++o) seg[(size_t)o] = png_stored_byte(o, src, n, last);
    return;
  }
  HostBits w{seg};
  for (int i = 0; i < C.nhdr; ++i) w.put(C.hdr[i]);
  for (int64_t i = 0; i < n; ++i) {
    if (tok[(size_t)i] == 1) w.put(C.lit[src[i]]);
    else if (tok[(size_t)i] >= 3) w.put(C.len[tok[(size_t)i] - 3]);
  }
  w.put(C.eob);
  if (!last) w.put(3u << 24);
  w.align();
  if (!last) { seg.push_back(0); seg.push_back(0); seg.push_back(0xff); seg.push_back(0xff); }
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------
constexpr int TPB = 256;
constexpr int PER = PNG_TILE / TPB;      // consecutive bytes of a tile per lane
constexpr int W_WORDS = 2304;            // bit buffer: a tile of 15-bit literals (1920 words) or the header (154), and the carried word

__global__ __launch_bounds__(TPB) void png_filter_kernel(const uint8_t* __restrict__ img, int64_t stride, int H, int rb, int bpp, int filter, uint8_t* __restrict__ filt) {
  const int row = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= H) return;
  const uint8_t* cur = img + (int64_t)row * stride;
  const uint8_t* prev = row > 0 ? cur - stride : nullptr;
  int t = filter;
  if (filter < 0) {
    uint64_t cost[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < rb; x += 64) {
      const int X = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = prev ? prev[x] : 0, c = (prev && x >= bpp) ? prev[x - bpp] : 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) cost[k] += png_cost(png_residual(k, X, a, b, c));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      for (int d = 32; d >= 1; d >>= 1) cost[k] += (uint64_t)__shfl_xor((unsigned long long)cost[k], d, 64);
    t = png_choose(cost);
  }
  uint8_t* dst = filt + (int64_t)row * ((int64_t)rb + 1);
  if (lane == 0) dst[0] = (uint8_t)t;
  for (int x = lane; x < rb; x += 64) {
    const int X = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = prev ? prev[x] : 0, c = (prev && x >= bpp) ? prev[x - bpp] : 0;
    dst[1 + x] = png_residual(t, X, a, b, c);
  }
}

struct SegShared {
  uint8_t B[PNG_TILE];
  int sa[TPB], sb[TPB];
  uint32_t W[W_WORDS];
  uint32_t hist[288];
  PngCodes C;
  PngScratch S;
};

// The symbols that start at this lane's PER bytes of the tile in sh.B (nt bytes): tok[j] as png_token.  All lanes call it; ends with a barrier.
__device__ inline void tile_tokens(SegShared& sh, int nt, int tid, int tok[PER]) {
  const int p0 = tid * PER;
  uint32_t f = 0;
  for (int j = 0; j < PER; ++j) {
    const int i = p0 + j;
    if (i < nt && (i == 0 || sh.B[i] != sh.B[i - 1])) f |= 1u << j;
  }
  sh.sa[tid] = f ? p0 + 31 - __clz(f) : -1;
  sh.sb[tid] = f ? p0 + __ffs(f) - 1 : nt;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {      // inclusive max scan forwards, min scan backwards
    const int a = tid >= d ? sh.sa[tid - d] : -1, b = tid + d < TPB ? sh.sb[tid + d] : nt;
    __syncthreads();
    sh.sa[tid] = max(sh.sa[tid], a); sh.sb[tid] = min(sh.sb[tid], b);
    __syncthreads();
  }
  int s = tid > 0 ? sh.sa[tid - 1] : -1, en = tid + 1 < TPB ? sh.sb[tid + 1] : nt;
  int e[PER];
#pragma unroll
  for (int j = PER - 1; j >= 0; --j) { e[j] = en; if (f >> j & 1) en = p0 + j; }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = p0 + j;
    if (f >> j & 1) s = i;
    tok[j] = i < nt ? png_token(i, s, e[j]) : 0;
  }
  __syncthreads();
}

__device__ inline void or_bits(uint32_t* W, uint32_t pos, uint32_t packed) {
  const uint32_t v = packed & 0xffffff, nb = packed >> 24, w = pos >> 5, sh = pos & 31;
  if (!nb) return;
  atomicOr(&W[w], v << sh);
  if (sh + nb > 32) atomicOr(&W[w + 1], v >> (32 - sh));
}

__global__ __launch_bounds__(TPB) void png_segment_kernel(const uint8_t* __restrict__ filt, int64_t raw, int64_t seg_bytes, int64_t nseg, uint8_t* slots, int64_t slot,
                                                          PngSegMeta* __restrict__ meta) {
  __shared__ SegShared sh;
  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int64_t n = raw - seg * seg_bytes < seg_bytes ? raw - seg * seg_bytes : seg_bytes;
  const bool last = seg == nseg - 1;
  const uint8_t* src = filt + seg * seg_bytes;
  uint8_t* dst = slots + seg * slot;
  uint32_t* dstw = (uint32_t*)dst;
  int tok[PER];

  for (int k = tid; k < 288; k += TPB) sh.hist[k] = 0;
  for (int k = tid; k < W_WORDS; k += TPB) sh.W[k] = 0;
  __syncthreads();
  // pass 1: histogram of the symbols
  for (int64_t base = 0; base < n; base += PNG_TILE) {
    const int nt = (int)(n - base < PNG_TILE ? n - base : PNG_TILE);
    for (int k = tid; k < nt; k += TPB) sh.B[k] = src[base + k];
    __syncthreads();
    tile_tokens(sh, nt, tid, tok);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      int nx, ex;
      if (tok[j] == 1) atomicAdd(&sh.hist[sh.B[tid * PER + j]], 1u);
      else if (tok[j] >= 3) atomicAdd(&sh.hist[257 + png_len_code(tok[j], &nx, &ex)], 1u);
    }
    __syncthreads();
  }
  if (tid == 0) sh.hist[256] = 1;
  __syncthreads();
  // the used symbols in ascending order of (count, symbol), then the codes on one lane
  for (int sym = tid; sym < PNG_NLL; sym += TPB) {
    const int r = png_sort_rank(sh.hist, PNG_NLL, sym);
    if (r >= 0) sh.S.keys[r] = png_sort_key(sh.hist, sym);
  }
  if (tid == 0) {
    int used = 0;
    for (int sym = 0; sym < PNG_NLL; ++sym) used += sh.hist[sym] != 0;
    sh.S.n_used = used;
  }
  __syncthreads();
  if (tid == 0) png_build_block(sh.hist, n, last, &sh.C, &sh.S);
  __syncthreads();

  int64_t size;
  if (sh.C.stored) {
    size = png_stored_bytes(n, last);
    for (int64_t o = tid; o < size; o += TPB) dst[o] = png_stored_byte(o, src, n, last);
  } else {
    // pass 2: the bits.  cur_bits (< 32 after a flush) bits stand in W[0]; words_out 32-bit words are in the slot.  Uniform over the lanes.
    uint32_t cur_bits = 0;
    int64_t words_out = 0;
    auto flush = [&](uint32_t added, bool final) {      // all lanes, behind a barrier that follows the ORs
      const uint32_t tb = cur_bits + added, nw = final ? (tb + 31) >> 5 : tb >> 5;
      for (uint32_t k = tid; k < nw; k += TPB) dstw[words_out + k] = sh.W[k];
      const uint32_t part = sh.W[nw];
      __syncthreads();
      for (uint32_t k = tid; k <= nw; k += TPB) sh.W[k] = 0;
      __syncthreads();
      if (tid == 0 && !final) sh.W[0] = part;
      __syncthreads();
      words_out += nw; cur_bits = final ? 0 : tb & 31;
    };
    if (tid == 0) {
      uint32_t pos = 0;
      for (int i = 0; i < sh.C.nhdr; ++i) { or_bits(sh.W, pos, sh.C.hdr[i]); pos += sh.C.hdr[i] >> 24; }
      sh.sa[0] = (int)pos;
    }
    __syncthreads();
    const uint32_t hdr_bits = (uint32_t)sh.sa[0];
    __syncthreads();
    flush(hdr_bits, false);
    for (int64_t base = 0; base < n; base += PNG_TILE) {
      const int nt = (int)(n - base < PNG_TILE ? n - base : PNG_TILE);
      for (int k = tid; k < nt; k += TPB) sh.B[k] = src[base + k];
      __syncthreads();
      tile_tokens(sh, nt, tid, tok);
      uint32_t code[PER];
      int mine = 0;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        code[j] = tok[j] == 1 ? sh.C.lit[sh.B[tid * PER + j]] : tok[j] >= 3 ? sh.C.len[tok[j] - 3] : 0u;
        mine += (int)(code[j] >> 24);
      }
      sh.sa[tid] = mine;
      __syncthreads();
      for (int d = 1; d < TPB; d <<= 1) {      // inclusive prefix sum of the lanes' bit counts
        const int a = tid >= d ? sh.sa[tid - d] : 0;
        __syncthreads();
        sh.sa[tid] += a;
        __syncthreads();
      }
      const uint32_t total = (uint32_t)sh.sa[TPB - 1];
      uint32_t pos = cur_bits + (uint32_t)(sh.sa[tid] - mine);
#pragma unroll
      for (int j = 0; j < PER; ++j) { or_bits(sh.W, pos, code[j]); pos += code[j] >> 24; }
      __syncthreads();
      flush(total, false);
    }
    if (tid == 0) {      // end of block, the marker's 000, padding; then 00 00 FF FF behind a segment that is not the last
      uint32_t pos = cur_bits;
      or_bits(sh.W, pos, sh.C.eob); pos += sh.C.eob >> 24;
      if (!last) pos += 3;
      pos = (pos + 7) & ~7u;
      if (!last) { pos += 16; or_bits(sh.W, pos, 0xffffu | 16u << 24); pos += 16; }
      sh.sa[0] = (int)(pos - cur_bits);
    }
    __syncthreads();
    const uint32_t tail = (uint32_t)sh.sa[0];
    __syncthreads();
    size = words_out * 4 + (cur_bits + tail) / 8;
    flush(tail, true);
  }
  __syncthreads();      // the slot's bytes, written by every lane, are read below by others

  // checksum pieces: CRC-32 of the slot's bytes, Adler-32 sums of the filtered bytes, each lane a stretch, combined by the rules
  const int64_t cs = (size + TPB - 1) / TPB, clo = min((int64_t)tid * cs, size), chi = min(clo + cs, size);
  sh.sa[tid] = (int)png_crc_shift(png_crc(dst + clo, chi - clo), (uint64_t)(size - chi));
  const int64_t as = (n + TPB - 1) / TPB, alo = min((int64_t)tid * as, n), ahi = min(alo + as, n);
  uint32_t S, T;
  png_adler_piece(src + alo, ahi - alo, &S, &T);
  sh.sb[tid] = (int)S;
  sh.W[tid] = png_adler_s2_term(S, T, (uint64_t)(n - ahi));
  __syncthreads();
  if (tid == 0) {
    uint32_t crc = 0;
    uint64_t s = 0, t = 0;
    for (int k = 0; k < TPB; ++k) { crc ^= (uint32_t)sh.sa[k]; s += (uint32_t)sh.sb[k]; t += sh.W[k]; }
    PngSegMeta m;
    m.size = (uint32_t)size; m.crc = crc; m.adler_s = (uint32_t)(s % PNG_ADLER_MOD); m.adler_t = (uint32_t)(t % PNG_ADLER_MOD);
    meta[seg] = m;
  }
}

__global__ __launch_bounds__(TPB) void png_finish_kernel(const PngSegMeta* __restrict__ meta, int64_t nseg, int64_t raw, int64_t seg_bytes, int H, int W, int ch,
                                                         int64_t* __restrict__ offs, uint8_t* __restrict__ out, int64_t* __restrict__ size_dev) {
  __shared__ int64_t sc[TPB];
  __shared__ uint32_t xs[TPB], ss[TPB], ts[TPB];
  const int tid = threadIdx.x;
  // exclusive scan of the sizes
  int64_t carry = 0;
  for (int64_t base = 0; base < nseg; base += TPB) {
    const int64_t i = base + tid;
    const int64_t mine = i < nseg ? (int64_t)meta[i].size : 0;
    sc[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
      const int64_t a = tid >= d ? sc[tid - d] : 0;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    if (i < nseg) offs[i] = carry + sc[tid] - mine;
    carry += sc[TPB - 1];
    __syncthreads();
  }
  const int64_t zbytes = carry;
  // every segment's pieces, moved in front of what follows it
  uint32_t crc = 0;
  uint64_t s = 0, t = 0;
  for (int64_t i = tid; i < nseg; i += TPB) {
    const PngSegMeta m = meta[i];
    const int64_t end = offs[i] + m.size;
    crc ^= png_crc_shift(m.crc, (uint64_t)(zbytes - end));
    const int64_t fend = (i + 1) * seg_bytes < raw ? (i + 1) * seg_bytes : raw;
    s += m.adler_s;
    t += png_adler_s2_term(m.adler_s, m.adler_t, (uint64_t)(raw - fend));
  }
  xs[tid] = crc; ss[tid] = (uint32_t)(s % PNG_ADLER_MOD); ts[tid] = (uint32_t)(t % PNG_ADLER_MOD);
  __syncthreads();
  if (tid == 0) {
    crc = 0; s = 1; t = (uint64_t)raw % PNG_ADLER_MOD;
    for (int k = 0; k < TPB; ++k) { crc ^= xs[k]; s += ss[k]; t += ts[k]; }
    const uint32_t adler = (uint32_t)(t % PNG_ADLER_MOD) << 16 | (uint32_t)(s % PNG_ADLER_MOD);
    *size_dev = png_frame(out, H, W, ch, zbytes, adler, crc);
  }
}

__global__ __launch_bounds__(TPB) void png_copy_kernel(const uint8_t* __restrict__ slots, int64_t slot, const PngSegMeta* __restrict__ meta, const int64_t* __restrict__ offs,
                                                       uint8_t* __restrict__ out) {
  const int64_t seg = blockIdx.x;
  const int64_t size = meta[seg].size;
  const uint8_t* src = slots + seg * slot;
  uint8_t* dst = out + PNG_FILE_HEAD + offs[seg];
  for (int64_t k = (int64_t)blockIdx.y * TPB + threadIdx.x; k < size; k += (int64_t)gridDim.y * TPB) dst[k] = src[k];
}

int png_check(const char* fn, const void* img, int64_t row_stride, int H, int W, int channels, int filter, const void* out, int64_t capacity, const void* size) {
  PNRF_REQUIRE(img && out && size, PNRF_E_ARG, "%s: null pointer", fn);
  PNRF_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= PNG_MAX_PIXELS, PNRF_E_ARG, "%s: image of %d x %d pixels (each side >= 1, at most 2^28 pixels)", fn, H, W);
  PNRF_REQUIRE(channels == 1 || channels == 3, PNRF_E_ARG, "%s: %d channels, need 1 or 3", fn, channels);
  PNRF_REQUIRE(filter >= -1 && filter <= 4, PNRF_E_ARG, "%s: filter %d outside -1 .. 4", fn, filter);
  PNRF_REQUIRE(row_stride >= (int64_t)W * channels, PNRF_E_ARG, "%s: row stride of %lld bytes below the row's %lld", fn, (long long)row_stride, (long long)W * channels);
  PNRF_REQUIRE(capacity >= png_max_file_bytes(H, W, channels), PNRF_E_ARG, "%s: room for %lld bytes, pnrf_png_max_bytes is %lld", fn, (long long)capacity,
               (long long)png_max_file_bytes(H, W, channels));
  return 0;
}

}  // namespace
}  // namespace pnrf

using namespace pnrf;

extern "C" int pnrf_png_segment_rows(void) { return PNG_SEGMENT_ROWS; }

extern "C" int64_t pnrf_png_max_bytes(int H, int W, int channels) {
  if (H < 1 || W < 1 || (int64_t)H * W > PNG_MAX_PIXELS || (channels != 1 && channels != 3)) return 0;
  return png_max_file_bytes(H, W, channels);
}

extern "C" int64_t pnrf_png_workspace_bytes(int H, int W, int channels) {
  if (H < 1 || W < 1 || (int64_t)H * W > PNG_MAX_PIXELS || (channels != 1 && channels != 3)) return 0;
  return png_layout(H, W, channels).total;
}

extern "C" int pnrf_png_encode_host(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int filter, uint8_t* out, int64_t capacity, int64_t* size) {
  if (int rc = png_check("pnrf_png_encode_host", img, row_stride, H, W, channels, filter, out, capacity, size)) return rc;
  const int rb = W * channels;
  const int64_t raw = png_raw_bytes(H, W, channels), nseg = png_segments(H), seg_bytes = png_segment_bytes(W, channels);
  std::vector<uint8_t> filt((size_t)raw), seg;
  for (int row = 0; row < H; ++row) {
    const uint8_t* cur = img + (int64_t)row * row_stride;
    const uint8_t* prev = row > 0 ? cur - row_stride : nullptr;
    auto nb = [&](int x, int* a, int* b, int* c) { *a = x >= channels ? cur[x - channels] : 0; *b = prev ? prev[x] : 0; *c = (prev && x >= channels) ? prev[x - channels] : 0; };
    int t = filter, a, b, c;
    if (filter < 0) {
      uint64_t cost[5] = {0, 0, 0, 0, 0};
      for (int x = 0; x < rb; ++x) {
        nb(x, &a, &b, &c);
        for (int k = 0; k < 5; ++k) cost[k] += png_cost(png_residual(k, cur[x], a, b, c));
      }
      t = png_choose(cost);
    }
    uint8_t* dst = &filt[(size_t)row * ((size_t)rb + 1)];
    dst[0] = (uint8_t)t;
    for (int x = 0; x < rb; ++x) { nb(x, &a, &b, &c); dst[1 + x] = png_residual(t, cur[x], a, b, c); }
  }
  int64_t z = 0;
  uint32_t crc = 0;
  uint64_t s = 1, t2 = (uint64_t)raw % PNG_ADLER_MOD;
  std::vector<int64_t> ends((size_t)nseg);
  std::vector<uint32_t> crcs((size_t)nseg);
  for (int64_t i = 0; i < nseg; ++i) {
    const int64_t lo = i * seg_bytes, n = raw - lo < seg_bytes ? raw - lo : seg_bytes;
    host_segment(&filt[(size_t)lo], n, i == nseg - 1, seg);
    if (z + (int64_t)seg.size() + PNG_FILE_HEAD + PNG_FILE_TAIL > capacity) { set_error("pnrf_png_encode_host: segment %lld leaves the bound", (long long)i); return PNRF_E_STATE; }
    memcpy(out + PNG_FILE_HEAD + z, seg.data(), seg.size());
    z += (int64_t)seg.size();
    ends[(size_t)i] = z; crcs[(size_t)i] = png_crc(seg.data(), (int64_t)seg.size());
    uint32_t S, T;
    png_adler_piece(&filt[(size_t)lo], n, &S, &T);
    s += S; t2 += png_adler_s2_term(S, T, (uint64_t)(raw - lo - n));
  }
  for (int64_t i = 0; i < nseg; ++i) crc ^= png_crc_shift(crcs[(size_t)i], (uint64_t)(z - ends[(size_t)i]));
  *size = png_frame(out, H, W, channels, z, (uint32_t)(t2 % PNG_ADLER_MOD) << 16 | (uint32_t)(s % PNG_ADLER_MOD), crc);
  return 0;
}

extern "C" int pnrf_png_encode_fwd(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int filter, uint8_t* out, int64_t capacity, int64_t* size_dev,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = png_check("pnrf_png_encode_fwd", img, row_stride, H, W, channels, filter, out, capacity, size_dev)) return rc;
  const PngLayout L = png_layout(H, W, channels);
  PNRF_REQUIRE(workspace && workspace_bytes >= L.total && ((uintptr_t)workspace & 15) == 0, PNRF_E_ARG,
               "pnrf_png_encode_fwd: workspace of %lld bytes (16-byte aligned) needed, got %lld at %p", (long long)L.total, (long long)workspace_bytes, workspace);
  PNRF_REQUIRE(((uintptr_t)size_dev & 7) == 0, PNRF_E_ARG, "pnrf_png_encode_fwd: size_dev not 8-byte aligned");
  uint8_t* ws = (uint8_t*)workspace;
  uint8_t *filt = ws + L.filt, *slots = ws + L.slots;
  PngSegMeta* meta = (PngSegMeta*)(ws + L.meta);
  int64_t* offs = (int64_t*)(ws + L.offs);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((H + 3) / 4)), dim3(TPB), 0, st, img, row_stride, H, W * channels, channels, filter, filt);
  PNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)L.nseg), dim3(TPB), 0, st, (const uint8_t*)filt, L.raw, L.seg_bytes, L.nseg, slots, L.slot, meta);
  PNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(TPB), 0, st, (const PngSegMeta*)meta, L.nseg, L.raw, L.seg_bytes, H, W, channels, offs, out, size_dev);
  PNRF_LAUNCH_CHECK();
  const unsigned split = L.slot >= 8 * 4096 ? 8u : (unsigned)((L.slot + 4095) / 4096);      // workgroups per slot
  hipLaunchKernelGGL(png_copy_kernel, dim3((unsigned)L.nseg, split), dim3(TPB), 0, st, (const uint8_t*)slots, L.slot, (const PngSegMeta*)meta, (const int64_t*)offs, out);
  PNRF_LAUNCH_CHECK();
  return 0;
}
