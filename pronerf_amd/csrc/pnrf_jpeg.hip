// pnrf_jpeg.hip — an 8-bit plane as the bytes of a baseline JPEG file: pnrf_jpeg_encode_host (plain C++, the twin) and pnrf_jpeg_encode_fwd (four
// launches in stream order).  Every format rule is a function of pnrf_jpeg_rules.h, called from both.
//   jpeg_transform_kernel  one lane per 8 x 8 block: colour conversion, edge replication, DCT, quantisation; 64 int16 in zigzag order into the workspace
//   jpeg_entropy_kernel    one workgroup per MCU row = restart interval, in tiles of 256 blocks, one lane per block: the block's bit count from the
//                          rule tables, a prefix sum, its codes ORed into LDS words (MSB first); then the tile's whole bytes: FF bytes counted per
//                          lane, a prefix sum, the stuffed bytes into the row's slot; the bits left over open the next tile; 1-bits fill the last
//                          byte, RSTm follows, the slot's length is recorded
//   jpeg_finish_kernel     one workgroup: exclusive scan of the slot lengths, the header, EOI, the file's length
//   jpeg_copy_kernel       each slot to its offset in the file
// Kernel boundaries are the only hand-off between workgroups; nothing is allocated, read back or decided on the host from the file's contents.
#include "pnrf_common.h"
#include "pnrf_jpeg_rules.h"

#include <string.h>

#include <vector>

namespace pnrf {
namespace {

struct JpegLayout { int64_t coef, slots, sizes, offs, total, rows, row_blocks, slot; };
JpegLayout jpeg_layout(int H, int W, int ch) {
  JpegLayout L;
  L.rows = jpeg_mcu_rows(H); L.row_blocks = jpeg_row_blocks(W, ch); L.slot = jpeg_slot_bytes(W, ch);
  auto up = [](int64_t x) { return (x + 15) / 16 * 16; };
  L.coef = 0;
  L.slots = up(L.rows * L.row_blocks * 64 * (int64_t)sizeof(int16_t));
  L.sizes = L.slots + L.rows * L.slot;
  L.offs = L.sizes + L.rows * 8;
  L.total = up(L.offs + L.rows * 8);
  return L;
}

bool jpeg_shape_ok(int H, int W, int ch) { return H >= 1 && W >= 1 && H <= JPEG_MAX_SIDE && W <= JPEG_MAX_SIDE && (ch == 1 || ch == 3); }

// block j of MCU row `row` (coding order: MCU j / ch, component j % ch) as 64 quantised coefficients in zigzag order; q: the component's table, row-major
__host__ __device__ inline void jpeg_block(const uint8_t* img, int64_t stride, int H, int W, int ch, int64_t row, int64_t j, const uint16_t* q, int16_t* zz) {
  const int c = (int)(j % ch), y0 = (int)row * 8, x0 = (int)(j / ch) * 8;
  int32_t d[64];
#pragma unroll
  for (int y = 0; y < 8; ++y)
#pragma unroll
    for (int x = 0; x < 8; ++x) d[8 * y + x] = jpeg_sample(img, stride, H, W, ch, c, y0 + y, x0 + x);
  jpeg_fdct(d);
#pragma unroll
  for (int k = 0; k < 64; ++k) zz[k] = (int16_t)jpeg_quantise(d[jpeg_natural(k)], q[jpeg_natural(k)]);
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------------
struct HostBits {
  std::vector<uint8_t>& out;
  uint64_t acc = 0;
  int n = 0;
  void byte(uint8_t b) { out.push_back(b); if (b == 0xff) out.push_back(0); }
  void put(uint32_t coded) {
    const int nb = (int)(coded >> 27);
    acc = acc << nb | (coded & 0x7ffffff); n += nb;
    while (n >= 8) { byte((uint8_t)(acc >> (n - 8))); n -= 8; }
  }
  void fill() { if (n > 0) put(((1u << (8 - n)) - 1) | (uint32_t)(8 - n) << 27); acc = 0; }
};

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------
constexpr int TPB = 256;
constexpr int TILE_BLOCKS = TPB;                                                  // blocks of an interval coded at once, one per lane
constexpr int W_WORDS = (TILE_BLOCKS * JPEG_BLOCK_MAX_BITS + 31) / 32 + 2;        // a tile at its worst, the bits carried in, a guard word

__global__ __launch_bounds__(TPB) void jpeg_transform_kernel(const uint8_t* __restrict__ img, int64_t stride, int H, int W, int ch, int quality, int64_t row_blocks,
                                                             int64_t nblocks, int16_t* __restrict__ coef) {
  __shared__ uint16_t q[2][64];
  if (threadIdx.x < 128) q[threadIdx.x >> 6][threadIdx.x & 63] = (uint16_t)jpeg_qtable(threadIdx.x >> 6, threadIdx.x & 63, quality);
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (b >= nblocks) return;
  const int64_t row = b / row_blocks, j = b % row_blocks;
  int16_t zz[64];
  jpeg_block(img, stride, H, W, ch, row, j, q[j % ch ? 1 : 0], zz);
  uint32_t* dst = (uint32_t*)(coef + b * 64);
#pragma unroll
  for (int k = 0; k < 32; ++k) dst[k] = (uint32_t)(uint16_t)zz[2 * k] | (uint32_t)(uint16_t)zz[2 * k + 1] << 16;
}

struct EntShared {
  uint32_t W[W_WORDS];
  JpegHuff huff[4];
  int sa[TPB];
};

// nb = coded >> 27 bits, MSB first, at bit position pos of W
__device__ inline void or_bits(uint32_t* W, uint32_t pos, uint32_t coded) {
  const uint32_t v = coded & 0x7ffffff, nb = coded >> 27, w = pos >> 5, s = pos & 31;
  if (!nb) return;
  if (s + nb <= 32) atomicOr(&W[w], v << (32 - s - nb));
  else { atomicOr(&W[w], v >> (s + nb - 32)); atomicOr(&W[w + 1], v << (64 - s - nb)); }
}
__device__ inline uint32_t byte_of(const uint32_t* W, uint32_t k) { return (W[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu; }

// inclusive prefix sum of v over the workgroup's lanes through sa; every lane calls it; returns the lane's inclusive sum, *total the workgroup's
__device__ inline int scan_incl(int* sa, int tid, int v, int* total) {
  sa[tid] = v;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const int a = tid >= d ? sa[tid - d] : 0;
    __syncthreads();
    sa[tid] += a;
    __syncthreads();
  }
  const int mine = sa[tid];
  *total = sa[TPB - 1];
  __syncthreads();
  return mine;
}

__global__ __launch_bounds__(TPB) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int ch, int64_t row_blocks, int64_t rows, uint8_t* __restrict__ slots, int64_t slot,
                                                           int64_t* __restrict__ sizes) {
  __shared__ EntShared sh;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int16_t* src = coef + row * row_blocks * 64;
  uint8_t* dst = slots + row * slot;
  if (tid < 4 && (ch == 3 || !(tid & 1))) jpeg_huff_build(tid, &sh.huff[tid]);
  for (int k = tid; k < W_WORDS; k += TPB) sh.W[k] = 0;
  __syncthreads();
  uint32_t cur_bits = 0;          // bits (< 8) that stand at the top of W[0]; uniform over the lanes, as bytes_out
  int64_t bytes_out = 0;
  for (int64_t base = 0; base < row_blocks; base += TILE_BLOCKS) {
    const int64_t b = base + tid;
    const bool have = b < row_blocks, final = base + TILE_BLOCKS >= row_blocks;
    const int16_t* zz = src + b * 64;
    const int t = have && b % ch ? 1 : 0;
    const int pred = have && b >= ch ? zz[-64 * ch] : 0;
    int mine = 0, total;
    if (have) jpeg_block_symbols(zz, pred, sh.huff[t], sh.huff[2 + t], [&](uint32_t c) { mine += (int)(c >> 27); });
    uint32_t pos = cur_bits + (uint32_t)(scan_incl(sh.sa, tid, mine, &total) - mine);
    if (have) jpeg_block_symbols(zz, pred, sh.huff[t], sh.huff[2 + t], [&](uint32_t c) { or_bits(sh.W, pos, c); pos += c >> 27; });
    uint32_t tb = cur_bits + (uint32_t)total;
    if (final && (tb & 7)) {      // the interval's last byte is filled with 1-bits
      const uint32_t fill = 8 - (tb & 7);
      if (tid == 0) or_bits(sh.W, tb, ((1u << fill) - 1) | fill << 27);
      tb += fill;
    }
    __syncthreads();
    // the tile's whole bytes, stuffed, into the slot: each lane a stretch
    const uint32_t nbytes = tb >> 3, per = (nbytes + TPB - 1) / TPB, lo = min((uint32_t)tid * per, nbytes), hi = min(lo + per, nbytes);
    int ff = 0, total_ff;
    for (uint32_t k = lo; k < hi; ++k) ff += byte_of(sh.W, k) == 0xffu;
    const uint32_t part = sh.W[nbytes >> 2] & (0xffu << (24 - 8 * (nbytes & 3)));      // the bits behind them (zeros where nothing was written)
    int64_t o = bytes_out + lo + (scan_incl(sh.sa, tid, ff, &total_ff) - ff);
    for (uint32_t k = lo; k < hi; ++k) {
      const uint32_t v = byte_of(sh.W, k);
      dst[o++] = (uint8_t)v;
      if (v == 0xffu) dst[o++] = 0;
    }
    bytes_out += (int64_t)nbytes + total_ff;
    __syncthreads();
    for (uint32_t k = tid; k <= (tb >> 5) + 1; k += TPB) sh.W[k] = 0;
    __syncthreads();
    if (tid == 0) sh.W[0] = part << (8 * (nbytes & 3));
    __syncthreads();
    cur_bits = tb & 7;
  }
  if (tid == 0) {
    if (row + 1 < rows) { dst[bytes_out] = 0xff; dst[bytes_out + 1] = (uint8_t)(0xd0 + (row & 7)); bytes_out += 2; }
    sizes[row] = bytes_out;
  }
}

__global__ __launch_bounds__(TPB) void jpeg_finish_kernel(const int64_t* __restrict__ sizes, int64_t rows, int H, int W, int ch, int quality, int64_t* __restrict__ offs,
                                                          uint8_t* __restrict__ out, int64_t* __restrict__ size_dev) {
  __shared__ int64_t sc[TPB];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  for (int64_t base = 0; base < rows; base += TPB) {
    const int64_t i = base + tid;
    const int64_t mine = i < rows ? sizes[i] : 0;
    sc[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
      const int64_t a = tid >= d ? sc[tid - d] : 0;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    if (i < rows) offs[i] = carry + sc[tid] - mine;
    carry += sc[TPB - 1];
    __syncthreads();
  }
  if (tid == 0) {
    const int head = jpeg_header(out, H, W, ch, quality);
    out[head + carry] = 0xff; out[head + carry + 1] = 0xd9;
    *size_dev = head + carry + 2;
  }
}

__global__ __launch_bounds__(TPB) void jpeg_copy_kernel(const uint8_t* __restrict__ slots, int64_t slot, const int64_t* __restrict__ sizes, const int64_t* __restrict__ offs, int head,
                                                        uint8_t* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int64_t size = sizes[row];
  const uint8_t* src = slots + row * slot;
  uint8_t* dst = out + head + offs[row];
  for (int64_t k = (int64_t)blockIdx.y * TPB + threadIdx.x; k < size; k += (int64_t)gridDim.y * TPB) dst[k] = src[k];
}

int jpeg_check(const char* fn, const void* img, int64_t row_stride, int H, int W, int channels, int quality, const void* out, int64_t capacity, const void* size) {
  PNRF_REQUIRE(img && out && size, PNRF_E_ARG, "%s: null pointer", fn);
  PNRF_REQUIRE(H >= 1 && W >= 1 && H <= JPEG_MAX_SIDE && W <= JPEG_MAX_SIDE, PNRF_E_ARG, "%s: image of %d x %d pixels (each side 1 .. 65535)", fn, H, W);
  PNRF_REQUIRE(channels == 1 || channels == 3, PNRF_E_ARG, "%s: %d channels, need 1 or 3", fn, channels);
  PNRF_REQUIRE(quality >= 1 && quality <= 100, PNRF_E_ARG, "%s: quality %d outside 1 .. 100", fn, quality);
  PNRF_REQUIRE(row_stride >= (int64_t)W * channels, PNRF_E_ARG, "%s: row stride of %lld bytes below the row's %lld", fn, (long long)row_stride, (long long)W * channels);
  PNRF_REQUIRE(capacity >= jpeg_max_file_bytes(H, W, channels), PNRF_E_ARG, "%s: room for %lld bytes, pnrf_jpeg_max_bytes is %lld", fn, (long long)capacity,
               (long long)jpeg_max_file_bytes(H, W, channels));
  return 0;
}

}  // namespace
}  // namespace pnrf

using namespace pnrf;

extern "C" int64_t pnrf_jpeg_max_bytes(int H, int W, int channels) { return jpeg_shape_ok(H, W, channels) ? jpeg_max_file_bytes(H, W, channels) : 0; }

extern "C" int64_t pnrf_jpeg_workspace_bytes(int H, int W, int channels) { return jpeg_shape_ok(H, W, channels) ? jpeg_layout(H, W, channels).total : 0; }

extern "C" int pnrf_jpeg_encode_host(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int quality, uint8_t* out, int64_t capacity, int64_t* size) {
  if (int rc = jpeg_check("pnrf_jpeg_encode_host", img, row_stride, H, W, channels, quality, out, capacity, size)) return rc;
  const int64_t rows = jpeg_mcu_rows(H), row_blocks = jpeg_row_blocks(W, channels);
  uint16_t q[2][64];
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) q[t][k] = (uint16_t)jpeg_qtable(t, k, quality);
  static thread_local JpegHuff huff[4];
  for (int id = 0; id < 4; ++id) jpeg_huff_build(id, &huff[id]);
  std::vector<uint8_t> head((size_t)jpeg_header_bytes(channels)), seg;
  std::vector<int16_t> zz((size_t)row_blocks * 64);
  int64_t at = jpeg_header(head.data(), H, W, channels, quality);
  if (at != (int64_t)head.size()) { set_error("pnrf_jpeg_encode_host: header of %lld bytes, expected %lld", (long long)at, (long long)head.size()); return PNRF_E_STATE; }
  memcpy(out, head.data(), head.size());
  for (int64_t row = 0; row < rows; ++row) {
    for (int64_t j = 0; j < row_blocks; ++j) jpeg_block(img, row_stride, H, W, channels, row, j, q[j % channels ? 1 : 0], &zz[(size_t)j * 64]);
    seg.clear();
    HostBits w{seg};
    for (int64_t j = 0; j < row_blocks; ++j) {
      const int t = j % channels ? 1 : 0;
      const int pred = j >= channels ? zz[(size_t)(j - channels) * 64] : 0;
      jpeg_block_symbols(&zz[(size_t)j * 64], pred, huff[t], huff[2 + t], [&](uint32_t c) { w.put(c); });
    }
    w.fill();
    if (row + 1 < rows) { seg.push_back(0xff); seg.push_back((uint8_t)(0xd0 + (row & 7))); }
    if ((int64_t)seg.size() > jpeg_interval_max_bytes(W, channels) || at + (int64_t)seg.size() + 2 > capacity) {
      set_error("pnrf_jpeg_encode_host: interval %lld leaves the bound", (long long)row);
      return PNRF_E_STATE;
    }
    memcpy(out + at, seg.data(), seg.size());
    at += (int64_t)seg.size();
  }
  out[at] = 0xff; out[at + 1] = 0xd9;
  *size = at + 2;
  return 0;
}

extern "C" int pnrf_jpeg_encode_fwd(const uint8_t* img, int64_t row_stride, int H, int W, int channels, int quality, uint8_t* out, int64_t capacity, int64_t* size_dev,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = jpeg_check("pnrf_jpeg_encode_fwd", img, row_stride, H, W, channels, quality, out, capacity, size_dev)) return rc;
  const JpegLayout L = jpeg_layout(H, W, channels);
  PNRF_REQUIRE(workspace && workspace_bytes >= L.total && ((uintptr_t)workspace & 15) == 0, PNRF_E_ARG,
               "pnrf_jpeg_encode_fwd: workspace of %lld bytes (16-byte aligned) needed, got %lld at %p", (long long)L.total, (long long)workspace_bytes, workspace);
  PNRF_REQUIRE(((uintptr_t)size_dev & 7) == 0, PNRF_E_ARG, "pnrf_jpeg_encode_fwd: size_dev not 8-byte aligned");
  uint8_t* ws = (uint8_t*)workspace;
  int16_t* coef = (int16_t*)(ws + L.coef);
  uint8_t* slots = ws + L.slots;
  int64_t *sizes = (int64_t*)(ws + L.sizes), *offs = (int64_t*)(ws + L.offs);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblocks = L.rows * L.row_blocks;
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((nblocks + TPB - 1) / TPB)), dim3(TPB), 0, st, img, row_stride, H, W, channels, quality, L.row_blocks, nblocks, coef);
  PNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)L.rows), dim3(TPB), 0, st, (const int16_t*)coef, channels, L.row_blocks, L.rows, slots, L.slot, sizes);
  PNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3(1), dim3(TPB), 0, st, (const int64_t*)sizes, L.rows, H, W, channels, quality, offs, out, size_dev);
  PNRF_LAUNCH_CHECK();
  const unsigned split = L.slot >= 8 * 4096 ? 8u : (unsigned)((L.slot + 4095) / 4096);      // workgroups per slot
  hipLaunchKernelGGL(jpeg_copy_kernel, dim3((unsigned)L.rows, split), dim3(TPB), 0, st, (const uint8_t*)slots, L.slot, (const int64_t*)sizes, (const int64_t*)offs,
                     jpeg_header_bytes(channels), out);
  PNRF_LAUNCH_CHECK();
  return 0;
}
