// png_host_check.cpp — the PNG encoder's host twin as a stand-alone program, for a sanitized build (tests/test_png_cpu.py compiles it together with
// pronerf_amd/csrc/pnrf_png.hip and pnrf_pack.hip under -fsanitize=address,undefined and runs it; no device is touched).
//  * small shapes (1 x 1 .. 3 x 9, rows around the segment length, runs around 258, noise, zeros), gray and RGB, adaptive and every forced filter,
//    through pnrf_png_encode_host into heap buffers of exactly pnrf_png_max_bytes, from images of exactly H x stride bytes: the sanitizer sees any
//    byte read or written outside them;
//  * the file's frame: signature, chunk lengths, IEND, the size against the bound; a second call gives the same bytes;
//  * one byte short of the bound is refused and nothing is written.
// Exit status 0 and no sanitizer report = pass.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pronerf_hip.h"

static uint32_t g_state = 2463534242u;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 17; g_state ^= g_state << 5; return g_state; }

#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      fprintf(stderr, "png_host_check: FAILED ");     \
      fprintf(stderr, __VA_ARGS__);                   \
      fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
      return 1;                                       \
    }                                                 \
  } while (0)

static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// kind 0: noise, 1: zeros, 2: smooth ramp, 3: runs of one value with lengths around 258
static int one(int H, int W, int ch, int pad, int kind, int filter, int* count) {
  const int64_t stride = (int64_t)W * ch + pad;
  std::vector<uint8_t> img((size_t)(H * stride));
  int run = 0, len = 255;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < stride; ++x) {
      uint8_t v = 0;
      if (kind == 0) v = (uint8_t)rnd();
      else if (kind == 2) v = (uint8_t)(x * 3 + y * 5);
      else if (kind == 3) { v = run < len ? 77 : (uint8_t)(78 + rnd() % 100); if (++run > len) { run = 0; len = 255 + (int)(rnd() % 8); } }
      img[(size_t)(y * stride + x)] = x < W * ch ? v : 0xa5;
    }
  const int64_t cap = pnrf_png_max_bytes(H, W, ch);
  CHECK(cap > 0, "%d x %d x %d: no bound", H, W, ch);
  std::vector<uint8_t> a((size_t)cap), b((size_t)cap, 0x5a);
  int64_t na = -1, nb = -1;
  CHECK(pnrf_png_encode_host(img.data(), stride, H, W, ch, filter, a.data(), cap - 1, &na) == PNRF_E_ARG && na == -1, "short buffer taken");
  CHECK(pnrf_png_encode_host(img.data(), stride, H, W, ch, filter, a.data(), cap, &na) == 0, "%s", pnrf_last_error());
  CHECK(pnrf_png_encode_host(img.data(), stride, H, W, ch, filter, b.data(), cap, &nb) == 0, "%s", pnrf_last_error());
  CHECK(na == nb && na <= cap && na >= 8 + 25 + 12 + 2 + 4 + 12 && memcmp(a.data(), b.data(), (size_t)na) == 0, "%d x %d x %d kind %d filter %d: sizes %lld, %lld of %lld", H, W, ch,
        kind, filter, (long long)na, (long long)nb, (long long)cap);
  CHECK(memcmp(a.data(), "\x89PNG\r\n\x1a\n", 8) == 0 && be32(&a[8]) == 13 && memcmp(&a[12], "IHDR", 4) == 0 && be32(&a[16]) == (uint32_t)W && be32(&a[20]) == (uint32_t)H, "IHDR");
  const uint32_t idat = be32(&a[33]);
  CHECK(memcmp(&a[37], "IDAT", 4) == 0 && (int64_t)idat + 8 + 25 + 12 + 12 == na && memcmp(&a[(size_t)na - 8], "IEND\xae\x42\x60\x82", 8) == 0, "IDAT of %u bytes in a file of %lld", idat,
        (long long)na);
  ++*count;
  return 0;
}

int main() {
  const int S = pnrf_png_segment_rows();
  int count = 0;
  const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 1}, {3, 2}, {3, 3}, {3, 4}, {3, 5}, {3, 6}, {3, 7}, {3, 8}, {3, 9}, {S - 1, 21}, {S, 21}, {S + 1, 21}, {2 * S + 1, 21}, {64, 33}};
  for (auto& s : shapes)
    for (int ch : {1, 3})
      for (int filter = -1; filter <= 4; ++filter)
        for (int kind = 0; kind < 3; ++kind)
          if (one(s[0], s[1], ch, (filter + kind) % 3 == 0 ? 7 : 0, kind, filter, &count)) return 1;
  for (int filter : {-1, 0})
    for (int W : {97, 1031, 4099, 70001})      // runs inside a row, across tiles, and a segment of more than one stored block
      if (one(W > 5000 ? 2 : 40, W, 1, 0, 3, filter, &count) || one(2, W, 3, 0, 0, filter, &count)) return 1;
  printf("%d images encoded\n", count);
  return 0;
}
