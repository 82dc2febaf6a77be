// jpeg_host_check.cpp — the JPEG encoder's host twin as a stand-alone program, for a sanitized build (tests/test_jpeg_cpu.py compiles it together with
// pronerf_amd/csrc/pnrf_jpeg.hip and pnrf_pack.hip under -fsanitize=address,undefined and runs it; no device is touched).
//  * the shapes of the tests' case list (1 x 1, 7 x 9, 8 x 8, 9 x 17, 72 x 16, 8 x 2056, 16 x 24, 24 x 32, 64 x 64, 21 x 33, 189 x 252), gray and RGB,
//    noise, a constant, 0 / 255 blocks and a ramp at quality 1, 50, 90 and 100, through pnrf_jpeg_encode_host into heap buffers of exactly
//    pnrf_jpeg_max_bytes, from images of exactly H x stride bytes: the sanitizer sees any byte read or written outside them;
//  * the file's frame: SOI, the header's length, EOI, the size against the bound; a second call gives the same bytes;
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
      fprintf(stderr, "jpeg_host_check: FAILED ");    \
      fprintf(stderr, __VA_ARGS__);                   \
      fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
      return 1;                                       \
    }                                                 \
  } while (0)

// kind 0: noise, 1: a constant, 2: smooth ramp, 3: 0 / 255 in cells 8 wide and 12 tall
static int one(int H, int W, int ch, int pad, int kind, int quality, int* count) {
  const int64_t stride = (int64_t)W * ch + pad;
  std::vector<uint8_t> img((size_t)(H * stride));
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < stride; ++x) {
      uint8_t v = 77;
      if (kind == 0) v = (uint8_t)rnd();
      else if (kind == 2) v = (uint8_t)(x * 3 + y * 5);
      else if (kind == 3) v = ((y / 12 + x / ch / 8) & 1) ? 255 : 0;
      img[(size_t)(y * stride + x)] = x < W * ch ? v : 0xa5;
    }
  const int64_t cap = pnrf_jpeg_max_bytes(H, W, ch);
  CHECK(cap > 0, "%d x %d x %d: no bound", H, W, ch);
  std::vector<uint8_t> a((size_t)cap, 0x5a), b((size_t)cap, 0x5a);
  int64_t na = -1, nb = -1;
  CHECK(pnrf_jpeg_encode_host(img.data(), stride, H, W, ch, quality, a.data(), cap - 1, &na) == PNRF_E_ARG && na == -1 && a[0] == 0x5a, "short buffer taken");
  CHECK(pnrf_jpeg_encode_host(img.data(), stride, H, W, ch, quality, a.data(), cap, &na) == 0, "%s", pnrf_last_error());
  CHECK(pnrf_jpeg_encode_host(img.data(), stride, H, W, ch, quality, b.data(), cap, &nb) == 0, "%s", pnrf_last_error());
  const int head = ch == 1 ? 330 : 613;
  CHECK(na == nb && na <= cap && na > head + 2 && memcmp(a.data(), b.data(), (size_t)na) == 0, "%d x %d x %d kind %d quality %d: sizes %lld, %lld of %lld", H, W, ch, kind, quality,
        (long long)na, (long long)nb, (long long)cap);
  CHECK(a[0] == 0xff && a[1] == 0xd8 && a[2] == 0xff && a[3] == 0xe0 && memcmp(&a[6], "JFIF", 5) == 0, "SOI / APP0");
  CHECK(a[(size_t)head - 8 - 2 * ch] == 0xff && a[(size_t)head - 7 - 2 * ch] == 0xda && a[(size_t)head - 1] == 0 && a[(size_t)head - 2] == 63, "SOS ends the header of %d bytes", head);
  CHECK(a[(size_t)na - 2] == 0xff && a[(size_t)na - 1] == 0xd9, "EOI");
  ++*count;
  return 0;
}

int main() {
  int count = 0;
  const int shapes[][2] = {{1, 1}, {7, 9}, {8, 8}, {9, 17}, {72, 16}, {8, 2056}, {16, 24}, {24, 32}, {64, 64}, {21, 33}, {189, 252}};
  for (auto& s : shapes)
    for (int ch : {1, 3})
      for (int kind = 0; kind < 4; ++kind)
        for (int quality : {1, 50, 90, 100})
          if (one(s[0], s[1], ch, (kind + quality) % 3 == 0 ? 7 : 0, kind, quality, &count)) return 1;
  printf("%d images encoded\n", count);
  return 0;
}
