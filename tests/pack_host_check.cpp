// pack_host_check.cpp — the packer's host half as a stand-alone program, for a sanitized build (tests/test_pack_image_cpu.py compiles it together with
// pronerf_amd/csrc/pnrf_pack.hip under -fsanitize=address,undefined and runs it; no device is touched).
//  * every net shape of tests/pack_cases.py through pnrf_mlp_pack_image (weights from a small generator of this file): the size query equals the bytes
//    written, a guard band behind the buffer stays untouched, the header's checksum is the payload's;
//  * truncated, padded, bit-flipped and count-edited copies of such images into pnrf_mlp_deserialize: every one refused on the host.
// Exit status 0 and no sanitizer report = pass.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pronerf_hip.h"

static uint32_t g_state = 12345u;
static float rnd(float a) {      // uniform in [-a, a)
  g_state = g_state * 1664525u + 1013904223u;
  return a * ((float)(g_state >> 8) / 8388608.f - 1.f);
}

struct Net {
  std::string name;
  int kind;
  std::vector<int> in_dim, out_dim;
  std::vector<std::vector<float>> W, b;
  void add(int in, int out) {
    in_dim.push_back(in); out_dim.push_back(out);
    W.emplace_back((size_t)in * out); b.emplace_back(out);
    for (auto& w : W.back()) w = rnd(0.15f);
    for (auto& x : b.back()) x = rnd(0.1f);
  }
};

// sampler / refine stack: in0 -> depth x 256 -> out, skip connections behind the backbone layers of `skips`
static Net mm_net(const char* name, int kind, int in0, int depth, int out, std::vector<int> skips = {}) {
  Net n; n.name = name; n.kind = kind;
  n.add(in0, 256);
  for (int l = 1; l < depth; ++l) {
    bool sk = false;
    for (int s : skips) sk = sk || s == l - 1;
    n.add(sk ? 256 + in0 : 256, 256);
  }
  n.add(256, out);
  return n;
}
static Net sampler(const char* name, int n_pts, int depth, std::vector<int> skips = {}) { return mm_net(name, PNRF_NET_SAMPLER, 6 * n_pts, depth, 27, skips); }
static Net refine(const char* name, int nb, int depth, std::vector<int> skips = {}) { return mm_net(name, PNRF_NET_REFINE, 48 + 24 * nb, depth, 35, skips); }
static Net nerf(const char* name, int netdepth) {
  Net n; n.name = name; n.kind = PNRF_NET_NERF;
  n.add(63, 256);
  for (int l = 0; l < netdepth - 2; ++l) n.add(256, 256);
  n.add(256 + 27, 4);
  return n;
}
static Net nerfcls() {
  Net n; n.name = "nerfcls"; n.kind = PNRF_NET_NERFCLS;
  n.add(63, 256);
  for (int l = 1; l < 8; ++l) n.add(l == 5 ? 256 + 63 : 256, 256);
  n.add(256, 256); n.add(256, 1); n.add(256 + 27, 128); n.add(128, 3);
  return n;
}

#define CHECK(cond, ...)                             \
  do {                                               \
    if (!(cond)) {                                   \
      fprintf(stderr, "pack_host_check: FAILED ");   \
      fprintf(stderr, __VA_ARGS__);                  \
      fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
      return 1;                                      \
    }                                                \
  } while (0)

static uint64_t fnv1a(const uint8_t* p, size_t n) {
  uint64_t x = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { x ^= p[i]; x *= 1099511628211ull; }
  return x;
}

// byte offsets in the 128-byte engine header (EngineHeader of pnrf_pack.hip)
enum { H_NSLOTS = 44, H_NBIAS = 64, H_N_OUT = 76, H_N_TVALS = 80, H_SKIPS = 84, H_PAYLOAD = 88, H_CHECKSUM = 96, H_NHID = 120, H_NB = 122, H_NPTS = 124, HEADER = 128 };
static const size_t GUARD = 4096;

static int pack(const Net& n, std::vector<uint8_t>* image) {
  const int nl = (int)n.W.size();
  std::vector<const float*> W(nl), b(nl);
  for (int l = 0; l < nl; ++l) { W[l] = n.W[l].data(); b[l] = n.b[l].data(); }
  int64_t size = -1, written = -1;
  CHECK(pnrf_mlp_pack_image(n.kind, W.data(), b.data(), n.in_dim.data(), n.out_dim.data(), nl, nullptr, 0, &size) == 0, "%s: size query: %s", n.name.c_str(), pnrf_last_error());
  CHECK(size > HEADER, "%s: size %lld", n.name.c_str(), (long long)size);
  std::vector<uint8_t> buf((size_t)size + GUARD, 0xa5);
  CHECK(pnrf_mlp_pack_image(n.kind, W.data(), b.data(), n.in_dim.data(), n.out_dim.data(), nl, buf.data(), size - 1, &written) == PNRF_E_ARG, "%s: short buffer taken", n.name.c_str());
  CHECK(buf[0] == 0xa5, "%s: short buffer written", n.name.c_str());
  CHECK(pnrf_mlp_pack_image(n.kind, W.data(), b.data(), n.in_dim.data(), n.out_dim.data(), nl, buf.data(), size, &written) == 0, "%s: %s", n.name.c_str(), pnrf_last_error());
  CHECK(written == size, "%s: size query %lld, written %lld", n.name.c_str(), (long long)size, (long long)written);
  for (size_t i = 0; i < GUARD; ++i) CHECK(buf[(size_t)size + i] == 0xa5, "%s: byte %zu behind the image written", n.name.c_str(), i);
  uint64_t payload, sum;
  memcpy(&payload, &buf[H_PAYLOAD], 8); memcpy(&sum, &buf[H_CHECKSUM], 8);
  CHECK(memcmp(buf.data(), "PNRFENG", 8) == 0 && payload == (uint64_t)size - HEADER, "%s: header (payload %llu of %lld bytes)", n.name.c_str(), (unsigned long long)payload, (long long)size);
  CHECK(sum == fnv1a(&buf[HEADER], (size_t)payload), "%s: checksum", n.name.c_str());
  buf.resize((size_t)size);
  image->swap(buf);
  return 0;
}

static int refused(const std::vector<uint8_t>& img, size_t size, const char* what, int* count) {
  pnrf_mlp_t* h = nullptr;
  const int rc = pnrf_mlp_deserialize(img.data(), (int64_t)size, &h);
  CHECK((rc == PNRF_E_ARG || rc == PNRF_E_STATE) && !h, "damaged image (%s) not refused on the host: rc %d, %s", what, rc, pnrf_last_error());
  ++*count;
  return 0;
}

static int damaged(const std::vector<uint8_t>& img, int* count) {
  const size_t size = img.size();
  for (size_t cut : {(size_t)0, (size_t)127, (size_t)HEADER, size / 2, size - 4, size - 1}) if (refused(img, cut, "truncated", count)) return 1;
  std::vector<uint8_t> x = img;
  x.resize(size + 8, 0);
  if (refused(x, size + 8, "padded", count)) return 1;
  for (size_t at : {(size_t)3, (size_t)9, (size_t)13, (size_t)17, (size_t)21, (size_t)25, (size_t)29, (size_t)33, (size_t)41, (size_t)H_PAYLOAD, (size_t)H_CHECKSUM + 7, (size_t)HEADER, size / 3,
                    size - 1}) {      // one bit, in every part of the header and in the payload
    x = img; x[at] ^= 0x04;
    if (refused(x, size, "bit flip", count)) return 1;
  }
  // counts edited under an intact checksum (the payload is untouched): a section longer or shorter than the kernels index, another shape
  const struct { int at, width, delta; } edits[] = {{H_NSLOTS, 4, 4}, {H_NSLOTS, 4, -4}, {H_NBIAS, 4, 1}, {H_NBIAS, 4, -256}, {H_N_OUT, 4, -1}, {H_N_TVALS, 4, 48}, {H_N_TVALS, 4, -48},
                                                   {H_SKIPS, 4, 1 << 30}, {H_NHID, 2, 1}, {H_NHID, 2, -1}, {H_NB, 2, 1}, {H_NPTS, 2, 1}};
  for (auto& e : edits) {
    x = img;
    int32_t v = 0;
    memcpy(&v, &x[e.at], e.width);
    v += e.delta;
    memcpy(&x[e.at], &v, e.width);
    if (refused(x, size, "count edit", count)) return 1;
  }
  return 0;
}

int main() {
  // the shapes of tests/pack_cases.py
  std::vector<Net> nets = {sampler("fern-sampler", 48, 6), refine("fern-refine", 4, 6), nerf("fern-nerf", 8),
                           sampler("smallest-sampler", 1, 2), refine("smallest-refine", 1, 2), nerf("smallest-nerf", 3),
                           sampler("offfern-sampler", 32, 8), refine("offfern-refine", 3, 8), nerf("offfern-nerf", 5),
                           sampler("skip4-sampler", 48, 6, {4}), refine("skip4-refine", 4, 6, {4}),
                           sampler("skip02-sampler", 5, 4, {0, 2}), refine("skip02-refine", 5, 4, {0, 2}),
                           sampler("deepest-sampler", 48, 32), refine("deepest-refine", 8, 32)};
  static const char* nb_names[] = {"nb2-refine", "nb3-refine", "nb4-refine", "nb5-refine", "nb6-refine", "nb7-refine", "nb8-refine"};
  for (int nb = 2; nb <= 8; ++nb) nets.push_back(refine(nb_names[nb - 2], nb, 2));
  nets.push_back(nerfcls());
  int n_refused = 0;
  for (const Net& n : nets) {
    std::vector<uint8_t> img;
    if (pack(n, &img)) return 1;
    const bool small = n.name.find("smallest") == 0 || n.name.find("skip02") == 0 || n.name == "nerfcls" || n.name == "nb5-refine";      // every net kind, with and without skips
    if (small && damaged(img, &n_refused)) return 1;
    printf("%-18s %9zu bytes\n", n.name.c_str(), img.size());
  }
  printf("%zu images packed, all damaged images refused (%d)\n", nets.size(), n_refused);
  return 0;
}
