// pnrf_pack.hip — host side: error state, weight packing into the MFMA weight stream.
// A net is packed on the host into an ENGINE IMAGE (header + the buffers of a handle in file order: pnrf_mlp_pack_image); pnrf_mlp_pack uploads
// that image the way pnrf_mlp_deserialize uploads one read from a file.
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include "pnrf_common.h"
#include "pnrf_pack_rules.h"

namespace pnrf {

static thread_local std::string g_err = "";

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

// ---- engine images ----------------------------------------------------------------------------------------------------
// One packed network as one flat byte image: a 128-byte header followed by the device buffers of the handle in a fixed order.
// This is what the reference keeps in its serialized TensorRT engines (pronerf/cli.py:105-157 builds them, trt_infer_v2.py
// deserializes them at start-up); here the "engine" is the pre-tiled weight stream, so the file is the stream.  Like a TensorRT
// plan it is only valid for the library build that wrote it: the header carries the ABI version and a tag of the stream layout.
#ifndef PNRF_LAYOUT_TAG
#define PNRF_LAYOUT_TAG 0u
#endif

struct EngineHeader {
  char magic[8];                 // "PNRFENG\0"
  uint32_t format, abi, layout_tag, slot_bytes;
  int32_t net, prec, in_dim, in_dim_x, out_dim;
  uint32_t nslots, nslots_fold, nslots_h16, nslots_b16;
  int32_t nbias_b16, nbias, n_in0, n_inx, n_out, n_tvals;
  uint32_t skips;                     // format 6: skip mask of a sampler / refine net (these four bytes were alignment padding, zero, in older formats)
  uint64_t payload_bytes, checksum;   // FNV-1a 64 of the payload
  uint32_t nslots_p1;                 // format 2: pass-1 stream of the two-pass sampler, its bias table and error-model constants
  int32_t nbias_p1, n_p1c;
  uint32_t nslots_f16;                // format 3: fp16-operand stream of the refine / NeRF stages
  uint16_t nhid, nb, npts;            // format 4: the net's free shape parameters (hidden layers behind layer 0, neighbour views, ray points)
  uint8_t reserved[2];
};
static constexpr uint32_t ENGINE_FORMAT = 6;      // 6: sampler / refine handles carry their skip mask (mmnetskips); 5: refine handles carry the 16x16x32 stream
static_assert(sizeof(EngineHeader) == 128, "engine header is 128 bytes");
static const char ENGINE_MAGIC[8] = {'P', 'N', 'R', 'F', 'E', 'N', 'G', 0};

// THE table of a handle's buffers = the sections of an image, in file order: X(device pointer in pnrf_mlp, its count — a field of that name in
// pnrf_mlp and in EngineHeader —, bytes per element).  Upload, free, serialize, deserialize and the header <-> handle copies all expand it.
#define PNRF_SECTIONS(X)                                                                                                               \
  X(d_blob, nslots, SLOT_BYTES) X(d_blob_fold, nslots_fold, SLOT_BYTES) X(d_blob_h16, nslots_h16, SLOT_BYTES) X(d_blob_b16, nslots_b16, SLOT_BYTES) \
  X(d_bias_b16, nbias_b16, 4) X(d_bias, nbias, 4) X(d_in0, n_in0, 4) X(d_inx, n_inx, 4) X(d_out, n_out, 4) X(d_tvals, n_tvals, 4)                 \
  X(d_blob_p1, nslots_p1, SLOT_BYTES) X(d_bias_p1, nbias_p1, 4) X(d_p1c, n_p1c, 4) X(d_blob_f16, nslots_f16, SLOT_BYTES)
// ... and the scalars that describe the net, under one name in both structs too
#define PNRF_NET_FIELDS(X) X(net) X(prec) X(in_dim) X(in_dim_x) X(out_dim) X(nhid) X(nb) X(npts) X(skips)

#define X(p, n, e) SEC_##p,
enum { PNRF_SECTIONS(X) ENGINE_SECTIONS };
#undef X
static_assert(ENGINE_SECTIONS == 14, "engine format 6 has 14 sections");

struct Section { void** dptr; size_t bytes; };
static void sections(pnrf_mlp* h, Section* s) {
#define X(p, n, e) *s++ = {(void**)&h->p, (size_t)h->n * (e)};
  PNRF_SECTIONS(X)
#undef X
}
static void header_to_handle(const EngineHeader& hd, pnrf_mlp* h) {
#define X(p, n, e) h->n = hd.n;
  PNRF_SECTIONS(X)
#undef X
#define X(f) h->f = hd.f;
  PNRF_NET_FIELDS(X)
#undef X
}
static void handle_to_header(const pnrf_mlp* h, EngineHeader* hd) {
  memset(hd, 0, sizeof(*hd));
  memcpy(hd->magic, ENGINE_MAGIC, 8);
  hd->format = ENGINE_FORMAT; hd->abi = PNRF_ABI_VERSION; hd->layout_tag = PNRF_LAYOUT_TAG; hd->slot_bytes = SLOT_BYTES;
#define X(p, n, e) hd->n = h->n;
  PNRF_SECTIONS(X)
#undef X
#define X(f) hd->f = (decltype(hd->f))h->f;
  PNRF_NET_FIELDS(X)
#undef X
}

// what the packer produces for a net kind (the counts the kernels rely on)
static void expected_counts(int net, int nhid, int nb, int npts, uint32_t skips, pnrf_mlp* w) {
  memset(w, 0, sizeof(*w));
  w->net = net; w->nhid = nhid; w->nb = nb; w->npts = npts; w->skips = skips;
  switch (net) {
    case PNRF_NET_SAMPLER: {
      const bool full = npts == S_NPTS && !skips;
      w->prec = PREC_F32; w->in_dim = 6 * npts; w->out_dim = S_OUT; w->nslots = full ? s_nslots(nhid) : 0; w->nslots_fold = sf_nslots(nhid, skips); w->nslots_h16 = sh_nslots(nhid, skips);
      w->nbias = s_nbias(nhid); w->n_in0 = S_KS0 * 4; w->n_out = 16 * S_NT_LAST; w->n_tvals = full ? S_NPTS : 0;
      w->nslots_p1 = p1_nslots(nhid, skips); w->nbias_p1 = p1_nbias(nhid); w->n_p1c = p1_nconst(nhid);
      break;
    }
    case PNRF_NET_REFINE:
      w->prec = PREC_BF16; w->in_dim = 48 + 24 * nb; w->out_dim = R_OUT; w->nslots = refine_slots(nhid, refine_nv(nb), skips); w->nbias = r_nbias(nhid);
      w->n_in0 = (3 * refine_nv(nb) + 3) * 16; w->n_out = R_NT_LAST * 32;
      if (!skips) { w->nslots_b16 = refine16_slots(nhid, refine16_nv(nb), false); w->nslots_fold = refine16_slots(nhid, refine16_nv(nb), true); w->nbias_b16 = r16_nbias(nhid); }
      w->nslots_f16 = w->nslots;
      break;
    case PNRF_NET_NERF:
      w->prec = PREC_BF16; w->in_dim = N_IN; w->in_dim_x = N_INV; w->out_dim = N_OUT; w->nslots = n_nslots(nhid); w->nslots_b16 = nb_nslots(nhid);
      w->nbias = n_nbias(nhid); w->nbias_b16 = nb_nbias(nhid); w->n_in0 = N_KS0 * 16; w->n_inx = N_KSX * 16; w->n_out = 32;
      w->nslots_f16 = w->nslots_b16;
      break;
    default:      // PNRF_NET_NERFCLS
      w->prec = PREC_BF16; w->in_dim = N_IN; w->in_dim_x = N_INV; w->out_dim = 4; w->nslots = C_NSLOTS; w->nslots_b16 = CB_NSLOTS;
      w->nbias = C_NBIAS; w->nbias_b16 = CB_NBIAS; w->n_in0 = N_KS0 * 16; w->n_inx = N_KSX * 16; w->n_out = 64;
      w->nslots_f16 = CB_NSLOTS;
      break;
  }
}

static uint64_t fnv1a(const uint8_t* p, size_t n) {
  uint64_t x = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { x ^= p[i]; x *= 1099511628211ull; }
  return x;
}

// an image being packed: the header and where each (zero-filled) section lies in the caller's memory
struct Image {
  EngineHeader hd;
  uint8_t* sec[ENGINE_SECTIONS];
  size_t bytes[ENGINE_SECTIONS];
};

// ---- layers and fragments ---------------------------------------------------------------------------------------------
// What an element of a stream IS — roundings, scalings, lane / row / feature indexing — is stated once, in pnrf_pack_rules.h, for this packer and for
// the device repack kernels (pnrf_repack.hip).  Here: which layers a net's streams have, with which maps, at which slots.
struct Layer {
  PackSrc W, b;              // the caller's W[l] / b[l] (by index: a device plan outlives the pointers of one call) or a derived matrix (by address)
  int in_dim, out_dim;
  int nt;                    // output tiles (32x32x16: 32 rows; 16x16x32 and f32: 16 rows)
  int nk;                    // k-steps (32x32x16: 16 features each; 16x16x32: 32 each; f32: 4 each, a multiple of 4)
  std::vector<int> in_map;   // 32x32x16: [nk][2][8]; 16x16x32: [nk][4][8]; f32: [nk][4]   -> input feature or -1
  std::vector<int> out_map;  // [nt][32] or [nt][16]: tile row -> output index or -1
  double wscale = 1.0;       // weights / biases are stored multiplied by these (in double, before the rounding to the stream's type):
  double bscale = 1.0;       // the log2(e) scaling of the ELU nets' streams, see elu_scaled() in pnrf_engine.h
  int x_from = 1 << 30;      // skip layer (mmnetskips): input columns >= x_from are the net input's (first-layer-like) and carry xscale instead of wscale
  double xscale = 1.0;
  int slot_align = 1;        // slots of the layer in a stream are rounded up to a multiple of this (skip layers: NSLOTS, pnrf_layout.h)
  float bpost = 1.f;         // bias table entries times this, in fp32 (pass 1: a skip layer's accumulators run at scale 2^11)
};
static PackSrc src_w(int l, int off = 0) { return PackSrc{nullptr, l, off}; }
static PackSrc src_b(int l) { return PackSrc{nullptr, PACK_MAX_LAYERS + l, 0}; }
static PackSrc src_at(const float* p) { return PackSrc{p, -1, 0}; }
// ELU nets on log2(e)-scaled activations: first layer W, every ELU layer's bias x log2(e); output layer W / log2(e).  The x-columns of a skip layer
// multiply the unscaled net input like the first layer's and get the factor too; its h-columns multiply scaled activations and do not
static void scale_for_elu(std::vector<Layer>& Ls) {
  for (size_t l = 0; l + 1 < Ls.size(); ++l) { Ls[l].bscale = LOG2E_D; Ls[l].xscale = LOG2E_D; }
  Ls.front().wscale = LOG2E_D;
  Ls.back().wscale = 1.0 / LOG2E_D;
}

// slots of a layer that is `frags` fragments long, and of the three fragment orders
static size_t frag_slots(const Layer& L, size_t frags) { const size_t s = (frags + SLOT_FRAGS - 1) / SLOT_FRAGS; return (s + L.slot_align - 1) / L.slot_align * L.slot_align; }
static size_t tile_slots(const Layer& L, int) { return frag_slots(L, (size_t)L.nt * L.nk); }                 // 32x32x16: [tile][k-step]
static size_t f32_slots(const Layer& L, int) { return frag_slots(L, (size_t)L.nt * (L.nk / 4)); }            // 16x16x4: [tile][4 k-steps]
static size_t pair_slots(const Layer& L, int planes) { return frag_slots(L, (size_t)(L.nt / 2) * L.nk * 2 * planes); }      // 16x16x32: paired 16-row tiles
static size_t b16_slots(const Layer& L, int) { return pair_slots(L, 1); }
static size_t h16x2_slots(const Layer& L, int) { return pair_slots(L, 2); }

// Where a net's packed bytes go: into an image in host memory (plan == nullptr: the matrices of P are read here), or — the sections of `img` being a
// handle's device buffers — into the tables of a device plan, which the repack kernels run on whatever matrices a call brings (P is never read)
struct PlanBuild {
  std::vector<PackEntry> entries;
  std::vector<int> maps;
  std::vector<RepackJob> jobs;
  std::vector<DeriveOp> ops;
  RepackPlan* plan;
  hipError_t err = hipSuccess;
};
struct Sink {
  const Image& img;
  PackPtrs P;
  PlanBuild* plan;
  std::vector<std::vector<float>> own;
  // a derived matrix of n floats, zero-filled: host memory, or device scratch owned by the plan
  float* derived(size_t n) {
    if (!plan) { own.emplace_back(n, 0.f); return own.back().data(); }
    void* d = nullptr;
    if (plan->err == hipSuccess) plan->err = hipMalloc(&d, n * sizeof(float));
    if (d) { plan->plan->allocs.push_back(d); plan->plan->scratch.push_back({d, n * sizeof(float)}); }
    return (float*)d;
  }
};
static PackLayer view(const Layer& L, const PackPtrs& P) {
  return PackLayer{resolve(P, L.W), resolve(P, L.b), L.in_map.data(), L.out_map.data(), L.in_dim, L.nt, L.nk, L.x_from, L.wscale, L.bscale, L.xscale, L.bpost};
}
static void pack_layer(const Layer& L, const PackPtrs& P, int kind, char* dst) {
  const PackLayer v = view(L, P);
  const int frags = pack_frags(kind, v);
  for (int f = 0; f < frags; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      PackLane o;
      if (pack_lane(kind, v, f, lane, &o)) memcpy(dst + (size_t)f * FRAG_BYTES + lane * 16, &o, 16);
    }
}
static void plan_layer(PlanBuild& pb, const Layer& L, int kind, size_t dst_off) {
  PackEntry e{L.W, L.b, (int)pb.maps.size(), 0, L.in_dim, L.nt, L.nk, L.x_from, L.wscale, L.bscale, L.xscale, L.bpost, kind, 0, (uint32_t)dst_off};
  pb.maps.insert(pb.maps.end(), L.in_map.begin(), L.in_map.end());
  e.out_map = (int)pb.maps.size();
  pb.maps.insert(pb.maps.end(), L.out_map.begin(), L.out_map.end());
  e.frags = pack_frags(kind, PackLayer{nullptr, nullptr, nullptr, nullptr, L.in_dim, L.nt, L.nk, L.x_from, 1.0, 1.0, 1.0, 1.f});
  RepackJob& j = pb.jobs.back();
  j.count++; j.max_frags = e.frags > j.max_frags ? e.frags : j.max_frags;
  pb.entries.push_back(e);
}
static void run_derive(const DeriveOp& op, const PackPtrs& P);
static void derive(Sink& sk, const DeriveOp& op) { if (sk.plan) sk.plan->ops.push_back(op); else run_derive(op, sk.P); }

// ---- the internal layout checks: whatever is written into a section must be exactly as long as expected_counts() made it ------------------------
// One weight stream: the layers' fragments, each layer at the slot where the one before it ends; the stream ends on a whole turn of the ring
template <class Slots, class Kind>
static int pack_stream(const std::vector<Layer>& Ls, Sink& sk, int s, const char* what, Slots slots_of, Kind kind_of, size_t* used = nullptr) {
  const Image& img = sk.img;
  size_t n = 0;
  for (size_t l = 0; l < Ls.size(); ++l) n += slots_of(Ls[l], (int)l);
  if (used) *used = n;
  PNRF_REQUIRE((size_t)pad_slots((int)n) * SLOT_BYTES == img.bytes[s], PNRF_E_SHAPE, "pnrf_mlp_pack: internal layout mismatch (%s stream: %d slots, kernels expect %zu)", what,
               pad_slots((int)n), img.bytes[s] / SLOT_BYTES);
  char* dst = (char*)img.sec[s];
  if (sk.plan) sk.plan->jobs.push_back(RepackJob{dst, (int)sk.plan->entries.size(), 0, 0});
  size_t off = 0;
  for (size_t l = 0; l < Ls.size(); ++l) {
    if (sk.plan) plan_layer(*sk.plan, Ls[l], kind_of((int)l), off);
    else pack_layer(Ls[l], sk.P, kind_of((int)l), dst + off);
    off += slots_of(Ls[l], (int)l) * SLOT_BYTES;
  }
  return 0;
}
static int pack_biases(const std::vector<Layer>& Ls, bool rows16, Sink& sk, int s, const char* what) {
  const Image& img = sk.img;
  const int rows = rows16 ? 16 : 32;
  size_t n = 0;
  for (auto& L : Ls) n += (size_t)L.nt * rows;
  PNRF_REQUIRE(n * sizeof(float) == img.bytes[s], PNRF_E_SHAPE, "pnrf_mlp_pack: internal layout mismatch (%s bias table: %zu floats, kernels expect %zu)", what, n, img.bytes[s] / sizeof(float));
  char* dst = (char*)img.sec[s];
  if (sk.plan) sk.plan->jobs.push_back(RepackJob{dst, (int)sk.plan->entries.size(), 0, 0});
  size_t off = 0;
  for (auto& L : Ls) {
    if (sk.plan) plan_layer(*sk.plan, L, rows16 ? PK_BIAS16 : PK_BIAS32, off);
    else pack_layer(L, sk.P, rows16 ? PK_BIAS16 : PK_BIAS32, dst + off);
    off += (size_t)L.nt * rows * sizeof(float);
  }
  return 0;
}
// the weight-independent sections: written into an image, left alone in a handle that is repacked
static int put_map(const std::vector<int>& m, Sink& sk, int s, const char* what) {
  const Image& img = sk.img;
  PNRF_REQUIRE(m.size() * sizeof(int) == img.bytes[s], PNRF_E_SHAPE, "pnrf_mlp_pack: internal layout mismatch (%s map: %zu entries, kernels expect %zu)", what, m.size(), img.bytes[s] / sizeof(int));
  if (!m.empty() && !sk.plan) memcpy(img.sec[s], m.data(), img.bytes[s]);
  return 0;
}
#define PNRF_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// ---- map builders -----------------------------------------------------------------------------------------------------
// The three engine geometries: lane groups that share a k-step, features per lane and k-step, rows of an output tile, k-steps of a hidden layer and
// which hidden unit (ks, group, j) is
struct Geom { int groups, per, tile_rows, ks_hid; int (*hidden)(int, int, int); };
static int hidden_f32(int kk, int q, int) { return hidden_feat_f32(kk, q); }
static int hidden_32(int ks, int h, int j) { return hidden_feat_bf16(ks, h, j); }
static int hidden_16(int ks, int g, int j) { return hidden_feat_h16(ks, g, j); }
static const Geom G32 = {2, 8, 32, KS_HID, hidden_32};          // v_mfma 32x32x16, bf16 / fp16
static const Geom G16 = {4, 8, 16, NB_KS_H, hidden_16};         // v_mfma 16x16x32, bf16 / fp16 / split fp16, 16-row tiles in pairs
static const Geom GF32 = {4, 1, 16, W_HID / 4, hidden_f32};     // v_mfma 16x16x4 f32

// nk more k-steps from a feature function feat(ks, group, j) -> input column or -1; `add` shifts the valid columns (the x- or view columns behind 256 h-columns)
template <class F>
static void append_ksteps(std::vector<int>& m, const Geom& G, int nk, F feat, int add = 0) {
  for (int ks = 0; ks < nk; ++ks)
    for (int g = 0; g < G.groups; ++g)
      for (int j = 0; j < G.per; ++j) {
        const int v = feat(ks, g, j);
        m.push_back(v >= 0 ? v + add : -1);
      }
}
template <class F>
static void add_ksteps(Layer& L, const Geom& G, int nk, F feat, int add = 0) { append_ksteps(L.in_map, G, nk, feat, add); L.nk += nk; }
template <class F>
static void set_ksteps(Layer& L, const Geom& G, int nk, F feat, int add = 0) { L.in_map.clear(); L.nk = 0; add_ksteps(L, G, nk, feat, add); }
static void hidden_inputs(Layer& L, const Geom& G, int add = 0) { set_ksteps(L, G, G.ks_hid, G.hidden, add); }
static std::vector<int> identity_out(int rows) {
  std::vector<int> m(rows);
  for (int i = 0; i < rows; ++i) m[i] = i;
  return m;
}
static void hidden_layer(Layer& L, const Geom& G) { hidden_inputs(L, G); L.nt = W_HID / G.tile_rows; L.out_map = identity_out(W_HID); }
// out_map of the first `n` network outputs in the first rows of `nt` tiles
static void first_rows_out(Layer& L, const Geom& G, int nt, int n) {
  L.nt = nt; L.out_map.assign((size_t)nt * G.tile_rows, -1);
  for (int i = 0; i < n; ++i) L.out_map[i] = i;
}
// module-level store map of a 32-row-tile last layer: (tile, half, reg) -> output index
static std::vector<int> half_order(const Layer& Z) {
  std::vector<int> m(Z.nt * 32);
  for (int to = 0; to < Z.nt; ++to) for (int h = 0; h < 2; ++h) for (int g = 0; g < 16; ++g) m[(to * 2 + h) * 16 + g] = Z.out_map[to * 32 + acc_row(g, h)];
  return m;
}
// ---- derived matrices: the ops (DeriveKind, pnrf_pack_rules.h), and their host execution ----------------------------------------------------------
static DeriveOp copy_op(float* dst, int ldd, PackSrc a, int lda, int rows, int cols) { return DeriveOp{DV_COPY, rows, cols, 0, dst, ldd, a, a, a, lda}; }
// fold n column groups of width 6 into one: dst[r][j] = sum_p a[r][6 p + j]
static DeriveOp fold6_op(float* dst, int ldd, PackSrc a, int lda, int rows, int n) { return DeriveOp{DV_FOLD6, rows, 6, n, dst, ldd, a, a, a, lda}; }
static void run_derive(const DeriveOp& op, const PackPtrs& P) {
  const float* A = resolve(P, op.a);
  if (op.kind == DV_WC) {                      // derive_elem's sums, k outermost: each element still adds its products in ascending k
    const float* B = resolve(P, op.b);
    std::vector<double> acc(op.cols);
    for (int r = 0; r < op.rows; ++r) {
      for (int c = 0; c < op.cols; ++c) acc[c] = 0.0;
      for (int k = 0; k < W_HID; ++k) {
        const double wv = (double)A[(size_t)r * op.lda + k];
        const float* row = B + (size_t)k * W_HID;
        for (int c = 0; c < op.cols; ++c) acc[c] = mac_d(acc[c], wv, (double)row[c]);
      }
      for (int c = 0; c < op.cols; ++c) op.dst[(size_t)r * op.ldd + c] = (float)acc[c];
    }
  } else if (op.kind == DV_COLMAX) {
    double cmax = 0.0;
    for (int j = 0; j < W_HID; ++j) cmax = max_keep(colnorm(A, op.lda, j), cmax);
    *op.dst = p1c_hidden(cmax);
  } else if (op.kind == DV_OUTMAX) {
    double mmax = 0.0;
    for (int k = 0; k < 8; ++k) for (int j = 0; j < W_HID; ++j) mmax = max_keep(sq_d(A[(size_t)k * op.lda + j]), mmax);
    *op.dst = p1c_out(mmax);
  } else {
    for (int e = 0, n = derive_elems(op); e < n; ++e) derive_elem(op, P, e);
  }
}
// the folded 6-vector as one k-step: group 0 supplies the 6 Pluecker features, the rest is padding (f32: two of four k-steps, one feature per quarter)
static int folded_in(int, int g, int j) { return g == 0 && j < 6 ? j : -1; }
static int folded_in_f32(int kk, int q, int) { return 4 * kk + q < 6 ? 4 * kk + q : -1; }

// ---- the nets -----------------------------------------------------------------------------------------------------------
struct Shape {
  int net, n_layers, nhid, in0, npts, nb;
  uint32_t skips;                          // bit i: Linear i + 1 (hidden layer i of the kernels) reads cat([x, h]) — a skip behind backbone layer i
  bool skip(int l) const { return l >= 1 && l < n_layers - 1 && ((skips >> (l - 1)) & 1u) != 0; }
};
typedef const float* const* Mats;

// Every argument and shape check of pnrf_mlp_pack; fills `s`
static int check_net(int net, Mats W, Mats b, const int* in_dim, const int* out_dim, int n_layers, Shape* s) {
  *s = Shape{net, n_layers, 0, 0, 0, 0, 0u};
  if (net == PNRF_NET_NERFCLS) {
    PNRF_REQUIRE(n_layers == C_NLIN, PNRF_E_SHAPE, "pnrf_mlp_pack: the NeRF class expects %d Linear layers (pts0..7, feature, alpha, views, rgb), got %d", C_NLIN, n_layers);
    const int ei[C_NLIN] = {N_IN, W_HID, W_HID, W_HID, W_HID, W_HID + N_IN, W_HID, W_HID, W_HID, W_HID, W_HID + N_INV, W_HID / 2};
    const int eo[C_NLIN] = {W_HID, W_HID, W_HID, W_HID, W_HID, W_HID, W_HID, W_HID, W_HID, 1, W_HID / 2, 3};
    for (int l = 0; l < C_NLIN; ++l) {
      PNRF_REQUIRE(W[l] && b[l], PNRF_E_ARG, "pnrf_mlp_pack: null weight/bias at layer %d", l);
      PNRF_REQUIRE(in_dim[l] == ei[l] && out_dim[l] == eo[l], PNRF_E_SHAPE, "pnrf_mlp_pack: NeRF-class layer %d is %dx%d, kernels are built for %dx%d",
                   l, out_dim[l], in_dim[l], eo[l], ei[l]);
    }
    s->in0 = N_IN;
    return 0;
  }
  PNRF_REQUIRE(net == PNRF_NET_SAMPLER || net == PNRF_NET_REFINE || net == PNRF_NET_NERF, PNRF_E_ARG,
               "pnrf_mlp_pack: unknown net kind %d", net);
  // Supported shapes (pnrf_layout.h, "free shape parameters"): width 256 and 8 samples per ray are fixed; free are the number of hidden layers
  // (mmnetdepth / netdepth), the sampler's ray points (N_point_ray_enc: input 6 P) and the refine net's neighbour views (num_neighbor: input 48 + 24 nb)
  static const char* SUPPORTED = "supported: hidden width 256, N_samples 8 (sampler 6*P -> D x 256 -> 27, any P >= 1; refine 48 + 24*nb -> D x 256 -> 35, nb = 1..8; "
                                 "DoNeRFTRT 63 -> (netdepth - 1) x 256 -> [256 + 27] -> 4 with 3 <= netdepth <= 8; sampler / refine depth 2 <= D <= 32, skip connections (mmnetskips) behind "
                                 "backbone layers 0 .. D - 2: such a layer has 256 + input width columns; the NeRF class: D = 8, skips = [4])";
  const int nhid = s->nhid = n_layers - 2;
  PNRF_REQUIRE(n_layers >= 3 && nhid <= MAX_NHID, PNRF_E_SHAPE, "pnrf_mlp_pack: net %d with %d Linear layers; %s", net, n_layers, SUPPORTED);
  const int in0 = s->in0 = in_dim[0];
  if (net == PNRF_NET_SAMPLER) {
    s->npts = in0 / 6;
    PNRF_REQUIRE(in0 >= 6 && in0 % 6 == 0, PNRF_E_SHAPE, "pnrf_mlp_pack: sampler input width %d is not 6 * N_point_ray_enc; %s", in0, SUPPORTED);
  } else if (net == PNRF_NET_REFINE) {
    s->nb = (in0 - 48) / 24;
    PNRF_REQUIRE(in0 >= 72 && (in0 - 48) % 24 == 0 && s->nb <= MAX_NB, PNRF_E_SHAPE, "pnrf_mlp_pack: refine input width %d is not 48 + 24 * num_neighbor with 1 <= num_neighbor <= %d; %s",
                 in0, MAX_NB, SUPPORTED);
  } else {
    PNRF_REQUIRE(in0 == N_IN, PNRF_E_SHAPE, "pnrf_mlp_pack: NeRF input width %d, kernels encode 10 positional octaves (63); %s", in0, SUPPORTED);
    // the reference's skip='auto' puts the view encoding at layer 7 D / 8 (run_nerf_helpers.py:1190-1201): the last layer only up to D = 8
    PNRF_REQUIRE(n_layers <= 8, PNRF_E_SHAPE, "pnrf_mlp_pack: DoNeRFTRT with netdepth %d: from 9 layers on skip='auto' feeds the view encoding into a hidden layer; %s", n_layers, SUPPORTED);
  }
  const int outN = net == PNRF_NET_SAMPLER ? S_OUT : net == PNRF_NET_REFINE ? R_OUT : N_OUT;
  const int last_in = net == PNRF_NET_NERF ? W_HID + N_INV : W_HID;
  for (int l = 0; l < n_layers; ++l) {
    int ei = l == 0 ? in0 : (l == n_layers - 1 ? last_in : W_HID);
    const int eo = l == n_layers - 1 ? outN : W_HID;
    PNRF_REQUIRE(W[l] && b[l], PNRF_E_ARG, "pnrf_mlp_pack: null weight/bias at layer %d", l);
    if (net != PNRF_NET_NERF && l >= 1 && l < n_layers - 1 && in_dim[l] == W_HID + in0) { s->skips |= 1u << (l - 1); ei = W_HID + in0; }
    PNRF_REQUIRE(in_dim[l] == ei && out_dim[l] == eo, PNRF_E_SHAPE,
                 "pnrf_mlp_pack: net %d layer %d is %dx%d where %dx%d is needed (or %d input columns for a skip layer, cat([x, h]), behind backbone layers 0 .. D - 2); %s",
                 net, l, out_dim[l], in_dim[l], eo, ei, W_HID + in0, SUPPORTED);
  }
  PNRF_REQUIRE(!(net == PNRF_NET_REFINE && s->skips) || refine_skip_lds(n_layers - 2, 4, refine_nv(s->nb)), PNRF_E_SHAPE,
               "pnrf_mlp_pack: refine net with skip connections (mmnetskips), %d layers and %d neighbour views: its bias table and the parked net input do not fit the LDS beside "
               "the weight ring (at most 31 layers with 7 or 8 views); %s", n_layers - 1, s->nb, SUPPORTED);
  return 0;
}

// The Linear layers of a sampler / refine / DoNeRFTRT stack as hidden layers of geometry G (first and last layer: the caller's).
// Skip layers: W = [h-columns (256) | x-columns], the x-columns as the stream's first layer sees the input — the sampler's P ray points folded into one
// Pluecker 6-vector, the refine net's as they are (kept in Wsk).  The hidden k-steps keep their maps; every stream appends its x k-steps
static void base_layers(Sink& sk, const Shape& s, const int* in_dim, const int* out_dim, const Geom& G, std::vector<Layer>& Ls) {
  const int xw = s.net == PNRF_NET_SAMPLER ? 6 : s.in0;
  Ls.resize(s.n_layers);
  for (int l = 0; l < s.n_layers; ++l) {
    Layer& L = Ls[l];
    L.W = src_w(l); L.b = src_b(l); L.in_dim = in_dim[l]; L.out_dim = out_dim[l];
    hidden_layer(L, G);
    if (!s.skip(l)) continue;
    const int ld = W_HID + xw, ldw = W_HID + s.in0;
    float* M = sk.derived((size_t)W_HID * ld);
    derive(sk, copy_op(M, ld, src_w(l, s.in0), ldw, W_HID, W_HID));
    if (s.net == PNRF_NET_SAMPLER) derive(sk, fold6_op(M + W_HID, ld, src_w(l), ldw, W_HID, s.npts));
    else derive(sk, copy_op(M + W_HID, ld, src_w(l), ldw, W_HID, s.in0));
    L.W = src_at(M); L.in_dim = ld; L.x_from = W_HID; L.slot_align = NSLOTS;
  }
}

static int pack_sampler(const Shape& s, const int* in_dim, const int* out_dim, Sink& sk) {
  const Image& img = sk.img;
  const int n = s.n_layers;
  const bool full_stream = s.npts == S_NPTS && !s.skips;      // the sampler's unfolded stream (module-level forward, SAMPLER_F32_FULL): P = 48, no skips
  std::vector<Layer> Ls;
  base_layers(sk, s, in_dim, out_dim, GF32, Ls);
  set_ksteps(Ls[0], GF32, S_KS0, [&](int kk, int q, int) { return full_stream ? sampler_in0(kk, q) : -1; });
  Layer& Z = Ls[n - 1];
  Z.nt = S_NT_LAST; Z.out_map.assign(16 * S_NT_LAST, -1);
  for (int tt = 0; tt < S_NT_LAST; ++tt) for (int q = 0; q < 4; ++q) for (int r = 0; r < 4; ++r) Z.out_map[tt * 16 + 4 * q + r] = sampler_out(tt, q, r);
  PNRF_TRY(put_map(Ls[0].in_map, sk, SEC_d_in0, "sampler input"));
  PNRF_TRY(put_map(Z.out_map, sk, SEC_d_out, "sampler output"));      // [tile][16 rows]: lane quarter q, reg r -> [tile*16 + 4q + r]
  PNRF_TRY(pack_biases(Ls, true, sk, SEC_d_bias, "sampler"));
  PNRF_REQUIRE(img.bytes[SEC_d_tvals] == (full_stream ? S_NPTS * sizeof(float) : 0), PNRF_E_SHAPE, "pnrf_mlp_pack: internal layout mismatch (ray points)");
  if (full_stream) {
    PNRF_TRY(pack_stream(Ls, sk, SEC_d_blob, "unfolded sampler", f32_slots, [](int) { return PK_F32; }));
    if (!sk.plan) pnrf_linspace(0.f, 1.f, S_NPTS, (float*)img.sec[SEC_d_tvals]);
  } else {
    PNRF_REQUIRE(img.bytes[SEC_d_blob] == 0, PNRF_E_SHAPE, "pnrf_mlp_pack: internal layout mismatch (unfolded stream of a sampler that has none)");
  }

  // every other stream has the folded first layer Wf[256x6] = sum_p W0[:, 6p:6p+6], and the folded input's k-step(s) behind the hidden ones of a skip layer
  float* wfold = sk.derived((size_t)W_HID * 6);
  derive(sk, fold6_op(wfold, 6, src_w(0), s.in0, W_HID, s.npts));
  auto fold_first = [&](std::vector<Layer>& Lx, const Geom& G, int nk, int (*feat)(int, int, int)) {
    Lx[0].W = src_at(wfold); Lx[0].in_dim = 6;
    set_ksteps(Lx[0], G, nk, feat);
    for (int l = 1; l < n - 1; ++l) if (s.skip(l)) add_ksteps(Lx[l], G, nk, feat, W_HID);
  };
  // second stream: exact fp32.  K = 6 padded to 16 = one fragment per tile
  std::vector<Layer> Lf = Ls;
  fold_first(Lf, GF32, 4 * SF_KS4_0, folded_in_f32);
  PNRF_TRY(pack_stream(Lf, sk, SEC_d_blob_fold, "folded sampler", f32_slots, [](int) { return PK_F32; }));

  // third stream: split fp16 (hi / lo*2^11) for layer_h16x2, hidden geometry of the 16x16x32 engine
  std::vector<Layer> Lh = Ls;
  scale_for_elu(Lh);                                         // weights only: this stream's kernel scales the shared bias table itself
  for (auto& L : Lh) hidden_inputs(L, G16);
  fold_first(Lh, G16, 1, folded_in);
  PNRF_TRY(pack_stream(Lh, sk, SEC_d_blob_h16, "split-fp16 sampler", h16x2_slots, [](int) { return PK_H16X2; }));

  // fourth stream = pass 1 of the two-pass scheme (sampler_p1_kernel): plain fp16 on the 32x32x16 engine, folded first layer in
  // split fp16; its own bias table in that engine's [tile][half][16] order, log2(e)-scaled for the ELU layers; and the constants of the
  // per-ray error model (pnrf_layout.h: P1_NCONST) taken from the fp32 weights
  std::vector<Layer> Lp = Ls;
  scale_for_elu(Lp);
  for (auto& L : Lp) hidden_layer(L, G32);
  fold_first(Lp, G32, 1, folded_in);                         // a skip layer's in_map = [16 hidden k-steps | the folded input's k-step]; fragments: PK_F16_SKIP
  Layer& Y = Lp[n - 1];
  Y.nt = 1; Y.out_map.assign(32, -1);
  for (int hh = 0; hh < 2; ++hh) for (int g = 0; g < 16; ++g) Y.out_map[acc_row(g, hh)] = sampler_p1_out(g, hh);
  size_t used = 0;
  PNRF_TRY(pack_stream(Lp, sk, SEC_d_blob_p1, "pass-1 sampler",
                       [&](const Layer& L, int l) { return l == 0 ? (size_t)P1_SLOTS_L0 : s.skip(l) ? (size_t)P1_SLOTS_SKIP : tile_slots(L, l); },
                       [&](int l) { return l == 0 ? PK_L0_F16X2 : s.skip(l) ? PK_F16_SKIP : PK_F16_32; }, &used));
  PNRF_REQUIRE(used == (size_t)p1_slots_used(s.nhid, s.skips) && img.bytes[SEC_d_p1c] == p1_nconst(s.nhid) * sizeof(float), PNRF_E_SHAPE,
               "pnrf_mlp_pack: internal layout mismatch (pass-1 stream uses %zu slots, %zu constants)", used, img.bytes[SEC_d_p1c] / sizeof(float));
  for (int l = 1; l < n - 1; ++l) if (s.skip(l)) Lp[l].bpost = P1_SKIP_SCALE;      // the skip layer's accumulators run at scale 2^11
  PNRF_TRY(pack_biases(Lp, false, sk, SEC_d_bias_p1, "pass-1"));
  float* p1c = (float*)img.sec[SEC_d_p1c];      // [0] output-layer constant, [1 + l] C of hidden layer l (sampler_p1_kernel)
  // C_l = max over input features j of the column norm sum_i W_l[i,j]^2 — of a skip layer over its h-columns only (they lie behind the x-columns in the
  // caller's matrix): the x-part is formed split-accurate like layer 0
  for (int l = 1; l <= s.nhid; ++l)
    derive(sk, DeriveOp{DV_COLMAX, 0, 0, 0, p1c + l, 0, src_w(l, s.skip(l) ? s.in0 : 0), src_w(l), src_w(l), in_dim[l]});
  derive(sk, DeriveOp{DV_OUTMAX, 0, 0, 0, p1c, 0, src_w(n - 1), src_w(n - 1), src_w(n - 1), W_HID});      // depth rows of the output layer
  return 0;
}

static int pack_refine(const Shape& s, const int* in_dim, const int* out_dim, Sink& sk) {
  const int n = s.n_layers, nbv = s.nb, nv = refine_nv(nbv);
  std::vector<Layer> Ls;
  base_layers(sk, s, in_dim, out_dim, G32, Ls);
  scale_for_elu(Ls);          // every refine kernel computes its ELU on the log2(e) scale
  auto in0 = [&](int ks, int h, int j) { return refine_in0_nv(nv, nbv, ks, h, j); };
  set_ksteps(Ls[0], G32, 3 * nv + 3, in0);
  for (int l = 1; l < n - 1; ++l) if (s.skip(l)) add_ksteps(Ls[l], G32, 3 * nv + 3, in0, W_HID);      // per tile: the 16 hidden k-steps, then layer 0's k-steps on the x-columns
  Layer& Z = Ls[n - 1];
  Z.nt = R_NT_LAST; Z.out_map.assign(64, -1);
  for (int h = 0; h < 2; ++h) for (int g = 0; g < 16; ++g) {
    Z.out_map[acc_row(g, h)] = refine_out0(g, h);
    Z.out_map[32 + acc_row(g, h)] = refine_out1(g, h);
  }
  PNRF_TRY(put_map(Ls[0].in_map, sk, SEC_d_in0, "refine input"));
  PNRF_TRY(put_map(half_order(Z), sk, SEC_d_out, "refine output"));
  PNRF_TRY(pack_stream(Ls, sk, SEC_d_blob, "refine bf16", tile_slots, [](int) { return PK_BF16_32; }));      // PNRF_VARIANT_BF16
  PNRF_TRY(pack_stream(Ls, sk, SEC_d_blob_f16, "refine fp16", tile_slots, [](int) { return PK_F16_32; }));   // the same stream with fp16 operands: default of the refine stage
  PNRF_TRY(pack_biases(Ls, false, sk, SEC_d_bias, "refine"));
  if (s.skips) return 0;          // (PNRF_VARIANT_REFINE_16X16 does not take skip nets)

  // the streams of the 16x16x32 engine (layer_e16 / refine16_kernel; fp16 operands, log2(e)-scaled like every refine stream) and their bias table:
  // the full first layer for rows from memory, and for the projecting head the first layer with the eight Pluecker 6-vectors folded into one
  const int nv4 = refine16_nv(nbv), fin = 6 + 24 * nbv;
  float* wfold = sk.derived((size_t)W_HID * fin);
  derive(sk, fold6_op(wfold, fin, src_w(0), s.in0, W_HID, 8));
  derive(sk, copy_op(wfold + 6, fin, src_w(0, 48), s.in0, W_HID, 24 * nbv));
  for (int fold = 0; fold < 2; ++fold) {
    std::vector<Layer> Lr = Ls;
    for (auto& L : Lr) hidden_layer(L, G16);
    if (fold) { Lr[0].W = src_at(wfold); Lr[0].in_dim = fin; }
    set_ksteps(Lr[0], G16, refine16_ks0(nv4, fold != 0), [&](int ks, int g, int j) { return refine16_in0(nv4, nbv, ks, g, j, fold != 0); });
    Layer& Y = Lr[n - 1];
    Y.nt = 2 * R16_NTP_LAST; Y.out_map.assign(16 * Y.nt, -1);
    for (int T = 0; T < Y.nt; ++T) for (int r16 = 0; r16 < 16; ++r16) Y.out_map[T * 16 + r16] = refine16_out(T, r16);
    PNRF_TRY(pack_stream(Lr, sk, fold ? SEC_d_blob_fold : SEC_d_blob_b16, fold ? "refine 16x16 folded" : "refine 16x16", b16_slots, [](int) { return PK_E16; }));
    if (!fold) PNRF_TRY(pack_biases(Lr, true, sk, SEC_d_bias_b16, "refine 16x16"));
  }
  return 0;
}

// the view embedding's one k-step on the 16x16x32 engine
static int nerf16_view_in(int, int g, int j) { return nerf16_inx(g, j); }

static int pack_nerf(const Shape& s, const int* in_dim, const int* out_dim, Sink& sk) {
  const int n = s.n_layers;
  std::vector<Layer> Ls, Lb;
  std::vector<int> inx_map;
  base_layers(sk, s, in_dim, out_dim, G32, Ls);
  Lb = Ls;
  set_ksteps(Ls[0], G32, N_KS0, nerf_in0);
  Layer& Z = Ls[n - 1];
  add_ksteps(Z, G32, N_KSX, nerf_inx, W_HID);      // the view columns behind the 256 h-columns
  append_ksteps(inx_map, G32, N_KSX, nerf_inx);
  Z.nt = 1; Z.out_map.assign(32, -1);
  for (int h = 0; h < 2; ++h) for (int g = 0; g < 16; ++g) Z.out_map[acc_row(g, h)] = nerf_out(g, h);
  PNRF_TRY(put_map(Ls[0].in_map, sk, SEC_d_in0, "NeRF input"));
  PNRF_TRY(put_map(inx_map, sk, SEC_d_inx, "NeRF view input"));
  PNRF_TRY(put_map(half_order(Z), sk, SEC_d_out, "NeRF output"));
  PNRF_TRY(pack_stream(Ls, sk, SEC_d_blob, "NeRF 32x32", tile_slots, [](int) { return PK_BF16_32; }));
  PNRF_TRY(pack_biases(Ls, false, sk, SEC_d_bias, "NeRF 32x32"));
  // second stream for the 16x16x32 engine (layer_b16): 16-row tiles in pairs, 32-deep k-steps; with bf16 and with fp16 operands (the default of the NeRF stage)
  for (auto& L : Lb) hidden_layer(L, G16);
  set_ksteps(Lb[0], G16, NB_KS0, nerf16_in0);
  add_ksteps(Lb[n - 1], G16, 1, nerf16_view_in, W_HID);
  first_rows_out(Lb[n - 1], G16, 2, N_OUT);                             // rows 0..3 of tile 0 = rgb, sigma; tile 1 is padding
  PNRF_TRY(pack_stream(Lb, sk, SEC_d_blob_b16, "NeRF bf16", b16_slots, [](int) { return PK_B16; }));
  PNRF_TRY(pack_stream(Lb, sk, SEC_d_blob_f16, "NeRF fp16", b16_slots, [](int) { return PK_E16; }));
  return pack_biases(Lb, true, sk, SEC_d_bias_b16, "NeRF 16x16");     // [tile][16 rows]
}

// NeRF-class fine net: 12 Linear modules -> 10 engine layers (feature_linear is folded into the views layer, which shares its layer with alpha).
static int pack_nerfcls(const int* in_dim, const int* out_dim, Sink& sk) {
  // E89: views layer with feature_linear folded in (helpers:842-848; see pnrf_layout.h) + alpha as row 128.
  //   rows 0..127: Wc[r, :256] = sum_k Wv[r, k] Wf[k, :]  (fp64), Wc[r, 256:283] = Wv[r, 256:283], bc[r] = bv[r] + sum_k Wv[r, k] bf[k]
  //   row 128    : Wc[128, :256] = Wa, no view inputs, bc[128] = ba
  const int VI = W_HID + N_INV, VO = W_HID / 2;
  float* Wc = sk.derived((size_t)(VO + 1) * VI);
  float* bc = sk.derived(VO + 1);
  derive(sk, DeriveOp{DV_WC, VO, W_HID, 0, Wc, VI, src_w(10), src_w(8), src_b(10), VI});
  derive(sk, DeriveOp{DV_BC, VO, 1, 0, bc, 1, src_w(10), src_b(8), src_b(10), VI});
  derive(sk, copy_op(Wc + W_HID, VI, src_w(10, W_HID), VI, VO, N_INV));
  derive(sk, copy_op(Wc + (size_t)VO * VI, VI, src_w(9), W_HID, 1, W_HID));
  derive(sk, copy_op(bc + VO, 1, src_b(9), 1, 1, 1));
  // the ten engine layers on one geometry: E0..E7 = pts0..7, E89, E10 = rgb (helpers:850)
  auto layers = [&](const Geom& G, int ks0, int (*in0)(int, int, int), int ksx, int (*inx)(int, int, int), int ks10) {
    std::vector<Layer> Ls(10);
    for (int e = 0; e < 10; ++e) {
      const int lin = e < 8 ? e : 11;
      Layer& L = Ls[e];
      L.W = src_w(lin); L.b = src_b(lin); L.in_dim = in_dim[lin]; L.out_dim = out_dim[lin];
      hidden_layer(L, G);
    }
    set_ksteps(Ls[0], G, ks0, in0);               // E0: positional k-steps (same slot order as the DoNeRFTRT first layer)
    hidden_inputs(Ls[5], G, N_IN);                // E5: input = cat[pts(63), h(256)] (helpers:838-839): the hidden k-steps on columns 63.., then the positional k-steps on columns 0..62
    add_ksteps(Ls[5], G, ks0, in0);
    Layer& E89 = Ls[8];
    E89.W = src_at(Wc); E89.b = src_at(bc); E89.in_dim = VI; E89.out_dim = VO + 1;
    add_ksteps(E89, G, ksx, inx, W_HID);
    first_rows_out(E89, G, 5 * 32 / G.tile_rows, VO + 1);      // rows 0..127 = view layer, alpha = output 128 -> the first row of a tile of its own
    set_ksteps(Ls[9], G, ks10, G.hidden);         // 128 inputs
    return Ls;
  };
  std::vector<Layer> Ls = layers(G32, N_KS0, nerf_in0, N_KSX, nerf_inx, C_KS10);
  Ls[9].nt = 1; Ls[9].out_map.assign(32, -1);
  for (int g = 0; g < 3; ++g) Ls[9].out_map[acc_row(g, 0)] = g;
  std::vector<int> inx_map;
  append_ksteps(inx_map, G32, N_KSX, nerf_inx);
  PNRF_TRY(put_map(Ls[0].in_map, sk, SEC_d_in0, "NeRF-class input"));
  PNRF_TRY(put_map(inx_map, sk, SEC_d_inx, "NeRF-class view input"));
  PNRF_TRY(put_map(std::vector<int>(64, -1), sk, SEC_d_out, "NeRF-class output"));      // module-level store map, rgb only (alpha handled by the kernel)
  PNRF_TRY(pack_stream(Ls, sk, SEC_d_blob, "NeRF-class 32x32", tile_slots, [](int) { return PK_BF16_32; }));
  PNRF_TRY(pack_biases(Ls, false, sk, SEC_d_bias, "NeRF-class 32x32"));
  // second stream for the 16x16x32 engine (nerf16_kernel<true>): same ten engine layers, 16-row tiles in pairs, 32-deep k-steps, with bf16 / fp16 operands
  std::vector<Layer> Lb = layers(G16, NB_KS0, nerf16_in0, 1, nerf16_view_in, CB_KS10);
  first_rows_out(Lb[9], G16, 2, 3);
  PNRF_TRY(pack_stream(Lb, sk, SEC_d_blob_b16, "NeRF-class bf16", b16_slots, [](int) { return PK_B16; }));
  PNRF_TRY(pack_stream(Lb, sk, SEC_d_blob_f16, "NeRF-class fp16", b16_slots, [](int) { return PK_E16; }));
  return pack_biases(Lb, true, sk, SEC_d_bias_b16, "NeRF-class 16x16");
}

static PackPtrs ptrs_of(Mats W, Mats b, int n_layers) {
  PackPtrs P{};
  for (int l = 0; l < n_layers && l < PACK_MAX_LAYERS; ++l) { P.m[l] = W[l]; P.m[PACK_MAX_LAYERS + l] = b[l]; }
  return P;
}
static int pack_net(const Shape& s, const int* in_dim, const int* out_dim, Sink& sk) {
  return s.net == PNRF_NET_SAMPLER  ? pack_sampler(s, in_dim, out_dim, sk)
         : s.net == PNRF_NET_REFINE ? pack_refine(s, in_dim, out_dim, sk)
         : s.net == PNRF_NET_NERF   ? pack_nerf(s, in_dim, out_dim, sk)
                                    : pack_nerfcls(in_dim, out_dim, sk);
}

// Checks, then the image: header from expected_counts(), zero-filled sections, the net kind's packer.  own: pack into this vector (pnrf_mlp_pack: no
// checksum, nobody reads it); else the serialize convention on (buf, capacity, size)
static int pack_image(int net, Mats W, Mats b, const int* in_dim, const int* out_dim, int n_layers, std::vector<uint8_t>* own, void* buf, int64_t capacity, int64_t* size) {
  Shape s;
  PNRF_TRY(check_net(net, W, b, in_dim, out_dim, n_layers, &s));
  pnrf_mlp want;
  expected_counts(net, s.nhid, s.nb, s.npts, s.skips, &want);
  Image img;
  handle_to_header(&want, &img.hd);
  Section sec[ENGINE_SECTIONS];
  sections(&want, sec);
  size_t payload = 0;
  for (int i = 0; i < ENGINE_SECTIONS; ++i) payload += img.bytes[i] = sec[i].bytes;
  *size = (int64_t)(sizeof(EngineHeader) + payload);
  if (own) { own->assign((size_t)*size, 0); buf = own->data(); }
  else if (!buf) return 0;                                          // size query
  else {
    PNRF_REQUIRE(capacity >= *size, PNRF_E_ARG, "pnrf_mlp_pack_image: buffer of %lld bytes, need %lld", (long long)capacity, (long long)*size);
    memset(buf, 0, (size_t)*size);
  }
  uint8_t* p = (uint8_t*)buf + sizeof(EngineHeader);
  for (int i = 0; i < ENGINE_SECTIONS; ++i) { img.sec[i] = p; p += img.bytes[i]; }
  Sink sk{img, ptrs_of(W, b, n_layers), nullptr, {}};
  PNRF_TRY(pack_net(s, in_dim, out_dim, sk));
  img.hd.payload_bytes = payload;
  if (!own) img.hd.checksum = fnv1a((const uint8_t*)buf + sizeof(EngineHeader), payload);
  memcpy(buf, &img.hd, sizeof(img.hd));
  return 0;
}

// ---- the device plan of a handle (pnrf_mlp_repack) ----------------------------------------------------------------------------------------------
// The nets' packers above, run with the handle's device buffers as the image's sections: they record the streams' and bias tables' layer tables and the
// derive ops instead of packing; the tables and the scratch of the derived matrices go to the device once.
static void free_plan(RepackPlan* p) {
  if (!p) return;
  for (void* d : p->allocs) (void)hipFree(d);
  delete p;
}
static const char* shape_text(char* buf, size_t n, int net, int nhid, int npts, int nb, uint32_t skips) {
  snprintf(buf, n, "net kind %d, %d hidden layers, %d ray points, %d neighbour views, skip mask %08x", net, nhid, npts, nb, skips);
  return buf;
}
int repack_prepare(pnrf_mlp* h, Mats W, Mats b, const int* in_dim, const int* out_dim, int n_layers) {
  Shape s;
  PNRF_TRY(check_net(h->net, W, b, in_dim, out_dim, n_layers, &s));
  char t0[160], t1[160];
  PNRF_REQUIRE(s.nhid == h->nhid && s.npts == h->npts && s.nb == h->nb && s.skips == h->skips, PNRF_E_SHAPE, "pnrf_mlp_repack: the weights are of another shape (%s) than the handle (%s)",
               shape_text(t0, sizeof(t0), s.net, s.nhid, s.npts, s.nb, s.skips), shape_text(t1, sizeof(t1), h->net, h->nhid, h->npts, h->nb, h->skips));
  int dev = -1;
  PNRF_HIP(hipGetDevice(&dev));
  PNRF_REQUIRE(dev == h->device, PNRF_E_STATE, "pnrf_mlp_repack: the handle lives on device %d, the current device is %d", h->device, dev);
  pnrf_mlp want;
  expected_counts(h->net, s.nhid, s.nb, s.npts, s.skips, &want);
  Image img;
  Section sec[ENGINE_SECTIONS], wsec[ENGINE_SECTIONS];
  sections(h, sec);
  sections(&want, wsec);
  for (int i = 0; i < ENGINE_SECTIONS; ++i) {
    PNRF_REQUIRE(sec[i].bytes == wsec[i].bytes && (sec[i].bytes == 0) == (*sec[i].dptr == nullptr), PNRF_E_STATE, "pnrf_mlp_repack: inconsistent handle (section %d)", i);
    img.sec[i] = (uint8_t*)*sec[i].dptr; img.bytes[i] = sec[i].bytes;
  }
  if (h->plan) return 0;
  RepackPlan* plan = new RepackPlan();
  PlanBuild pb;
  pb.plan = plan;
  Sink sk{img, ptrs_of(W, b, n_layers), &pb, {}};
  int rc = pack_net(s, in_dim, out_dim, sk);
  hipError_t e = pb.err;
  auto up = [&](const void* src, size_t bytes, void** dst) {
    if (rc || e != hipSuccess || !bytes) return;
    e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return;
    plan->allocs.push_back(*dst);
    e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  up(pb.entries.data(), pb.entries.size() * sizeof(PackEntry), (void**)&plan->d_entries);
  up(pb.maps.data(), pb.maps.size() * sizeof(int), (void**)&plan->d_maps);
  up(pb.ops.data(), pb.ops.size() * sizeof(DeriveOp), (void**)&plan->d_ops);
  if (!rc && e != hipSuccess) { set_error("pnrf_mlp_repack: device allocation/copy of the plan failed: %s", hipGetErrorString(e)); rc = (int)e; }
  if (rc) { free_plan(plan); return rc; }
  plan->jobs = pb.jobs;
  plan->n_ops = (int)pb.ops.size();
  for (auto& op : pb.ops) plan->max_elems = derive_elems(op) > plan->max_elems ? derive_elems(op) : plan->max_elems;
  plan->fresh = true;
  h->plan = plan;
  return 0;
}

// A (validated or just packed) image -> a handle on the current device
static int upload(const void* image, const char* who, pnrf_mlp_t** out) {
  EngineHeader hd;
  memcpy(&hd, image, sizeof(hd));
  pnrf_mlp* h = new pnrf_mlp();
  memset(h, 0, sizeof(*h));
  header_to_handle(hd, h);
  Section sec[ENGINE_SECTIONS];
  sections(h, sec);
  const uint8_t* p = (const uint8_t*)image + sizeof(EngineHeader);
  hipError_t e = hipGetDevice(&h->device);
  for (int i = 0; i < ENGINE_SECTIONS && e == hipSuccess; ++i) {
    if (sec[i].bytes) {
      e = hipMalloc(sec[i].dptr, sec[i].bytes);
      if (e == hipSuccess) e = hipMemcpy(*sec[i].dptr, p, sec[i].bytes, hipMemcpyHostToDevice);
    }
    p += sec[i].bytes;
  }
  if (e != hipSuccess) {
    set_error("%s: device allocation/copy failed: %s", who, hipGetErrorString(e));
    pnrf_mlp_free(h);
    return (int)e;
  }
  *out = h;
  return 0;
}

}  // namespace pnrf

using namespace pnrf;

extern "C" int pnrf_abi_version(void) { return PNRF_ABI_VERSION; }
extern "C" const char* pnrf_last_error(void) { return pnrf::g_err.c_str(); }

extern "C" int pnrf_linspace(float start, float end, int n, float* out) {
  PNRF_REQUIRE(out && n >= 1, PNRF_E_ARG, "pnrf_linspace: bad arguments");
  // torch.linspace (CPU, float): step = (end-start)/(n-1); i < n/2 ? start + step*i : end - step*(n-1-i)
  if (n == 1) { out[0] = start; return 0; }
  const float step = (end - start) / (float)(n - 1);
  const int half = n / 2;
  // torch's vectorised kernel evaluates start + step*i / end - step*(n-1-i) with one rounding (FMA)
  for (int i = 0; i < n; ++i) out[i] = i < half ? fmaf(step, (float)i, start) : fmaf(-step, (float)(n - 1 - i), end);
  return 0;
}

extern "C" int pnrf_mlp_pack_image(int net, const float* const* W, const float* const* b, const int* in_dim, const int* out_dim, int n_layers,
                                   void* buf, int64_t capacity, int64_t* size) {
  PNRF_REQUIRE(W && b && in_dim && out_dim && size, PNRF_E_ARG, "pnrf_mlp_pack: null argument");
  return pack_image(net, W, b, in_dim, out_dim, n_layers, nullptr, buf, capacity, size);
}

extern "C" int pnrf_mlp_pack(int net, const float* const* W, const float* const* b, const int* in_dim,
                             const int* out_dim, int n_layers, pnrf_mlp_t** out) {
  PNRF_REQUIRE(W && b && in_dim && out_dim && out, PNRF_E_ARG, "pnrf_mlp_pack: null argument");
  std::vector<uint8_t> image;
  int64_t size = 0;
  PNRF_TRY(pack_image(net, W, b, in_dim, out_dim, n_layers, &image, nullptr, 0, &size));
  return upload(image.data(), "pnrf_mlp_pack", out);
}

extern "C" int pnrf_mlp_free(pnrf_mlp_t* h) {
  if (!h) return 0;
  Section sec[ENGINE_SECTIONS];
  sections(h, sec);
  for (int i = 0; i < ENGINE_SECTIONS; ++i)
    if (*sec[i].dptr) (void)hipFree(*sec[i].dptr);
  free_plan(h->plan);
  delete h;
  return 0;
}

extern "C" int pnrf_mlp_serialize(const pnrf_mlp_t* hc, void* buf, int64_t capacity, int64_t* size) {
  PNRF_REQUIRE(hc && size, PNRF_E_ARG, "pnrf_mlp_serialize: null argument");
  pnrf_mlp* h = const_cast<pnrf_mlp*>(hc);
  Section sec[ENGINE_SECTIONS];
  sections(h, sec);
  size_t payload = 0;
  for (int i = 0; i < ENGINE_SECTIONS; ++i) {
    PNRF_REQUIRE((sec[i].bytes == 0) == (*sec[i].dptr == nullptr), PNRF_E_STATE, "pnrf_mlp_serialize: inconsistent handle (section %d)", i);
    payload += sec[i].bytes;
  }
  *size = (int64_t)(sizeof(EngineHeader) + payload);
  if (!buf) return 0;                                               // size query
  PNRF_REQUIRE(capacity >= *size, PNRF_E_ARG, "pnrf_mlp_serialize: buffer of %lld bytes, need %lld", (long long)capacity, (long long)*size);
  int prev = 0;
  PNRF_HIP(hipGetDevice(&prev));
  PNRF_HIP(hipSetDevice(h->device));
  uint8_t* p = (uint8_t*)buf + sizeof(EngineHeader);
  hipError_t e = hipSuccess;
  for (int i = 0; i < ENGINE_SECTIONS && e == hipSuccess; ++i) {
    if (sec[i].bytes) e = hipMemcpy(p, *sec[i].dptr, sec[i].bytes, hipMemcpyDeviceToHost);
    p += sec[i].bytes;
  }
  (void)hipSetDevice(prev);
  if (e != hipSuccess) { set_error("pnrf_mlp_serialize: device read failed: %s", hipGetErrorString(e)); return (int)e; }
  EngineHeader hd;
  handle_to_header(h, &hd);
  hd.payload_bytes = payload;
  hd.checksum = fnv1a((const uint8_t*)buf + sizeof(EngineHeader), payload);
  memcpy(buf, &hd, sizeof(hd));
  return 0;
}

extern "C" int pnrf_mlp_deserialize(const void* buf, int64_t size, pnrf_mlp_t** out) {
  PNRF_REQUIRE(buf && out, PNRF_E_ARG, "pnrf_mlp_deserialize: null argument");
  PNRF_REQUIRE(size >= (int64_t)sizeof(EngineHeader), PNRF_E_ARG, "pnrf_mlp_deserialize: %lld bytes is shorter than the header", (long long)size);
  EngineHeader hd;
  memcpy(&hd, buf, sizeof(hd));
  PNRF_REQUIRE(memcmp(hd.magic, ENGINE_MAGIC, 8) == 0, PNRF_E_ARG, "pnrf_mlp_deserialize: not an engine file (bad magic)");
  PNRF_REQUIRE(hd.format == ENGINE_FORMAT && hd.abi == PNRF_ABI_VERSION && hd.layout_tag == PNRF_LAYOUT_TAG && hd.slot_bytes == SLOT_BYTES, PNRF_E_STATE,
               "pnrf_mlp_deserialize: engine written by another build (format %u abi %u layout %08x, this library: %u %d %08x); export it again",
               hd.format, hd.abi, hd.layout_tag, ENGINE_FORMAT, PNRF_ABI_VERSION, (unsigned)PNRF_LAYOUT_TAG);
  PNRF_REQUIRE(hd.net == PNRF_NET_SAMPLER || hd.net == PNRF_NET_REFINE || hd.net == PNRF_NET_NERF || hd.net == PNRF_NET_NERFCLS, PNRF_E_ARG,
               "pnrf_mlp_deserialize: unknown net kind %d", hd.net);
  PNRF_REQUIRE(hd.nbias_b16 >= 0 && hd.nbias >= 0 && hd.n_in0 >= 0 && hd.n_inx >= 0 && hd.n_out >= 0 && (hd.n_tvals == 0 || hd.n_tvals == S_NPTS) &&
                   hd.nslots < (1u << 16) && hd.nslots_fold < (1u << 16) && hd.nslots_h16 < (1u << 16) && hd.nslots_b16 < (1u << 16) &&
                   hd.nbias < (1 << 24) && hd.nbias_b16 < (1 << 24) && hd.n_in0 < (1 << 20) && hd.n_inx < (1 << 20) && hd.n_out < (1 << 20) &&
                   hd.nslots_p1 < (1u << 16) && hd.nslots_f16 < (1u << 16) && hd.nbias_p1 >= 0 && hd.nbias_p1 < (1 << 24) && hd.n_p1c >= 0 && hd.n_p1c < (1 << 10),
               PNRF_E_ARG, "pnrf_mlp_deserialize: implausible section counts");
  // section counts the kernels of this net kind index with compile-time constants: an image whose counts differ (a crafted file with a
  // matching non-cryptographic checksum, or a stale one under the same layout tag) would make them read past the buffers
  const bool shape_ok = hd.net == PNRF_NET_NERFCLS ? (hd.nhid == 0 && hd.nb == 0 && hd.npts == 0)
                        : (hd.nhid >= 1 && hd.nhid <= MAX_NHID && (hd.net == PNRF_NET_REFINE ? (hd.nb >= 1 && hd.nb <= MAX_NB) : hd.nb == 0) &&
                           (hd.net == PNRF_NET_SAMPLER ? (hd.npts >= 1 && hd.npts < 4096) : hd.npts == 0));
  PNRF_REQUIRE(shape_ok, PNRF_E_ARG, "pnrf_mlp_deserialize: shape parameters (hidden layers %u, views %u, ray points %u) outside what net kind %d supports",
               hd.nhid, hd.nb, hd.npts, hd.net);
  PNRF_REQUIRE(hd.skips == 0 || ((hd.net == PNRF_NET_SAMPLER || hd.net == PNRF_NET_REFINE) && skip_mask_ok(hd.skips, hd.nhid)), PNRF_E_ARG,
               "pnrf_mlp_deserialize: skip mask %08x outside what net kind %d with %u hidden layers supports", hd.skips, hd.net, hd.nhid);
  pnrf_mlp want;
  expected_counts(hd.net, hd.nhid, hd.nb, hd.npts, hd.skips, &want);
  bool same = hd.prec == want.prec && hd.in_dim == want.in_dim && hd.in_dim_x == want.in_dim_x && hd.out_dim == want.out_dim;
  size_t payload = 0;
#define X(p, n, e) same = same && hd.n == want.n; payload += (size_t)hd.n * (e);
  PNRF_SECTIONS(X)
#undef X
  PNRF_REQUIRE(same, PNRF_E_ARG, "pnrf_mlp_deserialize: section counts do not match what net kind %d is packed as by this build", hd.net);
  PNRF_REQUIRE(payload == hd.payload_bytes && (int64_t)(sizeof(EngineHeader) + payload) == size, PNRF_E_ARG,
               "pnrf_mlp_deserialize: truncated or padded engine (%lld bytes, header describes %lld)", (long long)size, (long long)(sizeof(EngineHeader) + payload));
  PNRF_REQUIRE(fnv1a((const uint8_t*)buf + sizeof(EngineHeader), payload) == hd.checksum, PNRF_E_ARG, "pnrf_mlp_deserialize: checksum mismatch (corrupt engine file)");
  return upload(buf, "pnrf_mlp_deserialize", out);
}

extern "C" int pnrf_mlp_set_variant(pnrf_mlp_t* h, int variant) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_mlp_set_variant: null handle");
  const bool sampler = h->net == PNRF_NET_SAMPLER;
  const bool ok = variant == PNRF_VARIANT_DEFAULT || (sampler && (variant == PNRF_VARIANT_SAMPLER_F32 || variant == PNRF_VARIANT_SAMPLER_F32_FULL || variant == PNRF_VARIANT_SAMPLER_SPLIT)) ||
                  ((h->net == PNRF_NET_NERF || h->net == PNRF_NET_NERFCLS) && variant == PNRF_VARIANT_BF16_32X32) ||
                  (!sampler && variant == PNRF_VARIANT_BF16) || (h->net == PNRF_NET_REFINE && variant == PNRF_VARIANT_REFINE_16X16) || ((h->net == PNRF_NET_NERF || h->net == PNRF_NET_NERFCLS) && variant == PNRF_VARIANT_F16) ||
                  ((h->net == PNRF_NET_NERF || h->net == PNRF_NET_NERFCLS) && variant == PNRF_VARIANT_NERF_4X64);
  PNRF_REQUIRE(ok, PNRF_E_ARG, "pnrf_mlp_set_variant: variant %d does not exist for net kind %d", variant, h->net);
  const bool no_skips = (h->net == PNRF_NET_REFINE && (variant == PNRF_VARIANT_REFINE_16X16 || variant == PNRF_VARIANT_BF16)) || (sampler && variant == PNRF_VARIANT_SAMPLER_F32_FULL);
  PNRF_REQUIRE(!(h->skips && no_skips), PNRF_E_SHAPE, "pnrf_mlp_set_variant: variant %d is not built for nets with skip connections (mmnetskips; this net's mask: %08x); "
               "the default kernels and the sampler's SAMPLER_SPLIT / SAMPLER_F32 variants take them", variant, h->skips);
  h->variant = variant;
  return 0;
}

extern "C" int pnrf_mlp_set_shape(pnrf_mlp_t* h, int shape) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_mlp_set_shape: null handle");
  PNRF_REQUIRE(shape == PNRF_SHAPE_AUTO || shape == PNRF_SHAPE_WIDE || shape == PNRF_SHAPE_NARROW, PNRF_E_ARG,
               "pnrf_mlp_set_shape: PNRF_SHAPE_AUTO (0), _WIDE (8) or _NARROW (4), got %d", shape);
  PNRF_REQUIRE(!(shape == PNRF_SHAPE_WIDE && h->net == PNRF_NET_REFINE && h->skips && !(refine_nv(h->nb) <= 2 && refine_skip_lds(h->nhid, 8, refine_nv(h->nb)))), PNRF_E_SHAPE,
               "pnrf_mlp_set_shape: PNRF_SHAPE_WIDE of the refine stage is not built for this net with skip connections (mmnetskips; %d neighbour views, %d hidden layers): its "
               "parked net input fits the LDS of an 8-wave workgroup up to num_neighbor 4 (at 3 or 4 views: up to 18 hidden layers).  PNRF_SHAPE_AUTO launches it NARROW (same rows)", h->nb, h->nhid);
  h->shape = shape;
  return 0;
}

extern "C" int pnrf_mlp_skips(const pnrf_mlp_t* h, uint32_t* mask) {
  PNRF_REQUIRE(h && mask, PNRF_E_ARG, "pnrf_mlp_skips: null argument");
  *mask = h->skips;
  return 0;
}

extern "C" int pnrf_mlp_kind(const pnrf_mlp_t* h, int* net, int* in_dim, int* in_dim_x, int* out_dim) {
  PNRF_REQUIRE(h, PNRF_E_ARG, "pnrf_mlp_kind: null handle");
  if (net) *net = h->net;
  if (in_dim) *in_dim = h->in_dim;
  if (in_dim_x) *in_dim_x = h->in_dim_x;
  if (out_dim) *out_dim = h->out_dim;
  return 0;
}
