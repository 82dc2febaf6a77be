// pnrf_repack.hip — rewrite the weight-dependent sections of a packed net in place, on the device, from weights that live on the device.
// The element rules are those of the host packer (pnrf_pack_rules.h: both sides call the same functions); the tables — which layers a stream has, their
// maps, scales and slots — are built by the host packer's own code (pnrf_pack.hip: repack_prepare) on the first call and kept with the handle.
// One launch for all derived matrices, then one launch per weight stream and per bias table; no host synchronisation, no allocation after the first call.
#include "pnrf_common.h"

namespace pnrf {
namespace {

static_assert(W_HID == 256, "the pass-1 constants are reduced by one 256-thread block, a column per thread");

// grid (blocks of 256 elements, op).  Every op reads the caller's matrices only, so their order does not matter
__global__ __launch_bounds__(256) void repack_derive_kernel(const DeriveOp* __restrict__ ops, PackPtrs P) {
  const DeriveOp op = ops[blockIdx.y];
  if (op.kind == DV_COLMAX || op.kind == DV_OUTMAX) {
    if (blockIdx.x) return;
    __shared__ double v[W_HID];
    const float* A = resolve(P, op.a);
    const int j = threadIdx.x;
    if (op.kind == DV_COLMAX) v[j] = colnorm(A, op.lda, j);
    else {
      double m = 0.0;
      for (int k = 0; k < 8; ++k) m = max_keep(sq_d(A[(size_t)k * op.lda + j]), m);
      v[j] = m;
    }
    __syncthreads();
    if (j == 0) {      // the host's comparison, so that a NaN never wins; the maximum of the others does not depend on the order
      double m = 0.0;
      for (int i = 0; i < W_HID; ++i) m = max_keep(v[i], m);
      *op.dst = op.kind == DV_COLMAX ? p1c_hidden(m) : p1c_out(m);
    }
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < derive_elems(op)) derive_elem(op, P, e);
}

// grid (blocks of 4 fragments, layer of the stream): a thread writes the 16 bytes of one lane of one fragment
__global__ __launch_bounds__(256) void repack_stream_kernel(const PackEntry* __restrict__ entries, const int* __restrict__ maps, PackPtrs P, char* __restrict__ dst) {
  const PackEntry& e = entries[blockIdx.y];
  const int frag = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (frag >= e.frags) return;
  const PackLayer L = entry_layer(e, P, maps);
  PackLane o;
  if (pack_lane(e.kind, L, frag, lane, &o)) *(uint4*)(dst + e.dst_off + (size_t)frag * FRAG_BYTES + lane * 16) = make_uint4(o.w[0], o.w[1], o.w[2], o.w[3]);
}

}  // namespace
}  // namespace pnrf

using namespace pnrf;

extern "C" int pnrf_mlp_repack(pnrf_mlp_t* h, const float* const* W, const float* const* b, const int* in_dim, const int* out_dim, int n_layers, void* stream) {
  PNRF_REQUIRE(h && W && b && in_dim && out_dim, PNRF_E_ARG, "pnrf_mlp_repack: null argument");
  const int rc = repack_prepare(h, W, b, in_dim, out_dim, n_layers);      // every refusal is decided here, on the host, before the first launch
  if (rc) return rc;
  RepackPlan* plan = h->plan;
  hipStream_t st = (hipStream_t)stream;
  if (plan->fresh) {
    for (auto& s : plan->scratch) PNRF_HIP(hipMemsetAsync(s.first, 0, s.second, st));
    plan->fresh = false;
  }
  PackPtrs P{};
  for (int l = 0; l < n_layers; ++l) { P.m[l] = W[l]; P.m[PACK_MAX_LAYERS + l] = b[l]; }
  if (plan->n_ops) {
    repack_derive_kernel<<<dim3((plan->max_elems + 255) / 256, plan->n_ops), 256, 0, st>>>(plan->d_ops, P);
    PNRF_LAUNCH_CHECK();
  }
  for (const RepackJob& j : plan->jobs) {
    repack_stream_kernel<<<dim3((j.max_frags + 3) / 4, j.count), 256, 0, st>>>(plan->d_entries + j.first, plan->d_maps, P, j.dst);
    PNRF_LAUNCH_CHECK();
  }
  return 0;
}
