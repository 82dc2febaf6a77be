// pnrf_scene_impl.h — what the translation units that work on a device-resident scene share (pnrf_scene.hip: pose -> frame; pnrf_batch.hip: ray indices ->
// training batch): the scene object itself and the ONE statement of the camera ranking, so that the neighbour selection of a frame and the rank table of a
// training set cannot drift apart.
#pragma once
#include <stdint.h>

#include <vector>

#include "pnrf_common.h"
#include "pnrf_ieee.h"

struct pnrf_scene {
  int nv, Hf, Wf, format;
  int device;                 // -1 until the first pnrf_scene_set_view / pnrf_scene_set_intrinsics allocates the device arrays
  void* cache;                // [nv,Hf,Wf] texels: float4 (PNRF_SCENE_F32) or uchar4 (PNRF_SCENE_U8), w = 0
  float* poses;               // dev [nv,3,4] camera-to-world; a view's row is written by its ingest kernel (the forward calls need every view set)
  float* K;                   // dev [2,3,3]: K_target, K_ref
  std::vector<uint8_t> have;  // host: view v has been set
  int n_have;
  bool have_K;
};

namespace pnrf {

constexpr int SCENE_TPB = 256;
constexpr int SCENE_MAX_VIEWS = 4096;     // the ranking keeps one distance per view in LDS (16 KiB)

// Stable ascending rank of every view by the distance of its camera centre to (tx, ty, tz): ONE workgroup of SCENE_TPB threads, all of which must call.
//   d[v] = sqrt((dx dx + dy dy) + dz dz), every operation rounded once (render.select_neighbors: numpy's fp32 element-wise ops and its three-term sum);
//   rank by counting over the distances in LDS (sd, SCENE_MAX_VIEWS floats): rank(v) = #{u : d[u] < d[v], or equal and u < v}, a NaN behind every number —
//   the order of a stable ascending sort (np.argsort(kind='stable')).  emit(v, rank) is called once per view by the thread that owns it; the ranks are a
//   permutation of 0 .. nv - 1.  Ends without a barrier: the caller synchronises before it reads what emit wrote.
template <class Emit>
__device__ __forceinline__ void scene_rank_views(const float* __restrict__ poses, int nv, float tx, float ty, float tz, float* sd, Emit emit) {
  const int tid = threadIdx.x;
  for (int v = tid; v < nv; v += SCENE_TPB) {
    const float* p = poses + (int64_t)v * 12;
    const float dx = ieee_sub(tx, p[3]), dy = ieee_sub(ty, p[7]), dz = ieee_sub(tz, p[11]);
    sd[v] = ieee_sqrt(ieee_add(ieee_add(ieee_mul(dx, dx), ieee_mul(dy, dy)), ieee_mul(dz, dz)));
  }
  __syncthreads();
  for (int v = tid; v < nv; v += SCENE_TPB) {
    const float d = sd[v];
    int rank = 0;
    for (int u = 0; u < nv; ++u) {
      const float o = sd[u];
      rank += (o < d || (o == d && u < v) || (d != d && (o == o || u < v))) ? 1 : 0;
    }
    emit(v, rank);
  }
}

}  // namespace pnrf
