// pnrf_philox.h — Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of the training set's
// jitter and noise draws (pnrf_batch.hip), and the map from one of its words to a uniform inside (0, 1).  Host and device: the host entry point
// pnrf_philox4x32_10 runs this very code against the published known answers (tests/test_train_batch_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnrf {

__host__ __device__ static inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// u = (2 (x >> 9) + 1) 2^-24: an odd 24-bit integer scaled by a power of two — exact in fp32, 2^-24 <= u <= 1 - 2^-24.
__host__ __device__ static inline float philox_unit(uint32_t x) { return (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-8f; }

}  // namespace pnrf
