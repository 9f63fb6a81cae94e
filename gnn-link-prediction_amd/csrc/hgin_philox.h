// Philox4x32-10 (Salmon et al., SC'11; Random123), the one counter-based generator of libhgin.so: the negative
// samplers (hgin_linkpred.hip, A10 / A13 / A19 / A20), the edge-split rule (hgin_linksplit.hip, A21) and the neighbour
// sampler (hgin_neighbor.hip, A22) evaluate this text, pinned by Random123's published known-answer vectors through
// oracle/hgin_oracle.c.
#pragma once

#include "hgin_common.h"

namespace hgin {

struct U4 {
  uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * ctr.x;
    const uint64_t p1 = (uint64_t)M1 * ctr.z;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    ctr = U4{hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0};
    k0 += W0;
    k1 += W1;
  }
  return ctr;
}

}  // namespace hgin
