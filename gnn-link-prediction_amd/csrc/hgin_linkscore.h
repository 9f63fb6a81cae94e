// The score arithmetic and launch geometry shared by the full-candidate link kernels: A15 ranking
// (hgin_linkrank.hip) and A16 top-K retrieval (hgin_linktopk.hip).  Both must give a (query row, destination row) pair
// the same bits, so the K order lives here once: blocks of 8 features in ascending order; inside a block lane half h
// supplies features 4 h .. 4 h + 3, so the four MFMAs of a block take the feature pairs (0, 4), (1, 5), (2, 6), (3, 7);
// features past F are zeros on both operands.
#pragma once

#include "hgin_common.h"

namespace hgin {

constexpr int kRankBK = 32;              // features per LDS stage
constexpr int kRankRow = kRankBK + 4;    // LDS row stride in floats: the 16-B reads of 32 rows spread over the banks
constexpr int kRankTile = 128;           // queries per workgroup = destinations per tile
constexpr int kRankTargetBlocks = 512;   // two workgroups per CU on 256 CUs

// four consecutive features k .. k + 3 of a row; features at or past F read as zero, nothing past F is touched
template <bool VEC>
__device__ __forceinline__ float4 ld_k4(const float* __restrict__ row, int k, int F) {
  if constexpr (VEC) {   // F % 4 == 0 and 16-B aligned rows: k < F implies k + 3 < F
    return k < F ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    float4 v;
    v.x = k < F ? row[k] : 0.0f;
    v.y = k + 1 < F ? row[k + 1] : 0.0f;
    v.z = k + 2 < F ? row[k + 2] : 0.0f;
    v.w = k + 3 < F ? row[k + 3] : 0.0f;
    return v;
  }
}

__device__ __forceinline__ int64_t clamp_id(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__device__ __forceinline__ void mfma_k8(f32x16& acc, const float4& a, const float4& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// How a sweep over n_dst destinations is cut for n_query queries: enough contiguous ranges of destination tiles
// (splits) that query blocks x splits reaches kRankTargetBlocks workgroups, never an empty split.
struct SweepPlan {
  int64_t n_qblocks, n_tiles, tiles_per_split, splits;
};
inline SweepPlan sweep_plan(int64_t n_query, int64_t n_dst) {
  SweepPlan p;
  p.n_qblocks = ceil_div(n_query, kRankTile);
  p.n_tiles = ceil_div(n_dst, kRankTile);
  int64_t splits = ceil_div(kRankTargetBlocks, p.n_qblocks);
  if (splits > p.n_tiles) splits = p.n_tiles;
  p.tiles_per_split = ceil_div(p.n_tiles, splits);
  p.splits = ceil_div(p.n_tiles, p.tiles_per_split);
  return p;
}

}  // namespace hgin
