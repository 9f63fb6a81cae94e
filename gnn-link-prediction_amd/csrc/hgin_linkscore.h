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

// A19: the destinations [lo, lo + n) of the graph of source row s: g = src_seg[s] clamped into [0, n_graphs),
// dst_ptr[g] .. dst_ptr[g + 1] kept inside [0, n_dst].
__device__ __forceinline__ void seg_range(const int32_t* __restrict__ src_seg, const int32_t* __restrict__ dst_ptr,
                                          int n_graphs, int64_t s, int64_t n_dst, uint32_t& lo, uint32_t& n) {
  int g = src_seg[s];
  g = g < 0 ? 0 : (g >= n_graphs ? n_graphs - 1 : g);
  int64_t a = dst_ptr[g], b = dst_ptr[g + 1];
  a = a < 0 ? 0 : (a > n_dst ? n_dst : a);
  b = b < a ? a : (b > n_dst ? n_dst : b);
  lo = (uint32_t)a;
  n = (uint32_t)(b - a);
}

// A19: the destination tiles of this workgroup.  Its query columns' non-empty segments span the tiles
// [min lo / 128, ceil(max hi / 128)) (block-wide integer min / max through LDS); split `split` of `splits` takes a
// contiguous slice of them, which may be empty (t_beg >= t_end).  Every thread of the workgroup must call it.
__device__ __forceinline__ void seg_tile_slice(const uint32_t (&lo)[2], const uint32_t (&n)[2], int64_t split,
                                               int64_t splits, int64_t& t_beg, int64_t& t_end) {
  __shared__ int s_lo, s_hi;
  if (threadIdx.x == 0) {
    s_lo = 0x7fffffff;
    s_hi = 0;
  }
  __syncthreads();
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
    if (n[tn] != 0u) {
      atomicMin(&s_lo, (int)lo[tn]);
      atomicMax(&s_hi, (int)(lo[tn] + n[tn]));
    }
  __syncthreads();
  const int64_t lo_all = s_lo, hi_all = s_hi;
  t_beg = t_end = 0;
  if (hi_all <= lo_all) return;   // every segment of the block is empty
  const int64_t tile_lo = lo_all / kRankTile, tile_hi = (hi_all + kRankTile - 1) / kRankTile;
  const int64_t per = (tile_hi - tile_lo + splits - 1) / splits;
  t_beg = tile_lo + split * per;
  t_end = t_beg + per < tile_hi ? t_beg + per : tile_hi;
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
