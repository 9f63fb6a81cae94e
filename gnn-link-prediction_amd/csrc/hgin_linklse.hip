// A23 — full-candidate softmax link loss: log-sum-exp over every destination and its gradients (include/hgin.h A23).
//
// NOT IN REFERENCE: like A13 .. A22 the spec is build-defined (header include/hgin.h) and checked against a float64
// restatement in tests/test_linklse_host.py.
//
// lse[q] = log sum_{c in cand(q)} exp(score(q, c) * inv_t) over the destinations c that are not known neighbours of
// src[q].  The scores are the A15 / A16 bits (hgin_linkscore.h: K order, ld_k4, mfma_k8, tile constants, sweep_plan);
// no [Q, n_dst] object exists in the forward or in either backward.
//   k_lse_sweep   the A15 sweep (128 gathered queries x 128-destination tiles, 4 waves as 2 x 2, flat (tile, K-stage)
//                 pipeline) with an online log-sum-exp epilogue: per query column a lane keeps a running maximum and a
//                 running sum over the destination rows it holds; folded across the lane half, then across the two wm
//                 waves, then written as one (max, sum) partial per (split, query)
//   k_lse_merge   folds a query's split partials in ascending split order and takes the log
//   k_lse_bwd     recomputes the 128 x 128 block of t = score * inv_t as the sweep does, turns it into
//                 W = g * inv_t * exp(t - lse) in registers (same mask), and passes it through LDS, 32 rows of the swept
//                 side at a time, as operand A of a second MFMA product against those rows' embeddings.  <SRC>: a
//                 workgroup owns 128 queries x 128 output features and sweeps destination tiles (G_src); <DST>: it owns
//                 a destination tile and sweeps the query blocks (G_dst).  F > 128: 256 output features per workgroup;
//                 wider still: one workgroup per chunk of 256, each recomputing t.
//   k_lse_fold    where the stationary side is too short to fill the machine the swept side is split; every split
//                 writes a partial [rows, F] and this kernel adds them in ascending split order
// No float atomics, nothing depends on timing: every output element is written by one thread, every sum has a fixed
// order, so forward and gradients are run-to-run identical.
//
// Known edges are masked inside the sweep, not subtracted afterwards.  A15 can subtract because its counts are integers.
// Here the known neighbours of a source are exactly the high-scoring terms of a trained model: a sum minus its dominant
// terms keeps no digits (and a running maximum taken over them would scale every kept term towards zero).  Each lane
// keeps, per query column, a cursor into its source's sorted known row: opened by a lower-bound search at the first
// tile, advanced over the entries that fall into the current tile, which set bits for those among the 32 destination
// rows the lane holds.  With an average degree of about 6 this is cold code beside the MFMAs.
//
// A24 — the same three calls over graph-local candidates (include/hgin.h A24): cand(q) lies inside A19's segment of
// src[q].  Separate instantiations (SEG) of k_lse_sweep and k_lse_bwd: the query-stationary ones sweep only the tiles
// their block's segments cover (seg_tile_slice), the tile-stationary one skips the query blocks whose covered range
// (k_lse_blk_range) misses its tile.  The unsegmented instantiations keep their launches, traces and bits.
#include <cmath>

#include "hgin_linkscore.h"   // the K order, ld_k4, mfma_k8, the tile constants and the split plan (shared with A15 / A16)

namespace hgin {
namespace {

// output features per backward workgroup: 128 (two 32-column blocks per wave), or 256 (four) once F exceeds 128
inline int lse_feature_chunk(int64_t F) { return F > 128 ? 256 : 128; }
constexpr int64_t kNoKnown = int64_t(1) << 62;

// A lane's view of one source's sorted known row: entries [cur, end) are still ahead, nxt = col[cur] (kNoKnown: none).
struct KnownCursor {
  int cur, end;
  int64_t nxt;
};

// position the cursor at the first known column >= c0
__device__ __forceinline__ void known_open(KnownCursor& k, const int32_t* __restrict__ rowptr,
                                           const int32_t* __restrict__ col, int64_t s, int64_t c0) {
  k.cur = k.end = 0;
  k.nxt = kNoKnown;
  if (rowptr == nullptr) return;
  int lo = rowptr[s], hi = rowptr[s + 1];
  k.end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)col[mid] < c0) lo = mid + 1;
    else hi = mid;
  }
  k.cur = lo;
  k.nxt = lo < k.end ? (int64_t)col[lo] : kNoKnown;
}

// Consume the known columns inside tile [c0, c0 + 128); bit 16 tm + v is set when accumulator register v of block tm of
// this lane (wave row wm, lane half lh) is such a column: row 64 wm + 32 tm + 8 (v / 4) + 4 lh + v % 4 of the tile.
__device__ __forceinline__ uint32_t known_mask(KnownCursor& k, const int32_t* __restrict__ col, int64_t c0, int wm,
                                               int lh) {
  uint32_t mask = 0u;
  const int64_t c_end = c0 + kRankTile;
  while (k.nxt < c_end) {
    const int64_t r64 = k.nxt - c0;
    if (r64 >= 0) {
      const int r = (int)r64;
      if ((r >> 6) == wm && ((r >> 2) & 1) == lh) mask |= 1u << (16 * ((r >> 5) & 1) + 4 * ((r & 31) >> 3) + (r & 3));
    }
    ++k.cur;
    k.nxt = k.cur < k.end ? (int64_t)col[k.cur] : kNoKnown;
  }
  return mask;
}

// (m, s) <- (m, s) (+) (m2, s2): s is a sum of exp(t - m); an empty side has m = -inf, s = 0
__device__ __forceinline__ void lse_join(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) {
    s = 0.0f;
  } else {
    s = s * expf(m - mm) + s2 * expf(m2 - mm);
  }
  m = mm;
}

// ---- forward ------------------------------------------------------------------------------------------------------
// k_rank_sweep's geometry: workgroup = 4 waves as 2 x 2, each 64 destinations x 64 queries; in an accumulator block
// lane (li, lh) holds query column li and the destination rows 8 (v / 4) + 4 lh + v % 4.  blockIdx.x = split *
// n_qblocks + query block.  part[split * Q + q] = (max, sum) of the split's candidates of query q.
// A24 (SEG): a lane sums a destination only inside its query column's segment [lo, lo + n), and the workgroup's splits
// cut the tiles its 128 queries' segments cover (seg_tile_slice; tiles_per_split / n_tiles are then unused, `splits`
// is).  A slice may be empty; k_lse_merge reads every split, so it still writes its (-inf, 0).
template <bool VEC, bool SEG = false>
__global__ __launch_bounds__(256, 2) void k_lse_sweep(const int64_t* __restrict__ src, int64_t Q, int64_t n_src,
                                                      int64_t n_dst, const float* __restrict__ zs, int64_t lds_,
                                                      const float* __restrict__ zd, int64_t ldd, int F, float inv_t,
                                                      const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, float2* __restrict__ part,
                                                      int64_t n_qblocks, int64_t tiles_per_split, int64_t n_tiles,
                                                      int64_t splits = 1, const int32_t* __restrict__ src_seg = nullptr,
                                                      const int32_t* __restrict__ dst_ptr = nullptr, int n_graphs = 1) {
  __shared__ __attribute__((aligned(16))) float As[kRankTile * kRankRow];   // destinations
  __shared__ __attribute__((aligned(16))) float Bs[kRankTile * kRankRow];   // queries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int64_t qb = (int64_t)blockIdx.x % n_qblocks, split = (int64_t)blockIdx.x / n_qblocks;
  const int64_t q0 = qb * kRankTile;
  int64_t t_beg = split * tiles_per_split;
  int64_t t_end = t_beg + tiles_per_split < n_tiles ? t_beg + tiles_per_split : n_tiles;
  if constexpr (!SEG)
    if (t_beg >= t_end) return;

  // this lane's query columns
  float m[2] = {-INFINITY, -INFINITY}, s[2] = {0.0f, 0.0f};
  int64_t qcol[2];
  uint32_t slo[2] = {0u, 0u}, sn[2] = {0u, 0u};
  KnownCursor kc[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    qcol[tn] = q0 + wn * 64 + tn * 32 + li;
    const int64_t q = qcol[tn] < Q ? qcol[tn] : Q - 1;
    if constexpr (SEG) seg_range(src_seg, dst_ptr, n_graphs, clamp_id(src[q], n_src), n_dst, slo[tn], sn[tn]);
    else known_open(kc[tn], rowptr, col, clamp_id(src[q], n_src), t_beg * kRankTile);
  }
  if constexpr (SEG) {
    seg_tile_slice(slo, sn, split, splits, t_beg, t_end);
    if (t_beg >= t_end) {   // block-uniform: nothing of this split is a candidate
      if (lh == 0 && wm == 0) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          if (qcol[tn] < Q) part[split * Q + qcol[tn]] = make_float2(-INFINITY, 0.0f);
      }
      return;
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t q = qcol[tn] < Q ? qcol[tn] : Q - 1;
      known_open(kc[tn], rowptr, col, clamp_id(src[q], n_src), t_beg * kRankTile);
    }
  }

  // staging as k_rank_sweep: thread (r = tid / 8, kq = tid % 8) moves features 4 kq .. 4 kq + 3 of rows r + 32 i; rows
  // past the end are clamped to the last one (loaded, never counted)
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  const float* qrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t q = q0 + lr + 32 * i < Q ? q0 + lr + 32 * i : Q - 1;
    qrow[i] = zs + clamp_id(src[q], n_src) * lds_;
  }

  const int nk = (F + kRankBK - 1) / kRankBK;
  float4 ra[4], rb[4];
  auto load_stage = [&](int64_t tile, int kc_) {
    const int64_t c0 = tile * kRankTile;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t c = c0 + lr + 32 * i < n_dst ? c0 + lr + 32 * i : n_dst - 1;
      ra[i] = ld_k4<VEC>(zd + c * ldd, kc_ * kRankBK + lk, F);
      rb[i] = ld_k4<VEC>(qrow[i], kc_ * kRankBK + lk, F);
    }
  };

  load_stage(t_beg, 0);
  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t c0 = tile * kRankTile;
    uint32_t km[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) km[tn] = known_mask(kc[tn], col, c0, wm, lh);
    f32x16 acc[2][2];
    zero_acc(acc);
    for (int kc_ = 0; kc_ < nk; ++kc_) {
      __syncthreads();   // the previous stage's reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(As + (lr + 32 * i) * kRankRow + lk) = ra[i];
        *reinterpret_cast<float4*>(Bs + (lr + 32 * i) * kRankRow + lk) = rb[i];
      }
      __syncthreads();
      if (kc_ + 1 < nk) load_stage(tile, kc_ + 1);
      else if (tile + 1 < t_end) load_stage(tile + 1, 0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < kRankBK / 8; ++c) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          fa[t] = *reinterpret_cast<const float4*>(As + (wm * 64 + t * 32 + li) * kRankRow + c * 8 + lh * 4);
          fb[t] = *reinterpret_cast<const float4*>(Bs + (wn * 64 + t * 32 + li) * kRankRow + c * 8 + lh * 4);
        }
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) mfma_k8(acc[tm][tn], fa[tm], fb[tn]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    // online log-sum-exp in registers: t = score * inv_t, -inf for a row past n_dst or a known neighbour
    const int64_t cbase = c0 + wm * 64 + 4 * lh;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      float mx = -INFINITY;
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t c = cbase + tm * 32 + 8 * (v >> 2) + (v & 3);
          bool ok = c < n_dst && ((km[tn] >> (16 * tm + v)) & 1u) == 0u;
          if constexpr (SEG) ok = ok && (uint32_t)c - slo[tn] < sn[tn];   // unsigned: slo <= c < slo + sn
          const float t = ok ? acc[tm][tn][v] * inv_t : -INFINITY;
          acc[tm][tn][v] = t;
          mx = fmaxf(mx, t);
        }
      if (mx > m[tn]) {
        s[tn] *= expf(m[tn] - mx);   // m = -inf: s is 0 and stays 0
        m[tn] = mx;
      }
      if (m[tn] > -INFINITY) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int v = 0; v < 16; ++v) s[tn] += expf(acc[tm][tn][v] - m[tn]);
      }
    }
  }
  // fold: lane half, then the two wm waves (through LDS), one partial per (split, query)
  __syncthreads();   // the last stage's reads are done: As is free
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const float m2 = __shfl_xor(m[tn], 32, 64), s2 = __shfl_xor(s[tn], 32, 64);
    if (lh == 0) lse_join(m[tn], s[tn], m2, s2);
    if (lh == 0 && wm == 1) {
      As[2 * (wn * 64 + tn * 32 + li)] = m[tn];
      As[2 * (wn * 64 + tn * 32 + li) + 1] = s[tn];
    }
  }
  __syncthreads();
  if (lh == 0 && wm == 0) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      lse_join(m[tn], s[tn], As[2 * (wn * 64 + tn * 32 + li)], As[2 * (wn * 64 + tn * 32 + li) + 1]);
      if (qcol[tn] < Q) part[split * Q + qcol[tn]] = make_float2(m[tn], s[tn]);
    }
  }
}

__global__ __launch_bounds__(256) void k_lse_merge(const float2* __restrict__ part, int64_t Q, int64_t splits,
                                                   float* __restrict__ lse) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  float m = -INFINITY, s = 0.0f;
  for (int64_t sp = 0; sp < splits; ++sp) {
    const float2 p = part[sp * Q + q];
    lse_join(m, s, p.x, p.y);
  }
  lse[q] = s > 0.0f ? m + logf(s) : -INFINITY;
}

// ---- backward -----------------------------------------------------------------------------------------------------
// One template for both gradients.  The 128 x 128 block of t for (destination tile, query block) is computed exactly as
// in k_lse_sweep; SRC: the workgroup's query block `stat` is fixed and the tiles [it_beg, it_end) are swept, DST: the
// tile `stat` is fixed and the query blocks are swept.  W[c, q] = g[q] * inv_t * exp(t - lse[q]) (0 where masked)
// replaces t in the accumulators and goes through LDS in four chunks of 32 swept rows as operand A of
//   SRC: out[q, f] += sum_c W[c, q] * z_dst[c, f]        DST: out[c, f] += sum_q W[c, q] * z_src[src[q], f]
// (operand B: the chunk's 32 embedding rows x FC = 64 NU output features in their own LDS buffer, read as scalars down
// the rows).  Wave (wm, wn) owns output rows 64 wm .. 64 wm + 63 and output features f0 + 32 NU wn .. + 32 NU - 1; lane
// (li, lh) of an output block holds feature column li and rows 8 (v / 4) + 4 lh + v % 4.  NU = 2 up to F = 128, else 4:
// t is recomputed once per 256 output features.  blockIdx.x = (chunk * splits + split) * n_stat + stat.
// part = NULL: one split, rows go straight to out (SRC: row src[q]); else part[(split * rows + row) * F + f].
// One workgroup per CU (no scratch): at NU = 2 the two accumulator sets of 64, the prefetched stage and the second
// product's rows spill 50 .. 56 VGPRs when the kernel is held to the 256 registers of two per CU.
// A24 (SEG): W is also 0 outside the query column's segment.  SRC: the swept tiles are this split's slice of the tiles
// the block's segments cover (seg_tile_slice); an empty slice sweeps nothing and still writes its zeros (k_lse_fold
// adds every split).  DST: the plan's query blocks are swept, but a block whose covered range blk_rng[qb] = [lo, hi)
// (k_lse_blk_range) misses this tile is skipped whole, workgroup-uniformly, and the prefetch looks for the next block
// that is not; a tile every block skips writes zeros (g_dst is not cleared by the caller).
template <bool VEC, bool DST, int NU, bool SEG = false>
__global__ __launch_bounds__(256, 1) void k_lse_bwd(const int64_t* __restrict__ src, int64_t Q, int64_t n_src,
                                                    int64_t n_dst, const float* __restrict__ zs, int64_t lds_,
                                                    const float* __restrict__ zd, int64_t ldd, int F, float inv_t,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, const float* __restrict__ lse,
                                                    const float* __restrict__ g, float* __restrict__ out, int64_t ldo,
                                                    float* __restrict__ part, int64_t n_stat, int64_t per_split,
                                                    int64_t n_sweep, int64_t splits,
                                                    const int32_t* __restrict__ src_seg = nullptr,
                                                    const int32_t* __restrict__ dst_ptr = nullptr, int n_graphs = 1,
                                                    const int2* __restrict__ blk_rng = nullptr) {
  constexpr int FC = 64 * NU;     // output features of this workgroup
  constexpr int ZROW = FC + 4;    // LDS row stride of the second product's 32 embedding rows
  __shared__ __attribute__((aligned(16))) float As[kRankTile * kRankRow];   // destinations
  __shared__ __attribute__((aligned(16))) float Bs[kRankTile * kRankRow];   // queries; then the W chunk
  __shared__ __attribute__((aligned(16))) float Zs[32 * ZROW];              // the second product's embedding rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int64_t stat = (int64_t)blockIdx.x % n_stat;
  const int64_t rest = (int64_t)blockIdx.x / n_stat;
  const int64_t split = rest % splits;
  const int f0 = (int)(rest / splits) * FC;
  int64_t it_beg = split * per_split;
  int64_t it_end = it_beg + per_split < n_sweep ? it_beg + per_split : n_sweep;
  if constexpr (!SEG || DST)
    if (it_beg >= it_end) return;

  // this lane's query columns: g * inv_t, lse, whether the column counts, the cursor into the known row
  float gq[2], lq[2];
  bool qok[2];
  KnownCursor kc[2];
  uint32_t slo[2] = {0u, 0u}, sn[2] = {0u, 0u};   // SEG: the columns' segments
  auto open_segs = [&](int64_t qb) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t qc = qb * kRankTile + wn * 64 + tn * 32 + li;
      seg_range(src_seg, dst_ptr, n_graphs, clamp_id(src[qc < Q ? qc : Q - 1], n_src), n_dst, slo[tn], sn[tn]);
    }
  };
  auto open_cols = [&](int64_t qb, int64_t tile) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t qc = qb * kRankTile + wn * 64 + tn * 32 + li;
      const int64_t q = qc < Q ? qc : Q - 1;
      gq[tn] = g[q] * inv_t;
      lq[tn] = lse[q];
      qok[tn] = qc < Q && lq[tn] > -INFINITY;
      known_open(kc[tn], rowptr, col, clamp_id(src[q], n_src), tile * kRankTile);
    }
    if constexpr (SEG && DST) open_segs(qb);
  };
  // SEG, DST: the first query block at or after `it` whose covered destinations touch this tile (it_end: none)
  auto next_live = [&](int64_t it) -> int64_t {
    if constexpr (SEG && DST) {
      const int64_t c_lo = stat * kRankTile, c_hi = c_lo + kRankTile;
      for (; it < it_end; ++it) {
        const int2 r = blk_rng[it];
        if ((int64_t)r.x < c_hi && (int64_t)r.y > c_lo) break;
      }
    }
    return it;
  };
  if constexpr (SEG && !DST) {
    open_segs(stat);
    seg_tile_slice(slo, sn, split, splits, it_beg, it_end);   // may be empty: the zeros below are still written
  }
  if constexpr (SEG && DST) it_beg = next_live(it_beg);

  const int lr = tid >> 3, lk = (tid & 7) * 4;
  const float* arow[4];
  const float* brow[4];
  auto set_a = [&](int64_t tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t c = tile * kRankTile + lr + 32 * i;
      arow[i] = zd + (c < n_dst ? c : n_dst - 1) * ldd;
    }
  };
  auto set_b = [&](int64_t qb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t q = qb * kRankTile + lr + 32 * i;
      brow[i] = zs + clamp_id(src[q < Q ? q : Q - 1], n_src) * lds_;
    }
  };
  const int nk = (F + kRankBK - 1) / kRankBK;
  float4 ra[4], rb[4];
  auto load_stage = [&](int kc_) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = ld_k4<VEC>(arow[i], kc_ * kRankBK + lk, F);
      rb[i] = ld_k4<VEC>(brow[i], kc_ * kRankBK + lk, F);
    }
  };

  f32x16 acc2[2][NU];
  zero_acc(acc2);
  if (!SEG || it_beg < it_end) {   // block-uniform
    set_a(DST ? stat : it_beg);
    set_b(DST ? it_beg : stat);
    load_stage(0);
    if constexpr (!DST) open_cols(stat, it_beg);
  }
  for (int64_t it = it_beg, nxt; it < it_end; it = nxt) {
    nxt = next_live(it + 1);
    const int64_t tile = DST ? stat : it, qb = DST ? it : stat;
    const int64_t c0 = tile * kRankTile;
    if constexpr (DST) open_cols(qb, tile);
    uint32_t km[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) km[tn] = known_mask(kc[tn], col, c0, wm, lh);
    f32x16 acc[2][2];
    zero_acc(acc);
    for (int kc_ = 0; kc_ < nk; ++kc_) {
      __syncthreads();   // the previous stage's (or the previous second product's) reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(As + (lr + 32 * i) * kRankRow + lk) = ra[i];
        *reinterpret_cast<float4*>(Bs + (lr + 32 * i) * kRankRow + lk) = rb[i];
      }
      __syncthreads();
      if (kc_ + 1 < nk) {
        load_stage(kc_ + 1);
      } else if (nxt < it_end) {
        if constexpr (DST) set_b(nxt);
        else set_a(nxt);
        load_stage(0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < kRankBK / 8; ++c) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          fa[t] = *reinterpret_cast<const float4*>(As + (wm * 64 + t * 32 + li) * kRankRow + c * 8 + lh * 4);
          fb[t] = *reinterpret_cast<const float4*>(Bs + (wn * 64 + t * 32 + li) * kRankRow + c * 8 + lh * 4);
        }
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) mfma_k8(acc[tm][tn], fa[tm], fb[tn]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    // t -> W in registers, the forward's mask
    const int64_t cbase = c0 + wm * 64 + 4 * lh;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t c = cbase + tm * 32 + 8 * (v >> 2) + (v & 3);
          bool ok = qok[tn] && c < n_dst && ((km[tn] >> (16 * tm + v)) & 1u) == 0u;
          if constexpr (SEG) ok = ok && (uint32_t)c - slo[tn] < sn[tn];   // unsigned: slo <= c < slo + sn
          const float t = acc[tm][tn][v] * inv_t;
          acc[tm][tn][v] = ok ? gq[tn] * expf(t - lq[tn]) : 0.0f;
        }
    // the second product, 32 swept rows at a time (SRC: chunk = 2 wm + tm of the tile; DST: 2 wn + tn of the block)
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const float* zrow;
      if constexpr (DST) {
        const int64_t q = qb * kRankTile + ch * 32 + lr;
        zrow = zs + clamp_id(src[q < Q ? q : Q - 1], n_src) * lds_;
      } else {
        const int64_t c = c0 + ch * 32 + lr;
        zrow = zd + (c < n_dst ? c : n_dst - 1) * ldd;
      }
      float4 rz[FC / 32];
#pragma unroll
      for (int j = 0; j < FC / 32; ++j) rz[j] = ld_k4<VEC>(zrow, f0 + lk + 32 * j, F);
      __syncthreads();   // the first product's (or the previous chunk's) reads are done
      if constexpr (DST) {
        if (wn == (ch >> 1)) {
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int v = 0; v < 16; ++v)
              Bs[(wm * 64 + tm * 32 + 8 * (v >> 2) + 4 * lh + (v & 3)) * kRankRow + li] = acc[tm][ch & 1][v];
        }
      } else {
        if (wm == (ch >> 1)) {
#pragma unroll
          for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int vq = 0; vq < 4; ++vq)
              *reinterpret_cast<float4*>(Bs + (wn * 64 + tn * 32 + li) * kRankRow + 8 * vq + 4 * lh) =
                  make_float4(acc[ch & 1][tn][4 * vq], acc[ch & 1][tn][4 * vq + 1], acc[ch & 1][tn][4 * vq + 2],
                              acc[ch & 1][tn][4 * vq + 3]);
        }
      }
#pragma unroll
      for (int j = 0; j < FC / 32; ++j) *reinterpret_cast<float4*>(Zs + lr * ZROW + lk + 32 * j) = rz[j];
      __syncthreads();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float4 fa[2], fb[NU];
#pragma unroll
        for (int t = 0; t < 2; ++t)
          fa[t] = *reinterpret_cast<const float4*>(Bs + (wm * 64 + t * 32 + li) * kRankRow + kk * 8 + lh * 4);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const float* zc = Zs + (kk * 8 + lh * 4) * ZROW + wn * (32 * NU) + u * 32 + li;
          fb[u] = make_float4(zc[0], zc[ZROW], zc[2 * ZROW], zc[3 * ZROW]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int u = 0; u < NU; ++u)
            if (f0 + wn * (32 * NU) + u * 32 < F) mfma_k8(acc2[t][u], fa[t], fb[u]);   // wave-uniform
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  const int64_t n_rows = DST ? n_dst : Q;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t r = stat * kRankTile + wm * 64 + t * 32 + 8 * (v >> 2) + 4 * lh + (v & 3);
      if (r >= n_rows) continue;
      float* row;
      if (part != nullptr) row = part + (split * n_rows + r) * F;
      else row = out + (DST ? r : clamp_id(src[r], n_src)) * ldo;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int f = f0 + wn * (32 * NU) + u * 32 + li;
        if (f < F) row[f] = acc2[t][u][v];
      }
    }
}

// out[row(r), f] = sum over the splits, ascending; row(r) = idx[r] (G_src) or r (G_dst)
__global__ __launch_bounds__(256) void k_lse_fold(const float* __restrict__ part, int64_t splits, int64_t n_rows, int F,
                                                  const int64_t* __restrict__ idx, int64_t n_idx_rows,
                                                  float* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows * F) return;
  const int64_t r = i / F;
  const int f = (int)(i - r * F);
  float acc = 0.0f;
  for (int64_t sp = 0; sp < splits; ++sp) acc += part[(sp * n_rows + r) * F + f];
  const int64_t row = idx != nullptr ? clamp_id(idx[r], n_idx_rows) : r;
  out[row * ldo + f] = acc;
}

// A24: rng[qb] = [min lo, max hi) over the non-empty segments of query block qb's queries; (INT_MAX, 0) when it has
// none.  One workgroup of 128 threads per query block.
__global__ __launch_bounds__(kRankTile) void k_lse_blk_range(const int64_t* __restrict__ src, int64_t Q, int64_t n_src,
                                                              int64_t n_dst, const int32_t* __restrict__ src_seg,
                                                              const int32_t* __restrict__ dst_ptr, int n_graphs,
                                                              int2* __restrict__ rng) {
  __shared__ int s_lo, s_hi;
  if (threadIdx.x == 0) {
    s_lo = 0x7fffffff;
    s_hi = 0;
  }
  __syncthreads();
  const int64_t q = (int64_t)blockIdx.x * kRankTile + threadIdx.x;
  if (q < Q) {
    uint32_t lo, n;
    seg_range(src_seg, dst_ptr, n_graphs, clamp_id(src[q], n_src), n_dst, lo, n);
    if (n != 0u) {
      atomicMin(&s_lo, (int)lo);
      atomicMax(&s_hi, (int)(lo + n));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) rng[blockIdx.x] = make_int2(s_lo, s_hi);
}

struct LsePlans {
  SweepPlan fwd, dst;   // fwd also cuts bwd_src (query-stationary); dst: destination tiles stationary, query blocks swept
  size_t fwd_bytes, src_bytes, dst_bytes;
  size_t rng_bytes;     // A24: the query blocks' covered ranges, behind the partials of the segmented bwd_dst
};
LsePlans lse_plans(int64_t Q, int64_t n_dst, int64_t F) {
  LsePlans p;
  p.fwd = sweep_plan(Q, n_dst);
  p.dst = sweep_plan(n_dst, Q);
  p.fwd_bytes = align_up((size_t)p.fwd.splits * (size_t)Q * sizeof(float2), 256);
  p.src_bytes = p.fwd.splits > 1 ? align_up((size_t)p.fwd.splits * (size_t)Q * (size_t)F * sizeof(float), 256) : 0;
  p.dst_bytes = p.dst.splits > 1 ? align_up((size_t)p.dst.splits * (size_t)n_dst * (size_t)F * sizeof(float), 256) : 0;
  p.rng_bytes = align_up((size_t)p.fwd.n_qblocks * sizeof(int2), 256);
  return p;
}

// The split partials of a gradient, splits x rows x F floats, stay below 2^39 elements (2 TiB): their byte count fits
// a size_t with room to spare and k_lse_fold's grid, rows x F / 256 workgroups, fits the 2^31 of a launch.
constexpr int64_t kLseMaxPartial = int64_t(1) << 39;

int lse_check_shapes(const char* what, int64_t Q, int64_t n_dst, int64_t F) {
  HGIN_ARG_CHECK(Q >= 1 && Q < (int64_t(1) << 31), "%s: n_query = %lld must be in [1, 2^31)", what, (long long)Q);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  // splits <= 512, rows < 2^31, F < 2^24: the products below cannot overflow an int64
  const SweepPlan src = sweep_plan(Q, n_dst), dst = sweep_plan(n_dst, Q);
  HGIN_ARG_CHECK(src.splits == 1 || src.splits * Q * F < kLseMaxPartial,
                 "%s: the split partials of g_src (%lld x %lld x %lld floats) exceed 2^39 elements", what,
                 (long long)src.splits, (long long)Q, (long long)F);
  HGIN_ARG_CHECK(dst.splits == 1 || dst.splits * n_dst * F < kLseMaxPartial,
                 "%s: the split partials of g_dst (%lld x %lld x %lld floats) exceed 2^39 elements", what,
                 (long long)dst.splits, (long long)n_dst, (long long)F);
  return HGIN_OK;
}

int lse_check_operands(const char* what, const int64_t* src, int64_t Q, int64_t n_src, int64_t n_dst,
                       const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                       const int32_t* known_rowptr, const int32_t* known_col) {
  const int rc = lse_check_shapes(what, Q, n_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_src >= 1 && n_src < (int64_t(1) << 31), "%s: n_src must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(src != nullptr, "%s: src NULL", what);
  HGIN_ARG_CHECK(z_src != nullptr, "%s: z_src NULL", what);
  HGIN_ARG_CHECK(z_dst != nullptr, "%s: z_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "%s: leading dimension too small", what);
  HGIN_ARG_CHECK(std::isfinite(inv_t) && inv_t > 0.0f, "%s: inv_t = %g must be finite and > 0", what, (double)inv_t);
  HGIN_ARG_CHECK(known_rowptr == nullptr || known_col != nullptr, "%s: known_rowptr without known_col", what);
  return HGIN_OK;
}

int lse_check_ws(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  if (need != 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, need);
    return HGIN_E_WORKSPACE;
  }
  return HGIN_OK;
}

// A24's additional arguments
int lse_check_seg(const char* what, const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs) {
  HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
  HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  HGIN_ARG_CHECK(n_graphs >= 1 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [1, 2^31)", what,
                 (long long)n_graphs);
  return HGIN_OK;
}

size_t lse_workspace(const LsePlans& p, bool seg) {
  size_t need = p.fwd_bytes;
  if (p.src_bytes > need) need = p.src_bytes;
  const size_t dst = p.dst_bytes + (seg ? p.rng_bytes : 0);
  if (dst > need) need = dst;
  return need;
}

// A23 (src_seg = NULL) and A24 behind one set of checks and launches
int lse_fwd_impl(const char* what, const int64_t* src, int64_t Q, int64_t n_src, int64_t n_dst, const float* z_src,
                 int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                 const int32_t* known_rowptr, const int32_t* known_col, float* lse, void* ws, size_t ws_bytes,
                 const int32_t* src_seg, const int32_t* dst_ptr, int n_graphs, void* stream) {
  const bool seg = src_seg != nullptr;
  int rc = lse_check_operands(what, src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t, known_rowptr,
                              known_col);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(lse != nullptr, "%s: lse NULL", what);
  const LsePlans plans = lse_plans(Q, n_dst, F);
  const SweepPlan plan = plans.fwd;
  HGIN_ARG_CHECK(plan.n_qblocks * plan.splits < (int64_t(1) << 31), "%s: too many workgroups", what);
  rc = lse_check_ws(what, ws, ws_bytes, plans.fwd_bytes);
  if (rc != HGIN_OK) return rc;
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  float2* part = static_cast<float2*>(ws);
  const unsigned grid = (unsigned)(plan.n_qblocks * plan.splits);
  if (seg) {
    HGIN_TRACE("k_lse_sweep<%d,SEG> splits=%lld sweep=%lld", vec ? 4 : 1, (long long)plan.splits,
               (long long)plan.tiles_per_split);
    if (vec)
      k_lse_sweep<true, true><<<grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, inv_t,
                                                   known_rowptr, known_col, part, plan.n_qblocks,
                                                   plan.tiles_per_split, plan.n_tiles, plan.splits, src_seg, dst_ptr,
                                                   n_graphs);
    else
      k_lse_sweep<false, true><<<grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, inv_t,
                                                    known_rowptr, known_col, part, plan.n_qblocks,
                                                    plan.tiles_per_split, plan.n_tiles, plan.splits, src_seg, dst_ptr,
                                                    n_graphs);
  } else {
    HGIN_TRACE("k_lse_sweep<%d> splits=%lld sweep=%lld", vec ? 4 : 1, (long long)plan.splits,
               (long long)plan.tiles_per_split);
    if (vec)
      k_lse_sweep<true><<<grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, inv_t,
                                             known_rowptr, known_col, part, plan.n_qblocks, plan.tiles_per_split,
                                             plan.n_tiles);
    else
      k_lse_sweep<false><<<grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, inv_t,
                                              known_rowptr, known_col, part, plan.n_qblocks, plan.tiles_per_split,
                                              plan.n_tiles);
  }
  HGIN_TRACE("k_lse_merge splits=%lld", (long long)plan.splits);
  k_lse_merge<<<(unsigned)ceil_div(Q, 256), 256, 0, s>>>(part, Q, plan.splits, lse);
  return check_launch(what);
}

// both gradients, A23 (src_seg = NULL) and A24, behind one set of checks and launches
int lse_bwd_impl(const char* what, bool dst, const int64_t* src, int64_t Q, int64_t n_src, int64_t n_dst,
                 const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                 const int32_t* known_rowptr, const int32_t* known_col, const float* lse, const float* g, float* out,
                 int64_t ldo, void* ws, size_t ws_bytes, const int32_t* src_seg, const int32_t* dst_ptr, int n_graphs,
                 void* stream) {
  const bool seg = src_seg != nullptr;
  int rc = lse_check_operands(what, src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t, known_rowptr,
                              known_col);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(lse != nullptr, "%s: lse NULL", what);
  HGIN_ARG_CHECK(g != nullptr, "%s: g NULL", what);
  HGIN_ARG_CHECK(out != nullptr, "%s: %s NULL", what, dst ? "g_dst" : "g_src");
  HGIN_ARG_CHECK(ldo >= F, "%s: leading dimension too small", what);
  const LsePlans plans = lse_plans(Q, n_dst, F);
  const SweepPlan plan = dst ? plans.dst : plans.fwd;
  const int64_t chunks = ceil_div(F, lse_feature_chunk(F));
  const int64_t grid = plan.n_qblocks * plan.splits * chunks;
  HGIN_ARG_CHECK(grid < (int64_t(1) << 31), "%s: %lld workgroups exceed 2^31", what, (long long)grid);
  const size_t part_bytes = dst ? plans.dst_bytes : plans.src_bytes;
  rc = lse_check_ws(what, ws, ws_bytes, part_bytes + (seg && dst ? plans.rng_bytes : 0));
  if (rc != HGIN_OK) return rc;
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  float* part = plan.splits > 1 ? static_cast<float*>(ws) : nullptr;
  if (!dst) {   // rows of z_src that are no query's source
    hipError_t e = hipMemset2DAsync(out, (size_t)ldo * sizeof(float), 0, (size_t)F * sizeof(float), (size_t)n_src, s);
    if (e != hipSuccess) {
      set_error("%s: hipMemset2DAsync failed: %s", what, hipGetErrorString(e));
      return static_cast<int>(e);
    }
  }
  int2* rng = nullptr;
  if (seg && dst) {   // the query blocks' covered ranges, behind the partials
    rng = reinterpret_cast<int2*>(static_cast<char*>(ws) + part_bytes);
    HGIN_TRACE("k_lse_blk_range blocks=%lld", (long long)plans.fwd.n_qblocks);
    k_lse_blk_range<<<(unsigned)plans.fwd.n_qblocks, kRankTile, 0, s>>>(src, Q, n_src, n_dst, src_seg, dst_ptr,
                                                                         n_graphs, rng);
  }
  HGIN_TRACE("k_lse_bwd<%d,%s%s> splits=%lld sweep=%lld chunks=%lld", vec ? 4 : 1, dst ? "DST" : "SRC",
             seg ? ",SEG" : "", (long long)plan.splits, (long long)plan.tiles_per_split, (long long)chunks);
#define HGIN_LSE_BWD_NU(VEC_, DST_, NU_)                                                                              \
  do {                                                                                                                \
    if (seg)                                                                                                          \
      k_lse_bwd<VEC_, DST_, NU_, true><<<(unsigned)grid, 256, 0, s>>>(                                                \
          src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, inv_t, known_rowptr, known_col, lse, g, out,    \
          ldo, part, plan.n_qblocks, plan.tiles_per_split, plan.n_tiles, plan.splits, src_seg, dst_ptr, n_graphs,     \
          rng);                                                                                                       \
    else                                                                                                              \
      k_lse_bwd<VEC_, DST_, NU_><<<(unsigned)grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst,   \
                                                                (int)F, inv_t, known_rowptr, known_col, lse, g, out,  \
                                                                ldo, part, plan.n_qblocks, plan.tiles_per_split,      \
                                                                plan.n_tiles, plan.splits);                           \
  } while (0)
#define HGIN_LSE_BWD(VEC_, DST_)                 \
  do {                                           \
    if (F > 128) HGIN_LSE_BWD_NU(VEC_, DST_, 4); \
    else HGIN_LSE_BWD_NU(VEC_, DST_, 2);         \
  } while (0)
  if (dst) {
    if (vec) HGIN_LSE_BWD(true, true);
    else HGIN_LSE_BWD(false, true);
  } else {
    if (vec) HGIN_LSE_BWD(true, false);
    else HGIN_LSE_BWD(false, false);
  }
#undef HGIN_LSE_BWD
#undef HGIN_LSE_BWD_NU
  if (part != nullptr) {
    const int64_t n_rows = dst ? n_dst : Q;   // n_rows * F < 2^39 (lse_check_shapes): the grid is below 2^31
    HGIN_TRACE("k_lse_fold<%s> splits=%lld", dst ? "DST" : "SRC", (long long)plan.splits);
    k_lse_fold<<<(unsigned)ceil_div(n_rows * F, 256), 256, 0, s>>>(part, plan.splits, n_rows, (int)F,
                                                                     dst ? nullptr : src, n_src, out, ldo);
  }
  return check_launch(what);
}

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_link_lse_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, size_t* bytes) {
  const char* what = "hgin_link_lse_workspace_size";
  HGIN_ARG_CHECK(bytes != nullptr, "%s: bytes is NULL", what);
  const int rc = lse_check_shapes(what, n_query, n_dst, F);
  if (rc != HGIN_OK) return rc;
  *bytes = lse_workspace(lse_plans(n_query, n_dst, F), false);
  return HGIN_OK;
}

extern "C" int hgin_link_lse_fwd_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                     const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                     float inv_t, const int32_t* known_rowptr, const int32_t* known_col, float* lse,
                                     void* ws, size_t ws_bytes, void* stream) {
  return lse_fwd_impl("hgin_link_lse_fwd_f32", src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t,
                      known_rowptr, known_col, lse, ws, ws_bytes, nullptr, nullptr, 1, stream);
}

extern "C" int hgin_link_lse_bwd_src_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                         const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                         int64_t F, float inv_t, const int32_t* known_rowptr, const int32_t* known_col,
                                         const float* lse, const float* g, float* g_src, int64_t ld_gsrc, void* ws,
                                         size_t ws_bytes, void* stream) {
  return lse_bwd_impl("hgin_link_lse_bwd_src_f32", false, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F,
                      inv_t, known_rowptr, known_col, lse, g, g_src, ld_gsrc, ws, ws_bytes, nullptr, nullptr, 1,
                      stream);
}

extern "C" int hgin_link_lse_bwd_dst_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                         const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                         int64_t F, float inv_t, const int32_t* known_rowptr, const int32_t* known_col,
                                         const float* lse, const float* g, float* g_dst, int64_t ld_gdst, void* ws,
                                         size_t ws_bytes, void* stream) {
  return lse_bwd_impl("hgin_link_lse_bwd_dst_f32", true, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F,
                      inv_t, known_rowptr, known_col, lse, g, g_dst, ld_gdst, ws, ws_bytes, nullptr, nullptr, 1,
                      stream);
}

// ---- A24: the same three calls over graph-local candidates ------------------------------------------------------------
extern "C" int hgin_link_lse_seg_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, size_t* bytes) {
  const char* what = "hgin_link_lse_seg_workspace_size";
  HGIN_ARG_CHECK(bytes != nullptr, "%s: bytes is NULL", what);
  const int rc = lse_check_shapes(what, n_query, n_dst, F);
  if (rc != HGIN_OK) return rc;
  *bytes = lse_workspace(lse_plans(n_query, n_dst, F), true);
  return HGIN_OK;
}

extern "C" int hgin_link_lse_fwd_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                         const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                         int64_t F, float inv_t, const int32_t* known_rowptr, const int32_t* known_col,
                                         float* lse, void* ws, size_t ws_bytes, const int32_t* src_seg,
                                         const int32_t* dst_ptr, int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_lse_fwd_seg_f32";
  const int rc = lse_check_seg(what, src_seg, dst_ptr, n_graphs);
  if (rc != HGIN_OK) return rc;
  return lse_fwd_impl(what, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t, known_rowptr,
                      known_col, lse, ws, ws_bytes, src_seg, dst_ptr, (int)n_graphs, stream);
}

extern "C" int hgin_link_lse_bwd_src_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                             const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                             int64_t F, float inv_t, const int32_t* known_rowptr,
                                             const int32_t* known_col, const float* lse, const float* g, float* g_src,
                                             int64_t ld_gsrc, void* ws, size_t ws_bytes, const int32_t* src_seg,
                                             const int32_t* dst_ptr, int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_lse_bwd_src_seg_f32";
  const int rc = lse_check_seg(what, src_seg, dst_ptr, n_graphs);
  if (rc != HGIN_OK) return rc;
  return lse_bwd_impl(what, false, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t, known_rowptr,
                      known_col, lse, g, g_src, ld_gsrc, ws, ws_bytes, src_seg, dst_ptr, (int)n_graphs, stream);
}

extern "C" int hgin_link_lse_bwd_dst_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                             const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                             int64_t F, float inv_t, const int32_t* known_rowptr,
                                             const int32_t* known_col, const float* lse, const float* g, float* g_dst,
                                             int64_t ld_gdst, void* ws, size_t ws_bytes, const int32_t* src_seg,
                                             const int32_t* dst_ptr, int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_lse_bwd_dst_seg_f32";
  const int rc = lse_check_seg(what, src_seg, dst_ptr, n_graphs);
  if (rc != HGIN_OK) return rc;
  return lse_bwd_impl(what, true, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, inv_t, known_rowptr,
                      known_col, lse, g, g_dst, ld_gdst, ws, ws_bytes, src_seg, dst_ptr, (int)n_graphs, stream);
}
