// A15 — full-candidate filtered link ranking (include/hgin.h A15).
//
// NOT IN REFERENCE: the reference regresses path delay and ranks nothing; like A13 / A14 the spec is build-defined
// (header include/hgin.h) and checked against a float64 restatement in tests/test_linkrank_host.py.
//
// The operation is a GEMM whose output is only compared: score(q, c) = <z_src[pos[0, q]], z_dst[c]> for every
// destination c, against the query's threshold score(q, pos[1, q]).  Three kernels on one arithmetic
// (v_mfma_f32_32x32x2_f32, exact fp32 products and sums; operand A = destination rows, operand B = query rows):
//   k_rank_pairs<.., false>   threshold pre-pass: a wave scores 32 (query, own destination) pairs as the diagonal of
//                             one 32 x 32 MFMA block
//   k_rank_sweep              128 queries (gathered through pos[0]) x 128-destination tiles of z_dst streamed through
//                             LDS; the accumulators are compared in registers, two counters per query column live in
//                             registers over the whole sweep and are added once (integer atomics: deterministic)
//   k_rank_pairs<.., true>    filter: per query the distinct known neighbours of its source are scored the same way
//                             and what they contributed to the sweep's counts is subtracted; writes n_cand
// One K order everywhere: blocks of 8 features in ascending order; inside a block lane half h supplies features
// 4 h .. 4 h + 3, so the four MFMAs of a block take the feature pairs (0, 4), (1, 5), (2, 6), (3, 7).  Features past F
// are zeros on both operands (they add 0 * 0).  A given (query row, destination row) pair therefore gets bit-identical
// scores in all three kernels and in every tile position: a copy of the positive's destination row is always counted
// in n_equal.
#include "hgin_linkscore.h"   // the K order, ld_k4, mfma_k8, the tile constants and the split plan (shared with A16)

namespace hgin {
namespace {

// ---- the sweep ----------------------------------------------------------------------------------------------------
// Workgroup = 4 waves as 2 x 2, each 64 destinations x 64 queries (2 x 2 MFMA blocks).  In an accumulator block lane
// (li, lh) holds query column li and the destination rows 8 (v / 4) + 4 lh + v % 4, v < 16: one threshold and one
// pair of counters per lane and query block.  blockIdx.x = split * n_qblocks + query block; a split is a contiguous
// range of destination tiles.  The (tile, K-stage) sequence is one flat pipeline: the next stage's global loads are in
// flight under this stage's MFMAs, across tile boundaries too.
// A19 (SEG): a lane compares a destination only inside its query column's segment [lo, lo + n) (two more registers
// per column), and the workgroup's splits cut the tiles its 128 queries' segments cover instead of all n_tiles
// (tiles_per_split / n_tiles are then unused; `splits` is).
template <bool VEC, bool SEG>
__global__ __launch_bounds__(256, 2) void k_rank_sweep(const int64_t* __restrict__ pos, int64_t E, int64_t n_src,
                                                    int64_t n_dst, const float* __restrict__ zs, int64_t lds_,
                                                    const float* __restrict__ zd, int64_t ldd, int F,
                                                    const float* __restrict__ thr, int32_t* __restrict__ n_gt,
                                                    int32_t* __restrict__ n_eq, int64_t n_qblocks,
                                                    int64_t tiles_per_split, int64_t n_tiles, int64_t splits,
                                                    const int32_t* __restrict__ src_seg,
                                                    const int32_t* __restrict__ dst_ptr, int n_graphs) {
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
  float th[2];
  uint32_t dq[2], slo[2] = {0u, 0u}, sn[2] = {0u, 0u};
  int64_t qcol[2];
  int gt[2] = {0, 0}, eq[2] = {0, 0};
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    qcol[tn] = q0 + wn * 64 + tn * 32 + li;
    const int64_t q = qcol[tn] < E ? qcol[tn] : E - 1;
    th[tn] = thr[q];
    dq[tn] = (uint32_t)pos[E + q];
    if constexpr (SEG) seg_range(src_seg, dst_ptr, n_graphs, clamp_id(pos[q], n_src), n_dst, slo[tn], sn[tn]);
  }
  if constexpr (SEG) {
    seg_tile_slice(slo, sn, split, splits, t_beg, t_end);
    if (t_beg >= t_end) return;   // block-uniform
  }

  // staging: thread (r = tid / 8, kq = tid % 8) moves features 4 kq .. 4 kq + 3 of rows r, r + 32, r + 64, r + 96;
  // rows past the end are clamped to the last one (loaded, never counted)
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  const float* qrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t q = q0 + lr + 32 * i < E ? q0 + lr + 32 * i : E - 1;
    qrow[i] = zs + clamp_id(pos[q], n_src) * lds_;
  }

  const int nk = (F + kRankBK - 1) / kRankBK;
  float4 ra[4], rb[4];
  auto load_stage = [&](int64_t tile, int kc) {
    const int64_t c0 = tile * kRankTile;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t c = c0 + lr + 32 * i < n_dst ? c0 + lr + 32 * i : n_dst - 1;
      ra[i] = ld_k4<VEC>(zd + c * ldd, kc * kRankBK + lk, F);
      rb[i] = ld_k4<VEC>(qrow[i], kc * kRankBK + lk, F);
    }
  };

  load_stage(t_beg, 0);
  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    f32x16 acc[2][2];
    zero_acc(acc);
    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();   // the previous stage's reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(As + (lr + 32 * i) * kRankRow + lk) = ra[i];
        *reinterpret_cast<float4*>(Bs + (lr + 32 * i) * kRankRow + lk) = rb[i];
      }
      __syncthreads();
      if (kc + 1 < nk) load_stage(tile, kc + 1);
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
    // compare in registers: destination c counts when it exists and is not the query's own destination
    const uint32_t cbase = (uint32_t)(tile * kRankTile) + wm * 64 + 4 * lh;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const uint32_t c = cbase + tm * 32 + 8 * (v >> 2) + (v & 3);
        const bool in = c < (uint32_t)n_dst;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          bool ok = in && c != dq[tn];
          if constexpr (SEG) ok = ok && c - slo[tn] < sn[tn];   // unsigned: slo <= c < slo + sn
          const float x = acc[tm][tn][v];
          gt[tn] += (ok && x > th[tn]) ? 1 : 0;
          eq[tn] += (ok && x == th[tn]) ? 1 : 0;
        }
      }
  }
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    gt[tn] += __shfl_xor(gt[tn], 32, 64);
    eq[tn] += __shfl_xor(eq[tn], 32, 64);
    if (lh == 0 && qcol[tn] < E) {
      if (gt[tn]) atomicAdd(n_gt + qcol[tn], gt[tn]);
      if (eq[tn]) atomicAdd(n_eq + qcol[tn], eq[tn]);
    }
  }
}

// ---- pairs: thresholds and the filter -------------------------------------------------------------------------------
// A wave takes 32 queries; pair j = (destination row a_j, query j) is entry (j, j) of one 32 x 32 MFMA block whose
// operands come straight from global memory (lane (li, lh): row li, features 4 lh .. 4 lh + 3 of each block of 8).
// Entry (j, j) sits in lane j + 32 ((j % 8) / 4), accumulator register 4 (j / 8) + j % 4.
template <bool VEC>
__device__ __forceinline__ float diag_score(const float* __restrict__ a, const float* __restrict__ b, int F, int lh,
                                            int vsel) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  for (int k0 = 0; k0 < F; k0 += 8) {
    const float4 fa = ld_k4<VEC>(a, k0 + lh * 4, F);
    const float4 fb = ld_k4<VEC>(b, k0 + lh * 4, F);
    mfma_k8(acc, fa, fb);
  }
  float x = acc[0];
#pragma unroll
  for (int e = 1; e < 16; ++e) x = vsel == e ? acc[e] : x;
  return x;
}

// A19 (SEG, with FILTER): a known neighbour is subtracted only inside the query's segment [lo, lo + n), and
// n_cand = n - 1 - distinct.
template <bool VEC, bool FILTER, bool SEG = false>
__global__ __launch_bounds__(256) void k_rank_pairs(const int64_t* __restrict__ pos, int64_t E, int64_t n_src,
                                                    int64_t n_dst, const float* __restrict__ zs, int64_t lds_,
                                                    const float* __restrict__ zd, int64_t ldd, int F,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, float* __restrict__ thr,
                                                    int32_t* __restrict__ n_gt, int32_t* __restrict__ n_eq,
                                                    int32_t* __restrict__ n_cand,
                                                    const int32_t* __restrict__ src_seg = nullptr,
                                                    const int32_t* __restrict__ dst_ptr = nullptr,
                                                    int n_graphs = 0) {
  const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int64_t qbase = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (qbase >= E) return;   // the whole wave
  const bool valid = qbase + li < E;
  const int64_t q = valid ? qbase + li : E - 1;
  const int64_t s = clamp_id(pos[q], n_src), d = pos[E + q];
  const float* b = zs + s * lds_;
  const bool owner = lh == ((li & 7) >> 2);
  const int vsel = 4 * (li >> 3) + (li & 3);
  if constexpr (!FILTER) {
    const float x = diag_score<VEC>(zd + clamp_id(d, n_dst) * ldd, b, F, lh, vsel);
    if (owner && valid) thr[q] = x;
  } else {
    int beg = 0, deg = 0;
    if (rowptr != nullptr) {
      beg = rowptr[s];
      deg = rowptr[s + 1] - beg;
    }
    const float th = thr[q];
    uint32_t slo = 0u, sn = (uint32_t)n_dst;
    if constexpr (SEG) seg_range(src_seg, dst_ptr, n_graphs, s, n_dst, slo, sn);
    int sub_gt = 0, sub_eq = 0, distinct = 0;
    for (int t = 0; __any(t < deg); ++t) {   // wave-uniform trip count: every lane takes part in every MFMA
      const bool has = t < deg;
      const int64_t c = has ? (int64_t)col[beg + t] : 0;
      const bool dup = has && t > 0 && (int64_t)col[beg + t - 1] == c;   // columns are sorted: duplicates are adjacent
      bool ok = has && !dup && c != d && c >= 0 && c < n_dst;
      if constexpr (SEG) ok = ok && (uint32_t)c - slo < sn;
      const float x = diag_score<VEC>(zd + clamp_id(c, n_dst) * ldd, b, F, lh, vsel);
      if (ok) {
        ++distinct;
        sub_gt += x > th ? 1 : 0;
        sub_eq += x == th ? 1 : 0;
      }
    }
    if (owner && valid) {
      n_gt[q] -= sub_gt;
      n_eq[q] -= sub_eq;
      n_cand[q] = SEG ? (int32_t)sn - 1 - distinct : (int32_t)(n_dst - 1 - distinct);
    }
  }
}

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_link_full_rank_workspace_size(int64_t n_pos, int64_t n_dst, int64_t F, size_t* bytes) {
  const char* what = "hgin_link_full_rank_workspace_size";
  HGIN_ARG_CHECK(bytes != nullptr, "%s: bytes is NULL", what);
  HGIN_ARG_CHECK(n_pos >= 1 && n_pos < (int64_t(1) << 31), "%s: E = %lld must be in [1, 2^31)", what,
                 (long long)n_pos);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  *bytes = align_up((size_t)n_pos * sizeof(float), 256);   // the thresholds
  return HGIN_OK;
}

namespace {

// A15 (src_seg = NULL) and A19 behind one set of checks and launches
int full_rank_impl(const char* what, const int64_t* pos, int64_t n_pos, int64_t n_src, int64_t n_dst,
                   const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                   const int32_t* known_rowptr, const int32_t* known_col, int32_t* n_greater, int32_t* n_equal,
                   int32_t* n_cand, void* ws, size_t ws_bytes, const int32_t* src_seg, const int32_t* dst_ptr,
                   int n_graphs, void* stream) {
  const bool seg = src_seg != nullptr;
  const int64_t E = n_pos;
  HGIN_ARG_CHECK(E >= 1 && E < (int64_t(1) << 31), "%s: E = %lld must be in [1, 2^31)", what, (long long)E);
  HGIN_ARG_CHECK(n_src >= 1 && n_src < (int64_t(1) << 31), "%s: n_src must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(pos != nullptr, "%s: pos NULL", what);
  HGIN_ARG_CHECK(z_src != nullptr, "%s: z_src NULL", what);
  HGIN_ARG_CHECK(z_dst != nullptr, "%s: z_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "%s: leading dimension too small", what);
  HGIN_ARG_CHECK(known_rowptr == nullptr || known_col != nullptr, "%s: known_rowptr without known_col", what);
  HGIN_ARG_CHECK(n_greater != nullptr, "%s: n_greater NULL", what);
  HGIN_ARG_CHECK(n_equal != nullptr, "%s: n_equal NULL", what);
  HGIN_ARG_CHECK(n_cand != nullptr, "%s: n_cand NULL", what);
  const size_t need = align_up((size_t)E * sizeof(float), 256);
  if (ws == nullptr || ws_bytes < need) {
    set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, need);
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  float* thr = static_cast<float*>(ws);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  const unsigned pair_grid = (unsigned)ceil_div(E, 128);
  const SweepPlan plan = sweep_plan(E, n_dst);
  const int64_t n_qblocks = plan.n_qblocks, n_tiles = plan.n_tiles, tiles_per_split = plan.tiles_per_split;
  const int64_t splits = plan.splits;
  const unsigned sweep_grid = (unsigned)(n_qblocks * splits);

  int rc = memset_async(n_greater, 0, (size_t)E * sizeof(int32_t), s, what);
  if (rc != HGIN_OK) return rc;
  rc = memset_async(n_equal, 0, (size_t)E * sizeof(int32_t), s, what);
  if (rc != HGIN_OK) return rc;
  HGIN_TRACE("k_rank_pairs<%d,THR>", vec ? 4 : 1);
  HGIN_TRACE("k_rank_sweep<%d%s> splits=%lld", vec ? 4 : 1, seg ? ",SEG" : "", (long long)splits);
  HGIN_TRACE("k_rank_pairs<%d,FILTER%s>", vec ? 4 : 1, seg ? ",SEG" : "");
#define HGIN_RANK_LAUNCH(VEC_, SEG_)                                                                                 \
  do {                                                                                                               \
    k_rank_pairs<VEC_, false><<<pair_grid, 256, 0, s>>>(pos, E, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F,  \
                                                        nullptr, nullptr, thr, nullptr, nullptr, nullptr);           \
    k_rank_sweep<VEC_, SEG_><<<sweep_grid, 256, 0, s>>>(pos, E, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F,  \
                                                        thr, n_greater, n_equal, n_qblocks, tiles_per_split,         \
                                                        n_tiles, splits, src_seg, dst_ptr, n_graphs);                \
    k_rank_pairs<VEC_, true, SEG_><<<pair_grid, 256, 0, s>>>(pos, E, n_src, n_dst, z_src, ld_src, z_dst, ld_dst,     \
                                                             (int)F, known_rowptr, known_col, thr, n_greater,        \
                                                             n_equal, n_cand, src_seg, dst_ptr, n_graphs);           \
  } while (0)
  if (seg) {
    if (vec) HGIN_RANK_LAUNCH(true, true);
    else HGIN_RANK_LAUNCH(false, true);
  } else {
    if (vec) HGIN_RANK_LAUNCH(true, false);
    else HGIN_RANK_LAUNCH(false, false);
  }
#undef HGIN_RANK_LAUNCH
  return check_launch(what);
}

}  // namespace

extern "C" int hgin_link_full_rank_f32(const int64_t* pos, int64_t n_pos, int64_t n_src, int64_t n_dst,
                                       const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                       int64_t F, const int32_t* known_rowptr, const int32_t* known_col,
                                       int32_t* n_greater, int32_t* n_equal, int32_t* n_cand, void* ws,
                                       size_t ws_bytes, void* stream) {
  return full_rank_impl("hgin_link_full_rank_f32", pos, n_pos, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F,
                        known_rowptr, known_col, n_greater, n_equal, n_cand, ws, ws_bytes, nullptr, nullptr, 0, stream);
}

extern "C" int hgin_link_full_rank_seg_f32(const int64_t* pos, int64_t n_pos, int64_t n_src, int64_t n_dst,
                                           const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                           int64_t F, const int32_t* known_rowptr, const int32_t* known_col,
                                           int32_t* n_greater, int32_t* n_equal, int32_t* n_cand, void* ws,
                                           size_t ws_bytes, const int32_t* src_seg, const int32_t* dst_ptr,
                                           int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_full_rank_seg_f32";
  HGIN_ARG_CHECK(n_graphs >= 1 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [1, 2^31)", what,
                 (long long)n_graphs);
  HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
  HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  return full_rank_impl(what, pos, n_pos, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, known_rowptr, known_col,
                        n_greater, n_equal, n_cand, ws, ws_bytes, src_seg, dst_ptr, (int)n_graphs, stream);
}
