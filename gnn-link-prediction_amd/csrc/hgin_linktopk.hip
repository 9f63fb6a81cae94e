// A16 — top-K link retrieval (include/hgin.h A16).
//
// NOT IN REFERENCE: like A13 .. A15 the spec is build-defined (header include/hgin.h) and checked against a float64
// restatement in tests/test_linktopk_host.py.
//
// The operation is the A15 sweep with a selecting epilogue in place of the counting one: score(q, c) =
// <z_src[src[q]], z_dst[c]> for every destination c, streamed through registers, never written.  Two kernels:
//   k_topk_sweep   k_rank_sweep's tiling and pipeline (128 gathered queries x 128-destination tiles through LDS, 4
//                  waves as 2 x 2, v_mfma_f32_32x32x2_f32, the K order of hgin_linkscore.h: the bits of A15).  Each
//                  lane keeps, per query column, a register threshold = the k-th best of a private sorted list of k
//                  (score, index) entries in the workspace; the hot epilogue is one compare per accumulator.  A wave
//                  leaves it only when some lane passes (__any): that lane drops destinations past n_dst and known
//                  neighbours of its source (binary search in the sorted CSR row), inserts into its list and reloads
//                  the threshold.
//   k_topk_merge   one wave per query: k rounds of a wave-wide argmax over the heads of the query's 4 * splits lists
//                  under (score descending, index ascending); pads with -1 / -inf.
// A list belongs to one (query, split, wave row wm, lane half lh) and is touched by one lane only: no atomics, nothing
// depends on timing.  That lane meets its destinations in ascending index order (tile, then MFMA block, then
// accumulator register), so among equal scores the earlier entry is the smaller index: a candidate is inserted behind
// every entry whose score is >= its own, and a candidate equal to a full list's k-th entry loses to it by index.
#include <climits>

#include "hgin_linkscore.h"

namespace hgin {
namespace {

constexpr int kTopkMaxK = 128;
constexpr int kTopkMaxLists = 4 * kRankTargetBlocks;   // splits <= kRankTargetBlocks

// one list entry: x = the score's bits, y = the destination
__device__ __forceinline__ float entry_score(const int2* e) { return __int_as_float(e->x); }

// ---- the sweep ----------------------------------------------------------------------------------------------------
// Geometry as k_rank_sweep (hgin_linkrank.hip): in an accumulator block lane (li, lh) of wave (wm, wn) holds query
// column li and the destination rows 8 (v / 4) + 4 lh + v % 4, v < 16.  List of (query q, split, wm, lh):
// lists + ((q * splits + split) * 4 + 2 wm + lh) * k, its fill count in counts at the same index.
// A19 (SEG): the workgroup's splits cut the tiles its queries' segments cover (a workgroup with an empty slice leaves
// at once: the host zeroed the counts), and the insertion path drops a destination outside its column's segment.
template <bool VEC, bool SEG>
__global__ __launch_bounds__(256, 2) void k_topk_sweep(const int64_t* __restrict__ src, int64_t Q, int64_t n_src,
                                                    int64_t n_dst, const float* __restrict__ zs, int64_t lds_,
                                                    const float* __restrict__ zd, int64_t ldd, int F,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, int k, int2* lists,
                                                    int32_t* __restrict__ counts, int64_t n_qblocks,
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
    if (t_beg >= t_end) return;   // never: sweep_plan leaves no empty split
  // this lane's query columns: threshold (-inf until the list is full; +inf for a column past Q, which never passes),
  // fill count, and the known row of the source
  float th[2];
  int cnt[2] = {0, 0}, kbeg[2] = {0, 0}, kdeg[2] = {0, 0};
  uint32_t slo[2] = {0u, 0u}, sn[2] = {0u, 0u};
  int64_t qcol[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    qcol[tn] = q0 + wn * 64 + tn * 32 + li;
    th[tn] = qcol[tn] < Q ? -INFINITY : INFINITY;
    if (rowptr != nullptr && qcol[tn] < Q) {
      const int64_t s = clamp_id(src[qcol[tn]], n_src);
      kbeg[tn] = rowptr[s];
      kdeg[tn] = rowptr[s + 1] - kbeg[tn];
    }
    if constexpr (SEG) {
      if (qcol[tn] < Q) seg_range(src_seg, dst_ptr, n_graphs, clamp_id(src[qcol[tn]], n_src), n_dst, slo[tn], sn[tn]);
      if (sn[tn] == 0u) th[tn] = INFINITY;   // a graph without destinations: nothing passes, the row stays padded
    }
  }
  if constexpr (SEG) {
    seg_tile_slice(slo, sn, split, splits, t_beg, t_end);
    if (t_beg >= t_end) return;   // block-uniform
  }

  // staging: thread (r = tid / 8, kq = tid % 8) moves features 4 kq .. 4 kq + 3 of rows r, r + 32, r + 64, r + 96;
  // rows past the end are clamped to the last one (loaded, never selected)
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  const float* qrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t q = q0 + lr + 32 * i < Q ? q0 + lr + 32 * i : Q - 1;
    qrow[i] = zs + clamp_id(src[q], n_src) * lds_;
  }

  // the cold path of one passing accumulator: candidate c with score x for query column tn
  auto offer = [&](int tn, float x, uint32_t c) {
    if (c >= (uint32_t)n_dst) return;   // a clamped row of the last tile
    if constexpr (SEG)
      if (c - slo[tn] >= sn[tn]) return;   // outside the query's graph (unsigned: slo <= c < slo + sn)
    int lo = 0, hi = kdeg[tn];
    while (lo < hi) {   // first known column >= c
      const int mid = (lo + hi) >> 1;
      if ((uint32_t)col[kbeg[tn] + mid] < c) lo = mid + 1;
      else hi = mid;
    }
    if (lo < kdeg[tn] && (uint32_t)col[kbeg[tn] + lo] == c) return;   // a known edge
    int2* e = lists + ((qcol[tn] * splits + split) * 4 + 2 * wm + lh) * k;
    const int n = cnt[tn];
    lo = 0, hi = n;
    while (lo < hi) {   // entries are sorted by score, descending: the first one below x
      const int mid = (lo + hi) >> 1;
      if (entry_score(e + mid) >= x) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= k) return;   // not better than a full list's last entry
    // entries lo .. j - 1 move up by one (a full list drops its last).  A tail walk that reads eight entries at a
    // time and needs no search was measured slower at k = 100 (cfg2 187 ms against 150) and 3 % faster at k = 10.
    int j = n < k ? n : k - 1;
    for (; j - lo >= 4; j -= 4) {
      const int2 v0 = e[j - 1], v1 = e[j - 2], v2 = e[j - 3], v3 = e[j - 4];
      e[j] = v0, e[j - 1] = v1, e[j - 2] = v2, e[j - 3] = v3;
    }
    for (; j > lo; --j) e[j] = e[j - 1];
    e[lo] = make_int2(__float_as_int(x), (int)c);
    if (n < k) cnt[tn] = n + 1;
    if (cnt[tn] == k) th[tn] = entry_score(e + k - 1);
  };

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
    // hot epilogue: does any accumulator beat its column's threshold?
    bool pass = false;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int v = 0; v < 16; ++v)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) pass |= acc[tm][tn][v] > th[tn];
    if (__any(pass)) {
      // cold: per column the passing accumulators in ascending destination order (tm, then v); the threshold may
      // rise while the block is walked, so each one is compared again before it is offered
      const uint32_t cbase = (uint32_t)(tile * kRankTile) + wm * 64 + 4 * lh;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
          uint32_t m = 0;
#pragma unroll
          for (int v = 0; v < 16; ++v) m |= (acc[tm][tn][v] > th[tn] ? 1u : 0u) << v;
          while (m) {
            const int v = __ffs(m) - 1;
            m &= m - 1;
            float x = acc[tm][tn][0];
#pragma unroll
            for (int e = 1; e < 16; ++e) x = v == e ? acc[tm][tn][e] : x;
            if (x > th[tn]) offer(tn, x, cbase + tm * 32 + 8 * (v >> 2) + (v & 3));
          }
        }
    }
  }
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
    if (qcol[tn] < Q) counts[(qcol[tn] * splits + split) * 4 + 2 * wm + lh] = cnt[tn];
}

// ---- the merge ------------------------------------------------------------------------------------------------------
// One wave per query.  Lane l owns the lists l, l + 64, ... of the query's L = 4 * splits and holds the best of their
// heads; a round takes the wave-wide best under (score descending, index ascending) — destinations are distinct
// across a query's lists, so exactly one lane owns it —, lane 0 writes it, the owner advances that list and looks at
// its heads again.  An exhausted lane holds (-inf, INT_MAX), which loses to every entry.
__device__ __forceinline__ bool topk_before(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

__global__ __launch_bounds__(64) void k_topk_merge(const int2* __restrict__ lists, const int32_t* __restrict__ counts,
                                                   int L, int k, int32_t* __restrict__ top_idx,
                                                   float* __restrict__ top_score) {
  __shared__ int head[kTopkMaxLists];   // entry l is touched by lane l % 64 only
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x, base = q * L;
  for (int l = lane; l < L; l += 64) head[l] = 0;
  float bs;
  int bi, bl;
  auto rescan = [&]() {
    bs = -INFINITY, bi = INT_MAX, bl = -1;
    for (int l = lane; l < L; l += 64) {
      const int h = head[l];
      if (h < counts[base + l]) {
        const int2 e = lists[(base + l) * k + h];
        if (topk_before(__int_as_float(e.x), e.y, bs, bi)) bs = __int_as_float(e.x), bi = e.y, bl = l;
      }
    }
  };
  rescan();
  for (int j = 0; j < k; ++j) {
    float s = bs;
    int i = bi;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float os = __shfl_xor(s, off, 64);
      const int oi = __shfl_xor(i, off, 64);
      if (topk_before(os, oi, s, i)) s = os, i = oi;
    }
    if (i == INT_MAX) {   // wave-uniform: every list is exhausted
      for (int t = j + lane; t < k; t += 64) {
        top_idx[q * k + t] = -1;
        top_score[q * k + t] = -INFINITY;
      }
      break;
    }
    if (lane == 0) {
      top_idx[q * k + j] = i;
      top_score[q * k + j] = s;
    }
    if (bi == i) {
      ++head[bl];
      rescan();
    }
  }
}

inline size_t topk_lists_bytes(int64_t n_query, int64_t splits, int64_t k) {
  return align_up((size_t)n_query * (size_t)(4 * splits) * (size_t)k * sizeof(int2), 256);
}
inline size_t topk_counts_bytes(int64_t n_query, int64_t splits) {
  return align_up((size_t)n_query * (size_t)(4 * splits) * sizeof(int32_t), 256);
}

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_link_topk_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, int64_t k, size_t* bytes) {
  const char* what = "hgin_link_topk_workspace_size";
  HGIN_ARG_CHECK(bytes != nullptr, "%s: bytes is NULL", what);
  HGIN_ARG_CHECK(n_query >= 1 && n_query < (int64_t(1) << 31), "%s: n_query = %lld must be in [1, 2^31)", what,
                 (long long)n_query);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(k >= 1 && k <= kTopkMaxK, "%s: k = %lld must be in [1, %d]", what, (long long)k, kTopkMaxK);
  const SweepPlan plan = sweep_plan(n_query, n_dst);
  *bytes = topk_lists_bytes(n_query, plan.splits, k) + topk_counts_bytes(n_query, plan.splits);
  return HGIN_OK;
}

namespace {

// A16 (src_seg = NULL) and A19 behind one set of checks and launches
int topk_impl(const char* what, const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
              int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, const int32_t* known_rowptr,
              const int32_t* known_col, int64_t k, int32_t* top_idx, float* top_score, void* ws, size_t ws_bytes,
              const int32_t* src_seg, const int32_t* dst_ptr, int n_graphs, void* stream) {
  const bool seg = src_seg != nullptr;
  const int64_t Q = n_query;
  HGIN_ARG_CHECK(Q >= 1 && Q < (int64_t(1) << 31), "%s: n_query = %lld must be in [1, 2^31)", what, (long long)Q);
  HGIN_ARG_CHECK(n_src >= 1 && n_src < (int64_t(1) << 31), "%s: n_src must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(k >= 1 && k <= kTopkMaxK, "%s: k = %lld must be in [1, %d]", what, (long long)k, kTopkMaxK);
  HGIN_ARG_CHECK(src != nullptr, "%s: src NULL", what);
  HGIN_ARG_CHECK(z_src != nullptr, "%s: z_src NULL", what);
  HGIN_ARG_CHECK(z_dst != nullptr, "%s: z_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "%s: leading dimension too small", what);
  HGIN_ARG_CHECK(known_rowptr == nullptr || known_col != nullptr, "%s: known_rowptr without known_col", what);
  HGIN_ARG_CHECK(top_idx != nullptr, "%s: top_idx NULL", what);
  HGIN_ARG_CHECK(top_score != nullptr, "%s: top_score NULL", what);
  const SweepPlan plan = sweep_plan(Q, n_dst);
  const size_t lists_bytes = topk_lists_bytes(Q, plan.splits, k);
  const size_t need = lists_bytes + topk_counts_bytes(Q, plan.splits);
  if (ws == nullptr || ws_bytes < need) {
    set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, need);
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  int2* lists = static_cast<int2*>(ws);
  int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + lists_bytes);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  const unsigned sweep_grid = (unsigned)(plan.n_qblocks * plan.splits);
  const int L = (int)(4 * plan.splits);   // <= kTopkMaxLists

  if (seg) {   // a workgroup whose slice of its graphs' tiles is empty writes no count
    const int rc = memset_async(counts, 0, topk_counts_bytes(Q, plan.splits), s, what);
    if (rc != HGIN_OK) return rc;
  }
  HGIN_TRACE("k_topk_sweep<%d%s> splits=%lld", vec ? 4 : 1, seg ? ",SEG" : "", (long long)plan.splits);
  HGIN_TRACE("k_topk_merge");
#define HGIN_TOPK_SWEEP(VEC_, SEG_)                                                                                 \
  k_topk_sweep<VEC_, SEG_><<<sweep_grid, 256, 0, s>>>(src, Q, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, (int)F,   \
                                                      known_rowptr, known_col, (int)k, lists, counts,               \
                                                      plan.n_qblocks, plan.tiles_per_split, plan.n_tiles,           \
                                                      plan.splits, src_seg, dst_ptr, n_graphs)
  if (seg) {
    if (vec) HGIN_TOPK_SWEEP(true, true);
    else HGIN_TOPK_SWEEP(false, true);
  } else {
    if (vec) HGIN_TOPK_SWEEP(true, false);
    else HGIN_TOPK_SWEEP(false, false);
  }
#undef HGIN_TOPK_SWEEP
  k_topk_merge<<<(unsigned)Q, 64, 0, s>>>(lists, counts, L, (int)k, top_idx, top_score);
  return check_launch(what);
}

}  // namespace

extern "C" int hgin_link_topk_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                  const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                  const int32_t* known_rowptr, const int32_t* known_col, int64_t k, int32_t* top_idx,
                                  float* top_score, void* ws, size_t ws_bytes, void* stream) {
  return topk_impl("hgin_link_topk_f32", src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, known_rowptr,
                   known_col, k, top_idx, top_score, ws, ws_bytes, nullptr, nullptr, 0, stream);
}

extern "C" int hgin_link_topk_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                      const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                      int64_t F, const int32_t* known_rowptr, const int32_t* known_col, int64_t k,
                                      int32_t* top_idx, float* top_score, void* ws, size_t ws_bytes,
                                      const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                                      void* stream) {
  const char* what = "hgin_link_topk_seg_f32";
  HGIN_ARG_CHECK(n_graphs >= 1 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [1, 2^31)", what,
                 (long long)n_graphs);
  HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
  HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  return topk_impl(what, src, n_query, n_src, n_dst, z_src, ld_src, z_dst, ld_dst, F, known_rowptr, known_col, k,
                   top_idx, top_score, ws, ws_bytes, src_seg, dst_ptr, (int)n_graphs, stream);
}
