// A22 — neighbour-sampled mini-batches for the link head (include/hgin.h A22).
//
// NOT IN REFERENCE: the reference trains on whole graphs.  The rule is build-defined and a pure function of
// (seed, offset, r_slot, v): Floyd's subset algorithm on Philox4x32-10 words whose counter word two is 2.
//
// Five entry points, all plain launches (no workgroup waits on another):
//   offsets: (1) k_nbr_count, 256 frontier nodes per workgroup: cnt = min(d, f) (d when f = -1), an exclusive scan of
//            the tile in LDS, the tile sum to the workspace; (2) k_nbr_scan, ONE workgroup scans the tile sums with a
//            running carry and writes the total; (3) k_nbr_add adds each tile's offset.
//   sample:  a lane group of W lanes per frontier node (W = 8 for f <= 8, 16 for f <= 32, else 64; a lane keeps at most
//            two picks, in registers).  The group's lead lane reads the row bounds once.  Lane b evaluates Philox block b
//            (at most f / 4 <= W blocks), Floyd's f steps run in lockstep with the membership test as one ballot, the
//            ascending order comes from a rank count over the group's picks: O(f^2 / W) per node whatever d is.  Rows
//            with d <= f (and f = -1) are copied, W positions per round.
//   fresh:   out[j] = src[j] when the node map holds no local row for it, else the sentinel (the candidates of a hop).
//   map_set: map[ids[i]] = base + i (base >= 0) or -1 (base < 0: the clean-up).
//   emit:    (map_src[src[j]], dst_base + the frontier slot whose offset range holds j), a binary search per edge.
// A25 adds offsets_excl / sample_excl: the same rule over the positions of a row whose (destination, source) key is not
// in a sorted excluded set (k_nbr_count_excl, k_nbr_sample_excl below); the A22 kernels are not touched.
#include "hgin_common.h"
#include "hgin_philox.h"

namespace hgin {
namespace {

constexpr int kNbrThreads = 256;
constexpr int kNbrMaxFanout = 128;
constexpr int64_t kNbrMaxRows = (int64_t)1 << 31;
constexpr int64_t kNbrMaxGrid = 16384;
constexpr int kNbrScanThreads = 1024;

inline unsigned nbr_grid(int64_t items) {
  const int64_t g = ceil_div(items, kNbrThreads);
  return (unsigned)(g < 1 ? 1 : (g < kNbrMaxGrid ? g : kNbrMaxGrid));
}

// ---- offsets ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNbrThreads) void k_nbr_count(const int32_t* __restrict__ rowptr, int64_t n_rows,
                                                           const int64_t* __restrict__ frontier, int64_t n, int f,
                                                           int64_t* __restrict__ off, int64_t* __restrict__ tile_sum,
                                                           int64_t n_tiles) {
  constexpr int kWaves = kNbrThreads / kWave;
  __shared__ int64_t wsum[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i = tile * kNbrThreads + t;
    int64_t c = 0;
    if (i < n) {
      const int64_t v = frontier[i];
      if (v >= 0 && v < n_rows) {
        const int64_t d = (int64_t)rowptr[v + 1] - (int64_t)rowptr[v];
        c = d < 0 ? 0 : ((f < 0 || d <= f) ? d : (int64_t)f);
      }
    }
    int64_t inc = c;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int64_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int64_t s = wsum[k];
      before += k < w ? s : 0;
      total += s;
    }
    if (i < n) off[i] = before + inc - c;
    if (t == 0) tile_sum[tile] = total;
    __syncthreads();   // wsum is rewritten by the next tile
  }
}

// exclusive scan of the tile sums, in place, by ONE workgroup; total -> *out_total
__global__ __launch_bounds__(kNbrScanThreads) void k_nbr_scan(int64_t* __restrict__ tile_sum, int64_t n_tiles,
                                                              int64_t* __restrict__ out_total) {
  constexpr int kWaves = kNbrScanThreads / kWave;
  __shared__ int64_t wsum[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kNbrScanThreads) {
    const int64_t i = base + t;
    const int64_t own = i < n_tiles ? tile_sum[i] : 0;
    int64_t inc = own;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int64_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int64_t s = wsum[k];
      before += k < w ? s : 0;
      total += s;
    }
    if (i < n_tiles) tile_sum[i] = carry + before + inc - own;
    carry += total;
    __syncthreads();   // wsum is rewritten by the next pass
  }
  if (t == 0) *out_total = carry;
}

__global__ __launch_bounds__(kNbrThreads) void k_nbr_add(int64_t* __restrict__ off, int64_t n,
                                                         const int64_t* __restrict__ tile_off) {
  for (int64_t i = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNbrThreads)
    off[i] += tile_off[i / kNbrThreads];
}

// ---- sample ----------------------------------------------------------------------------------------------------------
// W lanes per frontier node, kSlots picks per lane: pick i lives in lane i % W, slot i / W (W * kSlots >= f).
template <int W, int kSlots>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_sample(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ perm, int64_t n_rows,
                                                            const int64_t* __restrict__ frontier, int64_t n, int f,
                                                            uint32_t k0, uint32_t k1, uint32_t offset,
                                                            uint32_t slot_base, const int64_t* __restrict__ off,
                                                            int64_t* __restrict__ out_src,
                                                            int64_t* __restrict__ out_eid, int64_t n_out) {
  constexpr int kGroups = kNbrThreads / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int gl = threadIdx.x & (W - 1);                 // lane inside the group
  const int gbase = lane & ~(W - 1);                    // first wave lane of the group
  const uint64_t gmask = (~(uint64_t)0 >> (64 - W)) << gbase;
  const int64_t n_pad = (n + kGroups - 1) / kGroups * kGroups;   // every lane of a wave runs the same trip count
  for (int64_t i = (int64_t)blockIdx.x * kGroups + threadIdx.x / W; i < n_pad; i += (int64_t)gridDim.x * kGroups) {
    // the lead lane reads the node and its row bounds once
    int64_t v = -1, base = 0;
    int32_t r0 = 0, r1 = 0;
    if (gl == 0 && i < n) {
      v = frontier[i];
      if (v >= 0 && v < n_rows) {
        r0 = rowptr[v];
        r1 = rowptr[v + 1];
        base = off[i];
      } else {
        v = -1;
      }
    }
    v = __shfl(v, gbase, kWave);
    r0 = __shfl(r0, gbase, kWave);
    r1 = __shfl(r1, gbase, kWave);
    base = __shfl(base, gbase, kWave);
    const int64_t d = v < 0 ? 0 : (r1 > r0 ? (int64_t)r1 - r0 : 0);
    const bool floyd = f > 0 && d > f;
    if (!floyd) {
      for (int64_t p = gl; p < d; p += W) {
        const int64_t o = base + p;
        if (o < n_out) {
          out_src[o] = (int64_t)col[r0 + p];
          out_eid[o] = (int64_t)perm[r0 + p];
        }
      }
    }
    if (__ballot(floyd) == 0) continue;   // wave-uniform
    // Philox block gl of this node (blocks 0 .. (f - 1) / 4 are used; f <= 4 W)
    const U4 blk = philox4x32_10(U4{(uint32_t)v, offset, 2u, slot_base + (uint32_t)gl}, k0, k1);
    uint32_t pick[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) pick[s] = 0xffffffffu;
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      for (int l = 0; l < W; ++l) {
        const int idx = s * W + l;
        if (idx >= f) break;   // f is uniform over the launch
        const int wsel = idx & 3;
        const uint32_t mine = wsel == 0 ? blk.x : (wsel == 1 ? blk.y : (wsel == 2 ? blk.z : blk.w));
        const uint32_t word = (uint32_t)__shfl((int)mine, gbase + (idx >> 2), kWave);
        const uint32_t J = (uint32_t)(d - f + idx);   // d < 2^31
        const uint32_t t = (uint32_t)(((uint64_t)word * ((uint64_t)J + 1u)) >> 32);
        bool hit = false;
#pragma unroll
        for (int q = 0; q < kSlots; ++q) hit = hit || (pick[q] == t);   // unset slots hold 0xffffffff > any t
        const bool taken = (__ballot(floyd && hit) & gmask) != 0;
        if (gl == l) pick[s] = taken ? J : t;
      }
    }
    // ascending CSR position: the rank of a pick is the number of smaller picks (they are distinct)
    uint32_t rank[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) rank[s] = 0;
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      for (int l = 0; l < W; ++l) {
        if (s * W + l >= f) break;
        const uint32_t other = (uint32_t)__shfl((int)pick[s], gbase + l, kWave);
#pragma unroll
        for (int q = 0; q < kSlots; ++q) rank[q] += other < pick[q] ? 1u : 0u;
      }
    }
    if (floyd) {
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (s * W + gl < f) {
          const int64_t o = base + rank[s];
          if (o < n_out) {
            out_src[o] = (int64_t)col[(int64_t)r0 + pick[s]];
            out_eid[o] = (int64_t)perm[(int64_t)r0 + pick[s]];
          }
        }
      }
    }
  }
}

// ---- A25: the same two steps with an excluded set ----------------------------------------------------------------------
// excl: ascending int64 keys v * 2^32 + u (repeats allowed).  A frontier node whose key range is empty takes the A22 path
// (no row read for the count, f positions for the picks).  A row with a non-empty range is swept by its whole wave, 64
// positions per round: a position is free when its key is not in the range (a binary search), the ballot of the free
// flags and its popcount prefix give d', the compaction slot of a copied row, or the CSR position of a picked rank.
// Every loop around a ballot or shuffle runs on wave-uniform values (ballot results and broadcasts).

// the first index in [lo, hi) whose key is >= key (hi when there is none)
__device__ __forceinline__ int64_t nbr_lower(const int64_t* __restrict__ excl, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (excl[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// [lo, hi) = the keys of destination v (sources lie in [0, 2^31), so v * 2^32 + 2^31 is above all of them)
__device__ __forceinline__ void nbr_key_range(const int64_t* __restrict__ excl, int64_t n_excl, int64_t v, int64_t& lo,
                                              int64_t& hi) {
  lo = nbr_lower(excl, 0, n_excl, v << 32);
  hi = nbr_lower(excl, lo, n_excl, (v << 32) | (int64_t)0x80000000);
}

__device__ __forceinline__ bool nbr_excluded(const int64_t* __restrict__ excl, int64_t lo, int64_t hi, int64_t key) {
  const int64_t at = nbr_lower(excl, lo, hi, key);
  return at < hi && excl[at] == key;
}

// free flag of position p0 + lane of a row (r0, d) of destination v, as a ballot; every argument but lane is wave-uniform
__device__ __forceinline__ uint64_t nbr_free_ballot(const int32_t* __restrict__ col, const int64_t* __restrict__ excl,
                                                    int64_t v, int32_t r0, int32_t d, int64_t lo, int64_t hi,
                                                    int64_t p0, int lane) {
  const int64_t p = p0 + lane;
  bool fr = false;
  if (p < d) fr = !nbr_excluded(excl, lo, hi, (v << 32) | (int64_t)(uint32_t)col[(int64_t)r0 + p]);
  return __ballot(fr);
}

// d' of a row, counted by the whole wave
__device__ __forceinline__ int32_t nbr_wave_free(const int32_t* __restrict__ col, const int64_t* __restrict__ excl,
                                                 int64_t v, int32_t r0, int32_t d, int64_t lo, int64_t hi, int lane) {
  int32_t cnt = 0;
  for (int64_t p0 = 0; p0 < d; p0 += kWave) cnt += __popcll(nbr_free_ballot(col, excl, v, r0, d, lo, hi, p0, lane));
  return cnt;
}

// the index of the n-th (from 0) set bit of m; n < popcount(m)
__device__ __forceinline__ int nbr_nth_bit(uint64_t m, int n) {
  int at = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll((m >> at) & (((uint64_t)1 << w) - 1));
    if (n >= c) {
      n -= c;
      at += w;
    }
  }
  return at;
}

// k_nbr_count with d' in the place of d: a lane finds its node's key range, then the wave sweeps the rows that have one
__global__ __launch_bounds__(kNbrThreads) void k_nbr_count_excl(const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col, int64_t n_rows,
                                                                const int64_t* __restrict__ frontier, int64_t n, int f,
                                                                const int64_t* __restrict__ excl, int64_t n_excl,
                                                                int64_t* __restrict__ off,
                                                                int64_t* __restrict__ tile_sum, int64_t n_tiles) {
  constexpr int kWaves = kNbrThreads / kWave;
  __shared__ int64_t wsum[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i = tile * kNbrThreads + t;
    int64_t v = -1, lo = 0, hi = 0;
    int32_t r0 = 0, d = 0;
    if (i < n) {
      v = frontier[i];
      if (v >= 0 && v < n_rows) {
        r0 = rowptr[v];
        const int32_t r1 = rowptr[v + 1];
        d = r1 > r0 ? r1 - r0 : 0;
        if (d > 0 && n_excl > 0 && col != nullptr) nbr_key_range(excl, n_excl, v, lo, hi);   // col NULL: no edges
      } else {
        v = -1;
      }
    }
    for (uint64_t m = __ballot(hi > lo); m != 0; m &= m - 1) {   // wave-uniform: one row with exclusions per turn
      const int l = __ffsll((unsigned long long)m) - 1;
      const int32_t cnt = nbr_wave_free(col, excl, __shfl(v, l, kWave), __shfl(r0, l, kWave), __shfl(d, l, kWave),
                                        __shfl(lo, l, kWave), __shfl(hi, l, kWave), lane);
      if (lane == l) d = cnt;
    }
    const int64_t c = (f < 0 || d <= f) ? (int64_t)d : (int64_t)f;
    int64_t inc = c;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int64_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int64_t s = wsum[k];
      before += k < w ? s : 0;
      total += s;
    }
    if (i < n) off[i] = before + inc - c;
    if (t == 0) tile_sum[tile] = total;
    __syncthreads();   // wsum is rewritten by the next tile
  }
}

// k_nbr_sample over the free positions of a row: lane groups, Philox blocks, Floyd steps and the rank count as there
template <int W, int kSlots>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_sample_excl(const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ col,
                                                                 const int32_t* __restrict__ perm, int64_t n_rows,
                                                                 const int64_t* __restrict__ frontier, int64_t n, int f,
                                                                 uint32_t k0, uint32_t k1, uint32_t offset,
                                                                 uint32_t slot_base, const int64_t* __restrict__ excl,
                                                                 int64_t n_excl, const int64_t* __restrict__ off,
                                                                 int64_t* __restrict__ out_src,
                                                                 int64_t* __restrict__ out_eid, int64_t n_out) {
  constexpr int kGroups = kNbrThreads / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int gl = threadIdx.x & (W - 1);                 // lane inside the group
  const int gbase = lane & ~(W - 1);                    // first wave lane of the group
  const uint64_t gmask = (~(uint64_t)0 >> (64 - W)) << gbase;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const int64_t n_pad = (n + kGroups - 1) / kGroups * kGroups;   // every lane of a wave runs the same trip count
  for (int64_t i = (int64_t)blockIdx.x * kGroups + threadIdx.x / W; i < n_pad; i += (int64_t)gridDim.x * kGroups) {
    // the lead lane reads the node, its row bounds and its key range once
    int64_t v = -1, base = 0, lo = 0, hi = 0;
    int32_t r0 = 0, r1 = 0;
    if (gl == 0 && i < n) {
      v = frontier[i];
      if (v >= 0 && v < n_rows) {
        r0 = rowptr[v];
        r1 = rowptr[v + 1];
        base = off[i];
        if (r1 > r0 && n_excl > 0) nbr_key_range(excl, n_excl, v, lo, hi);
      } else {
        v = -1;
      }
    }
    v = __shfl(v, gbase, kWave);
    r0 = __shfl(r0, gbase, kWave);
    r1 = __shfl(r1, gbase, kWave);
    base = __shfl(base, gbase, kWave);
    const int32_t d = v < 0 ? 0 : (r1 > r0 ? r1 - r0 : 0);
    const uint64_t xm = __ballot(hi > lo);            // the lead lanes of the rows with exclusions
    const bool swept = ((xm >> gbase) & 1) != 0;      // this group's row is one of them
    int32_t df = d;                                   // d'
    for (uint64_t m = xm; m != 0; m &= m - 1) {       // wave-uniform: the whole wave counts one such row per turn
      const int l = __ffsll((unsigned long long)m) - 1;
      const int32_t cnt = nbr_wave_free(col, excl, __shfl(v, l, kWave), __shfl(r0, l, kWave), __shfl(d, l, kWave),
                                        __shfl(lo, l, kWave), __shfl(hi, l, kWave), lane);
      if (gbase == l) df = cnt;
    }
    const bool floyd = f > 0 && df > f;
    if (!floyd && !swept) {
      for (int64_t p = gl; p < d; p += W) {
        const int64_t o = base + p;
        if (o < n_out) {
          out_src[o] = (int64_t)col[r0 + p];
          out_eid[o] = (int64_t)perm[r0 + p];
        }
      }
    }
    if (__ballot(floyd || swept) == 0) continue;   // wave-uniform
    uint32_t pick[kSlots], rank[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      pick[s] = 0xffffffffu;
      rank[s] = 0;
    }
    if (__ballot(floyd) != 0) {   // wave-uniform
      // Philox block gl of this node (blocks 0 .. (f - 1) / 4 are used; f <= 4 W)
      const U4 blk = philox4x32_10(U4{(uint32_t)v, offset, 2u, slot_base + (uint32_t)gl}, k0, k1);
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        for (int l = 0; l < W; ++l) {
          const int idx = s * W + l;
          if (idx >= f) break;   // f is uniform over the launch
          const int wsel = idx & 3;
          const uint32_t mine = wsel == 0 ? blk.x : (wsel == 1 ? blk.y : (wsel == 2 ? blk.z : blk.w));
          const uint32_t word = (uint32_t)__shfl((int)mine, gbase + (idx >> 2), kWave);
          const uint32_t J = (uint32_t)(df - f + idx);   // d' < 2^31
          const uint32_t t = (uint32_t)(((uint64_t)word * ((uint64_t)J + 1u)) >> 32);
          bool hit = false;
#pragma unroll
          for (int q = 0; q < kSlots; ++q) hit = hit || (pick[q] == t);   // unset slots hold 0xffffffff > any t
          const bool taken = (__ballot(floyd && hit) & gmask) != 0;
          if (gl == l) pick[s] = taken ? J : t;
        }
      }
      // ascending rank = ascending CSR position: the rank of a pick is the number of smaller picks (they are distinct)
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        for (int l = 0; l < W; ++l) {
          if (s * W + l >= f) break;
          const uint32_t other = (uint32_t)__shfl((int)pick[s], gbase + l, kWave);
#pragma unroll
          for (int q = 0; q < kSlots; ++q) rank[q] += other < pick[q] ? 1u : 0u;
        }
      }
    }
    // a picked rank t is CSR position q_t: pick itself on a row without exclusions
    uint32_t at[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) at[s] = pick[s];
    for (uint64_t m = xm; m != 0; m &= m - 1) {   // wave-uniform: the whole wave sweeps one row per turn
      const int l = __ffsll((unsigned long long)m) - 1;
      const int64_t bv = __shfl(v, l, kWave), blo = __shfl(lo, l, kWave), bhi = __shfl(hi, l, kWave);
      const int64_t bbase = __shfl(base, l, kWave);
      const int32_t br0 = __shfl(r0, l, kWave), bd = __shfl(d, l, kWave);
      const bool bfloyd = __shfl((int)floyd, l, kWave) != 0;
      int64_t run = 0;                             // free positions before this round
      for (int64_t p0 = 0; p0 < bd; p0 += kWave) {
        const uint64_t fb = nbr_free_ballot(col, excl, bv, br0, bd, blo, bhi, p0, lane);
        const int cnt = __popcll(fb);
        if (!bfloyd) {                             // copied row: the compaction slot is the popcount prefix
          if ((fb >> lane) & 1) {
            const int64_t o = bbase + run + __popcll(fb & below);
            if (o < n_out) {
              out_src[o] = (int64_t)col[(int64_t)br0 + p0 + lane];
              out_eid[o] = (int64_t)perm[(int64_t)br0 + p0 + lane];
            }
          }
        } else if (gbase == l) {                   // the row's own group: ranks run .. run + cnt - 1 lie in this round
#pragma unroll
          for (int s = 0; s < kSlots; ++s) {
            const int64_t rel = (int64_t)pick[s] - run;
            if (s * W + gl < f && rel >= 0 && rel < cnt) at[s] = (uint32_t)(p0 + nbr_nth_bit(fb, (int)rel));
          }
        }
        run += cnt;
      }
    }
    if (floyd) {
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (s * W + gl < f) {
          const int64_t o = base + rank[s];
          if (o < n_out) {
            out_src[o] = (int64_t)col[(int64_t)r0 + at[s]];
            out_eid[o] = (int64_t)perm[(int64_t)r0 + at[s]];
          }
        }
      }
    }
  }
}

// ---- fresh / map_set / emit ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNbrThreads) void k_nbr_fresh(const int32_t* __restrict__ map, int64_t n_nodes,
                                                           const int64_t* __restrict__ src, int64_t n,
                                                           int64_t sentinel, int64_t* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kNbrThreads) {
    const int64_t s = src[j];
    const bool in = s >= 0 && s < n_nodes;
    out[j] = (in && map[s] < 0) ? s : sentinel;
  }
}

__global__ __launch_bounds__(kNbrThreads) void k_nbr_map_set(int32_t* __restrict__ map, int64_t n_nodes,
                                                             const int64_t* __restrict__ ids, int64_t n,
                                                             int64_t base) {
  for (int64_t i = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNbrThreads) {
    const int64_t v = ids[i];
    if (v >= 0 && v < n_nodes) map[v] = base < 0 ? -1 : (int32_t)(base + i);
  }
}

__global__ __launch_bounds__(kNbrThreads) void k_nbr_emit(const int32_t* __restrict__ map_src, int64_t n_src_nodes,
                                                          const int64_t* __restrict__ src,
                                                          const int64_t* __restrict__ off, int64_t n_frontier,
                                                          int64_t dst_base, int64_t n_edges,
                                                          int64_t* __restrict__ out_src,
                                                          int64_t* __restrict__ out_dst) {
  for (int64_t j = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; j < n_edges;
       j += (int64_t)gridDim.x * kNbrThreads) {
    // the last frontier slot i with off[i] <= j (off[0] = 0 <= j; empty rows share an offset with their successor)
    int64_t lo = 0, hi = n_frontier - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (off[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const int64_t s = src[j];
    out_src[j] = (s >= 0 && s < n_src_nodes) ? (int64_t)map_src[s] : -1;
    out_dst[j] = dst_base + lo;
  }
}

inline size_t nbr_ws_bytes(int64_t n) { return align_up((size_t)(ceil_div(n, kNbrThreads) + 1) * sizeof(int64_t), 256); }

inline int nbr_fanout_ok(int f) { return f == -1 || (f >= 1 && f <= kNbrMaxFanout); }

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_neighbor_sample_workspace_size(int64_t n_frontier, size_t* bytes) {
  HGIN_ARG_CHECK(bytes != nullptr, "hgin_neighbor_sample_workspace_size: bytes NULL");
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows,
                 "hgin_neighbor_sample_workspace_size: n_frontier = %lld outside [0, 2^31)", (long long)n_frontier);
  *bytes = nbr_ws_bytes(n_frontier);
  return HGIN_OK;
}

extern "C" int hgin_neighbor_sample_offsets(const int32_t* rowptr, int64_t n_rows, const int64_t* frontier,
                                            int64_t n_frontier, int f, int64_t* off, void* ws, size_t ws_bytes,
                                            void* stream) {
  HGIN_ARG_CHECK(n_rows >= 0 && n_rows < kNbrMaxRows, "hgin_neighbor_sample_offsets: n_rows = %lld outside [0, 2^31)",
                 (long long)n_rows);
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows,
                 "hgin_neighbor_sample_offsets: n_frontier = %lld outside [0, 2^31)", (long long)n_frontier);
  HGIN_ARG_CHECK(nbr_fanout_ok(f), "hgin_neighbor_sample_offsets: f = %d (-1, or 1 .. %d)", f, kNbrMaxFanout);
  HGIN_ARG_CHECK(off != nullptr, "hgin_neighbor_sample_offsets: off NULL");
  if (n_frontier > 0) {
    HGIN_ARG_CHECK(rowptr != nullptr, "hgin_neighbor_sample_offsets: rowptr NULL");
    HGIN_ARG_CHECK(frontier != nullptr, "hgin_neighbor_sample_offsets: frontier NULL");
  }
  if (ws == nullptr || ws_bytes < nbr_ws_bytes(n_frontier)) {
    set_error("hgin_neighbor_sample_offsets: workspace NULL or too small (%zu bytes, need %zu)", ws_bytes,
              nbr_ws_bytes(n_frontier));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  int64_t* tile = reinterpret_cast<int64_t*>(ws);
  const int64_t n_tiles = ceil_div(n_frontier, kNbrThreads);
  if (n_tiles > 0) {
    HGIN_TRACE("k_nbr_count");
    k_nbr_count<<<(unsigned)(n_tiles < kNbrMaxGrid ? n_tiles : kNbrMaxGrid), kNbrThreads, 0, s>>>(
        rowptr, n_rows, frontier, n_frontier, f, off, tile, n_tiles);
    if (int rc = check_launch("hgin_neighbor_sample_offsets (count)")) return rc;
  }
  HGIN_TRACE("k_nbr_scan");
  k_nbr_scan<<<1, kNbrScanThreads, 0, s>>>(tile, n_tiles, off + n_frontier);
  if (int rc = check_launch("hgin_neighbor_sample_offsets (scan)")) return rc;
  if (n_tiles > 1) {
    HGIN_TRACE("k_nbr_add");
    k_nbr_add<<<nbr_grid(n_frontier), kNbrThreads, 0, s>>>(off, n_frontier, tile);
    if (int rc = check_launch("hgin_neighbor_sample_offsets (add)")) return rc;
  }
  return HGIN_OK;
}

extern "C" int hgin_neighbor_sample(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_rows,
                                    const int64_t* frontier, int64_t n_frontier, int f, uint64_t seed,
                                    uint32_t offset, int64_t r_slot, const int64_t* off, int64_t* out_src,
                                    int64_t* out_eid, int64_t n_out, void* stream) {
  HGIN_ARG_CHECK(n_rows >= 0 && n_rows < kNbrMaxRows, "hgin_neighbor_sample: n_rows = %lld outside [0, 2^31)",
                 (long long)n_rows);
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows, "hgin_neighbor_sample: n_frontier = %lld outside [0, 2^31)",
                 (long long)n_frontier);
  HGIN_ARG_CHECK(nbr_fanout_ok(f), "hgin_neighbor_sample: f = %d (-1, or 1 .. %d)", f, kNbrMaxFanout);
  HGIN_ARG_CHECK(r_slot >= 0 && r_slot < ((int64_t)1 << 26), "hgin_neighbor_sample: r_slot = %lld outside [0, 2^26)",
                 (long long)r_slot);
  HGIN_ARG_CHECK(n_out >= 0 && n_out < ((int64_t)1 << 40), "hgin_neighbor_sample: n_out = %lld outside [0, 2^40)",
                 (long long)n_out);
  HGIN_ARG_CHECK(f < 0 || n_out <= n_frontier * (int64_t)f,
                 "hgin_neighbor_sample: n_out = %lld above n_frontier * f = %lld", (long long)n_out,
                 (long long)(n_frontier * (int64_t)f));
  if (n_frontier == 0 || n_out == 0) return HGIN_OK;
  HGIN_ARG_CHECK(rowptr != nullptr, "hgin_neighbor_sample: rowptr NULL");
  HGIN_ARG_CHECK(col != nullptr, "hgin_neighbor_sample: col NULL");
  HGIN_ARG_CHECK(perm != nullptr, "hgin_neighbor_sample: perm NULL");
  HGIN_ARG_CHECK(frontier != nullptr, "hgin_neighbor_sample: frontier NULL");
  HGIN_ARG_CHECK(off != nullptr, "hgin_neighbor_sample: off NULL");
  HGIN_ARG_CHECK(out_src != nullptr, "hgin_neighbor_sample: out_src NULL");
  HGIN_ARG_CHECK(out_eid != nullptr, "hgin_neighbor_sample: out_eid NULL");
  hipStream_t s = as_stream(stream);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t slot_base = (uint32_t)(r_slot * 64);
  const int W = (f > 0 && f <= 8) ? 8 : ((f > 0 && f <= 32) ? 16 : 64);
  const int64_t groups = ceil_div(n_frontier, kNbrThreads / W);
  const unsigned grid = (unsigned)(groups < kNbrMaxGrid ? groups : kNbrMaxGrid);
  HGIN_TRACE("k_nbr_sample<%d>", W);
  if (W == 8)
    k_nbr_sample<8, 1><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1, offset,
                                                    slot_base, off, out_src, out_eid, n_out);
  else if (W == 16)
    k_nbr_sample<16, 2><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1,
                                                     offset, slot_base, off, out_src, out_eid, n_out);
  else
    k_nbr_sample<64, 2><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1,
                                                     offset, slot_base, off, out_src, out_eid, n_out);
  return check_launch("hgin_neighbor_sample");
}

extern "C" int hgin_neighbor_sample_offsets_excl(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                                                 const int64_t* frontier, int64_t n_frontier, int f,
                                                 const int64_t* excl, int64_t n_excl, int64_t* off, void* ws,
                                                 size_t ws_bytes, void* stream) {
  HGIN_ARG_CHECK(n_rows >= 0 && n_rows < kNbrMaxRows,
                 "hgin_neighbor_sample_offsets_excl: n_rows = %lld outside [0, 2^31)", (long long)n_rows);
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows,
                 "hgin_neighbor_sample_offsets_excl: n_frontier = %lld outside [0, 2^31)", (long long)n_frontier);
  HGIN_ARG_CHECK(nbr_fanout_ok(f), "hgin_neighbor_sample_offsets_excl: f = %d (-1, or 1 .. %d)", f, kNbrMaxFanout);
  HGIN_ARG_CHECK(n_excl >= 0 && n_excl < kNbrMaxRows,
                 "hgin_neighbor_sample_offsets_excl: n_excl = %lld outside [0, 2^31)", (long long)n_excl);
  HGIN_ARG_CHECK(excl != nullptr || n_excl == 0, "hgin_neighbor_sample_offsets_excl: excl NULL");
  HGIN_ARG_CHECK(off != nullptr, "hgin_neighbor_sample_offsets_excl: off NULL");
  if (n_frontier > 0) {
    HGIN_ARG_CHECK(rowptr != nullptr, "hgin_neighbor_sample_offsets_excl: rowptr NULL");
    HGIN_ARG_CHECK(frontier != nullptr, "hgin_neighbor_sample_offsets_excl: frontier NULL");
  }
  if (ws == nullptr || ws_bytes < nbr_ws_bytes(n_frontier)) {
    set_error("hgin_neighbor_sample_offsets_excl: workspace NULL or too small (%zu bytes, need %zu)", ws_bytes,
              nbr_ws_bytes(n_frontier));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  int64_t* tile = reinterpret_cast<int64_t*>(ws);
  const int64_t n_tiles = ceil_div(n_frontier, kNbrThreads);
  if (n_tiles > 0) {
    HGIN_TRACE("k_nbr_count_excl");
    k_nbr_count_excl<<<(unsigned)(n_tiles < kNbrMaxGrid ? n_tiles : kNbrMaxGrid), kNbrThreads, 0, s>>>(
        rowptr, col, n_rows, frontier, n_frontier, f, excl, n_excl, off, tile, n_tiles);
    if (int rc = check_launch("hgin_neighbor_sample_offsets_excl (count)")) return rc;
  }
  HGIN_TRACE("k_nbr_scan");
  k_nbr_scan<<<1, kNbrScanThreads, 0, s>>>(tile, n_tiles, off + n_frontier);
  if (int rc = check_launch("hgin_neighbor_sample_offsets_excl (scan)")) return rc;
  if (n_tiles > 1) {
    HGIN_TRACE("k_nbr_add");
    k_nbr_add<<<nbr_grid(n_frontier), kNbrThreads, 0, s>>>(off, n_frontier, tile);
    if (int rc = check_launch("hgin_neighbor_sample_offsets_excl (add)")) return rc;
  }
  return HGIN_OK;
}

extern "C" int hgin_neighbor_sample_excl(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_rows,
                                         const int64_t* frontier, int64_t n_frontier, int f, uint64_t seed,
                                         uint32_t offset, int64_t r_slot, const int64_t* excl, int64_t n_excl,
                                         const int64_t* off, int64_t* out_src, int64_t* out_eid, int64_t n_out,
                                         void* stream) {
  HGIN_ARG_CHECK(n_rows >= 0 && n_rows < kNbrMaxRows, "hgin_neighbor_sample_excl: n_rows = %lld outside [0, 2^31)",
                 (long long)n_rows);
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows,
                 "hgin_neighbor_sample_excl: n_frontier = %lld outside [0, 2^31)", (long long)n_frontier);
  HGIN_ARG_CHECK(nbr_fanout_ok(f), "hgin_neighbor_sample_excl: f = %d (-1, or 1 .. %d)", f, kNbrMaxFanout);
  HGIN_ARG_CHECK(r_slot >= 0 && r_slot < ((int64_t)1 << 26),
                 "hgin_neighbor_sample_excl: r_slot = %lld outside [0, 2^26)", (long long)r_slot);
  HGIN_ARG_CHECK(n_excl >= 0 && n_excl < kNbrMaxRows, "hgin_neighbor_sample_excl: n_excl = %lld outside [0, 2^31)",
                 (long long)n_excl);
  HGIN_ARG_CHECK(excl != nullptr || n_excl == 0, "hgin_neighbor_sample_excl: excl NULL");
  HGIN_ARG_CHECK(n_out >= 0 && n_out < ((int64_t)1 << 40), "hgin_neighbor_sample_excl: n_out = %lld outside [0, 2^40)",
                 (long long)n_out);
  HGIN_ARG_CHECK(f < 0 || n_out <= n_frontier * (int64_t)f,
                 "hgin_neighbor_sample_excl: n_out = %lld above n_frontier * f = %lld", (long long)n_out,
                 (long long)(n_frontier * (int64_t)f));
  if (n_frontier == 0 || n_out == 0) return HGIN_OK;
  HGIN_ARG_CHECK(rowptr != nullptr, "hgin_neighbor_sample_excl: rowptr NULL");
  HGIN_ARG_CHECK(col != nullptr, "hgin_neighbor_sample_excl: col NULL");
  HGIN_ARG_CHECK(perm != nullptr, "hgin_neighbor_sample_excl: perm NULL");
  HGIN_ARG_CHECK(frontier != nullptr, "hgin_neighbor_sample_excl: frontier NULL");
  HGIN_ARG_CHECK(off != nullptr, "hgin_neighbor_sample_excl: off NULL");
  HGIN_ARG_CHECK(out_src != nullptr, "hgin_neighbor_sample_excl: out_src NULL");
  HGIN_ARG_CHECK(out_eid != nullptr, "hgin_neighbor_sample_excl: out_eid NULL");
  hipStream_t s = as_stream(stream);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t slot_base = (uint32_t)(r_slot * 64);
  const int W = (f > 0 && f <= 8) ? 8 : ((f > 0 && f <= 32) ? 16 : 64);
  const int64_t groups = ceil_div(n_frontier, kNbrThreads / W);
  const unsigned grid = (unsigned)(groups < kNbrMaxGrid ? groups : kNbrMaxGrid);
  HGIN_TRACE("k_nbr_sample_excl<%d>", W);
  if (W == 8)
    k_nbr_sample_excl<8, 1><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1,
                                                         offset, slot_base, excl, n_excl, off, out_src, out_eid, n_out);
  else if (W == 16)
    k_nbr_sample_excl<16, 2><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1,
                                                          offset, slot_base, excl, n_excl, off, out_src, out_eid,
                                                          n_out);
  else
    k_nbr_sample_excl<64, 2><<<grid, kNbrThreads, 0, s>>>(rowptr, col, perm, n_rows, frontier, n_frontier, f, k0, k1,
                                                          offset, slot_base, excl, n_excl, off, out_src, out_eid,
                                                          n_out);
  return check_launch("hgin_neighbor_sample_excl");
}

extern "C" int hgin_neighbor_fresh(const int32_t* map, int64_t n_nodes, const int64_t* src, int64_t n,
                                   int64_t sentinel, int64_t* out, void* stream) {
  HGIN_ARG_CHECK(n_nodes >= 0 && n_nodes < kNbrMaxRows, "hgin_neighbor_fresh: n_nodes = %lld outside [0, 2^31)",
                 (long long)n_nodes);
  HGIN_ARG_CHECK(n >= 0 && n < ((int64_t)1 << 40), "hgin_neighbor_fresh: n = %lld outside [0, 2^40)", (long long)n);
  if (n == 0) return HGIN_OK;
  HGIN_ARG_CHECK(map != nullptr || n_nodes == 0, "hgin_neighbor_fresh: map NULL");
  HGIN_ARG_CHECK(src != nullptr, "hgin_neighbor_fresh: src NULL");
  HGIN_ARG_CHECK(out != nullptr, "hgin_neighbor_fresh: out NULL");
  HGIN_TRACE("k_nbr_fresh");
  k_nbr_fresh<<<nbr_grid(n), kNbrThreads, 0, as_stream(stream)>>>(map, n_nodes, src, n, sentinel, out);
  return check_launch("hgin_neighbor_fresh");
}

extern "C" int hgin_neighbor_map_set(int32_t* map, int64_t n_nodes, const int64_t* ids, int64_t n, int64_t base,
                                     void* stream) {
  HGIN_ARG_CHECK(n_nodes >= 0 && n_nodes < kNbrMaxRows, "hgin_neighbor_map_set: n_nodes = %lld outside [0, 2^31)",
                 (long long)n_nodes);
  HGIN_ARG_CHECK(n >= 0 && n < kNbrMaxRows, "hgin_neighbor_map_set: n = %lld outside [0, 2^31)", (long long)n);
  HGIN_ARG_CHECK(base < 0 || base + n <= kNbrMaxRows, "hgin_neighbor_map_set: base + n = %lld above 2^31",
                 (long long)(base + n));
  if (n == 0) return HGIN_OK;
  HGIN_ARG_CHECK(map != nullptr, "hgin_neighbor_map_set: map NULL");
  HGIN_ARG_CHECK(ids != nullptr, "hgin_neighbor_map_set: ids NULL");
  HGIN_TRACE("k_nbr_map_set");
  k_nbr_map_set<<<nbr_grid(n), kNbrThreads, 0, as_stream(stream)>>>(map, n_nodes, ids, n, base);
  return check_launch("hgin_neighbor_map_set");
}

extern "C" int hgin_neighbor_emit(const int32_t* map_src, int64_t n_src_nodes, const int64_t* src, const int64_t* off,
                                  int64_t n_frontier, int64_t dst_base, int64_t n_edges, int64_t* out_edge,
                                  void* stream) {
  HGIN_ARG_CHECK(n_src_nodes >= 0 && n_src_nodes < kNbrMaxRows,
                 "hgin_neighbor_emit: n_src_nodes = %lld outside [0, 2^31)", (long long)n_src_nodes);
  HGIN_ARG_CHECK(n_frontier >= 0 && n_frontier < kNbrMaxRows, "hgin_neighbor_emit: n_frontier = %lld outside [0, 2^31)",
                 (long long)n_frontier);
  HGIN_ARG_CHECK(n_edges >= 0 && n_edges < ((int64_t)1 << 40), "hgin_neighbor_emit: n_edges = %lld outside [0, 2^40)",
                 (long long)n_edges);
  HGIN_ARG_CHECK(dst_base >= 0 && dst_base + n_frontier <= kNbrMaxRows,
                 "hgin_neighbor_emit: dst_base = %lld outside [0, 2^31 - n_frontier]", (long long)dst_base);
  if (n_edges == 0) return HGIN_OK;
  HGIN_ARG_CHECK(n_frontier >= 1, "hgin_neighbor_emit: %lld edges of an empty frontier", (long long)n_edges);
  HGIN_ARG_CHECK(map_src != nullptr, "hgin_neighbor_emit: map_src NULL");
  HGIN_ARG_CHECK(src != nullptr, "hgin_neighbor_emit: src NULL");
  HGIN_ARG_CHECK(off != nullptr, "hgin_neighbor_emit: off NULL");
  HGIN_ARG_CHECK(out_edge != nullptr, "hgin_neighbor_emit: out_edge NULL");
  HGIN_TRACE("k_nbr_emit");
  k_nbr_emit<<<nbr_grid(n_edges), kNbrThreads, 0, as_stream(stream)>>>(map_src, n_src_nodes, src, off, n_frontier,
                                                                       dst_base, n_edges, out_edge, out_edge + n_edges);
  return check_launch("hgin_neighbor_emit");
}
