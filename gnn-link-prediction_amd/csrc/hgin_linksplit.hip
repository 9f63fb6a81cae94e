// A21 — leakage-free train / valid / test edge splits (include/hgin.h A21).
//
// NOT IN REFERENCE: the reference regresses path delay and holds no edge out.  The rule is build-defined: the part of
// an edge is a function of its endpoint pair (one Philox4x32-10 evaluation, counter = {s, d, 1, 0}), so a pair, its
// flipped twin in the reverse relation and every copy of a multi-edge land in the same part without any join.
//
// Both entry points are memory-bound (16 B read per edge; 1 B written by the parts kernel, 24 B per kept edge by the
// selection) and share one geometry: tiles of kTileEdges = 256 threads x 8 edges.
//   parts:   edge j * 256 + t of the tile belongs to thread t in round j, so every wave-instruction covers 512
//            contiguous bytes of each edge row (one form serves every E: the second row starts at 8 E bytes, which is
//            16-byte aligned only for even E); a workgroup issues its next tile's loads before the current tile's
//            Philox rounds.  The part bytes go through LDS so that a full tile leaves as 8-byte stores.
//   select:  (1) k_split_count, one wave per tile, 32 part bytes per lane as two 16-byte loads; (2) k_split_scan, one
//            workgroup, kScanWidth tile counts per pass, running carry; (3) k_split_scatter, wave w of the workgroup
//            owns edges [512 w, 512 w + 512) of the tile in rounds of 64, so ballot order is input order and kept lanes
//            of a round store to consecutive output slots.  Three plain launches, no workgroup waits on another.
#include "hgin_common.h"
#include "hgin_philox.h"

namespace hgin {
namespace {

constexpr int kTileThreads = 256;
constexpr int kTileRounds = 8;
constexpr int kTileEdges = kTileThreads * kTileRounds;   // 2048
constexpr int kTileWaves = kTileThreads / kWave;         // 4
constexpr int kWaveEdges = kTileEdges / kTileWaves;      // 512 = kTileRounds * kWave
constexpr int kScanThreads = 1024;
constexpr int kScanWidth = 2 * kScanThreads;             // tile counts per scan pass
constexpr int64_t kMaxEdges = (int64_t)1 << 40;
constexpr int64_t kMaxGrid = 16384;
constexpr int64_t kPartsGrid = 256 * 4;                  // workgroups of the parts kernel: 4 per CU, each walks its tiles

__device__ __forceinline__ uint32_t split_part(uint32_t s, uint32_t d, uint32_t k0, uint32_t k1, uint64_t b_test,
                                               uint64_t b_val, uint64_t b_sup) {
  const U4 x = philox4x32_10(U4{s, d, 1u, 0u}, k0, k1);
  return (uint64_t)x.x < b_test ? 3u : ((uint64_t)x.x < b_val ? 2u : ((uint64_t)x.y < b_sup ? 1u : 0u));
}

// The low words of the tile's endpoints (only they enter the counter), thread t taking edge j * 256 + t in round j.
__device__ __forceinline__ void parts_load(const int64_t* __restrict__ row_s, const int64_t* __restrict__ row_d,
                                           int64_t E, int64_t tile, int t, uint32_t (&s)[kTileRounds],
                                           uint32_t (&d)[kTileRounds]) {
#pragma unroll
  for (int j = 0; j < kTileRounds; ++j) {
    const int64_t e = tile * kTileEdges + j * kTileThreads + t;
    const int64_t ec = e < E ? e : E - 1;   // E >= 1 here
    s[j] = (uint32_t)row_s[ec];
    d[j] = (uint32_t)row_d[ec];
  }
}

// A workgroup walks its tiles with the next tile's loads issued before the current tile's Philox rounds: the kernel
// has about as much integer-multiply time as memory time, and workgroups that load, compute and store in lockstep
// overlap neither (one tile per workgroup ran at 2.2 TB/s of the 17 B per edge).
__global__ __launch_bounds__(kTileThreads) void k_split_parts(const int64_t* __restrict__ row_s,
                                                              const int64_t* __restrict__ row_d, int64_t E,
                                                              int64_t n_tiles, uint64_t seed, uint64_t b_test,
                                                              uint64_t b_val, uint64_t b_sup,
                                                              uint8_t* __restrict__ part,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) uint8_t sp[kTileEdges];
  __shared__ uint32_t sh[4];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int t = threadIdx.x;
  if (t < 4) sh[t] = 0;
  __syncthreads();
  uint32_t c1 = 0, c2 = 0, c3 = 0, c_all = 0;
  const bool part8 = (reinterpret_cast<uintptr_t>(part) & 7u) == 0;
  uint32_t s[kTileRounds], d[kTileRounds], ns[kTileRounds], nd[kTileRounds];
  parts_load(row_s, row_d, E, blockIdx.x, t, s, d);   // the grid is at most n_tiles
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * kTileEdges;
    const bool more = tile + gridDim.x < n_tiles;
    if (more) parts_load(row_s, row_d, E, tile + gridDim.x, t, ns, nd);
#pragma unroll
    for (int j = 0; j < kTileRounds; ++j) {
      const bool in = base + j * kTileThreads + t < E;
      const uint32_t p = split_part(s[j], d[j], k0, k1, b_test, b_val, b_sup);
      sp[j * kTileThreads + t] = (uint8_t)p;
      c_all += in ? 1u : 0u;
      c1 += (in && p == 1u) ? 1u : 0u;
      c2 += (in && p == 2u) ? 1u : 0u;
      c3 += (in && p == 3u) ? 1u : 0u;
    }
    __syncthreads();
    if (part8 && base + kTileEdges <= E) {
      reinterpret_cast<uint2*>(part + base)[t] = reinterpret_cast<const uint2*>(sp)[t];
    } else {
#pragma unroll
      for (int j = 0; j < kTileRounds; ++j) {
        const int64_t e = base + j * kTileThreads + t;
        if (e < E) part[e] = sp[j * kTileThreads + t];
      }
    }
    __syncthreads();   // sp is rewritten by the next tile
    if (more) {
#pragma unroll
      for (int j = 0; j < kTileRounds; ++j) {
        s[j] = ns[j];
        d[j] = nd[j];
      }
    }
  }
  atomicAdd(&sh[0], c_all - c1 - c2 - c3);
  atomicAdd(&sh[1], c1);
  atomicAdd(&sh[2], c2);
  atomicAdd(&sh[3], c3);
  __syncthreads();
  if (t < 4 && sh[t] != 0) atomicAdd(&hist[t], (unsigned long long)sh[t]);
}

__device__ __forceinline__ uint32_t kept(uint32_t keep_mask, uint32_t p) { return (keep_mask >> (p & 3u)) & 1u; }

__device__ __forceinline__ uint32_t kept_in_word(uint32_t keep_mask, uint32_t w) {
  return kept(keep_mask, w) + kept(keep_mask, w >> 8) + kept(keep_mask, w >> 16) + kept(keep_mask, w >> 24);
}

// (1) one wave per tile: lane l counts part bytes [32 l, 32 l + 32) of the tile
__global__ __launch_bounds__(kTileThreads) void k_split_count(const uint8_t* __restrict__ part, int64_t E,
                                                              uint32_t keep_mask, int64_t n_tiles,
                                                              uint32_t* __restrict__ cnt) {
  static_assert(kTileEdges == kWave * 32, "a lane owns 32 part bytes of its wave's tile");
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const bool vec = (reinterpret_cast<uintptr_t>(part) & 15u) == 0;
  for (int64_t tile = (int64_t)blockIdx.x * kTileWaves + w; tile < n_tiles; tile += (int64_t)gridDim.x * kTileWaves) {
    const int64_t b0 = tile * kTileEdges + lane * 32;
    uint32_t c = 0;
    if (vec && b0 + 32 <= E) {
      const uint4 u = *reinterpret_cast<const uint4*>(part + b0);
      const uint4 v = *reinterpret_cast<const uint4*>(part + b0 + 16);
      c = kept_in_word(keep_mask, u.x) + kept_in_word(keep_mask, u.y) + kept_in_word(keep_mask, u.z) +
          kept_in_word(keep_mask, u.w) + kept_in_word(keep_mask, v.x) + kept_in_word(keep_mask, v.y) +
          kept_in_word(keep_mask, v.z) + kept_in_word(keep_mask, v.w);
    } else {
      for (int i = 0; i < 32; ++i)
        if (b0 + i < E) c += kept(keep_mask, part[b0 + i]);
    }
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) c += __shfl_xor(c, o, kWave);
    if (lane == 0) cnt[tile] = c;
  }
}

// (2) exclusive scan of the tile counts by ONE workgroup: kScanWidth counts per pass (two per thread), the passes chained
// by a carry every thread holds; off[n_tiles] = the total.
__global__ __launch_bounds__(kScanThreads) void k_split_scan(const uint32_t* __restrict__ cnt, int64_t n_tiles,
                                                             int64_t* __restrict__ off) {
  constexpr int kWaves = kScanThreads / kWave;
  __shared__ uint32_t wsum[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kScanWidth) {
    const int64_t i0 = base + 2 * t;
    const uint32_t a = i0 < n_tiles ? cnt[i0] : 0u;
    const uint32_t b = i0 + 1 < n_tiles ? cnt[i0 + 1] : 0u;
    const uint32_t own = a + b;
    uint32_t inc = own;   // at most kScanWidth * kTileEdges = 2^22 per pass
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const uint32_t v = wsum[k];
      before += k < w ? v : 0u;
      total += v;
    }
    const int64_t ex = carry + (int64_t)before + (int64_t)(inc - own);
    if (i0 < n_tiles) off[i0] = ex;
    if (i0 + 1 < n_tiles) off[i0 + 1] = ex + (int64_t)a;
    carry += (int64_t)total;
    __syncthreads();   // wsum is rewritten by the next pass
  }
  if (t == 0) off[n_tiles] = carry;
}

// (3) scatter: rank = tile offset + kept edges of the earlier waves (LDS) + of this wave's earlier rounds + of the lower
// lanes of this round (ballot).  A store is also guarded by n_out, which the host has checked against the scanned total.
__global__ __launch_bounds__(kTileThreads) void k_split_scatter(const int64_t* __restrict__ row0,
                                                                const int64_t* __restrict__ row1,
                                                                const uint8_t* __restrict__ part, int64_t E,
                                                                uint32_t keep_mask, const int64_t* __restrict__ off,
                                                                int64_t n_tiles, int64_t* __restrict__ out0,
                                                                int64_t* __restrict__ out1, int64_t* __restrict__ eid,
                                                                int64_t n_out) {
  __shared__ uint32_t wcnt[kTileWaves];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint64_t lower = ((uint64_t)1 << lane) - 1u;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t tile_off = off[tile];
    if (off[tile + 1] == tile_off) continue;   // nothing kept here (the same for the whole workgroup)
    const int64_t base = tile * kTileEdges + w * kWaveEdges + lane;
    int64_t a[kTileRounds], b[kTileRounds];
    uint64_t m[kTileRounds];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < kTileRounds; ++j) {
      const int64_t e = base + j * kWave;
      const int64_t ec = e < E ? e : E - 1;   // E >= 1 here
      const uint32_t p = part[ec];
      a[j] = row0[ec];
      b[j] = row1[ec];
      m[j] = __ballot(e < E && kept(keep_mask, p) != 0u);
      mine += (uint32_t)__popcll(m[j]);
    }
    if (lane == 0) wcnt[w] = mine;
    __syncthreads();
    int64_t pos = tile_off;
#pragma unroll
    for (int k = 0; k < kTileWaves; ++k) pos += k < w ? (int64_t)wcnt[k] : 0;
#pragma unroll
    for (int j = 0; j < kTileRounds; ++j) {
      const int64_t r = pos + (int64_t)__popcll(m[j] & lower);
      if (((m[j] >> lane) & 1u) && r < n_out) {
        out0[r] = a[j];
        out1[r] = b[j];
        eid[r] = base + j * kWave;
      }
      pos += (int64_t)__popcll(m[j]);
    }
    __syncthreads();   // wcnt is rewritten by the next tile
  }
}

inline int64_t split_tiles(int64_t E) { return ceil_div(E, kTileEdges); }
inline size_t split_cnt_bytes(int64_t n_tiles) { return align_up((size_t)n_tiles * sizeof(uint32_t), 256); }
inline size_t split_off_bytes(int64_t n_tiles) { return align_up((size_t)(n_tiles + 1) * sizeof(int64_t), 256); }

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_link_split_geometry(int* tile_edges, int* scan_width) {
  if (tile_edges != nullptr) *tile_edges = kTileEdges;
  if (scan_width != nullptr) *scan_width = kScanWidth;
  return HGIN_OK;
}

extern "C" int hgin_link_split_parts(const int64_t* edge_index, int64_t E, int swap, uint64_t seed, uint64_t b_test,
                                     uint64_t b_val, uint64_t b_sup, uint8_t* part, int64_t* hist, void* stream) {
  constexpr uint64_t kOne = (uint64_t)1 << 32;
  HGIN_ARG_CHECK(E >= 0 && E < kMaxEdges, "hgin_link_split_parts: E = %lld outside [0, 2^40)", (long long)E);
  HGIN_ARG_CHECK(swap == 0 || swap == 1, "hgin_link_split_parts: swap = %d (0 or 1)", swap);
  HGIN_ARG_CHECK(b_test <= kOne && b_val <= kOne && b_sup <= kOne, "hgin_link_split_parts: a bound above 2^32");
  HGIN_ARG_CHECK(b_test <= b_val, "hgin_link_split_parts: b_val < b_test");
  if (E == 0) return HGIN_OK;
  HGIN_ARG_CHECK(edge_index != nullptr, "hgin_link_split_parts: edge_index NULL");
  HGIN_ARG_CHECK(part != nullptr, "hgin_link_split_parts: part NULL");
  HGIN_ARG_CHECK(hist != nullptr, "hgin_link_split_parts: hist NULL");
  const int64_t n_tiles = split_tiles(E);
  const int64_t grid = n_tiles < kPartsGrid ? n_tiles : kPartsGrid;
  const int64_t* row_s = edge_index + (swap ? E : 0);
  const int64_t* row_d = edge_index + (swap ? 0 : E);
  HGIN_TRACE("k_split_parts");
  k_split_parts<<<(unsigned)grid, kTileThreads, 0, as_stream(stream)>>>(
      row_s, row_d, E, n_tiles, seed, b_test, b_val, b_sup, part, reinterpret_cast<unsigned long long*>(hist));
  return check_launch("hgin_link_split_parts");
}

extern "C" int hgin_link_split_select_workspace_size(int64_t E, size_t* bytes) {
  HGIN_ARG_CHECK(bytes != nullptr, "hgin_link_split_select_workspace_size: bytes NULL");
  HGIN_ARG_CHECK(E >= 0 && E < kMaxEdges, "hgin_link_split_select_workspace_size: E = %lld outside [0, 2^40)",
                 (long long)E);
  const int64_t n_tiles = split_tiles(E);
  *bytes = split_cnt_bytes(n_tiles) + split_off_bytes(n_tiles);
  return HGIN_OK;
}

extern "C" int hgin_link_split_select(const int64_t* edge_index, const uint8_t* part, int64_t E, int keep_mask,
                                      int64_t* out_edge, int64_t* out_eid, int64_t n_out, void* ws, size_t ws_bytes,
                                      void* stream) {
  HGIN_ARG_CHECK(E >= 0 && E < kMaxEdges, "hgin_link_split_select: E = %lld outside [0, 2^40)", (long long)E);
  HGIN_ARG_CHECK(keep_mask >= 0 && keep_mask <= 15, "hgin_link_split_select: keep_mask = %d outside [0, 15]",
                 keep_mask);
  HGIN_ARG_CHECK(n_out >= 0 && n_out <= E, "hgin_link_split_select: n_out = %lld outside [0, E = %lld]",
                 (long long)n_out, (long long)E);
  if (E == 0) return HGIN_OK;
  HGIN_ARG_CHECK(part != nullptr, "hgin_link_split_select: part NULL");
  if (n_out > 0) {
    HGIN_ARG_CHECK(edge_index != nullptr, "hgin_link_split_select: edge_index NULL");
    HGIN_ARG_CHECK(out_edge != nullptr, "hgin_link_split_select: out_edge NULL");
    HGIN_ARG_CHECK(out_eid != nullptr, "hgin_link_split_select: out_eid NULL");
  }
  const int64_t n_tiles = split_tiles(E);
  if (ws == nullptr || ws_bytes < split_cnt_bytes(n_tiles) + split_off_bytes(n_tiles)) {
    set_error("hgin_link_split_select: workspace NULL or too small (%zu bytes, need %zu)", ws_bytes,
              split_cnt_bytes(n_tiles) + split_off_bytes(n_tiles));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ws);
  int64_t* off = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ws) + split_cnt_bytes(n_tiles));
  const int64_t count_grid = ceil_div(n_tiles, kTileWaves);
  HGIN_TRACE("k_split_count");
  k_split_count<<<(unsigned)(count_grid < kMaxGrid ? count_grid : kMaxGrid), kTileThreads, 0, s>>>(
      part, E, (uint32_t)keep_mask, n_tiles, cnt);
  if (int rc = check_launch("hgin_link_split_select (count)")) return rc;
  HGIN_TRACE("k_split_scan");
  k_split_scan<<<1, kScanThreads, 0, s>>>(cnt, n_tiles, off);
  if (int rc = check_launch("hgin_link_split_select (scan)")) return rc;
  // the scanned total decides whether the scatter stays inside the outputs: read it before launching it
  int64_t total = -1;
  hipError_t e = hipMemcpyAsync(&total, off + n_tiles, sizeof(total), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_error("hgin_link_split_select: reading the scanned total failed: %s", hipGetErrorString(e));
    return static_cast<int>(e);
  }
  HGIN_ARG_CHECK(total == n_out, "hgin_link_split_select: n_out = %lld but the parts in keep_mask hold %lld edges",
                 (long long)n_out, (long long)total);
  if (n_out == 0) return HGIN_OK;
  HGIN_TRACE("k_split_scatter");
  k_split_scatter<<<(unsigned)(n_tiles < kMaxGrid ? n_tiles : kMaxGrid), kTileThreads, 0, s>>>(
      edge_index, edge_index + E, part, E, (uint32_t)keep_mask, off, n_tiles, out_edge, out_edge + n_out, out_eid,
      n_out);
  return check_launch("hgin_link_split_select (scatter)");
}
