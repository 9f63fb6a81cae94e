// A10 + A11 — negative-edge sampler and dot-product link decoder.
//
// NOT IN REFERENCE: the reference regresses path delay (models.py:362-376, train.py:38-44) and has no
// sampler or decoder; BASELINE.json's north star asks for both.  Their specs are build-defined (header
// include/hgin.h) and pinned by the C restatement in oracle/hgin_oracle.c plus Random123's published
// Philox4x32-10 known-answer vectors.
//
// Sampler: sample c = offset + i uses Philox4x32-10 block b = c >> 2, word c & 3, with
//   counter = {lo32(b), hi32(b), 0, 0}, key = {lo32(seed), hi32(seed)};  out = (word * n_dst) >> 32.
// One Philox evaluation feeds four samples; each thread writes its four int32 as one 16-byte store.
// Decoder forward: a G-lane group per scored pair, float4 per lane, group reduction by xor-shuffles.
// Decoder backward: g_z[row] = sum over the row's pairs, in pair order, of g[pair] * z_other[other]
// (mul then add, no FMA) — a weighted variant of the A3 segmented sum over a CSR of the pairs.
#include "hgin_common.h"
#include "hgin_philox.h"   // U4, philox4x32_10 (shared with hgin_linksplit.hip)

namespace hgin {
namespace {

__device__ __forceinline__ int32_t reduce_range(uint32_t x, uint32_t n) {
  return (int32_t)(((uint64_t)x * (uint64_t)n) >> 32);
}

__global__ __launch_bounds__(256) void k_neg_sample(uint64_t seed, uint64_t offset, int64_t n, uint32_t n_dst,
                                                    int32_t* __restrict__ out) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  // thread handles the four samples i in [4q - head, 4q - head + 4) aligned to Philox blocks
  const uint64_t first_block = offset >> 2;
  const uint64_t last_block = (offset + (uint64_t)n + 3) >> 2;  // exclusive
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; (uint64_t)q < last_block - first_block;
       q += stride) {
    const uint64_t b = first_block + (uint64_t)q;
    const U4 x = philox4x32_10(U4{(uint32_t)b, (uint32_t)(b >> 32), 0u, 0u}, k0, k1);
    const int32_t v[4] = {reduce_range(x.x, n_dst), reduce_range(x.y, n_dst), reduce_range(x.z, n_dst),
                          reduce_range(x.w, n_dst)};
    const int64_t i0 = (int64_t)(b * 4 - offset);  // index of word 0 in out (may be < 0 at the head)
    if (i0 >= 0 && i0 + 3 < n && ((reinterpret_cast<uintptr_t>(out + i0) & 15u) == 0)) {
      *reinterpret_cast<int4*>(out + i0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (i0 + w >= 0 && i0 + w < n) out[i0 + w] = v[w];
    }
  }
}

// A19: the segment of a source row: g = src_seg[s] clamped into [0, n_graphs), destinations [lo, lo + n) = dst_ptr[g],
// dst_ptr[g + 1].  One src_seg load and two dst_ptr loads.
__device__ __forceinline__ void seg_of(const int32_t* __restrict__ src_seg, const int32_t* __restrict__ dst_ptr,
                                       int n_graphs, int64_t s, uint32_t& lo, uint32_t& n) {
  int g = src_seg[s];
  g = g < 0 ? 0 : (g >= n_graphs ? n_graphs - 1 : g);
  const int32_t a = dst_ptr[g], b = dst_ptr[g + 1];
  lo = (uint32_t)a;
  n = b > a ? (uint32_t)(b - a) : 0u;
}

// A19 draw: lo + hi32(word * n), kept below n_dst (an empty last segment would otherwise name row n_dst)
__device__ __forceinline__ int32_t reduce_seg(uint32_t x, uint32_t lo, uint32_t n, uint32_t n_dst) {
  const uint32_t v = lo + (uint32_t)reduce_range(x, n);
  return (int32_t)(v < n_dst ? v : n_dst - 1);
}

// A19 sampler: one thread per draw i (positive i / k), counter offset + i as k_neg_sample's.
__global__ __launch_bounds__(256) void k_neg_sample_seg(uint64_t seed, uint64_t offset, const int64_t* __restrict__ src,
                                                        int64_t n, int k, const int32_t* __restrict__ src_seg,
                                                        const int32_t* __restrict__ dst_ptr, int n_graphs,
                                                        int32_t* __restrict__ out) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t n_dst = (uint32_t)dst_ptr[n_graphs];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t c = offset + (uint64_t)i;
    const uint64_t b = c >> 2;
    const U4 x = philox4x32_10(U4{(uint32_t)b, (uint32_t)(b >> 32), 0u, 0u}, k0, k1);
    uint32_t lo, cnt;
    seg_of(src_seg, dst_ptr, n_graphs, src[i / k], lo, cnt);
    const uint32_t w = (uint32_t)c & 3u;
    const uint32_t r = w == 0 ? x.x : (w == 1 ? x.y : (w == 2 ? x.z : x.w));
    out[i] = reduce_seg(r, lo, cnt, n_dst);
  }
}

// ---- A20: draws from a source's non-neighbours ---------------------------------------------------------------------
// first index in [b, e) whose column is >= v (e if none); reads col[b .. e) only and ends whatever the columns hold
__device__ __forceinline__ int32_t col_lower_bound(const int32_t* __restrict__ col, int32_t b, int32_t e, int64_t v) {
  while (b < e) {
    const int32_t mid = b + ((e - b) >> 1);
    if ((int64_t)col[mid] < v) b = mid + 1;
    else e = mid;
  }
  return b;
}

// The known row of source s clipped to its draw window [lo, lo + n): col[cb .. cb + d) are the row's columns inside the
// window, f = n - d the free destinations (0 when the row covers the window, or claims more than it holds).  s is
// clamped into [0, n_src) as seg_of clamps g; clip = false (one pool: the window is every destination) takes the row
// whole.  rowptr == NULL: no known edges.
__device__ __forceinline__ void filt_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                         int64_t n_src, int64_t s, bool clip, uint32_t lo, uint32_t n, int32_t& cb,
                                         int32_t& d, uint32_t& f) {
  cb = 0;
  d = 0;
  if (rowptr != nullptr) {
    s = s < 0 ? 0 : (s >= n_src ? n_src - 1 : s);
    const int32_t rb = rowptr[s];
    int32_t re = rowptr[s + 1];
    re = re < rb ? rb : re;
    cb = rb;
    int32_t ce = re;
    if (clip) {
      cb = col_lower_bound(col, rb, re, (int64_t)lo);
      ce = col_lower_bound(col, cb, re, (int64_t)lo + (int64_t)n);
    }
    d = ce - cb;
  }
  f = (uint32_t)d < n ? n - (uint32_t)d : 0u;
}

// N draws of one positive from Philox words w (slots with on[u] false are skipped and return 0).  f == 0: the
// unfiltered draw lo + hi32(w n).  Otherwise r = hi32(w f) and j = how many of the window's columns c_i have
// (c_i - lo) - i <= r (that sequence is non-decreasing, so a binary search over crow[0 .. d) finds it); the draw is
// lo + r + j, the r-th free destination.  The search's interval lengths do not depend on the data, so the N searches
// advance together and each step is one batch of independent loads; every index stays inside [0, d), and r + j < n
// whatever the columns hold.  The result is kept below n_dst as reduce_seg keeps it.
template <int N>
__device__ __forceinline__ void filt_draws(const uint32_t (&w)[N], const bool (&on)[N],
                                           const int32_t* __restrict__ crow, int32_t d, uint32_t f, uint32_t lo,
                                           uint32_t n, uint32_t n_dst, int32_t (&out)[N]) {
  if (f == 0u) {
#pragma unroll
    for (int u = 0; u < N; ++u) out[u] = on[u] ? reduce_seg(w[u], lo, n, n_dst) : 0;
    return;
  }
  uint32_t r[N];
  int32_t j[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    r[u] = (uint32_t)reduce_range(w[u], f);
    j[u] = 0;
  }
  int32_t len = d;
  while (len > 0) {
    const int32_t half = len > 1 ? len >> 1 : 1;   // probe j + half - 1; the last step (len == 1) probes j itself
    int32_t c[N];
#pragma unroll
    for (int u = 0; u < N; ++u) c[u] = on[u] ? crow[j[u] + half - 1] : 0;
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int64_t v = (int64_t)c[u] - (int64_t)lo - (int64_t)(j[u] + half - 1);
      if (on[u] && v <= (int64_t)r[u]) j[u] += half;
    }
    len -= half;
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const uint32_t v = lo + r[u] + (uint32_t)j[u];
    out[u] = on[u] ? (int32_t)(v < n_dst ? v : n_dst - 1) : 0;
  }
}

// A20 sampler: k_neg_sample_seg's thread-per-draw form; n_graphs == 0: one pool of n_dst destinations.
__global__ __launch_bounds__(256) void k_neg_sample_filt(uint64_t seed, uint64_t offset,
                                                         const int64_t* __restrict__ src, int64_t n, int k,
                                                         uint32_t n_dst, const int32_t* __restrict__ src_seg,
                                                         const int32_t* __restrict__ dst_ptr, int n_graphs,
                                                         int64_t n_src, const int32_t* __restrict__ known_rowptr,
                                                         const int32_t* __restrict__ known_col,
                                                         int32_t* __restrict__ out) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t c = offset + (uint64_t)i;
    const uint64_t b = c >> 2;
    const U4 x = philox4x32_10(U4{(uint32_t)b, (uint32_t)(b >> 32), 0u, 0u}, k0, k1);
    const int64_t s = src[i / k];
    uint32_t lo = 0u, cnt = n_dst;
    if (n_graphs > 0) seg_of(src_seg, dst_ptr, n_graphs, s, lo, cnt);
    int32_t cb, d;
    uint32_t f;
    filt_row(known_rowptr, known_col, n_src, s, n_graphs > 0, lo, cnt, cb, d, f);
    const uint32_t wsel = (uint32_t)c & 3u;
    const uint32_t w[1] = {wsel == 0 ? x.x : (wsel == 1 ? x.y : (wsel == 2 ? x.z : x.w))};
    const bool on[1] = {true};
    int32_t v[1];
    filt_draws<1>(w, on, known_col + cb, d, f, lo, cnt, n_dst, v);
    out[i] = v[0];
  }
}

template <int VEC, int G>
__global__ __launch_bounds__(256) void k_dot_fwd(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                 int64_t n_pairs, const float* __restrict__ zs, int64_t lds,
                                                 const float* __restrict__ zd, int64_t ldd, int F,
                                                 float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, gl = lane % G;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t e = wave_id * (64 / G) + grp;
  const bool valid = e < n_pairs;
  float acc = 0.0f;
  if (valid) {
    const float* a = zs + (int64_t)src[e] * lds;
    const float* b = zd + (int64_t)dst[e] * ldd;
    for (int f = gl * VEC; f < F; f += G * VEC) {
      if (VEC == 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + f);
        const float4 y = *reinterpret_cast<const float4*>(b + f);
        acc = __fadd_rn(acc, __fmul_rn(x.x, y.x));
        acc = __fadd_rn(acc, __fmul_rn(x.y, y.y));
        acc = __fadd_rn(acc, __fmul_rn(x.z, y.z));
        acc = __fadd_rn(acc, __fmul_rn(x.w, y.w));
      } else {
        acc = __fadd_rn(acc, __fmul_rn(a[f], b[f]));
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, G));
  if (valid && gl == 0) score[e] = acc;
}

template <int VEC, int G>
__global__ __launch_bounds__(256) void k_dot_bwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const int32_t* __restrict__ perm, int64_t n_rows,
                                                 const float* __restrict__ g, const float* __restrict__ zo,
                                                 int64_t ldo, int F, float* __restrict__ gz, int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, gl = lane % G;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r = wave_id * (64 / G) + grp;
  if (r >= n_rows) return;
  const int beg = rowptr[r], end = rowptr[r + 1];
  for (int f = gl * VEC; f < F; f += G * VEC) {
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
    for (int k = beg; k < end; ++k) {
      const float w = g[perm[k]];
      const float* p = zo + (int64_t)col[k] * ldo + f;
      if (VEC == 4) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        acc[0] = __fadd_rn(acc[0], __fmul_rn(w, x.x));
        acc[VEC > 1 ? 1 : 0] = __fadd_rn(acc[VEC > 1 ? 1 : 0], __fmul_rn(w, x.y));
        acc[VEC > 2 ? 2 : 0] = __fadd_rn(acc[VEC > 2 ? 2 : 0], __fmul_rn(w, x.z));
        acc[VEC > 3 ? 3 : 0] = __fadd_rn(acc[VEC > 3 ? 3 : 0], __fmul_rn(w, x.w));
      } else {
        acc[0] = __fadd_rn(acc[0], __fmul_rn(w, p[0]));
      }
    }
    float* o = gz + r * ldg + f;
    if (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[VEC > 1 ? 1 : 0], acc[VEC > 2 ? 2 : 0],
                                                              acc[VEC > 3 ? 3 : 0]);
    else o[0] = acc[0];
  }
}

// ---- A13 / A14: fused sampled link loss and ranking -------------------------------------------------------------
// One G-lane group per positive edge e.  The group holds the source row in registers (ONE: the row fits one VEC-wide
// piece per lane; otherwise the general loop re-reads it from cache), and scores pair t = 0 (the positive) and
// t = 1..k (the negatives, destination regenerated from Philox counter offset + e * k + t - 1) against it, kInFlight
// destination rows per batch so that several random-row loads are outstanding per wave.
constexpr int kInFlight = 4;
constexpr int kLinkMaxGrid = 4096;   // persistent grid: the per-block loss partials stay few and in a fixed order

template <int VEC>
__device__ __forceinline__ void ld_piece(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    v[0] = p[0];
  }
}

template <int VEC>
__device__ __forceinline__ float dot_piece(float acc, const float (&a)[VEC], const float (&b)[VEC]) {
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc = __fadd_rn(acc, __fmul_rn(a[c], b[c]));
  return acc;
}

// acc += w * x with Kahan's compensation (item order kept, mul / add / sub only, no FMA).  Both gradient kernels use
// it because a row's item count has no bound (few destinations, or a hub source owning thousands of positives:
// thousands of terms that largely cancel), where a plain fp32 running sum loses sqrt(n) eps of its largest partial sum.
template <int VEC>
__device__ __forceinline__ void axpy_comp_piece(float (&acc)[VEC], float (&comp)[VEC], float w, const float (&x)[VEC]) {
#pragma unroll
  for (int c = 0; c < VEC; ++c) {
    const float y = __fsub_rn(__fmul_rn(w, x[c]), comp[c]);
    const float t = __fadd_rn(acc[c], y);
    comp[c] = __fsub_rn(__fsub_rn(t, acc[c]), y);
    acc[c] = t;
  }
}

template <int VEC>
__device__ __forceinline__ void st_piece(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

__device__ __forceinline__ uint32_t word_of(const U4& x, uint32_t w) {
  return w == 0 ? x.x : (w == 1 ? x.y : (w == 2 ? x.z : x.w));
}

// A17: the objective of the loss epilogue (include/hgin.h HGIN_LINK_OBJ_*).  kObjBce is A13's finish_pair, untouched.
constexpr int kObjBce = 0, kObjSoftmax = 1, kObjBpr = 2, kObjSelfAdv = 3;

// sigmoid(x) and softplus(x) from the one exp(-|x|), as finish_pair forms them
__device__ __forceinline__ void sig_softplus(float x, float& sig, float& sp) {
  const float ex = expf(-fabsf(x));
  sig = (x >= 0.0f ? 1.0f : ex) / (1.0f + ex);
  sp = __fadd_rn(fmaxf(x, 0.0f), log1pf(ex));
}

// the softmax argument of a score: scale * s kept finite, so that max / subtract never meet inf - inf
__device__ __forceinline__ float soft_arg(float s, float scale) {
  return fminf(fmaxf(__fmul_rn(s, scale), -3.402823466e38f), 3.402823466e38f);
}

// Weights by objective (launch_link_fwd): bce w_pos = 0.5 / E, w_neg = 0.5 / (E k); softmax w_pos = 1 / E (loss),
// w_neg = 1 / (tau E) (coefficients), xscale = 1 / tau; bpr w_neg = 1 / (E k); selfadv w_pos = 0.5 / E, xscale = alpha.
//
// A18 (GIVEN): positive e has K = k + m negatives: pairs t = 1 .. k are the draws above (uniform count k, which may
// be 0: then no Philox block is computed), pairs t = k + 1 .. k + m take destination given[e * m + (t - k - 1)].
// K takes k's place everywhere else (slots, neg, normalisers, ranks); a batch that straddles the boundary clips its
// Philox window to its drawn pairs.  Without GIVEN, K = k and given / m are not read.
//
// A19 (SEG): a draw of positive e lands in the destinations of its source's graph, lo + hi32(word * n) in place of
// hi32(word * n_dst): one src_seg load and two dst_ptr loads per positive, nothing else differs.  Without SEG
// src_seg / dst_ptr / n_graphs are not read.
//
// A20 (FILT): a draw of positive e is the r-th destination of its window that is not a known neighbour of its source
// (filt_row once per positive, filt_draws per batch of drawn pairs; given pairs are not searched).  Instantiated in
// its GIVEN and SEG form only: m == 0 (no given pair) and n_graphs == 0 (one pool, src_seg / dst_ptr not read) are
// run-time cases.  Without FILT n_src / known_rowptr / known_col are not read.
template <int VEC, int G, bool ONE, bool RANK, int OBJ, bool GIVEN, bool SEG, bool FILT = false>
__global__ __launch_bounds__(256) void k_link_fwd(const int64_t* __restrict__ pos, int64_t E, int k, uint64_t seed,
                                                  uint64_t offset, uint32_t n_dst, const float* __restrict__ zs,
                                                  int64_t lds, const float* __restrict__ zd, int64_t ldd, int F,
                                                  float w_pos, float w_neg, float xscale, float* __restrict__ coef,
                                                  int64_t* __restrict__ neg, float* __restrict__ partial,
                                                  int32_t* __restrict__ n_gt, int32_t* __restrict__ n_eq,
                                                  const int32_t* __restrict__ given, int m,
                                                  const int32_t* __restrict__ src_seg,
                                                  const int32_t* __restrict__ dst_ptr, int n_graphs,
                                                  int64_t n_src, const int32_t* __restrict__ known_rowptr,
                                                  const int32_t* __restrict__ known_col) {
  static_assert(!FILT || (GIVEN && SEG), "the filtered kernel exists in its GIVEN and SEG form only");
  constexpr bool TWO_PHASE = !RANK && (OBJ == kObjSoftmax || OBJ == kObjSelfAdv);
  constexpr bool POS_IS_SUM = !RANK && (OBJ == kObjSoftmax || OBJ == kObjBpr);
  constexpr int EPW = 64 / G;   // edges per wave
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, gl = lane % G;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  const int K = GIVEN ? k + m : k;   // negatives per positive
  const int64_t nk = E * (int64_t)K;
  const bool lane_has = gl * VEC < F;   // ONE: this lane holds a piece of the row
  float lsum = 0.0f;
  for (int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wv * EPW < E; wv += n_waves) {
    const int64_t e_raw = wv * EPW + grp;
    const bool valid = e_raw < E;
    const int64_t e = valid ? e_raw : E - 1;   // idle groups redo the last edge (no divergence around the shuffles)
    const bool writer = valid && gl == 0;
    const int64_t d0 = pos[E + e];
    const int64_t s0 = pos[e];
    const float* a = zs + s0 * lds;
    uint32_t seg_lo = 0u, seg_n = n_dst;
    if constexpr (SEG) {
      if (!FILT || n_graphs > 0) seg_of(src_seg, dst_ptr, n_graphs, s0, seg_lo, seg_n);
    }
    // A20 state of this positive: its known row inside the window and the count of free destinations
    int32_t f_cb = 0, f_d = 0;
    uint32_t f_free = seg_n;
    if constexpr (FILT) filt_row(known_rowptr, known_col, n_src, s0, n_graphs > 0, seg_lo, seg_n, f_cb, f_d, f_free);
    // pair t's loss term, coefficient and (t >= 1) drawn pair; e = exp(-|s|) serves softplus and sigmoid alike
    auto finish_pair = [&](int t, float s, int64_t idm) {
      const float ex = expf(-fabsf(s));
      // sigmoid(s) for a negative, sigmoid(-s) = 1 - sigmoid(s) for the positive (no cancellation near 1)
      const float sig = ((s >= 0.0f) != (t == 0) ? 1.0f : ex) / (1.0f + ex);
      const float w = t == 0 ? w_pos : w_neg;
      const float sp = __fadd_rn(fmaxf(t == 0 ? -s : s, 0.0f), log1pf(ex));   // softplus(-s) / softplus(s)
      lsum = __fadd_rn(lsum, __fmul_rn(w, sp));
      if (t == 0) {
        coef[e] = __fmul_rn(w, -sig);
      } else {
        const int64_t q = e * (int64_t)K + (t - 1);
        coef[E + q] = __fmul_rn(w, sig);
        neg[q] = s0;
        neg[nk + q] = idm;
      }
    };
    float av[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) av[c] = 0.0f;
    if (ONE && lane_has) ld_piece<VEC>(a + gl * VEC, av);
    const uint64_t base = offset + (uint64_t)e * (uint64_t)k;
    float s_pos = 0.0f;
    int gt = 0, eq = 0;
    // A17 state of this positive: online (max, sum - 1) of the softmax arguments (softmax: pairs 0 .. k, selfadv: the
    // negatives), identical in every lane of the group, and this lane's sum of the negatives' coefficients
    float m_run = -INFINITY, S_run = 0.0f, c_neg = 0.0f;
    // A17, batch loop: bpr finishes negative t against s_pos; the two-phase objectives park the raw score in the
    // pair's coefficient slot (selfadv's positive is independent of the normaliser and is finished here, as bce's)
    auto first_pass = [&](int t, float s, int64_t idm) {
      if (t == 0) {
        if constexpr (OBJ == kObjSelfAdv) {
          float sig, sp;
          sig_softplus(-s, sig, sp);
          lsum = __fadd_rn(lsum, __fmul_rn(w_pos, sp));
          coef[e] = __fmul_rn(w_pos, -sig);
        }
        return;
      }
      const int64_t q = e * (int64_t)K + (t - 1);
      neg[q] = s0;
      neg[nk + q] = idm;
      if constexpr (OBJ == kObjBpr) {
        float sig, sp;
        sig_softplus(__fsub_rn(s, s_pos), sig, sp);
        lsum = __fadd_rn(lsum, __fmul_rn(w_neg, sp));
        const float c = __fmul_rn(w_neg, sig);
        coef[E + q] = c;
        c_neg = __fadd_rn(c_neg, c);
      } else {
        coef[E + q] = s;
      }
    };
    // A17, after the last batch: the lane that parked pair t's score reads it back and finishes the pair
    auto second_pass = [&](int t) {
      if (t == 0) {
        if constexpr (OBJ == kObjSoftmax)   // logsumexp - x_0 = (max - x_0) + log(1 + the other terms)
          lsum = __fadd_rn(lsum, __fmul_rn(w_pos, __fadd_rn(__fsub_rn(m_run, soft_arg(s_pos, xscale)),
                                                           log1pf(S_run))));
        return;
      }
      const int64_t q = e * (int64_t)K + (t - 1);
      const float s = coef[E + q];
      const float p = expf(__fsub_rn(soft_arg(s, xscale), m_run)) / __fadd_rn(1.0f, S_run);
      if constexpr (OBJ == kObjSoftmax) {
        const float c = __fmul_rn(w_neg, p);
        coef[E + q] = c;
        c_neg = __fadd_rn(c_neg, c);
      } else {
        float sig, sp;
        sig_softplus(s, sig, sp);
        const float wp = __fmul_rn(w_pos, p);
        lsum = __fadd_rn(lsum, __fmul_rn(wp, sp));
        coef[E + q] = __fmul_rn(wp, sig);
      }
    };
    // GIVEN: the given ids of a batch are loaded one batch ahead, so that the id -> row load chain of a given pair
    // (a drawn id comes out of the ALU) is not exposed in front of every batch's row gather
    int32_t g_pre[kInFlight];
    auto load_given = [&](int tb) {
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int t = tb + u;
        g_pre[u] = 0;
        if (t > k && t <= K) g_pre[u] = given[e * (int64_t)m + (t - k - 1)];
      }
    };
    if constexpr (GIVEN) load_given(0);
    for (int t0 = 0; t0 <= K; t0 += kInFlight) {
      int32_t g_cur[kInFlight];
      if constexpr (GIVEN) {
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) g_cur[u] = g_pre[u];
        if (t0 + kInFlight <= K) load_given(t0 + kInFlight);
      }
      // destination ids of pairs t0 .. t0 + 3: the counters of the drawn ones span at most two Philox blocks
      const int tf = t0 == 0 ? 1 : t0;                       // first negative of the batch (drawn iff tf <= k)
      const int tl = t0 + kInFlight - 1 < k ? t0 + kInFlight - 1 : k;   // last drawn pair of the batch
      uint64_t b0 = 0;
      U4 X = U4{0u, 0u, 0u, 0u}, Y = X;
      if (!GIVEN || tf <= k) {   // GIVEN: a batch of given pairs only (k = 0: every batch) draws nothing
        const uint64_t c_first = base + (uint64_t)(tf - 1);
        b0 = c_first >> 2;
        X = philox4x32_10(U4{(uint32_t)b0, (uint32_t)(b0 >> 32), 0u, 0u}, k0, k1);
        Y = X;
        if ((int)(c_first & 3) + (tl - tf) >= 4) {
          const uint64_t b1 = b0 + 1;
          Y = philox4x32_10(U4{(uint32_t)b1, (uint32_t)(b1 >> 32), 0u, 0u}, k0, k1);
        }
      }
      int64_t id[kInFlight];
      uint32_t f_w[kInFlight];   // FILT: the words of the batch's drawn pairs
      bool f_on[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int t = t0 + u;
        id[u] = d0;
        f_w[u] = 0u;
        f_on[u] = false;
        if (t >= 1 && t <= k) {
          const uint64_t c = base + (uint64_t)(t - 1);
          const uint32_t wx = word_of(X, (uint32_t)c & 3u), wy = word_of(Y, (uint32_t)c & 3u);
          const uint32_t r = (c >> 2) == b0 ? wx : wy;
          if constexpr (FILT) { f_w[u] = r; f_on[u] = true; }
          else if constexpr (SEG) id[u] = reduce_seg(r, seg_lo, seg_n, n_dst);
          else id[u] = reduce_range(r, n_dst);
        } else if (GIVEN && t > k && t <= K) {
          id[u] = g_cur[u];
        }
      }
      if constexpr (FILT) {
        if (tf <= k) {   // uniform: a batch of given pairs only searches nothing
          int32_t f_id[kInFlight];
          filt_draws<kInFlight>(f_w, f_on, known_col + f_cb, f_d, f_free, seg_lo, seg_n, n_dst, f_id);
#pragma unroll
          for (int u = 0; u < kInFlight; ++u)
            if (f_on[u]) id[u] = f_id[u];
        }
      }
      float sc[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) sc[u] = 0.0f;
      if (ONE) {
        float bv[kInFlight][VEC];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
          for (int c = 0; c < VEC; ++c) bv[u][c] = 0.0f;
          if (lane_has && t0 + u <= K) ld_piece<VEC>(zd + id[u] * ldd + gl * VEC, bv[u]);   // t0, K uniform
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) sc[u] = dot_piece<VEC>(sc[u], av, bv[u]);
      } else {
        for (int f = gl * VEC; f < F; f += G * VEC) {
          float x[VEC], bv[kInFlight][VEC];
          ld_piece<VEC>(a + f, x);
#pragma unroll
          for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) bv[u][c] = 0.0f;
            if (t0 + u <= K) ld_piece<VEC>(zd + id[u] * ldd + f, bv[u]);
          }
#pragma unroll
          for (int u = 0; u < kInFlight; ++u) sc[u] = dot_piece<VEC>(sc[u], x, bv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) sc[u] = __fadd_rn(sc[u], __shfl_xor(sc[u], off, G));
      }
      if constexpr (RANK) {
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          const int t = t0 + u;
          if (t == 0) s_pos = sc[u];
          else if (t <= K) { gt += sc[u] > s_pos; eq += sc[u] == s_pos; }
        }
      } else if constexpr (OBJ != kObjBce) {
        // after the shuffles every lane of the group holds the batch's four scores
        if (t0 == 0) s_pos = sc[0];
        if constexpr (TWO_PHASE) {
          // online normaliser, pairs in order; t0, K are uniform, so masked pairs (t > K) are skipped by all lanes
          // S_run leaves out the maximum's own term exp(0) = 1, so that log1p(S_run) keeps a loss far below 1.  One
          // exp per pair serves both cases: a new maximum turns the old one into a term and rescales by exp(m - x),
          // anything else adds exp(x - m).  First pair: m = -inf, (0 + 1) * exp(-inf) = 0.
          constexpr int T_MIN = OBJ == kObjSoftmax ? 0 : 1;
#pragma unroll
          for (int u = 0; u < kInFlight; ++u)
            if (t0 + u >= T_MIN && t0 + u <= K) {
              const float x = soft_arg(sc[u], xscale);
              const bool up = x > m_run;
              const float ex = expf(-fabsf(__fsub_rn(x, m_run)));
              S_run = up ? __fmul_rn(__fadd_rn(S_run, 1.0f), ex) : __fadd_rn(S_run, ex);
              m_run = up ? x : m_run;
            }
        }
        if constexpr (G >= kInFlight) {
          float s = sc[0];
          int64_t idm = id[0];
#pragma unroll
          for (int u = 1; u < kInFlight; ++u)
            if (gl == u) { s = sc[u]; idm = id[u]; }
          if (valid && gl < kInFlight && t0 + gl <= K) first_pass(t0 + gl, s, idm);
        } else {
#pragma unroll
          for (int u = 0; u < kInFlight; ++u)
            if (writer && t0 + u <= K) first_pass(t0 + u, sc[u], id[u]);
        }
      } else if constexpr (G >= kInFlight) {
        // every lane holds the four scores: lane u of the group finishes pair t0 + u (one exp / log1p per batch
        // instead of four in a row on lane 0, and the group's stores fall side by side)
        float s = sc[0];
        int64_t idm = id[0];
#pragma unroll
        for (int u = 1; u < kInFlight; ++u)
          if (gl == u) { s = sc[u]; idm = id[u]; }
        if (valid && gl < kInFlight && t0 + gl <= K) finish_pair(t0 + gl, s, idm);
      } else {
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
          if (writer && t0 + u <= K) finish_pair(t0 + u, sc[u], id[u]);
      }
    }
    if (RANK && writer) {
      n_gt[e] = gt;
      n_eq[e] = eq;
    }
    if constexpr (TWO_PHASE) {
      // the (t0, u) -> lane mapping of the batch loop again: every lane reads the slots it wrote itself
      if constexpr (G >= kInFlight) {
        if (valid && gl < kInFlight)
          for (int t = gl; t <= K; t += kInFlight) second_pass(t);
      } else {
        if (writer)
          for (int t = 0; t <= K; ++t) second_pass(t);
      }
    }
    if constexpr (POS_IS_SUM) {
      // the positive's coefficient = -(sum of its negatives' stored coefficients): lanes 0 .. 3 in order.  For softmax
      // that is (p_0 - 1) / (tau E) without the cancellation near p_0 = 1.
      float c = c_neg;
      if constexpr (G >= kInFlight) {
        c = __shfl(c_neg, 0, G);
#pragma unroll
        for (int u = 1; u < kInFlight; ++u) c = __fadd_rn(c, __shfl(c_neg, u, G));
      }
      if (writer) coef[e] = -c;
    }
  }
  if (!RANK) {
    // block partial in a fixed order: xor-tree inside the wave, then the four waves in order
    __shared__ float wsum[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lsum = __fadd_rn(lsum, __shfl_xor(lsum, off, 64));
    if (lane == 0) wsum[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0)
      partial[blockIdx.x] = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0], wsum[1]), wsum[2]), wsum[3]);
  }
}

// loss[0] = the partials added in a fixed order: thread i takes i, i + 256, ... in order, then a 256-wide tree
__global__ __launch_bounds__(256) void k_link_loss_sum(const float* __restrict__ partial, int n,
                                                       float* __restrict__ loss) {
  __shared__ float sh[256];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) acc = __fadd_rn(acc, partial[i]);
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] = __fadd_rn(sh[threadIdx.x], sh[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = sh[0];
}

// Source-side gradient: a group per source row over the static CSC of the positives (rowptr / col = dst / perm =
// edge id).  Items of the row in order: for each of its positives in CSC order, t = 0 (the positive's destination)
// then its k negatives; acc += (g * c) * z_dst[id], kInFlight rows loaded per batch, added in item order,
// compensated (Kahan) like the destination side: a hub source's deg (k + 1) items are as unbounded as a destination's.
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_link_bwd_src(const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col,
                                                      const int32_t* __restrict__ perm, int64_t n_rows, int64_t E,
                                                      int k, const float* __restrict__ g,
                                                      const float* __restrict__ coef,
                                                      const int64_t* __restrict__ neg_dst,
                                                      const float* __restrict__ zd, int64_t ldd, int F,
                                                      float* __restrict__ gz, int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, gl = lane % G;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r = wave_id * (64 / G) + grp;
  if (r >= n_rows) return;
  const float gv = g[0];
  const int beg = rowptr[r], end = rowptr[r + 1];
  const int64_t n_items = (int64_t)(end - beg) * (k + 1);
  for (int f = gl * VEC; f < F; f += G * VEC) {
    float acc[VEC], comp[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = comp[c] = 0.0f;
    int p = beg, t = 0;
    // ids and weights of items i .. i + 3, branch-free so that each level of the index chain (perm / col, then the
    // drawn id and the coefficient) is one batch of independent loads; items past the end repeat the last one
    auto fetch = [&](int64_t i, int64_t (&id)[kInFlight], float (&w)[kInFlight]) {
      int pu[kInFlight], tu[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        pu[u] = p;
        tu[u] = t;
        if (i + u < n_items - 1) {
          if (++t > k) { t = 0; ++p; }
        }
      }
      int32_t ev[kInFlight], cv[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        ev[u] = perm[pu[u]];
        cv[u] = col[pu[u]];
      }
      int64_t q[kInFlight], nd[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        q[u] = (int64_t)ev[u] * k + (tu[u] > 0 ? tu[u] - 1 : 0);
        nd[u] = neg_dst[q[u]];
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        w[u] = __fmul_rn(gv, coef[tu[u] == 0 ? (int64_t)ev[u] : E + q[u]]);
        id[u] = tu[u] == 0 ? (int64_t)cv[u] : nd[u];
      }
    };
    for (int64_t i = 0; i < n_items; i += kInFlight) {
      int64_t id[kInFlight];
      float w[kInFlight];
      fetch(i, id, w);
      float x[kInFlight][VEC];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) ld_piece<VEC>(zd + id[u] * ldd + f, x[u]);
#pragma unroll
      for (int u = 0; u < kInFlight; ++u)
        if (i + u < n_items) axpy_comp_piece<VEC>(acc, comp, w[u], x[u]);
    }
    st_piece<VEC>(gz + r * ldg + f, acc);
  }
}

// Destination-side gradient: a group per destination row; items in order: the row's positives (static CSR of pos:
// prow / pcol = src / pperm = edge id), then the row's negatives of this step (stable CSR of the drawn pairs by
// destination: nrow / ncol = src / nperm = index e * k + j); acc += (g * c) * z_src[src], compensated (Kahan).
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_link_bwd_dst(const int32_t* __restrict__ prow,
                                                      const int32_t* __restrict__ pcol,
                                                      const int32_t* __restrict__ pperm,
                                                      const int32_t* __restrict__ nrow,
                                                      const int32_t* __restrict__ ncol,
                                                      const int32_t* __restrict__ nperm, int64_t n_rows, int64_t E,
                                                      const float* __restrict__ g, const float* __restrict__ coef,
                                                      const float* __restrict__ zs, int64_t lds, int F,
                                                      float* __restrict__ gz, int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, gl = lane % G;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r = wave_id * (64 / G) + grp;
  if (r >= n_rows) return;
  const float gv = g[0];
  const int pbeg = prow[r], nbeg = nrow[r];
  const int n1 = prow[r + 1] - pbeg;
  const int64_t n_items = (int64_t)n1 + (nrow[r + 1] - nbeg);
  for (int f = gl * VEC; f < F; f += G * VEC) {
    float acc[VEC], comp[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = comp[c] = 0.0f;
    // ids and weights of items i .. i + 3, branch-free (the positive / negative arrays chosen by pointer selects)
    // so that the index loads of a batch are independent; items past the end repeat the last one
    auto fetch = [&](int64_t i, int64_t (&id)[kInFlight], float (&w)[kInFlight]) {
      int32_t pm[kInFlight];
      int64_t cb[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int64_t it = i + u < n_items ? i + u : n_items - 1;
        const bool is_pos = it < n1;
        const int32_t* cp = is_pos ? pcol : ncol;
        const int32_t* pp = is_pos ? pperm : nperm;
        const int64_t off = is_pos ? pbeg + it : nbeg + (it - n1);
        id[u] = cp[off];
        pm[u] = pp[off];
        cb[u] = is_pos ? 0 : E;
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) w[u] = __fmul_rn(gv, coef[cb[u] + pm[u]]);
    };
    for (int64_t i = 0; i < n_items; i += kInFlight) {
      int64_t id[kInFlight];
      float w[kInFlight];
      fetch(i, id, w);
      float x[kInFlight][VEC];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) ld_piece<VEC>(zs + id[u] * lds + f, x[u]);
#pragma unroll
      for (int u = 0; u < kInFlight; ++u)
        if (i + u < n_items) axpy_comp_piece<VEC>(acc, comp, w[u], x[u]);
    }
    st_piece<VEC>(gz + r * ldg + f, acc);
  }
}


int pick_g(int64_t lanes) {
  int g = 1;
  while (g < lanes && g < 64) g <<= 1;
  return g;
}

}  // namespace
}  // namespace hgin

using namespace hgin;

extern "C" int hgin_neg_sample(uint64_t seed, uint64_t offset, int64_t n, int64_t n_dst, int32_t* out, void* stream) {
  HGIN_ARG_CHECK(n >= 0, "hgin_neg_sample: n < 0");
  HGIN_ARG_CHECK(n_dst > 0 && n_dst <= 0x7fffffffLL, "hgin_neg_sample: n_dst must be in [1, 2^31)");
  if (n == 0) return HGIN_OK;
  HGIN_ARG_CHECK(out != nullptr, "hgin_neg_sample: out NULL");
  const uint64_t blocks = ((offset + (uint64_t)n + 3) >> 2) - (offset >> 2);
  const int64_t grid = ceil_div((int64_t)blocks, 256);
  k_neg_sample<<<(unsigned)(grid < 65536 ? grid : 65536), 256, 0, as_stream(stream)>>>(seed, offset, n,
                                                                                       (uint32_t)n_dst, out);
  return check_launch("hgin_neg_sample");
}

#define HGIN_G_SWITCH(G_RUNTIME, ...)        \
  switch (G_RUNTIME) {                       \
    case 1: { constexpr int G = 1; __VA_ARGS__; } break;   \
    case 2: { constexpr int G = 2; __VA_ARGS__; } break;   \
    case 4: { constexpr int G = 4; __VA_ARGS__; } break;   \
    case 8: { constexpr int G = 8; __VA_ARGS__; } break;   \
    case 16: { constexpr int G = 16; __VA_ARGS__; } break; \
    case 32: { constexpr int G = 32; __VA_ARGS__; } break; \
    default: { constexpr int G = 64; __VA_ARGS__; } break; \
  }

extern "C" int hgin_dot_decode_fwd_f32(const int32_t* src, const int32_t* dst, int64_t n_pairs, const float* z_src,
                                       int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float* score,
                                       void* stream) {
  HGIN_ARG_CHECK(n_pairs >= 0 && F >= 0 && F < (1 << 24), "hgin_dot_decode_fwd_f32: bad sizes");
  if (n_pairs == 0) return HGIN_OK;
  HGIN_ARG_CHECK(src && dst && score && (F == 0 || (z_src && z_dst)), "hgin_dot_decode_fwd_f32: NULL operand");
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "hgin_dot_decode_fwd_f32: leading dimension too small");
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  const int g = pick_g(vec ? ceil_div(F, 4) : F);
  const int64_t waves = ceil_div(n_pairs, 64 / g);
  const unsigned grid = (unsigned)ceil_div(waves, 4);
  if (vec) {
    HGIN_G_SWITCH(g, k_dot_fwd<4, G><<<grid, 256, 0, s>>>(src, dst, n_pairs, z_src, ld_src, z_dst, ld_dst, (int)F,
                                                          score))
  } else {
    HGIN_G_SWITCH(g, k_dot_fwd<1, G><<<grid, 256, 0, s>>>(src, dst, n_pairs, z_src, ld_src, z_dst, ld_dst, (int)F,
                                                          score))
  }
  return check_launch("hgin_dot_decode_fwd_f32");
}

extern "C" int hgin_dot_decode_bwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_rows,
                                       const float* g_score, const float* z_other, int64_t ld_other, int64_t F,
                                       float* g_z, int64_t ld_g, void* stream) {
  HGIN_ARG_CHECK(n_rows >= 0 && F >= 0 && F < (1 << 24), "hgin_dot_decode_bwd_f32: bad sizes");
  if (n_rows == 0 || F == 0) return HGIN_OK;
  HGIN_ARG_CHECK(rowptr && g_z, "hgin_dot_decode_bwd_f32: NULL operand");
  HGIN_ARG_CHECK(ld_other >= F && ld_g >= F, "hgin_dot_decode_bwd_f32: leading dimension too small");
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_other) && aligned16(g_z) && ld_other % 4 == 0 && ld_g % 4 == 0;
  const int g = pick_g(vec ? ceil_div(F, 4) : F);
  const int64_t waves = ceil_div(n_rows, 64 / g);
  const unsigned grid = (unsigned)ceil_div(waves, 4);
  if (vec) {
    HGIN_G_SWITCH(g, k_dot_bwd<4, G><<<grid, 256, 0, s>>>(rowptr, col, perm, n_rows, g_score, z_other, ld_other,
                                                          (int)F, g_z, ld_g))
  } else {
    HGIN_G_SWITCH(g, k_dot_bwd<1, G><<<grid, 256, 0, s>>>(rowptr, col, perm, n_rows, g_score, z_other, ld_other,
                                                          (int)F, g_z, ld_g))
  }
  return check_launch("hgin_dot_decode_bwd_f32");
}

// ---- A13 / A14 entry points ---------------------------------------------------------------------------------------
namespace {

struct LinkShape {
  bool vec;
  int g;
  bool one;
  unsigned grid;
};

LinkShape link_shape(int64_t E, int64_t F, const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst) {
  LinkShape s;
  s.vec = F % 4 == 0 && aligned16(z_src) && aligned16(z_dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  const int64_t pieces = s.vec ? F / 4 : F;
  s.one = pieces <= 64;
  s.g = s.one ? pick_g(pieces) : 64;
  const int64_t blocks = ceil_div(ceil_div(E, 64 / s.g), 4);
  s.grid = (unsigned)(blocks < kLinkMaxGrid ? blocks : kLinkMaxGrid);
  return s;
}

int link_common_checks(const char* what, const int64_t* pos, int64_t E, int64_t k, int64_t n_dst, const float* z_src,
                       int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F) {
  HGIN_ARG_CHECK(E >= 1 && E < (int64_t(1) << 31), "%s: E = %lld must be in [1, 2^31)", what, (long long)E);
  HGIN_ARG_CHECK(k >= 1 && k < (int64_t(1) << 31), "%s: k = %lld must be >= 1", what, (long long)k);
  HGIN_ARG_CHECK(E * k < (int64_t(1) << 31), "%s: E * k = %lld must be < 2^31", what, (long long)(E * k));
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(pos != nullptr, "%s: pos NULL", what);
  HGIN_ARG_CHECK(z_src != nullptr, "%s: z_src NULL", what);
  HGIN_ARG_CHECK(z_dst != nullptr, "%s: z_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "%s: leading dimension too small", what);
  return HGIN_OK;
}

// GIVEN (A18): k uniform draws + m given destinations per positive (given int32 [E, m]); otherwise m = 0.
template <bool RANK, int OBJ = kObjBce, bool GIVEN = false, bool SEG = false, bool FILT = false>
void launch_link_fwd(const LinkShape& sh, hipStream_t s, const int64_t* pos, int64_t E, int k, uint64_t seed,
                     uint64_t offset, uint32_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst,
                     int64_t ld_dst, int F, float* coef, int64_t* neg, float* partial, int32_t* n_gt, int32_t* n_eq,
                     float param = 0.0f, const int32_t* given = nullptr, int m = 0, const int32_t* src_seg = nullptr,
                     const int32_t* dst_ptr = nullptr, int n_graphs = 0, int64_t n_src = 0,
                     const int32_t* known_rowptr = nullptr, const int32_t* known_col = nullptr) {
  const int K = k + m;
  float w_pos = (float)(0.5 / (double)E), w_neg = (float)(0.5 / ((double)E * (double)K)), xscale = 0.0f;
  if (OBJ == kObjSoftmax) {
    w_pos = (float)(1.0 / (double)E);
    w_neg = (float)(1.0 / ((double)param * (double)E));
    xscale = (float)(1.0 / (double)param);
  } else if (OBJ == kObjBpr) {
    w_neg = (float)(1.0 / ((double)E * (double)K));
  } else if (OBJ == kObjSelfAdv) {
    xscale = param;
  }
  constexpr const char* kEpilogue[] = {"LOSS", "SOFTMAX", "BPR", "SELFADV"};
  // FILT is one instantiation (GIVEN, SEG): its tag names what the call uses of it, then ,FILT
  HGIN_TRACE("k_link_fwd<%d,%d,%s,%s%s%s%s>", sh.vec ? 4 : 1, sh.g, sh.one ? "ONE" : "LOOP",
             RANK ? "RANK" : kEpilogue[OBJ], GIVEN && (!FILT || m > 0) ? ",GIVEN" : "",
             SEG && (!FILT || n_graphs > 0) ? ",SEG" : "", FILT ? ",FILT" : "");
#define HGIN_LINK_FWD(VEC_, G_, ONE_)                                                                               \
  k_link_fwd<VEC_, G_, ONE_, RANK, OBJ, GIVEN, SEG, FILT><<<sh.grid, 256, 0, s>>>(                                   \
      pos, E, k, seed, offset, n_dst, z_src, ld_src, z_dst, ld_dst, F, w_pos, w_neg, xscale, coef, neg, partial, n_gt, \
      n_eq, given, m, src_seg, dst_ptr, n_graphs, n_src, known_rowptr, known_col)
  if (sh.vec) {
    if (!sh.one) HGIN_LINK_FWD(4, 64, false);
    else HGIN_G_SWITCH(sh.g, HGIN_LINK_FWD(4, G, true))
  } else {
    if (!sh.one) HGIN_LINK_FWD(1, 64, false);
    else HGIN_G_SWITCH(sh.g, HGIN_LINK_FWD(1, G, true))
  }
#undef HGIN_LINK_FWD
}

}  // namespace

extern "C" int hgin_link_loss_workspace_size(int64_t n_pos, size_t* bytes) {
  HGIN_ARG_CHECK(bytes != nullptr, "hgin_link_loss_workspace_size: bytes is NULL");
  HGIN_ARG_CHECK(n_pos >= 1 && n_pos < (int64_t(1) << 31), "hgin_link_loss_workspace_size: E out of range");
  *bytes = (size_t)kLinkMaxGrid * sizeof(float);
  return HGIN_OK;
}

extern "C" int hgin_link_loss_fwd_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                      int64_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst,
                                      int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = link_common_checks("hgin_link_loss_fwd_f32", pos, n_pos, k, n_dst, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(coef != nullptr, "hgin_link_loss_fwd_f32: coef NULL");
  HGIN_ARG_CHECK(neg != nullptr, "hgin_link_loss_fwd_f32: neg NULL");
  HGIN_ARG_CHECK(loss != nullptr, "hgin_link_loss_fwd_f32: loss NULL");
  if (workspace == nullptr || workspace_bytes < (size_t)kLinkMaxGrid * sizeof(float)) {
    set_error("hgin_link_loss_fwd_f32: workspace %zu bytes < required %zu", workspace_bytes,
              (size_t)kLinkMaxGrid * sizeof(float));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  float* partial = static_cast<float*>(workspace);
  launch_link_fwd<false>(sh, s, pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src, ld_src, z_dst, ld_dst,
                         (int)F, coef, neg, partial, nullptr, nullptr);
  int rc2 = check_launch("hgin_link_loss_fwd_f32");
  if (rc2 != HGIN_OK) return rc2;
  HGIN_TRACE("k_link_loss_sum");
  k_link_loss_sum<<<1, 256, 0, s>>>(partial, (int)sh.grid, loss);
  return check_launch("hgin_link_loss_fwd_f32");
}

extern "C" int hgin_link_loss_fwd_obj_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                          int64_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst,
                                          int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss,
                                          void* workspace, size_t workspace_bytes, int32_t objective, float param,
                                          void* stream) {
  const char* what = "hgin_link_loss_fwd_obj_f32";
  const int rc = link_common_checks(what, pos, n_pos, k, n_dst, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(coef != nullptr, "%s: coef NULL", what);
  HGIN_ARG_CHECK(neg != nullptr, "%s: neg NULL", what);
  HGIN_ARG_CHECK(loss != nullptr, "%s: loss NULL", what);
  HGIN_ARG_CHECK(objective >= kObjBce && objective <= kObjSelfAdv, "%s: objective = %d must be in [0, 3]", what,
                 (int)objective);
  HGIN_ARG_CHECK(objective != kObjSoftmax || (std::isfinite(param) && param > 0.0f),
                 "%s: temperature = %g must be finite and > 0", what, (double)param);
  HGIN_ARG_CHECK(objective != kObjSelfAdv || (std::isfinite(param) && param >= 0.0f),
                 "%s: alpha = %g must be finite and >= 0", what, (double)param);
  if (workspace == nullptr || workspace_bytes < (size_t)kLinkMaxGrid * sizeof(float)) {
    set_error("%s: workspace %zu bytes < required %zu", what, workspace_bytes, (size_t)kLinkMaxGrid * sizeof(float));
    return HGIN_E_WORKSPACE;
  }
  if (objective == kObjBce)
    return hgin_link_loss_fwd_f32(pos, n_pos, k, seed, offset, n_dst, z_src, ld_src, z_dst, ld_dst, F, coef, neg, loss,
                                  workspace, workspace_bytes, stream);
  hipStream_t s = as_stream(stream);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  float* partial = static_cast<float*>(workspace);
#define HGIN_LINK_OBJ(OBJ_)                                                                                          \
  launch_link_fwd<false, OBJ_>(sh, s, pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src, ld_src, z_dst, ld_dst, \
                               (int)F, coef, neg, partial, nullptr, nullptr, param)
  if (objective == kObjSoftmax) HGIN_LINK_OBJ(kObjSoftmax);
  else if (objective == kObjBpr) HGIN_LINK_OBJ(kObjBpr);
  else HGIN_LINK_OBJ(kObjSelfAdv);
#undef HGIN_LINK_OBJ
  const int rc2 = check_launch(what);
  if (rc2 != HGIN_OK) return rc2;
  HGIN_TRACE("k_link_loss_sum");
  k_link_loss_sum<<<1, 256, 0, s>>>(partial, (int)sh.grid, loss);
  return check_launch(what);
}

extern "C" int hgin_link_rank_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                  int64_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst,
                                  int64_t ld_dst, int64_t F, int32_t* n_greater, int32_t* n_equal, void* stream) {
  const int rc = link_common_checks("hgin_link_rank_f32", pos, n_pos, k, n_dst, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_greater != nullptr, "hgin_link_rank_f32: n_greater NULL");
  HGIN_ARG_CHECK(n_equal != nullptr, "hgin_link_rank_f32: n_equal NULL");
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  launch_link_fwd<true>(sh, as_stream(stream), pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src, ld_src, z_dst,
                        ld_dst, (int)F, nullptr, nullptr, nullptr, n_greater, n_equal);
  return check_launch("hgin_link_rank_f32");
}

// ---- A18 entry points: k uniform + m given negatives per positive --------------------------------------------------
namespace {

int link_given_checks(const char* what, const int64_t* pos, int64_t E, int64_t k, int64_t n_dst, const int32_t* neg_dst,
                      int64_t m, const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F) {
  HGIN_ARG_CHECK(E >= 1 && E < (int64_t(1) << 31), "%s: E = %lld must be in [1, 2^31)", what, (long long)E);
  HGIN_ARG_CHECK(k >= 0 && k < (int64_t(1) << 31), "%s: k = %lld must be >= 0", what, (long long)k);
  HGIN_ARG_CHECK(m >= 1 && m < (int64_t(1) << 31), "%s: m = %lld must be >= 1", what, (long long)m);
  HGIN_ARG_CHECK(E * (k + m) < (int64_t(1) << 31), "%s: E * (k + m) = %lld must be < 2^31", what,
                 (long long)(E * (k + m)));
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(pos != nullptr, "%s: pos NULL", what);
  HGIN_ARG_CHECK(neg_dst != nullptr, "%s: neg_dst NULL", what);
  HGIN_ARG_CHECK(z_src != nullptr, "%s: z_src NULL", what);
  HGIN_ARG_CHECK(z_dst != nullptr, "%s: z_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_dst >= F, "%s: leading dimension too small", what);
  return HGIN_OK;
}

}  // namespace

extern "C" int hgin_link_loss_fwd_neg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                          int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src,
                                          int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float* coef,
                                          int64_t* neg, float* loss, void* workspace, size_t workspace_bytes,
                                          int32_t objective, float param, void* stream) {
  const char* what = "hgin_link_loss_fwd_neg_f32";
  const int rc = link_given_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(coef != nullptr, "%s: coef NULL", what);
  HGIN_ARG_CHECK(neg != nullptr, "%s: neg NULL", what);
  HGIN_ARG_CHECK(loss != nullptr, "%s: loss NULL", what);
  HGIN_ARG_CHECK(objective >= kObjBce && objective <= kObjSelfAdv, "%s: objective = %d must be in [0, 3]", what,
                 (int)objective);
  HGIN_ARG_CHECK(objective != kObjSoftmax || (std::isfinite(param) && param > 0.0f),
                 "%s: temperature = %g must be finite and > 0", what, (double)param);
  HGIN_ARG_CHECK(objective != kObjSelfAdv || (std::isfinite(param) && param >= 0.0f),
                 "%s: alpha = %g must be finite and >= 0", what, (double)param);
  if (workspace == nullptr || workspace_bytes < (size_t)kLinkMaxGrid * sizeof(float)) {
    set_error("%s: workspace %zu bytes < required %zu", what, workspace_bytes, (size_t)kLinkMaxGrid * sizeof(float));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  float* partial = static_cast<float*>(workspace);
#define HGIN_LINK_NEG(OBJ_)                                                                                          \
  launch_link_fwd<false, OBJ_, true>(sh, s, pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src, ld_src, z_dst, \
                                     ld_dst, (int)F, coef, neg, partial, nullptr, nullptr, param, neg_dst, (int)m)
  if (objective == kObjBce) HGIN_LINK_NEG(kObjBce);
  else if (objective == kObjSoftmax) HGIN_LINK_NEG(kObjSoftmax);
  else if (objective == kObjBpr) HGIN_LINK_NEG(kObjBpr);
  else HGIN_LINK_NEG(kObjSelfAdv);
#undef HGIN_LINK_NEG
  const int rc2 = check_launch(what);
  if (rc2 != HGIN_OK) return rc2;
  HGIN_TRACE("k_link_loss_sum");
  k_link_loss_sum<<<1, 256, 0, s>>>(partial, (int)sh.grid, loss);
  return check_launch(what);
}

extern "C" int hgin_link_rank_neg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                      int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src,
                                      int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                      int32_t* n_greater, int32_t* n_equal, void* stream) {
  const char* what = "hgin_link_rank_neg_f32";
  const int rc = link_given_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_greater != nullptr, "%s: n_greater NULL", what);
  HGIN_ARG_CHECK(n_equal != nullptr, "%s: n_equal NULL", what);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  launch_link_fwd<true, kObjBce, true>(sh, as_stream(stream), pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src,
                                       ld_src, z_dst, ld_dst, (int)F, nullptr, nullptr, nullptr, n_greater, n_equal,
                                       0.0f, neg_dst, (int)m);
  return check_launch(what);
}

// ---- A19 entry points: graph-local draws ----------------------------------------------------------------------------
namespace {

// m = 0 (then neg_dst may be NULL and k >= 1) or A18's k >= 0, m >= 1 with neg_dst
int link_seg_checks(const char* what, const int64_t* pos, int64_t E, int64_t k, int64_t n_dst, const int32_t* neg_dst,
                    int64_t m, const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                    const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs) {
  HGIN_ARG_CHECK(m >= 0 && m < (int64_t(1) << 31), "%s: m = %lld must be >= 0", what, (long long)m);
  const int rc = m == 0 ? link_common_checks(what, pos, E, k, n_dst, z_src, ld_src, z_dst, ld_dst, F)
                        : link_given_checks(what, pos, E, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_graphs >= 1 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [1, 2^31)", what,
                 (long long)n_graphs);
  HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
  HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  return HGIN_OK;
}

}  // namespace

extern "C" int hgin_neg_sample_seg(uint64_t seed, uint64_t offset, const int64_t* src, int64_t n_pos, int64_t k,
                                   const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int32_t* out,
                                   void* stream) {
  const char* what = "hgin_neg_sample_seg";
  HGIN_ARG_CHECK(n_pos >= 0 && n_pos < (int64_t(1) << 31), "%s: E = %lld must be in [0, 2^31)", what,
                 (long long)n_pos);
  HGIN_ARG_CHECK(k >= 0 && k < (int64_t(1) << 31), "%s: k = %lld must be >= 0", what, (long long)k);
  HGIN_ARG_CHECK(n_pos * k < (int64_t(1) << 31), "%s: E * k = %lld must be < 2^31", what, (long long)(n_pos * k));
  HGIN_ARG_CHECK(n_graphs >= 1 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [1, 2^31)", what,
                 (long long)n_graphs);
  if (n_pos * k == 0) return HGIN_OK;
  HGIN_ARG_CHECK(src != nullptr, "%s: src NULL", what);
  HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
  HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  HGIN_ARG_CHECK(out != nullptr, "%s: out NULL", what);
  const int64_t n = n_pos * k;
  const int64_t grid = ceil_div(n, 256);
  HGIN_TRACE("k_neg_sample_seg");
  k_neg_sample_seg<<<(unsigned)(grid < 65536 ? grid : 65536), 256, 0, as_stream(stream)>>>(
      seed, offset, src, n, (int)k, src_seg, dst_ptr, (int)n_graphs, out);
  return check_launch(what);
}

extern "C" int hgin_link_loss_fwd_seg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                          int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src,
                                          int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float* coef,
                                          int64_t* neg, float* loss, void* workspace, size_t workspace_bytes,
                                          int32_t objective, float param, const int32_t* src_seg,
                                          const int32_t* dst_ptr, int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_loss_fwd_seg_f32";
  const int rc = link_seg_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F, src_seg,
                                 dst_ptr, n_graphs);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(coef != nullptr, "%s: coef NULL", what);
  HGIN_ARG_CHECK(neg != nullptr, "%s: neg NULL", what);
  HGIN_ARG_CHECK(loss != nullptr, "%s: loss NULL", what);
  HGIN_ARG_CHECK(objective >= kObjBce && objective <= kObjSelfAdv, "%s: objective = %d must be in [0, 3]", what,
                 (int)objective);
  HGIN_ARG_CHECK(objective != kObjSoftmax || (std::isfinite(param) && param > 0.0f),
                 "%s: temperature = %g must be finite and > 0", what, (double)param);
  HGIN_ARG_CHECK(objective != kObjSelfAdv || (std::isfinite(param) && param >= 0.0f),
                 "%s: alpha = %g must be finite and >= 0", what, (double)param);
  if (workspace == nullptr || workspace_bytes < (size_t)kLinkMaxGrid * sizeof(float)) {
    set_error("%s: workspace %zu bytes < required %zu", what, workspace_bytes, (size_t)kLinkMaxGrid * sizeof(float));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  float* partial = static_cast<float*>(workspace);
#define HGIN_LINK_SEG(OBJ_, GIVEN_)                                                                                 \
  launch_link_fwd<false, OBJ_, GIVEN_, true>(sh, s, pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src, ld_src, \
                                             z_dst, ld_dst, (int)F, coef, neg, partial, nullptr, nullptr, param,     \
                                             neg_dst, (int)m, src_seg, dst_ptr, (int)n_graphs)
#define HGIN_LINK_SEG_OBJ(GIVEN_)                                   \
  do {                                                              \
    if (objective == kObjBce) HGIN_LINK_SEG(kObjBce, GIVEN_);       \
    else if (objective == kObjSoftmax) HGIN_LINK_SEG(kObjSoftmax, GIVEN_); \
    else if (objective == kObjBpr) HGIN_LINK_SEG(kObjBpr, GIVEN_);  \
    else HGIN_LINK_SEG(kObjSelfAdv, GIVEN_);                        \
  } while (0)
  if (m > 0) HGIN_LINK_SEG_OBJ(true);
  else HGIN_LINK_SEG_OBJ(false);
#undef HGIN_LINK_SEG_OBJ
#undef HGIN_LINK_SEG
  const int rc2 = check_launch(what);
  if (rc2 != HGIN_OK) return rc2;
  HGIN_TRACE("k_link_loss_sum");
  k_link_loss_sum<<<1, 256, 0, s>>>(partial, (int)sh.grid, loss);
  return check_launch(what);
}

extern "C" int hgin_link_rank_seg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                      int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src,
                                      int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                      int32_t* n_greater, int32_t* n_equal, const int32_t* src_seg,
                                      const int32_t* dst_ptr, int64_t n_graphs, void* stream) {
  const char* what = "hgin_link_rank_seg_f32";
  const int rc = link_seg_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F, src_seg,
                                 dst_ptr, n_graphs);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_greater != nullptr, "%s: n_greater NULL", what);
  HGIN_ARG_CHECK(n_equal != nullptr, "%s: n_equal NULL", what);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  if (m > 0)
    launch_link_fwd<true, kObjBce, true, true>(sh, as_stream(stream), pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst,
                                               z_src, ld_src, z_dst, ld_dst, (int)F, nullptr, nullptr, nullptr,
                                               n_greater, n_equal, 0.0f, neg_dst, (int)m, src_seg, dst_ptr,
                                               (int)n_graphs);
  else
    launch_link_fwd<true, kObjBce, false, true>(sh, as_stream(stream), pos, n_pos, (int)k, seed, offset,
                                                (uint32_t)n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, nullptr, nullptr,
                                                nullptr, n_greater, n_equal, 0.0f, nullptr, 0, src_seg, dst_ptr,
                                                (int)n_graphs);
  return check_launch(what);
}

// ---- A20 entry points: draws from each source's non-neighbours ------------------------------------------------------
namespace {

// the window (n_graphs = 0 with src_seg = dst_ptr = NULL: one pool; otherwise A19's) and the known CSR
int link_filt_window_checks(const char* what, const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                            int64_t n_src, const int32_t* known_rowptr, const int32_t* known_col) {
  HGIN_ARG_CHECK(n_graphs >= 0 && n_graphs < (int64_t(1) << 31), "%s: n_graphs = %lld must be in [0, 2^31)", what,
                 (long long)n_graphs);
  if (n_graphs == 0) {
    HGIN_ARG_CHECK(src_seg == nullptr && dst_ptr == nullptr, "%s: src_seg / dst_ptr given with n_graphs = 0", what);
  } else {
    HGIN_ARG_CHECK(src_seg != nullptr, "%s: src_seg NULL", what);
    HGIN_ARG_CHECK(dst_ptr != nullptr, "%s: dst_ptr NULL", what);
  }
  HGIN_ARG_CHECK(n_src >= 1 && n_src < (int64_t(1) << 31), "%s: n_src = %lld must be in [1, 2^31)", what,
                 (long long)n_src);
  HGIN_ARG_CHECK(known_rowptr == nullptr || known_col != nullptr, "%s: known_rowptr without known_col", what);
  HGIN_ARG_CHECK(known_col == nullptr || known_rowptr != nullptr, "%s: known_col without known_rowptr", what);
  return HGIN_OK;
}

int link_filt_checks(const char* what, const int64_t* pos, int64_t E, int64_t k, int64_t n_dst, const int32_t* neg_dst,
                     int64_t m, const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                     const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int64_t n_src,
                     const int32_t* known_rowptr, const int32_t* known_col) {
  HGIN_ARG_CHECK(m >= 0 && m < (int64_t(1) << 31), "%s: m = %lld must be >= 0", what, (long long)m);
  const int rc = m == 0 ? link_common_checks(what, pos, E, k, n_dst, z_src, ld_src, z_dst, ld_dst, F)
                        : link_given_checks(what, pos, E, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F);
  if (rc != HGIN_OK) return rc;
  return link_filt_window_checks(what, src_seg, dst_ptr, n_graphs, n_src, known_rowptr, known_col);
}

}  // namespace

extern "C" int hgin_neg_sample_filt(uint64_t seed, uint64_t offset, const int64_t* src, int64_t n_pos, int64_t k,
                                    int64_t n_dst, const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                                    int64_t n_src, const int32_t* known_rowptr, const int32_t* known_col, int32_t* out,
                                    void* stream) {
  const char* what = "hgin_neg_sample_filt";
  HGIN_ARG_CHECK(n_pos >= 0 && n_pos < (int64_t(1) << 31), "%s: E = %lld must be in [0, 2^31)", what,
                 (long long)n_pos);
  HGIN_ARG_CHECK(k >= 0 && k < (int64_t(1) << 31), "%s: k = %lld must be >= 0", what, (long long)k);
  HGIN_ARG_CHECK(n_pos * k < (int64_t(1) << 31), "%s: E * k = %lld must be < 2^31", what, (long long)(n_pos * k));
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  const int rc = link_filt_window_checks(what, src_seg, dst_ptr, n_graphs, n_src, known_rowptr, known_col);
  if (rc != HGIN_OK) return rc;
  if (n_pos * k == 0) return HGIN_OK;
  HGIN_ARG_CHECK(src != nullptr, "%s: src NULL", what);
  HGIN_ARG_CHECK(out != nullptr, "%s: out NULL", what);
  const int64_t n = n_pos * k;
  const int64_t grid = ceil_div(n, 256);
  HGIN_TRACE("k_neg_sample_filt");
  k_neg_sample_filt<<<(unsigned)(grid < 65536 ? grid : 65536), 256, 0, as_stream(stream)>>>(
      seed, offset, src, n, (int)k, (uint32_t)n_dst, src_seg, dst_ptr, (int)n_graphs, n_src, known_rowptr, known_col,
      out);
  return check_launch(what);
}

extern "C" int hgin_link_loss_fwd_filt_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed,
                                           uint64_t offset, int64_t n_dst, const int32_t* neg_dst, int64_t m,
                                           const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                                           int64_t F, float* coef, int64_t* neg, float* loss, void* workspace,
                                           size_t workspace_bytes, int32_t objective, float param,
                                           const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                                           int64_t n_src, const int32_t* known_rowptr, const int32_t* known_col,
                                           void* stream) {
  const char* what = "hgin_link_loss_fwd_filt_f32";
  const int rc = link_filt_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F, src_seg,
                                  dst_ptr, n_graphs, n_src, known_rowptr, known_col);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(coef != nullptr, "%s: coef NULL", what);
  HGIN_ARG_CHECK(neg != nullptr, "%s: neg NULL", what);
  HGIN_ARG_CHECK(loss != nullptr, "%s: loss NULL", what);
  HGIN_ARG_CHECK(objective >= kObjBce && objective <= kObjSelfAdv, "%s: objective = %d must be in [0, 3]", what,
                 (int)objective);
  HGIN_ARG_CHECK(objective != kObjSoftmax || (std::isfinite(param) && param > 0.0f),
                 "%s: temperature = %g must be finite and > 0", what, (double)param);
  HGIN_ARG_CHECK(objective != kObjSelfAdv || (std::isfinite(param) && param >= 0.0f),
                 "%s: alpha = %g must be finite and >= 0", what, (double)param);
  if (workspace == nullptr || workspace_bytes < (size_t)kLinkMaxGrid * sizeof(float)) {
    set_error("%s: workspace %zu bytes < required %zu", what, workspace_bytes, (size_t)kLinkMaxGrid * sizeof(float));
    return HGIN_E_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  float* partial = static_cast<float*>(workspace);
#define HGIN_LINK_FILT(OBJ_)                                                                                          \
  launch_link_fwd<false, OBJ_, true, true, true>(sh, s, pos, n_pos, (int)k, seed, offset, (uint32_t)n_dst, z_src,     \
                                                 ld_src, z_dst, ld_dst, (int)F, coef, neg, partial, nullptr, nullptr, \
                                                 param, neg_dst, (int)m, src_seg, dst_ptr, (int)n_graphs, n_src,      \
                                                 known_rowptr, known_col)
  if (objective == kObjBce) HGIN_LINK_FILT(kObjBce);
  else if (objective == kObjSoftmax) HGIN_LINK_FILT(kObjSoftmax);
  else if (objective == kObjBpr) HGIN_LINK_FILT(kObjBpr);
  else HGIN_LINK_FILT(kObjSelfAdv);
#undef HGIN_LINK_FILT
  const int rc2 = check_launch(what);
  if (rc2 != HGIN_OK) return rc2;
  HGIN_TRACE("k_link_loss_sum");
  k_link_loss_sum<<<1, 256, 0, s>>>(partial, (int)sh.grid, loss);
  return check_launch(what);
}

extern "C" int hgin_link_rank_filt_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                       int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src,
                                       int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                       int32_t* n_greater, int32_t* n_equal, const int32_t* src_seg,
                                       const int32_t* dst_ptr, int64_t n_graphs, int64_t n_src,
                                       const int32_t* known_rowptr, const int32_t* known_col, void* stream) {
  const char* what = "hgin_link_rank_filt_f32";
  const int rc = link_filt_checks(what, pos, n_pos, k, n_dst, neg_dst, m, z_src, ld_src, z_dst, ld_dst, F, src_seg,
                                  dst_ptr, n_graphs, n_src, known_rowptr, known_col);
  if (rc != HGIN_OK) return rc;
  HGIN_ARG_CHECK(n_greater != nullptr, "%s: n_greater NULL", what);
  HGIN_ARG_CHECK(n_equal != nullptr, "%s: n_equal NULL", what);
  const LinkShape sh = link_shape(n_pos, F, z_src, ld_src, z_dst, ld_dst);
  launch_link_fwd<true, kObjBce, true, true, true>(sh, as_stream(stream), pos, n_pos, (int)k, seed, offset,
                                                   (uint32_t)n_dst, z_src, ld_src, z_dst, ld_dst, (int)F, nullptr,
                                                   nullptr, nullptr, n_greater, n_equal, 0.0f, neg_dst, (int)m, src_seg,
                                                   dst_ptr, (int)n_graphs, n_src, known_rowptr, known_col);
  return check_launch(what);
}

extern "C" int hgin_link_loss_bwd_src_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                          int64_t n_src, int64_t n_pos, int64_t k, const float* g, const float* coef,
                                          const int64_t* neg, const float* z_dst, int64_t ld_dst, int64_t F,
                                          float* g_src, int64_t ld_g, void* stream) {
  const char* what = "hgin_link_loss_bwd_src_f32";
  HGIN_ARG_CHECK(n_pos >= 1 && n_pos < (int64_t(1) << 31), "%s: E must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(k >= 1 && k < (int64_t(1) << 31) && n_pos * k < (int64_t(1) << 31),
                 "%s: k must be >= 1 and E * k < 2^31", what);
  HGIN_ARG_CHECK(n_src >= 1 && n_src < (int64_t(1) << 31), "%s: n_src must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(rowptr && col && perm, "%s: rowptr / col / perm NULL", what);
  HGIN_ARG_CHECK(g && coef && neg, "%s: g / coef / neg NULL", what);
  HGIN_ARG_CHECK(z_dst && g_src, "%s: z_dst / g_src NULL", what);
  HGIN_ARG_CHECK(ld_dst >= F && ld_g >= F, "%s: leading dimension too small", what);
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_dst) && aligned16(g_src) && ld_dst % 4 == 0 && ld_g % 4 == 0;
  const int gsz = pick_g(vec ? ceil_div(F, 4) : F);
  const unsigned grid = (unsigned)ceil_div(ceil_div(n_src, 64 / gsz), 4);
  const int64_t* neg_dst = neg + n_pos * k;
  HGIN_TRACE("k_link_bwd_src<%d,%d>", vec ? 4 : 1, gsz);
  if (vec) {
    HGIN_G_SWITCH(gsz, k_link_bwd_src<4, G><<<grid, 256, 0, s>>>(rowptr, col, perm, n_src, n_pos, (int)k, g, coef,
                                                                 neg_dst, z_dst, ld_dst, (int)F, g_src, ld_g))
  } else {
    HGIN_G_SWITCH(gsz, k_link_bwd_src<1, G><<<grid, 256, 0, s>>>(rowptr, col, perm, n_src, n_pos, (int)k, g, coef,
                                                                 neg_dst, z_dst, ld_dst, (int)F, g_src, ld_g))
  }
  return check_launch(what);
}

extern "C" int hgin_link_loss_bwd_dst_f32(const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* pos_perm,
                                          const int32_t* neg_rowptr, const int32_t* neg_col, const int32_t* neg_perm,
                                          int64_t n_dst, int64_t n_pos, const float* g, const float* coef,
                                          const float* z_src, int64_t ld_src, int64_t F, float* g_dst, int64_t ld_g,
                                          void* stream) {
  const char* what = "hgin_link_loss_bwd_dst_f32";
  HGIN_ARG_CHECK(n_pos >= 1 && n_pos < (int64_t(1) << 31), "%s: E must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(n_dst >= 1 && n_dst < (int64_t(1) << 31), "%s: n_dst must be in [1, 2^31)", what);
  HGIN_ARG_CHECK(F >= 1 && F < (1 << 24), "%s: F must be in [1, 2^24)", what);
  HGIN_ARG_CHECK(pos_rowptr && pos_col && pos_perm, "%s: pos_rowptr / pos_col / pos_perm NULL", what);
  HGIN_ARG_CHECK(neg_rowptr && neg_col && neg_perm, "%s: neg_rowptr / neg_col / neg_perm NULL", what);
  HGIN_ARG_CHECK(g && coef, "%s: g / coef NULL", what);
  HGIN_ARG_CHECK(z_src && g_dst, "%s: z_src / g_dst NULL", what);
  HGIN_ARG_CHECK(ld_src >= F && ld_g >= F, "%s: leading dimension too small", what);
  hipStream_t s = as_stream(stream);
  const bool vec = F % 4 == 0 && aligned16(z_src) && aligned16(g_dst) && ld_src % 4 == 0 && ld_g % 4 == 0;
  const int gsz = pick_g(vec ? ceil_div(F, 4) : F);
  const unsigned grid = (unsigned)ceil_div(ceil_div(n_dst, 64 / gsz), 4);
  HGIN_TRACE("k_link_bwd_dst<%d,%d>", vec ? 4 : 1, gsz);
  if (vec) {
    HGIN_G_SWITCH(gsz, k_link_bwd_dst<4, G><<<grid, 256, 0, s>>>(pos_rowptr, pos_col, pos_perm, neg_rowptr, neg_col,
                                                                 neg_perm, n_dst, n_pos, g, coef, z_src, ld_src,
                                                                 (int)F, g_dst, ld_g))
  } else {
    HGIN_G_SWITCH(gsz, k_link_bwd_dst<1, G><<<grid, 256, 0, s>>>(pos_rowptr, pos_col, pos_perm, neg_rowptr, neg_col,
                                                                 neg_perm, n_dst, n_pos, g, coef, z_src, ld_src,
                                                                 (int)F, g_dst, ld_g))
  }
  return check_launch(what);
}
