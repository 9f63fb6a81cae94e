/*
 * hgin.h — C ABI of libhgin.so, the MI355X (gfx950) heterogeneous-GIN hot path.
 *
 * The reference (youssefshoeb/GNN-Link-Prediction) has no native code: its hot path is PyG
 * `MessagePassing.propagate` + `torch_scatter.scatter` + `torch.nn.Linear`/`PReLU` reached from
 * `models.py`.  Each entry point below names the reference interface it replaces (file:line in the
 * reference tree).  The Python host (gnn-link-prediction_amd/hgin) binds this header with ctypes;
 * INTEGRATION.md shows the binding.
 *
 * Conventions (all functions):
 *   - plain C types; device pointers are `void*`/typed pointers into HBM owned and allocated by the
 *     caller; kernels never allocate.  Scratch comes from a `*_workspace_size` query + caller buffer.
 *   - every call is asynchronous on the caller's HIP stream, passed as `void* stream`
 *     (a `hipStream_t`; NULL = the default stream).  Nothing here synchronises the device, so the calls
 *     can be captured into a hipGraph (one exception: hgin_link_split_select, A21, which sizes a
 *     compaction and says so).
 *   - return value: 0 = ok, > 0 = a hipError_t from the launch, < 0 = argument error (HGIN_E_*).
 *     `hgin_last_error()` returns a thread-local message for the last failing call.
 *   - row-major matrices carry an explicit leading dimension (elements, not bytes).
 *   - stateless and re-entrant; one host thread per GPU process.
 */
#ifndef HGIN_H_
#define HGIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGIN_ABI_VERSION 16

#define HGIN_OK 0
#define HGIN_E_ARG (-1)        /* bad size / null pointer / unsupported combination */
#define HGIN_E_ALIGN (-2)      /* pointer or leading dimension misaligned for the chosen path */
#define HGIN_E_WORKSPACE (-3)  /* workspace too small */

/* combine modes of the GIN self term, models.py:210-215 */
#define HGIN_COMBINE_NONE 0    /* out = aggregate only (also: every backward aggregate)          */
#define HGIN_COMBINE_ADD 1     /* out = aggregate + (1 + eps) * x_dst          (models.py:215)    */
#define HGIN_COMBINE_CONCAT 2  /* out = [aggregate | (1 + eps) * x_dst]        (models.py:212-213) */

/* status word bits written by hgin_csr_build into *d_status (device int32) */
#define HGIN_STATUS_ROW_OOR 1  /* a row index (the sorted key) was < 0 or >= n_rows */
#define HGIN_STATUS_COL_OOR 2  /* a column index was < 0 or >= n_cols               */
#define HGIN_STATUS_UNSORTED 4 /* a batch vector was not non-decreasing (global pooling) */

int hgin_abi_version(void);
const char* hgin_last_error(void);

/* Launch trace (test / diagnostics; no reference counterpart).  hgin_trace_enable(1) clears the record and
 * starts recording, at every dispatch site, the kernel variant launched (one '\n'-terminated tag per launch,
 * e.g. "k_ws_f32<256,256,EPI1>"); hgin_trace_enable(0) stops.  hgin_trace_read copies the record into buf
 * (NUL-terminated, at most cap - 1 bytes; the record is drained when it fits) and returns its full length.
 * Host-side only: nothing is synchronised. */
int hgin_trace_enable(int on);
size_t hgin_trace_read(char* buf, size_t cap);

/* ---- A12: COO -> CSR / CSC (stable) ------------------------------------------------------------
 * Replaces nothing in the reference directly: PyG scatters unsorted COO with atomics
 * (torch_scatter.scatter <- MessagePassing.propagate <- models.py:208).  The stable sort keeps, inside
 * every row, the original edge order, which is exactly the order CPU `scatter_add_` / `index_add_`
 * accumulate in, so segmented sums over this CSR are bit-identical to the reference's CPU path.
 *
 * edge_index: int64 [2, n_edges] row-major (the PyG layout, dataset.py:112-117).
 * key_row = 1: rows are destinations (CSR for the forward aggregate); key_row = 0: rows are sources
 *              (CSC, for the backward of index_select).
 * Outputs: rowptr int32 [n_rows + 1]; col int32 [n_edges] = the other endpoint, in sorted order;
 *          perm int32 [n_edges] = original edge id of each sorted position (may be NULL).
 * d_status: device int32, OR-ed with HGIN_STATUS_* on out-of-range indices (caller zeroes it).
 * n_edges, n_rows, n_cols < 2^31. */
int hgin_csr_workspace_size(int64_t n_edges, int64_t n_rows, size_t* bytes);
int hgin_csr_build(const int64_t* edge_index, int64_t n_edges, int key_row, int64_t n_rows,
                   int64_t n_cols, int32_t* rowptr, int32_t* col, int32_t* perm, int32_t* d_status,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- A3 + A4: GINConv message + aggregate + (1+eps) combine -------------------------------------
 * Replaces: MessagePassing.propagate (models.py:208: index_select gather + torch_scatter sum with
 * aggr='add', models.py:186; identity message models.py:219-220) fused with the self term
 * (models.py:210-215) — no [E, F] message tensor, no atomics, no separate cat / add kernel.
 *   agg[r, f]  = sum_{k = rowptr[r]}^{rowptr[r+1]-1} x_src[col[k], f]   (sequential in k, fp32, no FMA)
 *   NONE:   out[r, 0:f_src]              = agg
 *   ADD:    out[r, f]                    = agg + ((1 + eps[0]) * x_dst[r, f])   (f_dst == f_src)
 *   CONCAT: out[r, 0:f_src] = agg;  out[r, f_src:f_src+f_dst] = (1 + eps[0]) * x_dst[r, :]
 * eps: device float[1] (the GINConv eps Parameter, models.py:191-194).  Rows with no edges get 0.
 * out must not overlap x_src or x_dst (the kernels read them through restrict-qualified pointers); the
 * backward's running-gradient accumulation (ADD, eps 0) writes a fresh buffer for that reason.
 * Bit-exact against CPU scatter_add_ + cat / add on the same inputs.
 * The Python layer may skip this launch: the NONE-mode aggregate of a layer's data inputs (a resident graph's
 * features: no gradient, unchanged between steps) is computed once per (feature tensor, graph) and its output
 * reused read-only by the GEMMs that follow (hgin/ops.py STATIC_AGG).  The entry point and the ABI are unchanged;
 * a caller of the C interface that wants the same saving keeps the output and passes it on itself. */
int hgin_aggregate_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                       const float* x_src, int64_t ld_src, int64_t f_src,
                       const float* x_dst, int64_t ld_dst, int64_t f_dst,
                       const float* eps, int combine, float* out, int64_t ld_out, void* stream);

/* ---- A7 input: global mean / max pooling of the path features (GLOBAL_FEATS) --------------------------
 * Replaces torch_geometric.nn.global_mean_pool / global_max_pool of origin_input["path"] by path_batch and the
 * torch.gather that broadcasts them back to the rows (models.py:347-352; torch_scatter scatter mean / max):
 *   out[r, 0:f]  = mean of x[q, :] over the rows q of r's graph   (sequential row-order fp32 sum, one division)
 *   out[r, f:2f] = max  of x[q, :] over the same rows             (NaN propagates)
 * batch: int64 [n_rows] graph ids, non-decreasing (PyG collation, dataset.py:239-244: each graph's rows are one
 * contiguous run; ids may skip values); a descending pair ORs HGIN_STATUS_UNSORTED into *d_status (device int32,
 * caller zeroes it) and the outputs are then unspecified.  Deterministic; for graphs of at most 4096 rows the mean
 * is bit-identical to CPU scatter mean; longer graphs are summed in 2048-row chunk partials added in chunk order
 * (within fp32 rounding of the sequential sum).  f <= 4096; out must not overlap x.  No host synchronisation.
 * workspace: hgin_global_pool_workspace_size(n_rows, f). */
int hgin_global_pool_workspace_size(int64_t n_rows, int64_t f, size_t* bytes);
int hgin_global_pool_f32(const int64_t* batch, int64_t n_rows, const float* x, int64_t ldx, int64_t f,
                         float* out, int64_t ld_out, int* d_status, void* workspace, size_t workspace_bytes,
                         void* stream);
int hgin_global_pool_bf16(const int64_t* batch, int64_t n_rows, const uint16_t* x, int64_t ldx, int64_t f,
                          uint16_t* out, int64_t ld_out, int* d_status, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- A9: backward of the combine -----------------------------------------------------------------
 * Replaces the autograd of `(1 + eps) * x_r` + cat/add (models.py:212-215):
 *   g_x_dst[r, f] = (1 + eps) * g[r, f]                 (written if g_x_dst != NULL)
 *   g_eps[0]      = sum_{r, f} g[r, f] * x_dst[r, f]    (deterministic two-level reduction)
 * g points at the self-term columns of the combine gradient (ld_g is its row stride).
 * workspace: hgin_combine_bwd_workspace_size(n_rows) bytes. */
int hgin_combine_bwd_workspace_size(int64_t n_rows, size_t* bytes);
int hgin_combine_bwd_f32(const float* g, int64_t ld_g, const float* x_dst, int64_t ld_dst,
                         int64_t n_rows, int64_t f_dst, const float* eps, float* g_x_dst,
                         int64_t ld_gx, float* g_eps, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- A5: GIN MLP update on MFMA ------------------------------------------------------------------
 * Replaces GINLayer.mlp = Sequential(Linear(K, N), PReLU()) applied at models.py:217 (built at
 * models.py:236-239) and, when `accum` != NULL, the per-dst-type sum of HeteroConv(aggr='sum')
 * (models.py:286-298) for the second relation into the same node type:
 *   z = [a1 | a2] @ w^T + bias;  y = (z > 0 ? z : prelu[0] * z) [+ accum]
 * The A operand is the column concatenation of a1 ([M, k1], lda1) and a2 ([M, K - k1], lda2; NULL when
 * k1 == K), which also replaces the readout's torch.cat((x_path, raw path features)) (models.py:362-371).
 * a2_eps (device float[1], may be NULL): the a2 columns enter as (1 + a2_eps[0]) * a2 — the concat GINConv's
 * self term cat(aggregate, (1 + eps) * x_dst) (models.py:212-213) formed as the tile is loaded (the same
 * single-rounded fp32 product the aggregate's epilogue would store), so the [N_dst, F_src + F_dst] concat
 * need not be materialised.
 * w: [N, K] row-major (torch Linear.weight), bias: [N], prelu: device float[1].  Output rows are N wide.
 * z (pre-activation, saved for backward) may be NULL.  fp32 in, fp32 results (hgin_gemm_nt.hip: f32 MFMA
 * or the exact bf16 3-way operand split). */
int hgin_gin_mlp_fwd_f32(const float* a1, int64_t lda1, int64_t k1, const float* a2, int64_t lda2,
                         const float* a2_eps, const float* w, const float* bias, const float* prelu,
                         const float* accum, float* z, float* y, int64_t M, int64_t N, int64_t K,
                         const void* w_planes, void* stream);

/* ---- readout Linear without activation (models.py:326-330, the head Linear(mlp_layers[-1], 1)) ------
 *   y = [a1 | a2] @ w^T + bias     (same operand conventions as hgin_gin_mlp_fwd_f32) */
int hgin_linear_fwd_f32(const float* a1, int64_t lda1, int64_t k1, const float* a2, int64_t lda2,
                        const float* w, const float* bias, float* y, int64_t M, int64_t N, int64_t K,
                        const void* w_planes, void* stream);

/* ---- A3 / A9: long rows (degree skew) ------------------------------------------------------------------
 * The neighbour sums of rows too long for the row-per-lane-group walk of hgin_aggregate_* (whose CSR the
 * caller passes with these rows emptied, so it writes their self term and zeros for the sum): items holds
 * n_items chunks of consecutive edges as (begin, end) pairs into `col`, grouped by row in edge order; row j
 * of `long_rows` owns items [item_ptr[j], item_ptr[j + 1]).  Each chunk is summed in edge order (fp32), the
 * chunk sums of a row are added in chunk order, then (ADD) the self term (1 + eps[0]) * x_dst; the result
 * overwrites out[row, 0:f_src] (CONCAT's self columns stay as hgin_aggregate_* wrote them).  Deterministic
 * run to run; re-associated against the sequential sum (tolerance).  partial: n_items * f_src floats.
 * f_src, ld_src, ld_out multiples of 4. */
int hgin_aggregate_long_f32(const int32_t* col, const int32_t* items, int64_t n_items, const int32_t* long_rows,
                            const int32_t* item_ptr, int64_t n_long, const float* x_src, int64_t ld_src,
                            int64_t f_src, const float* x_dst, int64_t ld_dst, int64_t f_dst, const float* eps,
                            int combine, float* out, int64_t ld_out, float* partial, size_t partial_bytes,
                            void* stream);
int hgin_aggregate_long_bf16(const int32_t* col, const int32_t* items, int64_t n_items, const int32_t* long_rows,
                             const int32_t* item_ptr, int64_t n_long, const uint16_t* x_src, int64_t ld_src,
                             int64_t f_src, const uint16_t* x_dst, int64_t ld_dst, int64_t f_dst, const float* eps,
                             int combine, uint16_t* out, int64_t ld_out, float* partial, size_t partial_bytes,
                             void* stream);

/* ---- A9: PReLU + bias backward -------------------------------------------------------------------
 *   g_z = z > 0 ? g_y : prelu[0] * g_y;  g_prelu[0] = sum (z > 0 ? 0 : z * g_y);  g_bias[n] = sum_m g_z[m, n]
 * Deterministic (fixed-shape two-level reductions).  workspace: hgin_prelu_bwd_workspace_size. */
int hgin_prelu_bwd_workspace_size(int64_t M, int64_t N, size_t* bytes);
int hgin_prelu_bwd_f32(const float* g_y, int64_t ld_gy, const float* z, int64_t M, int64_t N, const float* prelu,
                       float* g_z, float* g_prelu, float* g_bias, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- plain GEMM on MFMA (backward of Linear) --------------------------------------------------------
 * c[M, N] = a[M, K] @ b[N, K]^T   ("NT", both operands K-contiguous), fp32 MFMA. */
int hgin_gemm_nt_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* c, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, const void* b_planes, void* stream);

/* ---- NT GEMM operand planes (ABI 2) --------------------------------------------------------------------
 * Every NT GEMM entry point (hgin_gin_mlp_fwd_*, hgin_linear_fwd_*, hgin_gemm_nt_*, hgin_gemm_nt_combine_*)
 * takes `w_planes` / `b_planes`: NULL, or the B operand ([N, K], the weight) pre-converted by
 * hgin_nt_planes_* — fp32: its three bf16 split planes, bf16: a copy — in the per-K-stage, XOR-swizzled
 * layout of the LDS-DMA GEMM kernel (k_nt2 in hgin_gemm_nt.hip).  With planes, shapes the kernel takes
 * (K and the A split column multiples of 32 (fp32) / 64 (bf16), 16-B aligned A rows, N a multiple of 128) run
 * on it; everything else runs on the register-staged kernel.  Results are bit-identical either way.
 * Size: hgin_nt_planes_size (elem_bytes 4 or 2) = N * K * 6 (fp32) or N * K * 2 (bf16) bytes. */
int hgin_nt_planes_size(int64_t N, int64_t K, int elem_bytes, size_t* bytes);
int hgin_nt_planes_f32(const float* b, int64_t ldb, int64_t N, int64_t K, void* out, void* stream);
int hgin_nt_planes_bf16(const uint16_t* b, int64_t ldb, int64_t N, int64_t K, void* out, void* stream);

/* ---- A9: dX GEMM with the self term's backward fused --------------------------------------------------
 * Replaces hgin_gemm_nt_* followed by hgin_combine_bwd_* in a GINConv backward (models.py:210-217 reached
 * from train.py:43): c[M, N] = a[M, K] @ b[N, K]^T (= g_comb = g_z W) and, over the self columns [cs, N)
 * (cs = F_src for concat, 0 for add; a multiple of 4), with C as stored:
 *   g_dst[m, j] = (1 + eps[0]) * c[m, cs + j]   (g_dst may be NULL)
 *   g_eps[0]    = sum_{m, j} c[m, cs + j] * x_dst[m, j]      (fixed-order per-workgroup partials + final)
 * so g_comb is not read back.  g_prev (may be NULL; may alias g_dst; row stride ld_gp): another relation's
 * gradient of the same node type, which g_dst accumulates onto (g_dst = g_prev + (1 + eps) c, one rounding
 * more) — autograd's gradient sum over the relations sharing x_dst, fused (hgin/ops.py hetero layer).
 * workspace: hgin_gemm_nt_combine_workspace_size.  Deterministic. */
int hgin_gemm_nt_combine_workspace_size(int64_t M, int64_t N, size_t* bytes);
int hgin_gemm_nt_combine_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* c, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, const float* x_dst, int64_t ld_xd, float* g_dst,
                             int64_t ld_gd, const float* g_prev, int64_t ld_gp, int64_t cs, const float* eps,
                             float* g_eps, void* workspace, size_t workspace_bytes, const void* b_planes,
                             void* stream);
int hgin_gemm_nt_combine_bf16(const uint16_t* a, int64_t lda, const uint16_t* b, int64_t ldb, uint16_t* c,
                              int64_t ldc, int64_t M, int64_t N, int64_t K, const uint16_t* x_dst, int64_t ld_xd,
                              uint16_t* g_dst, int64_t ld_gd, const uint16_t* g_prev, int64_t ld_gp, int64_t cs,
                              const float* eps, float* g_eps, void* workspace, size_t workspace_bytes,
                              const void* b_planes, void* stream);

/* ---- weight-gradient GEMM (backward of Linear: dW = g_z^T X) ----------------------------------------
 * out[N, K] = a[M, N]^T @ [b1 | b2],  b1 = columns [0, k1) ([M, k1], ldb1), b2 = columns [k1, K) ([M, K-k1],
 * ldb2; may be NULL when k1 == K).  Reduction over M split across workgroups into fp32 slabs summed in a
 * fixed order (deterministic).  workspace: hgin_gemm_tn_workspace_size. */
int hgin_gemm_tn_workspace_size(int64_t M, int64_t N, int64_t K, size_t* bytes);
int hgin_gemm_tn_f32(const float* a, int64_t lda, const float* b1, int64_t ldb1, int64_t k1, const float* b2,
                     int64_t ldb2, int64_t M, int64_t N, int64_t K, float* out, int64_t ldo, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- A9 fused: PReLU + bias backward folded into the weight-gradient GEMM ------------------------------
 * Replaces autograd of GINLayer.mlp = Sequential(Linear, PReLU) (models.py:236-239) and of the readout's
 * Linear + PReLU (models.py:300-330) at train.py:43 — hgin_prelu_bwd_* followed by hgin_gemm_tn_*:
 *   g_z = z > 0 ? g_y : prelu[0] * g_y
 *   g_w[N, K] = g_z^T @ [b1 | b2]                          (operand conventions of hgin_gemm_tn_f32)
 *   g_bias[n] = sum_m g_z[m, n];  g_prelu[0] = sum (z > 0 ? 0 : z * g_y)
 * fp32 with N, K >= 16 and g_z == NULL: one pass — g_z is formed while the A operand is staged and never
 * stored; bias / slope gradients come from per-split partials.  Otherwise (bf16, narrow shapes, or g_z
 * requested: g_z != NULL, dense, ld_gz == N) the two passes run, g_z in the caller's buffer or workspace.
 * Deterministic.  workspace: hgin_gin_mlp_bwd_w_workspace_size(M, N, K, element bytes 4 | 2, g_z != NULL).
 *
 * (A dX GEMM applying the same prologue to its A operand measured slower than the separate passes — the
 * z stream under the dX tile costs more than the g_z stream it saves — so dX reads a materialised g_z.) */
int hgin_gin_mlp_bwd_w_workspace_size(int64_t M, int64_t N, int64_t K, int elem_bytes, int have_gz, size_t* bytes);
int hgin_gin_mlp_bwd_w_f32(const float* g_y, int64_t ld_gy, const float* z, int64_t ldz, const float* prelu,
                           const float* b1, int64_t ldb1, int64_t k1, const float* b2, int64_t ldb2,
                           int64_t M, int64_t N, int64_t K, float* g_w, int64_t ldw, float* g_prelu, float* g_bias,
                           float* g_z, int64_t ld_gz, void* workspace, size_t workspace_bytes, void* stream);

/* ---- A9: self-term weight gradient of a first-layer GINConv (inputs are data) ---------------------------
 * Given G[N, KG] = g_z^T [aggregate | x_dst] (hgin_gin_mlp_bwd_w_* over both blocks; f = aggregate width):
 *   g_w[:, :f] = G[:, :f];  concat != 0: g_w[:, f:KG] = (1 + eps[0]) G[:, f:KG]
 *   g_eps[0] = sum_{n, j < KG - f} W[n, w0 + j] G[n, f + j]    (w0 = f for concat, 0 for add; W = the Linear weight)
 * i.e. d loss / d W and d loss / d eps of (1 + eps) * x_dst (models.py:210-215) without forming the [N_dst, K]
 * input gradient.  Replaces torch's scale / cat / product / sum (3-5 launches) with two.  Deterministic.
 * workspace: hgin_self_wgrad_workspace_size. */
int hgin_self_wgrad_workspace_size(int64_t N, int64_t KG, size_t* bytes);
int hgin_self_wgrad_f32(const float* G, int64_t ldg, const float* W, int64_t ldw, int64_t N, int64_t KG, int64_t f,
                        int concat, const float* eps, float* g_w, int64_t ld_gw, float* g_eps, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- cfg5: bf16 storage + bf16 MFMA, fp32 accumulate (BASELINE.json configs[4]) ---------------------
 * Same operations and operand conventions as the fp32 entry points above; `uint16_t` = a bfloat16 bit
 * pattern.  Every sum / product is formed in fp32 and each stored bf16 value is rounded once
 * (round-to-nearest-even, NaN -> 0x7FC0 — torch's float->bfloat16 conversion).  Parameters (eps, bias,
 * prelu) stay fp32; GEMM weights are bf16 copies of the fp32 masters; weight gradients come out fp32.
 *   hgin_aggregate_bf16     fp32 sequential edge-order sum of bf16 rows, then (1+eps)*x_dst, one rounding:
 *                           bit-exact vs CPU scatter_add_ over the fp32-widened inputs + .bfloat16().
 *   hgin_gin_mlp_fwd_bf16   z, y (and accum) bf16; v_mfma_f32_32x32x16_bf16.
 *   hgin_linear_fwd_bf16    the readout head: bf16 operands, fp32 output.
 *   hgin_gemm_nt_bf16       c (bf16) = a @ b^T.
 *   hgin_gemm_tn_bf16       out (fp32) = a^T [b1 | b2]; workspace: hgin_gemm_tn_workspace_size.
 *   hgin_prelu_bwd_bf16     g_z bf16; g_prelu / g_bias fp32 sums of the unrounded fp32 g_z.
 *   hgin_combine_bwd_bf16   g_x_dst bf16; g_eps fp32. */
int hgin_aggregate_bf16(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                        const uint16_t* x_src, int64_t ld_src, int64_t f_src,
                        const uint16_t* x_dst, int64_t ld_dst, int64_t f_dst,
                        const float* eps, int combine, uint16_t* out, int64_t ld_out, void* stream);
int hgin_gin_mlp_fwd_bf16(const uint16_t* a1, int64_t lda1, int64_t k1, const uint16_t* a2, int64_t lda2,
                          const float* a2_eps, const uint16_t* w, const float* bias, const float* prelu,
                          const uint16_t* accum, uint16_t* z, uint16_t* y, int64_t M, int64_t N, int64_t K,
                          const void* w_planes, void* stream);
int hgin_linear_fwd_bf16(const uint16_t* a1, int64_t lda1, int64_t k1, const uint16_t* a2, int64_t lda2,
                         const uint16_t* w, const float* bias, float* y, int64_t M, int64_t N, int64_t K,
                         const void* w_planes, void* stream);
int hgin_gemm_nt_bf16(const uint16_t* a, int64_t lda, const uint16_t* b, int64_t ldb, uint16_t* c, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, const void* b_planes, void* stream);
int hgin_gemm_tn_bf16(const uint16_t* a, int64_t lda, const uint16_t* b1, int64_t ldb1, int64_t k1,
                      const uint16_t* b2, int64_t ldb2, int64_t M, int64_t N, int64_t K, float* out, int64_t ldo,
                      void* workspace, size_t workspace_bytes, void* stream);
int hgin_prelu_bwd_bf16(const uint16_t* g_y, int64_t ld_gy, const uint16_t* z, int64_t M, int64_t N,
                        const float* prelu, uint16_t* g_z, float* g_prelu, float* g_bias, void* workspace,
                        size_t workspace_bytes, void* stream);
int hgin_gin_mlp_bwd_w_bf16(const uint16_t* g_y, int64_t ld_gy, const uint16_t* z, int64_t ldz, const float* prelu,
                            const uint16_t* b1, int64_t ldb1, int64_t k1, const uint16_t* b2, int64_t ldb2,
                            int64_t M, int64_t N, int64_t K, float* g_w, int64_t ldw, float* g_prelu,
                            float* g_bias, uint16_t* g_z, int64_t ld_gz, void* workspace, size_t workspace_bytes,
                            void* stream);
int hgin_combine_bwd_bf16(const uint16_t* g, int64_t ld_g, const uint16_t* x_dst, int64_t ld_dst,
                          int64_t n_rows, int64_t f_dst, const float* eps, uint16_t* g_x_dst, int64_t ld_gx,
                          float* g_eps, void* workspace, size_t workspace_bytes, void* stream);

/* z from y (ABI 8, round 6): a GINLayer MLP forward with no accum has y = prelu(z) exactly, so with a positive slope
 * z > 0 <=> y > 0 and z = y / slope.  hgin_gin_mlp_fwd_zy_bf16 = hgin_gin_mlp_fwd_bf16 (accum NULL) that may leave z
 * unwritten — it skips the z stores on the device when prelu[0] > 0 (the weight-stationary kernel; elsewhere it writes
 * z); hgin_gin_mlp_bwd_w_zy_bf16 = hgin_gin_mlp_bwd_w_bf16 for that layer (z / y / g_z dense [M, N], g_z required):
 * when prelu[0] > 0 it reads y in place of z (the PReLU-fused weight-stationary dW; other shapes restore z from y
 * in place first).  g_z, g_w and g_bias equal the plain pair's bit for bit; g_prelu = sum(y g_y | y <= 0) / slope,
 * the same sum up to the bf16 rounding of z.  Replaces, for the relations whose output starts a type's sum
 * (models.py:286-298 HeteroConv, the first relation into each type) and the readout's PReLU Linears, one of the
 * layer's three row streams (the z write: a third of the forward GEMM's HBM bytes). */
int hgin_gin_mlp_fwd_zy_bf16(const uint16_t* a1, int64_t lda1, int64_t k1, const uint16_t* a2, int64_t lda2,
                             const float* a2_eps, const uint16_t* w, const float* bias, const float* prelu,
                             uint16_t* z, uint16_t* y, int64_t M, int64_t N, int64_t K, void* stream);
int hgin_gin_mlp_bwd_w_zy_bf16(const uint16_t* g_y, int64_t ld_gy, uint16_t* z, const uint16_t* y,
                               const float* prelu, const uint16_t* b1, int64_t ldb1, int64_t k1,
                               const uint16_t* b2, int64_t ldb2, int64_t M, int64_t N, int64_t K, float* g_w,
                               int64_t ldw, float* g_prelu, float* g_bias, uint16_t* g_z, int64_t ld_gz,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- F3: fused readout head + MAPE loss ------------------------------------------------------------
 * Replaces the head Linear(K, 1) (models.py:326-330, :373-374) and train.py:38-42:
 *   out[m] = sum_k h[m, k] w[k] + b[0];   *loss_value = 100 * mean_m |(out[m] - y[m]) / y[m]|   (train.py:12-13)
 * written to device memory (no host sync).  Backward, given g_loss = d J / d loss_value (device float[1]):
 *   g_out[m] = ((100 g_loss / M) * sgn(q[m])) / y[m],  q = (out - y) / y   (torch's autograd of mape)
 *   g_h[m, k] = g_out[m] w[k] (g_h may be NULL);  g_w[k] = sum_m g_out[m] h[m, k];  g_b[0] = sum_m g_out[m]
 * Fixed-order reductions (deterministic).  h: fp32 or bf16 [M, K] (ldh); w [K], b [1], y [M], out [M] fp32.
 * m_valid: NULL, or a device int32 — only rows < *m_valid are labelled: the mean runs over them and the other
 * rows get zero gradient (padded static-shape batches replayed from a hipGraph).
 * workspace: hgin_head_mape_workspace_size(M, K). */
int hgin_head_mape_workspace_size(int64_t M, int64_t K, size_t* bytes);
int hgin_head_mape_fwd_f32(const float* h, int64_t ldh, int64_t M, int64_t K, const float* w, const float* b,
                           const float* y, const int32_t* m_valid, float* out, float* loss_value, void* workspace,
                           size_t workspace_bytes, void* stream);
int hgin_head_mape_fwd_bf16(const uint16_t* h, int64_t ldh, int64_t M, int64_t K, const float* w, const float* b,
                            const float* y, const int32_t* m_valid, float* out, float* loss_value, void* workspace,
                            size_t workspace_bytes, void* stream);
int hgin_head_mape_bwd_f32(const float* h, int64_t ldh, int64_t M, int64_t K, const float* w, const float* y,
                           const float* out, const float* g_loss, const int32_t* m_valid, float* g_h, int64_t ldg,
                           float* g_w, float* g_b, void* workspace, size_t workspace_bytes, void* stream);
int hgin_head_mape_bwd_bf16(const uint16_t* h, int64_t ldh, int64_t M, int64_t K, const float* w, const float* y,
                            const float* out, const float* g_loss, const int32_t* m_valid, uint16_t* g_h,
                            int64_t ldg, float* g_w, float* g_b, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---- F4: queueing-theory baseline (replaces QTBaseline.forward, models.py:54-158, run on the CPU) ----
 * Inputs prepared once per sample graph (hgin/qt.py): the path<->link edges (edge_type 0) as source runs
 * (run_ptr int32 [n_runs + 1], run_src [n_runs], dst [E0]) and a CSR by destination over all vertices
 * whose rows list edge ids by (position in run, edge id) (rowptr [N + 1], col [E0]; pos [E0]).
 *   hgin_qt_traffic   val[e] = a[src] * prod_{earlier edges e' of the run} (1 - bp[dst[e']])   (models.py:103-121)
 *   hgin_qt_link_sum  t[v] = sum over positions k (in order) of the in-order sum of val over row v's edges
 *                     at position k  — the reference's `T += scatter(...)` per position, same rounding
 *   hgin_qt_links     per link i (vertex link_ids[i]): rho = t / cap, bp = (1-rho) rho^B / ((1 - rho^(B+1))
 *                     + 1e-8), pi_0 and the 32-term occupancy series, x[v] = occ * 32000 / cap_raw
 *                     (models.py:125-145, :153); bp must be 0 at non-link vertices on entry
 *   hgin_qt_delay     out[src] = in-order sum of x[dst] over the run (models.py:154-156) */
int hgin_qt_traffic(const int32_t* run_ptr, int64_t n_runs, const int32_t* run_src, const int32_t* dst,
                    const float* a, const float* bp, float* val, void* stream);
int hgin_qt_link_sum(const int32_t* rowptr, const int32_t* col, const int32_t* pos, const float* val,
                     int64_t n_rows, float* t_out, void* stream);
int hgin_qt_links(const int32_t* link_ids, int64_t n_links, const float* t_sum, const float* cap,
                  const float* cap_raw, int buffer, float* bp, float* rho, float* pi0, float* occ, float* x,
                  void* stream);
int hgin_qt_delay(const int32_t* run_ptr, int64_t n_runs, const int32_t* run_src, const int32_t* dst,
                  const float* x, float* out, void* stream);

/* ---- F1: device-side batch collation (replaces PyG's host Collater, dataset.py:239-244) -------------
 * Executes n_desc "segment copy with an integer shift" descriptors in one launch (device array `descs`);
 * max_count = the largest descriptor count (sizes the grid).  Kinds:
 *   HGIN_COPY_F32     dst[i] = src[i]            (float, count elements)
 *   HGIN_COPY_I32_ADD dst[i] = src[i] + add      (int32)
 *   HGIN_COPY_I64_ADD dst[i] = src[i] + add      (int64)
 *   HGIN_FILL_I64     dst[i] = add               (int64)
 *   HGIN_FILL_I32     dst[i] = (int32)add        (int32)
 *   HGIN_COPY_B16     dst[i] = src[i]            (16-bit elements: bf16 features, cfg5) */
#define HGIN_COPY_F32 0
#define HGIN_COPY_I32_ADD 1
#define HGIN_COPY_I64_ADD 2
#define HGIN_FILL_I64 3
#define HGIN_FILL_I32 4
#define HGIN_COPY_B16 5
typedef struct hgin_copy_desc {
  const void* src;
  void* dst;
  int64_t count;
  int64_t add;
  int32_t kind;
  int32_t reserved;
} hgin_copy_desc;
int hgin_batched_copy(const hgin_copy_desc* descs, int64_t n_desc, int64_t max_count, void* stream);
/* Host memory the device reads in place (F1 collation, no reference counterpart): page-locked, mapped and coherent
 * (hipHostMallocCoherent: not cached on the device, so a buffer refilled by the host between launches is never read
 * stale).  hgin_batched_copy takes its descriptor table from such a buffer directly, without a host -> device copy
 * ahead of it.  The caller owns the buffer and must not refill it before the launch reading it has finished. */
int hgin_host_alloc(size_t bytes, void** ptr);
int hgin_host_free(void* ptr);

/* ---- A10: negative-edge sampler (NOT IN REFERENCE; build-defined) --------------
 * out[i] = hi32( philox4x32_10(counter = {lo32(offset+i), hi32(offset+i), 0, 0},
 *                              key = {lo32(seed), hi32(seed)}).x  *  n_dst ),  i in [0, n)
 * (Lemire multiply-shift range reduction).  int32 output. */
int hgin_neg_sample(uint64_t seed, uint64_t offset, int64_t n, int64_t n_dst, int32_t* out,
                    void* stream);

/* ---- A11: dot-product link decoder (NOT IN REFERENCE; build-defined) ------------
 * score[e] = sum_f z_src[src[e], f] * z_dst[dst[e], f]   (fp32)
 * Backward: g_z_src[s] = sum_{e: src[e]=s} g[e] * z_dst[dst[e]] over a CSR of the pairs by src
 * (rowptr/col/perm from hgin_csr_build with key_row = 0), and symmetrically for g_z_dst. */
int hgin_dot_decode_fwd_f32(const int32_t* src, const int32_t* dst, int64_t n_pairs,
                            const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                            int64_t F, float* score, void* stream);
int hgin_dot_decode_bwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                            int64_t n_rows, const float* g_score, const float* z_other,
                            int64_t ld_other, int64_t F, float* g_z, int64_t ld_g, void* stream);

/* ---- A13: fused sampled link loss (NOT IN REFERENCE; build-defined, ABI 9) -------------------------------------
 * The loss of A10 + A11 + BCE-with-logits in one pass, without materialising the negatives ahead of the scores.
 * pos: int64 [2, E] (row 0 = source ids into z_src, row 1 = destination ids into z_dst; the caller guarantees the
 * ranges, e.g. through hgin_csr_build's status).  For positive e and slot j < k the negative pair is
 * (pos[0, e], draw(offset + e * k + j)) with draw = hgin_neg_sample's definition (Philox block c >> 2, word c & 3,
 * multiply-shift into [0, n_dst)): the pairs hgin_neg_sample(seed, offset, E * k, n_dst) gives, sources repeated k
 * times.  Scores s = <z_src[src], z_dst[dst]> (fp32, mul then add, lane pieces joined by an xor tree).
 *   loss = 0.5 / E * sum_e softplus(-s_pos[e]) + 0.5 / (E k) * sum_{e, j} softplus(s_neg[e, j]),
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)) with the accurate expf / log1pf.
 * hgin_link_loss_fwd_f32 writes
 *   coef  float [E + E k]: coef[e] = 0.5 / E * (sigmoid(s_pos[e]) - 1), coef[E + e k + j] = 0.5 / (E k) * sigmoid(s_neg),
 *   neg   int64 [2, E k]:  the drawn pairs in hgin_csr_build's edge_index layout (row 0 sources, row 1 destinations),
 *   loss  float [1].
 *   (sigmoid(s) - 1 is formed as -sigmoid(-s), both from the one exp(-|s|) the softplus uses.)
 * Summation order of the loss (fixed, no float atomics): a persistent grid of at most 4096 workgroups; a group
 * takes its edges in order and their pairs t = 0 (positive), 1 .. k in batches of four; lane u < 4 of the group adds
 * the terms of the pairs t = u mod 4 in that order (groups narrower than four lanes: lane 0 adds all of them in
 * order); a workgroup joins its lanes by an xor tree per wave and adds its four waves in order into
 * partial[workgroup] (workspace:
 * hgin_link_loss_workspace_size); a second one-workgroup kernel adds the partials (thread i takes i, i + 256, ...
 * in order, then a 256-wide tree) into loss[0].  Run-to-run bit-identical.
 * Backward (g = device float [1], the upstream gradient of the loss; no host sync):
 *   hgin_link_loss_bwd_src_f32: rowptr / col / perm = hgin_csr_build(pos, key_row = 0) (static: one sort per pos).
 *     g_src[s] = sum over the row's positives in CSC order, and for each over t = 0 .. k in order, of
 *     (g * coef) * z_dst[id] (mul, mul, add; no FMA); rows without positives get exact zeros.  The running sum is
 *     compensated like the destination side's below: a hub source owning thousands of positives has as many items
 *     as a destination can have (one source owning E = 4000 positives, k = 5, F = 128: a plain fp32 sum measured
 *     2.2e-5 of that row's norm from float64, the compensated one 7.8e-8).
 *   hgin_link_loss_bwd_dst_f32: pos_* = hgin_csr_build(pos, key_row = 1) (static), neg_* = hgin_csr_build(neg,
 *     key_row = 1) (this step's negatives, one stable sort per step).  g_dst[d] = the row's positives in CSR order,
 *     then its negatives in CSR order (= ascending e k + j), each (g * coef) * z_src[src]; other rows exact zeros.
 *     This running sum carries Kahan's compensation term (same order, mul / add / sub only): a destination's pair
 *     count E (1 + k) / n_dst is unbounded, and with few destinations thousands of largely cancelling terms cost a
 *     plain fp32 sum more than the 1e-5 the gradients are held to (measured 1.2e-5 at n_dst = 1, E = 211, k = 5).
 * fp32 only.  E >= 1, k >= 1, E k < 2^31, 1 <= n_dst < 2^31, 1 <= F < 2^24: HGIN_E_ARG before any launch otherwise.
 * Rows are walked serially per lane group (no long-row split): destinations with very many pairs serialise. */
int hgin_link_loss_workspace_size(int64_t n_pos, size_t* bytes);
int hgin_link_loss_fwd_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                           int64_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst,
                           int64_t F, float* coef, int64_t* neg, float* loss, void* workspace,
                           size_t workspace_bytes, void* stream);
int hgin_link_loss_bwd_src_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_src,
                               int64_t n_pos, int64_t k, const float* g, const float* coef, const int64_t* neg,
                               const float* z_dst, int64_t ld_dst, int64_t F, float* g_src, int64_t ld_g,
                               void* stream);
int hgin_link_loss_bwd_dst_f32(const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* pos_perm,
                               const int32_t* neg_rowptr, const int32_t* neg_col, const int32_t* neg_perm,
                               int64_t n_dst, int64_t n_pos, const float* g, const float* coef, const float* z_src,
                               int64_t ld_src, int64_t F, float* g_dst, int64_t ld_g, void* stream);

/* ---- A14: sampled ranking for evaluation (NOT IN REFERENCE; build-defined, ABI 9) ------------------------------
 * The A13 forward with another epilogue: for every positive e, n_greater[e] / n_equal[e] (int32 [E]) = how many of
 * its k sampled negatives (same draws as A13) score above / exactly equal to the positive.  Writes nothing else. */
int hgin_link_rank_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset, int64_t n_dst,
                       const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                       int32_t* n_greater, int32_t* n_equal, void* stream);

/* ---- A17: ranking objectives of the fused link loss (NOT IN REFERENCE; build-defined, ABI 12) -------------------
 * hgin_link_loss_fwd_obj_f32 is hgin_link_loss_fwd_f32 with a choice of objective.  For positive e: s_0 =
 * <z_src[s], z_dst[d]>, s_j (j = 1 .. k) the scores of its k negatives; the negatives are the draws of A13 (Philox
 * counter offset + e k + j - 1, multiply-shift into [0, n_dst)), the scores are computed exactly as A13 computes them
 * (same piece order, same xor-tree), and neg is bit for bit what hgin_link_loss_fwd_f32 writes.  coef has A13's layout
 * (positives first, then negative e k + j - 1) and holds d loss / d score, so both A13 backward entry points serve
 * every objective unchanged.
 *
 *   objective              | loss                                              | coef[e]                | coef[E + e k + j - 1]
 *   -----------------------+---------------------------------------------------+------------------------+----------------------
 *   0 HGIN_LINK_OBJ_BCE    | A13, unchanged (the call forwards to A13's launch)| unchanged              | unchanged
 *   1 HGIN_LINK_OBJ_SOFTMAX| 1/E sum_e [ logsumexp_{t=0..k}(s_t / tau)         | (p_0 - 1) / (tau E)    | p_j / (tau E),
 *     param = tau > 0      |             - s_0 / tau ]                         |                        | p = softmax_t(s_t / tau)
 *   2 HGIN_LINK_OBJ_BPR    | 1/(E k) sum_e sum_j softplus(s_j - s_0)           | -sum_j sigmoid(s_j-s_0)| sigmoid(s_j - s_0)
 *                          |                                                   |   / (E k)              |   / (E k)
 *   3 HGIN_LINK_OBJ_SELFADV| 1/E sum_e 1/2 [ softplus(-s_0)                    | -1/2 sigmoid(-s_0) / E | 1/2 p_j sigmoid(s_j)
 *     param = alpha >= 0   |        + sum_j p_j softplus(s_j) ],               |                        |   / E
 *                          |   p_j = softmax_j(alpha s_j) over the k negatives,|                        |
 *                          |   a constant (no gradient flows through p)        |                        |
 *
 * Softmax / logsumexp subtract the running maximum, softplus and sigmoid go through exp(-|x|): nothing overflows for
 * finite scores of any size (selfadv: alpha s is formed in fp32, so |alpha s| must stay finite).  param is ignored by
 * objectives 0 and 2.
 * bpr: pair t = 0 is in the first batch, so every negative is finished as it arrives; the lanes that finish a
 * positive's negatives keep running sums of sigmoid(s_j - s_0), joined after the last batch (lane 0 .. 3 in order)
 * into coef[e].  softmax / selfadv need a normaliser over all of a positive's pairs and k has no bound, so they are
 * two-phase inside the same lane group and launch: phase 1 stores each pair's raw score into its coef slot (and the
 * drawn pair into neg) while every lane keeps an online (max, sum) of the group's scores, pairs in order t = 0 .. k
 * (the sum leaves out the maximum's own term, so logsumexp = max + log1p(sum) resolves losses far below 1, and the
 * softmax coefficient of the positive is formed as minus the sum of its negatives' stored coefficients, which has no
 * cancellation near p_0 = 1 and makes a positive's stored coefficients sum to zero within rounding; so does bpr's);
 * phase 2 walks the same pair -> lane mapping again, each lane reads back the slots it wrote itself (no fence
 * needed), overwrites them with the coefficients and adds the pair's loss term.  The loss is summed as in A13 (lane
 * sums, xor tree per wave, four waves in order, partials in order): run-to-run bit-identical.  Workspace, argument
 * ranges and status codes as hgin_link_loss_fwd_f32; additionally HGIN_E_ARG for an objective outside 0 .. 3, a
 * non-finite param, tau <= 0 or alpha < 0. */
#define HGIN_LINK_OBJ_BCE 0
#define HGIN_LINK_OBJ_SOFTMAX 1
#define HGIN_LINK_OBJ_BPR 2
#define HGIN_LINK_OBJ_SELFADV 3
int hgin_link_loss_fwd_obj_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                               int64_t n_dst, const float* z_src, int64_t ld_src, const float* z_dst,
                               int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss, void* workspace,
                               size_t workspace_bytes, int32_t objective, float param, void* stream);

/* ---- A18: caller-supplied negatives in the fused link loss and ranks (NOT IN REFERENCE; build-defined, ABI 13) ---
 * hgin_link_loss_fwd_neg_f32 / hgin_link_rank_neg_f32 are hgin_link_loss_fwd_obj_f32 / hgin_link_rank_f32 with
 * K = k + m negatives per positive, of which the caller supplies m: neg_dst int32 [E, m], row-major, destination ids
 * into z_dst; the caller guarantees 0 <= neg_dst < n_dst, as it does for pos (device data is not checked here).
 *
 *   pair t of positive e  | destination                                  | coefficient slot    | neg column
 *   ----------------------+----------------------------------------------+---------------------+------------
 *   t = 0                 | pos[1, e]                                    | coef[e]             | -
 *   t = 1 .. k            | draw(offset + e k + t - 1), A13's counter    | coef[E + e K + t-1] | e K + t - 1
 *                         | rule with the uniform count k                |                     |
 *   t = k + 1 .. k + m    | neg_dst[e m + t - k - 1]                     | coef[E + e K + t-1] | e K + t - 1
 *
 * The drawn part is bit for bit hgin_neg_sample(seed, offset, E k, n_dst); k = 0 draws nothing (no Philox block is
 * evaluated).  neg is int64 [2, E K] (row 0 = pos[0, e] repeated K times, row 1 = [k drawn | m given] per positive),
 * coef is float [E + E K].  K takes k's place in everything A13 / A14 / A17 define: the weights (bce 0.5 / (E K),
 * bpr 1 / (E K); softmax 1 / (tau E) and selfadv 0.5 / E do not depend on it), the softmax and selfadv normalisers run
 * over all K negatives, a softmax / bpr positive's coefficient is minus the sum of its K stored ones, the rank counts
 * cover all K negatives.  Pairs are still taken in batches of four, t = 0 first, lane u of a group finishing pair
 * t0 + u, and a batch may hold drawn and given pairs side by side; scores, loss terms and their summation order are
 * those of A13 / A17, so with equal destinations a given pair carries the bits of a drawn one: (k, neg_dst) and
 * (0, [draws | neg_dst]) agree bitwise, and (0, the K draws) agrees with hgin_link_loss_fwd_obj_f32 at k = K.
 * Backward: hgin_link_loss_bwd_src_f32 / hgin_link_loss_bwd_dst_f32 with K in place of k, on the coef / neg written here.
 * objective / param as A17 (0 = bce included).  Workspace: hgin_link_loss_workspace_size.  E >= 1, k >= 0, m >= 1,
 * E (k + m) < 2^31, other ranges and status codes as A17; HGIN_E_ARG for neg_dst = NULL. */
int hgin_link_loss_fwd_neg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                               int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                               const float* z_dst, int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss,
                               void* workspace, size_t workspace_bytes, int32_t objective, float param, void* stream);
int hgin_link_rank_neg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                           int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                           const float* z_dst, int64_t ld_dst, int64_t F, int32_t* n_greater, int32_t* n_equal,
                           void* stream);

/* ---- A15: full-candidate filtered ranking (NOT IN REFERENCE; build-defined, ABI 10) ----------------------------
 * For query q (s = pos[0, q], d = pos[1, q]; pos int64 [2, E] as in A13) and score(q, c) = <z_src[s], z_dst[c]>, the
 * candidate set C(q) is every c in [0, n_dst) with c != d and, when known_rowptr is given, (s, c) not a known edge.
 *   n_greater[q] = |{c in C(q): score(q, c) >  score(q, d)}|
 *   n_equal[q]   = |{c in C(q): score(q, c) == score(q, d)}|
 *   n_cand[q]    = |C(q)| = n_dst - 1 - |distinct known neighbours of s other than d|        (all int32 [E])
 * known_rowptr int32 [n_src + 1] / known_col int32: a CSR by source whose columns are sorted within each row;
 * repeated columns count once, columns outside [0, n_dst) are ignored.  known_rowptr = NULL: unfiltered.
 * Scores are exact-fp32 matrix-core dot products (v_mfma_f32_32x32x2_f32), features taken in blocks of 8 in ascending
 * order, inside a block in the pairs (0, 4), (1, 5), (2, 6), (3, 7); threshold, sweep and filter use this one
 * sequence, so a destination row equal to row d is counted in n_equal wherever it lies.  No score is written: every
 * 128-query block streams z_dst once and keeps two counters per query in registers; counts are joined by integer
 * atomics and the known neighbours' contributions are subtracted afterwards (deterministic, run-to-run identical).
 * Workspace: hgin_link_full_rank_workspace_size (one float per query).  fp32 only; rows need no alignment (16-byte
 * loads are used when F, both strides and both bases allow them).  1 <= E < 2^31, 1 <= n_src, n_dst < 2^31,
 * 1 <= F < 2^24, ld >= F: HGIN_E_ARG before any launch otherwise, also for known_rowptr without known_col;
 * HGIN_E_WORKSPACE for a workspace that is NULL or too small.  E * n_dst may exceed 2^31. */
int hgin_link_full_rank_workspace_size(int64_t n_pos, int64_t n_dst, int64_t F, size_t* bytes);
int hgin_link_full_rank_f32(const int64_t* pos, int64_t n_pos, int64_t n_src, int64_t n_dst, const float* z_src,
                            int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                            const int32_t* known_rowptr, const int32_t* known_col, int32_t* n_greater,
                            int32_t* n_equal, int32_t* n_cand, void* ws, size_t ws_bytes, void* stream);

/* ---- A16: top-K link retrieval (NOT IN REFERENCE; build-defined, ABI 11) ---------------------------------------
 * For query q (s = src[q]; src int64 [n_query], repeats allowed, the caller guarantees 0 <= s < n_src) and
 * score(q, c) = <z_src[s], z_dst[c]>, the candidate set C(q) is every c in [0, n_dst) such that, when known_rowptr is
 * given, (s, c) is not a known edge (there is no "own destination" here).  Row q of top_idx (int32 [n_query, k]) /
 * top_score (float [n_query, k]) holds the min(k, |C(q)|) best candidates ordered by (score descending, index
 * ascending) — a total order, so the result is unique —; the remaining slots hold idx = -1, score = -inf.
 * known_rowptr int32 [n_src + 1] / known_col int32: as in A15, a CSR by source whose columns are sorted within each
 * row (repeated columns are harmless, columns outside [0, n_dst) match nothing).  known_rowptr = NULL: unfiltered.
 * Scores carry the bits of the A15 kernels: exact-fp32 matrix-core dot products (v_mfma_f32_32x32x2_f32), features in
 * blocks of 8 in ascending order, inside a block in the pairs (0, 4), (1, 5), (2, 6), (3, 7), zeros past F.
 * top_score[q, j] is bit for bit the threshold hgin_link_full_rank_f32 computes for the pair (s, top_idx[q, j]), and
 * the output depends neither on how the destination range is split over workgroups nor on where a query sits in the
 * batch.  Inputs are finite; with NaN or +-inf embeddings (or finite ones whose score overflows) the selection is
 * unspecified (nothing out of bounds is touched).
 * No [n_query, n_dst] object exists: the A15 sweep (128 queries x 128-destination tiles) compares the accumulators
 * with one register threshold per lane and query column, the current k-th best of a private sorted list of k (score,
 * index) entries per (query, split, wave row, lane half) kept in the workspace; a second kernel merges a query's
 * 4 * splits lists under the total order.  No atomics, run-to-run identical.
 * Workspace: hgin_link_topk_workspace_size = n_query * 4 * splits * (8 k + 4) bytes (each term rounded up to 256),
 * splits = the A15 split count of (n_query, n_dst).  fp32 only; rows need no alignment (16-byte loads are used when F,
 * both strides and both bases allow them).  1 <= n_query < 2^31, 1 <= n_src, n_dst < 2^31, 1 <= F < 2^24, ld >= F,
 * 1 <= k <= 128 (k may exceed n_dst): HGIN_E_ARG before any launch otherwise, also for known_rowptr without
 * known_col; HGIN_E_WORKSPACE for a workspace that is NULL or too small. */
int hgin_link_topk_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, int64_t k, size_t* bytes);
int hgin_link_topk_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                       int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, const int32_t* known_rowptr,
                       const int32_t* known_col, int64_t k, int32_t* top_idx, float* top_score, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- A19: graph-local negatives and candidates (NOT IN REFERENCE; build-defined, ABI 14) --------------------------
 * A collated batch of G graphs (hgin.data.collate) keeps each graph's rows of a node type in one contiguous block.
 * The segmentation of a relation is src_seg int32 [n_src] (the graph of every source row, any order) and dst_ptr int32
 * [G + 1] (dst_ptr[0] = 0, dst_ptr[G] = n_dst, non-decreasing: graph g owns the destinations dst_ptr[g] ..
 * dst_ptr[g + 1] - 1; empty graphs are allowed).  For a source s: g = src_seg[s], lo = dst_ptr[g],
 * n = dst_ptr[g + 1] - lo.  The *_seg entry points are their A10 / A13 / A14 / A15 / A16 / A17 / A18 counterparts
 * under this rule; the unsegmented entry points, their launches and their bits are unchanged.
 *   Draw.  The negative with Philox counter c is lo + hi32(word(c) * n), word(c) = the word A10 uses at the same
 *     counter (block c >> 2, word c & 3, key = seed), c = offset + e k + t - 1 as in A13.  With G = 1 (lo = 0,
 *     n = n_dst) every draw is bit for bit A10's.
 *   Candidates of a query (s, d): the destinations c in [lo, lo + n) with c != d and (s, c) not a known edge.  Known
 *     edges that leave the graph are never candidates and are not subtracted:
 *     n_cand = n - 1 - |distinct known neighbours of s inside [lo, lo + n) other than d|.
 *   Top-K candidates of a query s: the destinations in [lo, lo + n) that are not known neighbours of s; a query whose
 *     graph has no destination (n = 0) returns a fully padded row (idx -1, score -inf).
 * The caller guarantees 0 <= src_seg < G, a valid dst_ptr and, where there are positives, that every positive's
 * destination lies in its source's graph (so n >= 1 there); device data is not checked.  Nothing is read out of range
 * even so: g is clamped into [0, G), dst_ptr values into [0, n_dst], a drawn id into [0, n_dst) as A15's clamp_id does.
 *   hgin_neg_sample_seg: out int32 [E k], draw i belongs to positive i / k (src = its source ids, int64 [E]) and has
 *     counter offset + i.
 *   hgin_link_loss_fwd_seg_f32: A18's argument list plus the segmentation; neg_dst = NULL with m = 0 is allowed (then
 *     k >= 1), and every objective is served.  One src_seg load and two dst_ptr loads per positive; pair batching,
 *     Philox window, scores, loss terms, summation order and the coef / neg layout are A13 / A17 / A18's, so both
 *     backward entry points serve it unchanged and a segmented draw carries the bits the same destination carries as
 *     a given negative.
 *   hgin_link_rank_seg_f32: A14 / A18's ranks over the segmented draws (neg_dst = NULL with m = 0 allowed).
 *   hgin_link_full_rank_seg_f32: A15 over the candidates above.  Threshold pre-pass as A15; in the sweep a lane
 *     compares a destination only inside its query column's segment, and a workgroup visits only the tiles
 *     min lo / 128 .. ceil(max hi / 128) of its 128 queries (block-wide min / max; each split takes a slice of that
 *     range, an empty slice returns at once), so queries sorted by graph cost E n_dst / G instead of E n_dst; the
 *     filter subtracts a known neighbour only inside the segment.  Scores keep A15's K order: a (query row,
 *     destination row) pair carries the bits it carries unsegmented, wherever its tile lies.
 *   hgin_link_topk_seg_f32: A16 with the same tile range; the in-segment test sits in the insertion path.  Workspace
 *     as hgin_link_topk_workspace_size (the per-list counts are zeroed first: a workgroup with an empty slice writes
 *     none).
 * Additional status: HGIN_E_ARG for src_seg / dst_ptr = NULL or n_graphs outside [1, 2^31). */
int hgin_neg_sample_seg(uint64_t seed, uint64_t offset, const int64_t* src, int64_t n_pos, int64_t k,
                        const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int32_t* out, void* stream);
int hgin_link_loss_fwd_seg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                               int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                               const float* z_dst, int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss,
                               void* workspace, size_t workspace_bytes, int32_t objective, float param,
                               const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, void* stream);
int hgin_link_rank_seg_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                           int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                           const float* z_dst, int64_t ld_dst, int64_t F, int32_t* n_greater, int32_t* n_equal,
                           const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, void* stream);
int hgin_link_full_rank_seg_f32(const int64_t* pos, int64_t n_pos, int64_t n_src, int64_t n_dst, const float* z_src,
                                int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                const int32_t* known_rowptr, const int32_t* known_col, int32_t* n_greater,
                                int32_t* n_equal, int32_t* n_cand, void* ws, size_t ws_bytes, const int32_t* src_seg,
                                const int32_t* dst_ptr, int64_t n_graphs, void* stream);
int hgin_link_topk_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                           int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, const int32_t* known_rowptr,
                           const int32_t* known_col, int64_t k, int32_t* top_idx, float* top_score, void* ws,
                           size_t ws_bytes, const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                           void* stream);

/* ---- A20: sampled negatives drawn from each source's non-neighbours (NOT IN REFERENCE; build-defined, ABI 15) ------
 * The draws of A10 / A13 / A14 / A17 / A18 / A19 are uniform over a window of destinations and may name a true edge.
 * The *_filt entry points draw uniformly over the window minus the source's known neighbours instead, from the same
 * Philox word: no rejection, no retry, draw i still has counter offset + i.
 *   Window of positive e (source s): [lo, lo + n) = [0, n_dst) without a segmentation (n_graphs = 0, src_seg = dst_ptr
 *     = NULL: one pool), A19's segment of s otherwise.
 *   Known row of s: known_col[known_rowptr[s] .. known_rowptr[s + 1]), the CSR by source of A15 / A16 (known_rowptr
 *     int32 [n_src + 1], known_col int32); the caller guarantees columns strictly increasing within a row and inside
 *     [0, n_dst).  c_0 < ... < c_{d-1} = the row's columns inside the window, found by two lower bounds on the row (known
 *     edges that leave the graph are ignored, as A19 ignores them for ranking); f = n - d free destinations.
 *   Draw of slot t = 1 .. k: counter c = offset + e k + t - 1, word w = block(c >> 2)[c & 3], key = seed, as A13.
 *     f == 0 (every destination of the window is a neighbour; such a source has no true negative):
 *       draw = lo + hi32(w * n), the unfiltered draw, which is then a known edge.
 *     otherwise r = hi32(w * f), j = the smallest index with (c_j - lo) - j > r (d if there is none; the sequence
 *       (c_i - lo) - i is non-decreasing, so j comes from a binary search), draw = lo + r + j: the r-th element,
 *       0-based, of the window minus the neighbours.  Exactly uniform over the complement (as uniform as A10 is over
 *       [0, n_dst)), deterministic.
 *     An empty row gives f = n, j = 0: bit for bit A13's draw (one pool) or A19's (segmented).
 *   Hand case: window [10, 16), known columns {11, 12, 15}: free = {10, 13, 14}, f = 3.  seed 0, offset 0 gives
 *     Random123's known-answer words 6627e8d5 e169c58d bc57ac4c 9b00dbd8, so r = 1, 2, 2, 1 and the draws are
 *     13, 14, 14, 13.
 * Given negatives (neg_dst, A18) are the caller's choice and are not filtered.  known need not contain the positives;
 * what is not in it can be drawn.  known_rowptr = known_col = NULL: no known edges (the *_seg / A18 bits).
 * A row that breaks the guarantee (unsorted, repeated or out-of-range columns) makes the draw unspecified; it still
 * lands inside the window clamped to [0, n_dst) and nothing is read outside the row: s is clamped into [0, n_src), a
 * row end below its start counts as empty, d > n counts as f = 0, and a drawn id is kept below n_dst as A19 keeps it.
 * Everything downstream is A13 / A14 / A17 / A18 / A19 unchanged: scores, loss terms, summation order, the coef / neg
 * layout, both backward entry points; a filtered draw of destination c contributes the bits c contributes as a given
 * negative.  In k_link_fwd the filter is one more compile-time flag, instantiated in its given + segmented form only
 * (m = 0 and n_graphs = 0 are run-time cases; HGIN_TRACE tag: the *_seg tag of what the call uses, then ",FILT"): row
 * bounds, window clip, d and f once per positive, one search per drawn pair (the searches of a batch of four advance
 * together; given pairs are not searched).  The unfiltered entry points, their instantiations and bits are unchanged.
 *   hgin_neg_sample_filt: hgin_neg_sample_seg's (src, n_pos, k) form plus n_dst (the pool when n_graphs = 0).
 *   hgin_link_loss_fwd_filt_f32: hgin_link_loss_fwd_seg_f32's arguments plus n_src / known_rowptr / known_col; neg_dst =
 *     NULL with m = 0 allowed (then k >= 1); every objective.
 *   hgin_link_rank_filt_f32: hgin_link_rank_seg_f32's likewise.
 * Status: the *_seg ranges and codes, with n_graphs = 0 allowed when src_seg = dst_ptr = NULL; HGIN_E_ARG before any
 * launch for n_graphs = 0 with a segmentation pointer, n_src < 1, known_rowptr without known_col or the reverse. */
int hgin_neg_sample_filt(uint64_t seed, uint64_t offset, const int64_t* src, int64_t n_pos, int64_t k, int64_t n_dst,
                         const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int64_t n_src,
                         const int32_t* known_rowptr, const int32_t* known_col, int32_t* out, void* stream);
int hgin_link_loss_fwd_filt_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                                int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                                const float* z_dst, int64_t ld_dst, int64_t F, float* coef, int64_t* neg, float* loss,
                                void* workspace, size_t workspace_bytes, int32_t objective, float param,
                                const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int64_t n_src,
                                const int32_t* known_rowptr, const int32_t* known_col, void* stream);
int hgin_link_rank_filt_f32(const int64_t* pos, int64_t n_pos, int64_t k, uint64_t seed, uint64_t offset,
                            int64_t n_dst, const int32_t* neg_dst, int64_t m, const float* z_src, int64_t ld_src,
                            const float* z_dst, int64_t ld_dst, int64_t F, int32_t* n_greater, int32_t* n_equal,
                            const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, int64_t n_src,
                            const int32_t* known_rowptr, const int32_t* known_col, void* stream);

/* ---- A21: leakage-free train / valid / test edge splits (NOT IN REFERENCE; build-defined, ABI 16) -----------------
 * The link head scores edges of a relation that the encoder also passes messages over; an edge that is held out has to
 * leave the relation and its reverse.  The part of an edge is a function of its endpoint pair, not of its position:
 *   x = philox4x32_10(counter = {(uint32)s, (uint32)d, 1, 0}, key = {lo32(seed), hi32(seed)})
 * for an edge (s, d) of the relation in its forward orientation (s = edge_index[0, e], d = edge_index[1, e]).  An edge
 * (d, s) of the reverse relation evaluates the same rule with swap = 1: s = edge_index[1, e], d = edge_index[0, e].
 * Word 2 of the counter is 1, so this stream is disjoint from the samplers' (A10 / A13 / A19 / A20: words 2 and 3 are 0).
 * The bounds are integers computed on the host and passed as uint64 so that 2^32 is representable:
 *   b_test = floor(test * 2^32), b_val = floor((test + val) * 2^32), b_sup = floor(disjoint * 2^32)
 *   part 3 (test)                     x.x < b_test
 *   part 2 (valid)                    not part 3, and x.x < b_val
 *   part 1 (train, supervision only)  not part 2 or 3, and x.y < b_sup
 *   part 0 (train, message)           none of the above
 * Consequences: a pair and its flipped twin get the same part without any join; all copies of a multi-edge get the
 * same part; the part does not depend on edge order; part sizes are binomial, not exact counts.  Only the low 32 bits
 * of an endpoint enter the counter (node counts are below 2^31 everywhere else in this header).
 *   hgin_link_split_parts: one Philox evaluation per edge; part uint8 [E] receives the part code and hist int64 [4]
 *     is INCREMENTED by the four part counts (the caller zeroes it): per-workgroup LDS counts, then one integer atomic
 *     per part and workgroup - integer sums do not depend on the order, so the result is deterministic.  E = 0 launches
 *     nothing.  HGIN_E_ARG for E < 0, a bound above 2^32, b_val < b_test, or a NULL pointer with E > 0.
 *   hgin_link_split_select: stable stream compaction of the edges whose part's bit is set in keep_mask (bit p = part p,
 *     4 bits; a part byte is read as part & 3).  out_edge int64 [2, n_out] (row stride n_out) receives the kept columns
 *     of edge_index (int64 [2, E], row stride E) in input order and out_eid int64 [n_out] their original positions, so
 *     that edge attributes can follow.  Fixed tiles of tile_edges edges (256 threads x 8); three plain launches:
 *     (1) per-tile counts, (2) an exclusive scan of the tile counts by one workgroup, scan_width tiles per pass with a
 *     running carry, (3) scatter with wave-ballot ranks (wave64) and LDS wave offsets.  No workgroup waits on another.
 *     Between (2) and (3) the scanned total is copied to the host and the stream is synchronised: when it disagrees
 *     with n_out the call returns HGIN_E_ARG and (3), which would write past the outputs, is not launched.  This is the
 *     one entry point that synchronises; it cannot be captured into a hipGraph.  E = 0 (then n_out must be 0) launches
 *     nothing; n_out = 0 with E > 0 runs (1) and (2) only and the outputs may be NULL.
 *     Workspace: hgin_link_split_select_workspace_size(E) = 4 bytes per tile + 8 bytes per tile + 8, each term rounded
 *     up to 256.  HGIN_E_ARG for E < 0 or E >= 2^40, keep_mask outside [0, 15], n_out outside [0, E], a NULL pointer
 *     that would be read or written; HGIN_E_WORKSPACE for a workspace that is NULL or too small.
 *   hgin_link_split_geometry: tile_edges and scan_width of this build (either pointer may be NULL). */
int hgin_link_split_parts(const int64_t* edge_index, int64_t E, int swap, uint64_t seed, uint64_t b_test,
                          uint64_t b_val, uint64_t b_sup, uint8_t* part, int64_t* hist, void* stream);
int hgin_link_split_select_workspace_size(int64_t E, size_t* bytes);
int hgin_link_split_select(const int64_t* edge_index, const uint8_t* part, int64_t E, int keep_mask, int64_t* out_edge,
                           int64_t* out_eid, int64_t n_out, void* ws, size_t ws_bytes, void* stream);
int hgin_link_split_geometry(int* tile_edges, int* scan_width);

/* ---- A22: neighbour-sampled mini-batches (NOT IN REFERENCE; build-defined; added to ABI 16 without a bump) ---------
 * The link head trains on batches of positive edges; the encoder then needs only a sampled L-hop neighbourhood of their
 * endpoints.  The section is purely additive (no earlier entry point changes), so HGIN_ABI_VERSION stays 16.
 *
 * The sampling rule, for one hop of one relation r = (s_type, name, d_type) that has slot r_slot in the sampler's
 * relation list: the relation's CSR by destination (hgin_csr_build, key_row = 1: rowptr, col, perm), a frontier of global
 * destination ids v_0 .. v_{n-1}, a fanout f (1 <= f <= 128, or -1 = every neighbour), seed (uint64) and offset (uint32,
 * the batch number).  Picks of frontier node v, d = rowptr[v + 1] - rowptr[v]:
 *   f == -1 or d <= f: every CSR position 0 .. d - 1; no Philox word is consumed.
 *   otherwise Floyd's subset algorithm (an exactly uniform f-subset of [0, d), no rejection loop): for i = 0 .. f - 1
 *     J = d - f + i
 *     w_i = word i & 3 of philox4x32_10(counter = {(uint32)v, offset, 2, (uint32)(r_slot * 64 + (i >> 2))},
 *                                      key = {lo32(seed), hi32(seed)})
 *     t = hi32((uint64)w_i * (J + 1));  pick t if it has not been picked yet, else pick J.
 *   Word 2 of the counter is 2, so this stream is disjoint from the negative samplers' (A10 / A13 / A19 / A20: word 2 is
 *   0) and from the split rule's (A21: word 2 is 1).
 *   The picked positions are emitted in ascending CSR position; pick p gives source col[rowptr[v] + p] and original edge
 *   position perm[rowptr[v] + p].
 * A node's picks depend only on (seed, offset, r_slot, v): not on where v sits in the frontier, not on the batch.
 *
 * The subgraph rule, for seeds = {type: ids} (repeats allowed, a type may be absent) and fanouts f_1 .. f_L:
 *   Local rows of a type: the unique seeds, ascending; then for hop h = 1 .. L in order the nodes of that type first
 *     reached at hop h, ascending by global id.
 *   Hop h: for each relation in list order, every node of d_type that joined at hop h - 1 (hop 1: the seeds) is
 *     expanded once with fanout f_h.  A node is expanded at most once per relation in a batch, at the hop where it first
 *     appears; nodes first reached at hop L are not expanded.
 *   Edges of relation r: hop-major, then frontier (local-row) order, then ascending CSR position, as (local src, local
 *     dst) int64 [2, E_r]; e_id[r] holds the original edge positions in the same order.  Every in-edge of an expanded
 *     node is contiguous and keeps its original relative order, so the stable CSR of the subgraph sums a fully sampled
 *     row in the full graph's order.
 *   The output does not depend on execution order: new nodes are found with a resident dense global -> local map per
 *   type (int32, -1 = not in the batch) that is only read while a hop's candidates are tested, a sort + unique of the
 *   candidates, and a write of the new rows before the hop's edges are relabelled.
 *
 * Entry points (plain launches; no workgroup waits on another; nothing synchronises):
 *   hgin_neighbor_sample_offsets: off int64 [n_frontier + 1] = the exclusive scan of min(d, f) (d when f = -1) over the
 *     frontier, off[n_frontier] = the number of sampled edges, which the caller reads to size the outputs.  Three
 *     launches: per-tile counts + scan (256 nodes), a scan of the tile sums by one workgroup, the tile offsets added.
 *     A frontier id outside [0, n_rows) counts as an empty row.  Workspace: hgin_neighbor_sample_workspace_size
 *     (n_frontier) = 8 bytes per tile + 8, rounded up to 256.
 *   hgin_neighbor_sample: out_src / out_eid int64 [n_out] at off[i] .. off[i + 1] for frontier node i; a lane group per
 *     node (8, 16 or 64 lanes by f), at most two picks per lane in registers, the membership test of a Floyd step one
 *     ballot, the ascending order a rank count: O(f^2) per node whatever d is.  A store is also guarded by n_out.
 *   hgin_neighbor_fresh: out[j] = src[j] when map[src[j]] < 0 (not yet a row of the batch), else sentinel.
 *   hgin_neighbor_map_set: map[ids[i]] = base + i for base >= 0; -1 for base < 0 (the clean-up).  ids are distinct.
 *   hgin_neighbor_emit: out_edge int64 [2, n_edges] (row stride n_edges): row 0 = map_src[src[j]], row 1 = dst_base + i
 *     for the frontier slot i with off[i] <= j < off[i + 1] (a binary search per edge).
 * Status: HGIN_E_ARG before any launch for a NULL pointer that would be read or written, f outside {-1} u [1, 128],
 *   n_rows / n_nodes / n_frontier outside [0, 2^31), r_slot outside [0, 2^26), n_out above n_frontier * f, edges of an
 *   empty frontier; HGIN_E_WORKSPACE for a workspace that is NULL or too small.  Empty inputs launch nothing. */
int hgin_neighbor_sample_workspace_size(int64_t n_frontier, size_t* bytes);
int hgin_neighbor_sample_offsets(const int32_t* rowptr, int64_t n_rows, const int64_t* frontier, int64_t n_frontier,
                                 int f, int64_t* off, void* ws, size_t ws_bytes, void* stream);
int hgin_neighbor_sample(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_rows,
                         const int64_t* frontier, int64_t n_frontier, int f, uint64_t seed, uint32_t offset,
                         int64_t r_slot, const int64_t* off, int64_t* out_src, int64_t* out_eid, int64_t n_out,
                         void* stream);
int hgin_neighbor_fresh(const int32_t* map, int64_t n_nodes, const int64_t* src, int64_t n, int64_t sentinel,
                        int64_t* out, void* stream);
int hgin_neighbor_map_set(int32_t* map, int64_t n_nodes, const int64_t* ids, int64_t n, int64_t base, void* stream);
int hgin_neighbor_emit(const int32_t* map_src, int64_t n_src_nodes, const int64_t* src, const int64_t* off,
                       int64_t n_frontier, int64_t dst_base, int64_t n_edges, int64_t* out_edge, void* stream);

/* ---- A23: full-candidate softmax link loss (NOT IN REFERENCE; build-defined; added to ABI 16 without a bump) -------
 * For query q (s = src[q]; src int64 [n_query], DISTINCT rows of z_src, the caller guarantees 0 <= s < n_src),
 * inv_t = fl32(1 / temperature) and the known CSR by source of A15 / A16 / A20 (known_rowptr int32 [n_src + 1] /
 * known_col int32, columns sorted within a row, no duplicates; known_rowptr = NULL: no known edges):
 *   cand(q) = { c in [0, n_dst) : (s, c) not in known }
 *   t[q, c] = fl32(score(q, c) * inv_t)      score = the A15 / A16 bits (exact-fp32 matrix-core dot products, features
 *                                            in blocks of 8 ascending, inside a block the pairs (0, 4) .. (3, 7))
 *   lse[q]  = log sum_{c in cand(q)} exp(t[q, c])      float [n_query]; -inf when cand(q) is empty
 * computed with a running maximum (no overflow for any finite t).  Backward for an upstream g float [n_query] and
 * P[q, c] = exp(t[q, c] - lse[q]) for c in cand(q), else 0:
 *   g_src[src[q], :] = g[q] * inv_t * sum_c P[q, c] * z_dst[c, :]         (rows of z_src not in src: zero)
 *   g_dst[c, :]      =        inv_t * sum_q g[q] * P[q, c] * z_src[src[q], :]
 * Where lse[q] = -inf, P is 0 and both gradients are 0 (no NaN, no inf).  With repeated sources g_src keeps one of the
 * repeats' rows: callers pass distinct sources.
 * No [n_query, n_dst] object exists in any pass: the forward is the A15 sweep (128 queries x 128-destination tiles)
 * with an online log-sum-exp epilogue, known neighbours masked inside the sweep (they are the dominant terms of a
 * trained model: subtracting them afterwards would keep no digits); both backward kernels recompute t from the operands
 * and lse, and use the 128 x 128 tile of g * inv_t * P as the operand of a second matrix-core product (g_src: a
 * workgroup owns 128 queries x 128 output features (256 once F > 128) and sweeps the destinations; g_dst: it owns 128
 * destinations and sweeps the queries; F > 256: one workgroup per chunk of 256 output features).  Where the stationary side is too short
 * to fill the machine the swept side is split (the A15 plan; for g_dst with the roles swapped) and the splits' partials
 * are added in ascending order.  No float atomics: forward and gradients are run-to-run identical.  The only inexact
 * steps are exp, log and the order of the sums.
 * Workspace: hgin_link_lse_workspace_size covers all three calls (forward: 8 bytes per (split, query); a gradient with
 * more than one split: 4 F bytes per (split, output row)).  fp32 only; rows need no alignment (16-byte loads are used
 * when F, both strides and both bases allow them).  1 <= n_query < 2^31, 1 <= n_src, n_dst < 2^31, 1 <= F < 2^24,
 * ld >= F, inv_t finite and > 0, split partials of a gradient (splits x output rows x F) below 2^39 floats: HGIN_E_ARG
 * before any launch otherwise, also for a NULL pointer and for known_rowptr without known_col; HGIN_E_WORKSPACE for a workspace that is needed and NULL or too small. */
int hgin_link_lse_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, size_t* bytes);
int hgin_link_lse_fwd_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                          int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                          const int32_t* known_rowptr, const int32_t* known_col, float* lse, void* ws, size_t ws_bytes,
                          void* stream);
int hgin_link_lse_bwd_src_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                              int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                              const int32_t* known_rowptr, const int32_t* known_col, const float* lse, const float* g,
                              float* g_src, int64_t ld_gsrc, void* ws, size_t ws_bytes, void* stream);
int hgin_link_lse_bwd_dst_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                              int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                              const int32_t* known_rowptr, const int32_t* known_col, const float* lse, const float* g,
                              float* g_dst, int64_t ld_gdst, void* ws, size_t ws_bytes, void* stream);

/* ---- A24: graph-local candidates for the full softmax link loss (NOT IN REFERENCE; build-defined; added to ABI 16
 * without a bump: purely additive, no earlier entry point changes) -----------------------------------------------------
 * A23 over A19's segmentation (src_seg int32 [n_src], dst_ptr int32 [n_graphs + 1]).  For s = src[q], [lo, lo + n) is
 * A19's segment of s (g = src_seg[s] clamped into [0, n_graphs), dst_ptr values kept inside [0, n_dst]):
 *   cand(q) = { c in [lo, lo + n) : (s, c) not in known }
 * and t, lse, P, g_src, g_dst are A23's over these candidates.  Known neighbours outside the segment are irrelevant.
 * lse[q] = -inf when n = 0 or the whole segment is known; both gradients are then exact zeros.  Scores keep the A15 K
 * order: a (query row, destination row) pair carries the bits it carries unsegmented, wherever its tile lies, and with
 * n_graphs = 1 all three calls give the unsegmented calls' bits (the slice rule below then cuts A23's splits).  The
 * unsegmented entry points, their launches and their bits are unchanged; the segmented kernels are separate
 * instantiations (traced as k_lse_sweep<4,SEG> / k_lse_bwd<4,SRC,SEG> / k_lse_bwd<4,DST,SEG>).
 *   hgin_link_lse_fwd_seg_f32, hgin_link_lse_bwd_src_seg_f32 (query-stationary): a lane keeps lo and n per query column
 *     and counts a destination only inside them; a workgroup sweeps only the tiles min lo / 128 .. ceil(max hi / 128)
 *     of its 128 queries (A19's block-wide min / max); split i of A23's `splits` takes the i-th slice of
 *     ceil(tiles / splits) of that range.  A slice may be empty: it then contributes (-inf, 0) to the merge and zeros
 *     to the fold.  Queries sorted by graph cost n_query n_dst / G instead of n_query n_dst.
 *   hgin_link_lse_bwd_dst_seg_f32 (tile-stationary): a small pre-kernel writes every query block's covered range
 *     [min lo, max hi) into the workspace; a workgroup skips, whole (no loads, no matrix-core work), every query block
 *     of its sweep whose range misses its tile, and prefetches the next block that is not skipped.  A tile every block
 *     skips writes zeros (g_dst need not be cleared by the caller).  Queries in any order are correct; shuffled ones
 *     skip nothing.
 * Deterministic as A23.  Workspace: hgin_link_lse_seg_workspace_size (>= A23's: 8 bytes per query block more behind
 * the g_dst partials) covers all three calls.  Status as A23, plus HGIN_E_ARG before any launch for src_seg or dst_ptr =
 * NULL or n_graphs outside [1, 2^31).  The caller guarantees 0 <= src_seg < n_graphs and a valid dst_ptr; nothing is read
 * out of range even so. */
int hgin_link_lse_seg_workspace_size(int64_t n_query, int64_t n_dst, int64_t F, size_t* bytes);
int hgin_link_lse_fwd_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst, const float* z_src,
                              int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F, float inv_t,
                              const int32_t* known_rowptr, const int32_t* known_col, float* lse, void* ws,
                              size_t ws_bytes, const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs,
                              void* stream);
int hgin_link_lse_bwd_src_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                  const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                  float inv_t, const int32_t* known_rowptr, const int32_t* known_col, const float* lse,
                                  const float* g, float* g_src, int64_t ld_gsrc, void* ws, size_t ws_bytes,
                                  const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, void* stream);
int hgin_link_lse_bwd_dst_seg_f32(const int64_t* src, int64_t n_query, int64_t n_src, int64_t n_dst,
                                  const float* z_src, int64_t ld_src, const float* z_dst, int64_t ld_dst, int64_t F,
                                  float inv_t, const int32_t* known_rowptr, const int32_t* known_col, const float* lse,
                                  const float* g, float* g_dst, int64_t ld_gdst, void* ws, size_t ws_bytes,
                                  const int32_t* src_seg, const int32_t* dst_ptr, int64_t n_graphs, void* stream);

/* ---- A25: neighbour sampling with an excluded set (NOT IN REFERENCE; build-defined; added to ABI 16 without a bump:
 * purely additive, no earlier entry point changes) ----------------------------------------------------------------------
 * A batch of supervised pairs must not pass messages over its own target edges.  A25 is A22's sampling rule over the
 * positions of a row that are not excluded, so that the pairs (and their flipped twins in the reverse relation) leave the
 * sampled neighbourhood of that batch alone; the sampler's graph and its CSRs stay as they are.
 *
 * Excluded set of one relation: excl int64 [n_excl], ascending, repeats allowed; key(v, u) = v * 2^32 + u for
 * destination v (the CSR row that is expanded) and source u, both in [0, 2^31).
 * Row of frontier node v, d = rowptr[v + 1] - rowptr[v]: position p in [0, d) is excluded iff
 * key(v, col[rowptr[v] + p]) occurs in excl; every copy of a multi-edge goes (as in A21, a pair's fate is a function of
 * the pair).  The free positions are q_0 < q_1 < .. < q_{d' - 1}.  Picks:
 *   f == -1 or d' <= f: every free position; no Philox word is consumed.
 *   otherwise A22's Floyd steps over [0, d'): for i = 0 .. f - 1
 *     J = d' - f + i
 *     w_i = the same word as A22: counter {(uint32)v, offset, 2, (uint32)(r_slot * 64 + (i >> 2))}, key = seed
 *     t = hi32((uint64)w_i * (J + 1));  pick t if it has not been picked yet, else pick J.
 *   A picked rank t means CSR position q_t.  Emission is in ascending CSR position, col / perm as in A22.
 * A row with no excluded position gives A22's picks bit for bit.  A key that names no edge, or a row that is not in the
 * frontier, has no effect.  The picks are a pure function of (seed, offset, r_slot, v, the excluded sources of v).
 *
 * Entry points (plain launches; no workgroup waits on another; no atomics; the output does not depend on execution
 * order):
 *   hgin_neighbor_sample_offsets_excl: off int64 [n_frontier + 1] = the exclusive scan of min(d', f) (d' when f = -1),
 *     the total in off[n_frontier].  A lane finds its node's key range in excl with two binary searches; a node with an
 *     empty range reads no row; the wave then sweeps the rows that have one, 64 positions per round (membership: a binary
 *     search of the position's key inside the node's range; d' = the popcounts of the free-flag ballots).  The scan and
 *     the tile offsets are A22's launches.  Workspace: hgin_neighbor_sample_workspace_size(n_frontier), as A22; nothing
 *     is carried from this call to the next one.
 *   hgin_neighbor_sample_excl: out_src / out_eid under the rule above.  A22's lane groups; the group's lead lane finds
 *     the key range; a row with an empty range takes A22's path (f positions read).  A row with exclusions is swept by
 *     the whole wave: once for d', and once more where the popcount prefix of the free-flag ballot is the compaction
 *     slot (copied rows) or maps the picked ranks to CSR positions (Floyd rows): O(d / 64 * log x_v + f^2 / W) for a row
 *     with x_v keys, unchanged otherwise.  No per-row list is kept in registers or LDS, so x_v is unbounded.  Every loop
 *     around a ballot or shuffle runs on wave-uniform values.
 *   n_excl = 0 (excl may then be NULL) gives the A22 calls' outputs bit for bit.
 * Status: as A22, plus HGIN_E_ARG before any launch for excl = NULL with n_excl > 0 and n_excl outside [0, 2^31).  The
 *   offsets call accepts col = NULL for a relation without edges (no row is swept then).  The A22 kernels and entry
 *   points are unchanged. */
int hgin_neighbor_sample_offsets_excl(const int32_t* rowptr, const int32_t* col, int64_t n_rows, const int64_t* frontier,
                                      int64_t n_frontier, int f, const int64_t* excl, int64_t n_excl, int64_t* off,
                                      void* ws, size_t ws_bytes, void* stream);
int hgin_neighbor_sample_excl(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t n_rows,
                              const int64_t* frontier, int64_t n_frontier, int f, uint64_t seed, uint32_t offset,
                              int64_t r_slot, const int64_t* excl, int64_t n_excl, const int64_t* off, int64_t* out_src,
                              int64_t* out_eid, int64_t n_out, void* stream);

/* ---- F4 widening: HetroGAT's graph attention (models.py:380-506, PyG 2.0.2 GATConv) ---------------------------
 * x_s / x_d: projected source / destination features [N, H * C] (row stride ld*), edges = the relation after
 * GATConv's self-loop handling, as CSR by destination (rowptr, col) and CSC by source (cptr, cdst, cpos = the CSR
 * position of each CSC entry).  fp32; one thread per (row, head); every sum in a fixed order (deterministic).
 *   hgin_gat_logits_f32:  a[n, h] = sum_c x[n, h, c] att[h, c]
 *   hgin_gat_fwd_f32:     alpha[k, h] (CSR order) = softmax over the row of leaky_relu(a_s[j_k, h] + a_d[i, h], slope)
 *                         (exp(e - max) / (sum + 1e-16), PyG's softmax); out[i, h, :] = sum_k alpha x_s[j_k, h, :]
 *                         + bias [+ accum].  a_d, bias, accum may be NULL.
 *   hgin_gat_bwd_dst_f32: g_pre[k, h] = d loss / d (a_s[j_k, h] + a_d[i, h]) (softmax + leaky_relu backward),
 *                         g_ad[i, h] = sum_k g_pre (less the rounding residue of the softmax backward's zero sum, so
 *                         accurate to eps sum_k |g_pre|), g_xd[i, h, :] = g_ad[i, h] att_dst[h, :] (g_ad / g_xd may be
 *                         NULL)
 *   hgin_gat_bwd_src_f32: g_as[j, h] = sum_k g_pre, g_xs[j, h, :] = sum_k alpha g_out[i_k, h, :] + g_as att_src[h, :]
 *   hgin_gat_wsum_f32:    out[h * C + c] = sum_n w[n, h] x[n, h * C + c] (w NULL: 1), fixed 256-row blocks in order;
 *                         workspace: hgin_gat_wsum_workspace_size. */
int hgin_gat_logits_f32(const float* x, int64_t ldx, int64_t n, int64_t H, int64_t C, const float* att, float* a,
                        void* stream);
int hgin_gat_fwd_f32(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t H, int64_t C, const float* xs,
                     int64_t ldxs, const float* as, const float* ad, float slope, const float* bias, const float* accum,
                     int64_t ld_acc, float* alpha, float* out, int64_t ldo, void* stream);
/* Round 5 (ABI 5): the forward attention in one pass, a_s formed from the gathered x_s rows (no a_s table):
 *   hgin_gat_attn_fwd_f32:  alpha / out as hgin_gat_fwd_f32 with a_s[j, h] = x_s[j, h, :] . att_src[h, :] (the same
 *                           per-lane arithmetic as hgin_gat_logits_f32's group form), the weighted sum divided once by
 *                           the softmax denominator at the end (online max / sum); needs the wave-group shape —
 *   hgin_gat_attn_supported: 1 when (H, C) and HGIN_GAT_WAVE allow it (C a multiple of 4 with C / 4 a power of two,
 *                           H * C <= 256; rows must also be 16-B aligned: HGIN_E_ARG otherwise).
 *   Replaces hgin_gat_logits_f32 (for a_s) + hgin_gat_fwd_f32 at models.py:413-418's GATConv.forward. */
int hgin_gat_attn_fwd_f32(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t H, int64_t C,
                          const float* xs, int64_t ldxs, const float* att_src, const float* ad, float slope,
                          const float* bias, const float* accum, int64_t ld_acc, float* alpha, float* out, int64_t ldo,
                          void* stream);
int hgin_gat_attn_supported(int64_t H, int64_t C);
int hgin_gat_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t H, int64_t C,
                         const float* xs, int64_t ldxs, const float* g_out, int64_t ldg, const float* alpha,
                         const float* as, const float* ad, float slope, const float* att_dst, float* g_pre, float* g_ad,
                         float* g_xd, int64_t ldgxd, void* stream);
int hgin_gat_bwd_src_f32(const int32_t* cptr, const int32_t* cdst, const int32_t* cpos, int64_t n_src, int64_t H,
                         int64_t C, const float* g_out, int64_t ldg, const float* alpha, const float* g_pre,
                         const float* att_src, float* g_as, float* g_xs, int64_t ldgxs, void* stream);
int hgin_gat_wsum_workspace_size(int64_t n, int64_t H, int64_t C, size_t* bytes);
int hgin_gat_wsum_f32(const float* x, int64_t ldx, int64_t n, int64_t H, int64_t C, const float* w, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- F1: the fused small-batch train step (the reference's real loop: batches of small graphs) -------------------
 * hgin_sb_step: a HetroGIN forward + sqrt-MAPE backward over a padded batch in 3 L + 1 launches, or (SbArgs.gat,
 * ABI 7) a one-layer HetroGAT's (models.py:380-506: k_sb_gat_fwd, the readout, k_sb_gat_bwd, the final sum) — replaces
 * the reference's train_one_epoch body (train.py:31-44) over DataLoader batches (dataset.py:239-244)
 * (csrc/hgin_smallbatch.hip); args points to the host-filled SbArgs struct (hgin/smallbatch.py mirrors its layout;
 * hgin_sb_args_size() = its size), readout_lds = hgin_sb_readout_lds_bytes(..., with_weights = args' ro_wlds, ...):
 * the readout tile's dynamic LDS, with the hidden readout weights staged or not.  Writes every parameter gradient
 * into the flat gradient buffer and loss_value.  Deterministic. */
size_t hgin_sb_args_size(void);
int hgin_sb_args_offsets(int64_t* out, int64_t n);   /* offsetof of 19 field groups, for the host mirror's check */
int hgin_sb_readout_lds_bytes(int64_t H, int64_t f_path, int concat_path, int nhid, const int32_t* widths,
                              int with_weights, size_t* bytes);
int hgin_sb_step(const void* args, size_t args_bytes, size_t readout_lds, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HGIN_H_ */
