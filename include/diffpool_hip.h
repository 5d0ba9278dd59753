/* diffpool_hip.h — C ABI of libdiffpool_hip.so (MI355X / gfx950).
 *
 * The reference (JiaxuanYou/graph-pooling) has no FFI of its own: its DiffPool path is stock
 * torch calls inside encoders.py / set2set.py / aggregators.py.  Each entry point below replaces
 * the torch call sites named in its comment (file:line relative to the reference root); the
 * Python modules in graph_pooling_amd/ bind them with ctypes.
 *
 * Conventions
 *   - every tensor is fp32, row-major; `ld*` is a row stride in ELEMENTS; batch-major [B, n, ·]
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns every
 *     buffer including the workspace; the library never allocates, frees or retains memory
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no call synchronises the
 *     device, so every entry point can be captured into a hipGraph
 *   - return value: 0 = ok; < 0 = argument / workspace error detected before any launch
 *     (DP_ERR_*); > 0 = the hipError_t of a failed launch.  dp_last_error_string() describes the
 *     last failure of the calling thread.  No C++ exception crosses this boundary.
 *   - `num_nodes` is int32[B] on the device (it replaces the host-built mask of
 *     construct_mask, encoders.py:1035-1046); NULL means "no masking"
 */
#ifndef DIFFPOOL_HIP_H
#define DIFFPOOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden */
#endif

#define DP_VERSION 100 /* 0.1.0 */

#define DP_OK 0
#define DP_ERR_INVALID_ARG (-1)
#define DP_ERR_WORKSPACE (-2)
#define DP_ERR_UNSUPPORTED (-3)
#define DP_ERR_DEVICE (-4)      /* a kernel enqueued by an EARLIER call on this device reported a failure */

/* layer flags */
#define DP_F_ADD_SELF 1   /* y += x before the weight (GraphConv add_self, encoders.py:966-967) */
#define DP_F_NORMALIZE 2  /* F.normalize(p=2, dim=2), encoders.py:971-972 */
#define DP_F_RELU 4
#define DP_F_BN 8         /* apply_bn after ReLU, encoders.py:1062-1064 */
#define DP_F_LAST_ONLY 16 /* readout of the last layer only (concat=False, encoders.py:1118-1119) */

#define DP_MAX_LAYERS 8
#define DP_MAX_LEVELS 4   /* pooling levels */
#define DP_MAX_PRED 4     /* hidden layers of pred_model */

int dp_version(void);
const char* dp_last_error_string(void);

/* Device-side failures.  Calls only ENQUEUE work, so a failure inside a kernel cannot be the return value of the call
 * that launched it.  Such a kernel raises a bit in a per-device word that lives in pinned, device-mapped HOST memory
 * (64 bytes per device, allocated on first use; the one allocation this library makes — no device memory, no sync):
 *   DP_DEVERR_BARRIER         a whole-level kernel's grid barrier gave up (its workgroups were not co-resident: the
 *                             device is shared with another process / stream).  The kernel also poisons its BatchNorm
 *                             statistics with NaN, so the step's outputs and gradients are NaN, never plausible.
 *   DP_DEVERR_NONFINITE_GRAD  dp_clip_adam_step met a non-finite gradient norm and SKIPPED the update (parameters and
 *                             moments untouched) — which is also what keeps a poisoned backward from ruining them.
 * The NEXT model-level entry on that device (dp_encoder_forward / _backward, dp_loss_forward / _backward, their
 * _packed forms, dp_clip_adam_step) finds the word set, clears it, returns DP_ERR_DEVICE before launching anything and
 * describes it in dp_last_error_string().  dp_device_error(clear) reads the current device's word directly (after a stream or
 * device synchronisation it is up to date); dp_device_error_describe(mask) is the text for a mask.  Escape hatch for
 * shared devices: DP_NO_L0_PERSIST=1 DP_NO_LEVEL_FUSION=1 together (no kernel with a grid barrier is used; either one
 * alone leaves the level-0 or the pooled-level whole-level kernels in place). */
#define DP_DEVERR_BARRIER 1
#define DP_DEVERR_NONFINITE_GRAD 2
int dp_device_error(int clear);
const char* dp_device_error_describe(int mask);

/* Launch timing of the two persistent level-0 kernels (k_level0_fwd / k_level0_bwd, dp_level0.hip) for bench.py's
 * roofline object: dp_profile_level0(1) makes every EAGER launch of them (a capturing stream is left alone) record a
 * pair of HIP events on the launch stream; dp_profile_level0_read(which, &us, &n) waits for the pairs recorded so far
 * and returns their summed elapsed time in microseconds and their number (which: 0 forward, 1 backward);
 * dp_profile_level0(0) switches it off and drops the pairs.  No reference counterpart (measurement only). */
int dp_profile_level0(int enable);
int dp_profile_level0_read(int which, double* total_us, int* launches);

/* Which form of dS = A (S dA'^T) + ... the LAST persistent level-0 backward on the current device took, per graph
 * (encoders.py:1279; for tests and diagnosis, not fast: it synchronises the device).  The forward kernel decides per
 * graph, exactly and on the device, whether the adjacency is bf16-exact and equal to its transpose bit for bit; for
 * such a graph A S is the saved A^T S and the backward kernel multiplies that instead of aggregating over A again.
 * verdicts[b] = 1: graph b took the short form, 0: the general one; *count = graphs of that launch (0 when no such
 * launch has run); at most `capacity` verdicts are written.  *rows_per_block (may be NULL) = the rows of a graph one
 * workgroup of that launch owned (16, 32, 48 or 64: the kernel instantiation; ceil(N / rows) workgroups per graph). */
int dp_level0_bwd_symmetric(int* verdicts, int capacity, int* count, int* rows_per_block);

/* ------------------------------------------------------------------ generic contraction
 * C[b] = act(alpha * op(A[b]) op(B[b]) + beta * C[b] + bias), fp32 MFMA (exact f32).
 * Replaces torch.matmul / @ at encoders.py:965,968,1278,1279,1311.  act: 0 none, 1 relu. */
int dp_bgemm_f32(const float* A, const float* B, float* C, const float* bias, int batch, int M, int N,
                 int K, int lda, int ldb, int ldc, long strideA, long strideB, long strideC, int transA,
                 int transB, float alpha, float beta, int act, void* stream);

/* Groups of up to DP_GEMM_GROUP_MAX contractions (same batch count) in ONE launch, optionally with K cut into `ksplit`
 * ranges run by different workgroups — the form the encoder's backward and pooling products use.  No reference
 * counterpart (the reference issues one torch.matmul per product).  Per problem, `split` says how the ranges combine:
 *   DP_GEMM_WHOLE_K   this problem walks its whole K in one workgroup whatever `ksplit` is (a sibling of split ones)
 *   DP_GEMM_ATOMIC    C += alpha * op(A) op(B) with float atomics (no bias, act or beta: C is accumulated into)
 *   DP_GEMM_SLABS     range ks writes alpha * (its partial product) + beta * (old value) at C + ks * sK, ranges
 *                     without any k write the beta term alone; the caller sums the slabs (no bias or act)
 *   DP_GEMM_TICKETS   every range stores its partial to the workspace, the last to arrive adds them in range order and
 *                     applies the full epilogue once: bit-reproducible
 * Strides sA, sB, sC and sK are in elements.  `bias` is tested for NULL only by the plan query. */
#define DP_GEMM_GROUP_MAX 4
#define DP_GEMM_WHOLE_K 0
#define DP_GEMM_ATOMIC 1
#define DP_GEMM_SLABS 2
#define DP_GEMM_TICKETS 3
typedef struct {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    int M, N, K, lda, ldb, ldc;
    int64_t sA, sB, sC;
    int tA, tB;
    float alpha, beta;
    int act;
    int split;
    int64_t sK;
} dp_gemm_problem;
size_t dp_sizeof_gemm_problem(void); /* sizeof(dp_gemm_problem): lets a binding check its struct layout */

/* dp_bgemm_plan: what the launcher does with each problem of such a group (dp_bgemm_f32 is a group of one at
 * ksplit = 1, split = DP_GEMM_WHOLE_K) — answered by the function the launcher itself decides with.  Host only: no GPU
 * call, and no pointer of `p` is read.  plan_out[i] is
 *   DP_GEMM_PLAN_NONE        not launched (M or N = 0)
 *   DP_GEMM_PLAN_SPLIT_BF16  diverted to the split-bf16 kernel (dp_bgemm_split_bf16), a launch of its own
 *   otherwise                DP_GEMM_PLAN(BM, BN, quad, ranges): the BM x BN workgroup tile of the launch the problem
 *                            ends up in (a mixed group worth more than 0.5 GFLOP is split into one launch per shape
 *                            class), quad = 1 for the 16-byte operand loader, 0 for the 4-byte one, and the number of
 *                            K ranges that are launched (ranges that would start past K are not, except with slabs).
 * Returns DP_OK, or DP_ERR_INVALID_ARG for a count, batch or ksplit out of range. */
#define DP_GEMM_PLAN_NONE 0
#define DP_GEMM_PLAN_SPLIT_BF16 1
#define DP_GEMM_PLAN(bm, bn, quad, ranges) (((bm) << 20) | ((bn) << 12) | ((quad) << 11) | (ranges))
#define DP_GEMM_PLAN_BM(plan) ((plan) >> 20)
#define DP_GEMM_PLAN_BN(plan) (((plan) >> 12) & 255)
#define DP_GEMM_PLAN_QUAD(plan) (((plan) >> 11) & 1)
#define DP_GEMM_PLAN_RANGES(plan) ((plan) & 2047)
#define DP_GEMM_MAX_KSPLIT 2047
int dp_bgemm_plan(const dp_gemm_problem* p, int count, int batch, int ksplit, int* plan_out);

/* dp_bgemm_group_f32 launches the group.  The workspace (dp_bgemm_group_workspace_bytes) holds the partials
 * [batch][ksplit][M][N] and the tickets of the DP_GEMM_TICKETS problems; the tickets are zero-filled on the stream in
 * front of the launch.  Refused with DP_ERR_INVALID_ARG before any launch: count > DP_GEMM_GROUP_MAX, leading
 * dimensions smaller than the rows, bias / act / beta with DP_GEMM_ATOMIC, bias / act with DP_GEMM_SLABS, sK <= 0 with
 * DP_GEMM_SLABS. */
size_t dp_bgemm_group_workspace_bytes(const dp_gemm_problem* p, int count, int batch, int ksplit);
int dp_bgemm_group_f32(const dp_gemm_problem* p, int count, int batch, int ksplit, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The same contraction (alpha = 1, beta in {0, 1}, no bias / activation) with BOTH fp32 operands split exactly into
 * three bf16 planes on the way to LDS and multiplied on the bf16 matrix cores — six plane products, fp32 accumulation;
 * the dropped cross terms are <= 2^-23 of a product, so the result is fp32-grade (not bit-identical to dp_bgemm_f32).
 * dp_bgemm_f32 and the encoder plans take this kernel by themselves for large shapes (M, N >= 96, K >= 64, >= 256
 * output tiles of 128 x 128); this entry runs it on any shape with every extent >= 4 (smaller ones: dp_bgemm_f32). */
int dp_bgemm_split_bf16(const float* A, const float* B, float* C, int batch, int M, int N, int K, int lda, int ldb,
                        int ldc, long strideA, long strideB, long strideC, int transA, int transB, float beta,
                        void* stream);

/* ------------------------------------------------------------------ adjacency aggregation
 * U[b] = op(adj[b]) · V[b] (+ beta U[b]):  adj [B,n,n], V [B,n,C] (ldv), U [B,n,C] (ldu); trans != 0 uses
 * adj^T.  The HBM-bound pass over the padded dense adjacency — torch.matmul(adj, x), encoders.py:965,
 * and its transpose in backward — as the LDS-panel kernel (any shape; shapes the panel kernel does not
 * take run on dp_bgemm_f32's kernel). */
int dp_adj_aggregate(const float* adj, const float* V, int ldv, float* U, int ldu, int B, int n, int C,
                     int trans, float beta, void* stream);

/* Packed adjacency (the reference multiplies the same fp32 adjacency 12 times per step, encoders.py:965,1279,
 * 1311).  dp_adj_pack makes ONE pass over adj [B,n,n] and writes bf16 copies of A and A^T (rows padded to
 * dp_adj_pack_ld(n) elements) plus a device flag that is 0 iff every entry is exactly representable in bf16
 * (always true for the 0/1 adjacency of graph_sampler.py:26).  dp_adj_aggregate_packed then computes the same
 * U = op(adj)·V with V split exactly into three bf16 planes (fp32-grade result, bf16 MFMA rate, half the
 * adjacency bytes) when the flag is 0, and with the fp32 loop otherwise — decided on the device, no sync.
 * `flag` points at a 256-byte, 16-byte-aligned device block: dp_adj_pack clears all of it and sets only word 0. */
int dp_adj_pack_ld(int n);
size_t dp_adj_pack_bytes(int B, int n);            /* bytes of ONE packed copy */
int dp_adj_pack(const float* adj, void* packed, void* packed_t, int* flag, int B, int n, void* stream);
/* dp_adj_pack as the encoder plans call it, with the side job: the pack launch's workgroups also clear zero_bytes bytes
 * at zero_p between them (a region that is not 16-byte aligned or no multiple of 16 bytes gets a launch of its own).
 * zero_p must not be NULL; zero_bytes = 0 is allowed and clears nothing. */
int dp_adj_pack_zero(const float* adj, void* packed, void* packed_t, int* flag, int B, int n, void* zero_p,
                     size_t zero_bytes, void* stream);
size_t dp_adj_aggregate_packed_workspace_bytes(int B, int n, int C);
/* presplit != 0: the workspace already holds the 3-plane split of this V from an earlier call (skips the split
 * pass — the encoder plan gets the split from V's producer kernel the same way). */
int dp_adj_aggregate_packed(const float* adj, const void* packed, const void* packed_t, const int* flag,
                            const float* V, int ldv, float* U, int ldu, int B, int n, int C, int trans, float beta,
                            int presplit, void* workspace, size_t workspace_bytes, void* stream);

/* dp_adj_aggregate_plan: what the two aggregation launchers (dp_adj_aggregate[_packed], dp_adj_aggregate_rownorm and
 * the encoder plans) launch for a shape, answered by the one host function both decide with.  Host only: no GPU call.
 * packed != 0: a packed adjacency and a workspace are given; fused != 0: the GraphConv-tail entry (trans and beta are
 * ignored); a_misalign: the low four bits of adj's address (0: 16-byte aligned).
 * plan_out[DP_AGG_PLAN_INTS] = { form (DP_AGG_FORM_*), CT (the kernel's column tiles; 0 for the GEMM forms), RT (panel
 * forms: rows per workgroup, 16 / 32; wide forms: waves per workgroup, 4 / 8), row tiles per graph, workgroups, dynamic
 * LDS bytes, fallback (DP_AGG_FB_*: the launch queued behind a wide form that runs only when the pack flag is set), the
 * fallback panel launch's CT, RT, row tiles, workgroups and LDS bytes (0 unless DP_AGG_FB_PANEL), split (1: V is split
 * into its three bf16 planes — the panel-bf16 and wide forms; 0 for every other form, also when a packed operand was given), declines (fused only: 1 = the entry launches nothing and the caller takes `form` through
 * dp_adj_aggregate[_packed]) }.  The tiles of the GEMM forms are dp_bgemm_plan's to report. */
#define DP_AGG_FORM_PANEL_F32 0       /* k_aggregate, fp32 loop */
#define DP_AGG_FORM_PANEL_BF16 1      /* k_aggregate on the packed operand (fp32 loop in the same launch if the flag is set) */
#define DP_AGG_FORM_WIDE 2            /* k_aggregate_wide: 128 rows x all columns, C <= 128 */
#define DP_AGG_FORM_WIDE_DMA 3        /* k_aggregate_wide_dma: 128 < C <= 320 */
#define DP_AGG_FORM_GEMM_F32 4        /* dp_bgemm_f32's kernel */
#define DP_AGG_FORM_GEMM_SPLIT_BF16 5 /* dp_bgemm_split_bf16's kernel */
#define DP_AGG_FB_NONE 0
#define DP_AGG_FB_PANEL 1
#define DP_AGG_FB_GEMM 2
#define DP_AGG_PLAN_INTS 14
int dp_adj_aggregate_plan(int B, int n, int C, int trans, int packed, int fused, int a_misalign, float beta,
                          int* plan_out);

/* ------------------------------------------------------------------ A1  GraphConv
 * y = l2norm((adj @ x [+ x]) @ W + b)   — GraphConv.forward, encoders.py:962-974.
 * x [B,n,Fin] (ldx), adj [B,n,n], W [Fin,Fout], bias [Fout] or NULL, y [B,n,Fout] (ldy),
 * invnorm [B,n] (saved for backward, may be NULL).  flags: DP_F_ADD_SELF | DP_F_NORMALIZE.
 * Workspace: dp_gcn_layer_workspace_bytes(). */
size_t dp_gcn_layer_workspace_bytes(int B, int n, int Fin, int Fout);
int dp_gcn_layer_fwd(const float* x, int ldx, const float* adj, const float* W, const float* bias,
                     float* y, int ldy, float* invnorm, int B, int n, int Fin, int Fout, int flags,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the above. dx / dadj may be NULL (not needed). dW [Fin,Fout] and db [Fout] are
 * OVERWRITTEN. */
int dp_gcn_layer_bwd(const float* x, int ldx, const float* adj, const float* W, const float* y, int ldy,
                     const float* invnorm, const float* dy, int lddy, float* dx, int lddx, float* dW,
                     float* db, float* dadj, int B, int n, int Fin, int Fout, int flags, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ A3  apply_bn
 * Batch-norm over the node index with batch statistics (a fresh BatchNorm1d(n) per call,
 * encoders.py:1048-1052): per node n, mean / biased variance over (batch, feature), eps 1e-5.
 * stats [n,2] receives (mean, rstd).  relu != 0 applies ReLU first (encoders.py:1062). */
size_t dp_bn_node_workspace_bytes(int B, int n, int F);
int dp_bn_node_fwd(const float* x, int ldx, float* y, int ldy, float* stats, int B, int n, int F,
                   int relu, void* workspace, size_t workspace_bytes, void* stream);
/* dx from dy; y is the forward OUTPUT (xhat), x the forward input (used for the ReLU mask when
 * relu != 0, may be NULL otherwise). */
int dp_bn_node_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy,
                   int lddy, float* dx, int lddx, int B, int n, int F, int relu, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ A5  assignment head
 * S = softmax_K(z @ Wp^T + bp) * mask — encoders.py:1273-1275. z [B,n,Din] (ldz), Wp [K,Din]
 * (nn.Linear layout), S [B,n,K]. */
size_t dp_assign_workspace_bytes(int B, int n, int Din, int K);
int dp_assign_softmax_mask_fwd(const float* z, int ldz, const float* Wp, const float* bp,
                               const int* num_nodes, float* S, int B, int n, int Din, int K,
                               void* workspace, size_t workspace_bytes, void* stream);
int dp_assign_softmax_mask_bwd(const float* z, int ldz, const float* Wp, const float* S, const float* dS,
                               const int* num_nodes, float* dz, int lddz, float* dWp, float* dbp, int B,
                               int n, int Din, int K, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------ A6  pooling
 * Xp = S^T Z [B,K,D], Ap = S^T A S [B,K,K] — encoders.py:1278-1279.
 * T [B,K,n] receives S^T A (saved for backward). */
int dp_pool_fwd(const float* S, const float* Z, int ldz, const float* adj, float* Xp, float* Ap, float* T,
                int B, int n, int K, int D, void* stream);
/* dS [B,n,K] (overwritten), dZ [B,n,D] (lddz; ACCUMULATED INTO), dadj [B,n,n] or NULL
 * (accumulated into). */
size_t dp_pool_bwd_workspace_bytes(int B, int n, int K, int D);
int dp_pool_bwd(const float* S, const float* Z, int ldz, const float* adj, const float* T, const float* dXp,
                const float* dAp, float* dS, float* dZ, int lddz, float* dadj, int B, int n, int K, int D,
                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ A7  max readout
 * out[b,f] = max_n (Z * mask)[b,n,f] — encoders.py:1079-1080,1257,1287.  argmax [B,F] int32
 * (-1 where a masked zero row wins: no gradient). */
int dp_masked_max_fwd(const float* Z, int ldz, const int* num_nodes, float* out, int ldo, int* argmax,
                      int B, int n, int F, void* stream);
/* dZ is ACCUMULATED INTO. */
int dp_masked_max_bwd(const float* dout, int ldo, const int* argmax, float* dZ, int lddz, int B, int n,
                      int F, void* stream);

/* ------------------------------------------------------------------ row kernels, as the encoder plans call them
 * The row-wise launchers behind the entries above (GraphConv tail, node BatchNorm, assignment softmax, column sums),
 * passed straight through with every optional operand: up to two column groups of a joint buffer, per-group outputs
 * with their own leading dimensions, BatchNorm partials, bias-gradient slabs, the 3-plane bf16 split (`vs`, the
 * layout dp_adj_aggregate_packed reads: Vs[b][plane][cb][k8][c][j], ((n + 31) / 32) * 4 k8 groups) and the folded
 * zero-fill.  No reference counterpart; they exist so that every compiled form can be tested on its own.
 *
 * dp_row_groups: G = 1 or 2 groups, group i is columns c0[i] .. c0[i] + w[i] of the joint buffer (c0 ascending, no
 * overlap).  dp_group_ptrs: per group a pointer ALREADY at the group's first column, and its leading dimension. */
typedef struct {
    int G;
    int c0[2];
    int w[2];
} dp_row_groups;
typedef struct {
    void* p[2];
    int ld[2];
} dp_group_ptrs;
size_t dp_sizeof_row_groups(void);
size_t dp_sizeof_group_ptrs(void);

/* dp_rowop_plan: the form a launcher takes, answered by the host function the launcher itself decides with.  Host
 * only: no GPU call.  `g` holds the groups (softmax: K = g->w[0]; masked max: unused, may be NULL); Bs = graphs the
 * BatchNorm statistics span (0: B).  flags: DP_ROWF_STATS (bn_apply_fwd: `part` given; rownorm_bwd: has_bn),
 * DP_ROWF_VS, DP_ROWF_ZERO (a zero region is given), DP_ROWF_ZERO_UNALIGNED (it is not 16-byte aligned or not a
 * multiple of 16 bytes), DP_ROWF_DBIAS (softmax_mask_bwd: a bias-gradient slab is given).
 * plan_out[DP_ROWOP_PLAN_INTS] = { kernel (DP_ROWK_*), NK (0: the any-width form; masked max: 32 = all rows of a thread
 * in one batch of loads, n <= 512), quad (1: 16-byte lanes), finalize (1: k_bn_finalize / k_bn_bwd_finalize runs in
 * front), generic (1: the generic softmax kernel, no _plan form), zero (DP_ROWZ_*) }. */
#define DP_ROWOP_ROWNORM_FWD 0
#define DP_ROWOP_ROWNORM_BWD 1
#define DP_ROWOP_BN_APPLY_FWD 2
#define DP_ROWOP_SOFTMAX_FWD 3
#define DP_ROWOP_SOFTMAX_BWD 4
#define DP_ROWOP_MASKED_MAX_FWD 5
#define DP_ROWK_ROWNORM_FWD 0
#define DP_ROWK_ROWNORM_BWD 1
#define DP_ROWK_BN_APPLY_FWD 2
#define DP_ROWK_SOFTMAX_FWD_PLAN 3
#define DP_ROWK_SOFTMAX_FWD 4
#define DP_ROWK_SOFTMAX_BWD_PLAN 5
#define DP_ROWK_SOFTMAX_BWD 6
#define DP_ROWK_MASKED_MAX_FWD 7
#define DP_ROWF_STATS 1
#define DP_ROWF_VS 2
#define DP_ROWF_ZERO 4
#define DP_ROWF_ZERO_UNALIGNED 8
#define DP_ROWF_DBIAS 16
#define DP_ROWZ_NONE 0
#define DP_ROWZ_FOLDED 1 /* the softmax kernel's own workgroups clear the region */
#define DP_ROWZ_APART 2  /* a zero-fill launch of its own in front */
#define DP_ROWOP_PLAN_INTS 6
int dp_rowop_plan(int op, const dp_row_groups* g, int n, int B, int Bs, int flags, int* plan_out);

/* Every entry below refuses with DP_ERR_INVALID_ARG, before any launch: G outside 1..2, a width below 1, overlapping
 * or descending groups, a leading dimension smaller than its rows, NULL required pointers, and a `vs` request the
 * launcher has no form for (see each entry).
 *
 * y_g = u / max(||u||, 1e-12), u = U[row, c0_g + c] (+ P[row, c0_g + c]) (+ bias_g[c]); normalize = 0: y = u.
 * P (same ld as U) and bias (NULL, or per group NULL / [w_g]) are optional.  invn [rows, G] (NULL, or 1 / max(||u||, eps)
 * out).  stats_mode 1 / 2 with part [rows, G, 2]: (row mean, row M2) of relu(y) / of y. */
int dp_rownorm_fwd(const float* U, int ldu, const float* P, const dp_row_groups* g, const dp_group_ptrs* bias,
                   const dp_group_ptrs* yout, float* invn, float* part, long rows, int normalize, int stats_mode,
                   void* stream);
/* The same tail fused behind the aggregation, as the encoder plans call it: u = adj[b] V[b] (+ P) (+ bias_g) over the
 * joint width C = c0[G-1] + w[G-1] of V [B, n, C] (ldv; P has V's layout), one launch (plus the flag-gated fallback
 * behind a wide form).  packed / packed_t / flag / workspace (dp_adj_aggregate_packed_workspace_bytes) are given
 * together or not at all; presplit as in dp_adj_aggregate_packed.  Returns DP_AGG_DECLINED for the shapes
 * dp_adj_aggregate_plan reports as declined: not an error — the arguments were accepted, nothing was launched and no
 * error string is set; the caller then runs dp_adj_aggregate[_packed] + dp_rownorm_fwd.  The value is negative so that it
 * can be neither DP_OK nor the hipError_t of a failed launch (> 0), and it is no DP_ERR_* code.
 * The groups must cover the joint width without a gap (c0[0] = 0, c0[1] = w[0]), as the encoder's do. */
#define DP_AGG_DECLINED (-5)
int dp_adj_aggregate_rownorm(const float* adj, const void* packed, const void* packed_t, const int* flag,
                             const float* V, int ldv, const float* P, const dp_row_groups* g,
                             const dp_group_ptrs* bias, const dp_group_ptrs* yout, float* invn, float* part, int B, int n,
                             int normalize, int stats_mode, int presplit, void* workspace, size_t workspace_bytes,
                             void* stream);
/* x = (relu?(y) - mu_n) * rstd_n per node index n and group, the statistics Chan-combined from part [Bs, n, G, 2]
 * (Bs = 0: B; Bs > B: the statistics span more graphs than the B normalised here); stats [n, G, 2] receives (mu, rstd).
 * part = NULL: no BatchNorm (ReLU only), stats unused. */
int dp_bn_apply_fwd(const float* Y, int ldy, const float* part, float* stats, const dp_row_groups* g,
                    const dp_group_ptrs* xout, int B, int n, int relu, int Bs, void* stream);
/* part [rows, G, 2] = (sum_c dx, sum_c dx * xhat) per row and group */
int dp_bn_bwd_partials(const dp_row_groups* g, const dp_group_ptrs* dx, const dp_group_ptrs* xhat, float* part,
                       long rows, void* stream);
/* dx -> (BatchNorm bwd, has_bn) -> (ReLU bwd, has_relu) -> (l2-normalise bwd, normalize) -> dU [B * n, ldu] at the
 * groups' columns.  part2 [Bs, n, G, 2] from dp_bn_bwd_partials (OVERWRITTEN when Bs > 32); dbias: NULL, or per group
 * NULL / the slab row of graph 0, graphs ld >= w_g apart — the column sums of dU are ADDED.  vs: NULL, or the 3-plane split of
 * dU [B, n, c0[G-1] + w[G-1]] out (16-byte aligned; refused when slabs + split need more than 64 KiB of LDS). */
int dp_rownorm_bwd(const dp_row_groups* g, const dp_group_ptrs* dx, const dp_group_ptrs* xhat,
                   const dp_group_ptrs* y, const float* invn, const float* stats, float* part2, float* dU, int ldu,
                   const dp_group_ptrs* dbias, int B, int n, int has_relu, int has_bn, int normalize, void* vs, int Bs,
                   void* stream);
/* S = softmax_K(logits) on rows n < num_nodes[b] (NULL: all), 0 elsewhere; S2: NULL or a second copy (ld lds);
 * vs: NULL or the 3-plane split of S out (16-byte aligned; refused for K > 768, where no plan form exists);
 * zero_p / zero_bytes: a region to clear on the way. */
int dp_softmax_mask_fwd(const float* logits, int ldl, float* S, int lds, const int* num_nodes, int B, int n, int K,
                        float* S2, void* vs, void* zero_p, size_t zero_bytes, void* stream);
/* dlogits = S * (dS (+ dS2) - <dS (+ dS2), S>).  dbias: NULL, or the slab row of graph 0 (graphs dbias_stride apart) the
 * column sums of dlogits are ADDED to.  dS2: NULL or a second addend, ld ldds.  Without dbias (and for K > 1024) dS2 is
 * first ADDED INTO dS, as one run of B * n * ldds floats: there both buffers must hold B * n * ldds floats — the last
 * row its full ldds too — and the padding of dS receives the padding of dS2. */
int dp_softmax_mask_bwd(const float* S, int lds, float* dS, int ldds, const int* num_nodes, float* dlogits, int ldl,
                        int B, int n, int K, float* dbias, long dbias_stride, const float* dS2, void* stream);
/* out[b, c] = sum_r X[b, r, c]; rowsplit > 1: `rowsplit` row ranges ADD into out with float atomics */
int dp_colsum_batched(const float* X, int ldx, long strideX, int rows, int cols, float* out, long strideOut, int batch,
                      int rowsplit, void* stream);

/* ------------------------------------------------------------------ A8  link-prediction loss
 * loss = sum_{n,m < n_b} [-A log(P+1e-7) - (1-A) log(1-P+1e-7)] / sum_b n_b^2,
 * P = min(S S^T, 1) — encoders.py:1309-1331 (adj_hop = 1).  loss_out: 1 float.  K <= 256 (DP_ERR_UNSUPPORTED above).
 * The adjacency comes either as the dense fp32 batch adj [B,n,n] or, in the _packed entries, in the packed form of
 * dp_adj_pack / dp_build_batch_packed: bf16 rows [B, n, dp_adj_pack_ld(n)] of A (adj_pk) and of A^T (adj_pkt; the same
 * buffer for a symmetric adjacency), both 16-byte aligned.  The two forms run the same tile walk, so on a bf16-exact
 * adjacency (0/1) they give bit-identical loss and dS.  dp_linkpred_workspace_bytes covers both forms.
 * n_b = num_nodes[b] clamped to n (NULL: n).  A graph with n_b = 0 beside non-empty ones contributes nothing to the loss
 * or to the normaliser, and its rows of dS are exactly 0 (left as they were under accumulate); a batch whose every n_b is
 * 0 has no normaliser and is not a valid input.
 *
 * dp_linkpred_plan(B, n, K): the kernels and the split that shape runs, answered by the host function the launchers
 * themselves decide with.  Host only: no GPU call; the same for both adjacency forms.
 * plan_out[DP_LINKPRED_PLAN_INTS] = { KT (the kernels' K tier: 16-column tiles, one of 1 2 3 4 6 8 12 16), CW (width of
 * the column tiles the backward walks: 64, or 32 for KT >= 12), col_tiles = ceil(n / CW), splits (column ranges the
 * backward's grid is split into so that a small batch still fills the chip, aiming at 512 workgroups; 1 = the non-split
 * form: no gradient partials, no reduce pass), split_tiles (column tiles per split; the last split may hold fewer),
 * forward workgroups (= loss partials) per graph = ceil(n / 64)^2, the forward kernel's dynamic LDS bytes, the backward
 * kernel's dynamic LDS bytes }.  The backward figure is the fp32 reader's: the packed reader holds no transposed A tile
 * in LDS and needs CW * 65 * 4 bytes less.  DP_ERR_UNSUPPORTED for K > 256, DP_ERR_INVALID_ARG for a NULL plan_out or
 * B, n, K < 1. */
#define DP_LINKPRED_PLAN_INTS 8
int dp_linkpred_plan(int B, int n, int K, int* plan_out);
size_t dp_linkpred_workspace_bytes(int B, int n, int K);
int dp_linkpred_loss_fwd(const float* S, const float* adj, const int* num_nodes, float* loss_out, int B,
                         int n, int K, void* workspace, size_t workspace_bytes, void* stream);
/* dS (+)= dloss * d loss / dS.  dloss: device pointer to 1 float (NULL = 1.0). */
int dp_linkpred_loss_bwd(const float* S, const float* adj, const int* num_nodes, const float* dloss,
                         float* dS, int accumulate, int B, int n, int K, void* workspace,
                         size_t workspace_bytes, void* stream);
int dp_linkpred_loss_fwd_packed(const float* S, const void* adj_pk, const int* num_nodes, float* loss_out, int B,
                                int n, int K, void* workspace, size_t workspace_bytes, void* stream);
int dp_linkpred_loss_bwd_packed(const float* S, const void* adj_pk, const void* adj_pkt, const int* num_nodes,
                                const float* dloss, float* dS, int accumulate, int B, int n, int K, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ assignment entropy (DiffPool's second auxiliary term)
 * E = ( sum_b sum_{i < n_b} sum_k -s_bik ln(s_bik + 1e-15) ) / sum_b n_b over S [B, n, K] (rows lds apart), the epsilon
 * added in fp32.  n_b = num_nodes[b] clamped into [0, n]; num_nodes NULL = every row valid (then B = 1, n = rows serves
 * a ragged [rows, K] assignment, rows counted in 64 bits).  The normaliser counts VALID nodes, not B * n: padding does
 * not shrink the term (no valid node at all: E = 0).  Rows i >= n_b are never read.  Terms are formed in fp32 and
 * summed in fp64 in a fixed order (no atomics): E is bit-identical from run to run.  Any K >= 1, lds / ldds >= K, any
 * 4-byte alignment (16-byte lanes are taken when pointers, leading dimensions and K allow).  NULL S / ent_out / dS /
 * workspace, B, n or K < 1, lds or ldds < K and a short workspace are DP_ERR_INVALID_ARG before any launch.  Nothing
 * allocates or synchronises: both entries can be captured into a hipGraph.
 * ent_out[0] = E.  total_inout: NULL, or one float that weight * E is ADDED to (fp32: old + fl(weight * E)) by the
 * launch that finishes the sum. */
size_t dp_assign_entropy_workspace_bytes(int B, int n, int K);
int dp_assign_entropy_fwd(const float* S, int lds, const int* num_nodes, float weight, float* ent_out,
                          float* total_inout, int B, int n, int K, void* workspace, size_t workspace_bytes,
                          void* stream);
/* dS (+)= dloss * weight * dE/dS,  dE/ds = -(ln(s + 1e-15) + s / (s + 1e-15)) / sum_b n_b.  dloss: device scalar or
 * NULL = 1.  Rows i >= n_b: written 0 (accumulate = 0) or left as they are (accumulate = 1); columns K..ldds-1 are
 * never written. */
int dp_assign_entropy_bwd(const float* S, int lds, const int* num_nodes, const float* dloss, float weight,
                          float* dS, int ldds, int accumulate, int B, int n, int K, void* stream);

/* ------------------------------------------------------------------ Frobenius link loss (the DiffPool paper's L_LP, squared)
 *     link = sum_b sum_{i,j < n_b} (a_bij - s_bi . s_bj)^2 / sum_b n_b^2
 * on the level-0 assignment: all pairs count, the diagonal included, no clamp; link * sum_b n_b^2 is the paper's
 * ||A - S S^T||_F^2 summed over the graphs.  The reference has no such term (its link term is the cross-entropy form of
 * A8): the definition is unpinned by the reference.  Evaluated without any n x n temporary as T0 - sum_i s_i . w_i +
 * sum_b ||G_b||_F^2 with T0 = sum a^2, W = (A + A^T) S and G_b = S_b^T S_b [K, K]; the backward is row-local,
 * dS_i (+)= dloss (4 G_b s_i - 2 w_i) / norm.  F is a difference of three non-negative sums: its absolute error scales
 * with T0 + sum s.w + T2, so near a perfect fit the RELATIVE error of the term is unbounded — inherent, not a defect.
 * G is summed in fp64 over row slabs of DP_FROB_LINK_SLAB global rows in a fixed order, the row term and T0 from fp32
 * products in fp64 in a fixed order, the quotient taken in fp64 and rounded once: no atomics, bit-identical repeats.
 *
 * S [B, N, K] (rows lds >= K apart), 1 <= K <= 256 (DP_ERR_UNSUPPORTED above, before any launch).  n_b = num_nodes[b]
 * clamped into [0, N], NULL = N.  Rows i >= n_b of S (and of W) are never read; adjacency entries outside the leading
 * n_b x n_b block are never read either.  link_norm (device scalar or NULL) replaces sum_b n_b^2, as in dp_loss_forward.
 * The forward writes W [B, N, K] (contiguous; rows i >= n_b are left as they are) and G [B, K, K], both caller-owned, for
 * the backward, which reads no adjacency.  loss_out[0] = link; total_inout: NULL, or one float the term is ADDED to
 * (fp32) by the launch that finishes the sum.  The fp32 entry takes any adjacency values (weighted, asymmetric); the
 * packed entry takes the bf16 rows of dp_adj_pack / dp_build_batch_packed (16-byte aligned, rows of dp_adj_pack_ld(N);
 * adj_pkt == adj_pk: one read and a factor 2) and equals the fp32 entry BIT FOR BIT on an adjacency bf16 holds exactly.
 * NULL pointers, B, N, K < 1, lds / ldds < K, a short workspace: DP_ERR_INVALID_ARG before any launch.  Nothing
 * allocates or synchronises, no memset / memcpy nodes: every entry can be captured into a hipGraph. */
#define DP_FROB_LINK_SLAB 512
size_t dp_frob_link_workspace_bytes(int B, int N, int K);
int dp_frob_link_fwd(const float* S, int lds, const float* adj, const int* num_nodes, const float* link_norm, float* W,
                     float* G, float* loss_out, float* total_inout, int B, int N, int K, void* workspace,
                     size_t workspace_bytes, void* stream);
int dp_frob_link_fwd_packed(const float* S, int lds, const void* adj_pk, const void* adj_pkt, const int* num_nodes,
                            const float* link_norm, float* W, float* G, float* loss_out, float* total_inout, int B, int N,
                            int K, void* workspace, size_t workspace_bytes, void* stream);
/* dloss: device scalar or NULL = 1.  accumulate = 0: rows i >= n_b are written 0; accumulate = 1: dS += and those rows
 * are left alone.  Columns K..ldds-1 are never written.  W / G: the forward's.  _bwd_packed is the same function under
 * the name of the forward it pairs with (the backward reads no adjacency). */
int dp_frob_link_bwd(const float* S, int lds, const float* W, const float* G, const int* num_nodes,
                     const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate, int B, int N, int K,
                     void* stream);
int dp_frob_link_bwd_packed(const float* S, int lds, const float* W, const float* G, const int* num_nodes,
                            const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate, int B,
                            int N, int K, void* stream);
/* The same term on CSR: one graph (n rows), or a ragged batch (block-diagonal CSR with GLOBAL column indices, node_off
 * int32 [B + 1] ON THE DEVICE, every graph >= 1 node) with one set of launches for the whole batch, none per graph.
 * CSR contract: 0/1 adjacency, each (i, j) stored at most once, so T0 is the number of stored entries (read from
 * indptr on the device).  W [n, K] = A S by the dp_csr_aggregate gather; indptr_t / indices_t: CSR of A^T, NULL or the
 * forward arrays themselves for an undirected graph (one gather, counted twice) — the backward is told with
 * symmetric != 0.  G [B, K, K].  Work O(n K^2 + nnz K), workspace O(n K + B K^2); a batch of one graph equals the
 * single-graph entry bit for bit. */
size_t dp_csr_frob_link_workspace_bytes(int n_total, int B, int K);
int dp_csr_frob_link_fwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                         const int* indices_t, const float* link_norm, float* W, float* G, float* loss_out,
                         float* total_inout, int n, int K, void* workspace, size_t workspace_bytes, void* stream);
int dp_csr_frob_link_bwd(const float* S, int lds, const float* W, const float* G, const float* link_norm,
                         const float* dloss, float* dS, int ldds, int accumulate, int symmetric, int n, int K,
                         void* stream);
int dp_csr_frob_link_batch_fwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                               const int* indices_t, const int* node_off, const float* link_norm, float* W, float* G,
                               float* loss_out, float* total_inout, int B, int n_total, int K, void* workspace,
                               size_t workspace_bytes, void* stream);
int dp_csr_frob_link_batch_bwd(const float* S, int lds, const float* W, const float* G, const int* node_off,
                               const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate,
                               int symmetric, int B, int n_total, int K, void* stream);
/* The weighted forms (a CSR that stores values, e.g. D^-1/2 A D^-1/2 of graph_sampler.py:27-29): values fp32 [nnz] in the
 * order of indices, values_t in the order of indices_t (needed only next to a transposed CSR of its own; NULL values, or
 * NULL values_t there, is DP_ERR_INVALID_ARG).  T0 = sum of the stored values' squares, summed in fp64 in a fixed order
 * by the row kernel; W = (A + A^T) S by dp_csr_aggregate_w.  Same launches and workspace as the unweighted entries; the
 * backward reads no adjacency: dp_csr_frob_link_bwd / _batch_bwd serve both.  Weights of 1.0 give the unweighted bits. */
int dp_csr_frob_link_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                           const int* indptr_t, const int* indices_t, const float* values_t, const float* link_norm,
                           float* W, float* G, float* loss_out, float* total_inout, int n, int K, void* workspace,
                           size_t workspace_bytes, void* stream);
int dp_csr_frob_link_batch_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                                 const int* indptr_t, const int* indices_t, const float* values_t, const int* node_off,
                                 const float* link_norm, float* W, float* G, float* loss_out, float* total_inout, int B,
                                 int n_total, int K, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ softmax cross entropy
 * loss = mean_b CE(logits_b, label_b) — F.cross_entropy, encoders.py:1127.  prob [B,C] is saved
 * for backward.  label: int64[B]. */
int dp_cross_entropy_fwd(const float* logits, const long long* label, float* loss_out, float* prob, int B,
                         int C, void* stream);
int dp_cross_entropy_bwd(const float* prob, const long long* label, const float* dloss, float* dlogits,
                         int B, int C, void* stream);

/* ------------------------------------------------------------------ A10  Set2Set
 * Set2Set.forward, set2set.py:32-57: n LSTM-attention steps over emb [B,n,d] -> out [B,d].
 * Weights in nn.LSTM layout: w_ih [4d,2d], w_hh [4d,d], b_ih [4d], b_hh [4d] (gates i,f,g,o);
 * pred: Wp [d,2d], bp [d].  `save` (dp_set2set_save_bytes) keeps per-step state for backward.
 * Limits: 1 <= n <= 1024 and 1 <= d <= 256 (one persistent workgroup per graph holds the recurrence); outside them
 * both calls return DP_ERR_UNSUPPORTED before any launch and touch no buffer.  n = 0 or d = 0 is DP_ERR_INVALID_ARG.
 * B = 0 is DP_OK without a kernel launch: the forward writes nothing, the backward zero-fills the six parameter
 * gradients (sums over no graph).
 * Strides: `lde` is the row stride of emb (graph b starts at emb + b*n*lde) and `ldde` that of demb, in elements, each
 * >= d.  Only the first d columns of a row are read / written; the columns beyond d are never touched, so emb and
 * demb may be column blocks of wider buffers.  out, dout and every parameter / parameter gradient are dense.
 * dp_set2set_plan(n, d): which k_set2set_* variant that shape runs (the forward and the backward take the same one) —
 * bit 0 weights in LDS, bit 1 embedding in LDS, bit 2 weights in registers; no bit set: both are read from global
 * memory.  DP_ERR_UNSUPPORTED (negative) outside the kernels' limits.  Host only: no GPU call, no error string. */
size_t dp_set2set_save_bytes(int B, int n, int d);
int dp_set2set_plan(int n, int d);
int dp_set2set_fwd(const float* emb, int lde, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, const float* Wp, const float* bp, float* out, int B, int n, int d,
                   void* save, size_t save_bytes, void* stream);
size_t dp_set2set_bwd_workspace_bytes(int B, int n, int d);
int dp_set2set_bwd(const float* emb, int lde, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, const float* Wp, const float* bp, const float* out, const float* dout,
                   float* demb, int ldde, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* dWp,
                   float* dbp, int B, int n, int d, const void* save, size_t save_bytes, void* workspace,
                   size_t workspace_bytes, void* stream);

/* A10 on a RAGGED batch (N4 conventions: graph b owns rows node_off[b] .. node_off[b+1]-1 of emb [n_total, .];
 * node_off int32 [B+1] on the device, node_off_host the same values on the host, read only by the host).  The batch
 * stands for the dense batch padded to T rows whose padded rows are exactly zero (the embedding mask,
 * encoders.py:1079-1080): the recurrence runs T steps, and with P_b = T - n_b zero rows, each with logit 0,
 *     m = max(max_i e_i, 0) if P_b > 0 else max_i e_i;  Z = sum_i exp(e_i - m) + P_b exp(-m);  a_i = exp(e_i - m) / Z
 * over the n_b real rows.  out [B,d] and the gradients are those of dp_set2set_fwd / _bwd on the padded batch (demb
 * [n_total, .]: real rows only).  A single graph is B = 1, T = n.  No row limit of 1024:
 * Limits: 1 <= d <= 256, 1 <= n_b <= DP_SET2SET_RAGGED_MAX_ROWS at every d, T >= max_b n_b, B <= 65535, B * T < 2^31.  d = 0, T = 0,
 * an empty graph, T < max_b n_b or a buffer too small: DP_ERR_INVALID_ARG; d > 256 or n_b above the bound:
 * DP_ERR_UNSUPPORTED; always before any launch, no buffer touched.  B = 0 as dp_set2set_*.
 * One persistent workgroup per graph; dp_set2set_ragged_plan(n_b, d) is the variant a graph of n_b rows runs, in the
 * bits of dp_set2set_plan: bit 1 the graph's embedding is staged in LDS (else read from global memory every step),
 * bit 2 the LSTM weights sit in registers (d <= 64; else read from global memory); bit 0 is never set.  A pass launches
 * one grid per bit-1 value present in the batch, so launch counts do not depend on B.  Host only.
 * Memory: the backward keeps a_t and de_t of every step, [T, n_b] per graph: `save` holds T * n_total floats of a_t
 * plus 8 * B * T * d of LSTM state, the backward workspace T * n_total floats of de_t plus 5 * B * T * d; the size
 * queries (host only, computed in size_t) return 0 for arguments the entries refuse.  save == NULL in the forward is
 * inference: nothing is saved and no T x n_b array is touched; `out` is bit for bit that of a saving run.
 * lde / ldde >= d are row strides as in A10; columns beyond d are never touched.  No atomics: fixed summation order,
 * two runs agree bit for bit. */
#define DP_SET2SET_RAGGED_MAX_ROWS 16384
int dp_set2set_ragged_plan(int n_b, int d);
size_t dp_set2set_ragged_save_bytes(const int* node_off_host, int B, int T, int d);
size_t dp_set2set_ragged_bwd_workspace_bytes(const int* node_off_host, int B, int T, int d);
int dp_set2set_ragged_fwd(const float* emb, int lde, const int* node_off, const int* node_off_host, int B, int T, int d,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* Wp,
                          const float* bp, float* out, void* save, size_t save_bytes, void* stream);
int dp_set2set_ragged_bwd(const float* emb, int lde, const int* node_off, const int* node_off_host, int B, int T, int d,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* Wp,
                          const float* bp, const float* out, const float* dout, float* demb, int ldde, float* dw_ih,
                          float* dw_hh, float* db_ih, float* db_hh, float* dWp, float* dbp, const void* save,
                          size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ A9  mean aggregator
 * out[i,:] = mean_{j in indices[indptr[i]:indptr[i+1]]} table[j,:] — MeanAggregator.forward with
 * num_sample=None, aggregators.py:50-62 (the row-normalised mask times the embedding matrix, as a
 * CSR gather-mean).  Rows with no neighbour give 0/0 = NaN in the reference; here too. */
int dp_mean_aggregate_fwd(const float* table, int ldt, const int* indptr, const int* indices, float* out,
                          int ldo, int n_rows, int feat, void* stream);
/* dtable [n_table, feat] is ACCUMULATED INTO (atomic adds). */
int dp_mean_aggregate_bwd(const float* dout, int ldo, const int* indptr, const int* indices, float* dtable,
                          int ldt, int n_rows, int feat, void* stream);

/* ------------------------------------------------------------------ N4  GraphConv on a CSR graph
 * The padded dense path stores a graph as an [N,N] block (load_data.py:79 drops graphs above max_nodes: DD's largest
 * has 5 748 nodes = 132 MB dense).  For such graphs the same layer runs on CSR:
 *     y = l2norm((A x [+ x]) W + b),   A x = sum over the neighbours listed in indices[indptr[i]:indptr[i+1]]
 * — GraphConv.forward (encoders.py:962-974) on ONE graph.  x [n,Fin] (ldx), y [n,Fout] (ldy); ax [n,Fin] receives
 * A x (+ x) and invnorm [n] the row norms' reciprocals (both saved for backward).  flags: DP_F_ADD_SELF | DP_F_NORMALIZE.
 * dp_csr_aggregate is the aggregation alone (mean != 0: the MeanAggregator's mean; beta: out = agg + beta * out). */
int dp_csr_aggregate(const float* table, int ldt, const int* indptr, const int* indices, float* out, int ldo,
                     int n_rows, int feat, int mean, float beta, void* stream);
size_t dp_sparse_gcn_layer_workspace_bytes(int n, int Fin, int Fout);
int dp_sparse_gcn_layer_fwd(const float* x, int ldx, const int* indptr, const int* indices, const float* W,
                            const float* bias, float* y, int ldy, float* ax, float* invnorm, int n, int Fin, int Fout,
                            int flags, void* workspace, size_t workspace_bytes, void* stream);
/* indptr_t / indices_t: CSR of A^T (the same arrays as the forward's for an undirected graph) — dx is then a gather,
 * deterministic; NULL: dx is accumulated with float atomics from the forward CSR.  dx may be NULL.  dW, db OVERWRITTEN. */
int dp_sparse_gcn_layer_bwd(const float* ax, const int* indptr, const int* indices, const int* indptr_t,
                            const int* indices_t, const float* W, const float* y, int ldy, const float* invnorm,
                            const float* dy, int lddy, float* dx, int lddx, float* dW, float* db, int n, int Fin,
                            int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream);
/* Weighted CSR (_w): the entries above read a stored entry as 1; these take its value — values fp32 [nnz] in the order
 * of indices, values_t in the order of indices_t — so GraphConv runs on the reference's default adjacency
 * D^-1/2 A D^-1/2 (graph_sampler.py:27-29, the `adj` of encoders.py:965) or on any weighted graph:
 *     (A x)_i = sum_e values[e] x[indices[e]].
 * dp_csr_aggregate_w has no `mean` (the reference defines no weighted mean).  The backward covers both forms of dx: the
 * gather over A^T with values_t, and with indptr_t == NULL the atomic scatter dx[indices[e]] += values[e] dax_i.  NULL
 * values, or NULL values_t next to an indices_t that is not `indices`, is DP_ERR_INVALID_ARG before any launch; all
 * other checks, the workspace (dp_sparse_gcn_layer_workspace_bytes) and the launch count are the unweighted entries'.
 * The summation order is theirs too: weights of exactly 1.0 give the same bits. */
int dp_csr_aggregate_w(const float* table, int ldt, const int* indptr, const int* indices, const float* values,
                       float* out, int ldo, int n_rows, int feat, float beta, void* stream);
int dp_sparse_gcn_layer_fwd_w(const float* x, int ldx, const int* indptr, const int* indices, const float* values,
                              const float* W, const float* bias, float* y, int ldy, float* ax, float* invnorm, int n,
                              int Fin, int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream);
int dp_sparse_gcn_layer_bwd_w(const float* ax, const int* indptr, const int* indices, const float* values,
                              const int* indptr_t, const int* indices_t, const float* values_t, const float* W,
                              const float* y, int ldy, const float* invnorm, const float* dy, int lddy, float* dx,
                              int lddx, float* dW, float* db, int n, int Fin, int Fout, int flags, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N4  level-0 pooling on a CSR graph
 * Xp = S^T Z [K,D], Ap = S^T A S [K,K] — encoders.py:1278-1279 on ONE graph whose 0/1 adjacency A is given as CSR
 * (row i lists the j with A[i,j] = 1).  S [n,K] (lds), Z [n,D] (ldz).  Xp / Ap OVERWRITTEN.  The forward gathers
 * (A S)_i into LDS row slab by row slab and multiplies S_slab^T [A S | Z]_slab on the fp32 matrix cores; the slabs'
 * partial K x (K+D) blocks are summed in slab order by a second launch: deterministic, no float atomics, and A S is
 * never written to memory.  1 <= K <= 256, 1 <= D <= 512 (DP_ERR_UNSUPPORTED outside), lds >= K, ldz >= D. */
size_t dp_csr_pool_workspace_bytes(int n, int K, int D);
int dp_csr_pool_fwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                    float* Xp, float* Ap, int n, int K, int D, void* workspace, size_t workspace_bytes, void* stream);
/* dS [n,K] OVERWRITTEN = (A S) dAp^T + (A^T S) dAp + Z dXp^T;  dZ [n,D] ACCUMULATED INTO += S dXp (dp_pool_bwd's
 * contract).  indptr_t / indices_t: CSR of A^T; pass the forward's arrays for an undirected graph (the A^T S gather is
 * then skipped).  Row-local: no atomics, bit-reproducible. */
int dp_csr_pool_bwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                    const int* indptr_t, const int* indices_t, const float* dXp, const float* dAp,
                    float* dS, int ldds, float* dZ, int lddz, int n, int K, int D,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Weighted CSR (_w): Ap = S^T A S and dS = (A S) dAp^T + (A^T S) dAp + Z dXp^T (encoders.py:1278-1279 and its
 * transpose) with A's stored values — values / values_t as in dp_sparse_gcn_layer_*_w, loaded next to the column indices
 * by the same gathers.  Same launches, limits, checks and workspace (dp_csr_pool_workspace_bytes); NULL values, or NULL
 * values_t next to an indices_t that is not `indices`, is DP_ERR_INVALID_ARG.  Weights of 1.0 give the unweighted bits. */
int dp_csr_pool_fwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      const float* values, float* Xp, float* Ap, int n, int K, int D, void* workspace,
                      size_t workspace_bytes, void* stream);
int dp_csr_pool_bwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                      const float* dXp, const float* dAp, float* dS, int ldds, float* dZ, int lddz, int n, int K, int D,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N4  link-prediction loss on a CSR graph
 * The loss of A8 — loss = sum_ij [-A log(P+1e-7) - (1-A) log(1-P+1e-7)] / n^2, P = min(S S^T, 1), encoders.py:1309-1331
 * (adj_hop = 1) — on ONE graph whose adjacency is given as CSR, for any n.  No n x n adjacency is read or built: for a
 * 0/1 adjacency the sum decomposes into
 *     sum_ij -log(1 - p_ij + eps)                                   (dense term: a P-tile walk over S alone, upper
 *                                                                    triangle, off-diagonal tiles counted twice)
 *   + sum_{(i,j) in E} [ -log(p_ij + eps) + log(1 - p_ij + eps) ]   (edge term: nnz dot products of S rows, a gather)
 * and the backward likewise into a tile walk plus a row-local gather over A and A^T.  S [n,K] (lds >= K), 1 <= K <= 256
 * (DP_ERR_UNSUPPORTED above), n >= 1.  CSR contract: 0/1 adjacency, each (i,j) listed at most once; self loops,
 * isolated nodes and empty rows are allowed.  Sums are taken in double in a fixed order and there are no float atomics:
 * loss and dS are bit-reproducible.  They agree with the dense entries of A8 to fp32 rounding, not bit for bit (the
 * summation is decomposed).  The workspace is O(n K): dp_csr_linkpred_workspace_bytes covers both directions; a short
 * or NULL workspace, n < 1, lds < K and NULL pointers are DP_ERR_INVALID_ARG before any launch. */
size_t dp_csr_linkpred_workspace_bytes(int n, int K);
/* dp_csr_linkpred_plan: what the host decides for one graph of n rows (a batch runs it per graph, n = n_b, on the graph's
 * own S / dS pointers), answered by the function the launchers themselves act on.  Host only: no stream, no GPU call.
 * s_misaligned / ds_misaligned: non-zero when the graph's S / dS is not 16-byte aligned.
 * plan_out[DP_CSR_LINKPRED_PLAN_INTS] = { KT (K tier of both dense kernels: 1 2 3 4 6 8 12 16), T = ceil(n / 64) row
 * blocks, the forward's row-block pairs (T + 1) / 2 (grid y), its column splits Z (grid x; a workgroup walks every Z-th
 * column tile), dense loss partials = pairs * Z, edge loss partials = ceil(n / 16); the backward's column tile width CW
 * (64, or 32 for KT >= 12), col_tiles = ceil(n / CW), splits (grid z; 1: no gradient partials and no reduce launch),
 * split_tiles (column tiles per split; the last may hold fewer); the forward edge kernel's VEC (floats per lane load:
 * 4 when K % 4 == 0, lds % 4 == 0 and S is 16-byte aligned, else 1) and NCH (16-lane chunks per row), the backward edge
 * kernel's VEC (4 needs ldds % 4 == 0 and an aligned dS as well) and NCH; the dense forward's and the dense backward's
 * dynamic LDS bytes }.  DP_ERR_UNSUPPORTED for K > 256; DP_ERR_INVALID_ARG for n < 1, K < 1, lds < K, ldds < K or a NULL
 * plan_out. */
#define DP_CSR_LINKPRED_PLAN_INTS 16
int dp_csr_linkpred_plan(int n, int K, int lds, int ldds, int s_misaligned, int ds_misaligned, int* plan_out);
int dp_csr_linkpred_loss_fwd(const float* S, int lds, const int* indptr, const int* indices, float* loss_out,
                             int n, int K, void* workspace, size_t workspace_bytes, void* stream);
/* dS (+)= dloss * dloss/dS; dloss: device scalar or NULL = 1; indptr_t/indices_t: CSR of A^T (the forward's arrays
   for an undirected graph: one gather and a factor 2) */
int dp_csr_linkpred_loss_bwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                             const int* indices_t, const float* dloss, float* dS, int ldds, int accumulate,
                             int n, int K, void* workspace, size_t workspace_bytes, void* stream);
/* Weighted CSR (_w): the loss of encoders.py:1309-1331 is linear in a_ij, so the dense term (the tile walk over all
 * pairs) is unchanged and the edge term becomes sum_{(i,j) stored} a_ij [ -log(p_ij + eps) + log(1 - p_ij + eps) ]; the
 * backward's edge coefficient scales likewise.  values / values_t as in dp_sparse_gcn_layer_*_w (an undirected graph —
 * indices_t == indices — must store a_ij = a_ji).  Same launches, checks and workspace (dp_csr_linkpred_workspace_bytes);
 * NULL values, or NULL values_t next to an indices_t that is not `indices`, is DP_ERR_INVALID_ARG.  Weights of 1.0 give
 * the unweighted bits. */
int dp_csr_linkpred_loss_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                               float* loss_out, int n, int K, void* workspace, size_t workspace_bytes, void* stream);
int dp_csr_linkpred_loss_bwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                               const int* indptr_t, const int* indices_t, const float* values_t, const float* dloss,
                               float* dS, int ldds, int accumulate, int n, int K, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N4  ragged batches of CSR graphs
 * B graphs with their node rows CONCATENATED, no padding: graph b owns rows node_off[b] .. node_off[b+1]-1 of every
 * [n_total, .] tensor (node_off: int32 [B+1] on the device, node_off[0] = 0, every graph has >= 1 node).  The entries
 * below compute what the dense entries compute on the same graphs padded to N = max_b n_b, without storing a padded
 * row.  The CSR of the batch is block diagonal: indptr [n_total+1] with GLOBAL edge offsets; column indices GLOBAL
 * (rows of the concatenated tensors) for GraphConv (dp_sparse_gcn_layer_* with n = n_total) and the pooling, graph-LOCAL
 * for the link loss.  No float atomics, every reduction in a fixed order: all results are bit-reproducible.
 *
 * dp_bn_ragged_*: apply_bn (A3) per NODE INDEX i < max_n = max_b n_b.  The statistics of index i run over the rows
 * node_off[b] + i of the cnt[i] graphs with n_b > i plus (B - cnt[i]) copies of pad [F] (NULL = zeros) — the value a
 * padded row of the dense batch has in front of the BatchNorm, relu(l2norm(bias)) of the GraphConv before it — with
 * divisor B*F, biased variance, eps 1e-5.  order: int32 [B], the graphs by size, largest first, so the owners of index
 * i are order[0 .. cnt[i]-1]; cnt: int32 [max_n].  relu != 0 applies ReLU first.  stats [max_n,2] = (mean, rstd).  A
 * wave owns one node index whatever its owner count.  The backward gives dx for the real rows and, when dpad != NULL,
 * dpad [F] (OVERWRITTEN): the padded rows' own dx, rstd_i (-mean(dy) - xhat_pad mean(dy xhat)) times (B - cnt[i]),
 * summed over i in a fixed order.  F <= 2048.  Only the backward needs a workspace. */
size_t dp_bn_ragged_workspace_bytes(int max_n, int F);
int dp_bn_ragged_fwd(const float* x, int ldx, float* y, int ldy, float* stats, const int* node_off, const int* order,
                     const int* cnt, const float* pad, int B, int max_n, int F, int relu, void* stream);
int dp_bn_ragged_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                     float* dx, int lddx, float* dpad, const int* node_off, const int* order, const int* cnt,
                     const float* pad, int B, int max_n, int F, int relu, void* workspace, size_t workspace_bytes,
                     void* stream);
/* pad [F] = relu(bias / max(||bias||, 1e-12)) (without DP_F_NORMALIZE: relu(bias); bias NULL: zeros) — the GraphConv
 * output of a row whose adjacency row is zero, after the ReLU; and dbias [F] (OVERWRITTEN) from dpad through the ReLU
 * gate and the l2norm Jacobian (F.normalize's: identity / eps below eps; a zero bias gives dbias = 0 since relu'(0) = 0).
 * One small launch each, no host synchronisation.  DP_F_ADD_SELF is DP_ERR_UNSUPPORTED (a padded row is then not a
 * constant of the layer). */
int dp_gcn_pad_const_fwd(const float* bias, float* pad, int F, int flags, void* stream);
int dp_gcn_pad_const_bwd(const float* bias, const float* dpad, float* dbias, int F, int flags, void* stream);

/* dp_segment_max_*: the max readout (A7) per graph of a ragged batch: out [B,F] (ldo), argmax int32 [B,F] graph-LOCAL
 * rows, ties to the lowest row.  floor_flag: int32 [B] or NULL; where non-zero the graph has padded rows in the dense
 * batch it stands for, so its result is max(max over its rows, 0) with argmax -1 where the zero wins (a real row holding
 * exactly 0 keeps its index, as dp_masked_max_fwd reports it).  chunk_tab: int32 [n_chunks,4] = {graph, first row, end
 * row, 0} (rows global), chunks of a graph consecutive and in row order, none crossing a graph boundary; chunk_off int32
 * [B+1] = a graph's chunk range.  Two launches for the whole batch (chunk partials, then a per-graph combine in chunk
 * order), so the parallelism comes from the rows.  The backward ACCUMULATES INTO dZ [n_total,F]; one writer per entry. */
size_t dp_segment_max_workspace_bytes(int n_chunks, int F);
int dp_segment_max_fwd(const float* Z, int ldz, const int* node_off, const int* chunk_tab, const int* chunk_off,
                       int n_chunks, const int* floor_flag, float* out, int ldo, int* argmax, int B, int F,
                       void* workspace, size_t workspace_bytes, void* stream);
int dp_segment_max_bwd(const float* dout, int ldo, const int* argmax, const int* node_off, float* dZ, int lddz, int B,
                       int F, void* stream);

/* The UNMASKED max readout of the base encoder (A11: torch.max over all P = pad_to rows of the dense batch) on a ragged
 * batch.  Behind apply_bn every padded row of node index i holds v[i,f] = (pad[f] - mean_i) rstd_i, so the padded rows of
 * a graph with n_b < P contribute max_{i >= n_b} v[i,f]: a suffix maximum over node indices.  n_min = min_b n_b (lower
 * indices have no padded row), n_idx = max_n + (P > max_n): the TAIL ROW max_n stands for every index >= max_n, whose B
 * rows all hold pad (statistics of pad alone: mean over f, biased variance, eps 1e-5).  Every table below is [n_idx, .];
 * rows below n_min are never read or written.  The argmax of these entries is the row of the DENSE batch: < n_b a real
 * row (graph-local), in n_b .. P-1 a padded one (the lowest index that attains the maximum; the tail reports max_n).
 *
 * dp_ragged_padval_fwd: padval rows n_min .. n_idx-1 from stats [n_idx,2] (rows < max_n as dp_bn_ragged_fwd wrote them;
 * row max_n is WRITTEN here when n_idx > max_n) and pad [F] (NULL = zeros).  One launch.
 * dp_ragged_suffix_max: sufv[i,f] = max_{j >= i} padval[j,f], sufi the lowest such j, for i = n_min .. n_idx-1.  Two
 * launches: maxima of 64-row blocks, then each block scans its rows downwards from the combined maxima of the blocks
 * above it; equal values keep the lowest index at both levels. */
int dp_ragged_padval_fwd(float* stats, const float* pad, float* padval, int ldp, int n_min, int max_n, int n_idx, int F,
                         void* stream);
size_t dp_ragged_suffix_max_workspace_bytes(int n_min, int n_idx, int F);
int dp_ragged_suffix_max(const float* padval, int ldp, float* sufv, int* sufi, int lds, int n_min, int n_idx, int F,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dp_segment_max_floor_*: dp_segment_max_* (same chunk tables, same first launch, workspace of
 * dp_segment_max_workspace_bytes) whose floor for the graphs with floor_flag != 0 is row n_b of the suffix table (sufv,
 * sufi: winner sufi[n_b,f]) or the constant row floor_row [F] (winner n_b) — one of the two, or neither (no floor).  A
 * real row wins an exact tie with the floor.  The backward ACCUMULATES INTO dZ for real winners and builds the floor's
 * gradient G in a fixed order (one thread per column walks b = 0 .. B-1): table != 0: G [n_idx, F] (ldg), rows
 * n_min .. n_idx-1 zero-filled here, G[i,f] = sum of dout[b,f] over the graphs whose winner is padded index i; table == 0:
 * G [F] (OVERWRITTEN) = sum over the graphs whose floor won.  G NULL: only dZ.  Launch counts do not depend on B. */
int dp_segment_max_floor_fwd(const float* Z, int ldz, const int* node_off, const int* chunk_tab, const int* chunk_off,
                             int n_chunks, const int* floor_flag, const float* sufv, const int* sufi, int lds,
                             int n_min, int n_idx, const float* floor_row, float* out, int ldo, int* argmax, int B,
                             int F, void* workspace, size_t workspace_bytes, void* stream);
int dp_segment_max_floor_bwd(const float* dout, int ldo, const int* argmax, const int* node_off, float* dZ, int lddz,
                             float* G, int ldg, int n_min, int n_idx, int table, int B, int F, void* stream);
/* dp_bn_ragged_bwd when the padded rows received output gradients: G [n_idx, F] (ldg) holds, per node index and feature,
 * the sum of dy over that index's padded rows (rows of indices without a padded row are not read).  With xhat_pad = v[i,f]:
 * mean(dy) and mean(dy xhat) of index i gain sum_f G and sum_f G v, dx of the real rows keeps its formula, and
 * dpad[f] = sum_i rstd_i (G[i,f] - (B - cnt[i]) (m1_i + v[i,f] m2_i)); the tail row counts as one index with cnt = 0.
 * (the per-workgroup partial rows of dpad are summed in double in a fixed order and rounded once: with G the running
 * sums reach hundreds of times an entry).  stats [n_idx,2]; workspace: dp_bn_ragged_workspace_bytes(n_idx, F).
 * G == NULL is dp_bn_ragged_bwd itself. */
int dp_bn_ragged_g_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                       float* dx, int lddx, float* dpad, const float* G, int ldg, const int* node_off, const int* order,
                       const int* cnt, const float* pad, int B, int max_n, int n_idx, int F, int relu, void* workspace,
                       size_t workspace_bytes, void* stream);
/* dp_gcn_pad_const_* without the ReLU: c [F] = bias / max(||bias||, 1e-12) (without DP_F_NORMALIZE: bias; NULL: zeros),
 * what a padded row holds behind the LAST GraphConv layer, and dbias [F] (OVERWRITTEN) through the l2norm Jacobian. */
int dp_gcn_row_const_fwd(const float* bias, float* c, int F, int flags, void* stream);
int dp_gcn_row_const_bwd(const float* bias, const float* dc, float* dbias, int F, int flags, void* stream);

/* dp_csr_pool_batch_*: the level-0 pooling of dp_csr_pool_* for every graph of the batch, Xp [B,K,D], Ap [B,K,K], from
 * the ragged S [n_total,K], Z [n_total,D] and the block-diagonal CSR (GLOBAL column indices).  The kernels are those of
 * dp_csr_pool_*, driven by tables: dp_csr_pool_batch_plan (host only, no GPU call) writes for the sizes node_off_host
 * the forward slab table [n_slabs,4] = {first row, end row, graph, 0}, slab_off [B+1] and the backward row-block table
 * [n_blocks,4], and counts_host[2] = {n_slabs, n_blocks}; with the table pointers NULL it only counts.  Graph b keeps
 * the slab partition and the row blocks a dp_csr_pool_* call on it alone would use, no slab or row block crosses a graph
 * boundary and the partials are summed per graph in slab order: every graph's result equals that call's BIT FOR BIT.
 * The caller copies the tables to the device once.  Limits and contract of dp_csr_pool_* (K <= 256, D <= 512; dS
 * OVERWRITTEN, dZ ACCUMULATED INTO); the launch count does not depend on B (2 forward, 2 backward). */
int dp_csr_pool_batch_plan(const int* node_off_host, int B, int K, int D, int* fwd_tab_host, int* slab_off_host,
                           int* bwd_tab_host, int* counts_host);
size_t dp_csr_pool_batch_workspace_bytes(int n_slabs, int B, int K, int D);
int dp_csr_pool_batch_fwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                          const int* fwd_tab, const int* slab_off, int n_slabs, float* Xp, float* Ap, int B,
                          int n_total, int K, int D, void* workspace, size_t workspace_bytes, void* stream);
int dp_csr_pool_batch_bwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                          const int* indptr_t, const int* indices_t, const int* bwd_tab, int n_blocks,
                          const float* dXp, const float* dAp, float* dS, int ldds, float* dZ, int lddz, int B,
                          int n_total, int K, int D, void* workspace, size_t workspace_bytes, void* stream);
/* The weighted forms (encoders.py:1278-1279 with stored values): values / values_t fp32 [nnz of the batch] in the order of
 * indices / indices_t — one array serves the GLOBAL and the graph-LOCAL index arrays.  Contract of dp_csr_pool_*_w. */
int dp_csr_pool_batch_fwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                            const float* values, const int* fwd_tab, const int* slab_off, int n_slabs, float* Xp,
                            float* Ap, int B, int n_total, int K, int D, void* workspace, size_t workspace_bytes,
                            void* stream);
int dp_csr_pool_batch_bwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                            const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                            const int* bwd_tab, int n_blocks, const float* dXp, const float* dAp, float* dS, int ldds,
                            float* dZ, int lddz, int B, int n_total, int K, int D, void* workspace,
                            size_t workspace_bytes, void* stream);

/* dp_csr_linkpred_batch_*: the link loss of a batch, sum_b (graph b's sum) / sum_b n_b^2 (encoders.py:1326-1331), with
 * O(n_total K) memory and no dense adjacency.  Built from PER-GRAPH launches of the dp_csr_linkpred_* kernels (the
 * tile walk is n_b^2 work per graph anyway) plus one final / scale launch for the batch, so the launch count grows with
 * B: 2B + 1 forward, up to 3B + 1 backward.  node_off_host is on the HOST; indptr is the batch's, the column indices
 * are graph-LOCAL.  Contract of dp_csr_linkpred_* otherwise. */
size_t dp_csr_linkpred_batch_workspace_bytes(const int* node_off_host, int B, int K);
int dp_csr_linkpred_batch_loss_fwd(const float* S, int lds, const int* indptr, const int* indices_local,
                                   const int* node_off_host, int B, float* loss_out, int K, void* workspace,
                                   size_t workspace_bytes, void* stream);
int dp_csr_linkpred_batch_loss_bwd(const float* S, int lds, const int* indptr, const int* indices_local,
                                   const int* indptr_t, const int* indices_t_local, const int* node_off_host, int B,
                                   const float* dloss, float* dS, int ldds, int accumulate, int K, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* The weighted forms (encoders.py:1309-1331 with stored values): contract of dp_csr_linkpred_loss_*_w, values / values_t
 * the batch's arrays (GLOBAL edge offsets, as indptr gives them). */
int dp_csr_linkpred_batch_loss_fwd_w(const float* S, int lds, const int* indptr, const int* indices_local,
                                     const float* values, const int* node_off_host, int B, float* loss_out, int K,
                                     void* workspace, size_t workspace_bytes, void* stream);
int dp_csr_linkpred_batch_loss_bwd_w(const float* S, int lds, const int* indptr, const int* indices_local,
                                     const float* values, const int* indptr_t, const int* indices_t_local,
                                     const float* values_t, const int* node_off_host, int B, const float* dloss,
                                     float* dS, int ldds, int accumulate, int K, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ================================================================== model-level entry points
 * One call enqueues the whole forward (or backward) of an encoder, so the Python host pays one
 * FFI crossing per pass instead of ~100.  Parameters live in ONE flat fp32 buffer; the cfg gives
 * the offset (in floats) of every tensor.  Gradients are written to a flat buffer of the same
 * layout (ready for a single RCCL all-reduce). */
typedef struct {
    int n_layers;                    /* L */
    int dims[DP_MAX_LAYERS + 1];     /* dims[0] = input width, dims[l] = output width of layer l */
    long w_off[DP_MAX_LAYERS];       /* weight [dims[l], dims[l+1]] offset in the flat buffer */
    long b_off[DP_MAX_LAYERS];       /* bias [dims[l+1]] offset, or -1 */
    long drop_off[DP_MAX_LAYERS];    /* layer-input dropout (GraphConv.forward, encoders.py:962-964): offset in the
                                        `dropout` buffer of a mask [B, n, dims[l]] holding 0 or 1/(1-p), or -1.
                                        Layer 0 (conv_first) has none in the reference; must be -1. */
} dp_stack_cfg;

/* Sync-BN exchange (data parallelism, SURVEY 8(e) mode ii).  apply_bn couples the whole batch (encoders.py:1048-1052);
 * when a batch is sharded over `bn_world` ranks the per-row partials every BatchNorm site produces must be gathered
 * from all ranks before they are combined.  The library calls `exchange` from inside dp_encoder_forward / backward,
 * between the launch that writes the local block and the launch that reads the gathered one; the callback must
 * ENQUEUE, on `stream`, an all-gather of `bytes_per_rank` bytes at `local` into `gathered` (rank-major,
 * bn_world * bytes_per_rank bytes; both are device pointers inside the call's workspace) and return 0. */
typedef int (*dp_exchange_fn)(void* user, const void* local, void* gathered, size_t bytes_per_rank, void* stream);

typedef struct {
    int B, N;                        /* batch, padded node count */
    int num_pooling;                 /* P */
    int n_nodes[DP_MAX_LEVELS + 1];  /* n_nodes[0] = N, n_nodes[j+1] = K_j (encoders.py:1203,1215) */
    dp_stack_cfg embed[DP_MAX_LEVELS + 1]; /* embed[0]: conv_first/.. ; embed[j+1]: after pool j */
    dp_stack_cfg assign[DP_MAX_LEVELS];    /* assign GCN of level j (input: assign_x / pooled X) */
    long assign_pred_w_off[DP_MAX_LEVELS]; /* Linear [K_j, Da_j] (encoders.py:1210) */
    long assign_pred_b_off[DP_MAX_LEVELS];
    int n_pred;                      /* number of Linear layers in pred_model (hidden + 1) */
    int pred_dims[DP_MAX_PRED + 2];  /* pred_dims[0] = D*(P+1) ... pred_dims[n_pred] = label_dim */
    long pred_w_off[DP_MAX_PRED + 1];
    long pred_b_off[DP_MAX_PRED + 1];
    int flags;                       /* DP_F_BN | DP_F_ADD_SELF */
    int readout;                     /* 0: max over nodes of the concat (DiffPool / base encoder),
                                        1: Set2Set (GcnSet2SetEncoder) */
    long s2s_off[6];                 /* w_ih, w_hh, b_ih, b_hh, pred.weight, pred.bias (readout 1) */
    int mask_readout;                /* 1: level-0 embedding is masked before readout (DiffPool,
                                        Set2Set encoder); 0: base encoder (encoders.py:1083-1122) */
    long n_params;                   /* total floats in the flat buffer */
    long n_graph_params;             /* params [0, n_graph_params) are the GCN stacks + assign heads
                                        (their gradients are reduced from per-graph slabs); the
                                        pred_model / Set2Set parameters follow */
    int bn_world;                    /* 0 / 1: apply_bn over the local batch; W > 1: over the W equal shards of a
                                        data-parallel batch (every rank passes the same B) through `exchange`.
                                        bn_world == 1 WITH `exchange` set runs the sync-BN launch sequence and every
                                        callback over one rank (a one-GPU rehearsal of the collective path) */
    dp_exchange_fn exchange;
    void* exchange_user;
} dp_encoder_cfg;

size_t dp_sizeof_encoder_cfg(void); /* sizeof(dp_encoder_cfg): lets a binding check its struct layout */
size_t dp_encoder_save_bytes(const dp_encoder_cfg* cfg);
/* The workspace of the model-level calls must be ZERO-FILLED ONCE after it is allocated (before its first use with
 * this cfg) and then left alone between calls: its first block holds the barrier state of the persistent level-0
 * kernel, which every launch leaves clean (also a launch whose barrier gave up).  A workspace with garbage there makes
 * the first forward time out: DP_DEVERR_BARRIER on the next entry, NaN logits, never a hang. */
size_t dp_encoder_workspace_bytes(const dp_encoder_cfg* cfg);

/* Where one saved activation of pooling level `level` sits inside the `save` buffer after dp_encoder_forward: the
 * reference keeps only the LAST level's S as `self.assign_tensor` (encoders.py:1276) for train.py:218-219's logging;
 * this gives a caller (and the parity tests) every level's S_j [B,n_j,K_j], X'_j [B,K_j,D], A'_j [B,K_j,K_j]
 * (encoders.py:1278-1279) and the embeddings Z_j [B,n_j,D] / assign-stack outputs [B,n_j,Da_j] without a second pass.
 * offset is in BYTES from `save`, count in 4-byte elements.  Returns DP_ERR_INVALID_ARG for a level without that tensor. */
#define DP_SAVE_S 0
#define DP_SAVE_XPOOL 1
#define DP_SAVE_ADJPOOL 2
#define DP_SAVE_Z 3
#define DP_SAVE_ZASSIGN 4
#define DP_SAVE_ARGMAX 5   /* int32 [B, readout width]: winning row of the max readout (-1: a masked zero row) */
int dp_encoder_save_locate(const dp_encoder_cfg* cfg, int level, int field, size_t* offset, size_t* count);

/* SoftPoolingGcnEncoder.forward (encoders.py:1231-1300), GcnEncoderGraph.forward (:1083-1122,
 * num_pooling = 0) and GcnSet2SetEncoder.forward (:1144-1157, readout = 1).
 * x [B,N,F], adj [B,N,N], assign_x [B,N,Fa] (may alias x), num_nodes int32[B] or NULL.
 * ypred [B,label_dim]; assign_out [B,N,K_0] (level-0 S, = assign_tensor when P = 1) or NULL when
 * P = 0; `save` keeps activations for backward.  dropout: the mask buffer addressed by the stacks' drop_off
 * (training with GraphConv dropout > 0; the caller draws the masks and passes the SAME buffer to backward), or
 * NULL (evaluation, or dropout 0: every drop_off is ignored). */
#define DP_MODE_EVAL 0   /* forward only (train.py:30-58 evaluate): nothing is prepared for a backward pass */
#define DP_MODE_TRAIN 1  /* a dp_encoder_backward with the SAME save and workspace buffers will follow: the forward also
                            clears the backward pass's accumulators (they live at the start of the workspace) on the side
                            of its adjacency-pack kernel, so the backward may be called with prezeroed = 1 — provided
                            nothing else used that workspace in between and it is the first backward of this forward */
/* labels_out: int64 [B] or NULL — the arg-max class of every graph (first index on ties), written by the prediction
 * head's own launch: evaluate() (train.py:42-44) moves B integers to the host instead of B x C logits. */
int dp_encoder_forward(const dp_encoder_cfg* cfg, const float* params, const float* x, const float* adj,
                       const float* assign_x, const int* num_nodes, const float* dropout, float* ypred,
                       float* assign_out, long long* labels_out, void* save, size_t save_bytes, void* workspace,
                       size_t workspace_bytes, int mode, void* stream);
/* d_ypred [B,label_dim]; d_assign [B,N,K_0] or NULL (gradient arriving at the level-0 assignment
 * from the link-prediction loss); grads: flat, same layout as params, OVERWRITTEN.
 * prezeroed: 1 iff the accumulators were cleared by a DP_MODE_TRAIN forward (see above); 0: this call clears them. */
int dp_encoder_backward(const dp_encoder_cfg* cfg, const float* params, const float* x, const float* adj,
                        const float* assign_x, const int* num_nodes, const float* dropout, const float* d_ypred,
                        const float* d_assign, float* grads, const void* save, size_t save_bytes,
                        void* workspace, size_t workspace_bytes, int prezeroed, void* stream);

/* The same two calls for a level-0 adjacency that is ALREADY in the packed form the kernels multiply from — bf16 rows
 * [B, N, dp_adj_pack_ld(N)] of A (adj_pk) and of A^T (adj_pkt; the same buffer for a symmetric adjacency), as written
 * by dp_build_batch_packed or dp_adj_pack: no fp32 [B,N,N] batch is written, read or converted (the
 * end-to-end training step).  The bf16 values ARE the adjacency (nothing to round).  Only configurations that take the
 * persistent level-0 plan accept it (N >= 64, N % 4 == 0, B * ceil(N / RB) <= CUs, no sync-BN, no add_self):
 * DP_ERR_UNSUPPORTED otherwise — the fp32 entries above serve every configuration and train.py.  The loss of such a
 * step, link prediction included, takes the same packed rows: dp_loss_forward_packed / dp_loss_backward_packed. */
int dp_encoder_forward_packed(const dp_encoder_cfg* cfg, const float* params, const float* x, const void* adj_pk,
                              const void* adj_pkt, const float* assign_x, const int* num_nodes, const float* dropout,
                              float* ypred, float* assign_out, long long* labels_out, void* save, size_t save_bytes,
                              void* workspace, size_t workspace_bytes, int mode, void* stream);
int dp_encoder_backward_packed(const dp_encoder_cfg* cfg, const float* params, const float* x, const void* adj_pk,
                               const void* adj_pkt, const float* assign_x, const int* num_nodes, const float* dropout,
                               const float* d_ypred, const float* d_assign, float* grads, const void* save,
                               size_t save_bytes, void* workspace, size_t workspace_bytes, int prezeroed, void* stream);

/* SoftPoolingGcnEncoder.loss (encoders.py:1302-1334): loss_out[0] = CE (+ link), loss_out[1] = link.
 * prob [B,C] saved for backward.  S / adj may be NULL when linkpred == 0.
 * d_ypred_unit [B,C] (may be NULL): d loss / d ypred for an upstream gradient of 1, (softmax - onehot) / B, written by
 * the same launch — `loss.backward()` (train.py:208) sends exactly that down, so the caller can hand it to
 * dp_encoder_backward without a gradient launch of its own. */
size_t dp_loss_workspace_bytes(int B, int N, int K, int linkpred);   /* also covers the _packed entries below */
/* link_norm (device scalar or NULL): replaces the link loss's normaliser sum_b n_b^2 (encoders.py:1326,1331).  Under
 * data parallelism every rank passes (sum over ALL ranks' graphs) / world_size, so that the mean over ranks of the
 * per-rank losses and gradients is the loss of the concatenated batch. */
int dp_loss_forward(const float* ypred, const long long* label, const float* S, const float* adj,
                    const int* num_nodes, const float* link_norm, float* loss_out, float* prob, float* d_ypred_unit,
                    int B, int C, int N, int K, int linkpred, void* workspace, size_t workspace_bytes, void* stream);
/* dloss: device scalar (NULL = 1).  d_ypred [B,C] (NULL: not wanted — the caller uses d_ypred_unit), dS [B,N,K]
 * (only when linkpred) overwritten. */
int dp_loss_backward(const float* prob, const long long* label, const float* S, const float* adj,
                     const int* num_nodes, const float* link_norm, const float* dloss, float* d_ypred, float* dS,
                     int B, int C, int N, int K, int linkpred, void* workspace, size_t workspace_bytes, void* stream);
/* The same two calls with the link loss reading the packed adjacency (adj_pk / adj_pkt as in A8 above, N rows of
 * dp_adj_pack_ld(N)) in place of adj: the loss of the step that dp_encoder_forward_packed / _backward_packed run.
 * adj_pk / adj_pkt may be NULL when linkpred == 0. */
int dp_loss_forward_packed(const float* ypred, const long long* label, const float* S, const void* adj_pk,
                           const void* adj_pkt, const int* num_nodes, const float* link_norm, float* loss_out,
                           float* prob, float* d_ypred_unit, int B, int C, int N, int K, int linkpred, void* workspace,
                           size_t workspace_bytes, void* stream);
int dp_loss_backward_packed(const float* prob, const long long* label, const float* S, const void* adj_pk,
                            const void* adj_pkt, const int* num_nodes, const float* link_norm, const float* dloss,
                            float* d_ypred, float* dS, int B, int C, int N, int K, int linkpred, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N1  on-device batch builder
 * Replaces GraphSampler.__getitem__ + collate + H2D of the dense batch (graph_sampler.py:97-109, train.py:197-201):
 * the host ships the batch's edge lists, the device writes adj [B,N,N] (0/1, zero padded), the node features
 * feats [B,N,Fout] (NULL: skip) and num_nodes [B].  Graph b owns edges [edge_ptr[b], edge_ptr[b+1]) with node ids
 * local to the graph, and node labels label[node_ptr[b] .. node_ptr[b+1]).  symmetric != 0 also sets adj[d][s]
 * (undirected edge lists that store each edge once).
 * feature_mode (graph_sampler.py:33-59): 0 one-hot node label (Fout = F), 1 identity (Fout = N), 2 degree as one
 * column (Fout = 1), 3 one-hot degree capped at 10 then the one-hot label (Fout = 11 + F); modes 2 and 3 need the
 * `degree` workspace (B*N ints).  assign_feats [B,N,N+Fout] (NULL: skip) = [identity | feats], the sampler's
 * assign_feat='id' (graph_sampler.py:85-87).
 * errors: device int, receives the number of skipped out-of-range entries (0 = clean batch).
 * max_edges_per_graph only sizes the launch. */
int dp_build_batch(const int* edge_src, const int* edge_dst, const int* edge_ptr, const int* node_label,
                   const int* node_ptr, float* adj, float* feats, float* assign_feats, int* num_nodes, int* errors,
                   int* degree, int B, int N, int F, int feature_mode, int symmetric, int max_edges_per_graph,
                   void* stream);

/* The same builder writing the adjacency straight into the packed form of dp_adj_pack (bf16 rows, ld =
 * dp_adj_pack_ld(N); 1.0 = 0x3F80): adj_pk receives A, adj_pkt receives A^T — for symmetric != 0 the two are equal
 * and the caller may pass the SAME buffer for both (dp_adj_pack_bytes(B, N) bytes each).  Feeds
 * dp_encoder_forward_packed / _backward_packed: the fp32 [B,N,N] batch is never materialised. */
int dp_build_batch_packed(const int* edge_src, const int* edge_dst, const int* edge_ptr, const int* node_label,
                          const int* node_ptr, void* adj_pk, void* adj_pkt, float* feats, float* assign_feats,
                          int* num_nodes, int* errors, int* degree, int B, int N, int F, int feature_mode, int symmetric,
                          int max_edges_per_graph, void* stream);
/* The input arrays of both builders may live in pinned host memory that the device can address (hipHostMalloc): the
 * kernels then fetch the ~190 KB of a DD batch over PCIe themselves and a captured training step needs no copy node.
 * dp_gather_labels copies the B graph labels the same way (int64, host-visible source -> device). */
int dp_gather_labels(const long long* graph_label, long long* label_out, int B, void* stream);

/* ------------------------------------------------------------------ N2  fused gradient clip + Adam step
 * train.py:209-210 on top of the Adam of train.py:173, over the flat fp32 parameter / gradient buffers (n floats):
 *   total = ||grads||_2;  grads *= min(1, max_norm / (total + 1e-6))   (max_norm <= 0: no clipping)
 *   exp_avg = b1 exp_avg + (1-b1) g;  exp_avg_sq = b2 exp_avg_sq + (1-b2) g^2
 *   params -= lr / (1 - b1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - b2^step) + eps)
 * step >= 1 is the 1-based count of this update.  total_norm_out: device float or NULL.  Two launches.
 * With max_norm <= 0 AND total_norm_out == NULL no norm is taken by either entry (this one then makes one launch), so
 * nothing looks at the gradient's finiteness: a non-finite gradient is NOT skipped and DP_DEVERR_NONFINITE_GRAD is not raised — the
 * update goes through and writes NaN into the elements concerned, as torch.optim.Adam alone would.  Give either
 * argument to keep the skip. */
size_t dp_clip_adam_workspace_bytes(void);
int dp_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, int step, float lr,
                      float beta1, float beta2, float eps, float max_norm, float* total_norm_out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same update with the step count kept ON THE DEVICE: step_counter (device int, the number of updates done so far;
 * zero it once) is incremented by the call and the bias corrections of the new count are computed by the kernel (in
 * double, as above).  The count goes up on a step that is skipped for a non-finite norm too: the norm kernel counts,
 * one launch ahead of the kernel that finds the norm non-finite.  No argument changes from step to step, so the call can sit inside a captured hipGraph together
 * with dp_build_batch_packed, dp_encoder_forward_packed, dp_loss_forward (dp_loss_forward_packed with the
 * link-prediction loss) and dp_encoder_backward_packed: one graph launch per training step (train.py:197-210). */
int dp_clip_adam_step_counted(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, int* step_counter,
                              float lr, float beta1, float beta2, float eps, float max_norm, float* total_norm_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N4  gradients to the stored values of a CSR
 * Every stored entry e = (i, j), j = indices[e], of a CsrGraph / CsrBatch is an independent variable a_e (the gradient
 * torch gives for a dense A built with index_put from `values`); its gradient is delivered in the order of `values`.
 * All four come from ONE kernel family, a sampled dense-dense product over the stored entries,
 *     out[e] = beta * out[e] + alpha * d * epi( sum_f P[i,f] Q[indices[e],f], a_e ),
 * P [n_rows,F] (ldp), Q [.,F] (ldq) row-major fp32, d = dscale[0] (device scalar; NULL: 1), epi the identity
 * (dp_csr_sddmm), the cross-entropy link derivative log(1 - p + 1e-7) - log(p + 1e-7) with p = min(t, 1), or the
 * Frobenius derivative 2 (a_e - t).  A group of 4 / 16 / 64 lanes serves one entry, P_i stays in registers over the
 * row's entries, a row is cut into chunks of 512 entries taken by separate waves, and every out[e] is one dot product
 * summed in a fixed order: no atomics, no temporary, bit-reproducible.  beta == 0: out is not read.  Any F >= 1;
 * F == 0 or n_rows == 0 writes nothing and returns DP_OK.  No gradient flows to P or Q through these entries.
 *
 * dp_csr_sddmm_plan (host only): plan_out[DP_CSR_SDDMM_PLAN_INTS] = { lanes per entry (4 / 16 / 64: the smallest group
 * that covers F in one visit, 64 above), floats per lane load (4 when F % 4 == 0, ldp % 4 == 0, ldq % 4 == 0 and
 * neither base is misaligned to 16 bytes; else 1), visits of lanes * floats columns whose P_i is held in registers
 * (1 .. 4), 1 when columns beyond those are walked with P_i re-read from the cache, entries per row chunk (512), rows per
 * workgroup (4) }, answered by the function the launcher acts on.  F < 1, ldp < F, ldq < F, NULL plan_out:
 * DP_ERR_INVALID_ARG. */
#define DP_CSR_SDDMM_PLAN_INTS 6
int dp_csr_sddmm_plan(int F, int ldp, int ldq, int p_misaligned, int q_misaligned, int* plan_out);
int dp_csr_sddmm(const float* P, int ldp, const float* Q, int ldq, const int* indptr, const int* indices, float* out,
                 int n_rows, int F, float alpha, const float* dscale, float beta, void* stream);
/* dvalues[e] OVERWRITTEN = dloss * dL/da_e of the link loss of dp_csr_linkpred_* (objective 0) or dp_csr_frob_link_*
 * (objective 1): inv_norm * (log(1 - p + 1e-7) - log(p + 1e-7)), or inv_norm * 2 (a_e - s_i . s_j) with a_e = values[e]
 * (NULL values: a 0/1 container, a_e = 1).  inv_norm = 1 / sum_b n_b^2 comes from the host; dloss: device scalar or
 * NULL = 1.  One launch serves one graph or a whole batch: indices are rows of S (the block-diagonal CSR with GLOBAL
 * columns and the concatenated S).  K >= 1 (no limit above), lds >= K. */
int dp_csr_link_dvalues(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                        float* dvalues, int n_rows, int K, int objective, float inv_norm, const float* dloss,
                        void* stream);
/* dvalues[e] OVERWRITTEN = (S dAp_b)_i . s_j of the pooling Ap_b = S_b^T A_b S_b (dp_csr_pool_* / dp_csr_pool_batch_*),
 * b the graph that owns row i.  dAp [B,K,K]; node_off_host: host int32 [B+1], or NULL for one graph (B must be 1).  The
 * workspace receives P = S dAp_b [n_total,K] (one GEMM for one graph, grouped GEMMs of up to 4 graphs for a batch), then
 * one SDDMM launch with Q = S runs over the block-diagonal CSR (GLOBAL columns).  K >= 1, lds >= K. */
size_t dp_csr_pool_dvalues_workspace_bytes(int n_total, int K);
int dp_csr_pool_dvalues(const float* S, int lds, const int* indptr, const int* indices, const float* dAp,
                        const int* node_off_host, int B, float* dvalues, int n_total, int K, void* workspace,
                        size_t workspace_bytes, void* stream);
/* dp_sparse_gcn_layer_bwd_w that also returns dvalues[e] OVERWRITTEN = dax_i . x_j, dax = dU W^T as the backward forms
 * it (add_self changes nothing here): the same launches in the same order, then one SDDMM with P = dax, Q = x (ldx).
 * dax is formed whenever dvalues is wanted, also with dx == NULL; dp_sparse_gcn_layer_workspace_bytes covers it.  dx,
 * dW, db are the bits of dp_sparse_gcn_layer_bwd_w.  A 0/1 container has no values: only the weighted form exists. */
int dp_sparse_gcn_layer_bwd_dv(const float* ax, const int* indptr, const int* indices, const float* values,
                               const int* indptr_t, const int* indices_t, const float* values_t, const float* W,
                               const float* y, int ldy, const float* invnorm, const float* dy, int lddy, float* dx,
                               int lddx, float* dW, float* db, const float* x, int ldx, float* dvalues, int n, int Fin,
                               int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ N5  learned edge weights on a CSR: edge softmax
 * and D^-1/2 A D^-1/2 on the device, both with their backward.  Segmented passes over the stored entries
 * of each row of a CsrGraph / CsrBatch (a batch is its block-diagonal CSR with GLOBAL columns: one launch sequence
 * serves both).  A group of 4 / 16 / 64 lanes serves one row, chosen from the mean row length nnz / n_rows; the lanes of
 * a group take consecutive entries (coalesced index and value loads) and a row longer than the group loops.  Every sum
 * has one order — the lane's entries ascending, then a DPP tree over the group — so a second run gives the same bits.
 * No atomics, no workspace.  n_rows == 0 or nnz == 0 writes nothing and returns DP_OK; every refusal
 * (DP_ERR_INVALID_ARG: a NULL or misaligned pointer, a negative count) comes before any launch.
 *
 * dp_csr_edge_plan (host only): plan_out[DP_CSR_EDGE_PLAN_INTS] = { lanes per row (4 while nnz <= 8 n_rows, 16 while
 * nnz <= 32 n_rows, 64 above), entries a lane of the softmax kernels keeps in registers (8 / 4 / 4), rows per workgroup
 * (256 / lanes), the longest row that is read once (lanes * entries per lane) }, answered by the function the launchers
 * act on.  n_rows < 0, nnz < 0, NULL plan_out: DP_ERR_INVALID_ARG. */
#define DP_CSR_EDGE_PLAN_INTS 4
int dp_csr_edge_plan(int n_rows, int nnz, int* plan_out);
/* Softmax over each row's stored entries: out[e] = exp(s_e - m_i) / sum_{e' in row i} exp(s_e' - m_i), m_i the row
 * maximum; scores, out fp32 [nnz] in the order of indices (which the entry does not need).  A row with one entry gives
 * exactly 1.0, a row with none is not touched.  A row that fits the registers is read once; a longer one runs a
 * per-lane running maximum and sum and is read a second time.  One launch. */
int dp_csr_edge_softmax_fwd(const float* scores, const int* indptr, float* out, int n_rows, int nnz, void* stream);
/* dscores[e] OVERWRITTEN = out_e (dout_e - sum_{row} out dout); a one-entry row gives exactly 0.  One launch. */
int dp_csr_edge_softmax_bwd(const float* out, const float* dout, const int* indptr, float* dscores, int n_rows, int nnz,
                            void* stream);
/* out[e] = values[e] * (r_i * r_j), j = indices[e], r = d^-1/2 (1 / sqrt, plain IEEE) written to rdeg [n] and kept for
 * the backward; d_c is the COLUMN sum of the stored values (graph_sampler.py:27-29: np.sum(adj, axis=0)), taken as the
 * sum of row c of the transposed CSR, whose entry k is the stored entry mirror[k] (int32 [nnz]).  The product order
 * makes symmetric values give out_ij == out_ji bit for bit.  values NULL: all ones (a 0/1 container).  mirror may be
 * NULL only when indices_t == indices: an undirected container, whose contract is a_ij = a_ji.  d_c <= 0 with entries
 * present gives inf or NaN as the reference does; a node with no entry in its row and none in its column has
 * rdeg = inf and touches no out[e].  Two launches. */
int dp_csr_sym_norm_fwd(const int* indptr, const int* indices, const float* values, const int* indptr_t,
                        const int* indices_t, const int* mirror, float* rdeg, float* out, int n, int nnz, void* stream);
/* dvalues[e] OVERWRITTEN = dout_e r_i r_j + G_j, G_c = -1/2 r_c^3 t_c (0 for a node with no entries), t_c =
 * sum_{e in row c} dout_e v_e r_col(e) + sum_{e in column c} dout_e v_e r_row(e) (a self loop counts in both sums): the
 * gradient torch gives for a dense A built with index_put and normalised with A.sum(0).  mirror is always required;
 * gdeg [n] is the workspace that receives G.  Two launches. */
int dp_csr_sym_norm_bwd(const int* indptr, const int* indices, const float* values, const int* indptr_t,
                        const int* indices_t, const int* mirror, const float* rdeg, const float* dout, float* gdeg,
                        float* dvalues, int n, int nnz, void* stream);

/* ------------------------------------------------------------------ N6  multi-head additive (GAT) edge attention on a
 * CSR, fused.  For every stored entry e = (i, j), j = indices[e], of a CsrGraph / CsrBatch (a batch is its
 * block-diagonal CSR with GLOBAL columns) and every head h < H:
 *     pre_eh = u_ih + v_jh,   s_eh = pre_eh > 0 ? pre_eh : slope * pre_eh   (torch's leaky_relu: derivative `slope` AT 0)
 *     a_eh   = exp(s_eh - m_ih) / z_ih,   m_ih the maximum of s over row i, z_ih = sum_{row i} exp(s - m_ih)
 *     out_e  = (sum_h a_eh) / H            heads summed h ascending, one IEEE division
 * u, v fp32 [n, H] at leading dimensions ldu, ldv >= H, 1 <= H <= DP_CSR_GAT_MAX_HEADS.  Scores, softmax and the mean run
 * in one pass over the stored entries; nothing of size nnz * H is written, and the backward recomputes every coefficient
 * from u, v and rowstat [n, 2H].  The launch form is N5's: a group of 4 / 16 / 64 lanes per row from the mean row length,
 * the lanes of a group on consecutive entries, a row longer than the group loops.  Every sum has one order — the lane's
 * entries ascending, then a DPP tree over the group — so a second run gives the same bits.  No atomics, no LDS.  A row
 * with one entry gives out = 1.0 exactly and contributes exactly 0 to every gradient; rows of 2^k entries whose v_j are
 * equal give exactly 2^-k (H = 1, 2, 4, 8).  n_rows == 0 or nnz == 0 writes nothing and returns DP_OK (the backward with
 * nnz == 0 and n > 0 still writes the zero du and dv); every refusal (DP_ERR_INVALID_ARG: a NULL or misaligned pointer,
 * an ld below H, a negative count, H outside 1 .. 8, a slope that is not finite) comes before any launch.
 *
 * dp_csr_gat_plan (host only): plan_out[DP_CSR_GAT_PLAN_INTS] = { lanes per row (4 while nnz <= 8 n_rows, 16 while
 * nnz <= 32 n_rows, 64 above), floats per load of the H contiguous values of v_j (4: H / 4 loads of 16 bytes, taken when
 * H % 4 == 0, ldv % 4 == 0 and the base is 16-byte aligned — v_misaligned == 0 —; 1 otherwise), entries a lane of the
 * forward and of the row pass of the backward keeps in registers (min(8 | 4 | 4, 16 / H): 16 scores at the most), rows
 * per workgroup (256 / lanes), the longest row that is read once (lanes * entries per lane) }, answered by the function
 * the launchers act on. */
#define DP_CSR_GAT_MAX_HEADS 8
#define DP_CSR_GAT_PLAN_INTS 5
int dp_csr_gat_plan(int n_rows, int nnz, int H, int ldv, int v_misaligned, int* plan_out);
/* out fp32 [nnz] in the order of indices; rowstat fp32 [n_rows, 2H] OVERWRITTEN: m_i0 .. m_i(H-1), z_i0 .. z_i(H-1), zeros
 * for a row without entries (which touches no out).  A row that fits the registers is read once; a longer one runs a
 * per-lane running maximum and sum per head and is read a second time.  One launch. */
int dp_csr_gat_fwd(const float* u, int ldu, const float* v, int ldv, const int* indptr, const int* indices, float* out,
                   float* rowstat, int n_rows, int nnz, int H, float slope, void* stream);
/* With g_e = dout_e / H:  t_ih = sum_{row i} a_eh g_e,  dpre_eh = a_eh (g_e - t_ih) (pre_eh > 0 ? 1 : slope),
 * du_ih OVERWRITTEN = sum_{row i} dpre_eh (zeros for a row without entries),  dv_ch OVERWRITTEN = sum_{column c} dpre_eh
 * (zeros for a column without entries), the column sum taken as row c of the transposed CSR, whose entry k is the stored
 * entry mirror[k] (int32 [nnz], always required) from row indices_t[k].  rowstat is the forward's; tdot fp32 [n, H] is the
 * workspace that receives t.  Two launches: over the rows (t, du), then over the transposed rows (dv, each coefficient
 * recomputed from u_r, v_c and the SOURCE row's rowstat_r and t_r; 16-byte loads there when H % 4 == 0, ldu % 4 == 0 and
 * u, rowstat and tdot are 16-byte aligned). */
int dp_csr_gat_bwd(const float* u, int ldu, const float* v, int ldv, const int* indptr, const int* indices,
                   const int* indptr_t, const int* indices_t, const int* mirror, const float* rowstat,
                   const float* dout, float* tdot, float* du, int lddu, float* dv, int lddv, int n, int nnz, int H,
                   float slope, void* stream);

/* ------------------------------------------------------------------ N7  multi-head GAT convolution on a CSR, attention
 * and aggregation fused.  z fp32 [n, H C] at ldz >= H C (head h: columns h C .. h C + C - 1), u, v fp32
 * [n, H] at ldu, ldv >= H, the CSR of a CsrGraph / CsrBatch (a batch is its block-diagonal CSR with GLOBAL columns).  The
 * stored values are NOT read: the coefficients a_eh of N6 (the same pre, s, m, z, a_eh = exp(s_eh - m_ih) / zsum_ih)
 * replace them, and are multiplied into the gathered neighbour rows in the pass that computes them:
 *     Y_ih = sum_{e in row i} a_eh z_j^h,     j = indices[e]
 *     mean_heads == 0:  y [n, H C],  y_i[h C + c] = Y_ih[c]
 *     mean_heads == 1:  y [n, C],    y_i[c] = (sum_h Y_ih[c]) / H      heads added h ascending, one IEEE division
 * Nothing of size nnz is written or saved; beyond the outputs only rowstat [n, 2H] (N6's layout: m, then zsum) and
 * tdot [n, H] exist.  Apart from the statistics pass: one wavefront per row, lanes across the H C columns, a
 * neighbour's row gathered as whole 256-byte (or, by 16-byte loads, 1 KiB) requests; a row of any length stays on its
 * wave.  Every sum has one order (stated in dp_csr_gat_conv.hip), so a second run gives the same bits.  No atomics, no
 * LDS.  A row with one entry gives y_i = z_j bit for bit (concat); rows of 2^k entries with equal v_j have a = 2^-k
 * exactly.  Limits: 1 <= H <= DP_CSR_GAT_MAX_HEADS, C >= 1 (DP_ERR_INVALID_ARG), H C <= DP_CSR_GAT_CONV_MAX_WIDTH
 * (DP_ERR_UNSUPPORTED above).  Every refusal (also: a NULL or misaligned pointer, an ld below its width, a negative
 * count, a slope that is not finite, mean_heads not 0 / 1) comes before any launch.  n_rows == 0 writes nothing;
 * nnz == 0 with n > 0 still writes the zero outputs.
 *
 * dp_csr_gat_conv_plan (host only): plan_out[DP_CSR_GAT_CONV_PLAN_INTS] = { floats per load of a gathered row (4: 16-byte
 * loads, taken when H C % 4 == 0, ldz % 4 == 0 and the base is 16-byte aligned — z_misaligned == 0 —; 1 otherwise),
 * column chunks per lane (the chunk is 64 floats-per-load columns; 1, 2, 4 or 8: the smallest that covers H C), 1 when
 * every 16-byte quad lies in one head (4-float loads and C % 4 == 0: one coefficient per quad, else one per column),
 * rows per workgroup (4), columns per lane, lanes per row of the forward's statistics pass (N6's rule: 4 while nnz <=
 * 8 n_rows, 16 while nnz <= 32 n_rows, 64 above) }, answered by the function the launchers act on.  The backward gathers z
 * (row pass) and dy (column pass) with one form: ask with ldz | lddy and with z_misaligned set when z or dy is off the
 * 16-byte grid, or when mean_heads and C % 4 != 0. */
#define DP_CSR_GAT_CONV_MAX_WIDTH 512
#define DP_CSR_GAT_CONV_PLAN_INTS 6
int dp_csr_gat_conv_plan(int n_rows, int nnz, int H, int C, int ldz, int z_misaligned, int* plan_out);
/* y OVERWRITTEN at ldy >= H C (concat) or >= C (mean), rowstat fp32 [n_rows, 2H] OVERWRITTEN; a row without entries gets
 * a zero y row and zero rowstat.  Two launches: the rows' statistics in N5's segmented form (a group of 4 / 16 / 64 lanes
 * per row, lanes across the entries, head after head), then the aggregation (one wave per row, lanes across the columns,
 * four neighbour rows in flight). */
int dp_csr_gat_conv_fwd(const float* z, int ldz, const float* u, int ldu, const float* v, int ldv, const int* indptr,
                        const int* indices, float* y, int ldy, float* rowstat, int n_rows, int nnz, int H, int C,
                        float slope, int mean_heads, void* stream);
/* With dY_ih = dy_i[h C ..] (concat, lddy >= H C) or dy_i / H (mean, lddy >= C):  g_eh = dY_ih . z_j^h,
 * t_ih = sum_{row i} a_eh g_eh,  dpre_eh = a_eh (g_eh - t_ih) (pre_eh > 0 ? 1 : slope),  du_ih = sum_{row i} dpre_eh,
 * dv_ch = sum_{column c} dpre_eh,  dz_c^h = sum_{column c} a_eh dY_r^h,  all OVERWRITTEN (zeros for a row / column
 * without entries); tdot fp32 [n, H] is the workspace that receives t.  The column sums run over row c of the transposed
 * CSR (indptr_t, indices_t; an undirected container passes the forward's arrays), whose entry k comes from source row
 * r = indices_t[k]: every coefficient is recomputed from u_r, v_c, rowstat_r, t_r, dy_r and z_c, so there is no mirror
 * argument.  rowstat is the forward's.  A row with one entry contributes exactly 0 to du and dv and dY_r to dz.  Two
 * launches: over the rows (t, then du: the row is gathered twice), then over the transposed rows (dv, dz). */
int dp_csr_gat_conv_bwd(const float* z, int ldz, const float* u, int ldu, const float* v, int ldv, const int* indptr,
                        const int* indices, const int* indptr_t, const int* indices_t, const float* rowstat,
                        const float* dy, int lddy, float* tdot, float* du, int lddu, float* dv, int lddv, float* dz,
                        int lddz, int n, int nnz, int H, int C, float slope, int mean_heads, void* stream);

/* ------------------------------------------------------------------ N8  GraphSAGE neighbour sampling fused with the mean
 * (DESIGN §4.10): MeanAggregator.forward(nodes, to_neighs, num_sample), aggregators.py:30-63 — the reference's
 * random.sample per node on the host (aggregators.py:38-42), its `set | {node}` under gcn (aggregators.py:44-47) and the
 * row-normalised mask times the embedding matrix (aggregators.py:50-62) — on the CSR of a CsrGraph / CsrBatch (GLOBAL
 * columns, unique and ascending in every row; the stored values are NOT read).  x fp32 [n, F] at ldx >= F.  Row r of the
 * result belongs to node i = nodes[r] (int32 [n_rows], distinct, in 0 .. n - 1; not checked here) or, with nodes == NULL
 * (then n_rows == n), to node r.  With d = the row's stored entries and k the sample size:
 *     key(i, j) = (h << 32) | j,  h = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *                 (i, j, 0, 0)  (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85)
 *     d <= k or k == DP_CSR_SAMPLE_ALL:  S(i) = N(i), thr_i = all-ones;   else thr_i = the k-th smallest key of the row
 *     and S(i) = { j : key(i, j) <= thr_i }: exactly k entries, uniform without replacement.
 *     self_mode DP_CSR_SAMPLE_SELF_NONE:    y_r = sum_{S(i)} x_j / cnt_i,  cnt_i = |S(i)|                       y [n_rows, F]
 *               DP_CSR_SAMPLE_SELF_GCN:     y_r = (sum_{S(i)} x_j + [i not in S(i)] x_i) / cnt_i,  cnt_i = |S(i) u {i}|
 *               DP_CSR_SAMPLE_SELF_CONCAT:  y_r = [x_i | sum_{S(i)} x_j / cnt_i],  cnt_i = |S(i)|              y [n_rows, 2F]
 * A row with cnt_i == 0 gets ZEROS in the mean part (the reference: 0 / 0 = NaN).  Saved for the backward: thr [n_rows]
 * (64-bit) and cnt [n_rows]; nothing of size nnz is written.  The order of every sum is fixed (dp_csr_sample.hip), no
 * atomics, a second run gives the same bits; with DP_CSR_SAMPLE_SELF_NONE a row with d <= k gives the bits of
 * dp_mean_aggregate_fwd.  Every refusal (k outside 1 .. DP_CSR_SAMPLE_MAX_K and not DP_CSR_SAMPLE_ALL, a self_mode that
 * is none of the three, a NULL or misaligned pointer, an ld below its width, a negative count, n_rows > n, n_rows != n
 * without nodes) comes before any launch; n_rows == 0 (forward), n == 0 (backward) or F == 0 returns without one.
 *
 * dp_csr_sample_mean_plan (host only, aggregators.py:30-63): plan_out[DP_CSR_SAMPLE_PLAN_INTS] = { rows per workgroup
 * (4: one wavefront each), workgroups of the forward, workgroups of the backward, the tier of a row of d entries (0: A,
 * d <= k, no hash; 1: B, k < d <= 64, one key per lane; 2: C, d > 64, chunks of 64), the row's key chunks (0 in tier A),
 * how many of them stay in registers (4 at most, the rest are recomputed), 64-column passes of the forward, 256-column
 * passes of the backward (the membership is evaluated once per pass) }, answered by the functions the launchers and the
 * kernels act on. */
#define DP_CSR_SAMPLE_ALL 0
#define DP_CSR_SAMPLE_MAX_K 64
#define DP_CSR_SAMPLE_SELF_NONE 0
#define DP_CSR_SAMPLE_SELF_GCN 1
#define DP_CSR_SAMPLE_SELF_CONCAT 2
#define DP_CSR_SAMPLE_PLAN_INTS 8
int dp_csr_sample_mean_plan(int n_rows, int n, int F, int k, int self_mode, int d, int* plan_out);
/* MeanAggregator.forward, aggregators.py:30-63.  y OVERWRITTEN at ldy >= F (2F under concat), thr (8-byte aligned) and
 * cnt OVERWRITTEN; `seed` carries the 64 bits of the seed.  One launch: a wavefront per target row draws the row's
 * sample once, then gathers it, lanes across the columns. */
int dp_csr_sample_mean_fwd(const float* x, int ldx, const int* indptr, const int* indices, const int* nodes, float* y,
                           int ldy, unsigned long long* thr, int* cnt, int n_rows, int n, int F, int k, int self_mode,
                           long seed, void* stream);
/* The backward of MeanAggregator.forward, aggregators.py:30-63 (autograd through aggregators.py:50-62 in the reference).
 *     dx_j = sum_{i in N^T(j), slot_i >= 0, key(i, j) <= thr_i} dy_slot(i) / cnt_i      sources ascending, one chain
 *            + dy_slot(j) / cnt_j   under gcn when j is a target and (j, j) was not sampled
 *            + dy_slot(j)[0 .. F)   under concat when j is a target (the neighbour terms then read dy[F .. 2F))
 * over the transposed CSR (indptr_t, indices_t; an undirected container passes the forward's arrays).  slot: int32 [n],
 * slot[nodes[r]] = r and -1 elsewhere, or NULL when every node is its own target row.  thr, cnt, seed: the forward's; an
 * all-ones thr_i skips the hash.  dx [n, F] at lddx >= F: EVERY row OVERWRITTEN (no zero-fill needed).  dy at lddy >= F
 * (2F under concat).  One launch, no atomics, a second run gives the same bits. */
int dp_csr_sample_mean_bwd(const float* dy, int lddy, const int* indptr_t, const int* indices_t, const int* slot,
                           const unsigned long long* thr, const int* cnt, float* dx, int lddx, int n, int F,
                           int self_mode, long seed, void* stream);

/* ------------------------------------------------------------------ N9  top-k (gPool / SAGPool) pooling on CSR
 * (DESIGN §4.11): keep the k_b best-scored nodes of every graph of a CsrGraph / CsrBatch, gate their features and build
 * the induced subgraph A' = A[perm][:, perm] as CSR on the device.  Graph b owns rows node_off[b] .. node_off[b+1]-1 and,
 * pooled, rows new_off[b] .. new_off[b+1]-1 with new_off[b+1] - new_off[b] = k_b, 1 <= k_b <= n_b, decided by the host.
 *     key_i = (ord(score_i) << 32) | (0xffffffff - local_i);  ord(bits) = ~bits for a set sign bit, bits | 0x80000000
 *             otherwise, after -0.0 is made +0.0 — every bit pattern has a place (a positive NaN above +inf, a negative
 *             one below -inf), so no score can send the selection out of bounds
 *     thr_b = the k_b-th largest key of graph b;  0 when k_b == n_b (no select: everything is kept)
 *     kept: key_i >= thr_b, exactly k_b nodes; new rows in ASCENDING old id: new_id[i] (int32 [n], -1 dropped) and
 *     perm[r] (int32 [n_out], the old global id of new row r)
 * Every refusal (a NULL or misaligned pointer, an ld below its width, a negative count, k_b outside 1 .. n_b, host tables
 * that do not add up, a capacity below the input's nnz, a workspace below the queried size) comes before any launch.
 *
 * dp_csr_topk_plan (host only): plan_out[DP_CSR_TOPK_PLAN_INTS] = { threads of the select workgroup (64 * ceil(max_n /
 * 256), 64 .. 1024), the tier of a graph of n_b nodes keeping k_b (0: k_b == n_b, no select; 1: at most 4 keys per
 * thread, held in registers; 2: the keys recomputed from score on every pass), its keys per thread (0 in tier 0), its
 * radix passes (4 for the score word + one per byte of n_b - 1; 0 in tier 0), the chunks of its prefix count, the
 * workgroups of the select (B), of an induce count / fill launch (32 kept rows each), the chunks of the one-workgroup
 * scan, the workgroups of the gather forward and of the backward (4 rows each) }, answered by the functions the
 * launchers and the kernels act on. */
#define DP_CSR_TOPK_PLAN_INTS 10
int dp_csr_topk_plan(int n, int n_out, int B, int max_n, int n_b, int k_b, int F, int* plan_out);
/* Workspace of dp_csr_topk_induce for n_out kept rows (one int per 32 rows, and the total). */
size_t dp_csr_topk_workspace_bytes(int n_out);
/* Select + renumber, ONE launch, one workgroup per graph.  score fp32 [n]; node_off / new_off int32 [B + 1] on the
 * DEVICE, node_off_host [B + 1] / kb_host [B] the same numbers on the HOST (checked here: 0 .. n, k_b in 1 .. n_b, the
 * k_b summing to n_out).  new_id [n], perm [n_out], thr [B] (8-byte aligned) OVERWRITTEN. */
int dp_csr_topk_select(const float* score, const int* node_off, const int* new_off, const int* node_off_host,
                       const int* kb_host, int* new_id, int* perm, unsigned long long* thr, int n, int n_out, int B,
                       void* stream);
/* The induced CSR of one direction, THREE launches (count per 32 kept rows; one workgroup scans the sums; recount,
 * offset and fill): indptr_out [n_out + 1], and for each kept entry, in stored order, indices_out (new GLOBAL column),
 * indices_local_out (minus new_off of the row's graph; NULL for a single graph: new_off and B are then not read) and
 * edge_map (its old position).  The three arrays hold `cap` entries, cap >= nnz = the entries of `indices`; the kept
 * count arrives in indptr_out[n_out].  A transposed CSR of its own takes a second call on indptr_t / indices_t. */
int dp_csr_topk_induce(const int* indptr, const int* indices, const int* new_id, const int* perm, const int* new_off,
                       int* indptr_out, int* indices_out, int* indices_local_out, int* edge_map, int n, int n_out, int B,
                       int nnz, int cap, void* workspace, size_t workspace_bytes, void* stream);
/* y[r] = x[perm[r]] * gate[perm[r]] (one fp32 multiply; gate NULL: a copy), y [n_out, F] at ldy OVERWRITTEN.  One
 * launch; n_out == 0 or F == 0 returns without one. */
int dp_csr_topk_gather_fwd(const float* x, int ldx, const float* gate, const int* perm, float* y, int ldy, int n, int n_out,
                           int F, void* stream);
/* dx[i] = dy[new_id[i]] * gate[i] and dgate[i] = sum_f dy[new_id[i], f] x[i, f] for a kept node, zeros for a dropped one:
 * EVERY row of dx [n, F] and dgate [n] OVERWRITTEN (no zero-fill, no atomics).  dgate: a lane sums its columns f = lane,
 * lane + 64, .. in one fma chain, then a butterfly over the 64 lanes — ceil(F / 64) + 6 roundings.  gate NULL: dx is the
 * scattered copy and dgate must be NULL; dgate NULL: x is not read.  One launch; n == 0 or F == 0 returns without one. */
int dp_csr_topk_gather_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gate, const int* new_id,
                           float* dx, int lddx, float* dgate, int n, int n_out, int F, void* stream);

/* ------------------------------------------------------------------ N10  sampled frontier blocks: nested GraphSAGE mini-batches
 * (DESIGN §4.12): MeanAggregator.forward, aggregators.py:30-63, evaluates the layer below on `unique_nodes_list` only,
 * the union of the sampled neighbourhoods (its lines 48-61).  For the target nodes T = nodes [n_rows] (int32, distinct,
 * in 0 .. n - 1; NULL with n_rows == n: every node), k and seed, with S(i) EXACTLY the sample of N8:
 *     src   int32 [n_src]  the ascending, duplicate-free ids of T u U_{i in T} S(i)  (T itself always, in every self mode)
 *     slot  int32 [n]      slot[src[s]] = s, -1 elsewhere
 *     thr [n_rows] (64-bit), cnt [n_rows]: as dp_csr_sample_mean_fwd writes them with DP_CSR_SAMPLE_SELF_NONE
 *     n_src int32 [1] ON THE DEVICE (the host reads it back once, 4 bytes)
 * The sampled mean then runs on COMPACT rows: x_src [n_src, F] holds the rows src of x, dx_src [n_src, F] their
 * gradients.  The selection, the compaction and the order of every sum are the code of N8 (dp_csr_sample_body.h), so with
 * x_src = x[src] the forward gives the bits of dp_csr_sample_mean_fwd(x, nodes = T), and the backward the rows src of
 * dp_csr_sample_mean_bwd's dx (whose other rows are zero).  The targets may be another block's src: that is the nested
 * form, and that block's slot then serves as tslot.
 * Indices built on the device are compared before they are used: a target id and a stored column against n, a slot
 * against n_src before x_src is read through it (out of range: the term is 0), src[s] against n, a fill position
 * against cap.  tslot's values index thr, cnt and dy and are the caller's (dp_csr_block_build's slot is below its n_src
 * by construction).  Every refusal (a NULL or misaligned pointer — thr 8-byte, the workspace 16-byte —, an ld below its
 * width, a negative count, n_rows > n, n_src > n, n_rows != n without nodes, k outside 1 .. DP_CSR_SAMPLE_MAX_K and not
 * DP_CSR_SAMPLE_ALL, a self_mode that is none of the three, cap or the workspace too small) comes before any launch;
 * n_rows == 0 (n_src == 0 in the backward), n == 0 or F == 0 returns without one.  No atomics; a second run gives the
 * same bits.
 *
 * dp_csr_block_plan (host only, aggregators.py:30-63): plan_out[DP_CSR_BLOCK_PLAN_INTS] = { flags per compaction chunk
 * (256), chunks of n nodes, steps of the one-workgroup scan (256 chunks each, a carry between them), the smallest cap
 * (min(n, n_rows (k + 1)); n under DP_CSR_SAMPLE_ALL), workgroups of the mark launch (4 target rows each), of the count
 * and of the fill launch (one per chunk), of the forward (4 rows each), of the backward at n_src = the smallest cap (4
 * rows each), 64-column passes of the forward, 256-column passes of the backward }, answered by the function the
 * launchers act on. */
#define DP_CSR_BLOCK_PLAN_INTS 11
int dp_csr_block_plan(int n_rows, int n, int F, int k, int* plan_out);
/* Workspace of dp_csr_block_build on n nodes (aggregators.py:30-63): one int per chunk of 256 nodes, and the total. */
size_t dp_csr_block_workspace_bytes(int n);
/* The block of MeanAggregator.forward's unique_nodes_list, aggregators.py:30-63.  FIVE launches whatever n_rows and n:
 * zero the flags (they live in slot); mark (one wavefront per target row runs N8's selection and stores 1 at the node and
 * at every selected column); count per chunk; one workgroup scans the counts; fill (src ascending, the flags turned into
 * slot in place).  slot [n], src [cap], n_src [1], thr [n_rows], cnt [n_rows] OVERWRITTEN; cap >= min(n, n_rows (k + 1)),
 * or n under DP_CSR_SAMPLE_ALL (n_src arrives as min(count, cap)).  No workgroup waits for another. */
int dp_csr_block_build(const int* indptr, const int* indices, const int* nodes, int n_rows, int n, int k, long seed,
                       int* slot, int* src, int cap, int* n_src, unsigned long long* thr, int* cnt, void* workspace,
                       size_t workspace_bytes, void* stream);
/* MeanAggregator.forward on the block's rows, aggregators.py:30-63: dp_csr_sample_mean_fwd with every gathered id, the
 * self row included, sent through slot.  x_src [n_src, F] at ldx >= F; y [n_rows, F | 2F], thr, cnt OVERWRITTEN (cnt by
 * self_mode's rule).  One launch. */
int dp_csr_block_mean_fwd(const float* x_src, int ldx, const int* indptr, const int* indices, const int* nodes,
                          const int* slot, int n_src, float* y, int ldy, unsigned long long* thr, int* cnt, int n_rows,
                          int n, int F, int k, int self_mode, long seed, void* stream);
/* Its backward, aggregators.py:30-63: one wavefront per src row s walks the transposed list of j = src[s] exactly as
 * dp_csr_sample_mean_bwd does.  tslot int32 [n]: the TARGETS' slot (tslot[nodes[r]] = r, -1 elsewhere; NULL: every node
 * its own target row).  EVERY row of dx_src [n_src, F] at lddx >= F OVERWRITTEN.  One launch. */
int dp_csr_block_mean_bwd(const float* dy, int lddy, const int* indptr_t, const int* indices_t, const int* tslot,
                          const int* src, int n_src, const unsigned long long* thr, const int* cnt, float* dx_src,
                          int lddx, int n, int F, int self_mode, long seed, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DIFFPOOL_HIP_H */
