// GraphSAGE neighbour sampling on the device, fused with the mean: MeanAggregator.forward with
// num_sample = k (aggregators.py:30-63) on the CSR of a CsrGraph / CsrBatch.  The reference draws random.sample per node
// on the host; here the sample is a pure function of (seed, i, j), so the forward draws it and takes its mean in one
// launch, saves O(m), and the backward re-derives it over the transposed CSR — nothing of size nnz is written.
//
//     key(i, j) = (h(seed, i, j) << 32) | j,   h = word 0 of Philox4x32-10, key (seed lo, seed hi), counter (i, j, 0, 0)
//     d = |N(i)| <= k, or k == DP_CSR_SAMPLE_ALL:  S(i) = N(i),  thr_i = all-ones
//     otherwise:  thr_i = the k-th smallest key of row i,  S(i) = { j in N(i) : key(i, j) <= thr_i }   (exactly k)
//     none:    y_r = sum_{S(i)} x_j / cnt_i,                    cnt_i = |S(i)|
//     gcn:     y_r = (sum_{S(i)} x_j + [i not in S(i)] x_i) / cnt_i,   cnt_i = |S(i) u {i}|
//     concat:  y_r = [x_i | sum_{S(i)} x_j / cnt_i],            cnt_i = |S(i)|
//     cnt_i == 0: zeros in the mean part (the reference divides 0 by 0)
//     dx_j = sum_{i in N^T(j), i a target, key(i, j) <= thr_i} dy_slot(i) / cnt_i   (+ the self term of gcn / concat)
//
// Forward: one wavefront per target row, lanes across the feature columns, the launch form of dp_meanagg.hip.  The
// selection happens ONCE per row, before the column loop:
//   tier A (d <= k)       no hash, no selection: the gather loop of dp_meanagg.hip over all stored ids, its order of
//                         summation and its scale, so self_mode "none" gives the bits of dp_mean_aggregate_fwd.
//   tier B (k < d <= 64)  one key per lane.  The k-th smallest by a bitwise radix select from the top bit down: per bit
//                         one 64-lane ballot and a popcount of the keys that share the decided prefix and have a 0 there;
//                         it stops as soon as one candidate is left (about log2 d + 2 bits for hashed keys; 64 at worst).
//   tier C (d > 64)       the same select over ceil(d / 64) chunks, the counts summed over the chunks per bit.
// Where the keys of tier C live: the first SM_KREG = 4 chunks (256 entries, 8 VGPRs + 4 for the ids) stay in registers,
// chunks beyond them are RECOMPUTED from indices on every visit.  LDS would either cap the row length or cost
// occupancy for every row to serve a hub row, and a spill-free register file cannot hold an unbounded row; 256 entries
// cover all but hub rows, and a hub row pays ~10 Philox evaluations per entry beyond the 256th, once per row (not per
// feature column).
// The selected ids are then compacted in ascending column order into ONE id per lane (k <= 64): chunk after chunk, lane
// base + t pulls the id at the t-th set bit of the chunk's ballot (a popcount binary search, then one __shfl).  The
// column loop hands them round by readlane exactly as tier A does: batches of 64 ids, four partial sums, entry q of a
// batch into partial q % 4 while four whole entries remain, the rest into partial 0, (s0 + s1) + (s2 + s3); gcn's self
// row joins partial 0 last; then * (1 / cnt).
//
// Backward: one wavefront per column j of the transposed CSR, 64 entries at a time: each lane loads its source i,
// slot_i, thr_i, cnt_i, tests key(i, j) <= thr_i (an all-ones thr_i skips the hash), the members are taken in ascending
// source order from the ballot, four dy rows in flight, ONE chain acc += dy / cnt (an IEEE division), the self term last.
// The membership is evaluated once per 256 feature columns.  No atomics, no LDS, plain vector stores, every dx row
// written; a second run gives the same bits.
//
// The device code lives in dp_csr_sample_body.h, which dp_csr_block.hip (the compact form on sampled blocks, DESIGN
// §4.12) instantiates as well: the kernels here are its BLOCK = false form.
#include "dp_csr_sample_body.h"

namespace dp {
namespace {

struct SamplePick {
    int rows_per_wg, grid_fwd, grid_bwd, tier, chunks, chunks_reg, col_passes_fwd, col_passes_bwd;
};
SamplePick sample_pick(int n_rows, int n, int F, int k, int d) {
    SamplePick p;
    p.rows_per_wg = SM_THREADS / 64;
    p.grid_fwd = cdiv(n_rows, p.rows_per_wg);
    p.grid_bwd = cdiv(n, p.rows_per_wg);
    p.tier = sm_tier(d, k);
    p.chunks = p.tier == 0 ? 0 : cdiv(d, 64);
    p.chunks_reg = p.chunks < SM_KREG ? p.chunks : SM_KREG;
    p.col_passes_fwd = cdiv(F, 64);
    p.col_passes_bwd = cdiv(F, SM_BWD_COLS);
    return p;
}

__global__ __launch_bounds__(SM_THREADS) void k_csr_sample_mean_fwd(const float* __restrict__ x, int ldx,
                                                                    const int* __restrict__ indptr,
                                                                    const int* __restrict__ indices,
                                                                    const int* __restrict__ nodes, float* __restrict__ y,
                                                                    int ldy, u64* __restrict__ thr_out,
                                                                    int* __restrict__ cnt_out, int n_rows, int F, int k,
                                                                    int mode, unsigned k0, unsigned k1) {
    sm_fwd_body<false>(x, ldx, indptr, indices, nodes, nullptr, 0, y, ldy, thr_out, cnt_out, n_rows, 0, F, k, mode, k0, k1);
}

__global__ __launch_bounds__(SM_THREADS) void k_csr_sample_mean_bwd(const float* __restrict__ dy, int lddy,
                                                                    const int* __restrict__ indptr_t,
                                                                    const int* __restrict__ indices_t,
                                                                    const int* __restrict__ slot,
                                                                    const u64* __restrict__ thr,
                                                                    const int* __restrict__ cnt, float* __restrict__ dx,
                                                                    int lddx, int n, int F, int mode, unsigned k0,
                                                                    unsigned k1) {
    sm_bwd_body<false>(dy, lddy, indptr_t, indices_t, slot, nullptr, 0, thr, cnt, dx, lddx, n, F, mode, k0, k1);
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_csr_sample_mean_plan(int n_rows, int n, int F, int k, int self_mode, int d, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n_rows);
    DP_NONNEG(n);
    DP_NONNEG(F);
    DP_NONNEG(d);
    SM_SHAPE(k, self_mode);
    DP_CHECK(n_rows <= n, DP_ERR_INVALID_ARG, "n_rows=%d exceeds n=%d", n_rows, n);
    const SamplePick p = sample_pick(n_rows, n, F, k, d);
    const int plan[DP_CSR_SAMPLE_PLAN_INTS] = {p.rows_per_wg,    p.grid_fwd,       p.grid_bwd,      p.tier, p.chunks,
                                               p.chunks_reg,     p.col_passes_fwd, p.col_passes_bwd};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

int dp_csr_sample_mean_fwd(const float* x, int ldx, const int* indptr, const int* indices, const int* nodes, float* y,
                           int ldy, unsigned long long* thr, int* cnt, int n_rows, int n, int F, int k, int self_mode,
                           long seed, void* stream) {
    DP_PTR(x); DP_PTR(indptr); DP_PTR(indices); DP_PTR(y); DP_PTR(thr); DP_PTR(cnt);
    DP_ALIGNED8(thr);
    if (nodes) DP_ALIGNED4(nodes);
    DP_NONNEG(n_rows);
    DP_NONNEG(n);
    DP_NONNEG(F);
    SM_SHAPE(k, self_mode);
    DP_CHECK(n_rows <= n, DP_ERR_INVALID_ARG, "n_rows=%d exceeds n=%d", n_rows, n);
    DP_CHECK(nodes || n_rows == n, DP_ERR_INVALID_ARG, "n_rows=%d differs from n=%d without nodes", n_rows, n);
    DP_LD(ldx, F);
    DP_LD(ldy, self_mode == DP_CSR_SAMPLE_SELF_CONCAT ? 2 * F : F);
    if (n_rows == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const SamplePick p = sample_pick(n_rows, n, F, k, 0);
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(k_csr_sample_mean_fwd, dim3(p.grid_fwd), dim3(SM_THREADS), 0, q.stream, x, ldx, indptr, indices,
                       nodes, y, ldy, thr, cnt, n_rows, F, k, self_mode, (unsigned)s, (unsigned)(s >> 32));
    q.check_launch("k_csr_sample_mean_fwd");
    return q.err;
}

int dp_csr_sample_mean_bwd(const float* dy, int lddy, const int* indptr_t, const int* indices_t, const int* slot,
                           const unsigned long long* thr, const int* cnt, float* dx, int lddx, int n, int F,
                           int self_mode, long seed, void* stream) {
    DP_PTR(dy); DP_PTR(indptr_t); DP_PTR(indices_t); DP_PTR(thr); DP_PTR(cnt); DP_PTR(dx);
    DP_ALIGNED8(thr);
    if (slot) DP_ALIGNED4(slot);
    DP_NONNEG(n);
    DP_NONNEG(F);
    SM_SHAPE(DP_CSR_SAMPLE_ALL, self_mode);
    DP_LD(lddy, self_mode == DP_CSR_SAMPLE_SELF_CONCAT ? 2 * F : F);
    DP_LD(lddx, F);
    if (n == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const SamplePick p = sample_pick(n, n, F, DP_CSR_SAMPLE_ALL, 0);
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(k_csr_sample_mean_bwd, dim3(p.grid_bwd), dim3(SM_THREADS), 0, q.stream, dy, lddy, indptr_t,
                       indices_t, slot, thr, cnt, dx, lddx, n, F, self_mode, (unsigned)s, (unsigned)(s >> 32));
    q.check_launch("k_csr_sample_mean_bwd");
    return q.err;
}

}  // extern "C"
