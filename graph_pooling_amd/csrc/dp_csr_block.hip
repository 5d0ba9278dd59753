// Sampled frontier blocks for nested GraphSAGE mini-batches: MeanAggregator.forward evaluates the layer
// below on `unique_nodes_list` only, the union of the sampled neighbourhoods (aggregators.py:30-63, lines 48-61).  For
// target nodes T (m distinct ids), k and a seed, the block is
//
//     src    int32 [n_src]  the ascending, duplicate-free ids of  T u U_{i in T} S(i),  S(i) the sample of §4.10
//     slot   int32 [n]      slot[src[s]] = s, -1 elsewhere
//     thr, cnt  [m]         what dp_csr_sample_mean_fwd writes with DP_CSR_SAMPLE_SELF_NONE
//     n_src                 on the device; the host reads it back once
//
// and the sampled mean then runs on COMPACT rows: x_src [n_src, F] in, y [m, F | 2F] out, dx_src [n_src, F] back.  The
// sample is a pure function of (seed, i, j), so this is the whole-graph computation of dp_csr_sample.hip restricted to
// the rows that matter, and gives its bits: the forward and the backward are dp_csr_sample_body.h's bodies with
// BLOCK = true, every gathered id sent through slot[].
//
// Build, five launches whatever m and n (the launches are the hand-off: no workgroup waits for another, no look-back, no
// atomics): zero the n flags (they live in `slot`); MARK, one wavefront per target row runs sm_select and stores the
// constant 1 at i and at every selected j; COUNT the set flags of every chunk of BK_CHUNK = 256 nodes; one workgroup
// SCANs the chunk counts, BK_SCAN = 256 at a step with a carry from step to step, and writes n_src; FILL recounts its
// chunk, offsets it from its scanned base, writes src ascending and turns the flags into slot in place.
//
// Every index built on the device is compared before it is used: a stored column against n before its flag is touched, a
// fill position against cap before the store (n_src is reported as min(count, cap)), a target id against n before
// indptr is read (the targets may be another block's src), and in the mean kernels a slot against n_src, src[s] against
// n.  Plain vector stores, plain C++ compares; a second run gives the same bits.
#include "dp_csr_sample_body.h"

namespace dp {
namespace {

constexpr int BK_CHUNK = 256;                                 // flags per compaction chunk: one workgroup, one flag a thread
constexpr int BK_SCAN = 256;                                  // chunk counts per scan step (the one workgroup's threads)

// the plan: one rule, for the launchers and for dp_csr_block_plan
struct BlockPick {
    int chunk, chunks, scan_steps, min_cap, grid_mark, grid_count, grid_fill, grid_fwd, grid_bwd, col_passes_fwd,
        col_passes_bwd;
};
inline int block_min_cap(int n_rows, int n, int k) {
    if (k == DP_CSR_SAMPLE_ALL) return n;
    const long most = (long)n_rows * (k + 1);
    return most < n ? (int)most : n;
}
inline int block_row_grid(int rows) { return cdiv(rows, SM_THREADS / 64); }
BlockPick block_pick(int n_rows, int n, int F, int k) {
    BlockPick p;
    p.chunk = BK_CHUNK;
    p.chunks = cdiv(n, BK_CHUNK);
    p.scan_steps = cdiv(p.chunks, BK_SCAN);
    p.min_cap = block_min_cap(n_rows, n, k);
    p.grid_mark = block_row_grid(n_rows);
    p.grid_count = p.chunks;
    p.grid_fill = p.chunks;
    p.grid_fwd = block_row_grid(n_rows);
    p.grid_bwd = block_row_grid(p.min_cap);                   // at n_src = its bound; the launcher passes the n_src it is given
    p.col_passes_fwd = cdiv(F, 64);
    p.col_passes_bwd = cdiv(F, SM_BWD_COLS);
    return p;
}
inline size_t block_ws_bytes(int n) { return (((size_t)cdiv(n, BK_CHUNK) + 1) * sizeof(int) + 15) & ~size_t(15); }

// ------------------------------------------------------------------------------------------------ the build
__global__ __launch_bounds__(BK_CHUNK) void k_csr_block_zero(int* __restrict__ flag, int n) {
    const long i = (long)blockIdx.x * BK_CHUNK + threadIdx.x;
    if (i < n) flag[i] = 0;
}

// one wavefront per target row: §4.10's selection, then the constant 1 at the node and at every selected column
__global__ __launch_bounds__(SM_THREADS) void k_csr_block_mark(const int* __restrict__ indptr,
                                                               const int* __restrict__ indices,
                                                               const int* __restrict__ nodes, int* __restrict__ flag,
                                                               u64* __restrict__ thr_out, int* __restrict__ cnt_out,
                                                               int n_rows, int n, int k, unsigned k0, unsigned k1) {
    const long r = (long)blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int i = nodes ? nodes[r] : (int)r;
    const SmRow R = sm_select<true>(indptr, indices, i, n, k, DP_CSR_SAMPLE_SELF_NONE, k0, k1, lane);
    if (lane == 0) {
        thr_out[r] = R.thr;
        cnt_out[r] = R.ns;
        if ((unsigned)i < (unsigned)n) flag[i] = 1;
    }
    if (R.all) {
        for (int e = R.beg + lane; e < R.end; e += 64) {
            const int j = indices[e];
            if ((unsigned)j < (unsigned)n) flag[j] = 1;
        }
    } else if (lane < R.ns) {
        if ((unsigned)R.mine < (unsigned)n) flag[R.mine] = 1;
    }
}

// the set flags of the workgroup's chunk, before this thread (ascending id) and in all: every thread gets both
__device__ __forceinline__ void bk_chunk_count(bool set, int* wtot, int& before, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 bal = __ballot(set);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    before = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < BK_CHUNK / 64; ++w) {
        const int c = wtot[w];
        before += w < wave ? c : 0;
        total += c;
    }
}

__global__ __launch_bounds__(BK_CHUNK) void k_csr_block_count(const int* __restrict__ flag, int* __restrict__ csum, int n) {
    __shared__ int wtot[BK_CHUNK / 64];
    const long i = (long)blockIdx.x * BK_CHUNK + threadIdx.x;
    int before, total;
    bk_chunk_count(i < n && flag[i] != 0, wtot, before, total);
    if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

// one workgroup: csum[0 .. nchunks) -> its exclusive prefix sums in place, BK_SCAN at a step with a carry; the total
// into csum[nchunks], and min(total, cap) into n_src
__global__ __launch_bounds__(BK_SCAN) void k_csr_block_scan(int* __restrict__ csum, int nchunks, int* __restrict__ n_src,
                                                            int cap) {
    __shared__ int wtot[BK_SCAN / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < nchunks; base += BK_SCAN) {
        const int c = base + tid;
        const int v = c < nchunks ? csum[c] : 0;
        int s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d, 64);
            if (lane >= d) s += t;
        }
        if (lane == 63) wtot[wave] = s;
        __syncthreads();
        int off = carry, tot = 0;
#pragma unroll
        for (int w = 0; w < BK_SCAN / 64; ++w) {
            const int t = wtot[w];
            off += w < wave ? t : 0;
            tot += t;
        }
        if (c < nchunks) csum[c] = off + s - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        csum[nchunks] = carry;
        *n_src = carry < cap ? carry : cap;
    }
}

__global__ __launch_bounds__(BK_CHUNK) void k_csr_block_fill(int* __restrict__ slot, const int* __restrict__ csum,
                                                             int* __restrict__ src, int n, int cap) {
    __shared__ int wtot[BK_CHUNK / 64];
    const long i = (long)blockIdx.x * BK_CHUNK + threadIdx.x;
    const bool set = i < n && slot[i] != 0;
    int before, total;
    bk_chunk_count(set, wtot, before, total);
    if (i < n) {
        const int pos = csum[blockIdx.x] + before;
        const bool ok = set && pos >= 0 && pos < cap;         // pos < cap holds by the host's bound; the guard keeps src in bounds
        if (ok) src[pos] = (int)i;
        slot[i] = ok ? pos : -1;
    }
}

// ------------------------------------------------------------------------------------------------ the mean on compact rows
__global__ __launch_bounds__(SM_THREADS) void k_csr_block_mean_fwd(const float* __restrict__ x_src, int ldx,
                                                                   const int* __restrict__ indptr,
                                                                   const int* __restrict__ indices,
                                                                   const int* __restrict__ nodes,
                                                                   const int* __restrict__ slot, int n_src,
                                                                   float* __restrict__ y, int ldy,
                                                                   u64* __restrict__ thr_out, int* __restrict__ cnt_out,
                                                                   int n_rows, int n, int F, int k, int mode, unsigned k0,
                                                                   unsigned k1) {
    sm_fwd_body<true>(x_src, ldx, indptr, indices, nodes, slot, n_src, y, ldy, thr_out, cnt_out, n_rows, n, F, k, mode, k0,
                      k1);
}

__global__ __launch_bounds__(SM_THREADS) void k_csr_block_mean_bwd(const float* __restrict__ dy, int lddy,
                                                                   const int* __restrict__ indptr_t,
                                                                   const int* __restrict__ indices_t,
                                                                   const int* __restrict__ tslot,
                                                                   const int* __restrict__ src, int n_src,
                                                                   const u64* __restrict__ thr,
                                                                   const int* __restrict__ cnt,
                                                                   float* __restrict__ dx_src, int lddx, int n, int F,
                                                                   int mode, unsigned k0, unsigned k1) {
    sm_bwd_body<true>(dy, lddy, indptr_t, indices_t, tslot, src, n_src, thr, cnt, dx_src, lddx, n, F, mode, k0, k1);
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_csr_block_plan(int n_rows, int n, int F, int k, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n_rows);
    DP_NONNEG(n);
    DP_NONNEG(F);
    SM_SHAPE(k, DP_CSR_SAMPLE_SELF_NONE);
    DP_CHECK(n_rows <= n, DP_ERR_INVALID_ARG, "n_rows=%d exceeds n=%d", n_rows, n);
    const BlockPick p = block_pick(n_rows, n, F, k);
    const int plan[DP_CSR_BLOCK_PLAN_INTS] = {p.chunk,      p.chunks,    p.scan_steps, p.min_cap,  p.grid_mark,     p.grid_count,
                                              p.grid_fill,  p.grid_fwd,  p.grid_bwd,   p.col_passes_fwd, p.col_passes_bwd};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

size_t dp_csr_block_workspace_bytes(int n) { return block_ws_bytes(n < 0 ? 0 : n); }

int dp_csr_block_build(const int* indptr, const int* indices, const int* nodes, int n_rows, int n, int k, long seed,
                       int* slot, int* src, int cap, int* n_src, unsigned long long* thr, int* cnt, void* workspace,
                       size_t workspace_bytes, void* stream) {
    DP_PTR(indptr); DP_PTR(indices); DP_PTR(slot); DP_PTR(src); DP_PTR(n_src); DP_PTR(thr); DP_PTR(cnt);
    DP_ALIGNED8(thr);
    if (nodes) DP_ALIGNED4(nodes);
    DP_NONNEG(n_rows);
    DP_NONNEG(n);
    SM_SHAPE(k, DP_CSR_SAMPLE_SELF_NONE);
    DP_CHECK(n_rows <= n, DP_ERR_INVALID_ARG, "n_rows=%d exceeds n=%d", n_rows, n);
    DP_CHECK(nodes || n_rows == n, DP_ERR_INVALID_ARG, "n_rows=%d differs from n=%d without nodes", n_rows, n);
    const BlockPick p = block_pick(n_rows, n, 0, k);
    DP_CHECK(cap >= p.min_cap, DP_ERR_INVALID_ARG, "cap=%d is below the block's bound %d", cap, p.min_cap);
    DP_ALIGNED16(workspace, false, "workspace must be there and 16-byte aligned");
    DP_CHECK(workspace_bytes >= block_ws_bytes(n), DP_ERR_WORKSPACE, "workspace too small: need >= %zu bytes, have %zu",
             block_ws_bytes(n), workspace_bytes);
    if (n_rows == 0 || n == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    int* csum = (int*)workspace;
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(k_csr_block_zero, dim3(p.chunks), dim3(BK_CHUNK), 0, q.stream, slot, n);
    q.check_launch("k_csr_block_zero");
    hipLaunchKernelGGL(k_csr_block_mark, dim3(p.grid_mark), dim3(SM_THREADS), 0, q.stream, indptr, indices, nodes, slot, thr,
                       cnt, n_rows, n, k, (unsigned)s, (unsigned)(s >> 32));
    q.check_launch("k_csr_block_mark");
    hipLaunchKernelGGL(k_csr_block_count, dim3(p.grid_count), dim3(BK_CHUNK), 0, q.stream, slot, csum, n);
    q.check_launch("k_csr_block_count");
    hipLaunchKernelGGL(k_csr_block_scan, dim3(1), dim3(BK_SCAN), 0, q.stream, csum, p.chunks, n_src, cap);
    q.check_launch("k_csr_block_scan");
    hipLaunchKernelGGL(k_csr_block_fill, dim3(p.grid_fill), dim3(BK_CHUNK), 0, q.stream, slot, csum, src, n, cap);
    q.check_launch("k_csr_block_fill");
    return q.err;
}

int dp_csr_block_mean_fwd(const float* x_src, int ldx, const int* indptr, const int* indices, const int* nodes,
                          const int* slot, int n_src, float* y, int ldy, unsigned long long* thr, int* cnt, int n_rows,
                          int n, int F, int k, int self_mode, long seed, void* stream) {
    DP_PTR(x_src); DP_PTR(indptr); DP_PTR(indices); DP_PTR(slot); DP_PTR(y); DP_PTR(thr); DP_PTR(cnt);
    DP_ALIGNED8(thr);
    if (nodes) DP_ALIGNED4(nodes);
    DP_NONNEG(n_src);
    DP_NONNEG(n_rows);
    DP_NONNEG(n);
    DP_NONNEG(F);
    SM_SHAPE(k, self_mode);
    DP_CHECK(n_rows <= n, DP_ERR_INVALID_ARG, "n_rows=%d exceeds n=%d", n_rows, n);
    DP_CHECK(n_src <= n, DP_ERR_INVALID_ARG, "n_src=%d exceeds n=%d", n_src, n);
    DP_CHECK(nodes || n_rows == n, DP_ERR_INVALID_ARG, "n_rows=%d differs from n=%d without nodes", n_rows, n);
    DP_LD(ldx, F);
    DP_LD(ldy, self_mode == DP_CSR_SAMPLE_SELF_CONCAT ? 2 * F : F);
    if (n_rows == 0 || n == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(k_csr_block_mean_fwd, dim3(block_pick(n_rows, n, F, k).grid_fwd), dim3(SM_THREADS), 0, q.stream,
                       x_src, ldx, indptr, indices, nodes, slot, n_src, y, ldy, thr, cnt, n_rows, n, F, k, self_mode,
                       (unsigned)s, (unsigned)(s >> 32));
    q.check_launch("k_csr_block_mean_fwd");
    return q.err;
}

int dp_csr_block_mean_bwd(const float* dy, int lddy, const int* indptr_t, const int* indices_t, const int* tslot,
                          const int* src, int n_src, const unsigned long long* thr, const int* cnt, float* dx_src,
                          int lddx, int n, int F, int self_mode, long seed, void* stream) {
    DP_PTR(dy); DP_PTR(indptr_t); DP_PTR(indices_t); DP_PTR(src); DP_PTR(thr); DP_PTR(cnt); DP_PTR(dx_src);
    DP_ALIGNED8(thr);
    if (tslot) DP_ALIGNED4(tslot);
    DP_NONNEG(n_src);
    DP_NONNEG(n);
    DP_NONNEG(F);
    SM_SHAPE(DP_CSR_SAMPLE_ALL, self_mode);
    DP_CHECK(n_src <= n, DP_ERR_INVALID_ARG, "n_src=%d exceeds n=%d", n_src, n);
    DP_LD(lddy, self_mode == DP_CSR_SAMPLE_SELF_CONCAT ? 2 * F : F);
    DP_LD(lddx, F);
    if (n_src == 0 || n == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(k_csr_block_mean_bwd, dim3(block_row_grid(n_src)), dim3(SM_THREADS), 0, q.stream, dy, lddy, indptr_t,
                       indices_t, tslot, src, n_src, thr, cnt, dx_src, lddx, n, F, self_mode, (unsigned)s,
                       (unsigned)(s >> 32));
    q.check_launch("k_csr_block_mean_bwd");
    return q.err;
}

}  // extern "C"
