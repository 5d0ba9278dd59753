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
#include "dp_entry.h"

namespace dp {
namespace {

typedef unsigned long long u64;

constexpr int SM_THREADS = 256;                               // four waves, one row each
constexpr int SM_KREG = 4;                                    // key chunks of a row held in registers
constexpr int SM_BWD_COLS = 256;                              // feature columns per membership evaluation (backward)
constexpr u64 SM_ALL = ~0ull;                                 // never a key: the low word is a node id < 2^31

__host__ __device__ inline unsigned philox_word0(unsigned k0, unsigned k1, unsigned c0, unsigned c1) {
    unsigned c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}
__host__ __device__ inline u64 sm_key(unsigned k0, unsigned k1, int i, int j) {
    return ((u64)philox_word0(k0, k1, (unsigned)i, (unsigned)j) << 32) | (unsigned)j;
}

// 0 / 1 / 2 = tier A / B / C of a row of d stored entries: the one rule, for the kernel and for the plan
__host__ __device__ inline int sm_tier(int d, int k) { return (k == DP_CSR_SAMPLE_ALL || d <= k) ? 0 : (d <= 64 ? 1 : 2); }

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

__device__ __forceinline__ u64 sm_readlane64(u64 v, int src) {     // src wave-uniform
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// position of the t-th (0-based) set bit of m; 0 <= t < popcount(m)
__device__ __forceinline__ int sm_nth_set_bit(u64 m, int t) {
    unsigned w = (unsigned)m;
    int pos = 0, c = __popc(w);
    if (t >= c) {
        t -= c;
        w = (unsigned)(m >> 32);
        pos = 32;
    }
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        const unsigned low = w & ((1u << s) - 1u);
        c = __popc(low);
        if (t >= c) {
            t -= c;
            w >>= s;
            pos += s;
        } else {
            w = low;
        }
    }
    return pos;
}

// cnt ids of `mine` (lane q holds id q), handed round by readlane: the inner loop of dp_meanagg.hip
__device__ __forceinline__ void sm_gather(const float* __restrict__ x, int ldx, int f, int mine, int cnt, float& s0,
                                          float& s1, float& s2, float& s3) {
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {
        const long r0 = __builtin_amdgcn_readlane(mine, j), r1 = __builtin_amdgcn_readlane(mine, j + 1);
        const long r2 = __builtin_amdgcn_readlane(mine, j + 2), r3 = __builtin_amdgcn_readlane(mine, j + 3);
        const float v0 = x[r0 * ldx + f], v1 = x[r1 * ldx + f];
        const float v2 = x[r2 * ldx + f], v3 = x[r3 * ldx + f];
        s0 += v0; s1 += v1; s2 += v2; s3 += v3;
    }
    for (; j < cnt; ++j) s0 += x[(long)__builtin_amdgcn_readlane(mine, j) * ldx + f];
}

__global__ __launch_bounds__(SM_THREADS) void k_csr_sample_mean_fwd(const float* __restrict__ x, int ldx,
                                                                    const int* __restrict__ indptr,
                                                                    const int* __restrict__ indices,
                                                                    const int* __restrict__ nodes, float* __restrict__ y,
                                                                    int ldy, u64* __restrict__ thr_out,
                                                                    int* __restrict__ cnt_out, int n_rows, int F, int k,
                                                                    int mode, unsigned k0, unsigned k1) {
    const long r = (long)blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int i = nodes ? nodes[r] : (int)r;
    const int beg = indptr[i], end = indptr[i + 1], d = end - beg;
    const bool all = sm_tier(d, k) == 0;
    u64 thr = SM_ALL;
    int ns = d, mine = 0;
    bool selfin = false;
    if (!all) {
        const int nch = (d + 63) >> 6;
        // the keys of the first SM_KREG chunks, one entry per lane and chunk; a lane beyond the row holds SM_ALL
        u64 kr[SM_KREG];
        int idr[SM_KREG];
#pragma unroll
        for (int c = 0; c < SM_KREG; ++c) {
            kr[c] = SM_ALL;
            idr[c] = 0;
            if (c < nch && c * 64 + lane < d) {
                idr[c] = indices[beg + c * 64 + lane];
                kr[c] = sm_key(k0, k1, i, idr[c]);
            }
        }
        auto key_at = [&](int c, int& id) -> u64 {            // c wave-uniform
            u64 key = SM_ALL;
            id = 0;
            if (c < SM_KREG) {
#pragma unroll
                for (int q = 0; q < SM_KREG; ++q)
                    if (q == c) key = kr[q], id = idr[q];
            } else if (c * 64 + lane < d) {
                id = indices[beg + c * 64 + lane];
                key = sm_key(k0, k1, i, id);
            }
            return key;
        };
        // bitwise select of the k-th smallest: `prefix` on the decided bits `mask`, kk-th smallest of the ncand candidates
        u64 prefix = 0ull, mask = 0ull;
        int kk = k, ncand = nch * 64;
        for (int b = 63; b >= 0 && ncand > 1; --b) {
            const u64 m2 = mask | (1ull << b);
            int c0 = 0, id;
            for (int c = 0; c < nch; ++c) c0 += __popcll(__ballot((key_at(c, id) & m2) == prefix));
            if (kk <= c0) {
                ncand = c0;
            } else {
                prefix |= 1ull << b;
                kk -= c0;
                ncand -= c0;
            }
            mask = m2;
        }
        for (int c = 0; c < nch; ++c) {                       // the one key left on the prefix
            int id;
            const u64 key = key_at(c, id);
            const u64 bl = __ballot((key & mask) == prefix);
            if (bl) thr = sm_readlane64(key, __ffsll((long long)bl) - 1);
        }
        // the selected ids, ascending, one per lane
        int base = 0;
        for (int c = 0; c < nch; ++c) {
            int id;
            const u64 key = key_at(c, id);
            const bool sel = key <= thr;
            const u64 bl = __ballot(sel);
            if (mode == DP_CSR_SAMPLE_SELF_GCN) selfin = selfin || __ballot(sel && id == i) != 0ull;
            const int nc = __popcll(bl);
            if (nc) {                                         // wave-uniform
                const int t = lane - base;
                const int src = sm_nth_set_bit(bl, min(max(t, 0), nc - 1));
                const int v = __shfl(id, src, 64);
                if (t >= 0 && t < nc) mine = v;
            }
            base += nc;
        }
        ns = base;
    } else if (mode == DP_CSR_SAMPLE_SELF_GCN) {
        for (int e0 = beg; e0 < end; e0 += 64)
            selfin = selfin || __ballot(e0 + lane < end && indices[min(e0 + lane, end - 1)] == i) != 0ull;
    }
    const bool addself = mode == DP_CSR_SAMPLE_SELF_GCN && !selfin;
    const int cnt_i = ns + (addself ? 1 : 0);
    if (lane == 0) {
        thr_out[r] = thr;
        cnt_out[r] = cnt_i;
    }
    const float scale = cnt_i ? 1.f / (float)cnt_i : 0.f;
    const int yoff = mode == DP_CSR_SAMPLE_SELF_CONCAT ? F : 0;
    for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = min(f0 + lane, F - 1);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (all) {
            for (int e0 = beg; e0 < end; e0 += 64) {
                const int cnt = min(64, end - e0);
                sm_gather(x, ldx, f, indices[e0 + min(lane, cnt - 1)], cnt, s0, s1, s2, s3);
            }
        } else {
            sm_gather(x, ldx, f, mine, ns, s0, s1, s2, s3);
        }
        float xi = 0.f;
        if (mode != DP_CSR_SAMPLE_SELF_NONE) xi = x[(long)i * ldx + f];
        if (addself) s0 += xi;
        if (f0 + lane < F) {
            y[r * ldy + yoff + f] = ((s0 + s1) + (s2 + s3)) * scale;
            if (mode == DP_CSR_SAMPLE_SELF_CONCAT) y[r * ldy + f] = xi;
        }
    }
}

__global__ __launch_bounds__(SM_THREADS) void k_csr_sample_mean_bwd(const float* __restrict__ dy, int lddy,
                                                                    const int* __restrict__ indptr_t,
                                                                    const int* __restrict__ indices_t,
                                                                    const int* __restrict__ slot,
                                                                    const u64* __restrict__ thr,
                                                                    const int* __restrict__ cnt, float* __restrict__ dx,
                                                                    int lddx, int n, int F, int mode, unsigned k0,
                                                                    unsigned k1) {
    const long j = (long)blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= n) return;                                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int beg = indptr_t[j], end = indptr_t[j + 1];
    const int sj = slot ? slot[j] : (int)j;                   // the column's own target row, or -1
    const int nboff = mode == DP_CSR_SAMPLE_SELF_CONCAT ? F : 0;
    for (int fg = 0; fg < F; fg += SM_BWD_COLS) {
        const int nu = min(4, (F - fg + 63) >> 6);            // 64-column groups of this pass, wave-uniform
        int f[4];
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = min(fg + u * 64 + lane, F - 1), acc[u] = 0.f;
        bool selfin = false;
        for (int e0 = beg; e0 < end; e0 += 64) {
            const bool valid = e0 + lane < end;
            const int i = valid ? indices_t[e0 + lane] : 0;
            const int s = valid ? (slot ? slot[i] : i) : -1;
            int c = 1;
            bool mem = false;
            if (s >= 0) {
                const u64 t = thr[s];
                c = cnt[s];
                mem = t == SM_ALL ? true : sm_key(k0, k1, i, (int)j) <= t;
            }
            u64 bl = __ballot(mem);
            if (mode == DP_CSR_SAMPLE_SELF_GCN) selfin = selfin || __ballot(mem && i == (int)j) != 0ull;
            const int cbits = __float_as_int((float)c);
            while (bl) {                                      // members in ascending source order, four rows in flight
                long sr[4];
                float cf[4], v[4][4];
                int m = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int src = bl ? __ffsll((long long)bl) - 1 : 0;
                    if (bl) ++m;
                    bl &= bl - 1ull;                          // 0 stays 0
                    sr[q] = __builtin_amdgcn_readlane(s, src);
                    cf[q] = __int_as_float(__builtin_amdgcn_readlane(cbits, src));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[q][u] = (q < m && u < nu) ? dy[sr[q] * lddy + nboff + f[u]] : 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < m) {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u < nu) acc[u] += v[q][u] / cf[q];
                    }
            }
        }
        const bool self_term = sj >= 0 && (mode == DP_CSR_SAMPLE_SELF_CONCAT || (mode == DP_CSR_SAMPLE_SELF_GCN && !selfin));
        if (self_term) {                                      // wave-uniform
            const float cj = mode == DP_CSR_SAMPLE_SELF_GCN ? (float)cnt[sj] : 1.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < nu) {
                    const float g = dy[(long)sj * lddy + f[u]];
                    acc[u] += mode == DP_CSR_SAMPLE_SELF_GCN ? g / cj : g;
                }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < nu && fg + u * 64 + lane < F) dx[j * lddx + f[u]] = acc[u];
    }
}

// the checks the three entries share
int sample_shape(int k, int self_mode) {
    DP_CHECK(k == DP_CSR_SAMPLE_ALL || (k >= 1 && k <= DP_CSR_SAMPLE_MAX_K), DP_ERR_INVALID_ARG,
             "k=%d must be 1 .. %d, or DP_CSR_SAMPLE_ALL (%d) for every neighbour", k, DP_CSR_SAMPLE_MAX_K,
             DP_CSR_SAMPLE_ALL);
    DP_CHECK(self_mode == DP_CSR_SAMPLE_SELF_NONE || self_mode == DP_CSR_SAMPLE_SELF_GCN ||
                 self_mode == DP_CSR_SAMPLE_SELF_CONCAT,
             DP_ERR_INVALID_ARG, "self_mode=%d must be 0 (none), 1 (gcn) or 2 (concat)", self_mode);
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

#define SM_SHAPE(k, self_mode) DP_TRY(sample_shape(k, self_mode))

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
