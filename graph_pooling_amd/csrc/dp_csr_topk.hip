// Top-k (gPool / SAGPool) pooling on the CSR of a CsrGraph / CsrBatch: keep the k_b best-scored nodes of
// every graph, gate their features, and hand back the induced subgraph A[perm][:, perm] as CSR, built on the device.
//
//     key_i = (ord(score_i) << 32) | (0xffffffff - local_i),   ord: the monotone map of the fp32 bits, -0.0 made +0.0
//             first (a positive NaN above +inf, a negative NaN below -inf: every bit pattern has a place)
//     thr_b = the k_b-th largest key of graph b (0 when k_b == n_b: nothing is selected, everything is kept)
//     kept  = { i : key_i >= thr_b }: exactly k_b nodes (the keys of a graph are distinct), numbered in ASCENDING old id
//     new_id[i] = the new global row of a kept node, -1 of a dropped one;   perm[new_id[i]] = i
//     indptr' / indices' / indices_local' / edge_map: the entries (i, j) with both ends kept, in the order they are stored
//     y_r = x[perm[r]] * gate[perm[r]];   dx_i = dy[new_id[i]] * gate_i,  dgate_i = sum_f dy[new_id[i], f] x[i, f]  (0 dropped)
//
// Select + renumber (one launch, one workgroup per graph, no hand-off between workgroups): a radix select of the 64-bit
// keys from the top byte down with a 256-bin LDS histogram per pass.  The low word of a key is 0xffffffff - local with
// local < n_b, so its bytes above ceil(bits(n_b - 1) / 8) are 0xff for every key and their passes are skipped:
// 4 + ceil(bits(n_b - 1) / 8) passes.  The workgroup has 64 * ceil(max_n / 256) threads (64 .. 1024); a graph of at
// most TK_KREG = 4 keys per thread keeps them in registers (tier 1), a larger one recomputes them from `score` on every
// pass (tier 2), k_b == n_b takes no select (tier 0).  Then one prefix count of key >= thr over the graph's rows in
// ascending id (ballots, the waves' totals through LDS) writes new_id and perm.
//
// Induced CSR (three launches, once more for a transposed CSR of its own), 8 lanes per kept row, 32 rows per workgroup:
// count the kept entries of the workgroup's rows into one sum per workgroup; one workgroup scans the sums; the third
// launch recounts its rows, offsets them from its own base and fills the arrays, a row's entries in stored order (a
// ballot per 8 entries).  No workgroup waits for another: the launches are the hand-off.
//
// Every index written is in range by construction, and the writes are guarded on top of that: a position in perm below
// k_b, a position in the output arrays below their capacity, an id read through perm / new_id / indices inside its
// array.  No atomics on memory (the LDS histogram counts integers), plain vector stores; a second run gives the same bits.
#include "dp_entry.h"

namespace dp {
namespace {

typedef unsigned long long u64;

constexpr int TK_MAX_THREADS = 1024;                          // the select workgroup at its largest
constexpr int TK_KREG = 4;                                    // keys a thread of the select holds in registers
constexpr int TK_ROW_LANES = 8;                               // lanes per kept row of the induce launches
constexpr int TK_ROW_THREADS = 256;
constexpr int TK_ROWS_PER_WG = TK_ROW_THREADS / TK_ROW_LANES; // 32
constexpr int TK_SCAN_THREADS = 1024;
constexpr int TK_GATHER_THREADS = 256;                        // four waves, one row each

__host__ __device__ inline unsigned tk_ord(unsigned bits) {
    if (bits == 0x80000000u) bits = 0u;                       // -0.0 ties with +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__host__ __device__ inline u64 tk_key(unsigned bits, int local) {
    return ((u64)tk_ord(bits) << 32) | (u64)(0xffffffffu - (unsigned)local);
}

// the plan: one rule each, for the launchers, the kernels and dp_csr_topk_plan
inline int tk_threads(int max_n) {
    const int t = 64 * cdiv(max_n, 64 * TK_KREG);
    return t < 64 ? 64 : (t > TK_MAX_THREADS ? TK_MAX_THREADS : t);
}
__host__ __device__ inline int tk_tier(int n_b, int k_b, int threads) {
    return k_b >= n_b ? 0 : (n_b <= threads * TK_KREG ? 1 : 2);
}
__host__ __device__ inline int tk_low_bytes(int n_b) {       // bytes of the key's low word that differ between keys
    int bits = 0;
    for (unsigned v = (unsigned)(n_b - 1); v; v >>= 1) ++bits;
    return (bits + 7) >> 3;
}
inline size_t tk_ws_bytes(int n_out) { return (((size_t)cdiv(n_out, TK_ROWS_PER_WG) + 1) * sizeof(int) + 15) & ~size_t(15); }

// ------------------------------------------------------------------------------------------------ select + renumber
__global__ __launch_bounds__(TK_MAX_THREADS) void k_csr_topk_select(const float* __restrict__ score,
                                                                    const int* __restrict__ node_off,
                                                                    const int* __restrict__ new_off,
                                                                    int* __restrict__ new_id, int* __restrict__ perm,
                                                                    u64* __restrict__ thr_out) {
    __shared__ int hist[256];
    __shared__ int wsum[TK_MAX_THREADS / 64];
    __shared__ int sel[2];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    const int g0 = node_off[b], nb = node_off[b + 1] - g0, o0 = new_off[b], kb = new_off[b + 1] - o0;
    const unsigned* sbits = reinterpret_cast<const unsigned*>(score) + g0;
    const int tier = tk_tier(nb, kb, T);                      // workgroup-uniform, as everything up to the prefix count
    u64 thr = 0ull;
    if (tier != 0) {
        u64 kr[TK_KREG];
#pragma unroll
        for (int c = 0; c < TK_KREG; ++c) {
            const int i = c * T + tid;
            kr[c] = (tier == 1 && i < nb) ? tk_key(sbits[i], i) : 0ull;
        }
        const int low = tk_low_bytes(nb);
        u64 prefix = 0ull, mask = 0ull;
        int kk = kb;                                          // the kk-th largest of the keys on the prefix
        for (int pass = 0; pass < 4 + low; ++pass) {
            if (pass == 4 && low < 4) {                       // the low word's constant bytes: all ones
                const u64 ones = (u64)(0xffffffffu << (8 * low));
                prefix |= ones;
                mask |= ones;
            }
            const int shift = pass < 4 ? 56 - 8 * pass : 8 * (low - 1 - (pass - 4));
            for (int i = tid; i < 256; i += T) hist[i] = 0;
            __syncthreads();
            if (tier == 1) {
#pragma unroll
                for (int c = 0; c < TK_KREG; ++c)
                    if (c * T + tid < nb && (kr[c] & mask) == prefix) atomicAdd(&hist[(int)(kr[c] >> shift) & 255], 1);
            } else {
                for (int i = tid; i < nb; i += T) {
                    const u64 key = tk_key(sbits[i], i);
                    if ((key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
                }
            }
            __syncthreads();
            if (wave == 0) {                                  // the digit that holds the kk-th largest: bins from the top
                const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
                int S = (h0 + h1) + (h2 + h3);                // -> the sum over the lanes from this one up
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int v = __shfl_down(S, d, 64);
                    if (lane + d < 64) S += v;
                }
                const u64 bal = __ballot(S >= kk);            // never empty: lane 0 holds every candidate, kk of them at least
                const int L = bal ? 63 - __clzll((long long)bal) : 0;
                const int above = __shfl(S, L < 63 ? L + 1 : 63, 64);
                int rem = kk - (L < 63 ? above : 0);
                const int a1 = __shfl(h1, L, 64), a2 = __shfl(h2, L, 64), a3 = __shfl(h3, L, 64);
                int q = 3;                                    // lane L's four bins from the top; bin 0 takes what is left
                if (rem > a3) { rem -= a3; q = 2;
                    if (rem > a2) { rem -= a2; q = 1;
                        if (rem > a1) { rem -= a1; q = 0; } } }
                if (lane == 0) {
                    sel[0] = 4 * L + q;
                    sel[1] = rem;
                }
            }
            __syncthreads();
            prefix |= (u64)(unsigned)sel[0] << shift;
            mask |= 0xffull << shift;
            kk = sel[1];
        }
        thr = prefix;                                         // all 64 bits decided: the k_b-th largest key itself
    }
    // prefix count of key >= thr in ascending id
    int running = 0;
    for (int base = 0; base < nb; base += T) {
        const int i = base + tid;
        const bool keep = i < nb && (tier == 0 || tk_key(sbits[i], i) >= thr);
        const u64 bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = running, tot = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = wsum[w];
            off += w < wave ? c : 0;
            tot += c;
        }
        const int pos = off + before;
        if (i < nb) {
            const bool ok = keep && pos < kb;                 // pos < kb holds by the select; the guard keeps perm in bounds
            new_id[g0 + i] = ok ? o0 + pos : -1;
            if (ok) perm[o0 + pos] = g0 + i;
        }
        running += tot;
        __syncthreads();
    }
    if (tid == 0) thr_out[b] = thr;
}

// ------------------------------------------------------------------------------------------------ induced CSR
// the stored entries of old row perm[r] that lead to a kept node, counted by the row's 8 lanes (every lane gets the sum)
__device__ __forceinline__ int tk_row_count(const int* __restrict__ indptr, const int* __restrict__ indices,
                                            const int* __restrict__ new_id, const int* __restrict__ perm, int r, int sub,
                                            int n, int n_out, int& beg, int& dlen) {
    beg = 0;
    dlen = 0;
    int cnt = 0;
    if (r < n_out) {
        const int i = perm[r];
        if ((unsigned)i < (unsigned)n) {
            beg = indptr[i];
            dlen = indptr[i + 1] - beg;
            for (int e = sub; e < dlen; e += TK_ROW_LANES) {
                const int j = indices[beg + e];
                cnt += ((unsigned)j < (unsigned)n && new_id[j] >= 0) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int d = 1; d < TK_ROW_LANES; d <<= 1) cnt += __shfl_xor(cnt, d, 64);
    return cnt;
}

__global__ __launch_bounds__(TK_ROW_THREADS) void k_csr_topk_count(const int* __restrict__ indptr,
                                                                   const int* __restrict__ indices,
                                                                   const int* __restrict__ new_id,
                                                                   const int* __restrict__ perm, int* __restrict__ bsum,
                                                                   int n, int n_out) {
    __shared__ int wtot[TK_ROW_THREADS / 64];
    const int tid = threadIdx.x, sub = tid & (TK_ROW_LANES - 1), grp = tid / TK_ROW_LANES;
    int beg, dlen;
    int c = tk_row_count(indptr, indices, new_id, perm, blockIdx.x * TK_ROWS_PER_WG + grp, sub, n, n_out, beg, dlen);
#pragma unroll
    for (int d = TK_ROW_LANES; d < 64; d <<= 1) c += __shfl_xor(c, d, 64);      // the wave's eight rows
    if ((tid & 63) == 0) wtot[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) bsum[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// one workgroup: bsum[0 .. nblk) -> its exclusive prefix sums in place, the total into bsum[nblk] and indptr_out[n_out];
// a pooled graph without entries gets the containers' one-element pad (zeros) when the arrays have room for it
__global__ __launch_bounds__(TK_SCAN_THREADS) void k_csr_topk_scan(int* __restrict__ bsum, int nblk,
                                                                   int* __restrict__ indptr_out, int n_out,
                                                                   int* __restrict__ indices_out,
                                                                   int* __restrict__ local_out, int* __restrict__ edge_map,
                                                                   int cap) {
    __shared__ int wtot[TK_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += TK_SCAN_THREADS) {
        const int i = base + tid;
        const int v = i < nblk ? bsum[i] : 0;
        int s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d, 64);
            if (lane >= d) s += t;
        }
        if (lane == 63) wtot[wave] = s;
        __syncthreads();
        int off = carry, tot = 0;
        for (int w = 0; w < TK_SCAN_THREADS / 64; ++w) {
            const int c = wtot[w];
            off += w < wave ? c : 0;
            tot += c;
        }
        if (i < nblk) bsum[i] = off + s - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        bsum[nblk] = carry;
        indptr_out[n_out] = carry;
        if (carry == 0 && cap >= 1) {
            indices_out[0] = 0;
            edge_map[0] = 0;
            if (local_out) local_out[0] = 0;
        }
    }
}

__global__ __launch_bounds__(TK_ROW_THREADS) void k_csr_topk_fill(const int* __restrict__ indptr,
                                                                  const int* __restrict__ indices,
                                                                  const int* __restrict__ new_id,
                                                                  const int* __restrict__ perm,
                                                                  const int* __restrict__ new_off,
                                                                  const int* __restrict__ bsum,
                                                                  int* __restrict__ indptr_out,
                                                                  int* __restrict__ indices_out,
                                                                  int* __restrict__ local_out, int* __restrict__ edge_map,
                                                                  int n, int n_out, int B, int cap) {
    __shared__ int rcnt[TK_ROWS_PER_WG];
    const int tid = threadIdx.x, lane = tid & 63, sub = tid & (TK_ROW_LANES - 1), grp = tid / TK_ROW_LANES;
    const int r = blockIdx.x * TK_ROWS_PER_WG + grp;
    int beg, dlen;
    const int c = tk_row_count(indptr, indices, new_id, perm, r, sub, n, n_out, beg, dlen);
    if (sub == 0) rcnt[grp] = c;
    __syncthreads();
    int rowoff = bsum[blockIdx.x];
    for (int g = 0; g < grp; ++g) rowoff += rcnt[g];
    int o0 = 0;
    if (local_out && r < n_out) {                             // the row's graph: the last b with new_off[b] <= r
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (new_off[mid] <= r) lo = mid; else hi = mid;
        }
        o0 = new_off[lo];
    }
    int dmax = dlen;                                          // the longest of the wave's eight rows: a wave-uniform loop
#pragma unroll
    for (int d = TK_ROW_LANES; d < 64; d <<= 1) dmax = max(dmax, __shfl_xor(dmax, d, 64));
    int written = 0;
    for (int e0 = 0; e0 < dmax; e0 += TK_ROW_LANES) {
        const int e = e0 + sub;
        int nj = -1;
        if (e < dlen) {
            const int j = indices[beg + e];
            if ((unsigned)j < (unsigned)n) nj = new_id[j];
        }
        const bool keep = nj >= 0;
        const u64 bal = __ballot(keep);
        const unsigned mine = (unsigned)(bal >> (lane & 56)) & 0xffu;      // the ballot of this row's eight lanes
        const int p = rowoff + written + __popc(mine & ((1u << sub) - 1u));
        if (keep && p < cap) {                                // p < cap holds (cap >= the input's nnz); the guard is free
            indices_out[p] = nj;
            if (local_out) local_out[p] = nj - o0;
            edge_map[p] = beg + e;
        }
        written += __popc(mine);
    }
    if (sub == 0 && r < n_out) indptr_out[r] = rowoff;
}

// ------------------------------------------------------------------------------------------------ gather * gate
__global__ __launch_bounds__(TK_GATHER_THREADS) void k_csr_topk_gather_fwd(const float* __restrict__ x, int ldx,
                                                                           const float* __restrict__ gate,
                                                                           const int* __restrict__ perm,
                                                                           float* __restrict__ y, int ldy, int n,
                                                                           int n_out, int F) {
    const long r = (long)blockIdx.x * (TK_GATHER_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_out) return;                                   // wave-uniform
    const int lane = threadIdx.x & 63;
    const int i = perm[r];
    const bool ok = (unsigned)i < (unsigned)n;
    const float g = (ok && gate) ? gate[i] : 1.f;
    for (int f = lane; f < F; f += 64) {
        float v = 0.f;
        if (ok) {
            v = x[(long)i * ldx + f];
            if (gate) v = v * g;
        }
        y[r * ldy + f] = v;
    }
}

__global__ __launch_bounds__(TK_GATHER_THREADS) void k_csr_topk_gather_bwd(const float* __restrict__ dy, int lddy,
                                                                           const float* __restrict__ x, int ldx,
                                                                           const float* __restrict__ gate,
                                                                           const int* __restrict__ new_id,
                                                                           float* __restrict__ dx, int lddx,
                                                                           float* __restrict__ dgate, int n, int n_out,
                                                                           int F) {
    const long i = (long)blockIdx.x * (TK_GATHER_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int r = new_id[i];
    const bool kept = (unsigned)r < (unsigned)n_out;          // wave-uniform
    const float g = (kept && gate) ? gate[i] : 1.f;
    float acc = 0.f;                                          // the lane's columns f = lane, lane + 64, ..: one fma chain
    for (int f = lane; f < F; f += 64) {
        float d = 0.f;
        if (kept) {
            d = dy[(long)r * lddy + f];
            if (dgate) acc = fmaf(d, x[i * ldx + f], acc);
            if (gate) d = d * g;
        }
        dx[i * lddx + f] = d;
    }
    if (dgate) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);    // a butterfly: every lane the same six additions
        if (lane == 0) dgate[i] = kept ? acc : 0.f;
    }
}

// host tables of a select: node_off_host [B + 1] from 0 to n, kb_host [B] in 1 .. n_b, summing to n_out
int topk_tables(const int* node_off_host, const int* kb_host, int n, int n_out, int B, int* max_n) {
    DP_CHECK(node_off_host[0] == 0 && node_off_host[B] == n, DP_ERR_INVALID_ARG,
             "node_off_host must run from 0 to n=%d, got %d .. %d", n, node_off_host[0], node_off_host[B]);
    long sum = 0;
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        const int nb = node_off_host[b + 1] - node_off_host[b];
        DP_CHECK(nb >= 1, DP_ERR_INVALID_ARG, "graph %d has %d nodes: every graph needs at least one", b, nb);
        DP_CHECK(kb_host[b] >= 1 && kb_host[b] <= nb, DP_ERR_INVALID_ARG, "k_b=%d of graph %d must be 1 .. n_b=%d",
                 kb_host[b], b, nb);
        sum += kb_host[b];
        mx = nb > mx ? nb : mx;
    }
    DP_CHECK(sum == n_out, DP_ERR_INVALID_ARG, "the k_b sum to %ld, n_out=%d", sum, n_out);
    *max_n = mx;
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_csr_topk_plan(int n, int n_out, int B, int max_n, int n_b, int k_b, int F, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n);
    DP_NONNEG(n_out);
    DP_NONNEG(B);
    DP_NONNEG(max_n);
    DP_NONNEG(F);
    DP_CHECK(n_b >= 1 && n_b <= (max_n > 0 ? max_n : 1), DP_ERR_INVALID_ARG, "n_b=%d must be 1 .. max_n=%d", n_b, max_n);
    DP_CHECK(k_b >= 1 && k_b <= n_b, DP_ERR_INVALID_ARG, "k_b=%d must be 1 .. n_b=%d", k_b, n_b);
    DP_CHECK(n_out <= n, DP_ERR_INVALID_ARG, "n_out=%d exceeds n=%d", n_out, n);
    const int T = tk_threads(max_n), tier = tk_tier(n_b, k_b, T), nblk = cdiv(n_out, TK_ROWS_PER_WG);
    const int plan[DP_CSR_TOPK_PLAN_INTS] = {T,
                                             tier,
                                             tier ? cdiv(n_b, T) : 0,
                                             tier ? 4 + tk_low_bytes(n_b) : 0,
                                             cdiv(n_b, T),
                                             B,
                                             nblk,
                                             cdiv(nblk, TK_SCAN_THREADS),
                                             cdiv(n_out, TK_GATHER_THREADS / 64),
                                             cdiv(n, TK_GATHER_THREADS / 64)};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

size_t dp_csr_topk_workspace_bytes(int n_out) { return tk_ws_bytes(n_out < 0 ? 0 : n_out); }

int dp_csr_topk_select(const float* score, const int* node_off, const int* new_off, const int* node_off_host,
                       const int* kb_host, int* new_id, int* perm, unsigned long long* thr, int n, int n_out, int B,
                       void* stream) {
    DP_PTR(score); DP_PTR(node_off); DP_PTR(new_off); DP_PTR(new_id); DP_PTR(perm); DP_PTR(thr);
    DP_NOTNULL(node_off_host);
    DP_NOTNULL(kb_host);
    DP_ALIGNED8(thr);
    DP_NONNEG(n);
    DP_NONNEG(n_out);
    DP_NONNEG(B);
    if (n == 0 && B == 0 && n_out == 0) return DP_OK;
    DP_CHECK(B >= 1, DP_ERR_INVALID_ARG, "B=%d: %d nodes need at least one graph", B, n);
    int max_n = 0;
    DP_TRY(topk_tables(node_off_host, kb_host, n, n_out, B, &max_n));
    Seq q(DP_STREAM(stream), nullptr, 0);
    hipLaunchKernelGGL(k_csr_topk_select, dim3(B), dim3(tk_threads(max_n)), 0, q.stream, score, node_off, new_off, new_id,
                       perm, thr);
    q.check_launch("k_csr_topk_select");
    return q.err;
}

int dp_csr_topk_induce(const int* indptr, const int* indices, const int* new_id, const int* perm, const int* new_off,
                       int* indptr_out, int* indices_out, int* indices_local_out, int* edge_map, int n, int n_out, int B,
                       int nnz, int cap, void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(indptr); DP_PTR(indices); DP_PTR(new_id); DP_PTR(perm); DP_PTR(indptr_out); DP_PTR(indices_out);
    DP_PTR(edge_map);
    if (indices_local_out) {
        DP_ALIGNED4(indices_local_out);
        DP_PTR(new_off);
    }
    DP_NONNEG(n);
    DP_NONNEG(n_out);
    DP_NONNEG(B);
    DP_NONNEG(nnz);
    DP_CHECK(n_out <= n, DP_ERR_INVALID_ARG, "n_out=%d exceeds n=%d", n_out, n);
    DP_CHECK(cap >= nnz, DP_ERR_INVALID_ARG, "cap=%d is below the input's nnz=%d", cap, nnz);
    DP_CHECK(!indices_local_out || B >= 1 || n_out == 0, DP_ERR_INVALID_ARG, "B=%d: indices_local_out needs the graphs", B);
    DP_ALIGNED16(workspace, false, "workspace must be there and 16-byte aligned");
    DP_CHECK(workspace_bytes >= tk_ws_bytes(n_out), DP_ERR_WORKSPACE, "workspace too small: need >= %zu bytes, have %zu",
             tk_ws_bytes(n_out), workspace_bytes);
    Seq q(DP_STREAM(stream), nullptr, 0);
    int* bsum = (int*)workspace;
    const int nblk = cdiv(n_out, TK_ROWS_PER_WG);
    if (nblk) {
        hipLaunchKernelGGL(k_csr_topk_count, dim3(nblk), dim3(TK_ROW_THREADS), 0, q.stream, indptr, indices, new_id, perm,
                           bsum, n, n_out);
        q.check_launch("k_csr_topk_count");
    }
    hipLaunchKernelGGL(k_csr_topk_scan, dim3(1), dim3(TK_SCAN_THREADS), 0, q.stream, bsum, nblk, indptr_out, n_out,
                       indices_out, indices_local_out, edge_map, cap);
    q.check_launch("k_csr_topk_scan");
    if (nblk) {
        hipLaunchKernelGGL(k_csr_topk_fill, dim3(nblk), dim3(TK_ROW_THREADS), 0, q.stream, indptr, indices, new_id, perm,
                           new_off, bsum, indptr_out, indices_out, indices_local_out, edge_map, n, n_out, B, cap);
        q.check_launch("k_csr_topk_fill");
    }
    return q.err;
}

int dp_csr_topk_gather_fwd(const float* x, int ldx, const float* gate, const int* perm, float* y, int ldy, int n, int n_out,
                           int F, void* stream) {
    DP_PTR(x); DP_PTR(perm); DP_PTR(y);
    if (gate) DP_ALIGNED4(gate);
    DP_NONNEG(n);
    DP_NONNEG(n_out);
    DP_NONNEG(F);
    DP_CHECK(n_out <= n, DP_ERR_INVALID_ARG, "n_out=%d exceeds n=%d", n_out, n);
    DP_LD(ldx, F);
    DP_LD(ldy, F);
    if (n_out == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    hipLaunchKernelGGL(k_csr_topk_gather_fwd, dim3(cdiv(n_out, TK_GATHER_THREADS / 64)), dim3(TK_GATHER_THREADS), 0,
                       q.stream, x, ldx, gate, perm, y, ldy, n, n_out, F);
    q.check_launch("k_csr_topk_gather_fwd");
    return q.err;
}

int dp_csr_topk_gather_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gate, const int* new_id,
                           float* dx, int lddx, float* dgate, int n, int n_out, int F, void* stream) {
    DP_PTR(dy); DP_PTR(new_id); DP_PTR(dx);
    if (gate) DP_ALIGNED4(gate);
    if (dgate) {
        DP_ALIGNED4(dgate);
        DP_CHECK(gate != nullptr, DP_ERR_INVALID_ARG, "dgate without gate");
        DP_PTR(x);
    }
    if (x) DP_ALIGNED4(x);
    DP_NONNEG(n);
    DP_NONNEG(n_out);
    DP_NONNEG(F);
    DP_CHECK(n_out <= n, DP_ERR_INVALID_ARG, "n_out=%d exceeds n=%d", n_out, n);
    DP_LD(lddy, F);
    DP_LD(lddx, F);
    if (dgate) DP_LD(ldx, F);
    if (n == 0 || F == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    hipLaunchKernelGGL(k_csr_topk_gather_bwd, dim3(cdiv(n, TK_GATHER_THREADS / 64)), dim3(TK_GATHER_THREADS), 0, q.stream,
                       dy, lddy, x, ldx, gate, new_id, dx, lddx, dgate, n, n_out, F);
    q.check_launch("k_csr_topk_gather_bwd");
    return q.err;
}

}  // extern "C"
