// The device code that dp_csr_sample.hip and dp_csr_block.hip share: Philox and the key,
// the tier rule, the radix select of a row's k-th smallest key, the pull compaction of the selected ids, the gather loop
// and the backward's membership walk.  Both units instantiate ONE body each for the forward and the backward,
// sm_fwd_body<BLOCK> / sm_bwd_body<BLOCK>:
//   BLOCK = false  the whole-graph form: x and dx are [n, F], an id is the row it names.
//   BLOCK = true   the compact form of a sampled block: x_src and dx_src are [n_src, F], every gathered id (the self row
//                  included) goes through slot[] first.  Every index that was built on the device is compared before it
//                  is used: a target id and a stored id against n before slot[] is read, a slot against n_src before
//                  x_src is read through it (out of range: the term is 0, never a fault), src[s] against n.
// The selection, the compaction and the order of every sum are the same statements in both forms, so the compact form
// gives the bits of the whole-graph form on the rows it holds.  sm_select is also what the block's mark launch runs.
#pragma once
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

// slot[j] of a stored or target id j, -1 for an id outside 0 .. n - 1 (BLOCK only)
__device__ __forceinline__ int sm_slot_of(const int* __restrict__ slot, int j, int n) {
    return (unsigned)j < (unsigned)n ? slot[j] : -1;
}

// x[row, f]; BLOCK: a row outside 0 .. n_rows - 1 reads as 0 (row wave-uniform: a scalar branch)
template <bool BLOCK>
__device__ __forceinline__ float sm_load(const float* __restrict__ x, long row, int ldx, int f, int n_rows) {
    if (BLOCK) return (unsigned long)row < (unsigned long)n_rows ? x[row * ldx + f] : 0.f;
    return x[row * ldx + f];
}

// cnt ids of `mine` (lane q holds id q), handed round by readlane: the inner loop of dp_meanagg.hip
template <bool BLOCK>
__device__ __forceinline__ void sm_gather(const float* __restrict__ x, int ldx, int f, int mine, int cnt, int n_x,
                                          float& s0, float& s1, float& s2, float& s3) {
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {
        const long r0 = __builtin_amdgcn_readlane(mine, j), r1 = __builtin_amdgcn_readlane(mine, j + 1);
        const long r2 = __builtin_amdgcn_readlane(mine, j + 2), r3 = __builtin_amdgcn_readlane(mine, j + 3);
        const float v0 = sm_load<BLOCK>(x, r0, ldx, f, n_x), v1 = sm_load<BLOCK>(x, r1, ldx, f, n_x);
        const float v2 = sm_load<BLOCK>(x, r2, ldx, f, n_x), v3 = sm_load<BLOCK>(x, r3, ldx, f, n_x);
        s0 += v0; s1 += v1; s2 += v2; s3 += v3;
    }
    for (; j < cnt; ++j) s0 += sm_load<BLOCK>(x, (long)__builtin_amdgcn_readlane(mine, j), ldx, f, n_x);
}

// What the selection of one target row leaves in the wave: the row's extent, whether every stored id is taken, the
// threshold, the number of selected ids, lane q's id (q < ns, ascending; tiers B and C only) and, under gcn, whether the
// node's own stored loop is among them.
struct SmRow {
    int beg, end;
    bool all;
    u64 thr;
    int ns, mine;
    bool selfin;
};

// The selection of node i's row, ONCE per row (every value wave-uniform but `mine`).  BLOCK: i outside 0 .. n - 1 is an
// empty row.
template <bool BLOCK>
__device__ __forceinline__ SmRow sm_select(const int* __restrict__ indptr, const int* __restrict__ indices, int i, int n,
                                           int k, int mode, unsigned k0, unsigned k1, int lane) {
    SmRow R;
    if (BLOCK) {
        const bool iok = (unsigned)i < (unsigned)n;
        R.beg = iok ? indptr[i] : 0;
        R.end = iok ? indptr[i + 1] : 0;
    } else {
        R.beg = indptr[i];
        R.end = indptr[i + 1];
    }
    const int beg = R.beg, end = R.end, d = end - beg;
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
    R.all = all;
    R.thr = thr;
    R.ns = ns;
    R.mine = mine;
    R.selfin = selfin;
    return R;
}

// The forward of one target row per wavefront.  BLOCK = false: x [n, F], slot / n_x / n unused.  BLOCK = true:
// x [n_x, F] holds the rows of the block's src, slot [n] maps a node id to its row.
template <bool BLOCK>
__device__ __forceinline__ void sm_fwd_body(const float* __restrict__ x, int ldx, const int* __restrict__ indptr,
                                            const int* __restrict__ indices, const int* __restrict__ nodes,
                                            const int* __restrict__ slot, int n_x, float* __restrict__ y, int ldy,
                                            u64* __restrict__ thr_out, int* __restrict__ cnt_out, int n_rows, int n,
                                            int F, int k, int mode, unsigned k0, unsigned k1) {
    const long r = (long)blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int i = nodes ? nodes[r] : (int)r;
    const SmRow R = sm_select<BLOCK>(indptr, indices, i, n, k, mode, k0, k1, lane);
    const int beg = R.beg, end = R.end, ns = R.ns;
    const bool all = R.all;
    int mine = R.mine;
    long self_row = i;                                        // the row of x that holds x_i
    if (BLOCK) {
        self_row = sm_slot_of(slot, i, n);
        if (!all) mine = lane < ns ? sm_slot_of(slot, mine, n) : -1;
    }
    const bool addself = mode == DP_CSR_SAMPLE_SELF_GCN && !R.selfin;
    const int cnt_i = ns + (addself ? 1 : 0);
    if (lane == 0) {
        thr_out[r] = R.thr;
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
                int id = indices[e0 + min(lane, cnt - 1)];
                if (BLOCK) id = sm_slot_of(slot, id, n);
                sm_gather<BLOCK>(x, ldx, f, id, cnt, n_x, s0, s1, s2, s3);
            }
        } else {
            sm_gather<BLOCK>(x, ldx, f, mine, ns, n_x, s0, s1, s2, s3);
        }
        float xi = 0.f;
        if (mode != DP_CSR_SAMPLE_SELF_NONE) xi = sm_load<BLOCK>(x, self_row, ldx, f, n_x);
        if (addself) s0 += xi;
        if (f0 + lane < F) {
            y[r * ldy + yoff + f] = ((s0 + s1) + (s2 + s3)) * scale;
            if (mode == DP_CSR_SAMPLE_SELF_CONCAT) y[r * ldy + f] = xi;
        }
    }
}

// The backward of one output row per wavefront.  BLOCK = false: row j of dx [n, F] is node j.  BLOCK = true: row s of
// dx [n_out, F] is node j = src[s]; slot is then the TARGETS' slot (or NULL: every node its own target row).
template <bool BLOCK>
__device__ __forceinline__ void sm_bwd_body(const float* __restrict__ dy, int lddy, const int* __restrict__ indptr_t,
                                            const int* __restrict__ indices_t, const int* __restrict__ slot,
                                            const int* __restrict__ src, int n_out, const u64* __restrict__ thr,
                                            const int* __restrict__ cnt, float* __restrict__ dx, int lddx, int n, int F,
                                            int mode, unsigned k0, unsigned k1) {
    const long row = (long)blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= (BLOCK ? n_out : n)) return;                   // wave-uniform
    const int lane = threadIdx.x & 63;
    long j = row;
    bool jok = true;
    if (BLOCK) {
        j = src[row];
        jok = (unsigned long)j < (unsigned long)n;
    }
    const int beg = jok ? indptr_t[j] : 0, end = jok ? indptr_t[j + 1] : 0;
    const int sj = jok ? (slot ? slot[j] : (int)j) : -1;      // the column's own target row, or -1
    const int nboff = mode == DP_CSR_SAMPLE_SELF_CONCAT ? F : 0;
    for (int fg = 0; fg < F; fg += SM_BWD_COLS) {
        const int nu = min(4, (F - fg + 63) >> 6);            // 64-column groups of this pass, wave-uniform
        int f[4];
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = min(fg + u * 64 + lane, F - 1), acc[u] = 0.f;
        bool selfin = false;
        for (int e0 = beg; e0 < end; e0 += 64) {
            bool valid = e0 + lane < end;
            const int i = valid ? indices_t[e0 + lane] : 0;
            if (BLOCK) valid = valid && (unsigned)i < (unsigned)n;
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
                    const int from = bl ? __ffsll((long long)bl) - 1 : 0;
                    if (bl) ++m;
                    bl &= bl - 1ull;                          // 0 stays 0
                    sr[q] = __builtin_amdgcn_readlane(s, from);
                    cf[q] = __int_as_float(__builtin_amdgcn_readlane(cbits, from));
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
            if (u < nu && fg + u * 64 + lane < F) dx[row * lddx + f[u]] = acc[u];
    }
}

// the checks the sampling entries of both units share
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

#define SM_SHAPE(k, self_mode) DP_TRY(::dp::sample_shape(k, self_mode))
