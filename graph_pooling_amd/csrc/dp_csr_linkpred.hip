// Link-prediction loss of DiffPool (SoftPoolingGcnEncoder.loss, encoders.py:1309-1331, adj_hop = 1) on ONE graph whose
// 0/1 adjacency is given as CSR (N4).  With p_ij = min(<S_i, S_j>, 1) and eps = 1e-7 the n^2 sum splits into
//     sum_ij [ -A_ij log(p_ij + eps) - (1 - A_ij) log(1 - p_ij + eps) ]
//       =  sum_ij        -log(1 - p_ij + eps)                            dense term: reads S only, symmetric in (i, j)
//       +  sum_(i,j) in E [ -log(p_ij + eps) + log(1 - p_ij + eps) ]     edge term: nnz dot products of S rows
// so no n x n adjacency is ever read or built; memory is O(n K).  loss = sum / n^2 and the backward scale dloss / n^2
// are formed in double, as k_link_final does (dp_linkpred.hip).
//
// Weighted entries (_w): the loss is linear in a_ij, so the dense term is unchanged and the edge term becomes
// a_ij [ -log(p_ij + eps) + log(1 - p_ij + eps) ] with values[e .. e+3] loaded next to indices[e .. e+3]; its backward
// coefficient scales likewise.  Weights of exactly 1.0 give the unweighted bits.
//
// CSR contract: 0/1 adjacency (or the stored values of the _w entries), every (i, j) listed at most once.  Self loops are allowed (their term comes from the edge
// kernels like any other edge); so are isolated nodes and empty rows.
//
// Dense forward : the P-tile walk of dp_linkpred.hip without an adjacency, over the upper triangle only (tiles with
//                 tr <= tc; off-diagonal tiles count twice).  A workgroup owns the row-block PAIR (p, T-1-p) — T+1
//                 tiles, the same for every pair — keeps the row block's S in LDS and walks every Z-th column tile
//                 (Z column splits fill the chip at small n); the next column block is fetched into registers while the
//                 current tile is computed.  Sums leave each thread as double; one double partial per workgroup.
// Dense backward: k_link_bwd's walk without either adjacency tile: recompute P, E = 2 scale g'(P),
//                 g'(p) = gate / (1 - min(p, 1) + eps), accumulate E S_c on the MFMA; column splits are combined in
//                 split order by k_csr_link_reduce.
// Edge forward  : a 16-lane team per row; neighbour ids and rows are fetched four at a time, 16-byte loads when
//                 K % 4 == 0 and the stride allows; the dot products are reduced on DPP inside the team.
// Edge backward : row-local gather in both directions, dS_i += scale [ sum_{j in N(i)} c_ij S_j + sum_{j in N^T(i)}
//                 c_ji S_j ], c = gate (-1 / (p + eps) - 1 / (1 - p + eps)); one gather and a factor 2 when the
//                 transposed CSR is the forward's.  It runs after the dense backward and adds into dS: one writer per
//                 row.
// No float atomics anywhere and every reduction has a fixed order: loss and dS are bit-reproducible run to run.
#include <algorithm>

#include "dp_entry.h"
#include "dp_link_tiles.h"

namespace dp {
namespace {

constexpr int LK_FWD_TARGET_WGS = 1024;   // dense forward: workgroups wanted (4 per CU) before column splits stop
constexpr int LK_BWD_TARGET_WGS = 512;    // dense backward: as link_bwd (dp_linkpred.hip)
constexpr int LK_TEAM_ROWS = 16;          // edge kernels: rows (16-lane teams) per 256-thread workgroup

// fixed tree over the 256 threads of the workgroup
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// ------------------------------------------------------------------ dense term
template <int KT>
__global__ __launch_bounds__(256) void k_csr_link_dense_fwd(const float* S, int lds_ld, int n, int K, int T,
                                                            double* partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[256];
    constexpr int KW = KT * 16, KP = KW + 2, NS = 64 * KW / 256;
    const int Z = gridDim.x, z = blockIdx.x, p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, kq = lane >> 4;
    float* Sr = lds;                 // [64][KP]
    float* Sc = lds + 64 * KP;       // [64][KP]
    float sc[NS];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int i = e / KW, k = e % KW;
            sc[m] = S[(long)min(c0 + i, n - 1) * lds_ld + min(k, K - 1)];     // raw: zeroed when it is written to LDS
        }
    };
    double tot = 0.0;
    for (int half = 0; half < 2; ++half) {
        const int tr = half ? T - 1 - p : p;
        if (half && tr == p) break;                   // odd T: the middle row block is its own partner
        int tc = tr + z;
        if (tc >= T) continue;
        const int r0 = tr * 64;
        __syncthreads();                              // the previous half's readers of Sr are done
        fetch(tc * 64);
        lk_stage<KT, 64>(S, lds_ld, r0, n, K, Sr);
        for (; tc < T; tc += Z) {
            const int c0 = tc * 64;
            __syncthreads();                          // previous tile's readers of Sc are done
#pragma unroll
            for (int m = 0; m < NS; ++m) {
                const int e = threadIdx.x + 256 * m;
                const int i = e / KW, k = e % KW;
                Sc[i * KP + k] = (c0 + i < n && k < K) ? sc[m] : 0.f;
            }
            __syncthreads();
            if (tc + Z < T) fetch((tc + Z) * 64);
            lk_f32x4 acc[2][2];
            lk_ptile<KT, 2>(Sr, Sc, K, wr, wc, l15, kq, acc);
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c = c0 + wc * 32 + j * 16 + l15;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + wr * 32 + i * 16 + kq * 4 + r;
                        const float pv = fminf(acc[i][j][r], 1.f);
                        const float l = -logf(1.f - pv + LINK_EPS);
                        sum += (row < n && c < n) ? l : 0.f;
                    }
                }
            tot += (double)(tc == tr ? sum : 2.f * sum);      // P is symmetric: tile (tc, tr) holds the same terms
        }
    }
    const double s = block_sum_f64(tot, red);
    if (threadIdx.x == 0) partial[(long)p * Z + z] = s;
}

// loss = sum(partials) / n^2 (one workgroup, double, fixed order); also the backward scale dloss / n^2
// (nn: n^2 of the graph, or sum_b n_b^2 of a batch)
__global__ __launch_bounds__(256) void k_csr_link_final(const double* partial, int count, double nn, float* out,
                                                        float* scale_out, const float* dloss) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        if (out) out[0] = (float)(s / nn);
        if (scale_out) scale_out[0] = (float)((dloss ? (double)dloss[0] : 1.0) / nn);
    }
}

// KT = ceil(K / 16) output column tiles per row block; the column tiles walked are CW = 32 NJ wide
template <int KT, int NJ>
__global__ __launch_bounds__(256) void k_csr_link_dense_bwd(const float* S, int lds_ld, const float* scale_ptr,
                                                            float* dS, int ldds, int n, int K, int accumulate,
                                                            float* part, int split_tiles) {
    // part != null: blockIdx.z walks only `split_tiles` column tiles and stores its partial row block to
    // part[z][row][K]; k_csr_link_reduce sums the splits in split order
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CW = 32 * NJ, KW = KT * 16, KP = KW + 2;
    constexpr int SA = CW + 4;      // E tile row stride: 4 SA = 16 mod 32, so (4 kq + r) rows x 16 cols spread over banks
    constexpr int NS = CW * KW / 256;
    const int r0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, kq = lane >> 4;
    float* Sr = lds;                 // [64][KP]
    float* Sc = Sr + 64 * KP;        // [CW][KP]
    float* Et = Sc + CW * KP;        // [64][SA]   E[i][j] = 2 scale g'(P[r0 + i][c0 + j])
    const float scale = scale_ptr[0];

    float sc[NS];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int i = e / KW, k = e % KW;
            sc[m] = S[(long)min(c0 + i, n - 1) * lds_ld + min(k, K - 1)];
        }
    };
    const int cbeg = part ? (int)blockIdx.z * split_tiles * CW : 0;
    const int cend = part ? min(n, cbeg + split_tiles * CW) : n;
    fetch(min(cbeg, n - 1));
    lk_stage<KT, 64>(S, lds_ld, r0, n, K, Sr);
    // this wave's share of the output block: rows wave*16.., all KT column tiles
    lk_f32x4 out[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) out[t] = (lk_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = cbeg; c0 < cend; c0 += CW) {
        __syncthreads();                              // previous iteration's readers of Sc / Et are done
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int i = e / KW, k = e % KW;
            Sc[i * KP + k] = (c0 + i < n && k < K) ? sc[m] : 0.f;
        }
        __syncthreads();
        if (c0 + CW < cend) fetch(c0 + CW);
        lk_f32x4 acc[2][NJ];
        lk_ptile<KT, NJ>(Sr, Sc, K, wr, wc, l15, kq, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int cj = wc * 16 * NJ + j * 16 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = wr * 32 + i * 16 + kq * 4 + r;
                    const float raw = acc[i][j][r];
                    const float g = lk_min_gate(raw) / (1.f - fminf(raw, 1.f) + LINK_EPS);
                    Et[ri * SA + cj] = (r0 + ri < n && c0 + cj < n) ? scale * (g + g) : 0.f;   // d/dP(r,c) + d/dP(c,r)
                }
            }
        __syncthreads();
        // out[16 rows of this wave][K] += E[rows][CW] · Sc[CW][K]
#pragma unroll 4
        for (int k0 = 0; k0 < CW; k0 += 4) {
            const float ev = Et[(wave * 16 + l15) * SA + k0 + kq];
#pragma unroll
            for (int t = 0; t < KT; ++t)
                out[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ev, Sc[(k0 + kq) * KP + t * 16 + l15], out[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int col = t * 16 + l15;
        if (col >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + wave * 16 + kq * 4 + r;
            if (row < n) {
                if (part) {
                    part[((long)blockIdx.z * n + row) * K + col] = out[t][r];
                } else {
                    float* q = dS + (long)row * ldds + col;
                    *q = accumulate ? *q + out[t][r] : out[t][r];
                }
            }
        }
    }
}

// dS[row, :] = (accumulate ? dS : 0) + sum_z part[z][row][:]
__global__ __launch_bounds__(256) void k_csr_link_reduce(const float* part, int splits, float* dS, int ldds, int n,
                                                         int K, int accumulate) {
    const long total = (long)n * K;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += part[(long)z * total + e];
        float* q = dS + (e / K) * ldds + e % K;
        *q = accumulate ? *q + v : v;
    }
}

// ------------------------------------------------------------------ edge term
template <int VEC> struct RowVec;
template <> struct RowVec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ float dot(T a, T b) { return a * b; }
};
template <> struct RowVec<4> {
    typedef lk_f32x4 T;
    static __device__ __forceinline__ T zero() { return (lk_f32x4){0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ float dot(T a, T b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
};

// A row of S spread over a 16-lane team: lane l15 holds columns (16 m + l15) VEC .. + VEC - 1 for m < NCH
// (NCH * 16 * VEC >= K).  Chunks past K are loaded from a clamped address; mask_row() zeroes them in ONE operand of the
// dot product, which is enough (the other operand's duplicates are finite).
template <int VEC, int NCH>
struct TeamRow {
    typename RowVec<VEC>::T v[NCH];
    __device__ __forceinline__ void load(const float* S, long lds, long row, int l15, int K) {
#pragma unroll
        for (int m = 0; m < NCH; ++m) {
            const int col = min((m * 16 + l15) * VEC, K - VEC);
            v[m] = *reinterpret_cast<const typename RowVec<VEC>::T*>(S + row * lds + col);
        }
    }
    __device__ __forceinline__ void mask(int l15, int K) {
#pragma unroll
        for (int m = 0; m < NCH; ++m)
            if ((m * 16 + l15) * VEC >= K) v[m] = RowVec<VEC>::zero();
    }
    __device__ __forceinline__ float dot(const TeamRow& o) const {     // the team's total, in all 16 lanes
        float d = 0.f;
#pragma unroll
        for (int m = 0; m < NCH; ++m) d += RowVec<VEC>::dot(v[m], o.v[m]);
        return row16_sum(d);
    }
};

__device__ __forceinline__ float edge_term(float raw) {
    const float pv = fminf(raw, 1.f);
    return -logf(pv + LINK_EPS) + logf(1.f - pv + LINK_EPS);
}
__device__ __forceinline__ float edge_coef(float raw) {
    const float pv = fminf(raw, 1.f);
    return lk_min_gate(raw) * (-1.f / (pv + LINK_EPS) - 1.f / (1.f - pv + LINK_EPS));
}

template <int VEC, int NCH, bool WT>
__device__ __forceinline__ void csr_link_edge_fwd_body(const float* S, int lds_ld, const int* indptr,
                                                       const int* indices, int n, int K, double* partial,
                                                       const float* values) {
    __shared__ double red[256];
    const int l15 = threadIdx.x & 15;
    const int row = blockIdx.x * LK_TEAM_ROWS + (threadIdx.x >> 4);
    const long lds = lds_ld;
    double tot = 0.0;
    if (row < n) {
        TeamRow<VEC, NCH> si;
        si.load(S, lds, row, l15, K);
        si.mask(l15, K);
        const int beg = indptr[row], end = indptr[row + 1];
        int e = beg;
        for (; e + 4 <= end; e += 4) {            // four neighbour rows in flight before the first dot product
            const long j0 = indices[e], j1 = indices[e + 1], j2 = indices[e + 2], j3 = indices[e + 3];
            TeamRow<VEC, NCH> a0, a1, a2, a3;
            a0.load(S, lds, j0, l15, K);
            a1.load(S, lds, j1, l15, K);
            a2.load(S, lds, j2, l15, K);
            a3.load(S, lds, j3, l15, K);
            float t0 = edge_term(si.dot(a0)), t1 = edge_term(si.dot(a1));
            float t2 = edge_term(si.dot(a2)), t3 = edge_term(si.dot(a3));
            if constexpr (WT) {
                t0 *= values[e]; t1 *= values[e + 1]; t2 *= values[e + 2]; t3 *= values[e + 3];
            }
            tot += (double)((t0 + t1) + (t2 + t3));
        }
        for (; e < end; ++e) {
            TeamRow<VEC, NCH> a0;
            a0.load(S, lds, indices[e], l15, K);
            float t0 = edge_term(si.dot(a0));
            if constexpr (WT) t0 *= values[e];
            tot += (double)t0;
        }
        if (l15 != 0) tot = 0.0;                  // every lane of the team holds the row's sum: count it once
    }
    const double s = block_sum_f64(tot, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the 0/1 kernel and the weighted one: one body, two names
template <int VEC, int NCH>
__global__ __launch_bounds__(256) void k_csr_link_edge_fwd(const float* S, int lds_ld, const int* indptr,
                                                           const int* indices, int n, int K, double* partial) {
    csr_link_edge_fwd_body<VEC, NCH, false>(S, lds_ld, indptr, indices, n, K, partial, nullptr);
}
template <int VEC, int NCH>
__global__ __launch_bounds__(256) void k_csr_link_edge_fwd_w(const float* S, int lds_ld, const int* indptr,
                                                             const int* indices, const float* values, int n, int K,
                                                             double* partial) {
    csr_link_edge_fwd_body<VEC, NCH, true>(S, lds_ld, indptr, indices, n, K, partial, values);
}

template <int VEC, int NCH, bool WT>
__device__ __forceinline__ void csr_link_edge_bwd_body(const float* S, int lds_ld, const int* indptr,
                                                       const int* indices, const int* indptr_t, const int* indices_t,
                                                       const float* scale_ptr, float* dS, int ldds, int n, int K,
                                                       int directed, const float* values, const float* values_t) {
    const int l15 = threadIdx.x & 15;
    const int row = blockIdx.x * LK_TEAM_ROWS + (threadIdx.x >> 4);
    if (row >= n) return;
    const long lds = lds_ld;
    typedef typename RowVec<VEC>::T V;
    TeamRow<VEC, NCH> si;
    si.load(S, lds, row, l15, K);
    si.mask(l15, K);
    V acc[NCH];
#pragma unroll
    for (int m = 0; m < NCH; ++m) acc[m] = RowVec<VEC>::zero();
    // p_ij = p_ji bit for bit (the same products in the same order), so both lists take c(<S_i, S_j>)
    auto walk = [&](const int* ip, const int* ix, const float* val) {
        const int beg = ip[row], end = ip[row + 1];
        int e = beg;
        for (; e + 4 <= end; e += 4) {
            const long j0 = ix[e], j1 = ix[e + 1], j2 = ix[e + 2], j3 = ix[e + 3];
            TeamRow<VEC, NCH> a0, a1, a2, a3;
            a0.load(S, lds, j0, l15, K);
            a1.load(S, lds, j1, l15, K);
            a2.load(S, lds, j2, l15, K);
            a3.load(S, lds, j3, l15, K);
            float c0 = edge_coef(si.dot(a0)), c1 = edge_coef(si.dot(a1));
            float c2 = edge_coef(si.dot(a2)), c3 = edge_coef(si.dot(a3));
            if constexpr (WT) {
                c0 *= val[e]; c1 *= val[e + 1]; c2 *= val[e + 2]; c3 *= val[e + 3];
            }
#pragma unroll
            for (int m = 0; m < NCH; ++m) acc[m] += (c0 * a0.v[m] + c1 * a1.v[m]) + (c2 * a2.v[m] + c3 * a3.v[m]);
        }
        for (; e < end; ++e) {
            TeamRow<VEC, NCH> a0;
            a0.load(S, lds, ix[e], l15, K);
            float c0 = edge_coef(si.dot(a0));
            if constexpr (WT) c0 *= val[e];
#pragma unroll
            for (int m = 0; m < NCH; ++m) acc[m] += c0 * a0.v[m];
        }
    };
    walk(indptr, indices, values);
    if (directed) walk(indptr_t, indices_t, values_t);
    const float f = directed ? scale_ptr[0] : 2.f * scale_ptr[0];
#pragma unroll
    for (int m = 0; m < NCH; ++m) {
        const int col = (m * 16 + l15) * VEC;
        if (col < K) {
            V* q = reinterpret_cast<V*>(dS + (long)row * ldds + col);
            *q = *q + f * acc[m];
        }
    }
}

template <int VEC, int NCH>
__global__ __launch_bounds__(256) void k_csr_link_edge_bwd(const float* S, int lds_ld, const int* indptr,
                                                           const int* indices, const int* indptr_t,
                                                           const int* indices_t, const float* scale_ptr, float* dS,
                                                           int ldds, int n, int K, int directed) {
    csr_link_edge_bwd_body<VEC, NCH, false>(S, lds_ld, indptr, indices, indptr_t, indices_t, scale_ptr, dS, ldds, n, K,
                                            directed, nullptr, nullptr);
}
template <int VEC, int NCH>
__global__ __launch_bounds__(256) void k_csr_link_edge_bwd_w(const float* S, int lds_ld, const int* indptr,
                                                             const int* indices, const float* values,
                                                             const int* indptr_t, const int* indices_t,
                                                             const float* values_t, const float* scale_ptr, float* dS,
                                                             int ldds, int n, int K, int directed) {
    csr_link_edge_bwd_body<VEC, NCH, true>(S, lds_ld, indptr, indices, indptr_t, indices_t, scale_ptr, dS, ldds, n, K,
                                           directed, values, values_t);
}

// ------------------------------------------------------------------ the plan (host only; dp_csr_linkpred_plan)
// Everything the host decides for one graph, in one place: the launchers below act on this record and
// dp_csr_linkpred_plan reports it, so what is reported is what runs.
constexpr size_t dense_fwd_lds(int kt) { return (size_t)2 * 64 * (kt * 16 + 2) * sizeof(float); }
constexpr size_t dense_bwd_lds(int kt, int cw) {
    return ((size_t)(64 + cw) * (kt * 16 + 2) + 64 * (cw + 4)) * sizeof(float);
}
struct CsrLinkPlan {
    int kt;                                      // K tier of both dense kernels
    int T, pairs, Z;                             // forward: row blocks, row-block pairs (grid y), column splits (grid x)
    int n_dense, n_edge;                         // forward partials: pairs * Z, then one per edge workgroup
    int cw, col_tiles, splits, split_tiles;      // backward: column tile width, tiles, grid z, tiles per split
    int fwd_vec, fwd_nch, bwd_vec, bwd_nch;      // edge kernels: floats per lane load, chunks of 16 lanes per row
    size_t fwd_lds, bwd_lds;                     // dynamic LDS of the dense kernels
    size_t part_floats;                          // backward partial buffer (0: no split)
};
// (VEC, NCH) of the edge kernels: 16-byte lanes cover 64 columns per chunk, 4-byte lanes 16
void edge_form(bool v4, int K, int& vec, int& nch) {
    vec = v4 ? 4 : 1;
    nch = v4 ? (K <= 64 ? 1 : K <= 128 ? 2 : 4) : (K <= 16 ? 1 : K <= 64 ? 4 : 16);
}
// s_al16 / ds_al16: S / dS of this graph are 16-byte aligned.  The forward reads neither ldds nor ds_al16.
CsrLinkPlan csr_link_plan(int n, int K, int lds, int ldds, bool s_al16, bool ds_al16) {
    CsrLinkPlan p;
    p.kt = lk_kt(K);
    p.T = cdiv(n, 64);
    p.pairs = (p.T + 1) / 2;
    p.Z = std::max(1, std::min(p.T, cdiv(LK_FWD_TARGET_WGS, p.pairs)));
    p.n_dense = p.pairs * p.Z;
    p.n_edge = cdiv(n, LK_TEAM_ROWS);
    // few row blocks: the column tiles are split over extra workgroups and the partials summed afterwards (link_bwd's
    // rule, dp_linkpred.hip)
    p.cw = p.kt >= 12 ? 32 : 64;
    p.col_tiles = cdiv(n, p.cw);
    const int row_blocks = cdiv(n, 64);
    const int want = std::max(1, std::min(p.col_tiles, cdiv(LK_BWD_TARGET_WGS, row_blocks)));
    p.split_tiles = cdiv(p.col_tiles, want);
    p.splits = cdiv(p.col_tiles, p.split_tiles);
    p.part_floats = p.splits > 1 ? (size_t)p.splits * n * K : 0;
    const bool v4f = K % 4 == 0 && lds % 4 == 0 && s_al16;
    edge_form(v4f, K, p.fwd_vec, p.fwd_nch);
    edge_form(v4f && ldds % 4 == 0 && ds_al16, K, p.bwd_vec, p.bwd_nch);
    p.fwd_lds = dense_fwd_lds(p.kt);
    p.bwd_lds = dense_bwd_lds(p.kt, p.cw);
    return p;
}

// ------------------------------------------------------------------ launch sequences
template <int KT>
void launch_dense_fwd(Seq& q, const float* S, int lds, int n, int K, int T, int Z, double* partial) {
    constexpr size_t bytes = dense_fwd_lds(KT);
    static_assert(bytes + 256 * sizeof(double) <= 160 * 1024, "csr_link_dense_fwd LDS");
    static DynLdsOnce attr;
    if (bytes > 64 * 1024)
        ensure_dyn_lds(q, attr, reinterpret_cast<const void*>(&k_csr_link_dense_fwd<KT>), (int)bytes,
                       "k_csr_link_dense_fwd");
    if (!q.ok()) return;
    hipLaunchKernelGGL((k_csr_link_dense_fwd<KT>), dim3(Z, (T + 1) / 2), dim3(256), bytes, q.stream, S, lds, n, K, T,
                       partial);
}

// the edge kernel of the plan's form
#define LK_EDGE_DISPATCH(KERNEL, vec, nch, ...)                                                             \
    do {                                                                                                    \
        const dim3 grid_(cdiv(n, LK_TEAM_ROWS));                                                            \
        if (vec == 4) {                                                                                     \
            if (nch == 1) hipLaunchKernelGGL((KERNEL<4, 1>), grid_, dim3(256), 0, q.stream, __VA_ARGS__);   \
            else if (nch == 2) hipLaunchKernelGGL((KERNEL<4, 2>), grid_, dim3(256), 0, q.stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<4, 4>), grid_, dim3(256), 0, q.stream, __VA_ARGS__);            \
        } else {                                                                                            \
            if (nch == 1) hipLaunchKernelGGL((KERNEL<1, 1>), grid_, dim3(256), 0, q.stream, __VA_ARGS__);   \
            else if (nch == 4) hipLaunchKernelGGL((KERNEL<1, 4>), grid_, dim3(256), 0, q.stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<1, 16>), grid_, dim3(256), 0, q.stream, __VA_ARGS__);           \
        }                                                                                                   \
    } while (0)

int fwd_partials(int n) {
    const CsrLinkPlan p = csr_link_plan(n, 1, 1, 1, true, true);      // neither count depends on K or the strides
    return p.n_dense + p.n_edge;
}
// the dense and the edge partials of one graph -> partial[0 .. fwd_partials(n) - 1]
void csr_link_fwd_graph(Seq& q, const float* S, int lds, const int* indptr, const int* indices, int n, int K,
                        double* partial, const float* values) {
    const CsrLinkPlan p = csr_link_plan(n, K, lds, K, aligned16(S), true);
    if (!q.ok()) return;
#define LK_FWD(KT_) \
    case KT_: launch_dense_fwd<KT_>(q, S, lds, n, K, p.T, p.Z, partial); break;
    switch (p.kt) { LK_FWD(1) LK_FWD(2) LK_FWD(3) LK_FWD(4) LK_FWD(6) LK_FWD(8) LK_FWD(12) LK_FWD(16) }
#undef LK_FWD
    q.check_launch("csr_link_dense_fwd");
    if (!q.ok()) return;
    if (values)
        LK_EDGE_DISPATCH(k_csr_link_edge_fwd_w, p.fwd_vec, p.fwd_nch, S, lds, indptr, indices, values, n, K,
                         partial + p.n_dense);
    else LK_EDGE_DISPATCH(k_csr_link_edge_fwd, p.fwd_vec, p.fwd_nch, S, lds, indptr, indices, n, K, partial + p.n_dense);
    q.check_launch("csr_link_edge_fwd");
}

template <int KT, int NJ>
void launch_dense_bwd(Seq& q, const float* S, int lds, const float* scale, float* dS, int ldds, int n, int K,
                      int accumulate, float* part, int splits, int split_tiles) {
    constexpr size_t bytes = dense_bwd_lds(KT, 32 * NJ);
    static_assert(bytes <= 160 * 1024, "csr_link_dense_bwd LDS");
    static DynLdsOnce attr;
    if (bytes > 64 * 1024)
        ensure_dyn_lds(q, attr, reinterpret_cast<const void*>(&k_csr_link_dense_bwd<KT, NJ>), (int)bytes,
                       "k_csr_link_dense_bwd");
    if (!q.ok()) return;
    hipLaunchKernelGGL((k_csr_link_dense_bwd<KT, NJ>), dim3(cdiv(n, 64), 1, part ? splits : 1), dim3(256), bytes,
                       q.stream, S, lds, scale, dS, ldds, n, K, accumulate, part, split_tiles);
}

// the dense backward's partial buffer (floats; 0: no split)
size_t bwd_part_floats(int n, int K) { return csr_link_plan(n, K, K, K, true, true).part_floats; }
// one graph's dS from the ready scale; `part`: bwd_part_floats(n, K) floats (null when that is 0)
void csr_link_bwd_graph(Seq& q, const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                        const int* indices_t, const float* scale, float* part, float* dS, int ldds, int accumulate,
                        int n, int K, int directed, const float* values, const float* values_t) {
    const CsrLinkPlan p = csr_link_plan(n, K, lds, ldds, aligned16(S), aligned16(dS));
    if (!p.part_floats) part = nullptr;
    if (!q.ok()) return;
#define LK_BWD(KT_, NJ_)                                                                                          \
    case KT_:                                                                                                     \
        launch_dense_bwd<KT_, NJ_>(q, S, lds, scale, dS, ldds, n, K, accumulate, part, p.splits, p.split_tiles);  \
        break;
    switch (p.kt) { LK_BWD(1, 2) LK_BWD(2, 2) LK_BWD(3, 2) LK_BWD(4, 2) LK_BWD(6, 2) LK_BWD(8, 2) LK_BWD(12, 1) LK_BWD(16, 1) }
#undef LK_BWD
    q.check_launch("csr_link_dense_bwd");
    if (!q.ok()) return;
    if (part) {
        const int blocks = std::min(cdiv((long)n * K, 256), 2048);
        hipLaunchKernelGGL(k_csr_link_reduce, dim3(blocks), dim3(256), 0, q.stream, (const float*)part, p.splits, dS,
                           ldds, n, K, accumulate);
        q.check_launch("csr_link_reduce");
    }
    if (values)
        LK_EDGE_DISPATCH(k_csr_link_edge_bwd_w, p.bwd_vec, p.bwd_nch, S, lds, indptr, indices, values, indptr_t,
                         indices_t, values_t, (const float*)scale, dS, ldds, n, K, directed);
    else
        LK_EDGE_DISPATCH(k_csr_link_edge_bwd, p.bwd_vec, p.bwd_nch, S, lds, indptr, indices, indptr_t, indices_t,
                         (const float*)scale, dS, ldds, n, K, directed);
    q.check_launch("csr_link_edge_bwd");
}

// ---- the launch sequences, written for a ragged batch: loss = sum_b (graph b's sum) / sum_b n_b^2
// (encoders.py:1326-1331).  A lone graph of n rows is the batch B = 1, off = {0, n}: the single-graph entries build that
// table on the stack and come here, so there is one forward and one backward sequence.  Per-graph launches of the
// kernels above — the tile walk is n_b^2 work per graph anyway — into one partial array, one final launch for the
// batch; the backward forms the scale once.  indptr is the batch's (row node_off[b] + i, GLOBAL edge offsets), the
// column indices are graph-LOCAL.  Launch count grows with B (a batched tile table is the open item).
double batch_norm(const int* off, int B) {
    double nn = 0.0;
    for (int b = 0; b < B; ++b) nn += (double)(off[b + 1] - off[b]) * (double)(off[b + 1] - off[b]);
    return nn;
}
void csr_link_batch_fwd_seq(Seq& q, const float* S, int lds, const int* indptr, const int* indices, const int* off,
                            int B, float* loss_out, int K, const float* values = nullptr) {
    size_t count = 0;
    for (int b = 0; b < B; ++b) count += fwd_partials(off[b + 1] - off[b]);
    double* partial = q.alloc<double>(count);
    if (!q.ok()) return;
    size_t at = 0;
    for (int b = 0; b < B && q.ok(); ++b) {
        const int n = off[b + 1] - off[b];
        csr_link_fwd_graph(q, S + (long)off[b] * lds, lds, indptr + off[b], indices, n, K, partial + at, values);
        at += fwd_partials(n);
    }
    if (!q.ok()) return;
    hipLaunchKernelGGL(k_csr_link_final, dim3(1), dim3(256), 0, q.stream, (const double*)partial, (int)count,
                       batch_norm(off, B), loss_out, (float*)nullptr, (const float*)nullptr);
    q.check_launch("csr_link_final");
}
void csr_link_batch_bwd_seq(Seq& q, const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                            const int* indices_t, const int* off, int B, const float* dloss, float* dS, int ldds,
                            int accumulate, int K, const float* values = nullptr, const float* values_t = nullptr) {
    float* scale = q.alloc<float>(64);
    size_t pf = 0;
    for (int b = 0; b < B; ++b) pf = std::max(pf, bwd_part_floats(off[b + 1] - off[b], K));
    float* part = pf ? q.alloc<float>(pf) : nullptr;       // reused graph after graph: the launches are stream-ordered
    if (!q.ok()) return;
    hipLaunchKernelGGL(k_csr_link_final, dim3(1), dim3(256), 0, q.stream, (const double*)nullptr, 0, batch_norm(off, B),
                       (float*)nullptr, scale, dloss);
    q.check_launch("csr_link_scale");
    const int directed = (indptr_t != indptr || indices_t != indices) ? 1 : 0;
    for (int b = 0; b < B && q.ok(); ++b)
        csr_link_bwd_graph(q, S + (long)off[b] * lds, lds, indptr + off[b], indices, indptr_t + off[b], indices_t, scale,
                           part, dS + (long)off[b] * ldds, ldds, accumulate, off[b + 1] - off[b], K, directed, values,
                           values_t);
}
size_t batch_sized_bytes(const int* off, int B, int K) {
    Seq f = Seq::sizing();
    csr_link_batch_fwd_seq(f, nullptr, K, nullptr, nullptr, off, B, nullptr, K);
    Seq b = Seq::sizing();
    csr_link_batch_bwd_seq(b, nullptr, K, nullptr, nullptr, nullptr, nullptr, off, B, nullptr, nullptr, K, 0, K);
    return std::max(f.ws_off, b.ws_off);
}

}  // namespace
}  // namespace dp

using namespace dp;

namespace {

// The checked bodies of all eight loss entries.  off_host: the batch's node offsets on the HOST; `single`: the caller
// is a single-graph entry and off_host its {0, n}, so the refusals speak of n and of `indices`, not of the batch's
// table and `indices_local`.
int check_batch(const char* entry, bool single, const int* off, int B, int K, int lds, const void* workspace,
                size_t workspace_bytes) {
    if (single) {
        DP_CHECK(off[1] >= 1, DP_ERR_INVALID_ARG, "%s: n=%d must be positive", entry, off[1]);
    } else {
        DP_CHECK(off != nullptr, DP_ERR_INVALID_ARG, "%s: node_off_host is NULL", entry);
        DP_CHECK(B >= 1, DP_ERR_INVALID_ARG, "%s: B=%d must be positive", entry, B);
    }
    DP_CHECK(K >= 1, DP_ERR_INVALID_ARG, "%s: K=%d must be positive", entry, K);
    DP_CHECK(K <= 256, DP_ERR_UNSUPPORTED, "%s: K=%d clusters exceed the fused tile kernel (max 256)", entry, K);
    DP_CHECK(lds >= K, DP_ERR_INVALID_ARG, "%s: lds=%d smaller than K=%d", entry, lds, K);
    DP_CHECK(off[0] == 0, DP_ERR_INVALID_ARG, "%s: node_off[0] must be 0", entry);
    for (int b = 0; b < B; ++b)
        DP_CHECK(off[b + 1] > off[b], DP_ERR_INVALID_ARG, "%s: graph %d has no node (node_off must increase)", entry, b);
    DP_ALIGNED16(workspace, false, "%s: workspace is NULL or not 16-byte aligned", entry);
    const size_t need = batch_sized_bytes(off, B, K);
    DP_CHECK(workspace_bytes >= need, DP_ERR_INVALID_ARG, "%s: workspace too small: need >= %zu bytes, have %zu", entry,
             need, workspace_bytes);
    return DP_OK;
}
// indices / indices_t under the name the entry's signature gives them
#define LK_INDICES(p)                                                                                 \
    do {                                                                                              \
        const char* sfx_ = single ? "" : "_local";                                                    \
        DP_CHECK((p) != nullptr, DP_ERR_INVALID_ARG, #p "%s is NULL", sfx_);                          \
        DP_CHECK(((uintptr_t)(p) & 3) == 0, DP_ERR_INVALID_ARG, #p "%s is not 4-byte aligned", sfx_); \
    } while (0)
#define LK_ALIGNED4(p) DP_CHECK(((uintptr_t)(p) & 3) == 0, DP_ERR_INVALID_ARG, "%s: " #p " is not 4-byte aligned", entry)

int link_fwd_entry(const char* entry, bool single, const float* S, int lds, const int* indptr, const int* indices,
                   const float* values, bool weighted, const int* node_off_host, int B, float* loss_out, int K,
                   void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(S); DP_PTR(indptr); LK_INDICES(indices); DP_PTR(loss_out);
    DP_VALUES(LK_ALIGNED4(values), "%s: values is NULL", entry);
    if (int rc = check_batch(entry, single, node_off_host, B, K, lds, workspace, workspace_bytes)) return rc;
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    csr_link_batch_fwd_seq(q, S, lds, indptr, indices, node_off_host, B, loss_out, K, weighted ? values : nullptr);
    return q.err;
}
int link_bwd_entry(const char* entry, bool single, const float* S, int lds, const int* indptr, const int* indices,
                   const float* values, const int* indptr_t, const int* indices_t, const float* values_t, bool weighted,
                   const int* node_off_host, int B, const float* dloss, float* dS, int ldds, int accumulate, int K,
                   void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(S); DP_PTR(indptr); LK_INDICES(indices); DP_PTR(indptr_t); LK_INDICES(indices_t); DP_PTR(dS);
    DP_VALUES(LK_ALIGNED4(values), "%s: values is NULL", entry);
    DP_VALUES_T(LK_ALIGNED4(values_t), "%s: values_t is NULL but the transposed CSR is one of its own", entry);
    DP_ALIGNED4(dloss);
    if (int rc = check_batch(entry, single, node_off_host, B, K, lds, workspace, workspace_bytes)) return rc;
    DP_CHECK(ldds >= K, DP_ERR_INVALID_ARG, "%s: ldds=%d smaller than K=%d", entry, ldds, K);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    csr_link_batch_bwd_seq(q, S, lds, indptr, indices, indptr_t, indices_t, node_off_host, B, dloss, dS, ldds, accumulate,
                           K, weighted ? values : nullptr,
                           weighted ? values_t_of(indices, indices_t, values, values_t) : nullptr);
    return q.err;
}
#undef LK_ALIGNED4
#undef LK_INDICES

}  // namespace

extern "C" {

size_t dp_csr_linkpred_batch_workspace_bytes(const int* node_off_host, int B, int K) {
    if (!node_off_host || B < 1 || K < 1 || K > 256 || node_off_host[0] != 0) return 0;
    for (int b = 0; b < B; ++b)
        if (node_off_host[b + 1] <= node_off_host[b]) return 0;
    return batch_sized_bytes(node_off_host, B, K);
}
size_t dp_csr_linkpred_workspace_bytes(int n, int K) {
    const int off[2] = {0, n};
    return dp_csr_linkpred_batch_workspace_bytes(off, 1, K);
}
int dp_csr_linkpred_plan(int n, int K, int lds, int ldds, int s_misaligned, int ds_misaligned, int* plan_out) {
    const char* entry = "dp_csr_linkpred_plan";
    DP_CHECK(plan_out != nullptr, DP_ERR_INVALID_ARG, "%s: plan_out is NULL", entry);
    DP_CHECK(n >= 1, DP_ERR_INVALID_ARG, "%s: n=%d must be positive", entry, n);
    DP_CHECK(K >= 1, DP_ERR_INVALID_ARG, "%s: K=%d must be positive", entry, K);
    DP_CHECK(K <= 256, DP_ERR_UNSUPPORTED, "%s: K=%d clusters exceed the fused tile kernel (max 256)", entry, K);
    DP_CHECK(lds >= K, DP_ERR_INVALID_ARG, "%s: lds=%d smaller than K=%d", entry, lds, K);
    DP_CHECK(ldds >= K, DP_ERR_INVALID_ARG, "%s: ldds=%d smaller than K=%d", entry, ldds, K);
    const CsrLinkPlan p = csr_link_plan(n, K, lds, ldds, !s_misaligned, !ds_misaligned);
    const int out[DP_CSR_LINKPRED_PLAN_INTS] = {p.kt, p.T, p.pairs, p.Z, p.n_dense, p.n_edge, p.cw, p.col_tiles,
                                                p.splits, p.split_tiles, p.fwd_vec, p.fwd_nch, p.bwd_vec, p.bwd_nch,
                                                (int)p.fwd_lds, (int)p.bwd_lds};
    for (int i = 0; i < DP_CSR_LINKPRED_PLAN_INTS; ++i) plan_out[i] = out[i];
    return DP_OK;
}

// ---- one graph: the batch of one, off = {0, n}
int dp_csr_linkpred_loss_fwd(const float* S, int lds, const int* indptr, const int* indices, float* loss_out, int n,
                             int K, void* workspace, size_t workspace_bytes, void* stream) {
    const int off[2] = {0, n};
    return link_fwd_entry("dp_csr_linkpred_loss_fwd", true, S, lds, indptr, indices, nullptr, false, off, 1, loss_out, K,
                          workspace, workspace_bytes, stream);
}
int dp_csr_linkpred_loss_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                               float* loss_out, int n, int K, void* workspace, size_t workspace_bytes, void* stream) {
    const int off[2] = {0, n};
    return link_fwd_entry("dp_csr_linkpred_loss_fwd_w", true, S, lds, indptr, indices, values, true, off, 1, loss_out, K,
                          workspace, workspace_bytes, stream);
}
int dp_csr_linkpred_loss_bwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                             const int* indices_t, const float* dloss, float* dS, int ldds, int accumulate, int n,
                             int K, void* workspace, size_t workspace_bytes, void* stream) {
    const int off[2] = {0, n};
    return link_bwd_entry("dp_csr_linkpred_loss_bwd", true, S, lds, indptr, indices, nullptr, indptr_t, indices_t,
                          nullptr, false, off, 1, dloss, dS, ldds, accumulate, K, workspace, workspace_bytes, stream);
}
int dp_csr_linkpred_loss_bwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                               const int* indptr_t, const int* indices_t, const float* values_t, const float* dloss,
                               float* dS, int ldds, int accumulate, int n, int K, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const int off[2] = {0, n};
    return link_bwd_entry("dp_csr_linkpred_loss_bwd_w", true, S, lds, indptr, indices, values, indptr_t, indices_t,
                          values_t, true, off, 1, dloss, dS, ldds, accumulate, K, workspace, workspace_bytes, stream);
}

// ---- a ragged batch (node_off_host: int32 [B + 1] on the HOST)
int dp_csr_linkpred_batch_loss_fwd(const float* S, int lds, const int* indptr, const int* indices_local,
                                   const int* node_off_host, int B, float* loss_out, int K, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return link_fwd_entry("dp_csr_linkpred_batch_loss_fwd", false, S, lds, indptr, indices_local, nullptr, false,
                          node_off_host, B, loss_out, K, workspace, workspace_bytes, stream);
}
int dp_csr_linkpred_batch_loss_fwd_w(const float* S, int lds, const int* indptr, const int* indices_local,
                                     const float* values, const int* node_off_host, int B, float* loss_out, int K,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return link_fwd_entry("dp_csr_linkpred_batch_loss_fwd_w", false, S, lds, indptr, indices_local, values, true,
                          node_off_host, B, loss_out, K, workspace, workspace_bytes, stream);
}
int dp_csr_linkpred_batch_loss_bwd(const float* S, int lds, const int* indptr, const int* indices_local,
                                   const int* indptr_t, const int* indices_t_local, const int* node_off_host, int B,
                                   const float* dloss, float* dS, int ldds, int accumulate, int K, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return link_bwd_entry("dp_csr_linkpred_batch_loss_bwd", false, S, lds, indptr, indices_local, nullptr, indptr_t,
                          indices_t_local, nullptr, false, node_off_host, B, dloss, dS, ldds, accumulate, K, workspace,
                          workspace_bytes, stream);
}
int dp_csr_linkpred_batch_loss_bwd_w(const float* S, int lds, const int* indptr, const int* indices_local,
                                     const float* values, const int* indptr_t, const int* indices_t_local,
                                     const float* values_t, const int* node_off_host, int B, const float* dloss,
                                     float* dS, int ldds, int accumulate, int K, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return link_bwd_entry("dp_csr_linkpred_batch_loss_bwd_w", false, S, lds, indptr, indices_local, values, indptr_t,
                          indices_t_local, values_t, true, node_off_host, B, dloss, dS, ldds, accumulate, K, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
