// Frobenius link loss of the soft assignment S (the DiffPool paper's L_LP, squared):
//
//     F      = sum_b sum_{i,j < n_b} (a_bij - s_bi . s_bj)^2  =  T0 - 2 T1 + T2
//     T0     = sum a^2                      (0/1 CSR: the number of stored entries; weighted CSR: sum of values^2)
//     2 T1   = sum_i s_i . w_i,   W = (A + A^T) S
//     T2     = sum_b ||G_b||_F^2,  G_b = S_b^T S_b  [K, K]
//     link   = F / sum_b n_b^2
//     dF/dS  = 4 S G - 2 W                  (row-local: dS_i = coef (4 G s_i - 2 w_i))
//
// No n x n temporary: O(n K^2 + nnz K) work, O(n K) memory.  One set of kernels serves two row layouts:
//     dense   S [B, N, K] (rows lds apart), graph b owns rows b N .. b N + n_b - 1, n_b = num_nodes[b] clamped to [0, N]
//     ragged  S [n_total, K], graph b owns rows node_off[b] .. node_off[b + 1] - 1 (one CSR graph: B = 1, no node_off)
// A row behind a graph's n_b is never read by any kernel here.
//
// Gram: rows are cut into slabs of FL_SLAB global rows; a workgroup owns (slab, 32 x 32 tile of G) and forms, for every
// graph that has rows in the slab, the partial product over those rows — fp32 operands from LDS, products and sums in
// fp64 — into slot slab + b (slabs and graphs both advance monotonically along the rows, so the slot is unique and at
// most slabs + B slots exist).  A second launch adds a graph's slots in slab order, rounds G_b to fp32 once (the backward
// reads it) and forms ||G_b||^2 from the fp64 values.
// Row term and dense T0: 64 lanes per row, fp32 products (s w, a a), fp64 sums in a fixed order (lane, LDS tree,
// partials by the finishing launch) as dp_assign_ent.hip does.  No atomics anywhere: every result is the same bits on
// every run.
#include "dp_common.h"

namespace dp {
namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_SLAB = DP_FROB_LINK_SLAB;    // global rows per Gram slab
constexpr int FL_TILE = 32;             // G is cut into 32 x 32 tiles
constexpr int FL_CHUNK = 64;            // rows staged per LDS visit of the Gram kernel (as doubles: 2 x 17 KB)
constexpr int FL_MAX_BLOCKS = 2048;     // row-term workgroups (8 per CU); the rest of the rows by the grid-stride loop
constexpr int FL_WROWS = 16;            // rows of W a workgroup of the dense aggregation owns
constexpr int FL_WCOLS = 32;            // adjacency columns (= rows of S) it stages per visit

struct FlLayout {
    const int* node_off;     // ragged: [B + 1]; null: dense (or one graph with N = n)
    const int* num_nodes;    // dense: [B] or null = N everywhere
    int N;                   // dense: rows per graph
    int B;
};

__device__ __forceinline__ long long fl_start(const FlLayout& L, int b) {
    return L.node_off ? (long long)L.node_off[b] : (long long)b * L.N;
}
__device__ __forceinline__ int fl_nb(const FlLayout& L, int b) {
    if (L.node_off) return L.node_off[b + 1] - L.node_off[b];
    if (!L.num_nodes) return L.N;
    const int v = L.num_nodes[b];
    return v < 0 ? 0 : (v > L.N ? L.N : v);
}
// the graph whose row range [start, start + N or next start) holds global row r
__device__ __forceinline__ int fl_graph_of(const FlLayout& L, long long r) {
    if (!L.node_off) return (int)(r / L.N);
    int lo = 0, hi = L.B - 1;                    // largest b with node_off[b] <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)L.node_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// fixed-order workgroup sum through LDS (every thread calls it; the total is returned to all)
template <typename T>
__device__ __forceinline__ T fl_block_sum(T v, T* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = FL_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    return sh[0];
}

// sum_b n_b^2 as a double (exact below 2^53), formed by the calling workgroup
__device__ __forceinline__ double fl_norm(const FlLayout& L, const float* link_norm, long long* shn) {
    if (link_norm) return (double)link_norm[0];
    long long c = 0;
    for (int b = threadIdx.x; b < L.B; b += FL_THREADS) {
        const long long nb = fl_nb(L, b);
        c += nb * nb;
    }
    return (double)fl_block_sum(c, shn);
}

__device__ __forceinline__ float fl_bf16(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// ----------------------------------------------------------------------------------------------- Gram partials
// grid (slabs, tiles * tiles); part [slabs + B][K][K] doubles
__global__ __launch_bounds__(FL_THREADS) void k_fl_gram_part(const float* __restrict__ S, int lds, FlLayout L,
                                                             double* __restrict__ part, long long rows, int K,
                                                             int tiles) {
    __shared__ double sa[FL_CHUNK][FL_TILE + 1];                 // widened once while staging, not once per product
    __shared__ double sb[FL_CHUNK][FL_TILE + 1];
    const int ta = blockIdx.y / tiles, tb = blockIdx.y % tiles;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const long long slab_lo = (long long)blockIdx.x * FL_SLAB;
    const long long slab_hi = slab_lo + FL_SLAB < rows ? slab_lo + FL_SLAB : rows;
    for (int b = fl_graph_of(L, slab_lo); b < L.B; ++b) {
        const long long gs = fl_start(L, b);
        if (gs >= slab_hi) break;
        const long long ge = gs + fl_nb(L, b);
        const long long lo = gs > slab_lo ? gs : slab_lo;
        const long long hi = ge < slab_hi ? ge : slab_hi;
        if (lo >= hi) continue;                                  // the slab starts in this graph's padding
        double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        for (long long r0 = lo; r0 < hi; r0 += FL_CHUNK) {
            const int nr = (int)(hi - r0 < FL_CHUNK ? hi - r0 : FL_CHUNK);
            __syncthreads();                                     // the previous chunk is consumed
            for (int e = threadIdx.x; e < FL_CHUNK * FL_TILE; e += FL_THREADS) {
                const int r = e / FL_TILE, c = e % FL_TILE;
                float va = 0.f, vb = 0.f;
                if (r < nr) {
                    const float* row = S + (size_t)(r0 + r) * (size_t)lds;
                    if (ta * FL_TILE + c < K) va = row[ta * FL_TILE + c];
                    if (ta == tb) vb = va;
                    else if (tb * FL_TILE + c < K) vb = row[tb * FL_TILE + c];
                }
                sa[r][c] = (double)va;
                sb[r][c] = (double)vb;
            }
            __syncthreads();
            for (int r = 0; r < nr; ++r) {
                const double a0 = sa[r][ty * 2], a1 = sa[r][ty * 2 + 1];
                const double b0 = sb[r][tx * 2], b1 = sb[r][tx * 2 + 1];
                acc[0][0] = fma(a0, b0, acc[0][0]);
                acc[0][1] = fma(a0, b1, acc[0][1]);
                acc[1][0] = fma(a1, b0, acc[1][0]);
                acc[1][1] = fma(a1, b1, acc[1][1]);
            }
        }
        double* out = part + ((size_t)blockIdx.x + (size_t)b) * (size_t)K * (size_t)K;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ga = ta * FL_TILE + ty * 2 + i, gb = tb * FL_TILE + tx * 2 + j;
                if (ga < K && gb < K) out[(size_t)ga * K + gb] = acc[i][j];
            }
    }
}

// grid (B, blocks over K * K): G_b = the graph's slots in slab order; g2part [B * blocks] = sums of squares
__global__ __launch_bounds__(FL_THREADS) void k_fl_gram_reduce(const double* __restrict__ part, FlLayout L,
                                                               float* __restrict__ G, double* __restrict__ g2part,
                                                               int K) {
    __shared__ double sh[FL_THREADS];
    const int b = blockIdx.x;
    const int e = blockIdx.y * FL_THREADS + threadIdx.x;
    const int nb = fl_nb(L, b);
    double g = 0.0;
    if (e < K * K && nb > 0) {
        const long long gs = fl_start(L, b);
        const long long t0 = gs / FL_SLAB, t1 = (gs + nb - 1) / FL_SLAB;
        // eight interleaved chains (slot t goes to chain (t - t0) % 8) keep eight loads in flight; the chains are then
        // added in a fixed order, so the sum is the same bits on every run
        double c8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const size_t kk = (size_t)K * (size_t)K;
        long long t = t0;
        for (; t + 7 <= t1; t += 8)
#pragma unroll
            for (int u = 0; u < 8; ++u) c8[u] += part[((size_t)(t + u) + (size_t)b) * kk + (size_t)e];
        for (int u = 0; t <= t1; ++t, ++u) c8[u] += part[((size_t)t + (size_t)b) * kk + (size_t)e];
        g = ((c8[0] + c8[1]) + (c8[2] + c8[3])) + ((c8[4] + c8[5]) + (c8[6] + c8[7]));
    }
    if (e < K * K) G[(size_t)b * K * K + e] = (float)g;
    const double tot = fl_block_sum(g * g, sh);
    if (threadIdx.x == 0) g2part[(size_t)b * gridDim.y + blockIdx.y] = tot;
}

// ----------------------------------------------------------------------------------------------- dense W = (A + A^T) S
// One workgroup: FL_WROWS rows of one graph, all K columns (16 column lanes, columns lane, lane + 16, ...).  The sum
// c_ij = a_ij + a^T_ij is formed once per entry in fp32 (exact for 0/1; twice a_ij when the caller's A^T IS its A) and
// the row of W accumulated over j in ascending order with one fma per term: the fp32 and the packed entry run the same
// arithmetic in the same order, so they agree bit for bit wherever bf16 holds the adjacency exactly.
// ADJ 1: fp32 [B, N, N], A^T read as the transposed element; ADJ 2: bf16 rows pk / pkt [B, N, ld].
// NQ: columns per lane, 16 NQ >= K (1, 2, 4, 8 or 16)
template <int ADJ, int NQ>
__global__ __launch_bounds__(FL_THREADS) void k_fl_w_dense(const float* __restrict__ S, int lds,
                                                           const void* __restrict__ adj, const void* __restrict__ adj_t,
                                                           int ld, const int* __restrict__ num_nodes,
                                                           float* __restrict__ W, int N, int K, int tiles) {
    __shared__ float sc[FL_WROWS][FL_WCOLS + 1];                 // a_ij
    __shared__ float sct[FL_WROWS][FL_WCOLS + 1];                // a^T_ij = a_ji
    __shared__ float ss[FL_WCOLS][256];                          // the chunk's rows of S (K <= 256)
    static_assert(FL_WROWS * FL_WCOLS == 2 * FL_THREADS, "two entries per thread");
    const int b = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * FL_WROWS;
    int nb = N;
    if (num_nodes) {
        const int v = num_nodes[b];
        nb = v < 0 ? 0 : (v > N ? N : v);
    }
    if (i0 >= nb) return;
    const int r = threadIdx.x >> 4, cl = threadIdx.x & 15;
    const bool same = adj == adj_t;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    for (int j0 = 0; j0 < nb; j0 += FL_WCOLS) {
        __syncthreads();                                         // the previous chunk is consumed
        // every load of the chunk is issued before the one barrier: a_ij along row i, a_ji along row j (fp32: the
        // transposed element, read coalesced over i; packed: the same position of the A^T copy), the rows of S
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = threadIdx.x + h * FL_THREADS;
            const int rr = e / FL_WCOLS, jj = e % FL_WCOLS;
            const int i = i0 + rr, j = j0 + jj;
            const bool in = i < nb && j < nb;
            if constexpr (ADJ == 1) {
                const float* A = static_cast<const float*>(adj) + (size_t)b * N * N;
                sc[rr][jj] = in ? A[(size_t)i * N + j] : 0.f;
                const int jt = e / FL_WROWS, rt = e % FL_WROWS;      // transposed walk of the same tile
                sct[rt][jt] = (i0 + rt < nb && j0 + jt < nb) ? A[(size_t)(j0 + jt) * N + i0 + rt] : 0.f;
            } else {
                const size_t at = ((size_t)b * N + i) * (size_t)ld + j;
                const float a = in ? fl_bf16(static_cast<const unsigned short*>(adj)[at]) : 0.f;
                sc[rr][jj] = a;
                sct[rr][jj] = same ? a : (in ? fl_bf16(static_cast<const unsigned short*>(adj_t)[at]) : 0.f);
            }
        }
        const int nj = nb - j0 < FL_WCOLS ? nb - j0 : FL_WCOLS;
        for (int e = threadIdx.x; e < nj * 16 * NQ; e += FL_THREADS) {      // columns K .. 16 NQ - 1 hold zeros
            const int jj = e / (16 * NQ), k = e % (16 * NQ);
            ss[jj][k] = k < K ? S[((size_t)b * N + j0 + jj) * (size_t)lds + k] : 0.f;
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            const float c = sc[r][jj] + sct[r][jj];              // fl(a_ij + a_ji): exact for 0/1
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = fmaf(c, ss[jj][cl + q * 16], acc[q]);
        }
    }
    if (i0 + r < nb) {
        float* wrow = W + ((size_t)b * N + i0 + r) * (size_t)K;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int k = cl + q * 16;
            if (k < K) wrow[k] = acc[q];
        }
    }
}

// ----------------------------------------------------------------------------------------------- row term (+ dense T0)
// part[2 blk] = sum over the workgroup's valid rows of s_i . w_i, part[2 blk + 1] = of sum_{j < n_b} a_ij^2
// ADJ 0: no adjacency (CSR: T0 is the entry count); 1: fp32, 4-byte loads; 2: fp32, 16-byte loads; 3: bf16, 16-byte loads;
// 4: weighted CSR — adj holds the stored values, row r's are indptr[r] .. indptr[r + 1] - 1, squared and summed in fp64
template <int ADJ>
__device__ __forceinline__ void fl_rows_body(const float* __restrict__ S, int lds, const float* __restrict__ W,
                                             const void* __restrict__ adj, int ld, const FlLayout& L,
                                             double* __restrict__ part, long long rows, int K,
                                             const int* __restrict__ indptr) {
    __shared__ double sh[FL_THREADS];
    const int grp = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double t1 = 0.0, t0 = 0.0;
    for (long long r = (long long)blockIdx.x * 4 + grp; r < rows; r += (long long)gridDim.x * 4) {
        int nb = 0;
        if (L.node_off == nullptr && (L.num_nodes != nullptr || (ADJ != 0 && ADJ != 4))) {
            const int b = (int)(r / L.N);
            nb = fl_nb(L, b);
            if ((int)(r - (long long)b * L.N) >= nb) continue;
        }
        const float* srow = S + (size_t)r * (size_t)lds;
        const float* wrow = W + (size_t)r * (size_t)K;
        for (int k = lane; k < K; k += 64) t1 += (double)(srow[k] * wrow[k]);
        if constexpr (ADJ == 1) {
            const float* arow = static_cast<const float*>(adj) + (size_t)r * (size_t)ld;
            for (int j = lane; j < nb; j += 64) {
                const float a = arow[j];
                t0 += (double)(a * a);
            }
        } else if constexpr (ADJ == 2) {
            const float* arow = static_cast<const float*>(adj) + (size_t)r * (size_t)ld;
            for (int j = lane * 4; j < nb; j += 256) {                // ld % 4 == 0: the 16 bytes lie inside the row
                const float4 v = *reinterpret_cast<const float4*>(arow + j);
                const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < nb) t0 += (double)(a[e] * a[e]);
            }
        } else if constexpr (ADJ == 3) {
            const unsigned short* arow = static_cast<const unsigned short*>(adj) + (size_t)r * (size_t)ld;
            for (int j = lane * 8; j < nb; j += 512) {                // ld % 8 == 0: the 16 bytes lie inside the row
                const uint4 v = *reinterpret_cast<const uint4*>(arow + j);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = fl_bf16((unsigned short)(w[e >> 1] >> ((e & 1) * 16)));
                    if (j + e < nb) t0 += (double)(a * a);
                }
            }
        } else if constexpr (ADJ == 4) {
            const float* val = static_cast<const float*>(adj);
            const int e1 = indptr[r + 1];
            for (int e = indptr[r] + lane; e < e1; e += 64) {
                const double a = (double)val[e];
                t0 += a * a;
            }
        }
    }
    const double s1 = fl_block_sum(t1, sh);
    const double s0 = fl_block_sum(t0, sh);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s1;
        part[2 * blockIdx.x + 1] = s0;
    }
}

template <int ADJ>
__global__ __launch_bounds__(FL_THREADS) void k_fl_rows(const float* __restrict__ S, int lds, const float* __restrict__ W,
                                                        const void* __restrict__ adj, int ld, FlLayout L,
                                                        double* __restrict__ part, long long rows, int K) {
    fl_rows_body<ADJ>(S, lds, W, adj, ld, L, part, rows, K, nullptr);
}
// the weighted CSR form (ADJ 4): values and the CSR's indptr
__global__ __launch_bounds__(FL_THREADS) void k_fl_rows_w(const float* __restrict__ S, int lds,
                                                          const float* __restrict__ W, const float* __restrict__ values,
                                                          const int* __restrict__ indptr, FlLayout L,
                                                          double* __restrict__ part, long long rows, int K) {
    fl_rows_body<4>(S, lds, W, values, 0, L, part, rows, K, indptr);
}

// ----------------------------------------------------------------------------------------------- finish
// one workgroup: F = T0 - wscale * sum s.w + sum ||G_b||^2 in fp64, divided by the normaliser in fp64, rounded once
__global__ __launch_bounds__(FL_THREADS) void k_fl_finish(const double* __restrict__ part, int nparts,
                                                          const double* __restrict__ g2part, int ng2, FlLayout L,
                                                          const int* __restrict__ nnz_ptr, const float* __restrict__ link_norm,
                                                          double wscale, float* __restrict__ loss_out,
                                                          float* __restrict__ total_inout) {
    __shared__ double sh[FL_THREADS];
    __shared__ long long shn[FL_THREADS];
    double a1 = 0.0, a0 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < nparts; i += FL_THREADS) {
        a1 += part[2 * i];
        a0 += part[2 * i + 1];
    }
    for (int i = threadIdx.x; i < ng2; i += FL_THREADS) a2 += g2part[i];
    const double t1 = fl_block_sum(a1, sh);
    double t0 = fl_block_sum(a0, sh);
    const double t2 = fl_block_sum(a2, sh);
    const double norm = fl_norm(L, link_norm, shn);
    if (threadIdx.x == 0) {
        if (nnz_ptr) t0 = (double)nnz_ptr[0];
        const float term = norm > 0.0 ? (float)(((t0 - wscale * t1) + t2) / norm) : 0.f;
        loss_out[0] = term;
        if (total_inout) total_inout[0] = total_inout[0] + term;
    }
}

// ----------------------------------------------------------------------------------------------- backward
// dS_i (+)= coef (4 G_b s_i - 2 wscale w_i), coef = dloss / norm.  Four rows per workgroup visit, 64 lanes per row, the
// row of S in LDS; G is symmetric, so column k of G_b s_i is read along a row of G (coalesced over the lanes).
__global__ __launch_bounds__(FL_THREADS) void k_fl_bwd(const float* __restrict__ S, int lds, const float* __restrict__ W,
                                                       const float* __restrict__ G, FlLayout L,
                                                       const float* __restrict__ link_norm, const float* __restrict__ dloss,
                                                       float wscale, float* __restrict__ dS, int ldds, int accumulate,
                                                       long long rows, int K) {
    __shared__ long long shn[FL_THREADS];
    __shared__ float ss[4][256];
    const int grp = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double norm = fl_norm(L, link_norm, shn);
    const float coef = norm > 0.0 ? (float)((double)(dloss ? dloss[0] : 1.f) / norm) : 0.f;
    const float w2 = 2.f * wscale;
    for (long long r0 = (long long)blockIdx.x * 4; r0 < rows; r0 += (long long)gridDim.x * 4) {
        const long long r = r0 + grp;
        int b = 0;
        bool valid = r < rows;
        if (valid) {
            b = fl_graph_of(L, r);
            valid = r - fl_start(L, b) < (long long)fl_nb(L, b);
        }
        __syncthreads();                                         // the previous visit's rows are consumed
        if (valid)
            for (int k = lane; k < K; k += 64) ss[grp][k] = S[(size_t)r * (size_t)lds + k];
        __syncthreads();
        if (r >= rows) continue;
        float* drow = dS + (size_t)r * (size_t)ldds;
        if (!valid) {
            if (!accumulate)
                for (int k = lane; k < K; k += 64) drow[k] = 0.f;
            continue;
        }
        const float* Gb = G + (size_t)b * K * K;
        const float* wrow = W + (size_t)r * (size_t)K;
        for (int k = lane; k < K; k += 64) {
            float gs = 0.f;
            for (int c = 0; c < K; ++c) gs = fmaf(Gb[(size_t)c * K + k], ss[grp][c], gs);
            const float d = coef * (4.f * gs - w2 * wrow[k]);
            drow[k] = accumulate ? drow[k] + d : d;
        }
    }
}

int fl_rows_grid(long long rows) {
    const long long blocks = (rows + 3) / 4;
    return (int)(blocks < FL_MAX_BLOCKS ? blocks : FL_MAX_BLOCKS);
}

}  // namespace

// doubles the forward carves out of the workspace: Gram slots, their squares' partials, the row-term partials
size_t frob_link_ws_doubles(long long rows, int B, int K) {
    const size_t slabs = (size_t)((rows + FL_SLAB - 1) / FL_SLAB);
    const size_t g2 = (size_t)B * (size_t)(((size_t)K * K + FL_THREADS - 1) / FL_THREADS);
    return (slabs + (size_t)B) * (size_t)K * (size_t)K + g2 + 2 * (size_t)FL_MAX_BLOCKS;
}

// W is already in place ([rows, K], every valid row written).  adj_kind: 0 none (nnz_ptr gives T0), 1 fp32 [B, N, N],
// 3 bf16 rows (ld = adj_pack_ld(N)), 4 the stored values of a weighted CSR (adj) with its indptr (csr_indptr; nnz_ptr null).
void frob_link_fwd(Seq& q, const float* S, int lds, const float* W, const void* adj, int adj_kind, int adj_ld,
                   const int* num_nodes, const int* node_off, const int* nnz_ptr, const float* link_norm, float wscale,
                   float* G, float* loss_out, float* total_inout, int B, int N, long long rows, int K,
                   const int* csr_indptr) {
    const size_t slabs = (size_t)((rows + FL_SLAB - 1) / FL_SLAB);
    const int tiles = (K + FL_TILE - 1) / FL_TILE;
    const int g2blocks = (K * K + FL_THREADS - 1) / FL_THREADS;
    double* part = q.alloc<double>((slabs + (size_t)B) * (size_t)K * (size_t)K);
    double* g2part = q.alloc<double>((size_t)B * g2blocks);
    double* rpart = q.alloc<double>(2 * (size_t)FL_MAX_BLOCKS);
    if (!q.ok()) return;
    const FlLayout L{node_off, num_nodes, N, B};
    hipLaunchKernelGGL(k_fl_gram_part, dim3((unsigned)slabs, tiles * tiles), dim3(FL_THREADS), 0, q.stream, S, lds, L, part,
                       rows, K, tiles);
    q.check_launch("k_fl_gram_part");
    hipLaunchKernelGGL(k_fl_gram_reduce, dim3(B, g2blocks), dim3(FL_THREADS), 0, q.stream, part, L, G, g2part, K);
    q.check_launch("k_fl_gram_reduce");
    const int grid = fl_rows_grid(rows);
    int kind = adj_kind;
    if (kind == 1 && ((uintptr_t)adj & 15) == 0 && (adj_ld & 3) == 0) kind = 2;
#define FL_ROWS(A) \
    hipLaunchKernelGGL((k_fl_rows<A>), dim3(grid), dim3(FL_THREADS), 0, q.stream, S, lds, W, adj, adj_ld, L, rpart, rows, K)
    if (kind == 0) FL_ROWS(0); else if (kind == 1) FL_ROWS(1); else if (kind == 2) FL_ROWS(2); else if (kind == 3) FL_ROWS(3);
    else hipLaunchKernelGGL(k_fl_rows_w, dim3(grid), dim3(FL_THREADS), 0, q.stream, S, lds, W, static_cast<const float*>(adj),
                            csr_indptr, L, rpart, rows, K);
#undef FL_ROWS
    q.check_launch("k_fl_rows");
    if (!q.ok()) return;
    hipLaunchKernelGGL(k_fl_finish, dim3(1), dim3(FL_THREADS), 0, q.stream, rpart, grid, g2part, B * g2blocks, L, nnz_ptr,
                       link_norm, (double)wscale, loss_out, total_inout);
    q.check_launch("k_fl_finish");
}

// W [B, N, K] = (A + A^T) S from the dense fp32 adjacency (adj_t null) or the packed rows pk / pkt (ld = adj_pack_ld(N))
void frob_link_w_dense(Seq& q, const float* S, int lds, const void* adj, const void* adj_t, int packed, int ld,
                       const int* num_nodes, float* W, int B, int N, int K) {
    if (!q.ok()) return;
    const int tiles = (N + FL_WROWS - 1) / FL_WROWS;
    const void* at = packed ? adj_t : adj;
#define FL_W(A, NQ) \
    hipLaunchKernelGGL((k_fl_w_dense<A, NQ>), dim3(B * tiles), dim3(FL_THREADS), 0, q.stream, S, lds, adj, at, ld, num_nodes, \
                       W, N, K, tiles)
#define FL_W_NQ(A) \
    do { if (K <= 16) FL_W(A, 1); else if (K <= 32) FL_W(A, 2); else if (K <= 64) FL_W(A, 4); else if (K <= 128) FL_W(A, 8); \
         else FL_W(A, 16); } while (0)
    if (packed) FL_W_NQ(2); else FL_W_NQ(1);
#undef FL_W_NQ
#undef FL_W
    q.check_launch("k_fl_w_dense");
}

void frob_link_bwd(Seq& q, const float* S, int lds, const float* W, const float* G, const int* num_nodes,
                   const int* node_off, const float* link_norm, const float* dloss, float wscale, float* dS, int ldds,
                   int accumulate, int B, int N, long long rows, int K) {
    if (!q.ok()) return;
    const FlLayout L{node_off, num_nodes, N, B};
    hipLaunchKernelGGL(k_fl_bwd, dim3(fl_rows_grid(rows)), dim3(FL_THREADS), 0, q.stream, S, lds, W, G, L, link_norm, dloss,
                       wscale, dS, ldds, accumulate, rows, K);
    q.check_launch("k_fl_bwd");
}

}  // namespace dp
