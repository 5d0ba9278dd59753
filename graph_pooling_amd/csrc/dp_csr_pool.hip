// Level-0 DiffPool pooling on ONE graph stored as CSR (N4): the sparse form of encoders.py:1278-1279,
//     Xp = S^T Z [K,D],   Ap = S^T A S [K,K],
// and its backward
//     dS = (A S) dAp^T + (A^T S) dAp + Z dXp^T   (overwritten),   dZ += S dXp.
//
// Forward.  The pooled block [Ap | Xp] = S^T [A S | Z] is a K x (K+D) result of a contraction over all n rows: tall and
// skinny.  A GEMM over a materialised A S gets a few dozen workgroups (the output is ~50 x 110 on DD) each walking
// 10^5 rows, and writes / re-reads the n x K product.  Here the rows are cut into slabs instead: workgroup (t, s) owns
// output column tile t (64 columns of [A S | Z], all K rows of the result) and row slab s.  Stage by stage (32 rows)
// it gathers (A S)_i = sum_{j in N(i)} S_j for its columns straight into LDS (Z columns are copied), stages
// S_stage [32 x K] next to it, and accumulates S_stage^T [A S | Z]_stage on v_mfma_f32_16x16x4_f32 (exact fp32
// products, the numerics of dp_gemm.hip).  Each workgroup writes its K x 64 partial; a second launch sums the slabs'
// partials in slab order.  No float atomics, so the result is bit-reproducible; A S never reaches memory.  The slab
// count is chosen so the grid holds >= 1024 workgroups (>= 4 per CU) when the graph has the rows for it.
//
// Backward.  Row-local: a workgroup owns 64 rows.  Phase 1 accumulates dS_rows = X_rows Wcat over 32-column chunks of
// X = [A S | A^T S | Z] (gathered / copied into LDS chunk by chunk) against Wcat = [dAp^T ; dAp ; dXp^T]; for an
// undirected graph (transposed CSR == forward CSR) A^T S = A S, so X = [A S | Z] and Wcat = [dAp^T + dAp ; dXp^T].
// Phase 2 accumulates S_rows dXp the same way and adds it to dZ.  Wcat and a zero-padded copy of dXp are laid out once
// per call by a small prologue launch (L2-resident afterwards).  No atomics: every row of dS / dZ has one writer.
#include <algorithm>

#include "dp_entry.h"

namespace dp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FWD_ROWS = 32;        // rows per forward stage
constexpr int FWD_TN = 64;          // output columns of [A S | Z] per forward workgroup
constexpr int FWD_TARGET_WGS = 1024;
constexpr int FWD_MIN_SLAB = 64;    // rows per slab at least (bounds the partial traffic on small graphs)
constexpr int BWD_ROWS = 64;        // rows per backward workgroup (4 waves x one 16-row MFMA tile)
constexpr int BWD_KC = 32;          // contraction chunk of the backward

template <int VEC> struct Vec;
template <> struct Vec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ void put(float* p, T v) { *p = v; }
};
template <> struct Vec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void put(float* p, T v) { *reinterpret_cast<f32x4*>(p) = v; }
};
template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T vload(const float* p) {
    return *reinterpret_cast<const typename Vec<VEC>::T*>(p);
}

// (A S)_row, columns c .. c+VEC-1: four neighbour rows in flight per lane before the first add.  WT: values[e .. e+3]
// are loaded next to indices[e .. e+3] and each row is multiplied before it is added, in the same order (weights of
// exactly 1.0 give the unweighted bits).
template <int VEC, bool WT>
__device__ __forceinline__ typename Vec<VEC>::T gather_row(const float* S, long lds, const int* indptr,
                                                           const int* indices, const float* values, int row, int c) {
    typedef typename Vec<VEC>::T T;
    const int beg = indptr[row], end = indptr[row + 1];
    T s0 = Vec<VEC>::zero(), s1 = s0, s2 = s0, s3 = s0;
    int e = beg;
    for (; e + 4 <= end; e += 4) {
        const long j0 = indices[e], j1 = indices[e + 1], j2 = indices[e + 2], j3 = indices[e + 3];
        if constexpr (WT) {
            const float w0 = values[e], w1 = values[e + 1], w2 = values[e + 2], w3 = values[e + 3];
            const T v0 = vload<VEC>(S + j0 * lds + c), v1 = vload<VEC>(S + j1 * lds + c);
            const T v2 = vload<VEC>(S + j2 * lds + c), v3 = vload<VEC>(S + j3 * lds + c);
            s0 += w0 * v0; s1 += w1 * v1; s2 += w2 * v2; s3 += w3 * v3;
        } else {
            const T v0 = vload<VEC>(S + j0 * lds + c), v1 = vload<VEC>(S + j1 * lds + c);
            const T v2 = vload<VEC>(S + j2 * lds + c), v3 = vload<VEC>(S + j3 * lds + c);
            s0 += v0; s1 += v1; s2 += v2; s3 += v3;
        }
    }
    for (; e < end; ++e) {
        if constexpr (WT) s0 += values[e] * vload<VEC>(S + (long)indices[e] * lds + c);
        else s0 += vload<VEC>(S + (long)indices[e] * lds + c);
    }
    return (s0 + s1) + (s2 + s3);
}

struct PoolFwdArgs {
    const float* S;
    const float* Z;
    const int* indptr;
    const int* indices;
    float* part;            // [nslab][K][K+D]
    int lds, ldz, n, K, D, rows_per_slab;
    const int* tab;         // batch: slab table {first row, end row, graph, 0} per slab (rows global); null: one graph
    const float* values;    // weighted kernels: fp32 [nnz] in the order of indices (behind the unweighted fields)
};

// MI / NI: 16x16 MFMA tiles per wave along the K result rows / the 64 output columns; WM waves along the rows
// (4 / WM along the columns).  TM = WM * MI * 16 >= K covers every result row, so A S is gathered once per column.
template <int MI, int NI, int WM, int VEC, bool WT>
__device__ __forceinline__ void csr_pool_fwd_body(const PoolFwdArgs& a) {
    constexpr int WN = 4 / WM;
    constexpr int TM = WM * MI * 16;
    static_assert(WN * NI * 16 == FWD_TN, "the column tile is 64 wide");
    constexpr int SP = TM + 16;        // LDS row strides = 16 mod 32: the two 16-lane k rows of an operand read
    constexpr int BP = FWD_TN + 16;    //   land on disjoint bank halves
    __shared__ __attribute__((aligned(16))) float Simg[FWD_ROWS * SP];
    __shared__ __attribute__((aligned(16))) float Bimg[FWD_ROWS * BP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    const int n0 = blockIdx.x * FWD_TN;
    const int KD = a.K + a.D;
    int rbeg = blockIdx.y * a.rows_per_slab;
    int rend = min(a.n, rbeg + a.rows_per_slab);
    if (a.tab) {                                      // a slab of the batch: never crosses a graph boundary
        rbeg = a.tab[blockIdx.y * 4];
        rend = a.tab[blockIdx.y * 4 + 1];
    }
    const long lds = a.lds, ldz = a.ldz;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // gather lanes: LPR lanes x VEC columns span the 64-column tile; a wave fills VEC rows per pass
    constexpr int LPR = FWD_TN / VEC;
    const int gcol = n0 + (lane % LPR) * VEC;
    const int grow = lane / LPR;
    for (int r0 = rbeg; r0 < rend; r0 += FWD_ROWS) {
        if (r0 != rbeg) __syncthreads();              // the previous stage's MFMA reads are done
        // S_stage [32 x TM] (zero past K and past the slab)
        constexpr int SV = TM / VEC;
#pragma unroll 4
        for (int idx = tid; idx < FWD_ROWS * SV; idx += 256) {
            const int r = idx / SV, m = (idx % SV) * VEC;
            typename Vec<VEC>::T v = Vec<VEC>::zero();
            if (r0 + r < rend && m < a.K) v = vload<VEC>(a.S + (long)(r0 + r) * lds + m);
            Vec<VEC>::put(&Simg[r * SP + m], v);
        }
        // [A S | Z]_stage, this tile's 64 columns
        for (int r = wave * VEC + grow; r < FWD_ROWS; r += 4 * VEC) {
            const int row = r0 + r;
            typename Vec<VEC>::T v = Vec<VEC>::zero();
            if (row < rend) {
                if (gcol < a.K) v = gather_row<VEC, WT>(a.S, lds, a.indptr, a.indices, a.values, row, gcol);
                else if (gcol < KD) v = vload<VEC>(a.Z + (long)row * ldz + (gcol - a.K));
            }
            Vec<VEC>::put(&Bimg[r * BP + (lane % LPR) * VEC], v);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FWD_ROWS; kk += 4) {
            float af[MI], bf[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = Simg[(kk + l4) * SP + wm * MI * 16 + i * 16 + l15];
#pragma unroll
            for (int j = 0; j < NI; ++j) bf[j] = Bimg[(kk + l4) * BP + wn * NI * 16 + j * 16 + l15];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // this slab's partial: C/D map of the 16x16 tile, col = lane & 15, row = (lane >> 4) * 4 + reg
    float* P = a.part + (long)blockIdx.y * a.K * KD;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = n0 + wn * NI * 16 + j * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = wm * MI * 16 + i * 16 + l4 * 4 + r;
                if (m < a.K && col < KD) P[(long)m * KD + col] = acc[i][j][r];
            }
        }
}

// the 0/1 kernel and the weighted one (values[e] multiplies neighbour row e): one body, two names
template <int MI, int NI, int WM, int VEC>
__global__ __launch_bounds__(256) void k_csr_pool_fwd(PoolFwdArgs a) {
    csr_pool_fwd_body<MI, NI, WM, VEC, false>(a);
}
template <int MI, int NI, int WM, int VEC>
__global__ __launch_bounds__(256) void k_csr_pool_fwd_w(PoolFwdArgs a) {
    csr_pool_fwd_body<MI, NI, WM, VEC, true>(a);
}

// [Ap | Xp] = sum over slabs of the partials, in slab order.  A workgroup sums 64 entries: wave w takes the slabs
// w, w + 4, ... and the four wave sums are added in wave order (a fixed tree: deterministic).
// Batch (slab_off != null): blockIdx.y is the graph, its slabs are slab_off[b] .. slab_off[b + 1] - 1 — the same tree
// per graph, so a graph's result has the bits of a single-graph call.
__global__ __launch_bounds__(256) void k_csr_pool_reduce(const float* part, int nslab, int K, int D, float* Xp,
                                                         float* Ap, const int* slab_off) {
    __shared__ float red[4][64];
    const int KD = K + D;
    const long total = (long)K * KD;
    const long e = (long)blockIdx.x * 64 + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    int s0 = 0, s1 = nslab;
    if (slab_off) {
        s0 = slab_off[blockIdx.y];
        s1 = slab_off[blockIdx.y + 1];
        Xp += (long)blockIdx.y * K * D;
        Ap += (long)blockIdx.y * K * K;
    }
    float s = 0.f;
    if (e < total) {
#pragma unroll 4
        for (int sl = s0 + wave; sl < s1; sl += 4) s += part[(long)sl * total + e];
    }
    red[wave][threadIdx.x & 63] = s;
    __syncthreads();
    if (wave != 0 || e >= total) return;
    const int l = threadIdx.x;
    const float v = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
    const int m = (int)(e / KD), c = (int)(e % KD);
    if (c < K) Ap[(long)m * K + c] = v;
    else Xp[(long)m * D + (c - K)] = v;
}

// Backward prologue: Wcat [KXp x WLD] and dXpP [Kp x Dp], zero-padded row-major copies the main kernel copies into LDS
// with 16-byte loads.  KX = K + D (undirected) or 2K + D.  blockIdx.y is the graph of a batch (its own dXp / dAp and
// its own copies).
__global__ __launch_bounds__(256) void k_csr_pool_bwd_prep(const float* dXp, const float* dAp, float* W, int KXp,
                                                           int WLD, float* dXpP, int Kp, int Dp, int K, int D,
                                                           int directed) {
    const long nw = (long)KXp * WLD, total = nw + (long)Kp * Dp;
    dXp += (long)blockIdx.y * K * D;
    dAp += (long)blockIdx.y * K * K;
    W += (long)blockIdx.y * nw;
    dXpP += (long)blockIdx.y * Kp * Dp;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e < nw) {
            const int k = (int)(e / WLD), c = (int)(e % WLD);
            float v = 0.f;
            if (c < K) {
                if (k < K) v = directed ? dAp[(long)c * K + k] : dAp[(long)c * K + k] + dAp[(long)k * K + c];
                else if (directed && k < 2 * K) v = dAp[(long)(k - K) * K + c];
                else if (k - (directed ? 2 * K : K) < D) v = dXp[(long)c * D + (k - (directed ? 2 * K : K))];
            }
            W[e] = v;
        } else {
            const long f = e - nw;
            const int k = (int)(f / Dp), c = (int)(f % Dp);
            dXpP[f] = (k < K && c < D) ? dXp[(long)k * D + c] : 0.f;
        }
    }
}

struct PoolBwdArgs {
    const float* S;
    const float* Z;
    const int* indptr;
    const int* indices;
    const int* indptr_t;
    const int* indices_t;
    const float* W;         // Wcat [KXp x WLD]
    const float* dXpP;      // [Kp x Dp]
    float* dS;
    float* dZ;
    int lds, ldz, ldds, lddz, n, K, D, KX, KXp, Kp, Dp, directed;
    const int* tab;         // batch: row-block table {first row, end row, graph, 0} (rows global); null: one graph
    const float* values;    // weighted kernels: fp32 [nnz] in the order of indices / of indices_t (behind the
    const float* values_t;  //   unweighted fields)
};

// NI: 16-column MFMA tiles per wave (NI * 16 >= K; also the dZ column block).  Wave w owns rows 16w .. 16w + 15 of the
// workgroup's 64 and every output column of the block.
template <int NI, int VEC, bool WT>
__device__ __forceinline__ void csr_pool_bwd_body(const PoolBwdArgs& a) {
    constexpr int TN = NI * 16;
    constexpr int XP = BWD_KC + 4;     // A image [64 rows][XP]: 16-byte rows for the gather's vector stores
    constexpr int WP = TN + 16;        // B image [32 k][WP]: = 16 mod 32
    __shared__ __attribute__((aligned(16))) float Ximg[BWD_ROWS * XP];
    __shared__ __attribute__((aligned(16))) float Wimg[BWD_KC * WP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    int row0 = blockIdx.x * BWD_ROWS, rend = a.n;
    const float* Wg = a.W;
    const float* dXg = a.dXpP;
    if (a.tab) {                                      // a row block of the batch: rows of one graph, its own Wcat / dXp
        row0 = a.tab[blockIdx.x * 4];
        rend = a.tab[blockIdx.x * 4 + 1];
        const long g = a.tab[blockIdx.x * 4 + 2];
        Wg += g * a.KXp * TN;
        dXg += g * a.Kp * a.Dp;
    }
    const long lds = a.lds, ldz = a.ldz;
    const int koff = a.directed ? 2 * a.K : a.K;      // first X column of Z

    f32x4 acc[NI];
    auto mfma_chunk = [&]() {
#pragma unroll
        for (int kk = 0; kk < BWD_KC; kk += 4) {
            const float af = Ximg[(wave * 16 + l15) * XP + kk + l4];
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Wimg[(kk + l4) * WP + j * 16 + l15], acc[j], 0, 0, 0);
        }
    };
    // B chunk: rows k0 .. k0 + 31 of a zero-padded [rows x ld] matrix, columns c0 .. c0 + TN - 1
    auto fill_b = [&](const float* B, long ld, int k0, int c0) {
        constexpr int BV = TN / 4;
#pragma unroll 4
        for (int idx = tid; idx < BWD_KC * BV; idx += 256) {
            const int k = idx / BV, c = (idx % BV) * 4;
            *reinterpret_cast<f32x4*>(&Wimg[k * WP + c]) = *reinterpret_cast<const f32x4*>(B + (long)(k0 + k) * ld + c0 + c);
        }
    };
    // A-chunk lanes: LPR lanes x VEC columns span the 32 columns; a wave fills 64 / LPR rows per pass
    constexpr int LPR = BWD_KC / VEC;
    constexpr int RPP = 64 / LPR;
    const int ac = (lane % LPR) * VEC;

    // ---- phase 1: dS = X Wcat
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < a.KXp; c0 += BWD_KC) {
        if (c0) __syncthreads();
        const int c = c0 + ac;
        for (int r = wave * 16 + lane / LPR; r < wave * 16 + 16; r += RPP) {
            const int row = row0 + r;
            typename Vec<VEC>::T v = Vec<VEC>::zero();
            if (row < rend) {
                if (c < a.K) v = gather_row<VEC, WT>(a.S, lds, a.indptr, a.indices, a.values, row, c);
                else if (c < koff) v = gather_row<VEC, WT>(a.S, lds, a.indptr_t, a.indices_t, a.values_t, row, c - a.K);
                else if (c < a.KX) v = vload<VEC>(a.Z + (long)row * ldz + (c - koff));
            }
            Vec<VEC>::put(&Ximg[r * XP + ac], v);
        }
        fill_b(Wg, TN, c0, 0);
        __syncthreads();
        mfma_chunk();
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int col = j * 16 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + l4 * 4 + r;
            if (row < rend && col < a.K) a.dS[(long)row * a.ldds + col] = acc[j][r];
        }
    }

    // ---- phase 2: dZ += S dXp, TN columns at a time
    for (int nb = 0; nb < a.D; nb += TN) {
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < a.Kp; c0 += BWD_KC) {
            __syncthreads();
            const int c = c0 + ac;
            for (int r = wave * 16 + lane / LPR; r < wave * 16 + 16; r += RPP) {
                const int row = row0 + r;
                typename Vec<VEC>::T v = Vec<VEC>::zero();
                if (row < rend && c < a.K) v = vload<VEC>(a.S + (long)row * lds + c);
                Vec<VEC>::put(&Ximg[r * XP + ac], v);
            }
            fill_b(dXg, a.Dp, c0, nb);
            __syncthreads();
            mfma_chunk();
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = nb + j * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wave * 16 + l4 * 4 + r;
                if (row < rend && col < a.D) {
                    float* p = a.dZ + (long)row * a.lddz + col;
                    *p = *p + acc[j][r];
                }
            }
        }
    }
}

template <int NI, int VEC>
__global__ __launch_bounds__(256) void k_csr_pool_bwd(PoolBwdArgs a) {
    csr_pool_bwd_body<NI, VEC, false>(a);
}
template <int NI, int VEC>
__global__ __launch_bounds__(256) void k_csr_pool_bwd_w(PoolBwdArgs a) {
    csr_pool_bwd_body<NI, VEC, true>(a);
}

// slab partition of the forward: >= FWD_TARGET_WGS workgroups when the rows allow, slabs a multiple of the stage
void fwd_slabs(int n, int K, int D, int* nslab, int* rows_per_slab) {
    const int ntn = cdiv(K + D, FWD_TN);
    int want = cdiv(FWD_TARGET_WGS, ntn);
    want = std::max(1, std::min(want, cdiv(n, FWD_MIN_SLAB)));
    const int rows = cdiv(cdiv(n, want), FWD_ROWS) * FWD_ROWS;
    *rows_per_slab = rows;
    *nslab = cdiv(n, rows);
}
int bwd_ni(int K) { return K <= 64 ? 4 : (K <= 128 ? 8 : 16); }

// tab / slab_off / nslab_batch / B: the slab table of a batch (dp_csr_pool_batch_plan); null / 0: one graph of n rows
void csr_pool_fwd_seq(Seq& q, const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      float* Xp, float* Ap, int n, int K, int D, const int* tab = nullptr,
                      const int* slab_off = nullptr, int nslab_batch = 0, int B = 1, const float* values = nullptr) {
    int nslab, rows;
    fwd_slabs(n, K, D, &nslab, &rows);
    if (nslab_batch) nslab = nslab_batch;
    float* part = q.alloc<float>((size_t)nslab * K * (K + D));
    if (!q.ok()) return;
    const bool v4 = K % 4 == 0 && D % 4 == 0 && lds % 4 == 0 && ldz % 4 == 0 && aligned16(S) && aligned16(Z);
    PoolFwdArgs a{S, Z, indptr, indices, part, lds, ldz, n, K, D, rows, tab, values};
    const dim3 grid(cdiv(K + D, FWD_TN), nslab);
#define DP_POOL_FWD_(KERNEL, MI, NI, WM)                                                       \
    do {                                                                                       \
        if (v4) hipLaunchKernelGGL((KERNEL<MI, NI, WM, 4>), grid, dim3(256), 0, q.stream, a); \
        else hipLaunchKernelGGL((KERNEL<MI, NI, WM, 1>), grid, dim3(256), 0, q.stream, a);    \
    } while (0)
#define DP_POOL_FWD(MI, NI, WM)                                  \
    do {                                                         \
        if (values) DP_POOL_FWD_(k_csr_pool_fwd_w, MI, NI, WM);  \
        else DP_POOL_FWD_(k_csr_pool_fwd, MI, NI, WM);           \
    } while (0)
    if (K <= 64) DP_POOL_FWD(2, 2, 2);
    else if (K <= 128) DP_POOL_FWD(4, 2, 2);
    else DP_POOL_FWD(4, 4, 4);
#undef DP_POOL_FWD
#undef DP_POOL_FWD_
    q.check_launch("csr_pool_fwd");
    hipLaunchKernelGGL(k_csr_pool_reduce, dim3(cdiv((long)K * (K + D), 64), B), dim3(256), 0, q.stream, part, nslab, K,
                       D, Xp, Ap, slab_off);
    q.check_launch("csr_pool_reduce");
}

void csr_pool_bwd_seq(Seq& q, const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      const int* indptr_t, const int* indices_t, const float* dXp, const float* dAp, float* dS,
                      int ldds, float* dZ, int lddz, int n, int K, int D, const int* tab = nullptr, int nblk_batch = 0,
                      int B = 1, const float* values = nullptr, const float* values_t = nullptr) {
    const int directed = (indptr_t != indptr || indices_t != indices) ? 1 : 0;
    const int NI = bwd_ni(K), TN = NI * 16;
    const int KX = (directed ? 2 * K : K) + D;
    const int KXp = cdiv(KX, BWD_KC) * BWD_KC, Kp = cdiv(K, BWD_KC) * BWD_KC, Dp = cdiv(D, TN) * TN;
    float* W = q.alloc<float>((size_t)B * KXp * TN);
    float* dXpP = q.alloc<float>((size_t)B * Kp * Dp);
    if (!q.ok()) return;
    const long prep = (long)KXp * TN + (long)Kp * Dp;
    hipLaunchKernelGGL(k_csr_pool_bwd_prep, dim3(std::min(cdiv(prep, 256), 1024), B), dim3(256), 0, q.stream, dXp, dAp, W,
                       KXp, TN, dXpP, Kp, Dp, K, D, directed);
    q.check_launch("csr_pool_bwd_prep");
    const bool v4 = K % 4 == 0 && D % 4 == 0 && lds % 4 == 0 && ldz % 4 == 0 && aligned16(S) && aligned16(Z);
    PoolBwdArgs a{S, Z, indptr, indices, indptr_t, indices_t, W, dXpP, dS, dZ, lds, ldz, ldds, lddz, n, K, D, KX, KXp,
                  Kp, Dp, directed, tab, values, values_t};
    const dim3 grid(nblk_batch ? nblk_batch : cdiv(n, BWD_ROWS));
#define DP_POOL_BWD_(KERNEL, NI_)                                                      \
    do {                                                                               \
        if (v4) hipLaunchKernelGGL((KERNEL<NI_, 4>), grid, dim3(256), 0, q.stream, a); \
        else hipLaunchKernelGGL((KERNEL<NI_, 1>), grid, dim3(256), 0, q.stream, a);    \
    } while (0)
#define DP_POOL_BWD(NI_)                                   \
    do {                                                   \
        if (values) DP_POOL_BWD_(k_csr_pool_bwd_w, NI_);   \
        else DP_POOL_BWD_(k_csr_pool_bwd, NI_);            \
    } while (0)
    if (NI == 4) DP_POOL_BWD(4);
    else if (NI == 8) DP_POOL_BWD(8);
    else DP_POOL_BWD(16);
#undef DP_POOL_BWD
#undef DP_POOL_BWD_
    q.check_launch("csr_pool_bwd");
}

size_t sized_bytes(int n, int K, int D) {
    Seq q = Seq::sizing();
    csr_pool_fwd_seq(q, nullptr, K, nullptr, D, nullptr, nullptr, nullptr, nullptr, n, K, D);
    const size_t f = q.ws_off;
    Seq b = Seq::sizing();
    csr_pool_bwd_seq(b, nullptr, K, nullptr, D, nullptr, nullptr, (const int*)1, nullptr, nullptr, nullptr, nullptr, K,
                     nullptr, D, n, K, D);
    return std::max(f, b.ws_off);
}

// Slab / row-block tables of a batch, on the host: graph b keeps the partition fwd_slabs(n_b) and the 64-row backward
// blocks a single-graph call would use, shifted to its first row.  Null tables: count only.
void batch_plan(const int* off, int B, int K, int D, int* ftab, int* soff, int* btab, int* counts) {
    int ns = 0, nb = 0;
    for (int b = 0; b < B; ++b) {
        const int n = off[b + 1] - off[b];
        int s, rows;
        fwd_slabs(n, K, D, &s, &rows);
        if (soff) soff[b] = ns;
        for (int i = 0; i < s; ++i, ++ns)
            if (ftab) {
                ftab[4 * ns] = off[b] + i * rows;
                ftab[4 * ns + 1] = std::min(off[b + 1], off[b] + (i + 1) * rows);
                ftab[4 * ns + 2] = b;
                ftab[4 * ns + 3] = 0;
            }
        for (int r = 0; r < n; r += BWD_ROWS, ++nb)
            if (btab) {
                btab[4 * nb] = off[b] + r;
                btab[4 * nb + 1] = std::min(off[b + 1], off[b] + r + BWD_ROWS);
                btab[4 * nb + 2] = b;
                btab[4 * nb + 3] = 0;
            }
    }
    if (soff) soff[B] = ns;
    counts[0] = ns;
    counts[1] = nb;
}

size_t batch_sized_bytes(int nslab, int B, int K, int D) {
    const size_t f = align256((size_t)nslab * K * (K + D) * sizeof(float));
    const int TN = bwd_ni(K) * 16;
    const int KXp = cdiv(2 * K + D, BWD_KC) * BWD_KC, Kp = cdiv(K, BWD_KC) * BWD_KC, Dp = cdiv(D, TN) * TN;
    const size_t b = align256((size_t)B * KXp * TN * sizeof(float)) + align256((size_t)B * Kp * Dp * sizeof(float));
    return std::max(f, b);
}

}  // namespace
}  // namespace dp

using namespace dp;

namespace {

// the tables of a batch (dp_csr_pool_batch_plan); a null PoolBatch: one graph of n rows
struct PoolBatch {
    const int* tab;         // forward: slab table; backward: row-block table
    const int* slab_off;    // forward only
    int count;              // slabs / row blocks
    int B;
};

int check_shape(const char* entry, int n, int K, int D, int lds, int ldz) {
    DP_CHECK(n > 0, DP_ERR_INVALID_ARG, "%s: n=%d must be positive", entry, n);
    DP_CHECK(K >= 1 && K <= 256, DP_ERR_UNSUPPORTED, "%s: K=%d outside the supported 1..256", entry, K);
    DP_CHECK(D >= 1 && D <= 512, DP_ERR_UNSUPPORTED, "%s: D=%d outside the supported 1..512", entry, D);
    DP_CHECK(lds >= K && ldz >= D, DP_ERR_INVALID_ARG, "%s: lds=%d / ldz=%d smaller than K=%d / D=%d", entry, lds, ldz,
             K, D);
    return DP_OK;
}

// The checked bodies of all eight entries; bt: the batch entries' tables, null from the single-graph ones (n: n_total
// of a batch).
int pool_fwd_entry(const char* entry, const float* S, int lds, const float* Z, int ldz, const int* indptr,
                   const int* indices, const float* values, bool weighted, const PoolBatch* bt, float* Xp, float* Ap,
                   int n, int K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    const int* fwd_tab = bt ? bt->tab : nullptr;
    const int* slab_off = bt ? bt->slab_off : nullptr;
    DP_NOTNULL(S); DP_NOTNULL(Z); DP_NOTNULL(indptr); DP_NOTNULL(indices);
    if (bt) { DP_NOTNULL(fwd_tab); DP_NOTNULL(slab_off); }
    DP_NOTNULL(Xp); DP_NOTNULL(Ap);
    DP_VALUES(DP_ALIGNED4(values), "%s: values is NULL", entry);
    DP_ALIGNED4(S); DP_ALIGNED4(Z); DP_ALIGNED4(indptr); DP_ALIGNED4(indices); DP_ALIGNED4(fwd_tab);
    DP_ALIGNED4(slab_off); DP_ALIGNED4(Xp); DP_ALIGNED4(Ap);
    if (int rc = check_shape(entry, n, K, D, lds, ldz)) return rc;
    if (bt)
        DP_CHECK(bt->B >= 1 && bt->B <= 65535 && bt->count >= bt->B && bt->count <= 65535, DP_ERR_INVALID_ARG,
                 "%s: B=%d / n_slabs=%d outside 1..65535 (every graph has a slab)", entry, bt->B, bt->count);
    DP_ALIGNED16(workspace, true, "%s: workspace is not 16-byte aligned", entry);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    csr_pool_fwd_seq(q, S, lds, Z, ldz, indptr, indices, Xp, Ap, n, K, D, fwd_tab, slab_off, bt ? bt->count : 0,
                     bt ? bt->B : 1, weighted ? values : nullptr);
    return q.err;
}

int pool_bwd_entry(const char* entry, const float* S, int lds, const float* Z, int ldz, const int* indptr,
                   const int* indices, const float* values, const int* indptr_t, const int* indices_t,
                   const float* values_t, bool weighted, const PoolBatch* bt, const float* dXp, const float* dAp,
                   float* dS, int ldds, float* dZ, int lddz, int n, int K, int D, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const int* bwd_tab = bt ? bt->tab : nullptr;
    DP_NOTNULL(S); DP_NOTNULL(Z); DP_NOTNULL(indptr); DP_NOTNULL(indices); DP_NOTNULL(indptr_t); DP_NOTNULL(indices_t);
    if (bt) DP_NOTNULL(bwd_tab);
    DP_NOTNULL(dXp); DP_NOTNULL(dAp); DP_NOTNULL(dS); DP_NOTNULL(dZ);
    DP_VALUES(DP_ALIGNED4(values), "%s: values is NULL", entry);
    DP_VALUES_T(DP_ALIGNED4(values_t), "%s: values_t is NULL but indices_t is a CSR of its own", entry);
    DP_ALIGNED4(S); DP_ALIGNED4(Z); DP_ALIGNED4(indptr); DP_ALIGNED4(indices); DP_ALIGNED4(indptr_t);
    DP_ALIGNED4(indices_t); DP_ALIGNED4(bwd_tab); DP_ALIGNED4(dXp); DP_ALIGNED4(dAp); DP_ALIGNED4(dS); DP_ALIGNED4(dZ);
    if (int rc = check_shape(entry, n, K, D, lds, ldz)) return rc;
    DP_CHECK(ldds >= K && lddz >= D, DP_ERR_INVALID_ARG, "%s: ldds=%d / lddz=%d smaller than K=%d / D=%d", entry, ldds,
             lddz, K, D);
    if (bt)
        DP_CHECK(bt->B >= 1 && bt->B <= 65535 && bt->count >= bt->B, DP_ERR_INVALID_ARG,
                 "%s: B=%d / n_blocks=%d (every graph has a row block)", entry, bt->B, bt->count);
    DP_ALIGNED16(workspace, true, "%s: workspace is not 16-byte aligned", entry);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    csr_pool_bwd_seq(q, S, lds, Z, ldz, indptr, indices, indptr_t, indices_t, dXp, dAp, dS, ldds, dZ, lddz, n, K, D,
                     bwd_tab, bt ? bt->count : 0, bt ? bt->B : 1, weighted ? values : nullptr,
                     weighted ? values_t_of(indices, indices_t, values, values_t) : nullptr);
    return q.err;
}

}  // namespace

extern "C" {

size_t dp_csr_pool_workspace_bytes(int n, int K, int D) {
    if (n <= 0 || K < 1 || K > 256 || D < 1 || D > 512) return 0;
    return sized_bytes(n, K, D);
}

int dp_csr_pool_fwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices, float* Xp,
                    float* Ap, int n, int K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    return pool_fwd_entry("dp_csr_pool_fwd", S, lds, Z, ldz, indptr, indices, nullptr, false, nullptr, Xp, Ap, n, K, D,
                          workspace, workspace_bytes, stream);
}
int dp_csr_pool_fwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      const float* values, float* Xp, float* Ap, int n, int K, int D, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return pool_fwd_entry("dp_csr_pool_fwd_w", S, lds, Z, ldz, indptr, indices, values, true, nullptr, Xp, Ap, n, K, D,
                          workspace, workspace_bytes, stream);
}

int dp_csr_pool_bwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                    const int* indptr_t, const int* indices_t, const float* dXp, const float* dAp, float* dS, int ldds,
                    float* dZ, int lddz, int n, int K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    return pool_bwd_entry("dp_csr_pool_bwd", S, lds, Z, ldz, indptr, indices, nullptr, indptr_t, indices_t, nullptr,
                          false, nullptr, dXp, dAp, dS, ldds, dZ, lddz, n, K, D, workspace, workspace_bytes, stream);
}
int dp_csr_pool_bwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                      const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                      const float* dXp, const float* dAp, float* dS, int ldds, float* dZ, int lddz, int n, int K, int D,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return pool_bwd_entry("dp_csr_pool_bwd_w", S, lds, Z, ldz, indptr, indices, values, indptr_t, indices_t, values_t,
                          true, nullptr, dXp, dAp, dS, ldds, dZ, lddz, n, K, D, workspace, workspace_bytes, stream);
}

// ---- the same on a ragged batch of B graphs (rows concatenated, block-diagonal CSR with GLOBAL column indices)
int dp_csr_pool_batch_plan(const int* node_off_host, int B, int K, int D, int* fwd_tab_host, int* slab_off_host,
                           int* bwd_tab_host, int* counts_host) {
    DP_NOTNULL(node_off_host); DP_NOTNULL(counts_host);
    DP_CHECK(B >= 1, DP_ERR_INVALID_ARG, "dp_csr_pool_batch_plan: B=%d must be positive", B);
    DP_CHECK(K >= 1 && K <= 256 && D >= 1 && D <= 512, DP_ERR_UNSUPPORTED,
             "dp_csr_pool_batch_plan: K=%d / D=%d outside the supported 1..256 / 1..512", K, D);
    DP_CHECK(node_off_host[0] == 0, DP_ERR_INVALID_ARG, "dp_csr_pool_batch_plan: node_off[0] must be 0");
    for (int b = 0; b < B; ++b)
        DP_CHECK(node_off_host[b + 1] > node_off_host[b], DP_ERR_INVALID_ARG,
                 "dp_csr_pool_batch_plan: graph %d has no node (node_off must increase)", b);
    batch_plan(node_off_host, B, K, D, fwd_tab_host, slab_off_host, bwd_tab_host, counts_host);
    return DP_OK;
}

size_t dp_csr_pool_batch_workspace_bytes(int n_slabs, int B, int K, int D) {
    if (n_slabs < 1 || B < 1 || K < 1 || K > 256 || D < 1 || D > 512) return 0;
    return batch_sized_bytes(n_slabs, B, K, D);
}

int dp_csr_pool_batch_fwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                          const int* fwd_tab, const int* slab_off, int n_slabs, float* Xp, float* Ap, int B,
                          int n_total, int K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    const PoolBatch bt{fwd_tab, slab_off, n_slabs, B};
    return pool_fwd_entry("dp_csr_pool_batch_fwd", S, lds, Z, ldz, indptr, indices, nullptr, false, &bt, Xp, Ap,
                          n_total, K, D, workspace, workspace_bytes, stream);
}
int dp_csr_pool_batch_fwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                            const float* values, const int* fwd_tab, const int* slab_off, int n_slabs, float* Xp,
                            float* Ap, int B, int n_total, int K, int D, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const PoolBatch bt{fwd_tab, slab_off, n_slabs, B};
    return pool_fwd_entry("dp_csr_pool_batch_fwd_w", S, lds, Z, ldz, indptr, indices, values, true, &bt, Xp, Ap,
                          n_total, K, D, workspace, workspace_bytes, stream);
}

int dp_csr_pool_batch_bwd(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                          const int* indptr_t, const int* indices_t, const int* bwd_tab, int n_blocks,
                          const float* dXp, const float* dAp, float* dS, int ldds, float* dZ, int lddz, int B,
                          int n_total, int K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    const PoolBatch bt{bwd_tab, nullptr, n_blocks, B};
    return pool_bwd_entry("dp_csr_pool_batch_bwd", S, lds, Z, ldz, indptr, indices, nullptr, indptr_t, indices_t,
                          nullptr, false, &bt, dXp, dAp, dS, ldds, dZ, lddz, n_total, K, D, workspace, workspace_bytes,
                          stream);
}
int dp_csr_pool_batch_bwd_w(const float* S, int lds, const float* Z, int ldz, const int* indptr, const int* indices,
                            const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                            const int* bwd_tab, int n_blocks, const float* dXp, const float* dAp, float* dS, int ldds,
                            float* dZ, int lddz, int B, int n_total, int K, int D, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const PoolBatch bt{bwd_tab, nullptr, n_blocks, B};
    return pool_bwd_entry("dp_csr_pool_batch_bwd_w", S, lds, Z, ldz, indptr, indices, values, indptr_t, indices_t,
                          values_t, true, &bt, dXp, dAp, dS, ldds, dZ, lddz, n_total, K, D, workspace, workspace_bytes,
                          stream);
}

}  // extern "C"
