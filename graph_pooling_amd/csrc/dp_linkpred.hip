// Link-prediction auxiliary loss of DiffPool (SoftPoolingGcnEncoder.loss, encoders.py:1309-1331):
//   P = min(S S^T, 1);  l = -A log(P + eps) - (1 - A) log(1 - P + eps), eps = 1e-7;
//   zero outside the n_b x n_b block; loss = sum(l) / sum_b n_b^2.
//
// The reference materialises ~10 [B,N,N] fp32 temporaries for this (80 % of its CPU step).  Here
// nothing of size N^2 is ever written:
//   forward : one workgroup per 64x64 tile of one graph forms P_tile = S_r S_c^T on the fp32 MFMA from two
//             S row-blocks staged in LDS, reads the A tile once, and reduces the loss terms with wave shuffles
//             to one partial per workgroup (tiles outside the n_b x n_b block exit immediately);
//   backward: one workgroup per 64-row block of dS walks the column tiles, RECOMPUTES each P tile, forms
//             E = dl/dP(r,c) + dl/dP(c,r) (the A^T tile comes through LDS so both reads are coalesced) and
//             accumulates dS_r += E S_c on the MFMA — dS = (D + D^T) S without ever storing D.
// Both kernels are written once over an adjacency reader: the dense fp32 batch, or the packed bf16 rows of A and A^T
// that dp_adj_pack / dp_build_batch_packed write (the captured training step holds nothing else).  The tile walk is
// the same for both, so on a bf16-exact (0/1) adjacency the two give bit-identical loss and dS.
#include "dp_link_tiles.h"      // lk_stage / lk_ptile / lk_block_sum / lk_kt, shared with dp_csr_linkpred.hip

namespace dp {

// ------------------------------------------------------------------ adjacency readers
// graph(b, n) is the reader of graph b; get() returns the raw element (clamped indices only) and value() decodes it at
// its use, so the wait for a load sits where the value is needed.  The backward's tiles at column offset c0 of row
// block r0 (CW columns):
//   rows : A[r0 + i][c0 + j], fetched into registers and put into the LDS image Ar [64][CW + 4] (as fp32);
//   cols : A[c0 + j][r0 + i]; put_cols() keeps the fetched tile (an LDS image, or the lane's own registers, since the
//          next tile's fetch overwrites `at`) and col_value() returns the value at MFMA fragment position (ri, cj).
struct LkAdjF32 {                     // dense fp32 adj [B, n, n]
    typedef float Raw;
    typedef float RowReg;
    const float* a;
    int ld;                           // row stride: n (set by graph())
    static constexpr bool kColLds = true;                  // A^T tile: column reads transposed through LDS [CW][65]
    template <int CW> static constexpr int row_regs() { return CW / 4; }
    __device__ __forceinline__ static float value(Raw v) { return v; }
    __device__ __forceinline__ LkAdjF32 graph(int b, int n) const { return LkAdjF32{a + (long)b * n * n, n}; }
    __device__ __forceinline__ Raw get(int row, int col) const { return a[(long)row * ld + col]; }
    template <int CW>
    __device__ __forceinline__ void fetch_rows(RowReg* ar, int n, int r0, int c0) const {
#pragma unroll
        for (int m = 0; m < CW / 4; ++m) {
            const int e = threadIdx.x + 256 * m;
            ar[m] = get(min(r0 + e / CW, n - 1), min(c0 + e % CW, n - 1));
        }
    }
    template <int CW, int SA>
    __device__ __forceinline__ static void put_rows(const RowReg* ar, float* Ar) {
#pragma unroll
        for (int m = 0; m < CW / 4; ++m) {
            const int e = threadIdx.x + 256 * m;
            Ar[(e / CW) * SA + e % CW] = ar[m];
        }
    }
    template <int CW, int NJ>
    __device__ __forceinline__ void fetch_cols(Raw* at, int n, int r0, int c0, int, int, int, int) const {
#pragma unroll
        for (int m = 0; m < CW / 4; ++m) {
            const int e = threadIdx.x + 256 * m;
            at[m] = get(min(c0 + (e >> 6), n - 1), min(r0 + (e & 63), n - 1));
        }
    }
    template <int CW>
    __device__ __forceinline__ static void put_cols(const Raw* at, float* At, Raw*) {
#pragma unroll
        for (int m = 0; m < CW / 4; ++m) {
            const int e = threadIdx.x + 256 * m;
            At[(e >> 6) * 65 + (e & 63)] = at[m];
        }
    }
    template <int NJ>
    __device__ __forceinline__ static float col_value(const float* At, const Raw*, int, int, int, int ri, int cj) {
        return At[cj * 65 + ri];
    }
};

struct LkAdjBf16 {                    // packed: bf16 rows pk [B, n, ld] of A, pkt of A^T (pk == pkt: symmetric)
    typedef unsigned Raw;             // one bf16 in the low half
    typedef uint4 RowReg;             // 8 bf16 of one row
    const unsigned short* pk;
    const unsigned short* pkt;
    int ld;                           // adj_pack_ld(n): a multiple of 8, so every 8-column chunk is 16-byte aligned
    static constexpr bool kColLds = false;                 // A^T comes row-wise from pkt: no transposing LDS image
    template <int CW> static constexpr int row_regs() { return CW / 32; }
    __device__ __forceinline__ static float value(Raw v) { return __uint_as_float(v << 16); }   // exact
    __device__ __forceinline__ LkAdjBf16 graph(int b, int n) const {
        return LkAdjBf16{pk + (long)b * n * ld, pkt + (long)b * n * ld, ld};
    }
    __device__ __forceinline__ Raw get(int row, int col) const { return pk[(long)row * ld + col]; }
    // 16-byte loads: chunk q = 8 columns; a chunk past the padded row is clamped to the row's last one — its columns
    // are >= n, so (like the fp32 reader's clamped columns) they only ever meet the nb mask
    template <int CW>
    __device__ __forceinline__ void fetch_rows(RowReg* ar, int n, int r0, int c0) const {
        constexpr int QR = CW / 8;
#pragma unroll
        for (int m = 0; m < CW / 32; ++m) {
            const int q = threadIdx.x + 256 * m;
            const int row = min(r0 + q / QR, n - 1), col = min(c0 + (q % QR) * 8, ld - 8);
            ar[m] = *reinterpret_cast<const uint4*>(pk + (long)row * ld + col);
        }
    }
    template <int CW, int SA>
    __device__ __forceinline__ static void put_rows(const RowReg* ar, float* Ar) {
        constexpr int QR = CW / 8;
#pragma unroll
        for (int m = 0; m < CW / 32; ++m) {
            const int q = threadIdx.x + 256 * m;
            float* d = Ar + (q / QR) * SA + (q % QR) * 8;
            const unsigned w[4] = {ar[m].x, ar[m].y, ar[m].z, ar[m].w};
            float v[8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[2 * t] = __uint_as_float(w[t] << 16);
                v[2 * t + 1] = __uint_as_float(w[t] & 0xffff0000u);
            }
            *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
    // A[c0 + cj][r0 + ri] = A^T[r0 + ri][c0 + cj]: each lane loads its own fragment positions from pkt rows
    // r0..r0+63 (16 lanes read 32 contiguous bytes of a row)
    template <int CW, int NJ>
    __device__ __forceinline__ void fetch_cols(Raw* at, int n, int r0, int c0, int wr, int wc, int l15, int kq) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = min(r0 + wr * 32 + i * 16 + kq * 4 + r, n - 1);
                    const int col = min(c0 + wc * 16 * NJ + j * 16 + l15, n - 1);
                    at[(i * NJ + j) * 4 + r] = pkt[(long)row * ld + col];
                }
    }
    template <int CW>
    __device__ __forceinline__ static void put_cols(const Raw* at, float*, Raw* cur) {
#pragma unroll
        for (int m = 0; m < CW / 4; ++m) cur[m] = at[m];
    }
    template <int NJ>
    __device__ __forceinline__ static float col_value(const float*, const Raw* cur, int i, int j, int r, int, int) {
        return value(cur[(i * NJ + j) * 4 + r]);
    }
};

// ------------------------------------------------------------------ forward
// The A values of a lane sit at its MFMA fragment positions (one column per lane per row), so they are read one
// element per load: 2 bytes each for the packed reader, 16 lanes covering 32 contiguous bytes of a row.
template <int KT, class Adj>
__global__ __launch_bounds__(256) void k_link_fwd(const float* S, int lds_ld, Adj adj, const int* num_nodes,
                                                  int n, int K, int tiles, float* partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int KP = KT * 16 + 2;
    const int b = blockIdx.y;
    const int tr = blockIdx.x / tiles, tc = blockIdx.x % tiles;
    const int nb = num_nodes ? min(num_nodes[b], n) : n;
    const int r0 = tr * 64, c0 = tc * 64;
    if (r0 >= nb || c0 >= nb) {
        if (threadIdx.x == 0) partial[(long)b * gridDim.x + blockIdx.x] = 0.f;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, kq = lane >> 4;
    // the A values this thread needs, issued first (clamped addresses, no branches) so they fly under the staging
    const Adj Ab = adj.graph(b, n);
    typename Adj::Raw av[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = min(r0 + wr * 32 + i * 16 + kq * 4 + r, n - 1);
                const int c = min(c0 + wc * 32 + j * 16 + l15, n - 1);
                av[i][j][r] = Ab.get(row, c);
            }
    float* Sr = lds;
    float* Sc = lds + 64 * KP;
    float* red = Sc + 64 * KP;
    const float* Sb = S + (long)b * n * lds_ld;
    lk_stage<KT, 64>(Sb, lds_ld, r0, n, K, Sr);
    lk_stage<KT, 64>(Sb, lds_ld, c0, n, K, Sc);
    __syncthreads();
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
                const float a = Adj::value(av[i][j][r]);
                const float l = -a * logf(pv + LINK_EPS) - (1.f - a) * logf(1.f - pv + LINK_EPS);
                sum += (row < nb && c < nb) ? l : 0.f;
            }
        }
    const float s = lk_block_sum(sum, red);
    if (threadIdx.x == 0) partial[(long)b * gridDim.x + blockIdx.x] = s;
}

// loss = sum(partials) / sum_b n_b^2  (single block; deterministic);  also the backward scale dloss / sum n_b^2
// norm (optional device scalar) replaces the local sum_b n_b^2: data-parallel ranks pass (global sum) / world so that
// the mean of the per-rank losses and gradients equals the single-batch loss of encoders.py:1326,1331
__global__ __launch_bounds__(256) void k_link_final(const float* partial, int count, const int* num_nodes, int B,
                                                    int n, float* out, float* scale_out, const float* dloss,
                                                    const float* norm) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) acc += partial ? partial[i] : 0.f;
    const float s = lk_block_sum(acc, red);
    if (threadIdx.x == 0) {
        double nn = 0.0;
        for (int b = 0; b < B; ++b) {
            const double v = num_nodes ? (double)min(num_nodes[b], n) : (double)n;
            nn += v * v;
        }
        if (norm) nn = (double)norm[0];
        if (out) out[0] = (float)((double)s / nn);
        if (scale_out) scale_out[0] = (float)((dloss ? (double)dloss[0] : 1.0) / nn);
    }
}

// ------------------------------------------------------------------ backward
// d l / d P at (a, p_raw); torch.min(a, b) backward: full gradient where a < b, half on ties, none above
__device__ inline float lk_dldp(float av, float raw) {
    const float pv = fminf(raw, 1.f);
    const float gate = raw < 1.f ? 1.f : (raw == 1.f ? 0.5f : 0.f);
    return gate * (-av / (pv + LINK_EPS) + (1.f - av) / (1.f - pv + LINK_EPS));
}

// KT = ceil(K / 16) output column tiles per row block; the column tiles walked are CW = 32 NJ wide.
// The next column tile's S rows and both A tiles are fetched into registers while the current one is computed on.
template <int KT, int NJ, class Adj>
__global__ __launch_bounds__(256) void k_link_bwd(const float* S, int lds_ld, Adj adj, const int* num_nodes,
                                                  const float* scale_ptr, float* dS, int ldds, int n, int K,
                                                  int accumulate, float* part, int split_tiles) {
    // part != null: blockIdx.z walks only `split_tiles` column tiles and stores its partial row block to
    // part[z][b][row][K]; k_link_reduce sums the splits in a fixed order (small batches: 160 workgroups walking 8
    // tiles each left most of the chip idle)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CW = 32 * NJ, KW = KT * 16, KP = KW + 2;
    constexpr int SA = CW + 4;      // E / A tile row stride: 4 SA = 16 mod 32, so (4 kq + r) rows x 16 cols spread over banks
    constexpr int NS = CW * KW / 256, NA = CW / 4, NR = Adj::template row_regs<CW>();
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * 64;
    const int nb = num_nodes ? min(num_nodes[b], n) : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, kq = lane >> 4;
    float* dSb = dS + (long)b * n * ldds;
    if (r0 >= nb) {                                   // rows outside the graph: gradient is zero
        if (part) return;                             // (the reduce pass writes those zeros)
        if (!accumulate)
            for (int e = threadIdx.x; e < 64 * KW; e += 256) {
                const int i = e / KW, k = e % KW;
                if (r0 + i < n && k < K) dSb[(long)(r0 + i) * ldds + k] = 0.f;
            }
        return;
    }
    float* Sr = lds;                 // [64][KP]
    float* Sc = Sr + 64 * KP;        // [CW][KP]
    float* Ar = Sc + CW * KP;        // [64][SA]   A[r0 + i][c0 + j], overwritten in place by E[i][j]
    float* At = Ar + 64 * SA;        // [CW][65]   A[c0 + j][r0 + i]  (fp32 reader only)
    const float* Sb = S + (long)b * n * lds_ld;
    const Adj Ab = adj.graph(b, n);
    const float scale = scale_ptr[0];

    float sc[NS];
    typename Adj::RowReg ar[NR];
    typename Adj::Raw at[NA], atc[NA];           // atc: the current tile's A^T values (packed reader only)
    auto fetch = [&](int c0) {
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int i = e / KW, k = e % KW;
            sc[m] = Sb[(long)min(c0 + i, n - 1) * lds_ld + min(k, K - 1)];    // raw: zeroed when it is written to LDS
        }
        Ab.template fetch_rows<CW>(ar, n, r0, c0);
        Ab.template fetch_cols<CW, NJ>(at, n, r0, c0, wr, wc, l15, kq);
    };
    const int cbeg = part ? (int)blockIdx.z * split_tiles * CW : 0;
    const int cend = part ? min(nb, cbeg + split_tiles * CW) : nb;
    fetch(min(cbeg, max(nb - 1, 0)));
    lk_stage<KT, 64>(Sb, lds_ld, r0, n, K, Sr);
    // this wave's share of the output block: rows wave*16.., all KT column tiles
    lk_f32x4 out[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) out[t] = (lk_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = cbeg; c0 < cend; c0 += CW) {
        __syncthreads();                              // previous iteration's readers of Sc / Ar (/ At) are done
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int i = e / KW, k = e % KW;
            Sc[i * KP + k] = (c0 + i < n && k < K) ? sc[m] : 0.f;
        }
        Adj::template put_rows<CW, SA>(ar, Ar);
        Adj::template put_cols<CW>(at, At, atc);
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
                    const float e = scale * (lk_dldp(Ar[ri * SA + cj], raw) +
                                             lk_dldp(Adj::template col_value<NJ>(At, atc, i, j, r, ri, cj), raw));
                    Ar[ri * SA + cj] = (r0 + ri < nb && c0 + cj < nb) ? e : 0.f;
                }
            }
        __syncthreads();
        // out[16 rows of this wave][K] += E[rows][CW] · Sc[CW][K]
#pragma unroll 4
        for (int k0 = 0; k0 < CW; k0 += 4) {
            const float ev = Ar[(wave * 16 + l15) * SA + k0 + kq];
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
                    part[(((long)blockIdx.z * gridDim.y + b) * n + row) * K + col] = out[t][r];
                } else {
                    float* p = dSb + (long)row * ldds + col;
                    *p = accumulate ? *p + out[t][r] : out[t][r];
                }
            }
        }
    }
}

// dS[b, row, :] = (accumulate ? dS : 0) + sum_z part[z][b][row][:]   (rows >= n_b: the sum is empty)
__global__ __launch_bounds__(256) void k_link_reduce(const float* part, int splits, const int* num_nodes, float* dS,
                                                     int ldds, int B, int n, int K, int accumulate) {
    const long total = (long)B * n * K;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int k = (int)(e % K);
        const long row = e / K;
        const int b = (int)(row / n), r = (int)(row % n);
        const int nb = num_nodes ? min(num_nodes[b], n) : n;
        float v = 0.f;
        if ((r / 64) * 64 < nb)                       // the row block ran: every split stored its partial
            for (int z = 0; z < splits; ++z) v += part[(long)z * total + e];
        float* p = dS + row * ldds + k;
        *p = accumulate ? *p + v : v;
    }
}

// ------------------------------------------------------------------ the plan (host only; dp_linkpred_plan)
// dynamic LDS of the two kernels, shared by the launchers' constants and the plan
constexpr size_t lk_fwd_lds(int kt) { return ((size_t)2 * 64 * (kt * 16 + 2) + 4) * sizeof(float); }
constexpr size_t lk_bwd_lds(int kt, int cw, bool col_lds) {
    return ((size_t)(64 + cw) * (kt * 16 + 2) + 64 * (cw + 4) + (col_lds ? cw * 65 : 0)) * sizeof(float);
}

// Everything link_fwd / link_bwd decide from (B, n, K), the same for both readers.  Small batches split the backward's
// column tiles over extra workgroups (>= ~512 in all) whose partials k_link_reduce sums afterwards; splits == 1 is the
// non-split form (no partials, k_link_bwd stores dS itself).  K > 256: kt = 0 and false; the sizes are still filled
// in (as for the widest walk), so that a workspace query answers before the launchers refuse.
bool linkpred_plan(int B, int n, int K, LinkPlan& p) {
    p.kt = lk_kt(K);
    p.cw = p.kt >= 12 ? 32 : 64;
    p.col_tiles = (n + p.cw - 1) / p.cw;
    const long base_wgs = (long)((n + 63) / 64) * B;
    int splits = (int)((512 + base_wgs - 1) / base_wgs);
    splits = splits < 1 ? 1 : (splits > p.col_tiles ? p.col_tiles : splits);
    p.split_tiles = (p.col_tiles + splits - 1) / splits;
    p.splits = (p.col_tiles + p.split_tiles - 1) / p.split_tiles;
    p.fwd_tiles = ((n + 63) / 64) * ((n + 63) / 64);
    p.fwd_lds = p.kt ? lk_fwd_lds(p.kt) : 0;
    p.bwd_lds = p.kt ? lk_bwd_lds(p.kt, p.cw, LkAdjF32::kColLds) : 0;
    return p.kt != 0;
}

// every instantiation is raised once per device to what it can ever need (static + dynamic LDS stay within 160 KiB)

template <int KT, class Adj>
static void launch_link_fwd(Seq& q, const float* S, int lds_ld, Adj adj, const int* num_nodes, int B, int n, int K,
                            int tiles, float* partial) {
    constexpr size_t bytes = lk_fwd_lds(KT);
    static DynLdsOnce attr;
    if (bytes > 64 * 1024)
        ensure_dyn_lds(q, attr, reinterpret_cast<const void*>(&k_link_fwd<KT, Adj>), (int)bytes, "k_link_fwd");
    if (!q.ok()) return;
    hipLaunchKernelGGL((k_link_fwd<KT, Adj>), dim3(tiles * tiles, B), dim3(256), bytes, q.stream, S, lds_ld, adj,
                       num_nodes, n, K, tiles, partial);
}

template <class Adj>
static void link_fwd(Seq& q, const float* S, int lds_ld, Adj adj, const int* num_nodes, float* loss_out, int B, int n,
                     int K, const float* norm) {
    if (q.err) return;
    LinkPlan plan;
    const bool fits = linkpred_plan(B, n, K, plan);
    const int tiles = (n + 63) / 64, kt = plan.kt;
    float* partial = q.alloc<float>((size_t)B * plan.fwd_tiles);
    if (!q.ok()) return;
    if (!fits) {
        set_error("linkpred: K=%d clusters exceed the fused tile kernel (max 256)", K);
        q.err = DP_ERR_UNSUPPORTED;
        return;
    }
#define LK_FWD(T) \
    case T: launch_link_fwd<T>(q, S, lds_ld, adj, num_nodes, B, n, K, tiles, partial); break;
    switch (kt) { LK_FWD(1) LK_FWD(2) LK_FWD(3) LK_FWD(4) LK_FWD(6) LK_FWD(8) LK_FWD(12) LK_FWD(16) }
#undef LK_FWD
    q.check_launch("link_fwd");
    hipLaunchKernelGGL(k_link_final, dim3(1), dim3(256), 0, q.stream, partial, B * tiles * tiles, num_nodes, B, n,
                       loss_out, (float*)nullptr, (const float*)nullptr, norm);
    q.check_launch("link_final");
}

template <int KT, int NJ, class Adj>
static void launch_link_bwd(Seq& q, const float* S, int lds_ld, Adj adj, const int* num_nodes, const float* scale,
                            float* dS, int ldds, int B, int n, int K, int accumulate, float* part, int splits,
                            int split_tiles) {
    constexpr int CW = 32 * NJ;
    constexpr size_t bytes = lk_bwd_lds(KT, CW, Adj::kColLds);
    static_assert(bytes <= 160 * 1024, "link_bwd LDS");
    static DynLdsOnce attr;
    if (bytes > 64 * 1024)
        ensure_dyn_lds(q, attr, reinterpret_cast<const void*>(&k_link_bwd<KT, NJ, Adj>), (int)bytes, "k_link_bwd");
    if (!q.ok()) return;
    hipLaunchKernelGGL((k_link_bwd<KT, NJ, Adj>), dim3((n + 63) / 64, B, part ? splits : 1), dim3(256), bytes, q.stream,
                       S, lds_ld, adj, num_nodes, scale, dS, ldds, n, K, accumulate, part, split_tiles);
}

template <class Adj>
static void link_bwd(Seq& q, const float* S, int lds_ld, Adj adj, const int* num_nodes, const float* dloss, float* dS,
                     int ldds, int B, int n, int K, int accumulate, const float* norm) {
    if (q.err) return;
    float* scale = q.alloc<float>(64);
    LinkPlan plan;
    const bool fits = linkpred_plan(B, n, K, plan);
    const int kt = plan.kt, splits = plan.splits, split_tiles = plan.split_tiles;
    float* part = splits > 1 ? q.alloc<float>((size_t)splits * B * n * K) : nullptr;
    if (!q.ok()) return;
    if (!fits) {
        set_error("linkpred backward: K=%d clusters exceed the fused tile kernel (max 256)", K);
        q.err = DP_ERR_UNSUPPORTED;
        return;
    }
    hipLaunchKernelGGL(k_link_final, dim3(1), dim3(256), 0, q.stream, (const float*)nullptr, 0, num_nodes, B, n,
                       (float*)nullptr, scale, dloss, norm);
    q.check_launch("link_scale");
#define LK_BWD(T, J)                                                                                             \
    case T:                                                                                                      \
        launch_link_bwd<T, J>(q, S, lds_ld, adj, num_nodes, scale, dS, ldds, B, n, K, accumulate, part, splits,  \
                              split_tiles);                                                                      \
        break;
    switch (kt) { LK_BWD(1, 2) LK_BWD(2, 2) LK_BWD(3, 2) LK_BWD(4, 2) LK_BWD(6, 2) LK_BWD(8, 2) LK_BWD(12, 1) LK_BWD(16, 1) }
#undef LK_BWD
    q.check_launch("link_bwd");
    if (part) {
        const long total = (long)B * n * K;
        long blocks = (total + 255) / 256;
        blocks = blocks > 2048 ? 2048 : blocks;
        hipLaunchKernelGGL(k_link_reduce, dim3((int)blocks), dim3(256), 0, q.stream, part, splits, num_nodes, dS, ldds, B,
                           n, K, accumulate);
        q.check_launch("link_reduce");
    }
}

void linkpred_fwd(Seq& q, const float* S, int lds_ld, const float* adj, const int* num_nodes, float* loss_out, int B,
                  int n, int K, const float* norm) {
    link_fwd(q, S, lds_ld, LkAdjF32{adj, n}, num_nodes, loss_out, B, n, K, norm);
}
void linkpred_bwd(Seq& q, const float* S, int lds_ld, const float* adj, const int* num_nodes, const float* dloss,
                  float* dS, int ldds, int B, int n, int K, int accumulate, const float* norm) {
    link_bwd(q, S, lds_ld, LkAdjF32{adj, n}, num_nodes, dloss, dS, ldds, B, n, K, accumulate, norm);
}
void linkpred_fwd_packed(Seq& q, const float* S, int lds_ld, const unsigned short* pk, const int* num_nodes,
                         float* loss_out, int B, int n, int K, const float* norm) {
    link_fwd(q, S, lds_ld, LkAdjBf16{pk, pk, adj_pack_ld(n)}, num_nodes, loss_out, B, n, K, norm);
}
void linkpred_bwd_packed(Seq& q, const float* S, int lds_ld, const unsigned short* pk, const unsigned short* pkt,
                         const int* num_nodes, const float* dloss, float* dS, int ldds, int B, int n, int K,
                         int accumulate, const float* norm) {
    link_bwd(q, S, lds_ld, LkAdjBf16{pk, pkt, adj_pack_ld(n)}, num_nodes, dloss, dS, ldds, B, n, K, accumulate, norm);
}

}  // namespace dp
