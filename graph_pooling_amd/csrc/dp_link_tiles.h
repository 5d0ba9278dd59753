// Tile helpers shared by the link-prediction kernels: dp_linkpred.hip (dense / packed adjacency) and
// dp_csr_linkpred.hip (CSR graph, adjacency-free tile walk).  P tiles of min(S S^T, 1) are formed on the fp32 MFMA from
// S row blocks staged in LDS and are never stored.
#pragma once
#include "dp_common.h"

namespace dp {

#define LINK_EPS 1e-7f
typedef float lk_f32x4 __attribute__((ext_vector_type(4)));

__device__ inline float lk_block_sum(float v, float* red) {
    v = wave64_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// LDS images of S row blocks are [rows][KP] with KW = 16 KT padded columns (zero beyond K) and KP = KW + 2, so the
// MFMA fragment read (16 rows x 2 k per 32-lane group) touches 32 distinct banks.
// (force-inlined: as a real call — which hipcc chose for KT >= 12 — its pointers are generic and every access a flat_load)
template <int KT, int ROWS>
__device__ __forceinline__ void lk_stage(const float* Sb, int lds_ld, int r0, int n, int K, float* dst) {
    constexpr int KW = KT * 16, KP = KW + 2;
    // loads first, selects and LDS writes after: a select right behind its load makes every load a round trip of
    // its own (the first version: one `s_waitcnt vmcnt(0)` per element, 32 serial round trips in the forward kernel)
    constexpr int NV = ROWS * KW / 256;
    float v[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) {
        const int e = threadIdx.x + 256 * m;
        const int i = e / KW, k = e % KW;
        v[m] = Sb[(long)min(r0 + i, n - 1) * lds_ld + min(k, K - 1)];
    }
#pragma unroll
    for (int m = 0; m < NV; ++m) {
        const int e = threadIdx.x + 256 * m;
        const int i = e / KW, k = e % KW;
        dst[i * KP + k] = (r0 + i < n && k < K) ? v[m] : 0.f;
    }
}

// P tile of a wave: rows wr*32.., cols wc*16*NJ.. ; acc[mi][ni] are 16x16 tiles
template <int KT, int NJ>
__device__ __forceinline__ void lk_ptile(const float* Sr, const float* Sc, int K, int wr, int wc, int l15, int kq,
                                lk_f32x4 (&acc)[2][NJ]) {
    constexpr int KP = KT * 16 + 2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (lk_f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {          // columns K..KW are zero in both images
        float a[2], b[NJ];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Sr[(wr * 32 + i * 16 + l15) * KP + k0 + kq];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = Sc[(wc * 16 * NJ + j * 16 + l15) * KP + k0 + kq];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// torch.min(a, b) backward: full gradient where a < b, half on ties, none above
__device__ inline float lk_min_gate(float raw) { return raw < 1.f ? 1.f : (raw == 1.f ? 0.5f : 0.f); }

// KT (column tiles of 16 the kernels are instantiated for) that holds K clusters; 0: K > 256
inline int lk_kt(int K) {
    const int kt = (K + 15) / 16;
    static const int steps[] = {1, 2, 3, 4, 6, 8, 12, 16};
    for (int s : steps)
        if (kt <= s) return s;
    return 0;
}

}  // namespace dp
