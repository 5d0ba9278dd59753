// The launch form shared by the segmented passes over the rows of a CSR (dp_csr_edge_ops.hip, dp_csr_gat.hip): a GROUP of
// L = 4 / 16 / 64 lanes serves one row, 256 / L rows per workgroup, lane `sub` of the group takes entries beg + sub,
// beg + sub + L, ...; a sum or a maximum over the row is the lane's own, then a DPP tree over the group.
#pragma once
#include "dp_common.h"

namespace dp {

constexpr int EO_THREADS = 256;

// The group is the smallest of 4 / 16 / 64 lanes that covers the MEAN row in two visits (mean <= 8: 4 lanes, <= 32: 16
// lanes, 64 above).
inline int eo_lanes(long n_rows, long nnz) { return nnz <= 8 * n_rows ? 4 : (nnz <= 32 * n_rows ? 16 : 64); }

template <int L>
__device__ __forceinline__ float eo_sum(float v) {
    if constexpr (L == 4) return quad4_sum(v);
    else if constexpr (L == 16) return row16_sum(v);
    else return wave64_sum(v);
}
template <int L>
__device__ __forceinline__ float eo_max(float v) {
    if constexpr (L == 4) {
        v = fmaxf(v, dpp_src<0xB1, 0xF, true>(v, v));      // quad_perm [1,0,3,2]
        v = fmaxf(v, dpp_src<0x4E, 0xF, true>(v, v));      // quad_perm [2,3,0,1]
        return v;
    } else if constexpr (L == 16) {
        return row16_max(v);
    } else {
        return wave64_max(v);
    }
}

// the row of this lane's group: its stored entries [beg, end) (none for a row beyond n_rows) and the lane's place
struct Seg {
    int row, beg, end, sub;
    bool live;
};
template <int L>
__device__ __forceinline__ Seg eo_seg(const int* __restrict__ indptr, int n_rows) {
    Seg g;
    const long row = (long)blockIdx.x * (EO_THREADS / L) + threadIdx.x / L;
    g.sub = threadIdx.x % L;
    g.live = row < n_rows;
    g.row = g.live ? (int)row : 0;
    g.beg = g.live ? indptr[g.row] : 0;
    g.end = g.live ? indptr[g.row + 1] : 0;
    return g;
}

}  // namespace dp
