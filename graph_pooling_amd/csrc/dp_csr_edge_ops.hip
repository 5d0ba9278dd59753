// Learned edge weights on a CSR adjacency: segmented passes over the stored entries of each CSR row.
//
//     edge softmax     out[e] = exp(s_e - m_i) / sum_{e' in row i} exp(s_e' - m_i), m_i the row maximum, and its backward
//                      ds_e = a_e (g_e - sum_row a g);
//     D^-1/2 A D^-1/2  d_c the column sum of the stored values (the row sum of row c of the transposed CSR, entry k of
//                      which is the stored entry mirror[k]), r = d^-1/2, out[e] = v_e (r_i r_j), and its backward
//                      dv_e = g_e r_i r_j + G_j, G_c = -1/2 r_c^3 t_c, t_c = sum_{row c} g v r_col + sum_{col c} g v r_row.
//
// Rows are short and skewed, so a row is served by a GROUP of L = 4 / 16 / 64 lanes chosen from the mean row length
// (edge_pick, the one place that decides; dp_csr_edge_plan reports it): 256 / L rows per workgroup, lane `sub` of the
// group takes entries beg + sub, beg + sub + L, ... — every index and value load is coalesced across the group — and a
// row longer than the group loops.  The softmax kernels keep up to R entries per lane in registers (a row of at most
// L * R entries is read once); a longer row runs a per-lane running maximum and sum and is read a second time for the
// output.  Every sum has one order: the lane's entries ascending, then a DPP tree over the group (the reductions sit
// outside every branch, so all lanes of a wave take part).  No atomics, no LDS, no temporary beyond the two [n] vectors
// of the normalisation; a second run gives the same bits.
#include <math.h>

#include "dp_csr_edge_seg.h"
#include "dp_entry.h"

namespace dp {
namespace {

struct EdgePick {
    int lanes, regs, rows_per_wg;
};

// The one place that decides the launch form.  The group is eo_lanes' (dp_csr_edge_seg.h: the smallest of 4 / 16 / 64
// lanes that covers the MEAN row in two visits); a narrow group holds more entries per lane, so that a row several times
// the mean still fits the registers: 4 x 8, 16 x 4, 64 x 4 entries.
constexpr int eo_regs(int lanes) { return lanes == 4 ? 8 : 4; }
EdgePick edge_pick(long n_rows, long nnz) {
    EdgePick k;
    k.lanes = eo_lanes(n_rows, nnz);
    k.regs = eo_regs(k.lanes);
    k.rows_per_wg = EO_THREADS / k.lanes;
    return k;
}

template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_softmax_fwd(const float* __restrict__ s,
                                                                 const int* __restrict__ indptr,
                                                                 float* __restrict__ out, int n_rows) {
    constexpr int R = eo_regs(L);
    const Seg g = eo_seg<L>(indptr, n_rows);
    const bool fits = g.end - g.beg <= L * R;
    float v[R];
    float m = -INFINITY, sum = 0.f;
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            v[k] = e < g.end ? s[e] : -INFINITY;
            m = fmaxf(m, v[k]);
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) {      // running maximum and sum (exp(-inf) = 0 starts it)
            const float x = s[e];
            const float mn = fmaxf(m, x);
            sum = sum * expf(m - mn) + expf(x - mn);
            m = mn;
        }
    }
    const float M = eo_max<L>(m);
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = expf(v[k] - M);                            // a slot beyond the row: exp(-inf) = 0
            sum += v[k];
        }
    } else {
        sum = sum * expf(m - M);
    }
    const float S = eo_sum<L>(sum);
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            if (e < g.end) out[e] = v[k] / S;
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) out[e] = expf(s[e] - M) / S;
    }
}

template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_softmax_bwd(const float* __restrict__ a,
                                                                 const float* __restrict__ dout,
                                                                 const int* __restrict__ indptr,
                                                                 float* __restrict__ ds, int n_rows) {
    constexpr int R = eo_regs(L);
    const Seg g = eo_seg<L>(indptr, n_rows);
    const bool fits = g.end - g.beg <= L * R;
    float av[R], gv[R];
    float acc = 0.f;
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            const bool in = e < g.end;
            av[k] = in ? a[e] : 0.f;
            gv[k] = in ? dout[e] : 0.f;
            acc = fmaf(av[k], gv[k], acc);
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) acc = fmaf(a[e], dout[e], acc);
    }
    const float dot = eo_sum<L>(acc);
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            if (e < g.end) ds[e] = av[k] * (gv[k] - dot);
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) ds[e] = a[e] * (dout[e] - dot);
    }
}

// r_c = d_c^-1/2, d_c the sum of row c of the transposed CSR (values NULL: the entry count; mirror NULL: its own order)
template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_sym_rdeg(const int* __restrict__ indptr_t,
                                                              const int* __restrict__ mirror,
                                                              const float* __restrict__ values,
                                                              float* __restrict__ rdeg, int n) {
    const Seg g = eo_seg<L>(indptr_t, n);
    float acc = 0.f;
    for (int k = g.beg + g.sub; k < g.end; k += L) acc += values ? values[mirror ? mirror[k] : k] : 1.f;
    const float d = eo_sum<L>(acc);
    if (g.live && g.sub == 0) rdeg[g.row] = 1.f / sqrtf(d);
}

template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_sym_scale(const int* __restrict__ indptr,
                                                               const int* __restrict__ indices,
                                                               const float* __restrict__ values,
                                                               const float* __restrict__ rdeg,
                                                               float* __restrict__ out, int n) {
    const Seg g = eo_seg<L>(indptr, n);
    const float ri = rdeg[g.row];
    for (int e = g.beg + g.sub; e < g.end; e += L) out[e] = (values ? values[e] : 1.f) * (ri * rdeg[indices[e]]);
}

// G_c = -1/2 r_c^3 t_c: the row part of t_c over the forward CSR, then the column part over the transposed one
template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_sym_gdeg(const int* __restrict__ indptr,
                                                              const int* __restrict__ indices,
                                                              const float* __restrict__ values,
                                                              const int* __restrict__ indptr_t,
                                                              const int* __restrict__ indices_t,
                                                              const int* __restrict__ mirror,
                                                              const float* __restrict__ rdeg,
                                                              const float* __restrict__ dout,
                                                              float* __restrict__ gdeg, int n) {
    const Seg g = eo_seg<L>(indptr, n);
    const int tbeg = g.live ? indptr_t[g.row] : 0, tend = g.live ? indptr_t[g.row + 1] : 0;
    float acc = 0.f;
    for (int e = g.beg + g.sub; e < g.end; e += L)
        acc += (dout[e] * (values ? values[e] : 1.f)) * rdeg[indices[e]];
    for (int k = tbeg + g.sub; k < tend; k += L) {
        const int e = mirror[k];
        acc += (dout[e] * (values ? values[e] : 1.f)) * rdeg[indices_t[k]];
    }
    const float t = eo_sum<L>(acc);
    if (g.live && g.sub == 0) {
        const float rc = rdeg[g.row];
        gdeg[g.row] = (g.end - g.beg) + (tend - tbeg) > 0 ? -0.5f * (rc * rc * rc) * t : 0.f;
    }
}

template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_edge_sym_dvalues(const int* __restrict__ indptr,
                                                                 const int* __restrict__ indices,
                                                                 const float* __restrict__ rdeg,
                                                                 const float* __restrict__ gdeg,
                                                                 const float* __restrict__ dout,
                                                                 float* __restrict__ dvalues, int n) {
    const Seg g = eo_seg<L>(indptr, n);
    const float ri = rdeg[g.row];
    for (int e = g.beg + g.sub; e < g.end; e += L) {
        const int j = indices[e];
        dvalues[e] = dout[e] * (ri * rdeg[j]) + gdeg[j];
    }
}

// one launch of kernel family `kern` over n_rows rows in the picked form
#define EO_LAUNCH(q, pick, n_rows, kern, ...)                                                         \
    do {                                                                                              \
        if ((q).ok()) {                                                                               \
            const dim3 grid(cdiv((n_rows), (pick).rows_per_wg)), block(EO_THREADS);                   \
            if ((pick).lanes == 4) hipLaunchKernelGGL((kern<4>), grid, block, 0, (q).stream, __VA_ARGS__);        \
            else if ((pick).lanes == 16) hipLaunchKernelGGL((kern<16>), grid, block, 0, (q).stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((kern<64>), grid, block, 0, (q).stream, __VA_ARGS__);             \
            (q).check_launch(#kern);                                                                  \
        }                                                                                             \
    } while (0)

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_csr_edge_plan(int n_rows, int nnz, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    const EdgePick k = edge_pick(n_rows, nnz);
    const int plan[DP_CSR_EDGE_PLAN_INTS] = {k.lanes, k.regs, k.rows_per_wg, k.lanes * k.regs};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

int dp_csr_edge_softmax_fwd(const float* scores, const int* indptr, float* out, int n_rows, int nnz, void* stream) {
    DP_PTR(scores); DP_PTR(indptr); DP_PTR(out);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    if (n_rows == 0 || nnz == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const EdgePick k = edge_pick(n_rows, nnz);
    EO_LAUNCH(q, k, n_rows, k_edge_softmax_fwd, scores, indptr, out, n_rows);
    return q.err;
}

int dp_csr_edge_softmax_bwd(const float* out, const float* dout, const int* indptr, float* dscores, int n_rows, int nnz,
                            void* stream) {
    DP_PTR(out); DP_PTR(dout); DP_PTR(indptr); DP_PTR(dscores);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    if (n_rows == 0 || nnz == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const EdgePick k = edge_pick(n_rows, nnz);
    EO_LAUNCH(q, k, n_rows, k_edge_softmax_bwd, out, dout, indptr, dscores, n_rows);
    return q.err;
}

int dp_csr_sym_norm_fwd(const int* indptr, const int* indices, const float* values, const int* indptr_t,
                        const int* indices_t, const int* mirror, float* rdeg, float* out, int n, int nnz, void* stream) {
    DP_PTR(indptr); DP_PTR(indices);
    DP_ALIGNED4(values);
    DP_PTR(indptr_t); DP_PTR(indices_t);
    DP_ALIGNED4(mirror);
    DP_CHECK(mirror != nullptr || !own_transpose(indices, indices_t), DP_ERR_INVALID_ARG,
             "mirror is NULL beside a transposed CSR of its own (indices_t is not indices)");
    DP_PTR(rdeg); DP_PTR(out);
    DP_NONNEG(n);
    DP_NONNEG(nnz);
    if (n == 0 || nnz == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const EdgePick k = edge_pick(n, nnz);
    EO_LAUNCH(q, k, n, k_edge_sym_rdeg, indptr_t, mirror, values, rdeg, n);
    EO_LAUNCH(q, k, n, k_edge_sym_scale, indptr, indices, values, (const float*)rdeg, out, n);
    return q.err;
}

int dp_csr_sym_norm_bwd(const int* indptr, const int* indices, const float* values, const int* indptr_t,
                        const int* indices_t, const int* mirror, const float* rdeg, const float* dout, float* gdeg,
                        float* dvalues, int n, int nnz, void* stream) {
    DP_PTR(indptr); DP_PTR(indices);
    DP_ALIGNED4(values);
    DP_PTR(indptr_t); DP_PTR(indices_t);
    DP_PTR(mirror); DP_PTR(rdeg); DP_PTR(dout); DP_PTR(gdeg); DP_PTR(dvalues);
    DP_NONNEG(n);
    DP_NONNEG(nnz);
    if (n == 0 || nnz == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const EdgePick k = edge_pick(n, nnz);
    EO_LAUNCH(q, k, n, k_edge_sym_gdeg, indptr, indices, values, indptr_t, indices_t, mirror, rdeg, dout, gdeg, n);
    EO_LAUNCH(q, k, n, k_edge_sym_dvalues, indptr, indices, rdeg, (const float*)gdeg, dout, dvalues, n);
    return q.err;
}

}  // extern "C"
