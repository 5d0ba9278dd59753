// Row entropy of the soft assignment S (DiffPool's second auxiliary objective):
//
//     E = ( sum_b sum_{i < n_b} sum_k  -s_bik ln(s_bik + eps) ) / sum_b n_b,           eps = 1e-15 added in fp32
//     dE/ds_bik = -( ln(s_bik + eps) + s_bik / (s_bik + eps) ) / sum_b n_b             (i < n_b; 0 for i >= n_b)
//
// A pure stream over S.  A row is served by a group of L = 4 / 16 / 64 lanes (the smallest that covers K in one visit,
// 64 with a strided loop above), each lane reading 16 bytes where pointer, leading dimension and K allow it and 4 bytes
// otherwise; a workgroup of 256 threads holds 256 / L rows at a time and walks the rows grid-strided, counted in 64
// bits.  Rows i >= n_b are never loaded (a branch round the load, not a multiplication by a mask).
//
// Forward: every term is formed in fp32 — fl(s * logf(fl(s + eps))) — and from there on summed in fp64: in the lane over
// everything it visits, over the workgroup through LDS in a fixed tree, and over the workgroups' partials by a second,
// one-workgroup launch in a fixed order.  No atomics, no ticket: E is the same bits on every run, and the only fp32
// roundings are the three of a term and the one of the final quotient (the bound in tests/assign_ent_cases.py).
// Backward: elementwise; the normaliser sum_b n_b is an integer sum every workgroup forms for itself.
#include "dp_common.h"

// every product and sum below rounds on its own (the bound counts them, and total_inout is specified as
// old + fl(weight * E)): hipcc's default would contract a * b + c into one fma
#pragma clang fp contract(off)

namespace dp {
namespace {

constexpr int AE_THREADS = 256;
constexpr int AE_MAX_BLOCKS = 2048;     // 8 workgroups per CU; the rest of the rows by the grid-stride loop
constexpr float AE_EPS = 1e-15f;

// n_b as the kernels use it: num_nodes[b] clamped into [0, n]
__device__ __forceinline__ int ae_nb(const int* num_nodes, int b, int n) {
    const int v = num_nodes[b];
    return v < 0 ? 0 : (v > n ? n : v);
}

// fixed-order workgroup sum through LDS (every thread calls it; the total is returned to all)
template <typename T>
__device__ __forceinline__ T ae_block_sum(T v, T* sh) {
    const int t = threadIdx.x;
    __syncthreads();          // sh may still be read by a previous call
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = AE_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    return sh[0];
}

// row r of [B, n]: is it a node of its graph?
__device__ __forceinline__ bool ae_row_valid(long long r, const int* num_nodes, int n, bool rows32) {
    if (!num_nodes) return true;
    int b, i;
    if (rows32) {
        const unsigned ru = (unsigned)r;
        b = (int)(ru / (unsigned)n);
        i = (int)(ru - (unsigned)b * (unsigned)n);
    } else {
        const long long bb = r / n;
        b = (int)bb;
        i = (int)(r - bb * n);
    }
    return i < ae_nb(num_nodes, b, n);
}

__device__ __forceinline__ float ae_term(float s) { return s * logf(s + AE_EPS); }          // s ln(s + eps) <= 0
__device__ __forceinline__ float ae_dterm(float s) {                                         // ln(s + eps) + s / (s + eps)
    const float se = s + AE_EPS;
    return logf(se) + s / se;
}

// L lanes per row, V floats per lane and visit (V = 4: 16-byte loads; needs S % 16 == 0, lds % 4 == 0, K % 4 == 0)
template <int L, int V>
__global__ __launch_bounds__(AE_THREADS) void k_assign_ent_fwd(const float* __restrict__ S, int lds,
                                                               const int* __restrict__ num_nodes, double* __restrict__ part,
                                                               long long rows, int n, int K) {
    __shared__ double sh[AE_THREADS];
    constexpr int G = AE_THREADS / L;                  // rows a workgroup holds at a time
    const int grp = threadIdx.x / L, lane = threadIdx.x % L;
    const bool rows32 = rows < (1ll << 31);
    double acc = 0.0;
    for (long long r = (long long)blockIdx.x * G + grp; r < rows; r += (long long)gridDim.x * G) {
        if (!ae_row_valid(r, num_nodes, n, rows32)) continue;
        const float* row = S + (size_t)r * (size_t)lds;
        for (int c = lane * V; c < K; c += L * V) {
            if constexpr (V == 4) {
                const float4 v = *reinterpret_cast<const float4*>(row + c);
                acc += (double)ae_term(v.x);
                acc += (double)ae_term(v.y);
                acc += (double)ae_term(v.z);
                acc += (double)ae_term(v.w);
            } else {
                acc += (double)ae_term(row[c]);
            }
        }
    }
    const double tot = ae_block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one workgroup: the partials in a fixed order, the normaliser, E and (optionally) total += weight * E
__global__ __launch_bounds__(AE_THREADS) void k_assign_ent_finish(const double* __restrict__ part, int nparts,
                                                                  const int* __restrict__ num_nodes, int B, int n,
                                                                  float weight, float* __restrict__ ent_out,
                                                                  float* __restrict__ total_inout) {
    __shared__ double sh[AE_THREADS];
    __shared__ long long shn[AE_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += AE_THREADS) acc += part[i];
    const double tot = ae_block_sum(acc, sh);
    long long norm = (long long)B * n;
    if (num_nodes) {
        long long c = 0;
        for (int b = threadIdx.x; b < B; b += AE_THREADS) c += ae_nb(num_nodes, b, n);
        norm = ae_block_sum(c, shn);
    }
    if (threadIdx.x == 0) {
        const float e = (float)(-tot / (double)(norm > 0 ? norm : 1));      // no valid node at all: E = 0
        ent_out[0] = e;
        if (total_inout) total_inout[0] = total_inout[0] + weight * e;     // exactly old + fl(w E): no fma (pragma above)
    }
}

template <int L, int V>
__global__ __launch_bounds__(AE_THREADS) void k_assign_ent_bwd(const float* __restrict__ S, int lds,
                                                               const int* __restrict__ num_nodes,
                                                               const float* __restrict__ dloss, float weight,
                                                               float* __restrict__ dS, int ldds, int accumulate,
                                                               long long rows, int B, int n, int K) {
    __shared__ long long shn[AE_THREADS];
    constexpr int G = AE_THREADS / L;
    const int grp = threadIdx.x / L, lane = threadIdx.x % L;
    const bool rows32 = rows < (1ll << 31);
    long long norm = rows;
    if (num_nodes) {
        long long c = 0;
        for (int b = threadIdx.x; b < B; b += AE_THREADS) c += ae_nb(num_nodes, b, n);
        norm = ae_block_sum(c, shn);
    }
    // d = (ln(s + eps) + s / (s + eps)) * coef,  coef = -(dloss * weight) / norm
    const float coef = -((dloss ? dloss[0] : 1.f) * weight) / (float)(norm > 0 ? norm : 1);
    for (long long r = (long long)blockIdx.x * G + grp; r < rows; r += (long long)gridDim.x * G) {
        float* drow = dS + (size_t)r * (size_t)ldds;
        if (!ae_row_valid(r, num_nodes, n, rows32)) {
            if (!accumulate) {
                for (int c = lane * V; c < K; c += L * V) {
                    if constexpr (V == 4) *reinterpret_cast<float4*>(drow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
                    else drow[c] = 0.f;
                }
            }
            continue;
        }
        const float* row = S + (size_t)r * (size_t)lds;
        for (int c = lane * V; c < K; c += L * V) {
            if constexpr (V == 4) {
                const float4 v = *reinterpret_cast<const float4*>(row + c);
                float4 d = make_float4(ae_dterm(v.x) * coef, ae_dterm(v.y) * coef, ae_dterm(v.z) * coef,
                                       ae_dterm(v.w) * coef);
                if (accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(drow + c);
                    d.x = o.x + d.x; d.y = o.y + d.y; d.z = o.z + d.z; d.w = o.w + d.w;
                }
                *reinterpret_cast<float4*>(drow + c) = d;
            } else {
                const float d = ae_dterm(row[c]) * coef;
                drow[c] = accumulate ? drow[c] + d : d;
            }
        }
    }
}

int ae_grid(long long rows, int lanes) {
    const long long g = AE_THREADS / lanes;
    const long long blocks = (rows + g - 1) / g;
    return (int)(blocks < AE_MAX_BLOCKS ? blocks : AE_MAX_BLOCKS);
}

}  // namespace

// The one place that decides the launch form: 16-byte lanes only when every pointer and leading dimension involved and
// K allow it; the lane group is the smallest of 4 / 16 / 64 that covers a row in one visit (64 and a loop above).
AssignEntPick assign_ent_pick(const void* S, int lds, const void* dS, int ldds, int K) {
    AssignEntPick p;
    const bool a16 = ((uintptr_t)S & 15) == 0 && (lds & 3) == 0 && (K & 3) == 0 &&
                     (dS == nullptr || (((uintptr_t)dS & 15) == 0 && (ldds & 3) == 0));
    p.quad = a16 ? 1 : 0;
    const int per = a16 ? 4 : 1;
    p.lanes = K <= 4 * per ? 4 : (K <= 16 * per ? 16 : 64);
    return p;
}

size_t assign_ent_part_doubles() { return AE_MAX_BLOCKS; }

void assign_entropy_fwd(Seq& q, const float* S, int lds, const int* num_nodes, float weight, float* ent_out,
                        float* total_inout, int B, int n, int K) {
    double* part = q.alloc<double>(assign_ent_part_doubles());
    if (!q.ok()) return;
    const long long rows = (long long)B * n;
    const AssignEntPick p = assign_ent_pick(S, lds, nullptr, 0, K);
    const int grid = ae_grid(rows, p.lanes);
#define AE_FWD(L, V) \
    hipLaunchKernelGGL((k_assign_ent_fwd<L, V>), dim3(grid), dim3(AE_THREADS), 0, q.stream, S, lds, num_nodes, part, rows, n, K)
    if (p.quad) {
        if (p.lanes == 4) AE_FWD(4, 4); else if (p.lanes == 16) AE_FWD(16, 4); else AE_FWD(64, 4);
    } else {
        if (p.lanes == 4) AE_FWD(4, 1); else if (p.lanes == 16) AE_FWD(16, 1); else AE_FWD(64, 1);
    }
#undef AE_FWD
    q.check_launch("k_assign_ent_fwd");
    if (!q.ok()) return;
    hipLaunchKernelGGL(k_assign_ent_finish, dim3(1), dim3(AE_THREADS), 0, q.stream, part, grid, num_nodes, B, n, weight,
                       ent_out, total_inout);
    q.check_launch("k_assign_ent_finish");
}

void assign_entropy_bwd(Seq& q, const float* S, int lds, const int* num_nodes, const float* dloss, float weight,
                        float* dS, int ldds, int accumulate, int B, int n, int K) {
    if (!q.ok()) return;
    const long long rows = (long long)B * n;
    const AssignEntPick p = assign_ent_pick(S, lds, dS, ldds, K);
    const int grid = ae_grid(rows, p.lanes);
#define AE_BWD(L, V)                                                                                                  \
    hipLaunchKernelGGL((k_assign_ent_bwd<L, V>), dim3(grid), dim3(AE_THREADS), 0, q.stream, S, lds, num_nodes, dloss, \
                       weight, dS, ldds, accumulate, rows, B, n, K)
    if (p.quad) {
        if (p.lanes == 4) AE_BWD(4, 4); else if (p.lanes == 16) AE_BWD(16, 4); else AE_BWD(64, 4);
    } else {
        if (p.lanes == 4) AE_BWD(4, 1); else if (p.lanes == 16) AE_BWD(16, 1); else AE_BWD(64, 1);
    }
#undef AE_BWD
    q.check_launch("k_assign_ent_bwd");
}

}  // namespace dp
