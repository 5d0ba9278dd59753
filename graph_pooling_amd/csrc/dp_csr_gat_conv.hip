// Multi-head GAT convolution on a CSR adjacency: the attention coefficients of dp_csr_gat.hip multiplied into
// the gathered neighbour features in the pass that computes them, per head, nothing of size nnz ever written.
//
//     pre_eh = u_ih + v_jh,  s_eh = pre_eh > 0 ? pre_eh : slope * pre_eh       (e = (i, j), j = indices[e]; derivative
//     a_eh   = exp(s_eh - m_ih) / zsum_ih                                       `slope` AT 0, as torch's leaky_relu)
//     Y_ih   = sum_{row i} a_eh z_j^h             z^h: columns hC .. hC + C - 1 of z [n, H C]
//     y_i    = [Y_i0 | .. | Y_i(H-1)]  (concat)   or   (sum_h Y_ih) / H  (mean: heads ascending, one division)
//
// and its backward, dY_ih = dy_i^h (concat) or dy_i / H (mean):
//
//     g_eh = dY_ih . z_j^h,  t_ih = sum_{row i} a_eh g_eh,  dpre_eh = a_eh (g_eh - t_ih) (pre_eh > 0 ? 1 : slope),
//     du_ih = sum_{row i} dpre_eh,  dv_ch = sum_{column c} dpre_eh,  dz_c^h = sum_{column c} a_eh dY_r^h
//
// the column sums over row c of the transposed CSR, whose entry k comes from source row r = indices_t[k]; the column pass
// recomputes a and g from u_r, v_c, rowstat_r, t_r, dy_r and its own z_c, so it needs no mirror permutation.
//
// The forward is two launches: the row statistics m, zsum in the segmented form of dp_csr_edge_seg.h (a group of 4 / 16 /
// 64 lanes per row from the mean row length, lanes across the entries), then the aggregation, which reads them back.
//
// Launch form of the aggregation and of both backward passes (the one of dp_meanagg.hip): one wavefront per row, lanes
// across the W = H C feature columns.  A lane owns K = VEC * NCH columns ("slots"): slot k is column
// (k / VEC) * 64 VEC + lane * VEC + k % VEC, read with one 4-byte load (VEC = 1) or as part of a 16-byte load (VEC = 4: W,
// the leading dimension and the base allow it).  A 64-column chunk may straddle heads: every slot carries its own head,
// or every 16-byte quad does where C % 4 == 0 (UNI).  The row's neighbour ids are fetched 64 at a time as one coalesced
// load and handed round by readlane.  conv_pick is the one place that decides (dp_csr_gat_conv_plan reports it).  A hub
// row stays on its wave.
//
// Orders of summation (one each, so a second run gives the same bits):
//   m, zsum    per head: lane `sub` of the row's group of L takes entries beg + sub, beg + sub + L, .. ascending (maximum,
//              then the sum of exp(s - m)), then the DPP tree of dp_common.h over the group.
//   Y          per column: four partial sums, entry number q of a batch of 64 ids into partial q % 4 by fma while four
//              whole entries remain in the batch, the batch's last cnt % 4 entries into partial 0; (p0 + p1) + (p2 + p3).
//   mean       heads ascending, then one division by H.
//   g_eh       per lane the products dY z of its slots of head h by fma, slots ascending, then wave64_sum.
//   t, du, dv  entries ascending, one chain (t by fma).     dz  per column: entries ascending, one fma chain.
// No atomics, no LDS, plain vector stores, no workspace beyond rowstat [n, 2H] and t [n, H].
#include <math.h>

#include <type_traits>

#include "dp_csr_edge_seg.h"
#include "dp_entry.h"

namespace dp {
namespace {

constexpr int GC_THREADS = 256;                               // four waves, one row each

struct ConvPick {
    int vec, nch, uni, lanes;
};
// The one place that decides the launch form.  ld: the leading dimensions of everything gathered, or-ed (a multiple of 4
// only if all are); misaligned: one of the gathered bases is off the 16-byte grid (or, for the backward of the mean, a
// quad of dy would straddle heads).
ConvPick conv_pick(long n_rows, long nnz, int W, int C, int ld, bool misaligned) {
    ConvPick k;
    k.lanes = eo_lanes(n_rows, nnz);                           // the statistics pass: edge_pick's rule
    k.vec = (W % 4 == 0 && ld % 4 == 0 && !misaligned) ? 4 : 1;
    const int need = (W + 64 * k.vec - 1) / (64 * k.vec);
    k.nch = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
    k.uni = (k.vec == 4 && C % 4 == 0) ? 1 : 0;
    return k;
}

__device__ __forceinline__ float gc_leaky(float pre, float slope) { return pre > 0.f ? pre : slope * pre; }

// The columns of a lane: K slots in NG coefficient groups of CG slots (one head each).
template <int VEC, int NCH, bool UNI>
struct Slots {
    static constexpr int K = VEC * NCH, CG = UNI ? 4 : 1, NG = K / CG;
    int col[K];          // clamped into [0, W): a slot beyond W reads what the last one reads and stores nothing
    bool on[K];
    int head[NG];
    __device__ __forceinline__ Slots(int lane, int W, int C) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = (k / VEC) * 64 * VEC + lane * VEC + k % VEC;
            on[k] = c < W;
            col[k] = on[k] ? c : W - VEC + k % VEC;
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) head[g] = col[g * CG] / C;
    }
    // the lane that owns the first column of its group's head writes that head's per-node results
    __device__ __forceinline__ bool owner(int g, int C) const { return on[g * CG] && col[g * CG] == head[g] * C; }
};

// the K slots of row `r` of x (at the slots' own columns, or at idx[k])
template <int VEC, int K>
__device__ __forceinline__ void gc_load(const float* __restrict__ x, long r, int ld, const int (&idx)[K], float (&out)[K]) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(x + r * ld + idx[4 * q]);
            out[4 * q] = t.x, out[4 * q + 1] = t.y, out[4 * q + 2] = t.z, out[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = x[r * ld + idx[k]];
    }
}

// g_eh for the head of every group of the lane: the lane's products of head h by fma, slots ascending, wave64_sum, heads
// ascending.  Both backward passes call it with (dY, z) in this order, so they get the same bits.
template <class S>
__device__ __forceinline__ void gc_head_dots(const S& sl, int H, const float (&dY)[S::K], const float (&zr)[S::K],
                                             float (&gs)[S::NG]) {
    float pg[S::NG];
#pragma unroll
    for (int g = 0; g < S::NG; ++g) {
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < S::CG; ++k) p = fmaf(dY[g * S::CG + k], zr[g * S::CG + k], p);
        pg[g] = sl.on[g * S::CG] ? p : 0.f;
        gs[g] = 0.f;
    }
    for (int h = 0; h < H; ++h) {
        float x = 0.f;
#pragma unroll
        for (int g = 0; g < S::NG; ++g) x += sl.head[g] == h ? pg[g] : 0.f;
        const float G = wave64_sum(x);
#pragma unroll
        for (int g = 0; g < S::NG; ++g) gs[g] = sl.head[g] == h ? G : gs[g];
    }
}

// rowstat [n, 2H]: m, then zsum, per head; zeros for a row without entries.  A group of L lanes per row, head after head.
template <int L>
__global__ __launch_bounds__(EO_THREADS) void k_gatc_stats(const float* __restrict__ u, int ldu,
                                                           const float* __restrict__ v, int ldv,
                                                           const int* __restrict__ indptr,
                                                           const int* __restrict__ indices, float* __restrict__ rowstat,
                                                           int n_rows, int H, float slope) {
    const Seg g = eo_seg<L>(indptr, n_rows);
    const bool any = g.end > g.beg;
    for (int h = 0; h < H; ++h) {
        const float ui = g.live ? u[(long)g.row * ldu + h] : 0.f;
        float m = -INFINITY, s = 0.f;
        for (int e = g.beg + g.sub; e < g.end; e += L) m = fmaxf(m, gc_leaky(ui + v[(long)indices[e] * ldv + h], slope));
        const float M = eo_max<L>(m);
        for (int e = g.beg + g.sub; e < g.end; e += L) s += expf(gc_leaky(ui + v[(long)indices[e] * ldv + h], slope) - M);
        const float Z = eo_sum<L>(s);
        if (g.live && g.sub == 0) {
            rowstat[(long)g.row * (2 * H) + h] = any ? M : 0.f;
            rowstat[(long)g.row * (2 * H) + H + h] = any ? Z : 0.f;
        }
    }
}

// y from z, u, v and the rowstat of k_gatc_stats.
template <int VEC, int NCH, bool UNI>
__global__ __launch_bounds__(GC_THREADS) void k_gatc_fwd(const float* __restrict__ z, int ldz,
                                                         const float* __restrict__ u, int ldu,
                                                         const float* __restrict__ v, int ldv,
                                                         const int* __restrict__ indptr,
                                                         const int* __restrict__ indices, float* __restrict__ y, int ldy,
                                                         const float* __restrict__ rowstat, int n_rows, int H, int C,
                                                         float slope, int mean) {
    using S = Slots<VEC, NCH, UNI>;
    constexpr int K = S::K, CG = S::CG, NG = S::NG;
    const long row = (long)blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                 // wave-uniform
    const int lane = threadIdx.x & 63, W = H * C;
    const int beg = indptr[row], end = indptr[row + 1];
    const S sl(lane, W, C);
    if (end == beg) {
        if (mean) {
            for (int c = lane; c < C; c += 64) y[row * ldy + c] = 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (sl.on[k]) y[row * ldy + sl.col[k]] = 0.f;
        }
        return;
    }
    float ug[NG], mg[NG], zg[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ug[g] = u[row * ldu + sl.head[g]];
        mg[g] = rowstat[row * (2 * H) + sl.head[g]];
        zg[g] = rowstat[row * (2 * H) + H + sl.head[g]];
    }
    // the aggregation: lanes across the columns, four neighbour rows in flight
    float acc[4][K];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[q][k] = 0.f;
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);
        const int mine = indices[e0 + min(lane, cnt - 1)];
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            long r[4];
            float zr[4][K], vj[4][NG];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                r[q] = __builtin_amdgcn_readlane(mine, j + q);
                gc_load<VEC, K>(z, r[q], ldz, sl.col, zr[q]);
#pragma unroll
                for (int g = 0; g < NG; ++g) vj[q][g] = v[r[q] * ldv + sl.head[g]];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float a = expf(gc_leaky(ug[g] + vj[q][g], slope) - mg[g]) / zg[g];
#pragma unroll
                    for (int k = 0; k < CG; ++k) acc[q][g * CG + k] = fmaf(a, zr[q][g * CG + k], acc[q][g * CG + k]);
                }
        }
        for (; j < cnt; ++j) {
            const long r = __builtin_amdgcn_readlane(mine, j);
            float zr[K];
            gc_load<VEC, K>(z, r, ldz, sl.col, zr);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float a = expf(gc_leaky(ug[g] + v[r * ldv + sl.head[g]], slope) - mg[g]) / zg[g];
#pragma unroll
                for (int k = 0; k < CG; ++k) acc[0][g * CG + k] = fmaf(a, zr[g * CG + k], acc[0][g * CG + k]);
            }
        }
    }
    float Y[K];
#pragma unroll
    for (int k = 0; k < K; ++k) Y[k] = (acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]);
    if (!mean) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (sl.on[k]) y[row * ldy + sl.col[k]] = Y[k];
        return;
    }
    // the mean over the heads: output column c takes column h C + c of every head from the lane and slot that own it
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = min(c0 + lane, C - 1);
        float sum = 0.f;
        for (int h = 0; h < H; ++h) {
            const int x = h * C + c;
            const int src_lane = (x % (64 * VEC)) / VEC, src_slot = (x / (64 * VEC)) * VEC + x % VEC;
            float val = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float t = __shfl(Y[k], src_lane, 64);
                val = src_slot == k ? t : val;
            }
            sum = h == 0 ? val : sum + val;
        }
        if (c0 + lane < C) y[row * ldy + c] = sum / (float)H;
    }
}

// the columns of dy that the slots read, and the scale of dY
template <class S>
__device__ __forceinline__ void gc_dy_cols(const S& sl, int C, int mean, int (&dyc)[S::K]) {
#pragma unroll
    for (int k = 0; k < S::K; ++k) dyc[k] = mean ? sl.col[k] % C : sl.col[k];
}
template <int K>
__device__ __forceinline__ void gc_scale(float (&dY)[K], int H, int mean) {
    if (mean) {
#pragma unroll
        for (int k = 0; k < K; ++k) dY[k] = dY[k] / (float)H;
    }
}

// Over the rows: t (first sweep), then du (second sweep), every coefficient recomputed from u, v and rowstat.
template <int VEC, int NCH, bool UNI>
__global__ __launch_bounds__(GC_THREADS) void k_gatc_bwd_rows(const float* __restrict__ z, int ldz,
                                                              const float* __restrict__ u, int ldu,
                                                              const float* __restrict__ v, int ldv,
                                                              const int* __restrict__ indptr,
                                                              const int* __restrict__ indices,
                                                              const float* __restrict__ rowstat,
                                                              const float* __restrict__ dy, int lddy,
                                                              float* __restrict__ tdot, float* __restrict__ du, int lddu,
                                                              int n, int H, int C, float slope, int mean) {
    using S = Slots<VEC, NCH, UNI>;
    constexpr int K = S::K, NG = S::NG;
    const long row = (long)blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63, W = H * C;
    const int beg = indptr[row], end = indptr[row + 1];
    if (end == beg) {
        if (lane < H) tdot[row * H + lane] = 0.f, du[row * lddu + lane] = 0.f;
        return;
    }
    const S sl(lane, W, C);
    int dyc[K];
    float dY[K], ug[NG], mg[NG], zg[NG], t[NG], acc[NG];
    gc_dy_cols(sl, C, mean, dyc);
    gc_load<VEC, K>(dy, row, lddy, dyc, dY);
    gc_scale<K>(dY, H, mean);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ug[g] = u[row * ldu + sl.head[g]];
        mg[g] = rowstat[row * (2 * H) + sl.head[g]];
        zg[g] = rowstat[row * (2 * H) + H + sl.head[g]];
        t[g] = 0.f;
        acc[g] = 0.f;
    }
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int e0 = beg; e0 < end; e0 += 64) {
            const int cnt = min(64, end - e0);
            const int mine = indices[e0 + min(lane, cnt - 1)];
            for (int j = 0; j < cnt; j += 2) {
                // two neighbour rows in flight (the second repeats the first at an odd end and is not used)
                const bool two = j + 1 < cnt;
                const long r0 = __builtin_amdgcn_readlane(mine, j), r1 = __builtin_amdgcn_readlane(mine, two ? j + 1 : j);
                float z0[K], z1[K], v0[NG], v1[NG], gs[NG];
                gc_load<VEC, K>(z, r0, ldz, sl.col, z0);
                gc_load<VEC, K>(z, r1, ldz, sl.col, z1);
#pragma unroll
                for (int g = 0; g < NG; ++g) v0[g] = v[r0 * ldv + sl.head[g]], v1[g] = v[r1 * ldv + sl.head[g]];
                gc_head_dots(sl, H, dY, z0, gs);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float pre = ug[g] + v0[g];
                    const float a = expf(gc_leaky(pre, slope) - mg[g]) / zg[g];
                    if (sweep == 0) t[g] = fmaf(a, gs[g], t[g]);
                    else acc[g] += (a * (gs[g] - t[g])) * (pre > 0.f ? 1.f : slope);
                }
                if (two) {                                     // wave-uniform
                    gc_head_dots(sl, H, dY, z1, gs);
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const float pre = ug[g] + v1[g];
                        const float a = expf(gc_leaky(pre, slope) - mg[g]) / zg[g];
                        if (sweep == 0) t[g] = fmaf(a, gs[g], t[g]);
                        else acc[g] += (a * (gs[g] - t[g])) * (pre > 0.f ? 1.f : slope);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
        if (sl.owner(g, C)) {
            tdot[row * H + sl.head[g]] = t[g];
            du[row * lddu + sl.head[g]] = acc[g];
        }
}

// Over the transposed rows: entry k of row c is the stored entry (r, c), r = indices_t[k]; a, g and dpre are recomputed
// from u_r, v_c, the SOURCE row's rowstat_r and t_r, dy_r and the column's own z_c.
template <int VEC, int NCH, bool UNI>
__global__ __launch_bounds__(GC_THREADS) void k_gatc_bwd_cols(const float* __restrict__ z, int ldz,
                                                              const float* __restrict__ u, int ldu,
                                                              const float* __restrict__ v, int ldv,
                                                              const int* __restrict__ indptr_t,
                                                              const int* __restrict__ indices_t,
                                                              const float* __restrict__ rowstat,
                                                              const float* __restrict__ tdot,
                                                              const float* __restrict__ dy, int lddy,
                                                              float* __restrict__ dv, int lddv, float* __restrict__ dz,
                                                              int lddz, int n, int H, int C, float slope, int mean) {
    using S = Slots<VEC, NCH, UNI>;
    constexpr int K = S::K, CG = S::CG, NG = S::NG;
    const long row = (long)blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63, W = H * C;
    const int beg = indptr_t[row], end = indptr_t[row + 1];
    const S sl(lane, W, C);
    if (end == beg) {
        if (lane < H) dv[row * lddv + lane] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (sl.on[k]) dz[row * lddz + sl.col[k]] = 0.f;
        return;
    }
    int dyc[K];
    float zc[K], vg[NG], dvacc[NG], dzacc[K];
    gc_dy_cols(sl, C, mean, dyc);
    gc_load<VEC, K>(z, row, ldz, sl.col, zc);
#pragma unroll
    for (int g = 0; g < NG; ++g) vg[g] = v[row * ldv + sl.head[g]], dvacc[g] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) dzacc[k] = 0.f;
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);
        const int mine = indices_t[e0 + min(lane, cnt - 1)];
        for (int j = 0; j < cnt; ++j) {
            const long r = __builtin_amdgcn_readlane(mine, j);
            float dY[K], gs[NG], ur[NG], mr[NG], zr[NG], tr[NG];
            gc_load<VEC, K>(dy, r, lddy, dyc, dY);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                ur[g] = u[r * ldu + sl.head[g]];
                mr[g] = rowstat[r * (2 * H) + sl.head[g]];
                zr[g] = rowstat[r * (2 * H) + H + sl.head[g]];
                tr[g] = tdot[r * H + sl.head[g]];
            }
            gc_scale<K>(dY, H, mean);
            gc_head_dots(sl, H, dY, zc, gs);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float pre = ur[g] + vg[g];
                const float a = expf(gc_leaky(pre, slope) - mr[g]) / zr[g];
                dvacc[g] += (a * (gs[g] - tr[g])) * (pre > 0.f ? 1.f : slope);
#pragma unroll
                for (int k = 0; k < CG; ++k) dzacc[g * CG + k] = fmaf(a, dY[g * CG + k], dzacc[g * CG + k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (sl.on[k]) dz[row * lddz + sl.col[k]] = dzacc[k];
#pragma unroll
    for (int g = 0; g < NG; ++g)
        if (sl.owner(g, C)) dv[row * lddv + sl.head[g]] = dvacc[g];
}

template <int V>
using ic = std::integral_constant<int, V>;

// f(ic<VEC>, ic<NCH>, ic<UNI>) of the picked form: VEC = 1 with 1 / 2 / 4 / 8 chunks of 64 columns, VEC = 4 with 1 / 2
// chunks of 256 and either head form
template <class F>
void conv_dispatch(const ConvPick& k, F&& f) {
    if (k.vec == 4) {
        if (k.nch == 1) k.uni ? f(ic<4>{}, ic<1>{}, ic<1>{}) : f(ic<4>{}, ic<1>{}, ic<0>{});
        else k.uni ? f(ic<4>{}, ic<2>{}, ic<1>{}) : f(ic<4>{}, ic<2>{}, ic<0>{});
    } else if (k.nch == 1) f(ic<1>{}, ic<1>{}, ic<0>{});
    else if (k.nch == 2) f(ic<1>{}, ic<2>{}, ic<0>{});
    else if (k.nch == 4) f(ic<1>{}, ic<4>{}, ic<0>{});
    else f(ic<1>{}, ic<8>{}, ic<0>{});
}

// the shape checks of the three entries
int conv_shape(int H, int C) {
    DP_CHECK(H >= 1 && H <= DP_CSR_GAT_MAX_HEADS, DP_ERR_INVALID_ARG, "H=%d must be 1 .. %d", H, DP_CSR_GAT_MAX_HEADS);
    DP_CHECK(C >= 1, DP_ERR_INVALID_ARG, "C=%d must be positive", C);
    DP_CHECK((long)H * C <= DP_CSR_GAT_CONV_MAX_WIDTH, DP_ERR_UNSUPPORTED, "H * C = %ld outside the supported 1..%d",
             (long)H * C, DP_CSR_GAT_CONV_MAX_WIDTH);
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

#define GC_SHAPE(H, C) DP_TRY(conv_shape(H, C))
#define GC_FLAGS(slope, mean_heads)                                                                      \
    do {                                                                                                 \
        DP_CHECK(isfinite(slope), DP_ERR_INVALID_ARG, "slope must be finite");                           \
        DP_CHECK((mean_heads) == 0 || (mean_heads) == 1, DP_ERR_INVALID_ARG, "mean_heads=%d must be 0 or 1", \
                 (int)(mean_heads));                                                                     \
    } while (0)

extern "C" {

int dp_csr_gat_conv_plan(int n_rows, int nnz, int H, int C, int ldz, int z_misaligned, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    GC_SHAPE(H, C);
    DP_LD(ldz, H * C);
    const ConvPick k = conv_pick(n_rows, nnz, H * C, C, ldz, z_misaligned != 0);
    const int plan[DP_CSR_GAT_CONV_PLAN_INTS] = {k.vec, k.nch, k.uni, GC_THREADS / 64, k.vec * k.nch, k.lanes};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

int dp_csr_gat_conv_fwd(const float* z, int ldz, const float* u, int ldu, const float* v, int ldv, const int* indptr,
                        const int* indices, float* y, int ldy, float* rowstat, int n_rows, int nnz, int H, int C,
                        float slope, int mean_heads, void* stream) {
    DP_PTR(z); DP_PTR(u); DP_PTR(v); DP_PTR(indptr); DP_PTR(indices); DP_PTR(y); DP_PTR(rowstat);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    GC_SHAPE(H, C);
    GC_FLAGS(slope, mean_heads);
    DP_LD(ldz, H * C);
    DP_LD(ldu, H);
    DP_LD(ldv, H);
    DP_LD(ldy, mean_heads ? C : H * C);
    if (n_rows == 0) return DP_OK;
    // nnz == 0: every row is empty, the launches write the zero rowstat and y (indptr all zero)
    Seq q(DP_STREAM(stream), nullptr, 0);
    const ConvPick k = conv_pick(n_rows, nnz, H * C, C, ldz, !aligned16(z));
    const dim3 sgrid(cdiv(n_rows, EO_THREADS / k.lanes)), sblock(EO_THREADS);
    if (k.lanes == 4)
        hipLaunchKernelGGL(k_gatc_stats<4>, sgrid, sblock, 0, q.stream, u, ldu, v, ldv, indptr, indices, rowstat, n_rows, H,
                           slope);
    else if (k.lanes == 16)
        hipLaunchKernelGGL(k_gatc_stats<16>, sgrid, sblock, 0, q.stream, u, ldu, v, ldv, indptr, indices, rowstat, n_rows,
                           H, slope);
    else
        hipLaunchKernelGGL(k_gatc_stats<64>, sgrid, sblock, 0, q.stream, u, ldu, v, ldv, indptr, indices, rowstat, n_rows,
                           H, slope);
    q.check_launch("k_gatc_stats");
    if (!q.ok()) return q.err;
    const dim3 grid(cdiv(n_rows, GC_THREADS / 64)), block(GC_THREADS);
    conv_dispatch(k, [&](auto vc, auto nc, auto uc) {
        hipLaunchKernelGGL((k_gatc_fwd<decltype(vc)::value, decltype(nc)::value, decltype(uc)::value != 0>), grid, block,
                           0, q.stream, z, ldz, u, ldu, v, ldv, indptr, indices, y, ldy, (const float*)rowstat, n_rows, H, C,
                           slope, mean_heads);
    });
    q.check_launch("k_gatc_fwd");
    return q.err;
}

int dp_csr_gat_conv_bwd(const float* z, int ldz, const float* u, int ldu, const float* v, int ldv, const int* indptr,
                        const int* indices, const int* indptr_t, const int* indices_t, const float* rowstat,
                        const float* dy, int lddy, float* tdot, float* du, int lddu, float* dv, int lddv, float* dz,
                        int lddz, int n, int nnz, int H, int C, float slope, int mean_heads, void* stream) {
    DP_PTR(z); DP_PTR(u); DP_PTR(v); DP_PTR(indptr); DP_PTR(indices); DP_PTR(indptr_t); DP_PTR(indices_t);
    DP_PTR(rowstat); DP_PTR(dy); DP_PTR(tdot); DP_PTR(du); DP_PTR(dv); DP_PTR(dz);
    DP_NONNEG(n);
    DP_NONNEG(nnz);
    GC_SHAPE(H, C);
    GC_FLAGS(slope, mean_heads);
    DP_LD(ldz, H * C);
    DP_LD(ldu, H);
    DP_LD(ldv, H);
    DP_LD(lddy, mean_heads ? C : H * C);
    DP_LD(lddu, H);
    DP_LD(lddv, H);
    DP_LD(lddz, H * C);
    if (n == 0) return DP_OK;
    // nnz == 0: every row and every column is empty, the two launches write the zero t, du, dv, dz
    Seq q(DP_STREAM(stream), nullptr, 0);
    // both passes gather with one form: z (rows) and dy (columns) must both allow the 16-byte loads, and a quad of the
    // mean's dy [n, C] must not straddle heads
    const ConvPick k =
        conv_pick(n, nnz, H * C, C, ldz | lddy, !aligned16(z) || !aligned16(dy) || (mean_heads && C % 4 != 0));
    const dim3 grid(cdiv(n, GC_THREADS / 64)), block(GC_THREADS);
    conv_dispatch(k, [&](auto vc, auto nc, auto uc) {
        hipLaunchKernelGGL((k_gatc_bwd_rows<decltype(vc)::value, decltype(nc)::value, decltype(uc)::value != 0>), grid,
                           block, 0, q.stream, z, ldz, u, ldu, v, ldv, indptr, indices, rowstat, dy, lddy, tdot, du, lddu,
                           n, H, C, slope, mean_heads);
    });
    q.check_launch("k_gatc_bwd_rows");
    if (!q.ok()) return q.err;
    conv_dispatch(k, [&](auto vc, auto nc, auto uc) {
        hipLaunchKernelGGL((k_gatc_bwd_cols<decltype(vc)::value, decltype(nc)::value, decltype(uc)::value != 0>), grid,
                           block, 0, q.stream, z, ldz, u, ldu, v, ldv, indptr_t, indices_t, rowstat, (const float*)tdot,
                           dy, lddy, dv, lddv, dz, lddz, n, H, C, slope, mean_heads);
    });
    q.check_launch("k_gatc_bwd_cols");
    return q.err;
}

}  // extern "C"
