// Multi-head additive (GAT) edge attention on a CSR adjacency: scores, softmax over each neighbour list and
// the mean over the heads in ONE segmented pass over the stored entries, nothing of size nnz * H ever written.
//
//     pre_eh = u_ih + v_jh,  s_eh = pre_eh > 0 ? pre_eh : slope * pre_eh       (e = (i, j), j = indices[e]; derivative
//     a_eh   = exp(s_eh - m_ih) / z_ih                                          `slope` AT 0, as torch's leaky_relu)
//     out_e  = (sum_h a_eh) / H                                                 heads ascending, one division
//
// and its backward, g_e = dout_e / H:
//
//     t_ih = sum_{row i} a_eh g_e,  dpre_eh = a_eh (g_e - t_ih) (pre_eh > 0 ? 1 : slope),
//     du_ih = sum_{row i} dpre_eh,  dv_ch = sum_{column c} dpre_eh              (row c of the transposed CSR; its entry k
//                                                                               is the stored entry mirror[k])
//
// The score is a function of two per-node scalars per head, so the backward recomputes every coefficient from u, v and
// the forward's rowstat [n, 2H] (m, then z).  The launch form is the one of dp_csr_edge_ops.hip (dp_csr_edge_seg.h): a
// group of 4 / 16 / 64 lanes per row from the mean row length, lane `sub` on entries beg + sub, beg + sub + L, ...; the H
// values of v_j are contiguous and are read with 16-byte loads where H, ldv and the base allow (VEC = 4), with 4-byte
// loads otherwise.  gat_pick is the one place that decides (dp_csr_gat_plan reports it).  Every sum has one order: the
// lane's entries ascending, then the DPP tree of dp_common.h, outside every branch.  No atomics, no LDS, plain vector
// stores.
#include <math.h>

#include <type_traits>

#include "dp_csr_edge_seg.h"
#include "dp_entry.h"

namespace dp {
namespace {

struct GatPick {
    int lanes, vec, regs, rows_per_wg;
};

// entries a lane keeps in registers: H scores per entry, 16 floats at the most (8 / 4 entries as the edge softmax where
// H allows)
constexpr int gat_regs(int lanes, int H) {
    const int base = lanes == 4 ? 8 : 4, cap = 16 / H;
    return base < cap ? base : cap;
}
constexpr bool gat_vec_ok(int H, int ld, bool misaligned) { return H % 4 == 0 && ld % 4 == 0 && !misaligned; }
// The one place that decides the launch form: the lane group by the rule of edge_pick (the mean row in two visits), the
// load form of the H contiguous values of a node, the register-held entries.
GatPick gat_pick(long n_rows, long nnz, int H, int ldv, bool v_misaligned) {
    GatPick k;
    k.lanes = eo_lanes(n_rows, nnz);
    k.vec = gat_vec_ok(H, ldv, v_misaligned) ? 4 : 1;
    k.regs = gat_regs(k.lanes, H);
    k.rows_per_wg = EO_THREADS / k.lanes;
    return k;
}

// the H contiguous values of one node: H / 4 loads of 16 bytes, or H of 4
template <int H, int VEC>
__device__ __forceinline__ void gat_load(const float* __restrict__ p, float (&x)[H]) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int q = 0; q < H / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * q);
            x[4 * q] = t.x, x[4 * q + 1] = t.y, x[4 * q + 2] = t.z, x[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int h = 0; h < H; ++h) x[h] = p[h];
    }
}
__device__ __forceinline__ float gat_leaky(float pre, float slope) { return pre > 0.f ? pre : slope * pre; }

// out [nnz] and rowstat [n, 2H] (m, z; zeros for a row without entries).  A row of at most L * R entries is read once; a
// longer one runs the per-lane running maximum and sum per head and is read a second time.
template <int L, int H, int VEC>
__global__ __launch_bounds__(EO_THREADS) void k_gat_fwd(const float* __restrict__ u, int ldu,
                                                        const float* __restrict__ v, int ldv,
                                                        const int* __restrict__ indptr,
                                                        const int* __restrict__ indices, float* __restrict__ out,
                                                        float* __restrict__ rowstat, int n_rows, float slope) {
    constexpr int R = gat_regs(L, H);
    const Seg g = eo_seg<L>(indptr, n_rows);
    const bool fits = g.end - g.beg <= L * R;
    float ui[H], m[H], sum[H], s[R][H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        ui[h] = g.live ? u[(long)g.row * ldu + h] : 0.f;
        m[h] = -INFINITY;
        sum[h] = 0.f;
    }
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            if (e < g.end) {
                float vj[H];
                gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    s[k][h] = gat_leaky(ui[h] + vj[h], slope);
                    m[h] = fmaxf(m[h], s[k][h]);
                }
            } else {
#pragma unroll
                for (int h = 0; h < H; ++h) s[k][h] = -INFINITY;
            }
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) {      // running maximum and sum (exp(-inf) = 0 starts it)
            float vj[H];
            gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const float x = gat_leaky(ui[h] + vj[h], slope);
                const float mn = fmaxf(m[h], x);
                sum[h] = sum[h] * expf(m[h] - mn) + expf(x - mn);
                m[h] = mn;
            }
        }
    }
    float M[H], S[H];
#pragma unroll
    for (int h = 0; h < H; ++h) M[h] = eo_max<L>(m[h]);
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
            for (int h = 0; h < H; ++h) {
                s[k][h] = expf(s[k][h] - M[h]);               // a slot beyond the row: exp(-inf) = 0
                sum[h] += s[k][h];
            }
        }
    } else {
#pragma unroll
        for (int h = 0; h < H; ++h) sum[h] = sum[h] * expf(m[h] - M[h]);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) S[h] = eo_sum<L>(sum[h]);
    if (g.live && g.sub == 0) {
        const bool any = g.end > g.beg;
        float* rs = rowstat + (long)g.row * (2 * H);
#pragma unroll
        for (int h = 0; h < H; ++h) {
            rs[h] = any ? M[h] : 0.f;
            rs[H + h] = any ? S[h] : 0.f;
        }
    }
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            if (e < g.end) {
                float acc = s[k][0] / S[0];
#pragma unroll
                for (int h = 1; h < H; ++h) acc += s[k][h] / S[h];
                out[e] = acc / (float)H;
            }
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) {
            float vj[H];
            gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const float a = expf(gat_leaky(ui[h] + vj[h], slope) - M[h]) / S[h];
                acc = h == 0 ? a : acc + a;
            }
            out[e] = acc / (float)H;
        }
    }
}

// Over the rows: a recomputed from u, v and rowstat, t = sum a g, then du = sum a (g - t) s'; t goes to tdot [n, H].
template <int L, int H, int VEC>
__global__ __launch_bounds__(EO_THREADS) void k_gat_bwd_rows(const float* __restrict__ u, int ldu,
                                                             const float* __restrict__ v, int ldv,
                                                             const int* __restrict__ indptr,
                                                             const int* __restrict__ indices,
                                                             const float* __restrict__ rowstat,
                                                             const float* __restrict__ dout,
                                                             float* __restrict__ tdot, float* __restrict__ du,
                                                             int lddu, int n_rows, float slope) {
    constexpr int R = gat_regs(L, H);
    const Seg g = eo_seg<L>(indptr, n_rows);
    const bool fits = g.end - g.beg <= L * R;
    const bool any = g.end > g.beg;
    float ui[H], mi[H], zi[H], acc[H], a[R][H], gv[R];
    unsigned pos = 0;                                          // bit k * H + h: pre > 0 (R * H <= 16)
#pragma unroll
    for (int h = 0; h < H; ++h) {
        ui[h] = g.live ? u[(long)g.row * ldu + h] : 0.f;
        mi[h] = any ? rowstat[(long)g.row * (2 * H) + h] : 0.f;
        zi[h] = any ? rowstat[(long)g.row * (2 * H) + H + h] : 1.f;
        acc[h] = 0.f;
    }
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = g.beg + k * L + g.sub;
            if (e < g.end) {
                float vj[H];
                gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
                gv[k] = dout[e] / (float)H;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const float pre = ui[h] + vj[h];
                    pos |= (pre > 0.f ? 1u : 0u) << (k * H + h);
                    a[k][h] = expf(gat_leaky(pre, slope) - mi[h]) / zi[h];
                    acc[h] = fmaf(a[k][h], gv[k], acc[h]);
                }
            } else {
                gv[k] = 0.f;
#pragma unroll
                for (int h = 0; h < H; ++h) a[k][h] = 0.f;
            }
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) {
            float vj[H];
            gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
            const float ge = dout[e] / (float)H;
#pragma unroll
            for (int h = 0; h < H; ++h)
                acc[h] = fmaf(expf(gat_leaky(ui[h] + vj[h], slope) - mi[h]) / zi[h], ge, acc[h]);
        }
    }
    float t[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        t[h] = eo_sum<L>(acc[h]);
        acc[h] = 0.f;
    }
    if (fits) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
            for (int h = 0; h < H; ++h)
                acc[h] += (a[k][h] * (gv[k] - t[h])) * ((pos >> (k * H + h)) & 1u ? 1.f : slope);
        }
    } else {
        for (int e = g.beg + g.sub; e < g.end; e += L) {
            float vj[H];
            gat_load<H, VEC>(v + (long)indices[e] * ldv, vj);
            const float ge = dout[e] / (float)H;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const float pre = ui[h] + vj[h];
                const float ae = expf(gat_leaky(pre, slope) - mi[h]) / zi[h];
                acc[h] += (ae * (ge - t[h])) * (pre > 0.f ? 1.f : slope);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const float d = eo_sum<L>(acc[h]);
        if (g.live && g.sub == 0) {
            tdot[(long)g.row * H + h] = t[h];
            du[(long)g.row * lddu + h] = d;
        }
    }
}

// Over the transposed rows: entry k of row c is the stored entry mirror[k] = (r, c), r = indices_t[k]; its coefficient is
// recomputed from u_r, v_c and the SOURCE row's rowstat_r and t_r.  VEC = 4: the H values of u_r, and the 2H of rowstat_r
// and H of tdot_r, by 16-byte loads.
template <int L, int H, int VEC>
__global__ __launch_bounds__(EO_THREADS) void k_gat_bwd_cols(const float* __restrict__ u, int ldu,
                                                             const float* __restrict__ v, int ldv,
                                                             const int* __restrict__ indptr_t,
                                                             const int* __restrict__ indices_t,
                                                             const int* __restrict__ mirror,
                                                             const float* __restrict__ rowstat,
                                                             const float* __restrict__ tdot,
                                                             const float* __restrict__ dout, float* __restrict__ dv,
                                                             int lddv, int n, float slope) {
    const Seg g = eo_seg<L>(indptr_t, n);
    float vc[H], acc[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        vc[h] = g.live ? v[(long)g.row * ldv + h] : 0.f;
        acc[h] = 0.f;
    }
    for (int k = g.beg + g.sub; k < g.end; k += L) {
        const int r = indices_t[k];
        const float ge = dout[mirror[k]] / (float)H;
        float ur[H], mr[H], zr[H], tr[H];
        gat_load<H, VEC>(u + (long)r * ldu, ur);
        gat_load<H, VEC>(rowstat + (long)r * (2 * H), mr);
        gat_load<H, VEC>(rowstat + (long)r * (2 * H) + H, zr);
        gat_load<H, VEC>(tdot + (long)r * H, tr);
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const float pre = ur[h] + vc[h];
            const float ae = expf(gat_leaky(pre, slope) - mr[h]) / zr[h];
            acc[h] += (ae * (ge - tr[h])) * (pre > 0.f ? 1.f : slope);
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const float d = eo_sum<L>(acc[h]);
        if (g.live && g.sub == 0) dv[(long)g.row * lddv + h] = d;
    }
}

template <int V>
using ic = std::integral_constant<int, V>;

// f(ic<L>, ic<H>, ic<VEC>) of the picked form; VEC = 4 exists for H = 4 and 8 only
template <class F>
void gat_dispatch(int lanes, int H, int vec, F&& f) {
    auto by_lanes = [&](auto hc, auto vc) {
        if (lanes == 4) f(ic<4>{}, hc, vc);
        else if (lanes == 16) f(ic<16>{}, hc, vc);
        else f(ic<64>{}, hc, vc);
    };
    auto by_vec = [&](auto hc) {
        if constexpr (decltype(hc)::value % 4 == 0) {
            if (vec == 4) return by_lanes(hc, ic<4>{});
        }
        by_lanes(hc, ic<1>{});
    };
    switch (H) {
        case 1: by_vec(ic<1>{}); break;
        case 2: by_vec(ic<2>{}); break;
        case 3: by_vec(ic<3>{}); break;
        case 4: by_vec(ic<4>{}); break;
        case 5: by_vec(ic<5>{}); break;
        case 6: by_vec(ic<6>{}); break;
        case 7: by_vec(ic<7>{}); break;
        default: by_vec(ic<8>{}); break;
    }
}

}  // namespace
}  // namespace dp

using namespace dp;

#define GAT_HEADS(H)                                                                                        \
    DP_CHECK((H) >= 1 && (H) <= DP_CSR_GAT_MAX_HEADS, DP_ERR_INVALID_ARG, "H=%d must be 1 .. %d", (int)(H), \
             DP_CSR_GAT_MAX_HEADS)
#define GAT_LD(ld, H) DP_CHECK((ld) >= (H), DP_ERR_INVALID_ARG, #ld "=%d smaller than H=%d", (int)(ld), (int)(H))
#define GAT_SLOPE(s) DP_CHECK(isfinite(s), DP_ERR_INVALID_ARG, "slope must be finite")

extern "C" {

int dp_csr_gat_plan(int n_rows, int nnz, int H, int ldv, int v_misaligned, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    GAT_HEADS(H);
    GAT_LD(ldv, H);
    const GatPick k = gat_pick(n_rows, nnz, H, ldv, v_misaligned != 0);
    const int plan[DP_CSR_GAT_PLAN_INTS] = {k.lanes, k.vec, k.regs, k.rows_per_wg, k.lanes * k.regs};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

int dp_csr_gat_fwd(const float* u, int ldu, const float* v, int ldv, const int* indptr, const int* indices, float* out,
                   float* rowstat, int n_rows, int nnz, int H, float slope, void* stream) {
    DP_PTR(u); DP_PTR(v); DP_PTR(indptr); DP_PTR(indices); DP_PTR(out); DP_PTR(rowstat);
    DP_NONNEG(n_rows);
    DP_NONNEG(nnz);
    GAT_HEADS(H);
    GAT_LD(ldu, H);
    GAT_LD(ldv, H);
    GAT_SLOPE(slope);
    if (n_rows == 0 || nnz == 0) return DP_OK;
    Seq q(DP_STREAM(stream), nullptr, 0);
    const GatPick k = gat_pick(n_rows, nnz, H, ldv, !aligned16(v));
    const dim3 grid(cdiv(n_rows, k.rows_per_wg)), block(EO_THREADS);
    gat_dispatch(k.lanes, H, k.vec, [&](auto lc, auto hc, auto vc) {
        hipLaunchKernelGGL((k_gat_fwd<decltype(lc)::value, decltype(hc)::value, decltype(vc)::value>), grid, block, 0,
                           q.stream, u, ldu, v, ldv, indptr, indices, out, rowstat, n_rows, slope);
    });
    q.check_launch("k_gat_fwd");
    return q.err;
}

int dp_csr_gat_bwd(const float* u, int ldu, const float* v, int ldv, const int* indptr, const int* indices,
                   const int* indptr_t, const int* indices_t, const int* mirror, const float* rowstat,
                   const float* dout, float* tdot, float* du, int lddu, float* dv, int lddv, int n, int nnz, int H,
                   float slope, void* stream) {
    DP_PTR(u); DP_PTR(v); DP_PTR(indptr); DP_PTR(indices); DP_PTR(indptr_t); DP_PTR(indices_t); DP_PTR(mirror);
    DP_PTR(rowstat); DP_PTR(dout); DP_PTR(tdot); DP_PTR(du); DP_PTR(dv);
    DP_NONNEG(n);
    DP_NONNEG(nnz);
    GAT_HEADS(H);
    GAT_LD(ldu, H);
    GAT_LD(ldv, H);
    GAT_LD(lddu, H);
    GAT_LD(lddv, H);
    GAT_SLOPE(slope);
    if (n == 0) return DP_OK;
    // nnz == 0: every row and every column is empty, the two launches write the zero du, dv (indptr all zero)
    Seq q(DP_STREAM(stream), nullptr, 0);
    const GatPick k = gat_pick(n, nnz, H, ldv, !aligned16(v));
    const int vec_u = gat_vec_ok(H, ldu, !aligned16(u) || !aligned16(rowstat) || !aligned16(tdot)) ? 4 : 1;
    const dim3 grid(cdiv(n, k.rows_per_wg)), block(EO_THREADS);
    gat_dispatch(k.lanes, H, k.vec, [&](auto lc, auto hc, auto vc) {
        hipLaunchKernelGGL((k_gat_bwd_rows<decltype(lc)::value, decltype(hc)::value, decltype(vc)::value>), grid, block,
                           0, q.stream, u, ldu, v, ldv, indptr, indices, rowstat, dout, tdot, du, lddu, n, slope);
    });
    q.check_launch("k_gat_bwd_rows");
    if (!q.ok()) return q.err;
    gat_dispatch(k.lanes, H, vec_u, [&](auto lc, auto hc, auto vc) {
        hipLaunchKernelGGL((k_gat_bwd_cols<decltype(lc)::value, decltype(hc)::value, decltype(vc)::value>), grid, block,
                           0, q.stream, u, ldu, v, ldv, indptr_t, indices_t, mirror, rowstat, (const float*)tdot, dout,
                           dv, lddv, n, slope);
    });
    q.check_launch("k_gat_bwd_cols");
    return q.err;
}

}  // extern "C"
