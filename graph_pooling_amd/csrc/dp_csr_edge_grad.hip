// Gradients to the stored values of a CSR adjacency: a sampled dense-dense product over the stored
// entries e = (i, j), j = indices[e],
//
//     out[e] = beta * out[e] + alpha * d * epi( sum_f P[i,f] Q[j,f], a_e )
//
// with epi the identity, the cross-entropy link derivative log(1 - p + eps) - log(p + eps), p = min(t, 1), or the
// Frobenius derivative 2 (a_e - t).  GraphConv (P = dax, Q = x), the level-0 pooling (P = S dA', Q = S) and both link
// objectives (P = Q = S) are this one kernel family.
//
// Four rows per workgroup, one wave per (row, chunk of 512 entries): the chunks of the workgroup's rows form one list
// and wave w takes every fourth item, so a long row is spread over the waves and a row with no entry costs nothing but
// its two indptr words.  A group of L = 4 / 16 / 64 lanes serves one entry (the smallest that covers F in one visit of
// 16- or 4-byte lanes; 64 lanes and up to four visits above, then a column loop); the 64 / L groups of a wave take
// entries e0 + t * (64 / L) + g in step t.  As in dp_meanagg.hip the 64 column ids of a sub-chunk come in as ONE
// coalesced load and are handed round (readlane for the 64-lane tier, whose entry is wave-uniform; a lane permute for the
// narrow tiers, whose groups read different lanes), and four entries' Q rows are in flight before the first multiply.
// P_i is loaded once per item and stays in registers.  Each dot is summed in a fixed order (the lane's columns
// ascending, then a DPP tree over the group), lands in the lane whose index is the entry's offset in the sub-chunk, and
// the epilogue, the beta term and the store run lane-parallel: 64 consecutive out[e] per store.  No atomics, no LDS
// exchange between workgroups, no temporary.
#include <type_traits>

#include "dp_entry.h"

namespace dp {
namespace {

constexpr int SD_ROWS = 4;        // rows (and waves) per workgroup
constexpr int SD_CHUNK = 512;     // entries of a row one wave takes (the ragged-list rule)
constexpr int SD_NV = 4;          // visits of L * V columns whose P_i is held in registers
constexpr float SD_EPS = 1e-7f;

enum { EPI_ID = 0, EPI_BCE = 1, EPI_FROB = 2 };

struct SddmmArgs {
    const float* P;
    int ldp;
    const float* Q;
    int ldq;
    const int* indptr;
    const int* indices;
    const float* values;      // EPI_FROB: a_e (null: 1)
    float* out;
    int n_rows, F;
    float alpha;
    const float* dscale;      // device scalar or null
    float beta;
};

template <int V> struct Pack;
template <> struct Pack<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <> struct Pack<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};

template <int L>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (L == 4) return quad4_sum(v);
    else if constexpr (L == 16) return row16_sum(v);
    else return wave64_sum(v);
}

template <int L, int V, int EPI>
__global__ __launch_bounds__(256) void k_csr_sddmm(SddmmArgs a) {
    constexpr int G = 64 / L;                 // entries a wave serves per step
    constexpr int NV = L == 64 ? SD_NV : 1;   // the narrow tiers cover F in one visit by construction
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane / L, sub = lane % L;
    const int F = a.F;
    const float coef = a.alpha * (a.dscale ? a.dscale[0] : 1.f);
    const int row0 = blockIdx.x * SD_ROWS;
    int item = wave;                          // position in the list of this workgroup's (row, chunk) items
    for (int r = 0; r < SD_ROWS; ++r) {
        const int row = row0 + r;
        if (row >= a.n_rows) break;
        const int beg = a.indptr[row], end = a.indptr[row + 1];
        const int nch = (end - beg + SD_CHUNK - 1) / SD_CHUNK;
        for (; item < nch; item += SD_ROWS) {
            const int cb = beg + item * SD_CHUNK;
            const int ce = min(end, cb + SD_CHUNK);
            const float* prow = a.P + (long)row * a.ldp;
            Pack<V> p[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = (v * L + sub) * V;
#pragma unroll
                for (int k = 0; k < V; ++k) p[v].v[k] = 0.f;
                if (c < F) p[v].load(prow + c);
            }
            for (int e0 = cb; e0 < ce; e0 += 64) {
                const int cnt = min(64, ce - e0);
                const int mine = a.indices[e0 + min(lane, cnt - 1)];
                const int steps = (cnt + G - 1) / G;
                float acc = 0.f;
                // U entries per group at once: their Q rows are requested before the first multiply
                auto run = [&](int t0, auto uc) {
                    constexpr int U = decltype(uc)::value;
                    Pack<V> qv[U][NV];
                    const float* qrow[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        int col;
                        if constexpr (G == 1) col = __builtin_amdgcn_readlane(mine, t0 + u);
                        else col = __shfl(mine, min((t0 + u) * G + g, cnt - 1), 64);
                        qrow[u] = a.Q + (long)col * a.ldq;
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            const int c = (v * L + sub) * V;
#pragma unroll
                            for (int k = 0; k < V; ++k) qv[u][v].v[k] = 0.f;
                            if (c < F) qv[u][v].load(qrow[u] + c);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float s = 0.f;
#pragma unroll
                        for (int v = 0; v < NV; ++v)
#pragma unroll
                            for (int k = 0; k < V; ++k) s = fmaf(p[v].v[k], qv[u][v].v[k], s);
                        if constexpr (L == 64) {          // columns beyond the register-held visits
                            for (int c = (NV * 64 + lane) * V; c < F; c += 64 * V) {
                                Pack<V> pp, qq;
                                pp.load(prow + c);
                                qq.load(qrow[u] + c);
#pragma unroll
                                for (int k = 0; k < V; ++k) s = fmaf(pp.v[k], qq.v[k], s);
                            }
                        }
                        s = group_sum<L>(s);
                        if (sub == t0 + u) acc = s;       // lane (g, t) keeps the dot of entry t * G + g
                    }
                };
                int t = 0;
                for (; t + 4 <= steps; t += 4) run(t, std::integral_constant<int, 4>{});
                for (; t < steps; ++t) run(t, std::integral_constant<int, 1>{});
                if constexpr (G > 1) acc = __shfl(acc, (lane % G) * L + lane / G, 64);      // -> lane j holds entry j
                if (lane < cnt) {
                    float rv;
                    if constexpr (EPI == EPI_BCE) {
                        const float pc = fminf(acc, 1.f);
                        rv = logf(1.f - pc + SD_EPS) - logf(pc + SD_EPS);
                    } else if constexpr (EPI == EPI_FROB) {
                        const float av = a.values ? a.values[e0 + lane] : 1.f;
                        rv = 2.f * (av - acc);
                    } else {
                        rv = acc;
                    }
                    float* o = a.out + e0 + lane;
                    rv = coef * rv;
                    *o = a.beta != 0.f ? fmaf(a.beta, *o, rv) : rv;
                }
            }
        }
        item -= nch;
    }
}

template <int L, int V>
void launch_epi(Seq& q, const SddmmArgs& a, int epi) {
    const dim3 grid((a.n_rows + SD_ROWS - 1) / SD_ROWS), block(64 * SD_ROWS);
    if (epi == EPI_BCE) hipLaunchKernelGGL((k_csr_sddmm<L, V, EPI_BCE>), grid, block, 0, q.stream, a);
    else if (epi == EPI_FROB) hipLaunchKernelGGL((k_csr_sddmm<L, V, EPI_FROB>), grid, block, 0, q.stream, a);
    else hipLaunchKernelGGL((k_csr_sddmm<L, V, EPI_ID>), grid, block, 0, q.stream, a);
}

struct SddmmPick {
    int lanes, vec, reg_visits, tail;
};

// The one place that decides the launch form: 16-byte lanes only when F, both leading dimensions and both bases allow
// them; the lane group is the smallest of 4 / 16 / 64 that covers F in one visit (64, more visits and a loop above).
SddmmPick sddmm_pick(int F, int ldp, int ldq, bool p_misaligned, bool q_misaligned) {
    SddmmPick k;
    k.vec = ((F & 3) == 0 && (ldp & 3) == 0 && (ldq & 3) == 0 && !p_misaligned && !q_misaligned) ? 4 : 1;
    k.lanes = F <= 4 * k.vec ? 4 : (F <= 16 * k.vec ? 16 : 64);
    const int per = k.lanes * k.vec;
    const int visits = (F + per - 1) / per;
    k.reg_visits = k.lanes == 64 ? (visits < SD_NV ? visits : SD_NV) : 1;
    k.tail = k.lanes == 64 && visits > SD_NV ? 1 : 0;
    return k;
}

void csr_sddmm(Seq& q, const SddmmArgs& a, int epi) {
    if (!q.ok() || a.n_rows <= 0 || a.F <= 0) return;
    const SddmmPick k = sddmm_pick(a.F, a.ldp, a.ldq, !aligned16(a.P), !aligned16(a.Q));
    if (k.vec == 4) {
        if (k.lanes == 4) launch_epi<4, 4>(q, a, epi);
        else if (k.lanes == 16) launch_epi<16, 4>(q, a, epi);
        else launch_epi<64, 4>(q, a, epi);
    } else {
        if (k.lanes == 4) launch_epi<4, 1>(q, a, epi);
        else if (k.lanes == 16) launch_epi<16, 1>(q, a, epi);
        else launch_epi<64, 1>(q, a, epi);
    }
    q.check_launch("k_csr_sddmm");
}

// P = S dA'_b per graph into the workspace, then the SDDMM with Q = S (dry: the workspace walk alone)
void pool_dvalues_seq(Seq& q, const float* S, int lds, const int* indptr, const int* indices, const float* dAp,
                      const int* off, int B, float* dvalues, int n_total, int K) {
    float* P = q.alloc<float>((size_t)n_total * K);
    if (q.err || q.dry) return;
    if (!off) {
        bgemm(q, S, dAp, P, nullptr, 1, n_total, K, K, lds, K, K, 0, 0, 0, false, false, 1.f, 0.f, 0);
    } else {
        for (int b0 = 0; b0 < B; b0 += GEMM_GROUP_MAX) {
            GemmDesc d[GEMM_GROUP_MAX];
            int cnt = 0;
            for (int b = b0; b < B && cnt < GEMM_GROUP_MAX; ++b, ++cnt)
                d[cnt] = GemmDesc{S + (long)off[b] * lds, dAp + (long)b * K * K, P + (long)off[b] * K, nullptr,
                                  off[b + 1] - off[b], K, K, lds, K, K, 0, 0, 0, false, false, 1.f, 0.f, 0, 0, 0,
                                  nullptr, 0, 0, 0};
            bgemm_group(q, d, cnt, 1);
        }
    }
    csr_sddmm(q, SddmmArgs{P, K, S, lds, indptr, indices, nullptr, dvalues, n_total, K, 1.f, nullptr, 0.f}, EPI_ID);
}

}  // namespace

// the GraphConv backward's SDDMM (dp_api.hip: sparse_gcn_bwd_seq): dvalues[e] = dax_i . x_j
void csr_sddmm_identity(Seq& q, const float* P, int ldp, const float* Q, int ldq, const int* indptr, const int* indices,
                        float* out, int n_rows, int F) {
    csr_sddmm(q, SddmmArgs{P, ldp, Q, ldq, indptr, indices, nullptr, out, n_rows, F, 1.f, nullptr, 0.f}, EPI_ID);
}

}  // namespace dp

using namespace dp;

#define SD_LD(ld, w) DP_CHECK((ld) >= (w), DP_ERR_INVALID_ARG, #ld "=%d smaller than " #w "=%d", (int)(ld), (int)(w))

extern "C" {

int dp_csr_sddmm_plan(int F, int ldp, int ldq, int p_misaligned, int q_misaligned, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_POS(F);
    SD_LD(ldp, F);
    SD_LD(ldq, F);
    const SddmmPick k = sddmm_pick(F, ldp, ldq, p_misaligned != 0, q_misaligned != 0);
    const int plan[DP_CSR_SDDMM_PLAN_INTS] = {k.lanes, k.vec, k.reg_visits, k.tail, SD_CHUNK, SD_ROWS};
    memcpy(plan_out, plan, sizeof(plan));
    return DP_OK;
}

int dp_csr_sddmm(const float* P, int ldp, const float* Q, int ldq, const int* indptr, const int* indices, float* out,
                 int n_rows, int F, float alpha, const float* dscale, float beta, void* stream) {
    DP_PTR(P); DP_PTR(Q); DP_PTR(indptr); DP_PTR(indices); DP_PTR(out);
    DP_ALIGNED4(dscale);
    DP_NONNEG(n_rows);
    DP_NONNEG(F);
    SD_LD(ldp, F);
    SD_LD(ldq, F);
    Seq q(DP_STREAM(stream), nullptr, 0);
    csr_sddmm(q, SddmmArgs{P, ldp, Q, ldq, indptr, indices, nullptr, out, n_rows, F, alpha, dscale, beta}, EPI_ID);
    return q.err;
}

int dp_csr_link_dvalues(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                        float* dvalues, int n_rows, int K, int objective, float inv_norm, const float* dloss,
                        void* stream) {
    DP_PTR(S); DP_PTR(indptr); DP_PTR(indices); DP_PTR(dvalues);
    DP_ALIGNED4(values);
    DP_ALIGNED4(dloss);
    DP_NONNEG(n_rows);
    DP_POS(K);
    SD_LD(lds, K);
    DP_CHECK(objective == 0 || objective == 1, DP_ERR_INVALID_ARG,
             "objective=%d: 0 (cross entropy) or 1 (frobenius)", objective);
    Seq q(DP_STREAM(stream), nullptr, 0);
    csr_sddmm(q, SddmmArgs{S, lds, S, lds, indptr, indices, values, dvalues, n_rows, K, inv_norm, dloss, 0.f},
              objective == 1 ? EPI_FROB : EPI_BCE);
    return q.err;
}

size_t dp_csr_pool_dvalues_workspace_bytes(int n_total, int K) {
    if (n_total < 0 || K < 0) return 0;
    Seq q = Seq::sizing();
    pool_dvalues_seq(q, nullptr, K, nullptr, nullptr, nullptr, nullptr, 1, nullptr, n_total, K);
    return q.ws_off + 256;
}

int dp_csr_pool_dvalues(const float* S, int lds, const int* indptr, const int* indices, const float* dAp,
                        const int* node_off_host, int B, float* dvalues, int n_total, int K, void* workspace,
                        size_t workspace_bytes, void* stream) {
    DP_PTR(S); DP_PTR(indptr); DP_PTR(indices); DP_PTR(dAp); DP_PTR(dvalues);
    DP_NONNEG(n_total);
    DP_POS(K);
    DP_POS(B);
    SD_LD(lds, K);
    if (node_off_host) {
        DP_CHECK(node_off_host[0] == 0 && node_off_host[B] == n_total, DP_ERR_INVALID_ARG,
                 "node_off_host runs %d .. %d, not 0 .. n_total=%d", node_off_host[0], node_off_host[B], n_total);
        for (int b = 0; b < B; ++b)
            DP_CHECK(node_off_host[b + 1] >= node_off_host[b], DP_ERR_INVALID_ARG, "node_off_host decreases at graph %d", b);
    } else {
        DP_CHECK(B == 1, DP_ERR_INVALID_ARG, "B=%d graphs need node_off_host", B);
    }
    DP_CHECK(workspace_bytes >= dp_csr_pool_dvalues_workspace_bytes(n_total, K) - 256, DP_ERR_WORKSPACE,
             "workspace too small: need >= %zu bytes, have %zu", dp_csr_pool_dvalues_workspace_bytes(n_total, K) - 256,
             workspace_bytes);
    if (n_total == 0) return DP_OK;
    DP_ALIGNED16(workspace, false, "workspace is NULL or not 16-byte aligned");
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    pool_dvalues_seq(q, S, lds, indptr, indices, dAp, node_off_host, B, dvalues, n_total, K);
    return q.err;
}

}  // extern "C"
