// Set2Set readout (dp_set2set.hip) on a RAGGED batch: graph b owns rows node_off[b] .. node_off[b+1]-1 of emb
// [n_total, .] and stands for the dense batch padded to T rows, whose padded rows are exactly zero behind the
// embedding mask.  Set2Set.forward (set2set.py:32-57) runs T steps — the padded size — and in every step a zero row has
// logit e = 0: with P_b = T - n_b,
//     m = max(max_i e_i, 0) if P_b > 0 else max_i e_i;   Z = sum_i exp(e_i - m) + P_b exp(-m);   a_i = exp(e_i - m) / Z,
// and the padded rows add nothing to r = sum_i a_i E_b[i].  In the backward a padded row has da = 0 and its de multiplies
// a zero row, so padding enters only through m and Z (the saved a_t already carry it).
//
// One persistent workgroup per graph walks the T steps over its own n_b rows (k_set2set_ragged_fwd / _bwd).  The
// softmax and <a, da> run over all 16 waves: thread i owns rows i, i + 1024, ...; the 16 wave results are combined in
// wave order, so two runs agree bit for bit.  Whether the graph's embedding is staged in LDS is a compile-time variant
// (EL) decided per graph by set2set_ragged_plan: every pass launches up to two grids of B workgroups, one per variant,
// and a workgroup whose graph belongs to the other grid leaves at once (it evaluates the same plan function).  The
// LSTM weights sit in registers for d <= 64 (WF) and are read from global memory above; they are never staged in LDS,
// which keeps room for the per-row vectors al / de / lat (2 n_b floats) up to n_b = 16 384 at every d.
//
// As in the dense kernels the per-step a_t and de_t are saved ([T, n_b] blocks per graph, graph b's block at
// T (node_off[b] - node_off[0])) and every weight / embedding gradient is a contraction after the kernel:
// dW_ih = DG^T QP, dW_hh = DG^T QP[:, :d] over the B T (graph, step) rows on the MFMA GEMM, and
// demb_b = A_b^T DR_b + DE_b^T H_b per graph (k_s2sr_demb: M = n_b differs per graph, so one grid of (row tile, graph)
// workgroups, each output a serial chain over t).  No atomics anywhere.
#include "dp_entry.h"

namespace dp {
namespace {

constexpr int SR_NT = 1024;
constexpr int SR_NW = SR_NT / 64;
constexpr int SR_MAX_ROWS = DP_SET2SET_RAGGED_MAX_ROWS;
constexpr unsigned SR_LDS_BYTES = 158 * 1024;
constexpr int SR_WF = 4, SR_EL = 2;                    // bits of dp_set2set_plan

// LDS of a graph of nb rows, in floats: [h, r, c, gates] 7d + 8 | rpart 1024 | red 32 | al / de [npad] | lat [npad] | 16
// | the embedding [nb][d] when staged
__host__ __device__ inline unsigned sr_lds_floats(int nb, int d, bool el) {
    const unsigned npad = (unsigned)(nb + 15) & ~15u;
    return 7u * d + 8 + 1024 + 32 + 2 * npad + 16 + (el ? (unsigned)nb * (unsigned)d : 0u);
}
__host__ __device__ inline bool sr_el(int nb, int d) { return sr_lds_floats(nb, d, true) * 4u <= SR_LDS_BYTES; }
inline bool sr_wf(int d) { return 4 * d <= 256 && ((2 * d + 3) >> 2) <= 32 && ((4 * d + 7) >> 3) <= 32; }

__device__ inline float sr_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct SRFwdArgs {
    const float* emb;
    int lde;
    const int* node_off;
    int base;                           // node_off[0]
    const float *w_ih, *w_hh, *b_ih, *b_hh, *Wp, *bp;
    float* out;                         // [B, d]
    float *QP, *H, *Cs, *G, *Aw, *QN;   // save arrays (all null: inference)
    int T, d;
    unsigned lds_floats;                // what the launch asked for
};

template <bool EL, bool WF>
__global__ __launch_bounds__(SR_NT) void k_set2set_ragged_fwd(SRFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = a.d, T = a.T;
    const int r0 = a.node_off[b], nb = a.node_off[b + 1] - r0;
    // (uniform) the other grid's graph; the second test never fires when node_off matches node_off_host
    if (nb < 1 || nb > T || sr_el(nb, d) != EL || sr_lds_floats(nb, d, EL) > a.lds_floats) return;
    const int npad = (nb + 15) & ~15;
    float* h = lds;                                    // [d]   } contiguous: the LSTM input q* = [h, r]
    float* r = h + d;                                  // [d]   }
    float* c = r + d;                                  // [d]
    float* gates = c + d;                              // [4d]  ACTIVATED gates i, f, g, o
    float* rpart = gates + 4 * d + 8;                  // [16][64]
    float* red = rpart + 1024;                         // [2][16] wave partials of the softmax
    float* al = red + 32;                              // [nb]
    float* le = al + 2 * npad + 16;                    // [nb][d] when EL
    for (int i = tid; i < 3 * d; i += SR_NT) h[i] = 0.f;       // h, r, c = 0 (set2set.py:42-45)
    const float* embg = a.emb + (long)r0 * a.lde;
    if constexpr (EL)
        for (int i = tid; i < nb * d; i += SR_NT) le[i] = embg[(long)(i / d) * a.lde + i % d];
    __syncthreads();
    const int lde = EL ? d : a.lde;
    auto Eat = [&](long i) -> float {
        if constexpr (EL) return le[i];
        else return embg[i];
    };
    const int lane = tid & 63, wave = tid >> 6;
    const int tl = tid & 15, team = tid >> 4;          // 64 sixteen-lane teams
    const int q4 = tid & 3, gteam = tid >> 2;          // 256 four-lane gate teams
    const int P = T - nb;                              // zero rows of the dense batch behind this graph
    const float Pf = (float)P;
    float* Ab = a.Aw ? a.Aw + (size_t)T * (size_t)(r0 - a.base) : nullptr;
    constexpr int GPT = 4;                             // gates per team slot: 4d <= 1024
    float gbias[GPT];
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
        const int g = min(gteam + 256 * i, 4 * d - 1);
        gbias[i] = a.b_ih[g] + a.b_hh[g];
    }
    const int kq = (2 * d + 3) >> 2;                   // terms per lane of a gate team
    const int k0 = q4 * kq, k1 = min(2 * d, k0 + kq);
    // gates = (W_ih[:, :d] + W_hh) h + W_ih[:, d:] r + b (q = h).  WF: a team owns ONE gate, its lanes keep their <= 32
    // combined weights in registers for all T steps
    constexpr int WREG = 32;
    float wreg[WF ? WREG : 1];
    if constexpr (WF) {
        const int gg = min(gteam, 4 * d - 1);
#pragma unroll
        for (int i = 0; i < WREG; ++i) {
            const int k = k0 + i;
            float v = 0.f;
            if (k < k1) {
                v = a.w_ih[(long)gg * 2 * d + k];
                if (k < d) v += a.w_hh[(long)gg * d + k];
            }
            wreg[i] = v;
        }
    }

    for (int t = 0; t < T; ++t) {
        const long bt = (long)b * T + t;
        // ---- q*_{t-1} = [h, r] is the LSTM input of this step
        if (a.QP && tid < 2 * d) a.QP[bt * 2 * d + tid] = h[tid];
        if constexpr (WF) {
            float acc = 0.f, acc2 = 0.f;
#pragma unroll
            for (int i = 0; i < WREG; i += 2) {
                acc += wreg[i] * h[min(k0 + i, 2 * d - 1)];
                acc2 += wreg[i + 1] * h[min(k0 + i + 1, 2 * d - 1)];
            }
            acc = quad4_sum(acc + acc2);
            if (q4 == 0 && gteam < 4 * d) {
                const float pre = acc + gbias[0];
                const float act = (gteam >= 2 * d && gteam < 3 * d) ? tanhf(pre) : sr_sigmoid(pre);
                gates[gteam] = act;
                if (a.G) a.G[bt * 4 * d + gteam] = act;
            }
        } else
#pragma unroll
        for (int i = 0; i < GPT; ++i) {
            if (256 * i >= 4 * d) break;               // (uniform)
            const int g = gteam + 256 * i, gg = min(g, 4 * d - 1);
            const float* wi = a.w_ih + (long)gg * 2 * d;       // a lane walks a contiguous piece of its gate's rows
            const float* wh = a.w_hh + (long)gg * d;
            float acc = 0.f, acc2 = 0.f;
            const int kh = min(k1, d);
            for (int k = k0; k < kh; ++k) acc += (wi[k] + wh[k]) * h[k];
            for (int k = max(k0, d); k < k1; ++k) acc2 += wi[k] * h[k];
            acc = quad4_sum(acc + acc2);
            if (q4 == 0 && g < 4 * d) {
                const float pre = acc + gbias[i];
                const float act = (gg >= 2 * d && gg < 3 * d) ? tanhf(pre) : sr_sigmoid(pre);
                gates[gg] = act;
                if (a.G) a.G[bt * 4 * d + gg] = act;
            }
        }
        lds_barrier();
        // ---- LSTM cell (gate order i, f, g, o)
        if (tid < d) {
            const int j = tid;
            const float cn = gates[d + j] * c[j] + gates[j] * gates[2 * d + j];
            const float hn = gates[3 * d + j] * tanhf(cn);
            c[j] = cn;
            h[j] = hn;
            if (a.G) {
                a.Cs[bt * d + j] = cn;
                a.H[bt * d + j] = hn;
            }
        }
        lds_barrier();
        // ---- e = emb . h over the graph's own rows (a padded row of the dense batch has e = 0)
        for (int row = team; row < nb; row += 64) {
            float s = 0.f;
            for (int k = tl; k < d; k += 16) s += Eat((long)row * lde + k) * h[k];
            s = row16_sum(s);
            if (tl == 0) al[row] = s;
        }
        lds_barrier();
        // ---- a = softmax over the nb real logits and P zeros: thread i owns rows i, i + 1024, ...
        float m = -INFINITY;
        for (int row = tid; row < nb; row += SR_NT) m = fmaxf(m, al[row]);
        m = wave64_max(m);
        if (lane == 0) red[wave] = m;
        lds_barrier();
        m = red[0];
#pragma unroll
        for (int w = 1; w < SR_NW; ++w) m = fmaxf(m, red[w]);
        if (P > 0) m = fmaxf(m, 0.f);
        float sum = 0.f;
        for (int row = tid; row < nb; row += SR_NT) {
            const float p = expf(al[row] - m);
            al[row] = p;
            sum += p;
        }
        sum = wave64_sum(sum);
        if (lane == 0) red[16 + wave] = sum;
        lds_barrier();
        float Z = red[16];
#pragma unroll
        for (int w = 1; w < SR_NW; ++w) Z += red[16 + w];
        if (P > 0) Z += Pf * expf(-m);
        const float inv = 1.f / Z;
        for (int row = tid; row < nb; row += SR_NT) {
            const float p = al[row] * inv;
            al[row] = p;
            if (Ab) Ab[(size_t)t * nb + row] = p;
        }
        lds_barrier();
        // ---- r = sum_n a[n] emb[n]: 16 row parts (one per wave) x 64 columns
        for (int j0 = 0; j0 < d; j0 += 64) {
            const int j = j0 + lane;
            float s = 0.f;
            if (j < d) {
#pragma unroll 4
                for (int row = wave; row < nb; row += 16) s += al[row] * Eat((long)row * lde + j);
            }
            rpart[wave * 64 + lane] = s;
            lds_barrier();
            if (wave == 0 && j < d) {
                float tsum = 0.f;
#pragma unroll
                for (int p = 0; p < 16; ++p) tsum += rpart[p * 64 + lane];
                r[j] = tsum;
            }
            lds_barrier();
        }
    }
    // ---- out = relu(Wp [h, r] + bp): one sixteen-lane team per output, the bias added last (dp_set2set.hip)
    if (a.QN && tid < 2 * d) a.QN[(long)b * 2 * d + tid] = h[tid];
    for (int j = team; j < d; j += 64) {
        const float* wr = a.Wp + (long)j * 2 * d;
        float s = 0.f;
        for (int k = tl; k < 2 * d; k += 16) s += wr[k] * h[k];
        s = row16_sum(s);
        if (tl == 0) a.out[(long)b * d + j] = fmaxf(s + a.bp[j], 0.f);
    }
}

struct SRBwdArgs {
    const float* emb;
    int lde;
    const int* node_off;
    int base;
    const float* wt;               // [2d][GS] (workspace, set2set_prep_weights)
    const float* Wp;
    const float* out;
    const float* dout;
    const float *Cs, *G, *Aw;
    float *DG, *DR, *DE, *DPRE;    // workspace outputs
    int T, d, GS;
    unsigned lds_floats;
};

template <bool EL, bool WF>
__global__ __launch_bounds__(SR_NT) void k_set2set_ragged_bwd(SRBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = a.d, T = a.T, GS = a.GS;
    const int r0 = a.node_off[b], nb = a.node_off[b + 1] - r0;
    if (nb < 1 || nb > T || sr_el(nb, d) != EL || sr_lds_floats(nb, d, EL) > a.lds_floats) return;   // (uniform)
    const int npad = (nb + 15) & ~15;
    float* dh = lds;                 // [d]  } contiguous: d q* = [dh, dr]
    float* dr = dh + d;              // [d]  }
    float* dc = dr + d;              // [d]
    float* dg = dc + d;              // [4d]
    float* rpart = dg + 4 * d + 8;   // [16][64]
    float* red = rpart + 1024;       // [16] wave partials of <a, da>
    float* de = red + 32;            // [nb]
    float* lat = de + npad;          // [nb] attention weights a_t of the step being processed
    float* le = lat + npad + 16;     // [nb][d] when EL
    const float* embg = a.emb + (long)r0 * a.lde;
    if constexpr (EL)
        for (int i = tid; i < nb * d; i += SR_NT) le[i] = embg[(long)(i / d) * a.lde + i % d];
    auto Eat = [&](long i) -> float {
        if constexpr (EL) return le[i];
        else return embg[i];
    };
    // ---- output layer: dpre = dout * (out > 0);  [dh, dr] = Wp^T dpre;  dc = 0
    for (int j = tid; j < d; j += SR_NT) {
        const float o = a.out[(long)b * d + j];
        const float v = o > 0.f ? a.dout[(long)b * d + j] : 0.f;
        dg[j] = v;                                   // borrow dg[0:d] for dpre
        a.DPRE[(long)b * d + j] = v;
        dc[j] = 0.f;
    }
    __syncthreads();
    for (int k = tid; k < 2 * d; k += SR_NT) {
        float s = 0.f;
        for (int j = 0; j < d; ++j) s += a.Wp[(long)j * 2 * d + k] * dg[j];
        dh[k] = s;                                   // (k >= d lands in dr)
    }
    __syncthreads();
    const int lde = EL ? d : a.lde;
    const int lane = tid & 63, wave = tid >> 6;
    const int tl = tid & 15, team = tid >> 4;
    const int q8 = tid & 7, oteam = tid >> 3;         // 128 eight-lane teams for [dh, dr] = Wt dg
    const int gq = (4 * d + 7) >> 3;                   // terms per lane there
    const int g0 = q8 * gq, g1 = min(4 * d, g0 + gq);
    constexpr int WREG = 32;                           // WF: one output per team, its weights in registers
    float wreg[WF ? WREG : 1];
    if constexpr (WF) {
        const long wr = (long)min(oteam, 2 * d - 1) * GS;
#pragma unroll
        for (int i = 0; i < WREG; ++i) wreg[i] = g0 + i < g1 ? a.wt[wr + g0 + i] : 0.f;
    }
    const size_t aoff = (size_t)T * (size_t)(r0 - a.base);
    const float* Ab = a.Aw + aoff;
    float* DEb = a.DE + aoff;

    // the saved gates and cell states of a step are fetched one step AHEAD into registers (dp_set2set.hip)
    float gn[6];
    auto prefetch = [&](int t) {
        const int tc = t < 0 ? 0 : t;                 // (the last prefetch is unused; keep the address valid)
        const int j = min(tid, d - 1);
        const long bt = (long)b * T + tc;
        const float* gs = a.G + bt * 4 * d;
        gn[0] = gs[j]; gn[1] = gs[d + j]; gn[2] = gs[2 * d + j]; gn[3] = gs[3 * d + j];
        gn[4] = a.Cs[bt * d + j];
        gn[5] = tc > 0 ? a.Cs[(bt - 1) * d + j] : 0.f;
    };
    prefetch(T - 1);
    for (int t = T - 1; t >= 0; --t) {
        const long bt = (long)b * T + t;
        // ---- r_t = sum a emb:  da = emb . dr ;  de = a * (da - <a, da>), both over the real rows only
        if (tid < d) a.DR[bt * d + tid] = dr[tid];
        for (int row = team; row < nb; row += 64) {
            float s = 0.f;
            for (int k = tl; k < d; k += 16) s += Eat((long)row * lde + k) * dr[k];
            s = row16_sum(s);
            if (tl == 0) de[row] = s;
        }
        lds_barrier();
        const float* at = Ab + (size_t)t * nb;
        float lsum = 0.f;
        for (int row = tid; row < nb; row += SR_NT) {      // thread i owns rows i, i + 1024, ...
            const float av = at[row];
            lat[row] = av;
            lsum += av * de[row];
        }
        lsum = wave64_sum(lsum);
        if (lane == 0) red[wave] = lsum;
        lds_barrier();
        float sdot = red[0];
#pragma unroll
        for (int w = 1; w < SR_NW; ++w) sdot += red[w];
        for (int row = tid; row < nb; row += SR_NT) {
            const float v = lat[row] * (de[row] - sdot);
            de[row] = v;
            DEb[(size_t)t * nb + row] = v;
        }
        lds_barrier();
        // ---- e = emb . h_t:  dh += sum_n de[n] emb[n]
        for (int j0 = 0; j0 < d; j0 += 64) {
            const int j = j0 + lane;
            float s = 0.f;
            if (j < d) {
#pragma unroll 2
                for (int row = wave; row < nb; row += 16) s += de[row] * Eat((long)row * lde + j);
            }
            rpart[wave * 64 + lane] = s;
            lds_barrier();
            if (wave == 0 && j < d) {
                float tsum = 0.f;
#pragma unroll
                for (int p = 0; p < 16; ++p) tsum += rpart[p * 64 + lane];
                dh[j] += tsum;
            }
            lds_barrier();
        }
        // ---- LSTM cell backward
        if (tid < d) {
            const int j = tid;
            const float ig = gn[0], fg = gn[1], gg = gn[2], og = gn[3];
            const float ct = gn[4];
            const float cp = gn[5];
            const float tc = tanhf(ct);
            const float dhj = dh[j];
            const float dct = dc[j] + dhj * og * (1.f - tc * tc);
            const float d_i = dct * gg * ig * (1.f - ig);
            const float d_f = dct * cp * fg * (1.f - fg);
            const float d_g = dct * ig * (1.f - gg * gg);
            const float d_o = dhj * tc * og * (1.f - og);
            dg[j] = d_i; dg[d + j] = d_f; dg[2 * d + j] = d_g; dg[3 * d + j] = d_o;
            float* o = a.DG + bt * 4 * d;
            o[j] = d_i; o[d + j] = d_f; o[2 * d + j] = d_g; o[3 * d + j] = d_o;
            dc[j] = dct * fg;
        }
        prefetch(t - 1);                               // the next step's saved state flies under the product below
        lds_barrier();
        // ---- [dh_{t-1}, dr_{t-1}] = Wt dg: eight lanes per output
        if constexpr (WF) {
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int i = 0; i < WREG; i += 2) {
                s0 += wreg[i] * dg[min(g0 + i, 4 * d - 1)];
                s1 += wreg[i + 1] * dg[min(g0 + i + 1, 4 * d - 1)];
            }
            s0 = oct8_sum(s0 + s1);
            if (q8 == 0 && oteam < 2 * d) dh[oteam] = s0;      // (k >= d lands in dr)
        } else
        for (int k = oteam; k < 2 * d; k += 128) {
            const long wr = (long)k * GS;
            float s = 0.f, s2 = 0.f;
            int g = g0;
            for (; g + 1 < g1; g += 2) {
                s += a.wt[wr + g] * dg[g];
                s2 += a.wt[wr + g + 1] * dg[g + 1];
            }
            if (g < g1) s += a.wt[wr + g] * dg[g];
            s = oct8_sum(s + s2);
            if (q8 == 0) dh[k] = s;                    // (k >= d lands in dr)
        }
        lds_barrier();
    }
}

// demb_b = A_b^T DR_b + DE_b^T H_b: workgroup (row tile, graph) takes 64 rows of graph b and all d columns, walks t in
// chunks of 16 staged in LDS; thread (ty, tx) holds rows ty * 4 .. + 3 and columns tx, tx + 16, ...  Every output is one
// serial chain over t = 0 .. T - 1.
constexpr int SD_TK = 16, SD_RT = 64;
template <int CS>
__global__ __launch_bounds__(256) void k_s2sr_demb(const float* Aw, const float* DE, const float* DR, const float* H,
                                                   const int* node_off, int base, float* demb, int ldde, int T, int d) {
    constexpr int W = CS * 16;
    __shared__ float As[SD_TK][SD_RT], Es[SD_TK][SD_RT], Rs[SD_TK][W], Hs[SD_TK][W];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int r0 = node_off[b], nb = node_off[b + 1] - r0;
    const int i0 = blockIdx.x * SD_RT;
    if (i0 >= nb) return;                                       // (uniform)
    const size_t aoff = (size_t)T * (size_t)(r0 - base);
    const float* Ab = Aw + aoff;
    const float* Eb = DE + aoff;
    const float* Rb = DR + (size_t)b * T * d;
    const float* Hb = H + (size_t)b * T * d;
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][CS];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < CS; ++c) acc[i][c] = 0.f;
    for (int t0 = 0; t0 < T; t0 += SD_TK) {
        for (int i = tid; i < SD_TK * SD_RT; i += 256) {
            const int k = i / SD_RT, rr = i % SD_RT;
            const int t = t0 + k, row = i0 + rr;
            const bool ok = t < T && row < nb;
            As[k][rr] = ok ? Ab[(size_t)t * nb + row] : 0.f;
            Es[k][rr] = ok ? Eb[(size_t)t * nb + row] : 0.f;
        }
        for (int i = tid; i < SD_TK * W; i += 256) {
            const int k = i / W, j = i % W;
            const int t = t0 + k;
            const bool ok = t < T && j < d;
            Rs[k][j] = ok ? Rb[(size_t)t * d + j] : 0.f;
            Hs[k][j] = ok ? Hb[(size_t)t * d + j] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SD_TK; ++k) {
            float av[4], ev[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = As[k][ty * 4 + i];
                ev[i] = Es[k][ty * 4 + i];
            }
#pragma unroll
            for (int c = 0; c < CS; ++c) {
                const float rv = Rs[k][tx + 16 * c], hv = Hs[k][tx + 16 * c];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][c] += av[i] * rv + ev[i] * hv;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i0 + ty * 4 + i;
        if (row >= nb) continue;
#pragma unroll
        for (int c = 0; c < CS; ++c) {
            const int j = tx + 16 * c;
            if (j < d) demb[(size_t)(r0 + row) * ldde + j] = acc[i][c];
        }
    }
}

struct SRLayout {   // offsets in floats
    size_t qp, h, c, g, qn, a, total;
};
SRLayout sr_layout(size_t B, size_t T, size_t n_total, size_t d) {
    SRLayout L{};
    size_t off = 0;
    auto take = [&](size_t cnt) {
        size_t o = off;
        off += (cnt + 63) & ~size_t(63);
        return o;
    };
    L.qp = take(B * T * 2 * d);
    L.h = take(B * T * d);
    L.c = take(B * T * d);
    L.g = take(B * T * 4 * d);
    L.qn = take(B * 2 * d);
    L.a = take(T * n_total);
    L.total = off;
    return L;
}

// what the host decides from node_off_host: the row counts, and per variant the largest graph (the grid's LDS)
struct SRBatch {
    int n_total, max_n, max_el, max_gl;      // max_el / max_gl: largest graph with / without its embedding in LDS, 0: none
};

}  // namespace

// The ONE place that picks the variant a graph of nb rows runs, for both passes (host only, no GPU call).
int set2set_ragged_plan(int nb, int d) {
    if (nb < 1 || d < 1 || d > 256 || nb > SR_MAX_ROWS || sr_lds_floats(nb, d, false) * 4u > SR_LDS_BYTES)
        return DP_ERR_UNSUPPORTED;
    return (sr_el(nb, d) ? SR_EL : 0) | (sr_wf(d) ? SR_WF : 0);
}

namespace {

int sr_check_batch(const char* entry, const int* node_off_host, int B, int T, int d, SRBatch& s) {
    DP_CHECK(node_off_host != nullptr, DP_ERR_INVALID_ARG, "%s: node_off_host is NULL", entry);
    DP_CHECK(B >= 0, DP_ERR_INVALID_ARG, "%s: B=%d must not be negative", entry, B);
    DP_CHECK(B <= 65535, DP_ERR_UNSUPPORTED, "%s: more than 65535 graphs", entry);
    DP_CHECK(d >= 1, DP_ERR_INVALID_ARG, "%s: d=%d must be positive", entry, d);
    DP_CHECK(d <= 256, DP_ERR_UNSUPPORTED, "%s: d=%d above the supported 256", entry, d);
    DP_CHECK(T >= 1, DP_ERR_INVALID_ARG, "%s: T=%d must be positive", entry, T);
    DP_CHECK(node_off_host[0] >= 0, DP_ERR_INVALID_ARG, "%s: node_off_host[0]=%d is negative", entry, node_off_host[0]);
    s = SRBatch{0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const long nb = (long)node_off_host[b + 1] - node_off_host[b];
        DP_CHECK(nb >= 1, DP_ERR_INVALID_ARG, "%s: graph %d has %ld rows (every graph needs at least one)", entry, b, nb);
        DP_CHECK(nb <= SR_MAX_ROWS, DP_ERR_UNSUPPORTED, "%s: graph %d has %ld rows, above the supported %d", entry, b, nb,
                 SR_MAX_ROWS);
        DP_CHECK(nb <= T, DP_ERR_INVALID_ARG, "%s: T=%d is below graph %d's %ld rows", entry, T, b, nb);
        const int plan = set2set_ragged_plan((int)nb, d);
        DP_CHECK(plan >= 0, DP_ERR_UNSUPPORTED, "%s: graph %d (%ld rows, d=%d) outside the persistent kernel's limits",
                 entry, b, nb, d);
        s.max_n = nb > s.max_n ? (int)nb : s.max_n;
        int& mx = (plan & SR_EL) ? s.max_el : s.max_gl;
        mx = nb > mx ? (int)nb : mx;
    }
    s.n_total = B > 0 ? node_off_host[B] - node_off_host[0] : 0;
    DP_CHECK((long)B * T < (1L << 31), DP_ERR_UNSUPPORTED, "%s: B * T = %ld (graph, step) rows, above 2^31 - 1", entry,
             (long)B * T);
    return DP_OK;
}

size_t sr_save_bytes(const SRBatch& s, int B, int T, int d) {
    return sr_layout((size_t)B, (size_t)T, (size_t)s.n_total, (size_t)d).total * sizeof(float) + 256;
}

template <typename Args, typename K>
void sr_launch(Seq& q, DynLdsOnce& at, K kern, Args a, int B, int max_nb, bool el, const char* what) {
    if (max_nb == 0 || !q.ok()) return;
    ensure_dyn_lds(q, at, reinterpret_cast<const void*>(kern), 160 * 1024, what);
    if (!q.ok()) return;
    a.lds_floats = sr_lds_floats(max_nb, a.d, el);
    hipLaunchKernelGGL(kern, dim3(B), dim3(SR_NT), (size_t)a.lds_floats * sizeof(float), q.stream, a);
    q.check_launch(what);
}

void sr_bwd_seq(Seq& q, const SRBatch& s, const float* emb, int lde, const int* node_off, int base, const float* w_ih,
                const float* w_hh, const float* Wp, const float* out, const float* dout, float* demb, int ldde,
                float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* dWp, float* dbp, int B, int T, int d,
                const float* sv) {
    const SRLayout L = sr_layout((size_t)B, (size_t)T, (size_t)s.n_total, (size_t)d);
    const int GS = 4 * d + 1;
    float* wt = q.alloc<float>((size_t)2 * d * GS);
    float* DG = q.alloc<float>((size_t)B * T * 4 * d);
    float* DR = q.alloc<float>((size_t)B * T * d);
    float* DE = q.alloc<float>((size_t)T * s.n_total);
    float* DPRE = q.alloc<float>((size_t)B * d);
    if (!q.ok()) return;
    if (B == 0) {
        // an empty batch: every parameter gradient is a sum over no graph (dp_set2set_bwd does the same)
        struct { float* p; size_t cnt; } z[6] = {{dw_ih, (size_t)8 * d * d}, {dw_hh, (size_t)4 * d * d},
                                                  {db_ih, (size_t)4 * d},     {db_hh, (size_t)4 * d},
                                                  {dWp, (size_t)2 * d * d},   {dbp, (size_t)d}};
        for (auto& e : z) {
            const hipError_t er = hipMemsetAsync(e.p, 0, e.cnt * sizeof(float), q.stream);
            if (er != hipSuccess && !q.err) {
                set_error("set2set_ragged_bwd: hipMemsetAsync: %s", hipGetErrorString(er));
                q.err = (int)er;
            }
        }
        return;
    }
    set2set_prep_weights(q, w_ih, w_hh, wt, d);
    SRBwdArgs a{};
    a.emb = emb; a.lde = lde; a.node_off = node_off; a.base = base; a.wt = wt; a.Wp = Wp; a.out = out; a.dout = dout;
    a.Cs = sv + L.c; a.G = sv + L.g; a.Aw = sv + L.a;
    a.DG = DG; a.DR = DR; a.DE = DE; a.DPRE = DPRE;
    a.T = T; a.d = d; a.GS = GS;
    static DynLdsOnce e1f1, e0f1, e1f0, e0f0;
    if (sr_wf(d)) {
        sr_launch(q, e1f1, &k_set2set_ragged_bwd<true, true>, a, B, s.max_el, true, "k_set2set_ragged_bwd");
        sr_launch(q, e0f1, &k_set2set_ragged_bwd<false, true>, a, B, s.max_gl, false, "k_set2set_ragged_bwd");
    } else {
        sr_launch(q, e1f0, &k_set2set_ragged_bwd<true, false>, a, B, s.max_el, true, "k_set2set_ragged_bwd");
        sr_launch(q, e0f0, &k_set2set_ragged_bwd<false, false>, a, B, s.max_gl, false, "k_set2set_ragged_bwd");
    }
    if (!q.ok()) return;
    const float* QP = sv + L.qp;
    const float* QN = sv + L.qn;
    const float* H = sv + L.h;
    // output layer: dWp = dpre^T [h_T, r_T];  dbp = colsum(dpre)
    bgemm(q, DPRE, QN, dWp, nullptr, 1, d, 2 * d, B, d, 2 * d, 2 * d, 0, 0, 0, true, false, 1.f, 0.f, 0);
    colsum_batched(q, DPRE, d, 0, B, d, dbp, 0, 1);
    // LSTM weights: contractions over all B T (graph, step) rows
    {
        GemmDesc g[2] = {
            {DG, QP, dw_ih, nullptr, 4 * d, 2 * d, B * T, 4 * d, 2 * d, 2 * d, 0, 0, 0, true, false, 1.f, 0.f, 0},
            {DG, QP, dw_hh, nullptr, 4 * d, d, B * T, 4 * d, 2 * d, d, 0, 0, 0, true, false, 1.f, 0.f, 0}};
        bgemm_group(q, g, 2, 1);
    }
    colsum_batched(q, DG, 4 * d, 0, B * T, 4 * d, db_ih, 0, 1);
    colsum_batched(q, DG, 4 * d, 0, B * T, 4 * d, db_hh, 0, 1);
    if (!q.ok()) return;
    // demb_b = A_b^T DR_b + DE_b^T H_b
    const dim3 grid((s.max_n + SD_RT - 1) / SD_RT, B);
    const float* Aw = sv + L.a;
    if (d <= 64)
        hipLaunchKernelGGL(k_s2sr_demb<4>, grid, dim3(256), 0, q.stream, Aw, (const float*)DE, (const float*)DR, H,
                           node_off, base, demb, ldde, T, d);
    else if (d <= 128)
        hipLaunchKernelGGL(k_s2sr_demb<8>, grid, dim3(256), 0, q.stream, Aw, (const float*)DE, (const float*)DR, H,
                           node_off, base, demb, ldde, T, d);
    else
        hipLaunchKernelGGL(k_s2sr_demb<16>, grid, dim3(256), 0, q.stream, Aw, (const float*)DE, (const float*)DR, H,
                           node_off, base, demb, ldde, T, d);
    q.check_launch("s2sr_demb");
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_set2set_ragged_plan(int n_b, int d) { return set2set_ragged_plan(n_b, d); }

size_t dp_set2set_ragged_save_bytes(const int* node_off_host, int B, int T, int d) {
    SRBatch s;
    if (sr_check_batch("dp_set2set_ragged_save_bytes", node_off_host, B, T, d, s) != DP_OK) return 0;
    return sr_save_bytes(s, B, T, d);
}

size_t dp_set2set_ragged_bwd_workspace_bytes(const int* node_off_host, int B, int T, int d) {
    SRBatch s;
    if (sr_check_batch("dp_set2set_ragged_bwd_workspace_bytes", node_off_host, B, T, d, s) != DP_OK) return 0;
    Seq q = Seq::sizing();
    sr_bwd_seq(q, s, 0, d, 0, 0, 0, 0, 0, 0, 0, 0, d, 0, 0, 0, 0, 0, 0, B, T, d, 0);
    return q.ws_off + 256;
}

int dp_set2set_ragged_fwd(const float* emb, int lde, const int* node_off, const int* node_off_host, int B, int T, int d,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* Wp,
                          const float* bp, float* out, void* save, size_t save_bytes, void* stream) {
    DP_PTR(emb); DP_PTR(node_off); DP_PTR(w_ih); DP_PTR(w_hh); DP_PTR(b_ih); DP_PTR(b_hh); DP_PTR(Wp); DP_PTR(bp);
    DP_PTR(out);
    SRBatch s;
    if (int rc = sr_check_batch("dp_set2set_ragged_fwd", node_off_host, B, T, d, s)) return rc;
    DP_CHECK(lde >= d, DP_ERR_INVALID_ARG, "dp_set2set_ragged_fwd: lde=%d smaller than the row width d=%d", lde, d);
    if (save) {
        DP_ALIGNED4(save);
        DP_CHECK(save_bytes >= sr_save_bytes(s, B, T, d), DP_ERR_INVALID_ARG,
                 "dp_set2set_ragged_fwd: save buffer too small: %zu < %zu", save_bytes, sr_save_bytes(s, B, T, d));
    }
    if (B == 0) return DP_OK;                          // (an empty batch has no output row: nothing to launch)
    Seq q((hipStream_t)stream, nullptr, 0);
    SRFwdArgs a{};
    a.emb = emb; a.lde = lde; a.node_off = node_off; a.base = node_off_host[0];
    a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh; a.Wp = Wp; a.bp = bp; a.out = out;
    if (save) {
        const SRLayout L = sr_layout((size_t)B, (size_t)T, (size_t)s.n_total, (size_t)d);
        float* sv = (float*)save;
        a.QP = sv + L.qp; a.H = sv + L.h; a.Cs = sv + L.c; a.G = sv + L.g; a.Aw = sv + L.a; a.QN = sv + L.qn;
    }
    a.T = T; a.d = d;
    static DynLdsOnce e1f1, e0f1, e1f0, e0f0;
    if (sr_wf(d)) {
        sr_launch(q, e1f1, &k_set2set_ragged_fwd<true, true>, a, B, s.max_el, true, "k_set2set_ragged_fwd");
        sr_launch(q, e0f1, &k_set2set_ragged_fwd<false, true>, a, B, s.max_gl, false, "k_set2set_ragged_fwd");
    } else {
        sr_launch(q, e1f0, &k_set2set_ragged_fwd<true, false>, a, B, s.max_el, true, "k_set2set_ragged_fwd");
        sr_launch(q, e0f0, &k_set2set_ragged_fwd<false, false>, a, B, s.max_gl, false, "k_set2set_ragged_fwd");
    }
    return q.err;
}

int dp_set2set_ragged_bwd(const float* emb, int lde, const int* node_off, const int* node_off_host, int B, int T, int d,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* Wp,
                          const float* bp, const float* out, const float* dout, float* demb, int ldde, float* dw_ih,
                          float* dw_hh, float* db_ih, float* db_hh, float* dWp, float* dbp, const void* save,
                          size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(emb); DP_PTR(node_off); DP_PTR(w_ih); DP_PTR(w_hh); DP_PTR(Wp); DP_PTR(out); DP_PTR(dout); DP_PTR(demb);
    DP_PTR(dw_ih); DP_PTR(dw_hh); DP_PTR(db_ih); DP_PTR(db_hh); DP_PTR(dWp); DP_PTR(dbp); DP_PTR(save);
    (void)b_ih; (void)b_hh; (void)bp;                  // (the biases enter no gradient but their own)
    SRBatch s;
    if (int rc = sr_check_batch("dp_set2set_ragged_bwd", node_off_host, B, T, d, s)) return rc;
    DP_CHECK(lde >= d && ldde >= d, DP_ERR_INVALID_ARG,
             "dp_set2set_ragged_bwd: lde=%d / ldde=%d smaller than the row width d=%d", lde, ldde, d);
    DP_CHECK(save_bytes >= sr_save_bytes(s, B, T, d), DP_ERR_INVALID_ARG,
             "dp_set2set_ragged_bwd: save buffer too small: %zu < %zu", save_bytes, sr_save_bytes(s, B, T, d));
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    sr_bwd_seq(q, s, emb, lde, node_off, node_off_host[0], w_ih, w_hh, Wp, out, dout, demb, ldde, dw_ih, dw_hh, db_ih,
               db_hh, dWp, dbp, B, T, d, (const float*)save);
    return q.err;
}

}  // extern "C"
