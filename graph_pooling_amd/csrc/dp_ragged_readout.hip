// The UNMASKED max readout of the base GCN encoder (GcnEncoderGraph, encoders.py:1083-1122) on a ragged batch of CSR
// graphs.  torch.max(x, dim=1) of the dense batch runs over all P = pad_to rows, the padded ones included, and behind
// apply_bn a padded row of node index i holds v[i, f] = (pad_f - mean_i) rstd_i: the layer's constant pushed through the
// statistics of ITS node index.  Nothing here stores a padded row:
//
//   dp_ragged_padval_fwd       the table v [n_idx, F] of those values, rows n_min .. n_idx - 1 (n_min = min_b n_b: lower
//                              indices have no padded row).  Row max_n, present when P > max_n, stands for every index
//                              >= max_n: all B rows of such an index hold `pad`, so they share one pair of statistics.
//   dp_ragged_suffix_max       sufv[i, f] = max_{j >= i} v[j, f] with the LOWEST j that attains it: what the padded rows
//                              of a graph with n_b = i contribute to its readout.  Two levels: maxima of 64-row blocks,
//                              then every block scans its rows downwards from the combined maxima of the blocks above.
//   dp_segment_max_floor_*     the segmented max of dp_segment_max_* with that table (graph b reads row n_b) or one
//                              constant row [F] (layers without BatchNorm, the last layer) as the floor of the graphs
//                              with padded rows; the backward splits dout into dZ (real winners) and G (padded winners).
//   dp_bn_ragged_g_bwd         dp_bn_ragged_bwd with the padded rows' output gradients G [n_idx, F].
//
// Max is exact and associative, so any tree gives the same bits; G is summed by one thread per column in ascending graph
// order.  No float atomics: every result is bit-reproducible.  Launch counts depend neither on B nor on max_n.
#include <algorithm>

#include "dp_entry.h"

namespace dp {
namespace {

constexpr float RR_BN_EPS = 1e-5f;      // BatchNorm1d eps (dp_csr_batch.hip RB_BN_EPS)
constexpr int RR_WAVES = 4;             // node indices per 256-thread workgroup
constexpr int SUF_ROWS = 64;            // table rows per scan block
constexpr int SUF_ROW_LANES = 4;        // row lanes of a block-maximum workgroup (x 64 feature lanes)

// One wave per table row i in n_min .. n_idx - 1.  i < max_n: the statistics dp_bn_ragged_fwd wrote.  i == max_n (the
// tail row): B * F values, B copies of pad — mean and biased variance over f of pad; written to stats row max_n.
__global__ __launch_bounds__(256) void k_ragged_padval(float* stats, const float* pad, float* padval, int ldp,
                                                       int n_min, int max_n, int n_idx, int F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = n_min + blockIdx.x * RR_WAVES + wave;
    if (i >= n_idx) return;
    float mu, rstd;
    if (i < max_n) {
        mu = stats[(long)i * 2];
        rstd = stats[(long)i * 2 + 1];
    } else {
        const float inv = 1.0f / (float)F;
        float s = 0.f, v2 = 0.f;
        if (pad)
            for (int f = lane; f < F; f += 64) s += pad[f];
        mu = wave64_sum(s) * inv;
        for (int f = lane; f < F; f += 64) {
            const float d = (pad ? pad[f] : 0.f) - mu;
            v2 += d * d;
        }
        rstd = 1.0f / sqrtf(wave64_sum(v2) * inv + RR_BN_EPS);
        if (lane == 0) {
            stats[(long)i * 2] = mu;
            stats[(long)i * 2 + 1] = rstd;
        }
    }
    float* row = padval + (long)i * ldp;
    for (int f = lane; f < F; f += 64) row[f] = ((pad ? pad[f] : 0.f) - mu) * rstd;
}

// Level 1: workgroup (ft, blk) takes rows n_min + blk * 64 .. of 64 features, 4 row lanes; ties to the lowest row.
__global__ __launch_bounds__(256) void k_suffix_block_max(const float* v, int ldv, int n_min, int n_idx, int F, float* bv,
                                                          int* bi) {
    __shared__ float sv[SUF_ROW_LANES][64];
    __shared__ int si[SUF_ROW_LANES][64];
    const int fl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + fl;
    const int r0 = n_min + blockIdx.y * SUF_ROWS, r1 = min(r0 + SUF_ROWS, n_idx);
    float best = -INFINITY;
    int idx = -1;
    if (f < F)
        for (int r = r0 + rl; r < r1; r += SUF_ROW_LANES) {
            const float x = v[(long)r * ldv + f];
            if (x > best) {
                best = x;
                idx = r;
            }
        }
    sv[rl][fl] = best;
    si[rl][fl] = idx;
    __syncthreads();
    if (rl == 0 && f < F) {
        for (int k = 1; k < SUF_ROW_LANES; ++k) {
            const float x = sv[k][fl];
            const int i = si[k][fl];
            if (i >= 0 && (x > best || (x == best && i < idx))) {
                best = x;
                idx = i;
            }
        }
        bv[(long)blockIdx.y * F + f] = best;
        bi[(long)blockIdx.y * F + f] = idx;
    }
}

// Level 2: thread (f, blk) combines the maxima of the blocks above its own in ascending order (strict >: the lowest
// index stays on equal values), then walks its rows downwards (>=: a lower row takes over an equal value).
__global__ __launch_bounds__(256) void k_suffix_scan(const float* v, int ldv, const float* bv, const int* bi, int n_min,
                                                     int n_idx, int n_blk, int F, float* sufv, int* sufi, int lds) {
    const int f = blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
    if (f >= F) return;
    float best = -INFINITY;
    int idx = -1;
    for (int k = blk + 1; k < n_blk; ++k) {
        const float x = bv[(long)k * F + f];
        const int i = bi[(long)k * F + f];
        if (i >= 0 && x > best) {
            best = x;
            idx = i;
        }
    }
    const int r0 = n_min + blk * SUF_ROWS, r1 = min(r0 + SUF_ROWS, n_idx);
    for (int r = r1 - 1; r >= r0; --r) {
        const float x = v[(long)r * ldv + f];
        if (x >= best) {
            best = x;
            idx = r;
        }
        sufv[(long)r * lds + f] = best;
        sufi[(long)r * lds + f] = idx;
    }
}

// Stage 2 of the segmented max: a graph's chunks in chunk order, then the floor of a graph with padded rows — row n_b of
// the suffix table (winner: its dense row index >= n_b) or the constant row (winner n_b).  A real row wins an exact tie:
// it has the lower dense index.
__global__ __launch_bounds__(256) void k_segment_max_floor_final(const float* pv, const int* pi, const int* chunk_off,
                                                                 const int* node_off, const int* floor_flag,
                                                                 const float* sufv, const int* sufi, int lds,
                                                                 int n_min, int n_idx, const float* floor_row, int F,
                                                                 float* out, int ldo, int* argmax, int lda) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    float best = -INFINITY;
    int bi = -1;
    for (int ch = chunk_off[b]; ch < chunk_off[b + 1]; ++ch) {       // ascending rows: strict > keeps the lowest row
        const float x = pv[(long)ch * F + f];
        const int i = pi[(long)ch * F + f];
        if (i >= 0 && x > best) {
            best = x;
            bi = i;
        }
    }
    const int nb = node_off[b + 1] - node_off[b];
    if (bi >= 0) bi -= node_off[b];
    if (floor_flag && floor_flag[b] && (floor_row || (sufv && nb >= n_min && nb < n_idx))) {
        const float fv = sufv ? sufv[(long)nb * lds + f] : floor_row[f];
        const int fi = sufv ? sufi[(long)nb * lds + f] : nb;
        if (fi >= nb && (bi < 0 || fv > best)) {
            best = fv;
            bi = fi;
        }
    }
    out[(long)b * ldo + f] = best;
    argmax[(long)b * lda + f] = bi;
}

// real winners: one thread per (b, f), one writer per dZ entry (dp_segment_max_bwd)
__global__ __launch_bounds__(256) void k_floor_bwd_real(const float* dout, int ldo, const int* argmax, int lda,
                                                        const int* node_off, float* dZ, int lddz, int B, int F) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * F) return;
    const int b = i / F, f = i % F;
    const int r = argmax[(long)b * lda + f];
    const int nb = node_off[b + 1] - node_off[b];
    if (r >= 0 && r < nb) dZ[((long)node_off[b] + r) * lddz + f] += dout[(long)b * ldo + f];
}

__global__ __launch_bounds__(256) void k_floor_zero_rows(float* G, int ldg, int r0, int r1, int F) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(r1 - r0) * F) return;
    G[((long)r0 + i / F) * ldg + i % F] = 0.f;
}

// padded winners: the thread of column f walks the graphs in ascending order.  table != 0: G [n_idx, F], zeroed before,
// G[i, f] += dout[b, f] for winner i in n_b .. n_idx - 1; table == 0: G [F] = the sum over the graphs whose floor won.
__global__ __launch_bounds__(256) void k_floor_bwd_pad(const float* dout, int ldo, const int* argmax, int lda,
                                                       const int* node_off, float* G, int ldg, int n_min, int n_idx,
                                                       int table, int B, int F) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float g = 0.f;
    for (int b = 0; b < B; ++b) {
        const int r = argmax[(long)b * lda + f];
        const int nb = node_off[b + 1] - node_off[b];
        if (r < nb) continue;
        const float d = dout[(long)b * ldo + f];
        if (!table)
            g += d;
        else if (r >= n_min && r < n_idx)
            G[(long)r * ldg + f] += d;
    }
    if (!table) G[f] = g;
}

struct BnRaggedGArgs {
    const float* x;         // [n_total, ldx] forward input (pre-ReLU), or y when relu == 0
    const float* y;         // [n_total, ldy] forward output (xhat)
    const float* dy;
    float* dx;
    const float* stats;     // [n_idx, 2] (mean, rstd)
    const int* node_off;    // [B + 1]
    const int* order;       // [B] graphs by size, largest first
    const int* cnt;         // [maxn] owners of each node index
    const float* pad;       // [F] or null (zeros)
    const float* G;         // [n_idx, ldg] output gradients of the padded rows, summed per (index, feature)
    float* dpad_part;       // [gridDim.x, F] per-workgroup partials of dpad, or null
    int ldx, ldy, lddy, lddx, ldg, B, maxn, nidx, F, relu;
};

// k_bn_ragged_bwd (dp_csr_batch.hip) with the padded rows' output gradients: the (B - cnt) padded rows of node index i
// together receive G[i, f] at xhat = v[i, f], which joins both means, and their own dx summed is
// rstd (G - (B - cnt) (m1 + v m2)).  The tail row (i == maxn) has no owner: cnt = 0.
__global__ __launch_bounds__(256) void k_bn_ragged_bwd_g(BnRaggedGArgs a) {
    extern __shared__ float dp_lds[];        // [RR_WAVES][F] when dpad_part
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * RR_WAVES + wave;
    const bool live = i < a.nidx;
    const int c = (live && i < a.maxn) ? min(a.cnt[i], a.B) : 0;
    const bool padded = live && c < a.B;
    const float inv = 1.0f / ((float)a.B * (float)a.F);
    const float mu = live ? a.stats[(long)i * 2] : 0.f, rstd = live ? a.stats[(long)i * 2 + 1] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < c; ++j) {
        const long row = (long)a.node_off[a.order[j]] + i;
        const float* gr = a.dy + row * a.lddy;
        const float* yr = a.y + row * a.ldy;
#pragma unroll 4
        for (int f = lane; f < a.F; f += 64) {
            const float g = gr[f];
            s1 += g;
            s2 += g * yr[f];
        }
    }
    if (padded) {
        const float* gp = a.G + (long)i * a.ldg;
        for (int f = lane; f < a.F; f += 64) {
            const float g = gp[f];
            const float xh = ((a.pad ? a.pad[f] : 0.f) - mu) * rstd;
            s1 += g;
            s2 += g * xh;
        }
    }
    const float m1 = wave64_sum(s1) * inv, m2 = wave64_sum(s2) * inv;
    for (int j = 0; j < c; ++j) {
        const long row = (long)a.node_off[a.order[j]] + i;
        const float* gr = a.dy + row * a.lddy;
        const float* yr = a.y + row * a.ldy;
        const float* xr = a.x + row * a.ldx;
        float* dr = a.dx + row * a.lddx;
#pragma unroll 4
        for (int f = lane; f < a.F; f += 64) {
            const float d = rstd * (gr[f] - m1 - yr[f] * m2);
            dr[f] = (!a.relu || xr[f] > 0.f) ? d : 0.f;
        }
    }
    if (!a.dpad_part) return;
    const float npad = (float)(a.B - c);
    for (int f = lane; f < a.F; f += 64) {
        float t = 0.f;
        if (padded) {
            const float xh = (a.pad[f] - mu) * rstd;
            t = rstd * (a.G[(long)i * a.ldg + f] - npad * (m1 + xh * m2));
        }
        dp_lds[wave * a.F + f] = t;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < a.F; f += 256)
        a.dpad_part[(long)blockIdx.x * a.F + f] =
            ((dp_lds[f] + dp_lds[a.F + f]) + dp_lds[2 * a.F + f]) + dp_lds[3 * a.F + f];
}

// out[f] = the sum over the `rows` partial rows of dpad: wave w takes rows w, w + 4, ... and the four wave sums are added
// in wave order, all in double, rounded once.  With G, dpad sums thousands of terms of both signs whose running sums
// reach hundreds of times an entry; fp32 running sums (k_ragged_colsum) would leave their rounding on it.
__global__ __launch_bounds__(256) void k_readout_colsum(const float* part, int rows, int F, float* out) {
    __shared__ double red[4][64];
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + l;
    double s = 0.0;
    if (f < F)
        for (int r = wave; r < rows; r += 4) s += (double)part[(long)r * F + f];
    red[wave][l] = s;
    __syncthreads();
    if (wave == 0 && f < F) out[f] = (float)(((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]);
}

}  // namespace
}  // namespace dp

using namespace dp;

namespace {
// the table's row range: n_min = min_b n_b <= max_n, n_idx = max_n or max_n + 1 (the tail row)
int check_table(const char* entry, int n_min, int max_n, int n_idx, int F) {
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "%s: F=%d must be positive", entry, F);
    DP_CHECK(F <= 2048, DP_ERR_UNSUPPORTED, "%s: F=%d above the supported 2048", entry, F);
    DP_CHECK(max_n >= 1 && n_min >= 1 && n_min <= max_n, DP_ERR_INVALID_ARG,
             "%s: n_min=%d, max_n=%d must satisfy 1 <= n_min <= max_n", entry, n_min, max_n);
    DP_CHECK(n_idx == max_n || n_idx == max_n + 1, DP_ERR_INVALID_ARG,
             "%s: n_idx=%d must be max_n=%d or max_n + 1 (the tail row)", entry, n_idx, max_n);
    return DP_OK;
}
}  // namespace

extern "C" {

int dp_ragged_padval_fwd(float* stats, const float* pad, float* padval, int ldp, int n_min, int max_n, int n_idx, int F,
                         void* stream) {
    DP_PTR(stats); DP_PTR(padval);
    if (int rc = check_table("dp_ragged_padval_fwd", n_min, max_n, n_idx, F)) return rc;
    DP_CHECK(ldp >= F, DP_ERR_INVALID_ARG, "dp_ragged_padval_fwd: ldp=%d smaller than F=%d", ldp, F);
    if (n_idx == n_min) return DP_OK;       // no node index has a padded row
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_ragged_padval, dim3(cdiv(n_idx - n_min, RR_WAVES)), dim3(256), 0, q.stream, stats, pad, padval,
                       ldp, n_min, max_n, n_idx, F);
    q.check_launch("ragged_padval");
    return q.err;
}

size_t dp_ragged_suffix_max_workspace_bytes(int n_min, int n_idx, int F) {
    if (n_min < 1 || n_idx <= n_min || F < 1 || F > 2048) return 0;
    return 2 * align256((size_t)cdiv(n_idx - n_min, SUF_ROWS) * F * sizeof(float));
}

int dp_ragged_suffix_max(const float* padval, int ldp, float* sufv, int* sufi, int lds, int n_min, int n_idx, int F,
                         void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(padval); DP_PTR(sufv); DP_PTR(sufi);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "dp_ragged_suffix_max: F=%d must be positive", F);
    DP_CHECK(F <= 2048, DP_ERR_UNSUPPORTED, "dp_ragged_suffix_max: F=%d above the supported 2048", F);
    DP_CHECK(n_min >= 1 && n_idx >= n_min, DP_ERR_INVALID_ARG,
             "dp_ragged_suffix_max: n_min=%d, n_idx=%d must satisfy 1 <= n_min <= n_idx", n_min, n_idx);
    DP_CHECK(ldp >= F && lds >= F, DP_ERR_INVALID_ARG, "dp_ragged_suffix_max: ldp=%d / lds=%d smaller than F=%d", ldp,
             lds, F);
    if (n_idx == n_min) return DP_OK;
    const int n_blk = cdiv(n_idx - n_min, SUF_ROWS);
    DP_CHECK(n_blk <= 65535, DP_ERR_UNSUPPORTED, "dp_ragged_suffix_max: more than 65535 scan blocks");
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    float* bv = q.alloc<float>((size_t)n_blk * F);
    int* bi = q.alloc<int>((size_t)n_blk * F);
    if (q.err) return q.err;
    hipLaunchKernelGGL(k_suffix_block_max, dim3(cdiv(F, 64), n_blk), dim3(256), 0, q.stream, padval, ldp, n_min, n_idx,
                       F, bv, bi);
    q.check_launch("suffix_block_max");
    hipLaunchKernelGGL(k_suffix_scan, dim3(cdiv(F, 256), n_blk), dim3(256), 0, q.stream, padval, ldp, (const float*)bv,
                       (const int*)bi, n_min, n_idx, n_blk, F, sufv, sufi, lds);
    q.check_launch("suffix_scan");
    return q.err;
}

int dp_segment_max_floor_fwd(const float* Z, int ldz, const int* node_off, const int* chunk_tab, const int* chunk_off,
                             int n_chunks, const int* floor_flag, const float* sufv, const int* sufi, int lds,
                             int n_min, int n_idx, const float* floor_row, float* out, int ldo, int* argmax, int B, int F, void* workspace,
                             size_t workspace_bytes, void* stream) {
    DP_PTR(Z); DP_PTR(node_off); DP_PTR(chunk_tab); DP_PTR(chunk_off); DP_PTR(out); DP_PTR(argmax);
    DP_CHECK(B >= 1 && F >= 1 && n_chunks >= B, DP_ERR_INVALID_ARG,
             "dp_segment_max_floor_fwd: B=%d, F=%d, n_chunks=%d (every graph has at least one chunk)", B, F, n_chunks);
    DP_CHECK(F <= 2048, DP_ERR_UNSUPPORTED, "dp_segment_max_floor_fwd: F=%d above the supported 2048", F);
    DP_CHECK(n_chunks <= 65535 && B <= 65535, DP_ERR_UNSUPPORTED,
             "dp_segment_max_floor_fwd: more than 65535 chunks / graphs");
    DP_CHECK(ldz >= F && ldo >= F, DP_ERR_INVALID_ARG, "dp_segment_max_floor_fwd: ldz=%d / ldo=%d smaller than F=%d", ldz,
             ldo, F);
    DP_CHECK(!(sufv && floor_row), DP_ERR_INVALID_ARG,
             "dp_segment_max_floor_fwd: the floor is the suffix table or one constant row, not both");
    DP_CHECK(!sufv == !sufi, DP_ERR_INVALID_ARG, "dp_segment_max_floor_fwd: sufv and sufi go together");
    DP_CHECK(!sufv || (lds >= F && n_min >= 1 && n_idx > n_min), DP_ERR_INVALID_ARG,
             "dp_segment_max_floor_fwd: lds=%d, n_min=%d, n_idx=%d for a suffix table of F=%d columns", lds, n_min, n_idx,
             F);
    DP_CHECK(!(sufv || floor_row) || floor_flag, DP_ERR_INVALID_ARG,
             "dp_segment_max_floor_fwd: a floor needs floor_flag (which graphs have padded rows)");
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    float* pv = q.alloc<float>((size_t)n_chunks * F);
    int* pi = q.alloc<int>((size_t)n_chunks * F);
    if (q.err) return q.err;
    segment_max_part(q, Z, ldz, chunk_tab, n_chunks, F, pv, pi);
    if (q.err) return q.err;
    hipLaunchKernelGGL(k_segment_max_floor_final, dim3(cdiv(F, 256), B), dim3(256), 0, q.stream, (const float*)pv,
                       (const int*)pi, chunk_off, node_off, floor_flag, sufv, sufi, lds, n_min, n_idx, floor_row, F, out, ldo,
                       argmax, F);
    q.check_launch("segment_max_floor_final");
    return q.err;
}

int dp_segment_max_floor_bwd(const float* dout, int ldo, const int* argmax, const int* node_off, float* dZ, int lddz,
                             float* G, int ldg, int n_min, int n_idx, int table, int B, int F, void* stream) {
    DP_PTR(dout); DP_PTR(argmax); DP_PTR(node_off); DP_PTR(dZ);
    DP_CHECK(B >= 1 && F >= 1, DP_ERR_INVALID_ARG, "dp_segment_max_floor_bwd: B=%d, F=%d must be positive", B, F);
    DP_CHECK(F <= 2048, DP_ERR_UNSUPPORTED, "dp_segment_max_floor_bwd: F=%d above the supported 2048", F);
    DP_CHECK(ldo >= F && lddz >= F, DP_ERR_INVALID_ARG, "dp_segment_max_floor_bwd: ldo=%d / lddz=%d smaller than F=%d",
             ldo, lddz, F);
    if (G) {
        DP_ALIGNED4(G);
        DP_CHECK(!table || (n_min >= 1 && n_idx >= n_min && ldg >= F), DP_ERR_INVALID_ARG,
                 "dp_segment_max_floor_bwd: n_min=%d, n_idx=%d, ldg=%d for a table of F=%d columns", n_min, n_idx, ldg, F);
    }
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_floor_bwd_real, dim3(cdiv((long)B * F, 256)), dim3(256), 0, q.stream, dout, ldo, argmax, F,
                       node_off, dZ, lddz, B, F);
    q.check_launch("segment_max_floor_bwd");
    if (G && table && n_idx > n_min) {
        hipLaunchKernelGGL(k_floor_zero_rows, dim3(cdiv((long)(n_idx - n_min) * F, 256)), dim3(256), 0, q.stream, G, ldg,
                           n_min, n_idx, F);
        q.check_launch("segment_max_floor_zero");
    }
    if (G && (!table || n_idx > n_min)) {
        hipLaunchKernelGGL(k_floor_bwd_pad, dim3(cdiv(F, 256)), dim3(256), 0, q.stream, dout, ldo, argmax, F, node_off, G,
                           ldg, n_min, n_idx, table ? 1 : 0, B, F);
        q.check_launch("segment_max_floor_pad");
    }
    return q.err;
}

int dp_bn_ragged_g_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                       float* dx, int lddx, float* dpad, const float* G, int ldg, const int* node_off, const int* order,
                       const int* cnt, const float* pad, int B, int max_n, int n_idx, int F, int relu, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!G)     // no padded row won anything: the plain backward over the real indices
        return dp_bn_ragged_bwd(x, ldx, y, ldy, stats, dy, lddy, dx, lddx, dpad, node_off, order, cnt, pad, B, max_n, F,
                                relu, workspace, workspace_bytes, stream);
    DP_PTR(y); DP_PTR(stats); DP_PTR(dy); DP_PTR(dx); DP_PTR(node_off); DP_PTR(order); DP_PTR(cnt);
    DP_ALIGNED4(G);
    DP_CHECK(!relu || x, DP_ERR_INVALID_ARG, "dp_bn_ragged_g_bwd: x is NULL but relu != 0");
    DP_CHECK(!dpad || pad, DP_ERR_INVALID_ARG, "dp_bn_ragged_g_bwd: dpad asked for but pad is NULL");
    DP_CHECK(B >= 1, DP_ERR_INVALID_ARG, "dp_bn_ragged_g_bwd: B=%d must be positive", B);
    if (int rc = check_table("dp_bn_ragged_g_bwd", 1, max_n, n_idx, F)) return rc;
    DP_CHECK(ldy >= F && lddy >= F && lddx >= F && ldg >= F && (!relu || ldx >= F), DP_ERR_INVALID_ARG,
             "dp_bn_ragged_g_bwd: a row stride is smaller than F=%d", F);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    const int blocks = cdiv(n_idx, RR_WAVES);
    float* part = dpad ? q.alloc<float>((size_t)blocks * F) : nullptr;
    if (q.err) return q.err;
    BnRaggedGArgs a{relu ? x : y, y, dy, dx, stats, node_off, order, cnt, pad, G, part,
                    relu ? ldx : ldy, ldy, lddy, lddx, ldg, B, max_n, n_idx, F, relu ? 1 : 0};
    hipLaunchKernelGGL(k_bn_ragged_bwd_g, dim3(blocks), dim3(256), dpad ? (size_t)RR_WAVES * F * sizeof(float) : 0,
                       q.stream, a);
    q.check_launch("bn_ragged_g_bwd");
    if (dpad) {
        hipLaunchKernelGGL(k_readout_colsum, dim3(cdiv(F, 64)), dim3(256), 0, q.stream, (const float*)part, blocks, F,
                           dpad);
        q.check_launch("bn_ragged_g_dpad");
    }
    return q.err;
}

}  // extern "C"
