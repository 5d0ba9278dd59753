// Row kernels of a RAGGED batch of CSR graphs (N4): B graphs whose node rows lie concatenated without padding,
// graph b in rows node_off[b] .. node_off[b + 1] - 1.  They compute what the dense kernels compute on the same graphs
// padded to N = max_b n_b, without storing a padded row:
//
//   dp_bn_ragged_*        apply_bn (encoders.py:1048-1052) per NODE INDEX over the batch.  In the dense batch a padded
//                         row of a GraphConv layer is the constant pad = relu(l2norm(bias)) (zero adjacency row), and it
//                         sits inside the statistics of its node index; here index i takes its statistics over the rows
//                         node_off[b] + i of the cnt[i] graphs that own it plus (B - cnt[i]) copies of `pad`.
//   dp_gcn_pad_const_*    that constant from the layer's bias, and the way back from its gradient to the bias gradient.
//   dp_gcn_row_const_*    the same without the ReLU: a padded row behind the last GraphConv layer (dp_ragged_readout.hip).
//   dp_segment_max_*      max readout per graph (encoders.py:1257) with the zero floor of a graph that has padded rows.
//
// Ownership.  `order` lists the graphs by size, largest first (ties by graph number), so the owners of index i are
// order[0 .. cnt[i] - 1]: below the smallest size every graph, from the second-largest size upward a single one.  A
// wave owns one node index whatever its owner count and walks the owners in that order; lanes stride over the
// features.  Wide ownership is never assumed: a batch of one giant graph gets max_b n_b waves.  That is a statement
// about correctness and grid size, not about speed — at the model's widths (F 20..32) under half of a wave's lanes are
// active and an index every graph owns costs three serial passes over B rows; packing 64 / F indices per wave is the
// open item.
// Every reduction has a fixed order and there are no float atomics: results are bit-reproducible run to run.
#include <algorithm>

#include "dp_entry.h"

namespace dp {
namespace {

constexpr float RB_BN_EPS = 1e-5f;      // BatchNorm1d eps (dp_rowops.hip BN_EPS)
constexpr float RB_L2_EPS = 1e-12f;     // F.normalize eps (dp_rowops.hip L2_EPS)
constexpr int RB_WAVES = 4;             // node indices per 256-thread workgroup
constexpr int SEG_ROW_LANES = 4;        // row lanes of a segment-max workgroup (x 64 feature lanes)

struct BnRaggedArgs {
    const float* x;         // [n_total, ldx] forward input (pre-ReLU)
    const float* y;         // [n_total, ldy] forward output (xhat); written by the forward
    const float* dy;        // backward only
    float* out;             // forward: y; backward: dx
    float* stats;           // [maxn, 2] (mean, rstd)
    const int* node_off;    // [B + 1]
    const int* order;       // [B] graphs by size, largest first
    const int* cnt;         // [maxn] owners of each node index
    const float* pad;       // [F] or null (zeros)
    float* dpad_part;       // backward: [gridDim.x, F] per-workgroup partials of dpad, or null
    int ldx, ldy, lddy, ldo, B, maxn, F, relu;
};

__global__ __launch_bounds__(256) void k_bn_ragged_fwd(BnRaggedArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * RB_WAVES + wave;
    if (i >= a.maxn) return;
    const int c = min(a.cnt[i], a.B);
    const float npad = (float)(a.B - c);
    const float inv = 1.0f / ((float)a.B * (float)a.F);
    // mean
    float s = 0.f, ps = 0.f;
    for (int j = 0; j < c; ++j) {
        const float* xr = a.x + ((long)a.node_off[a.order[j]] + i) * a.ldx;
#pragma unroll 4
        for (int f = lane; f < a.F; f += 64) {
            const float v = xr[f];
            s += a.relu ? fmaxf(v, 0.f) : v;
        }
    }
    if (a.pad && c < a.B)
        for (int f = lane; f < a.F; f += 64) ps += a.pad[f];
    const float mu = (wave64_sum(s) + npad * wave64_sum(ps)) * inv;
    // biased variance around the mean
    float v2 = 0.f, p2 = 0.f;
    for (int j = 0; j < c; ++j) {
        const float* xr = a.x + ((long)a.node_off[a.order[j]] + i) * a.ldx;
#pragma unroll 4
        for (int f = lane; f < a.F; f += 64) {
            const float v = xr[f];
            const float d = (a.relu ? fmaxf(v, 0.f) : v) - mu;
            v2 += d * d;
        }
    }
    if (c < a.B)
        for (int f = lane; f < a.F; f += 64) {
            const float d = (a.pad ? a.pad[f] : 0.f) - mu;
            p2 += d * d;
        }
    const float var = (wave64_sum(v2) + npad * wave64_sum(p2)) * inv;
    const float rstd = 1.0f / sqrtf(var + RB_BN_EPS);
    for (int j = 0; j < c; ++j) {
        const long row = (long)a.node_off[a.order[j]] + i;
        const float* xr = a.x + row * a.ldx;
        float* yr = a.out + row * a.ldo;
#pragma unroll 4
        for (int f = lane; f < a.F; f += 64) {
            const float v = xr[f];
            yr[f] = ((a.relu ? fmaxf(v, 0.f) : v) - mu) * rstd;
        }
    }
    if (lane == 0) {
        a.stats[(long)i * 2] = mu;
        a.stats[(long)i * 2 + 1] = rstd;
    }
}

// dx = gate * rstd * (dy - mean(dy) - xhat * mean(dy * xhat)), the means over the B * F values of the node index (a
// padded row has dy = 0).  The padded rows' own dx — rstd * (-mean(dy) - xhat_pad * mean(dy * xhat)), (B - cnt) copies —
// is the gradient of `pad`: each workgroup adds its node indices' terms in index order into one partial row.
__global__ __launch_bounds__(256) void k_bn_ragged_bwd(BnRaggedArgs a) {
    extern __shared__ float dp_lds[];        // [RB_WAVES][F] when dpad_part
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * RB_WAVES + wave;
    const bool live = i < a.maxn;
    const int c = live ? min(a.cnt[i], a.B) : 0;
    const float inv = 1.0f / ((float)a.B * (float)a.F);
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
    const float m1 = wave64_sum(s1) * inv, m2 = wave64_sum(s2) * inv;
    const float mu = live ? a.stats[(long)i * 2] : 0.f, rstd = live ? a.stats[(long)i * 2 + 1] : 0.f;
    for (int j = 0; j < c; ++j) {
        const long row = (long)a.node_off[a.order[j]] + i;
        const float* gr = a.dy + row * a.lddy;
        const float* yr = a.y + row * a.ldy;
        const float* xr = a.x + row * a.ldx;
        float* dr = a.out + row * a.ldo;
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
        if (live && c < a.B) {
            const float xh = (a.pad[f] - mu) * rstd;
            t = npad * rstd * (-m1 - xh * m2);
        }
        dp_lds[wave * a.F + f] = t;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < a.F; f += 256)
        a.dpad_part[(long)blockIdx.x * a.F + f] =
            ((dp_lds[f] + dp_lds[a.F + f]) + dp_lds[2 * a.F + f]) + dp_lds[3 * a.F + f];
}

// out[f] = sum over the `rows` partial rows, wave w taking rows w, w + 4, ... and the four wave sums added in wave
// order (the fixed tree of k_csr_pool_reduce)
__global__ __launch_bounds__(256) void k_ragged_colsum(const float* part, int rows, int F, float* out) {
    __shared__ float red[4][64];
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + l;
    float s = 0.f;
    if (f < F)
        for (int r = wave; r < rows; r += 4) s += part[(long)r * F + f];
    red[wave][l] = s;
    __syncthreads();
    if (wave == 0 && f < F) out[f] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
}

// fixed tree over the 256 threads of the workgroup
__device__ __forceinline__ float block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// pad = relu(u), u = bias / max(||bias||, 1e-12) (the GraphConv output of a row with a zero adjacency row); one workgroup.
// relu = 0: u itself (the last GraphConv layer has no ReLU behind it)
__global__ __launch_bounds__(256) void k_pad_const_fwd(const float* bias, float* pad, int F, int normalize, int relu) {
    __shared__ float red[256];
    float ss = 0.f;
    if (bias)
        for (int f = threadIdx.x; f < F; f += 256) ss += bias[f] * bias[f];
    ss = block_sum(ss, red);
    const float inv = normalize ? 1.f / fmaxf(sqrtf(ss), RB_L2_EPS) : 1.f;
    for (int f = threadIdx.x; f < F; f += 256) {
        const float u = bias ? bias[f] * inv : 0.f;
        pad[f] = relu ? fmaxf(u, 0.f) : u;
    }
}
// dbias = J^T (dpad * [u > 0]): J of u = b / max(||b||, eps) is inv (I - u u^T) above eps and inv I below
// (dp_rowops.hip `project`).  A zero bias gives u = 0, every ReLU gate closed and dbias = 0, as torch's relu'(0) = 0.
// relu = 0: no gate
__global__ __launch_bounds__(256) void k_pad_const_bwd(const float* bias, const float* dpad, float* dbias, int F,
                                                       int normalize, int relu) {
    __shared__ float red[256];
    float ss = 0.f;
    for (int f = threadIdx.x; f < F; f += 256) ss += bias[f] * bias[f];
    ss = block_sum(ss, red);
    const float inv = normalize ? 1.f / fmaxf(sqrtf(ss), RB_L2_EPS) : 1.f;
    const bool project = normalize && (inv < 1.0f / RB_L2_EPS);
    float dot = 0.f;
    for (int f = threadIdx.x; f < F; f += 256) {
        const float u = bias[f] * inv;
        dot += ((!relu || u > 0.f) ? dpad[f] : 0.f) * u;
    }
    dot = block_sum(dot, red);
    for (int f = threadIdx.x; f < F; f += 256) {
        const float u = bias[f] * inv;
        const float du = (!relu || u > 0.f) ? dpad[f] : 0.f;
        dbias[f] = inv * (du - (project ? u * dot : 0.f));
    }
}

// ------------------------------------------------------------------ segmented max readout
// Stage 1: workgroup (ft, ch) walks chunk ch of the chunk table — {graph, first row, end row, 0}, rows global, a chunk
// never crosses a graph boundary — for 64 features: 4 row lanes, ties to the lowest row (torch CPU max).  Stage 2
// combines a graph's chunks in chunk order and applies the zero floor exactly as k_masked_max_fwd does.
__global__ __launch_bounds__(256) void k_segment_max_part(const float* Z, int ldz, const int* tab, int F, float* pv,
                                                          int* pi) {
    __shared__ float sv[SEG_ROW_LANES][64];
    __shared__ int si[SEG_ROW_LANES][64];
    const int fl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + fl;
    const int ch = blockIdx.y;
    const int rbeg = tab[ch * 4 + 1], rend = tab[ch * 4 + 2];
    float best = -INFINITY;
    int bi = -1;
    if (f < F) {
        const float* z = Z + f;
#pragma unroll 4
        for (int r = rbeg + rl; r < rend; r += SEG_ROW_LANES) {
            const float v = z[(long)r * ldz];
            if (v > best) {
                best = v;
                bi = r;
            }
        }
    }
    sv[rl][fl] = best;
    si[rl][fl] = bi;
    __syncthreads();
    if (rl == 0 && f < F) {
        for (int k = 1; k < SEG_ROW_LANES; ++k) {
            const float v = sv[k][fl];
            const int i = si[k][fl];
            if (i >= 0 && (v > best || (v == best && i < bi))) {
                best = v;
                bi = i;
            }
        }
        pv[(long)ch * F + f] = best;
        pi[(long)ch * F + f] = bi;
    }
}
__global__ __launch_bounds__(256) void k_segment_max_final(const float* pv, const int* pi, const int* chunk_off,
                                                           const int* node_off, const int* floor_flag, int F,
                                                           float* out, int ldo, int* argmax, int lda) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    float best = -INFINITY;
    int bi = -1;
    for (int ch = chunk_off[b]; ch < chunk_off[b + 1]; ++ch) {       // ascending rows: strict > keeps the lowest row
        const float v = pv[(long)ch * F + f];
        const int i = pi[(long)ch * F + f];
        if (i >= 0 && v > best) {
            best = v;
            bi = i;
        }
    }
    if (bi >= 0) bi -= node_off[b];
    if (floor_flag && floor_flag[b] && !(best > 0.f)) {
        if (best < 0.f || bi < 0) {       // on an exact tie (best == 0) the real row has the lower index
            best = 0.f;
            bi = -1;
        }
    }
    out[(long)b * ldo + f] = best;
    argmax[(long)b * lda + f] = bi;
}
__global__ __launch_bounds__(256) void k_segment_max_bwd(const float* dout, int ldo, const int* argmax, int lda,
                                                         const int* node_off, float* dZ, int lddz, int B, int F) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * F) return;
    const int b = i / F, f = i % F;
    const int r = argmax[(long)b * lda + f];
    const int nb = node_off[b + 1] - node_off[b];
    if (r >= 0 && r < nb) dZ[((long)node_off[b] + r) * lddz + f] += dout[(long)b * ldo + f];
}

}  // namespace

void segment_max_part(Seq& q, const float* Z, int ldz, const int* chunk_tab, int n_chunks, int F, float* pv, int* pi) {
    if (!q.ok()) return;
    hipLaunchKernelGGL(k_segment_max_part, dim3(cdiv(F, 64), n_chunks), dim3(256), 0, q.stream, Z, ldz, chunk_tab, F, pv,
                       pi);
    q.check_launch("segment_max_part");
}

}  // namespace dp

using namespace dp;

namespace {
int check_ragged(const char* entry, int B, int maxn, int F) {
    DP_CHECK(B >= 1, DP_ERR_INVALID_ARG, "%s: B=%d must be positive", entry, B);
    DP_CHECK(maxn >= 1, DP_ERR_INVALID_ARG, "%s: max_n=%d must be positive", entry, maxn);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "%s: F=%d must be positive", entry, F);
    DP_CHECK(F <= 2048, DP_ERR_UNSUPPORTED, "%s: F=%d above the supported 2048", entry, F);
    return DP_OK;
}
}  // namespace

extern "C" {

size_t dp_bn_ragged_workspace_bytes(int max_n, int F) {
    if (max_n < 1 || F < 1 || F > 2048) return 0;
    return align256((size_t)cdiv(max_n, RB_WAVES) * F * sizeof(float));
}

int dp_bn_ragged_fwd(const float* x, int ldx, float* y, int ldy, float* stats, const int* node_off, const int* order,
                     const int* cnt, const float* pad, int B, int max_n, int F, int relu, void* stream) {
    DP_PTR(x); DP_PTR(y); DP_PTR(stats); DP_PTR(node_off); DP_PTR(order); DP_PTR(cnt);
    if (int rc = check_ragged("dp_bn_ragged_fwd", B, max_n, F)) return rc;
    DP_CHECK(ldx >= F && ldy >= F, DP_ERR_INVALID_ARG, "dp_bn_ragged_fwd: ldx=%d / ldy=%d smaller than F=%d", ldx, ldy, F);
    Seq q((hipStream_t)stream, nullptr, 0);
    BnRaggedArgs a{x, nullptr, nullptr, y, stats, node_off, order, cnt, pad, nullptr, ldx, ldy, 0, ldy, B, max_n, F,
                   relu ? 1 : 0};
    hipLaunchKernelGGL(k_bn_ragged_fwd, dim3(cdiv(max_n, RB_WAVES)), dim3(256), 0, q.stream, a);
    q.check_launch("bn_ragged_fwd");
    return q.err;
}

int dp_bn_ragged_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                     float* dx, int lddx, float* dpad, const int* node_off, const int* order, const int* cnt,
                     const float* pad, int B, int max_n, int F, int relu, void* workspace, size_t workspace_bytes,
                     void* stream) {
    DP_PTR(y); DP_PTR(stats); DP_PTR(dy); DP_PTR(dx); DP_PTR(node_off); DP_PTR(order); DP_PTR(cnt);
    DP_CHECK(!relu || x, DP_ERR_INVALID_ARG, "dp_bn_ragged_bwd: x is NULL but relu != 0");
    DP_CHECK(!dpad || pad, DP_ERR_INVALID_ARG, "dp_bn_ragged_bwd: dpad asked for but pad is NULL");
    if (int rc = check_ragged("dp_bn_ragged_bwd", B, max_n, F)) return rc;
    DP_CHECK(ldy >= F && lddy >= F && lddx >= F && (!relu || ldx >= F), DP_ERR_INVALID_ARG,
             "dp_bn_ragged_bwd: a row stride is smaller than F=%d", F);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    const int blocks = cdiv(max_n, RB_WAVES);
    float* part = dpad ? q.alloc<float>((size_t)blocks * F) : nullptr;
    if (q.err) return q.err;
    BnRaggedArgs a{relu ? x : y, y, dy, dx, const_cast<float*>(stats), node_off, order, cnt, pad, part,
                   relu ? ldx : ldy, ldy, lddy, lddx, B, max_n, F, relu ? 1 : 0};
    hipLaunchKernelGGL(k_bn_ragged_bwd, dim3(blocks), dim3(256), dpad ? (size_t)RB_WAVES * F * sizeof(float) : 0,
                       q.stream, a);
    q.check_launch("bn_ragged_bwd");
    if (dpad) {
        hipLaunchKernelGGL(k_ragged_colsum, dim3(cdiv(F, 64)), dim3(256), 0, q.stream, (const float*)part, blocks, F,
                           dpad);
        q.check_launch("bn_ragged_dpad");
    }
    return q.err;
}

int dp_gcn_pad_const_fwd(const float* bias, float* pad, int F, int flags, void* stream) {
    DP_PTR(pad);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "dp_gcn_pad_const_fwd: F=%d must be positive", F);
    DP_CHECK(!(flags & DP_F_ADD_SELF), DP_ERR_UNSUPPORTED,
             "dp_gcn_pad_const_fwd: with DP_F_ADD_SELF a padded row is not a constant of the layer");
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_pad_const_fwd, dim3(1), dim3(256), 0, q.stream, bias, pad, F, (flags & DP_F_NORMALIZE) ? 1 : 0,
                       1);
    q.check_launch("gcn_pad_const_fwd");
    return q.err;
}

int dp_gcn_pad_const_bwd(const float* bias, const float* dpad, float* dbias, int F, int flags, void* stream) {
    DP_PTR(bias); DP_PTR(dpad); DP_PTR(dbias);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "dp_gcn_pad_const_bwd: F=%d must be positive", F);
    DP_CHECK(!(flags & DP_F_ADD_SELF), DP_ERR_UNSUPPORTED,
             "dp_gcn_pad_const_bwd: with DP_F_ADD_SELF a padded row is not a constant of the layer");
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_pad_const_bwd, dim3(1), dim3(256), 0, q.stream, bias, dpad, dbias, F,
                       (flags & DP_F_NORMALIZE) ? 1 : 0, 1);
    q.check_launch("gcn_pad_const_bwd");
    return q.err;
}

int dp_gcn_row_const_fwd(const float* bias, float* c, int F, int flags, void* stream) {
    DP_PTR(c);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "dp_gcn_row_const_fwd: F=%d must be positive", F);
    DP_CHECK(!(flags & DP_F_ADD_SELF), DP_ERR_UNSUPPORTED,
             "dp_gcn_row_const_fwd: with DP_F_ADD_SELF a padded row is not a constant of the layer");
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_pad_const_fwd, dim3(1), dim3(256), 0, q.stream, bias, c, F, (flags & DP_F_NORMALIZE) ? 1 : 0, 0);
    q.check_launch("gcn_row_const_fwd");
    return q.err;
}

int dp_gcn_row_const_bwd(const float* bias, const float* dc, float* dbias, int F, int flags, void* stream) {
    DP_PTR(bias); DP_PTR(dc); DP_PTR(dbias);
    DP_CHECK(F >= 1, DP_ERR_INVALID_ARG, "dp_gcn_row_const_bwd: F=%d must be positive", F);
    DP_CHECK(!(flags & DP_F_ADD_SELF), DP_ERR_UNSUPPORTED,
             "dp_gcn_row_const_bwd: with DP_F_ADD_SELF a padded row is not a constant of the layer");
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_pad_const_bwd, dim3(1), dim3(256), 0, q.stream, bias, dc, dbias, F,
                       (flags & DP_F_NORMALIZE) ? 1 : 0, 0);
    q.check_launch("gcn_row_const_bwd");
    return q.err;
}

size_t dp_segment_max_workspace_bytes(int n_chunks, int F) {
    if (n_chunks < 1 || F < 1) return 0;
    return 2 * align256((size_t)n_chunks * F * sizeof(float));
}

int dp_segment_max_fwd(const float* Z, int ldz, const int* node_off, const int* chunk_tab, const int* chunk_off,
                       int n_chunks, const int* floor_flag, float* out, int ldo, int* argmax, int B, int F,
                       void* workspace, size_t workspace_bytes, void* stream) {
    DP_PTR(Z); DP_PTR(node_off); DP_PTR(chunk_tab); DP_PTR(chunk_off); DP_PTR(out); DP_PTR(argmax);
    DP_CHECK(B >= 1 && F >= 1 && n_chunks >= B, DP_ERR_INVALID_ARG,
             "dp_segment_max_fwd: B=%d, F=%d, n_chunks=%d (every graph has at least one chunk)", B, F, n_chunks);
    DP_CHECK(n_chunks <= 65535 && B <= 65535, DP_ERR_UNSUPPORTED, "dp_segment_max_fwd: more than 65535 chunks / graphs");
    DP_CHECK(ldz >= F && ldo >= F, DP_ERR_INVALID_ARG, "dp_segment_max_fwd: ldz=%d / ldo=%d smaller than F=%d", ldz, ldo, F);
    Seq q((hipStream_t)stream, workspace, workspace_bytes);
    float* pv = q.alloc<float>((size_t)n_chunks * F);
    int* pi = q.alloc<int>((size_t)n_chunks * F);
    if (q.err) return q.err;
    hipLaunchKernelGGL(k_segment_max_part, dim3(cdiv(F, 64), n_chunks), dim3(256), 0, q.stream, Z, ldz, chunk_tab, F, pv,
                       pi);
    q.check_launch("segment_max_part");
    hipLaunchKernelGGL(k_segment_max_final, dim3(cdiv(F, 256), B), dim3(256), 0, q.stream, (const float*)pv,
                       (const int*)pi, chunk_off, node_off, floor_flag, F, out, ldo, argmax, F);
    q.check_launch("segment_max_final");
    return q.err;
}

int dp_segment_max_bwd(const float* dout, int ldo, const int* argmax, const int* node_off, float* dZ, int lddz, int B,
                       int F, void* stream) {
    DP_PTR(dout); DP_PTR(argmax); DP_PTR(node_off); DP_PTR(dZ);
    DP_CHECK(B >= 1 && F >= 1, DP_ERR_INVALID_ARG, "dp_segment_max_bwd: B=%d, F=%d must be positive", B, F);
    DP_CHECK(ldo >= F && lddz >= F, DP_ERR_INVALID_ARG, "dp_segment_max_bwd: ldo=%d / lddz=%d smaller than F=%d", ldo, lddz, F);
    Seq q((hipStream_t)stream, nullptr, 0);
    hipLaunchKernelGGL(k_segment_max_bwd, dim3(cdiv((long)B * F, 256)), dim3(256), 0, q.stream, dout, ldo, argmax, F,
                       node_off, dZ, lddz, B, F);
    q.check_launch("segment_max_bwd");
    return q.err;
}

}  // extern "C"
