// extern "C" boundary of libdiffpool_hip.so: argument checks, then the launch sequences.
#include <cstdarg>

#include <cmath>

#include "dp_entry.h"

namespace dp {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

const Knobs& knobs() {
    static Knobs k;
    static std::once_flag once;
    std::call_once(once, [] {
        auto num = [](const char* name, long dflt) {
            const char* e = getenv(name);
            return e ? atol(e) : dflt;
        };
        k.agg_wide = (int)num("DP_AGG_WIDE", -1);
        k.agg_rt = (int)num("DP_AGG_RT", 0);
#ifdef DP_STAMP
        k.agg_debug = (int)num("DP_AGG_DEBUG", 0);
#else
        k.agg_debug = 0;
#endif
        k.no_pack = getenv("DP_NO_PACK") != nullptr;
        k.gemm_trace = getenv("DP_GEMM_TRACE") != nullptr;
        k.gemm_target_wgs = num("DP_GEMM_TARGET_WGS", 0);
        k.node_ksplit = (int)num("DP_NODE_KSPLIT", 0);
        k.no_head_fusion = getenv("DP_NO_HEAD_FUSION") != nullptr;
        k.no_level_fusion = getenv("DP_NO_LEVEL_FUSION") != nullptr;
        k.no_head_fold = getenv("DP_NO_HEAD_FOLD") != nullptr;
        k.no_split_gemm = getenv("DP_NO_SPLIT_GEMM") != nullptr;
        k.split_gemm_w4 = getenv("DP_SPLIT_GEMM_W4") != nullptr;
        k.no_agg_first = getenv("DP_NO_AGG_FIRST") != nullptr;
        k.no_widen_fusion = getenv("DP_NO_WIDEN_FUSION") != nullptr;
        k.no_rowpart_hook = getenv("DP_NO_ROWPART_HOOK") != nullptr;
        k.no_row_quads = getenv("DP_NO_ROW_QUADS") != nullptr;
        k.test_barrier_fail = getenv("DP_TEST_BARRIER_FAIL") != nullptr;
        k.no_l0_persist = getenv("DP_NO_L0_PERSIST") != nullptr;
        k.no_l0_persist_bwd = getenv("DP_NO_L0_PERSIST_BWD") != nullptr;
    });
    return k;
}

// ---- device-side failure word: one pinned, device-mapped host int per device ordinal (diffpool_hip.h); the same block
// carries, 64 ints further on, what the last persistent level-0 backward reports (level0_verdict_block)
namespace {
constexpr int DEV_BLOCK_INTS = 64 + 1 + 64 + 1, DEV_VERDICT_OFF = 64;
struct DevErrSlot {
    std::once_flag once;
    int* host = nullptr;
    int* dev = nullptr;
};
DevErrSlot g_dev_err[64];
DevErrSlot* dev_err_slot() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
    DevErrSlot& s = g_dev_err[d];
    std::call_once(s.once, [&s] {
        void* h = nullptr;
        if (hipHostMalloc(&h, DEV_BLOCK_INTS * sizeof(int), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return; }
        memset(h, 0, DEV_BLOCK_INTS * sizeof(int));
        void* dv = nullptr;
        if (hipHostGetDevicePointer(&dv, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return; }
        s.host = (int*)h;
        s.dev = (int*)dv;
    });
    return s.host ? &s : nullptr;
}
}  // namespace
int* device_error_word() {
    DevErrSlot* s = dev_err_slot();
    return s ? s->dev : nullptr;
}
int* level0_verdict_block() {
    DevErrSlot* s = dev_err_slot();
    return s ? s->dev + DEV_VERDICT_OFF : nullptr;
}
int device_error_take(bool clear) {
    DevErrSlot* s = dev_err_slot();
    if (!s) return 0;
    return clear ? __atomic_exchange_n(s->host, 0, __ATOMIC_ACQ_REL) : __atomic_load_n(s->host, __ATOMIC_ACQUIRE);
}
static int level0_verdicts_read(int* verdicts, int capacity, int* count, int* rows_per_block) {
    DevErrSlot* s = dev_err_slot();
    *count = 0;
    if (rows_per_block) *rows_per_block = 0;
    if (!s) return DP_OK;                      // no device: nothing ever ran
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("dp_level0_bwd_symmetric: hipDeviceSynchronize: %s", hipGetErrorString(e));
        return (int)e;
    }
    const volatile int* v = s->host + DEV_VERDICT_OFF;
    int n = v[0];
    n = n < 0 ? 0 : (n > 64 ? 64 : n);
    for (int b = 0; b < n && b < capacity; ++b) verdicts[b] = v[1 + b];
    *count = n;
    if (rows_per_block) *rows_per_block = n ? v[65] : 0;
    return DP_OK;
}
static const char* device_error_text(int mask) {
    if ((mask & DP_DEVERR_BARRIER) && (mask & DP_DEVERR_NONFINITE_GRAD))
        return "a whole-level kernel's grid barrier gave up (its workgroups were not co-resident: is the device shared? "
               "set DP_NO_L0_PERSIST=1 DP_NO_LEVEL_FUSION=1) and dp_clip_adam_step refused the resulting non-finite "
               "gradients";
    if (mask & DP_DEVERR_BARRIER)
        return "a whole-level kernel's grid barrier gave up: its workgroups were not co-resident (is the device shared "
               "with another process or stream? set DP_NO_L0_PERSIST=1 DP_NO_LEVEL_FUSION=1); that step's outputs are "
               "NaN";
    if (mask & DP_DEVERR_NONFINITE_GRAD)
        return "dp_clip_adam_step met a non-finite gradient norm and skipped the update (parameters untouched)";
    return mask ? "unknown device error bits" : "no device error";
}
int device_error_gate(const char* entry) {
    const int m = device_error_take(false);
    if (!m) return DP_OK;
    device_error_take(true);
    set_error("%s: a kernel of an EARLIER call on this device failed (mask %d): %s", entry, m, device_error_text(m));
    return DP_ERR_DEVICE;
}

void ensure_dyn_lds(Seq& q, DynLdsOnce& st, const void* fn, int bytes, const char* what) {
    if (q.err || q.dry) return;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < 64 &&
        (st.done.load(std::memory_order_acquire) >> dev & 1ull))
        return;
    std::lock_guard<std::mutex> lock(st.m);
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("%s: hipFuncSetAttribute(max dynamic LDS = %d): %s", what, bytes, hipGetErrorString(e));
        q.err = (int)e;
        return;
    }
    if (dev >= 0 && dev < 64) st.done.fetch_or(1ull << dev, std::memory_order_release);
}

namespace {

RowGroups one_group(int w) {
    RowGroups g{};
    g.G = 1;
    g.c0[0] = 0;
    g.w[0] = w;
    return g;
}
GroupPtrs gp(float* p, int ld) {
    GroupPtrs r{};
    r.p[0] = p;
    r.ld[0] = ld;
    return r;
}
GroupCPtrs gcp(const float* p, int ld) {
    GroupCPtrs r{};
    r.p[0] = p;
    r.ld[0] = ld;
    return r;
}

// ---- op-level sequences (each usable in dry mode for workspace sizing)
void gcn_layer_fwd_seq(Seq& q, const float* x, int ldx, const float* adj, const float* W, const float* bias, float* y,
                       int ldy, float* invn, int B, int n, int Fin, int Fout, int flags) {
    float* P = q.alloc<float>((size_t)B * n * Fout);
    float* U = q.alloc<float>((size_t)B * n * Fout);
    if (q.err) return;
    bgemm(q, x, W, P, nullptr, B, n, Fout, Fin, ldx, Fout, Fout, (long)n * ldx, 0, (long)n * Fout, false, false, 1.f,
          0.f, 0);
    const float* selfp = (flags & DP_F_ADD_SELF) ? P : nullptr;
    const int norm = (flags & DP_F_NORMALIZE) ? 1 : 0;
    if (!aggregate_rownorm_fwd(q, adj, P, Fout, selfp, gcp(bias, 0), one_group(Fout), gp(y, ldy), invn, nullptr, B, n,
                               norm, 0)) {
        bgemm(q, adj, P, U, nullptr, B, n, Fout, n, n, Fout, Fout, (long)n * n, (long)n * Fout, (long)n * Fout, false,
              false, 1.f, 0.f, 0);
        rownorm_fwd(q, U, Fout, selfp, gcp(bias, 0), one_group(Fout), gp(y, ldy), invn, nullptr, (long)B * n, norm, 0);
    }
}

void gcn_layer_bwd_seq(Seq& q, const float* x, int ldx, const float* adj, const float* W, const float* y, int ldy,
                       const float* invn, const float* dy, int lddy, float* dx, int lddx, float* dW, float* db,
                       float* dadj, int B, int n, int Fin, int Fout, int flags) {
    float* dU = q.alloc<float>((size_t)B * n * Fout);
    float* G = q.alloc<float>((size_t)B * n * Fout);
    float* P = dadj ? q.alloc<float>((size_t)B * n * Fout) : nullptr;
    if (q.err) return;
    const int norm = (flags & DP_F_NORMALIZE) ? 1 : 0;
    rownorm_bwd(q, gcp(dy, lddy), gcp(nullptr, 0), gcp(y, ldy), invn, nullptr, nullptr, one_group(Fout), dU, Fout,
                nullptr, B, n, 0, 0, norm);
    if (db) colsum_batched(q, dU, Fout, 0, B * n, Fout, db, 0, 1);
    aggregate(q, adj, dU, Fout, G, Fout, B, n, Fout, true, 0.f);
    if (flags & DP_F_ADD_SELF) axpy(q, G, dU, 1.f, (long)B * n * Fout);
    // dW = sum_b x_b^T G_b: one contraction over K = B*n rows (x rows of consecutive graphs are ldx apart)
    bgemm(q, x, G, dW, nullptr, 1, Fin, Fout, B * n, ldx, Fout, Fout, 0, 0, 0, true, false, 1.f, 0.f, 0);
    if (dx)
        bgemm(q, G, W, dx, nullptr, B, n, Fin, Fout, Fout, Fout, lddx, (long)n * Fout, 0, (long)n * lddx, false, true,
              1.f, 0.f, 0);
    if (dadj) {
        bgemm(q, x, W, P, nullptr, B, n, Fout, Fin, ldx, Fout, Fout, (long)n * ldx, 0, (long)n * Fout, false, false,
              1.f, 0.f, 0);
        bgemm(q, dU, P, dadj, nullptr, B, n, n, Fout, Fout, Fout, n, (long)n * Fout, (long)n * Fout, (long)n * n, false,
              true, 1.f, 0.f, 0);
    }
}

void bn_fwd_seq(Seq& q, const float* x, int ldx, float* y, int ldy, float* stats, int B, int n, int F, int relu) {
    float* part = q.alloc<float>((size_t)B * n * 2);
    float* tmp = q.alloc<float>((size_t)B * n * F);
    if (q.err) return;
    RowGroups g = one_group(F);
    rownorm_fwd(q, x, ldx, nullptr, gcp(nullptr, 0), g, gp(tmp, F), nullptr, part, (long)B * n, 0, relu ? 1 : 2);
    bn_apply_fwd(q, tmp, F, part, stats, g, gp(y, ldy), B, n, relu);
}

void bn_bwd_seq(Seq& q, const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                float* dx, int lddx, int B, int n, int F, int relu) {
    float* part = q.alloc<float>((size_t)B * n * 2);
    if (q.err) return;
    RowGroups g = one_group(F);
    bn_bwd_partials(q, gcp(dy, lddy), gcp(y, ldy), g, part, (long)B * n);
    // "y" operand of rownorm_bwd is only used for the ReLU mask: the forward input x
    rownorm_bwd(q, gcp(dy, lddy), gcp(y, ldy), gcp(relu ? x : y, relu ? ldx : ldy), nullptr, stats, part, g, dx, lddx,
                nullptr, B, n, relu, 1, 0);
}

void assign_fwd_seq(Seq& q, const float* z, int ldz, const float* Wp, const float* bp, const int* num_nodes, float* S,
                    int B, int n, int Din, int K) {
    float* logits = q.alloc<float>((size_t)B * n * K);
    if (q.err) return;
    bgemm(q, z, Wp, logits, bp, B, n, K, Din, ldz, Din, K, (long)n * ldz, 0, (long)n * K, false, true, 1.f, 0.f, 0);
    softmax_mask_fwd(q, logits, K, S, K, num_nodes, B, n, K);
}

void assign_bwd_seq(Seq& q, const float* z, int ldz, const float* Wp, const float* S, const float* dS,
                    const int* num_nodes, float* dz, int lddz, float* dWp, float* dbp, int B, int n, int Din, int K) {
    float* dlog = q.alloc<float>((size_t)B * n * K);
    if (q.err) return;
    softmax_mask_bwd(q, S, K, dS, K, num_nodes, dlog, K, B, n, K);
    bgemm(q, dlog, z, dWp, nullptr, 1, K, Din, B * n, K, ldz, Din, 0, 0, 0, true, false, 1.f, 0.f, 0);
    if (dbp) colsum_batched(q, dlog, K, 0, B * n, K, dbp, 0, 1);
    if (dz)
        bgemm(q, dlog, Wp, dz, nullptr, B, n, Din, K, K, Din, lddz, (long)n * K, 0, (long)n * lddz, false, false, 1.f,
              0.f, 0);
}

void pool_fwd_seq(Seq& q, const float* S, const float* Z, int ldz, const float* adj, float* Xp, float* Ap, float* T,
                  int B, int n, int K, int D) {
    bgemm(q, S, Z, Xp, nullptr, B, K, D, n, K, ldz, D, (long)n * K, (long)n * ldz, (long)K * D, true, false, 1.f, 0.f,
          0);
    bgemm(q, S, adj, T, nullptr, B, K, n, n, K, n, n, (long)n * K, (long)n * n, (long)K * n, true, false, 1.f, 0.f, 0);
    bgemm(q, T, S, Ap, nullptr, B, K, K, n, n, K, K, (long)K * n, (long)n * K, (long)K * K, false, false, 1.f, 0.f, 0);
}

void pool_bwd_seq(Seq& q, const float* S, const float* Z, int ldz, const float* adj, const float* T, const float* dXp,
                  const float* dAp, float* dS, float* dZ, int lddz, float* dadj, int B, int n, int K, int D) {
    float* V = q.alloc<float>((size_t)B * n * K);
    if (q.err) return;
    bgemm(q, S, dXp, dZ, nullptr, B, n, D, K, K, D, lddz, (long)n * K, (long)K * D, (long)n * lddz, false, false, 1.f,
          1.f, 0);
    bgemm(q, Z, dXp, dS, nullptr, B, n, K, D, ldz, D, K, (long)n * ldz, (long)K * D, (long)n * K, false, true, 1.f, 0.f,
          0);
    bgemm(q, T, dAp, dS, nullptr, B, n, K, K, n, K, K, (long)K * n, (long)K * K, (long)n * K, true, false, 1.f, 1.f, 0);
    bgemm(q, S, dAp, V, nullptr, B, n, K, K, K, K, K, (long)n * K, (long)K * K, (long)n * K, false, true, 1.f, 0.f, 0);
    bgemm(q, adj, V, dS, nullptr, B, n, K, n, n, K, K, (long)n * n, (long)n * K, (long)n * K, false, false, 1.f, 1.f, 0);
    if (dadj) {
        bgemm(q, S, dAp, V, nullptr, B, n, K, K, K, K, K, (long)n * K, (long)K * K, (long)n * K, false, false, 1.f, 0.f,
              0);
        bgemm(q, V, S, dadj, nullptr, B, n, n, K, K, K, n, (long)n * K, (long)n * K, (long)n * n, false, true, 1.f, 1.f,
              0);
    }
}

// pk != null: the link loss reads the packed adjacency (bf16 rows of A in pk, of A^T in pkt) instead of adj, with the
// same workspace carve-up, so the sizing below covers both
void loss_fwd_seq(Seq& q, const float* ypred, const long long* label, const float* S, const float* adj,
                  const int* num_nodes, const float* norm, float* loss_out, float* prob, float* dunit, int B, int C,
                  int N, int K, int linkpred, const unsigned short* pk = nullptr);
void loss_bwd_seq(Seq& q, const float* prob, const long long* label, const float* S, const float* adj,
                  const int* num_nodes, const float* norm, const float* dloss, float* d_ypred, float* dS, int B, int C,
                  int N, int K, int linkpred, const unsigned short* pk = nullptr, const unsigned short* pkt = nullptr) {
    if (d_ypred) ce_bwd(q, prob, label, dloss, 1.f, d_ypred, B, C);
    if (linkpred && pk) linkpred_bwd_packed(q, S, K, pk, pkt, num_nodes, dloss, dS, K, B, N, K, 0, norm);
    else if (linkpred) linkpred_bwd(q, S, K, adj, num_nodes, dloss, dS, K, B, N, K, 0, norm);
}

__global__ void k_add2(float* out, const float* a, const float* b) { out[0] = a[0] + b[0]; out[1] = b[0]; }

void loss_fwd_seq(Seq& q, const float* ypred, const long long* label, const float* S, const float* adj,
                  const int* num_nodes, const float* norm, float* loss_out, float* prob, float* dunit, int B, int C,
                  int N, int K, int linkpred, const unsigned short* pk) {
    float* tmp = q.alloc<float>(64);
    if (q.err) return;
    if (!linkpred) {                       // loss_out = (CE, 0): one launch
        ce_fwd(q, ypred, label, loss_out, prob, B, C, loss_out + 1, dunit);
        return;
    }
    ce_fwd(q, ypred, label, tmp, prob, B, C, nullptr, dunit);
    if (linkpred) {
        if (pk) linkpred_fwd_packed(q, S, K, pk, num_nodes, tmp + 1, B, N, K, norm);
        else linkpred_fwd(q, S, K, adj, num_nodes, tmp + 1, B, N, K, norm);
        if (q.ok()) {
            hipLaunchKernelGGL(k_add2, dim3(1), dim3(1), 0, q.stream, loss_out, tmp, tmp + 1);
            q.check_launch("loss_add");
        }
    }
}

template <typename F>
size_t sized(F&& f) {
    Seq q = Seq::sizing();
    f(q);
    return q.ws_off + 256;
}
// one workspace serves the forward and the backward: the larger of the two
template <typename F, typename G>
size_t sized(F&& fwd, G&& bwd) {
    const size_t f = sized(fwd), b = sized(bwd);
    return f > b ? f : b;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_version(void) { return DP_VERSION; }
const char* dp_last_error_string(void) { return dp::last_error(); }
int dp_device_error(int clear) { return device_error_take(clear != 0); }
const char* dp_device_error_describe(int mask) { return device_error_text(mask); }
int dp_level0_bwd_symmetric(int* verdicts, int capacity, int* count, int* rows_per_block) {
    DP_NOTNULL(count);
    DP_CHECK_ARG(capacity >= 0 && (capacity == 0 || verdicts != nullptr), "verdicts is NULL with capacity=%d", capacity);
    return level0_verdicts_read(verdicts, capacity, count, rows_per_block);
}
#define DEVICE_GATE(name) DP_TRY(device_error_gate(name))

int dp_bgemm_f32(const float* A, const float* B, float* C, const float* bias, int batch, int M, int N, int K,
                 int lda, int ldb, int ldc, long strideA, long strideB, long strideC, int transA, int transB,
                 float alpha, float beta, int act, void* stream) {
    DP_NOTNULL(A); DP_NOTNULL(B); DP_NOTNULL(C);
    DP_POS(batch); DP_POS(M); DP_POS(N);
    DP_CHECK_ARG(K >= 0, "K=%d must be >= 0", K);
    DP_CHECK_ARG(lda >= (transA ? M : K), "lda=%d too small", lda);
    DP_CHECK_ARG(ldb >= (transB ? K : N), "ldb=%d too small", ldb);
    DP_CHECK_ARG(ldc >= N, "ldc=%d < N=%d", ldc, N);
    Seq q(DP_STREAM(stream), nullptr, 0);
    bgemm(q, A, B, C, bias, batch, M, N, K, lda, ldb, ldc, strideA, strideB, strideC, transA != 0, transB != 0, alpha,
          beta, act);
    return q.err;
}

// ---- groups of contractions (dp_bgemm_plan / dp_bgemm_group_f32): dp_gemm_problem -> GemmDesc the way dp_model.hip
// fills it for each split-K form.  split_out, the row-partial hook, Seq::pred and Seq::fold_zero_p stay unset here.
static_assert(DP_GEMM_GROUP_MAX == GEMM_GROUP_MAX, "diffpool_hip.h and dp_common.h disagree on the group size");
size_t dp_sizeof_gemm_problem(void) { return sizeof(dp_gemm_problem); }
namespace {
bool gemm_tickets(const dp_gemm_problem& p, int ksplit) { return p.split == DP_GEMM_TICKETS && ksplit > 1; }
GemmDesc gemm_desc_of(const dp_gemm_problem& p, float* fix_part, int* fix_cnt) {
    GemmDesc d{p.A, p.B, p.C, p.bias, p.M, p.N, p.K, p.lda, p.ldb, p.ldc, (long)p.sA, (long)p.sB, (long)p.sC,
               p.tA != 0, p.tB != 0, p.alpha, p.beta, p.act, 0, 0, nullptr, 0, 0, 0};
    d.nosplit = p.split == DP_GEMM_WHOLE_K ? 1 : 0;
    d.atomic = p.split == DP_GEMM_ATOMIC ? 1 : 0;
    d.sK = p.split == DP_GEMM_SLABS ? (long)p.sK : 0;
    d.fix_part = fix_part;
    d.fix_cnt = fix_cnt;
    return d;
}
int gemm_group_check(const dp_gemm_problem* p, int count, int batch, int ksplit, bool pointers) {
    DP_NOTNULL(p);
    DP_CHECK_ARG(count >= 1 && count <= GEMM_GROUP_MAX, "count=%d out of range [1,%d]", count, GEMM_GROUP_MAX);
    DP_CHECK_ARG(batch >= 1 && batch <= 65535, "batch=%d out of range [1,65535]", batch);
    DP_CHECK_ARG(ksplit >= 1 && ksplit <= DP_GEMM_MAX_KSPLIT, "ksplit=%d out of range [1,%d]", ksplit,
                 DP_GEMM_MAX_KSPLIT);
    for (int i = 0; i < count; ++i) {
        const dp_gemm_problem& s = p[i];
        DP_CHECK_ARG(s.M >= 0 && s.N >= 0 && s.K >= 0, "problem %d: M=%d N=%d K=%d must not be negative", i, s.M, s.N, s.K);
        DP_CHECK_ARG(s.split >= DP_GEMM_WHOLE_K && s.split <= DP_GEMM_TICKETS, "problem %d: split=%d", i, s.split);
        DP_CHECK_ARG(s.act == 0 || s.act == 1, "problem %d: act=%d (0 none, 1 relu)", i, s.act);
        if (!pointers) continue;
        DP_CHECK_ARG(s.lda >= (s.tA ? s.M : s.K), "problem %d: lda=%d too small", i, s.lda);
        DP_CHECK_ARG(s.ldb >= (s.tB ? s.K : s.N), "problem %d: ldb=%d too small", i, s.ldb);
        DP_CHECK_ARG(s.ldc >= s.N, "problem %d: ldc=%d < N=%d", i, s.ldc, s.N);
        if (s.split == DP_GEMM_ATOMIC)
            DP_CHECK_ARG(!s.bias && !s.act && s.beta == 0.f,
                         "problem %d: atomic split-K accumulates into C and takes no bias, act or beta", i);
        if (s.split == DP_GEMM_SLABS) {
            DP_CHECK_ARG(!s.bias && !s.act, "problem %d: slab split-K takes no bias or act (the slabs are partial sums)", i);
            DP_CHECK_ARG(s.sK > 0, "problem %d: slab split-K needs sK > 0, the distance between two slabs", i);
        }
        if (s.M > 0 && s.N > 0) DP_CHECK_ARG(s.A && s.B && s.C, "problem %d: A, B or C is NULL", i);
    }
    return DP_OK;
}
// carves the partials and the tickets of the ticket problems out of q's workspace and launches (or only sizes: q.dry)
void gemm_group_seq(Seq& q, const dp_gemm_problem* p, int count, int batch, int ksplit) {
    GemmDesc d[GEMM_GROUP_MAX];
    size_t cnt_ints = 0;
    for (int i = 0; i < count; ++i)
        if (gemm_tickets(p[i], ksplit)) cnt_ints += gemm_fix_counters(batch, p[i].M, p[i].N);
    int* cnt = cnt_ints ? q.alloc<int>(cnt_ints) : nullptr;
    size_t off = 0;
    for (int i = 0; i < count; ++i) {
        float* part = nullptr;
        int* c = nullptr;
        if (gemm_tickets(p[i], ksplit) && p[i].M > 0 && p[i].N > 0) {
            part = q.alloc<float>((size_t)batch * ksplit * p[i].M * p[i].N);
            c = cnt + off;
            off += gemm_fix_counters(batch, p[i].M, p[i].N);
        }
        d[i] = gemm_desc_of(p[i], part, c);
    }
    if (q.err) return;
    if (cnt_ints) zero_fill(q, cnt, cnt_ints * sizeof(int));
    bgemm_group(q, d, count, batch, ksplit);
}
}  // namespace

int dp_bgemm_plan(const dp_gemm_problem* p, int count, int batch, int ksplit, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_TRY(gemm_group_check(p, count, batch, ksplit, false));
    GemmDesc d[GEMM_GROUP_MAX];
    float* const some = reinterpret_cast<float*>(sizeof(float));      // "has partials": never dereferenced
    for (int i = 0; i < count; ++i)
        d[i] = gemm_desc_of(p[i], gemm_tickets(p[i], ksplit) ? some : nullptr, nullptr);
    return bgemm_plan(d, count, batch, ksplit, plan_out);
}

size_t dp_bgemm_group_workspace_bytes(const dp_gemm_problem* p, int count, int batch, int ksplit) {
    if (gemm_group_check(p, count, batch, ksplit, false) != DP_OK) return 0;
    Seq q = Seq::sizing();
    gemm_group_seq(q, p, count, batch, ksplit);
    return q.ws_off;
}

int dp_bgemm_group_f32(const dp_gemm_problem* p, int count, int batch, int ksplit, void* workspace,
                       size_t workspace_bytes, void* stream) {
    DP_TRY(gemm_group_check(p, count, batch, ksplit, true));
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    gemm_group_seq(q, p, count, batch, ksplit);
    return q.err;
}

int dp_adj_aggregate(const float* adj, const float* V, int ldv, float* U, int ldu, int B, int n, int C, int trans,
                     float beta, void* stream) {
    DP_NOTNULL(adj); DP_NOTNULL(V); DP_NOTNULL(U);
    DP_POS(B); DP_POS(n); DP_POS(C);
    DP_CHECK_ARG(ldv >= C && ldu >= C, "ldv=%d/ldu=%d smaller than C=%d", ldv, ldu, C);
    Seq q(DP_STREAM(stream), nullptr, 0);
    aggregate(q, adj, V, ldv, U, ldu, B, n, C, trans != 0, beta);
    return q.err;
}

int dp_adj_pack_ld(int n) { return adj_pack_ld(n); }
size_t dp_adj_pack_bytes(int B, int n) { return (size_t)B * n * adj_pack_ld(n) * sizeof(unsigned short); }
// zeroing: dp_adj_pack_zero, whose zero_p is required; the plain name passes NULL and 0
static int adj_pack_entry(const float* adj, void* packed, void* packed_t, int* flag, int B, int n, bool zeroing,
                          void* zero_p, size_t zero_bytes, void* stream) {
    DP_NOTNULL(adj); DP_NOTNULL(packed); DP_NOTNULL(packed_t); DP_NOTNULL(flag);
    if (zeroing) DP_NOTNULL(zero_p);
    DP_POS(B); DP_POS(n);
    Seq q(DP_STREAM(stream), nullptr, 0);
    adj_pack(q, adj, (unsigned short*)packed, (unsigned short*)packed_t, flag, B, n, adj_pack_ld(n), false, zero_p,
             zero_bytes);
    return q.err;
}
int dp_adj_pack(const float* adj, void* packed, void* packed_t, int* flag, int B, int n, void* stream) {
    return adj_pack_entry(adj, packed, packed_t, flag, B, n, false, nullptr, 0, stream);
}
int dp_adj_pack_zero(const float* adj, void* packed, void* packed_t, int* flag, int B, int n, void* zero_p,
                     size_t zero_bytes, void* stream) {
    return adj_pack_entry(adj, packed, packed_t, flag, B, n, true, zero_p, zero_bytes, stream);
}
size_t dp_adj_aggregate_packed_workspace_bytes(int B, int n, int C) {
    return split3_elems(B, n, C) * sizeof(unsigned short) + 512;
}
int dp_adj_aggregate_packed(const float* adj, const void* packed, const void* packed_t, const int* flag,
                            const float* V, int ldv, float* U, int ldu, int B, int n, int C, int trans, float beta,
                            int presplit, void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(adj); DP_NOTNULL(packed); DP_NOTNULL(packed_t); DP_NOTNULL(flag); DP_NOTNULL(V); DP_NOTNULL(U);
    DP_POS(B); DP_POS(n); DP_POS(C);
    DP_CHECK_ARG(ldv >= C && ldu >= C, "ldv=%d/ldu=%d smaller than C=%d", ldv, ldu, C);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    unsigned short* vs = q.alloc<unsigned short>(split3_elems(B, n, C));
    if (q.err) return q.err;
    PackedAdj pk{(const unsigned short*)packed, (const unsigned short*)packed_t, adj_pack_ld(n), flag};
    aggregate(q, adj, V, ldv, U, ldu, B, n, C, trans != 0, beta, &pk, vs, presplit != 0);
    return q.err;
}

int dp_adj_aggregate_plan(int B, int n, int C, int trans, int packed, int fused, int a_misalign, float beta,
                          int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_POS(B); DP_POS(n); DP_POS(C);
    DP_CHECK_ARG(a_misalign >= 0 && a_misalign <= 15, "a_misalign=%d is not the low four bits of an address", a_misalign);
    const AggPick p = agg_pick(B, n, C, trans != 0, packed != 0, fused != 0, (unsigned)a_misalign, beta);
    const int out[DP_AGG_PLAN_INTS] = {p.form, p.ct, p.rt, p.tiles, p.grid, (int)p.lds, p.fallback, p.fb_ct, p.fb_rt,
                                       p.fb_tiles, p.fb_grid, (int)p.fb_lds, p.packed ? 1 : 0, p.declines ? 1 : 0};
    for (int i = 0; i < DP_AGG_PLAN_INTS; ++i) plan_out[i] = out[i];
    return DP_OK;
}

size_t dp_gcn_layer_workspace_bytes(int B, int n, int Fin, int Fout) {
    return sized([&](Seq& q) { gcn_layer_fwd_seq(q, 0, Fin, 0, 0, 0, 0, Fout, 0, B, n, Fin, Fout, 0); }, [&](Seq& q) {
        gcn_layer_bwd_seq(q, 0, Fin, 0, 0, 0, Fout, 0, 0, Fout, 0, Fin, 0, 0, (float*)1, B, n, Fin, Fout, 0);
    });
}
int dp_gcn_layer_fwd(const float* x, int ldx, const float* adj, const float* W, const float* bias, float* y, int ldy,
                     float* invnorm, int B, int n, int Fin, int Fout, int flags, void* workspace,
                     size_t workspace_bytes, void* stream) {
    DP_NOTNULL(x); DP_NOTNULL(adj); DP_NOTNULL(W); DP_NOTNULL(y);
    DP_POS(B); DP_POS(n); DP_POS(Fin); DP_POS(Fout);
    DP_CHECK_ARG(ldx >= Fin && ldy >= Fout, "ldx=%d/ldy=%d smaller than the row width", ldx, ldy);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    gcn_layer_fwd_seq(q, x, ldx, adj, W, bias, y, ldy, invnorm, B, n, Fin, Fout, flags);
    return q.err;
}
int dp_gcn_layer_bwd(const float* x, int ldx, const float* adj, const float* W, const float* y, int ldy,
                     const float* invnorm, const float* dy, int lddy, float* dx, int lddx, float* dW, float* db,
                     float* dadj, int B, int n, int Fin, int Fout, int flags, void* workspace, size_t workspace_bytes,
                     void* stream) {
    DP_NOTNULL(x); DP_NOTNULL(adj); DP_NOTNULL(W); DP_NOTNULL(y); DP_NOTNULL(dy); DP_NOTNULL(dW);
    DP_POS(B); DP_POS(n); DP_POS(Fin); DP_POS(Fout);
    DP_CHECK_ARG(!(flags & DP_F_NORMALIZE) || invnorm, "invnorm is NULL but DP_F_NORMALIZE is set");
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    gcn_layer_bwd_seq(q, x, ldx, adj, W, y, ldy, invnorm, dy, lddy, dx, lddx, dW, db, dadj, B, n, Fin, Fout, flags);
    return q.err;
}

size_t dp_bn_node_workspace_bytes(int B, int n, int F) {
    return sized([&](Seq& q) { bn_fwd_seq(q, 0, F, 0, F, 0, B, n, F, 1); },
                 [&](Seq& q) { bn_bwd_seq(q, 0, F, 0, F, 0, 0, F, 0, F, B, n, F, 1); });
}
int dp_bn_node_fwd(const float* x, int ldx, float* y, int ldy, float* stats, int B, int n, int F, int relu,
                   void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(x); DP_NOTNULL(y); DP_NOTNULL(stats);
    DP_POS(B); DP_POS(n); DP_POS(F);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    bn_fwd_seq(q, x, ldx, y, ldy, stats, B, n, F, relu);
    return q.err;
}
int dp_bn_node_bwd(const float* x, int ldx, const float* y, int ldy, const float* stats, const float* dy, int lddy,
                   float* dx, int lddx, int B, int n, int F, int relu, void* workspace, size_t workspace_bytes,
                   void* stream) {
    DP_NOTNULL(y); DP_NOTNULL(stats); DP_NOTNULL(dy); DP_NOTNULL(dx);
    DP_CHECK_ARG(!relu || x, "x is NULL but relu != 0");
    DP_POS(B); DP_POS(n); DP_POS(F);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    bn_bwd_seq(q, x, ldx, y, ldy, stats, dy, lddy, dx, lddx, B, n, F, relu);
    return q.err;
}

size_t dp_assign_workspace_bytes(int B, int n, int Din, int K) {
    return sized([&](Seq& q) { assign_fwd_seq(q, 0, Din, 0, 0, 0, 0, B, n, Din, K); });
}
int dp_assign_softmax_mask_fwd(const float* z, int ldz, const float* Wp, const float* bp, const int* num_nodes,
                               float* S, int B, int n, int Din, int K, void* workspace, size_t workspace_bytes,
                               void* stream) {
    DP_NOTNULL(z); DP_NOTNULL(Wp); DP_NOTNULL(S);
    DP_POS(B); DP_POS(n); DP_POS(Din); DP_POS(K);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    assign_fwd_seq(q, z, ldz, Wp, bp, num_nodes, S, B, n, Din, K);
    return q.err;
}
int dp_assign_softmax_mask_bwd(const float* z, int ldz, const float* Wp, const float* S, const float* dS,
                               const int* num_nodes, float* dz, int lddz, float* dWp, float* dbp, int B, int n, int Din,
                               int K, void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(z); DP_NOTNULL(Wp); DP_NOTNULL(S); DP_NOTNULL(dS); DP_NOTNULL(dWp);
    DP_POS(B); DP_POS(n); DP_POS(Din); DP_POS(K);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    assign_bwd_seq(q, z, ldz, Wp, S, dS, num_nodes, dz, lddz, dWp, dbp, B, n, Din, K);
    return q.err;
}

int dp_pool_fwd(const float* S, const float* Z, int ldz, const float* adj, float* Xp, float* Ap, float* T, int B, int n,
                int K, int D, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(Z); DP_NOTNULL(adj); DP_NOTNULL(Xp); DP_NOTNULL(Ap); DP_NOTNULL(T);
    DP_POS(B); DP_POS(n); DP_POS(K); DP_POS(D);
    Seq q(DP_STREAM(stream), nullptr, 0);
    pool_fwd_seq(q, S, Z, ldz, adj, Xp, Ap, T, B, n, K, D);
    return q.err;
}
size_t dp_pool_bwd_workspace_bytes(int B, int n, int K, int D) {
    return sized([&](Seq& q) { pool_bwd_seq(q, 0, 0, D, 0, 0, 0, 0, 0, 0, D, 0, B, n, K, D); });
}
int dp_pool_bwd(const float* S, const float* Z, int ldz, const float* adj, const float* T, const float* dXp,
                const float* dAp, float* dS, float* dZ, int lddz, float* dadj, int B, int n, int K, int D,
                void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(Z); DP_NOTNULL(adj); DP_NOTNULL(T); DP_NOTNULL(dXp); DP_NOTNULL(dAp); DP_NOTNULL(dS);
    DP_NOTNULL(dZ);
    DP_POS(B); DP_POS(n); DP_POS(K); DP_POS(D);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    pool_bwd_seq(q, S, Z, ldz, adj, T, dXp, dAp, dS, dZ, lddz, dadj, B, n, K, D);
    return q.err;
}

int dp_masked_max_fwd(const float* Z, int ldz, const int* num_nodes, float* out, int ldo, int* argmax, int B, int n,
                      int F, void* stream) {
    DP_NOTNULL(Z); DP_NOTNULL(out); DP_NOTNULL(argmax);
    DP_POS(B); DP_POS(n); DP_POS(F);
    Seq q(DP_STREAM(stream), nullptr, 0);
    masked_max_fwd(q, Z, ldz, num_nodes, out, ldo, argmax, F, B, n, F);
    return q.err;
}
int dp_masked_max_bwd(const float* dout, int ldo, const int* argmax, float* dZ, int lddz, int B, int n, int F,
                      void* stream) {
    DP_NOTNULL(dout); DP_NOTNULL(argmax); DP_NOTNULL(dZ);
    DP_POS(B); DP_POS(n); DP_POS(F);
    Seq q(DP_STREAM(stream), nullptr, 0);
    masked_max_bwd(q, dout, ldo, argmax, F, dZ, lddz, B, n, F);
    return q.err;
}

// ---- the row launchers as the encoder plans call them (dp_rowop_plan and the pass-through entries of diffpool_hip.h)
size_t dp_sizeof_row_groups(void) { return sizeof(dp_row_groups); }
size_t dp_sizeof_group_ptrs(void) { return sizeof(dp_group_ptrs); }
namespace {
int row_groups_check(const dp_row_groups* g) {
    DP_NOTNULL(g);
    DP_CHECK_ARG(g->G >= 1 && g->G <= 2, "G=%d out of range [1,2]", g->G);
    for (int i = 0; i < g->G; ++i) {
        DP_CHECK_ARG(g->w[i] >= 1, "group %d: width w=%d must be >= 1", i, g->w[i]);
        DP_CHECK_ARG(g->c0[i] >= 0, "group %d: c0=%d must not be negative", i, g->c0[i]);
    }
    if (g->G == 2)
        DP_CHECK_ARG(g->c0[1] >= g->c0[0] + g->w[0], "groups overlap: group 1 starts at column %d, group 0 ends at %d",
                     g->c0[1], g->c0[0] + g->w[0]);
    return DP_OK;
}
RowGroups row_groups_of(const dp_row_groups& g) {
    RowGroups r{};
    r.G = g.G;
    for (int i = 0; i < g.G; ++i) {
        r.c0[i] = g.c0[i];
        r.w[i] = g.w[i];
    }
    return r;
}
// need: every group's pointer must be there; otherwise a group may go without (bias, dbias)
int group_ptrs_check(const dp_row_groups& g, const dp_group_ptrs* p, const char* name, bool need) {
    DP_CHECK_ARG(p != nullptr, "%s is NULL", name);
    for (int i = 0; i < g.G; ++i) {
        DP_CHECK_ARG(!need || p->p[i], "%s: the pointer of group %d is NULL", name, i);
        DP_CHECK_ARG(!need || p->ld[i] >= g.w[i], "%s: ld=%d of group %d smaller than its width %d", name, p->ld[i], i,
                     g.w[i]);
    }
    return DP_OK;
}
GroupPtrs gptrs(const dp_row_groups& g, const dp_group_ptrs* p) {
    GroupPtrs r{};
    for (int i = 0; p && i < g.G; ++i) {
        r.p[i] = (float*)p->p[i];
        r.ld[i] = p->ld[i];
    }
    return r;
}
GroupCPtrs gcptrs(const dp_row_groups& g, const dp_group_ptrs* p) {
    GroupCPtrs r{};
    for (int i = 0; p && i < g.G; ++i) {
        r.p[i] = (const float*)p->p[i];
        r.ld[i] = p->ld[i];
    }
    return r;
}
int joint_width(const dp_row_groups& g) { return g.c0[g.G - 1] + g.w[g.G - 1]; }
}  // namespace
#define ROWS_OK(g) DP_TRY(row_groups_check(g))
#define GROUP_PTRS(g, p, need) DP_TRY(group_ptrs_check(*(g), p, #p, need))

int dp_rowop_plan(int op, const dp_row_groups* g, int n, int B, int Bs, int flags, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_CHECK_ARG(op >= DP_ROWOP_ROWNORM_FWD && op <= DP_ROWOP_MASKED_MAX_FWD, "op=%d is no row operation", op);
    RowPick p{};
    if (op == DP_ROWOP_MASKED_MAX_FWD) {
        DP_POS(n);
        p = masked_max_fwd_pick(n);
    } else {
        ROWS_OK(g);
        if (Bs <= 0) Bs = B;
        const RowGroups r = row_groups_of(*g);
        const bool zero = (flags & DP_ROWF_ZERO) != 0;
        switch (op) {
            case DP_ROWOP_ROWNORM_FWD: p = rownorm_fwd_pick(r); break;
            case DP_ROWOP_ROWNORM_BWD: p = rownorm_bwd_pick(r, (flags & DP_ROWF_STATS) != 0, Bs); break;
            case DP_ROWOP_BN_APPLY_FWD: p = bn_apply_fwd_pick(r, (flags & DP_ROWF_STATS) != 0, Bs); break;
            case DP_ROWOP_SOFTMAX_FWD:
                p = softmax_mask_fwd_pick(r.w[0], (flags & DP_ROWF_VS) != 0, zero, !(flags & DP_ROWF_ZERO_UNALIGNED));
                break;
            default: p = softmax_mask_bwd_pick(r.w[0], (flags & DP_ROWF_DBIAS) != 0); break;
        }
    }
    const int out[DP_ROWOP_PLAN_INTS] = {p.kernel, p.nk, p.quad, p.finalize, p.generic() ? 1 : 0, p.zero};
    for (int i = 0; i < DP_ROWOP_PLAN_INTS; ++i) plan_out[i] = out[i];
    return DP_OK;
}

int dp_rownorm_fwd(const float* U, int ldu, const float* P, const dp_row_groups* g, const dp_group_ptrs* bias,
                   const dp_group_ptrs* yout, float* invn, float* part, long rows, int normalize, int stats_mode,
                   void* stream) {
    ROWS_OK(g);
    DP_NOTNULL(U);
    GROUP_PTRS(g, yout, true);
    if (bias) GROUP_PTRS(g, bias, false);
    DP_POS(rows);
    DP_CHECK_ARG(ldu >= joint_width(*g), "ldu=%d smaller than the joint width %d", ldu, joint_width(*g));
    DP_CHECK_ARG(stats_mode >= 0 && stats_mode <= 2, "stats_mode=%d (0 none, 1 of relu(y), 2 of y)", stats_mode);
    DP_CHECK_ARG(!stats_mode || part, "part is NULL but stats_mode=%d", stats_mode);
    Seq q(DP_STREAM(stream), nullptr, 0);
    rownorm_fwd(q, U, ldu, P, gcptrs(*g, bias), row_groups_of(*g), gptrs(*g, yout), invn, part, rows, normalize != 0,
                stats_mode);
    return q.err;
}

int dp_adj_aggregate_rownorm(const float* adj, const void* packed, const void* packed_t, const int* flag, const float* V,
                             int ldv, const float* P, const dp_row_groups* g, const dp_group_ptrs* bias,
                             const dp_group_ptrs* yout, float* invn, float* part, int B, int n, int normalize,
                             int stats_mode, int presplit, void* workspace, size_t workspace_bytes, void* stream) {
    ROWS_OK(g);
    DP_NOTNULL(adj); DP_NOTNULL(V);
    GROUP_PTRS(g, yout, true);
    if (bias) GROUP_PTRS(g, bias, false);
    DP_POS(B); DP_POS(n);
    const int Cj = joint_width(*g);
    // (the tail kernels take the groups as one run of columns: the wide forms norm every column below c0[1] with group
    // 0)
    DP_CHECK_ARG(g->c0[0] == 0 && (g->G == 1 || g->c0[1] == g->w[0]),
                 "the groups must cover the joint width without a gap (c0 = %d, %d; w[0] = %d)", g->c0[0],
                 g->G == 2 ? g->c0[1] : 0, g->w[0]);
    DP_CHECK_ARG(ldv >= Cj, "ldv=%d smaller than the joint width %d", ldv, Cj);
    DP_CHECK_ARG(stats_mode >= 0 && stats_mode <= 2, "stats_mode=%d (0 none, 1 of relu(y), 2 of y)", stats_mode);
    DP_CHECK_ARG(!stats_mode || part, "part is NULL but stats_mode=%d", stats_mode);
    const bool any = packed || packed_t || flag || workspace;
    DP_CHECK_ARG(!any || (packed && packed_t && flag && workspace),
                 "packed, packed_t, flag and workspace are given together or not at all");
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    PackedAdj pk{(const unsigned short*)packed, (const unsigned short*)packed_t, adj_pack_ld(n), flag};
    unsigned short* vs = nullptr;
    if (any) {
        vs = q.alloc<unsigned short>(split3_elems(B, n, Cj));
        if (q.err) return q.err;
    }
    if (!aggregate_rownorm_fwd(q, adj, V, ldv, P, gcptrs(*g, bias), row_groups_of(*g), gptrs(*g, yout), invn, part, B, n,
                               normalize != 0, stats_mode, any ? &pk : nullptr, vs, presplit != 0))
        return DP_AGG_DECLINED;
    return q.err;
}

int dp_bn_apply_fwd(const float* Y, int ldy, const float* part, float* stats, const dp_row_groups* g,
                    const dp_group_ptrs* xout, int B, int n, int relu, int Bs, void* stream) {
    ROWS_OK(g);
    DP_NOTNULL(Y);
    GROUP_PTRS(g, xout, true);
    DP_POS(B); DP_POS(n);
    DP_CHECK_ARG(Bs >= 0, "Bs=%d must not be negative (0: B)", Bs);
    DP_CHECK_ARG(ldy >= joint_width(*g), "ldy=%d smaller than the joint width %d", ldy, joint_width(*g));
    DP_CHECK_ARG(!part || stats, "stats is NULL but part is given");
    Seq q(DP_STREAM(stream), nullptr, 0);
    bn_apply_fwd(q, Y, ldy, part, stats, row_groups_of(*g), gptrs(*g, xout), B, n, relu != 0, Bs);
    return q.err;
}

int dp_bn_bwd_partials(const dp_row_groups* g, const dp_group_ptrs* dx, const dp_group_ptrs* xhat, float* part,
                       long rows, void* stream) {
    ROWS_OK(g);
    GROUP_PTRS(g, dx, true);
    GROUP_PTRS(g, xhat, true);
    DP_NOTNULL(part);
    DP_POS(rows);
    Seq q(DP_STREAM(stream), nullptr, 0);
    bn_bwd_partials(q, gcptrs(*g, dx), gcptrs(*g, xhat), row_groups_of(*g), part, rows);
    return q.err;
}

int dp_rownorm_bwd(const dp_row_groups* g, const dp_group_ptrs* dx, const dp_group_ptrs* xhat, const dp_group_ptrs* y,
                   const float* invn, const float* stats, float* part2, float* dU, int ldu, const dp_group_ptrs* dbias,
                   int B, int n, int has_relu, int has_bn, int normalize, void* vs, int Bs, void* stream) {
    ROWS_OK(g);
    GROUP_PTRS(g, dx, true);
    GROUP_PTRS(g, y, true);
    if (has_bn) GROUP_PTRS(g, xhat, true);
    if (dbias) GROUP_PTRS(g, dbias, false);
    DP_NOTNULL(dU);
    DP_POS(B); DP_POS(n);
    DP_CHECK_ARG(Bs >= 0, "Bs=%d must not be negative (0: B)", Bs);
    DP_CHECK_ARG(B <= 65535, "B=%d exceeds the grid's second dimension (65535)", B);
    DP_CHECK_ARG(ldu >= joint_width(*g), "ldu=%d smaller than the joint width %d", ldu, joint_width(*g));
    DP_CHECK_ARG(!has_bn || (stats && part2), "has_bn is set but stats or part2 is NULL");
    DP_CHECK_ARG(!normalize || invn, "normalize is set but invn is NULL");
    const bool want = dbias && (dbias->p[0] || (g->G == 2 && dbias->p[1]));
    const size_t lds = ((want ? 16 : 0) + (vs ? 8 : 0)) * (size_t)joint_width(*g) * sizeof(float);
    DP_CHECK_ARG(lds <= 64 * 1024, "dbias / vs: the slabs and the split need %zu bytes of LDS at joint width %d, no form has "
                 "more than 64 KiB", lds, joint_width(*g));
    // (a slab's ld is the distance between the graphs' rows)
    for (int i = 0; dbias && i < g->G; ++i)
        DP_CHECK_ARG(!dbias->p[i] || B <= 1 || dbias->ld[i] >= g->w[i],
                     "dbias: ld=%d of group %d, the stride between graphs, smaller than its width %d", dbias->ld[i], i,
                     g->w[i]);
    if (vs) DP_ALIGNED16_P(vs);
    GroupPtrs db = gptrs(*g, dbias);
    Seq q(DP_STREAM(stream), nullptr, 0);
    rownorm_bwd(q, gcptrs(*g, dx), gcptrs(*g, has_bn ? xhat : nullptr), gcptrs(*g, y), invn, stats, part2,
                row_groups_of(*g), dU, ldu, dbias ? &db : nullptr, B, n, has_relu != 0, has_bn != 0, normalize != 0,
                (unsigned short*)vs, Bs);
    return q.err;
}

int dp_softmax_mask_fwd(const float* logits, int ldl, float* S, int lds, const int* num_nodes, int B, int n, int K,
                        float* S2, void* vs, void* zero_p, size_t zero_bytes, void* stream) {
    DP_NOTNULL(logits); DP_NOTNULL(S);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_CHECK_ARG(B <= 65535, "B=%d exceeds the grid's second dimension (65535)", B);
    DP_CHECK_ARG(ldl >= K && lds >= K, "ldl=%d/lds=%d smaller than K=%d", ldl, lds, K);
    DP_CHECK_ARG(!vs || !softmax_mask_fwd_pick(K, true, false, true).generic(),
                 "vs: K=%d is past the plan forms (16 rows of K floats must fit 48 KiB), the generic kernel writes no split",
                 K);
    DP_CHECK_ARG(!zero_bytes || zero_p, "zero_p is NULL but zero_bytes=%zu", zero_bytes);
    if (vs) DP_ALIGNED16_P(vs);
    Seq q(DP_STREAM(stream), nullptr, 0);
    softmax_mask_fwd(q, logits, ldl, S, lds, num_nodes, B, n, K, S2, (unsigned short*)vs, zero_bytes ? zero_p : nullptr,
                     zero_bytes);
    return q.err;
}

int dp_softmax_mask_bwd(const float* S, int lds, float* dS, int ldds, const int* num_nodes, float* dlogits, int ldl,
                        int B, int n, int K, float* dbias, long dbias_stride, const float* dS2, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(dS); DP_NOTNULL(dlogits);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_CHECK_ARG(B <= 65535, "B=%d exceeds the grid's second dimension (65535)", B);
    DP_CHECK_ARG(lds >= K && ldds >= K && ldl >= K, "lds=%d/ldds=%d/ldl=%d smaller than K=%d", lds, ldds, ldl, K);
    DP_CHECK_ARG(!dbias || B == 1 || dbias_stride >= K, "dbias_stride=%ld smaller than K=%d", dbias_stride, K);
    Seq q(DP_STREAM(stream), nullptr, 0);
    softmax_mask_bwd(q, S, lds, dS, ldds, num_nodes, dlogits, ldl, B, n, K, dbias, dbias_stride, dS2);
    return q.err;
}

int dp_colsum_batched(const float* X, int ldx, long strideX, int rows, int cols, float* out, long strideOut, int batch,
                      int rowsplit, void* stream) {
    DP_NOTNULL(X); DP_NOTNULL(out);
    DP_POS(rows); DP_POS(cols); DP_POS(batch);
    DP_CHECK_ARG(ldx >= cols, "ldx=%d smaller than cols=%d", ldx, cols);
    DP_CHECK_ARG(rowsplit >= 1 && rowsplit <= 65535, "rowsplit=%d out of range [1,65535]", rowsplit);
    DP_CHECK_ARG(batch <= 65535, "batch=%d exceeds the grid's second dimension (65535)", batch);
    Seq q(DP_STREAM(stream), nullptr, 0);
    colsum_batched(q, X, ldx, strideX, rows, cols, out, strideOut, batch, rowsplit);
    return q.err;
}

size_t dp_linkpred_workspace_bytes(int B, int n, int K) {
    return sized([&](Seq& q) { linkpred_fwd(q, 0, K, 0, 0, 0, B, n, K); },
                 [&](Seq& q) { linkpred_bwd(q, 0, K, 0, 0, 0, 0, K, B, n, K, 0); });
}
int dp_linkpred_plan(int B, int n, int K, int* plan_out) {
    DP_NOTNULL(plan_out);
    DP_POS(B); DP_POS(n); DP_POS(K);
    LinkPlan p;
    if (!linkpred_plan(B, n, K, p)) {
        set_error("linkpred: K=%d clusters exceed the fused tile kernel (max 256)", K);
        return DP_ERR_UNSUPPORTED;
    }
    const int out[DP_LINKPRED_PLAN_INTS] = {p.kt, p.cw, p.col_tiles, p.splits, p.split_tiles, p.fwd_tiles,
                                            (int)p.fwd_lds, (int)p.bwd_lds};
    for (int i = 0; i < DP_LINKPRED_PLAN_INTS; ++i) plan_out[i] = out[i];
    return DP_OK;
}
int dp_linkpred_loss_fwd(const float* S, const float* adj, const int* num_nodes, float* loss_out, int B, int n, int K,
                         void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(adj); DP_NOTNULL(loss_out);
    DP_POS(B); DP_POS(n); DP_POS(K);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    linkpred_fwd(q, S, K, adj, num_nodes, loss_out, B, n, K);
    return q.err;
}
int dp_linkpred_loss_bwd(const float* S, const float* adj, const int* num_nodes, const float* dloss, float* dS,
                         int accumulate, int B, int n, int K, void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(adj); DP_NOTNULL(dS);
    DP_POS(B); DP_POS(n); DP_POS(K);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    linkpred_bwd(q, S, K, adj, num_nodes, dloss, dS, K, B, n, K, accumulate);
    return q.err;
}
int dp_linkpred_loss_fwd_packed(const float* S, const void* adj_pk, const int* num_nodes, float* loss_out, int B,
                                int n, int K, void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(adj_pk); DP_NOTNULL(loss_out);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_ALIGNED16_P(adj_pk);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    linkpred_fwd_packed(q, S, K, static_cast<const unsigned short*>(adj_pk), num_nodes, loss_out, B, n, K);
    return q.err;
}
int dp_linkpred_loss_bwd_packed(const float* S, const void* adj_pk, const void* adj_pkt, const int* num_nodes,
                                const float* dloss, float* dS, int accumulate, int B, int n, int K, void* workspace,
                                size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(adj_pk); DP_NOTNULL(adj_pkt); DP_NOTNULL(dS);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_ALIGNED16_P(adj_pk); DP_ALIGNED16_P(adj_pkt);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    linkpred_bwd_packed(q, S, K, static_cast<const unsigned short*>(adj_pk),
                        static_cast<const unsigned short*>(adj_pkt), num_nodes, dloss, dS, K, B, n, K, accumulate);
    return q.err;
}

size_t dp_assign_entropy_workspace_bytes(int B, int n, int K) {
    if (B < 1 || n < 1 || K < 1) return 0;
    return sized([&](Seq& q) { assign_entropy_fwd(q, 0, K, 0, 0.f, 0, 0, B, n, K); });
}
int dp_assign_entropy_fwd(const float* S, int lds, const int* num_nodes, float weight, float* ent_out,
                          float* total_inout, int B, int n, int K, void* workspace, size_t workspace_bytes,
                          void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(ent_out);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_CHECK_ARG(lds >= K, "dp_assign_entropy_fwd: lds=%d smaller than K=%d", lds, K);
    DP_NOTNULL(workspace);
    DP_CHECK_ARG(workspace_bytes >= dp_assign_entropy_workspace_bytes(B, n, K),
                 "dp_assign_entropy_fwd: workspace too small: need >= %zu bytes, have %zu",
                 dp_assign_entropy_workspace_bytes(B, n, K), workspace_bytes);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    assign_entropy_fwd(q, S, lds, num_nodes, weight, ent_out, total_inout, B, n, K);
    return q.err;
}
int dp_assign_entropy_bwd(const float* S, int lds, const int* num_nodes, const float* dloss, float weight, float* dS,
                          int ldds, int accumulate, int B, int n, int K, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(dS);
    DP_POS(B); DP_POS(n); DP_POS(K);
    DP_CHECK_ARG(lds >= K, "dp_assign_entropy_bwd: lds=%d smaller than K=%d", lds, K);
    DP_CHECK_ARG(ldds >= K, "dp_assign_entropy_bwd: ldds=%d smaller than K=%d", ldds, K);
    Seq q(DP_STREAM(stream), nullptr, 0);
    assign_entropy_bwd(q, S, lds, num_nodes, dloss, weight, dS, ldds, accumulate, B, n, K);
    return q.err;
}

// ------------------------------------------------------------------ Frobenius link loss
// The checked bodies below serve every exported name of their op; `fn` is that name, for the messages.
#define FROB_K_OK(fn) \
    DP_CHECK(K <= 256, DP_ERR_UNSUPPORTED, "%s: K=%d clusters: the Frobenius link kernels support K <= 256", fn, K)
#define FROB_WS_OK(fn, need)                                                                                      \
    do {                                                                                                          \
        DP_NOTNULL(workspace);                                                                                    \
        DP_CHECK(workspace_bytes >= (need), DP_ERR_INVALID_ARG, "%s: workspace too small: need >= %zu bytes, have %zu", \
                 fn, (need), workspace_bytes);                                                                    \
    } while (0)

size_t dp_frob_link_workspace_bytes(int B, int N, int K) {
    if (B < 1 || N < 1 || K < 1 || K > 256) return 0;
    return frob_link_ws_doubles((long long)B * N, B, K) * sizeof(double) + 3 * 256 + 256;
}
// adj_pk / adj_pkt: the packed planes, or (packed == 0) the fp32 adjacency and NULL
static int frob_link_fwd_dense(const char* fn, const float* S, int lds, const void* adj_pk, const void* adj_pkt,
                               int packed, const int* num_nodes, const float* link_norm, float* W, float* G,
                               float* loss_out, float* total_inout, int B, int N, int K, void* workspace,
                               size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S);
    DP_CHECK(adj_pk != nullptr, DP_ERR_INVALID_ARG, "%s is NULL", packed ? "adj_pk" : "adj");
    if (packed) DP_NOTNULL(adj_pkt);
    DP_NOTNULL(W); DP_NOTNULL(G); DP_NOTNULL(loss_out);
    DP_POS(B); DP_POS(N); DP_POS(K);
    FROB_K_OK(fn);
    DP_CHECK(lds >= K, DP_ERR_INVALID_ARG, "%s: lds=%d smaller than K=%d", fn, lds, K);
    if (packed) {
        DP_ALIGNED16(adj_pk, true, "adj_pk is not 16-byte aligned");
        DP_ALIGNED16(adj_pkt, true, "adj_pkt is not 16-byte aligned");
    }
    FROB_WS_OK(fn, dp_frob_link_workspace_bytes(B, N, K));
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    const int ld = packed ? adj_pack_ld(N) : N;
    frob_link_w_dense(q, S, lds, adj_pk, adj_pkt, packed, ld, num_nodes, W, B, N, K);
    frob_link_fwd(q, S, lds, W, adj_pk, packed ? 3 : 1, ld, num_nodes, nullptr, nullptr, link_norm, 1.f, G, loss_out,
                  total_inout, B, N, (long long)B * N, K);
    return q.err;
}
int dp_frob_link_fwd(const float* S, int lds, const float* adj, const int* num_nodes, const float* link_norm, float* W,
                     float* G, float* loss_out, float* total_inout, int B, int N, int K, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return frob_link_fwd_dense("dp_frob_link_fwd", S, lds, adj, nullptr, 0, num_nodes, link_norm, W, G, loss_out,
                               total_inout, B, N, K, workspace, workspace_bytes, stream);
}
int dp_frob_link_fwd_packed(const float* S, int lds, const void* adj_pk, const void* adj_pkt, const int* num_nodes,
                            const float* link_norm, float* W, float* G, float* loss_out, float* total_inout, int B, int N,
                            int K, void* workspace, size_t workspace_bytes, void* stream) {
    return frob_link_fwd_dense("dp_frob_link_fwd_packed", S, lds, adj_pk, adj_pkt, 1, num_nodes, link_norm, W, G,
                               loss_out, total_inout, B, N, K, workspace, workspace_bytes, stream);
}
int dp_frob_link_bwd(const float* S, int lds, const float* W, const float* G, const int* num_nodes,
                     const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate, int B, int N, int K,
                     void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(W); DP_NOTNULL(G); DP_NOTNULL(dS);
    DP_POS(B); DP_POS(N); DP_POS(K);
    FROB_K_OK("dp_frob_link_bwd");
    DP_CHECK_ARG(lds >= K, "dp_frob_link_bwd: lds=%d smaller than K=%d", lds, K);
    DP_CHECK_ARG(ldds >= K, "dp_frob_link_bwd: ldds=%d smaller than K=%d", ldds, K);
    Seq q(DP_STREAM(stream), nullptr, 0);
    frob_link_bwd(q, S, lds, W, G, num_nodes, nullptr, link_norm, dloss, 1.f, dS, ldds, accumulate, B, N,
                  (long long)B * N, K);
    return q.err;
}
int dp_frob_link_bwd_packed(const float* S, int lds, const float* W, const float* G, const int* num_nodes,
                            const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate, int B,
                            int N, int K, void* stream) {
    return dp_frob_link_bwd(S, lds, W, G, num_nodes, link_norm, dloss, dS, ldds, accumulate, B, N, K, stream);
}

size_t dp_csr_frob_link_workspace_bytes(int n_total, int B, int K) {
    if (n_total < 1 || B < 1 || K < 1 || K > 256) return 0;
    return frob_link_ws_doubles(n_total, B, K) * sizeof(double) + 3 * 256 + 256;
}
// batch: node_off and B are the caller's and n its n_total; else one graph of n rows (node_off NULL, B = 1)
static int csr_frob_link_fwd(const char* fn, bool batch, const float* S, int lds, const int* indptr, const int* indices,
                             const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                             bool weighted, const int* node_off, const float* link_norm, float* W, float* G,
                             float* loss_out, float* total_inout, int B, int n, int K, void* workspace,
                             size_t workspace_bytes, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(indptr); DP_NOTNULL(indices);
    DP_VALUES((void)0, "values is NULL");
    if (batch) DP_NOTNULL(node_off);
    DP_NOTNULL(W); DP_NOTNULL(G); DP_NOTNULL(loss_out);
    if (batch) DP_POS(B);
    DP_CHECK(n > 0, DP_ERR_INVALID_ARG, "%s=%d must be positive", batch ? "n_total" : "n", n);
    DP_POS(K);
    FROB_K_OK(fn);
    if (batch)
        DP_CHECK(B <= n, DP_ERR_INVALID_ARG, "%s: B=%d graphs over n_total=%d rows (every graph has >= 1 node)", fn, B, n);
    DP_CHECK(lds >= K, DP_ERR_INVALID_ARG, "%s: lds=%d smaller than K=%d", fn, lds, K);
    DP_CHECK((indptr_t == nullptr) == (indices_t == nullptr), DP_ERR_INVALID_ARG,
             "%s: indptr_t and indices_t go together (both NULL: undirected)", fn);
    DP_VALUES_T((void)0, "%s: values_t is NULL but indices_t is a CSR of its own", fn);
    FROB_WS_OK(fn, dp_csr_frob_link_workspace_bytes(n, B, K));
    if (!weighted) values = nullptr;
    values_t = weighted ? values_t_of(indices, indices_t, values, values_t) : nullptr;
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    const bool directed = indptr_t && indices_t && !(indptr_t == indptr && indices_t == indices);
    csr_aggregate_fwd(q, S, lds, indptr, indices, W, K, n, K, 0, 0.f, values);                       // W = A S
    if (directed) csr_aggregate_fwd(q, S, lds, indptr_t, indices_t, W, K, n, K, 0, 1.f, values_t);   // += A^T S
    if (values)      // T0 = sum of the stored values' squares, by the row kernel (fp64, fixed order)
        frob_link_fwd(q, S, lds, W, values, 4, 0, nullptr, node_off, nullptr, link_norm, directed ? 1.f : 2.f, G,
                      loss_out, total_inout, B, n, n, K, indptr);
    else
        frob_link_fwd(q, S, lds, W, nullptr, 0, 0, nullptr, node_off, indptr + n, link_norm, directed ? 1.f : 2.f, G,
                      loss_out, total_inout, B, n, n, K);
    return q.err;
}
static int csr_frob_link_bwd(const char* fn, bool batch, const float* S, int lds, const float* W, const float* G,
                             const int* node_off, const float* link_norm, const float* dloss, float* dS, int ldds,
                             int accumulate, int symmetric, int B, int n, int K, void* stream) {
    DP_NOTNULL(S); DP_NOTNULL(W); DP_NOTNULL(G);
    if (batch) DP_NOTNULL(node_off);
    DP_NOTNULL(dS);
    if (batch) DP_POS(B);
    DP_CHECK(n > 0, DP_ERR_INVALID_ARG, "%s=%d must be positive", batch ? "n_total" : "n", n);
    DP_POS(K);
    FROB_K_OK(fn);
    DP_CHECK(lds >= K, DP_ERR_INVALID_ARG, "%s: lds=%d smaller than K=%d", fn, lds, K);
    DP_CHECK(ldds >= K, DP_ERR_INVALID_ARG, "%s: ldds=%d smaller than K=%d", fn, ldds, K);
    Seq q(DP_STREAM(stream), nullptr, 0);
    frob_link_bwd(q, S, lds, W, G, nullptr, node_off, link_norm, dloss, symmetric ? 2.f : 1.f, dS, ldds, accumulate, B, n,
                  n, K);
    return q.err;
}
int dp_csr_frob_link_fwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                         const int* indices_t, const float* link_norm, float* W, float* G, float* loss_out,
                         float* total_inout, int n, int K, void* workspace, size_t workspace_bytes, void* stream) {
    return csr_frob_link_fwd("dp_csr_frob_link_fwd", false, S, lds, indptr, indices, nullptr, indptr_t, indices_t,
                             nullptr, false, nullptr, link_norm, W, G, loss_out, total_inout, 1, n, K, workspace,
                             workspace_bytes, stream);
}
int dp_csr_frob_link_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                           const int* indptr_t, const int* indices_t, const float* values_t, const float* link_norm,
                           float* W, float* G, float* loss_out, float* total_inout, int n, int K, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return csr_frob_link_fwd("dp_csr_frob_link_fwd_w", false, S, lds, indptr, indices, values, indptr_t, indices_t,
                             values_t, true, nullptr, link_norm, W, G, loss_out, total_inout, 1, n, K, workspace,
                             workspace_bytes, stream);
}
int dp_csr_frob_link_bwd(const float* S, int lds, const float* W, const float* G, const float* link_norm,
                         const float* dloss, float* dS, int ldds, int accumulate, int symmetric, int n, int K,
                         void* stream) {
    return csr_frob_link_bwd("dp_csr_frob_link_bwd", false, S, lds, W, G, nullptr, link_norm, dloss, dS, ldds,
                             accumulate, symmetric, 1, n, K, stream);
}
int dp_csr_frob_link_batch_fwd(const float* S, int lds, const int* indptr, const int* indices, const int* indptr_t,
                               const int* indices_t, const int* node_off, const float* link_norm, float* W, float* G,
                               float* loss_out, float* total_inout, int B, int n_total, int K, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return csr_frob_link_fwd("dp_csr_frob_link_batch_fwd", true, S, lds, indptr, indices, nullptr, indptr_t, indices_t,
                             nullptr, false, node_off, link_norm, W, G, loss_out, total_inout, B, n_total, K, workspace,
                             workspace_bytes, stream);
}
int dp_csr_frob_link_batch_fwd_w(const float* S, int lds, const int* indptr, const int* indices, const float* values,
                                 const int* indptr_t, const int* indices_t, const float* values_t, const int* node_off,
                                 const float* link_norm, float* W, float* G, float* loss_out, float* total_inout, int B,
                                 int n_total, int K, void* workspace, size_t workspace_bytes, void* stream) {
    return csr_frob_link_fwd("dp_csr_frob_link_batch_fwd_w", true, S, lds, indptr, indices, values, indptr_t, indices_t,
                             values_t, true, node_off, link_norm, W, G, loss_out, total_inout, B, n_total, K, workspace,
                             workspace_bytes, stream);
}
int dp_csr_frob_link_batch_bwd(const float* S, int lds, const float* W, const float* G, const int* node_off,
                               const float* link_norm, const float* dloss, float* dS, int ldds, int accumulate,
                               int symmetric, int B, int n_total, int K, void* stream) {
    return csr_frob_link_bwd("dp_csr_frob_link_batch_bwd", true, S, lds, W, G, node_off, link_norm, dloss, dS, ldds,
                             accumulate, symmetric, B, n_total, K, stream);
}
#undef FROB_K_OK
#undef FROB_WS_OK

int dp_cross_entropy_fwd(const float* logits, const long long* label, float* loss_out, float* prob, int B, int C,
                         void* stream) {
    DP_NOTNULL(logits); DP_NOTNULL(label); DP_NOTNULL(loss_out);
    DP_POS(B); DP_POS(C);
    Seq q(DP_STREAM(stream), nullptr, 0);
    ce_fwd(q, logits, label, loss_out, prob, B, C);
    return q.err;
}
int dp_cross_entropy_bwd(const float* prob, const long long* label, const float* dloss, float* dlogits, int B, int C,
                         void* stream) {
    DP_NOTNULL(prob); DP_NOTNULL(label); DP_NOTNULL(dlogits);
    DP_POS(B); DP_POS(C);
    Seq q(DP_STREAM(stream), nullptr, 0);
    ce_bwd(q, prob, label, dloss, 1.f, dlogits, B, C);
    return q.err;
}

size_t dp_set2set_save_bytes(int B, int n, int d) { return set2set_save_bytes(B, n, d); }
int dp_set2set_plan(int n, int d) { return set2set_plan(n, d); }
int dp_set2set_fwd(const float* emb, int lde, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, const float* Wp, const float* bp, float* out, int B, int n, int d, void* save,
                   size_t save_bytes, void* stream) {
    DP_NOTNULL(emb); DP_NOTNULL(w_ih); DP_NOTNULL(w_hh); DP_NOTNULL(b_ih); DP_NOTNULL(b_hh); DP_NOTNULL(Wp);
    DP_NOTNULL(bp); DP_NOTNULL(out); DP_NOTNULL(save);
    DP_CHECK_ARG(B >= 0, "B=%d must not be negative", B);      // B == 0: DP_OK, nothing is launched
    DP_POS(n); DP_POS(d);
    DP_CHECK_ARG(lde >= d, "lde=%d smaller than the row width d=%d", lde, d);
    DP_CHECK_ARG(save_bytes >= set2set_save_bytes(B, n, d), "set2set save buffer too small: %zu < %zu",
                 save_bytes, set2set_save_bytes(B, n, d));
    Seq q(DP_STREAM(stream), nullptr, 0);
    set2set_fwd(q, emb, lde, w_ih, w_hh, b_ih, b_hh, Wp, bp, out, B, n, d, save);
    return q.err;
}
size_t dp_set2set_bwd_workspace_bytes(int B, int n, int d) {
    return sized([&](Seq& q) {
        set2set_bwd(q, 0, d, 0, 0, 0, 0, 0, 0, 0, 0, 0, d, 0, 0, 0, 0, 0, 0, B, n, d, 0);
    });
}
int dp_set2set_bwd(const float* emb, int lde, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, const float* Wp, const float* bp, const float* out, const float* dout,
                   float* demb, int ldde, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* dWp,
                   float* dbp, int B, int n, int d, const void* save, size_t save_bytes, void* workspace,
                   size_t workspace_bytes, void* stream) {
    DP_NOTNULL(emb); DP_NOTNULL(w_ih); DP_NOTNULL(w_hh); DP_NOTNULL(Wp); DP_NOTNULL(out); DP_NOTNULL(dout);
    DP_NOTNULL(demb); DP_NOTNULL(dw_ih); DP_NOTNULL(dw_hh); DP_NOTNULL(db_ih); DP_NOTNULL(db_hh); DP_NOTNULL(dWp);
    DP_NOTNULL(dbp); DP_NOTNULL(save);
    DP_CHECK_ARG(B >= 0, "B=%d must not be negative", B);      // B == 0: DP_OK, the parameter gradients are zeroed
    DP_POS(n); DP_POS(d);
    DP_CHECK_ARG(lde >= d && ldde >= d, "lde=%d / ldde=%d smaller than the row width d=%d", lde, ldde, d);
    DP_CHECK_ARG(save_bytes >= set2set_save_bytes(B, n, d), "set2set save buffer too small");
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    set2set_bwd(q, emb, lde, w_ih, w_hh, b_ih, b_hh, Wp, bp, out, dout, demb, ldde, dw_ih, dw_hh, db_ih, db_hh, dWp,
                dbp, B, n, d, save);
    return q.err;
}

int dp_mean_aggregate_fwd(const float* table, int ldt, const int* indptr, const int* indices, float* out, int ldo,
                          int n_rows, int feat, void* stream) {
    DP_NOTNULL(table); DP_NOTNULL(indptr); DP_NOTNULL(indices); DP_NOTNULL(out);
    DP_POS(n_rows); DP_POS(feat);
    Seq q(DP_STREAM(stream), nullptr, 0);
    mean_aggregate_fwd(q, table, ldt, indptr, indices, out, ldo, n_rows, feat);
    return q.err;
}
int dp_mean_aggregate_bwd(const float* dout, int ldo, const int* indptr, const int* indices, float* dtable, int ldt,
                          int n_rows, int feat, void* stream) {
    DP_NOTNULL(dout); DP_NOTNULL(indptr); DP_NOTNULL(indices); DP_NOTNULL(dtable);
    DP_POS(n_rows); DP_POS(feat);
    Seq q(DP_STREAM(stream), nullptr, 0);
    mean_aggregate_bwd(q, dout, ldo, indptr, indices, dtable, ldt, n_rows, feat);
    return q.err;
}

int dp_bgemm_split_bf16(const float* A, const float* B, float* C, int batch, int M, int N, int K, int lda, int ldb,
                        int ldc, long strideA, long strideB, long strideC, int transA, int transB, float beta,
                        void* stream) {
    DP_NOTNULL(A); DP_NOTNULL(B); DP_NOTNULL(C);
    DP_POS(batch); DP_POS(M); DP_POS(N); DP_POS(K);
    DP_CHECK_ARG(beta == 0.f || beta == 1.f, "beta must be 0 or 1");
    Seq q(DP_STREAM(stream), nullptr, 0);
    GemmDesc d{A, B, C, nullptr, M, N, K, lda, ldb, ldc, strideA, strideB, strideC, transA != 0, transB != 0, 1.f, beta,
               0, 0, 0, nullptr, 0, 0, 0};
    gemm_split_bf16(q, d, batch);
    return q.err;
}

// ------------------------------------------------------------------ N4: CSR GraphConv
static int csr_aggregate_entry(const float* table, int ldt, const int* indptr, const int* indices, const float* values,
                               bool weighted, float* out, int ldo, int n_rows, int feat, int mean, float beta,
                               void* stream) {
    DP_NOTNULL(table); DP_NOTNULL(indptr); DP_NOTNULL(indices);
    DP_VALUES((void)0, "values is NULL");
    DP_NOTNULL(out);
    DP_POS(n_rows); DP_POS(feat);
    Seq q(DP_STREAM(stream), nullptr, 0);
    csr_aggregate_fwd(q, table, ldt, indptr, indices, out, ldo, n_rows, feat, mean, beta, weighted ? values : nullptr);
    return q.err;
}
int dp_csr_aggregate(const float* table, int ldt, const int* indptr, const int* indices, float* out, int ldo, int n_rows,
                     int feat, int mean, float beta, void* stream) {
    return csr_aggregate_entry(table, ldt, indptr, indices, nullptr, false, out, ldo, n_rows, feat, mean, beta, stream);
}
int dp_csr_aggregate_w(const float* table, int ldt, const int* indptr, const int* indices, const float* values,
                       float* out, int ldo, int n_rows, int feat, float beta, void* stream) {
    return csr_aggregate_entry(table, ldt, indptr, indices, values, true, out, ldo, n_rows, feat, 0, beta, stream);
}
namespace {
void sparse_gcn_fwd_seq(Seq& q, const float* x, int ldx, const int* indptr, const int* indices, const float* W,
                        const float* bias, float* y, int ldy, float* ax, float* invn, int n, int Fin, int Fout,
                        int flags, const float* values = nullptr) {
    float* U = q.alloc<float>((size_t)n * Fout);
    if (q.err) return;
    csr_aggregate_fwd(q, x, ldx, indptr, indices, ax, Fin, n, Fin, 0, 0.f, values);
    if (flags & DP_F_ADD_SELF) axpy(q, ax, x, 1.f, (long)n * Fin);          // (x is contiguous: checked at the ABI)
    bgemm(q, ax, W, U, nullptr, 1, n, Fout, Fin, Fin, Fout, Fout, 0, 0, 0, false, false, 1.f, 0.f, 0);
    rownorm_fwd(q, U, Fout, nullptr, gcp(bias, 0), one_group(Fout), gp(y, ldy), invn, nullptr, n,
                (flags & DP_F_NORMALIZE) ? 1 : 0, 0);
}
void sparse_gcn_bwd_seq(Seq& q, const float* ax, const int* indptr, const int* indices, const int* indptr_t,
                        const int* indices_t, const float* W, const float* y, int ldy, const float* invn,
                        const float* dy, int lddy, float* dx, int lddx, float* dW, float* db, int n, int Fin, int Fout,
                        int flags, const float* values = nullptr, const float* values_t = nullptr,
                        const float* x = nullptr, int ldx = 0, float* dvalues = nullptr) {
    float* dU = q.alloc<float>((size_t)n * Fout);
    float* dax = (dx || dvalues) ? q.alloc<float>((size_t)n * Fin) : nullptr;
    if (q.err) return;
    rownorm_bwd(q, gcp(dy, lddy), gcp(nullptr, 0), gcp(y, ldy), invn, nullptr, nullptr, one_group(Fout), dU, Fout,
                nullptr, 1, n, 0, 0, (flags & DP_F_NORMALIZE) ? 1 : 0);
    if (db) colsum_batched(q, dU, Fout, 0, n, Fout, db, 0, 1);
    bgemm(q, ax, dU, dW, nullptr, 1, Fin, Fout, n, Fin, Fout, Fout, 0, 0, 0, true, false, 1.f, 0.f, 0);
    if (!dax) return;
    bgemm(q, dU, W, dax, nullptr, 1, n, Fin, Fout, Fout, Fout, Fin, 0, 0, 0, false, true, 1.f, 0.f, 0);
    if (dx) {
        if (indptr_t && indices_t) {
            csr_aggregate_fwd(q, dax, Fin, indptr_t, indices_t, dx, lddx, n, Fin, 0, 0.f, values_t);      // dx = A^T dax, a gather
        } else {
            zero_fill(q, dx, (size_t)n * Fin * sizeof(float));
            csr_aggregate_bwd_scatter(q, dax, Fin, indptr, indices, dx, lddx, n, Fin, 0, values);
        }
        if (flags & DP_F_ADD_SELF) axpy(q, dx, dax, 1.f, (long)n * Fin);
    }
    // dvalues[e] = dax_i . x_j: every stored entry of A x is its own variable (add_self's + x does not read A)
    if (dvalues) csr_sddmm_identity(q, dax, Fin, x, ldx, indptr, indices, dvalues, n, Fin);
}
}  // namespace
size_t dp_sparse_gcn_layer_workspace_bytes(int n, int Fin, int Fout) {
    return sized([&](Seq& q) { sparse_gcn_fwd_seq(q, 0, Fin, 0, 0, 0, 0, 0, Fout, 0, 0, n, Fin, Fout, 0); },
                 [&](Seq& q) {
                     sparse_gcn_bwd_seq(q, 0, 0, 0, 0, 0, 0, 0, Fout, 0, 0, Fout, (float*)1, Fin, 0, 0, n, Fin, Fout, 0);
                 });
}
static int sparse_gcn_fwd_entry(const float* x, int ldx, const int* indptr, const int* indices, const float* values,
                                bool weighted, const float* W, const float* bias, float* y, int ldy, float* ax,
                                float* invnorm, int n, int Fin, int Fout, int flags, void* workspace,
                                size_t workspace_bytes, void* stream) {
    DP_NOTNULL(x); DP_NOTNULL(indptr); DP_NOTNULL(indices);
    DP_VALUES((void)0, "values is NULL");
    DP_NOTNULL(W); DP_NOTNULL(y); DP_NOTNULL(ax); DP_NOTNULL(invnorm);
    DP_POS(n); DP_POS(Fin); DP_POS(Fout);
    DP_CHECK_ARG(!(flags & DP_F_ADD_SELF) || ldx == Fin, "add_self needs a contiguous x (ldx == Fin)");
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    sparse_gcn_fwd_seq(q, x, ldx, indptr, indices, W, bias, y, ldy, ax, invnorm, n, Fin, Fout, flags,
                       weighted ? values : nullptr);
    return q.err;
}
// x / ldx / dvalues: the gradient to the stored values (dp_sparse_gcn_layer_bwd_dv: want_dv); NULL from the others
static int sparse_gcn_bwd_entry(const char* fn, const float* ax, const int* indptr, const int* indices,
                                const float* values, const int* indptr_t, const int* indices_t, const float* values_t,
                                bool weighted, const float* W, const float* y, int ldy, const float* invnorm,
                                const float* dy, int lddy, float* dx, int lddx, float* dW, float* db, int n, int Fin,
                                int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream,
                                bool want_dv = false, const float* x = nullptr, int ldx = 0, float* dvalues = nullptr) {
    DP_NOTNULL(ax); DP_NOTNULL(indptr); DP_NOTNULL(indices);
    DP_VALUES((void)0, "values is NULL");
    DP_NOTNULL(W); DP_NOTNULL(y); DP_NOTNULL(invnorm); DP_NOTNULL(dy); DP_NOTNULL(dW);
    DP_POS(n); DP_POS(Fin); DP_POS(Fout);
    DP_CHECK_ARG((indptr_t == nullptr) == (indices_t == nullptr), "indptr_t and indices_t come together");
    DP_VALUES_T((void)0, "%s: values_t is NULL but indices_t is a CSR of its own", fn);
    DP_CHECK_ARG(!dx || lddx == Fin, "dx must be contiguous (lddx == Fin)");
    if (want_dv) {
        DP_NOTNULL(x); DP_NOTNULL(dvalues);
        DP_CHECK_ARG(ldx >= Fin, "ldx=%d smaller than Fin=%d", ldx, Fin);
    }
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    sparse_gcn_bwd_seq(q, ax, indptr, indices, indptr_t, indices_t, W, y, ldy, invnorm, dy, lddy, dx, lddx, dW, db, n,
                       Fin, Fout, flags, weighted ? values : nullptr,
                       weighted ? values_t_of(indices, indices_t, values, values_t) : nullptr, want_dv ? x : nullptr, ldx,
                       want_dv ? dvalues : nullptr);
    return q.err;
}
int dp_sparse_gcn_layer_fwd(const float* x, int ldx, const int* indptr, const int* indices, const float* W,
                            const float* bias, float* y, int ldy, float* ax, float* invnorm, int n, int Fin, int Fout,
                            int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return sparse_gcn_fwd_entry(x, ldx, indptr, indices, nullptr, false, W, bias, y, ldy, ax, invnorm, n, Fin, Fout,
                                flags, workspace, workspace_bytes, stream);
}
int dp_sparse_gcn_layer_fwd_w(const float* x, int ldx, const int* indptr, const int* indices, const float* values,
                              const float* W, const float* bias, float* y, int ldy, float* ax, float* invnorm, int n,
                              int Fin, int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return sparse_gcn_fwd_entry(x, ldx, indptr, indices, values, true, W, bias, y, ldy, ax, invnorm, n, Fin, Fout, flags,
                                workspace, workspace_bytes, stream);
}
int dp_sparse_gcn_layer_bwd(const float* ax, const int* indptr, const int* indices, const int* indptr_t,
                            const int* indices_t, const float* W, const float* y, int ldy, const float* invnorm,
                            const float* dy, int lddy, float* dx, int lddx, float* dW, float* db, int n, int Fin,
                            int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return sparse_gcn_bwd_entry("dp_sparse_gcn_layer_bwd", ax, indptr, indices, nullptr, indptr_t, indices_t, nullptr,
                                false, W, y, ldy, invnorm, dy, lddy, dx, lddx, dW, db, n, Fin, Fout, flags, workspace,
                                workspace_bytes, stream);
}
int dp_sparse_gcn_layer_bwd_w(const float* ax, const int* indptr, const int* indices, const float* values,
                              const int* indptr_t, const int* indices_t, const float* values_t, const float* W,
                              const float* y, int ldy, const float* invnorm, const float* dy, int lddy, float* dx,
                              int lddx, float* dW, float* db, int n, int Fin, int Fout, int flags, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return sparse_gcn_bwd_entry("dp_sparse_gcn_layer_bwd_w", ax, indptr, indices, values, indptr_t, indices_t, values_t,
                                true, W, y, ldy, invnorm, dy, lddy, dx, lddx, dW, db, n, Fin, Fout, flags, workspace,
                                workspace_bytes, stream);
}
int dp_sparse_gcn_layer_bwd_dv(const float* ax, const int* indptr, const int* indices, const float* values,
                               const int* indptr_t, const int* indices_t, const float* values_t, const float* W,
                               const float* y, int ldy, const float* invnorm, const float* dy, int lddy, float* dx,
                               int lddx, float* dW, float* db, const float* x, int ldx, float* dvalues, int n, int Fin,
                               int Fout, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return sparse_gcn_bwd_entry("dp_sparse_gcn_layer_bwd_dv", ax, indptr, indices, values, indptr_t, indices_t, values_t,
                                true, W, y, ldy, invnorm, dy, lddy, dx, lddx, dW, db, n, Fin, Fout, flags, workspace,
                                workspace_bytes, stream, true, x, ldx, dvalues);
}

// ------------------------------------------------------------------ model level
size_t dp_sizeof_encoder_cfg(void) { return sizeof(dp_encoder_cfg); }
size_t dp_encoder_save_bytes(const dp_encoder_cfg* cfg) {
    if (encoder_validate(cfg) != DP_OK) return 0;
    return encoder_save_bytes(*cfg) + 256;
}
size_t dp_encoder_workspace_bytes(const dp_encoder_cfg* cfg) {
    if (encoder_validate(cfg) != DP_OK) return 0;
    return sized([&](Seq& q) { encoder_forward(q, *cfg, 0, 0, 0, 0, 0, 0, 0, 0, 0, DP_MODE_TRAIN, 0); },
                 [&](Seq& q) { encoder_backward(q, *cfg, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); });
}
int dp_encoder_save_locate(const dp_encoder_cfg* cfg, int level, int field, size_t* offset, size_t* count) {
    DP_TRY(encoder_validate(cfg));
    DP_NOTNULL(offset); DP_NOTNULL(count);
    DP_CHECK_ARG(level >= 0 && level <= cfg->num_pooling, "level=%d out of range [0,%d]", level, cfg->num_pooling);
    return encoder_save_locate(*cfg, level, field, offset, count);
}
// The dense and the packed name of each pass share one body.  packed: adj_pk / adj_pkt are the bf16 planes of A and
// A^T; else adj_pk is the fp32 adjacency and adj_pkt NULL.  (Neither name checks the planes' alignment.)
static int encoder_forward_entry(const char* fn, bool packed, const dp_encoder_cfg* cfg, const float* params,
                                 const float* x, const void* adj_pk, const void* adj_pkt, const float* assign_x,
                                 const int* num_nodes, const float* dropout, float* ypred, float* assign_out,
                                 long long* labels_out, void* save, size_t save_bytes, void* workspace,
                                 size_t workspace_bytes, int mode, void* stream) {
    DP_TRY(encoder_validate(cfg));
    DP_NOTNULL(params); DP_NOTNULL(x);
    DP_CHECK_ARG(adj_pk != nullptr, "%s is NULL", packed ? "adj_pk" : "adj");
    if (packed) DP_NOTNULL(adj_pkt);
    DP_NOTNULL(ypred); DP_NOTNULL(save);
    DP_CHECK_ARG(cfg->num_pooling == 0 || assign_x, "assign_x is NULL");
    DP_CHECK_ARG(save_bytes >= encoder_save_bytes(*cfg), "save buffer too small: %zu < %zu", save_bytes,
                 encoder_save_bytes(*cfg));
    DEVICE_GATE(fn);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    DP_CHECK_ARG((mode & ~(DP_MODE_TRAIN)) == 0, "mode=%d: DP_MODE_EVAL or DP_MODE_TRAIN", mode);
    if (!packed)
        return encoder_forward(q, *cfg, params, x, static_cast<const float*>(adj_pk), assign_x, num_nodes, dropout,
                               ypred, assign_out, save, mode, labels_out);
    const PackedAdj given{static_cast<const unsigned short*>(adj_pk), static_cast<const unsigned short*>(adj_pkt),
                          adj_pack_ld(cfg->N), nullptr};
    return encoder_forward(q, *cfg, params, x, nullptr, assign_x, num_nodes, dropout, ypred, assign_out, save, mode,
                           labels_out, &given);
}
static int encoder_backward_entry(const char* fn, bool packed, const dp_encoder_cfg* cfg, const float* params,
                                  const float* x, const void* adj_pk, const void* adj_pkt, const float* assign_x,
                                  const int* num_nodes, const float* dropout, const float* d_ypred,
                                  const float* d_assign, float* grads, const void* save, size_t save_bytes,
                                  void* workspace, size_t workspace_bytes, int prezeroed, void* stream) {
    DP_TRY(encoder_validate(cfg));
    DP_NOTNULL(params); DP_NOTNULL(x);
    DP_CHECK_ARG(adj_pk != nullptr, "%s is NULL", packed ? "adj_pk" : "adj");
    if (packed) DP_NOTNULL(adj_pkt);
    DP_NOTNULL(d_ypred); DP_NOTNULL(grads); DP_NOTNULL(save);
    DP_CHECK_ARG(save_bytes >= encoder_save_bytes(*cfg), "save buffer too small: %zu < %zu", save_bytes,
                 encoder_save_bytes(*cfg));
    DEVICE_GATE(fn);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    if (!packed)
        return encoder_backward(q, *cfg, params, x, static_cast<const float*>(adj_pk), assign_x, num_nodes, dropout,
                                d_ypred, d_assign, grads, save, prezeroed);
    const PackedAdj given{static_cast<const unsigned short*>(adj_pk), static_cast<const unsigned short*>(adj_pkt),
                          adj_pack_ld(cfg->N), nullptr};
    return encoder_backward(q, *cfg, params, x, nullptr, assign_x, num_nodes, dropout, d_ypred, d_assign, grads, save,
                            prezeroed, &given);
}
int dp_encoder_forward(const dp_encoder_cfg* cfg, const float* params, const float* x, const float* adj,
                       const float* assign_x, const int* num_nodes, const float* dropout, float* ypred,
                       float* assign_out, long long* labels_out, void* save, size_t save_bytes, void* workspace,
                       size_t workspace_bytes, int mode, void* stream) {
    return encoder_forward_entry("dp_encoder_forward", false, cfg, params, x, adj, nullptr, assign_x, num_nodes,
                                 dropout, ypred, assign_out, labels_out, save, save_bytes, workspace, workspace_bytes,
                                 mode, stream);
}
int dp_encoder_forward_packed(const dp_encoder_cfg* cfg, const float* params, const float* x, const void* adj_pk,
                              const void* adj_pkt, const float* assign_x, const int* num_nodes, const float* dropout,
                              float* ypred, float* assign_out, long long* labels_out, void* save, size_t save_bytes,
                              void* workspace, size_t workspace_bytes, int mode, void* stream) {
    return encoder_forward_entry("dp_encoder_forward_packed", true, cfg, params, x, adj_pk, adj_pkt, assign_x,
                                 num_nodes, dropout, ypred, assign_out, labels_out, save, save_bytes, workspace,
                                 workspace_bytes, mode, stream);
}
int dp_encoder_backward(const dp_encoder_cfg* cfg, const float* params, const float* x, const float* adj,
                        const float* assign_x, const int* num_nodes, const float* dropout, const float* d_ypred,
                        const float* d_assign, float* grads, const void* save, size_t save_bytes, void* workspace,
                        size_t workspace_bytes, int prezeroed, void* stream) {
    return encoder_backward_entry("dp_encoder_backward", false, cfg, params, x, adj, nullptr, assign_x, num_nodes,
                                  dropout, d_ypred, d_assign, grads, save, save_bytes, workspace, workspace_bytes,
                                  prezeroed, stream);
}
int dp_encoder_backward_packed(const dp_encoder_cfg* cfg, const float* params, const float* x, const void* adj_pk,
                               const void* adj_pkt, const float* assign_x, const int* num_nodes, const float* dropout,
                               const float* d_ypred, const float* d_assign, float* grads, const void* save,
                               size_t save_bytes, void* workspace, size_t workspace_bytes, int prezeroed,
                               void* stream) {
    return encoder_backward_entry("dp_encoder_backward_packed", true, cfg, params, x, adj_pk, adj_pkt, assign_x,
                                  num_nodes, dropout, d_ypred, d_assign, grads, save, save_bytes, workspace,
                                  workspace_bytes, prezeroed, stream);
}

size_t dp_loss_workspace_bytes(int B, int N, int K, int linkpred) {
    return sized([&](Seq& q) { loss_fwd_seq(q, 0, 0, 0, 0, 0, 0, 0, 0, 0, B, 1, N, K, linkpred); },
                 [&](Seq& q) { loss_bwd_seq(q, 0, 0, 0, 0, 0, 0, 0, 0, 0, B, 1, N, K, linkpred); });
}
// packed: adj_pk / adj_pkt are the bf16 planes, 16-byte aligned whether or not linkpred reads them; else adj_pk is the
// fp32 adjacency and adj_pkt NULL
static int loss_forward_entry(const char* fn, bool packed, const float* ypred, const long long* label, const float* S,
                              const void* adj_pk, const void* adj_pkt, const int* num_nodes, const float* link_norm,
                              float* loss_out, float* prob, float* d_ypred_unit, int B, int C, int N, int K,
                              int linkpred, void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(ypred); DP_NOTNULL(label); DP_NOTNULL(loss_out); DP_NOTNULL(prob);
    DP_POS(B); DP_POS(C);
    DP_CHECK_ARG(!linkpred || (S && adj_pk && (adj_pkt || !packed) && N > 0 && K > 0), "linkpred needs S, %s, N, K",
                 packed ? "adj_pk, adj_pkt" : "adj");
    if (packed) {
        DP_ALIGNED16_P(adj_pk); DP_ALIGNED16_P(adj_pkt);
    }
    DEVICE_GATE(fn);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    loss_fwd_seq(q, ypred, label, S, packed ? nullptr : static_cast<const float*>(adj_pk), num_nodes, link_norm,
                 loss_out, prob, d_ypred_unit, B, C, N, K, linkpred,
                 packed ? static_cast<const unsigned short*>(adj_pk) : nullptr);
    return q.err;
}
static int loss_backward_entry(const char* fn, bool packed, const float* prob, const long long* label, const float* S,
                               const void* adj_pk, const void* adj_pkt, const int* num_nodes, const float* link_norm,
                               const float* dloss, float* d_ypred, float* dS, int B, int C, int N, int K, int linkpred,
                               void* workspace, size_t workspace_bytes, void* stream) {
    DP_NOTNULL(prob); DP_NOTNULL(label);
    DP_POS(B); DP_POS(C);
    DP_CHECK_ARG(!linkpred || (S && adj_pk && (adj_pkt || !packed) && dS && N > 0 && K > 0),
                 "linkpred needs S, %s, dS, N, K", packed ? "adj_pk, adj_pkt" : "adj");
    if (packed) {
        DP_ALIGNED16_P(adj_pk); DP_ALIGNED16_P(adj_pkt);
    }
    DEVICE_GATE(fn);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    loss_bwd_seq(q, prob, label, S, packed ? nullptr : static_cast<const float*>(adj_pk), num_nodes, link_norm, dloss,
                 d_ypred, dS, B, C, N, K, linkpred, packed ? static_cast<const unsigned short*>(adj_pk) : nullptr,
                 static_cast<const unsigned short*>(adj_pkt));
    return q.err;
}
int dp_loss_forward(const float* ypred, const long long* label, const float* S, const float* adj, const int* num_nodes,
                    const float* link_norm, float* loss_out, float* prob, float* d_ypred_unit, int B, int C, int N,
                    int K, int linkpred, void* workspace, size_t workspace_bytes, void* stream) {
    return loss_forward_entry("dp_loss_forward", false, ypred, label, S, adj, nullptr, num_nodes, link_norm, loss_out,
                              prob, d_ypred_unit, B, C, N, K, linkpred, workspace, workspace_bytes, stream);
}
int dp_loss_forward_packed(const float* ypred, const long long* label, const float* S, const void* adj_pk,
                           const void* adj_pkt, const int* num_nodes, const float* link_norm, float* loss_out,
                           float* prob, float* d_ypred_unit, int B, int C, int N, int K, int linkpred, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return loss_forward_entry("dp_loss_forward_packed", true, ypred, label, S, adj_pk, adj_pkt, num_nodes, link_norm,
                              loss_out, prob, d_ypred_unit, B, C, N, K, linkpred, workspace, workspace_bytes, stream);
}
int dp_loss_backward(const float* prob, const long long* label, const float* S, const float* adj, const int* num_nodes,
                     const float* link_norm, const float* dloss, float* d_ypred, float* dS, int B, int C, int N, int K,
                     int linkpred, void* workspace, size_t workspace_bytes, void* stream) {
    return loss_backward_entry("dp_loss_backward", false, prob, label, S, adj, nullptr, num_nodes, link_norm, dloss,
                               d_ypred, dS, B, C, N, K, linkpred, workspace, workspace_bytes, stream);
}
int dp_loss_backward_packed(const float* prob, const long long* label, const float* S, const void* adj_pk,
                            const void* adj_pkt, const int* num_nodes, const float* link_norm, const float* dloss,
                            float* d_ypred, float* dS, int B, int C, int N, int K, int linkpred, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return loss_backward_entry("dp_loss_backward_packed", true, prob, label, S, adj_pk, adj_pkt, num_nodes, link_norm,
                               dloss, d_ypred, dS, B, C, N, K, linkpred, workspace, workspace_bytes, stream);
}

// adj: the fp32 batch, or NULL beside the packed planes adj_pk / adj_pkt of dp_build_batch_packed
static int build_batch_entry(const int* edge_src, const int* edge_dst, const int* edge_ptr, const int* node_label,
                             const int* node_ptr, float* adj, void* adj_pk, void* adj_pkt, bool packed, float* feats,
                             float* assign_feats, int* num_nodes, int* errors, int* degree, int B, int N, int F,
                             int feature_mode, int symmetric, int max_edges_per_graph, void* stream) {
    DP_NOTNULL(edge_src); DP_NOTNULL(edge_dst); DP_NOTNULL(edge_ptr); DP_NOTNULL(node_ptr);
    if (packed) {
        DP_NOTNULL(adj_pk); DP_NOTNULL(adj_pkt);
    } else {
        DP_NOTNULL(adj);
    }
    DP_NOTNULL(num_nodes); DP_NOTNULL(errors);
    DP_POS(B); DP_POS(N);
    DP_CHECK_ARG(feature_mode >= 0 && feature_mode <= 3, "feature_mode=%d (0 default, 1 id, 2 deg-num, 3 deg)",
                 feature_mode);
    if (packed)
        DP_CHECK_ARG(adj_pk != adj_pkt || symmetric, "A and A^T may share one buffer only for a symmetric edge list");
    const bool labels = feature_mode == 0 || feature_mode == 3;
    DP_CHECK_ARG(!(feats || assign_feats) || !labels || (node_label && F > 0),
                 "label-based features need node labels and F > 0");
    DP_CHECK_ARG(feature_mode < 2 || degree, "deg / deg-num features need the degree workspace (B*N ints)");
    Seq q(DP_STREAM(stream), nullptr, 0);
    build_batch(q, edge_src, edge_dst, edge_ptr, node_label, node_ptr, adj, static_cast<unsigned short*>(adj_pk),
                static_cast<unsigned short*>(adj_pkt), feats, assign_feats, num_nodes, errors, degree, B, N, F,
                feature_mode, symmetric, max_edges_per_graph);
    return q.err;
}
int dp_build_batch(const int* edge_src, const int* edge_dst, const int* edge_ptr, const int* node_label,
                   const int* node_ptr, float* adj, float* feats, float* assign_feats, int* num_nodes, int* errors,
                   int* degree, int B, int N, int F, int feature_mode, int symmetric, int max_edges_per_graph,
                   void* stream) {
    return build_batch_entry(edge_src, edge_dst, edge_ptr, node_label, node_ptr, adj, nullptr, nullptr, false, feats,
                             assign_feats, num_nodes, errors, degree, B, N, F, feature_mode, symmetric,
                             max_edges_per_graph, stream);
}
int dp_build_batch_packed(const int* edge_src, const int* edge_dst, const int* edge_ptr, const int* node_label,
                          const int* node_ptr, void* adj_pk, void* adj_pkt, float* feats, float* assign_feats,
                          int* num_nodes, int* errors, int* degree, int B, int N, int F, int feature_mode,
                          int symmetric, int max_edges_per_graph, void* stream) {
    return build_batch_entry(edge_src, edge_dst, edge_ptr, node_label, node_ptr, nullptr, adj_pk, adj_pkt, true, feats,
                             assign_feats, num_nodes, errors, degree, B, N, F, feature_mode, symmetric,
                             max_edges_per_graph, stream);
}

int dp_gather_labels(const long long* graph_label, long long* label_out, int B, void* stream) {
    DP_NOTNULL(graph_label); DP_NOTNULL(label_out);
    DP_POS(B);
    Seq q(DP_STREAM(stream), nullptr, 0);
    gather_labels(q, graph_label, label_out, B);
    return q.err;
}

size_t dp_clip_adam_workspace_bytes(void) { return 4096; }
// step_counter: the device counter of dp_clip_adam_step_counted, which needs no host step; NULL: `step` is this
// update's 1-based count and the bias corrections come from the host
static int clip_adam_entry(const char* fn, bool counted, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                           long n, int* step_counter, int step, float lr, float beta1, float beta2, float eps,
                           float max_norm, float* total_norm_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
    DP_NOTNULL(params); DP_NOTNULL(grads); DP_NOTNULL(exp_avg); DP_NOTNULL(exp_avg_sq);
    if (counted) DP_NOTNULL(step_counter);
    DP_CHECK_ARG(n >= 0, "n=%ld must be >= 0", n);
    if (!counted) DP_CHECK_ARG(step >= 1, "step=%d is the 1-based count of this update", step);
    DP_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "betas (%g, %g) must lie in [0, 1)",
                 (double)beta1, (double)beta2);
    DEVICE_GATE(fn);
    Seq q(DP_STREAM(stream), workspace, workspace_bytes);
    if (counted) {
        clip_adam_step(q, params, grads, exp_avg, exp_avg_sq, n, max_norm, beta1, beta2, eps, 0.f, 0.f, total_norm_out,
                       step_counter, lr);
        return q.err;
    }
    // bias corrections in double on the host, exactly as torch.optim.Adam's single-tensor path computes them
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    clip_adam_step(q, params, grads, exp_avg, exp_avg_sq, n, max_norm, beta1, beta2, eps, (float)((double)lr / bc1),
                   (float)(1.0 / std::sqrt(bc2)), total_norm_out);
    return q.err;
}
int dp_clip_adam_step_counted(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, int* step_counter,
                              float lr, float beta1, float beta2, float eps, float max_norm, float* total_norm_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return clip_adam_entry("dp_clip_adam_step_counted", true, params, grads, exp_avg, exp_avg_sq, n, step_counter, 0,
                           lr, beta1, beta2, eps, max_norm, total_norm_out, workspace, workspace_bytes, stream);
}
int dp_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, int step, float lr,
                      float beta1, float beta2, float eps, float max_norm, float* total_norm_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return clip_adam_entry("dp_clip_adam_step", false, params, grads, exp_avg, exp_avg_sq, n, nullptr, step, lr, beta1,
                           beta2, eps, max_norm, total_norm_out, workspace, workspace_bytes, stream);
}

}  // extern "C"
