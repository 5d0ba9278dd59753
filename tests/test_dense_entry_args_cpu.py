"""Refusals and workspace sizes of the dense C entries (dp_api.hip) and of the six CSR edge / attention / sampling /
top-k units, pinned to the library of the commit before the entry layer got one check vocabulary and one checked body
per dense / packed pair (tests/golden/dense_entry_args.json, recorded from that commit's build).

The design is that of tests/test_csr_entry_args_cpu.py, whose helpers this module imports: every case is ONE fault in
an otherwise valid call (a NULL pointer, a pointer at address + 1, a scalar at a bad value), the entry must refuse it
before it launches anything, and the test compares the return code and the message byte for byte.  Host buffers stand
in for device ones; descriptors and host tables the library reads (dp_encoder_cfg, dp_row_groups, dp_group_ptrs,
dp_gemm_problem, node_off_host, kb_host) are real.  No case of the test is a valid call, and the module skips itself
when a GPU is visible.  Rows are argument refusals only, rc in {-1, -3}; what the bump allocator refuses (-2) stays
out.  The checks of the encoder, loss and Adam entries that sit behind the pending-device-error gate are in the table:
without a device the gate passes.

Every exported name of the seven units is in the table, in the size grid, or in NO_CHECKS with the reason.

Recording (on the PARENT commit's library, never on the tree under test):
    DP_LIB=<parent build>/libdiffpool_hip.so python -m tests.test_dense_entry_args_cpu --record
The recorder, unlike the test, also issues the VALID call of every entry, to prove that each case is one fault in a call
that gets past the argument checks.  On these host addresses such a call must find no device to launch on: the recorder
runs only where no GPU is visible and refuses, before any call, anywhere else.
"""
import ctypes as C
import json
import os
import re
import sys

import pytest

from graph_pooling_amd import _lib
from tests import test_csr_entry_args_cpu as csr
from tests.test_abi_cpu import _header_functions
from tests.test_csr_entry_args_cpu import BIG, INVALID, UNSUPPORTED, _addr, _differences, _ints

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dense_entry_args.json")
CSRC = os.path.join(os.path.dirname(HERE), "graph_pooling_amd", "csrc")
UNITS = ("dp_api", "dp_csr_edge_grad", "dp_csr_edge_ops", "dp_csr_gat", "dp_csr_gat_conv", "dp_csr_sample", "dp_csr_topk")
# exported entries that check no argument: constants, the error state, pure arithmetic on their arguments
NO_CHECKS = {"dp_version", "dp_last_error_string", "dp_device_error", "dp_device_error_describe", "dp_sizeof_gemm_problem",
             "dp_sizeof_row_groups", "dp_sizeof_group_ptrs", "dp_sizeof_encoder_cfg", "dp_adj_pack_ld", "dp_adj_pack_bytes",
             "dp_set2set_plan", "dp_clip_adam_workspace_bytes"}
INF = float("inf")

# scalars of a valid call that an entry's own dict does not name (every leading dimension is wide enough)
DEFAULTS = dict(B=2, n=8, N=8, K=4, D=4, F=4, C=4, Fin=4, Fout=4, Din=4, M=4, batch=1, rows=8, cols=4, n_rows=8, n_total=8,
                feat=4, d=4, nnz=16, H=2, flags=0, trans=0, transA=0, transB=0, alpha=1.0, beta=0.0, act=0, strideA=0,
                strideB=0, strideC=0, strideX=0, strideOut=0, relu=0, accumulate=0, presplit=0, normalize=0, stats_mode=0,
                Bs=0, has_relu=0, has_bn=0, weight=1.0, mode=0, prezeroed=0, linkpred=1, symmetric=1, slope=0.2,
                mean_heads=0, seed=7, self_mode=0, mean=0, inv_norm=1.0, objective=0, lr=0.1, beta1=0.9, beta2=0.999,
                eps=1e-8, max_norm=1.0, step=1, packed=0, fused=0, a_misalign=0, zero_bytes=0, dbias_stride=4, rowsplit=1,
                p_misaligned=0, q_misaligned=0, v_misaligned=0, z_misaligned=0, workspace_bytes=BIG, save_bytes=BIG)


# ------------------------------------------------------------------ descriptors the library reads
_KEEP = []


def _struct(s):
    _KEEP.append(s)
    return C.addressof(s)


def _groups(G=1, c0=(0, 4), w=(4, 4)):
    return _struct(_lib.RowGroups(G=G, c0=(C.c_int * 2)(*c0), w=(C.c_int * 2)(*w)))


def _gptrs(name, ld=4, p=True):
    a = _addr(name) if p else None
    return _struct(_lib.GroupPtrs(p=(C.c_void_p * 2)(a, a), ld=(C.c_int * 2)(ld, ld)))


def _problem(**over):
    f = dict(A=_addr("A"), B=_addr("B"), C=_addr("C"), M=4, N=4, K=4, lda=4, ldb=4, ldc=4, alpha=1.0)
    f.update(over)
    return _struct(_lib.GemmProblem(**f))


def _cfg(B, N, F, H, L, K=0):
    """dp_encoder_cfg of L GraphConv layers of width H on F features; K > 0: one pooling level down to K clusters."""
    c = _lib.EncoderCfg()
    c.B, c.N, c.num_pooling = B, N, 1 if K else 0
    c.n_nodes[0] = N

    def stack(st, dims):
        st.n_layers = len(dims) - 1
        st.dims[:len(dims)] = dims
        st.drop_off[:] = [-1] * _lib.DP_MAX_LAYERS

    stack(c.embed[0], [F] + [H] * L)
    if K:
        c.n_nodes[1] = K
        stack(c.assign[0], [F] + [H] * (L - 1) + [K])
        stack(c.embed[1], [H * L] + [H] * L)
    c.n_pred, c.pred_dims[0], c.pred_dims[1] = 1, H * L * (2 if K else 1), 2
    return c


SMALL, POOLED, NO_CFG = _struct(_cfg(1, 4, 2, 2, 1)), _struct(_cfg(1, 4, 2, 2, 1, K=2)), _struct(_lib.EncoderCfg())
OFF2 = _ints(0, 3, 8)


# ------------------------------------------------------------------ the table
# entry -> (valid scalars / special pointers, faults), the faults as in the CSR table.  E() spells the common ones:
# null / odd: pointer names; pos: scalars refused at 0 and -1; nonneg: refused at -1; ld: refused at 3 (the width is 4)
def E(null="", pos="", odd="", nonneg="", ld="", extra=(), **valid):
    f = [("null", null)] if null else []
    f += [("odd", odd)] if odd else []
    f += [("set", s, (0, -1)) for s in pos.split()] + [("set", s, (-1,)) for s in nonneg.split()]
    f += [("set", s, (3,)) for s in ld.split()]
    return valid, f + list(extra)


def _case(label, **over):
    return ("case", label, over)


def _encoder(packed, bwd):
    adj = "adj_pk adj_pkt" if packed else "adj"
    extra = [_case("cfg invalid", cfg=NO_CFG), ("set", "save_bytes", (0, _ws("dp_encoder_save_bytes", SMALL, less=257)))]
    if not bwd:
        extra += [("set", "mode", (2, -1)), _case("assign_x=NULL with num_pooling=1", cfg=POOLED, assign_x=None)]
    return E(f"cfg params x {adj} save " + ("d_ypred grads" if bwd else "ypred"), extra=extra, cfg=SMALL)


def _loss(packed, bwd):
    adj = "adj_pk adj_pkt" if packed else "adj"
    extra = [("set", "N", (0,)), ("set", "K", (0,))]
    if packed:
        extra += [("odd", adj), _case("linkpred=0 adj_pk+1", linkpred=0, adj_pk=_addr("adj_pk") + 1)]
    return E(("prob label " if bwd else "ypred label loss_out prob ") + f"S {adj}" + (" dS" if bwd else ""), "B C",
             extra=extra)


def _build_batch(packed):
    extra = [("set", "feature_mode", (-1, 4)), ("null", "node_label"), ("set", "F", (0,)),
             _case("feature_mode=2 degree=NULL", feature_mode=2, degree=None)]
    if packed:
        extra += [_case("adj_pkt=adj_pk symmetric=0", adj_pkt=_addr("adj_pk"), symmetric=0)]
    return E("edge_src edge_dst edge_ptr node_ptr num_nodes errors " + ("adj_pk adj_pkt" if packed else "adj"), "B N",
             extra=extra, feature_mode=0, max_edges_per_graph=16)


def _adam(counted):
    extra = [("set", "n", (-1,)), ("set", "beta1", (1.0, -0.5)), ("set", "beta2", (1.0,))]
    return E("params grads exp_avg exp_avg_sq" + (" step_counter" if counted else ""),
             extra=extra + ([] if counted else [("set", "step", (0,))]))


def _rows():
    g, t = _groups(), {}
    bad_g = [_case("G=0", g=_groups(G=0)), _case("G=3", g=_groups(G=3)), _case("w[0]=0", g=_groups(w=(0, 4))),
             _case("c0[0]=-1", g=_groups(c0=(-1, 4))), _case("groups overlap", g=_groups(G=2, c0=(0, 3)))]
    stats = [("set", "stats_mode", (-1, 3)), _case("stats_mode=1 part=NULL", stats_mode=1, part=None)]

    def gp(*names):
        return {n: _gptrs(n) for n in names}

    def bad_gp(n):
        return [_case(f"{n}: group pointer NULL", **{n: _gptrs(n, p=False)}), _case(f"{n}: ld=3", **{n: _gptrs(n, ld=3)})]

    t["dp_rowop_plan"] = E("plan_out g", extra=[("set", "op", (-1, 6)), _case("masked max n=0", op=5, n=0)] + bad_g, op=0, g=g)
    t["dp_rownorm_fwd"] = E("g U yout", "rows", ld="ldu", extra=bad_g + bad_gp("yout") + stats, g=g, **gp("yout", "bias"))
    t["dp_adj_aggregate_rownorm"] = E(
        "g adj V yout", "B n", ld="ldv", g=g, **gp("yout", "bias"),
        extra=bad_gp("yout") + stats + [_case("gap before group 0", g=_groups(c0=(1, 5))), ("null", "packed workspace")])
    t["dp_bn_apply_fwd"] = E("g Y xout stats", "B n", nonneg="Bs", ld="ldy", extra=bad_gp("xout"), g=g, **gp("xout"))
    t["dp_bn_bwd_partials"] = E("g dx xhat part", "rows", extra=bad_gp("dx") + bad_gp("xhat"), g=g, **gp("dx", "xhat"))
    t["dp_rownorm_bwd"] = E(
        "g dx y dU", "B n", nonneg="Bs", ld="ldu", g=g, dbias=None, vs=None, **gp("dx", "y", "xhat"),
        extra=bad_gp("dx") + bad_gp("y") + [
            ("set", "B", (65536,)), _case("has_bn=1 xhat=NULL", has_bn=1, xhat=None),
            _case("has_bn=1 stats=NULL", has_bn=1, stats=None), _case("normalize=1 invn=NULL", normalize=1, invn=None),
            _case("vs+1", vs=_addr("vs") + 1), _case("dbias: ld=3", dbias=_gptrs("dbias", ld=3)),
            _case("dbias and vs at joint width 1024", g=_groups(w=(1024, 4)), ldu=1024, vs=_addr("vs"),
                  **{n: _gptrs(n, ld=1024) for n in ("dx", "y", "dbias")})])
    return t


def _six_units():
    t = {}
    t["dp_csr_sddmm_plan"] = E("plan_out", "F", ld="ldp ldq")
    t["dp_csr_sddmm"] = E("P Q indptr indices out", odd="P Q indptr indices out dscale", nonneg="n_rows F", ld="ldp ldq")
    t["dp_csr_link_dvalues"] = E("S indptr indices dvalues", "K", "S indptr indices dvalues values dloss", "n_rows", "lds",
                                 [("set", "objective", (2, -1))])
    t["dp_csr_pool_dvalues"] = E(
        "S indptr indices dAp dvalues workspace", "K B", "S indptr indices dAp dvalues workspace", "n_total", "lds",
        [_case("node_off_host from 1", node_off_host=_ints(1, 3, 8)), _case("node_off_host decreases", node_off_host=_ints(0, 9, 8)),
         ("null", "node_off_host")], node_off_host=OFF2)
    t["dp_csr_edge_plan"] = E("plan_out", nonneg="n_rows nnz")
    for name, ptrs in (("dp_csr_edge_softmax_fwd", "scores indptr out"), ("dp_csr_edge_softmax_bwd", "out dout indptr dscores")):
        t[name] = E(ptrs, odd=ptrs, nonneg="n_rows nnz")
    ptrs = "indptr indices indptr_t indices_t rdeg out"
    t["dp_csr_sym_norm_fwd"] = E(ptrs + " mirror", odd=ptrs + " values mirror", nonneg="n nnz")
    ptrs = "indptr indices indptr_t indices_t mirror rdeg dout gdeg dvalues"
    t["dp_csr_sym_norm_bwd"] = E(ptrs, odd=ptrs + " values", nonneg="n nnz")

    heads, slope = [("set", "H", (0, 9))], [("set", "slope", (INF,))]
    lds = dict(ldu=2, ldv=2, lddu=2, lddv=2, ldz=8, ldy=8, lddy=8, lddz=8)

    def small(names):
        return [("set", n, (lds[n] - 1,)) for n in names.split()]

    t["dp_csr_gat_plan"] = E("plan_out", nonneg="n_rows nnz", extra=heads + small("ldv"), **lds)
    ptrs = "u v indptr indices out rowstat"
    t["dp_csr_gat_fwd"] = E(ptrs, odd=ptrs, nonneg="n_rows nnz", extra=heads + small("ldu ldv") + slope, **lds)
    ptrs = "u v indptr indices indptr_t indices_t mirror rowstat dout tdot du dv"
    t["dp_csr_gat_bwd"] = E(ptrs, odd=ptrs, nonneg="n nnz", extra=heads + small("ldu ldv lddu lddv") + slope, **lds)
    shape = heads + [("set", "C", (0, 1 << 20))]
    flags = slope + [("set", "mean_heads", (2,))]
    t["dp_csr_gat_conv_plan"] = E("plan_out", nonneg="n_rows nnz", extra=shape + small("ldz"), **lds)
    ptrs = "z u v indptr indices y rowstat"
    t["dp_csr_gat_conv_fwd"] = E(ptrs, odd=ptrs, nonneg="n_rows nnz", extra=shape + flags + small("ldz ldu ldv ldy") + [
        _case("mean_heads=1 ldy=3", mean_heads=1, ldy=3)], **lds)
    ptrs = "z u v indptr indices indptr_t indices_t rowstat dy tdot du dv dz"
    t["dp_csr_gat_conv_bwd"] = E(ptrs, odd=ptrs, nonneg="n nnz", extra=shape + flags + small("ldz ldu ldv lddy lddu lddv lddz"),
                                 **lds)

    shape = [("set", "k", (-1, 65)), ("set", "self_mode", (3, -1))]
    t["dp_csr_sample_mean_plan"] = E("plan_out", nonneg="n_rows n F d", extra=shape + [("set", "n_rows", (9,))], k=2)
    ptrs = "x indptr indices y thr cnt"
    t["dp_csr_sample_mean_fwd"] = E(ptrs, odd=ptrs + " nodes", nonneg="n_rows n F", ld="ldx ldy", k=2, extra=shape + [
        _case("thr+4", thr=_addr("thr") + 4), ("set", "n_rows", (9,)), _case("n_rows=4 nodes=NULL", n_rows=4, nodes=None),
        _case("self_mode=2 ldy=7", self_mode=2, ldy=7)])
    ptrs = "dy indptr_t indices_t thr cnt dx"
    t["dp_csr_sample_mean_bwd"] = E(ptrs, odd=ptrs + " slot", nonneg="n F", ld="lddy lddx", extra=shape[1:] + [
        _case("thr+4", thr=_addr("thr") + 4), _case("self_mode=2 lddy=7", self_mode=2, lddy=7)])

    tk = dict(n=8, n_out=4, B=2, max_n=5, n_b=5, k_b=2, nnz=16, cap=16, node_off_host=OFF2, kb_host=_ints(2, 2))
    over = [("set", "n_out", (9,))]
    t["dp_csr_topk_plan"] = E("plan_out", nonneg="n n_out B max_n F", extra=over + [("set", "n_b", (0, 6)), ("set", "k_b", (0, 6))], **tk)
    ptrs = "score node_off new_off new_id perm thr"
    t["dp_csr_topk_select"] = E(ptrs + " node_off_host kb_host", odd=ptrs, nonneg="n n_out B", extra=[
        _case("thr+4", thr=_addr("thr") + 4), ("set", "B", (0,)), _case("node_off_host from 1", node_off_host=_ints(1, 3, 8)),
        _case("an empty graph", node_off_host=_ints(0, 0, 8)), _case("k_b=4 of 3 nodes", kb_host=_ints(4, 2)),
        _case("the k_b sum to 5", kb_host=_ints(2, 3))], **tk)
    ptrs = "indptr indices new_id perm indptr_out indices_out edge_map new_off workspace"
    t["dp_csr_topk_induce"] = E(ptrs, odd=ptrs + " indices_local_out", nonneg="n n_out B nnz", extra=over + [
        ("set", "cap", (15,)), _case("B=0 with indices_local_out", B=0)], **tk)
    t["dp_csr_topk_gather_fwd"] = E("x perm y", odd="x perm y gate", nonneg="n n_out F", ld="ldx ldy", extra=over, **tk)
    t["dp_csr_topk_gather_bwd"] = E("dy new_id dx gate x", odd="dy new_id dx gate dgate x", nonneg="n n_out F",
                                    ld="lddy lddx ldx", extra=over, **tk)
    return t


def _table():
    t = {}
    t["dp_level0_bwd_symmetric"] = E("count verdicts", nonneg="capacity", capacity=4)
    t["dp_bgemm_f32"] = E("A B C", "batch M N", nonneg="K", ld="lda ldb ldc")
    group = [("set", "count", (0, 5)), ("set", "batch", (0, 65536)), ("set", "ksplit", (0, 2048)), _case("M=-1", p=_problem(M=-1)),
             _case("split=9", p=_problem(split=9)), _case("act=2", p=_problem(act=2))]
    t["dp_bgemm_plan"] = E("plan_out p", extra=group, p=_problem(), count=1, ksplit=1)
    t["dp_bgemm_group_f32"] = E("p", p=_problem(), count=1, ksplit=1, extra=group + [
        _case("lda=3", p=_problem(lda=3)), _case("ldb=3", p=_problem(ldb=3)), _case("ldc=3", p=_problem(ldc=3)),
        _case("atomic with beta", p=_problem(split=_lib.GEMM_ATOMIC, beta=1.0)),
        _case("slabs with act", p=_problem(split=_lib.GEMM_SLABS, act=1, sK=16)),
        _case("slabs with sK=0", p=_problem(split=_lib.GEMM_SLABS)), _case("A=NULL", p=_problem(A=None))])
    t["dp_adj_aggregate"] = E("adj V U", "B n C", ld="ldv ldu")
    t["dp_adj_pack"] = E("adj packed packed_t flag", "B n")
    t["dp_adj_pack_zero"] = E("adj packed packed_t flag zero_p", "B n", zero_bytes=256)
    t["dp_adj_aggregate_packed"] = E("adj packed packed_t flag V U", "B n C", ld="ldv ldu")
    t["dp_adj_aggregate_plan"] = E("plan_out", "B n C", extra=[("set", "a_misalign", (-1, 16))])
    t["dp_gcn_layer_fwd"] = E("x adj W y", "B n Fin Fout", ld="ldx ldy")
    t["dp_gcn_layer_bwd"] = E("x adj W y dy dW", "B n Fin Fout",
                              extra=[_case("normalize with invnorm=NULL", flags=_lib.F_NORMALIZE, invnorm=None)])
    t["dp_bn_node_fwd"] = E("x y stats", "B n F")
    t["dp_bn_node_bwd"] = E("y stats dy dx x", "B n F", relu=1)
    t["dp_assign_softmax_mask_fwd"] = E("z Wp S", "B n Din K")
    t["dp_assign_softmax_mask_bwd"] = E("z Wp S dS dWp", "B n Din K")
    t["dp_pool_fwd"] = E("S Z adj Xp Ap T", "B n K D")
    t["dp_pool_bwd"] = E("S Z adj T dXp dAp dS dZ", "B n K D")
    t["dp_masked_max_fwd"] = E("Z out argmax", "B n F")
    t["dp_masked_max_bwd"] = E("dout argmax dZ", "B n F")
    t.update(_rows())
    grid_y = [("set", "B", (65536,))]
    t["dp_softmax_mask_fwd"] = E("logits S", "B n K", ld="ldl lds", extra=grid_y + [
        _case("vs at K=1024", K=1024, ldl=1024, lds=1024), _case("zero_bytes=16 zero_p=NULL", zero_bytes=16, zero_p=None),
        _case("vs+1", vs=_addr("vs") + 1)])
    t["dp_softmax_mask_bwd"] = E("S dS dlogits", "B n K", ld="lds ldds ldl dbias_stride", extra=grid_y)
    t["dp_colsum_batched"] = E("X out", "rows cols batch", ld="ldx", extra=[("set", "rowsplit", (0, 65536)), ("set", "batch", (65536,))])
    t["dp_linkpred_plan"] = E("plan_out", "B n K", extra=[("set", "K", (257,))])
    t["dp_linkpred_loss_fwd"] = E("S adj loss_out", "B n K")
    t["dp_linkpred_loss_bwd"] = E("S adj dS", "B n K")
    t["dp_linkpred_loss_fwd_packed"] = E("S adj_pk loss_out", "B n K", "adj_pk")
    t["dp_linkpred_loss_bwd_packed"] = E("S adj_pk adj_pkt dS", "B n K", "adj_pk adj_pkt")
    need = _ws("dp_assign_entropy_workspace_bytes", 2, 8, 4)
    t["dp_assign_entropy_fwd"] = E("S ent_out workspace", "B n K", ld="lds", extra=[("set", "workspace_bytes", (0, need))])
    t["dp_assign_entropy_bwd"] = E("S dS", "B n K", ld="lds ldds")
    # the entries the CSR golden holds as well keep its cases; the _dv form adds its own
    for name, spec in csr._table().items():
        if name in _exported():
            t[name] = spec
    v, f = csr._gcn(True, True)
    t["dp_sparse_gcn_layer_bwd_dv"] = (v, f + [("null", "x dvalues"), ("set", "ldx", (3,))])
    t["dp_cross_entropy_fwd"] = E("logits label loss_out", "B C")
    t["dp_cross_entropy_bwd"] = E("prob label dlogits", "B C")
    need = _ws("dp_set2set_save_bytes", 2, 8, 4)
    t["dp_set2set_fwd"] = E("emb w_ih w_hh b_ih b_hh Wp bp out save", "n d", nonneg="B", ld="lde",
                            extra=[("set", "save_bytes", (0, need))])
    t["dp_set2set_bwd"] = E("emb w_ih w_hh Wp out dout demb dw_ih dw_hh db_ih db_hh dWp dbp save", "n d", nonneg="B",
                            ld="lde ldde", extra=[("set", "save_bytes", (0, need))])
    t["dp_mean_aggregate_fwd"] = E("table indptr indices out", "n_rows feat")
    t["dp_mean_aggregate_bwd"] = E("dout indptr indices dtable", "n_rows feat")
    t["dp_bgemm_split_bf16"] = E("A B C", "batch M N K", extra=[("set", "beta", (0.5,))])
    t["dp_encoder_save_locate"] = E("cfg offset count", cfg=SMALL, level=0, field=_lib.SAVE_Z, extra=[
        _case("cfg invalid", cfg=NO_CFG), ("set", "level", (-1, 1)), ("set", "field", (-1, 6, _lib.SAVE_S))])
    for packed in (False, True):
        sfx = "_packed" if packed else ""
        t["dp_encoder_forward" + sfx] = _encoder(packed, False)
        t["dp_encoder_backward" + sfx] = _encoder(packed, True)
        t["dp_loss_forward" + sfx] = _loss(packed, False)
        t["dp_loss_backward" + sfx] = _loss(packed, True)
        t["dp_build_batch" + sfx] = _build_batch(packed)
    t["dp_gather_labels"] = E("graph_label label_out", "B")
    t["dp_clip_adam_step_counted"] = _adam(True)
    t["dp_clip_adam_step"] = _adam(False)
    t.update(_six_units())
    return t


_EXPORTED = set()


def _exported():
    """Every name the seven units define with C linkage."""
    if not _EXPORTED:
        for u in UNITS:
            with open(os.path.join(CSRC, u + ".hip")) as f:
                _EXPORTED.update(re.findall(r"^(?:int|size_t|const char\*)\s+(dp_\w+)\s*\(", f.read(), flags=re.M))
    return _EXPORTED


# ------------------------------------------------------------------ workspace and save queries (host-only dry runs)
def _sizes(lib):
    out = {}

    def put(name, *a):
        shown = ",".join("cfg" + str(_CFGS.index(x)) if isinstance(x, tuple) else str(x) for x in a)
        args = [C.byref(_cfg(*x)) if isinstance(x, tuple) else x for x in a]
        out[f"{name}({shown})"] = getattr(lib, name)(*args)

    for B, n in ((1, 1), (2, 63), (20, 64), (3, 65), (20, 500), (1, 1025)):
        for F in (20, 64, 65, 256):
            put("dp_gcn_layer_workspace_bytes", B, n, F, 20)
            put("dp_gcn_layer_workspace_bytes", B, n, 20, F)
            put("dp_bn_node_workspace_bytes", B, n, F)
            put("dp_assign_workspace_bytes", B, n, 20, F)
            put("dp_pool_bwd_workspace_bytes", B, n, F, 20)
            put("dp_set2set_save_bytes", B, n, F)
            put("dp_set2set_bwd_workspace_bytes", B, n, F)
            put("dp_adj_aggregate_packed_workspace_bytes", B, n, F)
            for q in ("dp_linkpred_workspace_bytes", "dp_assign_entropy_workspace_bytes", "dp_frob_link_workspace_bytes"):
                put(q, B, n, F)
            put("dp_loss_workspace_bytes", B, n, F, 1)
            put("dp_csr_frob_link_workspace_bytes", n, B if B <= n else 1, F)
        put("dp_loss_workspace_bytes", B, n, 20, 0)
        put("dp_sparse_gcn_layer_workspace_bytes", n, 20, 64)
        put("dp_csr_pool_dvalues_workspace_bytes", n, 20)
        put("dp_csr_topk_workspace_bytes", n)
    for q in ("dp_assign_entropy_workspace_bytes", "dp_frob_link_workspace_bytes"):       # the two that answer 0 to a bad shape
        for shape in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (2, 8, 257)):
            put(q, *shape)
    prob = (_lib.GemmProblem * 2)(_lib.GemmProblem(M=20, N=40, K=500, lda=500, ldb=40, ldc=40, alpha=1.0, split=_lib.GEMM_TICKETS),
                                  _lib.GemmProblem(M=17, N=33, K=64, lda=64, ldb=33, ldc=33, alpha=1.0, split=_lib.GEMM_TICKETS))
    for count, batch, ksplit in ((1, 1, 1), (1, 3, 4), (2, 3, 4), (2, 20, 8), (0, 1, 1), (1, 1, 0)):
        out[f"dp_bgemm_group_workspace_bytes(tickets,{count},{batch},{ksplit})"] = \
            lib.dp_bgemm_group_workspace_bytes(prob, count, batch, ksplit)
    for c in _CFGS:
        put("dp_encoder_workspace_bytes", c)
        put("dp_encoder_save_bytes", c)
    out["dp_encoder_workspace_bytes(invalid)"] = lib.dp_encoder_workspace_bytes(C.byref(_lib.EncoderCfg()))
    out["dp_encoder_save_bytes(invalid)"] = lib.dp_encoder_save_bytes(C.byref(_lib.EncoderCfg()))
    return out


# (B, N, F, H, L, K): the smallest cfg and its pooled form, small-level and level-0 sized batches, the benchmark's shape
_CFGS = [(1, 4, 2, 2, 1, 0), (1, 4, 2, 2, 1, 2), (2, 16, 3, 8, 3, 4), (4, 32, 5, 8, 3, 8), (6, 160, 8, 12, 3, 16),
         (20, 500, 8, 30, 3, 50), (20, 1000, 89, 30, 3, 100), (3, 65, 7, 20, 2, 0), (3, 2049, 7, 64, 3, 0)]


# ------------------------------------------------------------------ running the table
def _cases(lib):
    """(entry, case label, argument list) of every fault of the table, and ("", entry, ...) for its valid call."""
    fns = _header_functions()
    for entry, (valid, faults) in _table().items():
        args = [a.split()[-1].lstrip("*") for a in fns[entry][1]]
        is_ptr = ["*" in a for a in fns[entry][1]]
        base = {}
        for a, p in zip(args, is_ptr):
            if a in valid:
                base[a] = valid[a]
            elif p:
                base[a] = None if a in ("stream", "floor_row") else _addr(a)
            else:
                base[a] = DEFAULTS.get(a, 64 if a.startswith("ld") else None)
        missing = [a for a, p in zip(args, is_ptr) if base[a] is None and not p]
        assert not missing, (entry, missing)

        def call(label, /, **over):
            unknown = set(over) - set(args)
            assert not unknown, (entry, label, unknown)
            return entry, label, [over.get(a, base[a]) for a in args]

        yield call("")
        for f in faults:
            if f[0] == "null":
                for p in f[1].split():
                    yield call(f"{p}=NULL", **{p: None})
            elif f[0] == "odd":
                for p in f[1].split():
                    yield call(f"{p}+1", **{p: base[p] + 1})
            elif f[0] == "set":
                for v in f[2]:
                    label = f"{f[1]}=need-1" if isinstance(v, tuple) else f"{f[1]}={v}"
                    if isinstance(v, tuple):              # ("ws", query, args): one byte below what the entry asks for
                        v = getattr(lib, v[1])(*[C.cast(x, C.POINTER(_lib.EncoderCfg)) if x in (SMALL, POOLED) else x
                                                 for x in v[2]]) - (v[3] if len(v) > 3 else 1)
                        assert v > 0, (entry, label)
                    over = {f[1]: v}
                    for ld in csr.WIDTHS.get(f[1], ()):
                        if ld in base and isinstance(base[ld], int) and v > base[ld]:
                            over[ld] = v
                    yield call(label, **over)
            else:
                yield call(f[1], **f[2])


def _ws(query, *a, less=1):                               # less: dp_encoder_save_bytes adds 256 bytes to what the entry asks for
    return ("ws", query, a, less)


def _run(lib, valid_calls=False):
    """Rows [entry, case, rc, message] of the faults; valid_calls: of the valid call of each entry instead."""
    rows = []
    for entry, label, args in _cases(lib):
        if (label == "") != valid_calls:
            continue
        fn = getattr(lib, entry)
        args = [C.cast(a, t) if isinstance(a, int) and hasattr(t, "contents") else a for a, t in zip(args, fn.argtypes)]
        rc = fn(*args)
        rows.append([entry, label, rc, lib.dp_last_error_string().decode() if rc else ""])
    return rows


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        pytest.skip("argument-refusal table runs only where no GPU is visible (host addresses stand in for device ones)")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_refusals_only(golden):
    assert "parent commit" in golden["header"]
    assert golden["rows"] and all(rc in (INVALID, UNSUPPORTED) and msg for _, _, rc, msg in golden["rows"])
    assert len({(e, c) for e, c, _, _ in golden["rows"]}) == len(golden["rows"])
    assert {e for e, _, _, _ in golden["rows"]} == set(_table())
    # no entry drops out unnoticed: the table, the size grid and the entries without a check are the seven units' exports
    sized = {k.split("(")[0] for k in golden["sizes"]}
    assert not (set(_table()) | sized) & NO_CHECKS
    assert set(_table()) | sized | NO_CHECKS == _exported()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(csr.GOLDEN)


def test_every_refusal_keeps_its_code_and_message(lib, golden):
    rows = _run(lib)
    assert all(rc in (INVALID, UNSUPPORTED) for _, _, rc, _ in rows), [r for r in rows if r[2] not in (INVALID, UNSUPPORTED)]
    assert _differences(rows, golden["rows"]) == []
    # negative control: one altered message is found
    bent = [list(r) for r in golden["rows"]]
    bent[len(bent) // 2][3] += "."
    assert len(_differences(rows, bent)) == 1


def test_workspace_queries_keep_their_sizes(lib, golden):
    sizes = _sizes(lib)
    assert sizes == golden["sizes"]
    assert sum(v > 0 for v in sizes.values()) > len(sizes) // 2


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    import torch
    if torch.cuda.is_available():
        sys.exit("--record issues valid calls on host addresses: it runs only where no GPU is visible")
    lib_ = _lib.load()
    rows_ = _run(lib_)
    let_through = [r for r in rows_ if r[2] not in (INVALID, UNSUPPORTED)]
    for r in let_through:
        print("NOT A REFUSAL (table error, not recorded):", r)
    # a case is one fault in an OTHERWISE VALID call: the valid call itself gets past every argument check
    # (the packed encoder entries take the persistent level-0 plan only, which no machine without a device offers: their
    # valid call gets past the argument checks and is refused, -3, by the plan)
    not_valid = [r for r in _run(lib_, valid_calls=True) if r[2] in (INVALID, UNSUPPORTED) and
                 not (r[0] in ("dp_encoder_forward_packed", "dp_encoder_backward_packed") and "level-0 plan" in r[3])]
    for r in not_valid:
        print("THE VALID CALL IS REFUSED (table error, not recorded):", r)
    if let_through or not_valid:
        sys.exit(1)
    with open(GOLDEN, "w") as f_:
        json.dump({"header": "recorded from the library of the parent commit (the tree before the dense entries moved to "
                             "the shared check vocabulary and one checked body per dense/packed pair) with "
                             "tests/test_dense_entry_args_cpu.py --record; rows: [entry, case, rc, message]",
                   "rows": rows_, "sizes": _sizes(lib_)}, f_, indent=0)
    print(f"recorded {len(rows_)} rows from {_lib.LIB_PATH}")
