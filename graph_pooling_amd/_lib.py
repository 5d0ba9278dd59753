"""ctypes binding of libdiffpool_hip.so (include/diffpool_hip.h).

The library is the product: if it is missing this module raises at first use — there is no
PyTorch / CPU fallback behind these calls.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DP_LIB") or os.path.join(_HERE, "libdiffpool_hip.so")   # DP_LIB: a diagnostic build

DP_MAX_LAYERS = 8
DP_MAX_LEVELS = 4
DP_MAX_PRED = 4

F_ADD_SELF, F_NORMALIZE, F_RELU, F_BN, F_LAST_ONLY = 1, 2, 4, 8, 16
MODE_EVAL, MODE_TRAIN = 0, 1
ERR_DEVICE = -4                                   # DP_ERR_DEVICE
DEVERR_BARRIER, DEVERR_NONFINITE_GRAD = 1, 2      # DP_DEVERR_*
SAVE_S, SAVE_XPOOL, SAVE_ADJPOOL, SAVE_Z, SAVE_ZASSIGN, SAVE_ARGMAX = 0, 1, 2, 3, 4, 5


class StackCfg(C.Structure):
    _fields_ = [("n_layers", C.c_int),
                ("dims", C.c_int * (DP_MAX_LAYERS + 1)),
                ("w_off", C.c_long * DP_MAX_LAYERS),
                ("b_off", C.c_long * DP_MAX_LAYERS),
                ("drop_off", C.c_long * DP_MAX_LAYERS)]


class EncoderCfg(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int),
                ("num_pooling", C.c_int),
                ("n_nodes", C.c_int * (DP_MAX_LEVELS + 1)),
                ("embed", StackCfg * (DP_MAX_LEVELS + 1)),
                ("assign", StackCfg * DP_MAX_LEVELS),
                ("assign_pred_w_off", C.c_long * DP_MAX_LEVELS),
                ("assign_pred_b_off", C.c_long * DP_MAX_LEVELS),
                ("n_pred", C.c_int),
                ("pred_dims", C.c_int * (DP_MAX_PRED + 2)),
                ("pred_w_off", C.c_long * (DP_MAX_PRED + 1)),
                ("pred_b_off", C.c_long * (DP_MAX_PRED + 1)),
                ("flags", C.c_int),
                ("readout", C.c_int),
                ("s2s_off", C.c_long * 6),
                ("mask_readout", C.c_int),
                ("n_params", C.c_long),
                ("n_graph_params", C.c_long),
                ("bn_world", C.c_int),
                ("exchange", C.c_void_p),
                ("exchange_user", C.c_void_p)]


class GemmProblem(C.Structure):
    """dp_gemm_problem (include/diffpool_hip.h): one contraction of a dp_bgemm_group_f32 / dp_bgemm_plan group."""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
                ("sA", C.c_int64), ("sB", C.c_int64), ("sC", C.c_int64),
                ("tA", C.c_int), ("tB", C.c_int),
                ("alpha", C.c_float), ("beta", C.c_float),
                ("act", C.c_int),
                ("split", C.c_int),
                ("sK", C.c_int64)]


class RowGroups(C.Structure):
    """dp_row_groups (include/diffpool_hip.h): one or two column groups of a joint buffer."""
    _fields_ = [("G", C.c_int), ("c0", C.c_int * 2), ("w", C.c_int * 2)]


class GroupPtrs(C.Structure):
    """dp_group_ptrs: per group a pointer at the group's first column and its leading dimension."""
    _fields_ = [("p", C.c_void_p * 2), ("ld", C.c_int * 2)]


# dp_rowop_plan: DP_ROWOP_*, DP_ROWK_*, DP_ROWF_*, DP_ROWZ_*
ROWOP_ROWNORM_FWD, ROWOP_ROWNORM_BWD, ROWOP_BN_APPLY_FWD, ROWOP_SOFTMAX_FWD, ROWOP_SOFTMAX_BWD, ROWOP_MASKED_MAX_FWD = range(6)
(ROWK_ROWNORM_FWD, ROWK_ROWNORM_BWD, ROWK_BN_APPLY_FWD, ROWK_SOFTMAX_FWD_PLAN, ROWK_SOFTMAX_FWD, ROWK_SOFTMAX_BWD_PLAN,
 ROWK_SOFTMAX_BWD, ROWK_MASKED_MAX_FWD) = range(8)
ROWF_STATS, ROWF_VS, ROWF_ZERO, ROWF_ZERO_UNALIGNED, ROWF_DBIAS = 1, 2, 4, 8, 16
ROWZ_NONE, ROWZ_FOLDED, ROWZ_APART = 0, 1, 2
ROWOP_PLAN_INTS = 6

# dp_adj_aggregate_plan: DP_AGG_FORM_*, DP_AGG_FB_*; DP_AGG_DECLINED of dp_adj_aggregate_rownorm
(AGG_FORM_PANEL_F32, AGG_FORM_PANEL_BF16, AGG_FORM_WIDE, AGG_FORM_WIDE_DMA, AGG_FORM_GEMM_F32,
 AGG_FORM_GEMM_SPLIT_BF16) = range(6)
AGG_FB_NONE, AGG_FB_PANEL, AGG_FB_GEMM = 0, 1, 2
AGG_PLAN_INTS = 14
AGG_DECLINED = -5

# dp_linkpred_plan: (KT, CW, col_tiles, splits, split_tiles, forward tiles per graph, forward LDS bytes, backward LDS bytes)
LINKPRED_PLAN_INTS = 8
# dp_csr_linkpred_plan: (KT, T, pairs, Z, dense partials, edge partials, CW, col_tiles, splits, split_tiles,
# forward edge VEC, NCH, backward edge VEC, NCH, dense forward LDS bytes, dense backward LDS bytes)
CSR_LINKPRED_PLAN_INTS = 16
# dp_csr_sddmm_plan: (lanes per entry, floats per lane load, register-held visits, column tail, row chunk, rows per workgroup)
CSR_SDDMM_PLAN_INTS = 6
# dp_csr_edge_plan: (lanes per row, entries a lane keeps in registers, rows per workgroup, longest row read once)
CSR_EDGE_PLAN_INTS = 4
# dp_csr_gat_plan: (lanes per row, floats per v load, entries a lane keeps in registers, rows per workgroup, longest row
# read once)
CSR_GAT_PLAN_INTS = 5
CSR_GAT_MAX_HEADS = 8
# dp_csr_gat_conv_plan: (floats per load of a gathered row, column chunks per lane, one coefficient per 16-byte quad, rows
# per workgroup, columns per lane, lanes per row of the forward's statistics pass)
CSR_GAT_CONV_PLAN_INTS = 6
CSR_GAT_CONV_MAX_WIDTH = 512
# dp_csr_sample_mean_plan: (rows per workgroup, forward workgroups, backward workgroups, tier of a row of d entries
# (0 A / 1 B / 2 C), its key chunks, of those in registers, 64-column forward passes, 256-column backward passes)
CSR_SAMPLE_PLAN_INTS = 8
CSR_SAMPLE_ALL, CSR_SAMPLE_MAX_K = 0, 64
CSR_SAMPLE_SELF = {"none": 0, "gcn": 1, "concat": 2}      # DP_CSR_SAMPLE_SELF_*
# dp_csr_topk_plan: (threads of the select workgroup, tier of a graph of n_b nodes keeping k_b (0 all kept / 1 keys in
# registers / 2 keys recomputed), its keys per thread, its radix passes, the chunks of its prefix count, workgroups of the
# select, of an induce count / fill launch, chunks of the scan, workgroups of the gather forward, of the backward)
CSR_TOPK_PLAN_INTS = 10
# dp_csr_block_plan: (flags per compaction chunk, chunks, scan steps, the smallest capacity of src (min(n, n_rows (k + 1));
# n for every neighbour), workgroups of the mark, count and fill launches, of the forward, of the backward at n_src = that
# capacity, 64-column forward passes, 256-column backward passes)
CSR_BLOCK_PLAN_INTS = 11

GEMM_GROUP_MAX = 4
GEMM_WHOLE_K, GEMM_ATOMIC, GEMM_SLABS, GEMM_TICKETS = 0, 1, 2, 3      # dp_gemm_problem.split
GEMM_PLAN_NONE, GEMM_PLAN_SPLIT_BF16 = 0, 1                           # DP_GEMM_PLAN_*


def gemm_plan_decode(plan):
    """(BM, BN, quad, ranges) of a dp_bgemm_plan code that names a tile (DP_GEMM_PLAN_BM / _BN / _QUAD / _RANGES)."""
    return plan >> 20, (plan >> 12) & 255, (plan >> 11) & 1, plan & 2047


# int (*dp_exchange_fn)(void* user, const void* local, void* gathered, size_t bytes_per_rank, void* stream)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


_P = C.c_void_p
_I = C.c_int
_L = C.c_long
_F = C.c_float
_Z = C.c_size_t

# name -> (restype, argtypes); mirrors include/diffpool_hip.h one to one
_PROTOS = {
    "dp_version": (_I, []),
    "dp_last_error_string": (C.c_char_p, []),
    "dp_device_error": (_I, [_I]),
    "dp_device_error_describe": (C.c_char_p, [_I]),
    "dp_profile_level0": (_I, [_I]),
    "dp_profile_level0_read": (_I, [_I, C.POINTER(C.c_double), C.POINTER(_I)]),
    "dp_level0_bwd_symmetric": (_I, [C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I)]),
    "dp_sizeof_encoder_cfg": (_Z, []),
    "dp_bgemm_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _I, _I, _F, _F, _I, _P]),
    "dp_bgemm_split_bf16": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _I, _I, _F, _P]),
    "dp_sizeof_gemm_problem": (_Z, []),
    "dp_bgemm_plan": (_I, [C.POINTER(GemmProblem), _I, _I, _I, C.POINTER(_I)]),
    "dp_bgemm_group_workspace_bytes": (_Z, [C.POINTER(GemmProblem), _I, _I, _I]),
    "dp_bgemm_group_f32": (_I, [C.POINTER(GemmProblem), _I, _I, _I, _P, _Z, _P]),
    "dp_adj_aggregate": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P]),
    "dp_adj_pack_ld": (_I, [_I]),
    "dp_adj_pack_bytes": (_Z, [_I, _I]),
    "dp_adj_pack": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "dp_adj_pack_zero": (_I, [_P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "dp_adj_aggregate_packed_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_adj_aggregate_packed": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _I, _P, _Z, _P]),
    "dp_adj_aggregate_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _F, C.POINTER(_I)]),
    "dp_gcn_layer_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dp_gcn_layer_fwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_gcn_layer_bwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_bn_node_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_bn_node_fwd": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_bn_node_bwd": (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_assign_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dp_assign_softmax_mask_fwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_assign_softmax_mask_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_pool_fwd": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dp_pool_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dp_pool_bwd": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_masked_max_fwd": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dp_masked_max_bwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "dp_sizeof_row_groups": (_Z, []),
    "dp_sizeof_group_ptrs": (_Z, []),
    "dp_rowop_plan": (_I, [_I, C.POINTER(RowGroups), _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_rownorm_fwd": (_I, [_P, _I, _P, C.POINTER(RowGroups), C.POINTER(GroupPtrs), C.POINTER(GroupPtrs), _P, _P, _L, _I,
                            _I, _P]),
    "dp_adj_aggregate_rownorm": (_I, [_P, _P, _P, _P, _P, _I, _P, C.POINTER(RowGroups), C.POINTER(GroupPtrs),
                                      C.POINTER(GroupPtrs), _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_bn_apply_fwd": (_I, [_P, _I, _P, _P, C.POINTER(RowGroups), C.POINTER(GroupPtrs), _I, _I, _I, _I, _P]),
    "dp_bn_bwd_partials": (_I, [C.POINTER(RowGroups), C.POINTER(GroupPtrs), C.POINTER(GroupPtrs), _P, _L, _P]),
    "dp_rownorm_bwd": (_I, [C.POINTER(RowGroups), C.POINTER(GroupPtrs), C.POINTER(GroupPtrs), C.POINTER(GroupPtrs), _P, _P,
                            _P, _P, _I, C.POINTER(GroupPtrs), _I, _I, _I, _I, _I, _P, _I, _P]),
    "dp_softmax_mask_fwd": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "dp_softmax_mask_bwd": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _L, _P, _P]),
    "dp_colsum_batched": (_I, [_P, _I, _L, _I, _I, _P, _L, _I, _I, _P]),
    "dp_linkpred_plan": (_I, [_I, _I, _I, C.POINTER(_I)]),
    "dp_linkpred_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_linkpred_loss_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_linkpred_loss_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_assign_entropy_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_assign_entropy_fwd": (_I, [_P, _I, _P, _F, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_assign_entropy_bwd": (_I, [_P, _I, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P]),
    "dp_frob_link_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_frob_link_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_frob_link_fwd_packed": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_frob_link_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dp_frob_link_bwd_packed": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dp_csr_frob_link_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_csr_frob_link_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "dp_csr_frob_link_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dp_csr_frob_link_batch_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_frob_link_batch_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dp_cross_entropy_fwd": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "dp_cross_entropy_bwd": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "dp_set2set_save_bytes": (_Z, [_I, _I, _I]),
    "dp_set2set_plan": (_I, [_I, _I]),
    "dp_set2set_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_set2set_bwd_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_set2set_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P,
                            _I, _I, _I, _P, _Z, _P, _Z, _P]),
    # Set2Set on a ragged batch (node_off_host is a host pointer, passed as an address)
    "dp_set2set_ragged_plan": (_I, [_I, _I]),
    "dp_set2set_ragged_save_bytes": (_Z, [_P, _I, _I, _I]),
    "dp_set2set_ragged_bwd_workspace_bytes": (_Z, [_P, _I, _I, _I]),
    "dp_set2set_ragged_fwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "dp_set2set_ragged_bwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P,
                                   _P, _P, _P, _Z, _P, _Z, _P]),
    "dp_mean_aggregate_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "dp_mean_aggregate_bwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "dp_csr_aggregate": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "dp_sparse_gcn_layer_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_sparse_gcn_layer_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_sparse_gcn_layer_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z,
                                     _P]),
    "dp_csr_pool_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_csr_pool_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_pool_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_linkpred_workspace_bytes": (_Z, [_I, _I]),
    "dp_csr_linkpred_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_linkpred_loss_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "dp_csr_linkpred_loss_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    # ragged batches of CSR graphs (host pointers — node_off_host, the plan's tables — are passed as addresses too)
    "dp_bn_ragged_workspace_bytes": (_Z, [_I, _I]),
    "dp_bn_ragged_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dp_bn_ragged_bwd": (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_gcn_pad_const_fwd": (_I, [_P, _P, _I, _I, _P]),
    "dp_gcn_pad_const_bwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "dp_segment_max_workspace_bytes": (_Z, [_I, _I]),
    "dp_segment_max_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _P, _Z, _P]),
    "dp_segment_max_bwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    # the base encoder's unmasked max readout on a ragged batch
    "dp_ragged_padval_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dp_ragged_suffix_max_workspace_bytes": (_Z, [_I, _I, _I]),
    "dp_ragged_suffix_max": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_segment_max_floor_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _I, _P, _Z, _P]),
    "dp_segment_max_floor_bwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dp_bn_ragged_g_bwd": (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z,
                                _P]),
    "dp_gcn_row_const_fwd": (_I, [_P, _P, _I, _I, _P]),
    "dp_gcn_row_const_bwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "dp_csr_pool_batch_plan": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "dp_csr_pool_batch_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dp_csr_pool_batch_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_pool_batch_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P,
                                   _Z, _P]),
    "dp_csr_linkpred_batch_workspace_bytes": (_Z, [_P, _I, _I]),
    "dp_csr_linkpred_batch_loss_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _P, _Z, _P]),
    "dp_csr_linkpred_batch_loss_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _Z, _P]),
    # weighted CSR: `values` behind each index array (`values_t` behind a transposed one)
    "dp_csr_aggregate_w": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "dp_sparse_gcn_layer_fwd_w": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_sparse_gcn_layer_bwd_w": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I,
                                       _P, _Z, _P]),
    "dp_csr_pool_fwd_w": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_pool_bwd_w": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_pool_batch_fwd_w": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_pool_batch_bwd_w": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I,
                                     _I, _P, _Z, _P]),
    "dp_csr_linkpred_loss_fwd_w": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "dp_csr_linkpred_loss_bwd_w": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_linkpred_batch_loss_fwd_w": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _Z, _P]),
    "dp_csr_linkpred_batch_loss_bwd_w": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_frob_link_fwd_w": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "dp_csr_frob_link_batch_fwd_w": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    # gradients to the stored values: the SDDMM family (node_off_host is a host pointer, passed as an address)
    "dp_csr_sddmm_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_sddmm": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _F, _P]),
    "dp_csr_link_dvalues": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P]),
    "dp_csr_pool_dvalues_workspace_bytes": (_Z, [_I, _I]),
    "dp_csr_pool_dvalues": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P, _Z, _P]),
    "dp_sparse_gcn_layer_bwd_dv": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _P,
                                        _I, _I, _I, _I, _P, _Z, _P]),
    # learned edge weights: softmax over each CSR row, D^-1/2 A D^-1/2 on the device, both with their backward
    "dp_csr_edge_plan": (_I, [_I, _I, C.POINTER(_I)]),
    "dp_csr_edge_softmax_fwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "dp_csr_edge_softmax_bwd": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "dp_csr_sym_norm_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "dp_csr_sym_norm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    # multi-head additive (GAT) edge attention, fused: scores, softmax over each CSR row and the mean over the heads
    "dp_csr_gat_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_gat_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "dp_csr_gat_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _F, _P]),
    # multi-head GAT convolution: the coefficients multiplied into the gathered neighbour rows, per head
    "dp_csr_gat_conv_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_gat_conv_fwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _F, _I, _P]),
    "dp_csr_gat_conv_bwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _I, _I, _I,
                                 _I, _I, _F, _I, _P]),
    # GraphSAGE neighbour sampling fused with the mean: the sample a function of (seed, i, j), re-derived in the backward
    "dp_csr_sample_mean_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_sample_mean_fwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _L, _P]),
    "dp_csr_sample_mean_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _L, _P]),
    # top-k (gPool / SAGPool) pooling: select + renumber, the induced CSR, gather * gate (node_off_host / kb_host are host
    # pointers, passed as addresses)
    "dp_csr_topk_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_topk_workspace_bytes": (_Z, [_I]),
    "dp_csr_topk_select": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dp_csr_topk_induce": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_csr_topk_gather_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dp_csr_topk_gather_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    # sampled frontier blocks for nested GraphSAGE mini-batches: src / slot built on the device, the sampled mean on
    # compact rows
    "dp_csr_block_plan": (_I, [_I, _I, _I, _I, C.POINTER(_I)]),
    "dp_csr_block_workspace_bytes": (_Z, [_I]),
    "dp_csr_block_build": (_I, [_P, _P, _P, _I, _I, _I, _L, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "dp_csr_block_mean_fwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _L, _P]),
    "dp_csr_block_mean_bwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _L, _P]),
    "dp_encoder_save_bytes": (_Z, [C.POINTER(EncoderCfg)]),
    "dp_encoder_workspace_bytes": (_Z, [C.POINTER(EncoderCfg)]),
    "dp_encoder_save_locate": (_I, [C.POINTER(EncoderCfg), _I, _I, C.POINTER(_Z), C.POINTER(_Z)]),
    "dp_encoder_forward": (_I, [C.POINTER(EncoderCfg), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _I, _P]),
    "dp_encoder_backward": (_I, [C.POINTER(EncoderCfg), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _I, _P]),
    "dp_encoder_forward_packed": (_I, [C.POINTER(EncoderCfg), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _I,
                                       _P]),
    "dp_encoder_backward_packed": (_I, [C.POINTER(EncoderCfg), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _I,
                                        _P]),
    "dp_build_batch": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dp_build_batch_packed": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dp_clip_adam_workspace_bytes": (_Z, []),
    "dp_clip_adam_step": (_I, [_P, _P, _P, _P, _L, _I, _F, _F, _F, _F, _F, _P, _P, _Z, _P]),
    "dp_clip_adam_step_counted": (_I, [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _P, _P, _Z, _P]),
    "dp_gather_labels": (_I, [_P, _P, _I, _P]),
    "dp_loss_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dp_loss_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_loss_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    # packed-adjacency link-prediction loss
    "dp_linkpred_loss_fwd_packed": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "dp_linkpred_loss_bwd_packed": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_loss_forward_packed": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dp_loss_backward_packed": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
}

EXPORTED_SYMBOLS = tuple(_PROTOS.keys())

_lib = None
_lock = threading.Lock()


def load():
    """Load the shared library (once). Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the DiffPool HIP extension is not built. Run "
                "graph_pooling_amd/csrc/build.sh (or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "There is no PyTorch fallback for this path.")
        # torch must load ITS libamdhip64 first: the .so then binds to that already-loaded runtime. Loading
        # ours first puts two HIP runtimes in one process and the second one finds no device.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(lib, name)      # AttributeError if the .so does not export what the header declares
            fn.restype = res
            fn.argtypes = args
        if lib.dp_sizeof_encoder_cfg() != C.sizeof(EncoderCfg):
            raise RuntimeError("dp_encoder_cfg layout mismatch between diffpool_hip.h and _lib.py: "
                               f"{lib.dp_sizeof_encoder_cfg()} vs {C.sizeof(EncoderCfg)}")
        if lib.dp_sizeof_gemm_problem() != C.sizeof(GemmProblem):
            raise RuntimeError("dp_gemm_problem layout mismatch between diffpool_hip.h and _lib.py: "
                               f"{lib.dp_sizeof_gemm_problem()} vs {C.sizeof(GemmProblem)}")
        if lib.dp_sizeof_row_groups() != C.sizeof(RowGroups) or lib.dp_sizeof_group_ptrs() != C.sizeof(GroupPtrs):
            raise RuntimeError("dp_row_groups / dp_group_ptrs layout mismatch between diffpool_hip.h and _lib.py")
        _lib = lib
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dp_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(f"{what or 'libdiffpool_hip'} failed (code {rc}): {msg}")


def level0_bwd_symmetric():
    """(verdicts, rows per workgroup) of the last persistent level-0 backward on the current device: per graph 1 where it
    took the symmetric-adjacency short form (dp_level0_bwd_symmetric; synchronises the device).  ([], 0) when no such
    launch has run."""
    out, n, rb = (C.c_int * 64)(), C.c_int(0), C.c_int(0)
    check(load().dp_level0_bwd_symmetric(out, 64, C.byref(n), C.byref(rb)), "dp_level0_bwd_symmetric")
    return list(out[:n.value]), rb.value


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_gpu_tensor(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on the GPU: the DiffPool HIP path has no CPU implementation "
                           "(move the model and its inputs to 'cuda')")
