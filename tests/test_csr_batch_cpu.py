"""Ragged batches of CSR graphs, host side (no GPU): CsrBatch construction, the new dp_* entries declared in
include/diffpool_hip.h and bound in _lib.py, argument errors raised before anything touches the device, and the
register / scratch budget of the new kernels (read offline from the gfx950 code object, as test_kernel_resources_cpu.py
does)."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseGcnEncoderGraph, SparseSoftPoolingGcnEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffpool_hip.h")
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")

NEW_SYMBOLS = {
    "dp_bn_ragged_workspace_bytes": 2, "dp_bn_ragged_fwd": 14, "dp_bn_ragged_bwd": 21,
    "dp_gcn_pad_const_fwd": 5, "dp_gcn_pad_const_bwd": 6,
    "dp_segment_max_workspace_bytes": 2, "dp_segment_max_fwd": 15, "dp_segment_max_bwd": 9,
    "dp_csr_pool_batch_plan": 8, "dp_csr_pool_batch_workspace_bytes": 4, "dp_csr_pool_batch_fwd": 18,
    "dp_csr_pool_batch_bwd": 23,
    "dp_csr_linkpred_batch_workspace_bytes": 3, "dp_csr_linkpred_batch_loss_fwd": 11,
    "dp_csr_linkpred_batch_loss_bwd": 16,
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------ construction
def _three():
    # graph 0: path 0-1-2; graph 1: one node, no edge; graph 2: five nodes, node 3 isolated
    return CsrBatch.from_edge_lists([3, 1, 5], [[0, 1], [], [0, 1, 2]], [[1, 2], [], [1, 2, 4]], "cpu")


def test_offsets_sizes_and_block_diagonal_csr():
    b = _three()
    assert b.num_graphs == 3 and b.n_total == 9 and b.max_n == 5 and b.pad_to == 5
    assert b.num_nodes.tolist() == [3, 1, 5]
    assert b.node_off_host.tolist() == [0, 3, 4, 9] and b.node_off.tolist() == [0, 3, 4, 9]
    assert b.node_off.dtype == torch.int32 and b.indptr.dtype == torch.int32
    assert b.indptr.tolist() == [0, 1, 3, 4, 4, 5, 7, 9, 9, 10]
    assert b.indices_local.tolist() == [1, 0, 2, 1, 1, 0, 2, 1, 4, 2]
    assert b.indices.tolist() == [1, 0, 2, 1, 5, 4, 6, 5, 8, 6]            # graph 2's columns shifted by its first row
    assert b.indptr_t is b.indptr and b.indices_t is b.indices             # undirected: one CSR
    # owners of node index i: graphs with n_b > i, largest graph first
    assert b.order.tolist() == [2, 0, 1] and b.cnt.tolist() == [3, 2, 2, 1, 1]
    assert b.has_padding and b.floor_flag.tolist() == [1, 1, 0]
    assert b.seg_off.tolist() == [0, 1, 2, 3] and b.seg_tab.tolist() == [[0, 0, 3, 0], [1, 3, 4, 0], [2, 4, 9, 0]]


def test_segment_chunks_never_cross_a_graph():
    sizes = [300, 1, 129, 128]
    b = CsrBatch.from_edge_lists(sizes, [[]] * 4, [[]] * 4, "cpu")
    tab, off = b.seg_tab.tolist(), b.seg_off.tolist()
    assert off == [0, 3, 4, 6, 7] and b.seg_chunks == 7
    for g, lo, hi, _ in tab:
        assert b.node_off_host[g] <= lo < hi <= b.node_off_host[g + 1] and hi - lo <= CsrBatch.SEG_ROWS
    assert b.indices.numel() >= 1                    # no edge at all: the index arrays still are not empty


def test_pad_to():
    sizes, e = [4, 2], [[], []]
    assert CsrBatch.from_edge_lists(sizes, e, e, "cpu").floor_flag.tolist() == [0, 1]
    assert CsrBatch.from_edge_lists(sizes, e, e, "cpu", pad_to=4).floor_flag.tolist() == [0, 1]
    b = CsrBatch.from_edge_lists(sizes, e, e, "cpu", pad_to=9)
    assert b.pad_to == 9 and b.max_n == 4 and b.floor_flag.tolist() == [1, 1] and b.cnt.tolist() == [2, 2, 1, 1]
    with pytest.raises(ValueError, match="pad_to = 3 is below the largest graph"):
        CsrBatch.from_edge_lists(sizes, e, e, "cpu", pad_to=3)
    with pytest.raises(ValueError, match="at least one node"):
        CsrBatch.from_edge_lists([4, 0], e, e, "cpu")
    with pytest.raises(ValueError, match="no graph"):
        CsrBatch.from_graphs([])
    with pytest.raises(ValueError, match="column index outside"):
        CsrBatch([2], [(np.array([0, 1, 1]), np.array([5]), None, None)], "cpu")


def test_directed_input_carries_the_transposed_csr():
    b = CsrBatch.from_edge_lists([3, 2], [[0, 0], [1]], [[1, 2], [0]], "cpu", symmetric=False)
    assert b.indptr.tolist() == [0, 2, 2, 2, 2, 3] and b.indices.tolist() == [1, 2, 3]
    assert b.indptr_t is not b.indptr
    assert b.indptr_t.tolist() == [0, 0, 1, 2, 3, 3] and b.indices_t.tolist() == [0, 0, 4]
    assert b.indices_t_local.tolist() == [0, 0, 1]


def test_round_trip_against_from_dense_and_from_graphs():
    rng = np.random.default_rng(0)
    sizes, N = [6, 1, 4], 8
    adj = torch.zeros(3, N, N)
    for g, n in enumerate(sizes):
        a = torch.from_numpy((rng.random((n, n)) < 0.4).astype(np.float32))
        adj[g, :n, :n] = torch.maximum(a, a.t())
    adj[1, 3, 5] = 1.0                                   # outside graph 1's single node: must be ignored
    b = CsrBatch.from_dense(adj, sizes, pad_to=N)
    assert b.pad_to == N and b.floor_flag.tolist() == [1, 1, 1]
    back = torch.zeros(3, N, N)
    ip, ix = b.indptr.tolist(), b.indices_local.tolist()
    for g, n in enumerate(sizes):
        for i in range(n):
            r = int(b.node_off_host[g]) + i
            for e in range(ip[r], ip[r + 1]):
                back[g, i, ix[e]] = 1.0
    adj[1, 3, 5] = 0.0
    assert torch.equal(back, adj)
    graphs = [CsrGraph.from_dense(adj[g, :n, :n]) for g, n in enumerate(sizes) if n > 1]
    b2 = CsrBatch.from_graphs(graphs)
    assert b2.num_nodes.tolist() == [6, 4] and b2.indptr_t is not b2.indptr       # from_dense graphs are directed CSRs
    one = CsrBatch.from_graphs(graphs[:1])
    assert one.num_graphs == 1 and one.n_total == 6 and not one.has_padding and one.floor_flag.tolist() == [0]
    assert one.indices.tolist() == one.indices_local.tolist() == graphs[0].indices.tolist()
    assert one.order.tolist() == [0] and one.cnt.tolist() == [1] * 6


# ------------------------------------------------------------------ ABI
def _header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"typedef struct \{.*?\} \w+;", "", src, flags=re.S)
    src = "\n".join(l for l in src.splitlines() if not l.strip().startswith("#"))
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(dp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_entries_are_declared_exported_and_bound(lib):
    fns = _header_functions()
    for name, arity in NEW_SYMBOLS.items():
        assert name in fns, f"{name} is not declared in diffpool_hip.h"
        assert len(fns[name]) == arity, (name, len(fns[name]))
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == arity, name


def test_pool_plan_keeps_every_slab_inside_its_graph(lib):
    sizes = [300, 41, 1, 1200, 64, 65]
    b = CsrBatch.from_edge_lists(sizes, [[]] * 6, [[]] * 6, "cpu")
    plan = b.pool_plan(50, 60)
    assert b.pool_plan(50, 60) is plan                   # built once per (K, D)
    fwd, soff, bwd = plan.fwd_tab.tolist(), plan.slab_off.tolist(), plan.bwd_tab.tolist()
    assert soff[0] == 0 and soff[-1] == plan.n_slabs == len(fwd) and plan.n_blocks == len(bwd)
    for g in range(6):
        lo, hi = int(b.node_off_host[g]), int(b.node_off_host[g + 1])
        rows = [r for r in fwd[soff[g]:soff[g + 1]]]
        assert rows[0][0] == lo and rows[-1][1] == hi and all(r[2] == g for r in rows)
        assert all(a[1] == c[0] for a, c in zip(rows, rows[1:]))       # consecutive, in row order
    assert sum(-(-n // 64) for n in sizes) == plan.n_blocks
    for lo, hi, g, _ in bwd:
        assert b.node_off_host[g] <= lo < hi <= b.node_off_host[g + 1] and hi - lo <= 64


def test_host_only_entries_refuse_bad_arguments(lib):
    """The plan and the *_workspace_bytes entries make no GPU call; the launch entries' refusals are checked in
    tests/test_gpu_csr_batch.py."""
    off = np.array([0, 3, 3], dtype=np.int32)            # graph 1 has no node
    counts = np.zeros(2, dtype=np.int32)
    assert lib.dp_csr_pool_batch_plan(off.ctypes.data, 2, 8, 8, None, None, None, counts.ctypes.data) == -1
    assert b"no node" in lib.dp_last_error_string()
    good = np.array([0, 3, 5], dtype=np.int32)
    assert lib.dp_csr_pool_batch_plan(good.ctypes.data, 2, 257, 8, None, None, None, counts.ctypes.data) == -3
    assert lib.dp_csr_linkpred_batch_workspace_bytes(off.ctypes.data, 2, 8) == 0
    assert lib.dp_csr_linkpred_batch_workspace_bytes(good.ctypes.data, 2, 8) > 0
    assert lib.dp_csr_linkpred_batch_workspace_bytes(good.ctypes.data, 2, 257) == 0
    assert lib.dp_bn_ragged_workspace_bytes(5748, 60) > 0 and lib.dp_bn_ragged_workspace_bytes(0, 60) == 0
    assert lib.dp_segment_max_workspace_bytes(7, 60) > 0
    assert lib.dp_csr_pool_batch_workspace_bytes(10, 2, 50, 60) > 0
    assert lib.dp_csr_pool_batch_workspace_bytes(10, 2, 257, 60) == 0


# ------------------------------------------------------------------ the classes
ARGS = dict(max_num_nodes=100, input_dim=7, hidden_dim=12, embedding_dim=12, label_dim=3, num_layers=3,
            assign_hidden_dim=12)


def test_forward_and_loss_check_their_arguments_before_the_device():
    b = _three()
    model = SparseSoftPoolingGcnEncoder(**ARGS, linkpred=True)
    with pytest.raises(ValueError, match="n_total = 9"):
        model(torch.zeros(8, 7), b)
    with pytest.raises(ValueError, match="n_total = 9"):
        model(torch.zeros(9, 7), b, assign_x=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="feature widths"):
        model(torch.zeros(9, 6), b)
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.zeros(9, 7), b)                      # shapes fine: no CPU implementation behind it
    pred = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="one class per graph of the batch \\(3\\), got 2"):
        model.loss(pred, torch.zeros(2, dtype=torch.long), b)
    with pytest.raises(ValueError, match="one row per graph"):
        model.loss(torch.zeros(2, 3), torch.zeros(3, dtype=torch.long), b)
    with pytest.raises(ValueError, match="no forward pass has run"):
        model.loss(pred, torch.zeros(3, dtype=torch.long), b)
    other = _three()
    model._saved = {"assign": [torch.zeros(9, 10)], "graph": other}      # as a forward on `other` leaves it
    with pytest.raises(ValueError, match="not the batch the last forward ran on"):
        model.loss(pred, torch.zeros(3, dtype=torch.long), b)
    with pytest.raises(NotImplementedError, match="adj_hop"):
        model.loss(pred, torch.zeros(3, dtype=torch.long), other, adj_hop=2)


def test_add_self_layers_are_refused_on_a_batch():
    """With add_self (concat=False) a padded row of the dense batch is not a constant of the layer.  The DiffPool
    constructor refuses concat=False on either path already; the batch's BatchNorm step says so itself as well."""
    from graph_pooling_amd.encoders import GraphConv
    layer = GraphConv(7, 12, add_self=True, normalize_embedding=True)
    with pytest.raises(NotImplementedError, match="add_self GraphConv layers"):
        _three().bn_relu(torch.zeros(9, 12), layer)
    with pytest.raises(ValueError, match="concat=False"):
        SparseSoftPoolingGcnEncoder(**ARGS, concat=False)


def test_base_encoder_refuses_a_batch_and_says_why():
    m = SparseGcnEncoderGraph(7, 12, 9, 3, 3)
    with pytest.raises(TypeError, match="unmasked.*suffix-max"):
        m(torch.zeros(9, 7), _three())


# ------------------------------------------------------------------ kernel resources
def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools not found")
@pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)")
def test_ragged_batch_kernels_do_not_spill():
    """The new row kernels are gather- and reduction-bound: no spills, no scratch, and few enough registers for full
    occupancy of 256-thread workgroups (<= 64 VGPRs: 8 waves per SIMD).  The table-driven pooling kernels keep the
    budget of test_sparse_pool_cpu.py."""
    res = KR.kernel_resources(LIB)
    ks = {d["name"]: d for d in res.values()}
    new = ["k_bn_ragged_fwd", "k_bn_ragged_bwd", "k_ragged_colsum", "k_pad_const_fwd", "k_pad_const_bwd",
           "k_segment_max_part", "k_segment_max_final", "k_segment_max_bwd"]
    for name in new:
        hits = [d for k, d in ks.items() if k.split("(")[0].split("::")[-1] == name or k == name]
        assert hits, (name, sorted(k for k in ks if "ragged" in k or "segment" in k))
        for d in hits:
            assert d["vgpr_spills"] == 0 and d["sgpr_spills"] == 0 and d["scratch"] == 0, d
            assert d["vgprs"] <= 64, d
    pool = [d for k, d in ks.items() if k.startswith("k_csr_pool_")]
    assert len(pool) >= 14
    for d in pool:
        assert d["vgpr_spills"] == 0 and d["sgpr_spills"] == 0 and d["scratch"] == 0, d
