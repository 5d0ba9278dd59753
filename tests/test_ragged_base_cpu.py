"""The base GCN encoder on ragged batches, host side (no GPU): the new class and its refusals, the new dp_* entries'
argument errors (reported before any launch) and workspace queries, the bound of the padded-row table on a table made
in float32 on the host, and the register / scratch budget of the new kernels (read offline from the gfx950 code object,
as tests/test_csr_batch_cpu.py does)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import GcnEncoderGraph
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseBatchGcnEncoderGraph, SparseGcnEncoderGraph
from tests import ragged_base_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")

NEW_SYMBOLS = {
    "dp_ragged_padval_fwd": 9, "dp_ragged_suffix_max_workspace_bytes": 3, "dp_ragged_suffix_max": 11,
    "dp_segment_max_floor_fwd": 21, "dp_segment_max_floor_bwd": 14, "dp_bn_ragged_g_bwd": 24,
    "dp_gcn_row_const_fwd": 5, "dp_gcn_row_const_bwd": 6,
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _three(pad_to=None):
    return CsrBatch.from_edge_lists([3, 1, 5], [[0, 1], [], [0, 1, 2]], [[1, 2], [], [1, 2, 4]], "cpu", pad_to=pad_to)


# ------------------------------------------------------------------ the class
def test_class_has_the_dense_class_state_dict():
    torch.manual_seed(0)
    dense = GcnEncoderGraph(7, 12, 9, 3, 3, pred_hidden_dims=[50])
    torch.manual_seed(0)
    new = SparseBatchGcnEncoderGraph(7, 12, 9, 3, 3, pred_hidden_dims=[50])
    assert isinstance(new, SparseGcnEncoderGraph)
    sd, sn = dense.state_dict(), new.state_dict()
    assert list(sd) == list(sn)
    for k in sd:
        assert sd[k].shape == sn[k].shape and torch.equal(sd[k], sn[k]), k
    new.load_state_dict(sd)


def test_table_rows_of_a_batch():
    b = _three()
    assert (b.min_n, b.max_n, b.pad_to, b.n_idx) == (1, 5, 5, 5)
    b = _three(pad_to=8)
    assert (b.min_n, b.max_n, b.pad_to, b.n_idx) == (1, 5, 8, 6)
    e = CsrBatch.from_edge_lists([4, 4], [[], []], [[], []], "cpu")
    assert e.n_idx == e.min_n == 4                       # no graph has a padded row


def test_forward_checks_its_arguments_before_the_device():
    b = _three()
    with pytest.raises(NotImplementedError, match="add_self GraphConv layers \\(concat=False\\) on a CsrBatch"):
        SparseBatchGcnEncoderGraph(7, 12, 9, 3, 3, concat=False)(torch.zeros(9, 7), b)
    model = SparseBatchGcnEncoderGraph(7, 12, 9, 3, 3)
    with pytest.raises(ValueError, match="n_total = 9"):
        model(torch.zeros(8, 7), b)
    with pytest.raises(ValueError, match="n_total = 9"):
        model(torch.zeros(9, 7, 1), b)
    with pytest.raises(ValueError, match="6 features"):
        model(torch.zeros(9, 6), b)
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.zeros(9, 7), b)                      # shapes fine: no CPU implementation behind it
    with pytest.raises(TypeError, match="CsrGraph"):
        model(torch.zeros(9, 7), "a batch")              # neither container: the parent's refusal
    with pytest.raises(NotImplementedError, match="dropout"):
        SparseBatchGcnEncoderGraph(7, 12, 9, 3, 3, dropout=0.5)
    with pytest.raises(RuntimeError, match="no batch forward"):
        model.saved_activation(0, "readout_argmax")
    with pytest.raises(ValueError, match="unknown activation"):
        model.saved_activation(0, "embedding")
    with pytest.raises(ValueError, match="one class per row"):
        model.loss(torch.zeros(3, 3), torch.zeros(2, dtype=torch.long))
    # the parent class keeps refusing a batch
    with pytest.raises(TypeError, match="unmasked.*suffix-max"):
        SparseGcnEncoderGraph(7, 12, 9, 3, 3)(torch.zeros(9, 7), b)


# ------------------------------------------------------------------ ABI
def test_new_entries_are_exported_and_bound(lib):
    for name, arity in NEW_SYMBOLS.items():
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == arity, name
    assert lib.dp_version() == 100


def test_workspace_queries(lib):
    assert lib.dp_ragged_suffix_max_workspace_bytes(1, 700, 60) == 2 * 2816      # 11 blocks x 60 x 4 bytes, 256-aligned
    assert lib.dp_ragged_suffix_max_workspace_bytes(37, 200, 64) == 2 * 3 * 64 * 4
    assert lib.dp_ragged_suffix_max_workspace_bytes(17, 17, 60) == 0                               # no row at all
    assert lib.dp_ragged_suffix_max_workspace_bytes(0, 17, 60) == 0
    assert lib.dp_ragged_suffix_max_workspace_bytes(1, 17, 2049) == 0
    # the BatchNorm backward with G walks n_idx node indices: the old query at n_idx
    assert lib.dp_bn_ragged_workspace_bytes(5749, 60) >= lib.dp_bn_ragged_workspace_bytes(5748, 60) > 0


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data                                  # a host address: every call below returns before using it
    err = lib.dp_last_error_string
    # padded-row table
    assert lib.dp_ragged_padval_fwd(None, p, p, 4, 1, 5, 5, 4, None) == -1 and b"NULL" in err()
    assert lib.dp_ragged_padval_fwd(p, p, p, 2, 1, 5, 5, 4, None) == -1 and b"ldp=2" in err()             # ld < F
    assert lib.dp_ragged_padval_fwd(p, p, p, 4096, 1, 5, 5, 2049, None) == -3 and b"2048" in err()
    assert lib.dp_ragged_padval_fwd(p, p, p, 4, 6, 5, 5, 4, None) == -1 and b"n_min" in err()
    assert lib.dp_ragged_padval_fwd(p, p, p, 4, 1, 5, 7, 4, None) == -1 and b"tail row" in err()
    assert lib.dp_ragged_padval_fwd(p, p, p, 4, 5, 5, 5, 4, None) == 0                                   # nothing to do
    # suffix maximum
    assert lib.dp_ragged_suffix_max(None, 4, p, p, 4, 1, 5, 4, p, 4096, None) == -1 and b"NULL" in err()
    assert lib.dp_ragged_suffix_max(p, 4, p, p, 2, 1, 5, 4, p, 4096, None) == -1 and b"lds=2" in err()
    assert lib.dp_ragged_suffix_max(p, 4096, p, p, 4096, 1, 5, 2049, p, 4096, None) == -3
    assert lib.dp_ragged_suffix_max(p, 4, p, p, 4, 0, 5, 4, p, 4096, None) == -1 and b"n_min=0" in err()
    assert lib.dp_ragged_suffix_max(p, 4, p, p, 4, 1, 5, 4, p, 16, None) == -2 and b"workspace too small" in err()
    # floored readout
    fwd = lib.dp_segment_max_floor_fwd
    assert fwd(None, 4, p, p, p, 1, p, p, p, 4, 1, 5, None, p, 4, p, 1, 4, p, 4096, None) == -1 and b"NULL" in err()
    assert fwd(p, 4, p, p, p, 1, p, p, p, 4, 1, 5, None, p, 4, p, 0, 4, p, 4096, None) == -1 and b"B=0" in err()
    assert fwd(p, 2, p, p, p, 1, p, p, p, 4, 1, 5, None, p, 4, p, 1, 4, p, 4096, None) == -1 and b"ldz=2" in err()
    assert fwd(p, 4096, p, p, p, 1, p, p, p, 4096, 1, 5, None, p, 4096, p, 1, 2049, p, 4096, None) == -3
    assert fwd(p, 4, p, p, p, 1, p, p, p, 4, 1, 5, p, p, 4, p, 1, 4, p, 4096, None) == -1 and b"not both" in err()
    assert fwd(p, 4, p, p, p, 1, p, p, None, 4, 1, 5, None, p, 4, p, 1, 4, p, 4096, None) == -1 and b"go together" in err()
    assert fwd(p, 4, p, p, p, 1, p, p, p, 2, 1, 5, None, p, 4, p, 1, 4, p, 4096, None) == -1 and b"lds=2" in err()
    assert fwd(p, 4, p, p, p, 1, None, None, None, 4, 1, 5, p, p, 4, p, 1, 4, p, 4096, None) == -1
    assert b"floor_flag" in err()
    assert fwd(p, 4, p, p, p, 1, p, p, p, 4, 1, 5, None, p, 4, p, 1, 4, p, 16, None) == -2                # short workspace
    bwd = lib.dp_segment_max_floor_bwd
    assert bwd(None, 4, p, p, p, 4, p, 4, 1, 5, 1, 1, 4, None) == -1 and b"NULL" in err()
    assert bwd(p, 4, p, p, p, 4, p, 4, 1, 5, 1, 0, 4, None) == -1 and b"B=0" in err()
    assert bwd(p, 2, p, p, p, 4, p, 4, 1, 5, 1, 1, 4, None) == -1 and b"ldo=2" in err()
    assert bwd(p, 4, p, p, p, 4, p, 2, 1, 5, 1, 1, 4, None) == -1 and b"ldg=2" in err()
    assert bwd(p, 4096, p, p, p, 4096, p, 4096, 1, 5, 1, 1, 2049, None) == -3
    # BatchNorm backward with G
    g = lib.dp_bn_ragged_g_bwd
    assert g(p, 4, None, 4, p, p, 4, p, 4, p, p, 4, p, p, p, p, 1, 5, 5, 4, 1, p, 4096, None) == -1 and b"NULL" in err()
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, p, 4, p, p, p, p, 0, 5, 5, 4, 1, p, 4096, None) == -1 and b"B=0" in err()
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, p, 2, p, p, p, p, 1, 5, 5, 4, 1, p, 4096, None) == -1 and b"stride" in err()
    assert g(p, 4096, p, 4096, p, p, 4096, p, 4096, p, p, 4096, p, p, p, p, 1, 5, 5, 2049, 1, p, 4096, None) == -3
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, p, 4, p, p, p, p, 1, 5, 7, 4, 1, p, 4096, None) == -1 and b"tail row" in err()
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, p, 4, p, p, p, None, 1, 5, 5, 4, 1, p, 4096, None) == -1
    assert b"dpad asked for but pad is NULL" in err()
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, p, 4, p, p, p, p, 1, 5, 5, 4, 1, p, 16, None) == -2            # short workspace
    # G = NULL is the old entry, with the old entry's refusals
    assert g(p, 4, p, 4, p, p, 4, p, 4, p, None, 4, p, p, p, None, 1, 5, 5, 4, 1, p, 4096, None) == -1
    assert b"dp_bn_ragged_bwd: dpad asked for" in err()
    # the row constant
    assert lib.dp_gcn_row_const_fwd(p, None, 4, 0, None) == -1 and b"NULL" in err()
    assert lib.dp_gcn_row_const_fwd(p, p, 0, 0, None) == -1 and b"F=0" in err()
    assert lib.dp_gcn_row_const_fwd(p, p, 4, _lib.F_ADD_SELF, None) == -3 and b"DP_F_ADD_SELF" in err()
    assert lib.dp_gcn_row_const_bwd(p, p, None, 4, 0, None) == -1 and b"NULL" in err()
    assert lib.dp_gcn_row_const_bwd(p, p, p, 4, _lib.F_ADD_SELF, None) == -3


# ------------------------------------------------------------------ the bound
def test_counted_bound_holds_for_a_float32_table_made_on_the_host():
    """The bound of tests/ragged_base_cases.py against a float32 evaluation of the same formula by torch on the CPU
    (pairwise sums: fewer roundings than the kernel's count allows), and the reference's own shape conventions."""
    sizes, P, F_ = [40, 7, 1, 12], 43, 20
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(sum(sizes), F_, generator=gen)
    pad = torch.rand(F_, generator=gen) * 0.5
    v64, bound = RC.padval_reference(x, pad, sizes, P)
    n_min, max_n, n_idx = RC.table_rows(sizes, P)
    assert (n_min, max_n, n_idx) == (1, 40, 41) and v64.shape == (41, F_)
    assert float(v64[:1].abs().max()) == 0 and float(bound[1:].min()) > 0
    h = RC.pad_rows(torch.relu(x), sizes, P, fill=pad)
    mu = h.mean(dim=(0, 2))
    r = 1.0 / torch.sqrt((h - mu[None, :, None]).pow(2).mean(dim=(0, 2)) + 1e-5)
    v32 = ((pad[None, :] - mu[:, None]) * r[:, None])[:n_idx].double()
    assert float(((v32 - v64).abs()[1:] / bound[1:]).max()) <= 1.0
    # a padded row of the float64 block holds the table's value; the tail rows are identical
    y = (h.double() - h.double().mean(dim=(0, 2))[None, :, None]) / torch.sqrt(
        (h.double() - h.double().mean(dim=(0, 2))[None, :, None]).pow(2).mean(dim=(0, 2))[None, :, None] + 1e-5)
    assert torch.allclose(y[2, 5], v64[5], rtol=1e-12, atol=1e-12)
    assert torch.equal(y[0, 41], y[0, 40]) and torch.allclose(y[0, 42], v64[40], rtol=1e-12, atol=1e-12)


def test_ring_with_chords_isolates_no_node():
    sizes = [5, 9, 3, 2, 1, 30]
    srcs, dsts = RC.ring_with_chords(sizes, 1)
    for n, s, d in zip(sizes, srcs, dsts):
        deg = np.bincount(np.concatenate([s, d]), minlength=n)
        assert (deg > 0).all() or n == 1, (n, deg)
        assert not (s == d).any()
    g = CsrGraph.from_edges(30, srcs[-1], dsts[-1], "cpu")
    assert (np.diff(g.indptr.numpy()) >= 2).all()


# ------------------------------------------------------------------ kernel resources
def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools not found")
@pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)")
def test_ragged_readout_kernels_do_not_spill():
    """Gather- and reduction-bound kernels: no spills, no scratch, at most 64 VGPRs (full occupancy of 256-thread
    workgroups), as tests/test_csr_batch_cpu.py asks of the kernels next to them."""
    res = KR.kernel_resources(LIB)
    ks = {d["name"]: d for d in res.values()}
    new = ["k_ragged_padval", "k_suffix_block_max", "k_suffix_scan", "k_segment_max_floor_final", "k_floor_bwd_real",
           "k_floor_zero_rows", "k_floor_bwd_pad", "k_bn_ragged_bwd_g", "k_readout_colsum", "k_pad_const_fwd",
           "k_pad_const_bwd"]
    for name in new:
        assert name in ks, (name, sorted(k for k in ks if "ragged" in k or "floor" in k or "suffix" in k))
        d = ks[name]
        assert d["vgpr_spills"] == 0 and d["sgpr_spills"] == 0 and d["scratch"] == 0, d
        assert d["vgprs"] <= 64, d
