"""Link-prediction loss on CSR graphs, host side (no GPU): the three dp_csr_linkpred_* symbols are exported and bound,
the workspace stays O(n K), argument errors come back before any launch, the kernels compile without scratch, and
SparseSoftPoolingGcnEncoder.loss names the expected call when it is given the wrong thing."""
import importlib.util
import os

import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.sparse import CsrGraph, SparseSoftPoolingGcnEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")
DP_ERR_INVALID_ARG, DP_ERR_UNSUPPORTED = -1, -3
SYMBOLS = ("dp_csr_linkpred_workspace_bytes", "dp_csr_linkpred_loss_fwd", "dp_csr_linkpred_loss_bwd")

ARGS = dict(max_num_nodes=100, input_dim=9, hidden_dim=12, embedding_dim=10, label_dim=3, num_layers=3,
            assign_hidden_dim=11, assign_ratio=0.25)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "diffpool_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(lib, name).argtypes is not None
    assert len(lib.dp_csr_linkpred_loss_fwd.argtypes) == 10
    assert len(lib.dp_csr_linkpred_loss_bwd.argtypes) == 15


def test_workspace_query_runs_without_a_gpu_and_stays_linear_in_n():
    lib = _lib.load()
    assert lib.dp_csr_linkpred_workspace_bytes(1, 1) > 0
    assert lib.dp_csr_linkpred_workspace_bytes(5748, 50) > 0
    # the bound: below 1 % of an n x n fp32 block at n = 65 536 (172 MB); [split][n][K] partials of an 8-way column
    # split would already be 134 MB
    n = 65536
    assert 0 < lib.dp_csr_linkpred_workspace_bytes(n, 64) < n * n * 4 // 100
    assert lib.dp_csr_linkpred_workspace_bytes(n, 256) < n * n * 4 // 100
    # outside the supported shapes there is nothing to size
    for bad in ((0, 50), (-3, 50), (100, 0), (100, 257)):
        assert lib.dp_csr_linkpred_workspace_bytes(*bad) == 0


def test_argument_errors_come_back_before_any_launch():
    """Host memory stands in for the device buffers: every call below must return before it would launch."""
    lib = _lib.load()
    n, K = 10, 8
    buf = torch.zeros(4096, dtype=torch.float32)
    idx = torch.zeros(64, dtype=torch.int32)
    ws = torch.zeros(lib.dp_csr_linkpred_workspace_bytes(n, K) + 16, dtype=torch.uint8)
    wsp = (ws.data_ptr() + 15) & ~15

    def fwd(S=buf.data_ptr(), lds=K, ip=idx.data_ptr(), ix=idx.data_ptr(), out=buf.data_ptr(), nn=n, kk=K, w=wsp,
            wb=ws.numel() - 16):
        return lib.dp_csr_linkpred_loss_fwd(S, lds, ip, ix, out, nn, kk, w, wb, None)

    def bwd(S=buf.data_ptr(), lds=K, ip=idx.data_ptr(), ix=idx.data_ptr(), ipt=idx.data_ptr(), ixt=idx.data_ptr(),
            dS=buf.data_ptr(), ldds=K, nn=n, kk=K, w=wsp, wb=ws.numel() - 16):
        return lib.dp_csr_linkpred_loss_bwd(S, lds, ip, ix, ipt, ixt, None, dS, ldds, 0, nn, kk, w, wb, None)

    for call in (fwd, bwd):
        assert call(nn=0) == DP_ERR_INVALID_ARG
        assert call(nn=-1) == DP_ERR_INVALID_ARG
        assert call(lds=K - 1) == DP_ERR_INVALID_ARG
        assert call(S=None) == DP_ERR_INVALID_ARG and "NULL" in lib.dp_last_error_string().decode()
        assert call(ip=None) == DP_ERR_INVALID_ARG
        assert call(ix=None) == DP_ERR_INVALID_ARG
        assert call(w=None) == DP_ERR_INVALID_ARG
        assert call(wb=8) == DP_ERR_INVALID_ARG and "workspace" in lib.dp_last_error_string().decode()
        assert call(kk=257, lds=257) == DP_ERR_UNSUPPORTED and "256" in lib.dp_last_error_string().decode()
        assert call(kk=0) == DP_ERR_INVALID_ARG
    assert fwd(out=None) == DP_ERR_INVALID_ARG
    assert bwd(dS=None) == DP_ERR_INVALID_ARG
    assert bwd(ipt=None) == DP_ERR_INVALID_ARG
    assert bwd(ixt=None) == DP_ERR_INVALID_ARG
    assert bwd(ldds=K - 1) == DP_ERR_INVALID_ARG


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
@pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)")
def test_csr_link_kernels_use_no_scratch():
    res = KR.kernel_resources(LIB)
    ks = {d["name"]: d for d in res.values() if d["name"].startswith("k_csr_link_")}
    for stem, count in (("k_csr_link_dense_fwd<", 8), ("k_csr_link_dense_bwd<", 8), ("k_csr_link_edge_fwd<", 6),
                        ("k_csr_link_edge_bwd<", 6)):
        assert len([k for k in ks if k.startswith(stem)]) == count, sorted(ks)
    assert "k_csr_link_final" in ks and "k_csr_link_reduce" in ks, sorted(ks)
    for d in ks.values():
        assert d["scratch"] == 0, d
        assert d["vgpr_spills"] == 0, d


def test_loss_names_the_expected_call():
    m = SparseSoftPoolingGcnEncoder(**ARGS, linkpred=True)
    with pytest.raises(NotImplementedError, match="link-prediction") as e:
        m.loss(None, None)
    assert "link-prediction" in str(e.value) and "loss(pred, label, graph)" in str(e.value)
    with pytest.raises(TypeError, match=r"loss\(pred, label, graph\).*CsrGraph"):
        m.loss(None, None, torch.zeros(1, 4, 4))
    ip = torch.zeros(8, dtype=torch.int32)
    g = CsrGraph(ip, torch.zeros(0, dtype=torch.int32))                 # n = 7
    with pytest.raises(NotImplementedError, match="adj_hop"):
        m.loss(None, None, g, adj_hop=2)
    with pytest.raises(ValueError, match="no forward pass"):
        m.loss(None, None, g)
    m._saved = {"assign": [torch.zeros(5, 25)]}                          # what a forward on a 5-node graph leaves
    with pytest.raises(ValueError, match=r"n = 7 .* n = 5"):
        m.loss(None, None, g)
    # linkpred=False: the graph argument is accepted and ignored, adj_hop is still refused
    m0 = SparseSoftPoolingGcnEncoder(**ARGS, linkpred=False)
    with pytest.raises(NotImplementedError, match="adj_hop"):
        m0.loss(None, None, g, adj_hop=2)
