"""N4 DiffPool on CSR graphs, host side (no GPU): SparseSoftPoolingGcnEncoder is parameter-compatible with
SoftPoolingGcnEncoder, refuses what it does not run, and the dp_csr_pool kernels compile without spills or scratch
(read offline from the gfx950 code object, as test_kernel_resources_cpu.py does)."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

from graph_pooling_amd.encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import SparseGcnEncoderGraph, SparseSoftPoolingGcnEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")

ARGS = dict(max_num_nodes=100, input_dim=9, hidden_dim=12, embedding_dim=10, label_dim=3, num_layers=3,
            assign_hidden_dim=11, assign_ratio=0.25)


@pytest.mark.parametrize("num_pooling", [1, 2, 3])
@pytest.mark.parametrize("hidden", [[], [50]])
def test_state_dict_keys_and_shapes_match_the_dense_class(num_pooling, hidden):
    ratio = 0.25 if num_pooling < 3 else 0.5
    kw = dict(ARGS, assign_ratio=ratio, num_pooling=num_pooling, pred_hidden_dims=hidden)
    dense = SoftPoolingGcnEncoder(**kw).state_dict()
    sparse = SparseSoftPoolingGcnEncoder(**kw)
    got = sparse.state_dict()
    assert list(got) == list(dense)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in dense.items()}
    sparse.load_state_dict(dense)          # parameters move between the two classes


def test_dense_constructor_refusals_still_apply():
    with pytest.raises(ValueError, match="concat=False"):
        SparseSoftPoolingGcnEncoder(**ARGS, concat=False)
    with pytest.raises(ValueError, match="assign_num_layers"):
        SparseSoftPoolingGcnEncoder(**ARGS, assign_num_layers=2)


def test_csr_path_refusals_name_the_reason():
    with pytest.raises(NotImplementedError, match="dropout"):
        SparseSoftPoolingGcnEncoder(**ARGS, dropout=0.1)
    with pytest.raises(ValueError, match="K_0 = 257"):
        SparseSoftPoolingGcnEncoder(**dict(ARGS, max_num_nodes=257, assign_ratio=1.0))
    SparseSoftPoolingGcnEncoder(**dict(ARGS, max_num_nodes=256, assign_ratio=1.0))          # K_0 = 256 is fine
    with pytest.raises(ValueError, match="D <= 512"):
        SparseSoftPoolingGcnEncoder(**dict(ARGS, hidden_dim=200, embedding_dim=200))        # D = 600
    m = SparseSoftPoolingGcnEncoder(**ARGS, linkpred=True)
    with pytest.raises(NotImplementedError, match="link-prediction"):
        m.loss(None, None)
    with pytest.raises(RuntimeError, match="no forward pass"):
        m.saved_activation(0, "assign")
    with pytest.raises(TypeError, match="CsrGraph"):
        m.forward(None, None)


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("hidden", [[], [50], [20, 10]])
def test_base_encoder_state_dict_equals_the_dense_class_under_one_seed(hidden, concat, bn):
    """SparseGcnEncoderGraph's contract: the dense class's keys, in its order, and its initial values."""
    kw = dict(pred_hidden_dims=hidden, concat=concat, bn=bn)
    torch.manual_seed(11)
    dense = GcnEncoderGraph(7, 12, 9, 3, 3, **kw).state_dict()
    torch.manual_seed(11)
    sparse = SparseGcnEncoderGraph(7, 12, 9, 3, 3, **kw).state_dict()
    assert list(sparse) == list(dense)
    for k, v in dense.items():
        assert torch.equal(sparse[k], v), k


def test_base_encoder_refusals():
    with pytest.raises(NotImplementedError, match="dropout on the CSR path"):
        SparseGcnEncoderGraph(7, 12, 9, 3, 3, dropout=0.5)
    m = SparseGcnEncoderGraph(7, 12, 9, 3, 3)
    with pytest.raises(TypeError, match="GcnEncoderGraph's"):         # the dense call form is not inherited
        m.forward(torch.zeros(2, 5, 7), torch.zeros(2, 5, 5))


def test_ops_sits_below_encoders_and_sparse():
    code = ("import sys, graph_pooling_amd.ops\n"
            "bad = [m for m in ('encoders', 'sparse', 'set2set') if 'graph_pooling_amd.' + m in sys.modules]\n"
            "assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ kernel resources
def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
@pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)")
def test_csr_pool_kernels_do_not_spill():
    res = KR.kernel_resources(LIB)
    ks = {d["name"]: d for d in res.values() if d["name"].startswith("k_csr_pool_")}
    fwd = [k for k in ks if k.startswith("k_csr_pool_fwd<")]
    bwd = [k for k in ks if k.startswith("k_csr_pool_bwd<")]
    assert len(fwd) == 6 and len(bwd) == 6, sorted(ks)
    assert "k_csr_pool_reduce" in ks and "k_csr_pool_bwd_prep" in ks, sorted(ks)
    for name, d in ks.items():
        assert d["vgpr_spills"] == 0, d
        assert d["sgpr_spills"] == 0, d
        assert d["scratch"] == 0, d
