"""What the assignment-entropy term shows without a GPU: header, exports and binding agree; argument errors come back
before any launch; the workspace does not grow with K; constructor and loss() validation on both classes; the new
kernels' resources; and — in numpy — that the forward bound of tests/assign_ent_cases.py tells the defects a kernel of
this kind can have from rounding."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import SparseSoftPoolingGcnEncoder
from tests import assign_ent_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")
DP_ERR_INVALID_ARG = -1
SYMBOLS = ("dp_assign_entropy_workspace_bytes", "dp_assign_entropy_fwd", "dp_assign_entropy_bwd")
ARGS = dict(max_num_nodes=100, input_dim=9, hidden_dim=12, embedding_dim=10, label_dim=3, num_layers=3,
            assign_hidden_dim=11, assign_ratio=0.25)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "diffpool_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(lib, name).argtypes is not None
    assert len(lib.dp_assign_entropy_fwd.argtypes) == 12
    assert len(lib.dp_assign_entropy_bwd.argtypes) == 12
    assert lib.dp_version() == 100


def test_workspace_is_positive_and_does_not_grow_with_k():
    lib = _lib.load()
    assert lib.dp_assign_entropy_workspace_bytes(1, 1, 1) > 0
    rows = 1 << 20
    small, wide = lib.dp_assign_entropy_workspace_bytes(1, rows, 8), lib.dp_assign_entropy_workspace_bytes(1, rows, 256)
    assert 0 < small == wide                                  # O(rows) at the most, never O(rows K)
    assert wide <= rows * 4
    assert lib.dp_assign_entropy_workspace_bytes(256, 1024, 256) <= 256 * 1024 * 4
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
        assert lib.dp_assign_entropy_workspace_bytes(*bad) == 0


def test_argument_errors_come_back_before_any_launch():
    """Host memory stands in for the device buffers: every call below must return before it would launch."""
    lib = _lib.load()
    B, n, K = 2, 5, 8
    buf = torch.zeros(4096, dtype=torch.float32)
    ws = torch.zeros(lib.dp_assign_entropy_workspace_bytes(B, n, K), dtype=torch.uint8)
    err = lambda: lib.dp_last_error_string().decode()          # noqa: E731

    def fwd(S=buf.data_ptr(), lds=K, out=buf.data_ptr(), b=B, nn=n, kk=K, w=ws.data_ptr(), wb=ws.numel()):
        return lib.dp_assign_entropy_fwd(S, lds, None, 0.5, out, None, b, nn, kk, w, wb, None)

    def bwd(S=buf.data_ptr(), lds=K, dS=buf.data_ptr(), ldds=K, b=B, nn=n, kk=K):
        return lib.dp_assign_entropy_bwd(S, lds, None, None, 0.5, dS, ldds, 0, b, nn, kk, None)

    for call in (fwd, bwd):
        assert call(S=None) == DP_ERR_INVALID_ARG and "S is NULL" in err()
        assert call(kk=0) == DP_ERR_INVALID_ARG and "K=0" in err()
        assert call(b=0) == DP_ERR_INVALID_ARG and "B=0" in err()
        assert call(nn=0) == DP_ERR_INVALID_ARG and "n=0" in err()
        assert call(nn=-3) == DP_ERR_INVALID_ARG
        assert call(lds=K - 1) == DP_ERR_INVALID_ARG and "lds=7" in err()
    assert fwd(out=None) == DP_ERR_INVALID_ARG and "ent_out is NULL" in err()
    assert fwd(w=None) == DP_ERR_INVALID_ARG and "workspace is NULL" in err()
    assert fwd(wb=8) == DP_ERR_INVALID_ARG and "workspace too small" in err()
    assert bwd(dS=None) == DP_ERR_INVALID_ARG and "dS is NULL" in err()
    assert bwd(ldds=K - 1) == DP_ERR_INVALID_ARG and "ldds=7" in err()


@pytest.mark.parametrize("cls", [SoftPoolingGcnEncoder, SparseSoftPoolingGcnEncoder])
def test_constructor_and_loss_validation(cls):
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="assign_ent_weight"):
            cls(**ARGS, assign_ent_weight=bad)
    m0 = cls(**ARGS)
    assert m0.assign_ent_weight == 0.0 and m0.assign_ent_loss is None and m0.assign_ent is True
    m = cls(**ARGS, linkpred=False, assign_ent_weight=0.3)
    assert m.assign_ent_weight == pytest.approx(0.3) and m.assign_ent_loss is None
    with pytest.raises(ValueError, match="no forward pass"):
        m.loss(torch.zeros(1, 3), torch.zeros(1, dtype=torch.int64))
    # sync-BN: refused, naming the global normaliser; weight 0 is not
    m._sync_bn = types.SimpleNamespace(active=True, world=2)
    with pytest.raises(NotImplementedError, match="global normaliser"):
        m.loss(torch.zeros(1, 3), torch.zeros(1, dtype=torch.int64))
    assert m.assign_ent_loss is None


def test_the_keyword_is_the_last_one_and_nothing_else_moved():
    import inspect
    for cls in (SoftPoolingGcnEncoder, SparseSoftPoolingGcnEncoder):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-2:] == ["args", "assign_ent_weight"], names
        assert names[1:8] == ["max_num_nodes", "input_dim", "hidden_dim", "embedding_dim", "label_dim", "num_layers",
                              "assign_hidden_dim"]
        assert list(inspect.signature(cls.loss).parameters) == ["self", "pred", "label", "adj", "batch_num_nodes",
                                                                "adj_hop"]


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
@pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)")
def test_entropy_kernels_use_no_scratch_and_do_not_spill():
    res = KR.kernel_resources(LIB)
    ks = {d["name"]: d for d in res.values() if d["name"].startswith("k_assign_ent_")}
    for stem in ("k_assign_ent_fwd<", "k_assign_ent_bwd<"):
        assert len([k for k in ks if k.startswith(stem)]) == 6, sorted(ks)       # 4 / 16 / 64 lanes x 4- / 16-byte
    assert "k_assign_ent_finish" in ks, sorted(ks)
    for d in ks.values():
        assert d["scratch"] == 0, d
        assert d["vgpr_spills"] == 0, d
        assert d["vgprs"] <= 64, d            # 8 waves per SIMD: the stream hides its latency by occupancy


# ---- the bound tells defects from rounding (numpy only)
def _near_uniform(B, n, K, seed):
    rng = np.random.default_rng(seed)
    return AC.softmax_rows(rng, B, n, K, scale=0.5)          # masked rows hold valid rows too: a leak is visible


@pytest.mark.parametrize("shape", AC.FAULT_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fault", AC.FAULTS)
def test_the_forward_bound_tells_each_defect_from_rounding(shape, fault):
    B, n, K = shape
    assert B * n <= 64 and K <= 64
    S = _near_uniform(B, n, K, seed=B * 10007 + n * 101 + K)
    seen = 0
    for mask in AC.MASKS:
        nn = AC.num_nodes(mask, B, n)
        bad = AC.faulty_entropy(S, nn, fault)
        if bad is None:
            continue
        e, mag = AC.entropy_ref(S, nn)
        seen += 1
        assert abs(bad - e) >= 10.0 * AC.fwd_bound(mag), (mask, bad, e, AC.fwd_bound(mag))
    if fault in ("last_column", "last_valid_row"):
        assert seen == len(AC.MASKS)
    elif fault == "quad_fourth_lane":
        assert seen == (len(AC.MASKS) if K % 4 else 0)
    elif n > 1:
        assert seen >= 1                      # the mask defects need a graph with n_b < n


def test_the_reference_is_the_definition():
    # s = 0 and s = 1: finite, 0 and 0 forward; gradients 34.5... and -1
    S = np.array([[[0.0, 1.0], [0.5, 0.5]]], dtype=np.float32)
    e, _ = AC.entropy_ref(S)
    assert e == pytest.approx(np.log(2.0) / 2.0, rel=1e-12)
    d, _ = AC.grad_ref(S, None, 1.0, 1.0)
    assert d[0, 0, 0] * 2 == pytest.approx(-np.log(float(np.float32(1e-15))), rel=1e-12)
    assert 34.5 < d[0, 0, 0] * 2 < 34.6 and d[0, 0, 1] * 2 == pytest.approx(-1.0, abs=1e-12)
    # rows past n_b do not count, whatever they hold; the normaliser is the valid rows
    S2 = np.concatenate([S, np.full((1, 2, 2), np.nan, dtype=np.float32)], axis=1)
    e2, _ = AC.entropy_ref(S2, np.array([2], dtype=np.int32))
    assert e2 == e
    d2, b2 = AC.grad_ref(S2, np.array([2], dtype=np.int32), 1.0, 1.0)
    assert (d2[0, 2:] == 0).all() and (b2[0, 2:] == 0).all() and np.array_equal(d2[0, :2], d[0])
