"""CPU checks of the packed-adjacency link-prediction loss at the C boundary: the four entries are declared in
include/diffpool_hip.h, exported by the library and bound in _lib with the header's argument kinds, and they check their
arguments before any launch; and CapturedTrainStep's linkpred flag.  No compute call is made (numerics:
tests/test_gpu_linkpred_packed.py)."""
import ctypes as C
import os
import re

import pytest

from graph_pooling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffpool_hip.h")

PACKED_ENTRIES = ("dp_linkpred_loss_fwd_packed", "dp_linkpred_loss_bwd_packed", "dp_loss_forward_packed",
                  "dp_loss_backward_packed")
# each packed entry is its fp32 twin with `const float* adj` replaced by the packed rows of A (and of A^T)
TWINS = {"dp_linkpred_loss_fwd_packed": ("dp_linkpred_loss_fwd", ["const void* adj_pk"]),
         "dp_linkpred_loss_bwd_packed": ("dp_linkpred_loss_bwd", ["const void* adj_pk", "const void* adj_pkt"]),
         "dp_loss_forward_packed": ("dp_loss_forward", ["const void* adj_pk", "const void* adj_pkt"]),
         "dp_loss_backward_packed": ("dp_loss_backward", ["const void* adj_pk", "const void* adj_pkt"])}


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(dp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        out[m.group(2)] = (m.group(1), [" ".join(a.split()) for a in m.group(3).split(",")])
    return out


def _kind(decl):
    d = decl.replace("const ", "").strip()
    if "*" in d:
        return "ptr"
    return " ".join(d.split()[:-1])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_packed_link_entries_are_declared_and_mirror_the_fp32_ones():
    decl = _declarations()
    for name in PACKED_ENTRIES:
        assert name in decl, f"{name} is not declared in diffpool_hip.h"
        twin, adj_args = TWINS[name]
        ret, args = decl[name]
        tret, targs = decl[twin]
        assert ret == tret == "int"
        i = targs.index("const float* adj")
        assert args == targs[:i] + adj_args + targs[i + 1:], name


def test_packed_link_entries_are_exported_and_bound(lib):
    raw = C.CDLL(_lib.LIB_PATH)
    cmap = {C.c_int: "int", C.c_long: "long", C.c_float: "float", C.c_size_t: "size_t", C.c_void_p: "ptr"}
    decl = _declarations()
    for name in PACKED_ENTRIES:
        assert hasattr(raw, name), f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.EXPORTED_SYMBOLS
        res, argtypes = _lib._PROTOS[name]
        assert res is C.c_int
        _, args = decl[name]
        assert [cmap[t] for t in argtypes] == [_kind(a) for a in args], name


def test_captured_train_step_takes_a_linkpred_model_only_with_linkpred_true():
    """CapturedTrainStep(..., linkpred=True) is how a linkpred model is captured; the flag and the model must agree,
    and the device-counted optimizer is needed either way.  All of it is checked before anything touches a GPU, so
    this runs on any host (a call that passes the checks would go on to capture, so none is made here)."""
    import numpy as np
    from graph_pooling_amd.batch_builder import DeviceBatchBuilder, EdgeListDataset
    from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
    from graph_pooling_amd.optim import FusedClipAdam
    from graph_pooling_amd.train_step import CapturedTrainStep
    from graph_pooling_amd.tu_dataset import TUGraph
    a = np.zeros((3, 3), dtype=np.float32)
    a[0, 1] = a[1, 0] = 1
    ds = EdgeListDataset.from_tu_graphs([TUGraph(a, np.zeros(3, dtype=np.int64), 0)] * 4)
    builder = DeviceBatchBuilder(ds, 64, 2, "cpu")
    for linkpred in (False, True):
        model = SoftPoolingGcnEncoder(64, 2, 4, 4, 2, 3, 4, assign_ratio=0.25, linkpred=linkpred)
        with pytest.raises(ValueError, match="device_step_counter"):
            CapturedTrainStep(model, FusedClipAdam(model), builder, 2, linkpred=linkpred)
        with pytest.raises(ValueError, match="disagree"):
            CapturedTrainStep(model, FusedClipAdam(model, device_step_counter=True), builder, 2,
                              linkpred=not linkpred)


def test_packed_entries_check_their_arguments_before_any_launch(lib):
    """NULL A^T rows and packed rows that are not 16-byte aligned (the kernels read them 16 bytes at a time) are argument
    errors; the entries return before anything is enqueued, so this runs on any host (the addresses are never read)."""
    S, out, dS = 0x10000, 0x20000, 0x30000
    pk, pkt = 0x40000, 0x50000
    B, n, K = 2, 64, 8
    assert lib.dp_linkpred_loss_bwd_packed(S, pk, None, None, None, dS, 0, B, n, K, None, 0, None) == -1
    assert b"adj_pkt" in lib.dp_last_error_string()
    assert lib.dp_linkpred_loss_fwd_packed(S, pk + 2, None, out, B, n, K, None, 0, None) == -1
    assert b"aligned" in lib.dp_last_error_string()
    assert lib.dp_linkpred_loss_bwd_packed(S, pk, pkt + 8, None, None, dS, 0, B, n, K, None, 0, None) == -1
    assert lib.dp_loss_forward_packed(0x60000, 0x70000, S, pk, None, None, None, out, 0x80000, None, B, 2, n, K, 1,
                                      None, 0, None) == -1
    assert b"linkpred needs" in lib.dp_last_error_string()
    assert lib.dp_loss_backward_packed(0x80000, 0x70000, S, pk + 4, pkt, None, None, None, None, dS, B, 2, n, K, 1,
                                       None, 0, None) == -1
