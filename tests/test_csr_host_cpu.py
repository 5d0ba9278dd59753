"""The host layer of the CSR path, without a GPU and without the library: `_lib.load` is replaced by a fake that takes
every entry's parameter names from include/diffpool_hip.h, checks the argument count and records each call that has a
`stream` parameter; `_lib.require_gpu_tensor` and `_lib.current_stream` are switched off, so the ops and the model
classes run forward and backward on CPU tensors (outputs are uninitialised memory: only the calls are looked at).

(a) What the wrappers pass: every parameter named like a container field (indptr, indices, values, their `_t` and
    `_local` forms, node_off) receives that field's address, for undirected / directed and 0/1 / weighted graphs and
    batches, and the `_w` entry is taken exactly when the container is weighted and the entry takes an adjacency.
(b) What the models launch: the sequence of (entry, every non-pointer argument) of one forward + loss + backward of
    each model class equals tests/golden/csr_host_calls.json, recorded with this module's recorder on the commit
    before the host layer was refactored.  To record: copy this file into a checkout of that commit and run
    `python -m tests.test_csr_host_cpu > tests/golden/csr_host_calls.json` there."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import (CsrBatch, CsrGraph, SparseBatchGcnEncoderGraph, SparseGcnSet2SetEncoder,
                                      SparseSoftPoolingGcnEncoder)
from tests.test_abi_cpu import _header_functions, _kind

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csr_host_calls.json")
FIELDS = ("indptr", "indices", "values", "indptr_t", "indices_t", "values_t", "indices_local", "indices_t_local",
          "node_off")


class FakeLib:
    """Stands in for the ctypes library: any dp_* entry of the header, called with the header's argument count, returns
    0 (a `*_bytes` query: 256; dp_csr_pool_batch_plan also writes counts = (1, 1)).  `calls` holds (entry, {parameter:
    argument}) of every call with a `stream` parameter, in order."""

    def __init__(self):
        self.protos = {name: ([a.split()[-1].lstrip("*") for a in args], [_kind(a) for a in args])
                       for name, (_, args) in _header_functions().items()}
        self.calls = []

    def __getattr__(self, name):
        if name not in self.__dict__.get("protos", ()):
            raise AttributeError(name)
        names = self.protos[name][0]

        def entry(*args):
            assert len(args) == len(names), f"{name}: {len(args)} arguments for {len(names)} parameters"
            if name.endswith("_bytes"):
                return 256
            if name == "dp_csr_pool_batch_plan":
                (C.c_int * 2).from_address(args[names.index("counts_host")])[:] = (1, 1)
            if "stream" in names:
                self.calls.append((name, dict(zip(names, args))))
            return 0
        return entry

    def scalars(self):
        """The recorded calls as [entry, {parameter: value}] with the pointer parameters left out."""
        out = []
        for name, args in self.calls:
            kinds = dict(zip(*self.protos[name]))
            out.append([name, {p: float(v) if kinds[p] == "float" else int(v)
                               for p, v in args.items() if kinds[p] != "ptr"}])
        return out


def fake_lib(setattr_):
    """Patch `_lib` (and nothing else) through a monkeypatch-style `setattr_`; returns the recording library."""
    lib = FakeLib()
    setattr_(_lib, "load", lambda: lib)
    setattr_(_lib, "require_gpu_tensor", lambda t, name: None)
    setattr_(_lib, "current_stream", lambda: 0)
    return lib


# ------------------------------------------------------------------ (a) every field lands in the parameter of its name
def _ring_edges(n):
    src = np.arange(n)
    return src, (src + 1) % n


def _ring_graph(directed, weighted):
    src, dst = _ring_edges(5)
    w = np.arange(1, 6, dtype=np.float32) / 4 if weighted else None
    return CsrGraph.from_edges(5, src, dst, "cpu", symmetric=not directed, weight=w)


def _ring_batch(directed, weighted):
    src, dst = _ring_edges(5)
    w = np.arange(1, 6, dtype=np.float32) / 4 if weighted else None      # the first graph only: the second gets ones
    return CsrBatch.from_edge_lists([5, 5], [src, src], [dst, dst], "cpu", symmetric=not directed, weights=[w, None])


def misplaced(calls, g):
    """What is wrong with the recorded calls of ops that ran on container `g`: a field in a parameter of another name,
    or the wrong one of an entry pair.  [] when every call is right."""
    bad = []
    undirected = g.indices_t is g.indices
    for name, args in calls:
        if name.endswith("_w") != (g.weighted and "indptr" in args):
            bad.append(f"{name}: weighted = {g.weighted}")
        for p in FIELDS:
            if p not in args:
                continue
            if args[p] is None and undirected and name.startswith("dp_csr_frob_link") and p.endswith("_t"):
                continue              # the Frobenius forward takes NULL for the transposed group of an undirected graph
            if args[p] != getattr(g, p).data_ptr():
                bad.append(f"{name}: parameter {p} did not get {type(g).__name__}.{p}")
    return bad


def _leaf(*shape):
    return torch.rand(*shape, requires_grad=True)


def _run_ops(g):
    """Forward and backward of every CSR op that takes container `g`; returns the entries it should have called,
    without the `_w`."""
    x, wt, b = _leaf(g.n, 3), _leaf(3, 4), _leaf(4)
    ops.csr_graph_conv(x, wt, b, g, _lib.F_NORMALIZE).sum().backward()
    s, z = _leaf(g.n, 2), _leaf(g.n, 4)
    batch = isinstance(g, CsrBatch)
    xp, ap = ops.csr_pool_batch(s, z, g) if batch else ops.csr_pool(s, z, g)
    (xp.sum() + ap.sum()).backward()
    (ops.csr_link_loss_batch(_leaf(g.n, 2), g) if batch else ops.csr_link_loss(_leaf(g.n, 2), g)).backward()
    ops.frob_link_loss(_leaf(g.n, 2), g).backward()
    mid = "_batch" if batch else ""
    return ["dp_sparse_gcn_layer_fwd", "dp_sparse_gcn_layer_bwd", f"dp_csr_pool{mid}_fwd", f"dp_csr_pool{mid}_bwd",
            f"dp_csr_linkpred{mid}_loss_fwd", f"dp_csr_linkpred{mid}_loss_bwd", f"dp_csr_frob_link{mid}_fwd",
            f"dp_csr_frob_link{mid}_bwd"]


@pytest.mark.parametrize("weighted", [False, True], ids=["01", "weighted"])
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("make", [_ring_graph, _ring_batch], ids=["graph", "batch"])
def test_every_container_field_lands_in_the_parameter_of_its_name(monkeypatch, make, directed, weighted):
    lib = fake_lib(monkeypatch.setattr)
    g = make(directed, weighted)
    assert g.weighted == weighted and (g.indices_t is g.indices) != directed
    want = _run_ops(g)
    sfx = "_w" if weighted else ""
    want = [n + (sfx if "frob_link" not in n or n.endswith("_fwd") else "") for n in want]      # that backward reads no adjacency
    assert [name for name, _ in lib.calls] == want
    assert misplaced(lib.calls, g) == []
    seen = {p for _, args in lib.calls for p in args if p in FIELDS}      # no field of the container went unchecked
    assert seen == {p for p in FIELDS if ("values" not in p or weighted) and (p in FIELDS[:6] or make is _ring_batch)}


def test_the_checker_reports_values_passed_for_values_t(monkeypatch):
    """Negative control: a wrapper handed a view of a directed weighted graph whose `values` and `values_t` are swapped
    passes each where the other belongs, and `misplaced` says so."""
    lib = fake_lib(monkeypatch.setattr)
    g = _ring_graph(directed=True, weighted=True)
    view = copy.copy(g)
    view.values, view.values_t = g.values_t, g.values
    xp, ap = ops.csr_pool(_leaf(5, 2), _leaf(5, 4), view)
    (xp.sum() + ap.sum()).backward()
    bad = misplaced(lib.calls, g)
    assert "dp_csr_pool_fwd_w: parameter values did not get CsrGraph.values" in bad
    assert "dp_csr_pool_bwd_w: parameter values_t did not get CsrGraph.values_t" in bad
    assert misplaced(lib.calls, view) == []


def test_a_graph_builds_its_batch_of_one_offsets_on_first_use():
    g = _ring_graph(directed=False, weighted=False)
    assert not {"node_off", "node_off_host"} & set(vars(g))          # constructing a graph copies nothing more
    assert (g.num_graphs, g.pad_to) == (1, 5)
    assert g.node_off_host.dtype == np.int32 and g.node_off_host.tolist() == [0, 5]
    assert g.node_off.dtype == torch.int32 and g.node_off.tolist() == [0, 5]
    assert g.node_off is g.node_off and g.node_off_host is g.node_off_host


# ------------------------------------------------------------------ (b) same launches, same scalars
def _norm_graph():
    return CsrGraph.from_edges(7, *_ring_edges(7), "cpu").normalized()


def _norm_batch(pad_to=None):
    (s7, d7), (s5, d5) = _ring_edges(7), _ring_edges(5)
    return CsrBatch.from_edge_lists([7, 5], [s7, s5], [d7, d5], "cpu", pad_to=pad_to).normalized()


def _diffpool(objective):
    return lambda: SparseSoftPoolingGcnEncoder(8, 3, 4, 4, 2, 3, 4, assign_ratio=0.5, num_pooling=1, linkpred=objective,
                                               assign_ent_weight=0.1)


MODEL_CASES = {
    "diffpool-bce-graph": (_diffpool("bce"), _norm_graph, True),
    "diffpool-bce-batch": (_diffpool("bce"), _norm_batch, True),
    "diffpool-frobenius-graph": (_diffpool("frobenius"), _norm_graph, True),
    "diffpool-frobenius-batch": (_diffpool("frobenius"), _norm_batch, True),
    "set2set-graph": (lambda: SparseGcnSet2SetEncoder(3, 4, 4, 2, 3), _norm_graph, False),
    "set2set-batch": (lambda: SparseGcnSet2SetEncoder(3, 4, 4, 2, 3), _norm_batch, False),
    "base-graph": (lambda: SparseBatchGcnEncoderGraph(3, 4, 4, 2, 3), _norm_graph, False),
    "base-batch": (lambda: SparseBatchGcnEncoderGraph(3, 4, 4, 2, 3), _norm_batch, False),
    "base-batch-padded": (lambda: SparseBatchGcnEncoderGraph(3, 4, 4, 2, 3), lambda: _norm_batch(pad_to=9), False),
}


def record_model_calls(setattr_, case):
    """[entry, {non-pointer parameter: value}] of one forward, loss and backward of a model case, in launch order."""
    make_model, make_graph, loss_takes_graph = MODEL_CASES[case]
    lib = fake_lib(setattr_)
    torch.manual_seed(0)
    model, g = make_model(), make_graph()
    nb = g.num_graphs if isinstance(g, CsrBatch) else 1
    pred = model(torch.rand(g.n, 3), g)
    label = torch.arange(nb) % 2
    loss = model.loss(pred, label, g) if loss_takes_graph else model.loss(pred, label)
    loss.backward()
    return lib.scalars()


@pytest.mark.parametrize("case", sorted(MODEL_CASES))
def test_models_launch_what_the_golden_record_says(monkeypatch, case):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(MODEL_CASES)
    got = record_model_calls(monkeypatch.setattr, case)
    assert len(got) > 10
    assert got == golden[case]


if __name__ == "__main__":
    with pytest.MonkeyPatch.context() as mp:
        cases = {case: record_model_calls(mp.setattr, case) for case in sorted(MODEL_CASES)}
    print("{\n" + ",\n".join(f'"{case}": [\n' + ",\n".join(" " + json.dumps(c) for c in calls) + "\n]"
                             for case, calls in cases.items()) + "\n}")      # one call per line
