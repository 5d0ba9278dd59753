"""The host layer of the CSR ops and modules that `tests/test_csr_host_cpu.py` does not reach — SDDMM, edge softmax,
symmetric normalisation, GAT attention, GAT convolution, sampled mean, top-k pooling; `EdgeAttention`, `GatConv`,
`SageConv`, `TopKPooling` — without a GPU and without the library, on that module's fake (`fake_lib`, `FakeLib`,
`misplaced` are imported from it, not copied).

(a) What the wrappers pass: every parameter named like a container field, `mirror` (-> `mirror_perm`) included, receives
    that field's address, for undirected / directed and 0/1 / weighted graphs and batches.  The two launches that walk
    the transposed CSR through parameters named `indptr` / `indices` (the dQ gather of the SDDMM backward, the second
    induce of a directed container) are checked against the transposed fields.  The substitute of an edgeless
    `CsrGraph` (`indptr` where the never-read `indices` would be NULL) has a test of its own.
(b) What they launch: the sequence of (entry, every non-pointer argument) of one forward + backward of each case equals
    tests/golden/csr_ops_host_calls.json, recorded with this module on the commit before the containers moved to
    `csr.py`.  To record: copy this file into a checkout of that commit and run
    `python -m tests.test_csr_ops_host_cpu > tests/golden/csr_ops_host_calls.json` there.

`csr_topk_pool` reads `indptr_out[-1]` back, which under the fake is uninitialised memory: this module's fake zero-fills
`indptr_out` of dp_csr_topk_induce, as `FakeLib` writes `counts_host` of dp_csr_pool_batch_plan."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, EdgeAttention, GatConv, SageConv, TopKPooling
from tests.test_csr_host_cpu import FakeLib, _ring_edges, _ring_graph, fake_lib, misplaced

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csr_ops_host_calls.json")
SEED = (1 << 63) + 12345          # at least 2^63: the entries take it as the signed word -(2^63) + 12345
# entries without a `_w` twin (dp_csr_aggregate_w is the SDDMM backward's gather whatever the container stores)
UNPAIRED = ("dp_csr_sddmm", "dp_csr_aggregate_w", "dp_csr_edge_softmax", "dp_csr_sym_norm", "dp_csr_gat", "dp_csr_sample_mean",
            "dp_csr_topk", "dp_bgemm")
# entries whose `values` parameter is an operand of the op (scores, a gradient), not the container's field
OPERAND_VALUES = ("dp_csr_aggregate_w", "dp_csr_sym_norm_fwd", "dp_csr_sym_norm_bwd")


class ZeroingLib(FakeLib):
    """`FakeLib` whose dp_csr_topk_induce zero-fills `indptr_out` (n_out + 1 ints): the wrapper reads its last one."""

    def __getattr__(self, name):
        entry = super().__getattr__(name)
        if name != "dp_csr_topk_induce":
            return entry
        names = self.protos[name][0]

        def induce(*args):
            a = dict(zip(names, args))
            C.memset(a["indptr_out"], 0, 4 * (a["n_out"] + 1))
            return entry(*args)
        return induce


def zeroing_lib(setattr_):
    """`fake_lib` with the library replaced by a `ZeroingLib`."""
    fake_lib(setattr_)
    lib = ZeroingLib()
    setattr_(_lib, "load", lambda: lib)
    return lib


# ------------------------------------------------------------------ containers and cases
def _ring_batch(directed, weighted):
    """The 7 + 5 ring batch padded to 9; weights on the first graph only: the second gets ones."""
    (s7, d7), (s5, d5) = _ring_edges(7), _ring_edges(5)
    w = np.arange(1, 8, dtype=np.float32) / 4 if weighted else None
    return CsrBatch.from_edge_lists([7, 5], [s7, s5], [d7, d5], "cpu", symmetric=not directed, pad_to=9, weights=[w, None])


CONTAINERS = {f"{kind}-{'directed' if d else 'undirected'}-{'weighted' if w else '01'}": (make, d, w)
              for kind, make in (("graph", _ring_graph), ("batch", _ring_batch)) for d in (False, True) for w in (False, True)}
EDGELESS = {"graph-edgeless": lambda: CsrGraph.from_edges(4, [], [], "cpu"),
            "batch-edgeless": lambda: CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")}


def _leaf(*shape):
    return torch.rand(*shape, requires_grad=True)


def _back(out):
    if out.requires_grad:
        out.sum().backward()


def _sample(num_sample, self_mode, some):
    def run(g):
        nodes = torch.tensor([g.n - 1, 0, 2], dtype=torch.int32) if some else None
        _back(ops.csr_sample_mean(_leaf(g.n, 3), g, num_sample, SEED, nodes, self_mode))
    return run


def _topk(with_gate, **count):
    def run(g):
        gate = _leaf(g.n) if with_gate else None
        _back(ops.csr_topk_pool(_leaf(g.n, 3), torch.rand(g.n), g, gate=gate, **count)[0])
    return run


def _attention(**kw):
    return lambda g: _back(EdgeAttention(3, 4, **kw)(torch.rand(g.n, 3), g).values)


OP_CASES = {
    "sddmm-alpha1": lambda g: _back(ops.csr_sddmm(_leaf(g.n, 3), _leaf(g.n, 3), g)),
    "sddmm-alpha0.5": lambda g: _back(ops.csr_sddmm(_leaf(g.n, 3), _leaf(g.n, 3), g, 0.5)),
    "edge-softmax": lambda g: _back(ops.csr_edge_softmax(_leaf(g.nnz), g)),
    "sym-normalize-values": lambda g: _back(ops.csr_sym_normalize(_leaf(g.nnz), g)),
    "sym-normalize-none": lambda g: _back(ops.csr_sym_normalize(None, g)),
    "gat-attention": lambda g: _back(ops.csr_gat_attention(_leaf(g.n, 3), _leaf(g.n, 3), g)),
    "gat-conv-concat": lambda g: _back(ops.csr_gat_conv(_leaf(g.n, 6), _leaf(g.n, 2), _leaf(g.n, 2), g, 2, concat=True)),
    "gat-conv-mean": lambda g: _back(ops.csr_gat_conv(_leaf(g.n, 6), _leaf(g.n, 2), _leaf(g.n, 2), g, 2, concat=False)),
    **{f"sample-{'all' if k is None else k}-{mode}-{'some' if some else 'every'}": _sample(k, mode, some)
       for k in (2, None) for mode in ("none", "gcn", "concat") for some in (False, True)},
    "topk-ratio": _topk(False, ratio=0.5),
    "topk-ratio-gate": _topk(True, ratio=0.5),
    "topk-k": _topk(False, k=2),
    "topk-k-gate": _topk(True, k=2),
    "EdgeAttention-softmax-dot": _attention(norm="softmax"),
    "EdgeAttention-sym-dot": _attention(norm="sym"),
    "EdgeAttention-softmax-additive": _attention(norm="softmax", score="additive", heads=2),
    "GatConv": lambda g: _back(GatConv(3, 3, heads=2)(torch.rand(g.n, 3), g)),
    "SageConv": lambda g: _back(SageConv(3, 4, num_sample=2)(torch.rand(g.n, 3), g, seed=SEED)),
    "TopKPooling-proj": lambda g: _back(TopKPooling(3, 0.5, "proj")(torch.rand(g.n, 3), g)[0]),
    "TopKPooling-gcn": lambda g: _back(TopKPooling(3, 0.5, "gcn")(torch.rand(g.n, 3), g)[0]),
}
EDGELESS_CASES = {"sample-2-gcn-every": OP_CASES["sample-2-gcn-every"], "topk-ratio-gate": OP_CASES["topk-ratio-gate"]}


def _make(container):
    if container in EDGELESS:
        return EDGELESS[container](), EDGELESS_CASES
    make, directed, weighted = CONTAINERS[container]
    return make(directed, weighted), OP_CASES


def record_op_calls(setattr_, container):
    """{case: ([entry, {non-pointer parameter: value}] of one forward + backward, the calls with their pointers)} of
    every case of a container, and the container."""
    lib = zeroing_lib(setattr_)
    torch.manual_seed(0)
    g, cases = _make(container)
    out = {}
    for case, run in cases.items():
        del lib.calls[:]
        run(g)
        out[case] = (lib.scalars(), list(lib.calls))
    return out, g


# ------------------------------------------------------------------ (a) every field lands in the parameter of its name
def _transposed(g):
    """The view of `g` that a launch over the transposed CSR sees in the parameters of the forward names."""
    t = copy.copy(g)
    t.indptr, t.indices, t.indptr_t, t.indices_t = g.indptr_t, g.indices_t, g.indptr, g.indices
    return t


def placed(calls, g):
    """`misplaced` for the ops of this module, plus `mirror` -> `mirror_perm`.  [] when every call is right."""
    bad, seen = [], {}
    for name, args in calls:
        nth = seen[name] = seen.get(name, 0) + 1
        over_t = nth == 2 and name in ("dp_csr_aggregate_w", "dp_csr_topk_induce")      # dQ; the induce of A^T
        shown = {p: v for p, v in args.items() if not (p == "values" and name in OPERAND_VALUES)}
        found = misplaced([(name, shown)], _transposed(g) if over_t else g)
        bad += [m for m in found if not (name.startswith(UNPAIRED) and m == f"{name}: weighted = {g.weighted}")]
        if "mirror" in args:
            null_ok = name == "dp_csr_sym_norm_fwd" and g.indices_t is g.indices      # its own order serves
            if not (args["mirror"] is None and null_ok) and args["mirror"] != g.mirror_perm.data_ptr():
                bad.append(f"{name}: parameter mirror did not get {type(g).__name__}.mirror_perm")
    return bad


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_record_holds_every_case(recorded):
    want = [f"{c}/{case}" for c in CONTAINERS for case in OP_CASES] + [f"{c}/{case}" for c in EDGELESS
                                                                         for case in EDGELESS_CASES]
    assert sorted(recorded) == sorted(want)


@pytest.mark.parametrize("container", sorted(CONTAINERS))
def test_ops_launch_what_the_golden_record_says_with_every_field_in_place(monkeypatch, recorded, container):
    got, g = record_op_calls(monkeypatch.setattr, container)
    _, directed, weighted = CONTAINERS[container]
    assert g.weighted == weighted and (g.indices_t is g.indices) != directed
    seen = set()
    for case, (scalars, calls) in got.items():
        assert scalars and scalars == recorded[f"{container}/{case}"], case
        assert placed(calls, g) == [], case
        seen |= {p for _, args in calls for p in args}
    assert {"indptr", "indices", "indptr_t", "indices_t", "mirror", "node_off"} <= seen


@pytest.mark.parametrize("container", sorted(EDGELESS))
def test_an_edgeless_container_launches_what_the_golden_record_says(monkeypatch, recorded, container):
    """The sampled mean under 'gcn' and the top-k pooling launch on a container without entries.  A CsrBatch hands over
    its one-element pad; a CsrGraph, whose `indices` is empty, `indptr` in its place: never read, never NULL."""
    got, g = record_op_calls(monkeypatch.setattr, container)
    assert g.nnz == 0
    for case, (scalars, calls) in got.items():
        assert scalars and scalars == recorded[f"{container}/{case}"], case
        if container == "batch-edgeless":
            assert g.indices.numel() == 1 and placed(calls, g) == [], case
            continue
        assert g.indices.numel() == 0
        by = {}
        for name, args in calls:
            by.setdefault(name, []).append(args)
        if case.startswith("sample"):
            (fwd,), (bwd,) = by["dp_csr_sample_mean_fwd"], by["dp_csr_sample_mean_bwd"]
            assert fwd["indptr"] == g.indptr.data_ptr() and fwd["indices"] == g.indptr.data_ptr()
            assert bwd["indptr_t"] == g.indptr_t.data_ptr() and bwd["indices_t"] == g.indptr_t.data_ptr()
        else:
            (induce,) = by["dp_csr_topk_induce"]
            assert induce["indptr"] == g.indptr.data_ptr() and induce["indices"] == g.indptr.data_ptr()
            assert (induce["nnz"], induce["cap"]) == (0, 1)


def test_the_checker_reports_indices_passed_for_indices_t(monkeypatch):
    """Negative control: a wrapper handed a view of a directed graph whose `indices` and `indices_t` are swapped passes
    each where the other belongs, and `placed` says so; so it does for a view with another `mirror_perm`."""
    lib = zeroing_lib(monkeypatch.setattr)
    g = _ring_graph(directed=True, weighted=False)
    view = copy.copy(g)
    view.indices, view.indices_t = g.indices_t, g.indices
    view.__dict__["mirror_perm"] = g.mirror_perm.clone()
    _back(ops.csr_gat_attention(_leaf(5, 3), _leaf(5, 3), view))
    bad = placed(lib.calls, g)
    assert "dp_csr_gat_fwd: parameter indices did not get CsrGraph.indices" in bad
    assert "dp_csr_gat_bwd: parameter indices_t did not get CsrGraph.indices_t" in bad
    assert "dp_csr_gat_bwd: parameter mirror did not get CsrGraph.mirror_perm" in bad
    assert placed(lib.calls, view) == []


if __name__ == "__main__":
    with pytest.MonkeyPatch.context() as mp:
        cases = {f"{c}/{case}": scalars for c in list(CONTAINERS) + list(EDGELESS)
                 for case, (scalars, _) in record_op_calls(mp.setattr, c)[0].items()}
    print("{\n" + ",\n".join(f'"{case}": [\n' + ",\n".join(" " + json.dumps(c) for c in calls) + "\n]"
                             for case, calls in cases.items()) + "\n}")      # one call per line
