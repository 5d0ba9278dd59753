"""tests/linkpred_cases.py without a GPU: the restated plan equals dp_linkpred_plan on every row, the table covers every
class it is meant to, every qualifying input meets the condition the counted bound rests on, the direct fp32 formula
meets that bound through the GPU test's own comparison, and each planted defect violates it on the row built for it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import linkpred_cases as LC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _case(name):
    c = LC.by_name(name)
    inp = LC.build(c)
    return c, inp, LC.reference(c, inp)


def _lib_plan(lib, B, n, K):
    out = (C.c_int * _lib.LINKPRED_PLAN_INTS)()
    assert lib.dp_linkpred_plan(B, n, K, out) == 0
    return tuple(out)


def test_restated_plan_equals_the_library_on_every_row(lib):
    for shape, want in LC.PINNED_PLANS.items():
        assert LC.plan(*shape)[:5] == want == _lib_plan(lib, *shape)[:5], shape
    for c in LC.CASES:
        assert LC.plan(c.B, c.n, c.K) == _lib_plan(lib, c.B, c.n, c.K), c.name
    for B, n, K in LC.REFUSED:
        out = (C.c_int * _lib.LINKPRED_PLAN_INTS)()
        assert K == LC.K_MAX + 1 and lib.dp_linkpred_plan(B, n, K, out) == -3
    for B in (1, 2, 7, 8, 9, 20, 64, 171, 512, 513):           # the 512-workgroup rule around its edges
        for n in (1, 32, 33, 64, 65, 128, 129, 500, 1000):
            for K in (1, 176, 177, 256):
                assert LC.plan(B, n, K) == _lib_plan(lib, B, n, K), (B, n, K)


def test_table_covers_every_class():
    cs = LC.CASES
    assert len({c.name for c in cs}) == len(cs) <= 60
    keys = [c[1:] for c in cs]
    assert len(set(map(str, keys))) == len(cs), "two rows are the same class"
    Ks = {c.K for c in cs}
    assert set(LC.K_EDGES) <= Ks and len([K for K in Ks if K % 4 and K not in LC.K_EDGES]) >= 2
    assert {50, 150} <= Ks and LC.K_MAX in Ks and [K for _, _, K in LC.REFUSED] == [LC.K_MAX + 1]
    ns = {c.n for c in cs}
    assert set(LC.N_SIZES) <= ns and {n % 8 for n in ns} >= {0, 3, 4, 7}
    big = [c for c in cs if c.n > 330 or c.B > 64]
    assert len(big) == 3 and {c.name for c in big} == {"nonsplit64", "nonsplit64_acc", "nonsplit32"}
    # backward plans
    classes = {LC.plan_class(c.B, c.n, c.K) for c in cs}
    assert classes >= {"one_tile", "nonsplit_cw64", "nonsplit_cw32", "split_all_cw64", "split_all_cw32",
                       "split_even_cw64", "split_even_cw32", "split_ragged_cw64"}, classes
    p = LC.plan(60, 300, 50)
    assert p[2:5] == (5, 2, 3)                                    # 5 tiles as 3 + 2

    def beyond(c, split):                                         # a whole 64-row block beyond n_b, in that form
        return (LC.plan(c.B, c.n, c.K)[3] > 1) == split and any((nb + 63) // 64 < (c.n + 63) // 64 for nb in LC.node_counts(c))
    assert any(beyond(c, False) and c.acc == 0 for c in cs) and any(beyond(c, False) and c.acc == 1 for c in cs)
    assert any(beyond(c, True) and c.acc == 0 for c in cs) and any(beyond(c, True) and c.acc == 1 for c in cs)
    assert any(LC.plan(c.B, c.n, c.K)[3] > 1 and LC.plan(c.B, c.n, c.K)[4] * LC.plan(c.B, c.n, c.K)[1] >= nb > 0
               for c in cs for nb in LC.node_counts(c)), "no split lies wholly beyond n_b"
    # n_b
    assert any(c.nn is None for c in cs) and any(c.nn == "full" for c in cs)
    inner = {int(nb) for c in cs for nb in LC.node_counts(c) if nb < c.n}
    assert {0, 1, 63, 64, 65, 128} <= inner
    zero = [c for c in cs if 0 in LC.node_counts(c)]
    assert zero and all((LC.node_counts(c) > 0).any() for c in zero)
    # adjacency
    for kind in ("sym", "dir", "weighted", "quarter", "outside7"):
        assert any(c.adj == kind for c in cs), kind
    assert all(LC.readers(c) == (("f32",) if c.adj == "weighted" else ("f32", "packed")) for c in cs)
    assert any(c.padnan and "packed" in LC.readers(c) and c.n % 8 for c in cs)
    # values of P, scalars
    assert {c.skind for c in cs} == {"softmax", "ties", "grid", "sharp"}
    assert {c.dloss for c in cs} >= {None, 1.7, -0.6} and {c.acc for c in cs} == {0, 1}
    assert any(c.norm and c.via == "loss" for c in cs) and any(not c.norm and c.via == "loss" for c in cs)
    assert all(c.acc == 0 for c in cs if c.via == "loss")
    sharp = LC.by_name("sharp")
    assert (sharp.B, sharp.n, sharp.K) == (2, 256, 50) and not LC.qualifies(sharp)
    assert set(LC.FAULT_ROW) == set(LC.FAULTS)


def test_inputs_are_what_their_class_says():
    for c in LC.CASES:
        inp = LC.build(c)
        A, S, nnv = inp["A"], inp["S"], inp["nnv"]
        sym = bool((A == A.transpose(0, 2, 1)).all())
        assert sym == (c.adj not in ("dir", "outside7")), c.name
        vals = set(np.unique(A).tolist())
        if c.adj in ("sym", "dir", "sym_loops"):
            assert vals <= {0.0, 1.0}
        if c.adj == "quarter":
            assert vals == {0.0, 0.25, 0.5}
        if c.adj == "weighted":
            assert (A.view(np.uint32) & 0xFFFF).any() and A.max() < 1.0
        else:
            LC.pack(A, (c.n + 7) // 8 * 8, c.padnan)             # bf16-exact
        for b in range(c.B):
            nb = int(nnv[b])
            out = np.ones((c.n, c.n), bool)
            out[:nb, :nb] = False
            assert (A[b][out] == (7.0 if c.adj == "outside7" else 0.0)).all()
            assert (np.abs(S[b, nb:]).sum(axis=1) > 0).all(), "rows >= n_b of S are filled: only the mask keeps them out"


def test_qualifying_rows_meet_the_condition_and_ties_are_exact():
    for c in LC.CASES:
        if c.B > 64:
            continue                                               # the batch-heavy rows: in the fp32 test below
        _, inp, ref = _case(c.name)
        if LC.qualifies(c):
            assert ref["margin"] >= 64 * (c.K + 1) * LC.U, (c.name, ref["margin"])
        if c.skind == "ties":
            S = torch.from_numpy(inp["S"])
            raw32 = S[0] @ S[0].t()
            rows = list(LC.TIE_ROWS)
            assert (raw32[rows][:, rows] == 1.0).all() and ref["ties"] >= 16 * c.B
            a = inp["A"][0]
            assert a[0, 0] == 1 and a[1, 1] == 0 and a[0, 1] == 1 and a[5, 6] == 0
        if c.skind == "grid":
            assert ref["ties"] > 0 and ref["above"] > 0 and ref["below"] > 0 and ref["margin"] == float("inf")
            S = torch.from_numpy(inp["S"][0])
            assert torch.equal((S @ S.t()).double(), S.double() @ S.double().t())       # exact in fp32
        if c.K == 1:
            assert ref["below"] == 0 and ref["above"] == 0                              # all ties
    c, inp, ref = _case("sharp")
    assert ref["near"] <= 8 * LC.U, ref["near"]                    # some inexact p within 8 u of 1


WORST = {}


@pytest.mark.parametrize("name", [c.name for c in LC.CASES if LC.qualifies(c)])
def test_fp32_formula_meets_the_counted_bound(name):
    c = LC.by_name(name)
    inp = LC.build(c)
    ref = LC.reference(c, inp)
    assert ref["margin"] >= 64 * (c.K + 1) * LC.U, (c.name, ref["margin"])
    f32 = LC.reference(c, inp, dtype=torch.float32, bounds=False)
    old = LC.prior(c, ref) if c.acc else None
    got = LC.full_output(c, inp, f32, old)
    r = LC.compare(c, inp, ref, np.float32(f32["loss"]), got, old)
    WORST[name] = (r["fwd"], r["bwd"])
    print(f"[linkpred] {name}: fp32 formula at {r['fwd']:.4f} (loss) and {r['bwd']:.4f} (dS) of the counted bound")
    assert not r["problems"], r["problems"]
    # the correct fp64 result, rounded to fp32 once, passes too
    assert not LC.compare(c, inp, ref, np.float32(ref["loss"]), LC.full_output(c, inp, ref, old), old)["problems"]


@pytest.mark.parametrize("fault", LC.FAULTS)
def test_planted_defect_violates_the_bound(fault):
    c, inp, ref = _case(LC.FAULT_ROW[fault])
    old = LC.prior(c, ref) if c.acc else None
    if fault in ("block_unwritten", "block_zeroed"):
        assert c.acc == (fault == "block_zeroed") and LC.plan(c.B, c.n, c.K)[3] > 1
        got = LC.full_output(c, inp, ref, old)
        hit = 0
        for b in range(c.B):
            r0 = (int(inp["nnv"][b]) + 63) // 64 * 64
            hit += r0 < c.n
            got[b, r0:] = 0.0 if c.acc else np.nan
        assert hit
        loss = ref["loss"]
    else:
        bad = LC.reference(c, inp, fault=fault, bounds=False)
        got, loss = LC.full_output(c, inp, bad, old), bad["loss"]
    if fault == "a_for_at":
        assert c.adj == "dir"
    if fault == "norm_ignored":
        assert c.norm
    r = LC.compare(c, inp, ref, np.float32(loss), got, old)
    assert r["problems"], (fault, r)
