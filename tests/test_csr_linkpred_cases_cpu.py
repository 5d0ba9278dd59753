"""tests/csr_linkpred_cases.py without a GPU: the restated plan equals dp_csr_linkpred_plan on every row and on a grid,
the refusals; the table covers every K tier edge, forward and backward walk class, edge form, scalar-form reason,
adjacency and S kind it is meant to (asserted from the library's plan entry and the built inputs, so that a deleted row
fails here); every row qualifies for the counted bound and the direct fp32 formula meets it; and each planted defect,
emulated as the wrong answer it would give, violates the bound on the row named for it."""
import ctypes as C
import os

import numpy as np
import pytest

from graph_pooling_amd import _lib
from tests import csr_linkpred_cases as CC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _lib_plan(lib, *args):
    out = (C.c_int * _lib.CSR_LINKPRED_PLAN_INTS)()
    assert lib.dp_csr_linkpred_plan(*args, out) == 0, lib.dp_last_error_string()
    return CC.Plan(*out)


@pytest.fixture(scope="module")
def plans(lib):
    """{row name: [the library's plan of each graph]}"""
    return {c.name: [_lib_plan(lib, *a) for a in CC.plan_args(c)] for c in CC.CASES}


def test_restated_plan_equals_the_library(lib, plans):
    assert len(CC.PLAN_FIELDS) == _lib.CSR_LINKPRED_PLAN_INTS
    for c in CC.CASES:
        assert plans[c.name] == CC.graph_plans(c), c.name
    for n in (1, 16, 17, 32, 33, 64, 65, 128, 129, 1024, 1025, 1472, 1473, 1536, 1537, 2880, 2881, 5748, 32704, 32705,
              65536):
        for K in (1, 4, 16, 17, 20, 64, 65, 128, 132, 176, 177, 256):
            for pad, s_mis, ds_mis in ((0, 0, 0), (3, 0, 0), (4, 1, 0), (4, 0, 1), (1, 1, 1)):
                for dpad in (0, 2):
                    args = (n, K, K + pad, K + pad + dpad, s_mis, ds_mis)
                    assert _lib_plan(lib, *args) == CC.plan(*args), args
    # pinned: DD's largest graph at K = 50; the first non-split multi-tile size; the first two-tile forward walk
    assert tuple(_lib_plan(lib, 5748, 50, 50, 50, 0, 0)) == (4, 90, 45, 23, 1035, 360, 64, 90, 6, 15, 1, 4, 1, 4,
                                                            4 * 2 * 64 * 66, 4 * (128 * 66 + 64 * 68))
    assert _lib_plan(lib, 32704, 8, 8, 8, 0, 0).splits == 2 and _lib_plan(lib, 32705, 8, 8, 8, 0, 0).splits == 1
    assert _lib_plan(lib, 2880, 8, 8, 8, 0, 0)[1:4] == (45, 23, 45) and _lib_plan(lib, 2881, 8, 8, 8, 0, 0)[1:4] == (46, 23, 45)


def test_plan_refusals(lib):
    assert "dp_csr_linkpred_plan" in _lib.EXPORTED_SYMBOLS
    out = (C.c_int * _lib.CSR_LINKPRED_PLAN_INTS)()
    assert lib.dp_csr_linkpred_plan(100, CC.REFUSED_K, 257, 257, 0, 0, out) == -3
    assert b"K=257" in lib.dp_last_error_string() and b"max 256" in lib.dp_last_error_string()
    assert lib.dp_csr_linkpred_plan(100, CC.K_MAX, 256, 256, 0, 0, out) == 0 and out[0] == 16
    for bad, text in (((0, 8, 8, 8), b"n=0 must be positive"), ((-3, 8, 8, 8), b"n=-3 must be positive"),
                      ((100, 0, 8, 8), b"K=0 must be positive"), ((100, 8, 7, 8), b"lds=7 smaller than K=8"),
                      ((100, 8, 8, 7), b"ldds=7 smaller than K=8")):
        assert lib.dp_csr_linkpred_plan(*bad, 0, 0, out) == -1 and text in lib.dp_last_error_string(), bad
    assert lib.dp_csr_linkpred_plan(100, 8, 8, 8, 0, 0, None) == -1 and b"plan_out is NULL" in lib.dp_last_error_string()


def test_table_covers_every_class(plans):
    cs = CC.CASES
    assert len({c.name for c in cs}) == len(cs) <= 48
    assert set(CC.FAULT_ROW) == set(CC.FAULTS) and all(CC.by_name(r) for r in CC.FAULT_ROW.values())
    every = [(c, p, n) for c in cs for p, n in zip(plans[c.name], c.sizes)]          # (row, library plan, n) per graph
    single = [(c, plans[c.name][0]) for c in cs if not c.batch]
    # K tiers: both edges of every KT, each tier seen by the library as that tier
    assert set(CC.K_EDGES) <= {c.K for c in cs}
    want_kt = dict(zip(CC.K_EDGES, (1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 12, 12, 16, 16)))
    for K, kt in want_kt.items():
        assert any(c.K == K and p.kt == kt for c, p in single), K
    combos = {(c.sizes, c.directed, c.dloss, c.acc) for c in cs if c.K in CC.K_EDGES and not c.batch}
    assert len(combos) >= len(CC.K_EDGES)
    # forward walk
    assert set(CC.N_EDGES) <= {n for c, p in single for n in c.sizes}
    assert {n for c, p in single for n in c.sizes if p.T == 1} >= {1, 7, 63, 64}
    assert any(p.T % 2 == 0 and p.T >= 2 for c, p in single) and any(p.T % 2 == 1 and p.T >= 3 for c, p in single)
    assert any(n % 64 and p.T > 1 for c, p, n in every) and any(n % 64 == 0 for c, p, n in every)
    two = [(c, p) for c, p in single if p.Z < p.T]                # a workgroup walks at least two column tiles
    assert any(c.K <= 16 for c, p in two) and any(c.K > 16 for c, p in two)
    assert all(p.T == 46 and p.Z == 45 and c.sizes == (2881,) for c, p in two)
    # backward walk: every class at both tile widths with both accumulate values; the batch rows add none of them
    seen = {(CC.bwd_class(p), c.acc) for c, p in single}
    for cw in (64, 32):
        for cls in ("one_tile", "split_all", "split_even", "split_ragged"):
            for acc in (0, 1):
                assert (f"{cls}_cw{cw}", acc) in seen, (cls, cw, acc)
    assert all(p.splits >= 2 for c, p, n in every if p.col_tiles >= 2)      # the non-split multi-tile walk: n >= 32 705
    assert all(p.kt >= 12 for c, p, n in every if p.cw == 32) and all(c.K >= 177 for c, p in single
                                                                      if p.cw == 32 and p.split_tiles >= 2)
    # edge forms: all six in the forward and in the backward, each with a full and a partial last chunk
    for K in CC.K_VEC16:
        assert any(c.K == K and p.fwd_vec == 4 and p.bwd_vec == 4 for c, p in single), K
    for K in CC.K_VEC4:
        assert any(c.K == K and p.fwd_vec == 1 and p.bwd_vec == 1 for c, p in single), K
    for form in ((4, 1), (4, 2), (4, 4), (1, 1), (1, 4), (1, 16)):
        for full in (True, False):
            assert any((p.fwd_vec, p.fwd_nch) == form and CC.chunk_full(*form, c.K) == full for c, p in single), (form, full)
            assert any((p.bwd_vec, p.bwd_nch) == form and CC.chunk_full(*form, c.K) == full for c, p in single), (form, full)
    # K % 4 == 0 forced scalar, one reason at a time
    k4 = [(c, p) for c, p in single if c.K % 4 == 0]
    assert any((c.K + c.spad) % 4 and not c.s_shift and p.fwd_vec == 1 and p.bwd_vec == 1 for c, p in k4)
    assert any(c.spad % 4 == 0 and c.s_shift and p.fwd_vec == 1 and p.bwd_vec == 1 for c, p in k4)
    assert any(c.spad == 0 and not c.s_shift and c.dpad % 4 and not c.ds_shift and (p.fwd_vec, p.bwd_vec) == (4, 1)
               for c, p in k4)
    assert any(c.spad == 0 and not c.s_shift and c.dpad % 4 == 0 and c.ds_shift and (p.fwd_vec, p.bwd_vec) == (4, 1)
               for c, p in k4)
    # scalars
    assert {c.dloss for c in cs} == {None, 1.7, -0.6} and {c.acc for c in cs} == {0, 1}
    assert {c.skind for c in cs} == {"softmax", "ties", "grid"}
    for kind in ("ties", "grid"):
        assert {c.directed for c in cs if c.skind == kind} == {False, True}
    assert any(c.loops for c in cs) and {c.directed for c in cs} == {False, True}
    # batches: at least three, graphs of different forward and backward classes, the largest not first, a 16-byte form
    # on the per-graph pointers, both accumulate values, one weighted; and a single directed weighted row
    batches = [c for c in cs if c.batch]
    assert len(batches) >= 3 and {c.acc for c in batches} == {0, 1}
    for c in batches:
        ps = plans[c.name]
        assert len({CC.bwd_class(p) for p in ps}) >= 2 and len({p.T for p in ps}) >= 2
        assert int(np.argmax(c.sizes)) > 0 and 1 in c.sizes
        assert len({(p.n_dense, p.n_edge) for p in ps}) >= 3          # the partial offsets differ graph by graph
    assert any(all(p.fwd_vec == 4 and p.bwd_vec == 4 for p in plans[c.name]) and any(n % 4 for n in c.sizes[:-1])
               for c in batches)
    assert any(max(p.splits for p in plans[c.name]) > 1 and plans[c.name][0].splits == 1 for c in batches)
    # the shared partial buffer, sized by the largest graph, is used again by a later, smaller split graph
    assert all(sum(p.splits > 1 for p in plans[c.name]) >= 2 for c in batches)
    assert sum(1 < plans[c.name][-1].splits < max(p.splits for p in plans[c.name]) for c in batches) >= 2
    assert any(c.weighted and c.directed for c in batches) and any(c.weighted and c.directed and not c.batch for c in cs)


def test_inputs_are_what_their_row_says():
    for c in CC.CASES:
        _, inp, ref = CC.case_data(c.name)
        off = inp["off"]
        assert inp["S"].shape == (sum(c.sizes), c.K) and (inp["indices_t"] is None) == (not c.directed)
        for b, g in enumerate(inp["graphs"]):
            n, A = g["n"], g["mask"]
            assert (A == A.T).all() == (not c.directed) or n < 3, c.name
            assert np.array_equal(g["a"] != 0, A) and int(g["ip"][-1]) == int(A.sum()) > 0 or (c.batch and n == 1)
            if not c.weighted:
                assert set(np.unique(g["a"])) <= {0.0, 1.0}
            else:
                assert (np.unique(g["val"]).size > min(8, g["val"].size // 2)) and (c.directed or np.array_equal(g["a"], g["a"].T))
            if n > 2:
                assert not A[0].any() and not A[:, 0].any(), "node 0 is isolated"
            if n >= CC.PLANT_MIN_N:                                # the 4-way unroll and its tail, in both lists
                assert set(CC.PLANTED_COUNTS) <= set(np.diff(g["ip"]).tolist()), c.name
                assert set(CC.PLANTED_COUNTS) <= set(np.diff(g["ipt"]).tolist()), c.name
            if c.loops and n >= CC.PLANT_MIN_N:
                assert np.diag(A).sum() >= 3
            # the batch arrays: global edge offsets, local indices
            e0, e1 = int(inp["indptr"][off[b]]), int(inp["indptr"][off[b + 1]])
            assert np.array_equal(inp["indices"][e0:e1], g["ix"]) and e1 - e0 == int(g["ip"][-1])
            assert g["ix"].size == 0 or g["ix"].max() < n
        if c.skind == "ties":
            t0, t1, t2, t3 = CC.TIE_ROWS
            S, A = inp["S"], inp["graphs"][0]["mask"]
            raw32 = S @ S.T
            assert (raw32[np.ix_(CC.TIE_ROWS, CC.TIE_ROWS)] == 1.0).all() and ref["ties"] == 16
            assert A[t0, t0] and not A[t1, t1] and A[t0, t1] and A[t1, t0] and not A[t2, t3] and not A[t3, t2]
            assert ref["ties_edge"] >= 3 and ref["ties_nonedge"] >= 3 and ref["above"] == 0
        if c.skind == "grid":
            S = inp["S"]
            assert np.array_equal(S * 4, np.round(S * 4)) and S.sum(axis=1).max() == 1.5
            assert np.array_equal((S @ S.T).astype(np.float64), S.astype(np.float64) @ S.astype(np.float64).T)
            assert ref["ties"] > 0 and ref["above"] > 0 and ref["below"] > 0 and ref["margin"] == float("inf")
            assert ref["ties_edge"] + ref["ties_nonedge"] == ref["ties"]
        if c.skind == "softmax":
            assert ref["ties"] == 0 and ref["above"] == 0


WORST = {}


@pytest.mark.parametrize("name", [c.name for c in CC.CASES])
def test_row_qualifies_and_the_fp32_formula_meets_the_counted_bound(name):
    c, inp, ref = CC.case_data(name)
    assert CC.qualifies(c, ref), (name, ref["margin"], 64 * (c.K + 1) * CC.U)
    old = CC.prior(c, ref) if c.acc else None
    loss32, d32 = CC.formula32(c, inp)
    r = CC.compare(c, ref, loss32, CC.output(d32, old), old)
    WORST[name] = (r["fwd"], r["bwd"])
    print(f"[csr linkpred] {name}: fp32 formula at {r['fwd']:.4f} (loss) and {r['bwd']:.4f} (dS) of the counted bound; "
          f"largest so far {max(v[0] for v in WORST.values()):.4f} / {max(v[1] for v in WORST.values()):.4f}")
    assert not r["problems"], r["problems"]
    # the decomposed evaluation the kernels perform, in float64, is the reference; rounded once it passes
    loss_e, d_e = CC.emulate(c, inp, None, old)
    assert abs(loss_e - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert not CC.compare(c, ref, np.float32(loss_e), d_e, old)["problems"]
    if c.acc:                                                      # the prior is of each element's own magnitude
        assert (np.abs(old) >= 0.99 * ref["mag"]).all() and (np.abs(old) <= 2.01 * ref["mag"]).all()


@pytest.mark.parametrize("fault", CC.FAULTS)
def test_planted_defect_violates_the_bound(fault, plans):
    c, inp, ref = CC.case_data(CC.FAULT_ROW[fault])
    p = plans[c.name][int(np.argmax(c.sizes))]
    need = {"offdiag_once": p.T >= 2, "last_col_tile_dropped": p.T >= 2 and c.sizes[0] % 64 != 0,
            "last_split_dropped": p.splits >= 2 and p.split_tiles >= 2, "tail_edges_skipped": c.sizes[0] >= CC.PLANT_MIN_N,
            "factor2_missing": not c.directed, "transposed_ignored": c.directed, "tie_gate_1": c.skind == "ties",
            "above_gate_1": ref["above"] > 0,
            "chunk_duplicates": p.fwd_vec == 4 and p.bwd_vec == 4 and not CC.chunk_full(4, p.fwd_nch, c.K),
            "accumulate_ignored": c.acc == 1, "dloss_ignored": c.dloss not in (None, 1.0), "batch_partial_offset": c.batch}
    assert need[fault], (fault, c.name)
    old = CC.prior(c, ref) if c.acc else None
    loss, dS = CC.emulate(c, inp, fault, old)
    r = CC.compare(c, ref, np.float32(loss), dS, old)
    print(f"[csr linkpred] {fault} on {c.name}: loss {r['fwd']:.3g}, dS {r['bwd']:.3g} of the bound")
    assert r["problems"], (fault, r)
