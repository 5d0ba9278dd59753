"""Top-k pooling on CSR without a GPU: the numpy restatement of tests/csr_topk_cases.py against a brute-force `sorted`
per graph and against the radix select taken in the kernel's order; the new C entries' symbols, signatures and argument
errors (every refusal comes back before a launch); the restatement of dp_csr_topk_plan against the library and what the
case table reaches (every tier, pass count and workgroup size); the kernels' resources from the built library;
`from_device_csr` of both containers against `from_edge_lists` of the restatement's induced edge lists, field for field;
that each planted mistake is told apart (the integer outputs by inequality, dgate by its bound); and the surface of
`ops.csr_topk_pool` and `TopKPooling`."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_topk_cases as TC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR

NEW = ("dp_csr_topk_plan", "dp_csr_topk_workspace_bytes", "dp_csr_topk_select", "dp_csr_topk_induce",
       "dp_csr_topk_gather_fwd", "dp_csr_topk_gather_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ the restatement
def _py_ord(f):
    """ord of one fp32 in plain Python integers, written independently of the numpy form."""
    (bits,) = struct.unpack("<I", struct.pack("<f", f)) if not isinstance(f, int) else (f,)
    if bits == 0x80000000:
        bits = 0
    return (bits ^ 0xFFFFFFFF) if bits >> 31 else bits + 0x80000000


def test_the_order_of_the_keys():
    bits = np.array([0xFFC00000, 0xFFFFFFFF, 0xFF800000, 0xC0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                     0x3F800000, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF], dtype=np.uint32)
    o = TC.ord_bits(bits).astype(np.int64)
    assert [int(v) for v in o] == [_py_ord(int(b)) for b in bits]
    # -NaN (both) < -inf < -2 < -tiny < -0 == +0 < tiny < 1 < +inf < NaNs
    assert o[1] < o[0] < o[2] < o[3] < o[4] < o[5] == o[6] < o[7] < o[8] < o[9] < o[10] < o[11] < o[12]
    k = TC.keys(np.array([0.5, 0.5, -0.0, 0.0], np.float32), np.array([0, 1, 2, 3]))
    assert k[0] > k[1] and k[2] > k[3] and k[1] > k[2]               # equal scores: the lower id wins


@pytest.mark.parametrize("case", [c for c in TC.CASES if TC.graph(c[0]).n <= 6000], ids=TC.case_id)
def test_the_restatement_against_a_brute_force_sort(case):
    gname, kind, sel, F, _, _ = case
    g, s, p = TC.graph(gname), TC.scores(gname, kind), TC.pooled(gname, kind, sel)
    bits = s.view(np.uint32)
    kept = []
    for b in range(g.B):
        lo, hi = int(g.off[b]), int(g.off[b + 1])
        nb = hi - lo
        kb = min(nb, sel[1]) if sel[0] == "k" else min(nb, max(1, math.ceil(sel[1] * nb)))
        assert kb == p.kb[b]
        ranked = sorted(range(nb), key=lambda i: (-_py_ord(int(bits[lo + i])), i))     # best first, ties to the lower id
        kept += sorted(lo + i for i in ranked[:kb])
    assert np.array_equal(p.perm, np.asarray(kept, dtype=np.int32))
    if kind in ("ties", "equal", "normal", "parity"):                # ordinary floats: their own order says the same
        for b in range(g.B):
            lo, hi = int(g.off[b]), int(g.off[b + 1])
            order = np.lexsort((np.arange(hi - lo), -s[lo:hi].astype(np.float64)))
            assert np.array_equal(np.sort(order[:p.kb[b]]) + lo, p.perm[p.new_off[b]:p.new_off[b + 1]])
    # the induced CSR against the dense A[perm][:, perm]
    if g.n <= 1100:
        a = np.zeros((g.n, g.n), dtype=np.int64)
        a[g.rows, g.indices] = np.arange(1, g.nnz + 1)               # the entry's position + 1
        sub = a[np.ix_(p.perm, p.perm)]
        r, c = np.nonzero(sub)
        assert np.array_equal(p.indptr, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=p.n_out))]))
        assert np.array_equal(p.indices, c) and np.array_equal(p.edge_map, sub[r, c] - 1)
        gb = np.searchsorted(p.new_off, r, side="right") - 1
        assert np.array_equal(p.local, c - p.new_off[gb])
        rt, ct = np.nonzero(sub.T)
        assert np.array_equal(p.indices_t, ct)
        if g.directed:                                               # entry q of the transposed CSR is stored entry t_perm[q]
            assert np.array_equal(g.t_perm[p.edge_map_t], sub.T[rt, ct] - 1)
        else:                                                        # an undirected graph: the same arrays both ways
            assert np.array_equal(p.edge_map_t, sub[rt, ct] - 1)


def _radix_select(keys, kb, nb):
    """thr by the kernel's passes: 256-bin histograms from the top byte down, the low word's constant bytes skipped."""
    low = TC.cdiv(int(nb - 1).bit_length(), 8)
    prefix, mask, kk = 0, 0, int(kb)
    shifts = [56, 48, 40, 32] + [8 * (low - 1 - t) for t in range(low)]
    for p_, shift in enumerate(shifts):
        if p_ == 4 and low < 4:
            ones = (0xFFFFFFFF << (8 * low)) & 0xFFFFFFFF
            prefix |= ones
            mask |= ones
        cand = keys[(keys & np.uint64(mask)) == np.uint64(prefix)]
        hist = np.bincount(((cand >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        for d in range(255, -1, -1):
            if kk <= hist[d]:
                break
            kk -= int(hist[d])
        prefix |= d << shift
        mask |= 0xFF << shift
    return prefix, len(shifts)


@pytest.mark.parametrize("case", [c for c in TC.CASES if c[0] in ("g257", "g4097", "g65537", "mixed", "bigmix", "g2")],
                         ids=TC.case_id)
def test_the_radix_select_in_the_kernels_order_finds_the_threshold(case):
    g, p = TC.graph(case[0]), TC.pooled(*case[:3])
    for b in range(g.B):
        nb = int(g.sizes[b])
        if p.kb[b] == nb:
            assert p.thr[b] == 0
            continue
        thr, passes = _radix_select(p.keys[g.off[b]:g.off[b + 1]], p.kb[b], nb)
        assert thr == int(p.thr[b])
        assert passes == TC.plan(g.n, p.n_out, g.B, int(g.sizes.max()), nb, int(p.kb[b]), 1)[3]


def test_the_kept_counts():
    assert list(TC.counts([1, 2, 3, 4, 64, 65, 63], ratio=0.5)) == [1, 1, 2, 2, 32, 33, 32]     # ceil on and next to an integer
    assert list(TC.counts([1, 7, 300], ratio=1e-9)) == [1, 1, 1] and list(TC.counts([1, 7, 300], ratio=1.0)) == [1, 7, 300]
    assert list(TC.counts([1, 7, 300], k=3)) == [1, 3, 3] and list(TC.counts([1, 7, 300], k=5000)) == [1, 7, 300]
    assert list(TC.counts([10], ratio=0.3)) == [3] and list(TC.counts([10], ratio=0.7)) == [7]
    assert list(TC.counts([100], ratio=0.07)) == [8]                 # the float64 product decides: 0.07 * 100 > 7
    from graph_pooling_amd import ops
    for sizes in ([1, 2, 63, 64, 65, 255, 1025], [10, 20, 30, 100]):
        for kind, v in TC.SELS + (("ratio", 0.7), ("ratio", 0.07), ("ratio", 1 / 3)):
            assert np.array_equal(ops.topk_counts(sizes, **{kind: v}), TC.counts(sizes, **{kind: v}))


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_and_bound(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[f][1]) == len(fns[f][1])
    assert names("dp_csr_topk_plan") == ["n", "n_out", "B", "max_n", "n_b", "k_b", "F", "plan_out"]
    assert names("dp_csr_topk_select") == ["score", "node_off", "new_off", "node_off_host", "kb_host", "new_id", "perm",
                                           "thr", "n", "n_out", "B", "stream"]
    assert names("dp_csr_topk_induce") == ["indptr", "indices", "new_id", "perm", "new_off", "indptr_out", "indices_out",
                                           "indices_local_out", "edge_map", "n", "n_out", "B", "nnz", "cap", "workspace",
                                           "workspace_bytes", "stream"]
    assert names("dp_csr_topk_gather_fwd") == ["x", "ldx", "gate", "perm", "y", "ldy", "n", "n_out", "F", "stream"]
    assert names("dp_csr_topk_gather_bwd") == ["dy", "lddy", "x", "ldx", "gate", "new_id", "dx", "lddx", "dgate", "n",
                                               "n_out", "F", "stream"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "diffpool_hip.h")).read()
    assert "#define DP_CSR_TOPK_PLAN_INTS 10" in header and _lib.CSR_TOPK_PLAN_INTS == TC.PLAN_INTS == 10
    assert lib.dp_version() == 100


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1 / -2."""
    buf = (C.c_double * 64)()
    ibuf = (C.c_int * 64)()
    p, i = C.addressof(buf), C.addressof(ibuf)
    off = (C.c_int * 3)(0, 4, 10)
    kb = (C.c_int * 2)(2, 3)
    o, k = C.addressof(off), C.addressof(kb)

    def select(score=p, noff=i, newoff=i, noff_h=o, kb_h=k, new_id=i, perm=i, thr=p, n=10, n_out=5, B=2):
        return lib.dp_csr_topk_select(score, noff, newoff, noff_h, kb_h, new_id, perm, thr, n, n_out, B, None)

    bad_off, bad_kb0, bad_kb9 = (C.c_int * 3)(0, 4, 9), (C.c_int * 2)(0, 5), (C.c_int * 2)(5, 3)
    flat = (C.c_int * 3)(0, 0, 10)
    for kw, text in ((dict(score=None), "score is NULL"), (dict(noff=None), "node_off is NULL"),
                     (dict(newoff=None), "new_off is NULL"), (dict(new_id=None), "new_id is NULL"),
                     (dict(perm=None), "perm is NULL"), (dict(thr=None), "thr is NULL"),
                     (dict(noff_h=None), "node_off_host is NULL"), (dict(kb_h=None), "kb_host is NULL"),
                     (dict(score=p + 2), "score is not 4-byte"), (dict(perm=i + 1), "perm is not 4-byte"),
                     (dict(thr=p + 4), "thr is not 8-byte"), (dict(n=-1), "n=-1 must not be negative"),
                     (dict(n_out=-1), "n_out=-1 must not be negative"), (dict(B=-1), "B=-1 must not be negative"),
                     (dict(B=0), "need at least one graph"),
                     (dict(noff_h=C.addressof(bad_off)), "node_off_host must run from 0 to n=10"),
                     (dict(noff_h=C.addressof(flat)), "graph 0 has 0 nodes"),
                     (dict(kb_h=C.addressof(bad_kb0)), "k_b=0 of graph 0 must be 1 .. n_b=4"),
                     (dict(kb_h=C.addressof(bad_kb9)), "k_b=5 of graph 0 must be 1 .. n_b=4"),
                     (dict(n_out=6), "the k_b sum to 5, n_out=6")):
        assert select(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert select(n=0, n_out=0, B=0) == 0                            # nothing to do, no launch

    def induce(ip=i, ix=i, new_id=i, perm=i, newoff=i, ipo=i, ixo=i, ilo=i, em=i, n=10, n_out=5, B=2, nnz=8, cap=8, ws=p,
               wsb=16):
        return lib.dp_csr_topk_induce(ip, ix, new_id, perm, newoff, ipo, ixo, ilo, em, n, n_out, B, nnz, cap, ws, wsb, None)

    for kw, text in ((dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(new_id=None), "new_id is NULL"), (dict(perm=None), "perm is NULL"),
                     (dict(ipo=None), "indptr_out is NULL"), (dict(ixo=None), "indices_out is NULL"),
                     (dict(em=None), "edge_map is NULL"), (dict(newoff=None), "new_off is NULL"),
                     (dict(ilo=i + 2), "indices_local_out is not 4-byte"), (dict(em=i + 1), "edge_map is not 4-byte"),
                     (dict(n=-1), "n=-1 must not"), (dict(n_out=-1), "n_out=-1 must not"), (dict(B=-1), "B=-1 must not"),
                     (dict(nnz=-1), "nnz=-1 must not"), (dict(n_out=11), "n_out=11 exceeds n=10"),
                     (dict(cap=7), "cap=7 is below the input's nnz=8"), (dict(ws=None), "workspace must be there"),
                     (dict(ws=p + 8), "workspace must be there and 16-byte aligned")):
        assert induce(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert lib.dp_csr_topk_workspace_bytes(5) == 16 and lib.dp_csr_topk_workspace_bytes(0) == 16
    assert lib.dp_csr_topk_workspace_bytes(97) == 32 and lib.dp_csr_topk_workspace_bytes(96) == 16
    assert induce(n_out=97, n=100, wsb=16) == -2 and "workspace too small: need >= 32 bytes, have 16" in _err(lib)

    def fwd(x=p, ldx=8, gate=None, perm=i, y=p, ldy=8, n=10, n_out=5, F=8):
        return lib.dp_csr_topk_gather_fwd(x, ldx, gate, perm, y, ldy, n, n_out, F, None)

    for kw, text in ((dict(x=None), "x is NULL"), (dict(perm=None), "perm is NULL"), (dict(y=None), "y is NULL"),
                     (dict(x=p + 1), "x is not 4-byte"), (dict(gate=p + 2), "gate is not 4-byte"),
                     (dict(ldx=7), "ldx=7 smaller than its width 8"), (dict(ldy=7), "ldy=7 smaller than its width 8"),
                     (dict(n=-1), "n=-1"), (dict(n_out=-1), "n_out=-1"), (dict(F=-1), "F=-1"),
                     (dict(n_out=11), "n_out=11 exceeds n=10")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert fwd(n_out=0) == 0 and fwd(F=0, ldx=0, ldy=0) == 0 and fwd(n=0, n_out=0) == 0

    def bwd(dy=p, lddy=8, x=p, ldx=8, gate=p, new_id=i, dx=p, lddx=8, dgate=p, n=10, n_out=5, F=8):
        return lib.dp_csr_topk_gather_bwd(dy, lddy, x, ldx, gate, new_id, dx, lddx, dgate, n, n_out, F, None)

    for kw, text in ((dict(dy=None), "dy is NULL"), (dict(new_id=None), "new_id is NULL"), (dict(dx=None), "dx is NULL"),
                     (dict(x=None), "x is NULL"), (dict(gate=None), "dgate without gate"),
                     (dict(dgate=p + 2), "dgate is not 4-byte"), (dict(dy=p + 3), "dy is not 4-byte"),
                     (dict(lddy=7), "lddy=7 smaller"), (dict(lddx=7), "lddx=7 smaller"), (dict(ldx=7), "ldx=7 smaller"),
                     (dict(n=-1), "n=-1"), (dict(F=-1), "F=-1"), (dict(n_out=11), "n_out=11 exceeds n=10")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert bwd(n=0, n_out=0) == 0 and bwd(F=0, lddy=0, lddx=0, ldx=0) == 0
    assert bwd(n=0, n_out=0, x=None, gate=None, dgate=None) == 0     # the ungated form takes neither x nor dgate


def test_plan_restatement_equals_the_library(lib):
    out = (C.c_int * _lib.CSR_TOPK_PLAN_INTS)()
    seen = set()
    for max_n in (1, 64, 255, 256, 257, 512, 513, 1023, 1024, 1025, 4096, 4097, 65536, 65537, 1 << 20):
        for n_b in {1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 4096, 4097, 65536, 65537, max_n}:
            if n_b > max_n:
                continue
            for k_b in {1, max(1, n_b // 2), max(1, n_b - 1), n_b}:
                for B, F in ((1, 1), (3, 65), (1000, 130)):
                    n = max_n + (B - 1)
                    n_out = k_b + (B - 1)
                    assert lib.dp_csr_topk_plan(n, n_out, B, max_n, n_b, k_b, F, out) == 0, _err(lib)
                    assert tuple(out) == TC.plan(n, n_out, B, max_n, n_b, k_b, F), (max_n, n_b, k_b, B)
                    seen.add(tuple(out)[:4])
    assert {t[1] for t in seen} == {0, 1, 2} and {t[0] for t in seen} >= {64, 128, 192, 320, 1024}
    assert {t[3] for t in seen} == {0, 5, 6, 7}
    assert (1024, 1, 4, 6) in seen and (1024, 2, 5, 6) in seen and (1024, 2, 1024, 7) in seen      # 4096 | 4097 | 2^20
    for bad, text in (((-1, 0, 1, 1, 1, 1, 1), "n=-1"), ((4, 5, 1, 4, 4, 4, 1), "n_out=5 exceeds n=4"),
                      ((4, 2, 1, 4, 5, 2, 1), "n_b=5 must be 1 .. max_n=4"), ((4, 2, 1, 4, 4, 0, 1), "k_b=0 must be 1 .. n_b=4"),
                      ((4, 2, 1, 4, 4, 5, 1), "k_b=5 must be 1 .. n_b=4"), ((4, 2, 1, 4, 4, 2, -1), "F=-1")):
        assert lib.dp_csr_topk_plan(*bad, out) == -1 and text in _err(lib), bad
    assert lib.dp_csr_topk_plan(4, 2, 1, 4, 4, 2, 1, None) == -1 and "plan_out is NULL" in _err(lib)


def _plans_of(case):
    g, kb = TC.graph(case[0]), TC.sel_counts(TC.graph(case[0]), case[2])
    return {TC.plan(g.n, int(kb.sum()), g.B, int(g.sizes.max()), int(nb), int(k), case[3]) for nb, k in zip(g.sizes, kb)}


def test_the_table_reaches_every_tier_and_every_edge():
    assert {c[1] for c in TC.CASES} == set(TC.SKINDS) and {c[3] for c in TC.CASES} == set(TC.FS)
    assert {c[4] for c in TC.CASES} == set(TC.LAYOUTS) and {c[5] for c in TC.CASES} == {True, False}
    assert {c[2] for c in TC.CASES} == set(TC.SELS) and {c[0] for c in TC.CASES} == set(TC.SPECS)
    assert {(c[3], c[4]) for c in TC.CASES} == {(F, lay) for F in TC.FS for lay in TC.LAYOUTS}
    for w in TC.FS:
        lds = {name: ld(w) for name, (ld, _) in TC.LAYOUTS.items()}
        assert lds["tight"] == w and lds["pad4"] % 4 == 0 and lds["pad4"] > w and lds["odd"] % 2 == 1 and lds["odd"] > w
    assert TC.LAYOUTS["mis"][1] == 1
    assert set(TC.SINGLE) >= {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097}
    plans = set().union(*(_plans_of(c) for c in TC.CASES))
    assert {p[1] for p in plans} == {0, 1, 2}                       # all kept, keys in registers, keys recomputed
    assert {p[0] for p in plans} >= {64, 128, 256, 320, 1024}       # the select workgroup from one wave to sixteen
    assert {p[3] for p in plans} == {0, 5, 6, 7}                    # 256 | 257 and 65536 | 65537 nodes
    assert {(p[1], p[2]) for p in plans} >= {(1, 1), (1, 4), (2, 5), (2, 65)}
    assert {p[6] for p in plans} >= {1, 2} and max(p[6] for p in plans) > TC.SCAN_THREADS       # the scan's second chunk
    # every score kind meets both select tiers; ties straddle the cut
    for kind in ("ties", "equal", "zeros", "special"):
        tiers = set().union(*({p[1] for p in _plans_of(c)} for c in TC.CASES if c[1] == kind))
        assert {1, 2} <= tiers, kind
    for gname in ("g257", "g4097"):
        p, s, g = TC.pooled(gname, "ties", ("ratio", 0.5)), TC.scores(gname, "ties"), TC.graph(gname)
        assert ((s == s[p.perm[0]]) & ~p.kept).any() or (s[p.kept].min() == s[~p.kept].max())
        assert s[p.kept].min() == s[~p.kept].max()                  # equal scores on both sides of the cut
    z = TC.scores("g257", "zeros")
    assert (z.view(np.uint32) == 0x80000000).any() and (z.view(np.uint32) == 0).any()
    sp = TC.scores("g4097", "special").view(np.uint32)
    assert {0x7F800000, 0xFF800000, TC.NAN_POS, TC.NAN_NEG} <= set(int(v) for v in sp)
    # the graphs: directed, undirected and weighted; rows of 0 .. 9 entries, a hub row, self loops
    kinds = {(TC.graph(n).directed, TC.graph(n).weighted) for n in TC.SPECS}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    g = TC.graph("g1024")
    lens = np.diff(g.indptr)
    assert g.directed and set(range(10)) <= set(lens) and lens.max() >= 300 and (g.rows == g.indices).any()
    assert TC.graph("g1025").indptr[-1] > 0 and not TC.graph("g1025").directed
    e = TC.graph("edgeless")
    assert not np.diff(e.indptr)[e.off[1]:e.off[2]].any() and TC.graph("padded").pad_to == 100 > 64
    assert TC.pooled("bipart", "parity", ("ratio", 0.5)).nnz == 0 and TC.graph("bipart").nnz > 0
    assert TC.pooled("bipart_batch", "parity", ("ratio", 0.5)).nnz == 0
    ks = {(int(k), int(n)) for c in TC.CASES for k, n in zip(TC.sel_counts(TC.graph(c[0]), c[2]), TC.graph(c[0]).sizes)}
    assert any(k == 1 < n for k, n in ks) and any(k == n > 1 for k, n in ks) and (3, 5) in ks and (5, 5) in ks


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_topk_kernels_use_no_scratch_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if "k_csr_topk_" in d["name"]}
    assert len(ks) == 6, sorted(ks)
    for what in ("select", "count", "scan", "fill", "gather_fwd", "gather_bwd"):
        assert any("k_csr_topk_" + what in n for n in ks), what
    for d in ks.values():
        print(d)
        assert d["scratch"] == 0 and d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 64 and d.get("agprs", 0) == 0 and d["lds_static"] <= 2048, d
        if "gather" in d["name"]:
            assert d["lds_static"] == 0, d


# ------------------------------------------------------------------ from_device_csr
def _same_fields(a, b):
    assert set(a.__dict__) == set(b.__dict__), set(a.__dict__) ^ set(b.__dict__)
    for k, v in a.__dict__.items():
        w = b.__dict__[k]
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and torch.equal(v, w), k
        elif isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and np.array_equal(v, w), k
        else:
            assert v == w, (k, v, w)


@pytest.mark.parametrize("gname,kind,sel", [("mixed", "ties", ("ratio", 0.5)), ("edgeless", "special", ("k", 3)),
                                            ("padded", "normal", ("ratio", 0.25)), ("bipart_batch", "parity", ("ratio", 0.5)),
                                            ("bigmix", "zeros", ("ratio", 0.3)), ("edgeless", "ties", ("ratio", 1e-9))])
def test_batch_from_device_csr_equals_from_edge_lists_field_for_field(gname, kind, sel):
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrBatch
    g, p = TC.graph(gname), TC.pooled(gname, kind, sel)
    pad_to = None if g.pad_to is None else int(ops.topk_counts([g.pad_to], **{sel[0]: sel[1]})[0])
    lists = p.edge_lists()
    ws = None
    if g.values is not None:
        r = np.repeat(np.arange(p.n_out), np.diff(p.indptr))
        gb = np.searchsorted(p.new_off, r, side="right") - 1
        ws = [g.values[p.edge_map][gb == b] for b in range(g.B)]
    want = CsrBatch.from_edge_lists(p.kb, [s for s, _ in lists], [d for _, d in lists], "cpu", symmetric=False,
                                    pad_to=pad_to, weights=ws)
    t = lambda a, pad=False: torch.from_numpy(np.concatenate([a, np.zeros(int(pad and a.size == 0), a.dtype)]))
    fv = None if g.values is None else t(g.values[p.edge_map], True)
    fvt = None if g.values is None else t(g.values_t[p.edge_map_t], True)
    got = CsrBatch.from_device_csr(p.kb, t(p.indptr), t(p.indices, True), t(p.local, True), t(p.indptr_t),
                                   t(p.indices_t, True), t(p.local_t, True), fv, fvt, pad_to=pad_to, nnz=p.nnz)
    assert got.__dict__.pop("nnz") == p.nnz == want.nnz
    want.__dict__.pop("nnz")
    if not g.directed:                                               # from_edge_lists(symmetric=False) made a trio of its own
        und = CsrBatch.from_device_csr(p.kb, t(p.indptr), t(p.indices, True), t(p.local, True), values=fv, pad_to=pad_to)
        assert und.indices_t is und.indices and und.indptr_t is und.indptr and und.indices_t_local is und.indices_local
        assert und.values_t is und.values
    _same_fields(want, got)


def test_graph_from_device_csr_and_the_refusals():
    from graph_pooling_amd.sparse import CsrBatch, CsrGraph
    g, p = TC.graph("g257"), TC.pooled("g257", "ties", ("ratio", 0.5))
    r = np.repeat(np.arange(p.n_out), np.diff(p.indptr))
    want = CsrGraph.from_edges(p.n_out, r, p.indices, "cpu", symmetric=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    got = CsrGraph.from_device_csr(p.n_out, t(p.indptr), t(p.indices), t(p.indptr_t), t(p.indices_t), nnz=p.nnz)
    assert got.nnz == p.nnz and got.n == want.n == p.n_out and not got.weighted
    for f in ("indptr", "indices", "indptr_t", "indices_t"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    und = CsrGraph.from_device_csr(p.n_out, t(p.indptr), t(p.indices))
    assert und.indices_t is und.indices and "nnz" not in und.__dict__ and und.nnz == p.nnz
    with pytest.raises(ValueError, match="come together"):
        CsrGraph.from_device_csr(p.n_out, t(p.indptr), t(p.indices), t(p.indptr_t))
    with pytest.raises(ValueError, match="int32"):
        CsrGraph.from_device_csr(p.n_out, t(p.indptr).long(), t(p.indices))
    with pytest.raises(ValueError, match="n \\+ 1"):
        CsrGraph.from_device_csr(p.n_out + 1, t(p.indptr), t(p.indices))
    with pytest.raises(ValueError, match="nnz = 3"):
        CsrGraph.from_device_csr(p.n_out, t(p.indptr), t(p.indices), nnz=3)
    ip, ix = t(p.indptr), t(p.indices)
    with pytest.raises(ValueError, match="n_total \\+ 1"):
        CsrBatch.from_device_csr([p.n_out + 1], ip, ix, ix)
    with pytest.raises(ValueError, match="come together"):
        CsrBatch.from_device_csr([p.n_out], ip, ix, ix, indptr_t=ip)
    with pytest.raises(ValueError, match="one at least"):
        CsrBatch.from_device_csr([p.n_out], ip, ix[:0], ix[:0])
    with pytest.raises(ValueError, match="at least one node"):
        CsrBatch.from_device_csr([0], ip[:1], ix, ix)
    with pytest.raises(ValueError, match="values_t without values"):
        CsrBatch.from_device_csr([p.n_out], ip, ix, ix, values_t=torch.zeros(ix.numel()))
    with pytest.raises(ValueError, match="pad_to"):
        CsrBatch.from_device_csr([p.n_out], ip, ix, ix, pad_to=1)


# ------------------------------------------------------------------ planted mistakes
def _outputs(p):
    return dict(thr=p.thr, perm=p.perm, new_id=p.new_id, indptr=p.indptr, indices=p.indices, local=p.local,
                edge_map=p.edge_map)


class _Wrong(TC.Pooled):
    """The restatement with one mistake planted: in the kept counts, in the order of the keys, in the numbering or in
    the induced CSR."""

    def __init__(self, gname, kind, sel, mistake):
        g, s = TC.graph(gname), TC.scores(gname, kind)
        self.mistake = mistake
        kb = TC.sel_counts(g, sel)
        if mistake == "floor for ceil":
            kb = np.minimum(g.sizes, np.maximum(1, np.floor(np.float64(sel[1]) * g.sizes).astype(np.int64)))
        local = (np.arange(g.n) - g.off[g.graph_of(np.arange(g.n))]).astype(np.uint64)
        bits = s.view(np.uint32)
        keys = None
        if mistake == "ties to the higher id":                       # the id itself in the low word
            keys = (TC.ord_bits(bits).astype(np.uint64) << np.uint64(32)) | local
        if mistake == "minus zero below plus zero":                  # ord without -0.0 made +0.0
            o = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
            keys = (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - local)
        super().__init__(g, s, kb, own_keys=keys)
        if mistake == "descending-score numbering":
            self.perm = np.concatenate([mine[np.argsort(self.keys[mine])[::-1]] for mine in
                                        (self.perm[self.new_off[b]:self.new_off[b + 1]] for b in range(g.B))])
            self.new_id = np.full(g.n, -1, np.int32)
            self.new_id[self.perm] = np.arange(self.n_out, dtype=np.int32)
            self.indptr, self.indices, self.local, self.edge_map = self._induce(g.rows, g.indices)

    def _induce(self, rows, cols):
        if self.mistake == "one endpoint dropped":                   # the row's end kept is enough
            em = np.nonzero(self.new_id[rows] >= 0)[0].astype(np.int32)
            r, c = self.new_id[rows[em]], np.maximum(self.new_id[cols[em]], 0)
            indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=self.n_out))]).astype(np.int32)
            gb = np.searchsorted(self.new_off, r, side="right") - 1
            return indptr, c.astype(np.int32), (c - self.new_off[gb]).astype(np.int32), em
        ip, ix, il, em = super()._induce(rows, cols)
        if self.mistake == "columns left in old ids":
            ix = cols[em].astype(np.int32)
        if self.mistake == "local and global swapped":
            ix, il = il, ix
        if self.mistake == "last block of the scan dropped":         # the rows of the last 32-row block start at 0
            ip = ip.copy()
            first = (self.n_out - 1) // TC.ROWS_PER_WG * TC.ROWS_PER_WG
            ip[first:] -= ip[first]
        return ip, ix, il, em


MISTAKES = ("ties to the higher id", "floor for ceil", "minus zero below plus zero", "descending-score numbering",
            "one endpoint dropped", "columns left in old ids", "local and global swapped",
            "last block of the scan dropped")


@pytest.mark.parametrize("mistake", MISTAKES)
def test_each_planted_mistake_changes_an_integer_output(mistake):
    gname, kind, sel = "mixed", "zeros" if "zero" in mistake else "ties", ("ratio", 0.3)
    right, wrong = _outputs(TC.pooled(gname, kind, sel)), _outputs(_Wrong(gname, kind, sel, mistake))
    differs = [k for k in right if right[k].shape != wrong[k].shape or not np.array_equal(right[k], wrong[k])]
    print(mistake, "->", differs)
    assert differs, mistake


def test_the_float_checks_reject_each_planted_mistake():
    case = ("mixed", "ties", ("ratio", 0.3), 130, "tight", True)
    p = TC.pooled(*case[:3])
    x, gate, dy = TC.inputs(case)
    y, dx = TC.forward32(x, gate, p.perm), TC.backward32(dy, gate, p)
    ref, mag = TC.dgate64(dy, x, p)
    bound = TC.dgate_bound(130, mag)
    assert not np.array_equal(y, x[p.perm]) and not np.array_equal(dx, TC.backward32(dy, None, p))     # the gate not applied
    dropped = np.nonzero(~p.kept)[0]
    assert dropped.size and not dx[dropped].any() and not ref[dropped].any() and not bound[dropped].any()
    bad = ref.copy()
    bad[dropped[0]] = 1e-30                                          # a non-zero dgate on a dropped node: bound 0 there
    assert TC.moved(ref, bad, bound) == float("inf") and TC.moved(ref, ref, bound) == 0.0
    bad_dx = dx.copy()
    bad_dx[dropped[0], 0] = 1e-30
    assert not np.array_equal(bad_dx, dx)
    # an fp32 evaluation in the kernel's order stays inside; one lane's column left out does not
    lanes = np.zeros((p.n_out, 64), dtype=np.float32)
    xs = x[p.perm]
    for f in range(130):
        lanes[:, f % 64] = (dy[:, f].astype(np.float64) * xs[:, f].astype(np.float64) + lanes[:, f % 64]).astype(np.float32)
    w = lanes
    for d in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ d]).astype(np.float32)
    got = np.zeros(p.g.n)
    got[p.perm] = w[:, 0]
    ratio = TC.moved(ref, got, bound)
    print(f"dgate in the kernel's order: |error| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    short = np.zeros(p.g.n)
    short[p.perm] = (dy[:, :129].astype(np.float64) * xs[:, :129]).sum(1)
    assert TC.moved(ref, short, bound) > 1.0
    assert TC.moved(ref, ref * (1 + 2.0 ** -12), bound) > 1.0


# ------------------------------------------------------------------ the Python surface
def test_csr_topk_pool_refusals():
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrGraph
    g = CsrGraph.from_edges(5, [0, 1], [1, 2], "cpu")
    x, s = torch.rand(5, 3), torch.rand(5)
    for kw, text in ((dict(), "exactly one of ratio and k"), (dict(ratio=0.5, k=2), "exactly one"),
                     (dict(ratio=0.0), "ratio must lie in"), (dict(ratio=1.5), "ratio must lie in"),
                     (dict(ratio=True), "ratio must lie in"), (dict(k=0), "k must be an integer >= 1"),
                     (dict(k=2.0), "k must be an integer")):
        with pytest.raises(ValueError, match=text):
            ops.csr_topk_pool(x, s, g, **kw)
    with pytest.raises(ValueError, match="expected x"):
        ops.csr_topk_pool(torch.rand(4, 3), s, g, ratio=0.5)
    with pytest.raises(ValueError, match="score must be a float32 tensor"):
        ops.csr_topk_pool(x, torch.rand(4), g, ratio=0.5)
    with pytest.raises(ValueError, match="score must be a float32 tensor"):
        ops.csr_topk_pool(x, s.double(), g, ratio=0.5)
    with pytest.raises(ValueError, match="gate must be a float32 tensor"):
        ops.csr_topk_pool(x, s, g, ratio=0.5, gate=torch.rand(5, 1))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.csr_topk_pool(x, s, g, ratio=0.5)
    for doc in (ops.csr_topk_pool.__doc__,):
        assert "hipGraph" in doc and "NaN" in doc and "ascending" in doc


def test_topk_pooling_parameters_and_the_flat_buffer():
    import graph_pooling_amd
    from graph_pooling_amd.optim import FusedClipAdam, _FlatModule
    from graph_pooling_amd.sparse import TopKPooling
    assert graph_pooling_amd.TopKPooling is TopKPooling and "TopKPooling" in graph_pooling_amd.__all__
    torch.manual_seed(3)
    proj, gcn = TopKPooling(6, 0.25), TopKPooling(6, ratio=1.0, score="gcn")
    assert [(n, tuple(q.shape)) for n, q in proj.named_parameters()] == [("p", (6,))]
    assert [(n, tuple(q.shape)) for n, q in gcn.named_parameters()] == [("weight", (6, 1)), ("bias", (1,))]
    assert float(proj.p.detach().abs().max()) <= 6 ** -0.5 and float(proj.p.detach().norm()) > 0 and not gcn.bias.any()
    for kw, text in ((dict(input_dim=0), "input_dim"), (dict(input_dim=4, ratio=0), "ratio must lie in"),
                     (dict(input_dim=4, ratio=1.1), "ratio must lie in"), (dict(input_dim=4, score="mlp"), "'proj' or 'gcn'")):
        with pytest.raises(ValueError, match=text):
            TopKPooling(**kw)
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        proj(torch.rand(3, 6), torch.eye(3))
    model = torch.nn.Sequential(proj, gcn)
    opt = FusedClipAdam(model, lr=0.01, clip=2.0)
    flat = opt.model
    assert isinstance(flat, _FlatModule)
    flat._ensure_flat(torch.device("cpu"))
    assert flat._flat.numel() == 6 + 6 + 1
    assert proj.p.data_ptr() == flat._flat.data_ptr() and gcn.bias.data_ptr() == flat._flat.data_ptr() + 4 * 12
