"""Learned edge weights on a CSR, without a GPU: the new C entries' symbols, signatures and argument errors (every refusal
comes back before a launch), the Python restatement of dp_csr_edge_plan over a sweep, what the case table reaches (every
lane tier at both register edges and both workgroup edges), the kernels' resources from the built library, that the
bounds of tests/csr_edge_ops_cases.py tell a bug from rounding on the table's inputs, `mirror_perm` / `directed()` on
host-built containers, and what `EdgeAttention` calls (the recording library of tests/test_csr_host_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, EdgeAttention
from tests import csr_edge_ops_cases as OC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR
from tests.test_csr_host_cpu import fake_lib

NEW = ("dp_csr_edge_plan", "dp_csr_edge_softmax_fwd", "dp_csr_edge_softmax_bwd", "dp_csr_sym_norm_fwd",
       "dp_csr_sym_norm_bwd")
KERNELS = ("k_edge_softmax_fwd", "k_edge_softmax_bwd", "k_edge_sym_rdeg", "k_edge_sym_scale", "k_edge_sym_gdeg",
           "k_edge_sym_dvalues")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_with_the_containers_field_names(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[f][1]) == len(fns[f][1])
    assert names("dp_csr_edge_plan") == ["n_rows", "nnz", "plan_out"]
    assert names("dp_csr_edge_softmax_fwd") == ["scores", "indptr", "out", "n_rows", "nnz", "stream"]
    assert names("dp_csr_edge_softmax_bwd") == ["out", "dout", "indptr", "dscores", "n_rows", "nnz", "stream"]
    head = ["indptr", "indices", "values", "indptr_t", "indices_t", "mirror", "rdeg"]
    assert names("dp_csr_sym_norm_fwd") == head + ["out", "n", "nnz", "stream"]
    assert names("dp_csr_sym_norm_bwd") == head + ["dout", "gdeg", "dvalues", "n", "nnz", "stream"]


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1."""
    buf = (C.c_float * 64)()
    ibuf = (C.c_int * 16)()
    p, i, j = C.addressof(buf), C.addressof(ibuf), C.addressof(ibuf) + 32
    fwd = lambda s=p, ip=i, out=p, n=2, nnz=4: lib.dp_csr_edge_softmax_fwd(s, ip, out, n, nnz, None)
    for kw, text in ((dict(s=None), "scores is NULL"), (dict(ip=None), "indptr is NULL"), (dict(out=None), "out is NULL"),
                     (dict(s=p + 2), "scores is not 4-byte"), (dict(ip=i + 1), "indptr is not 4-byte"),
                     (dict(out=p + 1), "out is not 4-byte"), (dict(n=-1), "n_rows=-1 must not be negative"),
                     (dict(nnz=-3), "nnz=-3 must not be negative")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert fwd(n=0) == 0 and fwd(nnz=0) == 0                       # nothing to do: OK, nothing launched
    bwd = lambda a=p, g=p, ip=i, ds=p, n=2, nnz=4: lib.dp_csr_edge_softmax_bwd(a, g, ip, ds, n, nnz, None)
    for kw, text in ((dict(a=None), "out is NULL"), (dict(g=None), "dout is NULL"), (dict(ip=None), "indptr is NULL"),
                     (dict(ds=None), "dscores is NULL"), (dict(g=p + 3), "dout is not 4-byte"),
                     (dict(n=-1), "n_rows=-1"), (dict(nnz=-1), "nnz=-1")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert bwd(n=0) == 0 and bwd(nnz=0) == 0
    sf = lambda ip=i, ix=i, v=p, ipt=i, ixt=i, mir=i, r=p, out=p, n=2, nnz=4: lib.dp_csr_sym_norm_fwd(
        ip, ix, v, ipt, ixt, mir, r, out, n, nnz, None)
    for kw, text in ((dict(ip=None), "indptr is NULL"), (dict(ix=None, ixt=j), "indices is NULL"),
                     (dict(v=p + 1), "values is not 4-byte"), (dict(ipt=None), "indptr_t is NULL"),
                     (dict(ixt=None), "indices_t is NULL"), (dict(mir=i + 2), "mirror is not 4-byte"),
                     (dict(mir=None, ixt=j), "mirror is NULL beside a transposed CSR of its own"),
                     (dict(r=None), "rdeg is NULL"), (dict(out=None), "out is NULL"), (dict(n=-1), "n=-1"),
                     (dict(nnz=-1), "nnz=-1")):
        assert sf(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    # NULL values (a 0/1 container) and, beside indices_t == indices, a NULL mirror pass the checks
    assert sf(v=None, n=0) == 0 and sf(mir=None, nnz=0) == 0 and sf(n=0) == 0
    sb = lambda ip=i, ix=i, v=p, ipt=i, ixt=i, mir=i, r=p, g=p, gd=p, dv=p, n=2, nnz=4: lib.dp_csr_sym_norm_bwd(
        ip, ix, v, ipt, ixt, mir, r, g, gd, dv, n, nnz, None)
    for kw, text in ((dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(v=p + 1), "values is not 4-byte"), (dict(ipt=None), "indptr_t is NULL"),
                     (dict(ixt=None), "indices_t is NULL"), (dict(mir=None), "mirror is NULL"),
                     (dict(r=None), "rdeg is NULL"), (dict(g=None), "dout is NULL"), (dict(gd=None), "gdeg is NULL"),
                     (dict(dv=None), "dvalues is NULL"), (dict(n=-1), "n=-1"), (dict(nnz=-1), "nnz=-1")):
        assert sb(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert sb(v=None, n=0) == 0 and sb(nnz=0) == 0


def test_plan_restatement_equals_the_library_over_a_sweep(lib):
    out = (C.c_int * _lib.CSR_EDGE_PLAN_INTS)()
    seen = set()
    rows = (0, 1, 3, 4, 5, 64, 576, 577, 5748, 1 << 20)
    for n_rows in rows:
        for nnz in sorted({0, 1, 7, n_rows, 5 * n_rows, 8 * n_rows, 8 * n_rows + 1, 32 * n_rows, 32 * n_rows + 1,
                           100 * n_rows, 6 << 20}):
            assert lib.dp_csr_edge_plan(n_rows, nnz, out) == 0
            assert tuple(out) == OC.plan(n_rows, nnz), (n_rows, nnz)
            seen.add(tuple(out))
    assert seen == {(4, 8, 64, 32), (16, 4, 16, 64), (64, 4, 4, 256)}
    assert lib.dp_csr_edge_plan(5748, 28534, out) == 0 and out[0] == 4          # DD's largest graph: about 5 per row
    for bad, text in (((-1, 4), "n_rows=-1"), ((4, -1), "nnz=-1")):
        assert lib.dp_csr_edge_plan(*bad, out) == -1 and text in _err(lib)
    assert lib.dp_csr_edge_plan(4, 4, None) == -1 and "plan_out is NULL" in _err(lib)


def test_the_table_reaches_every_tier_at_both_edges(lib):
    out = (C.c_int * _lib.CSR_EDGE_PLAN_INTS)()
    tiers = set()
    for name in OC.TIER_GRAPHS:
        g = OC.graph(name)
        assert lib.dp_csr_edge_plan(g.n, g.nnz, out) == 0 and tuple(out) == g.plan
        lanes, regs, rows_per_wg, fit = g.plan
        assert name.startswith(f"t{lanes}-")                         # the filler rows put the mean into the named tier
        lens = OC.row_len(g)
        assert tuple(lens[:len(OC.PLANTED)]) == OC.PLANTED
        assert fit in lens and fit + 1 in lens                       # the last row read once, the first read twice
        assert lens.max() == 530 > 2 * fit                           # a row that loops in every tier
        tiers.add((lanes, g.n % rows_per_wg))
        assert (g.rows == g.indices).any()                           # self loops
    assert tiers == {(l, e) for l in (4, 16, 64) for e in (0, 1)}    # n_rows at the workgroup edge and one past it
    u = OC.graph("undirected")
    assert not u.directed and (u.rows == u.indices).sum() >= 2 and OC.row_len(u).max() >= 70
    assert np.array_equal(u.values, u.values[u.mirror]) and not np.array_equal(u.mirror, np.arange(u.nnz))
    b = OC.graph("batch")
    assert list(np.diff(b.off)) == [37, 1, 64, 98] and OC.row_len(b).max() >= 64
    gr = b.graph_of_row()
    assert np.array_equal(gr[b.rows], gr[b.indices])                 # block diagonal
    for name in OC.GRAPHS:                                           # the mirror is the transposition
        g = OC.graph(name)
        assert np.array_equal(g.rows[g.mirror], g.indices_t) and np.array_equal(g.indices[g.mirror], g.rows_t)
    assert {k for _, k in OC.SOFTMAX_CASES} == set(OC.SOFTMAX_KINDS)
    assert {g for g, _ in OC.SOFTMAX_CASES} == {g for g, _ in OC.SYM_CASES} == set(OC.GRAPHS)


def test_the_softmax_inputs_are_what_their_names_say():
    for gname in OC.GRAPHS:
        g = OC.graph(gname)
        lens = OC.row_len(g)
        s = OC.softmax_inputs((gname, "ties"))
        assert len(np.unique(s)) == 4
        s = OC.softmax_inputs((gname, "equal"))
        ref, _ = OC.softmax_ref(g, s)
        pow2 = (lens & (lens - 1)) == 0
        assert np.array_equal(ref[pow2[g.rows]], (1.0 / lens[g.rows])[pow2[g.rows]]) and pow2[g.rows].any()
        s = OC.softmax_inputs((gname, "shift80"))
        assert s.max() > 80 and s.min() < -80
        s = OC.softmax_inputs((gname, "below200"))
        ref, bound = OC.softmax_ref(g, s)
        low = ref < OC.FLT_MIN
        assert low.sum() >= (lens >= 2).sum() // 2 and (bound[low] >= OC.FLT_MIN).all()
        assert np.isfinite(ref).all() and abs(np.bincount(g.rows, ref, g.n)[lens > 0] - 1).max() < 1e-12


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_edge_kernels_use_no_scratch_no_lds_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if d["name"].startswith("k_edge_")}
    assert sorted(ks) == sorted(f"{k}<{l}>" for k in KERNELS for l in (4, 16, 64))
    for d in ks.values():
        assert d["scratch"] == 0 and d["lds_static"] == 0, d
        assert d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 64, d


# ------------------------------------------------------------------ the bounds tell a bug from rounding
def _shifted_rows(g):
    """A segmentation off by one entry: every entry is summed with the row of the entry before it."""
    return np.concatenate([g.rows[:1], g.rows[:-1]])


@pytest.mark.parametrize("case", OC.SOFTMAX_CASES, ids=OC.case_id)
def test_softmax_bound_discriminates(case):
    g = OC.graph(case[0])
    s = OC.softmax_inputs(case)
    ref, bound = OC.softmax_ref(g, s)
    assert np.isfinite(ref).all() and (bound > 0).all()
    with np.errstate(all="ignore"):
        faults = {"last entry of a row dropped": OC.softmax_ref(g, s, drop_last=True)[0],
                  "sum over the wrong row by one entry": OC.softmax_ref(g, s, rows=_shifted_rows(g))[0]}
        if case[1] == "shift80":
            faults["no max subtraction"] = OC.softmax_ref(g, s, shift=False)[0]
    for what, other in faults.items():
        assert OC.moved(ref, other, bound) > 4.0, (what, OC.moved(ref, other, bound))


@pytest.mark.parametrize("case", [c for c in OC.SOFTMAX_BWD_CASES if c[1] == "ordinary"], ids=OC.case_id)
def test_softmax_bwd_bound_discriminates(case):
    g = OC.graph(case[0])
    a, dout = OC.softmax_bwd_inputs(case)
    ref, bound = OC.softmax_bwd_ref(g, a, dout)
    one = OC.row_len(g)[g.rows] == 1
    assert one.any() or case[0] == "undirected"                      # (its ring runs both ways: two entries at least)
    assert np.array_equal(a[one], np.ones(one.sum(), np.float32)) and not ref[one].any()
    faults = {"last entry of a row dropped": OC.softmax_bwd_ref(g, a, dout, drop_last=True)[0],
              "sum over the wrong row by one entry": OC.softmax_bwd_ref(g, a, dout, rows=_shifted_rows(g))[0]}
    for what, other in faults.items():
        assert OC.moved(ref, other, bound) > 4.0, (what, OC.moved(ref, other, bound))


@pytest.mark.parametrize("case", OC.SYM_CASES, ids=OC.case_id)
def test_sym_norm_bounds_discriminate(case):
    g = OC.graph(case[0])
    values = OC.sym_values(case)
    ref, bound, r, rbound = OC.sym_fwd_ref(g, values)
    assert np.isfinite(ref).all() and (bound > 0).all() and (rbound > 0).all()
    if g.directed:
        other = OC.sym_fwd_ref(g, values, degree="row")
        assert OC.moved(ref, other[0], bound) > 4.0 and OC.moved(r, other[2], rbound) > 4.0
        if values is not None:                                       # ones are their own permutation
            other = OC.sym_fwd_ref(g, values, mirror=False)
            assert OC.moved(ref, other[0], bound) > 4.0 and OC.moved(r, other[2], rbound) > 4.0
    else:
        assert np.array_equal(ref, ref[g.mirror])                    # a_ij = a_ji stays so
    values, rdeg, dout = OC.sym_bwd_inputs(case)
    dv, dbound, G, gbound = OC.sym_bwd_ref(g, values, rdeg, dout)
    assert np.isfinite(dv).all() and (dbound > 0).all()
    faults = {"row half of t_c missing": dict(halves=(False, True)), "column half of t_c missing": dict(halves=(True, False)),
              "a self loop counted once": dict(self_twice=False), "G taken at the row": dict(g_at="row"),
              "the factor -1/2 missing": dict(factor=1.0)}
    for what, kw in faults.items():
        other = OC.sym_bwd_ref(g, values, rdeg, dout, **kw)
        assert OC.moved(dv, other[0], dbound) > 4.0, (what, OC.moved(dv, other[0], dbound))
        if what != "G taken at the row":
            assert OC.moved(G, other[2], np.maximum(gbound, 1e-300)) > 4.0, what


def test_the_sym_norm_reference_is_autograd_of_the_dense_formula():
    """The backward formula against torch's fp64 autograd of A.sum(0) on a dense A built with index_put (directed, self
    loops)."""
    g = OC.graph("batch")
    v = torch.tensor(g.values.astype(np.float64), requires_grad=True)
    rows, cols = torch.from_numpy(g.rows), torch.from_numpy(g.indices.astype(np.int64))
    a = torch.zeros(g.n, g.n, dtype=torch.float64).index_put((rows, cols), v)
    r = a.sum(0).pow(-0.5)
    out = (r[:, None] * a * r[None, :])[rows, cols]
    dout = torch.from_numpy(OC.sym_bwd_inputs(("batch", "weighted"))[2].astype(np.float64))
    out.backward(dout)
    ref = OC.sym_fwd_ref(g, g.values)
    assert np.abs(out.detach().numpy() - ref[0]).max() < 1e-14
    dv = OC.sym_bwd_ref(g, g.values, ref[2], dout.numpy())[0]
    assert np.abs(v.grad.numpy() - dv).max() < 1e-13


# ------------------------------------------------------------------ mirror_perm, directed()
def _container(name, weighted=True):
    g = OC.graph(name)
    w = g.values if weighted else None
    if g.off is None:
        if g.directed:
            return CsrGraph.from_edges(g.n, g.rows, g.indices, "cpu", symmetric=False, weight=w)
        keep = g.rows <= g.indices                                   # one weight per unordered pair
        return CsrGraph.from_edges(g.n, g.rows[keep], g.indices[keep], "cpu", symmetric=True,
                                   weight=None if w is None else w[keep])
    gr = g.graph_of_row()[g.rows]
    parts = [(g.rows[gr == b] - g.off[b], g.indices[gr == b] - g.off[b], None if w is None else w[gr == b])
             for b in range(len(g.off) - 1)]
    return CsrBatch.from_edge_lists(np.diff(g.off), *zip(*[(s, d) for s, d, _ in parts]), "cpu", symmetric=False,
                                    weights=[p[2] for p in parts])


@pytest.mark.parametrize("name", ["t4-n577", "undirected", "batch"])
@pytest.mark.parametrize("weighted", [False, True], ids=["01", "weighted"])
def test_mirror_perm_and_directed_on_host_built_containers(name, weighted):
    g = OC.graph(name)
    c = _container(name, weighted)
    assert np.array_equal(c.indices.numpy(), g.indices) and (not weighted or np.array_equal(c.values.numpy(), g.values))
    m = c.mirror_perm
    assert m.dtype == torch.int32 and np.array_equal(m.numpy(), g.mirror) and c.mirror_perm is m      # cached
    d = c.directed()
    if g.directed:
        assert d is c and np.array_equal(c._t_perm.numpy(), g.mirror)
        return
    assert type(d) is type(c) and d is not c and c.indices_t is c.indices      # the original stays undirected
    assert d.indptr is c.indptr and d.indices is c.indices and d.values is c.values
    assert d.indices_t is not d.indices and d.indptr_t is not d.indptr
    assert torch.equal(d.indptr_t, c.indptr) and torch.equal(d.indices_t, c.indices)
    assert d._t_perm.dtype == torch.int64 and torch.equal(d._t_perm, m.long()) and d.mirror_perm is m
    if weighted:
        assert torch.equal(d.values_t, c.values[m.long()]) and d.weighted
        v = torch.rand(c.nnz, requires_grad=True)
        h = d.with_values(v)
        assert h.values is v and torch.equal(h.values_t, v.detach()[m.long()]) and not h.values_t.requires_grad
    else:
        assert d.values is None and d.values_t is None and not d.weighted


def test_directed_clones_the_local_indices_of_a_batch_and_keeps_an_edgeless_pad():
    b = CsrBatch.from_edge_lists([3, 2], [[0, 1], [0]], [[1, 2], [1]], "cpu", symmetric=True)
    d = b.directed()
    assert d.indices_t_local is not d.indices_local and torch.equal(d.indices_t_local, b.indices_local)
    assert d.indices_local is b.indices_local and b.indices_t_local is b.indices_local
    e = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    assert e.mirror_perm.numel() == 0 and e.directed().indices_t.numel() == 1
    lop = CsrGraph(torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"must store \(j, i\) beside every \(i, j\)"):
        lop.mirror_perm


# ------------------------------------------------------------------ what EdgeAttention calls
@pytest.mark.parametrize("norm", ["softmax", "sym"])
@pytest.mark.parametrize("name", ["undirected", "batch"])
def test_edge_attention_calls_the_new_entries_and_returns_a_container(monkeypatch, name, norm):
    lib = fake_lib(monkeypatch.setattr)
    c = _container(name)
    torch.manual_seed(0)
    att = EdgeAttention(3, 4, norm=norm)
    assert [n for n, _ in att.named_parameters()] == (["q.weight", "k.weight"] if norm == "softmax" else ["q.weight"])
    h = att(torch.rand(c.n, 3), c)
    assert type(h) is type(c) and h.weighted and h.values.shape == (c.nnz,) and h.values.requires_grad
    assert h.indptr is c.indptr and h.indices is c.indices
    assert (h.indices_t is not h.indices) == (norm == "softmax" or OC.graph(name).directed)
    h.values.sum().backward()
    names = [n for n, _ in lib.calls]
    if norm == "softmax":
        assert names == ["dp_bgemm_f32", "dp_bgemm_f32", "dp_csr_sddmm", "dp_csr_edge_softmax_fwd",
                         "dp_csr_edge_softmax_bwd", "dp_csr_aggregate_w", "dp_csr_aggregate_w"] + ["dp_bgemm_f32"] * 2
        assert att.q.weight.grad is not None and att.k.weight.grad is not None
    else:
        assert names[:4] == ["dp_bgemm_f32", "dp_csr_sddmm", "dp_csr_sym_norm_fwd", "dp_csr_sym_norm_bwd"]
        assert names[4:6] == ["dp_csr_aggregate_w"] * 2 and att.q.weight.grad is not None
    by = {}
    for n, a in lib.calls:
        by.setdefault(n, []).append(a)
    sd = by["dp_csr_sddmm"][0]
    assert sd["alpha"] == pytest.approx(0.5) and sd["F"] == 4 and sd["n_rows"] == c.n and sd["beta"] == 0.0
    assert sd["indptr"] == c.indptr.data_ptr() and sd["indices"] == c.indices.data_ptr()
    dp_, dq = by["dp_csr_aggregate_w"]                               # dP over the CSR, dQ over the transposed one
    assert dp_["indices"] == c.indices.data_ptr() and dq["indices"] == c.indices_t.data_ptr()
    assert dp_["indptr"] == c.indptr.data_ptr() and dq["indptr"] == c.indptr_t.data_ptr()
    for n in ("dp_csr_edge_softmax_fwd", "dp_csr_sym_norm_fwd", "dp_csr_sym_norm_bwd"):
        for a in by.get(n, []):
            assert a["nnz"] == c.nnz and a.get("n_rows", a.get("n")) == c.n
    if norm == "sym":
        f = by["dp_csr_sym_norm_fwd"][0]
        assert (f["mirror"] is None) == (c.indices_t is c.indices) and f["values"] is not None
        assert by["dp_csr_sym_norm_bwd"][0]["mirror"] == c.mirror_perm.data_ptr()


def test_edge_attention_refusals_and_the_edgeless_batch(monkeypatch):
    with pytest.raises(ValueError, match="norm must be 'softmax' or 'sym'"):
        EdgeAttention(3, 4, norm="row")
    lib = fake_lib(monkeypatch.setattr)
    att = EdgeAttention(3, 4)
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        att(torch.rand(5, 3), torch.eye(5))
    e = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    for norm in ("softmax", "sym"):
        del lib.calls[:]
        h = EdgeAttention(3, 4, norm=norm)(torch.rand(5, 3), e)
        assert h.weighted and h.nnz == 0 and h.values.shape == (1,)          # the pad `with_values` keeps
        assert not [n for n, _ in lib.calls if n != "dp_bgemm_f32"]          # nothing stored: no edge launch
    with pytest.raises(ValueError, match=r"x has 2 features"):
        att(torch.rand(5, 2), e)
