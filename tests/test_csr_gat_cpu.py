"""The fused additive attention without a GPU: the new C entries' symbols, signatures and argument errors (every refusal
comes back before a launch), the Python restatement of dp_csr_gat_plan over the table and a sweep, what the case table
reaches (every instantiation, both load forms, both register edges and both workgroup edges of every tier), the kernels'
resources from the built library, the backward formulas against fp64 autograd of the dense masked formulation, that the
bounds of tests/csr_gat_cases.py tell each planted fault from rounding while an fp32 emulation of the kernels' order
stays inside them, and the surface of `EdgeAttention`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.sparse import EdgeAttention
from tests import csr_gat_cases as GC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR

NEW = ("dp_csr_gat_plan", "dp_csr_gat_fwd", "dp_csr_gat_bwd")
KERNELS = ("k_gat_fwd", "k_gat_bwd_rows", "k_gat_bwd_cols")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_and_bound(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[f][1]) == len(fns[f][1])
    assert names("dp_csr_gat_plan") == ["n_rows", "nnz", "H", "ldv", "v_misaligned", "plan_out"]
    assert names("dp_csr_gat_fwd") == ["u", "ldu", "v", "ldv", "indptr", "indices", "out", "rowstat", "n_rows", "nnz",
                                       "H", "slope", "stream"]
    assert names("dp_csr_gat_bwd") == ["u", "ldu", "v", "ldv", "indptr", "indices", "indptr_t", "indices_t", "mirror",
                                       "rowstat", "dout", "tdot", "du", "lddu", "dv", "lddv", "n", "nnz", "H", "slope",
                                       "stream"]
    assert _lib.CSR_GAT_PLAN_INTS == 5 and _lib.CSR_GAT_MAX_HEADS == GC.MAX_HEADS == 8
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "diffpool_hip.h")).read()
    assert "#define DP_CSR_GAT_MAX_HEADS 8" in header and "#define DP_CSR_GAT_PLAN_INTS 5" in header


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1."""
    buf = (C.c_float * 64)()
    ibuf = (C.c_int * 16)()
    p, i = C.addressof(buf), C.addressof(ibuf)
    inf, nan = float("inf"), float("nan")
    fwd = lambda u=p, ldu=4, v=p, ldv=4, ip=i, ix=i, out=p, rs=p, n=2, nnz=4, H=4, slope=0.2: lib.dp_csr_gat_fwd(
        u, ldu, v, ldv, ip, ix, out, rs, n, nnz, H, slope, None)
    for kw, text in ((dict(u=None), "u is NULL"), (dict(v=None), "v is NULL"), (dict(ip=None), "indptr is NULL"),
                     (dict(ix=None), "indices is NULL"), (dict(out=None), "out is NULL"),
                     (dict(rs=None), "rowstat is NULL"), (dict(v=p + 2), "v is not 4-byte"),
                     (dict(ldu=3), "ldu=3 smaller than H=4"), (dict(ldv=3), "ldv=3 smaller than H=4"),
                     (dict(n=-1), "n_rows=-1 must not be negative"), (dict(nnz=-3), "nnz=-3 must not be negative"),
                     (dict(H=0), "H=0 must be 1 .. 8"), (dict(H=9, ldu=9, ldv=9), "H=9 must be 1 .. 8"),
                     (dict(slope=inf), "slope must be finite"), (dict(slope=nan), "slope must be finite")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert fwd(n=0) == 0 and fwd(nnz=0) == 0                       # nothing to do: OK, nothing launched
    bwd = lambda u=p, ldu=4, v=p, ldv=4, ip=i, ix=i, ipt=i, ixt=i, mir=i, rs=p, g=p, t=p, du=p, lddu=4, dv=p, lddv=4, \
        n=2, nnz=4, H=4, slope=0.2: lib.dp_csr_gat_bwd(u, ldu, v, ldv, ip, ix, ipt, ixt, mir, rs, g, t, du, lddu, dv,
                                                       lddv, n, nnz, H, slope, None)
    for kw, text in ((dict(u=None), "u is NULL"), (dict(v=None), "v is NULL"), (dict(ip=None), "indptr is NULL"),
                     (dict(ix=None), "indices is NULL"), (dict(ipt=None), "indptr_t is NULL"),
                     (dict(ixt=None), "indices_t is NULL"), (dict(mir=None), "mirror is NULL"),
                     (dict(rs=None), "rowstat is NULL"), (dict(g=None), "dout is NULL"), (dict(t=None), "tdot is NULL"),
                     (dict(du=None), "du is NULL"), (dict(dv=None), "dv is NULL"), (dict(g=p + 3), "dout is not 4-byte"),
                     (dict(ldu=3), "ldu=3 smaller"), (dict(ldv=2), "ldv=2 smaller"), (dict(lddu=1), "lddu=1 smaller"),
                     (dict(lddv=3), "lddv=3 smaller"), (dict(n=-1), "n=-1"), (dict(nnz=-1), "nnz=-1"),
                     (dict(H=0), "H=0 must be"), (dict(H=9, ldu=9, ldv=9, lddu=9, lddv=9), "H=9 must be"),
                     (dict(slope=-inf), "slope must be finite")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert bwd(n=0) == 0 and bwd(n=0, nnz=0) == 0


def test_plan_restatement_equals_the_library(lib):
    out = (C.c_int * _lib.CSR_GAT_PLAN_INTS)()
    for case in GC.CASES:
        g = GC.graph(case[0])
        ld, off = GC.layout_of(case)
        assert lib.dp_csr_gat_plan(g.n, g.nnz, case[1], ld, off, out) == 0
        assert tuple(out) == GC.case_plan(case), GC.case_id(case)
    seen = set()
    for n_rows in (0, 1, 5, 576, 5748, 1 << 20):
        for nnz in sorted({0, 7, 8 * n_rows, 8 * n_rows + 1, 32 * n_rows, 32 * n_rows + 1, 6 << 20}):
            for H in range(1, 9):
                for ldv, mis in ((H, 0), (H + 1, 0), (4 * (H // 4 + 1), 0), (4 * (H // 4 + 1), 1)):
                    assert lib.dp_csr_gat_plan(n_rows, nnz, H, ldv, mis, out) == 0
                    assert tuple(out) == GC.plan(n_rows, nnz, H, ldv, mis), (n_rows, nnz, H, ldv, mis)
                    seen.add((out[0], H, out[1], out[2]))
    regs = {1: (8, 4), 2: (8, 4), 3: (5, 4), 4: (4, 4), 5: (3, 3), 6: (2, 2), 7: (2, 2), 8: (2, 2)}
    assert seen == {(l, H, vec, regs[H][l != 4]) for l in (4, 16, 64) for H in range(1, 9)
                    for vec in ((1, 4) if H % 4 == 0 else (1,))}
    for bad, text in (((-1, 4, 1, 1, 0), "n_rows=-1"), ((4, -1, 1, 1, 0), "nnz=-1"), ((4, 4, 0, 1, 0), "H=0"),
                      ((4, 4, 9, 9, 0), "H=9"), ((4, 4, 4, 3, 0), "ldv=3 smaller than H=4")):
        assert lib.dp_csr_gat_plan(*bad, out) == -1 and text in _err(lib)
    assert lib.dp_csr_gat_plan(4, 4, 1, 1, 0, None) == -1 and "plan_out is NULL" in _err(lib)


def test_the_table_reaches_every_instantiation_and_edge():
    forms, edges = set(), set()
    for case in GC.CASES:
        g = GC.graph(case[0])
        lanes, vec, regs, rows_per_wg, fit = GC.case_plan(case)
        forms.add((lanes, case[1], vec))
        if case[0] in GC.TIER_GRAPHS:
            assert case[0].startswith(f"t{lanes}-")
            lens = GC.row_len(g)
            assert tuple(lens[:len(GC.PLANTED)]) == GC.PLANTED
            assert fit in lens and fit + 1 in lens                   # the last row read once, the first read twice
            assert lens.max() == 530 > 2 * fit and set(range(10)) <= set(lens)
            edges.add((lanes, g.n % rows_per_wg))
            assert (g.rows == g.indices).any()
    assert forms == {(l, H, vec) for l in (4, 16, 64) for H in GC.HEADS for vec in ((1, 4) if H % 4 == 0 else (1,))}
    assert edges == {(l, e) for l in (4, 16, 64) for e in (0, 1)}
    layouts = {(c[1], c[2]) for c in GC.CASES}
    assert {(H, l) for H in (4, 8) for l in GC.LAYOUTS} <= layouts
    for H in GC.HEADS:                                               # ld == H, a multiple of 4 above H, odd; one float off
        lds = {name: ld(H) for name, (ld, _) in GC.LAYOUTS.items()}
        assert lds["tight"] == H and lds["pad4"] % 4 == 0 and lds["pad4"] > H and lds["odd"] % 2 == 1 and lds["odd"] > H
    assert GC.LAYOUTS["mis"][1] == 1
    assert {c[3] for c in GC.CASES} == set(GC.KINDS) and {c[4] for c in GC.CASES} == set(GC.SLOPES)
    assert {c[0] for c in GC.CASES} == set(GC.GRAPHS)
    assert {c[4] for c in GC.CASES if c[3] == "kink"} == set(GC.SLOPES)
    u = GC.graph("undirected")
    assert not u.directed and (u.rows == u.indices).sum() >= 2
    assert list(np.diff(GC.graph("batch").off)) == [37, 1, 64, 98]
    for name in GC.GRAPHS:                                           # the mirror is the transposition
        g = GC.graph(name)
        assert np.array_equal(g.rows[g.mirror], g.indices_t) and np.array_equal(g.indices[g.mirror], g.rows_t)


def test_the_inputs_are_what_their_names_say():
    for case in GC.CASES:
        g = GC.graph(case[0])
        u, v = GC.inputs(case)                                       # asserts the margin from the kink
        lens = GC.row_len(g)
        ref, bound, stat, _ = GC.fwd_ref(g, u, v, case[4])
        assert np.isfinite(ref).all() and (bound > 0).all()
        assert abs(np.bincount(g.rows, ref, g.n)[lens > 0] - 1).max() < 1e-12
        assert np.array_equal(ref[lens[g.rows] == 1], np.ones((lens[g.rows] == 1).sum()))
        if case[3] == "equal":
            pow2 = ((lens & (lens - 1)) == 0)[g.rows]
            assert pow2.any() and np.array_equal(ref[pow2], (1.0 / lens[g.rows])[pow2])
        if case[3] == "shift80":
            assert u.max() > 80 and u.min() < -80
        if case[3] == "below200":
            s = GC._scores(g, u, v, case[4])[1]
            assert ((stat[:, :case[1]][g.rows] - s).max(axis=1) >= 200).sum() >= g.nnz // 10
        if case[3] == "kink":
            pre = GC._scores(g, u, v, case[4])[0]
            assert (pre == 0).all(axis=1).sum() >= (lens[::3] > 0).sum()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_gat_kernels_use_no_scratch_no_lds_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if d["name"].startswith("k_gat_")}
    want = [f"{k}<{l}, {H}, {vec}>" for k in KERNELS for l in (4, 16, 64) for H in range(1, 9)
            for vec in ((1, 4) if H % 4 == 0 else (1,))]
    assert sorted(n.replace(" ", "") for n in ks) == sorted(w.replace(" ", "") for w in want)
    for d in ks.values():
        assert d["scratch"] == 0 and d["lds_static"] == 0, d
        assert d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 128, d


# ------------------------------------------------------------------ the formulas are autograd's
@pytest.mark.parametrize("H,slope", [(1, 0.2), (3, 0.2), (4, 0.0), (2, 1.0)])
def test_the_reference_is_autograd_of_the_dense_masked_formulation(H, slope):
    """out and the backward formulas against torch's fp64 autograd of a dense masked softmax of leaky_relu(u_i + v_j),
    the kink planted (torch's leaky_relu takes the derivative `slope` at 0)."""
    case = ("batch", H, "tight", "kink", slope)
    g = GC.graph("batch")
    u32, v32 = GC.inputs(case)
    u = torch.tensor(u32.astype(np.float64), requires_grad=True)
    v = torch.tensor(v32.astype(np.float64), requires_grad=True)
    rows, cols = torch.from_numpy(g.rows), torch.from_numpy(g.indices.astype(np.int64))
    mask = torch.zeros(g.n, g.n, dtype=torch.bool).index_put((rows, cols), torch.tensor(True))
    s = torch.nn.functional.leaky_relu(u[:, None, :] + v[None, :, :], float(np.float32(slope)))       # [n, n, H]
    a = torch.softmax(s.masked_fill(~mask[:, :, None], -float("inf")), dim=1)
    has = mask.any(1)
    out = a[has].mean(2)[mask[has]]                                  # row-major over the stored entries
    ref, _, stat, _ = GC.fwd_ref(g, u32, v32, slope)
    assert np.abs(out.detach().numpy() - ref).max() < 1e-14
    dout = np.random.default_rng(1).uniform(-1, 1, g.nnz)
    out.backward(torch.from_numpy(dout))
    du, _, dv, _, _, _ = GC.bwd_ref(g, u32, v32, stat, dout, slope)
    assert np.abs(u.grad.numpy() - du).max() < 1e-13 and np.abs(v.grad.numpy() - dv).max() < 1e-13
    assert (GC._scores(g, u32, v32, slope)[0] == 0).any()


# ------------------------------------------------------------------ the bounds tell a bug from rounding
@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_an_fp32_evaluation_in_the_kernels_order_stays_inside(case):
    g = GC.graph(case[0])
    u, v = GC.inputs(case)
    lanes, _, regs, _, _ = GC.case_plan(case)
    H = case[1]
    ref, bound, stat, sbound = GC.fwd_ref(g, u, v, case[4])
    out, rs = GC.emulate_fwd(g, u, v, case[4], lanes, regs)
    assert GC.moved(ref, out, bound) <= 1.0, GC.moved(ref, out, bound)
    assert GC.moved(stat, rs, sbound) <= 1.0, GC.moved(stat, rs, sbound)
    lens = GC.row_len(g)[g.rows]
    assert np.array_equal(out[lens == 1], np.ones((lens == 1).sum(), np.float32))
    if case[3] == "equal" and H in (1, 2, 4, 8):
        pow2 = (lens & (lens - 1)) == 0
        assert np.array_equal(out[pow2].astype(np.float64), 1.0 / lens[pow2])
    dout = GC.bwd_inputs(case)[1]
    du, dub, dv, dvb, t, tb = GC.bwd_ref(g, u, v, rs, dout, case[4])
    edu, edv, et = GC.emulate_bwd(g, u, v, rs, dout, case[4], lanes)
    for what, want, got, bd in (("du", du, edu, dub), ("dv", dv, edv, dvb), ("t", t, et, tb)):
        assert GC.moved(want, got, bd) <= 1.0, (what, GC.moved(want, got, bd))
    assert not edu[GC.row_len(g) <= 1].any()                         # no entry, one entry: exactly 0


def _first_case_moved(fault):
    """The largest move of `fault(case)` (None: the fault does not apply to the case) over the table, in bounds; stops
    at the first case beyond 4."""
    worst = 0.0
    for case in GC.CASES:
        m = fault(case)
        if m is not None:
            worst = max(worst, m)
            if worst > 4.0:
                break
    return worst


def _fwd_fault(**kw):
    def fault(case):
        g = GC.graph(case[0])
        u, v = GC.inputs(case)
        ref, bound = GC.fwd_ref(g, u, v, case[4])[:2]
        return GC.moved(ref, GC.fwd_ref(g, u, v, case[4], **kw)[0], bound)
    return fault


def _head_stride_fault(case):
    """Head h of node j read at j * H + h inside a buffer of leading dimension ld > H (zeros in the padding)."""
    g = GC.graph(case[0])
    H, (ld, _) = case[1], GC.layout_of(case)
    if ld == H:
        return None
    u, v = GC.inputs(case)
    ref, bound = GC.fwd_ref(g, u, v, case[4])[:2]
    bad = GC.padded(v, ld, 0.0).reshape(-1)[:g.n * H].reshape(g.n, H)
    return GC.moved(ref, GC.fwd_ref(g, u, bad, case[4])[0], bound)


def _bwd_fault(which, **kw):
    def fault(case):
        if kw.get("mean") is False and case[1] == 1:
            return None
        g = GC.graph(case[0])
        u, v = GC.inputs(case)
        stat, dout = GC.bwd_inputs(case)
        good = GC.bwd_ref(g, u, v, stat, dout, case[4])
        bad = GC.bwd_ref(g, u, v, stat, dout, case[4], **kw)
        return max(GC.moved(good[2 * k], bad[2 * k], good[2 * k + 1]) for k in which)
    return fault


def _empty_du_fault(case):
    """An empty row's du left as the buffer held it (NaN)."""
    g = GC.graph(case[0])
    u, v = GC.inputs(case)
    stat, dout = GC.bwd_inputs(case)
    du, dub = GC.bwd_ref(g, u, v, stat, dout, case[4])[:2]
    empty = GC.row_len(g) == 0
    if not empty.any():
        return None
    assert not du[empty].any()
    return GC.moved(du, np.where(empty[:, None], np.nan, du), dub)


FAULTS = {
    "1 / H missing in the forward": lambda c: None if c[1] == 1 else _fwd_fault(mean=False)(c),
    "the slope ignored": lambda c: None if c[4] == 1.0 else _fwd_fault(no_slope=True)(c),
    "the slope applied on the positive side": lambda c: None if c[4] == 1.0 else _fwd_fault(positive_side=True)(c),
    "a row's last entry dropped": _fwd_fault(drop_last=True),
    "head h read with stride H where ld is padded": _head_stride_fault,
    "1 / H missing in the backward": _bwd_fault((0, 1), mean=False),
    "derivative 1 at the kink": lambda c: None if c[3] != "kink" or c[4] == 1.0 else _bwd_fault((0, 1), kink_one=True)(c),
    "a row's last entry dropped from t": _bwd_fault((0, 1, 2), drop_last=True),
    "- t omitted": _bwd_fault((0, 1), minus_t=False),
    "dv with the column's own rowstat and t": _bwd_fault((1,), own_stats=True),
    "dout[k] read for dout[mirror[k]]": _bwd_fault((1,), mirror=False),
    "an empty row's du left unwritten": _empty_du_fault,
}


@pytest.mark.parametrize("what", list(FAULTS))
def test_each_planted_fault_moves_the_reference_beyond_the_bound(what):
    assert _first_case_moved(FAULTS[what]) > 4.0, what


# ------------------------------------------------------------------ the surface of EdgeAttention
def test_edge_attention_defaults_keep_their_parameters_and_the_additive_form_has_its_own():
    torch.manual_seed(0)
    old = EdgeAttention(5, 4)
    assert list(old.state_dict()) == ["q.weight", "k.weight"] and old.q.weight.shape == (4, 5)
    assert list(EdgeAttention(5, 4, norm="sym").state_dict()) == ["q.weight"]
    torch.manual_seed(0)
    q = torch.nn.Linear(5, 4, bias=False)
    k = torch.nn.Linear(5, 4, bias=False)
    assert torch.equal(old.q.weight, q.weight) and torch.equal(old.k.weight, k.weight)      # the same draws, in order
    assert (old.score, old.heads, old.negative_slope) == ("dot", 1, 0.2)
    att = EdgeAttention(5, 4, score="additive", heads=3, negative_slope=0.1)
    assert sorted(att.state_dict()) == ["a_dst", "a_src", "q.weight"]
    assert att.q.weight.shape == (12, 5) and att.a_src.shape == att.a_dst.shape == (3, 4) and att.q.bias is None
    assert all(p.requires_grad and p.abs().sum() > 0 for p in att.parameters())
    assert EdgeAttention(5, 4, score="additive").heads == 1


def test_edge_attention_refusals():
    with pytest.raises(ValueError, match="'additive'"):
        EdgeAttention(5, 4, heads=2)
    with pytest.raises(ValueError, match="score='additive' goes with norm='softmax'"):
        EdgeAttention(5, 4, norm="sym", score="additive")
    with pytest.raises(ValueError, match="score must be 'dot' or 'additive'"):
        EdgeAttention(5, 4, score="mlp")
    for heads in (0, 9, 2.0):
        with pytest.raises(ValueError, match="heads must be 1 .. 8"):
            EdgeAttention(5, 4, score="additive", heads=heads)
    with pytest.raises(ValueError, match="norm must be"):
        EdgeAttention(5, 4, norm="row", score="additive")


def test_csr_gat_attention_refusals_and_the_edgeless_container():
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrBatch
    e = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    out = ops.csr_gat_attention(torch.rand(5, 2), torch.rand(5, 2), e)
    assert out.shape == (0,) and out.dtype == torch.float32
    with pytest.raises(ValueError, match=r"expected u \[n, H\] with n = 5"):
        ops.csr_gat_attention(torch.rand(4, 2), torch.rand(5, 2), e)
    with pytest.raises(ValueError, match="share H heads"):
        ops.csr_gat_attention(torch.rand(5, 2), torch.rand(5, 3), e)
    with pytest.raises(ValueError, match="share H heads"):
        ops.csr_gat_attention(torch.rand(5, 9), torch.rand(5, 9), e)
    with pytest.raises(ValueError, match="negative_slope must be finite"):
        ops.csr_gat_attention(torch.rand(5, 2), torch.rand(5, 2), e, float("nan"))
    b = CsrBatch.from_edge_lists([2, 3], [[0], [0]], [[1], [1]], "cpu")
    with pytest.raises(RuntimeError, match="must be a tensor on the GPU"):
        ops.csr_gat_attention(torch.rand(5, 2), torch.rand(5, 2), b)
