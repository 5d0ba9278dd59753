"""The fused GAT convolution without a GPU: the new C entries' symbols, signatures and argument errors (every refusal comes
back before a launch), the Python restatement of dp_csr_gat_conv_plan over the table and a sweep, what the case table
reaches (every instantiation, both load forms at the same width, every layout, kind, slope and both head modes), the
kernels' resources from the built library, the forward and backward formulas against fp64 autograd of the dense masked
formulation, that the bounds of tests/csr_gat_conv_cases.py tell each planted fault from rounding while an fp32 emulation
of the kernels' order stays inside them, and the surface of `GatConv` and `ops.csr_gat_conv`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_gat_cases as GC
from tests import csr_gat_conv_cases as CC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR

NEW = ("dp_csr_gat_conv_plan", "dp_csr_gat_conv_fwd", "dp_csr_gat_conv_bwd")
KERNELS = ("k_gatc_fwd", "k_gatc_bwd_rows", "k_gatc_bwd_cols")
STATS = ("k_gatc_stats<4>", "k_gatc_stats<16>", "k_gatc_stats<64>")
FORMS = ((1, 1, 0), (1, 2, 0), (1, 4, 0), (1, 8, 0), (4, 1, 0), (4, 1, 1), (4, 2, 0), (4, 2, 1))


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
    assert names("dp_csr_gat_conv_plan") == ["n_rows", "nnz", "H", "C", "ldz", "z_misaligned", "plan_out"]
    assert names("dp_csr_gat_conv_fwd") == ["z", "ldz", "u", "ldu", "v", "ldv", "indptr", "indices", "y", "ldy", "rowstat",
                                            "n_rows", "nnz", "H", "C", "slope", "mean_heads", "stream"]
    assert names("dp_csr_gat_conv_bwd") == ["z", "ldz", "u", "ldu", "v", "ldv", "indptr", "indices", "indptr_t",
                                            "indices_t", "rowstat", "dy", "lddy", "tdot", "du", "lddu", "dv", "lddv", "dz",
                                            "lddz", "n", "nnz", "H", "C", "slope", "mean_heads", "stream"]
    assert "mirror" not in names("dp_csr_gat_conv_bwd")
    assert _lib.CSR_GAT_CONV_PLAN_INTS == 6 and _lib.CSR_GAT_CONV_MAX_WIDTH == CC.MAX_WIDTH == 512
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "diffpool_hip.h")).read()
    assert "#define DP_CSR_GAT_CONV_MAX_WIDTH 512" in header and "#define DP_CSR_GAT_CONV_PLAN_INTS 6" in header


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1 / -2."""
    buf = (C.c_float * 64)()
    ibuf = (C.c_int * 16)()
    p, i = C.addressof(buf), C.addressof(ibuf)
    inf, nan = float("inf"), float("nan")

    def fwd(z=p, ldz=8, u=p, ldu=4, v=p, ldv=4, ip=i, ix=i, y=p, ldy=8, rs=p, n=2, nnz=4, H=4, Cc=2, slope=0.2, mean=0):
        return lib.dp_csr_gat_conv_fwd(z, ldz, u, ldu, v, ldv, ip, ix, y, ldy, rs, n, nnz, H, Cc, slope, mean, None)

    for kw, text in ((dict(z=None), "z is NULL"), (dict(u=None), "u is NULL"), (dict(v=None), "v is NULL"),
                     (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"), (dict(y=None), "y is NULL"),
                     (dict(rs=None), "rowstat is NULL"), (dict(z=p + 2), "z is not 4-byte"),
                     (dict(y=p + 1), "y is not 4-byte"), (dict(ldz=7), "ldz=7 smaller than its width 8"),
                     (dict(ldu=3), "ldu=3 smaller than its width 4"), (dict(ldv=3), "ldv=3 smaller than its width 4"),
                     (dict(ldy=7), "ldy=7 smaller than its width 8"), (dict(ldy=1, mean=1), "ldy=1 smaller than its width 2"),
                     (dict(n=-1), "n_rows=-1 must not be negative"), (dict(nnz=-3), "nnz=-3 must not be negative"),
                     (dict(H=0), "H=0 must be 1 .. 8"), (dict(H=9, ldu=9, ldv=9, ldz=18, ldy=18), "H=9 must be 1 .. 8"),
                     (dict(Cc=0), "C=0 must be positive"), (dict(Cc=-2), "C=-2 must be positive"),
                     (dict(slope=inf), "slope must be finite"), (dict(slope=nan), "slope must be finite"),
                     (dict(mean=2), "mean_heads=2 must be 0 or 1"), (dict(mean=-1), "mean_heads=-1 must be 0 or 1")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    rc = fwd(Cc=129, ldz=516, ldy=516)                             # H C = 516 > 512: unsupported, not invalid
    assert rc < 0 and rc != -1 and "H * C = 516 outside the supported 1..512" in _err(lib)
    assert fwd(n=0) == 0 and fwd(n=0, nnz=0) == 0                  # nothing to do: OK, nothing launched

    def bwd(z=p, ldz=8, u=p, ldu=4, v=p, ldv=4, ip=i, ix=i, ipt=i, ixt=i, rs=p, dy=p, lddy=8, t=p, du=p, lddu=4, dv=p,
            lddv=4, dz=p, lddz=8, n=2, nnz=4, H=4, Cc=2, slope=0.2, mean=0):
        return lib.dp_csr_gat_conv_bwd(z, ldz, u, ldu, v, ldv, ip, ix, ipt, ixt, rs, dy, lddy, t, du, lddu, dv, lddv, dz,
                                       lddz, n, nnz, H, Cc, slope, mean, None)

    for kw, text in ((dict(z=None), "z is NULL"), (dict(u=None), "u is NULL"), (dict(v=None), "v is NULL"),
                     (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(ipt=None), "indptr_t is NULL"), (dict(ixt=None), "indices_t is NULL"),
                     (dict(rs=None), "rowstat is NULL"), (dict(dy=None), "dy is NULL"), (dict(t=None), "tdot is NULL"),
                     (dict(du=None), "du is NULL"), (dict(dv=None), "dv is NULL"), (dict(dz=None), "dz is NULL"),
                     (dict(dy=p + 3), "dy is not 4-byte"), (dict(ldz=7), "ldz=7 smaller"), (dict(ldu=3), "ldu=3 smaller"),
                     (dict(ldv=2), "ldv=2 smaller"), (dict(lddy=7), "lddy=7 smaller"),
                     (dict(lddy=1, mean=1), "lddy=1 smaller than its width 2"), (dict(lddu=1), "lddu=1 smaller"),
                     (dict(lddv=3), "lddv=3 smaller"), (dict(lddz=7), "lddz=7 smaller"), (dict(n=-1), "n=-1"),
                     (dict(nnz=-1), "nnz=-1"), (dict(H=0), "H=0 must be"), (dict(Cc=0), "C=0 must be positive"),
                     (dict(H=9, ldu=9, ldv=9, lddu=9, lddv=9, ldz=18, lddy=18, lddz=18), "H=9 must be"),
                     (dict(slope=-inf), "slope must be finite"), (dict(mean=3), "mean_heads=3 must be 0 or 1")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    rc = bwd(Cc=129, ldz=516, lddy=516, lddz=516)
    assert rc < 0 and rc != -1 and "outside the supported 1..512" in _err(lib)
    assert bwd(n=0) == 0 and bwd(n=0, nnz=0) == 0


def test_plan_restatement_equals_the_library(lib):
    out = (C.c_int * _lib.CSR_GAT_CONV_PLAN_INTS)()
    for case in CC.CASES:
        g = CC.graph(case[0])
        W, wy = CC.widths(case)
        (ldz, off), (lddy, _) = CC.layout_of(case, W), CC.layout_of(case, wy)
        fplan, bplan = CC.case_plans(case)
        assert lib.dp_csr_gat_conv_plan(g.n, g.nnz, case[1], case[2], ldz, off, out) == 0
        assert tuple(out) == fplan, CC.case_id(case)
        mis = int(bool(off or (case[6] and case[2] % 4)))
        assert lib.dp_csr_gat_conv_plan(g.n, g.nnz, case[1], case[2], ldz | lddy, mis, out) == 0
        assert tuple(out) == bplan, CC.case_id(case)
    seen = set()
    for H in range(1, 9):
        for Cc in (1, 2, 3, 4, 5, 7, 8, 15, 16, 21, 32, 33, 63, 64, 65, 128, 170, 256, 512):
            if H * Cc > 512:
                continue
            W = H * Cc
            for ld, mis in ((W, 0), (W + 1, 0), (4 * (W // 4 + 1), 0), (4 * (W // 4 + 1), 1)):
                for n_rows, nnz in ((0, 0), (576, 8 * 576), (576, 8 * 576 + 1), (577, 32 * 577), (577, 32 * 577 + 1),
                                    (1 << 20, 6 << 20)):
                    assert lib.dp_csr_gat_conv_plan(n_rows, nnz, H, Cc, ld, mis, out) == 0
                    assert tuple(out) == CC.plan(n_rows, nnz, H, Cc, ld, mis), (n_rows, nnz, H, Cc, ld, mis)
                    assert out[4] * 64 >= W and out[3] == 4
                    seen.add(tuple(out)[:3] + (out[5],))
    assert seen == {f + (lanes,) for f in FORMS for lanes in (4, 16, 64)}
    for bad, text in (((-1, 4, 1, 1, 1, 0), "n_rows=-1"), ((4, -1, 1, 1, 1, 0), "nnz=-1"), ((4, 4, 0, 1, 1, 0), "H=0"),
                      ((4, 4, 9, 1, 9, 0), "H=9"), ((4, 4, 4, 0, 4, 0), "C=0"), ((4, 4, 4, 2, 7, 0), "ldz=7 smaller")):
        assert lib.dp_csr_gat_conv_plan(*bad, out) == -1 and text in _err(lib)
    assert lib.dp_csr_gat_conv_plan(4, 4, 8, 65, 520, 0, out) not in (0, -1) and "outside the supported" in _err(lib)
    assert lib.dp_csr_gat_conv_plan(4, 4, 1, 1, 1, 0, None) == -1 and "plan_out is NULL" in _err(lib)


def test_the_table_reaches_every_instantiation_and_edge():
    fwd, bwd, by_width, stats = set(), set(), {}, set()
    for case in CC.CASES:
        f, b = CC.case_plans(case)
        fwd.add(f[:3])
        bwd.add(b[:3])
        stats.add((f[5], case[1]))
        if case[0] in GC.TIER_GRAPHS:
            assert case[0].startswith(f"t{f[5]}-")
        by_width.setdefault((case[1], case[2]), set()).add(f[0])
    assert fwd == set(FORMS) and bwd == set(FORMS)
    assert stats >= {(lanes, H) for lanes in (4, 16, 64) for H in (1, 3, 4, 8)}   # every group size at one and more heads
    pairs = {(c[1], c[2]) for c in CC.CASES}
    assert pairs == set(CC.PAIRS) >= {(1, 1), (3, 21), (4, 16), (1, 65), (3, 5), (8, 1), (8, 64)}
    for H, Cc in CC.PAIRS:                                           # both load forms at the same width
        assert by_width[(H, Cc)] == ({1, 4} if H * Cc % 4 == 0 else {1})
        assert {(c[3], c[6]) for c in CC.CASES if (c[1], c[2]) == (H, Cc)} == {(l, m) for l in CC.LAYOUTS for m in (0, 1)}
        assert any(c[4] == "equal" for c in CC.CASES if (c[1], c[2]) == (H, Cc))
    for w in (1, 15, 63, 64, 65, 512):
        lds = {name: ld(w) for name, (ld, _) in CC.LAYOUTS.items()}
        assert lds["tight"] == w and lds["pad4"] % 4 == 0 and lds["pad4"] > w and lds["odd"] % 2 == 1 and lds["odd"] > w
    assert CC.LAYOUTS["mis"][1] == 1
    assert {c[4] for c in CC.CASES} == set(CC.KINDS) and {c[5] for c in CC.CASES} == set(CC.SLOPES)
    assert {c[0] for c in CC.CASES} == set(CC.GRAPHS) == set(GC.GRAPHS) | {"tiny"}
    assert {(c[5], c[6]) for c in CC.CASES} == {(s, m) for s in CC.SLOPES for m in (0, 1)}
    assert {c[5] for c in CC.CASES if c[4] == "kink"} == set(CC.SLOPES)
    for name in GC.TIER_GRAPHS:                                      # the planted rows: none, one, the batch edge, the hub
        lens = CC.row_len(CC.graph(name))
        assert tuple(lens[:len(GC.PLANTED)]) == GC.PLANTED and {0, 1, 3, 4, 5, 63, 64, 65, 128, 530} <= set(lens)
        assert CC.graph(name).n % 4 == int(name.endswith("577"))     # the last workgroup full, and with one row
    tiny = CC.graph("tiny")
    assert (CC.col_len(tiny) == 0).any() and (CC.row_len(tiny) == 0).any() and (tiny.rows == tiny.indices).any()
    assert ((CC.col_len(tiny) == 0) & (CC.row_len(tiny) == 1)).any()       # a one-entry row that nobody points at
    assert list(np.diff(CC.graph("batch").off)) == [37, 1, 64, 98]


def test_the_inputs_are_what_their_names_say():
    for case in CC.CASES:
        if case[3] != "tight" and case[4] == "ordinary":
            continue                                                 # the layouts share their inputs' construction
        g = CC.graph(case[0])
        z, u, v, dy = CC.inputs(case)                                # asserts the margin from the kink
        W, wy = CC.widths(case)
        assert z.shape == (g.n, W) and dy.shape == (g.n, wy) and u.shape == v.shape == (g.n, case[1])
        lens = CC.row_len(g)
        y, bound, _, _ = CC.fwd_ref(g, z, u, v, case[5], case[2], case[6])
        assert np.isfinite(y).all() and (bound > 0).all() and not y[lens == 0].any()
        if not case[6]:
            one = np.nonzero(lens == 1)[0]
            assert one.size or case[0] in ("undirected", "batch")
            assert np.array_equal(y[one], z[g.indices[g.indptr[one]]].astype(np.float64))
        if case[4] == "equal":
            assert np.array_equal(z * 64, np.rint(z * 64))


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_gat_conv_kernels_use_no_scratch_no_lds_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if d["name"].startswith("k_gatc_")}
    want = [f"{k}<{vec},{nch},{uni}>" for k in KERNELS for vec, nch, uni in FORMS] + list(STATS)
    assert sorted(n.replace(" ", "") for n in ks) == sorted(want)
    for d in ks.values():
        assert d["scratch"] == 0 and d["lds_static"] == 0, d
        assert d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 256 and d.get("agprs", 0) == 0, d


# ------------------------------------------------------------------ the formulas are autograd's
@pytest.mark.parametrize("H,Cc,slope,mean", [(1, 3, 0.2, 0), (3, 5, 0.2, 0), (3, 5, 0.2, 1), (4, 2, 0.0, 1), (2, 4, 1.0, 0)])
def test_the_reference_is_autograd_of_the_dense_masked_formulation(H, Cc, slope, mean):
    """y and the backward formulas against torch's fp64 autograd of a dense masked softmax of leaky_relu(u_i + v_j)
    multiplied into z per head, the kink planted (torch's leaky_relu takes the derivative `slope` at 0)."""
    case = ("batch", H, Cc, "tight", "kink", slope, mean)
    g = CC.graph("batch")
    z32, u32, v32, dy32 = CC.inputs(case)
    z, u, v = (torch.tensor(t.astype(np.float64), requires_grad=True) for t in (z32, u32, v32))
    rows, cols = torch.from_numpy(g.rows), torch.from_numpy(g.indices.astype(np.int64))
    mask = torch.zeros(g.n, g.n, dtype=torch.bool).index_put((rows, cols), torch.tensor(True))
    s = torch.nn.functional.leaky_relu(u[:, None, :] + v[None, :, :], float(np.float32(slope)))       # [n, n, H]
    a = torch.softmax(s.masked_fill(~mask[:, :, None], -float("inf")), dim=1)
    a = torch.where(mask.any(1)[:, None, None], a, torch.zeros_like(a))                # a row without entries: zeros
    Y = torch.einsum("ijh,jhc->ihc", a, z.view(g.n, H, Cc))
    y = Y.mean(1) if mean else Y.reshape(g.n, H * Cc)
    ref, _, stat, _ = CC.fwd_ref(g, z32, u32, v32, slope, Cc, mean)
    assert np.abs(y.detach().numpy() - ref).max() < 1e-13
    y.backward(torch.from_numpy(dy32.astype(np.float64)))
    got = CC.bwd_ref(g, z32, u32, v32, stat, dy32, slope, Cc, mean)
    for name, grad in (("du", u.grad), ("dv", v.grad), ("dz", z.grad)):
        assert np.abs(grad.numpy() - got[name][0]).max() < 1e-12, name
    assert (GC._scores(g, u32, v32, slope)[0] == 0).any()


# ------------------------------------------------------------------ the bounds tell a bug from rounding
@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_an_fp32_evaluation_in_the_kernels_order_stays_inside(case):
    g = CC.graph(case[0])
    z, u, v, dy = CC.inputs(case)
    H, Cc, slope, mean = case[1], case[2], case[5], case[6]
    ref, bound, stat, sbound = CC.fwd_ref(g, z, u, v, slope, Cc, mean)
    y, rs = CC.emulate_fwd(g, z, u, v, slope, Cc, mean)
    assert CC.moved(ref, y, bound) <= 1.0, CC.moved(ref, y, bound)
    assert CC.moved(stat, rs, sbound) <= 1.0, CC.moved(stat, rs, sbound)
    lens = CC.row_len(g)
    if not mean:
        one = np.nonzero(lens == 1)[0]
        assert np.array_equal(y[one], z[g.indices[g.indptr[one]]])                     # bit for bit
    if case[4] == "equal":
        pow2 = ((lens & (lens - 1)) == 0) & (lens > 0)
        assert pow2.sum() >= 5 and (mean or np.array_equal(y[pow2].astype(np.float64), ref[pow2]))
    bplan = CC.case_plans(case)[1]
    want = CC.bwd_ref(g, z, u, v, rs, dy, slope, Cc, mean)
    got = CC.emulate_bwd(g, z, u, v, rs, dy, slope, Cc, mean, bplan[0], bplan[2])
    for name in ("du", "dv", "dz", "t"):
        ratio = CC.moved(want[name][0], got[name], want[name][1])
        assert ratio <= 1.0, (name, ratio)
    assert not got["du"][lens <= 1].any()                            # no entry, one entry: exactly 0


def _first_case_moved(fault):
    """The largest move of `fault(case)` (None: the fault does not apply to the case) over the table, in bounds; stops
    at the first case beyond 4."""
    worst = 0.0
    for case in CC.CASES:
        if case[1] * case[2] > 130:
            continue                                                 # the narrow cases tell every fault
        m = fault(case)
        if m is not None:
            worst = max(worst, m)
            if worst > 4.0:
                break
    return worst


def _fwd_fault(applies=lambda c: True, **kw):
    def fault(case):
        if not applies(case):
            return None
        g = CC.graph(case[0])
        z, u, v, _ = CC.inputs(case)
        ref, bound = CC.fwd_ref(g, z, u, v, case[5], case[2], case[6])[:2]
        return CC.moved(ref, CC.fwd_ref(g, z, u, v, case[5], case[2], case[6], **kw)[0], bound)
    return fault


def _bwd_fault(which, applies=lambda c: True, **kw):
    def fault(case):
        if not applies(case):
            return None
        g = CC.graph(case[0])
        z, u, v, dy = CC.inputs(case)
        stat = CC.bwd_stat(case)
        good = CC.bwd_ref(g, z, u, v, stat, dy, case[5], case[2], case[6])
        bad = CC.bwd_ref(g, z, u, v, stat, dy, case[5], case[2], case[6], **kw)
        return max(CC.moved(good[k][0], bad[k][0], good[k][1]) for k in which)
    return fault


def _empty_fault(name, lens_of):
    """An empty row's du / an empty column's dz left as the buffer held it (NaN)."""
    def fault(case):
        g = CC.graph(case[0])
        empty = lens_of(g) == 0
        if not empty.any():
            return None
        z, u, v, dy = CC.inputs(case)
        val, bound = CC.bwd_ref(g, z, u, v, CC.bwd_stat(case), dy, case[5], case[2], case[6])[name]
        assert not val[empty].any()
        return CC.moved(val, np.where(empty[:, None], np.nan, val), bound)
    return fault


FAULTS = {
    "a row's last entry dropped": _fwd_fault(drop_last=True),
    "v_j read at the wrong head": _fwd_fault(lambda c: c[1] > 1, v_head=1),
    "the feature slice of the neighbouring head": _fwd_fault(lambda c: c[1] > 1, slice_off=1),
    "the feature slice off by C": lambda c: None if c[1] == 1 else _fwd_fault(slice_off=c[2])(c),
    "the last partial column chunk dropped": _fwd_fault(lambda c: not c[6] and (c[1] * c[2]) % 64 != 0, drop_chunk=True),
    "1 / H missing in the forward's mean": _fwd_fault(lambda c: c[6] and c[1] > 1, no_mean=True),
    "1 / H missing in the backward's mean": _bwd_fault(("du", "dv", "dz"), lambda c: c[6] and c[1] > 1, no_mean=True),
    "derivative 1 at the kink": _bwd_fault(("du", "dv"), lambda c: c[4] == "kink" and c[5] != 1.0, kink_one=True),
    "t of the wrong row": _bwd_fault(("du", "dv"), t_shift=1),
    "the source row's rowstat replaced by the column's": _bwd_fault(("dv", "dz"), own_stats=True),
    "dz gathered over A instead of A^T": _bwd_fault(("dz",), lambda c: c[0] != "undirected", over_a=True),
    "slope ignored in the backward": _bwd_fault(("du", "dv"), lambda c: c[5] != 1.0, no_slope=True),
    "an empty row's du left unwritten": _empty_fault("du", CC.row_len),
    "an empty column's dz left unwritten": _empty_fault("dz", CC.col_len),
}


@pytest.mark.parametrize("what", list(FAULTS))
def test_each_planted_fault_moves_the_reference_beyond_the_bound(what):
    assert _first_case_moved(FAULTS[what]) > 4.0, what


# ------------------------------------------------------------------ the surface of GatConv and ops.csr_gat_conv
def test_gat_conv_parameters_init_and_state_dict():
    import graph_pooling_amd
    from graph_pooling_amd.sparse import GatConv
    assert graph_pooling_amd.GatConv is GatConv and "GatConv" in graph_pooling_amd.__all__
    torch.manual_seed(0)
    m = GatConv(5, 4, heads=3)
    assert list(m.state_dict()) == ["a_src", "a_dst", "bias", "lin.weight"]
    assert m.lin.weight.shape == (12, 5) and m.lin.bias is None and m.a_src.shape == m.a_dst.shape == (3, 4)
    assert m.bias.shape == (12,) and not m.bias.any() and all(p.requires_grad for p in m.parameters())
    assert (m.heads, m.concat, m.negative_slope, m.out_dim) == (3, True, 0.2, 4)
    gain = torch.nn.init.calculate_gain("relu")
    for p in (m.lin.weight, m.a_src, m.a_dst):                       # Xavier-uniform, ReLU gain: inside its range, not zero
        lim = gain * (6.0 / (p.shape[0] + p.shape[1])) ** 0.5
        assert 0 < float(p.detach().abs().max()) <= lim and float(p.detach().abs().max()) > 0.5 * lim
    mean = GatConv(5, 4, heads=3, concat=False, negative_slope=0.1)
    assert mean.bias.shape == (4,) and mean.lin.weight.shape == (12, 5) and mean.negative_slope == 0.1
    assert list(GatConv(5, 4, bias=False).state_dict()) == ["a_src", "a_dst", "lin.weight"]
    assert GatConv(5, 4, bias=False).bias is None and GatConv(5, 4).heads == 1
    assert GatConv(5, 64, heads=8).bias.shape == (512,)
    doc = GatConv.__doc__
    assert "NO self loops" in doc and "exactly its stored\n    entries" in doc and "gets `bias`" in doc and "(i, i)" in doc


def test_gat_conv_refusals():
    from graph_pooling_amd.sparse import GatConv
    for heads in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="heads must be 1 .. 8"):
            GatConv(5, 4, heads=heads)
    for heads, out_dim in ((8, 65), (1, 513), (2, 0)):
        with pytest.raises(ValueError, match="heads \\* out_dim must be 1 .. 512"):
            GatConv(5, out_dim, heads=heads)
    with pytest.raises(ValueError, match="negative_slope must be finite"):
        GatConv(5, 4, negative_slope=float("inf"))
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        GatConv(5, 4)(torch.rand(3, 5), torch.eye(3))


def test_csr_gat_conv_refusals_and_the_edgeless_container():
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrBatch
    e = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    z, u, v = torch.rand(5, 6), torch.rand(5, 2), torch.rand(5, 2)
    out = ops.csr_gat_conv(z, u, v, e, 2)
    assert out.shape == (5, 6) and out.dtype == torch.float32 and not out.any()
    assert ops.csr_gat_conv(z, u, v, e, 2, concat=False).shape == (5, 3)
    with pytest.raises(ValueError, match=r"expected z \[n, heads \* C\] with n = 5"):
        ops.csr_gat_conv(torch.rand(4, 6), u, v, e, 2)
    with pytest.raises(ValueError, match=r"expected v \[n, heads\] with n = 5"):
        ops.csr_gat_conv(z, u, torch.rand(5), e, 2)
    with pytest.raises(ValueError, match=r"u and v must be \[n, heads\] with heads = 2"):
        ops.csr_gat_conv(z, u, torch.rand(5, 3), e, 2)
    with pytest.raises(ValueError, match="not a positive multiple of heads = 4"):
        ops.csr_gat_conv(z, torch.rand(5, 4), torch.rand(5, 4), e, 4)
    with pytest.raises(ValueError, match="more than the supported heads \\* C <= 512"):
        ops.csr_gat_conv(torch.rand(5, 516), u, v, e, 2)
    for heads in (0, 9, 2.0):
        with pytest.raises(ValueError, match="heads must be 1 .. 8"):
            ops.csr_gat_conv(z, u, v, e, heads)
    with pytest.raises(ValueError, match="negative_slope must be finite"):
        ops.csr_gat_conv(z, u, v, e, 2, float("nan"))
    b = CsrBatch.from_edge_lists([2, 3], [[0], [0]], [[1], [1]], "cpu")
    with pytest.raises(RuntimeError, match="must be a tensor on the GPU"):
        ops.csr_gat_conv(z, u, v, b, 2)
