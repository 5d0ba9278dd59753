"""CPU checks of the ragged Set2Set entries (dp_set2set_ragged_*): the host-only plan and size queries, the argument
checks that come before any launch, the SparseGcnSet2SetEncoder class surface, the kernels' register / LDS budget, and
the case table of tests/set2set_ragged_cases.py — it reaches every kernel variant, and its bound (set2set_cases.
anchor_bound) tells three restatement errors from rounding on every short row."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import GcnSet2SetEncoder
from tests import set2set_ragged_cases as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ------------------------------------------------------------------ plan and sizes
def test_plan_edges_and_refusals(lib):
    plan = lib.dp_set2set_ragged_plan
    assert plan(1, 1) == RS.W_REGS | RS.E_LDS and plan(100, 64) == RS.W_REGS | RS.E_LDS
    assert plan(5748, 60) == RS.W_REGS and plan(40, 65) == RS.E_LDS and plan(5748, 65) == 0
    # the stated bound holds at EVERY width, and leaves room above DD's largest graph (5 748 nodes): at least 8192 rows
    assert RS.MAX_ROWS >= 8192
    for d in (1, 64, 65, 128, 256):
        assert plan(RS.MAX_ROWS, d) >= 0 and plan(8192, d) >= 0, d
        assert plan(RS.MAX_ROWS + 1, d) == RS.ERR_UNSUPPORTED, d
    for n, d in ((0, 60), (-1, 60), (100, 0), (100, 257)):
        assert plan(n, d) == RS.ERR_UNSUPPORTED, (n, d)
    assert all(not plan(n, d) & 1 for n in (1, 100, 5000) for d in (8, 66, 256))       # bit 0 is never set
    # the embedding's edge: [n][d] floats beside 7 d + 2 n + ~1100 floats of vectors in 158 KiB
    for d in (8, 64, 256):
        e = RS.el_edge(d)
        assert 4 * (e * d + 7 * d + 2 * e + 1200) >= 158 * 1024 - 4 * (d + 64) > 4 * (e * d + 7 * d + 2 * e), (d, e)


def test_table_reaches_every_variant_and_edge(lib):
    seen = {RS.VARIANTS[lib.dp_set2set_ragged_plan(n, d)] for sizes, T, d, _ in RS.CASES for n in sizes}
    assert seen == set(RS.VARIANTS.values()), seen
    rows = {n for sizes, _, _, _ in RS.CASES for n in sizes}
    assert {1, 15, 16, 17, 63, 64, 65} <= rows and max(rows) > 1024
    assert {64, 65, 69, 70, 128, 129, 256} <= {d for _, _, d, _ in RS.CASES}
    for d in (64, 256):                                   # both sides of the LDS edge, in ONE batch (two grids)
        e = RS.el_edge(d)
        assert any(d == dd and {e, e + 1} <= set(sizes) for sizes, _, dd, _ in RS.CASES), d
    assert any(T > max(sizes) for sizes, T, _, _ in RS.CASES)
    assert any(len(sizes) == 1 and T == sizes[0] for sizes, T, _, _ in RS.CASES)
    assert any(all(n == T for n in sizes) and kind == "neg" for sizes, T, _, kind in RS.CASES)
    assert all(T >= max(sizes) for sizes, T, _, _ in RS.CASES) and len(RS.SHORT) >= 8


def test_size_queries_grow_as_T_times_n_total(lib):
    def sizes_of(sizes, T, d):
        off = _off(sizes)
        return (lib.dp_set2set_ragged_save_bytes(off.ctypes.data, len(sizes), T, d),
                lib.dp_set2set_ragged_bwd_workspace_bytes(off.ctypes.data, len(sizes), T, d))
    d = 16
    s1, w1 = sizes_of([100, 50], 100, d)
    s2, w2 = sizes_of([200, 100], 200, d)               # T and n_total doubled: the T x n_total arrays grow 4 x
    lstm = 4 * 2 * 100 * d                               # bytes of one [B, T, d] array at the first shape
    assert 4 * 100 * 150 <= s1 <= 4 * 100 * 150 + 9 * lstm + 8192
    assert 4 * 100 * 150 <= w1 <= 4 * 100 * 150 + 6 * lstm + 4 * 2 * d * (4 * d + 1) + 8192
    assert s2 - s1 >= 3 * 4 * 100 * 150 and w2 - w1 >= 3 * 4 * 100 * 150
    # 64-bit sizes: T * n_total past 2^31 elements
    big = [16384] * 9
    s, w = sizes_of(big, 16384, 8)
    assert s >= 4 * 16384 * 16384 * 9 > 2 ** 33 and w >= 4 * 16384 * 16384 * 9
    # what the entries refuse sizes to 0
    assert sizes_of([10, 20], 19, 8) == (0, 0) and sizes_of([10, 0], 19, 8) == (0, 0)
    assert sizes_of([10], 10, 257) == (0, 0) and sizes_of([RS.MAX_ROWS + 1], RS.MAX_ROWS + 1, 8) == (0, 0)


def test_argument_errors_come_before_any_launch(lib):
    """No GPU here: an entry that got as far as a launch would fail with a HIP error (> 0), not with DP_ERR_*.  The
    pointers are host addresses that are never read."""
    d = 8
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def fwd(sizes, T, d_, lde=None, save=p, save_bytes=1 << 40, emb=p):
        off = _off(sizes)
        return lib.dp_set2set_ragged_fwd(emb, d_ if lde is None else lde, p, off.ctypes.data, len(sizes), T, d_, p, p, p,
                                         p, p, p, p, save, save_bytes, None)

    def bwd(sizes, T, d_, ldde=None, save_bytes=1 << 40, ws_bytes=1 << 40):
        off = _off(sizes)
        return lib.dp_set2set_ragged_bwd(p, d_, p, off.ctypes.data, len(sizes), T, d_, p, p, p, p, p, p, p, p, p,
                                         d_ if ldde is None else ldde, p, p, p, p, p, p, p, save_bytes, p, ws_bytes, None)

    for call in (fwd, bwd):
        assert call([10, 20], 19, d) == RS.ERR_INVALID                       # T < max n_b
        assert b"T=19" in lib.dp_last_error_string()
        assert call([10, 20], 20, 0) == RS.ERR_INVALID                       # d = 0
        assert call([10, 20], 20, 257) == RS.ERR_UNSUPPORTED                 # d = 257
        assert call([5, RS.MAX_ROWS + 1], RS.MAX_ROWS + 1, d) == RS.ERR_UNSUPPORTED
        assert b"16384" in lib.dp_last_error_string()
        assert call([10, 0, 3], 20, d) == RS.ERR_INVALID                     # an empty graph
        assert call([10, 20], 20, d, save_bytes=1024) == RS.ERR_INVALID      # save buffer too small
        assert b"save buffer too small" in lib.dp_last_error_string()
    assert fwd([10, 20], 20, d, lde=d - 1) == RS.ERR_INVALID
    assert bwd([10, 20], 20, d, ldde=d - 1) == RS.ERR_INVALID
    assert fwd([10, 20], 20, d, emb=None) == RS.ERR_INVALID
    assert fwd([10, 20], 20, d, emb=p + 2) == RS.ERR_INVALID                 # not 4-byte aligned
    assert bwd([10, 20], 20, d, ws_bytes=1024) == -2                          # DP_ERR_WORKSPACE
    # B = 0 launches nothing and is DP_OK in the forward (nothing to write)
    off = _off([])
    assert lib.dp_set2set_ragged_fwd(p, d, p, off.ctypes.data, 0, 5, d, p, p, p, p, p, p, p, None, 0, None) == 0


# ------------------------------------------------------------------ the class surface
def test_class_state_dict_and_refusals():
    from graph_pooling_amd import SparseGcnSet2SetEncoder
    from graph_pooling_amd.sparse import CsrBatch
    for bn in (True, False):
        kw = dict(pred_hidden_dims=[10], bn=bn)
        torch.manual_seed(5)
        dense = GcnSet2SetEncoder(7, 12, 9, 3, 3, **kw)
        torch.manual_seed(5)
        sparse = SparseGcnSet2SetEncoder(7, 12, 9, 3, 3, **kw)
        assert list(sparse.state_dict()) == list(dense.state_dict())
        assert all(torch.equal(v, sparse.state_dict()[k]) for k, v in dense.state_dict().items())
        sparse.load_state_dict(dense.state_dict())
    with pytest.raises(NotImplementedError, match="dropout on the CSR path"):
        SparseGcnSet2SetEncoder(7, 12, 9, 3, 3, dropout=0.5)
    with pytest.raises(NotImplementedError, match="concat=False"):
        SparseGcnSet2SetEncoder(7, 12, 9, 3, 3, concat=False)
    m = SparseGcnSet2SetEncoder(7, 12, 9, 3, 3)
    batch = CsrBatch.from_edge_lists([3, 4], [np.array([0, 1]), np.array([0, 1, 2])],
                                     [np.array([1, 2]), np.array([1, 2, 3])], "cpu")
    with pytest.raises(ValueError, match=r"expected x \[n_total, F\] with n_total = 7"):
        m(torch.zeros(6, 7), batch)
    with pytest.raises(ValueError, match=r"expected x \[n_total, F\]"):
        m(torch.zeros(2, 7, 7), batch)
    with pytest.raises(ValueError, match="x has 5 features"):
        m(torch.zeros(7, 5), batch)
    with pytest.raises(TypeError, match="GcnSet2SetEncoder's"):
        m(torch.zeros(2, 5, 7), torch.zeros(2, 5, 5))
    with pytest.raises(RuntimeError, match="must be a tensor on the GPU"):
        m(torch.zeros(7, 7), batch)
    with pytest.raises(ValueError, match="one class per row"):
        m.loss(torch.zeros(2, 3), torch.zeros(3, dtype=torch.int64))


# ------------------------------------------------------------------ the bound tells an error from rounding
@pytest.mark.parametrize("case", RS.SHORT, ids=RS.case_id)
def test_bound_tells_a_restatement_error_from_rounding(case):
    """On every row with T <= 64: the restatement on ragged rows IS the oracle on the padded batch (1e-12), the fp32
    oracle sits inside anchor_bound, and each wrong restatement — one padded row too few in Z, T - 1 steps, and on the
    'neg' rows with padding the clamp of m forgotten for the real rows — sits outside it."""
    sizes, T, d, kind = case
    (emb, params, _), r64, r32 = RS.case_references(case)
    bound, e_o32, scale = RS.anchor_bound(r64["out"], r32["out"])
    assert scale > 0 and float((r64["out"] > 0).double().mean()) >= 0.25      # a live ReLU output
    e64, p64 = emb.double(), {k: v.double() for k, v in params.items()}
    logits = []
    with torch.no_grad():
        same = RS.restated(e64, sizes, T, p64, logits=logits)
        wrong = {w: RS.restated(e64, sizes, T, p64, wrong=w) for w in ("pad-1", "steps-1", "noclamp")}
    assert float((same - r64["out"]).abs().max()) <= 1e-12 * scale
    assert e_o32 <= bound
    padded = any(n < T for n in sizes)
    if kind == "neg":
        top = max(float(e.max()) for e in logits)
        assert top < (-1.0 if padded else 0.0), top          # every real logit of every step is negative
    errs = {w: float((v - r64["out"]).abs().max()) for w, v in wrong.items()}
    print(f"{RS.case_id(case)}: bound {bound:.3e} (oracle32 {e_o32:.3e}, scale {scale:.3e}); " +
          ", ".join(f"{w} {e:.3e}" for w, e in errs.items()))
    assert errs["pad-1"] > bound and errs["steps-1"] > bound, errs
    if kind == "neg" and padded:
        assert errs["noclamp"] > bound, errs
    if not padded:
        assert errs["noclamp"] <= 1e-12 * scale              # without padding there is no clamp to forget


# ------------------------------------------------------------------ kernel resources
def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libdiffpool_hip.so not built")
def test_ragged_set2set_kernels_do_not_spill_and_fit_lds():
    """1024 threads, one workgroup per CU, thousands of sequential steps: a spill is a scratch round trip in every step.
    Static LDS of the contraction kernel and the launchers' dynamic LDS (158 KiB at most) stay within 160 KiB."""
    res = KR.kernel_resources(_lib.LIB_PATH)
    ks = {v["name"]: v for v in res.values() if v["name"].startswith(("k_set2set_ragged_", "k_s2sr_"))}
    assert sum(k.startswith("k_set2set_ragged_fwd<") for k in ks) == 4, sorted(ks)
    assert sum(k.startswith("k_set2set_ragged_bwd<") for k in ks) == 4, sorted(ks)
    assert sum(k.startswith("k_s2sr_demb<") for k in ks) == 3, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (name, v)
        assert v["lds_static"] <= 160 * 1024, (name, v)
        if name.startswith("k_set2set_ragged_"):
            assert v["vgprs"] <= 128 and v["lds_static"] == 0, (name, v)
    lib = _lib.load()
    for d in (1, 64, 65, 256):                 # the dynamic LDS the launcher asks for, from the plan's own arithmetic
        for n in (1, RS.el_edge(d), RS.el_edge(d) + 1, RS.MAX_ROWS):
            el = bool(lib.dp_set2set_ragged_plan(n, d) & RS.E_LDS)
            floats = 7 * d + 8 + 1024 + 32 + 2 * ((n + 15) // 16 * 16) + 16 + (n * d if el else 0)
            assert 4 * floats <= 158 * 1024, (n, d)
