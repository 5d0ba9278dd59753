"""Gradients to the stored values of a CSR adjacency, without a GPU: the new C entries' symbols, signatures and argument
errors (every refusal comes back before a launch), the Python restatement of dp_csr_sddmm_plan over the case table and
the table's coverage of every tier and load form, `with_values` of both containers, what the ops and the model classes
call (the recording library of tests/test_csr_host_cpu.py), and that the bounds of tests/csr_edge_grad_cases.py tell a
bug from rounding on the table's inputs."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import CsrBatch, CsrGraph
from tests import csr_edge_grad_cases as EC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_host_cpu import FIELDS, GOLDEN, MODEL_CASES, fake_lib

NEW = ("dp_csr_sddmm_plan", "dp_csr_sddmm", "dp_csr_link_dvalues", "dp_csr_pool_dvalues_workspace_bytes",
       "dp_csr_pool_dvalues", "dp_sparse_gcn_layer_bwd_dv")
DV_ENTRIES = ("dp_csr_link_dvalues", "dp_csr_pool_dvalues", "dp_sparse_gcn_layer_bwd_dv")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_with_the_parameters_the_host_layer_names(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
    assert names("dp_csr_sddmm") == ["P", "ldp", "Q", "ldq", "indptr", "indices", "out", "n_rows", "F", "alpha", "dscale",
                                     "beta", "stream"]
    assert names("dp_csr_sddmm_plan") == ["F", "ldp", "ldq", "p_misaligned", "q_misaligned", "plan_out"]
    assert names("dp_csr_link_dvalues") == ["S", "lds", "indptr", "indices", "values", "dvalues", "n_rows", "K",
                                            "objective", "inv_norm", "dloss", "stream"]
    assert names("dp_csr_pool_dvalues") == ["S", "lds", "indptr", "indices", "dAp", "node_off_host", "B", "dvalues",
                                            "n_total", "K", "workspace", "workspace_bytes", "stream"]
    old, new = names("dp_sparse_gcn_layer_bwd_w"), names("dp_sparse_gcn_layer_bwd_dv")
    at = old.index("n")
    assert new == old[:at] + ["x", "ldx", "dvalues"] + old[at:]      # the _w arguments plus x, ldx and dvalues


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1 / -2."""
    buf = (C.c_float * 64)()
    ibuf = (C.c_int * 8)(0, 0, 0, 0, 0, 0, 0, 0)
    p, i = C.addressof(buf), C.addressof(ibuf)
    sd = lambda P=p, ldp=4, Q=p, ldq=4, ip=i, ix=i, out=p, n=2, F=4: lib.dp_csr_sddmm(P, ldp, Q, ldq, ip, ix, out, n, F,
                                                                                      1.0, None, 0.0, None)
    for kw, text in ((dict(P=None), "P is NULL"), (dict(Q=None), "Q is NULL"), (dict(ip=None), "indptr is NULL"),
                     (dict(ix=None), "indices is NULL"), (dict(out=None), "out is NULL"), (dict(P=p + 2), "P is not 4-byte"),
                     (dict(n=-1), "n_rows=-1"), (dict(F=-1), "F=-1"), (dict(ldp=3), "ldp=3 smaller than F=4"),
                     (dict(ldq=3), "ldq=3 smaller than F=4")):
        assert sd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert sd(n=0) == 0 and sd(F=0) == 0                           # nothing to do: OK, nothing launched
    lk = lambda S=p, lds=4, ip=i, ix=i, dv=p, n=2, K=4, obj=0: lib.dp_csr_link_dvalues(S, lds, ip, ix, None, dv, n, K, obj,
                                                                                       0.25, None, None)
    for kw, text in ((dict(S=None), "S is NULL"), (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(dv=None), "dvalues is NULL"), (dict(n=-2), "n_rows=-2"), (dict(K=0), "K=0 must be positive"),
                     (dict(lds=3), "lds=3 smaller than K=4"), (dict(obj=2), "objective=2"), (dict(obj=-1), "objective=-1")):
        assert lk(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    big = lib.dp_csr_pool_dvalues_workspace_bytes(2, 4)
    assert big >= 2 * 4 * 4 and lib.dp_csr_pool_dvalues_workspace_bytes(5748, 50) < 2 * 5748 * 50 * 4
    off = (C.c_int * 3)(0, 1, 2)
    pl = lambda S=p, lds=4, ip=i, ix=i, dAp=p, off=None, B=1, dv=p, n=2, K=4, ws=p, wsb=big: lib.dp_csr_pool_dvalues(
        S, lds, ip, ix, dAp, off, B, dv, n, K, ws, wsb, None)
    for kw, text in ((dict(S=None), "S is NULL"), (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(dAp=None), "dAp is NULL"), (dict(dv=None), "dvalues is NULL"), (dict(n=-1), "n_total=-1"),
                     (dict(K=0), "K=0"), (dict(B=0), "B=0"), (dict(lds=2), "lds=2 smaller than K=4"),
                     (dict(B=2), "B=2 graphs need node_off_host"),
                     (dict(B=2, off=C.addressof(off), n=3), "not 0 .. n_total=3"), (dict(ws=None), "workspace is NULL")):
        assert pl(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert pl(wsb=big - 512) == -2 and "workspace too small" in _err(lib)
    # the GraphConv backward: the _w entry's refusals, then those of x / ldx / dvalues
    dv = lambda ax=p, values=p, x=p, ldx=4, dvalues=p, ixt=i, values_t=p: lib.dp_sparse_gcn_layer_bwd_dv(
        ax, i, i, values, i, ixt, values_t, p, p, 4, p, p, 4, p, 4, p, p, x, ldx, dvalues, 2, 4, 4, 0, p, 1 << 20, None)
    for kw, text in ((dict(ax=None), "ax is NULL"), (dict(values=None), "values is NULL"), (dict(x=None), "x is NULL"),
                     (dict(dvalues=None), "dvalues is NULL"), (dict(ldx=3), "ldx=3 smaller than Fin=4"),
                     (dict(ixt=i + 4, values_t=None), "dp_sparse_gcn_layer_bwd_dv: values_t is NULL")):
        assert dv(**kw) == -1 and text in _err(lib), (kw, _err(lib))


def test_plan_restatement_equals_the_library_over_the_table(lib):
    out = (C.c_int * _lib.CSR_SDDMM_PLAN_INTS)()
    seen = set()
    for case in EC.SDDMM_CASES:
        _, F, pp, pq, mis, _, _ = case
        assert lib.dp_csr_sddmm_plan(F, F + pp, F + pq, int(mis), int(mis), out) == 0
        assert tuple(out) == EC.plan(F, F + pp, F + pq, mis, mis), case
        seen.add(tuple(out)[:4])
    for K in EC.LINK_K:                                             # P = Q = S, contiguous and aligned
        assert lib.dp_csr_sddmm_plan(K, K, K, 0, 0, out) == 0 and tuple(out) == EC.plan(K, K, K, False, False)
    assert {(l, v) for l, v, _, _ in seen} == {(l, v) for l in (4, 16, 64) for v in (1, 4)}      # every tier, both forms
    assert {r for l, _, r, _ in seen if l == 64} == {1, 2, 3, 4} and {t for _, _, _, t in seen} == {0, 1}
    assert {(v, t) for l, v, _, t in seen if l == 64} == {(1, 0), (1, 1), (4, 0), (4, 1)}       # the column loop in both
    for bad, text in (((0, 4, 4), "F=0 must be positive"), ((4, 3, 4), "ldp=3 smaller"), ((4, 4, 3), "ldq=3 smaller")):
        assert lib.dp_csr_sddmm_plan(*bad, 0, 0, out) == -1 and text in _err(lib)
    assert lib.dp_csr_sddmm_plan(4, 4, 4, 0, 0, None) == -1 and "NULL" in _err(lib)


def _tool():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_sddmm_kernels_use_no_scratch_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if d["name"].startswith("k_csr_sddmm<")}
    assert sorted(ks) == sorted(f"k_csr_sddmm<{l},{v},{e}>" for l in (4, 16, 64) for v in (1, 4) for e in (0, 1, 2))
    for d in ks.values():
        assert d["scratch"] == 0 and d["lds_static"] == 0, d
        assert d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 128, d


def test_the_table_reaches_every_row_shape():
    g = EC.graph("planted")
    deg = np.diff(g.indptr)
    assert tuple(deg[:len(EC.PLANTED)]) == EC.PLANTED
    assert (g.rows == g.indices).any()                                               # self loops
    long = EC.graph("long")
    assert np.diff(long.indptr)[EC.LONG_ROW] == EC.LONG_LEN > EC.CHUNK
    b = EC.graph("batch")
    assert all(int(b.indptr[o]) % 64 for o in b.off[1:-1])       # no graph's entries start on a 64-entry boundary
    assert (np.diff(b.off) == 1).any() and np.diff(b.indptr).max() >= 64
    assert {c[0] for c in EC.SDDMM_CASES} == set(EC.GRAPHS) and {c[5] for c in EC.SDDMM_CASES} == {0.0, 1.0}
    assert any(c[6] is None for c in EC.SDDMM_CASES) and any(c[6] is not None for c in EC.SDDMM_CASES)
    u = EC.graph("undirected")
    assert np.array_equal(EC.dense_of(u, np.ones(u.nnz)), EC.dense_of(u, np.ones(u.nnz)).T)


# ------------------------------------------------------------------ with_values
def _container(name, weighted=True):
    g = EC.graph(name)
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


@pytest.mark.parametrize("name", EC.GRAPHS)
@pytest.mark.parametrize("weighted", [False, True], ids=["01", "weighted"])
def test_with_values_shares_the_index_arrays_and_permutes_values_t(name, weighted):
    c = _container(name, weighted)
    nnz = int(c.indptr[-1])
    v = torch.rand(nnz, requires_grad=True)
    shared = [f for f in vars(c) if isinstance(getattr(c, f), torch.Tensor) and "values" not in f]
    assert {"indptr", "indices", "indptr_t", "indices_t"} <= set(shared)
    h = c.with_values(v)
    assert type(h) is type(c) and h.weighted and c.weighted == weighted
    for f in shared:                                   # every index array and table: the same tensor, not a copy
        assert getattr(h, f) is getattr(c, f), f
    assert h.values is v and (c.values is None or c.values is not v)
    # values_t against the dense transpose
    a = np.zeros((c.n, c.n))
    ip, ix = c.indptr.numpy().astype(np.int64), c.indices.numpy()
    a[np.repeat(np.arange(c.n), np.diff(ip)), ix] = v.detach().numpy()
    if c.indices_t is c.indices:
        assert h.values_t is h.values and "_t_perm" not in vars(c)
    else:
        ipt, ixt = c.indptr_t.numpy().astype(np.int64), c.indices_t.numpy()
        at = np.zeros_like(a)
        at[np.repeat(np.arange(c.n), np.diff(ipt)), ixt] = h.values_t.numpy()
        assert np.array_equal(at, a.T) and not h.values_t.requires_grad
        assert "_t_perm" in vars(c) and vars(h)["_t_perm"] is vars(c)["_t_perm"]      # computed once, cached, shared
        assert c.with_values(torch.rand(nnz))._t_perm is c._t_perm


def test_with_values_refusals_and_the_edgeless_pad():
    c = _container("planted")
    nnz = int(c.indptr[-1])
    with pytest.raises(ValueError, match=r"one value per stored entry \[927\]"):
        c.with_values(torch.ones(nnz + 1))
    with pytest.raises(ValueError, match="one value per stored entry"):
        c.with_values(torch.ones(nnz, 1))
    with pytest.raises(ValueError, match="must be float32"):
        c.with_values(torch.ones(nnz, dtype=torch.float64))
    with pytest.raises(TypeError, match="must be a tensor"):
        c.with_values(np.ones(nnz, dtype=np.float32))
    with pytest.raises(ValueError, match="is on meta but the index arrays are on cpu"):
        c.with_values(torch.ones(nnz, device="meta"))
    b = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    h = b.with_values(torch.zeros(0, requires_grad=True))
    assert h.weighted and h.values.shape == (1,) and not h.values.requires_grad and h.indices is b.indices
    with pytest.raises(ValueError, match="one value per stored entry"):
        b.with_values(torch.zeros(2))
    bad = CsrGraph(c.indptr, c.indices, c.indptr, c.indices.clone())      # a "transposed CSR" that is not the transpose
    with pytest.raises(ValueError, match="not the transpose"):
        bad.with_values(torch.ones(nnz))


# ------------------------------------------------------------------ what the ops and the models call
def _misplaced(calls, g):
    """tests/test_csr_host_cpu.misplaced for calls that include the new entries (which take `values` without a _w)."""
    bad = []
    for name, args in calls:
        for p in FIELDS:
            if p in args and args[p] is not None and args[p] != getattr(g, p).data_ptr():
                bad.append(f"{name}: parameter {p} did not get {type(g).__name__}.{p}")
    return bad


def _leaf(*shape):
    return torch.rand(*shape, requires_grad=True)


def _run_ops(g):
    ops.csr_graph_conv(_leaf(g.n, 3), _leaf(3, 4), _leaf(4), g, _lib.F_NORMALIZE).sum().backward()
    s, z = _leaf(g.n, 2), _leaf(g.n, 4)
    batch = isinstance(g, CsrBatch)
    xp, ap = ops.csr_pool_batch(s, z, g) if batch else ops.csr_pool(s, z, g)
    (xp.sum() + ap.sum()).backward()
    (ops.csr_link_loss_batch(_leaf(g.n, 2), g) if batch else ops.csr_link_loss(_leaf(g.n, 2), g)).backward()
    ops.frob_link_loss(_leaf(g.n, 2), g).backward()


@pytest.mark.parametrize("name", ["planted", "undirected", "batch"])
def test_ops_call_the_new_entries_exactly_when_values_require_grad(monkeypatch, name):
    lib = fake_lib(monkeypatch.setattr)
    c = _container(name)
    mid = "_batch" if isinstance(c, CsrBatch) else ""
    _run_ops(c)
    plain = [n for n, _ in lib.calls]
    assert not set(plain) & set(DV_ENTRIES)
    v = torch.rand(int(c.indptr[-1]), requires_grad=True)
    h = c.with_values(v)
    del lib.calls[:]
    _run_ops(h)
    assert [n for n, _ in lib.calls] == [
        "dp_sparse_gcn_layer_fwd_w", "dp_sparse_gcn_layer_bwd_dv", f"dp_csr_pool{mid}_fwd_w", f"dp_csr_pool{mid}_bwd_w",
        "dp_csr_pool_dvalues", f"dp_csr_linkpred{mid}_loss_fwd_w", f"dp_csr_linkpred{mid}_loss_bwd_w",
        "dp_csr_link_dvalues", f"dp_csr_frob_link{mid}_fwd_w", f"dp_csr_frob_link{mid}_bwd", "dp_csr_link_dvalues"]
    assert _misplaced(lib.calls, h) == [] and v.grad is not None and v.grad.shape == v.shape
    by = {}
    for n, a in lib.calls:
        by.setdefault(n, []).append(a)
    assert [a["objective"] for a in by["dp_csr_link_dvalues"]] == [0, 1]
    sizes = np.diff(h.node_off_host.astype(np.int64))
    assert all(a["inv_norm"] == pytest.approx(1.0 / float((sizes ** 2).sum())) and a["indices"] == h.indices.data_ptr()
               and a["values"] == v.data_ptr() for a in by["dp_csr_link_dvalues"])
    pool = by["dp_csr_pool_dvalues"][0]
    assert pool["B"] == h.num_graphs and (pool["node_off_host"] is None) == (mid == "")
    assert mid == "" or pool["node_off_host"] == h.node_off_host.ctypes.data
    # grad mode off, or values that do not require grad: today's calls
    for other in (c.with_values(v.detach()),):
        del lib.calls[:]
        _run_ops(other)
        assert [n for n, _ in lib.calls] == plain
    del lib.calls[:]
    with torch.no_grad():
        ops.csr_graph_conv(torch.rand(h.n, 3), torch.rand(3, 4), None, h, 0)
        ops.csr_link_loss_batch(torch.rand(h.n, 2), h) if mid else ops.csr_link_loss(torch.rand(h.n, 2), h)
    assert [n for n, _ in lib.calls] == ["dp_sparse_gcn_layer_fwd_w", f"dp_csr_linkpred{mid}_loss_fwd_w"]


def _model_calls(setattr_, case, transform):
    make_model, make_graph, loss_takes_graph = MODEL_CASES[case]
    lib = fake_lib(setattr_)
    torch.manual_seed(0)
    model, g = make_model(), make_graph()
    g, v = transform(g)
    nb = g.num_graphs if isinstance(g, CsrBatch) else 1
    pred = model(torch.rand(g.n, 3), g)
    label = torch.arange(nb) % 2
    loss = model.loss(pred, label, g) if loss_takes_graph else model.loss(pred, label)
    loss.backward()
    return lib.scalars(), v, model


@pytest.mark.parametrize("case", sorted(MODEL_CASES))
def test_models_fill_values_grad_and_launch_today_s_sequence_otherwise(monkeypatch, case):
    with open(GOLDEN) as f:
        golden = json.load(f)[case]
    # values without requires_grad: the golden record, call for call
    got, _, _ = _model_calls(monkeypatch.setattr, case, lambda g: (g.with_values(g.values.clone()), None))
    assert got == golden

    def grad(g):
        v = g.values.clone().requires_grad_(True)
        return g.with_values(v), v
    got, v, model = _model_calls(monkeypatch.setattr, case, grad)
    assert v.grad is not None and v.grad.shape == v.shape
    assert all(p.grad is not None for p in model.parameters())
    names = [n for n, _ in got]
    assert "dp_sparse_gcn_layer_bwd_dv" in names and "dp_sparse_gcn_layer_bwd_w" not in names
    if case.startswith("diffpool"):
        assert names.count("dp_csr_pool_dvalues") == 1 and names.count("dp_csr_link_dvalues") == 1
        link = [a for n, a in got if n == "dp_csr_link_dvalues"][0]
        assert link["objective"] == int("frobenius" in case)
    # the new launches taken out (and bwd_dv read as bwd_w): the golden record
    back = []
    for n, a in got:
        if n in ("dp_csr_pool_dvalues", "dp_csr_link_dvalues"):
            continue
        if n == "dp_sparse_gcn_layer_bwd_dv":
            n, a = "dp_sparse_gcn_layer_bwd_w", {k: x for k, x in a.items() if k != "ldx"}
        back.append([n, a])
    assert back == golden


# ------------------------------------------------------------------ the bounds tell a bug from rounding
def _shift(g):
    """A neighbouring row's P: row i + 1 for every stored entry (the last row takes row 0)."""
    return (g.rows + 1) % g.n


def _head64(g, ref):
    """A kernel that skips the tail of a row longer than 64: those entries keep 0."""
    pos = np.arange(g.nnz) - g.indptr[g.rows]
    return np.where(pos < 64, ref, 0.0)


def _check_faults(g, ref, bound, faults):
    for what, other in faults.items():
        if what == "tail of a long row skipped" and np.diff(g.indptr).max() <= 64:
            continue                                   # the batch's longest row holds exactly 64 entries
        assert EC.moved(ref, other, bound) > 4.0, (what, EC.moved(ref, other, bound))


@pytest.mark.parametrize("case", EC.SDDMM_CASES, ids=EC.sddmm_id)
def test_identity_bound_discriminates(case):
    gname, F, _, _, _, beta, d = case
    g = EC.graph(gname)
    P, Q, out0 = EC.sddmm_inputs(case)
    ref, bound = EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, d, beta)
    cols = g.indices.astype(np.int64)
    faults = {"neighbouring row's P": EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, d, beta, rows=_shift(g))[0],
              "tail of a long row skipped": _head64(g, ref)}
    if g.directed:
        faults["(j, i) for (i, j)"] = EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, d, beta, rows=cols, cols=g.rows)[0]
    if F > 1:
        faults["last column dropped"] = EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, d, beta, F=F - 1)[0]
    if d is not None:
        faults["dscale ignored"] = EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, None, beta)[0]
    if beta:
        faults["beta ignored"] = EC.sddmm_ref(g, P, Q, out0, EC.ALPHA, d, 0.0)[0]
    _check_faults(g, ref, bound, faults)


@pytest.mark.parametrize("case", EC.LINK_CASES, ids=EC.link_id)
def test_link_bounds_discriminate(case):
    gname, K, obj, over = case
    g = EC.graph(gname)
    S = EC.link_inputs(case)
    ref, bound = EC.link_ref(g, S, obj, EC.DLOSS, g.values)
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound > 0).all()
    faults = {"dloss ignored": EC.link_ref(g, S, obj, 1.0, g.values)[0],
              "neighbouring row's s_i": EC.link_ref(g, S, obj, EC.DLOSS, g.values, rows=_shift(g))[0],
              "tail of a long row skipped": _head64(g, ref)}
    if K > 1:
        faults["last column dropped"] = EC.link_ref(g, S[:, :K - 1], obj, EC.DLOSS, g.values)[0]
    if obj == 1:
        faults["factor 2 missing"] = EC.link_ref(g, S, obj, EC.DLOSS, g.values, factor=1.0)[0]
        faults["values read as ones"] = EC.link_ref(g, S, obj, EC.DLOSS, None)[0]
    if over:
        faults["clamp omitted"] = EC.link_ref(g, S, obj, EC.DLOSS, g.values, clamp=False)[0]
    _check_faults(g, ref, bound, faults)


def test_the_over_one_cases_do_reach_the_clamp():
    hit = 0
    for case in EC.LINK_CASES:
        if case[3]:
            g, S = EC.graph(case[0]), EC.link_inputs(case).astype(np.float64)
            hit += int((np.einsum("ef,ef->e", S[g.rows], S[g.indices]) > 1.0).sum())
    assert hit >= 2


@pytest.mark.parametrize("case", EC.POOL_CASES, ids=EC.pool_id)
def test_pool_bound_discriminates(case):
    g = EC.graph(case[0])
    S, dAp = EC.pool_inputs(case)
    ref, bound = EC.pool_ref(g, S, dAp)
    cols = g.indices.astype(np.int64)
    faults = {"neighbouring row's P": EC.pool_ref(g, S, dAp, rows=_shift(g))[0],
              "(j, i) for (i, j)": EC.pool_ref(g, S, dAp, rows=cols, cols=g.rows)[0],
              "dA' transposed": EC.pool_ref(g, S, np.transpose(dAp, (0, 2, 1)))[0]}
    if g.off is not None:
        gr = g.graph_of_row()
        faults["the wrong graph's dA'"] = EC.pool_ref(g, S, dAp, graph_of_row=(gr + 1) % dAp.shape[0])[0]
    for what, other in faults.items():
        if case[1] == 1 and what != "the wrong graph's dA'":
            continue                                   # K = 1: S is the constant 1, every row and column is alike
        assert EC.moved(ref, other, bound) > 4.0, (what, EC.moved(ref, other, bound))


@pytest.mark.parametrize("case", EC.GCN_CASES, ids=EC.gcn_id)
def test_gcn_bound_discriminates(case):
    g = EC.graph(case[0])
    x, W, b, dy = EC.gcn_inputs(case)
    ref, bound = EC.gcn_ref(g, x, W, b, dy, case[3])
    cols = g.indices.astype(np.int64)
    faults = {"neighbouring row's dax": EC.gcn_ref(g, x, W, b, dy, case[3], rows=_shift(g))[0],
              "(j, i) for (i, j)": EC.gcn_ref(g, x, W, b, dy, case[3], rows=cols, cols=g.rows)[0],
              "tail of a long row skipped": _head64(g, ref)}
    _check_faults(g, ref, bound, faults)
