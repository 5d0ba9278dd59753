"""Edge weights on the CSR path, the part that needs no GPU: the `_w` entries are exported with the header's
signatures and report every argument error before a launch; the containers' weight semantics on device="cpu";
`normalized()` against tu_dataset.normalized_adjacency; and the inputs of tests/test_gpu_csr_weights.py tell a bug from
rounding: a float64 reference computed with the weights ignored, with one weight dropped, or with `values` read in the
order of the transposed CSR differs from the weighted one by more than the bound the GPU test applies."""
import ctypes as C

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, tu_dataset
from graph_pooling_amd.sparse import CsrBatch, CsrGraph
from tests import csr_weights_cases as WC
from tests import frob_link_cases as FC
from tests.test_abi_cpu import _header_functions, _kind

INVALID, UNSUPPORTED = -1, -3
W_ENTRIES = ("dp_csr_aggregate_w", "dp_sparse_gcn_layer_fwd_w", "dp_sparse_gcn_layer_bwd_w", "dp_csr_pool_fwd_w",
             "dp_csr_pool_bwd_w", "dp_csr_pool_batch_fwd_w", "dp_csr_pool_batch_bwd_w", "dp_csr_linkpred_loss_fwd_w",
             "dp_csr_linkpred_loss_bwd_w", "dp_csr_linkpred_batch_loss_fwd_w", "dp_csr_linkpred_batch_loss_bwd_w",
             "dp_csr_frob_link_fwd_w", "dp_csr_frob_link_batch_fwd_w")


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------ ABI
def test_w_entries_are_exported_with_the_headers_signatures(lib):
    fns = _header_functions()
    cmap = {C.c_int: "int", C.c_long: "long", C.c_float: "float", C.c_size_t: "size_t", C.c_void_p: "ptr"}
    for name in W_ENTRIES:
        assert name in fns and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        ret, args = fns[name]
        res, argtypes = _lib._PROTOS[name]
        assert ret == "int" and res is C.c_int
        assert [_kind(a) for a in args] == [cmap[t] for t in argtypes], name
        # `values` follows each index array, `values_t` a transposed one
        names = [a.split()[-1].lstrip("*") for a in args]
        i = names.index("indices" if "indices" in names else "indices_local")
        assert names[i + 1] == "values", (name, names)
        if "indices_t" in names or "indices_t_local" in names:
            j = names.index("indices_t" if "indices_t" in names else "indices_t_local")
            assert names[j + 1] == "values_t", (name, names)
        # the unweighted entry keeps its signature: the _w list is that list plus the values
        plain = [a.split()[-1].lstrip("*") for a in fns[name[:-2]][1]]
        assert [a for a in names if a not in ("values", "values_t")] == [a for a in plain if a != "mean"], name


def _err(lib):
    return lib.dp_last_error_string().decode()


def test_w_entries_report_argument_errors_without_a_gpu(lib):
    buf = (C.c_float * 4096)()
    idx = (C.c_int * 64)()
    idx2 = (C.c_int * 64)()
    off = (C.c_int * 2)(0, 4)
    p, i, i2, o = C.addressof(buf), C.addressof(idx), C.addressof(idx2), C.addressof(off)
    big = 1 << 26

    assert lib.dp_csr_aggregate_w(p, 4, i, i, None, p, 4, 4, 4, 0.0, None) == INVALID and "values is NULL" in _err(lib)
    assert lib.dp_csr_aggregate_w(None, 4, i, i, p, p, 4, 4, 4, 0.0, None) == INVALID and "NULL" in _err(lib)
    assert lib.dp_csr_aggregate_w(p, 4, i, i, p, p, 4, 0, 4, 0.0, None) == INVALID and "positive" in _err(lib)

    gcn_f = lambda values, x=p, flags=0, ldx=4: lib.dp_sparse_gcn_layer_fwd_w(x, ldx, i, i, values, p, p, p, 4, p, p, 4, 4,
                                                                             4, flags, p, big, None)
    assert gcn_f(None) == INVALID and "values is NULL" in _err(lib)
    assert gcn_f(p, x=None) == INVALID and "NULL" in _err(lib)
    assert gcn_f(p, flags=1, ldx=5) == INVALID and "contiguous" in _err(lib)
    gcn_b = lambda values, ipt, ixt, values_t, lddx=4: lib.dp_sparse_gcn_layer_bwd_w(
        p, i, i, values, ipt, ixt, values_t, p, p, 4, p, p, 4, p, lddx, p, p, 4, 4, 4, 0, p, big, None)
    assert gcn_b(None, i, i, None) == INVALID and "values is NULL" in _err(lib)
    assert gcn_b(p, i2, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert gcn_b(p, i2, None, p) == INVALID and "come together" in _err(lib)
    assert gcn_b(p, i2, i2, p, lddx=5) == INVALID and "contiguous" in _err(lib)

    pool_f = lambda values, K=4, S=p, lds=4: lib.dp_csr_pool_fwd_w(S, lds, p, 4, i, i, values, p, p, 4, K, 4, p, big, None)
    assert pool_f(None) == INVALID and "values is NULL" in _err(lib)
    assert pool_f(p, S=None) == INVALID and "NULL" in _err(lib)
    assert pool_f(p, K=257, lds=257) == UNSUPPORTED and "supported" in _err(lib)
    assert pool_f(p, lds=3) == INVALID
    pool_b = lambda values, ixt, values_t, ldds=4: lib.dp_csr_pool_bwd_w(p, 4, p, 4, i, i, values, i, ixt, values_t, p, p, p,
                                                                        ldds, p, 4, 4, 4, 4, p, big, None)
    assert pool_b(None, i, None) == INVALID and "values is NULL" in _err(lib)
    assert pool_b(p, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert pool_b(p, i2, p, ldds=3) == INVALID and "ldds" in _err(lib)
    bat_f = lambda values, B=1: lib.dp_csr_pool_batch_fwd_w(p, 4, p, 4, i, i, values, i, i, 1, p, p, B, 4, 4, 4, p, big, None)
    assert bat_f(None) == INVALID and "values is NULL" in _err(lib)
    assert bat_f(p, B=0) == INVALID and "n_slabs" in _err(lib)
    bat_b = lambda values, ixt, values_t, B=1: lib.dp_csr_pool_batch_bwd_w(p, 4, p, 4, i, i, values, i, ixt, values_t, i, 1,
                                                                          p, p, p, 4, p, 4, B, 4, 4, 4, p, big, None)
    assert bat_b(None, i, None) == INVALID and "values is NULL" in _err(lib)
    assert bat_b(p, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert bat_b(p, i, None, B=0) == INVALID and "n_blocks" in _err(lib)

    lk_f = lambda values, K=4, ws=p, wsb=big: lib.dp_csr_linkpred_loss_fwd_w(p, K, i, i, values, p, 4, K, ws, wsb, None)
    assert lk_f(None) == INVALID and "values is NULL" in _err(lib)
    assert lk_f(p, K=257) == UNSUPPORTED
    assert lk_f(p, ws=None) == INVALID and "workspace" in _err(lib)
    assert lk_f(p, wsb=8) == INVALID and "too small" in _err(lib)
    lk_b = lambda values, ixt, values_t, ldds=4: lib.dp_csr_linkpred_loss_bwd_w(p, 4, i, i, values, i, ixt, values_t, None,
                                                                               p, ldds, 0, 4, 4, p, big, None)
    assert lk_b(None, i, None) == INVALID and "values is NULL" in _err(lib)
    assert lk_b(p, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert lk_b(p, i, None, ldds=3) == INVALID and "ldds" in _err(lib)
    lkb_f = lambda values, node_off=o: lib.dp_csr_linkpred_batch_loss_fwd_w(p, 4, i, i, values, node_off, 1, p, 4, p, big,
                                                                           None)
    assert lkb_f(None) == INVALID and "values is NULL" in _err(lib)
    assert lkb_f(p, node_off=None) == INVALID and "node_off_host" in _err(lib)
    lkb_b = lambda values, ixt, values_t: lib.dp_csr_linkpred_batch_loss_bwd_w(p, 4, i, i, values, i, ixt, values_t, o, 1,
                                                                              None, p, 4, 0, 4, p, big, None)
    assert lkb_b(None, i, None) == INVALID and "values is NULL" in _err(lib)
    assert lkb_b(p, i2, None) == INVALID and "values_t is NULL" in _err(lib)

    fr = lambda values, ipt, ixt, values_t, K=4, wsb=big: lib.dp_csr_frob_link_fwd_w(p, K, i, i, values, ipt, ixt, values_t,
                                                                                    None, p, p, p, None, 4, K, p, wsb, None)
    assert fr(None, None, None, None) == INVALID and "values is NULL" in _err(lib)
    assert fr(p, i2, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert fr(p, i2, None, None) == INVALID and "go together" in _err(lib)
    assert fr(p, None, None, None, K=257) == UNSUPPORTED
    assert fr(p, None, None, None, wsb=8) == INVALID and "too small" in _err(lib)
    frb = lambda values, ipt, ixt, values_t, B=1: lib.dp_csr_frob_link_batch_fwd_w(
        p, 4, i, i, values, ipt, ixt, values_t, i, None, p, p, p, None, B, 4, 4, p, big, None)
    assert frb(None, None, None, None) == INVALID and "values is NULL" in _err(lib)
    assert frb(p, i2, i2, None) == INVALID and "values_t is NULL" in _err(lib)
    assert frb(p, None, None, None, B=5) == INVALID and "every graph" in _err(lib)
    # the workspace queries serve both forms: there is no _w query
    assert not any(n.endswith("workspace_bytes_w") for n in _lib.EXPORTED_SYMBOLS)


# ------------------------------------------------------------------ containers
def _dense_of(g):
    return WC.dense(g)


def test_from_edges_mirrors_weights_and_handles_duplicates():
    g = CsrGraph.from_edges(4, [0, 1, 2, 1], [1, 2, 3, 0], "cpu", weight=[0.5, 2.0, 0.0, 0.5])   # (0,1) given both ways
    assert g.weighted and g.values_t is g.values and g.indices_t is g.indices
    a = _dense_of(g)
    assert np.array_equal(a, a.T) and a[0, 1] == 0.5 and a[1, 2] == 2.0
    assert g.indices.numel() == 6 and g.values.dtype == torch.float32           # the stored zero (2, 3) is kept
    assert g.values.tolist() == [0.5, 0.5, 2.0, 2.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="two weights"):
        CsrGraph.from_edges(3, [0, 1], [1, 0], "cpu", weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="two weights"):
        CsrGraph.from_edges(3, [0, 0], [1, 1], "cpu", symmetric=False, weight=[1.0, 2.0])
    same = CsrGraph.from_edges(3, [0, 0], [1, 1], "cpu", symmetric=False, weight=[1.5, 1.5])
    assert same.indices.tolist() == [1] and same.values.tolist() == [1.5] and same.values_t.tolist() == [1.5]
    with pytest.raises(ValueError, match="weights for"):
        CsrGraph.from_edges(3, [0, 1], [1, 2], "cpu", weight=[1.0])
    plain = CsrGraph.from_edges(3, [0, 0], [1, 1], "cpu")
    assert not plain.weighted and plain.values is None and plain.values_t is None


def test_directed_graph_carries_values_t_in_the_transposed_order():
    gh = WC.graph(40, 3, 1, directed=True)
    a = WC.dense(gh)
    assert (a != a.T).any() and gh.values_t is not gh.values
    assert np.array_equal(WC.dense(gh, transposed=True), a)
    assert not np.array_equal(WC.faulty(gh)["values in transposed order"], a)


def test_from_dense_weighted_round_trips():
    rng = np.random.default_rng(0)
    a = (rng.random((30, 30)) < 0.2) * rng.uniform(0.1, 3.0, (30, 30))
    t = torch.tensor(a, dtype=torch.float32)
    g = CsrGraph.from_dense(t, weighted=True)
    assert g.weighted and np.array_equal(WC.dense(g), t.double().numpy())
    assert np.array_equal(WC.dense(g, transposed=True), t.double().numpy())
    g01 = CsrGraph.from_dense(t)
    assert not g01.weighted and g01.indices.tolist() == g.indices.tolist()
    sizes = [30, 12]
    adj = torch.zeros(2, 30, 30)
    adj[0] = t
    adj[1, :12, :12] = t[:12, :12]
    adj[1, 12:, 12:] = 7.0                                   # outside the graph: never read
    b = CsrBatch.from_dense(adj, sizes, weighted=True)
    want = np.zeros((42, 42))
    want[:30, :30], want[30:, 30:] = t.double().numpy(), t[:12, :12].double().numpy()
    assert b.weighted and np.array_equal(WC.dense(b), want) and np.array_equal(WC.dense(b, transposed=True), want)
    assert not CsrBatch.from_dense(adj, sizes).weighted


def test_a_batch_of_mixed_graphs_gets_ones():
    gw = CsrGraph.from_edges(3, [0, 1], [1, 2], "cpu", weight=[0.5, 2.0])
    g1 = CsrGraph.from_edges(2, [0], [1], "cpu")
    b = CsrBatch.from_graphs([g1, gw])
    assert b.weighted and b.values.tolist() == [1.0, 1.0, 0.5, 0.5, 2.0, 2.0] and b.values_t is b.values
    assert b.values.numel() == b.indices.numel() == b.indices_local.numel()
    assert not CsrBatch.from_graphs([g1, g1]).weighted and CsrBatch.from_graphs([g1, g1]).values is None
    b2 = CsrBatch.from_edge_lists([2, 3], [[0], [0, 1]], [[1], [1, 2]], "cpu", weights=[None, [0.5, 2.0]])
    assert b2.values.tolist() == b.values.tolist()
    d = CsrBatch.from_edge_lists([2, 3], [[0], [0, 1]], [[1], [1, 2]], "cpu", symmetric=False, weights=[None, [0.5, 2.0]])
    assert d.values.tolist() == [1.0, 0.5, 2.0] and d.values_t.tolist() == [1.0, 0.5, 2.0] and d.values_t is not d.values
    assert d.indices_t.tolist() == [0, 2, 3]
    e = CsrBatch([2, 1], [(np.array([0, 1, 1]), np.array([1]), None, None, np.array([0.25])),
                          (np.array([0, 0]), np.zeros(0, np.int64), None, None)], "cpu")
    assert e.weighted and e.values.tolist() == [0.25]
    with pytest.raises(ValueError, match="values for"):
        CsrBatch([2], [(np.array([0, 1, 1]), np.array([1]), None, None, np.array([0.25, 1.0]))], "cpu")
    with pytest.raises(ValueError, match="floating point"):
        CsrBatch([2], [(np.array([0, 1, 1]), np.array([1]), None, None, np.array([1]))], "cpu")


def test_values_are_checked_for_length_dtype_and_device():
    ip, ix = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    ok = CsrGraph(ip, ix, values=torch.tensor([0.5, 0.5]))
    assert ok.weighted and ok.values_t is ok.values
    with pytest.raises(ValueError, match="one value per stored entry"):
        CsrGraph(ip, ix, values=torch.tensor([0.5]))
    with pytest.raises(ValueError, match="float32"):
        CsrGraph(ip, ix, values=torch.tensor([0.5, 0.5], dtype=torch.float64))
    with pytest.raises(TypeError, match="tensor"):
        CsrGraph(ip, ix, values=[0.5, 0.5])
    with pytest.raises(ValueError, match="is on"):
        CsrGraph(ip, ix, values=torch.tensor([0.5, 0.5], device="meta"))
    with pytest.raises(ValueError, match="needs values_t"):
        CsrGraph(ip, ix, ip.clone(), ix.clone(), values=torch.tensor([0.5, 0.5]))
    with pytest.raises(ValueError, match="values_t without values"):
        CsrGraph(ip, ix, values_t=torch.tensor([0.5, 0.5]))
    with pytest.raises(ValueError, match="a_ij = a_ji"):
        CsrGraph(ip, ix, values=torch.tensor([0.5, 0.5]), values_t=torch.tensor([0.5, 0.5]))


# ------------------------------------------------------------------ normalized()
def _ring(n, chords, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return np.concatenate([i, rng.integers(0, n, chords)]), np.concatenate([(i + 1) % n, rng.integers(0, n, chords)])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("symmetric", [True, False])
def test_normalized_equals_the_dense_normalisation_to_one_rounding(symmetric, weighted):
    n = 57
    src, dst = _ring(n, 40, 3)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    if symmetric:
        src, dst = np.minimum(src, dst), np.maximum(src, dst)
    _, first = np.unique(src * n + dst, return_index=True)
    src, dst = src[first], dst[first]
    w = np.random.default_rng(1).uniform(0.2, 3.0, src.size).astype(np.float32) if weighted else None
    g = CsrGraph.from_edges(n, src, dst, "cpu", symmetric=symmetric, weight=w)
    a = WC.dense(g, None if weighted else np.ones(g.indices.numel()))
    gn = g.normalized()
    assert gn.weighted and not g.weighted == (not weighted) and gn.indices is g.indices
    want = tu_dataset.normalized_adjacency(a)                 # float64 in, float64 out
    got = WC.dense(gn)
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want)).all() and (got != 0).sum() == (a != 0).sum()
    assert np.array_equal(WC.dense(gn, transposed=True), got)
    assert (gn.values_t is gn.values) == symmetric
    # the batch normalises every graph the same way
    b = CsrBatch.from_graphs([g, g]).normalized()
    assert b.weighted and np.array_equal(WC.dense(b)[:n, :n], got) and np.array_equal(WC.dense(b)[n:, n:], got)
    assert np.array_equal(WC.dense(b, transposed=True), WC.dense(b))


def test_normalized_raises_on_an_isolated_node():
    g = CsrGraph.from_edges(4, [0, 1], [1, 2], "cpu")         # node 3 has no edge
    with pytest.raises(ValueError, match="node 3 has degree 0"):
        g.normalized()
    with pytest.raises(ValueError, match="degree 0"):
        CsrBatch.from_graphs([CsrGraph.from_edges(2, [0], [1], "cpu"), g]).normalized()
    d = CsrGraph.from_edges(3, [0, 1, 2], [1, 2, 1], "cpu", symmetric=False)    # column 0 sums to 0 (axis=0)
    with pytest.raises(ValueError, match="node 0 has degree 0"):
        d.normalized()
    z = CsrGraph.from_edges(2, [0], [1], "cpu", weight=[0.0])                   # stored zeros only
    with pytest.raises(ValueError, match="degree 0"):
        z.normalized()


# ------------------------------------------------------------------ the GPU tests' inputs tell a bug from rounding
def _worst(ref_fault, ref, bound):
    return float((np.abs(np.asarray(ref_fault) - np.asarray(ref)) / np.maximum(bound, 1e-300)).max())


def _faults(gh, need_transposed):
    f = WC.faulty(gh)
    assert ("values in transposed order" in f) == need_transposed
    return f


def test_aggregation_inputs_discriminate():
    gh = WC.agg_graph()
    a, deg = WC.dense(gh), WC.degrees(gh)
    for feat in WC.AGG_FEATS:
        rng = np.random.default_rng(feat)
        x = rng.standard_normal((gh.n, feat)).astype(np.float32)
        old = rng.standard_normal((gh.n, feat)).astype(np.float32)
        for beta in (0.0, 1.0):
            ref, bound = WC.agg_ref(a, x, old, beta, deg)
            for what, af in _faults(gh, True).items():
                assert _worst(WC.agg_ref(af, x, old, beta, deg)[0], ref, bound) > 1.0, (feat, beta, what)


@pytest.mark.parametrize("directed", [False, True])
def test_gcn_layer_inputs_discriminate(directed):
    n, fin, fout = 203, 21, 34
    gh = WC.graph(n, 5, 11, directed=directed)
    a, deg, deg_t = WC.dense(gh), WC.degrees(gh), np.diff(gh.indptr_t.numpy().astype(np.int64))
    for flags in range(4):
        rng = np.random.default_rng(flags + 10)
        x = rng.standard_normal((n, fin)).astype(np.float32)
        W = (rng.standard_normal((fin, fout)) / np.sqrt(fin)).astype(np.float32)
        b = rng.uniform(-0.3, 0.3, fout).astype(np.float32)
        dy = rng.standard_normal((n, fout)).astype(np.float32)
        ref = WC.gcn_ref(a, x, W, b, dy, bool(flags & 1), bool(flags & 2), deg, deg_t, False)
        for what, af in _faults(gh, directed).items():
            bad = WC.gcn_ref(af, x, W, b, dy, bool(flags & 1), bool(flags & 2), deg, deg_t, False)
            for name in ("ax", "y", "dx", "dW"):
                assert _worst(bad[name][0], ref[name][0], ref[name][1]) > 1.0, (flags, what, name)


@pytest.mark.parametrize("n,K,D,directed", [(7, 7, 60, True), (300, 50, 60, False), (300, 50, 60, True),
                                            (1000, 64, 96, False), (1000, 128, 60, True)])
def test_pooling_inputs_discriminate(n, K, D, directed):
    for gh, sizes in ((WC.graph(n, 5, n * 7 + K, directed), [n]),
                      (WC.batch(WC.BATCH_SIZES, 5, n + K, directed), WC.BATCH_SIZES)):
        gen = np.random.default_rng(gh.n + K + D)
        S = gen.random((gh.n, K)).astype(np.float32)
        Z = (gen.random((gh.n, D)) - 0.5).astype(np.float32)
        dXp = gen.standard_normal((len(sizes) * K, D)).astype(np.float32)
        dAp = gen.standard_normal((len(sizes) * K, K)).astype(np.float32)
        a, deg, deg_t = WC.dense(gh), WC.degrees(gh), np.diff(gh.indptr_t.cpu().numpy().astype(np.int64))
        old = np.full((gh.n, D), 0.25)
        for what, af in _faults(gh, directed).items():
            hit = {"Ap": 0.0, "dS": 0.0}
            off = np.concatenate([[0], np.cumsum(sizes)])
            for b in range(len(sizes)):
                r = slice(off[b], off[b + 1])
                args = (S[r], Z[r], dXp[b * K:(b + 1) * K], dAp[b * K:(b + 1) * K], old[r], deg[r], deg_t[r])
                ref, bound = WC.pool_ref(a[r, r], *args)
                bad, _ = WC.pool_ref(af[r, r], *args)
                for name in hit:
                    hit[name] = max(hit[name], _worst(bad[name], ref[name], bound[name]))
            assert hit["Ap"] > 1.0 and hit["dS"] > 1.0, (what, hit)


def _graph_list(gh, sizes, S, a):
    deg, deg_t = WC.degrees(gh), np.diff(gh.indptr_t.cpu().numpy().astype(np.int64))
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(a[off[b]:off[b + 1], off[b]:off[b + 1]], S[off[b]:off[b + 1]], deg[off[b]:off[b + 1]],
             deg_t[off[b]:off[b + 1]]) for b in range(len(sizes))]


def _form(form, seed):
    directed, is_batch = form.startswith("directed"), form.endswith("batch")
    gh = WC.batch(WC.BATCH_SIZES, 4, seed, directed) if is_batch else WC.graph(300, 4, seed, directed)
    return gh, ([gh.n] if not is_batch else WC.BATCH_SIZES), directed


@pytest.mark.parametrize("form", ["graph", "directed", "batch", "directed batch"])
def test_link_loss_inputs_discriminate(form):
    for K in WC.LINK_K:
        gh, sizes, directed = _form(form, 40 + K)
        S = WC.assign_rows(np.random.default_rng(K), gh.n, K)
        ref = WC.link_ref(_graph_list(gh, sizes, S, WC.dense(gh)), 1.7)
        for what, af in _faults(gh, directed).items():
            bad = WC.link_ref(_graph_list(gh, sizes, S, af), 1.7)
            assert abs(bad["loss"] - ref["loss"]) > ref["loss_bound"], (K, what)
            assert _worst(bad["dS"], ref["dS"], ref["dS_bound"]) > 1.0, (K, what)
    for K in FC.K_CASES:
        gh, sizes, directed = _form(form, 90 + K)
        S = WC.assign_rows(np.random.default_rng(K + 1), gh.n, K)
        ref = WC.frob_ref([(a, s) for a, s, _, _ in _graph_list(gh, sizes, S, WC.dense(gh))])
        for what, af in _faults(gh, directed).items():
            bad = WC.frob_ref([(a, s) for a, s, _, _ in _graph_list(gh, sizes, S, af)])
            assert abs(bad["loss"] - ref["loss"]) > ref["loss_bound"], (K, what)
            assert _worst(bad["dS_all"], ref["dS_all"], ref["dS_bound"]) > 1.0, (K, what)
