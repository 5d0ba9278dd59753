"""The weighted CSR entries (dp_csr_aggregate_w, dp_sparse_gcn_layer_*_w, dp_csr_pool_*_w, dp_csr_linkpred_*_w,
dp_csr_frob_link_*_fwd_w) through the C ABI against float64 references computed from the dense weighted matrix, under
the derived bounds of tests/csr_weights_cases.py; weights of 1.0 against the unweighted entries bit for bit; exact
results on a small-integer grid; guard bands around every output; repeat runs bit for bit.

With DP_CSR_WEIGHTS_ANCHOR=<file> the largest |error| / bound per op and case is written there
(profiles/csr_weights_fp64_anchor.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.sparse import CsrGraph
from tests import csr_weights_cases as WC
from tests import frob_link_cases as FC
from tests.test_gpu_sparse_pool import OP_CASES

pytestmark = pytest.mark.gpu

GUARD = -7.25
FRONT, TAIL = 4, 8
RATIOS = {}


def _note(case, ratio):
    RATIOS[case] = max(RATIOS.get(case, 0.0), float(ratio))


def anchor_text(ratios):
    """The worst ratio per op (the case name's first word), then every case."""
    ops = {}
    for k, v in ratios.items():
        ops[k.split()[0]] = max(ops.get(k.split()[0], 0.0), v)
    lines = ["largest |error| / bound (bounds: tests/csr_weights_cases.py, u = 2^-24)", "", "per op"]
    lines += [f"{k:<72s} {ops[k]:8.4f}" for k in sorted(ops)]
    lines += ["", "per case"]
    lines += [f"{k:<72s} {ratios[k]:8.4f}" for k in sorted(ratios)]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_WEIGHTS_ANCHOR")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write(anchor_text(RATIOS))


class Buf:
    """[rows, cols] at leading dimension ld inside a guarded flat device allocation."""

    def __init__(self, rows, cols, ld=None, data=None, fill=GUARD):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        host = torch.full((FRONT + rows * self.ld + TAIL,), GUARD, dtype=torch.float32)
        v = self.view(host)
        v.fill_(fill)
        if data is not None:
            v.copy_(torch.as_tensor(np.asarray(data, dtype=np.float32)).reshape(rows, cols))
        self.host0 = host.clone()
        self.dev = host.cuda()

    def view(self, t):
        return t.as_strided((self.rows, self.cols), (self.ld, 1), FRONT)

    def ptr(self):
        return self.dev.data_ptr() + 4 * FRONT

    def back(self):
        """(values as float64 numpy, True when nothing outside the [rows, cols] window changed)."""
        h = self.dev.cpu()
        a, b = h.clone(), self.host0.clone()
        self.view(a).zero_()
        self.view(b).zero_()
        return self.view(h).clone().numpy(), torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(case, got, ref, bound, untouched=True):
    assert untouched, f"{case}: wrote outside its output"
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), case
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{case}: worst |error| / bound = {ratio:.4f}")
    _note(case, ratio)
    assert (err <= bound).all(), f"{case}: worst |error| / bound = {ratio:.3f}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


def _ones(g):
    """The same container with every weight 1.0."""
    import copy
    o = copy.copy(g)
    o.values = torch.ones_like(g.values)
    o.values_t = o.values if g.values_t is g.values else torch.ones_like(g.values_t)
    return o


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda").random_(0, 255)


def _odd_ld(width, extra):
    ld = width + extra
    return ld if ld % 2 else ld + 1


# ------------------------------------------------------------------ aggregation
def _agg(g, x, ldt, ldo, beta, old, weighted=True):
    lib = _lib.load()
    n, feat = x.shape
    tab = Buf(n, feat, ldt, data=x)
    out = Buf(n, feat, ldo, data=old)
    st = _lib.current_stream()
    if weighted:
        _lib.check(lib.dp_csr_aggregate_w(tab.ptr(), ldt, g.indptr.data_ptr(), g.indices.data_ptr(), g.values.data_ptr(),
                                          out.ptr(), ldo, n, feat, beta, st), "dp_csr_aggregate_w")
    else:
        _lib.check(lib.dp_csr_aggregate(tab.ptr(), ldt, g.indptr.data_ptr(), g.indices.data_ptr(), out.ptr(), ldo, n,
                                        feat, 0, beta, st), "dp_csr_aggregate")
    return out.back()


@pytest.fixture(scope="module")
def agg_case():
    g = WC.agg_graph()
    assert WC.degrees(g)[:len(WC.AGG_DEGREES)].tolist() == list(WC.AGG_DEGREES)
    return WC.to_device(g, "cuda"), WC.dense(g), WC.degrees(g)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("feat", WC.AGG_FEATS)
def test_aggregate_w_at_every_chunk_and_unroll_edge(agg_case, feat, beta):
    g, a, deg = agg_case
    rng = np.random.default_rng(feat)
    x = rng.standard_normal((g.n, feat)).astype(np.float32)
    old = rng.standard_normal((g.n, feat)).astype(np.float32)
    ldt, ldo = _odd_ld(feat, 2), _odd_ld(feat, 4)
    got, clean = _agg(g, x, ldt, ldo, beta, old)
    ref, bound = WC.agg_ref(a, x, old, beta, deg)
    _check(f"aggregate feat={feat} beta={beta:g}", got, ref, bound, clean)
    again, _ = _agg(g, x, ldt, ldo, beta, old)
    assert _bits(again) == _bits(got)
    one, _ = _agg(_ones(g), x, ldt, ldo, beta, old)
    plain, _ = _agg(g, x, ldt, ldo, beta, old, weighted=False)
    assert _bits(one) == _bits(plain)


def test_aggregate_w_is_exact_on_an_integer_grid():
    gh = WC.agg_graph(grid=True)
    g, a = WC.to_device(gh, "cuda"), WC.dense(gh)
    x = np.random.default_rng(3).integers(-8, 9, (g.n, 65)).astype(np.float32)
    got, clean = _agg(g, x, 67, 65, 0.0, np.zeros_like(x))
    assert clean and np.array_equal(got.astype(np.float64), a @ x.astype(np.float64))


# ------------------------------------------------------------------ sparse GCN layer
def _gcn(g, x, W, b, dy, flags, scatter, weighted=True):
    lib = _lib.load()
    n, fin = x.shape
    fout = W.shape[1]
    xd, Wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()
    y, ax, inv = Buf(n, fout, fout + 1), Buf(n, fin), Buf(n, 1)
    wsb = lib.dp_sparse_gcn_layer_workspace_bytes(n, fin, fout)
    ws = _ws(wsb)
    st = _lib.current_stream()
    head = (xd.data_ptr(), fin, g.indptr.data_ptr(), g.indices.data_ptr())
    tail = (Wd.data_ptr(), bd.data_ptr(), y.ptr(), fout + 1, ax.ptr(), inv.ptr(), n, fin, fout, flags, ws.data_ptr(), wsb,
            st)
    if weighted:
        _lib.check(lib.dp_sparse_gcn_layer_fwd_w(*head, g.values.data_ptr(), *tail), "dp_sparse_gcn_layer_fwd_w")
    else:
        _lib.check(lib.dp_sparse_gcn_layer_fwd(*head, *tail), "dp_sparse_gcn_layer_fwd")
    dyb = Buf(n, fout, fout + 3, data=dy)
    dx, dW, db = Buf(n, fin), Buf(fin, fout), Buf(1, fout)
    ipt, ixt = (None, None) if scatter else (g.indptr_t.data_ptr(), g.indices_t.data_ptr())
    tail = (Wd.data_ptr(), y.ptr(), fout + 1, inv.ptr(), dyb.ptr(), fout + 3, dx.ptr(), fin, dW.ptr(), db.ptr(), n, fin,
            fout, flags, ws.data_ptr(), wsb, st)
    if weighted:
        _lib.check(lib.dp_sparse_gcn_layer_bwd_w(ax.ptr(), g.indptr.data_ptr(), g.indices.data_ptr(),
                                                 g.values.data_ptr(), ipt, ixt,
                                                 None if scatter else g.values_t.data_ptr(), *tail),
                   "dp_sparse_gcn_layer_bwd_w")
    else:
        _lib.check(lib.dp_sparse_gcn_layer_bwd(ax.ptr(), g.indptr.data_ptr(), g.indices.data_ptr(), ipt, ixt, *tail),
                   "dp_sparse_gcn_layer_bwd")
    return {k: v.back() for k, v in dict(y=y, ax=ax, dx=dx, dW=dW, db=db).items()}


@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["plain", "add_self", "normalize", "add_self+normalize"])
@pytest.mark.parametrize("kind", ["undirected", "directed", "scatter"])
def test_sparse_gcn_layer_w_forward_and_backward(kind, flags):
    n, fin, fout = 203, 21, 34
    gh = WC.graph(n, 5, 11, directed=kind != "undirected")
    g, a = WC.to_device(gh, "cuda"), WC.dense(gh)
    if kind != "undirected":
        assert (a != a.T).any() and np.array_equal(WC.dense(gh, transposed=True), a)
    rng = np.random.default_rng(flags + 10)
    x = rng.standard_normal((n, fin)).astype(np.float32)
    W = (rng.standard_normal((fin, fout)) / np.sqrt(fin)).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, fout).astype(np.float32)
    dy = rng.standard_normal((n, fout)).astype(np.float32)
    scatter = kind == "scatter"
    got = _gcn(g, x, W, b, dy, flags, scatter)
    deg = WC.degrees(gh)
    deg_t = np.diff(gh.indptr_t.numpy().astype(np.int64))
    ref = WC.gcn_ref(a, x, W, b, dy, bool(flags & 1), bool(flags & 2), deg, deg_t, scatter)
    for name, (r, bound) in ref.items():
        val, clean = got[name]
        _check(f"gcn layer {kind} flags={flags} {name}", val.reshape(r.shape), r, bound, clean)
    again = _gcn(g, x, W, b, dy, flags, scatter)
    one = _gcn(_ones(g), x, W, b, dy, flags, scatter)
    plain = _gcn(g, x, W, b, dy, flags, scatter, weighted=False)
    for name in ref:
        if scatter and name == "dx":
            continue                                     # float atomics: the one form whose sum order is not fixed
        assert _bits(again[name][0]) == _bits(got[name][0]), name
        assert _bits(one[name][0]) == _bits(plain[name][0]), name


# ------------------------------------------------------------------ pooling
def _pool(g, S, Z, dXp, dAp, pad, dz_old, weighted=True, plan=None):
    """Forward and backward of the single-graph entries (plan None) or the batch entries; dict name -> Buf.back()."""
    lib = _lib.load()
    n, K = S.shape
    D = Z.shape[1]
    B = 1 if plan is None else g.num_graphs
    Sb, Zb = Buf(n, K, K + pad, data=S), Buf(n, D, D + pad, data=Z)
    Xp, Ap = Buf(B * K, D), Buf(B * K, K)
    dXb, dAb = torch.from_numpy(dXp).cuda(), torch.from_numpy(dAp).cuda()
    dS, dZ = Buf(n, K, K + pad), Buf(n, D, D + pad, data=dz_old)
    st = _lib.current_stream()
    wsb = lib.dp_csr_pool_workspace_bytes(n, K, D) if plan is None else \
        lib.dp_csr_pool_batch_workspace_bytes(plan.n_slabs, B, K, D)
    ws = _ws(wsb)
    head = (Sb.ptr(), K + pad, Zb.ptr(), D + pad, g.indptr.data_ptr(), g.indices.data_ptr())
    val = (g.values.data_ptr(),) if weighted else ()
    tr = (g.indptr_t.data_ptr(), g.indices_t.data_ptr()) + ((g.values_t.data_ptr(),) if weighted else ())
    w = "_w" if weighted else ""
    if plan is None:
        _lib.check(getattr(lib, "dp_csr_pool_fwd" + w)(*head, *val, Xp.ptr(), Ap.ptr(), n, K, D, ws.data_ptr(), wsb, st))
        _lib.check(getattr(lib, "dp_csr_pool_bwd" + w)(*head, *val, *tr, dXb.data_ptr(), dAb.data_ptr(), dS.ptr(),
                                                       K + pad, dZ.ptr(), D + pad, n, K, D, ws.data_ptr(), wsb, st))
    else:
        _lib.check(getattr(lib, "dp_csr_pool_batch_fwd" + w)(*head, *val, plan.fwd_tab.data_ptr(),
                                                             plan.slab_off.data_ptr(), plan.n_slabs, Xp.ptr(), Ap.ptr(),
                                                             B, n, K, D, ws.data_ptr(), wsb, st))
        _lib.check(getattr(lib, "dp_csr_pool_batch_bwd" + w)(*head, *val, *tr, plan.bwd_tab.data_ptr(), plan.n_blocks,
                                                             dXb.data_ptr(), dAb.data_ptr(), dS.ptr(), K + pad, dZ.ptr(),
                                                             D + pad, B, n, K, D, ws.data_ptr(), wsb, st))
    return {k: v.back() for k, v in dict(Xp=Xp, Ap=Ap, dS=dS, dZ=dZ).items()}


def _pool_inputs(n, K, D, B, seed):
    gen = np.random.default_rng(seed)
    S = gen.random((n, K)).astype(np.float32)
    Z = (gen.random((n, D)) - 0.5).astype(np.float32)
    dXp = gen.standard_normal((B * K, D)).astype(np.float32)
    dAp = gen.standard_normal((B * K, K)).astype(np.float32)
    return S, Z, dXp, dAp, np.full((n, D), 0.25, dtype=np.float32)


def _pool_against_reference(case, gh, plan_sizes, K, D, pad):
    """One graph (plan_sizes None) or the ragged batch `gh` against the per-graph float64 reference."""
    g = WC.to_device(gh, "cuda")
    plan = None if plan_sizes is None else g.pool_plan(K, D)
    sizes = [gh.n] if plan_sizes is None else plan_sizes
    S, Z, dXp, dAp, dz_old = _pool_inputs(gh.n, K, D, len(sizes), gh.n + K + D)
    got = _pool(g, S, Z, dXp, dAp, pad, dz_old, plan=plan)
    a = WC.dense(gh)
    deg, deg_t = WC.degrees(gh), np.diff(gh.indptr_t.cpu().numpy().astype(np.int64))
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b in range(len(sizes)):
        r = slice(off[b], off[b + 1])
        ref, bound = WC.pool_ref(a[r, r], S[r], Z[r], dXp[b * K:(b + 1) * K], dAp[b * K:(b + 1) * K], dz_old[r], deg[r],
                                 deg_t[r])
        for name in ("Xp", "Ap"):
            _check(f"{case} {name}", got[name][0][b * K:(b + 1) * K], ref[name], bound[name], got[name][1])
        for name in ("dS", "dZ"):
            _check(f"{case} {name}", got[name][0][r], ref[name], bound[name], got[name][1])
    again = _pool(g, S, Z, dXp, dAp, pad, dz_old, plan=plan)
    one = _pool(_ones(g), S, Z, dXp, dAp, pad, dz_old, plan=plan)
    plain = _pool(g, S, Z, dXp, dAp, pad, dz_old, weighted=False, plan=plan)
    for name in got:
        assert _bits(again[name][0]) == _bits(got[name][0]), name
        assert _bits(one[name][0]) == _bits(plain[name][0]), name


@pytest.mark.parametrize("n,K,D,directed,pad", OP_CASES)
def test_csr_pool_w_single_graph_and_batch(n, K, D, directed, pad):
    tag = f"K={K} D={D}{' directed' if directed else ''}{' pad' if pad else ''}"
    _pool_against_reference(f"pool n={n} {tag}", WC.graph(n, 5, n * 7 + K, directed), None, K, D, pad)
    _pool_against_reference(f"pool batch {tag}", WC.batch(WC.BATCH_SIZES, 5, n + K, directed), WC.BATCH_SIZES, K, D, pad)


def test_csr_pool_w_forward_is_exact_on_an_integer_grid():
    n, K, D = 300, 50, 60
    gh = WC.graph(n, 5, 5, directed=True, grid=True)
    g, a = WC.to_device(gh, "cuda"), WC.dense(gh)
    rng = np.random.default_rng(2)
    S = rng.integers(0, 3, (n, K)).astype(np.float32)
    Z = rng.integers(-4, 5, (n, D)).astype(np.float32)
    zk, zd = np.zeros((K, D), np.float32), np.zeros((K, K), np.float32)
    got = _pool(g, S, Z, zk, zd, 0, np.zeros((n, D), np.float32))
    S64, Z64 = S.astype(np.float64), Z.astype(np.float64)
    assert np.array_equal(got["Xp"][0].astype(np.float64), S64.T @ Z64)
    assert np.array_equal(got["Ap"][0].astype(np.float64), S64.T @ (a @ S64))


# ------------------------------------------------------------------ link losses
def _link(g, S, pad, dloss, weighted=True, batch=False):
    lib = _lib.load()
    n, K = S.shape
    Sb = Buf(n, K, K + pad, data=S)
    loss, dS = Buf(1, 1), Buf(n, K, K + pad)
    dl = torch.tensor([dloss], dtype=torch.float32).cuda()
    st = _lib.current_stream()
    val = (g.values.data_ptr(),) if weighted else ()
    valt = (g.values_t.data_ptr(),) if weighted else ()
    w = "_w" if weighted else ""
    if batch:
        off = g.node_off_host.ctypes.data
        wsb = lib.dp_csr_linkpred_batch_workspace_bytes(off, g.num_graphs, K)
        ws = _ws(wsb)
        head = (Sb.ptr(), K + pad, g.indptr.data_ptr(), g.indices_local.data_ptr())
        _lib.check(getattr(lib, "dp_csr_linkpred_batch_loss_fwd" + w)(*head, *val, off, g.num_graphs, loss.ptr(), K,
                                                                      ws.data_ptr(), wsb, st))
        _lib.check(getattr(lib, "dp_csr_linkpred_batch_loss_bwd" + w)(*head, *val, g.indptr_t.data_ptr(),
                                                                      g.indices_t_local.data_ptr(), *valt, off,
                                                                      g.num_graphs, dl.data_ptr(), dS.ptr(), K + pad, 0, K,
                                                                      ws.data_ptr(), wsb, st))
    else:
        wsb = lib.dp_csr_linkpred_workspace_bytes(n, K)
        ws = _ws(wsb)
        head = (Sb.ptr(), K + pad, g.indptr.data_ptr(), g.indices.data_ptr())
        _lib.check(getattr(lib, "dp_csr_linkpred_loss_fwd" + w)(*head, *val, loss.ptr(), n, K, ws.data_ptr(), wsb, st))
        _lib.check(getattr(lib, "dp_csr_linkpred_loss_bwd" + w)(*head, *val, g.indptr_t.data_ptr(),
                                                                g.indices_t.data_ptr(), *valt, dl.data_ptr(), dS.ptr(),
                                                                K + pad, 0, n, K, ws.data_ptr(), wsb, st))
    return dict(loss=loss.back(), dS=dS.back())


def _graph_list(gh, sizes, S):
    a = WC.dense(gh)
    deg, deg_t = WC.degrees(gh), np.diff(gh.indptr_t.cpu().numpy().astype(np.int64))
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(a[off[b]:off[b + 1], off[b]:off[b + 1]], S[off[b]:off[b + 1]], deg[off[b]:off[b + 1]],
             deg_t[off[b]:off[b + 1]]) for b in range(len(sizes))]


FORMS = ["graph", "directed", "batch", "directed batch"]


def _form(form, seed):
    directed, is_batch = form.startswith("directed"), form.endswith("batch")
    gh = WC.batch(WC.BATCH_SIZES, 4, seed, directed) if is_batch else WC.graph(300, 4, seed, directed)
    return gh, ([gh.n] if not is_batch else WC.BATCH_SIZES), is_batch


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", WC.LINK_K)
def test_csr_linkpred_w(K, form):
    gh, sizes, is_batch = _form(form, 40 + K)
    g = WC.to_device(gh, "cuda")
    S = WC.assign_rows(np.random.default_rng(K), gh.n, K)
    pad, dloss = (3 if K % 2 else 0), 1.7
    got = _link(g, S, pad, dloss, batch=is_batch)
    ref = WC.link_ref(_graph_list(gh, sizes, S), dloss)
    case = f"linkpred {form} K={K}"
    _check(case + " loss", got["loss"][0].reshape(()), np.float64(ref["loss"]), np.float64(ref["loss_bound"]),
           got["loss"][1])
    _check(case + " dS", got["dS"][0], ref["dS"], ref["dS_bound"], got["dS"][1])
    again = _link(g, S, pad, dloss, batch=is_batch)
    one = _link(_ones(g), S, pad, dloss, batch=is_batch)
    plain = _link(g, S, pad, dloss, weighted=False, batch=is_batch)
    for name in got:
        assert _bits(again[name][0]) == _bits(got[name][0]), name
        assert _bits(one[name][0]) == _bits(plain[name][0]), name


def _frob(g, S, dloss, weighted=True, batch=False):
    lib = _lib.load()
    n, K = S.shape
    B = g.num_graphs if batch else 1
    Sd = torch.from_numpy(S).cuda()
    W, G, loss, dS = Buf(n, K), Buf(B * K, K), Buf(1, 1), Buf(n, K)
    dl = torch.tensor([dloss], dtype=torch.float32).cuda()
    wsb = lib.dp_csr_frob_link_workspace_bytes(n, B, K)
    ws = _ws(wsb)
    st = _lib.current_stream()
    directed = g.indices_t is not g.indices
    csr = (Sd.data_ptr(), K, g.indptr.data_ptr(), g.indices.data_ptr()) + ((g.values.data_ptr(),) if weighted else ()) \
        + ((g.indptr_t.data_ptr(), g.indices_t.data_ptr()) if directed else (None, None)) \
        + (((g.values_t.data_ptr() if directed else None),) if weighted else ())
    w = "_w" if weighted else ""
    if batch:
        _lib.check(getattr(lib, "dp_csr_frob_link_batch_fwd" + w)(*csr, g.node_off.data_ptr(), None, W.ptr(), G.ptr(),
                                                                  loss.ptr(), None, B, n, K, ws.data_ptr(), wsb, st))
        _lib.check(lib.dp_csr_frob_link_batch_bwd(Sd.data_ptr(), K, W.ptr(), G.ptr(), g.node_off.data_ptr(), None,
                                                  dl.data_ptr(), dS.ptr(), K, 0, int(not directed), B, n, K, st))
    else:
        _lib.check(getattr(lib, "dp_csr_frob_link_fwd" + w)(*csr, None, W.ptr(), G.ptr(), loss.ptr(), None, n, K,
                                                            ws.data_ptr(), wsb, st))
        _lib.check(lib.dp_csr_frob_link_bwd(Sd.data_ptr(), K, W.ptr(), G.ptr(), None, dl.data_ptr(), dS.ptr(), K, 0,
                                            int(not directed), n, K, st))
    return {k: v.back() for k, v in dict(loss=loss, dS=dS, W=W, G=G).items()}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", FC.K_CASES)
def test_csr_frob_link_w(K, form):
    gh, sizes, is_batch = _form(form, 90 + K)
    g = WC.to_device(gh, "cuda")
    S = WC.assign_rows(np.random.default_rng(K + 1), gh.n, K)
    dloss = 1.75
    got = _frob(g, S, dloss, batch=is_batch)
    ref = WC.frob_ref([(a, s) for a, s, _, _ in _graph_list(gh, sizes, S)])
    case = f"frobenius {form} K={K}"
    _check(case + " loss", got["loss"][0].reshape(()), np.float64(ref["loss"]), np.float64(ref["loss_bound"]),
           got["loss"][1])
    _check(case + " dS", got["dS"][0], ref["dS_all"] * dloss, ref["dS_bound"] * dloss + 2 * WC.U * np.abs(ref["dS_all"]),
           got["dS"][1])
    assert got["W"][1] and got["G"][1]
    again = _frob(g, S, dloss, batch=is_batch)
    one = _frob(_ones(g), S, dloss, batch=is_batch)
    plain = _frob(g, S, dloss, weighted=False, batch=is_batch)
    for name in got:
        assert _bits(again[name][0]) == _bits(got[name][0]), name
        assert _bits(one[name][0]) == _bits(plain[name][0]), name
