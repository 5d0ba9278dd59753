"""The learned-edge-weight entries through the C ABI (dp_csr_edge_softmax_fwd / _bwd, dp_csr_sym_norm_fwd / _bwd): every
row of tests/csr_edge_ops_cases.py against float64 under the bounds derived there; every buffer one float off its
allocation, guard bands around every output, NaN behind the stored entries of every input; every case twice, bit for
bit; the exact cases (a one-entry row, rows of 2^k equal scores, a zero gradient); `sym_normalized()` against
`normalized()`; the bit symmetry of the 'sym' form on the undirected graph; the batch against its graphs one by one; and
one 2^18-node ring lattice of degree 6 for the grid.

With DP_CSR_EDGE_OPS_ANCHOR=<file> the largest |error| / bound per entry and case is written there
(profiles/csr_edge_ops_fp64_anchor.txt is such a run of this file alone)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, EdgeAttention
from tests import csr_edge_ops_cases as OC
from tests.test_gpu_csr_edge_grad import Buf, _stream

pytestmark = pytest.mark.gpu

RATIOS = {}
NAN_TAIL = 8


def _note(case, ratio):
    print(f"{case}: |error| / bound = {ratio:.4f}")
    RATIOS[case] = max(RATIOS.get(case, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_EDGE_OPS_ANCHOR")
    if path and RATIOS:
        per = {}
        for k, v in RATIOS.items():
            per[k.split()[0]] = max(per.get(k.split()[0], 0.0), v)
        lines = ["largest |error| / bound (bounds: tests/csr_edge_ops_cases.py, u = 2^-24)", "", "per entry"]
        lines += [f"{k:<64s} {per[k]:8.4f}" for k in sorted(per)]
        lines += ["", "per case"] + [f"{k:<64s} {RATIOS[k]:8.4f}" for k in sorted(RATIOS)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _in(data):
    """An input vector one float off its allocation, with NaN behind its last entry."""
    data = np.asarray(data, dtype=np.float32)
    return Buf(1, data.size + NAN_TAIL, data=np.concatenate([data, np.full(NAN_TAIL, np.nan, np.float32)]), off=1)


def _out(n):
    """An output vector one float off its allocation, NaN-filled inside guard bands."""
    return Buf(1, n, off=1)


_DEV = {}


def dev_graph(name):
    """The case graph's index arrays on the device (int32), made once: indptr, indices, indptr_t, indices_t, mirror."""
    if name not in _DEV:
        g = OC.graph(name)
        _DEV[name] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
                           for a in (g.indptr, g.indices, g.indptr_t, g.indices_t, g.mirror))
    return _DEV[name]


def _twice(run, outs):
    """Run `run(*fresh outputs)` twice; returns the first run's windows after checking guards and equal bits."""
    got = []
    for _ in range(2):
        bufs = [_out(n) for n in outs]
        run(*bufs)
        torch.cuda.synchronize()
        back = [b.back() for b in bufs]
        assert all(clean for _, clean in back), "wrote outside its window"
        got.append([w.reshape(-1) for w, _ in back])
    for a, b in zip(*got):
        assert np.array_equal(a, b, equal_nan=True), "repeat runs differ"
    return got[0]


def _check(what, got, ref, bound, written=None):
    written = np.ones(got.size, dtype=bool) if written is None else written
    assert np.isfinite(got[written]).all(), f"{what}: {int((~np.isfinite(got[written])).sum())} entries not written"
    assert np.isnan(got[~written]).all(), f"{what}: wrote where nothing is stored"
    ratio = float((np.abs(got[written].astype(np.float64) - ref[written]) / bound[written]).max()) if written.any() else 0.0
    _note(what, ratio)
    assert ratio <= 1.0, f"{what}: |error| / bound = {ratio:.3f}"


# ------------------------------------------------------------------ edge softmax
def _softmax_fwd(gname, s):
    g = OC.graph(gname)
    ip = dev_graph(gname)[0]
    lib = _lib.load()
    bs = _in(s)
    (got,) = _twice(lambda bo: _lib.check(lib.dp_csr_edge_softmax_fwd(bs.ptr(), ip.data_ptr(), bo.ptr(), g.n, g.nnz,
                                                                      _stream()), "dp_csr_edge_softmax_fwd"), [g.nnz])
    assert bs.back()[1]
    return got


@pytest.mark.parametrize("case", OC.SOFTMAX_CASES, ids=OC.case_id)
def test_softmax_fwd_against_fp64(case):
    g = OC.graph(case[0])
    s = OC.softmax_inputs(case)
    got = _softmax_fwd(case[0], s)
    ref, bound = OC.softmax_ref(g, s)
    _check("dp_csr_edge_softmax_fwd " + OC.case_id(case), got, ref, bound)
    lens = OC.row_len(g)[g.rows]
    assert np.array_equal(got[lens == 1], np.ones((lens == 1).sum(), np.float32))          # exactly 1.0
    if case[1] == "equal":
        pow2 = (lens & (lens - 1)) == 0
        assert pow2.any() and np.array_equal(got[pow2].astype(np.float64), 1.0 / lens[pow2])      # exactly 2^-k


@pytest.mark.parametrize("case", OC.SOFTMAX_BWD_CASES, ids=OC.case_id)
def test_softmax_bwd_against_fp64(case):
    g = OC.graph(case[0])
    ip = dev_graph(case[0])[0]
    a, dout = OC.softmax_bwd_inputs(case)
    lib = _lib.load()
    ba, bg = _in(a), _in(dout)
    (got,) = _twice(lambda bo: _lib.check(lib.dp_csr_edge_softmax_bwd(ba.ptr(), bg.ptr(), ip.data_ptr(), bo.ptr(), g.n,
                                                                      g.nnz, _stream()), "dp_csr_edge_softmax_bwd"),
                    [g.nnz])
    ref, bound = OC.softmax_bwd_ref(g, a, dout)
    _check("dp_csr_edge_softmax_bwd " + OC.case_id(case), got, ref, bound)
    lens = OC.row_len(g)[g.rows]
    assert not got[lens == 1].any()                                  # a one-entry row: exactly 0
    if case[1] == "zero-grad":
        assert not got.any()


def test_softmax_with_nothing_to_do_writes_nothing():
    lib = _lib.load()
    g = OC.graph("batch")
    ip = dev_graph("batch")[0]
    bs, bo = _in(np.ones(g.nnz)), _out(g.nnz)
    for n_rows, nnz in ((0, g.nnz), (g.n, 0)):
        _lib.check(lib.dp_csr_edge_softmax_fwd(bs.ptr(), ip.data_ptr(), bo.ptr(), n_rows, nnz, _stream()))
        _lib.check(lib.dp_csr_edge_softmax_bwd(bs.ptr(), bs.ptr(), ip.data_ptr(), bo.ptr(), n_rows, nnz, _stream()))
    torch.cuda.synchronize()
    got, clean = bo.back()
    assert clean and np.isnan(got).all()


# ------------------------------------------------------------------ D^-1/2 A D^-1/2
def _sym_fwd(gname, values, null_mirror=False):
    g = OC.graph(gname)
    ip, ix, ipt, ixt, mir = dev_graph(gname)
    if null_mirror:                          # an undirected container: its own arrays stand for the transposed CSR
        ipt, ixt, mir = ip, ix, None
    lib = _lib.load()
    bv = None if values is None else _in(values)
    return _twice(lambda br, bo: _lib.check(lib.dp_csr_sym_norm_fwd(
        ip.data_ptr(), ix.data_ptr(), None if bv is None else bv.ptr(), ipt.data_ptr(), ixt.data_ptr(), _lib.ptr(mir),
        br.ptr(), bo.ptr(), g.n, g.nnz, _stream()), "dp_csr_sym_norm_fwd"), [g.n, g.nnz])


@pytest.mark.parametrize("case", OC.SYM_CASES, ids=OC.case_id)
def test_sym_norm_fwd_against_fp64(case):
    g = OC.graph(case[0])
    values = OC.sym_values(case)
    ref, bound, r, rbound = OC.sym_fwd_ref(g, values)
    for null_mirror in ((False, True) if not g.directed else (False,)):
        rdeg, out = _sym_fwd(case[0], values, null_mirror)
        tag = OC.case_id(case) + ("-nomirror" if null_mirror else "")
        _check("dp_csr_sym_norm_fwd " + tag, out, ref, bound)
        _check("dp_csr_sym_norm_fwd(rdeg) " + tag, rdeg, r, rbound)
        if not g.directed:
            assert np.array_equal(out, out[g.mirror])                # a_ij == a_ji bit for bit


@pytest.mark.parametrize("case", OC.SYM_CASES, ids=OC.case_id)
def test_sym_norm_bwd_against_fp64(case):
    g = OC.graph(case[0])
    ip, ix, ipt, ixt, mir = dev_graph(case[0])
    values, rdeg, dout = OC.sym_bwd_inputs(case)
    lib = _lib.load()
    bv, br, bg = (None if values is None else _in(values)), _in(rdeg), _in(dout)
    gdeg, dv = _twice(lambda bgd, bdv: _lib.check(lib.dp_csr_sym_norm_bwd(
        ip.data_ptr(), ix.data_ptr(), None if bv is None else bv.ptr(), ipt.data_ptr(), ixt.data_ptr(), mir.data_ptr(),
        br.ptr(), bg.ptr(), bgd.ptr(), bdv.ptr(), g.n, g.nnz, _stream()), "dp_csr_sym_norm_bwd"), [g.n, g.nnz])
    ref, bound, G, gbound = OC.sym_bwd_ref(g, values, rdeg, dout)
    _check("dp_csr_sym_norm_bwd " + OC.case_id(case), dv, ref, bound)
    _check("dp_csr_sym_norm_bwd(gdeg) " + OC.case_id(case), gdeg, G, np.maximum(gbound, OC.FLT_MIN))


def test_sym_norm_leaves_an_isolated_node_alone():
    """Node 2 has no entry in its row and none in its column: rdeg = inf, G = 0, and nothing else changes."""
    g = CsrGraph.from_edges(4, [0, 0, 1, 3], [0, 1, 3, 0], "cuda", symmetric=False)
    v = torch.tensor([1.0, 2.0, 3.0, 4.0], device="cuda", requires_grad=True)
    out = ops.csr_sym_normalize(v, g)
    out.backward(torch.ones(4, device="cuda"))
    d = np.array([5.0, 2.0, 0.0, 3.0])
    with np.errstate(divide="ignore"):
        r = 1.0 / np.sqrt(d)
    ref = np.array([1, 2, 3, 4.0]) * r[[0, 0, 1, 3]] * r[[0, 1, 3, 0]]
    assert np.allclose(out.detach().cpu().numpy(), ref, rtol=1e-6) and torch.isfinite(v.grad).all()
    with pytest.raises(ValueError, match=r"node 2 has degree <= 0"):
        g.with_values(v.detach()).sym_normalized(check=True)
    assert g.with_values(v.detach()).sym_normalized().values.isfinite().all()


# ------------------------------------------------------------------ the containers
def _container(name, weighted=True):
    g = OC.graph(name)
    w = g.values if weighted else None
    if g.off is None:
        if g.directed:
            return CsrGraph.from_edges(g.n, g.rows, g.indices, "cuda", symmetric=False, weight=w)
        keep = g.rows <= g.indices
        return CsrGraph.from_edges(g.n, g.rows[keep], g.indices[keep], "cuda", symmetric=True,
                                   weight=None if w is None else w[keep])
    gr = g.graph_of_row()[g.rows]
    parts = [(g.rows[gr == b] - g.off[b], g.indices[gr == b] - g.off[b], None if w is None else w[gr == b])
             for b in range(len(g.off) - 1)]
    return CsrBatch.from_edge_lists(np.diff(g.off), *zip(*[(s, d) for s, d, _ in parts]), "cuda", symmetric=False,
                                    weights=[p[2] for p in parts])


@pytest.mark.parametrize("name", ["t4-n577", "t64-n576", "undirected", "batch"])
@pytest.mark.parametrize("weighted", [False, True], ids=["01", "weighted"])
def test_sym_normalized_against_normalized(name, weighted):
    """`normalized()` is the fp64 result rounded once: half a u on top of the entry's bound."""
    g = OC.graph(name)
    c = _container(name, weighted)
    host, dev = c.normalized(), c.sym_normalized(check=True)
    assert type(dev) is type(c) and dev.indices is c.indices and dev.weighted
    ref, bound = OC.sym_fwd_ref(g, g.values if weighted else None)[:2]
    for a, b, perm in ((dev.values, host.values, None), (dev.values_t, host.values_t, g.mirror)):
        got, want = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        bd = bound + OC.U * np.abs(ref)
        ratio = float((np.abs(got - want) / (bd if perm is None else bd[perm])).max())
        _note(f"sym_normalized-vs-normalized {name}-{'weighted' if weighted else '01'}", ratio)
        assert ratio <= 1.0
    if not g.directed:
        assert dev.values_t is dev.values


def test_sym_attention_is_bit_symmetric_on_the_undirected_graph():
    g = OC.graph("undirected")
    torch.manual_seed(3)
    x = torch.randn(g.n, 9, device="cuda")
    for weighted in (False, True):
        c = _container("undirected", weighted)
        h = EdgeAttention(9, 8, norm="sym").cuda()(x, c)
        a = h.values.detach().cpu().numpy()
        assert h.indices_t is h.indices and h.values_t is h.values and np.isfinite(a).all() and (a > 0).all()
        assert np.array_equal(a, a[g.mirror])


@pytest.mark.parametrize("norm", ["softmax", "sym"])
def test_the_batch_equals_its_graphs_one_by_one(norm):
    """The edge pipeline of `EdgeAttention` on the block-diagonal CSR and on each graph alone (the projections are taken
    once: the GEMM's tiling may depend on the row count, the edge kernels' plan must not differ here — asserted)."""
    g = OC.graph("batch")
    b = _container("batch")
    torch.manual_seed(4)
    q, k = torch.randn(g.n, 8, device="cuda"), torch.randn(g.n, 8, device="cuda")

    def edge(q, k, c):
        if norm == "softmax":
            return ops.csr_edge_softmax(ops.csr_sddmm(q, k, c, 8 ** -0.5), c)
        return ops.csr_sym_normalize(torch.sigmoid(ops.csr_sddmm(q, q, c, 8 ** -0.5)) * c.values, c)

    whole = edge(q, k, b).cpu().numpy()
    gr = g.graph_of_row()[g.rows]
    for j in range(len(g.off) - 1):
        lo, hi = int(g.off[j]), int(g.off[j + 1])
        sel = gr == j
        one = CsrGraph.from_edges(hi - lo, g.rows[sel] - lo, g.indices[sel] - lo, "cuda", symmetric=False,
                                  weight=g.values[sel])
        assert OC.plan(one.n, one.nnz) == g.plan
        assert np.array_equal(edge(q[lo:hi], k[lo:hi], one).cpu().numpy(), whole[sel]), f"graph {j}"


def test_a_ring_lattice_of_2_to_the_18_nodes():
    """4096 workgroups of the 4-lane tier: every row holds its six neighbours, the softmax of equal scores is 1/6 and the
    normalised 0/1 lattice 1/6 as well (both within their bounds), and softmax rows sum to 1."""
    n = 1 << 18
    i = np.arange(n)
    src, dst = np.repeat(i, 3), (np.repeat(i, 3) + np.tile([1, 2, 3], n)) % n
    c = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    assert c.nnz == 6 * n and OC.plan(n, c.nnz)[0] == 4
    rng = np.random.default_rng(7)
    s = torch.from_numpy(rng.uniform(-3, 3, c.nnz).astype(np.float32)).cuda()
    a = ops.csr_edge_softmax(s, c)
    s64 = s.double().view(n, 6)
    ref = torch.softmax(s64, dim=1).view(-1)
    bound = (6 * 2 + 3 * 6 + 6 + 2 + 14) * OC.U * ref               # n_l = 2, D <= 6, |x - M| <= 6, log2 L = 2
    assert float(((a.double() - ref).abs() / bound).max()) <= 1.0
    flat = ops.csr_edge_softmax(torch.full((c.nnz,), 0.25, device="cuda"), c)
    assert float((flat.double() - 1 / 6).abs().max()) <= 40 * OC.U / 6
    norm = c.sym_normalized().values
    assert float((norm.double() - 1 / 6).abs().max()) <= 6 * OC.U / 6      # rho = 2 each, two products
