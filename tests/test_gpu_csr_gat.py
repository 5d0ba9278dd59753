"""The fused additive attention through the C ABI (dp_csr_gat_fwd / _bwd): every row of tests/csr_gat_cases.py against
float64 under the bounds derived there; u, v, rowstat and the workspace at the case's leading dimension and base (NaN in
the padding), the [nnz] vectors one float off their allocation with NaN behind them, guard bands around every buffer,
NaN-filled outputs; every case twice, bit for bit; the exact cases (a one-entry row, rows of 2^k entries with equal v, an
empty row, an empty column, a zero gradient); H = 1 against dp_csr_edge_softmax_fwd on the same scores; calls with
nothing to do; and one 2^18-node ring lattice for the grid.

With DP_CSR_GAT_ANCHOR=<file> the largest |error| / bound per entry and case is written there
(profiles/csr_gat_fp64_anchor.txt is such a run of this file alone)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import CsrGraph
from tests import csr_edge_ops_cases as OC
from tests import csr_gat_cases as GC
from tests.test_gpu_csr_edge_grad import Buf, _stream
from tests.test_gpu_csr_edge_ops import _in, _out

pytestmark = pytest.mark.gpu

RATIOS = {}


def _note(case, ratio):
    print(f"{case}: |error| / bound = {ratio:.4f}")
    RATIOS[case] = max(RATIOS.get(case, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_GAT_ANCHOR")
    if path and RATIOS:
        per = {}
        for k, v in RATIOS.items():
            per[k.split()[0]] = max(per.get(k.split()[0], 0.0), v)
        lines = ["largest |error| / bound (bounds: tests/csr_gat_cases.py, u = 2^-24)", "", "per entry"]
        lines += [f"{k:<64s} {per[k]:8.4f}" for k in sorted(per)]
        lines += ["", "per case"] + [f"{k:<64s} {RATIOS[k]:8.4f}" for k in sorted(RATIOS)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


_DEV = {}


def dev_graph(name):
    """The case graph's index arrays on the device (int32), made once: indptr, indices, indptr_t, indices_t, mirror."""
    if name not in _DEV:
        g = GC.graph(name)
        _DEV[name] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
                           for a in (g.indptr, g.indices, g.indptr_t, g.indices_t, g.mirror))
    return _DEV[name]


def _check(what, got, ref, bound):
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} entries not written"
    ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max()) if got.size else 0.0
    _note(what, ratio)
    assert ratio <= 1.0, f"{what}: |error| / bound = {ratio:.3f}"


def _twice(run, make):
    """Run `run(*make())` twice on fresh outputs; the first run's windows after checking guards and equal bits."""
    got = []
    for _ in range(2):
        bufs = make()
        run(*bufs)
        torch.cuda.synchronize()
        back = [b.back() for b in bufs]
        assert all(clean for _, clean in back), "wrote outside its window"
        got.append([w for w, _ in back])
    for a, b in zip(*got):
        assert np.array_equal(a, b, equal_nan=True), "repeat runs differ"
    return got[0]


def _node_buf(case, data=None, cols=None):
    """[n, H] (or [n, cols]) at the case's layout: NaN in the padding and, for an output, in the window."""
    g = GC.graph(case[0])
    ld, off = GC.layout_of(case)
    if cols is None:
        return Buf(g.n, case[1], ld, data, off=off)
    return Buf(g.n, cols, data=data, off=off)             # rowstat [n, 2H] and tdot [n, H] are dense


def _forward(case, u, v):
    g, H = GC.graph(case[0]), case[1]
    ip, ix = dev_graph(case[0])[:2]
    lib = _lib.load()
    bu, bv = _node_buf(case, u), _node_buf(case, v)
    plan = (_lib.C.c_int * _lib.CSR_GAT_PLAN_INTS)()
    _lib.check(lib.dp_csr_gat_plan(g.n, g.nnz, H, bv.ld, bv.ptr() % 16 != 0, plan))
    assert tuple(plan) == GC.case_plan(case)
    out, stat = _twice(lambda bo, bs: _lib.check(lib.dp_csr_gat_fwd(
        bu.ptr(), bu.ld, bv.ptr(), bv.ld, ip.data_ptr(), ix.data_ptr(), bo.ptr(), bs.ptr(), g.n, g.nnz, H, case[4],
        _stream()), "dp_csr_gat_fwd"), lambda: [_out(g.nnz), _node_buf(case, cols=2 * H)])
    assert bu.back()[1] and bv.back()[1]
    return out.reshape(-1), stat, bu, bv


@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_forward_and_backward_against_fp64(case):
    g, H, slope = GC.graph(case[0]), case[1], case[4]
    ip, ix, ipt, ixt, mir = dev_graph(case[0])
    lib = _lib.load()
    u, v = GC.inputs(case)
    out, stat, bu, bv = _forward(case, u, v)
    ref, bound, sref, sbound = GC.fwd_ref(g, u, v, slope)
    tag = GC.case_id(case)
    _check("dp_csr_gat_fwd " + tag, out, ref, bound)
    _check("dp_csr_gat_fwd(rowstat) " + tag, stat, sref, sbound)
    lens = GC.row_len(g)
    per = lens[g.rows]
    assert np.array_equal(out[per == 1], np.ones((per == 1).sum(), np.float32))          # exactly 1.0
    assert not stat[lens == 0].any()                                                      # an empty row: zeros
    if case[3] == "equal" and H in (1, 2, 4, 8):
        pow2 = (per & (per - 1)) == 0
        assert pow2.any() and np.array_equal(out[pow2].astype(np.float64), 1.0 / per[pow2])      # exactly 2^-k
    # the backward on the forward's own rowstat (the reference takes the fp32 rowstat as its input)
    dout = GC.bwd_inputs(case)[1]
    bs, bg = _node_buf(case, stat, cols=2 * H), _in(dout)
    run = lambda bt, bdu, bdv: _lib.check(lib.dp_csr_gat_bwd(
        bu.ptr(), bu.ld, bv.ptr(), bv.ld, ip.data_ptr(), ix.data_ptr(), ipt.data_ptr(), ixt.data_ptr(), mir.data_ptr(),
        bs.ptr(), bg.ptr(), bt.ptr(), bdu.ptr(), bdu.ld, bdv.ptr(), bdv.ld, g.n, g.nnz, H, slope, _stream()),
        "dp_csr_gat_bwd")
    t, du, dv = _twice(run, lambda: [_node_buf(case, cols=H), _node_buf(case), _node_buf(case)])
    assert bu.back()[1] and bv.back()[1] and bs.back()[1] and bg.back()[1]
    rdu, dub, rdv, dvb, rt, tb = GC.bwd_ref(g, u, v, stat, dout, slope)
    _check("dp_csr_gat_bwd(du) " + tag, du, rdu, dub)
    _check("dp_csr_gat_bwd(dv) " + tag, dv, rdv, dvb)
    _check("dp_csr_gat_bwd(tdot) " + tag, t, rt, tb)
    assert not du[lens <= 1].any()                        # no entry: zeros written; one entry: exactly 0
    assert not dv[GC.col_len(g) == 0].any()               # a column without entries: a zero row


@pytest.mark.parametrize("case", [c for c in GC.CASES if c[3] == "ordinary" and c[4] == 0.2 and c[2] == "tight"][:6],
                         ids=GC.case_id)
def test_a_zero_gradient_and_a_one_entry_row_give_exact_zeros(case):
    """dout = 0 gives du = dv = 0 exactly; with dout non-zero on the one-entry rows ONLY, every gradient is exactly 0:
    such a row contributes nothing."""
    g, H = GC.graph(case[0]), case[1]
    ip, ix, ipt, ixt, mir = dev_graph(case[0])
    lib = _lib.load()
    u, v = GC.inputs(case)
    _, stat, bu, bv = _forward(case, u, v)
    bs = _node_buf(case, stat, cols=2 * H)
    single = GC.row_len(g)[g.rows] == 1
    assert single.any()
    for dout in (np.zeros(g.nnz, np.float32), np.where(single, np.float32(0.75), np.float32(0))):
        bg, bt, bdu, bdv = _in(dout), _node_buf(case, cols=H), _node_buf(case), _node_buf(case)
        _lib.check(lib.dp_csr_gat_bwd(bu.ptr(), bu.ld, bv.ptr(), bv.ld, ip.data_ptr(), ix.data_ptr(), ipt.data_ptr(),
                                      ixt.data_ptr(), mir.data_ptr(), bs.ptr(), bg.ptr(), bt.ptr(), bdu.ptr(), bdu.ld,
                                      bdv.ptr(), bdv.ld, g.n, g.nnz, H, case[4], _stream()), "dp_csr_gat_bwd")
        torch.cuda.synchronize()
        (du, c1), (dv, c2) = bdu.back(), bdv.back()
        assert c1 and c2 and not du.any() and not dv.any()


@pytest.mark.parametrize("case", [c for c in GC.CASES if c[1] == 1], ids=GC.case_id)
def test_one_head_against_the_edge_softmax_of_the_same_scores(case):
    """H = 1: the mean is the coefficient itself.  dp_csr_edge_softmax_fwd on the fp32 scores lies within its own bound
    of its fp64 result, which lies within the score part of this op's bound of this op's: the sum of both bounds."""
    g = GC.graph(case[0])
    ip = dev_graph(case[0])[0]
    lib = _lib.load()
    u, v = GC.inputs(case)
    out = _forward(case, u, v)[0]
    s32 = GC._scores32(g, u, v, case[4])[1].reshape(-1)
    bs, bo = _in(s32), _out(g.nnz)
    _lib.check(lib.dp_csr_edge_softmax_fwd(bs.ptr(), ip.data_ptr(), bo.ptr(), g.n, g.nnz, _stream()))
    torch.cuda.synchronize()
    soft, clean = bo.back()
    assert clean
    bound = OC.softmax_ref(g, s32, lanes=GC.case_plan(case)[0])[1] + GC.fwd_ref(g, u, v, case[4])[1]
    ratio = float((np.abs(out.astype(np.float64) - soft.reshape(-1)) / bound).max())
    _note("gat(H=1)-vs-edge-softmax " + GC.case_id(case), ratio)
    assert ratio <= 1.0


def test_calls_with_nothing_to_do():
    """n_rows == 0 or nnz == 0: the forward writes nothing; the backward with nnz == 0 and n > 0 writes the zero du, dv."""
    lib = _lib.load()
    case = ("batch", 3, "odd", "ordinary", 0.2)
    g = GC.graph("batch")
    ip, ix, ipt, ixt, mir = dev_graph("batch")
    zero_ip = torch.zeros(g.n + 1, dtype=torch.int32, device="cuda")
    u, v = GC.inputs(case)
    bu, bv = _node_buf(case, u), _node_buf(case, v)
    bo, bs = _out(g.nnz), _node_buf(case, cols=6)
    for n_rows, nnz in ((0, g.nnz), (g.n, 0)):
        _lib.check(lib.dp_csr_gat_fwd(bu.ptr(), bu.ld, bv.ptr(), bv.ld, ip.data_ptr(), ix.data_ptr(), bo.ptr(), bs.ptr(),
                                      n_rows, nnz, 3, 0.2, _stream()))
    torch.cuda.synchronize()
    for b in (bo, bs):
        got, clean = b.back()
        assert clean and np.isnan(got).all()
    bg = _in(np.ones(g.nnz))
    stat = _node_buf(case, np.zeros((g.n, 6)), cols=6)
    bt, bdu, bdv = _node_buf(case, cols=3), _node_buf(case), _node_buf(case)
    bwd = lambda iptr, n, nnz: _lib.check(lib.dp_csr_gat_bwd(
        bu.ptr(), bu.ld, bv.ptr(), bv.ld, iptr.data_ptr(), ix.data_ptr(), iptr.data_ptr(), ixt.data_ptr(), mir.data_ptr(),
        stat.ptr(), bg.ptr(), bt.ptr(), bdu.ptr(), bdu.ld, bdv.ptr(), bdv.ld, n, nnz, 3, 0.2, _stream()))
    bwd(ip, 0, g.nnz)
    torch.cuda.synchronize()
    for b in (bdu, bdv):
        got, clean = b.back()
        assert clean and np.isnan(got).all()
    bwd(zero_ip, g.n, 0)
    torch.cuda.synchronize()
    for b in (bdu, bdv):
        got, clean = b.back()
        assert clean and got.shape == (g.n, 3) and not got.any()


def test_a_ring_lattice_of_2_to_the_18_nodes():
    """4096 workgroups of the 4-lane tier through `ops.csr_gat_attention`: with v equal along every row the six
    coefficients are 1/6 within the forward bound (n_l = 2, D = 0, S <= 6), the rows sum to 1 and du, dv are finite; a
    uniform gradient gives du = 0 within rounding (sum_row a (g - t) = 0)."""
    n, H = 1 << 18, 4
    i = np.arange(n)
    src, dst = np.repeat(i, 3), (np.repeat(i, 3) + np.tile([1, 2, 3], n)) % n
    c = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    assert c.nnz == 6 * n and GC.plan(n, c.nnz, H, H, 0)[:2] == (4, 4)
    gen = torch.Generator().manual_seed(8)
    u = (3 * torch.rand(n, H, generator=gen)).cuda().requires_grad_(True)
    v = torch.full((n, H), 0.5, device="cuda", requires_grad=True)
    a = ops.csr_gat_attention(u, v, c)
    assert float((a.detach().double() - 1 / 6).abs().max()) <= ((6 * 2 + 2 + 14 + 4 * 6) + H + 1) * GC.U / 6
    a.backward(torch.ones_like(a))
    assert torch.isfinite(u.grad).all() and torch.isfinite(v.grad).all()
    assert float(u.grad.abs().max()) <= 64 * GC.U and float(v.grad.abs().max()) <= 64 * GC.U
    v2 = torch.randn(n, H, generator=gen).cuda()
    a2 = ops.csr_gat_attention(u.detach(), v2, c)
    assert float((a2.double().view(n, 6).sum(1) - 1).abs().max()) <= 128 * GC.U      # six entries of rho <= 100 u a_e
