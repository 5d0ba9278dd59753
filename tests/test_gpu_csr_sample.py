"""The fused sampled neighbour mean through the C ABI (dp_csr_sample_mean_fwd / _bwd): every row of
tests/csr_sample_cases.py.  thr and cnt equal the numpy restatement EXACTLY (which pins the sampled sets, not only their
means); y and dx lie within the derived bounds of float64.  Every input lies at the case's leading dimension and base
with NaN in its padding and a NaN row behind it, every output is NaN-filled inside guard bands that must stay untouched,
and every case runs twice, bit for bit.  The exact statements: the same seed gives the same bits and another seed moves
thr on the rows with d > k and on no others; k at or above the longest row with self_mode none gives the bits of
dp_mean_aggregate_fwd on the rows that hold anything and zeros on the others; data on the grid of 2^-6 gives the fp64
value itself where cnt is a power of two; k = 65 is refused; calls with nothing to do launch nothing.

With DP_CSR_SAMPLE_ANCHOR=<file> the largest |error| / bound per output and case is written there
(profiles/csr_sample_fp64_anchor.txt is such a run of this file alone)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_sample_cases as SC
from tests.test_gpu_csr_edge_grad import Buf, _stream

pytestmark = pytest.mark.gpu

RATIOS = {}


def _note(what, ratio):
    print(f"{what}: |error| / bound = {ratio:.4f}")
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_SAMPLE_ANCHOR")
    if path and RATIOS:
        per = {}
        for k, v in RATIOS.items():
            per[k.split()[0]] = max(per.get(k.split()[0], 0.0), v)
        lines = ["largest |error| / bound (bounds: tests/csr_sample_cases.py, u = 2^-24)", "", "per output"]
        lines += [f"{k:<72s} {per[k]:8.4f}" for k in sorted(per)]
        lines += ["", "per case"] + [f"{k:<72s} {RATIOS[k]:8.4f}" for k in sorted(RATIOS)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


_DEV = {}


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def dev_graph(name):
    """The case graph's index arrays on the device (int32), made once: indptr, indices, indptr_t, indices_t.  An
    undirected graph hands the forward's arrays over as the transposed ones."""
    if name not in _DEV:
        g = SC.graph(name)
        ip, ix = _i32(g.indptr), _i32(g.indices)
        _DEV[name] = (ip, ix, _i32(g.indptr_t), _i32(g.indices_t)) if g.directed else (ip, ix, ip, ix)
    return _DEV[name]


def dev_targets(gname, which):
    """(nodes, slot) on the device, or (None, None) for every node."""
    key = (gname, which)
    if key not in _DEV:
        t = SC.targets(gname, which)
        if t is None:
            _DEV[key] = (None, None)
        else:
            slot = np.full(SC.graph(gname).n, -1, dtype=np.int32)
            slot[t] = np.arange(t.size)
            _DEV[key] = (_i32(t), _i32(slot))
    return _DEV[key]


def _in(x, ld, off):
    """An input [rows, cols] at leading dimension ld: NaN in the padding and in one more row behind the last."""
    full = np.vstack([SC.padded(x, ld), np.full((1, ld), np.nan, np.float32)])
    return Buf(x.shape[0] + 1, ld, ld, full, off=off)


def _check(what, got, ref, bound):
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} entries not written"
    ratio = SC.moved(ref, got, bound)
    _note(what, ratio)
    assert ratio <= 1.0, f"{what}: |error| / bound = {ratio:.3f}"


class Run:
    """The case's inputs on the device and the two entries on them."""

    def __init__(self, case, grid=False, seed=SC.SEED):
        self.case, self.seed = case, seed
        gname, self.k, self.F, _, self.mode, which = case
        self.g = SC.graph(gname)
        self.s = SC.sample(gname, self.k, self.mode, which, seed)
        self.wy = 2 * self.F if self.mode == "concat" else self.F
        self.x, self.dy = SC.inputs(case, grid)
        (self.ldx, self.off), (self.ldy, _) = SC.layout_of(case, self.F), SC.layout_of(case, self.wy)
        self.bx = _in(self.x, self.ldx, self.off)
        self.lib = _lib.load()
        self.ix = dev_graph(gname)
        self.nodes, self.slot = dev_targets(gname, which)
        self.seed64 = seed - (1 << 64) if seed >= 1 << 63 else seed

    def forward(self):
        """(y, thr uint64, cnt) of two identical runs."""
        g, s, (ip, ix, _, _) = self.g, self.s, self.ix
        got = []
        for _ in range(2):
            by = Buf(s.m, self.wy, self.ldy, off=self.off)
            thr = torch.full((s.m + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            cnt = torch.full((s.m + 2,), -7, dtype=torch.int32, device="cuda")
            _lib.check(self.lib.dp_csr_sample_mean_fwd(
                self.bx.ptr(), self.ldx, ip.data_ptr(), ix.data_ptr(), _lib.ptr(self.nodes), by.ptr(), by.ld,
                thr.data_ptr() + 8, cnt.data_ptr() + 4, s.m, g.n, self.F, self.k, SC.MODES[self.mode], self.seed64,
                _stream()), "dp_csr_sample_mean_fwd")
            torch.cuda.synchronize()
            y, clean = by.back()
            thr, cnt = thr.cpu().numpy(), cnt.cpu().numpy()
            assert clean and self.bx.back()[1], "wrote outside its window"
            assert thr[0] == thr[-1] == 0x5A5A5A5A5A5A5A5A and cnt[0] == cnt[-1] == -7
            got.append((y, thr[1:-1].view(np.uint64), cnt[1:-1]))
        for a, b in zip(*got):
            assert np.array_equal(a, b, equal_nan=True), "repeat runs differ"
        return got[0]

    def backward(self, thr, cnt):
        g, s, (_, _, ipt, ixt) = self.g, self.s, self.ix
        bg = _in(self.dy, self.ldy, self.off)
        thr_d = torch.from_numpy(thr.view(np.int64).copy()).cuda()
        cnt_d = torch.from_numpy(np.ascontiguousarray(cnt, dtype=np.int32)).cuda()
        got = []
        for _ in range(2):
            bdx = Buf(g.n, self.F, self.ldx, off=self.off)
            _lib.check(self.lib.dp_csr_sample_mean_bwd(
                bg.ptr(), self.ldy, ipt.data_ptr(), ixt.data_ptr(), _lib.ptr(self.slot), thr_d.data_ptr(),
                cnt_d.data_ptr(), bdx.ptr(), bdx.ld, g.n, self.F, SC.MODES[self.mode], self.seed64, _stream()),
                "dp_csr_sample_mean_bwd")
            torch.cuda.synchronize()
            dx, clean = bdx.back()
            assert clean and bg.back()[1], "wrote outside its window"
            got.append(dx)
        assert np.array_equal(got[0], got[1], equal_nan=True), "repeat runs differ"
        return got[0]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_forward_and_backward_against_fp64(case):
    r = Run(case)
    s, tag = r.s, SC.case_id(case)
    y, thr, cnt = r.forward()
    assert np.array_equal(thr, s.thr), f"thr differs on {int((thr != s.thr).sum())} rows"      # the sampled sets themselves
    assert np.array_equal(cnt, s.cnt), f"cnt differs on {int((cnt != s.cnt).sum())} rows"
    ref, bound = SC.fwd_ref(s, r.x)
    _check("dp_csr_sample_mean_fwd " + tag, y, ref, bound)
    mean = y[:, r.F:] if r.mode == "concat" else y
    assert not mean[s.cnt == 0].any()                                 # an empty sample: zeros, not 0 / 0
    if r.mode == "concat":
        assert np.array_equal(y[:, :r.F], r.x[s.nodes])               # x_i copied bit for bit
    dx = r.backward(thr, cnt)
    dref, dbound = SC.bwd_ref(s, r.dy)
    _check("dp_csr_sample_mean_bwd " + tag, dx, dref, dbound)
    assert not dx[dbound == SC.FLT_MIN].any()                        # nothing sampled there: exactly zero


@pytest.mark.parametrize("case", [("directed", 10, 65, "odd", "gcn", "subset"),
                                  ("undirected", 25, 64, "tight", "none", "all"),
                                  ("batch", 2, 5, "mis", "concat", "all")], ids=SC.case_id)
def test_the_seed_decides_the_sample(case):
    """The same seed: the same thr, cnt and bits of y and dx (a fresh set of buffers).  Another seed: thr moves on the
    rows with more than k entries and on no others, and the result follows the new restatement."""
    a, b = Run(case), Run(case)
    ya, ta, ca = a.forward()
    yb, tb, cb = b.forward()
    assert np.array_equal(ya, yb) and np.array_equal(ta, tb) and np.array_equal(ca, cb)
    assert np.array_equal(a.backward(ta, ca), b.backward(tb, cb))
    for seed in (SC.SEED + 1, 1, (1 << 64) - 1, 1 << 32):
        o = Run(case, seed=seed)
        yo, to, co = o.forward()
        lens = SC.row_len(a.g)[a.s.nodes]
        assert np.array_equal(to != ta, lens > a.k)
        assert np.array_equal(to, o.s.thr) and np.array_equal(co, o.s.cnt)
        _check(f"other-seed {seed:#x} " + SC.case_id(case), yo, *SC.fwd_ref(o.s, o.x))
        assert not np.array_equal(yo, ya)


@pytest.mark.parametrize("gname,k,F,layout", [("directed", SC.ALL, 65, "odd"), ("undirected", SC.ALL, 64, "tight"),
                                              ("batch", SC.ALL, 130, "pad4"), ("batch", 64, 63, "mis"),
                                              ("directed", SC.ALL, 1, "tight")])
def test_taking_every_neighbour_gives_the_bits_of_the_mean_aggregator(gname, k, F, layout):
    """Every neighbour taken (ALL: every row; k = 64: the rows of up to 64 entries, beside longer ones that are
    sampled), self_mode none: dp_mean_aggregate_fwd bit for bit on the rows with d >= 1 (it gives 0 / 0 = NaN on the
    others, where the sampled mean gives zeros)."""
    case = (gname, k, F, layout, "none", "all")
    r = Run(case)
    g = r.g
    lens = SC.row_len(g)
    g_rows = np.ones(g.n, bool) if k == SC.ALL else lens <= k        # the batch at k = 64: its rows up to 64 entries
    y, thr, cnt = r.forward()
    ip, ix, _, _ = r.ix
    out = Buf(g.n, F, r.ldy, off=r.off)
    _lib.check(r.lib.dp_mean_aggregate_fwd(r.bx.ptr(), r.ldx, ip.data_ptr(), ix.data_ptr(), out.ptr(), out.ld, g.n, F,
                                           _stream()), "dp_mean_aggregate_fwd")
    torch.cuda.synchronize()
    want, clean = out.back()
    assert clean
    some = g_rows & (lens >= 1)
    assert some.sum() >= 50 and np.array_equal(y[some], want[some])
    assert (thr[g_rows] == SC.THR_ALL).all() and np.array_equal(cnt[g_rows], lens[g_rows])
    assert (lens == 0).any() and not y[lens == 0].any() and np.isnan(want[lens == 0]).all()


@pytest.mark.parametrize("case", [("directed", 64, 65, "tight", "none", "all"),
                                  ("directed", 2, 130, "odd", "concat", "subset"),
                                  ("undirected", SC.ALL, 63, "pad4", "gcn", "all"), ("batch", 1, 64, "mis", "gcn", "subset"),
                                  ("undirected", 64, 1, "tight", "concat", "all")], ids=SC.case_id)
def test_data_on_a_coarse_grid_gives_the_fp64_value_where_cnt_is_a_power_of_two(case):
    r = Run(case, grid=True)
    s = r.s
    y, thr, cnt = r.forward()
    assert np.array_equal(thr, s.thr) and np.array_equal(cnt, s.cnt)
    ref, _ = SC.fwd_ref(s, r.x)
    pow2 = (s.cnt > 0) & ((s.cnt & (s.cnt - 1)) == 0)
    assert pow2.sum() >= 5
    assert np.array_equal(y[pow2].astype(np.float64), ref[pow2])
    # the backward: a column all of whose terms divide by powers of two
    dx = r.backward(thr, cnt)
    dref, _ = SC.bwd_ref(s, r.dy)
    W = s.weights()
    cols = np.array([all((c & (c - 1)) == 0 for c in s.cnt[np.nonzero(W[:, j])[0]]) for j in range(r.g.n)])
    assert cols.any() and W[:, cols].any()
    assert np.array_equal(dx[cols].astype(np.float64), dref[cols])


def test_k_65_is_refused():
    lib = _lib.load()
    g = SC.graph("batch")
    ip, ix, ipt, ixt = dev_graph("batch")
    x = torch.zeros(g.n, 4, device="cuda")
    y = torch.full((g.n, 4), 3.0, device="cuda")
    thr = torch.zeros(g.n, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(g.n, dtype=torch.int32, device="cuda")
    rc = lib.dp_csr_sample_mean_fwd(x.data_ptr(), 4, ip.data_ptr(), ix.data_ptr(), None, y.data_ptr(), 4, thr.data_ptr(),
                                    cnt.data_ptr(), g.n, g.n, 4, 65, 0, 1, _stream())
    assert rc == -1 and "k=65 must be 1 .. 64" in lib.dp_last_error_string().decode()
    torch.cuda.synchronize()
    assert (y == 3.0).all() and not thr.any() and not cnt.any()
    rc = lib.dp_csr_sample_mean_fwd(x.data_ptr(), 4, ip.data_ptr(), ix.data_ptr(), None, y.data_ptr(), 4, thr.data_ptr(),
                                    cnt.data_ptr(), g.n, g.n, 4, 64, 0, 1, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and not y.any()
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrGraph
    c = CsrGraph.from_edges(g.n, g.rows, g.indices, "cuda", symmetric=False)
    with pytest.raises(ValueError, match="num_sample must be 1 .. 64 or None"):
        ops.csr_sample_mean(x, c, 65, 1)
    assert ops.csr_sample_mean(x, c, 64, 1).shape == (g.n, 4)


def test_calls_with_nothing_to_do_launch_nothing():
    """n_rows == 0, n == 0 or F == 0: OK and nothing written; an edgeless graph with n > 0 writes zeros (none), x_i (gcn)
    and the all-ones thr."""
    case = ("batch", 10, 5, "odd", "gcn", "all")
    r = Run(case)
    g, lib = r.g, r.lib
    ip, ix, ipt, ixt = r.ix
    by, bdx = Buf(g.n, 5, r.ldy), Buf(g.n, 5, r.ldx)
    bg = _in(r.dy, r.ldy, 0)
    thr = torch.full((g.n,), 77, dtype=torch.int64, device="cuda")
    cnt = torch.full((g.n,), 77, dtype=torch.int32, device="cuda")

    def fwd(iptr, m, n, F, mode=1, nodes=None):
        _lib.check(lib.dp_csr_sample_mean_fwd(r.bx.ptr(), r.ldx, iptr.data_ptr(), ix.data_ptr(), _lib.ptr(nodes), by.ptr(),
                                              by.ld, thr.data_ptr(), cnt.data_ptr(), m, n, F, 10, mode, 5, _stream()))

    def bwd(iptr, n, F, mode=1):
        _lib.check(lib.dp_csr_sample_mean_bwd(bg.ptr(), r.ldy, iptr.data_ptr(), ixt.data_ptr(), None, thr.data_ptr(),
                                              cnt.data_ptr(), bdx.ptr(), bdx.ld, n, F, mode, 5, _stream()))

    fwd(ip, 0, 0, 5)
    fwd(ip, 0, g.n, 5, nodes=cnt)
    fwd(ip, g.n, g.n, 0)
    bwd(ipt, 0, 5)
    bwd(ipt, g.n, 0)
    torch.cuda.synchronize()
    for b in (by, bdx):
        got, clean = b.back()
        assert clean and np.isnan(got).all()
    assert (thr == 77).all() and (cnt == 77).all()
    zero_ip = torch.zeros(g.n + 1, dtype=torch.int32, device="cuda")
    fwd(zero_ip, g.n, g.n, 5, mode=0)
    torch.cuda.synchronize()
    got, clean = by.back()
    assert clean and not got.any() and (thr == -1).all() and not cnt.any()
    fwd(zero_ip, g.n, g.n, 5, mode=1)
    bwd(zero_ip, g.n, 5, mode=1)
    torch.cuda.synchronize()
    got, clean = by.back()
    assert clean and np.array_equal(got, r.x) and (cnt == 1).all()    # gcn on an edgeless graph: the node itself
    dgot, clean = bdx.back()
    assert clean and np.array_equal(dgot, r.dy)
