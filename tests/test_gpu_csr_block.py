"""The sampled frontier blocks through the C ABI (dp_csr_block_build, dp_csr_block_mean_fwd / _bwd) on
every row of tests/csr_block_cases.py.

The build: src, slot, n_src, thr and cnt equal the numpy restatement EXACTLY.  They are read back and validated on the
host (ascending, unique, in range, slot[src[s]] == s, -1 elsewhere) BEFORE any kernel reads through them.  Every buffer is
guarded and filled with 0xFF, the workspace is exactly the queried size with a guard behind it, every run is done twice.

The mean: with x_src = x[src], y equals dp_csr_sample_mean_fwd(x, nodes = T) BIT FOR BIT, dx_src equals the rows src of
dp_csr_sample_mean_bwd's dx bit for bit, and that dx is exactly zero on every row outside src; both also lie within the
sibling's fp64 bounds (fwd_from / bwd_from).  The empty target set launches nothing; k = 65 is refused."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_block_cases as BC
from tests import csr_sample_cases as SC
from tests.test_gpu_csr_edge_grad import Buf, _stream
from tests.test_gpu_csr_sample import _check, _i32, _in, dev_graph

pytestmark = pytest.mark.gpu

FF = -1                                      # every byte 0xFF
GUARD_INTS = 64


def _seed64(seed):
    return seed - (1 << 64) if seed >= 1 << 63 else seed


class IntBuf:
    """`count` int32 (or int64) between two guard bands, every byte 0xFF."""

    def __init__(self, count, dtype=torch.int32):
        self.count = count
        self.dev = torch.full((count + 2 * GUARD_INTS,), FF, dtype=dtype, device="cuda")
        self.size = self.dev.element_size()

    def ptr(self):
        return self.dev.data_ptr() + GUARD_INTS * self.size

    def back(self):
        h = self.dev.cpu().numpy()
        clean = (h[:GUARD_INTS] == FF).all() and (h[GUARD_INTS + self.count:] == FF).all()
        return h[GUARD_INTS:GUARD_INTS + self.count], bool(clean)


_RING_DEV = {}


def _ring_dev(n):
    if n not in _RING_DEV:
        _RING_DEV.clear()                                             # one ring on the device at a time
        g = BC.ring(n)
        _RING_DEV[n] = (_i32(g.indptr), _i32(g.indices))
    return _RING_DEV[n]


def build(g, ip, ix, nodes, k, seed, cap=None):
    """(src [n_src], slot [n], n_src, thr uint64 [m], cnt [m], cap) of two identical guarded runs, as host arrays."""
    lib = _lib.load()
    m = g.n if nodes is None else int(nodes.size)
    cap = (g.n if k == BC.ALL else min(g.n, m * (k + 1))) if cap is None else cap
    nodes_d = None if nodes is None else _i32(nodes)
    wsb = lib.dp_csr_block_workspace_bytes(g.n)
    assert wsb == BC.workspace_bytes(g.n) and wsb % 16 == 0
    got = []
    for _ in range(2):
        slot, src, cnt, count = IntBuf(g.n), IntBuf(max(cap, 1)), IntBuf(m), IntBuf(1)
        thr = IntBuf(m, torch.int64)
        ws = IntBuf(wsb // 4)                                         # exactly the queried size, a guard behind it
        assert ws.ptr() % 16 == 0
        _lib.check(lib.dp_csr_block_build(ip.data_ptr(), ix.data_ptr(), _lib.ptr(nodes_d), m, g.n, k, _seed64(seed),
                                          slot.ptr(), src.ptr(), cap, count.ptr(), thr.ptr(), cnt.ptr(), ws.ptr(), wsb,
                                          _stream()), "dp_csr_block_build")
        torch.cuda.synchronize()
        out = [b.back() for b in (src, slot, count, thr, cnt, ws)]
        assert all(clean for _, clean in out), "wrote outside its window"
        (s, _), (sl, _), (c, _), (t, _), (cn, _), _ = out
        n_src = int(c[0])
        assert 0 <= n_src <= cap
        assert (s[n_src:] == FF).all(), "src written beyond n_src"
        got.append((s[:n_src].copy(), sl.copy(), n_src, t.view(np.uint64).copy(), cn.copy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b), "repeat runs differ"
    return got[0] + (cap,)


def validate(src, slot, n_src, n):
    """What a host must hold before a kernel reads through a device-built block."""
    assert src.size == n_src and slot.size == n
    if n_src:
        assert src.min() >= 0 and src.max() < n and (np.diff(src) > 0).all(), "src not ascending, unique and in range"
    assert np.array_equal(slot[src], np.arange(n_src)), "slot[src[s]] != s"
    rest = np.ones(n, bool)
    rest[src] = False
    assert (slot[rest] == -1).all(), "slot outside src is not -1"


def _equals(got, b):
    src, slot, n_src, thr, cnt, _ = got
    assert n_src == b.n_src, f"n_src = {n_src}, restated {b.n_src}"
    assert np.array_equal(src, b.src), f"src differs at {int((src != b.src).sum())} positions"
    assert np.array_equal(slot, b.slot), f"slot differs at {int((slot != b.slot).sum())} nodes"
    assert np.array_equal(thr, b.thr), f"thr differs on {int((thr != b.thr).sum())} rows"
    assert np.array_equal(cnt, b.cnt), f"cnt differs on {int((cnt != b.cnt).sum())} rows"


# ------------------------------------------------------------------ the build
@pytest.mark.parametrize("case", [c for c in BC.BUILD_CASES if c[1] != "empty"], ids=BC.build_id)
def test_build_equals_the_restatement(case):
    gname, tname, k = case
    g, b = SC.graph(gname), BC.block(gname, tname, k)
    ip, ix, _, _ = dev_graph(gname)
    got = build(g, ip, ix, BC.targets(gname, tname, k), k, BC.SEED)
    validate(got[0], got[1], got[2], g.n)
    _equals(got, b)
    if tname in ("seven", "nested") and k != BC.ALL and k <= 10:
        assert got[2] < g.n                                            # a strict subset where that matters
    assert np.isin(b.nodes, got[0]).all()                             # T is in src


@pytest.mark.parametrize("n", BC.RING_SIZES)
def test_build_on_ring_lattices_at_every_chunk_and_scan_edge(n):
    """One below, at and one above one chunk and one scan step; 2^20 + 1 nodes with 4096 targets: 17 scan steps with a
    carry and a last chunk of one node, which is a target."""
    g, b = BC.ring(n), BC.ring_block(n)
    plan = (_lib.C.c_int * _lib.CSR_BLOCK_PLAN_INTS)()
    _lib.check(_lib.load().dp_csr_block_plan(b.m, n, 1, BC.RING_K, plan))
    assert tuple(plan) == BC.plan(b.m, n, 1, BC.RING_K)
    if n == BC.BIG_RING:
        assert plan[2] >= 2 and n % plan[0] != 0 and b.m == 4096
    ip, ix = _ring_dev(n)
    got = build(g, ip, ix, BC.ring_targets(n), BC.RING_K, BC.SEED)
    validate(got[0], got[1], got[2], n)
    _equals(got, b)
    assert got[1][n - 1] == got[2] - 1                                # the last node closes src


@pytest.mark.parametrize("gname", BC.GRAPHS)
def test_a_larger_capacity_changes_nothing_and_the_smallest_is_enough(gname):
    g, k = SC.graph(gname), 2
    t = BC.targets(gname, "seven")
    ip, ix, _, _ = dev_graph(gname)
    a = build(g, ip, ix, t, k, BC.SEED)
    b = build(g, ip, ix, t, k, BC.SEED, cap=g.n)
    assert a[5] == 21 and b[5] == g.n
    for u, v in zip(a[:5], b[:5]):
        assert np.array_equal(u, v)
    other = build(g, ip, ix, t, k, BC.SEED + 1)                        # the seed decides the block
    assert not np.array_equal(other[3], a[3]) and not np.array_equal(other[0], a[0])


# ------------------------------------------------------------------ the mean on compact rows
class Run:
    def __init__(self, case):
        self.case = case
        gname, tname, self.k, self.F, layout, self.mode = case
        self.g, self.lib = SC.graph(gname), _lib.load()
        self.t = BC.targets(gname, tname, self.k)
        self.s = BC.sample(gname, tname, self.k, self.mode)
        self.m = self.s.m
        self.wy = 2 * self.F if self.mode == "concat" else self.F
        self.x, self.dy = BC.mean_inputs(case)
        lay = ("", 0, 0, layout)
        (self.ldx, self.off), (self.ldy, _) = SC.layout_of(lay, self.F), SC.layout_of(lay, self.wy)
        self.ix = dev_graph(gname)
        self.nodes = None if self.t is None else _i32(self.t)
        self.seed64 = _seed64(BC.SEED)
        self.mode_i = SC.MODES[self.mode]
        if self.t is None:
            self.tslot = None
        else:
            ts = np.full(self.g.n, -1, dtype=np.int32)
            ts[self.t] = np.arange(self.t.size)
            self.tslot = _i32(ts)

    def sibling(self):
        """(y, thr, cnt, dx) of dp_csr_sample_mean_fwd / _bwd on the whole x."""
        g, (ip, ix, ipt, ixt) = self.g, self.ix
        bx, by = _in(self.x, self.ldx, self.off), Buf(self.m, self.wy, self.ldy, off=self.off)
        thr = torch.empty(self.m, dtype=torch.int64, device="cuda")
        cnt = torch.empty(self.m, dtype=torch.int32, device="cuda")
        _lib.check(self.lib.dp_csr_sample_mean_fwd(bx.ptr(), self.ldx, ip.data_ptr(), ix.data_ptr(), _lib.ptr(self.nodes),
                                                   by.ptr(), by.ld, thr.data_ptr(), cnt.data_ptr(), self.m, g.n, self.F,
                                                   self.k, self.mode_i, self.seed64, _stream()), "dp_csr_sample_mean_fwd")
        bg, bdx = _in(self.dy, self.ldy, self.off), Buf(g.n, self.F, self.ldx, off=self.off)
        _lib.check(self.lib.dp_csr_sample_mean_bwd(bg.ptr(), self.ldy, ipt.data_ptr(), ixt.data_ptr(), _lib.ptr(self.tslot),
                                                   thr.data_ptr(), cnt.data_ptr(), bdx.ptr(), bdx.ld, g.n, self.F,
                                                   self.mode_i, self.seed64, _stream()), "dp_csr_sample_mean_bwd")
        torch.cuda.synchronize()
        return by.back()[0], thr.cpu().numpy().view(np.uint64), cnt.cpu().numpy(), bdx.back()[0]

    def compact(self, src, slot):
        """(y, thr, cnt, dx_src) of dp_csr_block_mean_fwd / _bwd on x[src], two guarded runs."""
        g, (ip, ix, ipt, ixt) = self.g, self.ix
        n_src = int(src.size)
        src_d, slot_d = _i32(src), _i32(slot)
        bx = _in(self.x[src], self.ldx, self.off)
        bg = _in(self.dy, self.ldy, self.off)
        got = []
        for _ in range(2):
            by, bdx = Buf(self.m, self.wy, self.ldy, off=self.off), Buf(n_src, self.F, self.ldx, off=self.off)
            thr, cnt = IntBuf(self.m, torch.int64), IntBuf(self.m)
            _lib.check(self.lib.dp_csr_block_mean_fwd(bx.ptr(), self.ldx, ip.data_ptr(), ix.data_ptr(),
                                                      _lib.ptr(self.nodes), slot_d.data_ptr(), n_src, by.ptr(), by.ld,
                                                      thr.ptr(), cnt.ptr(), self.m, g.n, self.F, self.k, self.mode_i,
                                                      self.seed64, _stream()), "dp_csr_block_mean_fwd")
            _lib.check(self.lib.dp_csr_block_mean_bwd(bg.ptr(), self.ldy, ipt.data_ptr(), ixt.data_ptr(),
                                                      _lib.ptr(self.tslot), src_d.data_ptr(), n_src, thr.ptr(), cnt.ptr(),
                                                      bdx.ptr(), bdx.ld, g.n, self.F, self.mode_i, self.seed64, _stream()),
                       "dp_csr_block_mean_bwd")
            torch.cuda.synchronize()
            (y, c0), (dx, c1), (t, c2), (c, c3) = by.back(), bdx.back(), thr.back(), cnt.back()
            assert c0 and c1 and c2 and c3 and bx.back()[1] and bg.back()[1], "wrote outside its window"
            got.append((y, t.view(np.uint64).copy(), c.copy(), dx))
        for a, b in zip(*got):
            assert np.array_equal(a, b, equal_nan=True), "repeat runs differ"
        return got[0]


@pytest.mark.parametrize("case", BC.MEAN_CASES, ids=BC.mean_id)
def test_the_compact_mean_has_the_bits_of_the_whole_graph_mean(case):
    r = Run(case)
    g, s, tag = r.g, r.s, BC.mean_id(case)
    ip, ix, _, _ = r.ix
    src, slot, n_src, thr_b, cnt_b, _ = build(g, ip, ix, r.t, r.k, BC.SEED)
    validate(src, slot, n_src, g.n)                                   # on the host, before a kernel reads through them
    _equals((src, slot, n_src, thr_b, cnt_b, 0), BC.block(case[0], case[1], r.k))
    y, thr, cnt, dx_src = r.compact(src, slot)
    assert np.array_equal(thr, s.thr) and np.array_equal(cnt, s.cnt)  # cnt by the self mode's rule
    want_y, want_thr, want_cnt, want_dx = r.sibling()
    assert np.array_equal(thr, want_thr) and np.array_equal(cnt, want_cnt)
    assert np.isfinite(y).all() and np.isfinite(dx_src).all(), "entries not written"
    assert np.array_equal(y, want_y), f"y differs from the whole-graph mean in {int((y != want_y).sum())} entries"
    assert np.array_equal(dx_src, want_dx[src]), "dx_src differs from the rows src of the whole-graph dx"
    rest = np.ones(g.n, bool)
    rest[src] = False
    assert not want_dx[rest].any()                                    # exactly zero outside src
    _check("dp_csr_block_mean_fwd " + tag, y, *SC.fwd_ref(s, r.x))
    dref, dbound = SC.bwd_ref(s, r.dy)
    _check("dp_csr_block_mean_bwd " + tag, dx_src, dref[src], dbound[src])
    assert not dref[rest].any()


def test_the_forward_on_the_big_ring_has_the_bits_of_the_whole_graph_mean():
    n = BC.BIG_RING
    g, b, t = BC.ring(n), BC.ring_block(n), BC.ring_targets(n)
    ip, ix = _ring_dev(n)
    lib = _lib.load()
    rng = np.random.default_rng(SC._seed("block-big-ring"))
    x = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    src, slot, nodes = _i32(b.src), _i32(b.slot), _i32(t)
    x_src = x[src.long()].contiguous()
    outs = []
    for compact in (False, True):
        y = torch.full((b.m, 6), float("nan"), device="cuda")
        thr = torch.empty(b.m, dtype=torch.int64, device="cuda")
        cnt = torch.empty(b.m, dtype=torch.int32, device="cuda")
        if compact:
            _lib.check(lib.dp_csr_block_mean_fwd(x_src.data_ptr(), 3, ip.data_ptr(), ix.data_ptr(), nodes.data_ptr(),
                                                 slot.data_ptr(), b.n_src, y.data_ptr(), 6, thr.data_ptr(), cnt.data_ptr(),
                                                 b.m, n, 3, BC.RING_K, 2, _seed64(BC.SEED), _stream()))
        else:
            _lib.check(lib.dp_csr_sample_mean_fwd(x.data_ptr(), 3, ip.data_ptr(), ix.data_ptr(), nodes.data_ptr(),
                                                  y.data_ptr(), 6, thr.data_ptr(), cnt.data_ptr(), b.m, n, 3, BC.RING_K, 2,
                                                  _seed64(BC.SEED), _stream()))
        torch.cuda.synchronize()
        outs.append((y.cpu().numpy(), thr.cpu().numpy().view(np.uint64), cnt.cpu().numpy()))
    for u, v in zip(*outs):
        assert np.array_equal(u, v)
    assert np.array_equal(outs[1][1], b.thr) and (outs[1][2] == BC.RING_K).all()


# ------------------------------------------------------------------ nothing to do, and refusals
def test_the_empty_target_set_launches_nothing_and_k_65_is_refused():
    lib = _lib.load()
    g = SC.graph("batch")
    ip, ix, ipt, ixt = dev_graph("batch")
    wsb = lib.dp_csr_block_workspace_bytes(g.n)
    slot, src, cnt, count, thr, ws = IntBuf(g.n), IntBuf(g.n), IntBuf(4), IntBuf(1), IntBuf(4, torch.int64), IntBuf(wsb // 4)
    by, bdx = Buf(4, 5), Buf(4, 5)
    nodes = _i32(np.arange(4))

    def call_build(m, n, k):
        return lib.dp_csr_block_build(ip.data_ptr(), ix.data_ptr(), nodes.data_ptr(), m, n, k, 5, slot.ptr(), src.ptr(), g.n,
                                      count.ptr(), thr.ptr(), cnt.ptr(), ws.ptr(), wsb, _stream())

    def call_fwd(m, n, F, k):
        return lib.dp_csr_block_mean_fwd(by.ptr(), 5, ip.data_ptr(), ix.data_ptr(), nodes.data_ptr(), slot.ptr(), 0,
                                         by.ptr(), 5, thr.ptr(), cnt.ptr(), m, n, F, k, 0, 5, _stream())

    def call_bwd(n_src, n, F):
        return lib.dp_csr_block_mean_bwd(by.ptr(), 5, ipt.data_ptr(), ixt.data_ptr(), slot.ptr(), src.ptr(), n_src,
                                         thr.ptr(), cnt.ptr(), bdx.ptr(), 5, n, F, 0, 5, _stream())

    assert call_build(0, g.n, 10) == 0 and call_build(0, 0, 10) == 0
    assert call_fwd(0, g.n, 5, 10) == 0 and call_fwd(4, g.n, 0, 10) == 0 and call_fwd(0, 0, 5, 10) == 0
    assert call_bwd(0, g.n, 5) == 0 and call_bwd(4, g.n, 0) == 0
    assert call_build(4, g.n, 65) == -1 and "k=65 must be 1 .. 64" in lib.dp_last_error_string().decode()
    assert call_fwd(4, g.n, 5, 65) == -1 and "k=65 must be 1 .. 64" in lib.dp_last_error_string().decode()
    torch.cuda.synchronize()
    for b in (slot, src, cnt, count, thr, ws):
        got, clean = b.back()
        assert clean and (got == FF).all()
    for b in (by, bdx):
        got, clean = b.back()
        assert clean and np.isnan(got).all()
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrGraph
    c = CsrGraph.from_edges(g.n, g.rows, g.indices, "cuda", symmetric=False)
    with pytest.raises(ValueError, match="num_sample must be 1 .. 64 or None"):
        ops.csr_sample_block(c, nodes, 65, 1)
    e = ops.csr_sample_block(c, torch.zeros(0, dtype=torch.int32, device="cuda"), 10, 1)
    assert e.n_src == 0 and e.src.numel() == 0 and (e.slot == -1).all() and e.slot.numel() == g.n
    assert ops.csr_block_mean(torch.zeros(0, 3, device="cuda"), e, "concat").shape == (0, 6)
