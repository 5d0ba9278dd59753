"""Top-k pooling through the C ABI (dp_csr_topk_select / _induce / _gather_fwd / _gather_bwd): every row of
tests/csr_topk_cases.py.  thr, perm, new_id, indptr', indices', indices_local', edge_map and the transposed set equal the
numpy restatement EXACTLY; x_out and dx equal the fp32 product bit for bit; dgate lies within the bound counted from the
kernel's summation order.  Every float input lies at the case's leading dimension and base with NaN in its padding,
every output is NaN- or 0xFF-filled inside guard bands that must stay untouched, the workspace has exactly the queried
size with a guard behind it, and every case runs twice, bit for bit.  Where every node is kept (ratio = 1, k above n_b)
the input graph's arrays come back value for value.

With DP_CSR_TOPK_ANCHOR=<file> the largest |error| / bound of dgate per case is written there
(profiles/csr_topk_fp64_anchor.txt is such a run of this file alone)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_topk_cases as TC
from tests.test_gpu_csr_edge_grad import Buf, _stream

pytestmark = pytest.mark.gpu

RATIOS = {}
G = 4                                                                # guard elements on either side of an integer window


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_TOPK_ANCHOR")
    if path and RATIOS:
        lines = ["dgate: largest |error| / bound (bound: tests/csr_topk_cases.py, (ceil(F / 64) + 6) roundings, u = 2^-24)",
                 "", f"{'all cases':<72s} {max(RATIOS.values()):8.4f}", "", "per case"]
        lines += [f"{k:<72s} {RATIOS[k]:8.4f}" for k in sorted(RATIOS)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


class IBuf:
    """An integer window of m elements inside a guarded device allocation, every byte 0xFF (-1) unless told otherwise."""

    def __init__(self, m, dtype=torch.int32, fill=-1):
        self.m, self.fill = m, fill
        self.t = torch.full((m + 2 * G,), fill, dtype=dtype, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + G * self.t.element_size()

    def back(self):
        h = self.t.cpu().numpy()
        assert (h[:G] == self.fill).all() and (h[G + self.m:] == self.fill).all(), "wrote outside its window"
        return h[G:G + self.m]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


_DEV = {}


def dev_graph(name):
    """(indptr, indices, indptr_t, indices_t, node_off) of a case graph on the device, int32, made once."""
    if name not in _DEV:
        g = TC.graph(name)
        ip, ix = _i32(g.indptr), _i32(g.indices if g.nnz else np.zeros(1))
        t = (_i32(g.indptr_t), _i32(g.indices_t if g.nnz else np.zeros(1))) if g.directed else (ip, ix)
        _DEV[name] = (ip, ix) + t + (_i32(g.off),)
    return _DEV[name]


def _in(x, ld, off):
    full = np.vstack([_padded(x, ld), np.full((1, ld), np.nan, np.float32)])
    return Buf(x.shape[0] + 1, ld, ld, full, off=off)


def _padded(x, ld):
    out = np.full((x.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def check_structure(indptr, indices, local, new_off, nnz):
    """The container invariants of a pooled CSR read back to the host."""
    n_out = indptr.size - 1
    assert indptr[0] == 0 and indptr[-1] == nnz and (np.diff(indptr) >= 0).all()
    rows = np.repeat(np.arange(n_out), np.diff(indptr))
    gb = np.searchsorted(new_off, rows, side="right") - 1
    ix = indices[:nnz]
    assert (ix >= new_off[gb]).all() and (ix < new_off[gb + 1]).all(), "a column outside its graph's new range"
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(ix)[same_row] > 0).all(), "columns not ascending and unique within a row"
    if local is not None:
        assert np.array_equal(local[:nnz], ix - new_off[gb])


def _select(lib, case, p, sc_dev, node_off, new_off):
    g = p.g
    node_off_host = np.ascontiguousarray(g.off, dtype=np.int32)
    kb_host = np.ascontiguousarray(p.kb, dtype=np.int32)
    got = []
    for _ in range(2):
        new_id, perm, thr = IBuf(g.n, fill=0x5A5A5A5A), IBuf(p.n_out), IBuf(g.B, torch.int64)      # -1 is a value of new_id
        _lib.check(lib.dp_csr_topk_select(sc_dev.data_ptr(), node_off.data_ptr(), new_off.data_ptr(),
                                          node_off_host.ctypes.data, kb_host.ctypes.data, new_id.ptr(), perm.ptr(),
                                          thr.ptr(), g.n, p.n_out, g.B, _stream()), "dp_csr_topk_select")
        torch.cuda.synchronize()
        got.append((new_id.back().copy(), perm.back().copy(), thr.back().view(np.uint64).copy(), new_id, perm))
    for a, b in zip(got[0][:3], got[1][:3]):
        assert np.array_equal(a, b), "repeat runs differ"
    return got[0]


def _induce(lib, p, ip, ix, nnz_in, new_id, perm, new_off, with_local):
    g = p.g
    cap = max(nnz_in, 1)
    wsb = lib.dp_csr_topk_workspace_bytes(p.n_out)
    got = []
    for _ in range(2):
        ws = torch.full((wsb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
        ipo, ixo, emo = IBuf(p.n_out + 1), IBuf(cap), IBuf(cap)
        ilo = IBuf(cap) if with_local else None
        _lib.check(lib.dp_csr_topk_induce(ip.data_ptr(), ix.data_ptr(), new_id.ptr(), perm.ptr(), new_off.data_ptr(),
                                          ipo.ptr(), ixo.ptr(), ilo.ptr() if ilo else None, emo.ptr(), g.n, p.n_out, g.B,
                                          nnz_in, cap, ws.data_ptr(), wsb, _stream()), "dp_csr_topk_induce")
        torch.cuda.synchronize()
        assert (ws[wsb:].cpu().numpy() == 0xA5).all(), "wrote past the queried workspace size"
        got.append((ipo.back().copy(), ixo.back().copy(), ilo.back().copy() if ilo else None, emo.back().copy()))
    for a, b in zip(got[0], got[1]):
        assert (a is None and b is None) or np.array_equal(a, b), "repeat runs differ"
    return got[0]


def _check_induced(what, got, p, indptr, indices, local, edge_map, with_local):
    ipo, ixo, ilo, emo = got
    nnz = int(indptr[-1])
    assert np.array_equal(ipo, indptr), f"{what}: indptr'"
    check_structure(ipo, ixo, ilo, p.new_off, nnz)
    assert np.array_equal(ixo[:nnz], indices), f"{what}: indices'"
    assert np.array_equal(emo[:nnz], edge_map), f"{what}: edge_map"
    if with_local:
        assert np.array_equal(ilo[:nnz], local), f"{what}: indices_local'"
    pad = 1 if nnz == 0 else 0                                       # a graph without kept entries gets the zero pad
    for a in (ixo, emo) + ((ilo,) if with_local else ()):
        assert (a[nnz + pad:] == -1).all(), f"{what}: wrote past nnz'"
        assert not pad or a[0] == 0, f"{what}: the one-element pad"


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_case_against_the_restatement(case):
    gname, kind, sel, F, layout, gated = case
    lib = _lib.load()
    g, p = TC.graph(gname), TC.pooled(gname, kind, sel)
    ip, ix, ipt, ixt, node_off = dev_graph(gname)
    new_off = _i32(p.new_off)
    plan = (_lib.C.c_int * _lib.CSR_TOPK_PLAN_INTS)()
    for nb, kb in zip(g.sizes, p.kb):
        _lib.check(lib.dp_csr_topk_plan(g.n, p.n_out, g.B, int(g.sizes.max()), int(nb), int(kb), F, plan))
        assert tuple(plan) == TC.plan(g.n, p.n_out, g.B, int(g.sizes.max()), int(nb), int(kb), F)
    sc = torch.from_numpy(TC.scores(gname, kind)).cuda()
    new_id, perm, thr, new_id_d, perm_d = _select(lib, case, p, sc, node_off, new_off)
    assert np.array_equal(thr, p.thr), "thr"
    assert np.array_equal(perm, p.perm), "perm"
    assert np.array_equal(new_id, p.new_id), "new_id"
    # only now, with perm and new_id checked, the launches that read through them
    with_local = gname in TC.BATCHES
    got = _induce(lib, p, ip, ix, g.nnz, new_id_d, perm_d, new_off, with_local)
    _check_induced("forward CSR", got, p, p.indptr, p.indices, p.local, p.edge_map, with_local)
    if g.directed:
        got_t = _induce(lib, p, ipt, ixt, g.nnz, new_id_d, perm_d, new_off, with_local)
        _check_induced("transposed CSR", got_t, p, p.indptr_t, p.indices_t, p.local_t, p.edge_map_t, with_local)
    if (p.kb == g.sizes).all():                                      # everything kept: the input graph, value for value
        assert np.array_equal(got[0], g.indptr) and np.array_equal(got[1][:g.nnz], g.indices)
        assert np.array_equal(got[3][:g.nnz], np.arange(g.nnz)) and np.array_equal(perm, np.arange(g.n))
    # gather * gate and its backward
    x, gate, dy = TC.inputs(case)
    ldf, off = TC.LAYOUTS[layout]
    ld = ldf(F)
    bx, bdy = _in(x, ld, off), _in(dy, ld, off)
    gate_d = None if gate is None else torch.from_numpy(gate).cuda()
    ref, mag = TC.dgate64(dy, x, p)
    bound = TC.dgate_bound(F, mag)
    for rep in range(2):
        by = Buf(p.n_out, F, ld, off=off)
        _lib.check(lib.dp_csr_topk_gather_fwd(bx.ptr(), ld, _lib.ptr(gate_d), perm_d.ptr(), by.ptr(), ld, g.n, p.n_out, F,
                                              _stream()), "dp_csr_topk_gather_fwd")
        bdx = Buf(g.n, F, ld, off=off)
        dgate = torch.full((g.n + 2,), float("nan"), device="cuda") if gated else None
        _lib.check(lib.dp_csr_topk_gather_bwd(bdy.ptr(), ld, bx.ptr() if gated else None, ld, _lib.ptr(gate_d),
                                              new_id_d.ptr(), bdx.ptr(), ld, dgate.data_ptr() + 4 if gated else None, g.n,
                                              p.n_out, F, _stream()), "dp_csr_topk_gather_bwd")
        torch.cuda.synchronize()
        y, clean_y = by.back()
        dx, clean_dx = bdx.back()
        assert clean_y and clean_dx and bx.back()[1] and bdy.back()[1], "wrote outside its window"
        assert np.array_equal(y.view(np.uint32), TC.forward32(x, gate, p.perm).view(np.uint32)), "x_out"
        assert np.array_equal(dx.view(np.uint32), TC.backward32(dy, gate, p).view(np.uint32)), "dx"
        if gated:
            dg = dgate.cpu().numpy()
            assert np.isnan(dg[0]) and np.isnan(dg[-1]) and np.isfinite(dg[1:-1]).all()
            ratio = TC.moved(ref, dg[1:-1], bound)
            print(f"dgate {TC.case_id(case)}: |error| / bound = {ratio:.4f}")
            RATIOS[TC.case_id(case)] = max(RATIOS.get(TC.case_id(case), 0.0), ratio)
            assert ratio <= 1.0, f"dgate: |error| / bound = {ratio:.3f}"
            if rep:
                assert np.array_equal(dg[1:-1], first), "repeat runs differ"
            first = dg[1:-1]


def test_one_graph_of_two_to_the_twenty_nodes():
    """The one-workgroup select at 2^20 nodes (1024 keys per thread recomputed over 7 passes, a 1024-chunk prefix count)
    and the induce launches with 16 384 row blocks: sixteen chunks of the scan."""
    lib = _lib.load()
    n = 1 << 20
    g = TC.ring(n)
    rng = np.random.default_rng(5)
    s = (rng.integers(0, 8, n) / 4).astype(np.float32)               # eight levels: ties decide at the cut
    p = TC.Pooled(g, s, TC.counts(g.sizes, ratio=0.5))
    assert TC.plan(n, p.n_out, 1, n, n, p.n_out, 1)[:5] == (1024, 2, 1024, 7, 1024)
    assert TC.plan(n, p.n_out, 1, n, n, p.n_out, 1)[6:8] == (16384, 16)
    ip, ix, node_off, new_off = _i32(g.indptr), _i32(g.indices), _i32(g.off), _i32(p.new_off)
    new_id, perm, thr, new_id_d, perm_d = _select(lib, None, p, torch.from_numpy(s).cuda(), node_off, new_off)
    assert np.array_equal(thr, p.thr) and np.array_equal(perm, p.perm) and np.array_equal(new_id, p.new_id)
    got = _induce(lib, p, ip, ix, g.nnz, new_id_d, perm_d, new_off, False)
    _check_induced("2^20 nodes", got, p, p.indptr, p.indices, p.local, p.edge_map, False)


def test_calls_with_nothing_to_do_launch_nothing():
    lib = _lib.load()
    t = torch.full((8,), float("nan"), device="cuda")
    i = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    assert lib.dp_csr_topk_gather_fwd(t.data_ptr(), 0, None, i.data_ptr(), t.data_ptr(), 0, 4, 2, 0, _stream()) == 0
    assert lib.dp_csr_topk_gather_fwd(t.data_ptr(), 2, None, i.data_ptr(), t.data_ptr(), 2, 4, 0, 2, _stream()) == 0
    assert lib.dp_csr_topk_gather_bwd(t.data_ptr(), 0, None, 0, None, i.data_ptr(), t.data_ptr(), 0, None, 4, 2, 0,
                                      _stream()) == 0
    assert lib.dp_csr_topk_select(t.data_ptr(), i.data_ptr(), i.data_ptr(), i.data_ptr(), i.data_ptr(), i.data_ptr(),
                                  i.data_ptr(), t.data_ptr(), 0, 0, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(t).all() and (i == -1).all()
