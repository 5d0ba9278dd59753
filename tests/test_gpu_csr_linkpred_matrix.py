"""The CSR link-prediction loss (dp_csr_linkpred_loss_*, dp_csr_linkpred_batch_loss_* and their _w twins) on every row
of tests/csr_linkpred_cases.py through the C ABI, against the float64 reference under the counted bound of
tests/csr_weights_cases.py: every K tier edge of the dense kernels, the forward's one- and two-tile walks, every
backward class (one tile, one tile per split, two per split even and ragged) at both tile widths and both accumulate
values, all six edge forms with a full and a partial last chunk, the three reasons a K % 4 == 0 takes the 4-byte form,
directed / undirected / weighted graphs with planted row lengths, ties and all three gates of min(., 1), dloss, and the
batch entries.

Per row: S, dS and the loss sit in guarded buffers (Buf of tests/test_gpu_csr_weights.py) and nothing outside an output
window may change; the workspace has exactly the queried size, is filled with 0xFF bytes (an unwritten partial read
back is a NaN) and has a guard band behind it; dS is NaN-filled when it is to be overwritten; a second run must give
the same bits; weights of 1.0 must give the plain entry's bits; and the plan that ran is asserted from
dp_csr_linkpred_plan on the very pointers the entries were given.

Every figure is printed ("[csr linkpred] ...") before it is asserted.  With DP_CSR_LINKPRED_ANCHOR=<file> the largest
|error| / bound per row is written there (profiles/csr_linkpred_fp64_anchor.txt is such a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_linkpred_cases as CC
from tests.test_gpu_csr_weights import GUARD, Buf

pytestmark = pytest.mark.gpu

WS_GUARD = 256                  # bytes behind the workspace
RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_CSR_LINKPRED_ANCHOR")
    if path and RESULTS:
        with open(path, "w") as f:
            f.write(CC.anchor_text(RESULTS))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Window:
    """[rows, K] at leading dimension ld, `shift` floats off the 16-byte boundary a Buf window starts on: the Buf holds
    `shift` guard columns in front of the K columns."""

    def __init__(self, rows, K, ld, shift, data):
        assert K + shift <= ld
        full = np.full((rows, K + shift), GUARD, dtype=np.float32)
        full[:, shift:] = data
        self.K, self.shift, self.full = K, shift, full
        self.buf = Buf(rows, K + shift, ld, data=full)

    def ptr(self):
        p = self.buf.ptr() + 4 * self.shift
        assert (p % 16 != 0) == (self.shift % 4 != 0) and p % 4 == 0
        return p

    def back(self):
        """(the [rows, K] values as float32 numpy, True when nothing outside them changed)."""
        got, clean = self.buf.back()
        got = got.astype(np.float32)
        lead_same = got[:, :self.shift].tobytes() == self.full[:, :self.shift].tobytes()
        return got[:, self.shift:].copy(), bool(clean and lead_same)


class Problem:
    """One row on the device.  run(weights) -> (loss float32 scalar, dS [n_total, K] float32); weights: None (the plain
    entries), "stored" or "ones" (the _w entries)."""

    def __init__(self, c, inp, old):
        self.lib = lib = _lib.load()
        self.c, self.inp, self.old = c, inp, old
        self.lds, self.ldds = CC.strides(c)
        self.rows = int(inp["off"][-1])
        self.S = Window(self.rows, c.K, self.lds, c.s_shift, inp["S"])
        self.indptr, self.indices, self.values = _dev(inp["indptr"]), _dev(inp["indices"]), _dev(inp["values"])
        if c.directed:
            self.indptr_t, self.indices_t, self.values_t = (_dev(inp["indptr_t"]), _dev(inp["indices_t"]),
                                                            _dev(inp["values_t"]))
        else:                                      # the same arrays twice: one gather and a factor 2
            self.indptr_t, self.indices_t, self.values_t = self.indptr, self.indices, self.values
        self.ones, self.ones_t = torch.ones_like(self.values), torch.ones_like(self.values_t)
        self.dl = None if c.dloss is None else torch.tensor([c.dloss], dtype=torch.float32).cuda()
        self.off = np.ascontiguousarray(inp["off"], dtype=np.int32)
        if c.batch:
            self.wsb = lib.dp_csr_linkpred_batch_workspace_bytes(self.off.ctypes.data, len(c.sizes), c.K)
        else:
            self.wsb = lib.dp_csr_linkpred_workspace_bytes(c.sizes[0], c.K)
        assert self.wsb > 0

    def plans(self):
        """dp_csr_linkpred_plan of every graph on the pointers of this problem's S and of a dS built like run()'s."""
        dS = Window(self.rows, self.c.K, self.ldds, self.c.ds_shift, 0.0)
        out = []
        for b, n in enumerate(self.c.sizes):
            ps = self.S.ptr() + 4 * int(self.off[b]) * self.lds
            pd = dS.ptr() + 4 * int(self.off[b]) * self.ldds
            buf = (C.c_int * _lib.CSR_LINKPRED_PLAN_INTS)()
            _lib.check(self.lib.dp_csr_linkpred_plan(n, self.c.K, self.lds, self.ldds, int(ps % 16 != 0), int(pd % 16 != 0),
                                                     buf), "dp_csr_linkpred_plan")
            out.append(CC.Plan(*buf))
        return out

    def run(self, weights=None):
        lib, c = self.lib, self.c
        K, B = c.K, len(c.sizes)
        ws = torch.full((self.wsb + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
        dS = Window(self.rows, K, self.ldds, c.ds_shift, self.old if c.acc else np.float32("nan"))
        loss = Buf(1, 1, fill=float("nan"))
        st = _lib.current_stream()
        w = "" if weights is None else "_w"
        val = () if weights is None else ((self.values if weights == "stored" else self.ones).data_ptr(),)
        valt = () if weights is None else ((self.values_t if weights == "stored" else self.ones_t).data_ptr(),)
        head = (self.S.ptr(), self.lds, self.indptr.data_ptr(), self.indices.data_ptr())
        tr = (self.indptr_t.data_ptr(), self.indices_t.data_ptr())
        if c.batch:
            off = self.off.ctypes.data
            fwd, bwd = "dp_csr_linkpred_batch_loss_fwd" + w, "dp_csr_linkpred_batch_loss_bwd" + w
            _lib.check(getattr(lib, fwd)(*head, *val, off, B, loss.ptr(), K, ws.data_ptr(), self.wsb, st), fwd)
            _lib.check(getattr(lib, bwd)(*head, *val, *tr, *valt, off, B, _lib.ptr(self.dl), dS.ptr(), self.ldds, c.acc, K,
                                         ws.data_ptr(), self.wsb, st), bwd)
        else:
            n = c.sizes[0]
            fwd, bwd = "dp_csr_linkpred_loss_fwd" + w, "dp_csr_linkpred_loss_bwd" + w
            _lib.check(getattr(lib, fwd)(*head, *val, loss.ptr(), n, K, ws.data_ptr(), self.wsb, st), fwd)
            _lib.check(getattr(lib, bwd)(*head, *val, *tr, *valt, _lib.ptr(self.dl), dS.ptr(), self.ldds, c.acc, n, K,
                                         ws.data_ptr(), self.wsb, st), bwd)
        torch.cuda.synchronize()
        assert bool((ws[self.wsb:] == 0xFF).all()), "the guard band behind the workspace was written"
        lv, lclean = loss.back()
        dv, dclean = dS.back()
        _, sclean = self.S.back()
        assert lclean and dclean and sclean, f"{c.name}: something outside the loss / dS windows changed"
        return lv.astype(np.float32).reshape(()), dv


@pytest.mark.parametrize("name", [c.name for c in CC.CASES])
def test_row_against_fp64_under_the_counted_bound(name):
    c, inp, ref = CC.case_data(name)
    assert CC.qualifies(c, ref)
    old = CC.prior(c, ref) if c.acc else None
    loss32, d32 = CC.formula32(c, inp)
    rf = CC.compare(c, ref, loss32, CC.output(d32, old), old)
    p = Problem(c, inp, old)
    got_plans = p.plans()
    assert got_plans == CC.graph_plans(c), (name, got_plans)        # the path that runs is the one the row is there for
    main = got_plans[int(np.argmax(c.sizes))]
    loss, dS = p.run("stored" if c.weighted else None)
    r = CC.compare(c, ref, loss, dS, old)
    print(f"[csr linkpred] {name} {CC.bwd_class(main)} {CC.plan_text(main)}: loss {float(loss):.9g} vs {ref['loss']:.9g}, "
          f"{r['fwd']:.4f} of its bound; dS {r['bwd']:.4f} of its bound (fp32 formula: {rf['fwd']:.4f}, {rf['bwd']:.4f})")
    RESULTS[name] = (CC.bwd_class(main), CC.plan_text(main), c.acc, r["fwd"], r["bwd"], rf["fwd"], rf["bwd"])
    failures = list(r["problems"])
    loss2, dS2 = p.run("stored" if c.weighted else None)
    if loss2.tobytes() != loss.tobytes() or dS2.tobytes() != dS.tobytes():
        failures.append("a second run gives other bits")
    plain = (loss, dS) if not c.weighted else p.run(None)
    one = p.run("ones")
    if one[0].tobytes() != plain[0].tobytes() or one[1].tobytes() != plain[1].tobytes():
        failures.append("weights of 1.0 do not give the plain entry's bits")
    assert not failures, failures


def test_k_257_is_refused_by_every_entry_before_any_launch():
    lib = _lib.load()
    n, K = 64, CC.REFUSED_K
    S = torch.full((n, K), 0.5, device="cuda")
    dS = torch.full((n, K), GUARD, device="cuda")
    loss = torch.full((1,), GUARD, device="cuda")
    ip = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    ix = torch.arange(n, dtype=torch.int32, device="cuda")
    val = torch.ones(n, device="cuda")
    off = np.array([0, n], dtype=np.int32)
    wsb = lib.dp_csr_linkpred_workspace_bytes(n, CC.K_MAX)
    assert lib.dp_csr_linkpred_workspace_bytes(n, K) == 0
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    st = _lib.current_stream()
    a = (S.data_ptr(), K, ip.data_ptr(), ix.data_ptr())
    t = (ip.data_ptr(), ix.data_ptr())
    v = (val.data_ptr(),)
    w = (ws.data_ptr(), wsb, st)
    o = off.ctypes.data
    rcs = [lib.dp_csr_linkpred_loss_fwd(*a, loss.data_ptr(), n, K, *w),
           lib.dp_csr_linkpred_loss_fwd_w(*a, *v, loss.data_ptr(), n, K, *w),
           lib.dp_csr_linkpred_loss_bwd(*a, *t, None, dS.data_ptr(), K, 0, n, K, *w),
           lib.dp_csr_linkpred_loss_bwd_w(*a, *v, *t, *v, None, dS.data_ptr(), K, 0, n, K, *w),
           lib.dp_csr_linkpred_batch_loss_fwd(*a, o, 1, loss.data_ptr(), K, *w),
           lib.dp_csr_linkpred_batch_loss_fwd_w(*a, *v, o, 1, loss.data_ptr(), K, *w),
           lib.dp_csr_linkpred_batch_loss_bwd(*a, *t, o, 1, None, dS.data_ptr(), K, 0, K, *w),
           lib.dp_csr_linkpred_batch_loss_bwd_w(*a, *v, *t, *v, o, 1, None, dS.data_ptr(), K, 0, K, *w)]
    assert rcs == [-3] * 8, rcs
    assert b"K=257" in lib.dp_last_error_string()
    torch.cuda.synchronize()
    assert bool((dS == GUARD).all()) and float(loss) == GUARD and bool((ws == 0xFF).all())
