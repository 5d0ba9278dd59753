"""The dense / packed link-prediction loss (dp_linkpred_loss_* and the link term of dp_loss_forward / dp_loss_backward
and their _packed twins) on every row of tests/linkpred_cases.py, against the float64 reference under the counted
bounds of that file: every K tier edge, the tile edges of n, every backward plan (one column tile, non-split with
several tiles at both widths, one tile per split, several per split, a ragged last split, splits and row blocks wholly
beyond n_b), masks, directed / weighted / padded adjacencies, ties and all three gates of min(., 1), dloss, accumulate
and link_norm.

Per row and reader: the workspace is sized exactly by the library's query and filled with 0xFF bytes (an unwritten
partial read back is a NaN), dS is pre-filled with NaN when it is to be overwritten, guard bands sit behind the
workspace, dS and the loss; rows >= n_b of dS must be exactly 0 (or the prior content under accumulate); a second run
must give the same bits; on a bf16-exact adjacency the packed reader must give the fp32 reader's bits; and the plan
that ran is asserted from dp_linkpred_plan.  Inputs with sharp assignments are held to the anchored criterion.

Every figure is printed ("[linkpred] ...") before it is asserted.  DP_LINKPRED_ANCHOR_OUT=<file> appends one line per
case and reader (profiles/linkpred_fp64_anchor.txt is the digest of such a file, made by
`python -m tests.linkpred_cases --digest <file> profiles/linkpred_fp64_anchor.txt`)."""
import ctypes as C

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import linkpred_cases as LC

pytestmark = pytest.mark.gpu

GUARD = -7.25
TAIL = 64                       # floats behind dS
WS_GUARD = 256                  # bytes behind the workspace
NCLASS = 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib_plan(lib, B, n, K):
    out = (C.c_int * _lib.LINKPRED_PLAN_INTS)()
    _lib.check(lib.dp_linkpred_plan(B, n, K, out), "dp_linkpred_plan")
    return tuple(out)


class Problem:
    """One case on the device for one reader; run() -> (loss float32 scalar, dS [B, n, K] float32 numpy)."""

    def __init__(self, c, inp, reader, old):
        self.lib = lib = _lib.load()
        self.c, self.reader, self.old = c, reader, old
        B, n, K = c.B, c.n, c.K
        self.S = _dev(inp["S"])
        self.nn = None if inp["nn"] is None else _dev(inp["nn"])
        if reader == "packed":
            ld = lib.dp_adj_pack_ld(n)
            assert ld % 8 == 0 and n <= ld < n + 8
            pk, pkt = LC.pack(inp["A"], ld, c.padnan)
            self.pk = _dev(pk.view(np.int16))
            # symmetric: one buffer given as both A and A^T
            self.pkt = self.pk if np.array_equal(pk, pkt) else _dev(pkt.view(np.int16))
            assert (self.pkt is self.pk) == (c.adj not in ("dir", "outside7"))
        else:
            self.A = _dev(inp["A"])
        self.dl = None if inp["dloss"] is None else torch.tensor([inp["dloss"]], dtype=torch.float32).cuda()
        self.norm = None if inp["norm"] is None else torch.tensor([inp["norm"]], dtype=torch.float32).cuda()
        self.wsb = (lib.dp_loss_workspace_bytes(B, n, K, 1) if c.via == "loss" else
                    lib.dp_linkpred_workspace_bytes(B, n, K))
        if c.via == "loss":
            g = torch.Generator().manual_seed(B * 1000 + K)
            self.ypred = (torch.randn(B, NCLASS, generator=g) * 2).cuda()
            self.label = torch.randint(0, NCLASS, (B,), generator=g).cuda()

    def _adj_args(self, bwd):
        if self.reader == "packed":
            return (self.pk.data_ptr(), self.pkt.data_ptr()) if (bwd or self.c.via == "loss") else (self.pk.data_ptr(),)
        return (self.A.data_ptr(),)

    def run(self):
        lib, c = self.lib, self.c
        B, n, K = c.B, c.n, c.K
        ws = torch.full((self.wsb + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        total = B * n * K
        if c.acc:
            dS = _dev(np.concatenate([self.old.reshape(-1), np.full(TAIL, GUARD, np.float32)]))
        else:
            dS = torch.full((total + TAIL,), float("nan"), device="cuda")
            dS[total:] = GUARD
        loss = torch.tensor([GUARD, float("nan"), float("nan"), GUARD], dtype=torch.float32).cuda()
        st = _lib.current_stream()
        sfx = "_packed" if self.reader == "packed" else ""
        extra = {}
        if c.via == "link":
            assert self.norm is None
            _lib.check(getattr(lib, "dp_linkpred_loss_fwd" + sfx)(
                self.S.data_ptr(), *self._adj_args(False), _lib.ptr(self.nn), loss.data_ptr() + 4, B, n, K,
                ws.data_ptr(), self.wsb, st), "dp_linkpred_loss_fwd" + sfx)
            _lib.check(getattr(lib, "dp_linkpred_loss_bwd" + sfx)(
                self.S.data_ptr(), *self._adj_args(True), _lib.ptr(self.nn), _lib.ptr(self.dl), dS.data_ptr(), c.acc,
                B, n, K, ws.data_ptr(), self.wsb, st), "dp_linkpred_loss_bwd" + sfx)
            h = loss.cpu()
            assert h[0] == GUARD and h[3] == GUARD and torch.isnan(h[2]), h
            out_loss = h[1].numpy().copy()
        else:
            prob = torch.full((B * NCLASS + 8,), GUARD, device="cuda")
            dy = torch.full((B * NCLASS + 8,), GUARD, device="cuda")
            _lib.check(getattr(lib, "dp_loss_forward" + sfx)(
                self.ypred.data_ptr(), self.label.data_ptr(), self.S.data_ptr(), *self._adj_args(False),
                _lib.ptr(self.nn), _lib.ptr(self.norm), loss.data_ptr() + 4, prob.data_ptr(), None, B, NCLASS, n, K, 1,
                ws.data_ptr(), self.wsb, st), "dp_loss_forward" + sfx)
            _lib.check(getattr(lib, "dp_loss_backward" + sfx)(
                prob.data_ptr(), self.label.data_ptr(), self.S.data_ptr(), *self._adj_args(True), _lib.ptr(self.nn),
                _lib.ptr(self.norm), _lib.ptr(self.dl), dy.data_ptr(), dS.data_ptr(), B, NCLASS, n, K, 1,
                ws.data_ptr(), self.wsb, st), "dp_loss_backward" + sfx)
            h = loss.cpu()
            assert h[0] == GUARD and h[3] == GUARD, h
            out_loss = h[2].numpy().copy()                           # loss_out[1]: the link term
            extra = dict(total=h[1].numpy().copy(), prob=prob, dy=dy.cpu())
            assert (prob[B * NCLASS:] == GUARD).all() and (dy[B * NCLASS:] == GUARD).all()
        torch.cuda.synchronize()
        assert (ws[self.wsb:] == 0xFF).all(), "the guard band behind the workspace was written"
        hd = dS.cpu()
        assert (hd[total:] == GUARD).all(), "the guard band behind dS was written"
        return out_loss, hd[:total].numpy().reshape(B, n, K).copy(), extra

    def check_loss_entries(self, link, extra):
        """loss_out[0] = CE + link (fp32 add of the two), and d_ypred is what the call without the link term writes."""
        lib, c = self.lib, self.c
        B = c.B
        st = _lib.current_stream()
        ce = torch.empty(1, device="cuda")
        prob = torch.empty(B, NCLASS, device="cuda")
        _lib.check(lib.dp_cross_entropy_fwd(self.ypred.data_ptr(), self.label.data_ptr(), ce.data_ptr(), prob.data_ptr(),
                                            B, NCLASS, st), "dp_cross_entropy_fwd")
        want = np.float32(ce.cpu().numpy()[0]) + np.float32(link)
        print(f"[linkpred] {c.name} {self.reader}: CE {float(ce):.8f} + link {float(link):.8f} = {float(extra['total']):.8f}")
        assert np.float32(extra["total"]).tobytes() == np.float32(want).tobytes()
        dy = torch.full((B * NCLASS + 8,), GUARD, device="cuda")
        wsb = lib.dp_loss_workspace_bytes(B, c.n, c.K, 0)
        ws = torch.full((wsb + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        _lib.check(lib.dp_loss_backward(extra["prob"].data_ptr(), self.label.data_ptr(), None, None, None, None,
                                        _lib.ptr(self.dl), dy.data_ptr(), None, B, NCLASS, c.n, c.K, 0, ws.data_ptr(),
                                        wsb, st), "dp_loss_backward")
        assert torch.equal(dy.cpu().view(torch.int32), extra["dy"].view(torch.int32)), "d_ypred depends on linkpred"


@pytest.mark.parametrize("name", [c.name for c in LC.CASES if LC.qualifies(c)])
def test_case_against_fp64_under_the_counted_bound(name):
    c = LC.by_name(name)
    lib = _lib.load()
    got_plan = _lib_plan(lib, c.B, c.n, c.K)
    assert got_plan == LC.plan(c.B, c.n, c.K), (name, got_plan)     # the path that runs is the one the row is there for
    inp = LC.build(c)
    ref = LC.reference(c, inp)
    assert ref["margin"] >= 64 * (c.K + 1) * LC.U
    old = LC.prior(c, ref) if c.acc else None
    f32 = LC.reference(c, inp, dtype=torch.float32, bounds=False)
    rf = LC.compare(c, inp, ref, np.float32(f32["loss"]), LC.full_output(c, inp, f32, old), old)
    first = None
    failures = []
    for reader in LC.readers(c):
        p = Problem(c, inp, reader, old)
        loss, dS, extra = p.run()
        r = LC.compare(c, inp, ref, loss, dS, old)
        print(f"[linkpred] {name} {reader} plan {got_plan[:5]} ({LC.plan_class(c.B, c.n, c.K)}): loss {float(loss):.9g} vs "
              f"{ref['loss']:.9g}, {r['fwd']:.4f} of its bound; dS {r['bwd']:.4f} of its bound "
              f"(fp32 formula: {rf['fwd']:.4f}, {rf['bwd']:.4f})")
        LC.record(c, reader, got_plan, r["fwd"], r["bwd"], (rf["fwd"], rf["bwd"]))
        failures += [f"{reader}: {m}" for m in r["problems"]]
        loss2, dS2, _ = p.run()
        if loss2.tobytes() != loss.tobytes() or dS2.tobytes() != dS.tobytes():
            failures.append(f"{reader}: a second run gives other bits")
        if c.via == "loss":
            p.check_loss_entries(loss, extra)
        if first is None:
            first = (loss, dS)
        elif LC.bf16_exact(c) and (loss.tobytes() != first[0].tobytes() or dS.tobytes() != first[1].tobytes()):
            failures.append("packed and fp32 readers differ in bits")
    assert not failures, failures


@pytest.mark.parametrize("reader", ["f32", "packed"])
def test_sharp_assignments_anchored_criterion(reader):
    """softmax(12 randn), B = 2, n = 256, K = 50: p within a few ulp of 1, where the direct fp32 formula is itself far
    from float64; max|dS_hip - dS_64| <= 4 max|dS_formula32 - dS_64| + 3e-7 max|dS_64| and the matching loss line,
    finite, and bit-reproducible."""
    c = LC.by_name("sharp")
    assert _lib_plan(_lib.load(), c.B, c.n, c.K) == LC.plan(c.B, c.n, c.K)
    inp = LC.build(c)
    ref = LC.reference(c, inp)
    assert ref["near"] <= 8 * LC.U
    f32 = LC.reference(c, inp, dtype=torch.float32, bounds=False)
    p = Problem(c, inp, reader, None)
    loss, dS, _ = p.run()
    r = LC.sharp_compare(ref, f32, loss, dS, inp["nnv"])
    text = (f"max|dS_64| {r['top']:.4e}  dS error: hip {r['e_hip']:.4e} formula32 {r['e_o32']:.4e}  "
            f"loss error: hip {r['l_hip']:.4e} formula32 {r['l_o32']:.4e}")
    print(f"[linkpred] sharp {reader}: {text}")
    LC.record(c, reader, LC.plan(c.B, c.n, c.K), 0.0, 0.0, None, text)
    assert np.isfinite(dS).all() and np.isfinite(loss)
    loss2, dS2, _ = p.run()
    assert loss2.tobytes() == loss.tobytes() and dS2.tobytes() == dS.tobytes()
    assert r["ok"], r


def test_k_257_is_refused_by_all_four_entries_before_any_launch():
    lib = _lib.load()
    for B, n, K in LC.REFUSED:
        ld = lib.dp_adj_pack_ld(n)
        S = torch.full((B, n, K), 0.5, device="cuda")
        A = torch.zeros(B, n, n, device="cuda")
        pk = torch.zeros(B, n, ld, dtype=torch.int16, device="cuda")
        dS = torch.full((B, n, K), GUARD, device="cuda")
        loss = torch.full((1,), GUARD, device="cuda")
        wsb = max(lib.dp_linkpred_workspace_bytes(B, n, K), lib.dp_linkpred_workspace_bytes(B, n, LC.K_MAX))
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
        st = _lib.current_stream()
        plan = (C.c_int * _lib.LINKPRED_PLAN_INTS)()
        assert lib.dp_linkpred_plan(B, n, K, plan) == -3
        rcs = [lib.dp_linkpred_loss_fwd(S.data_ptr(), A.data_ptr(), None, loss.data_ptr(), B, n, K, ws.data_ptr(), wsb, st),
               lib.dp_linkpred_loss_bwd(S.data_ptr(), A.data_ptr(), None, None, dS.data_ptr(), 0, B, n, K, ws.data_ptr(),
                                        wsb, st),
               lib.dp_linkpred_loss_fwd_packed(S.data_ptr(), pk.data_ptr(), None, loss.data_ptr(), B, n, K, ws.data_ptr(),
                                               wsb, st),
               lib.dp_linkpred_loss_bwd_packed(S.data_ptr(), pk.data_ptr(), pk.data_ptr(), None, None, dS.data_ptr(), 0,
                                               B, n, K, ws.data_ptr(), wsb, st)]
        assert rcs == [-3, -3, -3, -3], rcs
        assert b"K=257" in lib.dp_last_error_string()
        torch.cuda.synchronize()
        assert (dS == GUARD).all() and float(loss) == GUARD and (ws == 0xFF).all()
