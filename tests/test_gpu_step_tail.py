"""The kernels that close every training step or open every GraphSAGE layer, through the C ABI against float64
references under the derived bounds of tests/step_tail_cases.py: cross entropy and the step's loss without the link term
(dp_cross_entropy_fwd / _bwd, dp_loss_forward / _backward), the fused clip + Adam step (dp_clip_adam_step,
dp_clip_adam_step_counted) and the mean aggregator with its scatter backward (dp_mean_aggregate_fwd / _bwd,
dp_csr_aggregate with mean = 1).  Guard bands around every output and in/out buffer, odd leading dimensions where an
entry takes one, workspaces filled with noise, repeat runs bit for bit (but for the atomic scatter).

With DP_STEP_TAIL_ANCHOR=<file> the largest |error| / bound per op and case is written there
(profiles/step_tail_fp64_anchor.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_weights_cases as WC
from tests import step_tail_cases as SC
from tests.test_gpu_csr_weights import Buf, _bits, _odd_ld, _ws

pytestmark = pytest.mark.gpu

RATIOS = {}


def anchor_text(ratios):
    """The worst ratio per op (the key's first word), then every case."""
    ops = {}
    for k, v in ratios.items():
        ops[k.split()[0]] = max(ops.get(k.split()[0], 0.0), v)
    lines = ["largest |error| / bound (bounds: tests/step_tail_cases.py, U = 2^-24)", "", "per op"]
    lines += [f"{k:<72s} {ops[k]:8.4f}" for k in sorted(ops)]
    lines += ["", "per case"]
    lines += [f"{k:<72s} {ratios[k]:8.4f}" for k in sorted(ratios)]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", autouse=True)
def _anchor_file():
    yield
    path = os.environ.get("DP_STEP_TAIL_ANCHOR")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write(anchor_text(RATIOS))


def _check(op, case, got, ref, bound, untouched=True):
    """`op`: one word, the line of the anchor's per-op table."""
    assert untouched, f"{op} {case}: wrote outside its output"
    ratio = SC.worst(np.asarray(got).reshape(np.shape(ref)), ref, bound)
    print(f"{op} {case}: worst |error| / bound = {ratio:.4f}")
    key = f"{op} {case}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{op} {case}: worst |error| / bound = {ratio:.3f}"


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ cross entropy
def _ce_forward(logits, label, with_prob=True):
    lib = _lib.load()
    B, C = logits.shape
    ld, yd = torch.from_numpy(logits).cuda(), torch.from_numpy(label).cuda()
    loss, prob = Buf(1, 1), Buf(B, C)
    _lib.check(lib.dp_cross_entropy_fwd(ld.data_ptr(), yd.data_ptr(), loss.ptr(), prob.ptr() if with_prob else None, B, C,
                                        _lib.current_stream()), "dp_cross_entropy_fwd")
    _sync()
    return loss, prob


def _ce_backward(prob32, label, dloss):
    lib = _lib.load()
    B, C = prob32.shape
    pd, yd = torch.from_numpy(np.ascontiguousarray(prob32, dtype=np.float32)).cuda(), torch.from_numpy(label).cuda()
    dl = None if dloss is None else torch.tensor([dloss], dtype=torch.float32).cuda()
    out = Buf(B, C)
    _lib.check(lib.dp_cross_entropy_bwd(pd.data_ptr(), yd.data_ptr(), None if dl is None else dl.data_ptr(), out.ptr(), B,
                                        C, _lib.current_stream()), "dp_cross_entropy_bwd")
    _sync()
    return out


def _loss_forward(logits, label, with_unit=True):
    lib = _lib.load()
    B, C = logits.shape
    ld, yd = torch.from_numpy(logits).cuda(), torch.from_numpy(label).cuda()
    out, prob, unit = Buf(1, 2), Buf(B, C), Buf(B, C)
    wsb = lib.dp_loss_workspace_bytes(B, 1, 1, 0)
    ws = _ws(wsb)
    _lib.check(lib.dp_loss_forward(ld.data_ptr(), yd.data_ptr(), None, None, None, None, out.ptr(), prob.ptr(),
                                   unit.ptr() if with_unit else None, B, C, 0, 0, 0, ws.data_ptr(), wsb,
                                   _lib.current_stream()), "dp_loss_forward")
    _sync()
    return out, prob, unit


def _loss_backward(prob32, label, dloss):
    lib = _lib.load()
    B, C = prob32.shape
    pd, yd = torch.from_numpy(np.ascontiguousarray(prob32, dtype=np.float32)).cuda(), torch.from_numpy(label).cuda()
    dl = None if dloss is None else torch.tensor([dloss], dtype=torch.float32).cuda()
    out = Buf(B, C)
    wsb = lib.dp_loss_workspace_bytes(B, 1, 1, 0)
    ws = _ws(wsb)
    _lib.check(lib.dp_loss_backward(pd.data_ptr(), yd.data_ptr(), None, None, None, None,
                                    None if dl is None else dl.data_ptr(), out.ptr(), None, B, C, 0, 0, 0, ws.data_ptr(),
                                    wsb, _lib.current_stream()), "dp_loss_backward")
    _sync()
    return out


@pytest.mark.parametrize("c", SC.ce_cases(), ids=lambda c: c.id)
def test_cross_entropy_and_the_loss_without_the_link_term(c):
    logits, label = SC.ce_inputs(c)
    ref = SC.ce_ref(logits, label)
    loss, prob = _ce_forward(logits, label)
    (lv, l_ok), (pv, p_ok) = loss.back(), prob.back()
    _check("ce_loss", c.id, lv, *ref["loss"], l_ok)
    _check("ce_prob", c.id, pv, *ref["prob"], p_ok)
    # prob = NULL: the same loss bits, nothing else written
    loss0, prob0 = _ce_forward(logits, label, with_prob=False)
    assert _bits(loss0.back()[0]) == _bits(lv) and loss0.back()[1]
    assert prob0.back()[1] and _bits(prob0.back()[0]) == _bits(prob0.view(prob0.host0).numpy())
    # repeat run
    loss1, prob1 = _ce_forward(logits, label)
    assert _bits(loss1.back()[0]) == _bits(lv) and _bits(prob1.back()[0]) == _bits(pv)

    # the step's loss, linkpred = 0: (CE, 0) in a guarded pair, prob and the unit gradient the fused backward consumes
    out, fprob, unit = _loss_forward(logits, label)
    (ov, o_ok), (fpv, fp_ok), (uv, u_ok) = out.back(), fprob.back(), unit.back()
    assert o_ok and _bits(ov[0, :1]) == _bits(lv), "loss_out[0] is not dp_cross_entropy_fwd's loss"
    assert _bits(ov[0, 1:]) == _bits(np.zeros(1)), "loss_out[1] is not +0.0"
    _check("ce_prob", c.id + " loss_forward", fpv, *ref["prob"], fp_ok)
    _check("ce_dunit", c.id, uv, *ref["dunit"], u_ok)
    out0, fprob0, unit0 = _loss_forward(logits, label, with_unit=False)         # d_ypred_unit = NULL is accepted
    assert _bits(out0.back()[0]) == _bits(ov) and _bits(fprob0.back()[0]) == _bits(fpv)
    assert unit0.back()[1] and _bits(unit0.back()[0]) == _bits(unit0.view(unit0.host0).numpy())
    out1, fprob1, unit1 = _loss_forward(logits, label)
    assert _bits(out1.back()[0]) == _bits(ov) and _bits(fprob1.back()[0]) == _bits(fpv) \
        and _bits(unit1.back()[0]) == _bits(uv)

    for dloss in SC.CE_DLOSS:
        r = SC.ce_ref(logits, label, dloss)["dlogits"]
        tag = f"{c.id} dloss={'NULL' if dloss is None else dloss}"
        d = _ce_backward(pv, label, dloss)
        dv, d_ok = d.back()
        _check("ce_dlogits", tag, dv, *r, d_ok)
        e = _loss_backward(pv, label, dloss)
        ev, e_ok = e.back()
        _check("ce_dlogits", tag + " loss_backward", ev, *r, e_ok)
        assert _bits(_ce_backward(pv, label, dloss).back()[0]) == _bits(dv)
        assert _bits(_loss_backward(pv, label, dloss).back()[0]) == _bits(ev) == _bits(dv)


# ------------------------------------------------------------------ clip + Adam
class AdamRun:
    """One step of either entry from the state x, every buffer guarded."""

    def __init__(self, x, t, max_norm, want_norm, counted):
        lib = _lib.load()
        n = x["g"].size
        self.buf = {k: Buf(1, n, data=x[k]) for k in "pgmv"}
        self.norm = Buf(1, 1)
        self.counter = torch.tensor([-7, t - 1, -7], dtype=torch.int32).cuda()
        wsb = lib.dp_clip_adam_workspace_bytes()
        ws = _ws(wsb)
        b = self.buf
        head = (b["p"].ptr(), b["g"].ptr(), b["m"].ptr(), b["v"].ptr(), n)
        tail = (SC.LR, SC.BETA1, SC.BETA2, SC.ADAM_EPS, max_norm, self.norm.ptr() if want_norm else None, ws.data_ptr(),
                wsb, _lib.current_stream())
        if counted:
            self.rc = lib.dp_clip_adam_step_counted(*head, self.counter.data_ptr() + 4, *tail)
        else:
            self.rc = lib.dp_clip_adam_step(*head, t, *tail)
        _sync()

    def back(self):
        out = {k: b.back() for k, b in self.buf.items()}
        out["norm"] = self.norm.back()
        return out


@pytest.mark.parametrize("counted", [False, True], ids=["step", "counted"])
@pytest.mark.parametrize("c", SC.adam_cases(), ids=lambda c: c.id)
def test_clip_adam_one_step_from_a_given_state(c, counted):
    x = SC.adam_inputs(c)
    _, max_norm, want_norm = SC.ADAM_STATES[c.state]
    ref = SC.adam_ref(x, c.t, max_norm)
    run = AdamRun(x, c.t, max_norm, want_norm, counted)
    _lib.check(run.rc, "dp_clip_adam_step")
    got = run.back()
    entry = "counted" if counted else "step"
    for name in "gmvp":
        _check(f"adam_{entry}_{name}", c.id, got[name][0], ref[name][0][None, :], ref[name][1][None, :], got[name][1])
    if want_norm:
        _check(f"adam_{entry}_norm", c.id, got["norm"][0], *ref["norm"], got["norm"][1])
    else:
        assert got["norm"][1] and _bits(got["norm"][0]) == _bits(run.norm.view(run.norm.host0).numpy())
    if max_norm <= 0:
        assert _bits(got["g"][0]) == _bits(x["g"]), "g changed without clipping"
    assert run.counter.cpu().tolist() == ([-7, c.t, -7] if counted else [-7, c.t - 1, -7])
    again = AdamRun(x, c.t, max_norm, want_norm, counted).back()
    for name in got:
        assert _bits(again[name][0]) == _bits(got[name][0]), name


@pytest.mark.parametrize("counted", [False, True], ids=["step", "counted"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_clip_adam_skips_a_non_finite_gradient_norm(bad, counted):
    """Parameters, gradients, moments and every guard stay bit for bit and DP_DEVERR_NONFINITE_GRAD is raised.
    Behaviour found, and pinned here: the counted form's counter is incremented on the skipped step too (the norm kernel
    counts, one launch ahead of the kernel that finds the norm non-finite), so the next update takes the bias
    corrections of t + 1."""
    lib = _lib.load()
    c = SC.AdamCase(f"n={SC.NONFINITE_N} non-finite", SC.NONFINITE_N, "plain", 5)
    x = SC.adam_inputs(c)
    x["g"][40000] = bad
    assert lib.dp_device_error(0) == 0
    try:
        run = AdamRun(x, c.t, 2.0, True, counted)
        _lib.check(run.rc, "dp_clip_adam_step")
        got = run.back()
        for name in "pgmv":
            assert got[name][1], name
            assert _bits(got[name][0]) == _bits(x[name]), f"{name} changed on a skipped step"
        assert got["norm"][1] and not np.isfinite(got["norm"][0]).any()
        assert lib.dp_device_error(0) == _lib.DEVERR_NONFINITE_GRAD
        assert run.counter.cpu().tolist() == ([-7, c.t, -7] if counted else [-7, c.t - 1, -7])
    finally:
        _sync()
        lib.dp_device_error(1)
    assert lib.dp_device_error(0) == 0


@pytest.mark.parametrize("counted", [False, True], ids=["step", "counted"])
def test_clip_adam_without_clip_and_norm_does_not_look_at_finiteness(counted):
    """What diffpool_hip.h states for max_norm <= 0 with total_norm_out == NULL: no norm is taken, so a NaN gradient is
    not skipped and nothing is raised; the update is elementwise, so exactly that element turns NaN."""
    lib = _lib.load()
    c = SC.AdamCase("n=1000 no clip, no norm, one NaN", 1000, "no clip, no norm", 4)
    x = SC.adam_inputs(c)
    clean = AdamRun(x, c.t, 0.0, False, counted)
    _lib.check(clean.rc, "dp_clip_adam_step")
    want = clean.back()
    x["g"][7] = float("nan")
    assert lib.dp_device_error(0) == 0
    try:
        run = AdamRun(x, c.t, 0.0, False, counted)
        _lib.check(run.rc, "dp_clip_adam_step")
        got = run.back()
        assert lib.dp_device_error(0) == 0
    finally:
        _sync()
        lib.dp_device_error(1)
    others = np.arange(c.n) != 7
    for name in "pmv":
        assert got[name][1] and np.isnan(got[name][0][0, 7]), name
        assert _bits(got[name][0][0, others]) == _bits(want[name][0][0, others]), name
    assert got["g"][1] and _bits(got["g"][0]) == _bits(x["g"])
    assert got["norm"][1] and _bits(got["norm"][0]) == _bits(run.norm.view(run.norm.host0).numpy())


# ------------------------------------------------------------------ mean aggregation
@pytest.fixture(scope="module")
def agg_case():
    g = WC.agg_graph()
    assert WC.degrees(g)[:len(WC.AGG_DEGREES)].tolist() == list(WC.AGG_DEGREES)
    return WC.to_device(g, "cuda"), SC.dense01(g), WC.degrees(g)


def _mean_fwd(g, x, old, n_rows, ldt, ldo, beta=None):
    """beta None: dp_mean_aggregate_fwd; else dp_csr_aggregate(mean = 1, beta).  The output holds all n rows of `old`,
    so a row written past n_rows shows in the returned values."""
    lib = _lib.load()
    n, feat = x.shape
    tab, out = Buf(n, feat, ldt, data=x), Buf(n, feat, ldo, data=old)
    st = _lib.current_stream()
    if beta is None:
        _lib.check(lib.dp_mean_aggregate_fwd(tab.ptr(), ldt, g.indptr.data_ptr(), g.indices.data_ptr(), out.ptr(), ldo,
                                             n_rows, feat, st), "dp_mean_aggregate_fwd")
    else:
        _lib.check(lib.dp_csr_aggregate(tab.ptr(), ldt, g.indptr.data_ptr(), g.indices.data_ptr(), out.ptr(), ldo, n_rows,
                                        feat, 1, beta, st), "dp_csr_aggregate")
    _sync()
    assert tab.back()[1] and _bits(tab.back()[0]) == _bits(x)
    return out.back()


def _mean_bwd(g, dout, dt_old, ldo, ldt):
    lib = _lib.load()
    n_rows, feat = dout.shape
    db, dt = Buf(n_rows, feat, ldo, data=dout), Buf(g.n, feat, ldt, data=dt_old)
    _lib.check(lib.dp_mean_aggregate_bwd(db.ptr(), ldo, g.indptr.data_ptr(), g.indices.data_ptr(), dt.ptr(), ldt, n_rows,
                                         feat, _lib.current_stream()), "dp_mean_aggregate_bwd")
    _sync()
    return dt.back()


@pytest.mark.parametrize("n_rows", SC.MEAN_NROWS)
@pytest.mark.parametrize("feat", WC.AGG_FEATS)
def test_mean_aggregate_forward_and_scatter_backward(agg_case, feat, n_rows):
    g, a, deg = agg_case
    x = SC.mean_inputs(g.n, n_rows, feat)
    ldt, ldo = _odd_ld(feat, 2), _odd_ld(feat, 4)
    assert ldt != ldo
    case = f"feat={feat} n_rows={n_rows}"
    deg0 = np.repeat((deg[:n_rows] == 0)[:, None], feat, axis=1)
    assert deg0[0].all()
    plain = None
    for beta in (None, 0.0, 1.0):
        got, clean = _mean_fwd(g, x["x"], x["old"], n_rows, ldt, ldo, beta)
        ref, bound = SC.mean_fwd_ref(a, x["x"], n_rows, beta or 0.0, x["old"])
        assert np.array_equal(np.isnan(got[:n_rows]), deg0), f"{case}: NaN in other rows than those of degree 0"
        _check("mean_fwd", f"{case} {'entry' if beta is None else f'beta={beta:g}'}", got[:n_rows], ref, bound, clean)
        assert _bits(got[n_rows:]) == _bits(x["old"][n_rows:]), f"{case}: a row past n_rows was written"
        again, _ = _mean_fwd(g, x["x"], x["old"], n_rows, ldt, ldo, beta)
        assert _bits(again) == _bits(got)
        if beta is None:
            plain = got
        elif beta == 0.0:
            assert _bits(got) == _bits(plain), "dp_mean_aggregate_fwd is not dp_csr_aggregate(mean = 1, beta = 0)"

    ref, bound = SC.mean_bwd_ref(a, x["dout"], n_rows, x["dt_old"])
    for run in range(2):                                  # float atomics fix no order: both runs within bound, no bits
        got, clean = _mean_bwd(g, x["dout"], x["dt_old"], ldo, ldt)
        assert np.isfinite(got).all(), f"{case}: a row of degree 0 reached dtable"
        _check("mean_bwd", f"{case} run {run}", got, ref, bound, clean)


def test_mean_aggregate_is_exact_on_an_integer_grid():
    gh = SC.grid_graph()
    g, a = WC.to_device(gh, "cuda"), SC.dense01(gh)
    rng = np.random.default_rng(5)
    x, dout, old = (rng.integers(-8, 9, (g.n, 65)).astype(np.float32) for _ in range(3))
    got, clean = _mean_fwd(g, x, old, g.n, 67, 69)
    assert clean and np.array_equal(got.astype(np.float64), SC.mean_fwd_ref(a, x, g.n)[0])
    got, clean = _mean_bwd(g, dout, old, 69, 67)
    assert clean and np.array_equal(got.astype(np.float64), SC.mean_bwd_ref(a, dout, g.n, old)[0])
