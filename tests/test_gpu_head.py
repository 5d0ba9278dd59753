"""The prediction-head kernels of csrc/dp_head.hip -- k_head_fwd (last-level max readout + pred_model) and k_head_bwd
(pred_model's backward + the max-readout scatter of every level) -- at every staging round, readout form, MLP pass,
slice and batch edge of tests/head_cases.py, anchored to fp64.  Per case:

  (1) readout, exact: for the level the head kernel reads, every recorded winner is the LOWEST row holding the exact fp32
      column maximum of the saved embedding; for the other levels the winner holds the column's maximum value;
  (2) in this process, no knob: the head ALONE against an fp64 evaluation of the same operation on the GPU's own inputs
      (ypred and every pred_model gradient; bound max(8 e_ref, 16 * 2^-24 * max|ref|), e_ref the error of the same graph
      in fp32 torch on the CPU);
  (3) the whole model against the fp64 oracle with the HIP forward's winners forced in, at tests/parity.py's tolerances:
      the check of the d(features) scatter, which reaches the stack parameters of every level only through dZ;
  (4) the device error word reads 0;
  (5) a child with DP_NO_HEAD_FOLD=1: checks (1)-(3) on the child's tensors for every case whose no-knob backward folds
      into the last level's kernel, and which now runs k_head_bwd;
  (6) both children run under the kernel trace; split at the worker's markers, each case shows the table's plan:
      k_head_fwd once (`fused`) or not at all, k_head_bwd once (`kernel`) or not at all, k_reduce_slabs_head exactly
      where the head folds.  The no-knob child runs the table in REVERSE order and must carry the bits of this process's
      run (float-atomic bias sums of the generic sequence: rtol 1e-5 / atol 1e-7, named by rule in head_cases.loose_names);
  (7) model.predict returns the arg-max of the fp64 logits wherever their margin exceeds twice the bound of (2); with the
      last Linear's weight zero and bias (0.5, 0.7, 0.7) it returns class 1 for every graph (first index on ties).

The children run one at a time, each with a timeout; a child that ends by a signal or a timeout fails the module and no
later child is started.  Every figure is printed ("[head] ...") before it is asserted; profiles/head_fp64_anchor.txt
keeps those of the first full run."""
import collections
import csv
import functools
import glob
import os
import re
import shutil
import subprocess
import sys
import time

import pytest
import torch

from graph_pooling_amd import _lib
from tests import head_cases as HC
from tests import small_level_cases as SC
from tests.parity import close, grads_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_head_worker.py")
MARKER = "spin_kernel"               # torch.cuda._sleep: the worker's per-case boundary in the trace
CHILD_TIMEOUT = 120                  # a child takes 3.5 s under the trace (profiles/head_fp64_anchor.txt)
KERNELS = ("k_head_fwd", "k_head_bwd", "k_reduce_slabs_head")
_STATE = {"abort": None, "children": {}}
_BASE = re.compile(r"\bk_\w+")           # the kernel's function name inside the trace's demangled signature


# ---------------------------------------------------------------- this process's run
@functools.lru_cache(maxsize=None)
def _eager(name):
    """(tensors of head_cases.results, loss, predicted classes, device error word) of the no-knob step in this process."""
    assert not [k for k in os.environ if k.startswith("DP_") and k != "DP_LIB"], "this module tests the no-knob plan"
    c = HC.CASE[name]
    model, _, x, adj, nn_, label = HC.build(name)
    model = model.cuda()
    xd, ad = x.cuda(), adj.cuda()
    y, loss = HC.step(model, c, xd, ad, nn_, label.cuda())
    torch.cuda.synchronize()
    got = HC.results(model, c, y)
    labels = HC.call(model, c, xd, ad, nn_, predict=True).cpu()
    return got, loss.detach().cpu(), labels, _lib.load().dp_device_error(0)


def _check_readout(name, got, what, head_reads_last, nn_):
    """Check (1)."""
    c = HC.CASE[name]
    for j in range(c.P + 1):
        blk = HC.readout_rows(c, j, got[f"emb{j}"], nn_)
        win = got[f"argmax{j}"]
        top, first = HC.lowest_row_of_max(blk)
        held = SC.readout(blk, win)
        exact = head_reads_last and j == c.P
        wrong = int((win != first).sum()) if exact else int((held != top).sum())
        print(f"[head] {name} {what} level {j} ({tuple(blk.shape)}): {'lowest row of the maximum' if exact else 'holds the maximum'}"
              f", {wrong} of {win.numel()} winners wrong, {int((win < 0).sum())} are -1")
        assert win.shape == top.shape and wrong == 0
        assert int(win.max()) < blk.shape[1] and int(win.min()) >= (-1 if (c.fam == "P" and j == 0) else 0)
    if c.special == "tie":
        assert int(got[f"argmax{c.P}"][:, c.H * (c.L - 1):].abs().max()) == 0, "a tie did not go to row 0"
    if c.special == "neg":
        assert int((got["argmax0"] < 0).sum()) >= 1, "no level-0 winner is -1"


def _check(name, got, loss, what, fwd_plan):
    """Checks (1), (2) and (3) of one run's tensors; prints every figure before asserting."""
    c = HC.CASE[name]
    model, params, x, adj, nn_, label = HC.build(name)
    assert torch.isfinite(got["ypred"]).all()
    _check_readout(name, got, what, c.fam == "P" and fwd_plan == "fused", nn_)
    rows = HC.head_figures(c, params, label, got)
    for k, err, e_ref, bound, scale in rows:
        print(f"[head] {name} {what} {k}: error {err:.3e} e_ref {e_ref:.3e} ratio "
              f"{err / e_ref if e_ref else float('nan'):.2f} bound {bound:.3e} error/bound {err / bound:.3f} "
              f"max|ref| {scale:.3e}")
    bad = HC.failures(rows)
    assert not bad, f"{name} ({what}), the head alone against fp64: " + "; ".join(bad)
    yo, lo, grads = HC.end_to_end(c, params, x, adj, nn_, label, HC.winners(c, got))
    close(got["ypred"], yo)
    if loss is not None:
        close(loss, lo, 1e-4, 1e-6)
    for k, p in model.named_parameters():
        p.grad = got["grad." + k]
    grads_close(model, grads)
    return rows


@pytest.mark.parametrize("name", HC.NAMES)
def test_readout_head_alone_and_whole_model_against_fp64(name):
    c = HC.CASE[name]
    got, loss, _, dev_err = _eager(name)
    assert dev_err == 0, f"device error word {dev_err:#x}"
    _check(name, got, loss, f"{c.fwd}/{c.bwd}", c.fwd)


@pytest.mark.parametrize("name", HC.NAMES)
def test_predict_is_the_argmax_of_the_fp64_logits(name):
    c = HC.CASE[name]
    got, _, labels, _ = _eager(name)
    _, params, _, _, _, label = HC.build(name)
    y64 = HC.head_alone(c, params, label, got, torch.float64)["ypred"]
    bound = [r[3] for r in HC.head_figures(c, params, label, got) if r[0] == "ypred"][0]
    top2 = y64.topk(2, dim=1)[0]
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bound
    want = y64.max(dim=1)[1]
    print(f"[head] {name} predict: {int(sure.sum())} of {c.B} graphs decided beyond 2 x {bound:.3e}, "
          f"{int((labels[sure] != want[sure]).sum())} differ")
    assert labels.dtype == torch.int64 and labels.shape == (c.B,) and int(sure.sum()) >= 1
    assert int(labels.min()) >= 0 and int(labels.max()) < c.C
    assert torch.equal(labels[sure], want[sure])


def test_predict_gives_a_tie_to_the_first_index():
    c = HC.CASE[HC.PREDICT_TIE]
    model, _, x, adj, nn_, _ = HC.build(HC.PREDICT_TIE, predict_tie=True)
    model = model.cuda()
    labels = HC.call(model, c, x.cuda(), adj.cuda(), nn_, predict=True).cpu()
    print(f"[head] predict tie ({HC.PREDICT_TIE}, bias {HC.PREDICT_TIE_BIAS}): classes {sorted(set(labels.tolist()))}")
    assert torch.equal(labels, torch.ones(c.B, dtype=torch.int64))
    assert _lib.load().dp_device_error(0) == 0


# ---------------------------------------------------------------- the children
def _base(kernel):
    m = _BASE.search(kernel)
    return m.group(0) if m else ""


def _trace(out, order):
    """{case: Counter of kernel function names}, split at the worker's markers."""
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, os.listdir(out)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        if MARKER in r["Kernel_Name"]:
            segs.append(collections.Counter())
        elif segs:
            segs[-1][_base(r["Kernel_Name"])] += 1
    assert len(segs) == len(order), f"{len(segs)} case markers in the trace for {len(order)} cases"
    return dict(zip(order, segs))


def _child(knob, tmp_path_factory):
    """One worker under the kernel trace, once per module: (saved run, {case: Counter}, wall seconds)."""
    if knob in _STATE["children"]:
        res = _STATE["children"][knob]
        if isinstance(res, BaseException):
            pytest.fail(f"the child with DP_NO_HEAD_FOLD={knob} failed: {res}")
        return res
    if _STATE["abort"]:
        pytest.fail(f"not started: an earlier child {_STATE['abort']}")
    try:
        res = _STATE["children"][knob] = _run_child(knob, tmp_path_factory.mktemp("head"))
    except BaseException as e:
        _STATE["children"][knob] = e
        raise
    return res


def _run_child(knob, tmp):
    prof = shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    out, path = str(tmp / "trace"), str(tmp / "run.pt")
    # the library reads every set DP_* variable as "on": only DP_LIB and the row's own knob go through
    env = {k: v for k, v in os.environ.items() if not k.startswith("DP_") or k == "DP_LIB"}
    if knob:
        env["DP_NO_HEAD_FOLD"] = "1"
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable, WORKER, path]
    cmd += [] if knob else ["--reverse"]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STATE["abort"] = f"(DP_NO_HEAD_FOLD={knob}) timed out after {CHILD_TIMEOUT} s"
        raise AssertionError(_STATE["abort"]) from None
    wall = time.monotonic() - t0
    if r.returncode < 0 or r.returncode == 124 or r.returncode >= 128:
        _STATE["abort"] = f"(DP_NO_HEAD_FOLD={knob}) ended by a signal (exit status {r.returncode})"
        raise AssertionError(f"{_STATE['abort']}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    assert r.returncode == 0 and os.path.exists(path), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    run = torch.load(path)
    assert run["error"] is None, run["error"]
    assert sorted(run["order"]) == sorted(HC.NAMES)
    print(f"\n[head] child DP_NO_HEAD_FOLD={int(knob)}: {wall:.1f} s wall, "
          f"{sum(run['seconds'].values()):.1f} s in the cases, slowest "
          f"{max(run['seconds'], key=run['seconds'].get)} {max(run['seconds'].values()):.2f} s")
    return run, _trace(out, run["order"]), wall


@pytest.mark.parametrize("name", HC.FOLD)
def test_k_head_bwd_under_the_knob_against_fp64(name, tmp_path_factory):
    run, _, _ = _child(True, tmp_path_factory)
    _check(name, run["cases"][name], None, "fused/kernel(knob)", "fused")


@pytest.mark.parametrize("knob", [False, True], ids=["no_knob", "DP_NO_HEAD_FOLD"])
@pytest.mark.parametrize("name", HC.NAMES)
def test_the_trace_shows_the_plan_the_table_expects(name, knob, tmp_path_factory):
    c = HC.CASE[name]
    _, per_case, _ = _child(knob, tmp_path_factory)
    k = per_case[name]
    bwd = "kernel" if (knob and c.bwd == "fold") else c.bwd
    got = tuple(k[n] for n in KERNELS)
    print(f"[head] {name} {'knob' if knob else 'no knob'}: trace plan {c.fwd}/{bwd} "
          + " ".join(f"{n} x{v}" for n, v in zip(KERNELS, got)))
    assert got == (int(c.fwd == "fused"), int(bwd == "kernel"), int(bwd == "fold")), (c.fwd, bwd, got)


@pytest.mark.parametrize("name", HC.NAMES)
def test_reverse_order_in_a_child_carries_the_same_bits(name, tmp_path_factory):
    run, _, _ = _child(False, tmp_path_factory)
    assert run["order"] == list(reversed(HC.NAMES))
    c = HC.CASE[name]
    got, want = run["cases"][name], _eager(name)[0]
    assert set(got) == set(want)
    loose = HC.loose_names(HC.build(name)[0], c)
    differ = [k for k in got if k not in loose and not torch.equal(got[k], want[k])]
    assert not differ, f"the reverse-order child against this process: {differ}"
    for k in loose:
        assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-7), f"the reverse-order child against this process: {k}"
