"""The one-workgroup-per-graph kernels of csrc/dp_small.hip -- k_small_level_fwd/bwd (the whole-level tier) and
k_small_gcn_fwd/bwd (the per-layer tier) -- at every tier, tile edge, batch block and stack depth of
tests/small_level_cases.py, anchored to fp64.  Per case:

  (a) in this process, no knob: the level ALONE against an fp64 evaluation of the same operation on the GPU's own inputs
      (embedding, then the gradients of the level's stack and of pred_model; bound max(8 e_ref, 16 * 2^-24 * max|ref|),
      e_ref the error of the same graph in fp32 torch on the CPU), then the whole model against the fp64 oracle with the
      HIP forward's winners forced in, at tests/parity.py's tolerances -- the check of the level's input gradients,
      which reach level 0's stacks and assign_pred only through dX0 and dadj; the device error word reads 0;
  (b) a child with DP_NO_LEVEL_FUSION=1: the same two checks on the child's tensors for every case whose tier is
      `whole`, which now runs the per-layer kernels;
  (c) both children run under the kernel trace; split at the worker's markers, each case shows the table's tier: one
      k_small_level_fwd and one k_small_level_bwd (`whole`), L of k_small_gcn_fwd and L of k_small_gcn_bwd
      (`per_layer`), or neither family (`generic`); and k_reduce_slabs_head exactly where the head folds;
  (d) the no-knob child runs the table in REVERSE order and must carry the bits of this process's run: a stale tagged
      exchange entry, a sequence number or LDS content leaking from one launch geometry into the next, or any
      run-to-run nondeterminism, shows here (float-atomic bias sums of the generic sequence: rtol 1e-5 / atol 1e-7,
      named by rule in small_level_cases.loose_names);
  (e) three replays of a captured step carry the eager step's bits, for one case per tier and the Bmax case.

The children run one at a time, each with a timeout; a child that ends by a signal or a timeout fails the module and no
later child is started.  Every figure is printed ("[small-level] ...") before it is asserted;
profiles/small_level_fp64_anchor.txt keeps those of the first full run."""
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
from tests import small_level_cases as SC
from tests.parity import close, grads_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_small_level_worker.py")
MARKER = "spin_kernel"               # torch.cuda._sleep: the worker's per-case boundary in the trace
CHILD_TIMEOUT = 120                  # a child takes 3.5 s under the trace (profiles/small_level_fp64_anchor.txt)
WHOLE = [c.name for c in SC.CASES if c.tier == "whole"]
REPLAY = ["p_n16_b15", "p_e65", "p_n65", "p_bmax"]          # whole, per_layer, generic, and B = Bmax
_STATE = {"abort": None, "children": {}}
_BASE = re.compile(r"\bk_\w+")           # the kernel's function name inside the trace's demangled signature


def _bmax():
    return min(128, torch.cuda.get_device_properties(0).multi_processor_count // 2)


# ---------------------------------------------------------------- this process's run
@functools.lru_cache(maxsize=None)
def _eager(name):
    """(tensors of small_level_cases.results, loss, device error word) of the no-knob step in this process."""
    assert not [k for k in os.environ if k.startswith("DP_") and k != "DP_LIB"], "this module tests the no-knob plan"
    c = SC.CASE[name]
    model, _, x, adj, nn_, label = SC.build(name, _bmax())
    model = model.cuda()
    y, loss = SC.step(model, c, x.cuda(), adj.cuda(), nn_, label.cuda())
    torch.cuda.synchronize()
    return SC.results(model, c, y), loss.detach().cpu(), _lib.load().dp_device_error(0)


def _check(name, got, loss, what):
    """Checks (ii) and (i) of one run's tensors; prints every figure of (ii) before asserting."""
    c = SC.CASE[name]
    model, params, x, adj, nn_, label = SC.build(name, _bmax())
    assert torch.isfinite(got["ypred"]).all()
    rows = SC.level_figures(c, params, label, got, x, adj)
    for k, err, e_ref, bound, scale in rows:
        print(f"[small-level] {name} {what} {k}: error {err:.3e} e_ref {e_ref:.3e} ratio "
              f"{err / e_ref if e_ref else float('nan'):.2f} bound {bound:.3e} max|ref| {scale:.3e}")
    bad = SC.failures(rows)
    assert not bad, f"{name} ({what}), the level alone against fp64: " + "; ".join(bad)
    # (i) the whole model (the winners of the level under test were checked with the level; level 0's of family P here)
    win = [got["argmax0"]]
    if c.fam == "P":
        SC.check_winners(SC.level0_embedding(c, params, x, adj, nn_), got["argmax0"], name + " level 0")
        win.append(got["argmax1"])
    yo, lo, grads, _ = SC.end_to_end(c, params, x, adj, nn_, label, win)
    close(got["ypred"], yo)
    if loss is not None:
        close(loss, lo, 1e-4, 1e-6)
    for k, p in model.named_parameters():
        p.grad = got["grad." + k]
    grads_close(model, grads)


@pytest.mark.parametrize("name", SC.NAMES)
def test_level_alone_and_whole_model_against_fp64(name):
    got, loss, dev_err = _eager(name)
    assert dev_err == 0, f"device error word {dev_err:#x}"
    _check(name, got, loss, SC.CASE[name].tier)


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
            pytest.fail(f"the child with DP_NO_LEVEL_FUSION={knob} failed: {res}")
        return res
    if _STATE["abort"]:
        pytest.fail(f"not started: an earlier child {_STATE['abort']}")
    try:
        res = _STATE["children"][knob] = _run_child(knob, tmp_path_factory.mktemp("small_level"))
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
        env["DP_NO_LEVEL_FUSION"] = "1"
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable, WORKER, path]
    cmd += [] if knob else ["--reverse"]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STATE["abort"] = f"(DP_NO_LEVEL_FUSION={knob}) timed out after {CHILD_TIMEOUT} s"
        raise AssertionError(_STATE["abort"]) from None
    wall = time.monotonic() - t0
    if r.returncode < 0 or r.returncode == 124 or r.returncode >= 128:
        _STATE["abort"] = f"(DP_NO_LEVEL_FUSION={knob}) ended by a signal (exit status {r.returncode})"
        raise AssertionError(f"{_STATE['abort']}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    assert r.returncode == 0 and os.path.exists(path), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    run = torch.load(path)
    assert run["error"] is None, run["error"]
    assert sorted(run["order"]) == sorted(SC.NAMES) and run["bmax"] == _bmax()
    print(f"\n[small-level] child DP_NO_LEVEL_FUSION={int(knob)}: {wall:.1f} s wall, "
          f"{sum(run['seconds'].values()):.1f} s in the cases, slowest "
          f"{max(run['seconds'], key=run['seconds'].get)} {max(run['seconds'].values()):.2f} s")
    return run, _trace(out, run["order"]), wall


@pytest.mark.parametrize("name", WHOLE)
def test_per_layer_tier_under_the_knob_against_fp64(name, tmp_path_factory):
    run, _, _ = _child(True, tmp_path_factory)
    _check(name, run["cases"][name], None, "per_layer(knob)")


@pytest.mark.parametrize("knob", [False, True], ids=["no_knob", "DP_NO_LEVEL_FUSION"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_trace_shows_the_tier_the_table_expects(name, knob, tmp_path_factory):
    c = SC.CASE[name]
    _, per_case, _ = _child(knob, tmp_path_factory)
    k = per_case[name]
    tier = "per_layer" if (knob and c.tier == "whole") else c.tier
    got = {n: k[n] for n in ("k_small_level_fwd", "k_small_level_bwd", "k_small_gcn_fwd", "k_small_gcn_bwd")}
    print(f"[small-level] {name} {'knob' if knob else 'no knob'}: trace tier {tier} "
          + " ".join(f"{n} x{v}" for n, v in got.items()) + f" k_reduce_slabs_head x{k['k_reduce_slabs_head']}")
    want = {"whole": (1, 1, 0, 0), "per_layer": (0, 0, c.L, c.L), "generic": (0, 0, 0, 0)}[tier]
    assert tuple(got.values()) == want, (tier, got)
    folds = (not knob) and SC.head_folds(c, _bmax())
    assert k["k_reduce_slabs_head"] == (1 if folds else 0), "the head fold is not where small_head_fold_fits puts it"


def _same_bits(name, got, want, what):
    c = SC.CASE[name]
    assert set(got) == set(want)
    loose = SC.loose_names(SC.build(name, _bmax())[0], c, c.tier)
    differ = [k for k in got if k not in loose and not torch.equal(got[k], want[k])]
    assert not differ, f"{what}: {differ}"
    for k in loose:
        assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-7), f"{what}: {k}"


@pytest.mark.parametrize("name", SC.NAMES)
def test_reverse_order_in_a_child_carries_the_same_bits(name, tmp_path_factory):
    run, _, _ = _child(False, tmp_path_factory)
    assert run["order"] == list(reversed(SC.NAMES))
    _same_bits(name, run["cases"][name], _eager(name)[0], "the reverse-order child against this process")


@pytest.mark.parametrize("name", REPLAY)
def test_three_replays_of_a_captured_step_equal_the_eager_step(name):
    c = SC.CASE[name]
    want = _eager(name)[0]
    # a model of its own: no grad-accumulation node of an earlier eager step may be alive while the backward is captured
    model, _, x, adj, nn_, label = SC.build(name, _bmax())
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    nd = torch.from_numpy(nn_).cuda()                    # device num_nodes: no H2D inside the captured region
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            SC.step(model, c, xd, ad, nd, ld)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        y_static, _ = SC.step(model, c, xd, ad, nd, ld)
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        _same_bits(name, SC.results(model, c, y_static), want, f"replay {rep} against the eager step")
    del g
    assert _lib.load().dp_device_error(0) == 0


def test_the_cases_named_here_are_what_they_claim():
    assert [SC.CASE[n].tier for n in REPLAY[:3]] == ["whole", "per_layer", "generic"] and SC.CASE[REPLAY[3]].B == "bmax"
