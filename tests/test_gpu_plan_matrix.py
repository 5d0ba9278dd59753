"""Every alternate execution plan of the encoder against the CPU oracle.

dp_model.hip picks the kernels of a step from the batch geometry and from the DP_* environment knobs (dp_api.hip
knobs(), read once per process).  The README promises that no knob changes results beyond fp32 summation order.  Each
row of MATRIX below runs tests/_plan_worker.py in a fresh child with one knob setting, under the kernel trace, and
checks three things:

  * the worker's report: forward, assign_tensor, loss and every parameter gradient against the oracle; for `enz` also
    the evaluation forward and a captured hipGraph replay against the eager step, bit for bit (except the tensors the
    row names as float-atomic sums);
  * the witness: the multiset of (kernel, grid, workgroup) launches over the row's cases differs from the no-knob run's
    at the same cases — otherwise the knob was inert there and the row proved nothing;
  * the row's own kernel check (the plan the knob promises is the plan that ran).

The children run one at a time, each with a timeout.  A child that ends by a signal or a timeout stops the module: every
later row fails at once without starting another GPU process.  tests/test_knob_coverage_cpu.py keeps every knob the
library reads in this table (or in its list of exclusions)."""
import collections
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_plan_worker.py")
CASE_ORDER = ("enz", "dd", "odd", "widek", "p2", "er4", "er16", "b66", "mixed")   # a row's cases run in this order
MARKER = "spin_kernel"               # torch.cuda._sleep: the worker's per-case boundary in the trace
CHILD_TIMEOUT = 400
_STATE = {"abort": None, "reference": None}

_BASE = re.compile(r"(?:^|[\s:*&])(k_\w+|bgemm_kernel)\s*[<(]")


def base(kernel):
    """Kernel function name without namespace, template arguments or parameters ('' for kernels not of this library)."""
    m = _BASE.search(kernel)
    return m.group(1) if m else ""


def _match(kernel, pat):
    b = base(kernel)
    return b.startswith(pat[:-1]) if pat.endswith("*") else b == pat


def only(counter, *pats):
    """The launches of `counter` whose kernel matches one of the patterns ('name' exactly, 'prefix*')."""
    return collections.Counter({k: n for k, n in counter.items() if any(_match(k[0], p) for p in pats)})


def launched(counter, *pats):
    return sum(only(counter, *pats).values())


def summary(knob, ref):
    """'+name xN' / '-name xN': launches of the knob run the no-knob run lacks, and the other way round, by kernel."""
    plus, minus = collections.Counter(), collections.Counter()
    for k, n in (knob - ref).items():
        plus[base(k[0]) or k[0][:40]] += n
    for k, n in (ref - knob).items():
        minus[base(k[0]) or k[0][:40]] += n
    return " ".join([f"+{k} x{n}" for k, n in sorted(plus.items())] + [f"-{k} x{n}" for k, n in sorted(minus.items())])


def _trace(out, cases):
    """Per-case Counters of (kernel name, grid, workgroup), split at the worker's markers."""
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, os.listdir(out)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            segs.append(collections.Counter())
        elif segs:
            key = (name, tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"),
                   tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"))
            segs[-1][key] += 1
    other = sorted({r["Kernel_Name"][:80] for r in rows if not base(r["Kernel_Name"])})[:40]
    assert len(segs) == len(cases), f"{len(segs)} case markers in the trace for cases {cases}; other kernels: {other}"
    return dict(zip(cases, segs))


def run_child(env_extra, cases, tmpdir, loose=()):
    """One worker process under rocprofv3's kernel trace -> (report, {case: Counter}, wall seconds)."""
    if _STATE["abort"]:
        pytest.fail(f"not started: an earlier child {_STATE['abort']}")
    prof = shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    cases = [c for c in CASE_ORDER if c in cases]
    out = tempfile.mkdtemp(dir=str(tmpdir))
    report = os.path.join(out, "report.json")
    # the library reads every set DP_* variable as "on" (DP_NO_X=0 too): only DP_LIB and the row's knobs go through
    env = {k: v for k, v in os.environ.items() if not k.startswith("DP_") or k == "DP_LIB"}
    env.update(env_extra)
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable, WORKER, report]
    if loose:
        cmd += ["--loose", ",".join(loose)]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd + cases, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STATE["abort"] = f"with {env_extra} timed out after {CHILD_TIMEOUT} s"
        raise AssertionError(_STATE["abort"]) from None
    wall = time.monotonic() - t0
    if r.returncode < 0 or r.returncode == 124 or r.returncode >= 128:
        _STATE["abort"] = f"with {env_extra} ended by a signal (exit status {r.returncode})"
        raise AssertionError(f"{_STATE['abort']}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    assert r.returncode == 0 and os.path.exists(report), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with open(report) as f:
        rep = json.load(f)
    assert [c["name"] for c in rep["cases"]] == cases or not rep["ok"], rep
    return rep, _trace(out, [c["name"] for c in rep["cases"]]), wall


def _failures(rep):
    return "\n".join(f"{c['name']}: {c['error']}" for c in rep["cases"] if not c["ok"])


# ---------------------------------------------------------------- the kernel checks of the rows
class Run:
    """A row's trace next to the no-knob trace, over the row's cases: .knob / .ref (Counters), .cases {case: (k, r)}."""

    def __init__(self, per_case, ref_per_case, cases):
        self.cases = {c: (per_case[c], ref_per_case[c]) for c in cases}
        self.knob = sum((k for k, _ in self.cases.values()), collections.Counter())
        self.ref = sum((r for _, r in self.cases.values()), collections.Counter())


def absent(*pats, ref_has=True):
    """No launch of the patterns under the knob (and, with ref_has, some in the no-knob run: the knob removed them)."""
    def check(t):
        for p in pats:
            assert launched(t.knob, p) == 0, f"{p} launched {launched(t.knob, p)} times"
            if ref_has:
                assert launched(t.ref, p) > 0, f"the no-knob run has no {p} at these cases: the check is vacuous"
    return check


def both(*checks):
    def check(t):
        for c in checks:
            c(t)
    return check


def present(*pats):
    def check(t):
        for p in pats:
            assert launched(t.knob, p) > 0, f"{p} not launched"
    return check


def differs(*pats, what):
    """The launches (instantiation, grid, workgroup) of the patterns differ from the no-knob run's."""
    def check(t):
        k, r = only(t.knob, *pats), only(t.ref, *pats)
        assert r, f"the no-knob run has no {what} at these cases"
        assert k != r, f"{what}: same instantiations, grids and workgroups as the no-knob run"
    return check


def more_somewhere(*pats):
    """Some case launches the patterns more often under the knob than without it."""
    def check(t):
        hit = [c for c, (k, r) in t.cases.items() if launched(k, *pats) > launched(r, *pats)]
        assert hit, f"no case launches {pats} more often under the knob"
    return check


def witness_only(t):
    pass


GEMMS = ("bgemm_kernel", "k_gemm_split_bf16")
ROW_KERNELS = ("k_rownorm*", "k_widen_fwd", "k_bn_*", "k_softmax_mask*", "k_masked_max*")


class Row:
    def __init__(self, env, cases, check, loose=()):
        self.env, self.cases, self.check, self.loose = env, tuple(cases), check, tuple(loose)
        self.id = " ".join(f"{k}={v}" for k, v in env.items())


# The per-phase level-0 backward sums every GraphConv bias gradient of the level (both stacks) and the assign_pred bias
# gradient with float atomics (dp_model.hip: "bias gradients ... with float atomics", k_softmax_mask_bwd_plan): last-place
# differences between two runs of that plan, the captured replay included
ATOMIC_L0 = ("conv_first.bias", "conv_block.0.bias", "conv_last.bias", "assign_conv_first.bias",
             "assign_conv_block.0.bias", "assign_conv_last.bias", "assign_pred.bias")

MATRIX = [
    Row({"DP_NO_L0_PERSIST": "1"}, ("enz", "dd", "odd", "p2"), absent("k_level0_fwd", "k_level0_bwd"), ATOMIC_L0),
    Row({"DP_NO_L0_PERSIST_BWD": "1"}, ("enz", "dd", "odd"),
        both(present("k_level0_fwd"), absent("k_level0_bwd")), ATOMIC_L0),
    Row({"DP_NO_LEVEL_FUSION": "1"}, ("enz", "odd", "p2"),
        both(absent("k_small_level_*"), present("k_small_gcn_*"))),
    # the escape hatch of the device-error text (dp_api.hip): no kernel with a grid barrier at all
    Row({"DP_NO_LEVEL_FUSION": "1", "DP_NO_L0_PERSIST": "1"}, ("enz", "dd", "p2"),
        absent("k_level0_*", "k_small_level_*"), ATOMIC_L0),
    # enz, dd and p2 fold the head's backward into k_small_level_bwd; widek's last level (K = 153) runs k_head_bwd
    Row({"DP_NO_HEAD_FUSION": "1"}, ("enz", "dd", "p2", "widek"), absent("k_head_fwd", "k_head_bwd")),
    Row({"DP_NO_PACK": "1"}, ("enz", "dd", "widek"), absent("k_adj_pack*", "k_level0_*"), ATOMIC_L0),
    # er4 has too few 128 x 128 tiles for the split-bf16 GEMM (gemm_split_usable): er16 takes it
    Row({"DP_NO_SPLIT_GEMM": "1"}, ("er4", "er16"), absent("k_gemm_split_bf16")),
    Row({"DP_SPLIT_GEMM_W4": "1"}, ("er16",), differs("k_gemm_split_bf16", what="split-bf16 GEMM launches")),
    Row({"DP_AGG_WIDE": "0"}, ("dd", "widek", "er4"), absent("k_aggregate_wide*")),
    # widek and er4 already run k_aggregate_wide_dma for their widest operand: forcing adds k_aggregate_wide launches
    Row({"DP_AGG_WIDE": "1"}, ("dd", "widek", "er4"), more_somewhere("k_aggregate_wide*")),
    # dd aggregates inside k_level0_* and widek / er4 default to 16-row tiles: b66 is where 32 rows are the default
    Row({"DP_AGG_RT": "16"}, ("widek", "er4", "b66"), differs("k_aggregate", what="k_aggregate grids")),
    Row({"DP_AGG_RT": "32"}, ("widek", "er4", "b66"), differs("k_aggregate", what="k_aggregate grids")),
    Row({"DP_NODE_KSPLIT": "1"}, ("dd", "widek", "er4"), differs(*GEMMS, what="GEMM launches")),
    Row({"DP_NODE_KSPLIT": "8"}, ("dd", "widek", "er4"), differs(*GEMMS, what="GEMM launches")),
    Row({"DP_GEMM_TARGET_WGS": "64"}, ("dd", "er4"), differs(*GEMMS, what="GEMM launches")),
    Row({"DP_GEMM_TARGET_WGS": "4096"}, ("dd", "er4"), differs(*GEMMS, what="GEMM launches")),
    Row({"DP_NO_AGG_FIRST": "1"}, ("widek",), witness_only),
    Row({"DP_NO_WIDEN_FUSION": "1"}, ("widek", "er4"), absent("k_widen_fwd", "k_rownorm_bwd_mv")),
    Row({"DP_NO_ROW_QUADS": "1"}, ("widek", "er4"), differs(*ROW_KERNELS, what="row-kernel launches")),
    # enz and dd run no per-layer level backward (persistent level 0, whole-level pooled kernels): the hooks live in
    # the per-phase levels of odd and p2 and in widek's aggregate-first layer (k_scatter_add_cols_part)
    Row({"DP_NO_ROWPART_HOOK": "1"}, ("odd", "p2", "widek"), absent("k_scatter_add_cols_part")),
]


def _reference(tmp_path_factory):
    """The no-knob run over every case, once per module (its failure is remembered, never retried)."""
    if _STATE["reference"] is None:
        try:
            rep, per_case, wall = run_child({}, CASE_ORDER, tmp_path_factory.mktemp("plan_ref"))
            _STATE["reference"] = (rep, per_case, wall)
        except BaseException as e:
            _STATE["reference"] = e
            raise
    if isinstance(_STATE["reference"], BaseException):
        pytest.fail(f"the no-knob reference run failed: {_STATE['reference']}")
    return _STATE["reference"]


def test_no_knob_plans_against_the_oracle(tmp_path_factory):
    rep, per_case, wall = _reference(tmp_path_factory)
    print(f"\n[plan] no knob: {wall:.1f} s; " + ", ".join(f"{c['name']} {c['seconds']} s" for c in rep["cases"]))
    assert rep["ok"], _failures(rep)
    # `mixed`: the persistent forward with the per-phase backward (the worker also checks the launch counters)
    mixed = per_case["mixed"]
    assert launched(mixed, "k_level0_fwd") == 1 and launched(mixed, "k_level0_bwd") == 0, summary(mixed, collections.Counter())


@pytest.mark.parametrize("row", MATRIX, ids=[r.id for r in MATRIX])
def test_plan_against_the_oracle(row, tmp_path, tmp_path_factory):
    _, ref_cases, _ = _reference(tmp_path_factory)
    rep, per_case, wall = run_child(row.env, row.cases, tmp_path, row.loose)
    t = Run(per_case, ref_cases, [c["name"] for c in rep["cases"]])
    print(f"\n[plan] {row.id}: {wall:.1f} s; " +
          "; ".join(f"{c}: {summary(k, r) or 'same'}" for c, (k, r) in t.cases.items()))
    assert rep["ok"], _failures(rep)
    assert t.knob != t.ref, f"{row.id}: the same kernels, grids and workgroups as the no-knob run at {row.cases}"
    row.check(t)
