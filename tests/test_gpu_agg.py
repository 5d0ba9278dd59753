"""The adjacency aggregation of dp_agg.hip at every form, tile and loop edge: the table of tests/agg_cases.py
(test_agg_plan_cpu.py asserts what it reaches) through dp_adj_aggregate, dp_adj_pack + dp_adj_aggregate_packed,
dp_adj_aggregate_rownorm and dp_adj_pack_zero.  Every row runs twice and must give the same bits (a packed row the second
time with presplit = 1); the grid run is compared with the float64 product exactly over the whole U allocation, the dense
run at the bound derived in agg_cases.py, the fused tail at the counted-rounding bounds of rowop_cases.py with the
product's bound carried through; guard bands, padding columns and absent outputs exactly.

Rows that need DP_AGG_WIDE or DP_AGG_RT run in a fresh child process per knob setting (tests/_agg_worker.py), one after
another, each under its own timeout; a child that ends by a signal or a timeout stops the module.

DP_AGG_ANCHOR_OUT=<file> appends one line per row with its form and its largest error / bound
(profiles/agg_fp64_anchor.txt is the digest of such a file: `python -m tests.agg_cases --digest <file> <digest>`)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from graph_pooling_amd import _lib
from tests import agg_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
_STATE = {"abort": None}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    assert AC.knobs_unset(), "unset %s: the in-process rows are those of a process without knobs" % (AC.KNOBS,)
    return _lib.load()


@pytest.mark.parametrize("r", AC.gpu_rows(""), ids=AC.row_id)
def test_row(lib, r):
    plan, worst, bad = AC.run_row(lib, r)
    assert not bad, f"{r.id} {plan}: " + "; ".join(bad)


@pytest.mark.parametrize("env", [e for e in AC.ENVS if e])
def test_rows_that_need_a_knob_in_a_child_process(env):
    assert _STATE["abort"] is None, f"not started: an earlier child {_STATE['abort']}"
    rows = AC.gpu_rows(env)
    assert rows
    with tempfile.TemporaryDirectory() as tmp:
        report = os.path.join(tmp, "report.json")
        cmd = [sys.executable, os.path.join(ROOT, "tests", "_agg_worker.py"), report, env]
        try:
            p = subprocess.run(cmd, env=AC.child_env(env), cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _STATE["abort"] = f"with {AC.ENVS[env]} timed out after {CHILD_TIMEOUT} s"
            raise AssertionError(_STATE["abort"]) from None
        if p.returncode < 0 or p.returncode == 124 or p.returncode >= 128:
            _STATE["abort"] = f"with {AC.ENVS[env]} ended by a signal (exit status {p.returncode})"
            raise AssertionError(f"{_STATE['abort']}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        assert p.returncode == 0 and os.path.exists(report), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        with open(report) as f:
            rep = json.load(f)
    print(p.stdout[-6000:])
    assert [x["id"] for x in rep["rows"]] == [r.id for r in rows], "the child did not run every row of its knob setting"
    failed = [f"{x['id']}: {x['error']}" for x in rep["rows"] if not x["ok"]]
    assert not failed and rep["ok"], "\n".join(failed)
