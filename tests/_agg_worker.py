"""Child process of tests/test_agg_plan_cpu.py and tests/test_gpu_agg.py.  The library reads DP_AGG_WIDE and DP_AGG_RT
once per process, so the rows of tests/agg_cases.py that need one of them run here, in a fresh process that the parent
starts with the knob set:

    python tests/_agg_worker.py --plans ENV             no GPU: prints {row id: plan} of the rows of that knob setting
    python tests/_agg_worker.py REPORT.json ENV         runs those rows on the GPU (agg_cases.run_row)

ENV is a key of agg_cases.ENVS; the worker refuses to run when its environment is not that setting.  REPORT.json:
{"ok": bool, "rows": [{"id", "ok", "error", "worst", "seconds"}]}.  A library error ends the run at that row."""
import json
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_pooling_amd import _lib          # noqa: E402
from tests import agg_cases as AC           # noqa: E402


def _check_env(env):
    want = AC.ENVS[env]
    have = {k: os.environ[k] for k in AC.KNOBS if k in os.environ}
    assert have == want, f"knobs in the environment {have}, the rows of {env!r} need {want}"


def plans(env):
    lib = _lib.load()
    print(json.dumps({r.id: list(AC.plan_of(lib, r)) for r in AC.ROWS if r.env == env and r.kind != "pack"}))


def run(report, env):
    import torch
    lib = _lib.load()
    out = {"ok": True, "rows": []}
    fatal = False
    for r in AC.gpu_rows(env):
        t0 = time.monotonic()
        rec = {"id": r.id, "ok": True, "error": "", "worst": 0.0}
        fatal = False
        try:
            _, worst, bad = AC.run_row(lib, r)
            rec.update(ok=not bad, error="; ".join(bad)[-3000:], worst=worst if worst == worst else -1.0)
        except AssertionError as e:
            rec.update(ok=False, error=str(e)[-3000:])
        except Exception:                              # a library or runtime error: the process may be unusable
            rec.update(ok=False, error=traceback.format_exc()[-3000:])
            fatal = True
        rec["seconds"] = round(time.monotonic() - t0, 2)
        out["rows"].append(rec)
        out["ok"] = out["ok"] and rec["ok"]
        print(f"[agg-worker] {r.id}: {'ok' if rec['ok'] else 'FAILED ' + rec['error'][:300]} ({rec['seconds']} s)", flush=True)
        if fatal:
            break
    if not fatal:
        torch.cuda.synchronize()
    with open(report, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--plans":
        _check_env(sys.argv[2])
        plans(sys.argv[2])
    else:
        _check_env(sys.argv[2])
        run(sys.argv[1], sys.argv[2])
