"""Child process of tests/test_gpu_head.py: one training step of every case of tests/head_cases.py in THIS process's
plan, written with torch.save as {"order": [names], "cases": {name: tensors of head_cases.results}, "seconds": {name: s},
"error": text or None}.  The plan knob DP_NO_HEAD_FOLD is read once when the library loads, hence the process of its
own: with it set every case whose head backward folds into the last level's kernel runs k_head_bwd instead.  --reverse
runs the table last case first (the parent compares that run with its own, bit for bit: nothing may leak from one launch
geometry into the next).  Before each case the worker drains the stream and launches torch.cuda._sleep as a marker, so
that the parent can split the kernel trace per case (the convention of tests/_plan_worker.py).

    python tests/_head_worker.py OUT.pt [--reverse]"""
import os
import sys
import time
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import head_cases as HC                                   # noqa: E402

MARKER_CYCLES = 1000


def main():
    names = list(reversed(HC.NAMES)) if "--reverse" in sys.argv[2:] else list(HC.NAMES)
    out = {"order": [], "cases": {}, "seconds": {}, "error": None}
    for name in names:
        c = HC.CASE[name]
        torch.cuda.synchronize()
        torch.cuda._sleep(MARKER_CYCLES)                 # the parent's per-case boundary in the kernel trace
        torch.cuda.synchronize()
        t0 = time.monotonic()
        out["order"].append(name)
        try:
            model, _, x, adj, nn_, label = HC.build(name)
            model = model.cuda()
            y, _ = HC.step(model, c, x.cuda(), adj.cuda(), nn_, label.cuda())
            torch.cuda.synchronize()
            out["cases"][name] = HC.results(model, c, y)
        except Exception:                                # a library error: stop here, the process may be unusable
            out["error"] = f"{name}: {traceback.format_exc()[-3000:]}"
            break
        out["seconds"][name] = round(time.monotonic() - t0, 3)
    torch.save(out, sys.argv[1])
    print(f"{len(out['cases'])} cases, DP_NO_HEAD_FOLD={os.environ.get('DP_NO_HEAD_FOLD', '')!r}, "
          f"error: {out['error']}", flush=True)


if __name__ == "__main__":
    main()
