"""Child process of tests/test_gpu_head_grads_final.py: one training step of every case of
tests/head_grads_final_cases.py in THIS process's plan, written with torch.save as {case: {"ypred", gradients}}.
The plan knob DP_NO_HEAD_FOLD is read once when the library loads, hence the process of its own: with it set the
prediction-head backward runs as k_head_bwd and the step's final launch reduces the slabs only -- the independent
yardstick; without it (under a kernel trace) the run shows which kernels the folded plan launches.

    python tests/_head_grads_final_worker.py OUT.pt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import head_grads_final_cases as HC                       # noqa: E402


def main():
    out = {}
    for name, *_ in HC.CASES:
        model, _, x, adj, nn_, label = HC.build(name)
        model = model.cuda()
        y, _ = HC.step(model, x.cuda(), adj.cuda(), nn_, label.cuda())
        torch.cuda.synchronize()
        out[name] = HC.results(model, y)
    torch.save(out, sys.argv[1])
    print(f"{len(out)} cases, DP_NO_HEAD_FOLD={os.environ.get('DP_NO_HEAD_FOLD', '')!r}", flush=True)


if __name__ == "__main__":
    main()
