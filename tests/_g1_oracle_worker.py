"""The oracle's side of the G1 golden cases (tests/test_oracle_golden.py): oracle.graph_conv forward and backward on each
case's inputs, written to one .npz as <case>__y, <case>__gx, <case>__gadj, <case>__grad.<param>.

Run in a child process with MKL_CBWR=COMPATIBLE: MKL picks its float32 GEMM kernels by host CPU when it initialises, so
the same torch ops round alike on every x86-64 host only with the code path pinned before then — and G1's forward is
checked bit for bit against fixtures oracle/make_golden.py writes under the same setting.

    MKL_CBWR=COMPATIBLE python tests/_g1_oracle_worker.py OUT.npz CASE..."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import diffpool_oracle as O                               # noqa: E402


def main(out, cases):
    assert os.environ.get("MKL_CBWR") == "COMPATIBLE", "run with MKL_CBWR=COMPATIBLE (see the module docstring)"
    res = {}
    for name in cases:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)
        add_self, _, normalize = [bool(v) for v in z["cfg"]]
        P = {k[6:]: torch.from_numpy(z[k]).requires_grad_(True) for k in z.files if k.startswith("param.")}
        x = torch.from_numpy(z["x"]).requires_grad_(True)
        adj = torch.from_numpy(z["adj"]).requires_grad_(True)
        y = O.graph_conv(x, adj, P["weight"], P.get("bias"), add_self, normalize)
        (y * torch.from_numpy(z["gy"])).sum().backward()
        res.update({f"{name}__y": y, f"{name}__gx": x.grad, f"{name}__gadj": adj.grad})
        res.update({f"{name}__grad.{k}": v.grad for k, v in P.items()})
    np.savez(out, **{k: v.detach().numpy() for k, v in res.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
