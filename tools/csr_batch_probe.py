"""One torch.profiler step of SparseSoftPoolingGcnEncoder forward + loss + backward on a RAGGED batch (CsrBatch), kernels
by device time.  B = 20 graphs whose sizes are drawn with a fixed seed from 30..5748 (log-uniform, so most are small and
a few large, the largest pinned at DD's 5 748), degree ~10; widths as in DESIGN.md §9 item 6 (F 16, hidden / embedding
32, K_0 64, K_1 6, D 96), linkpred on.  No threshold: the output (profiles/csr_batch_probe.txt) is the record for whoever
tunes this path next.

    PYTHONPATH=. python tools/csr_batch_probe.py"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.sparse import CsrBatch, SparseSoftPoolingGcnEncoder  # noqa: E402


def sizes(b=20, lo=30, hi=5748, seed=0):
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), b)).astype(np.int64)
    s[int(np.argmax(s))] = hi
    return s


def batch(sz, deg=10, seed=1):
    rng = np.random.default_rng(seed)
    srcs, dsts = [], []
    for n in sz:
        m = int(n) * deg // 2
        s, d = rng.integers(0, n, m), rng.integers(0, n, m)
        keep = s != d
        srcs.append(s[keep])
        dsts.append(d[keep])
    return CsrBatch.from_edge_lists(sz, srcs, dsts, "cuda")


def main():
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    F_, H, E = 16, 32, 32
    sz = sizes()
    g = batch(sz)
    x = torch.randn(g.n_total, F_, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    label = torch.arange(g.num_graphs, device="cuda") % 2
    for linkpred in (False, True):
        model = SparseSoftPoolingGcnEncoder(640, F_, H, E, 2, 3, H, assign_ratio=0.1, num_pooling=2,
                                            linkpred=linkpred).cuda()

        def step():
            model.zero_grad(set_to_none=True)
            loss = model.loss(model(x, g), label, g)
            loss.backward()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            step()
        e1.record()
        e1.synchronize()
        print(f"B={g.num_graphs} sizes={sorted(sz.tolist())} n_total={g.n_total} nnz={int(g.indptr[-1])} F={F_} "
              f"hidden={H} embedding={E} K_0={model.assign_dims[0]} K_1={model.assign_dims[1]} "
              f"D={model.pred_input_dim} linkpred={linkpred}: {e0.elapsed_time(e1) / 10:.3f} ms per step (10 steps, "
              "host launch time included)")
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        tot = {}
        for ev in prof.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA:
                t = tot.setdefault(ev.name, [0.0, 0])
                t[0] += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                t[1] += 1
        total = sum(v[0] for v in tot.values())
        print(f"    device time of one profiled step: {total / 1e3:.3f} ms over {sum(v[1] for v in tot.values())} "
              "kernels; by time:")
        for name, (t, c) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:14]:
            print(f"    {t / 1e3:8.3f} ms  {100 * t / max(total, 1e-9):5.1f} %  x{c}  {name[:110]}")


if __name__ == "__main__":
    main()
