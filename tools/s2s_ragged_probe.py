"""One torch.profiler step of SparseGcnSet2SetEncoder forward + loss + backward on RAGGED batches (CsrBatch), kernels by
device time, at the reference's default widths (hidden / output 20, three GraphConv layers: Set2Set width d = 60):

  1. the batch of tools/csr_batch_probe.py: B = 20 graphs of 30..5748 nodes (same seed), pad_to = 5748 — past the dense
     Set2Set kernels' 1024 rows, so only the ragged path runs it; the save / workspace bytes of the readout are printed;
  2. B = 20 graphs of at most 1000 nodes with pad_to = 1000, where the dense GcnSet2SetEncoder runs the same graphs
     padded: both are timed in this job.

No threshold: the output (profiles/s2s_ragged_probe.txt) is the record for whoever tunes this path next.

    PYTHONPATH=. python tools/s2s_ragged_probe.py"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from csr_batch_probe import sizes  # noqa: E402
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.encoders import GcnSet2SetEncoder  # noqa: E402
from graph_pooling_amd.sparse import CsrBatch, SparseGcnSet2SetEncoder  # noqa: E402

F_, H, E = 16, 20, 20


def edges(sz, deg=10, seed=1):
    rng = np.random.default_rng(seed)
    srcs, dsts = [], []
    for n in sz:
        m = int(n) * deg // 2
        s, d = rng.integers(0, n, m), rng.integers(0, n, m)
        keep = s != d
        srcs.append(s[keep])
        dsts.append(d[keep])
    return srcs, dsts


def timed(step, reps):
    step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(step, top=12):
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
    print(f"    device time of one profiled step: {total / 1e3:.3f} ms over {sum(v[1] for v in tot.values())} kernels; "
          "by time:")
    for name, (t, c) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:top]:
        print(f"    {t / 1e3:10.3f} ms  {100 * t / max(total, 1e-9):5.1f} %  x{c}  {name[:110]}")


def run(sz, pad_to, reps, dense_too):
    lib = _lib.load()
    srcs, dsts = edges(sz)
    g = CsrBatch.from_edge_lists(sz, srcs, dsts, "cuda", pad_to=pad_to)
    x = torch.randn(g.n_total, F_, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    label = torch.arange(g.num_graphs, device="cuda") % 2
    torch.manual_seed(0)
    model = SparseGcnSet2SetEncoder(F_, H, E, 2, 3, pred_hidden_dims=[50]).cuda()
    d = model.pred_input_dim
    off = g.node_off_host.ctypes.data
    sb = lib.dp_set2set_ragged_save_bytes(off, g.num_graphs, g.pad_to, d)
    wb = lib.dp_set2set_ragged_bwd_workspace_bytes(off, g.num_graphs, g.pad_to, d)

    def step():
        model.zero_grad(set_to_none=True)
        model.loss(model(x, g), label).backward()

    ms = timed(step, reps)
    print(f"B={g.num_graphs} sizes={sorted(int(s) for s in sz)} n_total={g.n_total} pad_to={g.pad_to} F={F_} hidden={H} "
          f"embedding={E} d={d}; Set2Set save {sb / 2 ** 20:.1f} MiB, backward workspace {wb / 2 ** 20:.1f} MiB "
          f"(2 x T x n_total floats = {2 * 4 * g.pad_to * g.n_total / 2 ** 20:.1f} MiB of them)")
    print(f"  ragged SparseGcnSet2SetEncoder: {ms:.3f} ms per step ({reps} steps, host launch time included)")
    profiled(step)
    if not dense_too:
        return
    P = g.pad_to
    adj = torch.zeros(len(sz), P, P, device="cuda")
    xd = torch.zeros(len(sz), P, F_, device="cuda")
    o = 0
    for b, n in enumerate(sz):
        s, t = torch.from_numpy(srcs[b]).cuda(), torch.from_numpy(dsts[b]).cuda()
        adj[b, s, t] = 1.0
        adj[b, t, s] = 1.0
        xd[b, :n] = x[o:o + n]
        o += int(n)
    dense = GcnSet2SetEncoder(F_, H, E, 2, 3, pred_hidden_dims=[50]).cuda()
    dense.load_state_dict(model.state_dict())
    nn_ = [int(n) for n in sz]

    def dstep():
        dense.zero_grad(set_to_none=True)
        dense.loss(dense(xd, adj, nn_), label).backward()

    ms = timed(dstep, reps)
    print(f"  dense GcnSet2SetEncoder on the same graphs padded to {P}: {ms:.3f} ms per step ({reps} steps)")
    profiled(dstep)


def main():
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    run(sizes(), None, 2, dense_too=False)
    run(sizes(hi=1000), 1000, 5, dense_too=True)


if __name__ == "__main__":
    main()
