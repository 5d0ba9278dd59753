"""Timing of the link-prediction loss on a CSR graph (dp_csr_linkpred_loss_fwd / bwd, encoders.py:1309-1331 without an
n x n adjacency) at four shapes, and at DD's largest graph against the dense entries it replaces there
(dp_linkpred_loss_fwd / bwd with B = 1, N = n on the densified 132 MB adjacency) — same process, alternating
repetitions, the margin being the spread of the dense pair's own repeated medians.

Algorithmic work of the dense term: forward n^2 K flops (half the tiles, 2 flops per multiply-add), backward 4 n^2 K
(recompute P, then E S_c).  The edge launches are timed by name in a profiled call, so their share is visible.

    PYTHONPATH=. python tools/csr_link_probe.py > profiles/csr_link_probe.txt"""
import hashlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.sparse import CsrGraph  # noqa: E402

lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
REPS = 7


def median_us(call, target_ms=200.0):
    """Event-timed median of single calls (at least 5, about target_ms of work), in microseconds."""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    iters = int(min(100, max(5, target_ms / max(e0.elapsed_time(e1), 1e-3))))
    times = []
    for _ in range(iters):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1000)
    return statistics.median(times), iters


def graph(n, deg, seed):
    """Symmetric random graph with ~deg neighbours per row."""
    rng = np.random.default_rng(seed)
    m = n * deg // 2
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = src != dst
    return CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)


def kernel_times(call):
    """Device time per kernel name of ONE profiled call, microseconds."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    tot = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            tot[ev.name] = tot.get(ev.name, 0.0) + t
    return tot


def shape(n, deg, K, compare_dense):
    g = graph(n, deg, n + K)
    nnz = g.indices.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    S = torch.softmax(2 * torch.randn(n, K, device="cuda", generator=gen), -1)
    dS, loss = torch.empty(n, K, device="cuda"), torch.empty(1, device="cuda")
    wsb = lib.dp_csr_linkpred_workspace_bytes(n, K)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    ip, ix = g.indptr.data_ptr(), g.indices.data_ptr()

    def fwd():
        _lib.check(lib.dp_csr_linkpred_loss_fwd(S.data_ptr(), K, ip, ix, loss.data_ptr(), n, K, ws.data_ptr(), wsb, st),
                   "dp_csr_linkpred_loss_fwd")

    def bwd():
        _lib.check(lib.dp_csr_linkpred_loss_bwd(S.data_ptr(), K, ip, ix, ip, ix, None, dS.data_ptr(), K, 0, n, K,
                                                ws.data_ptr(), wsb, st), "dp_csr_linkpred_loss_bwd")

    def both():
        fwd()
        bwd()

    print(f"n={n} K={K} nnz={nnz} (mean degree {nnz / n:.1f}); workspace {wsb / 1e6:.2f} MB "
          f"(an n x n fp32 adjacency: {n * n * 4 / 1e6:.0f} MB)")
    fu, fi = median_us(fwd)
    bu, bi = median_us(bwd)
    print(f"    dp_csr_linkpred_loss_fwd {fu:10.1f} us  ({fi} calls)   dense term {n * n * K / fu / 1e6:6.1f} algorithmic "
          "TFLOP/s if it were the whole call")
    print(f"    dp_csr_linkpred_loss_bwd {bu:10.1f} us  ({bi} calls)   dense term {4 * n * n * K / bu / 1e6:6.1f} "
          "algorithmic TFLOP/s if it were the whole call")
    kt = kernel_times(both)
    for name, t in sorted(kt.items(), key=lambda kv: -kv[1]):
        if "k_csr_link" in name:
            print(f"        {t:10.1f} us  {name[:100]}")
    edge = sum(t for k, t in kt.items() if "k_csr_link_edge" in k)
    dense = sum(t for k, t in kt.items() if "k_csr_link_dense" in k)
    print(f"    one profiled fwd + bwd: dense-term kernels {dense:.1f} us ({5 * n * n * K / max(dense, 1e-9) / 1e6:.1f} "
          f"algorithmic TFLOP/s), edge-term kernels {edge:.1f} us")
    if not compare_dense:
        return

    A = torch.zeros(n, n, device="cuda")
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (g.indptr[1:] - g.indptr[:-1]).long())
    A[rows, g.indices.long()] = 1.0
    dSd, lossd = torch.empty(n, K, device="cuda"), torch.empty(1, device="cuda")
    wsbd = lib.dp_linkpred_workspace_bytes(1, n, K)
    wsd = torch.empty(wsbd, device="cuda", dtype=torch.uint8)

    def dense_both():
        _lib.check(lib.dp_linkpred_loss_fwd(S.data_ptr(), A.data_ptr(), None, lossd.data_ptr(), 1, n, K, wsd.data_ptr(),
                                            wsbd, st), "dp_linkpred_loss_fwd")
        _lib.check(lib.dp_linkpred_loss_bwd(S.data_ptr(), A.data_ptr(), None, None, dSd.data_ptr(), 0, 1, n, K,
                                            wsd.data_ptr(), wsbd, st), "dp_linkpred_loss_bwd")

    both()
    dense_both()
    torch.cuda.synchronize()
    print(f"    results: loss csr {float(loss):.8f} dense {float(lossd):.8f}; dS max diff / max "
          f"{float((dS - dSd).abs().max() / dSd.abs().max()):.1e}")
    new, old = [], []
    for _ in range(REPS):                                   # alternating repetitions of the two pairs
        old.append(median_us(dense_both)[0])
        new.append(median_us(both)[0])
    spread = max(old) - min(old)
    print(f"    fwd + bwd, {REPS} alternating medians, us:")
    print("        dense dp_linkpred_loss_*   : " + " ".join(f"{t:8.1f}" for t in old))
    print("        csr   dp_csr_linkpred_loss_*: " + " ".join(f"{t:8.1f}" for t in new))
    mo, mn = statistics.median(old), statistics.median(new)
    verdict = "not slower" if mn <= mo + spread else "SLOWER"
    print(f"    median of medians: dense {mo:.1f} us, csr {mn:.1f} us; spread of the dense series {spread:.1f} us -> "
          f"the CSR pair is {verdict} than the dense pair (requirement: csr <= dense + spread)")


if __name__ == "__main__":
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    shape(5748, 5, 50, True)
    shape(16384, 10, 64, False)
    shape(65536, 10, 64, False)
    shape(65536, 10, 256, False)
