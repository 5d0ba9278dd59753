"""Measurements of the Frobenius link entries (dp_frob_link_* / dp_csr_frob_link_*) on the GPU.

  PYTHONPATH=. python tools/frob_link_probe.py anchor > profiles/frob_link_fp64_anchor.txt
  PYTHONPATH=. python tools/frob_link_probe.py time   > profiles/frob_link_probe.txt

`anchor` runs the cases of tests/test_gpu_frob_link.py (their checks included) and prints, per case, the largest
|error| / bound the forward and the backward reached against the fp64 reference.
`time` times forward + backward of the new CSR term against the existing CSR cross-entropy link term of the same build
(dp_csr_linkpred_loss_*) at n = 5 748 (K 50 and 64) and n = 65 536 (K 64), alone on a ring lattice of 2^20 nodes (K 16),
and the dense entries at the DD shape: REPS alternating medians of event-timed calls, with the spread of each series."""
import hashlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.sparse import CsrGraph  # noqa: E402

REPS = 5


def anchor():
    from tests import frob_link_cases as FC
    from tests import test_gpu_frob_link as T
    for K in FC.K_CASES:
        T.test_dense_every_k_shape_and_mask_fp32_and_packed(K)
        T.test_csr_every_k(K)
        T.test_ragged_batch_every_k(K)
    for kind in ("weighted", "asymmetric", "weighted_asymmetric"):
        T.test_dense_fp32_entry_takes_weighted_and_asymmetric_adjacencies(kind)
    for n in (1, T.SLAB - 1, T.SLAB, T.SLAB + 1, 2 * T.SLAB + 1):
        T.test_csr_slab_edges(n)
    for shape in ("isolated_node", "directed", "self_loops", "no_edges"):
        T.test_csr_graph_shapes(shape)
    for directed in (False, True):
        T.test_ragged_batch_across_slab_edges(directed)
    T.test_ring_lattice_of_a_million_nodes()
    print("largest |error| / bound per case (bounds: tests/frob_link_cases.py, C_FWD = D + 4, C_BWD = max(K, D) + 4, "
          "u = 2^-24)")
    print("backward, accumulate = 1: the bound also holds the rounding of fl(old + d), u |old + d| with old ~ N(0, 1) far "
          "above d, so that ratio sits close to 1 by the nature of a rounding unit")
    print(f"{'case':44s} {'forward':>10s} {'backward':>10s} {'bwd acc=1':>10s}")
    worst = [0.0, 0.0, 0.0]
    for case, r in T.RATIOS.items():
        worst = [max(a, b) for a, b in zip(worst, r)]
        print(f"{case:44s} {r[0]:10.4f} {r[1]:10.4f} {r[2]:10.4f}")
    print(f"{'largest':44s} {worst[0]:10.4f} {worst[1]:10.4f} {worst[2]:10.4f}")


def median_us(call, target_ms=100.0):
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
    return statistics.median(times)


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


def show_kernels(call):
    for name, t in sorted(kernel_times(call).items(), key=lambda kv: -kv[1]):
        print(f"            {t:9.1f} us  {name[:96]}")


def series(call):
    return [median_us(call) for _ in range(REPS)]


def show(name, xs):
    print(f"        {name:34s}: " + " ".join(f"{t:9.1f}" for t in xs) +
          f"   median {statistics.median(xs):9.1f} us, spread {max(xs) - min(xs):.1f} us")


def csr_shape(lib, st, g, n, K, compare):
    nnz = int(g.indptr[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    S = torch.softmax(2 * torch.randn(n, K, device="cuda", generator=gen), -1)
    dS, out = torch.empty(n, K, device="cuda"), torch.empty(2, device="cuda")
    W, G = torch.empty(n, K, device="cuda"), torch.empty(K, K, device="cuda")
    wsb = lib.dp_csr_frob_link_workspace_bytes(n, 1, K)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    ip, ix = g.indptr.data_ptr(), g.indices.data_ptr()

    def frob():
        _lib.check(lib.dp_csr_frob_link_fwd(S.data_ptr(), K, ip, ix, None, None, None, W.data_ptr(), G.data_ptr(),
                                            out.data_ptr(), None, n, K, ws.data_ptr(), wsb, st), "dp_csr_frob_link_fwd")
        _lib.check(lib.dp_csr_frob_link_bwd(S.data_ptr(), K, W.data_ptr(), G.data_ptr(), None, None, dS.data_ptr(), K, 0,
                                            1, n, K, st), "dp_csr_frob_link_bwd")

    print(f"n={n} K={K} nnz={nnz} (mean degree {nnz / n:.1f}); Frobenius workspace {wsb / 1e6:.2f} MB + W {n * K * 4 / 1e6:.2f}"
          f" MB (an n x n fp32 adjacency: {n * n * 4 / 1e6:.0f} MB)")
    print(f"    fwd + bwd, {REPS} medians each, us:")
    if not compare:
        show("frobenius dp_csr_frob_link_*", series(frob))
        print("    one profiled fwd + bwd, per kernel:")
        show_kernels(frob)
        return
    wsbc = lib.dp_csr_linkpred_workspace_bytes(n, K)
    wsc = torch.empty(wsbc, device="cuda", dtype=torch.uint8)

    def bce():
        _lib.check(lib.dp_csr_linkpred_loss_fwd(S.data_ptr(), K, ip, ix, out.data_ptr() + 4, n, K, wsc.data_ptr(), wsbc,
                                                st), "dp_csr_linkpred_loss_fwd")
        _lib.check(lib.dp_csr_linkpred_loss_bwd(S.data_ptr(), K, ip, ix, ip, ix, None, dS.data_ptr(), K, 0, n, K,
                                                wsc.data_ptr(), wsbc, st), "dp_csr_linkpred_loss_bwd")

    new, old = [], []
    for _ in range(REPS):                                   # alternating repetitions of the two pairs
        old.append(median_us(bce))
        new.append(median_us(frob))
    show("cross-entropy dp_csr_linkpred_loss_*", old)
    show("frobenius     dp_csr_frob_link_*", new)
    print(f"    ratio of the medians: {statistics.median(old) / statistics.median(new):.1f}x")
    print("    one profiled fwd + bwd of the Frobenius term, per kernel:")
    show_kernels(frob)


def dense_shape(lib, st, B, N, K):
    gen = torch.Generator(device="cuda").manual_seed(0)
    S = torch.softmax(2 * torch.randn(B, N, K, device="cuda", generator=gen), -1)
    A = (torch.rand(B, N, N, device="cuda", generator=gen) < 0.02).float()
    A = torch.maximum(A, A.transpose(1, 2)).contiguous()
    nn = torch.randint(N // 2, N + 1, (B,), device="cuda", dtype=torch.int32, generator=gen)
    dS, out = torch.empty_like(S), torch.empty(2, device="cuda")
    W, G = torch.empty_like(S), torch.empty(B, K, K, device="cuda")
    wsb = lib.dp_frob_link_workspace_bytes(B, N, K)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    wsbl = lib.dp_linkpred_workspace_bytes(B, N, K)
    wsl = torch.empty(wsbl, device="cuda", dtype=torch.uint8)

    def frob():
        _lib.check(lib.dp_frob_link_fwd(S.data_ptr(), K, A.data_ptr(), nn.data_ptr(), None, W.data_ptr(), G.data_ptr(),
                                        out.data_ptr(), None, B, N, K, ws.data_ptr(), wsb, st), "dp_frob_link_fwd")
        _lib.check(lib.dp_frob_link_bwd(S.data_ptr(), K, W.data_ptr(), G.data_ptr(), nn.data_ptr(), None, None,
                                        dS.data_ptr(), K, 0, B, N, K, st), "dp_frob_link_bwd")

    def bce():
        _lib.check(lib.dp_linkpred_loss_fwd(S.data_ptr(), A.data_ptr(), nn.data_ptr(), out.data_ptr() + 4, B, N, K,
                                            wsl.data_ptr(), wsbl, st), "dp_linkpred_loss_fwd")
        _lib.check(lib.dp_linkpred_loss_bwd(S.data_ptr(), A.data_ptr(), nn.data_ptr(), None, dS.data_ptr(), 0, B, N, K,
                                            wsl.data_ptr(), wsbl, st), "dp_linkpred_loss_bwd")

    print(f"dense B={B} N={N} K={K}; Frobenius workspace {wsb / 1e6:.2f} MB")
    print(f"    fwd + bwd, {REPS} medians each, us:")
    new, old = [], []
    for _ in range(REPS):
        old.append(median_us(bce))
        new.append(median_us(frob))
    show("cross-entropy dp_linkpred_loss_*", old)
    show("frobenius     dp_frob_link_*", new)
    print("    one profiled fwd + bwd of the Frobenius term, per kernel:")
    show_kernels(frob)


def random_graph(n, deg, seed):
    rng = np.random.default_rng(seed)
    m = n * deg // 2
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = src != dst
    return CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)


def time_():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    csr_shape(lib, st, random_graph(5748, 5, 1), 5748, 50, True)
    csr_shape(lib, st, random_graph(5748, 5, 2), 5748, 64, True)
    csr_shape(lib, st, random_graph(65536, 10, 3), 65536, 64, True)
    n = 1 << 20
    i = torch.arange(n, device="cuda")[:, None]
    cols = torch.sort((i + torch.tensor([-2, -1, 1, 2], device="cuda")[None, :]) % n, dim=1).values
    ring = CsrGraph((torch.arange(n + 1, device="cuda") * 4).int(), cols.reshape(-1).int())
    csr_shape(lib, st, ring, n, 16, False)
    dense_shape(lib, st, 20, 500, 50)


if __name__ == "__main__":
    {"anchor": anchor, "time": time_}[sys.argv[1] if len(sys.argv) > 1 else "time"]()
