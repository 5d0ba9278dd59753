"""Timing of the level-0 pooling on a CSR graph (dp_csr_pool_fwd / bwd: X' = S^T Z, A' = S^T A S, encoders.py:1278-1279)
against the composition it replaces — dp_csr_aggregate(S) into the first K columns of [A S | Z] followed by one
dp_bgemm_f32 S^T [A S | Z] (transA; Z sits in the last D columns of that buffer from the start, uncounted) — plus one
whole SparseSoftPoolingGcnEncoder forward + backward at n = 2^20 and its three most expensive kernels.

Effective bytes = streamed S (n K 4) + Z (n D 4) + CSR ((n + 1 + nnz) 4) + gathered rows (nnz K 4).  "Effective":
gathered rows of S may be served by L2 / MALL, so the figure can exceed what HBM moved.

    PYTHONPATH=. python tools/csr_pool_probe.py"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.sparse import CsrGraph, SparseSoftPoolingGcnEncoder  # noqa: E402

lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream


def timed(call, target_ms=300.0):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    once = max(e0.elapsed_time(e1), 1e-3)
    iters = int(min(200, max(5, target_ms / once)))
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters, iters


def graph(n, deg, seed):
    """Symmetric random graph with ~deg neighbours per row (deg / 2 random edges per node, both directions)."""
    rng = np.random.default_rng(seed)
    m = n * deg // 2
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = src != dst
    return CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)


def shape(name, n, deg, K, D):
    g = graph(n, deg, n + K)
    nnz = g.indices.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    S = torch.rand(n, K, device="cuda", generator=gen)
    Z = torch.rand(n, D, device="cuda", generator=gen)
    Xp, Ap = torch.empty(K, D, device="cuda"), torch.empty(K, K, device="cuda")
    dXp, dAp = torch.randn(K, D, device="cuda", generator=gen), torch.randn(K, K, device="cuda", generator=gen)
    dS, dZ = torch.empty(n, K, device="cuda"), torch.zeros(n, D, device="cuda")
    wsb = lib.dp_csr_pool_workspace_bytes(n, K, D)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    ip, ix = g.indptr.data_ptr(), g.indices.data_ptr()

    def fwd():
        _lib.check(lib.dp_csr_pool_fwd(S.data_ptr(), K, Z.data_ptr(), D, ip, ix, Xp.data_ptr(), Ap.data_ptr(), n, K, D,
                                       ws.data_ptr(), wsb, st), "dp_csr_pool_fwd")

    def bwd():
        _lib.check(lib.dp_csr_pool_bwd(S.data_ptr(), K, Z.data_ptr(), D, ip, ix, ip, ix, dXp.data_ptr(), dAp.data_ptr(),
                                       dS.data_ptr(), K, dZ.data_ptr(), D, n, K, D, ws.data_ptr(), wsb, st),
                   "dp_csr_pool_bwd")

    W = torch.empty(n, K + D, device="cuda")
    W[:, K:] = Z
    C = torch.empty(K, K + D, device="cuda")

    def composed():
        _lib.check(lib.dp_csr_aggregate(S.data_ptr(), K, ip, ix, W.data_ptr(), K + D, n, K, 0, 0.0, st),
                   "dp_csr_aggregate")
        _lib.check(lib.dp_bgemm_f32(S.data_ptr(), W.data_ptr(), C.data_ptr(), None, 1, K, K + D, n, K, K + D, K + D,
                                    0, 0, 0, 1, 0, 1.0, 0.0, 0, st), "dp_bgemm_f32")

    fwd()
    composed()
    torch.cuda.synchronize()
    err = max(float((C[:, :K] - Ap).abs().max() / Ap.abs().max()), float((C[:, K:] - Xp).abs().max() / Xp.abs().max()))
    eff = (n * K + n * D + n + 1 + nnz + nnz * K) * 4
    print(f"{name}: n={n} nnz={nnz} K={K} D={D}  (fused vs composed results: max rel diff {err:.1e})")
    for label, call in (("dp_csr_pool_fwd", fwd), ("composition agg+bgemm", composed), ("dp_csr_pool_bwd", bwd)):
        us, it = timed(call)
        print(f"    {label:24s} {us:10.1f} us  {eff / us / 1e3:8.1f} GB/s effective   ({it} iterations)")


def model_profile(n=1 << 20):
    F_, H, E = 16, 32, 32
    g = graph(n, 10, 1)
    x = torch.randn(n, F_, device="cuda")
    model = SparseSoftPoolingGcnEncoder(640, F_, H, E, 2, 3, H, assign_ratio=0.1, num_pooling=2,
                                        linkpred=False).cuda()
    label = torch.tensor([1], device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        loss = model.loss(model(x, g), label)
        loss.backward()

    us, it = timed(step, 1000.0)
    print(f"SparseSoftPoolingGcnEncoder forward + backward: n={n} nnz={g.indices.numel()} F={F_} hidden={H} "
          f"embedding={E} K_0={model.assign_dims[0]} K_1={model.assign_dims[1]} D={model.pred_input_dim}: "
          f"{us / 1e3:.2f} ms per step ({it} steps)")
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
    print(f"    device time of one profiled step: {total / 1e3:.2f} ms over {sum(v[1] for v in tot.values())} kernels; "
          "three most expensive:")
    for name, (t, c) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:3]:
        print(f"    {t / 1e3:8.3f} ms  {100 * t / max(total, 1e-9):5.1f} %  x{c}  {name[:110]}")


if __name__ == "__main__":
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    shape("DD largest graph", 5748, 5, 50, 60)
    shape("2^20 nodes", 1 << 20, 10, 64, 96)
    shape("2^20 nodes, wide", 1 << 20, 10, 256, 256)
    model_profile()
