"""The fused additive attention (dp_csr_gat_fwd / _bwd) next to the same result composed from the existing ops, next to a
copy of the bytes it must move, and in front of the CSR DiffPool training step.

    python tools/csr_gat_ab.py [--other-root DIR] [--rounds 5] [--iters 40] [--out FILE]

Op level (one child process): a 2^20-node ring lattice of degree 6 and the 5 748-node graph of tools/csr_edge_ops_ab.py
(DD's size and mean degree), H = 1, 4, 8.  `fused`: `ops.csr_gat_attention` forward, and forward + backward.  `composed`:
per head the torch gathers u[rows, h] + v[cols, h], `leaky_relu`, `ops.csr_edge_softmax`, then the mean of the heads.
`copy`: a device-to-device copy of the bytes the fused entries must move (each array once: forward 8 nnz + 4 n + 16 n H,
backward 16 nnz + 8 n + 32 n H), taken in the same run.  One event pair round ten calls, the median of 20 pairs.  The
peak of `torch.cuda.max_memory_allocated` over one forward + backward above what is allocated before it, for both routes:
their difference is what the fusion does not allocate.

Step level: each measurement is one child process, the SparseSoftPoolingGcnEncoder step of tools/csr_edge_ops_ab.py
(forward + link loss + backward) with `EdgeAttention(89, 16)` as it is (`softmax`) and with `score="additive", heads=4`
(`additive4`) in front, `--iters` timed steps behind 10 warm-up steps; the driver alternates the configurations round by
round and reports medians, spreads and the ratios paired per round.  With --other-root also `other data`: the `data` step
of another checkout of the project with its library built (the parent commit)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(fn, iters, reps=1):
    """Median over `iters` event pairs of the time of one call (`reps` back-to-back calls per pair)."""
    import torch
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times)


def _dd_graph():
    import numpy as np
    from graph_pooling_amd.sparse import CsrGraph
    n = 5748
    rng = np.random.default_rng(0)
    ring = np.arange(n)
    src = np.concatenate([ring, rng.integers(0, n, 3 * n // 2)])
    dst = np.concatenate([(ring + 1) % n, rng.integers(0, n, 3 * n // 2)])
    keep = src != dst
    return CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)


def worker(root, mode, iters):
    sys.path.insert(0, root)
    import torch
    from graph_pooling_amd import sparse
    from graph_pooling_amd.sparse import SparseSoftPoolingGcnEncoder

    feat = 89
    g = _dd_graph()
    torch.manual_seed(0)
    model = SparseSoftPoolingGcnEncoder(500, feat, 64, 64, 2, 3, 64, assign_ratio=0.1, num_pooling=1,
                                        linkpred=True).cuda()
    att = None
    if mode == "data":
        g = g.normalized()
    elif mode == "softmax":
        att = sparse.EdgeAttention(feat, 16, norm="softmax").cuda()
    else:
        att = sparse.EdgeAttention(feat, 16, score="additive", heads=4).cuda()
    x = torch.randn(g.n, feat, device="cuda")
    label = torch.tensor([1], device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        h = g
        if att is not None:
            att.zero_grad(set_to_none=True)
            h = att(x, g)
        loss = model.loss(model(x, h), label, h)
        loss.backward()

    for _ in range(10):
        step()
    torch.cuda.synchronize()
    print(f"MEDIAN_MS {_median_ms(step, iters):.4f}")


def op_level(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrGraph

    n = 1 << 20
    i = np.arange(n)
    src, dst = np.repeat(i, 3), (np.repeat(i, 3) + np.tile([1, 2, 3], n)) % n
    graphs = (("lattice 2^20 x 6", CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)), ("DD-sized 5748", _dd_graph()))
    for gname, g in graphs:
        g.mirror_perm                                        # built once on the host, outside every timing
        ip = g.indptr.cpu().numpy().astype(np.int64)
        rows = torch.from_numpy(np.repeat(np.arange(g.n), np.diff(ip))).cuda()
        cols = g.indices[:g.nnz].long()
        for H in (1, 4, 8):
            gen = torch.Generator().manual_seed(H)
            u = torch.randn(g.n, H, generator=gen).cuda().requires_grad_(True)
            v = torch.randn(g.n, H, generator=gen).cuda().requires_grad_(True)
            w = torch.randn(g.nnz, generator=gen).cuda()

            def fused():
                return ops.csr_gat_attention(u, v, g, 0.2)

            def composed():
                heads = [ops.csr_edge_softmax(torch.nn.functional.leaky_relu(u[rows, h] + v[cols, h], 0.2), g)
                         for h in range(H)]
                return torch.stack(heads).mean(0) if H > 1 else heads[0]

            def both(route):
                def run():
                    u.grad = v.grad = None
                    route().backward(w)
                return run

            def fwd_only(route):
                def run():
                    with torch.no_grad():
                        route()
                return run

            err = float((fused().detach() - composed().detach()).abs().max())
            res = {}
            for name, route in (("fused", fused), ("composed", composed)):
                for _ in range(3):
                    both(route)()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                both(route)()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                res[name] = (_median_ms(fwd_only(route), 20, reps=10), _median_ms(both(route), 20, reps=10), peak)
            fb, bb = 8 * g.nnz + 4 * g.n + 16 * g.n * H, 16 * g.nnz + 8 * g.n + 32 * g.n * H
            copies = []
            for nbytes in (fb, fb + bb):
                half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                dstb = torch.empty_like(half)
                for _ in range(3):
                    dstb.copy_(half)
                copies.append(_median_ms(lambda: dstb.copy_(half), 20, reps=10))
            (ff, fa, fp), (cf, ca, cp) = res["fused"], res["composed"]
            print(f"OP {gname} H={H}: forward fused {1e3 * ff:.1f} us, composed {1e3 * cf:.1f} us ({cf / ff:.2f}x), copy of "
                  f"{fb / 1e6:.2f} MB {1e3 * copies[0]:.1f} us; forward+backward fused {1e3 * fa:.1f} us, composed "
                  f"{1e3 * ca:.1f} us ({ca / fa:.2f}x), copy of {(fb + bb) / 1e6:.2f} MB {1e3 * copies[1]:.1f} us; peak memory "
                  f"above the inputs fused {fp / 1e6:.2f} MB, composed {cp / 1e6:.2f} MB (difference {(cp - fp) / 1e6:.2f} "
                  f"MB); max |fused - composed| {err:.2e}", flush=True)


def child(root, mode, iters):
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--mode", mode,
                           "--iters", str(iters)], check=True, capture_output=True, text=True, timeout=600, cwd=root)


def measure(root, mode, iters):
    out = child(root, mode, iters)
    for line in out.stdout.splitlines():
        if line.startswith("MEDIAN_MS"):
            return float(line.split()[1])
    raise RuntimeError(f"no result from the worker:\n{out.stdout}\n{out.stderr}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-root")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--mode", default="data", choices=["data", "softmax", "additive4", "op"])
    a = ap.parse_args()
    if a.worker:
        op_level(a.root) if a.mode == "op" else worker(a.root, a.mode, a.iters)
        return
    lines = ["op level: events round 10 calls, median of 20; fused = ops.csr_gat_attention, composed = per head gathers, "
             "leaky_relu, ops.csr_edge_softmax, mean"]
    lines += [l[len("OP "):] for l in child(ROOT, "op", 1).stdout.splitlines() if l.startswith("OP ")]
    print("\n".join(lines), flush=True)
    cfgs = [("data", ROOT, "data"), ("softmax", ROOT, "softmax"), ("additive4", ROOT, "additive4")]
    if a.other_root:                                     # another checkout runs its own copy of the worker's `data` mode
        cfgs.insert(0, ("other data", os.path.abspath(a.other_root), "data"))
    res = {name: [] for name, _, _ in cfgs}
    for r in range(a.rounds):
        for name, root, mode in cfgs:
            res[name].append(measure(root, mode, a.iters))
        print("round", r, {k: round(v[-1], 4) for k, v in res.items()}, flush=True)
    step = [f"CSR DiffPool step (forward + link loss + backward), 5 748 nodes, F = 89, H = 64, K_0 = 50; "
            f"{a.rounds} alternating rounds, median of {a.iters} steps per run, ms"]
    for name, v in res.items():
        step.append(f"{name:<18s} median {statistics.median(v):8.4f}   spread {min(v):8.4f} .. {max(v):8.4f}   runs "
                    + " ".join(f"{t:.4f}" for t in v))

    def ratio(x, y):
        q = [p / s for p, s in zip(res[x], res[y])]
        return f"{x} / {y}: median {statistics.median(q):.4f}   spread {min(q):.4f} .. {max(q):.4f} (paired per round)"
    if a.other_root:
        step.append(ratio("data", "other data"))
    step += [ratio("softmax", "data"), ratio("additive4", "data"), ratio("additive4", "softmax")]
    print("\n".join(step))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines + step) + "\n")


if __name__ == "__main__":
    main()
