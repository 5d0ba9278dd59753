"""A/B of the CSR DiffPool training step with and without edge weights, from alternating runs in fresh processes.

    python tools/csr_weights_ab.py [--other-root DIR] [--rounds 7] [--iters 40] [--out FILE]

Each measurement is one child process (its own HIP context): a 5 748-node graph of DD's size and mean degree, the
SparseSoftPoolingGcnEncoder step (forward + link loss + backward), `--iters` timed steps behind 10 warm-up steps, timed
with events; the child prints the median step.  The driver alternates the configurations round by round (A B C, A B C,
...) so drift of the machine lands on all of them alike, and reports per configuration the median over the rounds and
the spread (min .. max), plus the paired ratios per round.

Configurations: `unweighted` and `weighted` (the same graph, `.normalized()`) from this tree; with --other-root also
`other unweighted`: the same step from another checkout of the project with its library built (the parent commit), run
with that checkout's Python package."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(root, weighted, iters):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from graph_pooling_amd.sparse import CsrGraph, SparseSoftPoolingGcnEncoder

    n, feat = 5748, 89
    rng = np.random.default_rng(0)
    ring = np.arange(n)
    src = np.concatenate([ring, rng.integers(0, n, 3 * n // 2)])
    dst = np.concatenate([(ring + 1) % n, rng.integers(0, n, 3 * n // 2)])
    keep = src != dst
    g = CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)
    if weighted:
        g = g.normalized()
    torch.manual_seed(0)
    model = SparseSoftPoolingGcnEncoder(500, feat, 64, 64, 2, 3, 64, assign_ratio=0.1, num_pooling=1,
                                        linkpred=True).cuda()
    x = torch.randn(n, feat, device="cuda")
    label = torch.tensor([1], device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        loss = model.loss(model(x, g), label, g)
        loss.backward()

    for _ in range(10):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    print(f"MEDIAN_MS {statistics.median(times):.4f}")


def measure(root, weighted, iters):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--weighted",
                          str(int(weighted)), "--iters", str(iters)], check=True, capture_output=True, text=True,
                         timeout=300, cwd=root)
    for line in out.stdout.splitlines():
        if line.startswith("MEDIAN_MS"):
            return float(line.split()[1])
    raise RuntimeError(f"no result from the worker:\n{out.stdout}\n{out.stderr}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-root")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--weighted", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        worker(a.root, a.weighted, a.iters)
        return
    cfgs = [("unweighted", ROOT, 0), ("weighted", ROOT, 1)]
    if a.other_root:
        cfgs.insert(0, ("other unweighted", os.path.abspath(a.other_root), 0))
    res = {name: [] for name, _, _ in cfgs}
    for r in range(a.rounds):
        for name, root, w in cfgs:
            res[name].append(measure(root, w, a.iters))
        print("round", r, {k: round(v[-1], 4) for k, v in res.items()}, flush=True)
    lines = [f"CSR DiffPool step (forward + link loss + backward), 5 748 nodes, F = 89, H = 64, K_0 = 50; "
             f"{a.rounds} alternating rounds, median of {a.iters} steps per run, ms"]
    for name, v in res.items():
        lines.append(f"{name:<18s} median {statistics.median(v):8.4f}   spread {min(v):8.4f} .. {max(v):8.4f}   runs "
                     + " ".join(f"{t:.4f}" for t in v))

    def ratio(x, y):
        q = [p / s for p, s in zip(res[x], res[y])]
        return f"{x} / {y}: median {statistics.median(q):.4f}   spread {min(q):.4f} .. {max(q):.4f} (paired per round)"
    if a.other_root:
        lines.append(ratio("unweighted", "other unweighted"))
    lines.append(ratio("weighted", "unweighted"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
