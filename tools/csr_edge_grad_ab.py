"""A/B of the CSR DiffPool training step with and without a gradient to the edge weights, from alternating runs in fresh
processes.

    python tools/csr_edge_grad_ab.py [--other-root DIR] [--rounds 7] [--iters 40] [--out FILE]

Each measurement is one child process (its own HIP context): a 5 748-node graph of DD's size and mean degree, the
SparseSoftPoolingGcnEncoder step (forward + link loss + backward), `--iters` timed steps behind 10 warm-up steps, timed
with events; the child prints the median step.  The driver alternates the configurations round by round (A B C, A B C,
...) so drift of the machine lands on all of them alike, and reports per configuration the median over the rounds and
the spread (min .. max), plus the paired ratios per round.

Configurations: `data` (the graph `.normalized()`, its values plain data: the step of tools/csr_weights_ab.py's
`weighted`) and `grad` (the same values behind `with_values(v)`, `v.requires_grad`: three more GraphConv SDDMMs per
stack, one for the pooling, one for the link loss) from this tree; with --other-root also `other data`: the `data` step
from another checkout of the project with its library built (the parent commit), run with that checkout's Python
package.  After the rounds one more child profiles a single `grad` step with torch.profiler and reports the share of
the k_csr_sddmm launches in the step's kernel time, next to the gathers that move the same nnz x F bytes."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(root, grad, iters, profile=False):
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
    g = g.normalized()
    if grad:
        g = g.with_values(g.values.clone().requires_grad_(True))
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
    if profile:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
              and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        total = sum(e.device_time for e in ev)
        for key in ("k_csr_sddmm", "k_csr_agg_fwd"):
            sel = [e for e in ev if key in e.name]
            print(f"PROFILE {key}: {len(sel)} launches, {sum(e.device_time for e in sel):.1f} us of {total:.1f} us kernel "
                  f"time in {len(ev)} launches ({100.0 * sum(e.device_time for e in sel) / total:.2f} %)")
        return
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    print(f"MEDIAN_MS {statistics.median(times):.4f}")


def child(root, grad, iters, profile=False):
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--grad",
                           str(int(grad)), "--iters", str(iters)] + (["--profile"] if profile else []), check=True,
                          capture_output=True, text=True, timeout=300, cwd=root)


def measure(root, grad, iters):
    out = child(root, grad, iters)
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
    ap.add_argument("--grad", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(a.root, a.grad, a.iters, a.profile)
        return
    cfgs = [("data", ROOT, 0), ("grad", ROOT, 1)]
    if a.other_root:
        cfgs.insert(0, ("other data", os.path.abspath(a.other_root), 0))
    res = {name: [] for name, _, _ in cfgs}
    for r in range(a.rounds):
        for name, root, w in cfgs:
            res[name].append(measure(root, w, a.iters))
        print("round", r, {k: round(v[-1], 4) for k, v in res.items()}, flush=True)
    lines = [f"CSR DiffPool step (forward + link loss + backward) on D^-1/2 A D^-1/2, 5 748 nodes, F = 89, H = 64, K_0 = 50; "
             f"{a.rounds} alternating rounds, median of {a.iters} steps per run, ms"]
    for name, v in res.items():
        lines.append(f"{name:<18s} median {statistics.median(v):8.4f}   spread {min(v):8.4f} .. {max(v):8.4f}   runs "
                     + " ".join(f"{t:.4f}" for t in v))

    def ratio(x, y):
        q = [p / s for p, s in zip(res[x], res[y])]
        return f"{x} / {y}: median {statistics.median(q):.4f}   spread {min(q):.4f} .. {max(q):.4f} (paired per round)"
    if a.other_root:
        lines.append(ratio("data", "other data"))
    lines.append(ratio("grad", "data"))
    lines.append("one profiled `grad` step:")
    lines += [l[len("PROFILE "):] for l in child(ROOT, 1, 1, profile=True).stdout.splitlines() if l.startswith("PROFILE ")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
