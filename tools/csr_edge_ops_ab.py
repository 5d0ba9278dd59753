"""A/B of the CSR DiffPool training step with learned edge weights in front (`EdgeAttention`), from alternating runs in
fresh processes, one profiled step per attention form, and the new kernels on a large lattice next to a copy.

    python tools/csr_edge_ops_ab.py [--other-root DIR] [--rounds 5] [--iters 40] [--out FILE]

Each measurement is one child process (its own HIP context): the 5 748-node graph of tools/csr_edge_grad_ab.py (DD's
size and mean degree), the SparseSoftPoolingGcnEncoder step (forward + link loss + backward), `--iters` timed steps behind
10 warm-up steps, timed with events; the child prints the median step.  The driver alternates the configurations round
by round so drift of the machine lands on all of them alike, and reports per configuration the median over the rounds
and the spread, plus the paired ratios per round.

Configurations: `data` (the graph `.normalized()`, its values plain data), `softmax` and `sym` (`EdgeAttention(89, 16,
norm)` in front of the same model, its projections trained through the step) from this tree; with --other-root also
`other data`: the `data` step from another checkout of the project with its library built (the parent commit), run with
that checkout's Python package.  After the rounds one child per attention form profiles a single step with
torch.profiler and reports the k_edge_* launches next to the k_csr_agg_fwd and k_csr_sddmm launches of that step, and one
more child times every new entry on a 2^20-node ring lattice of degree 6 (one event pair round ten calls, median of 20
pairs) next to a device-to-device copy of the bytes the entry moves, from the same run."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("k_edge_softmax_fwd", "k_edge_softmax_bwd", "k_edge_sym_rdeg", "k_edge_sym_scale", "k_edge_sym_gdeg",
        "k_edge_sym_dvalues", "k_csr_sddmm", "k_csr_agg_fwd")


def _median_ms(fn, iters, reps=1):
    """Median over `iters` event pairs of the time of one call (`reps` back-to-back calls per pair, for short kernels)."""
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


def worker(root, mode, iters, profile=False):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from graph_pooling_amd import sparse
    from graph_pooling_amd.sparse import CsrGraph, SparseSoftPoolingGcnEncoder

    n, feat = 5748, 89
    rng = np.random.default_rng(0)
    ring = np.arange(n)
    src = np.concatenate([ring, rng.integers(0, n, 3 * n // 2)])
    dst = np.concatenate([(ring + 1) % n, rng.integers(0, n, 3 * n // 2)])
    keep = src != dst
    g = CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)
    torch.manual_seed(0)
    model = SparseSoftPoolingGcnEncoder(500, feat, 64, 64, 2, 3, 64, assign_ratio=0.1, num_pooling=1,
                                        linkpred=True).cuda()
    att = None
    if mode == "data":
        g = g.normalized()
    else:
        att = sparse.EdgeAttention(feat, 16, norm=mode).cuda()
    x = torch.randn(n, feat, device="cuda")
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
    if profile:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
              and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        total = sum(e.device_time for e in ev)
        for key in KEYS:
            sel = [e for e in ev if key in e.name]
            if sel:
                t = sum(e.device_time for e in sel)
                print(f"PROFILE {mode}: {key}: {len(sel)} launches, {t:.1f} us of {total:.1f} us kernel time in {len(ev)} "
                      f"launches ({100.0 * t / total:.2f} %)")
        return
    print(f"MEDIAN_MS {_median_ms(step, iters):.4f}")


def lattice(root):
    """Every new entry on a 2^20-node ring lattice of degree 6 (symmetric weights), next to a device-to-device copy of
    the bytes it moves (compulsory traffic: each array once, the rdeg / gdeg gathers as one pass over [n])."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from graph_pooling_amd import _lib
    from graph_pooling_amd.sparse import CsrGraph

    n = 1 << 20
    i = np.arange(n)
    src, dst = np.repeat(i, 3), (np.repeat(i, 3) + np.tile([1, 2, 3], n)) % n
    w = np.random.default_rng(0).uniform(0.5, 1.5, src.size).astype(np.float32)
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True, weight=w)
    nnz = g.nnz
    lib, st = _lib.load(), _lib.current_stream()
    f = lambda k: torch.rand(k, device="cuda")
    s, dout, out, ds, rdeg, gdeg = f(nnz), f(nnz), f(nnz), f(nnz), f(n), f(n)
    ip, ix, v, mir = g.indptr.data_ptr(), g.indices.data_ptr(), g.values.data_ptr(), g.mirror_perm.data_ptr()
    entries = {
        "dp_csr_edge_softmax_fwd": (8 * nnz + 4 * n, lambda: lib.dp_csr_edge_softmax_fwd(
            s.data_ptr(), ip, out.data_ptr(), n, nnz, st)),
        "dp_csr_edge_softmax_bwd": (12 * nnz + 4 * n, lambda: lib.dp_csr_edge_softmax_bwd(
            out.data_ptr(), dout.data_ptr(), ip, ds.data_ptr(), n, nnz, st)),
        "dp_csr_sym_norm_fwd": (16 * nnz + 20 * n, lambda: lib.dp_csr_sym_norm_fwd(
            ip, ix, v, ip, ix, None, rdeg.data_ptr(), out.data_ptr(), n, nnz, st)),
        "dp_csr_sym_norm_bwd": (32 * nnz + 24 * n, lambda: lib.dp_csr_sym_norm_bwd(
            ip, ix, v, ip, ix, mir, rdeg.data_ptr(), dout.data_ptr(), gdeg.data_ptr(), ds.data_ptr(), n, nnz, st)),
    }
    lib.dp_csr_sym_norm_fwd(ip, ix, v, ip, ix, None, rdeg.data_ptr(), out.data_ptr(), n, nnz, st)      # a real rdeg
    for name, (nbytes, call) in entries.items():
        half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dstb = torch.empty_like(half)
        for _ in range(3):
            _lib.check(call(), name)
            dstb.copy_(half)
        t, c = _median_ms(call, 20, reps=10), _median_ms(lambda: dstb.copy_(half), 20, reps=10)
        print(f"LATTICE {name}: {1e3 * t:.1f} us for {nbytes / 1e6:.1f} MB ({nbytes / t / 1e6:.0f} GB/s); a copy of the same "
              f"bytes {1e3 * c:.1f} us ({nbytes / c / 1e6:.0f} GB/s); ratio {t / c:.2f}")


def child(root, mode, iters, profile=False):
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--mode", mode,
                           "--iters", str(iters)] + (["--profile"] if profile else []), check=True,
                          capture_output=True, text=True, timeout=300, cwd=root)


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
    ap.add_argument("--mode", default="data", choices=["data", "softmax", "sym", "lattice"])
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.worker:
        lattice(a.root) if a.mode == "lattice" else worker(a.root, a.mode, a.iters, a.profile)
        return
    cfgs = [("data", ROOT, "data"), ("softmax", ROOT, "softmax"), ("sym", ROOT, "sym")]
    if a.other_root:
        cfgs.insert(0, ("other data", os.path.abspath(a.other_root), "data"))
    res = {name: [] for name, _, _ in cfgs}
    for r in range(a.rounds):
        for name, root, mode in cfgs:
            res[name].append(measure(root, mode, a.iters))
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
        lines.append(ratio("data", "other data"))
    lines += [ratio("softmax", "data"), ratio("sym", "data")]
    lines.append("one profiled step per attention form:")
    for mode in ("softmax", "sym"):
        lines += [l[len("PROFILE "):] for l in child(ROOT, mode, 1, profile=True).stdout.splitlines()
                  if l.startswith("PROFILE ")]
    lines.append("the entries on a 2^20-node ring lattice of degree 6 (events round 10 calls, median of 20):")
    lines += [l[len("LATTICE "):] for l in child(ROOT, "lattice", 1).stdout.splitlines() if l.startswith("LATTICE ")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
