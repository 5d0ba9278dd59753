"""The fused sampled neighbour mean (`ops.csr_sample_mean`, dp_csr_sample_mean_fwd / _bwd) next to (a) the host-sampled
`MeanAggregator.forward` + backward on the same neighbour sets and (b) the unsampled `dp_mean_aggregate_fwd` / `_bwd` on
the same CSR.

    python tools/csr_sample_ab.py [--out FILE] [--log2n 16] [--rounds 9]

A ring lattice of 2^16 nodes and degree 32 (every node joined to the 16 nodes on either side), F = 64, k = 10.  `fused`:
forward + backward of `ops.csr_sample_mean` (self_mode none, every node a target).  `host`: `MeanAggregator.forward(nodes,
to_neighs, num_sample=10)` + backward with the host sampling (sorted + random.sample per node, the unique-node dict, the
two host-to-device copies) inside the timed window, one call per round.  `unsampled`: `aggregators.mean_aggregate` on the
whole CSR + backward (its backward scatters with atomics into a zero-filled table).  The three are timed in ALTERNATING
rounds in one process — a host clock round work that ends in a device synchronise, `calls` calls per window — and the
medians over the rounds are reported; every raw window is printed."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import numpy as np
    import torch
    from graph_pooling_amd import ops
    from graph_pooling_amd.aggregators import MeanAggregator, mean_aggregate
    from graph_pooling_amd.sparse import CsrGraph
    n, half, F, k = 1 << a.log2n, 16, 64, 10
    i = np.arange(n)
    src = np.repeat(i, half)
    dst = (src + np.tile(np.arange(1, half + 1), n)) % n
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    g.indptr_t, g.indices_t
    assert g.nnz == 2 * half * n
    ip, ix = g.indptr.cpu().numpy(), g.indices.cpu().numpy()
    to_neighs = [set(ix[ip[r]:ip[r + 1]].tolist()) for r in range(n)]
    nodes = list(range(n))
    x = torch.randn(n, F, device="cuda", requires_grad=True)
    dy = torch.randn(n, F, device="cuda")
    agg = MeanAggregator(lambda ids: x[ids], cuda=True)
    step = [0]

    def fused():
        x.grad = None
        step[0] += 1
        ops.csr_sample_mean(x, g, k, step[0]).backward(dy)

    def host():
        x.grad = None
        agg(nodes, to_neighs, num_sample=k).backward(dy)

    def unsampled():
        x.grad = None
        mean_aggregate(x, g.indptr, g.indices).backward(dy)

    def window(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    variants = (("fused", fused, 20), ("host", host, 1), ("unsampled", unsampled, 20))
    for _, fn, _ in variants:                                         # warm up every shape
        fn()
    lines = [f"ring lattice n = {n}, degree {2 * half}, nnz = {g.nnz}, F = {F}, k = {k}; forward + backward, ms per call; "
             f"host clock round a synchronised window; alternating rounds"]
    times = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, fn, calls in variants:
            t = window(fn, calls)
            times[name].append(t)
            line = f"round {r} {name:<9s} {t:10.4f} ms  ({calls} calls)"
            print(line, flush=True)
            lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    line = (f"medians: fused {med['fused']:.4f} ms, host-sampled MeanAggregator {med['host']:.2f} ms "
            f"({med['host'] / med['fused']:.0f}x), unsampled mean {med['unsampled']:.4f} ms "
            f"({med['unsampled'] / med['fused']:.2f}x)")
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
