"""A two-layer `SupervisedGraphSage` on nested mini-batches (`NestedSageEncoder`, dp_csr_block_*) next to the same two
`SageConv` layers stacked on the whole graph, where only the last layer takes the mini-batch.

    python tools/csr_block_ab.py [--out FILE] [--log2n 16] [--targets 256] [--rounds 9]

§4.10's ring lattice: 2^16 nodes, degree 32 (every node joined to the 16 nodes on either side), F = 64, hidden 64,
k = 10, 256 targets drawn once.  `nested`: forward + loss + backward of `SupervisedGraphSage(NestedSageEncoder)` — the
two block builds, their two 4-byte read-backs and the feature gather are inside the timed window.  `whole`: the same
layers and head with `conv2(conv1(x, g, seed_0), g, nodes, seed_1)`.  `blocks`: the two block builds alone (with their
read-backs), to show where the nested time goes.  The variants are timed in ALTERNATING rounds in one process — a host
clock round work that ends in a device synchronise, `calls` calls per window — and the medians over the rounds are
reported with their ranges; every raw window is printed."""
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
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import numpy as np
    import torch
    from graph_pooling_amd import NestedSageEncoder, SageConv
    from graph_pooling_amd.graphsage import SupervisedGraphSage
    from graph_pooling_amd.ops import hip_linear
    from graph_pooling_amd.sparse import CsrGraph
    n, half, F, H, k, C = 1 << a.log2n, 16, 64, 64, 10, 8
    src = np.repeat(np.arange(n), half)
    dst = (src + np.tile(np.arange(1, half + 1), n)) % n
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    g.indptr_t, g.indices_t
    rng = np.random.default_rng(5)
    nodes = rng.choice(n, a.targets, replace=False).astype(np.int64)
    nodes_dev = torch.from_numpy(nodes.astype(np.int32)).cuda()
    labels = torch.from_numpy(rng.integers(0, C, a.targets)).cuda()
    torch.manual_seed(1)
    x = torch.randn(n, F, device="cuda")
    c1, c2 = SageConv(F, H, num_sample=k).cuda(), SageConv(H, H, num_sample=k).cuda()
    enc = NestedSageEncoder(x, g, [c1, c2])
    model = SupervisedGraphSage(C, enc).cuda()
    step = [0]

    def nested():
        step[0] += 1
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(hip_linear(enc(nodes, seed=step[0]), model.weight.t()), labels).backward()

    def whole():
        step[0] += 1
        model.zero_grad(set_to_none=True)
        h = c2(c1(x, g, seed=enc.layer_seed(step[0], 0)), g, nodes_dev, seed=enc.layer_seed(step[0], 1), nodes_checked=True)
        torch.nn.functional.cross_entropy(hip_linear(h, model.weight.t()), labels).backward()

    def blocks():
        step[0] += 1
        enc.blocks(nodes, step[0])

    def window(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    variants = (("nested", nested, 20), ("whole", whole, 20), ("blocks", blocks, 20))
    for _, fn, _ in variants:                                         # warm up every shape
        fn()
    b0, b1 = enc.blocks(nodes, 1)
    lines = [f"ring lattice n = {n}, degree {2 * half}, nnz = {g.nnz}, F = {F}, hidden {H}, k = {k}, {a.targets} targets; "
             f"n_src = {b1.n_src} (layer 1), {b0.n_src} (layer 0) at seed 1; two-layer SupervisedGraphSage forward + loss + "
             f"backward, ms per call; host clock round a synchronised window; alternating rounds"]
    times = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, fn, calls in variants:
            t = window(fn, calls)
            times[name].append(t)
            line = f"round {r} {name:<7s} {t:10.4f} ms  ({calls} calls)"
            print(line, flush=True)
            lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    rng_of = lambda name: f"{min(times[name]):.4f} .. {max(times[name]):.4f}"
    line = (f"medians of {a.rounds}: nested {med['nested']:.4f} ms ({rng_of('nested')}), whole-graph stack "
            f"{med['whole']:.4f} ms ({rng_of('whole')}; {med['whole'] / med['nested']:.2f}x), of the nested time the two "
            f"block builds with their read-backs {med['blocks']:.4f} ms ({rng_of('blocks')})")
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
