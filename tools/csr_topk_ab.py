"""The fused top-k pooling (`ops.csr_topk_pool`: dp_csr_topk_select / _induce / _gather_*) next to the host route it
replaces, on a ragged batch of ring lattices.

    python tools/csr_topk_ab.py [--out FILE] [--graphs 64] [--nodes 1024] [--rounds 9]

`--graphs` ring lattices of `--nodes` nodes and degree 8 (every node joined to the 4 nodes on either side) in one
undirected 0/1 `CsrBatch`, F = 64, ratio = 0.5, gate = tanh(score).  `fused`: `ops.csr_topk_pool` (5 launches and the
4-byte read-back of nnz') and the backward of x_out (1 launch).  `host`: a `torch.topk` per graph, the kept ids sorted, a
boolean mask over a COO copy of the adjacency kept on the device, the surviving entries renumbered there, copied to the
host and handed to `CsrBatch.from_edge_lists`, x[perm] * gate[perm] and its backward by torch indexing.  Both give the
same perm and the same CSR (asserted once, before timing).  The two are timed in ALTERNATING rounds in one process — a
host clock round work that ends in a device synchronise, `calls` calls per window — and the medians and ranges over the
rounds are reported; every raw window is printed."""
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
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import numpy as np
    import torch
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrBatch
    B, nb, half, F, ratio = a.graphs, a.nodes, 4, 64, 0.5
    i = np.arange(nb)
    src = np.repeat(i, half)
    dst = (src + np.tile(np.arange(1, half + 1), nb)) % nb
    sizes = [nb] * B
    batch = CsrBatch.from_edge_lists(sizes, [src] * B, [dst] * B, "cuda", symmetric=True)
    n = batch.n_total
    assert batch.nnz == 2 * half * nb * B
    ip = batch.indptr.cpu().numpy().astype(np.int64)
    coo_r = torch.from_numpy(np.repeat(np.arange(n), np.diff(ip))).cuda()          # the COO copy the host route masks
    coo_c = batch.indices.long()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, F, generator=gen).cuda().requires_grad_(True)
    score = torch.randn(n, generator=gen).cuda()
    gate = torch.tanh(score)
    kb = ops.topk_counts(sizes, ratio=ratio)
    new_off = np.concatenate([[0], np.cumsum(kb)])
    dy = torch.randn(int(kb.sum()), F, device="cuda")
    kept = {}

    def fused():
        x.grad = None
        y, g, perm = ops.csr_topk_pool(x, score, batch, ratio=ratio, gate=gate)
        y.backward(dy)
        kept["fused"] = (g, perm)

    def host():
        x.grad = None
        ids = []
        for b in range(B):
            lo = b * nb
            ids.append(torch.topk(score[lo:lo + nb], int(kb[b])).indices.sort().values + lo)
        perm = torch.cat(ids)
        new_id = torch.full((n,), -1, dtype=torch.long, device="cuda")
        new_id[perm] = torch.arange(perm.numel(), device="cuda")
        keep = (new_id[coo_r] >= 0) & (new_id[coo_c] >= 0)
        r, c = new_id[coo_r[keep]].cpu().numpy(), new_id[coo_c[keep]].cpu().numpy()
        gb = np.searchsorted(new_off, r, side="right") - 1
        cut = np.searchsorted(gb, np.arange(B + 1))
        g = CsrBatch.from_edge_lists(kb, [r[cut[b]:cut[b + 1]] - new_off[b] for b in range(B)],
                                     [c[cut[b]:cut[b + 1]] - new_off[b] for b in range(B)], "cuda", symmetric=False)
        y = x[perm] * gate[perm][:, None]
        y.backward(dy)
        kept["host"] = (g, perm)

    def window(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    variants = (("fused", fused, 20), ("host", host, 2))
    for _, fn, _ in variants:                                         # warm up every shape
        fn()
    (gf, pf), (gh, ph) = kept["fused"], kept["host"]
    assert torch.equal(pf.long(), ph) and gf.nnz == gh.nnz and torch.equal(gf.indptr, gh.indptr)
    assert torch.equal(gf.indices, gh.indices) and torch.equal(gf.indices_local, gh.indices_local)
    lines = [f"{B} ring lattices of {nb} nodes, degree {2 * half}: n = {n}, nnz = {batch.nnz}, F = {F}, ratio = {ratio} -> "
             f"n' = {int(kb.sum())}, nnz' = {gf.nnz}; pooling forward (container included) + backward of x_out, ms per call; "
             f"host clock round a synchronised window; alternating rounds"]
    times = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, fn, calls in variants:
            t = window(fn, calls)
            times[name].append(t)
            line = f"round {r} {name:<6s} {t:10.4f} ms  ({calls} calls)"
            print(line, flush=True)
            lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    rng = {name: (min(v), max(v)) for name, v in times.items()}
    line = (f"medians: fused {med['fused']:.4f} ms ({rng['fused'][0]:.4f} - {rng['fused'][1]:.4f}), host route "
            f"{med['host']:.3f} ms ({rng['host'][0]:.3f} - {rng['host'][1]:.3f}), {med['host'] / med['fused']:.0f}x")
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
