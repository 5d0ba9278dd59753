"""Bits of every CSR op, this tree against another checkout of the project (the parent commit), in fresh processes.

    python tools/csr_entry_bits.py [--other-root DIR] [--out FILE]

One child process per tree, one after the other, each under a time limit.  A child runs every CSR op forward and
backward on fixed inputs and writes the raw outputs: the neighbour sum (dp_csr_aggregate), the GraphConv layer (with
the transposed arrays, and once without them: the atomic scatter), pooling, the cross-entropy link loss and the
Frobenius link loss — on one graph of 70 nodes (a 64-row tile and a tail) and on a ragged batch of sizes (1, 65, 30),
undirected and directed, weighted and 0/1, with K in {5, 8} clusters (4-byte and 16-byte lanes) and D = 20 features.

The driver compares the bytes.  The other tree is also run a second time and compared with itself: an output that is
not bit-stable there may only be the atomic scatter's dx; it is named and held to twice the fp64-anchored bound of its
GPU test (tests/csr_weights_cases.gcn_ref: each tree is within the bound of the same reference) instead.  Everything
else must be equal.  Exit status 1 on any difference."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIZES, K_CASES, D = 70, (1, 65, 30), (5, 8), 20
GCN_FLAGS = 3            # DP_F_ADD_SELF | DP_F_NORMALIZE
SCATTER = "gcn_scatter_dx"


def worker(root, out):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from graph_pooling_amd import _lib, ops
    from graph_pooling_amd.sparse import CsrGraph
    from tests import csr_weights_cases as WC

    lib = _lib.load()
    res = {}

    def keep(name, t):
        res[name] = t.detach().cpu().numpy().copy()

    def plain(g):           # the same container without its values
        if isinstance(g, CsrGraph):
            return CsrGraph(g.indptr, g.indices) if g.indices_t is g.indices else \
                CsrGraph(g.indptr, g.indices, g.indptr_t, g.indices_t)
        import copy
        p = copy.copy(g)
        p.weighted, p.values, p.values_t = False, None, None
        p._pool_plans = {}
        return p

    for form in ("graph", "batch"):
        for directed in (False, True):
            host = WC.graph(N, 4, 5, directed) if form == "graph" else WC.batch(list(SIZES), 4, 9, directed)
            gw = WC.to_device(host, "cuda")
            for weighted in (True, False):
                g = gw if weighted else plain(gw)
                tag = f"{form} {'directed' if directed else 'undirected'} {'weighted' if weighted else '0/1'}"
                rng = np.random.default_rng(17)
                n = g.n
                x = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).cuda()
                W = torch.from_numpy((rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)).cuda()
                b = torch.from_numpy(rng.uniform(-0.3, 0.3, D).astype(np.float32)).cuda()
                dy = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).cuda()
                # neighbour sum
                out_ = torch.full((n, D), 0.25, device="cuda")
                a = (g.indptr.data_ptr(), g.indices.data_ptr())
                if weighted:
                    _lib.check(lib.dp_csr_aggregate_w(x.data_ptr(), D, *a, g.values.data_ptr(), out_.data_ptr(), D, n, D, 1.0,
                                                      _lib.current_stream()))
                else:
                    _lib.check(lib.dp_csr_aggregate(x.data_ptr(), D, *a, out_.data_ptr(), D, n, D, 0, 1.0,
                                                    _lib.current_stream()))
                keep(f"{tag}: aggregate", out_)
                # GraphConv through the autograd wrapper (gathers over the transposed arrays)
                xr, Wr, br = x.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
                y = ops.csr_graph_conv(xr, Wr, br, g, GCN_FLAGS)
                y.backward(dy)
                for name, t in (("y", y), ("dx", xr.grad), ("dW", Wr.grad), ("db", br.grad)):
                    keep(f"{tag}: gcn {name}", t)
                if form == "graph":      # the backward without transposed arrays: float atomics
                    ax, inv = torch.empty(n, D, device="cuda"), torch.empty(n, device="cuda")
                    y2, dx, dW, db = (torch.empty(s, device="cuda") for s in ((n, D), (n, D), (D, D), (D,)))
                    wsb = lib.dp_sparse_gcn_layer_workspace_bytes(n, D, D)
                    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
                    v = (g.values.data_ptr(),) if weighted else ()
                    sfx = "_w" if weighted else ""
                    tail = (n, D, D, GCN_FLAGS, ws.data_ptr(), wsb, _lib.current_stream())
                    _lib.check(getattr(lib, "dp_sparse_gcn_layer_fwd" + sfx)(
                        x.data_ptr(), D, *a, *v, W.data_ptr(), b.data_ptr(), y2.data_ptr(), D, ax.data_ptr(), inv.data_ptr(),
                        *tail))
                    _lib.check(getattr(lib, "dp_sparse_gcn_layer_bwd" + sfx)(
                        ax.data_ptr(), *a, *v, None, None, *((None,) if weighted else ()), W.data_ptr(), y2.data_ptr(), D,
                        inv.data_ptr(), dy.data_ptr(), D, dx.data_ptr(), D, dW.data_ptr(), db.data_ptr(), *tail))
                    keep(f"{tag}: {SCATTER}", dx)
                    keep(f"{tag}: gcn_scatter dW", dW)
                    if weighted:
                        ref, bound = WC.gcn_ref(WC.dense(host), x.cpu().numpy(), W.cpu().numpy(), b.cpu().numpy(),
                                                dy.cpu().numpy(), True, True, WC.degrees(host),
                                                np.diff(host.indptr_t.numpy().astype(np.int64)), True)["dx"]
                    else:
                        ref, bound = WC.gcn_ref((WC.dense(host) != 0).astype(np.float64), x.cpu().numpy(), W.cpu().numpy(),
                                                b.cpu().numpy(), dy.cpu().numpy(), True, True, WC.degrees(host),
                                                np.diff(host.indptr_t.numpy().astype(np.int64)), True)["dx"]
                    res[f"{tag}: {SCATTER} bound"] = np.asarray(bound, dtype=np.float64) * np.ones_like(ref)
                for K in K_CASES:
                    s = torch.from_numpy(WC.assign_rows(np.random.default_rng(K), n, K).astype(np.float32)).cuda()
                    z = torch.from_numpy((np.random.default_rng(K + 1).random((n, D)) - 0.5).astype(np.float32)).cuda()
                    sr, zr = s.clone().requires_grad_(True), z.clone().requires_grad_(True)
                    xp, ap = g.pool(sr, zr)
                    gen = torch.Generator(device="cpu").manual_seed(K)
                    (xp * torch.randn(xp.shape, generator=gen).cuda()).sum().add(
                        (ap * torch.randn(ap.shape, generator=gen).cuda()).sum()).backward()
                    for name, t in (("Xp", xp), ("Ap", ap), ("dS", sr.grad), ("dZ", zr.grad)):
                        keep(f"{tag} K={K}: pool {name}", t)
                    for objective in ("bce", "frobenius"):
                        sr = s.clone().requires_grad_(True)
                        loss = g.link_loss(sr, objective)
                        (loss * 1.7).backward()
                        keep(f"{tag} K={K}: link {objective} loss", loss)
                        keep(f"{tag} K={K}: link {objective} dS", sr.grad)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print(f"WROTE {len(res)} arrays")


def run_child(root, out):
    subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--npz", out], check=True,
                   timeout=240, cwd=root)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-root")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--npz")
    a = ap.parse_args()
    if a.worker:
        worker(a.root, a.npz)
        return
    import numpy as np
    other = os.path.abspath(a.other_root) if a.other_root else ROOT
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(tmp, f"{i}.npz") for i in range(3)]
        run_child(ROOT, files[0])
        run_child(other, files[1])
        run_child(other, files[2])           # the other tree against itself: which ops are bit-stable at all
        this, oth, oth2 = (dict(np.load(f)) for f in files)
    assert this.keys() == oth.keys() == oth2.keys()
    names = [k for k in this if not k.endswith(" bound")]
    # (float atomics may also agree in two runs by chance: the scatter is held to its bound whenever its bytes differ)
    unstable = [k for k in names if oth[k].tobytes() != oth2[k].tobytes()
                or (k.endswith(SCATTER) and this[k].tobytes() != oth[k].tobytes())]
    lines = [f"CSR ops, this tree against {'the other checkout' if a.other_root else 'itself'}: {len(names)} outputs; "
             f"one graph of {N} nodes and the batch {SIZES}, undirected / directed, weighted / 0/1, K in {K_CASES}, D = {D}"]
    bad = 0
    for k in unstable:
        if not k.endswith(SCATTER):
            bad += 1
            lines.append(f"NOT BIT-STABLE in the other tree and not the atomic scatter: {k}")
            continue
        err = np.abs(this[k].astype(np.float64) - oth[k].astype(np.float64))
        worst = float((err / (2.0 * this[k + " bound"])).max())
        bad += worst > 1.0
        twice = "differs" if oth[k].tobytes() != oth2[k].tobytes() else "happens to agree"
        lines.append(f"float atomics, not held to bit equality (the other tree run twice {twice}): {k}; this - other "
                     f"is at most {worst:.3g} of twice its test's bound -> {'ok' if worst <= 1.0 else 'FAIL'}")
    differ = [k for k in names if k not in unstable and this[k].tobytes() != oth[k].tobytes()]
    for k in differ:
        lines.append(f"DIFFERENT BITS: {k}: max |this - other| = "
                     f"{float(np.abs(this[k].astype(np.float64) - oth[k].astype(np.float64)).max()):.3g}")
    bad += len(differ)
    lines.append(f"{len(names) - len(unstable) - len(differ)} of {len(names) - len(unstable)} bit-stable outputs have "
                 f"equal bytes in both trees; {len(unstable)} held to a bound; verdict: {'EQUAL' if not bad else 'DIFFERENT'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
