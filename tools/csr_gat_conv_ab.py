"""The fused GAT convolution (dp_csr_gat_conv_fwd / _bwd) next to the same layer composed per head from the existing
entries, next to a device copy of the bytes the fused entries must move.

    python tools/csr_gat_conv_ab.py [--out FILE]

A 2^20-node ring lattice of degree 6 and the 5 748-node graph of tools/csr_gat_ab.py (DD's size and mean degree);
(H, C) = (1, 8), (4, 8), (8, 8), (8, 64), concat.  `fused`: `ops.csr_gat_conv`, forward under no_grad, and forward +
backward.  `composed`: per head h the existing C entries on preallocated buffers — forward dp_csr_gat_fwd (H = 1, column h
of u, v) and dp_csr_aggregate_w on the head's slice of z; backward dp_csr_sddmm (the gradient of the coefficients,
dy^h . z^h per entry), dp_csr_gat_bwd, the coefficients permuted to the transposed order and dp_csr_aggregate_w over
A^T (dz^h) — so its time is launches and kernels only, with no autograd bookkeeping, and it keeps H coefficient vectors
[nnz] for the backward.  `copy`: a device-to-device copy of the bytes the fused entries must move when every array is
moved once (forward: z, y, u, v, rowstat, the CSR; backward: z, dy, dz, u, v, du, dv, t, rowstat, both CSRs), taken in the
same run.  One event pair round ten calls, the median of 20 pairs.  Peak memory: `torch.cuda.max_memory_allocated` over
one forward + backward above what is allocated before it (the composed route allocates its buffers inside)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, iters=20, reps=10):
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


def _graphs():
    import numpy as np
    from graph_pooling_amd.sparse import CsrGraph
    n = 1 << 20
    i = np.arange(n)
    src, dst = np.repeat(i, 3), (np.repeat(i, 3) + np.tile([1, 2, 3], n)) % n
    yield "lattice 2^20 x 6", CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    n = 5748
    rng = np.random.default_rng(0)
    ring = np.arange(n)
    src = np.concatenate([ring, rng.integers(0, n, 3 * n // 2)])
    dst = np.concatenate([(ring + 1) % n, rng.integers(0, n, 3 * n // 2)])
    keep = src != dst
    yield "DD-sized 5748", CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)


class Composed:
    """The layer per head on the existing C entries; every buffer is allocated here."""

    def __init__(self, g, z, u, v, H, C):
        import torch
        from graph_pooling_amd import _lib
        self.lib, self.g, self.z, self.u, self.v, self.H, self.C = _lib.load(), g, z, u, v, H, C
        f32 = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32)
        self.a = [f32(g.nnz) for _ in range(H)]                       # kept for the backward
        self.rs = [f32(g.n, 2) for _ in range(H)]
        self.y = f32(g.n, H * C)
        self.da, self.tdot, self.du, self.dv, self.dz = f32(g.nnz), f32(g.n), f32(g.n, H), f32(g.n, H), f32(g.n, H * C)
        self.a_t = f32(g.nnz)                                         # a coefficient vector in the transposed order
        self.mirror = g.mirror_perm.long()
        self.st = _lib.current_stream()
        self.check = _lib.check

    def forward(self):
        g, H, C, W, lib, st = self.g, self.H, self.C, self.H * self.C, self.lib, self.st
        ip, ix = g.indptr.data_ptr(), g.indices.data_ptr()
        for h in range(H):
            self.check(lib.dp_csr_gat_fwd(self.u.data_ptr() + 4 * h, H, self.v.data_ptr() + 4 * h, H, ip, ix,
                                          self.a[h].data_ptr(), self.rs[h].data_ptr(), g.n, g.nnz, 1, 0.2, st))
            self.check(lib.dp_csr_aggregate_w(self.z.data_ptr() + 4 * h * C, W, ip, ix, self.a[h].data_ptr(),
                                              self.y.data_ptr() + 4 * h * C, W, g.n, C, 0.0, st))
        return self.y

    def backward(self, dy):
        import torch
        g, H, C, W, lib, st = self.g, self.H, self.C, self.H * self.C, self.lib, self.st
        ip, ix, ipt, ixt = (t.data_ptr() for t in (g.indptr, g.indices, g.indptr_t, g.indices_t))
        for h in range(H):
            self.check(lib.dp_csr_sddmm(dy.data_ptr() + 4 * h * C, W, self.z.data_ptr() + 4 * h * C, W, ip, ix,
                                        self.da.data_ptr(), g.n, C, 1.0, None, 0.0, st))
            self.check(lib.dp_csr_gat_bwd(self.u.data_ptr() + 4 * h, H, self.v.data_ptr() + 4 * h, H, ip, ix, ipt, ixt,
                                          g.mirror_perm.data_ptr(), self.rs[h].data_ptr(), self.da.data_ptr(),
                                          self.tdot.data_ptr(), self.du.data_ptr() + 4 * h, H, self.dv.data_ptr() + 4 * h,
                                          H, g.n, g.nnz, 1, 0.2, st))
            torch.index_select(self.a[h], 0, self.mirror, out=self.a_t)
            self.check(lib.dp_csr_aggregate_w(dy.data_ptr() + 4 * h * C, W, ipt, ixt, self.a_t.data_ptr(),
                                              self.dz.data_ptr() + 4 * h * C, W, g.n, C, 0.0, st))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from graph_pooling_amd import ops
    lines = ["events round 10 calls, median of 20; fused = ops.csr_gat_conv (concat), composed = per head dp_csr_gat_fwd + "
             "dp_csr_aggregate_w / dp_csr_sddmm + dp_csr_gat_bwd + dp_csr_aggregate_w on preallocated buffers"]
    for gname, g in _graphs():
        g.mirror_perm, g.indptr_t, g.indices_t                        # built once, outside every timing
        for H, C in ((1, 8), (4, 8), (8, 8), (8, 64)):
            W = H * C
            gen = torch.Generator().manual_seed(W)
            z = torch.randn(g.n, W, generator=gen).cuda().requires_grad_(True)
            u = torch.randn(g.n, H, generator=gen).cuda().requires_grad_(True)
            v = torch.randn(g.n, H, generator=gen).cuda().requires_grad_(True)
            dy = torch.randn(g.n, W, generator=gen).cuda()

            def fused_fwd():
                with torch.no_grad():
                    return ops.csr_gat_conv(z, u, v, g, H)

            def fused_both():
                z.grad = u.grad = v.grad = None
                ops.csr_gat_conv(z, u, v, g, H).backward(dy)

            def composed_both(c=None):
                c = c or Composed(g, z.detach(), u.detach(), v.detach(), H, C)
                c.forward()
                c.backward(dy)
                return c

            peaks = {}
            for name, run in (("fused", fused_both), ("composed", composed_both)):
                run()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                keep = run()
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
                del keep
            comp = Composed(g, z.detach(), u.detach(), v.detach(), H, C)
            err = float((fused_fwd() - comp.forward()).abs().max())
            for _ in range(3):
                fused_both()
                composed_both(comp)
            ff, fa = _median_ms(fused_fwd), _median_ms(fused_both)
            cf, ca = _median_ms(comp.forward), _median_ms(lambda: composed_both(comp))
            csr = 4 * (g.n + 1 + g.nnz)
            fb = 4 * g.n * (2 * W + 4 * H) + csr
            bb = 4 * g.n * (3 * W + 7 * H) + 2 * csr
            copies = []
            for nbytes in (fb, fb + bb):
                half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                dstb = torch.empty_like(half)
                for _ in range(3):
                    dstb.copy_(half)
                copies.append(_median_ms(lambda: dstb.copy_(half)))
            del comp
            line = (f"{gname} H={H} C={C}: forward fused {1e3 * ff:.1f} us, composed {1e3 * cf:.1f} us ({cf / ff:.2f}x), "
                    f"copy of {fb / 1e6:.2f} MB {1e3 * copies[0]:.1f} us; forward+backward fused {1e3 * fa:.1f} us, composed "
                    f"{1e3 * ca:.1f} us ({ca / fa:.2f}x), copy of {(fb + bb) / 1e6:.2f} MB {1e3 * copies[1]:.1f} us; peak "
                    f"memory above the inputs fused {peaks['fused'] / 1e6:.2f} MB, composed {peaks['composed'] / 1e6:.2f} MB; "
                    f"max |fused - composed| {err:.2e}")
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
