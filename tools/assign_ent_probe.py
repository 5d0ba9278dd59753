"""Measurements of the assignment-entropy entries (dp_assign_entropy_fwd / _bwd) on the GPU.

  PYTHONPATH=. python tools/assign_ent_probe.py anchor     # largest error / bound ratio per case of the GPU op test
  PYTHONPATH=. python tools/assign_ent_probe.py stream     # achieved bytes/s at the ER and DD shapes, next to a device copy

`anchor` runs the cases of tests/test_gpu_assign_ent.py (their checks included) and prints, per shape, the largest
|error| / bound the forward and the backward (accumulate = 0 and = 1) reached against the fp64 reference
(profiles/assign_ent_fp64_anchor.txt).
`stream` times both entries with device events over S [B, N, K]: the forward reads S once (4 B N K bytes), the backward
reads S and writes dS (8 B N K; 12 B N K with accumulate = 1); the copy of the same S (read + write, 8 B N K) is the
streaming reference measured in the same process."""
import sys

import numpy as np
import torch

from graph_pooling_amd import _lib


def anchor():
    from tests import assign_ent_cases as AC
    from tests import test_gpu_assign_ent as T
    print(f"C_FWD = {AC.C_FWD}, C_BWD = {AC.C_BWD}, u = 2^-24")
    print(f"{'shape':>16} {'fwd err/bound':>14} {'bwd acc=0':>14} {'bwd acc=1':>14}")
    worst = [0.0, 0.0, 0.0]
    for B, n, K in AC.SMALL + AC.LOOP + AC.WRAP:
        seed = B * 100003 + n * 1009 + K
        r = [0.0, 0.0, 0.0]
        combos = [(p, o, m) for p in (0, 3) for o in (0, 1) for m in AC.MASKS] + [(4, 0, "mix")]
        if (B, n, K) in AC.LOOP + AC.WRAP:
            combos = [(0, 0, "mix"), (3, 1, "null"), (0, 1, "full")]
        for ld_pad, off, mask in combos:
            r = [max(a, b) for a, b in zip(r, T._check_case(B, n, K, ld_pad, off, mask, seed))]
        worst = [max(a, b) for a, b in zip(worst, r)]
        print(f"{f'{B}x{n}x{K}':>16} {r[0]:14.4f} {r[1]:14.4f} {r[2]:14.4f}")
    print(f"{'largest':>16} {worst[0]:14.4f} {worst[1]:14.4f} {worst[2]:14.4f}")


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts))


def stream():
    lib = _lib.load()
    st = _lib.current_stream()
    for name, (B, N, K), reps in (("ER", (256, 1024, 256), 30), ("DD", (20, 500, 50), 200)):
        S = torch.softmax(torch.randn(B, N, K, device="cuda"), dim=2)
        dS = torch.zeros_like(S)
        nn = torch.randint(N // 2, N + 1, (B,), device="cuda", dtype=torch.int32)
        out = torch.zeros(2, device="cuda")
        ws = torch.empty(lib.dp_assign_entropy_workspace_bytes(B, N, K), dtype=torch.uint8, device="cuda")
        nbytes = S.numel() * 4
        rows = {}
        for mask, nnp in (("no mask", None), ("num_nodes", nn.data_ptr())):
            valid = 1.0 if nnp is None else float(nn.sum()) / (B * N)
            rows[f"fwd, {mask}"] = (lambda nnp=nnp: _lib.check(lib.dp_assign_entropy_fwd(
                S.data_ptr(), K, nnp, 0.3, out.data_ptr(), None, B, N, K, ws.data_ptr(), ws.numel(), st)), nbytes * valid)
            rows[f"bwd acc=0, {mask}"] = (lambda nnp=nnp: _lib.check(lib.dp_assign_entropy_bwd(
                S.data_ptr(), K, nnp, None, 0.3, dS.data_ptr(), K, 0, B, N, K, st)), nbytes * (valid + 1.0))
            rows[f"bwd acc=1, {mask}"] = (lambda nnp=nnp: _lib.check(lib.dp_assign_entropy_bwd(
                S.data_ptr(), K, nnp, None, 0.3, dS.data_ptr(), K, 1, B, N, K, st)), nbytes * 3.0 * valid)
        rows["device copy of S (read + write)"] = (lambda: dS.copy_(S), nbytes * 2.0)
        print(f"{name} shape S [{B}, {N}, {K}] = {nbytes / 1e6:.1f} MB")
        for what, (fn, moved) in rows.items():
            med, best = _time(fn, reps)
            print(f"  {what:34s} median {med * 1e6:9.1f} us  best {best * 1e6:9.1f} us  "
                  f"{moved / med / 1e12:6.3f} TB/s (median; bytes the kernel has to move: {moved / 1e6:.1f} MB)")


if __name__ == "__main__":
    {"anchor": anchor, "stream": stream}[sys.argv[1] if len(sys.argv) > 1 else "stream"]()
