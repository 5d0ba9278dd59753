"""The link-prediction loss kernels at the DD shape (B = 20, N = 500, K = 50): the fp32 entries on the dense batch
against the packed entries on its bf16 rows, for a kernel trace:
  rocprofv3 --kernel-trace --stats -d OUT -o link -- python3 tools/linkpred_packed_probe.py [--reps 50]
The two forms alternate within each repetition; the run ends with a bit-identity check of loss and dS."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.encoders import PackedAdjacency  # noqa: E402
from oracle import diffpool_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    B, N, K = 20, 500, 50
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    _, adj, nn_, _ = O.make_batch(B, N, 3, n_min=30, p=0.02, seed=1)
    g = torch.Generator().manual_seed(2)
    S = (torch.softmax(torch.randn(B, N, K, generator=g), -1) * O.node_mask(N, nn_)).cuda().contiguous()
    ad, nd = adj.cuda(), torch.from_numpy(nn_).cuda()
    pa = PackedAdjacency.from_dense(ad)
    wsb = lib.dp_linkpred_workspace_bytes(B, N, K)
    ws = torch.zeros(wsb, device="cuda", dtype=torch.uint8)
    dl = torch.ones(1, device="cuda")
    out = {f: (torch.empty(1, device="cuda"), torch.empty_like(S)) for f in ("fp32", "packed")}

    def fp32():
        loss, dS = out["fp32"]
        _lib.check(lib.dp_linkpred_loss_fwd(S.data_ptr(), ad.data_ptr(), nd.data_ptr(), loss.data_ptr(), B, N, K,
                                            ws.data_ptr(), wsb, st))
        _lib.check(lib.dp_linkpred_loss_bwd(S.data_ptr(), ad.data_ptr(), nd.data_ptr(), dl.data_ptr(), dS.data_ptr(), 0,
                                            B, N, K, ws.data_ptr(), wsb, st))

    def packed():
        loss, dS = out["packed"]
        _lib.check(lib.dp_linkpred_loss_fwd_packed(S.data_ptr(), pa.pk.data_ptr(), nd.data_ptr(), loss.data_ptr(), B, N,
                                                   K, ws.data_ptr(), wsb, st))
        _lib.check(lib.dp_linkpred_loss_bwd_packed(S.data_ptr(), pa.pk.data_ptr(), pa.pkt.data_ptr(), nd.data_ptr(),
                                                   dl.data_ptr(), dS.data_ptr(), 0, B, N, K, ws.data_ptr(), wsb, st))

    for _ in range(args.reps):
        fp32()
        packed()
    torch.cuda.synchronize()
    same = torch.equal(out["fp32"][0], out["packed"][0]) and torch.equal(out["fp32"][1], out["packed"][1])
    print(json.dumps({"shape": [B, N, K], "reps": args.reps, "loss": float(out["packed"][0]), "bit_identical": same}))
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
