"""Probes for the symmetric-adjacency short form of the persistent level-0 backward (csrc/dp_level0.hip), each run once
per build (DP_LIB=<library>) in ONE job and compared afterwards:

  PYTHONPATH=. python tools/l0sym_probe.py dump DIR      one step at B 4, N 100 on a seeded DIRECTED 0/1 batch (no graph
                                                       is symmetric: every graph takes the general form): ypred, loss,
                                                       assignment and every gradient as DIR/<name>.npy
  PYTHONPATH=. python tools/l0sym_probe.py anchor FILE   on a seeded SYMMETRIC batch at B 4, N 100 and at the DD shape: per
                                                       parameter max |grad - grad64| / max |grad64| against the oracle run
                                                       in fp64 with the step's own readout winners, as JSON
  python tools/l0sym_probe.py compare DIR_A DIR_B      numpy.array_equal of two dump directories (also bench.py --dump-outputs)
  python tools/l0sym_probe.py ratio A.json B.json      both anchors and their ratio, as a table
"""
import json
import os
import sys

import numpy as np


def _step(B, N, F_, H, Cc, ratio, p, adj_edit, seed):
    import torch
    from graph_pooling_amd import _lib
    from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
    from oracle import diffpool_oracle as O
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=max(1, N // 10), p=p, seed=seed, n_classes=Cc)
    adj = adj_edit(adj)
    model = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=ratio, linkpred=False)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed - 1, bias_scale=0.1)
    model.load_state_dict(params)
    model = model.cuda()
    xd, ad = x.cuda(), adj.cuda().contiguous()
    y = model(xd, ad, nn_, assign_x=xd)
    win = [model.saved_activation(j, "readout_argmax").clone().cpu() for j in range(2)]
    loss = model.loss(y, label.cuda())
    loss.backward()
    form = _lib.level0_bwd_symmetric()
    out = {"ypred": y.detach(), "loss": loss.detach(), "assign_tensor": model.assign_tensor.detach()}
    out.update({"grad." + k: p_.grad for k, p_ in model.named_parameters()})
    return {k: v.cpu() for k, v in out.items()}, (params, x, adj, nn_, label, win), form


def dump(out_dir):
    import torch

    def directed(adj):          # drop edge directions independently: 0/1, inside n_b, no graph symmetric
        keep = torch.rand(adj.shape, generator=torch.Generator().manual_seed(3)) < 0.6
        adj = adj * keep
        assert all(not torch.equal(a, a.t()) for a in adj)
        return adj
    out, _, form = _step(4, 100, 5, 8, 3, 0.1, 0.1, directed, seed=1)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), v.numpy())
    print(f"dump: {len(out)} arrays to {out_dir}; verdicts {form[0]} (rows per workgroup {form[1]})")


def anchor(path):
    import torch
    from oracle import diffpool_oracle as O
    res = {}
    for name, shp in (("B4_N100", (4, 100, 5, 8, 3, 0.1, 0.1)), ("dd_B20_N500", (20, 500, 89, 20, 2, 0.1, 0.02))):
        out, (params, x, adj, nn_, label, win), form = _step(*shp, lambda a: a, seed=1)
        P = {k: v.double().requires_grad_(True) for k, v in params.items()}
        yo, inter = O.softpool_forward(P, x.double(), adj.double(), nn_, x.double(), winners=win)
        O.softpool_loss(yo, label, inter["assign_0"], adj.double(), nn_, False)[0].backward()
        res[name] = {"verdicts": form[0], "rows_per_workgroup": form[1],
                     "err": {k: float((out["grad." + k].double() - v.grad).abs().max() / v.grad.abs().max())
                             for k, v in P.items()}}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["verdicts"], max(v["err"].values())) for k, v in res.items()}))


def compare(a, b):
    na, nb = sorted(os.listdir(a)), sorted(os.listdir(b))
    differ = [n for n in na if n in nb and not np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))]
    print(f"arrays {len(na)} same names {na == nb} differ {differ}")


def ratio(a, b):
    A, Bj = json.load(open(a)), json.load(open(b))
    print("# max |grad - grad64| / max |grad64| per parameter, oracle in fp64 with the step's readout winners; the bound of")
    print("# tests/parity.py is 2e-5 (absolute floor, relative to the largest entry) + 1e-3 relative")
    for shape in A:
        print(f"## {shape}: verdicts general {A[shape]['verdicts']} short {Bj[shape]['verdicts']}")
        print(f"{'parameter':34s} {'general':>10s} {'short':>10s} {'ratio':>7s}")
        for k in A[shape]["err"]:
            ea, eb = A[shape]["err"][k], Bj[shape]["err"][k]
            print(f"{k:34s} {ea:10.3e} {eb:10.3e} {eb / ea if ea else float('nan'):7.2f}")


if __name__ == "__main__":
    {"dump": dump, "anchor": anchor, "compare": compare, "ratio": ratio}[sys.argv[1]](*sys.argv[2:])
