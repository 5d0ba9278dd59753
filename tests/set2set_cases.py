"""The Set2Set case table shared by test_set2set_plan_cpu.py and test_gpu_set2set.py, the seeded inputs of a case and its
CPU references (oracle.diffpool_oracle.set2set_forward in float64 and float32).

k_set2set_fwd / k_set2set_bwd (dp_set2set.hip) are compiled in five variants and the launcher picks one from (n, d)
alone (dp_set2set_plan), so the table is built to reach every variant and every edge of the kernels' loops:
  d   64 | 65 (weights leave the registers), 69 | 70 (weights leave LDS), 128 | 129 and 192 | 193 (2 | 3 | 4 passes
      over 256-gate chunks), 256 (upper limit: the gate clamp never fires)
  n   1, values that are not multiples of 16, 256 | 257 (rows >= 256 of the backward are read in place, not
      prefetched), 1000 at d = 60 (the reference's defaults: max_nodes 1000, three 20-wide layers), 1024 (upper limit)
d = 1 is left out on purpose: its ReLU output is all zero, so the case would check nothing."""
import functools

import torch

from oracle import diffpool_oracle as O

# plan bits of dp_set2set_plan (include/diffpool_hip.h)
W_LDS, E_LDS, W_REGS = 1, 2, 4
VARIANTS = {W_REGS | E_LDS: "WF+EL", W_REGS: "WF", W_LDS | E_LDS: "WL+EL", W_LDS: "WL", 0: "WG"}
ERR_UNSUPPORTED = -3

# (B, n, d)
CASES = [
    (3, 7, 12), (2, 1, 8), (2, 100, 64), (2, 256, 60), (2, 257, 60),          # WF+EL
    (2, 600, 64), (1, 1000, 60), (2, 1024, 40),                              # WF
    (2, 40, 65),                                                             # WL+EL
    (2, 300, 66), (2, 16, 69),                                               # WL
    (2, 50, 70), (2, 33, 128), (2, 45, 129), (2, 300, 130), (2, 37, 193), (2, 70, 200), (2, 20, 256),
    (2, 260, 256),                                                           # WG
]
REFUSED = [(1025, 60), (100, 257)]

PARAM_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "pred.weight",
              "pred.bias")
# every tensor a case is checked on: the output, the embedding gradient and the six parameter gradients
TENSORS = ("out", "demb") + PARAM_KEYS


def case_id(case):
    return "B%d-n%d-d%d" % case


def make_inputs(B, n, d):
    """emb = 0.3 * randn with the last third of graph 0's rows zero (padded nodes: the softmax still runs over them),
    parameters uniform in +-1/sqrt(d) (nn.LSTM / nn.Linear style), upstream gradient randn(B, d).  All float32."""
    g = torch.Generator().manual_seed(1000 * n + d)
    emb = 0.3 * torch.randn(B, n, d, generator=g)
    emb[0, n - n // 3:] = 0.0
    shapes = ((4 * d, 2 * d), (4 * d, d), (4 * d,), (4 * d,), (d, 2 * d), (d,))
    a = 1.0 / d ** 0.5
    params = {k: (torch.rand(s, generator=g) * 2 - 1) * a for k, s in zip(PARAM_KEYS, shapes)}
    gout = torch.randn(B, d, generator=g)
    return emb, params, gout


def reference(emb, params, gout, dtype):
    """set2set_forward and its gradients on the CPU in `dtype`, returned in float64: {tensor name: value}."""
    e = emb.to(dtype).requires_grad_(True)
    P = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    out = O.set2set_forward(e, P)
    (out * gout.to(dtype)).sum().backward()
    res = {"out": out.detach().double(), "demb": e.grad.double()}
    res.update({k: P[k].grad.double() for k in PARAM_KEYS})
    return res


@functools.lru_cache(maxsize=None)
def case_references(case):
    """(inputs, fp64 reference, fp32 oracle) of a table row; computed once per process."""
    inp = make_inputs(*case)
    return inp, reference(*inp, torch.float64), reference(*inp, torch.float32)


# Bound of the fp64-anchored check, per tensor:  max|gpu - ref64| <= M * max|oracle32 - ref64| + F * max|ref64|.
# M and F are those of test_gradients_no_worse_than_fp32_oracle_vs_fp64 (test_gpu_model.py), for the reasons given
# there: the yardstick is the fp32 oracle's own distance from fp64, and the floor of a few ulp of the tensor's largest
# entry covers tensors where that distance is, by luck, under one ulp.  CAP is absolute: whatever the oracle's error,
# no tensor is allowed more than 1e-5 of its largest entry (the oracle sits 1e-7 .. 8e-7 from fp64 on this table).
ANCHOR_M, ANCHOR_F, ANCHOR_CAP = 4.0, 3e-7, 1e-5


def anchor_bound(ref64, ref32):
    scale = float(ref64.abs().max())
    e_o32 = float((ref32 - ref64).abs().max())
    return min(ANCHOR_M * e_o32 + ANCHOR_F * scale, ANCHOR_CAP * scale), e_o32, scale


def forward_drop_last_row(emb, params, drop):
    """The recurrence of set2set_forward restated with the attention of every step running over the first n - 1 rows
    only when `drop` (a one-row error, as a tail loop that stops one row early would make it)."""
    B, n, d = emb.shape
    rows = emb[:, :n - 1] if drop else emb
    h, c, qs = emb.new_zeros(B, d), emb.new_zeros(B, d), emb.new_zeros(B, 2 * d)
    for _ in range(n):
        h, c = O.lstm_cell(qs, h, c, params["lstm.weight_ih_l0"], params["lstm.weight_hh_l0"],
                           params["lstm.bias_ih_l0"], params["lstm.bias_hh_l0"])
        a = torch.softmax(torch.einsum("bnd,bd->bn", rows, h), dim=1)
        qs = torch.cat([h, torch.einsum("bn,bnd->bd", a, rows)], dim=1)
    return torch.relu(torch.nn.functional.linear(qs, params["pred.weight"], params["pred.bias"]))
