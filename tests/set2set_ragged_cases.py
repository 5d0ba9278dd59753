"""The case table of the ragged Set2Set entries (dp_set2set_ragged_*, csrc/dp_set2set_ragged.hip), shared by
test_set2set_ragged_cpu.py and test_gpu_set2set_ragged.py: seeded inputs, the CPU references and a restatement of the
recurrence on ragged rows that can be made wrong on purpose.

A row is (sizes, T, d, kind): graph b has sizes[b] real rows, the batch stands for the dense batch zero-padded to T rows
(T steps, T-row softmax), d is the Set2Set width.  Inputs as set2set_cases.make_inputs: 0.3 * randn embedding, parameters
uniform in +-1/sqrt(d), upstream gradient randn.  kind 'neg' makes every real logit negative at every step: the
embedding is made positive (0.9 * |randn| + 0.15) and the bias of the cell gate g is -3, so c_t < 0 and h_t < 0 throughout
and e_i = emb_i . h_t < 0 (test_set2set_ragged_cpu.py asserts it of the reference).

References: oracle.diffpool_oracle.set2set_forward on the zero-padded [B, T, d] batch (ragged_base_cases.pad_rows) in
float64 and float32, gradients by autograd, demb unpadded.  Bound: set2set_cases.anchor_bound.

What each row is there for:
  n_b = 1 beside larger graphs at T = 20               the padded term P exp(-m) dominates Z
  every n_b = T with negative logits ('neg')           P = 0: the maximum must NOT be clamped at 0
  'neg' with P > 0                                     the clamp matters: all real logits far below the padded rows' 0
  15 | 16 | 17 and 63 | 64 | 65                        sixteen-lane team and wave edges of the row loops
  edge | edge + 1 at d = 64 and d = 256                the row count at which the embedding leaves LDS, read from
                                                       dp_set2set_ragged_plan (weights in registers / in global memory)
  1100 beside 5                                        past the dense kernels' 1024 rows; a thread owns two rows
  T > max n_b                                          pad_to above the largest graph
  d 64 | 65, 69 | 70, 128 | 129, 256                   the dense kernels' weight-placement edges and the gate loop's passes
  B = 1, P = 0                                         a single CsrGraph
"""
import functools

import torch

from graph_pooling_amd import _lib
from oracle import diffpool_oracle as O
from tests import ragged_base_cases as RC
from tests.set2set_cases import PARAM_KEYS, TENSORS, anchor_bound  # noqa: F401  (the bound is imported, not restated)

E_LDS, W_REGS = 2, 4                       # bits of dp_set2set_ragged_plan (include/diffpool_hip.h); bit 0 is never set
VARIANTS = {W_REGS | E_LDS: "WF+EL", W_REGS: "WF", E_LDS: "WG+EL", 0: "WG"}
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
MAX_ROWS = 16384                           # DP_SET2SET_RAGGED_MAX_ROWS


@functools.lru_cache(maxsize=None)
def el_edge(d):
    """The largest n_b whose embedding is staged in LDS at width d, asked of dp_set2set_ragged_plan (bisection: the
    LDS need grows with n_b)."""
    plan = _lib.load().dp_set2set_ragged_plan
    assert plan(1, d) & E_LDS and not plan(MAX_ROWS, d) & E_LDS
    lo, hi = 1, MAX_ROWS
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid, d) & E_LDS else (lo, mid)
    return lo


def _cases():
    e64, e256 = el_edge(64), el_edge(256)
    return [
        ((1, 9, 14), 20, 12, ""),
        ((7, 7, 7), 7, 12, "neg"),
        ((5, 12), 20, 12, "neg"),
        ((15, 16, 17), 17, 20, ""),
        ((63, 64, 65), 65, 8, ""),
        ((e64, e64 + 1, 3), e64 + 1, 64, ""),
        ((e256 + 1, e256), e256 + 1, 256, ""),
        ((1100, 5), 1100, 8, ""),
        ((10, 13), 20, 16, ""),
        ((5, 12), 12, 65, ""),
        ((6, 11), 11, 69, ""),
        ((11, 6), 11, 70, ""),
        ((4, 9), 9, 128, ""),
        ((9, 4), 9, 129, ""),
        ((23,), 23, 12, ""),
    ]


CASES = _cases()
# Rows on which the wrong restatements are checked.  The recurrence contracts towards a fixed point — by T = 40 one step
# more or less moves the output by 1e-10 — so every short row keeps T <= 23, where a missing step still shows.
SHORT = [c for c in CASES if c[1] <= 64]


def case_id(case):
    sizes, T, d, kind = case
    return "n" + "_".join(map(str, sizes)) + f"-T{T}-d{d}" + ("-" + kind if kind else "")


def make_inputs(sizes, T, d, kind=""):
    """(emb [n_total, d], params, gout [B, d]), float32, seeded by the row."""
    n_total, B = sum(sizes), len(sizes)
    g = torch.Generator().manual_seed(7919 * n_total + 31 * T + d)
    emb = 0.3 * torch.randn(n_total, d, generator=g)
    shapes = ((4 * d, 2 * d), (4 * d, d), (4 * d,), (4 * d,), (d, 2 * d), (d,))
    a = 1.0 / d ** 0.5
    params = {k: (torch.rand(s, generator=g) * 2 - 1) * a for k, s in zip(PARAM_KEYS, shapes)}
    gout = torch.randn(B, d, generator=g)
    if kind == "neg":
        emb = 3.0 * emb.abs() + 0.15
        params["lstm.bias_ih_l0"][2 * d:3 * d] = -3.0
    return emb, params, gout


def reference(case, dtype):
    """oracle.set2set_forward on the zero-padded batch and its gradients, in `dtype`, returned in float64."""
    sizes, T, d, kind = case
    emb, params, gout = make_inputs(*case)
    e = emb.to(dtype).requires_grad_(True)
    P = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    out = O.set2set_forward(RC.pad_rows(e, sizes, T), P)
    (out * gout.to(dtype)).sum().backward()
    res = {"out": out.detach().double(), "demb": e.grad.double()}
    res.update({k: P[k].grad.double() for k in PARAM_KEYS})
    return res


@functools.lru_cache(maxsize=None)
def case_references(case):
    """(inputs, fp64 reference, fp32 oracle) of a table row; computed once per process, never modified."""
    return make_inputs(*case), reference(case, torch.float64), reference(case, torch.float32)


def restated(emb, sizes, T, params, wrong="", logits=None):
    """The recurrence on RAGGED rows as diffpool_hip.h states it (graph b: its n_b rows, T steps, P_b = T - n_b zero
    rows as one term of the softmax denominator) -> out [B, d].  `wrong` makes one of three mistakes:
      'pad-1'    P_b - 1 padded rows in Z
      'noclamp'  the real rows are shifted by the unclamped max_i e_i while the padded term keeps exp(-max(m, 0)): the
                 clamp forgotten in one of its two places (shifting BOTH by the unclamped maximum is the same softmax)
      'steps-1'  T - 1 steps
    `logits`: a list that receives every step's real logits."""
    outs, o = [], 0
    w_ih, w_hh = params["lstm.weight_ih_l0"], params["lstm.weight_hh_l0"]
    b_ih, b_hh = params["lstm.bias_ih_l0"], params["lstm.bias_hh_l0"]
    for n in sizes:
        E = emb[o:o + n]
        o += n
        d = E.shape[1]
        P = T - n
        h, c, qs = E.new_zeros(1, d), E.new_zeros(1, d), E.new_zeros(1, 2 * d)
        for _ in range(T - 1 if wrong == "steps-1" else T):
            h, c = O.lstm_cell(qs, h, c, w_ih, w_hh, b_ih, b_hh)
            e = E @ h[0]
            if logits is not None:
                logits.append(e.detach())
            m_real = e.max()
            m = torch.clamp(m_real, min=0.0) if P > 0 else m_real
            p = torch.exp(e - (m_real if wrong == "noclamp" else m))
            Z = p.sum() + (P - 1 if wrong == "pad-1" else P) * torch.exp(-m)
            r = (p / Z) @ E
            qs = torch.cat([h, r[None]], dim=1)
        outs.append(torch.relu(torch.nn.functional.linear(qs, params["pred.weight"], params["pred.bias"])))
    return torch.cat(outs, dim=0)
