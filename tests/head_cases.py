"""Cases, training step and fp64 references shared by tests/test_gpu_head.py, its child process (tests/_head_worker.py)
and tests/test_head_cases_cpu.py: small models whose prediction head runs the two kernels of csrc/dp_head.hip --
k_head_fwd (the last pooled level's max readout + all of pred_model, one workgroup per graph) and k_head_bwd
(pred_model's backward + the max-readout scatter of every level, one workgroup per slice of HEAD_SLICE = 16 features) --
at a chosen (B, n, readout width, pred widths), everything below the head as small as it can be.

Family P -- SoftPoolingGcnEncoder(N = n 2^P, F = 3, H, E, C, L, H, assign_ratio 0.5, num_pooling P, linkpred False):
the levels have N, N/2, .., n rows, every level reads out rw = H(L-1)+E columns and d0 = rw (P+1).  The head kernel
reads the LAST level's embedding itself (HeadArgs::Z != null): one pass when rw <= 64 and n <= 64, else the looped form.
Family B -- GcnEncoderGraph(F = 3, H, E, C, L, hidden, concat): no pooled level, so Z == null and the forward kernel is
the MLP alone; d0 = H(L-1)+E (concat) or E (concat=False: DP_F_LAST_ONLY, the dZ pointer offset by the last layer's
column while ldz stays D).  No fold is possible there: k_head_bwd runs without any knob.

The plan, restated from dp_head.hip / dp_model.hip (dims = [d0, hidden.., C], nP = len(dims) - 1):
  head_fwd_lds_floats = sum dims[i] dims[i+1] + sum dims[1:] + 2 max(dims) + 512              <= 30 * 1024
  head_bwd_lds_floats = wup + B hup + 16 dims[1] + 16 B + 2 B max(dims[1:])                   <= 38 * 1024
                        (wup = sum_{i>=1} dims[i] dims[i+1], hup = sum dims[1:nP])
  head_supported:       1 <= B <= 1024 and both limits                                        (else `generic`, both ways)
  forward  `fused`:     head_supported -> one k_head_fwd;  `generic`: the GEMM head, no k_head_fwd
  backward `fold`:      family P, the last level on the whole-level tier (small_level_cases.planned_tier) and
                        small_head_fold_fits -> no k_head_bwd, one k_reduce_slabs_head
           `kernel`:    head_supported otherwise -> one k_head_bwd (every `fold` case under DP_NO_HEAD_FOLD=1)
           `generic`:   not head_supported -> neither
The bias-tail loop `e >= 4096` of k_head_fwd (zero-fill of a bias-free layer wider than one staging round) is
unreachable from these models: it needs a layer width d1 > 4096, and the backward LDS limit excludes that (16 d1 alone
is 65 552 floats).  No case is invented for it.  A head layer WITHOUT bias (pred_b_off < 0) is not reachable through the
modules either: the flat-parameter code (GcnEncoderGraph._tail_params) takes `lin.bias` of every Linear of pred_model
and fails on None, so the table has no such case.

Special cases: `tie` zeroes the last GraphConv weight of the last level, so every row of that column block is the same
normalised bias and every winner there must be row 0; `neg` is a ragged batch (n_min 1) in which some level-0 column has
a negative maximum over the real nodes, so a masked zero row holds it and the winner is -1; `nobias` builds the GCN stack
without biases (args.bias False) on full graphs with a dense adjacency, as small_level_cases does: the 4090-wide layer
of b_d4097 is past what the generic rownorm_bwd takes WITH a bias gradient (16 column sums of the layer's width in LDS:
the library answers "rownorm_bwd: invalid argument"), and the head under test is the same either way.

References, both fp64 and both on the model's fp32 parameters cast up:
  (2) the head alone, on the GPU's own inputs: readout features gathered from the saved embeddings and winners of every
      level (-1 -> 0) -> pred_model -> cross entropy, with autograd.  Compared: ypred and every pred_model gradient, each
      within max(FACTOR e_ref, FLOOR max|ref|), e_ref the max abs difference from fp64 of the same graph in fp32 torch on
      the CPU (FACTOR, FLOOR of tests/small_level_cases.py);
  (3) the whole model, with the GPU's winners forced in, at tests/parity.py's tolerances: the check of the d(features)
      scatter, which reaches the stack parameters of every level only through dZ."""
import collections
import types

import torch

from graph_pooling_amd.encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests import small_level_cases as SC
from tests.small_level_cases import ASSIGN_SHARPEN, FACTOR, FLOOR

HEAD_FWD_LDS_FLOATS = 30 * 1024
HEAD_BWD_LDS_FLOATS = 38 * 1024
HEAD_SLICE = 16
STAGE_ROUND = 4096                # floats one stage_issue / stage_commit round moves (256 threads x 16)
B_LIMIT = 1024
F = 3

Case = collections.namedtuple("Case", "name fam B n H E L P hidden C concat fwd bwd seed special")

#     name               fam  B     n   H     E   L  P  hidden         C  concat fwd        bwd        seed special
CASES = [
    # ---- family P: the readout forms of k_head_fwd
    Case("p_n1_rw5_lin",    "P", 3,    1,  2,    3,  2, 1, (),            2, True,  "fused",   "fold",    1, None),   # d0 10, L = 1
    Case("p_n5_rw13_h3_5",  "P", 2,    5,  4,    5,  3, 1, (3, 5),        2, True,  "fused",   "fold",    1, None),   # d0 26
    Case("p_n64_rw64_h65",  "P", 2,    64, 32,   32, 2, 1, (65,),         3, True,  "fused",   "kernel",  1, None),   # d0 128: too wide to fold
    Case("p_n65_rw64_deep", "P", 2,    65, 32,   32, 2, 1, (9, 8, 7, 6),  2, True,  "fused",   "kernel",  1, None),   # looped: n
    Case("p_n16_rw65",      "P", 2,    16, 32,   33, 2, 1, (),            2, True,  "fused",   "fold",    1, None),   # looped: rw
    Case("p_n2_rw130",      "P", 2,    2,  43,   44, 3, 1, (),            2, True,  "fused",   "fold",    3, None),   # d0 260
    Case("p_tie",           "P", 3,    4,  4,    4,  3, 1, (7, 5),        2, True,  "fused",   "fold",    1, "tie"),  # d0 24
    Case("p_pool2_rw21",    "P", 2,    3,  10,   11, 2, 2, (7, 5),        2, True,  "fused",   "fold",    1, None),   # d0 63
    Case("p_neg",           "P", 6,    4,  4,    4,  3, 1, (),            2, True,  "fused",   "fold",    1, "neg"),  # d0 24
    # ---- staging rounds and MLP passes
    Case("p_d64_h64",       "P", 2,    3,  16,   16, 2, 1, (64,),         2, True,  "fused",   "fold",    1, None),   # W0 4096
    Case("p_b64_h70_65",    "P", 64,   2,  4,    4,  2, 1, (70, 65),      2, True,  "fused",   "fold",    1, None),   # 4550 / 4480
    # forward LDS: 26 d1 + 2 d1 + d1 + 2 + 2 d1 + 512 = 31 d1 + 514: d1 = 974 -> 30 708, d1 = 975 -> 30 739
    Case("p_fwd_edge_in",   "P", 2,    5,  4,    5,  3, 1, (974,),        2, True,  "fused",   "fold",    1, None),
    Case("p_fwd_edge_out",  "P", 2,    5,  4,    5,  3, 1, (975,),        2, True,  "generic", "generic", 1, None),
    # ---- family B
    Case("b_d17_h241",      "B", 2,    6,  8,    9,  2, 0, (241,),        2, True,  "fused",   "kernel",  1, None),   # W0 4097
    Case("b_last_h257",     "B", 3,    7,  5,    16, 3, 0, (257,),        2, False, "fused",   "kernel",  1, None),   # cW0 4112
    Case("b_d4097",         "B", 2,    8,  4090, 7,  2, 0, (),            2, True,  "fused",   "kernel",  1, "nobias"),  # 257 slices
    Case("b_b1",            "B", 1,    6,  4,    4,  2, 0, (7, 5),        2, True,  "fused",   "kernel",  1, None),   # d0 8
    Case("b_b32",           "B", 32,   4,  8,    8,  2, 0, (5,),          3, True,  "fused",   "kernel",  1, None),   # B ks 512
    Case("b_b33",           "B", 33,   4,  8,    8,  2, 0, (5,),          3, True,  "fused",   "kernel",  1, None),   # B ks 528
    Case("b_b257",          "B", 257,  4,  8,    9,  2, 0, (),            2, True,  "fused",   "kernel",  1, None),   # 16 B 4112
    Case("b_b1024_c5",      "B", 1024, 4,  8,    8,  2, 0, (),            5, True,  "fused",   "kernel",  1, None),   # B C 5120
    Case("b_b1025",         "B", 1025, 4,  8,    8,  2, 0, (),            5, True,  "generic", "generic", 1, None),
    # backward LDS at B = 1024, C = 2: 2 d1 + 1024 d1 + 16 d1 + 16 384 + 2048 d1: d1 = 7 -> 38 014, d1 = 8 -> 41 104
    Case("b_bwd_edge_in",   "B", 1024, 4,  8,    8,  2, 0, (7,),          2, True,  "fused",   "kernel",  1, None),
    Case("b_bwd_edge_out",  "B", 1024, 4,  8,    8,  2, 0, (8,),          2, True,  "generic", "generic", 1, None),
]
# seed: chosen on the references alone (tests/test_head_cases_cpu.py) -- the fp64 head keeps every hidden pre-activation
# 1e-5 from ReLU's kink, and the whole model is conditioned well enough that fp32 torch on the CPU stays within 0.75 of
# tests/parity.py's gradient tolerances of fp64 (p_n2_rw130 at seed 1 is not: its level-0 assignment gradients are
# ~1e-4 and the fp32 CPU oracle itself misses the 1e-7 floor there).
CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
FOLD = [c.name for c in CASES if c.bwd == "fold"]
# the float counts quoted above: {case: (formula, floats)}
QUOTED = {
    "p_fwd_edge_in": ("fwd", 30708), "p_fwd_edge_out": ("fwd", 30739),
    "b_bwd_edge_in": ("bwd", 38014), "b_bwd_edge_out": ("bwd", 41104),
}
# model.predict on a model whose last Linear has weight 0 and bias PREDICT_TIE_BIAS: the logits ARE the bias, classes 1
# and 2 tie, and the first index must win
PREDICT_TIE = "b_b33"
PREDICT_TIE_BIAS = (0.5, 0.7, 0.7)


# ------------------------------------------------------------------ the plan formulas (dp_head.hip), restated
def readout_width(c):
    return c.H * (c.L - 1) + c.E if (c.fam == "P" or c.concat) else c.E


def pred_dims(c):
    return [readout_width(c) * (c.P + 1)] + list(c.hidden) + [c.C]


def level_nodes(c):
    """Rows of every level, level 0 first."""
    return [c.n * 2 ** (c.P - j) for j in range(c.P + 1)]


def head_fwd_lds_floats(dims):
    return sum(a * b for a, b in zip(dims, dims[1:])) + sum(dims[1:]) + 2 * max(dims) + 512


def head_bwd_lds_floats(B, dims):
    nP = len(dims) - 1
    wup = sum(dims[i] * dims[i + 1] for i in range(1, nP))
    hup = sum(dims[1:nP])
    return wup + B * hup + HEAD_SLICE * dims[1] + HEAD_SLICE * B + 2 * B * max(dims[1:])


def head_supported(B, dims):
    return (len(dims) >= 2 and 1 <= B <= B_LIMIT and head_fwd_lds_floats(dims) <= HEAD_FWD_LDS_FLOATS and
            head_bwd_lds_floats(B, dims) <= HEAD_BWD_LDS_FLOATS)


def sc_case(c):
    """The case as tests/small_level_cases.py describes one (its last level, BatchNorm and biases on)."""
    return SC.Case(c.name, c.fam, c.B, c.n, F, c.H, c.E, c.L, True, c.special != "nobias", c.concat, c.hidden, c.C, "",
                   c.seed)


def last_level_tier(c):
    return SC.planned_tier(sc_case(c))


def planned(c, no_head_fold=False):
    """(forward plan, backward plan) of the head."""
    dims = pred_dims(c)
    if not head_supported(c.B, dims):
        return "generic", "generic"
    fold = (not no_head_fold and c.fam == "P" and last_level_tier(c) == "whole" and
            SC.lds_level_bwd(c.n, SC.level_dims(sc_case(c))) + SC.lds_head(dims) <= SC.LIM)
    return "fused", "fold" if fold else "kernel"


def one_pass(c):
    """k_head_fwd keeps the level's rows in registers: family P with rw <= 64 and n <= 4 * 16."""
    return c.fam == "P" and readout_width(c) <= 64 and c.n <= 64


def stage_rounds(cnt):
    return -(-cnt // STAGE_ROUND)


# ------------------------------------------------------------------ models and the step
def build(name, predict_tie=False):
    """(model on the CPU with the case's fp32 parameters loaded, params, x, adj, num_nodes, label)."""
    c = CASE[name]
    N = level_nodes(c)[0]
    if c.fam == "P":
        n_min = 1 if c.special == "neg" else max(1, N // 2)
        x, adj, nn_, label = O.make_batch(c.B, N, F, n_min=n_min, p=0.3, seed=c.seed, n_classes=c.C)
        model = SoftPoolingGcnEncoder(N, F, c.H, c.E, c.C, c.L, c.H, assign_ratio=0.5, num_pooling=c.P,
                                      pred_hidden_dims=list(c.hidden), linkpred=False)
    else:
        full = c.special == "nobias"
        x, adj, nn_, label = O.make_batch(c.B, N, F, n_min=N if full else max(1, N // 2), p=0.6 if full else 0.3,
                                          seed=c.seed, n_classes=c.C)
        model = GcnEncoderGraph(F, c.H, c.E, c.C, c.L, pred_hidden_dims=list(c.hidden), concat=c.concat, bn=True,
                                args=types.SimpleNamespace(bias=not full))
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=c.seed, bias_scale=0.1)
    for k in params:
        if k.startswith("assign_pred") and k.endswith(".weight"):
            params[k] = params[k] * ASSIGN_SHARPEN
    if c.special == "tie":
        params["conv_last2.weight"] = torch.zeros_like(params["conv_last2.weight"])
    if predict_tie:
        k = last_linear(c)
        params[k + ".weight"] = torch.zeros_like(params[k + ".weight"])
        params[k + ".bias"] = torch.tensor(PREDICT_TIE_BIAS)
    model.load_state_dict(params)
    return model, params, x, adj, nn_, label


def last_linear(c):
    return f"pred_model.{2 * len(c.hidden)}" if c.hidden else "pred_model"


def call(model, c, xd, ad, nn_, predict=False):
    fn = model.predict if predict else model
    return fn(xd, ad, nn_, assign_x=xd) if c.fam == "P" else fn(xd, ad, nn_)


def step(model, c, xd, ad, nn_, ld):
    """One forward + loss + backward; (ypred, loss) -- the gradients are on the parameters."""
    model.zero_grad(set_to_none=True)
    y = call(model, c, xd, ad, nn_)
    loss = model.loss(y, ld)
    loss.backward()
    return y, loss


def results(model, c, y):
    """What a GPU run of a case leaves for the checks: ypred, every gradient ("grad." + name), the saved embedding and
    readout arg-max of every level."""
    out = {"ypred": y.detach().cpu().clone()}
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.detach().cpu().clone()
    for j in range(c.P + 1):
        out[f"emb{j}"] = model.saved_activation(j, "embedding").detach().cpu().clone()
        out[f"argmax{j}"] = model.saved_activation(j, "readout_argmax").detach().cpu().clone()
    return out


def head_names(params):
    return [k for k in params if k.startswith("pred_model")]


def loose_names(model, c):
    """Gradients a bit comparison between two runs leaves to rounding (rtol 1e-5 / atol 1e-7), by rule as
    small_level_cases.loose_names and head_grads_final_cases.atomic_bias_names name them: the generic per-phase sequence
    sums GraphConv bias gradients and the assign_pred bias gradient with float atomics.  Every level below the last (it
    carries two stacks, or runs the persistent kernels whose ordered sums pass the looser check as well), and the last
    level when its tier is `generic`.  Never a pred_model gradient."""
    ids = set()
    tier = last_level_tier(c)
    for kind, level, mods in model._graph_param_groups():
        if not (kind == "embed" and level == c.P) or tier == "generic":
            mods = [mods] if kind == "assign_pred" else mods
            ids |= {id(m.bias) for m in mods if m.bias is not None}
    return tuple("grad." + k for k, p in model.named_parameters() if id(p) in ids)


# ------------------------------------------------------------------ the references
def readout_block(c, z):
    """The columns of a level's embedding the readout takes."""
    return z if (c.fam == "P" or c.concat) else z[:, :, z.shape[2] - c.E:]


def readout_rows(c, j, z, nn_):
    """The block the max readout of level j ranges over: level 0 of family P is masked AT the readout (rows past
    num_nodes count as zeros), while the save buffer keeps those rows as the stack computed them."""
    z = readout_block(c, z)
    if c.fam == "P" and j == 0:
        real = torch.arange(z.shape[1]).view(1, -1, 1) < torch.as_tensor(nn_).view(-1, 1, 1)
        z = torch.where(real, z, torch.zeros((), dtype=z.dtype))
    return z


def lowest_row_of_max(z):
    """(column maxima [B, D], lowest row holding each) of z [B, n, D], exact."""
    top = z.max(dim=1)[0]
    rows = torch.arange(z.shape[1]).view(1, -1, 1).expand_as(z)
    first = torch.where(z == top.unsqueeze(1), rows, torch.full_like(rows, z.shape[1])).min(dim=1)[0]
    return top, first.to(torch.int32)


def features(c, got, dtype):
    """Readout features [B, d0] from the saved embeddings and winners of `got` (-1: the constant 0)."""
    return torch.cat([SC.readout(readout_block(c, got[f"emb{j}"]).to(dtype), got[f"argmax{j}"])
                      for j in range(c.P + 1)], dim=1)


def winners(c, got):
    return [got[f"argmax{j}"] for j in range(c.P + 1)]


def head_alone(c, params, label, got, dtype):
    """Reference (2) in `dtype`: {"ypred", "grad." + name for every pred_model parameter, "pre": hidden pre-activations}."""
    names = head_names(params)
    P = {k: params[k].to(dtype).clone().requires_grad_(True) for k in names}
    feat = features(c, got, dtype)
    y = O.mlp_head(feat, P, "pred_model", len(c.hidden))
    torch.nn.functional.cross_entropy(y, label).backward()
    out = {"ypred": y.detach(), "pre": [t.detach() for t in SC.head_pre(P, feat, len(c.hidden))]}
    out.update({"grad." + k: P[k].grad for k in names})
    return out


def head_figures(c, params, label, got):
    """Check (2) of one run: [(tensor, kernel error, e_ref, bound, max|ref|)] for ypred and every pred_model gradient;
    nothing is left out.  Errors are max abs differences from the fp64 reference."""
    r64 = head_alone(c, params, label, got, torch.float64)
    r32 = head_alone(c, params, label, got, torch.float32)
    rows = []
    for k in ["ypred"] + ["grad." + n for n in head_names(params)]:
        ref = r64[k]
        e_ref = float((r32[k].double() - ref).abs().max())
        scale = float(ref.abs().max())
        rows.append((k, float((got[k].double() - ref).abs().max()), e_ref, max(FACTOR * e_ref, FLOOR * scale), scale))
    return rows


failures = SC.failures


def end_to_end(c, params, x, adj, nn_, label, win, dtype=torch.float64):
    """Reference (3): (ypred, loss, {name: gradient}) of the whole model with `win` (a list per level, or None)."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x, adj = x.to(dtype), adj.to(dtype)
    if c.fam == "P":
        y, _ = O.softpool_forward(P, x, adj, nn_, x, num_layers=c.L, num_pooling=c.P, n_pred_hidden=len(c.hidden),
                                  bn=True, winners=win)
    else:
        y = SC.base_forward(sc_case(c), P, x, adj, None if win is None else win[0])[0]
    loss = torch.nn.functional.cross_entropy(y, label)
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in P.items()}


def parity_ratio(ref_grads, grads, rtol=1e-3, atol_rel=2e-5):
    """(largest |difference| / allowed, its tensor) under tests/parity.py's grads_close tolerances."""
    worst = (0.0, "")
    for k, g in ref_grads.items():
        allowed = max(1e-7, atol_rel * float(g.abs().max())) + rtol * g.abs()
        worst = max(worst, (float(((grads[k].double() - g.double()).abs() / allowed).max()), k))
    return worst


def oracle_got(c, params, x, adj, nn_, dtype=torch.float32):
    """The embeddings and winners `results` gives, from the CPU oracle in `dtype` with its own arg-max in place of a GPU
    run (lowest row on ties; at level 0 of family P a winning masked row is recorded as -1, as the library does)."""
    P = {k: v.to(dtype) for k, v in params.items()}
    x, adj = x.to(dtype), adj.to(dtype)
    keys0 = O._stack_keys("conv_first", "conv_block", "conv_last", c.L)
    if c.fam == "B":
        zs = [SC.stack_forward(x, adj, P, keys0, True, not c.concat)[0]]
    else:
        _, inter = O.softpool_forward(P, x, adj, nn_, x, num_layers=c.L, num_pooling=c.P, n_pred_hidden=len(c.hidden),
                                      bn=True, want_intermediates=True)
        zs = [O.gcn_stack(x, adj, P, keys0, O.node_mask(x.shape[1], nn_, dtype), True)]
        for i in range(c.P):
            zs.append(O.gcn_stack(inter[f"xpool_{i}"], inter[f"adjpool_{i}"], P, O.level_keys(i, c.P, c.L)[0], None, True))
    got = {}
    for j, z in enumerate(zs):
        first = lowest_row_of_max(readout_block(c, z))[1]
        if c.fam == "P" and j == 0:
            first = torch.where(first >= torch.as_tensor(nn_).view(-1, 1), torch.full_like(first, -1), first)
        got[f"emb{j}"], got[f"argmax{j}"] = z, first
    return got
