"""Cases, training step and fp64 references shared by tests/test_gpu_small_level.py, its child process
(tests/_small_level_worker.py) and tests/test_small_level_cases_cpu.py: small models whose level under test runs the
one-workgroup-per-graph kernels of csrc/dp_small.hip (k_small_level_fwd/bwd, the whole-level tier, and
k_small_gcn_fwd/bwd, the per-layer tier) at a chosen (B, n, dims, L, flags), everything else as small as it can be.

Family P -- the last pooled level of DiffPool: SoftPoolingGcnEncoder(N = 2n, F, H, E, C, L, H, assign_ratio 0.5,
num_pooling 1, linkpred False).  K = int(2n * 0.5) = n exactly and the level's dims are [H(L-1)+E, H, .., H, E].  The
batches are O.make_batch(..., n_min = max(1, n)): ragged at level 0, never empty.  BatchNorm off is reached through
NoBatchNormEncoder (the constructor always builds BatchNorm, as the reference does).  The constructor refuses
concat=False, so add_self is NOT reachable on a pooled level; and it always builds biases.

Family B -- level 0 of the base encoder: GcnEncoderGraph(F, H, E, C, L, pred_hidden_dims, concat, bn) at N = n, dims
[F, H, .., H, E].  It brings add_self (concat=False: also the last-layer-only readout), raw feature widths up to 256 as
dims[0], a stack without biases (args.bias False) and the backward with no input gradient (dX0 and dadj are null at
level 0).  Family B keeps n < 64 unless add_self is set: at N = 64 a plain level 0 is the persistent level-0 kernels'
(dp_model.hip encoder_plan), not dp_small.hip's.  Rows past num_nodes are ordinary nodes there (the base forward never
masks), so a stack WITHOUT biases gets full graphs and a dense adjacency: a zero row would sit exactly on ReLU's kink.

Expected tier (`whole`, `per_layer`, `generic`), derived by hand from dp_small.hip; LIM = 150 KiB = 38 400 floats:
  per-layer fwd(B,n,di,do) = n^2 + n di + di do + 2 n do + 2n + do + 2Bn + 16
  per-layer bwd(B,n,di,do) = 2n^2 + 2 n di + di do + 4 n do + 4n + 17 do + 2Bn + 16
  small_level_supported:    n <= 64, di, do <= 256, max(fwd, bwd) <= LIM          (every layer, else `generic`)
  level fwd  = n^2 + n dmax + 2 n omax + 2n + wtot + btot + 80                    (dmax over dims[:L], omax over dims[1:])
  level bwd  = 2n^2 + n d0 + 2 n D + (L-1) n omax + wtot + 2Ln + 3 n omax + 2n + 17 omax + 80   (D = sum dims[1:])
  small_level_fused_ok:     2 <= L <= 8, n <= 64, dims[0] <= 256, dims[l > 0] <= 64, both <= LIM,
                            B <= min(128, CUs // 2)                                (else `per_layer`)
  small_head_fold_fits:     level bwd + d1 d0 + wup + 2 hup + C <= LIM             (else k_head_bwd stays; still `whole`)
The tier is planned with the adjacency gradient counted (dadj = true) at every level, level 0 included.
level bwd - level fwd = n^2 + n (d0 + 2D + L omax - dmax) + 2Ln + 17 omax - btot > 0 always (d0 + D >= dmax, and
btot <= L omax <= 8 omax < 17 omax), so the whole-level FORWARD formula never decides a tier: no case can sit on
its boundary, and the table has none.  The backward's and the per-layer boundaries are the *_edge cases.
The functions lds_* below restate the formulas for tests/test_small_level_cases_cpu.py, which checks every tier and every
quoted float count of the table against them; the GPU test checks the table against the kernel trace.

Cases left out of the backward level check (ii), DROP_BWD: a last layer of width 1 has the exact gradient zero for its
own weight and bias (d/dy of y/|y| vanishes), so both yardstick and floor are zero there and the bound cannot be met
by rounding; every other check still runs on it.

References, both fp64 and both on the fp32 parameters of the model cast up (the GPU's own values):
  (i)  end to end: O.softpool_forward (family P) or the base forward written out below from O.graph_conv, O.bn_node and
       O.mlp_head (family B; O.base_forward takes no winners), with the HIP forward's max-readout winners forced in,
       after `check_winners` has shown that each holds the fp64 column maximum to 1e-6 of the column's largest entry;
  (ii) the level alone, on the GPU's own inputs: xpool / adjpool of level 0 read back from the save buffer (family P) or
       x / adj themselves (family B) -> stack -> forced-winner readout -> concatenation with the other level's readout
       features (recomputed from the GPU's saved level-0 embedding and arg-max) -> head -> cross entropy.  Leaves: the
       level's stack parameters and pred_model's.  The same graph in fp32 with torch on the CPU gives the yardstick
       e_ref (max abs difference from fp64, per tensor); the kernel passes a tensor when its own max abs difference is
       at most max(8 e_ref, 16 * 2^-24 * max|ref|).  The save buffer keeps the embedding of every level in training
       mode, so the forward compares the embedding itself."""
import collections
import types

import torch

from graph_pooling_amd.encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O

LIM = 150 * 1024 // 4            # floats of LDS a one-workgroup-per-graph kernel may ask for
BMAX_MI355X = 128                # min(128, CUs // 2) at 256 CUs; the GPU test reads the CU count at run time
FACTOR, FLOOR = 8.0, 16.0 * 2.0 ** -24
# Family P multiplies assign_pred.weight by this.  At the reference's initialisation the soft assignment is nearly
# uniform and the pooled rows are equal to ~1e-4: the columns of the pooled level then tie within fp32 rounding (no
# run's winners hold the fp64 maximum to 1e-6) and the whole model is conditioned 10-100 times worse than with the
# sharp assignment of a trained model, which this stands for.
ASSIGN_SHARPEN = 32.0

Case = collections.namedtuple("Case", "name fam B n F H E L bn bias concat hidden C tier seed")

# B: an int, or "bmax" / "bmax+1" (resolved by `batch_size`).  seed: chosen so that the fp64 reference alone keeps every
# pre-ReLU value of the level and of the head 1e-5 away from the kink (tests/test_small_level_cases_cpu.py).
#     name              fam  B        n   F    H    E   L  bn     bias   concat hidden  C  tier         seed
CASES = [
    # ---- family P, whole-level tier: every n*, width* and L* class
    Case("p_n1",            "P", 3,        1,  3,   5,   3,  3, True,  True,  True,  (),     2, "whole",     1),   # [13,5,5,3]
    Case("p_n15_l2",        "P", 2,        15, 3,   15,  4,  2, True,  True,  True,  (),     3, "whole",     1),   # [19,15,4]
    Case("p_n16_b15",       "P", 15,       16, 3,   16,  16, 3, True,  True,  True,  (7, 5), 2, "whole",     1),   # [48,16,16,16]
    Case("p_n17_b16",       "P", 16,       17, 3,   17,  13, 3, True,  True,  True,  (),     2, "whole",     2),   # [47,17,17,13]
    Case("p_n31_b17",       "P", 17,       31, 3,   33,  20, 3, True,  True,  True,  (),     3, "whole",     1),   # [86,33,33,20]
    Case("p_n32_l4_b1",     "P", 1,        32, 3,   20,  20, 4, True,  True,  True,  (7, 5), 2, "whole",     1),   # [80,20,20,20,20]
    # [127,63,64]: level bwd 36 598; the head (254 -> 50 -> 3) adds 50*254 + 150 + 100 + 3 = 12 953 -> 49 551 > LIM:
    # the case whose head is too large to fold (k_head_bwd stays, the level is still whole); p_n57_whole_edge, 166
    # floats under LIM, cannot take its 514-float head either
    Case("p_n33_nofold",    "P", 2,        33, 3,   63,  64, 2, True,  True,  True,  (50,),  3, "whole",     1),
    Case("p_n48_l8",        "P", 2,        48, 3,   8,   4,  8, True,  True,  True,  (),     2, "whole",     1),   # [60,8 x7,4]
    Case("p_n63_w1",        "P", 3,        63, 3,   4,   1,  3, True,  True,  True,  (),     2, "whole",     1),   # [9,4,4,1]
    Case("p_n64_h20",       "P", 5,        64, 3,   20,  20, 3, True,  True,  True,  (),     2, "whole",     1),   # [60,20,20,20]: bwd 29 044
    Case("p_n16_w64_nobn",  "P", 2,        16, 3,   64,  63, 2, False, True,  True,  (7, 5), 2, "whole",     1),   # [127,64,63]
    Case("p_b32_nobn",      "P", 32,       4,  3,   8,   8,  3, False, True,  True,  (7, 5), 2, "whole",     1),
    Case("p_b33_l4_nobn",   "P", 33,       8,  3,   4,   3,  4, False, True,  True,  (),     3, "whole",     1),   # [15,4,4,4,3]
    Case("p_bmax",          "P", "bmax",   4,  3,   8,   8,  3, True,  True,  True,  (),     2, "whole",     1),
    # ---- family P, the plan boundaries
    Case("p_bmax1",         "P", "bmax+1", 4,  3,   8,   8,  3, True,  True,  True,  (),     2, "per_layer", 1),   # B > Bmax
    # [96,32,32,32]: level bwd = 2n^2 + 456n + 5744: n = 57 -> 38 234 <= LIM, n = 58 -> 38 920 > LIM
    Case("p_n57_whole_edge", "P", 2,       57, 3,   32,  32, 3, True,  True,  True,  (),     2, "whole",     1),
    Case("p_n58_whole_edge", "P", 2,       58, 3,   32,  32, 3, True,  True,  True,  (),     2, "per_layer", 1),
    Case("p_n64_h32",       "P", 2,        64, 3,   32,  32, 3, True,  True,  True,  (),     2, "per_layer", 1),   # level bwd 43 120
    # [128,64,64]: level bwd = 2n^2 + 646n + 13 456 leaves the whole tier at n = 35 (38 516); per-layer bwd of layer 0 =
    # 2n^2 + (516 + 2B) n + 9296: B = 2, n = 47 -> 38 154 <= LIM, n = 48 -> 38 864 > LIM; B = 33, n = 47 -> 41 068 > LIM
    Case("p_n47_layer_edge", "P", 2,       47, 3,   64,  64, 2, True,  True,  True,  (),     2, "per_layer", 1),
    Case("p_n48_layer_edge", "P", 2,       48, 3,   64,  64, 2, True,  True,  True,  (),     2, "generic",   1),
    Case("p_n47_b33",       "P", 33,       47, 3,   64,  64, 2, True,  True,  True,  (),     2, "generic",   1),   # the B*n*2 term
    Case("p_n64_h64",       "P", 2,        64, 3,   64,  64, 3, True,  True,  True,  (),     2, "generic",   1),   # layer 0 bwd 63 056
    Case("p_n65",           "P", 2,        65, 3,   8,   8,  3, True,  True,  True,  (),     2, "generic",   1),   # n > 64
    Case("p_e65",           "P", 2,        16, 3,   8,   65, 3, True,  True,  True,  (),     2, "per_layer", 1),   # [81,8,8,65]
    # ---- family B
    Case("b_f3_addself",    "B", 2,        17, 3,   5,   4,  3, True,  True,  False, (),     2, "whole",     2),   # [3,5,5,4]
    Case("b_f89_b32",       "B", 32,       20, 89,  20,  20, 3, True,  True,  True,  (7, 5), 2, "whole",     1),
    Case("b_f255_nobias",   "B", 2,        16, 255, 16,  17, 2, True,  False, True,  (),     3, "whole",     1),   # [255,16,17]
    Case("b_f256_l4_nobn",  "B", 3,        15, 256, 33,  16, 4, False, True,  True,  (),     2, "whole",     1),   # [256,33,33,33,16]
    Case("b_n64_addself",   "B", 2,        64, 3,   20,  20, 3, True,  True,  False, (),     2, "whole",     1),   # [3,20,20,20]
    Case("b_wide",          "B", 2,        16, 156, 100, 56, 2, True,  True,  True,  (),     2, "per_layer", 1),   # [156,100,56]: layer 0 bwd 29 348
    Case("b_f257",          "B", 2,        16, 257, 8,   8,  2, True,  True,  True,  (),     2, "generic",   1),   # din > 256
]
CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
DROP_BWD = ("p_n63_w1",)         # see the module docstring; at most three
# the float counts quoted in the comments above: {case: (formula, layer or None, floats)}
QUOTED = {
    "p_n33_nofold": ("level_bwd", None, 36598), "p_n64_h20": ("level_bwd", None, 29044),
    "p_n57_whole_edge": ("level_bwd", None, 38234), "p_n58_whole_edge": ("level_bwd", None, 38920),
    "p_n64_h32": ("level_bwd", None, 43120), "p_n47_layer_edge": ("layer_bwd", 0, 38154),
    "p_n48_layer_edge": ("layer_bwd", 0, 38864), "p_n47_b33": ("layer_bwd", 0, 41068),
    "p_n64_h64": ("layer_bwd", 0, 63056), "b_wide": ("layer_bwd", 0, 29348),
}


# ------------------------------------------------------------------ the plan formulas (dp_small.hip), restated
def level_dims(c):
    d0 = c.H * (c.L - 1) + c.E if c.fam == "P" else c.F
    return [d0] + [c.H] * (c.L - 1) + [c.E]


def batch_size(c, bmax=BMAX_MI355X):
    return {"bmax": bmax, "bmax+1": bmax + 1}.get(c.B, c.B)


def lds_layer_fwd(B, n, di, do):
    return n * n + n * di + di * do + 2 * n * do + 2 * n + do + 2 * B * n + 16


def lds_layer_bwd(B, n, di, do):
    return 2 * n * n + 2 * n * di + di * do + 4 * n * do + 4 * n + 17 * do + 2 * B * n + 16


def lds_level_fwd(n, dims):
    L = len(dims) - 1
    wtot = sum(dims[l] * dims[l + 1] for l in range(L))
    return n * n + n * max(dims[:L]) + 2 * n * max(dims[1:]) + 2 * n + wtot + sum(dims[1:]) + 80


def lds_level_bwd(n, dims):
    L, omax, D = len(dims) - 1, max(dims[1:]), sum(dims[1:])
    wtot = sum(dims[l] * dims[l + 1] for l in range(L))
    return (2 * n * n + n * dims[0] + 2 * n * D + (L - 1) * n * omax + wtot + 2 * L * n + 3 * n * omax + 2 * n +
            17 * omax + 80)


def lds_head(pred_dims):
    """SmHead::lds_floats of a head with widths pred_dims = [d0, d1, .., C]."""
    nP = len(pred_dims) - 1
    wup = sum(pred_dims[i] * pred_dims[i + 1] for i in range(1, nP))
    return pred_dims[1] * pred_dims[0] + wup + 2 * sum(pred_dims[1:nP]) + pred_dims[-1]


def planned_tier(c, bmax=BMAX_MI355X, no_level_fusion=False):
    B, n, dims = batch_size(c, bmax), c.n, level_dims(c)
    for di, do in zip(dims, dims[1:]):
        if n > 64 or di > 256 or do > 256 or max(lds_layer_fwd(B, n, di, do), lds_layer_bwd(B, n, di, do)) > LIM:
            return "generic"
    whole = (not no_level_fusion and 2 <= c.L <= 8 and dims[0] <= 256 and max(dims[1:]) <= 64 and
             lds_level_fwd(n, dims) <= LIM and lds_level_bwd(n, dims) <= LIM and B <= bmax)
    return "whole" if whole else "per_layer"


def head_folds(c, bmax=BMAX_MI355X):
    """The head backward rides in k_small_level_bwd: family P on the whole-level tier, when its operands fit."""
    if c.fam != "P" or planned_tier(c, bmax) != "whole":
        return False
    dims = level_dims(c)
    return lds_level_bwd(c.n, dims) + lds_head([2 * sum(dims[1:])] + list(c.hidden) + [c.C]) <= LIM


# ------------------------------------------------------------------ models and the step
class NoBatchNormEncoder(SoftPoolingGcnEncoder):
    """The same model with the BatchNorm flag cleared in the configuration handed to the library."""

    def _flags(self):
        return 0


def stack_keys(c):
    """state_dict prefixes of the level under test, first layer first."""
    if c.fam == "P":
        return O.level_keys(0, 1, c.L)[0]
    return O._stack_keys("conv_first", "conv_block", "conv_last", c.L)


def head_names(params):
    return [k for k in params if k.startswith("pred_model")]


def level_names(c, params):
    """Parameters whose gradients the level check (ii) compares: the level's stack and pred_model."""
    return [k for k in params if k.rsplit(".", 1)[0] in stack_keys(c)] + head_names(params)


def build(name, bmax=BMAX_MI355X):
    """(model on the CPU with the case's fp32 parameters loaded, params, x, adj, num_nodes, label)."""
    c = CASE[name]
    B = batch_size(c, bmax)
    if c.fam == "P":
        N = 2 * c.n
        x, adj, nn_, label = O.make_batch(B, N, c.F, n_min=max(1, c.n), p=0.3, seed=c.seed, n_classes=c.C)
        cls = SoftPoolingGcnEncoder if c.bn else NoBatchNormEncoder
        model = cls(N, c.F, c.H, c.E, c.C, c.L, c.H, assign_ratio=0.5, num_pooling=1, pred_hidden_dims=list(c.hidden),
                    linkpred=False)
    else:
        full = not c.bias
        x, adj, nn_, label = O.make_batch(B, c.n, c.F, n_min=c.n if full else max(1, c.n // 2),
                                          p=0.6 if full else 0.3, seed=c.seed, n_classes=c.C)
        model = GcnEncoderGraph(c.F, c.H, c.E, c.C, c.L, pred_hidden_dims=list(c.hidden), concat=c.concat, bn=c.bn,
                                args=types.SimpleNamespace(bias=c.bias))
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=c.seed, bias_scale=0.1)
    if c.fam == "P":
        params["assign_pred.weight"] = params["assign_pred.weight"] * ASSIGN_SHARPEN
    model.load_state_dict(params)
    return model, params, x, adj, nn_, label


def step(model, c, xd, ad, nn_, ld):
    """One forward + loss + backward; (ypred, loss) -- the gradients are on the parameters."""
    model.zero_grad(set_to_none=True)
    y = model(xd, ad, nn_, assign_x=xd) if c.fam == "P" else model(xd, ad, nn_)
    loss = model.loss(y, ld)
    loss.backward()
    return y, loss


def results(model, c, y):
    """What a GPU run of a case leaves for the checks: ypred, every gradient ("grad." + name), the saved embedding and
    readout arg-max of every level, and the pooled level's inputs."""
    out = {"ypred": y.detach().cpu().clone()}
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.detach().cpu().clone()
    for j in range(2 if c.fam == "P" else 1):
        out[f"emb{j}"] = model.saved_activation(j, "embedding").detach().cpu().clone()
        out[f"argmax{j}"] = model.saved_activation(j, "readout_argmax").detach().cpu().clone()
    if c.fam == "P":
        out["xpool"] = model.saved_activation(0, "xpool").detach().cpu().clone()
        out["adjpool"] = model.saved_activation(0, "adjpool").detach().cpu().clone()
    return out


def loose_names(model, c, tier):
    """Gradients a bit comparison between two runs leaves to rounding (rtol 1e-5 / atol 1e-7): the generic per-phase
    sequence sums GraphConv bias gradients, and the assign_pred bias gradient, with float atomics.  By
    rule, from the model's own parameter groups: level 0 of family P always (it has two stacks, so never a small level;
    where it runs the persistent kernels the sums are ordered and pass the looser check as well), and the level under
    test when its tier is `generic`."""
    ids = set()
    under_test = 1 if c.fam == "P" else 0
    for kind, level, mods in model._graph_param_groups():
        # level 0 of family P: its embedding stack, its assignment stack and assign_pred (the level under test is level 1)
        if (c.fam == "P" and level == 0) or (kind == "embed" and level == under_test and tier == "generic"):
            mods = [mods] if kind == "assign_pred" else mods
            ids |= {id(m.bias) for m in mods if m.bias is not None}
    return tuple("grad." + k for k, p in model.named_parameters() if id(p) in ids)


# ------------------------------------------------------------------ the references
def stack_forward(x, adj, params, keys, bn, add_self):
    """The GCN stack written out (encoders.py:1054-1081): (concatenated output, pre-ReLU values of the non-last layers,
    post-ReLU values of the non-last layers before BatchNorm)."""
    outs, pre, act = [], [], []
    h = x
    for li, k in enumerate(keys):
        h = O.graph_conv(h, adj, params[k + ".weight"], params.get(k + ".bias"), add_self, True)
        if li < len(keys) - 1:
            pre.append(h)
            h = torch.relu(h)
            act.append(h)
            if bn:
                h = O.bn_node(h)
        outs.append(h)
    return torch.cat(outs, dim=2), pre, act


def readout(z, winners):
    """Max readout over the rows of z [B, n, D]; with winners (int [B, D], -1: the constant 0 of a masked row) forced."""
    if winners is None:
        return z.max(dim=1)[0]
    idx = winners.to(torch.int64)
    got = z.gather(1, idx.clamp_min(0).unsqueeze(1)).squeeze(1)
    return torch.where(idx >= 0, got, torch.zeros((), dtype=z.dtype))


def base_forward(c, params, x, adj, winners=None):
    """GcnEncoderGraph.forward (encoders.py:1083-1122) with forced winners: (ypred, readout features, z, pre, act)."""
    z, pre, act = stack_forward(x, adj, params, stack_keys(c), c.bn, not c.concat)
    zr = z if c.concat else z[:, :, z.shape[2] - c.E:]
    feat = readout(zr, winners)
    return O.mlp_head(feat, params, "pred_model", len(c.hidden)), feat, z, pre, act


def head_pre(params, feat, n_hidden):
    """Pre-activations of pred_model's hidden layers for the readout features `feat`."""
    pre, h = [], feat
    for i in range(n_hidden):
        z = torch.nn.functional.linear(h, params[f"pred_model.{2 * i}.weight"], params[f"pred_model.{2 * i}.bias"])
        pre.append(z)
        h = torch.relu(z)
    return pre


def check_winners(z, winners, what):
    """Each recorded winner holds the fp64 column maximum of z to within 1e-6 of the column's largest magnitude."""
    top = z.max(dim=1)[0]
    top = torch.where(winners < 0, top.clamp_min(0), top)    # -1: a masked zero row holds the maximum
    gap = (top - readout(z, winners)) / z.abs().amax(dim=1).clamp_min(1e-300)
    assert float(gap.max()) <= 1e-6, f"{what}: a recorded winner is {float(gap.max()):.3e} of the column below the maximum"


def level0_embedding(c, params, x, adj, nn_, dtype=torch.float64):
    """Family P: the masked level-0 embedding, a function of the batch and the parameters alone."""
    P = {k: v.to(dtype) for k, v in params.items()}
    return O.gcn_stack(x.to(dtype), adj.to(dtype), P, O._stack_keys("conv_first", "conv_block", "conv_last", c.L),
                       O.node_mask(x.shape[1], nn_, dtype), c.bn)


def end_to_end(c, params, x, adj, nn_, label, winners, dtype=torch.float64):
    """Reference (i): (ypred, loss, {name: gradient}, intermediates) with `winners` (a list per level, or None)."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x, adj = x.to(dtype), adj.to(dtype)
    if c.fam == "P":
        y, inter = O.softpool_forward(P, x, adj, nn_, x, num_layers=c.L, num_pooling=1, n_pred_hidden=len(c.hidden),
                                      bn=c.bn, want_intermediates=True, winners=winners)
    else:
        y, feat, z, pre, act = base_forward(c, P, x, adj, None if winners is None else winners[0])
        inter = {"readout": feat}
    loss = torch.nn.functional.cross_entropy(y, label)
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in P.items()}, inter


def level_alone(c, params, label, got, dtype, x=None, adj=None):
    """Reference (ii) in `dtype`, on the inputs the run `got` (see `results`) gave the level: {"emb": the level's
    embedding, "grad." + name: gradient for every name of `level_names`}, plus "pre" / "act" / "head_pre" lists."""
    names = level_names(c, params)
    P = {k: v.to(dtype).clone().requires_grad_(k in names) for k, v in params.items()}
    if c.fam == "P":
        z, pre, act = stack_forward(got["xpool"].to(dtype), got["adjpool"].to(dtype), P, stack_keys(c), c.bn, False)
        feat0 = readout(got["emb0"].to(dtype), got["argmax0"])          # the other level's readout: a constant
        feat = torch.cat([feat0, readout(z, got["argmax1"])], dim=1)
    else:
        z, pre, act = stack_forward(x.to(dtype), adj.to(dtype), P, stack_keys(c), c.bn, not c.concat)
        feat = readout(z if c.concat else z[:, :, z.shape[2] - c.E:], got["argmax0"])
    y = O.mlp_head(feat, P, "pred_model", len(c.hidden))
    torch.nn.functional.cross_entropy(y, label).backward()
    out = {"emb": z.detach(), "pre": [t.detach() for t in pre], "act": [t.detach() for t in act],
           "head_pre": [t.detach() for t in head_pre(P, feat.detach(), len(c.hidden))]}
    out.update({"grad." + k: P[k].grad for k in names})
    return out


def oracle_got(c, params, x, adj, nn_, dtype=torch.float32):
    """What `results` gives the level check, from the CPU oracle in `dtype` with its own arg-max in place of a GPU run
    (tests/test_small_level_cases_cpu.py)."""
    P = {k: v.to(dtype) for k, v in params.items()}
    x, adj = x.to(dtype), adj.to(dtype)
    if c.fam == "B":
        z = stack_forward(x, adj, P, stack_keys(c), c.bn, not c.concat)[0]
        zr = z if c.concat else z[:, :, z.shape[2] - c.E:]
        return {"emb0": z, "argmax0": zr.max(dim=1)[1].int()}
    _, inter = O.softpool_forward(P, x, adj, nn_, x, num_layers=c.L, n_pred_hidden=len(c.hidden), bn=c.bn,
                                  want_intermediates=True)
    z0 = O.gcn_stack(x, adj, P, O._stack_keys("conv_first", "conv_block", "conv_last", c.L),
                     O.node_mask(x.shape[1], nn_, dtype), c.bn)
    z1 = O.gcn_stack(inter["xpool_0"], inter["adjpool_0"], P, stack_keys(c), None, c.bn)
    return {"xpool": inter["xpool_0"], "adjpool": inter["adjpool_0"], "emb0": z0, "emb1": z1,
            "argmax0": z0.max(dim=1)[1].int(), "argmax1": z1.max(dim=1)[1].int()}


def level_figures(c, params, label, got, x=None, adj=None):
    """Check (ii) of one run: [(tensor, kernel error, e_ref, bound, max|ref|)] for the level's embedding and, unless the
    case is in DROP_BWD, for every gradient of `level_names`.  Errors are max abs differences from the fp64 reference."""
    r64 = level_alone(c, params, label, got, torch.float64, x, adj)
    r32 = level_alone(c, params, label, got, torch.float32, x, adj)
    emb_key = "emb1" if c.fam == "P" else "emb0"
    keys = ["emb"] + ([] if c.name in DROP_BWD else [k for k in r64 if k.startswith("grad.")])
    rows = []
    for k in keys:
        ref = r64[k]
        mine = got[emb_key if k == "emb" else k].double()
        e_ref = float((r32[k].double() - ref).abs().max())
        scale = float(ref.abs().max())
        rows.append((k, float((mine - ref).abs().max()), e_ref, max(FACTOR * e_ref, FLOOR * scale), scale))
    if rows[0][1] <= rows[0][3]:         # (a wrong embedding is reported as such, by `failures`, not as a wrong winner)
        check_winners(r64["emb"] if (c.fam == "P" or c.concat) else r64["emb"][:, :, r64["emb"].shape[2] - c.E:],
                      got["argmax1" if c.fam == "P" else "argmax0"], c.name)
    return rows


def failures(rows):
    return [f"{k}: error {err:.3e} > bound {bound:.3e} (e_ref {e:.3e}, ratio {err / e if e else float('inf'):.2f})"
            for k, err, e, bound, _ in rows if not err <= bound]
