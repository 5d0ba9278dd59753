"""Cases and the training step shared by tests/test_gpu_head_grads_final.py and its child process
(tests/_head_grads_final_worker.py): small DiffPool models whose last pooled level takes the whole-level backward kernel
with the prediction-head backward folded in, so that pred_model's dW / db are written by the step's final launch
(k_reduce_slabs_head, csrc/dp_rowops.hip).

N = 64 with assign_ratio 0.25: the pooled levels have 16 (and, with num_pooling 2, 4) clusters.  Over the ten cases
  B in {1, 5, 33}      the degenerate batch, an odd count, and more graphs than one 32-graph chunk of the chain loop;
  pred_hidden_dims in {[], [50], [7, 5]}   one, two and three Linear layers (odd widths, two rows of hidden gradients);
every pair of the two occurs, and label_dim (2, 6), BatchNorm (on, off) and num_pooling (1, 2) take both values with
each batch size; B = 33 also runs without BatchNorm at num_pooling 2 (more than one chunk on the plan without a wait).  SoftPoolingGcnEncoder's constructor always builds BatchNorm (as the reference does), so the plan
without it -- the one whose pooled-level backward waits for no other workgroup -- is reached through a subclass that
clears the flag; the oracle runs with bn=False for it."""
import torch

from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O

N, F_, H, RATIO = 64, 5, 8, 0.25

#        name            B   hidden   C  bn     P  seed
CASES = [
    ("b1_h50",           1,  (50,),   2, True,  1, 3),
    ("b5_lin_c6",        5,  (),      6, True,  1, 3),
    ("b33_h7x5",         33, (7, 5),  2, True,  1, 3),
    ("b33_h50_c6_nobn",  33, (50,),   6, False, 1, 3),
    ("b5_h7x5_c6_nobn_p2", 5, (7, 5), 6, False, 2, 3),
    ("b1_lin_nobn",      1,  (),      2, False, 1, 3),
    ("b33_lin_p2",       33, (),      2, True,  2, 3),
    ("b5_h50_p2",        5,  (50,),   2, True,  2, 3),
    ("b1_h7x5_c6_p2",    1,  (7, 5),  6, True,  2, 3),
    ("b33_h50_nobn_p2",  33, (50,),   2, False, 2, 3),
]
CASE = {c[0]: c for c in CASES}


def atomic_bias_names(model):
    """Bias gradients that bit comparisons leave to a rounding tolerance, as tests/test_gpu_head_fold.py does for
    enzymes_p3: with num_pooling 2, level 1 carries an assignment stack and runs the generic per-layer kernels, whose
    bias gradients are float-atomic sums -- last-place differences between two runs of ANY plan.  Taken
    from the model's own parameter groups, not from a list of names: level 1's embedding stack is
    conv_*_after_pool_0, and its assignment stack, being the LAST pooling's, carries the reference's plain names
    assign_conv_* (level 0's is assign_conv_*_0).  Empty for num_pooling 1."""
    if model.num_pooling < 2:
        return ()
    ids = set()
    for kind, level, mods in model._graph_param_groups():
        if kind in ("embed", "assign") and 1 <= level < model.num_pooling:
            ids |= {id(p) for m in mods for p in m.parameters()}
    return tuple(k for k, p in model.named_parameters() if id(p) in ids and k.endswith(".bias"))


class NoBatchNormEncoder(SoftPoolingGcnEncoder):
    """The same model with the BatchNorm flag cleared in the configuration handed to the library."""

    def _flags(self):
        return 0


def build(name):
    """(model on the CPU with the case's parameters loaded, params, x, adj, num_nodes, label)."""
    _, B, hidden, Cc, bn, P, seed = CASE[name]
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=8, p=0.1, seed=seed, n_classes=Cc)
    cls = SoftPoolingGcnEncoder if bn else NoBatchNormEncoder
    model = cls(N, F_, H, H, Cc, 3, H, assign_ratio=RATIO, num_pooling=P, pred_hidden_dims=list(hidden), linkpred=False)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed, bias_scale=0.1)
    model.load_state_dict(params)
    return model, params, x, adj, nn_, label


def step(model, xd, ad, nn_, ld):
    """One forward + loss + backward; (ypred, loss) -- the gradients are on the parameters."""
    model.zero_grad(set_to_none=True)
    y = model(xd, ad, nn_, assign_x=xd)
    loss = model.loss(y, ld)
    loss.backward()
    return y, loss


def results(model, y):
    out = {"ypred": y.detach().cpu()}
    for k, p in model.named_parameters():
        out[k] = p.grad.detach().cpu().clone()
    return out


def head_preactivations(params, feat, n_hidden):
    """Pre-activations of pred_model's hidden layers for the readout features `feat` (the ReLU-kink margin check)."""
    pre, h = [], feat
    for i in range(n_hidden):
        z = torch.nn.functional.linear(h, params[f"pred_model.{2 * i}.weight"], params[f"pred_model.{2 * i}.bias"])
        pre.append(z.detach())
        h = torch.relu(z)
    return pre
