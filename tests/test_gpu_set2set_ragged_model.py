"""SparseGcnSet2SetEncoder (graph_pooling_amd/sparse.py) on ragged CsrBatches and single CsrGraphs against
oracle.set2set_encoder_forward on the zero-padded dense batch: logits, loss and every parameter gradient (the conv
biases included: with non-zero biases the padded rows' constants sit in the BatchNorm statistics), with and without
BatchNorm and with pad_to above the largest graph.  Tolerances are the project's (tests/parity.py, as
test_gpu_ragged_base.py applies them): outputs rtol 1e-4 / atol 1e-5, loss 1e-4 / 1e-6, parameter gradients
grads_close(rtol=2e-3, atol_rel=1e-4)."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import SparseGcnSet2SetEncoder
from graph_pooling_amd.encoders import GcnSet2SetEncoder
from graph_pooling_amd.sparse import CsrBatch, CsrGraph
from oracle import diffpool_oracle as O
from tests import ragged_base_cases as RC
from tests.parity import close, grads_close

pytestmark = pytest.mark.gpu

NCLS = 3
# name: (sizes, pad_to, (F, H, E))
SHAPES = {"pad_to_max": ([23, 7, 1, 16], None, (9, 12, 10)), "pad_above": ([17, 30, 4], 36, (7, 10, 10))}


def _init(model, seed):
    """Parameters of `model` as {key: fp32 tensor}: torch's own initialisation under `seed` for the Linear / LSTM
    tensors, O.init_params' for the GraphConv weights, and GraphConv biases uniform in +-0.3 — so the padded rows of the
    dense batch hold non-zero constants in front of the mask."""
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    conv = O.init_params({k: v for k, v in shapes.items() if k.startswith("conv_")}, seed=seed, bias_scale=0.3)
    g = torch.Generator().manual_seed(seed + 100)
    params = {}
    for k, shp in shapes.items():
        if k in conv:
            params[k] = conv[k]
        else:
            # nn.Linear / nn.LSTM style: uniform in +-1/sqrt(fan_in); an LSTM bias [4d] goes with fan_in d
            fan = shp[1] if len(shp) == 2 else shp[0] // 4 if ".lstm." in k else shapes[k[:-4] + "weight"][1]
            params[k] = (torch.rand(shp, generator=g) * 2 - 1) / fan ** 0.5
    model.load_state_dict(params)
    return params


def _case(shape, bn, hidden, seed=2):
    sizes, pad_to, (F_, H, E) = SHAPES[shape]
    srcs, dsts = RC.ring_with_chords(sizes, seed)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda", pad_to=pad_to)
    P = batch.pad_to
    adj = RC.dense_adj(sizes, srcs, dsts, P)
    x = torch.randn(sum(sizes), F_, generator=torch.Generator().manual_seed(seed + 10))
    model = SparseGcnSet2SetEncoder(F_, H, E, NCLS, 3, pred_hidden_dims=hidden, bn=bn)
    params = _init(model, seed)
    label = torch.tensor([b % NCLS for b in range(len(sizes))])
    return model.cuda(), params, batch, adj, x, label, sizes, P


def _run(model, x, batch, label):
    model.zero_grad(set_to_none=True)
    ypred = model(x.cuda(), batch)
    loss = model.loss(ypred, label.cuda())
    loss.backward()
    return ypred, loss


def _away_from_relu_kinks(P64, xpad, adj, sizes, hidden, bn):
    """A check of the CASE (the margin rule of test_gpu_level0_phase0.py): no unit of Set2Set's own ReLU output or of
    pred_model's hidden layer sits closer to the kink than 1e-5 of the layer's largest pre-activation."""
    with torch.no_grad():
        z = O.gcn_stack(xpad, adj, P64, O._stack_keys("conv_first", "conv_block", "conv_last", 3),
                        O.node_mask(xpad.shape[1], sizes, xpad.dtype), bn)
        out = O.set2set_forward(z, P64, "s2s.")
        B, T, d = z.shape
        pres = []                                      # Set2Set's pre-activation: its recurrence restated up to q*_T
        h, c, qs = z.new_zeros(B, d), z.new_zeros(B, d), z.new_zeros(B, 2 * d)
        for _ in range(T):
            h, c = O.lstm_cell(qs, h, c, P64["s2s.lstm.weight_ih_l0"], P64["s2s.lstm.weight_hh_l0"],
                               P64["s2s.lstm.bias_ih_l0"], P64["s2s.lstm.bias_hh_l0"])
            a = torch.softmax(torch.einsum("bnd,bd->bn", z, h), dim=1)
            qs = torch.cat([h, torch.einsum("bn,bnd->bd", a, z)], dim=1)
        pres.append(torch.nn.functional.linear(qs, P64["s2s.pred.weight"], P64["s2s.pred.bias"]))
        assert float((torch.relu(pres[0]) - out).abs().max()) <= 1e-12
        if hidden:
            pres.append(torch.nn.functional.linear(out, P64["pred_model.0.weight"], P64["pred_model.0.bias"]))
    for pre in pres:
        assert float(pre.abs().min()) > 1e-5 * float(pre.abs().max()), \
            f"the case sits on a ReLU kink: |pre-activation| {float(pre.abs().min()):.3e}: choose another seed"


@pytest.mark.parametrize("hidden", [[], [20]], ids=["linear", "mlp20"])
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_equals_the_oracle_on_the_padded_batch(shape, bn, hidden):
    model, params, batch, adj, x, label, sizes, P = _case(shape, bn, hidden)
    P64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    xpad = RC.pad_rows(x.double(), sizes, P)
    assert any(float(v.abs().max()) > 0 for k, v in params.items() if k.startswith("conv_") and k.endswith(".bias"))
    _away_from_relu_kinks({k: v.detach() for k, v in P64.items()}, xpad, adj, sizes, hidden, bn)
    yo = O.set2set_encoder_forward(P64, xpad, adj, sizes, n_pred_hidden=len(hidden), bn=bn)
    lo = torch.nn.functional.cross_entropy(yo, label)
    lo.backward()
    ypred, loss = _run(model, x, batch, label)
    assert ypred.shape == (len(sizes), NCLS)
    close(ypred, yo.detach())
    close(loss, lo.detach(), 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in P64.items()}, rtol=2e-3, atol_rel=1e-4)
    assert torch.equal(model.predict(x.cuda(), batch).cpu(), yo.argmax(dim=1))


def test_dense_class_with_the_same_parameters_agrees():
    model, params, batch, adj, x, label, sizes, P = _case("pad_above", True, [20])
    dense = GcnSet2SetEncoder(7, 10, 10, NCLS, 3, pred_hidden_dims=[20], bn=True)
    dense.load_state_dict(model.state_dict())
    dense = dense.cuda()
    yd = dense(RC.pad_rows(x, sizes, P).cuda(), adj.float().cuda(), sizes)
    ld = dense.loss(yd, label.cuda())
    ld.backward()
    ypred, loss = _run(model, x, batch, label)
    close(ypred, yd)
    close(loss, ld, 1e-4, 1e-6)
    grads_close(model, {k: p.grad for k, p in dense.named_parameters()}, rtol=2e-3, atol_rel=1e-4)


def test_one_graph_batch_without_padding_equals_the_single_graph_call():
    n = 97
    srcs, dsts = RC.ring_with_chords([n], 3)
    g = CsrGraph.from_edges(n, srcs[0], dsts[0], "cuda", symmetric=True)
    batch = CsrBatch.from_graphs([g])
    assert batch.pad_to == n
    x = torch.randn(n, 9, generator=torch.Generator().manual_seed(1)).cuda()
    model = SparseGcnSet2SetEncoder(9, 12, 10, NCLS, 3, pred_hidden_dims=[20])
    _init(model, 4)
    model = model.cuda()
    label = torch.tensor([1]).cuda()
    y1 = model(x, g)
    assert y1.shape == (1, NCLS)
    l1 = model.loss(y1, label)
    l1.backward()
    g1 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    yb = model(x, batch)
    lb = model.loss(yb, label)
    lb.backward()
    close(yb, y1)
    close(lb, l1, 1e-4, 1e-6)
    grads_close(model, g1, rtol=2e-3, atol_rel=1e-4)


def test_training_steps_lower_the_loss():
    from graph_pooling_amd.optim import FusedClipAdam
    model, params, batch, adj, x, label, sizes, P = _case("pad_to_max", True, [20])
    opt = FusedClipAdam(model, lr=1e-2, clip=2.0)
    xd, ld = x.cuda(), label.cuda()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model.loss(model(xd, batch), ld)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k


def _kernel_launches(sizes):
    srcs, dsts = RC.ring_with_chords(sizes, 1)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda")
    model = SparseGcnSet2SetEncoder(9, 12, 10, NCLS, 3, pred_hidden_dims=[20]).cuda()
    x = torch.randn(sum(sizes), 9, generator=torch.Generator().manual_seed(0))
    label = torch.tensor([b % NCLS for b in range(len(sizes))])
    _run(model, x, batch, label)                                 # warm up: lazy module loads
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        _run(model, x, batch, label)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def test_launch_count_does_not_grow_with_the_batch():
    """Two graphs or eight: the same kernels, once each (the recurrence is one grid of B workgroups per pass, the
    embedding gradient one grid of (row tile, graph) workgroups)."""
    n2 = _kernel_launches([60, 30])
    n8 = _kernel_launches([60, 30, 50, 10, 40, 60, 24, 45])
    assert n2 == n8 and n2 > 0, (n2, n8)
