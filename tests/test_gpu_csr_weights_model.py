"""The three Sparse* model classes on WEIGHTED containers — the reference sampler's default D^-1/2 A D^-1/2
(`.normalized()`) — against the oracle on the padded dense normalised batch and against the dense classes with the same
parameters: normalised random graphs of 64 and 300 nodes as a CsrGraph, and a CsrBatch of [1, 37, 64, 130] nodes with
pad_to = 140.  Tolerances and helpers are those of the 0/1 model tests: parity.close (1e-4 / 1e-5; losses 1e-4 / 1e-6),
parity.grads_close(rtol=2e-3, atol_rel=1e-4) as tests/test_gpu_sparse.py / test_gpu_csr_batch.py use, the oracle's
backward on the winners the HIP forward recorded (gpu_winners), and the ReLU-kink guard of test_gpu_level0_phase0.py."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import SparseGcnSet2SetEncoder
from graph_pooling_amd.encoders import GcnEncoderGraph, GcnSet2SetEncoder, SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import (CsrBatch, CsrGraph, SparseBatchGcnEncoderGraph, SparseGcnEncoderGraph,
                                      SparseSoftPoolingGcnEncoder)
from oracle import diffpool_oracle as O
from tests import csr_weights_cases as WC
from tests import ragged_base_cases as RC
from tests.parity import close, grads_close, gpu_winners
from tests.test_gpu_level0_phase0 import _away_from_the_head_relu_kink
from tests.test_gpu_ragged_base import check_premises, ref_forward
from tests.test_gpu_set2set_ragged_model import _away_from_relu_kinks, _init

pytestmark = pytest.mark.gpu

NCLS = 3
SIZES, PAD_TO = [1, 37, 64, 130], 140
F_IN, HID = 9, 20
CONTAINERS = ["graph64", "graph300", "batch"]


def _container(name, seed=0, normalized=True, device="cuda"):
    """(container on the GPU, sizes, P, dense adjacency [B, P, P] float32 of exactly the container's values)."""
    sizes, P = ([int(name[5:])], int(name[5:])) if name.startswith("graph") else (SIZES, PAD_TO)
    srcs, dsts = RC.ring_with_chords(sizes, 50 + seed)
    if name == "batch":
        # the one-node graph gets a self loop: a node of degree 0 has no normalised adjacency
        srcs[0], dsts[0] = np.zeros(1, np.int64), np.zeros(1, np.int64)
        c = CsrBatch.from_edge_lists(sizes, srcs, dsts, device, pad_to=P)
    else:
        c = CsrGraph.from_edges(sizes[0], srcs[0], dsts[0], device)
    if normalized:
        c = c.normalized()
        assert c.weighted
    a = WC.dense(c) if c.weighted else WC.dense(c, np.ones(c.indices.numel()))
    adj = torch.zeros(len(sizes), P, P, dtype=torch.float64)
    o = 0
    for b, n in enumerate(sizes):
        adj[b, :n, :n] = torch.from_numpy(a[o:o + n, o:o + n])
        o += n
    return c, sizes, P, adj.float()


def _inputs(sizes, seed, f=F_IN):
    x = torch.randn(sum(sizes), f, generator=torch.Generator().manual_seed(seed + 10))
    label = torch.tensor([(b + 1) % NCLS for b in range(len(sizes))])
    return x, label


# ------------------------------------------------------------------ DiffPool
def _extra_terms(s0, adj, sizes, link, ent_w):
    """The Frobenius link term and the assignment-entropy term of the dense batch in plain torch (the oracle has the
    cross-entropy link term only)."""
    m = O.node_mask(adj.shape[1], sizes, s0.dtype)
    total = 0.0
    if link == "frobenius":
        r = (adj - s0 @ s0.transpose(1, 2)) * (m @ m.transpose(1, 2))
        total = total + (r * r).sum() / float(sum(n * n for n in sizes))
    if ent_w:
        total = total + ent_w * (-(s0 * torch.log(s0 + 1e-15)).sum(dim=2, keepdim=True) * m).sum() / float(sum(sizes))
    return total


def _diffpool(name, link, ent_w, seed=0):
    c, sizes, P, adj = _container(name, seed)
    x, label = _inputs(sizes, seed)
    kw = dict(assign_ratio=0.1, num_pooling=1, pred_hidden_dims=[50], linkpred=link, assign_ent_weight=ent_w)
    model = SparseSoftPoolingGcnEncoder(P, F_IN, HID, HID, NCLS, 3, HID, **kw)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed + 1, bias_scale=0.3)
    model.load_state_dict(params)
    dense = SoftPoolingGcnEncoder(P, F_IN, HID, HID, NCLS, 3, HID, **kw)
    return model.cuda(), dense, params, c, sizes, P, adj, x, label


@pytest.mark.parametrize("link,ent_w", [(True, 0.0), ("frobenius", 0.0), (True, 0.3)],
                         ids=["linkpred", "frobenius", "linkpred+entropy"])
@pytest.mark.parametrize("name", CONTAINERS)
def test_diffpool_on_a_normalised_container_equals_oracle_and_dense_class(name, link, ent_w):
    model, dense, params, c, sizes, P, adj, x, label = _diffpool(name, link, ent_w)
    ypred = model(x.cuda(), c)
    loss = model.loss(ypred, label.cuda(), c)
    loss.backward()
    win = gpu_winners(model, 2)
    xp = RC.pad_rows(x, sizes, P)
    yfree, _ = O.softpool_forward(params, xp, adj, sizes, xp, num_pooling=1, want_intermediates=True)
    close(ypred, yfree)
    Pm = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo, inter = O.softpool_forward(Pm, xp, adj, sizes, xp, num_pooling=1, winners=win)
    lo, _ = O.softpool_loss(yo, label, inter["assign_0"], adj, sizes, link is True)
    lo = lo + _extra_terms(inter["assign_0"], adj, sizes, link, ent_w)
    lo.backward()
    _away_from_the_head_relu_kink(Pm, inter)
    close(ypred, yo)
    close(loss, lo, 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in Pm.items()}, rtol=2e-3, atol_rel=1e-4)
    # the dense class with this model's state_dict on the padded dense normalised batch
    dense.load_state_dict(model.state_dict())
    dense = dense.cuda()
    yd = dense(xp.cuda(), adj.cuda(), np.array(sizes), assign_x=xp.cuda())
    ld = dense.loss(yd, label.cuda(), adj.cuda(), np.array(sizes))
    ld.backward()
    close(ypred, yd)
    close(loss, ld, 1e-4, 1e-6)
    grads_close(model, {k: p.grad for k, p in dense.named_parameters()}, rtol=2e-3, atol_rel=1e-4)


def test_weights_reach_the_model_output():
    """The same graphs as 0/1 and normalised containers give different predictions: the values are read."""
    model, _, params, c, sizes, P, adj, x, label = _diffpool("batch", True, 0.0)
    c01, _, _, adj01 = _container("batch", normalized=False)
    with torch.no_grad():
        yw, y01 = model(x.cuda(), c), model(x.cuda(), c01)
    assert float((yw - y01).abs().max()) > 1e-3
    xp = RC.pad_rows(x, sizes, P)
    close(y01, O.softpool_forward(params, xp, adj01, sizes, xp, num_pooling=1)[0])


@pytest.mark.parametrize("name", CONTAINERS)
def test_dense_state_dict_loads_into_the_sparse_class(name):
    _, dense, params, c, sizes, P, adj, x, label = _diffpool(name, True, 0.0, seed=3)
    dense.load_state_dict(params)
    dense = dense.cuda()
    xp = RC.pad_rows(x, sizes, P)
    with torch.no_grad():
        yd = dense(xp.cuda(), adj.cuda(), np.array(sizes), assign_x=xp.cuda())
    sparse = SparseSoftPoolingGcnEncoder(P, F_IN, HID, HID, NCLS, 3, HID, assign_ratio=0.1, num_pooling=1,
                                         pred_hidden_dims=[50], linkpred=True)
    sparse.load_state_dict(dense.state_dict())
    sparse = sparse.cuda()
    with torch.no_grad():
        ys = sparse(x.cuda(), c)
    close(ys, yd)


def test_three_optimiser_steps_on_a_weighted_batch_follow_the_dense_class():
    from graph_pooling_amd.optim import FusedClipAdam
    model, dense, params, c, sizes, P, adj, x, label = _diffpool("batch", True, 0.0, seed=5)
    dense.load_state_dict(model.state_dict())
    dense = dense.cuda()
    xp, nn_ = RC.pad_rows(x, sizes, P).cuda(), np.array(sizes)
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    opt_s, opt_d = FusedClipAdam(model, lr=1e-3, clip=2.0), FusedClipAdam(dense, lr=1e-3, clip=2.0)
    for step in range(3):
        opt_s.zero_grad()
        ls = model.loss(model(xd, c), ld, c)
        ls.backward()
        opt_s.step()
        opt_d.zero_grad()
        ldn = dense.loss(dense(xp, ad, nn_, assign_x=xp), ld, ad, nn_)
        ldn.backward()
        opt_d.step()
        # the gradients agree to grads_close's 2e-3; a step of lr = 1e-3 moves the loss by far less than that
        close(ls, ldn, 2e-3, 1e-5)
    assert torch.isfinite(ls)


def _kernel_launches(model, x, c, label):
    def run():
        model.zero_grad(set_to_none=True)
        ypred = model(x, c)
        return model.loss(ypred, label, c)
    run()                                            # warm up: plans, lazy module loads
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


@pytest.mark.parametrize("link", [True, "frobenius"])
@pytest.mark.parametrize("name", ["graph300", "batch"])
def test_a_weighted_forward_and_loss_launch_what_the_unweighted_ones_launch(name, link):
    model, _, _, cw, sizes, _, _, x, label = _diffpool(name, link, 0.2)
    c01 = _container(name, normalized=False)[0]
    assert cw.weighted and not c01.weighted
    nw, n01 = _kernel_launches(model, x.cuda(), cw, label.cuda()), _kernel_launches(model, x.cuda(), c01, label.cuda())
    assert nw == n01 and nw > 0, (nw, n01)


# ------------------------------------------------------------------ base GCN encoder
BASE_SEED = {"graph64": 0, "graph300": 0, "batch": 0}


def _base(name, hidden=(50,)):
    seed = BASE_SEED[name]
    c, sizes, P, adj = _container(name, seed)
    x, label = _inputs(sizes, seed)
    cls = SparseBatchGcnEncoderGraph if name == "batch" else SparseGcnEncoderGraph
    model = cls(F_IN, HID, HID, NCLS, 3, pred_hidden_dims=list(hidden))
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed + 2, bias_scale=0.3)
    model.load_state_dict(params)
    return model.cuda(), params, c, sizes, P, adj, x, label


@pytest.mark.parametrize("name", CONTAINERS)
def test_base_encoder_on_a_normalised_container_equals_reference_and_dense_class(name):
    """The float64 restatement of tests/test_gpu_ragged_base.py (the base class's readout is unmasked: padded rows win),
    run on the winners of the HIP forward, and the dense class on the padded dense normalised batch."""
    model, params, c, sizes, P, adj, x, label = _base(name)
    xd = x.cuda()
    ypred = model(xd, c)
    loss = torch.nn.functional.cross_entropy(ypred, label.cuda())
    loss.backward()
    P64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    xpad = RC.pad_rows(x.double(), sizes, P)
    yfree, layers = ref_forward(P64, xpad, adj.double(), 1, True)
    if name == "batch":
        check_premises([h.detach() for h in layers], sizes, P, True, two_indices=False)
        win = [model.saved_activation(li, "readout_argmax").clone().cpu() for li in range(3)]
    else:
        win = [h.detach().max(dim=1)[1] for h in layers]
        for h in layers:                             # every readout gap above 1e-4 of the layer's largest entry
            v = h.detach().max(dim=1)[0]
            below = torch.where(h.detach() < v.unsqueeze(1), h.detach(), torch.full_like(h, -float("inf"))).max(dim=1)[0]
            assert float(((v - below) / h.detach().abs().max()).min()) >= 1e-4
    yw, _ = ref_forward(P64, xpad, adj.double(), 1, True, winners=win)
    lo = torch.nn.functional.cross_entropy(yw, label)
    lo.backward()
    pre = torch.nn.functional.linear(torch.cat([torch.gather(h, 1, w.to(torch.int64).unsqueeze(1)).squeeze(1)
                                                for h, w in zip(layers, win)], dim=1),
                                     P64["pred_model.0.weight"], P64["pred_model.0.bias"]).detach()
    assert float(pre.abs().min()) > 1e-5 * float(pre.abs().max()), "the case sits on a ReLU kink of the head"
    close(ypred, yfree.detach())
    close(ypred, yw.detach())
    close(loss, lo.detach(), 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in P64.items()}, rtol=2e-3, atol_rel=1e-4)
    yo = O.base_forward(params, RC.pad_rows(x, sizes, P), adj, n_pred_hidden=1, bn=True, concat=True)
    close(ypred, yo)
    dense = GcnEncoderGraph(F_IN, HID, HID, NCLS, 3, pred_hidden_dims=[50])
    dense.load_state_dict(model.state_dict())
    dense = dense.cuda()
    with torch.no_grad():
        yd = dense(RC.pad_rows(x, sizes, P).cuda(), adj.cuda(), sizes)
    close(ypred, yd)


# ------------------------------------------------------------------ GCN + Set2Set
@pytest.mark.parametrize("name", CONTAINERS)
def test_set2set_encoder_on_a_normalised_container_equals_oracle_and_dense_class(name):
    seed = 2
    c, sizes, P, adj = _container(name, seed)
    F_, H, E = 7, 10, 10
    x, label = _inputs(sizes, seed, F_)
    model = SparseGcnSet2SetEncoder(F_, H, E, NCLS, 3, pred_hidden_dims=[20], bn=True)
    params = _init(model, seed)
    model = model.cuda()
    P64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    xpad = RC.pad_rows(x.double(), sizes, P)
    _away_from_relu_kinks({k: v.detach() for k, v in P64.items()}, xpad, adj.double(), sizes, [20], True)
    yo = O.set2set_encoder_forward(P64, xpad, adj.double(), sizes, n_pred_hidden=1, bn=True)
    lo = torch.nn.functional.cross_entropy(yo, label)
    lo.backward()
    ypred = model(x.cuda(), c)
    loss = model.loss(ypred, label.cuda())
    loss.backward()
    close(ypred, yo.detach())
    close(loss, lo.detach(), 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in P64.items()}, rtol=2e-3, atol_rel=1e-4)
    dense = GcnSet2SetEncoder(F_, H, E, NCLS, 3, pred_hidden_dims=[20], bn=True)
    dense.load_state_dict(model.state_dict())
    dense = dense.cuda()
    yd = dense(RC.pad_rows(x, sizes, P).cuda(), adj.cuda(), sizes)
    ld = dense.loss(yd, label.cuda())
    ld.backward()
    close(ypred, yd)
    close(loss, ld, 1e-4, 1e-6)
    grads_close(model, {k: p.grad for k, p in dense.named_parameters()}, rtol=2e-3, atol_rel=1e-4)
