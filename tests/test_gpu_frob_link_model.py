"""The Frobenius link objective through the model classes: SoftPoolingGcnEncoder(linkpred="frobenius") on dense and packed
batches against the linkpred=False model plus the direct double sum written in plain torch ops on its attached
assign_tensor (both arms share one forward bit for bit); the trace identity with the pooled adjacency; the CSR class
against the dense class; reproducible training; and — last in the file — CapturedTrainStep against the eager loop."""
import numpy as np
import pytest
import torch

from graph_pooling_amd.batch_builder import DeviceBatchBuilder, EdgeListDataset
from graph_pooling_amd.encoders import PackedAdjacency, SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseSoftPoolingGcnEncoder
from graph_pooling_amd.tu_dataset import TUGraph
from oracle import diffpool_oracle as O
from tests import frob_link_cases as FC
from tests.parity import close, gpu_winners, grads_close

pytestmark = pytest.mark.gpu

W_ENT = 0.3


def F_torch(S, adj, n_b):
    """The definition in plain fp32 torch ops on the attached assignment [B, N, K]: sum_b ||A_b - S_b S_b^T||_F^2 over
    the leading n_b x n_b blocks, divided by sum_b n_b^2."""
    B, N, _ = S.shape
    n_b = [N] * B if n_b is None else [int(v) for v in n_b]
    total = 0.0
    for b, n in enumerate(n_b):
        s = S[b, :n]
        r = adj[b, :n, :n] - s @ s.t()
        total = total + (r * r).sum()
    return total / float(sum(n * n for n in n_b))


def _pair(N, F_, H, ratio, num_pooling, ent_w, seed=2, ncls=3):
    """Two models from one seed: linkpred='frobenius' and linkpred=False."""
    out = []
    for link in ("frobenius", False):
        m = SoftPoolingGcnEncoder(N, F_, H, H, ncls, 3, H, assign_ratio=ratio, num_pooling=num_pooling, linkpred=link,
                                  assign_ent_weight=ent_w)
        params = O.init_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed, bias_scale=0.1)
        m.load_state_dict(params)
        out.append(m.cuda())
    return out


@pytest.mark.parametrize("ent_w", [0.0, W_ENT], ids=["no_entropy", "entropy"])
@pytest.mark.parametrize("num_pooling", [1, 2])
@pytest.mark.parametrize("B,N,F_,H,ratio", [(4, 100, 8, 12, 0.25), (20, 500, 89, 20, 0.1)], ids=["B4_N100", "DD"])
def test_dense_loss_and_gradients_equal_torch_autograd_of_the_direct_formula(B, N, F_, H, ratio, num_pooling, ent_w):
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=N // 4, p=0.05, seed=B + N, n_classes=3)
    model, model0 = _pair(N, F_, H, ratio, num_pooling, ent_w)
    assert model.linkpred is True and model.link_objective == "frobenius"
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()

    y = model(xd, ad, nn_, assign_x=xd)
    loss = model.loss(y, ld, ad, nn_)
    loss.backward()
    y0 = model0(xd, ad, nn_, assign_x=xd)
    assert torch.equal(y, y0) and torch.equal(model.assign_tensor, model0.assign_tensor)    # the forward is untouched
    f_t = F_torch(model0.assign_tensor, ad, nn_)
    base = model0.loss(y0, ld, None, nn_) if ent_w > 0 else model0.loss(y0, ld)
    ref = base + f_t
    ref.backward()
    close(loss, ref)
    close(model.link_loss, f_t)
    link = model.link_loss
    assert link.dim() == 0 and link.is_cuda and not link.requires_grad and float(link) > 0
    grads_close(model, {k: p.grad for k, p in model0.named_parameters()})
    # the total is fl(base + link) in fp32 exactly: the finishing kernel adds the term itself (the entropy term, when
    # on, is added after it)
    if ent_w == 0:
        want = base.detach().cpu().numpy() + link.cpu().numpy()
        assert loss.detach().cpu().numpy().tobytes() == np.float32(want).tobytes()
    # and it is NOT the cross-entropy link term
    bce = SoftPoolingGcnEncoder(N, F_, H, H, 3, 3, H, assign_ratio=ratio, num_pooling=num_pooling, linkpred=True).cuda()
    bce.load_state_dict(model.state_dict())
    yb = bce(xd, ad, nn_, assign_x=xd)
    bce.loss(yb, ld, ad, nn_)
    assert abs(float(bce.link_loss) - float(link)) > 1e-3 * float(link)


def test_link_loss_times_the_normaliser_is_t0_minus_twice_the_trace_of_the_pooled_adjacency_plus_gram():
    """link * sum n_b^2 = T0 - 2 tr(S^T A S) + ||S^T S||^2 with S^T A S the model's own level-0 pooled adjacency
    (saved_activation(0, 'adjpool')): T1 from an independent kernel.  Tolerance: the op bound of the term plus the
    forward parity tolerance (rtol 1e-4, tests/parity.py) on the pooled adjacency's trace, which enters twice."""
    B, N, F_, H = 4, 100, 8, 12
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=25, p=0.05, seed=9, n_classes=3)
    model, _ = _pair(N, F_, H, 0.25, 1, 0.0)
    xd, ad = x.cuda(), adj.cuda()
    y = model(xd, ad, nn_, assign_x=xd)
    model.loss(y, label.cuda(), ad, nn_)
    S = model.assign_tensor.detach().cpu().double().numpy()
    A = adj.double().numpy()
    graphs = [(A[b, :n, :n], S[b, :n]) for b, n in enumerate(int(v) for v in nn_)]
    ref = FC.batch_ref(graphs)
    t0 = sum(float((a * a).sum()) for a, _ in graphs)
    t2 = sum(float(((s.T @ s) ** 2).sum()) for _, s in graphs)
    ap = model.saved_activation(0, "adjpool").detach().cpu().double()
    tr = float(sum(torch.trace(ap[b]) for b in range(B)))
    got = float(model.link_loss) * ref["norm"]
    assert abs(got - (t0 - 2.0 * tr + t2)) <= FC.fwd_bound(ref) * ref["norm"] + 2.0 * 1e-4 * abs(tr), \
        (got, t0 - 2.0 * tr + t2, t0, tr, t2)


def _graphs(count, n_min, n_max, n_labels, p, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(n_min, n_max + 1))
        a = np.triu((rng.random((n, n)) < p).astype(np.float32), 1)
        out.append(TUGraph(a + a.T, rng.integers(0, n_labels, n), int(rng.integers(0, 2))))
    return out


def _builder_model(N, F_, H, seed, ent_w=0.0):
    torch.manual_seed(seed)
    return SoftPoolingGcnEncoder(N, F_, H, H, 2, 3, H, assign_ratio=0.1, linkpred="frobenius",
                                 assign_ent_weight=ent_w).cuda()


@pytest.mark.parametrize("ent_w", [0.0, W_ENT], ids=["no_entropy", "entropy"])
def test_packed_batch_is_bit_identical_to_the_dense_fp32_batch(ent_w):
    B, N, F_, H = 6, 160, 8, 12
    ds = EdgeListDataset.from_tu_graphs(_graphs(B + 3, N // 4, N, F_, 0.03, seed=B + N))
    builder = DeviceBatchBuilder(ds, N, F_, "cuda")
    idx = list(range(1, B + 1))
    model = _builder_model(N, F_, H, 0, ent_w)
    outs = []
    for batch in (builder.build(idx), builder.build(idx, packed=True)):
        assert isinstance(batch["adj"], PackedAdjacency) == bool(outs)
        model.zero_grad(set_to_none=True)
        y = model(batch["feats"], batch["adj"], batch["num_nodes_device"], assign_x=batch["assign_feats"])
        loss = model.loss(y, batch["label"], batch["adj"], batch["num_nodes_device"])
        loss.backward()
        outs.append((loss.detach().clone(), model.link_loss.clone(),
                     {k: p.grad.clone() for k, p in model.named_parameters()}))
    (l0, k0, g0), (l1, k1, g1) = outs
    assert torch.isfinite(l0) and float(k0) > 0
    assert torch.equal(l0, l1) and torch.equal(k0, k1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_every_way_of_starting_the_backward_pass_agrees():
    B, N, F_, H = 5, 40, 4, 8
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=5, p=0.15, seed=11, n_classes=3)
    model, _ = _pair(N, F_, H, 0.25, 1, W_ENT)
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()

    def grads(run):
        model.zero_grad(set_to_none=True)
        run(model.loss(model(xd, ad, nn_, assign_x=xd), ld, ad, nn_))
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in model.named_parameters()}

    fast = grads(lambda l: l.backward())
    slow = grads(lambda l: (l * 1).backward())
    twice = grads(lambda l: l.backward(gradient=torch.full((), 2.0, device="cuda")))
    for k in fast:
        close(slow[k], fast[k], 1e-5, 1e-8)
        close(twice[k], 2 * fast[k], 1e-4, 1e-6 * max(1.0, float(fast[k].abs().max())))


# ----------------------------------------------------------------------------- CSR
def _edge_lists(sizes, seed, deg=3):
    rng = np.random.default_rng(seed)
    srcs, dsts = [], []
    for n in sizes:
        s, d = rng.integers(1, n, n * deg), rng.integers(1, n, n * deg)
        keep = s != d
        srcs.append(s[keep])
        dsts.append(d[keep])
    return srcs, dsts


def _dense_adj(sizes, srcs, dsts, N):
    adj = torch.zeros(len(sizes), N, N)
    for b, (s, d) in enumerate(zip(srcs, dsts)):
        adj[b, s, d] = 1.0
        adj[b, d, s] = 1.0
    return adj


def _pad_rows(x, sizes, N):
    out = torch.zeros(len(sizes), N, x.shape[1], dtype=x.dtype)
    o = 0
    for b, n in enumerate(sizes):
        out[b, :n] = x[o:o + n]
        o += n
    return out


def _dense_and_sparse(sizes, K0, num_pooling=1, ent_w=0.0, seed=9):
    """The dense class on the graphs padded to N = max n_b and the CSR class holding its state_dict."""
    N, F_, H, ncls = max(sizes), 7, 16, 4
    ratio = (K0 + 0.5) / N
    srcs, dsts = _edge_lists(sizes, 21)
    adj = _dense_adj(sizes, srcs, dsts, N)
    x = torch.randn(sum(sizes), F_, generator=torch.Generator().manual_seed(4))
    label = torch.tensor([b % ncls for b in range(len(sizes))])
    kw = dict(assign_ratio=ratio, num_pooling=num_pooling, linkpred="frobenius", assign_ent_weight=ent_w)
    dense = SoftPoolingGcnEncoder(N, F_, H, H, ncls, 3, H, **kw)
    assert dense.assign_dims[0] == K0
    dense.load_state_dict(O.init_params({k: tuple(v.shape) for k, v in dense.state_dict().items()}, seed=seed,
                                        bias_scale=0.5))
    dense = dense.cuda()
    sparse = SparseSoftPoolingGcnEncoder(N, F_, H, H, ncls, 3, H, **kw)
    sparse.load_state_dict(dense.state_dict())                    # dense -> CSR transfer
    return dense, sparse.cuda(), adj, x, label, N


@pytest.mark.parametrize("sizes,K0", [([64], 16), ([300], 30), ([5748], 50), ([30, 12, 41], 10)],
                         ids=["graph64", "graph300", "graph5748", "batch"])
def test_csr_class_equals_the_dense_class_on_the_padded_graphs(sizes, K0):
    """Loss, link_loss and every gradient of the CSR class (one CsrGraph; a CsrBatch) against the dense class with the
    same state_dict (load_state_dict moves it) on the same graphs padded to max n_b, at the tolerances
    tests/test_gpu_csr_batch.py uses for its dense comparisons (loss 1e-4 / 1e-6, gradients grads_close(2e-3, 1e-4)).
    The max readouts must pick the same rows for the gradients to be comparable: checked first."""
    dense, sparse, adj, x, label, N = _dense_and_sparse(sizes, K0, ent_w=W_ENT if len(sizes) > 1 else 0.0)
    xp, ad = _pad_rows(x, sizes, N).cuda(), adj.cuda()
    yd = dense(xp, ad, np.array(sizes), assign_x=xp)
    ld_ = dense.loss(yd, label.cuda(), ad, np.array(sizes))
    ld_.backward()
    graph = CsrGraph.from_dense(ad[0]) if len(sizes) == 1 else CsrBatch.from_dense(ad, sizes, pad_to=N)
    ys = sparse(x.cuda(), graph)
    ls = sparse.loss(ys, label.cuda(), graph)
    ls.backward()
    close(ys, yd)
    close(ls, ld_, 1e-4, 1e-6)
    close(sparse.link_loss, dense.link_loss, 1e-4, 1e-6)
    assert float(sparse.link_loss.detach()) > 0
    for a, b in zip(gpu_winners(sparse, 2), gpu_winners(dense, 2)):
        assert torch.equal(a, b), "the two paths picked different max-readout rows: gradients are not comparable"
    grads_close(sparse, {k: p.grad for k, p in dense.named_parameters()}, rtol=2e-3, atol_rel=1e-4)


def test_training_with_the_frobenius_term_is_bit_reproducible_and_descends():
    """Three steps of plain SGD on a 5748-node graph (DD's largest), twice from the same parameters."""
    n, F_, H, Cc = 5748, 9, 20, 3
    rng = np.random.default_rng(n)
    src, dst = rng.integers(1, n, 3 * n), rng.integers(1, n, 3 * n)
    keep = src != dst
    g = CsrGraph.from_edges(n, src[keep], dst[keep], "cuda", symmetric=True)
    x = torch.randn(n, F_, generator=torch.Generator().manual_seed(n)).cuda()
    model = SparseSoftPoolingGcnEncoder(500, F_, H, H, Cc, 3, H, assign_ratio=0.1, linkpred="frobenius")
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=n + 1, bias_scale=0.1)
    model = model.cuda()
    label = torch.tensor([1], device="cuda")

    def train():
        model.load_state_dict(params)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        losses, links = [], []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = model.loss(model(x, g), label, g)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            links.append(float(model.link_loss))
        return losses, links, {k: p.detach().clone() for k, p in model.named_parameters()}

    l1, k1, p1 = train()
    l2, k2, p2 = train()
    assert l1 == l2 and k1 == k2
    for k in p1:
        assert torch.isfinite(p1[k]).all(), k
        assert torch.equal(p1[k], p2[k]), k
    assert l1[0] > l1[1] > l1[2], l1


# ----------------------------------------------------------------------------- captured step: LAST in this file
def test_captured_training_step_follows_the_eager_training_loop():
    """As tests/test_gpu_train_step.py does it and at its tolerances, with the Frobenius term in the objective.  Every
    reference to the eager losses and outputs is dropped before the capture (a live autograd graph at capture time is a
    known crash of the runtime's capture_end)."""
    from graph_pooling_amd.optim import FusedClipAdam
    from graph_pooling_amd.train_step import CapturedTrainStep
    B, N, F_, H = 6, 160, 8, 12
    ds = EdgeListDataset.from_tu_graphs(_graphs(5 * B, N // 4, N, F_, 0.03, seed=77))
    batches = [list(range(i * B, (i + 1) * B)) for i in range(5)]
    batches[3] = list(reversed(batches[3]))
    builder = DeviceBatchBuilder(ds, N, F_, "cuda")

    eager = _builder_model(N, F_, H, 4)
    opt_e = FusedClipAdam(eager, lr=1e-2, clip=2.0)
    losses_e, links_e = [], []
    for idx in batches:
        b = builder.build(idx, packed=True)
        eager.zero_grad(set_to_none=True)
        y = eager(b["feats"], b["adj"], b["num_nodes_device"], assign_x=b["feats"])
        loss = eager.loss(y, b["label"], b["adj"], b["num_nodes_device"])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
        links_e.append(float(eager.link_loss))
    del y, loss, b
    eager.link_loss = None

    cap = _builder_model(N, F_, H, 4)
    opt_c = FusedClipAdam(cap, lr=1e-2, clip=2.0, device_step_counter=True)
    p_init = {k: v.detach().clone() for k, v in cap.named_parameters()}
    step = CapturedTrainStep(cap, opt_c, builder, B, linkpred=True)
    for k, v in cap.named_parameters():
        assert torch.equal(v.detach(), p_init[k]), k
    losses_c, links_c = [], []
    for idx in batches:
        losses_c.append(float(step(idx)))
        links_c.append(float(cap.link_loss))
    assert step.skipped_entries() == 0
    np.testing.assert_allclose(losses_c, losses_e, rtol=1e-5)
    np.testing.assert_allclose(links_c, links_e, rtol=1e-5)
    assert len(set(losses_c)) == 5 and len(set(links_c)) == 5
    for (k, pe), (_, pc) in zip(eager.named_parameters(), cap.named_parameters()):
        np.testing.assert_allclose(pc.detach().cpu().numpy(), pe.detach().cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
