"""The link-prediction loss on the packed adjacency (bf16 rows of A and A^T: dp_linkpred_loss_fwd/bwd_packed,
dp_loss_forward/backward_packed) against the fp32 entries fed the dense batch — bit for bit, since both walk the same
tiles with the same values on a 0/1 adjacency — from the op level up to the captured training step."""
import gc

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.batch_builder import DeviceBatchBuilder, EdgeListDataset
from graph_pooling_amd.encoders import PackedAdjacency, SoftPoolingGcnEncoder
from graph_pooling_amd.tu_dataset import TUGraph
from oracle import diffpool_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DP_ERR_INVALID_ARG, DP_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assignment(B, n, K, nn_, seed):
    g = torch.Generator().manual_seed(seed)
    Sm = torch.softmax(torch.randn(B, n, K, generator=g) * 2, -1) * O.node_mask(n, nn_)
    Sm[0, 0] = 0.0
    Sm[0, 0, 1 % K] = 1.0        # a one-hot row: (S S^T)_00 == 1 exactly -> the tie branch of torch.min
    return Sm.cuda().contiguous()


def _both(lib, S, adj, nd, dloss, accumulate=0, dS0=None):
    """(loss, dS) of the fp32 entries on `adj` and of the packed entries on PackedAdjacency.from_dense(adj)."""
    B, n, K = S.shape
    pa = PackedAdjacency.from_dense(adj)
    wsb = lib.dp_linkpred_workspace_bytes(B, n, K)
    out = []
    for packed in (False, True):
        ws = torch.zeros(max(wsb, 256), device="cuda", dtype=torch.uint8)
        loss = torch.empty(1, device="cuda")
        dS = dS0.clone() if dS0 is not None else torch.empty_like(S)
        nptr = _lib.ptr(nd)
        if packed:
            _lib.check(lib.dp_linkpred_loss_fwd_packed(S.data_ptr(), pa.pk.data_ptr(), nptr, loss.data_ptr(), B, n, K,
                                                       ws.data_ptr(), wsb, _stream()), "fwd_packed")
            _lib.check(lib.dp_linkpred_loss_bwd_packed(S.data_ptr(), pa.pk.data_ptr(), pa.pkt.data_ptr(), nptr,
                                                       dloss.data_ptr(), dS.data_ptr(), accumulate, B, n, K,
                                                       ws.data_ptr(), wsb, _stream()), "bwd_packed")
        else:
            _lib.check(lib.dp_linkpred_loss_fwd(S.data_ptr(), adj.data_ptr(), nptr, loss.data_ptr(), B, n, K,
                                                ws.data_ptr(), wsb, _stream()), "fwd")
            _lib.check(lib.dp_linkpred_loss_bwd(S.data_ptr(), adj.data_ptr(), nptr, dloss.data_ptr(), dS.data_ptr(),
                                                accumulate, B, n, K, ws.data_ptr(), wsb, _stream()), "bwd")
        out.append((loss, dS))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ op level
GEOMS = [(3, 16, 4), (2, 100, 10), (3, 200, 20), (2, 150, 40), (2, 132, 50), (2, 130, 90), (1, 200, 128),
         (1, 140, 150), (1, 260, 256)]


@pytest.mark.parametrize("B,n,K", GEOMS)
def test_packed_link_loss_is_bit_identical_to_the_fp32_entries(lib, B, n, K):
    _, adj, nn_, _ = O.make_batch(B, n, 3, n_min=1, p=0.2, seed=K)
    S = _assignment(B, n, K, nn_, K)
    ad, nd = adj.cuda(), torch.from_numpy(nn_).cuda()
    (l0, d0), (l1, d1) = _both(lib, S, ad, nd, torch.tensor([1.7], device="cuda"))
    assert torch.isfinite(l0).all() and torch.isfinite(d0).all()
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert torch.equal(d0, d1), float((d0 - d1).abs().max())
    # and both are the reference loss (tests/test_gpu_ops.py::test_linkpred_loss has the gradient tolerance)
    torch.testing.assert_close(l1.cpu()[0], O.link_pred_loss(S.cpu(), adj, nn_), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,n,K", [(2, 150, 40), (1, 140, 150), (3, 200, 20)])
def test_asymmetric_adjacency_reads_a_from_pk_and_its_transpose_from_pkt(lib, B, n, K):
    """A directed 0/1 adjacency: pk != pkt.  The loss and dS are symmetric in A and A^T (P = S S^T is), so what shows
    that the backward reads A^T from pkt is that reading it from pk instead gives another dS."""
    _, adj, nn_, _ = O.make_batch(B, n, 3, n_min=n // 2, p=0.3, seed=K + 1)
    keep = torch.rand(B, n, n, generator=torch.Generator().manual_seed(3)) < 0.6
    adj = adj * keep                                 # drop edge directions independently: still 0/1, inside n_b
    assert not torch.equal(adj, adj.transpose(1, 2))
    S = _assignment(B, n, K, nn_, K + 1)
    ad, nd = adj.cuda().contiguous(), torch.from_numpy(nn_).cuda()
    pa = PackedAdjacency.from_dense(ad)
    assert not torch.equal(pa.pk, pa.pkt)
    (l0, d0), (l1, d1) = _both(lib, S, ad, nd, torch.tensor([0.6], device="cuda"))
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    torch.testing.assert_close(l1.cpu()[0], O.link_pred_loss(S.cpu(), adj, nn_), rtol=1e-5, atol=1e-6)
    wsb = lib.dp_linkpred_workspace_bytes(B, n, K)
    ws = torch.zeros(max(wsb, 256), device="cuda", dtype=torch.uint8)
    d_pk = torch.empty_like(S)
    _lib.check(lib.dp_linkpred_loss_bwd_packed(S.data_ptr(), pa.pk.data_ptr(), pa.pk.data_ptr(), nd.data_ptr(),
                                               torch.tensor([0.6], device="cuda").data_ptr(), d_pk.data_ptr(), 0, B, n,
                                               K, ws.data_ptr(), wsb, _stream()))
    assert not torch.equal(d_pk, d1)


@pytest.mark.parametrize("B,n,K", [(2, 100, 10), (1, 140, 150)])
def test_packed_link_loss_without_num_nodes_and_accumulating(lib, B, n, K):
    _, adj, nn_, _ = O.make_batch(B, n, 3, n_min=n // 2, p=0.2, seed=5)
    S = _assignment(B, n, K, [n] * B, 5)
    ad = adj.cuda()
    dloss = torch.tensor([1.3], device="cuda")
    (l0, d0), (l1, d1) = _both(lib, S, ad, None, dloss)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    torch.testing.assert_close(l1.cpu()[0], O.link_pred_loss(S.cpu(), adj, [n] * B), rtol=1e-5, atol=1e-6)
    base = torch.randn(B, n, K, generator=torch.Generator().manual_seed(9)).cuda()
    nd = torch.from_numpy(nn_).cuda()
    (_, a0), (_, a1) = _both(lib, S, ad, nd, dloss, accumulate=1, dS0=base)
    (_, f0), _ = _both(lib, S, ad, nd, dloss)
    assert torch.equal(a0, a1)
    assert not torch.equal(a1, base)
    torch.testing.assert_close(a1 - base, f0, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ module level
def _run(model, x, adj, nn_, label):
    model.zero_grad(set_to_none=True)
    y = model(x, adj, nn_, assign_x=x)
    loss = model.loss(y, label, adj, nn_)
    loss.backward()
    out = (y.detach().clone(), model.assign_tensor.detach().clone(), loss.detach().clone(),
           model.link_loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    model.assign_tensor = None
    return out


def _assert_runs_equal(r0, r1):
    (y0, s0, l0, k0, g0), (y1, s1, l1, k1, g1) = r0, r1
    assert torch.isfinite(y0).all() and torch.isfinite(l0)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    assert torch.equal(l0, l1) and torch.equal(k0, k1)
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_reference_golden_through_the_packed_adjacency(golden):
    a, params, _ = golden("g5_softpool_n100_f89_link")
    x = T(a["x"])
    B, N, F_ = x.shape
    H = params["conv_first.weight"].shape[1]
    E = params["conv_last.weight"].shape[1]
    K = params["assign_pred.weight"].shape[0]
    Cc = params["pred_model.2.weight"].shape[0]
    model = SoftPoolingGcnEncoder(N, F_, H, E, Cc, 3, H, assign_ratio=K / N + 1e-9, linkpred=True)
    model.load_state_dict(params)
    model = model.cuda()
    xd, ad, label = x.cuda(), T(a["adj"]).cuda(), T(a["label"]).cuda()
    dense = _run(model, xd, ad, a["num_nodes"], label)
    packed = _run(model, xd, PackedAdjacency.from_dense(ad), a["num_nodes"], label)
    _assert_runs_equal(dense, packed)
    torch.testing.assert_close(packed[2].cpu(), T(a["loss"]), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(packed[3].cpu(), T(a["link_loss"]), rtol=1e-5, atol=1e-6)


def _graphs(count, n_min, n_max, n_labels, p, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(n_min, n_max + 1))
        a = np.triu((rng.random((n, n)) < p).astype(np.float32), 1)
        out.append(TUGraph(a + a.T, rng.integers(0, n_labels, n), int(rng.integers(0, 2))))
    return out


def _model(N, F_, H, ratio, seed=0):
    torch.manual_seed(seed)
    return SoftPoolingGcnEncoder(N, F_, H, H, 2, 3, H, assign_ratio=ratio, linkpred=True).cuda()


@pytest.mark.parametrize("B,N,F_,H,ratio", [(6, 160, 8, 12, 0.1), (20, 500, 89, 20, 0.1)])
def test_packed_builder_with_link_loss_is_bit_identical_to_the_fp32_builder(B, N, F_, H, ratio):
    graphs = _graphs(B + 3, N // 4, N, F_, 0.03, seed=B + N + 1)
    ds = EdgeListDataset.from_tu_graphs(graphs)
    idx = list(range(1, B + 1))
    builder = DeviceBatchBuilder(ds, N, F_, "cuda")
    dense = builder.build(idx)
    packed = builder.build(idx, packed=True)
    assert isinstance(packed["adj"], PackedAdjacency)
    model = _model(N, F_, H, ratio)
    runs = []
    for batch in (dense, packed):
        runs.append(_run(model, batch["feats"], batch["adj"], batch["num_nodes_device"], batch["label"]))
    _assert_runs_equal(*runs)
    assert float(runs[1][3]) > 0.0


def test_captured_linkpred_training_step_follows_the_eager_training_loop():
    """Five training steps (different batches) of a linkpred model, eager on the packed batch and as
    CapturedTrainStep: same losses, same per-step link term in model.link_loss, same parameters."""
    from graph_pooling_amd.optim import FusedClipAdam
    from graph_pooling_amd.train_step import CapturedTrainStep
    B, N, F_, H = 6, 160, 8, 12
    graphs = _graphs(5 * B, N // 4, N, F_, 0.03, seed=78)
    ds = EdgeListDataset.from_tu_graphs(graphs)
    batches = [list(range(i * B, (i + 1) * B)) for i in range(5)]
    batches[2] = list(reversed(batches[2]))
    builder = DeviceBatchBuilder(ds, N, F_, "cuda")

    eager = _model(N, F_, H, 0.1, seed=5)
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
    eager.assign_tensor = None
    eager.link_loss = None
    gc.collect()

    cap = _model(N, F_, H, 0.1, seed=5)
    opt_c = FusedClipAdam(cap, lr=1e-2, clip=2.0, device_step_counter=True)
    p_init = {k: v.detach().clone() for k, v in cap.named_parameters()}
    step = CapturedTrainStep(cap, opt_c, builder, B, linkpred=True)
    for k, v in cap.named_parameters():              # capturing (and its warm-up) left the model where it was
        assert torch.equal(v.detach(), p_init[k]), k
    losses_c, links_c = [], []
    for idx in batches:
        losses_c.append(float(step(idx)))
        links_c.append(float(cap.link_loss))
    assert step.skipped_entries() == 0
    assert int(opt_c.step_dev.item()) == 5 and opt_c.step_count == 5
    np.testing.assert_allclose(losses_c, losses_e, rtol=1e-5)
    np.testing.assert_allclose(links_c, links_e, rtol=1e-5)
    assert len(set(links_c)) == 5 and min(links_c) > 0.0
    for (k, pe), (_, pc) in zip(eager.named_parameters(), cap.named_parameters()):
        np.testing.assert_allclose(pc.detach().cpu().numpy(), pe.detach().cpu().numpy(), rtol=2e-5, atol=2e-6,
                                   err_msg=k)


# ------------------------------------------------------------------ refusals
def test_packed_adjacency_of_another_batch_shape_is_refused_before_any_launch():
    B, N, F_ = 4, 128, 5
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=N // 2, p=0.05, seed=2)
    model = _model(N, F_, 8, 0.1)
    xd, ad = x.cuda(), adj.cuda()
    with torch.no_grad():
        y = model(xd, ad, nn_, assign_x=xd)
        for wrong in (PackedAdjacency.from_dense(ad[:B - 1]),
                      PackedAdjacency.from_dense(ad[:, :N - 8, :N - 8].contiguous())):
            with pytest.raises(ValueError, match="does not match the assignment"):
                model.loss(y, label.cuda(), wrong, nn_)
        ok = model.loss(y, label.cuda(), PackedAdjacency.from_dense(ad), nn_)      # the right one is accepted
        dense = model.loss(y, label.cuda(), ad, nn_)
    assert torch.equal(ok, dense)


def test_packed_entries_refuse_what_the_fp32_ones_refuse(lib):
    B, n, K = 1, 64, 257
    S = torch.zeros(B, n, K, device="cuda")
    adj = torch.zeros(B, n, n, device="cuda")
    pa = PackedAdjacency.from_dense(adj)
    wsb = lib.dp_linkpred_workspace_bytes(B, n, K)
    ws = torch.zeros(max(wsb, 256), device="cuda", dtype=torch.uint8)
    loss = torch.empty(1, device="cuda")
    dS = torch.empty_like(S)
    calls = {
        "fwd": (lib.dp_linkpred_loss_fwd(S.data_ptr(), adj.data_ptr(), None, loss.data_ptr(), B, n, K, ws.data_ptr(),
                                         wsb, _stream()), lib.dp_last_error_string()),
        "fwd_packed": (lib.dp_linkpred_loss_fwd_packed(S.data_ptr(), pa.pk.data_ptr(), None, loss.data_ptr(), B, n, K,
                                                       ws.data_ptr(), wsb, _stream()), lib.dp_last_error_string()),
        "bwd": (lib.dp_linkpred_loss_bwd(S.data_ptr(), adj.data_ptr(), None, None, dS.data_ptr(), 0, B, n, K,
                                         ws.data_ptr(), wsb, _stream()), lib.dp_last_error_string()),
        "bwd_packed": (lib.dp_linkpred_loss_bwd_packed(S.data_ptr(), pa.pk.data_ptr(), pa.pkt.data_ptr(), None, None,
                                                       dS.data_ptr(), 0, B, n, K, ws.data_ptr(), wsb, _stream()),
                       lib.dp_last_error_string()),
    }
    assert calls["fwd"] == calls["fwd_packed"] and calls["fwd"][0] == DP_ERR_UNSUPPORTED, calls
    assert calls["bwd"] == calls["bwd_packed"] and calls["bwd"][0] == DP_ERR_UNSUPPORTED, calls
    for rc, _ in calls.values():
        with pytest.raises(RuntimeError, match="K=257 clusters exceed"):
            _lib.check(rc)
    # a NULL A^T on the backward entry is an argument error, nothing is launched
    K = 8
    S8 = torch.zeros(B, n, K, device="cuda")
    d8 = torch.empty_like(S8)
    rc = lib.dp_linkpred_loss_bwd_packed(S8.data_ptr(), pa.pk.data_ptr(), None, None, None, d8.data_ptr(), 0, B, n, K,
                                         ws.data_ptr(), wsb, _stream())
    assert rc == DP_ERR_INVALID_ARG and b"adj_pkt" in lib.dp_last_error_string()
    torch.cuda.synchronize()
