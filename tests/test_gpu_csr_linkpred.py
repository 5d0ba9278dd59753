"""Link-prediction loss on CSR graphs (dp_csr_linkpred_loss_fwd / bwd, encoders.py:1309-1331 on ONE graph without an
n x n adjacency): the op against the direct formula in float64 on a densified adjacency, against the dense kernels
(dp_linkpred_loss_*), at n = 65 536 against a chunked float64 evaluation, and SparseSoftPoolingGcnEncoder(linkpred=True)
against the oracle's dense restatement (PARITY UNPINNED by the reference, which drops such graphs, load_data.py:79),
against the dense class, and as a bit-reproducible training loop.

Tolerances are those of the dense link-loss test (test_gpu_ops.py::test_linkpred_loss): loss rtol 1e-5 / atol 1e-6,
dS rtol 1e-3 with an absolute floor of 2e-5 x the largest reference entry.  The dense kernels this file compares with
are themselves anchored to float64, at counted bounds, by tests/test_gpu_linkpred_matrix.py.  Every op case first shows that the direct fp32 formula (the oracle's
link_pred_loss) meets the same tolerance against float64 on that input: where it does not, the input is wrong for a
tolerance test (fp32 resolves 1 - p to 6e-8 when assignments are sharp) and belongs to the anchored test below."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import CsrGraph, SparseSoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests.parity import close, grads_close, gpu_winners

pytestmark = pytest.mark.gpu

EPS = 1e-7


# ------------------------------------------------------------------ inputs and references
def _edges(n, deg, seed, loops=False):
    """Random edge list with mean out-degree ~deg; node 0 has no edge at all (n > 1).  `loops` adds self loops."""
    if n == 1:
        return np.array([0]), np.array([0])          # one node: a self loop (the CSR arrays must not be empty)
    rng = np.random.default_rng(seed)
    m = max(n * deg, 4)
    src, dst = rng.integers(1, n, m), rng.integers(1, n, m)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    if n == 2 or src.size == 0:                      # nodes 1.. cannot form an edge: give node 1 a self loop
        loops = True
    if loops:
        own = np.array([v for v in (1, 2, 5) if v < n])
        src, dst = np.concatenate([src, own]), np.concatenate([dst, own])
    return src, dst


def _graph(n, deg, seed, directed, loops=False):
    src, dst = _edges(n, deg, seed, loops)
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=not directed)
    A = torch.zeros(n, n, dtype=torch.float64)
    A[src, dst] = 1.0
    if not directed:
        A = torch.maximum(A, A.t())
    assert int(A.sum()) == g.indices.numel()         # the CSR lists every (i, j) exactly once
    assert n == 1 or (float(A[0].sum()) == 0 and float(A[:, 0].sum()) == 0)
    return g, A


def _assign(n, K, sharp, seed, onehot):
    gen = torch.Generator().manual_seed(seed)
    S = torch.softmax(torch.randn(n, K, generator=gen) * sharp, -1)
    if onehot and n >= 2:                            # rows 0 and 1 one-hot on the same cluster: <S_0, S_1> == 1 exactly,
        S[:2] = 0.0                                  # the tie branch of torch.min (and P_00 = P_11 = 1 on the diagonal)
        S[:2, min(1, K - 1)] = 1.0
    return S


def _direct(S, A, dtype, dloss=1.0):
    """The reference's formula as written, on the dense adjacency: (loss, dloss * d loss / dS)."""
    n = S.shape[0]
    s = S.to(dtype).clone().requires_grad_(True)
    a = A.to(dtype)
    p = torch.minimum(s @ s.t(), torch.ones((), dtype=dtype))
    ll = -a * torch.log(p + EPS) - (1 - a) * torch.log(1 - p + EPS)
    loss = ll.sum() / float(n * n)
    (loss * dloss).backward()
    return loss.detach(), s.grad


def _oracle32(S, A, dloss=1.0):
    s = S.clone().requires_grad_(True)
    lo = O.link_pred_loss(s[None], A.float()[None], None)
    (lo * dloss).backward()
    return lo.detach(), s.grad


def _ds_close(got, ref, offset=0.0):
    """rtol 1e-3 with the floor 2e-5 x max|dS_ref|; `offset`: what dS held before an accumulating call."""
    close(got, ref + offset, 1e-3, 2e-5 * float(ref.abs().max()))


def _run(lib, S_host, g, pad=0, dloss=None, accumulate=0, fill=0.0):
    """dp_csr_linkpred_loss_fwd + bwd on S [n, K] stored with row stride K + pad -> (loss [1], dS [n, K] view)."""
    n, K = S_host.shape
    S = torch.zeros(n, K + pad, device="cuda")[:, :K]
    S.copy_(S_host)
    dS = torch.full((n, K + pad), fill if accumulate else float("nan"), device="cuda")[:, :K]
    loss = torch.full((1,), float("nan"), device="cuda")
    wsb = lib.dp_csr_linkpred_workspace_bytes(n, K)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    dl = None if dloss is None else torch.tensor([dloss], device="cuda")
    st = _lib.current_stream()
    _lib.check(lib.dp_csr_linkpred_loss_fwd(S.data_ptr(), S.stride(0), g.indptr.data_ptr(), g.indices.data_ptr(),
                                            loss.data_ptr(), n, K, ws.data_ptr(), wsb, st), "dp_csr_linkpred_loss_fwd")
    _lib.check(lib.dp_csr_linkpred_loss_bwd(S.data_ptr(), S.stride(0), g.indptr.data_ptr(), g.indices.data_ptr(),
                                            g.indptr_t.data_ptr(), g.indices_t.data_ptr(), _lib.ptr(dl), dS.data_ptr(),
                                            dS.stride(0), accumulate, n, K, ws.data_ptr(), wsb, st),
               "dp_csr_linkpred_loss_bwd")
    torch.cuda.synchronize()
    return loss, dS


# (n, K, directed, row padding, self loops, one-hot pair, accumulate, dloss): n in {1, 7, 63, 64, 65, 300, 1000, 5748}
# and K in {1, 7, 50, 64, 256}; K % 4 == 0 with a dense stride takes the 16-byte gather, a padded stride (or any other
# K) the 4-byte one; node 0 is isolated in every graph with n > 1
OP_CASES = [
    (1, 1, False, 0, False, False, 0, None), (1, 50, True, 0, False, False, 1, 1.7),
    (7, 7, True, 3, False, True, 0, 1.7), (7, 256, False, 0, False, False, 1, None),
    (63, 50, False, 0, False, True, 1, 1.7), (63, 64, True, 0, False, False, 0, None),
    (64, 64, False, 0, False, True, 0, 1.7), (64, 1, True, 0, False, False, 1, None),
    (65, 64, False, 3, False, False, 1, 1.7), (65, 7, True, 0, True, False, 0, None),
    (300, 50, False, 0, False, True, 0, 1.7), (300, 50, True, 3, False, False, 1, None),
    (300, 256, True, 0, False, True, 0, None), (300, 64, False, 0, True, True, 1, 1.7),
    (300, 64, True, 3, True, False, 0, 1.7), (300, 1, False, 0, False, False, 0, 1.7),
    (1000, 64, False, 0, False, False, 0, None), (1000, 256, False, 3, False, False, 1, 1.7),
    (1000, 256, True, 0, False, False, 0, 1.7), (1000, 7, True, 0, False, True, 1, None),
    (1000, 50, True, 0, False, False, 0, 1.7), (1000, 128, False, 0, False, False, 1, None),
    (5748, 50, False, 0, False, False, 0, 1.7), (5748, 64, True, 0, False, True, 1, None),
]


@pytest.mark.parametrize("n,K,directed,pad,loops,onehot,accumulate,dloss", OP_CASES)
def test_csr_link_loss_matches_direct_float64(n, K, directed, pad, loops, onehot, accumulate, dloss):
    lib = _lib.load()
    g, A = _graph(n, 5, n * 11 + K, directed, loops)
    S = _assign(n, K, 1.0 if K == 256 else 2.0, n + K, onehot)
    dl = 1.0 if dloss is None else dloss
    l64, d64 = _direct(S, A, torch.float64, dl)
    # the input qualifies only if the direct fp32 formula itself meets the tolerance on it
    l32, d32 = _oracle32(S, A, dl)
    print(f"n={n} K={K}: oracle32 vs fp64: loss rel {abs(float(l32) - float(l64)) / abs(float(l64)):.1e}, "
          f"dS max err / max {float((d32.double() - d64).abs().max() / d64.abs().max()):.1e}")
    close(l32, l64, 1e-5, 1e-6)
    _ds_close(d32, d64)

    fill = 0.25 * float(d64.abs().max())
    loss, dS = _run(lib, S, g, pad, dloss, accumulate, fill)
    print(f"          hip vs fp64: loss rel {abs(float(loss) - float(l64)) / abs(float(l64)):.1e}, "
          f"dS max err / max {float((dS.cpu().double() - (d64 + (fill if accumulate else 0))).abs().max() / d64.abs().max()):.1e}")
    close(loss[0], l64, 1e-5, 1e-6)
    _ds_close(dS, d64, fill if accumulate else 0.0)
    loss2, dS2 = _run(lib, S, g, pad, dloss, accumulate, fill)
    assert torch.equal(loss, loss2) and torch.equal(dS, dS2)


@pytest.mark.parametrize("K,sharp", [(50, 12.0), (7, 6.0)])
def test_sharp_assignments_no_worse_than_the_fp32_formula_vs_fp64(K, sharp):
    """softmax(12 randn) at K = 50 / softmax(6 randn) at K = 7, n = 2000: many p_ij sit within a few ulp of 1, where fp32
    resolves 1 - p to 6e-8 and the direct fp32 formula is itself far from float64.  No tolerance test is possible on
    such input; the kernels are held to the project's anchored criterion instead,
    max|dS_hip - dS_64| <= 4 max|dS_oracle32 - dS_64| + 3e-7 max|dS_64|, and must stay finite and bit-reproducible."""
    lib = _lib.load()
    n = 2000
    g, A = _graph(n, 5, 77 + K, False)
    S = _assign(n, K, sharp, 5 + K, False)
    l64, d64 = _direct(S, A, torch.float64)
    l32, d32 = _oracle32(S, A)
    loss, dS = _run(lib, S, g)
    loss2, dS2 = _run(lib, S, g)
    assert torch.isfinite(loss).all() and torch.isfinite(dS).all()
    assert torch.equal(loss, loss2) and torch.equal(dS, dS2)
    e_hip = float((dS.cpu().double() - d64).abs().max())
    e_o32 = float((d32.double() - d64).abs().max())
    top = float(d64.abs().max())
    print(f"K={K}: max|dS_64| {top:.3e}; oracle32 err {e_o32:.3e} ({e_o32 / top:.2e} of max); hip err {e_hip:.3e} "
          f"({e_hip / top:.2e}); loss 64 / 32 / hip: {float(l64):.8f} {float(l32):.8f} {float(loss):.8f}")
    assert e_hip <= 4 * e_o32 + 3e-7 * top
    assert abs(float(loss) - float(l64)) <= 4 * abs(float(l32) - float(l64)) + 1e-6 * abs(float(l64))


@pytest.mark.parametrize("n", [300, 5748])
def test_csr_link_loss_agrees_with_the_dense_kernels(n):
    """dp_linkpred_loss_fwd / bwd with B = 1 on the densified adjacency.  Agreement to the tolerances, not bit identity:
    the CSR path sums the decomposed form (dense term over the upper triangle + edge term), the dense path the direct
    one."""
    lib = _lib.load()
    K = 50
    g, A = _graph(n, 5, n + 3, False)
    S = _assign(n, K, 2.0, n, True)
    loss, dS = _run(lib, S, g, dloss=1.7)
    Sd, Ad = S.cuda().contiguous(), A.float().cuda().contiguous()
    wsb = lib.dp_linkpred_workspace_bytes(1, n, K)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    lo, dSo = torch.empty(1, device="cuda"), torch.empty_like(Sd)
    dl = torch.tensor([1.7], device="cuda")
    st = _lib.current_stream()
    _lib.check(lib.dp_linkpred_loss_fwd(Sd.data_ptr(), Ad.data_ptr(), None, lo.data_ptr(), 1, n, K, ws.data_ptr(), wsb,
                                        st), "dp_linkpred_loss_fwd")
    _lib.check(lib.dp_linkpred_loss_bwd(Sd.data_ptr(), Ad.data_ptr(), None, dl.data_ptr(), dSo.data_ptr(), 0, 1, n, K,
                                        ws.data_ptr(), wsb, st), "dp_linkpred_loss_bwd")
    torch.cuda.synchronize()
    close(loss, lo, 1e-5, 1e-6)
    _ds_close(dS, dSo)


def test_csr_link_loss_at_65536_nodes_matches_chunked_float64():
    """n = 65 536, K = 64, ~10 neighbours per row: the dense path cannot hold this graph (17 GB of adjacency).  The
    reference is the direct formula in float64, evaluated with plain torch on the device in row chunks (autograd per
    chunk; nothing of the library).  Loss rtol x 10 for a sum of 4 10^9 terms, as the 2^20-row pooling test allows."""
    lib = _lib.load()
    n, K, chunk = 65536, 64, 512
    src, dst = _edges(n, 5, 19)
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)
    S = _assign(n, K, 2.0, 23, False)
    loss, dS = _run(lib, S, g)
    loss2, dS2 = _run(lib, S, g)
    assert torch.equal(loss, loss2) and torch.equal(dS, dS2)

    s64 = S.double().cuda().requires_grad_(True)
    ip, ix = g.indptr.long(), g.indices.long()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), ip[1:] - ip[:-1])
    one = torch.ones((), dtype=torch.float64, device="cuda")
    total = torch.zeros((), dtype=torch.float64, device="cuda")
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        e0, e1 = int(ip[r0]), int(ip[r1])
        a = torch.zeros(r1 - r0, n, dtype=torch.float64, device="cuda")
        a[rows[e0:e1] - r0, ix[e0:e1]] = 1.0
        p = torch.minimum(s64[r0:r1] @ s64.t(), one)
        part = (-a * torch.log(p + EPS) - (1 - a) * torch.log(1 - p + EPS)).sum() / float(n) / float(n)
        part.backward()
        total += part.detach()
    close(loss[0], total, 1e-4, 1e-6)
    _ds_close(dS, s64.grad)


# ------------------------------------------------------------------ the model
def _model_case(n, num_pooling, max_nodes=500, ratio=0.1):
    F_, H, E, Cc = 9, 20, 20, 3
    src, dst = _edges(n, 3, n)
    g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=True)           # node 0 stays isolated
    adj = torch.zeros(n, n)
    adj[src, dst] = 1.0
    adj = torch.maximum(adj, adj.t())
    x = torch.randn(n, F_, generator=torch.Generator().manual_seed(n))
    model = SparseSoftPoolingGcnEncoder(max_nodes, F_, H, E, Cc, 3, H, assign_ratio=ratio, num_pooling=num_pooling,
                                        pred_hidden_dims=[50], linkpred=True)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=n + num_pooling,
                           bias_scale=0.1)
    model.load_state_dict(params)
    return model.cuda(), params, g, adj, x, Cc


@pytest.mark.parametrize("num_pooling", [1, 2])
@pytest.mark.parametrize("n", [64, 300, 5748])
def test_sparse_diffpool_with_link_loss_equals_dense_oracle_PARITY_UNPINNED(n, num_pooling):
    """As test_gpu_sparse_pool.py's model test, with linkpred=True: forward first, then the oracle (dense, B = 1, N = n)
    with the winners the HIP forward recorded; total loss, model.link_loss and every parameter gradient."""
    model, params, g, adj, x, Cc = _model_case(n, num_pooling)
    label = torch.tensor([n % Cc])
    ypred = model(x.cuda(), g)
    loss = model.loss(ypred, label.cuda(), g)
    loss.backward()
    win = gpu_winners(model, num_pooling + 1)

    nn_ = [n]
    yo, _ = O.softpool_forward(params, x[None], adj[None], nn_, x[None], num_pooling=num_pooling)
    close(ypred, yo)
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yw, interw = O.softpool_forward(P, x[None], adj[None], nn_, x[None], num_pooling=num_pooling, winners=win)
    lo, link = O.softpool_loss(yw, label, interw["assign_0"], adj[None], nn_, True)
    lo.backward()
    close(ypred, yw)
    close(loss, lo, 1e-4, 1e-6)
    close(model.link_loss, link, 1e-4, 1e-6)
    assert model.link_loss.shape == () and float(model.link_loss) > 0
    grads_close(model, {k: v.grad for k, v in P.items()}, rtol=2e-3, atol_rel=1e-4)


@pytest.mark.parametrize("num_pooling", [1, 2])
def test_dense_linkpred_model_transfers_to_the_csr_class(num_pooling):
    """A dense SoftPoolingGcnEncoder(linkpred=True) and the CSR class holding its state_dict, on a graph of exactly
    max_num_nodes = 100 nodes: same loss, link loss and parameter gradients within the parity tolerances.  Both paths
    must route the max readouts to the same rows for the gradients to be comparable, which the test checks first."""
    N, F_, H, Cc = 100, 7, 16, 4
    src, dst = _edges(N, 3, 21)
    adj = torch.zeros(N, N)
    adj[src, dst] = 1.0
    adj = torch.maximum(adj, adj.t())
    x = torch.randn(N, F_, generator=torch.Generator().manual_seed(4))
    label = torch.tensor([2])
    dense = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=0.25, num_pooling=num_pooling, linkpred=True)
    params = O.init_params({k: tuple(v.shape) for k, v in dense.state_dict().items()}, seed=17, bias_scale=0.1)
    dense.load_state_dict(params)
    dense = dense.cuda()
    yd = dense(x[None].cuda(), adj[None].cuda(), np.array([N]))
    ld = dense.loss(yd, label.cuda(), adj[None].cuda(), np.array([N]))
    ld.backward()

    sparse = SparseSoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=0.25, num_pooling=num_pooling,
                                         linkpred=True)
    sparse.load_state_dict(dense.state_dict())
    sparse = sparse.cuda()
    g = CsrGraph.from_dense(adj.cuda())
    ys = sparse(x.cuda(), g)
    ls = sparse.loss(ys, label.cuda(), g)
    ls.backward()
    close(ys, yd)
    close(ls, ld, 1e-4, 1e-6)
    close(sparse.link_loss, dense.link_loss, 1e-4, 1e-6)
    for a, b in zip(gpu_winners(sparse, num_pooling + 1), gpu_winners(dense, num_pooling + 1)):
        assert torch.equal(a, b), "the two paths picked different max-readout rows: gradients are not comparable"
    grads_close(sparse, {k: p.grad.detach().cpu() for k, p in dense.named_parameters()}, rtol=2e-3, atol_rel=1e-4)


def test_training_with_the_link_loss_is_bit_reproducible_and_descends():
    """Three steps of plain SGD on a 5748-node graph (DD's largest), twice from the same parameters."""
    n = 5748
    model, params, g, _, x, Cc = _model_case(n, 1)
    xd, label = x.cuda(), torch.tensor([1], device="cuda")

    def train():
        model.load_state_dict(params)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = model.loss(model(xd, g), label, g)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, {k: p.detach().clone() for k, p in model.named_parameters()}

    l1, p1 = train()
    l2, p2 = train()
    print("losses:", l1)
    assert l1 == l2
    for k in p1:
        assert torch.isfinite(p1[k]).all(), k
        assert torch.equal(p1[k], p2[k]), k
    assert l1[0] > l1[1] > l1[2], l1
