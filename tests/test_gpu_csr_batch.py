"""Ragged batches of CSR graphs (CsrBatch): the new ops against float64 torch on the CPU — dp_bn_ragged_* with the padded
rows' constant and its gradient, dp_segment_max_*, dp_csr_pool_batch_* against the per-graph dp_csr_pool_* — and
SparseSoftPoolingGcnEncoder on a CsrBatch against the oracle's dense restatement on the same graphs PADDED to max n_b,
against the dense HIP module at pad_to = max_num_nodes, and against the single-graph call.

Tolerances are the project's (tests/parity.py): outputs rtol 1e-4 / atol 1e-5; parameter gradients
grads_close(rtol=2e-3, atol_rel=1e-4) as tests/test_gpu_sparse_pool.py uses for this path; pooled sums with the absolute
floor taken relative to the largest reference entry (`_close_scaled`, restated from that file)."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseSoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests.parity import close, grads_close, gpu_winners

pytestmark = pytest.mark.gpu


def _close_scaled(got, ref, scale=1.0):
    """parity.close (rtol 1e-4, atol 1e-5) with the absolute floor relative to the largest reference entry."""
    close(got, ref, 1e-4 * scale, 1e-5 * scale * max(1.0, float(ref.abs().max())))


def _edge_lists(sizes, seed, deg=3):
    """Per graph a random edge list (node 0 isolated when n > 2; a 1-node graph has no edge at all)."""
    rng = np.random.default_rng(seed)
    srcs, dsts = [], []
    for n in sizes:
        if n < 3:
            srcs.append(np.zeros(0, dtype=np.int64))
            dsts.append(np.zeros(0, dtype=np.int64))
            continue
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
    """ragged [n_total, F] -> [B, N, F] with zero rows behind each graph."""
    out = torch.zeros(len(sizes), N, x.shape[1], dtype=x.dtype)
    o = 0
    for b, n in enumerate(sizes):
        out[b, :n] = x[o:o + n]
        o += n
    return out


def _unpad(x, sizes):
    return torch.cat([x[b, :n] for b, n in enumerate(sizes)], dim=0)


class _Sizes:
    """What the ragged row ops need of a CsrBatch, for op tests without edges."""

    def __init__(self, sizes, pad_to=None):
        self.b = CsrBatch.from_edge_lists(sizes, [[]] * len(sizes), [[]] * len(sizes), "cuda", pad_to=pad_to)


# ------------------------------------------------------------------ ragged BatchNorm
BN_SIZES = {"equal": [17] * 5, "giant": [2000] + [30] * 12, "one_node": [1, 40, 7, 1], "single": [50],
            "two": [300, 41]}


@pytest.mark.parametrize("F_", [1, 20, 64, 512])
@pytest.mark.parametrize("name", list(BN_SIZES))
def test_ragged_bn_matches_padded_float64(name, F_):
    """dp_bn_ragged_fwd / bwd with a non-zero pad against the float64 dense statement: the batch padded to max n_b with
    every padded row holding `pad`, ReLU, statistics per node index over (batch, feature).  dx of the real rows and
    dpad = the sum of the padded rows' gradients.

    y and dpad are held to parity.close (rtol 1e-4 / atol 1e-5) as it stands; measured, dpad's worst case is 0.20 of
    that bound (giant, F = 1: |err| 5.5e-3 on an entry of 282).  dx keeps the same rtol / atol with the absolute floor
    taken relative to the largest reference entry (`_close_scaled`, no extra factor): dx = rstd (dy - mean(dy) - xhat
    mean(dy xhat)) scales with rstd, which reaches hundreds at F = 1 (a node index whose few values nearly coincide),
    so entries of a few hundred sit next to entries where the three terms cancel, and an entry's fp32 rounding is set
    by the terms, not by the entry — the reasoning grads_close applies to parameter gradients.  Measured against
    plain parity.close, dx reaches 1.34 of the bound in one case (two, F = 1: |err| 3.9e-4 beside entries of 101) and
    stays below 0.52 in every other; at F >= 20 it is below 0.04.  Each case prints its measured errors before asserting."""
    sizes = BN_SIZES[name]
    batch = _Sizes(sizes).b
    N, B = max(sizes), len(sizes)
    gen = torch.Generator().manual_seed(len(sizes) * 1000 + F_)
    x = torch.randn(sum(sizes), F_, generator=gen)
    pad = torch.rand(F_, generator=gen) * 0.5                    # post-ReLU constant: non-negative
    dy = torch.randn(sum(sizes), F_, generator=gen)

    x64 = x.double().requires_grad_(True)
    p64 = pad.double().requires_grad_(True)
    mask = O.node_mask(N, sizes, torch.float64)
    h = torch.relu(_pad_rows(x64, sizes, N)) * mask + p64 * (1 - mask)
    y64 = O.bn_node(h)
    (y64 * _pad_rows(dy.double(), sizes, N)).sum().backward()

    xd = x.cuda().requires_grad_(True)
    pd = pad.cuda().requires_grad_(True)
    y = ops.bn_relu_ragged(xd, pd, batch)
    y.backward(dy.cuda())
    close(y, _unpad(y64.detach(), sizes))
    for what, got, ref in (("dx", xd.grad, x64.grad), ("dpad", pd.grad, p64.grad)):
        err = (got.detach().cpu().double() - ref).abs()
        print(f"ragged bn {name} F={F_} {what}: max |err| {float(err.max()):.3e}, largest reference entry "
              f"{float(ref.abs().max()):.3e}, max err / (1e-5 + 1e-4 |ref|) {float((err / (1e-5 + 1e-4 * ref.abs())).max()):.3f}")
    _close_scaled(xd.grad, x64.grad)
    close(pd.grad, p64.grad)
    # bit-reproducible
    xd2 = x.cuda().requires_grad_(True)
    pd2 = pad.cuda().requires_grad_(True)
    y2 = ops.bn_relu_ragged(xd2, pd2, batch)
    y2.backward(dy.cuda())
    assert torch.equal(y, y2) and torch.equal(xd.grad, xd2.grad) and torch.equal(pd.grad, pd2.grad)


def test_ragged_bn_without_pad_is_the_zero_constant():
    sizes = [9, 4, 6]
    batch = _Sizes(sizes).b
    x = torch.randn(sum(sizes), 12, generator=torch.Generator().manual_seed(3))
    y = ops.bn_relu_ragged(x.cuda(), None, batch)
    yz = ops.bn_relu_ragged(x.cuda(), torch.zeros(12, device="cuda"), batch)
    assert torch.equal(y, yz)
    y64 = O.bn_node(torch.relu(_pad_rows(x.double(), sizes, 9)))
    close(y, _unpad(y64, sizes))


def test_ragged_bn_without_relu_through_the_c_entries():
    """relu = 0 (plain apply_bn) is reachable only through the C ABI: forward and backward (x may then be NULL: the
    backward needs it for the ReLU gate alone) against the float64 dense statement."""
    lib = _lib.load()
    sizes, F_ = [33, 7, 1, 20], 24
    batch = _Sizes(sizes).b
    N, B = max(sizes), len(sizes)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(sum(sizes), F_, generator=gen)
    pad = torch.randn(F_, generator=gen)
    dy = torch.randn(sum(sizes), F_, generator=gen)
    x64, p64 = x.double().requires_grad_(True), pad.double().requires_grad_(True)
    mask = O.node_mask(N, sizes, torch.float64)
    y64 = O.bn_node(_pad_rows(x64, sizes, N) * mask + p64 * (1 - mask))
    (y64 * _pad_rows(dy.double(), sizes, N)).sum().backward()
    xd, pd, dyd = x.cuda(), pad.cuda(), dy.cuda()
    y, stats = torch.empty_like(xd), torch.empty(N, 2, device="cuda")
    dx, dpad = torch.empty_like(xd), torch.empty_like(pd)
    st = _lib.current_stream()
    _lib.check(lib.dp_bn_ragged_fwd(xd.data_ptr(), F_, y.data_ptr(), F_, stats.data_ptr(), batch.node_off.data_ptr(),
                                    batch.order.data_ptr(), batch.cnt.data_ptr(), pd.data_ptr(), B, N, F_, 0, st),
               "dp_bn_ragged_fwd")
    wsb = lib.dp_bn_ragged_workspace_bytes(N, F_)
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    _lib.check(lib.dp_bn_ragged_bwd(None, F_, y.data_ptr(), F_, stats.data_ptr(), dyd.data_ptr(), F_, dx.data_ptr(), F_,
                                    dpad.data_ptr(), batch.node_off.data_ptr(), batch.order.data_ptr(),
                                    batch.cnt.data_ptr(), pd.data_ptr(), B, N, F_, 0, ws.data_ptr(), wsb, st),
               "dp_bn_ragged_bwd")
    close(y, _unpad(y64.detach(), sizes))
    _close_scaled(dx, x64.grad)
    close(dpad, p64.grad)


def test_launch_entries_refuse_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    assert lib.dp_bn_ragged_fwd(None, 4, None, 4, None, None, None, None, None, 1, 1, 4, 1, None) == -1
    assert b"NULL" in lib.dp_last_error_string()
    assert lib.dp_gcn_pad_const_fwd(p, p, 4, _lib.F_ADD_SELF, None) == -3
    assert b"DP_F_ADD_SELF" in lib.dp_last_error_string()
    assert lib.dp_bn_ragged_fwd(p, 4, p, 4, p, p, p, p, None, 0, 1, 4, 1, None) == -1          # B = 0
    assert lib.dp_bn_ragged_fwd(p, 2, p, 4, p, p, p, p, None, 1, 1, 4, 1, None) == -1          # ldx < F
    assert lib.dp_bn_ragged_fwd(p, 4096, p, 4096, p, p, p, p, None, 1, 1, 2049, 1, None) == -3  # F above the limit
    assert lib.dp_bn_ragged_bwd(p, 4, p, 4, p, p, 4, p, 4, p, p, p, p, None, 1, 1, 4, 1, p, 1024, None) == -1
    assert b"dpad asked for but pad is NULL" in lib.dp_last_error_string()
    assert lib.dp_segment_max_fwd(p, 4, p, p, p, 1, None, p, 4, p, 2, 4, p, 1024, None) == -1  # fewer chunks than graphs


@pytest.mark.parametrize("scale", [0.0, 0.5, 1e-20])
def test_pad_constant_and_its_bias_gradient(scale):
    """pad = relu(F.normalize(bias)) and dbias through the ReLU gate and the l2norm Jacobian, against torch float64
    autograd — also at a zero bias (every gate closed: dbias = 0) and below F.normalize's eps."""
    gen = torch.Generator().manual_seed(7)
    bias = (torch.rand(20, generator=gen) * 2 - 1) * scale
    dpad = torch.randn(20, generator=gen)
    b64 = bias.double().requires_grad_(True)
    p64 = torch.relu(torch.nn.functional.normalize(b64, p=2, dim=0, eps=1e-12))
    p64.backward(dpad.double())
    bd = bias.cuda().requires_grad_(True)
    p = ops.gcn_pad_const(bd, _lib.F_NORMALIZE)
    p.backward(dpad.cuda())
    close(p, p64.detach())
    _close_scaled(bd.grad, b64.grad)


# ------------------------------------------------------------------ segmented max
@pytest.mark.parametrize("floor", [False, True])
def test_segment_max_with_floor_and_ties(floor):
    """Against a per-graph torch max on the CPU.  Values are small integers, so every column has ties (lowest row
    wins) and, with the floor on, columns whose maximum is negative (the zero wins: arg-max -1) or exactly 0 (the real
    row keeps its index)."""
    sizes = [300, 1, 41, 700, 5]
    F_ = 70
    pad_to = 701 if floor else 700                   # 700: the largest graph has no padded row, so no floor for it
    batch = _Sizes(sizes, pad_to=pad_to).b
    gen = torch.Generator().manual_seed(11)
    z = torch.randint(-3, 3, (sum(sizes), F_), generator=gen).float()
    z[:, :10] -= 4.0                                    # all negative
    z[:, 10:20] = torch.minimum(z[:, 10:20], torch.zeros(()))      # maximum exactly 0 in most graphs
    dout = torch.randn(len(sizes), F_, generator=gen)
    zd = z.cuda().requires_grad_(True)
    out, arg = ops.segment_max(zd, batch)
    out.backward(dout.cuda())
    o, dz = 0, torch.zeros_like(z)
    for b, n in enumerate(sizes):
        v, i = z[o:o + n].max(dim=0)
        i = torch.tensor([int((z[o:o + n, f] == v[f]).nonzero()[0]) for f in range(F_)])       # lowest row on ties
        if n < pad_to:
            lose = v < 0
            v = torch.where(lose, torch.zeros(()), v)
            i = torch.where(lose, torch.full_like(i, -1), i)
        assert torch.equal(out[b].cpu(), v), b
        assert torch.equal(arg[b].cpu().long(), i), b
        for f in range(F_):
            if i[f] >= 0:
                dz[o + int(i[f]), f] += dout[b, f]
        o += n
    assert torch.equal(zd.grad.cpu(), dz)
    assert (arg[:3, :10].cpu() == -1).all() and (arg[0, 10:20].cpu() >= 0).all()      # 300 rows: a 0 is among them
    assert bool((arg[3, :10].cpu() == -1).all()) == floor


# ------------------------------------------------------------------ batched pooling
@pytest.mark.parametrize("K,D,directed", [(50, 60, False), (7, 33, True), (256, 512, False), (64, 96, True)])
def test_batched_csr_pool_equals_the_per_graph_calls_bit_for_bit(K, D, directed):
    """SAME ARITHMETIC: every graph keeps the slab partition and the row blocks of a single-graph call and its partials
    are summed in the same tree, so X', A', dS and dZ of the batch equal the per-graph dp_csr_pool_* results bit for
    bit (torch.equal, no tolerance)."""
    sizes = [300, 41, 1, 1200, 300, 2000, 64, 65]
    srcs, dsts = _edge_lists(sizes, 5)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda", symmetric=not directed)
    gen = torch.Generator().manual_seed(K + D)
    S = torch.rand(sum(sizes), K, generator=gen).cuda().requires_grad_(True)
    Z = (torch.rand(sum(sizes), D, generator=gen) - 0.5).cuda().requires_grad_(True)
    dXp = torch.randn(len(sizes), K, D, generator=gen).cuda()
    dAp = torch.randn(len(sizes), K, K, generator=gen).cuda()
    xp, ap = ops.csr_pool_batch(S, Z, batch)
    torch.autograd.backward([xp, ap], [dXp, dAp])
    o = 0
    for b, n in enumerate(sizes):
        src, dst = (srcs[b], dsts[b]) if n > 1 else (np.array([0]), np.array([0]))
        g = CsrGraph.from_edges(n, src, dst, "cuda", symmetric=not directed)
        if n == 1:                                       # the single-graph CSR cannot be empty: compare without the loop
            o += n
            continue
        s1 = S.detach()[o:o + n].clone().requires_grad_(True)
        z1 = Z.detach()[o:o + n].clone().requires_grad_(True)
        x1, a1 = ops.csr_pool(s1, z1, g)
        torch.autograd.backward([x1, a1], [dXp[b], dAp[b]])
        assert torch.equal(xp[b], x1) and torch.equal(ap[b], a1), b
        assert torch.equal(S.grad[o:o + n], s1.grad) and torch.equal(Z.grad[o:o + n], z1.grad), b
        o += n
    # the 1-node graph (no edge): X' = S^T Z, A' = 0
    o1 = sizes[0] + sizes[1]
    _close_scaled(xp[2], S.detach()[o1:o1 + 1].double().cpu().t() @ Z.detach()[o1:o1 + 1].double().cpu())
    assert float(ap[2].detach().abs().max()) == 0.0


# ------------------------------------------------------------------ the model
F_IN, HID, EMB, NCLS = 9, 20, 20, 3
MIXED = [300, 41, 1, 1200, 300, 2000]


def _model_case(sizes, num_pooling, linkpred, bias_scale=0.3, seed=0, pad_to=None, max_nodes=500):
    srcs, dsts = _edge_lists(sizes, 100 + seed)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda", pad_to=pad_to)
    N = max(sizes)
    adj = _dense_adj(sizes, srcs, dsts, N)
    x = torch.randn(sum(sizes), F_IN, generator=torch.Generator().manual_seed(seed + 1))
    model = SparseSoftPoolingGcnEncoder(max_nodes, F_IN, HID, EMB, NCLS, 3, HID, assign_ratio=0.1,
                                        num_pooling=num_pooling, pred_hidden_dims=[50], linkpred=linkpred)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed + num_pooling,
                           bias_scale=bias_scale)
    model.load_state_dict(params)
    label = torch.tensor([b % NCLS for b in range(len(sizes))])
    return model.cuda(), params, batch, adj, x, label


def _run(model, x, batch, label):
    model.zero_grad(set_to_none=True)
    ypred = model(x.cuda(), batch)
    loss = model.loss(ypred, label.cuda(), batch)
    loss.backward()
    return ypred, loss


@pytest.mark.parametrize("linkpred", [False, True])
@pytest.mark.parametrize("num_pooling", [1, 2])
@pytest.mark.parametrize("sizes", [MIXED, [150] * 4], ids=["mixed", "equal"])
def test_batch_equals_dense_oracle_on_the_padded_batch(sizes, num_pooling, linkpred):
    """ypred, pooled activations, loss, link loss and every parameter gradient against the oracle on the same graphs
    padded to max n_b (GraphConv biases of scale 0.3, so the padded rows' constants are not zero).  The oracle's
    backward runs with the winners the HIP forward recorded, as tests/test_gpu_sparse_pool.py does."""
    model, params, batch, adj, x, label = _model_case(sizes, num_pooling, linkpred)
    ypred, loss = _run(model, x, batch, label)
    win = gpu_winners(model, num_pooling + 1)
    N = max(sizes)
    xp = _pad_rows(x, sizes, N)
    yo, inter = O.softpool_forward(params, xp, adj, sizes, xp, num_pooling=num_pooling, want_intermediates=True)
    close(ypred, yo)
    assert ypred.shape == (len(sizes), NCLS)
    close(model.saved_activation(0, "assign"), _unpad(inter["assign_0"], sizes))
    for j in range(num_pooling):
        _close_scaled(model.saved_activation(j, "xpool"), inter[f"xpool_{j}"])
        _close_scaled(model.saved_activation(j, "adjpool"), inter[f"adjpool_{j}"])
        if j:
            close(model.saved_activation(j, "assign"), inter[f"assign_{j}"])
    assert model.assign_tensor.shape == (sum(sizes), model.assign_dims[0])
    assert model.saved_activation(0, "readout_argmax").shape == (len(sizes), model.pred_input_dim)

    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yw, interw = O.softpool_forward(P, xp, adj, sizes, xp, num_pooling=num_pooling, winners=win)
    lo, link = O.softpool_loss(yw, label, interw["assign_0"], adj, sizes, linkpred)
    lo.backward()
    close(ypred, yw)
    close(loss, lo, 1e-4, 1e-6)
    if linkpred:
        close(model.link_loss, link, 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in P.items()}, rtol=2e-3, atol_rel=1e-4)
    assert torch.equal(model.predict(x.cuda(), batch).cpu(), yo.argmax(dim=1))


def test_batch_with_a_5748_node_graph_forward():
    """DD's largest graph next to a small one (B = 2): forward only against the dense oracle at N = 5748."""
    sizes = [5748, 100]
    model, params, batch, adj, x, label = _model_case(sizes, 1, False, seed=3)
    with torch.no_grad():
        ypred = model(x.cuda(), batch)
    xp = _pad_rows(x, sizes, 5748)
    yo, inter = O.softpool_forward(params, xp, adj, sizes, xp, num_pooling=1, want_intermediates=True)
    close(ypred, yo)
    _close_scaled(model.saved_activation(0, "xpool"), inter["xpool_0"])
    _close_scaled(model.saved_activation(0, "adjpool"), inter["adjpool_0"])


@pytest.mark.parametrize("num_pooling", [1, 2])
def test_batch_equals_the_dense_hip_module_at_max_num_nodes(num_pooling):
    """SoftPoolingGcnEncoder on the batch padded to max_num_nodes = 100 > max n_b and the CSR class with its state_dict
    on CsrBatch.from_dense(..., pad_to=100): the zero floor then applies to every graph."""
    N, sizes = 100, [60, 33, 1, 80]
    srcs, dsts = _edge_lists(sizes, 21)
    adj = _dense_adj(sizes, srcs, dsts, N)
    x = torch.randn(sum(sizes), 7, generator=torch.Generator().manual_seed(4))
    dense = SoftPoolingGcnEncoder(N, 7, 16, 16, 4, 3, 16, assign_ratio=0.25, num_pooling=num_pooling, linkpred=False)
    sd = O.init_params({k: tuple(v.shape) for k, v in dense.state_dict().items()}, seed=9, bias_scale=0.5)
    dense.load_state_dict(sd)
    dense = dense.cuda()
    with torch.no_grad():
        yd = dense(_pad_rows(x, sizes, N).cuda(), adj.cuda(), np.array(sizes))
    sparse = SparseSoftPoolingGcnEncoder(N, 7, 16, 16, 4, 3, 16, assign_ratio=0.25, num_pooling=num_pooling,
                                         linkpred=False)
    sparse.load_state_dict(dense.state_dict())
    sparse = sparse.cuda()
    batch = CsrBatch.from_dense(adj.cuda(), sizes, pad_to=N)
    assert batch.floor_flag.cpu().tolist() == [1, 1, 1, 1]
    with torch.no_grad():
        ys = sparse(x.cuda(), batch)
    close(ys, yd)
    _close_scaled(sparse.saved_activation(0, "xpool"), dense.saved_activation(0, "xpool").cpu())


def test_padded_rows_reach_the_bias_gradients():
    """Term 3: GraphConv biases of scale 0.5 and a batch where most node indices have padded rows.  The gradients of
    conv_first.bias, conv_block.0.bias and the level-0 assign_conv biases hold under grads_close(2e-3, 1e-4) against
    the oracle on the padded batch, where autograd carries the padded rows' share."""
    sizes = [40, 8, 5, 3, 12, 6]
    model, params, batch, adj, x, label = _model_case(sizes, 2, True, bias_scale=0.5, seed=5, max_nodes=100)
    ypred, loss = _run(model, x, batch, label)
    win = gpu_winners(model, 3)
    xp = _pad_rows(x, sizes, 40)
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yw, interw = O.softpool_forward(P, xp, adj, sizes, xp, num_pooling=2, winners=win)
    lo, _ = O.softpool_loss(yw, label, interw["assign_0"], adj, sizes, True)
    lo.backward()
    keys = ["conv_first.bias", "conv_block.0.bias", "assign_conv_first_0.bias", "assign_conv_block_0.0.bias"]
    named = dict(model.named_parameters())
    for k in keys:
        ref = P[k].grad
        close(named[k].grad, ref, rtol=2e-3, atol=max(1e-7, 1e-4 * float(ref.abs().max())))
    grads_close(model, {k: v.grad for k, v in P.items()}, rtol=2e-3, atol_rel=1e-4)


def test_one_graph_batch_equals_the_single_graph_call():
    n = 300
    srcs, dsts = _edge_lists([n], 8)
    g = CsrGraph.from_edges(n, srcs[0], dsts[0], "cuda", symmetric=True)
    batch = CsrBatch.from_graphs([g])
    assert batch.num_graphs == 1 and not batch.has_padding and batch.floor_flag.cpu().tolist() == [0]
    model, params, _, _, x, label = _model_case([n], 2, True, seed=8)
    label = label[:1]
    y1 = model(x.cuda(), g)
    l1 = model.loss(y1, label.cuda(), g)
    model.zero_grad(set_to_none=True)
    l1.backward()
    g1 = {k: p.grad.clone() for k, p in model.named_parameters()}
    yb, lb = _run(model, x, batch, label)
    close(yb, y1)
    close(lb, l1, 1e-4, 1e-6)
    grads_close(model, g1, rtol=2e-3, atol_rel=1e-4)


def test_single_graph_run_keeps_nothing_of_a_batch_run_between():
    """One forward body serves both containers: a single-graph run after a batch run on the same model is bit for bit
    the single-graph run before it — ypred, loss, link loss, every parameter gradient, every saved activation."""
    sizes, num_pooling = [300, 41, 1], 2
    srcs, dsts = _edge_lists(sizes, 12)
    g = CsrGraph.from_edges(sizes[0], srcs[0], dsts[0], "cuda", symmetric=True)
    model, params, batch, _, x, label = _model_case(sizes, num_pooling, True, seed=12)
    x1, l1 = x[:sizes[0]].cuda(), label[:1].cuda()

    def single():
        model.zero_grad(set_to_none=True)
        ypred = model(x1, g)
        loss = model.loss(ypred, l1, g)
        loss.backward()
        out = {"ypred": ypred, "loss": loss, "link_loss": model.link_loss, "assign_tensor": model.assign_tensor}
        out.update({"grad " + k: p.grad for k, p in model.named_parameters()})
        for what in ("assign", "xpool", "adjpool", "embedding", "readout_argmax"):
            for j in range(num_pooling + (what in ("embedding", "readout_argmax"))):
                out[f"{what} {j}"] = model.saved_activation(j, what)
        return {k: v.detach().clone() for k, v in out.items()}

    first = single()
    _run(model, x, batch, label)
    assert model.assign_tensor.shape == (sum(sizes), model.assign_dims[0])
    third = single()
    assert first["assign_tensor"].shape == (1, sizes[0], model.assign_dims[0])
    assert first["embedding 0"].shape == (1, sizes[0], model.pred_input_dim)
    assert first["xpool 1"].shape == (1, model.assign_dims[1], model.pred_input_dim)
    assert first["readout_argmax 2"].shape == (1, model.pred_input_dim)
    assert list(third) == list(first)
    for k, v in first.items():
        assert third[k].shape == v.shape and torch.equal(third[k], v), k


def test_batch_is_bit_reproducible():
    model, params, batch, adj, x, label = _model_case([300, 41, 1, 700, 300], 2, True, seed=2)
    runs = []
    for _ in range(2):
        ypred, loss = _run(model, x, batch, label)
        runs.append((ypred.detach().clone(), loss.detach().clone(),
                     {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def _kernel_launches(sizes, linkpred):
    model, params, batch, adj, x, label = _model_case(sizes, 2, linkpred, seed=1)
    _run(model, x, batch, label)                     # warm up: plans, lazy module loads
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        _run(model, x, batch, label)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def test_launch_count_does_not_grow_with_the_batch():
    """Forward + loss + backward of a linkpred=False model launches the same number of kernels at B = 2 and B = 8.
    The link loss is built from per-graph launches (dp_csr_linkpred_batch_*), so a linkpred=True model adds launches
    in proportion to B: up to 5 per graph (2 forward, 3 backward)."""
    small, big = [200, 90], [200, 90, 150, 30, 170, 200, 64, 120]
    n2, n8 = _kernel_launches(small, False), _kernel_launches(big, False)
    assert n2 == n8 and n2 > 0, (n2, n8)
    l2, l8 = _kernel_launches(small, True), _kernel_launches(big, True)
    assert l2 > n2 and 0 < l8 - l2 <= 5 * 6, (n2, l2, l8)


def test_training_loop_on_ragged_batches_lowers_the_loss():
    from graph_pooling_amd.optim import FusedClipAdam
    model, params, batch, adj, x, label = _model_case([120, 41, 1, 300, 77, 200], 1, True, seed=6)
    opt = FusedClipAdam(model, lr=1e-2, clip=2.0)
    xd, ld = x.cuda(), label.cuda()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model.loss(model(xd, batch), ld, batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k


def test_batch_argument_errors_on_the_device():
    model, params, batch, adj, x, label = _model_case([30, 12], 1, True, seed=4)
    with pytest.raises(ValueError, match="n_total"):
        model(x.cuda()[:-1], batch)
    ypred = model(x.cuda(), batch)
    with pytest.raises(ValueError, match="one class per graph"):
        model.loss(ypred, torch.zeros(3, dtype=torch.long, device="cuda"), batch)
    other = CsrBatch.from_edge_lists([30, 12], [[1], [1]], [[2], [2]], "cuda")
    with pytest.raises(ValueError, match="not the batch the last forward ran on"):
        model.loss(ypred, label.cuda(), other)
    with pytest.raises(NotImplementedError, match="needs the CsrBatch"):
        model.loss(ypred, label.cuda())
