"""`ops.csr_topk_pool` under torch.autograd, `TopKPooling`, and the pooled containers in front of everything that takes one.

Every test reads a freshly pooled container back and asserts its structure (indptr monotone from 0 to nnz', columns
ascending, unique and inside their graph's new range, local = global - offset) and its equality with the numpy
restatement BEFORE any other kernel reads through it.  The op on a CsrGraph (undirected weighted, directed) and on
CsrBatches against the restatement and fp64 autograd; `TopKPooling` with both scores, the kept sets restated from the
score the module computed; the pooled container against `from_edge_lists` of the restated edge lists under GraphConv,
GatConv, SageConv, EdgeAttention, pool, link_loss, with_values, directed, normalized and sym_normalized, and with
ratio = 1 under the three sparse encoders, bit for bit; the stack GraphConv -> TopKPooling -> GatConv -> TopKPooling ->
SparseBatchGcnEncoderGraph -> loss against fp64 plain-torch autograd of the dense restatement on the same kept sets, at
the project's tolerance max(8 e_ref, 16 * 2^-24 * max|ref|); a `with_values` tensor's gradient through the pooling;
three FusedClipAdam steps twice, bit for bit; and the launch counts (5 undirected, 8 directed, 1 backward)."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import EdgeAttention, GatConv, SageConv, TopKPooling, ops
from graph_pooling_amd.encoders import GraphConv
from graph_pooling_amd.optim import FusedClipAdam
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseBatchGcnEncoderGraph
from oracle import diffpool_oracle as O
from tests import csr_topk_cases as TC
from tests.test_gpu_csr_edge_ops_model import _both, _encoder, _grads, _tol_check
from tests.test_gpu_csr_gat_conv_model import dense_layer
from tests.test_gpu_csr_sample_model import _launches
from tests.test_gpu_csr_topk import check_structure

pytestmark = pytest.mark.gpu

_CONT = {}


def container(gname):
    """The case graph as a container on the device: a CsrBatch for the batches, else a CsrGraph."""
    if gname not in _CONT:
        g = TC.graph(gname)
        if gname in TC.BATCHES:
            lists = g.edge_lists()
            c = CsrBatch.from_edge_lists(g.sizes, [s for s, _, _ in lists], [d for _, d, _ in lists], "cuda",
                                         symmetric=not g.directed, pad_to=g.pad_to,
                                         weights=[w for _, _, w in lists] if g.weighted else None)
        else:
            c = CsrGraph.from_edges(g.n, g.rows, g.indices, "cuda", symmetric=not g.directed, weight=g.values)
        assert (c.indices_t is c.indices) == (not g.directed) and c.weighted == g.weighted
        assert np.array_equal(c.indptr.cpu().numpy(), g.indptr) and np.array_equal(c.indices.cpu().numpy()[:g.nnz], g.indices)
        if g.weighted:
            assert np.array_equal(c.values.cpu().numpy()[:g.nnz], g.values)
        _CONT[gname] = c
    return _CONT[gname]


def validated(out, p, em=None, em_t=None):
    """Read the pooled container back, assert its invariants and its equality with the restatement `p`; only a container
    that passed may go to another kernel."""
    batch = isinstance(out, CsrBatch)
    assert "nnz" in out.__dict__ and out.nnz == p.nnz and out.n == p.n_out
    sets = [(out.indptr, out.indices, getattr(out, "indices_local", None), p.indptr, p.indices, p.local, em, p.edge_map)]
    undirected = out.indices_t is out.indices
    assert undirected == (not p.g.directed) and (out.indptr_t is out.indptr) == undirected
    if not undirected:
        sets.append((out.indptr_t, out.indices_t, getattr(out, "indices_t_local", None), p.indptr_t, p.indices_t, p.local_t,
                     em_t, p.edge_map_t))
    for ip, ix, il, rip, rix, ril, m, rm in sets:
        ip, ix = ip.cpu().numpy(), ix.cpu().numpy()
        il = None if il is None else il.cpu().numpy()
        assert ip.dtype == np.int32 and ix.dtype == np.int32
        assert ix.size == (max(p.nnz, 1) if batch else p.nnz), "the index arrays are narrowed to nnz' (one pad when 0)"
        check_structure(ip, ix, il, p.new_off, p.nnz)
        assert np.array_equal(ip, rip) and np.array_equal(ix[:p.nnz], rix)
        if il is not None:
            assert np.array_equal(il[:p.nnz], ril)
        if p.nnz == 0 and batch:
            assert ix[0] == 0 and il[0] == 0
        if m is not None:
            assert np.array_equal(m.cpu().numpy(), rm)
    if batch:
        assert np.array_equal(out.node_off_host, p.new_off) and np.array_equal(out.node_off.cpu().numpy(), p.new_off)
        assert np.array_equal(out.num_nodes, p.kb)
    if p.g.weighted:
        assert np.array_equal(out.values.detach().cpu().numpy()[:p.nnz], p.g.values[p.edge_map])
        assert np.array_equal(out.values_t.detach().cpu().numpy()[:p.nnz], p.g.values_t[p.edge_map_t])
        assert (out.values_t is out.values) == undirected
    return out


def restated_container(p, gname, ratio):
    """The pooled graph built by the host route from the restatement's edge lists."""
    g = p.g
    r = np.repeat(np.arange(p.n_out), np.diff(p.indptr))
    if gname not in TC.BATCHES:
        return CsrGraph.from_edges(p.n_out, r, p.indices, "cuda", symmetric=not g.directed,
                                   weight=g.values[p.edge_map] if g.weighted else None)
    lists = p.edge_lists()
    gb = np.searchsorted(p.new_off, r, side="right") - 1
    ws = [g.values[p.edge_map][gb == b] for b in range(g.B)] if g.weighted else None
    pad_to = None if g.pad_to is None else int(ops.topk_counts([g.pad_to], ratio=ratio)[0])
    return CsrBatch.from_edge_lists(p.kb, [s for s, _ in lists], [d for _, d in lists], "cuda", symmetric=not g.directed,
                                    pad_to=pad_to, weights=ws)


def pooled_pair(gname, kind, ratio):
    """(x_out, validated pooled container, host-route container, restatement) of a case graph at `ratio`."""
    c, p = container(gname), TC.pooled(gname, kind, ("ratio", ratio))
    s = torch.from_numpy(TC.scores(gname, kind)).cuda()
    x = torch.from_numpy(TC.inputs((gname, kind, ("ratio", ratio), 7, "tight", False))[0]).cuda()
    x_out, out, perm, new_id, thr, em, em_t = ops.csr_topk_pool_stats(x, s, c, ratio=ratio)
    assert np.array_equal(perm.cpu().numpy(), p.perm) and np.array_equal(new_id.cpu().numpy(), p.new_id)
    assert np.array_equal(thr.cpu().numpy().view(np.uint64), p.thr)
    return x_out, validated(out, p, em, em_t), restated_container(p, gname, ratio), p


OP_CASES = [("g256", "ties", ("ratio", 0.5)), ("g257", "special", ("ratio", 0.3)), ("g4097", "ties", ("k", 3000)),
            ("mixed", "zeros", ("ratio", 0.5)), ("edgeless", "ties", ("k", 3)), ("padded", "normal", ("ratio", 0.25)),
            ("bigmix", "equal", ("ratio", 0.3)), ("bipart", "parity", ("ratio", 0.5)),
            ("bipart_batch", "parity", ("ratio", 0.5)), ("padded", "ties", ("ratio", 1.0))]


@pytest.mark.parametrize("gname,kind,sel", OP_CASES, ids=[f"{g}-{k}-{s[0]}{s[1]:g}" for g, k, s in OP_CASES])
def test_csr_topk_pool_against_the_restatement_and_fp64_autograd(gname, kind, sel):
    c, g = container(gname), TC.graph(gname)
    p = TC.Pooled(g, TC.scores(gname, kind), TC.sel_counts(g, sel))
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(g.n, 9, generator=gen).cuda().requires_grad_(True)
    s = torch.from_numpy(TC.scores(gname, kind)).cuda()
    raw = torch.randn(g.n, generator=gen).cuda().requires_grad_(True)          # the gate's own leaf
    gate = torch.tanh(raw)
    x_out, out, perm, new_id, thr, em, em_t = ops.csr_topk_pool_stats(x, s, c, gate=gate, **{sel[0]: sel[1]})
    assert np.array_equal(perm.cpu().numpy(), p.perm) and perm.dtype == torch.int32
    assert np.array_equal(new_id.cpu().numpy(), p.new_id) and np.array_equal(thr.cpu().numpy().view(np.uint64), p.thr)
    validated(out, p, em, em_t)
    if isinstance(c, CsrBatch):
        want_pad = int(ops.topk_counts([c.pad_to], **{sel[0]: sel[1]})[0])
        assert out.pad_to == want_pad >= out.max_n and out.num_graphs == c.num_graphs
    pl = torch.from_numpy(p.perm).long()
    assert torch.equal(x_out.detach().cpu(), x.detach().cpu()[pl] * gate.detach().cpu()[pl][:, None])      # one multiply
    w = torch.randn(x_out.shape, generator=gen)
    x_out.backward(w.cuda())
    (o64, g64), (o32, g32) = _both(lambda xx, rr: xx[pl] * torch.tanh(rr)[pl][:, None], [x, raw], w)
    tag = f"{gname} {kind} {sel}"
    _tol_check(f"csr_topk_pool x_out {tag}", x_out, o64, o32)
    _tol_check(f"csr_topk_pool x.grad {tag}", x.grad, g64[0], g32[0])
    _tol_check(f"csr_topk_pool gate leaf grad {tag}", raw.grad, g64[1], g32[1])
    dropped = torch.from_numpy(~p.kept)
    assert not x.grad.cpu()[dropped].any() and not raw.grad.cpu()[dropped].any()
    plain, out2, perm2 = ops.csr_topk_pool(x.detach(), s, c, **{sel[0]: sel[1]})                         # no gate: a copy
    assert plain.grad_fn is None and torch.equal(plain, x.detach()[perm.long()]) and torch.equal(perm2, perm)
    assert torch.equal(out2.indptr, out.indptr) and torch.equal(out2.indices, out.indices)
    if (p.kb == g.sizes).all():                                       # ratio = 1: the input graph, value for value
        assert torch.equal(out.indptr, c.indptr) and torch.equal(out.indices, c.indices) and out.nnz == c.nnz
        assert torch.equal(out.values, c.values) and torch.equal(out.indices_local, c.indices_local)


@pytest.mark.parametrize("score", ["proj", "gcn"])
@pytest.mark.parametrize("gname", ["g256", "g257", "padded", "edgeless"])
def test_topk_pooling_module_keeps_the_restated_set_and_trains(gname, score):
    c, g = container(gname), TC.graph(gname)
    gen = torch.Generator().manual_seed(52)
    torch.manual_seed(8)
    layer = TopKPooling(7, ratio=0.4, score=score).cuda()
    x = torch.randn(g.n, 7, generator=gen).cuda().requires_grad_(True)
    s = layer.scores(x, c).detach()
    p = TC.Pooled(g, s.cpu().numpy(), TC.counts(g.sizes, ratio=0.4))              # restated from the module's own score
    x_out, out, perm = layer(x, c)
    assert np.array_equal(perm.cpu().numpy(), p.perm)
    validated(out, p)
    w = torch.randn(x_out.shape, generator=gen)
    x_out.backward(w.cuda())
    pl = torch.from_numpy(p.perm).long()
    rows, cols = torch.from_numpy(g.rows), torch.from_numpy(g.indices)
    vals = None if g.values is None else torch.from_numpy(g.values)

    def fn(xx, *ps):
        if score == "proj":
            sc = xx @ (ps[0] / ps[0].norm())
        else:
            a = torch.zeros(g.n, g.n, dtype=xx.dtype).index_put((rows, cols), torch.ones(rows.numel(), dtype=xx.dtype)
                                                                  if vals is None else vals.to(xx.dtype))
            sc = ((a @ xx + xx) @ ps[0] + ps[1]).view(-1)
        return xx[pl] * torch.tanh(sc)[pl][:, None]
    leaves = [x] + list(layer.parameters())
    (o64, g64), (o32, g32) = _both(fn, leaves, w)
    tag = f"{gname} {score}"
    _tol_check(f"TopKPooling x_out {tag}", x_out, o64, o32)
    for k, what in enumerate(["x.grad"] + [n + ".grad" for n, _ in layer.named_parameters()]):
        _tol_check(f"TopKPooling {what} {tag}", leaves[k].grad, g64[k], g32[k])


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: the pooled container and the host-route container differ"


@pytest.mark.parametrize("gname,kind", [("padded", "normal"), ("edgeless", "ties"), ("g256", "ties"), ("g257", "normal")])
def test_a_pooled_container_is_accepted_like_one_built_on_the_host(gname, kind):
    x_out, out, ref, p = pooled_pair(gname, kind, 0.5)
    assert type(out) is type(ref) and out.nnz == ref.nnz == p.nnz
    batch = isinstance(out, CsrBatch)
    torch.manual_seed(12)
    conv = GraphConv(7, 5, normalize_embedding=True).cuda()
    torch.nn.init.xavier_uniform_(conv.weight)
    gat, sage, att = GatConv(7, 4, heads=2).cuda(), SageConv(7, 6, num_sample=3).cuda(), EdgeAttention(7, 8).cuda()
    for name, f in (("csr_graph_conv", lambda c: ops.csr_graph_conv(x_out, conv.weight, conv.bias, c, conv._flags())),
                    ("GatConv", lambda c: gat(x_out, c)), ("SageConv", lambda c: sage(x_out, c, seed=5)),
                    ("EdgeAttention", lambda c: att(x_out, c).values),
                    ("with_values", lambda c: ops.csr_graph_conv(
                        x_out, conv.weight, conv.bias,
                        c.with_values(torch.full((c.nnz,), 0.5, device="cuda")), conv._flags())),
                    ("directed", lambda c: ops.csr_graph_conv(x_out, conv.weight, conv.bias, c.directed(), conv._flags())),
                    ("sym_normalized", lambda c: c.sym_normalized().values)):
        _same(f(out).detach(), f(ref).detach(), name)
    s = torch.softmax(torch.randn(out.n, 4, generator=torch.Generator().manual_seed(3)).cuda(), 1)
    _same(out.link_loss(s), ref.link_loss(s), "link_loss")
    _same(out.link_loss(s, "frobenius"), ref.link_loss(s, "frobenius"), "frobenius link_loss")
    for a, b in zip(out.pool(s, x_out), ref.pool(s, x_out)):
        _same(a, b, "pool")
    if batch:
        h5 = ops.csr_graph_conv(x_out, conv.weight, conv.bias, ref, conv._flags()).detach()      # the layer's own width
        _same(out.bn_relu(h5, conv), ref.bn_relu(h5, conv), "bn_relu")
        for a, b in zip(out.readout(x_out), ref.readout(x_out)):
            _same(a, b, "readout")
    try:
        nv = out.normalized().values
    except ValueError:                                                # a node of degree 0: both refuse
        with pytest.raises(ValueError, match="degree"):
            ref.normalized()
    else:
        _same(nv, ref.normalized().values, "normalized")
    assert torch.equal(out.mirror_perm, ref.mirror_perm) if not p.g.directed else torch.equal(out._t_perm, ref._t_perm)


ENC = [(kind, name) for kind in ("diffpool", "base", "s2s") for name in ("graph64", "batch")]


@pytest.mark.parametrize("kind,name", ENC, ids=["-".join(e) for e in ENC])
def test_the_three_encoders_take_the_container_pooled_at_ratio_one(kind, name):
    """Everything kept: the pooled container holds the input's arrays value for value, so the encoder gives its bits."""
    model, c, x, loss_of = _encoder(kind, name)
    score = torch.randn(c.n, generator=torch.Generator().manual_seed(2)).cuda()
    x_out, out, perm = ops.csr_topk_pool(x, score, c, ratio=1.0)
    nnz = c.nnz
    assert torch.equal(perm.cpu(), torch.arange(c.n, dtype=torch.int32)) and torch.equal(x_out, x) and out.nnz == nnz
    ip, ix = out.indptr.cpu().numpy(), out.indices.cpu().numpy()
    off = out.node_off_host if isinstance(out, CsrBatch) else np.array([0, out.n])
    il = out.indices_local.cpu().numpy() if isinstance(out, CsrBatch) else None
    check_structure(ip, ix, il, off.astype(np.int64), nnz)
    assert torch.equal(out.indptr, c.indptr) and torch.equal(out.indices[:nnz], c.indices[:nnz])
    assert torch.equal(out.indptr_t, c.indptr_t) and torch.equal(out.indices_t[:nnz], c.indices_t[:nnz])
    y0 = model(x, c)
    loss_of(y0, c).backward()
    g0 = _grads(model)
    model.zero_grad(set_to_none=True)
    y1 = model(x_out, out)
    loss_of(y1, out).backward()
    assert torch.equal(y0, y1)
    for k, g in _grads(model).items():
        assert torch.equal(g, g0[k]), k


# ------------------------------------------------------------------ the stack against the dense restatement
def _stack_modules():
    torch.manual_seed(21)
    conv = GraphConv(6, 8, normalize_embedding=True)
    torch.nn.init.xavier_uniform_(conv.weight)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    pool1, gat, pool2 = TopKPooling(8, 0.6), GatConv(8, 4, heads=2), TopKPooling(8, 0.5, score="gcn")
    enc = SparseBatchGcnEncoderGraph(8, 8, 8, 3, 3, pred_hidden_dims=[10], bn=True)
    for m in enc.modules():
        if isinstance(m, GraphConv):
            torch.nn.init.xavier_uniform_(m.weight)
            with torch.no_grad():
                m.bias.uniform_(-0.1, 0.1)
    return torch.nn.ModuleList([conv, pool1, gat, pool2, enc]).cuda()


def _stack_forward(mods, x, c, label):
    """The stack on the device; every pooled container is validated against the restatement of the score the module
    computed before the next layer reads it -> (loss, the two restatements)."""
    conv, pool1, gat, pool2, enc = mods
    g = TC.graph("padded")
    h = torch.relu(ops.csr_graph_conv(x, conv.weight, conv.bias, c, conv._flags()))
    p1 = TC.Pooled(g, pool1.scores(h, c).detach().cpu().numpy(), TC.counts(g.sizes, ratio=0.6))
    h1, c1, perm1 = pool1(h, c)
    assert np.array_equal(perm1.cpu().numpy(), p1.perm)
    validated(c1, p1)
    h2 = torch.nn.functional.elu(gat(h1, c1))
    g1 = p1.as_graph(c1.pad_to)                                      # the pooled graph: the next restatement's input
    p2 = TC.Pooled(g1, pool2.scores(h2, c1).detach().cpu().numpy(), TC.counts(g1.sizes, ratio=0.5))
    h3, c2, perm2 = pool2(h2, c1)
    assert np.array_equal(perm2.cpu().numpy(), p2.perm)
    validated(c2, p2)
    loss = torch.nn.functional.cross_entropy(enc(h3, c2), label)
    return loss, p1, p2, g1, c2


def test_the_stack_against_fp64_autograd_of_the_dense_restatement():
    mods = _stack_modules()
    conv, pool1, gat, pool2, enc = mods
    c, g = container("padded"), TC.graph("padded")
    gen = torch.Generator().manual_seed(53)
    x = torch.randn(g.n, 6, generator=gen).cuda().requires_grad_(True)
    label = torch.tensor([0, 2, 1]).cuda()
    loss, p1, p2, g1, c2 = _stack_forward(mods, x, c, label)
    loss.backward()
    names = [n for n, _ in mods.named_parameters()]
    enc_keys = [n for n, _ in enc.named_parameters()]
    pl1, pl2 = torch.from_numpy(p1.perm).long(), torch.from_numpy(p2.perm).long()
    pad2, off2 = c2.pad_to, p2.new_off

    def dense(n, rows, cols, vals, dt):
        return torch.zeros(n, n, dtype=dt).index_put((torch.from_numpy(rows), torch.from_numpy(cols)),
                                                     torch.from_numpy(vals).to(dt))

    def fn(xx, *ps):
        P = dict(zip(names, ps))
        dt = xx.dtype
        a0 = dense(g.n, g.rows, g.indices, g.values, dt)
        h = torch.relu(O.graph_conv(xx[None], a0[None], P["0.weight"], P["0.bias"], False, True)[0])
        s1 = h @ (P["1.p"] / P["1.p"].norm())
        h1 = h[pl1] * torch.tanh(s1)[pl1][:, None]
        r1, c1_ = torch.from_numpy(g1.rows), torch.from_numpy(g1.indices)
        h2 = torch.nn.functional.elu(dense_layer(h1, P["2.lin.weight"], P["2.a_src"], P["2.a_dst"], P["2.bias"], r1, c1_,
                                                 g1.n, 2, 0.2, True))
        a1 = dense(g1.n, g1.rows, g1.indices, g1.values, dt)
        s2 = ((a1 @ h2 + h2) @ P["3.weight"] + P["3.bias"]).view(-1)
        h3 = h2[pl2] * torch.tanh(s2)[pl2][:, None]
        a2 = a1[pl2][:, pl2]
        xd, ad = torch.zeros(g.B, pad2, 8, dtype=dt), torch.zeros(g.B, pad2, pad2, dtype=dt)
        for b in range(g.B):                                          # the dense batch padded to the pooled pad_to
            lo, hi = int(off2[b]), int(off2[b + 1])
            xd[b, :hi - lo] = h3[lo:hi]
            ad[b, :hi - lo, :hi - lo] = a2[lo:hi, lo:hi]
        ep = {k: P["4." + k] for k in enc_keys}
        y = O.base_forward(ep, xd, ad, num_layers=3, n_pred_hidden=1, bn=True, concat=True)
        return torch.nn.functional.cross_entropy(y, label.cpu()).reshape(1)

    leaves = [x] + [q for _, q in mods.named_parameters()]
    (o64, g64), (o32, g32) = _both(fn, leaves, torch.ones(1))
    _tol_check("stack loss", loss.reshape(1), o64, o32)
    for k, what in enumerate(["x"] + names):
        _tol_check(f"stack {what}.grad", leaves[k].grad, g64[k], g32[k])


def test_a_with_values_tensor_receives_its_gradient_through_the_pooling():
    gname = "edgeless"                                                # directed, weighted, one member without edges
    c, g = container(gname), TC.graph(gname)
    p = TC.pooled(gname, "ties", ("ratio", 0.5))
    gen = torch.Generator().manual_seed(54)
    v = torch.from_numpy(g.values).cuda().requires_grad_(True)
    cv = c.with_values(v)
    x = torch.randn(g.n, 5, generator=gen).cuda()
    s = torch.from_numpy(TC.scores(gname, "ties")).cuda()
    x_out, out, perm = ops.csr_topk_pool(x, s, cv, ratio=0.5)
    validated(out, p)
    assert out.values.requires_grad and not out.values_t.requires_grad
    torch.manual_seed(13)
    conv = GraphConv(5, 4, normalize_embedding=True).cuda()
    torch.nn.init.xavier_uniform_(conv.weight)
    y = ops.csr_graph_conv(x_out, conv.weight, conv.bias, out, conv._flags())
    w = torch.randn(y.shape, generator=gen)
    y.backward(w.cuda())
    pl = torch.from_numpy(p.perm).long()
    rows, cols = torch.from_numpy(g.rows), torch.from_numpy(g.indices)

    def fn(vv, ww, bb):
        a = torch.zeros(g.n, g.n, dtype=vv.dtype).index_put((rows, cols), vv)[pl][:, pl]
        return O.graph_conv(x.cpu().to(vv.dtype)[pl][None], a[None], ww, bb, False, True)[0]
    (o64, g64), (o32, g32) = _both(fn, [v, conv.weight, conv.bias], w)
    _tol_check("pooled GraphConv", y, o64, o32)
    _tol_check("values.grad through the pooling", v.grad, g64[0], g32[0])
    lost = np.ones(g.nnz, bool)
    lost[p.edge_map] = False
    assert not v.grad.cpu().numpy()[lost].any() and v.grad.cpu().numpy()[~lost].any()


def _train(steps=3):
    mods = _stack_modules()
    c, g = container("padded"), TC.graph("padded")
    x = torch.randn(g.n, 6, generator=torch.Generator().manual_seed(55)).cuda()
    label = torch.tensor([0, 2, 1]).cuda()
    start = [q.detach().clone() for q in mods.parameters()]
    opt = FusedClipAdam(mods, lr=0.01, clip=2.0)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = _stack_forward(mods, x, c, label)[0]
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return torch.stack(losses).cpu(), start, [q.detach().cpu().clone() for q in mods.parameters()]


def test_three_fused_adam_steps_reproduce_bit_for_bit():
    l1, start, end1 = _train()
    l2, _, end2 = _train()
    print("the stack: loss per step", [f"{float(t):.6f}" for t in l1])
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    for a, b, s in zip(end1, end2, start):
        assert torch.equal(a, b) and not torch.equal(a, s.cpu())


@pytest.mark.parametrize("gname,fwd", [("mixed", 5), ("bigmix", 8), ("g65", 5), ("g255", 8)])
def test_the_launch_counts_do_not_depend_on_the_batch(gname, fwd):
    c, g = container(gname), TC.graph(gname)
    assert not g.weighted and g.directed == (fwd == 8)
    p = TC.pooled(gname, "ties", ("ratio", 0.5))
    x = torch.randn(g.n, 65, device="cuda", requires_grad=True)
    s = torch.from_numpy(TC.scores(gname, "ties")).cuda()
    gate = torch.rand(g.n, device="cuda", requires_grad=True)
    kept = {}

    def run():
        kept["out"] = ops.csr_topk_pool(x, s, c, ratio=0.5, gate=gate)
    names = _launches(run)
    validated(kept["out"][1], p)
    mine = [n for n in names if "k_csr_topk_" in n]
    assert len(names) == len(mine) == fwd, names
    order = ["select"] + ["count", "scan", "fill"] * (2 if fwd == 8 else 1) + ["gather_fwd"]
    assert all("k_csr_topk_" + o in n for o, n in zip(order, mine)), mine
    dy = torch.randn(p.n_out, 65, device="cuda")
    names = _launches(lambda: torch.autograd.grad(kept["out"][0], [x, gate], dy, retain_graph=True))
    assert len(names) == 1 and "k_csr_topk_gather_bwd" in names[0], names
