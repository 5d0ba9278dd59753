"""The learned-edge-weight ops under torch.autograd and `EdgeAttention` in front of the three sparse encoders.

`ops.csr_sddmm`, `ops.csr_edge_softmax` and `ops.csr_sym_normalize` against plain-torch fp64 autograd of the dense
formulas (index_put, a -inf-masked softmax, A.sum(0)) on a directed graph, an undirected graph and a ragged batch.
`EdgeAttention` in front of SparseSoftPoolingGcnEncoder (link loss on), SparseBatchGcnEncoderGraph and
SparseGcnSet2SetEncoder: the upstream gradient is the one the existing ops return for the values (`a.retain_grad()`;
tests/test_gpu_csr_edge_grad_model.py pins it), and q.weight.grad / k.weight.grad are compared with fp64 autograd of the
edge pipeline alone under that gradient.  Every comparison uses the project's tolerance max(8 e_ref, 16 * 2^-24 *
max|ref|) per tensor, e_ref the error of an fp32 plain-torch evaluation of the same formula against fp64.  The encoder
behind the attention keeps its bits (the same values fed as data give the same ypred and parameter gradients, and a run
without attention is the same before and after), and ten Adam steps on the attention parameters reproduce bit for bit."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import EdgeAttention, SparseGcnSet2SetEncoder, ops
from tests import csr_edge_ops_cases as OC
from tests import test_gpu_csr_weights_model as WM
from tests.test_gpu_csr_edge_ops import _container
from tests.test_gpu_set2set_ragged_model import _init

pytestmark = pytest.mark.gpu

ATT = 8


def _tol_check(what, got, ref64, ref32):
    """The project's bound per tensor: max(8 e_ref, 16 * 2^-24 * max|ref|)."""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().double(), ref32.detach().double()
    e_ref = float((ref32 - ref64).abs().max())
    scale = float(ref64.abs().max())
    bound = max(8 * e_ref, 16 * OC.U * scale)
    err = float((got - ref64).abs().max())
    print(f"{what}: error {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e} max|ref| {scale:.3e}")
    assert got.shape == ref64.shape and scale > 0 and err <= bound, f"{what}: error {err:.3e} > bound {bound:.3e}"


def _stored(c):
    ip = c.indptr.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return torch.from_numpy(rows), c.indices.cpu().long()[:ip[-1]]


# ------------------------------------------------------------------ the dense formulas, in plain torch
def dense_sddmm(p, q, rows, cols, alpha):
    return alpha * (p @ q.T)[rows, cols]


def dense_softmax(s, rows, cols, n):
    a = torch.full((n, n), float("-inf"), dtype=s.dtype).index_put((rows, cols), s)
    return torch.softmax(a, dim=1)[rows, cols]


def dense_sym(v, rows, cols, n):
    a = torch.zeros(n, n, dtype=v.dtype).index_put((rows, cols), v)
    r = a.sum(0).pow(-0.5)
    return (r[:, None] * a * r[None, :])[rows, cols]


def _both(fn, leaves, upstream):
    """fn(*leaves) and the leaves' gradients under `upstream`, in fp64 and in fp32 on the CPU."""
    res = []
    for dt in (torch.float64, torch.float32):
        ls = [t.detach().cpu().to(dt).requires_grad_(True) for t in leaves]
        out = fn(*ls)
        out.backward(upstream.detach().cpu().to(dt))
        res.append((out.detach(), [t.grad for t in ls]))
    return res


GRAPHS = ["t4-n577", "undirected", "batch"]


@pytest.mark.parametrize("name", GRAPHS)
def test_csr_sddmm_and_its_gradients_against_fp64_autograd(name):
    c = _container(name)
    rows, cols = _stored(c)
    gen = torch.Generator().manual_seed(11)
    p, q = (torch.randn(c.n, ATT, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    w = torch.randn(c.nnz, generator=gen)
    out = ops.csr_sddmm(p, q, c, 0.375)
    out.backward(w.cuda())
    (o64, g64), (o32, g32) = _both(lambda a, b: dense_sddmm(a, b, rows, cols, 0.375), [p, q], w)
    _tol_check(f"csr_sddmm {name}", out, o64, o32)
    _tol_check(f"csr_sddmm dP {name}", p.grad, g64[0], g32[0])
    _tol_check(f"csr_sddmm dQ {name}", q.grad, g64[1], g32[1])
    # P = Q (the 'sym' form): both gradients land on the one leaf
    z = torch.randn(c.n, ATT, generator=gen).cuda().requires_grad_(True)
    ops.csr_sddmm(z, z, c).backward(w.cuda())
    (_, g64), (_, g32) = _both(lambda a: dense_sddmm(a, a, rows, cols, 1.0), [z], w)
    _tol_check(f"csr_sddmm dP + dQ {name}", z.grad, g64[0], g32[0])


@pytest.mark.parametrize("name", GRAPHS)
def test_csr_edge_softmax_against_fp64_autograd(name):
    c = _container(name)
    rows, cols = _stored(c)
    gen = torch.Generator().manual_seed(12)
    s = (3 * torch.randn(c.nnz, generator=gen)).cuda().requires_grad_(True)
    w = torch.randn(c.nnz, generator=gen)
    out = ops.csr_edge_softmax(s, c)
    out.backward(w.cuda())
    (o64, g64), (o32, g32) = _both(lambda t: dense_softmax(t, rows, cols, c.n), [s], w)
    _tol_check(f"csr_edge_softmax {name}", out, o64, o32)
    _tol_check(f"csr_edge_softmax dscores {name}", s.grad, g64[0], g32[0])


@pytest.mark.parametrize("name", GRAPHS)
def test_csr_sym_normalize_against_fp64_autograd(name):
    c = _container(name)
    rows, cols = _stored(c)
    gen = torch.Generator().manual_seed(13)
    v = c.values.detach().clone().requires_grad_(True)
    w = torch.randn(c.nnz, generator=gen)
    out = ops.csr_sym_normalize(v, c)
    out.backward(w.cuda())
    (o64, g64), (o32, g32) = _both(lambda t: dense_sym(t, rows, cols, c.n), [v], w)
    _tol_check(f"csr_sym_normalize {name}", out, o64, o32)
    _tol_check(f"csr_sym_normalize dvalues {name}", v.grad, g64[0], g32[0])
    plain = ops.csr_sym_normalize(None, _container(name, weighted=False))          # a 0/1 container: data
    (o64, _), (o32, _) = _both(lambda t: dense_sym(t, rows, cols, c.n), [torch.ones(c.nnz)], w)
    assert not plain.requires_grad
    _tol_check(f"csr_sym_normalize 0/1 {name}", plain, o64, o32)


# ------------------------------------------------------------------ EdgeAttention in front of the encoders
def _pipeline(norm, x, wq, wk, base, rows, cols, n):
    """`EdgeAttention.forward` restated on the dense formulas."""
    qx = x @ wq.T
    if norm == "softmax":
        return dense_softmax(dense_sddmm(qx, x @ wk.T, rows, cols, ATT ** -0.5), rows, cols, n)
    gate = torch.sigmoid(dense_sddmm(qx, qx, rows, cols, ATT ** -0.5)) * base
    return dense_sym(gate, rows, cols, n)


def _encoder(kind, name):
    """(model, container, x, loss(ypred, container))."""
    if kind == "diffpool":
        model, _, _, c, sizes, _, _, x, label = WM._diffpool(name, True, 0.0)
        ld = label.cuda()
        return model, c, x.cuda(), lambda y, g: model.loss(y, ld, g)
    if kind == "base":
        model, _, c, sizes, _, _, x, label = WM._base(name)
        ld = label.cuda()
        return model, c, x.cuda(), lambda y, g: torch.nn.functional.cross_entropy(y, ld)
    c, sizes, _, _ = WM._container(name, 2)
    x, label = WM._inputs(sizes, 2, 7)
    model = SparseGcnSet2SetEncoder(7, 10, 10, WM.NCLS, 3, pred_hidden_dims=[20], bn=True)
    _init(model, 2)
    model = model.cuda()
    ld = label.cuda()
    return model, c, x.cuda(), lambda y, g: model.loss(y, ld)


def _grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters()}


ENCODERS = [("diffpool", "graph64", "softmax"), ("diffpool", "batch", "sym"), ("diffpool", "batch", "softmax"),
            ("base", "batch", "softmax"), ("base", "graph64", "sym"), ("s2s", "graph64", "softmax"),
            ("s2s", "batch", "sym")]


@pytest.mark.parametrize("kind,name,norm", ENCODERS, ids=["-".join(e) for e in ENCODERS])
def test_edge_attention_trains_through_the_encoder(kind, name, norm):
    model, c, x, loss_of = _encoder(kind, name)
    # today's run, without attention
    y0 = model(x, c)
    loss_of(y0, c).backward()
    g0 = _grads(model)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    att = EdgeAttention(x.shape[1], ATT, norm=norm).cuda()
    h = att(x, c)
    a = h.values
    a.retain_grad()
    assert type(h) is type(c) and (h.indices_t is not h.indices) == (norm == "softmax")
    ypred = model(x, h)
    loss_of(ypred, h).backward()
    assert a.grad is not None and torch.isfinite(a.grad).all() and float(a.grad.abs().max()) > 0
    ga = _grads(model)
    # the edge pipeline alone, under the gradient the encoder returned for the values
    rows, cols = _stored(c)
    wk = att.k.weight if norm == "softmax" else att.q.weight
    base = c.values.detach()[:c.nnz]
    fn = lambda xx, wq, wk_, b: _pipeline(norm, xx, wq, wk_, b, rows, cols, c.n)
    (o64, g64), (o32, g32) = _both(fn, [x, att.q.weight, wk, base], a.grad[:c.nnz])
    tag = f"{kind}-{name}-{norm}"
    _tol_check(f"attention values {tag}", a[:c.nnz], o64, o32)
    _tol_check(f"q.weight.grad {tag}", att.q.weight.grad, g64[1], g32[1])      # 'sym': the one projection, both sides
    if norm == "softmax":
        _tol_check(f"k.weight.grad {tag}", att.k.weight.grad, g64[2], g32[2])
    # the encoder keeps its bits: the same values as data ...
    model.zero_grad(set_to_none=True)
    hd = h.with_values(a.detach())
    yd = model(x, hd)
    loss_of(yd, hd).backward()
    assert torch.equal(yd, ypred)
    for k_, g in _grads(model).items():
        assert torch.equal(g, ga[k_]), f"gradient of {k_} differs between learned values and the same values as data"
    # ... and with the attention removed, today's run again
    model.zero_grad(set_to_none=True)
    y1 = model(x, c)
    loss_of(y1, c).backward()
    assert torch.equal(y1, y0)
    for k_, g in _grads(model).items():
        assert torch.equal(g, g0[k_]), f"gradient of {k_} changed after an attention run"


def _train(norm):
    model, c, x, loss_of = _encoder("diffpool", "graph64")
    for p in model.parameters():
        p.requires_grad_(False)
    torch.manual_seed(6)
    att = EdgeAttention(x.shape[1], ATT, norm=norm).cuda()
    start = {k: p.detach().clone() for k, p in att.named_parameters()}
    opt = torch.optim.Adam(att.parameters(), lr=0.05)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        h = att(x, c)
        loss = loss_of(model(x, h), h)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return torch.stack(losses).cpu(), start, {k: p.detach().cpu() for k, p in att.named_parameters()}


@pytest.mark.parametrize("norm", ["softmax", "sym"])
def test_ten_adam_steps_on_the_attention_parameters_reproduce(norm):
    """The encoder is frozen (as in the edge-mask run of tests/test_gpu_csr_edge_grad_model.py); whether the loss fell is
    reported, not required."""
    l1, start, end1 = _train(norm)
    l2, _, end2 = _train(norm)
    print(f"{norm}: loss per step", [f"{float(t):.6f}" for t in l1], "fell" if float(l1[-1]) < float(l1[0]) else "did not fall")
    assert torch.isfinite(l1).all()
    for k in end1:
        assert not torch.equal(end1[k], start[k].cpu()), f"{k} did not move"
        assert torch.equal(end1[k], end2[k]), f"{k} differs between the two runs"
    assert torch.equal(l1, l2)
