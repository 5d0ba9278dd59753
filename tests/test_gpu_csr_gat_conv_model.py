"""`ops.csr_gat_conv` under torch.autograd and `GatConv` in front of the three sparse encoders.

The op and the module (heads 1 and 4, concat and mean) against plain-torch fp64 autograd of the dense formulas (a
-inf-masked softmax of leaky_relu(u_i + v_j) per head multiplied into the head's features) on a directed graph, an
undirected graph and a ragged batch: y and dz, du, dv for the op; the output, lin.weight.grad, a_src.grad, a_dst.grad,
bias.grad and x.grad for the module.  Every comparison uses the project's tolerance max(8 e_ref, 16 * 2^-24 * max|ref|)
per tensor (tests/test_gpu_csr_edge_ops_model.py).  Two stacked layers in front of SparseSoftPoolingGcnEncoder (link loss
on), the base GCN encoder and SparseGcnSet2SetEncoder on a CsrGraph, its directed view and a CsrBatch: the encoder's own
numbers are bit for bit those of feeding it the same h as data.  Ten Adam steps on the two layers with the encoder
frozen reproduce bit for bit with a loss that fell."""
import pytest
import torch

from graph_pooling_amd import GatConv, ops
from tests.test_gpu_csr_edge_ops import _container
from tests.test_gpu_csr_edge_ops_model import _both, _encoder, _grads, _stored, _tol_check

pytestmark = pytest.mark.gpu

TRAIN_SEED, TRAIN_LR = 6, 0.02


def dense_gat_conv(z, u, v, rows, cols, n, heads, slope, concat):
    mask = torch.zeros(n, n, dtype=torch.bool).index_put((rows, cols), torch.tensor(True))
    s = torch.nn.functional.leaky_relu(u[:, None, :] + v[None, :, :], slope)           # [n, n, H]
    a = torch.softmax(s.masked_fill(~mask[:, :, None], float("-inf")), dim=1)
    a = torch.where(mask.any(1)[:, None, None], a, torch.zeros_like(a))                # a row without entries: zeros
    y = torch.einsum("ijh,jhc->ihc", a, z.view(n, heads, -1))
    return y.reshape(n, -1) if concat else y.mean(1)


def dense_layer(x, w, a_src, a_dst, bias, rows, cols, n, heads, slope, concat):
    """`GatConv.forward` restated on the dense formulas."""
    z = x @ w.T
    zh = z.view(n, heads, -1)
    return dense_gat_conv(z, (zh * a_src).sum(-1), (zh * a_dst).sum(-1), rows, cols, n, heads, slope, concat) + bias


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("name", ["t4-n577", "undirected", "batch"])
def test_csr_gat_conv_against_fp64_autograd(name, heads, concat):
    c = _container(name)
    rows, cols = _stored(c)
    gen = torch.Generator().manual_seed(31)
    width = heads * 5
    z = torch.randn(c.n, width, generator=gen).cuda().requires_grad_(True)
    u, v = (torch.randn(c.n, heads, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    w = torch.randn(c.n, width if concat else 5, generator=gen)
    out = ops.csr_gat_conv(z, u, v, c, heads, 0.2, concat)
    assert out.shape == w.shape and out.dtype == torch.float32
    out.backward(w.cuda())
    fn = lambda zz, a, b: dense_gat_conv(zz, a, b, rows, cols, c.n, heads, 0.2, concat)
    (o64, g64), (o32, g32) = _both(fn, [z, u, v], w)
    tag = f"{name} H={heads} {'concat' if concat else 'mean'}"
    _tol_check(f"csr_gat_conv {tag}", out, o64, o32)
    for k, (leaf, what) in enumerate(((z, "dz"), (u, "du"), (v, "dv"))):
        _tol_check(f"csr_gat_conv {what} {tag}", leaf.grad, g64[k], g32[k])
    with torch.no_grad():                                            # nothing kept, the same bits
        plain = ops.csr_gat_conv(z, u, v, c, heads, 0.2, concat)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, out)


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("name", ["t4-n577", "batch"])
def test_gat_conv_module_against_fp64_autograd(name, heads, concat):
    c = _container(name)
    rows, cols = _stored(c)
    gen = torch.Generator().manual_seed(32)
    torch.manual_seed(3)
    layer = GatConv(7, 6, heads=heads, concat=concat).cuda()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=gen))
    x = torch.randn(c.n, 7, generator=gen).cuda().requires_grad_(True)
    out = layer(x, c)
    assert out.shape == (c.n, heads * 6 if concat else 6)
    w = torch.randn(out.shape, generator=gen)
    out.backward(w.cuda())
    fn = lambda xx, lw, s, d, b: dense_layer(xx, lw, s, d, b, rows, cols, c.n, heads, layer.negative_slope, concat)
    leaves = [x, layer.lin.weight, layer.a_src, layer.a_dst, layer.bias]
    (o64, g64), (o32, g32) = _both(fn, leaves, w)
    tag = f"{name} H={heads} {'concat' if concat else 'mean'}"
    _tol_check(f"GatConv {tag}", out, o64, o32)
    for k, what in enumerate(("x.grad", "lin.weight.grad", "a_src.grad", "a_dst.grad", "bias.grad")):
        _tol_check(f"GatConv {what} {tag}", leaves[k].grad, g64[k], g32[k])


STACKS = [(kind, name, directed) for kind in ("diffpool", "base", "s2s")
          for name, directed in (("graph64", False), ("graph64", True), ("batch", False))]


def _layers(x, seed):
    torch.manual_seed(seed)
    f = x.shape[1]
    return GatConv(f, 8, heads=4).cuda(), GatConv(32, f, heads=2, concat=False).cuda()


@pytest.mark.parametrize("kind,name,directed", STACKS, ids=[f"{k}-{n}{'-directed' if d else ''}" for k, n, d in STACKS])
def test_two_stacked_layers_in_front_of_the_encoder(kind, name, directed):
    model, c, x, loss_of = _encoder(kind, name)
    c = c.directed() if directed else c
    gat1, gat2 = _layers(x, 5)
    h = gat2(torch.nn.functional.elu(gat1(x, c)), c)
    assert h.shape == x.shape
    h.retain_grad()
    ypred = model(h, c)
    loss_of(ypred, c).backward()
    ga = _grads(model)
    for p in list(gat1.parameters()) + list(gat2.parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    # the encoder keeps its bits: the same h as data
    model.zero_grad(set_to_none=True)
    hd = h.detach().clone().requires_grad_(True)
    yd = model(hd, c)
    loss_of(yd, c).backward()
    assert torch.equal(yd, ypred) and torch.equal(hd.grad, h.grad)
    for k_, g in _grads(model).items():
        assert torch.equal(g, ga[k_]), f"gradient of {k_} differs between the layers' h and the same h as data"


def _train(seed=TRAIN_SEED, lr=TRAIN_LR):
    model, c, x, loss_of = _encoder("diffpool", "graph64")
    for p in model.parameters():
        p.requires_grad_(False)
    gat1, gat2 = _layers(x, seed)
    params = list(gat1.parameters()) + list(gat2.parameters())
    start = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        h = gat2(torch.nn.functional.elu(gat1(x, c)), c)
        loss = loss_of(model(h, c), c)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in params)
        opt.step()
        losses.append(loss.detach().clone())
    return torch.stack(losses).cpu(), start, [p.detach().cpu() for p in params]


def test_ten_adam_steps_on_two_layers_reproduce_and_the_loss_falls():
    """The encoder is frozen; the two runs agree bit for bit, every parameter moved and the loss fell (seed and rate
    chosen on the GPU; DESIGN §4.9 records the losses)."""
    l1, start, end1 = _train()
    l2, _, end2 = _train()
    print("two GatConv layers: loss per step", [f"{float(t):.6f}" for t in l1])
    assert torch.isfinite(l1).all()
    for a, b, s in zip(end1, end2, start):
        assert torch.equal(a, b) and not torch.equal(a, s.cpu())
    assert torch.equal(l1, l2)
    assert float(l1[-1]) < float(l1[0])
