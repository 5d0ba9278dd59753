"""`ops.csr_sample_block` / `ops.csr_block_mean` under torch.autograd, `SageConv.block` / `forward_block` and
`NestedSageEncoder` on top of them.

One layer: a one-layer `NestedSageEncoder` equals `SageEncoder` bit for bit, forward and parameter gradients.  Two
layers: the nested model against plain-torch fp64 autograd of the dense sample masks of both layers (the numpy
restatement, tests/csr_sample_cases.py) and against the whole-graph stack conv2(conv1(x, g, seed_0), g, nodes, seed_1),
both at the project's model bound max(8 e_ref, 16 * 2^-24 * max|ref|) with e_ref the fp32 run of the same reference (no
bit equality there: the first layer's GEMM has another M); the gradient of an `nn.Embedding` is exactly zero outside the
innermost src.  Three `FusedClipAdam` steps under `torch.manual_seed`, run twice, agree bit for bit; the launches per
block and per layer do not depend on m, n or B; a block costs one 4-byte read-back."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import NestedSageEncoder, SageConv, SageEncoder, ops
from graph_pooling_amd.graphsage import SupervisedGraphSage
from graph_pooling_amd.optim import FusedClipAdam
from graph_pooling_amd.sparse import CsrGraph
from tests import csr_block_cases as BC
from tests import csr_sample_cases as SC
from tests.test_gpu_csr_edge_ops_model import _both, _tol_check
from tests.test_gpu_csr_sample_model import _launches, container, dense_sage

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


@pytest.mark.parametrize("gname,tname,k", [("directed", "seven", 10), ("undirected", "lengths", 2), ("batch", "nested", 64),
                                           ("batch", "all", None), ("directed", "one", 1)])
def test_the_op_builds_the_restated_block_and_the_mean_has_the_bits_of_csr_sample_mean(gname, tname, k):
    kk = BC.ALL if k is None else k
    c, b = container(gname), BC.block(gname, tname, kk)
    t = BC.targets(gname, tname, kk)
    nodes = None if t is None else _dev(t)
    blk = ops.csr_sample_block(c, nodes, k, BC.SEED)
    assert blk.n_src == b.n_src and blk.k == kk and blk.seed == BC.SEED and blk.graph is c and blk.m == b.m
    assert np.array_equal(blk.src.cpu().numpy(), b.src) and np.array_equal(blk.slot.cpu().numpy(), b.slot)
    assert np.array_equal(blk.thr.cpu().numpy().view(np.uint64), b.thr) and np.array_equal(blk.cnt.cpu().numpy(), b.cnt)
    assert blk.src.dtype == blk.slot.dtype == blk.cnt.dtype == torch.int32 and blk.thr.dtype == torch.int64
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(c.n, 7, generator=gen).cuda().requires_grad_(True)
    for mode in SC.MODES:
        x_src = x.detach()[blk.src.long()].requires_grad_(True)
        y = ops.csr_block_mean(x_src, blk, mode)
        want = ops.csr_sample_mean(x, c, k, BC.SEED, nodes, mode)
        assert torch.equal(y, want), mode
        w = torch.randn(y.shape, generator=gen).cuda()
        y.backward(w)
        x.grad = None
        want.backward(w)
        assert x_src.grad.shape == (blk.n_src, 7) and torch.equal(x_src.grad, x.grad[blk.src.long()])
        rest = torch.ones(c.n, dtype=torch.bool, device="cuda")
        rest[blk.src.long()] = False
        assert not x.grad[rest].any()
        with torch.no_grad():
            assert ops.csr_block_mean(x_src, blk, mode).grad_fn is None


@pytest.mark.parametrize("gcn", [False, True], ids=["concat", "gcn"])
@pytest.mark.parametrize("gname", ["directed", "batch"])
def test_one_nested_layer_equals_the_sage_encoder_bit_for_bit(gname, gcn):
    c, g = container(gname), SC.graph(gname)
    nodes = BC.targets(gname, "lengths")
    torch.manual_seed(7)
    feats = torch.nn.Embedding(g.n, 9).cuda()
    conv = SageConv(9, 6, num_sample=10, gcn=gcn, bias=True).cuda()
    flat, nested = SageEncoder(feats, c, conv), NestedSageEncoder(feats, c, [conv])
    assert nested.embed_dim == flat.embed_dim == 6
    w = torch.randn(nodes.size, 6, generator=torch.Generator().manual_seed(52)).cuda()
    grads = []
    outs = []
    for enc in (flat, nested):
        for p in enc.parameters():
            p.grad = None
        out = enc(nodes, seed=SC.SEED)
        out.backward(w)
        outs.append(out.detach().clone())
        grads.append([p.grad.clone() for p in (conv.weight, conv.bias, feats.weight)])
    assert torch.equal(outs[0], outs[1])
    for a, b in zip(*grads):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    blk = nested.blocks(nodes, SC.SEED)[0]
    assert np.array_equal(blk.src.cpu().numpy(), BC.Block(g, SC.SEED, 10, nodes).src)
    with pytest.raises(ValueError, match="sampled with k = 10"):
        SageConv(9, 6, num_sample=5).cuda().forward_block(feats.weight[blk.src.long()], blk)


def _two_layer(gname, feats_module=False):
    c, g = container(gname), SC.graph(gname)
    nodes = BC.targets(gname, "seven")
    s0_seed, s1_seed = BC.layer_seed(SC.SEED, 0), BC.layer_seed(SC.SEED, 1)
    assert s0_seed == SC.SEED and s1_seed != SC.SEED
    torch.manual_seed(8)
    c1, c2 = SageConv(7, 8, num_sample=10).cuda(), SageConv(8, 5, num_sample=10, gcn=True).cuda()
    feats = torch.nn.Embedding(g.n, 7).cuda() if feats_module else torch.randn(g.n, 7).cuda().requires_grad_(True)
    return c, g, nodes, (s0_seed, s1_seed), c1, c2, feats


@pytest.mark.parametrize("gname", SC.GRAPHS)
def test_two_nested_layers_against_fp64_autograd_of_the_dense_masks_and_the_whole_graph_stack(gname):
    c, g, nodes, (seed0, seed1), c1, c2, x = _two_layer(gname)
    enc = NestedSageEncoder(x, c, [c1, c2])
    b0, b1 = enc.blocks(nodes, SC.SEED)
    r1 = BC.Block(g, seed1, 10, nodes)
    r0 = BC.Block(g, seed0, 10, r1.src)
    assert np.array_equal(b1.src.cpu().numpy(), r1.src) and np.array_equal(b0.src.cpu().numpy(), r0.src)
    assert b0.nodes is b1 and b0.n_src < g.n and b1.n_src < b0.n_src
    print(f"{gname}: m = {nodes.size}, n_src = {b1.n_src} (layer 1), {b0.n_src} (layer 0) of n = {g.n}")
    # the reference: the dense masks of both layers; layer 0 on EVERY node, its rows outside block 1's src are not read
    s0, s1 = SC.Sample(g, seed0, 10, "concat"), SC.Sample(g, seed1, 10, "gcn", nodes)
    w = torch.randn(nodes.size, 5, generator=torch.Generator().manual_seed(53))
    leaves = [x, c1.weight, c2.weight]

    def run(fn):
        for t in leaves:
            t.grad = None
        out = fn()
        out.backward(w.cuda())
        return out.detach().clone(), [t.grad.clone() for t in leaves]

    out_n, g_n = run(lambda: enc(nodes, seed=SC.SEED))
    out_w, g_w = run(lambda: c2(c1(x, c, seed=seed0), c, _dev(nodes), seed=seed1))
    (o64, g64), (o32, g32) = _both(lambda xx, w1, w2: dense_sage(dense_sage(xx, w1, s0), w2, s1), leaves, w)

    def held(what, a, b, ref64, ref32):
        """a against b at the model bound of the reference (ref64, its fp32 run ref32)."""
        e_ref = float((ref32.double() - ref64).abs().max())
        bound = max(8 * e_ref, 16 * 2.0 ** -24 * float(ref64.abs().max()))
        err = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())
        print(f"{what}: difference {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{what}: difference {err:.3e} > bound {bound:.3e}"

    _tol_check(f"nested two layers {gname}", out_n, o64, o32)
    _tol_check(f"whole-graph stack {gname}", out_w, o64, o32)
    held(f"nested against the whole-graph stack {gname}", out_n, out_w, o64, o32)
    for k, what in enumerate(("x.grad", "conv1.weight.grad", "conv2.weight.grad")):
        _tol_check(f"nested two layers {what} {gname}", g_n[k], g64[k], g32[k])
        _tol_check(f"whole-graph stack {what} {gname}", g_w[k], g64[k], g32[k])
        held(f"nested against the whole-graph stack {what} {gname}", g_n[k], g_w[k], g64[k], g32[k])
    rest = torch.ones(g.n, dtype=torch.bool)
    rest[torch.from_numpy(r0.src)] = False
    assert rest.any() and not g_n[0][rest.cuda()].any() and not g64[0][rest].any()


def test_the_gradient_of_an_embedding_is_exactly_zero_outside_the_innermost_src():
    c, g, nodes, _, c1, c2, emb = _two_layer("undirected", feats_module=True)
    seen = []

    def features(ids):                                                # a callable: called with the LongTensor of ids only
        seen.append(ids)
        return emb(ids)
    model = SupervisedGraphSage(3, NestedSageEncoder(features, c, [c1, c2])).cuda()
    torch.manual_seed(3)
    loss = model.loss(nodes, torch.arange(nodes.size).cuda() % 3)
    loss.backward()
    assert len(seen) == 1 and seen[0].dtype == torch.long and seen[0].numel() < g.n
    rest = torch.ones(g.n, dtype=torch.bool, device="cuda")
    rest[seen[0]] = False
    assert emb.weight.grad.shape == (g.n, 7) and not emb.weight.grad[rest].any()
    assert float(emb.weight.grad[seen[0]].abs().max()) > 0 and torch.isfinite(loss)
    model2 = SupervisedGraphSage(3, NestedSageEncoder(emb, c, [c1, c2])).cuda()      # the nn.Embedding itself
    assert sorted(n for n, _ in model2.named_parameters()) == ["enc.convs.0.weight", "enc.convs.1.weight",
                                                               "enc.features.weight", "weight"]


def _train(steps=3):
    gname = "undirected"
    c, g = container(gname), SC.graph(gname)
    nodes = BC.targets(gname, "lengths")
    torch.manual_seed(11)
    feats = torch.randn(g.n, 16).cuda()
    enc = NestedSageEncoder(feats, c, [SageConv(16, 12, num_sample=10), SageConv(12, 8, num_sample=5)])
    model = SupervisedGraphSage(4, enc).cuda()
    labels = torch.from_numpy((SC.row_len(g)[nodes] % 4)).cuda()
    start = [p.detach().clone() for p in model.parameters()]
    opt = FusedClipAdam(model, lr=0.01, clip=2.0)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = model.loss(nodes, labels)                             # the seed comes from torch's CPU generator
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return torch.stack(losses).cpu(), start, [p.detach().cpu().clone() for p in model.parameters()]


def test_three_fused_adam_steps_reproduce_bit_for_bit():
    l1, start, end1 = _train()
    l2, _, end2 = _train()
    print("SupervisedGraphSage(NestedSageEncoder): loss per step", [f"{float(t):.6f}" for t in l1])
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    for a, b, s in zip(end1, end2, start):
        assert torch.equal(a, b) and not torch.equal(a, s.cpu())


def _ring_container(n):
    g = BC.ring(n)
    rows = np.repeat(np.arange(n), 8)
    return CsrGraph.from_edges(n, rows, g.indices, "cuda", symmetric=True)


def test_launches_per_block_and_per_layer_do_not_depend_on_m_n_or_B():
    """A block is five launches, the compact mean one each way, whatever the targets, the graph and the batch; a block
    reads 4 bytes back."""
    counts = set()
    shapes = [(container("directed"), BC.targets("directed", "one")), (container("directed"), BC.targets("directed", "lengths")),
              (container("batch"), BC.targets("batch", "seven")), (_ring_container(BC.CHUNK * BC.SCAN + 1), BC.ring_targets(257))]
    for c, t in shapes:
        nodes = _dev(t)
        kept = {}

        def build():
            kept["b"] = ops.csr_sample_block(c, nodes, 2, 3, nodes_checked=True)
        names = _launches(build)
        own = [n for n in names if "k_csr_block_" in n]
        order = ("k_csr_block_zero", "k_csr_block_mark", "k_csr_block_count", "k_csr_block_scan", "k_csr_block_fill")
        assert len(names) == len(own) == 5 and all(o in n for o, n in zip(order, own)), names
        blk = kept["b"]
        inner = {}

        def nested():
            inner["b"] = ops.csr_sample_block(c, blk, 2, 4)
        assert len([n for n in _launches(nested) if "k_csr_block_" in n]) == 5
        x_src = torch.randn(blk.n_src, 65, device="cuda", requires_grad=True)
        dy = torch.randn(blk.m, 130, device="cuda")

        def fwd():
            kept["y"] = ops.csr_block_mean(x_src, blk, "concat")
        f = _launches(fwd)
        assert len(f) == 1 and "k_csr_block_mean_fwd" in f[0], f
        bwd = _launches(lambda: torch.autograd.grad(kept["y"], x_src, dy, retain_graph=True))
        own_b = [n for n in bwd if "k_csr_block_mean_bwd" in n]
        assert len(own_b) == 1, bwd                                  # beside it: the tslot scatter of tensor targets, in torch
        # the nested form scatters nothing: its backward is the one launch
        xi = torch.randn(inner["b"].n_src, 8, device="cuda", requires_grad=True)
        yi = ops.csr_block_mean(xi, inner["b"], "gcn")
        dyi = torch.ones_like(yi)
        bi = _launches(lambda: torch.autograd.grad(yi, xi, dyi, retain_graph=True))
        assert len(bi) == 1 and "k_csr_block_mean_bwd" in bi[0], bi
        counts.add((len(own), len(f), len(own_b), len(bwd), len(bi)))
    assert len(counts) == 1 and next(iter(counts))[:3] == (5, 1, 1), counts


def test_a_block_reads_four_bytes_back():
    c = container("directed")
    nodes = _dev(BC.targets("directed", "seven"))
    ops.csr_sample_block(c, nodes, 10, 1, nodes_checked=True)        # warm up
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        blk = ops.csr_sample_block(c, nodes, 10, 1, nodes_checked=True)
        inner = ops.csr_sample_block(c, blk, 10, 2)
        torch.cuda.synchronize()
    copies = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" in e.name.lower()]
    print([e.name for e in copies])
    assert len(copies) == 2, [e.name for e in copies]               # n_src of either block, and nothing else
    assert inner.nodes is blk and inner.n_src >= blk.n_src
