"""The symmetric-adjacency short form of the persistent level-0 backward (csrc/dp_level0.hip).

For A' = S^T A S the backward needs dS = A (S dA'^T) + (A^T S) dA' + Z dX'^T (encoders.py:1278-1279).  The forward kernel
decides per graph, exactly and on the device, whether the adjacency is bf16-exact AND equal to its transpose bit for bit;
for such a graph A S is the saved Tt = A^T S, so the backward multiplies Tt dA'^T row-locally and skips the split of V,
a graph barrier, the staging of its rows of A and the N x N x K aggregation.  Every other graph takes the general form.

Every case: forward outputs (ypred, assignment, loss) and every parameter gradient against the CPU oracle at the
tolerances of tests/parity.py (the short form is a reassociation: no tolerance of its own), the per-graph verdicts the
backward acted on (dp_level0_bwd_symmetric — without them a short form that is never taken would pass), the rows per
workgroup the launch used, and the step twice with torch.equal on everything.

The backward's bf16 / fp32 choice is per BATCH (one graph that bf16 cannot hold sends every graph's aggregation through
the fp32 products), and the short form is taken only on the bf16 path: a batch with one inexact graph reports 0 for all."""
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import PackedAdjacency, SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests.parity import close, grads_close, gpu_winners
from tests.test_gpu_level0 import _Counted

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each instantiation (rows per workgroup: the smallest of 16 / 32 / 48 / 64 with
# B * ceil(N / rows) <= CUs); graph `g` (all N nodes) is the one the cases edit
SHAPES = {
    # 16 rows, T = 4 blocks per graph
    "rb16": dict(B=3, N=64, F_=5, H=8, Cc=3, ratio=0.25, p=0.15, RB=16, sizes=[40, 64, 9], g=1),
    # 16 rows, T = 7, a last block of 4 rows, packed rows padded to 104 columns
    "ragged": dict(B=4, N=100, F_=5, H=8, Cc=3, ratio=0.1, p=0.1, RB=16, sizes=[100, 57, 16, 1], g=0),
    # 48 rows, T = 3: the <3> instantiation the DD workload runs
    "rb48": dict(B=64, N=144, F_=6, H=12, Cc=2, ratio=0.1, p=0.05, RB=48, sizes=None, g=1),
}
# one directed edge i -> j (A[i][j] = 1, A[j][i] = 0) per shape: i and j in different row blocks, inside one block, i in
# the last (partial, where there is one) block, j = N - 1
DIRECTED = {
    "rb16": {"blocks": (5, 40), "inside": (17, 29), "last": (62, 3), "lastcol": (20, 63)},
    "ragged": {"blocks": (5, 70), "inside": (33, 46), "last": (98, 10), "lastcol": (20, 99)},
    "rb48": {"blocks": (5, 100), "inside": (50, 60), "last": (140, 7), "lastcol": (3, 143)},
}


def _batch(shape, seed=1):
    s = SHAPES[shape]
    sizes = s["sizes"]
    if sizes is None:           # seeded sizes, graph g full
        gen = torch.Generator().manual_seed(seed + 50)
        sizes = torch.randint(s["N"] // 8, s["N"] + 1, (s["B"],), generator=gen).tolist()
        sizes[s["g"]] = s["N"]
    x, adj, nn_, label = O.make_batch(s["B"], s["N"], s["F_"], n_min=1, p=s["p"], seed=seed, n_classes=s["Cc"], sizes=sizes)
    assert torch.equal(adj, adj.transpose(1, 2))
    return x, adj, nn_, label


def _model(shape, linkpred, seed=1):
    s = SHAPES[shape]
    model = SoftPoolingGcnEncoder(s["N"], s["F_"], s["H"], s["H"], s["Cc"], 3, s["H"], assign_ratio=s["ratio"], linkpred=linkpred)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed - 1, bias_scale=0.1)
    model.load_state_dict(params)
    return model.cuda(), params


def _step(model, xd, ad, nn_, ld, linkpred):
    """One forward + loss + backward through the persistent pair: outputs, gradients, winners, (verdicts, rows per block)."""
    model.zero_grad(set_to_none=True)
    with _Counted() as cnt:
        ypred = model(xd, ad, nn_, assign_x=xd)
        win = gpu_winners(model, 2)
        loss = model.loss(ypred, ld, ad, nn_) if linkpred else model.loss(ypred, ld)
        loss.backward()
    assert cnt.n == [1, 1], f"persistent level-0 kernels launched {cnt.n} times (forward, backward): expected [1, 1]"
    return dict(ypred=ypred.detach().clone(), loss=loss.detach().clone(), assign=model.assign_tensor.detach().clone(),
                grads={k: p.grad.clone() for k, p in model.named_parameters()}, win=win, form=_lib.level0_bwd_symmetric())


def _same_bits(r, s, what):
    for name in ("ypred", "loss", "assign"):
        assert torch.equal(r[name], s[name]), f"{what}: {name} differs"
    assert set(r["grads"]) == set(s["grads"])
    for k in r["grads"]:
        assert torch.equal(r["grads"][k], s["grads"][k]), f"{what}: gradient of {k} differs"


def _case(shape, adj, expect, *, x, nn_, label, linkpred=False, masked=True, packed=False):
    """Runs the step twice on `adj`, holds it to the oracle and to the expected verdicts; returns the first run."""
    s = SHAPES[shape]
    model, params = _model(shape, linkpred)
    nn_arg = nn_ if masked else None
    xd, ld = x.cuda(), label.cuda()
    ad = adj.cuda().contiguous()
    if packed:
        ad = PackedAdjacency.from_dense(ad)
    first = _step(model, xd, ad, nn_arg, ld, linkpred)
    second = _step(model, xd, ad, nn_arg, ld, linkpred)
    _same_bits(first, second, "second run in the same process")
    for r in (first, second):
        verdicts, rows = r["form"]
        assert rows == s["RB"], f"{shape}: the launch used {rows} rows per workgroup, the case was built for {s['RB']}"
        assert verdicts == list(expect), f"{shape}: verdicts {verdicts}, expected {list(expect)}"
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo, inter = O.softpool_forward(P, x, adj, nn_arg, x, winners=first["win"])
    lo, _ = O.softpool_loss(yo, label, inter["assign_0"], adj, nn_arg, linkpred)
    lo.backward()
    close(first["ypred"], yo)
    close(first["assign"], inter["assign_0"], 1e-4, 1e-6)
    close(first["loss"], lo, 1e-4, 1e-6)
    for k, p_ in model.named_parameters():
        p_.grad = first["grads"][k]
    grads_close(model, {k: v.grad for k, v in P.items()})
    return first


def _directed(shape, adj, where):
    i, j = DIRECTED[shape][where]
    adj = adj.clone()
    adj[SHAPES[shape]["g"], i, j] = 1.0
    adj[SHAPES[shape]["g"], j, i] = 0.0
    return adj


def _all_but(shape, g=None):
    s = SHAPES[shape]
    return [0 if b == (s["g"] if g is None else g) else 1 for b in range(s["B"])]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_symmetric_01_graphs_take_the_short_form(shape):
    x, adj, nn_, label = _batch(shape)
    _case(shape, adj, [1] * SHAPES[shape]["B"], x=x, nn_=nn_, label=label)


@pytest.mark.parametrize("where", ["blocks", "inside", "last", "lastcol"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_directed_edge_sends_that_graph_alone_through_the_general_form(shape, where):
    """A batch that mixes both forms: the edited graph crosses the A V barrier, the others do not."""
    x, adj, nn_, label = _batch(shape)
    _case(shape, _directed(shape, adj, where), _all_but(shape), x=x, nn_=nn_, label=label)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_symmetric_bf16_exact_weights_take_the_short_form(shape):
    """Edge weights 0.5 and 2 (bf16 holds them): symmetric, exact — the short form on values that are not 0 / 1."""
    x, adj, nn_, label = _batch(shape)
    w = torch.where(torch.rand(adj.shape, generator=torch.Generator().manual_seed(7)) < 0.5, 0.5, 2.0)
    w = torch.triu(w, 1)
    adj = adj * (w + w.transpose(1, 2))
    assert set(adj.unique().tolist()) == {0.0, 0.5, 2.0} and torch.equal(adj, adj.transpose(1, 2))
    _case(shape, adj, [1] * SHAPES[shape]["B"], x=x, nn_=nn_, label=label)


@pytest.mark.parametrize("kind", ["weight_0.3", "one_and_one_plus_2^-20"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_values_bf16_cannot_hold_are_never_symmetric(shape, kind):
    """A symmetric pair of weight 0.3, and a pair 1 / 1 + 2^-20 whose bf16 truncations ARE equal: the graph is not
    bf16-exact, so its verdict is 0 whatever the bits say — and the batch-wide fp32 path reports 0 for every graph."""
    x, adj, nn_, label = _batch(shape)
    g, (i, j) = SHAPES[shape]["g"], DIRECTED[shape]["blocks"]
    adj = adj.clone()
    if kind == "weight_0.3":
        adj[g, i, j] = adj[g, j, i] = 0.3
    else:
        adj[g, i, j] = 1.0
        adj[g, j, i] = 1.0 + 2.0 ** -20
        assert float(adj[g, j, i]) != 1.0
    _case(shape, adj, [0] * SHAPES[shape]["B"], x=x, nn_=nn_, label=label)


def test_link_loss_gradient_enters_the_short_form():
    """linkpred=True: d_assign joins the same softmax backward that reads the row-local term."""
    x, adj, nn_, label = _batch("rb16")
    _case("rb16", adj, [1] * 3, x=x, nn_=nn_, label=label, linkpred=True)


@pytest.mark.parametrize("directed", [False, True])
def test_without_num_nodes(directed):
    x, adj, nn_, label = _batch("rb16")
    if directed:
        adj = _directed("rb16", adj, "blocks")
    _case("rb16", adj, _all_but("rb16") if directed else [1] * 3, x=x, nn_=nn_, label=label, masked=False)


@pytest.mark.parametrize("directed", [False, True])
def test_packed_adjacency_entry_is_bit_identical_to_the_fp32_entry(directed):
    """The packed input (bf16 rows of A and A^T handed in): same verdicts, and every output and gradient torch.equal to
    the run that was given the same adjacency in fp32."""
    x, adj, nn_, label = _batch("ragged")
    if directed:
        adj = _directed("ragged", adj, "last")
    expect = _all_but("ragged") if directed else [1] * 4
    dense = _case("ragged", adj, expect, x=x, nn_=nn_, label=label, linkpred=True)
    packed = _case("ragged", adj, expect, x=x, nn_=nn_, label=label, linkpred=True, packed=True)
    _same_bits(dense, packed, "packed-adjacency entry against the fp32 entry")
