"""The persistent level-0 kernels with work moved under the backward's graph barriers (csrc/dp_level0.hip: l0_arrive / l0_wait)
and the shared layer-0 input (`x` and `assign_x` one tensor: staged once).  Each case counts one forward and one backward
launch of the persistent pair, is held to the CPU oracle at the tolerances of test_gpu_level0, and runs twice in one
process with the second run bit-equal to the first."""
import pytest
import torch

from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests.parity import close, grads_close, gpu_winners
from tests.test_gpu_level0 import _Counted

pytestmark = pytest.mark.gpu


def _batch(B, N, F_, Cc, p, *, seed=1, sizes=None, weighted=False, assign_dim=-1):
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=max(1, N // 10), p=p, seed=seed, n_classes=Cc, sizes=sizes)
    if weighted:        # edge weights that bf16 cannot hold (the construction of test_gpu_level0)
        g = torch.Generator().manual_seed(seed + 100)
        w = torch.rand(B, N, N, generator=g) + 0.5
        adj = adj * (w + w.transpose(1, 2))
    xa = None
    if assign_dim > 0:  # an assign input of its own; zero rows past each graph's nodes like x
        g = torch.Generator().manual_seed(seed + 200)
        xa = torch.randn(B, N, assign_dim, generator=g) * O.node_mask(N, nn_)
    return x, adj, nn_, label, xa


def _gpu_run(model, xd, ad, nn_, ld, xad, linkpred):
    """One forward + loss + backward: (ypred, loss, assignment, gradients, readout winners), one launch of each kernel."""
    model.zero_grad(set_to_none=True)
    with _Counted() as cnt:
        ypred = model(xd, ad, nn_, assign_x=xad)
        win = gpu_winners(model, 2)
        loss = model.loss(ypred, ld, ad, nn_) if linkpred else model.loss(ypred, ld)
        loss.backward()
    assert cnt.n == [1, 1], f"persistent level-0 kernels launched {cnt.n} times (forward, backward): expected [1, 1]"
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    return ypred.detach().clone(), loss.detach().clone(), model.assign_tensor.detach().clone(), grads, win


def _same_bits(r, s, what):
    for i, name in enumerate(("ypred", "loss", "assignment")):
        assert torch.equal(r[i], s[i]), f"{what}: {name} differs"
    assert set(r[3]) == set(s[3])
    for k in r[3]:
        assert torch.equal(r[3][k], s[3][k]), f"{what}: gradient of {k} differs"


def _case(B, N, F_, H, Cc, ratio, p, linkpred, *, seed=1, sizes=None, weighted=False, assign_dim=-1, cloned=False):
    x, adj, nn_, label, xa = _batch(B, N, F_, Cc, p, seed=seed, sizes=sizes, weighted=weighted, assign_dim=assign_dim)
    model = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=ratio, linkpred=linkpred, assign_input_dim=assign_dim)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed - 1, bias_scale=0.1)
    model.load_state_dict(params)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    xad = xd if xa is None else xa.cuda()
    first = _gpu_run(model, xd, ad, nn_, ld, xad, linkpred)
    _same_bits(first, _gpu_run(model, xd, ad, nn_, ld, xad, linkpred), "second run in the same process")
    if cloned:          # the same values from another tensor: the staged-twice path
        other = _gpu_run(model, xd, ad, nn_, ld, xd.clone(), linkpred)
        _same_bits(first, other, "assign_x = x.clone() against assign_x = x")
        for a_, b_ in zip(first[4], other[4]):
            assert torch.equal(a_, b_)
    ypred, loss, assign, grads, win = first
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo, inter = O.softpool_forward(P, x, adj, nn_, x if xa is None else xa, winners=win)
    lo, _ = O.softpool_loss(yo, label, inter["assign_0"], adj, nn_, linkpred)
    lo.backward()
    close(ypred, yo)
    close(assign, inter["assign_0"], 1e-4, 1e-6)
    close(loss, lo, 1e-4, 1e-6)
    for k, p_ in model.named_parameters():
        p_.grad = grads[k]
    grads_close(model, {k: v.grad for k, v in P.items()})
    return params, (x, adj, nn_), ypred, win


@pytest.mark.parametrize("B,N,F_,H,ratio,p,linkpred", [
    (4, 64, 5, 8, 0.25, 0.15, False),
    (5, 132, 8, 12, 0.1, 0.05, True),          # last block of 4 rows, link loss
])
def test_shared_input_equals_the_staged_twice_path_bit_for_bit(B, N, F_, H, ratio, p, linkpred):
    """`assign_x is x` (the input rows staged once, both layer-0 products and both dW products from the one copy) against
    `assign_x = x.clone()` (equal values, another pointer: staged twice): every output and gradient torch.equal, and both
    right by the oracle."""
    _case(B, N, F_, H, 3, ratio, p, linkpred, cloned=True)


@pytest.mark.parametrize("N,linkpred,assign_dim", [(64, False, 7), (160, True, 7), (64, True, 5)])
def test_assign_input_of_its_own_is_not_shared(N, linkpred, assign_dim):
    """An `assign_x` of its own beside F = 5: another width (assign_input_dim = 7), or the SAME width with other values
    in another tensor — the flag must follow the pointers, not the widths — and the assign stack reads its own rows."""
    _case(4, N, 5, 8 if N == 64 else 12, 3, 0.25 if N == 64 else 0.1, 0.15 if N == 64 else 0.05, linkpred,
          assign_dim=assign_dim)


def test_weighted_adjacency_through_the_reordered_phases():
    """The fp32 aggregation fallback (an adjacency bf16 cannot hold) with the windows under the barriers filled."""
    _case(6, 160, 8, 12, 2, 0.1, 0.04, True, weighted=True)


def test_max_readout_partial_with_tiny_and_full_graphs():
    """Graphs of 1, 2 and N nodes in one batch, masked readout: the winners are rows of the graph (or -1, a masked zero
    row) and the oracle, given those winners, agrees."""
    sizes = [1, 2, 160, 17, 160, 3]
    params, (x, adj, nn_), ypred, win = _case(6, 160, 8, 12, 3, 0.1, 0.3, True, sizes=sizes)
    w0 = win[0]
    for b, n in enumerate(sizes):
        assert int(w0[b].max()) < n and int(w0[b].min()) >= -1, (b, n, w0[b])
    # ... and the oracle's own arg-max (no winners handed over) reads the same maxima
    close(ypred, O.softpool_forward(params, x, adj, nn_, x)[0])
