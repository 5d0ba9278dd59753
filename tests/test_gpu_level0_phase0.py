"""Phase 0 of the persistent level-0 forward (csrc/dp_level0.hip, k_level0_fwd) with the layer-0 product run under the
adjacency burst: the layer-0 inputs and weights are asked for ahead of the adjacency quads, committed while those are in
flight, multiplied, and only then are the quads converted; the biases are staged behind the split.  Every case counts one
forward and one backward launch of the persistent pair, checks the rows per workgroup the case was built for (so each
instantiation <1..4> of the kernel really runs), is held to the CPU oracle at the tolerances of test_gpu_level0, and runs
twice with the second run bit-equal to the first.

l0_geometry takes the smallest RB in {16, 32, 48, 64} with B * ceil(N / RB) <= 256 CUs:
  (4, 64) -> 16      (20, 256) -> 32      (40, 224) -> 48, last block 32 rows      (60, 224) -> 64
  (5, 132) -> 16, last block 4 rows      (4, 516) -> 16, two 512-column segments (only segment 0 is held across the product)"""
import types

import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import PackedAdjacency, SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests.parity import close, grads_close
from tests.test_gpu_level0_overlap import _batch, _gpu_run, _same_bits

pytestmark = pytest.mark.gpu


def _away_from_the_head_relu_kink(P, inter):
    """A check of the CASE, not of the kernels: the gradient is discontinuous where a hidden unit of pred_model sits at
    ReLU's kink.  Two correct fp32 evaluations differ by a few 1e-7 of the layer's scale there (sums of <= 100 terms in
    another order), so a unit whose pre-activation is closer to zero than that is on for one and off for the other, and
    every gradient behind it moves by a percent although both are right.  The cases keep a margin of 1e-5 of the
    largest pre-activation, some 40 roundings.  Seed 1 at B = 60, N = 224 has a unit at -1.5e-7 where the layer's
    largest is 2.4, half a rounding of that scale (the next smallest is 3.0e-4): the oracle's fp32 and fp64 gradients
    agree to 3e-7 there and another summation order moves all of them by up to 2 %.  That batch uses seed 2 (margin
    1.9e-4 of 2.6)."""
    pre = torch.nn.functional.linear(inter["readout"], P["pred_model.0.weight"], P["pred_model.0.bias"]).detach()
    assert float(pre.abs().min()) > 1e-5 * float(pre.abs().max()), \
        f"the case sits on a ReLU kink of the head: |pre-activation| {float(pre.abs().min()):.3e}: choose another seed"


def _case(B, N, F_, H, ratio, p, linkpred, RB, *, Cc=3, seed=1, weighted=False, assign_dim=-1, bias=True, packed=False):
    x, adj, nn_, label, xa = _batch(B, N, F_, Cc, p, seed=seed, weighted=weighted, assign_dim=assign_dim)
    model = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=ratio, linkpred=linkpred, assign_input_dim=assign_dim,
                                  args=types.SimpleNamespace(bias=bias))
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed - 1, bias_scale=0.1)
    assert any(k.startswith("conv_") and k.endswith(".bias") for k in params) == bias
    model.load_state_dict(params)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    xad = xd if xa is None else xa.cuda()
    first = _gpu_run(model, xd, ad, nn_, ld, xad, linkpred)
    assert _lib.level0_bwd_symmetric()[1] == RB, "the launch did not use the rows per workgroup this case was built for"
    _same_bits(first, _gpu_run(model, xd, ad, nn_, ld, xad, linkpred), "second run in the same process")
    if packed:          # the bf16 rows handed in (dp_encoder_forward_packed): the other body of phase 0, the same bits
        other = _gpu_run(model, xd, PackedAdjacency.from_dense(ad), nn_, ld, xad, linkpred)
        _same_bits(first, other, "packed adjacency against the fp32 adjacency")
    ypred, loss, assign, grads, win = first
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo, inter = O.softpool_forward(P, x, adj, nn_, x if xa is None else xa, winners=win)
    lo, _ = O.softpool_loss(yo, label, inter["assign_0"], adj, nn_, linkpred)
    lo.backward()
    _away_from_the_head_relu_kink(P, inter)
    close(ypred, yo)
    close(assign, inter["assign_0"], 1e-4, 1e-6)
    close(loss, lo, 1e-4, 1e-6)
    for k, p_ in model.named_parameters():
        p_.grad = grads[k]
    grads_close(model, {k: v.grad for k, v in P.items()})


@pytest.mark.parametrize("B,N,F_,H,ratio,p,RB", [
    (4, 64, 5, 8, 0.25, 0.15, 16),
    (20, 256, 8, 12, 0.1, 0.04, 32),
    (40, 224, 8, 12, 0.1, 0.04, 48),           # last block has 32 of 48 rows
    (60, 224, 8, 12, 0.1, 0.04, 64),
])
def test_every_instantiation(B, N, F_, H, ratio, p, RB):
    """k_level0_fwd<1..4>, one case each."""
    _case(B, N, F_, H, ratio, p, False, RB, seed=2 if B == 60 else 1)


def test_short_last_block():
    _case(5, 132, 8, 12, 0.1, 0.05, True, 16)


def test_two_column_segments():
    """N > 512: segment 0 is in flight across the product, segment 1 is fetched behind it."""
    _case(4, 516, 6, 8, 0.05, 0.02, False, 16)


def test_weighted_adjacency_raises_the_inexact_flag_behind_the_product():
    """An adjacency bf16 cannot hold: the exactness check now runs after the product, the fp32 fallback follows it."""
    _case(6, 160, 8, 12, 0.1, 0.04, True, 16, Cc=2, weighted=True)


@pytest.mark.parametrize("B,N,RB", [(4, 64, 16), (40, 224, 48)])
def test_assign_input_of_its_own(B, N, RB):
    """assign_input_dim = 7: x is not shared, four side regions are staged ahead of the adjacency."""
    _case(B, N, 5, 12, 0.1, 0.1, False, RB, assign_dim=7)


def test_input_rows_longer_than_one_stage():
    """64 rows x 140 features = 8960 floats > 8192 (4 quads per thread): the rest of the rows is fetched behind the
    staged part, in both bodies."""
    _case(60, 224, 140, 12, 0.1, 0.04, True, 64, assign_dim=7, packed=True)


@pytest.mark.parametrize("B,N,RB", [(5, 132, 16), (20, 256, 32)])
def test_no_bias(B, N, RB):
    """GraphConv layers without a bias: their slots are zeros (the bias staging moved behind the split)."""
    _case(B, N, 8, 12, 0.1, 0.05, True, RB, bias=False)


@pytest.mark.parametrize("B,N,RB,assign_dim", [(5, 132, 16, -1), (40, 224, 48, 7), (4, 516, 16, -1)])
def test_packed_entry(B, N, RB, assign_dim):
    """The packed-adjacency body of phase 0 gives the bits of the fp32 body (and both agree with the oracle)."""
    _case(B, N, 6, 12, 0.1 if N < 512 else 0.05, 0.04 if N < 512 else 0.02, True, RB, assign_dim=assign_dim, packed=True)
