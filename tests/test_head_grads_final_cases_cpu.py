"""The cases of tests/test_gpu_head_grads_final.py, checked without a GPU: the gradients its bit comparisons leave to a
rounding tolerance are exactly level 1's six biases (never a level-0 gradient), and every case's seed keeps the oracle's
own head pre-activations away from ReLU's kink (the margin of tests/test_gpu_level0_phase0.py)."""
import pytest

from oracle import diffpool_oracle as O
from tests import head_grads_final_cases as HC

NAMES = [c[0] for c in HC.CASES]


def test_the_cases_cover_what_they_claim():
    rows = [c[1:6] for c in HC.CASES]
    assert {(B, h) for B, h, *_ in rows} == {(B, h) for B in (1, 5, 33) for h in ((), (50,), (7, 5))}
    for B in (1, 5, 33):
        mine = [r for r in rows if r[0] == B]
        assert {r[2] for r in mine} == {2, 6} and {r[3] for r in mine} == {True, False} and {r[4] for r in mine} == {1, 2}
    assert (33, False, 2) in {(r[0], r[3], r[4]) for r in rows}


@pytest.mark.parametrize("name", NAMES)
def test_only_level_one_biases_are_compared_to_rounding(name):
    model = HC.build(name)[0]
    loose = set(HC.atomic_bias_names(model))
    if model.num_pooling == 1:
        assert not loose
        return
    level = {}
    for kind, lvl, mods in model._graph_param_groups():
        if kind in ("embed", "assign"):
            for k, p in model.named_parameters():
                if any(p is q for m in mods for q in m.parameters()):
                    level[k] = lvl
    assert len(loose) == 6 and all(k.endswith(".bias") and level[k] == 1 for k in loose), loose
    # level 0 (persistent kernel) and the last level (whole-level kernel) sum in a fixed order: compared bit for bit
    assert not loose & {"conv_first.bias", "conv_block.0.bias", "conv_last.bias", "assign_conv_first_0.bias",
                        "assign_conv_block_0.0.bias", "assign_conv_last_0.bias", "conv_first2.bias",
                        "conv_block2.0.bias", "conv_last2.bias"}
    assert {"assign_conv_first_0.bias", "conv_first2.bias"} <= set(level)


@pytest.mark.parametrize("name", NAMES)
def test_the_seed_keeps_the_head_away_from_the_relu_kink(name):
    _, B, hidden, Cc, bn, P, seed = HC.CASE[name]
    model, params, x, adj, nn_, label = HC.build(name)
    _, inter = O.softpool_forward(params, x, adj, nn_, x, num_pooling=P, n_pred_hidden=len(hidden), bn=bn)
    for i, pre in enumerate(HC.head_preactivations(params, inter["readout"], len(hidden))):
        assert float(pre.abs().min()) > 1e-5 * float(pre.abs().max()), (i, float(pre.abs().min()))
