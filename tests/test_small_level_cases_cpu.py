"""The cases of tests/test_gpu_small_level.py (tests/small_level_cases.py), checked without a GPU: the table covers the
classes it claims, on both small tiers where it must; every expected tier and quoted float count follows from the plan
formulas; each model has the level dims, n and B the table says; every seed keeps the fp64 reference away from ReLU's
kink and BatchNorm well conditioned; and the yardstick bound of the level check is one a correct fp32 implementation
(the fp32 CPU oracle) meets."""
import functools

import pytest
import torch

from tests import small_level_cases as SC

WHOLE = [c for c in SC.CASES if c.tier == "whole"]


def _widths(cases):
    return {d for c in cases for d in SC.level_dims(c)}


def test_the_table_covers_every_class():
    assert 25 <= len(SC.CASES) <= 35 and len(set(SC.NAMES)) == len(SC.NAMES)
    # starred classes: among the cases expected on the whole-level tier, which also run per layer under the knob
    assert {1, 15, 16, 17, 31, 32, 33, 48, 63, 64} <= {c.n for c in WHOLE}
    assert {1, 3, 5, 4, 15, 16, 17, 20, 33, 63, 64} <= _widths(WHOLE)
    assert any(all(a != b for a, b in zip(d, d[1:])) for d in map(SC.level_dims, WHOLE))
    assert {3, 89, 255, 256} <= {c.F for c in WHOLE if c.fam == "B"}
    assert {2, 3, 4, 8} <= {c.L for c in WHOLE}
    # the rest, anywhere in the table
    assert {1, 2, 15, 16, 17, 32, 33, "bmax", "bmax+1"} <= {c.B for c in SC.CASES}
    for c in SC.CASES:
        if isinstance(c.B, str) or c.B > 33:
            assert c.n <= 8 and max(c.H, c.E) <= 8, c.name                    # large batches stay cheap
    by = {c.name: c for c in SC.CASES}
    assert by["p_n65"].n == 65 and by["p_n65"].tier == "generic"
    assert by["p_e65"].E == 65 and by["p_e65"].tier == "per_layer"
    assert any(c.tier == "per_layer" and 64 < max(SC.level_dims(c)[1:]) <= 256 and c.name != "p_e65" for c in SC.CASES)
    assert by["b_f257"].F == 257 and by["b_f257"].tier == "generic"
    assert by["p_bmax1"].tier == "per_layer" and by["p_bmax1"].n == 4
    assert {True, False} <= {c.bn for c in WHOLE if c.fam == "P"} and {True, False} <= {c.bn for c in WHOLE if c.fam == "B"}
    assert any(not c.bias for c in WHOLE if c.fam == "B") and any(not c.concat for c in WHOLE if c.fam == "B")
    assert {(), (7, 5)} <= {c.hidden for c in WHOLE if c.fam == "P"}
    nofold = [c for c in WHOLE if c.fam == "P" and not SC.head_folds(c)]
    # (the whole-tier edge case leaves no room for any head: 38 234 + 2 * 256 + 2 floats)
    assert [c.name for c in nofold] == ["p_n33_nofold", "p_n57_whole_edge"]
    assert len(SC.DROP_BWD) <= 3 and set(SC.DROP_BWD) <= set(SC.NAMES)
    assert all(1 in (SC.CASE[k].n, *SC.level_dims(SC.CASE[k])) for k in SC.DROP_BWD)


def test_the_boundary_pairs_sit_on_the_limit():
    """Largest n inside the tier and the first n past it, at fixed widths and batch."""
    for inside, past, formula in (("p_n57_whole_edge", "p_n58_whole_edge", "level_bwd"),
                                  ("p_n47_layer_edge", "p_n48_layer_edge", "layer_bwd")):
        a, b = SC.CASE[inside], SC.CASE[past]
        assert a._replace(name="", n=0, tier="", seed=0) == b._replace(name="", n=0, tier="", seed=0) and b.n == a.n + 1
        assert SC.QUOTED[inside][0] == SC.QUOTED[past][0] == formula
        assert SC.QUOTED[inside][2] <= SC.LIM < SC.QUOTED[past][2]
        assert SC.planned_tier(a) != SC.planned_tier(b)
    # the same shape leaves the per-layer tier through its B * n * 2 term alone
    a, b = SC.CASE["p_n47_layer_edge"], SC.CASE["p_n47_b33"]
    assert a._replace(name="", B=0, tier="", seed=0) == b._replace(name="", B=0, tier="", seed=0)
    assert (a.tier, b.tier) == ("per_layer", "generic")


@pytest.mark.parametrize("name", SC.NAMES)
def test_expected_tier_follows_from_the_formulas(name):
    c = SC.CASE[name]
    assert SC.planned_tier(c) == c.tier
    assert SC.planned_tier(c, no_level_fusion=True) == ("per_layer" if c.tier == "whole" else c.tier)
    # the whole-level forward formula never decides (module docstring)
    assert SC.lds_level_fwd(c.n, SC.level_dims(c)) < SC.lds_level_bwd(c.n, SC.level_dims(c))
    if name in SC.QUOTED:
        formula, layer, floats = SC.QUOTED[name]
        dims, B = SC.level_dims(c), SC.batch_size(c)
        got = SC.lds_level_bwd(c.n, dims) if formula == "level_bwd" else \
            SC.lds_layer_bwd(B, c.n, dims[layer], dims[layer + 1])
        assert got == floats


@functools.lru_cache(maxsize=None)
def _built(name):
    return SC.build(name)


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_model_has_the_shapes_the_table_says(name):
    c = SC.CASE[name]
    model, params, x, adj, nn_, label = _built(name)
    sd = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    keys = SC.stack_keys(c)
    dims = [sd[keys[0] + ".weight"][0]] + [sd[k + ".weight"][1] for k in keys]
    assert dims == SC.level_dims(c) and len(keys) == c.L
    assert all((k + ".bias" in sd) == c.bias for k in keys)
    B = SC.batch_size(c)
    assert x.shape[0] == adj.shape[0] == len(nn_) == label.shape[0] == B
    if c.fam == "P":
        assert adj.shape[1] == 2 * c.n and model.assign_dims == [c.n] and sd["assign_pred.weight"][0] == c.n
        assert int(nn_.min()) >= max(1, c.n)
        assert sd["pred_model.weight" if not c.hidden else "pred_model.0.weight"][1] == 2 * sum(dims[1:])
    else:
        assert adj.shape[1] == c.n and (c.n < 64 or not c.concat)
        assert sd["pred_model.weight" if not c.hidden else "pred_model.0.weight"][1] == \
            (sum(dims[1:]) if c.concat else c.E)
    n_lin = sum(k.startswith("pred_model") and k.endswith(".weight") for k in sd)
    assert n_lin == len(c.hidden) + 1


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_seed_keeps_the_reference_off_the_kink_and_batchnorm_conditioned(name):
    c = SC.CASE[name]
    model, params, x, adj, nn_, label = _built(name)
    got = SC.oracle_got(c, params, x, adj, nn_, torch.float64)       # the fp64 forward with its own arg-max
    r64 = SC.level_alone(c, params, label, got, torch.float64, x, adj)
    assert len(r64["pre"]) == c.L - 1 and len(r64["head_pre"]) == len(c.hidden)
    for i, t in enumerate(r64["pre"] + r64["head_pre"]):
        assert float(t.abs().min()) > 1e-5 * float(t.abs().max()), \
            f"pre-activation {i} sits on a ReLU kink ({float(t.abs().min()):.3e}): choose another seed"
    if c.bn and name not in SC.DROP_BWD:
        for i, t in enumerate(r64["act"]):
            mu = t.mean(dim=(0, 2), keepdim=True)
            assert float((t - mu).pow(2).mean(dim=(0, 2)).min()) >= 1e-6, f"layer {i}: a degenerate BatchNorm row"


@pytest.mark.parametrize("name", SC.NAMES)
def test_a_correct_fp32_implementation_meets_the_bound(name):
    """The level check of the GPU test, with the fp32 CPU oracle's whole-model step in the GPU's place."""
    c = SC.CASE[name]
    model, params, x, adj, nn_, label = _built(name)
    got = SC.oracle_got(c, params, x, adj, nn_, torch.float32)
    win = [got["argmax0"], got["argmax1"]] if c.fam == "P" else [got["argmax0"]]
    _, _, grads, _ = SC.end_to_end(c, params, x, adj, nn_, label, win, torch.float32)
    got.update({"grad." + k: g for k, g in grads.items()})
    rows = SC.level_figures(c, params, label, got, x, adj)
    want = 1 if name in SC.DROP_BWD else 1 + len(SC.level_names(c, params))
    assert len(rows) == want
    for k, err, e_ref, bound, scale in rows:
        assert e_ref == e_ref and e_ref < float("inf") and 0 < bound < float("inf"), (k, e_ref, bound)
    assert not SC.failures(rows), SC.failures(rows)


@pytest.mark.parametrize("name", ["p_n16_b15", "p_n64_h64", "b_f3_addself", "b_f257"])
def test_gradients_left_to_rounding_are_named_by_rule(name):
    c = SC.CASE[name]
    model = _built(name)[0]
    loose = set(SC.loose_names(model, c, c.tier))
    assert all(k.endswith(".bias") for k in loose)
    level0 = {"grad." + k + ".bias" for k in ("conv_first", "conv_block.0", "conv_last", "assign_conv_first",
                                              "assign_conv_block.0", "assign_conv_last", "assign_pred")}
    under_test = {"grad." + k + ".bias" for k in SC.stack_keys(c)}
    if c.fam == "P":
        assert loose == level0 | (under_test if c.tier == "generic" else set())
    else:
        assert loose == (under_test if c.tier == "generic" else set())
