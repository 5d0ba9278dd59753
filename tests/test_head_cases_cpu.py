"""The cases of tests/test_gpu_head.py (tests/head_cases.py), checked without a GPU: the table reaches every edge of
csrc/dp_head.hip it claims; every expected plan and quoted float count follows from the restated formulas and each
boundary pair sits one step apart on opposite sides of its limit; each model has the widths, rows and batch the table
says; every seed keeps the fp64 head away from ReLU's kink and the whole model conditioned; the forced outcomes (tie, -1
winner, predict tie) hold on the fp64 reference alone; and the head check leaves nothing out and is one a correct fp32
implementation meets."""
import functools
import os

import pytest
import torch

from oracle import diffpool_oracle as O
from tests import head_cases as HC
from tests import small_level_cases as SC

BY = HC.CASE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_limits_are_the_kernels_own():
    with open(os.path.join(ROOT, "graph_pooling_amd", "csrc", "dp_head.hip")) as f:
        src = f.read()
    assert "HEAD_FWD_LDS_FLOATS = 30 * 1024" in src and "HEAD_BWD_LDS_FLOATS = 38 * 1024" in src
    assert "constexpr int HEAD_SLICE = 16;" in src and "a.B > 1024" in src
    assert "a.rw <= 64 && a.n <= 4 * RU" in src and "constexpr int RU = 16;" in src
    assert "(din + 3) / 4" in src and "j0 += 64" in src
    assert HC.STAGE_ROUND == 256 * 16 and "e0 += NT * 16" in src


def test_the_table_reaches_every_readout_form():
    P = [c for c in HC.CASES if c.fam == "P" and c.fwd == "fused"]
    shapes = {(c.n, HC.readout_width(c)) for c in P}
    assert {(1, 5), (5, 13), (64, 64), (65, 64), (16, 65), (2, 130)} <= shapes
    assert HC.one_pass(BY["p_n1_rw5_lin"]) and HC.one_pass(BY["p_n5_rw13_h3_5"]) and HC.one_pass(BY["p_n64_rw64_h65"])
    assert not HC.one_pass(BY["p_n65_rw64_deep"]) and not HC.one_pass(BY["p_n16_rw65"])
    assert not HC.one_pass(BY["p_n2_rw130"])
    assert 5 % 4 != 0                                        # n = 5: rows wave + 4u are a partial set in wave 0 only
    assert BY["p_n2_rw130"].n < 3 and -(-130 // 64) == 3     # waves 2-3 own no row; three column passes
    assert 65 % 64 == 1                                      # second column pass with one live lane
    assert any(c.P == 2 for c in P) and any(c.special == "tie" for c in P) and any(c.special == "neg" for c in P)
    assert all(c.fwd == "fused" for c in HC.CASES if c.special)
    # odd rw: a backward slice of 16 features straddles the level boundary
    for name in ("p_n5_rw13_h3_5", "p_pool2_rw21"):
        assert HC.readout_width(BY[name]) % HC.HEAD_SLICE != 0


def test_the_table_reaches_every_mlp_and_staging_edge():
    dims = {c.name: HC.pred_dims(c) for c in HC.CASES}
    fused = [c for c in HC.CASES if c.fwd == "fused"]
    assert any(len(dims[c.name]) == 2 and c.C == 2 for c in fused)                         # L = 1
    d = dims["p_n5_rw13_h3_5"]
    assert d[1:3] == [3, 5] and [-(-k // 4) for k in d[1:3]] == [1, 2] and 3 * 1 >= 3 and 3 * 2 >= 5   # fourth wave empty
    assert any(64 < w <= 128 for c in fused for w in dims[c.name][1:])                    # two output passes
    assert any(len(c.hidden) == 4 for c in fused)                                         # DP_MAX_PRED hidden layers
    assert dims["p_d64_h64"][0] * dims["p_d64_h64"][1] == HC.STAGE_ROUND                  # exactly one round
    d = dims["b_d17_h241"]
    assert d[0] * d[1] == HC.STAGE_ROUND + 1 and d[0] == 17 and -(-d[0] // 16) == 2 and d[0] - 16 == 1   # ks = 1
    assert HC.HEAD_SLICE * dims["b_last_h257"][1] == 4112 and not BY["b_last_h257"].concat
    d = dims["p_b64_h70_65"]
    assert d[1] * d[2] == 4550 and BY["p_b64_h70_65"].B * d[1] == 4480
    d = dims["b_d4097"]
    assert d == [4097, 2] and HC.stage_rounds(d[0] * d[1]) == 3 and -(-d[0] // 16) == 257 and BY["b_d4097"].n == 8
    d0s = {dims[c.name][0] for c in fused}
    assert {0, 1, 15} <= {d % 16 for d in d0s if d >= 16} and any(d < 16 for d in d0s)
    # batch
    assert {1, 32, 33, 257, 1024} <= {c.B for c in fused} and BY["b_b1025"].B == 1025
    a, b = BY["b_b32"], BY["b_b33"]
    assert a._replace(name="", B=0) == b._replace(name="", B=0) and dims["b_b32"][0] >= 16
    assert (a.B * 16, b.B * 16) == (512, 528)                                             # 2 x 256 threads cover 512
    assert 16 * BY["b_b257"].B > HC.STAGE_ROUND
    c = BY["b_b1024_c5"]
    assert c.B * c.C == 5120 and not c.hidden and c.C == 5
    # every shape is tiny
    for c in HC.CASES:
        assert HC.level_nodes(c)[0] <= 130, c.name
        assert c.B <= 64 or (c.B in (257, 1024, 1025) and c.n <= 4), c.name
        assert c.C >= 2, "a width-1 last layer would have to be left out of the gradient check"
    assert len(HC.CASES) <= 30 and len(set(HC.NAMES)) == len(HC.NAMES)


def test_the_boundary_pairs_sit_on_the_limit():
    for inside, past, formula, limit in (("p_fwd_edge_in", "p_fwd_edge_out", "fwd", HC.HEAD_FWD_LDS_FLOATS),
                                         ("b_bwd_edge_in", "b_bwd_edge_out", "bwd", HC.HEAD_BWD_LDS_FLOATS)):
        a, b = BY[inside], BY[past]
        strip = dict(name="", hidden=(), fwd="", bwd="", seed=0)
        assert a._replace(**strip) == b._replace(**strip)
        assert len(a.hidden) == 1 and b.hidden == (a.hidden[0] + 1,)
        assert HC.QUOTED[inside][0] == HC.QUOTED[past][0] == formula
        assert HC.QUOTED[inside][1] <= limit < HC.QUOTED[past][1]
        assert a.fwd == "fused" and (b.fwd, b.bwd) == ("generic", "generic")
        # the other formula is far from deciding
        other = HC.head_bwd_lds_floats if formula == "fwd" else lambda B, d: HC.head_fwd_lds_floats(d)
        assert other(b.B, HC.pred_dims(b)) <= (HC.HEAD_BWD_LDS_FLOATS if formula == "fwd" else HC.HEAD_FWD_LDS_FLOATS)
    assert (BY["p_fwd_edge_in"].B, BY["p_fwd_edge_in"].C, HC.pred_dims(BY["p_fwd_edge_in"])[0]) == (2, 2, 26)
    assert (BY["b_bwd_edge_in"].B, BY["b_bwd_edge_in"].hidden) == (1024, (7,))
    assert 14 + 7168 + 112 + 16384 + 14336 == 38014 == HC.head_bwd_lds_floats(1024, HC.pred_dims(BY["b_bwd_edge_in"]))
    # B = 1024 against B = 1025, nothing else changed, and neither LDS limit near
    a, b = BY["b_b1024_c5"], BY["b_b1025"]
    strip = dict(name="", B=0, fwd="", bwd="")
    assert a._replace(**strip) == b._replace(**strip) and (a.B, b.B) == (HC.B_LIMIT, HC.B_LIMIT + 1)
    assert HC.head_bwd_lds_floats(b.B, HC.pred_dims(b)) <= HC.HEAD_BWD_LDS_FLOATS
    assert (a.fwd, a.bwd, b.fwd, b.bwd) == ("fused", "kernel", "generic", "generic")


@pytest.mark.parametrize("name", HC.NAMES)
def test_expected_plan_follows_from_the_formulas(name):
    c = BY[name]
    assert HC.planned(c) == (c.fwd, c.bwd)
    assert HC.planned(c, no_head_fold=True) == (c.fwd, "kernel" if c.bwd == "fold" else c.bwd)
    if c.fam == "B":
        assert c.P == 0 and c.bwd != "fold"
    if name in HC.QUOTED:
        formula, floats = HC.QUOTED[name]
        dims = HC.pred_dims(c)
        assert (HC.head_fwd_lds_floats(dims) if formula == "fwd" else HC.head_bwd_lds_floats(c.B, dims)) == floats


def test_both_backward_plans_are_reached_in_family_p():
    assert len(HC.FOLD) >= 8 and any(c.fam == "P" and c.bwd == "kernel" for c in HC.CASES)
    # every edge of k_head_bwd that only family P has runs the kernel at least under the knob
    assert {"p_n5_rw13_h3_5", "p_pool2_rw21", "p_neg", "p_tie", "p_b64_h70_65", "p_fwd_edge_in"} <= set(HC.FOLD)


@functools.lru_cache(maxsize=None)
def _built(name):
    return HC.build(name)


@functools.lru_cache(maxsize=None)
def _got64(name):
    c = BY[name]
    _, params, x, adj, nn_, _ = _built(name)
    return HC.oracle_got(c, params, x, adj, nn_, torch.float64)


@pytest.mark.parametrize("name", HC.NAMES)
def test_the_model_has_the_shapes_the_table_says(name):
    c = BY[name]
    model, params, x, adj, nn_, label = _built(name)
    sd = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    lins = [k for k in sd if k.startswith("pred_model") and k.endswith(".weight")]
    dims = [sd[lins[0]][1]] + [sd[k][0] for k in lins]
    assert dims == HC.pred_dims(c) and all(k[:-7] + ".bias" in sd for k in lins)
    assert lins[-1] == HC.last_linear(c) + ".weight"
    assert x.shape[0] == adj.shape[0] == len(nn_) == label.shape[0] == c.B
    assert adj.shape[1] == HC.level_nodes(c)[0] and x.shape[2] == HC.F
    got = _got64(name)
    assert [got[f"emb{j}"].shape[1] for j in range(c.P + 1)] == HC.level_nodes(c)
    assert all(got[f"argmax{j}"].shape == (c.B, HC.readout_width(c)) for j in range(c.P + 1))
    if c.fam == "P":
        assert model.assign_dims == HC.level_nodes(c)[1:] and HC.level_nodes(c)[-1] == c.n
        assert int(nn_.max()) > int(nn_.min()) or c.B == 1 or c.n == 1, "the batch is ragged"
    else:
        assert model.concat == c.concat and got["emb0"].shape[2] == c.H * (c.L - 1) + c.E


@pytest.mark.parametrize("name", HC.NAMES)
def test_the_seed_keeps_the_head_off_the_relu_kink(name):
    c = BY[name]
    _, params, _, _, _, label = _built(name)
    r64 = HC.head_alone(c, params, label, _got64(name), torch.float64)
    assert len(r64["pre"]) == len(c.hidden)
    for i, t in enumerate(r64["pre"]):
        assert float(t.abs().min()) >= 1e-5, \
            f"hidden pre-activation {i} is {float(t.abs().min()):.3e} from ReLU's kink: choose another seed"


@pytest.mark.parametrize("name", HC.NAMES)
def test_the_seed_keeps_the_whole_model_conditioned(name):
    """Check (3) of the GPU test, with fp32 torch on the CPU in the GPU's place, has room: a case whose own reference
    cannot meet tests/parity.py's tolerances would test the conditioning of the model, not the scatter."""
    c = BY[name]
    _, params, x, adj, nn_, label = _built(name)
    win = HC.winners(c, HC.oracle_got(c, params, x, adj, nn_, torch.float32))
    g32 = HC.end_to_end(c, params, x, adj, nn_, label, win, torch.float32)[2]
    g64 = HC.end_to_end(c, params, x, adj, nn_, label, win, torch.float64)[2]
    ratio, k = HC.parity_ratio(g64, g32)
    assert ratio <= 0.75, f"{k}: fp32 on the CPU is at {ratio:.2f} of the parity tolerance: choose another seed"


def test_the_tie_case_has_identical_rows_in_the_zeroed_block():
    c = BY["p_tie"]
    z = _got64("p_tie")["emb1"]
    blk = z[:, :, c.H * (c.L - 1):]
    assert blk.shape[2] == c.E and c.n > 1 and float(blk.abs().min()) > 0
    assert torch.equal(blk, blk[:, :1].expand_as(blk)), "rows of the zeroed block differ"
    assert int(_got64("p_tie")["argmax1"][:, c.H * (c.L - 1):].abs().max()) == 0
    rest = z[:, :, :c.H * (c.L - 1)]
    assert not torch.equal(rest, rest[:, :1].expand_as(rest))


def test_the_negative_maximum_case_has_a_column_a_masked_row_wins():
    c = BY["p_neg"]
    _, _, x, _, nn_, _ = _built("p_neg")
    got = _got64("p_neg")
    z = got["emb0"]
    real = torch.arange(z.shape[1]).view(1, -1, 1) < torch.as_tensor(nn_).view(-1, 1, 1)
    top_real = torch.where(real, z, torch.full_like(z, -float("inf"))).max(dim=1)[0]
    short = torch.as_tensor(nn_).view(-1, 1) < z.shape[1]
    hit = (top_real < -1e-3) & short
    assert int(hit.sum()) >= 1, "no level-0 column has a negative maximum over the real nodes"
    assert torch.equal(got["argmax0"] < 0, (top_real < 0) & short)
    assert int(nn_.min()) >= 1


def test_the_predict_tie_logits_equal_the_bias_exactly():
    c = BY[HC.PREDICT_TIE]
    assert c.C == 3 and c.fwd == "fused" and HC.PREDICT_TIE_BIAS[1] == HC.PREDICT_TIE_BIAS[2] > HC.PREDICT_TIE_BIAS[0]
    _, params, x, adj, nn_, label = HC.build(HC.PREDICT_TIE, predict_tie=True)
    for dtype in (torch.float64, torch.float32):
        y = HC.end_to_end(c, params, x, adj, nn_, label, None, dtype)[0]
        assert torch.equal(y, torch.tensor(HC.PREDICT_TIE_BIAS).to(dtype).expand_as(y))
    assert torch.equal(y.max(dim=1)[1], torch.ones(c.B, dtype=torch.int64))          # first index on the tie


@pytest.mark.parametrize("name", HC.NAMES)
def test_a_correct_fp32_implementation_meets_the_bound_and_nothing_is_left_out(name):
    """The head check of the GPU test, with the fp32 CPU oracle's whole-model step in the GPU's place."""
    c = BY[name]
    _, params, x, adj, nn_, label = _built(name)
    got = HC.oracle_got(c, params, x, adj, nn_, torch.float32)
    y, _, grads = HC.end_to_end(c, params, x, adj, nn_, label, HC.winners(c, got), torch.float32)
    got["ypred"] = y
    got.update({"grad." + k: g for k, g in grads.items()})
    rows = HC.head_figures(c, params, label, got)
    assert [r[0] for r in rows] == ["ypred"] + ["grad." + k for k in HC.head_names(params)]
    assert len(rows) == 1 + 2 * (len(c.hidden) + 1)
    for k, err, e_ref, bound, scale in rows:
        assert e_ref == e_ref and e_ref < float("inf") and 0 < bound < float("inf") and scale > 0, (k, e_ref, bound)
    assert not HC.failures(rows), HC.failures(rows)


@pytest.mark.parametrize("name", ["p_n5_rw13_h3_5", "p_pool2_rw21", "p_n65_rw64_deep", "b_b32", "b_d4097"])
def test_gradients_left_to_rounding_are_named_by_rule(name):
    c = BY[name]
    model = _built(name)[0]
    loose = set(HC.loose_names(model, c))
    assert all(k.endswith(".bias") and "pred_model" not in k for k in loose)
    last = {"grad." + k + ".bias" for k in _last_level_keys(c)}
    graph_bias = {"grad." + k for k, _ in model.named_parameters() if k.endswith(".bias") and "pred_model" not in k}
    assert loose == (graph_bias if HC.last_level_tier(c) == "generic" else graph_bias - last)


def _last_level_keys(c):
    """state_dict prefixes of the last level's embedding stack."""
    if c.fam == "B":
        return SC.stack_keys(HC.sc_case(c))
    return O.level_keys(c.P - 1, c.P, c.L)[0]
