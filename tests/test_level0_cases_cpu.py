"""The cases of tests/test_gpu_level0_matrix.py (tests/level0_cases.py), checked without a GPU: every row's plan, rows per
workgroup and quoted count follow from the restated envelope at 256 CUs; the `pp` rows cover every depth, tile count,
register slot, combine slot, block size and extent the kernels distinguish, and every rejected edge has a twin on the
edge; each model has the stacks the table says; every seed keeps the fp64 reference off ReLU's kink and the fp32 oracle's
winners on the fp64 maxima; and the bound of checks (i) and (ii) is one a correct fp32 implementation (the fp32 CPU
oracle, fed through the GPU test's own comparison) meets."""
import functools

import pytest
import torch

from tests import level0_cases as LC

PP = [c for c in LC.CASES if c.plan == "pp"]


@pytest.mark.parametrize("name", LC.NAMES)
def test_plan_and_rows_follow_from_the_restated_envelope(name):
    c = LC.CASE[name]
    r = LC.plan(c)
    assert (r["plan"], r["rows"]) == (c.plan, c.rows)
    if c.plan == "pp":
        # the forward (sized with the readout merge) and the backward (without it) cut the rows alike
        assert r["fwd_rows"] == r["rows"] and r["fwd_bytes"] <= 159 * 1024 and r["bwd_bytes"] <= 160 * 1024
    for what, value in LC.QUOTED.get(name, {}).items():
        assert r[what] == value, (what, r[what], value)


def test_the_quoted_relations_hold():
    r = {n: LC.plan(LC.CASE[n]) for n in LC.NAMES}
    assert r["p_k64"]["bwd_staged"] > r["p_k64"]["ra"]                      # why its backward is per-phase
    assert r["b_w64"]["bwd_bytes"] > r["b_w64"]["fwd_bytes"]
    assert r["p_rb48_w"]["fwd_bytes"] <= 162816 < r["p_rb48_w"]["fwd_bytes"] + 4 * 1024
    assert LC.CASE["p_k1"].K == 1 and set(LC.DROP_ZERO) == {"p_k1"} and len(LC.DROP_ZERO) <= 2
    assert not set(LC.TWO_ASSOC) - set(LC.NAMES)


def test_fewer_cus_move_the_plan_as_the_formula_says():
    """The GPU test recomputes the plan for the device's CU count: B * ceil(N / RB) <= CUs picks the rows."""
    c = LC.CASE["p_b64"]
    assert [LC.plan(c, cus)["rows"] for cus in (256, 255, 128, 127, 64, 63)] == [16, 32, 32, 64, 64, 0]


def _highest_slot(c):
    return (max(w for s in LC.stacks(c) for w in s[1:]) - 1) // 16


def _tiles(c):
    st = LC.stacks(c)
    return {(sum(s[l + 1] for s in st) + 15) // 16 for l in range(c.L)}


def _segments(c):
    return (c.N + 511) // 512


def test_the_pp_cases_cover_every_class():
    assert len(set(LC.NAMES)) == len(LC.NAMES)
    assert {1, 2, 3, 4, 8} <= {c.L for c in PP}
    assert set().union(*[_tiles(c) for c in PP]) >= {1, 2, 3, 4, 5, 6}
    assert {_highest_slot(c) for c in PP} == {0, 1, 2, 3}
    for fam in "PB":
        assert {True, False} <= {c.bn for c in PP if c.fam == fam}
        assert {True, False} <= {c.bias for c in PP if c.fam == fam}
    assert {"B", "S"} <= {c.fam for c in PP}                               # G = 1 with and without the max readout
    assert {16, 32, 48, 64} <= {c.rows for c in PP if c.fam == "P"}
    assert {16, 32, 48, 64} <= {c.rows for c in PP if c.fam == "B"}
    assert {1, 16, 17, 33, 49, 64} <= {c.B for c in PP if c.fam == "P"}
    assert {1, 2, 3} <= {_segments(c) for c in PP}
    assert any(c.N % c.rows == 4 for c in PP if c.fam == "P") and any(c.N % c.rows == 4 for c in PP if c.fam == "B")
    assert {1, 32, 33, 48, 49, 64} <= {c.K for c in PP if c.fam == "P"}
    assert any(c.H != c.E and c.E != c.Ha and c.H != c.Ha for c in PP if c.fam == "P")
    assert any(c.Fa for c in LC.CASES)
    # every adjacency kind on every width / joint-width case that runs the pair, `sym` alone elsewhere
    for c in LC.CASES:
        want = LC.KINDS if (c.name.startswith(("p_w", "p_ct")) and c.plan == "pp") else ("sym",)
        assert tuple(k for n, k in LC.VARIANTS if n == c.name) == want
    assert [c.name for c in LC.CASES if LC.linkpred(c)] == [n for n in LC.NAMES if n.startswith("p_k")]
    for c in LC.CASES:
        if c.B > 20:                                                      # large batches stay cheap
            assert c.N <= 224 and max(c.H, c.E) <= 64, c.name


def test_every_rejected_edge_has_a_twin_on_the_edge():
    gg = [c.name for c in LC.CASES if c.plan == "gg"]
    assert set(LC.TWINS) | {"p_n66"} == set(gg)            # (N % 4: every other case is its twin)
    for out, inside in LC.TWINS.items():
        assert LC.CASE[inside].plan in ("pp", "pg") and LC.CASE[out].fam == LC.CASE[inside].fam
    C = LC.CASE
    assert (C["p_ct97"].H + C["p_ct97"].Ha, C["p_ct96"].H + C["p_ct96"].Ha) == (97, 96)
    assert (C["p_h65"].H, C["p_ct96_l2"].H, C["b_w65"].H, C["b_e65"].E, C["b_w64"].H) == (65, 64, 65, 65, 64)
    assert (C["p_k65"].K, C["p_k64"].K, C["p_b65"].B, C["p_b64"].B) == (65, 64, 65, 64)
    assert (C["p_f257"].F, C["p_f256"].F, C["p_f129"].F, C["p_f129"].Fa, C["p_f128"].F) == (257, 256, 129, 128, 128)
    assert C["p_n66"].N % 4 == 2


@functools.lru_cache(maxsize=None)
def _built(name, kind):
    return LC.build(name, kind)


@pytest.mark.parametrize("name", LC.NAMES)
def test_the_model_has_the_stacks_the_table_says(name):
    c = LC.CASE[name]
    model, params, x, ax, adj, nn_, label = _built(name, "sym")
    sd = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    st = LC.stacks(c)
    groups = [LC.emb_keys(c)] + ([LC.pool_keys(c)[1]] if c.fam == "P" else [])
    for keys, dims in zip(groups, st):
        assert [sd[keys[0] + ".weight"][0]] + [sd[k + ".weight"][1] for k in keys] == dims and len(keys) == c.L
        assert all((k + ".bias" in sd) == c.bias for k in keys)
    assert x.shape == (c.B, c.N, c.F) and adj.shape == (c.B, c.N, c.N) and len(nn_) == c.B
    assert int(nn_[LC.full_graph(c)]) == c.N
    if c.B >= 3 and (c.bias or c.fam != "B"):
        assert int(nn_.min()) == 1
    if c.fam == "P":
        assert model.assign_dims == [c.K] and ax.shape[2] == (c.Fa or c.F) and model.linkpred == LC.linkpred(c)
        assert bool(model._flags()) == c.bn
    else:
        assert model.bn == c.bn


@pytest.mark.parametrize("name,kind", LC.VARIANTS, ids=LC.IDS)
def test_the_adjacency_is_of_its_kind(name, kind):
    c = LC.CASE[name]
    adj = _built(name, kind)[4]
    sym = [bool(torch.equal(a, a.t())) for a in adj]
    exact = bool(torch.equal(adj, adj.bfloat16().float()))
    if kind == "sym":
        assert all(sym) and exact and set(adj.unique().tolist()) <= {0.0, 1.0}
    elif kind == "dir":
        assert exact and [int(s) for s in sym] == LC.expected_verdicts(c, kind)
        i, j = (adj[LC.full_graph(c)] != adj[LC.full_graph(c)].t()).nonzero()[0].tolist()
        assert max(i, j) // 64 == (c.N - 1) // 64 and min(i, j) < 16          # last row block, first row block
    else:
        assert all(sym) and not exact and LC.expected_verdicts(c, kind) == [0] * c.B


@pytest.mark.parametrize("name,kind", LC.VARIANTS, ids=LC.IDS)
def test_the_seed_keeps_the_reference_off_the_kink_and_the_winners_on_the_maxima(name, kind):
    c = LC.CASE[name]
    rows = LC.conditioning(name, kind)
    assert len(rows) == (c.L - 1) * len(LC.stacks(c))
    for i, lo, hi in rows:
        assert lo > 1e-5 * hi, f"pre-activation {i} sits on a ReLU kink ({lo:.3e} of {hi:.3e}): choose another seed"
    # the fp32 oracle's own arg-max against the fp64 forward
    model, params, x, ax, adj, nn_, label = _built(name, kind)
    f64 = LC.level0_forward(c, params, x, ax, adj, nn_, torch.float64)
    f32 = LC.level0_forward(c, params, x, ax, adj, nn_, torch.float32)
    for j, (z64, z32) in enumerate(zip(f64["z"], f32["z"])):
        LC.check_winners(z64, z32.max(dim=1)[1].int(), f"{name}-{kind} level {j}")
    # ... and with room to spare, in either association
    for j, assoc, gap in LC.winner_gaps(name, kind):
        assert gap <= LC.WINNER_MARGIN, f"level {j}, {assoc}: an fp32 winner sits {gap:.3e} below the fp64 maximum"


@pytest.mark.parametrize("name,kind", LC.VARIANTS, ids=LC.IDS)
def test_a_correct_fp32_implementation_meets_the_bound(name, kind):
    """Checks (i) and (ii) of the GPU test, with the fp32 CPU oracle's step in the GPU's place."""
    c = LC.CASE[name]
    params = _built(name, kind)[1]
    rows = LC.figures(name, kind, LC.oracle_got(name, kind, torch.float32))
    fwd = [r for r in rows if r[0] == "i"]
    bwd = [r for r in rows if r[0] == "ii"]
    assert [r[1] for r in fwd] == list(LC.FWD_KEYS[c.fam])                     # no case is left out of (i)
    if name in LC.DROP_ZERO:
        assert 2 < len(bwd) < 2 + len(params)
    else:
        assert len(bwd) == 2 + len(params)
    first = ["grad." + k for k in LC.level0_names(c, params)]
    kept = [k for k in first if k in {r[1] for r in bwd}]                      # level 0's own parameters come first
    assert [r[1] for r in bwd[:2]] == ["ypred", "loss"] and [r[1] for r in bwd[2:2 + len(kept)]] == kept
    for _, k, err, e_ref, bound, scale in rows:
        assert e_ref == e_ref and e_ref < float("inf") and 0 < bound < float("inf"), (k, e_ref, bound)
    assert not LC.failures(rows), LC.failures(rows)


@pytest.mark.parametrize("name", ["p_w33", "p_b17", "b_w64", "s_l3"])
def test_the_bound_tells_a_wrong_column_from_rounding(name):
    """Defects far smaller than a wrong register slot, column tile or combine slot leaves, put into the fp32 oracle's
    run: the last column of the embedding off by 1e-4 of itself, one weight gradient's last column off by 1e-3, two
    clusters swapped in one row of the assignment."""
    c = LC.CASE[name]
    good = LC.oracle_got(name, "sym", torch.float32)
    assert not LC.failures(LC.figures(name, "sym", good))

    def failed(**changed):
        return {r[1] for r in LC.figures(name, "sym", {**good, **changed}) if not r[2] <= r[4]}

    emb = good["embedding"].clone()
    emb[:, :, -1] *= 1.0 + 1e-4
    assert "embedding" in failed(embedding=emb)
    k = "grad." + LC.emb_keys(c)[0] + ".weight"
    g = good[k].clone()
    g[:, -1] *= 1.0 + 1e-3
    assert k in failed(**{k: g})
    if c.fam == "P":
        s = good["assign"].clone()
        s[LC.full_graph(c), c.N - 1] = s[LC.full_graph(c), c.N - 1].roll(1)       # two clusters swapped in one row
        assert "assign" in failed(assign=s)


def test_the_written_out_forward_is_the_oracles():
    """Family P at L = 1 takes level0_cases.softpool_written_out in place of O.softpool_forward: at L = 3 the two give
    the same fp64 loss and gradients to rounding."""
    c = LC.CASE["p_w17"]
    _, params, x, ax, adj, nn_, label = _built("p_w17", "sym")
    win = [z.max(dim=1)[1].int() for z in LC.level0_forward(c, params, x, ax, adj, nn_, torch.float64)["z"]]
    a = LC.whole_model(c, params, x, ax, adj, nn_, label, win, torch.float64)
    b = LC.whole_model(c, params, x, ax, adj, nn_, label, win, torch.float64, written_out=True)
    assert set(a) == set(b)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-13 * max(1.0, float(a[k].abs().max())), k


@pytest.mark.parametrize("name", ["p_w16", "p_k64", "p_k65", "b_w65", "b_n1028", "s_l3"])
def test_gradients_left_to_rounding_are_named_by_rule(name):
    c = LC.CASE[name]
    model = _built(name, "sym")[0]
    loose = set(LC.loose_names(c, model, c.plan))
    assert all(k.endswith(".bias") for k in loose)
    l0 = {"grad." + k + ".bias" for k in LC.emb_keys(c)}
    l0a = {"grad." + k + ".bias" for k in LC.pool_keys(c)[1] + ["assign_pred"]}
    l1 = {"grad." + k + ".bias" for k in LC.pool_keys(c)[0]}
    want = {"p_w16": set(), "p_k64": l0 | l0a, "p_k65": l0 | l0a | l1, "b_w65": set(), "b_n1028": set(), "s_l3": set()}
    assert loose == want[name]
