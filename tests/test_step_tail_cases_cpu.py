"""The inputs and bounds of tests/test_gpu_step_tail.py, the part that needs no GPU: for every case a plain fp32
evaluation of the kernel's formula lies within the derived bound of the float64 reference, and every seeded mistake —
the errors the bounds exist to notice — exceeds the bound by at least 2x on at least one case of its family (the cases
that ADAM_SEPARATES names by more than the factor it states).  Then the argument checks of the entries, which return
before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

from graph_pooling_amd import _lib
from tests import csr_weights_cases as WC
from tests import step_tail_cases as SC

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _ratios(got, ref, names=None):
    return {k: SC.worst(got[k], *ref[k]) for k in (names or ref)}


# ------------------------------------------------------------------ cross entropy
def test_ce_table_holds_the_shapes_scales_and_label_forms():
    cases = SC.ce_cases()
    assert len({c.id for c in cases}) == len(cases)
    assert {(c.B, c.C, c.scale) for c in cases} >= {(B, Cc, s) for B, Cc in SC.CE_SHAPES for s in SC.CE_SCALES}
    assert {c.labels for c in cases} == {"random", "first", "last"} and any(c.equal_row for c in cases)
    for c in cases:
        logits, label = SC.ce_inputs(c)
        assert logits.dtype == np.float32 and label.dtype == np.int64
        assert label.min() >= 0 and label.max() < c.C
        if c.labels != "random":
            assert (label == (0 if c.labels == "first" else c.C - 1)).all()
        if c.equal_row:
            assert (logits[c.B // 2] == logits[c.B // 2, 0]).all()


@pytest.mark.parametrize("c", SC.ce_cases(), ids=lambda c: c.id)
def test_ce_fp32_emulation_is_within_the_bound(c):
    logits, label = SC.ce_inputs(c)
    for dloss in SC.CE_DLOSS:
        ref = SC.ce_ref(logits, label, dloss)
        r = _ratios(SC.ce_emulate(logits, label, dloss), ref)
        assert max(r.values()) <= 1.0, r
        assert all(np.isfinite(b).all() and (b > 0).all() for _, b in ref.values())


@pytest.mark.parametrize("mistake,output", zip(SC.CE_MISTAKES, ("loss", "loss", "dunit")))
def test_ce_bounds_reject_each_seeded_mistake(mistake, output):
    hit = {}
    for c in SC.ce_cases():
        logits, label = SC.ce_inputs(c)
        ref = SC.ce_ref(logits, label)
        hit[c.id] = _ratios(SC.ce_emulate(logits, label, mistake=mistake), ref, [output])[output]
    assert max(hit.values()) >= 2.0, (mistake, hit)
    if mistake == "no max subtraction":                  # fp32 overflows at scale 90 where float64 does not
        big = [c for c in SC.ce_cases() if c.scale == 90.0 and c.B * c.C >= 15]
        assert big and all(hit[c.id] >= 2.0 for c in big), hit
        with np.errstate(all="ignore"):
            for c in big:
                l64 = SC.ce_inputs(c)[0].astype(np.float64)
                assert np.isfinite(np.log(np.exp(l64).sum(axis=1))).all()
    if mistake == "d_ypred_unit without / B":            # every batch of more than one graph
        assert all(v >= 2.0 for k, v in hit.items() if not k.startswith("B=1 ")), hit


# ------------------------------------------------------------------ clip + Adam
def test_adam_table_holds_the_sizes_states_and_step_counts():
    cases = SC.adam_cases()
    assert len({c.id for c in cases}) == len(cases)
    assert {c.n for c in cases if c.state == "plain"} >= set(SC.ADAM_SIZES) >= {1, 63, 64, 65, 255, 256, 257, 65280, 65281,
                                                                               65536, 65537, 196613}
    assert {c.t for c in cases} == set(SC.ADAM_STEPS) | {3}
    for n in SC.ADAM_STATE_SIZES:
        assert {c.state for c in cases if c.n == n} == set(SC.ADAM_STATES)
    wgs = lambda n: min((n + 255) // 256, SC.OPT_WGS)
    assert wgs(65280) == 255 and wgs(65281) == 256 and math.ceil(65536 / (256 * 256)) == 1 \
        and math.ceil(65537 / (256 * 256)) == 2                       # the launch's size edges are in ADAM_SIZES
    for c in cases:
        x = SC.adam_inputs(c)
        assert (x["v"] >= 0).all() and np.abs(x["g"]).max() < 2.0 ** 40
        assert all(x[k].dtype == np.float32 and x[k].shape == (c.n,) for k in "pgmv")
    x = SC.adam_inputs(next(c for c in cases if c.id == "n=1000 small-norm t=3"))
    assert 2e-4 < np.linalg.norm(x["g"].astype(np.float64)) < 4e-4


@pytest.mark.parametrize("c", SC.adam_cases(), ids=lambda c: c.id)
def test_adam_fp32_emulation_is_within_the_bound(c):
    x = SC.adam_inputs(c)
    max_norm = SC.ADAM_STATES[c.state][1]
    ref = SC.adam_ref(x, c.t, max_norm)
    got = SC.adam_emulate(x, c.t, max_norm)
    r = _ratios(got, ref)
    assert max(r.values()) <= 1.0, r
    if max_norm <= 0:
        assert np.array_equal(got["g"], x["g"]) and not ref["g"][1].any()
    if c.state == "active":
        assert float(ref["g"][0].std()) < 0.1 * float(x["g"].std())       # the clip is active
    if c.state == "loose" or (c.state == "plain" and c.n <= 257):
        assert np.array_equal(ref["g"][0], x["g"].astype(np.float64))     # and here it is not
        assert np.array_equal(got["g"], x["g"])


@pytest.mark.parametrize("mistake", SC.ADAM_MISTAKES)
def test_adam_bounds_reject_each_seeded_mistake(mistake):
    state, factor = SC.ADAM_SEPARATES[mistake]
    named = [c for c in SC.adam_cases() if c.state == state and c.n in SC.ADAM_STATE_SIZES and c.t == 3]
    assert sorted(c.n for c in named) == sorted(SC.ADAM_STATE_SIZES), (mistake, "its separating cases left the table")
    for c in named:
        x = SC.adam_inputs(c)
        max_norm = SC.ADAM_STATES[c.state][1]
        r = _ratios(SC.adam_emulate(x, c.t, max_norm, mistake), SC.adam_ref(x, c.t, max_norm))
        assert max(r.values()) >= max(factor, 2.0), (mistake, c.id, r)


def test_what_the_other_states_can_and_cannot_tell_apart():
    """What the fp32 tolerance of tests/test_gpu_optim.py could not see: with ||g|| of order 1 or more the 1e-6 of the
    clip coefficient moves nothing by more than the roundings the bound allows, so the "small-norm" state is the one that
    carries that check."""
    mistake = "clip coefficient without the 1e-6"
    for c in SC.adam_cases():
        if c.state == "small-norm":
            continue
        x = SC.adam_inputs(c)
        max_norm = SC.ADAM_STATES[c.state][1]
        r = max(_ratios(SC.adam_emulate(x, c.t, max_norm, mistake), SC.adam_ref(x, c.t, max_norm)).values())
        assert r <= 1.0, (mistake, c.id, r)
    for c in SC.adam_cases():                            # the t - 1 mistake: any early step shows it
        if c.t <= 10:
            x = SC.adam_inputs(c)
            max_norm = SC.ADAM_STATES[c.state][1]
            r = _ratios(SC.adam_emulate(x, c.t, max_norm, "bias corrections of t - 1"), SC.adam_ref(x, c.t, max_norm))
            assert r["p"] >= 2.0, (c.id, r)


# ------------------------------------------------------------------ mean aggregation
@pytest.fixture(scope="module")
def agg():
    g = WC.agg_graph()
    assert WC.degrees(g)[:len(WC.AGG_DEGREES)].tolist() == list(WC.AGG_DEGREES)
    return g, SC.dense01(g), SC.csr_arrays(g)


@pytest.mark.parametrize("n_rows", SC.MEAN_NROWS)
def test_mean_fp32_emulation_is_within_the_bound(agg, n_rows):
    g, a, (ip, ix) = agg
    for feat in WC.AGG_FEATS:
        x = SC.mean_inputs(g.n, n_rows, feat)
        for beta in (0.0, 1.0):
            ref, bound = SC.mean_fwd_ref(a, x["x"], n_rows, beta, x["old"])
            got = SC.mean_fwd_emulate(ip, ix, x["x"], n_rows, beta, x["old"])
            assert SC.worst(got, ref, bound) <= 1.0, (feat, beta)
            deg0 = WC.degrees(g)[:n_rows] == 0
            assert deg0[0] and np.array_equal(np.isnan(ref), np.repeat(deg0[:, None], feat, axis=1))
        ref, bound = SC.mean_bwd_ref(a, x["dout"], n_rows, x["dt_old"])
        assert np.isfinite(ref).all()
        assert SC.worst(SC.mean_bwd_emulate(ip, ix, x["dout"], n_rows, x["dt_old"]), ref, bound) <= 1.0, feat


@pytest.mark.parametrize("mistake", SC.MEAN_MISTAKES)
def test_mean_bounds_reject_each_seeded_mistake(agg, mistake):
    g, a, (ip, ix) = agg
    n_rows = g.n
    for feat in WC.AGG_FEATS:
        x = SC.mean_inputs(g.n, n_rows, feat)
        ref, bound = SC.mean_fwd_ref(a, x["x"], n_rows)
        got = SC.mean_fwd_emulate(ip, ix, x["x"], n_rows, mistake=mistake)
        rows = ~np.isnan(ref[:, 0])
        per_row = np.array([SC.worst(got[r], ref[r], bound[r]) if rows[r] else 0.0 for r in range(n_rows)])
        assert per_row.max() >= 2.0, (mistake, feat)
        deg = WC.degrees(g)
        if mistake == "tail of the 4-way unroll dropped":         # every row whose degree is no multiple of 4
            assert (per_row[:9] >= 2.0).tolist() == [d % 4 != 0 for d in WC.AGG_DEGREES], per_row[:9]
        if mistake == "only the first 64-id chunk read":          # the rows of 65 and 129 entries, and only those
            assert (per_row >= 2.0).tolist() == (deg > 64).tolist(), per_row[:9]
    if mistake == "1 / (deg + 1)":
        x = SC.mean_inputs(g.n, n_rows, 65)
        ref, bound = SC.mean_bwd_ref(a, x["dout"], n_rows, x["dt_old"])
        assert SC.worst(SC.mean_bwd_emulate(ip, ix, x["dout"], n_rows, x["dt_old"], mistake), ref, bound) >= 2.0


def test_mean_integer_grid_is_exact_in_fp32():
    g = SC.grid_graph()
    a, (ip, ix) = SC.dense01(g), SC.csr_arrays(g)
    deg = WC.degrees(g)
    assert sorted(set(deg.tolist())) == list(SC.GRID_DEGREES)
    rng = np.random.default_rng(5)
    x, dout, old = (rng.integers(-8, 9, (g.n, 65)).astype(np.float32) for _ in range(3))
    ref, bound = SC.mean_fwd_ref(a, x, g.n)
    assert np.array_equal(SC.mean_fwd_emulate(ip, ix, x, g.n).astype(np.float64), ref)
    ref, _ = SC.mean_bwd_ref(a, dout, g.n, old)
    assert np.array_equal(SC.mean_bwd_emulate(ip, ix, dout, g.n, old).astype(np.float64), ref)


# ------------------------------------------------------------------ argument checks (no launch, no device)
def test_entries_report_argument_errors_without_a_gpu(lib):
    buf = (C.c_float * 1024)()
    idx = (C.c_longlong * 64)()
    ints = (C.c_int * 64)()
    ws = (C.c_char * 4096)()
    p, y, i, w = C.addressof(buf), C.addressof(idx), C.addressof(ints), C.addressof(ws)
    err = lambda: lib.dp_last_error_string().decode()

    assert lib.dp_cross_entropy_fwd(None, y, p, p, 4, 3, None) == INVALID and "NULL" in err()
    assert lib.dp_cross_entropy_fwd(p, None, p, p, 4, 3, None) == INVALID and "NULL" in err()
    assert lib.dp_cross_entropy_fwd(p, y, None, p, 4, 3, None) == INVALID and "NULL" in err()
    assert lib.dp_cross_entropy_fwd(p, y, p, p, 0, 3, None) == INVALID and "positive" in err()
    assert lib.dp_cross_entropy_fwd(p, y, p, None, 4, 0, None) == INVALID and "positive" in err()
    assert lib.dp_cross_entropy_bwd(None, y, None, p, 4, 3, None) == INVALID and "NULL" in err()
    assert lib.dp_cross_entropy_bwd(p, y, None, None, 4, 3, None) == INVALID and "NULL" in err()
    assert lib.dp_cross_entropy_bwd(p, y, None, p, 4, -1, None) == INVALID and "positive" in err()
    fwd = lambda ypred=p, label=y, out=p, prob=p, B=4, Cc=3: lib.dp_loss_forward(
        ypred, label, None, None, None, None, out, prob, None, B, Cc, 0, 0, 0, w, 4096, None)
    assert fwd(ypred=None) == INVALID and fwd(label=None) == INVALID and fwd(out=None) == INVALID
    assert fwd(prob=None) == INVALID and "NULL" in err()
    assert fwd(B=0) == INVALID and fwd(Cc=0) == INVALID and "positive" in err()
    assert lib.dp_loss_forward(p, y, None, None, None, None, p, p, None, 4, 3, 0, 0, 1, w, 4096, None) == INVALID \
        and "linkpred" in err()
    assert lib.dp_loss_forward(p, y, None, None, None, None, p, p, None, 4, 3, 0, 0, 0, w, 8, None) != 0   # workspace
    bwd = lambda prob=p, label=y, B=4, Cc=3: lib.dp_loss_backward(prob, label, None, None, None, None, None, p, None, B,
                                                                 Cc, 0, 0, 0, w, 4096, None)
    assert bwd(prob=None) == INVALID and bwd(label=None) == INVALID and "NULL" in err()
    assert bwd(B=0) == INVALID and bwd(Cc=-2) == INVALID and "positive" in err()

    step = lambda params=p, n=4, t=1, b1=0.9, b2=0.999, wsb=4096: lib.dp_clip_adam_step(
        params, p, p, p, n, t, 1e-3, b1, b2, 1e-8, 2.0, None, w, wsb, None)
    assert step(t=0) == INVALID and "1-based" in err()
    assert step(t=-3) == INVALID
    assert step(params=None) == INVALID and "NULL" in err()
    assert step(b1=1.0) == INVALID and "[0, 1)" in err()
    assert step(b2=-0.1) == INVALID and step(b2=1.5) == INVALID
    assert step(n=-1) == INVALID
    assert step(wsb=8) != 0 and "workspace" in err()
    counted = lambda params=p, counter=i, b1=0.9, wsb=4096, n=4: lib.dp_clip_adam_step_counted(
        params, p, p, p, n, counter, 1e-3, b1, 0.999, 1e-8, 2.0, None, w, wsb, None)
    assert counted(counter=None) == INVALID and "NULL" in err()
    assert counted(params=None) == INVALID
    assert counted(b1=1.0) == INVALID and "[0, 1)" in err()
    assert counted(n=-1) == INVALID
    assert counted(wsb=8) != 0 and "workspace" in err()
    assert lib.dp_clip_adam_workspace_bytes() >= 4 * SC.OPT_WGS

    for name in ("dp_mean_aggregate_fwd", "dp_mean_aggregate_bwd"):
        f = getattr(lib, name)
        assert f(None, 4, i, i, p, 4, 4, 4, None) == INVALID and "NULL" in err()
        assert f(p, 4, None, i, p, 4, 4, 4, None) == INVALID and f(p, 4, i, None, p, 4, 4, 4, None) == INVALID
        assert f(p, 4, i, i, None, 4, 4, 4, None) == INVALID and "NULL" in err()
        assert f(p, 4, i, i, p, 4, 0, 4, None) == INVALID and "positive" in err()
        assert f(p, 4, i, i, p, 4, 4, 0, None) == INVALID and "positive" in err()
    assert lib.dp_csr_aggregate(p, 4, i, i, None, 4, 4, 4, 1, 0.0, None) == INVALID and "NULL" in err()
    assert lib.dp_csr_aggregate(p, 4, i, i, p, 4, -1, 4, 1, 0.0, None) == INVALID and "positive" in err()
