"""CPU checks of the aggregation case table (tests/agg_cases.py): every row's recorded plan is dp_adj_aggregate_plan's
answer — the answer of agg_pick, the one function aggregate() and aggregate_rownorm_fwd() of dp_agg.hip decide with (rows
with a knob are asked in a child process that has it set); the tier edges of its rules are where this file says; the
table reaches every launch_agg_rt / launch_aggw / launch_aggw_dma instantiation the source names, with both epilogues
where the form has both; the shapes the issue of each loop asks for are there; the grid inputs have the properties the
exact comparison rests on; a CPU emulation of every form stays inside every bound and equals the grid reference bit for
bit, and each of five defects fails a row of the form it belongs to; the new entries refuse what the kernels' contracts
exclude before any launch."""
import ctypes as C
import os
import re

import pytest
import torch

from graph_pooling_amd import _lib
from tests import agg_cases as AC
from tests import rowop_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_pooling_amd", "csrc", "dp_agg.hip")
F = {name: i for i, name in enumerate(AC.FORMS)}


@pytest.fixture(scope="module")
def lib():
    assert AC.knobs_unset(), "unset %s: the table records the plans of a process without knobs" % (AC.KNOBS,)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _instantiations():
    """The template arguments at every call of the three launchers in dp_agg.hip (TRANS stands for both passes)."""
    src = open(SRC).read()
    panel = {(int(a), int(b), int(c)) for a, b, c in re.findall(r"launch_agg_rt<TRANS, (\d+), (\d+), (\d+)>\(", src)}
    wide = {int(a) for a in re.findall(r"launch_aggw<(\d+)>\(", src)}
    dma = {(int(a), int(b)) for a, b in re.findall(r"launch_aggw_dma<(\d+), (\d+)>\(", src)}
    # no call of a launcher that this reading would miss (the definitions name template parameters, not numbers)
    calls = len(re.findall(r"\blaunch_agg(?:_rt|w|w_dma)<[^>]*>\(q", src))
    assert calls == len(panel) + len(wide) + len(dma), (calls, len(panel), len(wide), len(dma))
    return panel, wide, dma


def test_every_recorded_plan_is_the_launchers(lib):
    rows = [r for r in AC.ROWS if r.kind != "pack"]
    assert set(AC.PLANS) == {r.id for r in rows}
    got = {r.id: AC.plan_of(lib, r) for r in rows if r.env == ""}
    for env in AC.ENVS:                       # one child after another, each under its own timeout
        if env:
            got.update(AC.child_plans(env, timeout=120))
    wrong = [f"{k}: recorded {AC.PLANS[k]}, dp_adj_aggregate_plan {got.get(k)}" for k in AC.PLANS if AC.PLANS[k] != got.get(k)]
    assert not wrong, "\n".join(wrong[:20])


def test_tier_edges_of_the_rules(lib):
    q = lambda *a, **k: AC.query(lib, *a, **k)                                       # noqa: E731
    # the row tile: B ceil(n / 32) at 255 | 256
    assert (q(255, 20, 16).rt, q(256, 20, 16).rt) == (16, 32)
    assert (q(15, 500, 40).rt, q(16, 500, 40).rt) == (16, 32) and q(16, 500, 40).grid == 16 * 16
    assert (q(127, 64, 16, trans=1).rt, q(128, 64, 16, trans=1).rt) == (16, 32)
    # ... unless 32 transposed rows do not fit the 160 KiB: n at 1280 | 1284
    assert (q(256, 1280, 16, trans=1).rt, q(256, 1284, 16, trans=1).rt) == (32, 16)
    assert q(256, 1280, 16, trans=1).lds == 160 * 1024
    # the wide kernel by itself: B ceil(n / 128) at 511 | 512, C <= 128
    assert (q(511, 128, 8, packed=1).form, q(512, 128, 8, packed=1).form) == (F["panel_bf16"], F["wide"])
    assert (q(255, 256, 128, packed=1).form, q(256, 256, 128, packed=1).form) == (F["panel_bf16"], F["wide"])
    assert q(512, 128, 8, packed=1).fallback == _lib.AGG_FB_PANEL and q(512, 128, 8).form == F["panel_f32"]
    # C at 128 | 129 and 320 | 321
    assert (q(2, 128, 128, packed=1).form, q(2, 128, 129, packed=1).form) == (F["panel_bf16"], F["wide_dma"])
    assert (q(2, 128, 128).form, q(2, 128, 129).form) == (F["panel_f32"], F["gemm_f32"])
    p320, p321 = q(2, 128, 320, packed=1), q(2, 128, 321, packed=1)
    assert (p320.form, p320.ct, p320.rt, p320.fallback, p320.split) == (F["wide_dma"], 20, 4, _lib.AGG_FB_GEMM, 1)
    assert (p321.form, p321.split) == (F["gemm_f32"], 0)
    # the packed operand: n at 124 | 128, and its LDS limit at 3584 | 3588
    assert [(p.form, p.split) for p in (q(2, 124, 16, packed=1), q(2, 128, 16, packed=1))] == \
        [(F["panel_f32"], 0), (F["panel_bf16"], 1)]
    assert [q(1, n, 16, packed=1).form for n in (3584, 3588)] == [F["panel_bf16"], F["panel_f32"]]
    # the split-bf16 GEMM for a general adjacency at a big batch: C < 48 stays on the panel kernel; widths the split
    # kernel has no tile for stay too; the fused entry declines where the plain one diverts; beta = 0.5 never diverts
    assert [q(256, 1024, c).form for c in (47, 48, 64, 65, 79, 80, 128)] == \
        [F["panel_f32"], F["gemm_split_bf16"], F["gemm_split_bf16"], F["panel_f32"], F["panel_f32"], F["gemm_split_bf16"],
         F["gemm_split_bf16"]]
    assert [q(256, 1024, c, fused=1).declines for c in (47, 48, 79, 80)] == [0, 1, 0, 1]
    assert q(256, 1024, 80, beta=0.5).form == F["panel_f32"] and q(256, 1024, 80, beta=1.0).form == F["gemm_split_bf16"]
    assert q(256, 1024, 80, packed=1).form == F["wide"]
    assert (q(31, 1024, 80).form, q(32, 1024, 80).form) == (F["panel_f32"], F["gemm_split_bf16"])       # 256 tiles
    assert (q(256, 92, 80).form, q(256, 96, 80).form) == (F["panel_f32"], F["gemm_split_bf16"])
    # a product too wide for the panel kernel takes the split kernel by the same rule
    assert (q(256, 1024, 130).form, q(2, 1024, 130).form) == (F["gemm_split_bf16"], F["gemm_f32"])
    # the 160 KiB of the transposed panel: n at 2560 | 2564; the NN panel has no such limit
    assert [q(1, n, 16, trans=1).form for n in (2560, 2564)] == [F["panel_f32"], F["gemm_f32"]]
    assert q(1, 2560, 16, trans=1).lds == 160 * 1024 and q(1, 4096, 16).form == F["panel_f32"]
    assert q(1, 2560, 16, fused=1, trans=1).form == F["panel_f32"]          # the fused entry is NN whatever `trans` says
    # n % 4, n < 4, the alignment of A
    assert [q(2, n, 16).form for n in (3, 4, 66, 67, 68)] == [F["gemm_f32"], F["panel_f32"], F["gemm_f32"], F["gemm_f32"],
                                                              F["panel_f32"]]
    assert [q(2, 64, 16, misalign=m).form for m in (0, 4, 8, 12)] == [F["panel_f32"]] + [F["gemm_f32"]] * 3
    assert q(2, 64, 16, fused=1, misalign=4).declines == 1 and q(2, 67, 16, fused=1).declines == 1
    # a wide form's fallback: the predicated panel kernel where it takes the shape, the predicated GEMM otherwise
    assert q(512, 128, 8, packed=1, misalign=4).fallback == _lib.AGG_FB_GEMM
    out = (C.c_int * _lib.AGG_PLAN_INTS)()
    assert lib.dp_adj_aggregate_plan(1, 4, 4, 0, 0, 0, 16, 0.0, out) == -1 and b"a_misalign" in lib.dp_last_error_string()
    assert lib.dp_adj_aggregate_plan(1, 4, 4, 0, 0, 0, 0, 0.0, None) == -1
    assert lib.dp_adj_aggregate_plan(0, 4, 4, 0, 0, 0, 0, 0.0, out) == -1


def test_geometry_restated_agrees_with_the_query(lib):
    """CT, tiles, workgroups and LDS bytes of every form, restated from the kernels' layouts."""
    def panel_lds(trans, n, ct, rt):
        kp = n if trans else min(n, 1024)
        panel = ((n + 15) // 16) * 16 * rt if trans else rt * (((kp + 255) // 256) * 256 + 4)
        pk = (rt * (((n + 511) // 512) * 512 + 8) * 2 + 3) // 4
        fl = (max(panel, pk) + 3) & ~3
        return 4 * max(fl, 5 * rt * (16 * ct + 1))
    for r in AC.ROWS:
        if r.kind == "pack":
            continue
        p = AC.PLANS[r.id]
        form = AC.form_name(p)
        trans = r.trans if r.kind == "plain" else 0
        if form.startswith("panel"):
            assert p.ct == (r.C + 15) // 16 and p.rt in (16, 32) and p.tiles == (r.n + p.rt - 1) // p.rt
            assert p.grid == p.tiles * r.B and p.lds == panel_lds(trans, r.n, p.ct, p.rt) <= 160 * 1024
            assert p.fallback == _lib.AGG_FB_NONE and p.split == (form == "panel_bf16")
        elif form == "wide":
            assert p.ct == (r.C + 15) // 16 <= 8 and p.rt == 4 and p.tiles == (r.n + 127) // 128
            assert p.grid == p.tiles * r.B and p.lds == 2 * 3 * p.ct * 2 * 1024 and p.split == 1
        elif form == "wide_dma":
            ct = (r.C + 15) // 16
            assert p.ct == ct + ct % 2 and p.rt == (8 if p.ct <= 18 else 4) and p.tiles == (r.n + 32 * p.rt - 1) // (32 * p.rt)
            assert p.grid == p.tiles * r.B and p.lds == (2 * 3 * p.ct * 512 + 3 * p.rt * 1024) * 2 <= 160 * 1024
        else:
            assert p[1:6] == (0, 0, 0, 0, 0) and p.fallback == _lib.AGG_FB_NONE
        if p.fallback == _lib.AGG_FB_PANEL:
            assert p.fb_ct == (r.C + 15) // 16 and p.fb_tiles == (r.n + p.fb_rt - 1) // p.fb_rt
            assert p.fb_grid == p.fb_tiles * r.B and p.fb_lds == panel_lds(trans, r.n, p.fb_ct, p.fb_rt)
        else:
            assert p[7:12] == (0, 0, 0, 0, 0)
        assert not p.declines, r.id


def test_table_reaches_every_instantiation():
    panel, wide, dma = _instantiations()
    assert panel == {(ct, rt, 4) for ct in range(1, 9) for rt in (16, 32)}
    assert wide == set(range(1, 9)) and dma == {(10, 8), (12, 8), (14, 8), (16, 8), (18, 8), (20, 4)}
    rows = [(r, AC.PLANS[r.id]) for r in AC.ROWS if r.kind != "pack" and not r.o.get("cpu_only")]
    for ct, rt, _ in sorted(panel):
        for loop in ("panel_f32", "panel_bf16"):
            hit = [r for r, p in rows if AC.form_name(p) == loop and (p.ct, p.rt) == (ct, rt)]
            if loop == "panel_f32":           # the fp32 loop: both passes with the plain epilogue, the tail behind NN
                assert {(r.kind, r.trans) for r in hit} == {("plain", 0), ("plain", 1), ("fused", 0)}, (ct, rt, loop)
            else:                             # the bf16 loop of the same kernel: every CT, both epilogues
                assert {r.kind for r, p in rows if AC.form_name(p) == loop and p.ct == ct} == {"plain", "fused"}, (ct, loop)
        # ... and as the predicated fallback behind a wide form
    assert {(r.kind, r.trans) for r, p in rows if p.fallback == _lib.AGG_FB_PANEL and r.flagged} == \
        {("plain", 0), ("plain", 1), ("fused", 0)}
    for ct in sorted(wide):
        hit = [r for r, p in rows if AC.form_name(p) == "wide" and p.ct == ct]
        assert {r.kind for r in hit} == {"plain", "fused"} and {r.trans for r in hit} == {0, 1}, ct
        assert {r.beta != 0 for r in hit if r.kind == "plain"} == {True, False}, ct
    for ct, waves in sorted(dma):
        hit = [r for r, p in rows if AC.form_name(p) == "wide_dma" and (p.ct, p.rt) == (ct, waves)]
        assert hit and {r.kind for r in hit} == {"plain"}, (ct, waves)
    # the plan names no form the source does not launch
    for r, p in rows:
        form = AC.form_name(p)
        assert (form.startswith("panel") and (p.ct, p.rt, 4) in panel) or (form == "wide" and p.ct in wide) or \
            (form == "wide_dma" and (p.ct, p.rt) in dma) or form.startswith("gemm"), (r.id, p)
    # the knob rows take the tile the heuristic would not
    for r, p in rows:
        if r.env in ("rt16", "rt32"):
            assert p.rt == int(r.env[2:]) != (32 if ((r.n + 31) // 32) * r.B >= 256 else 16), r.id


def test_shapes_of_every_loop_are_present():
    P = AC.PLANS
    plain = [r for r in AC.of("plain")]
    f32 = [r for r in plain if AC.form_name(P[r.id]) == "panel_f32" and not r.packed]
    for trans in (0, 1):
        assert set(AC.PANEL_N) <= {r.n for r in f32 if r.trans == trans}
        assert {16 * ct for ct in range(1, 9)} | {16 * ct + 1 for ct in range(8)} <= {r.C for r in f32 if r.trans == trans}
    grids = {P[r.id].grid for r in f32}
    assert {1, 3, 7, 8, 9} <= grids and any(g % 8 == 5 and g > 8 for g in grids), sorted(grids)[:20]
    assert P["plain-lastpanel-1x2560x16T"].lds == 160 * 1024
    gemm = {r.id for r in plain if AC.form_name(P[r.id]) == "gemm_f32"}
    assert {"plain-gemm-1x2564x16T", "plain-gemm-2x67x20N", "plain-gemm-off1-2x64x20N", "plain-gemm-2x64x130N",
            "plain-gemm-2x131x20Np"} <= gemm
    assert AC.BY_ID["plain-gemm-1x2564x16T"].o.get("cpu_only") and sum(1 for r in AC.ROWS if r.o.get("cpu_only")) == 1
    for form in ("panel_f32", "panel_bf16", "wide", "wide_dma"):
        hit = [r for r in plain if AC.form_name(P[r.id]) == form]
        assert {r.beta for r in hit} == {0.0, 1.0, 0.5}, form
        assert {r.vpad > 0 for r in hit} == {True, False} and {r.upad > 0 for r in hit} == {True, False}, form
        assert {r.trans for r in hit} == {0, 1}
        if form != "panel_f32":
            assert {r.trans for r in hit if r.flagged} == {0, 1}, form
    bf16 = [r for r in plain if AC.form_name(P[r.id]) == "panel_bf16"]
    assert set(AC.BF16_N) <= {r.n for r in bf16}
    wide = [r for r in plain if AC.form_name(P[r.id]) == "wide"]
    assert {(P[r.id].ct, r.n) for r in wide if r.env == "wide"} >= {(ct, n) for ct in range(1, 9) for n in AC.WIDE_N}
    assert {129, 131, 260} <= {r.n for r in wide} and all(r.B in (2, 3) for r in wide if r.env == "wide")
    assert {P[r.id].fallback for r in wide if r.flagged} == {_lib.AGG_FB_PANEL, _lib.AGG_FB_GEMM}
    assert [(r.B, r.n, r.C) for r in wide if r.env == ""] == [(512, 128, 8)]
    dma = [r for r in plain if AC.form_name(P[r.id]) == "wide_dma"]
    assert set(AC.DMA_C) <= {r.C for r in dma} and set(AC.DMA_N) | {131, 260} <= {r.n for r in dma}
    assert all(r.env == "" for r in dma) and {P[r.id].rt for r in dma} == {4, 8}
    assert any(r.flagged and P[r.id].fallback == _lib.AGG_FB_GEMM for r in dma)
    # the tail: on the three forms, every group layout, every operand both ways
    fused = AC.of("fused")
    for form in ("panel_f32", "panel_bf16", "wide"):
        hit = [r for r in fused if AC.form_name(P[r.id]) == form]
        assert {r.o["w"] for r in hit} >= set(AC.PAIRS) | {(20,)}, form
        assert any(len(r.o["w"]) == 2 and r.o["w"][0] % 16 for r in hit)
        assert {r.o["normalize"] for r in hit} == {0, 1} and {r.o["stats"] for r in hit} == {0, 1, 2}, form
        for k in ("part", "invn", "P", "sep", "ypad"):
            assert {bool(r.o[k]) for r in hit} == {True, False}, (form, k)
        assert {tuple(r.o["bias"]) for r in hit} >= {(0,), (1,), (0, 0), (1, 1), (0, 1), (1, 0)}, form
        assert any(not any(r.o["bias"]) and not r.o["P"] and r.o["normalize"] for r in hit), form    # the clamp's row
        assert any(r.n % (P[r.id].rt if form != "wide" else 128) for r in hit), form                 # rows past n
    assert {r.n for r in AC.of("pack")} >= set(AC.PACK_N) and sum(1 for r in AC.of("pack") if r.o["zero"]) == 3


def test_what_the_rules_put_out_of_reach(lib):
    """No knob set: no shape reaches a wide form without the packed operand, the wide kernel at C <= 128 below 512
    workgroups, a panel form at C > 128 or n % 4 != 0, the bf16 loop below n = 128, the tail behind a DMA form or a
    GEMM, or a 32-row transposed tile above n = 1280."""
    for B in (1, 3, 64, 511, 512):
        for n in (4, 67, 124, 128, 131, 132, 1280, 1284, 2564):
            for Cc in (1, 47, 48, 128, 129, 320, 321):
                for packed in (0, 1):
                    for trans in (0, 1):
                        p = AC.query(lib, B, n, Cc, trans, packed)
                        form = AC.form_name(p)
                        if form in ("wide", "wide_dma"):
                            assert packed and n >= 128 and Cc <= 320 and p.fallback != _lib.AGG_FB_NONE
                            assert (form == "wide") == (Cc <= 128) and (Cc > 128 or B * ((n + 127) // 128) >= 512)
                        else:
                            assert p.fallback == _lib.AGG_FB_NONE
                        if form.startswith("panel"):
                            assert Cc <= 128 and n % 4 == 0 and (form == "panel_f32" or (packed and n >= 128))
                            assert not (trans and n > 1280 and p.rt == 32)
                        assert p.split == (1 if form in ("panel_bf16", "wide", "wide_dma") else 0)
                        f = AC.query(lib, B, n, Cc, trans, packed, fused=1)
                        if f.declines:
                            assert f == AC.query(lib, B, n, Cc, 0, packed)._replace(declines=1)
                        else:
                            assert AC.form_name(f) in ("panel_f32", "panel_bf16", "wide") and Cc <= 128 and n % 4 == 0
                            assert f.fallback in (_lib.AGG_FB_NONE, _lib.AGG_FB_PANEL)


def _defects_of(r, p):
    form = AC.form_name(p)
    if r.flagged or form.startswith("gemm"):
        return ()
    out = ["step"]
    if form in ("panel_bf16", "wide", "wide_dma"):
        out.append("lo")
    if form == "panel_f32" and r.n % 16:
        out.append("tail")
    if r.kind == "fused":
        out += ["divisor"] + (["dup"] if r.C % 16 else [])
    return out


def test_grid_inputs_have_the_properties_the_exact_comparison_rests_on():
    for r in AC.ROWS:
        if r.kind == "pack" or r.B * r.n * r.n > 2 ** 22:
            continue
        M, V = AC._product_inputs(r, "grid")
        nz = M != 0
        assert int(nz.sum(2).max()) <= 8 and int(nz.sum(1).max()) <= 8, r.id
        assert bool(nz.any(1).all()) and bool(nz.any(2).all()), r.id                  # every k column, every row
        assert float(M.abs().sum(2).max()) <= 11 + (AC.FLAG_VALUE if r.flagged else 0), r.id
        first, last = AC.edge_rows(r.n)
        for rows_ in (first, last):
            cols = AC.edge_columns(r.n)[:AC.EDGE_PER_ROW * len(rows_)]
            assert {0, r.n - 1} <= set(cols) and bool(nz[:, rows_][:, :, cols].any(1).all()), r.id
            # what the five extra entries per row reach: with 16 rows every panel and segment edge, and every k-step
            # edge up to n = 640; a short last tile reaches fewer
            if len(rows_) == 16:
                want = {c for e in range(256, r.n, 256) for c in (e - 1, e)}
                if r.n <= 640:
                    want |= {c for e in range(16, r.n, 16) for c in (e - 1, e)}
                assert want <= set(cols), r.id
        k = V * 2.0 ** 18
        assert bool((k == k.round()).all()) and float(k.abs().min()) >= 1 and float(k.abs().max()) < 2 ** 19, r.id
        if r.packed:
            hi, mid, lo = AC.split3(V)
            # (a rounded-to-nearest plane and its signed remainder hold nine bits each: the low plane gets the last two
            # of V's twenty, so about a third of its entries are non-zero)
            assert bool(((hi + mid) + lo == V).all()) and float((mid != 0).float().mean()) > 0.9 and \
                float((lo != 0).float().mean()) > 0.2, r.id
    # the edge list at a panel shape: both sides of 1024 and of every 256, then the k-steps
    assert AC.edge_columns(2052)[:8] == [0, 2051, 1023, 1024, 2047, 2048, 511, 512]
    assert {15, 16, 31, 32, 127, 128} <= set(AC.edge_columns(132)) and len(AC.edge_columns(132)) == 2 + 2 * 8


def _emulation_rows():
    """Every form, epilogue and loop edge at the sizes the CPU does in a moment."""
    return [r for r in AC.ROWS if r.kind != "pack" and r.B * r.n * r.n * (r.C + 16) <= 2 ** 26]


def test_emulation_stays_inside_the_bounds_and_defects_do_not(lib):
    caught = {}
    seen = set()
    for r in _emulation_rows():
        p = AC.PLANS[r.id]
        form = AC.form_name(p)
        seen.add((r.kind, form))
        for mode in ("grid", "dense"):
            d = AC.inputs(r.id, mode)
            for defect in (None,) + (tuple(_defects_of(r, p)) if mode == "grid" or r.kind == "fused" else ()):
                if r.kind == "plain":
                    got = AC.emulate_plain(r, p, d, defect)
                    if mode == "grid":
                        ok = torch.equal(got.double(), d["ref"])
                    else:
                        ok = RC.ratio((got.double() - d["ref"]).abs(), d["bound"]) <= 1.0
                else:
                    errs = AC.tail_errors(r, d, AC.emulate_tail(r, p, d, defect))
                    ok = all(e <= 1.0 for _, e in errs)
                    if defect is None and mode == "grid":        # the product itself is exact on the grid
                        prod = AC.emulate_product(r, p, d["M"], d["V"])
                        ok = ok and torch.equal(prod.double(), d["prod"])
                if defect is None:
                    assert ok, f"{r.id} {mode}: the emulation of {form} misses its own check"
                else:
                    key = (r.kind, form, defect)
                    caught[key] = caught.get(key, 0) + (0 if ok else 1)
                    if mode == "grid" and r.kind == "plain":
                        assert not ok, f"{r.id}: defect {defect!r} passes the exact comparison"
    assert seen >= {("plain", f) for f in ("panel_f32", "panel_bf16", "wide", "wide_dma", "gemm_f32")} | \
        {("fused", f) for f in ("panel_f32", "panel_bf16", "wide")}
    want = {("plain", "panel_f32", "step"), ("plain", "panel_f32", "tail"), ("plain", "panel_bf16", "lo"),
            ("plain", "panel_bf16", "step"), ("plain", "wide", "lo"), ("plain", "wide", "step"), ("plain", "wide_dma", "lo"),
            ("plain", "wide_dma", "step")}
    for f in ("panel_f32", "panel_bf16", "wide"):
        want |= {("fused", f, "dup"), ("fused", f, "divisor"), ("fused", f, "step")}
    want |= {("fused", "panel_bf16", "lo"), ("fused", "wide", "lo"), ("fused", "panel_f32", "tail")}
    missed = sorted(k for k in want if not caught.get(k))
    assert not missed, f"defects no row catches: {missed}"


def test_the_new_entries_refuse_before_any_launch(lib):
    g = _lib.RowGroups(G=2, c0=(C.c_int * 2)(0, 8), w=(C.c_int * 2)(8, 8))
    yp = _lib.GroupPtrs()
    yp.p[0], yp.p[1], yp.ld[0], yp.ld[1] = 16, 16, 8, 8
    one = C.c_void_p(16)

    def call(g=g, yp=yp, adj=one, V=one, ldv=16, part=one, stats=1, pk=(None, None, None, None), B=1, n=4):
        return lib.dp_adj_aggregate_rownorm(adj, pk[0], pk[1], pk[2], V, ldv, None, C.byref(g) if g else None, None,
                                            C.byref(yp) if yp else None, None, part, B, n, 1, stats, 0, pk[3], 0, None)

    def err():
        return lib.dp_last_error_string()

    for bad, text in ((_lib.RowGroups(G=3), b"G=3"), (_lib.RowGroups(G=0), b"G=0"),
                      (_lib.RowGroups(G=1, c0=(C.c_int * 2)(0, 0), w=(C.c_int * 2)(0, 0)), b"width"),
                      (_lib.RowGroups(G=2, c0=(C.c_int * 2)(0, 4), w=(C.c_int * 2)(8, 8)), b"overlap"),
                      (_lib.RowGroups(G=2, c0=(C.c_int * 2)(8, 0), w=(C.c_int * 2)(8, 8)), b"overlap"),
                      (_lib.RowGroups(G=2, c0=(C.c_int * 2)(0, 9), w=(C.c_int * 2)(8, 8)), b"without a gap"),
                      (_lib.RowGroups(G=1, c0=(C.c_int * 2)(4, 0), w=(C.c_int * 2)(8, 0)), b"without a gap")):
        assert call(g=bad) == -1 and text in err(), (text, err())
    assert call(g=None) == -1 and b"NULL" in err()
    assert call(adj=None) == -1 and b"NULL" in err() and call(V=None) == -1 and b"NULL" in err()
    assert call(yp=None) == -1 and b"NULL" in err()
    short = _lib.GroupPtrs()
    short.p[0], short.p[1], short.ld[0], short.ld[1] = 16, 16, 8, 7
    assert call(yp=short) == -1 and b"ld=7" in err()
    gone = _lib.GroupPtrs()
    gone.p[0], gone.ld[0], gone.ld[1] = 16, 8, 8
    assert call(yp=gone) == -1 and b"group 1 is NULL" in err()
    assert call(ldv=15) == -1 and b"ldv=15" in err()
    assert call(part=None) == -1 and b"part is NULL" in err() and call(stats=3) == -1 and b"stats_mode=3" in err()
    assert call(pk=(one, None, one, one)) == -1 and b"together" in err()
    assert call(B=0) == -1 and call(n=0) == -1
    # a shape the fused entry declines answers so without a launch (and without a GPU)
    assert call(n=67, ldv=16) == _lib.AGG_DECLINED
    # ... with a status that is none the entry can otherwise return: not DP_OK, no DP_ERR_* (-1 .. -4), and not positive,
    # where the hipError_t of a failed launch lives (hipErrorInvalidValue is 1)
    hdr = open(os.path.join(ROOT, "include", "diffpool_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (DP_OK|DP_ERR_\w+|DP_AGG_DECLINED) \(?(-?\d+)\)?", hdr)}
    assert codes["DP_AGG_DECLINED"] == _lib.AGG_DECLINED < 0 and len(codes) >= 6
    assert all(v != _lib.AGG_DECLINED for k, v in codes.items() if k != "DP_AGG_DECLINED")
    assert lib.dp_adj_pack_zero(None, one, one, one, 1, 4, one, 16, None) == -1 and b"NULL" in err()
    assert lib.dp_adj_pack_zero(one, one, one, one, 1, 4, None, 16, None) == -1 and b"NULL" in err()
