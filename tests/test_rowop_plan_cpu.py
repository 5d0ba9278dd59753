"""CPU checks of the row-kernel case table (tests/rowop_cases.py): every row's recorded plan is dp_rowop_plan's answer —
the answer of the pick functions the launchers of dp_rowops.hip decide with; the table reaches every instantiation the
six launchers name, with one and with two groups and with the optional operands present and absent; the tier edges are
there; the pick rule restated here agrees with the query over all widths; the fp64 references tell the defects a row
kernel can have from rounding at the bounds test_gpu_rowops.py applies; the pass-through entries refuse what the
kernels' contracts exclude before any launch."""
import collections
import ctypes as C
import os
import re

import pytest
import torch

from graph_pooling_amd import _lib
from tests import rowop_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_pooling_amd", "csrc", "dp_rowops.hip")
# launcher -> (kernel family of the plan, kernels it may launch)
LAUNCHERS = {"rownorm_fwd": "k_rownorm_fwd", "rownorm_bwd": "k_rownorm_bwd", "bn_apply": "k_bn_apply_fwd",
             "softmax_fwd": "k_softmax_mask_fwd_plan", "softmax_bwd": "k_softmax_mask_bwd_plan"}


@pytest.fixture(scope="module")
def lib():
    assert "DP_NO_ROW_QUADS" not in os.environ, "unset DP_NO_ROW_QUADS: the table records the plans with the quad forms"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _instantiations():
    """{kernel: {(NK, quad)}} read off the hipLaunchKernelGGL lines of dp_rowops.hip."""
    out = {}
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?(k_\w+)(?:<([^>]*)>)?", open(SRC).read()):
        name, targs = m.group(1), m.group(2)
        if targs is None:
            out.setdefault(name, set())
            continue
        t = [a.strip() for a in targs.split(",")]
        out.setdefault(name, set()).add((int(t[0]), 1 if t[-1] == "true" else 0))
    return out


def test_every_recorded_plan_is_the_launchers(lib):
    wrong = [f"{c.id}: recorded {RC.PLANS.get(c.id)}, dp_rowop_plan {RC.plan_of(lib, c)}" for c in RC.CASES
             if RC.plan_args(c) is not None and RC.PLANS.get(c.id) != RC.plan_of(lib, c)]
    assert not wrong, "\n".join(wrong[:20])
    assert set(RC.PLANS) == {c.id for c in RC.CASES if RC.plan_args(c) is not None}


def test_table_reaches_every_instantiation(lib):
    inst = _instantiations()
    assert {"k_bn_finalize", "k_bn_bwd_finalize", "k_softmax_mask_fwd", "k_softmax_mask_bwd", "k_masked_max_fwd",
            "k_colsum_batched"} <= set(inst)
    for fam, kernel in LAUNCHERS.items():
        forms = inst[kernel]
        assert len(forms) >= 4, (kernel, forms)
        rows = [(c, RC.PLANS[c.id]) for c in RC.of(fam)]
        for nk, quad in sorted(forms):
            hit = [c for c, p in rows if p[1] == nk and p[2] == quad and not p[4]]
            assert hit, f"{kernel}<{nk}{', true' if quad else ''}>: no row"
            if fam in ("rownorm_fwd", "rownorm_bwd", "bn_apply"):
                assert {c.G for c in hit} == {1, 2}, f"{kernel}<{nk}, quad={quad}>: G = {sorted({c.G for c in hit})} only"
            # every optional operand and flag of the launcher, both ways in this very instantiation (bias, stats, dbias
            # and zero, which are no booleans, below)
            per_form = {"rownorm_fwd": ("P", "invn", "normalize"), "bn_apply": ("part", "relu"),
                        "rownorm_bwd": ("bn", "relu", "normalize", "vs"), "softmax_fwd": ("S2", "vs", "nn"),
                        "softmax_bwd": ("dS2", "nn")}[fam]
            assert set(per_form) | {"bias", "stats", "dbias", "zero"} >= {k for c in hit for k in c.o}, (fam, per_form)
            for k in per_form:
                assert {bool(c.o[k]) for c in hit} == {True, False}, f"{kernel}<{nk}, quad={quad}>: {k} never both ways"
            if fam == "rownorm_fwd":
                assert {any(c.o["bias"]) for c in hit} == {True, False} and len({c.o["stats"] for c in hit}) >= 2
            if fam == "rownorm_bwd":
                assert {bool(c.o["dbias"]) for c in hit} == {True, False}
                assert {(c.o["bn"], c.o["relu"]) for c in hit} >= {(1, 0), (1, 1), (0, 1), (0, 0)}
            if fam == "softmax_fwd":
                assert {c.o["zero"] is not None for c in hit} == {True, False}
        # the generic softmax kernels: the operands they take, both ways (the forward one writes no split and folds no
        # zero region; the backward one has no slab of its own)
        if fam.startswith("softmax"):
            gen = [c for c, p in rows if p[4]]
            for k in {"softmax_fwd": ("S2", "nn"), "softmax_bwd": ("dS2", "nn", "dbias")}[fam]:
                assert {bool(c.o[k]) for c in gen} == {True, False}, f"generic {fam}: {k} never both ways"
        # the plan has no form the source does not launch
        assert {(p[1], p[2]) for _, p in rows if not p[4]} <= forms
    # with and without the finalize kernel; generic and plan; the zero-fill folded in and apart; both loops of the max
    for fam in ("rownorm_bwd", "bn_apply"):
        assert {RC.PLANS[c.id][3] for c in RC.of(fam)} == {0, 1}
    for fam in ("softmax_fwd", "softmax_bwd"):
        assert {RC.PLANS[c.id][4] for c in RC.of(fam)} == {0, 1}
    assert {RC.PLANS[c.id][5] for c in RC.of("softmax_fwd")} == {_lib.ROWZ_NONE, _lib.ROWZ_FOLDED, _lib.ROWZ_APART}
    assert {RC.PLANS[c.id][1] for c in RC.of("masked_max")} == {0, 32}
    # dbias slabs for none, one or both groups; slabs of one group only on either side
    db = {c.o["dbias"] for c in RC.of("rownorm_bwd")}
    assert {None, (1,), (1, 1), (0, 1), (1, 0)} <= db


def test_tier_edges_and_shapes_are_present():
    edges = {"rownorm_fwd": (32, 64, 128, 256, 320, 512), "rownorm_bwd": (32, 64, 128, 256, 320, 512),
             "bn_apply": (32, 64, 128), "softmax_fwd": (64, 128, 256, 320, 512, 768),
             "softmax_bwd": (64, 128, 256, 320, 512)}
    for fam, es in edges.items():
        ws = {c.w[0] for c in RC.of(fam) if c.G == 1}
        assert set(RC.WIDTHS) <= ws
        for e in es:
            assert {e - 1, e, e + 1 if e != 768 else 772} <= ws, (fam, e)
    for fam in RC.FAMILIES:
        assert any(c.off == 1 for c in RC.of(fam)) and any(c.tight for c in RC.of(fam)), fam
    assert {1, 15, 16, 17} <= {c.B * c.n for c in RC.of("bn_apply") if c.o["part"]}
    assert {768, 772} <= {c.w[0] for c in RC.of("softmax_fwd")}
    for fam in ("rownorm_fwd", "bn_apply", "softmax_fwd", "softmax_bwd"):
        assert any(c.B * c.n * c.G > 65536 for c in RC.of(fam)), fam
    assert {1, 7, 8, 9, 17} <= {c.n for c in RC.of("rownorm_bwd")} and {1, 3} <= {c.B for c in RC.of("rownorm_bwd")}
    assert {1, 2, 16, 17, 32, 33, 40} <= {c.Bs for c in RC.of("bn_apply")}
    assert any(c.Bs == 2 * c.B for c in RC.of("bn_apply")) and any(c.Bs == 2 * c.B for c in RC.of("rownorm_bwd"))
    assert {15, 16, 17} <= {c.n for c in RC.of("softmax_fwd")} and {63, 64, 65} <= {c.n for c in RC.of("softmax_bwd")}
    assert {1, 511, 512, 513, 530} <= {c.n for c in RC.of("masked_max")}
    assert {63, 64, 65, 130} <= {c.w[0] for c in RC.of("masked_max")}
    assert {(c.n, c.o["split"]) for c in RC.of("colsum")} >= {(r, s) for r in (1, 15, 16, 17, 100) for s in (1, 8)} | {(5, 8)}
    flags = {(c.o["bn"], c.o["relu"], c.o["normalize"]) for c in RC.of("rownorm_bwd")}
    assert len(flags) == 8
    assert any(c.G == 2 and c.c0[1] % 4 for c in RC.of("rownorm_fwd") if RC.PLANS[c.id][2])


def _pick(fam, w, Bs=0, stats=False):
    """The pick rule, restated: (NK, quad, finalize)."""
    maxw = max(w)
    quads = 128 < maxw <= 512 and all(x >= 4 and x % 4 == 0 for x in w)
    fin = 1 if stats and Bs > 32 else 0
    if fam == "bn_apply":
        return (2 if maxw <= 32 else 4 if maxw <= 64 else 8 if maxw <= 128 else 0), 0, fin
    if quads:
        return (4 if maxw <= 256 else 5 if maxw <= 320 else 8), 1, fin
    top = (320, 20) if fam == "rownorm_fwd" else (256, 16)
    return (2 if maxw <= 32 else 4 if maxw <= 64 else 8 if maxw <= 128 else top[1] if maxw <= top[0] else 0), 0, fin


def _softmax_pick(K, plan_wanted, limit):
    if not plan_wanted or 16 * K * 4 > limit:
        return 0, 0, 1
    if 128 < K <= 512 and K % 4 == 0:
        return (4 if K <= 256 else 5 if K <= 320 else 8), 1, 0
    return (4 if K <= 64 else 8 if K <= 128 else 16 if K <= 256 else 0), 0, 0


def test_pick_rule_restated_agrees_with_the_query(lib):
    ops = {"rownorm_fwd": _lib.ROWOP_ROWNORM_FWD, "rownorm_bwd": _lib.ROWOP_ROWNORM_BWD,
           "bn_apply": _lib.ROWOP_BN_APPLY_FWD}
    grid = (1, 2, 3, 4, 5, 8, 31, 32, 33, 64, 65, 128, 129, 132, 255, 256, 257, 260, 320, 321, 324, 512, 513, 516, 800)
    for fam, op in ops.items():
        for Bs, flags in ((0, 0), (32, _lib.ROWF_STATS), (33, _lib.ROWF_STATS), (33, 0)):
            want_stats = bool(flags) and fam != "rownorm_fwd"
            for w in range(1, 801):
                p = RC.query(lib, op, (w,), 8, 2, Bs, flags)
                assert (p[1], p[2], p[3]) == _pick(fam, (w,), Bs, want_stats), (fam, w, Bs, flags, p)
            if Bs == 33 and flags:
                for w0 in grid:
                    for w1 in grid:
                        p = RC.query(lib, op, (w0, w1), 8, 2, Bs, flags)
                        assert (p[1], p[2], p[3]) == _pick(fam, (w0, w1), Bs, want_stats), (fam, w0, w1, p)
    for K in range(1, 801):
        for flags in (0, _lib.ROWF_VS, _lib.ROWF_ZERO, _lib.ROWF_ZERO | _lib.ROWF_ZERO_UNALIGNED,
                      _lib.ROWF_VS | _lib.ROWF_ZERO):
            p = RC.query(lib, _lib.ROWOP_SOFTMAX_FWD, (K,), 8, 2, 0, flags)
            assert (p[1], p[2], p[4]) == _softmax_pick(K, flags != 0, 48 * 1024), (K, flags, p)
            fits = 16 * K * 4 <= 48 * 1024
            zero = _lib.ROWZ_NONE if not flags & _lib.ROWF_ZERO else \
                _lib.ROWZ_FOLDED if fits and not flags & _lib.ROWF_ZERO_UNALIGNED else _lib.ROWZ_APART
            assert p[5] == zero and p[0] == (_lib.ROWK_SOFTMAX_FWD if p[4] else _lib.ROWK_SOFTMAX_FWD_PLAN)
        for flags in (0, _lib.ROWF_DBIAS):
            p = RC.query(lib, _lib.ROWOP_SOFTMAX_BWD, (K,), 8, 2, 0, flags)
            assert (p[1], p[2], p[4]) == _softmax_pick(K, flags != 0, 64 * 1024), (K, flags, p)
    assert RC.query(lib, _lib.ROWOP_SOFTMAX_BWD, (1025,), 8, 2, 0, _lib.ROWF_DBIAS)[4] == 1
    out = (C.c_int * _lib.ROWOP_PLAN_INTS)()
    for n in (1, 511, 512, 513, 530):
        assert lib.dp_rowop_plan(_lib.ROWOP_MASKED_MAX_FWD, None, n, 1, 0, 0, out) == 0
        assert tuple(out)[:2] == (_lib.ROWK_MASKED_MAX_FWD, 32 if n <= 512 else 0)


def test_backward_formula_is_autograd_of_the_fp64_forward():
    """rownorm_bwd_math states dU by formula (the clamp branch of F.normalize has no other statement); on rows off the
    clamp it must be what autograd gives for the float64 forward u -> l2-normalise -> ReLU -> BatchNorm over Bs graphs."""
    for cid in ("rownorm_bwd-20-Bs6-3x9", "rownorm_bwd-132x8-Bs6-3x7", "rownorm_bwd-20-f111-3x9"):
        c = RC.BY_ID[cid]
        Bs = c.Bs or c.B
        g = torch.Generator().manual_seed(5)
        d = dict(DX=[], Y=[], X=[], invn=None, stats=torch.zeros(c.n, c.G, 2, dtype=torch.float64))
        inv_all, want = [], []
        for i, w in enumerate(c.w):
            u = torch.randn(Bs, c.n, w, generator=g, dtype=torch.float64).requires_grad_()
            nrm = u.norm(dim=2, keepdim=True)
            y = u / nrm
            r = y.clamp_min(0) if c.o["relu"] else y
            mu = r.mean((0, 2), keepdim=True)
            var = ((r - mu) ** 2).mean((0, 2), keepdim=True)
            x = (r - mu) / (var + RC.BN_EPS).sqrt()
            dx = torch.randn(Bs, c.n, w, generator=g, dtype=torch.float64)
            x.backward(dx)
            want.append(u.grad[:c.B].reshape(c.B * c.n, w))
            d["DX"].append(dx.reshape(-1, w)), d["Y"].append(y.detach().reshape(-1, w))
            d["X"].append(x.detach().reshape(-1, w))
            inv_all.append((1 / nrm).detach().reshape(-1))
            d["stats"][:, i, 1] = (1 / (var + RC.BN_EPS).sqrt()).detach().reshape(-1)
        d["invn"] = torch.stack(inv_all, 1)
        got = RC.rownorm_bwd_math(c, d, torch.float64)
        for i in range(c.G):
            assert float((got[i]["dU"] - want[i]).abs().max()) <= 1e-11 * float(want[i].abs().max()), cid


def _worst(err, bound):
    return RC.ratio(err, bound)


def test_references_tell_the_defects_from_rounding():
    """On the table's own inputs the faithful fp32 evaluation stays inside the bound and each defect leaves it: one
    dropped column; the last quad lane unmasked, on every row whose recorded plan is a quad form (RC._quad_again: the
    loads are clamped, so the row's last quad enters the norm, the mean, the dot or the softmax sum twice); a divisor of
    w + 1 / Bs + 1; the neighbour group's first column included in the norm; `v >= best` in the max.
    Not asked to show, because they change nothing: a dropped column of a one-column row; a divisor defect on a row mean
    of exactly 0, which only the forward partials can have (a zero row; the BatchNorm inputs have mean 3 and the means
    of the backward are sums of random dx); an unmasked quad lane where the kernel uses no reduction over the row
    (rownorm_fwd with neither normalize nor statistics, rownorm_bwd without normalize — its means come from
    k_bn_bwd_partials and its dot goes unused)."""
    n_checked, n_quad = 0, collections.Counter()
    for c in RC.CASES:
        if c.B * c.n > 2000:
            continue
        d = RC.inputs(c.id)
        quad = bool(RC.PLANS[c.id][2]) if c.id in RC.PLANS else False
        if c.fam == "rownorm_fwd":
            norm, stats = c.o["normalize"], c.o["stats"]
            ref = RC.rownorm_fwd_math(c, d, torch.float64)
            defects = [None] + (["column"] if norm else []) + (["neighbour"] if norm and c.G == 2 else []) + \
                (["divisor"] if norm and stats else []) + (["quad"] if quad and (norm or stats) else [])
            for defect in defects:
                got = RC.rownorm_fwd_math(c, d, torch.float32, defect)
                for i in range(c.G):
                    by, _, bmean, _ = RC.rownorm_fwd_bounds(c, ref[i])
                    live = slice(2, None) if norm and c.B * c.n >= 3 and d["bias"][i] is None else slice(None)
                    if defect == "divisor" or defect == "quad" and not norm:
                        r = _worst((got[i]["mean"].double() - ref[i]["mean"]).abs()[live], bmean[live])
                    else:
                        r = _worst((got[i]["y"].double() - ref[i]["y"]).abs()[live], by[live])
                    if defect is None:
                        assert r <= 1.0, (c.id, i, r)
                    elif (c.w[i] > 1 or defect != "column") and (defect != "divisor" or float(ref[i]["mean"].abs().max()) > 0):
                        assert r > 1.0, (c.id, defect, i, r)
                    n_checked += 1
                    n_quad[c.fam] += defect == "quad"
        if c.fam == "bn_apply" and c.o["part"]:
            ref = RC.bn_apply_math(c, d, torch.float64)
            for defect in (None, "divisor"):
                got = RC.bn_apply_math(c, d, torch.float32, defect)
                for i in range(c.G):
                    r = _worst((got[i]["x"].double() - ref[i]["x"]).abs(), RC.bn_apply_bounds(c, ref[i])[0])
                    assert (r <= 1.0) if defect is None else (r > 1.0), (c.id, defect, i, r)
                    n_checked += 1
        if c.fam == "rownorm_bwd":
            ref, emu = RC.rownorm_bwd_math(c, d, torch.float64), RC.rownorm_bwd_math(c, d, torch.float32)
            for defect in ["column"] + (["divisor"] if c.o["bn"] else []) + (["quad"] if quad and c.o["normalize"] else []):
                got = RC.rownorm_bwd_math(c, d, torch.float32, defect)
                for i in range(c.G):
                    r = _worst((got[i]["dU"].double() - ref[i]["dU"]).abs(), RC.rownorm_bwd_bound(ref[i], emu[i]))
                    if c.w[i] > 1:
                        assert r > 1.0, (c.id, defect, i, r)
                    n_checked += 1
                    n_quad[c.fam] += defect == "quad"
        if c.fam in ("softmax_fwd", "softmax_bwd") and c.w[0] > 1:
            math_, bound_, key = (RC.softmax_fwd_math, RC.softmax_fwd_bound, "s") if c.fam == "softmax_fwd" else \
                (RC.softmax_bwd_math, RC.softmax_bwd_bound, "dl")
            ref = math_(c, d, torch.float64)
            b = bound_(c, ref)
            ok = _worst((math_(c, d, torch.float32)[key].double() - ref[key]).abs(), b)
            bad = _worst((math_(c, d, torch.float32, "column")[key].double() - ref[key]).abs(), b)
            assert ok <= 1.0 < bad, (c.id, ok, bad)
            if quad:
                bad = _worst((math_(c, d, torch.float32, "quad")[key].double() - ref[key]).abs(), b)
                assert bad > 1.0, (c.id, "quad", bad)
                n_quad[c.fam] += 1
            n_checked += 1
        if c.fam == "masked_max" and c.n >= 18:
            out, am = RC.masked_max_ref(c, d)
            out2, am2 = RC.masked_max_ref(c, d, rule_ge=True)
            assert torch.equal(out, out2) and not torch.equal(am, am2), c.id
            n_checked += 1
    assert n_checked > 300
    # the quad defect was shown on every quad form of every family that has them
    for fam in ("rownorm_fwd", "rownorm_bwd", "softmax_fwd", "softmax_bwd"):
        forms = {RC.PLANS[c.id][1] for c in RC.of(fam) if RC.PLANS[c.id][2]}
        assert forms == {4, 5, 8} and n_quad[fam] >= 6, (fam, forms, n_quad[fam])


def test_wrappers_refuse_before_any_launch(lib):
    """NULL or never-read device pointers throughout: a call that reached a launch would fault, these return first."""
    some = 64

    def groups(G=1, c0=(0, 8), w=(8, 8)):
        g = _lib.RowGroups()
        g.G = G
        for i in range(2):
            g.c0[i], g.w[i] = c0[i], w[i]
        return g

    def ptrs(p=(some, some), ld=(8, 8)):
        gp = _lib.GroupPtrs()
        for i in range(2):
            gp.p[i], gp.ld[i] = p[i], ld[i]
        return gp

    def fwd(g, U=some, ldu=16, yout=None, part=None, stats_mode=0, rows=4):
        yout = ptrs() if yout is None else yout
        rc = lib.dp_rownorm_fwd(U, ldu, None, C.byref(g), None, C.byref(yout), None, part, rows, 1, stats_mode, None)
        return rc, lib.dp_last_error_string()

    for kw, msg in [(dict(g=groups(G=0)), b"G=0"), (dict(g=groups(G=3)), b"G=3"), (dict(g=groups(w=(0, 8))), b"w=0"),
                    (dict(g=groups(G=2, c0=(0, 7))), b"overlap"), (dict(g=groups(), U=None), b"NULL"),
                    (dict(g=groups(), yout=ptrs(p=(None, None))), b"NULL"), (dict(g=groups(), yout=ptrs(ld=(7, 7))), b"ld=7"),
                    (dict(g=groups(G=2), ldu=15), b"ldu=15"), (dict(g=groups(), stats_mode=1), b"part is NULL"),
                    (dict(g=groups(), stats_mode=3), b"stats_mode=3"), (dict(g=groups(), rows=0), b"rows=0")]:
        rc, text = fwd(**kw)
        assert rc == -1 and msg in text, (rc, text, msg)
    g, gp = groups(), ptrs()
    assert lib.dp_rownorm_fwd(some, 16, None, None, None, C.byref(gp), None, None, 4, 1, 0, None) == -1
    assert lib.dp_bn_apply_fwd(some, 16, some, None, C.byref(g), C.byref(gp), 2, 4, 1, 0, None) == -1
    assert b"stats is NULL" in lib.dp_last_error_string()
    assert lib.dp_bn_apply_fwd(some, 7, None, None, C.byref(g), C.byref(gp), 2, 4, 1, 0, None) == -1
    assert lib.dp_bn_apply_fwd(some, 8, None, None, C.byref(g), C.byref(gp), 2, 4, 1, -1, None) == -1
    assert lib.dp_bn_bwd_partials(C.byref(g), C.byref(gp), C.byref(gp), None, 4, None) == -1
    bwd = lambda g, has_bn=0, normalize=0, xhat=None, invn=None, vs=None, dbias=None, dU=some, ldu=1100: \
        lib.dp_rownorm_bwd(C.byref(g), C.byref(gp), xhat, C.byref(gp), invn, None, None, dU, ldu, dbias, 2, 4, 0, has_bn,
                           normalize, vs, 0, None)
    assert bwd(g, has_bn=1) == -1 and b"xhat is NULL" in lib.dp_last_error_string()
    assert bwd(g, has_bn=1, xhat=C.byref(gp)) == -1 and b"stats or part2" in lib.dp_last_error_string()
    assert bwd(g, normalize=1) == -1 and b"invn is NULL" in lib.dp_last_error_string()
    assert bwd(g, dU=None) == -1 and bwd(g, ldu=7) == -1 and bwd(groups(G=2, c0=(0, 4))) == -1
    wide, wp = groups(w=(1024, 8)), ptrs(ld=(1024, 1024))
    rc = lib.dp_rownorm_bwd(C.byref(wide), C.byref(wp), None, C.byref(wp), None, None, None, some, 1100, C.byref(wp), 2, 4,
                            0, 0, 0, some, 0, None)
    assert rc == -1 and b"vs" in lib.dp_last_error_string() and b"LDS" in lib.dp_last_error_string()
    assert bwd(g, vs=some + 2) == -1 and b"16-byte" in lib.dp_last_error_string()
    rc = lib.dp_rownorm_bwd(C.byref(g), C.byref(gp), None, C.byref(gp), None, None, None, some, 1100,
                            C.byref(ptrs(ld=(7, 7))), 2, 4, 0, 0, 0, None, 0, None)
    assert rc == -1 and b"stride between graphs" in lib.dp_last_error_string()
    sf = lambda K=8, vs=None, zp=None, zb=0, ldl=1000, S=some: \
        lib.dp_softmax_mask_fwd(some, ldl, S, 1000, None, 2, 4, K, None, vs, zp, zb, None)
    assert sf(K=772, vs=some) == -1 and b"K=772" in lib.dp_last_error_string()
    assert sf(K=0) == -1 and sf(ldl=7) == -1 and sf(S=None) == -1 and sf(zb=16) == -1 and sf(vs=some + 4) == -1
    sb = lambda K=8, dS=some, dbias=None, stride=0: \
        lib.dp_softmax_mask_bwd(some, 1000, dS, 1000, None, some, 1000, 2, 4, K, dbias, stride, None, None)
    assert sb(dS=None) == -1 and sb(K=1001) == -1 and sb(dbias=some, stride=7) == -1
    assert b"dbias_stride=7" in lib.dp_last_error_string()
    cs = lambda X=some, ldx=8, split=1, rows=4: lib.dp_colsum_batched(X, ldx, 32, rows, 8, some, 8, 2, split, None)
    assert cs(X=None) == -1 and cs(ldx=7) == -1 and cs(split=0) == -1 and cs(rows=0) == -1
    out = (C.c_int * _lib.ROWOP_PLAN_INTS)()
    assert lib.dp_rowop_plan(9, C.byref(g), 4, 1, 0, 0, out) == -1 and lib.dp_rowop_plan(0, None, 4, 1, 0, 0, out) == -1
    assert lib.dp_rowop_plan(0, C.byref(g), 4, 1, 0, 0, None) == -1
