"""CPU checks of the fp32 GEMM case table (tests/gemm_cases.py): through dp_bgemm_plan — answered by gemm_pick, the
host function bgemm_group itself takes its tile and K ranges from — the table reaches all seven workgroup tiles with
every transpose pair and both operand loaders, the diversion to the split-bf16 kernel, the split by shape class, the
shrinking of ksplit and every split-K form; every row's recorded plan is the query's answer; the edge values are
present for every tile; the wrapper refuses what the kernel's contract excludes before any launch; the integer pass is
exact in fp32; and the fp64 reference tells a truncated operand or one dropped k term from rounding at the bound
test_gpu_gemm.py applies."""
import ctypes as C
import os

import pytest
import torch

from graph_pooling_amd import _lib
from tests import gemm_cases as GC

# knobs that change what dp_bgemm_plan answers (dp_api.hip: knobs())
PLAN_KNOBS = ("DP_GEMM_TARGET_WGS", "DP_NO_SPLIT_GEMM", "DP_SPLIT_GEMM_W4")


@pytest.fixture(scope="module")
def lib():
    set_ = [k for k in PLAN_KNOBS if k in os.environ]
    assert not set_, f"unset {set_}: these knobs change the GEMM launcher's plan, the table records the default plan"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _tiled(row):
    return [(p, pl) for p, pl in zip(row.problems, row.plan) if pl not in (GC.BF16, GC.NONE)]


def test_every_recorded_plan_is_the_launchers(lib):
    ids = [r.id for r in GC.ROWS]
    assert len(ids) == len(set(ids))
    wrong = [f"{r.id}: recorded {r.plan}, dp_bgemm_plan {GC.plan_of(lib, r)}" for r in GC.ROWS
             if GC.plan_of(lib, r) != r.plan]
    assert not wrong, "\n".join(wrong)


def test_picks_from_the_formula_stated_independently(lib):
    """Largest tile with >= 512 workgroups (batch x tiles), never taller than the problem; N picks the family."""
    tile = lambda b, M, N: GC.plan_single(lib, b, M, N)[:2]
    # 65 x 65: 4 tiles of 64 x 64, 6 of 32 x 64.  512 / 4 = 128; 512 / 6 = 85.3
    assert tile(85, 65, 65) == (16, 64) and tile(86, 65, 65) == (32, 64) and tile(127, 65, 65) == (32, 64)
    assert tile(128, 65, 65) == (64, 64)
    # 129 x 32: 2 tiles of 128 x 32, 3 of 64 x 32
    assert tile(256, 129, 32) == (128, 32) and tile(255, 129, 32) == (64, 32) and tile(170, 129, 32) == (32, 32)
    assert tile(171, 129, 32) == (64, 32)
    assert tile(10 ** 4, 500, 16) == (64, 16) and tile(1, 1, 1) == (64, 16)
    assert tile(1, 17, 33) == (32, 64) and tile(1, 32, 33) == (32, 64) and tile(1, 16, 33) == (16, 64)
    assert tile(65535, 64, 32) == (64, 32)                       # never <128,32> for M <= 64
    assert tile(65535, 32, 32) == (32, 32) and tile(65535, 32, 64) == (32, 64) and tile(65535, 16, 64) == (16, 64)
    # test_gpu_ops.py::test_bgemm_shapes: its seven shapes reach exactly three tiles at batch 3
    shapes = [(1, 1, 1), (50, 60, 500), (500, 40, 500), (89, 20, 37), (33, 129, 65), (64, 64, 32), (7, 300, 3)]
    assert {tile(3, M, N) for M, N, _ in shapes} == {(64, 16), (32, 32), (16, 64)}
    # the loader: 16-byte loads need four elements along each operand's contiguous dimension
    quad = lambda M, N, K, tA, tB: GC.plan_single(lib, 2, M, N, K, tA, tB)[2]
    assert quad(8, 8, 3, 0, 0) == 0 and quad(8, 8, 3, 1, 0) == 1 and quad(8, 8, 3, 1, 1) == 0 and quad(8, 8, 4, 0, 1) == 1
    assert quad(3, 8, 8, 1, 0) == 0 and quad(3, 8, 8, 0, 0) == 1 and quad(8, 3, 8, 0, 0) == 0 and quad(8, 3, 8, 0, 1) == 1


def test_diversion_limits(lib):
    """gemm_split_usable: M >= 96, N >= 80 or in [48, 64], K >= 40, >= 256 tiles of 128 x 128 (128 x 64), alpha 1."""
    bf = lambda b, M, N, K: GC.plan_single(lib, b, M, N, K) == GC.BF16
    assert bf(256, 96, 80, 40) and bf(256, 96, 48, 40) and bf(256, 96, 64, 40) and bf(128, 129, 80, 40)
    assert not any((bf(256, 95, 80, 40), bf(256, 96, 79, 40), bf(256, 96, 47, 40), bf(256, 96, 65, 40),
                    bf(256, 96, 80, 39), bf(255, 96, 80, 40)))
    div = [r for r in GC.SINGLE if r.plan == (GC.BF16,)]
    assert len(div) == 2 and {r.problems[0].N >= 80 for r in div} == {True, False}
    near = {(r.batch, p.M, p.N, p.K) for r in GC.SINGLE for p in r.problems if r.plan != (GC.BF16,)}
    assert {(256, 95, 80, 40), (256, 96, 79, 40), (256, 96, 47, 40), (256, 96, 80, 39), (255, 96, 80, 40)} <= near


def test_table_reaches_every_tile_transpose_loader_and_split_form(lib):
    seen = set()
    for r in GC.ROWS:
        for p, (bm, bn, quad, ranges) in _tiled(r):
            seen.add(((bm, bn), (p.tA, p.tB)))
            seen.add(((bm, bn), "quad" if quad else "dword"))
    for t in GC.TILES:
        for what in [(0, 0), (0, 1), (1, 0), (1, 1), "quad", "dword"]:
            assert (t, what) in seen, f"tile {t}: no row with {what}"
    plans = [pl for r in GC.ROWS for pl in r.plan]
    assert GC.BF16 in plans and GC.NONE in plans
    for form in (GC.ATOMIC, GC.SLABS, GC.TICKETS):
        ks = {r.ksplit for r in GC.GROUPS for p in r.problems if p.split == form}
        assert {2, 4, 8} <= ks, (GC.SPLIT_NAMES[form], ks)
        # K = 40 at ksplit 8: the shared-C forms run 2 ranges, the slabs all 8 (six of them zero partials)
        r40 = [(p, pl) for r in GC.GROUPS if r.ksplit == 8 for p, pl in zip(r.problems, r.plan)
               if p.split == form and p.K == 40]
        assert r40 and all(pl[3] == (8 if form == GC.SLABS else 2) for _, pl in r40)
        # K an exact multiple of ksplit * 32, and one more
        ex = {(p.K % (r.ksplit * GC.KT)) for r in GC.GROUPS for p in r.problems if p.split == form and r.ksplit > 1}
        assert {0, 1} <= ex, (GC.SPLIT_NAMES[form], ex)
    # group sizes, an empty problem in the middle, a split problem beside a whole-K sibling
    assert {2, 3, 4} <= {len(r.problems) for r in GC.GROUPS}
    assert any(r.plan[1] == GC.NONE and len(r.problems) == 4 and r.problems[1].M == 0 for r in GC.GROUPS)
    assert any({p.split for p in r.problems} >= {GC.WHOLE, s} and r.ksplit > 1 for r in GC.GROUPS
               for s in (GC.SLABS,)) and any({p.split for p in r.problems} >= {GC.WHOLE, GC.TICKETS} for r in GC.GROUPS)
    assert any(p.split == GC.TICKETS and p.bias and p.beta and p.act and r.ksplit > 1 for r in GC.GROUPS
               for p in r.problems)
    # different transposes and loaders inside one launch
    assert any(len({(p.tA, p.tB) for p in r.problems}) >= 3 and {pl[2] for pl in r.plan if pl != GC.NONE} == {0, 1}
               for r in GC.GROUPS)


def test_class_split_group(lib):
    """Mixed shape classes above 0.5 GFLOP: each class is a launch with its own tile; below, one launch, one tile."""
    apart, together = GC.BY_ID["g2-class-split"], GC.BY_ID["g2-class-together"]
    assert apart.problems == together.problems
    flops = lambda r: sum(2.0 * p.M * p.N * p.K * r.batch for p in r.problems)
    assert flops(apart) > 0.5e9 > flops(together)
    assert len({pl[:2] for pl in apart.plan}) == 2 and len({pl[:2] for pl in together.plan}) == 1
    # each class gets the tile it would get alone
    for p, pl in zip(apart.problems, apart.plan):
        assert GC.plan_single(lib, apart.batch, p.M, p.N, p.K, p.tA, p.tB) == pl


def test_edge_values_are_present_for_every_tile(lib):
    for (bm, bn) in GC.TILES:
        rows = [(r, p) for r in GC.SINGLE for p, pl in _tiled(r) if pl[:2] == (bm, bn)]
        Ms, Ns, Ks = {p.M for _, p in rows}, {p.N for _, p in rows}, {p.K for _, p in rows}
        assert set(GC.K_EDGES) <= Ks, (bm, bn, sorted(set(GC.K_EDGES) - Ks))
        want_m = {47, 48, 49, 15, 16} if (bm, bn) == (16, 64) else {bm - 1, bm, bm + 1}
        want_n = {bn - 1, bn} if bn <= 32 else {bn - 1, bn, bn + 1}
        assert want_m <= Ms and want_n <= Ns, (bm, bn, sorted(Ms), sorted(Ns))
        assert any(p.M > bm and p.N > bn for _, p in rows) or bn <= 32            # more than one block each way
        assert any(p.M > bm for _, p in rows)
        assert {p.alpha for _, p in rows} == set(GC.ALPHAS) and {p.beta for _, p in rows} == set(GC.BETAS)
        assert {p.bias for _, p in rows} == {0, 1} and any(p.act for _, p in rows)
        for opt in ("off1", "sB0", "tight"):
            assert any(opt in p.opts for _, p in rows), (bm, bn, opt)
        for r, p in rows:
            L = GC.layout(r, 0)
            assert L.ldc > p.N and L.ldc % 2 == 1
            if "tight" not in p.opts:
                assert L.lda > L.a_cols and L.ldb > L.b_cols and L.lda % 2 == 1 and L.ldb % 2 == 1
        # what the table leaves out cannot be reached at all
        for batch, M, N in GC.UNREACHABLE[(bm, bn)]:
            assert GC.plan_single(lib, batch, M, N)[:2] != (bm, bn), (bm, bn, batch, M, N)
    assert any(p.M == 1 and p.N == 1 for r in GC.SINGLE for p in r.problems)
    assert 140 <= len(GC.ROWS) <= 160


def test_wrapper_refuses_before_any_launch(lib):
    """NULL device pointers throughout: a call that got as far as a launch would fault, these return first."""
    def call(count=1, batch=1, ksplit=1, **kw):
        f = dict(M=8, N=8, K=8, lda=8, ldb=8, ldc=8, alpha=1.0)
        f.update(kw)
        arr = (_lib.GemmProblem * 5)(*[_lib.GemmProblem(**f)] * 5)
        rc = lib.dp_bgemm_group_f32(arr, count, batch, ksplit, None, 0, None)
        return rc, lib.dp_last_error_string()
    some = 16            # a non-NULL address that is never read
    for kw, msg in [(dict(count=5), b"count=5"), (dict(count=0), b"count=0"), (dict(batch=0), b"batch=0"),
                    (dict(batch=65536), b"batch=65536"), (dict(ksplit=0), b"ksplit=0"),
                    (dict(lda=7), b"lda=7"), (dict(ldb=7), b"ldb=7"), (dict(ldc=7), b"ldc=7 < N=8"),
                    (dict(tA=1, M=9, lda=8, ldc=9), b"lda=8"), (dict(tB=1, K=9, lda=9, ldb=8), b"ldb=8"),
                    (dict(split=4), b"split=4"), (dict(act=2), b"act=2"), (dict(M=-1), b"negative"),
                    (dict(split=GC.ATOMIC, bias=some), b"atomic"), (dict(split=GC.ATOMIC, act=1), b"atomic"),
                    (dict(split=GC.ATOMIC, beta=1.0), b"atomic"),
                    (dict(split=GC.SLABS, sK=64, bias=some), b"slab"), (dict(split=GC.SLABS, sK=64, act=1), b"slab"),
                    (dict(split=GC.SLABS, sK=0), b"sK > 0"),
                    (dict(), b"NULL")]:
        rc, text = call(**kw)
        assert rc == -1 and msg in text, (kw, rc, text)
    # tickets without a workspace
    arr = (_lib.GemmProblem * 1)(_lib.GemmProblem(A=some, B=some, C=some, M=8, N=8, K=64, lda=64, ldb=8, ldc=8,
                                                  alpha=1.0, split=GC.TICKETS))
    assert lib.dp_bgemm_group_workspace_bytes(arr, 1, 2, 2) > 0
    assert lib.dp_bgemm_group_f32(arr, 1, 2, 2, None, 0, None) == -2 and b"workspace" in lib.dp_last_error_string()
    plan = (C.c_int * 1)()
    assert lib.dp_bgemm_plan(arr, 1, 2, 2048, plan) == -1 and lib.dp_bgemm_plan(None, 1, 2, 2, plan) == -1


def test_integer_rows_fit_fp32_exactly():
    assert all(GC.exact_fits_fp32(r) for r in GC.ROWS)
    r = GC.BY_ID["tickets-ks4-bias-beta-relu"]
    (d,), ((ref, _, _),) = GC.row_references(r.id, "int")
    assert float(d["opA"].abs().max()) == GC.INT_MAX and bool((d["opA"] == d["opA"].round()).all())
    assert bool((ref.float().double() == ref).all()) and bool((ref > 0).any()) and bool((ref == 0).any())


def test_relu_rows_have_both_signs():
    for r in GC.ROWS:
        for i, p in enumerate(r.problems):
            if p.act:
                for mode in ("int", "real"):
                    d = GC.make_inputs(r, mode)
                    (pre, _, _), = GC.reference(r._replace(problems=(p._replace(act=0),), plan=(r.plan[i],)), [d[i]],
                                                torch.float64)
                    frac = float((pre > 0).double().mean())
                    assert 0.2 < frac < 0.8, (r.id, mode, frac)


def _truncated(t):
    """float32 tensor with the low 13 mantissa bits cleared."""
    return (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def test_reference_sees_a_truncated_operand():
    """In every real-valued row, the fp64 product of A with its low 13 mantissa bits cleared (an operand that went
    through an 11-bit format on its way) misses the bound of test_gpu_gemm.py by at least 10 x."""
    worst = None
    for r in GC.ROWS:
        inputs, refs = GC.row_references(r.id, "real")
        for i, p in enumerate(r.problems):
            if r.plan[i] == GC.NONE:
                continue
            ref, mag, terms = refs[i]
            d = dict(inputs[i], opA=_truncated(inputs[i]["opA"]))
            (got, _, _), = GC.reference(r._replace(problems=(p,), plan=(r.plan[i],)), [d], torch.float64)
            ratio = float(GC.ratio((got - ref).abs(), GC.bound(r, i, mag, terms)).max())
            assert ratio >= 10.0, f"{r.id} problem {i}: a truncated A is only {ratio:.1f} x the bound"
            worst = ratio if worst is None else min(worst, ratio)
    print(f"truncated A: at least {worst:.1f} x the bound in every row")


def test_reference_sees_one_dropped_k_term():
    """At the row with the largest K, the product without its last k term misses the bound by at least 2 x."""
    r, i = max(((r, i) for r in GC.ROWS for i, p in enumerate(r.problems) if r.plan[i] not in (GC.NONE, GC.BF16)),
               key=lambda ri: ri[0].problems[ri[1]].K)
    p = r.problems[i]
    assert p.K >= 500
    inputs, refs = GC.row_references(r.id, "real")
    ref, mag, terms = refs[i]
    d = dict(inputs[i])
    d["opA"] = d["opA"].clone()
    d["opA"][:, :, p.K - 1] = 0.0
    (got, _, _), = GC.reference(r._replace(problems=(p,), plan=(r.plan[i],)), [d], torch.float64)
    ratio = float(((got - ref).abs() / GC.bound(r, i, mag, terms)).min())
    print(f"{r.id} (K = {p.K}): one dropped k term is at least {ratio:.1f} x the bound at every entry")
    assert ratio >= 2.0, ratio
