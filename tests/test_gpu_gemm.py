"""bgemm_kernel (dp_gemm.hip) at every tile, transpose body, loader, split-K form and group layout, and the rows
dp_bgemm_f32 diverts to the split-bf16 kernel: the table of tests/gemm_cases.py (test_gemm_plan_cpu.py asserts what it
reaches).  Single problems go through dp_bgemm_f32, groups through dp_bgemm_group_f32.  Every row runs twice:

integer pass   operands, bias and old C are integers in [-4, 4], so every product and partial sum is exact in fp32
               whatever the order, the tile, the split or the atomics: the whole C allocation — guard rows and columns
               included — must equal the int64 reference with torch.equal.  C is NaN where the contract says it is
               overwritten (beta = 0, no atomics), the workspace is NaN throughout, the padding of A and B is NaN.
               Slab rows: every slab is the exact partial over its own K range, the ranges without any k exact zeros.
real pass      against the float64 product, elementwise
                   |got - ref64| <= (K + ranges + 4) * 2^-24 * mag,  mag = |alpha| |A||B| + |beta| |C0| + |bias|
               the bound of a K-term fma chain, `ranges` partial sums and the epilogue — derived, not measured (a slab
               counts the k of its own range); 2e-6 * mag for the diverted rows, the bar of
               test_bgemm_split_bf16_is_fp32_grade.  The ticket rows run twice and must be bit-identical.

DP_GEMM_ANCHOR_OUT=<file> appends one line per row with its plan and its worst err / (2^-24 * mag)
(profiles/gemm_fp64_anchor.txt is such a file)."""
import os

import pytest
import torch

from graph_pooling_amd import _lib
from tests import gemm_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def S():
    return torch.cuda.current_stream().cuda_stream


def run_row(lib, row, inputs):
    """One launch of the row on fresh device copies of its buffers; returns the flat C allocations (on the CPU)."""
    dev, ptrs = [], []
    for i, p in enumerate(row.problems):
        d, L = inputs[i], GC.layout(row, i)
        a, b, c = d["Abuf"].cuda(), d["Bbuf"].cuda(), d["Cbuf"].cuda()
        bias = d["bias"].cuda() if p.bias else None
        dev.append((a, b, c, bias))
        ptrs.append((a.data_ptr() + 4 * L.off, b.data_ptr() + 4 * L.off, c.data_ptr() + 4 * L.off,
                     bias.data_ptr() if p.bias else None))
    if row.entry == "f32":
        (p,), L, (pa, pb, pc, pbias) = row.problems, GC.layout(row, 0), ptrs[0]
        rc = lib.dp_bgemm_f32(pa, pb, pc, pbias, row.batch, p.M, p.N, p.K, L.lda, L.ldb, L.ldc, L.sA, L.sB, L.sC,
                              p.tA, p.tB, p.alpha, p.beta, p.act, S())
    else:
        arr = GC.struct_of(row, ptrs)
        wsb = lib.dp_bgemm_group_workspace_bytes(arr, len(row.problems), row.batch, row.ksplit)
        ws = torch.full((max(int(wsb), 256),), 0xFF, dtype=torch.uint8, device="cuda")          # NaN throughout
        rc = lib.dp_bgemm_group_f32(arr, len(row.problems), row.batch, row.ksplit, ws.data_ptr(), wsb, S())
    _lib.check(rc, row.id)
    torch.cuda.synchronize()
    return [c.cpu() for _, _, c, _ in dev]


def _plan_text(row):
    return " ".join(pl if isinstance(pl, str) else "<%d,%d>%s/%d" % (pl[0], pl[1], "q" if pl[2] else "d", pl[3])
                    for pl in row.plan)


@pytest.mark.parametrize("row", GC.ROWS, ids=GC.row_id)
def test_integer_pass_is_exact(lib, row):
    assert GC.plan_of(lib, row) == row.plan
    inputs, refs = GC.row_references(row.id, "int")
    got = run_row(lib, row, inputs)
    for i, p in enumerate(row.problems):
        want = inputs[i]["Cbuf"].clone()
        GC.c_view(row, i, want)[...] = refs[i][0].float()
        assert bool((refs[i][0].float().double() == refs[i][0]).all())
        if not torch.equal(got[i], want):
            L = GC.layout(row, i)
            valid = torch.zeros_like(want, dtype=torch.bool)
            GC.c_view(row, i, valid)[...] = True
            diff = ~((got[i] == want) | (got[i].isnan() & want.isnan()))
            n_in, n_guard = int((diff & valid).sum()), int((diff & ~valid).sum())
            idx = diff.nonzero()[:5, 0] - L.off
            where = [(int(k) // (L.c_rows * L.ldc), int(k) // L.ldc % L.c_rows, int(k) % L.ldc) for k in idx]
            pytest.fail(f"{row.id} problem {i} [{_plan_text(row)}]: {n_in} wrong entries, {n_guard} guard words "
                        f"changed; first at (block, row, col) {where}: got "
                        f"{[float(got[i][k + L.off]) for k in idx]}, want {[float(want[k + L.off]) for k in idx]}")


@pytest.mark.parametrize("row", GC.ROWS, ids=GC.row_id)
def test_real_pass_against_fp64(lib, row):
    inputs, refs = GC.row_references(row.id, "real")
    got = run_row(lib, row, inputs)
    worst, bad = [], []
    try:
        for i, p in enumerate(row.problems):
            ref, mag, terms = refs[i]
            g = GC.c_view(row, i, got[i]).double()
            assert torch.isfinite(g).all(), f"{row.id} problem {i}: non-finite values"
            err = (g - ref).abs()
            ulps = float(GC.ratio(err, GC.U * mag).max()) if err.numel() else 0.0
            over = float(GC.ratio(err, GC.bound(row, i, mag, terms)).max()) if err.numel() else 0.0
            worst.append(ulps)
            print(f"{row.id} problem {i} [{_plan_text(row)}]: worst err / (2^-24 mag) {ulps:.3f}, "
                  f"{over:.4f} of the bound (terms {int(terms.max())})")
            if not bool((err <= GC.bound(row, i, mag, terms)).all()):
                bad.append(f"problem {i}: err / (2^-24 mag) {ulps:.3f}, {over:.3f} x the bound")
            # the guards are as they were
            want = inputs[i]["Cbuf"].clone()
            GC.c_view(row, i, want)[...] = GC.c_view(row, i, got[i])
            assert torch.equal(torch.nan_to_num(got[i], nan=1e30), torch.nan_to_num(want, nan=1e30)), \
                f"{row.id} problem {i}: wrote outside its M x N entries"
        assert not bad, f"{row.id} [{_plan_text(row)}]: " + "; ".join(bad)
        if any(p.split == GC.TICKETS for p in row.problems):
            again = run_row(lib, row, inputs)
            for i in range(len(row.problems)):
                assert torch.equal(got[i].view(torch.int32), again[i].view(torch.int32)), \
                    f"{row.id} problem {i}: two runs on the same inputs differ"
    finally:
        path = os.environ.get("DP_GEMM_ANCHOR_OUT")
        if path:
            with open(path, "a") as f:
                f.write(f"{row.id:44s} {_plan_text(row):40s} " + " ".join(f"{w:6.3f}" for w in worst) +
                        ("  OVER THE BOUND (see the test output)" if bad else "") + "\n")


def test_relu_is_visible_on_a_signed_product(lib):
    """The signed sibling of test_gpu_ops.py::test_bgemm_asymmetric_identity_and_strides, whose act = 1 acts on a
    non-negative matrix: A = I against B with both signs, act = 1 must give max(B, 0) and act = 0 B itself."""
    M = N = K = 48
    Bm = (torch.arange(K * 70, dtype=torch.float32).reshape(K, 70) - 1000.0) * 0.25
    assert bool((Bm[:, :N] < 0).any()) and bool((Bm[:, :N] > 0).any())
    Ad, Bd = torch.eye(M).repeat(2, 1, 1).cuda(), Bm.cuda()
    for act in (1, 0):
        Cd = torch.full((2, M, 80), GC.GUARD, device="cuda")
        _lib.check(lib.dp_bgemm_f32(Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), None, 2, M, N, K, K, 70, 80, M * K, 0,
                                    M * 80, 0, 0, 1.0, 0.0, act, S()))
        want = Bm[:, :N].clamp_min(0.0) if act else Bm[:, :N]
        assert torch.equal(Cd[:, :, :N].cpu(), want.repeat(2, 1, 1))
        assert bool((Cd[:, :, N:] == GC.GUARD).all())
