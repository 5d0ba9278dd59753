"""The fp32 GEMM case table shared by test_gemm_plan_cpu.py and test_gpu_gemm.py, the seeded inputs of a row and its CPU
references (exact integers, and the float64 product).

bgemm_kernel (dp_gemm.hip) is compiled for seven workgroup tiles, four transpose bodies and two operand loaders, and
runs K in one of three split forms; the launcher picks the tile from the shapes of the launch and the batch count
(gemm_pick, reported by dp_bgemm_plan).  Every row records the plan it is expected to get, (BM, BN, quad, ranges) per
problem, "bf16" for a problem the launcher diverts to the split-bf16 kernel or "none" for one it does not launch.  The
batch counts were chosen with dp_bgemm_plan, not by hand; test_gemm_plan_cpu.py holds every recorded plan to the query.

SINGLE rows go through dp_bgemm_f32.  Per tile: the eleven K of K_EDGES (4-byte loader below 4, one slot sticking out
past the end, 1 to 5 slabs of 32 through the two-deep prefetch), all four transposes, M and N one below, at and one above
the tile edge, alpha, beta and bias from their sets, a ReLU row, a row with A, B and C one float off their allocation,
a row with B shared by the batch (sB = 0) and a row with lda / ldb equal to the widths (every other row has odd
leading dimensions larger than the widths).  What the launcher's rules make unreachable is left out and asserted
unreachable by the CPU test (UNREACHABLE): N = BN + 1 on the tiles with BN <= 32 (N picks the tile family), M = 17 on
<16,64> (M in (16, 32] always takes <32,64>; the table has 47, 48, 49 instead) and a 1 x 1 problem anywhere but <64,16>.

GROUP rows go through dp_bgemm_group_f32: 2, 3 and 4 problems of different shape, transposes and loader, an empty
problem in the middle, a group the launcher splits by shape class, and the three split-K forms at ksplit 2, 4 and 8 with
K an exact multiple of ksplit * 32, one more than that, and K = 40 at ksplit 8 (two ranges have work)."""
import collections
import ctypes as C
import functools

import torch

from graph_pooling_amd import _lib

WHOLE, ATOMIC, SLABS, TICKETS = _lib.GEMM_WHOLE_K, _lib.GEMM_ATOMIC, _lib.GEMM_SLABS, _lib.GEMM_TICKETS
SPLIT_NAMES = {WHOLE: "whole", ATOMIC: "atomic", SLABS: "slabs", TICKETS: "tickets"}
TILES = ((64, 16), (128, 32), (64, 32), (32, 32), (64, 64), (32, 64), (16, 64))
K_EDGES = (1, 3, 4, 5, 31, 32, 33, 64, 65, 97, 129)
ALPHAS, BETAS = (1.0, 0.5, -2.0), (0.0, 1.0, 2.0)
KT = 32                      # K slab of the kernel: split-K ranges are whole slabs
BF16, NONE = "bf16", "none"
U = 2.0 ** -24               # unit roundoff of fp32

# opts (a string of words): "tight" lda / ldb equal the widths; "off1" A, B and C start one float into their allocation;
# "sB0" one B for the whole batch (stride 0).  An ATOMIC problem always accumulates into C: its `beta` is 1 in the
# reference and in `mag`, and 0 in the struct handed to the library (which refuses any other value there).
P = collections.namedtuple("P", "tA tB M N K alpha beta bias act split opts")
Row = collections.namedtuple("Row", "id entry batch ksplit problems plan")     # entry: "f32" | "group"


def _s(batch, tA, tB, M, N, K, alpha, beta, bias, act, opts, plan):
    rid = "%s-%dx%dx%d-b%d-a%g-c%g%s%s%s" % ("NT"[tA] + "NT"[tB], M, N, K, batch, alpha, beta, "-bias" if bias else "",
                                              "-relu" if act else "", "-" + opts.replace(" ", "-") if opts else "")
    return Row(rid, "f32", batch, 1, (P(tA, tB, M, N, K, alpha, beta, bias, act, WHOLE, opts),), (plan,))


def _g(name, batch, ksplit, problems, plan):
    return Row(name, "group", batch, ksplit, tuple(P(*p) for p in problems), tuple(plan))


# ---------------------------------------------------------------------------------------------------- single problems
# (batch, tA, tB, M, N, K, alpha, beta, bias, act, opts, plan)
SINGLE = [_s(*r) for r in [
    # <64,16>: N <= 16
    (2, 0, 0, 63, 15, 1, 1.0, 0.0, 0, 0, "", (64, 16, 0, 1)),
    (2, 1, 0, 64, 16, 3, 0.5, 1.0, 1, 0, "", (64, 16, 1, 1)),
    (2, 0, 1, 65, 15, 4, -2.0, 2.0, 0, 0, "", (64, 16, 1, 1)),
    (2, 1, 1, 63, 16, 5, 1.0, 1.0, 1, 0, "", (64, 16, 1, 1)),
    (2, 0, 0, 64, 15, 31, 0.5, 2.0, 0, 0, "", (64, 16, 1, 1)),
    (2, 1, 0, 65, 16, 32, -2.0, 0.0, 1, 0, "", (64, 16, 1, 1)),
    (2, 0, 1, 63, 15, 33, 1.0, 2.0, 0, 0, "", (64, 16, 1, 1)),
    (2, 1, 1, 64, 16, 64, 0.5, 0.0, 1, 0, "", (64, 16, 1, 1)),
    (2, 0, 0, 65, 15, 65, -2.0, 1.0, 0, 0, "", (64, 16, 1, 1)),
    (2, 1, 0, 63, 16, 97, 1.0, 0.0, 1, 0, "", (64, 16, 1, 1)),
    (2, 0, 1, 64, 15, 129, 0.5, 1.0, 0, 0, "", (64, 16, 1, 1)),
    (2, 1, 0, 129, 16, 33, -2.0, 1.0, 1, 1, "", (64, 16, 1, 1)),
    (2, 0, 1, 129, 15, 65, 1.0, 1.0, 1, 0, "off1", (64, 16, 1, 1)),
    (3, 1, 1, 65, 16, 97, 1.0, 2.0, 0, 0, "sB0", (64, 16, 1, 1)),
    (2, 0, 0, 129, 16, 64, 0.5, 0.0, 1, 0, "tight", (64, 16, 1, 1)),
    (2, 0, 0, 1, 1, 33, 1.0, 1.0, 1, 0, "", (64, 16, 0, 1)),
    # <128,32>: N in (16, 32], M > 64, >= 512 workgroups of 128 x 32
    (512, 0, 0, 127, 31, 1, 1.0, 0.0, 0, 0, "", (128, 32, 0, 1)),
    (512, 1, 0, 128, 32, 3, 0.5, 1.0, 1, 0, "", (128, 32, 1, 1)),
    (256, 0, 1, 129, 31, 4, -2.0, 2.0, 0, 0, "", (128, 32, 1, 1)),
    (512, 1, 1, 127, 32, 5, 1.0, 1.0, 1, 0, "", (128, 32, 1, 1)),
    (512, 0, 0, 128, 31, 31, 0.5, 2.0, 0, 0, "", (128, 32, 1, 1)),
    (256, 1, 0, 129, 32, 32, -2.0, 0.0, 1, 0, "", (128, 32, 1, 1)),
    (512, 0, 1, 127, 31, 33, 1.0, 2.0, 0, 0, "", (128, 32, 1, 1)),
    (256, 1, 1, 129, 32, 64, 0.5, 0.0, 1, 0, "", (128, 32, 1, 1)),
    (256, 0, 0, 129, 31, 65, -2.0, 1.0, 0, 0, "", (128, 32, 1, 1)),
    (256, 1, 0, 129, 32, 97, 1.0, 0.0, 1, 0, "", (128, 32, 1, 1)),
    (256, 0, 1, 129, 31, 129, 0.5, 1.0, 0, 0, "", (128, 32, 1, 1)),
    (256, 1, 0, 129, 32, 33, -2.0, 1.0, 1, 1, "", (128, 32, 1, 1)),
    (256, 0, 1, 129, 31, 65, 1.0, 1.0, 1, 0, "off1", (128, 32, 1, 1)),
    (171, 1, 1, 257, 32, 97, 1.0, 2.0, 0, 0, "sB0", (128, 32, 1, 1)),
    (256, 0, 0, 129, 32, 64, 0.5, 0.0, 1, 0, "tight", (128, 32, 1, 1)),
    # <64,32>: N in (16, 32], M > 32, >= 512 workgroups of 64 x 32 and not enough of 128 x 32
    (512, 0, 0, 63, 31, 1, 1.0, 0.0, 0, 0, "", (64, 32, 0, 1)),
    (512, 1, 0, 64, 32, 3, 0.5, 1.0, 1, 0, "", (64, 32, 1, 1)),
    (256, 0, 1, 65, 31, 4, -2.0, 2.0, 0, 0, "", (64, 32, 1, 1)),
    (512, 1, 1, 63, 32, 5, 1.0, 1.0, 1, 0, "", (64, 32, 1, 1)),
    (512, 0, 0, 64, 31, 31, 0.5, 2.0, 0, 0, "", (64, 32, 1, 1)),
    (256, 1, 0, 65, 32, 32, -2.0, 0.0, 1, 0, "", (64, 32, 1, 1)),
    (512, 0, 1, 63, 31, 33, 1.0, 2.0, 0, 0, "", (64, 32, 1, 1)),
    (256, 1, 1, 65, 32, 64, 0.5, 0.0, 1, 0, "", (64, 32, 1, 1)),
    (256, 0, 0, 65, 31, 65, -2.0, 1.0, 0, 0, "", (64, 32, 1, 1)),
    (256, 1, 0, 65, 32, 97, 1.0, 0.0, 1, 0, "", (64, 32, 1, 1)),
    (256, 0, 1, 65, 31, 129, 0.5, 1.0, 0, 0, "", (64, 32, 1, 1)),
    (256, 1, 0, 65, 32, 33, -2.0, 1.0, 1, 1, "", (64, 32, 1, 1)),
    (256, 0, 1, 65, 31, 65, 1.0, 1.0, 1, 0, "off1", (64, 32, 1, 1)),
    (171, 1, 1, 129, 32, 97, 1.0, 2.0, 0, 0, "sB0", (64, 32, 1, 1)),
    (256, 0, 0, 65, 32, 64, 0.5, 0.0, 1, 0, "tight", (64, 32, 1, 1)),
    # <32,32>: N in (16, 32] at a small batch
    (2, 0, 0, 31, 31, 1, 1.0, 0.0, 0, 0, "", (32, 32, 0, 1)),
    (2, 1, 0, 32, 32, 3, 0.5, 1.0, 1, 0, "", (32, 32, 1, 1)),
    (2, 0, 1, 33, 31, 4, -2.0, 2.0, 0, 0, "", (32, 32, 1, 1)),
    (2, 1, 1, 31, 32, 5, 1.0, 1.0, 1, 0, "", (32, 32, 1, 1)),
    (2, 0, 0, 32, 31, 31, 0.5, 2.0, 0, 0, "", (32, 32, 1, 1)),
    (2, 1, 0, 33, 32, 32, -2.0, 0.0, 1, 0, "", (32, 32, 1, 1)),
    (2, 0, 1, 31, 31, 33, 1.0, 2.0, 0, 0, "", (32, 32, 1, 1)),
    (2, 1, 1, 32, 32, 64, 0.5, 0.0, 1, 0, "", (32, 32, 1, 1)),
    (2, 0, 0, 33, 31, 65, -2.0, 1.0, 0, 0, "", (32, 32, 1, 1)),
    (2, 1, 0, 31, 32, 97, 1.0, 0.0, 1, 0, "", (32, 32, 1, 1)),
    (2, 0, 1, 32, 31, 129, 0.5, 1.0, 0, 0, "", (32, 32, 1, 1)),
    (2, 1, 0, 65, 32, 33, -2.0, 1.0, 1, 1, "", (32, 32, 1, 1)),
    (2, 0, 1, 65, 31, 65, 1.0, 1.0, 1, 0, "off1", (32, 32, 1, 1)),
    (3, 1, 1, 97, 32, 97, 1.0, 2.0, 0, 0, "sB0", (32, 32, 1, 1)),
    (2, 0, 0, 65, 32, 64, 0.5, 0.0, 1, 0, "tight", (32, 32, 1, 1)),
    # <64,64>: N > 32, M > 32, >= 512 workgroups of 64 x 64
    (512, 0, 0, 63, 63, 1, 1.0, 0.0, 0, 0, "", (64, 64, 0, 1)),
    (512, 1, 0, 64, 64, 3, 0.5, 1.0, 1, 0, "", (64, 64, 1, 1)),
    (128, 0, 1, 65, 65, 4, -2.0, 2.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 1, 1, 63, 65, 5, 1.0, 1.0, 1, 0, "", (64, 64, 1, 1)),
    (256, 0, 0, 65, 63, 31, 0.5, 2.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 1, 0, 65, 64, 32, -2.0, 0.0, 1, 0, "", (64, 64, 1, 1)),
    (256, 0, 1, 64, 65, 33, 1.0, 2.0, 0, 0, "", (64, 64, 1, 1)),
    (128, 1, 1, 65, 65, 64, 0.5, 0.0, 1, 0, "", (64, 64, 1, 1)),
    (128, 0, 0, 65, 65, 65, -2.0, 1.0, 0, 0, "", (64, 64, 1, 1)),
    (128, 1, 0, 65, 65, 97, 1.0, 0.0, 1, 0, "", (64, 64, 1, 1)),
    (128, 0, 1, 65, 65, 129, 0.5, 1.0, 0, 0, "", (64, 64, 1, 1)),
    (128, 1, 0, 65, 65, 33, -2.0, 1.0, 1, 1, "", (64, 64, 1, 1)),
    (128, 0, 1, 65, 65, 65, 1.0, 1.0, 1, 0, "off1", (64, 64, 1, 1)),
    (86, 1, 1, 129, 65, 97, 1.0, 2.0, 0, 0, "sB0", (64, 64, 1, 1)),
    (128, 0, 0, 65, 65, 64, 0.5, 0.0, 1, 0, "tight", (64, 64, 1, 1)),
    # <32,64>: N > 32 and M in (16, 32] at any batch, or M > 32 with >= 512 workgroups of 32 x 64 but not of 64 x 64
    (2, 0, 0, 31, 63, 1, 1.0, 0.0, 0, 0, "", (32, 64, 0, 1)),
    (2, 1, 0, 32, 64, 3, 0.5, 1.0, 1, 0, "", (32, 64, 1, 1)),
    (128, 0, 1, 33, 65, 4, -2.0, 2.0, 0, 0, "", (32, 64, 1, 1)),
    (2, 1, 1, 31, 65, 5, 1.0, 1.0, 1, 0, "", (32, 64, 1, 1)),
    (2, 0, 0, 32, 63, 31, 0.5, 2.0, 0, 0, "", (32, 64, 1, 1)),
    (256, 1, 0, 33, 64, 32, -2.0, 0.0, 1, 0, "", (32, 64, 1, 1)),
    (2, 0, 1, 31, 63, 33, 1.0, 2.0, 0, 0, "", (32, 64, 1, 1)),
    (2, 1, 1, 32, 64, 64, 0.5, 0.0, 1, 0, "", (32, 64, 1, 1)),
    (128, 0, 0, 33, 65, 65, -2.0, 1.0, 0, 0, "", (32, 64, 1, 1)),
    (2, 1, 0, 17, 65, 97, 1.0, 0.0, 1, 0, "", (32, 64, 1, 1)),
    (128, 0, 1, 33, 65, 129, 0.5, 1.0, 0, 0, "", (32, 64, 1, 1)),
    (128, 1, 0, 33, 65, 33, -2.0, 1.0, 1, 1, "", (32, 64, 1, 1)),
    (128, 0, 1, 33, 65, 65, 1.0, 1.0, 1, 0, "off1", (32, 64, 1, 1)),
    (3, 1, 1, 31, 129, 97, 1.0, 2.0, 0, 0, "sB0", (32, 64, 1, 1)),
    (128, 0, 0, 33, 65, 64, 0.5, 0.0, 1, 0, "tight", (32, 64, 1, 1)),
    # <16,64>: N > 32 and M <= 16, or M > 32 at a small batch
    (2, 0, 0, 15, 63, 1, 1.0, 0.0, 0, 0, "", (16, 64, 0, 1)),
    (2, 1, 0, 16, 64, 3, 0.5, 1.0, 1, 0, "", (16, 64, 1, 1)),
    (2, 0, 1, 47, 65, 4, -2.0, 2.0, 0, 0, "", (16, 64, 1, 1)),
    (2, 1, 1, 48, 63, 5, 1.0, 1.0, 1, 0, "", (16, 64, 1, 1)),
    (2, 0, 0, 49, 64, 31, 0.5, 2.0, 0, 0, "", (16, 64, 1, 1)),
    (2, 1, 0, 15, 65, 32, -2.0, 0.0, 1, 0, "", (16, 64, 1, 1)),
    (2, 0, 1, 16, 63, 33, 1.0, 2.0, 0, 0, "", (16, 64, 1, 1)),
    (2, 1, 1, 47, 64, 64, 0.5, 0.0, 1, 0, "", (16, 64, 1, 1)),
    (2, 0, 0, 48, 65, 65, -2.0, 1.0, 0, 0, "", (16, 64, 1, 1)),
    (2, 1, 0, 49, 63, 97, 1.0, 0.0, 1, 0, "", (16, 64, 1, 1)),
    (2, 0, 1, 33, 64, 129, 0.5, 1.0, 0, 0, "", (16, 64, 1, 1)),
    (2, 1, 0, 49, 65, 33, -2.0, 1.0, 1, 1, "", (16, 64, 1, 1)),
    (2, 0, 1, 33, 129, 65, 1.0, 1.0, 1, 0, "off1", (16, 64, 1, 1)),
    (3, 1, 1, 65, 65, 97, 1.0, 2.0, 0, 0, "sB0", (16, 64, 1, 1)),
    (85, 0, 0, 65, 65, 64, 0.5, 0.0, 1, 0, "tight", (16, 64, 1, 1)),
    # diverted by dp_bgemm_f32 to the split-bf16 kernel: M >= 96, N >= 80 or N in [48, 64], K >= 40 and >= 256 tiles of
    # 128 x 128 (128 x 64 for the narrow N) ...
    (256, 0, 0, 96, 80, 40, 1.0, 0.0, 0, 0, "", BF16),
    (256, 1, 0, 96, 48, 40, 1.0, 1.0, 0, 0, "", BF16),
    # ... and one row just outside each of those limits, which stays on the fp32 kernel
    (256, 0, 0, 95, 80, 40, 1.0, 0.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 0, 0, 96, 79, 40, 1.0, 0.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 1, 0, 96, 47, 40, 1.0, 1.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 1, 0, 96, 65, 40, 1.0, 1.0, 0, 0, "", (64, 64, 1, 1)),
    (256, 0, 0, 96, 80, 39, 1.0, 0.0, 0, 0, "", (64, 64, 1, 1)),
    (255, 0, 0, 96, 80, 40, 1.0, 0.0, 0, 0, "", (64, 64, 1, 1)),
]]

# ------------------------------------------------------------------------------------------------------------- groups
# problem: (tA, tB, M, N, K, alpha, beta, bias, act, split, opts)
GROUPS = [
    # several problems in one grid: the tile0 prefix search, one tile shape for all
    _g("g2-mixed", 3, 1, [(0, 0, 20, 40, 50, 1.0, 0.0, 1, 0, WHOLE, ""),
                          (1, 0, 31, 17, 3, 0.5, 1.0, 0, 0, WHOLE, "")], [(32, 64, 1, 1), (32, 64, 1, 1)]),
    _g("g3-mixed", 2, 1, [(0, 1, 65, 20, 33, -2.0, 2.0, 1, 0, WHOLE, ""),
                          (0, 0, 7, 30, 2, 1.0, 0.0, 0, 0, WHOLE, "off1"),
                          (1, 1, 31, 9, 70, 1.0, 1.0, 0, 1, WHOLE, "")],
       [(32, 32, 1, 1), (32, 32, 0, 1), (32, 32, 1, 1)]),
    _g("g4-mixed", 2, 1, [(0, 0, 50, 60, 89, 1.0, 1.0, 0, 0, WHOLE, ""),
                          (0, 1, 89, 50, 60, 1.0, 0.0, 1, 1, WHOLE, ""),
                          (1, 0, 3, 70, 45, 0.5, 0.0, 0, 0, WHOLE, "sB0"),
                          (1, 1, 60, 2, 37, -2.0, 2.0, 1, 0, WHOLE, "")],
       [(16, 64, 1, 1), (16, 64, 1, 1), (16, 64, 0, 1), (16, 64, 1, 1)]),
    _g("g4-empty-in-the-middle", 2, 1, [(0, 0, 40, 12, 20, 1.0, 0.0, 1, 0, WHOLE, ""),
                                        (0, 0, 0, 12, 20, 1.0, 0.0, 0, 0, WHOLE, ""),
                                        (1, 0, 70, 16, 33, 0.5, 1.0, 0, 0, WHOLE, ""),
                                        (0, 1, 5, 3, 9, 1.0, 2.0, 0, 0, WHOLE, "")],
       [(64, 16, 1, 1), NONE, (64, 16, 1, 1), (64, 16, 1, 1)]),
    # mixed shape classes worth more than 0.5 GFLOP: one launch per class, each with its own tile ...
    _g("g2-class-split", 128, 1, [(0, 0, 128, 40, 400, 1.0, 0.0, 0, 0, WHOLE, ""),
                                  (1, 0, 20, 20, 400, 1.0, 1.0, 0, 0, WHOLE, "")], [(32, 64, 1, 1), (32, 32, 1, 1)]),
    # ... and the same pair under the threshold: one launch, one tile
    _g("g2-class-together", 32, 1, [(0, 0, 128, 40, 400, 1.0, 0.0, 0, 0, WHOLE, ""),
                                    (1, 0, 20, 20, 400, 1.0, 1.0, 0, 0, WHOLE, "")], [(16, 64, 1, 1), (16, 64, 1, 1)]),
    # split-K with float atomics into a non-zero C
    _g("atomic-ks2-K64", 3, 2, [(1, 0, 20, 30, 64, 1.0, 1.0, 0, 0, ATOMIC, "")], [(32, 32, 1, 2)]),
    _g("atomic-ks4-K129", 2, 4, [(0, 1, 50, 12, 129, 0.5, 1.0, 0, 0, ATOMIC, "")], [(64, 16, 1, 3)]),
    _g("atomic-ks8-K256", 2, 8, [(1, 0, 60, 60, 256, -2.0, 1.0, 0, 0, ATOMIC, "")], [(16, 64, 1, 8)]),
    _g("atomic-ks8-K257", 2, 8, [(1, 1, 33, 40, 257, 1.0, 1.0, 0, 0, ATOMIC, "")], [(16, 64, 1, 5)]),
    _g("atomic-ks8-K40", 3, 8, [(1, 0, 20, 70, 40, 1.0, 1.0, 0, 0, ATOMIC, "")], [(32, 64, 1, 2)]),
    # split-K into slabs at C + ks * sK: every range writes, the ones without any k write zeros
    _g("slabs-ks2-K64", 3, 2, [(1, 0, 20, 30, 64, 1.0, 0.0, 0, 0, SLABS, "")], [(32, 32, 1, 2)]),
    _g("slabs-ks4-K129", 2, 4, [(1, 0, 50, 12, 129, 0.5, 0.0, 0, 0, SLABS, "")], [(64, 16, 1, 4)]),
    _g("slabs-ks8-K256", 2, 8, [(1, 0, 60, 60, 256, -2.0, 0.0, 0, 0, SLABS, "")], [(16, 64, 1, 8)]),
    _g("slabs-ks8-K257", 2, 8, [(0, 1, 33, 40, 257, 1.0, 0.0, 0, 0, SLABS, "")], [(16, 64, 1, 8)]),
    _g("slabs-ks8-K40", 3, 8, [(1, 0, 20, 70, 40, 1.0, 0.0, 0, 0, SLABS, "")], [(32, 64, 1, 8)]),
    _g("slabs-ks4-K40-beta", 2, 4, [(1, 0, 33, 20, 40, 1.0, 2.0, 0, 0, SLABS, "")], [(32, 32, 1, 4)]),
    # deterministic split-K: partials, tickets, the last range applies the whole epilogue once
    _g("tickets-ks2-K64", 3, 2, [(1, 0, 20, 30, 64, 1.0, 0.0, 0, 0, TICKETS, "")], [(32, 32, 1, 2)]),
    _g("tickets-ks4-K129", 2, 4, [(1, 0, 50, 12, 129, 0.5, 1.0, 0, 0, TICKETS, "")], [(64, 16, 1, 3)]),
    _g("tickets-ks8-K256", 2, 8, [(1, 0, 60, 60, 256, -2.0, 2.0, 1, 0, TICKETS, "")], [(16, 64, 1, 8)]),
    _g("tickets-ks8-K257", 2, 8, [(1, 1, 33, 40, 257, 1.0, 0.0, 0, 0, TICKETS, "")], [(16, 64, 1, 5)]),
    _g("tickets-ks8-K40", 3, 8, [(0, 0, 20, 70, 40, 1.0, 0.0, 0, 0, TICKETS, "")], [(32, 64, 1, 2)]),
    _g("tickets-ks4-bias-beta-relu", 2, 4, [(1, 0, 70, 33, 200, -2.0, 2.0, 1, 1, TICKETS, "")], [(16, 64, 1, 4)]),
    _g("tickets-ks1", 2, 1, [(1, 0, 20, 30, 64, 1.0, 1.0, 1, 0, TICKETS, "")], [(32, 32, 1, 1)]),
    # the pooled products S^T Z and T^T S in one launch, both with tickets
    _g("tickets-ks4-pair", 3, 4, [(1, 0, 12, 30, 300, 1.0, 0.0, 0, 0, TICKETS, ""),
                                  (1, 0, 12, 12, 300, 1.0, 0.0, 0, 0, TICKETS, "")],
       [(32, 32, 1, 4), (32, 32, 1, 4)]),
    # a split problem next to a sibling that walks its whole K in one workgroup
    _g("slabs-ks4-with-whole-sibling", 3, 4, [(1, 0, 10, 30, 260, 1.0, 0.0, 0, 0, SLABS, ""),
                                              (0, 0, 260, 30, 10, 1.0, 0.0, 0, 0, WHOLE, "sB0")],
       [(32, 32, 1, 4), (32, 32, 1, 1)]),
    _g("atomic-ks2-with-whole-sibling", 2, 2, [(1, 0, 30, 20, 100, 1.0, 0.0, 0, 0, SLABS, ""),
                                               (0, 1, 100, 30, 20, 1.0, 0.0, 1, 1, WHOLE, ""),
                                               (0, 1, 100, 30, 20, 1.0, 1.0, 0, 0, ATOMIC, "")],
       [(32, 32, 1, 2), (32, 32, 1, 1), (32, 32, 1, 1)]),
    _g("tickets-ks8-with-whole-sibling", 2, 8, [(0, 0, 65, 40, 3, 0.5, 1.0, 1, 1, WHOLE, ""),
                                                (1, 0, 40, 65, 500, 1.0, 1.0, 0, 0, TICKETS, "")],
       [(16, 64, 0, 1), (16, 64, 1, 8)]),
]

ROWS = SINGLE + GROUPS
BY_ID = {r.id: r for r in ROWS}

# what the launcher's rules put out of reach, as (batch, M, N): the tile each gets instead is asserted by the CPU test
UNREACHABLE = {
    (64, 16): [(2, 64, 17), (512, 64, 17)],             # N = BN + 1 moves to the N <= 32 family
    (128, 32): [(512, 128, 33), (512, 1, 1)],
    (64, 32): [(512, 64, 33), (512, 1, 1)],
    (32, 32): [(2, 32, 33), (2, 1, 1)],
    (64, 64): [(512, 1, 1)],
    (32, 64): [(2, 1, 1)],
    (16, 64): [(2, 17, 64), (1, 17, 64), (2, 1, 1)],     # M in (16, 32] always takes <32,64>
}


def row_id(row):
    return row.id


# ------------------------------------------------------------------------------------------------------------ layouts
def _odd_ld(width):
    """A leading dimension larger than the width and odd: no row after the first is 16-byte aligned."""
    return width + (1 if width % 2 == 0 else 2)


Layout = collections.namedtuple("Layout", "a_rows a_cols lda b_rows b_cols ldb ldc c_rows nb_b off slabs sK sA sB sC")


def layout(row, i):
    """Extents of problem i's buffers.  A is [batch][a_rows][lda], B [nb_b][b_rows][ldb], C [batch][slabs][M + 1][ldc]:
    one guard row behind every M rows and ldc - N >= 1 guard columns; `off` floats lie in front of each of them."""
    p = row.problems[i]
    a_rows, a_cols = (p.K, p.M) if p.tA else (p.M, p.K)
    b_rows, b_cols = (p.N, p.K) if p.tB else (p.K, p.N)
    tight = "tight" in p.opts
    lda = max(a_cols, 1) if tight else _odd_ld(a_cols)
    ldb = max(b_cols, 1) if tight else _odd_ld(b_cols)
    ldc = _odd_ld(p.N)
    slabs = row.ksplit if p.split == SLABS else 1
    sK = (p.M + 1) * ldc
    return Layout(a_rows, a_cols, lda, b_rows, b_cols, ldb, ldc, p.M + 1, 1 if "sB0" in p.opts else row.batch,
                  1 if "off1" in p.opts else 0, slabs, sK if p.split == SLABS else 0, a_rows * lda,
                  0 if "sB0" in p.opts else b_rows * ldb, slabs * sK)


def k_ranges(p, ksplit):
    """[(kbeg, kend)] of the K ranges a problem is cut into (whole slabs of KT); empty ranges have kbeg >= kend."""
    if p.split == WHOLE or ksplit <= 1:
        return [(0, p.K)]
    kchunk = -(-p.K // (ksplit * KT)) * KT
    return [(ks * kchunk, min(p.K, (ks + 1) * kchunk)) for ks in range(ksplit)]


def ranges_with_work(p, ksplit):
    return max(1, sum(1 for b, e in k_ranges(p, ksplit) if e > b))


def struct_of(row, ptrs=None):
    """The dp_gemm_problem array of a row; ptrs[i] = (A, B, C, bias) addresses (None: NULL operands, and a non-NULL
    marker where the problem has a bias, for the plan query, which reads no pointer)."""
    arr = (_lib.GemmProblem * len(row.problems))()
    for i, p in enumerate(row.problems):
        L = layout(row, i)
        a, b, c, bias = ptrs[i] if ptrs else (None, None, None, 16 if p.bias else None)
        arr[i] = _lib.GemmProblem(A=a, B=b, C=c, bias=bias, M=p.M, N=p.N, K=p.K, lda=L.lda, ldb=L.ldb, ldc=L.ldc,
                                  sA=L.sA, sB=L.sB, sC=L.sC, tA=p.tA, tB=p.tB, alpha=p.alpha,
                                  beta=0.0 if p.split == ATOMIC else p.beta, act=p.act, split=p.split, sK=L.sK)
    return arr


def plan_of(lib, row):
    """The launcher's answer for a row, in the form the table records it."""
    out = (C.c_int * len(row.problems))()
    rc = lib.dp_bgemm_plan(struct_of(row), len(row.problems), row.batch, row.ksplit, out)
    assert rc == 0, lib.dp_last_error_string()
    return tuple(NONE if v == _lib.GEMM_PLAN_NONE else BF16 if v == _lib.GEMM_PLAN_SPLIT_BF16
                 else _lib.gemm_plan_decode(v) for v in out)


def plan_single(lib, batch, M, N, K=8, tA=0, tB=0):
    return plan_of(lib, _s(batch, tA, tB, M, N, K, 1.0, 0.0, 0, 0, "", None))[0]


# ------------------------------------------------------------------------------------------------------------- inputs
GUARD = -777.0          # what the guard rows and columns of C hold; NaN fills what the contract says is overwritten
INT_MAX = 4


def _signed_unit(shape, g):
    """Magnitudes uniform in [0.5, 1]."""
    return 0.5 + 0.5 * torch.rand(shape, generator=g)


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def make_inputs(row, mode):
    """Per problem {A, B, C0, bias, Cbuf, Abuf, Bbuf}: float32 CPU tensors.  A, B are the operands as stored
    ([batch][rows][cols]); C0 [batch][slabs][M][N] the old C; the *buf tensors are the flat allocations: NaN in the
    padding of A and B, GUARD in the guards of C, `off` floats of padding in front.

    mode "int": every value an integer in [-4, 4], so every product and partial sum is exact in fp32 in any order.
    mode "real": magnitudes uniform in [0.5, 1] with random signs s[m] u[k] for A and u[k] t[n] for B: the operands'
    signs are random, every output is a sum of K terms of ONE sign s[m] t[n] (both signs occur across the output), so
    nothing cancels and the derived bound (K + ranges + 4) u mag is a bound relative to the entry itself."""
    assert mode in ("int", "real")
    out = []
    for i, p in enumerate(row.problems):
        L = layout(row, i)
        g = torch.Generator().manual_seed(7919 * (ROWS.index(row) + 1) + 101 * i + (0 if mode == "int" else 53))
        B_ = row.batch

        def values(shape, sign=None):
            if mode == "int":
                return torch.randint(-INT_MAX, INT_MAX + 1, shape, generator=g).float()
            return _signed_unit(shape, g) * (sign if sign is not None else _signs(shape, g))
        sm, uk, tn = _signs((B_, p.M, 1), g), _signs((B_, 1, p.K), g), _signs((B_, 1, p.N), g)
        if L.nb_b == 1:                 # one B for the whole batch: its signs cannot depend on the graph
            uk, tn = uk[:1].expand(B_, 1, p.K), tn[:1].expand(B_, 1, p.N)
        opA = values((B_, p.M, p.K), sm * uk)                     # op(A): [M][K]
        opB = values((L.nb_b, p.K, p.N), (uk.transpose(1, 2) * tn)[:L.nb_b])
        A = opA.transpose(1, 2).contiguous() if p.tA else opA
        Bm = opB.transpose(1, 2).contiguous() if p.tB else opB
        C0 = values((B_, L.slabs, p.M, p.N))
        bias = values((p.N,)) if p.bias else None

        def buf(t, rows_alloc, ld, fill):
            nb = t.shape[0] * (t.shape[1] if t.dim() == 4 else 1)
            flat = torch.full((L.off + nb * rows_alloc * ld,), fill)
            v = flat[L.off:].view(nb, rows_alloc, ld)
            v[:, :t.shape[-2], :t.shape[-1]] = t.reshape(nb, t.shape[-2], t.shape[-1])
            return flat
        reads_c = p.split == ATOMIC or p.beta != 0.0
        cbuf = buf(C0 if reads_c else torch.full_like(C0, float("nan")), L.c_rows, L.ldc, GUARD)
        out.append(dict(A=A, B=Bm, opA=opA, opB=opB, C0=C0, bias=bias, reads_c=reads_c,
                        Abuf=buf(A, L.a_rows, L.lda, float("nan")), Bbuf=buf(Bm, L.b_rows, L.ldb, float("nan")),
                        Cbuf=cbuf))
    return out


def c_view(row, i, flat):
    """[batch][slabs][M][N] view of problem i's valid entries inside its flat C allocation."""
    p, L = row.problems[i], layout(row, i)
    return flat[L.off:].view(row.batch, L.slabs, L.c_rows, L.ldc)[:, :, :p.M, :p.N]


# --------------------------------------------------------------------------------------------------------- references
def reference(row, inputs, dtype):
    """Per problem (ref, mag, terms): the result [batch][slabs][M][N] in float64 computed in `dtype` (torch.int64 for
    the integer pass: exact; torch.float64 for the real-valued pass), mag = |alpha| |A||B| + |beta| |C0| + |bias| and
    terms = K + ranges + 4, the rounding steps of the bound (a slab counts the k of its own range, in one range)."""
    res = []
    for i, p in enumerate(row.problems):
        d = inputs[i]
        beta = 1.0 if p.split == ATOMIC else p.beta
        opA, opB = d["opA"].to(dtype), d["opB"].to(dtype).expand(row.batch, p.K, p.N)
        spans = k_ranges(p, row.ksplit) if p.split == SLABS else [(0, p.K)]
        prods, mags, terms = [], [], []
        for kb, ke in spans:
            kb, ke = min(kb, p.K), max(min(ke, p.K), min(kb, p.K))
            prods.append((opA[:, :, kb:ke] @ opB[:, kb:ke, :]).double())
            mags.append(opA[:, :, kb:ke].abs().double() @ opB[:, kb:ke, :].abs().double())
            terms.append((ke - kb) + (1 if p.split == SLABS else ranges_with_work(p, row.ksplit)) + 4)
        prod, mag = torch.stack(prods, 1), torch.stack(mags, 1)
        c0 = d["C0"].double()
        ref = p.alpha * prod + (beta * c0 if beta != 0.0 else 0.0)
        mag = abs(p.alpha) * mag + abs(beta) * c0.abs()
        if p.bias:
            ref = ref + d["bias"].double()
            mag = mag + d["bias"].double().abs()
        if p.act:
            ref = ref.clamp_min(0.0)
        res.append((ref, mag, torch.tensor(terms, dtype=torch.float64).view(1, -1, 1, 1)))
    return res


@functools.lru_cache(maxsize=4)
def row_references(rid, mode):
    """(inputs, references) of a row for one pass; computed once per process and pass."""
    row = BY_ID[rid]
    inputs = make_inputs(row, mode)
    return inputs, reference(row, inputs, torch.int64 if mode == "int" else torch.float64)


def exact_fits_fp32(row):
    """The integer pass's exactness condition: |alpha| K max|a| max|b| + |beta| max|c0| + max|bias| < 2^24."""
    return all(abs(p.alpha) * p.K * INT_MAX * INT_MAX + (1.0 if p.split == ATOMIC else abs(p.beta)) * INT_MAX
               + INT_MAX < 2 ** 24 for p in row.problems)


DIVERTED_RTOL = 2e-6        # the bar of test_bgemm_split_bf16_is_fp32_grade, for rows the launcher diverts


def bound(row, i, mag, terms):
    """Elementwise bound of the real-valued pass for problem i."""
    if row.plan[i] == BF16:
        return DIVERTED_RTOL * mag
    return terms * U * mag


def ratio(err, bnd):
    """err / bound elementwise; 0 where both are 0 (a slab without any k and without a beta term is exactly zero)."""
    return torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
