"""The case table of the row kernels (dp_rowops.hip), their inputs and their float64 references — shared by
test_rowop_plan_cpu.py (what the table reaches, what the references can tell apart) and test_gpu_rowops.py.

Families: rownorm_fwd (k_rownorm_fwd), bn_apply (k_bn_finalize + k_bn_apply_fwd), rownorm_bwd (k_bn_bwd_partials +
k_bn_bwd_finalize + k_rownorm_bwd), softmax_fwd, softmax_bwd (generic and _plan kernels), masked_max (forward and
backward), colsum (k_colsum_batched).  Every row records the plan dp_rowop_plan answers for it (PLANS, written by
`python -m tests.rowop_cases`, never by hand; `--digest` makes profiles/rowops_fp64_anchor.txt from a GPU run's file).

Layout.  Every buffer is an allocation of FRONT + off guard words, the rows, and TAIL guard words, all GUARD; leading
dimensions are odd and larger than the rows unless the case is `tight`; `off` = 1 starts every buffer one float into a
16-byte aligned allocation.  After a launch everything outside an output's own entries must be as it was.

Bounds, U = 2^-24.  D(w) = ceil(w / 16) + 8 bounds the number of additions any term of a team reduction over w terms
goes through (a lane's own terms — w / 16 of them, the quad forms take theirs four at a time — and four xor-shuffle
steps), so a sum of w terms t is within D(w) U sum |t| of the exact one, the roundings of the terms themselves counted
apart.  sqrt, reciprocal and division are taken as correctly rounded to 2 U (the compiler's default), expf as 2 U.
  rownorm_fwd   u = U + P + bias: 2 roundings, du <= 2 U (|U| + |P| + |bias|) =: 2 U mu.  ss = sum u^2: relative
                (D(w) + 1) U from the sum and 4 U sum(|u| mu) / ss from du; the norm halves it; inv = 1 / max(norm, eps)
                adds 4 U:  rel(inv) = U ((D(w) + 1) / 2 + 2 sum(|u| mu) / ss + 4).
                |dy| <= inv du + |y| (rel(inv) + 3 U).  The partials follow from dy: dmean <= mean(dy) + (D(w) + 1) U
                mean |v|, dM2 <= sum (2 |t| e + e^2) + (D(w) + 4) U M2 with t = v - mean, e = dy + dmean.
  bn_apply      mu = sum pm / Bs: dmu = (D(Bs) + 1) U sum |pm| / Bs.  var = sum (pq + w d^2) / (Bs w), d = pm - mu:
                dvar = (D(Bs) + 5) U var + 2 sum |d| (dmu + U |d|) / Bs.  rstd = (var + eps)^-1/2: rel(rstd) = dvar /
                (2 (var + eps)) + 4 U.  x = (v - mu) rstd: |dx| <= rstd (dmu + U |v - mu|) + |x| (rel(rstd) + U).
  softmax_fwd   e_c = expf(l_c - m): rel_c = (|l_c - m| + 2) U.  sum e: relative D(K) U + sum s_c rel_c.  s = e / sum:
                |ds_c| <= s_c (rel_c + D(K) U + sum_k s_k rel_k + 3 U) + 2^-126 (expf underflows where fp64 does not).
  softmax_bwd   dsum = dS + dS2: 1 rounding.  dot = sum s d: ddot = (D(K) + 2) U sum |s d|.
                |ddl_c| <= s_c (ddot + U (|d_c| + |dot|) + U |d_c|) + U |dl_c|.
  colsum        (ceil(rows / 16) + 16 + rowsplit) U (sum |x| + |old|).
  bn_bwd_partials  D(w) U sum |dx| and (D(w) + 1) U sum |dx xhat| (the products rounded once).
Run-time bounds (rownorm_bwd: the BatchNorm backward through its two means and the projected l2 backward cancel, a
count of roundings says nothing useful there): the same formula evaluated in fp32 torch on the CPU, its largest error
in the row against the fp64 reference, times 4 because the kernel sums in another order, plus a floor of 4 U times the
summed magnitudes of the formula's terms.  The bias-gradient slabs add the dU bounds of their rows and
(ceil(n / 8) + 24) U sum |dU| for the sums (16 LDS rows, one atomic per 8-row workgroup).
Exact: masked max (values; arg-max by the lowest index), the bf16 planes (hi + mid + lo summed in fp32 equal the fp32
output bit for bit, padding 0; below |v| = 2^-110 three bf16 numbers cannot hold 24 bits and the sum is within 2^-134,
see vs_check), zero regions, guard bands, masked softmax rows."""
import collections
import ctypes as C
import functools
import math
import zlib

import torch

from graph_pooling_amd import _lib

U = 2.0 ** -24
GUARD = -7.25
FRONT, TAIL = 4, 8
L2_EPS = float(torch.tensor(1e-12, dtype=torch.float32))
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
SLAB0 = 0.5            # what the bias-gradient slabs hold before the launch (the kernels add into them)
TINY = 2.0 ** -126
INV_CLAMP = float(torch.tensor(1.0) / torch.tensor(1e-12))       # 1.f / eps in fp32: the saved inverse norm of the clamp branch

FAMILIES = ("rownorm_fwd", "bn_apply", "rownorm_bwd", "softmax_fwd", "softmax_bwd", "masked_max", "colsum")
WIDTHS = (1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 132, 255, 256, 257, 260, 316, 319, 320, 321, 324,
          508, 511, 512, 513, 516)
SOFTMAX_WIDTHS = WIDTHS + (767, 768, 772)
# (w0, w1, gap between the groups): small/wide, wide/small, both wide; quad-eligible pairs and the same pairs made
# ineligible by a width of 2 or 4k + 1; one pair per scalar tier; gap 1 puts c0[1] off a multiple of 4
PAIRS = ((3, 17, 0), (33, 64, 3), (65, 128, 0), (129, 255, 0), (321, 513, 0), (8, 260, 0), (260, 8, 1), (132, 256, 1),
         (132, 257, 1), (2, 132, 0), (324, 512, 0))

Case = collections.namedtuple("Case", "id fam G c0 w B n Bs o off tight sep")


def D(w):
    return (w + 15) // 16 + 8


def _case(fam, tag, w, B, n, Bs=0, gap=0, off=0, tight=False, sep=False, **o):
    w = tuple(w)
    c0 = (0,) if len(w) == 1 else (0, w[0] + gap)
    name = "%s-%s-%s-%dx%d" % (fam, "x".join(map(str, w)), tag, B, n)
    return Case(name, fam, len(w), c0, w, B, n, Bs, dict(o), off, tight, sep)


def _build():
    rows = []
    ROWN = (1, 15, 16, 17)
    BNB = ((1, 1), (2, 2), (3, 16), (3, 17), (3, 32), (3, 33), (3, 40), (3, 6))          # (B, Bs)
    NBWD = (1, 7, 8, 9, 17)
    for i, w in enumerate(WIDTHS):
        n = ROWN[i % 4]
        # ---- rownorm_fwd: everything on / everything off
        rows.append(_case("rownorm_fwd", "all", [w], 1, n, P=1, bias=(1,), normalize=1, stats=1 + i % 2, invn=1))
        rows.append(_case("rownorm_fwd", "bare", [w], 1, n + 16, P=0, bias=(0,), normalize=1, stats=0, invn=0))
        # ---- bn_apply
        B, Bs = BNB[i % len(BNB)]
        rows.append(_case("bn_apply", "bn", [w], B, 6, Bs, part=1, relu=i % 2))
        rows.append(_case("bn_apply", "relu", [w], 2, 9, 0, part=0, relu=1))
        # ---- rownorm_bwd
        nb = NBWD[i % 5]
        rows.append(_case("rownorm_bwd", "all", [w], 1 + 2 * (i % 2), nb, 0, bn=1, relu=1, normalize=1, dbias=(1,),
                          vs=1 if w <= 516 else 0))
        rows.append(_case("rownorm_bwd", "bare", [w], 3 - 2 * (i % 2), NBWD[(i + 2) % 5], 0, bn=0, relu=0, normalize=1,
                          dbias=None, vs=0))
    for i, w in enumerate(SOFTMAX_WIDTHS):
        nf, nb = (15, 16, 17)[i % 3], (63, 64, 65)[i % 3]
        fits = w <= 768
        rows.append(_case("softmax_fwd", "plan", [w], 3, nf, S2=1, vs=1 if fits else 0, zero="aligned" if i % 2 else "odd",
                          nn=(0, 1, nf)))
        rows.append(_case("softmax_fwd", "generic", [w], 2, nf + 1, S2=0, vs=0, zero=None, nn=None))
        rows.append(_case("softmax_bwd", "plan", [w], 2, nb, dbias=1, dS2=i % 2, nn=(1, nb)))
        rows.append(_case("softmax_bwd", "generic", [w], 2, nb, dbias=0, dS2=(i + 1) % 2, nn=None))
    # the plan forms with one operand at a time: vs without a zero region and the reverse
    for w in (16, 65, 129, 132, 260, 324, 513):
        rows.append(_case("softmax_fwd", "vs-only", [w], 2, 17, S2=0, vs=1, zero=None, nn=None))
        rows.append(_case("softmax_fwd", "zero-only", [w], 2, 33, S2=0, vs=0, zero="aligned", nn=(33, 5)))
        rows.append(_case("softmax_bwd", "one", [w], 3, 65, dbias=1, dS2=0, nn=None))
        rows.append(_case("softmax_bwd", "two", [w], 1, 130, dbias=1, dS2=1, nn=(100,)))
    # ---- two groups
    for i, (w0, w1, gap) in enumerate(PAIRS):
        sep = i % 2 == 0
        rows.append(_case("rownorm_fwd", "all", [w0, w1], 1, 17, gap=gap, sep=sep, P=1, bias=(1, 1), normalize=1,
                          stats=1, invn=1))
        rows.append(_case("rownorm_fwd", "bias1", [w0, w1], 1, 16, gap=gap, sep=not sep, P=0, bias=(0, 1), normalize=1,
                          stats=0, invn=0))
        B, Bs = BNB[(i + 3) % len(BNB)]
        rows.append(_case("bn_apply", "bn", [w0, w1], B, 6, Bs, gap=gap, sep=sep, part=1, relu=1))
        rows.append(_case("bn_apply", "relu", [w0, w1], 1, 17, 0, gap=gap, sep=not sep, part=0, relu=i % 2))
        lds_ok = (16 + 8) * (w0 + w1 + gap) * 4 <= 64 * 1024
        rows.append(_case("rownorm_bwd", "all", [w0, w1], 3, 9, 0, gap=gap, sep=sep, bn=1, relu=1, normalize=1,
                          dbias=(1, 1), vs=1 if lds_ok else 0))
        rows.append(_case("rownorm_bwd", "slab1", [w0, w1], 1, 17, 0, gap=gap, sep=not sep, bn=0, relu=1, normalize=1,
                          dbias=(0, 1), vs=0))
    # ---- flags of the backward: every combination of has_bn, has_relu, normalize; statistics over Bs graphs
    for k in range(8):
        bn, relu, norm = k & 1, k >> 1 & 1, k >> 2 & 1
        rows.append(_case("rownorm_bwd", "f%d%d%d" % (bn, relu, norm), [20], 3, 9, 0, bn=bn, relu=relu, normalize=norm,
                          dbias=(1,) if k % 3 == 0 else None, vs=k % 2))
        rows.append(_case("rownorm_bwd", "f%d%d%d" % (bn, relu, norm), [12, 132], 2, 8, 0, gap=1, sep=bool(k & 1), bn=bn,
                          relu=relu, normalize=norm, dbias=(1, 0) if k % 2 else None, vs=1 - k % 2))
    # ... and at one width of every other form (scalar <4> <8> <16> <0>, quad <4> <5> <8>), so that each instantiation
    # runs with each flag both ways
    for w in (50, 100, 201, 600, 132, 260, 324):
        for k in range(8):
            bn, relu, norm = k & 1, k >> 1 & 1, k >> 2 & 1
            rows.append(_case("rownorm_bwd", "f%d%d%d" % (bn, relu, norm), [w], 2, 9, 0, bn=bn, relu=relu, normalize=norm,
                              dbias=(1,) if k % 3 == 0 else None, vs=k % 2))
    for B, Bs in ((3, 6), (2, 33), (3, 40), (1, 17)):
        rows.append(_case("rownorm_bwd", "Bs%d" % Bs, [20], B, 9, Bs, bn=1, relu=1, normalize=1, dbias=(1,), vs=0))
        rows.append(_case("rownorm_bwd", "Bs%d" % Bs, [132, 8], B, 7, Bs, gap=1, bn=1, relu=0, normalize=1, dbias=None,
                          vs=0))
        rows.append(_case("bn_apply", "Bs%d" % Bs, [20, 260], B, 5, Bs, part=1, relu=1))
    # ---- normalize off (the BatchNorm entry's use of k_rownorm_fwd: statistics of y itself)
    for w in ([7], [50], [100], [201], [600], [132], [260], [324], [20, 12]):          # one width per form
        rows.append(_case("rownorm_fwd", "plain", w, 1, 33, P=0, bias=(0,) * len(w), normalize=0, stats=2, invn=0))
    # ---- BatchNorm on 1, 15, 16 and 17 rows
    for n in (1, 15, 16, 17):
        rows.append(_case("bn_apply", "rows", [33], 1, n, 0, part=1, relu=n % 2))
        rows.append(_case("bn_apply", "rows", [8, 132], 1, n, 0, gap=1, part=1, relu=1 - n % 2))
    # ---- the generic softmax backward with a node count
    rows.append(_case("softmax_bwd", "generic-nn", [33], 3, 65, dbias=0, dS2=1, nn=(0, 1, 65)))
    # ---- past the 64 KiB of the plan backward: the generic kernel, then the column sums into the slab
    rows.append(_case("softmax_bwd", "wide", [1025], 2, 63, dbias=1, dS2=1, nn=None))
    rows.append(_case("softmax_bwd", "wide", [1025], 1, 256, dbias=1, dS2=0, nn=(200,)))      # 8 row ranges, atomics
    # ---- alignment: every buffer one float into its allocation; ld equal to the width
    for fam, kw in (("rownorm_fwd", dict(P=1, bias=(1,), normalize=1, stats=1, invn=1)),
                    ("bn_apply", dict(part=1, relu=1)),
                    ("rownorm_bwd", dict(bn=1, relu=1, normalize=1, dbias=(1,), vs=1)),
                    ("softmax_fwd", dict(S2=1, vs=1, zero="aligned", nn=None)),
                    ("softmax_bwd", dict(dbias=1, dS2=1, nn=None))):
        B, n = (2, 17) if fam != "bn_apply" else (3, 6)
        for w in (260, 324, 20):
            rows.append(_case(fam, "off1", [w], B, n, off=1, **kw))
        rows.append(_case(fam, "tight", [132], B, n, tight=True, **kw))
    # ---- the second trip of the grid-stride loop: more than 65536 (row, group) items
    for w in (4, 5):
        rows.append(_case("rownorm_fwd", "stride", [w], 1, 66000, P=0, bias=(1,), normalize=1, stats=1, invn=1))
        rows.append(_case("bn_apply", "stride", [w], 2, 33000, 0, part=1, relu=1))
        rows.append(_case("softmax_fwd", "stride", [w], 1, 66000, S2=0, vs=0, zero=None, nn=(40000,)))
        rows.append(_case("softmax_bwd", "stride", [w], 1, 66000, dbias=0, dS2=0, nn=None))
    rows.append(_case("rownorm_fwd", "stride2", [4, 5], 1, 33000, gap=1, P=1, bias=(0, 0), normalize=1, stats=0, invn=0))
    # ---- masked max (forward, then backward on the same case)
    for n in (1, 23, 511, 512, 513, 530):
        for F in (63, 64, 65, 130):
            if n in (1, 23) and F != 65:
                continue
            rows.append(_case("masked_max", "mask", [F], 4, n, nn=(0, 1, n, n + 5)))
        rows.append(_case("masked_max", "nomask", [65], 2, n, nn=None))
    # ---- column sums
    for r in (1, 15, 16, 17, 100, 5):
        for c in (63, 64, 65):
            for batch, split in ((1, 1), (3, 8)) if r != 5 else ((3, 8),):
                rows.append(_case("colsum", "s%d" % split, [c], batch, r, split=split))
    for fam, kw in (("masked_max", dict(nn=(0, 1, 23, 28))), ("colsum", dict(split=1)), ("colsum", dict(split=8))):
        tag = "-s%d" % kw["split"] if "split" in kw else ""
        rows.append(_case(fam, "off1" + tag, [65], 4, 23, off=1, **kw))
        rows.append(_case(fam, "tight" + tag, [65], 4, 23, tight=True, **kw))
    rows.append(_case("colsum", "s8", [65], 1, 100, split=8))
    rows.append(_case("colsum", "s1", [64], 3, 100, split=1))
    return tuple(rows)


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [k for k, v in collections.Counter(c.id for c in CASES).items() if v > 1]


def of(fam):
    return [c for c in CASES if c.fam == fam]


def case_id(c):
    return c.id


# ------------------------------------------------------------------------------------------------ the plan query
def groups_struct(c):
    g = _lib.RowGroups()
    g.G = c.G
    for i in range(c.G):
        g.c0[i], g.w[i] = c.c0[i], c.w[i]
    return g


def plan_args(c):
    """(op, n, B, Bs, flags) of dp_rowop_plan for the case; None for a family without a pick (colsum)."""
    o = c.o
    if c.fam == "rownorm_fwd":
        return _lib.ROWOP_ROWNORM_FWD, c.n, c.B, 0, 0
    if c.fam == "bn_apply":
        return _lib.ROWOP_BN_APPLY_FWD, c.n, c.B, c.Bs, _lib.ROWF_STATS if o["part"] else 0
    if c.fam == "rownorm_bwd":
        return _lib.ROWOP_ROWNORM_BWD, c.n, c.B, c.Bs, _lib.ROWF_STATS if o["bn"] else 0
    if c.fam == "softmax_fwd":
        f = (_lib.ROWF_VS if o["vs"] else 0) | (_lib.ROWF_ZERO if o["zero"] else 0)
        return _lib.ROWOP_SOFTMAX_FWD, c.n, c.B, 0, f | (_lib.ROWF_ZERO_UNALIGNED if o["zero"] == "odd" else 0)
    if c.fam == "softmax_bwd":
        return _lib.ROWOP_SOFTMAX_BWD, c.n, c.B, 0, _lib.ROWF_DBIAS if o["dbias"] else 0
    if c.fam == "masked_max":
        return _lib.ROWOP_MASKED_MAX_FWD, c.n, c.B, 0, 0
    return None


def query(lib, op, w, n=8, B=1, Bs=0, flags=0, c0=None):
    g = _lib.RowGroups()
    g.G = len(w)
    for i, wi in enumerate(w):
        g.w[i] = wi
        g.c0[i] = c0[i] if c0 else (0 if i == 0 else w[0])
    out = (C.c_int * _lib.ROWOP_PLAN_INTS)()
    _lib.check(lib.dp_rowop_plan(op, C.byref(g), n, B, Bs, flags, out), "dp_rowop_plan")
    return tuple(out)


def plan_of(lib, c):
    a = plan_args(c)
    if a is None:
        return None
    op, n, B, Bs, flags = a
    return query(lib, op, c.w, n, B, Bs, flags, c.c0)


# ------------------------------------------------------------------------------------------------ buffers
def ld_of(c, width):
    if c.tight:
        return width
    return width + 1 if width % 2 == 0 else width + 2


def joint(c):
    return c.c0[-1] + c.w[-1]


class Buf:
    """A flat allocation with guards and a [rows, width] view at leading dimension ld, column offset c0."""

    def __init__(self, rows, width, ld, off, dtype=torch.float32, fill=GUARD):
        self.rows, self.width, self.ld, self.off = rows, width, ld, FRONT + off
        self.flat = torch.full((self.off + max(rows - 1, 0) * ld + width + (ld - width) + TAIL,), fill, dtype=dtype)

    def view(self, t=None, c0=0, w=None):
        t = self.flat if t is None else t
        return t.as_strided((self.rows, self.width if w is None else w), (self.ld, 1), self.off + c0)

    def byte_offset(self, c0=0):
        return (self.off + c0) * self.flat.element_size()


def _gen(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.id.encode()))
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _joint_in(c, rows, data):
    """Joint input buffer [rows, ld]: `data` is a list of per-group [rows, w_g] tensors; the gap columns stay GUARD."""
    b = Buf(rows, joint(c), ld_of(c, joint(c)), c.off)
    for i in range(c.G):
        b.view(c0=c.c0[i], w=c.w[i])[...] = data[i]
    return b


def _group_out(c, rows, fill=GUARD):
    """Per-group output buffers: separate allocations with their own leading dimensions (sep) or one joint buffer.
    Returns [(Buf, c0 within the Buf)] per group."""
    if c.sep or c.G == 1:
        return [(Buf(rows, c.w[i], ld_of(c, c.w[i] + 2 * i), c.off, fill=fill), 0) for i in range(c.G)]
    b = Buf(rows, joint(c), ld_of(c, joint(c)), c.off, fill=fill)
    return [(b, c.c0[i]) for i in range(c.G)]


def _group_in(c, rows, data):
    bufs = _group_out(c, rows)
    for i, (b, c0) in enumerate(bufs):
        b.view(c0=c0, w=c.w[i])[...] = data[i]
    return bufs


# ------------------------------------------------------------------------------------------------ vs planes
def vs_dims(n, cols):
    return (cols + 15) // 16, ((n + 31) // 32) * 4


def vs_elems(B, n, cols):
    ct, k8 = vs_dims(n, cols)
    return B * 3 * ct * k8 * 128


def vs_decode(vs, B, n, cols):
    """dp_agg.hip: Vs[b][plane][cb][k8][c][j] = plane(V[b][8 k8 + j][16 cb + c]), zero padded in k to a multiple of
    32 and in c to 16 CT.  vs: int16 tensor.  Returns float32 [3, B, 8 K8, 16 CT], each plane widened to fp32."""
    ct, k8 = vs_dims(n, cols)
    v = vs.view(torch.int16).reshape(B, 3, ct, k8, 16, 8).to(torch.int32) << 16
    v = v.view(torch.float32)
    return v.permute(1, 0, 3, 5, 2, 4).reshape(3, B, k8 * 8, ct * 16)


def vs_check(vs, fp32_out, B, n, cols):
    """None when hi + mid + lo (summed in fp32, that order) equal fp32_out [B, n, cols] bit for bit and all padding is
    zero; a message otherwise."""
    pl = vs_decode(vs, B, n, cols)
    total = (pl[0] + pl[1]) + pl[2]
    want = torch.zeros_like(total)
    want[:, :n, :cols] = fp32_out
    # three bf16 planes hold 24 mantissa bits only while the lowest of them is a bf16 number: ulp(v) >= 2^-133, that is
    # |v| >= 2^-110.  Below, the low plane rounds on the bf16 denormal grid: half a step, 2^-134, at the most.
    big = want.abs() >= 2.0 ** -110
    if not torch.equal(torch.where(big, total, want), want):
        bad = ((total != want) & big).nonzero()
        return "planes differ from the fp32 output at %d places, first (b, row, col) %s" % (len(bad), bad[0].tolist())
    if bool(((total.double() - want.double()).abs() > 2.0 ** -134).any()):
        return "planes of a value below 2^-110 are further than 2^-134 from it"
    pad = torch.ones_like(total, dtype=torch.bool)
    pad[:, :n, :cols] = False
    for k in range(3):
        if bool((pl[k][pad].view(torch.int32) != 0).any()):
            return "plane %d: padding is not zero" % k
    return None


# ------------------------------------------------------------------------------------------------ rownorm_fwd
def _rf_inputs(c):
    g, o, rows = _gen(c), c.o, c.B * c.n
    Ug = [_randn(g, rows, w) for w in c.w]
    Pg = [_randn(g, rows, w) for w in c.w] if o["P"] else None
    bias = [(_randn(g, w) * 0.5 if o["bias"][i] else None) for i, w in enumerate(c.w)]
    if rows >= 3 and o["normalize"]:
        for i in range(c.G):
            if bias[i] is None:           # an exact zero row, and one whose norm is 1e-13
                Ug[i][0] = 0.0
                Ug[i][1] = 0.0
                Ug[i][1, 0] = 1e-13
                if Pg:
                    Pg[i][0] = 0.0
                    Pg[i][1] = 0.0
    return dict(Ug=Ug, Pg=Pg, bias=bias)


def _quad_again(t):
    """The defect `the last quad lane unmasked`.  Every quad form loads lane tl + 16 k from quad min(tl + 16 k, nq - 1) —
    the address is clamped, the lane is masked afterwards — so the first lane past the row that loses its mask adds the
    row's own last four columns to the reduction a second time."""
    return torch.cat([t, t[..., -4:]], -1)


def rownorm_fwd_math(c, d, dt, drop=None):
    """y, inv, (mean, M2) per group in dtype dt.  drop: a defect (test_rowop_plan_cpu.py)."""
    o, out = c.o, []
    for i in range(c.G):
        u = d["Ug"][i].to(dt)
        mu = u.abs()
        if d["Pg"]:
            u = u + d["Pg"][i].to(dt)
            mu = mu + d["Pg"][i].to(dt).abs()
        if d["bias"][i] is not None:
            u = u + d["bias"][i].to(dt)
            mu = mu + d["bias"][i].to(dt).abs()
        un = u
        if drop == "column":
            un = u.clone()
            un[:, -1] = 0
        if drop == "neighbour" and c.G == 2:
            un = torch.cat([u, d["Ug"][1 - i].to(dt)[:, :1]], 1)
        if drop == "quad":
            un = _quad_again(u)
        if drop == "dup":                 # a clamped duplicate of the last column counted in the norm (agg_cases.py)
            un = torch.cat([u, u[:, -1:]], 1)
        ss = (un * un).sum(1, keepdim=True)
        inv = 1.0 / ss.sqrt().clamp_min(L2_EPS) if o["normalize"] else torch.ones_like(ss)
        y = u * inv
        v = y.clamp_min(0) if o["stats"] == 1 else y
        wdiv = c.w[i] + 1 if drop == "divisor" else c.w[i]
        mean = (_quad_again(v) if drop == "quad" else v).sum(1, keepdim=True) / wdiv
        m2 = ((v - mean) ** 2).sum(1, keepdim=True)
        out.append(dict(u=u, mu=mu, ss=ss, inv=inv, y=y, v=v, mean=mean, m2=m2))
    return out


def rownorm_fwd_bounds(c, r):
    """r: one group's float64 results -> bounds of y, inv, mean, M2."""
    w = r["y"].shape[1]
    du = 2 * U * r["mu"]
    if c.o["normalize"]:
        ss = r["ss"].clamp_min(1e-300)
        rel = U * ((D(w) + 1) / 2 + 2 * (r["u"].abs() * r["mu"]).sum(1, keepdim=True) / ss + 4)
        rel = torch.where(r["ss"] > 0, rel, torch.full_like(rel, 2 * U))
    else:
        rel = torch.zeros_like(r["ss"])
    by = r["inv"] * du + r["y"].abs() * (rel + 3 * U) + TINY
    binv = r["inv"] * (rel + 2 * U)
    dmean = by.sum(1, keepdim=True) / w + (D(w) + 1) * U * r["v"].abs().sum(1, keepdim=True) / w
    e = by + dmean
    t = (r["v"] - r["mean"]).abs()
    dm2 = (2 * t * e + e * e).sum(1, keepdim=True) + (D(w) + 4) * U * r["m2"] + TINY
    return by, binv, dmean + TINY, dm2


# ------------------------------------------------------------------------------------------------ bn_apply
def _bn_inputs(c):
    g, o = _gen(c), c.o
    Bs = c.Bs or c.B
    Yall = [3.0 + _randn(g, Bs, c.n, w) for w in c.w]            # mean 3, unit spread
    for y in Yall:
        if c.n >= 3:
            y[:, 2, :] = 1.5                                     # a node index whose rows are constant: variance 0
        y[0, 0, 0] = -2.0
    part = None
    if o["part"]:
        part = torch.empty(Bs, c.n, c.G, 2)
        for i, y in enumerate(Yall):
            v = y.clamp_min(0) if o["relu"] else y
            mean = v.mean(2)
            part[:, :, i, 0] = mean
            part[:, :, i, 1] = ((v - mean[..., None]) ** 2).sum(2)
    return dict(Yg=[y[:c.B].reshape(c.B * c.n, -1).contiguous() for y in Yall], part=part)


def bn_apply_math(c, d, dt, defect=None):
    o, out = c.o, []
    Bs = c.Bs or c.B
    for i in range(c.G):
        w = c.w[i]
        y = d["Yg"][i].to(dt).reshape(c.B, c.n, w)
        if defect == "column":
            y = y.clone()
            y[..., -1] = 0
        v = y.clamp_min(0) if o["relu"] else y
        if d["part"] is None:
            out.append(dict(x=v.reshape(c.B * c.n, w), v=v))
            continue
        pm, pq = d["part"][:, :, i, 0].to(dt), d["part"][:, :, i, 1].to(dt)
        div = Bs + 1 if defect == "divisor" else Bs
        mu = pm.sum(0) / div
        dd = pm - mu
        var = (pq + w * dd * dd).sum(0) / (div * w)
        rstd = 1.0 / (var + BN_EPS).sqrt()
        x = (v - mu[None, :, None]) * rstd[None, :, None]
        out.append(dict(x=x.reshape(c.B * c.n, w), v=v, mu=mu, rstd=rstd, var=var, pm=pm, dd=dd))
    return out


def bn_apply_bounds(c, r):
    if "mu" not in r:
        return torch.zeros_like(r["x"]), None, None
    Bs, w = c.Bs or c.B, r["x"].shape[1]
    dmu = (D(Bs) + 1) * U * r["pm"].abs().sum(0) / Bs
    dvar = (D(Bs) + 5) * U * r["var"] + 2 * (r["dd"].abs() * (dmu + U * r["dd"].abs())).sum(0) / Bs
    rel = dvar / (2 * (r["var"] + BN_EPS)) + 4 * U
    vm = (r["v"] - r["mu"][None, :, None]).abs()
    bx = r["rstd"][None, :, None] * (dmu[None, :, None] + U * vm) + r["x"].reshape(c.B, c.n, w).abs() * (rel[None, :, None] + U)
    return bx.reshape(c.B * c.n, w) + TINY, dmu + TINY, r["rstd"] * rel + TINY


# ------------------------------------------------------------------------------------------------ rownorm_bwd
def _rb_inputs(c):
    """A consistent forward in fp32 (u -> y -> relu -> BatchNorm over Bs graphs) gives the saved operands; dx random.
    Rows 0 / 1 of graph 0 have norm 0 / 1e-13 (the clamp branch), row 2 has dx nearly parallel to y, some u are 0."""
    g, o = _gen(c), c.o
    Bs = c.Bs or c.B
    rows = Bs * c.n
    Y, X, DX, INV, RSTD = [], [], [], [], []
    for i, w in enumerate(c.w):
        u = _randn(g, Bs, c.n, w)
        u[..., ::5] = u[..., ::5] * (torch.rand(Bs, c.n, u[..., ::5].shape[-1], generator=g) > 0.3)
        if o["normalize"] and c.n >= 3:
            u[0, 0] = 0.0
            u[0, 1] = 0.0
            u[0, 1, 0] = 1e-13
        nrm = u.double().norm(dim=2, keepdim=True)
        inv = (1.0 / nrm.clamp_min(L2_EPS)).float() if o["normalize"] else torch.ones(Bs, c.n, 1)
        y = u * inv
        r = y.clamp_min(0) if o["relu"] else y
        mu = r.double().mean((0, 2))
        var = ((r.double() - mu[None, :, None]) ** 2).mean((0, 2))
        rstd = (1.0 / (var + BN_EPS).sqrt()).float()
        x = ((r.double() - mu[None, :, None]) * rstd[None, :, None].double()).float()
        dx = _randn(g, Bs, c.n, w)
        if c.n >= 3 and not o["bn"]:
            dx[:, 2] = 2.0 * y[:, 2] + 1e-3 * dx[:, 2]
        Y.append(y.reshape(rows, w)), X.append(x.reshape(rows, w)), DX.append(dx.reshape(rows, w))
        INV.append(inv.reshape(rows)), RSTD.append(rstd)
    stats = torch.zeros(c.n, c.G, 2)
    stats[:, :, 1] = torch.stack(RSTD, 1)
    return dict(Y=Y, X=X, DX=DX, invn=torch.stack(INV, 1).contiguous(), stats=stats)


def rownorm_bwd_math(c, d, dt, defect=None):
    """dU per group [B * n, w] and the magnitudes of its terms, in dtype dt."""
    o, out = c.o, []
    Bs = c.Bs or c.B
    nr = c.B * c.n
    for i, w in enumerate(c.w):
        dx = d["DX"][i].to(dt).reshape(Bs, c.n, w)
        y = d["Y"][i].to(dt).reshape(Bs, c.n, w)
        if defect == "column":
            dx = dx.clone()
            dx[..., -1] = 0
        dd, mag = dx, dx.abs()
        if o["bn"]:
            xh = d["X"][i].to(dt).reshape(Bs, c.n, w)
            rstd = d["stats"][:, i, 1].to(dt)[None, :, None]
            cnt = (Bs + 1 if defect == "divisor" else Bs) * w
            m0 = dx.sum((0, 2), keepdim=True) / cnt
            m1 = (dx * xh).sum((0, 2), keepdim=True) / cnt
            dd = rstd * (dx - m0 - xh * m1)
            mag = rstd * (dx.abs() + m0.abs() + (xh * m1).abs())
        if o["relu"]:
            dd = torch.where(y > 0, dd, torch.zeros_like(dd))
            mag = torch.where(y > 0, mag, torch.zeros_like(mag))
        if o["normalize"]:
            inv = d["invn"][:, i].to(dt).reshape(Bs, c.n, 1)
            project = inv < INV_CLAMP
            dot = (_quad_again(dd * y) if defect == "quad" else dd * y).sum(2, keepdim=True)
            mag = inv * (mag + torch.where(project, y.abs() * (mag * y.abs()).sum(2, keepdim=True), torch.zeros_like(mag)))
            dd = torch.where(project, inv * (dd - y * dot), inv * dd)
        out.append(dict(dU=dd[:c.B].reshape(nr, w), mag=mag[:c.B].reshape(nr, w)))
    return out


def bn_bwd_partials_ref(c, d, i):
    """(sum_c dx, sum_c dx xhat) of group i per row, [rows, 2] in float64, and the bound: a team sum of w terms, the
    products rounded once."""
    dx, xh = d["DX"][i].double(), d["X"][i].double()
    w = c.w[i]
    ref = torch.stack([dx.sum(1), (dx * xh).sum(1)], 1)
    bound = torch.stack([D(w) * U * dx.abs().sum(1), (D(w) + 1) * U * (dx * xh).abs().sum(1)], 1) + TINY
    return ref, bound


def rownorm_bwd_bound(ref, emu):
    """Run-time bound of one group's dU from its fp64 reference and the fp32 evaluation of the same formula."""
    err = (emu["dU"].double() - ref["dU"]).abs().amax(1, keepdim=True)
    return 4 * err + 4 * U * ref["mag"] + TINY


# ------------------------------------------------------------------------------------------------ softmax
def _num_nodes(c):
    nn = c.o.get("nn")
    if nn is None:
        return None
    return torch.tensor([nn[b % len(nn)] for b in range(c.B)], dtype=torch.int32)


def _sf_inputs(c):
    g = _gen(c)
    K = c.w[0]
    l = torch.rand(c.B, c.n, K, generator=g) * 2 - 1
    last = c.n - 1
    l[:, last] = 0.375                                   # a row of equal logits
    if c.n >= 3:
        l[:, 1, ::3] = 80.0                              # logits at +-80
        l[:, 1, 1::3] = -80.0
    return dict(logits=l.reshape(c.B * c.n, K), nn=_num_nodes(c))


def softmax_fwd_math(c, d, dt, defect=None):
    K = c.w[0]
    l = d["logits"].to(dt)
    m = l.amax(1, keepdim=True)
    e = (l - m).exp()
    es = e
    if defect == "column" and K > 1:
        es = e[:, :-1]
    if defect == "quad":
        es = _quad_again(e)
    s = e / es.sum(1, keepdim=True)
    valid = torch.ones(c.B, c.n, dtype=torch.bool)
    if d["nn"] is not None:
        valid = torch.arange(c.n)[None, :] < d["nn"][:, None].long()
    valid = valid.reshape(-1, 1)
    return dict(s=torch.where(valid, s, torch.zeros_like(s)), lm=(l - m).abs(), valid=valid)


def softmax_fwd_bound(c, r):
    K = c.w[0]
    rel = (r["lm"] + 2) * U
    tot = (r["s"] * rel).sum(1, keepdim=True)
    b = r["s"] * (rel + D(K) * U + tot + 3 * U) + TINY
    return torch.where(r["valid"], b, torch.zeros_like(b))


def _sb_inputs(c):
    g = _gen(c)
    K = c.w[0]
    f = softmax_fwd_math(c, _sf_inputs(c), torch.float32)
    dS = _randn(g, c.B * c.n, K)
    dS2 = _randn(g, c.B * c.n, K) if c.o["dS2"] else None
    return dict(S=f["s"].contiguous(), dS=dS, dS2=dS2, nn=_num_nodes(c))


def softmax_bwd_math(c, d, dt, defect=None):
    s, dv = d["S"].to(dt), d["dS"].to(dt)
    mag = dv.abs()
    if d["dS2"] is not None:
        dv = dv + d["dS2"].to(dt)
        mag = mag + d["dS2"].to(dt).abs()
    sd = s * dv
    if defect == "column" and c.w[0] > 1:
        sd = sd[:, :-1]
    if defect == "quad":
        sd = _quad_again(sd)
    dot = sd.sum(1, keepdim=True)
    return dict(dl=s * (dv - dot), s=s, dv=dv, dot=dot, sabs=(s * dv).abs().sum(1, keepdim=True), mag=mag)


def softmax_bwd_bound(c, r):
    K = c.w[0]
    ddot = (D(K) + 2) * U * r["sabs"]
    return r["s"] * (ddot + U * (r["dv"].abs() + r["dot"].abs()) + U * r["mag"]) + U * r["dl"].abs() + TINY


# ------------------------------------------------------------------------------------------------ masked max
def _mm_inputs(c):
    g = _gen(c)
    F, n = c.w[0], c.n
    Z = _randn(g, c.B, n, F)
    r = min(5, max(n - 17, 0))
    top = float(Z.abs().max()) + 1.0
    if n >= 18:
        Z[:, r, 0] = top                                 # a tie across the 16 row lanes: rows r and r + 16
        Z[:, r + 16, 0] = top
        Z[:, r + 3, 1] = top                             # and between neighbours
        Z[:, r + 4, 1] = top
    if F > 3:
        Z[:, :, 2] = -Z[:, :, 2].abs() - 0.5             # an all-negative column
        Z[:, :, 3] = -Z[:, :, 3].abs() - 0.5             # a valid maximum of exactly 0
        Z[:, 0, 3] = 0.0
    return dict(Z=Z, nn=_num_nodes(c), dout=_randn(g, c.B, F))


def masked_max_ref(c, d, rule_ge=False):
    """out [B, F], argmax [B, F] by the lowest-index rule over the rows of Z * mask; -1 where a masked row wins.
    rule_ge: the defect `v >= best` (the highest index wins a tie among the valid rows)."""
    Z, n = d["Z"], c.n
    nb = torch.full((c.B,), n) if d["nn"] is None else d["nn"].long().clamp(max=n)
    valid = torch.arange(n)[None, :] < nb[:, None]
    Zm = torch.where(valid[:, :, None], Z, torch.zeros_like(Z))
    out = Zm.amax(1)
    idx = torch.arange(n)[None, :, None].expand_as(Zm)
    hit = Zm == out[:, None, :]
    hit = hit & valid[:, :, None]                        # (a valid row precedes every masked one)
    if rule_ge:
        am = torch.where(hit, idx, torch.full_like(idx, -1)).amax(1)
    else:
        am = torch.where(hit, idx, torch.full_like(idx, n)).amin(1)
        am = torch.where(am >= n, torch.full_like(am, -1), am)
    return out, am.to(torch.int32)


# ------------------------------------------------------------------------------------------------ colsum
def _cs_inputs(c):
    return dict(X=_randn(_gen(c), c.B, c.n, c.w[0]))


def colsum_ref(c, d):
    X = d["X"].double()
    old = SLAB0 if c.o["split"] > 1 else 0.0
    ref = X.sum(1) + old
    bound = ((c.n + 15) // 16 + 16 + c.o["split"]) * U * (X.abs().sum(1) + abs(old)) + TINY
    return ref, bound


INPUTS = dict(rownorm_fwd=_rf_inputs, bn_apply=_bn_inputs, rownorm_bwd=_rb_inputs, softmax_fwd=_sf_inputs,
              softmax_bwd=_sb_inputs, masked_max=_mm_inputs, colsum=_cs_inputs)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """The case's inputs (CPU, fp32), made once and shared: treat them as read-only."""
    c = BY_ID[cid]
    return INPUTS[c.fam](c)


def ratio(err, bound):
    """Largest err / bound; entries with bound 0 must have err 0 (inf otherwise)."""
    err, bound = err.double(), bound.double()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                          torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


PLANS = {}
try:
    from tests.rowop_plans import PLANS  # noqa: F401,E402  (written by `python -m tests.rowop_cases`)
except ImportError:
    pass


def digest(src, dst):
    """profiles/rowops_fp64_anchor.txt from the per-case file test_gpu_rowops.py appends under DP_ROWOPS_ANCHOR_OUT."""
    per = {f: [0, 0, -1.0, "-"] for f in FAMILIES}
    for line in open(src):
        cid, rest = line.split(None, 1)                          # id, plan (a tuple or None), worst, failures
        worst = float(rest[rest.index(")") + 1 if rest[0] == "(" else 4:].split()[0])
        e = per[BY_ID[cid].fam]
        e[0] += 1
        e[1] += "FAILED" in rest
        if worst > e[2]:
            e[2], e[3] = worst, cid
    with open(dst, "w") as f:
        f.write("# tests/test_gpu_rowops.py on an MI355X (gfx950): per family the cases run, the failures, and the largest\n"
                "# error / bound over all outputs of all cases (bounds: tests/rowop_cases.py; exact comparisons count as 0).\n"
                "# Made by `python -m tests.rowop_cases --digest <DP_ROWOPS_ANCHOR_OUT file> <this file>`.\n"
                "family          cases  failed      worst  at\n")
        for fam in FAMILIES:
            f.write("%-14s %6d %7d %10.4f  %s\n" % (fam, *per[fam]))


if __name__ == "__main__":
    import os
    import sys
    if sys.argv[1:2] == ["--digest"]:
        digest(sys.argv[2], sys.argv[3])
        sys.exit(0)
    lib = _lib.load()
    assert "DP_NO_ROW_QUADS" not in os.environ
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rowop_plans.py")
    with open(path, "w") as f:
        f.write('"""The plan dp_rowop_plan answers for every row of tests/rowop_cases.py: (kernel, NK, quad, finalize,\n'
                'generic, zero).  Written by `python -m tests.rowop_cases`; test_rowop_plan_cpu.py holds the query to it."""\n')
        f.write("PLANS = {\n")
        for c in CASES:
            if plan_args(c) is not None:
                f.write("    %r: %r,\n" % (c.id, plan_of(lib, c)))
        f.write("}\n")
    print("wrote", path, len(CASES), "cases")
