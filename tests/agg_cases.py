"""The case table of the adjacency aggregation (dp_agg.hip), its inputs, its float64 references, a CPU emulation of
every form and the GPU runner — shared by test_agg_plan_cpu.py (what the table reaches, what the references can tell
apart), test_gpu_agg.py and its child processes (tests/_agg_worker.py).

Kinds: plain (U = op(A) V + beta U through dp_adj_aggregate / dp_adj_aggregate_packed), fused (the GraphConv tail behind
the product, dp_adj_aggregate_rownorm), pack (dp_adj_pack / dp_adj_pack_zero).  Every row records the plan
dp_adj_aggregate_plan answers for it (tests/agg_plans.py, written by `python -m tests.agg_cases`, never by hand; rows
with a knob are asked in a child process that has the knob set).  `--digest` makes profiles/agg_fp64_anchor.txt from a
GPU run's file.

Data.  M = op(A) is what is built; A = M^T for a transposed row.
  grid   M has three cyclic diagonals (every row and every k column is hit three times) with entries from {0.5, 1, 2}
         (fp32 forms) or {1} (packed forms), and entries of 0.5 / 1 in the first 16 and the last (n - 1) % 16 + 1 rows —
         rows of the first and the last row tile of every form — at columns 0, n - 1 and both sides of every panel
         (1024), segment (256, 512) and k-step (16) edge, in that order, as many as five per row allow: at most 8
         non-zeros per row (sum of |M| <= 11) and 5 per column.  V = k 2^-18, 1 <= |k| < 2^19; U0 = m 2^-17, |m| < 2^17.
         Every partial sum of products in any order is a multiple of 2^-19 below 2^5: exact in fp32.  The comparison is
         torch.equal over the whole U allocation.  A flagged row (one entry 1 + 2^-8, not a bf16 number) has the V row it
         meets on the 2^-10 grid.
  dense  density 0.3, |M| in [0.5, 1] (fp32 forms) or 1 (packed forms); |V| in [0.5, 1] with signs s[k] t[c].
         Bound per entry, any summation order of exact or once-rounded products (n products, at most n + 3 additions
         with the cross-wave sum, one more with beta, rounded up):  (n + 8) 2^-24 (|M| |V| + |beta| |U0|).
  fused  u = M V (+ P) (+ bias) per group, then the tail of rowop_cases.rownorm_fwd_math; its counted-rounding bounds
         (rowop_cases.rownorm_fwd_bounds) with the product's bound added to the rounding of u.
Layout: U, the outputs of the tail, invn and part are allocations of FRONT guard words, the rows at a leading dimension
that may exceed the width, and TAIL guard words; entries start as NaN (beta = 0), guards as GUARD, V's padding columns
are NaN.  After a launch everything outside an output's own entries must be as it was."""
import collections
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys
import zlib

import torch

from graph_pooling_amd import _lib
from tests import rowop_cases as RC

U24 = 2.0 ** -24
GUARD = -7.25
FRONT, TAIL = 4, 8
ENVS = {"": {}, "wide": {"DP_AGG_WIDE": "1"}, "rt16": {"DP_AGG_RT": "16"}, "rt32": {"DP_AGG_RT": "32"}}
KNOBS = ("DP_AGG_WIDE", "DP_AGG_RT", "DP_NO_PACK", "DP_NO_SPLIT_GEMM", "DP_SPLIT_GEMM_W4")
FORMS = ("panel_f32", "panel_bf16", "wide", "wide_dma", "gemm_f32", "gemm_split_bf16")
PLAN_FIELDS = ("form", "ct", "rt", "tiles", "grid", "lds", "fallback", "fb_ct", "fb_rt", "fb_tiles", "fb_grid", "fb_lds",
               "split", "declines")
Plan = collections.namedtuple("Plan", PLAN_FIELDS)

Row = collections.namedtuple("Row", "id kind B n C trans packed beta flagged off vpad upad env o")


def _row(kind, tag, B, n, C, trans=0, packed=0, beta=0.0, flagged=0, off=0, vpad=0, upad=0, env="", **o):
    name = "%s-%s-%dx%dx%d%s%s%s%s" % (kind, tag, B, n, C, "T" if trans else "N", "p" if packed else "",
                                       "f" if flagged else "", "-" + env if env else "")
    return Row(name, kind, B, n, C, trans, packed, beta, flagged, off, vpad, upad, env, dict(o))


def _fused(tag, B, n, w, packed=0, env="", flagged=0, **kw):
    o = dict(w=tuple(w), normalize=1, stats=1, part=1, invn=1, P=1, bias=(1,) * len(w), sep=0, ypad=1)
    o.update(kw)
    return _row("fused", tag + "-" + "+".join(map(str, w)), B, n, sum(w), 0, packed, 0.0, flagged, 0, 1, 0, env, **o)


BETAS = (0.0, 1.0, 0.5)
PANEL_N = (4, 8, 12, 16, 20, 64, 68, 128, 132, 192, 196, 256, 260, 1024, 1028, 1040, 2052)
BF16_N = (128, 132, 160, 256, 260, 288, 384, 512, 516)
WIDE_N = (128, 160, 192, 256, 288)
DMA_C = (129, 144, 145, 160, 161, 208, 225, 276, 289, 305, 320)
DMA_N = (128, 160, 192, 224)
PACK_N = (1, 3, 5, 63, 64, 65)
PAIRS = ((20, 20), (17, 3), (1, 1), (64, 64))


def _build():
    rows = []
    i = 0

    def pads():
        return dict(vpad=(0, 3)[i % 2], upad=(3, 0, 1)[i % 3])

    # ---- panel fp32: every CT at both of its width edges, both row tiles (B ceil(n / 32) at 255 | 256), both passes
    for ct in range(1, 9):
        for trans in (0, 1):
            for B in (255, 256):
                for Cc in (16 * ct, 16 * (ct - 1) + 1):
                    if Cc == 16 * ct and B == 255 and ct not in (1, 2, 5, 8) and trans:
                        continue
                    i += 1
                    rows.append(_row("plain", "ct", B, (4, 12, 20)[i % 3], Cc, trans, beta=BETAS[i % 3], **pads()))
    # ---- panel fp32: the K loop.  Workgroups: 1, 3, 7, 8, 9, 8 k + 5
    PB = {4: 1, 8: 3, 12: 7, 16: 8, 20: 4, 64: 2, 68: 9, 128: 1, 132: 1, 192: 1, 196: 1, 256: 2, 260: 1, 1024: 1,
          1028: 1, 1040: 1, 2052: 1}
    for n in PANEL_N:
        for trans in (0, 1):
            i += 1
            rows.append(_row("plain", "k", PB[n], n, (16, 17, 40, 5)[i % 4], trans, beta=BETAS[i % 3], **pads()))
    rows.append(_row("plain", "k", 9, 16, 8, 0, beta=1.0, upad=1))
    rows.append(_row("plain", "k", 9, 16, 8, 1, beta=0.0, vpad=2))
    rows.append(_row("plain", "lastpanel", 1, 2560, 16, 1))
    rows.append(_row("plain", "lastpanel", 1, 2560, 16, 0, beta=0.5))
    # ---- ... and what the panel kernel does not take: the GEMM
    rows.append(_row("plain", "gemm", 1, 2564, 16, 1, cpu_only=1))
    rows.append(_row("plain", "gemm", 2, 67, 20, 0, beta=0.5, upad=1))
    rows.append(_row("plain", "gemm", 2, 67, 20, 1, vpad=1))
    rows.append(_row("plain", "gemm-off1", 2, 64, 20, 0, off=1, beta=1.0))
    rows.append(_row("plain", "gemm-off1", 2, 64, 20, 1, off=1))
    rows.append(_row("plain", "gemm", 2, 64, 130, 0, vpad=1, upad=2))
    rows.append(_row("plain", "gemm", 2, 132, 130, 1, beta=1.0))
    # ---- the row-tile knob
    for env, B, n in (("rt32", 1, 20), ("rt32", 3, 68), ("rt16", 256, 20), ("rt16", 8, 1028)):
        for trans in (0, 1):
            i += 1
            rows.append(_row("plain", "knob", B, n, (24, 100)[trans], trans, beta=BETAS[i % 3], env=env, **pads()))
    # ---- panel bf16
    for n in BF16_N:
        for trans in (0, 1):
            i += 1
            rows.append(_row("plain", "k", (1, 3, 2)[i % 3], n, (16, 17, 40, 5)[i % 4], trans, 1, beta=BETAS[i % 3], **pads()))
    for ct in range(1, 9):
        for k, Cc in enumerate((16 * ct, 16 * (ct - 1) + 1)):
            i += 1
            rows.append(_row("plain", "ct", (2, 64)[k], 128, Cc, (ct + k) % 2, 1, beta=BETAS[i % 3], **pads()))
    for trans in (0, 1):
        rows.append(_row("plain", "flag", 2, 132, 20, trans, 1, beta=BETAS[1 + trans], flagged=1, upad=1))
        rows.append(_row("plain", "flag", 3, 288, 33, trans, 1, flagged=1, vpad=1))
    rows.append(_row("plain", "gemm", 2, 131, 20, 0, 1, beta=1.0))
    rows.append(_row("plain", "gemm", 2, 131, 20, 1, 1))
    # ---- wide, forced: CT 1..8 at psteps 2, 3, 3, 4, 5
    for ct in range(1, 9):
        for k, n in enumerate(WIDE_N):
            i += 1
            Cc = 16 * ct if (ct + k) % 2 else 16 * (ct - 1) + 1
            rows.append(_row("plain", "k", 2 + i % 2, n, Cc, (ct + k) % 2, 1, beta=BETAS[(ct + k) % 3], env="wide", **pads()))
    for n in (129, 131, 260):
        for trans in (0, 1):
            i += 1
            rows.append(_row("plain", "rows", 2, n, 40, trans, 1, beta=(0.5, 1.0)[trans], env="wide", **pads()))
    for trans in (0, 1):
        rows.append(_row("plain", "flag", 2, 160, 40, trans, 1, beta=(1.0, 0.0)[trans], flagged=1, env="wide", upad=1))
        rows.append(_row("plain", "flag", 2, 131, 24, trans, 1, beta=(0.0, 0.5)[trans], flagged=1, env="wide", vpad=1))
    rows.append(_row("plain", "heuristic", 512, 128, 8, 0, 1))
    rows.append(_row("plain", "heuristic", 511, 128, 8, 1, 1, beta=1.0))           # one short: the panel kernel
    # ---- wide DMA
    for k, Cc in enumerate(DMA_C):
        for j in (0, 1):
            i += 1
            n = DMA_N[(2 * k + j) % 4]
            rows.append(_row("plain", "k", 2 + i % 2, n, Cc, (k + j) % 2, 1, beta=BETAS[(k + j) % 3], **pads()))
    for n, Cc in ((131, 129), (131, 320), (260, 161), (260, 289)):
        i += 1
        rows.append(_row("plain", "rows", 2, n, Cc, i % 2, 1, beta=BETAS[i % 3], **pads()))
    rows.append(_row("plain", "flag", 2, 160, 144, 0, 1, beta=1.0, flagged=1, upad=1))
    rows.append(_row("plain", "flag", 2, 128, 305, 1, 1, flagged=1, vpad=1))
    # ---- the fused tail: every panel instantiation of the NN pass (fp32 loop), every wide one, the bf16 loop
    for ct in range(1, 9):
        for B in (255, 256):
            i += 1
            w = 16 * ct if (ct + B) % 2 else 16 * (ct - 1) + 1
            rows.append(_fused("ct", B, (12, 20)[i % 2], [w], stats=i % 3, P=i % 2, bias=(i // 2 % 2,), invn=i % 2,
                               normalize=1 if i % 4 else 0))
        i += 1
        rows.append(_fused("ct", 2, 160, [16 * ct if ct % 2 else 16 * (ct - 1) + 1], 1, "wide", stats=i % 3, P=i % 2,
                           bias=((i + 1) % 2,), invn=i % 2))
        rows.append(_fused("ct", 2, (132, 288)[ct % 2], [16 * (ct - 1) + 1 if ct % 2 else 16 * ct], 1, stats=(i + 1) % 3,
                           P=(i + 1) % 2, bias=(i % 2,)))
    # group layouts x operands, on the three forms (n = 20: rows past n in the last 16-row tile; 132 / 160 likewise)
    for k, w in enumerate(PAIRS + ((20,),)):
        for f, (B, n, packed, env) in enumerate(((3, 20, 0, ""), (2, 132, 1, ""), (2, 160, 1, "wide"))):
            i += 1
            G = len(w)
            rows.append(_fused("all", B, n, w, packed, env, stats=1 + (k + f) % 2, sep=(k + f) % 2))
            rows.append(_fused("bare", B, n, w, packed, env, stats=0, part=(k + f) % 2, invn=0, P=0, bias=(0,) * G,
                               sep=(k + f + 1) % 2))
            rows.append(_fused("bias1", B, n, w, packed, env, stats=2, P=(k + f) % 2, bias=(0, 1)[:G] if k % 2 else (1, 0)[:G],
                               normalize=(k + f) % 2, ypad=0))
    rows.append(_fused("flag", 2, 132, (17, 3), 1, flagged=1))
    rows.append(_fused("flag", 2, 160, (20, 20), 1, "wide", flagged=1, stats=2))
    rows.append(_fused("k", 1, 1028, (20, 20), 0))
    rows.append(_fused("k", 1, 516, (17, 3), 1))
    rows.append(_fused("knob", 2, 68, (20, 20), 0, "rt32"))
    rows.append(_fused("knob", 256, 20, (17, 3), 0, "rt16"))
    # ---- dp_adj_pack
    for n in PACK_N:
        rows.append(_row("pack", "n", 3, n, 1, zero=0))
    rows.append(_row("pack", "zero", 3, 65, 1, zero=16 * 37))          # 12 workgroups, 37 sixteen-byte words
    rows.append(_row("pack", "zero", 2, 64, 1, zero=16 * 3))           # fewer words than workgroups
    rows.append(_row("pack", "zero", 2, 63, 1, zero=16 * 5 + 8))       # no multiple of 16 bytes: a launch of its own
    return tuple(rows)


ROWS = _build()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS), [k for k, v in collections.Counter(r.id for r in ROWS).items() if v > 1]


def of(kind, env=None):
    return [r for r in ROWS if r.kind == kind and (env is None or r.env == env)]


def row_id(r):
    return r.id


def gpu_rows(env):
    return [r for r in ROWS if r.env == env and not r.o.get("cpu_only")]


# ------------------------------------------------------------------------------------------------ the plan query
def query(lib, B, n, Cc, trans=0, packed=0, fused=0, misalign=0, beta=0.0):
    out = (C.c_int * _lib.AGG_PLAN_INTS)()
    _lib.check(lib.dp_adj_aggregate_plan(B, n, Cc, trans, packed, fused, misalign, beta, out), "dp_adj_aggregate_plan")
    return Plan(*out)


def plan_of(lib, r):
    if r.kind == "pack":
        return None
    return query(lib, r.B, r.n, r.C, r.trans, r.packed, 1 if r.kind == "fused" else 0, 4 * r.off, r.beta)


def form_name(p):
    return FORMS[p.form]


def knobs_unset():
    return not any(k in os.environ for k in KNOBS)


def child_env(env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(ENVS[env])
    return e


def child_plans(env, timeout=120):
    """{id: Plan} of the rows with this knob setting, asked in a fresh process that has the knob set (no GPU call)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_agg_worker.py")
    p = subprocess.run([sys.executable, worker, "--plans", env], env=child_env(env), capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return {k: Plan(*v) for k, v in json.loads(p.stdout.splitlines()[-1]).items()}


PLANS = {}
try:
    from tests.agg_plans import PLANS as _RAW  # noqa: E402  (written by `python -m tests.agg_cases`)
    PLANS = {k: Plan(*v) for k, v in _RAW.items()}
except ImportError:
    pass


# ------------------------------------------------------------------------------------------------ inputs
def _gen(r, mode):
    g = torch.Generator()
    g.manual_seed(zlib.crc32((r.id + mode).encode()))
    return g


def _pick(g, vals, *shape):
    return torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), shape, generator=g)]


def edge_columns(n):
    """Columns 0 and n - 1, then both sides of every panel, segment and k-step edge below n, most important first."""
    out = [0, n - 1]
    for period in (1024, 512, 256, 16):
        for e in range(period, n, period):
            out += [e - 1, e]
    seen, res = set(), []
    for c in out:
        if 0 <= c < n and c not in seen:
            seen.add(c)
            res.append(c)
    return res


def edge_rows(n):
    """(rows of the first 16-row tile, rows of the last 16-row tile): inside the first / last row tile of every form."""
    return list(range(min(16, n))), list(range(16 * ((n - 1) // 16), n))


EDGE_PER_ROW = 5


def grid_m(r, g):
    B, n = r.B, r.n
    vals = (1.0,) if r.packed else (0.5, 1.0, 2.0)
    M = torch.zeros(B, n, n)
    rr = torch.arange(n)
    shifts = torch.randperm(n, generator=g)[:3].tolist()
    for s in shifts:
        M[:, rr, (rr + s) % n] = _pick(g, vals, B, n)
    ev = (1.0,) if r.packed else (0.5, 1.0)
    for rows in edge_rows(n):
        cols = edge_columns(n)[:EDGE_PER_ROW * len(rows)]
        for j, c in enumerate(cols):
            M[:, rows[j % len(rows)], c] = _pick(g, ev, B)
    return M


def dense_m(r, g):
    B, n = r.B, r.n
    keep = torch.rand(B, n, n, generator=g) < 0.3
    mag = torch.ones(B, n, n) if r.packed else 0.5 + 0.5 * torch.rand(B, n, n, generator=g)
    return torch.where(keep, mag, torch.zeros(()))


FLAG_VALUE = 1.0 + 2.0 ** -8          # nine significant bits: not a bf16 number


def _product_inputs(r, mode):
    """M = op(A) [B, n, n], V [B, n, C] (fp32, CPU)."""
    g = _gen(r, mode)
    B, n, Cc = r.B, r.n, r.C
    if mode == "grid":
        M = grid_m(r, g)
        k = torch.randint(1, 2 ** 19, (B, n, Cc), generator=g).float()
        V = k * _pick(g, (-1.0, 1.0), B, n, Cc) * 2.0 ** -18
    else:
        M = dense_m(r, g)
        s, t = _pick(g, (-1.0, 1.0), B, n, 1), _pick(g, (-1.0, 1.0), B, 1, Cc)
        V = (0.5 + 0.5 * torch.rand(B, n, Cc, generator=g)) * s * t
    if r.flagged:
        b, row, col = B - 1, n // 2, n // 3
        M[b, row, col] = FLAG_VALUE if mode == "grid" else 0.7
        if mode == "grid":
            V[b, col] = torch.round(V[b, col] * 2.0 ** 10) * 2.0 ** -10
            V[b, col] = torch.where(V[b, col] == 0, torch.full_like(V[b, col], 2.0 ** -10), V[b, col])
    return M, V


@functools.lru_cache(maxsize=4)
def inputs(rid, mode):
    """The row's inputs and float64 reference (CPU), made once: treat them as read-only."""
    r = BY_ID[rid]
    g = _gen(r, mode + "+")
    B, n, Cc = r.B, r.n, r.C
    M, V = _product_inputs(r, mode)
    d = dict(M=M, V=V)
    if r.kind == "plain":
        if mode == "grid":
            U0 = torch.randint(-2 ** 17 + 1, 2 ** 17, (B, n, Cc), generator=g).float() * 2.0 ** -17
        else:
            U0 = torch.randn(B, n, Cc, generator=g)
        d["U0"] = U0
        absprod = torch.bmm(M.double().abs(), V.double().abs())
        d["ref"] = torch.bmm(M.double(), V.double()) + (r.beta * U0.double() if r.beta else 0.0)
        d["bound"] = (n + 8) * U24 * (absprod + abs(r.beta) * U0.double().abs())
        return d
    o = r.o
    w = o["w"]
    c0 = (0,) + ((w[0],) if len(w) == 2 else ())
    if all(not b for b in o["bias"]) and n >= 2:               # an all-zero row with no bias: the 1e-12 clamp
        M[0, 1, :] = 0.0
    if o["P"]:
        P = torch.randint(-2 ** 17 + 1, 2 ** 17, (B, n, Cc), generator=g).float() * 2.0 ** -17 if mode == "grid" else \
            torch.randn(B, n, Cc, generator=g)
        if all(not b for b in o["bias"]) and n >= 2:
            P[0, 1, :] = 0.0
        d["P"] = P
    d["bias"] = [(torch.randint(-2 ** 9, 2 ** 9, (wi,), generator=g).float() * 2.0 ** -10 if o["bias"][i] else None)
                 for i, wi in enumerate(w)]
    prod = torch.bmm(M.double(), V.double())
    pb = (n + 8) * U24 * torch.bmm(M.double().abs(), V.double().abs()) if mode == "dense" else torch.zeros_like(prod)
    d["prod"], d["pb"], d["c0"] = prod, pb, c0
    c = tail_case(r)
    res = RC.rownorm_fwd_math(c, tail_operands(r, d, prod), torch.float64)
    d["tail"] = res
    d["tail_bounds"] = [tail_bounds(c, res[i], pb[..., c0[i]:c0[i] + w[i]].reshape(B * n, w[i])) for i in range(len(w))]
    return d


def tail_case(r):
    """The row as a rownorm_fwd case of rowop_cases (its reference and bounds are reused, not restated)."""
    o, w = r.o, r.o["w"]
    c0 = (0,) + ((w[0],) if len(w) == 2 else ())
    return RC.Case(r.id, "rownorm_fwd", len(w), c0, tuple(w), r.B, r.n, 0,
                   dict(P=o["P"], bias=o["bias"], normalize=o["normalize"], stats=o["stats"], invn=o["invn"]), 0, False,
                   bool(o["sep"]))


def tail_operands(r, d, prod):
    w, c0, rows = r.o["w"], d["c0"], r.B * r.n
    return dict(Ug=[prod[..., c0[i]:c0[i] + w[i]].reshape(rows, w[i]) for i in range(len(w))],
                Pg=[d["P"][..., c0[i]:c0[i] + w[i]].reshape(rows, w[i]) for i in range(len(w))] if r.o["P"] else None,
                bias=d["bias"])


def tail_bounds(c, res, pb):
    """rowop_cases.rownorm_fwd_bounds with the product's own error pb added to the rounding error of u: that function
    takes du = 2 U mu, so mu grows by pb / (2 U) (and by the rounding of the erroneous part, second order)."""
    r = dict(res)
    r["mu"] = res["mu"] + pb * (1 + 4 * RC.U) / (2 * RC.U)
    return RC.rownorm_fwd_bounds(c, r)


def op_to_a(r, M):
    return M.transpose(1, 2).contiguous() if r.trans else M


# ------------------------------------------------------------------------------------------------ CPU emulation
def split3(V):
    """k_split3: hi + mid + lo == V, each a bf16 number (round to nearest even), as fp32 tensors."""
    hi = V.bfloat16().float()
    r1 = V - hi
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()
    return hi, mid, lo


def emulate_product(r, plan, M, V, defect=None):
    """fp32 emulation of the form `plan` names: the k-steps in each wave's order, the waves summed in the kernel's
    order, the three planes low first.  (The order inside one k-step is the matrix core's; a k-step is one fp32 bmm
    here.)  defect: 'lo' (the low plane dropped), 'step' (the last k-step of the wave that owns it dropped), 'tail'
    (the panel's K tail not zeroed: it holds the clamped duplicates the DMA left there)."""
    B, n = r.B, r.n
    form = form_name(plan)
    if r.flagged and form in ("panel_bf16", "wide", "wide_dma"):
        form = "panel_f32" if (form == "panel_bf16" or plan.fallback == _lib.AGG_FB_PANEL) else "gemm_f32"
    zero = torch.zeros(B, n, V.shape[2])
    if form in ("gemm_f32", "gemm_split_bf16"):
        acc = zero.clone()
        for k0 in range(0, n, 16):
            acc = acc + torch.bmm(M[:, :, k0:k0 + 16], V[:, k0:k0 + 16])
        return acc
    if form == "panel_f32":
        acc = [zero.clone() for _ in range(4)]
        kpanel = n if r.trans else min(n, 1024)
        for kbase in range(0, n, kpanel):
            kw = min(kpanel, n - kbase)
            steps = (kw + 15) // 16
            last = kbase + kpanel >= n
            for s in range(steps):
                if defect == "step" and last and s == steps - 1:
                    continue
                k0, k1 = kbase + 16 * s, min(kbase + 16 * s + 16, n)
                acc[s % 4] = acc[s % 4] + torch.bmm(M[:, :, k0:k1], V[:, k0:k1])
                if defect == "tail" and last and s == steps - 1 and kw % 16:
                    for k in range(kw, 16 * steps):      # NN: A[row, n - 4 + k % 4]; TN: A[n - 1, row]; both meet V[n - 1]
                        dup = M[:, :, n - 1] if r.trans else M[:, :, n - 4 + k % 4]
                        acc[s % 4] = acc[s % 4] + dup.unsqueeze(2) * V[:, n - 1:n]
        return ((acc[0] + acc[1]) + acc[2]) + acc[3]
    hi, mid, lo = split3(V)
    if defect == "lo":
        lo = torch.zeros_like(lo)
    waves = 4 if form == "panel_bf16" else 1
    acc = [zero.clone() for _ in range(waves)]
    steps = (n + 31) // 32
    for s in range(steps):
        if defect == "step" and s == steps - 1:
            continue
        k0, k1 = 32 * s, min(32 * s + 32, n)
        for plane in (lo, mid, hi):
            acc[s % waves] = acc[s % waves] + torch.bmm(M[:, :, k0:k1], plane[:, k0:k1])
    out = acc[0]
    for a in acc[1:]:
        out = out + a
    return out


def emulate_plain(r, plan, d, defect=None):
    u = emulate_product(r, plan, d["M"], d["V"], defect)
    return u + torch.tensor(r.beta, dtype=torch.float32) * d["U0"] if r.beta else u


def emulate_tail(r, plan, d, defect=None):
    """The tail in fp32 on the emulated product.  defect: those of emulate_product, 'dup' (one clamped duplicate column
    counted in the norm), 'divisor' (w + 1 in the mean)."""
    prod = emulate_product(r, plan, d["M"], d["V"], defect if defect in ("lo", "step", "tail") else None)
    return RC.rownorm_fwd_math(tail_case(r), tail_operands(r, d, prod), torch.float32,
                               drop=defect if defect in ("dup", "divisor") else None)


def tail_errors(r, d, got):
    """[(what, error / bound)] of a tail result `got` (rownorm_fwd_math's layout) against the row's reference."""
    out = []
    o = r.o
    for i, res in enumerate(d["tail"]):
        by, binv, bmean, bm2 = d["tail_bounds"][i]
        out.append(("y%d" % i, RC.ratio((got[i]["y"].double() - res["y"]).abs(), by)))
        if o["invn"]:
            out.append(("invn%d" % i, RC.ratio((got[i]["inv"].double() - res["inv"]).abs(), binv)))
        if o["stats"] and o["part"]:
            out.append(("mean%d" % i, RC.ratio((got[i]["mean"].double() - res["mean"]).abs(), bmean)))
            out.append(("m2_%d" % i, RC.ratio((got[i]["m2"].double() - res["m2"]).abs(), bm2)))
    return out


def pack_reference(A, ld):
    """dp_adj_pack: the high 16 bits of every entry, rows padded with zeros to ld; the transpose likewise; the flag."""
    B, n, _ = A.shape
    bits = A.contiguous().view(torch.int32)
    hi = (bits >> 16).to(torch.int16)
    P = torch.zeros(B, n, ld, dtype=torch.int16)
    P[:, :, :n] = hi
    Pt = torch.zeros(B, n, ld, dtype=torch.int16)
    Pt[:, :, :n] = hi.transpose(1, 2)
    return P, Pt, int(bool((bits & 0xFFFF).ne(0).any()))


def pack_input(r):
    g = _gen(r, "pack")
    A = _pick(g, (0.0, 1.0, 0.5, -2.0, 3.0), r.B, r.n, r.n)
    A[r.B - 1, r.n - 1, r.n - 1] = FLAG_VALUE            # the last entry of the batch: no bf16 number
    return A


# ------------------------------------------------------------------------------------------------ the GPU runner
class Alloc:
    """FRONT guard words, rows x ld words, TAIL guard words; entries [rows, w] at column c0 of the rows."""

    def __init__(self, rows, w, ld, fill=GUARD, dtype=torch.float32):
        self.rows, self.w, self.ld = rows, w, ld
        self.flat = torch.full((FRONT + rows * ld + TAIL,), fill, dtype=dtype)

    def view(self, t=None, c0=0, w=None):
        t = self.flat if t is None else t
        return t.as_strided((self.rows, self.w if w is None else w), (self.ld, 1), FRONT + c0)


def _same_outside(what, got, want, bad):
    a, b = torch.nan_to_num(got, nan=1e30), torch.nan_to_num(want, nan=1e30)
    if not torch.equal(a, b):
        bad.append(f"{what}: wrote outside its own entries (or left some unwritten)")


class Packed:
    def __init__(self, lib, r, Ad, A, S, bad):
        B, n = r.B, r.n
        nb = lib.dp_adj_pack_bytes(B, n)
        self.pk = torch.full((nb // 2 + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        self.pkt = torch.full((nb // 2 + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        self.flag = torch.full((64,), 7, dtype=torch.int32, device="cuda")
        _lib.check(lib.dp_adj_pack(Ad.data_ptr(), self.pk.data_ptr(), self.pkt.data_ptr(), self.flag.data_ptr(), B, n, S()),
                   "dp_adj_pack")
        ld = lib.dp_adj_pack_ld(n)
        P, Pt, f = pack_reference(A, ld)
        if not (torch.equal(self.pk[:nb // 2].cpu().view(B, n, ld), P) and
                torch.equal(self.pkt[:nb // 2].cpu().view(B, n, ld), Pt) and
                bool((self.pk[nb // 2:] == 0x5A5A).all()) and bool((self.pkt[nb // 2:] == 0x5A5A).all())):
            bad.append("dp_adj_pack: the packed copies are not the high halves of A and A^T")
        fl = self.flag.cpu()
        if int(fl[0]) != f or bool(fl[1:].ne(0).any()):
            bad.append(f"dp_adj_pack: flag block {fl[:4].tolist()}, expected [{f}, 0, ...]")
        self.ws_bytes = lib.dp_adj_aggregate_packed_workspace_bytes(B, n, r.C)
        self.ws = torch.full((self.ws_bytes + 64,), 0x7F, dtype=torch.uint8, device="cuda")


def run_plain(lib, r, mode, S):
    """One plain row on the GPU, twice.  Returns (largest error / bound, [failures])."""
    d = inputs(r.id, mode)
    bad = []
    B, n, Cc = r.B, r.n, r.C
    A = op_to_a(r, d["M"])
    Ah = torch.full((B * n * n + 8,), float("nan"))
    Ah[r.off:r.off + B * n * n] = A.reshape(-1)
    Ad = Ah.cuda()
    Aptr = Ad.data_ptr() + 4 * r.off
    ldv, ldu = Cc + r.vpad, Cc + r.upad
    Vh = Alloc(B * n, Cc, ldv, fill=float("nan"))
    Vh.view()[...] = d["V"].reshape(B * n, Cc)
    Vd = Vh.flat.cuda()
    Uh = Alloc(B * n, Cc, ldu)
    Uh.view()[...] = d["U0"].reshape(B * n, Cc) if r.beta else float("nan")
    pk = Packed(lib, r, Ad[r.off:], A, S, bad) if r.packed else None
    outs = []
    for rep in (0, 1):
        Ud = Uh.flat.cuda()
        if pk:
            _lib.check(lib.dp_adj_aggregate_packed(Aptr, pk.pk.data_ptr(), pk.pkt.data_ptr(), pk.flag.data_ptr(),
                                                   Vd.data_ptr() + 4 * FRONT, ldv, Ud.data_ptr() + 4 * FRONT, ldu, B, n, Cc,
                                                   r.trans, r.beta, rep, pk.ws.data_ptr(), pk.ws_bytes, S()),
                       "dp_adj_aggregate_packed")         # the second run reuses the first one's split (presplit = 1)
        else:
            _lib.check(lib.dp_adj_aggregate(Aptr, Vd.data_ptr() + 4 * FRONT, ldv, Ud.data_ptr() + 4 * FRONT, ldu, B, n, Cc,
                                            r.trans, r.beta, S()), "dp_adj_aggregate")
        torch.cuda.synchronize()
        outs.append(Ud.cpu())
    if not torch.equal(torch.nan_to_num(outs[0], nan=1e30), torch.nan_to_num(outs[1], nan=1e30)):
        bad.append("two runs differ" + (" (presplit 0 against 1)" if pk else ""))
    if pk and not bool((pk.ws[pk.ws_bytes:] == 0x7F).all()):
        bad.append("wrote past the workspace")
    got = Uh.view(outs[0]).reshape(B, n, Cc)
    worst = 0.0
    if not bool(torch.isfinite(got).all()):
        bad.append("non-finite entries in U")
        worst = math.inf
    elif mode == "grid":
        want = Uh.flat.clone()
        Uh.view(want)[...] = d["ref"].float().reshape(B * n, Cc)
        assert torch.equal(Uh.view(want).double(), d["ref"].reshape(B * n, Cc)), "the grid reference is no fp32 number"
        if not torch.equal(outs[0], want):
            diff = (got.double() - d["ref"]).abs()
            bad.append(f"grid: not exact over the U allocation ({int((diff > 0).sum())} entries differ, largest {float(diff.max()):.3e})")
            worst = math.inf
    else:
        worst = RC.ratio((got.double() - d["ref"]).abs(), d["bound"])
        if not worst <= 1.0:
            bad.append(f"dense: {worst:.3f} x the bound")
        want = Uh.flat.clone()
        Uh.view(want)[...] = got.reshape(B * n, Cc)
        _same_outside("U", outs[0], want, bad)
    return worst, bad


def run_fused(lib, r, mode, S):
    d = inputs(r.id, mode)
    bad = []
    o, B, n, Cc = r.o, r.B, r.n, r.C
    w, c0, G, rows = o["w"], d["c0"], len(o["w"]), r.B * r.n
    A = d["M"]
    Ad = A.reshape(-1).cuda()
    ldv = Cc + r.vpad
    Vh = Alloc(rows, Cc, ldv, fill=float("nan"))
    Vh.view()[...] = d["V"].reshape(rows, Cc)
    Vd = Vh.flat.cuda()
    Pd = None
    if o["P"]:
        Ph = Alloc(rows, Cc, ldv, fill=float("nan"))
        Ph.view()[...] = d["P"].reshape(rows, Cc)
        Pd = Ph.flat.cuda()
    biasd = [b.cuda() if b is not None else None for b in d["bias"]]
    if o["sep"] or G == 1:
        ybufs = [(Alloc(rows, w[i], w[i] + o["ypad"] * (1 + 2 * i)), 0) for i in range(G)]
    else:
        jb = Alloc(rows, Cc, Cc + o["ypad"] * 3)
        ybufs = [(jb, c0[i]) for i in range(G)]
    for i, (b, cc) in enumerate(ybufs):
        b.view(c0=cc, w=w[i])[...] = float("nan")
    invh = Alloc(rows, G, G, fill=float("nan")) if o["invn"] else None
    parth = Alloc(rows, 2 * G, 2 * G, fill=float("nan")) if o["part"] else None
    pk = Packed(lib, r, Ad, A, S, bad) if r.packed else None
    g = _lib.RowGroups()
    g.G = G
    for i in range(G):
        g.c0[i], g.w[i] = c0[i], w[i]
    runs = []
    for rep in (0, 1):
        uniq = {id(b): b for b, _ in ybufs}
        yd = {k: b.flat.cuda() for k, b in uniq.items()}
        invd = invh.flat.cuda() if invh else None
        partd = parth.flat.cuda() if parth else None
        yp, bp = _lib.GroupPtrs(), _lib.GroupPtrs()
        for i, (b, cc) in enumerate(ybufs):
            yp.p[i], yp.ld[i] = yd[id(b)].data_ptr() + 4 * (FRONT + cc), b.ld
            if biasd[i] is not None:
                bp.p[i], bp.ld[i] = biasd[i].data_ptr(), w[i]
        rc = lib.dp_adj_aggregate_rownorm(
            Ad.data_ptr(), pk.pk.data_ptr() if pk else None, pk.pkt.data_ptr() if pk else None,
            pk.flag.data_ptr() if pk else None, Vd.data_ptr() + 4 * FRONT, ldv, Pd.data_ptr() + 4 * FRONT if o["P"] else None,
            C.byref(g), C.byref(bp) if any(o["bias"]) else None, C.byref(yp),
            invd.data_ptr() + 4 * FRONT if invh else None, partd.data_ptr() + 4 * FRONT if parth else None, B, n,
            o["normalize"], o["stats"], rep if pk else 0, pk.ws.data_ptr() if pk else None, pk.ws_bytes if pk else 0, S())
        assert rc != _lib.AGG_DECLINED, f"{r.id}: the fused entry declined"
        _lib.check(rc, "dp_adj_aggregate_rownorm")
        torch.cuda.synchronize()
        runs.append(({k: v.cpu() for k, v in yd.items()}, invd.cpu() if invh else None, partd.cpu() if parth else None))
    flat0 = [t for t in list(runs[0][0].values()) + [runs[0][1], runs[0][2]] if t is not None]
    flat1 = [t for t in list(runs[1][0].values()) + [runs[1][1], runs[1][2]] if t is not None]
    if not all(torch.equal(torch.nan_to_num(a, nan=1e30), torch.nan_to_num(b, nan=1e30)) for a, b in zip(flat0, flat1)):
        bad.append("two runs differ" + (" (presplit 0 against 1)" if pk else ""))
    ygot, invgot, partgot = runs[0]
    got = []
    wants = {k: b.flat.clone() for k, b in {id(b): b for b, _ in ybufs}.items()}
    for i, (b, cc) in enumerate(ybufs):
        y = b.view(ygot[id(b)], cc, w[i]).clone()
        b.view(wants[id(b)], cc, w[i])[...] = y
        e = dict(y=y)
        if invh:
            e["inv"] = invh.view(invgot)[:, i:i + 1].clone()
        if parth and o["stats"]:
            pv = parth.view(partgot)
            e["mean"], e["m2"] = pv[:, 2 * i:2 * i + 1].clone(), pv[:, 2 * i + 1:2 * i + 2].clone()
        got.append(e)
    for k, wv in wants.items():
        _same_outside("y", ygot[k], wv, bad)
    if invh:
        wv = invh.flat.clone()
        invh.view(wv)[...] = invh.view(invgot)
        _same_outside("invn", invgot, wv, bad)
    if parth:
        wv = parth.flat.clone()
        if o["stats"]:
            parth.view(wv)[...] = parth.view(partgot)
        _same_outside("part", partgot, wv, bad)            # stats_mode 0: part stays as it was, entries included
    worst = 0.0
    for e in got:
        for k, v in e.items():
            if not bool(torch.isfinite(v).all()):
                bad.append(f"{k}: non-finite entries")
    if not bad:
        for what, ratio in tail_errors(r, d, got):
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append(f"{mode} {what}: {ratio:.3f} x the bound")
    else:
        worst = math.inf
    return worst, bad


def run_pack(lib, r, S):
    bad = []
    B, n = r.B, r.n
    A = pack_input(r)
    Ad = A.cuda()
    nb, ld = lib.dp_adj_pack_bytes(B, n), lib.dp_adj_pack_ld(n)
    zb = r.o["zero"]
    for exact_input in (False, True):
        if exact_input:
            Ad = torch.where(A == FLAG_VALUE, torch.ones(()), A).cuda()          # every entry a bf16 number: flag 0
        Ah = Ad.cpu()
        pk = torch.full((nb // 2 + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        pkt = torch.full((nb // 2 + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        flag = torch.full((64,), 7, dtype=torch.int32, device="cuda")
        zr = torch.full((zb + 64,), 0x33, dtype=torch.uint8, device="cuda")
        if zb:
            _lib.check(lib.dp_adj_pack_zero(Ad.data_ptr(), pk.data_ptr(), pkt.data_ptr(), flag.data_ptr(), B, n,
                                            zr.data_ptr() + 16, zb, S()), "dp_adj_pack_zero")
        else:
            _lib.check(lib.dp_adj_pack(Ad.data_ptr(), pk.data_ptr(), pkt.data_ptr(), flag.data_ptr(), B, n, S()),
                       "dp_adj_pack")
        torch.cuda.synchronize()
        P, Pt, f = pack_reference(Ah, ld)
        if not torch.equal(pk[:nb // 2].cpu().view(B, n, ld), P):
            bad.append("P is not the high half of A, zero padded")
        if not torch.equal(pkt[:nb // 2].cpu().view(B, n, ld), Pt):
            bad.append("Pt is not the high half of A^T, zero padded")
        if not (bool((pk[nb // 2:] == 0x5A5A).all()) and bool((pkt[nb // 2:] == 0x5A5A).all())):
            bad.append("wrote past the packed copies")
        fl = flag.cpu()
        if int(fl[0]) != f or bool(fl[1:].ne(0).any()):
            bad.append(f"flag block {fl[:4].tolist()}, expected [{f}, 0, ...]")
        z = zr.cpu()
        if not (bool((z[:16] == 0x33).all()) and bool((z[16:16 + zb] == 0).all()) and bool((z[16 + zb:] == 0x33).all())):
            bad.append("the side zero-fill did not clear exactly its region")
    return 0.0, bad


def S_current():
    return torch.cuda.current_stream().cuda_stream


def run_row(lib, r, S=S_current):
    """The row on the GPU: (plan, largest error / bound over its runs, [failures])."""
    plan = plan_of(lib, r)
    bad = []
    if plan is not None and PLANS.get(r.id) != plan:
        bad.append(f"plan {plan} is not the recorded {PLANS.get(r.id)}")
    worst = 0.0
    if r.kind == "pack":
        worst, b = run_pack(lib, r, S)
        bad += b
    else:
        for mode in ("grid", "dense"):
            wv, b = (run_plain if r.kind == "plain" else run_fused)(lib, r, mode, S)
            print(f"{r.id} {mode}: error / bound {wv:.4f}")
            worst = max(worst, wv)
            bad += [f"{mode}: {x}" for x in b]
    path = os.environ.get("DP_AGG_ANCHOR_OUT")
    if path:
        with open(path, "a") as f:
            f.write(f"{r.id:44s} {form_name(plan) if plan else 'pack':16s} {worst:8.4f}" +
                    ("  FAILED: " + "; ".join(bad) if bad else "") + "\n")
    return plan, worst, bad


def digest(src, dst):
    """profiles/agg_fp64_anchor.txt from the per-row file the GPU runs append under DP_AGG_ANCHOR_OUT."""
    per = {}
    for line in open(src):
        f = line.split()
        rid, form, worst = f[0], f[1], float(f[2])
        key = (BY_ID[rid].kind, form)
        e = per.setdefault(key, [0, 0, -1.0, "-"])
        e[0] += 1
        e[1] += "FAILED" in line
        if worst > e[2]:
            e[2], e[3] = worst, rid
    with open(dst, "w") as f:
        f.write("# tests/test_gpu_agg.py on an MI355X (gfx950): per kind and primary form the rows run, the failures, and the\n"
                "# largest error / bound over the grid and the dense run of all rows (bounds: tests/agg_cases.py; the exact\n"
                "# grid comparison counts as 0 when it holds).  A flagged row runs its form's fp32 fallback.\n"
                "# Made by `python -m tests.agg_cases --digest <DP_AGG_ANCHOR_OUT file> <this file>`.\n"
                "kind   form              rows  failed      worst  at\n")
        for key in sorted(per):
            f.write("%-6s %-16s %5d %7d %10.4f  %s\n" % (key[0], key[1], *per[key]))


def write_plans(lib):
    assert knobs_unset(), "unset %s: the table records the plans of a process without knobs" % (KNOBS,)
    plans = {r.id: plan_of(lib, r) for r in ROWS if r.env == "" and r.kind != "pack"}
    for env in ENVS:
        if env:
            plans.update(child_plans(env))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agg_plans.py")
    with open(path, "w") as f:
        f.write('"""The plan dp_adj_aggregate_plan answers for every row of tests/agg_cases.py, in the order of\n'
                'agg_cases.PLAN_FIELDS.  Written by `python -m tests.agg_cases`; test_agg_plan_cpu.py holds the query to it."""\n')
        f.write("PLANS = {\n")
        for r in ROWS:
            if r.kind != "pack":
                f.write("    %r: %r,\n" % (r.id, tuple(plans[r.id])))
        f.write("}\n")
    print("wrote", path, len(ROWS), "rows")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--digest"]:
        digest(sys.argv[2], sys.argv[3])
        sys.exit(0)
    write_plans(_lib.load())
