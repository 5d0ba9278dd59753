"""Cases, inputs, fp64 reference and counted error bounds of the dense / packed link-prediction loss
(dp_linkpred_loss_* and the link term of dp_loss_forward / dp_loss_backward; dp_linkpred.hip: k_link_fwd, k_link_final,
k_link_bwd, k_link_reduce).

Definition (include/diffpool_hip.h, A8), n_b = num_nodes[b] clamped to n (absent: n), eps = 1e-7:

    raw = S S^T,  p = min(raw, 1),  l = -a ln(p + eps) - (1 - a) ln(1 - p + eps)  on the n_b x n_b block, 0 outside,
    loss = sum_b sum l / norm,  norm = sum_b n_b^2 or the link_norm operand.

The reference is this formula in float64 on the fp32 inputs, one graph at a time (never more than one graph's n x n
temporaries), and its gradient by float64 autograd: torch.minimum sends the full gradient where raw < 1, half of it
where raw == 1 and none above.  With g(a, p) = gate (-a / (p + eps) + (1 - a) / (1 - p + eps)) and
G_rc = g(a_rc, p_rc) + g(a_cr, p_rc) that gradient is dS = (dloss / norm) G S.

Bounds (u = 2^-24; counted from the kernels' arithmetic, not fitted; first order, widened by W = 1 + 1/64, see
"qualification").

p.  A P entry is K products summed on the fp32 MFMA: at most K + 1 roundings of a sum of non-negative terms,
  dp = (K + 1) u p.  dp = 0 where the entry is exact: both rows hold at most one non-zero, or S lies on the quarter grid
  (every product a multiple of 1/16 and every sum below 2^20).
forward, per element:
  * fl(p + eps) rounds once and fl(fl(1 - p) + eps) twice: with dp that is an absolute error of
    W dp / (p + eps) + u on the first logarithm and W dp / (1 - p + eps) + 2 u on the second;
  * logf is within 1 ulp = 2 u of either logarithm; fl(1 - a), the two products and their sum round once each: 3 u:
    el = W dp (a / (p + eps) + (1 - a) / (1 - p + eps)) + u (a + 2 (1 - a)) + 5 u (a |ln(p + eps)| + (1 - a) |ln(1 - p + eps)|)
    (the kernels add float(1e-7), 1.2e-8 relative off eps: under u / 5 of either logarithm and inside the u above).
  * the sum: 16 terms per lane, 6 wave-shuffle steps, 3 adds of the four waves' sums; k_link_final: ceil(count / 256)
    adds per lane over the count = B ceil(n / 64)^2 per-tile partials, 6 + 3 again; the quotient by the fp64 normaliser
    is rounded once: LEN = 35 + ceil(count / 256) roundings on sum |l|.
  |loss - loss_64| <= (sum el + LEN u sum |l|) / norm.
backward, per element of dS:
  * g: the quotients round once on top of their rounded denominators, fl(1 - a) once, the sum of the two once:
    eg = W dp h(a, p) + 5 u (a / (p + eps) + (1 - a) / (1 - p + eps)),  h = a / (p + eps)^2 + (1 - a) / (1 - p + eps)^2
    the second derivative, taken from the fp64 values;
  * E = scale (g_rc + g_cr): the sum, the product and scale = fl(dloss / norm) round once each: 3 u more;
  * dS_rk = sum_c E_rc s_ck on the MFMA: one rounding per product and one per column walked (a column >= n_b adds an
    exact zero), min(n_b, split_tiles CW) columns per split, then k_link_reduce's `splits` adds:
    (columns + splits + 1) u sum_c |E_rc| s_ck.
  |dS - dS_64|_rk <= |dloss| / norm ( sum_c gate (W dp (h_rc + h_cr) + 8 u (gabs_rc + gabs_cr)) |s_ck|
                                      + (columns + splits + 1) u sum_c |G_rc| |s_ck| ),
  and accumulate = 1 adds the rounding of fl(old + d): u |old + d|.
qualification.  The first-order terms neglect dp^2 / (1 - p)^2 and a gate that flips.  An input qualifies for these
  bounds only when every inexact P entry has 1 - p >= 64 (K + 1) u in float64: then dp / (1 - p) <= 1 / 64, the second
  order term is under 1/64 of the first (hence W), and no fp32 raw reaches 1 where the fp64 one is below it.  Inputs
  that do not qualify (sharp assignments: fp32 resolves 1 - p to 6e-8) are held to the anchored criterion of
  tests/test_gpu_csr_linkpred.py instead: max|dS_hip - dS_64| <= 4 max|dS_fp32formula - dS_64| + 3e-7 max|dS_64|.

`python -m tests.linkpred_cases` prints the table with its plans; `--digest <file> <out>` makes
profiles/linkpred_fp64_anchor.txt from the per-case file tests/test_gpu_linkpred_matrix.py appends under
DP_LINKPRED_ANCHOR_OUT.
"""
import collections
import os
import sys
import zlib

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-7
W1 = 1.0 + 1.0 / 64.0
K_MAX = 256
K_EDGES = (1, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 256)
N_SIZES = (1, 7, 63, 64, 65, 100, 127, 128, 129, 131, 260)
PINNED_PLANS = {(20, 500, 50): (4, 64, 8, 4, 2), (1, 260, 256): (16, 32, 9, 9, 1), (256, 128, 8): (1, 64, 2, 1, 2),
                (512, 64, 192): (12, 32, 2, 1, 2), (30, 321, 20): (2, 64, 6, 3, 2)}


# ------------------------------------------------------------------ the plan, restated (dp_linkpred_plan)
def plan(B, n, K):
    """(KT, CW, col_tiles, splits, split_tiles, forward tiles per graph, forward LDS bytes, backward LDS bytes)."""
    kt16 = (K + 15) // 16
    kt = next((s for s in (1, 2, 3, 4, 6, 8, 12, 16) if kt16 <= s), 0)
    assert kt, "K > 256 has no plan"
    cw = 32 if kt >= 12 else 64
    col_tiles = -(-n // cw)
    base = -(-n // 64) * B
    splits = min(max(-(-512 // base), 1), col_tiles)
    split_tiles = -(-col_tiles // splits)
    splits = -(-col_tiles // split_tiles)
    kp = kt * 16 + 2
    return (kt, cw, col_tiles, splits, split_tiles, (-(-n // 64)) ** 2, 4 * (2 * 64 * kp + 4),
            4 * ((64 + cw) * kp + 64 * (cw + 4) + cw * 65))


def plan_class(B, n, K):
    kt, cw, col_tiles, splits, split_tiles = plan(B, n, K)[:5]
    if col_tiles == 1:
        return "one_tile"
    if splits == 1:
        return f"nonsplit_cw{cw}"
    if split_tiles == 1:
        return f"split_all_cw{cw}"
    return f"split_{'even' if col_tiles % split_tiles == 0 else 'ragged'}_cw{cw}"


# ------------------------------------------------------------------ the case table
# nn: None (num_nodes NULL), "full" (every n_b = n), a list (cycled over the batch)
# adj: sym / dir (0/1), weighted (values in (0, 1) bf16 cannot hold: fp32 reader only), quarter (0.25 / 0.5),
#      outside7 (directed 0/1, 7.0 everywhere outside the n_b x n_b blocks), loops: self loops on
# skind: softmax (2 randn), ties (softmax with one-hot pairs planted), grid (multiples of 1/4, row sums up to 1.5),
#        sharp (softmax(12 randn): does not qualify for the counted bound)
# padnan: the packed rows' padding columns n .. ld-1 hold the bf16 NaN pattern 0x7FC0;  via: "link" = dp_linkpred_loss_*,
# "loss" = dp_loss_forward / dp_loss_backward (accumulate = 0 only);  norm: link_norm = 1.5 sum n_b^2 given
Case = collections.namedtuple("Case", "name B n K nn adj skind dloss acc norm padnan via")


def _c(name, B, n, K, nn=None, adj="sym", skind="softmax", dloss=None, acc=0, norm=False, padnan=False, via="link"):
    return Case(name, B, n, K, nn, adj, skind, dloss, acc, norm, padnan, via)


CASES = [
    # every K tier edge, each at another n / mask / adjacency / scalar combination
    _c("k1_n1", 2, 1, 1),
    _c("k1_n65", 3, 65, 1, [65, 1, 33], adj="sym_loops", dloss=1.7),
    _c("k16_n7", 2, 7, 16, adj="dir", dloss=-0.6, acc=1),
    _c("k17_n63", 2, 63, 17, [63, 40]),
    _c("k32_n64", 2, 64, 32, "full", adj="dir", dloss=1.7),
    _c("k33_n65", 2, 65, 33, [65, 64], acc=1),
    _c("k48_n100", 2, 100, 48, [63, 100], adj="weighted"),
    _c("k49_n127", 1, 127, 49),
    _c("k64_n128", 2, 128, 64, [128, 65], adj="dir", dloss=-0.6),
    _c("k65_n129", 2, 129, 65, [128, 129], acc=1, padnan=True),
    _c("k96_n131", 2, 131, 96, [131, 64], adj="quarter"),
    _c("k97_n100", 1, 100, 97, adj="dir", padnan=True),
    _c("k128_n129", 2, 129, 128, [129, 1], adj="sym_loops"),
    _c("k129_n131", 2, 131, 129, [63, 131], adj="dir", acc=1),
    _c("k192_n127", 1, 127, 192, "full", dloss=1.7),
    _c("k193_n65", 2, 65, 193, [65, 33], adj="dir"),
    _c("k256_n260", 1, 260, 256),
    # K % 4 != 0 inside a tier; split form with row blocks and whole splits beyond n_b, accumulate 0 and 1
    _c("k50_n260_beyond", 2, 260, 50, [260, 65]),
    _c("k50_n260_beyond_acc", 2, 260, 50, [260, 65], acc=1, dloss=1.7),
    _c("k150_n131", 2, 131, 150, [131, 100], adj="weighted", dloss=-0.6),
    # masks
    _c("nb0", 3, 100, 20, [100, 0, 37]),
    _c("nb1", 2, 64, 20, [1, 1], adj="sym_loops"),
    _c("outside7", 2, 131, 20, [65, 100], adj="outside7", padnan=True),
    # values of P
    _c("ties", 2, 100, 10, [100, 64], skind="ties", dloss=1.7),
    _c("ties_dir_acc", 2, 65, 17, [65, 40], adj="dir", skind="ties", acc=1),
    _c("grid", 2, 131, 8, [131, 70], skind="grid"),
    _c("grid_dir", 2, 100, 33, [100, 64], adj="dir", skind="grid", dloss=-0.6),
    # link_norm, through the loss entries
    _c("norm", 3, 100, 20, [100, 37, 64], dloss=1.7, norm=True, via="loss"),
    _c("norm_dir", 2, 129, 50, [129, 65], adj="dir", norm=True, via="loss"),
    _c("loss_nonorm", 2, 65, 17, [65, 20], dloss=-0.6, via="loss"),
    # the backward plans only a large batch reaches
    _c("nonsplit64", 256, 128, 16, [128, 64, 100, 1, 65, 128, 37], dloss=1.7),
    _c("nonsplit64_acc", 256, 128, 9, [128, 64, 100, 1, 65, 128, 37], adj="dir", acc=1),
    _c("nonsplit32", 512, 64, 129, [64, 33, 64, 1, 50]),
    _c("split_even64", 30, 321, 20, [321, 128, 300, 65], dloss=1.7),
    _c("split_even32", 58, 165, 193, [165, 64, 130], adj="dir", acc=1),
    _c("split_ragged", 60, 300, 50, [300, 192, 250, 70], adj="dir"),
    # sharp assignments: the anchored criterion
    _c("sharp", 2, 256, 50, skind="sharp", dloss=1.7),
]
REFUSED = [(2, 64, 257)]           # K = 257: DP_ERR_UNSUPPORTED from all four entries (its twin on the edge: k256_n260)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def readers(c):
    return ("f32",) if c.adj == "weighted" else ("f32", "packed")


def qualifies(c):
    return c.skind != "sharp"


def bf16_exact(c):
    return c.adj != "weighted"


def node_counts(c):
    """int array [B] of n_b (None / "full": n)."""
    if c.nn is None or c.nn == "full":
        return np.full(c.B, c.n, dtype=np.int32)
    return np.array([c.nn[b % len(c.nn)] for b in range(c.B)], dtype=np.int32)


# ------------------------------------------------------------------ inputs
def quarter_grid(rng, rows, K, draws=6):
    """Multiples of 1/4 with row sums up to 1.5: every product and sum the kernels form is exact in fp32, and raw
    reaches values below, at and above 1."""
    S = np.zeros((rows, K), dtype=np.float32)
    # most of the mass on three columns, so that rows meet often enough for raw to pass 1 at any K
    idx = np.where(rng.random((rows, draws)) < 0.7, rng.integers(0, min(K, 3), (rows, draws)), rng.integers(0, K, (rows, draws)))
    keep = rng.random((rows, draws)) < 0.8
    for d in range(draws):
        np.add.at(S, (np.arange(rows)[keep[:, d]], idx[keep[:, d], d]), np.float32(0.25))
    return S


def _softmax(rng, shape, scale):
    z = rng.standard_normal(shape) * scale
    z -= z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


TIE_ROWS = (0, 1, 5, 6)             # one-hot on one cluster: raw == 1 exactly on and off the diagonal


def build(c):
    """dict: S [B, n, K], A [B, n, n] float32, nn (int32 [B] or None), nnv (always an array), dloss, norm (float or None).
    Every row of S is filled, also rows >= n_b: the mask, not a zero row, has to keep them out."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    B, n, K = c.B, c.n, c.K
    nnv = node_counts(c)
    if c.skind == "grid":
        S = quarter_grid(rng, B * n, K).reshape(B, n, K)
    else:
        S = _softmax(rng, (B, n, K), 12.0 if c.skind == "sharp" else 2.0)
    if c.skind == "ties":
        S[:, TIE_ROWS, :] = 0.0
        S[:, TIE_ROWS, min(2, K - 1)] = 1.0
    A = (rng.random((B, n, n)) < 0.2)
    if c.adj in ("sym", "sym_loops", "weighted", "quarter"):
        A = np.triu(A, 1)
        A = A | A.transpose(0, 2, 1)
    else:
        A = A & ~np.eye(n, dtype=bool)[None]
    A = A.astype(np.float32)
    if c.adj == "sym_loops":
        A += np.eye(n, dtype=np.float32)[None]
    if c.adj == "weighted":
        w = rng.uniform(0.05, 0.95, (B, n, n)).astype(np.float32)
        A *= np.triu(w, 1) + np.triu(w, 1).transpose(0, 2, 1)
    if c.adj == "quarter":
        w = np.where(rng.random((B, n, n)) < 0.5, 0.25, 0.5).astype(np.float32)
        A *= np.triu(w, 1) + np.triu(w, 1).transpose(0, 2, 1)
    if c.skind == "ties":            # the tied pairs with a = 1 and a = 0, on and off the diagonal
        A[:, 0, 0], A[:, 1, 1] = 1.0, 0.0
        A[:, 0, 1], A[:, 1, 0] = 1.0, 1.0
        A[:, 5, 6], A[:, 6, 5] = 0.0, 0.0
    for b in range(B):
        nb = int(nnv[b])
        fill = 7.0 if c.adj == "outside7" else 0.0
        A[b, nb:, :] = fill
        A[b, :, nb:] = fill
    norm = float(np.float32(1.5 * float((nnv.astype(np.float64) ** 2).sum()))) if c.norm else None
    return dict(S=S, A=A, nn=None if c.nn is None else nnv, nnv=nnv, dloss=c.dloss, norm=norm)


def pack(A, ld, padnan):
    """bf16 rows [B, n, ld] (uint16 bit patterns) of A and of A^T; A must be bf16-exact."""
    bits = np.ascontiguousarray(A).view(np.uint32)
    assert not (bits & 0xFFFF).any(), "the adjacency is not bf16-exact"
    B, n, _ = A.shape
    out = []
    for src in (bits, np.ascontiguousarray(bits.transpose(0, 2, 1))):
        pk = np.full((B, n, ld), 0x7FC0 if padnan else 0, dtype=np.uint16)
        pk[:, :, :n] = (src >> 16).astype(np.uint16)
        out.append(pk)
    return out[0], out[1]


# ------------------------------------------------------------------ the fp64 reference and the bound's terms
FAULTS = ("tie_gate_1", "a_for_at", "mask_at_n", "last_tile_dropped", "split_omitted", "block_unwritten",
          "block_zeroed", "norm_ignored")
# the row each planted defect has to be caught on
FAULT_ROW = {"tie_gate_1": "ties", "a_for_at": "k64_n128", "mask_at_n": "outside7", "last_tile_dropped": "k49_n127",
             "split_omitted": "split_ragged", "block_unwritten": "k50_n260_beyond",
             "block_zeroed": "k50_n260_beyond_acc", "norm_ignored": "norm"}


def _graph(a, s, K, exact_all, dtype=torch.float64, gate_tie=0.5, cols=None, a_for_at=False, bounds=True):
    """One graph cut to its block: a [m, m], s [m, K] (torch, fp32 values).  Returns (sum l, d sum l / d s) in `dtype`
    by autograd and, in float64, the terms of the bounds.  Planted defects of the backward's tile walk: cols: row
    block r walks only these columns, so E_rc is lost for every other c; a_for_at: E_rc = 2 g(a_rc) (A read for A^T)."""
    s = s.to(dtype).clone().requires_grad_(True)
    a = a.to(dtype)
    raw = s @ s.t()
    if gate_tie == 0.5:
        p = torch.minimum(raw, torch.ones((), dtype=dtype))
    else:                            # a defect: the whole gradient on ties
        p = torch.where(raw <= 1, raw, torch.ones((), dtype=dtype))
    l = -a * torch.log(p + EPS) - (1 - a) * torch.log(1 - p + EPS)
    tot = l.sum()
    (g,) = torch.autograd.grad(tot, s)
    out = dict(sum=float(tot.detach()), grad=g.detach())
    if cols is not None or a_for_at:
        with torch.no_grad():
            sd, pd = s.detach(), p.detach()
            gv = torch.where(raw.detach() < 1, 1.0, torch.where(raw.detach() == 1, 0.5, 0.0)).to(dtype) * (
                -a / (pd + EPS) + (1 - a) / (1 - pd + EPS))
            G = 2 * gv if a_for_at else gv + gv.t()
            if cols is not None:
                keep = torch.zeros_like(G)
                keep[:, cols] = 1
                G = G * keep
            out["grad"] = G @ sd
    if not bounds:
        return out
    with torch.no_grad():
        s, raw, p = s.detach(), raw.detach(), p.detach()
        nz = (s != 0).sum(dim=1)
        exact = torch.ones_like(raw, dtype=torch.bool) if exact_all else ((nz[:, None] <= 1) & (nz[None, :] <= 1))
        dp = torch.where(exact, torch.zeros_like(p), (K + 1) * U * p)
        i1, i2 = 1.0 / (p + EPS), 1.0 / (1 - p + EPS)
        lab = a * torch.log(p + EPS).abs() + (1 - a) * torch.log(1 - p + EPS).abs()
        el = W1 * dp * (a * i1 + (1 - a) * i2) + U * (a + 2 * (1 - a)) + 5 * U * lab
        gate = torch.where(raw < 1, 1.0, torch.where(raw == 1, 0.5, 0.0)).to(torch.float64)
        gabs = a * i1 + (1 - a) * i2
        h = a * i1 * i1 + (1 - a) * i2 * i2
        gval = gate * (-a * i1 + (1 - a) * i2)
        G = gval + gval.t()
        eE = gate * (W1 * dp * (h + h.t()) + 8 * U * (gabs + gabs.t()))
        sa = s.abs()
        out.update(el=float(el.sum()), lab=float(lab.sum()), ein=eE @ sa, mag=G.abs() @ sa,
                   margin=float((1 - p)[~exact].min()) if (~exact).any() else float("inf"),
                   near=float((1 - raw)[~exact].abs().min()) if (~exact).any() else float("inf"),
                   ties=int((raw == 1).sum()), above=int((raw > 1).sum()), below=int((raw < 1).sum()))
    return out


def reference(c, inp, dtype=torch.float64, fault=None, bounds=True):
    """loss, dS per graph ([n_b, K], dloss and the normaliser applied), and (bounds=True) the bound of the loss and of
    every element of dS.  dtype=torch.float32 is the direct fp32 formula; `fault` plants a defect (float64)."""
    B, n, K = c.B, c.n, c.K
    kt, cw, col_tiles, splits, split_tiles = plan(B, n, K)[:5]
    nnv = inp["nnv"]
    norm = inp["norm"] if inp["norm"] is not None else float((nnv.astype(np.float64) ** 2).sum())
    if fault == "norm_ignored":
        norm = float((nnv.astype(np.float64) ** 2).sum())
    dl = 1.0 if inp["dloss"] is None else float(inp["dloss"])
    S, A = torch.from_numpy(inp["S"]), torch.from_numpy(inp["A"])
    tot = el = lab = 0.0
    dS, bnd, info = [], [], dict(margin=float("inf"), near=float("inf"), ties=0, above=0, below=0)
    for b in range(B):
        m = n if fault == "mask_at_n" else int(nnv[b])
        a = A[b, :m, :m]
        cols = None
        if fault == "last_tile_dropped":
            cols = np.arange(0, min(m, (col_tiles - 1) * cw)) if col_tiles > 1 else np.arange(0, max(m - cw // 2, 0))
        if fault == "split_omitted":                  # the first split's partial never reaches the sum
            cols = np.arange(min(m, split_tiles * cw), m)
        if m == 0:
            dS.append(torch.zeros(0, K, dtype=dtype))
            bnd.append(torch.zeros(0, K, dtype=torch.float64))
            continue
        r = _graph(a, S[b, :m], K, c.skind == "grid", dtype, 1.0 if fault == "tie_gate_1" else 0.5, cols,
                   fault == "a_for_at", bounds)
        tot += r["sum"]
        dS.append(r["grad"] * (dl / norm))
        if bounds:
            el, lab = el + r["el"], lab + r["lab"]
            walked = min(m, split_tiles * cw)
            bnd.append((r["ein"] + (walked + splits + 1) * U * r["mag"]) * (abs(dl) / norm))
            info["margin"], info["near"] = min(info["margin"], r["margin"]), min(info["near"], r["near"])
            for k in ("ties", "above", "below"):
                info[k] += r[k]
    out = dict(loss=tot / norm, dS=dS, norm=norm, dloss=dl)
    if bounds:
        count = B * plan(B, n, K)[5]
        out.update(loss_bound=(el + (35 + -(-count // 256)) * U * lab) / norm, dS_bound=bnd, **info)
    return out


def prior(c, ref):
    """What dS holds before an accumulating call: 0.25 max|dS_64| in size, every element of [B, n, K]."""
    top = max((float(d.abs().max()) for d in ref["dS"] if d.numel()), default=1.0)
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + 1)
    return (0.25 * top * rng.choice([-1.0, 1.0], (c.B, c.n, c.K)) * rng.uniform(0.5, 1.0, (c.B, c.n, c.K))).astype(np.float32)


def full_output(c, inp, res, old=None):
    """[B, n, K] float32 of a result given per graph (res["dS"]), as a correct entry leaves the buffer: rows >= n_b hold
    0, or `old` under accumulate, and the valid rows old + d."""
    out = np.zeros((c.B, c.n, c.K), dtype=np.float32) if old is None else old.copy()
    for b in range(c.B):
        m = min(res["dS"][b].shape[0], c.n)
        d = res["dS"][b].to(torch.float64).numpy()[:m]
        out[b, :m] = (d + (old[b, :m].astype(np.float64) if old is not None else 0.0)).astype(np.float32)
        if old is None:
            out[b, m:] = 0.0
    return out


def compare(c, inp, ref, loss, dS, old=None):
    """The GPU test's comparison, also fed with the fp32 formula and the planted defects: loss (float) and dS
    ([B, n, K] float32 as the entry left it) against `ref` (float64, with bounds).  Returns dict(fwd, bwd: the largest
    |error| / bound; problems: what failed)."""
    problems = []
    fr = abs(float(loss) - ref["loss"]) / ref["loss_bound"] if ref["loss_bound"] > 0 else float(loss != ref["loss"])
    if not np.isfinite(float(loss)) or fr > 1.0:
        problems.append(f"loss {float(loss)!r} vs {ref['loss']!r}: {fr:.3f} of the bound")
    br = 0.0
    for b in range(c.B):
        m = int(inp["nnv"][b])
        got = dS[b]
        if old is None:
            if not (got[m:] == 0).all():          # NaN != 0: an unwritten row fails here
                problems.append(f"graph {b}: rows >= n_b = {m} are not exactly 0")
        elif got[m:].tobytes() != old[b, m:].tobytes():
            problems.append(f"graph {b}: rows >= n_b = {m} changed under accumulate")
        if m == 0:
            continue
        want = ref["dS"][b].numpy()
        tol = ref["dS_bound"][b].numpy()
        if old is not None:
            want = want + old[b, :m].astype(np.float64)
            tol = tol + U * (np.abs(want) + tol)
        err = np.abs(got[:m].astype(np.float64) - want)
        if not np.isfinite(got[:m]).all():
            problems.append(f"graph {b}: non-finite dS")
            br = float("inf")
            continue
        ratio = float((err / np.maximum(tol, 1e-300)).max()) if (tol > 0).all() else float(
            np.where(tol > 0, err / np.maximum(tol, 1e-300), np.where(err > 0, np.inf, 0.0)).max())
        br = max(br, ratio)
        if ratio > 1.0:
            i = np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape)
            problems.append(f"graph {b}: dS{i} = {got[:m][i]!r} vs {want[i]!r}: {ratio:.3f} of the bound")
    return dict(fwd=fr, bwd=br, problems=problems)


def sharp_compare(ref, f32, loss, dS, nnv):
    """The anchored criterion on an input that does not qualify: (e_hip, e_formula32, max|dS_64|, loss errors, ok)."""
    e_hip = max(float(np.abs(dS[b, :int(nnv[b])].astype(np.float64) - ref["dS"][b].numpy()).max()) for b in range(len(nnv)))
    e_o32 = max(float((f32["dS"][b].double() - ref["dS"][b]).abs().max()) for b in range(len(nnv)))
    top = max(float(d.abs().max()) for d in ref["dS"])
    l_hip, l_o32 = abs(float(loss) - ref["loss"]), abs(f32["loss"] - ref["loss"])
    ok = e_hip <= 4 * e_o32 + 3e-7 * top and l_hip <= 4 * l_o32 + 1e-6 * abs(ref["loss"])
    return dict(e_hip=e_hip, e_o32=e_o32, top=top, l_hip=l_hip, l_o32=l_o32, ok=ok)


# ------------------------------------------------------------------ recorded results
def record(c, reader, got_plan, fwd, bwd, f32=None, extra=""):
    """Appends one line per case and reader to the file DP_LINKPRED_ANCHOR_OUT names."""
    path = os.environ.get("DP_LINKPRED_ANCHOR_OUT")
    if not path:
        return
    with open(path, "a") as f:
        f.write(f"{c.name} {reader} {plan_class(c.B, c.n, c.K)} {'x'.join(map(str, got_plan[:5]))} {c.acc} {fwd:.4f} {bwd:.4f} "
                f"{f32[0] if f32 else 0.0:.4f} {f32[1] if f32 else 0.0:.4f} {extra}\n")


def digest(src, dst):
    """profiles/linkpred_fp64_anchor.txt from the per-case file tests/test_gpu_linkpred_matrix.py appends."""
    rows, sharp = [], []
    for line in open(src):
        t = line.split()
        (sharp if t[0].startswith("sharp") else rows).append(t)
    with open(dst, "w") as f:
        f.write("# tests/test_gpu_linkpred_matrix.py on an MI355X (gfx950): largest |error| / bound per case and reader against\n"
                "# the fp64 reference (bounds: tests/linkpred_cases.py, counted, u = 2^-24); plan = KT x CW x col_tiles x splits\n"
                "# x split_tiles as dp_linkpred_plan answered it; formula32: the same ratios of the direct fp32 formula (torch,\n"
                "# CPU) on that input.  Made by `python -m tests.linkpred_cases --digest <DP_LINKPRED_ANCHOR_OUT file> <this file>`.\n")
        f.write("# accumulate = 1: the bound also holds the rounding of fl(old + d), u |old + d| with old above d, so that ratio sits\n"
                "# close to 1 by the nature of a rounding unit, for the kernels and the fp32 formula alike.\n")
        f.write(f"{'case':<22}{'reader':<8}{'class':<20}{'plan':<16}{'acc':>4}{'forward':>9}{'backward':>10}{'f32 fwd':>9}{'f32 bwd':>9}\n")
        worst = {"0": [0.0] * 4, "1": [0.0] * 4}
        for t in rows:
            v = [float(x) for x in t[5:9]]
            worst[t[4]] = [max(a, b) for a, b in zip(worst[t[4]], v)]
            f.write(f"{t[0]:<22}{t[1]:<8}{t[2]:<20}{t[3]:<16}{t[4]:>4}{v[0]:>9.4f}{v[1]:>10.4f}{v[2]:>9.4f}{v[3]:>9.4f}\n")
        for acc, w in worst.items():
            f.write(f"{'largest, accumulate = ' + acc:<70}{w[0]:>9.4f}{w[1]:>10.4f}{w[2]:>9.4f}{w[3]:>9.4f}\n")
        for t in sharp:
            f.write(f"# {t[0]} {t[1]} (anchored criterion, not the counted bound): {' '.join(t[9:])}\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--digest"]:
        digest(sys.argv[2], sys.argv[3])
    else:
        for c in CASES:
            print(f"{c.name:<22}{str((c.B, c.n, c.K)):<18}{plan_class(c.B, c.n, c.K):<20}{plan(c.B, c.n, c.K)}")
