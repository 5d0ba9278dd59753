"""Case table, fp64 references and derived error bounds of the fused GAT convolution (dp_csr_gat_conv_fwd / _bwd;
dp_csr_gat_conv_plan restated), shared by tests/test_csr_gat_conv_cpu.py (which shows that these inputs tell a bug from
rounding) and tests/test_gpu_csr_gat_conv.py.  The graphs, the kinds of u and v and the kink are those of
tests/csr_gat_cases.py.

Every reference is float64 on the fp32 inputs; u = 2^-24, first order, counted from the kernels' arithmetic
(dp_csr_gat_conv.hip).  One wave serves a row of `len` entries; in the forward's statistics pass a group of L = 4 / 16 /
64 lanes does (L from the mean row length, `csr_gat_cases.plan`), n_l = ceil(len / L) entries per lane.  expf is
budgeted at 4 u of its value on top of the error of its argument, a division is correctly rounded, a chain of n
additions (or fmas) carries n u sum |terms|.

  scores     as csr_gat_cases.py: |ds_e| <= 2 u |s_e|.
  rowstat    m, zsum per head with L lanes across the entries, then the DPP tree over the group: the bounds of
             csr_gat_cases.py (m: 2 u S_i;  zsum: (6 n_l + 3 D + log2 L + 14 + 4 S_i) u zsum).
  a_eh       fl(expf(fl(s - m)) / zsum), the coefficient of csr_gat_cases.py and its bound:
                 rho_eh = (6 n_l + 3 D + |s - m| + log2 L + 14 + 4 S_i) u, relative.
  forward    Y_ih[c] = sum_e a_eh z_j[c] by fma into four partial sums (entry q of a batch of 64 ids into partial q % 4,
             the batch's last cnt % 4 entries into partial 0), then (p0 + p1) + (p2 + p3): a term passes at most
             n_p + 2 roundings, n_p = ceil(len / 4) + 3 ceil(len / 64):
                 |dY| <= sum_e rho_eh a_eh |z_j[c]| + (n_p + 2) u sum_e a_eh |z_j[c]| + FLT_MIN.
             mean: heads ascending and one division:  (sum_h |dY_h|) / H + (H + 1) u (sum_h |Y_h|) / H + 2 FLT_MIN.
  backward   rowstat (fp32) is an INPUT: the reference takes a_eh = exp(s_eh - m_ih) / zsum_ih on it.  The recomputed
             coefficient: alpha_e = (2 |s| + |s - m| + 5) u, relative (as csr_gat_cases.py).
             dY: exact (concat) or fl(dy / H), one u (mean; `q` below is 1 then, else 0).
             g_eh = dY_ih . z_j^h: per lane an fma chain over its at most K = 8 slots, a sum over its groups (inside the
             same K), the 6 steps of the tree:   dg_e = (K + 6 + q) u sum_c |dY z|.
             t_i = sum_row a g, one fma chain:   dt_i = sum_row ((alpha_e + u) |a g| + a dg_e) + len u sum_row |a g|.
             dpre = fl(fl(a fl(g - t)) s'):
                 ddpre_e = |s'| a (dg_e + dt_i) + (alpha_e + 3 u) |dpre_e| + FLT_MIN (1 + |g| + |t|).
             du_i = sum_row dpre, one chain:   sum_row ddpre + len u sum_row |dpre|;
             dv_c = sum_col dpre likewise with len_T(c) (the column pass reads the fp32 t of the row pass and recomputes
             the same a and, bit for bit, the same g).
             dz_c[x] = sum_col a dY_r[x], one fma chain:
                 sum_col (alpha_e + q u) a |dY| + (len_T + 1) u sum_col a |dY| + FLT_MIN.

The exact statements: a one-entry row has a = expf(0) / 1 = 1, so y_i = fma(1, z_j, 0) = z_j bit for bit, t = g and
dpre = 0; a row of 2^k entries with equal v_j has zsum = 2^k and a = 2^-k exactly, and with z on the grid of 2^-6 (the
'equal' kind) every partial sum of Y is exact, whatever its order."""
import functools

import numpy as np

from tests import csr_gat_cases as GC
from tests.csr_gat_cases import FLT_MIN, MARGIN, U, _seed, col_len, moved, row_len      # noqa: F401  (re-exported)

MAX_WIDTH = 512
# (H, C): width 1; the 64-column chunk edge from both sides; a chunk that straddles heads with C % 4 != 0; two heads in one
# 16-byte quad; the limit; and the widths that reach the 4-chunk form (130) and the 2-chunk 16-byte form whose quads
# straddle heads (260)
PAIRS = ((1, 1), (3, 21), (4, 16), (1, 65), (3, 5), (8, 1), (8, 64), (2, 65), (4, 65))
LAYOUTS = {"tight": (lambda w: w, 0), "pad4": (lambda w: 4 * (w // 4 + 1), 0),
           "odd": (lambda w: w + 1 if w % 2 == 0 else w + 2, 0), "mis": (lambda w: 4 * (w // 4 + 1), 1)}
KINDS = GC.KINDS
SLOPES = GC.SLOPES
ZGRID = 64.0
GRAPHS = GC.GRAPHS + ("tiny",)


def _tiny():
    """Seven nodes for what the graphs of csr_gat_cases.py lack, a column without entries: row 0 holds nothing, nobody
    points at node 6, rows 1 and 6 hold one entry, node 3 a self loop."""
    src, dst = [1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 6], [0, 1, 3, 3, 0, 5, 0, 1, 2, 5, 4, 2, 2]
    g = GC.Csr(7, src, dst, 77, True)
    order = np.lexsort((g.rows, g.indices))                 # the transposed CSR: by column, source rows ascending
    g.indices_t = g.rows[order].astype(np.int32)
    g.indptr_t = np.concatenate([[0], np.cumsum(np.bincount(g.indices, minlength=g.n))]).astype(np.int32)
    g.lanes = GC.plan(g.n, g.nnz, 1, 1, 0)[0]
    return g


_TINY = []


def graph(name):
    """The case graph: "tiny" is this module's own, every other name one of `csr_gat_cases.graph`."""
    if name != "tiny":
        return GC.graph(name)
    if not _TINY:
        _TINY.append(_tiny())
    return _TINY[0]


def _tiny_uv(case):
    """u, v [n, H] of the tiny graph on the grids of csr_gat_cases.py (2^-12, and 2^-12 + 2^-13), the kink u_i = -v_j
    planted on the first entry of every third row; the margin of every other |pre| is asserted."""
    gname, H, _, kind, _ = case
    assert kind in ("ordinary", "kink")
    g = graph(gname)
    rng = np.random.default_rng(_seed("gatc-uv-" + case_id(case)))
    u = (np.rint(rng.uniform(-3.0, 3.0, (g.n, H)) * 4096.0) / 4096.0).astype(np.float32)
    v = ((np.rint(rng.uniform(-3.0, 3.0, (g.n, H)) * 4096.0) + 0.5) / 4096.0).astype(np.float32)
    if kind == "kink":
        rows = np.arange(0, g.n, 3)
        rows = rows[row_len(g)[rows] > 0]
        u[rows] = -v[g.indices[g.indptr[rows]]]
    pre = u.astype(np.float64)[g.rows] + v.astype(np.float64)[g.indices]
    assert np.array_equal(pre, (u[g.rows] + v[g.indices]).astype(np.float64))      # exact in fp32
    zero = pre == 0
    assert (np.abs(pre[~zero]) >= MARGIN).all() and zero.any() == (kind == "kink")
    return u, v


def plan(n_rows, nnz, H, C, ld, misaligned):
    """(floats per load, column chunks per lane, one coefficient per quad, rows per workgroup, columns per lane, lanes per
    row of the statistics pass) as dp_csr_gat_conv_plan answers.  The backward: ld = ldz | lddy, misaligned = z or dy
    off the 16-byte grid, or the mean with C % 4 != 0."""
    W = H * C
    vec = 4 if W % 4 == 0 and ld % 4 == 0 and not misaligned else 1
    need = -(-W // (64 * vec))
    nch = 1 if need <= 1 else (2 if need <= 2 else (4 if need <= 4 else 8))
    return vec, nch, int(vec == 4 and C % 4 == 0), 4, vec * nch, GC.plan(n_rows, nnz, 1, 1, 0)[0]


# ------------------------------------------------------------------ the table: (graph, H, C, layout, kind, slope, mean)
def _table():
    cases, lay = [], list(LAYOUTS)
    small = ("t4-n576", "t4-n577", "undirected", "batch")          # the graphs that carry the widest pairs
    for gi, gname in enumerate(GC.GRAPHS):                         # every graph at every pair, layouts and modes in turn
        for pi, (H, C) in enumerate(PAIRS):
            if H * C > 130 and gname not in small:
                continue
            cases.append((gname, H, C, lay[(gi + pi) % 4], "ordinary", 0.2, (gi + pi) % 2))
    for H, C in PAIRS:                                             # every pair in every layout and both modes
        gname = "t4-n577" if H * C > 130 else "t16-n577"
        for li, layout in enumerate(lay):
            for mean in (0, 1):
                cases.append((gname, H, C, layout, "ordinary", 0.2, mean))
    for kind in KINDS[1:]:                                         # the other inputs
        for gname, layout, (H, C) in (("t4-n577", "odd", (3, 5)), ("t64-n576", "pad4", (4, 16)), ("batch", "tight", (8, 1)),
                                      ("t16-n576", "mis", (3, 21))):
            for mean in (0, 1):
                cases.append((gname, H, C, layout, kind, 0.2, mean))
    for pi, (H, C) in enumerate(PAIRS):                            # a row and a column without entries, every pair
        for mean in (0, 1):
            cases.append(("tiny", H, C, lay[pi % 4], "ordinary", 0.2, mean))
    cases.append(("tiny", 3, 5, "tight", "kink", 0.0, 0))
    for H, C in PAIRS:                                             # exact 2^-k at every pair
        cases.append(("t4-n576" if H * C > 130 else "t16-n576", H, C, "tight", "equal", 0.2, 0))
    for slope in SLOPES[1:]:                                       # slope 1 (u_i cancels), slope 0 (whole rows may tie)
        for gname, layout, (H, C) in (("t4-n576", "mis", (4, 16)), ("t16-n577", "pad4", (1, 65)),
                                      ("undirected", "odd", (3, 21))):
            for mean in (0, 1):
                cases.append((gname, H, C, layout, "ordinary", slope, mean))
        cases.append(("batch", 3, 5, "pad4", "kink", slope, 0))
        cases.append(("t16-n576", 8, 1, "tight", "ties", slope, 1))
    return list(dict.fromkeys(cases))


CASES = _table()


def case_id(case):
    return "-".join(str(c) for c in case)


def widths(case):
    """(W, width of y and dy)."""
    W = case[1] * case[2]
    return W, case[2] if case[6] else W


def layout_of(case, width):
    """(ld, off) of a buffer of `width` columns in the case's layout."""
    ld, off = LAYOUTS[case[3]]
    return ld(width), off


def case_plans(case):
    """(the forward's plan, the backward's)."""
    W, wy = widths(case)
    (ldz, off), (lddy, _) = layout_of(case, W), layout_of(case, wy)
    g = graph(case[0])
    return (plan(g.n, g.nnz, case[1], case[2], ldz, off),
            plan(g.n, g.nnz, case[1], case[2], ldz | lddy, off or (case[6] and case[2] % 4 != 0)))


def uv_case(case):
    """The case of csr_gat_cases.py whose u, v these are."""
    return (case[0], case[1], case[3], case[4], case[5])


@functools.lru_cache(maxsize=4)
def inputs(case):
    """(z [n, W], u, v [n, H], dy [n, W or C]) fp32.  u, v: `csr_gat_cases.inputs` (the kink planted and its margin
    asserted there; the tiny graph's by `_tiny_uv`); z, dy U(-1, 1), in the 'equal' kind on the grid of 2^-6."""
    g = graph(case[0])
    u, v = _tiny_uv(uv_case(case)) if case[0] == "tiny" else GC.inputs(uv_case(case))
    W, wy = widths(case)
    rng = np.random.default_rng(_seed("gatc-" + case_id(case)))
    z = rng.uniform(-1.0, 1.0, (g.n, W)).astype(np.float32)
    dy = rng.uniform(-1.0, 1.0, (g.n, wy)).astype(np.float32)
    if case[4] == "equal":
        z = (np.rint(z * ZGRID) / ZGRID).astype(np.float32)
    return z, u, v, dy


def padded(x, ld, fill=np.nan):
    return GC.padded(x, ld, fill)


def stat_lanes(g):
    """Lanes per row of the forward's statistics pass."""
    return GC.plan(g.n, g.nnz, 1, 1, 0)[0]


def _seg_sum(idx, x, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, idx, x)
    return out


def _wide(a, C):
    """[., H] -> [., H C]: every head's value under its C columns."""
    return np.repeat(a, C, axis=1)


# ------------------------------------------------------------------ forward
def fwd_ref(g, z, u, v, slope, C, mean, drop_last=False, v_head=0, slice_off=0, drop_chunk=False, no_mean=False):
    """(y, bound, rowstat [n, 2H], rowstat bound).  The keyword arguments are a faulty kernel's: every row's last entry
    left out, v_j read at head h + v_head, the feature slice slice_off columns on, the last partial 64-column chunk not
    stored (zeros), the 1 / H of the mean missing."""
    H = u.shape[1]
    W = H * C
    if v_head:
        v = np.roll(v, -v_head, axis=1)
    _, s = GC._scores(g, u, v, slope)
    L = stat_lanes(g)
    _, _, stat, sbound = GC.fwd_ref(g, u, v, slope, lanes=L, drop_last=drop_last)
    live = np.ones(g.nnz, dtype=bool)
    if drop_last:
        live[g.indptr[1:][row_len(g) > 0] - 1] = False
    m, zs = stat[:, :H], stat[:, H:]
    lens = row_len(g)
    lo, big = np.full((g.n, H), np.inf), np.zeros((g.n, H))
    np.minimum.at(lo, g.rows[live], s[live])
    np.maximum.at(big, g.rows, np.abs(s))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.where(live[:, None], np.exp(s - m[g.rows]) / zs[g.rows], 0.0)
        n_l = (-(-lens // L))[:, None]
        base = 6 * n_l + 3 * (m - lo) + np.log2(L) + 14 + 4 * big
        rho = (base[g.rows] + np.abs(s - m[g.rows])) * U
    zj = np.asarray(z, np.float64)[g.indices]
    if slice_off:
        zj = np.roll(zj, -slice_off, axis=1)
    aw, rw = _wide(a, C), _wide(np.where(live[:, None], rho, 0.0), C)
    Y = _seg_sum(g.rows, aw * zj, g.n)
    mag = _seg_sum(g.rows, aw * np.abs(zj), g.n)
    n_p = (-(-lens // 4) + 3 * -(-lens // 64))[:, None]
    bY = _seg_sum(g.rows, rw * aw * np.abs(zj), g.n) + (n_p + 2) * U * mag + FLT_MIN
    if drop_chunk and W % 64:
        Y[:, W - W % 64:] = 0.0
    if not mean:
        return Y, bY, stat, sbound
    Yh, bh = Y.reshape(g.n, H, C), bY.reshape(g.n, H, C)
    y = Yh.sum(1) / (1 if no_mean else H)
    return y, bh.sum(1) / H + (H + 1) * U * np.abs(Yh).sum(1) / H + 2 * FLT_MIN, stat, sbound


# ------------------------------------------------------------------ backward
def bwd_stat(case):
    """The fp32 rowstat the backward reads: the rounding of the fp64 one."""
    z, u, v, _ = inputs(case)
    g = graph(case[0])
    return GC.fwd_ref(g, u, v, case[5], lanes=stat_lanes(g))[2].astype(np.float32)


def bwd_ref(g, z, u, v, stat, dy, slope, C, mean, kink_one=False, t_shift=0, own_stats=False, over_a=False,
            no_slope=False, no_mean=False):
    """{name: (value, bound)} of du, dv, dz, t on the fp32 rowstat.  The keyword arguments are a faulty kernel's: derivative
    1 at the kink, t of row i + t_shift, the column pass with the column's own rowstat, dz gathered over A for A^T, the
    slope ignored (derivative 1 everywhere), the 1 / H of the mean missing."""
    H = u.shape[1]
    K, q = 8, 1 if mean else 0
    sl = float(np.float32(slope))
    pre, s = GC._scores(g, u, v, slope)
    stat = np.asarray(stat, np.float64)
    m, zs = stat[:, :H], stat[:, H:]
    dy64 = np.asarray(dy, np.float64)
    dY = np.tile(dy64 / (1 if no_mean else H), (1, H)) if mean else dy64                  # [n, W]
    d = np.where((pre >= 0) if kink_one else (pre > 0), 1.0, 1.0 if no_slope else sl)
    rows, cols = g.rows, g.indices.astype(np.int64)
    lens, lens_t = row_len(g)[:, None], col_len(g)[:, None]
    z64 = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = np.exp(s - m[rows]) / zs[rows]
        prod = dY[rows] * z64[cols]                                                        # [nnz, W]
        ge = prod.reshape(g.nnz, H, C).sum(2)
        gabs = np.abs(prod).reshape(g.nnz, H, C).sum(2)
        t = _seg_sum(rows, a * ge, g.n)
        T = _seg_sum(rows, np.abs(a * ge), g.n)
        tt = np.roll(t, -t_shift, axis=0) if t_shift else t
        dpre = a * (ge - tt[rows]) * d
        du = _seg_sum(rows, dpre, g.n)
        if own_stats:
            a_col = np.exp(s - m[cols]) / zs[cols]
            a_col = np.where(np.isfinite(a_col), a_col, 0.0)
            dcol = a_col * (ge - tt[rows]) * d
        else:
            a_col, dcol = a, dpre
        dv = _seg_sum(cols, dcol, g.n)
        if over_a:
            dz = _seg_sum(rows, _wide(a_col, C) * dY[cols], g.n)
        else:
            dz = _seg_sum(cols, _wide(a_col, C) * dY[rows], g.n)
        alpha = (2 * np.abs(s) + np.abs(s - m[rows]) + 5) * U
        dg = (K + 6 + q) * U * gabs
        dt = _seg_sum(rows, (alpha + U) * np.abs(a * ge) + a * dg, g.n) + lens * U * T
        ddpre = np.abs(d) * a * (dg + dt[rows]) + (alpha + 3 * U) * np.abs(dpre) + FLT_MIN * (
            1 + np.abs(ge) + np.abs(t[rows]))
        dub = _seg_sum(rows, ddpre, g.n) + lens * U * _seg_sum(rows, np.abs(dpre), g.n) + FLT_MIN
        dvb = _seg_sum(cols, ddpre, g.n) + lens_t * U * _seg_sum(cols, np.abs(dpre), g.n) + FLT_MIN
        adY = _wide(a, C) * np.abs(dY[rows])
        dzb = _seg_sum(cols, (_wide(alpha, C) + q * U) * adY, g.n) + (lens_t + 1) * U * _seg_sum(cols, adY, g.n) + FLT_MIN
    return {"du": (du, dub), "dv": (dv, dvb), "dz": (dz, dzb), "t": (t, dt + FLT_MIN)}


# ------------------------------------------------------------------ the kernels' order in fp32 (numpy)
def _slot_of(W, vec):
    """(lane, slot) of every column."""
    x = np.arange(W)
    return (x % (64 * vec)) // vec, (x // (64 * vec)) * vec + x % vec


def _fma(a, b, c):
    return (a.astype(np.float64) * b + c).astype(np.float32)


def _coef32(g, u, v, stat, slope):
    """(pre, a) fp32 as the kernels recompute them from rowstat."""
    H = u.shape[1]
    pre, s = GC._scores32(g, u, v, slope)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return pre, (np.exp(s - stat[:, :H][g.rows]).astype(np.float32) / stat[:, H:][g.rows]).astype(np.float32)


def emulate_fwd(g, z, u, v, slope, C, mean):
    """(y, rowstat) of k_gatc_fwd in fp32 numpy, in the kernel's order."""
    H = u.shape[1]
    W = H * C
    _, s = GC._scores32(g, u, v, slope)
    lens = row_len(g)
    L = stat_lanes(g)
    where = GC._place(g.indptr, g.n, L)
    arr = np.full((g.n, L, where[3], H), -np.inf, dtype=np.float32)
    arr[where[0], where[1], where[2]] = s
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = arr.max(axis=(1, 2))
        p = np.exp(s - M[g.rows]).astype(np.float32)
        Z = GC._lane_sums(p, where[:3], g.n, L, where[3])
        stat = np.where((lens == 0)[:, None], 0, np.concatenate([M, Z], axis=1)).astype(np.float32)
        _, a = _coef32(g, u, v, stat, slope)
    # the four partial sums: entry q of a batch of 64 into partial q % 4 while four whole entries remain, else partial 0
    pos = np.arange(g.nnz) - g.indptr.astype(np.int64)[g.rows]
    qb = pos % 64
    cnt = np.minimum(64, lens[g.rows] - (pos - qb))
    part = np.where(qb < 4 * (cnt // 4), qb % 4, 0)
    acc = np.zeros((g.n, 4, W), dtype=np.float32)
    order = np.zeros(g.nnz, dtype=np.int64)                        # the entry's place in its partial's chain
    key = g.rows * 4 + part
    seen = np.zeros(g.n * 4, dtype=np.int64)
    for e in np.argsort(key, kind="stable"):
        order[e] = seen[key[e]]
        seen[key[e]] += 1
    aw = _wide(a, C)
    for step in range(int(order.max(initial=-1)) + 1):
        e = np.nonzero(order == step)[0]
        acc[g.rows[e], part[e]] = _fma(aw[e], z[g.indices[e]], acc[g.rows[e], part[e]])
    Y = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    if not mean:
        return Y, stat
    Yh = Y.reshape(g.n, H, C)
    y = Yh[:, 0]
    for h in range(1, H):
        y = y + Yh[:, h]
    return (y / np.float32(H)).astype(np.float32), stat


def _head_dots32(dYr, zc, H, C, vec, uni):
    """g [entries, H] of gc_head_dots in fp32: per lane its slots of head h (by fma inside a quad where the quad shares a
    head, then the groups added ascending), then the tree over the 64 lanes."""
    E, W = dYr.shape
    lane, slot = _slot_of(W, vec)
    K = int(slot.max()) + 1
    head = np.arange(W) // C
    out = np.zeros((E, H), dtype=np.float32)
    for h in range(H):
        x = np.zeros((E, 64), dtype=np.float32)
        if uni:
            for grp in range(-(-K // 4)):
                pg = np.zeros((E, 64), dtype=np.float32)
                for k in range(4 * grp, 4 * grp + 4):
                    c = np.nonzero((slot == k) & (head == h))[0]
                    pg[:, lane[c]] = _fma(dYr[:, c], zc[:, c], pg[:, lane[c]])
                x = x + pg
        else:
            for k in range(K):
                c = np.nonzero((slot == k) & (head == h))[0]
                x[:, lane[c]] = x[:, lane[c]] + (dYr[:, c] * zc[:, c]).astype(np.float32)
        out[:, h] = GC._tree(x)
    return out


def _chain(x, idx, n, fma_with=None):
    """Per segment the sum of x [entries, .] in ascending entry order, one chain (the entries of a segment are contiguous
    in `idx` order): fp32."""
    order = np.argsort(idx, kind="stable")
    idx_s = idx[order]
    start = np.searchsorted(idx_s, np.arange(n))
    place = np.arange(idx.size) - start[idx_s]
    acc = np.zeros((n,) + x.shape[1:], dtype=np.float32)
    for step in range(int(place.max(initial=-1)) + 1):
        e = order[place == step]
        acc[idx[e]] = (acc[idx[e]] + x[e]) if fma_with is None else _fma(x[e], fma_with[e], acc[idx[e]])
    return acc


def emulate_bwd(g, z, u, v, stat, dy, slope, C, mean, vec, uni):
    """{du, dv, dz, t} of k_gatc_bwd_rows / k_gatc_bwd_cols in fp32 numpy, in the kernels' order."""
    H = u.shape[1]
    dY = np.tile((dy / np.float32(H)).astype(np.float32), (1, H)) if mean else dy
    pre, a = _coef32(g, u, v, stat, slope)
    cols = g.indices.astype(np.int64)
    ge = _head_dots32(dY[g.rows], z[cols], H, C, vec, uni)
    t = _chain(a, g.rows, g.n, fma_with=ge)
    d = np.where(pre > 0, np.float32(1), np.float32(slope)).astype(np.float32)
    dpre = ((a * (ge - t[g.rows])) * d).astype(np.float32)
    du = _chain(dpre, g.rows, g.n)
    # the transposed CSR lists column c's entries by ascending source row: the stable order of `cols`
    dv = _chain(dpre, cols, g.n)
    dz = _chain(_wide(a, C), cols, g.n, fma_with=dY[g.rows])
    return {"du": du, "dv": dv, "dz": dz, "t": t}
