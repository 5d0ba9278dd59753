"""Case table, fp64 references and derived error bounds of the fused additive attention (dp_csr_gat_fwd / _bwd;
dp_csr_gat_plan restated), shared by tests/test_csr_gat_cpu.py (which shows that these inputs tell a bug from rounding)
and tests/test_gpu_csr_gat.py.  The graph builders are those of tests/csr_edge_ops_cases.py.

Every reference is float64 on the fp32 inputs; u = 2^-24, first order, counted from the kernels' arithmetic
(dp_csr_gat.hip).  L lanes serve a row of `len` entries, n_l = ceil(len / L) entries per lane; a segmented sum of terms t
carries (n_l + log2 L) u sum |t| (the lane's entries ascending, then the DPP tree).  expf is budgeted at 4 u of its value
on top of the error of its argument, the division is correctly rounded, as in tests/csr_edge_ops_cases.py.

  scores     pre = fl(u_i + v_j): u |pre|.  s = pre or fl(slope pre): the product carries the relative error of pre and
             rounds once:  |ds_e| <= 2 u |s_e|.
  forward    Per head the row softmax of csr_edge_ops_cases.py on the fp32 scores,
                 (6 n_l + 3 D + |s_e - m_i| + log2 L + 14) u a_e      (D = max - min of the row; covers the register path),
             plus what the score errors move: d log a_e = ds_e - sum_row a ds, at most 2 max_row |ds| = 4 u S_i,
             S_i = max_row |s|:   rho_eh = (6 n_l + 3 D + |s - m| + log2 L + 14 + 4 S_i) u, relative to a_eh.
             The mean adds the H coefficients (at most H roundings of the partial sum <= sum_h a) and divides once:
                 |out err| <= (sum_h rho_eh a_eh) / H + (H + 1) u out_e + 2 FLT_MIN
             (a coefficient and the result below the smallest normal may each be flushed).
             rowstat: m is a maximum of the fp32 scores, |dm| <= 2 u S_i; z relative (6 n_l + 3 D + log2 L + 14 + 4 S_i) u.
  backward   rowstat (fp32) is an INPUT: the reference takes a_eh = exp(s_eh - m_ih) / z_ih on it.  The recomputed fp32
             coefficient: the argument fl(s - m) is off by 2 u |s| + u |s - m|, expf 4 u, the division one:
                 alpha_e = (2 |s| + |s - m| + 5) u, relative.   g_e = fl(dout_e / H): one u.
             t_i = sum_row a g by fma:   dt_i = sum_row (alpha_e + 1 u) |a g| + (n_l + log2 L) u sum_row |a g|.
             dpre = fl(fl(a fl(g - t)) s'): the difference carries u |g| + dt and rounds, the products round once each:
                 ddpre_e = |s'| a (u |g| + dt_i) + (alpha_e + 3 u) |dpre_e| + FLT_MIN (1 + |g| + |t|).
             du_i = sum_row dpre:   sum_row ddpre + (n_l + log2 L) u sum_row |dpre|;
             dv_c = sum_col dpre:   sum_col ddpre + (n_c + log2 L) u sum_col |dpre|,  n_c = ceil(len_T(c) / L)
             (the column pass reads the fp32 t of the row pass and recomputes the same a).

The kink: pre = 0 takes the derivative `slope` (torch's leaky_relu).  The 'kink' case plants u_i = -v_j exactly on the
first entry of every third row; every input lies on a grid of 2^-12 (u) and 2^-12 + 2^-13 (v), so that u + v is exact in
fp32 and every other |pre| is at least MARGIN = 2^-13: `inputs` asserts it, and no rounding of the kernels can cross the
kink."""
import numpy as np

from tests import csr_edge_ops_cases as OC
from tests.csr_edge_ops_cases import FLT_MIN, U, Csr, _seed, col_len, moved, row_len      # noqa: F401  (re-exported)

THREADS = 256
MAX_HEADS = 8
HEADS = (1, 2, 3, 4, 8)
MARGIN = 2.0 ** -13
GRID = 4096.0
# the lengths of csr_edge_ops_cases.py and the register edges it lacks: 4 x 5 (+1) at H = 3, 64 x 2 at H = 8
PLANTED = OC.PLANTED + (20, 21, 128)
N_EDGE = OC.N_EDGE


def plan(n_rows, nnz, H, ldv, v_misaligned):
    """(lanes per row, floats per v load, entries per lane in registers, rows per workgroup, longest row read once) as
    dp_csr_gat_plan answers."""
    lanes = 4 if nnz <= 8 * n_rows else (16 if nnz <= 32 * n_rows else 64)
    vec = 4 if H % 4 == 0 and ldv % 4 == 0 and not v_misaligned else 1
    regs = min(8 if lanes == 4 else 4, 16 // H)
    return lanes, vec, regs, THREADS // lanes, lanes * regs


# ------------------------------------------------------------------ graphs
TIER_GRAPHS = tuple(f"t{lanes}-n{n}" for lanes in (4, 16, 64) for n in (N_EDGE, N_EDGE + 1))
GRAPHS = TIER_GRAPHS + ("undirected", "batch")
_GRAPHS = {}


def graph(name):
    """The case graph with its transposed CSR (indptr_t, indices_t, rows_t), `mirror` and `lanes`."""
    if name not in _GRAPHS:
        if name in TIER_GRAPHS:
            lanes, n = int(name[1:name.index("-")]), int(name[name.index("n") + 1:])
            seed = 10 + lanes + n
            rng = np.random.default_rng(seed)
            fill = rng.integers(*OC.FILLER[lanes], n)
            g = Csr(n, *OC._ringed_rows(n, lambda r: PLANTED[r] if r < len(PLANTED) else int(fill[r]), rng, (3, 11, 40)),
                    seed, True)
            g.indptr_t, g.indices_t, g.mirror = OC._transposed(g)
            g.rows_t = np.repeat(np.arange(g.n), np.diff(g.indptr_t.astype(np.int64)))
            g.lanes = plan(g.n, g.nnz, 1, 1, 0)[0]
        else:
            g = OC.graph(name)
        _GRAPHS[name] = g
    return _GRAPHS[name]


def _per_lane(length, lanes):
    return -(-length // lanes)


# ------------------------------------------------------------------ the table
# layout: (ld of H, base one float off the 16-byte grid)
LAYOUTS = {"tight": (lambda H: H, 0), "pad4": (lambda H: 4 * (H // 4 + 1), 0),
           "odd": (lambda H: H + 1 if H % 2 == 0 else H + 2, 0), "mis": (lambda H: 4 * (H // 4 + 1), 1)}
KINDS = ("ordinary", "ties", "equal", "shift80", "below200", "kink")
SLOPES = (0.2, 1.0, 0.0)


def _table():
    cases, lay = [], list(LAYOUTS)
    for gi, gname in enumerate(GRAPHS):                    # every graph at every H, the layouts in turn
        for hi, H in enumerate(HEADS):
            cases.append((gname, H, lay[(gi + hi) % 4], "ordinary", 0.2))
    for gname in ("t4-n576", "t64-n577"):                  # H = 4, 8 in every layout: both load forms
        for H in (4, 8):
            for layout in lay:
                cases.append((gname, H, layout, "ordinary", 0.2))
    for kind in KINDS[1:]:                                 # the other inputs
        for gname, layout in (("t4-n577", "odd"), ("t64-n576", "pad4"), ("batch", "tight")):
            for H in (2, 8):
                cases.append((gname, H, layout, kind, 0.2))
    for H in HEADS:                                        # exact 2^-k at every H
        cases.append(("t16-n576", H, "tight", "equal", 0.2))
    for slope in SLOPES[1:]:                               # slope 1 (u_i cancels), slope 0 (whole rows may tie)
        for gname, layout in (("t4-n576", "mis"), ("t16-n577", "pad4"), ("undirected", "odd")):
            for H in (1, 4):
                cases.append((gname, H, layout, "ordinary", slope))
        cases.append(("batch", 3, "pad4", "kink", slope))
        cases.append(("t16-n576", 8, "tight", "ties", slope))
    cases.append(("t4-n576", 4, "tight", "below200", 1.0))
    return list(dict.fromkeys(cases))


CASES = _table()


def case_id(case):
    return "-".join(str(c) for c in case)


def layout_of(case):
    """(ld, off) of the case's u and v buffers."""
    ld, off = LAYOUTS[case[2]]
    return ld(case[1]), off


def case_plan(case):
    g = graph(case[0])
    ld, off = layout_of(case)
    return plan(g.n, g.nnz, case[1], ld, off)


def _grid(rng, shape, half):
    return ((np.rint(rng.uniform(-3.0, 3.0, shape) * GRID) + (0.5 if half else 0.0)) / GRID).astype(np.float32)


def inputs(case):
    """(u, v) fp32 [n, H].  ordinary: the grids of the docstring in (-3, 3); ties: four and three values; equal: v_jh one
    value per head (rows of 2^k entries give exactly 2^-k); shift80: u plus 80 on even rows and on rows of 64 entries and
    more, minus 80 on the others; below200: every fifth node's v lowered by 210 / slope (its entries lie 200 below the
    row's maximum and more); kink: u_i = -v_j on the first entry of every third row."""
    gname, H, _, kind, slope = case
    g = graph(gname)
    rng = np.random.default_rng(_seed("gat-" + case_id(case)))
    u, v = _grid(rng, (g.n, H), False), _grid(rng, (g.n, H), True)
    if kind == "ties":
        u = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=np.float32), (g.n, H))
        v = rng.choice(np.array([-0.75, 0.25, 1.75], dtype=np.float32), (g.n, H))
    elif kind == "equal":
        v = np.broadcast_to(v[:1], (g.n, H)).copy()
    elif kind == "shift80":
        up = (np.arange(g.n) % 2 == 0) | (row_len(g) >= 64)
        u = (u + np.where(up, 80.0, -80.0).astype(np.float32)[:, None]).astype(np.float32)
    elif kind == "below200":
        assert slope > 0
        v[3::5] -= np.float32(210.0 / slope)
    elif kind == "kink":
        rows = np.arange(0, g.n, 3)
        rows = rows[row_len(g)[rows] > 0]
        u[rows] = -v[g.indices[g.indptr[rows]]]
    pre = u.astype(np.float64)[g.rows] + v.astype(np.float64)[g.indices]
    assert np.array_equal(pre, (u[g.rows] + v[g.indices]).astype(np.float64))      # exact in fp32
    zero = pre == 0
    assert (np.abs(pre[~zero]) >= MARGIN).all() and zero.any() == (kind == "kink"), case_id(case)
    return u, v


def padded(x, ld, fill=np.nan):
    """[n, H] inside [n, ld]: what the kernels read at leading dimension ld."""
    out = np.full((x.shape[0], ld), fill, dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def _seg_sum(idx, x, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, idx, x)
    return out


def _scores(g, u, v, slope, positive_side=False, no_slope=False):
    pre = np.asarray(u, np.float64)[g.rows] + np.asarray(v, np.float64)[g.indices]
    sl = float(np.float32(slope))
    if no_slope:
        return pre, pre
    return pre, np.where(pre > 0, sl * pre, pre) if positive_side else np.where(pre > 0, pre, sl * pre)


# ------------------------------------------------------------------ forward
def fwd_ref(g, u, v, slope, lanes=None, mean=True, positive_side=False, no_slope=False, drop_last=False):
    """(out, bound, rowstat [n, 2H], rowstat bound).  mean / positive_side / no_slope / drop_last are a faulty kernel's:
    the 1 / H missing, the slope applied to the positive side, no slope at all, the last entry of every row left out of
    the row's maximum and sum."""
    lanes = g.lanes if lanes is None else lanes
    H = u.shape[1]
    _, s = _scores(g, u, v, slope, positive_side, no_slope)
    live = np.ones(g.nnz, dtype=bool)
    if drop_last:
        live[g.indptr[1:][row_len(g) > 0] - 1] = False
    m, lo, big = np.full((g.n, H), -np.inf), np.full((g.n, H), np.inf), np.zeros((g.n, H))
    np.maximum.at(m, g.rows[live], s[live])
    np.minimum.at(lo, g.rows[live], s[live])
    np.maximum.at(big, g.rows, np.abs(s))
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(live[:, None], np.exp(s - m[g.rows]), 0.0)
        z = _seg_sum(g.rows, e, g.n)
        a = e / z[g.rows]
        out = a.sum(1) / (H if mean else 1)
        n_l = _per_lane(row_len(g), lanes)[:, None]
        base = 6 * n_l + 3 * (m - lo) + np.log2(lanes) + 14 + 4 * big                  # per row and head
        rho = (base[g.rows] + np.abs(s - m[g.rows])) * U
        bound = (rho * a).sum(1) / H + (H + 1) * U * out + 2 * FLT_MIN
        empty = (row_len(g) == 0)[:, None]
        stat = np.where(empty, 0.0, np.concatenate([m, z], axis=1))
        sbound = np.where(empty, FLT_MIN, np.concatenate([2 * U * big, base * U * z], axis=1) + FLT_MIN)
    return out, bound, stat, sbound


# ------------------------------------------------------------------ backward
def bwd_inputs(case):
    """(rowstat fp32 — the rounding of the fp64 one —, dout U(-1, 1))."""
    g = graph(case[0])
    u, v = inputs(case)
    stat = fwd_ref(g, u, v, case[4])[2].astype(np.float32)
    rng = np.random.default_rng(_seed("gat-bwd-" + case_id(case)))
    return stat, rng.uniform(-1.0, 1.0, g.nnz).astype(np.float32)


def bwd_ref(g, u, v, stat, dout, slope, lanes=None, mean=True, kink_one=False, drop_last=False, minus_t=True,
            own_stats=False, mirror=True):
    """(du, du bound, dv, dv bound, t, t bound) on the fp32 rowstat.  The keyword arguments are a faulty kernel's: g
    without 1 / H, derivative 1 at the kink, the last entry of every row left out of t, `- t` omitted, dv with the
    column's own rowstat and t, dout[k] read for dout[mirror[k]] in the column pass."""
    lanes = g.lanes if lanes is None else lanes
    H = u.shape[1]
    sl = float(np.float32(slope))
    pre, s = _scores(g, u, v, slope)
    stat = np.asarray(stat, np.float64)
    m, z = stat[:, :H], stat[:, H:]
    ge = (np.asarray(dout, np.float64) / (H if mean else 1))[:, None]
    d = np.where((pre >= 0) if kink_one else (pre > 0), 1.0, sl)
    live = np.ones((g.nnz, 1))
    if drop_last:
        live[g.indptr[1:][row_len(g) > 0] - 1] = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = np.exp(s - m[g.rows]) / z[g.rows]
        t = _seg_sum(g.rows, a * ge * live, g.n)
        T = _seg_sum(g.rows, np.abs(a * ge), g.n)
        dpre = a * (ge - (t[g.rows] if minus_t else 0.0)) * d
        du = _seg_sum(g.rows, dpre, g.n)
        cols = g.indices.astype(np.int64)
        if own_stats:                       # a_(r,c) from the column's own m, z and t
            dcol = np.exp(s - m[cols]) / z[cols] * (ge - t[cols]) * d
        elif not mirror:                    # entry k of the transposed CSR reads dout[k]
            gk = np.empty_like(ge)
            gk[g.mirror] = ge               # stored entry mirror[k] takes dout[k]
            dcol = a * (gk - t[g.rows]) * d
        else:
            dcol = dpre
        dv = _seg_sum(cols, np.where(np.isfinite(dcol), dcol, 0.0) if own_stats else dcol, g.n)
        alpha = (2 * np.abs(s) + np.abs(s - m[g.rows]) + 5) * U
        tree = np.log2(lanes)
        n_l = _per_lane(row_len(g), lanes)[:, None]
        n_c = _per_lane(col_len(g), lanes)[:, None]
        dt = _seg_sum(g.rows, (alpha + U) * np.abs(a * ge), g.n) + (n_l + tree) * U * T
        ddpre = np.abs(d) * a * (U * np.abs(ge) + dt[g.rows]) + (alpha + 3 * U) * np.abs(dpre) + FLT_MIN * (
            1 + np.abs(ge) + np.abs(t[g.rows]))
        dub = _seg_sum(g.rows, ddpre, g.n) + (n_l + tree) * U * _seg_sum(g.rows, np.abs(dpre), g.n) + FLT_MIN
        dvb = _seg_sum(cols, ddpre, g.n) + (n_c + tree) * U * _seg_sum(cols, np.abs(dpre), g.n) + FLT_MIN
    return du, dub, dv, dvb, t, dt + FLT_MIN


# ------------------------------------------------------------------ the kernels' order in fp32 (numpy)
def _place(indptr, n, lanes):
    """(row, lane, slot) of every entry of a CSR in the kernels' order, and the slots per lane of the longest row."""
    lens = np.diff(indptr.astype(np.int64))
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(rows.size) - indptr.astype(np.int64)[rows]
    return rows, pos % lanes, pos // lanes, max(1, int(_per_lane(lens.max(initial=0), lanes)))


def _tree(x, op=np.add):
    while x.shape[1] > 1:
        x = op(x[:, 0::2], x[:, 1::2])
    return x[:, 0]


def _lane_sums(x, where, n, lanes, slots, fma_with=None):
    """Per row the kernels' sum of x [entries, H] (fp32): each lane its entries ascending, then the tree.  fma_with: the
    terms are x * fma_with fused into the running sum."""
    rows, lane, slot = where
    H = x.shape[1]
    arr = np.zeros((n, lanes, slots, H), dtype=np.float32)
    arr[rows, lane, slot] = x
    if fma_with is not None:
        garr = np.zeros((n, lanes, slots, 1), dtype=np.float32)
        garr[rows, lane, slot] = fma_with
    acc = np.zeros((n, lanes, H), dtype=np.float32)
    for k in range(slots):
        if fma_with is None:
            acc = acc + arr[:, :, k]
        else:
            acc = (arr[:, :, k].astype(np.float64) * garr[:, :, k] + acc).astype(np.float32)
    return _tree(acc)


def _scores32(g, u, v, slope):
    pre = u[g.rows] + v[g.indices]
    return pre, np.where(pre > 0, pre, np.float32(slope) * pre).astype(np.float32)


def emulate_fwd(g, u, v, slope, lanes, regs):
    """(out, rowstat) of k_gat_fwd in fp32 numpy, in the kernel's order: a row of at most lanes * regs entries through the
    registers, a longer one through the running maximum and sum."""
    H = u.shape[1]
    _, s = _scores32(g, u, v, slope)
    rows, lane, slot, slots = where = _place(g.indptr, g.n, lanes)
    arr = np.full((g.n, lanes, slots, H), -np.inf, dtype=np.float32)
    arr[rows, lane, slot] = s
    with np.errstate(invalid="ignore", over="ignore"):
        M = arr.max(axis=(1, 2))
        p = np.exp(s - M[g.rows]).astype(np.float32)
        S_reg = _lane_sums(p, where[:3], g.n, lanes, slots)
        m, acc = np.full((g.n, lanes, H), -np.inf, dtype=np.float32), np.zeros((g.n, lanes, H), dtype=np.float32)
        for k in range(slots):
            x = arr[:, :, k]
            ok = np.isfinite(x)
            mn = np.maximum(m, x)
            new = (acc * np.exp(m - mn) + np.exp(x - mn)).astype(np.float32)
            acc, m = np.where(ok, new, acc), np.where(ok, mn, m)
        S_str = _tree((acc * np.exp(m - M[:, None])).astype(np.float32))
        fits = (row_len(g) <= lanes * regs)[:, None]
        S = np.where(fits, S_reg, np.where(row_len(g)[:, None] > 0, S_str, 0)).astype(np.float32)
        a = (p / S[g.rows]).astype(np.float32)
    out = a[:, 0]
    for h in range(1, H):
        out = out + a[:, h]
    empty = (row_len(g) == 0)[:, None]
    return (out / np.float32(H)).astype(np.float32), np.where(empty, 0, np.concatenate([M, S], axis=1)).astype(np.float32)


def emulate_bwd(g, u, v, stat, dout, slope, lanes):
    """(du, dv, t) of k_gat_bwd_rows / k_gat_bwd_cols in fp32 numpy, in the kernels' order."""
    H = u.shape[1]
    pre, s = _scores32(g, u, v, slope)
    m, z = stat[:, :H], stat[:, H:]
    where = _place(g.indptr, g.n, lanes)
    a = (np.exp(s - m[g.rows]) / z[g.rows]).astype(np.float32)
    ge = (dout / np.float32(H)).astype(np.float32)[:, None]
    t = _lane_sums(a, where[:3], g.n, lanes, where[3], fma_with=ge)
    d = np.where(pre > 0, np.float32(1), np.float32(slope)).astype(np.float32)
    dpre = ((a * (ge - t[g.rows])) * d).astype(np.float32)
    du = _lane_sums(dpre, where[:3], g.n, lanes, where[3])
    where_t = _place(g.indptr_t, g.n, lanes)
    dv = _lane_sums(dpre[g.mirror], where_t[:3], g.n, lanes, where_t[3])
    return du, dv, t
