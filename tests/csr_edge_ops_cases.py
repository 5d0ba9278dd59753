"""Case table, fp64 references and derived error bounds of the learned-edge-weight entries (dp_csr_edge_softmax_fwd / _bwd,
dp_csr_sym_norm_fwd / _bwd; dp_csr_edge_plan restated), shared by tests/test_csr_edge_ops_cpu.py (which shows that these
inputs tell a bug from rounding) and tests/test_gpu_csr_edge_ops.py.

Every reference is float64 on the fp32 inputs.  Bounds are rounding counts times the magnitudes they act on, u = 2^-24,
first order, counted from the kernels' arithmetic (dp_csr_edge_ops.hip).  A row of `len` entries is served by L lanes
(the plan's first int); a lane sums its n_l = ceil(len / L) entries in ascending order (n_l roundings, each below u times
the sum of the absolute terms), then a DPP tree of log2 L levels adds one rounding each: a segmented sum of terms t
carries at most (n_l + log2 L) u sum |t|.  expf and logf are budgeted at 4 u of their value (the budget of
tests/csr_weights_cases.py), on top of the error of their argument: fl(x - M) is off by u |x - M|, which exp turns into
the same RELATIVE error.  sqrt and the division are correctly rounded (one u each).

  softmax fwd   out_e = exp(x_e - M) / S.  D = max - min of the row.
                In registers (len <= L R): p_e = expf(fl(x_e - M)) carries (|x_e - M| + 4) u; S sums at most R terms per
                lane and the tree, every term within (D + 4) u: (D + 4 + R + log2 L) u; the quotient rounds once:
                (|x_e - M| + D + R + log2 L + 9) u.
                Streaming (len > L R): per step sum <- sum * expf(m - m') + expf(x - m').  What is already in the sum takes
                (|m - m'| + 4) u from the factor, one u from the product, one from the addition; over the lane's n_l steps
                the |m - m'| telescope to at most D: (6 n_l + D) u.  A new term enters within (D + 4) u.  The lane's sum
                is moved to the row maximum by expf(m_l - M): (D + 4 + 1) u; the tree: log2 L u; p_e and the quotient as
                above: (6 n_l + 3 D + |x_e - M| + log2 L + 14) u.
                The streaming count covers the register one (n_l >= 1, R <= 8), so ONE bound serves every row:
                    |err| <= (6 n_l + 3 D + |x_e - M| + log2 L + 14) u out_e + FLT_MIN,
                the floor of one smallest normal because a result below it may be flushed to zero.
  softmax bwd   ds_e = a_e (g_e - dot), dot = sum_row a g by fma: (n_l + log2 L) u T, T = sum_row |a g|; the difference
                and the product round once each:
                    |err| <= (n_l + log2 L) u |a_e| T + 3 u |ds_e| + FLT_MIN      (2 u |ds_e| and one u of second order).
  sym norm fwd  d_c sums positive terms: relative (n_c + log2 L) u, n_c = ceil(len_T(c) / L) over the transposed row; a
                0/1 container counts exactly.  r_c = 1 / sqrt(d_c): half of that plus the two roundings:
                rho_c = (n_c + log2 L) / 2 + 2.   out_e = v_e (r_i r_j), two products:
                    |rdeg err| <= rho_c u r_c,        |err| <= (rho_i + rho_j + 2) u |out_e|.
  sym norm bwd  the fp32 rdeg is an INPUT (the reference is taken on it).  t_c sums (g v) r terms, two roundings each, over
                the row and the transposed row of c: n_t = ceil(len(c) / L) + ceil(len_T(c) / L) additions per lane and the
                tree: (n_t + log2 L + 2) u T_c, T_c = sum |g v r|.  G_c = -1/2 (r r r) t: three roundings:
                    |gdeg err| <= 1/2 r_c^3 (n_t + log2 L + 2) u T_c + 3 u |G_c|;
                dv_e = fl(fl(g_e fl(r_i r_j)) + G_j): two roundings on the product, one on the sum:
                    |err| <= 2 u |g_e r_i r_j| + |gdeg err|_j + u |dv_e|.
"""
import numpy as np

from tests.csr_edge_grad_cases import BATCH_SIZES, U, Csr, _seed, moved      # noqa: F401  (moved: re-exported)

FLT_MIN = float(np.finfo(np.float32).tiny)
THREADS = 256
# stored entries of rows 0 .. of the planted graphs: the issue's lengths, and every tier's register edge (L R, L R + 1)
PLANTED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65, 129, 256, 257, 530)
HUB_ROW = PLANTED.index(530)
N_EDGE = 576                       # a multiple of every tier's rows per workgroup (64, 16, 4); N_EDGE + 1 is one past it
FILLER = {4: (1, 8), 16: (10, 31), 64: (40, 61)}      # the other rows' lengths [lo, hi): they set the mean, so the tier
N_UND = 200


def plan(n_rows, nnz):
    """(lanes per row, entries a lane keeps in registers, rows per workgroup, longest row read once) as dp_csr_edge_plan
    answers."""
    lanes = 4 if nnz <= 8 * n_rows else (16 if nnz <= 32 * n_rows else 64)
    regs = 8 if lanes == 4 else 4
    return lanes, regs, THREADS // lanes, lanes * regs


# ------------------------------------------------------------------ graphs
def _ringed_rows(n, length_of, rng, self_loops=()):
    """Directed: row r holds length_of(r) entries, of which one is the ring r -> r + 1 (so every column has an entry
    wherever the row before it has one); rows in `self_loops` keep (r, r)."""
    src, dst = [], []
    for r in range(n):
        d = length_of(r)
        if d == 0:
            continue
        ring = (r + 1) % n
        if d == PLANTED[HUB_ROW]:
            cols = np.arange(d)                                    # columns 0 .. 529: also column 1, which row 0 leaves out
            if ring not in cols:
                cols[-1] = ring
        else:
            others = np.setdiff1d(np.arange(n), [ring, r])
            cols = np.concatenate([[ring], rng.choice(others, d - 1, replace=False)])
            if r in self_loops and d >= 2:
                cols[1] = r
        src.append(np.full(d, r))
        dst.append(cols)
    return np.concatenate(src), np.concatenate(dst)


def _tier_graph(lanes, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = FILLER[lanes]
    fill = rng.integers(lo, hi, n)
    return Csr(n, *_ringed_rows(n, lambda r: PLANTED[r] if r < len(PLANTED) else int(fill[r]), rng, (3, 11, 40)), seed,
               True)


def _undirected(n, seed):
    """Symmetric pattern: a ring both ways, random pairs, two self loops and a hub of 70 neighbours."""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    ring = np.arange(n)
    s, d = np.concatenate([s, ring, [5, 77], np.full(70, 9)]), np.concatenate(
        [d, (ring + 1) % n, [5, 77], rng.choice(n, 70, replace=False)])
    return np.concatenate([s, d]), np.concatenate([d, s])


def _batch(sizes, seed):
    """Block-diagonal directed CSR with GLOBAL columns, a ring under every graph (the one-node graph: a self loop)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for b, nb in enumerate(sizes):
        ring = np.arange(nb)
        s, d = rng.integers(0, nb, 3 * nb), rng.integers(0, nb, 3 * nb)
        s, d = np.concatenate([ring, s]), np.concatenate([(ring + 1) % nb, d])
        if nb == 64:
            s, d = np.concatenate([s, np.full(64, 7)]), np.concatenate([d, np.arange(64)])
        src.append(s + off[b])
        dst.append(d + off[b])
    return np.concatenate(src), np.concatenate(dst), off


def _transposed(g):
    """(indptr_t, indices_t, mirror): the CSR of A^T and, for its entry k, the stored entry mirror[k] of A."""
    order = np.lexsort((g.rows, g.indices)).astype(np.int32)
    indptr_t = np.zeros(g.n + 1, dtype=np.int64)
    np.add.at(indptr_t, g.indices.astype(np.int64) + 1, 1)
    return np.cumsum(indptr_t).astype(np.int32), g.rows[order].astype(np.int32), order


TIER_GRAPHS = tuple(f"t{lanes}-n{n}" for lanes in (4, 16, 64) for n in (N_EDGE, N_EDGE + 1))
GRAPHS = TIER_GRAPHS + ("undirected", "batch")
_GRAPHS = {}


def graph(name):
    """The case graph `name` with its transposed CSR (indptr_t, indices_t, rows_t), `mirror`, its `plan` and `lanes`."""
    if name not in _GRAPHS:
        if name in TIER_GRAPHS:
            lanes, n = int(name[1:name.index("-")]), int(name[name.index("n") + 1:])
            g = _tier_graph(lanes, n, 10 + lanes + n)
        elif name == "undirected":
            g = Csr(N_UND, *_undirected(N_UND, 5), 5, False)
        elif name == "batch":
            s, d, off = _batch(BATCH_SIZES, 6)
            g = Csr(int(off[-1]), s, d, 6, True, off=off.astype(np.int32))
        else:
            raise KeyError(name)
        g.indptr_t, g.indices_t, g.mirror = _transposed(g)
        g.rows_t = np.repeat(np.arange(g.n), np.diff(g.indptr_t.astype(np.int64)))
        if not g.directed:                                   # a_ij = a_ji, bit for bit
            assert np.array_equal(g.indptr_t, g.indptr) and np.array_equal(g.indices_t, g.indices)
            g.values = (np.float32(0.5) * (g.values + g.values[g.mirror])).astype(np.float32)
        g.plan = plan(g.n, g.nnz)
        g.lanes = g.plan[0]
        col = np.zeros(g.n)
        np.add.at(col, g.indices, g.values.astype(np.float64))
        assert (col > 0).all(), f"{name}: a node without a positive column sum"
        _GRAPHS[name] = g
    return _GRAPHS[name]


def row_len(g):
    return np.diff(g.indptr.astype(np.int64))


def col_len(g):
    return np.diff(g.indptr_t.astype(np.int64))


def _per_lane(length, lanes):
    return -(-length // lanes)


# ------------------------------------------------------------------ softmax
SOFTMAX_KINDS = ("ordinary", "ties", "equal", "shift80", "below200")
SOFTMAX_CASES = [(gname, kind) for gname in GRAPHS for kind in SOFTMAX_KINDS]


def case_id(case):
    return "-".join(str(c) for c in case)


def softmax_inputs(case):
    """fp32 scores [nnz].  ordinary: U(-3, 3); ties: four values; equal: one value per row (a row of 2^k entries gives
    exactly 2^-k); shift80: U(-8.5, 8.5) plus 80 on even rows and on rows of 64 entries and more, minus 80 on the others
    (no single exp overflows fp32, but without the max subtraction the sum of a long row does); below200: ordinary with the second entry of every row 200 below the row's maximum."""
    gname, kind = case
    g = graph(gname)
    rng = np.random.default_rng(_seed(case_id(case)))
    if kind == "ties":
        s = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=np.float32), g.nnz)
    elif kind == "equal":
        s = rng.uniform(-3.0, 3.0, g.n).astype(np.float32)[g.rows]
    elif kind == "shift80":
        up = (g.rows % 2 == 0) | (row_len(g)[g.rows] >= 64)
        s = rng.uniform(-8.5, 8.5, g.nnz).astype(np.float32) + np.where(up, 80.0, -80.0).astype(np.float32)
    else:
        s = rng.uniform(-3.0, 3.0, g.nnz).astype(np.float32)
        if kind == "below200":
            m = np.full(g.n, -np.inf, dtype=np.float32)
            np.maximum.at(m, g.rows, s)
            second = g.indptr[:-1][row_len(g) >= 2] + 1
            low = (m[g.rows[second]] - np.float32(200.0)).astype(np.float32)
            keep = s[second] < m[g.rows[second]]                     # never the maximum itself
            s[second[keep]] = low[keep]
    return s.astype(np.float32)


def softmax_ref(g, s, rows=None, shift=True, drop_last=False, lanes=None):
    """(reference, bound) of dp_csr_edge_softmax_fwd.  rows / shift / drop_last are a faulty kernel's: the sum taken over
    another segmentation, no max subtraction (then in fp32, as the kernel would), the last entry of every row left out."""
    rows = g.rows if rows is None else rows
    lanes = g.lanes if lanes is None else lanes
    x = np.asarray(s, np.float64)
    live = np.ones(g.nnz, dtype=bool)
    if drop_last:
        live[g.indptr[1:][row_len(g) > 0] - 1] = False
    if not shift:
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(np.asarray(s, np.float32))
            tot = np.zeros(g.n, dtype=np.float32)
            np.add.at(tot, rows, e)
            return (e / tot[rows]).astype(np.float64), None
    m = np.full(g.n, -np.inf)
    np.maximum.at(m, rows[live], x[live])
    lo = np.full(g.n, np.inf)
    np.minimum.at(lo, rows[live], x[live])
    e = np.where(live, np.exp(x - m[rows]), 0.0)
    tot = np.zeros(g.n)
    np.add.at(tot, rows, e)
    out = e / tot[rows]
    n_l = _per_lane(row_len(g), lanes)[g.rows]
    d = (m - lo)[g.rows]
    bound = (6 * n_l + 3 * d + np.abs(x - m[g.rows]) + np.log2(lanes) + 14) * U * out + FLT_MIN
    return out, bound


SOFTMAX_BWD_CASES = [(gname, kind) for gname in GRAPHS for kind in ("ordinary", "zero-grad")]


def softmax_bwd_inputs(case):
    """(a, g): a the fp32 rounding of an fp64 softmax of ordinary scores (a one-entry row holds exactly 1), g the
    gradient — U(-1, 1), or all zero."""
    gname, kind = case
    gr = graph(gname)
    a, _ = softmax_ref(gr, softmax_inputs((gname, "ordinary")))
    rng = np.random.default_rng(_seed("bwd-" + case_id(case)))
    dout = rng.uniform(-1.0, 1.0, gr.nnz).astype(np.float32)
    return a.astype(np.float32), dout * np.float32(kind != "zero-grad")


def softmax_bwd_ref(g, a, dout, rows=None, drop_last=False):
    rows = g.rows if rows is None else rows
    a64, g64 = np.asarray(a, np.float64), np.asarray(dout, np.float64)
    live = np.ones(g.nnz)
    if drop_last:
        live[g.indptr[1:][row_len(g) > 0] - 1] = 0.0
    dot, mag = np.zeros(g.n), np.zeros(g.n)
    np.add.at(dot, rows, a64 * g64 * live)
    np.add.at(mag, rows, np.abs(a64 * g64))
    ds = a64 * (g64 - dot[rows])
    n_l = _per_lane(row_len(g), g.lanes)[g.rows]
    return ds, (n_l + np.log2(g.lanes)) * U * np.abs(a64) * mag[g.rows] + 3 * U * np.abs(ds) + FLT_MIN


# ------------------------------------------------------------------ D^-1/2 A D^-1/2
# (graph, stored values or a 0/1 container)
SYM_CASES = [(gname, w) for gname in GRAPHS for w in ("weighted", "01")]


def sym_values(case):
    g = graph(case[0])
    return g.values if case[1] == "weighted" else None


def _rho(g):
    return (_per_lane(col_len(g), g.lanes) + np.log2(g.lanes)) / 2.0 + 2.0


def sym_fwd_ref(g, values, degree="column", mirror=True):
    """(out, out bound, rdeg, rdeg bound).  degree='row' and mirror=False are a faulty kernel's: row sums taken for the
    column sums, the transposed row summed over values[k] instead of values[mirror[k]]."""
    v = np.ones(g.nnz) if values is None else np.asarray(values, np.float64)
    d = np.zeros(g.n)
    if degree == "row":
        np.add.at(d, g.rows, v)
    elif mirror:
        np.add.at(d, g.rows_t, v[g.mirror])
    else:
        np.add.at(d, g.rows_t, v)
    with np.errstate(divide="ignore", invalid="ignore"):          # a faulty degree may be 0
        r = 1.0 / np.sqrt(d)
        out = v * (r[g.rows] * r[g.indices])
    rho = _rho(g) if values is not None else np.full(g.n, 2.0)          # a 0/1 container counts its degree exactly
    return out, (rho[g.rows] + rho[g.indices] + 2) * U * np.abs(out), r, rho * U * r


def sym_bwd_inputs(case):
    """(values or None, rdeg fp32 — the rounding of the fp64 d^-1/2 —, dout U(-1, 1))."""
    g = graph(case[0])
    values = sym_values(case)
    r = sym_fwd_ref(g, values)[2].astype(np.float32)
    rng = np.random.default_rng(_seed("sym-bwd-" + case_id(case)))
    return values, r, rng.uniform(-1.0, 1.0, g.nnz).astype(np.float32)


def sym_bwd_ref(g, values, rdeg, dout, halves=(True, True), self_twice=True, g_at="column", factor=-0.5):
    """(dvalues, bound, gdeg, gdeg bound).  The keyword arguments are a faulty kernel's: one half of t_c missing, a self
    loop counted in the row half only, G read at the entry's row, the factor -1/2 left out."""
    v = np.ones(g.nnz) if values is None else np.asarray(values, np.float64)
    r, go = np.asarray(rdeg, np.float64), np.asarray(dout, np.float64)
    cols = g.indices.astype(np.int64)
    t, mag = np.zeros(g.n), np.zeros(g.n)
    row_term, col_term = go * v * r[cols], go * v * r[g.rows]
    if not self_twice:
        col_term = np.where(g.rows == cols, 0.0, col_term)
    if halves[0]:
        np.add.at(t, g.rows, row_term)
    if halves[1]:
        np.add.at(t, cols, col_term)
    np.add.at(mag, g.rows, np.abs(go * v * r[cols]))
    np.add.at(mag, cols, np.abs(go * v * r[g.rows]))
    has = (row_len(g) + col_len(g)) > 0
    G = np.where(has, factor * r ** 3 * t, 0.0)
    n_t = _per_lane(row_len(g), g.lanes) + _per_lane(col_len(g), g.lanes)
    eG = np.where(has, 0.5 * r ** 3 * (n_t + np.log2(g.lanes) + 2) * U * mag + 3 * U * np.abs(G), 0.0)
    at = cols if g_at == "column" else g.rows
    lead = go * r[g.rows] * r[cols]
    dv = lead + G[at]
    return dv, 2 * U * np.abs(lead) + eG[cols] + U * np.abs(dv), G, eG
