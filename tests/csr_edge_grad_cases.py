"""Case table, fp64 references and derived error bounds of the gradients to the stored values of a CSR adjacency
(dp_csr_sddmm, dp_csr_link_dvalues, dp_csr_pool_dvalues, dp_sparse_gcn_layer_bwd_dv), shared by
tests/test_csr_edge_grad_cpu.py (which shows that these inputs tell a bug from rounding) and
tests/test_gpu_csr_edge_grad.py.

Every reference is float64 on the fp32 inputs; every stored entry e = (i, j) is its own variable.  Bounds are rounding
counts times sums of absolute terms, u = 2^-24, first order, counted from the kernel's arithmetic:

  identity     out = beta out0 + (alpha d) t, t the fp32 dot over F columns: whatever the order, its error is below
               F u sum |P_if Q_jf|; alpha d rounds once, its product with t once, the fused beta term once:
               (F + 3) u (|alpha d| sum |P Q| + |beta out0|)                                       (the issue's bound).
  bce          r = log(1 - p + eps) - log(p + eps), p = min(t, 1).  t carries (K + 1) u m, m = sum |s_i s_j|; min does
               not grow it; 1 - p and + eps round once each, logf is good to 2 u of its value (4 u budgeted, as
               tests/csr_weights_cases.py does):  dq = ((K + 4) u m + 2 u) / (1 - p + eps) + 4 u |log(1 - p + eps)|,
               dp likewise with p + eps; the difference rounds once and the coefficient c = inv_norm dloss twice:
               |c| (dq + dp) + 3 u |c r|.  Where t > 1 in float64 AND fp32 the clamp makes p exact (dq, dp keep the 2 u
               and 4 u terms only).  Premise, asserted: no reference t within 1e-4 below 1 (first order would not hold).
  frobenius    r = 2 (a - t): the subtraction rounds once, the doubling is exact: |c| 2 ((K + 1) u m + 3 u |a - t|).
  pooling      P = S dA'_b on the fp32 matrix cores (exact products, K terms: (K + 8) u of the absolute terms, the
               budget of tests/csr_weights_cases.py), then the identity form over K columns: (2 K + 11) u
               (|S| |dA'_b|)_i . |s_j|.
  GraphConv    dax = dU W^T with the error e_dax of tests/csr_weights_cases.gcn_ref (restated here, as that function
               does not return dax), then the identity form over Fin columns: (Fin + 3) u |dax_i| . |x_j| + e_dax_i . |x_j|.
"""
import zlib

import numpy as np

from tests import csr_weights_cases as WC

U = 2.0 ** -24
EPS = 1e-7


def _seed(text):
    return zlib.crc32(text.encode())          # the same in every process (hash() is salted)


CHUNK, ROWS_PER_WG, REG_VISITS = 512, 4, 4
PLANTED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 129)      # stored entries of rows 0 .. 13 of the planted graphs
N = 200
N_LONG, LONG_ROW, LONG_LEN = 560, 14, 530                      # one row beyond the 512-entry chunk needs n > 512
BATCH_SIZES = [37, 1, 64, 98]


# ------------------------------------------------------------------ graphs: raw CSR (numpy) of every case
class Csr:
    """indptr / indices (int32), rows (the row of every stored entry), values (fp32), n; directed: a transposed CSR of
    its own; off: node offsets of a batch (None: one graph)."""

    def __init__(self, n, src, dst, seed, directed, off=None):
        key = np.unique(np.asarray(src, np.int64) * n + np.asarray(dst, np.int64))
        self.n, self.directed, self.off = n, directed, off
        self.rows, self.indices = (key // n).astype(np.int64), (key % n).astype(np.int32)
        self.indptr = np.zeros(n + 1, dtype=np.int32)
        np.add.at(self.indptr, self.rows + 1, 1)
        self.indptr = np.cumsum(self.indptr, dtype=np.int64).astype(np.int32)
        self.nnz = key.size
        self.values = np.random.default_rng(seed + 1000).uniform(0.1, 2.0, self.nnz).astype(np.float32)

    def graph_of_row(self):
        off = np.array([0, self.n]) if self.off is None else np.asarray(self.off)
        return np.searchsorted(off, np.arange(self.n), side="right") - 1


def _planted(n, lengths, seed, extra_rows=()):
    """Directed: row r holds lengths[r] entries for r < len(lengths), the others 0 .. 6; rows 3, 11 and 40 keep a self
    loop (where they hold an entry at all)."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for r in range(n):
        d = lengths[r] if r < len(lengths) else int(rng.integers(0, 7))
        d = dict(extra_rows).get(r, d)
        cols = rng.choice(n, d, replace=False)
        if d and r in (3, 11, 40) and r not in cols:
            cols[0] = r
        src.append(np.full(d, r))
        dst.append(cols)
    return np.concatenate(src), np.concatenate(dst)


def _undirected(n, seed):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    s, d = np.concatenate([s, [5, 77]]), np.concatenate([d, [5, 77]])      # two self loops
    hub = rng.choice(n, 70, replace=False)                                  # one row above 64 entries
    s, d = np.concatenate([s, np.full(70, 9)]), np.concatenate([d, hub])
    return np.concatenate([s, d]), np.concatenate([d, s])


def _batch(sizes, seed):
    """Block-diagonal directed CSR with GLOBAL columns; graph 2 has a row of 64 entries (one full sub-chunk of column ids) and the stored entries of no graph end on a multiple of 64."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for b, nb in enumerate(sizes):
        if nb == 1:
            s, d = np.zeros(1, np.int64), np.zeros(1, np.int64)             # the one-node graph: a self loop
        else:
            s, d = rng.integers(0, nb, 4 * nb), rng.integers(0, nb, 4 * nb)
        if nb == 64:
            s, d = np.concatenate([s, np.full(64, 7)]), np.concatenate([d, np.arange(64)])
        src.append(s + off[b])
        dst.append(d + off[b])
    return np.concatenate(src), np.concatenate(dst), off


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        if name == "planted":
            _GRAPHS[name] = Csr(N, *_planted(N, PLANTED, 3), 3, True)
        elif name == "long":
            _GRAPHS[name] = Csr(N_LONG, *_planted(N_LONG, (), 4, {LONG_ROW: LONG_LEN, 15: 0, 16: 70}), 4, True)
        elif name == "undirected":
            _GRAPHS[name] = Csr(N, *_undirected(N, 5), 5, False)
        elif name == "batch":
            s, d, off = _batch(BATCH_SIZES, 6)
            _GRAPHS[name] = Csr(int(off[-1]), s, d, 6, True, off=off.astype(np.int32))
        else:
            raise KeyError(name)
    return _GRAPHS[name]


GRAPHS = ("planted", "long", "undirected", "batch")


# ------------------------------------------------------------------ the launch plan, restated
def plan(F, ldp, ldq, p_mis, q_mis):
    """(lanes, floats per lane, register-held visits, column tail, chunk, rows per workgroup) as dp_csr_sddmm_plan answers."""
    vec = 4 if F % 4 == 0 and ldp % 4 == 0 and ldq % 4 == 0 and not p_mis and not q_mis else 1
    lanes = 4 if F <= 4 * vec else (16 if F <= 16 * vec else 64)
    visits = -(-F // (lanes * vec))
    return (lanes, vec, min(visits, REG_VISITS) if lanes == 64 else 1, int(lanes == 64 and visits > REG_VISITS), CHUNK,
            ROWS_PER_WG)


# ------------------------------------------------------------------ the identity form
# (graph, F, ldp - F, ldq - F, bases one float off their allocation, beta, dscale or None)
FS = (1, 3, 4, 5, 16, 17, 64, 65, 256, 260, 1100)
SDDMM_CASES = (
    [("planted", F, 0, 0, False, 0.0, None) for F in FS]
    + [("planted", F, 4, 8, False, 1.0, 1.5) for F in (4, 16, 64, 256, 260, 1100)]          # padded, still 16-byte lanes
    + [("planted", F, 0, 0, True, 0.0, -0.5) for F in (4, 16, 64, 256, 260)]                 # misaligned: 4-byte lanes
    + [("planted", F, 1, 3, False, 1.0, None) for F in (4, 64)]                              # odd leading dimensions
    + [("planted", 130, 0, 0, False, 0.0, None), ("planted", 520, 0, 4, False, 1.0, None)]   # three visits in registers
    + [("long", F, 0, 0, False, 1.0, 2.0) for F in (4, 5, 64, 65)]
    + [("undirected", 17, 3, 0, False, 0.0, None), ("undirected", 16, 0, 0, False, 1.0, None),
       ("batch", 16, 0, 4, False, 0.0, 0.25), ("batch", 3, 0, 0, False, 1.0, None)])
ALPHA = 0.75


def sddmm_id(case):
    g, F, pp, pq, mis, beta, d = case
    return f"{g}-F{F}-ld+{pp}+{pq}{'-off1' if mis else ''}-beta{beta:g}{'' if d is None else f'-d{d:g}'}"


def sddmm_inputs(case, grid=False):
    """P, Q [n, F], out0 [nnz] fp32.  grid: small integers (every product and sum exact in fp32)."""
    g, F = graph(case[0]), case[1]
    rng = np.random.default_rng(_seed(sddmm_id(case)))
    if grid:
        draw = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
    else:
        draw = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)
    return draw(g.n, F), draw(g.n, F), draw(g.nnz)


def sddmm_ref(g, P, Q, out0, alpha, d, beta, rows=None, cols=None, F=None):
    """(reference, bound) of the identity form.  rows / cols / F: what a faulty kernel would read instead."""
    rows = g.rows if rows is None else rows
    cols = g.indices.astype(np.int64) if cols is None else cols
    P, Q = np.asarray(P, np.float64)[:, :F], np.asarray(Q, np.float64)[:, :F]
    c = alpha * (1.0 if d is None else d)
    dot = np.einsum("ef,ef->e", P[rows], Q[cols])
    mag = np.einsum("ef,ef->e", np.abs(P[rows]), np.abs(Q[cols]))
    old = beta * np.asarray(out0, np.float64)
    return old + c * dot, (P.shape[1] + 3) * U * (abs(c) * mag + np.abs(old))


# ------------------------------------------------------------------ the two link epilogues
LINK_K = (1, 4, 7, 16, 50, 64, 256)
LINK_CASES = ([("planted", K, obj, False) for K in LINK_K for obj in (0, 1)]
              + [(gname, K, obj, False) for gname in ("long", "undirected", "batch") for K in (7, 64) for obj in (0, 1)]
              + [("planted", 7, 0, True), ("undirected", 4, 0, True)])      # rows scaled so that some s_i . s_j > 1
DLOSS = 0.625


def link_id(case):
    g, K, obj, over = case
    return f"{g}-K{K}-{'frob' if obj else 'bce'}{'-over1' if over else ''}"


def link_inputs(case):
    g, K, obj, over = case
    rng = np.random.default_rng(_seed(link_id(case)))
    S = WC.assign_rows(rng, graph(g).n, K)
    return (S * np.float32(1.6)) if over else S


def inv_norm(g):
    off = np.array([0, g.n]) if g.off is None else np.asarray(g.off, np.int64)
    return 1.0 / float((np.diff(off) ** 2).sum())


def link_ref(g, S, obj, dloss, values=None, rows=None, cols=None, clamp=True, factor=2.0):
    """(reference, bound) of dp_csr_link_dvalues; the keyword arguments are a faulty kernel's."""
    rows = g.rows if rows is None else rows
    cols = g.indices.astype(np.int64) if cols is None else cols
    S64 = np.asarray(S, np.float64)
    K = S64.shape[1]
    t = np.einsum("ef,ef->e", S64[rows], S64[cols])
    m = np.einsum("ef,ef->e", np.abs(S64[rows]), np.abs(S64[cols]))
    c = inv_norm(g) * dloss
    if obj == 1:
        a = np.ones(g.nnz) if values is None else np.asarray(values, np.float64)
        return c * factor * (a - t), abs(c) * 2.0 * ((K + 1) * U * m + 3 * U * np.abs(a - t))
    assert not ((t < 1.0) & (t > 1.0 - 1e-4)).any(), "a reference p sits just below the clamp: replace the case"
    p = np.minimum(t, 1.0) if clamp else t
    with np.errstate(invalid="ignore", divide="ignore"):
        lq, lp = np.log(1.0 - p + EPS), np.log(p + EPS)
    dt = np.where(t > 1.0, 0.0, (K + 4) * U * m)                  # clamped in both precisions: p = 1 exactly
    dq = (dt + 2 * U) / np.abs(1.0 - p + EPS) + 4 * U * np.abs(lq)
    dp_ = (dt + 2 * U) / (p + EPS) + 4 * U * np.abs(lp)
    r = lq - lp
    return c * r, abs(c) * (dq + dp_) + 3 * U * np.abs(c * r)


# ------------------------------------------------------------------ pooling
POOL_CASES = [("planted", 1), ("planted", 4), ("planted", 5), ("planted", 20), ("planted", 64), ("planted", 256),
              ("long", 20), ("undirected", 17), ("batch", 4), ("batch", 20), ("batch", 65)]


def pool_id(case):
    return f"{case[0]}-K{case[1]}"


def pool_inputs(case):
    g, K = graph(case[0]), case[1]
    rng = np.random.default_rng(_seed(pool_id(case)))
    B = 1 if g.off is None else len(g.off) - 1
    return WC.softmax_rows(rng, g.n, K), rng.standard_normal((B, K, K)).astype(np.float32)


def pool_ref(g, S, dAp, graph_of_row=None, rows=None, cols=None):
    rows = g.rows if rows is None else rows
    cols = g.indices.astype(np.int64) if cols is None else cols
    gr = g.graph_of_row() if graph_of_row is None else graph_of_row
    S64, d64 = np.asarray(S, np.float64), np.asarray(dAp, np.float64)
    K = S64.shape[1]
    P = np.einsum("nk,nkl->nl", S64, d64[gr])
    Pm = np.einsum("nk,nkl->nl", np.abs(S64), np.abs(d64[gr]))
    return (np.einsum("ef,ef->e", P[rows], S64[cols]),
            (2 * K + 11) * U * np.einsum("ef,ef->e", Pm[rows], np.abs(S64[cols])))


# ------------------------------------------------------------------ GraphConv
# (graph, Fin, Fout, flags: 1 add_self | 2 normalize, dx wanted)
GCN_CASES = [("planted", 3, 5, 2, True), ("planted", 4, 8, 3, True), ("planted", 17, 20, 2, False),
             ("planted", 64, 16, 0, True), ("planted", 300, 12, 2, True), ("long", 9, 20, 3, True),
             ("undirected", 16, 7, 2, True), ("batch", 65, 9, 2, True)]


def gcn_id(case):
    return f"{case[0]}-Fin{case[1]}-Fout{case[2]}-flags{case[3]}{'' if case[4] else '-nodx'}"


def gcn_inputs(case):
    g, fin, fout = graph(case[0]), case[1], case[2]
    rng = np.random.default_rng(_seed(gcn_id(case)))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(g.n, fin), f(fin, fout) / np.float32(np.sqrt(fin)), f(fout) * np.float32(0.3), f(g.n, fout)


def dense_of(g, values=None):
    a = np.zeros((g.n, g.n))
    a[g.rows, g.indices] = g.values if values is None else values
    return a


def gcn_ref(g, x, W, b, dy, flags, rows=None, cols=None):
    """(dvalues reference, bound): the forward and dU / dax of tests/csr_weights_cases.gcn_ref with their errors."""
    a = dense_of(g)
    deg = np.diff(g.indptr.astype(np.int64))
    x, W, b, dy = (np.asarray(t, np.float64) for t in (x, W, b, dy))
    fin, fout = W.shape
    add_self, normalize = bool(flags & 1), bool(flags & 2)
    ax = a @ x + (x if add_self else 0.0)
    e_ax = (deg[:, None] + 3) * U * (np.abs(a) @ np.abs(x) + (np.abs(x) if add_self else 0.0))
    z = ax @ W + b
    e_z = (fin + 3) * U * (np.abs(ax) @ np.abs(W) + np.abs(b)) + e_ax @ np.abs(W)
    if normalize:
        inv = 1.0 / np.maximum(np.sqrt((z * z).sum(axis=1, keepdims=True)), 1e-12)
        y = z * inv
        rel = (fout + 6) * U + np.sqrt((e_z * e_z).sum(axis=1, keepdims=True)) * inv
        e_y = e_z * inv + np.abs(y) * rel + 2 * U * np.abs(y)
        ydy = (y * dy).sum(axis=1, keepdims=True)
        dU = inv * (dy - y * ydy)
        m_dU = inv * (np.abs(dy) + np.abs(y) * (np.abs(y) * np.abs(dy)).sum(axis=1, keepdims=True))
        e_ydy = (fout + 2) * U * (np.abs(y) * np.abs(dy)).sum(axis=1, keepdims=True) \
            + (e_y * np.abs(dy)).sum(axis=1, keepdims=True)
        e_dU = (6 * U + rel) * m_dU + inv * (e_y * np.abs(ydy) + np.abs(y) * e_ydy)
    else:
        dU, e_dU = dy, np.zeros_like(dy)
    dax = dU @ W.T
    e_dax = (fout + 3) * U * (np.abs(dU) @ np.abs(W).T) + e_dU @ np.abs(W).T
    rows = g.rows if rows is None else rows
    cols = g.indices.astype(np.int64) if cols is None else cols
    ref = np.einsum("ef,ef->e", dax[rows], x[cols])
    bound = (fin + 3) * U * np.einsum("ef,ef->e", np.abs(dax[rows]), np.abs(x[cols])) \
        + np.einsum("ef,ef->e", e_dax[rows], np.abs(x[cols]))
    return ref, bound


def moved(ref, other, bound):
    """Largest |other - ref| / bound over the entries (NaN / inf in `other` counts as moved without limit)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(np.asarray(other) - ref) / bound
    return float(np.nanmax(np.where(np.isfinite(other), d, np.inf))) if d.size else 0.0
