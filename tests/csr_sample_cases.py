"""Case table, numpy restatement, fp64 references and derived error bounds of the fused sampled neighbour mean
(dp_csr_sample_mean_fwd / _bwd, dp_csr_sample_mean_plan restated), shared by tests/test_csr_sample_cpu.py
(which shows that these inputs tell a bug from rounding), tests/test_gpu_csr_sample.py and
tests/test_gpu_csr_sample_model.py.

The restatement: `philox4x32_10` (ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
0xBB67AE85), key(i, j) = (word 0 at key (seed lo, seed hi), counter (i, j, 0, 0)) << 32 | j, and per target row the
threshold thr_i (the k-th smallest key; all-ones when the row has at most k entries or k is ALL), the sampled set
{j : key <= thr_i}, and cnt_i (|S|, or |S u {i}| under gcn).  `Sample.weights()` is the dense [m, n] matrix W with
W[r, j] = [j in S(i) or (gcn and j == i)] / cnt_i (a zero row where cnt_i == 0), so that

    mean = W x,     y = mean (none, gcn)  or  [x[nodes] | mean] (concat)
    dx   = W^T dy_mean  (+ dy[:, :F] scattered to the target nodes under concat)

Every reference is float64 on the fp32 inputs.  The bounds are counted from the kernels' arithmetic
(dp_csr_sample.hip), u = 2^-24, gamma(n) = n u / (1 - n u):

  forward   four partial sums (entry q of a batch of 64 ids into partial q % 4 while four whole entries remain, the
            rest and gcn's self row into partial 0), (s0 + s1) + (s2 + s3), then the scale: a term passes at most
            n_f = ceil(cnt / 4) + 3 ceil(cnt / 64) + 2 roundings, plus one for the scale:
                |dy_r[c]| <= gamma(n_f + 1) sum_j W[r, j] |x_j[c]| + FLT_MIN;     concat's copy of x_i is exact.
  backward  one chain over the len_T(j) entries of column j (members only, in ascending source order), each term with
            the one rounding of dy / cnt, the self term last:
                |ddx_j[c]| <= gamma(len_T(j) + 2) (sum_r W[r, j] |dy_r[c]| + [self] |dy_slot(j)[c]|) + FLT_MIN.

The exact statement: on data on the grid of 2^-6 a row whose cnt is a power of two gives the fp64 value itself (every
partial sum is exact, whatever its order, and so is the scale)."""
import functools
import hashlib

import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
ALL = 0                                      # DP_CSR_SAMPLE_ALL
MAX_K = 64
THR_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = {"none": 0, "gcn": 1, "concat": 2}
KS = (1, 2, 10, 25, 64, ALL)
FS = (1, 63, 64, 65, 130)
# the issue's lengths for every k of KS (0, 1, k - 1, k, k + 1, 63 .. 65, 127 .. 129, 200) and the edge of the chunks the
# kernel keeps in registers (4 x 64 = 256): 256, 257 and a row beyond it
PLANTED = (0, 1, 2, 3, 9, 10, 11, 24, 25, 26, 63, 64, 65, 127, 128, 129, 200, 256, 257, 300)
LAYOUTS = {"tight": (lambda w: w, 0), "pad4": (lambda w: 4 * (w // 4 + 1), 0),
           "odd": (lambda w: w + 1 if w % 2 == 0 else w + 2, 0), "mis": (lambda w: 4 * (w // 4 + 1), 1)}
TARGETS = ("all", "subset")
GRAPHS = ("directed", "undirected", "batch")
SEED = 0x9E3779B97F4A7C15                    # the table's seed: both key words non-zero, the top bit set


def _seed(text):
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def moved(ref, got, bound):
    """The largest |got - ref| / bound."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / bound).max()) if np.size(ref) else 0.0


# ------------------------------------------------------------------ Philox4x32-10 and the keys
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint32 arrays) of Philox4x32-10 at counter (c0 .. c3) and key (k0, k1), broadcast."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & m32 for a in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return tuple(np.broadcast_arrays(*(a.astype(np.uint32) for a in (c0, c1, c2, c3))))


def keys(seed, i, j):
    """key(i, j) as uint64 arrays (i, j broadcast; seed a Python int in [0, 2^64), or an array of such)."""
    seed = np.asarray(seed, dtype=np.uint64)
    h = philox4x32_10(i, j, 0, 0, seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32))[0]
    return (h.astype(np.uint64) << np.uint64(32)) | (np.asarray(j, dtype=np.uint64) + np.zeros_like(h, dtype=np.uint64))


# ------------------------------------------------------------------ the graphs
class Csr:
    """A host CSR with GLOBAL columns, unique and ascending in every row, and its transposed CSR (sources ascending)."""

    def __init__(self, n, rows, cols, directed, off=None):
        key = np.unique(np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64))
        self.n, self.directed = int(n), bool(directed)
        self.rows, self.indices = (key // n).astype(np.int64), (key % n).astype(np.int32)
        self.nnz = int(key.size)
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=n))]).astype(np.int32)
        order = np.lexsort((self.rows, self.indices))
        self.indices_t = self.rows[order].astype(np.int32)
        self.cols_t = self.indices[order].astype(np.int64)            # the column of every transposed entry
        self.indptr_t = np.concatenate([[0], np.cumsum(np.bincount(self.indices, minlength=n))]).astype(np.int32)
        self.off = np.array([0, n], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)
        if not directed:
            assert np.array_equal(self.indptr, self.indptr_t) and np.array_equal(self.indices, self.indices_t)


def row_len(g):
    return np.diff(g.indptr).astype(np.int64)


def col_len(g):
    return np.diff(g.indptr_t).astype(np.int64)


def _directed():
    """301 nodes: every length of PLANTED twice (rows 0 .. 39; odd rows hold their self loop where they hold anything),
    the rest 0 .. 12 entries at random columns, every fifth of them with its self loop."""
    n, rng = 301, np.random.default_rng(_seed("sample-directed"))
    rows, cols = [], []
    lens = list(PLANTED) * 2 + list(rng.integers(0, 13, n - 2 * len(PLANTED)))
    for i, d in enumerate(lens):
        d = int(d)
        others = np.delete(np.arange(n), i)
        loop = d > 0 and (i % 2 == 1 if i < 2 * len(PLANTED) else i % 5 == 0)
        c = rng.choice(others, d - int(loop), replace=False)
        c = np.concatenate([c, [i]]) if loop else c
        rows += [i] * d
        cols += list(c)
    return Csr(n, rows, cols, True)


def _undirected():
    """341 nodes: the planted nodes 0 .. 39 (every length of PLANTED twice, the second copy with a self loop where it
    holds anything) are joined to nodes of the pool 40 .. 340 only, so their lengths are exact; the pool's own lengths are
    what that leaves, plus a few edges among its members."""
    n, rng = 341, np.random.default_rng(_seed("sample-undirected"))
    pool = np.arange(2 * len(PLANTED), n)
    rows, cols = [], []
    for i, d in enumerate(list(PLANTED) * 2):
        loop = d > 0 and i >= len(PLANTED)
        c = rng.choice(pool, d - int(loop), replace=False)
        rows += [i] * (d - int(loop)) + list(c) + ([i] if loop else [])
        cols += list(c) + [i] * (d - int(loop)) + ([i] if loop else [])
    a, b = rng.choice(pool, 150), rng.choice(pool, 150)
    rows += list(a) + list(b)
    cols += list(b) + list(a)
    return Csr(n, rows, cols, False)


BATCH_SIZES = (70, 5, 131)
BATCH_LENS = ((0, 1, 2, 9, 10, 11, 63, 64, 65), (), (0, 1, 3, 24, 25, 26, 65, 127, 128, 129))


def batch_edge_lists():
    """Per graph of the batch (sizes BATCH_SIZES, the second edgeless): graph-local (src, dst), directed."""
    rng = np.random.default_rng(_seed("sample-batch"))
    out = []
    for n, planted in zip(BATCH_SIZES, BATCH_LENS):
        src, dst = [], []
        if planted:
            lens = list(planted) * 2 + list(rng.integers(0, 8, n - 2 * len(planted)))
            for i, d in enumerate(lens):
                d = int(d)
                loop = d > 0 and i % 2 == 1
                c = rng.choice(np.delete(np.arange(n), i), d - int(loop), replace=False)
                src += [i] * d
                dst += list(c) + ([i] if loop else [])
        out.append((np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)))
    return out


def _batch():
    off = np.concatenate([[0], np.cumsum(BATCH_SIZES)])
    rows = np.concatenate([s + off[b] for b, (s, _) in enumerate(batch_edge_lists())])
    cols = np.concatenate([d + off[b] for b, (_, d) in enumerate(batch_edge_lists())])
    return Csr(int(off[-1]), rows, cols, True, off)


@functools.lru_cache(maxsize=None)
def graph(name):
    return {"directed": _directed, "undirected": _undirected, "batch": _batch}[name]()


@functools.lru_cache(maxsize=None)
def targets(gname, which):
    """None ("all"), or a shuffled strict subset of the nodes (int32) that leaves out at least one node of every row
    length the graph has and keeps at least one of every length it has twice."""
    if which == "all":
        return None
    g = graph(gname)
    lens, rng = row_len(g), np.random.default_rng(_seed("sample-targets-" + gname))
    out = np.zeros(g.n, dtype=bool)
    for d in np.unique(lens):
        members = np.nonzero(lens == d)[0]
        out[rng.choice(members, max(1, members.size // 3), replace=False)] = True
        if members.size >= 2:
            assert not out[members].all()
    keep = np.nonzero(~out)[0]
    rng.shuffle(keep)
    assert 0 < keep.size < g.n and not np.array_equal(keep, np.sort(keep))
    return keep.astype(np.int32)


# ------------------------------------------------------------------ the selection
class Sample:
    """The sample of `nodes` (None: every node) on graph g at (seed, k, mode): thr uint64 [m], cnt int64 [m], `sel` a
    bool per stored entry (False in rows that are no target), `addself` bool [m] (gcn: the node joins its sample)."""

    def __init__(self, g, seed, k, mode, nodes=None):
        assert k == ALL or 1 <= k <= MAX_K
        self.g, self.seed, self.k, self.mode = g, seed, k, mode
        self.nodes = np.arange(g.n, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
        self.m = self.nodes.size
        self.slot = np.full(g.n, -1, dtype=np.int64)
        self.slot[self.nodes] = np.arange(self.m)
        key = keys(seed, g.rows, g.indices)
        self.key = key
        self.thr = np.full(self.m, THR_ALL, dtype=np.uint64)
        self.sel = np.zeros(g.nnz, dtype=bool)
        ns = np.zeros(self.m, dtype=np.int64)
        self.selfin = np.zeros(self.m, dtype=bool)
        for r, i in enumerate(self.nodes):
            lo, hi = int(g.indptr[i]), int(g.indptr[i + 1])
            if k != ALL and hi - lo > k:
                self.thr[r] = np.sort(key[lo:hi])[k - 1]
            self.sel[lo:hi] = key[lo:hi] <= self.thr[r]
            ns[r] = int(self.sel[lo:hi].sum())
            self.selfin[r] = bool((self.sel[lo:hi] & (g.indices[lo:hi] == i)).any())
        self.ns = ns
        self.addself = (mode == "gcn") & ~self.selfin
        self.cnt = ns + self.addself

    def mask(self):
        """[m, n] float64 0/1: the sampled entries, plus the node itself under gcn."""
        g = self.g
        M = np.zeros((self.m, g.n))
        e = np.nonzero(self.sel)[0]
        M[self.slot[g.rows[e]], g.indices[e]] = 1.0
        M[np.nonzero(self.addself)[0], self.nodes[self.addself]] = 1.0
        return M

    def weights(self):
        return self.mask() / np.maximum(self.cnt, 1)[:, None]


@functools.lru_cache(maxsize=None)
def sample(gname, k, mode, which, seed=SEED):
    return Sample(graph(gname), seed, k, mode, targets(gname, which))


# ------------------------------------------------------------------ references and bounds
def n_fwd(cnt):
    """Roundings a term passes in the forward, the scale included."""
    cnt = np.asarray(cnt, dtype=np.int64)
    return -(-cnt // 4) + 3 * -(-cnt // 64) + 2 + 1


def fwd_from(W, cnt, x, nodes, mode):
    """(y float64, bound) of the forward with the dense weights W [m, n]."""
    x64 = x.astype(np.float64)
    mean, mag = W @ x64, np.abs(W) @ np.abs(x64)
    bound = gamma(n_fwd(cnt))[:, None] * mag + FLT_MIN
    if mode == "concat":
        return np.hstack([x64[nodes], mean]), np.hstack([np.full_like(mean, FLT_MIN), bound])
    return mean, bound


def fwd_ref(s, x):
    return fwd_from(s.weights(), s.cnt, x, s.nodes, s.mode)


def bwd_from(W, g, dy, nodes, mode, self_term=True):
    """(dx float64 [n, F], bound) of the backward with the dense weights W [m, n]."""
    dy64 = dy.astype(np.float64)
    F = dy.shape[1] // 2 if mode == "concat" else dy.shape[1]
    dmean = dy64[:, F:] if mode == "concat" else dy64
    dx, mag = W.T @ dmean, np.abs(W).T @ np.abs(dmean)
    if mode == "concat" and self_term:
        dx[nodes] += dy64[:, :F]
        mag[nodes] += np.abs(dy64[:, :F])
    return dx, gamma(col_len(g) + 2)[:, None] * mag + FLT_MIN


def bwd_ref(s, dy):
    return bwd_from(s.weights(), s.g, dy, s.nodes, s.mode)


def plan(n_rows, n, F, k, d):
    """dp_csr_sample_mean_plan restated: (rows per workgroup, forward workgroups, backward workgroups, tier of a row of d
    entries, its key chunks, of those in registers, 64-column forward passes, 256-column backward passes)."""
    tier = 0 if k == ALL or d <= k else (1 if d <= 64 else 2)
    chunks = 0 if tier == 0 else -(-d // 64)
    return (4, -(-n_rows // 4), -(-n // 4), tier, chunks, min(chunks, 4), -(-F // 64), -(-F // 256))


# ------------------------------------------------------------------ inputs
def inputs(case, grid=False):
    """x [n, F], dy [m, F or 2F] fp32 of the case; grid=True: on the grid of 2^-6 in [-4, 4]."""
    gname, k, F, _, mode, which = case
    g, t = graph(gname), targets(gname, which)
    m = g.n if t is None else t.size
    rng = np.random.default_rng(_seed("sample-in-" + case_id(case)))
    wy = 2 * F if mode == "concat" else F
    if grid:
        return ((np.rint(rng.uniform(-4, 4, (g.n, F)) * 64) / 64).astype(np.float32),
                (np.rint(rng.uniform(-4, 4, (m, wy)) * 64) / 64).astype(np.float32))
    return rng.standard_normal((g.n, F)).astype(np.float32), rng.standard_normal((m, wy)).astype(np.float32)


def padded(a, ld):
    """[rows, ld] fp32: `a` in the leading columns, NaN behind them."""
    out = np.full((a.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def layout_of(case, width):
    ld, off = LAYOUTS[case[3]]
    return ld(width), off


def case_id(case):
    gname, k, F, layout, mode, which = case
    return f"{gname}-k{'all' if k == ALL else k}-F{F}-{layout}-{mode}-{which}"


# ------------------------------------------------------------------ the table: (graph, k, F, layout, mode, targets)
def _table():
    cases, lay, modes = [], list(LAYOUTS), list(MODES)
    for gi, gname in enumerate(GRAPHS):                          # every graph at every k and F; the rest in turn
        for ki, k in enumerate(KS):
            for fi, F in enumerate(FS):
                cases.append((gname, k, F, lay[(gi + ki + fi) % 4], modes[(gi + ki + 2 * fi) % 3], TARGETS[(ki + fi) % 2]))
    for k in KS:                                                 # every k in every mode on both target forms
        for mode in modes:
            for which in TARGETS:
                cases.append(("directed", k, 65, "odd", mode, which))
                cases.append(("undirected", k, 64, "pad4", mode, which))
    for F in FS:                                                 # every width in every layout and mode
        for li, layout in enumerate(lay):
            for mode in modes:
                cases.append(("directed", 10, F, layout, mode, TARGETS[li % 2]))
    for mode in modes:                                           # the batch in every mode on both target forms
        for which in TARGETS:
            cases.append(("batch", 10, 63, "mis", mode, which))
            cases.append(("batch", 64, 130, "tight", mode, which))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return tuple(out)


CASES = _table()
