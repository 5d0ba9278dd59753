"""Top-k pooling on CSR (dp_csr_topk_*) restated in numpy — this file is the definition the kernels are
held to — with the fp64 forward and backward, the restatement of dp_csr_topk_plan, the dgate bound and the case table.

    k_b   = min(n_b, max(1, ceil(float64(ratio) * n_b)))   or   min(k, n_b)
    key_i = (ord(score_i) << 32) | (0xffffffff - local_i),  ord(bits) = ~bits under a set sign bit, bits | 0x80000000
            otherwise, after -0.0 is made +0.0
    thr_b = the k_b-th largest key of graph b, 0 when k_b == n_b;   kept: key_i >= thr_b
    new rows in ascending old id: perm [n'], new_id [n] (-1: dropped); A' = A[perm][:, perm] as CSR with global and
    graph-local columns and edge_map (the old position of every kept entry), the same for a transposed CSR of its own
    x_out[r] = x[perm[r]] * gate[perm[r]];  dx_i = dy[new_id[i]] * gate_i;  dgate_i = sum_f dy[new_id[i], f] x[i, f]

The integer outputs, x_out and dx are compared EXACTLY (x_out and dx are one fp32 multiply).  dgate: the kernel sums a
lane's columns f = lane, lane + 64, .. in one fma chain (ceil(F / 64) roundings) and then adds the 64 lanes in a butterfly
(6 roundings), so |dgate - exact| <= gamma_r * sum_f |dy x|, gamma_r = r u / (1 - r u), r = ceil(F / 64) + 6, u = 2^-24."""
import math
import zlib

import numpy as np

U = 2.0 ** -24
PLAN_INTS = 10
KREG, MAX_THREADS, ROWS_PER_WG, SCAN_THREADS = 4, 1024, 32, 1024


# ------------------------------------------------------------------ keys, counts, plan
def ord_bits(bits):
    b = np.asarray(bits, dtype=np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def keys(score, local):
    """uint64 keys of fp32 scores at graph-local ids."""
    bits = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    low = (np.uint64(0xFFFFFFFF) - np.asarray(local, dtype=np.uint64))
    return (ord_bits(bits).astype(np.uint64) << np.uint64(32)) | low


def counts(sizes, ratio=None, k=None):
    assert (ratio is None) != (k is None)
    if k is not None:
        return np.array([min(int(k), int(n)) for n in sizes], dtype=np.int64)
    return np.array([min(int(n), max(1, math.ceil(float(np.float64(ratio) * np.float64(int(n)))))) for n in sizes],
                    dtype=np.int64)


def cdiv(a, b):
    return -(-a // b)


def threads(max_n):
    return min(MAX_THREADS, max(64, 64 * cdiv(max_n, 64 * KREG)))


def plan(n, n_out, B, max_n, n_b, k_b, F):
    """dp_csr_topk_plan restated."""
    T = threads(max_n)
    tier = 0 if k_b >= n_b else (1 if n_b <= T * KREG else 2)
    passes = 4 + cdiv(int(n_b - 1).bit_length(), 8)
    nblk = cdiv(n_out, ROWS_PER_WG)
    return (T, tier, cdiv(n_b, T) if tier else 0, passes if tier else 0, cdiv(n_b, T), B, nblk, cdiv(nblk, SCAN_THREADS),
            cdiv(n_out, 4), cdiv(n, 4))


# ------------------------------------------------------------------ graphs
class Graph:
    """A batch of graphs as one block-diagonal host CSR with GLOBAL columns (a single graph: one member)."""

    def __init__(self, sizes, directed, weighted, edgeless=(), pad_to=None, seed=0, bipartite=False):
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n, self.B = int(self.off[-1]), len(sizes)
        self.directed, self.weighted, self.pad_to = directed, weighted, pad_to
        rows, cols = [], []
        for b, nb in enumerate(self.sizes):
            nb = int(nb)
            if b in edgeless:
                continue
            i = np.arange(nb, dtype=np.int64)
            if bipartite:                                            # even nodes to odd nodes only
                r = np.repeat(i[::2], 3)
                c = (r + 1 + 2 * np.tile(np.arange(3), i[::2].size)) % nb
                ok = (c % 2 == 1)
                r, c = r[ok], c[ok]
            else:
                lens = (i * 7 + b + seed) % 10                       # row lengths 0 .. 9
                r = np.repeat(i, lens)
                j = np.concatenate([np.arange(x) for x in lens]) if nb < 5000 else _ranges(lens)
                c = (r * 2654435761 + j * 40503 + 17 * seed + b) % nb
                loops = i[i % 7 == 3] if nb > 3 else i[:1]         # self loops
                hub = np.arange(min(nb, 300), dtype=np.int64)        # one hub row
                r = np.concatenate([r, loops, np.full(hub.size, nb // 2)])
                c = np.concatenate([c, loops, hub])
            if not directed:
                r, c = np.concatenate([r, c]), np.concatenate([c, r])
            rows.append(r + self.off[b])
            cols.append(c + self.off[b])
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
        key = np.unique(rows * self.n + cols)
        self.rows, self.indices = (key // max(self.n, 1)), (key % max(self.n, 1))
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=self.n))]).astype(np.int64)
        self.nnz = int(key.size)
        order = np.lexsort((self.rows, self.indices))                # the transposed CSR: by column, then by row
        self.t_perm = order
        self.rows_t, self.indices_t = self.indices[order], self.rows[order]
        self.indptr_t = np.concatenate([[0], np.cumsum(np.bincount(self.rows_t, minlength=self.n))]).astype(np.int64)
        self.values = self.values_t = None
        if weighted:
            rng = np.random.default_rng(100 + seed)
            v = rng.uniform(0.25, 1.0, self.nnz).astype(np.float32)
            if not directed:                                         # a_ij = a_ji
                lo, hi = np.minimum(self.rows, self.indices), np.maximum(self.rows, self.indices)
                v = (((lo * 31 + hi * 17) % 97 + 24) / 128.0).astype(np.float32)
            self.values, self.values_t = v, v[order]
        if not directed:
            assert np.array_equal(self.indptr, self.indptr_t) and np.array_equal(self.indices, self.indices_t)

    def graph_of(self, node):
        return np.searchsorted(self.off, node, side="right") - 1

    def edge_lists(self):
        """Per graph (src, dst[, weight]) with graph-local ids: what `CsrBatch.from_edge_lists(symmetric=False)` takes."""
        out = []
        gb = self.graph_of(self.rows)
        for b in range(self.B):
            m = gb == b
            out.append((self.rows[m] - self.off[b], self.indices[m] - self.off[b],
                        None if self.values is None else self.values[m]))
        return out


def _ranges(lens):
    """concatenate([arange(x) for x in lens]) without the Python loop."""
    tot = int(lens.sum())
    start = np.repeat(np.cumsum(lens) - lens, lens)
    return np.arange(tot, dtype=np.int64) - start


def ring(n):
    """One undirected 0/1 ring of n nodes (every node joined to its two neighbours) as a `Graph`, without the generator's
    sorts: the large single graph of the GPU test."""
    g = Graph.__new__(Graph)
    g.sizes, g.off, g.n, g.B = np.array([n], dtype=np.int64), np.array([0, n], dtype=np.int64), n, 1
    g.directed, g.weighted, g.pad_to, g.values, g.values_t = False, False, None, None, None
    i = np.arange(n, dtype=np.int64)
    cols = np.sort(np.stack([(i - 1) % n, (i + 1) % n], 1), 1)
    g.rows, g.indices = np.repeat(i, 2), cols.reshape(-1)
    g.indptr = 2 * np.arange(n + 1, dtype=np.int64)
    g.nnz = 2 * n
    g.rows_t, g.indices_t, g.indptr_t, g.t_perm = g.rows, g.indices, g.indptr, np.arange(2 * n)
    return g


SINGLE = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 65537)
SPECS = {f"g{n}": dict(sizes=(n,), directed=(i % 2 == 1), weighted=(i % 3 == 0), seed=i) for i, n in enumerate(SINGLE)}
SPECS.update(
    mixed=dict(sizes=(257, 1, 64, 2, 65, 63, 1025, 255), directed=False, weighted=False, seed=21),
    edgeless=dict(sizes=(5, 7, 300), directed=True, weighted=True, edgeless=(1,), seed=22),
    padded=dict(sizes=(40, 17, 64), directed=False, weighted=True, pad_to=100, seed=23),
    bigmix=dict(sizes=(4097, 256, 1024, 1023), directed=True, weighted=False, seed=24),
    bipart=dict(sizes=(20,), directed=False, weighted=True, bipartite=True, seed=25),
    bipart_batch=dict(sizes=(20, 12), directed=True, weighted=False, bipartite=True, seed=26),
)
BATCHES = ("mixed", "edgeless", "padded", "bigmix", "bipart_batch")      # held as a CsrBatch; the others as a CsrGraph
_G = {}


def graph(name):
    if name not in _G:
        _G[name] = Graph(**SPECS[name])
    return _G[name]


# ------------------------------------------------------------------ scores
SKINDS = ("ties", "equal", "zeros", "special", "normal", "parity")
NAN_POS, NAN_NEG, NAN_SIG = 0x7FC00000, 0xFFC00000, 0x7F800001


def scores(gname, kind):
    g = graph(gname)
    rng = np.random.default_rng(7 + len(gname) + SKINDS.index(kind))
    n = g.n
    if kind == "ties":                                               # four levels: long runs of equal scores at any cut
        s = rng.integers(0, 4, n).astype(np.float32) / 2
    elif kind == "equal":
        s = np.full(n, 0.5, np.float32)
    elif kind == "zeros":                                            # +0.0 against -0.0, a few values around them
        s = np.where(rng.integers(0, 2, n) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        s[rng.integers(0, n, max(1, n // 8))] = 1.0
        s[rng.integers(0, n, max(1, n // 8))] = -1.0
    elif kind == "special":                                          # +-inf and a NaN of each sign among normal scores
        s = rng.standard_normal(n).astype(np.float32)
        bits = s.view(np.uint32)
        for v in (0x7F800000, 0xFF800000, NAN_POS, NAN_NEG, NAN_SIG, 0xFFFFFFFF, 0x80000000, 0x00000001, 0x80000001):
            bits[rng.integers(0, n, max(1, n // 16))] = v
    elif kind == "parity":                                           # even local ids beat odd ones
        s = (1.0 - (np.arange(n) - g.off[g.graph_of(np.arange(n))]) % 2).astype(np.float32)
    else:
        s = rng.standard_normal(n).astype(np.float32)
    return s


# ------------------------------------------------------------------ the restatement
class Pooled:
    """Everything dp_csr_topk_select / _induce write for graph `g`, scores `s` and the kept counts `kb`."""

    def __init__(self, g, s, kb, own_keys=None):
        """`own_keys`: keys to select by instead of `keys(s, local)` (the CPU test plants wrong orders with it)."""
        self.g, self.kb = g, np.asarray(kb, dtype=np.int64)
        self.new_off = np.concatenate([[0], np.cumsum(self.kb)]).astype(np.int64)
        self.n_out = int(self.new_off[-1])
        local = np.arange(g.n) - g.off[g.graph_of(np.arange(g.n))]
        self.keys = keys(s, local) if own_keys is None else own_keys
        self.thr = np.zeros(g.B, dtype=np.uint64)
        kept = np.zeros(g.n, dtype=bool)
        for b in range(g.B):
            lo, hi = int(g.off[b]), int(g.off[b + 1])
            kk = self.keys[lo:hi]
            if self.kb[b] < hi - lo:
                self.thr[b] = np.sort(kk)[::-1][self.kb[b] - 1]
            kept[lo:hi] = kk >= self.thr[b]
        self.kept = kept
        self.perm = np.nonzero(kept)[0].astype(np.int32)             # ascending old id
        assert self.perm.size == self.n_out
        self.new_id = np.full(g.n, -1, dtype=np.int32)
        self.new_id[self.perm] = np.arange(self.n_out, dtype=np.int32)
        (self.indptr, self.indices, self.local, self.edge_map) = self._induce(g.rows, g.indices)
        if g.directed:
            (self.indptr_t, self.indices_t, self.local_t, self.edge_map_t) = self._induce(g.rows_t, g.indices_t)
        else:
            self.indptr_t, self.indices_t, self.local_t, self.edge_map_t = (self.indptr, self.indices, self.local,
                                                                            self.edge_map)
        self.nnz = int(self.indptr[-1])

    def _induce(self, rows, cols):
        both = (self.new_id[rows] >= 0) & (self.new_id[cols] >= 0) if rows.size else np.zeros(0, bool)
        em = np.nonzero(both)[0].astype(np.int32)
        r, c = self.new_id[rows[em]], self.new_id[cols[em]]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=self.n_out))]).astype(np.int32)
        gb = np.searchsorted(self.new_off, r, side="right") - 1
        return indptr, c.astype(np.int32), (c - self.new_off[gb]).astype(np.int32), em

    def as_graph(self, pad_to=None):
        """The pooled graph as a `Graph`: the input of the next pooling layer's restatement."""
        g, out = self.g, Graph.__new__(Graph)
        out.sizes, out.off, out.n, out.B = self.kb, self.new_off, self.n_out, g.B
        out.directed, out.weighted, out.pad_to, out.nnz = g.directed, g.weighted, pad_to, self.nnz
        rows = lambda ip: np.repeat(np.arange(self.n_out, dtype=np.int64), np.diff(ip))
        out.rows, out.indices, out.indptr = rows(self.indptr), self.indices.astype(np.int64), self.indptr.astype(np.int64)
        out.rows_t, out.indices_t = rows(self.indptr_t), self.indices_t.astype(np.int64)
        out.indptr_t = self.indptr_t.astype(np.int64)
        out.values = None if g.values is None else g.values[self.edge_map]
        out.values_t = None if g.values is None else g.values_t[self.edge_map_t]
        return out

    def edge_lists(self):
        """Per pooled graph (src, dst) with graph-local ids."""
        r = np.repeat(np.arange(self.n_out), np.diff(self.indptr))
        gb = np.searchsorted(self.new_off, r, side="right") - 1
        return [(r[gb == b] - self.new_off[b], self.local[gb == b]) for b in range(self.g.B)]


def forward32(x, gate, perm):
    """The fp32 product the kernel must give bit for bit."""
    y = x[perm]
    return y if gate is None else (y * gate[perm][:, None]).astype(np.float32)


def backward32(dy, gate, p):
    dx = np.zeros((p.g.n, dy.shape[1]), dtype=np.float32)
    dx[p.perm] = dy if gate is None else (dy * gate[p.perm][:, None]).astype(np.float32)
    return dx


def dgate64(dy, x, p):
    """(dgate in fp64, sum_f |dy x|) over all n rows; zeros on a dropped node."""
    prod = dy.astype(np.float64) * x[p.perm].astype(np.float64)
    ref, mag = np.zeros(p.g.n), np.zeros(p.g.n)
    ref[p.perm], mag[p.perm] = prod.sum(1), np.abs(prod).sum(1)
    return ref, mag


def dgate_bound(F, mag):
    r = cdiv(F, 64) + 6
    return (r * U / (1.0 - r * U)) * mag


def moved(ref, got, bound):
    """max |got - ref| / bound; an entry with bound 0 must be exact."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    zero = bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ------------------------------------------------------------------ layouts, inputs, cases
LAYOUTS = {"tight": (lambda w: w, 0), "pad4": (lambda w: (w // 4 + 1) * 4, 0), "odd": (lambda w: (w + 1) | 1, 0),
           "mis": (lambda w: w + 3, 1)}                              # (leading dimension, floats off the 16-byte grid)
FS = (1, 63, 64, 65, 130)
SELS = (("ratio", 0.5), ("ratio", 0.25), ("ratio", 1e-9), ("ratio", 1.0), ("k", 3), ("k", 5000), ("ratio", 0.3))


def sel_counts(g, sel):
    return counts(g.sizes, **{sel[0]: sel[1]})


def inputs(case):
    """(x [n, F], gate [n] or None, dy [n', F]) of a case, fp32."""
    gname, kind, sel, F, _, gated = case
    g = graph(gname)
    rng = np.random.default_rng(zlib.crc32(repr((gname, kind, F)).encode()))
    x = rng.standard_normal((g.n, F)).astype(np.float32)
    gate = np.tanh(rng.standard_normal(g.n)).astype(np.float32) if gated else None
    dy = rng.standard_normal((int(sel_counts(g, sel).sum()), F)).astype(np.float32)
    return x, gate, dy


_P = {}


def pooled(gname, kind, sel):
    key = (gname, kind, sel)
    if key not in _P:
        g = graph(gname)
        _P[key] = Pooled(g, scores(gname, kind), sel_counts(g, sel))
    return _P[key]


def _cases():
    out = []
    lay = list(LAYOUTS)
    for i, n in enumerate(SINGLE):                                   # every planted size as a single graph
        F = 1 if n > 5000 else FS[i % 5]
        out.append((f"g{n}", SKINDS[i % 5], SELS[i % len(SELS)], F, lay[i % 4], i % 4 != 3))
        out.append((f"g{n}", SKINDS[(i + 2) % 5], SELS[(i + 3) % len(SELS)], 1 if n > 5000 else FS[(i + 1) % 5],
                    lay[(i + 1) % 4], i % 4 != 1))
    for kind in ("ties", "equal", "zeros", "special"):              # every score kind in both select tiers
        out.append(("g257", kind, ("ratio", 0.5), 64, "tight", True))
        out.append(("g4097", kind, ("ratio", 0.5), 1, "tight", True))
    out.append(("g65537", "ties", ("ratio", 0.5), 1, "tight", True))
    out.append(("g4096", "ties", ("ratio", 0.25), 1, "mis", False))
    for j, b in enumerate(("mixed", "edgeless", "padded", "bigmix")):
        for m, sel in enumerate(SELS):
            out.append((b, SKINDS[(j + m) % 5], sel, FS[(j + m) % 5] if b != "bigmix" else 1, lay[(j + m) % 4],
                        (j + m) % 3 != 0))
    for F in FS:                                                     # every width at every layout
        for name in LAYOUTS:
            out.append(("padded", "normal", ("ratio", 0.5), F, name, F != 64))
    out.append(("bipart", "parity", ("ratio", 0.5), 65, "odd", True))          # the kept set has no edge: nnz' = 0
    out.append(("bipart_batch", "parity", ("ratio", 0.5), 63, "pad4", True))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2][0]}{c[2][1]:g}-F{c[3]}-{c[4]}-{'gate' if c[5] else 'copy'}"
