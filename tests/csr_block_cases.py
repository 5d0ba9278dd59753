"""Case table and numpy restatement of the sampled frontier blocks (dp_csr_block_build, dp_csr_block_mean_fwd / _bwd,
dp_csr_block_plan restated), shared by tests/test_csr_block_cpu.py, tests/test_gpu_csr_block.py and
tests/test_gpu_csr_block_model.py.

Philox, the keys, `Sample`, the three graphs, the layouts and the fp64 bounds `fwd_from` / `bwd_from` are those of
tests/csr_sample_cases.py (imported, not copied).  Restated here: for targets T, k and a seed

    src   = the ascending, duplicate-free ids of T u U_{i in T} S(i)     slot[src[s]] = s, -1 elsewhere
    thr_r = the k-th smallest key of row T[r] when it has more than k entries, else all-ones;  cnt_r = |S(T[r])|

`Block` walks the target rows only (it never hashes a row that is no target), so it also serves the 2^20-node ring;
`from_sample` derives the same block from the sibling's `Sample`, and the CPU test holds the two against each other and
against a brute-force set union.

The compact mean needs no bound of its own: with x_src = x[src] it must give the BITS of dp_csr_sample_mean_fwd, and
dx_src the rows src of dp_csr_sample_mean_bwd's dx, so the sibling's bounds hold for it as they stand."""
import functools

import numpy as np

from tests import csr_sample_cases as SC

ALL, THR_ALL, MODES, LAYOUTS, GRAPHS, FS, SEED = SC.ALL, SC.THR_ALL, SC.MODES, SC.LAYOUTS, SC.GRAPHS, SC.FS, SC.SEED
KS = (1, 2, 10, 64, ALL)
TARGET_SETS = ("one", "seven", "lengths", "all", "empty", "nested")
LAYER_STEP = 0x9E3779B97F4A7C15              # layer l of a nested stack samples with (seed + l * this) mod 2^64
CHUNK, SCAN = 256, 256                       # flags per compaction chunk; chunk counts per scan step


def layer_seed(seed, layer):
    return (seed + layer * LAYER_STEP) % (1 << 64)


# ------------------------------------------------------------------ the restatement
class Block:
    """src, slot, n_src, thr (uint64 [m]), cnt (int64 [m]) of the targets `nodes` (None: every node) on g at (seed, k)."""

    def __init__(self, g, seed, k, nodes=None):
        assert k == ALL or 1 <= k <= SC.MAX_K
        self.g, self.seed, self.k = g, seed, k
        self.nodes = np.arange(g.n, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
        self.m = self.nodes.size
        self.thr = np.full(self.m, THR_ALL, dtype=np.uint64)
        self.cnt = np.zeros(self.m, dtype=np.int64)
        picked = [self.nodes]
        for r, i in enumerate(self.nodes):
            cols = g.indices[int(g.indptr[i]):int(g.indptr[i + 1])]
            if k != ALL and cols.size > k:
                key = SC.keys(seed, int(i), cols)
                self.thr[r] = np.sort(key)[k - 1]
                cols = cols[key <= self.thr[r]]
            self.cnt[r] = cols.size
            picked.append(cols.astype(np.int64))
        self.src = np.unique(np.concatenate(picked))
        self.n_src = int(self.src.size)
        self.slot = np.full(g.n, -1, dtype=np.int64)
        self.slot[self.src] = np.arange(self.n_src)


def from_sample(s):
    """(src, slot) from the sibling's `Sample` (any self mode: the targets are in src whatever the mode)."""
    g = s.g
    src = np.unique(np.concatenate([s.nodes, g.indices[s.sel].astype(np.int64)]))
    slot = np.full(g.n, -1, dtype=np.int64)
    slot[src] = np.arange(src.size)
    return src, slot


def plan(n_rows, n, F, k):
    """dp_csr_block_plan restated: (flags per chunk, chunks, scan steps, smallest cap, workgroups of mark, count, fill,
    forward, backward at n_src = the smallest cap, 64-column forward passes, 256-column backward passes)."""
    chunks = -(-n // CHUNK)
    cap = n if k == ALL else min(n, n_rows * (k + 1))
    return (CHUNK, chunks, -(-chunks // SCAN), cap, -(-n_rows // 4), chunks, chunks, -(-n_rows // 4), -(-cap // 4),
            -(-F // 64), -(-F // 256))


def workspace_bytes(n):
    return ((-(-n // CHUNK) + 1) * 4 + 15) // 16 * 16


# ------------------------------------------------------------------ ring lattices of degree 8 (the compaction's edges)
class Ring:
    """n nodes on a ring, each joined to the four on either side: undirected, every row 8 entries, ascending."""

    def __init__(self, n):
        assert n > 8
        self.n, self.directed = int(n), False
        offs = np.array([-4, -3, -2, -1, 1, 2, 3, 4], dtype=np.int64)
        self.indices = np.sort((np.arange(n, dtype=np.int64)[:, None] + offs) % n, axis=1).astype(np.int32).reshape(-1)
        self.indptr = (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32)
        self.indptr_t, self.indices_t, self.nnz = self.indptr, self.indices, 8 * int(n)


BIG_RING = (1 << 20) + 1
# one below, at and one above one chunk; the same around one scan step; the ring of 2^20 + 1 nodes: 4097 chunks (the last
# holds one node), 17 scan steps with a carry
RING_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * SCAN - 1, CHUNK * SCAN, CHUNK * SCAN + 1, BIG_RING)
RING_K = 2                                   # 8 entries a row: every row is sampled (tier B)


@functools.lru_cache(maxsize=None)
def ring(n):
    return Ring(n)


@functools.lru_cache(maxsize=None)
def ring_targets(n):
    """Shuffled distinct targets that hold node 0 and the last node (the partial chunk): 4096 on the big ring, about a
    fifth of the nodes elsewhere."""
    rng = np.random.default_rng(SC._seed(f"block-ring-{n}"))
    count = 4096 if n == BIG_RING else min(max(7, n // 5), 1024)
    t = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), count - 2, replace=False)])
    rng.shuffle(t)
    return t.astype(np.int32)


@functools.lru_cache(maxsize=None)
def ring_block(n):
    return Block(ring(n), SEED, RING_K, ring_targets(n))


# ------------------------------------------------------------------ target sets on the three graphs
@functools.lru_cache(maxsize=None)
def targets(gname, tname, k=10):
    """int32 ids, or None for "all".  "nested": the src of the block of "seven" at layer 1's seed (the targets of layer
    0 in a two-layer stack, at the same k; the block on them is then drawn at SEED = layer 0's seed)."""
    g = SC.graph(gname)
    rng = np.random.default_rng(SC._seed(f"block-targets-{gname}-{tname}"))
    lens = SC.row_len(g)
    if tname == "all":
        return None
    if tname == "empty":
        return np.zeros(0, dtype=np.int32)
    if tname == "one":
        return np.array([int(np.nonzero(lens == 65)[0][0])], dtype=np.int32)      # a row of tier C
    if tname == "seven":
        t = rng.choice(g.n, 7, replace=False)
        assert not np.array_equal(t, np.sort(t))
        return t.astype(np.int32)
    if tname == "lengths":
        t = np.array([rng.choice(np.nonzero(lens == d)[0]) for d in np.unique(lens)])
        rng.shuffle(t)
        return t.astype(np.int32)
    assert tname == "nested"
    return Block(g, layer_seed(SEED, 1), k, targets(gname, "seven")).src.astype(np.int32)


@functools.lru_cache(maxsize=None)
def block(gname, tname, k):
    return Block(SC.graph(gname), SEED, k, targets(gname, tname, k))


@functools.lru_cache(maxsize=None)
def sample(gname, tname, k, mode):
    return SC.Sample(SC.graph(gname), SEED, k, mode, targets(gname, tname, k))


BUILD_CASES = tuple((g, t, k) for g in GRAPHS for t in TARGET_SETS for k in KS)


def build_id(case):
    g, t, k = case
    return f"{g}-{t}-k{'all' if k == ALL else k}"


# ------------------------------------------------------------------ the mean's table: (graph, targets, k, F, layout, mode)
def _mean_table():
    cases, lay, modes, sets = [], list(LAYOUTS), list(MODES), ("seven", "lengths", "all", "nested", "one")
    for gi, gname in enumerate(GRAPHS):                          # every graph at every k and F; the rest in turn
        for ki, k in enumerate(KS):
            for fi, F in enumerate(FS):
                cases.append((gname, sets[(gi + ki + fi) % 5], k, F, lay[(gi + ki + fi) % 4], modes[(gi + ki + 2 * fi) % 3]))
    for F in FS:                                                 # every width in every layout and mode
        for li, layout in enumerate(lay):
            for mode in modes:
                cases.append(("directed", ("lengths", "nested")[li % 2], 10, F, layout, mode))
    for gname in GRAPHS:                                         # the nested form in every mode on every graph
        for mode in modes:
            cases.append((gname, "nested", 2, 65, "odd", mode))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return tuple(out)


MEAN_CASES = _mean_table()


def mean_id(case):
    g, t, k, F, layout, mode = case
    return f"{g}-{t}-k{'all' if k == ALL else k}-F{F}-{layout}-{mode}"


def mean_inputs(case):
    """x [n, F], dy [m, F or 2F] fp32 of the case."""
    gname, tname, k, F, _, mode = case
    g, t = SC.graph(gname), targets(gname, tname, k)
    m = g.n if t is None else t.size
    rng = np.random.default_rng(SC._seed("block-in-" + mean_id(case)))
    return (rng.standard_normal((g.n, F)).astype(np.float32),
            rng.standard_normal((m, 2 * F if mode == "concat" else F)).astype(np.float32))
