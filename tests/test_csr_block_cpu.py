"""The sampled frontier blocks without a GPU: the restatement of tests/csr_block_cases.py against a
brute-force Python set union and against the sibling's `Sample`; the new C entries' symbols, signatures and every
refusal (each comes back before a launch); dp_csr_block_plan restated and held against the library; what the table
reaches (every chunk and scan-step edge, every tier A / B / C); the new kernels' resources read from the gfx950 library;
that each seeded mistake changes an integer output or leaves the sibling's bound; the surface of the ops and modules."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_block_cases as BC
from tests import csr_sample_cases as SC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR

NEW = ("dp_csr_block_plan", "dp_csr_block_workspace_bytes", "dp_csr_block_build", "dp_csr_block_mean_fwd",
       "dp_csr_block_mean_bwd")
KERNELS = ("k_csr_block_zero", "k_csr_block_mark", "k_csr_block_count", "k_csr_block_scan", "k_csr_block_fill",
           "k_csr_block_mean_fwd", "k_csr_block_mean_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ the restatement
def _brute(g, seed, k, nodes):
    """src as a Python set union, the sample of a row as its k smallest keys."""
    out = set(int(i) for i in nodes)
    for i in nodes:
        cols = [int(j) for j in g.indices[int(g.indptr[i]):int(g.indptr[i + 1])]]
        if k != BC.ALL and len(cols) > k:
            cols = sorted(cols, key=lambda j: int(SC.keys(seed, int(i), j)))[:k]
        out |= set(cols)
    return sorted(out)


@pytest.mark.parametrize("gname", BC.GRAPHS)
def test_the_restatement_is_the_set_union(gname):
    g = SC.graph(gname)
    for tname in BC.TARGET_SETS:
        for k in BC.KS:
            b = BC.block(gname, tname, k)
            assert b.src.tolist() == _brute(g, BC.SEED, k, b.nodes), (tname, k)
            assert np.array_equal(b.slot[b.src], np.arange(b.n_src)) and (b.slot >= 0).sum() == b.n_src
            assert np.isin(b.nodes, b.src).all()                      # T itself, always
            for mode in SC.MODES:                                     # the sibling's Sample, in every self mode
                s = BC.sample(gname, tname, k, mode)
                src, slot = BC.from_sample(s)
                assert np.array_equal(src, b.src) and np.array_equal(slot, b.slot) and np.array_equal(s.thr, b.thr)
                if mode != "gcn":
                    assert np.array_equal(s.cnt, b.cnt)
            if tname in ("seven", "nested") and k != BC.ALL and k <= 10:
                assert b.n_src < g.n, (tname, k)                      # a strict subset wherever that matters
    seven = [BC.block(gname, "seven", k).n_src for k in (1, 2, 10)]
    nested = [BC.block(gname, "nested", k).n_src for k in (1, 2, 10)]
    print(f"{gname}: n = {g.n}, n_src of seven targets {seven}, of their second hop {nested}")
    assert 7 < seven[0] <= seven[2] and nested[2] > seven[2]
    assert BC.block(gname, "empty", 10).n_src == 0 and BC.block(gname, "all", 10).n_src == g.n
    assert BC.targets(gname, "nested", 10).size == BC.Block(g, BC.layer_seed(BC.SEED, 1), 10,
                                                             BC.targets(gname, "seven")).n_src


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_and_bound(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[f][1]) == len(fns[f][1])
    assert names("dp_csr_block_plan") == ["n_rows", "n", "F", "k", "plan_out"]
    assert names("dp_csr_block_workspace_bytes") == ["n"]
    assert names("dp_csr_block_build") == ["indptr", "indices", "nodes", "n_rows", "n", "k", "seed", "slot", "src", "cap",
                                           "n_src", "thr", "cnt", "workspace", "workspace_bytes", "stream"]
    assert names("dp_csr_block_mean_fwd") == ["x_src", "ldx", "indptr", "indices", "nodes", "slot", "n_src", "y", "ldy",
                                              "thr", "cnt", "n_rows", "n", "F", "k", "self_mode", "seed", "stream"]
    assert names("dp_csr_block_mean_bwd") == ["dy", "lddy", "indptr_t", "indices_t", "tslot", "src", "n_src", "thr", "cnt",
                                              "dx_src", "lddx", "n", "F", "self_mode", "seed", "stream"]
    root = os.path.join(os.path.dirname(_lib.__file__), "..")
    header = open(os.path.join(root, "include", "diffpool_hip.h")).read()
    assert "#define DP_CSR_BLOCK_PLAN_INTS 11" in header and _lib.CSR_BLOCK_PLAN_INTS == 11
    section = header[header.index("N10  sampled frontier blocks"):]
    assert section.count("aggregators.py:30-63") >= 6                 # the section and each of the five entries
    assert lib.dp_version() == 100
    build = open(os.path.join(root, "graph_pooling_amd", "csrc", "build.sh")).read()
    assert "dp_csr_block.hip" in build and "dp_csr_sample_body.h -nt" in build
    for unit in ("dp_csr_sample.hip", "dp_csr_block.hip"):            # both units instantiate the one shared body
        text = open(os.path.join(root, "graph_pooling_amd", "csrc", unit)).read()
        assert '#include "dp_csr_sample_body.h"' in text and "sm_fwd_body<" in text and "sm_bwd_body<" in text
        assert "philox_word0(unsigned" not in text and "sm_nth_set_bit(u64" not in text


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1 / -2."""
    buf = (C.c_double * 64)()
    ibuf = (C.c_int * 64)()
    p, i = C.addressof(buf), C.addressof(ibuf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    w = p if p % 16 == 0 else p + 8
    need = lib.dp_csr_block_workspace_bytes(8)
    assert need == 16 == BC.workspace_bytes(8)

    def build(ip=i, ix=i, nodes=i, m=4, n=8, k=2, seed=1, slot=i, src=i, cap=8, n_src=i, thr=p, cnt=i, ws=w, wsb=64):
        return lib.dp_csr_block_build(ip, ix, nodes, m, n, k, seed, slot, src, cap, n_src, thr, cnt, ws, wsb, None)

    for kw, text in ((dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"), (dict(slot=None), "slot is NULL"),
                     (dict(src=None), "src is NULL"), (dict(n_src=None), "n_src is NULL"), (dict(thr=None), "thr is NULL"),
                     (dict(cnt=None), "cnt is NULL"), (dict(ws=None), "workspace must be there"),
                     (dict(ws=w + 4), "16-byte aligned"), (dict(ip=i + 1), "indptr is not 4-byte"),
                     (dict(nodes=i + 2), "nodes is not 4-byte"), (dict(slot=i + 1), "slot is not 4-byte"),
                     (dict(src=i + 3), "src is not 4-byte"), (dict(thr=p + 4), "thr is not 8-byte"),
                     (dict(m=-1), "n_rows=-1 must not be negative"), (dict(n=-1, m=0), "n=-1 must not be negative"),
                     (dict(m=9), "n_rows=9 exceeds n=8"), (dict(nodes=None), "n_rows=4 differs from n=8 without nodes"),
                     (dict(k=65), "k=65 must be 1 .. 64"), (dict(k=-1), "k=-1 must be 1 .. 64"),
                     (dict(cap=7), "cap=7 is below the block's bound 8"), (dict(k=1, cap=7), "cap=7 is below the block's bound 8"),
                     (dict(k=0, cap=7), "cap=7 is below the block's bound 8"), (dict(m=1, k=2, cap=2), "bound 3")):
        assert build(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert build(wsb=need - 1) == -2 and "workspace too small: need >= 16" in _err(lib)
    assert build(m=0) == 0 and build(m=0, n=0, nodes=None, cap=0) == 0          # nothing to do, no launch

    def fwd(x=p, ldx=8, ip=i, ix=i, nodes=i, slot=i, n_src=6, y=p, ldy=8, thr=p, cnt=i, m=4, n=8, F=8, k=10, mode=0):
        return lib.dp_csr_block_mean_fwd(x, ldx, ip, ix, nodes, slot, n_src, y, ldy, thr, cnt, m, n, F, k, mode, 1, None)

    for kw, text in ((dict(x=None), "x_src is NULL"), (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(slot=None), "slot is NULL"), (dict(y=None), "y is NULL"), (dict(thr=None), "thr is NULL"),
                     (dict(cnt=None), "cnt is NULL"), (dict(x=p + 2), "x_src is not 4-byte"),
                     (dict(slot=i + 1), "slot is not 4-byte"), (dict(thr=p + 4), "thr is not 8-byte"),
                     (dict(nodes=i + 1), "nodes is not 4-byte"), (dict(ldx=7), "ldx=7 smaller than its width 8"),
                     (dict(ldy=7), "ldy=7 smaller than its width 8"), (dict(ldy=15, mode=2), "ldy=15 smaller than its width 16"),
                     (dict(m=-1), "n_rows=-1"), (dict(n=-2, m=0, n_src=0), "n=-2"), (dict(F=-1), "F=-1"),
                     (dict(n_src=-1), "n_src=-1 must not be negative"), (dict(n_src=9), "n_src=9 exceeds n=8"),
                     (dict(k=65), "k=65 must be 1 .. 64"), (dict(mode=3), "self_mode=3 must be"),
                     (dict(m=9), "n_rows=9 exceeds n=8"), (dict(nodes=None), "n_rows=4 differs from n=8 without nodes")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert fwd(m=0) == 0 and fwd(F=0, ldx=0, ldy=0) == 0 and fwd(m=0, n=0, n_src=0, nodes=None) == 0

    def bwd(dy=p, lddy=8, ipt=i, ixt=i, tslot=i, src=i, n_src=6, thr=p, cnt=i, dx=p, lddx=8, n=8, F=8, mode=0):
        return lib.dp_csr_block_mean_bwd(dy, lddy, ipt, ixt, tslot, src, n_src, thr, cnt, dx, lddx, n, F, mode, 1, None)

    for kw, text in ((dict(dy=None), "dy is NULL"), (dict(ipt=None), "indptr_t is NULL"), (dict(ixt=None), "indices_t is NULL"),
                     (dict(src=None), "src is NULL"), (dict(thr=None), "thr is NULL"), (dict(cnt=None), "cnt is NULL"),
                     (dict(dx=None), "dx_src is NULL"), (dict(dy=p + 3), "dy is not 4-byte"),
                     (dict(tslot=i + 2), "tslot is not 4-byte"), (dict(src=i + 1), "src is not 4-byte"),
                     (dict(thr=p + 4), "thr is not 8-byte"), (dict(lddy=7), "lddy=7 smaller than its width 8"),
                     (dict(lddy=15, mode=2), "lddy=15 smaller than its width 16"), (dict(lddx=7), "lddx=7 smaller"),
                     (dict(n=-1, n_src=0), "n=-1"), (dict(F=-1), "F=-1"), (dict(n_src=-1), "n_src=-1"),
                     (dict(n_src=9), "n_src=9 exceeds n=8"), (dict(mode=3), "self_mode=3 must be")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert bwd(n_src=0) == 0 and bwd(F=0, lddy=0, lddx=0) == 0 and bwd(n=0, n_src=0) == 0
    assert bwd(n_src=0, tslot=None) == 0


def test_plan_and_workspace_restatements_equal_the_library(lib):
    out = (C.c_int * _lib.CSR_BLOCK_PLAN_INTS)()
    for n_rows, n in ((0, 0), (1, 1), (4, 255), (5, 256), (7, 257), (256, 65535), (4096, 65536), (65537, 65537),
                      (4096, BC.BIG_RING), (1 << 20, 1 << 21), (1 << 27, (1 << 31) - 1)):
        for F in (0, 1, 63, 64, 65, 130, 256, 257):
            for k in BC.KS + (63,):
                assert lib.dp_csr_block_plan(n_rows, n, F, k, out) == 0
                assert tuple(out) == BC.plan(n_rows, n, F, k), (n_rows, n, F, k)
        assert lib.dp_csr_block_workspace_bytes(n) == BC.workspace_bytes(n)
    assert lib.dp_csr_block_workspace_bytes(-5) == BC.workspace_bytes(0) == 16
    for bad, text in (((-1, 4, 1, 1), "n_rows=-1"), ((4, -1, 1, 1), "n=-1"), ((4, 4, -1, 1), "F=-1"),
                      ((4, 4, 1, 65), "k=65 must be"), ((5, 4, 1, 1), "n_rows=5 exceeds n=4")):
        assert lib.dp_csr_block_plan(*bad, out) == -1 and text in _err(lib), bad
    assert lib.dp_csr_block_plan(4, 4, 1, 1, None) == -1 and "plan_out is NULL" in _err(lib)


def test_the_table_reaches_every_chunk_and_step_edge_and_every_tier():
    plans = {n: BC.plan(BC.ring_targets(n).size, n, 1, BC.RING_K) for n in BC.RING_SIZES}
    chunk, step = BC.CHUNK, BC.CHUNK * BC.SCAN
    assert [plans[n][1] for n in (chunk - 1, chunk, chunk + 1)] == [1, 1, 2]
    assert [plans[n][2] for n in (step - 1, step, step + 1)] == [1, 1, 2]
    big = plans[BC.BIG_RING]
    assert big[2] >= 2 and BC.BIG_RING % chunk == 1 and BC.ring_targets(BC.BIG_RING).size == 4096
    for n in BC.RING_SIZES:
        t = BC.ring_targets(n)
        assert np.unique(t).size == t.size and {0, n - 1} <= set(t.tolist()) and not np.array_equal(t, np.sort(t))
        g = BC.ring(n)
        assert (np.diff(g.indptr) == 8).all() and (np.diff(g.indices.reshape(n, 8), axis=1) > 0).all()
    b = BC.ring_block(step + 1)
    assert b.n_src < step + 1 and b.slot[step] == b.n_src - 1 and (b.src >= step).sum() >= 1      # beyond the first scan step
    assert (b.cnt == BC.RING_K).all() and (b.thr != BC.THR_ALL).all()
    # the three graphs: every target set at every k, every tier among the targets' rows
    assert {(c[0], c[1], c[2]) for c in BC.BUILD_CASES} == {(g, t, k) for g in BC.GRAPHS for t in BC.TARGET_SETS for k in BC.KS}
    for gname in BC.GRAPHS:
        lens = SC.row_len(SC.graph(gname))
        for tname in ("lengths", "all", "nested"):
            t = BC.targets(gname, tname, 10)
            rows = lens if t is None else lens[t]
            assert {SC.plan(1, 1, 1, 10, int(d))[3] for d in rows} == {0, 1, 2}, (gname, tname)
        t = BC.targets(gname, "lengths")
        assert set(lens[t]) == set(lens) and t.size == np.unique(lens).size
        assert SC.plan(1, 1, 1, 10, int(lens[BC.targets(gname, "one")[0]]))[3] == 2
        mine = [c for c in BC.MEAN_CASES if c[0] == gname]
        assert {(c[2], c[3]) for c in mine} == {(k, F) for k in BC.KS for F in BC.FS}
        assert {c[5] for c in mine} == set(SC.MODES) and {c[1] for c in mine} >= {"seven", "lengths", "all", "nested", "one"}
    assert {(c[3], c[4], c[5]) for c in BC.MEAN_CASES if c[0] == "directed"} >= {(F, l, m) for F in BC.FS for l in SC.LAYOUTS
                                                                                for m in SC.MODES}


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_block_kernels_use_no_scratch_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if "k_csr_block_" in d["name"]}
    assert len(ks) == len(KERNELS) and all(any(k in n for n in ks) for k in KERNELS), sorted(ks)
    for name, d in ks.items():
        print(d)
        assert d["scratch"] == 0 and d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0 and d.get("agprs", 0) == 0, d
        assert d["vgprs"] <= 128, d
        if "mean" in name or "mark" in name:
            assert d["lds_static"] == 0, d                            # the sibling's budget: no LDS in the sampling bodies
        else:
            assert d["lds_static"] <= 16, d                           # one int per wave of the chunk


# ------------------------------------------------------------------ the compaction, emulated, and the seeded mistakes
def _compact(flags, cap, lose_carry=False, drop_last_chunk=False):
    """count / scan / fill as the three launches do them: (src, slot, n_src)."""
    n = flags.size
    chunks = -(-n // BC.CHUNK)
    csum = np.array([int(flags[c * BC.CHUNK:(c + 1) * BC.CHUNK].sum()) for c in range(chunks)], dtype=np.int64)
    if drop_last_chunk:
        csum[-1] = 0
    base, carry = np.zeros(chunks, dtype=np.int64), 0
    for s0 in range(0, chunks, BC.SCAN):
        part = csum[s0:s0 + BC.SCAN]
        base[s0:s0 + BC.SCAN] = (0 if lose_carry else carry) + np.cumsum(part) - part
        carry += int(part.sum())
    src, slot = np.full(cap, -9, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for c in range(chunks):
        if drop_last_chunk and c == chunks - 1:
            continue
        ids = c * BC.CHUNK + np.nonzero(flags[c * BC.CHUNK:(c + 1) * BC.CHUNK])[0]
        pos = base[c] + np.arange(ids.size)
        ok = pos < cap
        src[pos[ok]] = ids[ok]
        slot[ids[ok]] = pos[ok]
    return src[:min(carry, cap)], slot, min(carry, cap)


def _valid(src, slot, n):
    ok = src.size == 0 or (src.min() >= 0 and src.max() < n and (np.diff(src) > 0).all())
    return bool(ok and np.array_equal(slot[src], np.arange(src.size)) and (slot >= 0).sum() == src.size)


@pytest.mark.parametrize("n", [n for n in BC.RING_SIZES if n != BC.BIG_RING] + [BC.BIG_RING])
def test_the_emulated_compaction_equals_the_restatement_and_its_mistakes_do_not(n):
    b = BC.ring_block(n)
    flags = np.zeros(n, dtype=bool)
    flags[b.src] = True
    src, slot, n_src = _compact(flags, min(n, b.m * (BC.RING_K + 1)))
    assert n_src == b.n_src and np.array_equal(src, b.src) and np.array_equal(slot, b.slot) and _valid(src, slot, n)
    src, slot, n_src = _compact(flags, n, drop_last_chunk=True)      # the last chunk holds node n - 1, a target
    assert n_src < b.n_src and not np.array_equal(slot, b.slot)
    if BC.plan(b.m, n, 1, BC.RING_K)[2] >= 2:
        src, slot, n_src = _compact(flags, n, lose_carry=True)
        assert not np.array_equal(slot, b.slot) and not _valid(src, slot, n)


@pytest.mark.parametrize("gname", ("directed", "undirected"))
def test_each_seeded_mistake_changes_an_integer_output_or_leaves_the_bound(gname):
    g, k, F = SC.graph(gname), 10, 65
    t = BC.targets(gname, "lengths")
    b = BC.block(gname, "lengths", k)
    lens = SC.row_len(g)
    # a target left out of src (one that nothing samples)
    sampled = np.zeros(g.n, bool)
    for mode in ("none",):
        s = BC.sample(gname, "lengths", k, mode)
        sampled[g.indices[s.sel]] = True
    lonely = [i for i in t if not sampled[i]]
    assert lonely
    src = b.src[b.src != lonely[0]]
    assert not np.array_equal(src, b.src) and src.size == b.n_src - 1
    # a node sampled by exactly one target left out
    hits = np.bincount(g.indices[s.sel], minlength=g.n)
    once = [j for j in np.nonzero(hits == 1)[0] if j not in set(t.tolist())]
    assert once and once[0] in set(b.src.tolist())
    assert np.setdiff1d(b.src, [once[0]]).size == b.n_src - 1
    # a duplicate in src, slot off by one: the host's validation tells
    dup = np.sort(np.concatenate([b.src, b.src[:1]]))
    assert not _valid(dup, b.slot, g.n) and _valid(b.src, b.slot, g.n)
    off = np.where(b.slot >= 0, b.slot + 1, -1)
    assert not _valid(b.src, off, g.n) and not np.array_equal(off, b.slot)
    # k + 1 and k - 1 entries: cnt moves on every sampled row, src moves, and the mean leaves the sibling's bound
    x = np.random.default_rng(SC._seed("block-mistake")).standard_normal((g.n, F)).astype(np.float32)
    ref, bound = SC.fwd_ref(s, x)
    big = lens[t] > k
    for other in (k + 1, k - 1):
        bo = BC.Block(g, BC.SEED, other, t)
        assert (bo.cnt[big] == other).all() and (b.cnt[big] == k).all() and not np.array_equal(bo.src, b.src)
        so = SC.Sample(g, BC.SEED, other, "none", t)
        got, _ = SC.fwd_from(so.weights(), so.cnt, x, so.nodes, "none")
        assert ((np.abs(got - ref) / bound)[big].max(1) > 1.0).all()
    # one seed for both layers: the inner block of a two-layer stack differs from the one drawn at layer 0's seed
    outer = BC.Block(g, BC.layer_seed(BC.SEED, 1), k, BC.targets(gname, "seven"))
    right = BC.Block(g, BC.layer_seed(BC.SEED, 0), k, outer.src)
    wrong = BC.Block(g, BC.layer_seed(BC.SEED, 1), k, outer.src)
    assert not np.array_equal(right.thr, wrong.thr) and not np.array_equal(right.src, wrong.src)
    assert np.array_equal(right.src, BC.block(gname, "nested", k).src)


# ------------------------------------------------------------------ the surface of the ops and modules
def test_the_surface_of_the_ops_and_modules():
    import graph_pooling_amd
    from graph_pooling_amd import ops
    from graph_pooling_amd.graphsage import SupervisedGraphSage
    from graph_pooling_amd.sparse import CsrGraph, NestedSageEncoder, SageConv
    assert graph_pooling_amd.NestedSageEncoder is NestedSageEncoder and "NestedSageEncoder" in graph_pooling_amd.__all__
    g = CsrGraph.from_edges(5, [0, 1], [1, 2], "cpu")
    other = CsrGraph.from_edges(5, [0], [1], "cpu")
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)
    # an empty target set: an empty block, nothing launched (no GPU here)
    e = ops.csr_sample_block(g, i32(), 10, 7)
    assert isinstance(e, ops.SampledBlock) and e.n_src == 0 and e.src.numel() == 0 and e.m == 0
    assert e.slot.tolist() == [-1] * 5 and e.k == 10 and e.seed == 7 and e.graph is g and e.thr.dtype == torch.int64
    assert set(ops.SampledBlock.__slots__) == {"graph", "nodes", "src", "slot", "n_src", "thr", "cnt", "k", "seed"}
    assert ops.csr_sample_block(g, e, None, 1).k == _lib.CSR_SAMPLE_ALL          # a block as the targets (empty too)
    out = ops.csr_block_mean(torch.zeros(0, 3), e, "concat")
    assert out.shape == (0, 6) and out.grad_fn is None
    for k in (0, 65, -3, 1.5, True):
        with pytest.raises(ValueError, match="num_sample must be 1 .. 64 or None"):
            ops.csr_sample_block(g, i32(0), k, 7)
    for seed in (-1, 1 << 64, 0.5, None):
        with pytest.raises(ValueError, match="seed must be a Python int"):
            ops.csr_sample_block(g, i32(0), 10, seed)
    for nodes, text in ((torch.tensor([0, 1]), "int32 tensor"), (i32(0, 0), "distinct"), (i32(5), "outside 0 .. 4"),
                        (i32(-1), "outside 0 .. 4"), ([0, 1], "int32 tensor")):
        with pytest.raises(ValueError, match=text):
            ops.csr_sample_block(g, nodes, 10, 7)
    with pytest.raises(ValueError, match="another container"):
        ops.csr_sample_block(other, e, 10, 7)
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        ops.csr_sample_block(torch.eye(3), i32(0), 10, 7)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.csr_sample_block(g, i32(0, 1), 10, 7)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.csr_sample_block(g, None, 10, 7)
    with pytest.raises(TypeError, match="SampledBlock"):
        ops.csr_block_mean(torch.zeros(0, 3), g)
    with pytest.raises(ValueError, match="self_mode must be"):
        ops.csr_block_mean(torch.zeros(0, 3), e, "mean")
    with pytest.raises(ValueError, match="expected x_src"):
        ops.csr_block_mean(torch.zeros(2, 3), e)
    # SageConv.block / forward_block
    torch.manual_seed(0)
    c1, c2 = SageConv(3, 4, num_sample=10), SageConv(4, 2, num_sample=5, gcn=True)
    blk = c1.block(g, i32(), seed=3)
    assert blk.k == 10 and blk.seed == 3 and c1.forward_block(torch.zeros(0, 3), blk).shape == (0, 4)
    with pytest.raises(ValueError, match="sampled with k = 10"):
        c2.forward_block(torch.zeros(0, 4), blk)
    with pytest.raises(ValueError, match="expected x_src"):
        c1.forward_block(torch.zeros(0, 5), blk)
    with pytest.raises(TypeError, match="SampledBlock"):
        c1.forward_block(torch.zeros(0, 3), g)
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        c1.block(torch.eye(3), i32())
    torch.manual_seed(4)
    a = c1.block(g, i32()).seed
    torch.manual_seed(4)
    assert c1.block(g, i32()).seed == a                                # seed=None: torch's CPU generator
    # NestedSageEncoder
    feats = torch.rand(5, 3)
    enc = NestedSageEncoder(feats, g, [c1, c2])
    assert enc.embed_dim == 2 and list(enc.state_dict()) == ["convs.0.weight", "convs.1.weight"]
    assert NestedSageEncoder.layer_seed(5, 0) == 5 and NestedSageEncoder.layer_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert NestedSageEncoder.layer_seed((1 << 64) - 1, 1) == 0x9E3779B97F4A7C15 - 1 == BC.layer_seed((1 << 64) - 1, 1)
    none = np.zeros(0, dtype=np.int64)
    blocks = enc.blocks(none, 9)
    assert len(blocks) == 2 and blocks[0].nodes is blocks[1] and blocks[1].k == 5 and blocks[0].k == 10
    assert blocks[1].seed == BC.layer_seed(9, 1) and blocks[0].seed == 9
    assert enc(none, seed=9).shape == (0, 2)
    for bad, text in (([0, 0], "distinct"), ([5], "outside 0 .. 4"), ([0.5], "integer node ids")):
        with pytest.raises(ValueError, match=text):
            enc(bad)
    with pytest.raises(ValueError, match="seed must be a Python int"):
        enc.blocks([0], -1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        enc([0, 1], seed=1)
    with pytest.raises(TypeError, match="non-empty sequence of SageConv"):
        NestedSageEncoder(feats, g, [])
    with pytest.raises(TypeError, match="non-empty sequence of SageConv"):
        NestedSageEncoder(feats, g, [torch.nn.Linear(3, 4)])
    with pytest.raises(ValueError, match="follows one of out_dim"):
        NestedSageEncoder(feats, g, [c1, SageConv(5, 2)])
    with pytest.raises(TypeError, match="graph must be"):
        NestedSageEncoder(feats, None, [c1])
    with pytest.raises(TypeError, match="features must be"):
        NestedSageEncoder(3, g, [c1])
    emb = NestedSageEncoder(torch.nn.Embedding(5, 3), g, [c1, c2])
    model = SupervisedGraphSage(2, emb)
    assert sorted(n for n, _ in model.named_parameters()) == ["enc.convs.0.weight", "enc.convs.1.weight",
                                                              "enc.features.weight", "weight"]
    for doc in (SageConv.__doc__, NestedSageEncoder.__doc__, ops.csr_sample_block.__doc__, ops.csr_block_mean.__doc__):
        assert "hipGraph" in doc
    assert "targets" in ops.csr_sample_block.__doc__ and "weighted sampling" in ops.csr_sample_block.__doc__ and "num_sample > 64" in ops.csr_sample_block.__doc__
