"""The fused sampled neighbour mean without a GPU: the Philox known answers of the restatement, the uniformity and the
row-to-row independence of the restated sampler, the new C entries' symbols, signatures and argument errors (every
refusal comes back before a launch), the restatement of dp_csr_sample_mean_plan against the library, what the case table
reaches (every tier and every chunk edge), the kernels' resources from the built library, the restated formulas against
fp64 autograd of the dense mask, the conditioning of the table's data, that the bounds of tests/csr_sample_cases.py
reject each planted mistake, and the surface of `SageConv`, `SageEncoder` and `ops.csr_sample_mean`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import csr_sample_cases as SC
from tests.test_abi_cpu import _header_functions
from tests.test_csr_edge_grad_cpu import KR

NEW = ("dp_csr_sample_mean_plan", "dp_csr_sample_mean_fwd", "dp_csr_sample_mean_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _err(lib):
    return lib.dp_last_error_string().decode()


# ------------------------------------------------------------------ Philox and the sampler
def test_philox_known_answers():
    assert int(SC.philox4x32_10(0, 0, 0, 0, 0, 0)[0]) == 0x6627E8D5
    out = SC.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert int(out[0]) == 0xD16CFE09
    assert [int(w) for w in SC.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # the key: word 0 above the column, the seed's halves as the Philox key, (i, j, 0, 0) as its counter
    seed, i, j = 0x299F31D0A4093822, 0x243F6A88, 0x05A308D3
    assert int(SC.keys(seed, i, j)) == (int(SC.philox4x32_10(i, j, 0, 0, 0xA4093822, 0x299F31D0)[0]) << 32) | j


ROWS = ((13, 5), (65, 10), (200, 25), (11, 10), (64, 1))
N_SEEDS = 4096


def _seeds():
    return ((np.arange(N_SEEDS, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)))[:, None]


def _inclusion(i, cols, k):
    """[N_SEEDS, d] bool: column cols[c] sampled for row i under seed s (the k smallest keys)."""
    key = SC.keys(_seeds(), i, np.asarray(cols)[None, :])
    thr = np.sort(key, axis=1)[:, k - 1]
    inc = key <= thr[:, None]
    assert (inc.sum(1) == k).all()                                   # exactly k, whatever the seed
    return inc


@pytest.mark.parametrize("d,k", ROWS)
def test_the_restated_sampler_is_uniform(d, k):
    cols = np.arange(d) * 3 + 1
    inc = _inclusion(1000 + d, cols, k).astype(np.float64)
    p = k / d
    single = np.abs(inc.sum(0) - N_SEEDS * p) / np.sqrt(N_SEEDS * p * (1 - p))
    print(f"(d, k) = ({d}, {k}): worst single count {single.max():.2f} sigma")
    assert (single <= 5.0).all()
    p2 = k * (k - 1) / (d * (d - 1))
    joint = inc.T @ inc
    pairs = joint[np.triu_indices(d, 1)]
    sigma = np.sqrt(N_SEEDS * p2 * (1 - p2))
    dev = np.abs(pairs - N_SEEDS * p2)
    print(f"(d, k) = ({d}, {k}): worst pair {dev.max() / sigma if sigma else 0.0:.2f} sigma over {pairs.size} pairs")
    assert (dev <= 6.0 * sigma).all()


def test_two_rows_that_share_columns_draw_independently():
    d, k = 13, 5
    cols = np.arange(d) * 7 + 2
    a, b = _inclusion(3, cols, k).astype(np.float64), _inclusion(4, cols, k).astype(np.float64)
    p = (k / d) ** 2
    joint = a.T @ b                                                   # column c in row 3's sample and c' in row 4's
    dev = np.abs(joint - N_SEEDS * p) / np.sqrt(N_SEEDS * p * (1 - p))
    print(f"worst joint count across two rows {dev.max():.2f} sigma over {joint.size} pairs")
    assert (dev <= 6.0).all()
    assert not np.array_equal(a, b)


def test_the_selection_of_the_restatement():
    """thr is the k-th smallest key, exactly min(d, k) entries are taken, an all-ones thr takes all, another seed moves
    the rows with d > k and no others."""
    g = SC.graph("directed")
    lens = SC.row_len(g)
    for k in SC.KS:
        s = SC.sample("directed", k, "none", "all")
        assert np.array_equal(s.ns, lens if k == SC.ALL else np.minimum(lens, k))
        assert np.array_equal(s.thr == SC.THR_ALL, np.ones(g.n, bool) if k == SC.ALL else lens <= k)
        gcn = SC.sample("directed", k, "gcn", "all")
        assert np.array_equal(gcn.cnt, gcn.ns + ~gcn.selfin) and gcn.selfin.any() and (~gcn.selfin).any()
        if k != SC.ALL:
            other = SC.Sample(g, SC.SEED + 1, k, "none")
            assert np.array_equal(other.thr != s.thr, lens > k)
    full = SC.sample("directed", 10, "gcn", "all")
    stored_self = np.array([(g.indices[g.indptr[i]:g.indptr[i + 1]] == i).any() for i in range(g.n)])
    assert (stored_self & ~full.selfin & (lens > 10)).any()          # a stored self loop that the sample left out


# ------------------------------------------------------------------ symbols, signatures, refusals
def test_new_entries_are_declared_and_bound(lib):
    fns = _header_functions()
    names = lambda f: [a.split()[-1].lstrip("*") for a in fns[f][1]]
    for f in NEW:
        assert f in fns and hasattr(lib, f) and f in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[f][1]) == len(fns[f][1])
    assert names("dp_csr_sample_mean_plan") == ["n_rows", "n", "F", "k", "self_mode", "d", "plan_out"]
    assert names("dp_csr_sample_mean_fwd") == ["x", "ldx", "indptr", "indices", "nodes", "y", "ldy", "thr", "cnt", "n_rows",
                                               "n", "F", "k", "self_mode", "seed", "stream"]
    assert names("dp_csr_sample_mean_bwd") == ["dy", "lddy", "indptr_t", "indices_t", "slot", "thr", "cnt", "dx", "lddx",
                                               "n", "F", "self_mode", "seed", "stream"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "diffpool_hip.h")).read()
    for text in ("#define DP_CSR_SAMPLE_ALL 0", "#define DP_CSR_SAMPLE_MAX_K 64", "#define DP_CSR_SAMPLE_PLAN_INTS 8",
                 "#define DP_CSR_SAMPLE_SELF_NONE 0", "#define DP_CSR_SAMPLE_SELF_GCN 1",
                 "#define DP_CSR_SAMPLE_SELF_CONCAT 2"):
        assert text in header
    assert (_lib.CSR_SAMPLE_ALL, _lib.CSR_SAMPLE_MAX_K, _lib.CSR_SAMPLE_PLAN_INTS) == (SC.ALL, SC.MAX_K, 8)
    assert _lib.CSR_SAMPLE_SELF == SC.MODES
    block = header[header.index("N8  GraphSAGE neighbour sampling"):]
    assert block.count("aggregators.py:30-63") >= 4                  # the section and each of the three entries
    assert lib.dp_version() == 100


def test_every_argument_error_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached a launch would fail with a HIP error (a positive code), not -1."""
    buf = (C.c_double * 64)()
    ibuf = (C.c_int * 16)()
    p, i = C.addressof(buf), C.addressof(ibuf)

    def fwd(x=p, ldx=8, ip=i, ix=i, nodes=None, y=p, ldy=8, thr=p, cnt=i, m=4, n=4, F=8, k=10, mode=0, seed=1):
        return lib.dp_csr_sample_mean_fwd(x, ldx, ip, ix, nodes, y, ldy, thr, cnt, m, n, F, k, mode, seed, None)

    for kw, text in ((dict(x=None), "x is NULL"), (dict(ip=None), "indptr is NULL"), (dict(ix=None), "indices is NULL"),
                     (dict(y=None), "y is NULL"), (dict(thr=None), "thr is NULL"), (dict(cnt=None), "cnt is NULL"),
                     (dict(x=p + 2), "x is not 4-byte"), (dict(y=p + 1), "y is not 4-byte"),
                     (dict(thr=p + 4), "thr is not 8-byte"), (dict(nodes=i + 1), "nodes is not 4-byte"),
                     (dict(ldx=7), "ldx=7 smaller than its width 8"), (dict(ldy=7), "ldy=7 smaller than its width 8"),
                     (dict(ldy=15, mode=2), "ldy=15 smaller than its width 16"),
                     (dict(m=-1), "n_rows=-1 must not be negative"), (dict(n=-2, m=0), "n=-2 must not be negative"),
                     (dict(F=-1), "F=-1 must not be negative"), (dict(k=65), "k=65 must be 1 .. 64"),
                     (dict(k=-1), "k=-1 must be 1 .. 64"), (dict(k=1 << 20), "must be 1 .. 64"),
                     (dict(mode=3), "self_mode=3 must be"), (dict(mode=-1), "self_mode=-1 must be"),
                     (dict(m=5, nodes=i), "n_rows=5 exceeds n=4"), (dict(m=3), "n_rows=3 differs from n=4 without nodes")):
        assert fwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert fwd(m=0, n=0) == 0 and fwd(F=0, ldx=0, ldy=0) == 0 and fwd(m=0, nodes=i) == 0     # nothing to do, no launch
    assert fwd(m=0, n=0, k=0) == 0                                    # the sentinel for every neighbour

    def bwd(dy=p, lddy=8, ipt=i, ixt=i, slot=None, thr=p, cnt=i, dx=p, lddx=8, n=4, F=8, mode=0, seed=1):
        return lib.dp_csr_sample_mean_bwd(dy, lddy, ipt, ixt, slot, thr, cnt, dx, lddx, n, F, mode, seed, None)

    for kw, text in ((dict(dy=None), "dy is NULL"), (dict(ipt=None), "indptr_t is NULL"),
                     (dict(ixt=None), "indices_t is NULL"), (dict(thr=None), "thr is NULL"), (dict(cnt=None), "cnt is NULL"),
                     (dict(dx=None), "dx is NULL"), (dict(dy=p + 3), "dy is not 4-byte"),
                     (dict(dx=p + 2), "dx is not 4-byte"), (dict(thr=p + 4), "thr is not 8-byte"),
                     (dict(slot=i + 2), "slot is not 4-byte"), (dict(lddy=7), "lddy=7 smaller than its width 8"),
                     (dict(lddy=15, mode=2), "lddy=15 smaller than its width 16"),
                     (dict(lddx=7), "lddx=7 smaller than its width 8"), (dict(n=-1), "n=-1 must not be negative"),
                     (dict(F=-1), "F=-1 must not be negative"), (dict(mode=3), "self_mode=3 must be")):
        assert bwd(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert bwd(n=0) == 0 and bwd(F=0, lddy=0, lddx=0) == 0


def test_plan_restatement_equals_the_library(lib):
    out = (C.c_int * _lib.CSR_SAMPLE_PLAN_INTS)()
    seen = set()
    for n_rows, n in ((0, 0), (1, 1), (4, 4), (5, 301), (301, 301), (1 << 20, 1 << 21)):
        for F in (0, 1, 63, 64, 65, 130, 256, 257, 1000):
            for k in SC.KS + (63,):
                for d in (0, 1, k - 1 if k else 5, k, k + 1, 63, 64, 65, 127, 128, 129, 200, 256, 257, 300, 100000):
                    if d < 0:
                        continue
                    for mode in (0, 1, 2):
                        assert lib.dp_csr_sample_mean_plan(n_rows, n, F, k, mode, d, out) == 0
                        assert tuple(out) == SC.plan(n_rows, n, F, k, d), (n_rows, n, F, k, d)
                        seen.add(tuple(out)[3:6])
    assert {t for t, _, _ in seen} == {0, 1, 2} and {(c, r) for t, c, r in seen if t == 2} >= {(2, 2), (4, 4), (5, 4)}
    for bad, text in (((-1, 4, 1, 1, 0, 1), "n_rows=-1"), ((4, -1, 1, 1, 0, 1), "n=-1"), ((4, 4, -1, 1, 0, 1), "F=-1"),
                      ((4, 4, 1, 65, 0, 1), "k=65 must be"), ((4, 4, 1, 1, 3, 1), "self_mode=3"),
                      ((4, 4, 1, 1, 0, -1), "d=-1"), ((5, 4, 1, 1, 0, 1), "n_rows=5 exceeds n=4")):
        assert lib.dp_csr_sample_mean_plan(*bad, out) == -1 and text in _err(lib), bad
    assert lib.dp_csr_sample_mean_plan(4, 4, 1, 1, 0, 1, None) == -1 and "plan_out is NULL" in _err(lib)


def test_the_table_reaches_every_tier_and_every_chunk_edge():
    assert {c[0] for c in SC.CASES} == set(SC.GRAPHS) and {c[1] for c in SC.CASES} == set(SC.KS)
    assert {c[2] for c in SC.CASES} == set(SC.FS) and {c[3] for c in SC.CASES} == set(SC.LAYOUTS)
    for gname in SC.GRAPHS:                                          # every k, F, mode and target form on every graph
        mine = [c for c in SC.CASES if c[0] == gname]
        assert {(c[1], c[2]) for c in mine} == {(k, F) for k in SC.KS for F in SC.FS}
        assert {(c[4], c[5]) for c in mine} == {(m, t) for m in SC.MODES for t in SC.TARGETS}
    assert {(c[1], c[4], c[5]) for c in SC.CASES if c[0] == "directed"} == {(k, m, t) for k in SC.KS for m in SC.MODES
                                                                            for t in SC.TARGETS}
    assert {(c[2], c[3], c[4]) for c in SC.CASES if c[0] == "directed"} >= {(F, l, m) for F in SC.FS for l in SC.LAYOUTS
                                                                            for m in SC.MODES}
    for w in (1, 63, 64, 65, 130, 260):
        lds = {name: ld(w) for name, (ld, _) in SC.LAYOUTS.items()}
        assert lds["tight"] == w and lds["pad4"] % 4 == 0 and lds["pad4"] > w and lds["odd"] % 2 == 1 and lds["odd"] > w
    assert SC.LAYOUTS["mis"][1] == 1
    for gname in ("directed", "undirected"):
        g = SC.graph(gname)
        lens = SC.row_len(g)
        assert tuple(lens[:len(SC.PLANTED)]) == SC.PLANTED == tuple(lens[len(SC.PLANTED):2 * len(SC.PLANTED)])
        assert g.n % 4 == 1                                          # the last workgroup holds one row
        for k in SC.KS[:-1]:
            assert {0, 1, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 200} <= set(lens)
            plans = {SC.plan(g.n, g.n, 64, k, int(d))[3:6] for d in lens}
            assert {t for t, _, _ in plans} == ({0, 2} if k == 64 else {0, 1, 2})
            assert {(c, r) for t, c, r in plans if t == 2} == {(2, 2), (3, 3), (4, 4), (5, 4)}    # 65 .. 128, .., 257 .. 300
        self_loop = np.array([(g.indices[g.indptr[i]:g.indptr[i + 1]] == i).any() for i in range(g.n)])
        assert self_loop.any() and (~self_loop & (lens > 0)).any()
        t = SC.targets(gname, "subset")
        assert 0 < t.size < g.n and np.unique(t).size == t.size and not np.array_equal(t, np.sort(t))
        for d in np.unique(lens):                                    # one node of every length left out
            assert not np.isin(np.nonzero(lens == d)[0], t).all()
        for d in SC.PLANTED:                                         # and one of every planted length kept
            assert np.isin(np.nonzero(lens == d)[0], t).any()
    und = SC.graph("undirected")
    assert {65, 128, 129, 200, 257, 300} <= set(SC.col_len(und))      # the backward's 64-entry batches and their edges
    d = SC.graph("directed")
    assert d.directed and not np.array_equal(d.indices, d.indices_t)  # a transposed CSR of its own
    b = SC.graph("batch")
    assert list(np.diff(b.off)) == list(SC.BATCH_SIZES) and b.directed
    assert not SC.row_len(b)[b.off[1]:b.off[2]].any() and not SC.col_len(b)[b.off[1]:b.off[2]].any()     # the edgeless one
    assert (b.indices[b.indptr[b.off[2]]:] >= b.off[2]).all() and {0, 1, 64, 65, 128, 129} <= set(SC.row_len(b))


@pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                     "llvm-readelf) not found")
def test_sample_kernels_use_no_scratch_no_lds_and_do_not_spill(lib):
    ks = {d["name"]: d for d in KR.kernel_resources(_lib.LIB_PATH).values() if "k_csr_sample_mean_" in d["name"]}
    assert len(ks) == 2 and any("fwd" in n for n in ks) and any("bwd" in n for n in ks), sorted(ks)
    for d in ks.values():
        print(d)
        assert d["scratch"] == 0 and d["lds_static"] == 0, d
        assert d["vgpr_spills"] == 0 and d.get("sgpr_spills", 0) == 0, d
        assert d["vgprs"] <= 128 and d.get("agprs", 0) == 0, d


# ------------------------------------------------------------------ the formulas are autograd's
@pytest.mark.parametrize("mode", list(SC.MODES))
@pytest.mark.parametrize("which", SC.TARGETS)
def test_the_reference_is_autograd_of_the_dense_mask(mode, which):
    case = ("batch", 10, 5, "tight", mode, which)
    s = SC.sample("batch", 10, mode, which)
    x32, dy32 = SC.inputs(case)
    x = torch.tensor(x32.astype(np.float64), requires_grad=True)
    mask, cnt, nodes = torch.from_numpy(s.mask()), torch.from_numpy(s.cnt.astype(np.float64)), torch.from_numpy(s.nodes)
    mean = torch.where(cnt[:, None] > 0, mask.div(cnt.clamp(min=1)[:, None]) @ x, torch.zeros(()).double())
    y = torch.cat([x[nodes], mean], 1) if mode == "concat" else mean
    ref, bound = SC.fwd_ref(s, x32)
    assert np.abs(y.detach().numpy() - ref).max() < 1e-13 and (bound > 0).all()
    y.backward(torch.from_numpy(dy32.astype(np.float64)))
    dref, dbound = SC.bwd_ref(s, dy32)
    assert np.abs(x.grad.numpy() - dref).max() < 1e-13 and (dbound > 0).all()
    # the mask restated from the sets: row r holds the k smallest keys of node nodes[r] (and the node under gcn)
    g = s.g
    for r in (0, s.m // 2, s.m - 1):
        i = int(s.nodes[r])
        cols = g.indices[g.indptr[i]:g.indptr[i + 1]].astype(np.int64)
        key = SC.keys(SC.SEED, i, cols)
        want = set(cols[np.argsort(key)[:10]].tolist()) | ({i} if mode == "gcn" else set())
        assert set(np.nonzero(s.mask()[r])[0].tolist()) == want and s.cnt[r] == len(want)


def test_the_data_is_well_conditioned():
    """On at least 99 % of the entries of every case the result stands 64 bounds clear of zero: an error of the size of
    the result cannot hide in the bound."""
    for case in SC.CASES:
        gname, k, F, _, mode, which = case
        s = SC.sample(gname, k, mode, which)
        x, dy = SC.inputs(case)
        ref, bound = SC.fwd_ref(s, x)
        live = np.repeat((s.cnt > 0)[:, None], ref.shape[1], 1)
        if mode == "concat":
            live[:, :F] = True
        assert (np.abs(ref[live]) > 64 * bound[live]).mean() > 0.99, SC.case_id(case)
        dref, dbound = SC.bwd_ref(s, dy)
        live = dref != 0
        assert live.any() and (np.abs(dref[live]) > 64 * dbound[live]).mean() > 0.99, SC.case_id(case)
        assert np.isfinite(ref).all() and np.isfinite(dref).all()


# ------------------------------------------------------------------ the bounds tell a bug from rounding
def _weights_of(s, sel=None, cnt=None, addself=None):
    """Dense weights with parts of the sample replaced (the planted mistakes)."""
    g = s.g
    sel = s.sel if sel is None else sel
    addself = s.addself if addself is None else addself
    M = np.zeros((s.m, g.n))
    e = np.nonzero(sel)[0]
    M[s.slot[g.rows[e]], g.indices[e]] = 1.0
    M[np.nonzero(addself)[0], s.nodes[addself]] += 1.0
    cnt = s.cnt if cnt is None else cnt
    return M / np.maximum(cnt, 1)[:, None]


def _select_count(s, count):
    """The entry mask with `count` smallest keys per target row with more than k entries (the others as they are)."""
    g, sel = s.g, s.sel.copy()
    for r, i in enumerate(s.nodes):
        lo, hi = int(g.indptr[i]), int(g.indptr[i + 1])
        if s.thr[r] != SC.THR_ALL:
            sel[lo:hi] = False
            sel[lo + np.argsort(s.key[lo:hi])[:count]] = True
    return sel


@pytest.mark.parametrize("which", SC.TARGETS)
@pytest.mark.parametrize("gname", ("directed", "undirected"))
def test_the_bounds_reject_each_planted_mistake(gname, which):
    k, F = 10, 65
    g = SC.graph(gname)
    lens = SC.row_len(g)
    for mode in SC.MODES:
        case = (gname, k, F, "tight", mode, which)
        s = SC.sample(gname, k, mode, which)
        x, dy = SC.inputs(case)
        ref, bound = SC.fwd_ref(s, x)
        dref, dbound = SC.bwd_ref(s, dy)
        d_of = lens[s.nodes]
        big = d_of > k

        def fwd_moved(W, rows):
            got, _ = SC.fwd_from(W, s.cnt, x, s.nodes, mode)
            worst = np.abs(got - ref) / bound
            assert (worst[~rows] <= 1.0).all()                       # the mistake stays where it was planted
            return worst[rows].max(1)

        def bwd_moved(W, self_term=True):
            got, _ = SC.bwd_from(W, g, dy, s.nodes, mode, self_term)
            return (np.abs(got - dref) / dbound).max()

        # dividing by d instead of cnt
        assert (fwd_moved(_weights_of(s, cnt=np.where(big, d_of + s.addself, s.cnt)), big) > 1.0).all()
        # k + 1 entries selected, and k - 1 (`<` for `<=` at the threshold)
        for count in (k + 1, k - 1):
            sel = _select_count(s, count)
            cnt = np.where(big, count + s.addself, s.cnt)
            if mode == "gcn":                                        # a self loop that enters or leaves: cnt by its rule
                selfin = np.array([(sel[g.indptr[i]:g.indptr[i + 1]] & (g.indices[g.indptr[i]:g.indptr[i + 1]] == i)).any()
                                   for i in s.nodes])
                W = _weights_of(s, sel=sel, addself=~selfin, cnt=np.where(big, count + ~selfin, s.cnt))
            else:
                W = _weights_of(s, sel=sel, cnt=cnt)
            # under gcn a row whose entry gained or lost IS its self loop keeps its set S u {i}: no mistake there
            differ = big & (W != s.weights()).any(1)
            assert differ.sum() >= 0.9 * big.sum() and (mode == "gcn" or differ.sum() == big.sum())
            assert (fwd_moved(W, differ) > 1.0).all(), (mode, count)
            assert bwd_moved(W) > 1.0
        # the self node counted twice under gcn: a stored and sampled self loop, and the node added on top
        if mode == "gcn":
            assert s.selfin.any()
            W = _weights_of(s, addself=np.ones(s.m, bool), cnt=s.ns + 1)
            twice = s.selfin & (s.ns > 1)                            # a sample of the self loop alone: 2 x_i / 2 = x_i
            assert twice.sum() >= 3 and (fwd_moved(W, twice) > 1.0).all()
            assert bwd_moved(W) > 1.0
        # the self term missing under concat (the backward drops dy[:, :F])
        if mode == "concat":
            assert bwd_moved(s.weights(), self_term=False) > 1.0
            got, _ = SC.fwd_ref(s, x)
            got[:, :F] = 0.0
            assert SC.moved(ref, got, bound) > 1.0
        # a backward that ignores membership: every stored entry of a target row
        stored = np.zeros(g.nnz, bool)
        stored[s.slot[g.rows] >= 0] = True
        assert bwd_moved(_weights_of(s, sel=stored)) > 1.0
        # a backward that divides by the column's cnt_j instead of the row's cnt_i
        every = SC.sample(gname, k, mode, "all")
        Wj = s.mask() / np.maximum(every.cnt, 1)[None, :]
        assert bwd_moved(Wj) > 1.0
        # a dropped last chunk: the entries behind the last multiple of 64 of a row never seen
        sa = SC.sample(gname, SC.ALL, mode, which)
        ref_a, bound_a = SC.fwd_ref(sa, x)
        sel = sa.sel.copy()
        long_rows = np.zeros(sa.m, bool)
        for r, i in enumerate(sa.nodes):
            lo, hi = int(g.indptr[i]), int(g.indptr[i + 1])
            if hi - lo > 64:
                sel[lo + 64 * ((hi - lo - 1) // 64):hi] = False
                long_rows[r] = True
        got, _ = SC.fwd_from(_weights_of(sa, sel=sel), sa.cnt, x, sa.nodes, mode)
        assert long_rows.any() and ((np.abs(got - ref_a) / bound_a)[long_rows].max(1) > 1.0).all()
        dgot, _ = SC.bwd_from(_weights_of(sa, sel=sel), g, dy, sa.nodes, mode)
        dref_a, dbound_a = SC.bwd_ref(sa, dy)
        assert SC.moved(dref_a, dgot, dbound_a) > 1.0


def test_an_fp32_evaluation_in_the_kernels_order_stays_inside():
    """The forward's four partial sums and the backward's one chain, evaluated in fp32 in the kernels' order on three
    cases, stay inside the bounds that reject the mistakes above."""
    f32 = np.float32
    for case in (("directed", 10, 65, "tight", "gcn", "subset"), ("undirected", SC.ALL, 5, "tight", "concat", "all"),
                 ("batch", 64, 3, "tight", "none", "all")):
        gname, k, F, _, mode, which = case
        s, g = SC.sample(gname, k, mode, which), SC.graph(gname)
        x, dy = SC.inputs(case)
        ref, bound = SC.fwd_ref(s, x)
        y = np.zeros((s.m, F), dtype=f32)
        for r, i in enumerate(s.nodes):
            lo, hi = int(g.indptr[i]), int(g.indptr[i + 1])
            ids = g.indices[lo:hi][s.sel[lo:hi]]
            p = np.zeros((4, F), dtype=f32)
            for b0 in range(0, ids.size, 64):
                batch = ids[b0:b0 + 64]
                q4 = batch.size - batch.size % 4
                for q, j in enumerate(batch):
                    p[q % 4 if q < q4 else 0] += x[j]
            if s.addself[r]:
                p[0] += x[i]
            scale = f32(1) / f32(s.cnt[r]) if s.cnt[r] else f32(0)
            y[r] = ((p[0] + p[1]) + (p[2] + p[3])) * scale
        got = np.hstack([x[s.nodes], y]) if mode == "concat" else y
        assert SC.moved(ref, got, bound) <= 1.0
        dref, dbound = SC.bwd_ref(s, dy)
        dx = np.zeros((g.n, F), dtype=f32)
        off = F if mode == "concat" else 0
        for j in range(g.n):
            for e in range(int(g.indptr_t[j]), int(g.indptr_t[j + 1])):
                i = int(g.indices_t[e])
                r = s.slot[i]
                if r >= 0 and (s.thr[r] == SC.THR_ALL or SC.keys(SC.SEED, i, j) <= s.thr[r]):
                    dx[j] += dy[r, off:off + F] / f32(s.cnt[r])
            r = s.slot[j]
            if r >= 0 and mode == "concat":
                dx[j] += dy[r, :F]
            elif r >= 0 and mode == "gcn" and s.addself[r]:
                dx[j] += dy[r] / f32(s.cnt[r])
        assert SC.moved(dref, dx, dbound) <= 1.0


# ------------------------------------------------------------------ the surface of SageConv, SageEncoder and the op
def test_sage_conv_parameters_and_refusals():
    import graph_pooling_amd
    from graph_pooling_amd.sparse import CsrGraph, SageConv, SageEncoder
    assert graph_pooling_amd.SageConv is SageConv and graph_pooling_amd.SageEncoder is SageEncoder
    assert {"SageConv", "SageEncoder"} <= set(graph_pooling_amd.__all__)
    torch.manual_seed(0)
    m = SageConv(5, 4)
    assert list(m.state_dict()) == ["weight"] and m.weight.shape == (4, 10) and m.bias is None and m.num_sample == 10
    w = m.weight.detach()
    assert float(w.abs().max()) <= (6.0 / 14) ** 0.5 and float(w.std()) > 0.1                         # Xavier-uniform
    g = SageConv(5, 4, num_sample=None, gcn=True, bias=True)
    assert g.weight.shape == (4, 5) and g.bias.shape == (4,) and not g.bias.any() and g.num_sample is None
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_sample must be 1 .. 64 or None"):
            SageConv(5, 4, num_sample=bad)
    with pytest.raises(ValueError, match="must be positive"):
        SageConv(0, 4)
    with pytest.raises(TypeError, match="CsrGraph or CsrBatch"):
        m(torch.rand(3, 5), torch.eye(3))
    e = CsrGraph.from_edges(3, [0], [1], "cpu")
    with pytest.raises(ValueError, match="expected x"):
        m(torch.rand(4, 5), e)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        m(torch.rand(3, 5), e, seed=1)
    with pytest.raises(TypeError, match="conv must be a SageConv"):
        SageEncoder(torch.rand(3, 5), e, torch.nn.Linear(5, 4))
    with pytest.raises(TypeError, match="graph must be"):
        SageEncoder(torch.rand(3, 5), None, m)
    enc = SageEncoder(torch.rand(3, 5), e, m)
    assert enc.embed_dim == 4 and list(enc.state_dict()) == ["conv.weight"]
    for bad, text in (([0, 0], "distinct"), ([3], "outside 0 .. 2"), ([-1], "outside 0 .. 2"), ([0.5], "integer node ids"),
                      (np.zeros((2, 2), dtype=np.int64), "1-d")):
        with pytest.raises(ValueError, match=text):
            enc(bad)
    emb = SageEncoder(torch.nn.Embedding(3, 5), e, m)
    assert sorted(n for n, _ in emb.named_parameters()) == ["conv.weight", "features.weight"]
    for doc in (SageConv.__doc__, graph_pooling_amd.ops.csr_sample_mean.__doc__):
        assert "hipGraph" in doc and "NaN" in doc and "num_sample" in doc


def test_fused_clip_adam_lays_a_plain_module_out_in_one_flat_buffer():
    """A module without the encoders' flat-buffer protocol (SupervisedGraphSage over a SageEncoder) is wrapped: every
    parameter a view into one fp32 buffer in parameters() order, values kept, re-flattened after a re-bind."""
    from graph_pooling_amd.graphsage import SupervisedGraphSage
    from graph_pooling_amd.optim import FusedClipAdam, _FlatModule
    from graph_pooling_amd.sparse import CsrGraph, SageConv, SageEncoder
    torch.manual_seed(1)
    e = CsrGraph.from_edges(3, [0], [1], "cpu")
    model = SupervisedGraphSage(2, SageEncoder(torch.nn.Embedding(3, 5), e, SageConv(5, 4)))
    before = [p.detach().clone() for p in model.parameters()]
    opt = FusedClipAdam(model, lr=0.01, clip=2.0)
    flat = opt.model
    assert isinstance(flat, _FlatModule) and flat.module is model
    flat._ensure_flat(torch.device("cpu"))
    assert flat._flat.numel() == sum(p.numel() for p in before) and flat._flat.dtype == torch.float32
    off = 0
    for p, b, (o, n, shape) in zip(model.parameters(), before, flat._flat_index):
        assert (o, n, shape) == (off, p.numel(), tuple(p.shape)) and torch.equal(p.detach(), b)
        assert p.data_ptr() == flat._flat.data_ptr() + 4 * o
        off += n
    buf = flat._flat
    flat._ensure_flat(torch.device("cpu"))
    assert flat._flat is buf                                          # nothing re-bound: nothing re-flattened
    model.weight.data = model.weight.data.clone()
    flat._ensure_flat(torch.device("cpu"))
    assert flat._flat is not buf and model.weight.data_ptr() == flat._flat.data_ptr() + 4 * flat._flat_index[0][0]
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()                                                    # no CPU path


def test_csr_sample_mean_refusals_and_the_edgeless_container():
    from graph_pooling_amd import ops
    from graph_pooling_amd.sparse import CsrBatch, CsrGraph
    e = CsrGraph.from_edges(5, [], [], "cpu")
    x = torch.rand(5, 3)
    out = ops.csr_sample_mean(x, e, 10, 7)                            # edgeless, "none": zeros, nothing launched
    assert out.shape == (5, 3) and not out.any() and out.grad_fn is None
    b = CsrBatch.from_edge_lists([2, 3], [[], []], [[], []], "cpu")
    assert ops.csr_sample_mean(x, b, None, 0).shape == (5, 3)
    y, thr, cnt = ops.csr_sample_mean_stats(x, e, 10, 7)
    assert (thr == -1).all() and not cnt.any() and thr.dtype == torch.int64 and cnt.dtype == torch.int32
    none = ops.csr_sample_mean(x, e, 10, 7, nodes=torch.zeros(0, dtype=torch.int32), self_mode="concat")
    assert none.shape == (0, 6)
    g = CsrGraph.from_edges(5, [0, 1], [1, 2], "cpu")
    for k in (0, 65, -3, 1.5, True):
        with pytest.raises(ValueError, match="num_sample must be 1 .. 64 or None"):
            ops.csr_sample_mean(x, g, k, 7)
    for seed in (-1, 1 << 64, 0.5, None):
        with pytest.raises(ValueError, match="seed must be a Python int"):
            ops.csr_sample_mean(x, g, 10, seed)
    with pytest.raises(ValueError, match="self_mode must be"):
        ops.csr_sample_mean(x, g, 10, 7, self_mode="mean")
    with pytest.raises(ValueError, match="expected x"):
        ops.csr_sample_mean(torch.rand(4, 3), g, 10, 7)
    for nodes, text in ((torch.tensor([0, 1]), "int32 tensor"), (torch.tensor([0, 0], dtype=torch.int32), "distinct"),
                        (torch.tensor([5], dtype=torch.int32), "outside 0 .. 4"),
                        (torch.tensor([-1], dtype=torch.int32), "outside 0 .. 4"), ([0, 1], "int32 tensor")):
        with pytest.raises(ValueError, match=text):
            ops.csr_sample_mean(x, g, 10, 7, nodes=nodes)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.csr_sample_mean(x, g, 10, 7)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.csr_sample_mean(x, e, 10, 7, self_mode="gcn")            # edgeless, but the node itself is gathered
    assert ops._sample_args("t", None, (1 << 64) - 1, "gcn") == (0, -1, 1)
    assert ops._sample_args("t", 64, 1 << 63, "concat") == (64, -(1 << 63), 2)
