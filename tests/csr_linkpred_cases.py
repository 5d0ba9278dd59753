"""Cases, inputs, fp64 reference and counted error bounds of the CSR link-prediction loss (dp_csr_linkpred_loss_*,
dp_csr_linkpred_batch_loss_* and their _w twins; dp_csr_linkpred.hip: k_csr_link_dense_fwd / _bwd, k_csr_link_reduce,
k_csr_link_edge_fwd / _bwd, k_csr_link_final).

Definition (include/diffpool_hip.h, N4), eps = 1e-7, a_ij the stored value (1 for the plain entries, 0 where nothing
is stored), per graph of n_b rows:

    raw = S S^T,  p = min(raw, 1),  l = -a ln(p + eps) - (1 - a) ln(1 - p + eps),
    loss = sum_b sum l / sum_b n_b^2,   dS = dloss d loss / dS (added to dS under accumulate).

The reference is this formula in float64 on the fp32 inputs and the dense weighted matrix, one graph at a time
(tests/csr_weights_cases.link_terms / link_ref), with the bound counted there from these kernels' arithmetic.  Two
things are said to it that the older inputs never needed: the gate of torch.minimum (1/2 where raw == 1 exactly, 0
above), and which P entries are exact in fp32 (both rows one-hot with value 1, or S on the quarter grid): there the
(K + 4) u p term is 0, so that a planted tie (1 / (1 - p + eps) = 1e7) does not blow the bound up.

qualification.  The bound is first order in the error of p.  A row of the table qualifies only when every inexact P
  entry has 1 - p >= 64 (K + 1) u in float64 (then the neglected second-order term is under 1/64 of the first and no
  fp32 raw reaches 1 where the fp64 one is below it) and when the direct fp32 formula (torch fp32 autograd on the
  densified graph) itself meets the bound.  A row that does not gets another input, never a wider bound; every row of
  this table is held to the counted bound.
accumulate.  The kernels add into dS twice: the dense term (k_csr_link_dense_bwd, or k_csr_link_reduce under a split)
  forms fl(old + dense), the edge kernel then fl(. + edge).  The bound gains u |old + d| for the last rounding; the
  first one is u |old + dense| <= u (|old| + |dense|).  prior() therefore draws old element by element from
  [1, 2] x the magnitude sum_c |G_rc| |s_ck| |dloss| / norm of that element of dS: u |old| is then at most 2 u of
  absolute terms of which the bound already counts n + K + 8 (dense) and deg + 8 (edge) roundings, and a result that
  ignores accumulate is still wrong by |old| >= that magnitude, some 1e5 bounds.  An old of the size of max|dS| in every
  element would put two roundings of |old| on elements whose own terms are far smaller, beside a bound of one.

The non-split walk over several column tiles (splits == 1 with col_tiles > 1) needs ceil(n / 64) >= 512, n >= 32 705: it
stays with the 65 536-row test of tests/test_gpu_csr_linkpred.py.

`python -m tests.csr_linkpred_cases` prints the table with each row's plan.
"""
import collections
import functools
import zlib

import numpy as np
import torch

from tests import csr_weights_cases as WC
from tests.linkpred_cases import quarter_grid

U = WC.U
EPS = WC.EPS
K_MAX = 256
K_EDGES = (1, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 256)
N_EDGES = (1, 7, 63, 64, 65, 127, 128, 129, 131)
K_VEC16 = (4, 20, 64, 68, 128, 132, 256)          # 16-byte edge forms: partial and full last chunks of <4,1> <4,2> <4,4>
K_VEC4 = (1, 16, 17, 63, 65, 255)                 # 4-byte edge forms <1,1> <1,4> <1,16>
PLANTED_COUNTS = (0, 1, 3, 4, 5, 8, 9)            # stored entries per row: the 4-way unroll and its tail
PLANT_MIN_N = 32                                  # graphs of at least this many rows carry the planted rows
TIE_ROWS = (16, 17, 20, 21)                       # one-hot on one cluster: raw == 1 exactly on and off the diagonal
PLAN_FIELDS = ("kt", "T", "pairs", "Z", "n_dense", "n_edge", "cw", "col_tiles", "splits", "split_tiles", "fwd_vec",
               "fwd_nch", "bwd_vec", "bwd_nch", "fwd_lds", "bwd_lds")
Plan = collections.namedtuple("Plan", PLAN_FIELDS)


# ------------------------------------------------------------------ the plan, restated (dp_csr_linkpred_plan)
def _cdiv(a, b):
    return -(-a // b)


def _edge_form(v4, K):
    if v4:
        return 4, (1 if K <= 64 else 2 if K <= 128 else 4)
    return 1, (1 if K <= 16 else 4 if K <= 64 else 16)


def plan(n, K, lds, ldds, s_mis=0, ds_mis=0):
    """The 16 ints of dp_csr_linkpred_plan for one graph, as a Plan."""
    kt16 = _cdiv(K, 16)
    kt = next((s for s in (1, 2, 3, 4, 6, 8, 12, 16) if kt16 <= s), 0)
    assert kt, "K > 256 has no plan"
    T = _cdiv(n, 64)
    pairs = (T + 1) // 2
    Z = max(1, min(T, _cdiv(1024, pairs)))
    cw = 32 if kt >= 12 else 64
    col_tiles = _cdiv(n, cw)
    want = max(1, min(col_tiles, _cdiv(512, T)))
    split_tiles = _cdiv(col_tiles, want)
    splits = _cdiv(col_tiles, split_tiles)
    v4f = K % 4 == 0 and lds % 4 == 0 and not s_mis
    v4b = v4f and ldds % 4 == 0 and not ds_mis
    kp = kt * 16 + 2
    return Plan(kt, T, pairs, Z, pairs * Z, _cdiv(n, 16), cw, col_tiles, splits, split_tiles, *_edge_form(v4f, K),
                *_edge_form(v4b, K), 4 * 2 * 64 * kp, 4 * ((64 + cw) * kp + 64 * (cw + 4)))


def bwd_class(p):
    if p.col_tiles == 1:
        return f"one_tile_cw{p.cw}"
    assert p.splits > 1, "the non-split multi-tile walk (n >= 32 705) is not in this table"
    if p.split_tiles == 1:
        return f"split_all_cw{p.cw}"
    return f"split_{'even' if p.col_tiles % p.split_tiles == 0 else 'ragged'}_cw{p.cw}"


def chunk_full(vec, nch, K):
    """True when the last 16-lane chunk of the edge form is full (K == NCH * 16 * VEC)."""
    return K == nch * 16 * vec


# ------------------------------------------------------------------ the case table
# sizes: rows per graph (one entry: the single-graph entries unless batch);  spad / dpad: lds = K + spad, ldds = K + dpad;
# s_shift / ds_shift: floats by which S / dS start off a 16-byte boundary;  skind: softmax, ties (softmax with one-hot
# pairs planted), grid (multiples of 1/4, row sums up to 1.5);  weighted: stored values in (0.1, 2), through the _w entries
Case = collections.namedtuple("Case", "name sizes K directed loops skind dloss acc spad dpad s_shift ds_shift batch weighted")


def _c(name, sizes, K, directed=False, loops=False, skind="softmax", dloss=None, acc=0, spad=0, dpad=0, s_shift=0,
       ds_shift=0, batch=False, weighted=False):
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    return Case(name, tuple(sizes), K, directed, loops, skind, dloss, acc, spad, dpad, s_shift, ds_shift,
                batch or len(sizes) > 1, weighted)


CASES = [
    # every K tier edge, each at another n / direction / scalar combination
    _c("k1_n1", 1, 1),
    _c("k16_n7_ldsodd", 7, 16, directed=True, dloss=-0.6, acc=1, spad=3, dpad=3),
    _c("k17_n63", 63, 17),
    _c("k32_n64", 64, 32, directed=True, dloss=1.7),
    _c("k33_n65", 65, 33, acc=1),
    _c("k48_n100_w", 100, 48, directed=True, weighted=True),
    _c("k49_n127", 127, 49, dloss=1.7),
    _c("k64_n128", 128, 64, directed=True, dloss=-0.6),
    _c("k65_n129", 129, 65, acc=1),
    _c("k96_n131_grid", 131, 96, skind="grid"),
    _c("k97_n100", 100, 97, directed=True),
    _c("k128_n129", 129, 128, loops=True),
    _c("k129_n131", 131, 129, directed=True, acc=1),
    _c("k192_n127", 127, 192, dloss=1.7),
    _c("k193_n65", 65, 193, directed=True, acc=1),
    _c("k256_n7", 7, 256),
    _c("k256_n32_smis", 32, 256, acc=1, spad=4, s_shift=1, dloss=1.7),
    # edge forms: partial last chunks of the 16-byte forms, the 4-byte tiers, and K % 4 == 0 forced scalar
    _c("k4_n131_ties", 131, 4, skind="ties", loops=True),
    _c("k20_n128_ties", 128, 20, directed=True, skind="ties", dloss=1.7, acc=1),
    _c("k68_n63", 63, 68, loops=True),
    _c("k132_n64", 64, 132, dloss=-0.6),
    _c("k63_n129", 129, 63, directed=True),
    _c("k255_n65", 65, 255),
    _c("k64_n127_ldsodd", 127, 64, spad=3, dpad=3),
    _c("k128_n100_smis", 100, 128, directed=True, spad=4, s_shift=1),
    _c("k20_n65_lddsodd", 65, 20, dpad=3, dloss=1.7),
    _c("k128_n131_dsmis", 131, 128, acc=1, dpad=4, ds_shift=1),
    _c("k8_n100_grid", 100, 8, directed=True, skind="grid", dloss=-0.6, acc=1),
    # the forward's column loop runs twice in a workgroup (Z < T)
    _c("fwd2_k8_n2881", 2881, 8),
    _c("fwd2_k40_n2881", 2881, 40, directed=True, acc=1, dloss=1.7),
    # backward splits of two column tiles: even and ragged, both tile widths, both accumulate values
    _c("even64_n1473", 1473, 50),
    _c("even64_n1536_acc", 1536, 17, directed=True, acc=1),
    _c("ragged64_n1537", 1537, 20, dloss=-0.6),
    _c("ragged64_n1600_acc", 1600, 33, acc=1),
    _c("even32_n1057", 1057, 193),
    _c("even32_n1088_acc", 1088, 256, directed=True, acc=1, dloss=1.7),
    _c("ragged32_n1025", 1025, 177, directed=True),
    _c("ragged32_n1056_acc", 1056, 192, acc=1),
    # batches: graphs of different plan classes, the largest not first
    _c("batch_k20", [7, 1537, 1, 65], 20, dloss=1.7),
    _c("batch_k50_dir_w", [65, 1, 131, 7], 50, directed=True, weighted=True, acc=1),
    _c("batch_k193", [33, 1025, 1, 64], 193, directed=True, dloss=-0.6),
]
REFUSED_K = K_MAX + 1


def by_name(name):
    return next(c for c in CASES if c.name == name)


def offsets(c):
    return np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int32)


def strides(c):
    return c.K + c.spad, c.K + c.dpad


def graph_plans(c):
    """The plan of every graph of the row, on the pointers the entries hand to the launchers: graph b's S starts
    s_shift + off[b] * lds floats off a 16-byte boundary."""
    lds, ldds = strides(c)
    off = offsets(c)
    return [plan(int(n), c.K, lds, ldds, (c.s_shift + int(off[b]) * lds) % 4 != 0,
                 (c.ds_shift + int(off[b]) * ldds) % 4 != 0) for b, n in enumerate(c.sizes)]


def plan_args(c):
    lds, ldds = strides(c)
    off = offsets(c)
    return [(int(n), c.K, lds, ldds, int((c.s_shift + int(off[b]) * lds) % 4 != 0),
             int((c.ds_shift + int(off[b]) * ldds) % 4 != 0)) for b, n in enumerate(c.sizes)]


# ------------------------------------------------------------------ inputs
def _adjacency(rng, n, directed, loops, ties):
    """bool [n, n].  n >= PLANT_MIN_N: node 0 isolated; rows 1..6 store exactly PLANTED_COUNTS[1:] entries and (directed)
    columns 8..13 are stored in exactly that many rows, all towards nodes >= 16, which carry the random edges."""
    A = np.zeros((n, n), dtype=bool)
    if n == 1:
        A[0, 0] = True                              # the CSR arrays of a lone graph must not be empty
        return A
    if n < PLANT_MIN_N:
        R = rng.random((n, n)) < 0.4
        R[0, :] = R[:, 0] = False
        np.fill_diagonal(R, False)
        A = R | R.T if not directed else R
        A[1, 1] = True                              # never empty
        return A
    m = n - 16
    R = rng.random((m, m)) < min(0.5, 5.0 / m)
    np.fill_diagonal(R, False)
    A[16:, 16:] = R | R.T if not directed else R
    for r, cnt in zip(range(1, 7), PLANTED_COUNTS[1:]):
        A[r, 16 + rng.choice(m, cnt, replace=False)] = True
    if directed:
        for col, cnt in zip(range(8, 14), PLANTED_COUNTS[1:]):
            A[16 + rng.choice(m, cnt, replace=False), col] = True
    else:
        A = A | A.T
    if loops:
        A[[18, 19, 25], [18, 19, 25]] = True
    if ties:                                        # tied pairs on and off the diagonal, on an edge and on a non-edge
        t0, t1, t2, t3 = TIE_ROWS
        A[t0, t0], A[t1, t1], A[t2, t2], A[t3, t3] = True, False, False, False
        A[t0, t1] = A[t1, t0] = True
        A[t2, t3] = A[t3, t2] = False
    return A


def _csr(M):
    """(indptr, indices, rows) int64 of the non-zeros of M, row by row."""
    r, cidx = np.nonzero(M)
    ip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M.shape[0]))])
    return ip, cidx, r


def _assign(rng, c, n):
    K = c.K
    if c.skind == "grid":
        return quarter_grid(rng, n, K)
    S = WC.assign_rows(rng, n, K)
    if c.skind == "ties":
        assert n >= PLANT_MIN_N and K >= 2
        S[list(TIE_ROWS), :] = 0.0
        S[list(TIE_ROWS), min(2, K - 1)] = 1.0
    return S


def build(c):
    """dict: S [n_total, K] float32; graphs: per graph dict(n, a float64 [n, n] of stored values, mask bool, ip / ix / val
    and ipt / ixt / valt: the graph's own CSR and that of its transpose, local indices); the concatenated batch arrays
    indptr, indices (local), values and their _t twins (None for an undirected graph: the forward's arrays serve)."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    graphs, Ss = [], []
    for n in c.sizes:
        A = _adjacency(rng, n, c.directed, c.loops, c.skind == "ties")
        if c.weighted:
            w = rng.uniform(0.1, 2.0, (n, n))
            if not c.directed:
                w = np.triu(w) + np.triu(w, 1).T
            w = w.astype(np.float32).astype(np.float64)
        else:
            w = np.ones((n, n))
        a = np.where(A, w, 0.0)
        ip, ix, _ = _csr(A)
        ipt, ixt, _ = _csr(A.T)
        graphs.append(dict(n=n, a=a, mask=A, ip=ip, ix=ix, val=a[np.nonzero(A)].astype(np.float32),
                           ipt=ipt, ixt=ixt, valt=a.T[np.nonzero(A.T)].astype(np.float32)))
        Ss.append(_assign(rng, c, n))

    def cat(key_ip, key_ix, key_v):
        ip = [np.zeros(1, np.int64)]
        base = 0
        for g in graphs:
            ip.append(g[key_ip][1:] + base)
            base += int(g[key_ip][-1])
        return (np.concatenate(ip).astype(np.int32), np.concatenate([g[key_ix] for g in graphs]).astype(np.int32),
                np.concatenate([g[key_v] for g in graphs]).astype(np.float32))
    indptr, indices, values = cat("ip", "ix", "val")
    out = dict(S=np.concatenate(Ss).astype(np.float32), graphs=graphs, indptr=indptr, indices=indices, values=values,
               indptr_t=None, indices_t=None, values_t=None, off=offsets(c))
    if c.directed:
        out["indptr_t"], out["indices_t"], out["values_t"] = cat("ipt", "ixt", "valt")
    return out


def exact_entries(c, S):
    """bool [n, n]: the P entries whose fp32 value is the float64 one."""
    n = S.shape[0]
    if c.skind == "grid":
        return np.ones((n, n), dtype=bool)
    onehot = ((S != 0).sum(axis=1) <= 1) & np.isin(S, (0.0, 1.0)).all(axis=1)
    return onehot[:, None] & onehot[None, :]


# ------------------------------------------------------------------ the fp64 reference, the bound, the fp32 formula
def reference(c, inp):
    """WC.link_ref of the row (loss, loss_bound, dS, dS_bound over all rows, dloss applied) with: mag (the absolute
    terms of every element of dS, for prior()), margin (the smallest 1 - p of an inexact entry), ties / above / below."""
    off = inp["off"]
    tuples, mags = [], []
    info = dict(margin=float("inf"), ties=0, above=0, below=0, ties_edge=0, ties_nonedge=0)
    for b, g in enumerate(inp["graphs"]):
        S = inp["S"][off[b]:off[b + 1]].astype(np.float64)
        ex = exact_entries(c, S)
        tuples.append((g["a"], S, np.diff(g["ip"]), np.diff(g["ipt"]), ex))
        raw = S @ S.T
        p = np.minimum(raw, 1.0)
        gate = np.where(raw < 1.0, 1.0, np.where(raw == 1.0, 0.5, 0.0))
        coef = gate * (1.0 / (1.0 - p + EPS) + np.abs(g["a"]) * (1.0 / (p + EPS) + 1.0 / (1.0 - p + EPS)))
        mags.append((coef + coef.T) @ np.abs(S))
        if (~ex).any():
            info["margin"] = min(info["margin"], float((1.0 - p)[~ex].min()))
        info["ties"] += int((raw == 1).sum())
        info["ties_edge"] += int(((raw == 1) & g["mask"]).sum())
        info["ties_nonedge"] += int(((raw == 1) & ~g["mask"]).sum())
        info["above"] += int((raw > 1).sum())
        info["below"] += int((raw < 1).sum())
    dl = 1.0 if c.dloss is None else float(c.dloss)
    ref = WC.link_ref(tuples, dl)
    nn = float(sum(n * n for n in c.sizes))
    ref.update(info, mag=np.concatenate(mags) * abs(dl) / nn, dl=dl, nn=nn)
    return ref


def qualifies(c, ref):
    return ref["margin"] >= 64 * (c.K + 1) * U


def formula32(c, inp):
    """The direct fp32 formula: torch fp32 autograd on the densified graph -> (loss, dS [n_total, K] float64)."""
    off = inp["off"]
    nn = float(sum(n * n for n in c.sizes))
    dl = 1.0 if c.dloss is None else float(c.dloss)
    tot, grads = 0.0, []
    for b, g in enumerate(inp["graphs"]):
        s = torch.from_numpy(inp["S"][off[b]:off[b + 1]]).clone().requires_grad_(True)
        a = torch.from_numpy(g["a"].astype(np.float32))
        p = torch.minimum(s @ s.t(), torch.ones(()))
        t = (-a * torch.log(p + EPS) - (1 - a) * torch.log(1 - p + EPS)).sum()
        (gr,) = torch.autograd.grad(t, s)
        tot += float(t.detach())
        grads.append((gr * np.float32(dl / nn)).double().numpy())
    return np.float32(tot / nn), np.concatenate(grads)


def prior(c, ref):
    """What dS holds before an accumulating call (see "accumulate" above): [n_total, K] float32."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + 1)
    shape = ref["mag"].shape
    return (ref["mag"] * rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape)).astype(np.float32)


def output(d, old=None):
    """float32 [n_total, K] of a result d (float64, without the prior) as a correct entry leaves dS."""
    return (d if old is None else d + old.astype(np.float64)).astype(np.float32)


def compare(c, ref, loss, dS, old=None):
    """loss (float) and dS [n_total, K] as the entry left it against `ref`: dict(fwd, bwd: largest |error| / bound,
    problems)."""
    problems = []
    fr = abs(float(loss) - ref["loss"]) / ref["loss_bound"]
    if not np.isfinite(float(loss)) or fr > 1.0:
        problems.append(f"loss {float(loss)!r} vs {ref['loss']!r}: {fr:.3f} of the bound")
    want, tol = ref["dS"], ref["dS_bound"]
    if old is not None:
        want = want + old.astype(np.float64)
        tol = tol + U * np.abs(want)
    got = np.asarray(dS, dtype=np.float64)
    if not np.isfinite(got).all():
        return dict(fwd=fr, bwd=float("inf"), problems=problems + ["non-finite dS"])
    ratio = np.abs(got - want) / np.maximum(tol, 1e-300)
    br = float(ratio.max())
    if br > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        problems.append(f"dS{i} = {got[i]!r} vs {want[i]!r}: {br:.3f} of the bound")
    return dict(fwd=fr, bwd=br, problems=problems)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(case, inputs, reference), built once per process and shared: treat as read-only."""
    c = by_name(name)
    inp = build(c)
    return c, inp, reference(c, inp)


# ------------------------------------------------------------------ planted defects: the wrong answers they would give
FAULTS = ("offdiag_once", "last_col_tile_dropped", "last_split_dropped", "tail_edges_skipped", "factor2_missing",
          "transposed_ignored", "tie_gate_1", "above_gate_1", "chunk_duplicates", "accumulate_ignored", "dloss_ignored",
          "batch_partial_offset")
# the row each defect has to be caught on
FAULT_ROW = {"offdiag_once": "k49_n127", "last_col_tile_dropped": "k33_n65", "last_split_dropped": "ragged64_n1537",
             "tail_edges_skipped": "k17_n63", "factor2_missing": "k49_n127", "transposed_ignored": "k32_n64",
             "tie_gate_1": "k4_n131_ties", "above_gate_1": "k96_n131_grid", "chunk_duplicates": "k68_n63",
             "accumulate_ignored": "k33_n65", "dloss_ignored": "k32_n64", "batch_partial_offset": "batch_k20"}


def _walk(S, raw, ip, ix, val, K, form, fault, gate_of):
    """The edge kernels' walk over one CSR: (sum of the forward terms, [n, K] sum_j c_ij s_j) in float64."""
    n = S.shape[0]
    cnt = np.diff(ip)
    rows = np.repeat(np.arange(n), cnt)
    keep = np.ones(rows.size, dtype=bool)
    if fault == "tail_edges_skipped":               # only whole groups of four are walked
        keep = (np.arange(rows.size) - ip[rows]) < 4 * (cnt[rows] // 4)
    rows, cols, w = rows[keep], ix[keep], val[keep].astype(np.float64)
    r = raw[rows, cols]
    vec, nch = form
    if fault == "chunk_duplicates" and vec == 4:    # lanes past K read columns K-4 .. K-1 again, unmasked
        extra = nch * 16 - K // 4
        r = r + extra * (S[rows, K - 4:] * S[cols, K - 4:]).sum(axis=1)
    p = np.minimum(r, 1.0)
    fsum = float((w * (-np.log(p + EPS) + np.log(1.0 - p + EPS))).sum())
    coef = w * gate_of(r) * (-1.0 / (p + EPS) - 1.0 / (1.0 - p + EPS))
    out = np.zeros_like(S)
    np.add.at(out, rows, coef[:, None] * S[cols])
    return fsum, out


def emulate(c, inp, fault=None, old=None):
    """The decomposed evaluation the kernels perform (dense term over the tile walk, edge term over the CSR lists), in
    float64, with one planted defect: (loss, dS as it would be left).  fault None reproduces the reference."""
    off = inp["off"]
    nn = float(sum(n * n for n in c.sizes))
    dl = 1.0 if (c.dloss is None or fault == "dloss_ignored") else float(c.dloss)

    def gate_of(r):
        return np.where(r < 1.0, 1.0, np.where(r == 1.0, 1.0 if fault == "tie_gate_1" else 0.5,
                                                1.0 if fault == "above_gate_1" else 0.0))
    sums, ds = [], []
    for b, (g, pl) in enumerate(zip(inp["graphs"], graph_plans(c))):
        n = g["n"]
        S = inp["S"][off[b]:off[b + 1]].astype(np.float64)
        raw = S @ S.T
        p = np.minimum(raw, 1.0)
        tile = np.arange(n) // 64
        Wt = np.ones((n, n))
        if fault == "offdiag_once":                 # tile (tr, tc), tr < tc, stands for (tc, tr) too: counted once
            Wt[tile[:, None] > tile[None, :]] = 0.0
        colmask = np.ones(n)
        if fault == "last_col_tile_dropped":
            assert n % 64 and pl.T > 1
            Wt[np.maximum(tile[:, None], tile[None, :]) == pl.T - 1] = 0.0
            colmask[(pl.col_tiles - 1) * pl.cw:] = 0.0
        if fault == "last_split_dropped":
            assert pl.splits > 1
            colmask[(pl.splits - 1) * pl.split_tiles * pl.cw:] = 0.0
        dense_sum = float((Wt * -np.log(1.0 - p + EPS)).sum())
        dense_d = ((2.0 * gate_of(raw) / (1.0 - p + EPS)) * colmask[None, :]) @ S
        fs, ed = _walk(S, raw, g["ip"], g["ix"], g["val"], c.K, (pl.bwd_vec, pl.bwd_nch), fault, gate_of)
        if fault == "chunk_duplicates":
            fs = _walk(S, raw, g["ip"], g["ix"], g["val"], c.K, (pl.fwd_vec, pl.fwd_nch), fault, gate_of)[0]
        if c.directed:
            if fault != "transposed_ignored":
                ed = ed + _walk(S, raw, g["ipt"], g["ixt"], g["valt"], c.K, (pl.bwd_vec, pl.bwd_nch), fault, gate_of)[1]
        else:
            ed = ed * (1.0 if fault == "factor2_missing" else 2.0)
        sums.append(dense_sum + fs)
        ds.append((dense_d + ed) * (dl / nn))
    if fault == "batch_partial_offset":             # graph 1's partials are read where graph 0's lie
        assert len(sums) > 1
        sums[1] = sums[0]
    d = np.concatenate(ds)
    return sum(sums) / nn, output(d, None if fault == "accumulate_ignored" else old)


# ------------------------------------------------------------------ recorded results
def anchor_text(rows):
    """profiles/csr_linkpred_fp64_anchor.txt from {name: (class, plan, acc, fwd, bwd, f32 fwd, f32 bwd)}."""
    lines = ["# tests/test_gpu_csr_linkpred_matrix.py on an MI355X (gfx950): largest |error| / bound per row against the fp64",
             "# reference (bounds: tests/csr_weights_cases.link_terms as tests/csr_linkpred_cases.py calls it, counted,",
             "# u = 2^-24).  class and plan (KT, forward T x Z, backward CW x col_tiles x splits x split_tiles, forward and",
             "# backward edge form VEC.NCH) are those of the row's largest graph as dp_csr_linkpred_plan answered them;",
             "# formula32: the same ratios of the direct fp32 formula (torch, CPU) on that input.",
             f"{'row':<22}{'class':<19}{'plan':<34}{'acc':>4}{'loss':>9}{'dS':>9}{'f32 loss':>10}{'f32 dS':>9}"]
    worst = [0.0] * 4
    for name in [c.name for c in CASES if c.name in rows]:
        cls, pl, acc, *v = rows[name]
        worst = [max(a, b) for a, b in zip(worst, v)]
        lines.append(f"{name:<22}{cls:<19}{pl:<34}{acc:>4}{v[0]:>9.4f}{v[1]:>9.4f}{v[2]:>10.4f}{v[3]:>9.4f}")
    lines.append(f"{'largest':<79}{worst[0]:>9.4f}{worst[1]:>9.4f}{worst[2]:>10.4f}{worst[3]:>9.4f}")
    return "\n".join(lines) + "\n"


def plan_text(p):
    return (f"kt{p.kt} f{p.T}x{p.Z} b{p.cw}x{p.col_tiles}x{p.splits}x{p.split_tiles} "
            f"e{p.fwd_vec}.{p.fwd_nch}/{p.bwd_vec}.{p.bwd_nch}")


def main_plan(c):
    """The plan of the row's largest graph."""
    return graph_plans(c)[int(np.argmax(c.sizes))]


if __name__ == "__main__":
    for c in CASES:
        p = main_plan(c)
        print(f"{c.name:<22}{str(c.sizes):<22}K={c.K:<5}{bwd_class(p):<19}{plan_text(p)}")
