"""Inputs, fp64 reference and error bounds of the Frobenius link entries (dp_frob_link_* / dp_csr_frob_link_*).

Definition (include/diffpool_hip.h; unpinned by the reference, which has no such term), n_b = num_nodes[b] (absent: n):

    link = sum_b sum_{i,j < n_b} (a_bij - s_bi . s_bj)^2 / sum_b n_b^2

The reference below is this double sum, taken directly in float64 on the fp32 inputs (P = S S^T formed per graph), and
its gradient -2 ((A - P) + (A - P)^T) S / norm.  The kernels evaluate F = T0 - sum_i s_i . w_i + sum_b ||G_b||^2 with
T0 = sum a^2, W = (A + A^T) S, G_b = S_b^T S_b, so that sum_i s_i . w_i = 2 T1, T1 = sum a_ij (s_i . s_j), T2 = sum p^2.

F is a difference of three non-negative sums: the error of any fp32 evaluation scales with T0 + 2 |T1| + T2, not with
F, and near a perfect fit the relative error of F is unbounded.  That is inherent, not a defect.

Bounds (u = 2^-24; counted from the arithmetic of dp_frob_link.hip, not fitted).  D = the largest number of non-zero
terms one row of W sums: entries of row i of A plus entries of row i of A^T (an upper count for a symmetric dense
adjacency, where the two coincide and the kernel adds them first).

Forward.
  * W: c_ij = fl(a_ij + a_ji) rounds once (exact for 0/1); the row sum takes one fma per non-zero term, D roundings (a
    zero term adds exactly nothing); the CSR gather sums the same D terms in fp32 and its beta = 1 pass adds one: at
    most (D + 1) u |W|.
  * row term: fl(s w) rounds once, the sums run in fp64 (2^-53 per step: budgeted as u / 2 of the magnitude):
    (D + 2.5) u on sum s . w = 2 T1.
  * T0: fl(a a) rounds once (exact for 0/1; the CSR count is exact): u T0.
  * T2: G is summed in fp64 from exact products: u / 2 budgeted.
  * T0 - 2 T1 + T2 and the quotient by the normaliser in fp64, rounded to fp32 once: u |F| <= u (T0 + 2 |T1| + T2).
  Total <= C_FWD(D) u (T0 + 2 |T1| + T2) / norm with C_FWD(D) = D + 4.
  total_inout: fl(old + term), one more rounding u |old + term|.

Backward.  d = fl(coef * fl(4 gs - 2 w)), gs = sum_c fma(G_ck, s_c):
  * G rounded to fp32 once, K fma roundings: (K + 1) u on 4 |S| |G|;   * W as above: (D + 1) u on 2 |W|;
  * 4 gs and 2 w are exact, the difference rounds once, coef = fl(dloss / norm) once, the product once: 3 u on both.
  Total <= C_BWD(K, D) u (4 |S| |G| + 2 |W|) |dloss| / norm per element, C_BWD = max(K, D) + 4, with |G| = |S|^T |S| and
  |W| = (|A| + |A^T|) |S|.  accumulate = 1: fl(old + d), one more rounding u |old + d|.
"""
import numpy as np

U = 2.0 ** -24
SLAB = 512               # DP_FROB_LINK_SLAB: global rows per Gram slab
K_CASES = (1, 2, 3, 16, 17, 64, 65, 256)


def c_fwd(D):
    return D + 4.0


def c_bwd(K, D):
    return max(K, D) + 4.0


# ---- inputs
def softmax_rows(rng, rows, K, scale=2.0):
    z = rng.standard_normal((rows, K)) * scale
    z -= z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def random_adj(rng, n, p=0.15, symmetric=True, self_loops=False):
    """0/1 [n, n] float32."""
    a = (rng.random((n, n)) < p)
    if symmetric:
        a = np.triu(a, 1)
        a = a | a.T
    else:
        a = a & ~np.eye(n, dtype=bool)
    if self_loops:
        a = a | np.eye(n, dtype=bool)
    return a.astype(np.float32)


def dense_batch(rng, B, N, nn, p=0.15, symmetric=True, weighted=False, self_loops=False):
    """[B, N, N] float32, zero outside each graph's leading n_b x n_b block; weighted: entries 0.5 / 2 instead of 1."""
    A = np.zeros((B, N, N), dtype=np.float32)
    for b in range(B):
        n = int(nn[b])
        a = random_adj(rng, n, p, symmetric, self_loops)
        if weighted:
            w = np.where(rng.random((n, n)) < 0.5, 0.5, 2.0).astype(np.float32)
            if symmetric:
                w = np.triu(w) + np.triu(w, 1).T
            a = a * w
        A[b, :n, :n] = a
    return A


def ring_lattice_csr(n):
    """i <-> i +- 1, i +- 2 (mod n), n >= 5: (indptr, indices) int32, rows sorted."""
    i = np.arange(n, dtype=np.int64)[:, None]
    cols = np.sort((i + np.array([-2, -1, 1, 2])[None, :]) % n, axis=1)
    return (np.arange(n + 1, dtype=np.int64) * 4).astype(np.int32), cols.reshape(-1).astype(np.int32)


def csr_of(a):
    """Dense [n, n] -> (indptr, indices) int32 of the non-zero entries."""
    r, c = np.nonzero(a)
    indptr = np.zeros(a.shape[0] + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr).astype(np.int32), c.astype(np.int32)


def cliques_one_hot(sizes, K):
    """Disjoint cliques WITH self loops and the one-hot assignment that fits them: A = S S^T exactly."""
    n = int(sum(sizes))
    S = np.zeros((n, K), dtype=np.float32)
    r = 0
    for c, m in enumerate(sizes):
        S[r:r + m, c % K] = 1.0
        r += m
    # two cliques sharing a column would break the fit: the caller keeps len(sizes) <= K
    assert len(sizes) <= K
    return (S @ S.T).astype(np.float32), S


def quarter_grid(rng, rows, K):
    """S on the grid of multiples of 1/4 with row sums <= 1: every product and sum the kernels form is exact in fp32."""
    S = np.zeros((rows, K), dtype=np.float32)
    for i in range(rows):
        for _ in range(4):
            if rng.random() < 0.8:
                S[i, int(rng.integers(K))] += 0.25
    return S


# ---- the fp64 reference (one graph: a [n, n], s [n, K], both already cut to the valid rows)
def graph_terms(a, s):
    """(F, T0, T1, T2, dF/dS, |grad magnitude|, D) in float64."""
    a = a.astype(np.float64)
    s = s.astype(np.float64)
    p = s @ s.T
    r = a - p
    F = float((r * r).sum())
    T0, T1, T2 = float((a * a).sum()), float((a * p).sum()), float((p * p).sum())
    dS = -2.0 * ((r + r.T) @ s)
    sa, aa = np.abs(s), np.abs(a)
    mag = 4.0 * (sa @ (sa.T @ sa)) + 2.0 * ((aa + aa.T) @ sa)
    nz = (a != 0)
    D = int((nz.sum(axis=1) + nz.sum(axis=0)).max()) if a.size else 0
    return F, T0, T1, T2, dS, mag, D


def batch_ref(graphs, norm=None):
    """graphs: list of (a [n_b, n_b], s [n_b, K]).  Returns dict: loss, mag = (T0 + 2|T1| + T2) / norm, norm, D, and per
    graph dS / norm and the gradient magnitude / norm (for dloss = 1)."""
    terms = [graph_terms(a, s) for a, s in graphs]
    if norm is None:
        norm = float(sum(s.shape[0] ** 2 for _, s in graphs))
    F = sum(t[0] for t in terms)
    mag = sum(t[1] + 2.0 * abs(t[2]) + t[3] for t in terms)
    return dict(loss=F / norm, F=F, mag=mag / norm, norm=norm, D=max(t[6] for t in terms),
                T=(sum(t[1] for t in terms), sum(t[2] for t in terms), sum(t[3] for t in terms)),
                dS=[t[4] / norm for t in terms], dmag=[t[5] / norm for t in terms])


def fwd_bound(ref):
    return c_fwd(ref["D"]) * U * ref["mag"]


def bwd_bound(ref, K, b, dloss=1.0):
    return c_bwd(K, ref["D"]) * U * ref["dmag"][b] * abs(dloss)


# ---- an fp32 restatement of the decomposed evaluation (numpy; tests/test_frob_link_cpu.py)
def fp32_restatement(graphs, norm=None):
    """The kernels' arithmetic in numpy: W and the products s w, a a in float32, every sum of those and G in float64,
    the quotient in float64, rounded to float32 once."""
    t0 = t1 = t2 = 0.0
    if norm is None:
        norm = float(sum(s.shape[0] ** 2 for _, s in graphs))
    for a, s in graphs:
        a32, s32 = a.astype(np.float32), s.astype(np.float32)
        c = (a32 + a32.T).astype(np.float32)
        w = np.zeros_like(s32)
        for j in range(a32.shape[0]):                           # ascending j, one rounding per term
            w = (w + c[:, j:j + 1] * s32[j:j + 1, :]).astype(np.float32)
        t1 += float((s32 * w).astype(np.float32).astype(np.float64).sum())
        t0 += float((a32 * a32).astype(np.float32).astype(np.float64).sum())
        g = s32.astype(np.float64).T @ s32.astype(np.float64)
        t2 += float((g * g).sum())
    return float(np.float32((t0 - t1 + t2) / norm))


# ---- defects the forward bound must tell from rounding, float64 throughout
FAULTS = ("dropped_last_row", "dropped_edge", "t1_once", "divisor_BN2", "no_diagonal", "neighbour_leaks_into_G")


def faulty_loss(graphs, fault, N=None):
    """The term as an evaluation with the named defect would return it; graphs as in batch_ref; N: the padded size the
    divisor defect uses."""
    norm = float(sum(s.shape[0] ** 2 for _, s in graphs))
    gs = [(a.astype(np.float64), s.astype(np.float64)) for a, s in graphs]
    if fault == "no_diagonal":
        F = 0.0
        for a, s in gs:
            r = a - s @ s.T
            np.fill_diagonal(r, 0.0)
            F += (r * r).sum()
        return F / norm
    if fault == "divisor_BN2":
        return sum(graph_terms(a, s)[0] for a, s in graphs) / float(len(graphs) * N * N)
    t0 = t1 = t2 = 0.0
    for k, (a, s) in enumerate(gs):
        if fault == "dropped_last_row" and k == len(gs) - 1:
            a, s = a[:-1, :-1], s[:-1]
        if fault == "dropped_edge" and k == 0:
            a = a.copy()
            i, j = np.argwhere(np.abs(a) == np.abs(a).max())[0]       # the first of the heaviest entries
            a[i, j] = 0.0
        g = s.T @ s
        if fault == "neighbour_leaks_into_G" and k + 1 < len(gs):
            nxt = gs[k + 1][1][:1]
            g = g + nxt.T @ nxt
        t0 += (a * a).sum()
        t1 += (s * (a @ s)).sum() if fault == "t1_once" else (s * ((a + a.T) @ s)).sum() / 2.0
        t2 += (g * g).sum()
    return (t0 - (t1 if fault == "t1_once" else 2.0 * t1) + t2) / norm
