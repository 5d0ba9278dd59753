"""Case table, fp64 reference and error bound of the assignment-entropy entries (dp_assign_entropy_fwd / _bwd).

Definition (include/diffpool_hip.h), eps = float32(1e-15) added in fp32, n_b = num_nodes[b] (absent: n):

    E          = ( sum_b sum_{i<n_b} sum_k -s ln(s + eps) ) / sum_b n_b
    dE/ds_bik  = -( ln(s + eps) + s / (s + eps) ) / sum_b n_b      (i < n_b; 0 for i >= n_b)

The reference evaluates these formulas in float64 on the fp32 S.

Bound (u = 2^-24; derived from the kernel's arithmetic in dp_assign_ent.hip, not fitted)

Forward.  A term is t = fl(s * logf(x)), x = fl(s + eps):
  * x = (s + eps)(1 + d), |d| <= u, moves ln x by at most u ABSOLUTE, so the term by s u;
  * logf: HIP documents 1 ulp; 2 ulp are budgeted: 4 u |ln x| relative to the logarithm, 4 u |s ln| on the term;
  * the product rounds once: u |s ln|.
  From there on every sum runs in fp64 (lane, workgroup tree, the partials): at most rows * K * 2^-53 relative, under
  2^-29 for the largest case here — budgeted as u / 2 of the magnitude.  The quotient by the normaliser is formed in
  fp64 and rounded to fp32 once: u |E| <= u sum|s ln| / norm.
  Total: u (sum s + 6.5 sum|s ln|) / norm  <=  C_FWD u (sum|s ln(s+eps)| + sum s) / norm with C_FWD = 7.
  The path does not grow with the shape, so one constant serves every case.

Backward.  d = fl(fl(L + q) * coef), L = logf(x), q = fl(s / x), coef = fl(-fl(g w) / fl(norm)):
  * L: u (from x) + 4 u |ln|;   * q <= 1: the division is correctly rounded, u, and x's rounding moves it by u: 2 u;
  * the sum rounds once: u (|ln| + 1);   * coef: three roundings, 3 u (|ln| + 1);   * the product: u (|ln| + 1).
  Total u (9 |ln| + 8) |coef|  <=  C_BWD u (|ln(s+eps)| + 1) |w g| / norm with C_BWD = 10 (second-order terms in the
  slack).  With accumulate = 1 the result is fl(old + d): one more rounding, u |old + d|, added to the bound there.
"""
import numpy as np

U = 2.0 ** -24
EPS = np.float64(np.float32(1e-15))
C_FWD = 7.0
C_BWD = 10.0

# launch geometry the table below leans on (dp_assign_ent.hip): 256 threads, at most 2048 workgroups
THREADS, MAX_BLOCKS = 256, 2048


def pick(K, aligned16):
    """(lanes per row, quad) as assign_ent_pick answers: aligned16 = pointers 16-byte aligned and leading dimensions
    multiples of 4."""
    quad = bool(aligned16 and K % 4 == 0)
    per = 4 if quad else 1
    return (4 if K <= 4 * per else 16 if K <= 16 * per else 64), quad


def rows_per_sweep(K, aligned16):
    return MAX_BLOCKS * (THREADS // pick(K, aligned16)[0])


# ---- shapes of the GPU op test: (B, n, K, kind)
SMALL = [(B, n, K) for B in (1, 3) for n in (1, 7, 129) for K in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)]
# the strided loop above one visit per row (K > 256 with 16-byte lanes, K > 64 without)
LOOP = [(2, 40, 1024), (2, 5, 1025)]
# wraps the grid-stride loop: K = 65 takes 64 lanes per row, 4 rows per workgroup, 2048 workgroups = 8192 rows a sweep;
# 8200 rows leave a second sweep of 8 rows (two workgroups, the rest idle)
WRAP = [(1, 8200, 65)]
assert rows_per_sweep(65, False) == 8192 and rows_per_sweep(65, True) == 8192
# the CSR form: one "graph" of 2^20 rows, no mask; 4 lanes per row -> 131072 rows a sweep, 8 sweeps
CSR = [(1, 1 << 20, 8)]
MASKS = ("null", "full", "one", "mix")


def num_nodes(mask, B, n):
    """int32 [B] or None."""
    if mask == "null":
        return None
    if mask == "full":
        return np.full(B, n, dtype=np.int32)
    if mask == "one":
        return np.ones(B, dtype=np.int32)
    return np.array([(n, 1, max(n // 2, 1))[b % 3] for b in range(B)], dtype=np.int32)       # mix


def valid_rows(nn, B, n):
    """bool [B, n]."""
    if nn is None:
        return np.ones((B, n), dtype=bool)
    return np.arange(n)[None, :] < np.clip(nn, 0, n)[:, None]


def softmax_rows(rng, B, n, K, scale=3.0):
    z = rng.standard_normal((B, n, K)) * scale
    z -= z.max(axis=2, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def special_rows(S, rng):
    """Some rows exactly one-hot, some with exact zeros (where the row is wide enough)."""
    B, n, K = S.shape
    for b in range(B):
        for i in range(0, n, 3):
            S[b, i] = 0.0
            S[b, i, int(rng.integers(K))] = 1.0
        if K >= 3:
            for i in range(1, n, 3):
                S[b, i, int(rng.integers(K))] = 0.0
    return S


# ---- the fp64 reference
def entropy_ref(S, nn=None):
    """(E, magnitude) in float64; magnitude = (sum|s ln(s+eps)| + sum s) / norm over the valid rows."""
    B, n, K = S.shape
    v = valid_rows(nn, B, n)
    s = S.astype(np.float64)[v]                      # selected, never multiplied: masked rows may hold anything
    norm = max(int(v.sum()), 1)
    t = s * np.log(s + EPS)
    return -t.sum() / norm, (np.abs(t).sum() + s.sum()) / norm


def fwd_bound(mag):
    return C_FWD * U * mag


def grad_ref(S, nn, g, w):
    """(dS, bound) in float64 for dloss = g and weight = w; masked rows exactly 0 with bound 0."""
    B, n, K = S.shape
    v = valid_rows(nn, B, n)
    norm = max(int(v.sum()), 1)
    s = np.where(v[:, :, None], S.astype(np.float64), 0.5)      # masked rows: any finite stand-in, zeroed below
    ln = np.log(s + EPS)
    d = -(ln + s / (s + EPS)) * (g * w) / norm
    bound = C_BWD * U * (np.abs(ln) + 1.0) * abs(g * w) / norm
    return np.where(v[:, :, None], d, 0.0), np.where(v[:, :, None], bound, 0.0)


# ---- defects the forward bound must tell from rounding (tests/test_assign_ent_cpu.py), float64 throughout
FAULT_CASES = [(1, 7, 5), (3, 7, 3), (3, 7, 63), (2, 32, 64), (1, 64, 33), (3, 21, 62), (2, 9, 2)]


def faulty_entropy(S, nn, fault):
    """E as a kernel with the named defect would return it; None where the defect cannot occur for this input."""
    B, n, K = S.shape
    v = valid_rows(nn, B, n)
    s64 = S.astype(np.float64)
    term = -(s64 * np.log(s64 + EPS))
    norm = max(int(v.sum()), 1)
    good = term[v].sum()
    if fault == "last_column":
        return term[:, :, :K - 1][v].sum() / norm
    if fault == "last_valid_row":
        b = B - 1
        last = int(v[b].sum()) - 1
        return (good - term[b, last].sum()) / norm
    if fault == "masked_row_leaks":
        for b in range(B):
            nb = int(v[b].sum())
            if nb < n:
                return (good + term[b, nb].sum()) / norm
        return None
    if fault == "divisor_BN":
        return None if norm == B * n else good / (B * n)
    if fault == "quad_fourth_lane":
        # the last quad of a row whose width is no multiple of 4 reads on into the next row's first entries; the one
        # lane that loses its mask adds the entry right after the row (rows packed, lds = K)
        if K % 4 == 0:
            return None
        flat = term.reshape(-1)
        extra = sum(flat[(b * n + i) * K + K] for b in range(B) for i in range(n)
                    if v[b, i] and (b * n + i) * K + K < flat.size)
        return (good + extra) / norm
    raise ValueError(fault)


FAULTS = ("last_column", "last_valid_row", "masked_row_leaks", "divisor_BN", "quad_fourth_lane")
