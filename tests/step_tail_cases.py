"""Case tables, inputs, float64 references, derived error bounds and fp32 emulations of the kernels that close every
training step or open every GraphSAGE layer: cross entropy (k_ce_fwd / k_ce_bwd, dp_rowops.hip), the fused clip + Adam
step (k_sqnorm_partials / k_clip_adam, dp_optim.hip) and the mean aggregator with its scatter backward (k_csr_agg_fwd /
k_csr_agg_bwd_scatter with mean = 1, dp_meanagg.hip).  Shared by tests/test_step_tail_cases_cpu.py (which shows that every
bound admits a correct fp32 evaluation and rejects each seeded mistake by at least 2x) and tests/test_gpu_step_tail.py.

Every reference is float64 on the fp32 inputs.  Bounds are first-order rounding counts, U = 2^-24 (one fp32 rounding,
relative), counted from the kernels' arithmetic; expf / logf / sqrtf / a division are taken at 2 U of their value, as
everywhere in this suite.  A contraction of a product and an add into one FMA only removes a rounding.  TINY = 2^-126
(the smallest normal fp32) is added wherever a result can fall below the normal range and be flushed.  No bound is a
literal tolerance and none is the run-time form of rowop_cases.py (the formula in fp32 on the CPU times a factor): that
form is for cancelling formulas, and nothing cancels here.  In particular the Adam quotient m / (sqrt(v) inv + eps) near
sqrt(v) inv ~ eps has a denominator that is a sum of two positive terms, so its relative error is at most the larger of
its terms' and the count below stays useful there (the "tiny" cases: |error| / bound of a correct fp32 evaluation < 1,
of eps moved inside the root > 100).

Cross entropy, row b of C logits l (one thread per row, rows b, b + 256, ... on the same thread):
  m = max l is exact.  d_c = l_c - m rounds once: U |d_c| absolute in the argument of expf, hence U |d_c| relative in
  e_c = expf(d_c), plus expf's 2 U.  s = sum e_c, added in order: C - 1 adds of positive terms, (C - 1) U s.
      err(s) = sum_c e_c (|d_c| + 2) U + (C - 1) U s + C TINY
  lse = m + logf(s): err(lse) = err(s) / s + 2 U |log s| + U |lse|.   t_b = lse - l_y: err(t_b) = err(lse) + U |t_b|.
  loss = (sum_b t_b) / B: a thread adds ceil(B / 256) terms, the LDS tree 8 more, then one division:
      err(loss) = [sum_b err(t_b) + (ceil(B / 256) + 8) U sum_b |t_b|] / B + 2 U |loss|
  prob_c = expf(l_c - lse): the argument carries err(lse) and its own rounding U |l_c - lse|:
      err(prob_c) = prob_c (err(lse) + U |l_c - lse| + 2 U) + TINY
  d_ypred_unit = (prob_c - [y = c]) / B: err = (err(prob_c) + U |prob_c - [y = c]|) / B + 2 U |d_ypred_unit| + TINY
  dlogits = g (prob_c - [y = c]), g = dloss / B (k_ce_bwd, fed the forward's prob):
      err = |g| (err(prob_c) + U |prob_c - [y = c]|) + 3 U |dlogits| + TINY       (2 U the quotient g, U the product)
  The two gradients divide by B / multiply by 1 / B: both within bound, not equal bit for bit.

Clip + Adam over n floats, wgs = min(ceil(n / 256), 256) workgroups of 256 (OPT_WGS = 256):
  sum of squares: a thread adds k = ceil(n / (256 wgs)) rounded squares, the wave sum 6 more, the four waves 3, then
  k_clip_adam adds at most 4 partials per lane and 6 more in its wave sum: an entry sees at most k + 19 adds and its
  product, all terms positive: (k + 20) U relative.  total = sqrtf: rho_n = ((k + 20) / 2 + 2) U relative.
  coefficient c = min(max_norm / (total + 1e-6), 1): the sum rounds once, the quotient 2 U:
      rho_c = rho_n total / (total + 1e-6) + 3 U relative;  0 where even (1 - rho_c) max_norm / (total + 1e-6) > 1
      (there the kernel's c is exactly 1) and 0 for max_norm <= 0.
  g' = g c:                  err(g') = |g| err(c) + U |g'|                     (0 without clipping: g' = g bit for bit)
  m' = b1 m + (1 - b1) g':   err(m') = U |b1 m| + 2 U |(1 - b1) g'| + (1 - b1) err(g') + U |m'|
  v' = b2 v + (1 - b2) g'^2: err(v') = U b2 v + 3 U (1 - b2) g'^2 + 2 (1 - b2) |g'| err(g') + U v'
      (1 - b in fp32 is what the kernel multiplies by; the reference takes that fp32 value: for b in [0.5, 1) it is
      exact, and one of the U above is there for the b that are not)
  r = sqrtf(v'):             err(r) = err(v') / (2 r) + 2 U r
  den = r inv + eps:         err(den) = err(r) inv + 2 U r inv + U den      (inv = 1 / sqrt(1 - b2^t), double -> fp32: U)
  q = m' / den:              err(q) = err(m') / den + |m'| err(den) / den^2 + 2 U |q|
  p' = p - step q:           err(p') = step err(q) + 2 U |step q| + U |p'|  (step = lr / (1 - b1^t), double -> fp32: U)
  The reference takes lr, the betas, eps and max_norm at their fp32 values (the entries take floats) and the bias
  corrections in float64.  |g| stays below 2^40 in every case, so the fp32 sum of n <= 2^18 squares stays below 2^98
  and cannot overflow; clipping of gradients whose SQUARES overflow fp32 is outside these tests.

Mean aggregation, row i with deg stored entries (one wave per row, lanes across the columns):
  forward: four partial sums filled 4 entries at a time, the up to 3 left-over entries onto the first, (s0 + s1) +
  (s2 + s3): an entry sees at most floor(deg / 4) + 5 adds; scale = 1 / deg (2 U) multiplies once (U):
      err = (floor(deg / 4) + 8) U sum_j |x_j| / deg      (+ U (sum_j |x_j| / deg + |old|) with beta = 1)
  A row of degree 0 is 0 * (1 / 0) = NaN in every column, as the reference's mask.div(0) gives.
  backward (float atomics, any order): dtable_j = old_j + sum_{i -> j} dout_i / deg_i; each term is a quotient and a
  product (3 U) and passes through at most indeg_j adds, indeg_j the stored entries (i, j) with i < n_rows:
      err = (indeg_j + 3) U (|old_j| + sum_i |dout_i| / deg_i);  0 for indeg_j = 0: the row is not touched.
  A row i of degree 0 has no entry and contributes nothing.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

from graph_pooling_amd.sparse import CsrGraph

U = 2.0 ** -24
TINY = 2.0 ** -126
F = np.float32


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def worst(got, ref, bound):
    """Largest |got - ref| / bound; inf where got is not finite but ref is, or where the NaN patterns differ."""
    got, ref, bound = (np.asarray(t, dtype=np.float64) for t in (got, ref, bound))
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan) or np.isinf(got[~nan]).any():
        return math.inf
    if not (~nan).any():
        return 0.0
    err = np.abs(got - ref)[~nan]
    b = np.broadcast_to(bound, ref.shape)[~nan]
    return float(np.where(err == 0.0, 0.0, err / np.maximum(b, 1e-300)).max())


# ------------------------------------------------------------------ cross entropy
CE_SHAPES = ((1, 1), (1, 2), (5, 3), (20, 6), (255, 2), (256, 4), (257, 2), (513, 7))
CE_SCALES = (1.0, 30.0, 90.0)
CE_DLOSS = (None, 1.7)
CE_MISTAKES = ("divide by B - 1", "no max subtraction", "d_ypred_unit without / B")
CeCase = namedtuple("CeCase", "id B C scale labels equal_row")


def ce_cases():
    cases = [CeCase(f"B={B} C={C} scale={s:g}", B, C, s, "random", False) for B, C in CE_SHAPES for s in CE_SCALES]
    cases.append(CeCase("B=20 C=6 scale=1 labels=0", 20, 6, 1.0, "first", False))
    cases.append(CeCase("B=257 C=2 scale=30 labels=C-1", 257, 2, 30.0, "last", False))
    cases.append(CeCase("B=5 C=3 scale=90 equal-row", 5, 3, 90.0, "random", True))
    return cases


def ce_inputs(c):
    """(logits fp32 [B, C], label int64 [B]), every label inside [0, C)."""
    rng = _rng("ce " + c.id)
    logits = (rng.standard_normal((c.B, c.C)) * c.scale).astype(F)
    label = {"random": rng.integers(0, c.C, c.B), "first": np.zeros(c.B, dtype=np.int64),
             "last": np.full(c.B, c.C - 1)}[c.labels].astype(np.int64)
    if c.equal_row:
        logits[c.B // 2, :] = logits[c.B // 2, 0]
    return logits, label


def ce_ref(logits, label, dloss=None):
    """name -> (float64 reference, bound) for loss, prob, dunit, dlogits (module docstring)."""
    l = np.asarray(logits, dtype=np.float64)
    B, C = l.shape
    rows = np.arange(B)
    m = l.max(axis=1, keepdims=True)
    d = l - m
    e = np.exp(d)
    s = e.sum(axis=1, keepdims=True)
    lse = m + np.log(s)
    e_s = (e * (np.abs(d) + 2.0)).sum(axis=1, keepdims=True) * U + (C - 1) * U * s + C * TINY
    e_lse = e_s / s + 2 * U * np.abs(np.log(s)) + U * np.abs(lse)
    t = (lse[:, 0] - l[rows, label])
    e_t = e_lse[:, 0] + U * np.abs(t)
    loss = t.sum() / B
    e_loss = (e_t.sum() + (math.ceil(B / 256) + 8) * U * np.abs(t).sum()) / B + 2 * U * abs(loss)
    p = np.exp(l - lse)
    e_p = p * (e_lse + U * np.abs(l - lse) + 2 * U) + TINY
    oh = np.zeros_like(p)
    oh[rows, label] = 1.0
    diff = p - oh
    e_diff = e_p + U * np.abs(diff)
    dunit = diff / B
    g = (1.0 if dloss is None else float(F(dloss))) / B
    dlog = g * diff
    return dict(loss=(np.float64(loss), np.float64(e_loss)), prob=(p, e_p),
                dunit=(dunit, e_diff / B + 2 * U * np.abs(dunit) + TINY),
                dlogits=(dlog, abs(g) * e_diff + 3 * U * np.abs(dlog) + TINY))


def ce_emulate(logits, label, dloss=None, mistake=None):
    """k_ce_fwd / k_ce_bwd in fp32 NumPy, in the kernel's order of operations; `mistake`: one of CE_MISTAKES."""
    assert mistake is None or mistake in CE_MISTAKES
    l = np.asarray(logits, dtype=F)
    B, C = l.shape
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        m = np.zeros(B, dtype=F) if mistake == "no max subtraction" else l.max(axis=1)
        s = np.zeros(B, dtype=F)
        for c in range(C):
            s = s + np.exp(l[:, c] - m)
        lse = m + np.log(s)
        t = lse - l[rows, label]
        acc = np.zeros(256, dtype=F)
        for b0 in range(0, B, 256):
            chunk = t[b0:b0 + 256]
            acc[:chunk.size] += chunk
        w = 128
        while w:
            acc[:w] += acc[w:2 * w]
            w >>= 1
        loss = acc[0] / F(B - 1 if mistake == "divide by B - 1" else B)
        prob = np.exp(l - lse[:, None])
        oh = np.zeros((B, C), dtype=F)
        oh[rows, label] = 1.0
        dunit = prob - oh
        if mistake != "d_ypred_unit without / B":
            dunit = dunit / F(B)
        g = F(1.0 if dloss is None else dloss) * F(1.0) / F(B)
        dlog = g * (prob - oh)
    return dict(loss=loss, prob=prob, dunit=dunit, dlogits=dlog)


# ------------------------------------------------------------------ clip + Adam
LR, BETA1, BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
OPT_WGS = 256
ADAM_SIZES = (1, 63, 64, 65, 255, 256, 257, 65280, 65281, 65536, 65537, 196613)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_STATE_SIZES = (1000, 196613)
# state -> (gradient scale, max_norm, total_norm_out given)
# ("plain": 0.1 sqrt(n) passes max_norm = 2 from n = 400, so the size sweep has the coefficient exactly 1 up to n = 257 and
# below 1 above; "loose" is the given-but-inactive clip at every size)
ADAM_STATES = {"plain": (0.1, 2.0, True), "active": (10.0, 2.0, True), "small-norm": (1e-5, 1e-4, True),
               "tiny": (1e-8, 0.0, True), "no clip, no norm": (0.1, 0.0, False), "norm only": (0.1, 0.0, True),
               "loose": (0.1, 1e9, True)}
ADAM_MISTAKES = ("clip coefficient without the 1e-6", "bias corrections of t - 1", "eps inside the square root",
                 "moments from the unclipped gradient")
# the states that tell a mistake from rounding, by more than this factor, at both sizes: these cases stay in the table
ADAM_SEPARATES = {"clip coefficient without the 1e-6": ("small-norm", 100.0), "eps inside the square root": ("tiny", 100.0),
                  "moments from the unclipped gradient": ("active", 2.0), "bias corrections of t - 1": ("plain", 2.0)}
NONFINITE_N = 65537
AdamCase = namedtuple("AdamCase", "id n state t")


def adam_cases():
    cases = [AdamCase(f"n={n} plain t={ADAM_STEPS[i % 5]}", n, "plain", ADAM_STEPS[i % 5]) for i, n in enumerate(ADAM_SIZES)]
    cases += [AdamCase(f"n={n} {state} t=3", n, state, 3) for n in ADAM_STATE_SIZES for state in ADAM_STATES]
    cases += [AdamCase(f"n=1000 active t={t}", 1000, "active", t) for t in ADAM_STEPS]
    return cases


def adam_inputs(c):
    """dict p, g, m, v (fp32 [n]): random parameters, moments on the gradient's scale, v >= 0."""
    rng = _rng("adam " + c.id)
    scale = ADAM_STATES[c.state][0]
    g = (rng.standard_normal(c.n) * scale).astype(F)
    p = rng.standard_normal(c.n).astype(F)
    m = (rng.standard_normal(c.n) * scale).astype(F)
    v = ((rng.standard_normal(c.n) * scale) ** 2).astype(F)
    assert np.abs(g).max() < 2.0 ** 40
    return dict(p=p, g=g, m=m, v=v)


def adam_ref(x, t, max_norm):
    """name -> (float64 reference, bound) for norm, g, m, v, p after ONE step from the state x (module docstring)."""
    p, g, m, v = (np.asarray(x[k], dtype=np.float64) for k in "pgmv")
    n = g.size
    wgs = min((n + 255) // 256, OPT_WGS)
    k = math.ceil(n / (256 * wgs))
    b1, b2, eps, lr = (float(F(z)) for z in (BETA1, BETA2, ADAM_EPS, LR))
    omb1, omb2 = float(F(1) - F(BETA1)), float(F(1) - F(BETA2))
    tn = math.sqrt(float((g * g).sum()))
    rho_n = ((k + 20) / 2 + 2) * U
    c, e_c = 1.0, 0.0
    if max_norm > 0:
        small = float(F(1e-6))
        xq = float(F(max_norm)) / (tn + small)
        rho_c = rho_n * tn / (tn + small) + 3 * U
        c = min(xq, 1.0)
        e_c = 0.0 if xq * (1 - rho_c) > 1.0 else rho_c * c
    gi = g * c
    e_g = np.abs(g) * e_c + U * np.abs(gi) if max_norm > 0 else np.zeros_like(g)
    mi = b1 * m + omb1 * gi
    e_m = U * np.abs(b1 * m) + 2 * U * np.abs(omb1 * gi) + omb1 * e_g + U * np.abs(mi)
    vi = b2 * v + omb2 * gi * gi
    e_v = U * b2 * v + 3 * U * omb2 * gi * gi + 2 * omb2 * np.abs(gi) * e_g + U * vi
    r = np.sqrt(vi)
    e_r = e_v / (2 * np.maximum(r, 1e-300)) + 2 * U * r
    step = lr / (1.0 - b1 ** t)
    inv = 1.0 / math.sqrt(1.0 - b2 ** t)
    den = r * inv + eps
    e_den = e_r * inv + 2 * U * r * inv + U * den
    q = mi / den
    e_q = e_m / den + np.abs(mi) * e_den / den ** 2 + 2 * U * np.abs(q)
    pn = p - step * q
    e_p = step * e_q + 2 * U * np.abs(step * q) + U * np.abs(pn)
    return dict(norm=(np.float64(tn), np.float64(rho_n * tn)), g=(gi, e_g), m=(mi, e_m), v=(vi, e_v), p=(pn, e_p))


def adam_emulate(x, t, max_norm, mistake=None):
    """k_sqnorm_partials / k_clip_adam in fp32 NumPy (the sum of squares in NumPy's own order); `mistake`: one of
    ADAM_MISTAKES."""
    assert mistake is None or mistake in ADAM_MISTAKES
    p, g, m, v = (np.asarray(x[k], dtype=F) for k in "pgmv")
    b1, b2, eps = F(BETA1), F(BETA2), F(ADAM_EPS)
    with np.errstate(all="ignore"):
        tn = np.sqrt(np.sum(g * g, dtype=F))
        c = F(1)
        if max_norm > 0:
            small = F(0) if mistake == "clip coefficient without the 1e-6" else F(1e-6)
            c = np.minimum(F(max_norm) / (tn + small), F(1))
        gi = g * c
        gm = g if mistake == "moments from the unclipped gradient" else gi
        mi = b1 * m + (F(1) - b1) * gm
        vi = b2 * v + (F(1) - b2) * gm * gm
        tt = np.float64(t - 1 if mistake == "bias corrections of t - 1" else t)
        step = F(np.float64(F(LR)) / (1.0 - np.float64(b1) ** tt))
        inv = F(1.0 / np.sqrt(1.0 - np.float64(b2) ** tt))
        den = np.sqrt(vi + eps) * inv if mistake == "eps inside the square root" else np.sqrt(vi) * inv + eps
        pn = p - step * (mi / den)
    return dict(norm=tn, g=gi, m=mi, v=vi, p=pn)


# ------------------------------------------------------------------ mean aggregation
MEAN_NROWS = (1, 3, 4, 5, 160)
MEAN_MISTAKES = ("1 / (deg + 1)", "tail of the 4-way unroll dropped", "only the first 64-id chunk read")
GRID_DEGREES = (1, 2, 4, 8, 16, 32, 64, 128)


def csr_arrays(g):
    """(indptr, indices) as int64 NumPy."""
    ip = g.indptr.cpu().numpy().astype(np.int64)
    return ip, g.indices.cpu().numpy().astype(np.int64)[:ip[-1]]


def dense01(g):
    """float64 [n, n] with 1 at every stored entry: the mean aggregator reads no weights."""
    ip, ix = csr_arrays(g)
    a = np.zeros((g.n, g.n))
    a[np.repeat(np.arange(g.n), np.diff(ip)), ix] = 1.0
    return a


def grid_graph(device="cpu"):
    """Directed 0/1 graph of 160 nodes, every degree a power of two (GRID_DEGREES in turn)."""
    n = 160
    rng = np.random.default_rng(11)
    src = np.concatenate([np.full(GRID_DEGREES[r % 8], r) for r in range(n)])
    dst = np.concatenate([rng.choice(n, GRID_DEGREES[r % 8], replace=False) for r in range(n)])
    return CsrGraph.from_edges(n, src, dst, device, symmetric=False)


def mean_inputs(n, n_rows, feat):
    rng = _rng(f"mean {n_rows} {feat}")
    r = lambda rows: rng.standard_normal((rows, feat)).astype(F)
    return dict(x=r(n), old=r(n), dout=r(n_rows), dt_old=r(n))


def mean_fwd_ref(a, x, n_rows, beta=0.0, old=None):
    """(reference [n_rows, feat], NaN in the rows of degree 0; bound)."""
    a = a[:n_rows]
    x = np.asarray(x, dtype=np.float64)
    deg = a.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        ref = np.where(deg > 0, (a @ x) / deg, np.nan)
        mag = np.where(deg > 0, (a @ np.abs(x)) / deg, 0.0)
    bound = (deg // 4 + 8) * U * mag
    if beta:
        o = np.asarray(old, dtype=np.float64)[:n_rows]
        ref = ref + beta * o
        bound = bound + U * (mag + np.abs(beta * o))
    return ref, bound


def mean_bwd_ref(a, dout, n_rows, dt_old):
    """(reference [n, feat] = old + A_mean^T dout over the first n_rows rows of A, bound)."""
    a = a[:n_rows]
    dout, old = np.asarray(dout, dtype=np.float64), np.asarray(dt_old, dtype=np.float64)
    deg = a.sum(axis=1, keepdims=True)
    am = np.where(deg > 0, a / np.maximum(deg, 1.0), 0.0)
    indeg = (am > 0).sum(axis=0)[:, None]
    ref = old + am.T @ dout
    mag = np.abs(old) + am.T @ np.abs(dout)
    return ref, np.where(indeg > 0, (indeg + 3) * U * mag, 0.0)


def mean_fwd_emulate(ip, ix, x, n_rows, beta=0.0, old=None, mistake=None):
    """k_csr_agg_fwd with mean = 1 in fp32 NumPy, in the kernel's order; `mistake`: one of MEAN_MISTAKES."""
    assert mistake is None or mistake in MEAN_MISTAKES
    x = np.asarray(x, dtype=F)
    out = np.empty((n_rows, x.shape[1]), dtype=F)
    with np.errstate(all="ignore"):
        for row in range(n_rows):
            ids = ix[ip[row]:ip[row + 1]]
            s = np.zeros((4, x.shape[1]), dtype=F)
            for e0 in range(0, ids.size, 64):
                chunk = ids[e0:e0 + 64]
                j = 0
                while j + 4 <= chunk.size:
                    for k in range(4):
                        s[k] += x[chunk[j + k]]
                    j += 4
                if mistake != "tail of the 4-way unroll dropped":
                    for jj in range(j, chunk.size):
                        s[0] += x[chunk[jj]]
                if mistake == "only the first 64-id chunk read":
                    break
            scale = F(1) / F(ids.size + (1 if mistake == "1 / (deg + 1)" else 0))
            v = ((s[0] + s[1]) + (s[2] + s[3])) * scale
            out[row] = v + F(beta) * np.asarray(old, dtype=F)[row] if beta else v
    return out


def mean_bwd_emulate(ip, ix, dout, n_rows, dt_old, mistake=None):
    """k_csr_agg_bwd_scatter with mean = 1 in fp32 NumPy, the adds in row order."""
    assert mistake in (None, "1 / (deg + 1)")
    dt = np.array(dt_old, dtype=F)
    dout = np.asarray(dout, dtype=F)
    with np.errstate(all="ignore"):
        for row in range(n_rows):
            ids = ix[ip[row]:ip[row + 1]]
            g = dout[row] * (F(1) / F(ids.size + (1 if mistake else 0)))
            for j in ids:
                dt[j] += g
    return dt
