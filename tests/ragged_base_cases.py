"""Inputs, fp64 reference and error bound of the padded-row table (dp_ragged_padval_fwd), and the graphs of the ragged
base-encoder tests (tests/test_gpu_ragged_base.py).

The table.  In the dense batch padded to P rows, node index i holds, in front of apply_bn, the rows relu(x) of the cnt_i
graphs that own it and (B - cnt_i) copies of `pad`; every padded row of the index comes out as

    v[i, f] = (pad_f - mu_i) r_i,      mu_i = mean over (b, f),   r_i = 1 / sqrt(var_i + 1e-5)  (biased variance).

Indices i >= max_n have no owner: mu, r are those of `pad` alone and one table row (max_n) stands for all of them.  The
reference below forms the padded [B, P, F] block in float64 from the fp32 inputs and reads v off a padded row.

Bound (u = 2^-24; counted from the arithmetic of k_bn_ragged_fwd / k_ragged_padval, not fitted).  T = ceil(F / 64) is
the number of features one lane walks.
  * mu: a lane adds cnt_i T real values and T pad values in sequence, the wave tree adds 6 levels, then one product by
    (B - cnt_i), one sum of the two parts and one product by 1 / (B F): C_mu = (cnt_i + 1) T + 9 roundings on a sum of
    magnitudes, so |d mu| <= C_mu u A_i with A_i = mean |h| over the index's B F values.
  * var: each d = fl(h - mu^) rounds once, d d once, and the sum takes the same C_mu roundings: a relative error of
    (C_mu + 3) u on a sum of squares; using mu^ for mu adds (d mu)^2 exactly.  var + eps, sqrtf and the quotient round
    once each (correctly rounded; budgeted at 2 u each): r^ = r (1 + rho),
    |rho| <= (C_mu + 3) u / 2 + (d mu)^2 r^2 / 2 + 5 u.
  * v^ = fl(fl(pad - mu^) r^): |v^ - v| <= r |d mu| + |v| (|rho| + 2 u).
Total, with 1 % on top for the products of first-order terms (C u < 1e-3 at every shape used):

    |v^ - v| <= 1.01 [ r_i C_mu u A_i + |v| ((C_mu + 3) u / 2 + (C_mu u A_i r_i)^2 / 2 + 7 u) ].

The tail row has cnt = 0 and B F copies of pad, summed as F values: C_mu = T + 7.
"""
import numpy as np
import torch

U = 2.0 ** -24
BN_EPS = 1e-5


def pad_rows(x, sizes, P, fill=None):
    """ragged [n_total, F] -> [B, P, F]; the rows behind each graph hold `fill` [F] (None: zeros)."""
    out = torch.zeros(len(sizes), P, x.shape[1], dtype=x.dtype)
    if fill is not None:
        out = out + fill
    o = 0
    for b, n in enumerate(sizes):
        out[b, :n] = x[o:o + n]
        o += n
    return out


def unpad(x, sizes):
    return torch.cat([x[b, :n] for b, n in enumerate(sizes)], dim=0)


def table_rows(sizes, P):
    """(n_min, max_n, n_idx) of the padded-row table."""
    return int(min(sizes)), int(max(sizes)), int(max(sizes)) + int(P > max(sizes))


def padval_reference(x, pad, sizes, P):
    """float64 (v [n_idx, F], bound [n_idx, F]) from fp32 x [n_total, F] (pre-ReLU) and pad [F]; rows below n_min are
    zero in both (those indices have no padded row)."""
    n_min, max_n, n_idx = table_rows(sizes, P)
    B, F_ = len(sizes), x.shape[1]
    h = pad_rows(torch.relu(x.double()), sizes, P, fill=pad.double())
    mu = h.mean(dim=(0, 2))
    var = (h - mu[None, :, None]).pow(2).mean(dim=(0, 2))
    r = 1.0 / torch.sqrt(var + BN_EPS)
    A = h.abs().mean(dim=(0, 2))
    T = -(-F_ // 64)
    cnt = torch.tensor([sum(1 for n in sizes if n > i) for i in range(P)], dtype=torch.float64)
    c_mu = torch.where(torch.arange(P) < max_n, (cnt + 1) * T + 9, torch.full((P,), T + 7.0, dtype=torch.float64))
    v = (pad.double()[None, :] - mu[:, None]) * r[:, None]
    dmu = c_mu * U * A
    rho = (c_mu + 3) * U / 2 + (dmu * r) ** 2 / 2 + 7 * U
    bound = 1.01 * ((r * dmu)[:, None] + v.abs() * rho[:, None])
    v, bound = v[:n_idx].clone(), bound[:n_idx].clone()
    v[:n_min] = 0
    bound[:n_min] = 0
    return v, bound


def ring_with_chords(sizes, seed):
    """Per graph an edge list: the ring 0 - 1 - ... - (n-1) - 0 plus n // 2 random chords, so no node is isolated (an
    isolated real node holds exactly what a padded row holds, which would hide a wrong winner).  n = 2: one edge; n = 1:
    none — its single node IS isolated, there is no other graph on one node."""
    rng = np.random.default_rng(seed)
    srcs, dsts = [], []
    for n in sizes:
        if n == 1:
            s = d = np.zeros(0, dtype=np.int64)
        elif n == 2:
            s, d = np.array([0]), np.array([1])
        else:
            ring = np.arange(n)
            cs, cd = rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)
            keep = cs != cd
            s, d = np.concatenate([ring, cs[keep]]), np.concatenate([(ring + 1) % n, cd[keep]])
        srcs.append(s.astype(np.int64))
        dsts.append(d.astype(np.int64))
    return srcs, dsts


def dense_adj(sizes, srcs, dsts, P, dtype=torch.float64):
    adj = torch.zeros(len(sizes), P, P, dtype=dtype)
    for b, (s, d) in enumerate(zip(srcs, dsts)):
        adj[b, s, d] = 1.0
        adj[b, d, s] = 1.0
    return adj
