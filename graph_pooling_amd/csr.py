"""The CSR containers of the sparse path: `CsrGraph` (one graph) and `CsrBatch` (a ragged batch), on one base class.

`CsrContainer` holds what the two share, once: the stored-entry count and the permutations between the CSR and its
transpose (cached on first use), `directed()` / `sym_normalized()` / `with_values()` / `normalized()`, the `values` /
`values_t` pairing rule and the check of index arrays handed over on a device.  Each class adds its constructors and
the four steps of the DiffPool model that differ between one graph and a batch (`bn_relu`, `readout`, `pool`,
`link_loss`).  `HostCsr` is the host record the constructors pass around.

Sits above `ops` (the containers' steps are ops) and below `sparse`, which holds the model classes and re-exports
`CsrGraph`, `CsrBatch` and `HostCsr`.
"""
from __future__ import annotations

import copy
from functools import cached_property
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _lib, ops


# ----------------------------------------------------------------------------- CSR helpers
def _check_values(values, indices, what):
    """A container's `values`: an fp32 tensor with one entry per stored index, on the indices' device."""
    if not isinstance(values, torch.Tensor):
        raise TypeError(f"{what} must be a tensor, got {type(values).__name__}")
    if values.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {values.dtype}")
    if values.dim() != 1 or values.numel() != indices.numel():
        raise ValueError(f"{what} must hold one value per stored entry [{indices.numel()}], got {tuple(values.shape)}")
    if values.device != indices.device:
        raise ValueError(f"{what} is on {values.device} but the index arrays are on {indices.device}")
    return values.contiguous()


def _check_device_arrays(what, arrays, indptr, rows, rows_name):
    """The index arrays a `from_device_csr` takes, as (name, tensor) pairs: each a contiguous 1-d int32 tensor on
    indptr's device, the `indptr*` ones holding rows + 1 offsets (`rows_name` is how the message calls `rows`)."""
    for name, t in arrays:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-d int32 tensor")
        if t.device != indptr.device:
            raise ValueError(f"{what}: {name} is on {t.device}, indptr on {indptr.device}")
        if name.startswith("indptr") and t.numel() != rows + 1:
            raise ValueError(f"{what}: {name} must hold {rows_name} + 1 = {rows + 1} offsets, got {t.numel()}")


class HostCsr(NamedTuple):
    """One graph's CSR as host arrays with graph-local columns — the per-graph record of `CsrBatch.__init__`, and what
    the containers' host code passes around.  The transposed trio is None for an undirected graph, `values` /
    `values_t` (one per stored entry, next to `indices` / `indices_t`) None for a 0/1 graph."""
    indptr: Any
    indices: Any
    indptr_t: Any = None
    indices_t: Any = None
    values: Any = None
    values_t: Any = None


def _host_csr(n, src, dst, symmetric=True, weight=None):
    """The host part of `CsrGraph.from_edges`: edge list -> HostCsr (int32 indices sorted by row then column, duplicates
    merged, fp32 values), raising on an entry given with two weights."""
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    w = None
    if weight is not None:
        w = np.asarray(weight, dtype=np.float32).reshape(-1)
        if w.size != src.size:
            raise ValueError(f"CsrGraph.from_edges: {w.size} weights for {src.size} edges")
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        if w is not None:
            w = np.concatenate([w, w])
    if w is None:
        key = np.unique(src * n + dst)
    else:
        order = np.argsort(src * n + dst, kind="stable")
        key, w = (src * n + dst)[order], w[order]
        first = np.ones(key.size, dtype=bool)
        first[1:] = key[1:] != key[:-1]
        head = np.maximum.accumulate(np.where(first, np.arange(key.size), 0))     # first entry of each run
        clash = np.nonzero(w != w[head])[0]
        if clash.size:
            e = int(clash[0])
            raise ValueError(f"CsrGraph.from_edges: entry ({int(key[e] // n)}, {int(key[e] % n)}) is given with two "
                             f"weights ({w[head[e]]:g} and {w[e]:g})")
        key, w = key[first], w[first]
    rows, cols = key // n, key % n

    def csr(r, c):
        order = np.lexsort((c, r))
        r, c = r[order], c[order]
        indptr = np.zeros(n + 1, dtype=np.int32)
        np.add.at(indptr, r + 1, 1)
        return (np.cumsum(indptr, dtype=np.int64).astype(np.int32), c.astype(np.int32),
                None if w is None else np.ascontiguousarray(w[order]))
    (ip, ix, val), (ipt, ixt, valt) = csr(rows, cols), (None, None, None) if symmetric else csr(cols, rows)
    return HostCsr(ip, ix, ipt, ixt, val, valt)


def _read_back(g):
    """A container's CSR read back to the host once -> HostCsr, trimmed to the indptr[-1] stored entries (an edgeless
    batch pads its arrays)."""
    def trio(indptr, indices, values):
        ip = indptr.cpu().numpy()
        return ip, indices.cpu().numpy()[:ip[-1]], None if values is None else values.cpu().numpy()[:ip[-1]]
    ip, ix, val = trio(g.indptr, g.indices, g.values)
    ipt, ixt, valt = (None, None, None) if g.undirected else trio(g.indptr_t, g.indices_t, g.values_t)
    return HostCsr(ip, ix, ipt, ixt, val, valt)


def _normalized_values(n, h, what):
    """(values, values_t | None), fp32, of D^-1/2 A D^-1/2 for the HostCsr `h` of n nodes.  The degree is the column sum
    of the stored values (ones for a 0/1 graph) as the reference takes it (graph_sampler.py:27: np.sum(adj, axis=0)), in
    float64 on the host, rounded once.  A node of degree 0 raises, naming the container `what`: the reference's
    inf * 0 = NaN row has no place in a CSR."""
    def rows(indptr):          # the row of every stored entry
        return np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))
    val = np.ones(h.indices.size) if h.values is None else h.values.astype(np.float64)
    deg = np.zeros(n, dtype=np.float64)
    np.add.at(deg, h.indices, val)
    bad = np.nonzero(~(deg > 0))[0]
    if bad.size:
        raise ValueError(f"{what}.normalized(): node {int(bad[0])} has degree {deg[bad[0]]:g} (column sum of the stored "
                         f"values; {bad.size} such node(s)): D^-1/2 A D^-1/2 is not defined there")
    inv = 1.0 / np.sqrt(deg)
    new = ((val * inv[rows(h.indptr)]) * inv[h.indices]).astype(np.float32)
    if h.indptr_t is None:
        return new, None
    valt = np.ones(val.size) if h.values_t is None else h.values_t.astype(np.float64)
    return new, ((valt * inv[h.indices_t]) * inv[rows(h.indptr_t)]).astype(np.float32)      # (r, c) of A^T is a_cr


def _transpose_perm(g):
    """For a container with a transposed CSR of its own: int64 [nnz] on the device with values_t = values[perm] — entry k
    of the transposed CSR, (r, c) of A^T, is the stored entry (c, r) of A.  Computed on the host from the two CSRs (one
    read-back); raises when they are not each other's transpose."""
    h = _read_back(g)
    n = h.indptr.size - 1
    rows = lambda ip: np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip.astype(np.int64)))
    key = rows(h.indptr) * n + h.indices.astype(np.int64)               # (i, j) of every stored entry of A
    key_t = h.indices_t.astype(np.int64) * n + rows(h.indptr_t)         # ... and of every entry of A^T, as (c, r)
    order = np.argsort(key, kind="stable")
    pos = np.minimum(np.searchsorted(key[order], key_t), max(key.size - 1, 0))
    if key.size != key_t.size or (key.size and (key[order][pos] != key_t).any()):
        raise ValueError(f"{type(g).__name__}.with_values: indptr_t / indices_t are not the transpose of indptr / indices")
    return torch.from_numpy(order[pos]).to(g.indices.device)


def _mirror_perm(g):
    """int32 [nnz] on the device: entry k of the transposed CSR is the stored entry mirror_perm[k].  A container with a
    transposed CSR of its own has it as `_t_perm`; an undirected one's transposed CSR is its own arrays, so entry k =
    (r, c) maps to the stored (c, r) (one read-back; raises when the stored pattern is not symmetric)."""
    if not g.undirected:
        return g._t_perm.to(torch.int32)
    h = _read_back(g)
    n = h.indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(h.indptr.astype(np.int64)))
    key = rows * n + h.indices.astype(np.int64)               # sorted: rows ascending, columns ascending within a row
    key_t = h.indices.astype(np.int64) * n + rows
    pos = np.minimum(np.searchsorted(key, key_t), max(key.size - 1, 0))
    if key.size and (key[pos] != key_t).any():
        raise ValueError(f"{type(g).__name__}.mirror_perm: an undirected container (no transposed CSR of its own) must "
                         "store (j, i) beside every (i, j)")
    return torch.from_numpy(pos.astype(np.int32)).to(g.indices.device)


class CsrContainer:
    """What `CsrGraph` and `CsrBatch` share.  A container has int32 `indptr` / `indices` and `indptr_t` / `indices_t` on
    one device, `n` rows, `weighted` and — when weighted — fp32 `values` / `values_t`.  An UNDIRECTED container has no
    transposed CSR of its own: its `_t` fields ARE the forward tensors (`undirected` tests that identity)."""

    is_batch = False          # a CsrBatch: graph-local index arrays, per-graph tables, the batch entries of the ops
    # how the pairing rule's refusals name the two forms
    _UNDIRECTED = "an undirected graph (no transposed CSR of its own)"
    _DIRECTED = "a weighted graph with a transposed CSR of its own"

    @property
    def undirected(self):
        return self.indices_t is self.indices

    nnz = cached_property(lambda self: int(self.indptr[-1]))          # stored entries (one read-back, then cached)
    _t_perm = cached_property(_transpose_perm)
    mirror_perm = cached_property(_mirror_perm)

    def _set_values(self, values, values_t, what):
        """The `values` / `values_t` pairing rule, for a container whose index arrays are set: an undirected one takes
        `values_t` as `values` or None, a weighted directed one needs `values_t`, `values_t` without `values` is
        refused.  Sets `weighted`, `values` and `values_t`; `what` opens every message."""
        self.weighted = values is not None
        self.values = self.values_t = None
        if values is None:
            if values_t is not None:
                raise ValueError(f"{what}: values_t without values")
            return
        self.values = _check_values(values, self.indices, f"{what}: values")
        if self.undirected:
            if values_t is not None and values_t is not values:
                raise ValueError(f"{what}: {self._UNDIRECTED} stores a_ij = a_ji: values_t must be values or None")
            self.values_t = self.values
        elif values_t is None:
            raise ValueError(f"{what}: {self._DIRECTED} needs values_t")
        else:
            self.values_t = _check_values(values_t, self.indices_t, f"{what}: values_t")

    def directed(self):
        """A container of the same class with a transposed CSR of its OWN: cloned index arrays and `values_t =
        values[mirror_perm]` (data).  Values that are not symmetric — a softmax over each row — must not ride an
        undirected container, whose dx gathers and factor-2 link form assume a_ij = a_ji.  A container that already has
        a transposed CSR returns itself."""
        if not self.undirected:
            return self
        perm = self.mirror_perm.long()
        new = copy.copy(self)
        new.indptr_t, new.indices_t = self.indptr.clone(), self.indices.clone()
        if self.is_batch:
            new.indices_t_local = self.indices_local.clone()
        if self.weighted:
            new.values_t = self.values.detach()[perm] if self.nnz else self.values.detach().clone()
        new.__dict__["_t_perm"], new.__dict__["mirror_perm"] = perm, self.mirror_perm      # the same pattern: nothing to redo
        return new

    def sym_normalized(self, check=False):
        """`self.with_values(ops.csr_sym_normalize(self.values, self))`: D^-1/2 A D^-1/2 of the stored values (ones for a
        0/1 container) on the device (dp_csr_sym_norm_*), the degree the column sum as in `normalized()`; no read-back,
        and differentiable when `values` require grad.  check=True reads one flag back and raises ValueError as
        `normalized()` does for a node of degree <= 0; without it such a node gives inf / NaN as the reference does."""
        stored = None if not self.weighted else (self.values if self.values.numel() == self.nnz else self.values[:self.nnz])
        values, rdeg = ops.csr_sym_normalize_rdeg(stored, self)
        if check and not bool(torch.isfinite(rdeg).all()):                              # the one flag read back
            bad = torch.nonzero(~torch.isfinite(rdeg)).reshape(-1)
            raise ValueError(f"{type(self).__name__}.sym_normalized(): node {int(bad[0])} has degree <= 0 (column sum of "
                             f"the stored values; {bad.numel()} such node(s)): D^-1/2 A D^-1/2 is not defined there")
        return self.with_values(values)

    def with_values(self, values):
        """A new container with the same index arrays and tables (a shallow copy: shared, not copied) and `values` —
        fp32 [nnz] on the indices' device, in the order of `indices` — as its stored entries; a 0/1 container becomes
        weighted.  `values` may carry autograd history: every op that reads the adjacency then returns its gradient
        (each stored entry an independent variable, also (i, j) and (j, i) of an undirected container).
        `values_t` stays data: `values` itself for an undirected container, else `values[perm]` with the permutation
        between the two CSRs computed once on the host and cached.  An edgeless batch keeps its one-element pad (pass an
        empty tensor)."""
        what = f"{type(self).__name__}.with_values: values"
        nnz = self.nnz
        if nnz == 0 and isinstance(values, torch.Tensor) and values.numel() == 0:      # an edgeless batch keeps its pad
            _check_values(values, self.indices[:0], what)
            values = torch.zeros(self.indices.numel(), device=self.indices.device, dtype=torch.float32)
        else:
            values = _check_values(values, self.indices[:nnz] if nnz else self.indices, what)
        perm = None if self.undirected else self._t_perm          # cached on `self` BEFORE the copy: shared from then on
        new = copy.copy(self)
        new.weighted = True
        new.values = values
        new.values_t = values if perm is None else values.detach()[perm]      # data: it only feeds the dx / dS gathers
        return new

    def normalized(self):
        """A new weighted container holding D^-1/2 A D^-1/2 (of every graph of a batch) — what GraphSampler(normalize=True)
        feeds the dense model (graph_sampler.py:27-29; `tu_dataset.normalized_adjacency`): the degree is the column sum
        of the stored values (ones for a 0/1 container), as the reference takes it (axis=0).  Computed once on the host
        in float64 and rounded to fp32; everything but `values` / `values_t` is shared with this container.  A node of
        degree 0 raises ValueError."""
        val, val_t = _normalized_values(self.n, _read_back(self), type(self).__name__)
        pad = np.zeros(int(self.is_batch and val.size == 0), dtype=np.float32)      # the one-element pad of an edgeless batch
        dev = self.indices.device
        new = copy.copy(self)
        new.weighted = True
        new.values = torch.from_numpy(np.concatenate([val, pad])).to(dev)
        new.values_t = new.values if val_t is None else torch.from_numpy(np.concatenate([val_t, pad])).to(dev)
        return new


class CsrGraph(CsrContainer):
    """CSR of one graph's adjacency on the device: int32 indptr [n + 1], indices [nnz] — row i lists the j with
    A[i, j] != 0 (0/1 adjacency, graph_sampler.py:26) — plus the CSR of A^T for the backward gather (the same arrays
    for an undirected graph).  `values` (fp32 [nnz] on the device, in the order of `indices`; `values_t` in the order
    of `indices_t`, the same tensor for an undirected graph) makes it a weighted adjacency: A[i, indices[e]] =
    values[e], stored zeros allowed.  `weighted` tells which.

    `bn_relu`, `readout`, `pool` and `link_loss` are the four steps of the DiffPool model that differ between one graph
    and a `CsrBatch`; `ARG` and `rows()` are how the model's messages name the container and its node rows."""

    ARG = "graph"

    def __init__(self, indptr, indices, indptr_t=None, indices_t=None, values=None, values_t=None):
        self.indptr, self.indices = indptr, indices
        self.indptr_t = indptr if indptr_t is None else indptr_t
        self.indices_t = indices if indices_t is None else indices_t
        self.n = indptr.numel() - 1
        self._set_values(values, values_t, "CsrGraph")

    # the batch-of-one view (no padding) for the ops that take either container; the offsets are made on first use
    num_graphs = 1
    pad_to = property(lambda self: self.n)
    node_off_host = cached_property(lambda self: np.array([0, self.n], dtype=np.int32))
    node_off = cached_property(lambda self: torch.from_numpy(self.node_off_host).to(self.indptr.device))

    def rows(self):
        return f"[n, F] with n = {self.n}"

    def bn_relu(self, h, layer):
        """apply_bn after ReLU behind GraphConv `layer`: dp_bn_node_* with B = 1."""
        return ops.bn_relu_nodes(h)

    def readout(self, z):
        """Max over the node rows -> (out [1, D], arg-max rows [1, D]): dp_masked_max_*."""
        return ops.row_max(z)

    def pool(self, s, z):
        """S^T Z [1, K, D] and S^T A S [1, K, K] (dp_csr_pool_*), shaped as the one-graph dense batch the pooled
        levels run on."""
        xp, ap = ops.csr_pool(s, z, self)
        return xp.unsqueeze(0), ap.unsqueeze(0)

    def link_loss(self, s, objective="bce"):
        """The link term of the assignment s [n, K]: the reference's cross-entropy form, or 'frobenius'."""
        return ops.frob_link_loss(s, self) if objective == "frobenius" else ops.csr_link_loss(s, self)

    @staticmethod
    def from_edges(n, src, dst, device, symmetric=True, weight=None):
        """Edge list -> CSR (both directions when symmetric, duplicates removed, no self loops added).  `weight`: one
        value per edge (mirrored when symmetric; zeros are stored) -> a weighted graph; an (i, j) given twice with two
        different weights — also as (i, j) and (j, i) under symmetric=True — raises, with the same weight it is
        merged."""
        h = _host_csr(n, src, dst, symmetric, weight)
        return CsrGraph(*(None if a is None else torch.from_numpy(a).to(device) for a in h))

    @staticmethod
    def from_device_csr(n, indptr, indices, indptr_t=None, indices_t=None, values=None, values_t=None, nnz=None):
        """One graph from index arrays that already live on a device (`ops.csr_topk_pool` builds them there): int32
        `indptr` [n + 1] and `indices` (ascending and unique in a row), the transposed pair for a directed graph, `values`
        / `values_t` beside them for a weighted one.  Nothing is read back and nothing is checked beyond shapes, dtypes
        and devices.  `nnz`: the stored entries when the caller knows them (it fills the `nnz` cache)."""
        what = "CsrGraph.from_device_csr"
        if (indptr_t is None) != (indices_t is None):
            raise ValueError(f"{what}: indptr_t and indices_t come together")
        named = (("indptr", indptr), ("indices", indices), ("indptr_t", indptr_t), ("indices_t", indices_t))
        _check_device_arrays(what, named if indptr_t is not None else named[:2], indptr, int(n), "n")
        if nnz is not None and int(nnz) != indices.numel():
            raise ValueError(f"{what}: nnz = {nnz} but indices holds {indices.numel()} entries")
        g = CsrGraph(indptr, indices, indptr_t, indices_t, values, values_t)
        if nnz is not None:
            g.__dict__["nnz"] = int(nnz)
        return g

    @staticmethod
    def from_dense(adj, weighted=False):
        """[n, n] tensor (any device) -> CSR on adj's device (testing aid); weighted=True keeps the nonzero values."""
        a = adj.detach().cpu().numpy()
        r, c = np.nonzero(a != 0)
        return CsrGraph.from_edges(a.shape[0], r, c, adj.device, symmetric=False,
                                   weight=a[r, c].astype(np.float32) if weighted else None)


class _PoolPlan:
    """Device tables of dp_csr_pool_batch_* for one (K, D): see dp_csr_pool_batch_plan."""

    def __init__(self, node_off_host, k, d, device):
        lib = _lib.load()
        b = node_off_host.size - 1
        counts = np.zeros(2, dtype=np.int32)
        off = node_off_host.ctypes.data
        _lib.check(lib.dp_csr_pool_batch_plan(off, b, k, d, None, None, None, counts.ctypes.data),
                   "dp_csr_pool_batch_plan")
        self.n_slabs, self.n_blocks = int(counts[0]), int(counts[1])
        fwd = np.zeros((self.n_slabs, 4), dtype=np.int32)
        soff = np.zeros(b + 1, dtype=np.int32)
        bwd = np.zeros((self.n_blocks, 4), dtype=np.int32)
        _lib.check(lib.dp_csr_pool_batch_plan(off, b, k, d, fwd.ctypes.data, soff.ctypes.data, bwd.ctypes.data,
                                              counts.ctypes.data), "dp_csr_pool_batch_plan")
        self.fwd_tab = torch.from_numpy(fwd).to(device)
        self.slab_off = torch.from_numpy(soff).to(device)
        self.bwd_tab = torch.from_numpy(bwd).to(device)


class CsrBatch(CsrContainer):
    """A RAGGED batch of B graphs on the device: node rows concatenated without padding (graph b owns rows
    node_off[b] .. node_off[b+1]-1 of every [n_total, .] tensor), standing for the dense batch of the same graphs padded
    to `pad_to` nodes (default: max_b n_b).

    Fields: `num_graphs`, `num_nodes` (host int array [B]), `node_off` (int32 [B+1] on the device) / `node_off_host`,
    `n_total`, `max_n`, `min_n`, `pad_to`, `n_idx`.  The adjacency is one block-diagonal CSR: `indptr` [n_total+1] with `indices` holding
    GLOBAL columns (rows of the concatenated tensors: GraphConv, pooling) and `indices_local` graph-local ones (link
    loss); `indptr_t` / `indices_t` / `indices_t_local` the CSR of A^T — the same tensors unless a graph is directed.
    A batch is `weighted` if any of its graphs is (the others get ones): `values` / `values_t`, fp32 in the order of
    `indices` / `indices_t`, serve the global and the graph-local index arrays alike.

    `pad_to` only decides which graphs get the max readout's zero floor (n_b < pad_to: the dense batch has a masked
    zero row for them); host code that knows `max_num_nodes` reproduces a dense run at that padding with it.  Everything
    the kernels need is laid out here, once: the size order and owner counts of the node-index BatchNorm, the row
    chunks of the segmented max, the floor flags, and (on first use per (K, D), then cached) the pooling's slab tables."""

    SEG_ROWS = 128          # rows per chunk of the segmented max readout
    ARG = "batch"
    is_batch = True
    _UNDIRECTED = "an undirected batch"
    _DIRECTED = "a weighted batch with a transposed CSR"

    def __init__(self, sizes, parts, device, pad_to=None):
        """`parts`: per graph a `HostCsr`, or a plain (indptr, indices, indptr_t, indices_t[, values, values_t]): host
        arrays with graph-local columns, the transposed pair None for an undirected graph; values (float, one per stored
        entry; values_t next to a transposed pair) or None / absent for a 0/1 graph.  Use the from_* constructors."""
        sizes = self._init_sizes(sizes, len(parts), device, pad_to)
        parts = [p if isinstance(p, HostCsr) else HostCsr(*p) for p in parts]
        directed = any(p.indptr_t is not None for p in parts)
        self.weighted = any(p.values is not None for p in parts)

        def stack(transposed):
            ips, loc, glob, vals, e0 = [], [], [], [], 0
            for b, p in enumerate(parts):
                own = transposed and p.indptr_t is not None          # an undirected graph's A^T is its A
                ip, ix, v = (p.indptr_t, p.indices_t, p.values_t) if own else (p.indptr, p.indices, p.values)
                ip, ix = np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int64)
                n = int(sizes[b])
                if ip.size != n + 1 or ip[0] != 0 or ip[-1] != ix.size or (np.diff(ip) < 0).any():
                    raise ValueError(f"CsrBatch: graph {b}: indptr does not describe {n} rows over {ix.size} entries")
                if ix.size and (ix.min() < 0 or ix.max() >= n):
                    raise ValueError(f"CsrBatch: graph {b}: column index outside 0..{n - 1}")
                if self.weighted:
                    if v is None:
                        if p.values is not None:
                            raise ValueError(f"CsrBatch: graph {b}: a weighted graph with a transposed CSR needs values_t")
                        v = np.ones(ix.size, dtype=np.float32)
                    v = np.asarray(v)
                    if v.ndim != 1 or v.size != ix.size:
                        raise ValueError(f"CsrBatch: graph {b}: {v.size} values for {ix.size} stored entries")
                    if not np.issubdtype(v.dtype, np.floating):
                        raise ValueError(f"CsrBatch: graph {b}: values must be floating point, got {v.dtype}")
                    vals.append(v.astype(np.float32))
                ips.append(ip[:-1] + e0)
                loc.append(ix)
                glob.append(ix + int(self.node_off_host[b]))
                e0 += ix.size
            if e0 >= 2 ** 31:
                raise ValueError("CsrBatch: more than 2^31 - 1 edges in one batch")
            ips.append(np.array([e0]))
            pad = [np.zeros(1, dtype=np.int64)] if e0 == 0 else []      # the kernels want non-NULL index arrays
            dev = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int32)).to(self.device)
            val = None
            if self.weighted:
                fpad = [np.zeros(1, dtype=np.float32)] if e0 == 0 else []
                val = torch.from_numpy(np.concatenate(vals + fpad).astype(np.float32)).to(self.device)
            return dev(ips), dev(glob + pad), dev(loc + pad), val

        self.indptr, self.indices, self.indices_local, self.values = stack(False)
        if directed:
            self.indptr_t, self.indices_t, self.indices_t_local, self.values_t = stack(True)
        else:
            self.indptr_t, self.indices_t, self.indices_t_local = self.indptr, self.indices, self.indices_local
            self.values_t = self.values
        self._init_tables()

    def _init_sizes(self, sizes, n_parts, device, pad_to):
        """The checks and host numbers every constructor starts with -> sizes as int64 [B].  `n_parts`: how many graphs
        the caller brought (None: it brings device arrays of the whole batch)."""
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        if sizes.size == 0:
            raise ValueError("CsrBatch: no graph")
        if (sizes < 1).any():
            raise ValueError(f"CsrBatch: every graph needs at least one node, got sizes {sizes.tolist()}")
        if n_parts is not None and n_parts != sizes.size:
            raise ValueError(f"CsrBatch: {sizes.size} sizes but {n_parts} graphs")
        if int(sizes.sum()) >= 2 ** 31:
            raise ValueError("CsrBatch: more than 2^31 - 1 nodes in one batch")
        self.num_graphs = int(sizes.size)
        self.num_nodes = sizes.astype(np.int64)
        self.max_n = int(sizes.max())
        self.pad_to = self.max_n if pad_to is None else int(pad_to)
        if self.pad_to < self.max_n:
            raise ValueError(f"CsrBatch: pad_to = {self.pad_to} is below the largest graph ({self.max_n} nodes)")
        self.node_off_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.n_total = self.n = int(self.node_off_host[-1])
        self.device = torch.device(device)
        return sizes

    def _init_tables(self, node_off=None):
        """The host-made tables of the kernels, from the sizes alone: `node_off`, the size order and owner counts of the
        node-index BatchNorm, the floor flags, the row chunks of the segmented max, the pool-plan cache.  `node_off`: the
        offsets when the caller already has them on the device."""
        sizes = self.num_nodes
        self.node_off = torch.from_numpy(self.node_off_host).to(self.device) if node_off is None else node_off
        # node-index BatchNorm: graphs by size, largest first; cnt[i] = graphs with n_b > i
        order = np.argsort(-sizes, kind="stable")
        asc = np.sort(sizes)
        cnt = self.num_graphs - np.searchsorted(asc, np.arange(self.max_n), side="right")
        self.order = torch.from_numpy(order.astype(np.int32)).to(self.device)
        self.cnt = torch.from_numpy(cnt.astype(np.int32)).to(self.device)
        self.has_padding = bool((sizes < self.max_n).any())
        # the unmasked readout's table of padded-row values: node indices min_n .. n_idx - 1 have a padded row in the
        # dense batch; row max_n (there when pad_to > max_n) stands for every index from max_n up
        self.min_n = int(sizes.min())
        self.n_idx = self.max_n + int(self.pad_to > self.max_n)
        self.floor_flag = torch.from_numpy((sizes < self.pad_to).astype(np.int32)).to(self.device)
        # segmented max: row chunks that never cross a graph boundary
        tab, seg_off = [], [0]
        for b in range(self.num_graphs):
            lo, hi = int(self.node_off_host[b]), int(self.node_off_host[b + 1])
            for r in range(lo, hi, self.SEG_ROWS):
                tab.append((b, r, min(hi, r + self.SEG_ROWS), 0))
            seg_off.append(len(tab))
        self.seg_chunks = len(tab)
        self.seg_tab = torch.from_numpy(np.asarray(tab, dtype=np.int32)).to(self.device)
        self.seg_off = torch.from_numpy(np.asarray(seg_off, dtype=np.int32)).to(self.device)
        self._pool_plans = {}

    def pool_plan(self, k, d):
        """Slab / row-block tables of the batched pooling for cluster count k and embedding width d (built once)."""
        plan = self._pool_plans.get((k, d))
        if plan is None:
            plan = self._pool_plans[(k, d)] = _PoolPlan(self.node_off_host, k, d, self.device)
        return plan

    # -- the four steps of the DiffPool model that differ from a single CsrGraph's
    def rows(self):
        return f"[n_total, F] with n_total = {self.n_total} (the batch's graphs concatenated)"

    def bn_relu(self, h, layer):
        """apply_bn after ReLU behind GraphConv `layer`, per node index over the batch: the padded rows of the dense
        batch enter the statistics as the layer's constant relu(l2norm(bias)) (dp_bn_ragged_*), whose gradient flows
        back into the bias."""
        if layer.add_self:
            raise NotImplementedError("add_self GraphConv layers (concat=False) on a CsrBatch: a padded row of the dense "
                                      "batch is then not a constant of the layer")
        pad = ops.gcn_pad_const(layer.bias, layer._flags()) if self.has_padding and layer.bias is not None else None
        return ops.bn_relu_ragged(h, pad, self)

    def readout(self, z):
        """Max over each graph's rows, with the zero floor of a graph that has padded rows -> (out [B, D], graph-local
        arg-max rows [B, D]): dp_segment_max_*."""
        return ops.segment_max(z, self)

    def pool(self, s, z):
        """Per graph S^T Z [B, K, D] and S^T A S [B, K, K]: dp_csr_pool_batch_*."""
        return ops.csr_pool_batch(s, z, self)

    def link_loss(self, s, objective="bce"):
        """The link term of the ragged assignment s [n_total, K]: the reference's cross-entropy form (per-graph
        launches), or 'frobenius' (one set of launches for the batch)."""
        return ops.frob_link_loss(s, self) if objective == "frobenius" else ops.csr_link_loss_batch(s, self)

    @staticmethod
    def from_graphs(graphs, pad_to=None):
        """A batch of existing `CsrGraph`s (their arrays are read back to the host once)."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("CsrBatch: no graph")
        for g in graphs:
            if not isinstance(g, CsrGraph):
                raise TypeError(f"CsrBatch.from_graphs: expected CsrGraph, got {type(g).__name__}")
        return CsrBatch([g.n for g in graphs], [_read_back(g) for g in graphs], graphs[0].indptr.device, pad_to=pad_to)

    @staticmethod
    def from_edge_lists(sizes, srcs, dsts, device, symmetric=True, pad_to=None, weights=None):
        """Per graph an edge list (graph-local node ids) -> the batch; `symmetric` as in `CsrGraph.from_edges`.
        `weights`: per graph the edges' weights (`CsrGraph.from_edges`' `weight`), or None for a 0/1 graph."""
        if weights is None:
            weights = [None] * len(sizes)
        if not (len(sizes) == len(srcs) == len(dsts) == len(weights)):
            raise ValueError("CsrBatch.from_edge_lists: sizes, srcs, dsts (and weights) must have one entry per graph")
        parts = [_host_csr(int(n), src, dst, symmetric, w) for n, src, dst, w in zip(sizes, srcs, dsts, weights)]
        return CsrBatch(sizes, parts, device, pad_to=pad_to)

    @staticmethod
    def from_device_csr(sizes, indptr, indices, indices_local, indptr_t=None, indices_t=None, indices_t_local=None,
                        values=None, values_t=None, pad_to=None, nnz=None, node_off=None):
        """A batch from index arrays that already live on a device (`ops.csr_topk_pool` builds them there) plus the host
        sizes: the block-diagonal CSR as the class stores it — int32 `indptr` [n_total + 1], `indices` (GLOBAL columns,
        ascending and unique in a row, inside the row's graph), `indices_local` (minus the graph's offset), an edgeless
        batch padded to one element — and, for a directed batch, the transposed trio; `values` / `values_t` beside them
        for a weighted one.  Nothing is read back and nothing is checked beyond shapes, dtypes and devices: the arrays
        are trusted as the kernels' own output is.  `nnz`: the stored entries when the caller knows them (it fills the
        `nnz` cache); `node_off`: int32 [B + 1] on the device when the caller has it.  Every host table is made from
        `sizes` exactly as the other constructors make it."""
        what = "CsrBatch.from_device_csr"
        self = CsrBatch.__new__(CsrBatch)
        self._init_sizes(sizes, None, indptr.device, pad_to)
        trios = [(("indptr", indptr), ("indices", indices), ("indices_local", indices_local))]
        if (indptr_t is None) != (indices_t is None) or (indptr_t is None) != (indices_t_local is None):
            raise ValueError(f"{what}: indptr_t, indices_t and indices_t_local come together")
        if indptr_t is not None:
            trios.append((("indptr_t", indptr_t), ("indices_t", indices_t), ("indices_t_local", indices_t_local)))
        for trio in trios:
            _check_device_arrays(what, trio, indptr, self.n_total, "n_total")
            (_, _), (gn, ix), (ln, il) = trio
            if ix.numel() != il.numel() or ix.numel() < 1:
                raise ValueError(f"{what}: {gn} and {ln} must hold the same entries, one at least (an edgeless batch "
                                 f"keeps a one-element pad), got {ix.numel()} and {il.numel()}")
        if nnz is not None and not (int(nnz) == indices.numel() or (int(nnz) == 0 and indices.numel() == 1)):
            raise ValueError(f"{what}: nnz = {nnz} but indices holds {indices.numel()} entries")
        self.indptr, self.indices, self.indices_local = indptr, indices, indices_local
        if indptr_t is None:
            self.indptr_t, self.indices_t, self.indices_t_local = indptr, indices, indices_local
        else:
            self.indptr_t, self.indices_t, self.indices_t_local = indptr_t, indices_t, indices_t_local
        self._set_values(values, values_t, what)
        if node_off is not None and (node_off.dtype != torch.int32 or node_off.numel() != self.num_graphs + 1
                                     or node_off.device != indptr.device):
            raise ValueError(f"{what}: node_off must be int32 [B + 1] on the arrays' device")
        self._init_tables(node_off)
        if nnz is not None:
            self.__dict__["nnz"] = int(nnz)
        return self

    @staticmethod
    def from_dense(adj, num_nodes, pad_to=None, weighted=False):
        """[B, N, N] tensor (any device) + node counts -> the batch on adj's device, reading only the leading
        n_b x n_b block of each graph (testing aid, like `CsrGraph.from_dense`); weighted=True keeps the nonzero
        values."""
        a = adj.detach().cpu().numpy()
        nn_ = np.asarray(num_nodes, dtype=np.int64).reshape(-1)
        if a.ndim != 3 or a.shape[0] != nn_.size or a.shape[1] != a.shape[2]:
            raise ValueError(f"CsrBatch.from_dense: adj {tuple(a.shape)} does not match {nn_.size} node counts")
        if (nn_ > a.shape[1]).any():
            raise ValueError("CsrBatch.from_dense: a node count exceeds the padded size")
        srcs, dsts, ws = [], [], []
        for b, n in enumerate(nn_):
            r, c = np.nonzero(a[b, :n, :n] != 0)
            srcs.append(r)
            dsts.append(c)
            ws.append(a[b, :n, :n][r, c].astype(np.float32) if weighted else None)
        return CsrBatch.from_edge_lists(nn_, srcs, dsts, adj.device, symmetric=False, pad_to=pad_to, weights=ws)
