"""GCN graph encoder on CSR graphs — for graphs beyond the padded dense path.

The reference pads every graph to `max_nodes` and DROPS the ones above it (load_data.py:79: `if max_nodes is not None
and G.number_of_nodes() > max_nodes: continue`); DD's largest graph has 5 748 nodes (132 MB as a dense fp32 block).
`SparseGcnEncoderGraph` runs the same model as `GcnEncoderGraph` (encoders.py:976-1134: GraphConv -> ReLU -> apply_bn per
layer, max readout per layer, concat, pred_model) on ONE graph given as CSR, so such graphs can be classified with
the parameters trained on the dense path: same constructor arguments, same `state_dict` keys, and on a graph that
fits the dense path the same numbers (tests/test_gpu_sparse.py checks it against the oracle's dense restatement).

The neighbour sum  A x  is the CSR gather of dp_csr_aggregate (the MeanAggregator's kernel with mean = 0,
aggregators.py:50-62), the transform, bias, l2-normalisation and their backward the kernels of the dense path
(dp_sparse_gcn_layer_fwd / bwd); apply_bn on a single graph is dp_bn_node_* with B = 1; the Linear layers of the
prediction head run on dp_bgemm_f32 (`hip_linear`).  No torch arithmetic on the path.  The autograd wrappers of these
entries live in `ops.py`; this module holds the CSR containers and the model classes.

`SparseBatchGcnEncoderGraph` is the same base model on a ragged `CsrBatch`.  The base class's max readout is unmasked,
so in the dense batch the padded rows compete: behind apply_bn a padded row holds the layer's constant pushed through
the statistics of its node index, and a small graph's readout is often such a value.  The subclass keeps a table of
those values per node index (dp_ragged_padval_fwd), takes its suffix maximum (dp_ragged_suffix_max) as the floor of
the segmented max (dp_segment_max_floor_*), and sends a padded winner's gradient back through its node index's
statistics (dp_bn_ragged_g_bwd) and into the bias (dp_gcn_pad_const_* / dp_gcn_row_const_*).  The parent class keeps
refusing a batch, and says so.

`SparseGcnSet2SetEncoder` is `GcnSet2SetEncoder` on either container: the GCN stack as above, the embedding mask for
free (a ragged batch stores no padded row, and the dense batch's are zero behind the mask), and the Set2Set readout
on dp_set2set_ragged_*, where the zero rows of the dense batch are one closed-form term of every step's softmax.

`SparseSoftPoolingGcnEncoder` does the same for DiffPool (`SoftPoolingGcnEncoder`) on one `CsrGraph` or on a ragged
`CsrBatch`, in ONE forward and one loss.  The two containers differ in four steps, each a method of the container:
`bn_relu` (dp_bn_node_* / dp_bn_ragged_*), `readout` (dp_masked_max_* / dp_segment_max_*), `pool` — S^T Z, S^T A S,
encoders.py:1278-1279 — (dp_csr_pool_* / dp_csr_pool_batch_*) and `link_loss` — encoders.py:1309-1331, never forming
an n x n adjacency — (dp_csr_linkpred_loss_* / dp_csr_linkpred_batch_*).  A single graph is NOT a batch of one: it
keeps its own kernels.  The small pooled levels run on the dense per-op entries as a dense batch [B, K, .], B = 1
behind a CsrGraph.

`EdgeAttention` computes the stored values of either container from the node features — scores on the stored entries
(dp_csr_sddmm), a softmax over each neighbour list (dp_csr_edge_softmax_*) or a symmetric gate under D^-1/2 A D^-1/2
(dp_csr_sym_norm_*), or GAT's additive multi-head scores with their softmax and head mean in one fused pass
(dp_csr_gat_*) — and hands the three encoders a weighted container through which its projections train.

`SageConv` / `SageEncoder` are GraphSAGE's mean-aggregator layer and the encoder `SupervisedGraphSage` expects, on either
container, with the neighbour sample drawn on the device in the launch that takes its mean (dp_csr_sample_mean_*).

`TopKPooling` is the hard pooling next to DiffPool's soft one (gPool / SAGPool): it keeps the best-scored nodes of every
graph and returns the induced subgraph as a container of the input's class, built on the device (dp_csr_topk_*) and
wrapped by `CsrGraph.from_device_csr` / `CsrBatch.from_device_csr`, so it feeds everything above.
"""
from __future__ import annotations

import copy
from functools import cached_property
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .encoders import (GcnEncoderGraph, GcnSet2SetEncoder, SoftPoolingGcnEncoder, _refuse_ent_under_sync_bn,
                       _refuse_frob_under_sync_bn)
from .ops import hip_linear  # noqa: F401  (tests and tools import it from here)


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
    undirected = g.indptr_t is g.indptr and g.indices_t is g.indices
    ipt, ixt, valt = (None, None, None) if undirected else trio(g.indptr_t, g.indices_t, g.values_t)
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
    if g.indices_t is not g.indices:
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


def _directed(g):
    """`CsrGraph.directed` / `CsrBatch.directed`."""
    if g.indices_t is not g.indices:
        return g
    perm = g.mirror_perm.long()
    new = copy.copy(g)
    new.indptr_t, new.indices_t = g.indptr.clone(), g.indices.clone()
    if hasattr(g, "indices_local"):
        new.indices_t_local = g.indices_local.clone()
    if g.weighted:
        new.values_t = g.values.detach()[perm] if g.nnz else g.values.detach().clone()
    new.__dict__["_t_perm"], new.__dict__["mirror_perm"] = perm, g.mirror_perm      # the same pattern: nothing to redo
    return new


def _sym_normalized(g, check):
    """`CsrGraph.sym_normalized` / `CsrBatch.sym_normalized`."""
    stored = None if not g.weighted else (g.values if g.values.numel() == g.nnz else g.values[:g.nnz])
    values, rdeg = ops.csr_sym_normalize_rdeg(stored, g)
    if check and not bool(torch.isfinite(rdeg).all()):                              # the one flag read back
        bad = torch.nonzero(~torch.isfinite(rdeg)).reshape(-1)
        raise ValueError(f"{type(g).__name__}.sym_normalized(): node {int(bad[0])} has degree <= 0 (column sum of the "
                         f"stored values; {bad.numel()} such node(s)): D^-1/2 A D^-1/2 is not defined there")
    return g.with_values(values)


def _with_values(g, values):
    """`CsrGraph.with_values` / `CsrBatch.with_values`: a shallow copy of container `g` that shares every index array and
    table and stores `values` (which may carry autograd history)."""
    what = f"{type(g).__name__}.with_values: values"
    nnz = g.nnz
    if nnz == 0 and isinstance(values, torch.Tensor) and values.numel() == 0:      # an edgeless batch keeps its pad
        _check_values(values, g.indices[:0], what)
        values = torch.zeros(g.indices.numel(), device=g.indices.device, dtype=torch.float32)
    else:
        values = _check_values(values, g.indices[:nnz] if nnz else g.indices, what)
    perm = None if g.indices_t is g.indices else g._t_perm          # cached on `g` BEFORE the copy: shared from then on
    new = copy.copy(g)
    new.weighted = True
    new.values = values
    new.values_t = values if perm is None else values.detach()[perm]      # data: it only feeds the dx / dS gathers
    return new


class CsrGraph:
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
        self.weighted = values is not None
        self.values = self.values_t = None
        if values is None:
            if values_t is not None:
                raise ValueError("CsrGraph: values_t without values")
            return
        self.values = _check_values(values, indices, "CsrGraph: values")
        if self.indices_t is self.indices:
            if values_t is not None and values_t is not values:
                raise ValueError("CsrGraph: an undirected graph (no transposed CSR of its own) stores a_ij = a_ji: "
                                 "values_t must be values or None")
            self.values_t = self.values
        elif values_t is None:
            raise ValueError("CsrGraph: a weighted graph with a transposed CSR of its own needs values_t")
        else:
            self.values_t = _check_values(values_t, self.indices_t, "CsrGraph: values_t")

    # the batch-of-one view (no padding) for the ops that take either container; the offsets are made on first use
    num_graphs = 1
    pad_to = property(lambda self: self.n)
    node_off_host = cached_property(lambda self: np.array([0, self.n], dtype=np.int32))
    node_off = cached_property(lambda self: torch.from_numpy(self.node_off_host).to(self.indptr.device))

    def rows(self):
        return f"[n, F] with n = {self.n}"

    nnz = cached_property(lambda self: int(self.indptr[-1]))          # stored entries (one read-back, then cached)
    _t_perm = cached_property(_transpose_perm)
    mirror_perm = cached_property(_mirror_perm)

    def directed(self):
        """A container of the same class with a transposed CSR of its OWN: cloned index arrays and `values_t =
        values[mirror_perm]` (data).  Values that are not symmetric — a softmax over each row — must not ride an
        undirected container, whose dx gathers and factor-2 link form assume a_ij = a_ji.  A container that already has
        a transposed CSR returns itself."""
        return _directed(self)

    def sym_normalized(self, check=False):
        """`self.with_values(ops.csr_sym_normalize(self.values, self))`: D^-1/2 A D^-1/2 of the stored values (ones for a
        0/1 container) on the device (dp_csr_sym_norm_*), the degree the column sum as in `normalized()`; no read-back,
        and differentiable when `values` require grad.  check=True reads one flag back and raises ValueError as
        `normalized()` does for a node of degree <= 0; without it such a node gives inf / NaN as the reference does."""
        return _sym_normalized(self, check)

    def with_values(self, values):
        """A new container with the same index arrays (shared, not copied) and `values` — fp32 [nnz] on the indices'
        device, in the order of `indices` — as its stored entries; a 0/1 container becomes weighted.  `values` may carry
        autograd history: every op that reads the adjacency then returns its gradient (each stored entry an independent
        variable, also (i, j) and (j, i) of an undirected container).  `values_t` stays data: `values` itself
        for an undirected container, else `values[perm]` with the permutation between the two CSRs computed once on the
        host and cached.  An edgeless batch keeps its one-element pad (pass an empty tensor)."""
        return _with_values(self, values)

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
        if (indptr_t is None) != (indices_t is None):
            raise ValueError("CsrGraph.from_device_csr: indptr_t and indices_t come together")
        for name, t in (("indptr", indptr), ("indices", indices), ("indptr_t", indptr_t), ("indices_t", indices_t)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"CsrGraph.from_device_csr: {name} must be a contiguous 1-d int32 tensor")
            if t.device != indptr.device:
                raise ValueError(f"CsrGraph.from_device_csr: {name} is on {t.device}, indptr on {indptr.device}")
            if name.startswith("indptr") and t.numel() != int(n) + 1:
                raise ValueError(f"CsrGraph.from_device_csr: {name} must hold n + 1 = {int(n) + 1} offsets, got {t.numel()}")
        if nnz is not None and int(nnz) != indices.numel():
            raise ValueError(f"CsrGraph.from_device_csr: nnz = {nnz} but indices holds {indices.numel()} entries")
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

    def normalized(self):
        """A new weighted graph holding D^-1/2 A D^-1/2 — what GraphSampler(normalize=True) feeds the dense model
        (graph_sampler.py:27-29; `tu_dataset.normalized_adjacency`): the degree is the column sum of the stored values
        (ones for a 0/1 graph), as the reference takes it (axis=0).  Computed once on the host in float64 and rounded
        to fp32; the index arrays are shared.  A node of degree 0 raises ValueError."""
        val, val_t = (torch.from_numpy(v).to(self.indices.device) if v is not None else None
                      for v in _normalized_values(self.n, _read_back(self), "CsrGraph"))
        if self.indices_t is self.indices:
            return CsrGraph(self.indptr, self.indices, values=val)
        return CsrGraph(self.indptr, self.indices, self.indptr_t, self.indices_t, val, val_t)


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


class CsrBatch:
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

    nnz = cached_property(lambda self: int(self.indptr[-1]))          # stored entries (one read-back, then cached)
    _t_perm = cached_property(_transpose_perm)
    mirror_perm = cached_property(_mirror_perm)

    def directed(self):
        """A container of the same class with a transposed CSR of its OWN: cloned index arrays and `values_t =
        values[mirror_perm]` (data).  Values that are not symmetric — a softmax over each row — must not ride an
        undirected container, whose dx gathers and factor-2 link form assume a_ij = a_ji.  A container that already has
        a transposed CSR returns itself."""
        return _directed(self)

    def sym_normalized(self, check=False):
        """`self.with_values(ops.csr_sym_normalize(self.values, self))`: D^-1/2 A D^-1/2 of the stored values (ones for a
        0/1 container) on the device (dp_csr_sym_norm_*), the degree the column sum as in `normalized()`; no read-back,
        and differentiable when `values` require grad.  check=True reads one flag back and raises ValueError as
        `normalized()` does for a node of degree <= 0; without it such a node gives inf / NaN as the reference does."""
        return _sym_normalized(self, check)

    def with_values(self, values):
        """A new container with the same index arrays (shared, not copied) and `values` — fp32 [nnz] on the indices'
        device, in the order of `indices` — as its stored entries; a 0/1 container becomes weighted.  `values` may carry
        autograd history: every op that reads the adjacency then returns its gradient (each stored entry an independent
        variable, also (i, j) and (j, i) of an undirected container).  `values_t` stays data: `values` itself
        for an undirected container, else `values[perm]` with the permutation between the two CSRs computed once on the
        host and cached.  An edgeless batch keeps its one-element pad (pass an empty tensor)."""
        return _with_values(self, values)

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
        self = CsrBatch.__new__(CsrBatch)
        self._init_sizes(sizes, None, indptr.device, pad_to)
        trios = [("indptr", indptr, "indices", indices, "indices_local", indices_local)]
        if (indptr_t is None) != (indices_t is None) or (indptr_t is None) != (indices_t_local is None):
            raise ValueError("CsrBatch.from_device_csr: indptr_t, indices_t and indices_t_local come together")
        if indptr_t is not None:
            trios.append(("indptr_t", indptr_t, "indices_t", indices_t, "indices_t_local", indices_t_local))
        for pn, ip, gn, ix, ln, il in trios:
            for name, t in ((pn, ip), (gn, ix), (ln, il)):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                    raise ValueError(f"CsrBatch.from_device_csr: {name} must be a contiguous 1-d int32 tensor")
                if t.device != indptr.device:
                    raise ValueError(f"CsrBatch.from_device_csr: {name} is on {t.device}, indptr on {indptr.device}")
            if ip.numel() != self.n_total + 1:
                raise ValueError(f"CsrBatch.from_device_csr: {pn} must hold n_total + 1 = {self.n_total + 1} offsets, got "
                                 f"{ip.numel()}")
            if ix.numel() != il.numel() or ix.numel() < 1:
                raise ValueError(f"CsrBatch.from_device_csr: {gn} and {ln} must hold the same entries, one at least (an "
                                 f"edgeless batch keeps a one-element pad), got {ix.numel()} and {il.numel()}")
        if nnz is not None and not (int(nnz) == indices.numel() or (int(nnz) == 0 and indices.numel() == 1)):
            raise ValueError(f"CsrBatch.from_device_csr: nnz = {nnz} but indices holds {indices.numel()} entries")
        self.indptr, self.indices, self.indices_local = indptr, indices, indices_local
        self.weighted = values is not None
        self.values = self.values_t = None
        if values is None and values_t is not None:
            raise ValueError("CsrBatch.from_device_csr: values_t without values")
        if values is not None:
            self.values = _check_values(values, indices, "CsrBatch.from_device_csr: values")
        if indptr_t is None:
            if values_t is not None and values_t is not values:
                raise ValueError("CsrBatch.from_device_csr: an undirected batch stores a_ij = a_ji: values_t must be "
                                 "values or None")
            self.indptr_t, self.indices_t, self.indices_t_local = indptr, indices, indices_local
            self.values_t = self.values
        else:
            self.indptr_t, self.indices_t, self.indices_t_local = indptr_t, indices_t, indices_t_local
            if self.weighted:
                if values_t is None:
                    raise ValueError("CsrBatch.from_device_csr: a weighted batch with a transposed CSR needs values_t")
                self.values_t = _check_values(values_t, indices_t, "CsrBatch.from_device_csr: values_t")
        if node_off is not None and (node_off.dtype != torch.int32 or node_off.numel() != self.num_graphs + 1
                                     or node_off.device != indptr.device):
            raise ValueError("CsrBatch.from_device_csr: node_off must be int32 [B + 1] on the arrays' device")
        self._init_tables(node_off)
        if nnz is not None:
            self.__dict__["nnz"] = int(nnz)
        return self

    def normalized(self):
        """A new weighted batch holding D^-1/2 A D^-1/2 of every graph (`CsrGraph.normalized`: column sums of the stored
        values, host float64, a node of degree 0 raises).  Everything but `values` / `values_t` is shared with this
        batch."""
        val, val_t = _normalized_values(self.n_total, _read_back(self), "CsrBatch")
        pad = np.zeros(int(val.size == 0), dtype=np.float32)          # the one-element pad of an edgeless batch
        new = copy.copy(self)
        new.weighted = True
        new.values = torch.from_numpy(np.concatenate([val, pad])).to(self.device)
        new.values_t = new.values if val_t is None else torch.from_numpy(np.concatenate([val_t, pad])).to(self.device)
        return new

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


def _check_node_rows(graph, x, input_dim, assign_x=None, assign_input_dim=None):
    """The forwards' input check: x is a GPU tensor `graph.rows()` of width `input_dim` — and, in the DiffPool forward,
    assign_x one of width `assign_input_dim`."""
    named = (("x", x),) if assign_input_dim is None else (("x", x), ("assign_x", assign_x))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != graph.n:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"expected {name} {graph.rows()}, got {got}")
    if assign_input_dim is None:
        if x.shape[1] != input_dim:
            raise ValueError(f"x has {x.shape[1]} features, the encoder was built for {input_dim}")
    elif x.shape[1] != input_dim or assign_x.shape[1] != assign_input_dim:
        raise ValueError(f"feature widths {x.shape[1]}/{assign_x.shape[1]} do not match the model "
                         f"({input_dim}/{assign_input_dim})")
    for name, t in named:
        _lib.require_gpu_tensor(t, name)


def _cross_entropy_loss(model, pred, label):
    """Cross entropy of the prediction (encoders.py:1124-1127) on dp_cross_entropy_*; label [B] for a batch."""
    if pred.dim() != 2 or not isinstance(label, torch.Tensor) or label.numel() != pred.shape[0]:
        got = label.numel() if isinstance(label, torch.Tensor) else label.__class__.__name__
        raise ValueError(f"{type(model).__name__}.loss(pred, label): label must hold one class per row of pred "
                         f"{tuple(pred.shape)}, got {got}")
    return ops.cross_entropy(pred, label.reshape(-1))


def _gcn_stack(mods, h, graph, bn=True):
    """gcn_forward (encoders.py:1054-1081) on the node rows h [n, F] of a CsrGraph or a CsrBatch: the CSR GraphConv, then
    ReLU -> apply_bn as the container does it (`graph.bn_relu`) for every layer but the last; yields each layer's
    output as soon as it is enqueued."""
    for i, m in enumerate(mods):
        h = ops.csr_graph_conv(h, m.weight, m.bias, graph, m._flags())
        if i < len(mods) - 1:
            h = graph.bn_relu(h, m) if bn else torch.relu(h)      # ReLU is fused into the BN kernel
        yield h


def _gcn_stack_dense(mods, h, adj):
    """`_gcn_stack` on a dense batch h [B, n, F], adj [B, n, n]: the pooled levels (dp_gcn_layer_*, dp_bn_node_*), with
    B = 1 behind a CsrGraph."""
    for i, m in enumerate(mods):
        h = ops.graph_conv(h, adj, m.weight, m.bias, m._flags())
        if i < len(mods) - 1:
            h = ops.bn_relu_nodes(h)
        yield h


class SparseGcnEncoderGraph(GcnEncoderGraph):
    """`GcnEncoderGraph` (encoders.py:976-1134) on one CSR graph: forward(x [n, F], graph) -> ypred [1, label_dim].

    Same constructor arguments and `state_dict` keys as the dense class (it IS the dense class's module tree: conv_first
    / conv_block.i / conv_last / pred_model...), so parameters move between the two with load_state_dict."""

    def __init__(self, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=[], concat=True,
                 bn=True, dropout=0.0, args=None):
        if dropout > 0.001:
            raise NotImplementedError("dropout on the CSR path")
        super().__init__(input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=pred_hidden_dims,
                         concat=concat, bn=bn, dropout=dropout, args=args)

    def forward(self, x, graph: CsrGraph):
        if isinstance(graph, CsrBatch):
            raise TypeError("SparseGcnEncoderGraph takes one CsrGraph per call: its max readout is unmasked, so on a "
                            "batch the padded rows' post-BatchNorm values enter the maximum (a suffix-max over node "
                            "indices), which its subclass SparseBatchGcnEncoderGraph computes; "
                            "SparseSoftPoolingGcnEncoder accepts a CsrBatch too")
        if not isinstance(graph, CsrGraph):
            raise TypeError("SparseGcnEncoderGraph.forward(x [n, F], graph: CsrGraph): the dense (x [B, N, F], adj, "
                            "batch_num_nodes) form is GcnEncoderGraph's")
        if x.dim() != 2 or x.shape[0] != graph.n:
            raise ValueError(f"expected x [n, F] with n = {graph.n}, got {tuple(x.shape)}")
        mods = self._stack_modules(self.conv_first, self.conv_block, self.conv_last)
        outs = [ops.row_max(h)[0] for h in _gcn_stack(mods, x, graph, self.bn)]      # torch.max(x, dim=1), :1093
        return ops.mlp_head(torch.cat(outs, dim=1) if self.concat else outs[-1], self._pred_linears())

    @torch.no_grad()
    def predict(self, x, graph):
        return self.forward(x, graph).argmax(dim=1)


class SparseBatchGcnEncoderGraph(SparseGcnEncoderGraph):
    """`GcnEncoderGraph` on a ragged `CsrBatch`: forward(x [n_total, F], batch) -> ypred [B, label_dim], computing what
    the dense class computes on the same graphs padded to `batch.pad_to` rows, without storing a padded row.  Same
    constructor and `state_dict` keys as the dense class; a `CsrGraph` goes to the parent's forward.

    The base class's readout is UNMASKED (encoders.py:1093: torch.max over all rows, the mask of :1087 is never used),
    so the padded rows of the dense batch compete.  Behind GraphConv -> ReLU -> apply_bn a padded row of node index i
    holds (p - mean_i) rstd_i, p = relu(l2norm(bias)): a different value per node index, and a graph with n_b rows
    sees the maximum over the indices n_b .. pad_to - 1 (`ops.bn_relu_ragged_padval` makes the table, indices from
    max_n up share one row; `ops.segment_max_floor` takes its suffix maximum).  Without BatchNorm every padded row
    holds p, behind the last layer l2norm(bias): one constant row as the floor.  The gradient of a padded winner flows
    through its node index's statistics into every graph that owns the index, and into the layer's bias.

    `saved_activation(layer, 'readout_argmax')` gives the winners of the last batch forward as rows of the DENSE batch.

    Not on this path: concat=False (add_self: a padded row is then not a constant of the layer), dropout."""

    def forward(self, x, graph):
        if not isinstance(graph, CsrBatch):
            self._saved_argmax = None
            return super().forward(x, graph)
        batch = graph
        if not self.concat:
            raise NotImplementedError("add_self GraphConv layers (concat=False) on a CsrBatch: a padded row of the dense "
                                      "batch is then not a constant of the layer")
        _check_node_rows(batch, x, self.input_dim)
        h = x.contiguous().float()
        mods = self._stack_modules(self.conv_first, self.conv_block, self.conv_last)
        floored = batch.n_idx > batch.min_n          # some graph has a padded row in the dense batch
        outs, argmax = [], []
        for i, m in enumerate(mods):
            flags = m._flags()
            h = ops.csr_graph_conv(h, m.weight, m.bias, batch, flags)
            if not floored:
                floor = None
                if i < len(mods) - 1:
                    h = ops.bn_relu_ragged(h, None, batch) if self.bn else torch.relu(h)
            elif i == len(mods) - 1:                 # no ReLU, no BatchNorm: every padded row holds l2norm(bias)
                floor = self._row_const(ops.gcn_row_const, m, flags, h)
            elif self.bn:
                pad = None if m.bias is None else ops.gcn_pad_const(m.bias, flags)
                h, floor = ops.bn_relu_ragged_padval(h, pad, batch)
            else:                                    # every padded row holds relu(l2norm(bias))
                h = torch.relu(h)
                floor = self._row_const(ops.gcn_pad_const, m, flags, h)
            out, arg = ops.segment_max_floor(h, floor, batch)                                    # :1093, :1100, :1107
            outs.append(out)
            argmax.append(arg)
        self._saved_argmax = argmax
        return ops.mlp_head(torch.cat(outs, dim=1), self._pred_linears())

    @staticmethod
    def _row_const(fn, layer, flags, like):
        if layer.bias is None:
            return torch.zeros(layer.weight.shape[1], device=like.device, dtype=torch.float32)
        return fn(layer.bias, flags)

    def loss(self, pred, label, type='softmax'):
        """Cross entropy of the prediction (encoders.py:1124-1127) on dp_cross_entropy_*; label [B] for a batch."""
        return _cross_entropy_loss(self, pred, label) if type == 'softmax' else super().loss(pred, label, type=type)

    def saved_activation(self, level, what):
        """'readout_argmax' of GraphConv layer `level` of the LAST batch forward: int32 [B, F_layer] rows of the dense
        batch — a value < n_b is a real row (graph-local), a value in [n_b, pad_to) a padded row (the lowest node index
        that holds the maximum; max_n stands for every index from max_n up).  Detached: clone to keep it."""
        if what != "readout_argmax":
            raise ValueError(f"saved_activation(): unknown activation {what!r} on the CSR path")
        saved = getattr(self, "_saved_argmax", None)
        if saved is None:
            raise RuntimeError("saved_activation(): no batch forward pass has run yet")
        if not 0 <= level < len(saved):
            raise IndexError(f"saved_activation(): layer {level} out of range ({len(saved)} layers)")
        return saved[level].detach()


# ----------------------------------------------------------------------------- GCN + Set2Set on CSR graphs
class SparseGcnSet2SetEncoder(GcnSet2SetEncoder):
    """`GcnSet2SetEncoder` (encoders.py:1137-1157) on one `CsrGraph` — forward(x [n, F], graph) -> ypred [1, label_dim]
    — or on a ragged `CsrBatch` — forward(x [n_total, F], batch) -> ypred [B, label_dim], computing what the dense
    class computes on the same graphs padded to `batch.pad_to` rows.  Same constructor and `state_dict` keys as the
    dense class (it IS the dense class's module tree), so `load_state_dict(dense.state_dict())` works.

    The embedding is the concatenation of every GraphConv layer's output (gcn_forward, encoders.py:1078) times the
    embedding mask (:1079-1080), so the padded rows of the dense batch are exactly zero: a ragged batch stores none of
    them.  They still take part in the readout: Set2Set runs `pad_to` steps and its softmax runs over all `pad_to`
    rows, where a zero row has logit 0 (`ops.set2set_ragged`: one term P_b exp(-m) in the denominator).  In front of
    the mask `CsrBatch.bn_relu` puts the padded rows' constants into the BatchNorm statistics and carries their
    gradient into the bias; no readout gradient reaches a padded row.  No row limit of 1024: a graph may have up to
    16 384 nodes (dp_set2set_ragged_*); the per-step attention kept for the backward costs 2 * pad_to * n_total floats.

    Not on this path: dropout; concat=False (gcn_forward concatenates every layer whatever the flag, while `s2s` is
    built for `pred_input_dim`, and on a batch add_self breaks the padded rows' constant)."""

    def __init__(self, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=[], concat=True,
                 bn=True, dropout=0.0, args=None):
        if dropout > 0.001:
            raise NotImplementedError("dropout on the CSR path")
        if not concat:
            raise NotImplementedError("concat=False on the CSR Set2Set path: gcn_forward concatenates every layer "
                                      "whatever the flag while s2s is built for pred_input_dim, and on a CsrBatch an "
                                      "add_self layer's padded row is not a constant of the layer")
        super().__init__(input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=pred_hidden_dims,
                         concat=concat, bn=bn, dropout=dropout, args=args)

    def forward(self, x, graph):
        """x [n, F] and a CsrGraph -> ypred [1, label_dim]; x [n_total, F] and a CsrBatch -> ypred [B, label_dim]."""
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError("SparseGcnSet2SetEncoder.forward(x [n, F], graph: CsrGraph or CsrBatch): the dense "
                            "(x [B, N, F], adj, batch_num_nodes) form is GcnSet2SetEncoder's")
        _check_node_rows(graph, x, self.input_dim)
        mods = self._stack_modules(self.conv_first, self.conv_block, self.conv_last)
        z = torch.cat(list(_gcn_stack(mods, x.contiguous().float(), graph, self.bn)), dim=1)      # :1078
        return ops.mlp_head(self.s2s(z, graph), self._pred_linears())                             # :1152-1156

    @torch.no_grad()
    def predict(self, x, graph):
        """Arg-max class per graph: int64 [B] on the device ([1] for a CsrGraph)."""
        return self.forward(x, graph).argmax(dim=1)

    def loss(self, pred, label, type='softmax'):
        """Cross entropy of the prediction (encoders.py:1124-1127) on dp_cross_entropy_*; label [B] for a batch."""
        return _cross_entropy_loss(self, pred, label) if type == 'softmax' else super().loss(pred, label, type=type)


# ----------------------------------------------------------------------------- DiffPool on a CSR graph
class SparseSoftPoolingGcnEncoder(SoftPoolingGcnEncoder):
    """`SoftPoolingGcnEncoder` (DiffPool, encoders.py:1160-1334 with the SURVEY.md Appendix B fixes D3 / D4) on a graph
    given as CSR: forward(x [n, F], graph) -> ypred [1, label_dim], for any n — also graphs above `max_num_nodes`,
    which the padded dense path (and the reference, load_data.py:79) cannot hold — or on a `CsrBatch` (B graphs, rows
    concatenated): forward(x [n_total, F], batch) -> ypred [B, label_dim].

    Same constructor and `state_dict` keys / shapes as the dense class (it IS the dense class's module tree), so a
    model trained on the dense path scores large graphs after `load_state_dict`.  `max_num_nodes` only fixes the
    cluster counts K_j = int(max_num_nodes * assign_ratio^(j+1)), as in the dense class.

    One body serves both containers.  Level 0 runs on the node rows: GraphConv as dp_sparse_gcn_layer_* (for a batch on
    the block-diagonal CSR), the assignment softmax as dp_assign_softmax_mask_* (no mask: every row is a node), and
    apply_bn (ReLU fused), the max readout and the pooling S^T Z, S^T A S as the container does them.  A CsrGraph:
    dp_bn_node_* with B = 1, dp_masked_max_*, dp_csr_pool_*.  A CsrBatch computes what the dense class computes on the
    same graphs padded to max_b n_b: the BatchNorm statistics per node index include the padded rows' constants
    (dp_bn_ragged_*), the readout has the zero floor of a graph with padded rows (dp_segment_max_*), the pooling is
    taken per graph (dp_csr_pool_batch_*).  The pooled levels are dense [B, K_j, K_j] graphs (B = 1 behind a CsrGraph)
    on the dense per-op entries (dp_gcn_layer_*, dp_bn_node_*, dp_assign_softmax_mask_*, dp_pool_*, dp_masked_max_*);
    pred_model on `hip_linear`, the loss on dp_cross_entropy_*.

    Both containers may carry one fp32 value per stored entry (`values`, and `values_t` for the CSR of A^T): the
    weighted adjacency of the dense path, e.g. the reference sampler's default D^-1/2 A D^-1/2 (graph_sampler.py:27-29),
    which `normalized()` builds.  Every op then takes its `_w` entry (`graph.weighted`), with the launches of the 0/1
    call.  Values that do not require grad are data; `graph.with_values(v)` with `v.requires_grad` makes every stored
    entry a variable: GraphConv, the level-0 pooling and both link objectives then return `v.grad` (one SDDMM launch
    each, dp_csr_sddmm's kernel).  `normalized()` is host float64 and not differentiated.

    A linkpred=True model (the constructor default, train.py --linkpred) trains here too: `loss(pred, label, graph)`
    adds the link-prediction term on dp_csr_linkpred_loss_* (per graph of a batch: dp_csr_linkpred_batch_*) — the n^2
    part of the sum does not depend on the adjacency and is a tile walk over S, the rest a gather over the edges;
    O(n K_0) memory, no dense adjacency.  `assign_ent_weight=w` adds w times the assignment-entropy term of the level-0
    assignment (ops.assign_entropy: normalised by the number of nodes), with or without the graph argument.

    Differences of a CsrBatch forward from the dense class's saved tensors: level-0 'assign' / 'embedding' and
    `assign_tensor` stay RAGGED, [n_total, .] (dense: [B, N, .]); level-0 'readout_argmax' rows are graph-local.

    Not on this path: dropout, adj_hop > 1, K_0 > 256 or a concatenated embedding wider than 512
    (dp_csr_pool's limits); on a CsrBatch also concat=False."""

    def __init__(self, max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers,
                 assign_hidden_dim, assign_ratio=0.25, assign_num_layers=-1, num_pooling=1,
                 pred_hidden_dims=[50], concat=True, bn=True, dropout=0.0, linkpred=True,
                 assign_input_dim=-1, args=None, assign_ent_weight=0.0):
        if dropout > 0.001:
            raise NotImplementedError("dropout on the CSR path")
        super().__init__(max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers,
                         assign_hidden_dim, assign_ratio=assign_ratio, assign_num_layers=assign_num_layers,
                         num_pooling=num_pooling, pred_hidden_dims=pred_hidden_dims, concat=concat, bn=bn,
                         dropout=dropout, linkpred=linkpred, assign_input_dim=assign_input_dim, args=args,
                         assign_ent_weight=assign_ent_weight)
        if self.assign_dims[0] > 256:
            raise ValueError(f"K_0 = {self.assign_dims[0]} clusters: the CSR pooling kernel (dp_csr_pool) supports "
                             "K_0 <= 256")
        if self.pred_input_dim > 512:
            raise ValueError(f"concatenated embedding width {self.pred_input_dim}: the CSR pooling kernel "
                             "(dp_csr_pool) supports D <= 512")
        self._saved = None

    def forward(self, x, graph, assign_x=None):
        """x [n, F] and a CsrGraph -> ypred [1, label_dim]; x [n_total, F] and a CsrBatch -> ypred [B, label_dim]."""
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError("SparseSoftPoolingGcnEncoder.forward(x [n, F], graph: CsrGraph[, assign_x]): the dense "
                            "(x [B, N, F], adj, batch_num_nodes) form is SoftPoolingGcnEncoder's")
        x_a = x if assign_x is None else assign_x
        _check_node_rows(graph, x, self.input_dim, x_a, self.assign_input_dim)
        x, x_a = x.contiguous().float(), x_a.contiguous().float()

        def embed(stack, first, block, last, h, adj):
            """One GraphConv stack's embedding: the concatenation of all its layers' outputs (encoders.py:1078)."""
            return torch.cat(list(stack(self._stack_modules(first, block, last), h, adj)), dim=-1)

        saved = {"assign": [], "xpool": [], "adjpool": [], "embedding": [], "graph": graph}
        z = embed(_gcn_stack, self.conv_first, self.conv_block, self.conv_last, x, graph)                 # :1254
        saved["embedding"].append(z)
        out, arg = graph.readout(z)                                                                       # :1257
        outs, argmax = [out], [arg]
        adj = graph                      # the adjacency of the current level: the container, then dense [B, K, K] blocks
        for i in range(self.num_pooling):                                                                 # :1263
            pred = self.assign_pred_modules[i]
            za = embed(_gcn_stack if i == 0 else _gcn_stack_dense, self.assign_conv_first_modules[i],
                       self.assign_conv_block_modules[i], self.assign_conv_last_modules[i], x_a, adj)
            s = ops.assign_softmax(za, pred.weight, pred.bias)      # :1273; level 0: every row is a node, no mask
            xp, adj = graph.pool(s, z) if i == 0 else ops.dense_pool(s, z, adj)                           # :1278-1279
            x_a = xp                                                # :1280; D4: level >= 1 assigns from X'
            z = embed(_gcn_stack_dense, self.conv_first_after_pool[i], self.conv_block_after_pool[i],
                      self.conv_last_after_pool[i], xp, adj)                                              # :1282-1284
            out, arg = ops.row_max(z)                                                                     # :1287
            outs.append(out)
            argmax.append(arg)
            saved["assign"].append(s)
            saved["xpool"].append(xp)
            saved["adjpool"].append(adj)
            saved["embedding"].append(z)
        ypred = ops.mlp_head(torch.cat(outs, dim=1), self._pred_linears())                                # :1295-1299
        saved["readout_argmax"] = argmax
        self._saved = saved
        s0 = saved["assign"][0]          # [1, n, K_0] as the dense class keeps it; RAGGED [n_total, K_0] for a batch
        self.assign_tensor = s0.unsqueeze(0) if isinstance(graph, CsrGraph) else s0
        return ypred

    @torch.no_grad()
    def predict(self, x, graph: CsrGraph, assign_x=None):
        """Arg-max class of the graph: int64 [1] on the device ([B] for a CsrBatch)."""
        return self.forward(x, graph, assign_x=assign_x).argmax(dim=1)

    def loss(self, pred, label, adj=None, batch_num_nodes=None, adj_hop=1):
        """Cross entropy of the prediction (encoders.py:1124-1127), plus — for a linkpred=True model — the
        link-prediction term of the level-0 assignment (encoders.py:1309-1331) on dp_csr_linkpred_loss_* (for a batch
        dp_csr_linkpred_batch_*: sum_b sum_{i,j<n_b} l_ij / sum_b n_b^2).  `adj` is then the CsrGraph or CsrBatch the
        forward ran on, in the position where train.py:207 passes the dense batch: loss(pred, label, graph), with
        label [B] for a batch.  The link term is kept in `self.link_loss`, as the dense class does."""
        last = None if self._saved is None else self._saved.get("graph")
        kind = CsrBatch if isinstance(adj, CsrBatch) or isinstance(last, CsrBatch) else CsrGraph
        call = f"SparseSoftPoolingGcnEncoder.loss(pred, label, {kind.ARG})"
        if kind is CsrBatch:
            nb = (adj if isinstance(adj, CsrBatch) else last).num_graphs
            if pred.dim() != 2 or pred.shape[0] != nb:
                raise ValueError(f"{call}: pred {tuple(pred.shape)} does not hold one row per graph of the batch ({nb})")
            if not isinstance(label, torch.Tensor) or label.numel() != nb:
                got = label.numel() if isinstance(label, torch.Tensor) else type(label).__name__
                raise ValueError(f"{call}: label must hold one class per graph of the batch ({nb}), got {got}")
            label = label.reshape(-1)
        if adj_hop != 1:
            raise NotImplementedError("adj_hop > 1 is never used by the reference's callers (train.py:207)")
        if self.linkpred:                            # every refusal of the link term comes before the first launch
            if adj is None:
                raise NotImplementedError(f"{call}: the link-prediction loss (linkpred=True) needs the {kind.__name__} "
                                          "the forward ran on; it cannot be formed from the prediction alone")
            if not isinstance(adj, kind):
                raise TypeError(f"{call}: {kind.ARG} must be the {kind.__name__} of the last forward, got "
                                f"{type(adj).__name__} (the dense (pred, label, adj, batch_num_nodes) form is "
                                "SoftPoolingGcnEncoder's)")
            if self._saved is None:
                raise ValueError(f"{call}: no forward pass has run yet, so there is no assignment to score")
            s0 = self._saved["assign"][0]            # attached: dS of the link term and of the pooling add up
            if kind is CsrBatch and last is not adj:
                raise ValueError(f"{call}: this is not the batch the last forward ran on; pass the batch of that forward")
            if adj.n != s0.shape[0]:
                raise ValueError(f"{call}: {kind.ARG} has n = {adj.n} nodes but the last forward ran on n = "
                                 f"{s0.shape[0]}; pass the {kind.ARG} of that forward")
            if self.link_objective == "frobenius":
                _refuse_frob_under_sync_bn(self)
        # enqueued in this order: entropy (its own refusals first), link, cross entropy; summed as ce + link + ent
        terms = [self._assign_ent_term(call)] if self.assign_ent_weight > 0 else []
        if self.linkpred:
            self.link_loss = adj.link_loss(s0, self.link_objective)
            terms.insert(0, self.link_loss)
        return sum(terms, ops.cross_entropy(pred, label))

    def _assign_ent_term(self, call):
        """assign_ent_weight * E of the last forward's level-0 assignment (ops.assign_entropy: every row of the ragged
        [n_total, K_0] assignment is a node, so the normaliser is n_total — the dense class's sum_b n_b on the same
        graphs).  The assignment is the attached one: its dS adds to the pooling's and the link term's.  The unweighted
        E is kept in `self.assign_ent_loss`."""
        _refuse_ent_under_sync_bn(self)
        if self._saved is None:
            raise ValueError(f"{call}: no forward pass has run yet, so there is no assignment to score")
        ent = ops.assign_entropy(self._saved["assign"][0])
        self.assign_ent_loss = ent.detach()
        return self.assign_ent_weight * ent

    def saved_activation(self, level, what):
        """One activation of the LAST forward call, shaped as the dense class returns it with B = 1: 'assign' [1, n_j,
        K_j], 'xpool' [1, K_j, D], 'adjpool' [1, K_j, K_j], 'embedding' [1, n_j, D] (levels 0 .. num_pooling) and
        'readout_argmax' int32 [1, D] (levels 0 .. num_pooling).  Detached views: clone to keep them.

        After a CsrBatch forward: 'xpool' [B, K_j, D], 'adjpool' [B, K_j, K_j], pooled-level 'assign' / 'embedding'
        [B, K_j, .] and 'readout_argmax' [B, D] as the dense class returns them; the level-0 'assign' / 'embedding' stay
        ragged, [n_total, .], and the level-0 arg-max rows are graph-local (-1: the zero floor of a graph with padded
        rows holds the maximum)."""
        if self._saved is None:
            raise RuntimeError("saved_activation(): no forward pass has run yet")
        if what not in ("assign", "xpool", "adjpool", "embedding", "readout_argmax"):
            raise ValueError(f"saved_activation(): unknown activation {what!r} on the CSR path")
        seq = self._saved[what]
        if not 0 <= level < len(seq):
            raise IndexError(f"saved_activation(): level {level} out of range for {what!r} ({len(seq)} levels)")
        t = seq[level].detach()
        if not isinstance(self._saved.get("graph"), CsrBatch) and what != "readout_argmax" and t.dim() == 2:
            return t.unsqueeze(0)                    # a single graph's level-0 'assign' / 'embedding' [n, .]
        return t


# ----------------------------------------------------------------------------- learned edge weights
class EdgeAttention(torch.nn.Module):
    """Edge weights computed from the node features, on the stored entries of a CsrGraph / CsrBatch: forward(x, graph)
    returns a weighted container that the three sparse encoders take unchanged — `ypred = model(x, att(x, g))` — and
    through which the projections train (`ops.csr_sddmm`, `ops.csr_edge_softmax`, `ops.csr_sym_normalize`).

    norm="softmax": two bias-free Linear layers q, k [att_dim, input_dim] on `hip_linear`; the scores
    q(x)_i . k(x)_j / sqrt(att_dim) of every stored (i, j) go through a softmax over each node's neighbour list.  The
    rows then sum to 1 and a_ij != a_ji, so the result rides `graph.directed()`.
    norm="sym": one projection q; the gate sigmoid(q(x)_i . q(x)_j / sqrt(att_dim)) is symmetric bit for bit (the
    products commute and the summation order is fixed), is multiplied by the stored values of a weighted container, and
    is normalised as D^-1/2 A D^-1/2 with the gated degrees; the result keeps the container's form.

    score="additive" (with norm="softmax"): GAT's scores on `heads` heads, the mean over the heads of
    softmax_j(leaky_relu(a_src_h . q_h(x_i) + a_dst_h . q_h(x_j), negative_slope)), in one fused pass
    (`ops.csr_gat_attention`).  One bias-free q: Linear(input_dim, heads * att_dim) and a_src, a_dst [heads, att_dim];
    the per-head vectors q.weight.view(H, d, F)^T a are [H, F] matrices, so u and v are two `hip_linear` calls and
    [n, heads * att_dim] is never formed.  The result rides `graph.directed()`."""

    def __init__(self, input_dim, att_dim, norm="softmax", score="dot", heads=1, negative_slope=0.2):
        super().__init__()
        if norm not in ("softmax", "sym"):
            raise ValueError(f"EdgeAttention: norm must be 'softmax' or 'sym', got {norm!r}")
        if score not in ("dot", "additive"):
            raise ValueError(f"EdgeAttention: score must be 'dot' or 'additive', got {score!r}")
        if score == "additive" and norm != "softmax":
            raise ValueError(f"EdgeAttention: score='additive' goes with norm='softmax', got norm={norm!r}")
        if not isinstance(heads, int) or not 1 <= heads <= 8:
            raise ValueError(f"EdgeAttention: heads must be 1 .. 8, got {heads!r}")
        if heads > 1 and score == "dot":
            raise ValueError(f"EdgeAttention: heads={heads} needs score='additive' (the dot-product score has one head)")
        self.input_dim, self.att_dim, self.norm = input_dim, att_dim, norm
        self.score, self.heads, self.negative_slope = score, heads, float(negative_slope)
        if score == "additive":
            self.q = torch.nn.Linear(input_dim, heads * att_dim, bias=False)
            self.a_src = torch.nn.Parameter(torch.empty(heads, att_dim))
            self.a_dst = torch.nn.Parameter(torch.empty(heads, att_dim))
            gain = torch.nn.init.calculate_gain("relu")              # GAT's initialisation: Xavier, ReLU gain
            torch.nn.init.xavier_uniform_(self.q.weight, gain=gain)
            torch.nn.init.xavier_uniform_(self.a_src, gain=gain)
            torch.nn.init.xavier_uniform_(self.a_dst, gain=gain)
            return
        self.q = torch.nn.Linear(input_dim, att_dim, bias=False)
        if norm == "softmax":
            self.k = torch.nn.Linear(input_dim, att_dim, bias=False)

    def forward(self, x, graph):
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"EdgeAttention.forward(x, graph: CsrGraph or CsrBatch), got {type(graph).__name__}")
        _check_node_rows(graph, x, self.input_dim)
        x = x.contiguous().float()
        if self.score == "additive":
            w = self.q.weight.view(self.heads, self.att_dim, self.input_dim)
            wu = torch.einsum("hdf,hd->hf", w, self.a_src)           # [H, F]: a_src_h . q_h(x) = (W_h^T a_src_h) . x
            wv = torch.einsum("hdf,hd->hf", w, self.a_dst)
            a = ops.csr_gat_attention(hip_linear(x, wu), hip_linear(x, wv), graph, self.negative_slope)
            return graph.directed().with_values(a)
        scale = float(self.att_dim) ** -0.5
        qx = hip_linear(x, self.q.weight)
        if self.norm == "softmax":
            a = ops.csr_edge_softmax(ops.csr_sddmm(qx, hip_linear(x, self.k.weight), graph, scale), graph)
            return graph.directed().with_values(a)
        gate = torch.sigmoid(ops.csr_sddmm(qx, qx, graph, scale))
        if graph.weighted:
            gate = gate * (graph.values if graph.values.numel() == graph.nnz else graph.values[:graph.nnz])
        return graph.with_values(ops.csr_sym_normalize(gate, graph))


# ----------------------------------------------------------------------------- graph-attention layer
class GatConv(torch.nn.Module):
    """One multi-head graph-attention (GAT) layer on a CsrGraph / CsrBatch: forward(x, graph) returns
    [n, heads * out_dim] (concat=True, the heads side by side) or [n, out_dim] (concat=False, their mean), plus `bias`.

    z = lin(x) with lin: Linear(input_dim, heads * out_dim, bias=False) on `hip_linear`; per head h the scores
    leaky_relu(a_src_h . z_i^h + a_dst_h . z_j^h, negative_slope) go through a softmax over node i's stored entries and the
    coefficients are multiplied into the neighbours' z_j^h in one fused pass (`ops.csr_gat_conv`): nothing of size nnz is
    written, the only temporaries are [n, heads * out_dim].  a_src, a_dst are [heads, out_dim] (Xavier-uniform with the
    ReLU gain, as `EdgeAttention`'s additive form), bias [heads * out_dim] or [out_dim], zero at the start.

    The layer adds NO self loops and does not read the container's stored values: a node attends exactly its stored
    entries, and a node without any gets `bias`.  GAT's usual self-attention comes from listing (i, i) in the edge list,
    which `CsrGraph.from_edges` / `CsrBatch.from_edge_lists` accept.  Layers stack, and their output feeds the three
    sparse encoders unchanged.  Limits: 1 <= heads <= 8, heads * out_dim <= 512."""

    def __init__(self, input_dim, out_dim, heads=1, concat=True, negative_slope=0.2, bias=True):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= 8:
            raise ValueError(f"GatConv: heads must be 1 .. 8, got {heads!r}")
        if not isinstance(out_dim, int) or out_dim < 1 or heads * out_dim > _lib.CSR_GAT_CONV_MAX_WIDTH:
            raise ValueError(f"GatConv: heads * out_dim must be 1 .. {_lib.CSR_GAT_CONV_MAX_WIDTH}, got heads={heads}, "
                             f"out_dim={out_dim!r}")
        slope = float(negative_slope)
        if slope != slope or slope in (float("inf"), float("-inf")):
            raise ValueError(f"GatConv: negative_slope must be finite, got {negative_slope!r}")
        self.input_dim, self.out_dim, self.heads = input_dim, out_dim, heads
        self.concat, self.negative_slope = bool(concat), slope
        self.lin = torch.nn.Linear(input_dim, heads * out_dim, bias=False)
        self.a_src = torch.nn.Parameter(torch.empty(heads, out_dim))
        self.a_dst = torch.nn.Parameter(torch.empty(heads, out_dim))
        gain = torch.nn.init.calculate_gain("relu")                  # GAT's initialisation: Xavier, ReLU gain
        torch.nn.init.xavier_uniform_(self.lin.weight, gain=gain)
        torch.nn.init.xavier_uniform_(self.a_src, gain=gain)
        torch.nn.init.xavier_uniform_(self.a_dst, gain=gain)
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(heads * out_dim if self.concat else out_dim))
        else:
            self.register_parameter("bias", None)

    def forward(self, x, graph):
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"GatConv.forward(x, graph: CsrGraph or CsrBatch), got {type(graph).__name__}")
        _check_node_rows(graph, x, self.input_dim)
        z = hip_linear(x.contiguous().float(), self.lin.weight)
        zh = z.view(graph.n, self.heads, self.out_dim)
        u, v = (zh * self.a_src).sum(-1), (zh * self.a_dst).sum(-1)
        y = ops.csr_gat_conv(z, u, v, graph, self.heads, self.negative_slope, self.concat)
        return y if self.bias is None else y + self.bias


# ----------------------------------------------------------------------------- GraphSAGE layer
class SageConv(torch.nn.Module):
    """One GraphSAGE layer with the mean aggregator on a CsrGraph / CsrBatch, the neighbour sample drawn on the device:
    forward(x, graph, nodes=None, seed=None) = relu(W [x_i | mean_{j in S(i)} x_j])  (gcn=False, the reference's Encoder
    over its MeanAggregator, aggregators.py:30-63)  or  relu(W mean_{S(i) u {i}} x_j)  (gcn=True), [m, out_dim].

    S(i) is `num_sample` of node i's stored neighbours without replacement (all of them when it has no more, or with
    num_sample=None), drawn and averaged in ONE fused launch (`ops.csr_sample_mean`): no Python loop over the nodes, no
    host-to-device copy, nothing of size nnz written.  `weight` is [out_dim, 2 input_dim] ([out_dim, input_dim] under
    gcn), Xavier-uniform, applied on `hip_linear`; `bias` [out_dim] is off by default, as in the reference.

    `seed`: a Python int in [0, 2^64) fixes the sample; None draws one from torch's CPU generator (no device sync,
    reproducible under `torch.manual_seed`).  The layer samples in training AND in evaluation, as the reference does.
    `nodes`: None for every node (layers stack on the whole graph), or an int32 device tensor of distinct node ids —
    the last layer of a stack may take the mini-batch.  Nested mini-batch sampling across layers (a sample of the
    sample's neighbourhood) is out of scope, as are weighted sampling, num_sample > 64 and hipGraph capture of the op
    (the seed is a kernel argument and would be frozen).  A node without neighbours gets a zero mean, not NaN."""

    def __init__(self, input_dim, out_dim, num_sample=10, gcn=False, bias=False):
        super().__init__()
        if num_sample is not None and (not isinstance(num_sample, int) or isinstance(num_sample, bool)
                                       or not 1 <= num_sample <= _lib.CSR_SAMPLE_MAX_K):
            raise ValueError(f"SageConv: num_sample must be 1 .. {_lib.CSR_SAMPLE_MAX_K} or None, got {num_sample!r}")
        if not isinstance(input_dim, int) or not isinstance(out_dim, int) or input_dim < 1 or out_dim < 1:
            raise ValueError(f"SageConv: input_dim and out_dim must be positive, got {input_dim!r} and {out_dim!r}")
        self.input_dim, self.out_dim, self.num_sample, self.gcn = input_dim, out_dim, num_sample, bool(gcn)
        self.weight = torch.nn.Parameter(torch.empty(out_dim, input_dim if self.gcn else 2 * input_dim))
        torch.nn.init.xavier_uniform_(self.weight)
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_dim))
        else:
            self.register_parameter("bias", None)

    def forward(self, x, graph, nodes=None, seed=None, nodes_checked=False):
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"SageConv.forward(x, graph: CsrGraph or CsrBatch), got {type(graph).__name__}")
        _check_node_rows(graph, x, self.input_dim)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())       # the CPU generator: no device sync
        h = ops.csr_sample_mean(x, graph, self.num_sample, seed, nodes, "gcn" if self.gcn else "concat",
                                nodes_checked)
        return torch.relu(hip_linear(h, self.weight, self.bias))


class SageEncoder(torch.nn.Module):
    """The reference's Encoder for `SupervisedGraphSage` on the device: forward(nodes) -> [len(nodes), embed_dim], the
    `SageConv` layer `conv` over `graph` on the features of ALL nodes, evaluated at `nodes`.

    `features`: an fp32 tensor [n, F] (kept as a buffer), an `nn.Embedding` (its weight trains), or a callable / module
    mapping a LongTensor of node ids to their features.  `nodes`: a list, a numpy array or a tensor of distinct node
    ids (checked on the host: ValueError).  `seed` as in `SageConv.forward`."""

    def __init__(self, features, graph, conv):
        super().__init__()
        if not isinstance(conv, SageConv):
            raise TypeError(f"SageEncoder: conv must be a SageConv, got {type(conv).__name__}")
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"SageEncoder: graph must be a CsrGraph or CsrBatch, got {type(graph).__name__}")
        if isinstance(features, torch.Tensor) and not isinstance(features, torch.nn.Parameter):
            self.register_buffer("features", features, persistent=False)
        elif isinstance(features, (torch.nn.Module, torch.nn.Parameter)) or callable(features):
            self.features = features
        else:
            raise TypeError(f"SageEncoder: features must be a tensor, an nn.Embedding or a callable, got "
                            f"{type(features).__name__}")
        self.graph, self.conv, self.embed_dim = graph, conv, conv.out_dim

    def _x(self):
        f = self.features
        if isinstance(f, torch.Tensor):
            return f
        if isinstance(f, torch.nn.Embedding):
            return f.weight
        return f(torch.arange(self.graph.n, device=self.graph.indptr.device))

    def forward(self, nodes, seed=None):
        ids = ops.check_target_nodes("SageEncoder", nodes, self.graph.n)
        dev = self.graph.indptr.device
        return self.conv(self._x(), self.graph, ids.to(device=dev, dtype=torch.int32), seed, nodes_checked=True)


# ----------------------------------------------------------------------------- top-k pooling
class TopKPooling(torch.nn.Module):
    """Hard top-k pooling on a CsrGraph / CsrBatch: forward(x, graph) -> (x', graph', perm) keeps the
    ceil(ratio * n_b) best-scored nodes of every graph (`ops.csr_topk_pool`), gates their features with tanh(score) and
    returns the induced subgraph as a container of the input's class, so layers stack to any depth at O(n + nnz).

    score="proj": gPool of Graph U-Nets, s = x . p / ||p|| with a learned p [input_dim] (on `hip_linear`).
    score="gcn": SAGPool, s = (A x + x) W + b with W [input_dim, 1] on `ops.csr_graph_conv` (the container's stored
    values weigh the sum; pass a `normalized()` container for the usual D^-1/2 A D^-1/2).
    The selection itself passes no gradient; the score trains through the gate.  perm int32 [n'] holds the old global id
    of every new row, in ascending order within a graph.  Not on this path: `min_score`, unpooling, hipGraph capture."""

    def __init__(self, input_dim, ratio=0.5, score="proj"):
        super().__init__()
        if not isinstance(input_dim, int) or isinstance(input_dim, bool) or input_dim < 1:
            raise ValueError(f"TopKPooling: input_dim must be a positive integer, got {input_dim!r}")
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"TopKPooling: ratio must lie in (0, 1], got {ratio!r}")
        if score not in ("proj", "gcn"):
            raise ValueError(f"TopKPooling: score must be 'proj' or 'gcn', got {score!r}")
        self.input_dim, self.ratio, self.score = input_dim, float(ratio), score
        if score == "proj":
            self.p = torch.nn.Parameter(torch.empty(input_dim))
            bound = float(input_dim) ** -0.5
            torch.nn.init.uniform_(self.p, -bound, bound)
        else:
            self.weight = torch.nn.Parameter(torch.empty(input_dim, 1))
            torch.nn.init.xavier_uniform_(self.weight)
            self.bias = torch.nn.Parameter(torch.zeros(1))

    def scores(self, x, graph):
        """The score of every node, fp32 [n], with autograd history."""
        if self.score == "proj":
            return hip_linear(x, (self.p / self.p.norm()).view(1, -1)).view(-1)
        return ops.csr_graph_conv(x, self.weight, self.bias, graph, _lib.F_ADD_SELF).view(-1)

    def forward(self, x, graph):
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"TopKPooling.forward(x, graph: CsrGraph or CsrBatch), got {type(graph).__name__}")
        _check_node_rows(graph, x, self.input_dim)
        x = x.contiguous().float()
        s = self.scores(x, graph)
        return ops.csr_topk_pool(x, s, graph, ratio=self.ratio, gate=torch.tanh(s))
