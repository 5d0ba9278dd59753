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
entries live in `ops.py`; this module holds the CSR container and the two model classes.

`SparseSoftPoolingGcnEncoder` does the same for DiffPool (`SoftPoolingGcnEncoder`): level 0 on the CSR ops above plus
dp_csr_pool_fwd / bwd for the pooling S^T Z, S^T A S (encoders.py:1278-1279), the small pooled levels on the dense
per-op entries with B = 1, and the link-prediction loss (encoders.py:1309-1331) on dp_csr_linkpred_loss_fwd / bwd,
which never forms an n x n adjacency.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
from .ops import hip_linear  # noqa: F401  (tests and tools import it from here)


# ----------------------------------------------------------------------------- CSR helpers
class CsrGraph:
    """CSR of one graph's adjacency on the device: int32 indptr [n + 1], indices [nnz] — row i lists the j with
    A[i, j] != 0 (0/1 adjacency, graph_sampler.py:26) — plus the CSR of A^T for the backward gather (the same arrays
    for an undirected graph)."""

    def __init__(self, indptr, indices, indptr_t=None, indices_t=None):
        self.indptr, self.indices = indptr, indices
        self.indptr_t = indptr if indptr_t is None else indptr_t
        self.indices_t = indices if indices_t is None else indices_t
        self.n = indptr.numel() - 1

    @staticmethod
    def from_edges(n, src, dst, device, symmetric=True):
        """Edge list -> CSR (both directions when symmetric, duplicates removed, no self loops added)."""
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        if symmetric:
            src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        key = np.unique(src * n + dst)
        rows, cols = key // n, key % n

        def csr(r, c):
            order = np.lexsort((c, r))
            r, c = r[order], c[order]
            indptr = np.zeros(n + 1, dtype=np.int32)
            np.add.at(indptr, r + 1, 1)
            return (torch.from_numpy(np.cumsum(indptr, dtype=np.int64).astype(np.int32)).to(device),
                    torch.from_numpy(c.astype(np.int32)).to(device))
        ip, ix = csr(rows, cols)
        if symmetric:
            return CsrGraph(ip, ix)
        ipt, ixt = csr(cols, rows)
        return CsrGraph(ip, ix, ipt, ixt)

    @staticmethod
    def from_dense(adj):
        """[n, n] tensor (any device) -> CSR on adj's device (testing aid)."""
        a = adj.detach().cpu().numpy() != 0
        r, c = np.nonzero(a)
        return CsrGraph.from_edges(a.shape[0], r, c, adj.device, symmetric=False)


def _gcn_stack(mods, h, graph, bn=True):
    """gcn_forward (encoders.py:1054-1081) on one graph: GraphConv -> ReLU -> apply_bn for every layer but the last;
    yields each layer's output as soon as it is enqueued.  `graph` is a CsrGraph, or a pooled level's dense K x K
    adjacency (dp_gcn_layer_* with B = 1)."""
    for i, m in enumerate(mods):
        if isinstance(graph, CsrGraph):
            h = ops.csr_graph_conv(h, m.weight, m.bias, graph, m._flags())
        else:
            h = ops.graph_conv(h.unsqueeze(0), graph.unsqueeze(0), m.weight, m.bias, m._flags())[0]
        if i < len(mods) - 1:
            h = ops.bn_relu_nodes(h) if bn else torch.relu(h)      # ReLU is fused into the BN kernel
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


# ----------------------------------------------------------------------------- DiffPool on a CSR graph
class SparseSoftPoolingGcnEncoder(SoftPoolingGcnEncoder):
    """`SoftPoolingGcnEncoder` (DiffPool, encoders.py:1160-1334 with the SURVEY.md Appendix B fixes D3 / D4) on ONE graph
    given as CSR: forward(x [n, F], graph) -> ypred [1, label_dim], for any n — also graphs above `max_num_nodes`,
    which the padded dense path (and the reference, load_data.py:79) cannot hold.

    Same constructor and `state_dict` keys / shapes as the dense class (it IS the dense class's module tree), so a
    model trained on the dense path scores large graphs after `load_state_dict`.  `max_num_nodes` only fixes the
    cluster counts K_j = int(max_num_nodes * assign_ratio^(j+1)), as in the dense class.

    Level 0 runs on the CSR kernels: GraphConv as dp_sparse_gcn_layer_*, apply_bn as dp_bn_node_* with B = 1 (ReLU
    fused), the assignment softmax as dp_assign_softmax_mask_* (no mask: every row is a node), and the pooling
    S^T Z, S^T A S as dp_csr_pool_*.  The pooled levels are K_j x K_j dense graphs and run on the dense per-op entries
    with B = 1 (dp_gcn_layer_*, dp_bn_node_*, dp_assign_softmax_mask_*, dp_pool_*); readouts on dp_masked_max_*,
    pred_model on `hip_linear`, the loss on dp_cross_entropy_*.

    A linkpred=True model (the constructor default, train.py --linkpred) trains here too: `loss(pred, label, graph)`
    adds the link-prediction term on dp_csr_linkpred_loss_* — the n^2 part of the sum does not depend on the adjacency
    and is a tile walk over S, the rest a gather over the edges; O(n K_0) memory, no dense adjacency.

    Not on this path: dropout, adj_hop > 1, batches of graphs, K_0 > 256 or a concatenated embedding wider than 512
    (dp_csr_pool's limits)."""

    def __init__(self, max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers,
                 assign_hidden_dim, assign_ratio=0.25, assign_num_layers=-1, num_pooling=1,
                 pred_hidden_dims=[50], concat=True, bn=True, dropout=0.0, linkpred=True,
                 assign_input_dim=-1, args=None):
        if dropout > 0.001:
            raise NotImplementedError("dropout on the CSR path")
        super().__init__(max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers,
                         assign_hidden_dim, assign_ratio=assign_ratio, assign_num_layers=assign_num_layers,
                         num_pooling=num_pooling, pred_hidden_dims=pred_hidden_dims, concat=concat, bn=bn,
                         dropout=dropout, linkpred=linkpred, assign_input_dim=assign_input_dim, args=args)
        if self.assign_dims[0] > 256:
            raise ValueError(f"K_0 = {self.assign_dims[0]} clusters: the CSR pooling kernel (dp_csr_pool) supports "
                             "K_0 <= 256")
        if self.pred_input_dim > 512:
            raise ValueError(f"concatenated embedding width {self.pred_input_dim}: the CSR pooling kernel "
                             "(dp_csr_pool) supports D <= 512")
        self._saved = None

    def _embed(self, first, block, last, h, graph):
        """One GraphConv stack's embedding: the concatenation of all its layers' outputs (encoders.py:1078)."""
        return torch.cat(list(_gcn_stack(self._stack_modules(first, block, last), h, graph)), dim=1)

    # -- public surface
    def forward(self, x, graph: CsrGraph, assign_x=None):
        if not isinstance(graph, CsrGraph):
            raise TypeError("SparseSoftPoolingGcnEncoder.forward(x [n, F], graph: CsrGraph[, assign_x]): the dense "
                            "(x [B, N, F], adj, batch_num_nodes) form is SoftPoolingGcnEncoder's")
        _lib.require_gpu_tensor(x, "x")
        x_a = x if assign_x is None else assign_x
        _lib.require_gpu_tensor(x_a, "assign_x")
        if x.dim() != 2 or x.shape[0] != graph.n or x_a.dim() != 2 or x_a.shape[0] != graph.n:
            raise ValueError(f"expected x / assign_x [n, F] with n = {graph.n}, got {tuple(x.shape)} / "
                             f"{tuple(x_a.shape)}")
        if x.shape[1] != self.input_dim or x_a.shape[1] != self.assign_input_dim:
            raise ValueError(f"feature widths {x.shape[1]}/{x_a.shape[1]} do not match the model "
                             f"({self.input_dim}/{self.assign_input_dim})")
        x, x_a = x.contiguous().float(), x_a.contiguous().float()
        saved = {"assign": [], "xpool": [], "adjpool": [], "embedding": []}
        z = self._embed(self.conv_first, self.conv_block, self.conv_last, x, graph)                       # :1254
        saved["embedding"].append(z)
        out, arg = ops.row_max(z)                                                                         # :1257
        outs, argmax = [out], [arg]
        adj, s0 = graph, None            # the adjacency of the current level: the CSR graph, then dense K x K blocks
        for i in range(self.num_pooling):                                                                 # :1263
            pred = self.assign_pred_modules[i]
            za = self._embed(self.assign_conv_first_modules[i], self.assign_conv_block_modules[i],
                             self.assign_conv_last_modules[i], x_a, adj)    # :1269-1271; D4: level >= 1 assigns from X'
            s = ops.assign_softmax(za, pred.weight, pred.bias)                                            # :1273
            if i == 0:
                xp, adj = ops.csr_pool(s, z, graph)                                                       # :1278-1279
                s0 = s
            else:
                xp, adj = ops.dense_pool(s, z, adj)
            x_a = xp                                                                                      # :1280
            z = self._embed(self.conv_first_after_pool[i], self.conv_block_after_pool[i],
                            self.conv_last_after_pool[i], xp, adj)                                        # :1282-1284
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
        self.assign_tensor = s0.unsqueeze(0)        # level-0 assignment [1, n, K_0], as the dense class keeps it
        return ypred

    @torch.no_grad()
    def predict(self, x, graph: CsrGraph, assign_x=None):
        """Arg-max class of the graph: int64 [1] on the device."""
        return self.forward(x, graph, assign_x=assign_x).argmax(dim=1)

    def loss(self, pred, label, adj=None, batch_num_nodes=None, adj_hop=1):
        """Cross entropy of the prediction (encoders.py:1124-1127), plus — for a linkpred=True model — the
        link-prediction term of the level-0 assignment (encoders.py:1309-1331) on dp_csr_linkpred_loss_*.  `adj` is
        then the CsrGraph the forward ran on, in the position where train.py:207 passes the dense batch:
        loss(pred, label, graph).  The link term is kept in `self.link_loss`, as the dense class does."""
        if self.linkpred:
            call = "SparseSoftPoolingGcnEncoder.loss(pred, label, graph)"
            if adj is None:
                raise NotImplementedError(f"{call}: the link-prediction loss (linkpred=True) needs the CsrGraph the "
                                          "forward ran on; it cannot be formed from the prediction alone")
            if not isinstance(adj, CsrGraph):
                raise TypeError(f"{call}: graph must be the CsrGraph of the last forward, got {type(adj).__name__} "
                                "(the dense (pred, label, adj, batch_num_nodes) form is SoftPoolingGcnEncoder's)")
        if adj_hop != 1:
            raise NotImplementedError("adj_hop > 1 is never used by the reference's callers (train.py:207)")
        if not self.linkpred:
            return ops.cross_entropy(pred, label)
        if self._saved is None:
            raise ValueError(f"{call}: no forward pass has run yet, so there is no assignment to score")
        s0 = self._saved["assign"][0]                # attached: dS of the link term and of the pooling add up
        if adj.n != s0.shape[0]:
            raise ValueError(f"{call}: graph has n = {adj.n} nodes but the last forward ran on n = {s0.shape[0]}; "
                             "pass the graph of that forward")
        self.link_loss = ops.csr_link_loss(s0, adj)
        return ops.cross_entropy(pred, label) + self.link_loss

    def saved_activation(self, level, what):
        """One activation of the LAST forward call, shaped as the dense class returns it with B = 1: 'assign' [1, n_j,
        K_j], 'xpool' [1, K_j, D], 'adjpool' [1, K_j, K_j], 'embedding' [1, n_j, D] (levels 0 .. num_pooling) and
        'readout_argmax' int32 [1, D] (levels 0 .. num_pooling).  Detached views: clone to keep them."""
        if self._saved is None:
            raise RuntimeError("saved_activation(): no forward pass has run yet")
        if what not in ("assign", "xpool", "adjpool", "embedding", "readout_argmax"):
            raise ValueError(f"saved_activation(): unknown activation {what!r} on the CSR path")
        seq = self._saved[what]
        if not 0 <= level < len(seq):
            raise IndexError(f"saved_activation(): level {level} out of range for {what!r} ({len(seq)} levels)")
        return seq[level].detach() if what == "readout_argmax" else seq[level].detach().unsqueeze(0)
