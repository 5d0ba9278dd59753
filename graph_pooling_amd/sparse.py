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
entries live in `ops.py`, the CSR containers (`CsrGraph`, `CsrBatch`, `HostCsr`; exported from here too) in `csr.py`; this
module holds the model classes.

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
container, with the neighbour sample drawn on the device in the launch that takes its mean (dp_csr_sample_mean_*);
`NestedSageEncoder` stacks the layers on nested mini-batches, each on the sampled frontier of the one above
(dp_csr_block_*).

`TopKPooling` is the hard pooling next to DiffPool's soft one (gPool / SAGPool): it keeps the best-scored nodes of every
graph and returns the induced subgraph as a container of the input's class, built on the device (dp_csr_topk_*) and
wrapped by `CsrGraph.from_device_csr` / `CsrBatch.from_device_csr`, so it feeds everything above.
"""
from __future__ import annotations

import torch

from . import _lib, ops
from .csr import CsrBatch, CsrGraph, HostCsr  # noqa: F401  (the containers' public home stays this module too)
from .encoders import (GcnEncoderGraph, GcnSet2SetEncoder, SoftPoolingGcnEncoder, _refuse_ent_under_sync_bn,
                       _refuse_frob_under_sync_bn)
from .ops import hip_linear  # noqa: F401  (tests and tools import it from here)


def _check_node_rows(graph, x, input_dim, assign_x=None, assign_input_dim=None):
    """The forwards' input check: x is a GPU tensor `graph.rows()` of width `input_dim` — and, in the DiffPool forward,
    assign_x one of width `assign_input_dim`."""
    named = (("x", x),) if assign_input_dim is None else (("x", x), ("assign_x", assign_x))
    for name, t in named:
        ops.check_rows("", graph, name, t)
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
        self.input_dim, self.out_dim, self.heads = input_dim, out_dim, heads
        self.concat, self.negative_slope = bool(concat), ops.finite_slope("GatConv", negative_slope)
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
    the last layer of a stack may take the mini-batch.

    Nested mini-batches: `block(graph, nodes, seed)` builds the layer's `ops.SampledBlock` on the device —
    `src`, the targets and everything their samples reach — and `forward_block(x_src, block)` is the same layer on the
    COMPACT rows x_src [n_src, input_dim], with the bits of forward(x, graph, nodes, seed) at x_src = x[block.src];
    `nodes` may be the block of the layer above (`NestedSageEncoder` stacks them).  Out of scope: weighted sampling,
    num_sample > 64, a `src` order with the targets first, and hipGraph capture of either form (the seed is a kernel
    argument and would be frozen; a block costs one read-back).  A node without neighbours gets a zero mean, not NaN."""

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

    def _k(self):
        return _lib.CSR_SAMPLE_ALL if self.num_sample is None else self.num_sample

    def block(self, graph, nodes, seed=None, nodes_checked=False):
        """The layer's sampled block for the targets `nodes` (an int32 device tensor of distinct ids, None, or the
        `SampledBlock` of the layer above): `ops.csr_sample_block` at this layer's num_sample."""
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"SageConv.block(graph: CsrGraph or CsrBatch, nodes), got {type(graph).__name__}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())       # the CPU generator: no device sync
        return ops.csr_sample_block(graph, nodes, self.num_sample, seed, nodes_checked)

    def forward_block(self, x_src, block):
        """relu(W [x_i | mean] ) (or the gcn form) for the block's targets from the compact rows x_src
        [block.n_src, input_dim] -> [m, out_dim]."""
        if not isinstance(block, ops.SampledBlock):
            raise TypeError(f"SageConv.forward_block(x_src, block: SampledBlock), got {type(block).__name__}")
        if block.k != self._k():
            raise ValueError(f"SageConv.forward_block: the block was sampled with k = {block.k}, the layer has num_sample = "
                             f"{self.num_sample} (k = {self._k()})")
        if not isinstance(x_src, torch.Tensor) or x_src.dim() != 2 or tuple(x_src.shape) != (block.n_src, self.input_dim):
            got = tuple(x_src.shape) if isinstance(x_src, torch.Tensor) else type(x_src).__name__
            raise ValueError(f"SageConv.forward_block: expected x_src [{block.n_src}, {self.input_dim}], got {got}")
        if block.m == 0:
            return x_src.new_zeros((0, self.out_dim), dtype=torch.float32)
        h = ops.csr_block_mean(x_src, block, "gcn" if self.gcn else "concat")
        return torch.relu(hip_linear(h, self.weight, self.bias))


LAYER_SEED_STEP = 0x9E3779B97F4A7C15                      # layer l samples with (seed + l * this) mod 2^64


class NestedSageEncoder(torch.nn.Module):
    """A stack of `SageConv` layers on nested mini-batches, the reference's Encoder over Encoder for
    `SupervisedGraphSage`: forward(nodes) -> [len(nodes), embed_dim], every layer evaluated on the sampled frontier of
    the layer above only, as MeanAggregator.forward calls `features` on its unique_nodes_list (aggregators.py:30-63).

    convs[0] is the innermost layer (it reads `features`), convs[-1] the one whose targets are `nodes`.  forward builds
    the blocks from the last layer inwards — the block of layer l - 1 has the `src` of layer l's block as its targets —
    evaluates `features` at the innermost `src` ONLY (a tensor by index_select; an `nn.Embedding` or a callable is called
    with the LongTensor of ids), then runs the layers outwards with `SageConv.forward_block`.  Layer l samples with
    (seed + l * 0x9E3779B97F4A7C15) mod 2^64, so the layers draw independently; seed=None draws one from torch's CPU
    generator.  One 4-byte read-back per layer; no hipGraph capture.  `blocks(nodes, seed)` returns the list
    (innermost first) for inspection."""

    def __init__(self, features, graph, convs):
        super().__init__()
        convs = list(convs)
        if not convs or not all(isinstance(c, SageConv) for c in convs):
            raise TypeError("NestedSageEncoder: convs must be a non-empty sequence of SageConv layers")
        for a, b in zip(convs, convs[1:]):
            if b.input_dim != a.out_dim:
                raise ValueError(f"NestedSageEncoder: a layer of input_dim {b.input_dim} follows one of out_dim {a.out_dim}")
        if not isinstance(graph, (CsrGraph, CsrBatch)):
            raise TypeError(f"NestedSageEncoder: graph must be a CsrGraph or CsrBatch, got {type(graph).__name__}")
        if isinstance(features, torch.Tensor) and not isinstance(features, torch.nn.Parameter):
            self.register_buffer("features", features, persistent=False)
        elif isinstance(features, (torch.nn.Module, torch.nn.Parameter)) or callable(features):
            self.features = features
        else:
            raise TypeError(f"NestedSageEncoder: features must be a tensor, an nn.Embedding or a callable, got "
                            f"{type(features).__name__}")
        self.graph, self.convs, self.embed_dim = graph, torch.nn.ModuleList(convs), convs[-1].out_dim

    @staticmethod
    def layer_seed(seed, layer):
        return (seed + layer * LAYER_SEED_STEP) % (1 << 64)

    def blocks(self, nodes, seed):
        """The layers' blocks, innermost first: blocks[-1] has the targets `nodes`, blocks[l - 1] the targets blocks[l]."""
        ids = ops.check_target_nodes("NestedSageEncoder", nodes, self.graph.n)
        if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
            raise ValueError(f"NestedSageEncoder: seed must be a Python int in [0, 2^64), got {seed!r}")
        targets = ids.to(device=self.graph.indptr.device, dtype=torch.int32)
        out = []
        for layer in range(len(self.convs) - 1, -1, -1):
            targets = self.convs[layer].block(self.graph, targets, self.layer_seed(seed, layer), nodes_checked=True)
            out.append(targets)
        return out[::-1]

    def forward(self, nodes, seed=None):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())       # the CPU generator: no device sync
        blocks = self.blocks(nodes, seed)
        ids = blocks[0].src.long()
        f = self.features
        h = f.index_select(0, ids) if isinstance(f, torch.Tensor) else f(ids)
        for conv, block in zip(self.convs, blocks):
            h = conv.forward_block(h, block)
        return h


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
