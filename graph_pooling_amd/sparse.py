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
prediction head run on dp_bgemm_f32 (`hip_linear`).  No torch arithmetic on the path.

`SparseSoftPoolingGcnEncoder` does the same for DiffPool (`SoftPoolingGcnEncoder`): level 0 on the CSR ops above plus
dp_csr_pool_fwd / bwd for the pooling S^T Z, S^T A S (encoders.py:1278-1279), the small pooled levels on the dense
per-op entries with B = 1.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .encoders import GraphConv, SoftPoolingGcnEncoder, _GraphConvFn


# ----------------------------------------------------------------------------- Linear on the HIP GEMM
class _LinearFn(torch.autograd.Function):
    """y = x W^T + b (nn.Linear layout, W [out, in]) on dp_bgemm_f32 — forward and both gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        _lib.require_gpu_tensor(x, "x")
        x = x.contiguous().float()
        w = weight.contiguous()
        rows, fin = x.shape
        fout = w.shape[0]
        y = torch.empty(rows, fout, device=x.device, dtype=torch.float32)
        st = _lib.current_stream()
        _lib.check(lib.dp_bgemm_f32(x.data_ptr(), w.data_ptr(), y.data_ptr(), _lib.ptr(bias), 1, rows, fout, fin, fin, fin,
                                    fout, 0, 0, 0, 0, 1, 1.0, 0.0, 0, st), "dp_bgemm_f32")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        rows, fin = x.shape
        fout = w.shape[0]
        st = _lib.current_stream()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)          # dx = dy W
            _lib.check(lib.dp_bgemm_f32(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), None, 1, rows, fin, fout, fout, fin,
                                        fin, 0, 0, 0, 0, 0, 1.0, 0.0, 0, st), "dp_bgemm_f32")
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)          # dW = dy^T x
            _lib.check(lib.dp_bgemm_f32(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), None, 1, fout, fin, rows, fout, fin,
                                        fin, 0, 0, 0, 1, 0, 1.0, 0.0, 0, st), "dp_bgemm_f32")
        if ctx.has_bias and ctx.needs_input_grad[2]:
            ones = torch.ones(1, rows, device=x.device, dtype=torch.float32)      # db = 1^T dy
            db = torch.empty(fout, device=x.device, dtype=torch.float32)
            _lib.check(lib.dp_bgemm_f32(ones.data_ptr(), dy.data_ptr(), db.data_ptr(), None, 1, 1, fout, rows, rows,
                                        fout, fout, 0, 0, 0, 0, 0, 1.0, 0.0, 0, st), "dp_bgemm_f32")
        return dx, dw, db


def hip_linear(x, weight, bias=None):
    """nn.Linear's arithmetic (x @ weight.T + bias) on the library's fp32 MFMA GEMM; x [rows, in]."""
    return _LinearFn.apply(x, weight, bias)


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


class _SparseGraphConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, g, flags):
        lib = _lib.load()
        _lib.require_gpu_tensor(x, "x")
        x = x.contiguous().float()
        w = weight.contiguous()
        n, fin = x.shape
        fout = w.shape[1]
        y = torch.empty(n, fout, device=x.device, dtype=torch.float32)
        ax = torch.empty(n, fin, device=x.device, dtype=torch.float32)
        invn = torch.empty(n, device=x.device, dtype=torch.float32)
        wsb = lib.dp_sparse_gcn_layer_workspace_bytes(n, fin, fout)
        ws = torch.empty(wsb, device=x.device, dtype=torch.uint8)
        _lib.check(lib.dp_sparse_gcn_layer_fwd(x.data_ptr(), fin, g.indptr.data_ptr(), g.indices.data_ptr(), w.data_ptr(),
                                               _lib.ptr(bias), y.data_ptr(), fout, ax.data_ptr(), invn.data_ptr(), n,
                                               fin, fout, flags, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_sparse_gcn_layer_fwd")
        ctx.save_for_backward(ax, w, y, invn)
        ctx.g, ctx.flags, ctx.ws, ctx.has_bias = g, flags, ws, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        ax, w, y, invn = ctx.saved_tensors
        g = ctx.g
        n, fin = ax.shape
        fout = w.shape[1]
        dy = dy.contiguous()
        dx = torch.empty_like(ax) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty(fout, device=ax.device, dtype=torch.float32) if ctx.has_bias else None
        _lib.check(lib.dp_sparse_gcn_layer_bwd(ax.data_ptr(), g.indptr.data_ptr(), g.indices.data_ptr(),
                                               g.indptr_t.data_ptr(), g.indices_t.data_ptr(), w.data_ptr(), y.data_ptr(),
                                               fout, invn.data_ptr(), dy.data_ptr(), fout, _lib.ptr(dx), fin,
                                               dw.data_ptr(), _lib.ptr(db), n, fin, fout, ctx.flags, ctx.ws.data_ptr(),
                                               ctx.ws.numel(), _lib.current_stream()), "dp_sparse_gcn_layer_bwd")
        return dx, dw, db, None, None


class _BnNodeFn(torch.autograd.Function):
    """apply_bn (encoders.py:1048-1052) after ReLU on ONE graph: dp_bn_node_* with a batch of one."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = x.contiguous()
        n, f = x.shape
        y = torch.empty_like(x)
        stats = torch.empty(n, 2, device=x.device, dtype=torch.float32)
        wsb = lib.dp_bn_node_workspace_bytes(1, n, f)
        ws = torch.empty(wsb, device=x.device, dtype=torch.uint8)
        _lib.check(lib.dp_bn_node_fwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), 1, n, f, 1, ws.data_ptr(), wsb,
                                      _lib.current_stream()), "dp_bn_node_fwd")
        ctx.save_for_backward(x, y, stats)
        ctx.ws = ws
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, stats = ctx.saved_tensors
        n, f = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _lib.check(lib.dp_bn_node_bwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), dy.data_ptr(), f, dx.data_ptr(),
                                      f, 1, n, f, 1, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream()),
                   "dp_bn_node_bwd")
        return dx


class _RowMaxFn(torch.autograd.Function):
    """max over the node rows (torch.max(x, dim=1), encoders.py:1093) through dp_masked_max_* with B = 1."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = x.contiguous()
        n, f = x.shape
        out = torch.empty(1, f, device=x.device, dtype=torch.float32)
        arg = torch.empty(1, f, device=x.device, dtype=torch.int32)
        _lib.check(lib.dp_masked_max_fwd(x.data_ptr(), f, None, out.data_ptr(), f, arg.data_ptr(), 1, n, f,
                                         _lib.current_stream()), "dp_masked_max_fwd")
        ctx.save_for_backward(arg)
        ctx.shape = (n, f)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        n, f = ctx.shape
        dx = torch.zeros(n, f, device=dout.device, dtype=torch.float32)
        dout = dout.contiguous()
        _lib.check(lib.dp_masked_max_bwd(dout.data_ptr(), f, arg.data_ptr(), dx.data_ptr(), f, 1, n, f,
                                         _lib.current_stream()), "dp_masked_max_bwd")
        return dx


class SparseGcnEncoderGraph(nn.Module):
    """`GcnEncoderGraph` (encoders.py:976-1134) on one CSR graph: forward(x [n, F], graph) -> ypred [1, label_dim].

    Same constructor arguments and `state_dict` keys as the dense class (conv_first / conv_block.i / conv_last /
    pred_model...), so parameters move between the two with load_state_dict."""

    def __init__(self, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=[], concat=True,
                 bn=True, dropout=0.0, args=None):
        super().__init__()
        if dropout > 0.001:
            raise NotImplementedError("dropout on the CSR path")
        self.concat, self.bn, self.num_layers, self.label_dim = concat, bn, num_layers, label_dim
        bias = True if args is None else args.bias
        add_self = not concat
        self.conv_first = GraphConv(input_dim, hidden_dim, add_self=add_self, normalize_embedding=True, bias=bias)
        self.conv_block = nn.ModuleList([GraphConv(hidden_dim, hidden_dim, add_self=add_self, normalize_embedding=True,
                                                   bias=bias) for _ in range(num_layers - 2)])
        self.conv_last = GraphConv(hidden_dim, embedding_dim, add_self=add_self, normalize_embedding=True, bias=bias)
        pin = hidden_dim * (num_layers - 1) + embedding_dim if concat else embedding_dim
        if len(pred_hidden_dims) == 0:
            self.pred_model = nn.Linear(pin, label_dim)
        else:
            layers = []
            for d in pred_hidden_dims:
                layers += [nn.Linear(pin, d), nn.ReLU()]
                pin = d
            layers.append(nn.Linear(pin, label_dim))
            self.pred_model = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, GraphConv):
                nn.init.xavier_uniform_(m.weight.data, gain=nn.init.calculate_gain('relu'))
                if m.bias is not None:
                    nn.init.constant_(m.bias.data, 0.0)

    def _conv(self, m, x, g):
        flags = (_lib.F_ADD_SELF if m.add_self else 0) | (_lib.F_NORMALIZE if m.normalize_embedding else 0)
        return _SparseGraphConvFn.apply(x, m.weight, m.bias, g, flags)

    def forward(self, x, graph: CsrGraph):
        if x.dim() != 2 or x.shape[0] != graph.n:
            raise ValueError(f"expected x [n, F] with n = {graph.n}, got {tuple(x.shape)}")
        outs = []
        h = x
        for m in [self.conv_first] + list(self.conv_block):
            h = self._conv(m, h, graph)
            h = _BnNodeFn.apply(h) if self.bn else torch.relu(h)      # ReLU is fused into the BN kernel
            outs.append(_RowMaxFn.apply(h))
        outs.append(_RowMaxFn.apply(self._conv(self.conv_last, h, graph)))
        feat = torch.cat(outs, dim=1) if self.concat else outs[-1]
        if isinstance(self.pred_model, nn.Linear):
            return hip_linear(feat, self.pred_model.weight, self.pred_model.bias)
        h = feat
        lins = [m for m in self.pred_model if isinstance(m, nn.Linear)]
        for i, lin in enumerate(lins):
            h = hip_linear(h, lin.weight, lin.bias)
            if i < len(lins) - 1:
                h = torch.relu(h)
        return h

    @torch.no_grad()
    def predict(self, x, graph):
        return self.forward(x, graph).argmax(dim=1)


# ----------------------------------------------------------------------------- DiffPool on a CSR graph
class _ReadoutFn(torch.autograd.Function):
    """Max readout of one level's concatenated embedding (encoders.py:1257,1287) via dp_masked_max_* with B = 1; the
    arg-max rows go to `holder` (saved_activation(level, 'readout_argmax'))."""

    @staticmethod
    def forward(ctx, x, holder):
        lib = _lib.load()
        x = x.contiguous()
        n, f = x.shape
        out = torch.empty(1, f, device=x.device, dtype=torch.float32)
        arg = torch.empty(1, f, device=x.device, dtype=torch.int32)
        _lib.check(lib.dp_masked_max_fwd(x.data_ptr(), f, None, out.data_ptr(), f, arg.data_ptr(), 1, n, f,
                                         _lib.current_stream()), "dp_masked_max_fwd")
        holder.append(arg)
        ctx.save_for_backward(arg)
        ctx.shape = (n, f)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        n, f = ctx.shape
        dx = torch.zeros(n, f, device=dout.device, dtype=torch.float32)
        _lib.check(lib.dp_masked_max_bwd(dout.contiguous().data_ptr(), f, arg.data_ptr(), dx.data_ptr(), f, 1, n, f,
                                         _lib.current_stream()), "dp_masked_max_bwd")
        return dx, None


class _AssignFn(torch.autograd.Function):
    """S = softmax(z Wp^T + bp) (encoders.py:1273) on one graph: dp_assign_softmax_mask_* with B = 1, no mask."""

    @staticmethod
    def forward(ctx, z, weight, bias):
        lib = _lib.load()
        z = z.contiguous()
        n, din = z.shape
        k = weight.shape[0]
        w = weight.contiguous()
        s = torch.empty(n, k, device=z.device, dtype=torch.float32)
        wsb = lib.dp_assign_workspace_bytes(1, n, din, k)
        ws = torch.empty(wsb, device=z.device, dtype=torch.uint8)
        _lib.check(lib.dp_assign_softmax_mask_fwd(z.data_ptr(), din, w.data_ptr(), bias.data_ptr(), None, s.data_ptr(),
                                                  1, n, din, k, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_assign_softmax_mask_fwd")
        ctx.save_for_backward(z, w, s)
        ctx.ws = ws
        return s

    @staticmethod
    def backward(ctx, ds):
        lib = _lib.load()
        z, w, s = ctx.saved_tensors
        n, din = z.shape
        k = w.shape[0]
        ds = ds.contiguous()
        dz, dw = torch.empty_like(z), torch.empty_like(w)
        db = torch.empty(k, device=z.device, dtype=torch.float32)
        _lib.check(lib.dp_assign_softmax_mask_bwd(z.data_ptr(), din, w.data_ptr(), s.data_ptr(), ds.data_ptr(), None,
                                                  dz.data_ptr(), din, dw.data_ptr(), db.data_ptr(), 1, n, din, k,
                                                  ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream()),
                   "dp_assign_softmax_mask_bwd")
        return dz, dw, db


class _CsrPoolFn(torch.autograd.Function):
    """Level-0 pooling X' = S^T Z, A' = S^T A S (encoders.py:1278-1279) with A as CSR: dp_csr_pool_fwd / bwd."""

    @staticmethod
    def forward(ctx, s, z, g):
        lib = _lib.load()
        s, z = s.contiguous(), z.contiguous()
        n, k = s.shape
        d = z.shape[1]
        xp = torch.empty(k, d, device=s.device, dtype=torch.float32)
        ap = torch.empty(k, k, device=s.device, dtype=torch.float32)
        wsb = lib.dp_csr_pool_workspace_bytes(n, k, d)
        ws = torch.empty(wsb, device=s.device, dtype=torch.uint8)
        _lib.check(lib.dp_csr_pool_fwd(s.data_ptr(), k, z.data_ptr(), d, g.indptr.data_ptr(), g.indices.data_ptr(),
                                       xp.data_ptr(), ap.data_ptr(), n, k, d, ws.data_ptr(), wsb,
                                       _lib.current_stream()), "dp_csr_pool_fwd")
        ctx.save_for_backward(s, z)
        ctx.g, ctx.ws = g, ws
        return xp, ap

    @staticmethod
    def backward(ctx, dxp, dap):
        lib = _lib.load()
        s, z = ctx.saved_tensors
        g = ctx.g
        n, k = s.shape
        d = z.shape[1]
        dxp = torch.zeros(k, d, device=s.device) if dxp is None else dxp.contiguous()
        dap = torch.zeros(k, k, device=s.device) if dap is None else dap.contiguous()
        ds = torch.empty_like(s)
        dz = torch.zeros_like(z)
        _lib.check(lib.dp_csr_pool_bwd(s.data_ptr(), k, z.data_ptr(), d, g.indptr.data_ptr(), g.indices.data_ptr(),
                                       g.indptr_t.data_ptr(), g.indices_t.data_ptr(), dxp.data_ptr(), dap.data_ptr(),
                                       ds.data_ptr(), k, dz.data_ptr(), d, n, k, d, ctx.ws.data_ptr(), ctx.ws.numel(),
                                       _lib.current_stream()), "dp_csr_pool_bwd")
        return ds, dz, None


class _DensePoolFn(torch.autograd.Function):
    """Pooling of a pooled level (K_j x K_j dense adjacency): dp_pool_fwd / bwd with B = 1."""

    @staticmethod
    def forward(ctx, s, z, adj):
        lib = _lib.load()
        s, z, adj = s.contiguous(), z.contiguous(), adj.contiguous()
        n, k = s.shape
        d = z.shape[1]
        xp = torch.empty(k, d, device=s.device, dtype=torch.float32)
        ap = torch.empty(k, k, device=s.device, dtype=torch.float32)
        t = torch.empty(k, n, device=s.device, dtype=torch.float32)
        _lib.check(lib.dp_pool_fwd(s.data_ptr(), z.data_ptr(), d, adj.data_ptr(), xp.data_ptr(), ap.data_ptr(),
                                   t.data_ptr(), 1, n, k, d, _lib.current_stream()), "dp_pool_fwd")
        ctx.save_for_backward(s, z, adj, t)
        return xp, ap

    @staticmethod
    def backward(ctx, dxp, dap):
        lib = _lib.load()
        s, z, adj, t = ctx.saved_tensors
        n, k = s.shape
        d = z.shape[1]
        dxp = torch.zeros(k, d, device=s.device) if dxp is None else dxp.contiguous()
        dap = torch.zeros(k, k, device=s.device) if dap is None else dap.contiguous()
        ds, dz = torch.empty_like(s), torch.zeros_like(z)
        dadj = torch.zeros_like(adj) if ctx.needs_input_grad[2] else None
        wsb = lib.dp_pool_bwd_workspace_bytes(1, n, k, d)
        ws = torch.empty(wsb, device=s.device, dtype=torch.uint8)
        _lib.check(lib.dp_pool_bwd(s.data_ptr(), z.data_ptr(), d, adj.data_ptr(), t.data_ptr(), dxp.data_ptr(),
                                   dap.data_ptr(), ds.data_ptr(), dz.data_ptr(), d, _lib.ptr(dadj), 1, n, k, d,
                                   ws.data_ptr(), wsb, _lib.current_stream()), "dp_pool_bwd")
        return ds, dz, dadj


class _CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy with mean reduction (encoders.py:1127) on dp_cross_entropy_fwd / bwd."""

    @staticmethod
    def forward(ctx, logits, label):
        lib = _lib.load()
        logits = logits.contiguous()
        b, c = logits.shape
        label = label.to(device=logits.device, dtype=torch.int64).contiguous()
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        prob = torch.empty_like(logits)
        _lib.check(lib.dp_cross_entropy_fwd(logits.data_ptr(), label.data_ptr(), loss.data_ptr(), prob.data_ptr(), b, c,
                                            _lib.current_stream()), "dp_cross_entropy_fwd")
        ctx.save_for_backward(prob, label)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        prob, label = ctx.saved_tensors
        b, c = prob.shape
        dloss = dloss.contiguous().float()
        dlogits = torch.empty_like(prob)
        _lib.check(lib.dp_cross_entropy_bwd(prob.data_ptr(), label.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), b,
                                            c, _lib.current_stream()), "dp_cross_entropy_bwd")
        return dlogits, None


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

    Not on this path: dropout, the link-prediction loss (an n^2 term; `loss` refuses it, forward / predict work for a
    linkpred model), K_0 > 256 or a concatenated embedding wider than 512 (dp_csr_pool's limits)."""

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

    # -- stacks
    @staticmethod
    def _stack(first, block, last):
        return [first] + list(block) + [last]

    def _sparse_stack(self, mods, h, graph):
        """gcn_forward (encoders.py:1054-1081) on the CSR graph: GraphConv -> ReLU -> apply_bn, concat of all layers."""
        outs = []
        for i, m in enumerate(mods):
            flags = (_lib.F_ADD_SELF if m.add_self else 0) | (_lib.F_NORMALIZE if m.normalize_embedding else 0)
            h = _SparseGraphConvFn.apply(h, m.weight, m.bias, graph, flags)
            if i < len(mods) - 1:
                h = _BnNodeFn.apply(h)           # ReLU fused into the BN kernel; bn is always on here
            outs.append(h)
        return torch.cat(outs, dim=1)

    @staticmethod
    def _dense_stack(mods, h, adj):
        """The same on a pooled level's dense K x K adjacency (dp_gcn_layer_* with B = 1)."""
        outs = []
        for i, m in enumerate(mods):
            h = _GraphConvFn.apply(h.unsqueeze(0), adj.unsqueeze(0), m.weight, m.bias, m._flags())[0]
            if i < len(mods) - 1:
                h = _BnNodeFn.apply(h)
            outs.append(h)
        return torch.cat(outs, dim=1)

    def _head(self, feat):
        if isinstance(self.pred_model, nn.Linear):
            return hip_linear(feat, self.pred_model.weight, self.pred_model.bias)
        lins = [m for m in self.pred_model if isinstance(m, nn.Linear)]
        h = feat
        for i, lin in enumerate(lins):
            h = hip_linear(h, lin.weight, lin.bias)
            if i < len(lins) - 1:
                h = torch.relu(h)
        return h

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
        argmax = []
        saved = {"assign": [], "xpool": [], "adjpool": [], "embedding": []}
        z = self._sparse_stack(self._stack(self.conv_first, self.conv_block, self.conv_last), x, graph)   # :1254
        saved["embedding"].append(z)
        outs = [_ReadoutFn.apply(z, argmax)]                                                              # :1257
        adj, s0 = None, None
        for i in range(self.num_pooling):                                                                 # :1263
            amods = self._stack(self.assign_conv_first_modules[i], self.assign_conv_block_modules[i],
                                self.assign_conv_last_modules[i])
            pred = self.assign_pred_modules[i]
            if i == 0:
                za = self._sparse_stack(amods, x_a, graph)                                                # :1269-1271
                s = _AssignFn.apply(za, pred.weight, pred.bias)                                           # :1273
                xp, adj = _CsrPoolFn.apply(s, z, graph)                                                   # :1278-1279
                s0 = s
            else:
                za = self._dense_stack(amods, x_a, adj)                         # D4: level >= 1 assigns from X'
                s = _AssignFn.apply(za, pred.weight, pred.bias)
                xp, adj = _DensePoolFn.apply(s, z, adj)
            x_a = xp                                                                                      # :1280
            z = self._dense_stack(self._stack(self.conv_first_after_pool[i], self.conv_block_after_pool[i],
                                              self.conv_last_after_pool[i]), xp, adj)                     # :1282-1284
            outs.append(_ReadoutFn.apply(z, argmax))                                                      # :1287
            saved["assign"].append(s)
            saved["xpool"].append(xp)
            saved["adjpool"].append(adj)
            saved["embedding"].append(z)
        ypred = self._head(torch.cat(outs, dim=1))                                                        # :1295-1299
        saved["readout_argmax"] = argmax
        self._saved = saved
        self.assign_tensor = s0.unsqueeze(0)        # level-0 assignment [1, n, K_0], as the dense class keeps it
        return ypred

    @torch.no_grad()
    def predict(self, x, graph: CsrGraph, assign_x=None):
        """Arg-max class of the graph: int64 [1] on the device."""
        return self.forward(x, graph, assign_x=assign_x).argmax(dim=1)

    def loss(self, pred, label, adj=None, batch_num_nodes=None, adj_hop=1):
        """Cross entropy of the prediction (encoders.py:1124-1127).  The link-prediction term (encoders.py:1309-1331)
        is an n^2 pass over the graph and is not offered on the CSR path: a linkpred=True model refuses."""
        if self.linkpred:
            raise NotImplementedError("SparseSoftPoolingGcnEncoder.loss: the link-prediction loss (linkpred=True) is an "
                                      "n^2 term over the CSR graph and is not supported on this path; build the model "
                                      "with linkpred=False to train on CSR graphs (forward / predict work either way)")
        if adj_hop != 1:
            raise NotImplementedError("adj_hop > 1 is never used by the reference's callers (train.py:207)")
        return _CrossEntropyFn.apply(pred, label)

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
