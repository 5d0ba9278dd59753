"""The per-op layer: one autograd wrapper per dp_*_fwd / dp_*_bwd pair of libdiffpool_hip.so that the package calls
outside the whole-model entries (dp_encoder_* / dp_loss_*, encoders.py), each exposed as a plain function.

Sits below `encoders`, `csr`, `sparse` and `graphsage`: it imports only `_lib`, numpy and torch.  Every wrapper makes its inputs
contiguous, allocates the outputs and the workspace the C entry asks for, and keeps for the backward what the forward
wrote (the workspace included, where the backward entry reads it).  No torch arithmetic, no CPU path.  Line numbers
cite the reference's encoders.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def _f32(like, *shape):
    """A fresh, uninitialised fp32 tensor on `like`'s device."""
    return torch.empty(*shape, device=like.device, dtype=torch.float32)


def _workspace(nbytes, like):
    """The buffer a dp_*_workspace_bytes call asked for, on `like`'s device."""
    return torch.empty(nbytes, device=like.device, dtype=torch.uint8)


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
        y = _f32(x, rows, fout)
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
            db = _f32(x, fout)
            _lib.check(lib.dp_bgemm_f32(ones.data_ptr(), dy.data_ptr(), db.data_ptr(), None, 1, 1, fout, rows, rows,
                                        fout, fout, 0, 0, 0, 0, 0, 1.0, 0.0, 0, st), "dp_bgemm_f32")
        return dx, dw, db


def hip_linear(x, weight, bias=None):
    """nn.Linear's arithmetic (x @ weight.T + bias) on the library's fp32 MFMA GEMM; x [rows, in]."""
    return _LinearFn.apply(x, weight, bias)


def mlp_head(feat, linears):
    """pred_model (encoders.py:1295-1299) on `hip_linear`: ReLU between the Linear layers, none after the last."""
    for i, lin in enumerate(linears):
        feat = hip_linear(feat, lin.weight, lin.bias)
        if i < len(linears) - 1:
            feat = torch.relu(feat)
    return feat


# ----------------------------------------------------------------------------- GraphConv, dense and CSR
class _GraphConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, weight, bias, flags):
        lib = _lib.load()
        _lib.require_gpu_tensor(x, "x")
        x = x.contiguous().float()
        adj = adj.contiguous().float()
        B, n, fin = x.shape
        fout = weight.shape[1]
        y, invn = _f32(x, B, n, fout), _f32(x, B, n)
        wsb = lib.dp_gcn_layer_workspace_bytes(B, n, fin, fout)
        ws = _workspace(wsb, x)
        w = weight.contiguous()
        _lib.check(lib.dp_gcn_layer_fwd(x.data_ptr(), fin, adj.data_ptr(), w.data_ptr(), _lib.ptr(bias),
                                        y.data_ptr(), fout, invn.data_ptr(), B, n, fin, fout, flags,
                                        ws.data_ptr(), wsb, _lib.current_stream()), "dp_gcn_layer_fwd")
        ctx.save_for_backward(x, adj, w, y, invn)
        ctx.flags, ctx.ws, ctx.has_bias = flags, ws, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, adj, w, y, invn = ctx.saved_tensors
        B, n, fin = x.shape
        fout = w.shape[1]
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dadj = torch.empty_like(adj) if ctx.needs_input_grad[1] else None
        dw = torch.empty_like(w)
        db = _f32(x, fout) if ctx.has_bias else None
        _lib.check(lib.dp_gcn_layer_bwd(x.data_ptr(), fin, adj.data_ptr(), w.data_ptr(), y.data_ptr(), fout,
                                        invn.data_ptr(), dy.data_ptr(), fout, _lib.ptr(dx), fin, dw.data_ptr(),
                                        _lib.ptr(db), _lib.ptr(dadj), B, n, fin, fout, ctx.flags,
                                        ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream()), "dp_gcn_layer_bwd")
        return dx, dadj, dw, db, None


def graph_conv(x, adj, weight, bias, flags):
    """y = l2norm((adj @ x [+ x]) @ W + b) (encoders.py:945-974) on a dense batch: x [B, n, F], adj [B, n, n],
    W [F, F']; `flags` is `GraphConv._flags()`."""
    return _GraphConvFn.apply(x, adj, weight, bias, flags)


def _weighted(graph):
    """A CsrGraph / CsrBatch that stores values: its ops take the `_w` entries (same launches; the values are data)."""
    return bool(getattr(graph, "weighted", False))


def _csr_args(g, local=False, null_t=False):
    """How every CSR entry takes the adjacency of a CsrGraph / CsrBatch `g`: (entry-name suffix, (indptr, indices
    [, values]), (indptr_t, indices_t [, values_t])) as device pointers — the values and the suffix of the weighted
    entry when `g` stores values.  `local`: the graph-local index arrays of a CsrBatch (link loss).  `null_t`: NULL for
    the transposed group of an undirected container (the Frobenius entries then skip the A^T S gather)."""
    ix, ix_t = (g.indices_local, g.indices_t_local) if local else (g.indices, g.indices_t)
    null = null_t and g.undirected
    if _weighted(g):
        return ("_w", (g.indptr.data_ptr(), ix.data_ptr(), g.values.data_ptr()),
                (None, None, None) if null else (g.indptr_t.data_ptr(), ix_t.data_ptr(), g.values_t.data_ptr()))
    return "", (g.indptr.data_ptr(), ix.data_ptr()), (None, None) if null else (g.indptr_t.data_ptr(), ix_t.data_ptr())


def _csr_index_args(g, mirror=None):
    """`_csr_args` for the entries that read no stored values: ((indptr, indices), (indptr_t, indices_t[, mirror_perm])) as
    device pointers, no suffix.  An edgeless CsrGraph has empty `indices`: `indptr` goes in their place — never read, never
    NULL (an edgeless CsrBatch keeps a one-element pad).  `mirror`: 'always' appends the container's `mirror_perm`
    (built on first use), 'own' NULL for an undirected container, whose own order serves as the transposed one."""
    ix = g.indices if g.indices.numel() else g.indptr
    ix_t = g.indices_t if g.indices_t.numel() else g.indptr_t
    at = (g.indptr_t.data_ptr(), ix_t.data_ptr())
    if mirror is not None:
        at += (None if mirror == "own" and g.undirected else g.mirror_perm.data_ptr(),)
    return (g.indptr.data_ptr(), ix.data_ptr()), at


def check_rows(who, graph, name, t, cols=None):
    """`t` is a tensor [n, cols] with n = graph.n, else ValueError.  `who` opens the message ('csr_sddmm: ', or '');
    cols None: the rows as the container words them (`graph.rows()`)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != graph.n:
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        want = graph.rows() if cols is None else f"[n, {cols}] with n = {graph.n}"
        raise ValueError(f"{who}expected {name} {want}, got {got}")


def finite_slope(who, negative_slope):
    """A leaky-ReLU slope as a finite float, else ValueError."""
    slope = float(negative_slope)
    if slope != slope or slope in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: negative_slope must be finite, got {negative_slope!r}")
    return slope


def _call(lib, name, *args):
    """Call the C entry `name` and raise on a non-zero return code."""
    _lib.check(getattr(lib, name)(*args), name)


def _grad_values(graph):
    """The container's `values` when a gradient is wanted for them (they require grad and grad mode is on), else None:
    the one more tensor input of the Functions that read the adjacency.  With None the entries called are those of a
    container whose values are data."""
    v = getattr(graph, "values", None)
    return v if v is not None and v.requires_grad and torch.is_grad_enabled() else None


def _link_dvalues(lib, s, g, objective, dloss):
    """dloss * dL/dvalues of a link term (objective 0: cross entropy, 1: Frobenius) of s [n, k] on container `g`, in the
    order of `g.values` — dp_csr_link_dvalues: one launch for a graph or a batch (the block-diagonal CSR, global
    columns), 1 / sum_b n_b^2 from the host."""
    n, k = s.shape
    dv = torch.empty_like(g.values)
    sizes = g.node_off_host.astype("int64")
    inv_norm = 1.0 / float(((sizes[1:] - sizes[:-1]) ** 2).sum())
    _call(lib, "dp_csr_link_dvalues", s.data_ptr(), k, *_csr_args(g)[1], dv.data_ptr(), n, k, objective, inv_norm,
          dloss.data_ptr(), _lib.current_stream())
    return dv


def _pool_dvalues(lib, s, g, dap):
    """dvalues of A' = S^T A S for the gradient dap [B, k, k] ([k, k] for one graph): dp_csr_pool_dvalues."""
    n, k = s.shape
    dv = torch.empty_like(g.values)
    wsb = lib.dp_csr_pool_dvalues_workspace_bytes(n, k)
    ws = _workspace(wsb, s)
    _call(lib, "dp_csr_pool_dvalues", s.data_ptr(), k, *_csr_args(g)[1][:2], dap.data_ptr(),
          g.node_off_host.ctypes.data if g.is_batch else None, g.num_graphs, dv.data_ptr(), n, k, ws.data_ptr(), wsb,
          _lib.current_stream())
    return dv


class _CsrGraphConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, g, flags, vals=None):
        lib = _lib.load()
        _lib.require_gpu_tensor(x, "x")
        x = x.contiguous().float()
        w = weight.contiguous()
        n, fin = x.shape
        fout = w.shape[1]
        y, ax, invn = _f32(x, n, fout), _f32(x, n, fin), _f32(x, n)
        wsb = lib.dp_sparse_gcn_layer_workspace_bytes(n, fin, fout)
        ws = _workspace(wsb, x)
        sfx, a, _ = _csr_args(g)
        _call(lib, "dp_sparse_gcn_layer_fwd" + sfx, x.data_ptr(), fin, *a, w.data_ptr(), _lib.ptr(bias), y.data_ptr(),
              fout, ax.data_ptr(), invn.data_ptr(), n, fin, fout, flags, ws.data_ptr(), wsb, _lib.current_stream())
        ctx.save_for_backward(ax, w, y, invn, *((x,) if vals is not None else ()))      # dvalues[e] = dax_i . x_j
        ctx.g, ctx.flags, ctx.ws, ctx.has_bias = g, flags, ws, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        ax, w, y, invn = ctx.saved_tensors[:4]
        g = ctx.g
        n, fin = ax.shape
        fout = w.shape[1]
        dy = dy.contiguous()
        dx = torch.empty_like(ax) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = _f32(ax, fout) if ctx.has_bias else None
        sfx, a, at = _csr_args(g)
        if ctx.needs_input_grad[5]:
            x = ctx.saved_tensors[4]
            dv = torch.empty_like(g.values)
            _call(lib, "dp_sparse_gcn_layer_bwd_dv", ax.data_ptr(), *a, *at, w.data_ptr(), y.data_ptr(), fout,
                  invn.data_ptr(), dy.data_ptr(), fout, _lib.ptr(dx), fin, dw.data_ptr(), _lib.ptr(db), x.data_ptr(), fin,
                  dv.data_ptr(), n, fin, fout, ctx.flags, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream())
            return dx, dw, db, None, None, dv
        _call(lib, "dp_sparse_gcn_layer_bwd" + sfx, ax.data_ptr(), *a, *at, w.data_ptr(), y.data_ptr(), fout,
              invn.data_ptr(), dy.data_ptr(), fout, _lib.ptr(dx), fin, dw.data_ptr(), _lib.ptr(db), n, fin, fout,
              ctx.flags, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream())
        return dx, dw, db, None, None, None


def csr_graph_conv(x, weight, bias, graph, flags):
    """`graph_conv` on node rows x [n, F] with the adjacency as CSR: `graph` (a CsrGraph, or a CsrBatch with its
    block-diagonal CSR and n = n_total) carries int32 indptr / indices of A and of A^T (the neighbour sum A x is the
    gather of dp_csr_aggregate, the backward gathers over A^T) and, when it is `weighted`, their fp32 values.  Values that
    require grad receive dvalues[e] = dax_i . x_j (dp_sparse_gcn_layer_bwd_dv); `values_t` stays data."""
    return _CsrGraphConvFn.apply(x, weight, bias, graph, flags, _grad_values(graph))


# ----------------------------------------------------------------------------- row ops on one graph (B = 1)
def _bnf(x):
    """(B, n, f) of x [n, f] (one graph) or x [B, n, f] (a dense batch)."""
    return (1,) + tuple(x.shape) if x.dim() == 2 else tuple(x.shape)


class _BnReluNodesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = x.contiguous()
        b, n, f = _bnf(x)
        y = torch.empty_like(x)
        stats = _f32(x, n, 2)
        wsb = lib.dp_bn_node_workspace_bytes(b, n, f)
        ws = _workspace(wsb, x)
        _lib.check(lib.dp_bn_node_fwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), b, n, f, 1, ws.data_ptr(), wsb,
                                      _lib.current_stream()), "dp_bn_node_fwd")
        ctx.save_for_backward(x, y, stats)
        ctx.ws = ws
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, stats = ctx.saved_tensors
        b, n, f = _bnf(x)
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _lib.check(lib.dp_bn_node_bwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), dy.data_ptr(), f, dx.data_ptr(),
                                      f, b, n, f, 1, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream()),
                   "dp_bn_node_bwd")
        return dx


def bn_relu_nodes(x):
    """apply_bn (encoders.py:1048-1052) after ReLU on ONE graph, x [n, f]: dp_bn_node_* with a batch of one, the ReLU
    fused into the kernel.  x [B, n, f]: the same on a dense batch (the pooled levels of the CSR DiffPool model)."""
    return _BnReluNodesFn.apply(x)


class _RowMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = x.contiguous()
        b, n, f = _bnf(x)
        out = _f32(x, b, f)
        arg = torch.empty(b, f, device=x.device, dtype=torch.int32)
        _lib.check(lib.dp_masked_max_fwd(x.data_ptr(), f, None, out.data_ptr(), f, arg.data_ptr(), b, n, f,
                                         _lib.current_stream()), "dp_masked_max_fwd")
        ctx.save_for_backward(arg)
        ctx.shape = tuple(x.shape)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)      # no zero-fill launch for the unused gradient of `arg`
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        b, n, f = (1,) + ctx.shape if len(ctx.shape) == 2 else ctx.shape
        dx = torch.zeros(ctx.shape, device=dout.device, dtype=torch.float32)
        dout = dout.contiguous()
        _lib.check(lib.dp_masked_max_bwd(dout.data_ptr(), f, arg.data_ptr(), dx.data_ptr(), f, b, n, f,
                                         _lib.current_stream()), "dp_masked_max_bwd")
        return dx


def row_max(x):
    """Max over the node rows of x [n, f] (torch.max(x, dim=1), encoders.py:1093; the readouts :1257, :1287) through
    dp_masked_max_* with B = 1 and no mask -> (out [1, f], arg-max rows int32 [1, f], not differentiable).  x [B, n, f]:
    per graph of a dense batch -> (out [B, f], arg-max [B, f])."""
    return _RowMaxFn.apply(x)


# ----------------------------------------------------------------------------- DiffPool's assignment and pooling
class _AssignFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, bias):
        lib = _lib.load()
        z = z.contiguous()
        b, n, din = _bnf(z)
        k = weight.shape[0]
        w = weight.contiguous()
        s = _f32(z, *z.shape[:-1], k)
        wsb = lib.dp_assign_workspace_bytes(b, n, din, k)
        ws = _workspace(wsb, z)
        _lib.check(lib.dp_assign_softmax_mask_fwd(z.data_ptr(), din, w.data_ptr(), bias.data_ptr(), None, s.data_ptr(),
                                                  b, n, din, k, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_assign_softmax_mask_fwd")
        ctx.save_for_backward(z, w, s)
        ctx.ws = ws
        return s

    @staticmethod
    def backward(ctx, ds):
        lib = _lib.load()
        z, w, s = ctx.saved_tensors
        b, n, din = _bnf(z)
        k = w.shape[0]
        ds = ds.contiguous()
        dz, dw, db = torch.empty_like(z), torch.empty_like(w), _f32(z, k)
        _lib.check(lib.dp_assign_softmax_mask_bwd(z.data_ptr(), din, w.data_ptr(), s.data_ptr(), ds.data_ptr(), None,
                                                  dz.data_ptr(), din, dw.data_ptr(), db.data_ptr(), b, n, din, k,
                                                  ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream()),
                   "dp_assign_softmax_mask_bwd")
        return dz, dw, db


def assign_softmax(z, weight, bias):
    """S = softmax(z Wp^T + bp) (encoders.py:1273) on one graph, z [n, d]: dp_assign_softmax_mask_* with B = 1 and no
    mask (every row is a node).  z [B, n, d]: a dense batch (pooled levels), the real B.  The ragged rows of a
    CsrBatch are the first form with n = n_total."""
    return _AssignFn.apply(z, weight, bias)


class _CsrPoolFn(torch.autograd.Function):
    """One node for both containers: a CsrGraph takes dp_csr_pool_*, a CsrBatch dp_csr_pool_batch_* on its slab tables
    (`CsrBatch.pool_plan`)."""

    @staticmethod
    def forward(ctx, s, z, g, vals=None):
        lib = _lib.load()
        s, z = s.contiguous(), z.contiguous()
        n, k = s.shape
        d = z.shape[1]
        sfx, a, _ = _csr_args(g)
        head = (s.data_ptr(), k, z.data_ptr(), d, *a)
        if g.is_batch:
            b, plan = g.num_graphs, g.pool_plan(k, d)
            xp, ap = _f32(s, b, k, d), _f32(s, b, k, k)
            wsb = lib.dp_csr_pool_batch_workspace_bytes(plan.n_slabs, b, k, d)
            ws = _workspace(wsb, s)
            _call(lib, "dp_csr_pool_batch_fwd" + sfx, *head, plan.fwd_tab.data_ptr(), plan.slab_off.data_ptr(),
                  plan.n_slabs, xp.data_ptr(), ap.data_ptr(), b, n, k, d, ws.data_ptr(), wsb, _lib.current_stream())
        else:
            plan = None
            xp, ap = _f32(s, k, d), _f32(s, k, k)
            wsb = lib.dp_csr_pool_workspace_bytes(n, k, d)
            ws = _workspace(wsb, s)
            _call(lib, "dp_csr_pool_fwd" + sfx, *head, xp.data_ptr(), ap.data_ptr(), n, k, d, ws.data_ptr(), wsb,
                  _lib.current_stream())
        ctx.save_for_backward(s, z)
        ctx.g, ctx.plan, ctx.ws = g, plan, ws
        return xp, ap

    @staticmethod
    def backward(ctx, dxp, dap):
        lib = _lib.load()
        s, z = ctx.saved_tensors
        g, plan = ctx.g, ctx.plan
        n, k = s.shape
        d = z.shape[1]
        dxp, dap = dxp.contiguous(), dap.contiguous()
        ds = torch.empty_like(s)
        dz = torch.zeros_like(z)
        sfx, a, at = _csr_args(g)
        head = (s.data_ptr(), k, z.data_ptr(), d, *a, *at)
        grads = (dxp.data_ptr(), dap.data_ptr(), ds.data_ptr(), k, dz.data_ptr(), d)
        tail = (n, k, d, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream())
        if g.is_batch:
            _call(lib, "dp_csr_pool_batch_bwd" + sfx, *head, plan.bwd_tab.data_ptr(), plan.n_blocks, *grads, g.num_graphs,
                  *tail)
        else:
            _call(lib, "dp_csr_pool_bwd" + sfx, *head, *grads, *tail)
        return ds, dz, None, _pool_dvalues(lib, s, g, dap) if ctx.needs_input_grad[3] else None


def csr_pool(s, z, graph):
    """Level-0 pooling X' = S^T Z [k, d], A' = S^T A S [k, k] (encoders.py:1278-1279) with A as CSR: dp_csr_pool_*."""
    return _CsrPoolFn.apply(s, z, graph, _grad_values(graph))


class _DensePoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, z, adj):
        lib = _lib.load()
        s, z, adj = s.contiguous(), z.contiguous(), adj.contiguous()
        b, n, k = _bnf(s)
        d = z.shape[-1]
        lead = s.shape[:-2]
        xp, ap, t = _f32(s, *lead, k, d), _f32(s, *lead, k, k), _f32(s, *lead, k, n)
        _lib.check(lib.dp_pool_fwd(s.data_ptr(), z.data_ptr(), d, adj.data_ptr(), xp.data_ptr(), ap.data_ptr(),
                                   t.data_ptr(), b, n, k, d, _lib.current_stream()), "dp_pool_fwd")
        ctx.save_for_backward(s, z, adj, t)
        return xp, ap

    @staticmethod
    def backward(ctx, dxp, dap):
        lib = _lib.load()
        s, z, adj, t = ctx.saved_tensors
        b, n, k = _bnf(s)
        d = z.shape[-1]
        dxp, dap = dxp.contiguous(), dap.contiguous()
        ds, dz = torch.empty_like(s), torch.zeros_like(z)
        dadj = torch.zeros_like(adj) if ctx.needs_input_grad[2] else None
        wsb = lib.dp_pool_bwd_workspace_bytes(b, n, k, d)
        ws = _workspace(wsb, s)
        _lib.check(lib.dp_pool_bwd(s.data_ptr(), z.data_ptr(), d, adj.data_ptr(), t.data_ptr(), dxp.data_ptr(),
                                   dap.data_ptr(), ds.data_ptr(), dz.data_ptr(), d, _lib.ptr(dadj), b, n, k, d,
                                   ws.data_ptr(), wsb, _lib.current_stream()), "dp_pool_bwd")
        return ds, dz, dadj


def dense_pool(s, z, adj):
    """The same pooling on a pooled level (dense n x n adjacency): dp_pool_* with B = 1; with a leading batch
    dimension on all three (as the CSR DiffPool model calls it, B = 1 behind a CsrGraph), on a dense batch."""
    return _DensePoolFn.apply(s, z, adj)


# ----------------------------------------------------------------------------- ragged batch of CSR graphs
class _PadConstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bias, flags):
        lib = _lib.load()
        bias = bias.contiguous()
        f = bias.numel()
        pad = _f32(bias, f)
        _lib.check(lib.dp_gcn_pad_const_fwd(bias.data_ptr(), pad.data_ptr(), f, flags, _lib.current_stream()),
                   "dp_gcn_pad_const_fwd")
        ctx.save_for_backward(bias)
        ctx.flags = flags
        return pad

    @staticmethod
    def backward(ctx, dpad):
        lib = _lib.load()
        (bias,) = ctx.saved_tensors
        f = bias.numel()
        dpad = dpad.contiguous()
        dbias = torch.empty_like(bias)
        _lib.check(lib.dp_gcn_pad_const_bwd(bias.data_ptr(), dpad.data_ptr(), dbias.data_ptr(), f, ctx.flags,
                                            _lib.current_stream()), "dp_gcn_pad_const_bwd")
        return dbias, None


def gcn_pad_const(bias, flags):
    """relu(l2norm(bias)) [F]: what a padded row of the dense batch holds after a GraphConv layer and its ReLU (its
    adjacency row is zero, encoders.py:962-972) — dp_gcn_pad_const_*; the backward returns the bias gradient."""
    return _PadConstFn.apply(bias, flags)


class _BnReluRaggedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad, batch):
        lib = _lib.load()
        x = x.contiguous()
        n, f = x.shape
        pad = None if pad is None else pad.contiguous()
        y = torch.empty_like(x)
        stats = _f32(x, batch.max_n, 2)
        _lib.check(lib.dp_bn_ragged_fwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), batch.node_off.data_ptr(),
                                        batch.order.data_ptr(), batch.cnt.data_ptr(), _lib.ptr(pad), batch.num_graphs,
                                        batch.max_n, f, 1, _lib.current_stream()), "dp_bn_ragged_fwd")
        ctx.save_for_backward(x, y, stats, pad)
        ctx.batch = batch
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, stats, pad = ctx.saved_tensors
        batch = ctx.batch
        n, f = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dpad = torch.empty_like(pad) if pad is not None and ctx.needs_input_grad[1] else None
        wsb = lib.dp_bn_ragged_workspace_bytes(batch.max_n, f)
        ws = _workspace(wsb, x)
        _lib.check(lib.dp_bn_ragged_bwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), dy.data_ptr(), f,
                                        dx.data_ptr(), f, _lib.ptr(dpad), batch.node_off.data_ptr(),
                                        batch.order.data_ptr(), batch.cnt.data_ptr(), _lib.ptr(pad), batch.num_graphs,
                                        batch.max_n, f, 1, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_bn_ragged_bwd")
        return dx, dpad, None


def bn_relu_ragged(x, pad, batch):
    """apply_bn after ReLU per node index over a ragged batch, x [n_total, f]: what `bn_relu_nodes` gives on the dense
    batch padded to max_b n_b, whose padded rows all hold `pad` [f] (None: zeros) — dp_bn_ragged_*.  `batch` carries
    node_off, the size order and the owner counts (CsrBatch)."""
    return _BnReluRaggedFn.apply(x, pad, batch)


class _SegmentMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, batch):
        lib = _lib.load()
        z = z.contiguous()
        n, f = z.shape
        b = batch.num_graphs
        out = _f32(z, b, f)
        arg = torch.empty(b, f, device=z.device, dtype=torch.int32)
        nch = batch.seg_chunks
        wsb = lib.dp_segment_max_workspace_bytes(nch, f)
        ws = _workspace(wsb, z)
        _lib.check(lib.dp_segment_max_fwd(z.data_ptr(), f, batch.node_off.data_ptr(), batch.seg_tab.data_ptr(),
                                          batch.seg_off.data_ptr(), nch, batch.floor_flag.data_ptr(), out.data_ptr(), f,
                                          arg.data_ptr(), b, f, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_segment_max_fwd")
        ctx.save_for_backward(arg)
        ctx.batch, ctx.shape = batch, (n, f)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        n, f = ctx.shape
        batch = ctx.batch
        dz = torch.zeros(n, f, device=dout.device, dtype=torch.float32)
        dout = dout.contiguous()
        _lib.check(lib.dp_segment_max_bwd(dout.data_ptr(), f, arg.data_ptr(), batch.node_off.data_ptr(), dz.data_ptr(),
                                          f, batch.num_graphs, f, _lib.current_stream()), "dp_segment_max_bwd")
        return dz, None


def segment_max(z, batch):
    """Max readout per graph of a ragged batch, z [n_total, f] -> (out [B, f], graph-local arg-max rows int32 [B, f]):
    graphs with padded rows in the dense batch the CsrBatch stands for (n_b < pad_to) are floored at 0, arg-max -1
    where the zero wins — dp_segment_max_*."""
    return _SegmentMaxFn.apply(z, batch)


# -- the base encoder's UNMASKED max readout on a ragged batch: the padded rows enter the maximum
class _RowConstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bias, flags):
        lib = _lib.load()
        bias = bias.contiguous()
        f = bias.numel()
        c = _f32(bias, f)
        _lib.check(lib.dp_gcn_row_const_fwd(bias.data_ptr(), c.data_ptr(), f, flags, _lib.current_stream()),
                   "dp_gcn_row_const_fwd")
        ctx.save_for_backward(bias)
        ctx.flags = flags
        return c

    @staticmethod
    def backward(ctx, dc):
        lib = _lib.load()
        (bias,) = ctx.saved_tensors
        f = bias.numel()
        dc = dc.contiguous()
        dbias = torch.empty_like(bias)
        _lib.check(lib.dp_gcn_row_const_bwd(bias.data_ptr(), dc.data_ptr(), dbias.data_ptr(), f, ctx.flags,
                                            _lib.current_stream()), "dp_gcn_row_const_bwd")
        return dbias, None


def gcn_row_const(bias, flags):
    """l2norm(bias) [F], `gcn_pad_const` without the ReLU: what a padded row of the dense batch holds behind the LAST
    GraphConv layer (no ReLU, no BatchNorm behind it) — dp_gcn_row_const_*; the backward returns the bias gradient."""
    return _RowConstFn.apply(bias, flags)


class _BnReluRaggedPadvalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad, batch):
        lib = _lib.load()
        x = x.contiguous()
        n, f = x.shape
        pad = None if pad is None else pad.contiguous()
        y = torch.empty_like(x)
        stats = _f32(x, batch.n_idx, 2)
        padval = _f32(x, batch.n_idx, f)
        st = _lib.current_stream()
        _lib.check(lib.dp_bn_ragged_fwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), batch.node_off.data_ptr(),
                                        batch.order.data_ptr(), batch.cnt.data_ptr(), _lib.ptr(pad), batch.num_graphs,
                                        batch.max_n, f, 1, st), "dp_bn_ragged_fwd")
        _lib.check(lib.dp_ragged_padval_fwd(stats.data_ptr(), _lib.ptr(pad), padval.data_ptr(), f, batch.min_n,
                                            batch.max_n, batch.n_idx, f, st), "dp_ragged_padval_fwd")
        ctx.save_for_backward(x, y, stats, pad)
        ctx.batch = batch
        ctx.set_materialize_grads(False)      # G = None: no padded row won anything, no zero table is made up
        return y, padval

    @staticmethod
    def backward(ctx, dy, g):
        lib = _lib.load()
        x, y, stats, pad = ctx.saved_tensors
        batch = ctx.batch
        n, f = x.shape
        dy = torch.zeros_like(x) if dy is None else dy.contiguous()
        g = None if g is None else g.contiguous()
        dx = torch.empty_like(x)
        dpad = torch.empty_like(pad) if pad is not None and ctx.needs_input_grad[1] else None
        wsb = lib.dp_bn_ragged_workspace_bytes(batch.n_idx, f)
        ws = _workspace(wsb, x)
        _lib.check(lib.dp_bn_ragged_g_bwd(x.data_ptr(), f, y.data_ptr(), f, stats.data_ptr(), dy.data_ptr(), f,
                                          dx.data_ptr(), f, _lib.ptr(dpad), _lib.ptr(g), f, batch.node_off.data_ptr(),
                                          batch.order.data_ptr(), batch.cnt.data_ptr(), _lib.ptr(pad), batch.num_graphs,
                                          batch.max_n, batch.n_idx, f, 1, ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_bn_ragged_g_bwd")
        return dx, dpad, None


def bn_relu_ragged_padval(x, pad, batch):
    """`bn_relu_ragged` that also returns what the PADDED rows of the dense batch hold behind the BatchNorm: (y [n_total,
    f], padval [batch.n_idx, f]) with padval[i] = (pad - mean_i) rstd_i for the node indices i >= batch.min_n that have
    a padded row (lower rows are not written; row max_n, there when pad_to > max_n, stands for every index from max_n
    up) — dp_bn_ragged_fwd + dp_ragged_padval_fwd.  The backward takes (dy, G), G the gradient of padval (the padded
    rows' output gradients summed per node index): dp_bn_ragged_g_bwd."""
    return _BnReluRaggedPadvalFn.apply(x, pad, batch)


class _SegmentMaxFloorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, floor, batch):
        lib = _lib.load()
        z = z.contiguous()
        n, f = z.shape
        b = batch.num_graphs
        st = _lib.current_stream()
        out = _f32(z, b, f)
        arg = torch.empty(b, f, device=z.device, dtype=torch.int32)
        sufv = sufi = row = None
        if floor is not None and floor.dim() == 2:
            floor = floor.contiguous()
            sufv = torch.empty_like(floor)
            sufi = torch.empty(floor.shape, device=z.device, dtype=torch.int32)
            wsb = lib.dp_ragged_suffix_max_workspace_bytes(batch.min_n, batch.n_idx, f)
            ws = _workspace(wsb, z)
            _lib.check(lib.dp_ragged_suffix_max(floor.data_ptr(), f, sufv.data_ptr(), sufi.data_ptr(), f, batch.min_n,
                                                batch.n_idx, f, ws.data_ptr(), wsb, st), "dp_ragged_suffix_max")
        elif floor is not None:
            row = floor.contiguous()
        nch = batch.seg_chunks
        wsb = lib.dp_segment_max_workspace_bytes(nch, f)
        ws = _workspace(wsb, z)
        _lib.check(lib.dp_segment_max_floor_fwd(z.data_ptr(), f, batch.node_off.data_ptr(), batch.seg_tab.data_ptr(),
                                                batch.seg_off.data_ptr(), nch, batch.floor_flag.data_ptr(),
                                                _lib.ptr(sufv), _lib.ptr(sufi), f, batch.min_n, batch.n_idx,
                                                _lib.ptr(row), out.data_ptr(), f, arg.data_ptr(), b, f, ws.data_ptr(),
                                                wsb, st), "dp_segment_max_floor_fwd")
        ctx.save_for_backward(arg)
        ctx.batch, ctx.shape = batch, (n, f)
        ctx.floor_shape = None if floor is None else tuple(floor.shape)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        n, f = ctx.shape
        batch = ctx.batch
        dz = torch.zeros(n, f, device=dout.device, dtype=torch.float32)
        dout = dout.contiguous()
        g = None
        if ctx.floor_shape is not None and ctx.needs_input_grad[1]:
            g = torch.empty(ctx.floor_shape, device=dout.device, dtype=torch.float32)
        table = 1 if ctx.floor_shape is not None and len(ctx.floor_shape) == 2 else 0
        _lib.check(lib.dp_segment_max_floor_bwd(dout.data_ptr(), f, arg.data_ptr(), batch.node_off.data_ptr(),
                                                dz.data_ptr(), f, _lib.ptr(g), f, batch.min_n, batch.n_idx, table,
                                                batch.num_graphs, f, _lib.current_stream()),
                   "dp_segment_max_floor_bwd")
        return dz, g, None


def segment_max_floor(z, floor, batch):
    """The UNMASKED max readout per graph of a ragged batch (torch.max over all pad_to rows of the dense batch,
    encoders.py:1093), z [n_total, f] -> (out [B, f], arg-max rows of the DENSE batch int32 [B, f]: < n_b a real row,
    graph-local; in [n_b, pad_to) a padded one).  `floor` is what the padded rows hold: the table [batch.n_idx, f] of
    `bn_relu_ragged_padval` (graph b takes the suffix maximum from node index n_b up, lowest index on equal values:
    dp_ragged_suffix_max), one constant row [f] (winner n_b), or None (no graph has a padded row).  A real row wins an
    exact tie.  The backward returns (dz, G) with G shaped like `floor` — dp_segment_max_floor_*."""
    return _SegmentMaxFloorFn.apply(z, floor, batch)


def csr_pool_batch(s, z, batch):
    """`csr_pool` for every graph of a ragged batch: X' [B, k, d], A' [B, k, k] from s [n_total, k], z [n_total, d] —
    dp_csr_pool_batch_*, two launches per direction whatever B."""
    return _CsrPoolFn.apply(s, z, batch, _grad_values(batch))


def csr_link_loss_batch(s, batch):
    """The link-prediction loss of a ragged batch, sum_b sum_{i,j < n_b} l_ij / sum_b n_b^2 (encoders.py:1326-1331), of
    s [n_total, k]: dp_csr_linkpred_batch_* (per-graph launches of the single-graph kernels, one final launch)."""
    return _CsrLinkLossFn.apply(s, batch, _grad_values(batch))


# ----------------------------------------------------------------------------- Set2Set on ragged rows
class _Set2SetRaggedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, keep, w_ih, w_hh, b_ih, b_hh, wp, bp):
        lib = _lib.load()
        _lib.require_gpu_tensor(emb, "embedding")
        emb = emb.contiguous().float()
        n_total, d = emb.shape
        off, off_host, nb, t = graph.node_off, graph.node_off_host.ctypes.data, graph.num_graphs, graph.pad_to
        ts = [p.contiguous() for p in (w_ih, w_hh, b_ih, b_hh, wp, bp)]
        out = _f32(emb, nb, d)
        sb = lib.dp_set2set_ragged_save_bytes(off_host, nb, t, d) if keep else 0
        save = _workspace(sb, emb) if keep else None
        _lib.check(lib.dp_set2set_ragged_fwd(emb.data_ptr(), d, off.data_ptr(), off_host, nb, t, d,
                                             *[p.data_ptr() for p in ts], out.data_ptr(), _lib.ptr(save), sb,
                                             _lib.current_stream()), "dp_set2set_ragged_fwd")
        ctx.save_for_backward(emb, *ts, out)
        ctx.s2s = (graph, save)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        emb, w_ih, w_hh, b_ih, b_hh, wp, bp, out = ctx.saved_tensors
        graph, save = ctx.s2s
        if save is None:
            raise RuntimeError("set2set_ragged: the forward ran without a save buffer (torch.no_grad()), there is "
                               "nothing to differentiate")
        n_total, d = emb.shape
        off, off_host, nb, t = graph.node_off, graph.node_off_host.ctypes.data, graph.num_graphs, graph.pad_to
        dout = dout.contiguous().float()
        demb = torch.empty_like(emb)
        grads = [torch.empty_like(p) for p in (w_ih, w_hh, b_ih, b_hh, wp, bp)]
        wsb = lib.dp_set2set_ragged_bwd_workspace_bytes(off_host, nb, t, d)
        ws = _workspace(wsb, emb)
        _lib.check(lib.dp_set2set_ragged_bwd(emb.data_ptr(), d, off.data_ptr(), off_host, nb, t, d,
                                             w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                                             wp.data_ptr(), bp.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                             demb.data_ptr(), d, *[g.data_ptr() for g in grads], save.data_ptr(),
                                             save.numel(), ws.data_ptr(), wsb, _lib.current_stream()),
                   "dp_set2set_ragged_bwd")
        return (demb, None, None, *grads)


def set2set_ragged(emb, graph, w_ih, w_hh, b_ih, b_hh, wp, bp):
    """Set2Set.forward (set2set.py:32-57) of the ragged rows emb [n_total, d] of a CsrBatch -> [B, d]: what the dense
    kernels give on the batch zero-padded to `pad_to` rows (that many steps, the padded rows' zero logits in every
    softmax), on dp_set2set_ragged_*; a CsrGraph is the batch of one without padding -> [1, d].  Parameters in nn.LSTM /
    nn.Linear layout.  Under torch.no_grad() no per-step state is kept (the entry gets no save buffer)."""
    check_rows("set2set_ragged: ", graph, "embedding", emb, "d")
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (emb, w_ih, w_hh, b_ih, b_hh, wp, bp))
    return _Set2SetRaggedFn.apply(emb, graph, keep, w_ih, w_hh, b_ih, b_hh, wp, bp)


# ----------------------------------------------------------------------------- loss
class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label):
        lib = _lib.load()
        logits = logits.contiguous()
        b, c = logits.shape
        label = label.to(device=logits.device, dtype=torch.int64).contiguous()
        loss = _f32(logits, ())
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


def cross_entropy(logits, label):
    """F.cross_entropy with mean reduction (encoders.py:1127) on dp_cross_entropy_fwd / bwd; logits [b, c]."""
    return _CrossEntropyFn.apply(logits, label)


class _CsrLinkLossFn(torch.autograd.Function):
    """One node for both containers: a CsrGraph takes dp_csr_linkpred_loss_*, a CsrBatch dp_csr_linkpred_batch_* with its
    graph-local columns and the host offsets in the place of n."""

    @staticmethod
    def forward(ctx, s, g, vals=None):
        lib = _lib.load()
        _lib.require_gpu_tensor(s, "s")
        s = s.contiguous().float()
        n, k = s.shape
        loss = _f32(s, ())
        sfx, a, _ = _csr_args(g, local=g.is_batch)
        if g.is_batch:
            off = g.node_off_host.ctypes.data
            wsb = lib.dp_csr_linkpred_batch_workspace_bytes(off, g.num_graphs, k)
            ws = _workspace(wsb, s)
            _call(lib, "dp_csr_linkpred_batch_loss_fwd" + sfx, s.data_ptr(), k, *a, off, g.num_graphs, loss.data_ptr(), k,
                  ws.data_ptr(), wsb, _lib.current_stream())
        else:
            wsb = lib.dp_csr_linkpred_workspace_bytes(n, k)
            ws = _workspace(wsb, s)
            _call(lib, "dp_csr_linkpred_loss_fwd" + sfx, s.data_ptr(), k, *a, loss.data_ptr(), n, k, ws.data_ptr(), wsb,
                  _lib.current_stream())
        ctx.save_for_backward(s)
        ctx.g, ctx.ws = g, ws
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        (s,) = ctx.saved_tensors
        g = ctx.g
        n, k = s.shape
        dloss = dloss.contiguous().float()
        ds = torch.empty_like(s)
        sfx, a, at = _csr_args(g, local=g.is_batch)
        tail = (k, ctx.ws.data_ptr(), ctx.ws.numel(), _lib.current_stream())
        if g.is_batch:
            _call(lib, "dp_csr_linkpred_batch_loss_bwd" + sfx, s.data_ptr(), k, *a, *at, g.node_off_host.ctypes.data,
                  g.num_graphs, dloss.data_ptr(), ds.data_ptr(), k, 0, *tail)
        else:
            _call(lib, "dp_csr_linkpred_loss_bwd" + sfx, s.data_ptr(), k, *a, *at, dloss.data_ptr(), ds.data_ptr(), k, 0, n,
                  *tail)
        return ds, None, _link_dvalues(lib, s, g, 0, dloss) if ctx.needs_input_grad[2] else None


def csr_link_loss(s, graph):
    """DiffPool's link-prediction loss (encoders.py:1309-1331) of the assignment s [n, k] on ONE graph given as CSR
    (0/1 adjacency, or the stored values of a weighted graph; each edge listed once): dp_csr_linkpred_loss_* — a tile
    walk over s for the n^2 term that does not depend on the adjacency plus a gather over the edges, O(n k) memory.
    Returns the device scalar."""
    return _CsrLinkLossFn.apply(s, graph, _grad_values(graph))


# ----------------------------------------------------------------------------- assignment entropy
class _AssignEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, num_nodes):
        lib = _lib.load()
        _lib.require_gpu_tensor(s, "s")
        s = s.contiguous().float()
        b, n, k = (1,) + tuple(s.shape) if s.dim() == 2 else tuple(s.shape)
        ent = _f32(s, ())
        wsb = lib.dp_assign_entropy_workspace_bytes(b, n, k)
        ws = _workspace(wsb, s)
        _lib.check(lib.dp_assign_entropy_fwd(s.data_ptr(), k, _lib.ptr(num_nodes), 1.0, ent.data_ptr(), None, b, n, k,
                                             ws.data_ptr(), wsb, _lib.current_stream()), "dp_assign_entropy_fwd")
        ctx.save_for_backward(s)
        ctx.num_nodes, ctx.dims = num_nodes, (b, n, k)
        return ent

    @staticmethod
    def backward(ctx, dent):
        lib = _lib.load()
        (s,) = ctx.saved_tensors
        b, n, k = ctx.dims
        dent = dent.contiguous().float()
        ds = torch.empty_like(s)
        _lib.check(lib.dp_assign_entropy_bwd(s.data_ptr(), k, _lib.ptr(ctx.num_nodes), dent.data_ptr(), 1.0,
                                             ds.data_ptr(), k, 0, b, n, k, _lib.current_stream()),
                   "dp_assign_entropy_bwd")
        return ds, None


def assign_entropy(s, num_nodes=None):
    """DiffPool's assignment-entropy term E = sum over the valid rows of -s ln(s + 1e-15) / (number of valid rows) on
    dp_assign_entropy_*: s [rows, K] (a ragged assignment: every row is a node) or [B, n, K] with `num_nodes` int32 [B]
    on the device naming each graph's valid rows (None: all n).  The normaliser counts valid rows, not B * n.  Returns
    the device scalar."""
    if not isinstance(s, torch.Tensor) or s.dim() not in (2, 3):
        got = tuple(s.shape) if isinstance(s, torch.Tensor) else type(s).__name__
        raise ValueError(f"assign_entropy(s, num_nodes): s must be [rows, K] or [B, n, K], got {got}")
    if num_nodes is not None:
        if s.dim() != 3:
            raise ValueError("assign_entropy(s, num_nodes): num_nodes goes with s [B, n, K]")
        _lib.require_gpu_tensor(num_nodes, "num_nodes")
        if num_nodes.dtype != torch.int32 or num_nodes.numel() != s.shape[0]:
            raise ValueError(f"assign_entropy(s, num_nodes): num_nodes must be int32 [{s.shape[0]}], got "
                             f"{num_nodes.dtype} {tuple(num_nodes.shape)}")
        num_nodes = num_nodes.contiguous()
    return _AssignEntropyFn.apply(s, num_nodes)


# ----------------------------------------------------------------------------- Frobenius link loss
class _FrobLinkFn(torch.autograd.Function):
    """One node for the four forms: `kind` 'dense' (fp32 adjacency), 'packed' (PackedAdjacency), 'csr' (CsrGraph),
    'batch' (CsrBatch).  The forward saves W = (A + A^T) S (CSR of an undirected graph: A S) and the Gram matrices; the
    backward reads no adjacency."""

    @staticmethod
    def forward(ctx, s, adj, num_nodes, kind, vals=None):
        lib = _lib.load()
        _lib.require_gpu_tensor(s, "s")
        s = s.contiguous().float()
        st = _lib.current_stream()
        loss = _f32(s, ())
        k = s.shape[-1]
        if kind in ("dense", "packed"):
            b, n, _ = s.shape
            wsb = lib.dp_frob_link_workspace_bytes(b, n, k)
            ws = _workspace(wsb, s)
            w, g = torch.empty_like(s), _f32(s, (b, k, k))
            tail = (_lib.ptr(num_nodes), None, w.data_ptr(), g.data_ptr(), loss.data_ptr(), None, b, n, k, ws.data_ptr(),
                    wsb, st)
            if kind == "packed":
                _lib.check(lib.dp_frob_link_fwd_packed(s.data_ptr(), k, adj.pk.data_ptr(), adj.pkt.data_ptr(), *tail),
                           "dp_frob_link_fwd_packed")
            else:
                adj = adj.contiguous().float()
                _lib.check(lib.dp_frob_link_fwd(s.data_ptr(), k, adj.data_ptr(), *tail), "dp_frob_link_fwd")
            ctx.sym = 0
        else:
            n = s.shape[0]
            b = adj.num_graphs if kind == "batch" else 1
            wsb = lib.dp_csr_frob_link_workspace_bytes(n, b, k)
            ws = _workspace(wsb, s)
            w, g = torch.empty_like(s), _f32(s, (b, k, k))
            sfx, a, at = _csr_args(adj, null_t=True)
            if kind == "batch":
                _call(lib, "dp_csr_frob_link_batch_fwd" + sfx, s.data_ptr(), k, *a, *at, adj.node_off.data_ptr(), None,
                      w.data_ptr(), g.data_ptr(), loss.data_ptr(), None, b, n, k, ws.data_ptr(), wsb, st)
            else:
                _call(lib, "dp_csr_frob_link_fwd" + sfx, s.data_ptr(), k, *a, *at, None, w.data_ptr(), g.data_ptr(),
                      loss.data_ptr(), None, n, k, ws.data_ptr(), wsb, st)
            ctx.sym = int(at[0] is None)          # an undirected container: W = A S
        ctx.save_for_backward(s, w, g)
        ctx.kind, ctx.num_nodes, ctx.b = kind, num_nodes, b
        ctx.adj = adj if kind == "batch" or vals is not None else None
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        s, w, g = ctx.saved_tensors
        k = s.shape[-1]
        dloss = dloss.contiguous().float()
        ds = torch.empty_like(s)
        st = _lib.current_stream()
        head = (s.data_ptr(), k, w.data_ptr(), g.data_ptr())
        if ctx.kind in ("dense", "packed"):
            fn = lib.dp_frob_link_bwd_packed if ctx.kind == "packed" else lib.dp_frob_link_bwd
            _lib.check(fn(*head, _lib.ptr(ctx.num_nodes), None, dloss.data_ptr(), ds.data_ptr(), k, 0, s.shape[0],
                          s.shape[1], k, st), "dp_frob_link_bwd")
        elif ctx.kind == "batch":
            _lib.check(lib.dp_csr_frob_link_batch_bwd(*head, ctx.adj.node_off.data_ptr(), None, dloss.data_ptr(),
                                                      ds.data_ptr(), k, 0, ctx.sym, ctx.b, s.shape[0], k, st),
                       "dp_csr_frob_link_batch_bwd")
        else:
            _lib.check(lib.dp_csr_frob_link_bwd(*head, None, dloss.data_ptr(), ds.data_ptr(), k, 0, ctx.sym, s.shape[0], k,
                                                st), "dp_csr_frob_link_bwd")
        return ds, None, None, None, _link_dvalues(lib, s, ctx.adj, 1, dloss) if ctx.needs_input_grad[4] else None


def frob_link_loss(s, adj, num_nodes=None):
    """The Frobenius link loss sum_b sum_{i,j < n_b} (a_bij - s_bi . s_bj)^2 / sum_b n_b^2 — the DiffPool paper's
    ||A - S S^T||_F^2 over the normaliser of the cross-entropy link term; all pairs, the diagonal included, no clamp;
    unpinned by the reference, which has no such term — on dp_frob_link_* / dp_csr_frob_link_*, without any n x n
    temporary.  Dense: s [B, N, K] with adj an fp32 [B, N, N] tensor (any values) or a `PackedAdjacency`, `num_nodes`
    int32 [B] on the device (None: all N).  Ragged: s [n, K] with a `CsrGraph`, or s [n_total, K] with a `CsrBatch`
    (0/1 adjacency, or a weighted container's stored values; each entry stored once).  Returns the device scalar."""
    if not isinstance(s, torch.Tensor) or s.dim() not in (2, 3):
        got = tuple(s.shape) if isinstance(s, torch.Tensor) else type(s).__name__
        raise ValueError(f"frob_link_loss(s, adj, num_nodes): s must be [n, K] or [B, N, K], got {got}")
    if s.dim() == 3:
        if isinstance(adj, torch.Tensor):
            if tuple(adj.shape) != (s.shape[0], s.shape[1], s.shape[1]):
                raise ValueError(f"frob_link_loss: adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
            _lib.require_gpu_tensor(adj, "adj")
            kind = "dense"
        elif hasattr(adj, "pk") and hasattr(adj, "pkt"):
            if adj.B != s.shape[0] or adj.N != s.shape[1]:
                raise ValueError(f"frob_link_loss: packed adjacency [B={adj.B}, N={adj.N}] does not match s "
                                 f"{tuple(s.shape)}")
            kind = "packed"
        else:
            raise TypeError("frob_link_loss: s [B, N, K] goes with an fp32 [B, N, N] tensor or a PackedAdjacency, got "
                            f"{type(adj).__name__}")
        if num_nodes is not None:
            _lib.require_gpu_tensor(num_nodes, "num_nodes")
            if num_nodes.dtype != torch.int32 or num_nodes.numel() != s.shape[0]:
                raise ValueError(f"frob_link_loss: num_nodes must be int32 [{s.shape[0]}], got {num_nodes.dtype} "
                                 f"{tuple(num_nodes.shape)}")
            num_nodes = num_nodes.contiguous()
        return _FrobLinkFn.apply(s, adj, num_nodes, kind)
    if num_nodes is not None:
        raise ValueError("frob_link_loss: num_nodes goes with s [B, N, K]")
    if not (hasattr(adj, "indptr") and hasattr(adj, "indices")):
        raise TypeError(f"frob_link_loss: s [n, K] goes with a CsrGraph or a CsrBatch, got {type(adj).__name__}")
    if adj.n != s.shape[0]:
        raise ValueError(f"frob_link_loss: the {adj.ARG} has n = {adj.n} rows but s has {s.shape[0]}")
    return _FrobLinkFn.apply(s, adj, None, "batch" if adj.is_batch else "csr", _grad_values(adj))


# ----------------------------------------------------------------------------- learned edge weights on a CSR
def _edge_vec(t, g, what):
    """An fp32 [nnz] tensor of container `g` (one number per stored entry, in the order of `indices`), contiguous."""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != g.nnz:
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what} must hold one number per stored entry [{g.nnz}], got {got}")
    if g.nnz:
        _lib.require_gpu_tensor(t, what)
    return t.contiguous().float()


class _CsrSddmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q, g, alpha):
        lib = _lib.load()
        p, q = p.contiguous().float(), q.contiguous().float()
        f = p.shape[1]
        out = _f32(p, g.nnz)
        _call(lib, "dp_csr_sddmm", p.data_ptr(), f, q.data_ptr(), f, *_csr_index_args(g)[0], out.data_ptr(), g.n, f, alpha,
              None, 0.0, _lib.current_stream())
        ctx.save_for_backward(p, q)
        ctx.g, ctx.alpha = g, alpha
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        p, q = ctx.saved_tensors
        g, f = ctx.g, p.shape[1]
        dv = dout.contiguous() if ctx.alpha == 1.0 else dout * ctx.alpha      # A(alpha dout): one [nnz] scaling
        dp = dq = None
        a, at = _csr_index_args(g)
        if ctx.needs_input_grad[0]:          # dP = A(dout) Q: the weighted gather with the gradient as the values
            dp = torch.empty_like(p)
            _call(lib, "dp_csr_aggregate_w", q.data_ptr(), f, *a, dv.data_ptr(), dp.data_ptr(), f, g.n, f, 0.0,
                  _lib.current_stream())
        if ctx.needs_input_grad[1]:          # dQ = A(dout)^T P: the same entry on the transposed CSR, dout[mirror]
            dq = torch.empty_like(q)
            dvt = dv[g.mirror_perm.long()]
            _call(lib, "dp_csr_aggregate_w", p.data_ptr(), f, *at, dvt.data_ptr(), dq.data_ptr(), f, g.n, f, 0.0,
                  _lib.current_stream())
        return dp, dq, None, None


def csr_sddmm(p, q, graph, alpha=1.0):
    """alpha * p_i . q_j on every stored entry (i, j) of a CsrGraph / CsrBatch -> [graph.nnz] in the order of `indices`
    (dp_csr_sddmm; p, q [n, F], for a batch the concatenated rows).  Differentiable in p and q without a new kernel and
    without an atomic scatter: dP = A(dout) Q is dp_csr_aggregate_w with the gradient as the values, dQ = A(dout)^T P the
    same entry on the transposed CSR with dout[mirror_perm]."""
    for name, t in (("p", p), ("q", q)):
        check_rows("csr_sddmm: ", graph, name, t)
    if p.shape[1] != q.shape[1] or p.shape[1] < 1:
        raise ValueError(f"csr_sddmm: p and q must share a width F >= 1, got {p.shape[1]} and {q.shape[1]}")
    if graph.nnz == 0:                       # an edgeless batch: nothing stored, nothing launched
        return _f32(p, 0)
    _lib.require_gpu_tensor(p, "p")
    _lib.require_gpu_tensor(q, "q")
    return _CsrSddmmFn.apply(p, q, graph, float(alpha))


class _CsrEdgeSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, g):
        lib = _lib.load()
        out = torch.empty_like(scores)
        _call(lib, "dp_csr_edge_softmax_fwd", scores.data_ptr(), _csr_index_args(g)[0][0], out.data_ptr(), g.n, g.nnz,
              _lib.current_stream())
        ctx.save_for_backward(out)
        ctx.g = g
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (out,) = ctx.saved_tensors
        g = ctx.g
        dout = dout.contiguous()
        ds = torch.empty_like(out)
        _call(lib, "dp_csr_edge_softmax_bwd", out.data_ptr(), dout.data_ptr(), _csr_index_args(g)[0][0], ds.data_ptr(),
              g.n, g.nnz, _lib.current_stream())
        return ds, None


def csr_edge_softmax(scores, graph):
    """Softmax of scores [nnz] over each node's neighbour list (each row of the CSR; for a batch its block-diagonal
    CSR) -> [nnz]: dp_csr_edge_softmax_*.  A row with one entry gives exactly 1."""
    scores = _edge_vec(scores, graph, "csr_edge_softmax: scores")
    return scores if graph.nnz == 0 else _CsrEdgeSoftmaxFn.apply(scores, graph)


class _CsrSymNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, g):
        lib = _lib.load()
        dev = g.indptr.device
        out = torch.empty(g.nnz, device=dev, dtype=torch.float32)
        rdeg = torch.empty(g.n, device=dev, dtype=torch.float32)
        # an undirected container stores a_ij = a_ji: its own order serves as the transposed one (no mirror read)
        a, at = _csr_index_args(g, mirror="own")
        _call(lib, "dp_csr_sym_norm_fwd", *a, _lib.ptr(values), *at, rdeg.data_ptr(), out.data_ptr(), g.n, g.nnz,
              _lib.current_stream())
        if values is not None:
            ctx.save_for_backward(values, rdeg)
        ctx.g = g
        ctx.mark_non_differentiable(rdeg)
        return out, rdeg

    @staticmethod
    def backward(ctx, dout, _drdeg):
        lib = _lib.load()
        values, rdeg = ctx.saved_tensors
        g = ctx.g
        dout = dout.contiguous()
        dv, gdeg = torch.empty_like(values), torch.empty_like(rdeg)
        a, at = _csr_index_args(g, mirror="always")
        _call(lib, "dp_csr_sym_norm_bwd", *a, values.data_ptr(), *at, rdeg.data_ptr(), dout.data_ptr(), gdeg.data_ptr(),
              dv.data_ptr(), g.n, g.nnz, _lib.current_stream())
        return dv, None


def csr_sym_normalize_rdeg(values, graph):
    """(D^-1/2 A D^-1/2 as [nnz] values, r = d^-1/2 [n]) of container `graph` with the stored `values` ([nnz], or None for
    a 0/1 container: ones) — dp_csr_sym_norm_*: d is the column sum of the values as the reference takes it
    (graph_sampler.py:27-29), on the device, differentiable in `values` (every stored entry its own variable)."""
    if values is not None:
        values = _edge_vec(values, graph, "csr_sym_normalize: values")
    dev = graph.indptr.device
    if graph.nnz == 0:
        out = torch.empty(0, device=dev, dtype=torch.float32) if values is None else values
        return out, torch.full((graph.n,), float("inf"), device=dev, dtype=torch.float32)
    _lib.require_gpu_tensor(graph.indptr, "the container's index arrays")
    if values is None:
        with torch.no_grad():
            return _CsrSymNormFn.apply(None, graph)
    return _CsrSymNormFn.apply(values, graph)


def csr_sym_normalize(values, graph):
    """`csr_sym_normalize_rdeg` without the degrees: the [nnz] values of D^-1/2 A D^-1/2."""
    return csr_sym_normalize_rdeg(values, graph)[0]


# ----------------------------------------------------------------------------- additive multi-head attention
class _CsrGatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, g, slope):
        lib = _lib.load()
        u, v = u.contiguous().float(), v.contiguous().float()
        heads = u.shape[1]
        out, rowstat = _f32(u, g.nnz), _f32(u, g.n, 2 * heads)
        _call(lib, "dp_csr_gat_fwd", u.data_ptr(), heads, v.data_ptr(), heads, *_csr_index_args(g)[0], out.data_ptr(),
              rowstat.data_ptr(), g.n, g.nnz, heads, slope, _lib.current_stream())
        ctx.save_for_backward(u, v, rowstat)
        ctx.g, ctx.slope = g, slope
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        u, v, rowstat = ctx.saved_tensors
        g, heads = ctx.g, u.shape[1]
        dout = dout.contiguous()
        du, dv, tdot = torch.empty_like(u), torch.empty_like(v), torch.empty_like(u)
        a, at = _csr_index_args(g, mirror="always")
        _call(lib, "dp_csr_gat_bwd", u.data_ptr(), heads, v.data_ptr(), heads, *a, *at, rowstat.data_ptr(),
              dout.data_ptr(), tdot.data_ptr(), du.data_ptr(), heads, dv.data_ptr(), heads, g.n, g.nnz, heads,
              ctx.slope, _lib.current_stream())
        return du, dv, None, None


def csr_gat_attention(u, v, graph, negative_slope=0.2):
    """The mean over H heads of softmax_j(leaky_relu(u_ih + v_jh)) on every stored entry (i, j) of a CsrGraph / CsrBatch
    -> fp32 [graph.nnz] in the order of `indices`: dp_csr_gat_fwd / _bwd, one fused pass (u, v [n, H], 1 <= H <= 8, for a
    batch the concatenated rows).  Nothing of size nnz * H is written: the backward recomputes the coefficients from u, v
    and the [n, 2H] row maxima and sums, and returns du, dv.  A row with one entry gives exactly 1."""
    for name, t in (("u", u), ("v", v)):
        check_rows("csr_gat_attention: ", graph, name, t, "H")
    if u.shape[1] != v.shape[1] or not 1 <= u.shape[1] <= _lib.CSR_GAT_MAX_HEADS:
        raise ValueError(f"csr_gat_attention: u and v must share H heads, 1 <= H <= {_lib.CSR_GAT_MAX_HEADS}, got "
                         f"{u.shape[1]} and {v.shape[1]}")
    slope = finite_slope("csr_gat_attention", negative_slope)
    if graph.nnz == 0:                       # an edgeless container: nothing stored, nothing launched
        return _f32(u, 0)
    _lib.require_gpu_tensor(u, "u")
    _lib.require_gpu_tensor(v, "v")
    return _CsrGatFn.apply(u, v, graph, slope)


# ----------------------------------------------------------------------------- multi-head GAT convolution
class _CsrGatConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, u, v, g, heads, slope, mean):
        lib = _lib.load()
        z, u, v = z.contiguous().float(), u.contiguous().float(), v.contiguous().float()
        width = z.shape[1]
        c = width // heads
        y, rowstat = _f32(z, g.n, c if mean else width), _f32(z, g.n, 2 * heads)
        _call(lib, "dp_csr_gat_conv_fwd", z.data_ptr(), width, u.data_ptr(), heads, v.data_ptr(), heads,
              *_csr_index_args(g)[0], y.data_ptr(), y.shape[1], rowstat.data_ptr(), g.n, g.nnz, heads, c, slope, mean,
              _lib.current_stream())
        ctx.save_for_backward(z, u, v, rowstat)
        ctx.g, ctx.heads, ctx.slope, ctx.mean = g, heads, slope, mean
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        z, u, v, rowstat = ctx.saved_tensors
        g, heads = ctx.g, ctx.heads
        dy = dy.contiguous()
        dz, du, dv, tdot = torch.empty_like(z), torch.empty_like(u), torch.empty_like(v), torch.empty_like(u)
        a, at = _csr_index_args(g)
        _call(lib, "dp_csr_gat_conv_bwd", z.data_ptr(), z.shape[1], u.data_ptr(), heads, v.data_ptr(), heads, *a, *at,
              rowstat.data_ptr(), dy.data_ptr(), dy.shape[1], tdot.data_ptr(), du.data_ptr(), heads, dv.data_ptr(), heads,
              dz.data_ptr(), z.shape[1], g.n, g.nnz, heads, z.shape[1] // heads, ctx.slope, ctx.mean,
              _lib.current_stream())
        return dz, du, dv, None, None, None, None


def csr_gat_conv(z, u, v, graph, heads, negative_slope=0.2, concat=True):
    """One graph-attention layer's aggregation on a CsrGraph / CsrBatch: per head h the softmax over node i's stored
    entries of leaky_relu(u_ih + v_jh) multiplied into the neighbours' head-h features, y_i^h = sum_j a_ijh z_j^h
    (dp_csr_gat_conv_fwd / _bwd; z [n, heads * C] with head h in columns h C .. h C + C - 1, u, v [n, heads],
    1 <= heads <= 8, heads * C <= 512; for a batch the concatenated rows).  concat=True returns [n, heads * C], the heads
    side by side; concat=False their mean [n, C].  The container's stored values are not read.  Nothing of size nnz is
    written or saved: the backward recomputes every coefficient from u, v and the [n, 2 heads] row maxima and sums, and
    returns dz, du, dv.  A node without stored entries gets a zero row.  An edgeless container returns zeros without a
    launch and without an autograd node: z, u and v then receive NO gradient (None, not zeros)."""
    if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= _lib.CSR_GAT_MAX_HEADS:
        raise ValueError(f"csr_gat_conv: heads must be 1 .. {_lib.CSR_GAT_MAX_HEADS}, got {heads!r}")
    for name, t, cols in (("z", z, "heads * C"), ("u", u, "heads"), ("v", v, "heads")):
        check_rows("csr_gat_conv: ", graph, name, t, cols)
    if u.shape[1] != heads or v.shape[1] != heads:
        raise ValueError(f"csr_gat_conv: u and v must be [n, heads] with heads = {heads}, got {tuple(u.shape)} and "
                         f"{tuple(v.shape)}")
    width = z.shape[1]
    if width == 0 or width % heads:
        raise ValueError(f"csr_gat_conv: z has {width} columns, not a positive multiple of heads = {heads}")
    if width > _lib.CSR_GAT_CONV_MAX_WIDTH:
        raise ValueError(f"csr_gat_conv: z has {width} columns, more than the supported heads * C <= "
                         f"{_lib.CSR_GAT_CONV_MAX_WIDTH}")
    slope = finite_slope("csr_gat_conv", negative_slope)
    if graph.nnz == 0:                       # an edgeless container: every node gets a zero row, nothing launched
        return z.new_zeros((graph.n, width if concat else width // heads), dtype=torch.float32)
    for name, t in (("z", z), ("u", u), ("v", v)):
        _lib.require_gpu_tensor(t, name)
    return _CsrGatConvFn.apply(z, u, v, graph, heads, slope, 0 if concat else 1)


# ----------------------------------------------------------------------------- sampled neighbour mean
class _CsrSampleMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, nodes, k, seed, mode):
        lib = _lib.load()
        x = x.contiguous().float()
        n, feat = x.shape
        m = n if nodes is None else nodes.numel()
        width = 2 * feat if mode == _lib.CSR_SAMPLE_SELF["concat"] else feat
        y = _f32(x, m, width)
        thr = torch.empty(m, device=x.device, dtype=torch.int64)
        cnt = torch.empty(m, device=x.device, dtype=torch.int32)
        _call(lib, "dp_csr_sample_mean_fwd", x.data_ptr(), feat, *_csr_index_args(g)[0], _lib.ptr(nodes), y.data_ptr(),
              width, thr.data_ptr(), cnt.data_ptr(), m, n, feat, k, mode, seed, _lib.current_stream())
        ctx.save_for_backward(thr, cnt)
        ctx.g, ctx.nodes, ctx.seed, ctx.mode, ctx.shape = g, nodes, seed, mode, (n, feat)
        ctx.mark_non_differentiable(thr, cnt)
        ctx.set_materialize_grads(False)                                 # no zero-filled "gradients" of thr and cnt
        return y, thr, cnt

    @staticmethod
    def backward(ctx, dy, _dthr, _dcnt):
        if dy is None:
            return None, None, None, None, None, None
        lib = _lib.load()
        thr, cnt = ctx.saved_tensors
        g, nodes, (n, feat) = ctx.g, ctx.nodes, ctx.shape
        dy = dy.contiguous()
        slot = None
        if nodes is not None:                                            # plumbing: one scatter
            slot = torch.full((n,), -1, device=dy.device, dtype=torch.int32)
            slot[nodes.long()] = torch.arange(nodes.numel(), device=dy.device, dtype=torch.int32)
        dx = _f32(dy, n, feat)
        _call(lib, "dp_csr_sample_mean_bwd", dy.data_ptr(), dy.shape[1], *_csr_index_args(g)[1], _lib.ptr(slot),
              thr.data_ptr(), cnt.data_ptr(), dx.data_ptr(), feat, n, feat, ctx.mode, ctx.seed, _lib.current_stream())
        return dx, None, None, None, None, None


def _sample_args(who, num_sample, seed, self_mode):
    """(k of the C entries, the seed as the signed 64-bit word they take, DP_CSR_SAMPLE_SELF_*) or ValueError."""
    if num_sample is None:
        k = _lib.CSR_SAMPLE_ALL
    elif isinstance(num_sample, int) and not isinstance(num_sample, bool) and 1 <= num_sample <= _lib.CSR_SAMPLE_MAX_K:
        k = num_sample
    else:
        raise ValueError(f"{who}: num_sample must be 1 .. {_lib.CSR_SAMPLE_MAX_K} or None (all neighbours), got "
                         f"{num_sample!r}")
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: seed must be a Python int in [0, 2^64), got {seed!r}")
    if self_mode not in _lib.CSR_SAMPLE_SELF:
        raise ValueError(f"{who}: self_mode must be 'none', 'gcn' or 'concat', got {self_mode!r}")
    return k, seed - (1 << 64) if seed >= 1 << 63 else seed, _lib.CSR_SAMPLE_SELF[self_mode]


def check_target_nodes(who, nodes, n):
    """`nodes` of `csr_sample_mean` as host numbers: integers, distinct, in 0 .. n - 1, else ValueError."""
    a = torch.as_tensor(nodes).detach().cpu()
    if a.dim() != 1 or a.is_floating_point() or a.is_complex() or a.dtype == torch.bool:
        raise ValueError(f"{who}: nodes must be a 1-d list of integer node ids, got shape {tuple(a.shape)} of {a.dtype}")
    a = a.long()
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError(f"{who}: node id outside 0 .. {n - 1}")
    if torch.unique(a).numel() != a.numel():
        raise ValueError(f"{who}: nodes must be distinct")
    return a


def csr_sample_mean_stats(x, graph, num_sample, seed, nodes=None, self_mode="none", nodes_checked=False):
    """`csr_sample_mean` with what it saves: (y, thr int64 [m], cnt int32 [m]).  thr holds the bits of each target row's
    64-bit threshold (-1: every neighbour taken), cnt the divisor; both are data."""
    k, seed64, mode = _sample_args("csr_sample_mean", num_sample, seed, self_mode)
    check_rows("csr_sample_mean: ", graph, "x", x, "F")
    if nodes is not None:
        if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int32 or nodes.dim() != 1:
            raise ValueError("csr_sample_mean: nodes must be None or an int32 tensor [m] of distinct node ids")
        if not nodes_checked:
            check_target_nodes("csr_sample_mean", nodes, graph.n)
    m = graph.n if nodes is None else nodes.numel()
    feat = x.shape[1]
    width = 2 * feat if self_mode == "concat" else feat
    if (graph.nnz == 0 and self_mode == "none") or m == 0 or feat == 0:   # nothing to gather: zeros, nothing launched
        y = x.new_zeros((m, width), dtype=torch.float32)
        return (y, torch.full((m,), -1, device=x.device, dtype=torch.int64),
                torch.zeros(m, device=x.device, dtype=torch.int32))
    _lib.require_gpu_tensor(x, "x")
    _lib.require_gpu_tensor(graph.indptr, "the container's index arrays")
    if nodes is not None:
        _lib.require_gpu_tensor(nodes, "nodes")
        nodes = nodes.contiguous()
    return _CsrSampleMeanFn.apply(x, graph, nodes, k, seed64, mode)


def csr_sample_mean(x, graph, num_sample, seed, nodes=None, self_mode="none", nodes_checked=False):
    """GraphSAGE's sampled neighbour mean on a CsrGraph / CsrBatch, drawn and taken in one fused launch
    (dp_csr_sample_mean_fwd / _bwd; MeanAggregator.forward with num_sample, aggregators.py:30-63).

    x fp32 [n, F] (for a batch the concatenated rows); `num_sample` = k in 1 .. 64, or None for every neighbour; `seed` a
    Python int in [0, 2^64); `nodes` None (row r of the result is node r) or an int32 device tensor [m] of DISTINCT node
    ids (row r is node nodes[r]; range and distinctness are checked on the host, ValueError — one read-back, which a
    caller that built `nodes` from host numbers it has checked itself skips with nodes_checked=True).  A node with at
    most k stored neighbours takes all of them; otherwise the k entries with the smallest
    key(i, j) = (h(seed, i, j) << 32) | j, h word 0 of Philox4x32-10 with the seed as its key and (i, j, 0, 0) as its counter — uniform without replacement,
    independent from row to row, and a pure function of (seed, i, j): the same seed gives the same sample and the same
    bits.  The container's stored values are not read (the sampled mean is unweighted, as the reference's).

    self_mode 'none': the mean over the sample, [m, F].  'gcn': the node joins its own sample as in the reference's
    gcn=True (`set | {i}`; a stored and sampled self loop is not counted twice), [m, F].  'concat': [x_i | mean], [m, 2F],
    GraphSAGE's own combination.  A node whose sample is empty gets ZEROS in the mean part, not the reference's
    0 / 0 = NaN.  Nothing of size nnz is written or saved: the backward re-derives the sample from the saved [m] thresholds
    over the transposed CSR, in a fixed order and without atomics (a second run gives the same bits).  An edgeless
    container with 'none' (and a call without target rows or columns) returns zeros without a launch and without an
    autograd node.  Not for hipGraph capture: the seed is a kernel argument and would be frozen."""
    return csr_sample_mean_stats(x, graph, num_sample, seed, nodes, self_mode, nodes_checked)[0]


# ----------------------------------------------------------------------------- sampled frontier blocks
class SampledBlock:
    """One layer's sampled block of a nested GraphSAGE mini-batch (`csr_sample_block`): for the targets T and the sample
    S(i) of `csr_sample_mean` at (k, seed),

    graph   the container;   k  the sample size as the C entries take it (0: every neighbour);   seed  in [0, 2^64)
    nodes   the targets: an int32 device tensor [m] of distinct ids, None (every node), or — the nested form — the
            SampledBlock whose `src` they are
    src     int32 [n_src], the ascending, duplicate-free ids of T u U_{i in T} S(i);   n_src  a Python int
    slot    int32 [n], slot[src[s]] = s and -1 elsewhere
    thr, cnt  int64 / int32 [m]: each target row's threshold bits (-1: every neighbour taken) and |S(i)|

    All of it is data (no autograd history)."""

    __slots__ = ("graph", "nodes", "src", "slot", "n_src", "thr", "cnt", "k", "seed")

    def __init__(self, graph, nodes, src, slot, n_src, thr, cnt, k, seed):
        self.graph, self.nodes, self.src, self.slot, self.n_src = graph, nodes, src, slot, n_src
        self.thr, self.cnt, self.k, self.seed = thr, cnt, k, seed

    @property
    def targets(self):
        """The target ids as the kernels read them: an int32 tensor [m], or None for every node."""
        return self.nodes.src if isinstance(self.nodes, SampledBlock) else self.nodes

    @property
    def m(self):
        t = self.targets
        return self.graph.n if t is None else t.numel()


def _seed_word(seed):
    """A seed in [0, 2^64) as the signed 64-bit word the C entries take."""
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def csr_sample_block(graph, nodes, num_sample, seed, nodes_checked=False):
    """The sampled block of one GraphSAGE layer, built on the device (dp_csr_block_build; the `unique_nodes_list` of
    MeanAggregator.forward, aggregators.py:30-63): a `SampledBlock` whose `src` holds, ascending and without duplicates,
    the targets and every node that `csr_sample_mean(.., num_sample, seed, nodes)` would gather for them — the sample is
    the same pure function of (seed, i, j).

    `nodes`: an int32 device tensor [m] of DISTINCT node ids (range and distinctness are checked on the host as in
    `csr_sample_mean`, unless nodes_checked=True), None for every node, or ANOTHER SampledBlock of the same container:
    the targets are then that block's `src` — the layer below in a nested mini-batch — and its `slot` serves the
    backward; nothing is scattered and nothing is read back for it.  Five launches whatever m and n, and ONE 4-byte
    read-back (n_src).  An empty target set returns an empty block without a launch.  Not for hipGraph capture (the
    read-back; the seed is a kernel argument); weighted sampling, num_sample > 64 and a `src` order with the targets
    first are out of scope."""
    k, seed64, _ = _sample_args("csr_sample_block", num_sample, seed, "none")
    if not hasattr(graph, "indptr") or not hasattr(graph, "n"):
        raise TypeError(f"csr_sample_block: graph must be a CsrGraph or CsrBatch, got {type(graph).__name__}")
    n = graph.n
    if isinstance(nodes, SampledBlock):
        if nodes.graph is not graph:
            raise ValueError("csr_sample_block: the block passed as nodes belongs to another container")
        targets = nodes.src
    elif nodes is None:
        targets = None
    else:
        if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int32 or nodes.dim() != 1:
            raise ValueError("csr_sample_block: nodes must be an int32 tensor [m] of distinct node ids, None or a "
                             "SampledBlock")
        if not nodes_checked:
            check_target_nodes("csr_sample_block", nodes, n)
        nodes = targets = nodes.contiguous()
    m = n if targets is None else targets.numel()
    dev = graph.indptr.device
    if m == 0 or n == 0:                                          # nothing to sample: nothing launched
        return SampledBlock(graph, nodes, torch.zeros(0, device=dev, dtype=torch.int32),
                            torch.full((n,), -1, device=dev, dtype=torch.int32), 0,
                            torch.full((m,), -1, device=dev, dtype=torch.int64),
                            torch.zeros(m, device=dev, dtype=torch.int32), k, seed)
    _lib.require_gpu_tensor(graph.indptr, "the container's index arrays")
    if targets is not None:
        _lib.require_gpu_tensor(targets, "nodes")
    lib = _lib.load()
    cap = n if k == _lib.CSR_SAMPLE_ALL else min(n, m * (k + 1))
    i32 = lambda count: torch.empty(count, device=dev, dtype=torch.int32)
    slot, src, count, cnt = i32(n), i32(cap), i32(1), i32(m)
    thr = torch.empty(m, device=dev, dtype=torch.int64)
    wsb = lib.dp_csr_block_workspace_bytes(n)
    ws = _workspace(wsb, slot)
    _call(lib, "dp_csr_block_build", *_csr_index_args(graph)[0], _lib.ptr(targets), m, n, k, seed64, slot.data_ptr(),
          src.data_ptr(), cap, count.data_ptr(), thr.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, _lib.current_stream())
    n_src = int(count.item())                                     # the one read-back of a block: 4 bytes
    return SampledBlock(graph, nodes, src[:n_src], slot, n_src, thr, cnt, k, seed)


class _CsrBlockMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, block, mode):
        lib = _lib.load()
        x_src = x_src.contiguous().float()
        feat = x_src.shape[1]
        g, targets, m = block.graph, block.targets, block.m
        width = 2 * feat if mode == _lib.CSR_SAMPLE_SELF["concat"] else feat
        y = _f32(x_src, m, width)
        thr = torch.empty(m, device=x_src.device, dtype=torch.int64)
        cnt = torch.empty(m, device=x_src.device, dtype=torch.int32)
        _call(lib, "dp_csr_block_mean_fwd", x_src.data_ptr(), feat, *_csr_index_args(g)[0], _lib.ptr(targets),
              block.slot.data_ptr(), block.n_src, y.data_ptr(), width, thr.data_ptr(), cnt.data_ptr(), m, g.n, feat,
              block.k, mode, _seed_word(block.seed), _lib.current_stream())
        ctx.save_for_backward(thr, cnt)
        ctx.block, ctx.mode, ctx.feat = block, mode, feat
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        thr, cnt = ctx.saved_tensors
        block, feat = ctx.block, ctx.feat
        g, dy = block.graph, dy.contiguous()
        if isinstance(block.nodes, SampledBlock):                        # nested: the outer block's slot IS the targets'
            tslot = block.nodes.slot
        elif block.nodes is None:
            tslot = None
        else:                                                            # plumbing: one scatter
            tslot = torch.full((g.n,), -1, device=dy.device, dtype=torch.int32)
            tslot[block.nodes.long()] = torch.arange(block.m, device=dy.device, dtype=torch.int32)
        dx = _f32(dy, block.n_src, feat)
        _call(lib, "dp_csr_block_mean_bwd", dy.data_ptr(), dy.shape[1], *_csr_index_args(g)[1], _lib.ptr(tslot),
              block.src.data_ptr(), block.n_src, thr.data_ptr(), cnt.data_ptr(), dx.data_ptr(), feat, g.n, feat, ctx.mode,
              _seed_word(block.seed), _lib.current_stream())
        return dx, None, None


def csr_block_mean(x_src, block, self_mode="none"):
    """`csr_sample_mean` on the compact rows of a `SampledBlock` (dp_csr_block_mean_fwd / _bwd; MeanAggregator.forward on
    its unique_nodes_list, aggregators.py:30-63): x_src fp32 [n_src, F] holds the features of `block.src`, the result is
    [m, F] ('none', 'gcn') or [m, 2F] ('concat'), row r for the block's r-th target, and autograd reaches x_src as
    [n_src, F].  With x_src = x[block.src] the result has the bits of `csr_sample_mean(x, graph, k, seed, targets)`, and
    the gradient is the rows `block.src` of that op's (whose other rows are zero): the selection and the order of every
    sum are the same device code.  A block without targets (or F == 0) returns zeros without a launch.  Not for hipGraph
    capture: the seed is a kernel argument and would be frozen."""
    if not isinstance(block, SampledBlock):
        raise TypeError(f"csr_block_mean: block must be a SampledBlock, got {type(block).__name__}")
    if self_mode not in _lib.CSR_SAMPLE_SELF:
        raise ValueError(f"csr_block_mean: self_mode must be 'none', 'gcn' or 'concat', got {self_mode!r}")
    if not isinstance(x_src, torch.Tensor) or x_src.dim() != 2 or x_src.shape[0] != block.n_src:
        got = tuple(x_src.shape) if isinstance(x_src, torch.Tensor) else type(x_src).__name__
        raise ValueError(f"csr_block_mean: expected x_src [n_src, F] with n_src = {block.n_src}, got {got}")
    feat = x_src.shape[1]
    if block.m == 0 or feat == 0:
        return x_src.new_zeros((block.m, 2 * feat if self_mode == "concat" else feat), dtype=torch.float32)
    _lib.require_gpu_tensor(x_src, "x_src")
    return _CsrBlockMeanFn.apply(x_src, block, _lib.CSR_SAMPLE_SELF[self_mode])


# ----------------------------------------------------------------------------- top-k pooling
class _CsrTopkGatherFn(torch.autograd.Function):
    """x_out = x[perm] * gate[perm] and its gradients to x and gate (dp_csr_topk_gather_fwd / _bwd): one launch each."""

    @staticmethod
    def forward(ctx, x, gate, perm, new_id):
        lib = _lib.load()
        x = x.contiguous().float()
        gate = None if gate is None else gate.contiguous().float()
        n, feat = x.shape
        y = _f32(x, perm.numel(), feat)
        _call(lib, "dp_csr_topk_gather_fwd", x.data_ptr(), feat, _lib.ptr(gate), perm.data_ptr(), y.data_ptr(), feat, n,
              perm.numel(), feat, _lib.current_stream())
        ctx.save_for_backward(*((x, gate) if gate is not None else ()))
        ctx.new_id, ctx.shape, ctx.n_out = new_id, (n, feat), perm.numel()
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        n, feat = ctx.shape
        x, gate = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        dy = dy.contiguous()
        dx = _f32(dy, n, feat)
        want_dgate = gate is not None and ctx.needs_input_grad[1]
        dgate = (_f32(dy, n) if feat else torch.zeros(n, device=dy.device)) if want_dgate else None
        _call(lib, "dp_csr_topk_gather_bwd", dy.data_ptr(), feat, _lib.ptr(x) if want_dgate else None, feat, _lib.ptr(gate),
              ctx.new_id.data_ptr(), dx.data_ptr(), feat, _lib.ptr(dgate), n, ctx.n_out, feat, _lib.current_stream())
        return dx, dgate, None, None


def topk_counts(num_nodes, ratio=None, k=None):
    """The kept count of every graph, on the host: k_b = min(n_b, max(1, ceil(float64(ratio) * n_b))) for 0 < ratio <= 1,
    or min(k, n_b) for an integer k >= 1 — exactly one of the two — as int64 [B]."""
    if (ratio is None) == (k is None):
        raise ValueError("csr_topk_pool: give exactly one of ratio and k")
    nn = np.asarray(num_nodes, dtype=np.int64).reshape(-1)
    if k is not None:
        if not isinstance(k, int) or isinstance(k, bool) or k < 1:
            raise ValueError(f"csr_topk_pool: k must be an integer >= 1, got {k!r}")
        return np.minimum(k, nn)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"csr_topk_pool: ratio must lie in (0, 1], got {ratio!r}")
    kb = np.ceil(np.float64(ratio) * nn.astype(np.float64)).astype(np.int64)
    return np.minimum(nn, np.maximum(1, kb))


def csr_topk_pool_stats(x, score, graph, ratio=None, k=None, gate=None):
    """`csr_topk_pool` with what it computes on the way: (x_out, graph_out, perm, new_id int32 [n] (-1: dropped), thr
    int64 [B] (the bits of every graph's threshold key; 0 where everything is kept), edge_map int32 [nnz'], edge_map_t
    (the same tensor for an undirected container)).  All but x_out are data."""
    batch = graph.is_batch
    sizes = np.asarray(graph.num_nodes if batch else [graph.n], dtype=np.int64)
    kb = topk_counts(sizes, ratio, k)
    n = graph.n
    check_rows("csr_topk_pool: ", graph, "x", x, "F")
    for name, t in (("score", score), ("gate", gate)):
        if t is None and name == "gate":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n:
            got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"csr_topk_pool: {name} must be a float32 tensor [n] with n = {n}, got {got}")
    if n == 0:
        raise ValueError("csr_topk_pool: the container has no node")
    _lib.require_gpu_tensor(x, "x")
    _lib.require_gpu_tensor(score, "score")
    _lib.require_gpu_tensor(graph.indptr, "the container's index arrays")
    if gate is not None:
        _lib.require_gpu_tensor(gate, "gate")
    lib = _lib.load()
    dev, stream = x.device, _lib.current_stream()
    nb, n_out = int(sizes.size), int(kb.sum())
    node_off_host = np.ascontiguousarray(graph.node_off_host, dtype=np.int32)
    kb_host = np.ascontiguousarray(kb, dtype=np.int32)
    new_off_host = np.concatenate([[0], np.cumsum(kb)]).astype(np.int32)
    new_off = torch.from_numpy(new_off_host).to(dev)
    i32 = lambda m: torch.empty(m, device=dev, dtype=torch.int32)
    new_id, perm, thr = i32(n), i32(n_out), torch.empty(nb, device=dev, dtype=torch.int64)
    sc = score.detach().contiguous()
    _call(lib, "dp_csr_topk_select", sc.data_ptr(), graph.node_off.data_ptr(), new_off.data_ptr(),
          node_off_host.ctypes.data, kb_host.ctypes.data, new_id.data_ptr(), perm.data_ptr(), thr.data_ptr(), n, n_out, nb,
          stream)
    wsb = lib.dp_csr_topk_workspace_bytes(n_out)
    ws = _workspace(wsb, x)

    def induce(adjacency, nnz):                                 # nnz: the stored entries, or the pad of an edgeless batch
        cap = max(nnz, 1)
        ip, ix, em = i32(n_out + 1), i32(cap), i32(cap)
        il = i32(cap) if batch else None
        _call(lib, "dp_csr_topk_induce", *adjacency, new_id.data_ptr(), perm.data_ptr(), new_off.data_ptr(), ip.data_ptr(),
              ix.data_ptr(), _lib.ptr(il), em.data_ptr(), n, n_out, nb, nnz, cap, ws.data_ptr(), wsb, stream)
        return ip, ix, il, em

    directed = not graph.undirected
    a, at = _csr_index_args(graph)
    fwd = induce(a, graph.indices.numel())
    bwd = induce(at, graph.indices_t.numel()) if directed else None

    def narrowed(arrs):
        ip, ix, il, em = arrs
        m = int(ip[-1])                                         # the one read-back of this direction
        keep = max(m, 1) if batch else m                        # an edgeless batch keeps its one-element pad
        return m, ip, ix[:keep], None if il is None else il[:keep], em[:m]

    nnz_out, ip, ix, il, em = narrowed(fwd)
    ipt = ixt = ilt = None
    em_t = em
    if directed:
        _, ipt, ixt, ilt, em_t = narrowed(bwd)
    values = values_t = None
    if graph.weighted:
        def picked(v, m):
            if m.numel() == 0 and batch:
                return torch.zeros(1, device=dev, dtype=torch.float32)
            return v[m.long()]
        values = picked(graph.values, em)
        values_t = picked(graph.values_t.detach(), em_t) if directed else None
    if batch:
        pad_to = int(topk_counts([graph.pad_to], ratio, k)[0])
        out = type(graph).from_device_csr(kb, ip, ix, il, ipt, ixt, ilt, values, values_t, pad_to=pad_to, nnz=nnz_out,
                                          node_off=new_off)
    else:
        out = type(graph).from_device_csr(n_out, ip, ix, ipt, ixt, values, values_t, nnz=nnz_out)
    x_out = _CsrTopkGatherFn.apply(x, gate, perm, new_id)
    return x_out, out, perm, new_id, thr, em, em_t


def csr_topk_pool(x, score, graph, ratio=None, k=None, gate=None):
    """Top-k pooling (gPool of Graph U-Nets; SAGPool when the score comes from a GraphConv) on a CsrGraph / CsrBatch:
    (x_out, graph_out, perm) with the k_b best-scored nodes of every graph kept — `topk_counts`: ceil(ratio * n_b), or
    min(k, n_b) — `graph_out` the induced subgraph A[perm][:, perm] as a container of the input's class, built on the
    device, and perm int32 [n'] the old global id of every new row.

    x fp32 [n, F], score fp32 [n], gate fp32 [n] or None.  Node i beats node j of its graph when score_i > score_j, or
    on equal scores when i < j; -0.0 ties with +0.0, a positive NaN ranks above +inf and a negative one below -inf, so
    exactly k_b nodes are kept whatever the scores hold.  The kept nodes keep their relative order (ascending old id),
    so rows stay sorted and an undirected container stays undirected.  x_out[r] = x[perm[r]] * gate[perm[r]] (one fp32
    multiply; a copy without gate) with gradients to x and to gate — `score` gets none through the selection; pass
    gate = tanh(score) for gPool's.  A weighted container's values' = values[edge_map] by torch indexing, so values with
    autograd history (`with_values`) receive their gradient.  The host reads back 4 bytes (nnz') per call, 8 for a
    directed container; 5 launches forward (8 directed), 1 backward, whatever B and n.  Not for hipGraph capture."""
    return csr_topk_pool_stats(x, score, graph, ratio, k, gate)[:3]
