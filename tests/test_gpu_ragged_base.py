"""The base GCN encoder on ragged CSR batches (SparseBatchGcnEncoderGraph): its UNMASKED max readout, in which the padded
rows of the dense batch compete.

Op level: the padded-row table against float64 under a counted bound (tests/ragged_base_cases.py); the suffix maximum
and the floored segmented max bit for bit against numpy on small-integer tables (every column has ties); the readout's
backward exact against a host loop; dp_bn_ragged_g_bwd against float64 autograd of the padded statement in which the
padded rows receive output gradients; the pad constant without the ReLU.

Model level: against a plain-torch float64 restatement of GcnEncoderGraph.forward (encoders.py:1083-1122) on the same
graphs padded to pad_to rows, kept in this file (`ref_forward`).  The backward of the reference runs with the winners the
HIP forward recorded (tests/parity.py), after the HIP winners have been shown to hold the reference's maximum.  Each case
first asserts, on the reference alone, that padded rows do win, that real rows win as well, and that no near-tie decides.

Tolerances are the project's (tests/parity.py): outputs rtol 1e-4 / atol 1e-5; parameter gradients grads_close(rtol=2e-3,
atol_rel=1e-4), the tolerance tests/test_gpu_sparse.py uses for the single-graph base model; dx under `_close_scaled`
as tests/test_gpu_csr_batch.py documents it.

DP_RAGGED_BASE_ANCHOR_OUT=<file> appends one line per padded-row-table case with its worst error / bound
(profiles/ragged_base_fp64_anchor.txt is such a file)."""
import os

import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib, ops
from graph_pooling_amd.sparse import CsrBatch, CsrGraph, SparseBatchGcnEncoderGraph, SparseGcnEncoderGraph
from oracle import diffpool_oracle as O
from tests import ragged_base_cases as RC
from tests.parity import close, grads_close

pytestmark = pytest.mark.gpu

# the shapes of tests/test_gpu_csr_batch.py's BatchNorm test
BN_SIZES = {"equal": [17] * 5, "giant": [2000] + [30] * 12, "one_node": [1, 40, 7, 1], "single": [50],
            "two": [300, 41]}


def _close_scaled(got, ref, scale=1.0):
    """parity.close (rtol 1e-4, atol 1e-5) with the absolute floor relative to the largest reference entry."""
    close(got, ref, 1e-4 * scale, 1e-5 * scale * max(1.0, float(ref.abs().max())))


def _sizes_batch(sizes, pad_to=None):
    """A CsrBatch without edges: what the ragged row ops need."""
    return CsrBatch.from_edge_lists(sizes, [[]] * len(sizes), [[]] * len(sizes), "cuda", pad_to=pad_to)


# ------------------------------------------------------------------ the padded-row table
@pytest.mark.parametrize("F_", [1, 20, 64, 512])
@pytest.mark.parametrize("tail", [0, 3])
@pytest.mark.parametrize("name", list(BN_SIZES))
def test_padded_row_table_matches_float64_under_the_counted_bound(name, tail, F_):
    """padval rows n_min .. n_idx - 1 against the float64 padded statement, elementwise under the bound of
    tests/ragged_base_cases.py; rows below n_min are never written; y is unchanged by the extra output."""
    sizes = BN_SIZES[name]
    P = max(sizes) + tail
    n_min, max_n, n_idx = RC.table_rows(sizes, P)
    batch = _sizes_batch(sizes, pad_to=P)
    assert (batch.min_n, batch.max_n, batch.n_idx) == (n_min, max_n, n_idx)
    gen = torch.Generator().manual_seed(len(sizes) * 1000 + F_ + tail)
    x = torch.randn(sum(sizes), F_, generator=gen)
    pad = torch.rand(F_, generator=gen) * 0.5
    v64, bound = RC.padval_reference(x, pad, sizes, P)
    lib = _lib.load()
    xd, pd = x.cuda(), pad.cuda()
    y, stats = torch.empty_like(xd), torch.empty(n_idx, 2, device="cuda")
    table = torch.full((n_idx, F_), float("nan"), device="cuda")
    st = _lib.current_stream()
    _lib.check(lib.dp_bn_ragged_fwd(xd.data_ptr(), F_, y.data_ptr(), F_, stats.data_ptr(), batch.node_off.data_ptr(),
                                    batch.order.data_ptr(), batch.cnt.data_ptr(), pd.data_ptr(), len(sizes), max_n, F_,
                                    1, st), "dp_bn_ragged_fwd")
    _lib.check(lib.dp_ragged_padval_fwd(stats.data_ptr(), pd.data_ptr(), table.data_ptr(), F_, n_min, max_n, n_idx, F_,
                                        st), "dp_ragged_padval_fwd")
    got = table.cpu().double()
    assert torch.isnan(got[:n_min]).all()                       # never written
    if n_idx == n_min:
        return
    err = (got[n_min:] - v64[n_min:]).abs()
    ratio = float((err / bound[n_min:]).max())
    print(f"padded-row table {name} tail={tail} F={F_}: rows {n_min}..{n_idx - 1}, max |err| {float(err.max()):.3e}, "
          f"worst err / bound {ratio:.4f}")
    path = os.environ.get("DP_RAGGED_BASE_ANCHOR_OUT")
    if path:
        with open(path, "a") as f:
            f.write(f"{name:9s} sizes={str(sizes) if len(sizes) < 6 else str(sizes[:2]) + '...':24s} P={P:5d} F={F_:4d} "
                    f"rows={n_idx - n_min:5d}  max|err| {float(err.max()):.3e}  worst err/bound {ratio:.4f}\n")
    assert torch.isfinite(got[n_min:]).all()
    assert ratio <= 1.0, ratio
    # the autograd wrapper gives the same table and the same y as bn_relu_ragged
    y2, tab2 = ops.bn_relu_ragged_padval(xd, pd, batch)
    assert torch.equal(y2, y) and torch.equal(tab2[n_min:], table[n_min:])
    assert torch.equal(y2, ops.bn_relu_ragged(xd, pd, batch))


# ------------------------------------------------------------------ suffix maximum and floored readout
def _host_readout(z, sizes, P, table=None, row=None):
    """numpy: (out [B, F], arg [B, F]) of the unmasked max with the floor from `table` [n_idx, F] (suffix maximum from
    row n_b, lowest index on equal values) or the constant `row` [F] (winner n_b); a real row wins an exact tie."""
    B, F_ = len(sizes), z.shape[1]
    out, arg = np.zeros((B, F_), dtype=np.float32), np.zeros((B, F_), dtype=np.int32)
    o = 0
    for b, n in enumerate(sizes):
        seg = z[o:o + n]
        i = seg.argmax(axis=0)                                  # numpy: the first occurrence
        v = seg[i, np.arange(F_)]
        if n < P and table is not None:
            t = table[n:]
            j = t.argmax(axis=0)
            fv, fi = t[j, np.arange(F_)], j + n
        elif n < P and row is not None:
            fv, fi = row, np.full(F_, n)
        else:
            fv, fi = np.full(F_, -np.inf, dtype=np.float32), np.zeros(F_, dtype=np.int64)
        win = fv > v
        out[b], arg[b] = np.where(win, fv, v), np.where(win, fi, i)
        o += n
    return out, arg


def _host_backward(dout, arg, sizes, n_rows, F_, table_rows=None):
    """dZ [n_total, F] and G ([table_rows, F] or [F]) by a loop in ascending b, float32 adds in that order."""
    dz = np.zeros((n_rows, F_), dtype=np.float32)
    g = np.zeros((table_rows, F_) if table_rows else (F_,), dtype=np.float32)
    o = 0
    for b, n in enumerate(sizes):
        for f in range(F_):
            r = int(arg[b, f])
            if r < n:
                dz[o + r, f] += dout[b, f]
            elif table_rows:
                g[r, f] = np.float32(g[r, f] + dout[b, f])
            else:
                g[f] = np.float32(g[f] + dout[b, f])
        o += n
    return dz, g


READOUT_CASES = [([300, 1, 41, 700, 5], 700), ([300, 1, 41, 700, 5], 701), ([17] * 4, 17), ([17] * 4, 19), ([50], 50),
                 ([50], 53), ([200, 37, 180], 200)]


@pytest.mark.parametrize("F_", [1, 64, 65, 512])
@pytest.mark.parametrize("sizes,P", READOUT_CASES, ids=[f"{len(s)}x{max(s)}-P{p}" for s, p in READOUT_CASES])
def test_suffix_max_and_floor_readout_bit_for_bit(sizes, P, F_):
    """Small-integer tables force ties: padded against padded gives the lowest index, real against padded the real
    row.  [300, 1, 41, 700, 5] spans 11 scan blocks from n_min = 1; [200, 37, 180] three from n_min = 37.  P = max_n:
    the largest graph has no floor; P > max_n: it has the tail row's.  Forward, dZ and G are exact, twice."""
    n_min, max_n, n_idx = RC.table_rows(sizes, P)
    batch = _sizes_batch(sizes, pad_to=P)
    gen = torch.Generator().manual_seed(7 * P + F_)
    n_tot = sum(sizes)
    z = torch.randint(-3, 4, (n_tot, F_), generator=gen).float()
    z[:, : F_ // 4] -= 5.0                                       # columns the floor wins
    table = torch.randint(-3, 3, (n_idx, F_), generator=gen).float()
    if n_idx > 650:
        table[650, : max(1, F_ // 2)] = 9.0                      # one padded row that several graphs pick
    dout = torch.randn(len(sizes), F_, generator=gen)
    lib = _lib.load()
    if n_idx > n_min:
        # the suffix table itself
        tv = table.clone()
        tv[:n_min] = float("nan")                               # rows below n_min are never read
        tvd = tv.cuda()
        sufv = torch.full((n_idx, F_), float("nan"), device="cuda")
        sufi = torch.full((n_idx, F_), -7, device="cuda", dtype=torch.int32)
        wsb = lib.dp_ragged_suffix_max_workspace_bytes(n_min, n_idx, F_)
        ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
        _lib.check(lib.dp_ragged_suffix_max(tvd.data_ptr(), F_, sufv.data_ptr(), sufi.data_ptr(), F_, n_min, n_idx, F_,
                                            ws.data_ptr(), wsb, _lib.current_stream()), "dp_ragged_suffix_max")
        t = table.numpy()
        for i in sorted({n_min, min(n_min + 63, n_idx - 1), min(n_min + 64, n_idx - 1), (n_min + n_idx) // 2, n_idx - 1}
                        | set(sizes) & set(range(n_min, n_idx))):
            j = t[i:].argmax(axis=0)
            assert np.array_equal(sufv[i].cpu().numpy(), t[i:][j, np.arange(F_)]), i
            assert np.array_equal(sufi[i].cpu().numpy(), j + i), i
        assert torch.isnan(sufv[:n_min]).all() and (sufi[:n_min] == -7).all()
        floors = [("table", tvd), ("row", table[n_idx - 1].clone().cuda())]
    else:
        floors = [("none", None), ("row", table[0].clone().cuda())]            # no graph has a padded row
    for kind, floor in floors:
        runs = []
        for _ in range(2):
            zd = z.cuda().requires_grad_(True)
            fl = None if floor is None else floor.clone().requires_grad_(True)
            out, arg = ops.segment_max_floor(zd, fl, batch)
            out.backward(dout.cuda())
            runs.append((out.detach().cpu(), arg.cpu(), zd.grad.cpu(), None if fl is None or fl.grad is None
                         else fl.grad.cpu()))
        eo, ea = _host_readout(z.numpy(), sizes, P, table=table.numpy() if kind == "table" else None,
                               row=floor.cpu().numpy() if kind == "row" else None)
        out, arg, dz, g = runs[0]
        assert np.array_equal(out.numpy(), eo), kind
        assert np.array_equal(arg.numpy(), ea), kind
        edz, eg = _host_backward(dout.numpy(), ea, sizes, n_tot, F_, table_rows=n_idx if kind == "table" else None)
        assert np.array_equal(dz.numpy(), edz), kind
        if kind == "table":
            assert np.array_equal(g.numpy()[n_min:], eg[n_min:])
            padded = ea >= np.asarray(sizes)[:, None]
            assert F_ < 64 or (padded.any() and (~padded).any())
            if n_idx > 650:                                     # several graphs win the same (i, f)
                assert (np.sum(ea[:, 0] == 650) >= 3)
        elif kind == "row":
            assert np.array_equal(g.numpy(), eg)
        for a, b_ in zip(runs[0][:3], runs[1][:3]):
            assert torch.equal(a, b_), kind
        if g is not None:
            lo = n_min if kind == "table" else 0
            assert torch.equal(g[lo:], runs[1][3][lo:]), kind


# ------------------------------------------------------------------ BatchNorm backward with padded-row gradients
@pytest.mark.parametrize("F_", [1, 20, 64, 512])
@pytest.mark.parametrize("name", list(BN_SIZES))
def test_ragged_bn_backward_with_padded_row_gradients(name, F_):
    """dx and dpad against float64 autograd of the padded statement (pad_to = max_n + 3, so the tail row exists) in
    which one padded row of every node index i >= n_min receives G[i] as its output gradient: indices owned by
    several graphs (one_node: 1..6), by one graph (giant, two, one_node), by none (the tail row, every shape).  y and
    dpad under parity.close, dx under `_close_scaled` — the argument of tests/test_gpu_csr_batch.py's
    test_ragged_bn_matches_padded_float64: dx scales with rstd, which reaches hundreds at F = 1, so an entry's fp32
    rounding is set by its terms, not by the entry.  Measured (each case prints its figures): dpad at most 0.59 of
    the bound (giant, F = 512: |err| 5.1e-5 beside entries of 597); dx 1.34 of plain parity.close in one case (two,
    F = 1: |err| 3.9e-4 beside entries of 28, the case the old test reports too) and below 0.56 in every other.
    G = NULL is dp_bn_ragged_bwd bit for bit."""
    sizes = BN_SIZES[name]
    B, P = len(sizes), max(sizes) + 3
    n_min, max_n, n_idx = RC.table_rows(sizes, P)
    batch = _sizes_batch(sizes, pad_to=P)
    gen = torch.Generator().manual_seed(len(sizes) * 1000 + F_)
    x = torch.randn(sum(sizes), F_, generator=gen)
    pad = torch.rand(F_, generator=gen) * 0.5
    dy = torch.randn(sum(sizes), F_, generator=gen)
    G = torch.randn(n_idx, F_, generator=gen)
    G[:n_min] = 0

    x64 = x.double().requires_grad_(True)
    p64 = pad.double().requires_grad_(True)
    mask = O.node_mask(P, sizes, torch.float64)
    h = torch.relu(RC.pad_rows(x64, sizes, P)) * mask + p64 * (1 - mask)
    y64 = O.bn_node(h)
    dyp = RC.pad_rows(dy.double(), sizes, P)
    for i in range(n_min, n_idx):
        b = next(b for b, n in enumerate(sizes) if n <= i)       # a graph for which row i is padded
        dyp[b, i] = G[i].double()
    (y64 * dyp).sum().backward()

    xd = x.cuda().requires_grad_(True)
    pd = pad.cuda().requires_grad_(True)
    y, table = ops.bn_relu_ragged_padval(xd, pd, batch)
    Gd = G.cuda()
    Gd[:n_min] = float("nan")                                   # rows without a padded row are not read
    torch.autograd.backward([y, table], [dy.cuda(), Gd])
    close(y, RC.unpad(y64.detach(), sizes))
    for what, got, ref in (("dx", xd.grad, x64.grad), ("dpad", pd.grad, p64.grad)):
        err = (got.detach().cpu().double() - ref).abs()
        print(f"ragged bn + G {name} F={F_} {what}: max |err| {float(err.max()):.3e}, largest reference entry "
              f"{float(ref.abs().max()):.3e}, max err / (1e-5 + 1e-4 |ref|) "
              f"{float((err / (1e-5 + 1e-4 * ref.abs())).max()):.3f}")
    _close_scaled(xd.grad, x64.grad)
    close(pd.grad, p64.grad)

    # G = NULL through the C entries: the old entry's bits
    lib = _lib.load()
    st = _lib.current_stream()
    stats = torch.empty(n_idx, 2, device="cuda")
    yb = torch.empty_like(xd)
    xr, dyd = x.cuda(), dy.cuda()
    _lib.check(lib.dp_bn_ragged_fwd(xr.data_ptr(), F_, yb.data_ptr(), F_, stats.data_ptr(), batch.node_off.data_ptr(),
                                    batch.order.data_ptr(), batch.cnt.data_ptr(), pad.cuda().data_ptr(), B, max_n, F_, 1,
                                    st), "dp_bn_ragged_fwd")
    res = []
    padd = pad.cuda()
    for entry in ("old", "new"):
        dx, dpad = torch.empty_like(xr), torch.empty_like(padd)
        wsb = lib.dp_bn_ragged_workspace_bytes(n_idx, F_)
        ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
        if entry == "old":
            rc = lib.dp_bn_ragged_bwd(xr.data_ptr(), F_, yb.data_ptr(), F_, stats.data_ptr(), dyd.data_ptr(), F_,
                                      dx.data_ptr(), F_, dpad.data_ptr(), batch.node_off.data_ptr(),
                                      batch.order.data_ptr(), batch.cnt.data_ptr(), padd.data_ptr(), B, max_n, F_, 1,
                                      ws.data_ptr(), wsb, st)
        else:
            rc = lib.dp_bn_ragged_g_bwd(xr.data_ptr(), F_, yb.data_ptr(), F_, stats.data_ptr(), dyd.data_ptr(), F_,
                                        dx.data_ptr(), F_, dpad.data_ptr(), None, F_, batch.node_off.data_ptr(),
                                        batch.order.data_ptr(), batch.cnt.data_ptr(), padd.data_ptr(), B, max_n, n_idx,
                                        F_, 1, ws.data_ptr(), wsb, st)
        _lib.check(rc, entry)
        res.append((dx, dpad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("scale", [0.0, 0.5, 1e-20])
def test_row_constant_without_relu_and_its_bias_gradient(scale):
    """c = F.normalize(bias) and dbias through the l2norm Jacobian against torch float64 autograd — also at a zero bias
    and below F.normalize's eps, where the Jacobian is identity / eps."""
    gen = torch.Generator().manual_seed(7)
    bias = (torch.rand(20, generator=gen) * 2 - 1) * scale
    dc = torch.randn(20, generator=gen)
    b64 = bias.double().requires_grad_(True)
    c64 = torch.nn.functional.normalize(b64, p=2, dim=0, eps=1e-12)
    c64.backward(dc.double())
    bd = bias.cuda().requires_grad_(True)
    c = ops.gcn_row_const(bd, _lib.F_NORMALIZE)
    c.backward(dc.cuda())
    close(c, c64.detach())
    _close_scaled(bd.grad, b64.grad)
    if scale == 0.5:
        assert float(c.min()) < 0                               # no ReLU
        assert torch.equal(torch.relu(c), ops.gcn_pad_const(bd.detach(), _lib.F_NORMALIZE))


def test_launch_entries_refuse_bad_arguments_with_a_gpu_present():
    lib = _lib.load()
    p = torch.zeros(64, device="cuda").data_ptr()
    assert lib.dp_segment_max_floor_fwd(p, 4, p, p, p, 1, p, p, p, 4, 1, 2, p, p, 4, p, 1, 4, p, 4096, None) == -1
    assert b"not both" in lib.dp_last_error_string()
    assert lib.dp_segment_max_floor_fwd(p, 4, p, p, p, 1, None, None, None, 4, 1, 2, p, p, 4, p, 1, 4, p, 4096, None) == -1
    assert b"floor_flag" in lib.dp_last_error_string()


# ------------------------------------------------------------------ the model
NCLS = 3
SIZES_A = [5, 9, 9, 14, 3, 1, 14]
SIZES_B = [300, 30, 17, 8, 30, 17, 8, 30, 17, 8]
SIZES_C = [70, 33, 5, 64, 65, 1]
# (sizes, pad_to, (F, H, E), seed with bn / without): the seed draws the chords, the parameters and x.  About one seed
# in three keeps every readout gap above 1e-4 of the layer's largest entry at these widths (hundreds of maxima per
# case); the ones below do, and check_premises asserts it.
SHAPES = {"a": (SIZES_A, None, (7, 12, 9), {True: 2, False: 2}), "a_pad20": (SIZES_A, 20, (7, 12, 9), {True: 2, False: 2}),
          "b": (SIZES_B, None, (9, 20, 20), {True: 8, False: 10}), "c": (SIZES_C, None, (20, 64, 65), {True: 8, False: 9})}


def ref_forward(P64, xpad, adj, n_pred_hidden, bn, winners=None):
    """GcnEncoderGraph.forward (encoders.py:1083-1122) in plain torch on the padded batch xpad [B, P, F], adj [B, P, P]:
    GraphConv (l2-normalised) -> ReLU -> apply_bn for every layer but the last, torch.max over ALL P rows per layer,
    concat, pred_model.  `winners`: per layer int [B, F_layer] rows that replace the arg-max.  Returns (ypred, layers)."""
    keys = ["conv_first", "conv_block.0", "conv_last"]
    h, outs, layers = xpad, [], []
    for li, k in enumerate(keys):
        h = torch.matmul(torch.matmul(adj, h), P64[k + ".weight"]) + P64[k + ".bias"]
        h = torch.nn.functional.normalize(h, p=2, dim=2, eps=1e-12)
        if li < len(keys) - 1:
            h = torch.relu(h)
            if bn:
                mu = h.mean(dim=(0, 2), keepdim=True)
                var = (h - mu).pow(2).mean(dim=(0, 2), keepdim=True)
                h = (h - mu) / torch.sqrt(var + 1e-5)
        layers.append(h)
        if winners is None:
            outs.append(h.max(dim=1)[0])
        else:
            outs.append(torch.gather(h, 1, winners[li].to(torch.int64).unsqueeze(1)).squeeze(1))
    feat = torch.cat(outs, dim=1)
    names = ["pred_model"] if n_pred_hidden == 0 else [f"pred_model.{2 * i}" for i in range(n_pred_hidden + 1)]
    for i, nme in enumerate(names):
        feat = torch.nn.functional.linear(feat, P64[nme + ".weight"], P64[nme + ".bias"])
        if i < len(names) - 1:
            feat = torch.relu(feat)
    return feat, layers


def check_premises(layers, sizes, P, bn, two_indices=True):
    """On the reference alone: every layer has a padded and a real winner among the graphs with padding; with BN some
    layer has two different padded indices winning; every readout gap that is not an exact tie (the maximum against the
    largest value below it) is at least 1e-4 of the layer's largest entry.  Returns the smallest relative gap."""
    nb = torch.tensor(sizes)
    two_pad, worst = False, float("inf")
    for li, h in enumerate(layers):
        v, i = h.max(dim=1)
        padded = (i >= nb[:, None])[nb < P]
        assert padded.any(), f"layer {li}: no padded row wins"
        assert (~padded).any(), f"layer {li}: no real row wins among the graphs with padding"
        if bn and li < len(layers) - 1:
            two_pad = two_pad or len({int(t) for t in i[i >= nb[:, None]]}) >= 2
        below = torch.where(h < v.unsqueeze(1), h, torch.full_like(h, -float("inf"))).max(dim=1)[0]
        gap = (v - below)[torch.isfinite(below)] / float(h.abs().max())
        worst = min(worst, float(gap.min()))
    assert two_pad or not (bn and two_indices), "no BatchNorm layer has two different padded indices winning"
    assert worst >= 1e-4, f"a readout gap of {worst:.2e} of the layer's largest entry"
    return worst


def _case(shape, bn, hidden, bias_scale=0.3, seed=None):
    sizes, pad_to, (F_, H, E), seeds = SHAPES[shape]
    seed = seeds[bn] if seed is None else seed
    srcs, dsts = RC.ring_with_chords(sizes, seed)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda", pad_to=pad_to)
    P = batch.pad_to
    adj = RC.dense_adj(sizes, srcs, dsts, P)
    x = torch.randn(sum(sizes), F_, generator=torch.Generator().manual_seed(seed + 10))
    model = SparseBatchGcnEncoderGraph(F_, H, E, NCLS, 3, pred_hidden_dims=hidden, bn=bn)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed, bias_scale=bias_scale)
    model.load_state_dict(params)
    label = torch.tensor([b % NCLS for b in range(len(sizes))])
    return model.cuda(), params, batch, adj, x, label, sizes, P


def _run(model, x, batch, label):
    model.zero_grad(set_to_none=True)
    xd = x.cuda().requires_grad_(True)
    ypred = model(xd, batch)
    loss = model.loss(ypred, label.cuda())
    loss.backward()
    return ypred, loss, xd.grad


def _check_against_reference(model, params, batch, adj, x, label, sizes, P, bn, hidden, two_indices=True):
    P64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    xpad = RC.pad_rows(x64, sizes, P)
    yfree, layers = ref_forward(P64, xpad, adj, len(hidden), bn)
    gap = check_premises([h.detach() for h in layers], sizes, P, bn, two_indices)
    print(f"smallest readout gap: {gap:.2e} of the layer's largest entry")
    ypred, loss, dx = _run(model, x, batch, label)
    assert ypred.shape == (len(sizes), NCLS)
    win = [model.saved_activation(li, "readout_argmax").clone().cpu() for li in range(3)]
    nb = torch.tensor(sizes)
    for li, (w, h) in enumerate(zip(win, layers)):
        assert w.dtype == torch.int32 and w.shape == (len(sizes), h.shape[2])
        assert int(w.min()) >= 0 and int(w.max()) < P
        assert bool((w[nb == P] < P).all()) and bool((w[(w >= nb[:, None])] <= max(sizes)).all())
        # the HIP winners hold the reference's maximum
        held = torch.gather(h.detach(), 1, w.to(torch.int64).unsqueeze(1)).squeeze(1)
        close(held, h.detach().max(dim=1)[0])
    yw, _ = ref_forward(P64, xpad, adj, len(hidden), bn, winners=win)
    lo = torch.nn.functional.cross_entropy(yw, label)
    lo.backward()
    close(ypred, yfree.detach())
    close(ypred, yw.detach())
    close(loss, lo.detach(), 1e-4, 1e-6)
    grads_close(model, {k: v.grad for k, v in P64.items()}, rtol=2e-3, atol_rel=1e-4)
    _close_scaled(dx, x64.grad)
    assert torch.equal(model.predict(x.cuda(), batch).cpu(), yfree.argmax(dim=1))
    return win


@pytest.mark.parametrize("hidden", [[], [50]], ids=["linear", "mlp50"])
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_equals_the_float64_restatement_on_the_padded_batch(shape, bn, hidden):
    model, params, batch, adj, x, label, sizes, P = _case(shape, bn, hidden)
    win = _check_against_reference(model, params, batch, adj, x, label, sizes, P, bn, hidden)
    nb = torch.tensor(sizes)
    assert any(bool((w >= nb[:, None]).any()) for w in win)      # the HIP run took padded winners too


def test_batch_with_zero_biases():
    """Zero GraphConv biases: every padded row is zero in front of the BatchNorm and behind the last layer; behind the
    BatchNorm it is -mean_i rstd_i, still a value per node index — but the same in every column, so one node index holds
    the suffix maximum of all columns and the premise of two different padded winners does not apply (no seed of eight
    gave two); the other premises hold and are asserted."""
    model, params, batch, adj, x, label, sizes, P = _case("a_pad20", True, [50], bias_scale=0.0)
    _check_against_reference(model, params, batch, adj, x, label, sizes, P, True, [50], two_indices=False)


def test_one_graph_batch_without_padding_equals_the_single_graph_call():
    n = 97
    srcs, dsts = RC.ring_with_chords([n], 3)
    g = CsrGraph.from_edges(n, srcs[0], dsts[0], "cuda", symmetric=True)
    batch = CsrBatch.from_graphs([g])
    assert batch.pad_to == n and batch.n_idx == batch.min_n == n
    x = torch.randn(n, 9, generator=torch.Generator().manual_seed(1)).cuda()
    single = SparseGcnEncoderGraph(9, 20, 20, NCLS, 3, pred_hidden_dims=[50])
    params = O.init_params({k: tuple(v.shape) for k, v in single.state_dict().items()}, seed=4, bias_scale=0.3)
    single.load_state_dict(params)
    model = SparseBatchGcnEncoderGraph(9, 20, 20, NCLS, 3, pred_hidden_dims=[50])
    model.load_state_dict(single.state_dict())
    single, model = single.cuda(), model.cuda()
    label = torch.tensor([1]).cuda()
    y1 = single(x, g)
    l1 = torch.nn.functional.cross_entropy(y1, label)
    l1.backward()
    yb = model(x, batch)
    lb = model.loss(yb, label)
    lb.backward()
    close(yb, y1)
    close(lb, l1, 1e-4, 1e-6)
    grads_close(model, {k: p.grad for k, p in single.named_parameters()}, rtol=2e-3, atol_rel=1e-4)
    close(model(x, g), y1)                                       # a CsrGraph goes to the parent's forward


def test_two_runs_are_bit_identical():
    model, params, batch, adj, x, label, sizes, P = _case("b", True, [50])
    runs = []
    for _ in range(2):
        ypred, loss, dx = _run(model, x, batch, label)
        runs.append((ypred.detach().clone(), loss.detach().clone(), dx.clone(),
                     {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k


def _kernel_launches(sizes):
    srcs, dsts = RC.ring_with_chords(sizes, 1)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda")
    model = SparseBatchGcnEncoderGraph(9, 20, 20, NCLS, 3, pred_hidden_dims=[50]).cuda()
    x = torch.randn(sum(sizes), 9, generator=torch.Generator().manual_seed(0))
    label = torch.tensor([b % NCLS for b in range(len(sizes))])
    _run(model, x, batch, label)                                 # warm up: lazy module loads
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        _run(model, x, batch, label)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def test_launch_count_does_not_grow_with_the_batch():
    n2, n8 = _kernel_launches([200, 90]), _kernel_launches([200, 90, 150, 30, 170, 200, 64, 120])
    assert n2 == n8 and n2 > 0, (n2, n8)


def test_batch_with_a_5748_node_graph_forward():
    """DD's largest graph next to a small one: a finite forward that agrees with the oracle's dense base_forward."""
    sizes = [5748, 100]
    srcs, dsts = RC.ring_with_chords(sizes, 3)
    batch = CsrBatch.from_edge_lists(sizes, srcs, dsts, "cuda")
    x = torch.randn(sum(sizes), 9, generator=torch.Generator().manual_seed(3))
    model = SparseBatchGcnEncoderGraph(9, 20, 20, NCLS, 3, pred_hidden_dims=[50])
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=3, bias_scale=0.3)
    model.load_state_dict(params)
    model = model.cuda()
    with torch.no_grad():
        ypred = model(x.cuda(), batch)
    assert torch.isfinite(ypred).all()
    adj = RC.dense_adj(sizes, srcs, dsts, 5748, dtype=torch.float32)
    yo = O.base_forward(params, RC.pad_rows(x, sizes, 5748), adj, n_pred_hidden=1)
    close(ypred, yo)
    w = model.saved_activation(1, "readout_argmax").cpu()
    assert bool((w[1] >= 100).any()) and int(w.max()) < 5748     # the small graph's readout takes padded rows


def test_training_steps_lower_the_loss():
    from graph_pooling_amd.optim import FusedClipAdam
    model, params, batch, adj, x, label, sizes, P = _case("c", True, [50])
    opt = FusedClipAdam(model, lr=1e-2, clip=2.0)
    xd, ld = x.cuda(), label.cuda()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model.loss(model(xd, batch), ld)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k
