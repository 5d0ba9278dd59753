"""k_head_fwd's staging burst (csrc/dp_head.hip): the feature row, every layer's weights and biases arrive by LDS-DMA in
64-float pieces dealt to the eight waves of the workgroup, weight rows of an even length >= 16 at an odd LDS stride (a
piece per row), everything behind one wait.  Small models (tests/head_cases.py builds them) put pred_model at the shapes
where that can go wrong:

  A  segment tails: a first Linear of 15 (5 x 3), 63, 64 and 65 floats, of 512 (one piece for each of the 8 waves) and of
     544 floats; with odd segment lengths the next segment starts at an LDS offset that is no multiple of 4;
  B  a Linear WITHOUT bias between two with one (its bias cells are zero-filled by plain stores).  The modules cannot
     train such a head (the flat-parameter code takes every Linear's bias), so this case is a forward under no_grad of a
     subclass that leaves the missing bias out of the flat buffer (it reaches into the encoder's private _tail_params /
     _pred_linears / _last_save to do so), checked on ypred alone: against fp64, a second run, and three replays of the
     captured forward;
  C  depth: one Linear, and five (DP_MAX_PRED + 1);
  D  width: dout 64, 65 and 68 (the second group of four waves takes outputs 64..); din 3 (the fourth k-quarter is
     empty), 5, 16 (padded rows), 64;
  E  stale feature columns: family P reads its last level out at featoff > 0; the evaluation save buffer -- the caller's
     -- is prefilled with 1e30 before one forward and with 0 before another, and no logit may move;
  F  B = 1 and B = 2;
  G  the LDS budget: d1 = 974 (the largest head head_supported takes at d0 = 26) and 975 (refused: the GEMM head), and
     the padded layout's own fallback: d1 = 943 (odd strides fit the limit) and 944 (they do not: dense rows).  Which
     head ran is read from the run itself: the step is profiled in this process and launches k_head_fwd exactly once
     where the table says `fused` and never where it says `generic`.  Which LDS LAYOUT a fused launch used (odd strides
     or dense rows) leaves no trace in anything the run produces -- the same bits either way, and the profiler's events
     carry no LDS size: the `(padded)` / `(dense)` tags printed here restate dp_head.hip's formulas, and on either side
     of that boundary only the outputs are checked.

Every case: the head alone against fp64 on the GPU's own inputs (head_cases.head_figures: ypred and every pred_model
gradient within max(8 e_ref, 16 * 2^-24 * max|ref|)); a second run in this process carries the same bits; three replays
of a captured step carry the same bits; the device error word reads 0.  Every figure is printed before it is asserted;
profiles/hfwd_fp64_anchor.txt keeps those of the first full run."""
import functools
import types

import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
from oracle import diffpool_oracle as O
from tests import head_cases as HC

pytestmark = pytest.mark.gpu

HEAD_FWD_THREADS = 512
HEAD_PAD_MIN_DIN = 16
PIECE = 64

C_ = HC.Case
#    name            fam  B  n  H  E  L  P  hidden        C  concat fwd       bwd       seed special
CASES = [
    C_("s_w15_din5_3", "B", 2, 6, 2, 3, 2, 0, (3,),         2, True, "fused",   "kernel",  1, None),   # 5 x 3, then din 3
    C_("s_w63",        "B", 2, 6, 3, 4, 2, 0, (9,),         2, True, "fused",   "kernel",  1, None),   # 7 x 9
    C_("s_w64_pad",    "P", 2, 3, 4, 4, 2, 1, (4,),         2, True, "fused",   "fold",    1, None),   # 16 x 4, stride 17
    C_("s_w65",        "B", 2, 6, 6, 7, 2, 0, (5,),         2, True, "fused",   "kernel",  1, None),   # 13 x 5
    C_("s_w512_o64",   "P", 2, 3, 2, 2, 2, 1, (64,),        2, True, "fused",   "fold",    1, None),   # 8 x 64; then din 64
    C_("s_w520_o65",   "P", 2, 3, 2, 2, 2, 1, (65,),        2, True, "fused",   "fold",    1, None),   # 8 x 65
    C_("s_w544_o68",   "P", 2, 3, 2, 2, 2, 1, (68,),        3, True, "fused",   "fold",    1, None),   # 8 x 68
    C_("s_lin",        "P", 2, 3, 4, 4, 2, 1, (),           2, True, "fused",   "fold",    1, None),   # one Linear
    C_("s_deep",       "P", 2, 3, 4, 4, 2, 1, (9, 8, 7, 6), 2, True, "fused",   "fold",    1, None),   # five
    C_("s_b1",         "B", 1, 6, 4, 4, 2, 0, (7, 5),       2, True, "fused",   "kernel",  1, None),
    C_("s_pad_in",     "P", 2, 5, 4, 5, 3, 1, (943,),       2, True, "fused",   "fold",    1, None),   # 32 d1 + 514 = 30 690
    C_("s_pad_out",    "P", 2, 5, 4, 5, 3, 1, (944,),       2, True, "fused",   "fold",    1, None),   # 32 d1 + 516 = 30 724
    C_("s_lds_in",     "P", 2, 5, 4, 5, 3, 1, (974,),       2, True, "fused",   "fold",    1, None),   # 31 d1 + 514 = 30 708
    C_("s_lds_out",    "P", 2, 5, 4, 5, 3, 1, (975,),       2, True, "generic", "generic", 1, None),   # 30 739
]
NAMES = [c.name for c in CASES]
CASE = {c.name: c for c in CASES}


def _build(name):
    """head_cases.build for a case of THIS table (head_cases' own dictionary is left alone): (model on the CPU with the
    case's fp32 parameters loaded, params, x, adj, num_nodes, label)."""
    c = CASE[name]
    N = HC.level_nodes(c)[0]
    x, adj, nn_, label = O.make_batch(c.B, N, HC.F, n_min=max(1, N // 2), p=0.3, seed=c.seed, n_classes=c.C)
    if c.fam == "P":
        model = SoftPoolingGcnEncoder(N, HC.F, c.H, c.E, c.C, c.L, c.H, assign_ratio=0.5, num_pooling=c.P,
                                      pred_hidden_dims=list(c.hidden), linkpred=False)
    else:
        model = GcnEncoderGraph(HC.F, c.H, c.E, c.C, c.L, pred_hidden_dims=list(c.hidden), concat=c.concat, bn=True,
                                args=types.SimpleNamespace(bias=True))
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=c.seed, bias_scale=0.1)
    for k in params:
        if k.startswith("assign_pred") and k.endswith(".weight"):
            params[k] = params[k] * HC.ASSIGN_SHARPEN
    model.load_state_dict(params)
    return model, params, x, adj, nn_, label


# ------------------------------------------------------------------ the layout, restated from dp_head.hip
def w_stride(din, padded):
    return din + 1 if (padded and din % 2 == 0 and din >= HEAD_PAD_MIN_DIN) else din


def fwd_lds_floats(dims, padded):
    return (sum(w_stride(a, padded) * b for a, b in zip(dims, dims[1:])) + sum(dims[1:]) + 2 * max(dims) + 512)


def layout(dims):
    """'padded' | 'dense' | 'generic' of a head the backward limit does not decide."""
    if fwd_lds_floats(dims, False) > HC.HEAD_FWD_LDS_FLOATS:
        return "generic"
    return "padded" if fwd_lds_floats(dims, True) <= HC.HEAD_FWD_LDS_FLOATS else "dense"


def test_the_table_holds_the_shapes_it_names():
    d = {c.name: HC.pred_dims(c) for c in CASES}
    w0 = {k: v[0] * v[1] for k, v in d.items()}
    nw = HEAD_FWD_THREADS // PIECE
    assert [w0[k] for k in ("s_w15_din5_3", "s_w63", "s_w64_pad", "s_w65", "s_w512_o64", "s_w544_o68")] == \
        [15, 63, 64, 65, nw * PIECE, nw * PIECE + 32]
    assert d["s_w15_din5_3"] == [5, 3, 2] and d["s_w512_o64"][1:] == [64, 2] and d["s_w520_o65"][1] == 65
    assert len(d["s_lin"]) == 2 and len(d["s_deep"]) == _lib.DP_MAX_PRED + 2
    assert w_stride(16, True) == 17 and w_stride(8, True) == 8 and w_stride(13, True) == 13 and w_stride(64, True) == 65
    assert [layout(d[k]) for k in ("s_pad_in", "s_pad_out", "s_lds_in", "s_lds_out")] == \
        ["padded", "dense", "dense", "generic"]
    assert fwd_lds_floats(d["s_pad_in"], True) == 30690 and fwd_lds_floats(d["s_pad_out"], True) == 30724
    assert fwd_lds_floats(d["s_lds_in"], False) == 30708 and fwd_lds_floats(d["s_lds_out"], False) == 30739
    for c in CASES:
        assert HC.planned(c) == (c.fwd, c.bwd), (c.name, HC.planned(c))
        if c.fam == "P":
            assert HC.readout_width(c) * c.P > 0          # featoff of the level the head reads out


# ------------------------------------------------------------------ the runs
def _run(model, c, xd, ad, nn_, ld):
    y, loss = HC.step(model, c, xd, ad, nn_, ld)
    torch.cuda.synchronize()
    return HC.results(model, c, y)


@functools.lru_cache(maxsize=None)
def _eager(name):
    """(first run, second run, device error word) of the training step in this process."""
    c = CASE[name]
    model, _, x, adj, nn_, label = _build(name)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    first = _run(model, c, xd, ad, nn_, ld)
    second = _run(model, c, xd, ad, nn_, ld)
    return first, second, _lib.load().dp_device_error(0)


def _differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("name", NAMES)
def test_the_head_alone_against_fp64_and_a_second_run(name):
    c = CASE[name]
    first, second, dev_err = _eager(name)
    _, params, _, _, _, label = _build(name)
    rows = HC.head_figures(c, params, label, first)
    for k, err, e_ref, bound, scale in rows:
        print(f"[hfwd] {name} ({layout(HC.pred_dims(c))}) {k}: error {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e} "
              f"error/bound {err / bound:.3f} max|ref| {scale:.3e}")
    loose = HC.loose_names(_build(name)[0], c)
    differ = [k for k in _differing(first, second) if k not in loose]
    print(f"[hfwd] {name}: second run, tensors with other bits {differ}; device error word {dev_err:#x}")
    assert torch.isfinite(first["ypred"]).all()
    bad = HC.failures(rows)
    assert not bad, f"{name}, the head alone against fp64: " + "; ".join(bad)
    assert not differ
    for k in loose:
        assert torch.allclose(first[k], second[k], rtol=1e-5, atol=1e-7), k
    assert dev_err == 0


@pytest.mark.parametrize("name", NAMES)
def test_three_replays_of_a_captured_step_carry_the_same_bits(name):
    c = CASE[name]
    model, _, x, adj, nn_, label = _build(name)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    nn_dev = torch.as_tensor(nn_, dtype=torch.int32).cuda()

    def fwd_bwd():
        y = HC.call(model, c, xd, ad, nn_dev)
        model.loss(y, ld).backward()
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        y = fwd_bwd()
    runs = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        runs.append({"ypred": y.detach().cpu().clone(),
                     **{"grad." + k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}})
    loose = HC.loose_names(model, c)
    differ = [[k for k in _differing(runs[0], r) if k not in loose] for r in runs[1:]]
    eager = _eager(name)[0]
    print(f"[hfwd] {name}: replays 2 and 3 against replay 1, tensors with other bits {differ}; ypred against the eager "
          f"run equal: {torch.equal(runs[0]['ypred'], eager['ypred'])}")
    assert differ == [[], []]
    assert torch.equal(runs[0]["ypred"], eager["ypred"])
    assert _lib.load().dp_device_error(0) == 0


@pytest.mark.parametrize("name", [c.name for c in CASES if c.fam == "P" and c.fwd == "fused"])
def test_stale_feature_columns_never_reach_the_logits(name):
    c = CASE[name]
    model, _, x, adj, nn_, _ = _build(name)
    model = model.cuda().eval()
    xd, ad = x.cuda(), adj.cuda()
    out = {}
    with torch.no_grad():
        HC.call(model, c, xd, ad, nn_)                    # the first evaluation forward makes the plan and its buffer
        plan, buf = model._last_save
        assert buf is plan.eval_save()
        words = buf[:buf.numel() // 4 * 4].view(torch.float32)
        for fill in (0.0, 1e30):
            words.fill_(fill)
            out[fill] = HC.call(model, c, xd, ad, nn_).cpu().clone()
    moved = int((out[0.0] != out[1e30]).sum())
    print(f"[hfwd] {name}: featoff {HC.readout_width(c) * c.P}, save buffer prefilled with 1e30 against 0: {moved} of "
          f"{out[0.0].numel()} logits moved, max |logit| {float(out[1e30].abs().max()):.3e}")
    assert torch.isfinite(out[1e30]).all() and moved == 0
    assert _lib.load().dp_device_error(0) == 0


def _head_fwd_launches(fn):
    """Launches of k_head_fwd while fn() runs, from the profiler's device events."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum("k_head_fwd" in n for n in names), len(names)


@pytest.mark.parametrize("name", NAMES)
def test_the_run_launches_the_head_the_table_expects(name):
    c = CASE[name]
    model, _, x, adj, nn_, label = _build(name)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    _run(model, c, xd, ad, nn_, ld)                              # warm up: the plan, lazy module loads
    heads, launches = _head_fwd_launches(lambda: HC.step(model, c, xd, ad, nn_, ld))
    print(f"[hfwd] {name}: table plan {c.fwd}, one step launches k_head_fwd x{heads} among {launches} kernels")
    assert launches > 0
    assert heads == int(c.fwd == "fused")


# ------------------------------------------------------------------ B: a Linear without bias
class _NoMidBias(GcnEncoderGraph):
    def _tail_params(self):
        return [p for p in super()._tail_params() if p is not None]


def test_a_linear_without_bias_between_two_with_one():
    Bn, N, H, E, L, hidden, Cn = 2, 6, 4, 5, 2, (16, 6), 3            # dims 9-16-6-3: the bias-less layer has padded rows
    x, adj, nn_, _ = O.make_batch(Bn, N, HC.F, n_min=3, p=0.3, seed=1, n_classes=Cn)
    model = _NoMidBias(HC.F, H, E, Cn, L, pred_hidden_dims=list(hidden), concat=True, bn=True)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1, bias_scale=0.1)
    model.load_state_dict(params)
    lins = model._pred_linears()
    assert len(lins) == 3
    lins[1].bias = None
    model = model.cuda().eval()
    xd, ad = x.cuda(), adj.cuda()
    nn_dev = torch.as_tensor(nn_, dtype=torch.int32).cuda()
    with torch.no_grad():
        y = model(xd, ad, nn_dev).cpu()
        y2 = model(xd, ad, nn_dev).cpu()
        z = model.saved_activation(0, "embedding").cpu().clone()
        win = model.saved_activation(0, "readout_argmax").cpu().clone()
        heads, _ = _head_fwd_launches(lambda: model(xd, ad, nn_dev))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(xd, ad, nn_dev)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yg = model(xd, ad, nn_dev)
        replays = []
        for _ in range(3):
            g.replay()
            torch.cuda.synchronize()
            replays.append(yg.cpu().clone())
    assert model._last_save[0].cfg.pred_b_off[1] == -1 and int(win.min()) >= 0

    def head(dtype):
        feat = torch.gather(z.to(dtype), 1, win.long().clamp(min=0).unsqueeze(1)).squeeze(1)
        for i, lin in enumerate(lins):
            feat = feat @ lin.weight.detach().cpu().to(dtype).t()
            if lin.bias is not None:
                feat = feat + lin.bias.detach().cpu().to(dtype)
            if i < len(lins) - 1:
                feat = torch.relu(feat)
        return feat

    ref = head(torch.float64)
    e_ref = float((head(torch.float32).double() - ref).abs().max())
    err = float((y.double() - ref).abs().max())
    bound = max(HC.FACTOR * e_ref, HC.FLOOR * float(ref.abs().max()))
    print(f"[hfwd] no-bias layer (dims {[z.shape[2]] + list(hidden) + [Cn]}): ypred error {err:.3e} e_ref {e_ref:.3e} "
          f"bound {bound:.3e} error/bound {err / bound:.3f}; second run equal: {torch.equal(y, y2)}; "
          f"k_head_fwd x{heads}; three replays equal to the eager run: {[torch.equal(r, y) for r in replays]}")
    assert err <= bound and torch.equal(y, y2)
    assert heads == 1
    assert all(torch.equal(r, y) for r in replays)
    assert _lib.load().dp_device_error(0) == 0
