"""k_set2set_fwd / k_set2set_bwd (dp_set2set.hip) at every launch variant, anchored to fp64.

The launchers pick one of five kernel variants from (n, d) alone (dp_set2set_plan); the table in tests/set2set_cases.py
reaches all of them and the edges of their loops (tests/test_set2set_plan_cpu.py asserts that).  Every case calls
dp_set2set_fwd / dp_set2set_bwd directly through ctypes and holds the output, the embedding gradient and the six
parameter gradients to

    max|gpu - ref64| <= 4 * max|oracle32 - ref64| + 3e-7 * max|ref64|,   and never more than 1e-5 * max|ref64|

where ref64 / oracle32 are oracle.diffpool_oracle.set2set_forward on the CPU in float64 / float32: the yardstick is the
fp32 oracle's own distance from fp64, never the kernel's output.  A single attention row dropped moves the output by
2.4e-3 of its largest entry at n = 1024 (test_set2set_plan_cpu.py), 240 x the widest bound granted here.

The save buffer, the backward workspace and every output are filled with 0xFF bytes (NaN) before each call: nothing
may depend on what they held.  DP_S2S_ANCHOR_OUT=<file> appends one line per case with the eight ratios
max|gpu - ref64| / max|oracle32 - ref64| (profiles/set2set_fp64_anchor.txt is such a file)."""
import os

import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import GcnSet2SetEncoder
from graph_pooling_amd.set2set import Set2Set
from oracle import diffpool_oracle as O
from tests import set2set_cases as SC
from tests.parity import close, grads_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def S():
    return torch.cuda.current_stream().cuda_stream


def poison(*shape):
    """float32 tensor of `shape` on the GPU, every byte 0xFF (a NaN)."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((max(4 * n, 4),), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)[:n].view(*shape)


def poison_bytes(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


def run_gpu(lib, emb, params, gout, pad_e=0, pad_de=0):
    """One dp_set2set_fwd + dp_set2set_bwd pair.  emb is read as a view of a [B, n, d + pad_e] buffer and demb written
    into a [B, n, d + pad_de] buffer; the extra columns hold NaN.  Returns ({tensor name: GPU tensor}, demb buffer)."""
    B, n, d = emb.shape
    ebuf = poison(B, n, d + pad_e)
    ebuf[:, :, :d] = emb.cuda()
    P = [params[k].cuda().contiguous() for k in SC.PARAM_KEYS]
    go = gout.cuda().contiguous()
    out = poison(B, d)
    sb = lib.dp_set2set_save_bytes(B, n, d)
    save = poison_bytes(sb)
    _lib.check(lib.dp_set2set_fwd(ebuf.data_ptr(), d + pad_e, *[p.data_ptr() for p in P], out.data_ptr(), B, n, d,
                                  save.data_ptr(), sb, S()), "dp_set2set_fwd")
    dbuf = poison(B, n, d + pad_de)
    grads = [poison(*p.shape) for p in P]
    wsb = lib.dp_set2set_bwd_workspace_bytes(B, n, d)
    ws = poison_bytes(wsb)
    _lib.check(lib.dp_set2set_bwd(ebuf.data_ptr(), d + pad_e, *[p.data_ptr() for p in P], out.data_ptr(),
                                  go.data_ptr(), dbuf.data_ptr(), d + pad_de, *[g.data_ptr() for g in grads], B, n, d,
                                  save.data_ptr(), sb, ws.data_ptr(), wsb, S()), "dp_set2set_bwd")
    torch.cuda.synchronize()
    res = {"out": out, "demb": dbuf[:, :, :d]}
    res.update(dict(zip(SC.PARAM_KEYS, grads)))
    return res, dbuf


def check_anchored(got, r64, r32, what):
    """The fp64-anchored bound on every tensor; returns the ratios max|gpu - ref64| / max|oracle32 - ref64|."""
    ratios, bad = [], []
    for k in SC.TENSORS:
        g = got[k].detach().cpu().double()
        assert torch.isfinite(g).all(), f"{what} {k}: non-finite values"
        bound, e_o32, scale = SC.anchor_bound(r64[k], r32[k])
        e_gpu = float((g - r64[k]).abs().max())
        ratios.append(e_gpu / e_o32 if e_o32 > 0 else float("inf") if e_gpu > 0 else 0.0)
        print(f"{what} {k}: |gpu-fp64| {e_gpu:.3e}  |oracle32-fp64| {e_o32:.3e}  bound {bound:.3e}  scale {scale:.3e}")
        if e_gpu > bound:
            bad.append(f"{k}: |gpu-fp64| {e_gpu:.3e} > bound {bound:.3e} (|oracle32-fp64| {e_o32:.3e}, "
                       f"largest entry {scale:.3e})")
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratios


# ------------------------------------------------------------------ every case against fp64
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_case_against_fp64(lib, case):
    B, n, d = case
    variant = SC.VARIANTS[lib.dp_set2set_plan(n, d)]
    (emb, params, gout), r64, r32 = SC.case_references(case)
    got, _ = run_gpu(lib, emb, params, gout)
    ratios = None
    try:
        ratios = check_anchored(got, r64, r32, f"{SC.case_id(case)} [{variant}]")
    finally:
        path = os.environ.get("DP_S2S_ANCHOR_OUT")
        if path:
            with open(path, "a") as f:
                f.write(f"{SC.case_id(case):16s} {variant:6s} " +
                        (" ".join(f"{r:7.3f}" for r in ratios) if ratios else "OVER THE BOUND (see the test output)") +
                        "\n")


# one case per variant, each with rows >= 256 where the table has them (the backward's in-place tail)
PER_VARIANT = [(2, 257, 60), (2, 600, 64), (2, 40, 65), (2, 300, 66), (2, 300, 130)]


def test_per_variant_cases_cover_the_five_variants(lib):
    assert all(c in SC.CASES for c in PER_VARIANT)
    assert {lib.dp_set2set_plan(n, d) for _, n, d in PER_VARIANT} == set(SC.VARIANTS)


# ------------------------------------------------------------------ strides
@pytest.mark.parametrize("case", PER_VARIANT, ids=SC.case_id)
def test_row_strides(lib, case):
    """lde = d + 5 and ldde = d + 3 (the C ABI offers both; the Python module always passes d): bit-identical results,
    and the columns of demb's buffer beyond d keep their bytes."""
    B, n, d = case
    (emb, params, gout), _, _ = SC.case_references(case)
    dense, _ = run_gpu(lib, emb, params, gout)
    strided, dbuf = run_gpu(lib, emb, params, gout, pad_e=5, pad_de=3)
    for k in SC.TENSORS:
        assert torch.equal(bits(dense[k]), bits(strided[k])), f"{k} differs between dense and padded row strides"
    assert dbuf.shape == (B, n, d + 3)
    assert bool((bits(dbuf[:, :, d:]) == -1).all()), "dp_set2set_bwd wrote beyond column d of demb"


# ------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("case", PER_VARIANT, ids=SC.case_id)
def test_bit_reproducible_run_to_run(lib, case):
    (emb, params, gout), _, _ = SC.case_references(case)
    first, _ = run_gpu(lib, emb, params, gout)
    second, _ = run_gpu(lib, emb, params, gout)
    for k in SC.TENSORS:
        assert torch.equal(first[k], second[k]), f"{k} differs between two runs on the same inputs"


# ------------------------------------------------------------------ module and encoder level
def test_module_d90_through_autograd():
    """Set2Set(90, 180) (GcnSet2SetEncoder at --hidden-dim 30 --output-dim 30: weights read from global memory, two
    gate chunks) with torch's own initialisation, through autograd."""
    B, n, d = 3, 120, 90
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(90)
        m = Set2Set(d, 2 * d)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert set(params) == set(SC.PARAM_KEYS)
    g = torch.Generator().manual_seed(91)
    emb = 0.3 * torch.randn(B, n, d, generator=g)
    emb[0, 80:] = 0.0
    gout = torch.randn(B, d, generator=g)
    assert _lib.load().dp_set2set_plan(n, d) == 0
    m = m.cuda()
    e_d = emb.cuda().requires_grad_(True)
    out = m(e_d)
    (out * gout.cuda()).sum().backward()
    got = {"out": out, "demb": e_d.grad}
    got.update({k: p.grad for k, p in m.named_parameters()})
    r64, r32 = SC.reference(emb, params, gout, torch.float64), SC.reference(emb, params, gout, torch.float32)
    check_anchored(got, r64, r32, "Set2Set(90, 180) n=120")


def test_encoder_d90_against_oracle():
    """One GcnSet2SetEncoder(F, 30, 30, C, 3) step: the readout is Set2Set at d = 90 over N = 120 rows with padded
    nodes, against O.set2set_encoder_forward, tolerances of test_set2set_encoder_against_reference_golden."""
    B, N, F_, Cc = 4, 120, 5, 4
    x, adj, nn_, label = O.make_batch(B, N, F_, n_min=30, n_max=110, p=0.08, seed=12, n_classes=Cc)
    assert max(nn_) < N
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(13)
        model = GcnSet2SetEncoder(F_, 30, 30, Cc, 3)
    sd = model.state_dict()
    params = O.init_params({k: tuple(v.shape) for k, v in sd.items() if not k.startswith("s2s.lstm")}, seed=14,
                           bias_scale=0.1)
    params.update({k: v.detach().clone() for k, v in sd.items() if k.startswith("s2s.lstm")})
    assert params["s2s.pred.weight"].shape == (90, 180)
    model.load_state_dict(params)
    model = model.cuda()
    ypred = model(x.cuda(), adj.cuda(), nn_)
    loss = model.loss(ypred, label.cuda())
    loss.backward()
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo = O.set2set_encoder_forward(P, x, adj, nn_)
    lo, _ = O.softpool_loss(yo, label)
    lo.backward()
    close(ypred, yo)
    close(loss, lo, 1e-5, 1e-6)
    grads_close(model, {k: v.grad for k, v in P.items()})


# ------------------------------------------------------------------ refusals and empty shapes
def _call_pair(lib, B, n, d, alloc_n=None):
    """dp_set2set_fwd then dp_set2set_bwd on NaN-filled outputs sized for max(B, 1) graphs of `alloc_n` rows.  Returns
    (rc_fwd, msg_fwd, rc_bwd, msg_bwd, out, demb, grads)."""
    Ba, na = max(B, 1), max(alloc_n or n, 1)
    emb = torch.zeros(Ba, na, d, device="cuda")
    shapes = ((4 * d, 2 * d), (4 * d, d), (4 * d,), (4 * d,), (d, 2 * d), (d,))
    P = [torch.zeros(s, device="cuda") for s in shapes]
    out, demb, grads = poison(Ba, d), poison(Ba, na, d), [poison(*s) for s in shapes]
    go = torch.zeros(Ba, d, device="cuda")
    sb = max(lib.dp_set2set_save_bytes(Ba, na, d), lib.dp_set2set_save_bytes(B, n, d))
    save = poison_bytes(sb)
    rc_f = lib.dp_set2set_fwd(emb.data_ptr(), d, *[p.data_ptr() for p in P], out.data_ptr(), B, n, d,
                              save.data_ptr(), sb, S())
    msg_f = lib.dp_last_error_string()
    wsb = max(lib.dp_set2set_bwd_workspace_bytes(Ba, na, d), lib.dp_set2set_bwd_workspace_bytes(B, n, d))
    ws = poison_bytes(wsb)
    rc_b = lib.dp_set2set_bwd(emb.data_ptr(), d, *[p.data_ptr() for p in P], out.data_ptr(), go.data_ptr(),
                              demb.data_ptr(), d, *[g.data_ptr() for g in grads], B, n, d, save.data_ptr(), sb,
                              ws.data_ptr(), wsb, S())
    msg_b = lib.dp_last_error_string()
    torch.cuda.synchronize()
    return rc_f, msg_f, rc_b, msg_b, out, demb, grads


def _untouched(*tensors):
    return all(bool((bits(t) == -1).all()) for t in tensors)


@pytest.mark.parametrize("n,d", SC.REFUSED)
def test_shapes_outside_the_limits_are_refused(lib, n, d):
    assert lib.dp_set2set_plan(n, d) == SC.ERR_UNSUPPORTED
    rc_f, msg_f, rc_b, msg_b, out, demb, grads = _call_pair(lib, 2, n, d)
    for rc, msg in ((rc_f, msg_f), (rc_b, msg_b)):
        assert rc == SC.ERR_UNSUPPORTED
        assert b"n <= 1024" in msg and b"d <= 256" in msg and (f"n={n}".encode() in msg), msg
    assert _untouched(out, demb, *grads)


def test_empty_batch_is_ok_without_a_launch(lib):
    """B = 0 (decided on the host: dim3(0) is not a valid grid): DP_OK; the forward writes nothing; the backward
    zero-fills the parameter gradients, which are sums over no graph, and writes no demb."""
    rc_f, _, rc_b, _, out, demb, grads = _call_pair(lib, 0, 50, 70)
    assert rc_f == 0 and rc_b == 0
    assert _untouched(out, demb)
    assert all(bool((g == 0).all()) for g in grads)


def test_zero_rows_are_refused(lib):
    """n = 0 (the oracle's answer would be relu(bp)): refused as an invalid argument before any launch, like every
    other entry of the library refuses an empty extent."""
    rc_f, msg_f, rc_b, msg_b, out, demb, grads = _call_pair(lib, 2, 0, 70)
    assert rc_f == -1 and b"n=0 must be positive" in msg_f
    assert rc_b == -1 and b"n=0 must be positive" in msg_b
    assert _untouched(out, demb, *grads)
    assert lib.dp_set2set_plan(0, 70) == SC.ERR_UNSUPPORTED
