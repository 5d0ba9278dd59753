"""dp_set2set_ragged_fwd / _bwd (csrc/dp_set2set_ragged.hip) on every row of tests/set2set_ragged_cases.py, anchored to
fp64: out, demb and the six parameter gradients against oracle.set2set_forward on the zero-padded [B, T, d] batch, within
set2set_cases.anchor_bound

    max|gpu - ref64| <= min(4 * max|oracle32 - ref64| + 3e-7 * max|ref64|, 1e-5 * max|ref64|).

Every run reads emb out of a wider buffer that starts one float off its allocation and holds NaN wherever no graph's row
is (in front of the first row, behind the last, in the columns beyond d), and writes demb into a wider NaN-filled
buffer: nothing but the d columns of the n_total rows may change, and no NaN may reach a result."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import ragged_base_cases as RC
from tests import set2set_cases as SC
from tests import set2set_ragged_cases as RS

pytestmark = pytest.mark.gpu

GUARD = 3          # NaN rows in front of node_off[0] and behind the last row


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def S():
    return torch.cuda.current_stream().cuda_stream


def poison(n):
    """n float32 on the GPU, every byte 0xFF (a NaN)."""
    return torch.full((max(4 * n, 4),), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)[:n]


def bits(t):
    return t.contiguous().view(torch.int32)


def run_ragged(lib, case, inputs, pad_e=5, pad_de=3, keep=True, backward=True):
    """One dp_set2set_ragged_fwd (+ _bwd) call.  emb lives in rows GUARD .. GUARD + n_total - 1 of a NaN-filled
    [n_total + 2 GUARD, d + pad_e] buffer that starts one float into its allocation; node_off starts at GUARD.  demb goes
    into a NaN-filled buffer of the same shape with d + pad_de columns; out [B, d] sits between two NaN guard rows.
    Returns ({tensor: GPU tensor}, demb buffer, out buffer)."""
    sizes, T, d, _ = case
    emb, params, gout = inputs
    B, n_total = len(sizes), sum(sizes)
    rows = n_total + 2 * GUARD
    lde, ldde = d + pad_e, d + pad_de
    ebuf = poison(rows * lde + 1)[1:].view(rows, lde)
    ebuf[GUARD:GUARD + n_total, :d] = emb.cuda()
    off_host = (np.concatenate([[0], np.cumsum(sizes)]) + GUARD).astype(np.int32)
    off = torch.from_numpy(off_host).cuda()
    P = [params[k].cuda().contiguous() for k in SC.PARAM_KEYS]
    obuf = poison((B + 2) * d).view(B + 2, d)
    out = obuf[1:B + 1]
    sb = lib.dp_set2set_ragged_save_bytes(off_host.ctypes.data, B, T, d)
    assert sb > 0
    save = poison(sb // 4 + 1) if keep else None
    _lib.check(lib.dp_set2set_ragged_fwd(ebuf.data_ptr(), lde, off.data_ptr(), off_host.ctypes.data, B, T, d,
                                         *[p.data_ptr() for p in P], out.data_ptr(), _lib.ptr(save), sb if keep else 0,
                                         S()), "dp_set2set_ragged_fwd")
    res, dbuf = {"out": out}, None
    if backward:
        go = gout.cuda().contiguous()
        dbuf = poison(rows * ldde + 1)[1:].view(rows, ldde)
        grads = [poison(p.numel()).view(p.shape) for p in P]
        wsb = lib.dp_set2set_ragged_bwd_workspace_bytes(off_host.ctypes.data, B, T, d)
        ws = poison(wsb // 4 + 1)
        _lib.check(lib.dp_set2set_ragged_bwd(ebuf.data_ptr(), lde, off.data_ptr(), off_host.ctypes.data, B, T, d,
                                             *[p.data_ptr() for p in P], out.data_ptr(), go.data_ptr(), dbuf.data_ptr(),
                                             ldde, *[g.data_ptr() for g in grads], save.data_ptr(), sb, ws.data_ptr(),
                                             wsb, S()), "dp_set2set_ragged_bwd")
        res["demb"] = dbuf[GUARD:GUARD + n_total, :d]
        res.update(dict(zip(SC.PARAM_KEYS, grads)))
    torch.cuda.synchronize()
    return res, dbuf, obuf


def check_anchored(got, r64, r32, what, tensors=SC.TENSORS):
    bad = []
    for k in tensors:
        g = got[k].detach().cpu().double()
        assert torch.isfinite(g).all(), f"{what} {k}: non-finite values"
        bound, e_o32, scale = RS.anchor_bound(r64[k], r32[k])
        e_gpu = float((g - r64[k]).abs().max())
        print(f"{what} {k}: |gpu-fp64| {e_gpu:.3e}  |oracle32-fp64| {e_o32:.3e}  bound {bound:.3e}  scale {scale:.3e}")
        if e_gpu > bound:
            bad.append(f"{k}: |gpu-fp64| {e_gpu:.3e} > bound {bound:.3e} (|oracle32-fp64| {e_o32:.3e}, "
                       f"largest entry {scale:.3e})")
    assert not bad, f"{what}: " + "; ".join(bad)


def variants_of(lib, case):
    return "/".join(sorted({RS.VARIANTS[lib.dp_set2set_ragged_plan(n, case[2])] for n in case[0]}))


# ------------------------------------------------------------------ every row against fp64, guards untouched
@pytest.mark.parametrize("case", RS.CASES, ids=RS.case_id)
def test_case_against_fp64(lib, case):
    sizes, T, d, _ = case
    inputs, r64, r32 = RS.case_references(case)
    got, dbuf, obuf = run_ragged(lib, case, inputs)
    check_anchored(got, r64, r32, f"{RS.case_id(case)} [{variants_of(lib, case)}]")
    n_total = sum(sizes)
    assert bool((bits(obuf[0]) == -1).all()) and bool((bits(obuf[-1]) == -1).all()), "wrote outside out [B, d]"
    assert bool((bits(dbuf[:GUARD]) == -1).all()) and bool((bits(dbuf[GUARD + n_total:]) == -1).all()), \
        "dp_set2set_ragged_bwd wrote demb rows of no graph"
    assert bool((bits(dbuf[:, d:]) == -1).all()), "dp_set2set_ragged_bwd wrote beyond column d of demb"


# rows that take both grids (either side of the LDS edge), the multi-row threads, padding, and the widest d
REPEATED = [c for c in RS.CASES if c[2] in (64, 256) or max(c[0]) > 1024 or c[:2] == ((1, 9, 14), 20)]


@pytest.mark.parametrize("case", REPEATED, ids=RS.case_id)
def test_bit_reproducible_and_stride_independent(lib, case):
    """Two runs agree bit for bit; dense row strides (lde = ldde = d) give the same bits as the wide buffers; and the
    inference call (save = NULL) gives the saving run's `out` bit for bit."""
    inputs, _, _ = RS.case_references(case)
    first, _, _ = run_ragged(lib, case, inputs)
    second, _, _ = run_ragged(lib, case, inputs)
    tight, _, _ = run_ragged(lib, case, inputs, pad_e=0, pad_de=0)
    for k in SC.TENSORS:
        assert torch.equal(bits(first[k]), bits(second[k])), f"{k} differs between two runs on the same inputs"
        assert torch.equal(bits(first[k]), bits(tight[k])), f"{k} differs between wide and dense row strides"
    infer, _, _ = run_ragged(lib, case, inputs, keep=False, backward=False)
    assert torch.equal(bits(first["out"]), bits(infer["out"])), "inference (save = NULL) differs from the saving run"


# ------------------------------------------------------------------ against the dense entries
DENSE_ROWS = [c for c in RS.CASES if c[1] <= 1024]


@pytest.mark.parametrize("case", DENSE_ROWS, ids=RS.case_id)
def test_against_the_dense_entries(lib, case):
    """dp_set2set_fwd / _bwd on the zero-padded [B, T, d] batch sit within anchor_bound of fp64 too, and the two paths
    disagree by no more than the sum of their bounds."""
    sizes, T, d, _ = case
    (emb, params, gout), r64, r32 = RS.case_references(case)
    B = len(sizes)
    dense_emb = RC.pad_rows(emb, sizes, T).cuda().contiguous()
    P = [params[k].cuda().contiguous() for k in SC.PARAM_KEYS]
    out = torch.empty(B, d, device="cuda")
    sb = lib.dp_set2set_save_bytes(B, T, d)
    save = torch.empty(sb, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dp_set2set_fwd(dense_emb.data_ptr(), d, *[p.data_ptr() for p in P], out.data_ptr(), B, T, d,
                                  save.data_ptr(), sb, S()), "dp_set2set_fwd")
    demb = torch.empty_like(dense_emb)
    grads = [torch.empty_like(p) for p in P]
    wsb = lib.dp_set2set_bwd_workspace_bytes(B, T, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    go = gout.cuda().contiguous()
    _lib.check(lib.dp_set2set_bwd(dense_emb.data_ptr(), d, *[p.data_ptr() for p in P], out.data_ptr(), go.data_ptr(),
                                  demb.data_ptr(), d, *[g.data_ptr() for g in grads], B, T, d, save.data_ptr(), sb,
                                  ws.data_ptr(), wsb, S()), "dp_set2set_bwd")
    torch.cuda.synchronize()
    dense = {"out": out, "demb": RC.unpad(demb.cpu(), sizes)}
    dense.update(dict(zip(SC.PARAM_KEYS, grads)))
    check_anchored(dense, r64, r32, f"{RS.case_id(case)} [dense]")
    ragged, _, _ = run_ragged(lib, case, (emb, params, gout))
    check_anchored(ragged, r64, r32, f"{RS.case_id(case)} [ragged]")
    for k in SC.TENSORS:
        bound, _, _ = RS.anchor_bound(r64[k], r32[k])
        diff = float((ragged[k].cpu().double() - dense[k].cpu().double()).abs().max())
        assert diff <= 2 * bound, f"{k}: ragged and dense entries differ by {diff:.3e} > {2 * bound:.3e}"


# ------------------------------------------------------------------ DD's largest graph, forward only
def test_forward_at_5748_rows(lib):
    """{5748, 40} at T = 5748 (DD's largest graph, past the dense kernels' 1024 rows), d = 8 (its embedding does not fit
    LDS), inference call.  The float64 reference is the oracle on the padded batch under no_grad."""
    from oracle import diffpool_oracle as O
    case = ((5748, 40), 5748, 8, "")
    emb, params, gout = RS.make_inputs(*case)
    assert lib.dp_set2set_ragged_plan(5748, 8) == RS.W_REGS and lib.dp_set2set_ragged_plan(40, 8) & RS.E_LDS
    with torch.no_grad():
        r = {}
        for dt in (torch.float64, torch.float32):
            out = O.set2set_forward(RC.pad_rows(emb.to(dt), case[0], case[1]), {k: v.to(dt) for k, v in params.items()})
            r[dt] = {"out": out.double()}
    got, _, _ = run_ragged(lib, case, (emb, params, gout), keep=False, backward=False)
    check_anchored(got, r[torch.float64], r[torch.float32], "n5748_40-T5748-d8", tensors=("out",))
    assert float((r[torch.float64]["out"] > 0).double().mean()) >= 0.25


# ------------------------------------------------------------------ refusals with a GPU present
def test_refusals_launch_nothing(lib):
    """T < max n_b, d = 0, d = 257, a graph above the stated bound and a save buffer too small: the right code, and
    neither `out` nor any gradient buffer is touched."""
    d = 8
    emb = torch.zeros(64, d, device="cuda")
    par = [torch.zeros(n, device="cuda") for n in (8 * 257 * 257, 4 * 257 * 257, 4 * 257, 4 * 257, 2 * 257 * 257, 257)]
    out, demb = poison(4 * 257).view(4, 257), poison(64 * 257)
    grads = [poison(p.numel()) for p in par]
    big = poison(1 << 16)

    def both(sizes, T, d_, save_bytes=None):
        off_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        off = torch.from_numpy(off_host).cuda()
        B = len(sizes)
        sb = big.numel() * 4 if save_bytes is None else save_bytes
        lde = max(d_, 1)
        rf = lib.dp_set2set_ragged_fwd(emb.data_ptr(), lde, off.data_ptr(), off_host.ctypes.data, B, T, d_,
                                       *[p.data_ptr() for p in par], out.data_ptr(), big.data_ptr(), sb, S())
        rb = lib.dp_set2set_ragged_bwd(emb.data_ptr(), lde, off.data_ptr(), off_host.ctypes.data, B, T, d_,
                                       *[p.data_ptr() for p in par], out.data_ptr(), out.data_ptr(), demb.data_ptr(),
                                       lde, *[g.data_ptr() for g in grads], big.data_ptr(), sb, big.data_ptr(),
                                       big.numel() * 4, S())
        return rf, rb

    assert both([10, 20], 19, d) == (RS.ERR_INVALID, RS.ERR_INVALID)
    assert both([10, 20], 20, 0) == (RS.ERR_INVALID, RS.ERR_INVALID)
    assert both([10, 20], 20, 257) == (RS.ERR_UNSUPPORTED, RS.ERR_UNSUPPORTED)
    assert both([5, RS.MAX_ROWS + 1], RS.MAX_ROWS + 1, d) == (RS.ERR_UNSUPPORTED, RS.ERR_UNSUPPORTED)
    assert both([10, 20], 20, d, save_bytes=512) == (RS.ERR_INVALID, RS.ERR_INVALID)
    torch.cuda.synchronize()
    for t in [out, demb, big] + grads:
        assert bool((bits(t) == -1).all()), "a refused call wrote to one of its buffers"


def test_empty_batch(lib):
    """B = 0 as the dense entries: DP_OK, the forward writes nothing, the backward zero-fills the six parameter
    gradients (sums over no graph) and leaves demb alone."""
    d = 8
    off_host = np.zeros(1, dtype=np.int32)
    off = torch.from_numpy(off_host).cuda()
    emb = torch.zeros(4, d, device="cuda")
    P = [torch.zeros(s, device="cuda") for s in ((4 * d, 2 * d), (4 * d, d), (4 * d,), (4 * d,), (d, 2 * d), (d,))]
    out, demb = poison(d), poison(4 * d)
    grads = [poison(p.numel()).view(p.shape) for p in P]
    sb = lib.dp_set2set_ragged_save_bytes(off_host.ctypes.data, 0, 5, d)
    wsb = lib.dp_set2set_ragged_bwd_workspace_bytes(off_host.ctypes.data, 0, 5, d)
    assert sb > 0 and wsb > 0
    save, ws = poison(sb // 4 + 1), poison(wsb // 4 + 1)
    _lib.check(lib.dp_set2set_ragged_fwd(emb.data_ptr(), d, off.data_ptr(), off_host.ctypes.data, 0, 5, d,
                                         *[p.data_ptr() for p in P], out.data_ptr(), save.data_ptr(), sb, S()),
               "dp_set2set_ragged_fwd")
    _lib.check(lib.dp_set2set_ragged_bwd(emb.data_ptr(), d, off.data_ptr(), off_host.ctypes.data, 0, 5, d,
                                         *[p.data_ptr() for p in P], out.data_ptr(), out.data_ptr(), demb.data_ptr(), d,
                                         *[g.data_ptr() for g in grads], save.data_ptr(), sb, ws.data_ptr(), wsb, S()),
               "dp_set2set_ragged_bwd")
    torch.cuda.synchronize()
    assert bool((bits(out) == -1).all()) and bool((bits(demb) == -1).all())
    for g in grads:
        assert bool((g == 0).all())
