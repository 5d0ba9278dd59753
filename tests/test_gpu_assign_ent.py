"""dp_assign_entropy_fwd / _bwd through the C entries, against the fp64 reference and the derived bound of
tests/assign_ent_cases.py, with guard bands around ent_out, total_inout and dS: every width tier and load form (K in
one visit of 4 / 16 / 64 lanes, the strided loop above), tight and padded leading dimensions, buffers one float off
their allocation, every mask, the grid-stride wrap and the 2^20-row CSR form."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from tests import assign_ent_cases as AC

pytestmark = pytest.mark.gpu

GUARD = -7.25
FRONT, TAIL = 4, 8           # floats; FRONT keeps an offset of 0 on a 16-byte boundary
WEIGHT, DLOSS, OLD_TOTAL = float(np.float32(0.3)), 1.75, 2.5      # the weight as the fp32 the entry receives


class Buf:
    """[rows, K] at leading dimension ld inside a guarded flat device allocation, `off` floats past FRONT."""

    def __init__(self, rows, K, ld, off, data=None, fill=GUARD):
        self.rows, self.K, self.ld, self.start = rows, K, ld, FRONT + off
        host = torch.full((self.start + rows * ld + TAIL,), fill, dtype=torch.float32)
        if data is not None:
            self.view(host).copy_(torch.as_tensor(data).reshape(rows, K))
        self.host0 = host.clone()
        self.dev = host.cuda()

    def view(self, t):
        return t.as_strided((self.rows, self.K), (self.ld, 1), self.start)

    def ptr(self):
        return self.dev.data_ptr() + 4 * self.start

    def back(self):
        """(values [rows, K] float64 numpy, flat host copy)."""
        h = self.dev.cpu()
        return self.view(h).double().numpy(), h

    def outside_untouched(self, h):
        """Everything that is not an entry of the view holds its initial bits."""
        a, b = h.clone(), self.host0.clone()
        self.view(a).zero_()
        self.view(b).zero_()
        return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Scalars:
    """ent_out and total_inout, each with guards on both sides: [G, ent, G, G, total, G]."""

    def __init__(self):
        self.dev = torch.tensor([GUARD, GUARD, GUARD, GUARD, OLD_TOTAL, GUARD], dtype=torch.float32).cuda()

    def ent_ptr(self):
        return self.dev.data_ptr() + 4

    def total_ptr(self):
        return self.dev.data_ptr() + 16

    def back(self):
        return self.dev.cpu()


def _fwd(lib, sb, nn_dev, B, n, K, sc, with_total, ws):
    _lib.check(lib.dp_assign_entropy_fwd(sb.ptr(), sb.ld, _lib.ptr(nn_dev), WEIGHT, sc.ent_ptr(),
                                         sc.total_ptr() if with_total else None, B, n, K, ws.data_ptr(), ws.numel(),
                                         _lib.current_stream()), "dp_assign_entropy_fwd")


def _make_S(B, n, K, seed):
    rng = np.random.default_rng(seed)
    return AC.special_rows(AC.softmax_rows(rng, B, n, K), rng)


def _masked_fill(S, nn, B, n, value):
    """S with the rows past n_b replaced: valid uniform rows (a leak would move E) or NaN (a leak would poison it)."""
    v = AC.valid_rows(nn, B, n)
    out = S.copy()
    out[~v] = value
    return out


def _check_case(B, n, K, ld_pad, off, mask, seed):
    """Runs every check of one layout; returns the largest |error| / bound of the forward and of the backward with
    accumulate = 0 and = 1 (tools/assign_ent_probe.py records them)."""
    lib = _lib.load()
    worst_f, worst_b = 0.0, [0.0, 0.0]
    rows, ld = B * n, K + ld_pad
    S = _make_S(B, n, K, seed)
    nn = AC.num_nodes(mask, B, n)
    nn_dev = None if nn is None else torch.from_numpy(nn).cuda()
    e_ref, mag = AC.entropy_ref(S, nn)
    bound = AC.fwd_bound(mag)
    ws = torch.empty(lib.dp_assign_entropy_workspace_bytes(B, n, K), dtype=torch.uint8, device="cuda")
    tag = f"B={B} n={n} K={K} ld={ld} off={off} mask={mask}"

    # ---- forward: masked rows hold valid rows in one run, NaN in the other; with and without total_inout
    got = []
    for fill, with_total in ((1.0 / K, True), (float("nan"), False)):
        sb = Buf(rows, K, ld, off, data=_masked_fill(S, nn, B, n, fill))
        sc = Scalars()
        _fwd(lib, sb, nn_dev, B, n, K, sc, with_total, ws)
        h = sc.back()
        e = float(h[1])
        assert np.isfinite(e), tag
        worst_f = max(worst_f, abs(e - e_ref) / bound)
        assert abs(e - e_ref) <= bound, (tag, e, e_ref, bound, abs(e - e_ref) / bound)
        assert h[0] == GUARD and h[2] == GUARD and h[3] == GUARD and h[5] == GUARD, (tag, h)
        if with_total:      # exactly old + fl(weight * E) in fp32
            want = np.float32(OLD_TOTAL) + np.float32(WEIGHT) * h[1].numpy()
            assert h[4].numpy().tobytes() == np.float32(want).tobytes(), (tag, h)
        else:
            assert float(h[4]) == OLD_TOTAL, (tag, h)
        assert torch.equal(sb.dev.cpu().view(torch.int32), sb.host0.view(torch.int32)), tag     # S is read only
        got.append(h[1].numpy().tobytes())
    assert got[0] == got[1], tag                 # what the masked rows hold changes nothing, bit for bit

    # ---- backward
    sb = Buf(rows, K, ld, off, data=_masked_fill(S, nn, B, n, float("nan")))
    g_dev = torch.tensor([DLOSS], dtype=torch.float32).cuda()
    rng = np.random.default_rng(seed + 1)
    old = rng.standard_normal((rows, K)).astype(np.float32)
    v = np.repeat(AC.valid_rows(nn, B, n).reshape(rows, 1), K, axis=1)
    for acc in (0, 1):
        for dl in (None, g_dev):
            g = 1.0 if dl is None else DLOSS
            d_ref, d_bound = AC.grad_ref(S, nn, g, WEIGHT)
            d_ref, d_bound = d_ref.reshape(rows, K), d_bound.reshape(rows, K)
            # tight: S and dS share the layout (16-byte lanes where K allows); padded: ldds differs from lds
            db = Buf(rows, K, ld if ld_pad in (0, 4) else ld + 1, off, data=old)
            _lib.check(lib.dp_assign_entropy_bwd(sb.ptr(), sb.ld, _lib.ptr(nn_dev), _lib.ptr(dl), WEIGHT, db.ptr(),
                                                 db.ld, acc, B, n, K, _lib.current_stream()), "dp_assign_entropy_bwd")
            out, h = db.back()
            assert db.outside_untouched(h), (tag, acc)               # guards and the columns K..ldds-1
            if acc:
                want = old.astype(np.float64) + d_ref
                tol = d_bound + AC.U * np.abs(want)                  # fl(old + d): one more rounding
                assert np.array_equal(db.view(h).numpy()[~v].view(np.int32), old[~v].view(np.int32)), (tag, "masked")
            else:
                want, tol = d_ref, d_bound
                assert (out[~v] == 0).all(), (tag, "masked rows must be exactly 0")
            assert np.isfinite(out).all(), (tag, acc)
            err = np.abs(out - want)
            if v.any():
                worst_b[acc] = max(worst_b[acc], float((err[v] / tol[v]).max()))
            assert (err <= tol).all(), (tag, acc, g, worst_b)
    return worst_f, worst_b[0], worst_b[1]


SMALL_IDS = [f"B{B}-n{n}-K{K}" for B, n, K in AC.SMALL]


@pytest.mark.parametrize("shape", AC.SMALL, ids=SMALL_IDS)
def test_every_width_tier_mask_layout_and_alignment(shape):
    B, n, K = shape
    seed = B * 100003 + n * 1009 + K
    for ld_pad in (0, 3):
        for off in (0, 1):
            for mask in AC.MASKS:
                _check_case(B, n, K, ld_pad, off, mask, seed)
    _check_case(B, n, K, 4, 0, "mix", seed)      # 16-byte lanes with padding columns behind the row (K % 4 == 0)


@pytest.mark.parametrize("shape", AC.LOOP + AC.WRAP, ids=lambda s: "x".join(map(str, s)))
def test_strided_loop_and_grid_stride_wrap(shape):
    B, n, K = shape
    for ld_pad, off, mask in ((0, 0, "mix"), (3, 1, "null"), (0, 1, "full")):
        _check_case(B, n, K, ld_pad, off, mask, seed=K * 7 + n)


def test_csr_form_of_a_million_rows():
    """(1, 2^20, 8), no mask: the row count of a large ragged batch; eight sweeps of the grid-stride loop."""
    (B, n, K), = AC.CSR
    lib = _lib.load()
    S = AC.softmax_rows(np.random.default_rng(5), B, n, K)
    e_ref, mag = AC.entropy_ref(S)
    Sd = torch.from_numpy(S).cuda()
    ws = torch.empty(lib.dp_assign_entropy_workspace_bytes(B, n, K), dtype=torch.uint8, device="cuda")
    sc = Scalars()
    _lib.check(lib.dp_assign_entropy_fwd(Sd.data_ptr(), K, None, WEIGHT, sc.ent_ptr(), None, B, n, K, ws.data_ptr(),
                                         ws.numel(), _lib.current_stream()), "dp_assign_entropy_fwd")
    e = float(sc.back()[1])
    assert abs(e - e_ref) <= AC.fwd_bound(mag), (e, e_ref, AC.fwd_bound(mag))
    dS = torch.full((n * K + TAIL,), GUARD, dtype=torch.float32, device="cuda")
    _lib.check(lib.dp_assign_entropy_bwd(Sd.data_ptr(), K, None, None, WEIGHT, dS.data_ptr(), K, 0, B, n, K,
                                         _lib.current_stream()), "dp_assign_entropy_bwd")
    d_ref, d_bound = AC.grad_ref(S, None, 1.0, WEIGHT)
    h = dS.cpu()
    assert (h[n * K:] == GUARD).all()
    err = np.abs(h[:n * K].double().numpy().reshape(B, n, K) - d_ref)
    assert (err <= d_bound).all(), float((err / d_bound).max())


def test_forward_is_bit_identical_from_run_to_run_and_under_graph_capture():
    lib = _lib.load()
    B, n, K = 3, 2731, 65                      # 8193 rows: every workgroup of the grid, one row into the second sweep
    S = _make_S(B, n, K, 11)
    nn = AC.num_nodes("mix", B, n)
    nn_dev = torch.from_numpy(nn).cuda()
    Sd = torch.from_numpy(S).cuda()
    ws = torch.empty(lib.dp_assign_entropy_workspace_bytes(B, n, K), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    dS = torch.zeros(B, n, K, dtype=torch.float32, device="cuda")

    def run():
        _lib.check(lib.dp_assign_entropy_fwd(Sd.data_ptr(), K, nn_dev.data_ptr(), WEIGHT, out.data_ptr(), None, B, n, K,
                                             ws.data_ptr(), ws.numel(), _lib.current_stream()), "dp_assign_entropy_fwd")
        _lib.check(lib.dp_assign_entropy_bwd(Sd.data_ptr(), K, nn_dev.data_ptr(), None, WEIGHT, dS.data_ptr(), K, 0, B,
                                             n, K, _lib.current_stream()), "dp_assign_entropy_bwd")

    run()
    first, d_first = out.cpu().clone(), dS.cpu().clone()
    e_ref, mag = AC.entropy_ref(S, nn)
    assert abs(float(first[0]) - e_ref) <= AC.fwd_bound(mag)
    for _ in range(2):
        out.zero_()
        ws.random_(0, 255)                     # what an earlier call left in the workspace is never read
        run()
        assert torch.equal(out.cpu().view(torch.int32), first.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.zero_()
    dS.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), first.view(torch.int32))
    assert torch.equal(dS.cpu().view(torch.int32), d_first.view(torch.int32))


def test_exact_values_at_zero_and_one():
    """s = 0 and s = 1 give finite values and gradients: 0 and 34.5..., 0 and -1 (times 1 / rows)."""
    lib = _lib.load()
    S = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32).cuda()
    ws = torch.empty(lib.dp_assign_entropy_workspace_bytes(1, 2, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1,), GUARD, device="cuda")
    dS = torch.empty_like(S)
    _lib.check(lib.dp_assign_entropy_fwd(S.data_ptr(), 3, None, 1.0, out.data_ptr(), None, 1, 2, 3, ws.data_ptr(),
                                         ws.numel(), _lib.current_stream()), "dp_assign_entropy_fwd")
    _lib.check(lib.dp_assign_entropy_bwd(S.data_ptr(), 3, None, None, 1.0, dS.data_ptr(), 3, 0, 1, 2, 3,
                                         _lib.current_stream()), "dp_assign_entropy_bwd")
    assert float(out[0]) == 0.0
    d = dS.cpu().double().numpy() * 2
    want = -np.log(float(np.float32(1e-15)))
    assert np.allclose(d[S.cpu().numpy() == 0], want, rtol=1e-6, atol=0) and 34.5 < want < 34.6
    assert np.allclose(d[S.cpu().numpy() == 1], -1.0, rtol=1e-6, atol=0)
