"""dp_frob_link_* and dp_csr_frob_link_* through the C entries, against the direct fp64 double sum and the derived
bounds of tests/frob_link_cases.py: exact cases, every K tier on all four forms, the slab edges of the Gram kernel,
ragged batches, masks, padded and offset buffers with guard bands, weighted and asymmetric adjacencies, accumulate /
dloss / total_inout, packed == fp32 bit for bit, repeat runs bit for bit, and a ring lattice of 2^20 nodes."""
import numpy as np
import pytest
import torch

from graph_pooling_amd import _lib
from graph_pooling_amd.encoders import PackedAdjacency
from tests import frob_link_cases as FC

pytestmark = pytest.mark.gpu

GUARD = -7.25
FRONT, TAIL = 4, 8
DLOSS, OLD_TOTAL = 1.75, 2.5
SLAB = FC.SLAB


RATIOS = {}             # case -> largest |error| / bound: [forward, backward, backward with accumulate = 1]


def _note(case, fwd=0.0, bwd=0.0, acc=0.0):
    r = RATIOS.setdefault(case, [0.0, 0.0, 0.0])
    r[0], r[1], r[2] = max(r[0], float(fwd)), max(r[1], float(bwd)), max(r[2], float(acc))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Buf:
    """[rows, K] at leading dimension ld inside a guarded flat device allocation, `off` floats past FRONT."""

    def __init__(self, rows, K, ld, off, data=None, fill=GUARD):
        self.rows, self.K, self.ld, self.start = rows, K, ld, FRONT + off
        host = torch.full((self.start + rows * ld + TAIL,), fill, dtype=torch.float32)
        if data is not None:
            self.view(host).copy_(torch.as_tensor(np.asarray(data, dtype=np.float32)).reshape(rows, K))
        self.host0 = host.clone()
        self.dev = host.cuda()

    def view(self, t):
        return t.as_strided((self.rows, self.K), (self.ld, 1), self.start)

    def ptr(self):
        return self.dev.data_ptr() + 4 * self.start

    def back(self):
        h = self.dev.cpu()
        return self.view(h).clone(), h

    def outside_untouched(self, h):
        a, b = h.clone(), self.host0.clone()
        self.view(a).zero_()
        self.view(b).zero_()
        return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _bits(x):
    return np.asarray(x, dtype=np.float32).tobytes()


def _graphs_of(S, A, nn):
    B, N, _ = S.shape
    nn = np.full(B, N) if nn is None else np.clip(nn, 0, N)
    return [(A[b, :nn[b], :nn[b]], S[b, :nn[b]]) for b in range(B)]


def _mask_fill(S, nn, value):
    out = S.copy()
    if nn is not None:
        for b in range(S.shape[0]):
            out[b, int(nn[b]):] = value
    return out


class Dense:
    """One dense problem on the device; `run` calls the fp32 or the packed entry and returns (loss bits, total, W, G)."""

    def __init__(self, S, A, nn, lds_pad=0, off=0, nan_outside=True):
        self.lib = _lib.load()
        self.B, self.N, self.K = S.shape
        self.S, self.A, self.nn = S, A, nn
        self.sb = Buf(self.B * self.N, self.K, self.K + lds_pad, off,
                      data=_mask_fill(S, nn, float("nan")).reshape(-1, self.K))
        Ad = A.copy()
        if nan_outside and nn is not None:          # entries outside the n_b x n_b block are never read
            for b in range(self.B):
                Ad[b, int(nn[b]):, :] = np.nan
                Ad[b, :, int(nn[b]):] = np.nan
        self.A_dev = _dev(Ad)
        self.nn_dev = None if nn is None else _dev(np.asarray(nn, dtype=np.int32))
        self.ws = torch.empty(self.lib.dp_frob_link_workspace_bytes(self.B, self.N, self.K), dtype=torch.uint8,
                              device="cuda")
        self.W = torch.full((self.B * self.N * self.K + TAIL,), GUARD, device="cuda")
        self.G = torch.full((self.B * self.K * self.K + TAIL,), GUARD, device="cuda")
        self.pk = None

    def pack(self, share=False):
        pk = PackedAdjacency.from_dense(_dev(self.A))
        self.pk = (pk.pk, pk.pk if share else pk.pkt)

    def fwd(self, packed=False, with_total=False, link_norm=None):
        lib = self.lib
        sc = torch.tensor([GUARD, GUARD, GUARD, GUARD, OLD_TOTAL, GUARD], dtype=torch.float32).cuda()
        tail = (_lib.ptr(self.nn_dev), _lib.ptr(link_norm), self.W.data_ptr(), self.G.data_ptr(), sc.data_ptr() + 4,
                sc.data_ptr() + 16 if with_total else None, self.B, self.N, self.K, self.ws.data_ptr(), self.ws.numel(),
                _lib.current_stream())
        if packed:
            _lib.check(lib.dp_frob_link_fwd_packed(self.sb.ptr(), self.sb.ld, self.pk[0].data_ptr(),
                                                   self.pk[1].data_ptr(), *tail), "dp_frob_link_fwd_packed")
        else:
            _lib.check(lib.dp_frob_link_fwd(self.sb.ptr(), self.sb.ld, self.A_dev.data_ptr(), *tail), "dp_frob_link_fwd")
        h = sc.cpu()
        assert h[0] == GUARD and h[2] == GUARD and h[3] == GUARD and h[5] == GUARD, h
        assert (self.W[-TAIL:] == GUARD).all() and (self.G[-TAIL:] == GUARD).all()
        assert torch.equal(self.sb.dev.cpu().view(torch.int32), self.sb.host0.view(torch.int32))      # S is read only
        return h[1].numpy().copy(), h[4].numpy().copy()

    def bwd(self, accumulate, dloss, ldds_pad=0, off=0, old=None, packed=False):
        lib = self.lib
        rows = self.B * self.N
        db = Buf(rows, self.K, self.K + ldds_pad, off, data=old)
        dl = None if dloss is None else torch.tensor([dloss], dtype=torch.float32).cuda()
        fn = lib.dp_frob_link_bwd_packed if packed else lib.dp_frob_link_bwd
        _lib.check(fn(self.sb.ptr(), self.sb.ld, self.W.data_ptr(), self.G.data_ptr(), _lib.ptr(self.nn_dev), None,
                      _lib.ptr(dl), db.ptr(), db.ld, accumulate, self.B, self.N, self.K, _lib.current_stream()),
                   "dp_frob_link_bwd")
        out, h = db.back()
        assert db.outside_untouched(h)
        return out.numpy().reshape(self.B, self.N, self.K)

    def check(self, packed=False, ldds_pad=0, off=0):
        """Forward and backward against the reference and the bounds; returns (loss bits, dS) of accumulate = 0."""
        ref = FC.batch_ref(_graphs_of(self.S, self.A, self.nn))
        tag = f"B={self.B} N={self.N} K={self.K} nn={None if self.nn is None else list(self.nn)} packed={packed}"
        loss, total = self.fwd(packed, with_total=True)
        case = f"{'packed' if packed else 'dense'} B={self.B} N={self.N} K={self.K}"
        _note(case, fwd=abs(float(loss) - ref["loss"]) / FC.fwd_bound(ref))
        assert abs(float(loss) - ref["loss"]) <= FC.fwd_bound(ref), (tag, float(loss), ref["loss"], FC.fwd_bound(ref))
        assert _bits(total) == _bits(np.float32(OLD_TOTAL) + np.float32(loss)), (tag, total, loss)
        loss2, total2 = self.fwd(packed, with_total=False)
        assert _bits(loss2) == _bits(loss) and float(total2) == OLD_TOTAL, tag
        nnv = np.full(self.B, self.N) if self.nn is None else np.clip(self.nn, 0, self.N)
        rng = np.random.default_rng(7)
        old = rng.standard_normal((self.B, self.N, self.K)).astype(np.float32)
        first = None
        for acc in (0, 1):
            for dl in (None, DLOSS):
                g = 1.0 if dl is None else dl
                out = self.bwd(acc, dl, ldds_pad, off, old=old.reshape(-1, self.K), packed=packed)
                for b in range(self.B):
                    n = int(nnv[b])
                    want = ref["dS"][b] * g
                    tol = FC.bwd_bound(ref, self.K, b, g)
                    if acc:
                        want = want + old[b, :n].astype(np.float64)
                        tol = tol + FC.U * (np.abs(want) + tol)        # fl(old + d'): u |old + d'|, d' within tol of d
                        assert _bits(out[b, n:]) == _bits(old[b, n:]), (tag, "masked rows are left alone")
                    else:
                        assert (out[b, n:] == 0).all(), (tag, "masked rows must be exactly 0")
                    err = np.abs(out[b, :n].astype(np.float64) - want)
                    _note(case, **{"acc" if acc else "bwd": (err / np.maximum(tol, 1e-300)).max()})
                    assert np.isfinite(out[b, :n]).all() and (err <= tol).all(), (tag, acc, dl, b,
                                                                                  float((err / np.maximum(tol, 1e-300)).max()))
                if acc == 0 and dl is None:
                    first = out
        return _bits(loss), first


def _problem(B, N, K, nn, seed, symmetric=True, weighted=False, self_loops=False, p=0.15):
    rng = np.random.default_rng(seed)
    nnv = np.full(B, N) if nn is None else np.asarray(nn)
    A = FC.dense_batch(rng, B, N, nnv, p=p, symmetric=symmetric, weighted=weighted, self_loops=self_loops)
    S = FC.softmax_rows(rng, B * N, K).reshape(B, N, K)
    return S, A


DENSE_SHAPES = [(1, 16, None), (1, 16, [5]), (3, 100, [100, 1, 37]), (3, 132, None), (3, 132, [1, 132, 77]),
                (1, 132, [131]), (3, 16, [16, 1, 9]), (1, 100, None)]


@pytest.mark.parametrize("K", FC.K_CASES)
def test_dense_every_k_shape_and_mask_fp32_and_packed(K):
    """B in {1, 3}, N in {16, 100, 132}, ragged node counts including 1 and N, and none; padded lds / ldds and buffers
    one float off their allocation; accumulate 0 / 1, dloss given / NULL, the total_inout add; the packed entry equals
    the fp32 entry bit for bit on the 0/1 adjacency (also with one buffer given as both A and A^T)."""
    for k, (B, N, nn) in enumerate(DENSE_SHAPES):
        S, A = _problem(B, N, K, nn, seed=1000 * K + k, self_loops=(k % 2 == 1))
        pad, off = ((0, 0), (3, 1), (4, 0), (1, 0))[k % 4]
        d = Dense(S, A, nn, lds_pad=pad, off=off)
        bits, dS = d.check(packed=False, ldds_pad=(pad + 1) if pad == 3 else pad, off=off)
        d.pack(share=False)
        bits_p, dS_p = d.check(packed=True, ldds_pad=pad, off=off)
        assert bits_p == bits and _bits(dS_p) == _bits(dS), (K, B, N, nn)
        d.pack(share=True)                           # symmetric: A^T is A, one read and a factor 2
        assert _bits(d.fwd(packed=True)[0]) == bits
        assert _bits(d.bwd(0, None, packed=True)) == _bits(dS)


@pytest.mark.parametrize("kind", ["weighted", "asymmetric", "weighted_asymmetric"])
def test_dense_fp32_entry_takes_weighted_and_asymmetric_adjacencies(kind):
    for B, N, K, nn in ((3, 100, 17, [100, 40, 1]), (1, 132, 64, None)):
        S, A = _problem(B, N, K, nn, seed=31 + N, symmetric="asym" not in kind, weighted="weighted" in kind, p=0.2)
        assert ("weighted" not in kind) or (np.isin(A, (0.0, 0.5, 2.0)).all() and (A == 0.5).any() and (A == 2.0).any())
        assert ("asym" not in kind) or (A != A.transpose(0, 2, 1)).any()
        Dense(S, A, nn).check()


def test_dense_asymmetric_packed_uses_both_copies():
    B, N, K, nn = 2, 132, 16, [132, 60]
    S, A = _problem(B, N, K, nn, seed=77, symmetric=False, p=0.2)
    d = Dense(S, A, nn)
    bits, dS = d.check()
    d.pack()
    bits_p, dS_p = d.check(packed=True)
    assert bits_p == bits and _bits(dS_p) == _bits(dS)


def test_link_norm_replaces_the_normaliser():
    B, N, K, nn = 3, 100, 16, [100, 50, 3]
    S, A = _problem(B, N, K, nn, seed=5)
    d = Dense(S, A, nn)
    ref = FC.batch_ref(_graphs_of(S, A, np.asarray(nn)), norm=777.0)
    loss, _ = d.fwd(link_norm=torch.tensor([777.0], device="cuda"))
    assert abs(float(loss) - ref["loss"]) <= FC.fwd_bound(ref)


# ---- exact cases
def _csr_call(S, indptr, indices, t=None, node_off=None, lds=None, dloss=None, accumulate=0, old=None):
    """The single-graph entry (node_off None) or the batch entry; returns (loss float32, dS [n, K] float32 numpy)."""
    lib = _lib.load()
    n, K = S.shape
    B = 1 if node_off is None else len(node_off) - 1
    Sd, ip, ix = _dev(S), _dev(indptr), _dev(indices if len(indices) else np.zeros(1, np.int32))
    tp = (None, None) if t is None else (_dev(t[0]), _dev(t[1]))
    ws = torch.empty(lib.dp_csr_frob_link_workspace_bytes(n, B, K), dtype=torch.uint8, device="cuda")
    ws.random_(0, 255)
    W = torch.full((n * K + TAIL,), GUARD, device="cuda")
    G = torch.full((B * K * K + TAIL,), GUARD, device="cuda")
    out = torch.full((3,), GUARD, device="cuda")
    dS = torch.full((n * K + TAIL,), GUARD, device="cuda") if old is None else _dev(np.concatenate(
        [old.reshape(-1), np.full(TAIL, GUARD, np.float32)]))
    dl = None if dloss is None else torch.tensor([dloss], dtype=torch.float32).cuda()
    st = _lib.current_stream()
    sym = int(t is None)
    if node_off is None:
        _lib.check(lib.dp_csr_frob_link_fwd(Sd.data_ptr(), K, ip.data_ptr(), ix.data_ptr(), _lib.ptr(tp[0]),
                                            _lib.ptr(tp[1]), None, W.data_ptr(), G.data_ptr(), out.data_ptr() + 4, None,
                                            n, K, ws.data_ptr(), ws.numel(), st), "dp_csr_frob_link_fwd")
        _lib.check(lib.dp_csr_frob_link_bwd(Sd.data_ptr(), K, W.data_ptr(), G.data_ptr(), None, _lib.ptr(dl),
                                            dS.data_ptr(), K, accumulate, sym, n, K, st), "dp_csr_frob_link_bwd")
    else:
        no = _dev(np.asarray(node_off, dtype=np.int32))
        _lib.check(lib.dp_csr_frob_link_batch_fwd(Sd.data_ptr(), K, ip.data_ptr(), ix.data_ptr(), _lib.ptr(tp[0]),
                                                  _lib.ptr(tp[1]), no.data_ptr(), None, W.data_ptr(), G.data_ptr(),
                                                  out.data_ptr() + 4, None, B, n, K, ws.data_ptr(), ws.numel(), st),
                   "dp_csr_frob_link_batch_fwd")
        _lib.check(lib.dp_csr_frob_link_batch_bwd(Sd.data_ptr(), K, W.data_ptr(), G.data_ptr(), no.data_ptr(), None,
                                                  _lib.ptr(dl), dS.data_ptr(), K, accumulate, sym, B, n, K, st),
                   "dp_csr_frob_link_batch_bwd")
    h, d = out.cpu(), dS.cpu()
    assert h[0] == GUARD and h[2] == GUARD
    assert (d[n * K:] == GUARD).all() and (W[-TAIL:] == GUARD).all() and (G[-TAIL:] == GUARD).all()
    return h[1].numpy().copy(), d[:n * K].numpy().reshape(n, K).copy()


def _block_diag_csr(parts):
    """[(a [n_b, n_b])] -> (indptr, global indices, node_off) of the block-diagonal batch."""
    ips, ixs, off, e0 = [np.zeros(1, np.int64)], [], [0], 0
    for a in parts:
        ip, ix = FC.csr_of(a)
        ips.append(ip[1:].astype(np.int64) + e0)
        ixs.append(ix.astype(np.int64) + off[-1])
        e0 += len(ix)
        off.append(off[-1] + a.shape[0])
    return (np.concatenate(ips).astype(np.int32), np.concatenate(ixs).astype(np.int32) if e0 else np.zeros(0, np.int32),
            np.asarray(off, dtype=np.int32))


def test_a_perfect_fit_is_exactly_zero_on_every_form():
    """Disjoint cliques with self loops and the one-hot assignment that fits them: loss 0.0 and dS exactly zero."""
    sizes, K = (5, 1, 9, 17), 6
    a, s = FC.cliques_one_hot(sizes, K)
    n = a.shape[0]
    N = 36
    A = np.zeros((2, N, N), np.float32)
    S = np.zeros((2, N, K), np.float32)
    A[0, :n, :n], S[0, :n] = a, s
    a1, s1 = FC.cliques_one_hot((3, 4), K)
    A[1, :7, :7], S[1, :7] = a1, s1
    d = Dense(S, A, [n, 7])
    loss, _ = d.fwd()
    assert _bits(loss) == _bits(0.0) and not d.bwd(0, DLOSS).any()
    d.pack()
    loss, _ = d.fwd(packed=True)
    assert _bits(loss) == _bits(0.0) and not d.bwd(0, DLOSS, packed=True).any()
    ip, ix = FC.csr_of(a)
    loss, dS = _csr_call(s, ip, ix, dloss=DLOSS)
    assert _bits(loss) == _bits(0.0) and not dS.any()
    bip, bix, off = _block_diag_csr([a, a1])
    loss, dS = _csr_call(np.concatenate([s, s1]), bip, bix, node_off=off, dloss=DLOSS)
    assert _bits(loss) == _bits(0.0) and not dS.any()


def test_quarter_grid_assignment_gives_the_rounded_fp64_value_bit_for_bit():
    rng = np.random.default_rng(3)
    nn, N, K = [40, 13, 1], 40, 5
    A = FC.dense_batch(rng, 3, N, nn, p=0.3, self_loops=True)
    S = FC.quarter_grid(rng, 3 * N, K).reshape(3, N, K)
    graphs = _graphs_of(S, A, np.asarray(nn))
    ref = FC.batch_ref(graphs)
    want = _bits(np.float32(np.float64(ref["F"]) / np.float64(ref["norm"])))
    assert ref["F"] == round(ref["F"] * 256) / 256 and ref["F"] > 1              # small-integer sums of 1/256ths
    d = Dense(S, A, nn)
    assert _bits(d.fwd()[0]) == want
    d.pack()
    assert _bits(d.fwd(packed=True)[0]) == want
    bip, bix, off = _block_diag_csr([a for a, _ in graphs])
    assert _bits(_csr_call(np.concatenate([s for _, s in graphs]), bip, bix, node_off=off)[0]) == want
    one = FC.batch_ref(graphs[:1])
    ip, ix = FC.csr_of(graphs[0][0])
    assert _bits(_csr_call(graphs[0][1], ip, ix)[0]) == _bits(np.float32(one["F"] / one["norm"]))


# ---- CSR: every K, the slab edges, graph shapes
def _check_csr(a, S, directed=False, batch_sizes=None):
    """One graph (or, with batch_sizes, the ragged batch a is the block diagonal of) against the reference."""
    n, K = S.shape
    if batch_sizes is None:
        graphs, node_off = [(a, S)], None
        ip, ix = FC.csr_of(a)
    else:
        off = np.concatenate([[0], np.cumsum(batch_sizes)])
        graphs = [(a[off[b]:off[b + 1], off[b]:off[b + 1]], S[off[b]:off[b + 1]]) for b in range(len(batch_sizes))]
        ip, ix, node_off = _block_diag_csr([g[0] for g in graphs])
    t = FC.csr_of(a.T) if directed else None
    ref = FC.batch_ref(graphs)
    tag = f"n={n} K={K} directed={directed} batch={batch_sizes}"
    loss, dS = _csr_call(S, ip, ix, t=t, node_off=node_off)
    case = f"{'csr' if batch_sizes is None else 'batch'} n={n} K={K}{' directed' if directed else ''}"
    _note(case, fwd=abs(float(loss) - ref["loss"]) / FC.fwd_bound(ref))
    assert abs(float(loss) - ref["loss"]) <= FC.fwd_bound(ref), (tag, float(loss), ref["loss"], FC.fwd_bound(ref))
    want = np.concatenate(ref["dS"])
    tol = np.concatenate([FC.bwd_bound(ref, K, b) for b in range(len(graphs))])
    err = np.abs(dS.astype(np.float64) - want)
    _note(case, bwd=(err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all(), (tag, float((err / np.maximum(tol, 1e-300)).max()))
    # dloss and accumulate = 1
    old = np.random.default_rng(1).standard_normal((n, K)).astype(np.float32)
    loss2, dS2 = _csr_call(S, ip, ix, t=t, node_off=node_off, dloss=DLOSS, accumulate=1, old=old)
    assert _bits(loss2) == _bits(loss), tag                       # two runs, other workspace contents: the same bits
    want2 = want * DLOSS + old
    err = np.abs(dS2.astype(np.float64) - want2)
    tol2 = tol * DLOSS
    tol2 = tol2 + FC.U * (np.abs(want2) + tol2)
    _note(case, acc=(err / np.maximum(tol2, 1e-300)).max())
    assert (err <= tol2).all(), tag
    return loss, dS


def _sparse_graph(rng, n, deg=3, symmetric=True, self_loops=False, isolated=()):
    """A sparse 0/1 [n, n] (dense storage: the reference needs it anyway) with about deg entries a row."""
    a = np.zeros((n, n), dtype=np.float32)
    if n > 1:
        r = np.repeat(np.arange(n), deg)
        c = rng.integers(0, n, size=r.size)
        keep = r != c
        a[r[keep], c[keep]] = 1.0
    if symmetric:
        a = np.maximum(a, a.T)
    if self_loops:
        a[np.arange(0, n, 3), np.arange(0, n, 3)] = 1.0
    for i in isolated:
        a[i, :] = 0.0
        a[:, i] = 0.0
    return a


@pytest.mark.parametrize("K", FC.K_CASES)
def test_csr_every_k(K):
    rng = np.random.default_rng(K)
    n = 300
    _check_csr(_sparse_graph(rng, n), FC.softmax_rows(rng, n, K))


@pytest.mark.parametrize("n", [1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1])
def test_csr_slab_edges(n):
    rng = np.random.default_rng(n)
    _check_csr(_sparse_graph(rng, n), FC.softmax_rows(rng, n, 17))


@pytest.mark.parametrize("shape", ["isolated_node", "directed", "self_loops", "no_edges"])
def test_csr_graph_shapes(shape):
    rng = np.random.default_rng(11)
    n, K = 257, 16
    a = _sparse_graph(rng, n, symmetric=shape != "directed", self_loops=shape == "self_loops",
                      isolated=(0, 100, n - 1) if shape == "isolated_node" else ())
    if shape == "no_edges":
        a[:] = 0.0
    assert shape != "directed" or (a != a.T).any()
    _check_csr(a, FC.softmax_rows(rng, n, K), directed=shape == "directed")


@pytest.mark.parametrize("K", FC.K_CASES)
def test_ragged_batch_every_k(K):
    rng = np.random.default_rng(100 + K)
    sizes = (1, 70, 3, 129, 7)
    n = sum(sizes)
    a = np.zeros((n, n), np.float32)
    off = 0
    for m in sizes:
        a[off:off + m, off:off + m] = _sparse_graph(rng, m, self_loops=True)
        off += m
    _check_csr(a, FC.softmax_rows(rng, n, K), batch_sizes=sizes)


@pytest.mark.parametrize("directed", [False, True])
def test_ragged_batch_across_slab_edges(directed):
    """Sizes (1, slab + 1, 3, 2 slab, 7): graphs that share a slab, graphs cut by slab edges, a graph of several slabs."""
    rng = np.random.default_rng(9)
    sizes = (1, SLAB + 1, 3, 2 * SLAB, 7)
    n = sum(sizes)
    a = np.zeros((n, n), np.float32)
    off = 0
    for m in sizes:
        a[off:off + m, off:off + m] = _sparse_graph(rng, m, symmetric=not directed)
        off += m
    _check_csr(a, FC.softmax_rows(rng, n, 16), directed=directed, batch_sizes=sizes)


def test_a_batch_of_one_equals_the_single_graph_entry_bit_for_bit():
    rng = np.random.default_rng(4)
    n, K = 2 * SLAB + 5, 33
    a = _sparse_graph(rng, n)
    S = FC.softmax_rows(rng, n, K)
    ip, ix = FC.csr_of(a)
    l1, d1 = _csr_call(S, ip, ix, dloss=DLOSS)
    l2, d2 = _csr_call(S, ip, ix, node_off=[0, n], dloss=DLOSS)
    assert _bits(l1) == _bits(l2) and _bits(d1) == _bits(d2)
    l3, d3 = _csr_call(S, ip, ix, dloss=DLOSS)
    assert _bits(l1) == _bits(l3) and _bits(d1) == _bits(d3)                       # and two runs agree


def test_dense_two_runs_are_bit_identical():
    S, A = _problem(3, 132, 65, [132, 1, 77], seed=8)
    d = Dense(S, A, [132, 1, 77])
    l1, _ = d.fwd()
    g1 = d.bwd(0, DLOSS)
    d.ws.random_(0, 255)
    d.W.fill_(GUARD)
    d.G.fill_(GUARD)
    l2, _ = d.fwd()
    assert _bits(l1) == _bits(l2) and _bits(g1) == _bits(d.bwd(0, DLOSS))


def test_ring_lattice_of_a_million_nodes():
    """n = 2^20, i <-> i +- 1, i +- 2, K = 16: forward and backward against a chunked fp64 evaluation of G, W and the
    three terms on the device (the direct double sum has 2^40 pairs)."""
    lib = _lib.load()
    n, K = 1 << 20, 16
    ip, ix = FC.ring_lattice_csr(n)
    g = torch.Generator(device="cuda").manual_seed(3)
    S = torch.softmax(2.0 * torch.randn(n, K, device="cuda", generator=g), dim=1)
    ipd, ixd = _dev(ip), _dev(ix)
    ws = torch.empty(lib.dp_csr_frob_link_workspace_bytes(n, 1, K), dtype=torch.uint8, device="cuda")
    W = torch.empty(n, K, device="cuda")
    G = torch.empty(K, K, device="cuda")
    out = torch.full((3,), GUARD, device="cuda")
    dS = torch.full((n * K + TAIL,), GUARD, device="cuda")
    st = _lib.current_stream()
    _lib.check(lib.dp_csr_frob_link_fwd(S.data_ptr(), K, ipd.data_ptr(), ixd.data_ptr(), None, None, None, W.data_ptr(),
                                        G.data_ptr(), out.data_ptr() + 4, None, n, K, ws.data_ptr(), ws.numel(), st),
               "dp_csr_frob_link_fwd")
    _lib.check(lib.dp_csr_frob_link_bwd(S.data_ptr(), K, W.data_ptr(), G.data_ptr(), None, None, dS.data_ptr(), K, 0, 1,
                                        n, K, st), "dp_csr_frob_link_bwd")
    S64 = S.double()
    G64 = torch.zeros(K, K, dtype=torch.float64, device="cuda")
    W64 = torch.zeros(n, K, dtype=torch.float64, device="cuda")
    nbr = ixd.long().reshape(n, 4)
    for lo in range(0, n, 1 << 18):
        hi = lo + (1 << 18)
        G64 += S64[lo:hi].T @ S64[lo:hi]
        W64[lo:hi] = S64[nbr[lo:hi]].sum(dim=1)                      # A S; A is symmetric: W = 2 A S
    T0, T1, T2 = float(n * 4), float((S64 * W64).sum()), float((G64 * G64).sum())
    norm = float(n) * float(n)
    D = 8
    bound = FC.c_fwd(D) * FC.U * (T0 + 2 * T1 + T2) / norm
    loss = float(out[1])
    assert out[0] == GUARD and out[2] == GUARD
    _note("csr ring lattice n=2^20 K=16", fwd=abs(loss - (T0 - 2 * T1 + T2) / norm) / bound)
    assert abs(loss - (T0 - 2 * T1 + T2) / norm) <= bound, (loss, (T0 - 2 * T1 + T2) / norm, bound)
    want = (4.0 * S64 @ G64 - 4.0 * W64) / norm
    tol = FC.c_bwd(K, D) * FC.U * (4.0 * S64 @ G64 + 4.0 * W64) / norm
    got = dS[:n * K].reshape(n, K).double()
    assert (dS[n * K:] == GUARD).all()
    _note("csr ring lattice n=2^20 K=16", bwd=float(((got - want).abs() / tol).max()))
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())
