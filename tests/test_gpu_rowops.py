"""The row kernels of dp_rowops.hip at every width tier, load form and group layout: the table of tests/rowop_cases.py
(test_rowop_plan_cpu.py asserts what it reaches) through the pass-through entries dp_rownorm_fwd, dp_bn_apply_fwd,
dp_bn_bwd_partials + dp_rownorm_bwd, dp_softmax_mask_fwd / _bwd, dp_masked_max_fwd / _bwd and dp_colsum_batched, each
compared with the float64 reference of the same operation at the bounds derived in rowop_cases.py; masked max, the
bf16 planes, the zero regions and the guard bands around every output exactly.

DP_ROWOPS_ANCHOR_OUT=<file> appends one line per case with its plan and its largest error / bound
(profiles/rowops_fp64_anchor.txt is the per-family digest of such a file, made by
`python -m tests.rowop_cases --digest <file> profiles/rowops_fp64_anchor.txt`)."""
import ctypes as C
import os

import pytest
import torch

from graph_pooling_amd import _lib
from tests import rowop_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def S():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """Device copies of Bufs; after the launch, `out` returns an output's entries and asserts that nothing else of
    its allocation changed."""

    def __init__(self):
        self.d = {}

    def up(self, buf):
        if id(buf) not in self.d:
            self.d[id(buf)] = (buf, buf.flat.cuda())
        return self.d[id(buf)][1]

    def ptr(self, buf, c0=0):
        return self.up(buf).data_ptr() + buf.byte_offset(c0)

    def group_ptrs(self, bufs):
        gp = _lib.GroupPtrs()
        for i, (b, c0) in enumerate(bufs):
            if b is not None:
                gp.p[i], gp.ld[i] = self.ptr(b, c0), b.ld
        return gp

    def out(self, what, buf, views):
        """views: [(c0, w)] written by the kernel -> the list of their contents; everything else must be unchanged."""
        got = self.d[id(buf)][1].cpu()
        want = buf.flat.clone()
        res = []
        for c0, w in views:
            v = buf.view(got, c0, w)
            buf.view(want, c0, w)[...] = v
            res.append(v.clone())
        if got.dtype.is_floating_point:
            got, want = torch.nan_to_num(got, nan=1e30), torch.nan_to_num(want, nan=1e30)
        assert torch.equal(got, want), f"{what}: wrote outside its own entries"
        return res


def tensor_buf(t, off=0):
    """A Buf around a dense tensor (1 row)."""
    b = RC.Buf(1, t.numel(), t.numel(), off, dtype=t.dtype, fill=RC.GUARD if t.dtype.is_floating_point else 0x5A)
    b.view()[...] = t.reshape(1, -1)
    return b


class Report:
    def __init__(self, case, lib):
        self.case, self.worst, self.bad = case, 0.0, []
        self.plan = RC.plan_of(lib, case)

    def close(self, what, got, ref, bound):
        got = got.double()
        assert bool(torch.isfinite(got).all()), f"{self.case.id} {what}: non-finite values"
        r = RC.ratio((got - ref).abs(), bound)
        print(f"{self.case.id} {what}: error / bound {r:.4f}")
        self.worst = max(self.worst, r)
        if not r <= 1.0:
            self.bad.append(f"{what}: {r:.3f} x the bound")

    def exact(self, what, ok, msg=""):
        if not ok:
            self.bad.append(f"{what}: {msg or 'not exact'}")

    def done(self):
        path = os.environ.get("DP_ROWOPS_ANCHOR_OUT")
        if path:
            with open(path, "a") as f:
                f.write(f"{self.case.id:44s} {str(self.plan):26s} {self.worst:8.4f}" +
                        ("  FAILED: " + "; ".join(self.bad) if self.bad else "") + "\n")
        assert not self.bad, f"{self.case.id} {self.plan}: " + "; ".join(self.bad)


def _recorded(lib, c):
    if RC.plan_args(c) is not None:
        assert RC.plan_of(lib, c) == RC.PLANS[c.id], (c.id, RC.plan_of(lib, c), RC.PLANS[c.id])


@pytest.mark.parametrize("c", RC.of("rownorm_fwd"), ids=RC.case_id)
def test_rownorm_fwd(lib, c):
    _recorded(lib, c)
    d, o, rows = RC.inputs(c.id), c.o, c.B * c.n
    dev, rep = Dev(), Report(c, lib)
    Ub = RC._joint_in(c, rows, d["Ug"])
    Pb = RC._joint_in(c, rows, d["Pg"]) if d["Pg"] else None
    bias = [(tensor_buf(b, c.off), 0) if b is not None else (None, 0) for b in d["bias"]]
    yb = RC._group_out(c, rows)
    invb = tensor_buf(torch.full((rows * c.G,), RC.GUARD), c.off) if o["invn"] else None
    partb = tensor_buf(torch.full((rows * c.G * 2,), RC.GUARD), c.off) if o["stats"] else None
    g, gb, gy = RC.groups_struct(c), dev.group_ptrs(bias), dev.group_ptrs(yb)
    _lib.check(lib.dp_rownorm_fwd(dev.ptr(Ub), Ub.ld, dev.ptr(Pb) if Pb else None, C.byref(g),
                                  C.byref(gb) if any(b is not None for b in d["bias"]) else None, C.byref(gy),
                                  dev.ptr(invb) if invb else None, dev.ptr(partb) if partb else None, rows,
                                  o["normalize"], o["stats"], S()), c.id)
    torch.cuda.synchronize()
    ref = RC.rownorm_fwd_math(c, d, torch.float64)
    ys = {}
    for i, (b, c0) in enumerate(yb):
        ys.setdefault(id(b), (b, []))[1].append((c0, c.w[i]))
    got_y = [v for b, views in ys.values() for v in dev.out("y", b, views)]
    inv = dev.out("invn", invb, [(0, rows * c.G)])[0].reshape(rows, c.G) if invb else None
    part = dev.out("part", partb, [(0, rows * c.G * 2)])[0].reshape(rows, c.G, 2) if partb else None
    for i in range(c.G):
        by, binv, bmean, bm2 = RC.rownorm_fwd_bounds(c, ref[i])
        rep.close(f"y[{i}]", got_y[i], ref[i]["y"], by)
        if inv is not None:
            rep.close(f"invn[{i}]", inv[:, i:i + 1], ref[i]["inv"], binv)
        if part is not None:
            rep.close(f"mean[{i}]", part[:, i, 0:1], ref[i]["mean"], bmean)
            rep.close(f"M2[{i}]", part[:, i, 1:2], ref[i]["m2"], bm2)
        if o["normalize"] and rows >= 3 and d["bias"][i] is None:
            rep.exact(f"zero row of group {i}", bool((got_y[i][0] == 0).all()), "a row of norm 0 must give 0")
            if inv is not None:
                rep.exact("invn of the zero row", float(inv[0, i]) == float(torch.tensor(1.0) / torch.tensor(1e-12)))
    rep.done()


@pytest.mark.parametrize("c", RC.of("bn_apply"), ids=RC.case_id)
def test_bn_apply_fwd(lib, c):
    _recorded(lib, c)
    d, o, rows = RC.inputs(c.id), c.o, c.B * c.n
    dev, rep = Dev(), Report(c, lib)
    Yb = RC._joint_in(c, rows, d["Yg"])
    partb = tensor_buf(d["part"], c.off) if o["part"] else None
    statb = tensor_buf(torch.full((c.n * c.G * 2,), RC.GUARD), c.off)
    xb = RC._group_out(c, rows)
    g, gx = RC.groups_struct(c), dev.group_ptrs(xb)
    _lib.check(lib.dp_bn_apply_fwd(dev.ptr(Yb), Yb.ld, dev.ptr(partb) if partb else None, dev.ptr(statb), C.byref(g),
                                   C.byref(gx), c.B, c.n, o["relu"], c.Bs, S()), c.id)
    torch.cuda.synchronize()
    ref = RC.bn_apply_math(c, d, torch.float64)
    xs = {}
    for i, (b, c0) in enumerate(xb):
        xs.setdefault(id(b), (b, []))[1].append((c0, c.w[i]))
    got_x = [v for b, views in xs.values() for v in dev.out("x", b, views)]
    stats = dev.out("stats", statb, [(0, c.n * c.G * 2)] if o["part"] else [])
    for i in range(c.G):
        bx, bmu, brstd = RC.bn_apply_bounds(c, ref[i])
        rep.close(f"x[{i}]", got_x[i], ref[i]["x"], bx)
        if o["part"]:
            st = stats[0].reshape(c.n, c.G, 2)
            rep.close(f"mu[{i}]", st[:, i, 0], ref[i]["mu"], bmu)
            rep.close(f"rstd[{i}]", st[:, i, 1], ref[i]["rstd"], brstd)
    rep.done()


@pytest.mark.parametrize("c", RC.of("rownorm_bwd"), ids=RC.case_id)
def test_bn_bwd_partials_then_rownorm_bwd(lib, c):
    _recorded(lib, c)
    d, o = RC.inputs(c.id), c.o
    Bs = c.Bs or c.B
    rows, rall, ct = c.B * c.n, Bs * c.n, RC.joint(c)
    dev, rep = Dev(), Report(c, lib)
    dxb, yb = RC._group_in(c, rall, d["DX"]), RC._group_in(c, rall, d["Y"])
    xb = RC._group_in(c, rall, d["X"]) if o["bn"] else [(None, 0)] * c.G
    invb, statb = tensor_buf(d["invn"], c.off), tensor_buf(d["stats"], c.off)
    partb = tensor_buf(torch.full((rall * c.G * 2,), RC.GUARD), c.off)
    dUb = RC.Buf(rows, ct, RC.ld_of(c, ct), c.off)
    stride = [w + 3 for w in c.w]
    want_db = o["dbias"] or (0,) * c.G
    dbb = [(RC.Buf(c.B, c.w[i], stride[i], c.off, fill=RC.SLAB0), 0) if want_db[i] else (None, 0) for i in range(c.G)]
    vsb = tensor_buf(torch.full((RC.vs_elems(c.B, c.n, ct),), 0x5A5A, dtype=torch.int16)) if o["vs"] else None
    g = RC.groups_struct(c)
    gdx, gy, gx, gdb = dev.group_ptrs(dxb), dev.group_ptrs(yb), dev.group_ptrs(xb), dev.group_ptrs(dbb)
    part = None
    if o["bn"]:
        _lib.check(lib.dp_bn_bwd_partials(C.byref(g), C.byref(gdx), C.byref(gx), dev.ptr(partb), rall, S()), c.id)
        torch.cuda.synchronize()
        part = dev.out("part", partb, [(0, rall * c.G * 2)])[0].reshape(rall, c.G, 2)     # (Bs > 32 overwrites it below)
    _lib.check(lib.dp_rownorm_bwd(C.byref(g), C.byref(gdx), C.byref(gx) if o["bn"] else None, C.byref(gy),
                                  dev.ptr(invb), dev.ptr(statb), dev.ptr(partb), dev.ptr(dUb), dUb.ld,
                                  C.byref(gdb) if o["dbias"] else None, c.B, c.n, o["relu"], o["bn"], o["normalize"],
                                  dev.ptr(vsb, 4) if vsb else None, c.Bs, S()), c.id)
    torch.cuda.synchronize()
    ref = RC.rownorm_bwd_math(c, d, torch.float64)
    emu = RC.rownorm_bwd_math(c, d, torch.float32)
    got = dev.out("dU", dUb, [(c.c0[i], c.w[i]) for i in range(c.G)])
    for b in [b for b, _ in dxb + yb + xb if b is not None] + [invb, statb]:
        dev.out("an input", b, [])
    dev.out("part", partb, [(0, rall * c.G * 2)] if o["bn"] else [])
    for i in range(c.G):
        if part is not None:
            pref, pb = RC.bn_bwd_partials_ref(c, d, i)
            rep.close(f"part[{i}]", part[:, i], pref, pb)
        bound = RC.rownorm_bwd_bound(ref[i], emu[i])
        assert RC.ratio((emu[i]["dU"].double() - ref[i]["dU"]).abs(), bound) <= 1.0
        rep.close(f"dU[{i}]", got[i], ref[i]["dU"], bound)
        if dbb[i][0] is not None:
            slab = dev.out("dbias", dbb[i][0], [(0, c.w[i])])[0]
            r3, b3 = ref[i]["dU"].reshape(c.B, c.n, -1), bound.expand_as(ref[i]["dU"]).reshape(c.B, c.n, -1)
            bdb = b3.sum(1) + ((c.n + 7) // 8 + 24) * RC.U * (r3.abs().sum(1) + RC.SLAB0)
            rep.close(f"dbias[{i}]", slab, r3.sum(1) + RC.SLAB0, bdb)
    if vsb:
        vs = dev.out("vs", vsb, [(4, RC.vs_elems(c.B, c.n, ct))])[0].reshape(-1)
        dense = torch.zeros(rows, ct)
        for i in range(c.G):
            dense[:, c.c0[i]:c.c0[i] + c.w[i]] = got[i]
        msg = RC.vs_check(vs, dense.reshape(c.B, c.n, ct), c.B, c.n, ct)
        rep.exact("vs", msg is None, msg)
    rep.done()


def _zero_region(kind):
    """(Buf of bytes poisoned 0xA5, byte offset of the region, its size): 16-byte aligned with a multiple-of-16 size, or
    neither."""
    off, size = (32, 4096 + 48) if kind == "aligned" else (36, 1000 + 6)
    return torch.full((off + size + 64,), 0xA5, dtype=torch.uint8), off, size


@pytest.mark.parametrize("c", RC.of("softmax_fwd"), ids=RC.case_id)
def test_softmax_mask_fwd(lib, c):
    _recorded(lib, c)
    d, o, rows, K = RC.inputs(c.id), c.o, c.B * c.n, c.w[0]
    dev, rep = Dev(), Report(c, lib)
    lb = RC.Buf(rows, K, K if c.tight else RC.ld_of(c, K + 2), c.off)
    lb.view()[...] = d["logits"]
    Sb = RC.Buf(rows, K, RC.ld_of(c, K), c.off)
    S2b = RC.Buf(rows, K, Sb.ld, c.off) if o["S2"] else None
    nn = d["nn"].cuda() if d["nn"] is not None else None
    vsb = tensor_buf(torch.full((RC.vs_elems(c.B, c.n, K),), 0x5A5A, dtype=torch.int16)) if o["vs"] else None
    zero = zoff = zsize = zdev = None
    if o["zero"]:
        zero, zoff, zsize = _zero_region(o["zero"])
        zdev = zero.cuda()
        assert (zdev.data_ptr() + zoff) % 16 == (0 if o["zero"] == "aligned" else 4)
    _lib.check(lib.dp_softmax_mask_fwd(dev.ptr(lb), lb.ld, dev.ptr(Sb), Sb.ld, nn.data_ptr() if nn is not None else None,
                                       c.B, c.n, K, dev.ptr(S2b) if S2b else None, dev.ptr(vsb, 4) if vsb else None,
                                       zdev.data_ptr() + zoff if o["zero"] else None, zsize if o["zero"] else 0, S()),
               c.id)
    torch.cuda.synchronize()
    ref = RC.softmax_fwd_math(c, d, torch.float64)
    bound = RC.softmax_fwd_bound(c, ref)
    got = dev.out("S", Sb, [(0, K)])[0]
    dev.out("logits", lb, [])
    rep.close("S", got, ref["s"], bound)
    rep.exact("masked rows", bool((got[~ref["valid"].reshape(-1)] == 0).all()), "a masked row is not exactly 0")
    if S2b:
        rep.exact("S2", torch.equal(dev.out("S2", S2b, [(0, K)])[0], got), "the second copy differs from S")
    if vsb:
        vs = dev.out("vs", vsb, [(4, RC.vs_elems(c.B, c.n, K))])[0].reshape(-1)
        msg = RC.vs_check(vs, got.reshape(c.B, c.n, K), c.B, c.n, K)
        rep.exact("vs", msg is None, msg)
    if o["zero"]:
        z = zdev.cpu()
        rep.exact("zero region", bool((z[zoff:zoff + zsize] == 0).all()), "not all zero")
        rep.exact("around the zero region", bool((z[:zoff] == 0xA5).all()) and bool((z[zoff + zsize:] == 0xA5).all()),
                  "bytes outside the region changed")
    rep.done()


@pytest.mark.parametrize("c", RC.of("softmax_bwd"), ids=RC.case_id)
def test_softmax_mask_bwd(lib, c):
    _recorded(lib, c)
    d, o, rows, K = RC.inputs(c.id), c.o, c.B * c.n, c.w[0]
    dev, rep = Dev(), Report(c, lib)
    Sb = RC.Buf(rows, K, RC.ld_of(c, K), c.off)
    Sb.view()[...] = d["S"]
    dSb = RC.Buf(rows, K, K if c.tight else RC.ld_of(c, K + 2), c.off)
    dSb.view()[...] = d["dS"]
    dS2b = None
    if d["dS2"] is not None:
        dS2b = RC.Buf(rows, K, dSb.ld, c.off)
        dS2b.view()[...] = d["dS2"]
        if rep.plan[4]:             # the generic path folds dS2 into dS over rows * ldds contiguous floats
            dS2b.flat[dS2b.off:] = 0.0
            dS2b.view()[...] = d["dS2"]
    dlb = RC.Buf(rows, K, K if c.tight else RC.ld_of(c, K + 4), c.off)
    stride = K + 5
    dbb = RC.Buf(c.B, K, stride, c.off, fill=RC.SLAB0) if o["dbias"] else None
    nn = d["nn"].cuda() if d["nn"] is not None else None
    _lib.check(lib.dp_softmax_mask_bwd(dev.ptr(Sb), Sb.ld, dev.ptr(dSb), dSb.ld, nn.data_ptr() if nn is not None else None,
                                       dev.ptr(dlb), dlb.ld, c.B, c.n, K, dev.ptr(dbb) if dbb else None, stride,
                                       dev.ptr(dS2b) if dS2b else None, S()), c.id)
    torch.cuda.synchronize()
    ref = RC.softmax_bwd_math(c, d, torch.float64)
    bound = RC.softmax_bwd_bound(c, ref)
    got = dev.out("dlogits", dlb, [(0, K)])[0]
    dev.out("S", Sb, [])
    if not rep.plan[4] or dS2b is None:
        dev.out("dS", dSb, [])
    else:                           # dS + dS2 where the rows are, dS2's zeros added to the padding, nothing else
        folded = dev.out("dS", dSb, [(0, K)])[0]
        rep.exact("dS + dS2", torch.equal(folded, d["dS"] + d["dS2"]), "the folded addend is not dS + dS2")
    rep.close("dlogits", got, ref["dl"], bound)
    if dbb:
        slab = dev.out("dbias", dbb, [(0, K)])[0]
        r3, b3 = ref["dl"].reshape(c.B, c.n, K), bound.reshape(c.B, c.n, K)
        bdb = b3.sum(1) + ((c.n + 63) // 64 + (c.n + 15) // 16 + 24) * RC.U * (r3.abs().sum(1) + RC.SLAB0)
        rep.close("dbias", slab, r3.sum(1) + RC.SLAB0, bdb)
    rep.done()


@pytest.mark.parametrize("c", RC.of("masked_max"), ids=RC.case_id)
def test_masked_max_fwd_and_bwd(lib, c):
    _recorded(lib, c)
    d, F = RC.inputs(c.id), c.w[0]
    dev, rep = Dev(), Report(c, lib)
    Zb = RC.Buf(c.B * c.n, F, RC.ld_of(c, F), c.off)
    Zb.view()[...] = d["Z"].reshape(c.B * c.n, F)
    outb = RC.Buf(c.B, F, RC.ld_of(c, F if c.tight else F + 2), c.off)
    argb = RC.Buf(c.B, F, F, c.off, dtype=torch.int32, fill=-77)          # (the entry takes no leading dimension for it)
    nn = d["nn"].cuda() if d["nn"] is not None else None
    _lib.check(lib.dp_masked_max_fwd(dev.ptr(Zb), Zb.ld, nn.data_ptr() if nn is not None else None, dev.ptr(outb),
                                     outb.ld, dev.ptr(argb), c.B, c.n, F, S()), c.id)
    torch.cuda.synchronize()
    out, am = RC.masked_max_ref(c, d)
    got, garg = dev.out("out", outb, [(0, F)])[0], dev.out("argmax", argb, [(0, F)])[0]
    assert bool(torch.isfinite(got).all())
    rep.exact("out", torch.equal(got, out), "max values differ")
    rep.exact("argmax", torch.equal(garg, am), f"{int((garg != am).sum())} arg-max entries differ")
    # backward: dZ[b, argmax, f] += dout[b, f], one fp32 add each
    dZb = RC.Buf(c.B * c.n, F, RC.ld_of(c, F if c.tight else F + 2), c.off, fill=0.25)
    dob = RC.Buf(c.B, F, RC.ld_of(c, F), c.off)
    dob.view()[...] = d["dout"]
    _lib.check(lib.dp_masked_max_bwd(dev.ptr(dob), dob.ld, dev.ptr(argb), dev.ptr(dZb), dZb.ld, c.B, c.n, F, S()), c.id)
    torch.cuda.synchronize()
    want = torch.full((c.B, c.n, F), 0.25)
    bi, fi = (am >= 0).nonzero(as_tuple=True)
    want[bi, am[bi, fi].long(), fi] += d["dout"][bi, fi]
    gz = dev.out("dZ", dZb, [(0, F)])[0]
    assert bool(torch.isfinite(gz).all())
    rep.exact("dZ", torch.equal(gz, want.reshape(c.B * c.n, F)), "the scattered gradient differs")
    rep.done()


@pytest.mark.parametrize("c", RC.of("colsum"), ids=RC.case_id)
def test_colsum_batched(lib, c):
    d, cols, split = RC.inputs(c.id), c.w[0], c.o["split"]
    dev, rep = Dev(), Report(c, lib)
    Xb = RC.Buf(c.B * c.n, cols, RC.ld_of(c, cols), c.off)
    Xb.view()[...] = d["X"].reshape(c.B * c.n, cols)
    ob = RC.Buf(c.B, cols, cols if c.tight else cols + 3, c.off, fill=RC.SLAB0 if split > 1 else RC.GUARD)
    _lib.check(lib.dp_colsum_batched(dev.ptr(Xb), Xb.ld, c.n * Xb.ld, c.n, cols, dev.ptr(ob), ob.ld, c.B, split, S()),
               c.id)
    torch.cuda.synchronize()
    ref, bound = RC.colsum_ref(c, d)
    rep.close("out", dev.out("out", ob, [(0, cols)])[0], ref, bound)
    rep.done()
