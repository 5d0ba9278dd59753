"""Refusals and workspace sizes of the CSR / ragged C entries, pinned to the library of the commit before the entry
layer was folded into one checked body per op (tests/golden/csr_entry_args.json, recorded from that commit's build).

Every case is ONE fault in an otherwise valid call, so the entry must refuse it before it launches anything: the test
compares the return code and the message byte for byte.  The pointers are addresses of real host buffers; the
node_off_host arrays are real because the library reads them.  No case is a valid call, and the module skips itself
when a GPU is visible, so a check that went missing can never turn into a launch on these host addresses.

Cases whose refusal comes from the bump allocator (DP_ERR_WORKSPACE, -2: the pooling, GraphConv and ragged entries do not
size their workspace up front) are not in the table: the golden holds argument refusals only, rc in {-1, -3}.

Recording (on the PARENT commit's library, never on the tree under test):
    DP_LIB=<parent build>/libdiffpool_hip.so python -m tests.test_csr_entry_args_cpu --record
"""
import ctypes as C
import json
import os
import sys

import pytest

from graph_pooling_amd import _lib
from tests.test_abi_cpu import _header_functions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csr_entry_args.json")
INVALID, UNSUPPORTED = -1, -3
BIG = 1 << 26

# ------------------------------------------------------------------ host buffers
_BUFS = {}


def _addr(name):
    """64-byte aligned address of a 4 KiB host buffer of its own per name."""
    if name not in _BUFS:
        raw = (C.c_char * (4096 + 64))()
        _BUFS[name] = (raw, (C.addressof(raw) + 63) & ~63)
    return _BUFS[name][1]


def _ints(*v):
    key = "ints:" + ",".join(map(str, v))
    if key not in _BUFS:
        arr = (C.c_int * max(len(v), 1))(*v)
        _BUFS[key] = (arr, C.addressof(arr))
    return _BUFS[key][1]


OFF2, OFF2_FROM1, OFF2_EQUAL = (0, 3, 8), (1, 3, 8), (0, 3, 3)        # a batch of two graphs, 3 + 5 rows
# a leading dimension and the width it must cover (a scalar fault past its bound widens them: still one fault)
WIDTHS = {"K": ("lds", "ldds"), "D": ("ldz", "lddz"), "d": ("lde", "ldde"), "feat": ("ldt", "ldo"),
          "F": ("ldx", "ldy", "lddy", "lddx", "ldz", "ldo", "lddz", "ldp", "lds", "ldg")}


# ------------------------------------------------------------------ the table
# entry -> (valid scalars / special pointers, faults).  Every pointer argument not named in the first dict is the
# address of a buffer of its own.  Faults:
#   ("null", names)  each pointer NULL            ("odd", names)   each pointer at address + 1
#   ("set", name, values)  a scalar at each value ("case", label, {arg: value})  anything else, spelled out
def _ws(query, *a):
    return ("ws", query, a)


def _pool(weighted, bwd, batch):
    v = dict(n=8, n_total=8, K=4, D=4, lds=4, ldz=4, ldds=4, lddz=4, B=1, n_slabs=1, n_blocks=1, workspace_bytes=BIG)
    ptrs = "S Z indptr indices" + (" indptr_t indices_t dXp dAp dS dZ" if bwd else " Xp Ap")
    ptrs += (" bwd_tab" if bwd else " fwd_tab slab_off") if batch else ""
    ptrs += " values" if weighted else ""
    f = [("null", ptrs), ("odd", ptrs), ("odd", "workspace"), ("set", "n_total" if batch else "n", (0, -1)),
         ("set", "K", (0, -1, 257)), ("set", "D", (0, -1, 513)), ("set", "lds", (3,)), ("set", "ldz", (3,))]
    if bwd:
        f += [("set", "ldds", (3,)), ("set", "lddz", (3,))]
        if weighted:
            f += [("null", "values_t"), ("odd", "values_t")]
    if batch:
        f += [("set", "B", (0, -1, 65536)), ("set", "n_blocks" if bwd else "n_slabs", (0,))]
        if not bwd:
            f += [("set", "n_slabs", (65536,))]
    return v, f


def _link(weighted, bwd, batch):
    ix = "indices_local" if batch else "indices"
    ixt = "indices_t_local" if batch else "indices_t"
    v = dict(n=8, K=4, lds=4, ldds=4, accumulate=0, workspace_bytes=BIG)
    if batch:
        v.update(B=2, node_off_host=_ints(*OFF2))
    ptrs = f"S indptr {ix}" + (f" indptr_t {ixt} dS" if bwd else " loss_out") + (" values" if weighted else "")
    need = _ws("dp_csr_linkpred_batch_workspace_bytes", _ints(*OFF2), 2, 4) if batch else \
        _ws("dp_csr_linkpred_workspace_bytes", 8, 4)
    f = [("null", ptrs + " workspace"), ("odd", ptrs + " workspace"), ("set", "K", (0, -1, 257)), ("set", "lds", (3,)),
         ("set", "workspace_bytes", (0, need))]
    if bwd:
        f += [("odd", "dloss"), ("set", "ldds", (3,))]
        if weighted:
            f += [("null", "values_t"), ("odd", "values_t")]
    if batch:
        f += [("null", "node_off_host"), ("set", "B", (0, -1)),
              ("case", "node_off[0]=1", dict(node_off_host=_ints(*OFF2_FROM1))),
              ("case", "node_off equal neighbours", dict(node_off_host=_ints(*OFF2_EQUAL)))]
    else:
        f += [("set", "n", (0, -1))]
    return v, f


def _frob_dense(packed):
    v = dict(B=2, N=8, K=4, lds=4, workspace_bytes=BIG)
    need = _ws("dp_frob_link_workspace_bytes", 2, 8, 4)
    f = [("null", "S W G loss_out workspace " + ("adj_pk adj_pkt" if packed else "adj")), ("set", "B", (0, -1)),
         ("set", "N", (0, -1)), ("set", "K", (0, -1, 257)), ("set", "lds", (3,)), ("set", "workspace_bytes", (0, need))]
    if packed:
        f += [("odd", "adj_pk adj_pkt")]
    return v, f


def _frob_csr(weighted, batch):
    v = dict(n=8, n_total=8, B=2, K=4, lds=4, workspace_bytes=BIG)
    need = _ws("dp_csr_frob_link_workspace_bytes", 8, 2 if batch else 1, 4)
    f = [("null", "S indptr indices W G loss_out workspace" + (" values" if weighted else "") + (" node_off" if batch else "")),
         ("null", "indptr_t"), ("null", "indices_t"), ("set", "n_total" if batch else "n", (0, -1)),
         ("set", "K", (0, -1, 257)), ("set", "lds", (3,)), ("set", "workspace_bytes", (0, need))]
    if weighted:
        f += [("null", "values_t")]
    if batch:
        f += [("set", "B", (0, -1, 9))]
    return v, f


def _frob_bwd(csr, batch):
    v = dict(B=2, N=8, n=8, n_total=8, K=4, lds=4, ldds=4, accumulate=0, symmetric=1)
    f = [("null", "S W G dS" + (" node_off" if batch else "")), ("set", "K", (0, -1, 257)), ("set", "lds", (3,)),
         ("set", "ldds", (3,))]
    f += [("set", s, (0, -1)) for s in ((("B", "n_total") if batch else ("n",)) if csr else ("B", "N"))]
    return v, f


def _gcn(weighted, bwd):
    v = dict(n=8, Fin=4, Fout=4, ldx=4, ldy=4, lddy=4, lddx=4, flags=0, workspace_bytes=BIG)
    ptrs = ("ax indptr indices W y invnorm dy dW" if bwd else "x indptr indices W y ax invnorm") + \
        (" values" if weighted else "")
    f = [("null", ptrs), ("set", "n", (0, -1)), ("set", "Fin", (0, -1)), ("set", "Fout", (0, -1))]
    if bwd:
        f += [("null", "indptr_t"), ("null", "indices_t"), ("set", "lddx", (3,))]
        if weighted:
            f += [("null", "values_t")]
    else:
        f += [("case", "add_self with ldx != Fin", dict(flags=1, ldx=5))]
    return v, f


def _bn_bwd(g):
    v = dict(B=2, max_n=5, n_idx=6, F=4, ldx=4, ldy=4, lddy=4, lddx=4, ldg=4, relu=1, workspace_bytes=BIG)
    ptrs = "y stats dy dx node_off order cnt"
    f = [("null", ptrs), ("odd", ptrs), ("null", "x"), ("null", "pad"), ("set", "B", (0, -1)), ("set", "max_n", (0, -1)),
         ("set", "F", (0, -1, 2049))] + [("set", ld, (3,)) for ld in ("ldx", "ldy", "lddy", "lddx")]
    if g:
        f += [("odd", "G"), ("set", "n_idx", (4, 7)), ("set", "ldg", (3,))]
    return v, f


def _const(names):
    return dict(F=4, flags=0), [("null", names), ("odd", names), ("set", "F", (0, -1)), ("set", "flags", (1,))]


def _seg_fwd(floor):
    v = dict(B=2, F=4, n_chunks=2, ldz=4, ldo=4, lds=4, n_min=2, n_idx=5, floor_row=None, workspace_bytes=BIG)
    ptrs = "Z node_off chunk_tab chunk_off out argmax"
    f = [("null", ptrs), ("odd", ptrs), ("set", "B", (0, -1)), ("set", "F", (0, -1)), ("set", "n_chunks", (0, 1, 65536)),
         ("case", "B=65536", dict(B=65536, n_chunks=65536)), ("set", "ldz", (3,)), ("set", "ldo", (3,))]
    if floor:
        f += [("set", "F", (2049,)), ("case", "sufv and floor_row", dict(floor_row=_addr("floor_row"))),
              ("null", "sufv"), ("null", "sufi"), ("null", "floor_flag"), ("set", "lds", (3,)), ("set", "n_min", (0, -1)),
              ("set", "n_idx", (2, 1))]
    return v, f


def _seg_bwd(floor):
    v = dict(B=2, F=4, ldo=4, lddz=4, ldg=4, n_min=2, n_idx=5, table=1)
    ptrs = "dout argmax node_off dZ"
    f = [("null", ptrs), ("odd", ptrs), ("set", "B", (0, -1)), ("set", "F", (0, -1)), ("set", "ldo", (3,)),
         ("set", "lddz", (3,))]
    if floor:
        f += [("set", "F", (2049,)), ("odd", "G"), ("set", "n_min", (0, -1)), ("set", "n_idx", (1,)), ("set", "ldg", (3,))]
    return v, f


def _s2s(bwd):
    off = _ints(*OFF2)
    v = dict(B=2, T=5, d=4, lde=4, ldde=4, node_off_host=off, save_bytes=BIG, workspace_bytes=BIG)
    ptrs = "emb node_off w_ih w_hh Wp out" + (" dout demb dw_ih dw_hh db_ih db_hh dWp dbp save" if bwd else " b_ih b_hh bp")
    need = _ws("dp_set2set_ragged_save_bytes", off, 2, 5, 4)
    f = [("null", ptrs + " node_off_host"), ("odd", ptrs), ("set", "B", (-1, 65536)), ("set", "d", (0, -1, 257)),
         ("set", "T", (0, -1, 4)), ("case", "node_off_host[0]=-1", dict(node_off_host=_ints(-1, 3, 8))),
         ("case", "node_off_host equal neighbours", dict(node_off_host=_ints(*OFF2_EQUAL))), ("set", "lde", (3,)),
         ("set", "save_bytes", (0, need))]
    f += [("set", "ldde", (3,))] if bwd else [("odd", "save")]
    return v, f


def _table():
    t = {}
    for w in ("", "_w"):
        t["dp_csr_pool_fwd" + w] = _pool(bool(w), False, False)
        t["dp_csr_pool_bwd" + w] = _pool(bool(w), True, False)
        t["dp_csr_pool_batch_fwd" + w] = _pool(bool(w), False, True)
        t["dp_csr_pool_batch_bwd" + w] = _pool(bool(w), True, True)
        t["dp_csr_linkpred_loss_fwd" + w] = _link(bool(w), False, False)
        t["dp_csr_linkpred_loss_bwd" + w] = _link(bool(w), True, False)
        t["dp_csr_linkpred_batch_loss_fwd" + w] = _link(bool(w), False, True)
        t["dp_csr_linkpred_batch_loss_bwd" + w] = _link(bool(w), True, True)
        t["dp_csr_frob_link_fwd" + w] = _frob_csr(bool(w), False)
        t["dp_csr_frob_link_batch_fwd" + w] = _frob_csr(bool(w), True)
        t["dp_sparse_gcn_layer_fwd" + w] = _gcn(bool(w), False)
        t["dp_sparse_gcn_layer_bwd" + w] = _gcn(bool(w), True)
        t["dp_csr_aggregate" + w] = (dict(ldt=4, ldo=4, n_rows=8, feat=4, mean=0, beta=0.0),
                                     [("null", "table indptr indices out" + (" values" if w else "")),
                                      ("set", "n_rows", (0, -1)), ("set", "feat", (0, -1))])
    t["dp_csr_pool_batch_plan"] = (
        dict(node_off_host=_ints(*OFF2), B=2, K=4, D=4),
        [("null", "node_off_host counts_host"), ("set", "B", (0, -1)), ("set", "K", (0, -1, 257)),
         ("set", "D", (0, -1, 513)), ("case", "node_off[0]=1", dict(node_off_host=_ints(*OFF2_FROM1))),
         ("case", "node_off equal neighbours", dict(node_off_host=_ints(*OFF2_EQUAL)))])
    t["dp_frob_link_fwd"] = _frob_dense(False)
    t["dp_frob_link_fwd_packed"] = _frob_dense(True)
    t["dp_frob_link_bwd"] = _frob_bwd(False, False)
    t["dp_frob_link_bwd_packed"] = _frob_bwd(False, False)
    t["dp_csr_frob_link_bwd"] = _frob_bwd(True, False)
    t["dp_csr_frob_link_batch_bwd"] = _frob_bwd(True, True)
    t["dp_bn_ragged_fwd"] = (dict(B=2, max_n=5, F=4, ldx=4, ldy=4, relu=0),
                             [("null", "x y stats node_off order cnt"), ("odd", "x y stats node_off order cnt"),
                              ("set", "B", (0, -1)), ("set", "max_n", (0, -1)), ("set", "F", (0, -1, 2049)),
                              ("set", "ldx", (3,)), ("set", "ldy", (3,))])
    t["dp_bn_ragged_bwd"] = _bn_bwd(False)
    t["dp_bn_ragged_g_bwd"] = _bn_bwd(True)
    t["dp_gcn_pad_const_fwd"] = _const("pad")
    t["dp_gcn_pad_const_bwd"] = _const("bias dpad dbias")
    t["dp_gcn_row_const_fwd"] = _const("c")
    t["dp_gcn_row_const_bwd"] = _const("bias dc dbias")
    t["dp_segment_max_fwd"] = _seg_fwd(False)
    t["dp_segment_max_bwd"] = _seg_bwd(False)
    t["dp_segment_max_floor_fwd"] = _seg_fwd(True)
    t["dp_segment_max_floor_bwd"] = _seg_bwd(True)
    t["dp_ragged_padval_fwd"] = (dict(ldp=4, n_min=2, max_n=5, n_idx=6, F=4),
                                 [("null", "stats padval"), ("odd", "stats padval"), ("set", "F", (0, -1, 2049)),
                                  ("set", "n_min", (0, -1, 6)), ("set", "max_n", (0, -1)), ("set", "n_idx", (4, 7)),
                                  ("set", "ldp", (3,))])
    t["dp_ragged_suffix_max"] = (dict(ldp=4, lds=4, n_min=2, n_idx=6, F=4, workspace_bytes=BIG),
                                 [("null", "padval sufv sufi"), ("odd", "padval sufv sufi"), ("set", "F", (0, -1, 2049)),
                                  ("set", "n_min", (0, -1)), ("set", "n_idx", (1,)), ("set", "ldp", (3,)),
                                  ("set", "lds", (3,))])
    t["dp_set2set_ragged_fwd"] = _s2s(False)
    t["dp_set2set_ragged_bwd"] = _s2s(True)
    return t


# ------------------------------------------------------------------ workspace queries
N_GRID, K_GRID, D_GRID = (1, 63, 64, 65, 129, 5748), (1, 5, 8, 64, 65, 128, 192, 256), (1, 20, 64, 512)


def _sizes(lib):
    out = {}
    for n in N_GRID:
        off = _ints(0, n)
        for K in K_GRID:
            out[f"dp_csr_linkpred_workspace_bytes({n},{K})"] = lib.dp_csr_linkpred_workspace_bytes(n, K)
            out[f"dp_csr_linkpred_batch_workspace_bytes([0,{n}],1,{K})"] = \
                lib.dp_csr_linkpred_batch_workspace_bytes(off, 1, K)
            out[f"dp_csr_frob_link_workspace_bytes({n},1,{K})"] = lib.dp_csr_frob_link_workspace_bytes(n, 1, K)
            for D in D_GRID:
                out[f"dp_csr_pool_workspace_bytes({n},{K},{D})"] = lib.dp_csr_pool_workspace_bytes(n, K, D)
                out[f"dp_csr_pool_batch_workspace_bytes({max(1, n // 64)},1,{K},{D})"] = \
                    lib.dp_csr_pool_batch_workspace_bytes(max(1, n // 64), 1, K, D)
        for D in D_GRID:
            out[f"dp_sparse_gcn_layer_workspace_bytes({n},{D},20)"] = lib.dp_sparse_gcn_layer_workspace_bytes(n, D, 20)
            out[f"dp_sparse_gcn_layer_workspace_bytes({n},20,{D})"] = lib.dp_sparse_gcn_layer_workspace_bytes(n, 20, D)
    for n in (1, 63, 64, 65, 129):           # graphs the persistent Set2Set kernel takes
        off = _ints(0, n, n + 3)
        for d in (1, 20, 64):
            out[f"dp_set2set_ragged_save_bytes([0,{n},{n + 3}],2,{n},{d})"] = lib.dp_set2set_ragged_save_bytes(off, 2, n, d)
            out[f"dp_set2set_ragged_bwd_workspace_bytes([0,{n},{n + 3}],2,{n},{d})"] = \
                lib.dp_set2set_ragged_bwd_workspace_bytes(off, 2, n, d)
    return out


# ------------------------------------------------------------------ running the table
def _cases(lib):
    """(entry, case label, argument list) of every fault of the table."""
    fns = _header_functions()
    for entry, (valid, faults) in _table().items():
        args = [a.split()[-1].lstrip("*") for a in fns[entry][1]]
        is_ptr = ["*" in a for a in fns[entry][1]]
        base = {a: (valid[a] if a in valid else (_addr(a) if p else None)) for a, p in zip(args, is_ptr)}
        base["stream"] = None
        missing = [a for a, v in base.items() if v is None and a not in ("stream", "floor_row")]
        assert not missing, (entry, missing)

        def call(label, **over):
            unknown = set(over) - set(args)
            assert not unknown, (entry, label, unknown)
            return entry, label, [over.get(a, base[a]) for a in args]

        for f in faults:
            if f[0] == "null":
                for p in f[1].split():
                    yield call(f"{p}=NULL", **{p: None})
            elif f[0] == "odd":
                for p in f[1].split():
                    yield call(f"{p}+1", **{p: base[p] + 1})
            elif f[0] == "set":
                for v in f[2]:
                    label = f"{f[1]}=need-1" if isinstance(v, tuple) else f"{f[1]}={v}"
                    if isinstance(v, tuple):              # ("ws", query, args): one byte below what the query asks for
                        v = getattr(lib, v[1])(*v[2]) - 1
                        assert v > 0, (entry, label)
                    over = {f[1]: v}
                    for ld in WIDTHS.get(f[1], ()):
                        if ld in base and isinstance(base[ld], int) and v > base[ld]:
                            over[ld] = v
                    yield call(label, **over)
            else:
                yield call(f[1], **f[2])


def _run(lib):
    rows = []
    for entry, label, args in _cases(lib):
        rc = getattr(lib, entry)(*args)
        rows.append([entry, label, rc, lib.dp_last_error_string().decode() if rc else ""])
    return rows


def _differences(rows, golden_rows):
    want = {(e, c): (rc, msg) for e, c, rc, msg in golden_rows}
    got = {(e, c): (rc, msg) for e, c, rc, msg in rows}
    return [(k, got.get(k), want.get(k)) for k in sorted(set(want) | set(got)) if got.get(k) != want.get(k)]


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        pytest.skip("argument-refusal table runs only where no GPU is visible (host addresses stand in for device ones)")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_refusals_only(golden):
    assert "parent commit" in golden["header"]
    assert golden["rows"] and all(rc in (INVALID, UNSUPPORTED) and msg for _, _, rc, msg in golden["rows"])
    assert len({(e, c) for e, c, _, _ in golden["rows"]}) == len(golden["rows"])
    assert {e for e, _, _, _ in golden["rows"]} == set(_table())


def test_every_refusal_keeps_its_code_and_message(lib, golden):
    rows = _run(lib)
    assert all(rc in (INVALID, UNSUPPORTED) for _, _, rc, _ in rows), [r for r in rows if r[2] not in (INVALID, UNSUPPORTED)]
    assert _differences(rows, golden["rows"]) == []
    # negative control: one altered message is found
    bent = [list(r) for r in golden["rows"]]
    bent[len(bent) // 2][3] += "."
    assert len(_differences(rows, bent)) == 1


def test_workspace_queries_keep_their_sizes(lib, golden):
    sizes = _sizes(lib)
    assert sizes == golden["sizes"]
    assert any(v > 0 for v in sizes.values())
    for n in N_GRID:                          # a lone graph is the batch of one
        for K in K_GRID:
            single = sizes[f"dp_csr_linkpred_workspace_bytes({n},{K})"]
            assert single > 0 and single == sizes[f"dp_csr_linkpred_batch_workspace_bytes([0,{n}],1,{K})"]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    lib_ = _lib.load()
    rows_ = _run(lib_)
    let_through = [r for r in rows_ if r[2] not in (INVALID, UNSUPPORTED)]
    for r in let_through:
        print("NOT A REFUSAL (table error, not recorded):", r)
    if let_through:
        sys.exit(1)
    with open(GOLDEN, "w") as f_:
        json.dump({"header": "recorded from the library of the parent commit (the tree before the one-checked-body "
                             "refactor of the CSR entries) with tests/test_csr_entry_args_cpu.py --record; "
                             "rows: [entry, case, rc, message]",
                   "rows": rows_, "sizes": _sizes(lib_)}, f_, indent=0)
    print(f"recorded {len(rows_)} rows from {_lib.LIB_PATH}")
