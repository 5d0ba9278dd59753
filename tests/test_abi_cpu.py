"""CPU checks of the drop-in boundary: the C-ABI library loads here (no GPU), exports every symbol
include/diffpool_hip.h declares, and the ctypes binding agrees with the header on every signature.
No compute call is made."""
import ctypes as C
import os
import re

import pytest

from graph_pooling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffpool_hip.h")


def _header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"typedef struct \{.*?\} \w+;", "", src, flags=re.S)
    src = "\n".join(l for l in src.splitlines() if not l.strip().startswith("#"))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(dp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        arglist = [] if args in ("void", "") else [a.strip() for a in args.split(",")]
        out[name] = (ret, arglist)
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    fns = _header_functions()
    assert len(fns) >= 30
    for name in fns:
        assert hasattr(lib, name), f"{name} declared in diffpool_hip.h but not exported by the .so"
    assert set(fns) == set(_lib.EXPORTED_SYMBOLS), set(fns) ^ set(_lib.EXPORTED_SYMBOLS)


def _kind(ctype_decl: str) -> str:
    d = ctype_decl.replace("const ", "").strip()
    if "*" in d:
        return "ptr"
    base = d.split()[0] if " " in d else d
    first = " ".join(d.split()[:-1]) if len(d.split()) > 1 else d
    for k in ("size_t", "long long", "long", "int", "float"):
        if first == k:
            return k
    return base


def test_ctypes_signatures_match_header(lib):
    fns = _header_functions()
    cmap = {C.c_int: "int", C.c_long: "long", C.c_float: "float", C.c_size_t: "size_t", C.c_void_p: "ptr",
            C.c_char_p: "ptr"}
    for name, (ret, args) in fns.items():
        res, argtypes = _lib._PROTOS[name]
        assert len(args) == len(argtypes), f"{name}: header has {len(args)} args, binding {len(argtypes)}"
        for i, (decl, ct) in enumerate(zip(args, argtypes)):
            kind = _kind(decl)
            got = "ptr" if (ct not in cmap) else cmap[ct]
            assert kind == got, f"{name} arg {i} ({decl!r}): header {kind}, binding {got}"


def test_version_and_error_string(lib):
    assert lib.dp_version() == 100
    assert isinstance(lib.dp_last_error_string(), bytes)
    assert lib.dp_sizeof_encoder_cfg() == C.sizeof(_lib.EncoderCfg)
    assert lib.dp_sizeof_gemm_problem() == C.sizeof(_lib.GemmProblem) == 112
    assert lib.dp_sizeof_row_groups() == C.sizeof(_lib.RowGroups) == 20
    assert lib.dp_sizeof_group_ptrs() == C.sizeof(_lib.GroupPtrs) == 24


def test_device_error_word_decode(lib):
    """diffpool_hip.h "Device-side failures": the text for every mask of the per-device error word, and a quiet read on
    a host without a GPU (no word can be set up: reads as 0, never crashes)."""
    assert lib.dp_device_error(0) == 0 and lib.dp_device_error(1) == 0
    none, bar = lib.dp_device_error_describe(0), lib.dp_device_error_describe(_lib.DEVERR_BARRIER)
    nonf, both = lib.dp_device_error_describe(_lib.DEVERR_NONFINITE_GRAD), lib.dp_device_error_describe(3)
    assert none == b"no device error"
    assert b"grid barrier gave up" in bar and b"DP_NO_LEVEL_FUSION" in bar and b"non-finite" not in bar
    assert b"non-finite gradient norm" in nonf and b"skipped the update" in nonf and b"barrier" not in nonf
    assert b"grid barrier gave up" in both and b"non-finite" in both
    # the escape hatch names BOTH knobs: DP_NO_LEVEL_FUSION alone leaves the persistent level-0 kernels and their
    # barriers in place (tests/test_gpu_plan_matrix.py runs the pair and finds no barrier kernel)
    for text in (bar, both):
        assert b"DP_NO_L0_PERSIST=1" in text and b"DP_NO_LEVEL_FUSION=1" in text, text
    assert b"unknown" in lib.dp_device_error_describe(64)


def test_argument_errors_are_reported_before_any_launch(lib):
    # NULL pointers / bad dims must come back as DP_ERR_INVALID_ARG with a message (no GPU needed)
    rc = lib.dp_bgemm_f32(None, None, None, None, 1, 4, 4, 4, 4, 4, 4, 0, 0, 0, 0, 0, 1.0, 0.0, 0, None)
    assert rc == -1 and b"NULL" in lib.dp_last_error_string()
    # a group entry answers before it looks at a pointer: a bad count, then NULL operands
    prob = (_lib.GemmProblem * 1)(_lib.GemmProblem(M=4, N=4, K=4, lda=4, ldb=4, ldc=4, alpha=1.0))
    plan = (C.c_int * 1)()
    assert lib.dp_bgemm_plan(prob, 5, 1, 1, plan) == -1 and b"count=5" in lib.dp_last_error_string()
    assert lib.dp_bgemm_plan(prob, 1, 1, 1, plan) == 0 and _lib.gemm_plan_decode(plan[0]) == (64, 16, 1, 1)
    assert lib.dp_bgemm_group_f32(prob, 1, 1, 1, None, 0, None) == -1 and b"NULL" in lib.dp_last_error_string()
    # the row launchers' pass-through entries and their plan query: a bad descriptor, then NULL operands
    g = _lib.RowGroups(G=2, c0=(C.c_int * 2)(0, 4), w=(C.c_int * 2)(8, 8))
    out = (C.c_int * _lib.ROWOP_PLAN_INTS)()
    assert lib.dp_rowop_plan(_lib.ROWOP_ROWNORM_FWD, C.byref(g), 4, 1, 0, 0, out) == -1
    assert b"overlap" in lib.dp_last_error_string()
    g.c0[1] = 8
    assert lib.dp_rowop_plan(_lib.ROWOP_ROWNORM_FWD, C.byref(g), 4, 1, 0, 0, out) == 0
    assert tuple(out) == (_lib.ROWK_ROWNORM_FWD, 2, 0, 0, 0, 0)
    for name in ("dp_rownorm_fwd", "dp_bn_apply_fwd", "dp_bn_bwd_partials", "dp_rownorm_bwd", "dp_softmax_mask_fwd",
                 "dp_softmax_mask_bwd", "dp_colsum_batched"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert lib.dp_colsum_batched(None, 8, 0, 4, 8, None, 8, 1, 1, None) == -1 and b"NULL" in lib.dp_last_error_string()
    rc = lib.dp_masked_max_fwd(1, 4, None, 1, 4, 1, 0, 3, 4, None)
    assert rc == -1 and b"B=0" in lib.dp_last_error_string()
    # the aggregation's plan query (host only) and its fused pass-through entry
    for name in ("dp_adj_aggregate_plan", "dp_adj_aggregate_rownorm", "dp_adj_pack_zero"):
        assert name in _lib.EXPORTED_SYMBOLS
    plan = (C.c_int * _lib.AGG_PLAN_INTS)()
    assert lib.dp_adj_aggregate_plan(20, 500, 40, 0, 0, 0, 0, 0.0, plan) == 0
    assert tuple(plan)[:6] == (_lib.AGG_FORM_PANEL_F32, 3, 32, 16, 320, 66048)
    assert lib.dp_adj_aggregate_plan(20, 500, 40, 0, 0, 0, 0, 0.0, None) == -1 and b"NULL" in lib.dp_last_error_string()
    # the link loss's plan query (host only): the pinned plans of five shapes, then its refusals
    assert "dp_linkpred_plan" in _lib.EXPORTED_SYMBOLS
    lp = (C.c_int * _lib.LINKPRED_PLAN_INTS)()
    for shape, want in (((20, 500, 50), (4, 64, 8, 4, 2)), ((1, 260, 256), (16, 32, 9, 9, 1)),
                        ((256, 128, 8), (1, 64, 2, 1, 2)), ((512, 64, 192), (12, 32, 2, 1, 2)),
                        ((30, 321, 20), (2, 64, 6, 3, 2))):
        assert lib.dp_linkpred_plan(*shape, lp) == 0 and tuple(lp)[:5] == want, (shape, tuple(lp))
    assert lib.dp_linkpred_plan(20, 500, 50, lp) == 0
    assert tuple(lp)[5:] == (64, 4 * (2 * 64 * 66 + 4), 4 * (128 * 66 + 64 * 68 + 64 * 65))
    assert lib.dp_linkpred_plan(20, 500, 257, lp) == -3 and b"K=257" in lib.dp_last_error_string()
    assert lib.dp_linkpred_plan(20, 500, 256, lp) == 0 and tuple(lp)[:2] == (16, 32)
    assert lib.dp_linkpred_plan(20, 500, 50, None) == -1 and b"NULL" in lib.dp_last_error_string()
    for bad in ((0, 500, 50), (20, 0, 50), (20, 500, 0), (-1, 500, 50)):
        assert lib.dp_linkpred_plan(*bad, lp) == -1 and b"must be positive" in lib.dp_last_error_string(), bad
    # the CSR link loss's plan query (host only): DD's largest graph at K = 50, an ENZYMES-sized one, the refusals
    assert "dp_csr_linkpred_plan" in _lib.EXPORTED_SYMBOLS
    cp = (C.c_int * _lib.CSR_LINKPRED_PLAN_INTS)()
    assert lib.dp_csr_linkpred_plan(5748, 50, 50, 50, 0, 0, cp) == 0
    assert tuple(cp) == (4, 90, 45, 23, 1035, 360, 64, 90, 6, 15, 1, 4, 1, 4, 4 * 2 * 64 * 66, 4 * (128 * 66 + 64 * 68))
    assert lib.dp_csr_linkpred_plan(126, 28, 28, 28, 0, 0, cp) == 0 and tuple(cp)[:4] + tuple(cp)[6:14] == (
        2, 2, 1, 2, 64, 2, 2, 1, 4, 1, 4, 1)
    assert lib.dp_csr_linkpred_plan(126, 28, 28, 30, 0, 0, cp) == 0 and tuple(cp)[10:14] == (4, 1, 1, 4)
    assert lib.dp_csr_linkpred_plan(126, 28, 28, 28, 1, 0, cp) == 0 and tuple(cp)[10:14] == (1, 4, 1, 4)
    assert lib.dp_csr_linkpred_plan(126, 257, 257, 257, 0, 0, cp) == -3 and b"K=257" in lib.dp_last_error_string()
    assert lib.dp_csr_linkpred_plan(126, 28, 28, 28, 0, 0, None) == -1 and b"NULL" in lib.dp_last_error_string()
    for bad, text in (((0, 28, 28, 28), b"must be positive"), ((126, 0, 28, 28), b"must be positive"),
                      ((126, 28, 27, 28), b"lds=27 smaller"), ((126, 28, 28, 27), b"ldds=27 smaller")):
        assert lib.dp_csr_linkpred_plan(*bad, 0, 0, cp) == -1 and text in lib.dp_last_error_string(), bad
    yp = _lib.GroupPtrs()
    rc = lib.dp_adj_aggregate_rownorm(None, None, None, None, None, 16, None, C.byref(g), None, C.byref(yp), None, None,
                                      1, 4, 1, 0, 0, None, 0, None)
    assert rc == -1 and b"NULL" in lib.dp_last_error_string()
    cfg = _lib.EncoderCfg()
    assert lib.dp_encoder_save_bytes(C.byref(cfg)) == 0          # invalid cfg -> 0 + message
    assert b"must be positive" in lib.dp_last_error_string()


def test_workspace_queries_run_without_gpu(lib):
    assert lib.dp_gcn_layer_workspace_bytes(4, 16, 3, 8) > 0
    # the link loss is tile-fused: its workspace is per-tile loss partials and [splits,B,N,K] gradient partials,
    # never a [B,N,N] temporary
    assert 0 < lib.dp_linkpred_workspace_bytes(20, 500, 50) < 20 * 500 * 500 * 4 // 2
    assert lib.dp_linkpred_workspace_bytes(256, 1024, 256) < 1 << 20          # big batches need no split
    assert lib.dp_bn_node_workspace_bytes(4, 16, 8) > 0
    # tickets: [batch][ksplit][M][N] partials and one counter per 16 x 16 block; no other split form needs any
    prob = (_lib.GemmProblem * 1)(_lib.GemmProblem(M=20, N=40, K=500, lda=500, ldb=40, ldc=40, alpha=1.0,
                                                   split=_lib.GEMM_TICKETS))
    assert lib.dp_bgemm_group_workspace_bytes(prob, 1, 3, 4) >= 4 * (3 * 4 * 20 * 40 + 3 * 2 * 3)
    assert lib.dp_bgemm_group_workspace_bytes(prob, 1, 3, 1) == 0
    prob[0].split = _lib.GEMM_SLABS
    assert lib.dp_bgemm_group_workspace_bytes(prob, 1, 3, 4) == 0


def test_product_has_no_cpu_fallback():
    """The modules must refuse CPU tensors instead of silently computing something else."""
    import torch
    from graph_pooling_amd.encoders import SoftPoolingGcnEncoder
    m = SoftPoolingGcnEncoder(16, 3, 8, 8, 2, 3, 8, assign_ratio=0.25, linkpred=False)
    x = torch.zeros(2, 16, 3)
    adj = torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        m(x, adj, [3, 4], assign_x=x)


def test_nothing_in_the_product_imports_the_oracle():
    pkg = os.path.join(ROOT, "graph_pooling_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                for line in open(os.path.join(dirpath, f)).read().splitlines():
                    assert not re.match(r"\s*(from|import)\s+\.*oracle", line), (f, line)
                    assert "diffpool_oracle" not in line, (f, line)
