"""Every DP_* knob the library reads has a line in README.md's knob table and either a row of its own in the plan matrix
(tests/test_gpu_plan_matrix.py: the knob's plan against the CPU oracle) or a written reason in EXCLUDED.  A new knob
cannot arrive without a plan test, and no row can leave the matrix unnoticed."""
import glob
import os
import re

from tests import _plan_worker
from tests.test_gpu_plan_matrix import CASE_ORDER, MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_pooling_amd", "csrc")
API = os.path.join(CSRC, "dp_api.hip")

# knobs that select no alternate plan of the encoder, or whose plan has a test of its own
EXCLUDED = {
    "DP_NO_HEAD_FOLD": "its plan is held bit-identical to the folded head by tests/test_gpu_head_fold.py and checked "
                       "against fp64 at every edge of k_head_bwd by tests/test_gpu_head.py",
    "DP_GEMM_TRACE": "only writes a host-side log of the GEMM shapes; it selects no kernel",
    "DP_AGG_DEBUG": "read only in DP_STAMP diagnostic builds, where it ablates phases of the panel kernel on purpose "
                    "(timing only, wrong results)",
    "DP_TEST_BARRIER_FAIL": "test-only: makes the grid barriers give up; the give-up path is "
                            "tests/test_gpu_edge_cases.py::test_grid_barrier_give_up_is_reported_not_silent",
}


def _read(path):
    with open(path) as f:
        return f.read()


def _knobs_body(api_src):
    m = re.search(r"const Knobs& knobs\(\) \{(.*?)\n\}", api_src, re.S)
    assert m, "knobs() not found in dp_api.hip"
    return m.group(1)


def knobs_read(api_src, other_srcs=()):
    """{knob: 'num' | 'flag'}: the names knobs() reads (num(...) -> a value, getenv(...) != nullptr -> a switch), plus any
    getenv("DP_...") elsewhere in the sources (which would break the read-once contract, but is a knob all the same)."""
    out = {}
    for name in re.findall(r'num\("(DP_[A-Z0-9_]+)"', _knobs_body(api_src)):
        out[name] = "num"
    for src in (_knobs_body(api_src),) + tuple(other_srcs):
        for name in re.findall(r'getenv\("(DP_[A-Z0-9_]+)"\)', src):
            out.setdefault(name, "flag")
    return out


def library_knobs():
    api = _read(API)
    others = [_read(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
              if p != API]
    return knobs_read(api, others)


def readme_knobs():
    names = set()
    for line in _read(os.path.join(ROOT, "README.md")).splitlines():
        if line.startswith("| `DP_"):
            names |= set(re.findall(r"`(DP_[A-Z0-9_]+)", line.split("|")[1]))
    return names


def escape_hatches(api_src):
    """The knob sets the device-error texts tell a user to set (dp_api.hip device_error_text)."""
    m = re.search(r"device_error_text\(int mask\) \{(.*?)\n\}", api_src, re.S)
    assert m, "device_error_text() not found in dp_api.hip"
    body = re.sub(r'"\s*\n\s*"', "", m.group(1))          # join the adjacent string literals
    return {frozenset(re.findall(r"(DP_[A-Z0-9_]+)=1", s)) for s in re.findall(r"set (DP_[^);]*)", body)}


def uncovered(knobs, matrix, excluded):
    """What the matrix misses: a switch needs a row of its own, a valued knob two rows of its own with different values."""
    problems = []
    single = {}
    for row in matrix:
        if len(row.env) == 1:
            (k, v), = row.env.items()
            single.setdefault(k, set()).add(v)
    for k, kind in sorted(knobs.items()):
        if k in excluded:
            continue
        need = 2 if kind == "num" else 1
        if len(single.get(k, ())) < need:
            problems.append(f"{k} ({kind}): {len(single.get(k, ()))} row(s) of its own in the plan matrix, needs {need}")
    return problems


def test_every_knob_is_in_the_readme_table():
    missing = sorted(set(library_knobs()) - readme_knobs())
    assert not missing, f"knobs the library reads but README.md's table does not list: {missing}"


def test_every_knob_has_plan_matrix_rows_or_a_reason():
    knobs = library_knobs()
    assert not uncovered(knobs, MATRIX, EXCLUDED), uncovered(knobs, MATRIX, EXCLUDED)
    for k, why in EXCLUDED.items():
        assert k in knobs, f"EXCLUDED lists {k}, which the library no longer reads"
        assert len(why) > 20, k
        assert all(k not in row.env for row in MATRIX), f"{k} is both excluded and in the matrix"


def test_matrix_rows_are_well_formed():
    knobs = library_knobs()
    assert tuple(_plan_worker.CASES) == CASE_ORDER
    ids = [row.id for row in MATRIX]
    assert len(ids) == len(set(ids)), "duplicate rows"
    for row in MATRIX:
        assert row.env and set(row.env) <= set(knobs), f"{row.id}: sets a variable the library does not read"
        assert row.cases and set(row.cases) <= set(CASE_ORDER), row.id
        assert callable(row.check), row.id


def test_the_escape_hatch_of_the_device_error_text_is_a_matrix_row():
    hatches = escape_hatches(_read(API))
    assert hatches == {frozenset({"DP_NO_L0_PERSIST", "DP_NO_LEVEL_FUSION"})}, hatches
    rows = {frozenset(row.env) for row in MATRIX}
    for h in hatches:
        assert h in rows, f"no plan-matrix row runs the escape hatch {sorted(h)}"


def test_the_guard_notices_a_new_knob_and_a_removed_row():
    api = _read(API)
    body = _knobs_body(api)
    assert "DP_FOO" not in api
    fooled = api.replace(body, body + '\n        k.foo = getenv("DP_FOO") != nullptr;', 1)
    knobs = knobs_read(fooled)
    assert knobs["DP_FOO"] == "flag"
    assert any("DP_FOO" in p for p in uncovered(knobs, MATRIX, EXCLUDED))
    valued = api.replace(body, body + '\n        k.foo = (int)num("DP_FOO", 0);', 1)
    assert knobs_read(valued)["DP_FOO"] == "num"
    real = library_knobs()
    for i, row in enumerate(MATRIX):
        rest = MATRIX[:i] + MATRIX[i + 1:]
        hatch_kept = frozenset(row.env) not in {frozenset(r.env) for r in rest} and \
            frozenset(row.env) in escape_hatches(api)
        assert uncovered(real, rest, EXCLUDED) or hatch_kept, f"removing the row {row.id} goes unnoticed"
