"""Register / scratch / code budget of the persistent level-0 forward (csrc/dp_level0.hip, k_level0_fwd<1..4>) with the
layer-0 product run under the adjacency burst: the adjacency quads (4 * MI registers x 4) stay live across the product, so a
spill would land on the step's critical path.  Read offline from the gfx950 code object of the built library
(tools/kernel_resources.py; needs the ROCm LLVM tools, no GPU).  The figures to hold are those of the build before the
reorder: no instantiation may use more scratch, <3> (the flagship's) has none, and the code may not grow by more than
2 KiB (scheduling differences: the change adds no product, it moves one)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")

# tools/kernel_resources.py on the library built from the parent commit
PARENT = {
    "k_level0_fwd<1>": {"code_bytes": 57028, "scratch": 0},
    "k_level0_fwd<2>": {"code_bytes": 65256, "scratch": 0},
    "k_level0_fwd<3>": {"code_bytes": 73868, "scratch": 0},
    "k_level0_fwd<4>": {"code_bytes": 81804, "scratch": 80},
}
CODE_MARGIN = 2 * 1024


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KR = _tool()
pytestmark = [
    pytest.mark.skipif(not KR.tools_available(), reason="ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, "
                                                        "llvm-readelf) not found"),
    pytest.mark.skipif(not os.path.exists(LIB), reason="libdiffpool_hip.so not built (graph_pooling_amd/csrc/build.sh)"),
]


@pytest.fixture(scope="module")
def fwd():
    by_name = {d["name"]: d for d in KR.kernel_resources(LIB).values() if d["name"].startswith("k_level0_fwd<")}
    assert sorted(by_name) == sorted(PARENT), sorted(by_name)
    return by_name


@pytest.mark.parametrize("name", sorted(PARENT))
def test_no_more_scratch_and_no_more_than_2k_of_code_over_the_parent(fwd, name):
    d = fwd[name]
    assert d["scratch"] <= PARENT[name]["scratch"], d
    assert 0 < d["code_bytes"] <= PARENT[name]["code_bytes"] + CODE_MARGIN, d


def test_the_flagship_instantiation_has_no_spill_and_no_scratch(fwd):
    d = fwd["k_level0_fwd<3>"]
    assert d["vgpr_spills"] == 0, d
    assert d["scratch"] == 0, d
