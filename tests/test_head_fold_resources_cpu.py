"""Register / scratch budget of the pooled-level backward kernel with the prediction-head backward folded in
(csrc/dp_small.hip, SmallHeadFold), read offline from the gfx950 code object of the built library
(tools/kernel_resources.py; needs the ROCm LLVM tools, no GPU).  The kernel runs 1024 threads, one workgroup per CU:
a spill would be a scratch round trip on the step's critical path."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")


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


def test_small_level_backward_with_the_head_fold_does_not_spill():
    res = KR.kernel_resources(LIB)
    d = [v for v in res.values() if v["name"] == "k_small_level_bwd"]
    assert len(d) == 1, sorted(v["name"] for v in res.values())
    d = d[0]
    assert d["vgpr_spills"] == 0, d
    assert d["scratch"] == 0, d
    assert d["vgprs"] <= 128, d           # 16 waves per CU: four per SIMD, 128 VGPRs each
    assert d["code_bytes"] <= 32 * 1024, d
