"""Register / scratch / code budget of the two kernels that share the prediction head's backward, read offline from the
gfx950 code object of the built library (tools/kernel_resources.py; needs the ROCm LLVM tools, no GPU):

  k_small_level_bwd  runs 1024 threads, one workgroup per CU, on the step's dependent chain: no VGPR spill, no scratch,
                     at most 128 VGPRs (16 waves per CU), and -- having lost the head poll and the head's dW / db loop to
                     the final launch -- no more code than it had with them: 25 908 bytes before, 21 772 after.  (Its
                     SGPR-to-VGPR-lane spills, no memory traffic, fell from 105 to 87 and may not rise above 105.)
  k_reduce_slabs_head  the step's final launch in the folded-head plan, whose extra workgroups hold 2 x 32 loaded operands
                     per thread before the adds: no spill of either kind and no scratch;
  k_reduce_slabs     the slab-only kernel every other plan keeps launching: as lean as it was (16 VGPRs at most, so
                     that two of its 1024-thread workgroups share a CU when there are more tiles than CUs)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")
SMALL_LEVEL_BWD_CODE_BEFORE = 25908          # bytes, with the head poll and the dW / db loop in the kernel
SMALL_LEVEL_BWD_SGPR_SPILLS_BEFORE = 105


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
def kernels():
    res = KR.kernel_resources(LIB)

    def one(name):
        d = [v for v in res.values() if v["name"] == name]
        assert len(d) == 1, sorted(v["name"] for v in res.values())
        return d[0]
    return one


def test_small_level_backward_does_not_spill_and_did_not_grow(kernels):
    d = kernels("k_small_level_bwd")
    assert d["vgpr_spills"] == 0, d
    assert d["scratch"] == 0, d
    assert d["vgprs"] <= 128, d
    assert d["sgpr_spills"] <= SMALL_LEVEL_BWD_SGPR_SPILLS_BEFORE, d
    assert d["code_bytes"] <= SMALL_LEVEL_BWD_CODE_BEFORE, d


def test_the_final_launch_does_not_spill(kernels):
    d = kernels("k_reduce_slabs_head")
    assert d["vgpr_spills"] == 0 and d["sgpr_spills"] == 0 and d["scratch"] == 0, d
    assert d["vgprs"] <= 128, d              # 1024 threads per workgroup
    d = kernels("k_reduce_slabs")
    assert d["vgpr_spills"] == 0 and d["sgpr_spills"] == 0 and d["scratch"] == 0, d
    assert d["vgprs"] <= 16, d
