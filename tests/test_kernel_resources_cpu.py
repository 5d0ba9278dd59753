"""Register / scratch / code-size budget of the persistent level-0 kernels at the DD shape (MI = 3), read offline from
the gfx950 code object of the built library (tools/kernel_resources.py; needs the ROCm LLVM tools, no GPU).

Both kernels run 512 threads, one workgroup per CU, so each wave has 256 VGPRs: at that cap every spill reload is a
scratch round trip inside a latency-bound phase chain.  The budget: no VGPR spills, no scratch, and no
instantiation larger than it was before the aggregation bodies were cut down."""
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

# code bytes of every instantiation before this budget was set: none may grow back past them
CODE_BEFORE = {"k_level0_fwd<1>": 72392, "k_level0_fwd<2>": 85388, "k_level0_fwd<3>": 100304, "k_level0_fwd<4>": 112144,
               "k_level0_bwd<1>": 64076, "k_level0_bwd<2>": 76880, "k_level0_bwd<3>": 92064, "k_level0_bwd<4>": 102484}
SCRATCH_BEFORE = {"k_level0_fwd<1>": 0, "k_level0_fwd<2>": 0, "k_level0_fwd<3>": 92, "k_level0_fwd<4>": 248,
                  "k_level0_bwd<1>": 0, "k_level0_bwd<2>": 32, "k_level0_bwd<3>": 228, "k_level0_bwd<4>": 420}


@pytest.fixture(scope="module")
def level0():
    res = KR.kernel_resources(LIB)
    by_name = {d["name"]: d for d in res.values() if d["name"].startswith("k_level0_")}
    assert set(by_name) == set(CODE_BEFORE), sorted(by_name)
    return by_name


@pytest.mark.parametrize("name", ["k_level0_fwd<3>", "k_level0_bwd<3>"])
def test_dd_level0_kernels_do_not_spill(level0, name):
    d = level0[name]
    assert d["vgpr_spills"] == 0, d
    assert d["scratch"] == 0, d
    assert d["vgprs"] <= 256, d


def test_dd_level0_backward_fits_the_instruction_cache(level0):
    assert level0["k_level0_bwd<3>"]["code_bytes"] <= 64 * 1024, level0["k_level0_bwd<3>"]


@pytest.mark.parametrize("name", sorted(CODE_BEFORE))
def test_no_level0_instantiation_grows(level0, name):
    d = level0[name]
    assert 0 < d["code_bytes"] <= CODE_BEFORE[name], d
    assert d["scratch"] <= SCRATCH_BEFORE[name], d


def test_demangled_names():
    assert KR.demangle_short("_ZN2dp12_GLOBAL__N_112k_level0_fwdILi3EEEvNS0_6L0ArgsE") == "k_level0_fwd<3>"
    assert KR.demangle_short("_ZN2dp12_GLOBAL__N_112k_level0_bwdILi4EEEvNS0_7L0BArgsE") == "k_level0_bwd<4>"
