"""CPU checks of the Set2Set case table (tests/set2set_cases.py): through dp_set2set_plan — the host function both
launchers of dp_set2set.hip take their kernel variant from — the table reaches all five variants of k_set2set_fwd /
k_set2set_bwd and every edge of their loops, each case has a live (not all-zero) ReLU output, and the fp64 reference
tells a one-row error from rounding by two orders of magnitude at the bound test_gpu_set2set.py applies."""
import os

import pytest
import torch

from graph_pooling_amd import _lib
from oracle import diffpool_oracle as O
from tests import set2set_cases as SC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _forward64(emb, params):
    return O.set2set_forward(emb.double(), {k: v.double() for k, v in params.items()})


def test_plan_matches_the_launcher_arithmetic(lib):
    """The variant edges in d and n, stated independently of the table: weights stay in registers up to d = 64, in LDS
    up to d = 69; the embedding joins them in LDS while [n][d] fits beside them in 158 KiB."""
    plan = lib.dp_set2set_plan
    assert plan(100, 60) == SC.W_REGS | SC.E_LDS                 # the benchmark's enzymes_s2s shape
    assert plan(100, 64) == SC.W_REGS | SC.E_LDS and plan(40, 65) == SC.W_LDS | SC.E_LDS
    assert plan(16, 69) & SC.W_LDS and plan(16, 70) == 0
    assert plan(1000, 60) == SC.W_REGS and plan(1024, 40) == SC.W_REGS
    assert plan(1024, 256) == 0 and plan(1, 1) == SC.W_REGS | SC.E_LDS
    # [n][d] floats of embedding (beside the [2d][4d + 1] weights when those are in LDS) do not fit in 158 KiB
    for n, d, w_floats in ((600, 64, 0), (300, 66, 2 * 66 * (4 * 66 + 1))):
        assert 4 * (n * d + w_floats) > 158 * 1024 - 4 * (7 * d + 2 * n + 1100) and not plan(n, d) & SC.E_LDS
    # no instance stages the embedding beside weights read from global memory
    assert all(plan(n, d) == 0 for n in (1, 50, 1024) for d in (70, 128, 256))


def test_refusals(lib):
    for n, d in SC.REFUSED + [(0, 60), (100, 0), (-1, 60)]:
        assert lib.dp_set2set_plan(n, d) == SC.ERR_UNSUPPORTED, (n, d)
    assert (1025, 60) in SC.REFUSED and (100, 257) in SC.REFUSED


def test_table_reaches_every_variant(lib):
    seen = {}
    for (B, n, d) in SC.CASES:
        p = lib.dp_set2set_plan(n, d)
        assert p in SC.VARIANTS, f"n={n} d={d}: plan {p}"
        seen.setdefault(SC.VARIANTS[p], []).append((n, d))
    assert set(seen) == set(SC.VARIANTS.values()), f"variants without a case: {set(SC.VARIANTS.values()) - set(seen)}"
    # rows whose variant the issue's formulas give: assert what the query says
    assert lib.dp_set2set_plan(16, 69) == SC.W_LDS and lib.dp_set2set_plan(40, 65) == SC.W_LDS | SC.E_LDS
    assert lib.dp_set2set_plan(257, 60) == SC.W_REGS | SC.E_LDS and lib.dp_set2set_plan(600, 64) == SC.W_REGS


def test_table_contains_every_edge():
    ds = {d for _, _, d in SC.CASES}
    ns = {n for _, n, _ in SC.CASES}
    assert {64, 65, 69, 70, 128, 129, 256} <= ds and ds & {192, 193}
    assert {1, 256, 257, 1024} <= ns and any(n % 16 for n in ns)
    assert any((n, d) == (1000, 60) for _, n, d in SC.CASES)
    assert sum(n in (1000, 1024) for _, n, _ in SC.CASES) <= 2           # (the CPU reference time goes with n^2)
    assert 1 not in ds
    assert len(set(SC.CASES)) == len(SC.CASES) and all(B >= 1 for B, _, _ in SC.CASES)
    # the backward tail (rows >= 256) runs in a variant of each weight placement
    assert all(any(n > 256 and lo <= d <= hi for _, n, d in SC.CASES) for lo, hi in ((1, 64), (65, 69), (70, 256)))


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_case_output_is_not_all_zero(case):
    """At least a quarter of the fp64 reference outputs are positive: a case whose ReLU is shut checks no gradient."""
    emb, params, _ = SC.make_inputs(*case)
    with torch.no_grad():
        out = _forward64(emb, params)
    frac = float((out > 0).double().mean())
    print(f"{SC.case_id(case)}: positive outputs {frac:.2f}")
    assert frac >= 0.25, frac
    n = case[1]
    assert bool((emb[0, n - n // 3:] == 0).all()) and (n < 3 or bool((emb[0, :n - n // 3] != 0).any()))


def test_reference_sees_a_dropped_attention_row():
    """Sensitivity of the check at (n 1024, d 40): the fp64 reference with the LAST attention row left out of every
    step differs from the true reference by at least 100 x the largest bound test_gpu_set2set.py ever grants
    (1e-5 of the tensor's largest entry).  Measured when the test was written: 2.4e-3 of the largest output, all of it
    in graph 1, whose last row is a real node.  Graph 0's last row is a padded zero row: leaving it out only moves the
    softmax normalisation, 4e-5 — which is why the table gives the long cases a second, unpadded graph."""
    case = (2, 1024, 40)
    assert case in SC.CASES
    emb, params, _ = SC.make_inputs(*case)
    with torch.no_grad():
        e64, p64 = emb.double(), {k: v.double() for k, v in params.items()}
        true = _forward64(emb, params)
        same = SC.forward_drop_last_row(e64, p64, drop=False)
        dropped = SC.forward_drop_last_row(e64, p64, drop=True)
    assert float((same - true).abs().max()) <= 1e-12 * float(true.abs().max())     # the restatement is the oracle
    rel = float((dropped - true).abs().max()) / float(true.abs().max())
    print(f"one dropped attention row at n=1024, d=40: {rel:.3e} of the largest output")
    assert rel >= 100 * SC.ANCHOR_CAP, rel
