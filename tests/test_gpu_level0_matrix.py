"""The persistent level-0 kernels (csrc/dp_level0.hip: k_level0_fwd / k_level0_bwd) at every depth, width, register slot,
BatchNorm combine slot, cluster tier, block size and extent of tests/level0_cases.py, anchored to fp64, and the per-phase
sequence on the shapes one step outside each edge of their envelope.  Per case, in this process:

  - the launches of the pair are counted (dp_profile_level0) and must be [1, 1], [1, 0] or [0, 0] as level0_cases.plan
    predicts for THIS device's CU count; for [1, 1] the backward's rows per workgroup and its per-graph symmetric-form
    verdicts (dp_level0_bwd_symmetric) are the predicted ones: all 1 for a symmetric 0/1 batch, 0 for the graph with a
    directed edge alone, all 0 for weights bf16 cannot hold;
  - check (i): level 0's saved outputs against fp64, and the recorded winners of every level against the fp64 maxima;
  - check (ii): ypred, the loss and every parameter gradient against the fp64 loss with those winners forced;
    both at max(8 e_ref, 16 * 2^-24 * max|ref|), e_ref the error of the same graph in fp32 torch on the CPU;
  - a second identical step is torch.equal to the first on every output and gradient (bias gradients the per-phase
    sequence sums with float atomics: rtol 1e-5 / atol 1e-7, named by rule in level0_cases.loose_names);
  - the evaluation-mode forward is torch.equal to the training forward;
  - the device error word reads 0.

Every figure is printed ("[level0] ...") before it is asserted.  DP_L0_ANCHOR_OUT=<file> appends one line per case and
tensor (profiles/level0_fp64_anchor.txt is the digest of such a file, made by
`python -m tests.level0_cases --digest <file> profiles/level0_fp64_anchor.txt`)."""
import os

import pytest
import torch

from graph_pooling_amd import _lib
from tests import level0_cases as LC
from tests.test_gpu_level0 import _Counted

pytestmark = pytest.mark.gpu

LAUNCHES = {"pp": [1, 1], "pg": [1, 0], "gg": [0, 0]}
_STATE = {"device_error": None}      # set by the first case that ends with a device error: no later case touches the GPU


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same_bits(got, want, loose, what):
    assert set(got) == set(want)
    differ = [k for k in got if k not in loose and not torch.equal(got[k], want[k])]
    assert not differ, f"{what}: {differ}"
    for k in loose:
        assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-7), f"{what}: {k}"


@pytest.mark.parametrize("name,kind", LC.VARIANTS, ids=LC.IDS)
def test_level0_against_fp64(name, kind):
    assert not [k for k in os.environ if k.startswith("DP_") and k not in ("DP_LIB", "DP_L0_ANCHOR_OUT")], \
        "this module tests the no-knob plan"
    if _STATE["device_error"]:
        pytest.fail(f"not run: {_STATE['device_error']}")
    try:
        _case(name, kind)
    except RuntimeError as e:            # a HIP error is sticky: every later launch would fail, or worse
        _STATE["device_error"] = f"{name}-{kind} ended with {type(e).__name__}: {str(e)[:200]}"
        raise


def _case(name, kind):
    c = LC.CASE[name]
    want = LC.plan(c, _cus())
    model, params, x, ax, adj, nn_, label = LC.build(name, kind)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    axd = xd if ax is x else ax.cuda()
    runs = []
    for rep in range(2):
        with _Counted() as cnt:
            y, loss = LC.step(model, c, xd, axd, ad, nn_, ld)
        got = LC.results(model, c, y, loss)
        print(f"[level0] {name}-{kind} step {rep}: launches {cnt.n}, predicted {want['plan']} at {want['rows']} rows "
              f"({_cus()} CUs; the table at 256: {c.plan} {c.rows})")
        assert cnt.n == LAUNCHES[want["plan"]], \
            f"persistent level-0 kernels launched {cnt.n} times (forward, backward): the plan is {want['plan']}"
        if want["plan"] == "pp":
            verdicts, rows = _lib.level0_bwd_symmetric()
            assert rows == want["rows"], f"the backward used {rows} rows per workgroup, the geometry says {want['rows']}"
            if c.fam == "P":
                assert verdicts == LC.expected_verdicts(c, kind), (kind, verdicts)
        runs.append(got)
    first = runs[0]
    assert all(torch.isfinite(v).all() for v in first.values() if v.is_floating_point())
    rows = LC.figures(name, kind, first)
    for check, k, err, e_ref, bound, scale in rows:
        print(f"[level0] {name}-{kind} ({check}) {k}: error {err:.3e} e_ref {e_ref:.3e} ratio "
              f"{err / e_ref if e_ref else float('nan'):.2f} bound {bound:.3e} max|ref| {scale:.3e}")
    LC.record(name, kind, want["plan"], rows)
    bad = LC.failures(rows)
    assert not bad, f"{name}-{kind} against fp64: " + "; ".join(bad)
    _same_bits(runs[1], first, LC.loose_names(c, model, want["plan"], _cus()), "the second identical step")
    with _Counted() as cnt, torch.no_grad():
        y_eval = LC.forward(model, c, xd, axd, ad, nn_)
    assert cnt.n == [LAUNCHES[want["plan"]][0], 0]
    assert torch.equal(y_eval.cpu(), first["ypred"]), "the evaluation-mode forward differs from the training forward"
    dev_err = _lib.load().dp_device_error(0)
    assert dev_err == 0, f"device error word {dev_err:#x}"
