"""The prediction head's parameter gradients, written by the step's final launch (k_reduce_slabs_head,
csrc/dp_rowops.hip) when the head backward is folded into the last pooled level's kernel (k_small_level_bwd,
csrc/dp_small.hip).  The cases (tests/head_grads_final_cases.py) are the smallest shapes at which this code can go
wrong; each is checked three ways:

  (a) every gradient and ypred carry the same bits as the plan that keeps k_head_bwd (DP_NO_HEAD_FOLD=1, one child
      process for all cases: the knob is read once per process);
  (b) every gradient is within tests/parity.py's tolerance of the CPU oracle, run with the winners of the HIP forward's
      max readout, at a seed whose head pre-activations keep away from ReLU's kink;
  (c) three replays of a captured step carry the same bits as the eager step.

One kernel trace of the folded plan over all cases shows that the fold is really taken at these shapes: no k_head_bwd,
one k_small_level_bwd and one k_reduce_slabs_head per step, and no slab-only k_reduce_slabs."""
import csv
import functools
import glob
import os
import shutil
import subprocess
import sys

import pytest
import torch

from oracle import diffpool_oracle as O
from tests import head_grads_final_cases as HC
from tests.parity import close, grads_close, gpu_winners

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_head_grads_final_worker.py")
NAMES = [c[0] for c in HC.CASES]


def _env(no_fold):
    env = dict(os.environ)
    env.pop("DP_NO_HEAD_FOLD", None)
    if no_fold:
        env["DP_NO_HEAD_FOLD"] = "1"
    return env


@pytest.fixture(scope="module")
def separate(tmp_path_factory):
    """{case: {"ypred", gradients}} of the plan with k_head_bwd, computed once."""
    path = str(tmp_path_factory.mktemp("head_grads_final") / "separate.pt")
    r = subprocess.run([sys.executable, WORKER, path], env=_env(True), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    return torch.load(path)


@functools.lru_cache(maxsize=None)
def _eager(name):
    """The folded plan's step in this process: (results, winners of every level's max readout, loss)."""
    assert "DP_NO_HEAD_FOLD" not in os.environ, "this module tests the folded plan: unset DP_NO_HEAD_FOLD"
    model, _, x, adj, nn_, label = HC.build(name)
    model = model.cuda()
    y, loss = HC.step(model, x.cuda(), adj.cuda(), nn_, label.cuda())
    torch.cuda.synchronize()
    P = HC.CASE[name][5]
    return HC.results(model, y), gpu_winners(model, P + 1), loss.detach().cpu()


@functools.lru_cache(maxsize=None)
def _loose(name):
    return HC.atomic_bias_names(HC.build(name)[0])


def _same_bits(name, got, want, what):
    assert set(got) == set(want)
    loose = _loose(name)
    differ = [k for k in got if k not in loose and not torch.equal(got[k], want[k])]
    assert not differ, f"{what}: {differ}"
    for k in loose:
        assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-7), f"{what}: {k}"


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_as_the_plan_with_the_separate_head_kernel(name, separate):
    got = _eager(name)[0]
    assert torch.isfinite(got["ypred"]).all()
    _same_bits(name, got, separate[name], "folded plan against DP_NO_HEAD_FOLD=1")


@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_the_cpu_oracle(name):
    _, B, hidden, Cc, bn, P, seed = HC.CASE[name]
    got, win, loss = _eager(name)
    model, params, x, adj, nn_, label = HC.build(name)
    Pm = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo, inter = O.softpool_forward(Pm, x, adj, nn_, x, num_pooling=P, n_pred_hidden=len(hidden), bn=bn, winners=win)
    lo, _ = O.softpool_loss(yo, label)
    lo.backward()
    # a check of the CASE: no hidden unit of pred_model at ReLU's kink (tests/test_gpu_level0_phase0.py explains the margin)
    for i, pre in enumerate(HC.head_preactivations(params, inter["readout"].detach(), len(hidden))):
        assert float(pre.abs().min()) > 1e-5 * float(pre.abs().max()), \
            f"hidden layer {i} of the head sits on a ReLU kink ({float(pre.abs().min()):.3e}): choose another seed"
    close(got["ypred"], yo)
    close(loss, lo, 1e-4, 1e-6)
    for k, p_ in model.named_parameters():
        p_.grad = got[k]
    grads_close(model, {k: v.grad for k, v in Pm.items()})


@pytest.mark.parametrize("name", NAMES)
def test_three_replays_of_a_captured_step_equal_the_eager_step(name):
    want = _eager(name)[0]
    # a model of its own: no grad-accumulation node of an earlier eager step may be alive while the backward is captured
    model, _, x, adj, nn_, label = HC.build(name)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    nd = torch.from_numpy(nn_).cuda()                    # device num_nodes: no H2D inside the captured region
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            HC.step(model, xd, ad, nd, ld)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        y_static, _ = HC.step(model, xd, ad, nd, ld)
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        _same_bits(name, HC.results(model, y_static), want, f"replay {rep} against the eager step")
    del g


def test_the_folded_plan_is_taken_at_every_case(tmp_path):
    prof = shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    out = str(tmp_path / "trace")
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                        WORKER, str(tmp_path / "folded.pt")], env=_env(False), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, os.listdir(out)
    names = [row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))]
    count = {k: sum(k in nm for nm in names) for k in ("k_head_bwd", "k_small_level_bwd", "k_reduce_slabs_head")}
    count["k_reduce_slabs"] = sum("k_reduce_slabs" in nm and "k_reduce_slabs_head" not in nm for nm in names)
    assert count == {"k_head_bwd": 0, "k_small_level_bwd": len(NAMES), "k_reduce_slabs_head": len(NAMES),
                     "k_reduce_slabs": 0}, count
