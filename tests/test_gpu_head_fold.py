"""The prediction-head backward folded into the last pooled level's whole-level backward kernel (csrc/dp_small.hip,
SmallHeadFold): every gradient and ypred must be bit-identical to the plan that keeps k_head_bwd (DP_NO_HEAD_FOLD=1,
read once when the library loads, so that side runs in a child process), reproducible run to run, and a captured step
must replay the folded plan: k_small_level_bwd runs and k_head_bwd does not."""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one training step of a bench.py workload; writes {"ypred", parameter gradients} with torch.save
_STEP = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import bench
w = bench.WORKLOADS[sys.argv[2]]
model, batch, _ = bench.make_model_and_batch(w, False, torch.device("cuda"))
out = {}
for rep in range(2):
    model.zero_grad(set_to_none=True)
    y = model(batch["x"], batch["adj"], batch["nn"], assign_x=batch["x"])
    model.loss(y, batch["label"]).backward()
torch.cuda.synchronize()
out["ypred"] = y.detach().cpu()
for name, p in model.named_parameters():
    out[name] = p.grad.detach().cpu()
torch.save(out, sys.argv[3])
"""


def _step(workload, tmp_path, tag, no_fold):
    env = dict(os.environ)
    env.pop("DP_NO_HEAD_FOLD", None)
    if no_fold:
        env["DP_NO_HEAD_FOLD"] = "1"
    path = str(tmp_path / f"{workload}_{tag}.pt")
    r = subprocess.run([sys.executable, "-c", _STEP, ROOT, workload, path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return torch.load(path)


# enzymes_p3's level 1 has an assignment stack, so it runs the generic per-layer kernels, whose bias gradients are
# float-atomic sums (last-place differences between runs of ANY plan); those are compared to rounding
ATOMIC_BIAS = {"enzymes_p3": ("conv_first_after_pool_0.bias", "conv_block_after_pool_0.0.bias",
                              "conv_last_after_pool_0.bias", "assign_conv_first_1.bias", "assign_conv_block_1.0.bias",
                              "assign_conv_last_1.bias")}


@pytest.mark.parametrize("workload", ["dd", "enzymes_p3"])
def test_head_fold_is_bit_identical_to_the_separate_head_kernel(workload, tmp_path):
    folded = _step(workload, tmp_path, "fold", False)
    separate = _step(workload, tmp_path, "sep", True)
    assert set(folded) == set(separate)
    loose = ATOMIC_BIAS.get(workload, ())
    differ = [k for k in folded if k not in loose and not torch.equal(folded[k], separate[k])]
    assert not differ, differ
    for k in loose:
        assert torch.allclose(folded[k], separate[k], rtol=1e-5, atol=1e-7), k
    assert torch.isfinite(folded["ypred"]).all()


def test_head_fold_is_bit_reproducible_run_to_run(tmp_path):
    a = _step("dd", tmp_path, "a", False)
    b = _step("dd", tmp_path, "b", False)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ


def _trace_counts(tmp_path, extra_env, workload="dd"):
    """Kernel launches of a short captured bench.py run under the kernel trace: {kernel name fragment: count}."""
    prof = shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    out = tempfile.mkdtemp(dir=str(tmp_path))
    env = dict(os.environ)
    env.pop("DP_NO_HEAD_FOLD", None)
    env.update(extra_env)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                        os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--workload", workload],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, os.listdir(out)
    names = [row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))]
    return {k: sum(k in nm for nm in names) for k in ("k_head_bwd", "k_small_level_bwd", "k_head_fwd")}


def test_captured_step_replays_the_folded_head(tmp_path):
    folded = _trace_counts(tmp_path, {})
    # every step (warm-up, capture, replays) ran the pooled-level backward, and none the separate head backward
    assert folded["k_small_level_bwd"] >= 6 and folded["k_head_fwd"] >= 6, folded
    assert folded["k_head_bwd"] == 0, folded
    separate = _trace_counts(tmp_path, {"DP_NO_HEAD_FOLD": "1"})
    assert separate["k_head_bwd"] == separate["k_small_level_bwd"] >= 6, separate


def test_enzymes_p3_takes_the_folded_head(tmp_path):
    # the bit-identity test above means something at this shape only if the fold is really taken there
    folded = _trace_counts(tmp_path, {}, "enzymes_p3")
    assert folded["k_small_level_bwd"] >= 6 and folded["k_head_bwd"] == 0, folded

