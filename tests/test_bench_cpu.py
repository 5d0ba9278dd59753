"""bench.py's command line and its --dump-outputs writer: host-side, no GPU."""
import sys

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_ones(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE_ELEMS * 3 + 5, dtype=torch.float32)
    named = [("ypred", torch.randn(20, 2)), ("loss", torch.tensor(0.5)), ("pred_class", torch.tensor([1, 0, 1])),
             ("assign_tensor", big)]
    bench.dump_outputs(str(tmp_path / "a"), named)
    bench.dump_outputs(str(tmp_path / "b"), named)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["assign_tensor.sample.npy", "loss.npy", "pred_class.npy", "ypred.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "ypred.npy"), named[0][1].numpy())
    assert np.load(tmp_path / "a" / "pred_class.npy").dtype == np.float64
    s = np.load(tmp_path / "a" / "assign_tensor.sample.npy")
    assert s.shape == (bench.DUMP_SAMPLE_ELEMS,)
    assert np.all(np.diff(s) == 3)                      # a fixed stride through the flattened tensor


def test_dump_outputs_refuses_more_than_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), [("ypred", torch.zeros(26))])
    assert not any(tmp_path.iterdir())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_step_counts_that_time_nothing(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
