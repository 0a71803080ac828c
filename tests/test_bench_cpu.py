"""bench.py on CPU: the --full / --dump-outputs options and the output dump's dtype and size budget."""
import numpy as np
import pytest
import torch

import bench


def test_full_is_off_by_default_and_steps_must_be_positive():
    assert not bench.parse([]).full and bench.parse(["--full"]).full
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_keeps_small_arrays_whole_and_their_dtype(tmp_path):
    arrays = {"loss": torch.tensor(2.5), "y": torch.randn(3, 5, generator=torch.Generator().manual_seed(0)).bfloat16(),
              "f64": torch.arange(4, dtype=torch.float64), "n": 7}
    assert bench.dump_outputs(str(tmp_path), arrays) == ["f64", "loss", "n", "y"]
    out = {n: np.load(tmp_path / f"{n}.npy") for n in arrays}
    assert out["loss"].shape == () and out["loss"].dtype == np.float32 and float(out["loss"]) == 2.5
    assert out["y"].dtype == np.float32 and np.array_equal(out["y"], arrays["y"].float().numpy())
    assert out["f64"].dtype == np.float64 and out["n"].dtype == np.float64 and float(out["n"]) == 7


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path):
    arrays = {"small": torch.arange(10, dtype=torch.float32), "big": torch.arange(5000, dtype=torch.float32).view(50, 100),
              "bigger": torch.arange(8000, dtype=torch.float64)}
    budget = 16000
    bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sum(v.nbytes for v in a.values()) <= budget
    assert np.array_equal(a["small"], np.arange(10))
    for n in ("big", "bigger"):
        v = a[n]
        assert v.ndim == 1 and 0 < v.size < arrays[n].numel()
        assert np.all(np.diff(v) > 0) and set(v) <= set(arrays[n].reshape(-1).tolist())   # sorted sample of the elements
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy"))                       # the same sample every time
