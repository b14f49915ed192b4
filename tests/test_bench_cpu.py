"""bench.py's host-side pieces: the options of a plain and a --full run, and how --dump-outputs turns what a
step returned into .npy arrays within its size budget.  No kernel is launched here."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_bench_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = p.stdout.decode()
    assert "--full" in text and "--dump-outputs" in text and "--steps" in text


def test_host_arrays_dtypes():
    idx = torch.tensor([[0, 1, 1], [2, 0, 2]])
    got = bench.host_arrays({"f32": torch.ones(2, 3), "f64": torch.ones(2, dtype=torch.float64),
                             "i64": torch.arange(4), "empty": torch.zeros(0),
                             "sp": torch.sparse_coo_tensor(idx, torch.tensor([1.0, 2.0, 3.0]), (2, 3))})
    assert sorted(got) == ["f32", "f64", "i64", "sp_indices", "sp_values"]
    assert got["f32"].dtype == np.float32 and got["f32"].shape == (2, 3)
    assert got["f64"].dtype == np.float64
    assert got["i64"].dtype == np.float64 and got["i64"].tolist() == [0, 1, 2, 3]
    assert got["sp_indices"].dtype == np.float64 and got["sp_indices"].shape == (2, 3)
    assert got["sp_values"].tolist() == [1.0, 2.0, 3.0]


def test_budget_keeps_small_sets_whole():
    arrays = {"a": np.arange(10, dtype=np.float32), "b": np.ones((4, 4), dtype=np.float64)}
    out, sampled = bench.budget_arrays(arrays)
    assert not sampled and all(out[k] is arrays[k] for k in arrays)


def test_budget_samples_large_sets_the_same_way_every_time():
    rng = np.random.default_rng(0)
    arrays = {"big": rng.standard_normal(3_000_000).astype(np.float32).reshape(3000, 1000),
              "big2": rng.standard_normal(2_000_000).astype(np.float32),
              "small": np.arange(100, dtype=np.float64)}
    budget = 8 * 10 ** 6
    out, sampled = bench.budget_arrays(arrays, budget=budget)
    assert sum(a.nbytes for a in out.values()) <= budget
    assert set(sampled) == {"big", "big2"} and out["small"] is arrays["small"]
    again, _ = bench.budget_arrays(arrays, budget=budget)
    for k in out:
        assert np.array_equal(out[k], again[k])
    # the sample is the flattened array at the seeded positions
    pos = bench.sample_index("big", arrays["big"].size, sampled["big"][1])
    assert np.array_equal(out["big"], arrays["big"].reshape(-1)[pos])
    assert len(np.unique(pos)) == len(pos)
