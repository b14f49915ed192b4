"""bench.py's plain run: the result line it prints and what --dump-outputs writes.  Needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def _dumped(path):
    arrays = {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}
    assert arrays and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    assert all(np.isfinite(a).all() for a in arrays.values())
    return arrays


def test_plain_dense_line_and_outputs(tmp_path):
    out = str(tmp_path / "dense")
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--T", "16", "--dump-outputs", out)
    assert all(k in line for k in HEADLINE), line
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert not any(k in line for k in ("roofline", "variants", "value_spread", "cpu_baseline", "kernel_table"))
    a = _dumped(out)
    assert a["belief"].shape == (16, 256, 32)
    assert a["hidden_num_nodes"].tolist() == [16.0] * 256
    np.testing.assert_allclose(a["loss"], a["belief"].astype(np.float64).mean(), rtol=1e-5)
    assert any(k.startswith("grad_0_") for k in a)


def test_plain_sparse_line_and_outputs(tmp_path):
    out = str(tmp_path / "sparse")
    line = _bench("--gpus", "1", "--config", "cfg4", "--steps", "2", "--warmup", "1", "--dump-outputs", out)
    assert all(k in line for k in HEADLINE), line
    assert line["steps"] == 2 and "cfg4" in line["metric"] and "roofline" not in line
    a = _dumped(out)
    assert "out" in a and "loss" in a and any(k.startswith("grad_0_") for k in a)
