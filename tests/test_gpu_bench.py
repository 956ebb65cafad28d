"""A plain `bench.py` run (no --full): the headline region alone, the contract's fields in the last line, and
--dump-outputs writing what the last timed step returned -- the same inputs, so the same forward output, in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3",
                        "--points", "20000", "--details", "", "--dump-outputs", out_dir], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_bench_line_and_dumped_outputs(mc, tmp_path):
    line, outs = _plain_run(str(tmp_path / "a"))
    assert line["steps"] == 6 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "points/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("MC-convolved points/sec")
    # nothing but the headline was measured
    for k in ("roofline", "cpu_baseline", "strong"):
        assert line[k] is None, k
    assert "layers" not in line and "configs" not in line
    assert outs["conv_out"].shape == (20000, 64) and outs["features_grad"].shape == (20000, 1)
    assert {"Conv_weights_grad", "Conv_biases_grad", "Conv_weights2_grad", "Conv_biases2_grad", "Conv_weights3_grad",
            "Conv_biases3_grad"} <= set(outs)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in outs.values())
    assert np.abs(outs["conv_out"]).max() > 0 and np.abs(outs["Conv_weights2_grad"]).max() > 0
    # a second process with the same arguments: the same inputs, the same (deterministic) forward output
    _, again = _plain_run(str(tmp_path / "b"))
    assert np.array_equal(again["conv_out"], outs["conv_out"])
    for k, a in outs.items():
        assert np.abs(again[k] - a).max() <= 1e-4 * max(np.abs(a).max(), 1e-30), k
