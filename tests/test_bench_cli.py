"""bench.py's command line: a plain run is the headline only (set up, warm up, the timed steps, the
JSON line), `--full` adds the figures that take runs of their own, and `--dump-outputs DIR` writes what
the last timed step computed as float64 .npy files, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_options_are_there():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_dump_outputs_float64_and_whole_below_the_cap(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path), {"x": np.arange(6, dtype=np.float32).reshape(3, 2), "obj_val": 1.5})
    x = np.load(tmp_path / "x.npy")
    assert x.dtype == np.float64 and x.shape == (3, 2) and np.array_equal(x, np.arange(6).reshape(3, 2))
    assert np.load(tmp_path / "obj_val.npy").dtype == np.float64
    assert not (tmp_path / "sample_rows.npy").exists()


def test_dump_outputs_seeded_row_sample_above_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 1000)
    rows = 500
    x = np.arange(rows * 4, dtype=np.float64).reshape(rows, 4)
    obj = np.arange(rows, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "obj_val": obj})
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))
    assert total <= 8 * 1000
    idx = np.load(tmp_path / "a" / "sample_rows.npy").astype(int)
    assert len(idx) > 0 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "x.npy"), x[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obj_val.npy"), obj[idx])
    for f in os.listdir(tmp_path / "a"):             # a fixed sample: the same rows every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path, gpu_required):
    n, steps = 1024, 2
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--order", str(n), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["config"]["iterations_in_timed_region"] == steps
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert "full_solve" not in line["config"] and line["cpu_baseline"]["value"] is None
    x = np.load(out / "x.npy")
    assert x.dtype == np.float64 and x.shape == (n,) and np.all(np.isfinite(x))
    for name in ("obj_val", "g", "mult_g", "mult_x_L", "mult_x_U"):
        assert np.load(out / (name + ".npy")).dtype == np.float64
