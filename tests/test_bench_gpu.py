"""bench.py's N = 1 line on a small grid: a plain run carries the headline and nothing that runs work of its own after
the timed steps; --full adds those legs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--size", "512", "--leadtimes", "4", "--steps", "2", "--warmup", "1"]
# what only --full runs: keys of the line, keys of line["config"]
FULL_KEYS = ("cpu_baseline",)
FULL_CONFIG_KEYS = ("host_path_ms", "spectral", "config4_one_gpu", "steps_loop", "steps_e2e")


def run_bench(*extra):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
                          cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert line["metric"] == "Mpixels*leadsteps/s (LK+semilag) at 512x512 fp32" and line["unit"] == "Mpx*leadsteps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(512 * 512 * 4 / (line["ms_per_step"] * 1e-3) / 1e6)
    assert line["lk_semilag_value"] == line["value"] and line["config"]["lk_in_step"] is True
    assert line["roofline"]["kernel_ms"] > 0 and line["config"]["lk_ms_per_step"] is not None
    return line


def test_plain_run_is_the_headline_alone(tmp_path):
    line = run_bench("--dump-outputs", str(tmp_path))
    for key in FULL_KEYS:
        assert key not in line, key
    for key in FULL_CONFIG_KEYS:
        assert key not in line["config"], key
    assert line["advection_value"] is None and line["member_loop_value"] is None
    # --dump-outputs still writes what the last timed step returned
    motion = np.load(tmp_path / "motion_field.npy")
    out = np.load(tmp_path / "extrapolated.npy")
    assert motion.shape == (2, 512, 512) and out.shape == (4, 512, 512) and out.dtype == np.float32
    assert np.isfinite(motion).all() and np.isfinite(out).any()


def test_full_run_adds_the_other_legs():
    line = run_bench("--full")
    for key in FULL_KEYS:
        assert key in line, key
    for key in FULL_CONFIG_KEYS:
        assert key in line["config"], key
    assert line["cpu_baseline"]["value"] > 0 and line["config"]["host_path_ms"] > 0
    assert line["advection_value"] > 0 and line["member_loop_value"] > 0
    # the --no-* switches still select among the legs
    line = run_bench("--full", "--no-cpu-baseline", "--no-spectral", "--no-steps-loop")
    assert "cpu_baseline" not in line and "spectral" not in line["config"] and "steps_loop" not in line["config"]
    assert "host_path_ms" in line["config"] and line["advection_value"] > 0
