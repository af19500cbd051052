"""bench.py as the driver calls it: a plain run prints the headline line only, --steps sets the timed steps, and
--dump-outputs writes what the last timed step computed - the same numbers from run to run on the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config")
FULL_ONLY = ("roofline", "kernels_ms", "value_cold_first_look", "cpu_baseline", "end_to_end_s", "other_configs")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_and_dump(tmp_path):
    """12^3 Octet cantilever, 3 timed steps: the headline keys and nothing of --full; u and K*probe in float64, twice."""
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        line = _bench("--steps", "3", "--warmup", "1", "--cells", "12", "--dump-outputs", str(d))
        for key in HEADLINE:
            assert key in line, key
        assert not [key for key in FULL_ONLY if key in line]
        assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["config"]["converged"] == 1
        outs.append(_load(d))
    a, b = outs
    assert set(a) == {"u", "K_bsr_probe"}
    n = a["u"].shape[0]
    for name, arr in a.items():
        assert arr.dtype == np.float64 and arr.shape == (n, 6) and np.isfinite(arr).all(), name
    assert a["u"][:, 2].min() < 0.0                   # the cantilever is loaded in -Z
    for name in a:
        assert np.linalg.norm(a[name] - b[name]) <= 1e-10 * np.linalg.norm(b[name]), name


def test_design_loop_steps_and_dump(tmp_path):
    """configs[3] on an 8^3 lattice: --steps sets the design iterations; the last one's compliance, gradient, u and radii."""
    line = _bench("--config", "3", "--cells", "8", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and "roofline" not in line
    out = _load(tmp_path)
    assert set(out) == {"compliance", "gradient", "u", "radii"}
    assert out["compliance"].shape == (1,) and out["gradient"].shape == out["radii"].shape == (8 ** 3,)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in out.values())
    assert out["compliance"][0] == pytest.approx(line["config"]["compliance_first_last"][1], rel=1e-12)
