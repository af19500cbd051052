"""The objective of the response sensitivities and its derivative (csrc/pl_objective.h: the host arithmetic between the passes of
pl_transient_sens and pl_harmonic_sens) against its restatements dynamics_host.objective / harmonic_objective, at the edges
where such code goes wrong: all outputs zero, all weights zero, a zero weight on the largest output, a zero output at p = 2,
outputs near the overflow and underflow limits, a single row.  The driver tests/native/objective_cases.cpp is built with
AddressSanitizer + UndefinedBehaviorSanitizer and run once, as its own process, for all cases.  CPU only.

Tolerance: both sides are double-precision chains of fewer than ten roundings, amplified by at most p <= 32 in pow: under
1e-13 relative to the largest entry; 1e-12 is asserted.  Where the restatement gives J = 0 or a zero derivative the header must
give exactly that."""
import os
import subprocess

import numpy as np
import pytest

from pylatticedso_amd import dynamics_host as DH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "objective_cases.cpp")
RTOL = 1e-12


def _cases():
    """name -> (complex?, kind, p, y, weight or None)"""
    rng = np.random.default_rng(16)
    n = 7
    yr = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)
    yc = yr * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, n))
    w = rng.uniform(0.2, 2.0, n)
    out = {}
    for cx, y in ((False, yr), (True, yc)):
        t = "c" if cx else "r"
        top = int(np.abs(y).argmax())
        for kind, p in ((0, 8.0), (1, 8.0), (2, 2.0), (2, 8.0), (2, 32.0)):
            tag = f"{t}-kind{kind}" + (f"-p{p:g}" if kind == 2 else "")
            out[tag] = (cx, kind, p, y, None)
            out[tag + "-weights"] = (cx, kind, p, y, w)
            out[tag + "-outputs_zero"] = (cx, kind, p, 0.0 * y, w)
            out[tag + "-weights_zero"] = (cx, kind, p, y, 0.0 * w)
            w_top = w.copy()
            w_top[top] = 0.0
            out[tag + "-zero_weight_on_largest"] = (cx, kind, p, y, w_top)
            out[tag + "-single_row"] = (cx, kind, p, y[:1], None)
            out[tag + "-single_row-weights"] = (cx, kind, p, y[:1], w[:1])
            if kind == 2:      # finite only because of the scaling by the largest |y|
                out[tag + "-times_1e150"] = (cx, kind, p, 1e150 * y, w)
                out[tag + "-times_1e-150"] = (cx, kind, p, 1e-150 * y, w)
        y0 = y.copy()
        y0[(top + 1) % n] = 0.0
        out[f"{t}-kind2-p2-one_output_zero"] = (cx, 2, 2.0, y0, None)
        out[f"{t}-kind2-p2-one_output_zero-weights"] = (cx, 2, 2.0, y0, w)
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """name -> (J, derivative) of the header, from one run of the driver"""
    exe = str(tmp_path_factory.mktemp("objective") / "objective_cases")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip(f"this toolchain has no asan_ubsan runtime: {build.stderr[-200:]}")
    assert build.returncode == 0, build.stderr[-2000:]
    lines = []
    for cx, kind, p, y, w in CASES.values():
        flat = np.asarray(y, complex).view(float) if cx else np.asarray(y, float)
        nums = list(flat) + ([] if w is None else list(w))
        lines.append(f"{'c' if cx else 'r'} {kind} {p!r} {len(y)} {0 if w is None else 1} " + " ".join(repr(float(v)) for v in nums))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    rows = [np.array(line.split(), float) for line in run.stdout.splitlines()]
    assert len(rows) == len(CASES)
    return {name: (row[0], row[1:]) for name, row in zip(CASES, rows)}


@pytest.mark.parametrize("name", list(CASES))
def test_objective_header_matches_its_restatement(native, name):
    cx, kind, p, y, w = CASES[name]
    if cx:
        J_ref, g = DH.harmonic_objective(y, kind, p, w)
        d_ref = np.asarray(g, complex).view(float)
    else:
        J_ref, d_ref = DH.objective(y, kind, p, w)
    J, d = native[name]
    assert d.shape == d_ref.shape
    assert np.isfinite(J_ref) and np.isfinite(d_ref).all()
    print(f"{name}: J {J!r} ref {J_ref!r}  max|dd| {np.abs(d - d_ref).max()!r} of {np.abs(d_ref).max()!r}")
    if J_ref == 0.0:
        assert J == 0.0
    else:
        assert abs(J - J_ref) <= RTOL * abs(J_ref)
    if not d_ref.any():
        assert not d.any()
    else:
        assert np.abs(d - d_ref).max() <= RTOL * np.abs(d_ref).max()
