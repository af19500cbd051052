"""pylatticedso_amd/csrc/pl_nodeword.h (lever arms of the PCG vector kernels as three signed bytes: the search for the
exponent and the packing) under AddressSanitizer + UndefinedBehaviorSanitizer, through the stand-alone driver
tests/native/nodeword_main.cpp: exact round trip on dyadic inputs, the smallest exponent, refusal of 0.7-spaced inputs, of
magnitude 128 (127 is accepted), of -0.0 and of non-finite values.  CPU only, a few seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "nodeword_main.cpp")


def test_rel_byte_packing_under_sanitizers(tmp_path):
    exe = str(tmp_path / "nodeword_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert run.stdout.strip().endswith("OK")
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    # the question the GPU fall-back test asks: which one-aggregate lattice overflows a byte
    fits = subprocess.run([exe, "overflow", "40", "2", "2", "1.0"], capture_output=True, text=True, env=env, timeout=120)
    over = subprocess.run([exe, "overflow", "140", "2", "2", "1.0"], capture_output=True, text=True, env=env, timeout=120)
    assert (fits.returncode, fits.stdout.strip()) == (3, "fits 1") and (over.returncode, over.stdout.strip()) == (0, "overflow")
