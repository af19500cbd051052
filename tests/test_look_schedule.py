"""The look schedule of the PCG loops (pylatticedso_amd/csrc/pl_schedule.h): how many iterations the host queues before
it downloads the residual history again.  The device runs every chunk to its end, so the schedule decides which iterate the
ordinary form returns: the chunk sequences are pinned, not approximated.  A plain C++ program drives the header on a
synthetic history (slot i holds q^(i + 1), ||b||^2 = 1); the expected sequences were computed from the solver's formulas in
double precision, every ceil() argument at least 0.02 away from an integer.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pylatticedso_amd", "csrc", "pl_schedule.h")

PROGRAM = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s"

// argv: q rtol max_iter check_every extra last_iterations direct ref_cg stall_from(-1: none)
int main(int argc, char **argv) {
  if (argc != 10) return 2;
  const double q = std::atof(argv[1]), rtol = std::atof(argv[2]);
  const int max_iter = std::atoi(argv[3]), stall = std::atoi(argv[9]);
  auto slot = [&](int i) { return std::pow(q, (double)((stall >= 0 && i > stall ? stall : i) + 1)); };
  pl::LookParams lp;
  lp.check_every = std::atoi(argv[4]);
  lp.max_iter = max_iter;
  lp.target = rtol * rtol;
  lp.rr0 = 1.0;
  lp.extra = std::atoi(argv[5]);
  lp.last_iterations = std::atoi(argv[6]);
  lp.dd_ready = std::atoi(argv[7]) != 0;
  lp.ref_cg = std::atoi(argv[8]) != 0;
  pl::LookSchedule look(lp);
  int k = 0, largest = 0;
  while (k < max_iter) {
    const int todo = look.todo(k);
    if (todo <= 0 || todo > look.max_chunk()) return 3;
    largest = todo > largest ? todo : largest;
    std::printf("%%d ", todo);
    bool converged = false;
    for (int j = 0; j < todo; ++j) converged = converged || slot(k + j) <= lp.target;
    k += todo;
    if (converged) break;
    look.missed(k, slot(k - 1));
  }
  std::printf("\n");
  return 0;
}
'''

# defaults: adaptive, extra = 0, last_iterations = 0, not direct, not reference-CG, no stall
BASE = dict(q=0.91, rtol=1e-8, max_iter=1000, check_every=0, extra=0, last_iterations=0, direct=0, ref_cg=0, stall=-1)
CASES = [
    ("q080", dict(q=0.80), [32] * 4 + [28, 7, 2, 2]),
    ("q091", dict(), [32] * 11 + [29, 8, 2]),
    ("q091_extra1", dict(extra=1), [32] * 11 + [30, 8, 2]),
    ("q091_last391", dict(last_iterations=391), [388, 2, 2]),
    ("q091_last391_refcg", dict(last_iterations=391, ref_cg=1), [32] * 11 + [29, 8, 2]),
    ("q091_every10", dict(check_every=10), [10] * 40),
    ("q091_max100", dict(max_iter=100), [32, 32, 32, 4]),
    ("q005_direct", dict(q=0.05, direct=1), [2, 8, 2, 2]),
    ("q055_direct", dict(q=0.55, direct=1), [2, 32, 21, 5, 2]),
    ("q091_stall100", dict(stall=100), [32] * 31 + [8]),
    ("q097_rtol1e-6_extra1", dict(q=0.97, rtol=1e-6, max_iter=2000, extra=1), [32] * 28 + [10, 2]),
    ("q091_max1_direct", dict(max_iter=1, direct=1), [1]),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("look_schedule")
    src = d / "look.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = d / "look"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    return str(exe)


@pytest.mark.parametrize("name,over,expected", CASES, ids=[c[0] for c in CASES])
def test_chunk_sequence(program, name, over, expected):
    a = dict(BASE, **over)
    argv = [program] + [repr(a[k]) for k in ("q", "rtol", "max_iter", "check_every", "extra", "last_iterations", "direct",
                                             "ref_cg", "stall")]
    got = [int(v) for v in subprocess.check_output(argv, text=True).split()]
    assert got == expected, (name, got)


def test_header_stands_alone():
    """No HIP and nothing of the project behind it: a plain C++ program can use the schedule."""
    includes = [ln.split()[1] for ln in open(HEADER) if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
