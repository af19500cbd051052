"""Deviations behind the bounds of tests/test_gpu_node_words.py: for every case of its iterate-equality test, the relative L2
deviation of u_1, u_2, u_3 and of the full solve between TWO runs of the switch-off path (PL_NODE_WORDS=0), and between the
switch-on and a switch-off run.  Prints one line per case and the maxima per precision; the bound is ten times the off / off
maximum.  usage: python tools/measure_node_words.py [repeats of the off / off pair, default 2]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402

import test_gpu_node_words as T   # noqa: E402
from oracle import precond_cases as C   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
worst = {p: {"off": np.zeros(4), "on": np.zeros(4)} for p in (0, 1)}
for name, precision, tm in T.CASES:
    for bset in C.BOUNDARY_SETS:
        try:
            base = T._solves(name, precision, tm, bset, False)
        except Exception as e:                      # (a case that cannot be built: say so and go on)
            print(f"MEASURE lattice={name} precision={precision} tile_modes={tm} set={bset} NOT BUILT: {e!r}", flush=True)
            continue
        off = np.zeros(4)
        for _ in range(reps):
            again = T._solves(name, precision, tm, bset, False)
            off = np.maximum(off, [T._rel(a[0], b[0]) for a, b in zip(again, base)])
        on_runs = T._solves(name, precision, tm, bset, True)
        on = np.array([T._rel(a[0], b[0]) for a, b in zip(on_runs, base)])
        worst[precision]["off"] = np.maximum(worst[precision]["off"], off)
        worst[precision]["on"] = np.maximum(worst[precision]["on"], on)
        print(f"MEASURE lattice={name} precision={precision} tile_modes={tm} set={bset} "
              f"off/off={' '.join(f'{d:.3e}' for d in off)} on/off={' '.join(f'{d:.3e}' for d in on)} "
              f"its={on_runs[-1][1]['iterations']}/{base[-1][1]['iterations']} info={on_runs[0][2]}", flush=True)
for p in (0, 1):
    for k in ("off", "on"):
        print(f"MAX precision={p} {k}/off u_1 u_2 u_3 full = {' '.join(f'{d:.3e}' for d in worst[p][k])}")
