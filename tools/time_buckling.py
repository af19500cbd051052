#!/usr/bin/env python3
"""Times the device buckling pass (pl_buckling, pl_buckling_pnorm) on the 50^3 Octet lattice of
bench.py beside its yardstick, pl_stress_pnorm in the same run: the stress pass streams a superset of the operands (the same
record, segment lengths, radius, connectivity and node rows; it writes four station values per strut where the buckling
pass writes one utilisation).  One process, one GPU; one warm-up and --reps timed repetitions per row.  Kernel times are HIP
events around the launches of one call (the library prints them when PL_TIMING is set), wall times are taken around the
Python call, which includes the transfers of the outputs to the host.

    python tools/time_buckling.py --out profiles/r10_buckling
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["PL_TIMING"] = "1"

from time_stress import _summary, _timed                               # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

RATIOS = (("value only", "pl_buckling_pnorm value only (p = 8)", "pl_stress_pnorm value only (p = 8, where = 1)"),
          ("with derivatives", "pl_buckling_pnorm with dbp_du, dbp_dr (p = 8)",
           "pl_stress_pnorm with dphi_du, dphi_dr (p = 8, where = 1)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r10_buckling")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=50)
    ap.add_argument("--geom", default="Octet")
    a = ap.parse_args()
    n = a.cells
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": n, "y": n, "z": n},
                                 "radii": [0.05], "geom_types": [a.geom]},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})
    lat = L.lattice
    dev = L.device_model()
    dev.set_bc(L.fixed_DOF)
    dev.assemble()
    u = np.random.default_rng(0).standard_normal((lat.n_nodes, 6)) * 1e-3
    rows = {"pl_buckling (util + n_axial + n_crit)": lambda: dev.buckling(u),
            RATIOS[0][1]: lambda: dev.buckling_pnorm(8, u, want_grad=False),
            RATIOS[1][1]: lambda: dev.buckling_pnorm(8, u),
            "pl_buckling_pnorm value only, Engesser, length = 0": lambda: dev.buckling_pnorm(8, u, length=0, shear=1, want_grad=False),
            RATIOS[0][2]: lambda: dev.stress_pnorm(8, u, where=1, want_grad=False),
            RATIOS[1][2]: lambda: dev.stress_pnorm(8, u, where=1)}
    res = {"lattice": f"{n}^3 {a.geom}", "n_nodes": int(lat.n_nodes), "n_beams": int(lat.n_beams), "reps": a.reps, "rows": {}}
    for name, fn in rows.items():
        walls, kernels = [], []
        for rep in range(a.reps + 1):
            w, k, _ = _timed(fn)
            if rep:
                walls.append(w)
                kernels.append(k)
        res["rows"][name] = {"wall": _summary(walls), "kernel_hip_events": _summary(kernels)}
    res["kernel_ratio_buckling_over_stress"] = {
        what: res["rows"][b]["kernel_hip_events"]["median_ms"] / res["rows"][s]["kernel_hip_events"]["median_ms"]
        for what, b, s in RATIOS}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; medians of {a.reps} warm repetitions"]
    for name, r in res["rows"].items():
        k = r["kernel_hip_events"]
        lines.append(f"  {name:58} wall {r['wall']['median_ms']:9.2f} ms" +
                     (f"   kernels (HIP events) {k['median_ms']:8.3f} ms" if k else ""))
    for what, ratio in res["kernel_ratio_buckling_over_stress"].items():
        lines.append(f"  kernel time, buckling / stress, {what}: {ratio:.3f}")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    dev.close()


if __name__ == "__main__":
    main()
