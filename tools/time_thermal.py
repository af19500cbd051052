#!/usr/bin/env python3
"""Times the thermal load gather (pl_thermal_load) on the 50^3 Octet lattice of bench.py beside its
yardstick, k_stress_gather of pl_stress_pnorm in the same run: both walk the same sliced-ELL incidence, one thread per node.
One process, one GPU; one warm-up and --reps timed repetitions per row.  Kernel times are HIP events around the launches of one
call (the library prints them when PL_TIMING is set; the last line of a call is the stage that ends it).  k_stress_gather has
no stage of its own: it is the difference of pl_stress_pnorm with (dphi_du, dphi_dr) and with dphi_dr alone.  Run the tool
under `rocprofv3 --kernel-trace --stats` for the per-kernel times themselves.

    python tools/time_thermal.py --out profiles/r17_thermal
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["PL_TIMING"] = "1"

from time_stress import _summary, _timed                               # noqa: E402
from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r17_thermal")
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
    rng = np.random.default_rng(0)
    u = np.ascontiguousarray((rng.standard_normal((lat.n_nodes, 6)) * 1e-3).ravel())
    lib, p = dev._lib, _capi._ptr
    f, du = np.empty(6 * lat.n_nodes), np.empty(6 * lat.n_nodes)
    n_free, dr = np.empty(lat.n_beams), np.empty(lat.n_beams)
    phi = C.c_double()

    def pnorm(with_du):
        assert lib.pl_stress_pnorm(dev._h, p(u), 1, 8.0, C.byref(phi), None, p(du) if with_du else None, p(dr)) == 0

    def load(with_f):
        assert lib.pl_thermal_load(dev._h, p(f) if with_f else None, p(n_free)) == 0

    rows = {"pl_stress_pnorm with dphi_dr (no thermal state)": lambda: pnorm(False),
            "pl_stress_pnorm with dphi_du, dphi_dr (no thermal state)": lambda: pnorm(True)}
    res = {"lattice": f"{n}^3 {a.geom}", "n_nodes": int(lat.n_nodes), "n_beams": int(lat.n_beams), "reps": a.reps, "rows": {}}

    def run(rows):
        for name, fn in rows.items():
            walls, kernels = [], []
            for rep in range(a.reps + 1):
                w, k, _ = _timed(fn)
                if rep:
                    walls.append(w)
                    kernels.append(k)
            res["rows"][name] = {"wall": _summary(walls), "kernel_hip_events": _summary(kernels)}

    run(rows)
    dev.set_thermal(7e-5, 40.0 + 10.0 * (2.0 * rng.random(lat.n_nodes) - 1.0))
    run({"pl_thermal_load, n_free only (k_thermal_strut)": lambda: load(False),
         "pl_thermal_load, f_th and n_free (last stage: k_thermal_load)": lambda: load(True),
         "pl_thermal_sens (last stage: k_thermal_sens)": lambda: dev.thermal_sens(u),
         "pl_stress_pnorm with dphi_du, dphi_dr (thermal state; last stage: the pass)": lambda: pnorm(True)})
    k = {name: r["kernel_hip_events"]["median_ms"] for name, r in res["rows"].items()}
    res["k_stress_gather_ms_by_difference"] = (k["pl_stress_pnorm with dphi_du, dphi_dr (no thermal state)"] -
                                               k["pl_stress_pnorm with dphi_dr (no thermal state)"])
    # what the gather has to move: a 64-byte record and 8 bytes of delta per strut visit (two visits per strut), the
    # 8-byte incidence entry of the visit, and six doubles written per node
    res["k_thermal_load_model_bytes"] = int(2 * lat.n_beams * (64 + 8 + 8) + 48 * lat.n_nodes)
    t = k["pl_thermal_load, f_th and n_free (last stage: k_thermal_load)"]
    res["k_thermal_load_model_GB_per_s"] = res["k_thermal_load_model_bytes"] / (t * 1e-3) / 1e9
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; medians of {a.reps} warm repetitions"]
    for name, r in res["rows"].items():
        kk = r["kernel_hip_events"]
        lines.append(f"  {name:76} wall {r['wall']['median_ms']:9.2f} ms" +
                     (f"   last stage (HIP events) {kk['median_ms']:8.4f} ms" if kk else ""))
    lines.append(f"  k_stress_gather by difference: {res['k_stress_gather_ms_by_difference']:.4f} ms")
    lines.append(f"  k_thermal_load: {res['k_thermal_load_model_bytes']} model bytes, "
                 f"{res['k_thermal_load_model_GB_per_s']:.0f} GB/s at the measured time")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    dev.close()


if __name__ == "__main__":
    main()
