#!/usr/bin/env python3
"""Times the device stress pass (pl_stress, pl_stress_pnorm) on the 50^3 Octet lattice of bench.py
beside the path it replaces: HipLattice.records() (every 64-byte record to the host) + the numpy pass
exportSimulationResults._section_forces.  One process, one GPU; one warm-up and --reps timed repetitions per row.
Kernel times are HIP events around the launches of one call (the library prints them when PL_TIMING is set), wall times
are taken around the Python call, which includes the transfers of the outputs to the host.

    python tools/time_stress.py --out profiles/r09_stress
"""
import argparse
import importlib.util
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["PL_TIMING"] = "1"

from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import FullScaleLatticeSimulation  # noqa: E402


def _timed(fn):
    """(wall ms, kernel ms from the library's PL_TIMING line on stderr or None, result)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            out = fn()
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.findall(r"kernel_hip_event\s+([0-9.]+) ms", text)
    return wall, (float(m[-1]) if m else None), out


def _summary(ms):
    ms = [m for m in ms if m is not None]
    return {"min_ms": min(ms), "median_ms": float(np.median(ms)), "max_ms": max(ms), "all_ms": ms} if ms else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r09_stress")
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
    model = FullScaleLatticeSimulation(L, dev)
    model.u = u
    spec = importlib.util.spec_from_file_location(
        "export_simulation_results", os.path.join(ROOT, "src", "pyLatticeSim", "export_simulation_results.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ex = mod.exportSimulationResults(model, "time_stress", out_dir=tempfile.gettempdir())
    rows = {"pl_stress (station + peak)": lambda: dev.stress(u),
            "pl_stress_pnorm value only (p = 8)": lambda: dev.stress_pnorm(8, u, want_grad=False),
            "pl_stress_pnorm with dphi_du, dphi_dr (p = 8)": lambda: dev.stress_pnorm(8, u),
            "records() download": lambda: dev.records(),
            "records() + numpy _section_forces": lambda: ex._section_forces(u)}
    res = {"lattice": f"{n}^3 {a.geom}", "n_nodes": int(lat.n_nodes), "n_beams": int(lat.n_beams), "reps": a.reps, "rows": {}}
    for name, fn in rows.items():
        walls, kernels = [], []
        for rep in range(a.reps + 1):
            w, k, _ = _timed(fn)
            if rep:
                walls.append(w)
                kernels.append(k)
        res["rows"][name] = {"wall": _summary(walls), "kernel_hip_events": _summary(kernels)}
    # streaming cost of the operands of one station pass: record 64 B + segment lengths 24 B + radius 8 B + two node rows
    # 96 B (cached across the struts of a node) + connectivity 8 B read, 160 B stations + 8 B peak written
    res["station_pass_bytes_per_strut"] = 64 + 24 + 8 + 96 + 8 + 160 + 8
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; medians of {a.reps} warm repetitions"]
    for name, r in res["rows"].items():
        k = r["kernel_hip_events"]
        lines.append(f"  {name:48} wall {r['wall']['median_ms']:9.2f} ms" +
                     (f"   kernels (HIP events) {k['median_ms']:8.3f} ms" if k else ""))
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    dev.close()


if __name__ == "__main__":
    main()
