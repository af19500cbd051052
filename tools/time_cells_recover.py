"""Cell recovery (pl_cells_recover) and the analytic exact-DDM gradient it makes possible.

Part 1 - kernel time (HIP events around the launch, the library's PL_TIMING "kernel_hip_event" line) and whole-call time of pl_cells_recover
for 1 000 and 32 768 instances of the BCC + Hybrid1 + Hybrid4 cell and of the plain BCC cell (u and lam recovered, sens on),
beside pl_schur_cells on the same 1 000 instances.
Part 2 - LatticeOpti in exact DDM mode on the 3 x 3 x 3 triple-hybrid lattice of tools/time_schur_cells.py: seconds per
objective + gradient with ddm_gradient = "finite_difference" (the parent commit's path, 1 + 2 G condensations per
representative) and "analytic" (one condensation + one recovery), for a unit_cell design (27 representatives) and a
constant hybrid one (1 representative).

Usage: python tools/time_cells_recover.py [--out FILE] [--skip-opti]"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pylatticedso_amd import _capi                                            # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                           # noqa: E402
from pylatticedso_amd.utils_schur import node_order_to_simulate               # noqa: E402


def _cell(geoms, radii):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": list(radii), "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": True}})


class _Stages:
    """The library's PL_TIMING lines ("[<call>] <stage> <ms> ms" on stderr) of the calls inside the block."""

    def __init__(self, call):
        self.tag = f"[{call}]"

    def __enter__(self):
        os.environ["PL_TIMING"] = "1"
        sys.stderr.flush()
        self._f = tempfile.TemporaryFile(mode="w+")
        self._saved = os.dup(2)
        os.dup2(self._f.fileno(), 2)
        self.ms = {}
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self._saved, 2)
        os.close(self._saved)
        os.environ.pop("PL_TIMING", None)
        self._f.seek(0)
        for line in self._f:
            if line.startswith(self.tag):
                parts = line.split()
                self.ms[parts[1]] = self.ms.get(parts[1], 0.0) + float(parts[2])
        self._f.close()


def part1(rng, reps=5):
    rows = []
    for geoms in (["BCC", "Hybrid1", "Hybrid4"], ["BCC"]):
        L = _cell(geoms, [0.03] * len(geoms))
        lat, pen = L.lattice, L.penalized
        order = node_order_to_simulate(L, 0)
        for n in (1000, 32768):
            rad = lat.beam_radius[None, :] * rng.uniform(0.5, 1.5, size=(n, 1))
            ub, lb = rng.standard_normal((n, 6 * len(order))), rng.standard_normal((n, 6 * len(order)))
            args = (lat.node_xyz, lat.beam_conn, order, rad, pen.seg_len, pen.seg_nsub)
            kern = {"pl_cells_recover": [], "pl_schur_cells": []}
            call = {"pl_cells_recover": [], "pl_schur_cells": []}
            for k in range(reps + 1):                       # (first round: module load, not kept)
                with _Stages("pl_cells_recover") as st:
                    t0 = time.perf_counter()
                    out = _capi.cells_recover(*args, ub, L.young_modulus, L.poisson_ratio, lam_b=lb)
                    t1 = time.perf_counter()
                assert (out["info"] == 0).all()
                if k:
                    kern["pl_cells_recover"].append(st.ms.get("kernel_hip_event", 0.0))
                    call["pl_cells_recover"].append(1e3 * (t1 - t0))
                if n > 1000:                                # (S of 32 768 triple-hybrid instances is 6 GB on the host)
                    continue
                with _Stages("pl_schur_cells") as st2:
                    t2 = time.perf_counter()
                    _, info = _capi.schur_cells(*args, L.young_modulus, L.poisson_ratio)
                    t3 = time.perf_counter()
                assert (info == 0).all()
                if k:
                    kern["pl_schur_cells"].append(st2.ms.get("kernel_hip_event", 0.0))
                    call["pl_schur_cells"].append(1e3 * (t3 - t2))
            row = {"cell": "+".join(geoms), "nodes": lat.n_nodes, "struts": lat.n_beams, "boundary": len(order),
                   "n_inst": n, "reps": reps}
            for name in kern:
                if not kern[name]:
                    continue
                row[name + "_kernel_ms"] = float(np.median(kern[name]))
                row[name + "_kernel_ms_per_1000"] = float(np.median(kern[name])) * 1000.0 / n
                row[name + "_call_ms"] = float(np.median(call[name]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def part2(reps=5):
    from pylatticedso_amd.lattice_opti import LatticeOpti
    preset = {
        "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 3, "z": 3},
                     "radii": [0.03, 0.03, 0.03], "geom_types": ["BCC", "Hybrid1", "Hybrid4"]},
        "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                  "DDM": {"enable_preconditioner": False, "max_iterations": 5000,
                                          "schur_complement_computation": {"type": "exact"}}},
        "boundary_conditions": {
            "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                       "Value": [0, 0, 0, 0, 0, 0]}},
            "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}},
        "optimization_informations": {
            "objective_function": "min", "objective_type": "compliance", "max_iterations": 5,
            "optimization_parameters": {"type": "unit_cell", "hybrid": True},
            "constraints": {"relative_density": {"value": 0.05}},
            "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "DDM"}}
    out = {}
    for design in ("unit_cell", "constant"):
        p = copy.deepcopy(preset)
        p["optimization_informations"]["optimization_parameters"]["type"] = design
        res = {}
        for mode in ("finite_difference", "analytic"):
            rng = np.random.default_rng(3)
            L = LatticeOpti(p, ddm_gradient=mode)
            n = L.number_parameters
            times, grads = [], []
            for k in range(reps + 1):
                x = list(rng.uniform(0.3, 0.7, size=n))
                t0 = time.perf_counter()
                L.objective(x)
                grads.append(np.asarray(L.gradient(x)))
                if k:
                    times.append(time.perf_counter() - t0)
            res[mode] = {"parameters": n, "representatives": int(L.schur_complements.shape[0]),
                         "s_per_objective_plus_gradient": times, "median_s": float(np.median(times))}
            res[mode + "_last_gradient"] = grads[-1]
        a, f = res.pop("analytic_last_gradient"), res.pop("finite_difference_last_gradient")
        res["gradient_rel_difference"] = float(np.linalg.norm(a - f) / np.linalg.norm(f))
        out[design] = res
        print(json.dumps({design: res}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-opti", action="store_true")
    a = ap.parse_args()
    res = {"cells": part1(np.random.default_rng(1))}
    if not a.skip_opti:
        res["latticeopti_exact_ddm_3x3x3_triple_hybrid"] = part2()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
