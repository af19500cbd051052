"""Exact cell Schur complements: pl_schur per cell (one PCG solve per boundary dof) against ONE pl_schur_cells launch.

Part 1 - for BCC, Hybrid1 and BCC + Hybrid1 + Hybrid4 cells at n_inst = 1, 125, 1 000 random radius sets: the per-cell
path (pl_schur on a handle per cell, timed on up to 8 cells and scaled to n_inst) and the batched path split into host
preparation (penalised segments of every radius set, get_schur_complements_batch's own loop), upload, kernel (launch +
synchronise) and download (the library's PL_TIMING stage marks).
Part 2 - LatticeOpti in exact DDM mode on a 3 x 3 x 3 triple-hybrid lattice (81 radius parameters, every cell its own
radius set): seconds per objective + gradient with the per-cell path (before) and the batched one (after).

Usage: python tools/time_schur_cells.py [--out FILE] [--skip-opti]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pylatticedso_amd import _capi                                            # noqa: E402
from pylatticedso_amd import lattice_arrays as LA                             # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                           # noqa: E402
from pylatticedso_amd.utils_schur import node_order_to_simulate               # noqa: E402


def _cell(geoms, radii):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": list(radii), "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": True}})


class _Stages:
    """The library's PL_TIMING lines ("[pl_schur_cells] <stage> <ms> ms" on stderr) of the calls inside the block."""

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
            if line.startswith("[pl_schur_cells]"):
                parts = line.split()
                self.ms[parts[1]] = self.ms.get(parts[1], 0.0) + float(parts[2])
        self._f.close()


def part1(rng):
    rows = []
    from dataclasses import replace
    for geoms in (["BCC"], ["Hybrid1"], ["BCC", "Hybrid1", "Hybrid4"]):
        L = _cell(geoms, [0.03] * len(geoms))
        lat = L.lattice
        order = node_order_to_simulate(L, 0)
        # per-cell path: pl_schur on a handle of the cell (what get_schur_complement did), warm-up first
        per = []
        for k in range(9):
            t0 = time.perf_counter()
            dev = _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, L.penalized.seg_len,
                                   L.penalized.seg_nsub, L.young_modulus, L.poisson_ratio, precond=5)
            dev.assemble()
            dev.schur(order, rtol=1e-13, max_iter=200000)
            dev.close()
            if k:
                per.append(time.perf_counter() - t0)
        per_cell_s = float(np.median(per))
        for n in (1, 125, 1000):
            radii = rng.uniform(0.01, 0.1, size=(n, len(geoms)))
            _capi.schur_cells(lat.node_xyz, lat.beam_conn, order, lat.beam_radius, L.penalized.seg_len,
                              L.penalized.seg_nsub, L.young_modulus, L.poisson_ratio)       # warm-up (module load)
            t0 = time.perf_counter()
            rad = radii[:, lat.beam_type]
            slen, nsub = [], []
            for r in rad:
                lr = replace(lat, beam_radius=r)
                pen = LA.penalize(lr, LA.compute_lzone(lr, True))
                slen.append(pen.seg_len)
                nsub.append(pen.seg_nsub)
            slen, nsub = np.stack(slen), np.stack(nsub)
            t1 = time.perf_counter()
            with _Stages() as st:
                S, info = _capi.schur_cells(lat.node_xyz, lat.beam_conn, order, rad, slen, nsub, L.young_modulus,
                                            L.poisson_ratio)
            t2 = time.perf_counter()
            assert (info == 0).all()
            row = {"cell": "+".join(geoms), "nodes": lat.n_nodes, "struts": lat.n_beams, "boundary": len(order),
                   "n_inst": n, "pl_schur_per_cell_ms": 1e3 * per_cell_s, "pl_schur_total_s": per_cell_s * n,
                   "batch_host_prep_ms": 1e3 * (t1 - t0), "batch_call_ms": 1e3 * (t2 - t1),
                   "batch_validate_ms": st.ms.get("validate", 0.0), "batch_upload_ms": st.ms.get("upload", 0.0),
                   "batch_kernel_ms": st.ms.get("kernel", 0.0), "batch_download_ms": st.ms.get("download", 0.0)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def part2():
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
    rng = np.random.default_rng(3)
    fits = _capi.schur_cells_fits
    for label, force_per_cell in (("before_per_cell_pl_schur", True), ("after_batched", False)):
        _capi.schur_cells_fits = (lambda *a: False) if force_per_cell else fits
        try:
            L = LatticeOpti(preset)
            n = L.number_parameters
            times, objs = [], []
            for k in range(3):
                x = list(rng.uniform(0.3, 0.7, size=n))
                t0 = time.perf_counter()
                objs.append(L.objective(x))
                L.gradient(x)
                times.append(time.perf_counter() - t0)
            out[label] = {"parameters": n, "s_per_objective_plus_gradient": times, "median_s": float(np.median(times)),
                          "objectives": objs}
        finally:
            _capi.schur_cells_fits = fits
        print(json.dumps({label: out[label]}), flush=True)
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
