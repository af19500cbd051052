"""Compliance of a compressed 2 x 2 x 3 BCC column under a volume bound, without and with a bound on its global buckling
load: the "global_buckling" constraint of LatticeOpti (FEM mode) holds lambda_min (sum_i lambda_i^-p)^(1/p) - 1 <= 0 over the
n_modes smallest load factors of (K + lambda K_g(u)) phi = 0 (pl_buckling_modes), which keeps lambda_1 >= lambda_min; its
gradient comes from pl_buckling_modes_sens, adjoint for u(r) included.  The column buckles as a whole (lambda_1 = 2.21 at the
start) long before its first strut does (3.56 on its middle segment), so the strut check of buckling_constrained_bcc.py
does not see this limit."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 3
gain = float(sys.argv[2]) if len(sys.argv) > 2 else 1.1                 # lambda_min / lambda_1 of the volume-only optimum
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 2, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": 60,
        "optimization_parameters": {"type": "linear", "direction": ["z"]},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}
modes = {"n_modes": 4, "p": 8, "n_sub": 12}


def run(p):
    L = LatticeOpti(p)
    L.redefine_optim_parameters(disp=False)
    sol = L.optimize_lattice()
    L.objective(sol.x)
    return L, sol


def lambda_1(L, x):
    L.objective(x)
    return float(L.global_buckling(modes["n_modes"], n_sub=modes["n_sub"])["load_factor"][0])


free, sol0 = run(preset)
before = lambda_1(free, sol0.x)
bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"]["global_buckling"] = dict(modes, value=gain * before)
con, sol1 = run(bounded)
after = lambda_1(con, sol1.x)
print(f"lambda_1 before: {before:.6g} (volume bound only)   lambda_1 after: {after:.6g} (lambda_min = {gain * before:.6g})")
print(json.dumps({"struts": free.lattice.n_beams, "lambda_min": gain * before,
                  "volume_only": {"x": list(map(float, sol0.x)), "compliance": free.compute_compliance(),
                                  "lambda_1": before, "strut_load_factor_middle_segment": 1.0 / free.max_strut_buckling(),
                                  "relative_density": free.relative_density()},
                  "volume_and_global_buckling": {"x": list(map(float, sol1.x)), "compliance": con.compute_compliance(),
                                                 "lambda_1": after,
                                                 "global_buckling_constraint": con.global_buckling_constraint(sol1.x),
                                                 "min_load_factor_history": con._history["min_load_factor"],
                                                 "strut_load_factor_middle_segment": 1.0 / con.max_strut_buckling(),
                                                 "relative_density": con.relative_density()}}))
