"""Compliance of a compressed 2 x 2 x 3 BCC column with a z-graded radius under a volume bound, without and with a lower
bound on its first natural frequency: the "frequency" constraint of LatticeOpti (FEM mode) holds
(2 pi f_min)^2 (sum_i (omega_i^2)^-p)^(1/p) - 1 <= 0 over the n_modes lowest frequencies of K phi = omega^2 M phi
(pl_vibration_modes, consistent strut mass), which keeps f_1 >= f_min; its gradient comes from pl_vibration_modes_sens in
one pass over the struts, without an adjoint solve.  Three modes hold whole clusters of this column: the double first
bending frequency and the simple torsional one."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 3
gain = float(sys.argv[2]) if len(sys.argv) > 2 else 1.1                 # f_min / f_1 of the volume-only optimum
density = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
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
modes = {"density": density, "n_modes": 3, "p": 8, "n_sub": 12}


def run(p):
    L = LatticeOpti(p)
    L.redefine_optim_parameters(disp=False)
    sol = L.optimize_lattice()
    L.objective(sol.x)
    return L, sol


def f_1(L, x):
    L.objective(x)
    return float(L.natural_frequencies(modes["n_modes"], density=density, n_sub=modes["n_sub"])["frequency"][0])


free, sol0 = run(preset)
before = f_1(free, sol0.x)
bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"]["frequency"] = dict(modes, value=gain * before)
con, sol1 = run(bounded)
after = f_1(con, sol1.x)
print(f"f_1 before: {before:.6g} Hz (volume bound only)   f_1 after: {after:.6g} Hz (f_min = {gain * before:.6g} Hz)")
print(json.dumps({"struts": free.lattice.n_beams, "f_min": gain * before,
                  "volume_only": {"x": list(map(float, sol0.x)), "compliance": free.compute_compliance(), "f_1": before,
                                  "relative_density": free.relative_density()},
                  "volume_and_frequency": {"x": list(map(float, sol1.x)), "compliance": con.compute_compliance(), "f_1": after,
                                           "frequency_constraint": con.frequency_constraint(sol1.x),
                                           "min_frequency_history": con._history["min_frequency"],
                                           "relative_density": con.relative_density()}}))
