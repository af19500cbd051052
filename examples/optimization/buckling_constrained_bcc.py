"""Compliance of a compressed BCC column under a volume bound, without and with a bound on the Euler buckling utilisation
of its struts: the "buckling" constraint of LatticeOpti (FEM mode) holds the p-norm of beta = max(0, -N) / N_cr over all
struts (pl_buckling_pnorm) below beta_allow; its gradient is the adjoint one (pl_sens with K lam = dB/du)."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "src"))
from pyLatticeOpti.lattice_opti import LatticeOpti      # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 4
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
column = {"p": 8, "length": 1, "k_eff": 1.0, "shear": 0}


def run(p):
    L = LatticeOpti(p)
    L.redefine_optim_parameters(disp=False)
    sol = L.optimize_lattice()
    L.objective(sol.x)
    return L, sol


free, sol0 = run(preset)
free.constraints_dict["buckling"] = dict(column, value=1.0)
b0 = free.buckling_constraint(sol0.x) + 1.0                  # B_8 of the volume-constrained optimum
bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"]["buckling"] = dict(column, value=0.95 * b0)
con, sol1 = run(bounded)
print(json.dumps({"struts": free.lattice.n_beams, "beta_allow": 0.95 * b0,
                  "volume_only": {"x": list(map(float, sol0.x)), "compliance": free.compute_compliance(), "b_8": b0,
                                  "max_strut_buckling": free.max_strut_buckling()},
                  "volume_and_buckling": {"x": list(map(float, sol1.x)), "compliance": con.compute_compliance(),
                                          "buckling_constraint": con.buckling_constraint(sol1.x),
                                          "max_strut_buckling": con.max_strut_buckling(),
                                          "relative_density": con.relative_density()}}))
