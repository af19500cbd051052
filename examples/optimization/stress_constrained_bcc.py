"""Compliance of a small BCC cantilever under a volume bound, without and with a bound on the strut stresses: the
"max_stress" constraint of LatticeOpti (FEM mode) holds the p-norm of the von Mises stresses at the ends of every strut's
middle segment (pl_stress_pnorm) below s_allow; its gradient is the adjoint one (pl_sens with K lam = dPhi/du)."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "src"))
from pyLatticeOpti.lattice_opti import LatticeOpti      # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 1 else 4
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": nx, "y": 2, "z": 2},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": 60,
        "optimization_parameters": {"type": "linear", "direction": ["x"]},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}


def run(p):
    L = LatticeOpti(p)
    L.redefine_optim_parameters(disp=False)
    sol = L.optimize_lattice()
    L.objective(sol.x)
    return L, sol


free, sol0 = run(preset)
free.constraints_dict["max_stress"] = {"value": 1.0, "p": 8, "where": 1}
phi0 = free.stress_constraint(sol0.x) + 1.0                 # Phi_8 of the volume-constrained optimum
bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"]["max_stress"] = {"value": 0.95 * phi0, "p": 8, "where": 1}
con, sol1 = run(bounded)
print(json.dumps({"struts": free.lattice.n_beams, "s_allow": 0.95 * phi0,
                  "volume_only": {"x": list(map(float, sol0.x)), "compliance": free.compute_compliance(), "phi_8": phi0,
                                  "max_strut_stress": free.max_strut_stress(where=1)},
                  "volume_and_stress": {"x": list(map(float, sol1.x)), "compliance": con.compute_compliance(),
                                        "stress_constraint": con.stress_constraint(sol1.x),
                                        "max_strut_stress": con.max_strut_stress(where=1),
                                        "relative_density": con.relative_density()}}))
