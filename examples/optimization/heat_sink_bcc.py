"""A small BCC block as a heat sink: its base face Zmin is held at a hot temperature and every strut gives heat to the ambient
air through its surface (lumped convection).  The design maximises the dissipated power under the volume
bound, with a bound on the temperature of the free nodes (the p-norm of T - T_inf over them).  Conduction grows with r^2 and
the film with r, so thick struts near the base carry the heat up and the rest of the volume is spent on surface.  Only the
conduction problem is solved at each design - one pl_cond_solve for the state, one adjoint solve per gradient.  The example
prints the gradient beside central differences at three variables and the objective history."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 8
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {
        "enable": True, "material": "VeroClear", "periodicity": False,
        "thermal": {"alpha": 7e-5,
                    "conduction": {"conductivity": 0.2, "reference": 20.0,
                                   "Temperature": {"Base": {"Surface": ["Zmin"], "Value": 90.0}},
                                   "Convection": {"film": 0.05, "ambient": 20.0}}}},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"], "Value": [0] * 6}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "max", "objective_type": "heat_dissipation", "max_iterations": iters,
        "optimization_parameters": {"type": "unit_cell"},
        "constraints": {"relative_density": {"value": 0.05}, "max_temperature": {"limit": 11.5, "p": 8}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}

L = LatticeOpti(preset)
theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
L.objective(theta)
g = np.asarray(L.gradient(theta))
rows = []
for i in (0, 5, 11):
    tp, tm = list(theta), list(theta)
    tp[i] += 1e-4
    tm[i] -= 1e-4
    rows.append({"variable": i, "gradient": float(g[i]), "central_difference": (L.objective(tp) - L.objective(tm)) / 2e-4})
L.redefine_optim_parameters(max_iteration=iters, disp=False)
sol = L.optimize_lattice()
print(json.dumps({"parameters": L.number_parameters, "gradient_check": rows, "iterations": int(sol.nit),
                  "dissipated_power_history": [float(v) for v in L._history["objective"]],
                  "peak_temperature_rise_history": L._history["max_temperature"],
                  "dissipated_power_last": float(L.dissipated_power()),
                  "max_temperature_constraint_last": float(L.max_temperature_constraint(sol.x)),
                  "relative_density": L.relative_density()}, indent=1))
