"""A graded BCC lattice whose temperature is the solution of a conduction problem on its own struts: cold on Zmin, a heat inflow
on Zmax, clamped on Xmin and loaded on Xmax.  The temperature rise scales like 1 / r^2, so the thermal load depends on the design
twice - through the strut stiffness and through the temperature.  LatticeOpti's adjoint gradient carries both (the chain term
-mu^T dK_T/dr T of DESIGN.md section 10l: one extra scalar solve per gradient); the example prints it beside central
differences and beside the gradient that takes the temperature as fixed, then runs a few SLSQP iterations."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {
        "enable": True, "material": "VeroClear", "periodicity": False,
        "thermal": {"alpha": 7e-5,
                    "conduction": {"conductivity": 0.2, "reference": 20.0,
                                   "Temperature": {"Cold": {"Surface": ["Zmin"], "Value": 20.0}},
                                   "HeatFlow": {"Top": {"Surface": ["Zmax"], "Value": 1.5}}}}},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"], "Value": [0] * 6}},
        "Force": {"Load": {"Surface": ["Xmax", "Zmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": iters,
        "optimization_parameters": {"type": "unit_cell"}, "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}

L = LatticeOpti(preset)
theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
L.objective(theta)
g = np.asarray(L.gradient(theta))
L.conduction_chain = False
L.objective(theta)
g_fixed_T = np.asarray(L.gradient(theta))
L.conduction_chain = True
rows = []
for i in (0, 5, 11):
    tp, tm = list(theta), list(theta)
    tp[i] += 1e-4
    tm[i] -= 1e-4
    rows.append({"variable": i, "gradient": float(g[i]), "central_difference": (L.objective(tp) - L.objective(tm)) / 2e-4,
                 "gradient_with_the_temperature_taken_as_fixed": float(g_fixed_T[i])})
L.redefine_optim_parameters(max_iteration=iters, disp=False)
sol = L.optimize_lattice()
print(json.dumps({"parameters": L.number_parameters, "gradient_check": rows, "iterations": int(sol.nit),
                  "compliance_first": float(L.initial_value_objective), "compliance_last": float(L.denorm_objective),
                  "largest_temperature": float(L.temperature_field.max()),
                  "relative_density": L.relative_density()}, indent=1))
