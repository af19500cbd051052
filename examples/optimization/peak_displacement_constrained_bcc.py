"""The clamped BCC tower of examples/simulation/transient_step_load_bcc_tower.py under a suddenly applied tip load, its radius
graded along z, with a bound on the peak of the tip displacement over time: the "peak_displacement" constraint of LatticeOpti
(FEM mode) holds (sum_n |y_n|^p)^(1/p) / max_displacement - 1 <= 0 for the output y_n = l . u_n of the Newmark run
(pl_transient_sens), l the force pattern scaled to unit norm, which keeps max_n |y_n| <= max_displacement; its gradient is the
discrete adjoint of the scheme, one backward sweep in time.  The objective is the static compliance under a volume bound, as
in the sibling examples (the package has no volume objective): the start design violates the peak bound, the volume bound
leaves room to meet it."""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 3
gain = float(sys.argv[2]) if len(sys.argv) > 2 else 0.8                 # max_displacement / J_p of the start design
density = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
n_steps = 80
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 2, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["X"], "Value": [0.01]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": 30,
        "optimization_parameters": {"type": "linear", "direction": ["z"]},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}

# the start design: its first frequency sets the time step (40 steps per period), its J_p the bound
start = LatticeOpti(preset)
start._initialize_optimization_solver()
x0 = start.initial_parameters
start.objective(x0)
omega1 = float(np.sqrt(start.natural_frequencies(2, density=density, n_sub=12)["omega2"][0]))
run = {"dt": 2.0 * np.pi / omega1 / 40.0, "n_steps": n_steps, "density": density, "damping": [0.05 * omega1, 0.002 / omega1],
       "p": 8, "max_displacement": 1.0}
probe = copy.deepcopy(preset)
probe["optimization_informations"]["constraints"]["peak_displacement"] = run
probe = LatticeOpti(probe)
J0 = probe.peak_displacement_constraint(x0) + 1.0
peak0 = probe._last_peak_displacement[1]
rho0 = probe.relative_density()

bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"].update(
    relative_density={"value": 1.5 * rho0}, peak_displacement=dict(run, max_displacement=gain * J0))
con = LatticeOpti(bounded)
con.redefine_optim_parameters(disp=False)
sol = con.optimize_lattice()
c = con.peak_displacement_constraint(sol.x)
J1, peak1 = con._last_peak_displacement
print(f"peak before: {peak0:.6g} (J_p {J0:.6g})   bound: {gain * J0:.6g}   peak after: {peak1:.6g} (J_p {J1:.6g})")
print(json.dumps({"struts": con.lattice.n_beams, "omega_1": omega1, "dt": run["dt"], "steps": n_steps,
                  "start": {"x": list(map(float, x0)), "J_p": J0, "peak": peak0, "relative_density": rho0},
                  "bounded": {"x": list(map(float, sol.x)), "J_p": J1, "peak": peak1, "peak_displacement_constraint": c,
                              "compliance": con.compute_compliance(), "relative_density": con.relative_density(),
                              "peak_displacement_history": con._history["peak_displacement"]}}))
