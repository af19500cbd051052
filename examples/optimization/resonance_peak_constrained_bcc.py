"""The clamped BCC tower of examples/simulation/frequency_response_bcc_tower.py under a harmonic sideways load on its top face,
its radius graded along z, with a bound on the resonance peak of a top corner over a band around the first natural frequency:
the "resonance_peak" constraint of LatticeOpti (FEM mode) holds (sum_k |y_k|^p)^(1/p) / max_amplitude - 1 <= 0 for the complex
output y_k = l^T u(w_k) of the frequency response (pl_harmonic_sens), l the x displacement of the corner, which keeps
max_k |y_k| <= max_amplitude; the matrix of every frequency is complex symmetric, so the adjoint fields are solved beside the
fields in the same passes.  The objective is the static compliance under a volume bound, as in the sibling examples (the
package has no volume objective): the start design violates the peak bound, the volume bound leaves room to meet it - by
lowering the peak or by moving the resonance out of the band."""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 3
gain = float(sys.argv[2]) if len(sys.argv) > 2 else 0.6                 # max_amplitude / J_p of the start design
density = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
n_freq = 24
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


def first_frequency(L):
    return float(L.natural_frequencies(2, density=density, n_sub=12)["frequency"][0])


# the start design: its first frequency sets the band (0.7 f_1 ... 1.3 f_1) and the damping, its J_p the bound
start = LatticeOpti(preset)
start._initialize_optimization_solver()
x0 = start.initial_parameters
start.objective(x0)
f1 = first_frequency(start)
omega1 = 2.0 * np.pi * f1
xyz = np.asarray(start.lattice.node_xyz).reshape(-1, 3)
corner = int(np.argmax(xyz @ np.array([1.0, 1.0, 10.0])))              # the top corner at the largest x and y
run = {"frequencies_hz": np.linspace(0.7 * f1, 1.3 * f1, n_freq).tolist(), "density": density,
       "damping": [0.05 * omega1, 0.002 / omega1], "output": [corner, 0], "p": 8, "max_amplitude": 1.0}
probe = copy.deepcopy(preset)
probe["optimization_informations"]["constraints"]["resonance_peak"] = run
probe = LatticeOpti(probe)
J0 = probe.resonance_peak_constraint(x0) + 1.0
peak0 = probe._last_resonance_peak[1]
rho0 = probe.relative_density()

bounded = copy.deepcopy(preset)
bounded["optimization_informations"]["constraints"].update(
    relative_density={"value": 1.5 * rho0}, resonance_peak=dict(run, max_amplitude=gain * J0))
con = LatticeOpti(bounded)
con.redefine_optim_parameters(disp=False)
sol = con.optimize_lattice()
c = con.resonance_peak_constraint(sol.x)
J1, peak1 = con._last_resonance_peak
f1_after = first_frequency(con)
print(f"peak before: {peak0:.6g} (J_p {J0:.6g}, f_1 {f1:.6g} Hz)   bound: {gain * J0:.6g}   "
      f"peak after: {peak1:.6g} (J_p {J1:.6g}, f_1 {f1_after:.6g} Hz)")
print(json.dumps({"struts": con.lattice.n_beams, "band_hz": [run["frequencies_hz"][0], run["frequencies_hz"][-1]],
                  "frequencies": n_freq, "corner_node": corner,
                  "start": {"x": list(map(float, x0)), "J_p": J0, "peak": peak0, "f_1": f1, "relative_density": rho0},
                  "bounded": {"x": list(map(float, sol.x)), "J_p": J1, "peak": peak1, "f_1": f1_after,
                              "resonance_peak_constraint": c, "compliance": con.compute_compliance(),
                              "relative_density": con.relative_density(),
                              "resonance_peak_history": con._history["resonance_peak"]}}))
