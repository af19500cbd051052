"""Transient response of a clamped BCC tower to a suddenly applied tip load (pl_set_mass, pl_transient,
LatticeSim.transient_response): implicit Newmark steps (average acceleration) of M a + C v + K u = f with the consistent mass of
the struts, undamped and with Rayleigh damping.  Prints the dynamic amplification of the top face's corner nodes - peak
displacement over the static one, 2 for one undamped degree of freedom - and the energy balance kinetic + strain - external
work, which stays 0 without damping and falls by what the damper takes with it."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
density = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0              # in units consistent with the Young modulus and the lengths
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 2, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["X"], "Value": [0.01]}}}}

tower = LatticeSim(preset)
solve_FEM_FenicsX(tower, rtol=1e-10)                                    # the static answer the response is measured against
omega1 = float(np.sqrt(tower.natural_frequencies(2, density=density, n_sub=12)["omega2"][0]))
dt = 2.0 * np.pi / omega1 / 40.0                                        # 40 steps per period of the first bending mode
xyz = tower.lattice.node_xyz
corners = np.flatnonzero((xyz[:, 2] > xyz[:, 2].max() - 1e-9) & np.isin(xyz[:, 0], (xyz[:, 0].min(), xyz[:, 0].max()))
                         & np.isin(xyz[:, 1], (xyz[:, 1].min(), xyz[:, 1].max())))
report = {"struts": tower.lattice.n_beams, "nodes": tower.lattice.n_nodes, "omega_1": omega1, "dt": dt, "steps": n_steps}
for name, damping in (("undamped", (0.0, 0.0)), ("rayleigh", (0.05 * omega1, 0.002 / omega1))):
    out = tower.transient_response(dt, n_steps, density, damping=damping, probes=corners, rtol=1e-10)
    e = tower.transient_energy
    balance = e[:, 0] + e[:, 1] - e[:, 2]
    report[name] = {"amplification": [float(v) for v in tower.dynamic_amplification()],
                    "peak_strain_energy": float(e[:, 1].max()),
                    "energy_balance_largest": float(np.abs(balance).max()), "energy_balance_last": float(balance[-1]),
                    "pcg_iterations_per_step": float(out["iters"][1:].mean())}
print(json.dumps(report))
