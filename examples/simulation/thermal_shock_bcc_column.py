"""Thermal shock of a BCC column (LatticeSim.transient_temperature, pl_cond_transient): a 1 x 1 x nz column rests at the ambient,
its base jumps to 90 and the heat front climbs against the convective loss of the struts, under backward Euler.  The probe
histories along the column, the time the tip needs for 95 % of its steady rise, the heat balance - and, the cold head clamped
and the hot base free, the thermal stress of a few snapshots: set_temperature takes any row of the history, so the peak stress
is seen DURING the transient, where the gradient behind the front is steepest, and not at its end."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 4
n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 120
kappa, film, rho_c, alpha, t_hot, ambient, dt = 0.2, 0.005, 2.0, 7e-5, 90.0, 20.0, 0.5
dofs = ["X", "Y", "Z", "RX", "RY", "RZ"]
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {"Displacement": {"Head": {"Surface": ["Zmax"], "DOF": dofs, "Value": [0] * 6}}}}

column = LatticeSim(preset)
lat = column.lattice
z = lat.node_xyz[:, 2]
T_steady = column.solve_temperature(kappa, {"Base": {"Surface": ["Zmin"], "Value": t_hot}}, reference=ambient,
                                    convection={"film": film, "ambient": ambient})
# one probe per layer of nodes, the first node of each
layers = np.unique(np.round(z, 9))
probes = [int(np.flatnonzero(np.isclose(z, h))[0]) for h in layers]
snap_every = 2
hist = column.transient_temperature(dt, n_steps, rho_c, theta=1.0, probes=probes, snap_every=snap_every)
tip = hist["probe"][:, -1] - ambient
reached = np.flatnonzero(tip >= 0.95 * (T_steady[probes[-1]] - ambient))
U, Q_in, Q_c, Q_R = hist["heat"].T
# the thermal stress of the snapshots and of the steady state
stress = {}
for k in sorted({min(2 ** j, len(hist["snaps"])) - 1 for j in range(7)}):
    column.set_temperature(hist["snaps"][k] - ambient, alpha)
    solve_FEM_FenicsX(column)
    stress[f"t = {dt * snap_every * (k + 1):g}"] = column.max_strut_stress()
column.set_temperature(T_steady - ambient, alpha)
solve_FEM_FenicsX(column)
stress["steady"] = column.max_strut_stress()
rows = np.linspace(0, n_steps, 7).astype(int)
print(json.dumps({"struts": lat.n_beams, "dt": dt, "steps": n_steps, "layer_heights": layers.tolist(),
                  "probe_histories_by_layer": {f"t = {hist['times'][r]:g}": np.round(hist["probe"][r], 4).tolist() for r in rows},
                  "steady_by_layer": np.round(T_steady[probes], 4).tolist(),
                  "time_to_95_percent_of_the_steady_tip_rise": float(hist["times"][reached[0]]) if len(reached) else None,
                  "stored_heat_U": np.round(U[rows], 6).tolist(), "supplied_by_the_base_Q_R": np.round(Q_R[rows], 6).tolist(),
                  "lost_to_the_ambient_Q_c": np.round(Q_c[rows], 6).tolist(),
                  "largest_balance_defect": float(np.abs((U - U[0]) - (Q_in + Q_R - Q_c)).max()),
                  "pcg_iterations_per_step": float(hist["iters"][1:].mean()),
                  "max_sigma_vm_of_the_snapshots": stress}, indent=1))
