"""A BCC column between a hot and a cold face (LatticeSim.solve_temperature, pl_cond_solve): every strut is one conductor
g = kappa pi r^2 / L between its nodes, the temperatures solve the graph Laplacian on the device, the strut heat flows add up to
the heat that crosses the column, and - the faces clamped - the temperature drop loads the struts: the thermal stress that
results (set_temperature("conduction", alpha))."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 4
kappa = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2
alpha, t_hot, t_cold, t_ref = 7e-5, 90.0, 20.0, 20.0
dofs = ["X", "Y", "Z", "RX", "RY", "RZ"]
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {"Displacement": {"Foot": {"Surface": ["Zmin"], "DOF": dofs, "Value": [0] * 6},
                                             "Head": {"Surface": ["Zmax"], "DOF": dofs, "Value": [0] * 6}}}}

column = LatticeSim(preset)
T = column.solve_temperature(kappa, {"Hot": {"Surface": ["Zmin"], "Value": t_hot}, "Cold": {"Surface": ["Zmax"], "Value": t_cold}},
                             reference=t_ref)
Q = column.strut_heat_flow()
lat = column.lattice
z = lat.node_xyz[:, 2]
# the heat that crosses the mid-plane of the first cell: every strut that leaves the hot face
za, zb = z[lat.beam_conn[:, 0]], z[lat.beam_conn[:, 1]]
crossing = float(np.where((za == z.min()) & (zb > za), Q, 0.0).sum() - np.where((zb == z.min()) & (za > zb), Q, 0.0).sum())
g = kappa * np.pi * 0.05 ** 2 / (np.sqrt(3.0) / 2.0)
column.set_temperature("conduction", alpha)
solve_FEM_FenicsX(column)
n = column.strut_buckling(length=0)["n_axial"]
print(json.dumps({"struts": lat.n_beams, "kappa": kappa, "temperatures_by_layer": sorted({round(float(t), 6) for t in T}, reverse=True),
                  "heat_through_the_column": crossing, "series_estimate_4g_over_2nz_times_dT": 4 * g / (2 * nz) * (t_hot - t_cold),
                  "largest_strut_heat_flow": float(np.abs(Q).max()),
                  "pcg_iterations": column.conduction_stats["iterations"],
                  "max_sigma_vm": column.max_strut_stress(), "largest_compression": float(-n.min()) if n.min() < 0 else 0.0,
                  "max_buckling_utilisation": column.max_strut_buckling()}, indent=1))
