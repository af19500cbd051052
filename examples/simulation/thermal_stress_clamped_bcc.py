"""A BCC column heated between two clamped faces (LatticeSim.set_temperature, pl_set_thermal): the struts want to grow, the
faces do not let them, and every strut ends in compression.  Prints the largest von Mises stress and the largest Euler
buckling utilisation of any strut against the temperature rise; cooled by the same amount the struts are in tension and
the utilisation is exactly 0."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 3
alpha = float(sys.argv[2]) if len(sys.argv) > 2 else 7e-5
dofs = ["X", "Y", "Z", "RX", "RY", "RZ"]
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {"Displacement": {"Foot": {"Surface": ["Zmin"], "DOF": dofs, "Value": [0] * 6},
                                             "Head": {"Surface": ["Zmax"], "DOF": dofs, "Value": [0] * 6}}}}

column = LatticeSim(preset)
rows = []
for dT in (-40.0, 10.0, 20.0, 40.0, 80.0):
    column.set_temperature(dT, alpha)
    solve_FEM_FenicsX(column)
    n = column.strut_buckling(length=0)["n_axial"]
    rows.append({"dT": dT, "max_sigma_vm": column.max_strut_stress(), "max_buckling_utilisation": column.max_strut_buckling(),
                 "largest_compression": float(-n.min()) if n.min() < 0 else 0.0,
                 "largest_restrained_force": float(abs(column.thermal_strut_forces()).max())})
print(json.dumps({"struts": column.lattice.n_beams, "alpha": alpha, "rows": rows}, indent=1))
