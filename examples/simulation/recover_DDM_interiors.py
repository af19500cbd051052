"""Domain-decomposition solve with exact cell Schur complements, recovery of the cell interiors and export of the whole
field - what a FEM solve offers afterwards, on a DDM result (cf. compare_FEM_DDM.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "src"))

from pyLatticeSim.lattice_sim import LatticeSim                                   # noqa: E402
from pyLatticeSim.utils_simulation import solve_FEM_FenicsX                       # noqa: E402
from pyLatticeSim.export_simulation_results import exportSimulationResults        # noqa: E402

preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 4, "y": 2, "z": 2},
                 "radii": [0.04, 0.03], "geom_types": ["BCC", "Hybrid1"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                              "DDM": {"enable_preconditioner": True, "preconditioner_type": "exact", "max_iterations": 1000,
                                      "schur_complement_computation": {"type": "exact"}}},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}}

lattice = LatticeSim(preset, enable_domain_decomposition_solver=True)
# one radius set per cell: every cell is its own representative, the recovered field is the FEM field
rng = np.random.default_rng(0)
radii = np.stack([0.03 + 0.03 * rng.random(lattice.get_number_cells()),
                  0.025 + 0.02 * rng.random(lattice.get_number_cells())], axis=1)
lattice.set_cell_radii(radii)
xsol, info, _, _ = lattice.solve_DDM(recover_interior=True)
print("CG info", info, "-", lattice.iteration, "iterations")

interior = np.setdiff1d(np.arange(lattice.lattice.n_nodes), np.unique(lattice.cell_boundary_nodes()))
print(len(interior), "interior nodes recovered, largest displacement", np.abs(lattice.displacement_vector[interior]).max())

# the same lattice by FEM
fem_preset = {**preset, "simulation_parameters": {k: v for k, v in preset["simulation_parameters"].items() if k != "DDM"}}
fem = LatticeSim(fem_preset)
fem.set_cell_radii(radii)
_, model = solve_FEM_FenicsX(fem)
err = np.linalg.norm(lattice.displacement_vector - model.u) / np.linalg.norm(model.u)
print("whole field against the FEM solve:", err)

export = exportSimulationResults(lattice.ddm_result_model(), "ddm_recovered")
export.full_export()
print("written:", export.pvd_path)
