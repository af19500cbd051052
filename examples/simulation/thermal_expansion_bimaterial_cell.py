"""Homogenised thermal expansion of a bi-material Octet + BCC cell over the radius ratio
(HomogenizedCell.thermal_expansion): the Octet struts expand with alpha_1, the BCC struts with alpha_2 < alpha_1, and the
stiffer family pulls the cell's expansion towards its own coefficient.  No solve beyond the six of the homogenisation:
alpha_hom = H^-1 tau with H_kl = u_k^T K u_l and tau_k = u_k^T f_th of the six total fields."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.homogenization_cell import HomogenizedCell       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

alpha_octet, alpha_bcc = 7e-5, 2e-5
r_octet = 0.04
rows = []
for ratio in (0.5, 1.0, 1.5, 2.0):
    cell = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": [r_octet, ratio * r_octet], "geom_types": ["Octet", "BCC"]},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                       "boundary_conditions": {}})
    analysis = HomogenizedCell(cell)
    analysis.prepare_simulation()
    analysis.apply_dirichlet_for_homogenization()
    analysis.periodic_boundary_condition()
    analysis.solve_full_homogenization()
    beam_alpha = np.where(np.asarray(cell.lattice.beam_type) == 0, alpha_octet, alpha_bcc)
    a = analysis.thermal_expansion(alpha_octet, beam_alpha)
    rows.append({"r_bcc / r_octet": ratio, "alpha_hom": [float(v) for v in a], "alpha_hom / alpha_octet": float(a[0] / alpha_octet)})
print(json.dumps({"alpha_octet": alpha_octet, "alpha_bcc": alpha_bcc, "rows": rows}, indent=1))
