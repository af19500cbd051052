"""Inverse design of a hybrid unit cell: which radii of a BCC + Cubic cell give a wanted Young modulus Ex and shear modulus
Gxy?  The diagonal struts of the BCC family carry the shear, the axis-parallel struts of the Cubic family the normal
stiffness, so the two moduli pin the two radii.  For a cubic cell Ex and Gxy follow from three entries of the homogenised
matrix (H00, H01, H33); their targets are taken from a cell that exists (radii 0.06 / 0.04), so the fit has an exact answer to
find.  ``fit_cell_radii`` runs scipy's least_squares with the analytic Jacobian of
``HomogenizedCell.homogenized_sensitivity(per="radius")``: six periodic solves and ONE pl_sens_gram call per evaluation,
no finite differences over whole homogenisations."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "src"))
from pyLatticeSim.homogenization_cell import fit_cell_radii                # noqa: E402
from pyLatticeSim.lattice_sim import LatticeSim                            # noqa: E402
from pyLatticeSim.utils_simulation import get_homogenized_sensitivities    # noqa: E402


def cell(radii):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": [float(r) for r in radii], "geom_types": ["BCC", "Cubic"]},
                       "simulation_parameters": {"enable": False, "material": "VeroClear", "periodicity": True}})


def moduli(analysis):
    M = analysis.orthotropicMatrix
    return M[0, 0], M[3, 3]


wanted = [float(v) for v in sys.argv[1:3]] if len(sys.argv) > 2 else [0.06, 0.04]
H_target, _, reference = get_homogenized_sensitivities(cell(wanted))
Ex_t, Gxy_t = moduli(reference)
print(f"target: Ex = {Ex_t:.6f}  Gxy = {Gxy_t:.6f}   (the cell with radii {wanted})")

start = cell([0.05, 0.05])
result, analysis = fit_cell_radii(start, H_target, rows=[(0, 0), (0, 1), (3, 3)])
Ex, Gxy = moduli(analysis)
print(f"reached: Ex = {Ex:.6f}  Gxy = {Gxy:.6f}   radii = {np.array2string(result.x, precision=8)}")
print(f"evaluations: {result.nfev}   residual / |target| = {np.sqrt(2.0 * result.cost):.2e}   ({result.message})")
d = analysis.orthotropic_sensitivity(per="radius")
print("dEx / d radii  =", np.array2string(d["Ex"], precision=4), "  dGxy / d radii =", np.array2string(d["Gxy"], precision=4))
