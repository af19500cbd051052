"""Global linear buckling of a BCC column under end compression (pl_buckling_modes, LatticeSim.global_buckling): the
factors by which the applied load may grow before cells or the whole column buckle together, beside the factor at which
the first strut buckles on its own (1 / max_strut_buckling, pl_buckling).  The two checks see different failures: the
global analysis takes every strut as one element between its joints, the strut check takes the joints as immovable."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_modes = int(sys.argv[2]) if len(sys.argv) > 2 else 4
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 2, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["Z"], "Value": [-0.1]}}}}

column = LatticeSim(preset)
solve_FEM_FenicsX(column)
out = column.global_buckling(n_modes, n_sub=max(12, 4 * ((2 * n_modes + 3) // 4)))
tip = [float(abs(m[:, :3]).max()) for m in column.buckling_modes[:out["n_found"]]]
print(json.dumps({"struts": column.lattice.n_beams, "nodes": column.lattice.n_nodes,
                  "global_load_factors": [float(v) for v in column.buckling_load_factors],
                  "mode_residuals": [float(v) for v in out["residual"]],
                  "largest_mode_displacement": tip,
                  "outer_iterations": out["outer_iterations"],
                  "strut_load_factor_pinned": 1.0 / column.max_strut_buckling(length=0),
                  "strut_load_factor_middle_segment": 1.0 / column.max_strut_buckling(length=1),
                  "strut_load_factor_clamped": 1.0 / column.max_strut_buckling(length=0, k_eff=0.5)}))
