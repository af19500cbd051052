"""Natural frequencies of a clamped BCC tower (pl_set_mass, pl_vibration_modes, LatticeSim.natural_frequencies): the lowest
frequencies and modes of K phi = omega^2 M phi with the consistent mass of the struts, without and with a payload on the top
face, and the struts whose radius moves the first frequency most (pl_vibration_modes_sens).  Every strut is one element
between its joints: a strut vibrating between its own two joints is not resolved."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_modes = int(sys.argv[2]) if len(sys.argv) > 2 else 5
density = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0              # in units consistent with the Young modulus and the lengths
preset = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 2, "z": nz},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["Z"], "Value": [-0.1]}}}}

tower = LatticeSim(preset)
solve_FEM_FenicsX(tower)                                                # supports on the device; the loads play no part
kw = dict(n_sub=max(12, 4 * ((2 * n_modes + 3) // 4)))
bare = tower.natural_frequencies(n_modes, density=density, **kw)
sens = tower.natural_frequency_sensitivity(p=8)
first = sens["domega2_dr"][0]
xyz = tower.lattice.node_xyz
strut_mass = density * float((np.pi * tower.lattice.beam_radius ** 2
                              * np.linalg.norm(xyz[tower.lattice.beam_conn[:, 1]] - xyz[tower.lattice.beam_conn[:, 0]], axis=1)).sum())
top = xyz[:, 2] > xyz[:, 2].max() - 1e-9
payload = np.where(top, strut_mass / top.sum(), 0.0)                    # the tower's own mass again, spread over the top face
loaded = tower.natural_frequencies(n_modes, density=density, node_mass=payload, **kw)
print(json.dumps({"struts": tower.lattice.n_beams, "nodes": tower.lattice.n_nodes, "strut_mass": strut_mass,
                  "frequencies_hz": [float(v) for v in bare["frequency"]],
                  "mode_residuals": [float(v) for v in bare["residual"]],
                  "outer_iterations": bare["outer_iterations"],
                  "frequencies_hz_with_payload": [float(v) for v in loaded["frequency"]],
                  "struts_that_raise_f1_most": [int(b) for b in np.argsort(-first)[:5]],
                  "struts_that_lower_f1_most": [int(b) for b in np.argsort(first)[:5]]}))
