"""Condense a Diamond + Kelvin unit cell - 38 boundary nodes, beyond the size the batched exact kernel holds - onto its
boundary nodes by column blocks: `column_block` columns of the Schur complement per PCG pass (pl_schur_block) instead of one
solve per boundary dof (pl_schur)."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "src"))

from pyLatticeSim.lattice_sim import LatticeSim                   # noqa: E402
from pyLatticeSim.utils_schur import get_schur_complement         # noqa: E402

preset = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                       "radii": [0.03, 0.03], "geom_types": ["Diamond", "Kelvin"]},
          "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": True}}
cell = LatticeSim(preset)
get_schur_complement(cell, column_block=0)                        # warm-up: handle, records, workspace
results = {}
for block in (None, 0):
    t0 = time.perf_counter()
    results[block] = get_schur_complement(cell, column_block=block)
    label = "one solve per column (pl_schur)" if block is None else "column blocks (pl_schur_block)"
    print(f"{label:34s} {1e3 * (time.perf_counter() - t0):8.1f} ms")
S, S1 = results[0], results[None]
print(f"{cell.geom_types} cell: S is {S.shape[0]} x {S.shape[1]}, asymmetry {np.abs(S - S.T).max() / np.abs(S).max():.1e}, "
      f"difference between the two paths {np.linalg.norm(S - S1) / np.linalg.norm(S1):.1e}")
