"""Frequency response of a clamped BCC tower (pl_set_mass, pl_harmonic, LatticeSim.frequency_response): the tower of
natural_frequencies_bcc_tower.py under a harmonic sideways load on its top face, swept through its first three bending
resonances with Rayleigh damping (0.05 omega_1, 0.002 / omega_1), and the same band under a base shaken sideways.  The peaks of
the sweep are printed beside natural_frequencies().  Every frequency is one complex symmetric system, solved by COCG; the
frequencies of the sweep iterate in lock step, 32 per pass."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_freq = int(sys.argv[2]) if len(sys.argv) > 2 else 64
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
solve_FEM_FenicsX(tower)                                                # supports and the force set on the device
modes = tower.natural_frequencies(8, density=density, n_sub=16)
hz = modes["frequency"]
# the bending modes in x come in pairs with those in y (a square tower), torsion lies between: sweep past the third pair
band = np.linspace(0.5 * hz[0], 1.1 * hz[5], n_freq)
w1 = 2.0 * np.pi * hz[0]
damping = (0.05 * w1, 0.002 / w1)
xyz = tower.lattice.node_xyz
corner = np.flatnonzero((xyz[:, 2] > xyz[:, 2].max() - 1e-9) & (xyz[:, 0] == xyz[:, 0].min()) & (xyz[:, 1] == xyz[:, 1].min()))
out = tower.frequency_response(band, density, damping=damping, probes=corner, max_iter=20000)
peaks = tower.dynamic_stiffness_peaks()[0]
static = float(np.linalg.norm(tower.displacement_vector[corner[0], :3]))
base = tower.frequency_response(band, density, damping=damping, probes=corner, base_acceleration=0, max_iter=20000)
T = np.abs(tower.frf_transmissibility[:, 0, 0])
print(json.dumps({"struts": tower.lattice.n_beams, "nodes": tower.lattice.n_nodes,
                  "natural_frequencies_hz": [float(v) for v in hz],
                  "band_hz": [float(band[0]), float(band[-1])], "frequencies": int(n_freq),
                  "peak_frequencies_hz": [float(v) for v in peaks["frequency"]],
                  "peak_amplitude_over_static": [float(v / static) for v in peaks["amplitude"]],
                  "iterations_min_max": [int(out["iters"].min()), int(out["iters"].max())],
                  "dissipated_power_at_peaks": [float(-0.5 * 2.0 * np.pi * band[i] * out["power"][i, 1]) for i in peaks["index"]],
                  "base_transmissibility_max": float(T.max()), "base_transmissibility_at_hz": float(band[int(T.argmax())]),
                  "base_iterations_min_max": [int(base["iters"].min()), int(base["iters"].max())]}))
