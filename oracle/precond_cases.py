"""Lattices and boundary sets the preconditioner tests share (tests/test_precond_reference_host.py measures the sensitivity
floor of exactly the inputs tests/test_gpu_precond.py runs on the device).

A boundary set is built FROM the solver's partition (HipLattice.partition(); recorded in tests/golden/precond_partition.npz
for the host test, which has no device - the GPU test asserts that the record is still what the library cuts):
  a  a clamped face, a tip load and an interior load (forces and moments in every direction, so that every mode of the
     levels carries part of the residual);
  b  a plus rollers (single dofs of some nodes fixed) and non-zero prescribed values;
  c  a plus a node with all six dofs fixed whose struts all stay inside its own tile - strictly inside a tile and an
     aggregate: the struts at it are in-aggregate struts that touch a Dirichlet dof (Coarse::fix_list);
  d  a plus one tile with every node but one fixed: six free dofs under 6 or 12 tile modes (rank-deficient B_t).
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import timoshenko_oracle as O

E, NU = 1013.0, 0.3
LATTICES = ("bcc_6x3x3", "octet_4x3x3", "bcchybrid1hybrid4_3x2x1_size")
# opts.tile_nodes: 32 where that cuts at least four tiles and two aggregates.  On the two generated lattices it does not,
# whatever opts.coarse_max_dofs: 3 tiles on the BCC one, a single aggregate on the Octet one (the brick edge follows from
# tile_nodes alone, pl_tile.h spatial_order, and an aggregate spans at least 1.5 bricks per axis, pl_coarse.h) - 16 there
# (16 and 12 tiles, two aggregates each)
TILE_NODES = {"bcc_6x3x3": 16, "octet_4x3x3": 16, "bcchybrid1hybrid4_3x2x1_size": 32}
# opts.coarse_max_dofs per modes of the dense level (the same aggregates for both)
COARSE_MAX_DOFS = {6: 600, 12: 1200}
BOUNDARY_SETS = ("a", "b", "c", "d")
MODE_PAIRS = ((6, 6), (12, 6), (12, 12))
# inputs every group of solver forms of tests/test_gpu_precond.py runs on (its tolerance is held against their floors)
GROUP_CASES = {"fp64": tuple((n, b) for n in LATTICES for b in BOUNDARY_SETS),
               "fp32": (("bcc_6x3x3", "b"), ("bcc_6x3x3", "c"))}
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


class Lattice:
    """node_xyz, beam_conn, beam_radius, seg_len, seg_nsub of one test lattice, and its oracle matrix (lazily)."""

    def __init__(self, name):
        from pylatticedso_amd import lattice_arrays as LA
        self.name = name
        if name == "bcc_6x3x3":
            lat = LA.generate((1, 1, 1), (6, 3, 3), ["BCC"], [0.05])
            pen = LA.penalize(lat, LA.compute_lzone(lat))
        elif name == "octet_4x3x3":
            lat = LA.generate((1, 1, 1), (4, 3, 3), ["Octet"], [0.03])
            pen = LA.penalize(lat, LA.compute_lzone(lat))
        else:
            from pylatticedso_amd.lattice_sim import LatticeSim
            g = np.load(os.path.join(GOLDEN, f"lattice_{name}.npz"))
            L = LatticeSim(json.loads(str(g["preset_json"])))
            lat, pen = L.lattice, L.penalized
        self.xyz = np.ascontiguousarray(lat.node_xyz, float)
        self.conn = np.ascontiguousarray(lat.beam_conn, np.int32)
        self.radius = np.ascontiguousarray(lat.beam_radius, float)
        self.seg_len, self.seg_nsub = np.asarray(pen.seg_len), np.asarray(pen.seg_nsub)
        self.n_nodes = len(self.xyz)
        self._K = None

    @property
    def scalars(self):
        return np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(self.radius, self.seg_len, self.seg_nsub)])

    @property
    def K(self):
        if self._K is None:
            self._K = O.assemble_condensed(self.xyz, self.conn, self.scalars).toarray()
        return self._K

    def device(self, **kw):
        from pylatticedso_amd import _capi
        return _capi.HipLattice(self.xyz, self.conn, self.radius, self.seg_len, self.seg_nsub, E, NU, **kw)


def recorded_partition(name, coarse_modes):
    g = np.load(os.path.join(GOLDEN, "precond_partition.npz"))
    return {"tile": g[f"{name}__{coarse_modes}__tile"], "agg": g[f"{name}__{coarse_modes}__agg"]}


def _load(n, nodes, scale):
    f = np.zeros((n, 6))
    pat = np.array([[0.3, -0.2, -1.0, 0.2, 0.5, -0.3], [-0.4, 0.5, 0.3, -0.4, 0.1, 0.6]])
    for q, i in enumerate(nodes):
        f[i] = scale * pat[q % 2]
    return f


def boundary_set(which, lat, part):
    """(fixed (N, 6) uint8, ubar (N, 6), f (N, 6), info) of boundary set a / b / c / d on ``lat`` under partition ``part``."""
    xyz, conn, N = lat.xyz, lat.conn, lat.n_nodes
    tile, agg = np.asarray(part["tile"]), np.asarray(part["agg"])
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    fixed = np.zeros((N, 6), np.uint8)
    ubar = np.zeros((N, 6))
    face = xyz[:, 0] == lo[0]
    fixed[face] = 1
    far = np.flatnonzero(xyz[:, 0] == hi[0])
    tip = far[np.argmax(xyz[far, 1] + 2.0 * xyz[far, 2])]
    mid = 0.5 * (lo + hi) + np.array([0.26, 0.24, -0.23]) * (hi - lo) / 3.0
    inner = int(np.argmin(((xyz - mid) ** 2).sum(axis=1)))
    f = _load(N, [tip, inner], 0.1)
    info = {"tip": int(tip), "inner": inner}
    nbr = [[] for _ in range(N)]
    for ia, ib in conn:
        nbr[ia].append(int(ib))
        nbr[ib].append(int(ia))
    if which == "b":
        floor = np.flatnonzero((xyz[:, 1] == lo[1]) & ~face)
        for q, i in enumerate(floor[::2]):                      # rollers: one or two dofs of a node
            fixed[i, 1] = 1
            ubar[i, 1] = 1e-3 * (1 + q % 3)
            if q % 3 == 0:
                fixed[i, 3] = 1
                ubar[i, 3] = -2e-3
        ubar[face, 0] = 2e-3 * (xyz[face, 2] - lo[2])           # the clamped face tilts
        ubar[face, 4] = 2e-3
        info["rollers"] = [int(i) for i in floor[::2]]
        assert len(info["rollers"]) >= 2
    elif which == "c":
        cand = [i for i in range(N) if not face[i] and len(nbr[i]) >= 3 and all(tile[j] == tile[i] for j in nbr[i])
                and not any(face[j] for j in nbr[i]) and i not in (tip, inner)]
        assert cand, "no node strictly inside a tile: choose another tile size"
        i = cand[len(cand) // 2]
        fixed[i] = 1
        ubar[i, :3] = [1e-3, -5e-4, 2e-4]
        info["inside"] = int(i)
    elif which == "d":
        sizes = {int(t): int((tile == t).sum()) for t in np.unique(tile)}
        ok = [t for t in sizes if sizes[t] >= 3 and not face[tile == t].any() and tile[tip] != t and tile[inner] != t]
        assert ok, "no tile away from the clamped face and the loads"
        t = min(ok, key=lambda q: (sizes[q], q))
        nodes = np.flatnonzero(tile == t)
        keep = max(nodes, key=lambda i: (sum(tile[j] == t for j in nbr[i]), -i))
        for i in nodes:
            if i != keep:
                fixed[i] = 1
        f[keep] = 0.05 * np.array([0.2, 0.1, -0.3, 0.01, -0.02, 0.03])
        info.update(tile=int(t), free_node=int(keep), tile_nodes=len(nodes))
    elif which != "a":
        raise ValueError(which)
    f = np.where(fixed != 0, 0.0, f)
    return fixed, ubar, f, info
