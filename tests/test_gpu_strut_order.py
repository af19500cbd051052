"""Per-strut outputs come back in the caller's strut numbering whatever order the handle keeps its struts in: a handle
that reorders nodes (reorder = 1, its strut permutation checked to be no identity) returns the same arrays as a handle that
keeps the caller's node order (reorder = 0), for every call that downloads rows per strut - one value (sens, stress peak,
the three buckling outputs), 8 (records), 12 (node_mod) and 20 (stress stations) per strut."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

E, NU = 1013.0, 0.3


def _lattice():
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                                    "radii": [0.05, 0.04], "geom_types": ["BCC", "Octet"]},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                       "boundary_conditions": {
                           "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                      "Value": [0, 0, 0, 0, 0, 0]}},
                           "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})


def _per_strut_outputs(L, mult, u, lam, reorder):
    """(every per-strut array of the handle, home tile of every strut in the caller's strut order)"""
    lat, pen = L.lattice, L.penalized
    with _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU, reorder=reorder,
                          tile_nodes=16, beam_mult=mult) as dev:
        dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
        dev.assemble()
        out = {"sens": dev.sens(u, lam), "node_mod": dev.node_mod(u), "records": dev.records()}
        for where in (0, 1):
            out.update({f"stress{where}.{k}": v for k, v in dev.stress(u, where=where).items()})
        for length in (0, 1):
            out.update({f"buckling{length}.{k}": v for k, v in dev.buckling(u, length=length, k_eff=0.7, shear=1).items()})
        tile = dev.partition()["tile"]
    return out, tile[np.asarray(lat.beam_conn)].min(axis=1)


def test_reordered_handle_returns_the_callers_strut_order():
    L = _lattice()
    n, nb = L.lattice.n_nodes, L.lattice.n_beams
    rng = np.random.default_rng(11)
    mult = rng.integers(1, 5, nb).astype(float)
    u = rng.standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3
    lam = rng.standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3
    plain, _ = _per_strut_outputs(L, mult, u, lam, reorder=0)
    moved, home = _per_strut_outputs(L, mult, u, lam, reorder=1)
    # the device numbers struts by home tile (the smaller tile of the two ends): where the home tiles do not ascend along the
    # caller's struts, the device order is another one
    assert home.min() >= 0 and (np.diff(home) < 0).any()
    assert set(plain) == set(moved) and len(plain) == 3 + 2 * 6 + 2 * 3
    for name in sorted(plain):
        a, b = plain[name], moved[name]
        assert a.shape == b.shape and a.shape[0] == nb, name
        assert not np.isnan(a).all(), name
        # every one of these is computed strut by strut from the same operands: bitwise equal (so it is on the commit
        # before the single download helper, where each call permuted its rows itself)
        assert np.array_equal(a, b, equal_nan=True), (name, np.nanmax(np.abs(a - b)))
