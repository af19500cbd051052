"""pl_schur_block (the Schur complement of a node subset, `block` columns per PCG pass, generated and contracted on the
device) against the exact batched condensation, the committed dolfinx goldens, the oracle's dense condensation and
pl_schur; and the three opt-in call sites of the multi-column solver."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import timoshenko_oracle as O                              # noqa: E402
from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_schur import get_schur_complement, node_order_to_simulate   # noqa: E402

E, NU = 1013.0, 0.3
BLOCKS = [1, 6, 32, 0]


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def _cell(geoms, radii, penalised=True):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": [float(r) for r in radii], "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": penalised, "material": "VeroClear", "periodicity": True}})


def _arrays(L):
    lat, pen = L.lattice, L.penalized
    return (lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, node_order_to_simulate(L, 0))


def _dofs(nodes):
    return (6 * np.asarray(nodes)[:, None] + np.arange(6)).ravel()


def _oracle_K(xyz, conn, rad, seg_len, seg_nsub):
    sc = np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(rad, seg_len, seg_nsub)])
    return np.asarray(O.assemble_condensed(xyz, conn, sc).todense())


def _symmetric(S):
    return np.linalg.norm(S - S.T) <= 1e-8 * np.linalg.norm(S)


@pytest.mark.parametrize("geom", sorted(_BUILTIN))
def test_block_condensation_against_the_exact_batched_kernel(geom):
    """schur(block=b), b in {1, 6, 32, 0}, within 1e-8 of schur_cells for every built-in cell that fits it."""
    L = _cell([geom], [0.04])
    xyz, conn, rad, sl, sn, order = _arrays(L)
    if _capi.schur_cells_fits(len(xyz), len(conn), len(order)):
        S0, info = _capi.schur_cells(xyz, conn, order, rad, sl, sn, E, NU)
        assert info[0] == 0
    else:      # beyond the batched kernel: the oracle's dense condensation stands in
        K = _oracle_K(xyz, conn, rad, sl, sn)
        bd, it = _dofs(order), _dofs(np.setdiff1d(np.arange(len(xyz)), order))
        S0 = [K[np.ix_(bd, bd)] - K[np.ix_(bd, it)] @ np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)])]
    with _capi.HipLattice(xyz, conn, rad, sl, sn, E, NU, reorder=0) as dev:
        dev.assemble()
        for b in BLOCKS:
            S = dev.schur(order, rtol=1e-13, max_iter=200000, block=b)
            print(geom, "block", b, "against schur_cells", _rel(S, S0[0]))
            assert _rel(S, S0[0]) < 1e-8, (geom, b)
            assert _symmetric(S)


@pytest.mark.parametrize("geom", ["BCC", "Hybrid1", "Hybrid4"])
def test_block_condensation_against_dolfinx_goldens(golden_dir, geom):
    """the construction and the bound of test_schur_complement_matches_dolfinx_golden, through pl_schur_block."""
    sg = np.load(os.path.join(golden_dir, f"schur_{geom}.npz"))
    for r, G in list(zip(sg["radius_values"].ravel(), sg["schur_matrices"]))[::2]:
        L = _cell([geom], [r], penalised=geom == "BCC")
        order = node_order_to_simulate(L, 0)
        dev = L.device_model()
        dev.assemble()
        for b in BLOCKS:
            S = dev.schur(order, rtol=1e-13, max_iter=200000, block=b)
            assert S.shape == G.shape
            assert _rel(S, G) < 1e-8, (geom, r, b)
        dev.close()


def test_cell_beyond_the_batched_limit():
    """Diamond + Kelvin (38 boundary nodes) against the oracle's dense K_BB - K_BI K_II^-1 K_IB and against
    schur(block=None) at 1e-8; symmetric; the handle's boundary data survive the call."""
    L = _cell(["Diamond", "Kelvin"], [0.03, 0.03])
    xyz, conn, rad, sl, sn, order = _arrays(L)
    assert not _capi.schur_cells_fits(len(xyz), len(conn), len(order))
    K = _oracle_K(xyz, conn, rad, sl, sn)
    interior = np.setdiff1d(np.arange(len(xyz)), order)
    bd, it = _dofs(order), _dofs(interior)
    ref = K[np.ix_(bd, bd)] - K[np.ix_(bd, it)] @ np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)])
    rng = np.random.default_rng(1)
    n = len(xyz)
    fixed = np.zeros((n, 6), bool)
    fixed[order[:6]] = True
    f = np.where(fixed, 0.0, 1e-3 * rng.standard_normal((n, 6)))
    with _capi.HipLattice(xyz, conn, rad, sl, sn, E, NU, reorder=0, precond=5) as dev:
        dev.assemble()
        dev.set_bc(fixed, None, f)
        u_before, _ = dev.solve(rtol=1e-12, max_iter=200000)
        Sb = {}
        for b in BLOCKS:
            Sb[b] = dev.schur(order, rtol=1e-13, max_iter=200000, block=b)
            print("block", b, "against the oracle", _rel(Sb[b], ref))
            assert _rel(Sb[b], ref) < 1e-8
            assert _symmetric(Sb[b])
        u_after, _ = dev.solve(rtol=1e-12, max_iter=200000)      # the boundary data are what they were
        assert _rel(u_after, u_before) < 1e-7
        S1 = dev.schur(order, rtol=1e-13, max_iter=200000)
        for b in BLOCKS:
            assert _rel(Sb[b], S1) < 1e-8
    # the opt-in of get_schur_complement
    Sd = get_schur_complement(L)
    Sc = get_schur_complement(L, column_block=32)
    L._device.close()
    print("get_schur_complement(column_block=32) against the default", _rel(Sc, Sd))
    assert _rel(Sc, Sd) < 1e-8


def test_paired_fallback_of_recover_cell_interiors():
    """the lattice and the bounds of test_lattice_of_over_limit_cells_through_recover_cell_interiors, with u and lam
    solved as two columns and the cell matrices condensed by column blocks."""
    preset = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                           "radii": [0.03, 0.03], "geom_types": ["Diamond", "Kelvin"]},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                        "DDM": {"enable_preconditioner": False, "max_iterations": 5000,
                                                "schur_complement_computation": {"type": "exact"}}},
              "boundary_conditions": {
                  "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                             "Value": [0, 0, 0, 0, 0, 0]}},
                  "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}}
    L = LatticeSim(preset, enable_domain_decomposition_solver=True)
    L.schur_column_block = 32
    L.set_cell_radii([[0.03, 0.03], [0.035, 0.028]])
    lat, pen = L.lattice, L.penalized
    cb = L.cell_boundary_nodes()
    rng = np.random.default_rng(17)
    bnd = np.unique(cb)
    L.displacement_vector[:] = 0.0
    L.displacement_vector[bnd] = rng.standard_normal((len(bnd), 6))
    before = L.displacement_vector.copy()
    lam = np.zeros_like(before)
    lam[bnd] = rng.standard_normal((len(bnd), 6))
    sens = L.recover_cell_interiors(lam=lam, want_sens=True)
    assert np.array_equal(L.displacement_vector[bnd], before[bnd])
    expect = np.zeros(lat.n_beams)
    for c in range(2):
        beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
        nodes = np.unique(lat.beam_conn[beams])
        conn, order = np.searchsorted(nodes, lat.beam_conn[beams]), np.searchsorted(nodes, cb[c])
        interior = np.setdiff1d(np.arange(len(nodes)), order)
        K = _oracle_K(lat.node_xyz[nodes], conn, lat.beam_radius[beams], pen.seg_len[beams], pen.seg_nsub[beams])
        bd, it = _dofs(order), _dofs(interior)
        # the cell matrix itself came through pl_schur_block
        Sref = K[np.ix_(bd, bd)] - K[np.ix_(bd, it)] @ np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)])
        assert _rel(L.schur_complements[L.cell_schur_index[c]], Sref) < 1e-8
        A = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)])
        err = _rel(L.displacement_vector[nodes[interior]].ravel(), A @ before[cb[c]].ravel())
        print("cell", c, "interior rows against the oracle", err)
        assert err < 1e-8
        lam_c = lam[nodes].copy()
        lam_c[interior] = (A @ lam[cb[c]].ravel()).reshape(-1, 6)
        with _capi.HipLattice(lat.node_xyz[nodes], conn, lat.beam_radius[beams], pen.seg_len[beams], pen.seg_nsub[beams],
                              E, NU) as dev:
            dev.assemble()
            ref = dev.sens(L.displacement_vector[nodes], lam_c)
        b, s = L.cell_strut_sens[c]
        assert np.array_equal(b, beams)
        print("cell", c, "sensitivities", np.abs(s - ref).max() / np.abs(ref).max())
        assert np.abs(s - ref).max() < 1e-7 * np.abs(ref).max()
        np.add.at(expect, beams, s)
    assert np.allclose(sens, expect, rtol=0, atol=1e-14 * np.abs(expect).max())


OPTI = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "displacement", "max_iterations": 5,
        "optimization_parameters": {"type": "unit_cell"},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}


@pytest.mark.parametrize("objective,data,fn", [("displacement", {"Surface": ["Xmax"], "DOF": ["Z"]}, "max"),
                                                ("displacement_ratio", {"Surface": ["Zmax"], "DOF": ["Z"]}, "min")])
def test_paired_adjoint_gradient(objective, data, fn):
    """LatticeOpti(paired_adjoint=True) against paired_adjoint=False, 1e-7 relative."""
    p = copy.deepcopy(OPTI)
    p["optimization_informations"].update(objective_type=objective, objective_data=data, objective_function=fn)
    grads = {}
    for paired in (False, True):
        opt = LatticeOpti(copy.deepcopy(p), paired_adjoint=paired)
        theta = list(0.3 + 0.4 * np.random.default_rng(2).random(opt.number_parameters))
        opt.objective(theta)
        grads[paired] = np.asarray(opt.gradient(theta), dtype=float).copy()
        if opt._device is not None:
            opt._device.close()
    print(objective, "paired against separate adjoint", _rel(grads[True], grads[False]))
    assert np.linalg.norm(grads[False]) > 0
    assert _rel(grads[True], grads[False]) < 1e-7
