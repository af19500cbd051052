"""Backward half of the exact DDM (pl_cells_recover: cell interiors u_I = -K_II^-1 K_IB u_B and the per-strut
sensitivities lam_e^T (dK_e/dr) u_e on the recovered fields, one workgroup per instance) against the CPU oracle, the
device's own operator, pl_sens, central differences of pl_schur_cells, the FEM field and the LatticeOpti gradients."""
import copy
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import timoshenko_oracle as O                              # noqa: E402
from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_schur import node_order_to_simulate        # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

E, NU = 1013.0, 0.3


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


def _recover_any(L, ub, lb):
    """The fields of a one-cell lattice: the batched kernel when the cell fits, LatticeSim's per-cell fallback beyond."""
    xyz, conn, rad, sl, sn, order = _arrays(L)
    if _capi.schur_cells_fits(len(xyz), len(conn), len(order)):
        out = _capi.cells_recover(xyz, conn, order, rad, sl, sn, ub, E, NU, lam_b=lb)
        assert out["info"][0] == 0
        return out["u"][0], out["lam"][0], out["sens"][0], True
    src = {"xyz": xyz, "radius": rad, "seg_len": sl, "seg_nsub": sn}
    u, lam, s = L._recover_cell_by_solve(src, conn, order, ub, lb, True)
    return u, lam, s, False


CELLS = [[g] for g in _BUILTIN] + [["BCC", "Hybrid1", "Hybrid4"], ["Kelvin", "BCC"]]


@pytest.mark.parametrize("geoms", CELLS, ids=["+".join(g) for g in CELLS])
def test_every_builtin_cell_against_oracle_and_the_devices_own_operator(geoms):
    """Items 1 - 3: interior values against -solve(K_II, K_IB u_b) of the host oracle (1e-10; 1e-8 through the fallback);
    lam_full^T K u_full == lam_b^T S u_b with K applied by HipLattice.spmv and S from pl_schur_cells, interior rows of
    K u_full vanish (1e-10); sens == pl_sens on the same fields (1e-12 of max |sens|); fixing the boundary dofs on a handle
    and solving reproduces u_full (1e-9)."""
    rng = np.random.default_rng(11)
    for r in (0.02, 0.035, 0.05):
        L = _cell(geoms, [r] * len(geoms))
        xyz, conn, rad, sl, sn, order = _arrays(L)
        n = len(xyz)
        interior = np.setdiff1d(np.arange(n), order)
        ub, lb = rng.standard_normal(6 * len(order)), rng.standard_normal(6 * len(order))
        u, lam, sens, batched = _recover_any(L, ub, lb)
        assert np.array_equal(u[order].ravel(), ub) and np.array_equal(lam[order].ravel(), lb)
        if len(interior):
            K = _oracle_K(xyz, conn, rad, sl, sn)
            bd, it = _dofs(order), _dofs(interior)
            for full, vb in ((u, ub), (lam, lb)):
                ref = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)] @ vb)
                err = _rel(full[interior].ravel(), ref)
                print(geoms, r, "interior vs oracle", err, "batched" if batched else "fallback")
                assert err < (1e-10 if batched else 1e-8), geoms
        with _capi.HipLattice(xyz, conn, rad, sl, sn, E, NU, precond=5) as dev:
            dev.assemble()
            Ku = dev.spmv(u)
            if batched:
                S, info = _capi.schur_cells(xyz, conn, order, rad, sl, sn, E, NU)
                assert info[0] == 0
                lhs, rhs = float((lam * Ku).sum()), float(lb @ S[0] @ ub)
                print(geoms, r, "energy identity", abs(lhs - rhs) / abs(rhs))
                assert abs(lhs - rhs) < 1e-10 * abs(rhs)
                if len(interior):
                    u0 = np.zeros_like(u)
                    u0[order] = u[order]
                    g = dev.spmv(u0)[interior]                       # K_IB u_b
                    assert np.linalg.norm(Ku[interior]) < 1e-10 * np.linalg.norm(g)
                ref_s = dev.sens(u, lam)
                print(geoms, r, "sens vs pl_sens", np.abs(sens - ref_s).max() / np.abs(ref_s).max())
                assert np.abs(sens - ref_s).max() < 1e-12 * np.abs(ref_s).max()
                if len(interior):
                    fixed = np.zeros((n, 6), bool)
                    fixed[order] = True
                    dev.set_bc(fixed, np.where(fixed, u, 0.0), None)
                    dev.assemble()
                    us, _ = dev.solve(rtol=1e-13, max_iter=200000)
                    assert _rel(us, u) < 1e-9, geoms
        if L._device is not None:
            L._device.close()


def test_over_limit_cell_goes_through_the_fallback():
    """A cell beyond the kernel's limits (Diamond + Kelvin: 38 boundary nodes) through LatticeSim._recover_cell_by_solve:
    u and lam against the oracle at 1e-8 (the bound the per-column condensation of the same cell is held to), interior
    rows of K u_full vanish to 1e-8 of ||K_IB u_b||, sens equal to pl_sens on the same fields (1e-12 of max |sens|); a
    zero field and lam = None are handled."""
    L = _cell(["Diamond", "Kelvin"], [0.03, 0.03])
    xyz, conn, rad, sl, sn, order = _arrays(L)
    assert len(order) > _capi.SCHUR_CELLS_MAX_BOUNDARY and not _capi.schur_cells_fits(len(xyz), len(conn), len(order))
    with pytest.raises(_capi.PlError) as e:
        _capi.cells_recover(xyz, conn, order, rad, sl, sn, np.zeros(6 * len(order)), E, NU)
    assert e.value.code == _capi.PL_ERR_ARG
    rng = np.random.default_rng(13)
    ub, lb = rng.standard_normal(6 * len(order)), rng.standard_normal(6 * len(order))
    u, lam, sens, batched = _recover_any(L, ub, lb)
    assert not batched
    interior = np.setdiff1d(np.arange(len(xyz)), order)
    assert len(interior) > 0
    assert np.array_equal(u[order].ravel(), ub) and np.array_equal(lam[order].ravel(), lb)
    K = _oracle_K(xyz, conn, rad, sl, sn)
    bd, it = _dofs(order), _dofs(interior)
    for full, vb in ((u, ub), (lam, lb)):
        ref = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)] @ vb)
        err = _rel(full[interior].ravel(), ref)
        print("Diamond+Kelvin fallback: interior vs oracle", err)
        assert err < 1e-8
    with _capi.HipLattice(xyz, conn, rad, sl, sn, E, NU, precond=5) as dev:
        dev.assemble()
        u0 = np.zeros_like(u)
        u0[order] = u[order]
        g = dev.spmv(u0)[interior]
        assert np.linalg.norm(dev.spmv(u)[interior]) < 1e-8 * np.linalg.norm(g)
        ref_s = dev.sens(u, lam)
        print("Diamond+Kelvin fallback: sens vs pl_sens", np.abs(sens - ref_s).max() / np.abs(ref_s).max())
        assert np.abs(sens - ref_s).max() < 1e-12 * np.abs(ref_s).max()
        ref_uu = dev.sens(u)
    src = {"xyz": xyz, "radius": rad, "seg_len": sl, "seg_nsub": sn}
    u2, lam2, s2 = L._recover_cell_by_solve(src, conn, order, ub, None, True)        # lam = u
    assert lam2 is None and _rel(u2, u) < 1e-9 and np.abs(s2 - ref_uu).max() < 1e-8 * np.abs(ref_uu).max()
    u3, lam3, s3 = L._recover_cell_by_solve(src, conn, order, np.zeros_like(ub), lb, True)   # a zero state
    assert not u3.any() and not s3.any() and _rel(lam3, lam) < 1e-9
    u4, _, s4 = L._recover_cell_by_solve(src, conn, order, ub, None, False)
    assert s4 is None and _rel(u4, u) < 1e-9
    if L._device is not None:
        L._device.close()


def test_lattice_of_over_limit_cells_through_recover_cell_interiors():
    """2 x 1 x 1 Diamond + Kelvin in exact DDM mode, one radius set per cell: recover_cell_interiors(want_sens=True) takes the
    per-cell fallback for both cells.  Interior rows against the oracle on each cell's own struts (1e-8); the per-cell
    sensitivities against pl_sens on the recovered state and the oracle's adjoint field (1e-7 of max |sens|: bilinear in two
    fields that each carry up to 1e-8); the lattice-wide array is the sum of the cells' values on their strut indices."""
    L = LatticeSim(_lattice_preset(["Diamond", "Kelvin"], [0.03, 0.03], cells=(2, 1, 1)),
                   enable_domain_decomposition_solver=True)
    L.set_cell_radii([[0.03, 0.03], [0.035, 0.028]])
    assert L.schur_complements.shape[0] == 2 and L.schur_complements.shape[1] > 6 * _capi.SCHUR_CELLS_MAX_BOUNDARY
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
        assert len(interior) > 0
        K = _oracle_K(lat.node_xyz[nodes], conn, lat.beam_radius[beams], pen.seg_len[beams], pen.seg_nsub[beams])
        bd, it = _dofs(order), _dofs(interior)
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
        print("cell", c, "sens against pl_sens", np.abs(s - ref).max() / np.abs(ref).max())
        assert np.abs(s - ref).max() < 1e-7 * np.abs(ref).max()
        np.add.at(expect, beams, s)
    assert np.array_equal(sens, expect)


def _type_sums(L, sens):
    bt = L.lattice.beam_type
    return np.array([sens[bt == j].sum() for j in range(len(L.geom_types))])


@pytest.mark.parametrize("geoms,radii", [(["BCC", "Hybrid1", "Hybrid4"], [0.03, 0.04, 0.05]),
                                         (["BCC", "Hybrid1"], [0.05, 0.03]), (["Kelvin", "BCC"], [0.03, 0.045])],
                         ids=["triple", "BCC+Hybrid1", "Kelvin+BCC"])
def test_sens_against_central_differences_of_the_schur_complement(geoms, radii):
    """Item 4: for every radius parameter j, sum over the struts of type j of sens against
    lam_b^T [(S(r + h) - S(r - h)) / (2 h)] u_b, h = max(1e-8, 1e-6 max(1, |r|)), both S from pl_schur_cells at fixed
    segment geometry: relative 1e-5."""
    L = _cell(geoms, radii)
    xyz, conn, rad, sl, sn, order = _arrays(L)
    rng = np.random.default_rng(5)
    ub, lb = rng.standard_normal(6 * len(order)), rng.standard_normal(6 * len(order))
    out = _capi.cells_recover(xyz, conn, order, rad, sl, sn, ub, E, NU, lam_b=lb, want=("sens",))
    assert out["info"][0] == 0 and set(out) == {"sens", "info"}
    got = _type_sums(L, out["sens"][0])
    bt = L.lattice.beam_type
    for j, rj in enumerate(radii):
        h = max(1e-8, 1e-6 * max(1.0, abs(rj)))
        rads = np.stack([rad, rad])
        rads[0, bt == j] = rj + h
        rads[1, bt == j] = rj - h
        S, info = _capi.schur_cells(xyz, conn, order, rads, sl, sn, E, NU)
        assert (info == 0).all()
        fd = float(lb @ ((S[0] - S[1]) / (2 * h)) @ ub)
        print(geoms, j, "analytic", got[j], "central difference", fd, "rel", abs(got[j] - fd) / abs(fd))
        assert abs(got[j] - fd) < 1e-5 * abs(fd), (geoms, j)
    # lam = u when no adjoint is given
    o2 = _capi.cells_recover(xyz, conn, order, rad, sl, sn, ub, E, NU, want=("lam", "u", "sens"))
    assert np.array_equal(o2["lam"], o2["u"])


def test_bitwise_reproducible_wherever_the_instance_sits():
    L = _cell(["BCC", "Hybrid1", "Hybrid4"], [0.03, 0.04, 0.05])
    xyz, conn, rad, sl, sn, order = _arrays(L)
    rng = np.random.default_rng(7)
    n = 1000
    scale = rng.uniform(0.5, 1.5, size=(n, 1))
    rads = rad[None, :] * scale
    rads[0] = rads[n - 1] = rad
    ub, lb = rng.standard_normal(6 * len(order)), rng.standard_normal(6 * len(order))
    alone = _capi.cells_recover(xyz, conn, order, rad, sl, sn, ub, E, NU, lam_b=lb)
    a = _capi.cells_recover(xyz, conn, order, rads, sl, sn, ub, E, NU, lam_b=lb)
    b = _capi.cells_recover(xyz, conn, order, rads, sl, sn, ub, E, NU, lam_b=lb)
    assert (a["info"] == 0).all() and alone["info"][0] == 0
    for k in ("u", "lam", "sens"):
        assert np.isfinite(a[k]).all()
        assert np.array_equal(a[k][0], alone[k][0]) and np.array_equal(a[k][n - 1], alone[k][0])
        assert np.array_equal(a[k], b[k])


def test_bad_instances_are_reported_alone():
    L = _cell(["BCC"], [0.04])
    xyz, conn, rad, sl, sn, order = _arrays(L)
    # the BCC cell plus an interior node Z hanging off the centre node C by one strut
    c = int(np.setdiff1d(np.arange(len(xyz)), order)[0])
    xyz2 = np.vstack([xyz, xyz[c] + [0.0, 0.0, 0.2]])
    conn2 = np.vstack([conn, [c, len(xyz)]])
    rad2, sl2, sn2 = np.append(rad, 0.04), np.vstack([sl, [0.0, 0.2, 0.0]]), np.vstack([sn, [0, 4, 0]])
    rads = np.tile(rad2, (4, 1))
    rads[1, 0] = 0.0                      # a zero radius
    rads[2, :-1] = 1e-9                   # C's struts to the boundary vanish: C and Z float together
    ub = np.random.default_rng(3).standard_normal(6 * len(order))
    out = _capi.cells_recover(xyz2, conn2, order, rads, sl2, sn2, ub, E, NU)
    info = out["info"]
    assert info[1] == -1 and info[2] > 0 and info[0] == 0 and info[3] == 0
    for k in ("u", "lam", "sens"):
        assert np.isnan(out[k][1]).all() and np.isnan(out[k][2]).all()
        assert np.isfinite(out[k][0]).all() and np.array_equal(out[k][0], out[k][3])
    K = _oracle_K(xyz2, conn2, rad2, sl2, sn2)
    interior = np.setdiff1d(np.arange(len(xyz2)), order)
    bd, it = _dofs(order), _dofs(interior)
    ref = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)] @ ub)
    assert _rel(out["u"][0][interior].ravel(), ref) < 1e-10
    # 33 boundary nodes: a chain of 34 nodes
    xyz3 = np.stack([np.arange(34) * 0.1, np.zeros(34), np.zeros(34)], axis=1)
    conn3 = np.stack([np.arange(33), np.arange(1, 34)], axis=1)
    with pytest.raises(_capi.PlError) as e:
        _capi.cells_recover(xyz3, conn3, np.arange(33), np.full(33, 0.02), np.tile([0.0, 0.1, 0.0], (33, 1)),
                            np.tile([0, 2, 0], (33, 1)), np.zeros(6 * 33), E, NU)
    assert e.value.code == _capi.PL_ERR_ARG
    # a cell without interior nodes is legal: nothing to solve, the sensitivities are still those of pl_sens
    xyz4 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float)
    conn4 = np.array([[0, 1], [1, 2], [2, 0]])
    rad4 = np.array([0.03, 0.04, 0.05])
    len4 = np.linalg.norm(xyz4[conn4[:, 1]] - xyz4[conn4[:, 0]], axis=1)
    sl4, sn4 = np.stack([0 * len4, len4, 0 * len4], axis=1), np.tile([0, 6, 0], (3, 1))
    u4 = np.random.default_rng(4).standard_normal(18)
    o4 = _capi.cells_recover(xyz4, conn4, np.array([2, 0, 1]), rad4, sl4, sn4, u4, E, NU)
    assert o4["info"][0] == 0 and np.array_equal(o4["u"][0][[2, 0, 1]].ravel(), u4)
    with _capi.HipLattice(xyz4, conn4, rad4, sl4, sn4, E, NU) as dev:
        dev.assemble()
        ref4 = dev.sens(o4["u"][0])
    assert np.abs(o4["sens"][0] - ref4).max() < 1e-12 * np.abs(ref4).max()


def _lattice_preset(geoms, radii, cells=(3, 2, 2), ddm=True):
    p = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                      "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                      "radii": list(radii), "geom_types": list(geoms)},
         "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
         "boundary_conditions": {
             "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                        "Value": [0, 0, 0, 0, 0, 0]}},
             "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}}
    if ddm:
        p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 5000,
                                             "schur_complement_computation": {"type": "exact"}}
    return p


def _twelve_radius_sets():
    rng = np.random.default_rng(21)
    return np.stack([0.03 + 0.03 * rng.random(12), 0.025 + 0.02 * rng.random(12)], axis=1)


def _interior_rows(L):
    mask = np.ones(L.lattice.n_nodes, bool)
    mask[np.unique(L.cell_boundary_nodes())] = False
    return np.flatnonzero(mask)


def test_fem_field_in_fem_field_out():
    """Item 7: 3 x 2 x 2 BCC + Hybrid1, penalised, 12 radius sets; every cell is fed the FEM displacements of its boundary
    nodes and must give back the FEM displacements of its interior nodes, to 1e-7 of ||u|| (the FEM solver's own bar)."""
    radii = _twelve_radius_sets()
    Lf = LatticeSim(_lattice_preset(["BCC", "Hybrid1"], [0.04, 0.03], ddm=False))
    Lf.set_cell_radii(radii)
    _, model = solve_FEM_FenicsX(Lf)
    Ld = LatticeSim(_lattice_preset(["BCC", "Hybrid1"], [0.04, 0.03]), enable_domain_decomposition_solver=True)
    Ld.set_cell_radii(radii)
    assert Ld.schur_complements.shape[0] == 12
    assert np.array_equal(Ld.lattice.beam_conn, Lf.lattice.beam_conn)
    rows = _interior_rows(Ld)
    assert len(rows) >= 12
    bnd = np.setdiff1d(np.arange(Ld.lattice.n_nodes), rows)
    Ld.displacement_vector[:] = 0.0
    Ld.displacement_vector[bnd] = model.u[bnd]
    Ld.recover_cell_interiors()
    assert np.array_equal(Ld.displacement_vector[bnd], model.u[bnd])
    err = np.linalg.norm(Ld.displacement_vector[rows] - model.u[rows]) / np.linalg.norm(model.u)
    print("interior rows against the FEM field:", err)
    assert err < 1e-7


def test_through_solve_ddm(tmp_path):
    """Item 8."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "src"))
    from pyLatticeSim.export_simulation_results import exportSimulationResults
    radii = _twelve_radius_sets()
    Lf = LatticeSim(_lattice_preset(["BCC", "Hybrid1"], [0.04, 0.03], ddm=False))
    Lf.set_cell_radii(radii)
    _, model = solve_FEM_FenicsX(Lf)
    Ld = LatticeSim(_lattice_preset(["BCC", "Hybrid1"], [0.04, 0.03]), enable_domain_decomposition_solver=True)
    Ld.set_cell_radii(radii)
    xs0, info0, _, _ = Ld.solve_DDM()
    rows = _interior_rows(Ld)
    assert info0 == 0 and not Ld.displacement_vector[rows].any()          # default: interiors stay as they were
    xs, info, _, _ = Ld.solve_DDM(recover_interior=True)
    assert info == 0 and np.array_equal(xs, xs0)
    bnd = np.setdiff1d(np.arange(Ld.lattice.n_nodes), rows)
    nrm = np.linalg.norm(model.u)
    e_int = np.linalg.norm(Ld.displacement_vector[rows] - model.u[rows]) / nrm
    e_bnd = np.linalg.norm(Ld.displacement_vector[bnd] - model.u[bnd]) / nrm
    print("DDM against FEM: interior rows", e_int, "boundary rows", e_bnd)
    assert e_int <= 10 * e_bnd
    # one radius set: the representative's matrix serves every cell; the recovered field carries the energy of the
    # operator solve_DDM solved
    L1 = LatticeSim(_lattice_preset(["BCC", "Hybrid1"], [0.04, 0.03]), enable_domain_decomposition_solver=True)
    assert L1.schur_complements.shape[0] == 1
    _, info1, _, _ = L1.solve_DDM(recover_interior=True)
    assert info1 == 0
    lat = L1.lattice
    cb = L1.cell_boundary_nodes()
    src = L1._schur_cell_data[0]
    e_full = e_schur = 0.0
    with _capi.HipLattice(src["xyz"], src["conn"], src["radius"], src["seg_len"], src["seg_nsub"], E, NU) as dev:
        dev.assemble()
        for c in range(lat.n_cells):
            beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
            nodes = np.unique(lat.beam_conn[beams])
            uc = L1.displacement_vector[nodes]
            e_full += float((uc * dev.spmv(uc)).sum())
            ub = L1.displacement_vector[cb[c]].ravel()
            e_schur += float(ub @ L1.schur_complements[0] @ ub)
    print("energy of the recovered field", e_full, "of the condensed operator", e_schur)
    assert abs(e_full - e_schur) < 1e-10 * abs(e_schur)
    # penalisation points and the export work as after a FEM solve
    for L in (Ld, L1):
        pts = L._node_mod_rows("displacement_vector")
        assert np.isfinite(pts).all()
        from pylatticedso_amd.views import _tables
        t = _tables(L)
        centre = rows[0]                                                   # a BCC centre node ...
        near = np.flatnonzero((L.lattice.beam_conn[t.pen_strut] == centre).any(axis=1))
        assert len(near) >= 2 and np.abs(pts[near]).max(axis=1).min() > 0  # ... and the points on its struts moved
        ex = exportSimulationResults(L.ddm_result_model(), "ddm", out_dir=str(tmp_path))
        ex.full_export()
        assert os.path.exists(ex.pvd_path)


def _opti_preset(geoms, radii, cells, objective_type, ddm, gradient=None):
    p = _lattice_preset(geoms, radii, cells, ddm=ddm)
    p["boundary_conditions"]["Force"] = {"Load": {"Surface": ["Xmax", "Zmax"], "DOF": ["Z"], "Value": [-0.1]}}
    info = {"objective_function": "min", "objective_type": objective_type, "max_iterations": 5,
            "optimization_parameters": {"type": "unit_cell", "hybrid": False},
            "constraints": {"relative_density": {"value": 0.05}},
            "enable_parameter_normalization": True, "enable_gradient_computing": True,
            "simulation_type": "DDM" if ddm else "FEM"}
    if objective_type == "displacement":
        info["objective_data"] = {"Surface": ["Xmax"], "DOF": ["Z"]}
    if objective_type == "displacement_ratio":
        info["objective_data"] = {"Surface": ["Zmax"], "DOF": ["Z"]}
    p["optimization_informations"] = info
    if gradient is not None:
        p["simulation_parameters"]["DDM"]["schur_complement_computation"]["gradient"] = gradient
    return p


@pytest.mark.parametrize("objective_type", ["compliance", "displacement", "displacement_ratio"])
@pytest.mark.parametrize("geoms,radii,cells", [(["BCC"], [0.05], (3, 1, 1)),
                                               (["BCC", "Hybrid1", "Hybrid4"], [0.04, 0.03, 0.035], (3, 2, 2))],
                         ids=["bcc3x1x1", "triple3x2x2"])
def test_lattice_opti_analytic_gradient(geoms, radii, cells, objective_type):
    """Item 9: gradient() with ddm_gradient="analytic" against "finite_difference" (1e-5), against the FEM-mode gradient
    and central differences of objective() (2e-3; on every parameter of the 3-parameter case, on 6 of the 36 of the
    3 x 2 x 2 case, drawn with a fixed seed, to bound the run time); objective() identical in both modes; no dS/dr matrices in analytic mode;
    the default stays the finite-difference path."""
    La = LatticeOpti(_opti_preset(geoms, radii, cells, objective_type, True), ddm_gradient="analytic")
    Lp = LatticeOpti(_opti_preset(geoms, radii, cells, objective_type, True, gradient="analytic"))
    Ld = LatticeOpti(_opti_preset(geoms, radii, cells, objective_type, True))
    Lf = LatticeOpti(_opti_preset(geoms, radii, cells, objective_type, False))
    assert La.ddm_gradient == Lp.ddm_gradient == "analytic" and Ld.ddm_gradient == "finite_difference"
    n = La.number_parameters
    x = list(0.3 + 0.5 * np.random.default_rng(2).random(n))
    oa, od = La.objective(x), Ld.objective(x)
    assert np.array_equal(oa, od) and np.array_equal(La.schur_complements, Ld.schur_complements)
    Lp.objective(x)
    Lf.objective(x)
    ga, gp, gd, gf = (np.asarray(L.gradient(x)) for L in (La, Lp, Ld, Lf))
    assert La.schur_gradients is None and Lp.schur_gradients is None
    assert Ld.schur_gradients is not None and len(Ld.schur_gradients) == Ld.schur_complements.shape[0]
    assert np.array_equal(ga, gp)
    print(objective_type, geoms, "analytic vs finite difference", _rel(ga, gd), "vs FEM", _rel(ga, gf))
    assert _rel(ga, gd) < 1e-5
    assert _rel(ga, gf) < 2e-3
    h = 1e-4
    idx = np.arange(n) if n <= 6 else np.random.default_rng(9).choice(n, 6, replace=False)
    fd = np.zeros(len(idx))
    for k, i in enumerate(idx):
        xp, xm = list(x), list(x)
        xp[i] += h
        xm[i] -= h
        fd[k] = (La.objective(xp) - La.objective(xm)) / (2 * h)
    print(objective_type, geoms, "analytic vs central differences of objective()", _rel(ga[idx], fd))
    assert np.linalg.norm(ga[idx] - fd) < 2e-3 * np.linalg.norm(fd)


def test_analytic_mode_needs_exact_matrices(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "opti_ddm.npz"))
    preset = json.loads(str(g["unit_cell_displacement_preset_json"]))
    with pytest.raises(ValueError):
        LatticeOpti(copy.deepcopy(preset), data_roots=[golden_dir], ddm_gradient="analytic")
    with pytest.raises(ValueError):
        LatticeOpti(copy.deepcopy(preset), data_roots=[golden_dir], ddm_gradient="exact")
    L = LatticeSim(preset, enable_domain_decomposition_solver=True, data_roots=[golden_dir])
    with pytest.raises(NotImplementedError):
        L.recover_cell_interiors()
