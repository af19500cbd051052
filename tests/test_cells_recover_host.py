"""Host side of the cell recovery (pl_cells_recover), no GPU: the wrapper's argument checks, the C ABI without a device,
and how LatticeSim.recover_cell_interiors / LatticeOpti's analytic gradient mode group cells, choose the strut data they
send and place the results - with numpy stand-ins built on the oracle in place of the device calls."""
import os

import numpy as np
import pytest

from oracle import timoshenko_oracle as O
from pylatticedso_amd import _capi

E, NU = 1013.0, 0.3


def _bcc_cell_arrays():
    xyz = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)] + [[0.5, 0.5, 0.5]], float)
    conn = np.array([[k, 8] for k in range(8)], np.int32)
    L = np.sqrt(0.75)
    return xyz, conn, np.arange(8), np.full(8, 0.05), np.tile([0.0, L, 0.0], (8, 1)), np.tile([0, 10, 0], (8, 1))


def test_wrapper_argument_checks():
    xyz, conn, bn, rad, sl, sn = _bcc_cell_arrays()
    ub = np.zeros(48)
    with pytest.raises(ValueError):                  # connectivity must be (B, 2) integers
        _capi.cells_recover(xyz, conn.astype(float), bn, rad, sl, sn, ub, E, NU)
    with pytest.raises(ValueError):                  # boundary list must be 1-D integers
        _capi.cells_recover(xyz, conn, bn.astype(float), rad, sl, sn, ub, E, NU)
    with pytest.raises(ValueError):
        _capi.cells_recover(xyz, conn, bn.reshape(2, 4), rad, sl, sn, ub, E, NU)
    with pytest.raises(ValueError):                  # per-strut array of the wrong length
        _capi.cells_recover(xyz, conn, bn, rad[:-1], sl, sn, ub, E, NU)
    with pytest.raises(ValueError):
        _capi.cells_recover(xyz, conn, bn, rad, sl, sn.astype(float), ub, E, NU)
    with pytest.raises(ValueError):                  # boundary values: 6 per boundary node
        _capi.cells_recover(xyz, conn, bn, rad, sl, sn, ub[:-1], E, NU)
    with pytest.raises(ValueError):
        _capi.cells_recover(xyz, conn, bn, rad, sl, sn, ub, E, NU, lam_b=np.zeros(47))
    with pytest.raises(ValueError):                  # leading axes of per-instance arrays disagree
        _capi.cells_recover(xyz, conn, bn, np.stack([rad] * 2), sl, sn, np.zeros((3, 48)), E, NU)
    with pytest.raises(ValueError):
        _capi.cells_recover(xyz, conn, bn, rad, sl, sn, np.zeros((3, 48)), E, NU, lam_b=np.zeros((2, 48)))
    for want in ((), ("u", "S"), "reactions"):       # what to return
        with pytest.raises(ValueError):
            _capi.cells_recover(xyz, conn, bn, rad, sl, sn, ub, E, NU, want=want)


def _library():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.load_library()


def test_no_device_and_bad_arguments_from_the_library():
    import ctypes as C
    import torch
    lib = _library()
    xyz, conn, bn, rad, sl, sn = _bcc_cell_arrays()
    bn = bn.astype(np.int32)
    sn = np.ascontiguousarray(sn, np.int32)
    ub, uf, sens = np.zeros(48), np.empty(54), np.empty(8)
    info = np.empty(1, np.int32)
    p = _capi._ptr
    opts = _capi.default_opts(lib)

    def call(opts=opts, n_inst=1, nb=8, bnodes=bn, conn=conn, n_nodes=9, u_b=ub, u_full=uf, sens=sens, info=info):
        return lib.pl_cells_recover(C.byref(opts), n_inst, n_nodes, len(conn), p(conn), nb, p(bnodes), p(xyz), p(rad),
                                    p(sl), p(sn), p(u_b), None, p(u_full), None, p(sens), p(info))

    # argument errors are reported whether or not a device is there
    assert call(n_inst=0) == _capi.PL_ERR_ARG
    assert call(u_b=None) == _capi.PL_ERR_ARG and call(info=None) == _capi.PL_ERR_ARG          # null pointers
    assert call(u_full=None, sens=None) == _capi.PL_ERR_ARG                                     # nothing asked for
    assert call(bnodes=np.array([0, 1, 2, 3, 4, 5, 6, 9], np.int32)) == _capi.PL_ERR_ARG      # out of range
    assert call(bnodes=np.array([0, 1, 2, 3, 4, 5, 6, 6], np.int32)) == _capi.PL_ERR_ARG      # listed twice
    assert call(conn=np.array([[0, 8]] * 7 + [[8, 8]], np.int32)) == _capi.PL_ERR_ARG          # strut on one node
    assert call(nb=33, n_nodes=34) == _capi.PL_ERR_ARG                                          # over the limits
    assert call(nb=8, n_nodes=8 + 17) == _capi.PL_ERR_ARG
    assert b"too large" in lib.pl_last_error()
    raw = _capi.PlOpts()                                                                        # not stamped
    assert call(opts=raw) == _capi.PL_ERR_ARG
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert call() == _capi.PL_ERR_NODEVICE
    assert call(u_full=None) == _capi.PL_ERR_NODEVICE                                           # a subset of the outputs
    for kw in ({}, {"lam_b": ub}, {"want": ("sens",)}, {"want": "u"}):
        with pytest.raises(_capi.PlError) as e:
            _capi.cells_recover(xyz, conn, bn, rad, sl, sn, ub, E, NU, **kw)
        assert e.value.code == _capi.PL_ERR_NODEVICE


# ---------------------------------------------------------------------------------------------------------------------
# LatticeSim / LatticeOpti with stand-ins for the two device calls
# ---------------------------------------------------------------------------------------------------------------------
def _K(xyz, conn, rad, seg_len, seg_nsub):
    sc = np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(rad, seg_len, seg_nsub)])
    return np.asarray(O.assemble_condensed(xyz, conn, sc).todense())


def _split(n_nodes, order):
    interior = np.setdiff1d(np.arange(n_nodes), order)
    dofs = lambda nodes: (6 * np.asarray(nodes)[:, None] + np.arange(6)).ravel()      # noqa: E731
    return interior, dofs(order), dofs(interior)


class _Schur:
    """Stands in for _capi.schur_cells: the oracle's Schur complement of every instance."""

    def __init__(self):
        self.calls = []

    def __call__(self, node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, young, poisson, **kw):
        rad = np.asarray(beam_radius)
        self.calls.append(dict(rad=rad, conn=np.asarray(beam_conn), order=np.asarray(boundary_nodes)))
        out = []
        for i in range(len(rad)):
            sc = np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(rad[i], seg_len[i], seg_nsub[i])])
            K = O.assemble_condensed(node_xyz[i], beam_conn, sc)
            out.append(np.asarray(O.schur_complement(K, _split(len(node_xyz[i]), boundary_nodes)[1])))
        return np.stack(out), np.zeros(len(rad), np.int32)


class _Recover:
    """Stands in for _capi.cells_recover: interiors by the oracle; sens[i, b] = 1000 radius[i, b] + b + u_b[i, 0]."""

    def __init__(self):
        self.calls = []

    def __call__(self, node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, u_b, young, poisson,
                 lam_b=None, want=("u", "lam", "sens"), **kw):
        rad, ub = np.asarray(beam_radius), np.asarray(u_b)
        self.calls.append(dict(xyz=np.asarray(node_xyz), conn=np.asarray(beam_conn), order=np.asarray(boundary_nodes),
                               rad=rad, seg_len=np.asarray(seg_len), seg_nsub=np.asarray(seg_nsub), u_b=ub,
                               lam_b=None if lam_b is None else np.asarray(lam_b), want=tuple(want), kw=kw,
                               young=young, poisson=poisson))
        n = node_xyz.shape[1]
        interior, bd, it = _split(n, boundary_nodes)
        u = np.zeros((len(rad), n, 6))
        for i in range(len(rad)):
            K = _K(node_xyz[i], beam_conn, rad[i], seg_len[i], seg_nsub[i])
            u[i][boundary_nodes] = ub[i].reshape(-1, 6)
            if len(interior):
                u[i][interior] = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)] @ ub[i]).reshape(-1, 6)
        out = {"info": np.zeros(len(rad), np.int32)}
        if "u" in want:
            out["u"] = u
        if "sens" in want:
            out["sens"] = 1000.0 * rad + np.arange(rad.shape[1])[None, :] + ub[:, :1]
        return out


def _ddm_preset(cells=(3, 1, 1), geoms=("BCC",), radii=(0.05,), kind="exact"):
    comp = {"type": kind} if kind == "exact" else {"type": kind, "precision_greedy": 1e-6}
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                         "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                         "radii": list(radii), "geom_types": list(geoms)},
            "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                      "DDM": {"enable_preconditioner": False, "max_iterations": 5000,
                                              "schur_complement_computation": comp}},
            "boundary_conditions": {
                "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                           "Value": [0, 0, 0, 0, 0, 0]}},
                "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}}


def _cell_parts(L, c):
    lat = L.lattice
    beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
    return beams, np.unique(lat.beam_conn[beams])


def test_recover_groups_by_topology_and_sends_the_representatives_strut_data(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    schur, rec = _Schur(), _Recover()
    monkeypatch.setattr(_capi, "schur_cells", schur)
    monkeypatch.setattr(_capi, "cells_recover", rec)
    L = LatticeSim(_ddm_preset((4, 1, 1)), enable_domain_decomposition_solver=True)
    L.set_cell_radii([[0.03], [0.05], [0.03], [0.07]])
    assert list(L.cell_schur_index) == [0, 1, 0, 2] and len(L._schur_cell_data) == 3
    lat, pen = L.lattice, L.penalized
    cb = L.cell_boundary_nodes()
    rng = np.random.default_rng(0)
    bnd = np.unique(cb)
    interior = np.setdiff1d(np.arange(lat.n_nodes), bnd)
    assert len(interior) == 4
    L.displacement_vector[:] = 0.0
    L.displacement_vector[bnd] = rng.standard_normal((len(bnd), 6))
    before = L.displacement_vector.copy()
    lam = rng.standard_normal(before.shape)
    sens = L.recover_cell_interiors(lam=lam, want_sens=True)
    # one topology (every BCC cell has the same connectivity and boundary order): one call, one instance per cell
    assert len(rec.calls) == 1
    call = rec.calls[0]
    assert call["rad"].shape == (4, 8) and call["want"] == ("u", "sens")
    assert call["young"] == L.young_modulus and call["kw"]["pen_coef"] == L.penalization_coefficient
    reps = [0, 1, 0, 3]                      # the cell whose strut data each cell is sent with
    for c in range(4):
        beams_r, nodes_r = _cell_parts(L, reps[c])
        assert np.array_equal(call["rad"][c], lat.beam_radius[beams_r])
        assert np.array_equal(call["xyz"][c], lat.node_xyz[nodes_r])
        assert np.array_equal(call["seg_len"][c], pen.seg_len[beams_r])
        assert np.array_equal(call["seg_nsub"][c], pen.seg_nsub[beams_r])
        assert np.array_equal(call["u_b"][c], before[cb[c]].ravel())          # ... with the cell's OWN boundary values
        assert np.array_equal(call["lam_b"][c], lam[cb[c]].ravel())
        _, nodes = _cell_parts(L, c)
        assert np.array_equal(nodes[call["order"]], cb[c])
    # cell 2 has cell 0's radii but not its penalised segments (an inner cell against a corner cell): the representative's
    # data is what was sent, deliberately
    assert not np.array_equal(pen.seg_len[_cell_parts(L, 2)[0]], pen.seg_len[_cell_parts(L, 0)[0]])
    # interior rows written, boundary rows untouched
    assert np.array_equal(L.displacement_vector[bnd], before[bnd])
    for c in range(4):
        beams_r, nodes_r = _cell_parts(L, reps[c])
        _, nodes = _cell_parts(L, c)
        K = _K(lat.node_xyz[nodes_r], call["conn"], lat.beam_radius[beams_r], pen.seg_len[beams_r], pen.seg_nsub[beams_r])
        it_local, bd, it = _split(len(nodes), call["order"])
        ref = -np.linalg.solve(K[np.ix_(it, it)], K[np.ix_(it, bd)] @ before[cb[c]].ravel())
        assert np.allclose(L.displacement_vector[nodes[it_local]].ravel(), ref, rtol=1e-12, atol=0)
    # sensitivities on the lattice's strut indices
    expect = np.zeros(lat.n_beams)
    for c in range(4):
        beams, _ = _cell_parts(L, c)
        s = 1000.0 * lat.beam_radius[_cell_parts(L, reps[c])[0]] + np.arange(8) + before[cb[c]].ravel()[0]
        np.add.at(expect, beams, s)
        assert np.array_equal(L.cell_strut_sens[c][0], beams) and np.array_equal(L.cell_strut_sens[c][1], s)
    assert np.array_equal(sens, expect)
    # without sensitivities: only the field is asked for, nothing is returned
    rec.calls.clear()
    assert L.recover_cell_interiors() is None
    assert rec.calls[0]["want"] == ("u",) and rec.calls[0]["lam_b"] is None


def test_two_topologies_make_two_calls(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    monkeypatch.setattr(_capi, "schur_cells", _Schur())
    rec = _Recover()
    monkeypatch.setattr(_capi, "cells_recover", rec)
    L = LatticeSim(_ddm_preset((2, 1, 1)), enable_domain_decomposition_solver=True)
    # renumber the struts of cell 1 inside the cell -> strut table: same cell, another connectivity array
    lat = L.lattice
    seg = slice(lat.cell_beam_ptr[1], lat.cell_beam_ptr[2])
    lat.cell_beam_idx[seg] = lat.cell_beam_idx[seg][::-1].copy()
    L.displacement_vector[:] = np.random.default_rng(1).standard_normal(L.displacement_vector.shape)
    L.recover_cell_interiors()
    assert len(rec.calls) == 2 and all(c["rad"].shape[0] == 1 for c in rec.calls)
    # cell 1 is no longer numbered like its representative (cell 0): it was sent with its own strut data
    beams1, nodes1 = _cell_parts(L, 1)
    assert np.array_equal(rec.calls[1]["rad"][0], lat.beam_radius[beams1])
    assert np.array_equal(rec.calls[1]["xyz"][0], lat.node_xyz[nodes1])


def test_cells_beyond_the_kernel_take_the_per_cell_solve(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    monkeypatch.setattr(_capi, "schur_cells", _Schur())
    rec = _Recover()
    monkeypatch.setattr(_capi, "cells_recover", rec)
    L = LatticeSim(_ddm_preset((3, 1, 1)), enable_domain_decomposition_solver=True)
    L.set_cell_radii([[0.03], [0.05], [0.03]])
    monkeypatch.setattr(_capi, "schur_cells_fits", lambda *a: False)
    seen = []

    def by_solve(self, src, conn, order, ub, lb, want_sens):
        seen.append(dict(src=src, conn=conn, order=order, ub=ub, lb=lb, want_sens=want_sens))
        k = len(seen)
        n = len(src["xyz"])
        u = np.full((n, 6), float(k))
        u[order] = np.asarray(ub).reshape(-1, 6)
        return u, None if lb is None else u + 1.0, (np.arange(len(conn)) + 100.0 * k if want_sens else None)

    monkeypatch.setattr(LatticeSim, "_recover_cell_by_solve", by_solve)
    lat = L.lattice
    cb = L.cell_boundary_nodes()
    bnd = np.unique(cb)
    L.displacement_vector[:] = 0.0
    L.displacement_vector[bnd] = np.random.default_rng(4).standard_normal((len(bnd), 6))
    before = L.displacement_vector.copy()
    lam = np.random.default_rng(5).standard_normal(before.shape)
    sens = L.recover_cell_interiors(lam=lam, want_sens=True)
    assert not rec.calls and len(seen) == 3 and all(c["want_sens"] for c in seen)
    reps = [0, 1, 0]
    expect = np.zeros(lat.n_beams)
    for c in range(3):
        beams_r, nodes_r = _cell_parts(L, reps[c])
        beams, nodes = _cell_parts(L, c)
        assert np.array_equal(seen[c]["src"]["radius"], lat.beam_radius[beams_r])        # the representative's strut data
        assert np.array_equal(seen[c]["src"]["xyz"], lat.node_xyz[nodes_r])
        assert np.array_equal(seen[c]["ub"], before[cb[c]].ravel()) and np.array_equal(seen[c]["lb"], lam[cb[c]].ravel())
        assert np.array_equal(nodes[seen[c]["order"]], cb[c])
        interior = np.setdiff1d(nodes, cb[c])
        assert np.array_equal(L.displacement_vector[interior], np.full((len(interior), 6), c + 1.0))
        assert np.array_equal(L.cell_strut_sens[c][1], np.arange(8) + 100.0 * (c + 1))
        np.add.at(expect, beams, L.cell_strut_sens[c][1])
    assert np.array_equal(L.displacement_vector[bnd], before[bnd]) and np.array_equal(sens, expect)
    seen.clear()
    assert L.recover_cell_interiors() is None
    assert len(seen) == 3 and not any(c["want_sens"] for c in seen) and all(c["lb"] is None for c in seen)


def test_surrogate_and_installed_matrices_cannot_be_recovered(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    monkeypatch.setattr(_capi, "schur_cells", _Schur())
    L = LatticeSim(_ddm_preset(), enable_domain_decomposition_solver=True)
    L.set_schur_complements(L.schur_complements[0])             # matrices from elsewhere: no strut data behind them
    with pytest.raises(ValueError):
        L.recover_cell_interiors()
    L.calculate_schur_complement_cells()
    L.type_schur_complement_computation = "RBF"                 # a surrogate mode
    with pytest.raises(NotImplementedError):
        L.recover_cell_interiors()


def _opti_preset(**kw):
    p = _ddm_preset((3, 1, 1), ("BCC", "Hybrid1"), (0.05, 0.04))
    p["optimization_informations"] = {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": 5,
        "optimization_parameters": {"type": "unit_cell", "hybrid": False},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "DDM"}
    p["simulation_parameters"]["DDM"]["schur_complement_computation"].update(kw)
    return p


def test_analytic_mode_condenses_every_representative_once(monkeypatch):
    from pylatticedso_amd.lattice_opti import LatticeOpti
    schur, rec = _Schur(), _Recover()
    monkeypatch.setattr(_capi, "schur_cells", schur)
    monkeypatch.setattr(_capi, "cells_recover", rec)
    x = [0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    counts = {}
    for mode, L in (("finite_difference", LatticeOpti(_opti_preset())),
                    ("analytic", LatticeOpti(_opti_preset(), ddm_gradient="analytic")),
                    ("preset", LatticeOpti(_opti_preset(gradient="analytic")))):
        assert L.ddm_gradient == ("finite_difference" if mode == "finite_difference" else "analytic")
        schur.calls.clear()
        L.set_optimization_parameters(x)
        L._flush_schur()
        assert len(schur.calls) == 1 and L.schur_complements.shape[0] == 3
        counts[mode] = schur.calls[0]["rad"].shape[0]
        if mode == "finite_difference":
            assert L.schur_gradients is not None and len(L.schur_gradients) == 3 and len(L.schur_gradients[0]) == 2
        else:
            assert L.schur_gradients is None
    # three representatives, two radius parameters each: 1 + 2 G instances per representative against one
    assert counts == {"finite_difference": 3 * 5, "analytic": 3, "preset": 3}
    # the (cell, geometry) sums of the per-strut sensitivities, times the cells' gradient factor
    L.displacement_vector[:] = np.random.default_rng(2).standard_normal(L.displacement_vector.shape)
    rec.calls.clear()
    s_cell = L._ddm_cell_sensitivities()
    assert len(rec.calls) == 1 and rec.calls[0]["want"] == ("u", "sens") and rec.calls[0]["lam_b"] is None
    lat = L.lattice
    assert s_cell.shape == (3, 2)
    for c in range(3):
        beams, s = L.cell_strut_sens[c]
        for j in range(2):
            assert np.isclose(s_cell[c, j], s[lat.beam_type[beams] == j].sum() * L._cell_gfac[c], rtol=1e-14)
    with pytest.raises(ValueError):
        LatticeOpti(_opti_preset(), ddm_gradient="central")
    fem = _opti_preset()
    fem["optimization_informations"]["simulation_type"] = "FEM"
    fem["simulation_parameters"].pop("DDM")
    with pytest.raises(ValueError):                     # the switch belongs to the DDM mode
        LatticeOpti(fem, ddm_gradient="analytic")
