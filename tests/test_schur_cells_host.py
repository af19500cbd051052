"""Host side of the batched exact cell condensation (pl_schur_cells), no GPU: the wrapper's argument checks, the C ABI
without a device, and how LatticeSim.calculate_schur_complement_cells groups cells, de-duplicates radius sets and
builds the central-difference variants - with a stub in place of the device call."""
import os

import numpy as np
import pytest

from pylatticedso_amd import _capi

E, NU = 1013.0, 0.3


def _bcc_cell_arrays():
    xyz = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)] + [[0.5, 0.5, 0.5]], float)
    conn = np.array([[k, 8] for k in range(8)], np.int32)
    L = np.sqrt(0.75)
    return xyz, conn, np.arange(8), np.full(8, 0.05), np.tile([0.0, L, 0.0], (8, 1)), np.tile([0, 10, 0], (8, 1))


def test_wrapper_argument_checks():
    xyz, conn, bn, rad, sl, sn = _bcc_cell_arrays()
    with pytest.raises(ValueError):                  # connectivity must be (B, 2) integers
        _capi.schur_cells(xyz, conn.astype(float), bn, rad, sl, sn, E, NU)
    with pytest.raises(ValueError):
        _capi.schur_cells(xyz, conn[:, :1], bn, rad, sl, sn, E, NU)
    with pytest.raises(ValueError):                  # boundary list must be 1-D integers
        _capi.schur_cells(xyz, conn, bn.reshape(2, 4), rad, sl, sn, E, NU)
    with pytest.raises(ValueError):
        _capi.schur_cells(xyz, conn, bn.astype(float), rad, sl, sn, E, NU)
    with pytest.raises(ValueError):                  # per-strut array of the wrong length
        _capi.schur_cells(xyz, conn, bn, rad[:-1], sl, sn, E, NU)
    with pytest.raises(ValueError):                  # leading axes of per-instance arrays disagree
        _capi.schur_cells(np.stack([xyz] * 3), conn, bn, np.stack([rad] * 2), sl, sn, E, NU)
    with pytest.raises(ValueError):                  # n_inst that the per-instance arrays do not have
        _capi.schur_cells(np.stack([xyz] * 3), conn, bn, rad, sl, sn, E, NU, n_inst=4)
    with pytest.raises(ValueError):
        _capi.schur_cells(xyz, conn, bn, rad, sl, sn.astype(float), E, NU)
    with pytest.raises(ValueError):
        _capi.schur_cells(xyz[:, :2], conn, bn, rad, sl, sn, E, NU)
    assert _capi.schur_cells_fits(9, 8, 8) and _capi.schur_cells_fits(35, 70, 26)
    assert not _capi.schur_cells_fits(34, 33, 33) and not _capi.schur_cells_fits(40, 60, 20)
    assert not _capi.schur_cells_fits(9, 513, 8)


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
    S = np.empty((48, 48))
    info = np.empty(1, np.int32)
    p = _capi._ptr
    opts = _capi.default_opts(lib)

    def call(opts=opts, n_inst=1, nb=8, bnodes=bn, conn=conn):
        return lib.pl_schur_cells(C.byref(opts), n_inst, 9, len(conn), p(conn), nb, p(bnodes), p(xyz), p(rad), p(sl),
                                  p(sn), p(S), p(info))

    # argument errors are reported whether or not a device is there
    assert call(n_inst=0) == _capi.PL_ERR_ARG
    assert call(bnodes=np.array([0, 1, 2, 3, 4, 5, 6, 9], np.int32)) == _capi.PL_ERR_ARG      # out of range
    assert call(bnodes=np.array([0, 1, 2, 3, 4, 5, 6, 6], np.int32)) == _capi.PL_ERR_ARG      # listed twice
    assert call(conn=np.array([[0, 8]] * 7 + [[8, 8]], np.int32)) == _capi.PL_ERR_ARG          # strut on one node
    raw = _capi.PlOpts()                                                                        # not stamped
    assert call(opts=raw) == _capi.PL_ERR_ARG
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert call() == _capi.PL_ERR_NODEVICE
    with pytest.raises(_capi.PlError) as e:
        _capi.schur_cells(xyz, conn, bn, rad, sl, sn, E, NU)
    assert e.value.code == _capi.PL_ERR_NODEVICE


def _ddm_preset(nx=3):
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": nx, "y": 1, "z": 1},
                         "radii": [0.05], "geom_types": ["BCC"]},
            "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                      "DDM": {"enable_preconditioner": False, "max_iterations": 5000,
                                              "schur_complement_computation": {"type": "exact"}}},
            "boundary_conditions": {
                "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                           "Value": [0, 0, 0, 0, 0, 0]}},
                "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}}


class _Stub:
    """Stands in for _capi.schur_cells: records every call, returns S_i = sum(radius_i) * I + mean(seg_len_i) * J."""

    def __init__(self):
        self.calls = []

    def __call__(self, node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, young, poisson, **kw):
        rad = np.asarray(beam_radius)
        self.calls.append(dict(xyz=np.asarray(node_xyz), conn=np.asarray(beam_conn), order=np.asarray(boundary_nodes),
                               rad=rad, seg_len=np.asarray(seg_len), young=young, poisson=poisson, kw=kw))
        m = 6 * len(boundary_nodes)
        S = np.stack([r.sum() * np.eye(m) + np.mean(s) * np.ones((m, m)) for r, s in zip(rad, np.asarray(seg_len))])
        return S, np.zeros(len(rad), np.int32)


def test_exact_branch_groups_deduplicates_and_builds_central_differences(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    stub = _Stub()
    monkeypatch.setattr(_capi, "schur_cells", stub)
    L = LatticeSim(_ddm_preset(4), enable_domain_decomposition_solver=True)
    assert len(stub.calls) == 1                                    # every cell has the same radius: one representative
    assert stub.calls[0]["rad"].shape[0] == 1
    stub.calls.clear()
    L.enable_gradient_computing = True
    radii = np.array([[0.03], [0.05], [0.03], [0.07]])
    L.set_cell_radii(radii)
    lat, pen = L.lattice, L.penalized
    # three distinct radius sets, one topology (connectivity + boundary order: every BCC cell has the same): one call
    reps = [0, 1, 3]
    assert list(L.cell_schur_index) == [0, 1, 0, 2]
    assert len(stub.calls) == 1
    call = stub.calls[0]
    assert call["rad"].shape[0] == 3 * 3                           # each representative + its +h / -h variants
    assert call["young"] == L.young_modulus and call["poisson"] == L.poisson_ratio
    assert call["kw"]["pen_coef"] == L.penalization_coefficient
    for i, c in enumerate(reps):
        beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
        nodes = np.unique(lat.beam_conn[beams])
        assert np.array_equal(call["xyz"][3 * i], lat.node_xyz[nodes])
        base, plus, minus = call["rad"][3 * i:3 * i + 3]
        assert np.array_equal(base, lat.beam_radius[beams])
        r = radii[c, 0]
        h = max(1e-8, 1e-6 * max(1.0, abs(r)))
        assert np.allclose(plus, r + h, rtol=0, atol=1e-15) and np.allclose(minus, r - h, rtol=0, atol=1e-15)
        for k in range(3):                                         # segments fixed across the variants
            assert np.array_equal(call["seg_len"][3 * i + k], pen.seg_len[beams])
        S = L.schur_complements[i]
        assert np.array_equal(S, base.sum() * np.eye(len(S)) + np.mean(pen.seg_len[beams]) * np.ones(S.shape))
        G = L.schur_gradients[i]
        assert len(G) == 1
        expect = (plus.sum() - minus.sum()) / ((r + h) - (r - h))
        assert np.allclose(np.diag(G[0]), expect, rtol=1e-12)
    # boundary order of the call = the cell's boundary nodes in the representative's local numbering
    cb = L.cell_boundary_nodes()[0]
    beams = lat.cell_beam_idx[lat.cell_beam_ptr[0]:lat.cell_beam_ptr[1]]
    nodes = np.unique(lat.beam_conn[beams])
    assert np.array_equal(nodes[call["order"]], cb)


def test_exact_branch_falls_back_beyond_the_kernel(monkeypatch):
    from pylatticedso_amd.lattice_sim import LatticeSim
    stub = _Stub()
    monkeypatch.setattr(_capi, "schur_cells", stub)
    monkeypatch.setattr(_capi, "schur_cells_fits", lambda *a: False)
    seen = []

    def by_columns(self, c, beams, nodes, conn, order, radii):
        seen.append(c)
        return np.eye(6 * len(order)) * (c + 1), None

    monkeypatch.setattr(LatticeSim, "_schur_cell_by_columns", by_columns)
    L = LatticeSim(_ddm_preset(3), enable_domain_decomposition_solver=True)
    L.set_cell_radii([[0.03], [0.05], [0.03]])
    assert not stub.calls and seen[-2:] == [0, 1]
    assert list(L.cell_schur_index) == [0, 1, 0] and L.schur_complements[1][0, 0] == 2.0
