"""Strut stress pass on the device (pl_stress / pl_stress_pnorm, csrc/pl_stress.h) against its numpy restatement
(stress_host.py), bitwise reproducibility, derivatives against central differences of the device's own Phi_p, the bounds
of the aggregate, and the error codes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import stress_host as SH                         # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

E, NU = 1013.0, 0.3
FIELDS = ("N", "V", "T", "Mb", "sigma_vm")


def _lattice(geoms, cells, radii=None, penalised=True):
    radii = radii or [0.05 - 0.01 * i for i in range(len(geoms))]
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                                 "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                                 "radii": radii, "geom_types": list(geoms)},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})
    return L


def _device(L, penalised=True, **kw):
    lat, pen = L.lattice, L.penalized
    if penalised:
        sl, sn = pen.seg_len, pen.seg_nsub
    else:                                            # one segment per strut, the sub-element count of the whole strut
        sl = np.zeros_like(pen.seg_len)
        sl[:, 1] = pen.seg_len.sum(axis=1)
        sn = np.zeros_like(pen.seg_nsub)
        sn[:, 1] = np.maximum(pen.seg_nsub.sum(axis=1), 1)
    return _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, sl, sn, E, NU, **kw)


def _generic_field(n, seed):
    """A displacement field without any symmetry: no N, T or Mb sits at zero."""
    return np.random.default_rng(seed).standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3


def _compare(dev, u, where):
    got, ref = dev.stress(u, where=where), dev.stress_host(u, where=where)
    for name in FIELDS:
        g, r = got[name], ref[name]
        assert g.shape == r.shape == (dev.n_beams, 4)
        assert np.array_equal(np.isnan(g), np.isnan(r)), name            # absent stations in the same places
        if np.isnan(r).all():
            continue
        scale = np.nanmax(np.abs(r))
        assert np.nanmax(np.abs(g - r)) <= 1e-12 * scale, (name, where, np.nanmax(np.abs(g - r)) / scale)
    assert np.abs(got["peak"] - ref["peak"]).max() <= 1e-12 * ref["peak"].max()
    return got


CASES = [((g,), pen) for g in sorted(_BUILTIN) for pen in (True, False)] + \
        [(("BCC", "Hybrid1"), True), (("BCC", "Hybrid1"), False), (("Octet", "Hybrid4"), True), (("Octet", "Hybrid4"), False)]


@pytest.mark.parametrize("geoms,penalised", CASES, ids=lambda v: "+".join(v) if isinstance(v, tuple) else ("pen" if v else "plain"))
def test_parity_with_the_restatement(geoms, penalised):
    """every field at every station within 1e-12 of its largest magnitude, NaN in the same places, where = 0 and 1,
    on reorder = 0 and reorder = 1 handles (strut and node permutations)."""
    L = _lattice(geoms, (1, 1, 1))
    u = _generic_field(L.lattice.n_nodes, 7)
    for reorder in (0, 1):
        with _device(L, penalised, reorder=reorder) as dev:
            dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
            dev.assemble()
            for where in (0, 1):
                got = _compare(dev, u, where)
                if where == 0:
                    present = ~np.isnan(got["sigma_vm"])
                    assert present[:, 0].all() and present[:, 3].all()
                    if not penalised:
                        assert not present[:, 1:3].any()
                else:
                    assert np.isnan(got["sigma_vm"][:, [0, 3]]).all()
            phi, smax, du, dr = dev.stress_pnorm(8, u)
            phi_h, smax_h, du_h, dr_h = dev.stress_pnorm_host(8, u)
            assert abs(phi - phi_h) <= 1e-12 * phi_h and abs(smax - smax_h) <= 1e-12 * smax_h
            assert np.abs(du - du_h).max() <= 1e-10 * np.abs(du_h).max()
            assert np.abs(dr - dr_h).max() <= 1e-10 * np.abs(dr_h).max()


@pytest.mark.parametrize("reorder", [0, 1])
def test_parity_with_strut_multiplicity(reorder):
    L = _lattice(("Octet",), (2, 2, 1), [0.04])
    rng = np.random.default_rng(3)
    mult = rng.integers(1, 5, L.lattice.n_beams).astype(float)
    u = _generic_field(L.lattice.n_nodes, 8)
    with _device(L, reorder=reorder, beam_mult=mult) as dev, _device(L, reorder=reorder) as one:
        for d in (dev, one):
            d.set_bc(np.zeros((d.n_nodes, 6), bool))
            d.assemble()
        got = _compare(dev, u, 0)
        _compare(dev, u, 1)
        # k parallel copies between the same nodes deform alike: one copy carries what the single strut carries
        single = one.stress(u)
        for name in FIELDS:
            assert np.nanmax(np.abs(got[name] - single[name])) <= 1e-12 * np.nanmax(np.abs(single[name])), name
        phi, smax, du, dr = dev.stress_pnorm(6, u, where=1)
        phi_h, smax_h, du_h, dr_h = dev.stress_pnorm_host(6, u, where=1)
        assert abs(phi - phi_h) <= 1e-12 * phi_h
        assert np.abs(du - du_h).max() <= 1e-10 * np.abs(du_h).max() and np.abs(dr - dr_h).max() <= 1e-10 * np.abs(dr_h).max()


def test_null_u_is_the_last_solution():
    L = _lattice(("BCC",), (3, 2, 2))
    f = np.zeros((L.lattice.n_nodes, 6))
    f[:, :3] = L.applied_force[:, :3]
    with _device(L) as dev:
        dev.set_bc(L.fixed_DOF, None, f)
        dev.assemble()
        u, _ = dev.solve(rtol=1e-10)
        a, b = dev.stress(None), dev.stress(u)
        for name in FIELDS + ("peak",):
            assert np.array_equal(a[name], b[name], equal_nan=True), name
        pa, pb = dev.stress_pnorm(8, None), dev.stress_pnorm(8, u)
        assert pa[0] == pb[0] and pa[1] == pb[1] and np.array_equal(pa[2], pb[2]) and np.array_equal(pa[3], pb[3])
        assert pa[1] == np.nanmax(a["sigma_vm"]) == a["peak"].max()


def test_bitwise_reproducible_over_many_blocks():
    L = _lattice(("Octet",), (6, 6, 6), [0.03])
    assert L.lattice.n_beams > 5000                                # > 20 blocks of 256 struts in both reductions
    u = _generic_field(L.lattice.n_nodes, 9)
    with _device(L) as dev:
        dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
        dev.assemble()
        for where in (0, 1):
            a, b = dev.stress_pnorm(8, u, where=where), dev.stress_pnorm(8, u, where=where)
            assert a[0] == b[0] and a[1] == b[1]
            assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
            s1, s2 = dev.stress(u, where=where), dev.stress(u, where=where)
            assert all(s1[k].tobytes() == s2[k].tobytes() for k in s1)
        phi_h, smax_h, _, _ = dev.stress_pnorm_host(8, u, want_grad=False)
        phi, smax, _, _ = dev.stress_pnorm(8, u, want_grad=False)
        assert smax == smax_h or abs(smax - smax_h) <= 1e-12 * smax_h
        assert abs(phi - phi_h) <= 1e-12 * phi_h


@pytest.mark.parametrize("where", [0, 1])
def test_derivatives_against_central_differences_of_the_device(where):
    L = _lattice(("BCC", "Hybrid1"), (2, 2, 2))
    lat = L.lattice
    rng = np.random.default_rng(21)
    u = _generic_field(lat.n_nodes, 10)
    rad = lat.beam_radius * (0.8 + 0.4 * rng.random(lat.n_beams))
    p = 8
    with _device(L) as dev:
        dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
        dev.update_radii(rad)
        dev.assemble()
        phi, smax, du, dr = dev.stress_pnorm(p, u, where=where)
        assert smax <= phi

        def value(u_):
            return dev.stress_pnorm(p, u_, where=where, want_grad=False)[0]
        hu = 1e-6                                  # of max|u|: small against the DIFFERENCES of neighbouring displacements
        for k in range(8):
            d = rng.standard_normal(u.shape) * np.abs(u).max()
            fd = (value(u + hu * d) - value(u - hu * d)) / (2 * hu)
            an = float((du * d).sum())
            assert abs(an - fd) <= 2e-3 * abs(fd), ("u", k, an, fd)
        h = 1e-4
        for k in range(8):
            e = rng.standard_normal(lat.n_beams) * rad
            vals = []
            for sgn in (1.0, -1.0):
                dev.update_radii(rad + sgn * h * e)
                dev.assemble()
                vals.append(value(u))
            fd = (vals[0] - vals[1]) / (2 * h)
            an = float(dr @ e)
            assert abs(an - fd) <= 2e-3 * abs(fd), ("r", k, an, fd)


def test_aggregate_bounds():
    L = _lattice(("Octet",), (3, 3, 3), [0.04])
    u = _generic_field(L.lattice.n_nodes, 12)
    with _device(L) as dev:
        dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
        dev.assemble()
        for where in (0, 1):
            st = dev.stress(u, where=where)
            n = int((~np.isnan(st["sigma_vm"])).sum())
            prev = np.inf
            for p in (1, 2, 4, 8, 16, 64, 200):
                phi, smax, _, _ = dev.stress_pnorm(p, u, where=where, want_grad=False)
                assert smax == np.nanmax(st["sigma_vm"])
                assert smax <= phi <= n ** (1.0 / p) * smax * (1 + 1e-12)
                assert phi <= prev * (1 + 1e-12)
                prev = phi
        # zero field: Phi = 0 and zero derivatives
        phi, smax, du, dr = dev.stress_pnorm(8, np.zeros((dev.n_nodes, 6)))
        assert phi == 0.0 and smax == 0.0 and not du.any() and not dr.any()


def test_error_codes():
    L = _lattice(("BCC",), (2, 1, 1))
    u = _generic_field(L.lattice.n_nodes, 1)
    lib = _capi.load_library()
    p = _capi._ptr
    with _device(L) as dev:
        with pytest.raises(_capi.PlError) as e:                     # before pl_assemble
            dev.stress(u)
        assert e.value.code == _capi.PL_ERR_STATE
        with pytest.raises(_capi.PlError) as e:
            dev.stress_pnorm(8, u)
        assert e.value.code == _capi.PL_ERR_STATE
        dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
        dev.assemble()
        with pytest.raises(_capi.PlError) as e:                     # u = NULL without a solve
            dev.stress(None)
        assert e.value.code == _capi.PL_ERR_STATE
        for where in (-1, 2):
            with pytest.raises(_capi.PlError) as e:
                dev.stress(u, where=where)
            assert e.value.code == _capi.PL_ERR_ARG
            with pytest.raises(_capi.PlError) as e:
                dev.stress_pnorm(8, u, where=where)
            assert e.value.code == _capi.PL_ERR_ARG
        for bad_p in (0.5, 0.0, -2.0, float("nan")):
            with pytest.raises(_capi.PlError) as e:
                dev.stress_pnorm(bad_p, u)
            assert e.value.code == _capi.PL_ERR_ARG
        uf = np.ascontiguousarray(u.ravel())
        assert lib.pl_stress(dev._h, p(uf), 0, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_stress_pnorm(dev._h, p(uf), 0, 8.0, None, None, None, None) == _capi.PL_ERR_ARG
        # a subset of the outputs is fine
        peak = np.empty(dev.n_beams)
        assert lib.pl_stress(dev._h, p(uf), 0, None, p(peak)) == _capi.PL_OK
        phi = C.c_double()
        assert lib.pl_stress_pnorm(dev._h, p(uf), 0, 8.0, C.byref(phi), None, None, None) == _capi.PL_OK
        assert phi.value >= peak.max() > 0
    # DDM handle
    S = np.eye(12)[None]
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), S, np.zeros(1, np.int32))
    try:
        u2 = np.zeros(12)
        out = np.empty(1)
        assert lib.pl_stress(ddm._h, p(u2), 0, None, p(out)) == _capi.PL_ERR_STATE
        assert lib.pl_stress_pnorm(ddm._h, p(u2), 0, 8.0, p(out), None, None, None) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
