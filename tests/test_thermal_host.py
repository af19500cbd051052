"""Host side of the thermal loads (pl_set_thermal / pl_thermal_load / pl_thermal_sens), no GPU: the numpy restatement
(pylatticedso_amd/thermal_host.py, the yardstick of the device parity tests) pinned on stress_host.records and
geometric_host.elastic_matrix - free expansion of a clamped-at-one-node lattice, a strut held at both ends in closed form,
the radius derivatives against central differences, and the homogenised expansion of a periodic cell."""
import numpy as np
import pytest
import scipy.linalg

from pylatticedso_amd import buckling_host as BH
from pylatticedso_amd import geometric_host as GH
from pylatticedso_amd import stress_host as SH
from pylatticedso_amd import thermal_host as TH
from pylatticedso_amd.homogenization_cell import imposed_displacement, periodic_masters

E, NU, KAPPA, PEN = 1013.0, 0.3, 0.9, 1.5


def _lattice(cells, geoms, radii):
    from pylatticedso_amd.lattice_sim import LatticeSim
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                                    "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                                    "radii": list(radii), "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                       "boundary_conditions": {
                           "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                      "Value": [0, 0, 0, 0, 0, 0]}},
                           "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})


class _Problem:
    """2 x 1 x 1 BCC + Hybrid1 with random radii and multiplicities: records, dense K and the restatement's calls."""

    def __init__(self, seed=5):
        L = _lattice((2, 1, 1), ("BCC", "Hybrid1"), (0.05, 0.04))
        lat, pen = L.lattice, L.penalized
        rng = np.random.default_rng(seed)
        self.L = L
        self.xyz, self.conn, self.sl, self.sn = lat.node_xyz, lat.beam_conn, pen.seg_len, pen.seg_nsub
        self.nn, self.nb = lat.n_nodes, lat.n_beams
        self.mat = (L.young_modulus, L.poisson_ratio, KAPPA, L.penalization_coefficient)
        self.mult = rng.integers(1, 3, self.nb).astype(float)
        self.rad = lat.beam_radius * (0.8 + 0.4 * rng.random(self.nb))
        self.rng = rng

    def records(self, rad=None):
        return SH.records(self.xyz, self.conn, self.rad if rad is None else rad, self.sl, self.sn, *self.mat, self.mult)

    def matrix(self, rad=None):
        return GH.elastic_matrix(self.records(rad), self.conn, self.nn).toarray()

    def solve(self, fixed, f, rad=None):
        """u (N, 6) of K u = f on the free dofs, zero on the fixed ones."""
        free = np.flatnonzero(~np.asarray(fixed, bool).ravel())
        K = self.matrix(rad)
        u = np.zeros(6 * self.nn)
        u[free] = scipy.linalg.solve(K[np.ix_(free, free)], np.asarray(f).ravel()[free], assume_a="pos")
        return u.reshape(-1, 6)


def test_free_expansion_of_a_lattice_held_at_one_node():
    """Uniform dT, node 0 clamped: u = alpha dT (x - x_0) with zero rotations, every mechanical N vanishes.  Bounds of the
    issue: 1e-10 of the largest displacement, 1e-12 of the largest n_free (observed 3e-12 and 6e-15)."""
    P = _Problem()
    assert (P.mult == 1).any() and (P.mult == 2).any() and (P.sl[:, 0] > 0).any()
    alpha, dT = 7e-5, 40.0
    rec = P.records()
    delta = TH.elongation(P.xyz, P.conn, alpha, dT)
    f_th, n_free = TH.thermal_load(rec, P.conn, P.nn, delta, P.mult)
    assert not f_th[:, 3:].any()
    fixed = np.zeros((P.nn, 6), bool)
    fixed[0] = True
    u = P.solve(fixed, f_th)
    want = np.zeros((P.nn, 6))
    want[:, :3] = alpha * dT * (P.xyz - P.xyz[0])
    err_u = np.abs(u - want).max() / np.abs(want).max()
    N = TH.axial_force(rec, P.conn, u, delta, P.mult)
    err_n = np.abs(N).max() / np.abs(n_free).max()
    print(f"free expansion: displacement error {err_u:.2e}, mechanical N / max n_free {err_n:.2e}")
    assert err_u <= 1e-10 and err_n <= 1e-12
    # the stress and buckling restatements see the same mechanical force through their offset
    fth = TH.restrained_force(rec, delta)
    Em, nu, kappa, pen = P.mat
    st = SH.strut_stress(rec, P.conn, P.rad, P.sl, u, pen, P.mult, 0, fth)
    assert np.nanmax(np.abs(st["N"])) <= 1e-12 * np.abs(n_free).max()
    bk = BH.strut_buckling(rec, P.conn, P.rad, P.sl, u, Em, nu, kappa, P.mult, 0, 1.0, 0, fth)
    assert np.abs(bk["n_axial"] - N).max() <= 1e-12 * np.abs(n_free).max()
    # and without the offset they are what they were: the restrained force shows up as tension
    plain = SH.strut_stress(rec, P.conn, P.rad, P.sl, u, pen, P.mult, 0)
    assert np.allclose(plain["N"][:, 0], n_free, rtol=1e-9, atol=0)


@pytest.mark.parametrize("mult", [None, 2.0])
def test_single_strut_clamped_at_both_ends(mult):
    """N = -E S_eff alpha dT with the series sum of the three segments L / S_eff = sum l_i / S_i; k copies carry it each."""
    seg_len, seg_n = (0.11, 0.53, 0.07), (3, 9, 2)
    r, alpha, dT = 0.04, 2e-5, 55.0
    L = sum(seg_len)
    t = np.array([2.0, -1.0, 0.5])
    t /= np.linalg.norm(t)
    xyz = np.array([[0.3, 0.1, -0.2], [0.3, 0.1, -0.2] + L * t])
    S = [np.pi * (PEN * r) ** 2, np.pi * r ** 2, np.pi * (PEN * r) ** 2]
    S_eff = L / sum(l / s for l, s in zip(seg_len, S))
    m = None if mult is None else [mult]
    rec = SH.records(xyz, [[0, 1]], [r], [seg_len], [seg_n], E, NU, KAPPA, PEN, m)
    delta = TH.elongation(xyz, [[0, 1]], alpha, [dT, dT])
    assert np.isclose(delta[0], alpha * L * dT, rtol=1e-14)
    f, n_free = TH.thermal_load(rec, [[0, 1]], 2, delta, m)
    assert np.isclose(n_free[0], E * S_eff * alpha * dT, rtol=1e-13)
    assert np.allclose(f[1, :3], (mult or 1.0) * n_free[0] * t, rtol=1e-13) and np.allclose(f[0], -f[1], rtol=1e-15)
    u = np.zeros((2, 6))
    N = TH.axial_force(rec, [[0, 1]], u, delta, m)
    assert np.isclose(N[0], -E * S_eff * alpha * dT, rtol=1e-13)
    fth = TH.restrained_force(rec, delta)
    st = SH.strut_stress(rec, [[0, 1]], [r], [seg_len], u, PEN, m, 0, fth)
    assert np.allclose(st["N"][0], N[0], rtol=1e-13)
    assert st["V"][0].max() <= 1e-14 * abs(N[0]) and st["Mb"][0].max() <= 1e-14 * abs(N[0]) * L     # only N shifts
    bk = BH.strut_buckling(rec, [[0, 1]], [r], [seg_len], u, E, NU, KAPPA, m, 1, 1.0, 0, fth)
    assert np.isclose(bk["util"][0], E * S_eff * alpha * dT / bk["n_crit"][0], rtol=1e-13)
    cooled = BH.strut_buckling(rec, [[0, 1]], [r], [seg_len], u, E, NU, KAPPA, m, 1, 1.0, 0, -fth)
    assert cooled["util"][0] == 0.0 and cooled["n_axial"][0] > 0


def test_thermal_sens_and_total_derivative_against_central_differences():
    """lam^T d f_th / dr_b and the total derivative of q.u, K u = f_ext + f_th with Dirichlet dofs, per-strut alpha and a
    strictly positive random dT (40 +- 10), against central differences of the restatement: h = 1e-6 r, 2e-3 of the
    difference (the project's finite-difference bounds)."""
    P = _Problem(seed=11)
    rng = P.rng
    alpha = (2.0 + 5.0 * rng.random(P.nb)) * 1e-5
    dT = 40.0 + 10.0 * (2.0 * rng.random(P.nn) - 1.0)
    assert dT.min() > 0
    delta = TH.elongation(P.xyz, P.conn, alpha, dT)
    fixed = np.asarray(P.L.fixed_DOF, bool)
    assert fixed.any() and not fixed.all()
    f_ext = np.where(fixed, 0.0, rng.standard_normal((P.nn, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05]) * 1e-2)
    q = np.where(fixed, 0.0, rng.standard_normal((P.nn, 6)))

    def f_th(rad):
        return TH.thermal_load(P.records(rad), P.conn, P.nn, delta, P.mult)[0]

    def objective(rad):
        return float((q * P.solve(fixed, f_ext + f_th(rad), rad)).sum())

    rec = P.records()
    u = P.solve(fixed, f_ext + f_th(P.rad))
    lam = P.solve(fixed, q)
    lam_any = rng.standard_normal((P.nn, 6))
    ts_any = TH.thermal_sens(rec, P.conn, P.rad, delta, lam_any)
    drec = SH.drecords_dr(P.xyz, P.conn, P.rad, P.sl, P.sn, *P.mat, P.mult)
    total = -GH._pairing(drec, P.conn, u, lam) + TH.thermal_sens(rec, P.conn, P.rad, delta, lam)
    worst = [0.0, 0.0]
    for b in range(P.nb):
        h = 1e-6 * P.rad[b]
        e = np.zeros(P.nb)
        e[b] = h
        fd = float((lam_any * (f_th(P.rad + e) - f_th(P.rad - e))).sum()) / (2 * h)
        worst[0] = max(worst[0], abs(ts_any[b] - fd) / abs(fd))
        assert abs(ts_any[b] - fd) <= 2e-3 * abs(fd), ("thermal_sens", b, ts_any[b], fd)
        fd = (objective(P.rad + e) - objective(P.rad - e)) / (2 * h)
        worst[1] = max(worst[1], abs(total[b] - fd) / abs(fd))
        assert abs(total[b] - fd) <= 2e-3 * abs(fd), ("total", b, total[b], fd)
    print(f"central differences: thermal_sens {worst[0]:.2e}, total derivative {worst[1]:.2e}")
    # the thermal term matters: without it the total derivative misses the bound
    plain = -GH._pairing(drec, P.conn, u, lam)
    assert np.abs(plain - total).max() > 2e-3 * np.abs(total).max()


def _cell(geoms, radii):
    L = _lattice((1, 1, 1), geoms, radii)
    lat, pen = L.lattice, L.penalized
    rec = SH.records(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, L.young_modulus,
                     L.poisson_ratio, KAPPA, L.penalization_coefficient)
    return lat, rec


def _direct_expansion(lat, rec, alpha):
    """The stress-free periodic cell solved directly: u = W a + P v with the six macro strain fields W, the periodic
    fluctuation P v (first master group's translations anchored) and K u = f_th in that space - no use of the total fields."""
    xyz, N = lat.node_xyz, lat.n_nodes
    K = GH.elastic_matrix(rec, lat.beam_conn, N).toarray()
    master, _ = periodic_masters(xyz, lat.cell_coord[0], lat.cell_size[0])
    masters = np.unique(master)
    slot = np.full(N, -1, np.int64)
    slot[masters] = np.arange(len(masters))
    cols = (6 * slot[master][:, None] + np.arange(6)).ravel()
    Pm = np.zeros((6 * N, 6 * len(masters)))
    Pm[np.arange(6 * N), cols] = 1.0
    W = np.stack([imposed_displacement(c, xyz).ravel() for c in range(1, 7)], axis=1)
    T = np.hstack([W, Pm[:, 3:]])
    f = TH.thermal_load(rec, lat.beam_conn, N, TH.elongation(xyz, lat.beam_conn, alpha, 1.0))[0].ravel()
    return scipy.linalg.solve(T.T @ K @ T, T.T @ f, assume_a="pos")[:6]


@pytest.mark.parametrize("geoms,radii", [(("BCC",), (0.05,)), (("Octet", "BCC"), (0.04, 0.06))], ids=["BCC", "Octet+BCC"])
def test_homogenized_expansion_of_one_material(geoms, radii):
    lat, rec = _cell(geoms, radii)
    alpha = 7e-5
    got = TH.homogenized_expansion(rec, lat.beam_conn, lat.node_xyz, lat.cell_coord[0], lat.cell_size[0], alpha)
    assert np.abs(got - alpha * np.array([1, 1, 1, 0, 0, 0])).max() <= 1e-10 * alpha, got / alpha
    direct = _direct_expansion(lat, rec, alpha)
    assert np.abs(got - direct).max() <= 1e-10 * np.abs(direct).max()


def test_homogenized_expansion_of_the_bimaterial_cell():
    """Octet + BCC, radii 0.04 / 0.06, alpha 7e-5 on beam_type 0 and 2e-5 on the rest: 0.736349 x 7e-5 on the normal
    components, no shear (1e-5 relative), equal to the direct zero-macro-stress solve to 1e-10."""
    lat, rec = _cell(("Octet", "BCC"), (0.04, 0.06))
    alpha = np.where(np.asarray(lat.beam_type) == 0, 7e-5, 2e-5)
    assert (alpha == 7e-5).any() and (alpha == 2e-5).any()
    got = TH.homogenized_expansion(rec, lat.beam_conn, lat.node_xyz, lat.cell_coord[0], lat.cell_size[0], alpha)
    want = 0.736349 * 7e-5 * np.array([1, 1, 1, 0, 0, 0])
    print("bi-material alpha_hom / 7e-5:", got / 7e-5)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), got / 7e-5
    direct = _direct_expansion(lat, rec, alpha)
    assert np.abs(got - direct).max() <= 1e-10 * np.abs(direct).max()


def test_c_abi_declares_the_thermal_entry_points():
    import os
    import re
    from pylatticedso_amd import _capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pylattice_hip.h")).read()
    for name in ("pl_set_thermal", "pl_thermal_load", "pl_thermal_sens"):
        assert re.search(r"^int " + name + r"\(pl_handle h", hdr, flags=re.M), name
        assert name in _capi.EXPORTS
