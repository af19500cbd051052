"""Host side of the steady heat conduction on the strut graph (pl_set_conduction / pl_cond_spmv / pl_cond_solve / pl_cond_flux /
pl_cond_sens / pl_thermal_load_adjoint), no GPU: the numpy restatement (pylatticedso_amd/conduction_host.py, the yardstick of
the device parity tests) on hand-built graphs with known answers, the properties of the Laplacian, the heat balance, and the
radius derivatives - cond_sens and the whole thermo-elastic chain - against central differences of the restatement itself."""
import os
import re

import numpy as np

from pylatticedso_amd import conduction_host as CH

KAPPA_SHEAR = 0.9


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


def test_one_strut():
    xyz = np.array([[0.1, 0.2, 0.3], [0.1 + 0.3, 0.2 - 0.4, 0.3 + 1.2]])     # L = 1.3
    r, kappa = 0.04, 0.25
    g = CH.conductance(xyz, [[0, 1]], [r], kappa)
    assert np.isclose(g[0], kappa * np.pi * r * r / 1.3, rtol=1e-15)
    assert np.isclose(CH.conductance(xyz, [[0, 1]], [r], [kappa], [3.0])[0], 3.0 * g[0], rtol=1e-15)
    T = CH.solve([[0, 1]], 2, g, [1, 0], [50.0, 0.0], [0.0, 0.7])       # node 0 held at 50, 0.7 flows in at node 1
    assert T[0] == 50.0 and np.isclose(T[1], 50.0 + 0.7 / g[0], rtol=1e-14)
    assert np.isclose(CH.flux([[0, 1]], g, T)[0], -0.7, rtol=1e-13)     # from A to B: the inflow leaves through node 0


def test_series_and_parallel():
    """Three nodes in series: the inner temperature is the conductance-weighted mean, the flow that of the series conductance.
    Two struts in parallel between the same nodes: the conductances add, and k copies are k struts."""
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 2.0, 0]])
    conn = np.array([[0, 1], [1, 2]])
    g = CH.conductance(xyz, conn, [0.05, 0.03], [0.2, 0.5])
    T = CH.solve(conn, 3, g, [1, 0, 1], [80.0, 0.0, 20.0])
    assert np.isclose(T[1], (g[0] * 80.0 + g[1] * 20.0) / (g[0] + g[1]), rtol=1e-14)
    Q = CH.flux(conn, g, T)
    series = g[0] * g[1] / (g[0] + g[1])
    assert np.allclose(Q, series * 60.0, rtol=1e-13)
    xyz2 = np.array([[0.0, 0, 0], [0.0, 0, 1.5]])
    conn2 = np.array([[0, 1], [1, 0]])                                   # the second one the other way round
    g2 = CH.conductance(xyz2, conn2, [0.05, 0.02], 0.3)
    T2 = CH.solve(conn2, 2, g2, [1, 0], [10.0, 0.0], [0.0, 2.0])
    assert np.isclose(T2[1], 10.0 + 2.0 / (g2[0] + g2[1]), rtol=1e-14)
    Q2 = CH.flux(conn2, g2, T2)
    assert np.isclose(Q2[0], -2.0 * g2[0] / g2.sum(), rtol=1e-13) and np.isclose(Q2[1], 2.0 * g2[1] / g2.sum(), rtol=1e-13)
    gk = CH.conductance(xyz2, conn2[:1], [0.05], 0.3, [4.0])
    Tk = CH.solve(conn2[:1], 2, gk, [1, 0], [10.0, 0.0], [0.0, 2.0])
    assert np.isclose(Tk[1], 10.0 + 2.0 / (4.0 * g2[0]), rtol=1e-14)
    assert np.isclose(CH.flux(conn2[:1], gk, Tk, [4.0])[0], -0.5, rtol=1e-13)      # one of the four copies


def _bcc222():
    L = _lattice((2, 2, 2), ("BCC",), (0.05,))
    lat = L.lattice
    rng = np.random.default_rng(2)
    rad = lat.beam_radius * (0.8 + 0.4 * rng.random(lat.n_beams))
    kap = 0.1 + 0.3 * rng.random(lat.n_beams)
    return L, lat, rad, kap, rng


def test_laplacian_properties():
    L, lat, rad, kap, rng = _bcc222()
    g = CH.conductance(lat.node_xyz, lat.beam_conn, rad, kap)
    K = CH.laplacian(lat.beam_conn, lat.n_nodes, g)
    scale = np.abs(K).max()
    assert np.abs(K.sum(axis=1)).max() <= 1e-13 * scale
    assert np.array_equal(K, K.T)
    w = np.linalg.eigvalsh(K)
    assert w[0] >= -1e-12 * w[-1]
    assert abs(w[0]) <= 1e-12 * w[-1] and w[1] > 1e-6 * w[-1]          # one zero: the lattice is connected
    assert np.abs(K @ np.ones(lat.n_nodes)).max() <= 1e-13 * scale       # ... and the constants are its null space
    x = rng.standard_normal(lat.n_nodes)
    assert np.abs(CH.spmv(lat.beam_conn, lat.n_nodes, g, x) - K @ x).max() <= 1e-13 * np.abs(K @ x).max()
    fixed = rng.random(lat.n_nodes) < 0.3
    P = np.diag((~fixed).astype(float))
    assert np.abs(CH.spmv(lat.beam_conn, lat.n_nodes, g, x, fixed) - P @ K @ P @ x).max() <= 1e-13 * np.abs(K @ x).max()


def test_heat_balance_between_a_hot_and_a_cold_face():
    """Hot face Xmin, cold face Xmax, an inflow on the Ymax nodes in between: what the Dirichlet nodes take up, K_T T there,
    balances the prescribed inflow to 1e-12 (of the sum of the magnitudes)."""
    L, lat, rad, kap, rng = _bcc222()
    hot, cold = L.find_point_on_lattice_surface(["Xmin"]), L.find_point_on_lattice_surface(["Xmax"])
    fixed = np.zeros(lat.n_nodes, bool)
    fixed[hot] = fixed[cold] = True
    t_bar = np.zeros(lat.n_nodes)
    t_bar[hot], t_bar[cold] = 90.0, 20.0
    q = np.zeros(lat.n_nodes)
    src = np.setdiff1d(L.find_point_on_lattice_surface(["Ymax"]), np.flatnonzero(fixed))
    q[src] = 0.4 / len(src)
    g = CH.conductance(lat.node_xyz, lat.beam_conn, rad, kap)
    T = CH.solve(lat.beam_conn, lat.n_nodes, g, fixed, t_bar, q)
    assert np.array_equal(T[fixed], t_bar[fixed])
    out = CH.laplacian(lat.beam_conn, lat.n_nodes, g) @ T                 # net outflow of every node into the struts
    assert np.abs(out[~fixed] - q[~fixed]).max() <= 1e-12 * np.abs(out).max()
    assert abs(out[fixed].sum() + q.sum()) <= 1e-12 * (np.abs(out[fixed]).sum() + q.sum())
    # the same balance in strut flows: what leaves the hot face minus what reaches the cold one
    Q = CH.flux(lat.beam_conn, g, T)
    net = np.zeros(lat.n_nodes)
    np.add.at(net, lat.beam_conn[:, 0], Q)
    np.add.at(net, lat.beam_conn[:, 1], -Q)
    assert np.abs(net - out).max() <= 1e-12 * np.abs(out).max()


class _Coupled:
    """2 x 2 x 2 BCC + Hybrid1, clamped at Xmin with a load on Xmax; temperature fixed on Zmin, heat inflow on Zmax, so T - T_ref
    scales like 1 / r^2.  INFLOW is the total on the Zmax face."""
    INFLOW = 2.0
    ALPHA, KAPPA, T_COLD, T_REF = 7e-5, 0.2, 20.0, 20.0

    def __init__(self):
        L = _lattice((2, 2, 2), ("BCC", "Hybrid1"), (0.05, 0.04))
        lat, pen = L.lattice, L.penalized
        rng = np.random.default_rng(7)
        self.xyz, self.conn, self.sl, self.sn = lat.node_xyz, lat.beam_conn, pen.seg_len, pen.seg_nsub
        self.nn, self.nb = lat.n_nodes, lat.n_beams
        self.mat = (L.young_modulus, L.poisson_ratio, KAPPA_SHEAR, L.penalization_coefficient)
        self.mult = rng.integers(1, 3, self.nb).astype(float)
        self.rad = lat.beam_radius * (0.8 + 0.4 * rng.random(self.nb))
        self.fixed_dof = np.asarray(L.fixed_DOF, bool)
        self.f_ext = np.zeros((self.nn, 6))
        self.f_ext[:, :3] = L.applied_force[:, :3]
        self.q = np.where(self.fixed_dof, 0.0, rng.standard_normal((self.nn, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1]))
        cold, top = L.find_point_on_lattice_surface(["Zmin"]), L.find_point_on_lattice_surface(["Zmax"])
        self.t_fixed = np.zeros(self.nn, bool)
        self.t_fixed[cold] = True
        self.t_bar = np.where(self.t_fixed, self.T_COLD, 0.0)
        self.heat = np.zeros(self.nn)
        self.heat[top] = self.INFLOW / len(top)
        self.beam_alpha = self.ALPHA * (0.7 + 0.6 * rng.random(self.nb))
        self.rng = rng

    def args(self, rad):
        return (self.xyz, self.conn, rad, self.sl, self.sn, self.mat, self.mult, self.fixed_dof, self.f_ext)

    def state(self, rad):
        return CH.coupled_state(*self.args(rad), self.beam_alpha, self.KAPPA, self.t_fixed, self.t_bar, self.heat, self.T_REF)

    def objective(self, rad):
        return float((self.q * self.state(rad)["u"]).sum())

    def gradient(self, chain):
        return CH.coupled_gradient(*self.args(self.rad), self.q, self.beam_alpha, self.KAPPA, self.t_fixed, self.t_bar,
                                   self.heat, self.T_REF, chain=chain)


def _misses(g, fd, gmax):
    return abs(g - fd) >= 2e-3 * max(abs(fd), gmax)


def test_cond_sens_against_central_differences():
    """mu^T (dK_T / dr_b) T for random mu, T against central differences of mu^T K_T(r) T, step 1e-4, on every strut."""
    P = _Coupled()
    T, mu = 20.0 + 50.0 * P.rng.random(P.nn), P.rng.standard_normal(P.nn)

    def form(rad):
        return float(mu @ CH.spmv(P.conn, P.nn, CH.conductance(P.xyz, P.conn, rad, P.KAPPA, P.mult), T))

    got = CH.cond_sens(P.conn, P.rad, CH.conductance(P.xyz, P.conn, P.rad, P.KAPPA, P.mult), T, mu)
    worst = 0.0
    for b in range(P.nb):
        e = np.zeros(P.nb)
        e[b] = 1e-4
        fd = (form(P.rad + e) - form(P.rad - e)) / 2e-4
        worst = max(worst, abs(got[b] - fd) / max(abs(fd), np.abs(got).max()))
        assert not _misses(got[b], fd, np.abs(got).max()), (b, got[b], fd)
    print(f"cond_sens against central differences: worst {worst:.2e} of the bound's scale")


def test_coupled_gradient_against_central_differences():
    """d(q . u)/dr_b of K u = f_ext + f_th(T(r) - T_ref, r) with K_T(r) T = q_heat: the whole chain against central differences
    of the restatement (step 1e-4, |g - fd| < 2e-3 max(|fd|, max|g|)) on 12 struts; without the mu term the gradient misses
    that bound (total inflow 2.0 on the Zmax face, the first value tried: 10 of the 12 checked struts miss, the worst at
    3.3e-2 of the scale against 7.5e-7 with the term)."""
    P = _Coupled()
    g, g_plain = P.gradient(True), P.gradient(False)
    gmax = np.abs(g).max()
    checked = P.rng.choice(P.nb, 12, replace=False)
    missed_plain, worst, worst_plain = 0, 0.0, 0.0
    for b in checked:
        e = np.zeros(P.nb)
        e[b] = 1e-4
        fd = (P.objective(P.rad + e) - P.objective(P.rad - e)) / 2e-4
        worst = max(worst, abs(g[b] - fd) / max(abs(fd), gmax))
        worst_plain = max(worst_plain, abs(g_plain[b] - fd) / max(abs(fd), np.abs(g_plain).max()))
        assert not _misses(g[b], fd, gmax), (b, g[b], fd)
        missed_plain += _misses(g_plain[b], fd, np.abs(g_plain).max())
    print(f"coupled gradient: worst {worst:.2e}; without the mu term worst {worst_plain:.2e}, "
          f"{missed_plain} of {len(checked)} miss the bound (inflow {P.INFLOW})")
    assert missed_plain >= 1


def test_thermal_load_adjoint_is_the_transpose_of_the_thermal_load():
    """c . dT = lam . f_th(dT) for random lam and dT (f_th is linear in dT)."""
    from pylatticedso_amd import stress_host as SH
    from pylatticedso_amd import thermal_host as TH
    P = _Coupled()
    rec = SH.records(P.xyz, P.conn, P.rad, P.sl, P.sn, *P.mat, P.mult)
    lam, dT = P.rng.standard_normal((P.nn, 6)), P.rng.standard_normal(P.nn)
    c = CH.thermal_load_adjoint(rec, P.conn, P.nn, P.beam_alpha, lam)
    f = TH.thermal_load(rec, P.conn, P.nn, TH.elongation(P.xyz, P.conn, P.beam_alpha, dT), P.mult)[0]
    assert abs(c @ dT - (lam * f).sum()) <= 1e-12 * np.abs(lam * f).sum()


def test_c_abi_declares_the_conduction_entry_points():
    from pylatticedso_amd import _capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pylattice_hip.h")).read()
    for name in ("pl_set_conduction", "pl_cond_spmv", "pl_cond_solve", "pl_cond_flux", "pl_cond_sens",
                 "pl_thermal_load_adjoint"):
        assert re.search(r"^int " + name + r"\(pl_handle h", hdr, flags=re.M), name
        assert name in _capi.EXPORTS
    assert re.search(r"^#define PL_ABI_VERSION 6u$", hdr, flags=re.M)
