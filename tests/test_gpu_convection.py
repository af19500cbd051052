"""Lumped strut-surface convection and the thermal aggregates on the device (pl_set_convection / pl_cond_solve_adjoint /
pl_cond_film / pl_temp_pnorm and the convective forms of pl_cond_spmv / pl_cond_solve / pl_cond_sens, csrc/pl_conduction.h)
against the numpy restatement (conduction_host.py): parity of the products, the solved temperatures against a dense host solve,
bitwise reproducibility over many blocks, the life of the state, the error codes, and the way up through LatticeSim and
LatticeOpti with the gradients of the thermal objectives and of the max_temperature constraint against central differences."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import conduction_host as CH                     # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

E, NU = 1013.0, 0.3
ALL6 = ["X", "Y", "Z", "RX", "RY", "RZ"]
T_INF = 20.0


def _preset(geoms, cells, radii, fixed="Xmin", loaded="Xmax", value=-0.1):
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                         "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                         "radii": list(radii), "geom_types": list(geoms)},
            "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
            "boundary_conditions": {
                "Displacement": {"Fixed": {"Surface": [fixed], "DOF": ALL6, "Value": [0, 0, 0, 0, 0, 0]}},
                "Force": {"Load": {"Surface": [loaded], "DOF": ["Z"], "Value": [value]}}}}


def _lattice(geoms, cells, radii=None):
    return LatticeSim(_preset(geoms, cells, radii or [0.05 - 0.01 * i for i in range(len(geoms))]))


def _device(L, **kw):
    lat, pen = L.lattice, L.penalized
    dev = _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU, **kw)
    dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
    return dev


def _inputs(dev, seed):
    """Random conductivities and films per strut (one film zero), a random mask, and two random nodal fields."""
    rng = np.random.default_rng(seed)
    kap = 0.1 + 0.3 * rng.random(dev.n_beams)
    film = 0.02 + 0.06 * rng.random(dev.n_beams)
    film[rng.integers(dev.n_beams)] = 0.0
    fixed = rng.random(dev.n_nodes) < 0.3
    fixed[rng.integers(dev.n_nodes)] = True
    return kap, film, fixed, 20.0 + 60.0 * rng.random(dev.n_nodes), rng.standard_normal(dev.n_nodes)


def _close(got, ref, tol, what):
    """|got - ref| <= tol x the largest magnitude of ref."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    assert err <= tol * scale, (what, err / scale if scale else err)


def _compare(dev, T, mu, fixed):
    """The products against the restatement: values within 1e-12 of the largest magnitude, cond_sens within 1e-10 (the bounds
    of tests/test_gpu_conduction.py)."""
    _close(dev.cond_spmv(T), dev.cond_spmv_host(T), 1e-12, "(K_T + H) x")
    _close(dev.cond_spmv(T, fixed), dev.cond_spmv_host(T, fixed), 1e-12, "P (K_T + H) P x")
    assert not dev.cond_spmv(T, fixed)[fixed].any()
    _close(dev.cond_sens(T, mu), dev.cond_sens_host(T, mu), 1e-10, "cond_sens")
    Qc, P = dev.cond_film(T, total=True)
    Qc_h, P_h = dev.cond_film_host(T, total=True)
    _close(Qc, Qc_h, 1e-12, "Qc")
    _close(dev.cond_film(T), Qc_h, 1e-12, "Qc alone")
    assert abs(P - P_h) <= 1e-12 * np.abs(Qc_h * (1.0 if dev._mult is None else dev._mult)).sum(), "P"
    free = ~fixed
    for nodes, ref, p in ((None, 25.0, 8.0), (free, 25.0, 8.0), (free, T_INF, 1.0), (None, 40.0, 3.5)):
        got = dev.temp_pnorm(T, p, ref, nodes, gradient=True)
        want = dev.temp_pnorm_host(T, p, ref, nodes, gradient=True)
        assert want["phi"] >= want["max"] > 0.0
        for k in ("phi", "max", "sum"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, p, got[k], want[k])
        _close(got["dphi_dT"], want["dphi_dT"], 1e-12, "dphi_dT")
        if nodes is not None:
            assert not got["dphi_dT"][~nodes].any()
    # a reference above every temperature: all outputs zero
    got = dev.temp_pnorm(T, 8.0, T.max() + 1.0, None, gradient=True)
    assert got["phi"] == 0.0 and got["max"] == 0.0 and got["sum"] == 0.0 and not got["dphi_dT"].any()
    # a NaN adds nothing
    Tn = T.copy()
    Tn[0] = np.nan
    got, want = dev.temp_pnorm(Tn, 8.0, 25.0, None, gradient=True), dev.temp_pnorm_host(Tn, 8.0, 25.0, None, gradient=True)
    assert abs(got["phi"] - want["phi"]) <= 1e-12 * want["phi"] and got["dphi_dT"][0] == 0.0


CASES = [("BCC",), ("Octet",), ("BCC", "Hybrid1"), ("Octet", "Hybrid4")]


@pytest.mark.parametrize("geoms", CASES, ids=lambda v: "+".join(v))
def test_parity_with_the_restatement(geoms):
    """1 x 1 x 1 cells, reorder 0 and 1 (node and strut permutations), 1, 4 and 16 lanes per node; each with a multiplicity
    vector and one film for every strut, and with a film per strut."""
    L = _lattice(geoms, (1, 1, 1))
    mult = np.random.default_rng(8).integers(1, 3, L.lattice.n_beams).astype(float)
    for reorder, lpn in ((0, 4), (1, 1), (1, 4), (1, 16)):
        with _device(L, reorder=reorder, lanes_per_node=lpn, beam_mult=mult) as dev:
            dev.assemble()
            kap, film, fixed, T, mu = _inputs(dev, 3)
            dev.set_conduction(0.0, kap)
            dev.set_convection(0.05, T_INF)
            _compare(dev, T, mu, fixed)
        with _device(L, reorder=reorder, lanes_per_node=lpn) as dev:
            dev.assemble()
            dev.set_conduction(0.0, kap)
            dev.set_convection(0.0, T_INF, film)
            _compare(dev, T, mu, fixed)
            plain = dev.cond_sens(T, mu, convective=False)                # the switch lifts the state and puts it back
            _close(plain, CH.cond_sens(dev.beam_conn, dev._radius, dev._g_host(), T, mu), 1e-10, "cond_sens without the bracket")
            _close(dev.cond_sens(T, mu), dev.cond_sens_host(T, mu), 1e-10, "cond_sens after the switch")


def _faces(L, dev, dirichlet):
    """Hot Zmin (dirichlet) and a total inflow of 1.5 on Zmax."""
    lo, hi = L.find_point_on_lattice_surface(["Zmin"]), L.find_point_on_lattice_surface(["Zmax"])
    fixed = np.zeros(dev.n_nodes, bool)
    t_bar = np.random.default_rng(1).random(dev.n_nodes)                # (values on free nodes must not matter)
    if dirichlet:
        fixed[lo] = True
        t_bar[lo] = 90.0
    q = np.zeros(dev.n_nodes)
    q[hi] = 1.5 / len(hi)
    return fixed, t_bar, q


@pytest.mark.parametrize("dirichlet", [True, False], ids=["hot-face+inflow", "no-fixed-node"])
def test_solved_temperatures_against_the_dense_host_solve(dirichlet):
    """2 x 2 x 2 BCC, rtol 1e-12: relative L2 error below 1e-7, the bound of tests/test_gpu_conduction.py; the adjoint solve
    the same way; the heat balance of the solved field."""
    L = _lattice(("BCC",), (2, 2, 2))
    with _device(L) as dev:
        dev.assemble()
        kap = 0.1 + 0.3 * np.random.default_rng(6).random(dev.n_beams)
        dev.set_conduction(0.0, kap)
        dev.set_convection(0.05, T_INF)
        fixed, t_bar, q = _faces(L, dev, dirichlet)
        T, st = dev.cond_solve(fixed, t_bar, q, rtol=1e-12, max_iter=10000)
        ref = dev.cond_solve_host(fixed, t_bar, q)
        err = np.linalg.norm(T - ref) / np.linalg.norm(ref)
        print(f"\nsolved temperatures against the dense host solve: relative L2 error {err:.2e}, "
              f"{st['iterations']} iterations, rel_residual {st['rel_residual']:.2e}")
        assert err < 1e-7
        assert st["converged"] == 1 and 0 < st["iterations"] <= 10000 and st["rel_residual"] <= 1e-12
        assert T[fixed].tobytes() == t_bar[fixed].tobytes()
        assert ref.max() > ref.min() + 10.0 and ref.min() >= T_INF       # a field, and no undershoot
        mu, _ = dev.cond_solve(fixed, None, q, rtol=1e-12, max_iter=10000, adjoint=True)
        ref_mu = dev.cond_solve_host(fixed, None, q, adjoint=True)
        assert np.linalg.norm(mu - ref_mu) < 1e-7 * np.linalg.norm(ref_mu) and not mu[fixed].any()
        # balance: P = free inflow + Dirichlet reaction heat
        _, P = dev.cond_film(T, total=True)
        H = dev._H_host()[0]
        reaction = (dev.cond_spmv(T) - H * T_INF)[fixed].sum()
        assert abs(P - (q[~fixed].sum() + reaction)) <= 1e-9 * P
        if not dirichlet:
            assert abs(P - 1.5) <= 1e-9 * 1.5


def test_bitwise_reproducible_over_many_blocks():
    """6 x 6 x 6 Octet, more than one block of nodes and of struts, so the two-stage folds run: two calls return equal bytes."""
    L = _lattice(("Octet",), (6, 6, 6), [0.03])
    assert L.lattice.n_beams > 5000 and L.lattice.n_nodes > 4 * 256
    with _device(L) as dev:
        dev.assemble()
        kap, film, fixed, T, mu = _inputs(dev, 6)
        dev.set_conduction(0.0, kap)
        dev.set_convection(0.0, T_INF, film)
        for call in (lambda: dev.cond_spmv(T), lambda: dev.cond_spmv(T, fixed), lambda: dev.cond_sens(T, mu),
                     lambda: dev.cond_film(T), lambda: dev.temp_pnorm(T, 8.0, 25.0, ~fixed, gradient=True)["dphi_dT"]):
            assert call().tobytes() == call().tobytes()
        totals = [dev.cond_film(T, total=True)[1] for _ in range(2)]
        assert np.float64(totals[0]).tobytes() == np.float64(totals[1]).tobytes()
        norms = [dev.temp_pnorm(T, 8.0, 25.0, ~fixed) for _ in range(2)]
        assert all(np.float64(norms[0][k]).tobytes() == np.float64(norms[1][k]).tobytes() for k in ("phi", "max", "sum"))
        _compare(dev, T, mu, fixed)


def test_state_survives_new_radii_and_clears():
    """Convection survives update_radii + assemble and c ~ r shows in cond_film; clear_convection gives back the bytes of a
    handle that never had it; a new conduction state drops it."""
    L = _lattice(("Octet",), (2, 2, 1), [0.04])
    with _device(L) as dev, _device(L) as plain:
        kap, film, fixed, T, mu = _inputs(dev, 5)
        for d in (dev, plain):
            d.assemble()
            d.set_conduction(0.0, kap)
        dev.set_convection(0.0, T_INF, film)
        Qc = dev.cond_film(T)
        assert dev.cond_spmv(T).tobytes() != plain.cond_spmv(T).tobytes()
        for d in (dev, plain):
            d.update_radii(0.8 * L.lattice.beam_radius)
            d.assemble()
        _compare(dev, T, mu, fixed)
        _close(dev.cond_film(T), 0.8 * Qc, 1e-12, "c ~ r")
        dev.clear_convection()
        for m in (None, fixed):
            assert dev.cond_spmv(T, m).tobytes() == plain.cond_spmv(T, m).tobytes()
        assert dev.cond_sens(T, mu).tobytes() == plain.cond_sens(T, mu).tobytes()
        dev.set_convection(0.05, T_INF)
        dev.set_conduction(0.0, kap)                                      # a new conduction state: no convection
        assert dev._convection is None
        assert dev.cond_spmv(T).tobytes() == plain.cond_spmv(T).tobytes()


def test_error_codes():
    L = _lattice(("BCC",), (2, 1, 1))
    lib = _capi.load_library()
    p = _capi._ptr

    def code(fn, *a, **kw):
        with pytest.raises(_capi.PlError) as e:
            fn(*a, **kw)
        return e.value.code

    with _device(L) as dev:
        n, nb = dev.n_nodes, dev.n_beams
        x, yb, out3 = np.arange(n, dtype=float), np.empty(nb), np.zeros(3)
        y, tot = np.empty(n), np.zeros(1)
        none, fixed = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        fixed[0] = 1
        assert lib.pl_temp_pnorm(dev._h, p(x), None, 0.0, 8.0, p(out3), None) == _capi.PL_ERR_STATE   # not assembled
        assert b"pl_assemble" in lib.pl_last_error()
        dev.assemble()
        assert lib.pl_temp_pnorm(dev._h, p(x), None, 0.0, 8.0, p(out3), None) == _capi.PL_OK          # no conduction state
        assert out3[1] == n - 1.0
        for bad in (0.5, np.nan, np.inf, -2.0):
            assert lib.pl_temp_pnorm(dev._h, p(x), None, 0.0, bad, p(out3), None) == _capi.PL_ERR_ARG
        assert lib.pl_temp_pnorm(dev._h, None, None, 0.0, 8.0, p(out3), None) == _capi.PL_ERR_ARG
        assert lib.pl_temp_pnorm(dev._h, p(x), None, 0.0, 8.0, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_temp_pnorm(dev._h, p(x), None, 0.0, 8.0, None, p(y)) == _capi.PL_OK
        assert code(dev.set_convection, 0.05, T_INF) == _capi.PL_ERR_STATE                           # no conduction state
        assert b"pl_set_conduction" in lib.pl_last_error()
        dev.set_conduction(0.2)
        assert code(dev.cond_film, x) == _capi.PL_ERR_STATE                                          # no convection state
        assert b"pl_set_convection" in lib.pl_last_error()
        for bad in (-1.0, np.nan, np.inf):
            assert code(dev.set_convection, bad, T_INF) == _capi.PL_ERR_ARG
            bf = np.full(nb, 0.05)
            bf[nb // 2] = bad
            assert code(dev.set_convection, 0.0, T_INF, bf) == _capi.PL_ERR_ARG
        assert code(dev.set_convection, 0.0, T_INF, np.zeros(nb)) == _capi.PL_ERR_ARG                # every film zero
        for bad in (np.nan, np.inf):
            assert code(dev.set_convection, 0.05, bad) == _capi.PL_ERR_ARG
        assert dev._convection is None
        # the two all-zero-mask cases, and a NULL mask
        assert lib.pl_cond_solve(dev._h, p(none), None, None, 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve_adjoint(dev._h, p(none), p(x), 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        dev.set_convection(0.05, T_INF)
        assert lib.pl_cond_solve(dev._h, p(none), None, None, 1e-8, 100, p(y), None) == _capi.PL_OK
        assert np.abs(y - T_INF).max() <= 1e-6 * T_INF                    # nothing flows in: the ambient everywhere
        assert lib.pl_cond_solve(dev._h, None, None, None, 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve_adjoint(dev._h, p(none), p(x), 1e-8, 100, p(y), None) == _capi.PL_OK
        assert lib.pl_cond_solve_adjoint(dev._h, p(none), None, 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve_adjoint(dev._h, None, p(x), 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve_adjoint(dev._h, p(fixed), p(x), 1e-8, 100, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve_adjoint(dev._h, p(fixed), p(x), 0.0, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_film(dev._h, None, p(yb), p(tot)) == _capi.PL_ERR_ARG
        assert lib.pl_cond_film(dev._h, p(x), None, None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_film(dev._h, p(x), None, p(tot)) == _capi.PL_OK
        assert lib.pl_cond_film(dev._h, p(x), p(yb), None) == _capi.PL_OK
        assert abs(tot[0] - dev.cond_film_host(x, total=True)[1]) <= 1e-12 * abs(tot[0])
        dev.update_radii(dev._radius)                                     # clears the assembly, not the state
        assert code(dev.cond_film, x) == _capi.PL_ERR_STATE
        assert b"pl_assemble" in lib.pl_last_error()
        dev.assemble()
        assert dev.cond_film(x).shape == (nb,)
        dev.clear_conduction()                                            # takes the convection with it
        assert dev._convection is None
        dev.set_conduction(0.2)
        assert code(dev.cond_film, x) == _capi.PL_ERR_STATE
        assert b"pl_set_convection" in lib.pl_last_error()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        two, one, o3 = np.zeros(2), np.ones(2, np.uint8), np.zeros(3)
        assert lib.pl_set_convection(ddm._h, 0.05, None, T_INF) == _capi.PL_ERR_STATE
        assert lib.pl_cond_film(ddm._h, p(two), p(two), None) == _capi.PL_ERR_STATE
        assert lib.pl_cond_solve_adjoint(ddm._h, p(one), p(two), 1e-8, 10, p(two), None) == _capi.PL_ERR_STATE
        assert lib.pl_temp_pnorm(ddm._h, p(two), None, 0.0, 8.0, p(o3), None) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            xn, xb, o3 = np.zeros(dev.n_nodes), np.zeros(dev.n_beams), np.zeros(3)
            m = np.ones(dev.n_nodes, np.uint8)
            assert lib.pl_set_convection(dev._h, 0.05, None, T_INF) == _capi.PL_ERR_STATE
            assert lib.pl_cond_film(dev._h, p(xn), p(xb), None) == _capi.PL_ERR_STATE
            assert lib.pl_cond_solve_adjoint(dev._h, p(m), p(xn), 1e-8, 10, p(xn), None) == _capi.PL_ERR_STATE
            assert lib.pl_temp_pnorm(dev._h, p(xn), None, 0.0, 8.0, p(o3), None) == _capi.PL_ERR_STATE


# ---------------------------------------------------------------------------------------------------------------------
# LatticeSim
# ---------------------------------------------------------------------------------------------------------------------
CONDUCTION = {"conductivity": 0.2, "reference": 20.0, "Temperature": {"Hot": {"Surface": ["Zmin"], "Value": 90.0}},
              "HeatFlow": {"Top": {"Surface": ["Zmax"], "Value": 1.5}}, "Convection": {"film": 0.05, "ambient": T_INF}}


def test_through_lattice_sim():
    """A preset with the "Convection" block equals the hand-built handle (both PCG solves stop at rtol 1e-12: 1e-9 of the
    field), dissipated_power satisfies the balance, and a problem without a prescribed temperature is accepted with convection
    only."""
    p = _preset(("BCC",), (2, 2, 2), [0.05])
    p["simulation_parameters"]["thermal"] = {"alpha": 7e-5, "conduction": copy.deepcopy(CONDUCTION)}
    L = LatticeSim(p)
    assert L.conduction["convection"] == {"film": 0.05, "ambient": T_INF, "beam_film": None}
    T = L.solve_temperature()
    with _device(_lattice(("BCC",), (2, 2, 2))) as dev:
        dev.assemble()
        dev.set_conduction(0.2)
        dev.set_convection(0.05, T_INF)
        fixed, t_bar, q = _faces(L, dev, True)
        T_hand, _ = dev.cond_solve(fixed, t_bar, q, rtol=1e-12)
        ref_T = dev.cond_solve_host(fixed, t_bar, q)
        Qc_ref, P_ref = dev.cond_film_host(ref_T, total=True)
        H = dev._H_host()[0]
        reaction = (dev.cond_spmv_host(ref_T) - H * T_INF)[fixed].sum()
    assert np.linalg.norm(T - T_hand) <= 1e-9 * np.linalg.norm(T_hand)
    assert np.linalg.norm(T - ref_T) < 1e-7 * np.linalg.norm(ref_T)
    _close(L.strut_heat_loss(), Qc_ref, 1e-7, "strut_heat_loss")
    P = L.dissipated_power()
    assert abs(P - P_ref) <= 1e-7 * P_ref
    assert abs(P - (1.5 + reaction)) <= 1e-7 * P
    peak, phi = L.max_temperature(p=8)
    free = ~fixed
    assert abs(peak - (ref_T[free] - T_INF).max()) <= 1e-7 * peak and peak == L.max_temperature()
    assert abs(phi - CH.temp_pnorm(ref_T, 8.0, T_INF, free)[0]) <= 1e-7 * phi and phi >= peak
    assert abs(L.max_temperature(reference=30.0) - (peak - 10.0)) <= 1e-12 * peak
    # convection only: accepted; without it the refusal stays
    L2 = _lattice(("BCC",), (2, 2, 2))
    T2 = L2.solve_temperature(0.2, None, q, convection={"film": 0.05, "ambient": T_INF})
    assert abs(L2.dissipated_power() - 1.5) <= 1e-9 * 1.5 and T2.min() > T_INF
    with pytest.raises(ValueError):
        _lattice(("BCC",), (2, 2, 2)).solve_temperature(0.2, None, q)
    with pytest.raises(ValueError):
        L2.solve_temperature(0.2, np.full(L2.lattice.n_nodes, np.nan), q)
    # the same problem without the block: no convection on the handle any more
    L2.solve_temperature(0.2, (fixed, t_bar), q)
    assert L2._device._convection is None
    with pytest.raises(RuntimeError, match="convection"):
        L2.dissipated_power()
    for sim in (L, L2):
        sim._device.close()


# ---------------------------------------------------------------------------------------------------------------------
# LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
OPTI = _preset(("BCC",), (3, 2, 2), [0.05])
OPTI["gradient"] = {"radii": {"rule": "linear", "direction_x": True, "direction_y": False, "direction_z": False,
                              "parameter_x": 0.2, "parameter_y": 0.0, "parameter_z": 0.0}}
OPTI["boundary_conditions"]["Force"]["Load"]["Surface"] = ["Xmax", "Zmax"]
OPTI["simulation_parameters"]["thermal"] = {"alpha": 7e-5, "conduction": copy.deepcopy(CONDUCTION)}
OPTI["optimization_informations"] = {
    "objective_function": "min", "objective_type": "thermal_compliance", "max_iterations": 5,
    "optimization_parameters": {"type": "unit_cell"},
    "constraints": {"relative_density": {"value": 0.05}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}
IDXS = [0, 5, 11]


def _opti(**opt):
    p = copy.deepcopy(OPTI)
    constraints = opt.pop("constraints", {})
    p["optimization_informations"].update(opt)
    p["optimization_informations"]["constraints"].update(constraints)
    return p


def _fd(value, theta, i, h=1e-4):
    tp, tm = list(theta), list(theta)
    tp[i] += h
    tm[i] -= h
    return (value(tp) - value(tm)) / (2 * h)


def _check_gradient(L, value, gradient, what, must_miss=True):
    """Central differences, step 1e-4 and the 2e-3 bound of tests/test_gpu_conduction.py, at variables 0, 5 and 11; with the
    convective bracket of cond_sens switched off at least one of them misses the bound (must_miss), or, where the temperature
    is a small part of the gradient, every one of them is further from the difference quotient than the full gradient is."""
    assert L.number_parameters == 12
    theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
    value(theta)
    g = np.asarray(gradient(theta))
    fds = {i: _fd(value, theta, i) for i in IDXS}
    value(theta)
    L.convection_chain = False
    wrong = np.asarray(gradient(theta))
    L.convection_chain = True
    for i in IDXS:
        print(f"\n{what} variable {i}: gradient {g[i]:.8e}, difference quotient {fds[i]:.8e}, "
              f"without the convective bracket {wrong[i]:.8e}")
    for i in IDXS:
        assert abs(g[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(g).max()), (what, i, g[i], fds[i])
    if must_miss:
        assert any(not abs(wrong[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(wrong).max()) for i in IDXS), (wrong, fds)
    else:
        assert all(abs(wrong[i] - fds[i]) > abs(g[i] - fds[i]) for i in IDXS), (wrong, g, fds)
    # the switch left nothing behind (the adjoint solves stop at rtol 1e-10 from a warm start: not the same bits)
    assert np.abs(np.asarray(gradient(theta)) - g).max() <= 1e-8 * np.abs(g).max()


@pytest.mark.parametrize("objective,sense", [("thermal_compliance", "min"), ("heat_dissipation", "max")])
def test_thermal_objective_gradients(objective, sense):
    L = LatticeOpti(_opti(objective_type=objective, objective_function=sense))
    assert not L._needs_mechanics and L._needs_temperature
    _check_gradient(L, L.objective, L.gradient, objective)
    assert getattr(L, "_model", None) is None                             # no mechanical equilibrium was solved
    L._device.close()


def test_max_temperature_constraint():
    """Phi_p / limit - 1 and its gradient beside a mechanical objective; the peak is kept for the history."""
    L = LatticeOpti(_opti(objective_type="compliance", constraints={"max_temperature": {"limit": 60.0}}))
    assert L._needs_mechanics and L._needs_temperature and "max_temperature" in L._history
    theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
    v = L.max_temperature_constraint(theta)
    phi, peak = L._last_max_temperature
    free = ~L.conduction["fixed"]
    assert v == phi / 60.0 - 1.0 and phi >= peak > 0.0
    assert abs(peak - (L.temperature_field[free] - T_INF).max()) <= 1e-12 * peak
    assert abs(phi - CH.temp_pnorm(L.temperature_field, 8.0, T_INF, free)[0]) <= 1e-12 * phi
    _check_gradient(L, L.max_temperature_constraint, L.max_temperature_constraint_gradient, "max_temperature")
    L._device.close()


def test_compliance_gradient_under_a_conduction_driven_temperature_with_convection():
    """The existing thermo-elastic chain of LatticeOpti._sens: the adjoint operator is K_T + H and cond_sens carries the bracket.
    The mechanical part dominates this gradient (the bracket moves it by 5e-4 of its largest component), so the check without
    the bracket is the weaker one of _check_gradient."""
    L = LatticeOpti(_opti(objective_type="compliance"))
    assert L.conduction_driven and L._needs_mechanics and not L._needs_temperature
    _check_gradient(L, L.objective, L.gradient, "compliance", must_miss=False)
    L._device.close()


def test_refusals():
    p = _opti(objective_type="heat_dissipation", objective_function="max")
    del p["simulation_parameters"]["thermal"]["conduction"]["Convection"]
    with pytest.raises(ValueError, match="Convection"):
        LatticeOpti(p)
    p = _opti(objective_type="thermal_compliance")
    del p["simulation_parameters"]["thermal"]
    with pytest.raises(ValueError, match="conduction problem"):
        LatticeOpti(p)
    ddm = {"geometry": _preset(("BCC",), (2, 1, 1), [0.05])["geometry"],
           "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                     "DDM": {"enable_preconditioner": False, "max_iterations": 1000,
                                             "schur_complement_computation": {"type": "exact"}}},
           "boundary_conditions": _preset(("BCC",), (2, 1, 1), [0.05])["boundary_conditions"]}
    info = dict(copy.deepcopy(OPTI["optimization_informations"]), simulation_type="DDM",
                optimization_parameters={"type": "constant", "hybrid": False})
    for change in ({"objective_type": "thermal_compliance"}, {"objective_type": "heat_dissipation"},
                   {"objective_type": "compliance", "constraints": {"max_temperature": {"limit": 60.0}}}):
        with pytest.raises(NotImplementedError, match="FEM"):
            LatticeOpti(dict(copy.deepcopy(ddm), optimization_informations=dict(info, **change)))
