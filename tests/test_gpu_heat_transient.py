"""Transient heat conduction on the device (pl_set_heat_capacity / pl_cond_transient, csrc/pl_heat.h) against the dense numpy
restatement (conduction_host.transient): every row, the balance columns and the snapshots on small lattices in every node
ordering and lane mapping, several blocks with a grid tail, a continued history, the closed form, the heat balance, the steady
limit, the life of the state, the error codes, and LatticeSim.transient_temperature.  All solves stop at rtol = 1e-12."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import conduction_host as CH                     # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

E, NU = 1013.0, 0.3
ALL6 = ["X", "Y", "Z", "RX", "RY", "RZ"]
T_INF = 20.0
RTOL = 1e-12


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


def _device(L, radius=None, **kw):
    lat, pen = L.lattice, L.penalized
    dev = _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius if radius is None else radius, pen.seg_len,
                           pen.seg_nsub, E, NU, **kw)
    dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
    return dev


def _inputs(n_nodes, n_beams, n_steps, seed):
    """Random materials per strut (one film zero), node capacities, a random 30 % mask, end values, a start field, two patterns
    with random amplitudes and a ramp."""
    rng = np.random.default_rng(seed)
    film = 0.02 + 0.06 * rng.random(n_beams)
    film[rng.integers(n_beams)] = 0.0
    fixed = rng.random(n_nodes) < 0.3
    fixed[rng.integers(n_nodes)] = True
    return {"kappa": 0.1 + 0.3 * rng.random(n_beams), "film": film, "rho_c": 1.0 + 2.0 * rng.random(n_beams),
            "node_capacity": 0.01 * rng.random(n_nodes), "fixed": fixed, "t_bar": 60.0 + 30.0 * rng.random(n_nodes),
            "t0": 20.0 + 5.0 * rng.random(n_nodes), "patterns": rng.standard_normal((2, n_nodes)),
            "amp": rng.standard_normal((n_steps + 1, 2)), "bar_amp": np.linspace(0.0, 1.0, n_steps + 1) ** 2}


def _set_states(dev, d):
    dev.set_conduction(0.0, d["kappa"])
    dev.set_convection(0.0, T_INF, d["film"])
    dev.set_heat_capacity(0.0, d["rho_c"], d["node_capacity"])


def _run_both(dev, d, dt, n_steps, theta, snap_every=0):
    """(device dict, host dict) of the same call, every node probed."""
    args = dict(theta=theta, fixed=d["fixed"], t_bar=d["t_bar"], bar_amp=d["bar_amp"], patterns=d["patterns"], amp=d["amp"],
                t0=d["t0"], probes=np.arange(dev.n_nodes), snap_every=snap_every)
    return dev.cond_transient(dt, n_steps, rtol=RTOL, max_iter=10000, **args), dev.cond_transient_host(dt, n_steps, **args)


def _check_rows(got, ref, fixed, tol=1e-7, what=""):
    """probe, snaps and state within tol of the largest |T - T_inf| of the restatement, every balance column within tol of its
    largest magnitude, the fixed nodes bit-equal to their row value, iters[0] = 0."""
    rise = np.abs(ref["T"] - T_INF).max()
    assert rise > 1.0, what
    err = np.abs(got["probe"] - ref["T"]).max() / rise
    errs = [np.abs(got["heat"][:, k] - ref["heat"][:, k]).max() / np.abs(ref["heat"][:, k]).max() for k in range(4)]
    print(f"\n{what}: rows {err:.2e} of the largest rise, balance columns {['%.2e' % e for e in errs]}, "
          f"iterations {got['iters'].tolist()}")
    assert err <= tol, (what, err)
    assert np.abs(got["state"] - ref["state"]).max() <= tol * rise, what
    if "snaps" in ref:
        assert got["snaps"].shape == ref["snaps"].shape and np.abs(got["snaps"] - ref["snaps"]).max() <= tol * rise, what
    assert max(errs) <= tol, (what, errs)
    assert got["probe"][:, fixed].tobytes() == ref["bar"][:, fixed].tobytes(), what
    assert got["state"][fixed].tobytes() == ref["bar"][-1, fixed].tobytes(), what
    assert got["iters"][0] == 0 and (got["iters"][1:] > 0).all(), what
    assert np.array_equal(got["times"], ref["times"])


CASES = [("BCC",), ("Octet",), ("BCC", "Hybrid1"), ("Octet", "Hybrid4")]


@pytest.mark.parametrize("geoms", CASES, ids=lambda v: "+".join(v))
def test_rows_against_the_restatement(geoms):
    """1 x 1 x 1 cells at (reorder, lanes per node) = (0, 4), (1, 1), (1, 4), (1, 16), theta = 1/2 and 1, 6 steps."""
    L = _lattice(geoms, (1, 1, 1))
    lat = L.lattice
    mult = np.random.default_rng(8).integers(1, 3, lat.n_beams).astype(float)
    radius = lat.beam_radius * (0.8 + 0.4 * np.random.default_rng(2).random(lat.n_beams))
    d = _inputs(lat.n_nodes, lat.n_beams, 6, 3)
    for reorder, lpn in ((0, 4), (1, 1), (1, 4), (1, 16)):
        with _device(L, radius, reorder=reorder, lanes_per_node=lpn, beam_mult=mult) as dev:
            dev.assemble()
            _set_states(dev, d)
            for theta in (0.5, 1.0):
                got, ref = _run_both(dev, d, 0.2, 6, theta, snap_every=2)
                assert got["snaps"].shape == (3, dev.n_nodes)
                _check_rows(got, ref, d["fixed"], what=f"{'+'.join(geoms)} reorder {reorder} lpn {lpn} theta {theta}")


def test_several_blocks_and_a_continued_history():
    """6 x 6 x 6 Octet: more than one block of nodes, N no multiple of the block.  3 steps against the dense restatement; 6
    steps in one call against 3 + 3 continued from ``state``, within 1e-10 of the largest rise."""
    L = _lattice(("Octet",), (6, 6, 6), [0.03])
    N = L.lattice.n_nodes
    assert N > 4 * 256 and N % 256 != 0
    d = _inputs(N, L.lattice.n_beams, 6, 6)
    d["bar_amp"] = None                       # (a continued call starts its ramp from its own start field)
    with _device(L) as dev:
        dev.assemble()
        _set_states(dev, d)
        d3 = dict(d, amp=d["amp"][:4])
        got, ref = _run_both(dev, d3, 0.2, 3, 1.0, snap_every=3)
        _check_rows(got, ref, d["fixed"], what="6 x 6 x 6 Octet, 3 steps")
        whole = dev.cond_transient(0.2, 6, 1.0, d["fixed"], d["t_bar"], None, d["patterns"], d["amp"], d["t0"], rtol=RTOL,
                                   probes=np.arange(N))
        second = dev.cond_transient(0.2, 3, 1.0, d["fixed"], d["t_bar"], None, d["patterns"], d["amp"][3:], got["state"],
                                    rtol=RTOL, probes=np.arange(N))
        rise = np.abs(ref["T"] - T_INF).max()
        assert np.abs(whole["probe"][:4] - got["probe"]).max() <= 1e-10 * rise
        err = np.abs(whole["probe"][3:] - second["probe"]).max() / rise
        print(f"\n6 steps against 3 + 3: {err:.2e} of the largest rise")
        assert err <= 1e-10
        assert np.abs(whole["state"] - second["state"]).max() <= 1e-10 * rise


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_closed_form_on_the_device(theta):
    """2 x 2 x 2 BCC, uniform radii, no fixed node, no inflow, from 90 in an ambient of 20: the field stays uniform and
    T_n - T_inf = 70 ((1 - (1 - theta) a) / (1 + theta a))^n, a = 2 h dt / (rho_c r) = 0.3; within 1e-9 of 70."""
    L = _lattice(("BCC",), (2, 2, 2), [0.05])
    with _device(L) as dev:
        dev.assemble()
        dev.set_conduction(0.2)
        dev.set_convection(0.05, T_INF)
        dev.set_heat_capacity(2.0)
        out = dev.cond_transient(0.3, 10, theta, t0=np.full(dev.n_nodes, 90.0), rtol=RTOL, probes=np.arange(dev.n_nodes))
    want = 70.0 * ((1.0 - (1.0 - theta) * 0.3) / (1.0 + theta * 0.3)) ** np.arange(11)
    err = np.abs(out["probe"] - T_INF - want[:, None]).max()
    print(f"\nclosed form on the device, theta = {theta}: largest error {err:.2e}")
    assert err <= 1e-9 * 70.0


def _balance_case():
    """The balance case of tests/test_heat_transient_host.py."""
    L = _lattice(("BCC", "Hybrid1"), (2, 2, 2), [0.05, 0.04])
    lat = L.lattice
    rng = np.random.default_rng(11)
    N, B, n_steps = lat.n_nodes, lat.n_beams, 12
    rad = lat.beam_radius * (0.8 + 0.4 * rng.random(B))
    mult = rng.integers(1, 3, B).astype(float)
    rho_c, node_cap = 1.0 + 2.0 * rng.random(B), 0.01 * rng.random(N)
    fixed = np.zeros(N, bool)
    fixed[L.find_point_on_lattice_surface(["Zmin"])] = True
    t_bar = 60.0 + 30.0 * rng.random(N)
    d = {"fixed": fixed, "t_bar": t_bar, "bar_amp": np.linspace(0.0, 1.0, n_steps + 1) ** 2,
         "patterns": rng.standard_normal((2, N)), "amp": rng.standard_normal((n_steps + 1, 2)), "t0": 20.0 + 5.0 * rng.random(N)}
    return L, rad, mult, rho_c, node_cap, d, n_steps


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_balance_on_the_device(theta):
    """U_n - U_0 = Q_in + Q_R - Q_c in every row within 1e-8 of the largest column: the solver's residual at rtol = 1e-12
    over the run."""
    L, rad, mult, rho_c, node_cap, d, n_steps = _balance_case()
    with _device(L, rad, beam_mult=mult) as dev:
        dev.assemble()
        dev.set_conduction(0.2)
        dev.set_convection(0.05, T_INF)
        dev.set_heat_capacity(0.0, rho_c, node_cap)
        got, ref = _run_both(dev, d, 0.2, n_steps, theta)
    U, Qin, Qc, QR = got["heat"].T
    assert Qin[0] == 0.0 and Qc[0] == 0.0 and QR[0] == 0.0
    scale = np.abs(got["heat"]).max()
    defect = np.abs((U - U[0]) - (Qin + QR - Qc)).max() / scale
    print(f"\nbalance on the device, theta = {theta}: defect {defect:.2e} of the largest column")
    assert defect <= 1e-8
    _check_rows(got, ref, d["fixed"], what=f"balance case, theta {theta}")


def _faces(L, n):
    lo, hi = L.find_point_on_lattice_surface(["Zmin"]), L.find_point_on_lattice_surface(["Zmax"])
    fixed = np.zeros(n, bool)
    fixed[lo] = True
    t_bar = np.where(fixed, 90.0, 0.0)
    q = np.zeros(n)
    q[hi] = 1.5 / len(hi)
    return fixed, t_bar, q


def test_steady_limit():
    """Large backward-Euler steps end at the steady field of cond_solve at the same rtol, within 1e-7."""
    L = _lattice(("BCC",), (2, 2, 2), [0.05])
    with _device(L) as dev:
        dev.assemble()
        dev.set_conduction(0.2)
        dev.set_convection(0.05, T_INF)
        dev.set_heat_capacity(2.0)
        fixed, t_bar, q = _faces(L, dev.n_nodes)
        out = dev.cond_transient(50.0, 12, 1.0, fixed, t_bar, None, q[None], np.ones((13, 1)), rtol=RTOL, max_iter=10000)
        T, _ = dev.cond_solve(fixed, t_bar, q, rtol=RTOL, max_iter=10000)
    err = np.abs(out["state"] - T).max() / np.abs(T - T_INF).max()
    print(f"\nsteady limit: {err:.2e} of the largest rise")
    assert err <= 1e-7


def test_state_and_life():
    L = _lattice(("Octet",), (2, 2, 1), [0.04])
    lat = L.lattice
    d = _inputs(lat.n_nodes, lat.n_beams, 4, 5)
    x = np.random.default_rng(4).standard_normal(lat.n_nodes)
    with _device(L) as dev:
        f = np.zeros((dev.n_nodes, 6))
        f[L.find_point_on_lattice_surface(["Xmax"]), 2] = -0.1
        mask = np.zeros((dev.n_nodes, 6), bool)
        mask[L.find_point_on_lattice_surface(["Xmin"])] = True
        dev.set_bc(mask, None, f)
        dev.assemble()
        _set_states(dev, d)
        u0, _ = dev.solve(rtol=1e-10)
        before = (dev.cond_solve(d["fixed"], d["t_bar"], d["patterns"][0], rtol=RTOL)[0], dev.cond_spmv(x),
                  dev.cond_spmv(x, d["fixed"]))
        got, ref = _run_both(dev, d, 0.2, 4, 1.0)
        _check_rows(got, ref, d["fixed"], what="2 x 2 x 1 Octet")
        after = (dev.cond_solve(d["fixed"], d["t_bar"], d["patterns"][0], rtol=RTOL)[0], dev.cond_spmv(x),
                 dev.cond_spmv(x, d["fixed"]))
        for a, b in zip(before, after):                    # steady conduction is not touched (below 64 blocks: one order)
            assert a.tobytes() == b.tobytes()
        u1, _ = dev.solve(rtol=1e-10)                      # and neither is the mechanical state
        assert np.abs(u1 - u0).max() <= 1e-8 * np.abs(u0).max()
        # new radii: C, g and c follow them
        dev.update_radii(0.8 * lat.beam_radius)
        dev.assemble()
        got2, ref2 = _run_both(dev, d, 0.2, 4, 0.5)
        _check_rows(got2, ref2, d["fixed"], what="after update_radii")
        assert np.abs(ref2["T"] - CH.transient(dev.beam_conn, dev.n_nodes, dev._g_host(), dev.heat_capacity_host(), 0.2, 4, 0.5,
                                               d["fixed"], d["t_bar"], d["bar_amp"], d["patterns"], d["amp"], d["t0"],
                                               dev._H_host()[0], T_INF)["T"]).max() == 0.0
        assert np.allclose(dev.heat_capacity_host() - d["node_capacity"],
                           0.64 * (CH.heat_capacity(lat.node_xyz, lat.beam_conn, lat.beam_radius, d["rho_c"])), rtol=1e-13)
        # insulated: no convection state, an all-zero mask (and a NULL one) - the stored heat stays
        dev.clear_convection()
        t0 = 20.0 + 60.0 * np.random.default_rng(9).random(dev.n_nodes)
        for fx in (np.zeros(dev.n_nodes, bool), None):
            ins = dev.cond_transient(5.0, 4, 1.0, fixed=fx, t0=t0, rtol=RTOL, probes=np.arange(dev.n_nodes))
            U = ins["heat"][:, 0]
            assert np.abs(U - U[0]).max() <= 1e-9 * abs(U[0]) and not ins["heat"][:, 1:].any()
            ref_ins = dev.cond_transient_host(5.0, 4, 1.0, fixed=fx, t0=t0)
            assert np.abs(ins["probe"] - ref_ins["T"]).max() <= 1e-7 * np.abs(ref_ins["T"]).max()
        # a new conduction state drops the capacity
        dev.set_conduction(0.0, d["kappa"])
        assert dev._heat_capacity is None
        with pytest.raises(_capi.PlError) as e:
            dev.cond_transient(0.2, 2, 1.0, t0=t0)
        assert e.value.code == _capi.PL_ERR_STATE and b"pl_set_heat_capacity" in dev._lib.pl_last_error()
        dev.set_heat_capacity(2.0)
        dev.clear_heat_capacity()
        with pytest.raises(_capi.PlError) as e:
            dev.cond_transient(0.2, 2, 1.0, t0=t0)
        assert e.value.code == _capi.PL_ERR_STATE


def test_error_codes():
    """Argument and state checks on the host: nothing is launched before they pass."""
    L = _lattice(("BCC",), (2, 1, 1))
    lib = _capi.load_library()
    p = _capi._ptr

    def code(fn, *a, **kw):
        with pytest.raises(_capi.PlError) as e:
            fn(*a, **kw)
        return e.value.code

    with _device(L) as dev:
        n, nb = dev.n_nodes, dev.n_beams
        assert code(dev.set_heat_capacity, 2.0) == _capi.PL_ERR_STATE                  # no conduction state
        assert b"pl_set_conduction" in lib.pl_last_error()
        dev.set_conduction(0.2)
        for bad in (-1.0, np.nan, np.inf):
            assert code(dev.set_heat_capacity, bad) == _capi.PL_ERR_ARG
            br = np.full(nb, 2.0)
            br[nb // 2] = bad
            assert code(dev.set_heat_capacity, 0.0, br) == _capi.PL_ERR_ARG
            nc = np.zeros(n)
            nc[n // 2] = bad
            assert code(dev.set_heat_capacity, 2.0, None, nc) == _capi.PL_ERR_ARG
        assert code(dev.set_heat_capacity, 0.0, np.zeros(nb)) == _capi.PL_ERR_ARG      # a zero strut value
        assert dev._heat_capacity is None
        assert code(dev.cond_transient, 0.1, 2) == _capi.PL_ERR_STATE                  # no heat capacity
        assert b"pl_set_heat_capacity" in lib.pl_last_error()
        dev.set_heat_capacity(2.0)
        assert code(dev.cond_transient, 0.1, 2) == _capi.PL_ERR_STATE                  # not assembled
        assert b"pl_assemble" in lib.pl_last_error()
        dev.assemble()
        dev.set_convection(0.05, T_INF)
        fixed = np.zeros(n, bool)
        fixed[0] = True
        ok = dict(fixed=fixed, t_bar=np.full(n, 90.0), rtol=1e-10, max_iter=1000)
        assert dev.cond_transient(0.1, 2, **ok)["iters"].tolist()[0] == 0
        for dt in (0.0, -0.1, np.nan, np.inf):
            assert code(dev.cond_transient, dt, 2, **ok) == _capi.PL_ERR_ARG
        assert code(dev.cond_transient, 0.1, 0, **ok) == _capi.PL_ERR_ARG
        for theta in (0.49, 1.01, np.nan, -1.0):
            assert code(dev.cond_transient, 0.1, 2, theta, **ok) == _capi.PL_ERR_ARG
        assert code(dev.cond_transient, 0.1, 2, patterns=np.zeros((5, n)), amp=np.zeros((3, 5)), **ok) == _capi.PL_ERR_ARG
        heat, out = np.zeros((3, 4)), np.zeros(3 * n)
        z = np.zeros(3)
        assert lib.pl_cond_transient(dev._h, 2, 0.1, 1.0, None, None, None, -1, None, None, None, 1e-10, 100, 0, None, None,
                                     p(heat), 0, None, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_transient(dev._h, 2, 0.1, 1.0, None, None, None, 1, None, p(z), None, 1e-10, 100, 0, None, None,
                                     p(heat), 0, None, None, None) == _capi.PL_ERR_ARG       # n_pat > 0 without patterns
        for probes in ([n], [-1], [0, n + 3]):
            assert code(dev.cond_transient, 0.1, 2, probes=probes, **ok) == _capi.PL_ERR_ARG
        for kw in (dict(rtol=0.0), dict(rtol=-1e-8), dict(max_iter=0)):
            assert code(dev.cond_transient, 0.1, 2, **dict(ok, **kw)) == _capi.PL_ERR_ARG
        for bad in (np.nan, np.inf):                                                   # data that is not a number
            spoilt = np.full(n, 30.0)
            spoilt[n // 2] = bad
            assert code(dev.cond_transient, 0.1, 2, **dict(ok, t0=spoilt)) == _capi.PL_ERR_ARG
            assert code(dev.cond_transient, 0.1, 2, **dict(ok, t_bar=spoilt)) == _capi.PL_ERR_ARG
            assert code(dev.cond_transient, 0.1, 2, bar_amp=[0.0, bad, 1.0], **ok) == _capi.PL_ERR_ARG
            assert code(dev.cond_transient, 0.1, 2, patterns=spoilt[None], amp=np.ones((3, 1)), **ok) == _capi.PL_ERR_ARG
            assert code(dev.cond_transient, 0.1, 2, patterns=np.ones((1, n)), amp=[[1.0], [bad], [1.0]], **ok) == _capi.PL_ERR_ARG
        assert b"finite" in lib.pl_last_error()
        assert lib.pl_cond_transient(dev._h, 2, 0.1, 1.0, None, None, None, 0, None, None, None, 1e-10, 100, 0, None, None,
                                     p(heat), 0, p(out), None, None) == _capi.PL_ERR_ARG     # snaps without snap_every
        assert lib.pl_cond_transient(None, 2, 0.1, 1.0, None, None, None, 0, None, None, None, 1e-10, 100, 0, None, None,
                                     p(heat), 0, None, None, None) == _capi.PL_ERR_ARG
        # max_iter = 1: step 1 misses rtol, and the outputs stay as the caller filled them
        pr = np.arange(n, dtype=np.int32)
        fx8 = fixed.astype(np.uint8)
        tb = np.full(n, 90.0)
        probe, heat, snaps = np.full((3, n), -7.0), np.full((3, 4), -7.0), np.full((2, n), -7.0)
        state, iters = np.full(n, -7.0), np.full(3, -7, np.int32)
        rc = lib.pl_cond_transient(dev._h, 2, 0.1, 1.0, p(fx8), p(tb), None, 0, None, None, None, 1e-14, 1, n, p(pr), p(probe),
                                   p(heat), 1, p(snaps), p(state), p(iters))
        assert rc == _capi.PL_ERR_NOCONV and b"step 1 " in lib.pl_last_error()
        for a in (probe, heat, snaps, state, iters):
            assert (a == -7).all()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        heat = np.zeros((3, 4))
        assert lib.pl_set_heat_capacity(ddm._h, 2.0, None, None) == _capi.PL_ERR_STATE
        assert lib.pl_cond_transient(ddm._h, 2, 0.1, 1.0, None, None, None, 0, None, None, None, 1e-10, 100, 0, None, None,
                                     p(heat), 0, None, None, None) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            heat = np.zeros((3, 4))
            assert lib.pl_set_heat_capacity(dev._h, 2.0, None, None) == _capi.PL_ERR_STATE
            assert lib.pl_cond_transient(dev._h, 2, 0.1, 1.0, None, None, None, 0, None, None, None, 1e-10, 100, 0, None, None,
                                         p(heat), 0, None, None, None) == _capi.PL_ERR_STATE


DDM_PRESET = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                           "radii": [0.05], "geom_types": ["BCC"]},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                        "DDM": {"enable_preconditioner": False, "max_iterations": 1000,
                                                "schur_complement_computation": {"type": "exact"}}},
              "boundary_conditions": _preset(("BCC",), (2, 1, 1), [0.05])["boundary_conditions"]}


def test_through_lattice_sim():
    """3 x 2 x 2 BCC, cold Zmin, 1.5 in on Zmax, convection: transient_temperature against conduction_host.transient."""
    L = _lattice(("BCC",), (3, 2, 2), [0.05])
    lat = L.lattice
    with pytest.raises(RuntimeError, match="solve_temperature"):
        L.transient_temperature(0.2, 4, 2.0)
    assert L.temperature_history is None
    T_steady = L.solve_temperature(0.2, {"Surface": ["Zmin"], "Value": 5.0}, {"Surface": ["Zmax"], "Value": 1.5},
                                   convection={"film": 0.05, "ambient": T_INF})
    n_steps, dt = 8, 0.25
    ramp = lambda t: min(t / 1.0, 1.0)                                           # noqa: E731
    out = L.transient_temperature(dt, n_steps, 2.0, theta=0.5, amplitude=ramp, fixed_amplitude=np.ones(n_steps + 1),
                                  snap_every=4, rtol=RTOL)
    assert L.temperature_history is out and np.array_equal(L.temperature_field, T_steady)
    kept = L._device._heat_capacity
    again = L.transient_temperature(dt, n_steps, 2.0, theta=0.5, amplitude=ramp, fixed_amplitude=np.ones(n_steps + 1), rtol=RTOL)
    assert L._device._heat_capacity is kept                                      # the same capacity is not set again
    assert again["probe"].tobytes() == out["probe"].tobytes()                    # (below 64 blocks: one order of every sum)
    c = L.conduction
    g = CH.conductance(lat.node_xyz, lat.beam_conn, lat.beam_radius, 0.2)
    H = CH.convection_diag(lat.beam_conn, lat.n_nodes, CH.film_conductance(lat.node_xyz, lat.beam_conn, lat.beam_radius, 0.05))
    C = CH.heat_capacity(lat.node_xyz, lat.beam_conn, lat.beam_radius, 2.0)
    amp = np.array([ramp(t) for t in dt * np.arange(n_steps + 1)])[:, None]
    ref = CH.transient(lat.beam_conn, lat.n_nodes, g, C, dt, n_steps, 0.5, c["fixed"], c["t_bar"], np.ones(n_steps + 1),
                       c["heat_flow"][None], amp, None, H, T_INF)
    rise = np.abs(ref["T"] - T_INF).max()
    assert rise > 10.0 and out["probe"].shape == ref["T"].shape
    assert np.abs(out["probe"] - ref["T"]).max() <= 1e-7 * rise
    assert np.abs(out["snaps"] - ref["T"][[4, 8]]).max() <= 1e-7 * rise
    for k in range(4):
        assert np.abs(out["heat"][:, k] - ref["heat"][:, k]).max() <= 1e-7 * np.abs(ref["heat"][:, k]).max()
    # per-strut capacities, chosen probes, a scalar start field
    out2 = L.transient_temperature(dt, 2, None, initial=30.0, probes=[3, 1], beam_heat_capacity=np.full(lat.n_beams, 2.0))
    ref2 = CH.transient(lat.beam_conn, lat.n_nodes, g, C, dt, 2, 1.0, c["fixed"], c["t_bar"], None, c["heat_flow"][None],
                        np.ones((3, 1)), np.full(lat.n_nodes, 30.0), H, T_INF)
    assert np.abs(out2["probe"] - ref2["T"][:, [3, 1]]).max() <= 1e-7 * np.abs(ref2["T"] - T_INF).max()
    with pytest.raises(ValueError, match="amplitude"):
        L.transient_temperature(dt, 4, 2.0, amplitude=np.ones(3))
    compat = LatticeSim(_preset(("BCC",), (2, 1, 1), [0.05]), reference_compat=True)
    with pytest.raises(NotImplementedError):
        compat.transient_temperature(0.2, 4, 2.0)
    ddm = LatticeSim(copy.deepcopy(DDM_PRESET), enable_domain_decomposition_solver=True)
    with pytest.raises(NotImplementedError):
        ddm.transient_temperature(0.2, 4, 2.0)
