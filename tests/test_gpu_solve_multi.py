"""Several right-hand sides in one PCG pass (pl_spmv_multi / pl_solve_multi, csrc/pl_multi.h): the k-column operator against
the CPU oracle and, bit for bit, against the single-column gather kernel; the k-column Jacobi PCG against a dense direct
solve, against k single solves, with columns of very different difficulty (the freeze rule), next to the handle's
single-column state, its error codes, and under the periodic constraints of the homogenisation."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import timoshenko_oracle as O                              # noqa: E402
from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.homogenization_cell import HomogenizedCell       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402

E, NU = 1013.0, 0.3


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def _cantilever(geoms, cells, radii=None):
    radii = radii or [0.05 - 0.01 * i for i in range(len(geoms))]
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                                    "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                                    "radii": radii, "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                       "boundary_conditions": {
                           "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                      "Value": [0, 0, 0, 0, 0, 0]}},
                           "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})


def _device(L, **kw):
    lat, pen = L.lattice, L.penalized
    return _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU, **kw)


def _oracle_K(L):
    lat, pen = L.lattice, L.penalized
    sc = np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(lat.beam_radius, pen.seg_len, pen.seg_nsub)])
    return np.asarray(O.assemble_condensed(lat.node_xyz, lat.beam_conn, sc).todense())


def _direct(K, fixed, ubar, f):
    """np.linalg.solve on the free dofs with the Dirichlet data lifted; the full field."""
    fx = np.asarray(fixed, bool).ravel()
    u = np.where(fx, np.asarray(ubar).ravel(), 0.0)
    b = (np.asarray(f).ravel() - K @ u)[~fx]
    u[~fx] = np.linalg.solve(K[np.ix_(~fx, ~fx)], b)
    return u.reshape(-1, 6)


def _tip_load(L):
    f = np.zeros((L.lattice.n_nodes, 6))
    f[:, :3] = L.applied_force[:, :3]
    return f


def _true_residual(dev, fixed, ubar, f, u):
    """||P (f - K u)|| / ||P (f - K ubar)|| with the single-column operator."""
    free = ~fixed
    lift = np.where(fixed, ubar, 0.0)
    b = (f - dev.spmv(lift))[free]
    r = (f - dev.spmv(u))[free]
    return np.linalg.norm(r) / np.linalg.norm(b)


def _allow(it):
    return max(3, it // 40)


WIDTHS = [1, 2, 3, 4, 5, 8, 13, 64]


@pytest.mark.parametrize("geom", sorted(_BUILTIN))
def test_operator_against_oracle_and_single_column_kernel(geom):
    """every column of spmv_multi within 1e-13 of the oracle's K @ x (plain and masked), on reorder = 0 / 1 handles;
    on a spmv_kernel = 2 handle bitwise equal to spmv(x) and to itself at another position in another block width."""
    L = _cantilever([geom], (3, 2, 2), [0.04])
    K = _oracle_K(L)
    n = L.lattice.n_nodes
    rng = np.random.default_rng(5)
    X = rng.standard_normal((64, n, 6))
    fixed = rng.random((n, 6)) < 0.2
    m = (~fixed).ravel().astype(float)
    ref = (K @ X.reshape(64, -1).T).T
    ref_m = (m[:, None] * (K @ (m[:, None] * X.reshape(64, -1).T))).T
    for reorder in (0, 1):
        with _device(L, reorder=reorder, spmv_kernel=2) as dev:
            dev.assemble()
            dev.set_bc(fixed)
            single = [dev.spmv(X[j]) for j in range(13)]
            single_m = [dev.spmv_free(X[j]) for j in range(5)]
            worst = 0.0
            for k in WIDTHS:
                Y = dev.spmv_multi(X[:k])
                Ym = dev.spmv_multi(X[:k], masked=True)
                assert Y.shape == (k, n, 6)
                for j in range(k):
                    worst = max(worst, _rel(Y[j].ravel(), ref[j]), _rel(Ym[j].ravel(), ref_m[j]))
                    assert _rel(Y[j].ravel(), ref[j]) < 1e-13, (geom, reorder, k, j)
                    assert _rel(Ym[j].ravel(), ref_m[j]) < 1e-13, (geom, reorder, k, j)
                    if j < 13:
                        assert np.array_equal(Y[j], single[j]), (geom, reorder, k, j)
                    if j < 5:
                        assert np.array_equal(Ym[j], single_m[j]), (geom, reorder, k, j)
            # the same vector at another position of another block width
            Z = dev.spmv_multi(np.stack([X[7], X[0], X[3], X[0], X[1], X[0]]))
            assert np.array_equal(Z[1], single[0]) and np.array_equal(Z[3], single[0]) and np.array_equal(Z[5], single[0])
            assert np.array_equal(Z[0], single[7]) and np.array_equal(Z[2], single[3])
            print(geom, "reorder", reorder, "worst relative error against the oracle", worst)
        # a handle with the default kernel choice serves the same call
        with _device(L, reorder=reorder) as dev:
            dev.assemble()
            Y = dev.spmv_multi(X[:5])
            for j in range(5):
                assert _rel(Y[j].ravel(), ref[j]) < 1e-13


def _columns(L, rng):
    """7 columns on the cantilever mask: different loads, one with prescribed support displacements, one all zero."""
    n = L.lattice.n_nodes
    fixed = L.fixed_DOF.copy()
    f = np.zeros((7, n, 6))
    ubar = np.zeros((7, n, 6))
    f[0] = _tip_load(L)
    f[1, :, 1] = 1e-3
    f[2, :, :3] = 1e-3 * rng.standard_normal((n, 3))
    f[3, :, 3:] = 1e-4 * rng.standard_normal((n, 3))
    f[4] = 0.5 * f[0]
    ubar[4][fixed] = 1e-3 * rng.standard_normal(int(fixed.sum()))          # non-zero prescribed displacements
    # column 5: all zero
    f[6, L.lattice.n_nodes // 2, 0] = 0.05
    f[:, fixed] = 0.0
    return fixed, ubar, f


@pytest.mark.parametrize("geoms", [["BCC"], ["Octet"], ["BCC", "Hybrid1", "Hybrid4"]], ids=lambda g: "+".join(g))
def test_columns_against_a_direct_solve(geoms):
    """7 columns at rtol 1e-12 within 1e-7 of np.linalg.solve on the oracle's K; the zero column is its lifting."""
    L = _cantilever(geoms, (4, 3, 3))
    K = _oracle_K(L)
    fixed, ubar, f = _columns(L, np.random.default_rng(2))
    with _device(L) as dev:
        dev.set_bc(fixed)
        dev.assemble()
        U, stats = dev.solve_multi(ubar, f, rtol=1e-12, max_iter=100000)
    for j in range(7):
        if j == 5:
            assert np.array_equal(U[j], np.zeros_like(U[j]))
            assert stats[j]["iterations"] == 0 and stats[j]["converged"] == 1
            continue
        ref = _direct(K, fixed, ubar[j], f[j])
        print("+".join(geoms), "column", j, "iterations", stats[j]["iterations"], "error", _rel(U[j], ref))
        assert stats[j]["converged"] == 1
        assert _rel(U[j], ref) < 1e-7
    # a zero column with prescribed values returns exactly its lifting
    with _device(L) as dev:
        dev.set_bc(np.ones_like(fixed))
        dev.assemble()
        ub = np.random.default_rng(3).standard_normal((2,) + fixed.shape)
        U, stats = dev.solve_multi(ub, None, rtol=1e-12)
        assert np.array_equal(U, ub) and all(s["iterations"] == 0 and s["converged"] == 1 for s in stats)


def test_same_answer_as_single_solves():
    """every column against set_bc + solve on a precond = 1 handle at rtol 1e-8: true residual (single-column
    operator) below 5e-8, iteration counts within max(3, iterations // 40)."""
    L = _cantilever(["BCC", "Hybrid1", "Hybrid4"], (4, 3, 3))
    fixed, ubar, f = _columns(L, np.random.default_rng(4))
    with _device(L, precond=1) as dev:
        dev.set_bc(fixed)
        dev.assemble()
        U, stats = dev.solve_multi(ubar, f, rtol=1e-8)
        for j in range(7):
            if j == 5:
                continue
            res = _true_residual(dev, fixed, ubar[j], f[j], U[j])
            dev.set_bc(fixed, ubar[j], f[j])
            u1, st1 = dev.solve(rtol=1e-8)
            print("column", j, "true residual", res, "iterations multi / single", stats[j]["iterations"], st1["iterations"],
                  "difference", _rel(U[j], u1))
            assert res < 5e-8
            assert abs(stats[j]["iterations"] - st1["iterations"]) <= _allow(st1["iterations"])


def test_columns_of_different_difficulty_freeze_independently():
    """a unit load next to the support, a smooth tip load and that load scaled by 1e-100 / 1e+100 in one call.
    rtol = 1e-13: two converged columns agree to about cond * rtol (their dot products are summed in a run-dependent order
    and 1e+-100 is no power of two, so they are different CG runs), hence a comparison at 1e-12 needs a tolerance below it;
    at rtol = 1e-8 the scaled columns were measured 1e-11 apart."""
    L = _cantilever(["BCC"], (3, 2, 2))
    n = L.lattice.n_nodes
    fixed = L.fixed_DOF.copy()
    xyz = L.lattice.node_xyz
    near = int(np.argmin(np.where(fixed.any(axis=1), np.inf, xyz[:, 0])))
    f = np.zeros((4, n, 6))
    f[0, near, 2] = 1.0
    f[1] = _tip_load(L)
    f[2] = 1e-100 * f[1]
    f[3] = 1e+100 * f[1]
    rtol = 1e-13
    with _device(L, precond=1) as dev:
        dev.set_bc(fixed)
        dev.assemble()
        U, stats = dev.solve_multi(None, f, rtol=rtol)
        assert np.isfinite(U).all()
        its = [s["iterations"] for s in stats]
        print("iterations", its, "relative residuals", [s["rel_residual"] for s in stats])
        assert all(s["converged"] == 1 for s in stats) and len(set(its)) > 1
        for j, fac in ((2, 1e-100), (3, 1e+100)):
            err = _rel(U[j] / fac, U[1])
            print("column scaled by", fac, "against the unscaled one", err)
            assert err < 1e-12
        zero = np.zeros((n, 6))
        for j in range(4):
            alone, st = dev.solve_multi(None, f[j:j + 1], rtol=rtol)
            ra, rb = _true_residual(dev, fixed, zero, f[j], alone[0]), _true_residual(dev, fixed, zero, f[j], U[j])
            print("column", j, "alone / in the block: residuals", ra, rb, "difference", _rel(alone[0], U[j]))
            assert ra < 5e-8 and rb < 5e-8
            assert _rel(alone[0], U[j]) < 1e-7


def test_single_column_state_of_the_handle_is_untouched():
    """solve() -> solve_multi() -> solve() on a precond = 3, warm_start = 4 handle equals solve() -> solve()."""
    L = _cantilever(["BCC"], (6, 4, 4))
    fixed = L.fixed_DOF.copy()
    f = _tip_load(L)
    fm = np.stack([2.0 * f, np.roll(f, 1, axis=1)])
    fm[:, fixed] = 0.0
    out = {}
    for with_multi in (False, True):
        with _device(L, precond=3, warm_start=4) as dev:
            dev.set_bc(fixed, None, f)
            dev.assemble()
            u0, st0 = dev.solve(rtol=1e-10)
            s0 = dev.sens(None)
            if with_multi:
                Um, stm = dev.solve_multi(None, fm, rtol=1e-10)
                assert all(s["converged"] == 1 for s in stm)
                assert _rel(Um[0], 2.0 * u0) < 1e-7
                assert dev.last_stats["iterations"] == st0["iterations"]
                s1 = dev.sens(None)                  # still the single solve's field
                assert np.array_equal(s0, s1)
            dev.set_bc(fixed, None, 1.01 * f)
            u1, st1 = dev.solve(rtol=1e-10)
            out[with_multi] = (u1, st1["iterations"], st1["precond_used"])
    print("second solve: iterations without / with the multi call", out[False][1], out[True][1])
    assert out[True][2] == out[False][2] == 3
    assert abs(out[True][1] - out[False][1]) <= _allow(out[False][1])
    assert _rel(out[True][0], out[False][0]) < 1e-7


def test_error_codes():
    """Argument, state and convergence errors of the three entry points."""
    L = _cantilever(["BCC"], (4, 3, 3), [0.02])
    n = L.lattice.n_nodes
    lib = _capi.load_library()
    fixed = L.fixed_DOF.copy()
    f = np.ascontiguousarray(np.broadcast_to(_tip_load(L), (2, n, 6)))
    u = np.empty((_capi.MULTI_MAX + 1, 6 * n))
    big = np.zeros((_capi.MULTI_MAX + 1, 6 * n))

    def call(dev, k, u_arr=u, stats=None):
        return lib.pl_solve_multi(dev._h, k, None, _capi._ptr(big), 1e-8, 1000, _capi._ptr(u_arr), stats)

    with _device(L, precond=1) as dev:
        with pytest.raises(_capi.PlError) as e:
            dev.solve_multi(None, f)
        assert e.value.code == _capi.PL_ERR_STATE                            # before pl_assemble
        dev.assemble()
        assert call(dev, 2) == _capi.PL_ERR_STATE                            # before pl_set_bc
        assert lib.pl_spmv_multi(dev._h, 2, 1, _capi._ptr(big), _capi._ptr(u)) == _capi.PL_ERR_STATE
        dev.set_bc(fixed)
        assert call(dev, 0) == _capi.PL_ERR_ARG
        assert call(dev, _capi.MULTI_MAX + 1) == _capi.PL_ERR_ARG
        assert call(dev, 2, None) == _capi.PL_ERR_ARG
        assert lib.pl_spmv_multi(dev._h, 0, 0, _capi._ptr(big), _capi._ptr(u)) == _capi.PL_ERR_ARG
        assert lib.pl_spmv_multi(dev._h, _capi.MULTI_MAX + 1, 0, _capi._ptr(big), _capi._ptr(u)) == _capi.PL_ERR_ARG
        st = (_capi.PlStats * 2)()
        st[0].struct_size = C.sizeof(_capi.PlStats)
        st[1].struct_size = C.sizeof(_capi.PlStats) - 8
        assert call(dev, 2, u, st) == _capi.PL_ERR_ARG
        with pytest.raises(ValueError):
            dev.solve_multi(None, np.zeros((2, n, 5)))
        with pytest.raises(ValueError):
            dev.spmv_multi(np.zeros((_capi.MULTI_MAX + 1, n, 6)))
        # max_iter = 1 on a hard problem: PL_ERR_NOCONV, the zero column still converged, everything finite
        f3 = np.concatenate([f, np.zeros((1, n, 6))])
        U, stats = dev.solve_multi(None, f3, rtol=1e-10, max_iter=1, raise_on_noconv=False)
        assert [s["converged"] for s in stats] == [0, 0, 1] and np.isfinite(U).all()
        assert all(np.isfinite(s["rel_residual"]) for s in stats)
        with pytest.raises(_capi.PlError) as e:
            dev.solve_multi(None, f3, rtol=1e-10, max_iter=1)
        assert e.value.code == _capi.PL_ERR_NOCONV
    # a DDM handle
    S = np.eye(12)
    with _capi.HipLattice.ddm(2, np.array([[0, 1]]), S, np.array([0])) as ddm:
        x = np.zeros((2, 12))
        assert lib.pl_spmv_multi(ddm._h, 2, 0, _capi._ptr(x), _capi._ptr(x.copy())) == _capi.PL_ERR_STATE
        assert b"DDM" in lib.pl_last_error()
        assert lib.pl_solve_multi(ddm._h, 2, None, _capi._ptr(x), 1e-8, 10, _capi._ptr(x.copy()), None) == _capi.PL_ERR_STATE
        bn = np.array([0], np.int32)
        assert lib.pl_schur_block(ddm._h, _capi._ptr(bn), 1, 1e-8, 10, 0, _capi._ptr(np.zeros((6, 6)))) == _capi.PL_ERR_STATE
    # a loopback multi-rank handle
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            x = np.zeros((2, 6 * dev.n_nodes))
            assert lib.pl_spmv_multi(dev._h, 2, 0, _capi._ptr(x), _capi._ptr(x.copy())) == _capi.PL_ERR_STATE
            assert b"multi-rank" in lib.pl_last_error()
            assert lib.pl_solve_multi(dev._h, 2, None, _capi._ptr(x), 1e-8, 10, _capi._ptr(x.copy()), None) == _capi.PL_ERR_STATE


class _Counting:
    """Forwards to a HipLattice and counts the solver calls that reach it."""

    def __init__(self, dev):
        self._dev = dev
        self.calls = {"solve": 0, "solve_multi": 0, "spmv": 0, "spmv_multi": 0}

    def __getattr__(self, name):
        attr = getattr(self._dev, name)
        if name in self.calls:
            def counted(*a, **kw):
                self.calls[name] += 1
                return attr(*a, **kw)
            return counted
        return attr


@pytest.mark.parametrize("geom,penalised", [("BCC", True), ("Hybrid1", False), ("Hybrid4", False)])
def test_batched_homogenisation(golden_dir, geom, penalised):
    """HomogenizedCell(batched=True) against tests/golden/homogenized_from_schur.npz at 2e-8, its six fields against
    batched=False at 1e-8; one solve_multi and no solve reaches the handle."""
    fx = np.load(os.path.join(golden_dir, "homogenized_from_schur.npz"))
    for r, Cref in zip(fx[f"{geom}_radius"], fx[f"{geom}_C"]):
        preset = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                               "radii": [float(r)], "geom_types": [geom]},
                  "simulation_parameters": {"enable": penalised, "material": "VeroClear", "periodicity": True}}
        res = {}
        for batched in (True, False):
            L = LatticeSim(preset)
            dev = _Counting(L.device_model(precond=1))
            a = HomogenizedCell(L, device=dev, batched=batched)
            a.prepare_simulation()
            a.apply_dirichlet_for_homogenization()
            a.periodic_boundary_condition()
            res[batched] = (a.solve_full_homogenization(), a.saveDataToExport, dict(dev.calls), list(a.pcg_iterations))
            L._device.close()
        H, fields, calls, its = res[True]
        print(geom, r, "against the golden", np.linalg.norm(H - Cref) / np.linalg.norm(Cref), "iterations", its, res[False][3])
        assert calls["solve_multi"] == 1 and calls["solve"] == 0 and calls["spmv_multi"] == 2 and calls["spmv"] == 0
        assert res[False][2]["solve_multi"] == 0 and res[False][2]["solve"] == 6
        assert len(its) == 6 and max(its) > 0
        assert np.linalg.norm(H - Cref) < 2e-8 * np.linalg.norm(Cref), (geom, r)
        for ub, us in zip(fields, res[False][1]):
            assert np.linalg.norm(ub - us) < 1e-8 * np.linalg.norm(us)
