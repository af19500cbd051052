"""Global linear buckling on the device (pl_geom_spmv_multi / pl_buckling_modes, csrc/pl_geom.h) against its numpy / scipy
restatement (geometric_host.py): the geometric product on every built-in geometry, the column against the Engesser load,
load factors and modes against the dense eigen-solution built from the handle's own K, scaling, the all-tension case, the
error codes, and the way up through LatticeSim."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import geometric_host as GH                      # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

E, NU = 1013.0, 0.3


def _preset(geoms, cells, radii, fixed="Zmin", loaded="Zmax", dof="Z", value=-0.1):
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                         "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                         "radii": list(radii), "geom_types": list(geoms)},
            "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
            "boundary_conditions": {
                "Displacement": {"Fixed": {"Surface": [fixed], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                           "Value": [0, 0, 0, 0, 0, 0]}},
                "Force": {"Load": {"Surface": [loaded], "DOF": [dof], "Value": [value]}}}}


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
    """A displacement field without any symmetry: struts in tension and in compression, no N at zero
    (as tests/test_gpu_buckling.py)."""
    return np.random.default_rng(seed).standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3


def _loads(L):
    f = np.zeros((L.lattice.n_nodes, 6))
    f[:, :3] = np.asarray(L.applied_force)[:, :3]
    return f


def _bsr(dev):
    """the handle's own K as a scipy matrix"""
    dev.assemble_bsr(False)
    rowptr, col, vals = dev.get_bsr()
    A = sp.bsr_matrix((vals, col, rowptr), shape=(6 * dev.n_nodes, 6 * dev.n_nodes)).tocsr()
    A.sum_duplicates()
    return A


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("penalised", [True, False], ids=["pen", "plain"])
@pytest.mark.parametrize("geom", sorted(_BUILTIN))
def test_operator_parity_with_the_restatement(geom, penalised):
    """K_g X on reorder = 0 and 1 handles, n_rhs = 1, 2, 3, 5 (KB = 1, 2, 4 and a padded block), masked and unmasked, within
    1e-12 of the largest magnitude (the bound of the stress and buckling parity tests), and X^T K_g Y = Y^T K_g X."""
    L = LatticeSim(_preset((geom,), (1, 1, 1), [0.05]))
    n = L.lattice.n_nodes
    u = _generic_field(n, 7)
    rng = np.random.default_rng(11)
    X, Y = rng.standard_normal((5, n, 6)), rng.standard_normal((5, n, 6))
    mask = rng.random((n, 6)) < 0.25
    mask[0] = True
    for reorder in (0, 1):
        with _device(L, penalised, reorder=reorder) as dev:
            dev.set_bc(mask)
            dev.assemble()
            for k in (1, 2, 3, 5):
                for masked in (False, True):
                    got = dev.geom_spmv_multi(X[:k], u, masked=masked)
                    ref = dev.geom_spmv_multi_host(X[:k], u, masked=masked, fixed=mask)
                    assert got.shape == ref.shape == (k, n, 6)
                    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
                    assert scale > 0 and err <= 1e-12 * scale, (geom, reorder, k, masked, err / scale)
                    if masked:
                        assert not got[:, mask].any()
            gx, gy = dev.geom_spmv_multi(X, u), dev.geom_spmv_multi(Y, u)
            for j in range(5):
                a, b = float((Y[j] * gx[j]).sum()), float((X[j] * gy[j]).sum())
                assert abs(a - b) <= 1e-12 * float((np.abs(Y[j]) * np.abs(gx[j])).sum()), (geom, reorder, j, a, b)


def test_null_u_is_the_last_solution_and_multiplicity_doubles():
    L = LatticeSim(_preset(("BCC",), (3, 2, 2), [0.05], fixed="Xmin", loaded="Xmax"))
    n = L.lattice.n_nodes
    X = np.random.default_rng(4).standard_normal((3, n, 6))
    with _device(L) as dev, _device(L, beam_mult=np.full(L.lattice.n_beams, 2.0)) as two:
        for d in (dev, two):
            d.set_bc(L.fixed_DOF, None, _loads(L))
            d.assemble()
        with pytest.raises(_capi.PlError) as e:
            dev.geom_spmv_multi(X)                                     # u = NULL without a solve
        assert e.value.code == _capi.PL_ERR_STATE
        u, _ = dev.solve(rtol=1e-10)
        a, b = dev.geom_spmv_multi(X), dev.geom_spmv_multi(X, u)
        assert np.array_equal(a, b) and np.abs(a).max() > 0
        # the same u on records of multiplicity 2: every record carries twice the axial force
        c = two.geom_spmv_multi(X, u)
        assert np.abs(c - 2.0 * b).max() <= 1e-12 * np.abs(c).max()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the column
# ---------------------------------------------------------------------------------------------------------------------
def _column_device(n_struts=8, n_sub=4, pull=False):
    """The pinned-pinned column of tests/test_geometric_host.py: collinear plain struts of length 1 and radius 0.05 along x,
    unit end compression (pull: tension).  Returns (handle, fixed (N, 6), Engesser load)."""
    n, radius = n_struts + 1, 0.05
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.arange(n)
    conn = np.column_stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int32)
    sl = np.zeros((n - 1, 3))
    sl[:, 1] = 1.0
    sn = np.zeros((n - 1, 3), np.int32)
    sn[:, 1] = n_sub
    fixed = np.zeros((n, 6), bool)
    fixed[0, [0, 1, 2, 3]] = True                       # pin: the three displacements, and the twist about the axis
    fixed[-1, [1, 2]] = True                            # roller
    f = np.zeros((n, 6))
    f[-1, 0] = 1.0 if pull else -1.0
    S, I = np.pi * radius ** 2, 0.25 * np.pi * radius ** 4
    n_e = np.pi ** 2 * E * I / float(n_struts) ** 2
    dev = _capi.HipLattice(xyz, conn, np.full(n - 1, radius), sl, sn, E, NU, kappa=0.9)
    dev.set_bc(fixed, None, f)
    dev.assemble()
    return dev, fixed, n_e / (1.0 + n_e / (0.9 * E / (2 * (1 + NU)) * S))


def test_pinned_column_buckles_at_the_engesser_load():
    """8 collinear struts of 4 sub-elements, pinned-pinned, unit end compression: lambda_1 = lambda_2 within 1e-8 and within
    0.5 % of the Engesser load (0.083 % is the offset of the dense solution)."""
    dev, fixed, n_cr = _column_device()
    with dev:
        dev.solve(rtol=1e-12, max_iter=100000)
        out = dev.buckling_modes(2)
        lam = out["load_factor"]
        print(f"\ncolumn: lambda = {lam}, Engesser load {n_cr:.8g}, ratio {lam[0] / n_cr:.6f}, "
              f"{out['outer_iterations']} outer steps, residual {out['residual']}")
        assert out["n_found"] == 2
        assert abs(lam[1] - lam[0]) <= 1e-8 * lam[0]
        assert abs(lam[0] / n_cr - 1.0) <= 5e-3
        assert not out["modes"][:, fixed].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. load factors and modes against the dense solution
# ---------------------------------------------------------------------------------------------------------------------
# n_sub: the host iteration (geometric_host.buckling_modes_subspace, exact solves) was run on every input first and the
# input kept with 8 columns only where it converged within max_outer / 2 = 50 outer steps.  The towers under end compression
# did not (58 steps penalised, 64 plain: their fourth factor sits in a cluster of six, 2.24 ... 2.26, and 8 columns end inside
# it); with 12 columns they take 17 and 16 steps.  8 columns: lateral load 34 and 34 steps, the Octet 20.
ORACLE = [("tower-compression", "BCC", (2, 2, 4), "Z", -0.1, 12), ("tower-lateral", "BCC", (2, 2, 4), "X", 0.1, 8)]
ORACLE_CASES = [c + (pen,) for c in ORACLE for pen in (True, False)] + [("octet-compression", "Octet", (2, 2, 2), "Z", -0.1, 8, True)]


@pytest.mark.parametrize("name,geom,cells,dof,value,n_sub,penalised", ORACLE_CASES,
                         ids=[f"{c[0]}-{'pen' if c[-1] else 'plain'}" for c in ORACLE_CASES])
def test_load_factors_and_modes_against_the_dense_solution(name, geom, cells, dof, value, n_sub, penalised):
    """pl_buckling_modes(n_modes = 4, max_outer = 100) returns PL_OK; the load factors agree with scipy.linalg.eigh on the
    handle's own K (get_bsr) and the restatement's K_g within 1e-6 relative, the residuals recomputed with those matrices
    are <= 1e-4, the modes are K-orthonormal within 1e-8, vanish on the fixed dofs and have their largest component positive."""
    L = LatticeSim(_preset((geom,), cells, [0.05], dof=dof, value=value))
    n = L.lattice.n_nodes
    fixed = np.asarray(L.fixed_DOF).reshape(n, 6) != 0
    with _device(L, penalised) as dev:
        dev.set_bc(fixed, None, _loads(L))
        dev.assemble()
        u, _ = dev.solve(rtol=1e-12, max_iter=100000)
        out = dev.buckling_modes(4, n_sub=n_sub, max_outer=100)          # raises unless PL_OK
        same = dev.buckling_modes(4, u, n_sub=n_sub, max_outer=100)
        # u = NULL is the last solution (the inner PCG sums with atomics: equal to rounding, not to the bit)
        assert same["n_found"] == out["n_found"] and np.abs(same["load_factor"] / out["load_factor"] - 1.0).max() <= 1e-9
        K = _bsr(dev)
        Kg = GH.geometric_matrix(dev.records(), dev.beam_conn, u, n)
        dense = GH.buckling_modes_dense(K, Kg, fixed, 4)
        lam, ref = out["load_factor"], dense["load_factor"]
        V = out["modes"].reshape(4, -1)
        free = ~fixed.reshape(-1)
        res = [np.linalg.norm((K @ v + l * (Kg @ v))[free]) / np.linalg.norm((K @ v)[free]) for v, l in zip(V, lam)]
        gram = V @ (K @ V.T)
        print(f"\n{name}: device {lam}, dense {ref}, relative difference {np.abs(lam / ref - 1).max():.2e}, "
              f"{out['outer_iterations']} outer steps, residuals {np.array(res)} (device's own {out['residual']}), "
              f"orthonormality {np.abs(gram - np.eye(4)).max():.2e}")
        assert out["n_found"] == dense["n_found"] == 4
        assert np.abs(lam / ref - 1.0).max() <= 1e-6
        assert max(res) <= 1e-4
        assert np.abs(out["residual"] - np.array(res)).max() <= 1e-6
        assert np.abs(gram - np.eye(4)).max() <= 1e-8
        assert not V[:, ~free].any()
        assert all(v[np.argmax(np.abs(v))] > 0 for v in V)
        assert np.all(np.diff(lam) >= 0)
        # 5. twice the displacements, twice the axial forces: every load factor halves
        half = dev.buckling_modes(4, 2.0 * u, n_sub=n_sub, max_outer=100)
        assert np.abs(2.0 * half["load_factor"] / lam - 1.0).max() <= 1e-6


def test_a_solve_after_the_modes_is_unchanged():
    """the handle's single-column state is left alone: the last solution is still on the device, and the same pl_solve
    gives what it gave before"""
    L = LatticeSim(_preset(("BCC",), (2, 2, 3), [0.05]))
    with _device(L) as dev:
        dev.set_bc(L.fixed_DOF, None, _loads(L))
        dev.assemble()
        u1, st1 = dev.solve(rtol=1e-12)
        x = np.random.default_rng(6).standard_normal((1, dev.n_nodes, 6))
        before = dev.geom_spmv_multi(x)
        assert dev.buckling_modes(2)["n_found"] == 2
        assert np.array_equal(dev.geom_spmv_multi(x), before)            # u = NULL: still the solution of pl_solve
        assert np.array_equal(before, dev.geom_spmv_multi(x, u1))
        u2, st2 = dev.solve(rtol=1e-12)
        assert np.abs(u2 - u1).max() <= 1e-9 * np.abs(u1).max()


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing to find
# ---------------------------------------------------------------------------------------------------------------------
def test_two_collinear_struts_in_tension_have_no_factor():
    dev, fixed, _ = _column_device(n_struts=2, n_sub=4, pull=True)
    with dev:
        u, _ = dev.solve(rtol=1e-12)
        assert (dev.buckling(u, length=0)["n_axial"] > 0).all()
        out = dev.buckling_modes(2)                                    # PL_OK
        assert out["n_found"] == 0
        assert np.isnan(out["load_factor"]).all() and np.isnan(out["modes"]).all() and np.isnan(out["residual"]).all()
        zero = dev.buckling_modes(2, np.zeros_like(u))                 # u = 0: K_g vanishes
        assert zero["n_found"] == 0 and np.isnan(zero["load_factor"]).all() and zero["outer_iterations"] <= 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. error codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    L = LatticeSim(_preset(("BCC",), (2, 1, 1), [0.05]))
    n = L.lattice.n_nodes
    u = np.ascontiguousarray(_generic_field(n, 1).ravel())
    x = np.ascontiguousarray(np.random.default_rng(2).standard_normal(6 * n))
    y = np.empty_like(x)
    lib, p = _capi.load_library(), _capi._ptr
    lam, res = np.empty(4), np.empty(4)
    found, outer = C.c_int32(), C.c_int32()

    def modes(h, n_modes=2, n_sub=8, lam_=lam, found_=found, outer_=outer):
        return lib.pl_buckling_modes(h, p(u), n_modes, n_sub, 1e-10, 10000, 1e-9, 50, p(lam_), None, p(res),
                                     None if found_ is None else C.byref(found_), None if outer_ is None else C.byref(outer_))

    with _device(L) as dev:
        assert modes(dev._h) == _capi.PL_ERR_STATE                      # before pl_assemble
        assert lib.pl_geom_spmv_multi(dev._h, p(u), 1, 0, p(x), p(y)) == _capi.PL_ERR_STATE
        dev.assemble()
        assert modes(dev._h) == _capi.PL_ERR_STATE                      # before pl_set_bc
        assert b"pl_set_bc" in lib.pl_last_error()
        assert lib.pl_geom_spmv_multi(dev._h, p(u), 1, 1, p(x), p(y)) == _capi.PL_ERR_STATE      # the masked product too
        assert lib.pl_geom_spmv_multi(dev._h, p(u), 1, 0, p(x), p(y)) == _capi.PL_OK
        dev.set_bc(L.fixed_DOF)
        assert lib.pl_buckling_modes(dev._h, None, 2, 8, 1e-10, 10000, 1e-9, 50, p(lam), None, None, C.byref(found),
                                     C.byref(outer)) == _capi.PL_ERR_STATE   # u = NULL without a solve
        assert modes(dev._h, n_modes=5) == _capi.PL_ERR_ARG             # n_modes > n_sub / 2
        assert modes(dev._h, n_sub=6) == _capi.PL_ERR_ARG
        assert modes(dev._h, n_sub=36) == _capi.PL_ERR_ARG
        assert modes(dev._h, n_modes=0) == _capi.PL_ERR_ARG
        assert modes(dev._h, lam_=None) == _capi.PL_ERR_ARG
        assert modes(dev._h, found_=None) == _capi.PL_ERR_ARG
        assert modes(dev._h, outer_=None) == _capi.PL_ERR_ARG
        assert lib.pl_geom_spmv_multi(dev._h, p(u), 0, 0, p(x), p(y)) == _capi.PL_ERR_ARG
        assert lib.pl_geom_spmv_multi(dev._h, p(u), _capi.MULTI_MAX + 1, 0, p(x), p(y)) == _capi.PL_ERR_ARG
        assert lib.pl_geom_spmv_multi(dev._h, p(u), 1, 0, None, p(y)) == _capi.PL_ERR_ARG
        assert modes(dev._h) == _capi.PL_OK and modes(dev._h, n_modes=4, n_sub=0) == _capi.PL_OK   # modes = NULL is fine
        master = np.arange(n, dtype=np.int32)
        master[n - 1] = n - 2
        dev.set_periodic(master)
        assert modes(dev._h) == _capi.PL_ERR_STATE
        assert b"periodic" in lib.pl_last_error()
    S = np.eye(12)[None]
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), S, np.zeros(1, np.int32))
    try:
        u2, x2, y2 = np.zeros(12), np.ones(12), np.empty(12)
        assert lib.pl_geom_spmv_multi(ddm._h, p(u2), 1, 0, p(x2), p(y2)) == _capi.PL_ERR_STATE
        assert lib.pl_buckling_modes(ddm._h, p(u2), 2, 8, 1e-10, 100, 1e-9, 50, p(lam), None, None, C.byref(found),
                                     C.byref(outer)) == _capi.PL_ERR_STATE
    finally:
        ddm.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. LatticeSim
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_sim_global_buckling():
    L = LatticeSim(_preset(("BCC",), (2, 2, 3), [0.05]))
    with pytest.raises(RuntimeError):
        L.global_buckling(2)
    _, model = solve_FEM_FenicsX(L, rtol=1e-12)
    u_before = np.array(model.u)
    out = L.global_buckling(2)
    direct = model.device.buckling_modes(2, model._u_solver)
    assert np.array_equal(out["load_factor"], direct["load_factor"]) and np.array_equal(out["modes"], direct["modes"])
    assert L.buckling_load_factors.shape == (2,) and L.buckling_modes.shape == (2, L.lattice.n_nodes, 6)
    assert out["n_found"] == 2 and np.all(L.buckling_load_factors > 0)
    # the struts' own utilisation says nothing about this failure: the two numbers are printed side by side
    print(f"\nglobal load factors {L.buckling_load_factors}, 1 / max strut utilisation {1.0 / L.max_strut_buckling():.6g}")
    _, again = solve_FEM_FenicsX(L, rtol=1e-12)
    assert np.abs(np.array(again.u) - u_before).max() <= 1e-9 * np.abs(u_before).max()
