"""Steady heat conduction on the strut graph on the device (pl_set_conduction / pl_cond_spmv / pl_cond_solve / pl_cond_flux /
pl_cond_sens / pl_thermal_load_adjoint, csrc/pl_conduction.h) against the numpy restatement (conduction_host.py): parity of the
products, strut multiplicity, the solved temperatures against a dense host solve, bitwise reproducibility, the untouched
mechanical path, the way up through LatticeSim and LatticeOpti with the thermo-elastic chain term, and the error codes."""
import copy

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import conduction_host as CH                     # noqa: E402
from pylatticedso_amd import geometric_host as GH                      # noqa: E402
from pylatticedso_amd import thermal_host as TH                        # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

E, NU = 1013.0, 0.3
ALL6 = ["X", "Y", "Z", "RX", "RY", "RZ"]


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


def _field6(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3


def _inputs(dev, seed):
    """Random conductivities per strut, a random mask with prescribed temperatures, and two random nodal fields."""
    rng = np.random.default_rng(seed)
    kap = 0.1 + 0.3 * rng.random(dev.n_beams)
    fixed = rng.random(dev.n_nodes) < 0.3
    fixed[rng.integers(dev.n_nodes)] = True
    t_bar = 20.0 + 60.0 * rng.random(dev.n_nodes)
    return kap, fixed, t_bar, 20.0 + 60.0 * rng.random(dev.n_nodes), rng.standard_normal(dev.n_nodes)


def _close(got, ref, tol, what):
    """|got - ref| <= tol x the largest magnitude of ref."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    assert err <= tol * scale, (what, err / scale if scale else err)


def _compare(dev, T, mu, lam, fixed):
    """The products against the restatement: values within 1e-12 of the largest magnitude, cond_sens within 1e-10 (the bounds
    of tests/test_gpu_stress.py)."""
    _close(dev.cond_spmv(T), dev.cond_spmv_host(T), 1e-12, "K_T x")
    _close(dev.cond_spmv(T, fixed), dev.cond_spmv_host(T, fixed), 1e-12, "P K_T P x")
    assert not dev.cond_spmv(T, fixed)[fixed].any()
    _close(dev.cond_flux(T), dev.cond_flux_host(T), 1e-12, "Q")
    _close(dev.cond_sens(T, mu), dev.cond_sens_host(T, mu), 1e-10, "cond_sens")
    _close(dev.thermal_load_adjoint(lam), dev.thermal_load_adjoint_host(lam), 1e-12, "thermal_load_adjoint")


CASES = [("BCC",), ("Octet",), ("BCC", "Hybrid1"), ("Octet", "Hybrid4")]


@pytest.mark.parametrize("geoms", CASES, ids=lambda v: "+".join(v))
def test_parity_with_the_restatement(geoms):
    """1 x 1 x 1 cells, reorder 0 and 1 (node and strut permutations), 1, 4 and 16 lanes per node, random conductivities per
    strut, a random mask."""
    L = _lattice(geoms, (1, 1, 1))
    lam = _field6(L.lattice.n_nodes, 17)
    for reorder, lpn in ((0, 4), (1, 1), (1, 4), (1, 16)):
        with _device(L, reorder=reorder, lanes_per_node=lpn) as dev:
            dev.assemble()
            kap, fixed, t_bar, T, mu = _inputs(dev, 3)
            dev.set_conduction(0.0, kap)
            alpha = (2.0 + 5.0 * np.random.default_rng(4).random(dev.n_beams)) * 1e-5
            dev.set_thermal(0.0, np.zeros(dev.n_nodes), alpha)
            _compare(dev, T, mu, lam, fixed)
            # the transpose property on the device: c . dT = lam . f_th(dT)
            dev.set_thermal(0.0, T, alpha)
            f = dev.thermal_load()[0]
            c = dev.thermal_load_adjoint(lam)
            assert abs(c @ T - (lam * f).sum()) <= 1e-11 * np.abs(lam * f).sum()
    with _device(L) as dev:                                             # one conductivity for every strut
        dev.assemble()
        dev.set_conduction(0.37)
        _close(dev.cond_spmv(T), dev.cond_spmv_host(T), 1e-12, "scalar kappa")


@pytest.mark.parametrize("reorder", [0, 1])
def test_strut_multiplicity_and_new_radii(reorder):
    """2 x 2 x 1 Octet with multiplicities 1 and 2: k copies conduct k times, Q is that of one copy; then the conductances
    follow update_radii + assemble without another set_conduction."""
    L = _lattice(("Octet",), (2, 2, 1), [0.04])
    rng = np.random.default_rng(3)
    mult = rng.integers(1, 3, L.lattice.n_beams).astype(float)
    assert (mult == 1).any() and (mult == 2).any()
    lam = _field6(L.lattice.n_nodes, 18)
    with _device(L, reorder=reorder, beam_mult=mult) as dev, _device(L, reorder=reorder) as one:
        kap, fixed, t_bar, T, mu = _inputs(dev, 5)
        for d in (dev, one):
            d.assemble()
            d.set_conduction(0.0, kap)
            d.set_thermal(7e-5, np.zeros(d.n_nodes))
        _compare(dev, T, mu, lam, fixed)
        g1 = CH.conductance(one.node_xyz, one.beam_conn, one._radius, kap)
        _close(dev.cond_spmv(T), CH.spmv(one.beam_conn, one.n_nodes, mult * g1, T), 1e-12, "k copies conduct k times")
        _close(dev.cond_flux(T), one.cond_flux(T), 1e-12, "Q of one copy")
        rad = L.lattice.beam_radius * (0.8 + 0.4 * rng.random(dev.n_beams))
        dev.update_radii(rad)
        with pytest.raises(_capi.PlError) as e:
            dev.cond_spmv(T)
        assert e.value.code == _capi.PL_ERR_STATE                         # not assembled
        dev.assemble()
        _compare(dev, T, mu, lam, fixed)
        _close(dev.cond_spmv(T), CH.spmv(one.beam_conn, one.n_nodes, mult * g1 * (rad / one._radius) ** 2, T), 1e-12, "g ~ r^2")


def _faces(L, dev, inflow):
    """Temperature problem on a lattice: hot Zmin and cold Zmax (inflow False), or cold Zmin and a total inflow on Zmax."""
    lo, hi = L.find_point_on_lattice_surface(["Zmin"]), L.find_point_on_lattice_surface(["Zmax"])
    fixed = np.zeros(dev.n_nodes, bool)
    t_bar = np.random.default_rng(1).random(dev.n_nodes)                # (values on free nodes must not matter)
    q = None
    fixed[lo] = True
    if inflow:
        t_bar[lo] = 20.0
        q = np.zeros(dev.n_nodes)
        q[hi] = 1.5 / len(hi)
    else:
        fixed[hi] = True
        t_bar[lo], t_bar[hi] = 90.0, 20.0 + 5.0 * np.random.default_rng(2).random(len(hi))
    return fixed, t_bar, q


@pytest.mark.parametrize("inflow", [False, True], ids=["two-faces", "face+inflow"])
def test_solved_temperatures_against_the_dense_host_solve(inflow):
    """2 x 2 x 2 BCC, rtol 1e-12: relative L2 error below 1e-7, the bound tests/test_gpu_parity.py asks of solved fields."""
    L = _lattice(("BCC",), (2, 2, 2))
    with _device(L) as dev:
        dev.assemble()
        kap = 0.1 + 0.3 * np.random.default_rng(6).random(dev.n_beams)
        dev.set_conduction(0.0, kap)
        fixed, t_bar, q = _faces(L, dev, inflow)
        T, st = dev.cond_solve(fixed, t_bar, q, rtol=1e-12, max_iter=10000)
        ref = dev.cond_solve_host(fixed, t_bar, q)
        err = np.linalg.norm(T - ref) / np.linalg.norm(ref)
        print(f"\nsolved temperatures against the dense host solve: relative L2 error {err:.2e}, "
              f"{st['iterations']} iterations, rel_residual {st['rel_residual']:.2e}")
        assert err < 1e-7
        assert st["converged"] == 1 and 0 < st["iterations"] <= 10000 and st["rel_residual"] <= 1e-12
        assert T[fixed].tobytes() == t_bar[fixed].tobytes()
        assert ref.max() > ref.min() + 10.0                               # (a field, not a constant)
        # the residual the statistics speak of, formed anew: P (q - K_T T)
        r = np.where(fixed, 0.0, (0.0 if q is None else q) - dev.cond_spmv(T))
        b = np.where(fixed, 0.0, (0.0 if q is None else q) - dev.cond_spmv(np.where(fixed, t_bar, 0.0)))
        assert np.linalg.norm(r) <= 1e-10 * np.linalg.norm(b)


def test_bitwise_reproducible_over_many_blocks():
    """6 x 6 x 6 Octet: the per-node and per-strut products return the same bytes; cond_solve is not claimed to (its scalar
    products are summed with atomics)."""
    L = _lattice(("Octet",), (6, 6, 6), [0.03])
    assert L.lattice.n_beams > 5000 and L.lattice.n_nodes > 4 * 256
    lam = _field6(L.lattice.n_nodes, 19)
    with _device(L) as dev:
        dev.assemble()
        kap, fixed, t_bar, T, mu = _inputs(dev, 6)
        dev.set_conduction(0.0, kap)
        dev.set_thermal(7e-5, np.zeros(dev.n_nodes))
        for call in (lambda: dev.cond_spmv(T), lambda: dev.cond_spmv(T, fixed), lambda: dev.cond_flux(T),
                     lambda: dev.cond_sens(T, mu), lambda: dev.thermal_load_adjoint(lam)):
            assert call().tobytes() == call().tobytes()
        _compare(dev, T, mu, lam, fixed)


def test_nothing_else_moves():
    """With a conduction state set (and used), spmv, thermal_load, stress and a solve_FEM_FenicsX displacement are byte-equal to
    those of the same handle without it.  The handle runs the per-node gather K*p and the Jacobi preconditioner: every sum of
    that solve has a fixed order on a lattice of one block, so two solves of one handle can be compared byte by byte at all."""
    L = _lattice(("BCC", "Hybrid1"), (2, 1, 1))
    L.set_temperature(lambda x: 30.0 + 20.0 * x[:, 2], 7e-5)
    L.device_model(precond=1, spmv_kernel=2)
    u = _field6(L.lattice.n_nodes, 5)
    names = ["u", "spmv", "f_th", "n_free", "N", "V", "T", "Mb", "sigma_vm", "peak"]

    def outputs():
        _, model = solve_FEM_FenicsX(L)
        dev = model.device
        s = dev.stress(u)
        return [model.u.copy(), dev.spmv(u), dev.thermal_load()[0], dev.thermal_load()[1]] + \
            [s[k] for k in ("N", "V", "T", "Mb", "sigma_vm", "peak")]

    outputs()                                                           # (every compared solve is a repeated one)
    before = outputs()
    dev = L._device
    dev.set_conduction(0.2)
    fixed = np.zeros(dev.n_nodes, bool)
    fixed[:3] = True
    dev.cond_solve(fixed, np.full(dev.n_nodes, 50.0), np.where(fixed, 0.0, 0.01))
    dev.cond_flux(np.arange(dev.n_nodes, dtype=float))
    dev.thermal_load_adjoint(u)
    with_state = outputs()
    dev.clear_conduction()
    after = outputs()
    for name, a, b, c in zip(names, before, with_state, after):
        print(f"\n{name}: with the state {np.nanmax(np.abs(a - b)):.3e}, after clearing {np.nanmax(np.abs(a - c)):.3e} off")
    for name, a, b, c in zip(names, before, with_state, after):
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
    dev.close()


CONDUCTION = {"conductivity": 0.2, "reference": 20.0, "Temperature": {"Cold": {"Surface": ["Zmin"], "Value": 20.0}},
              "HeatFlow": {"Top": {"Surface": ["Zmax"], "Value": 1.5}}}


def test_through_lattice_sim():
    """A preset with a "conduction" block: solve_temperature equals the cond_solve of the hand-built handle (both PCG solves
    stop at rtol 1e-12 on a Laplacian whose condition is of the order 1e2: 1e-9 of the field), and the mechanical solve under
    delta_T = "conduction" matches the dense host solve of K u = f_ext + f_th(T) to 1e-7."""
    p = _preset(("BCC",), (2, 2, 2), [0.05])
    alpha = 7e-5
    p["simulation_parameters"]["thermal"] = {"alpha": alpha, "conduction": copy.deepcopy(CONDUCTION)}
    L = LatticeSim(p)
    assert L.conduction is not None and L.conduction_driven
    T = L.solve_temperature()
    with _device(_lattice(("BCC",), (2, 2, 2))) as dev:
        dev.assemble()
        dev.set_conduction(0.2)
        fixed, t_bar, q = _faces(L, dev, True)
        T_hand, _ = dev.cond_solve(fixed, t_bar, q, rtol=1e-12)
        ref_T = dev.cond_solve_host(fixed, t_bar, q)
    assert np.linalg.norm(T - T_hand) <= 1e-9 * np.linalg.norm(T_hand)
    assert np.linalg.norm(T - ref_T) < 1e-7 * np.linalg.norm(ref_T)
    Q = L.strut_heat_flow()
    _close(Q, CH.flux(L.lattice.beam_conn, CH.conductance(L.lattice.node_xyz, L.lattice.beam_conn, L.lattice.beam_radius, 0.2),
                      ref_T), 1e-7, "strut_heat_flow")
    _, model = solve_FEM_FenicsX(L)
    dev = model.device
    rec = dev.records()
    f_h = TH.thermal_load(rec, dev.beam_conn, dev.n_nodes, TH.elongation(dev.node_xyz, dev.beam_conn, alpha, ref_T - 20.0))[0]
    K = GH.elastic_matrix(rec, dev.beam_conn, dev.n_nodes).toarray()
    free = np.flatnonzero(~np.asarray(L.fixed_DOF, bool).ravel())
    f = np.zeros((dev.n_nodes, 6))
    f[:, :3] = L.applied_force[:, :3]
    ref = np.zeros(6 * dev.n_nodes)
    ref[free] = scipy.linalg.solve(K[np.ix_(free, free)], (f + f_h).ravel()[free], assume_a="pos")
    err = np.linalg.norm(model.u.ravel() - ref) / np.linalg.norm(ref)
    plain = np.zeros(6 * dev.n_nodes)
    plain[free] = scipy.linalg.solve(K[np.ix_(free, free)], f.ravel()[free], assume_a="pos")
    print(f"\nmechanical solve under the conduction temperature against the dense host solve: relative L2 error {err:.2e}")
    assert err < 1e-7
    assert np.linalg.norm(ref - plain) > 1e-3 * np.linalg.norm(ref)         # (the temperature does load the lattice)
    # new radii: the temperature is solved again before the mechanical solve
    L._device.update_radii(0.8 * L.lattice.beam_radius)
    solve_FEM_FenicsX(L)
    free_T = ~L.conduction["fixed"]
    hot = (L.temperature_field[free_T] - 20.0) / (ref_T[free_T] - 20.0)
    assert np.abs(hot - 1.0 / 0.64).max() <= 1e-7                  # T - T_cold ~ 1 / r^2 under a given inflow
    # given as arrays, the same problem
    L2 = _lattice(("BCC",), (2, 2, 2))
    t = np.full(L2.lattice.n_nodes, np.nan)
    t[fixed] = 20.0
    T2 = L2.solve_temperature(0.2, t, q, reference=20.0)
    assert np.linalg.norm(T2 - ref_T) < 1e-7 * np.linalg.norm(ref_T)
    L2.set_temperature("conduction", alpha)
    assert L2.conduction_driven
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
    "objective_function": "min", "objective_type": "compliance", "max_iterations": 5,
    "optimization_parameters": {"type": "unit_cell"},
    "constraints": {"relative_density": {"value": 0.05}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}


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


@pytest.mark.parametrize("objective", ["compliance", "displacement"])
def test_objective_gradient_under_a_conduction_driven_temperature(objective):
    """Central differences of the objective, step 1e-4 and the 2e-3 bound, at the three variables tests/test_gpu_thermal.py
    checks.  With the chain term switched off - the temperature taken as fixed - at least one of them misses the bound."""
    opt = {} if objective == "compliance" else dict(objective_type="displacement", objective_function="max",
                                                    objective_data={"Surface": ["Xmax"], "DOF": ["Z"]})
    L = LatticeOpti(_opti(**opt))
    assert L.conduction_driven
    theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
    idxs = [0, 5, 11]
    L.objective(theta)
    g = np.asarray(L.gradient(theta))
    fds = {i: _fd(L.objective, theta, i) for i in idxs}
    L.objective(theta)
    L.conduction_chain = False
    wrong = np.asarray(L.gradient(theta))
    L.conduction_chain = True
    for i in idxs:
        print(f"\n{objective} variable {i}: gradient {g[i]:.8e}, difference quotient {fds[i]:.8e}, "
              f"without the chain term {wrong[i]:.8e}")
    for i in idxs:
        assert abs(g[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(g).max()), (objective, i, g[i], fds[i])
    assert any(not abs(wrong[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(wrong).max()) for i in idxs), (wrong, fds)
    L._device.close()


@pytest.mark.parametrize("key,settings", [("buckling", {"value": 1.0}), ("max_stress", {"value": 1.0, "p": 8, "where": 1})])
def test_stress_and_buckling_constraints_refuse(key, settings):
    L = LatticeOpti(_opti(constraints={key: settings}))
    theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
    value, grad = ((L.buckling_constraint, L.buckling_constraint_gradient) if key == "buckling" else
                   (L.stress_constraint, L.stress_constraint_gradient))
    for fn in (value, grad):
        with pytest.raises(ValueError, match="conduction-driven"):
            fn(theta)


# ---------------------------------------------------------------------------------------------------------------------
# error codes
# ---------------------------------------------------------------------------------------------------------------------
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
        x, lam = np.arange(n, dtype=float), _field6(n, 1)
        fixed = np.zeros(n, bool)
        fixed[0] = True
        calls = [(dev.cond_spmv, x), (dev.cond_solve, fixed), (dev.cond_flux, x), (dev.cond_sens, x, x),
                 (dev.thermal_load_adjoint, lam)]
        dev.assemble()
        for c in calls:                                                   # before pl_set_conduction
            assert code(*c) == _capi.PL_ERR_STATE
            assert b"pl_set_conduction" in lib.pl_last_error()
        for bad in (0.0, -1.0, np.nan, np.inf):
            if bad != 0.0:
                assert code(dev.set_conduction, bad) == _capi.PL_ERR_ARG
            bk = np.full(nb, 0.2)
            bk[nb // 2] = bad
            assert code(dev.set_conduction, 0.2, bk) == _capi.PL_ERR_ARG
        assert dev._conduction is None
        dev.update_radii(dev._radius)                                     # clears the assembly
        dev.set_conduction(0.2)
        for c in calls:                                                   # before pl_assemble
            assert code(*c) == _capi.PL_ERR_STATE
            assert b"pl_assemble" in lib.pl_last_error()
        dev.assemble()                                                    # the state survived
        assert code(dev.thermal_load_adjoint, lam) == _capi.PL_ERR_STATE  # no thermal state: no alpha
        assert b"pl_set_thermal" in lib.pl_last_error()
        dev.set_thermal(7e-5, np.zeros(n))
        assert dev.thermal_load_adjoint(lam).shape == (n,)
        assert code(dev.cond_solve, np.zeros(n, bool)) == _capi.PL_ERR_ARG        # a mask that fixes nothing
        y, fx = np.empty(n), np.ascontiguousarray(fixed, dtype=np.uint8)
        yb = np.empty(nb)
        assert lib.pl_cond_spmv(dev._h, 0, None, None, p(y)) == _capi.PL_ERR_ARG
        assert lib.pl_cond_spmv(dev._h, 0, None, p(x), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_spmv(dev._h, 1, None, p(x), p(y)) == _capi.PL_ERR_ARG  # masked without a mask
        assert lib.pl_cond_spmv(dev._h, 0, None, p(x), p(y)) == _capi.PL_OK
        assert lib.pl_cond_solve(dev._h, None, None, None, 1e-8, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve(dev._h, p(fx), None, None, 1e-8, 100, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve(dev._h, p(fx), None, None, 0.0, 100, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve(dev._h, p(fx), None, None, 1e-8, 0, p(y), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_solve(dev._h, p(fx), None, None, 1e-8, 100, p(y), None) == _capi.PL_OK and not y.any()
        assert lib.pl_cond_flux(dev._h, None, p(yb)) == _capi.PL_ERR_ARG
        assert lib.pl_cond_flux(dev._h, p(x), None) == _capi.PL_ERR_ARG
        assert lib.pl_cond_sens(dev._h, p(x), None, p(yb)) == _capi.PL_ERR_ARG
        assert lib.pl_cond_sens(dev._h, p(x), p(x), None) == _capi.PL_ERR_ARG
        assert lib.pl_thermal_load_adjoint(dev._h, None, p(y)) == _capi.PL_ERR_ARG
        # max_iter = 1: PL_ERR_NOCONV, the outputs still written
        q = np.where(fixed, 0.0, 0.01 * (1.0 + np.arange(n) % 3))
        assert code(dev.cond_solve, fixed, np.full(n, 30.0), q, rtol=1e-12, max_iter=1) == _capi.PL_ERR_NOCONV
        T, st = dev.cond_solve(fixed, np.full(n, 30.0), q, rtol=1e-12, max_iter=1, raise_on_noconv=False)
        assert st["converged"] == 0 and st["iterations"] == 1 and st["rel_residual"] > 1e-12
        assert T[0] == 30.0 and np.isfinite(T).all() and np.abs(T[1:]).max() > 0
        dev.clear_conduction()
        assert code(dev.cond_spmv, x) == _capi.PL_ERR_STATE
    # DDM handle
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        two, six, one = np.zeros(2), np.zeros(12), np.ones(2, np.uint8)
        assert lib.pl_set_conduction(ddm._h, 0.2, None) == _capi.PL_ERR_STATE
        assert lib.pl_cond_spmv(ddm._h, 0, None, p(two), p(two)) == _capi.PL_ERR_STATE
        assert lib.pl_cond_solve(ddm._h, p(one), None, None, 1e-8, 10, p(two), None) == _capi.PL_ERR_STATE
        assert lib.pl_cond_flux(ddm._h, p(two), p(two)) == _capi.PL_ERR_STATE
        assert lib.pl_cond_sens(ddm._h, p(two), p(two), p(two)) == _capi.PL_ERR_STATE
        assert lib.pl_thermal_load_adjoint(ddm._h, p(six), p(two)) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
    # a loopback multi-rank handle (pl_dist_init)
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            xn, x6, xb = np.zeros(dev.n_nodes), np.zeros(6 * dev.n_nodes), np.zeros(dev.n_beams)
            m = np.ones(dev.n_nodes, np.uint8)
            assert lib.pl_set_conduction(dev._h, 0.2, None) == _capi.PL_ERR_STATE
            assert lib.pl_cond_spmv(dev._h, 0, None, p(xn), p(xn)) == _capi.PL_ERR_STATE
            assert lib.pl_cond_solve(dev._h, p(m), None, None, 1e-8, 10, p(xn), None) == _capi.PL_ERR_STATE
            assert lib.pl_cond_flux(dev._h, p(xn), p(xb)) == _capi.PL_ERR_STATE
            assert lib.pl_cond_sens(dev._h, p(xn), p(xn), p(xb)) == _capi.PL_ERR_STATE
            assert lib.pl_thermal_load_adjoint(dev._h, p(x6), p(xn)) == _capi.PL_ERR_STATE


DDM_PRESET = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                           "radii": [0.05], "geom_types": ["BCC"]},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                        "DDM": {"enable_preconditioner": False, "max_iterations": 1000,
                                                "schur_complement_computation": {"type": "exact"}}},
              "boundary_conditions": _preset(("BCC",), (2, 1, 1), [0.05])["boundary_conditions"]}


def test_ddm_mode_and_reference_compat_refuse():
    L = LatticeSim(copy.deepcopy(DDM_PRESET), enable_domain_decomposition_solver=True)
    with pytest.raises(ValueError, match="FEM"):
        L.solve_temperature(0.2, {"Surface": ["Zmin"], "Value": 20.0})
    p = copy.deepcopy(DDM_PRESET)
    p["simulation_parameters"]["thermal"] = {"alpha": 7e-5, "conduction": copy.deepcopy(CONDUCTION)}
    with pytest.raises(ValueError, match="FEM"):
        LatticeSim(copy.deepcopy(p), enable_domain_decomposition_solver=True)
    p["optimization_informations"] = dict(copy.deepcopy(OPTI["optimization_informations"]), simulation_type="DDM",
                                          optimization_parameters={"type": "constant", "hybrid": False})
    with pytest.raises(ValueError, match="thermal"):
        LatticeOpti(p)
    compat = LatticeSim(_preset(("BCC",), (2, 1, 1), [0.05]), reference_compat=True)
    with pytest.raises(NotImplementedError):
        compat.solve_temperature(0.2, {"Surface": ["Zmin"], "Value": 20.0})
