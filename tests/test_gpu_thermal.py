"""Thermal loads on the device (pl_set_thermal / pl_thermal_load / pl_thermal_sens, csrc/pl_thermal.h) and the thermal-aware
stress and buckling passes against their numpy restatements (thermal_host.py, stress_host.py, buckling_host.py): exact
states without a solve, a solved state against a dense host solve, the untouched plain path, bitwise reproducibility,
derivatives against central differences of the device, the way up through LatticeSim, LatticeOpti and HomogenizedCell, and
the error codes."""
import copy

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import geometric_host as GH                      # noqa: E402
from pylatticedso_amd import thermal_host as TH                        # noqa: E402
from pylatticedso_amd.homogenization_cell import HomogenizedCell       # noqa: E402
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


def _device(L, penalised=True, **kw):
    lat, pen = L.lattice, L.penalized
    if penalised:
        sl, sn = pen.seg_len, pen.seg_nsub
    else:                                            # one segment per strut, the sub-element count of the whole strut
        sl = np.zeros_like(pen.seg_len)
        sl[:, 1] = pen.seg_len.sum(axis=1)
        sn = np.zeros_like(pen.seg_nsub)
        sn[:, 1] = np.maximum(pen.seg_nsub.sum(axis=1), 1)
    dev = _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, sl, sn, E, NU, **kw)
    dev.set_bc(np.zeros((dev.n_nodes, 6), bool))
    return dev


def _generic_field(n, seed):
    """The generic displacement field of tests/test_gpu_buckling.py: no symmetry, tension and compression, no N at zero."""
    return np.random.default_rng(seed).standard_normal((n, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3


def _thermal_inputs(dev, seed):
    """A random positive dT per node and a random expansion coefficient per strut, sized so that the thermal strain is of
    the order of the strains of ``_generic_field``."""
    rng = np.random.default_rng(seed)
    return 40.0 + 10.0 * (2.0 * rng.random(dev.n_nodes) - 1.0), (2.0 + 5.0 * rng.random(dev.n_beams)) * 1e-5


def _close(got, ref, tol, what):
    """|got - ref| <= tol x the largest magnitude of ref, NaN in the same places."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    if np.isnan(ref).all():
        return
    scale = np.nanmax(np.abs(ref))
    err = np.nanmax(np.abs(got - ref))
    assert err <= tol * scale, (what, err / scale if scale else err)


def _compare(dev, u, lam, p=8):
    """Every output of the thermal calls and of the thermal-aware passes against the restatement: values within 1e-12 of
    the largest magnitude, derivatives within 1e-10 (the bounds of tests/test_gpu_stress.py and tests/test_gpu_buckling.py)."""
    f, n_free = dev.thermal_load()
    f_h, n_free_h = dev.thermal_load_host()
    _close(f, f_h, 1e-12, "f_th")
    _close(n_free, n_free_h, 1e-12, "n_free")
    assert not f[:, 3:].any()
    _close(dev.thermal_sens(lam), dev.thermal_sens_host(lam), 1e-10, "thermal_sens(lam)")
    for where in (0, 1):
        got, ref = dev.stress(u, where=where), dev.stress_host(u, where=where)
        for name in ("N", "V", "T", "Mb", "sigma_vm", "peak"):
            _close(got[name], ref[name], 1e-12, ("stress", where, name))
        a, b = dev.stress_pnorm(p, u, where=where), dev.stress_pnorm_host(p, u, where=where)
        assert abs(a[0] - b[0]) <= 1e-12 * b[0] and abs(a[1] - b[1]) <= 1e-12 * b[1]
        _close(a[2], b[2], 1e-10, ("dphi_du", where))
        _close(a[3], b[3], 1e-10, ("dphi_dr", where))
    out = {}
    for length, shear in ((0, 0), (1, 1)):
        kw = dict(length=length, k_eff=0.7, shear=shear)
        got, ref = dev.buckling(u, **kw), dev.buckling_host(u, **kw)
        for name in ("util", "n_axial", "n_crit"):
            _close(got[name], ref[name], 1e-12, ("buckling", length, shear, name))
        assert np.array_equal(got["util"] == 0.0, ~(got["n_axial"] < 0) & ~np.isnan(got["util"]))   # tension: exactly 0
        a, b = dev.buckling_pnorm(p, u, **kw), dev.buckling_pnorm_host(p, u, **kw)
        assert abs(a[0] - b[0]) <= 1e-12 * b[0] and abs(a[1] - b[1]) <= 1e-12 * b[1]
        _close(a[2], b[2], 1e-10, ("dbp_du", length, shear))
        _close(a[3], b[3], 1e-10, ("dbp_dr", length, shear))
        out[length] = got
    return n_free, out


CASES = [(g, pen) for g in (("BCC",), ("Octet",), ("BCC", "Hybrid1"), ("Octet", "Hybrid4")) for pen in (True, False)]


@pytest.mark.parametrize("geoms,penalised", CASES, ids=lambda v: "+".join(v) if isinstance(v, tuple) else ("pen" if v else "plain"))
def test_parity_with_the_restatement(geoms, penalised):
    """1 x 1 x 1 cells, reorder 0 and 1 (node and strut permutations), 1, 4 and 16 lanes per node; the thermal state shifts
    the outputs (the comparison is not one of two plain passes)."""
    L = _lattice(geoms, (1, 1, 1))
    u = _generic_field(L.lattice.n_nodes, 7)
    lam = _generic_field(L.lattice.n_nodes, 17)
    for reorder, lpn in ((0, 4), (1, 1), (1, 4), (1, 16)):
        with _device(L, penalised, reorder=reorder, lanes_per_node=lpn) as dev:
            dev.assemble()
            plain = dev.buckling(u, length=0)["n_axial"]
            dT, alpha = _thermal_inputs(dev, 3)
            dev.set_thermal(0.0, dT, alpha)
            n_free, out = _compare(dev, u, lam)
            assert (n_free > 0).all()
            _close(out[0]["n_axial"], plain - n_free, 1e-12, "N = (F.t - F_th) / k")
            assert (out[0]["util"] > 0).any() and (out[0]["n_axial"] > 0).any()
    # lam = None is the last solution
    f = np.zeros((L.lattice.n_nodes, 6))
    f[:, :3] = L.applied_force[:, :3]
    with _device(L, penalised) as dev:
        dev.set_bc(L.fixed_DOF, None, f)
        dev.assemble()
        dT, alpha = _thermal_inputs(dev, 3)
        dev.set_thermal(0.0, dT, alpha)
        usol, _ = dev.solve(rtol=1e-10)
        _close(dev.thermal_sens(None), dev.thermal_sens_host(usol), 1e-10, "thermal_sens(None)")
        assert np.array_equal(dev.thermal_sens(None), dev.thermal_sens(usol))


@pytest.mark.parametrize("reorder", [0, 1])
def test_parity_with_strut_multiplicity(reorder):
    """2 x 2 x 1 Octet with multiplicities 1 and 2; one copy carries what the single strut carries."""
    L = _lattice(("Octet",), (2, 2, 1), [0.04])
    mult = np.random.default_rng(3).integers(1, 3, L.lattice.n_beams).astype(float)
    assert (mult == 1).any() and (mult == 2).any()
    u = _generic_field(L.lattice.n_nodes, 8)
    lam = _generic_field(L.lattice.n_nodes, 18)
    with _device(L, reorder=reorder, beam_mult=mult) as dev, _device(L, reorder=reorder) as one:
        dev.assemble()
        one.assemble()
        dT, alpha = _thermal_inputs(dev, 4)
        for d in (dev, one):
            d.set_thermal(0.0, dT, alpha)
        n_free, out = _compare(dev, u, lam, p=6)
        n_free_1 = one.thermal_load()[1]
        _close(n_free, n_free_1, 1e-12, "n_free of one copy")
        _close(dev.thermal_load()[0], TH.thermal_load(one.records(), one.beam_conn, one.n_nodes,
                                                      TH.elongation(one.node_xyz, one.beam_conn, alpha, dT) * mult)[0],
               1e-12, "k copies push k times")
        for length in (0, 1):
            single = one.buckling(u, length=length, k_eff=0.7, shear=length)
            for name in ("util", "n_axial", "n_crit"):
                _close(out[length][name], single[name], 1e-12, (length, name))


def test_exact_state_without_a_solve():
    """2 x 2 x 2 BCC, uniform dT, u_ex = alpha dT (x - x_0): K u_ex = f_th, no mechanical force, no utilisation."""
    L = _lattice(("BCC",), (2, 2, 2))
    alpha, dT = 7e-5, 40.0
    with _device(L) as dev:
        dev.assemble()
        dev.set_thermal(alpha, np.full(dev.n_nodes, dT))
        u_ex = np.zeros((dev.n_nodes, 6))
        u_ex[:, :3] = alpha * dT * (dev.node_xyz - dev.node_xyz[0])
        f, n_free = dev.thermal_load()
        mult = np.ones(dev.n_beams)
        scale = np.abs(mult * n_free).max()
        assert np.abs(dev.spmv(u_ex) - f).max() <= 1e-12 * scale
        N = dev.stress(u_ex)["N"]
        assert np.nanmax(np.abs(N)) <= 1e-12 * n_free.max()
        bk = dev.buckling(u_ex)
        ok = ~np.isnan(bk["util"])
        assert np.all(bk["util"][ok & ~(bk["n_axial"] < 0)] == 0.0)
        assert np.nanmax(bk["util"]) <= 1e-12 * n_free.max() / np.nanmin(bk["n_crit"])


COLUMN = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 3},
                       "radii": [0.05], "geom_types": ["BCC"]},
          "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
          "boundary_conditions": {"Displacement": {"Foot": {"Surface": ["Zmin"], "DOF": ALL6, "Value": [0] * 6},
                                                   "Head": {"Surface": ["Zmax"], "DOF": ALL6, "Value": [0] * 6}}}}


def test_solved_state_through_lattice_sim():
    """2 x 2 x 2 BCC held at node 0 and heated: the displacements against the host dense solve of the same system within the
    1e-7 relative L2 that tests/test_gpu_parity.py asks of solved displacements; then a column between clamped faces."""
    L = _lattice(("BCC",), (2, 2, 2))
    L.fixed_DOF[:] = False
    L.fixed_DOF[0] = True
    L.applied_force[:] = 0.0
    L.displacement_vector[:] = 0.0
    alpha = 7e-5
    L.set_temperature(lambda x: 30.0 + 20.0 * x[:, 2], alpha)          # a temperature drop across the lattice
    _, model = solve_FEM_FenicsX(L)
    dev = model.device
    dT = 30.0 + 20.0 * L.lattice.node_xyz[:, 2]
    rec = dev.records()
    f_h, n_free_h = TH.thermal_load(rec, dev.beam_conn, dev.n_nodes, TH.elongation(dev.node_xyz, dev.beam_conn, alpha, dT))
    K = GH.elastic_matrix(rec, dev.beam_conn, dev.n_nodes).toarray()
    free = np.flatnonzero(~np.asarray(L.fixed_DOF, bool).ravel())
    ref = np.zeros(6 * dev.n_nodes)
    ref[free] = scipy.linalg.solve(K[np.ix_(free, free)], f_h.ravel()[free], assume_a="pos")
    err = np.linalg.norm(model.u.ravel() - ref) / np.linalg.norm(ref)
    print(f"\nsolved thermal state against the dense host solve: relative L2 error {err:.2e}")
    assert err < 1e-7
    _close(L.thermal_strut_forces(), n_free_h, 1e-12, "thermal_strut_forces")
    # the supports answer K u - f_th: nothing here, the lattice expands freely about node 0 up to the temperature gradient
    R = model.reactions
    assert np.abs(R[0]).max() <= 1e-6 * np.abs(f_h).max()
    st = L.strut_stress()
    _close(st["N"], dev.stress_host(model._u_solver)["N"], 1e-12, "mechanical N of strut_stress")
    with pytest.raises(RuntimeError, match="thermal prestress"):
        L.global_buckling()
    L.clear_temperature()
    assert L.thermal is None and dev._thermal is None
    L._device.close()

    hot = LatticeSim(copy.deepcopy(COLUMN))
    hot.set_temperature(40.0, alpha)
    solve_FEM_FenicsX(hot)
    bk = hot.strut_buckling()
    d = hot.lattice.node_xyz[hot.lattice.beam_conn[:, 1]] - hot.lattice.node_xyz[hot.lattice.beam_conn[:, 0]]
    axial = np.abs(d[:, 2]) > 0.5 * np.linalg.norm(d, axis=1)
    assert axial.any() and np.all(bk["n_axial"][axial] < 0) and np.all(bk["util"][axial] > 0)
    assert hot.max_strut_buckling() > 0 and hot.max_strut_stress() > 0
    cold = LatticeSim(copy.deepcopy(COLUMN))
    cold.set_temperature(-40.0, alpha)
    solve_FEM_FenicsX(cold)
    back = cold.strut_buckling()
    assert np.all(back["util"][axial] == 0.0) and np.all(back["n_axial"][axial] > 0)
    preset = copy.deepcopy(COLUMN)
    preset["simulation_parameters"]["thermal"] = {"alpha": alpha, "delta_T": 40.0}
    same = LatticeSim(preset)
    solve_FEM_FenicsX(same)
    assert np.array_equal(same.strut_buckling()["util"], bk["util"], equal_nan=True)
    for sim in (hot, cold, same):
        sim._device.close()


def _four_outputs(dev, u):
    s, b = dev.stress(u), dev.buckling(u, length=0)
    sp, bp = dev.stress_pnorm(8, u), dev.buckling_pnorm(8, u, length=0)
    return [s[k] for k in ("N", "V", "T", "Mb", "sigma_vm", "peak")] + [b[k] for k in ("util", "n_axial", "n_crit")] + \
        [np.array(sp[:2]), sp[2], sp[3], np.array(bp[:2]), bp[2], bp[3]]


def test_nothing_moves_without_a_thermal_state():
    L = _lattice(("BCC", "Hybrid1"), (2, 1, 1))
    u = _generic_field(L.lattice.n_nodes, 5)
    with _device(L) as dev:
        dev.assemble()
        before = _four_outputs(dev, u)
        dev.set_thermal(7e-5, np.zeros(dev.n_nodes))
        zero = _four_outputs(dev, u)
        dev.set_thermal(7e-5, np.full(dev.n_nodes, 40.0))
        shifted = _four_outputs(dev, u)
        dev.clear_thermal()
        after = _four_outputs(dev, u)
    for a, z, c in zip(before, zero, after):
        assert a.tobytes() == z.tobytes() == c.tobytes()
    assert shifted[0].tobytes() != before[0].tobytes()                 # (the state does reach the kernels)


def test_bitwise_reproducible_over_many_blocks():
    L = _lattice(("Octet",), (6, 6, 6), [0.03])
    assert L.lattice.n_beams > 5000                                # > 20 blocks of 256 struts
    u = _generic_field(L.lattice.n_nodes, 9)
    lam = _generic_field(L.lattice.n_nodes, 19)
    with _device(L) as dev:
        dev.assemble()
        dT, alpha = _thermal_inputs(dev, 6)
        dev.set_thermal(0.0, dT, alpha)
        a, b = dev.thermal_load(), dev.thermal_load()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert dev.thermal_sens(lam).tobytes() == dev.thermal_sens(lam).tobytes()
        for call in (lambda: dev.stress_pnorm(8, u), lambda: dev.buckling_pnorm(8, u, length=0)):
            a, b = call(), call()
            assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def test_derivatives_against_central_differences_of_the_device():
    """Steps, bound and kink guard of tests/test_gpu_buckling.py::test_derivatives_against_central_differences_of_the_device,
    the guard on the thermal-aware n_axial; thermal_sens against central differences of thermal_load."""
    L = _lattice(("BCC",), (2, 1, 1))
    lat = L.lattice
    rng = np.random.default_rng(21)
    u = _generic_field(lat.n_nodes, 10)
    lam = _generic_field(lat.n_nodes, 20)
    rad = lat.beam_radius * (0.8 + 0.4 * rng.random(lat.n_beams))
    p = 8
    with _device(L) as dev:
        dev.update_radii(rad)
        dev.assemble()
        dT, alpha = _thermal_inputs(dev, 8)
        dev.set_thermal(0.0, dT, alpha)
        calls = {"stress": lambda u_, g: dev.stress_pnorm(p, u_, where=0, want_grad=g),
                 "buckling": lambda u_, g: dev.buckling_pnorm(p, u_, want_grad=g, length=0, k_eff=0.8, shear=1)}
        grads = {k: c(u, True) for k, c in calls.items()}
        ts = dev.thermal_sens(lam)
        N0 = dev.buckling(u, length=0)["n_axial"]
        assert (N0 < 0).any() and (N0 > 0).any()
        hu = 1e-6
        for k in range(4):
            d = rng.standard_normal(u.shape) * np.abs(u).max()
            assert np.all(np.abs(N0) > 100 * np.abs(dev.buckling(u + hu * d, length=0)["n_axial"] - N0)), "kink (u)"
            for name, call in calls.items():
                fd = (call(u + hu * d, False)[0] - call(u - hu * d, False)[0]) / (2 * hu)
                an = float((grads[name][2] * d).sum())
                assert abs(an - fd) <= 2e-3 * abs(fd), (name, "u", k, an, fd)
        h = 1e-4
        for k in range(4):
            e = rng.standard_normal(lat.n_beams) * rad
            vals, loads = {n: [] for n in calls}, []
            for sgn in (1.0, -1.0):
                dev.update_radii(rad + sgn * h * e)
                dev.assemble()
                for name, call in calls.items():
                    vals[name].append(call(u, False)[0])
                loads.append(dev.thermal_load()[0])
                assert np.all(np.abs(N0) > 100 * np.abs(dev.buckling(u, length=0)["n_axial"] - N0)), "kink (r)"
            for name in calls:
                fd = (vals[name][0] - vals[name][1]) / (2 * h)
                an = float(grads[name][3] @ e)
                assert abs(an - fd) <= 2e-3 * abs(fd), (name, "r", k, an, fd)
            fd = float((lam * (loads[0] - loads[1])).sum()) / (2 * h)
            an = float(ts @ e)
            assert abs(an - fd) <= 2e-3 * abs(fd), ("thermal_sens", k, an, fd)


# ---------------------------------------------------------------------------------------------------------------------
# LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
OPTI = _preset(("BCC",), (3, 2, 2), [0.05])
OPTI["gradient"] = {"radii": {"rule": "linear", "direction_x": True, "direction_y": False, "direction_z": False,
                              "parameter_x": 0.2, "parameter_y": 0.0, "parameter_z": 0.0}}
OPTI["boundary_conditions"]["Force"]["Load"]["Surface"] = ["Xmax", "Zmax"]
OPTI["simulation_parameters"]["thermal"] = {"alpha": 7e-5, "delta_T": 40.0}
OPTI["optimization_informations"] = {
    "objective_function": "min", "objective_type": "compliance", "max_iterations": 5,
    "optimization_parameters": {"type": "unit_cell"},
    "constraints": {"relative_density": {"value": 0.05}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}


def _opti(buckling=None, stress=None, graded=True, **opt):
    p = copy.deepcopy(OPTI)
    if not graded:
        p.pop("gradient")
    p["optimization_informations"].update(opt)
    if buckling is not None:
        p["optimization_informations"]["constraints"]["buckling"] = buckling
    if stress is not None:
        p["optimization_informations"]["constraints"]["max_stress"] = stress
    return p


def _theta(L):
    return list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters)), [0, 5, 11]


def _fd(value, theta, i, h=1e-4):
    tp, tm = list(theta), list(theta)
    tp[i] += h
    tm[i] -= h
    return (value(tp) - value(tm)) / (2 * h)


@pytest.mark.parametrize("objective", ["compliance", "displacement"])
def test_objective_gradient_under_a_thermal_load(objective):
    """Central differences of the objective, step 1e-4 and the 2e-3 bound of test_buckling_constraint_gradient.  The
    compliance J = f_ext . u has the adjoint K lam = f_ext, not u: the gradient formed with lam = u misses the same bound."""
    opt = {} if objective == "compliance" else dict(objective_type="displacement", objective_function="max",
                                                    objective_data={"Surface": ["Xmax"], "DOF": ["Z"]})
    L = LatticeOpti(_opti(**opt))
    assert L.thermal is not None
    theta, idxs = _theta(L)
    L.objective(theta)
    g = np.asarray(L.gradient(theta))
    fds = {i: _fd(L.objective, theta, i) for i in idxs}
    for i in idxs:
        print(f"\n{objective} variable {i}: gradient {g[i]:.8e}, difference quotient {fds[i]:.8e}")
        assert abs(g[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(g).max()), (objective, i, g[i], fds[i])
    if objective == "compliance":
        L.objective(theta)
        L._adjoint = lambda q: L._model.u                              # the adjoint of a lattice without thermal load
        wrong = np.asarray(L.gradient(theta))
        del L._adjoint
        assert any(not abs(wrong[i] - fds[i]) < 2e-3 * max(abs(fds[i]), np.abs(wrong).max()) for i in idxs), (wrong, fds)


@pytest.mark.parametrize("key,settings", [("buckling", {"value": 1.0}), ("max_stress", {"value": 1.0, "p": 8, "where": 1})])
def test_constraint_gradient_under_a_thermal_load(key, settings):
    L = LatticeOpti(_opti(**({"buckling": settings} if key == "buckling" else {"stress": settings})))
    theta, idxs = _theta(L)
    L.objective(theta)
    value = L.buckling_constraint if key == "buckling" else L.stress_constraint
    g = (L.buckling_constraint_gradient if key == "buckling" else L.stress_constraint_gradient)(theta)
    assert g.shape == (L.number_parameters,) and np.abs(g).max() > 0
    for i in idxs:
        fd = _fd(value, theta, i)
        print(f"\n{key} variable {i}: gradient {g[i]:.8e}, difference quotient {fd:.8e}")
        assert abs(g[i] - fd) < 2e-3 * max(abs(fd), np.abs(g).max()), (key, i, g[i], fd)


def test_five_iterations_with_density_and_buckling_under_a_thermal_load():
    """Five SLSQP iterations under the volume bound and a buckling bound 20 % above the start's B_p, as
    tests/test_gpu_buckling.py::test_five_iterations_with_density_and_buckling, with the preset's thermal block.  The buckling
    constraint carries an analytic Jacobian and ends feasible to SLSQP's ftol.  The density constraint is handed to SLSQP
    without one: scipy differentiates it forward with the step optim_eps in the normalised variables, so its linear model -
    and with it the feasibility of a run that stops at the iteration limit, not at convergence - is good to that step
    relative to the constraint's own scale, the bound: rho - rho_max <= optim_eps * rho_max."""
    par = {"type": "linear", "direction": ["x", "z"]}
    probe = LatticeOpti(_opti({"value": 1.0}, graded=False, optimization_parameters=par))
    probe._initialize_optimization_solver()
    b0 = probe.buckling_constraint(probe.initial_parameters) + 1.0
    assert b0 > 0
    L = LatticeOpti(_opti({"value": 1.2 * b0}, graded=False, optimization_parameters=par))
    L.redefine_optim_parameters(max_iteration=5, disp=False)
    sol = L.optimize_lattice()
    assert len(L.constraints) == 2 and L.thermal is not None
    c = L.buckling_constraint(sol.x)
    print(f"\nB_p at the start {b0:.6g}; after {sol.nit} iterations: buckling constraint {c:.3e}, "
          f"relative density {L.relative_density():.5f}, compliance {L.compute_compliance():.6g}")
    assert c <= L.optim_ftol, c
    rho_max = float(L.constraints_dict["relative_density"]["value"])
    excess = L.density_constraint(sol.x)
    print(f"relative density above its bound by {excess:.3e} (allowed {L.optim_eps * rho_max:.1e})")
    assert excess <= L.optim_eps * rho_max, excess


# ---------------------------------------------------------------------------------------------------------------------
# homogenised expansion
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geoms,radii,bimaterial", [(("BCC",), (0.05,), False), (("Octet", "BCC"), (0.04, 0.06), True)],
                         ids=["BCC", "Octet+BCC-bimaterial"])
def test_homogenized_cell_thermal_expansion(geoms, radii, bimaterial):
    """alpha_hom on the device against thermal_host.homogenized_expansion to 1e-8, the bound the device homogenisation is held
    to against its fixture."""
    L = _lattice(geoms, (1, 1, 1), list(radii))
    lat = L.lattice
    alpha = 7e-5
    beam_alpha = np.where(np.asarray(lat.beam_type) == 0, 7e-5, 2e-5) if bimaterial else None
    cell = HomogenizedCell(L)
    with pytest.raises(RuntimeError):
        cell.thermal_expansion(alpha)
    cell.prepare_simulation()
    cell.apply_dirichlet_for_homogenization()
    cell.periodic_boundary_condition()
    cell.solve_full_homogenization()
    got = cell.thermal_expansion(alpha, beam_alpha)
    ref = TH.homogenized_expansion(cell.device.records(), lat.beam_conn, lat.node_xyz, lat.cell_coord[0], lat.cell_size[0],
                                   alpha if beam_alpha is None else beam_alpha)
    print("\nalpha_hom / 7e-5:", got / 7e-5)
    assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max(), (got, ref)
    if bimaterial:
        assert abs(got[0] / 7e-5 - 0.736349) <= 1e-5 and np.abs(got[3:]).max() <= 1e-8 * got[0]
    else:
        assert np.abs(got - alpha * np.array([1, 1, 1, 0, 0, 0])).max() <= 1e-8 * alpha
    assert cell.device._thermal is None
    L._device.close()


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
        lam = _generic_field(n, 1)
        dT = np.full(n, 10.0)
        assert code(dev.thermal_load) == _capi.PL_ERR_STATE              # before pl_set_thermal (and before assembly)
        assert code(dev.thermal_sens, lam) == _capi.PL_ERR_STATE
        dev.set_thermal(1e-5, dT)
        assert code(dev.thermal_load) == _capi.PL_ERR_STATE              # before pl_assemble
        assert code(dev.thermal_sens, lam) == _capi.PL_ERR_STATE
        assert b"pl_assemble" in lib.pl_last_error()
        dev.clear_thermal()
        dev.assemble()
        assert code(dev.thermal_load) == _capi.PL_ERR_STATE              # assembled, but no thermal state
        assert b"pl_set_thermal" in lib.pl_last_error()
        dev.set_thermal(1e-5, dT)
        assert code(dev.thermal_sens, None) == _capi.PL_ERR_STATE        # lam = NULL without a solve
        assert lib.pl_thermal_load(dev._h, None, None) == _capi.PL_ERR_ARG
        assert lib.pl_thermal_sens(dev._h, p(np.ascontiguousarray(lam.ravel())), None) == _capi.PL_ERR_ARG
        f = np.empty((n, 6))
        assert lib.pl_thermal_load(dev._h, p(f), None) == _capi.PL_OK    # a subset of the outputs is fine
        nf = np.empty(nb)
        assert lib.pl_thermal_load(dev._h, None, p(nf)) == _capi.PL_OK
        assert np.array_equal(f, dev.thermal_load()[0]) and np.array_equal(nf, dev.thermal_load()[1])
        for bad in (np.nan, np.inf, -np.inf):
            bad_dT = dT.copy()
            bad_dT[n // 2] = bad
            assert code(dev.set_thermal, 1e-5, bad_dT) == _capi.PL_ERR_ARG
            assert code(dev.set_thermal, bad, dT) == _capi.PL_ERR_ARG
            bad_alpha = np.full(nb, 1e-5)
            bad_alpha[nb // 2] = bad
            assert code(dev.set_thermal, 1e-5, dT, bad_alpha) == _capi.PL_ERR_ARG
        assert np.array_equal(nf, dev.thermal_load()[1])                 # a refused call leaves the state alone
        # K_g from K_e u_e would ignore the thermal prestress
        dev.set_bc(L.fixed_DOF)
        u = _generic_field(n, 2)
        assert code(dev.buckling_modes, 2, u) == _capi.PL_ERR_STATE
        assert b"thermal" in lib.pl_last_error()
        assert code(dev.geom_spmv_multi, u[None], u) == _capi.PL_ERR_STATE
        assert b"thermal" in lib.pl_last_error()
        dev.clear_thermal()
        assert dev.geom_spmv_multi(u[None], u).shape == (1, n, 6)
    # DDM handle
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        two, out = np.zeros(2), np.empty(12)
        assert lib.pl_set_thermal(ddm._h, 1e-5, None, p(two)) == _capi.PL_ERR_STATE
        assert lib.pl_thermal_load(ddm._h, p(out), None) == _capi.PL_ERR_STATE
        assert lib.pl_thermal_sens(ddm._h, None, p(out)) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
    # a loopback multi-rank handle (pl_dist_init)
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            dT, f, out = np.zeros(dev.n_nodes), np.empty(6 * dev.n_nodes), np.empty(dev.n_beams)
            assert lib.pl_set_thermal(dev._h, 1e-5, None, p(dT)) == _capi.PL_ERR_STATE
            assert lib.pl_thermal_load(dev._h, p(f), None) == _capi.PL_ERR_STATE
            assert lib.pl_thermal_sens(dev._h, None, p(out)) == _capi.PL_ERR_STATE


DDM_PRESET = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                           "radii": [0.05], "geom_types": ["BCC"]},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False,
                                        "DDM": {"enable_preconditioner": False, "max_iterations": 1000,
                                                "schur_complement_computation": {"type": "exact"}}},
              "boundary_conditions": _preset(("BCC",), (2, 1, 1), [0.05])["boundary_conditions"]}


def test_ddm_mode_refuses_a_temperature():
    L = LatticeSim(copy.deepcopy(DDM_PRESET), enable_domain_decomposition_solver=True)
    L.set_temperature(40.0, 7e-5)
    with pytest.raises(ValueError, match="thermal"):
        L.solve_DDM()
    L.clear_temperature()
    assert L.solve_DDM()[0] is not None
    p = copy.deepcopy(DDM_PRESET)
    p["simulation_parameters"]["thermal"] = {"alpha": 7e-5, "delta_T": 40.0}
    p["optimization_informations"] = dict(copy.deepcopy(OPTI["optimization_informations"]), simulation_type="DDM",
                                          optimization_parameters={"type": "constant", "hybrid": False})
    with pytest.raises(ValueError, match="thermal"):
        LatticeOpti(p)
