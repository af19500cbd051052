"""The p-norm stress constraint of LatticeOpti (FEM mode) on the GPU: its gradient against central differences, an SLSQP
run in which it is active, presets without the key unchanged, DDM mode refused; LatticeSim.strut_stress and the export."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd.lattice_opti import LatticeOpti            # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim              # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX  # noqa: E402

BASE = {
    "geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                 "radii": [0.05], "geom_types": ["BCC"]},
    "gradient": {"radii": {"rule": "linear", "direction_x": True, "direction_y": False, "direction_z": False,
                           "parameter_x": 0.2, "parameter_y": 0.0, "parameter_z": 0.0}},
    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
    "boundary_conditions": {
        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                   "Value": [0, 0, 0, 0, 0, 0]}},
        "Force": {"Load": {"Surface": ["Xmax", "Zmax"], "DOF": ["Z"], "Value": [-0.1]}}},
    "optimization_informations": {
        "objective_function": "min", "objective_type": "compliance", "max_iterations": 5,
        "optimization_parameters": {"type": "unit_cell"},
        "constraints": {"relative_density": {"value": 0.05}},
        "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}}


def _preset(stress=None, graded=True, **opt):
    p = copy.deepcopy(BASE)
    if not graded:
        p.pop("gradient")
    p["optimization_informations"].update(opt)
    if stress is not None:
        p["optimization_informations"]["constraints"]["max_stress"] = stress
    return p


@pytest.mark.parametrize("where", [1, 0])
@pytest.mark.parametrize("kind", ["unit_cell", "linear"])
def test_stress_constraint_gradient(kind, where):
    """stress_constraint_gradient against central differences of stress_constraint, graded BCC preset, step 1e-4 and the
    2e-3 bound of the objective checks (tests/test_gpu_opti.py)."""
    par = {"type": "unit_cell"} if kind == "unit_cell" else {"type": "linear", "direction": ["x", "z"]}
    L = LatticeOpti(_preset({"value": 1.0, "p": 8, "where": where}, optimization_parameters=par))
    if kind == "unit_cell":
        theta = list(0.3 + 0.4 * np.random.default_rng(0).random(L.number_parameters))
        idxs = [0, 5, 11]
    else:
        theta, idxs = [0.2, -0.1, 0.5], [0, 1, 2]
    L.objective(theta)
    g = L.stress_constraint_gradient(theta)
    assert g.shape == (L.number_parameters,) and np.abs(g).max() > 0
    h = 1e-4
    for i in idxs:
        tp, tm = list(theta), list(theta)
        tp[i] += h
        tm[i] -= h
        fd = (L.stress_constraint(tp) - L.stress_constraint(tm)) / (2 * h)
        assert abs(g[i] - fd) < 2e-3 * max(abs(fd), np.abs(g).max()), (kind, where, i, g[i], fd)


def test_constraint_is_active_in_the_loop():
    """compliance under a volume bound, without and with the stress bound: s_allow = 0.9 x the unconstrained optimum's Phi_p
    (measured here), so the unconstrained optimum violates it; the constrained one satisfies it to SLSQP's accuracy (its
    ftol, times ten) and cannot have a lower compliance.

    "cannot be lower" is a statement about the OPTIMA of the two problems, so the preset is one on which SLSQP reaches them:
    the "linear" radius field in x and z (three variables), both runs must end with status 0.  With one variable per cell
    (unit_cell, 12 variables) the problem is not convex and the comparison says nothing: from the symmetric start the
    volume-only run stops on a symmetric stationary point (compliance 0.1333, 9 iterations), the run with the extra
    constraint leaves it and ends lower (0.1026, stress bound inactive) - measured while writing this test.
    Measured here: compliance 0.1713 -> 0.1882, Phi_8 181.8 -> 163.6 (= s_allow, constraint value 1e-10)."""
    def run(stress):
        L = LatticeOpti(_preset(stress, graded=False, optimization_parameters={"type": "linear", "direction": ["x", "z"]}))
        L.redefine_optim_parameters(max_iteration=60, ftol=1e-8, disp=False)
        sol = L.optimize_lattice()
        L.objective(sol.x)
        return L, sol

    free, sol0 = run(None)
    assert sol0.status == 0 and "max_stress" not in free._history
    free.constraints_dict["max_stress"] = {"value": 1.0, "p": 8, "where": 1}
    phi0 = free.stress_constraint(sol0.x) + 1.0
    c0 = free.compute_compliance()
    s_allow = 0.9 * phi0
    con, sol1 = run({"value": s_allow, "p": 8, "where": 1})
    assert sol1.status == 0, sol1.message
    g1 = con.stress_constraint(sol1.x)
    c1 = con.compute_compliance()
    print(f"\nvolume only: compliance {c0:.6g}, Phi_8 {phi0:.6g}; with s_allow = {s_allow:.6g}: compliance {c1:.6g}, "
          f"constraint {g1:.3e}, iterations {sol0.nit} / {sol1.nit}")
    assert g1 <= 10 * 1e-8, g1
    assert c1 >= c0, (c0, c1)
    assert phi0 / s_allow - 1.0 > 0.1                                # the unconstrained optimum violates the bound
    assert con.relative_density() <= 0.05 * 1.02
    hist = con._history["max_stress"]
    assert len(hist) == len(con._history["iteration"]) and all(v is None or v > 0 for v in hist)
    assert con._last_stress[1] <= con._last_stress[0]                # sigma_max <= Phi_p


class _Tape:
    """Records what the device handle answers (solve, sens, reactions) and which radii it is given, then plays the answers
    back in the same order.  On play-back the real call is still made, so the handle's state stays that of a plain run, but
    the recorded answer is returned, and the arguments must be the recorded ones bit for bit."""
    ANSWERS = ("solve", "sens", "reactions")
    INPUTS = ("update_radii",)

    def __init__(self, monkeypatch):
        from pylatticedso_amd._capi import HipLattice
        self.events, self.pos, self.replay = [], 0, False
        for name in self.ANSWERS + self.INPUTS:
            monkeypatch.setattr(HipLattice, name, self._wrap(name, getattr(HipLattice, name)))

    @staticmethod
    def _key(args, kw):
        def one(v):
            return v if v is None or np.isscalar(v) else np.asarray(v, dtype=float).tobytes()
        return tuple(one(v) for v in args) + tuple((k, one(v)) for k, v in sorted(kw.items()))

    def _wrap(self, name, real):
        def call(dev, *args, **kw):
            out = real(dev, *args, **kw)
            key = self._key(args, kw)
            if not self.replay:
                self.events.append((name, key, copy.deepcopy(out)))
                return out
            assert self.pos < len(self.events), f"{name}: call {self.pos} was not made by the first run"
            rname, rkey, rout = self.events[self.pos]
            assert (rname, rkey) == (name, key), f"call {self.pos}: {name} with other arguments than {rname} of the first run"
            self.pos += 1
            return copy.deepcopy(rout)
        return call


def test_preset_without_the_key_is_unchanged(monkeypatch):
    """the constraint list, the history and the optimum of a preset without "max_stress": the same bits from the refactored
    gradient chain as from the chain written out (the former body of calculate_gradient).

    Two SLSQP runs on the device are not comparable bit for bit whatever the host code does: the PCG's dot products are
    summed with floating-point atomics into slots (pl_kernels.h, block_dot), so two pl_solve calls on the same system differ
    in the last bits (seen here: sol.fun 1.2019163607424082 against 1.2019163607423187 from two runs of the SAME code).  The
    host code is what this change touches on this path, so it is compared at equal device answers: the first run records
    every answer of the handle, the second run - written-out chain - gets the same answers back, and has to ask the same
    questions: every radius vector uploaded and every field passed to pl_sens equal bit for bit, call for call."""
    tape = _Tape(monkeypatch)
    L = LatticeOpti(_preset())
    L.redefine_optim_parameters(max_iteration=4, disp=False)
    sol = L.optimize_lattice()
    assert len(L.constraints) == 1 and "max_stress" not in L._history
    assert sum(e[0] == "solve" for e in tape.events) >= 4 and sum(e[0] == "sens" for e in tape.events) >= 4
    tape.replay = True
    M = LatticeOpti(_preset())
    M.redefine_optim_parameters(max_iteration=4, disp=False)

    def written_out():
        lat = M.lattice
        s = M.strut_sensitivities()
        s_cell = np.zeros((lat.n_cells, len(M.geom_types)))
        np.add.at(s_cell, (M._beam_cell, lat.beam_type), s * M._cell_gfac[M._beam_cell])
        return s_cell.ravel()
    M.calculate_gradient = written_out
    sol2 = M.optimize_lattice()
    assert tape.pos == len(tape.events)                               # the second run made every call of the first
    assert np.array_equal(sol.x, sol2.x) and sol.fun == sol2.fun and sol.nit == sol2.nit
    for k in ("objective_norm", "objective", "relative_density", "parameters"):
        assert L._history[k] == M._history[k], k


def test_ddm_mode_refuses_the_key():
    p = _preset({"value": 1.0}, graded=False, simulation_type="DDM")
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError, match="max_stress"):
        LatticeOpti(p)


def test_lattice_sim_strut_stress_and_export(tmp_path):
    import importlib.util
    import os
    p = _preset(graded=False)
    p.pop("optimization_informations")
    L = LatticeSim(p)
    with pytest.raises(RuntimeError):
        L.strut_stress()
    _, model = solve_FEM_FenicsX(L)
    st = L.strut_stress()
    ref = model.device.stress_host(model._u_solver)
    assert np.nanmax(np.abs(st["sigma_vm"] - ref["sigma_vm"])) <= 1e-12 * np.nanmax(ref["sigma_vm"])
    assert L.max_strut_stress() == st["peak"].max() > 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("export_simulation_results",
                                                  os.path.join(root, "src", "pyLatticeSim", "export_simulation_results.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ex = mod.exportSimulationResults(model, "stress", out_dir=str(tmp_path))
    ex.full_export()
    assert "sigma_vm" not in ex._cell_fields                       # full_export writes what it wrote before
    plain = open(os.path.join(str(tmp_path), "stress_p0_000000.vtu")).read()
    assert 'Name="sigma_vm"' not in plain
    ex.export_stress()
    ex.export_finalize()
    from pylatticedso_amd.views import _tables
    t = _tables(L)
    assert ex._cell_fields["sigma_vm"].shape == ex._cell_fields["N"].shape == (t.n_beams,)
    assert not np.isnan(ex._cell_fields["sigma_vm"]).any()
    assert np.isclose(ex._cell_fields["sigma_vm"].max(), st["peak"].max(), rtol=1e-12)
    text = open(os.path.join(str(tmp_path), "stress_p0_000000.vtu")).read()
    assert 'Name="sigma_vm" NumberOfComponents="1"' in text and 'Name="N" NumberOfComponents="1"' in text
