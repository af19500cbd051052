"""pl_sens_gram (the per-strut Gram of several fields in dK_e/dr, one pass) and what stands on it - the radius sensitivities
of the homogenised stiffness and the inverse design of a cell - on the device: against pl_sens pair by
pair, against the numpy restatement (homogenization_host), against central differences of the DEVICE homogenisation, and
the two solvers of HomogenizedCell against each other."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                             # noqa: E402
from pylatticedso_amd import homogenization_host as HH                         # noqa: E402
from pylatticedso_amd import stress_host as SH                                 # noqa: E402
from pylatticedso_amd.homogenization_cell import HomogenizedCell, fit_cell_radii   # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                            # noqa: E402
from pylatticedso_amd.utils_simulation import get_homogenized_sensitivities  # noqa: E402

E, NU, KAPPA, PEN = 1013.0, 0.3, 0.9, 1.5


# ---- the kernel ------------------------------------------------------------------------------------------------------
class Block:
    """4 x 3 x 3 BCC cells with penalised joints: 288 struts = one full workgroup and a ragged second one (32 struts, half a
    wave).  A few struts of multiplicity 2, eight seeded random columns, and pl_sens for every pair of them, computed once."""

    def __init__(self):
        L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 4, "y": 3, "z": 3},
                                     "radii": [0.05], "geom_types": ["BCC"]},
                        "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False}})
        lat, pen = L.lattice, L.penalized
        assert lat.n_beams == 288 and (pen.seg_len[:, [0, 2]] > 0).any()
        rng = np.random.default_rng(5)
        self.mult = np.ones(lat.n_beams)
        self.mult[rng.choice(lat.n_beams, 7, replace=False)] = 2.0
        self.args = (lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU)
        self.dev = _capi.HipLattice(*self.args, kappa=KAPPA, pen_coef=PEN)
        self.dev.set_multiplicity(self.mult)
        self.X = rng.standard_normal((8, lat.n_nodes, 6))
        self.pairs = {(k, l): self.dev.sens(self.X[l], self.X[k]) for k in range(8) for l in range(k, 8)}


@pytest.fixture(scope="module")
def block():
    b = Block()
    yield b
    b.dev.close()


@pytest.mark.parametrize("n_rhs", [1, 2, 6, 8])
def test_sens_gram_equals_pl_sens_pair_by_pair(block, n_rhs):
    """Same fp64 arithmetic as k_sens, another order of the sums (deformations first, then the record's force): a few
    dozen roundings and no cancellation beyond the pairing's own - 1e-12 of the largest entry of the pair's row."""
    dev = block.dev
    G = dev.sens_gram(block.X[:n_rhs])
    assert G.shape == (n_rhs, n_rhs, dev.n_beams)
    for k in range(n_rhs):
        for l in range(k, n_rhs):
            ref = block.pairs[(k, l)]
            err = np.abs(G[k, l] - ref).max() / np.abs(ref).max()
            assert err < 1e-12, (k, l, err)
    assert np.array_equal(G, G.transpose(1, 0, 2))                          # exact: the lower triangle is the mirror
    assert np.array_equal(dev.sens_gram(block.X[:n_rhs]), G)                 # two calls, the same bits
    assert np.array_equal(dev.sens_gram(block.X[:n_rhs].reshape(n_rhs, -1)), G)


def test_sens_gram_equals_the_host_restatement(block):
    drec = SH.drecords_dr(*block.args, KAPPA, PEN, block.mult)
    ref = HH.sens_gram(drec, block.dev.beam_conn, block.X[:6])
    G = block.dev.sens_gram(block.X[:6])
    for k in range(6):
        for l in range(6):
            err = np.abs(G[k, l] - ref[k, l]).max() / np.abs(ref[k, l]).max()
            assert err < 1e-11, (k, l, err)
    # the multiplicity entered: a strut that counts twice has twice the derivative of the single one
    single = HH.sens_gram(SH.drecords_dr(*block.args, KAPPA, PEN), block.dev.beam_conn, block.X[:1])[0, 0]
    assert np.allclose(G[0, 0], block.mult * single, rtol=1e-10, atol=1e-11 * np.abs(single).max())


def test_sens_gram_errors_and_kernel_timing_id(block):
    dev, lib = block.dev, block.dev._lib
    n6 = 6 * dev.n_nodes
    x = np.zeros((9, n6))
    out = np.empty((45, dev.n_beams))
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731
    assert lib.pl_sens_gram(dev._h, 0, p(x), p(out)) == _capi.PL_ERR_ARG
    assert lib.pl_sens_gram(dev._h, 9, p(x), p(out)) == _capi.PL_ERR_ARG
    assert lib.pl_sens_gram(dev._h, 2, None, p(out)) == _capi.PL_ERR_ARG
    assert lib.pl_sens_gram(dev._h, 2, p(x), None) == _capi.PL_ERR_ARG
    with pytest.raises(_capi.PlError) as e:
        dev.sens_gram(x)                                                     # nine columns through the binding
    assert e.value.code == _capi.PL_ERR_ARG
    with pytest.raises(ValueError):
        dev.sens_gram(np.zeros((2, n6 + 1)))
    with _capi.HipLattice.ddm(10, np.arange(10)[None, :], np.eye(60), np.zeros(1, np.int32)) as ddm:
        assert lib.pl_sens_gram(ddm._h, 1, p(np.zeros(60)), p(out)) == _capi.PL_ERR_STATE
    # pl_time_kernel 12 = the kernel alone on the columns of the last call
    with _capi.HipLattice(*block.args, kappa=KAPPA, pen_coef=PEN) as fresh:
        fresh.set_bc(np.zeros((fresh.n_nodes, 6), bool))
        fresh.assemble()
        with pytest.raises(_capi.PlError) as e:
            fresh.time_kernel(12, reps=2)
        assert e.value.code == _capi.PL_ERR_STATE
        G = fresh.sens_gram(block.X[:6])
        assert fresh.time_kernel(12, reps=3) > 0.0
        assert np.array_equal(fresh.sens_gram(block.X[:6]), G)


# ---- homogenised stiffness -------------------------------------------------------------------------------------------
def _analysis(golden_dir, name, solver="device"):
    """HomogenizedCell of a golden cell with every strut radius scaled by U(1, 1.4) through update_radii (segments untouched),
    solved; returns (analysis, radii)."""
    g = np.load(os.path.join(golden_dir, f"lattice_{name}_1x1x1_periodic.npz"))
    L = LatticeSim(json.loads(str(g["preset_json"])))
    a = HomogenizedCell(L, solver=solver, rtol=1e-13)
    r = a.device._radius * np.random.default_rng(11).uniform(1.0, 1.4, a.device.n_beams)
    a.device.update_radii(r)
    a.prepare_simulation()
    a.apply_dirichlet_for_homogenization()
    a.periodic_boundary_condition()
    a.solve_full_homogenization()
    return a, r


FD_TOL = 1e-6


@pytest.mark.parametrize("name", ["bcc", "bcchybrid1"])
def test_homogenized_sensitivity_matches_differences_of_the_device_homogenisation(golden_dir, name):
    """Central differences of the DEVICE homogenisation (update_radii(r +- h), assemble, six PCG solves at rtol 1e-13;
    segments untouched), three struts, h = 1e-4 r.  The differences carry their truncation (host test: <= 8.5e-9 at this
    step) and the solver's error: a relative error e of the matrix is amplified by H / (2 h r dH/dr_b) ~ B / (3 * 2e-4), 7e4
    for the 40 struts of bcchybrid1, so e ~ 1e-12 would show as 7e-8.  FD_TOL = 1e-6 - the tolerance of the host test -
    leaves a factor ten above that and stays ten below the cap of 1e-5.  Observed on the first run: 1.5e-9 ... 2.1e-9 (bcc)
    and 1.9e-9 ... 6.9e-9 (bcchybrid1), i.e. the truncation of the differences alone; the solves did not show."""
    a, r = _analysis(golden_dir, name)
    dev = a.device
    H_raw = a.homogenizeMatrix_raw.copy()
    assert np.linalg.norm(H_raw - H_raw.T) > 1e-3 * np.linalg.norm(H_raw)
    U = np.stack(a.saveDataToExport)
    dH = a.homogenized_sensitivity()
    raw = a.dHomogenizeMatrix_raw.copy()
    assert dH.shape == raw.shape == (6, 6, dev.n_beams)
    assert np.array_equal(dH, 0.5 * (raw + raw.transpose(1, 0, 2)))
    # the host formula on the device's own fields
    drec = SH.drecords_dr(dev.node_xyz, dev.beam_conn, r, dev._seg_len, dev._seg_nsub, *dev._material, mult=dev._mult)
    ref = HH.homogenized_sensitivity(drec, dev.beam_conn, U)
    assert np.abs(raw - ref).max() < 1e-9 * np.abs(ref).max()
    # engineering constants: the class's dict against the host chain rule
    d = a.orthotropic_sensitivity()
    dc = HH.engineering_constants_sensitivity(H_raw, raw)
    assert list(d) == list(HH.CONSTANTS) and all(np.array_equal(d[n], dc[i]) for i, n in enumerate(HH.CONSTANTS))
    per_radius = a.homogenized_sensitivity(per="radius")
    n_geom = len(a.lattice.radii)
    assert per_radius.shape == (6, 6, n_geom) and np.allclose(per_radius.sum(axis=2), dH.sum(axis=2), rtol=1e-12)
    with pytest.raises(ValueError):
        a.homogenized_sensitivity(per="cell")
    worst = 0.0
    for b in np.random.default_rng(3).choice(dev.n_beams, 3, replace=False):
        Hs = []
        for sign in (1.0, -1.0):
            rr = r.copy()
            rr[b] += sign * 1e-4 * r[b]
            dev.update_radii(rr)
            dev.assemble()
            a.solve_full_homogenization()
            Hs.append(a.homogenizeMatrix_raw.copy())
        fd = (Hs[0] - Hs[1]) / (2e-4 * r[b])
        err = np.abs(raw[:, :, b] - fd).max() / np.abs(raw[:, :, b]).max()
        print(name, "strut", b, "device dH_raw vs differences of the device homogenisation", err)
        worst = max(worst, err)
    a.lattice._device.close()
    assert worst < FD_TOL, worst


def test_host_and_device_solvers_give_the_same_sensitivities_and_order_of_calls(golden_dir):
    g = np.load(os.path.join(golden_dir, "lattice_bcchybrid1_1x1x1_periodic.npz"))
    a0 = HomogenizedCell(LatticeSim(json.loads(str(g["preset_json"]))))
    with pytest.raises(RuntimeError):
        a0.homogenized_sensitivity()
    with pytest.raises(RuntimeError):
        a0.orthotropic_sensitivity()
    a0.lattice._device.close()
    out = {}
    for solver in ("device", "host"):
        a, _ = _analysis(golden_dir, "bcchybrid1", solver)
        out[solver] = (a.homogenized_sensitivity(), a.orthotropic_sensitivity(per="radius"))
        a.lattice._device.close()
    assert np.abs(out["device"][0] - out["host"][0]).max() < 1e-8 * np.abs(out["host"][0]).max()
    for n in HH.CONSTANTS:
        assert np.allclose(out["device"][1][n], out["host"][1][n], rtol=1e-7, atol=1e-8 * np.abs(out["host"][1]["Ex"]).max())


def _hybrid(radii):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": [float(r) for r in radii], "geom_types": ["BCC", "Cubic"]},
                       "simulation_parameters": {"enable": False, "material": "VeroClear", "periodicity": True}})


def test_fit_cell_radii_recovers_a_hybrid_cell():
    """BCC + Cubic cell, joint penalisation off (the Jacobian is exact): from (0.05, 0.05) to the matrix of (0.06, 0.04)."""
    want = np.array([0.06, 0.04])
    Lt = _hybrid(want)
    target, dH, at = get_homogenized_sensitivities(Lt)
    assert dH.shape == (6, 6, 2)
    Lt._device.close()
    L = _hybrid([0.05, 0.05])
    res, a = fit_cell_radii(L, target)
    print("fit_cell_radii: nfev", res.nfev, "x", res.x, "cost", res.cost)
    assert np.abs(res.x - want).max() < 1e-6 * want.min()
    assert res.nfev <= 12
    iu = np.triu_indices(6)
    assert np.linalg.norm((a.homogenizeMatrix - target)[iu]) < 1e-8 * np.linalg.norm(target[iu])
    assert np.allclose(L.radii, res.x)
    L._device.close()
    two = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                                   "radii": [0.05], "geom_types": ["BCC"]},
                      "simulation_parameters": {"enable": False, "material": "VeroClear", "periodicity": True}})
    with pytest.raises(ValueError):
        fit_cell_radii(two, target)
