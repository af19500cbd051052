"""Sensitivities of the global buckling load factors on the device (pl_buckling_modes_sens, csrc/pl_geom.h; DESIGN.md section
10d) against the numpy / scipy restatement (geometric_host.buckling_sensitivity): the kernels with exact dense eigenpairs,
the weighted sum, the whole chain pl_buckling_modes -> pl_buckling_modes_sens against differences of the device's own load
factors, the handle's state, the error codes, and the way up through LatticeSim and LatticeOpti.

The towers are those of tests/test_buckling_sens_host.py (cases A and B), plus a 2 x 2 x 2 Octet with multiplicity 2 on every
third strut."""
import copy
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import geometric_host as GH                      # noqa: E402
from pylatticedso_amd import stress_host as SH                         # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

from test_buckling_sens_host import CASES, E, KAPPA, NU, PEN, Tower, preset, tower   # noqa: E402


def _tower(name):
    if name != "octet":
        return tower(name)
    t = Tower("Z", -0.1, True, cells=(2, 2, 2), geom="Octet")
    t.mult = np.where(np.arange(t.n_beams) % 3 == 0, 2.0, 1.0)
    return t


def _device(t, radius=None, **kw):
    dev = _capi.HipLattice(t.xyz, t.conn, t.radius if radius is None else radius, t.seg_len, t.seg_nsub, E, NU, kappa=KAPPA,
                           pen_coef=PEN, beam_mult=t.mult, **kw)
    dev.set_bc(t.fixed, None, t.f)
    dev.assemble()
    return dev


def _bsr(dev):
    """the handle's own K as a scipy matrix"""
    dev.assemble_bsr(False)
    rowptr, col, vals = dev.get_bsr()
    A = sp.bsr_matrix((vals, col, rowptr), shape=(6 * dev.n_nodes, 6 * dev.n_nodes)).tocsr()
    A.sum_duplicates()
    return A


class _Case:
    """One handle, its equilibrium, the dense eigenpairs of its own K and the restatement's rows for five modes: computed
    once, shared by the tests below and left unchanged."""

    def __init__(self, name):
        self.name, self.t = name, _tower(name)
        t = self.t
        self.dev = _device(t)
        self.u, _ = self.dev.solve(rtol=1e-12, max_iter=100000)
        self.rec = self.dev.records()
        self.drec = SH.drecords_dr(t.xyz, t.conn, t.radius, t.seg_len, t.seg_nsub, E, NU, KAPPA, PEN, t.mult)
        Kg = GH.geometric_matrix(self.rec, t.conn, self.u, t.n)
        self.dense = GH.buckling_modes_dense(_bsr(self.dev), Kg, t.fixed, 5)
        assert self.dense["n_found"] == 5
        self.lam, self.modes = self.dense["load_factor"], self.dense["modes"]
        self.rows, self.load = GH.buckling_sensitivity(self.rec, self.drec, t.conn, self.u, t.fixed, self.lam, self.modes)


_cases = {}


@pytest.fixture(scope="module", params=["A", "B", "octet"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


@pytest.fixture(scope="module")
def case_a():
    if "A" not in _cases:
        _cases["A"] = _Case("A")
    return _cases["A"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels, with exact eigenpairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 5])
def test_kernel_parity_with_the_restatement(case, k):
    """Rows within 1e-8 max|row| of the restatement (sparse LU adjoint; a Jacobi-CG adjoint at 1e-12 differs from it by
    1.3e-10 on the host), adj_load within 1e-12 of its largest magnitude, and w_i . du = phi_i . K_g(du) phi_i on the device
    itself within 1e-11.  k = 1, 4, 5: column blocks of 1, 4 and a padded second block."""
    c = case
    out = c.dev.buckling_modes_sens(c.lam[:k], c.modes[:k], c.u, rtol=1e-12, want_load=True)
    rows, load = out["dlam_dr"], out["adj_load"]
    assert rows.shape == (k, c.t.n_beams) and load.shape == (k, c.t.n, 6)
    err = (np.abs(rows - c.rows[:k]).max(axis=1) / np.abs(c.rows[:k]).max(axis=1)).max()
    lerr = np.abs(load - c.load[:k]).max() / np.abs(c.load[:k]).max()
    print(f"\n{c.name}, {k} modes: rows {err:.2e} of max|row|, adj_load {lerr:.2e} of its largest magnitude")
    assert err <= 1e-8
    assert lerr <= 1e-12
    # u = NULL: the solution of the last solve, the same numbers
    null = c.dev.buckling_modes_sens(c.lam[:k], c.modes[:k], rtol=1e-12)["dlam_dr"]
    assert np.array_equal(null, rows)
    du = np.random.default_rng(7).standard_normal((c.t.n, 6)) * 1e-3
    gphi = c.dev.geom_spmv_multi(c.modes[:k], du)
    for i in range(k):
        a, b = float((load[i] * du).sum()), float((c.modes[i] * gphi[i]).sum())
        assert abs(a - b) <= 1e-11 * float((np.abs(load[i]) * np.abs(du)).sum()), (c.name, k, i, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the weighted sum, skipped modes, scaling
# ---------------------------------------------------------------------------------------------------------------------
def test_weighted_sum_and_skipped_modes(case):
    c = case
    w = np.array([0.7, -1.3, 0.2, 2.1, 0.4])
    out = c.dev.buckling_modes_sens(c.lam, c.modes, c.u, weights=w)
    rows, dsum = out["dlam_dr"], out["dsum_dr"]
    ref = w @ rows
    assert dsum.shape == (c.t.n_beams,)
    assert np.abs(dsum - ref).max() <= 1e-13 * np.abs(ref).max()
    only = c.dev.buckling_modes_sens(c.lam, c.modes, c.u, weights=w, want_rows=False)
    assert sorted(only) == ["dsum_dr"] and np.abs(only["dsum_dr"] - ref).max() <= 1e-8 * np.abs(ref).max()
    # a NaN factor: a NaN row, left out of the sum; the mode of such an entry is NaN too (pl_buckling_modes)
    lam, modes = c.lam.copy(), c.modes.copy()
    lam[2], modes[2] = np.nan, np.nan
    out2 = c.dev.buckling_modes_sens(lam, modes, c.u, weights=w, want_load=True)
    keep = [0, 1, 3, 4]
    assert np.isnan(out2["dlam_dr"][2]).all() and np.isnan(out2["adj_load"][2]).all()
    assert np.array_equal(out2["adj_load"][keep], c.dev.buckling_modes_sens(c.lam, c.modes, c.u, want_rows=False,
                                                                            want_load=True)["adj_load"][keep])
    # (two PCG passes in different column blocks: the bound of the parity test)
    assert (np.abs(out2["dlam_dr"][keep] - rows[keep]) / np.abs(rows).max(axis=1)[keep, None]).max() <= 1e-8
    ref2 = w[keep] @ out2["dlam_dr"][keep]
    assert np.abs(out2["dsum_dr"] - ref2).max() <= 1e-13 * np.abs(ref2).max()
    # every factor NaN: nothing to do
    none = c.dev.buckling_modes_sens(np.full(2, np.nan), modes[:2], c.u, weights=w[:2])
    assert np.isnan(none["dlam_dr"]).all() and not none["dsum_dr"].any()


def test_scaling_a_mode_by_three_leaves_its_row(case):
    """Within 1e-12 of max|row|.  kk, q_b and w all scale by 9, so the row is the same up to what the adjoint solve leaves
    open, and that is its tolerance times the conditioning: the host's Jacobi-CG at rtol = 1e-12 moves a row by 4e-13 when the
    two solves stop at the same iteration and by 1e-10 when they do not (case B: 235 against 242 iterations), at 1e-14 by
    3e-14.  A bound of 1e-12 on the rows therefore needs the adjoint at 1e-14, which is what this test asks for."""
    c = case
    a = c.dev.buckling_modes_sens(c.lam[:2], c.modes[:2], c.u, rtol=1e-14)["dlam_dr"]
    modes = c.modes[:2].copy()
    modes[1] *= 3.0
    b = c.dev.buckling_modes_sens(c.lam[:2], modes, c.u, rtol=1e-14)["dlam_dr"]
    err = np.abs(a[1] - b[1]).max() / np.abs(a[1]).max()
    print(f"\n{c.name}: mode scaled by 3, its row changes by {err:.2e} of max|row|")
    assert np.array_equal(a[0], b[0])
    assert err <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_differences_of_the_devices_own_factors(case_a):
    """buckling_modes(4, n_sub = 12) with its defaults, then buckling_modes_sens: rows within 1e-3 max|row| of the restatement
    on dense modes (subspace modes at tol = 1e-9 cost <= 1.1e-5 on the host), and dlam_dr @ dr within 1e-3 relative of the
    central difference of the DEVICE's factors at r +- 1e-4 dr, dr = U(-1, 1) r (truncation <= 9.2e-5, eigenvalue noise about
    1.4e-5 on the host)."""
    c, t = case_a, case_a.t
    with _device(t) as dev:
        dev.solve(rtol=1e-12, max_iter=100000)
        out = dev.buckling_modes(4, n_sub=12)
        assert out["n_found"] == 4
        rows = dev.buckling_modes_sens(out["load_factor"], out["modes"])["dlam_dr"]
        err = (np.abs(rows - c.rows[:4]).max(axis=1) / np.abs(c.rows[:4]).max(axis=1)).max()
        dr = np.random.default_rng(11).uniform(-1.0, 1.0, t.n_beams) * t.radius
        lam = []
        for sign in (1.0, -1.0):
            dev.update_radii(t.radius + sign * 1e-4 * dr)
            dev.assemble()
            dev.solve(rtol=1e-12, max_iter=100000)
            lam.append(dev.buckling_modes(4, n_sub=12)["load_factor"])
        fd = (lam[0] - lam[1]) / 2e-4
        got = rows @ dr
        rel = np.abs(got / fd - 1.0)
        print(f"\nend to end: rows {err:.2e} of max|row| from the restatement on dense modes; directional derivative {got}, "
              f"difference quotient {fd}, relative difference {rel}")
        assert err <= 1e-3
        assert rel.max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 4. the handle's state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_solve_after_the_call_returns_the_same_bits(case_a):
    """pl_solve with the per-node gather product and the Jacobi preconditioner sums in a fixed order (the default K*p
    accumulates with atomics and repeats itself to rounding only), so its bits can be compared.  A second pl_solve on a
    handle is scheduled from the history of the first (its iteration count decides when the residual is first looked at), so
    it is compared with the second solve of a twin handle that made no call in between: the same bits and the same
    iteration count, and the solution of the last solve is still the one u = NULL reads."""
    c = case_a
    fixed_order = dict(spmv_kernel=2, precond=1)
    with _device(c.t, **fixed_order) as dev, _device(c.t, **fixed_order) as twin:
        first = [d.solve(rtol=1e-12, max_iter=100000)[0] for d in (dev, twin)]
        assert np.array_equal(first[0], first[1])
        x = np.random.default_rng(6).standard_normal((1, dev.n_nodes, 6))
        before = dev.geom_spmv_multi(x)
        dev.buckling_modes_sens(c.lam[:4], c.modes[:4], weights=np.ones(4), want_load=True)
        assert np.array_equal(dev.geom_spmv_multi(x), before)            # u = NULL: still the solution of pl_solve
        again = [d.solve(rtol=1e-12, max_iter=100000) for d in (dev, twin)]
        assert np.array_equal(again[0][0], again[1][0])
        assert again[0][1]["iterations"] == again[1][1]["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. error codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    t = tower("A")
    lib, p = _capi.load_library(), _capi._ptr
    n6 = 6 * t.n
    u = np.ascontiguousarray(np.random.default_rng(1).standard_normal(n6) * 1e-3)
    lam = np.array([1.5, 1.7])
    phi = np.ascontiguousarray(np.random.default_rng(2).standard_normal((2, n6)))
    wts = np.ones(2)
    rows, dsum, load = np.empty((17, t.n_beams)), np.empty(t.n_beams), np.empty((17, n6))

    def sens(h, u_=u, n=2, rows_=rows, dsum_=None, load_=None, wts_=None, lam_=lam, phi_=phi):
        return lib.pl_buckling_modes_sens(h, p(u_), n, p(lam_), p(phi_), 1e-10, 10000, p(wts_), p(rows_), p(dsum_), p(load_))

    with _capi.HipLattice(t.xyz, t.conn, t.radius, t.seg_len, t.seg_nsub, E, NU, kappa=KAPPA, pen_coef=PEN) as dev:
        assert sens(dev._h) == _capi.PL_ERR_STATE                       # before pl_assemble
        dev.assemble()
        assert sens(dev._h) == _capi.PL_ERR_STATE                       # before pl_set_bc
        assert b"pl_set_bc" in lib.pl_last_error()
        dev.set_bc(t.fixed, None, t.f)
        assert sens(dev._h, u_=None) == _capi.PL_ERR_STATE              # u = NULL without a solve
        assert sens(dev._h, n=0) == _capi.PL_ERR_ARG
        big = np.full(17, 1.5)
        assert sens(dev._h, n=17, lam_=big, phi_=np.zeros((17, n6))) == _capi.PL_ERR_ARG
        assert sens(dev._h, rows_=None) == _capi.PL_ERR_ARG             # all three outputs NULL
        assert sens(dev._h, dsum_=dsum) == _capi.PL_ERR_ARG             # dsum_dr without weights
        assert b"weights" in lib.pl_last_error()
        assert sens(dev._h, lam_=None) == _capi.PL_ERR_ARG
        assert sens(dev._h, phi_=None) == _capi.PL_ERR_ARG
        assert sens(dev._h) == _capi.PL_OK
        assert sens(dev._h, rows_=None, dsum_=dsum, wts_=wts) == _capi.PL_OK
        assert sens(dev._h, rows_=None, load_=load) == _capi.PL_OK
        master = np.arange(t.n, dtype=np.int32)
        master[t.n - 1] = t.n - 2
        dev.set_periodic(master)
        assert sens(dev._h) == _capi.PL_ERR_STATE
        assert b"periodic" in lib.pl_last_error()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        r2 = np.empty((2, 1))
        assert lib.pl_buckling_modes_sens(ddm._h, p(np.zeros(12)), 2, p(lam), p(np.ones((2, 12))), 1e-10, 100, None, p(r2), None,
                                          None) == _capi.PL_ERR_STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            m6 = 6 * dev.n_nodes
            rr = np.empty((2, dev.n_beams))
            assert lib.pl_buckling_modes_sens(dev._h, p(np.zeros(m6)), 2, p(lam), p(np.ones((2, m6))), 1e-10, 100, None, p(rr),
                                              None, None) == _capi.PL_ERR_STATE
            assert b"multi-rank" in lib.pl_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 6. LatticeSim and LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_sim_global_buckling_sensitivity():
    L = LatticeSim(preset((2, 2, 3), *CASES["A"][:2]))
    with pytest.raises(RuntimeError):
        L.global_buckling_sensitivity()
    solve_FEM_FenicsX(L, rtol=1e-12)
    with pytest.raises(RuntimeError):
        L.global_buckling_sensitivity()                                # no global_buckling yet
    L.global_buckling(4, n_sub=12)
    out = L.global_buckling_sensitivity(p=8)
    nb = L.lattice.n_beams
    assert sorted(out) == ["aggregate", "dJ_dr", "dlam_dr"]
    assert out["dJ_dr"].shape == (nb,) and out["dlam_dr"].shape == (4, nb)
    J, wts = GH.load_factor_aggregate(L.buckling_load_factors, 8)
    assert out["aggregate"] == J >= 1.0 / L.buckling_load_factors[0]
    ref = wts @ out["dlam_dr"]
    assert np.abs(out["dJ_dr"] - ref).max() <= 1e-12 * np.abs(ref).max()
    # thicker struts carry more: the aggregate of 1 / lambda falls with the radii on the whole
    assert out["dJ_dr"].sum() < 0
    assert sorted(L.global_buckling_sensitivity(want_rows=False)) == ["aggregate", "dJ_dr"]


OPTI = preset((2, 2, 3), *CASES["A"][:2])
OPTI["optimization_informations"] = {
    "objective_function": "min", "objective_type": "compliance", "max_iterations": 4,
    "optimization_parameters": {"type": "linear", "direction": ["x", "z"]},
    "constraints": {"relative_density": {"value": 0.2}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}
GLOBAL = {"value": 1.0, "n_modes": 4, "p": 8, "n_sub": 12}


def _opti(constraints, **opt):
    p = copy.deepcopy(OPTI)
    p["optimization_informations"].update(opt)
    p["optimization_informations"]["constraints"].update(constraints)
    return p


def test_global_buckling_constraint_gradient():
    """global_buckling_constraint_gradient against central differences of global_buckling_constraint in every design
    variable, step 1e-4, within 1e-3 relative."""
    L = LatticeOpti(_opti({"global_buckling": GLOBAL}))
    theta = [0.2, -0.1, 0.5]
    L.objective(theta)
    g = L.global_buckling_constraint_gradient(theta)
    assert g.shape == (L.number_parameters,) == (3,) and np.abs(g).max() > 0
    assert abs(GLOBAL["value"] * L._last_global_buckling[0] - 1.0 - L.global_buckling_constraint(theta)) <= 1e-8
    h = 1e-4
    for i in range(3):
        tp, tm = list(theta), list(theta)
        tp[i] += h
        tm[i] -= h
        fd = (L.global_buckling_constraint(tp) - L.global_buckling_constraint(tm)) / (2 * h)
        print(f"\nvariable {i}: gradient {g[i]:.8e}, difference quotient {fd:.8e}, relative difference {abs(g[i] / fd - 1):.2e}")
        assert abs(g[i] - fd) <= 1e-3 * abs(fd), (i, g[i], fd)


def test_aggregate_gradient_of_the_strut_constraint_is_what_it_was():
    """_aggregate_gradient now ends in _strut_gradient_to_parameters, shared with the global constraint: with the same
    adjoint field it returns, bit for bit, the chain written out as it stood before."""
    L = LatticeOpti(_opti({"buckling": {"value": 0.5, "p": 4, "length": 0, "k_eff": 0.5, "shear": 1}}))
    theta = [0.2, -0.1, 0.5]
    L.objective(theta)
    _, _, dq_du, dq_dr = L.strut_buckling_aggregate(want_grad=True)
    lam = L._adjoint(dq_du)
    L._adjoint = lambda q: lam                                          # one adjoint field for both evaluations
    got = L._aggregate_gradient(dq_du, dq_dr)
    s = dq_dr - L.device_model().sens(L._model.u, lam)
    g = L._chain_cell_sensitivities(L._strut_to_cell(s))
    scale = np.ones(L.number_parameters)
    scale[-1] = L.max_radius - L.min_radius
    assert L.enable_normalization and np.abs(got).max() > 0
    assert np.array_equal(got, g * scale)
    assert np.array_equal(L.buckling_constraint_gradient(theta), got / 0.5)


def test_four_iterations_towards_a_larger_load_factor():
    """lambda_min = 1.1 lambda_1 of the start (an infeasible start) under a volume bound with room to grow: after four SLSQP
    iterations the constraint value is <= 1e-6, and every iteration records lambda_1."""
    probe = LatticeOpti(_opti({"global_buckling": GLOBAL}))
    probe._initialize_optimization_solver()
    x0 = probe.initial_parameters
    J0 = probe.global_buckling_constraint(x0) + 1.0
    lam1 = probe._last_global_buckling[1]
    rho0 = probe.relative_density()
    assert J0 >= 1.0 / lam1 > 0
    L = LatticeOpti(_opti({"global_buckling": dict(GLOBAL, value=1.1 * lam1), "relative_density": {"value": 1.5 * rho0}}))
    assert L.global_buckling_constraint(x0) > 0.09
    L.redefine_optim_parameters(max_iteration=4, disp=False)
    sol = L.optimize_lattice()
    assert len(L.constraints) == 2
    c = L.global_buckling_constraint(sol.x)
    print(f"\nlambda_1 at the start {lam1:.6g}, wanted {1.1 * lam1:.6g}; after {sol.nit} iterations: constraint {c:.3e}, "
          f"lambda_1 {L._last_global_buckling[1]:.6g}, relative density {L.relative_density():.5f} (bound {1.5 * rho0:.5f})")
    assert c <= 1e-6, c
    assert L._last_global_buckling[1] >= 1.1 * lam1 * (1.0 - 1e-6)
    hist = L._history["min_load_factor"]
    assert len(hist) == len(L._history["iteration"]) >= 1 and all(v is None or v > 0 for v in hist)
    assert any(v is not None for v in hist)
    assert "max_buckling" not in L._history


def test_ddm_mode_refuses_the_key():
    p = _opti({"global_buckling": GLOBAL}, simulation_type="DDM")
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError, match="global_buckling"):
        LatticeOpti(p)
