"""Natural frequencies on the device (pl_set_mass / pl_mass_spmv_multi / pl_vibration_modes / pl_vibration_modes_sens,
csrc/pl_mass.h) against the numpy / scipy restatement (mass_host.py): the mass product on every
built-in geometry, frequencies and modes against the dense eigen-solution of the handle's own K and the restated M, the
sensitivity kernel with exact dense eigenpairs, the whole chain against differences of the device's own frequencies, the
handle's state, the error codes, and the way up through LatticeSim and LatticeOpti.

The lattices are those of tests/test_mass_host.py: A (graded, penalised 2 x 2 x 3 BCC tower), B (the uniform plain tower, a
double first frequency) and C (graded plain 2 x 2 x 2 Octet); A and C carry one strut of multiplicity 2 and a point mass on
the top face."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import geometric_host as GH                      # noqa: E402
from pylatticedso_amd import mass_host as MH                           # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

from test_mass_host import E, KAPPA, NU, PEN, RHO, _preset, case       # noqa: E402


def _device(c, radius=None, rotary=True, **kw):
    dev = _capi.HipLattice(c.xyz, c.conn, c.radius if radius is None else radius, c.sl, c.sn, E, NU, kappa=KAPPA,
                           pen_coef=PEN, beam_mult=c.mult, **kw)
    dev.set_bc(c.fixed)
    dev.assemble()
    dev.set_mass(RHO, rotary, c.node_mass)
    return dev


def _bsr(dev):
    """the handle's own K as a scipy matrix"""
    dev.assemble_bsr(False)
    rowptr, col, vals = dev.get_bsr()
    A = sp.bsr_matrix((vals, col, rowptr), shape=(6 * dev.n_nodes, 6 * dev.n_nodes)).tocsr()
    A.sum_duplicates()
    return A


N_DENSE = {"A": 4, "B": 5, "C": 4}          # whole clusters: B's spectrum is double, simple, double


class _Case:
    """One handle, the dense eigenpairs of its own K and the restated M, and the restatement's rows: computed once, shared
    by the tests below and left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        self.dev = _device(self.c)
        self.K, self.M = _bsr(self.dev), self.dev.mass_matrix_host()
        self.dense = MH.vibration_modes_dense(self.K, self.M, self.c.fixed, N_DENSE[name])
        self.om2, self.modes = self.dense["omega2"], self.dense["modes"]
        self.rows = self.dev.vibration_modes_sens_host(self.om2, self.modes, self.c.fixed)


_cases = {}


def _get(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=["A", "B", "C"])
def dcase(request):
    return _get(request.param)


@pytest.fixture(scope="module")
def case_a():
    return _get("A")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(_BUILTIN))
def test_operator_parity_with_the_restatement(geom):
    """M X on reorder = 0 and 1 handles, n_rhs = 1, 2, 3, 5 (KB = 1, 2, 4 and a padded block), masked and unmasked, with and
    without the rotary inertia and the point masses, within 1e-12 of the largest magnitude (the bound of the K_g product),
    and X^T M Y = Y^T M X."""
    L = LatticeSim(_preset(geom, (1, 1, 1)))
    lat, pen = L.lattice, L.penalized
    n = lat.n_nodes
    rng = np.random.default_rng(11)
    X, Y = rng.standard_normal((5, n, 6)), rng.standard_normal((5, n, 6))
    mask = rng.random((n, 6)) < 0.25
    mask[0] = True
    radius = 0.03 + 0.04 * rng.random(lat.n_beams)
    nm = 0.05 * rng.random(n)
    worst = 0.0
    for reorder in (0, 1):
        with _capi.HipLattice(lat.node_xyz, lat.beam_conn, radius, pen.seg_len, pen.seg_nsub, E, NU, reorder=reorder) as dev:
            dev.set_bc(mask)
            dev.assemble()
            for rotary in (False, True):
                for node_mass in (None, nm):
                    dev.set_mass(RHO, rotary, node_mass)
                    for masked in (False, True):
                        ref = dev.mass_spmv_multi_host(X, masked=masked, fixed=mask)
                        scale = np.abs(ref).max()
                        for k in (1, 2, 3, 5):
                            got = dev.mass_spmv_multi(X[:k], masked=masked)
                            assert got.shape == (k, n, 6)
                            err = np.abs(got - ref[:k]).max()
                            worst = max(worst, err / scale)
                            assert scale > 0 and err <= 1e-12 * scale, (geom, reorder, rotary, masked, k, err / scale)
                            if masked:
                                assert not got[:, mask].any()
            mx, my = dev.mass_spmv_multi(X), dev.mass_spmv_multi(Y)
            for j in range(5):
                a, b = float((Y[j] * mx[j]).sum()), float((X[j] * my[j]).sum())
                assert abs(a - b) <= 1e-12 * float((np.abs(Y[j]) * np.abs(mx[j])).sum()), (geom, reorder, j, a, b)
                assert float((X[j] * mx[j]).sum()) > 0.0
    print(f"\n{geom}: M X within {worst:.2e} of the largest magnitude")


def test_multiplicity_doubles_and_the_records_follow_the_radii():
    c = case("B")
    X = np.random.default_rng(4).standard_normal((3, c.n, 6))
    mult = np.ones(c.B)
    mult[5] = 2.0
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU) as dev:
        dev.assemble()
        dev.set_mass(RHO)
        one = dev.mass_spmv_multi(X)
        dev.set_multiplicity(mult)
        dev.assemble()
        two = dev.mass_spmv_multi(X)
        # the doubled strut adds its own share once more: its element matrix on its two nodes
        Me = MH.element_matrix(c.xyz[c.conn[5, 1]] - c.xyz[c.conn[5, 0]], c.radius[5], RHO)
        extra = np.zeros_like(X)
        ia, ib = c.conn[5]
        xe = np.concatenate([X[:, ia], X[:, ib]], axis=1)
        ye = xe @ Me.T
        extra[:, ia] += ye[:, :6]
        extra[:, ib] += ye[:, 6:]
        assert np.abs(two - one - extra).max() <= 1e-12 * np.abs(two).max()
        # new radii need no further call
        dev.update_radii(1.5 * c.radius)
        dev.assemble()
        ref = dev.mass_spmv_multi_host(X)
        assert np.abs(dev.mass_spmv_multi(X) - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(ref).max() > 2.0 * np.abs(two).max()


# ---------------------------------------------------------------------------------------------------------------------
# 2. frequencies and modes
# ---------------------------------------------------------------------------------------------------------------------
def test_frequencies_and_modes_against_the_dense_solution(dcase):
    """omega^2 within 1e-6 of scipy.linalg.eigh on the handle's own K and the restated M, residuals <= 1e-4,
    M-orthonormality within 1e-8 (the bounds of DESIGN.md section 10d)."""
    d = dcase
    k = N_DENSE[d.name]
    out = d.dev.vibration_modes(k, n_sub=12)
    assert out["n_found"] == k
    rel = np.abs(out["omega2"] / d.om2 - 1.0).max()
    V = out["modes"].reshape(k, -1)
    orth = np.abs(V @ (d.M @ V.T) - np.eye(k)).max()
    print(f"\n{d.name}: omega^2 {out['omega2']}, {out['outer_iterations']} outer steps, relative error {rel:.2e}, "
          f"residual {out['residual'].max():.2e}, M-orthonormality {orth:.2e}")
    assert rel <= 1e-6
    assert out["residual"].max() <= 1e-4
    assert orth <= 1e-8
    assert not V[:, d.c.fixed.reshape(-1)].any()
    assert all(v[np.argmax(np.abs(v))] > 0 for v in V)
    # the residual is what it says, on the free dofs
    free = ~d.c.fixed.reshape(-1)
    for j in range(k):
        kp, mp = (d.K @ V[j])[free], (d.M @ V[j])[free]
        assert abs(np.linalg.norm(kp - out["omega2"][j] * mp) / np.linalg.norm(kp) - out["residual"][j]) <= 1e-9


def test_modes_only_and_max_outer(case_a):
    dev, lib, p = case_a.dev, _capi.load_library(), _capi._ptr
    om2 = np.empty(2)
    found, outer = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.pl_vibration_modes(dev._h, 2, 8, 1e-10, 100000, 1e-9, 200, p(om2), None, None, p(found), p(outer))
    assert rc == _capi.PL_OK and found[0] == 2
    assert np.abs(om2 / case_a.om2[:2] - 1.0).max() <= 1e-6
    rc = lib.pl_vibration_modes(dev._h, 2, 8, 1e-10, 100000, 1e-14, 1, p(om2), None, None, p(found), p(outer))
    assert rc == _capi.PL_ERR_NOCONV and outer[0] == 1
    assert b"max_outer" in lib.pl_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the sensitivity kernel, with exact eigenpairs
# ---------------------------------------------------------------------------------------------------------------------
def test_sensitivity_parity_with_the_restatement(dcase):
    """Rows on dense eigenpairs within 1e-12 of max|row| of the restatement: per-strut fp64 arithmetic with no solve."""
    d = dcase
    for k in (1, 2, len(d.om2)):
        rows = d.dev.vibration_modes_sens(d.om2[:k], d.modes[:k])["domega2_dr"]
        err = np.abs(rows - d.rows[:k]).max(axis=1) / np.abs(d.rows[:k]).max(axis=1)
        print(f"\n{d.name}, {k} mode(s): rows within {err.max():.2e} of max|row|")
        assert err.max() <= 1e-12


def test_weighted_sum_scaling_and_skipped_modes(case_a):
    d = case_a
    k = len(d.om2)
    wts = np.array([0.7, -1.3, 2.0, 0.4])[:k]
    out = d.dev.vibration_modes_sens(d.om2, d.modes, weights=wts)
    ref = wts @ out["domega2_dr"]
    assert np.abs(out["dsum_dr"] - ref).max() <= 1e-13 * np.abs(ref).max()
    only = d.dev.vibration_modes_sens(d.om2, d.modes, weights=wts, want_rows=False)
    assert sorted(only) == ["dsum_dr"] and np.array_equal(only["dsum_dr"], out["dsum_dr"])
    # a mode scaled by 3 keeps its row
    modes = d.modes.copy()
    modes[1] *= 3.0
    scaled = d.dev.vibration_modes_sens(d.om2, modes)["domega2_dr"]
    assert np.abs(scaled - out["domega2_dr"]).max(axis=1).max() <= 1e-12 * np.abs(out["domega2_dr"]).max()
    # a NaN omega^2 marks a mode to skip: a NaN row, nothing in the sum
    om2 = d.om2.copy()
    om2[2] = np.nan
    skip = d.dev.vibration_modes_sens(om2, d.modes, weights=wts)
    assert np.isnan(skip["domega2_dr"][2]).all()
    keep = [0, 1, 3]
    assert np.array_equal(skip["domega2_dr"][keep], out["domega2_dr"][keep])
    ref = wts[keep] @ out["domega2_dr"][keep]
    assert np.abs(skip["dsum_dr"] - ref).max() <= 1e-13 * np.abs(ref).max()
    none = d.dev.vibration_modes_sens(np.full(2, np.nan), d.modes[:2], weights=np.ones(2))
    assert np.isnan(none["domega2_dr"]).all() and not none["dsum_dr"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_differences_of_the_devices_own_frequencies(case_a):
    """vibration_modes(4, n_sub = 12), then vibration_modes_sens: domega2_dr @ dr within 1e-3 relative of the central
    difference of the DEVICE's omega^2 at r +- 1e-4 dr, dr = U(-1, 1) r (as DESIGN.md section 10d)."""
    c = case_a.c
    with _device(c) as dev:
        out = dev.vibration_modes(4, n_sub=12)
        rows = dev.vibration_modes_sens(out["omega2"], out["modes"])["domega2_dr"]
        err = (np.abs(rows - case_a.rows).max(axis=1) / np.abs(case_a.rows).max(axis=1)).max()
        dr = np.random.default_rng(11).uniform(-1.0, 1.0, c.B) * c.radius
        om2 = []
        for sign in (1.0, -1.0):
            dev.update_radii(c.radius + sign * 1e-4 * dr)
            dev.assemble()
            om2.append(dev.vibration_modes(4, n_sub=12)["omega2"])
        fd = (om2[0] - om2[1]) / 2e-4
        got = rows @ dr
        rel = np.abs(got / fd - 1.0)
        print(f"\nend to end: rows {err:.2e} of max|row| from the restatement on dense modes; directional derivative {got}, "
              f"difference quotient {fd}, relative difference {rel}")
        assert err <= 1e-3
        assert rel.max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 5. the handle's state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_solve_after_the_calls_returns_the_same_bits(case_a):
    """As tests/test_gpu_buckling_sens.py: the per-node gather product and the Jacobi preconditioner sum in a fixed order, and
    the second solve of a handle is compared with the second solve of a twin that made no call in between."""
    c = case_a.c
    f = np.zeros((c.n, 6))
    f[c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9, 0] = 0.01
    fixed_order = dict(spmv_kernel=2, precond=1)
    with _device(c, **fixed_order) as dev, _device(c, **fixed_order) as twin:
        for d in (dev, twin):
            d.set_bc(c.fixed, None, f)
        first = [d.solve(rtol=1e-12, max_iter=100000)[0] for d in (dev, twin)]
        assert np.array_equal(first[0], first[1]) and np.abs(first[0]).max() > 0
        out = dev.vibration_modes(4, n_sub=8)
        dev.vibration_modes_sens(out["omega2"], out["modes"], weights=np.ones(4))
        dev.mass_spmv_multi(out["modes"], masked=True)
        again = [d.solve(rtol=1e-12, max_iter=100000) for d in (dev, twin)]
        assert np.array_equal(again[0][0], again[1][0])
        assert again[0][1]["iterations"] == again[1][1]["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. error codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = case("A")
    lib, p = _capi.load_library(), _capi._ptr
    n6 = 6 * c.n
    OK, ARG, STATE = _capi.PL_OK, _capi.PL_ERR_ARG, _capi.PL_ERR_STATE
    x = np.ascontiguousarray(np.random.default_rng(1).standard_normal((2, n6)))
    y = np.empty_like(x)
    om2 = np.array([1.5, 1.7])
    wts = np.ones(2)
    rows, dsum = np.empty((17, c.B)), np.empty(c.B)
    o2, modes, res = np.empty(4), np.empty((4, n6)), np.empty(4)
    found, outer = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def spmv(h, n=2, masked=0, x_=x, y_=y):
        return lib.pl_mass_spmv_multi(h, n, masked, p(x_), p(y_))

    def vib(h, n=4, n_sub=8, rtol=1e-10, it=100000, tol=1e-9, mo=200, o2_=o2, found_=found, outer_=outer):
        return lib.pl_vibration_modes(h, n, n_sub, rtol, it, tol, mo, p(o2_), p(modes), p(res), p(found_), p(outer_))

    def sens(h, n=2, om2_=om2, phi_=x, wts_=None, rows_=rows, dsum_=None):
        return lib.pl_vibration_modes_sens(h, n, p(om2_), p(phi_), p(wts_), p(rows_), p(dsum_))

    assert lib.pl_set_mass(None, 1.0, 1, None) == ARG
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN) as dev:
        h = dev._h
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.pl_set_mass(h, bad, 1, None) == ARG
        assert b"density" in lib.pl_last_error()
        assert lib.pl_set_mass(h, 1.0, 2, None) == ARG
        nm = np.zeros(c.n)
        nm[3] = -1e-9
        assert lib.pl_set_mass(h, 1.0, 1, p(nm)) == ARG
        assert b"node_mass" in lib.pl_last_error()
        assert spmv(h) == STATE and vib(h) == STATE and sens(h) == STATE          # before pl_assemble
        dev.assemble()
        assert spmv(h) == STATE                                                    # before pl_set_mass
        assert b"pl_set_mass" in lib.pl_last_error()
        assert lib.pl_set_mass(h, RHO, 1, None) == OK
        assert spmv(h) == OK
        assert spmv(h, masked=1) == STATE and vib(h) == STATE and sens(h) == STATE # before pl_set_bc
        assert b"pl_set_bc" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert spmv(h, masked=1) == OK
        assert spmv(h, n=0) == ARG and spmv(h, n=_capi.MULTI_MAX + 1) == ARG
        assert spmv(h, x_=None) == ARG and spmv(h, y_=None) == ARG
        assert vib(h, n=0) == ARG and vib(h, n=5) == ARG                           # n_modes 1 ... n_sub / 2
        assert vib(h, n_sub=6) == ARG and vib(h, n_sub=36) == ARG
        assert vib(h, rtol=0.0) == ARG and vib(h, it=0) == ARG and vib(h, tol=0.0) == ARG and vib(h, mo=0) == ARG
        assert vib(h, o2_=None) == ARG and vib(h, found_=None) == ARG and vib(h, outer_=None) == ARG
        assert vib(h) == OK and found[0] == 4
        assert sens(h, n=0) == ARG
        assert sens(h, n=17, om2_=np.full(17, 1.5), phi_=np.zeros((17, n6))) == ARG
        assert sens(h, rows_=None) == ARG                                          # both outputs NULL
        assert sens(h, dsum_=dsum) == ARG                                          # dsum_dr without weights
        assert b"weights" in lib.pl_last_error()
        assert sens(h, om2_=None) == ARG and sens(h, phi_=None) == ARG
        assert sens(h) == OK
        assert sens(h, rows_=None, dsum_=dsum, wts_=wts) == OK
        master = np.arange(c.n, dtype=np.int32)
        master[c.n - 1] = c.n - 2
        dev.set_periodic(master)
        assert spmv(h) == STATE and vib(h) == STATE and sens(h) == STATE
        assert b"periodic" in lib.pl_last_error()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        assert lib.pl_set_mass(ddm._h, 1.0, 1, None) == STATE
        x12 = np.ones((2, 12))
        assert lib.pl_mass_spmv_multi(ddm._h, 2, 0, p(x12), p(np.empty((2, 12)))) == STATE
        assert vib(ddm._h) == STATE
        assert lib.pl_vibration_modes_sens(ddm._h, 2, p(om2), p(x12), None, p(np.empty((2, 1))), None) == STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            m6 = 6 * dev.n_nodes
            assert lib.pl_set_mass(dev._h, 1.0, 1, None) == STATE
            assert b"multi-rank" in lib.pl_last_error()
            assert lib.pl_mass_spmv_multi(dev._h, 2, 0, p(np.ones((2, m6))), p(np.empty((2, m6)))) == STATE
            assert vib(dev._h) == STATE
            assert lib.pl_vibration_modes_sens(dev._h, 2, p(om2), p(np.ones((2, m6))), None, p(np.empty((2, dev.n_beams))),
                                               None) == STATE


# ---------------------------------------------------------------------------------------------------------------------
# 7. LatticeSim and LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_sim_natural_frequencies():
    L = LatticeSim(_preset("BCC", (2, 2, 3)))
    with pytest.raises(RuntimeError):
        L.natural_frequencies()
    solve_FEM_FenicsX(L, rtol=1e-10)
    with pytest.raises(RuntimeError):
        L.natural_frequency_sensitivity()
    n = L.lattice.n_nodes
    nm = np.where(L.lattice.node_xyz[:, 2] > 2.5, 0.01, 0.0)
    out = L.natural_frequencies(5, density=RHO, node_mass=nm, n_sub=12)
    dev = L._device
    fixed = np.asarray(L.fixed_DOF).reshape(n, 6) != 0
    ref = MH.vibration_modes_dense(_bsr(dev), dev.mass_matrix_host(), fixed, 5)
    assert out["n_found"] == 5
    assert np.abs(L.vibration_omega2 / ref["omega2"] - 1.0).max() <= 1e-6
    assert np.abs(L.natural_frequencies_hz / (np.sqrt(ref["omega2"]) / (2 * np.pi)) - 1.0).max() <= 1e-6
    assert L.vibration_modes.shape == (5, n, 6) and np.array_equal(out["frequency"], L.natural_frequencies_hz)
    sens = L.natural_frequency_sensitivity(p=8)
    nb = L.lattice.n_beams
    assert sorted(sens) == ["aggregate", "dJ_dr", "domega2_dr"]
    assert sens["dJ_dr"].shape == (nb,) and sens["domega2_dr"].shape == (5, nb)
    J, wts = GH.load_factor_aggregate(L.vibration_omega2, 8)
    assert sens["aggregate"] == J >= 1.0 / L.vibration_omega2[0]
    ref = wts @ sens["domega2_dr"]
    assert np.abs(sens["dJ_dr"] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert sorted(L.natural_frequency_sensitivity(want_rows=False)) == ["aggregate", "dJ_dr"]


OPTI = _preset("BCC", (2, 2, 3))
OPTI["optimization_informations"] = {
    "objective_function": "min", "objective_type": "compliance", "max_iterations": 4,
    "optimization_parameters": {"type": "linear", "direction": ["x", "z"]},
    "constraints": {"relative_density": {"value": 0.2}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}
# three modes: the (nearly) double first frequency and the simple third - whole clusters
FREQ = {"value": 0.05, "density": RHO, "n_modes": 3, "p": 8, "n_sub": 12}


def _opti(constraints, **opt):
    p = copy.deepcopy(OPTI)
    p["optimization_informations"].update(opt)
    p["optimization_informations"]["constraints"].update(constraints)
    return p


def test_frequency_constraint_gradient():
    """frequency_constraint_gradient against central differences of frequency_constraint in the three variables of the
    linear parameterisation, step 1e-4, within 1e-3 relative."""
    L = LatticeOpti(_opti({"frequency": FREQ}))
    assert "min_frequency" in L._history
    theta = [0.2, -0.1, 0.5]
    L.objective(theta)
    g = L.frequency_constraint_gradient(theta)
    assert g.shape == (L.number_parameters,) == (3,) and np.abs(g).max() > 0
    J, f1 = L._last_frequency
    assert abs((2 * np.pi * FREQ["value"]) ** 2 * J - 1.0 - L.frequency_constraint(theta)) <= 1e-8
    assert J >= 1.0 / (2 * np.pi * f1) ** 2
    h = 1e-4
    for i in range(3):
        tp, tm = list(theta), list(theta)
        tp[i] += h
        tm[i] -= h
        fd = (L.frequency_constraint(tp) - L.frequency_constraint(tm)) / (2 * h)
        print(f"\nvariable {i}: gradient {g[i]:.8e}, difference quotient {fd:.8e}, relative difference {abs(g[i] / fd - 1):.2e}")
        assert abs(g[i] - fd) <= 1e-3 * abs(fd), (i, g[i], fd)
    assert "min_frequency" not in LatticeOpti(_opti({}))._history


def test_ddm_mode_refuses_the_key():
    p = _opti({"frequency": FREQ}, simulation_type="DDM")
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError, match="frequency"):
        LatticeOpti(p)
