"""The numpy / scipy restatement of the frequency-response sensitivities (dynamics_host.harmonic_sensitivity; DESIGN.md section
10j): the adjoint gradient against central differences of ``harmonic`` in every radius of lattices A and C, the exact structure
of the formulas, the COCG variant against the dense one, and the argument checks.  No device.

The lattices are those of tests/test_mass_host.py; the frequencies W = {0, 0.5 w_1, 0.98 w_1, mid(w_1, w_3), mid(w_6, w_7),
mid(w_20, w_21)}, the damping D = (0.05 w_1, 0.002 / w_1) and the top-face load are those of tests/test_gpu_harmonic.py (w_i
from the dense eigen-solution of the restated K and M), l is the generic vector of tests/test_dynamics_sens_host.py, base_dir =
(0.6, 0, 0.8).  Central differences: h = 1e-6 and 1e-5 of the largest |FD| entry, the step and bar of section 10h."""
import numpy as np
import pytest
import scipy.linalg

from pylatticedso_amd import dynamics_host as DH
from pylatticedso_amd import geometric_host as GH
from pylatticedso_amd import mass_host as MH

from test_mass_host import RHO, case

BASE_DIR = np.array([0.6, 0.0, 0.8])
# (load, base, out_vec): dead load; shaken base; out_vec = None without and with a base
CASES = {"dead": (True, False, True), "base": (True, True, True), "self": (True, False, False), "self_base": (True, True, False)}


class _Setup:
    """One lattice with its frequencies, load and output vector: computed once, shared by the tests, left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        c = self.c
        self.K, self.M = c.K(), c.M()
        self.free = GH._free(c.fixed, 6 * c.n)
        Kf, Mf = self.K[self.free][:, self.free].toarray(), self.M[self.free][:, self.free].toarray()
        w = np.sqrt(scipy.linalg.eigh(Kf, Mf, eigvals_only=True))
        self.w = w
        self.W = np.array([0.0, 0.5 * w[0], 0.98 * w[0], 0.5 * (w[0] + w[2]), 0.5 * (w[5] + w[6]), 0.5 * (w[19] + w[20])])
        self.D = (0.05 * w[0], 0.002 / w[0])
        top = np.flatnonzero(c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9)
        f = np.zeros((c.n, 6))
        f[top, 0], f[top, 2] = 0.03, -0.1
        self.load = np.where(c.fixed, 0.0, f).reshape(-1)
        rng = np.random.default_rng(7)
        self.l = (rng.standard_normal((c.n, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])).reshape(-1)
        self.d = c.xyz[c.conn[:, 1]] - c.xyz[c.conn[:, 0]]
        self.drec = c.drec()
        self.dM = MH.delement_matrix_dr(self.d, c.radius, RHO, c.mult, True)
        self.e = np.zeros((c.n, 6))
        self.e[:, :3] = BASE_DIR

    def sens(self, which, kind, omegas=None, weight=None, p=8.0, damping=None, solver=None, load=None):
        has_load, base, has_l = CASES[which]
        rm, rk = self.D if damping is None else damping
        return DH.harmonic_sensitivity(self.K, self.M, self.c.fixed, self.c.conn, self.drec, self.dM,
                                       self.W if omegas is None else omegas, self.load if load is None else load,
                                       self.l if has_l else None, kind, p, weight, BASE_DIR if base else None, rm, rk, solver)

    def outputs(self, K, M):
        """{case: y (n_freq,)} of ``harmonic`` with the matrices K, M: the base load, and with it an l = f, follow M.  The
        cases with the same load share their fields."""
        fx = self.c.fixed.reshape(-1)
        y = {}
        for base in (False, True):
            f = self.load.astype(complex)
            if base:
                f = np.where(fx, 0.0, f - M @ self.e.reshape(-1))
            u = DH.harmonic(K, M, self.c.fixed, self.W, f, *self.D)["u"].reshape(len(self.W), -1)
            for which, (_, b, has_l) in CASES.items():
                if b == base:
                    y[which] = u @ (np.where(fx, 0.0, self.l) if has_l else f)
        return y


_setups = {}


def _setup(name):
    if name not in _setups:
        _setups[name] = _Setup(name)
    return _setups[name]


@pytest.mark.parametrize("name", ["A", "C"])
def test_gradient_agrees_with_central_differences(name):
    """Every radius, all three kinds (kind 2 with p = 8), dead load, shaken base, out_vec = None without and with a base:
    h = 1e-6, within 1e-5 of the largest |FD| entry.  Measured: at most 2.9e-8 on A (1.75e-7 for out_vec = None with a base,
    which passes only with the doubled dM e_dir term) and 1.0e-8 on C."""
    s = _setup(name)
    c = s.c
    h = 1e-6
    wts = 0.5 + np.random.default_rng(3).random(len(s.W))
    kinds = [(0, wts, 8.0), (1, wts, 8.0), (2, None, 8.0)]
    fd = {which: np.zeros((3, c.B)) for which in CASES}
    for b in range(c.B):
        Jpm = {which: [] for which in CASES}
        for sg in (+1.0, -1.0):
            r = c.radius.copy()
            r[b] += sg * h
            y = s.outputs(c.K(r), c.M(r))
            for which in CASES:
                Jpm[which].append([DH.harmonic_objective(y[which], k, p, w)[0] for k, w, p in kinds])
        for which in CASES:
            fd[which][:, b] = (np.array(Jpm[which][0]) - np.array(Jpm[which][1])) / (2.0 * h)
    for which in CASES:
        for i, (k, w, p) in enumerate(kinds):
            got = s.sens(which, k, weight=w, p=p)
            assert got["y"].shape == (len(s.W),) and got["dJ_dr"].shape == (c.B,) and got["dy_dr"].shape == (len(s.W), c.B)
            assert got["lam"].shape == (len(s.W), c.n, 6) and not got["lam"][:, c.fixed].any()
            err = np.abs(got["dJ_dr"] - fd[which][i]).max() / np.abs(fd[which][i]).max()
            print(f"{name} {which} kind {k}: J = {got['J']:.6e}, gradient within {err:.2e} of the largest central difference")
            assert np.abs(fd[which][i]).max() > 0 and err <= 1e-5, (which, k, err)


@pytest.mark.parametrize("name", ["A", "C"])
def test_exact_structure(name):
    s = _setup(name)
    nf = len(s.W)
    # a weight on one frequency alone gives the gradient of a call with that frequency alone
    k = 3
    wk = np.zeros(nf)
    wk[k] = 1.0
    for which in ("dead", "self_base"):
        for kind in (0, 1, 2):
            one = s.sens(which, kind, omegas=s.W[k:k + 1])
            alone = s.sens(which, kind, weight=wk)
            assert one["J"] == pytest.approx(alone["J"], rel=1e-13)
            assert np.abs(one["dJ_dr"] - alone["dJ_dr"]).max() <= 1e-12 * np.abs(one["dJ_dr"]).max()
    # kind 0 is linear in the weights
    rng = np.random.default_rng(5)
    wa, wb = rng.random(nf), rng.random(nf)
    ga, gb, gab = (s.sens("base", 0, weight=w)["dJ_dr"] for w in (wa, wb, wa + 2.0 * wb))
    assert np.abs(gab).max() > 0 and np.abs(gab - ga - 2.0 * gb).max() <= 1e-12 * np.abs(gab).max()
    # the 2-norm: d sqrt(sum |y|^2) = d(1/2 sum |y|^2) / sqrt(sum |y|^2)
    g2, g1 = s.sens("base", 2, p=2.0), s.sens("base", 1)
    assert g2["J"] == pytest.approx(np.sqrt(2.0 * g1["J"]), rel=1e-14)
    assert np.abs(g2["dJ_dr"] - g1["dJ_dr"] / g2["J"]).max() <= 1e-12 * np.abs(g2["dJ_dr"]).max()
    # w = 0: the static l^T K^-1 f and its derivative -lam^T dK u
    st = s.sens("dead", 1, omegas=[0.0])
    Kf = s.K[s.free][:, s.free].toarray()
    u, lam = np.zeros(6 * s.c.n), np.zeros(6 * s.c.n)
    u[s.free] = np.linalg.solve(Kf, s.load[s.free])
    lam[s.free] = np.linalg.solve(Kf, s.l[s.free])
    ref = -GH._pairing(s.drec, s.c.conn, u.reshape(-1, 6), lam.reshape(-1, 6))
    assert st["y"][0].imag == 0.0 and st["y"][0].real == pytest.approx(float(s.l[s.free] @ u[s.free]), rel=1e-10)
    assert not st["dy_dr"].imag.any()
    assert np.abs(st["dy_dr"][0].real - ref).max() <= 1e-9 * np.abs(ref).max()
    # undamped below w_1 every y is real and kind 0 gives exact zeros
    und = s.sens("base", 0, omegas=[0.0, 0.3 * s.w[0], 0.5 * s.w[0]], damping=(0.0, 0.0))
    assert np.abs(und["y"].real).min() > 0 and not und["y"].imag.any()
    assert und["J"] == 0.0 and not und["dJ_dr"].any()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_jacobi_cocg_variant_against_dense(name):
    """jacobi_cocg(1e-10, 4000) against the dense solve, relative to each quantity's largest magnitude, within 1e-8 (the bar
    of section 10i), over the four load cases and the three kinds.  Measured: y 1.1e-11, J 2.2e-11, dJ_dr 3.1e-11 at the most;
    iterations 73 ... 380."""
    s = _setup(name)
    worst = {"y": 0.0, "J": 0.0, "dJ_dr": 0.0}
    its = []
    for which in CASES:
        for kind in (0, 1, 2):
            ref = s.sens(which, kind)
            got = s.sens(which, kind, solver=DH.jacobi_cocg(1e-10, 4000))
            assert not got["status"].any()
            rows = 2 if CASES[which][2] else 1
            assert (got["iterations"][:rows] > 0).all() and got["iterations"].max() < 4000
            its.append(got["iterations"][rows - 1])
            for q in worst:
                scale = np.abs(ref[q]).max()
                worst[q] = max(worst[q], float(np.abs(got[q] - ref[q]).max() / scale))
    print(f"{name}: COCG at 1e-10 against dense: {worst}; iterations {np.min(its)} ... {np.max(its)}")
    for q in worst:
        assert worst[q] <= 1e-8, (q, worst[q])


def test_argument_checks():
    s = _setup("A")
    y = np.array([1.0 + 2.0j, -0.5j, 0.0])
    for kind in (0, 1, 2):
        J, g = DH.harmonic_objective(y, kind)
        assert np.isfinite(J) and g.shape == (3,) and g.dtype == complex
    assert DH.harmonic_objective(np.zeros(3), 2)[0] == 0.0 and not DH.harmonic_objective(np.zeros(3), 2)[1].any()
    assert DH.harmonic_objective([1e200 + 1e200j, 1.0], 2, 8.0)[0] == pytest.approx(np.sqrt(2.0) * 1e200, rel=1e-12)
    with pytest.raises(ValueError):
        DH.harmonic_objective(y, 3)
    with pytest.raises(ValueError):
        DH.harmonic_objective(y, 2, 1.5)
    with pytest.raises(ValueError):
        DH.harmonic_objective(y, 0, 8.0, -np.ones(3))
    with pytest.raises(ValueError):
        DH.harmonic_objective(y, 0, 8.0, np.array([1.0, np.inf, 1.0]))
    with pytest.raises(ValueError):
        DH.harmonic_objective(y, 0, 8.0, np.ones(2))
    with pytest.raises(ValueError):
        s.sens("dead", 3)
    with pytest.raises(ValueError):
        s.sens("dead", 2, p=1.0)
    with pytest.raises(ValueError):
        s.sens("dead", 1, omegas=[-1.0])
    with pytest.raises(ValueError):
        s.sens("dead", 1, damping=(-0.1, 0.0))
    with pytest.raises(ValueError):
        s.sens("dead", 1, weight=np.ones(2))
    with pytest.raises(ValueError):
        s.sens("dead", 1, load=np.zeros(5))
    with pytest.raises(ValueError):
        DH.harmonic_sensitivity(s.K, s.M, s.c.fixed, s.c.conn, s.drec, s.dM, s.W, None, s.l)
    with pytest.raises(ValueError):
        DH.harmonic_sensitivity(s.K, s.M, s.c.fixed, s.c.conn, s.drec, s.dM, s.W, s.load, np.zeros(7))
    # no dead load at all is legal with a base
    only_base = DH.harmonic_sensitivity(s.K, s.M, s.c.fixed, s.c.conn, s.drec, s.dM, s.W, None, s.l, 1, base_dir=BASE_DIR,
                                        ray_m=s.D[0], ray_k=s.D[1])
    assert only_base["J"] > 0 and only_base["dJ_dr"].any()
