"""The numpy / scipy restatement of the transient sensitivities (dynamics_host.newmark_sensitivity): the
discrete adjoint of the Newmark scheme against central differences of ``newmark`` in every radius of lattices A and C, the
exact structure of the backward sweep, and its Jacobi-PCG variant against the Cholesky one.  No device.

The lattices are those of tests/test_mass_host.py; dt = T_1 / 40 from the dense eigen-solution, 40 steps, a step load on the
top face plus a half-sine base acceleration, a non-zero u0.  Central differences: h = 1e-6 and 1e-5 of the largest |FD| entry,
the step and bar of the frequency rows in tests/test_mass_host.py."""
import numpy as np
import pytest
import scipy.linalg

from pylatticedso_amd import dynamics_host as DH
from pylatticedso_amd import geometric_host as GH
from pylatticedso_amd import mass_host as MH

from test_mass_host import RHO, case

N_STEPS = 40
SCHEMES = {"damped": (0.25, 0.5, True), "undamped": (0.25, 0.5, False), "general": (0.31, 0.6, True)}


class _Setup:
    """One lattice with its loads, output vector and time step: computed once, shared by the tests, left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        c = self.c
        self.K, self.M = c.K(), c.M()
        self.free = GH._free(c.fixed, 6 * c.n)
        Kf, Mf = self.K[self.free][:, self.free].toarray(), self.M[self.free][:, self.free].toarray()
        om2, phi = scipy.linalg.eigh(Kf, Mf, subset_by_index=[0, 0])
        self.w1 = float(np.sqrt(om2[0]))
        self.dt = 2.0 * np.pi / self.w1 / 40.0
        top = np.flatnonzero(c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9)
        f = np.zeros((c.n, 6))
        f[top, 0], f[top, 2] = 0.03, -0.1
        self.load = np.where(c.fixed, 0.0, f)
        u_static = np.linalg.solve(Kf, self.load.reshape(-1)[self.free])
        self.u0 = np.zeros(6 * c.n)
        self.u0[self.free] = 0.3 * np.abs(u_static).max() / np.abs(phi[:, 0]).max() * phi[:, 0]
        self.v0 = np.zeros(6 * c.n)
        self.v0[self.free] = 0.2 * self.w1 * u_static
        rng = np.random.default_rng(7)
        self.l = (rng.standard_normal((c.n, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])).reshape(-1)
        self.base_dir = np.array([0.6, 0.0, 0.8])
        self.d = c.xyz[c.conn[:, 1]] - c.xyz[c.conn[:, 0]]
        self.drec = c.drec()
        self.dM = MH.delement_matrix_dr(self.d, c.radius, RHO, c.mult, True)

    def base_acc(self, n_steps):
        t = self.dt * np.arange(n_steps + 1)
        return np.where(t < 20 * self.dt, 0.4 * np.sin(np.pi * t / (20 * self.dt)), 0.0)

    def scheme(self, which):
        beta, gamma, damped = SCHEMES[which]
        rm, rk = (0.05 * self.w1, 0.002 / self.w1) if damped else (0.0, 0.0)
        return dict(beta=beta, gamma=gamma, ray_m=rm, ray_k=rk)

    def sens(self, kind, which="damped", n_steps=N_STEPS, weight=None, p=8.0, solve=None, v0=False, base=True):
        return DH.newmark_sensitivity(self.K, self.M, self.c.fixed, self.c.conn, self.drec, self.dM, self.dt, n_steps, self.l,
                                      kind, p, weight, self.load[None], np.ones((n_steps + 1, 1)),
                                      self.base_dir if base else None, self.base_acc(n_steps) if base else None, self.u0,
                                      self.v0 if v0 else None, solve=solve, **self.scheme(which))

    def outputs(self, radius, which, v0):
        """y (N_STEPS + 1,) of ``newmark`` at the radii ``radius``: the base load follows M."""
        c = self.c
        K, M = c.K(radius), c.M(radius)
        e = np.zeros((c.n, 6))
        e[:, :3] = self.base_dir
        pats = np.stack([self.load.reshape(-1), -(M @ e.reshape(-1))])
        amp = np.column_stack([np.ones(N_STEPS + 1), self.base_acc(N_STEPS)])
        out = DH.newmark(K, M, c.fixed, self.dt, N_STEPS, pats, amp, self.u0, self.v0 if v0 else None, **self.scheme(which))
        return out["u"].reshape(N_STEPS + 1, -1) @ np.where(c.fixed.reshape(-1), 0.0, self.l)


_setups = {}


def _setup(name):
    if name not in _setups:
        _setups[name] = _Setup(name)
    return _setups[name]


@pytest.mark.parametrize("name,which", [("A", "damped"), ("A", "undamped"), ("A", "general"), ("C", "damped"), ("C", "undamped")])
def test_gradient_agrees_with_central_differences(name, which):
    """Every radius, all three kinds (kind 2 with p = 8), h = 1e-6, within 1e-5 of the largest |FD| entry.  Measured: at most
    8.3e-8 (A) and 1.1e-9 (C)."""
    s = _setup(name)
    c = s.c
    v0 = which == "general"
    h = 1e-6
    wts = 0.5 + np.random.default_rng(3).random(N_STEPS + 1)
    cases = [(0, wts, 8.0), (1, wts, 8.0), (2, None, 8.0)]
    fd = np.zeros((3, c.B))
    for b in range(c.B):
        Jpm = []
        for sg in (+1.0, -1.0):
            r = c.radius.copy()
            r[b] += sg * h
            y = s.outputs(r, which, v0)
            Jpm.append([DH.objective(y, k, p, w)[0] for k, w, p in cases])
        fd[:, b] = (np.array(Jpm[0]) - np.array(Jpm[1])) / (2.0 * h)
    for i, (k, w, p) in enumerate(cases):
        got = s.sens(k, which, weight=w, p=p, v0=v0)
        assert got["y"].shape == (N_STEPS + 1,) and got["dJ_dr"].shape == (c.B,) and got["lam"].shape == (N_STEPS + 1, c.n, 6)
        assert not got["lam"][:, c.fixed].any()
        err = np.abs(got["dJ_dr"] - fd[i]).max() / np.abs(fd[i]).max()
        print(f"{name} {which} kind {k}: J = {got['J']:.6e}, gradient within {err:.2e} of the largest central difference")
        assert np.abs(fd[i]).max() > 0 and err <= 1e-5


@pytest.mark.parametrize("name", ["A", "C"])
def test_exact_structure_of_the_backward_sweep(name):
    s = _setup(name)
    B = s.c.B
    # weights on row 0 alone: y_0 = l . u_0 does not follow the design
    w0 = np.zeros(N_STEPS + 1)
    w0[0] = 1.0
    for kind in (0, 1, 2):
        g = s.sens(kind, weight=w0)
        assert g["J"] != 0.0 and not g["dJ_dr"].any() and not g["lam"].any()
    # weights on row k alone: the rows after k do not matter
    k = 17
    for kind in (0, 1, 2):
        wk = np.zeros(k + 1)
        wk[k] = 1.0
        short = s.sens(kind, n_steps=k, weight=wk)
        long_ = s.sens(kind, n_steps=k + 10, weight=np.concatenate([wk, np.zeros(10)]))
        assert short["J"] == pytest.approx(long_["J"], rel=1e-13)
        assert np.abs(short["dJ_dr"] - long_["dJ_dr"]).max() <= 1e-12 * np.abs(short["dJ_dr"]).max()
        assert not long_["lam"][k + 1:].any()
    # kind 0 is linear in the weights
    rng = np.random.default_rng(5)
    wa, wb = rng.random(N_STEPS + 1), rng.random(N_STEPS + 1)
    ga, gb, gab = (s.sens(0, weight=w)["dJ_dr"] for w in (wa, wb, wa + 2.0 * wb))
    assert np.abs(gab - ga - 2.0 * gb).max() <= 1e-12 * np.abs(gab).max()
    # the 2-norm: d sqrt(sum y^2) = d(1/2 sum y^2) / sqrt(sum y^2)
    g2, g1 = s.sens(2, p=2.0), s.sens(1)
    assert g2["J"] == pytest.approx(np.sqrt(2.0 * g1["J"]), rel=1e-14)
    assert np.abs(g2["dJ_dr"] - g1["dJ_dr"] / g2["J"]).max() <= 1e-12 * np.abs(g2["dJ_dr"]).max()
    assert g2["dJ_dr"].shape == (B,)
    with pytest.raises(ValueError):
        s.sens(3)
    with pytest.raises(ValueError):
        s.sens(2, p=1.5)
    with pytest.raises(ValueError):
        s.sens(0, weight=-np.ones(N_STEPS + 1))


# measured distance of the Jacobi-PCG variant (rtol = 1e-12) from the Cholesky variant, relative to the largest magnitude of
# each quantity, over A and C, damped and undamped, all kinds: J 1.9e-12, y 5.2e-12, dJ_dr 4.6e-11; the bars are ten times
# that
PCG_BAR = {"J": 1.9e-11, "y": 5.2e-11, "dJ_dr": 4.6e-10}


@pytest.mark.parametrize("name", ["A", "C"])
@pytest.mark.parametrize("which", ["damped", "undamped"])
def test_jacobi_pcg_variant_against_cholesky(name, which):
    s = _setup(name)
    worst = {q: 0.0 for q in PCG_BAR}
    for kind in (0, 1, 2):
        counts = []
        ref = s.sens(kind, which)
        got = s.sens(kind, which, solve=DH.jacobi_pcg(1e-12, counts=counts))
        assert len(counts) == 2 * (N_STEPS + 1)
        for q in worst:
            scale = np.abs(ref[q]).max()
            worst[q] = max(worst[q], float(np.abs(got[q] - ref[q]).max() / scale))
    print(f"{name} {which}: Jacobi PCG at 1e-12 against Cholesky: {worst}")
    for q, bar in PCG_BAR.items():
        assert worst[q] <= bar, (q, worst[q])
