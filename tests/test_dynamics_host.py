"""The numpy / scipy restatement of the transient response (dynamics_host.py) on the lattices of tests/test_mass_host.py: a
single mode against the scheme's exact phase, the energy identities, the step-load response against the static solution, the
Jacobi-PCG variant against the dense solves, and the argument checks.  No device.

beta = 1/4, gamma = 1/2, dt = T_1 / 40, 200 steps.  Measured: single-mode deviation 6.7e-12 / 5.7e-12 / 1.2e-12 of max|phi_1|
on A / B / C (bar 1e-9), energy drift <= 1.9e-13 (bar 1e-10), kinetic + strain - W <= 7.6e-15 of the energy (bar 1e-10),
peak / static displacement in the direction of the load 1.85 - 1.87; Jacobi-PCG solves within 7.5e-12 of the Cholesky ones."""
import numpy as np
import pytest
import scipy.linalg

from pylatticedso_amd import dynamics_host as DH

from test_mass_host import case

N_STEPS = 200


class _Dyn:
    """K, M, the dense eigenpairs on the free dofs and the static solution of one lattice: computed once, left unchanged."""

    def __init__(self, name):
        c = case(name)
        self.name, self.c, self.K, self.M = name, c, c.K(), c.M()
        self.fixed = c.fixed.reshape(-1)
        self.free = np.flatnonzero(~self.fixed)
        Kf = self.K[self.free][:, self.free].toarray() if hasattr(self.K, "toarray") else np.asarray(self.K)[np.ix_(self.free, self.free)]
        Mf = self.M[self.free][:, self.free].toarray() if hasattr(self.M, "toarray") else np.asarray(self.M)[np.ix_(self.free, self.free)]
        self.Kf, self.Mf = Kf, Mf
        self.om2, self.phi = scipy.linalg.eigh(Kf, Mf)
        self.dt = 2.0 * np.pi / np.sqrt(self.om2[0]) / 40.0
        self.n6 = self.fixed.size
        top = c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9
        f = np.zeros((c.n, 6))
        f[top, 0], f[top, 2] = 0.03, -0.1               # the top face pushed sideways and down
        self.load = np.where(c.fixed, 0.0, f).reshape(-1)
        self.u_static = np.zeros(self.n6)
        self.u_static[self.free] = np.linalg.solve(Kf, self.load[self.free])

    def full(self, x):
        out = np.zeros(self.n6)
        out[self.free] = x
        return out


_dyn = {}


@pytest.fixture(scope="module", params=["A", "B", "C"])
def dyn(request):
    if request.param not in _dyn:
        _dyn[request.param] = _Dyn(request.param)
    return _dyn[request.param]


def test_newmark_phase():
    assert DH.newmark_phase(0.0, 0.1) == 0.0
    assert abs(DH.newmark_phase(2.0, 1.0) - np.pi / 2) <= 1e-15
    assert np.allclose(DH.newmark_phase(np.array([1.0, 3.0]), 0.2), 2 * np.arctan([0.1, 0.3]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("mode", [0, -1])
def test_a_single_mode_keeps_its_shape_and_turns_by_the_exact_phase(dyn, mode):
    """u0 = phi, v0 = 0, no load, no damping: u_n = phi cos(n theta), theta = 2 atan(omega dt / 2), exactly."""
    phi, om = dyn.full(dyn.phi[:, mode]), np.sqrt(dyn.om2[mode])
    out = DH.newmark(dyn.K, dyn.M, dyn.fixed, dyn.dt, N_STEPS, u0=phi)
    th = DH.newmark_phase(om, dyn.dt)
    want = np.cos(th * np.arange(N_STEPS + 1))[:, None] * phi[None, :]
    err = np.abs(out["u"].reshape(N_STEPS + 1, -1) - want).max() / np.abs(phi).max()
    print(f"\n{dyn.name} mode {mode}: omega^2 = {dyn.om2[mode]:.4g}, deviation {err:.2e}")
    assert err <= 1e-9
    assert not out["u"].reshape(N_STEPS + 1, -1)[:, dyn.fixed].any()


def test_free_vibration_keeps_its_energy(dyn):
    rng = np.random.default_rng(3)
    u0 = dyn.full(dyn.phi[:, :6] @ rng.standard_normal(6))
    v0 = dyn.full(dyn.phi[:, :6] @ (np.sqrt(dyn.om2[:6]) * rng.standard_normal(6)))
    out = DH.newmark(dyn.K, dyn.M, dyn.fixed, dyn.dt, N_STEPS, u0=u0, v0=v0)
    tot = out["energy"][:, 0] + out["energy"][:, 1]
    assert tot[0] > 0 and not out["energy"][:, 2].any()
    assert np.abs(tot / tot[0] - 1.0).max() <= 1e-10


def test_step_load_energy_balance_and_amplification(dyn):
    amp = np.ones((N_STEPS + 1, 1))
    out = DH.newmark(dyn.K, dyn.M, dyn.fixed, dyn.dt, N_STEPS, dyn.load[None], amp)
    e = out["energy"]
    assert np.abs(e[:, 0] + e[:, 1] - e[:, 2]).max() <= 1e-10 * e[:, 1].max()
    # peak displacement in the direction of the load, f.u, between 1 and 2 times the static one: with K u_s = f and
    # 1/2 u.K u <= W = f.u, the distance w = u - u_s has |w|_K <= |u_s|_K, so f.u = f.u_s + u_s.K w <= 2 f.u_s (one dof
    # alone may pass 2 when several modes meet)
    ratio = (out["u"].reshape(N_STEPS + 1, -1) @ dyn.load).max() / float(dyn.load @ dyn.u_static)
    print(f"\npeak / static = {ratio:.3f}")
    assert 1.0 < ratio < 2.0
    # the state and the probe rows are views of the same history
    assert np.array_equal(out["state"][0], out["u"][-1]) and np.array_equal(out["state"][2], out["a"][-1])
    pr = DH.newmark(dyn.K, dyn.M, dyn.fixed, dyn.dt, 5, dyn.load[None], amp[:6], probes=[3, 1], snap_every=2)
    assert pr["probe"].shape == (6, 3, 2, 6) and np.array_equal(pr["probe"][:, 1, 0], pr["v"][:, 3])
    assert pr["snaps"].shape == (2, dyn.c.n, 6) and np.array_equal(pr["snaps"][1], pr["u"][4])


def test_rayleigh_damping_dissipates_and_settles_on_the_static_solution(dyn):
    w1 = np.sqrt(dyn.om2[0])
    amp = np.ones((N_STEPS + 1, 1))
    out = DH.newmark(dyn.K, dyn.M, dyn.fixed, dyn.dt, N_STEPS, dyn.load[None], amp, ray_m=0.05 * w1, ray_k=0.002 / w1)
    e = out["energy"]
    bal = e[:, 0] + e[:, 1] - e[:, 2]
    assert np.diff(bal).max() <= 1e-12 * e[:, 1].max()        # what the damper takes never comes back
    # the energy of the distance to the static solution falls monotonically
    d = out["u"].reshape(N_STEPS + 1, -1)[:, dyn.free] - dyn.u_static[dyn.free]
    v = out["v"].reshape(N_STEPS + 1, -1)[:, dyn.free]
    dist = 0.5 * np.einsum("ni,ij,nj->n", d, dyn.Kf, d) + 0.5 * np.einsum("ni,ij,nj->n", v, dyn.Mf, v)
    assert np.diff(dist).max() <= 1e-12 * dist[0] and dist[-1] < dist[0]


def test_jacobi_pcg_solves_reproduce_the_dense_solves():
    """The yardstick of the device check: the restatement against itself with a host Jacobi PCG at rtol = 1e-12."""
    d = _dyn.setdefault("A", None) or _Dyn("A")
    _dyn["A"] = d
    amp = np.ones((N_STEPS + 1, 1))
    ref = DH.newmark(d.K, d.M, d.fixed, d.dt, N_STEPS, d.load[None], amp)
    counts = []
    got = DH.newmark(d.K, d.M, d.fixed, d.dt, N_STEPS, d.load[None], amp, solve=DH.jacobi_pcg(1e-12, counts=counts))
    err = np.abs(got["u"] - ref["u"]).max() / np.abs(ref["u"]).max()
    print(f"\nhost PCG vs Cholesky: {err:.2e} of max|u|, iterations {min(counts)} - {max(counts)}")
    assert err <= 1e-9 and len(counts) == N_STEPS + 1


def test_argument_checks():
    K = M = np.eye(6)
    fixed = np.zeros(6, bool)
    ok = dict(dt=0.1, n_steps=2)
    DH.newmark(K, M, fixed, **ok)
    for bad in (dict(dt=0.0), dict(dt=-1.0), dict(n_steps=0), dict(gamma=0.4), dict(beta=0.2), dict(gamma=0.6, beta=0.3),
                dict(ray_m=-1.0), dict(ray_k=-1e-3)):
        with pytest.raises(ValueError):
            DH.newmark(K, M, fixed, **{**ok, **bad})
    DH.newmark(K, M, fixed, gamma=0.6, beta=0.31, **ok)         # just inside the stability limit 0.3025
