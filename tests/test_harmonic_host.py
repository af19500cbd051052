"""The numpy / scipy restatement of the frequency response (dynamics_host.harmonic, jacobi_cocg) on the lattices of
tests/test_mass_host.py: the dense solve against the full modal sum, the two power identities, the Jacobi-preconditioned COCG
against the dense solve, the undamped response below the first resonance, the static limit, and the argument checks.  No device.

Frequencies W = {0, 0.5 w_1, 0.98 w_1, mid(w_1, w_3), mid(w_6, w_7), mid(w_20, w_21)}, damping D = (0.05 w_1, 0.002 / w_1), the
top-face load of tests/test_dynamics_host.py.  Measured: dense solve within 6.6e-12 / 5.4e-12 / 1.3e-12 of max|u| of the modal
sum on A / B / C (bar 1e-9), power identities within 6.4e-13 of the larger side (bar 1e-10); COCG at rtol = 1e-10 within
8.2e-11 / 8.8e-12 / 7.6e-11 of the dense solve (bar 1e-8) in 185 - 353 / 106 - 172 / 74 - 165 iterations (bar: half of 4000)."""
import numpy as np
import pytest

from pylatticedso_amd import dynamics_host as DH

from test_dynamics_host import _Dyn


class _Harm(_Dyn):
    """The lattice of _Dyn with the frequencies W, the damping D and the dense solution at them: computed once, left unchanged."""

    def __init__(self, name):
        super().__init__(name)
        w = np.sqrt(self.om2)
        self.w = w
        self.W = np.array([0.0, 0.5 * w[0], 0.98 * w[0], 0.5 * (w[0] + w[2]), 0.5 * (w[5] + w[6]), 0.5 * (w[19] + w[20])])
        self.D = (0.05 * w[0], 0.002 / w[0])
        self.dense = DH.harmonic(self.K, self.M, self.fixed, self.W, self.load, *self.D)

    def modal(self, omega, ray_m, ray_k):
        """sum_i phi_i (phi_i^T f) / (w_i^2 - w^2 + i w (ray_m + ray_k w_i^2)) with all modes (phi^T M phi = 1)"""
        q = self.phi.T @ self.load[self.free]
        den = self.om2 - omega * omega + 1j * omega * (ray_m + ray_k * self.om2)
        out = np.zeros(self.n6, complex)
        out[self.free] = self.phi @ (q / den)
        return out


_harm = {}


@pytest.fixture(scope="module", params=["A", "B", "C"])
def harm(request):
    if request.param not in _harm:
        _harm[request.param] = _Harm(request.param)
    return _harm[request.param]


def test_dense_solve_equals_the_full_modal_sum(harm):
    u = harm.dense["u"].reshape(len(harm.W), -1)
    worst = 0.0
    for k, w in enumerate(harm.W):
        ref = harm.modal(w, *harm.D)
        err = np.abs(u[k] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= 1e-9, (harm.name, k, err)
    assert not u[:, harm.fixed].any()
    print(f"\n{harm.name}: dense solve within {worst:.2e} of the modal sum")


def test_power_identities(harm):
    """Re f^T u = u^H K u - w^2 u^H M u and -Im f^T u = w (ray_m u^H M u + ray_k u^H K u) >= 0."""
    rm, rk = harm.D
    worst = 0.0
    for w, (re, im, uku, umu) in zip(harm.W, harm.dense["power"]):
        a, b = re, uku - w * w * umu
        c, d = -im, w * (rm * umu + rk * uku)
        assert uku > 0 and umu > 0 and d >= 0.0
        for x, y in ((a, b), (c, d)):
            big = max(abs(x), abs(y))                      # the larger side
            worst = max(worst, abs(x - y) / big if big > 0 else 0.0)
            assert abs(x - y) <= 1e-10 * big, (harm.name, w, x, y)
    print(f"\n{harm.name}: power identities within {worst:.2e}")


def test_jacobi_cocg_reproduces_the_dense_solve(harm):
    counts = []
    out = DH.harmonic(harm.K, harm.M, harm.fixed, harm.W, harm.load, *harm.D, solver=DH.jacobi_cocg(1e-10, 4000, counts))
    ref = harm.dense["u"]
    err = [float(np.abs(out["u"][k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(len(harm.W))]
    print(f"\n{harm.name}: COCG iterations {[c[0] for c in counts]}, error against the dense solve {max(err):.2e}")
    assert [c[1] for c in counts] == [0] * len(harm.W)
    assert np.array_equal(out["iterations"], [c[0] for c in counts]) and not out["status"].any()
    assert max(err) <= 1e-8
    assert max(c[0] for c in counts) <= 2000
    scale = np.abs(harm.dense["power"]).max(axis=0)
    assert (np.abs(out["power"] - harm.dense["power"]).max(axis=0) <= 1e-8 * scale).all()


def test_undamped_below_the_first_resonance_is_real_and_zero_frequency_is_static(harm):
    out = DH.harmonic(harm.K, harm.M, harm.fixed, [0.0, 0.5 * harm.w[0]], harm.load)
    assert not out["u"].imag.any() and not out["power"][:, 1].any()
    u0 = out["u"][0].real.reshape(-1)
    assert np.abs(u0 - harm.u_static).max() <= 1e-12 * np.abs(harm.u_static).max()
    # below w_1 every mode answers in phase, a little more than statically: the load does more work
    assert out["power"][1, 0] > out["power"][0, 0] > 0.0
    cocg = DH.harmonic(harm.K, harm.M, harm.fixed, [0.5 * harm.w[0]], harm.load, solver=DH.jacobi_cocg(1e-10, 4000))
    assert not cocg["u"].imag.any()
    assert np.abs(cocg["u"][0] - out["u"][1]).max() <= 1e-8 * np.abs(out["u"][1]).max()


def test_a_complex_load_and_loads_on_fixed_dofs():
    h = _harm.get("B") or _Harm("B")
    _harm["B"] = h
    w = h.W[3:4]
    phase = np.exp(0.7j)
    a = DH.harmonic(h.K, h.M, h.fixed, w, phase * h.load, *h.D)["u"][0]
    assert np.abs(a - phase * h.dense["u"][3]).max() <= 1e-12 * np.abs(a).max()
    f = h.load.copy()
    f[h.fixed] = 5.0                                   # ignored
    assert np.array_equal(DH.harmonic(h.K, h.M, h.fixed, w, f, *h.D)["u"][0], h.dense["u"][3])


def test_breakdown_and_iteration_limit_are_reported():
    h = _harm.get("B") or _Harm("B")
    _harm["B"] = h
    counts = []
    DH.harmonic(h.K, h.M, h.fixed, h.W[4:5], h.load, *h.D, solver=DH.jacobi_cocg(1e-10, 8, counts))
    assert counts == [(8, 1)]
    counts.clear()
    out = DH.harmonic(h.K, h.M, h.fixed, [1.0], np.zeros(h.n6), solver=DH.jacobi_cocg(1e-10, 8, counts))
    assert counts == [(0, 0)] and not out["u"].any()
    # K = I, M = diag(0, 2, ...), w = 1: A = diag(1, -1, ...), so r^T z and p^T A p of the load of ones vanish
    counts.clear()
    one = DH.harmonic(np.eye(6), np.diag([0.0, 2.0] * 3), np.zeros(6, bool), [1.0], np.ones(6),
                      solver=DH.jacobi_cocg(1e-10, 8, counts))
    assert counts == [(1, 2)] and not one["u"].any() and one["status"].tolist() == [2]


def test_argument_checks():
    h = _harm.get("B") or _Harm("B")
    _harm["B"] = h
    for bad in ([-1.0], [np.nan], [np.inf], []):
        with pytest.raises(ValueError):
            DH.harmonic(h.K, h.M, h.fixed, bad, h.load)
    with pytest.raises(ValueError):
        DH.harmonic(h.K, h.M, h.fixed, [1.0], h.load, ray_m=-1e-3)
    with pytest.raises(ValueError):
        DH.harmonic(h.K, h.M, h.fixed, [1.0], h.load, ray_k=-1e-3)
    out = DH.harmonic(h.K, h.M, h.fixed, 2.0, h.load.reshape(-1, 6))       # a scalar frequency, an (N, 6) load
    assert out["u"].shape == (1, h.c.n, 6) and out["omega"].shape == (1,) and "iterations" not in out
