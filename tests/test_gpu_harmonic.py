"""Frequency response on the device (pl_harm_spmv / pl_harmonic, csrc/pl_harm.h) against the existing
products and the numpy / scipy restatement (dynamics_host.harmonic): the fused complex product on every built-in geometry and
lane mapping, the response against the dense solve on the handle's own K, the power identities, the static and the undamped
limits, the lock step of the frequencies of a pass, reciprocity, a shaken base through LatticeSim, a frequency that runs out of
iterations, a breakdown, the handle's state and the error codes.

The lattices are those of tests/test_mass_host.py (A, B, C), the frequencies W = {0, 0.5 w_1, 0.98 w_1, mid(w_1, w_3),
mid(w_6, w_7), mid(w_20, w_21)} with w_i from the dense eigen-solution of the handle's own K and the restated M, the damping
D = (0.05 w_1, 0.002 / w_1), rtol = 1e-10, max_iter = 4000 (no converged case may use more than half of it).  Bars: 1e-12 of the
largest magnitude on the product (the bound of its siblings), 1e-8 of each quantity's largest magnitude against the dense solve
(the restatement's own COCG is within 8.2e-11 of it) and on the power identities, 1e-9 at w = 0 against pl_solve_multi.

Left out: the undamped solve at w = w_1 exactly.  The system is singular there and what COCG does with it depends on the last
bits: the host restatement converges on B after 1841 iterations and runs into max_iter on A and C, so no status can be asserted
from it.  The iteration limit is tested on a frequency that is merely slow, the breakdown status on a load whose
r^T z vanishes exactly."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.geometries import _BUILTIN                       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

from test_mass_host import E, KAPPA, NU, PEN, RHO, _preset, case       # noqa: E402

RTOL, MAX_ITER = 1e-10, 4000


def _device(c, **kw):
    dev = _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN, beam_mult=c.mult, **kw)
    dev.set_bc(c.fixed)
    dev.assemble()
    dev.set_mass(RHO, True, c.node_mass)
    return dev


class _Case:
    """One handle, the dense eigenvalues of its own K and the restated M on the free dofs, the top-face load, four probes, the
    restatement's dense solution at W with D and the device's: computed once, shared by the tests below, left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        c = self.c
        self.dev = _device(c)
        self.dev.assemble_bsr(False)
        rowptr, col, vals = self.dev.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * c.n, 6 * c.n)).tocsr()
        K.sum_duplicates()
        self.K, self.M = K, sp.csr_matrix(self.dev.mass_matrix_host())
        self.fixed = c.fixed.reshape(-1)
        self.free = np.flatnonzero(~self.fixed)
        self.Kf = K[self.free][:, self.free].toarray()
        self.Mf = self.M[self.free][:, self.free].toarray()
        w = np.sqrt(scipy.linalg.eigh(self.Kf, self.Mf, eigvals_only=True))
        self.w = w
        self.W = np.array([0.0, 0.5 * w[0], 0.98 * w[0], 0.5 * (w[0] + w[2]), 0.5 * (w[5] + w[6]), 0.5 * (w[19] + w[20])])
        self.D = (0.05 * w[0], 0.002 / w[0])
        top = np.flatnonzero(c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9)
        f = np.zeros((c.n, 6))
        f[top, 0], f[top, 2] = 0.03, -0.1
        self.load = np.where(c.fixed, 0.0, f)
        self.probes = np.array([top[0], top[-1], c.n // 2, int(np.flatnonzero(~c.fixed.all(axis=1))[0])], np.int32)
        self.host = self.dev.harmonic_host(c.fixed, self.W, self.load, *self.D)
        self.out = self.dev.harmonic(self.W, self.load, *self.D, probes=self.probes, fields=True, rtol=RTOL, max_iter=MAX_ITER)


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
# 1. the fused complex product
# ---------------------------------------------------------------------------------------------------------------------
# (c_K, c_M) per frequency: purely real, purely imaginary, general, M alone, K alone
COEF = np.array([[1.0, -2.5], [0.3j, 1.7j], [1.0 + 0.2j, -0.9 + 0.05j], [0.0, 1.0], [1.0, 0.0]])


def _product_checks(dev, X, Y, mask, nm, tag):
    n = dev.n_nodes
    worst = 0.0
    for rotary in (False, True):
        for node_mass in (None, nm):
            dev.set_mass(RHO, rotary, node_mass)
            for masked in (False, True):
                kx = dev.spmv_multi(X.real, masked=masked) + 1j * dev.spmv_multi(X.imag, masked=masked)
                mx = dev.mass_spmv_multi(X.real, masked=masked) + 1j * dev.mass_spmv_multi(X.imag, masked=masked)
                ref = COEF[:, 0, None, None] * kx + COEF[:, 1, None, None] * mx
                for k in (1, 2, 3, 5):
                    got = dev.harm_spmv(COEF[:k], X[:k], masked=masked)
                    assert got.shape == (k, n, 6) and got.dtype == np.complex128
                    scale = np.abs(ref[:k]).max()
                    err = np.abs(got - ref[:k]).max()
                    worst = max(worst, err / scale)
                    assert scale > 0 and err <= 1e-12 * scale, (tag, rotary, masked, k, err / scale)
                    if masked:
                        assert not got[:, mask].any()
                # the same coefficients as four reals per frequency
                again = dev.harm_spmv(np.ascontiguousarray(COEF[:3]).view(np.float64).reshape(3, 4), X[:3], masked=masked)
                assert np.array_equal(again, dev.harm_spmv(COEF[:3], X[:3], masked=masked))
    ax, ay = dev.harm_spmv(COEF, X), dev.harm_spmv(COEF, Y)
    for j in range(X.shape[0]):                       # complex symmetric: X^T (A Y) = Y^T (A X), unconjugated
        a, b = (Y[j] * ax[j]).sum(), (X[j] * ay[j]).sum()
        assert abs(a - b) <= 1e-12 * float((np.abs(Y[j]) * np.abs(ax[j])).sum()), (tag, j, a, b)
    return worst


def _complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("geom", sorted(_BUILTIN))
def test_complex_product_equals_the_combination_of_the_real_products(geom):
    """(c_K K + c_M M) X for complex X on reorder = 0 and 1 handles of a 2 x 2 x 2 lattice, n_freq = 1, 2, 3, 5 with distinct
    coefficients per frequency (purely real, purely imaginary, general, M alone, K alone), masked and unmasked, with and
    without the rotary inertia and the point masses, within 1e-12 of the largest magnitude of the combination of spmv_multi and
    mass_spmv_multi on the real and imaginary parts, and X^T (A Y) = Y^T (A X)."""
    L = LatticeSim(_preset(geom, (2, 2, 2)))
    lat, pen = L.lattice, L.penalized
    n = lat.n_nodes
    rng = np.random.default_rng(11)
    X, Y = _complex(rng, (5, n, 6)), _complex(rng, (5, n, 6))
    mask = rng.random((n, 6)) < 0.25
    mask[0] = True
    radius = 0.03 + 0.04 * rng.random(lat.n_beams)
    nm = 0.05 * rng.random(n)
    worst = 0.0
    for reorder in (0, 1):
        with _capi.HipLattice(lat.node_xyz, lat.beam_conn, radius, pen.seg_len, pen.seg_nsub, E, NU, reorder=reorder) as dev:
            dev.set_bc(mask)
            dev.assemble()
            worst = max(worst, _product_checks(dev, X, Y, mask, nm, (geom, reorder)))
    print(f"\n{geom}: complex product within {worst:.2e} of the largest magnitude")


@pytest.mark.parametrize("lpn", [1, 2, 4, 8, 16])
def test_complex_product_at_every_lane_mapping(lpn):
    """The same on lattice C (63 nodes: more than one slice at every mapping, a last slice that is not full) with 1, 2, 4, 8
    and 16 lanes per node."""
    c = case("C")
    rng = np.random.default_rng(5)
    X, Y = _complex(rng, (5, c.n, 6)), _complex(rng, (5, c.n, 6))
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, beam_mult=c.mult, lanes_per_node=lpn) as dev:
        dev.set_bc(c.fixed)
        dev.assemble()
        worst = _product_checks(dev, X, Y, c.fixed, c.node_mass, ("C", lpn))
    print(f"\nlanes per node {lpn}: within {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the response
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_response_equals_the_dense_solve(dcase):
    """Fields, probes and the four power sums at W with D against the restatement's dense solve on the handle's own K, within
    1e-8 of each quantity's largest magnitude; both power identities within 1e-8 of the larger side."""
    out, host = dcase.out, dcase.host
    assert not out["status"].any() and (out["relres"] <= RTOL).all()
    assert out["iters"].max() <= MAX_ITER // 2 and out["iters"].min() > 0
    e_field = _rel(out["fields"], host["u"])
    per_freq = [_rel(out["fields"][k], host["u"][k]) for k in range(len(dcase.W))]
    e_probe = _rel(out["probe"], host["u"][:, dcase.probes])
    e_power = [_rel(out["power"][:, q], host["power"][:, q]) for q in range(4)]
    print(f"\n{dcase.name}: iterations {out['iters'].tolist()}, fields {e_field:.2e} (per frequency {max(per_freq):.2e}), "
          f"probes {e_probe:.2e}, power {max(e_power):.2e}")
    assert e_field <= 1e-8 and e_probe <= 1e-8 and max(e_power) <= 1e-8
    assert np.array_equal(out["probe"], out["fields"][:, dcase.probes])
    assert not out["fields"][:, dcase.c.fixed].any()
    rm, rk = dcase.D
    worst = 0.0
    for w, (re, im, uku, umu) in zip(dcase.W, out["power"]):
        for x, y in ((re, uku - w * w * umu), (-im, w * (rm * umu + rk * uku))):
            big = max(abs(x), abs(y))
            worst = max(worst, abs(x - y) / big if big > 0 else 0.0)
            assert abs(x - y) <= 1e-8 * big, (dcase.name, w, x, y)
        assert -im >= 0.0
    print(f"{dcase.name}: power identities within {worst:.2e}")


def test_zero_frequency_is_the_static_solve_and_the_undamped_response_is_real(dcase):
    dev = dcase.dev
    static = dev.solve_multi(f=dcase.load[None], rtol=1e-12, max_iter=100000)[0][0]
    assert _rel(dcase.out["fields"][0], static) <= 1e-9
    und = dev.harmonic([0.5 * dcase.w[0]], dcase.load, probes=dcase.probes, fields=True, rtol=RTOL, max_iter=MAX_ITER)
    assert und["status"][0] == 0 and np.abs(und["fields"].real).max() > 0
    assert (und["fields"].imag == 0.0).all() and (und["probe"].imag == 0.0).all() and und["power"][0, 1] == 0.0


def test_frequencies_of_a_pass_iterate_in_lock_step(dcase):
    """Every frequency of the six-frequency call returns the bits and the iteration count of a call with that frequency alone
    and of passes of 1, 2 and 32 frequencies - the first frequencies are frozen long before the last one ends."""
    dev, out = dcase.dev, dcase.out
    assert out["iters"].min() < out["iters"].max()
    kw = dict(probes=dcase.probes, fields=True, rtol=RTOL, max_iter=MAX_ITER)
    for k, w in enumerate(dcase.W):
        one = dev.harmonic([w], dcase.load, *dcase.D, **kw)
        assert one["iters"][0] == out["iters"][k], (dcase.name, k)
        assert np.array_equal(one["fields"][0], out["fields"][k]) and np.array_equal(one["power"][0], out["power"][k])
        assert one["relres"][0] == out["relres"][k]
    for block in (1, 2, 32):
        again = dev.harmonic(dcase.W, dcase.load, *dcase.D, block=block, **kw)
        for q in ("fields", "probe", "power", "iters", "relres", "status"):
            assert np.array_equal(again[q], out[q]), (dcase.name, block, q)


def test_reciprocity(case_a):
    """A unit load at dof a read at dof b equals a unit load at b read at a."""
    dev = case_a.dev
    (na, da), (nb, db) = (int(case_a.probes[0]), 0), (int(case_a.probes[2]), 2)
    assert not case_a.c.fixed[na, da] and not case_a.c.fixed[nb, db]
    w = case_a.W[3:5]
    got = []
    for (n_in, d_in), (n_out, d_out) in (((na, da), (nb, db)), ((nb, db), (na, da))):
        f = np.zeros((case_a.c.n, 6))
        f[n_in, d_in] = 1.0
        out = dev.harmonic(w, f, *case_a.D, probes=[n_out], rtol=RTOL, max_iter=MAX_ITER)
        got.append(out["probe"][:, 0, d_out])
    assert np.abs(got[0]).min() > 0
    assert (np.abs(got[0] - got[1]) <= 1e-8 * np.maximum(np.abs(got[0]), np.abs(got[1]))).all(), got


def test_a_frequency_that_runs_out_of_iterations(case_a):
    """max_iter = 8 stops one frequency of three: undamped at 1e8 w_1 and 2e8 w_1 the operator is -w^2 M to 1e-12, and the load
    is the eigenvector of M D^-1 (D = diag M), so COCG ends in a step or two there; at mid(w_6, w_7) it needs hundreds.
    PL_ERR_NOCONV, status 1 for that frequency alone, the other two written and correct."""
    dev, c = case_a.dev, case_a.c
    dg = np.diag(case_a.Mf)
    y = np.linalg.eigh(case_a.Mf / np.sqrt(np.outer(dg, dg)))[1][:, -1]
    load = np.zeros(6 * c.n)
    load[case_a.free] = np.sqrt(dg) * y
    w = np.array([1e8 * case_a.w[0], case_a.W[4], 2e8 * case_a.w[0]])
    with pytest.raises(_capi.PlError) as e:
        dev.harmonic(w, load, fields=True, rtol=RTOL, max_iter=8)
    assert e.value.code == _capi.PL_ERR_NOCONV
    out = dev.harmonic(w, load, fields=True, rtol=RTOL, max_iter=8, raise_on_noconv=False)
    assert out["status"].tolist() == [0, 1, 0] and out["iters"][1] == 8 and out["iters"][[0, 2]].max() <= 8
    assert out["relres"][1] > RTOL and np.isfinite(out["fields"]).all()
    host = dev.harmonic_host(c.fixed, w, load)
    for k in (0, 2):
        assert _rel(out["fields"][k], host["u"][k]) <= 1e-8
        assert _rel(out["power"][k], host["power"][k]) <= 1e-8
    # a zero load is frozen before iteration 0
    zero = dev.harmonic(w, np.zeros(6 * c.n), fields=True, rtol=RTOL, max_iter=8)
    assert not zero["status"].any() and not zero["iters"].any() and not zero["fields"].any()


def test_a_breakdown_is_flagged_apart_from_the_iteration_limit():
    """Two copies of a clamped tripod, the second shifted by 4 along x (coordinates that subtract exactly), reorder = 0 and one
    lane per node: the twin apexes have the same diagonal bit for bit, so the load e_a + i e_a' has r^T z = 1 / d - 1 / d = 0
    at the start.  COCG cannot take a step: status 2 after one iteration at every frequency, x = 0, PL_ERR_NOCONV."""
    tripod = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 1.0]])
    xyz = np.vstack([tripod, tripod + np.array([4.0, 0.0, 0.0])])
    conn = np.array([[0, 3], [1, 3], [2, 3], [4, 7], [5, 7], [6, 7]], np.int32)
    length = np.linalg.norm(xyz[conn[:, 1]] - xyz[conn[:, 0]], axis=1)
    seg_len = np.column_stack([np.zeros(6), length, np.zeros(6)])
    seg_nsub = np.tile(np.array([0, 20, 0], np.int32), (6, 1))
    fixed = np.ones((8, 6), bool)
    fixed[[3, 7]] = False
    load = np.zeros((8, 6), complex)
    load[3, 2], load[7, 2] = 1.0, 1.0j
    with _capi.HipLattice(xyz, conn, np.full(6, 0.05), seg_len, seg_nsub, E, NU, reorder=0, lanes_per_node=1) as dev:
        dev.set_bc(fixed)
        dev.assemble()
        dev.set_mass(RHO)
        w1 = float(np.sqrt(dev.vibration_modes_host(fixed, 1, dense=True)["omega2"][0]))
        omegas = [0.5 * w1, 2.0 * w1]
        with pytest.raises(_capi.PlError) as e:
            dev.harmonic(omegas, load, 0.05 * w1, 0.002 / w1, fields=True, rtol=RTOL, max_iter=MAX_ITER)
        assert e.value.code == _capi.PL_ERR_NOCONV
        out = dev.harmonic(omegas, load, 0.05 * w1, 0.002 / w1, fields=True, rtol=RTOL, max_iter=MAX_ITER, raise_on_noconv=False)
        assert out["status"].tolist() == [2, 2] and out["iters"].tolist() == [1, 1]
        assert not out["fields"].any() and (out["relres"] == 1.0).all()
        # one apex alone is an ordinary solve
        load[7, 2] = 0.0
        one = dev.harmonic(omegas, load, 0.05 * w1, 0.002 / w1, fields=True, rtol=RTOL, max_iter=MAX_ITER)
        assert not one["status"].any() and np.abs(one["fields"][:, 3]).max() > 0 and not one["fields"][:, 7].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. LatticeSim
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_sim_frequency_response_of_a_shaken_base():
    L = LatticeSim(_preset("BCC", (2, 2, 3)))
    with pytest.raises(RuntimeError):
        L.frequency_response([1.0], RHO)
    with pytest.raises(RuntimeError):
        L.dynamic_stiffness_peaks()
    solve_FEM_FenicsX(L, rtol=1e-10)
    n = L.lattice.n_nodes
    fixed = np.asarray(L.fixed_DOF).reshape(n, 6) != 0
    dev = L._device
    dev.set_mass(RHO)
    w = np.sqrt(dev.vibration_modes_host(fixed, 3, dense=True)["omega2"])
    damping = (0.05 * w[0], 0.002 / w[0])
    hz = np.concatenate([[0.0], np.linspace(0.6 * w[0], 1.3 * w[2], 12)]) / (2.0 * np.pi)
    loaded = np.flatnonzero(np.abs(L.applied_force[:n, :3]).sum(axis=1) > 0)
    out = L.frequency_response(hz, RHO, damping=damping, base_acceleration=2, rtol=RTOL, max_iter=MAX_ITER)
    assert L.frf_probe.shape == (hz.size, loaded.size, 6) and L.frf_power.shape == (hz.size, 4)
    assert np.array_equal(L.frf_frequency, hz) and L.frf_iterations.shape == (hz.size,) and not out["status"].any()
    ez = np.zeros((n, 6))
    ez[:, 2] = 1.0
    pattern = -(dev.mass_matrix_host() @ ez.reshape(-1))
    host = dev.harmonic_host(fixed, 2.0 * np.pi * hz, pattern, *damping)
    assert _rel(L.frf_probe, host["u"][:, loaded]) <= 1e-8
    assert _rel(L.frf_power, host["power"]) <= 1e-8
    # the rigid value at w = 0: the structure rides on its base, the relative part of the transmissibility is 0
    T = L.frf_transmissibility
    assert T.shape == (hz.size, loaded.size, 3)
    assert np.array_equal(T[0], np.broadcast_to(np.array([0.0, 0.0, 1.0]), T[0].shape))
    assert np.abs(T[1:, :, 2]).max() > 1.0
    # the force set as the load, and its peaks
    direct = L.frequency_response(hz[1:], RHO, damping=damping, probes=loaded[:2], rtol=RTOL, max_iter=MAX_ITER)
    assert L.frf_transmissibility is None and direct["probe"].shape == (hz.size - 1, 2, 6)
    force = np.zeros((n, 6))
    force[:, :3] = L.applied_force[:n, :3]
    assert np.array_equal(direct["probe"], dev.harmonic(2.0 * np.pi * hz[1:], force, *damping, probes=loaded[:2], rtol=RTOL,
                                                        max_iter=MAX_ITER)["probe"])
    peaks = L.dynamic_stiffness_peaks()
    assert len(peaks) == 2
    amp = np.linalg.norm(L.frf_probe[:, :, :3], axis=2)
    for j, pk in enumerate(peaks):
        assert pk["index"].size >= 1 and np.array_equal(pk["amplitude"], amp[pk["index"], j])
        assert np.array_equal(pk["frequency"], hz[1:][pk["index"]]) and amp[:, j].max() in pk["amplitude"]
    with pytest.raises(NotImplementedError):
        LatticeSim(_preset("BCC", (2, 2, 2)), reference_compat=True).frequency_response(hz, RHO)
    p = _preset("BCC", (2, 2, 2))
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError):
        LatticeSim(p, enable_domain_decomposition_solver=True).frequency_response(hz, RHO)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the handle's state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_solve_after_the_calls_returns_the_same_bits(case_a):
    c = case_a.c
    f = np.zeros((c.n, 6))
    f[c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9, 0] = 0.01
    fixed_order = dict(spmv_kernel=2, precond=1)
    X = _complex(np.random.default_rng(2), (3, c.n, 6))
    with _device(c, **fixed_order) as dev, _device(c, **fixed_order) as twin:
        for d in (dev, twin):
            d.set_bc(c.fixed, None, f)
        first = [d.solve(rtol=1e-12, max_iter=100000)[0] for d in (dev, twin)]
        assert np.array_equal(first[0], first[1]) and np.abs(first[0]).max() > 0
        modes0 = dev.vibration_modes(3, n_sub=8)
        trans0 = dev.transient(2.0 * np.pi / case_a.w[0] / 40.0, 10, f[None], np.ones((11, 1)), rtol=1e-10, probes=[1, 2])
        dev.harm_spmv(COEF[:3], X, masked=True)
        dev.harmonic(case_a.W[1:4], f, *case_a.D, probes=[1, 2], fields=True, rtol=RTOL, max_iter=MAX_ITER)
        modes1 = dev.vibration_modes(3, n_sub=8)
        trans1 = dev.transient(2.0 * np.pi / case_a.w[0] / 40.0, 10, f[None], np.ones((11, 1)), rtol=1e-10, probes=[1, 2])
        assert np.array_equal(modes0["omega2"], modes1["omega2"]) and np.array_equal(modes0["modes"], modes1["modes"])
        for q in ("probe", "energy", "state", "iters"):
            assert np.array_equal(trans0[q], trans1[q]), q
        again = [d.solve(rtol=1e-12, max_iter=100000) for d in (dev, twin)]
        assert np.array_equal(again[0][0], again[1][0])
        assert again[0][1]["iterations"] == again[1][1]["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. error codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = case("A")
    lib, p = _capi.load_library(), _capi._ptr
    n6 = 6 * c.n
    OK, ARG, STATE = _capi.PL_OK, _capi.PL_ERR_ARG, _capi.PL_ERR_STATE
    x = np.ascontiguousarray(_complex(np.random.default_rng(1), (2, n6)))
    y = np.empty_like(x)
    coef = np.array([[1.0, 0.1, -2.0, 0.3], [1.0, 0.0, -5.0, 0.0]])
    load = np.zeros(n6)
    load[n6 - 4] = -0.1
    omega = np.array([0.0, 3.0])
    probes = np.array([1, c.n - 1], np.int32)
    probe, power = np.empty((2, 2, 6), np.complex128), np.empty((2, 4))
    iters, relres, status = np.zeros(2, np.int32), np.zeros(2), np.zeros(2, np.int32)

    def spmv(h, n=2, masked=0, coef_=coef, x_=x, y_=y):
        return lib.pl_harm_spmv(h, n, p(coef_), masked, p(x_), p(y_))

    def run(h, n=2, omega_=omega, rm=0.1, rk=1e-3, load_=load, n_probe=2, probes_=probes, rtol=1e-8, it=4000, block=0,
            probe_=probe, iters_=iters, relres_=relres, status_=status):
        return lib.pl_harmonic(h, n, p(omega_), rm, rk, p(load_), None, n_probe, p(probes_), rtol, it, block, p(probe_), None,
                               p(power), p(iters_), p(relres_), p(status_))

    assert run(None) == ARG and spmv(None) == ARG
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN) as dev:
        h = dev._h
        assert spmv(h) == STATE and run(h) == STATE                                # before pl_assemble
        dev.assemble()
        assert run(h) == STATE and spmv(h) == STATE                                # before pl_set_mass
        assert b"pl_set_mass" in lib.pl_last_error()
        dev.set_mass(RHO)
        assert spmv(h) == OK
        assert spmv(h, masked=1) == STATE and run(h) == STATE                      # before pl_set_bc
        assert b"pl_set_bc" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert spmv(h, masked=1) == OK and run(h) == OK and not status.any()
        assert spmv(h, n=0) == ARG and spmv(h, n=_capi.MULTI_MAX // 2 + 1) == ARG
        assert spmv(h, x_=None) == ARG and spmv(h, y_=None) == ARG and spmv(h, coef_=None) == ARG
        assert spmv(h, coef_=np.array([[1.0, np.nan, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])) == ARG
        assert run(h, n=0) == ARG
        assert run(h, omega_=np.array([0.0, -1.0])) == ARG and run(h, omega_=np.array([np.inf, 1.0])) == ARG
        assert b"omega" in lib.pl_last_error()
        assert run(h, rm=-1e-3) == ARG and run(h, rk=-1e-3) == ARG
        assert run(h, rtol=0.0) == ARG and run(h, it=0) == ARG
        assert run(h, block=-1) == ARG and run(h, block=_capi.MULTI_MAX // 2 + 1) == ARG
        assert run(h, probes_=np.array([1, c.n], np.int32)) == ARG and run(h, probes_=np.array([-1, 0], np.int32)) == ARG
        assert b"probe" in lib.pl_last_error()
        assert run(h, probes_=None) == ARG and run(h, probe_=None) == ARG
        assert run(h, omega_=None) == ARG and run(h, load_=None) == ARG
        assert run(h, iters_=None) == ARG and run(h, relres_=None) == ARG and run(h, status_=None) == ARG
        assert run(h, n_probe=0, probes_=None, probe_=None) == OK
        assert run(h, block=1) == OK and run(h, block=32) == OK
        ubar = np.zeros((c.n, 6))
        ubar[c.fixed] = 1e-3
        dev.set_bc(c.fixed, ubar)
        assert run(h) == STATE and b"prescribed" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert run(h) == OK
        master = np.arange(c.n, dtype=np.int32)
        master[c.n - 1] = c.n - 2
        dev.set_periodic(master)
        assert spmv(h) == STATE and run(h) == STATE
        assert b"periodic" in lib.pl_last_error()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        x12 = np.ones((2, 12), np.complex128)
        assert lib.pl_harm_spmv(ddm._h, 2, p(coef), 0, p(x12), p(np.empty_like(x12))) == STATE
        assert run(ddm._h, load_=np.zeros(12), probes_=np.array([0, 1], np.int32)) == STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            m6 = 6 * dev.n_nodes
            xm = np.ones((2, m6), np.complex128)
            assert lib.pl_harm_spmv(dev._h, 2, p(coef), 0, p(xm), p(np.empty_like(xm))) == STATE
            assert run(dev._h, load_=np.zeros(m6), probes_=np.array([0, 1], np.int32)) == STATE
            assert b"multi-rank" in lib.pl_last_error()
