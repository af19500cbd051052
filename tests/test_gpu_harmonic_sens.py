"""Radius sensitivities of the frequency response on the device (pl_harmonic_sens, csrc/pl_harm_sens.h)
against the numpy / scipy restatement on the handle's own K (dynamics_host.harmonic_sensitivity), the bits it shares with
pl_harmonic, frequency counts around the groups of the contraction and the passes of the solver, central differences through
pl_update_radii, the handle's state, the error codes, and the Python layers above it.

The lattices are those of tests/test_mass_host.py (A, B, C); the frequencies W, the damping D and the top-face load those of
tests/test_gpu_harmonic.py; l the generic vector of tests/test_dynamics_sens_host.py; base_dir = (0.6, 0, 0.8).  rtol = 1e-10,
max_iter = 4000 (no converged solve may use more than 2000).  Bars: 1e-8 of each quantity's largest magnitude against the
restatement's dense solves (the bar of section 10i), 1e-5 of the largest difference quotient on central differences with
h = 1e-6 (section 10h)."""
import copy
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd import dynamics_host as DH                       # noqa: E402
from pylatticedso_amd.lattice_opti import LatticeOpti                  # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_simulation import solve_FEM_FenicsX        # noqa: E402

from test_mass_host import E, KAPPA, NU, PEN, RHO, _preset, case       # noqa: E402

RTOL, MAX_ITER = 1e-10, 4000
BASE_DIR = np.array([0.6, 0.0, 0.8])
# (dead load, base, out_vec)
LOADS = {"dead": (True, False, True), "base": (True, True, True), "self": (True, False, False), "self_base": (True, True, False)}
KINDS = (0, 1, 2)


def _device(c, **kw):
    dev = _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN, beam_mult=c.mult, **kw)
    dev.set_bc(c.fixed)
    dev.assemble()
    dev.set_mass(RHO, True, c.node_mass)
    return dev


class _Case:
    """One lattice with a handle per node ordering, the dense eigenvalues of its own K and the restated M, the frequencies, the
    top-face load, the generic output vector and weights: computed once, shared, left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        c = self.c
        self.devs = {r: _device(c, reorder=r) for r in (0, 1)}
        dev = self.devs[0]
        dev.assemble_bsr(False)
        rowptr, col, vals = dev.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * c.n, 6 * c.n)).tocsr()
        K.sum_duplicates()
        self.free = np.flatnonzero(~c.fixed.reshape(-1))
        Kf = K[self.free][:, self.free].toarray()
        self.Mf = sp.csr_matrix(dev.mass_matrix_host())[self.free][:, self.free].toarray()
        w = np.sqrt(scipy.linalg.eigh(Kf, self.Mf, eigvals_only=True))
        self.w = w
        self.W = np.array([0.0, 0.5 * w[0], 0.98 * w[0], 0.5 * (w[0] + w[2]), 0.5 * (w[5] + w[6]), 0.5 * (w[19] + w[20])])
        self.D = (0.05 * w[0], 0.002 / w[0])
        self.top = np.flatnonzero(c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9)
        f = np.zeros((c.n, 6))
        f[self.top, 0], f[self.top, 2] = 0.03, -0.1
        self.load = np.where(c.fixed, 0.0, f)
        self.l = np.random.default_rng(7).standard_normal((c.n, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])

    def weights(self, n):
        return 0.5 + np.random.default_rng(3).random(n)

    def args(self, which, kind, omegas=None, damped=True, weight="w"):
        """the keyword arguments harmonic_sens and harmonic_sens_host share"""
        _, base, has_l = LOADS[which]
        omegas = self.W if omegas is None else np.asarray(omegas, float)
        rm, rk = self.D if damped else (0.0, 0.0)
        if isinstance(weight, str):
            weight = None if kind == 2 else self.weights(len(omegas))
        return dict(omegas=omegas, load=self.load, out_vec=self.l if has_l else None, kind=kind, p=8.0, weight=weight,
                    base_dir=BASE_DIR if base else None, ray_m=rm, ray_k=rk)

    def reference(self, reorder, which, omegas=None, damped=True):
        """The restatement once for all kinds: its y and dy_dr with harmonic_objective give J and dJ_dr of every kind."""
        ref = self.devs[reorder].harmonic_sens_host(self.c.fixed, **self.args(which, 1, omegas, damped))
        out = {}
        for kind in KINDS:
            wt = self.args(which, kind, omegas, damped)["weight"]
            J, g = DH.harmonic_objective(ref["y"], kind, 8.0, wt)
            out[kind] = {"J": J, "y": ref["y"], "dJ_dr": (g[:, None] * ref["dy_dr"]).real.sum(axis=0)}
        return out


_cases = {}


def _get(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _errors(got, ref):
    """distance relative to each quantity's largest magnitude; a reference that is exactly zero asks for exact zeros"""
    errs = {}
    for q in ("J", "y", "dJ_dr"):
        a, b = np.atleast_1d(got[q]), np.atleast_1d(ref[q])
        scale = np.abs(b).max()
        errs[q] = (0.0 if not a.any() else np.inf) if scale == 0.0 else float(np.abs(a - b).max() / scale)
    return errs


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(LOADS))
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_equals_the_restatement(name, reorder, which):
    """J, y and dJ_dr of the three kinds, damped with D at W and undamped at {0, 0.5 w_1}, within 1e-8 of each quantity's
    largest magnitude of the restatement's dense solves on the handle's own K."""
    d = _get(name)
    dev = d.devs[reorder]
    for damped, omegas in ((True, d.W), (False, np.array([0.0, 0.5 * d.w[0]]))):
        ref = d.reference(reorder, which, omegas, damped)
        for kind in KINDS:
            got = dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, **d.args(which, kind, omegas, damped))
            nf = len(omegas)
            assert got["y"].shape == (nf,) and got["y"].dtype == np.complex128 and got["dJ_dr"].shape == (d.c.B,)
            assert got["iters"].shape == got["relres"].shape == got["status"].shape == (2, nf)
            errs = _errors(got, ref[kind])
            it = got["iters"]
            print(f"\n{name} reorder={reorder} {which} damped={damped} kind {kind}: {errs}; iterations forward "
                  f"{it[0].min()} - {it[0].max()}, adjoint {it[1].min()} - {it[1].max()}")
            assert max(errs.values()) <= 1e-8, errs
            assert not got["status"].any() and (got["relres"] <= RTOL).all()
            assert it.max() <= MAX_ITER // 2 and it[0].min() > 0
            if LOADS[which][2]:
                assert it[1].min() > 0
            else:
                assert not it[1].any() and not got["relres"][1].any()
            if not damped:      # real fields: y is real, kind 0 is exactly zero
                assert not got["y"].imag.any() and np.abs(got["y"].real).min() > 0
                if kind == 0:
                    assert got["J"] == 0.0 and not got["dJ_dr"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the forward block is pl_harmonic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [False, True])
def test_outputs_are_the_fields_of_pl_harmonic(base):
    """y of an output vector with one entry is that entry of pl_harmonic's field bit for bit (a sum with one non-zero term has
    no order), with the iteration counts and the status of that call."""
    d = _get("A")
    c, dev = d.c, d.devs[1]
    load = d.load
    if base:
        e = np.zeros((1, c.n, 6))
        e[0, :, :3] = BASE_DIR
        load = np.where(c.fixed, 0.0, d.load - dev.mass_spmv_multi(e)[0])
    node, dof = int(d.top[1]), 2
    plain = dev.harmonic(d.W, load, *d.D, probes=[node], rtol=RTOL, max_iter=MAX_ITER)
    l = np.zeros((c.n, 6))
    l[node, dof] = 1.0
    a = d.args("base" if base else "dead", 2)
    a["out_vec"] = l
    for block in (0, 1, 5):
        got = dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, block=block, **a)
        assert np.array_equal(got["y"], plain["probe"][:, 0, dof]) and np.abs(got["y"]).min() > 0
        assert np.array_equal(got["iters"][0], plain["iters"]) and np.array_equal(got["status"][0], plain["status"])
        assert np.array_equal(got["relres"][0], plain["relres"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. frequency counts around the groups of the contraction and the passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_freq", [1, 3, 4, 5, 16, 17, 33])
def test_frequency_counts_and_pass_sizes(n_freq):
    """n_freq frequencies from 0.3 w_1 to mid(w_6, w_7) with D: dJ_dr is the same bits for block = 0, 1 and 5 and in two calls,
    with a generic l (16 frequencies per pass) and with out_vec = None (32 per pass), and agrees with the restatement."""
    d = _get("A")
    dev = d.devs[1]
    omegas = np.linspace(0.3 * d.w[0], 0.5 * (d.w[5] + d.w[6]), n_freq) if n_freq > 1 else np.array([0.98 * d.w[0]])
    for which in ("base", "self_base"):
        ref = d.reference(1, which, omegas)
        for kind in (0, 2):
            a = d.args(which, kind, omegas)
            first = dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
            errs = _errors(first, ref[kind])
            print(f"\nA n_freq {n_freq} {which} kind {kind}: {errs}")
            assert max(errs.values()) <= 1e-8, errs
            assert np.abs(first["dJ_dr"]).max() > 0
            for block in (0, 1, 5) if kind == 2 else ():
                again = dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, block=block, **a)
                assert again["J"] == first["J"]
                for q in ("y", "dJ_dr", "iters", "relres", "status"):
                    assert np.array_equal(again[q], first[q]), (which, kind, block, q)


# ---------------------------------------------------------------------------------------------------------------------
# 4. central differences on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_central_differences_through_update_radii():
    """Eight struts of A, strut 3 (multiplicity 2) and the penalised struts among them: two calls per strut and load case at
    r +- 1e-6 through pl_update_radii + pl_assemble, all three objectives from the y of those calls, kind 2 also from the
    call's own J - the derivative record and the mass scaling the handle really uses."""
    d = _get("A")
    c = d.c
    struts = [0, 3, 17, 31, 46, 58, 77, 95]
    assert c.mult[3] == 2.0 and (c.sl[struts][:, [0, 2]] > 0).any()
    h = 1e-6
    wts = d.weights(len(d.W))
    kinds = [(0, wts, 8.0), (1, wts, 8.0), (2, None, 8.0)]
    with _device(c) as dev:
        for which in ("base", "self_base"):
            grads = [dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, **d.args(which, k))["dJ_dr"] for k, _, _ in kinds]
            a = d.args(which, 2)
            fd, fd_own = np.zeros((3, len(struts))), np.zeros(len(struts))
            for i, b in enumerate(struts):
                side = []
                for sg in (+1.0, -1.0):
                    r = c.radius.copy()
                    r[b] += sg * h
                    dev.update_radii(r)
                    dev.assemble()
                    side.append(dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, **a))
                for q, (k, w, p) in enumerate(kinds):
                    fd[q, i] = (DH.harmonic_objective(side[0]["y"], k, p, w)[0]
                                - DH.harmonic_objective(side[1]["y"], k, p, w)[0]) / (2.0 * h)
                fd_own[i] = (side[0]["J"] - side[1]["J"]) / (2.0 * h)
            dev.update_radii(c.radius)
            dev.assemble()
            for q, (k, _, _) in enumerate(kinds):
                err = np.abs(grads[q][struts] - fd[q]).max() / np.abs(fd[q]).max()
                print(f"\n{which} kind {k}: device gradient within {err:.2e} of the largest central difference")
                assert np.abs(fd[q]).max() > 0 and err <= 1e-5
            assert np.abs(grads[2][struts] - fd_own).max() <= 1e-5 * np.abs(fd_own).max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the handle's state
# ---------------------------------------------------------------------------------------------------------------------
def test_the_handle_keeps_its_state():
    """A pl_solve, pl_harmonic, pl_transient and pl_vibration_modes after the calls return the bits of a twin handle that never
    made them."""
    d = _get("A")
    c = d.c
    f = np.zeros((c.n, 6))
    f[c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9, 0] = 0.01
    fixed_order = dict(spmv_kernel=2, precond=1)
    with _device(c, **fixed_order) as dev, _device(c, **fixed_order) as twin:
        for q in (dev, twin):
            q.set_bc(c.fixed, None, f)
        first = [q.solve(rtol=1e-12, max_iter=100000)[0] for q in (dev, twin)]
        assert np.array_equal(first[0], first[1]) and np.abs(first[0]).max() > 0
        for which in ("base", "self"):
            for kind in KINDS:
                got = dev.harmonic_sens(rtol=RTOL, max_iter=MAX_ITER, **d.args(which, kind))
                assert np.abs(got["dJ_dr"]).max() > 0
        after = []
        for q in (dev, twin):
            u, st = q.solve(rtol=1e-12, max_iter=100000)
            modes = q.vibration_modes(3, n_sub=8)
            tr = q.transient(2.0 * np.pi / d.w[0] / 40.0, 10, f[None], np.ones((11, 1)), ray_m=d.D[0], ray_k=d.D[1], rtol=1e-10,
                             probes=[1, 2])
            hm = q.harmonic(d.W[1:4], f, *d.D, probes=[1, 2], fields=True, rtol=RTOL, max_iter=MAX_ITER)
            after.append((u, st["iterations"], modes, tr, hm))
        assert np.array_equal(after[0][0], after[1][0]) and after[0][1] == after[1][1]
        assert np.array_equal(after[0][2]["omega2"], after[1][2]["omega2"])
        assert np.array_equal(after[0][2]["modes"], after[1][2]["modes"])
        for q in ("probe", "energy", "state", "iters"):
            assert np.array_equal(after[0][3][q], after[1][3][q]), q
        for q in ("probe", "fields", "power", "iters", "relres", "status"):
            assert np.array_equal(after[0][4][q], after[1][4][q]), q


# ---------------------------------------------------------------------------------------------------------------------
# 6. error and status codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = case("A")
    lib, p = _capi.load_library(), _capi._ptr
    n6 = 6 * c.n
    OK, ARG, STATE = _capi.PL_OK, _capi.PL_ERR_ARG, _capi.PL_ERR_STATE
    load = np.zeros(n6)
    load[n6 - 4] = -0.1
    l = np.zeros(n6)
    l[n6 - 6] = 1.0
    omega = np.array([0.0, 3.0])
    bdir = np.array([0.0, 0.0, 1.0])
    J = C.c_double(-7.0)
    y, grad = np.full(2, -7.0 + 0j), np.full(c.B, -7.0)
    iters, relres, status = np.zeros((2, 2), np.int32), np.zeros((2, 2)), np.zeros((2, 2), np.int32)

    def run(h, n=2, omega_=omega, rm=0.1, rk=1e-3, load_=load, im_=None, bd=None, l_=l, kind=2, pp=8.0, w=None, rtol=1e-8,
            it=4000, block=0, J_=J, y_=y, g_=grad, iters_=iters, relres_=relres, status_=status):
        return lib.pl_harmonic_sens(h, n, p(omega_), rm, rk, p(load_), p(im_), p(bd), p(l_), kind, pp, p(w), rtol, it, block,
                                    C.byref(J_) if J_ is not None else None, p(y_), p(g_), p(iters_), p(relres_), p(status_))

    assert run(None) == ARG
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN) as dev:
        h = dev._h
        assert run(h) == STATE                                                       # before pl_assemble
        dev.assemble()
        assert run(h) == STATE and b"pl_set_bc" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert run(h) == STATE and b"pl_set_mass" in lib.pl_last_error()
        dev.set_mass(RHO)
        assert J.value == -7.0 and (y == -7.0).all() and (grad == -7.0).all()
        assert run(h) == OK and J.value > 0 and np.abs(grad).max() > 0 and not status.any()
        assert run(h, y_=None) == OK and run(h, iters_=None, relres_=None, status_=None) == OK
        assert run(h, n=0) == ARG
        assert run(h, omega_=np.array([0.0, -1.0])) == ARG and run(h, omega_=np.array([np.inf, 1.0])) == ARG
        assert b"omega" in lib.pl_last_error()
        assert run(h, omega_=None) == ARG
        assert run(h, rm=-1e-3) == ARG and run(h, rk=-1e-3) == ARG
        assert run(h, rtol=0.0) == ARG and run(h, it=0) == ARG
        assert run(h, kind=-1) == ARG and run(h, kind=3) == ARG
        assert run(h, pp=1.5) == ARG and run(h, kind=1, pp=1.5) == OK and run(h, pp=2.0) == OK
        assert run(h, w=np.array([1.0, -1e-3])) == ARG and b"weight" in lib.pl_last_error()
        assert run(h, w=np.array([1.0, np.inf])) == ARG and run(h, w=np.array([0.0, 2.0])) == OK
        assert run(h, J_=None) == ARG and run(h, g_=None) == ARG
        assert run(h, load_=None) == ARG and b"neither" in lib.pl_last_error()
        assert run(h, load_=None, bd=bdir) == OK and J.value > 0                     # the base load alone
        assert run(h, bd=bdir) == OK and run(h, im_=load) == OK
        assert run(h, l_=None) == OK and run(h, l_=None, bd=bdir) == OK
        # the pass limit: PL_MULTI_MAX / 4 with an adjoint block, PL_MULTI_MAX / 2 without
        quarter, half = _capi.MULTI_MAX // 4, _capi.MULTI_MAX // 2
        assert run(h, block=-1) == ARG and run(h, block=quarter + 1) == ARG and run(h, block=quarter) == OK
        assert run(h, l_=None, block=quarter + 1) == OK and run(h, l_=None, block=half) == OK
        assert run(h, l_=None, block=half + 1) == ARG and b"block" in lib.pl_last_error()
        # a zero load: nothing moves, the adjoint still solves
        assert run(h, load_=np.zeros(n6)) == OK and J.value == 0.0 and not grad.any() and not y.any()
        assert not iters[0].any() and iters[1].min() > 0
        # an objective that is not a finite number: |y|^2 overflows
        assert run(h, l_=np.full(n6, 1e200), kind=1) == _capi.PL_ERR_NAN and b"finite" in lib.pl_last_error()
        assert run(h) == OK                                                          # the handle is still usable
        ubar = np.zeros((c.n, 6))
        ubar[c.fixed] = 1e-3
        dev.set_bc(c.fixed, ubar)
        assert run(h) == STATE and b"prescribed" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert run(h) == OK
        master = np.arange(c.n, dtype=np.int32)
        master[c.n - 1] = c.n - 2
        dev.set_periodic(master)
        assert run(h) == STATE and b"periodic" in lib.pl_last_error()
    ddm = _capi.HipLattice.ddm(2, np.array([[0, 1]], np.int32), np.eye(12)[None], np.zeros(1, np.int32))
    try:
        assert run(ddm._h, load_=np.zeros(12), l_=np.ones(12), g_=np.zeros(8)) == STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            m6 = 6 * dev.n_nodes
            assert run(dev._h, load_=np.zeros(m6), l_=np.ones(m6), g_=np.zeros(dev.n_beams)) == STATE
            assert b"multi-rank" in lib.pl_last_error()


def test_a_solve_that_runs_out_of_iterations_in_either_block():
    """max_iter = 8 and the slow frequency of test_gpu_harmonic.test_a_frequency_that_runs_out_of_iterations: undamped at
    1e8 w_1 and 2e8 w_1 the operator is -w^2 M to 1e-12 and the eigenvector of M D^-1 (D = diag M) ends COCG in a step or two;
    at mid(w_6, w_7) it needs hundreds.  PL_ERR_NOCONV from the forward block (that load, the same vector as l), and from the
    adjoint block alone (a zero load, which is converged at iteration 0, and a generic l): J, y and dJ_dr stay untouched, the
    status rows are filled."""
    d = _get("A")
    c, dev = d.c, d.devs[1]
    lib, p = _capi.load_library(), _capi._ptr
    dg = np.diag(d.Mf)
    v = np.linalg.eigh(d.Mf / np.sqrt(np.outer(dg, dg)))[1][:, -1]
    quick = np.zeros(6 * c.n)
    quick[d.free] = np.sqrt(dg) * v
    w = np.array([1e8 * d.w[0], d.W[4], 2e8 * d.w[0]])
    J = C.c_double(-7.0)
    y, grad = np.full(3, -7.0 + 0j), np.full(c.B, -7.0)

    def run(load, l, it):
        iters, relres, status = np.full((2, 3), -7, np.int32), np.full((2, 3), -7.0), np.full((2, 3), -7, np.int32)
        rc = lib.pl_harmonic_sens(dev._h, 3, p(w), 0.0, 0.0, p(load), None, None, p(l), 2, 8.0, None, RTOL, it, 0, C.byref(J),
                                  p(y), p(grad), p(iters), p(relres), p(status))
        return rc, iters, relres, status

    rc, iters, relres, status = run(quick, quick, 8)
    assert rc == _capi.PL_ERR_NOCONV and b"without convergence" in lib.pl_last_error()
    assert status.tolist() == [[0, 1, 0], [0, 1, 0]] and iters[:, 1].tolist() == [8, 8] and iters[:, [0, 2]].max() <= 8
    assert (relres[:, 1] > RTOL).all() and (relres[:, [0, 2]] <= RTOL).all()
    assert J.value == -7.0 and (y == -7.0).all() and (grad == -7.0).all()
    rc, iters, relres, status = run(np.zeros(6 * c.n), d.l.reshape(-1), 8)
    assert rc == _capi.PL_ERR_NOCONV
    assert not status[0].any() and not iters[0].any() and not relres[0].any()
    assert status[1].any() and iters[1].max() == 8
    assert J.value == -7.0 and (y == -7.0).all() and (grad == -7.0).all()
    with pytest.raises(_capi.PlError) as e:
        dev.harmonic_sens(w, quick, quick, max_iter=8)
    assert e.value.code == _capi.PL_ERR_NOCONV
    out = dev.harmonic_sens(w, quick, quick, max_iter=8, raise_on_noconv=False)
    assert out["J"] is None and out["dJ_dr"] is None and out["status"].tolist() == [[0, 1, 0], [0, 1, 0]]
    rc, iters, relres, status = run(quick, quick, MAX_ITER)                          # the handle is still usable
    assert rc == _capi.PL_OK and not status.any() and J.value > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. LatticeSim and LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
_tower = {}


def _tower_band():
    """omega_1 of the clamped 2 x 2 x 3 BCC tower of the presets below, from the dense eigen-solution, and a band of eight
    frequencies (Hz) around it: computed once."""
    if not _tower:
        L = LatticeSim(_preset("BCC", (2, 2, 3)))
        solve_FEM_FenicsX(L, rtol=1e-10)
        n = L.lattice.n_nodes
        fixed = np.asarray(L.fixed_DOF).reshape(n, 6) != 0
        L._device.set_mass(RHO)
        w1 = float(np.sqrt(L._device.vibration_modes_host(fixed, 1, dense=True)["omega2"][0]))
        _tower.update(w1=w1, hz=np.linspace(0.8, 1.2, 8) * w1 / (2.0 * np.pi), damping=(0.05 * w1, 0.002 / w1))
    return _tower


def test_lattice_sim_frequency_response_sensitivity():
    L = LatticeSim(_preset("BCC", (2, 2, 3)))
    with pytest.raises(RuntimeError):
        L.frequency_response_sensitivity()
    solve_FEM_FenicsX(L, rtol=1e-10)
    with pytest.raises(RuntimeError):
        L.frequency_response_sensitivity()
    n = L.lattice.n_nodes
    t = _tower_band()
    hz, damping = t["hz"], t["damping"]
    kw = dict(ray_m=damping[0], ray_k=damping[1], rtol=RTOL, max_iter=MAX_ITER)
    # a shaken base: the load follows the design
    L.frequency_response(hz, RHO, damping=damping, base_acceleration=0, rtol=RTOL, max_iter=MAX_ITER)
    node = int(L._frf_probes[0])
    got = L.frequency_response_sensitivity((node, 0))
    l = np.zeros((n, 6))
    l[node, 0] = 1.0
    want = L._device.harmonic_sens(2.0 * np.pi * hz, None, l, 2, 8.0, base_dir=(1, 0, 0), **kw)
    assert got["J"] == want["J"] and got["J"] >= np.abs(got["y"]).max() > 0
    assert np.array_equal(got["y"], want["y"]) and np.array_equal(got["dJ_dr"], want["dJ_dr"])
    assert got["dJ_dr"].shape == (L.lattice.n_beams,) and np.abs(got["dJ_dr"]).max() > 0
    assert np.array_equal(got["y"], L.frf_probe[:, 0, 0])           # that entry of the probed response, bit for bit
    arr = L.frequency_response_sensitivity(l, kind=1, weight=np.linspace(0.0, 1.0, hz.size))
    one = L.frequency_response_sensitivity((node, 0), kind=1, weight=np.linspace(0.0, 1.0, hz.size))
    assert arr["J"] == one["J"] and np.array_equal(arr["dJ_dr"], one["dJ_dr"])
    # the force set as the load, the default output: the load itself
    L.frequency_response(hz, RHO, damping=damping, rtol=RTOL, max_iter=MAX_ITER)
    force = np.zeros((n, 6))
    force[:, :3] = L.applied_force[:n, :3]
    got = L.frequency_response_sensitivity(kind=0, weight=np.pi * hz)
    want = L._device.harmonic_sens(2.0 * np.pi * hz, force, None, 0, 8.0, np.pi * hz, **kw)
    assert got["J"] == want["J"] > 0 and np.array_equal(got["dJ_dr"], want["dJ_dr"]) and not got["iters"][1].any()
    assert np.abs(got["y"] - (L.frf_power[:, 0] + 1j * L.frf_power[:, 1])).max() <= 1e-12 * np.abs(got["y"]).max()
    with pytest.raises(NotImplementedError):
        LatticeSim(_preset("BCC", (2, 2, 2)), reference_compat=True).frequency_response_sensitivity()
    p = _preset("BCC", (2, 2, 2))
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError):
        LatticeSim(p, enable_domain_decomposition_solver=True).frequency_response_sensitivity()


OPTI = _preset("BCC", (2, 2, 3))
OPTI["boundary_conditions"]["Force"]["Load"].update(DOF=["X"], Value=[0.02])
OPTI["optimization_informations"] = {
    "objective_function": "min", "objective_type": "compliance", "max_iterations": 3,
    "optimization_parameters": {"type": "linear", "direction": ["x", "z"]},
    "constraints": {"relative_density": {"value": 0.2}},
    "enable_parameter_normalization": True, "enable_gradient_computing": True, "simulation_type": "FEM"}


def _opti(constraints, **opt):
    p = copy.deepcopy(OPTI)
    p["optimization_informations"].update(opt)
    p["optimization_informations"]["constraints"].update(constraints)
    return p


def _peak(**kw):
    t = _tower_band()
    return dict(dict(max_amplitude=1.0, frequencies_hz=t["hz"].tolist(), density=RHO, damping=list(t["damping"]), p=8,
                     rtol=1e-12, max_iter=MAX_ITER), **kw)


def test_resonance_peak_constraint_gradient():
    """resonance_peak_constraint_gradient against central differences of resonance_peak_constraint in the three variables of
    the linear parameterisation, step 1e-4, within 1e-3 relative (the step and bar of the frequency and the peak displacement
    constraints), for the lateral tip load read at a top node and for a shaken base read through the load itself."""
    top_node = int(np.argmax(np.asarray(LatticeOpti(_opti({})).lattice.node_xyz).reshape(-1, 3)[:, 2]))
    for extra in (dict(output=[top_node, 0]), dict(base_acceleration=[1, 0, 0])):
        L = LatticeOpti(_opti({"resonance_peak": _peak(max_amplitude=0.5, **extra)}))
        assert "resonance_peak" in L._history
        theta = [0.2, -0.1, 0.5]
        L.objective(theta)
        g = L.resonance_peak_constraint_gradient(theta)
        assert g.shape == (L.number_parameters,) == (3,) and np.abs(g).max() > 0
        J, peak = L._last_resonance_peak
        assert J >= peak > 0 and abs(J / 0.5 - 1.0 - L.resonance_peak_constraint(theta)) <= 1e-12
        h = 1e-4
        for i in range(3):
            tp, tm = list(theta), list(theta)
            tp[i] += h
            tm[i] -= h
            fd = (L.resonance_peak_constraint(tp) - L.resonance_peak_constraint(tm)) / (2 * h)
            print(f"\n{sorted(extra)} variable {i}: gradient {g[i]:.8e}, difference quotient {fd:.8e}, relative difference "
                  f"{abs(g[i] / fd - 1):.2e}")
            assert abs(g[i] - fd) <= 1e-3 * abs(fd), (i, g[i], fd)
    assert "resonance_peak" not in LatticeOpti(_opti({}))._history


def test_three_iterations_lower_a_violated_resonance_peak():
    """max_amplitude = 0.9 J_p of the start (an infeasible start) under a volume bound with room to grow: three SLSQP
    iterations lower the constraint value, and every iteration records the peak."""
    probe = LatticeOpti(_opti({"resonance_peak": _peak()}))
    probe._initialize_optimization_solver()
    x0 = probe.initial_parameters
    J0 = probe.resonance_peak_constraint(x0) + 1.0
    rho0 = probe.relative_density()
    assert J0 >= probe._last_resonance_peak[1] > 0
    L = LatticeOpti(_opti({"resonance_peak": _peak(max_amplitude=0.9 * J0), "relative_density": {"value": 1.5 * rho0}}))
    c0 = L.resonance_peak_constraint(x0)
    assert c0 == pytest.approx(1.0 / 0.9 - 1.0, rel=1e-9)
    L.redefine_optim_parameters(max_iteration=3, disp=False)
    sol = L.optimize_lattice()
    assert len(L.constraints) == 2
    c = L.resonance_peak_constraint(sol.x)
    print(f"\nJ_p at the start {J0:.6g}, bound {0.9 * J0:.6g}; after {sol.nit} iterations: constraint {c0:.3e} -> {c:.3e}, peak "
          f"{L._last_resonance_peak[1]:.6g}, relative density {L.relative_density():.5f} (bound {1.5 * rho0:.5f})")
    assert c < c0
    hist = L._history["resonance_peak"]
    assert len(hist) == len(L._history["iteration"]) >= 1 and all(v is None or v > 0 for v in hist)
    assert any(v is not None for v in hist)


def test_ddm_mode_refuses_the_key():
    p = _opti({"resonance_peak": _peak()}, simulation_type="DDM")
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError, match="resonance_peak"):
        LatticeOpti(p)
