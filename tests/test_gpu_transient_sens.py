"""Transient sensitivities on the device (pl_transient_sens, csrc/pl_dyn_sens.h) against the numpy /
scipy restatement (dynamics_host.newmark_sensitivity) on the handle's own K, against central differences through
pl_update_radii + pl_assemble, against pl_transient (the forward pass), the determinism of the contraction, the handle's
state, the chunks of the adjoint, the error codes and the way up through LatticeSim.

The lattices are those of tests/test_mass_host.py (A, B, C); dt = T_1 / 40 with T_1 from the dense eigen-solution, 40 steps,
rtol = 1e-12, the damped (0.05 omega_1, 0.002 / omega_1) and the undamped average-acceleration scheme, and once beta = 0.31,
gamma = 0.6.  Bars: 1e-8 of each quantity's largest magnitude against the restatement (the bar of the histories in
tests/test_gpu_transient.py); h = 1e-6 and 1e-5 of the largest central difference (tests/test_mass_host.py)."""
import copy

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

N_STEPS, RTOL, MAX_ITER = 40, 1e-12, 5000
T = _capi.TRANSIENT_SENS_CHUNK


def _device(c, **kw):
    dev = _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN, beam_mult=c.mult, **kw)
    dev.set_bc(c.fixed)
    dev.assemble()
    dev.set_mass(RHO, True, c.node_mass)
    return dev


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


class _Case:
    """One lattice with a handle per node ordering, omega_1 of its own K and the restated M, a step load on the top face, a
    half-sine base acceleration, a generic output vector and a start state: computed once, shared, left unchanged."""

    def __init__(self, name):
        self.name, self.c = name, case(name)
        c = self.c
        self.devs = {r: _device(c, reorder=r) for r in (0, 1)}
        dev = self.devs[0]
        dev.assemble_bsr(False)
        rowptr, col, vals = dev.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * c.n, 6 * c.n)).tocsr()
        K.sum_duplicates()
        free = np.flatnonzero(~c.fixed.reshape(-1))
        Kf = K[free][:, free].toarray()
        Mf = sp.csr_matrix(dev.mass_matrix_host())[free][:, free].toarray()
        om2, phi = scipy.linalg.eigh(Kf, Mf, subset_by_index=[0, 0])
        self.w1 = float(np.sqrt(om2[0]))
        self.dt = 2.0 * np.pi / self.w1 / 40.0
        self.damping = (0.05 * self.w1, 0.002 / self.w1)
        top = np.flatnonzero(c.xyz[:, 2] > c.xyz[:, 2].max() - 1e-9)
        f = np.zeros((c.n, 6))
        f[top, 0], f[top, 2] = 0.03, -0.1
        self.load = np.where(c.fixed, 0.0, f)
        self.top = top
        u_static = np.linalg.solve(Kf, self.load.reshape(-1)[free])
        self.u0, self.v0 = np.zeros(6 * c.n), np.zeros(6 * c.n)
        self.u0[free] = 0.3 * np.abs(u_static).max() / np.abs(phi[:, 0]).max() * phi[:, 0]
        self.v0[free] = 0.2 * self.w1 * u_static
        self.u0, self.v0 = self.u0.reshape(c.n, 6), self.v0.reshape(c.n, 6)
        self.l = np.random.default_rng(7).standard_normal((c.n, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
        self.base_dir = np.array([0.6, 0.0, 0.8])
        self.weights = 0.5 + np.random.default_rng(3).random(N_STEPS + 1)

    def base_acc(self, n_steps=N_STEPS):
        t = self.dt * np.arange(n_steps + 1)
        return np.where(t < 20 * self.dt, 0.4 * np.sin(np.pi * t / (20 * self.dt)), 0.0)

    def args(self, kind, damped=True, base=True, n_steps=N_STEPS, weight="w", start=False, scheme=(0.25, 0.5)):
        """the keyword arguments transient_sens and transient_sens_host share"""
        rm, rk = self.damping if damped else (0.0, 0.0)
        if isinstance(weight, str):
            weight = None if kind == 2 else self.weights[: n_steps + 1]
        kw = dict(dt=self.dt, n_steps=n_steps, out_vec=self.l, kind=kind, p=8.0, weight=weight, patterns=self.load[None],
                  amp=np.ones((n_steps + 1, 1)), beta=scheme[0], gamma=scheme[1], ray_m=rm, ray_k=rk)
        if base:
            kw.update(base_dir=self.base_dir, base_acc=self.base_acc(n_steps))
        if start:
            kw.update(u0=self.u0, v0=self.v0)
        return kw

    def both(self, reorder, **kw):
        a = self.args(**kw)
        got = self.devs[reorder].transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
        ref = self.devs[reorder].transient_sens_host(self.c.fixed, **a)
        return got, ref


_cases = {}


def _get(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _errors(got, ref):
    return {"J": abs(got["J"] - ref["J"]) / abs(ref["J"]), "y": _rel(got["y"], ref["y"]), "dJ_dr": _rel(got["dJ_dr"], ref["dJ_dr"])}


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_equals_the_restatement(name, reorder, damped, base):
    d = _get(name)
    for kind in (0, 1, 2):
        got, ref = d.both(reorder, kind=kind, damped=damped, base=base)
        assert got["y"].shape == (N_STEPS + 1,) and got["dJ_dr"].shape == (d.c.B,) and got["iters"].shape == (2, N_STEPS + 1)
        errs = _errors(got, ref)
        it = got["iters"]
        print(f"\n{name} reorder={reorder} damped={damped} base={base} kind {kind}: {errs}; iterations forward "
              f"{it[0, 1:].min()} - {it[0, 1:].max()}, adjoint {it[1, 1:].min()} - {it[1, 1:].max()}")
        assert max(errs.values()) <= 1e-8, errs
        assert it.max() < MAX_ITER and it[:, 1:].min() > 0


def test_general_scheme_with_a_start_state():
    """beta = 0.31, gamma = 0.6: c3 != cv and c2 != cu, so no coefficient of the recursion hides behind another."""
    d = _get("A")
    for kind in (0, 1, 2):
        got, ref = d.both(1, kind=kind, start=True, scheme=(0.31, 0.6))
        errs = _errors(got, ref)
        print(f"\nA general scheme kind {kind}: {errs}")
        assert max(errs.values()) <= 1e-8, errs


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_central_differences_through_update_radii():
    """Eight struts of A, strut 3 (multiplicity 2) and the penalised struts among them: two calls per strut at r +- 1e-6
    through pl_update_radii + pl_assemble, all three objectives from the y of those calls, kind 2 also from the call's own J."""
    d = _get("A")
    c = d.c
    struts = [0, 3, 17, 31, 46, 58, 77, 95]
    assert c.mult[3] == 2.0 and (c.sl[struts][:, [0, 2]] > 0).any()
    h = 1e-6
    a = d.args(kind=2, start=True)
    cases = [(0, d.weights, 8.0), (1, d.weights, 8.0), (2, None, 8.0)]
    with _device(c) as dev:
        grads = [dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **d.args(kind=k, start=True))["dJ_dr"] for k, _, _ in cases]
        fd, fd_own = np.zeros((3, len(struts))), np.zeros(len(struts))
        for i, b in enumerate(struts):
            side = []
            for sg in (+1.0, -1.0):
                r = c.radius.copy()
                r[b] += sg * h
                dev.update_radii(r)
                dev.assemble()
                side.append(dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a))
            for q, (k, w, p) in enumerate(cases):
                fd[q, i] = (DH.objective(side[0]["y"], k, p, w)[0] - DH.objective(side[1]["y"], k, p, w)[0]) / (2.0 * h)
            fd_own[i] = (side[0]["J"] - side[1]["J"]) / (2.0 * h)
    for q, (k, _, _) in enumerate(cases):
        err = np.abs(grads[q][struts] - fd[q]).max() / np.abs(fd[q]).max()
        print(f"\nkind {k}: device gradient within {err:.2e} of the largest central difference")
        assert err <= 1e-5
    assert np.abs(grads[2][struts] - fd_own).max() <= 1e-5 * np.abs(fd_own).max()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the forward pass is pl_transient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [False, True])
def test_outputs_are_the_history_of_pl_transient(base):
    """y of an output vector with one entry is that entry of pl_transient's u history bit for bit (a sum with one non-zero
    term has no order); a generic output vector agrees within the rounding of a 6N-term dot product."""
    d = _get("A")
    c, dev = d.c, d.devs[1]
    every = np.arange(c.n, dtype=np.int32)
    rm, rk = d.damping
    pats, amp = d.load[None], np.ones((N_STEPS + 1, 1))
    if base:
        e = np.zeros((1, c.n, 6))
        e[0, :, :3] = d.base_dir
        pats, amp = np.concatenate([pats, -dev.mass_spmv_multi(e)]), np.column_stack([amp, d.base_acc()])
    hist = dev.transient(d.dt, N_STEPS, pats, amp, u0=d.u0, v0=d.v0, ray_m=rm, ray_k=rk, rtol=RTOL, max_iter=MAX_ITER,
                         probes=every)
    u = hist["probe"][:, 0]
    node, dof = int(d.top[1]), 2
    a = d.args(kind=2, base=base, start=True)
    for scale in (1.0, -2.5):
        l = np.zeros((c.n, 6))
        l[node, dof] = scale
        a["out_vec"] = l
        got = dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
        assert np.array_equal(got["y"], scale * u[:, node, dof]) and np.abs(got["y"]).max() > 0
        assert np.array_equal(got["iters"][0], hist["iters"])
    a["out_vec"] = d.l
    got = dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
    lm = np.where(c.fixed, 0.0, d.l)
    want = (u * lm[None]).sum(axis=(1, 2))
    assert np.abs(got["y"] - want).max() <= 1e-13 * (np.abs(u) * np.abs(lm)[None]).sum(axis=(1, 2)).max()


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism and the handle's state
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits_and_the_handle_keeps_its_state():
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
        for kind in (0, 1, 2):
            a = d.args(kind=kind, start=True)
            one = dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
            two = dev.transient_sens(rtol=RTOL, max_iter=MAX_ITER, **a)
            assert one["J"] == two["J"] and np.abs(one["dJ_dr"]).max() > 0
            for q in ("y", "dJ_dr", "iters"):
                assert np.array_equal(one[q], two[q]), (kind, q)
        kw = dict(ray_m=d.damping[0], ray_k=d.damping[1], rtol=1e-10, probes=[1, 2])
        after = []
        for q in (dev, twin):
            u, st = q.solve(rtol=1e-12, max_iter=100000)
            modes = q.vibration_modes(3, n_sub=8)
            tr = q.transient(d.dt, 10, f[None], np.ones((11, 1)), **kw)
            after.append((u, st["iterations"], modes, tr))
        assert np.array_equal(after[0][0], after[1][0]) and after[0][1] == after[1][1]
        assert np.array_equal(after[0][2]["omega2"], after[1][2]["omega2"])
        assert np.array_equal(after[0][2]["modes"], after[1][2]["modes"])
        for q in ("probe", "energy", "state", "iters"):
            assert np.array_equal(after[0][3][q], after[1][3][q]), q


# ---------------------------------------------------------------------------------------------------------------------
# 5. row 0 and the chunks of the adjoint
# ---------------------------------------------------------------------------------------------------------------------
def test_weights_on_row_0_alone_give_exact_zeros():
    d = _get("A")
    w0 = np.zeros(N_STEPS + 1)
    w0[0] = 1.0
    for kind in (0, 1, 2):
        got = d.devs[1].transient_sens(rtol=RTOL, max_iter=MAX_ITER, **d.args(kind=kind, weight=w0, start=True))
        assert got["J"] != 0.0 and not got["dJ_dr"].any() and not got["iters"][1].any()


@pytest.mark.parametrize("n_steps", [T - 1, T, T + 1, 2 * T])
def test_chunk_lengths_agree_with_the_restatement(n_steps):
    """n_steps + 1 rows around the chunk of the adjoint: one full chunk, one row more, two rows more, two full chunks and a row."""
    d = _get("C")
    for kind in (0, 2):
        got, ref = d.both(1, kind=kind, n_steps=n_steps, weight=None, start=True)
        errs = _errors(got, ref)
        print(f"\nC n_steps {n_steps} kind {kind}: {errs}")
        assert max(errs.values()) <= 1e-8, errs


# ---------------------------------------------------------------------------------------------------------------------
# 6. error codes
# ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = case("A")
    lib, p = _capi.load_library(), _capi._ptr
    n6 = 6 * c.n
    OK, ARG, STATE, NOCONV = _capi.PL_OK, _capi.PL_ERR_ARG, _capi.PL_ERR_STATE, _capi.PL_ERR_NOCONV
    pat = np.zeros((1, c.n, 6))
    pat[0, c.n - 1, 2] = -0.1
    amp = np.ones((6, 1))
    l = np.zeros((c.n, 6))
    l[c.n - 1, 2] = 1.0
    bdir, bacc = np.array([0.0, 0.0, 1.0]), np.linspace(0.0, 1.0, 6)
    import ctypes as C
    J = C.c_double(-7.0)
    y, grad, iters = np.full(6, -7.0), np.full(c.B, -7.0), np.full((2, 6), -7, np.int32)

    def run(h, n_steps=5, dt=0.1, beta=0.25, gamma=0.5, rm=0.0, rk=0.0, n_pat=1, pat_=pat, amp_=amp, bd=None, ba=None,
            rtol=1e-8, it=5000, l_=l, kind=2, pp=8.0, w=None, J_=J, y_=y, g_=grad):
        return lib.pl_transient_sens(h, n_steps, dt, beta, gamma, rm, rk, n_pat, p(pat_), p(amp_), p(bd), p(ba), None, None,
                                     rtol, it, p(l_), kind, pp, p(w), C.byref(J_) if J_ is not None else None, p(y_), p(g_),
                                     p(iters))

    assert run(None) == ARG
    with _capi.HipLattice(c.xyz, c.conn, c.radius, c.sl, c.sn, E, NU, kappa=KAPPA, pen_coef=PEN) as dev:
        h = dev._h
        assert run(h) == STATE                                                       # before pl_assemble
        dev.assemble()
        assert run(h) == STATE and b"pl_set_bc" in lib.pl_last_error()
        dev.set_bc(c.fixed)
        assert run(h) == STATE and b"pl_set_mass" in lib.pl_last_error()
        dev.set_mass(RHO)
        assert J.value == -7.0 and (y == -7.0).all() and (grad == -7.0).all() and (iters == -7).all()
        assert run(h) == OK and J.value > 0 and np.abs(grad).max() > 0
        assert run(h, y_=None) == OK
        assert run(h, n_steps=0) == ARG and run(h, dt=0.0) == ARG and run(h, dt=-0.1) == ARG
        assert run(h, gamma=0.49) == ARG and run(h, beta=0.24) == ARG and run(h, gamma=0.6, beta=0.3) == ARG
        assert b"stable" in lib.pl_last_error()
        assert run(h, gamma=0.6, beta=0.31) == OK
        assert run(h, rm=-1e-3) == ARG and run(h, rk=-1e-3) == ARG
        assert run(h, n_pat=5, pat_=np.zeros((5, n6)), amp_=np.ones((6, 5))) == ARG
        assert run(h, pat_=None) == ARG and run(h, amp_=None) == ARG
        assert run(h, rtol=0.0) == ARG and run(h, it=0) == ARG
        assert run(h, kind=-1) == ARG and run(h, kind=3) == ARG
        assert run(h, pp=1.5) == ARG and run(h, kind=1, pp=1.5) == OK and run(h, pp=2.0) == OK
        assert run(h, w=np.array([1, 1, -1e-3, 1, 1, 1.0])) == ARG and b"weight" in lib.pl_last_error()
        assert run(h, w=np.array([1, 0, 0, 2, 1, 1.0])) == OK
        assert run(h, l_=None) == ARG and run(h, J_=None) == ARG and run(h, g_=None) == ARG
        assert run(h, bd=bdir) == ARG and b"base_acc" in lib.pl_last_error()
        assert run(h, bd=bdir, ba=bacc) == OK
        assert run(h, n_pat=0, pat_=None, amp_=None, bd=bdir, ba=bacc) == OK and J.value > 0     # the base load alone
        assert run(h, n_pat=0, pat_=None, amp_=None) == OK and J.value == 0.0 and not grad.any()  # nothing moves
        J.value = -7.0
        y[:], grad[:], iters[:] = -7.0, -7.0, -7
        assert run(h, it=1, rtol=1e-12) == NOCONV
        assert b"forward solve of step 0" in lib.pl_last_error()
        assert J.value == -7.0 and (y == -7.0).all() and (grad == -7.0).all() and (iters == -7).all()
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
        assert run(ddm._h, pat_=np.zeros((1, 12)), l_=np.ones(12), g_=np.zeros(8)) == STATE
    finally:
        ddm.close()
    from pylatticedso_amd.loopback import LoopbackGroup
    with LoopbackGroup((1, 1, 1), (4, 2, 2), ["BCC"], [0.05], 2, axis=0, young=E, poisson=NU) as g:
        for dev in g.devs:
            m6 = 6 * dev.n_nodes
            assert run(dev._h, pat_=np.zeros((1, m6)), l_=np.ones(m6), g_=np.zeros(dev.n_beams)) == STATE
            assert b"multi-rank" in lib.pl_last_error()


def test_adjoint_pass_names_its_row_when_it_misses_rtol():
    """A forward pass that needs no iteration (no load, nothing moves) and an adjoint pass that does (kind 0: c_n = w_n
    whatever y is): max_iter = 1 stops in the adjoint solve of the last row, and nothing is written."""
    d = _get("A")
    c = d.c
    with pytest.raises(RuntimeError, match="adjoint solve of step 5"):
        d.devs[1].transient_sens(d.dt, 5, d.l, kind=0, rtol=1e-12, max_iter=1)
    got = d.devs[1].transient_sens(d.dt, 5, d.l, kind=0, rtol=1e-12, max_iter=MAX_ITER)
    assert got["J"] == 0.0 and not got["y"].any() and not got["iters"][0].any() and got["iters"][1, 1:].min() > 0
    assert got["dJ_dr"].shape == (c.B,)


# ---------------------------------------------------------------------------------------------------------------------
# 7. LatticeSim and LatticeOpti
# ---------------------------------------------------------------------------------------------------------------------
_tower = {}


def _tower_step():
    """dt = T_1 / 40 of the clamped 2 x 2 x 3 BCC tower of the presets below, from the dense eigen-solution: computed once."""
    if not _tower:
        L = LatticeSim(_preset("BCC", (2, 2, 3)))
        solve_FEM_FenicsX(L, rtol=1e-10)
        n = L.lattice.n_nodes
        fixed = np.asarray(L.fixed_DOF).reshape(n, 6) != 0
        L._device.set_mass(RHO)
        w1 = float(np.sqrt(L._device.vibration_modes_host(fixed, 1, dense=True)["omega2"][0]))
        _tower.update(w1=w1, dt=2.0 * np.pi / w1 / 40.0)
    return _tower


def test_lattice_sim_transient_sensitivity():
    L = LatticeSim(_preset("BCC", (2, 2, 3)))
    with pytest.raises(RuntimeError):
        L.transient_sensitivity()
    solve_FEM_FenicsX(L, rtol=1e-10)
    with pytest.raises(RuntimeError):
        L.transient_sensitivity()
    n = L.lattice.n_nodes
    t = _tower_step()
    dt, damping = t["dt"], (0.05 * t["w1"], 0.002 / t["w1"])
    a_g = 0.3 * np.sin(np.pi * np.arange(N_STEPS + 1) / N_STEPS)
    L.transient_response(dt, N_STEPS, RHO, base_acceleration=((1, 0, 0), a_g), damping=damping, rtol=RTOL)
    force = np.zeros((n, 6))
    force[:, :3] = L.applied_force[:n, :3]
    kw = dict(patterns=force[None], amp=np.ones((N_STEPS + 1, 1)), base_dir=(1, 0, 0), base_acc=a_g, ray_m=damping[0],
              ray_k=damping[1], rtol=RTOL)
    # the default output: the force pattern scaled to unit norm, the p-norm over time with p = 8
    got = L.transient_sensitivity()
    want = L._device.transient_sens(dt, N_STEPS, force / np.linalg.norm(force), 2, 8.0, **kw)
    assert got["J"] == want["J"] and got["J"] >= np.abs(got["y"]).max() > 0
    assert np.array_equal(got["y"], want["y"]) and np.array_equal(got["dJ_dr"], want["dJ_dr"])
    assert got["dJ_dr"].shape == (L.lattice.n_beams,)
    # a (node, dof) output is that entry of the probed history of the response, and an array output is read as it is
    node = int(L._transient_probes[0])
    one = L.transient_sensitivity((node, 0), kind=1, weight=np.linspace(0.0, 1.0, N_STEPS + 1))
    assert np.array_equal(one["y"], L.transient_probe[:, 0, 0, 0])
    l = np.zeros((n, 6))
    l[node, 0] = 1.0
    arr = L.transient_sensitivity(l, kind=1, weight=np.linspace(0.0, 1.0, N_STEPS + 1))
    assert arr["J"] == one["J"] and np.array_equal(arr["dJ_dr"], one["dJ_dr"])
    with pytest.raises(NotImplementedError):
        LatticeSim(_preset("BCC", (2, 2, 2)), reference_compat=True).transient_sensitivity()
    p = _preset("BCC", (2, 2, 2))
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError):
        LatticeSim(p, enable_domain_decomposition_solver=True).transient_sensitivity()


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
    t = _tower_step()
    return dict(dict(max_displacement=1.0, dt=t["dt"], n_steps=N_STEPS, density=RHO, damping=[0.05 * t["w1"], 0.002 / t["w1"]],
                     p=8, rtol=1e-12), **kw)


def test_peak_displacement_constraint_gradient():
    """peak_displacement_constraint_gradient against central differences of peak_displacement_constraint in the three
    variables of the linear parameterisation, step 1e-4, within 1e-3 relative (the step and bar of the frequency and the
    global buckling constraints), under a suddenly applied lateral tip load plus a base acceleration."""
    a_g = (0.2 * np.sin(np.pi * np.arange(N_STEPS + 1) / 20.0)).tolist()
    L = LatticeOpti(_opti({"peak_displacement": _peak(max_displacement=0.5, base_acceleration=[[1, 0, 0], a_g])}))
    assert "peak_displacement" in L._history
    theta = [0.2, -0.1, 0.5]
    L.objective(theta)
    g = L.peak_displacement_constraint_gradient(theta)
    assert g.shape == (L.number_parameters,) == (3,) and np.abs(g).max() > 0
    J, peak = L._last_peak_displacement
    assert J >= peak > 0 and abs(J / 0.5 - 1.0 - L.peak_displacement_constraint(theta)) <= 1e-12
    h = 1e-4
    for i in range(3):
        tp, tm = list(theta), list(theta)
        tp[i] += h
        tm[i] -= h
        fd = (L.peak_displacement_constraint(tp) - L.peak_displacement_constraint(tm)) / (2 * h)
        print(f"\nvariable {i}: gradient {g[i]:.8e}, difference quotient {fd:.8e}, relative difference {abs(g[i] / fd - 1):.2e}")
        assert abs(g[i] - fd) <= 1e-3 * abs(fd), (i, g[i], fd)
    assert "peak_displacement" not in LatticeOpti(_opti({}))._history


def test_three_iterations_lower_a_violated_peak_displacement():
    """max_displacement = 0.9 J_p of the start (an infeasible start) under a volume bound with room to grow: three SLSQP
    iterations lower the constraint value, and every iteration records the peak."""
    probe = LatticeOpti(_opti({"peak_displacement": _peak()}))
    probe._initialize_optimization_solver()
    x0 = probe.initial_parameters
    J0 = probe.peak_displacement_constraint(x0) + 1.0
    rho0 = probe.relative_density()
    assert J0 >= probe._last_peak_displacement[1] > 0
    L = LatticeOpti(_opti({"peak_displacement": _peak(max_displacement=0.9 * J0), "relative_density": {"value": 1.5 * rho0}}))
    c0 = L.peak_displacement_constraint(x0)
    assert c0 == pytest.approx(1.0 / 0.9 - 1.0, rel=1e-9)
    L.redefine_optim_parameters(max_iteration=3, disp=False)
    sol = L.optimize_lattice()
    assert len(L.constraints) == 2
    c = L.peak_displacement_constraint(sol.x)
    print(f"\nJ_p at the start {J0:.6g}, bound {0.9 * J0:.6g}; after {sol.nit} iterations: constraint {c0:.3e} -> {c:.3e}, peak "
          f"{L._last_peak_displacement[1]:.6g}, relative density {L.relative_density():.5f} (bound {1.5 * rho0:.5f})")
    assert c < c0
    hist = L._history["peak_displacement"]
    assert len(hist) == len(L._history["iteration"]) >= 1 and all(v is None or v > 0 for v in hist)
    assert any(v is not None for v in hist)


def test_ddm_mode_refuses_the_key():
    p = _opti({"peak_displacement": _peak()}, simulation_type="DDM")
    p["simulation_parameters"]["DDM"] = {"enable_preconditioner": False, "max_iterations": 1000,
                                         "schur_complement_computation": {"type": "exact"}}
    with pytest.raises(NotImplementedError, match="peak_displacement"):
        LatticeOpti(p)
