"""numpy / scipy restatement of the transient response (csrc/pl_dyn.h, pl_transient): implicit Newmark
time stepping of M a + C v + K u = f(t) on the free dofs, C = ray_m M + ray_k K, in acceleration form.  No device.

Step n -> n + 1 with dt:
    ut = u_n + dt v_n + dt^2 (1/2 - beta) a_n,   vt = v_n + dt (1 - gamma) a_n
    (M (1 + gamma dt ray_m) + K (beta dt^2 + gamma dt ray_k)) a_{n+1} = f_{n+1} - K ut - C vt
    u_{n+1} = ut + beta dt^2 a_{n+1},   v_{n+1} = vt + gamma dt a_{n+1}
and M a_0 = f_0 - K u_0 - C v_0.  With beta = 1/4, gamma = 1/2 (the average acceleration) an undamped mode of frequency omega
is carried with its amplitude kept and the phase ``newmark_phase(omega, dt)`` per step.

``harmonic`` restates the frequency response (csrc/pl_harm.h, pl_harmonic): the steady state under
f e^{iwt}, one complex symmetric system per frequency, with ``jacobi_cocg`` the device's solver."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp


def check_scheme(dt, n_steps, beta, gamma, ray_m=0.0, ray_k=0.0):
    """The argument checks of pl_transient: unconditionally stable implicit schemes only."""
    if not (dt > 0.0 and np.isfinite(dt)):
        raise ValueError("dt must be positive and finite")
    if int(n_steps) < 1:
        raise ValueError("n_steps must be at least 1")
    if not gamma >= 0.5:
        raise ValueError("gamma must be at least 1/2")
    if not beta >= 0.25 * (0.5 + gamma) ** 2:
        raise ValueError("beta must be at least (1/2 + gamma)^2 / 4 (unconditionally stable schemes only)")
    if not (ray_m >= 0.0 and ray_k >= 0.0):
        raise ValueError("the Rayleigh coefficients must not be negative")


def newmark_phase(omega, dt):
    """Phase advance per step of an undamped mode under the average-acceleration scheme: 2 atan(omega dt / 2)."""
    return 2.0 * np.arctan(0.5 * np.asarray(omega, float) * dt)


def jacobi_pcg(rtol, max_iter=100000, counts=None):
    """A ``solve`` for ``newmark``: Jacobi-preconditioned CG from a zero start to ||r|| <= rtol ||b||, the solver of the
    device.  counts: a list that receives the iterations of every solve."""
    def solve(S, b):
        dinv = 1.0 / S.diagonal()
        x = np.zeros_like(b)
        r = b.copy()
        bb = float(r @ r)
        it = 0
        if bb > 0.0:
            z = dinv * r
            p = z.copy()
            rz = float(r @ z)
            while it < max_iter:
                Ap = S @ p
                alpha = rz / float(p @ Ap)
                x += alpha * p
                r -= alpha * Ap
                it += 1
                if float(r @ r) <= rtol * rtol * bb:
                    break
                z = dinv * r
                rz_new = float(r @ z)
                p = z + (rz_new / rz) * p
                rz = rz_new
        if counts is not None:
            counts.append(it)
        return x
    return solve


def _dense_solver():
    cache = {}

    def solve(S, b):
        key = id(S)
        if key not in cache:
            cache.clear()
            cache[key] = (S, scipy.linalg.cho_factor(S.toarray() if sp.issparse(S) else np.asarray(S)))
        return scipy.linalg.cho_solve(cache[key][1], b)
    return solve


def newmark(K, M, fixed, dt, n_steps, patterns=None, amp=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0, ray_k=0.0,
            solve=None, probes=None, snap_every=0):
    """The arrays of pl_transient from the matrices K, M (6N x 6N, dense or sparse) and the mask fixed (N, 6) / (6N,).

    patterns (n_pat, 6N) or (n_pat, N, 6) with amp (n_steps + 1, n_pat) give the load f_n = amp[n] @ patterns; u0, v0 (6N,)
    or None = 0; all are read with the fixed dofs zeroed.  solve(S, b): the solver of the reduced systems (free dofs only);
    None = dense Cholesky, factorised once per matrix.  Returns a dict: u, v, a (n_steps + 1, N, 6) - the whole history -,
    probe (n_steps + 1, 3, n_probe, 6) for the node indices ``probes``, energy (n_steps + 1, 3) = kinetic, strain, external
    work (trapezoid), snaps (n_steps // snap_every, N, 6) if snap_every > 0, state (3, N, 6) and time (n_steps + 1,)."""
    check_scheme(dt, n_steps, beta, gamma, ray_m, ray_k)
    n_steps = int(n_steps)
    fx = np.asarray(fixed).reshape(-1) != 0
    n6 = fx.size
    free = np.flatnonzero(~fx)
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    Kf, Mf = K[free][:, free].tocsr(), M[free][:, free].tocsr()
    Cf = ray_m * Mf + ray_k * Kf
    if patterns is None:
        P = np.zeros((0, free.size))
        A = np.zeros((n_steps + 1, 0))
    else:
        P = np.asarray(patterns, float).reshape(-1, n6)[:, free]
        A = np.asarray(amp, float).reshape(n_steps + 1, P.shape[0])
    u = np.zeros(free.size) if u0 is None else np.asarray(u0, float).reshape(-1)[free].copy()
    v = np.zeros(free.size) if v0 is None else np.asarray(v0, float).reshape(-1)[free].copy()
    solve = solve or _dense_solver()
    S = ((1.0 + gamma * dt * ray_m) * Mf + (beta * dt * dt + gamma * dt * ray_k) * Kf).tocsr()

    U, V, Acc = (np.zeros((n_steps + 1, n6)) for _ in range(3))
    energy = np.zeros((n_steps + 1, 3))
    f = A[0] @ P
    a = solve(Mf, f - Kf @ u - Cf @ v)
    work = 0.0
    for n in range(n_steps + 1):
        if n > 0:
            ut = u + dt * v + dt * dt * (0.5 - beta) * a
            vt = v + dt * (1.0 - gamma) * a
            f_new = A[n] @ P
            a = solve(S, f_new - Kf @ ut - Cf @ vt)
            u_new = ut + beta * dt * dt * a
            v = vt + gamma * dt * a
            work += 0.5 * float((f + f_new) @ (u_new - u))
            u, f = u_new, f_new
        U[n, free], V[n, free], Acc[n, free] = u, v, a
        energy[n] = 0.5 * float(v @ (Mf @ v)), 0.5 * float(u @ (Kf @ u)), work
    N = n6 // 6
    out = {"u": U.reshape(-1, N, 6), "v": V.reshape(-1, N, 6), "a": Acc.reshape(-1, N, 6), "energy": energy,
           "time": dt * np.arange(n_steps + 1),
           "state": np.stack([U[-1], V[-1], Acc[-1]]).reshape(3, N, 6)}
    pr = np.zeros(0, int) if probes is None else np.asarray(probes, int).reshape(-1)
    out["probe"] = np.stack([out["u"][:, pr], out["v"][:, pr], out["a"][:, pr]], axis=1)
    if snap_every and snap_every > 0:
        out["snaps"] = out["u"][snap_every::snap_every][: n_steps // snap_every].copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Discrete adjoint of the scheme: radius sensitivities of one scalar output per row (csrc/pl_dyn_sens.h, pl_transient_sens;
# DESIGN.md section 10h)
# ---------------------------------------------------------------------------------------------------------------------
def objective(y, kind, p=8.0, weight=None):
    """(J, c) with c_n = dJ/dy_n for the outputs y (n_steps + 1,) and weights w >= 0 (None = 1):
    kind 0: J = sum w y, 1: J = 1/2 sum w y^2, 2: J = (sum w |y|^p)^(1/p), p >= 2 (c = 0 where J = 0)."""
    y = np.asarray(y, float).reshape(-1)
    w = np.ones_like(y) if weight is None else np.asarray(weight, float).reshape(-1)
    if w.shape != y.shape or (w < 0.0).any():
        raise ValueError("weight must have one entry per row and must not be negative")
    if kind == 0:
        return float(w @ y), w.copy()
    if kind == 1:
        return 0.5 * float(w @ (y * y)), w * y
    if kind == 2:
        if not p >= 2.0:
            raise ValueError("p must be at least 2")
        # scaled by the largest |y|: no overflow of |y|^p
        top = float(np.abs(y).max())
        if top == 0.0:
            return 0.0, np.zeros_like(y)
        s = np.abs(y) / top
        Js = float(w @ s ** p) ** (1.0 / p)
        if Js == 0.0:
            return 0.0, np.zeros_like(y)
        return top * Js, Js ** (1.0 - p) * w * s ** (p - 1.0) * np.sign(y)
    raise ValueError("kind must be 0, 1 or 2")


def newmark_sensitivity(K, M, fixed, conn, drec_dr, dM_dr, dt, n_steps, out_vec, kind=2, p=8.0, weight=None, patterns=None,
                        amp=None, base_dir=None, base_acc=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0, ray_k=0.0,
                        solve=None):
    """What pl_transient_sens computes: J of the outputs y_n = l . u_n of ``newmark`` and dJ/dr_b at fixed segment geometry
    by the discrete adjoint of the scheme (discretise, then differentiate).

    conn (B, 2), drec_dr (B, 8) the radius derivative of the condensed records (stress_host.drecords_dr) and dM_dr
    (B, 12, 12) that of the mass elements (mass_host.delement_matrix_dr) give dK_e/dr_b and dM_e/dr_b; out_vec = l (6N,) or
    (N, 6), read with the fixed dofs zeroed.  base_dir (3,) with base_acc (n_steps + 1,) adds the load -a_g[n] M e_dir, e_dir
    the rigid translation of ALL nodes: the only load that follows the design.  Point masses have no derivative.

    With c2 = dt^2 (1/2 - beta), c3 = dt (1 - gamma), cu = beta dt^2, cv = gamma dt and c_n = dJ/dy_n, mu = nu = 0, for
    n = N ... 1:
        S lam_n = (cu + cv dt + c2) mu + (cv + c3) nu - cu c_n l
        mu, nu <- mu - c_n l - K lam_n,  nu + dt mu - C lam_n            (the OLD mu on the right)
    and M lam_0 = c2 mu + c3 nu;
        dJ/dr_b = sum_n lam_n,e^T dK_e (u_n + ray_k v_n)_e + lam_n,e^T dM_e (a_n + ray_m v_n + a_g[n] e_dir)_e.
    Returns a dict: J, y (n_steps + 1,), dJ_dr (B,), lam (n_steps + 1, N, 6), c (n_steps + 1,)."""
    from . import geometric_host as GH
    n_steps = int(n_steps)
    fx = np.asarray(fixed).reshape(-1) != 0
    n6 = fx.size
    N = n6 // 6
    free = np.flatnonzero(~fx)
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    P = np.zeros((0, n6)) if patterns is None else np.asarray(patterns, float).reshape(-1, n6)
    A = np.zeros((n_steps + 1, 0)) if patterns is None else np.asarray(amp, float).reshape(n_steps + 1, P.shape[0])
    e_dir = np.zeros((N, 6))
    a_g = np.zeros(n_steps + 1)
    if base_dir is not None:
        if base_acc is None:
            raise ValueError("base_dir needs base_acc")
        e_dir[:, :3] = np.asarray(base_dir, float).reshape(3)
        a_g = np.asarray(base_acc, float).reshape(n_steps + 1)
        P = np.vstack([P, -(M @ e_dir.reshape(-1))[None]])
        A = np.column_stack([A, a_g])
    fwd = newmark(K, M, fixed, dt, n_steps, P if P.shape[0] else None, A if P.shape[0] else None, u0, v0, beta, gamma,
                  ray_m, ray_k, solve)
    U, V, Acc = (fwd[q].reshape(n_steps + 1, n6) for q in "uva")
    l = np.where(fx, 0.0, np.asarray(out_vec, float).reshape(-1))
    y = U @ l
    J, c = objective(y, kind, p, weight)

    Kf, Mf = K[free][:, free].tocsr(), M[free][:, free].tocsr()
    Cf = ray_m * Mf + ray_k * Kf
    S = ((1.0 + gamma * dt * ray_m) * Mf + (beta * dt * dt + gamma * dt * ray_k) * Kf).tocsr()
    solve = solve or _dense_solver()
    c2, c3, cu, cv = dt * dt * (0.5 - beta), dt * (1.0 - gamma), beta * dt * dt, gamma * dt
    lf = l[free]
    mu, nu = np.zeros(free.size), np.zeros(free.size)
    lam = np.zeros((n_steps + 1, n6))
    for n in range(n_steps, 0, -1):
        x = solve(S, (cu + cv * dt + c2) * mu + (cv + c3) * nu - cu * c[n] * lf)
        lam[n, free] = x
        mu, nu = mu - c[n] * lf - Kf @ x, nu + dt * mu - Cf @ x
    lam[0, free] = solve(Mf, c2 * mu + c3 * nu)

    conn = np.asarray(conn).reshape(-1, 2)
    drec = np.asarray(drec_dr, float).reshape(-1, 8)
    dM = np.asarray(dM_dr, float).reshape(-1, 12, 12)
    ia, ib = conn[:, 0], conn[:, 1]
    wK = (U + ray_k * V).reshape(-1, N, 6)
    wM = (Acc + ray_m * V).reshape(-1, N, 6) + a_g[:, None, None] * e_dir[None]
    lam3 = lam.reshape(-1, N, 6)
    grad = np.zeros(len(conn))
    for n in range(n_steps + 1):
        le = np.concatenate([lam3[n][ia], lam3[n][ib]], axis=1)
        we = np.concatenate([wM[n][ia], wM[n][ib]], axis=1)
        grad += GH._pairing(drec, conn, wK[n], lam3[n]) + np.einsum("bi,bij,bj->b", le, dM, we)
    return {"J": J, "y": y, "dJ_dr": grad, "lam": lam3, "c": c}


# ---------------------------------------------------------------------------------------------------------------------
# Frequency response: the steady state under a harmonic load (csrc/pl_harm.h, pl_harmonic)
# ---------------------------------------------------------------------------------------------------------------------
def harmonic_coefficients(omegas, ray_m=0.0, ray_k=0.0):
    """(c_K, c_M) of A(w) = c_K K + c_M M: c_K = 1 + i w ray_k, c_M = i w ray_m - w^2, with the argument checks of pl_harmonic."""
    w = np.atleast_1d(np.asarray(omegas, float)).reshape(-1)
    if w.size < 1:
        raise ValueError("at least one frequency is needed")
    if not (np.isfinite(w).all() and (w >= 0.0).all()):
        raise ValueError("omega must be finite and not negative")
    if not (ray_m >= 0.0 and ray_k >= 0.0 and np.isfinite(ray_m) and np.isfinite(ray_k)):
        raise ValueError("the Rayleigh coefficients must be finite and not negative")
    return w, 1.0 + 1j * w * ray_k, 1j * w * ray_m - w * w


def jacobi_cocg(rtol, max_iter=100000, counts=None):
    """A ``solver`` for ``harmonic``: the device's algorithm, the conjugate orthogonal CG (CG with the unconjugated form
    x^T y) on the complex symmetric A, preconditioned with its diagonal, from a zero start to ||r|| <= rtol ||b||.
    counts: a list that receives (iterations, status) of every solve; status 0 converged, 1 max_iter, 2 breakdown (a zero or
    non-finite p^T A p or r^T z)."""
    counts = [] if counts is None else counts

    def bad(v):
        return not np.isfinite(v) or v == 0.0

    def solve(A, b):
        d = A.diagonal()
        dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
        b = np.asarray(b, complex)
        x = np.zeros_like(b)
        r = b.copy()
        bb = float(np.vdot(r, r).real)
        it, status = 0, 0
        if bb > 0.0:
            z = dinv * r
            p = z.copy()
            rho = r @ z
            status = 1
            while it < max_iter:
                Ap = A @ p
                sigma = p @ Ap
                if bad(rho) or bad(sigma):
                    it += 1
                    status = 2
                    break
                alpha = rho / sigma
                x += alpha * p
                r -= alpha * Ap
                it += 1
                if float(np.vdot(r, r).real) <= rtol * rtol * bb:
                    status = 0
                    break
                z = dinv * r
                rho_new = r @ z
                if bad(rho_new):
                    status = 2
                    break
                p = z + (rho_new / rho) * p
                rho = rho_new
        counts.append((it, status))
        return x
    solve.counts = counts
    return solve


def harmonic(K, M, fixed, omegas, f, ray_m=0.0, ray_k=0.0, solver=None):
    """The arrays of pl_harmonic from the matrices K, M (6N x 6N, dense or sparse) and the mask fixed (N, 6) / (6N,):
    ((1 + i w ray_k) K + (i w ray_m - w^2) M) u = f on the free dofs for every w of ``omegas``, the fixed dofs at zero.

    f (6N,) or (N, 6), real or complex, is read with the fixed dofs zeroed.  solver(A, b): the solver of the reduced complex
    system (A sparse); None = a dense solve.  Returns a dict: omega (n_freq,), u (n_freq, N, 6) complex and power (n_freq, 4)
    = Re f^T u, Im f^T u (unconjugated), u^H K u, u^H M u; with a ``jacobi_cocg`` solver also iterations and status (n_freq,)."""
    w, cK, cM = harmonic_coefficients(omegas, ray_m, ray_k)
    fx = np.asarray(fixed).reshape(-1) != 0
    n6 = fx.size
    free = np.flatnonzero(~fx)
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    Kf, Mf = K[free][:, free].tocsr(), M[free][:, free].tocsr()
    ff = np.asarray(f, complex).reshape(-1)[free]
    U = np.zeros((w.size, n6), complex)
    power = np.zeros((w.size, 4))
    counts = getattr(solver, "counts", None)
    n0 = 0 if counts is None else len(counts)
    for k in range(w.size):
        A = (cK[k] * Kf + cM[k] * Mf).tocsr()
        u = np.linalg.solve(A.toarray(), ff) if solver is None else solver(A, ff)
        U[k, free] = u
        fu = ff @ u
        power[k] = fu.real, fu.imag, np.vdot(u, Kf @ u).real, np.vdot(u, Mf @ u).real
    out = {"omega": w, "u": U.reshape(w.size, n6 // 6, 6), "power": power}
    if counts is not None:
        out["iterations"] = np.array([c[0] for c in counts[n0:]], int)
        out["status"] = np.array([c[1] for c in counts[n0:]], int)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Radius sensitivities of the frequency response (csrc/pl_harm_sens.h, pl_harmonic_sens)
# ---------------------------------------------------------------------------------------------------------------------
def harmonic_objective(y, kind, p=8.0, weight=None):
    """(J, g) with g_k = dJ/dy_k in the sense dJ = sum_k Re(g_k dy_k), for the complex outputs y (n_freq,) and weights w >= 0
    (None = 1): kind 0: J = -sum w Im y (g = i w), 1: J = 1/2 sum w |y|^2 (g = w conj(y)), 2: J = (sum w |y|^p)^(1/p), p >= 2
    (g = J^(1-p) w |y|^(p-2) conj(y), 0 where J = 0)."""
    y = np.asarray(y, complex).reshape(-1)
    w = np.ones(y.size) if weight is None else np.asarray(weight, float).reshape(-1)
    if w.shape != y.shape or not np.isfinite(w).all() or (w < 0.0).any():
        raise ValueError("weight must have one finite entry per frequency and must not be negative")
    if kind == 0:
        return -float(w @ y.imag), 1j * w
    if kind == 1:
        return 0.5 * float(w @ (np.abs(y) ** 2)), w * np.conj(y)
    if kind == 2:
        if not (p >= 2.0 and np.isfinite(p)):
            raise ValueError("p must be at least 2")
        # scaled by the largest |y|: no overflow of |y|^p
        top = float(np.abs(y).max())
        if top == 0.0:
            return 0.0, np.zeros_like(y)
        s = np.abs(y) / top
        Js = float(w @ s ** p) ** (1.0 / p)
        if Js == 0.0:
            return 0.0, np.zeros_like(y)
        c = np.where(s > 0.0, Js ** (1.0 - p) * w * np.where(s > 0.0, s, 1.0) ** (p - 2.0) / top, 0.0)
        return top * Js, c * np.conj(y)
    raise ValueError("kind must be 0, 1 or 2")


def harmonic_sensitivity(K, M, fixed, conn, drec_dr, dM_dr, omegas, f=None, out_vec=None, kind=2, p=8.0, weight=None,
                         base_dir=None, ray_m=0.0, ray_k=0.0, solver=None):
    """What pl_harmonic_sens computes: J of the outputs y_k = l^T u_k (unconjugated) of ``harmonic`` and dJ/dr_b at fixed
    segment geometry (discretise, then differentiate).

    conn (B, 2), drec_dr (B, 8) the radius derivative of the condensed records (stress_host.drecords_dr) and dM_dr
    (B, 12, 12) that of the mass elements (mass_host.delement_matrix_dr) give dK_e/dr_b and dM_e/dr_b.  f (6N,) or (N, 6),
    real or complex, is a dead load (None = 0); base_dir (3,) adds the load -M e_dir of a base shaken with unit acceleration,
    e_dir the rigid translation of ALL nodes: the only load that follows the design.  out_vec = l (6N,) or (N, 6) real, read
    with the fixed dofs zeroed; None: l is the whole load.  Point masses have no derivative.

    A_k = c_K K + c_M M is complex symmetric, so A_k lam_k = l has the matrix of the forward solve and
        dy_k/dr_b = -[c_K lam_e^T dK_e u_e + c_M lam_e^T dM_e u_e + s lam_e^T dM_e e_dir,e]        s = 1 with base_dir, else 0
    (out_vec = None: lam_k = u_k, no second solve, and s = 2: l follows the design too);  dJ/dr_b = sum_k Re(g_k dy_k/dr_b)
    with (J, g) = ``harmonic_objective``.  Returns a dict: J, y (n_freq,) complex, dJ_dr (B,), dy_dr (n_freq, B) complex,
    lam (n_freq, N, 6) complex, u (n_freq, N, 6) complex; with a ``jacobi_cocg`` solver also iterations and status
    (2, n_freq) = forward, adjoint (zeros with out_vec = None)."""
    from . import geometric_host as GH
    w, cK, cM = harmonic_coefficients(omegas, ray_m, ray_k)
    fx = np.asarray(fixed).reshape(-1) != 0
    n6 = fx.size
    N = n6 // 6
    M = sp.csr_matrix(M)
    if f is None and base_dir is None:
        raise ValueError("neither a load nor base_dir")
    load = np.zeros(n6, complex) if f is None else np.asarray(f, complex).reshape(-1).copy()
    if load.size != n6:
        raise ValueError(f"f must have {n6} entries")
    e_dir = np.zeros((N, 6))
    s = 0.0
    if base_dir is not None:
        e_dir[:, :3] = np.asarray(base_dir, float).reshape(3)
        load = load - M @ e_dir.reshape(-1)
        s = 1.0
    load[fx] = 0.0
    fwd = harmonic(K, M, fixed, w, load, ray_m, ray_k, solver)
    U = fwd["u"]
    its = np.zeros((2, w.size), int)
    sts = np.zeros((2, w.size), int)
    if "iterations" in fwd:
        its[0], sts[0] = fwd["iterations"], fwd["status"]
    if out_vec is None:
        l = load
        lam = U
        s *= 2.0
    else:
        l = np.asarray(out_vec, float).reshape(-1)
        if l.size != n6:
            raise ValueError(f"out_vec must have {n6} entries")
        l = np.where(fx, 0.0, l)
        adj = harmonic(K, M, fixed, w, l, ray_m, ray_k, solver)
        lam = adj["u"]
        if "iterations" in adj:
            its[1], sts[1] = adj["iterations"], adj["status"]
    y = U.reshape(w.size, n6) @ l
    J, g = harmonic_objective(y, kind, p, weight)

    conn = np.asarray(conn).reshape(-1, 2)
    drec = np.asarray(drec_dr, float).reshape(-1, 8)
    dM = np.asarray(dM_dr, float).reshape(-1, 12, 12)
    ia, ib = conn[:, 0], conn[:, 1]
    ee = np.concatenate([e_dir[ia], e_dir[ib]], axis=1)
    dy = np.zeros((w.size, len(conn)), complex)
    for k in range(w.size):
        u, la = U[k], lam[k]
        qK = (GH._pairing(drec, conn, u.real, la.real) - GH._pairing(drec, conn, u.imag, la.imag)
              + 1j * (GH._pairing(drec, conn, u.imag, la.real) + GH._pairing(drec, conn, u.real, la.imag)))
        ue = np.concatenate([u[ia], u[ib]], axis=1)
        le = np.concatenate([la[ia], la[ib]], axis=1)
        qM = np.einsum("bi,bij,bj->b", le, dM, ue)
        qE = np.einsum("bi,bij,bj->b", le, dM, ee)
        dy[k] = -(cK[k] * qK + cM[k] * qM + s * qE)
    grad = (g[:, None] * dy).real.sum(axis=0)
    out = {"J": J, "y": y, "dJ_dr": grad, "dy_dr": dy, "lam": lam, "u": U, "g": g}
    if "iterations" in fwd:
        out["iterations"], out["status"] = its, sts
    return out
