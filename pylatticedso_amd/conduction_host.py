"""Numpy restatement of steady heat conduction on the strut graph (include/pylattice_hip.h: pl_set_conduction / pl_cond_spmv /
pl_cond_solve / pl_cond_flux / pl_cond_sens / pl_thermal_load_adjoint; csrc/pl_conduction.h), the
counterpart of thermal_host.py.

Dense and vectorised over the struts, no device call.  Strut b joins A = beam_conn[b, 0] and B = beam_conn[b, 1], d = x_B - x_A,
L = |d|.  Each strut is one two-node conductor of uniform circular section of the plain radius r over the node-to-node length;
penalised end zones and the overlap at the joints are ignored, a multiplicity k counts k times:

    g_b = k_b kappa_b pi r_b^2 / L_b,   d g_b / d r_b = 2 g_b / r_b
    (K_T T)_i = sum over struts b at i of g_b (T_i - T_other)
    K_T T = q on the free nodes, T = T_bar on the nodes of a Dirichlet mask (one flag per node)
    Q_b = g_b (T_A - T_B) / k_b                                heat flow of one copy from A to B

With dT = T - T_ref as the node_dT of the thermal loads, the transpose of d f_th / d dT applied to a mechanical field lam is
c_i = sum over struts b at i of (1/2) alpha_b L_b ka_b t_b . (lam_u,B - lam_u,A); with K_T mu = c on the free thermal nodes
(mu = 0 on the others) every q(u(T(r), r), r) with K lam = dq/du gains dq/dr_b += -(2 g_b / r_b) (mu_A - mu_B) (T_A - T_B).

Lumped strut-surface convection (pl_set_convection / pl_cond_film / pl_temp_pnorm): every strut end
exchanges with an ambient at T_inf through the film conductance

    c_b = k_b h_b pi r_b L_b,   d c_b / d r_b = c_b / r_b,   H_i = sum over struts b at i of c_b
    (K_T + diag H) T = q + H T_inf on the free nodes, T = T_bar on the fixed ones
    Qc_b = c_b [(T_A - T_inf) + (T_B - T_inf)] / k_b,   P = sum_b k_b Qc_b = sum_i H_i (T_i - T_inf)

and for J(T(r), r) with (K_T + H) mu = dJ/dT on the free nodes, mu = 0 on the fixed ones,

    dJ/dr_b = dJ/dr_b at fixed T - (2 g_b / r_b)(mu_A - mu_B)(T_A - T_B) - (c_b / r_b)[mu_A (T_A - T_inf) + mu_B (T_B - T_inf)].

Every function takes the convection through optional arguments (H, c, t_inf) that default to none.

Transient conduction (pl_set_heat_capacity / pl_cond_transient; csrc/pl_heat.h): the lumped capacity

    C_i = sum over struts b at i of (1/2) k_b (rho c)_b pi r_b^2 L_b + node_capacity_i,
    C dT/dt + (K_T + H) T = q(t) + H T_inf on the free nodes, T = T_bar(t) on the fixed ones,

stepped by the one-step theta scheme in increment form (``transient``), and solved exactly for data constant in time by the
generalised eigen-decomposition of (K_T + H, C) on the free nodes (``transient_exact``).
"""
from __future__ import annotations

import numpy as np

from . import stress_host as SH
from . import thermal_host as TH


def _length(node_xyz, conn):
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    d = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    return np.sqrt(SH._dot(d, d))


def conductance(node_xyz, beam_conn, radius, kappa, mult=None):
    """(B,) g_b = k kappa pi r^2 / L; kappa a scalar or (B,)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    r = np.asarray(radius, dtype=float).reshape(-1)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    return k * np.asarray(kappa, dtype=float) * (np.pi * r * r) / _length(node_xyz, conn)


def laplacian(beam_conn, node_count, g):
    """Dense (N, N) K_T of the conductances g."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    g = np.asarray(g, dtype=float)
    K = np.zeros((node_count, node_count))
    a, b = conn[:, 0], conn[:, 1]
    np.add.at(K, (a, a), g)
    np.add.at(K, (b, b), g)
    np.add.at(K, (a, b), -g)
    np.add.at(K, (b, a), -g)
    return K


def film_conductance(node_xyz, beam_conn, radius, film, mult=None):
    """(B,) c_b = k h pi r L, the film conductance of one strut end; film a scalar or (B,)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    r = np.asarray(radius, dtype=float).reshape(-1)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    return k * np.asarray(film, dtype=float) * (np.pi * r) * _length(node_xyz, conn)


def convection_diag(beam_conn, node_count, c):
    """(N,) H_i = sum over the struts at node i of c_b."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    c = np.broadcast_to(np.asarray(c, dtype=float), (len(conn),))
    H = np.zeros(node_count)
    np.add.at(H, conn[:, 0], c)
    np.add.at(H, conn[:, 1], c)
    return H


def spmv(beam_conn, node_count, g, x, fixed=None, H=None):
    """K_T x per strut, fixed not None: P K_T P x (what pl_cond_spmv returns).  H (N,) given: K_T + diag(H)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    x = np.asarray(x, dtype=float).reshape(-1)
    if fixed is not None:
        x = np.where(np.asarray(fixed).astype(bool), 0.0, x)
    flow = np.asarray(g, dtype=float) * (x[conn[:, 0]] - x[conn[:, 1]])
    y = np.zeros(node_count)
    np.add.at(y, conn[:, 0], flow)
    np.add.at(y, conn[:, 1], -flow)
    if H is not None:
        y = y + np.asarray(H, dtype=float) * x
    return y if fixed is None else np.where(np.asarray(fixed).astype(bool), 0.0, y)


def solve(beam_conn, node_count, g, fixed, t_bar=None, q=None, H=None, t_inf=0.0):
    """(N,) T of K_T T = q on the free nodes, T = t_bar on the fixed ones: a dense solve.  H (N,) given: the convective
    problem (K_T + diag H) T = q + H t_inf, for which a mask that fixes no node is valid."""
    import scipy.linalg
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    if not fixed.any() and H is None:
        raise ValueError("conduction_host.solve: the mask fixes no node")
    K = laplacian(beam_conn, node_count, g)
    if H is not None:
        K = K + np.diag(np.asarray(H, dtype=float))
    T = np.zeros(node_count)
    if t_bar is not None:
        T[fixed] = np.broadcast_to(np.asarray(t_bar, dtype=float), (node_count,))[fixed]
    rhs = -K @ T
    if q is not None:
        rhs = rhs + np.asarray(q, dtype=float).reshape(-1)
    if H is not None:
        rhs = rhs + np.asarray(H, dtype=float) * t_inf
    free = np.flatnonzero(~fixed)
    if len(free):
        T[free] = scipy.linalg.solve(K[np.ix_(free, free)], rhs[free], assume_a="pos")
    return T


def flux(beam_conn, g, T, mult=None):
    """(B,) Q_b = g (T_A - T_B) / k of one copy of every strut, from A to B."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    T = np.asarray(T, dtype=float).reshape(-1)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    return np.asarray(g, dtype=float) * (T[conn[:, 0]] - T[conn[:, 1]]) / k


def cond_sens(beam_conn, radius, g, T, mu, c=None, t_inf=0.0):
    """(B,) mu^T (dK_T / dr_b) T = (2 g / r) (mu_A - mu_B) (T_A - T_B) - the output of pl_cond_sens.  c (B,) given: plus the
    convective bracket (c / r) [mu_A (T_A - t_inf) + mu_B (T_B - t_inf)]."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    T = np.asarray(T, dtype=float).reshape(-1)
    mu = np.asarray(mu, dtype=float).reshape(-1)
    r = np.asarray(radius, dtype=float)
    a, b = conn[:, 0], conn[:, 1]
    out = 2.0 * np.asarray(g, dtype=float) / r * (mu[a] - mu[b]) * (T[a] - T[b])
    if c is not None:
        out = out + np.asarray(c, dtype=float) / r * (mu[a] * (T[a] - t_inf) + mu[b] * (T[b] - t_inf))
    return out


def film_loss(beam_conn, c, T, t_inf, mult=None):
    """(B,) Qc_b = c [(T_A - t_inf) + (T_B - t_inf)] / k, the convective loss of one copy of every strut - the output of
    pl_cond_film; the dissipated power is P = sum k Qc."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    T = np.asarray(T, dtype=float).reshape(-1)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    return np.asarray(c, dtype=float) * ((T[conn[:, 0]] - t_inf) + (T[conn[:, 1]] - t_inf)) / k


def temp_pnorm(T, p, reference=0.0, nodes=None):
    """(Phi_p, v_max, sum (v / v_max)^p, dPhi/dT (N,)) of v = max(T - reference, 0) over the nodes of ``nodes`` (flags, None =
    all), evaluated as v_max (sum (v / v_max)^p)^(1/p) - the outputs of pl_temp_pnorm.  A NaN adds nothing."""
    T = np.asarray(T, dtype=float).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = np.where(T - reference > 0.0, T - reference, 0.0)
    if nodes is not None:
        v = np.where(np.asarray(nodes).reshape(-1) != 0, v, 0.0)
    vmax = float(v.max()) if v.size else 0.0
    if not vmax > 0.0:
        return 0.0, 0.0, 0.0, np.zeros_like(v)
    ratio = v / vmax
    ssum = float((ratio[v > 0.0] ** p).sum())
    grad = np.where(v > 0.0, ratio ** (p - 1.0), 0.0) * ssum ** (1.0 / p - 1.0)
    return vmax * ssum ** (1.0 / p), vmax, ssum, grad


def thermal_gradient(functional, node_xyz, beam_conn, radius, kappa, fixed, t_bar=None, q=None, film=None, t_inf=0.0,
                     mult=None, p=8.0, reference=None, nodes=None, convective_bracket=True):
    """(J, dJ/dr (B,)) of a thermal functional of the conduction problem with lumped convection, the adjoint chain on dense
    matrices.  functional: "thermal_compliance" J = q . (T - t_inf) over the free nodes; "heat_dissipation" J = P;
    "temp_pnorm" J = Phi_p of T - reference (default t_inf) over ``nodes`` (default the free nodes).  film None: no convection
    (heat_dissipation is then undefined).  convective_bracket = False leaves the (c / r) [...] term of the chain out - the
    gradient that is wrong."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    r = np.asarray(radius, dtype=float).reshape(-1)
    N = len(np.asarray(node_xyz).reshape(-1, 3))
    fx = np.asarray(fixed).astype(bool).reshape(-1)
    g = conductance(node_xyz, conn, r, kappa, mult)
    c = None if film is None else film_conductance(node_xyz, conn, r, film, mult)
    H = None if c is None else convection_diag(conn, N, c)
    qq = np.zeros(N) if q is None else np.where(fx, 0.0, np.asarray(q, dtype=float).reshape(-1))
    T = solve(conn, N, g, fx, t_bar, qq, H, t_inf)
    partial = np.zeros(len(conn))
    if functional == "thermal_compliance":
        J, dJdT = float(qq @ (T - t_inf)), qq
    elif functional == "heat_dissipation":
        if c is None:
            raise ValueError("heat_dissipation needs convection")
        k = 1.0 if mult is None else np.asarray(mult, dtype=float)
        kQc = k * film_loss(conn, c, T, t_inf, mult)
        J, dJdT, partial = float(kQc.sum()), H, kQc / r
    elif functional == "temp_pnorm":
        J, _, _, dJdT = temp_pnorm(T, p, t_inf if reference is None else reference, ~fx if nodes is None else nodes)
    else:
        raise ValueError(f"unknown functional {functional!r}")
    mu = solve(conn, N, g, fx, None, np.where(fx, 0.0, dJdT), H, 0.0)
    grad = partial - cond_sens(conn, r, g, T, mu, c if convective_bracket else None, t_inf)
    return J, grad


def heat_capacity(node_xyz, beam_conn, radius, rho_c, mult=None, node_capacity=None):
    """(N,) lumped heat capacity C_i = sum over the struts at node i of (1/2) k rho_c pi r^2 L + node_capacity_i: half of every
    copy's volume to each end times the volumetric heat capacity; rho_c a scalar or (B,)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    r = np.asarray(radius, dtype=float).reshape(-1)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    cap = np.broadcast_to(0.5 * k * np.asarray(rho_c, dtype=float) * (np.pi * r * r) * _length(node_xyz, conn), (len(conn),))
    N = len(np.asarray(node_xyz).reshape(-1, 3))
    C = np.zeros(N)
    np.add.at(C, conn[:, 0], cap)
    np.add.at(C, conn[:, 1], cap)
    return C if node_capacity is None else C + np.asarray(node_capacity, dtype=float).reshape(-1)


def row_value(t0, t_bar, s):
    """The prescribed temperature of a fixed node in a row of ramp value s: t0 + s (t_bar - t0), in this order (the device
    evaluates the same three roundings, so fixed nodes compare bit for bit)."""
    t0 = np.asarray(t0, dtype=float)
    d = np.asarray(t_bar, dtype=float) - t0
    return t0 + s * d


def transient(beam_conn, node_count, g, C, dt, n_steps, theta=1.0, fixed=None, t_bar=None, bar_amp=None, patterns=None,
              amp=None, t0=None, H=None, t_inf=0.0):
    """The one-step theta scheme of pl_cond_transient on dense matrices (numpy.linalg.solve): C dT/dt + (K_T + H) T = q(t) + H t_inf
    on the free nodes, T = t0 + s_n (t_bar - t0) on the fixed ones (s = bar_amp (n_steps + 1,), None = 1), in increment form

        (C/dt + theta (K_T + H)) dT = q_theta + H t_inf - (K_T + H) W on the free rows,
        W = T_n on free nodes, (1 - theta) T_n + theta T_bar,n+1 on fixed ones, q_theta = theta q_{n+1} + (1 - theta) q_n,

    q_n = amp[n] @ patterns (values on fixed nodes ignored).  t0 None = t_inf everywhere, t_bar None = 0, fixed None = no fixed
    node.  Returns a dict: T (n_steps + 1, N); heat (n_steps + 1, 4) = U, Q_in, Q_c, Q_R (the stored heat sum C (T - t_inf) and
    the cumulative inflow, convective loss and heat supplied by the fixed nodes: U_n - U_0 = Q_in + Q_R - Q_c); bar
    (n_steps + 1, N) the prescribed row values (read on the fixed nodes only)."""
    N, n_steps = int(node_count), int(n_steps)
    rows = n_steps + 1
    fx = np.zeros(N, bool) if fixed is None else (np.asarray(fixed).reshape(-1) != 0)
    free = np.flatnonzero(~fx)
    C = np.asarray(C, dtype=float).reshape(-1)
    Hd = np.zeros(N) if H is None else np.asarray(H, dtype=float).reshape(-1)
    A = laplacian(beam_conn, N, g) + np.diag(Hd)
    start = np.full(N, float(t_inf)) if t0 is None else np.array(t0, dtype=float).reshape(-1)
    tb = np.zeros(N) if t_bar is None else np.broadcast_to(np.asarray(t_bar, dtype=float).reshape(-1), (N,))
    s = np.ones(rows) if bar_amp is None else np.asarray(bar_amp, dtype=float).reshape(-1)
    bar = np.stack([row_value(start, tb, s[n]) for n in range(rows)])
    if patterns is None:
        q = np.zeros((rows, N))
    else:
        pat = np.asarray(patterns, dtype=float).reshape(-1, N)
        q = np.asarray(amp, dtype=float).reshape(rows, pat.shape[0]) @ pat
    q = np.where(fx[None, :], 0.0, q)
    T = np.zeros((rows, N))
    T[0] = np.where(fx, bar[0], start)
    heat = np.zeros((rows, 4))
    heat[0, 0] = C @ (T[0] - t_inf)
    S = np.diag(C / dt) + theta * A
    Sff = S[np.ix_(free, free)]
    for n in range(n_steps):
        W = np.where(fx, (1.0 - theta) * T[n] + theta * bar[n + 1], T[n])
        qt = theta * q[n + 1] + (1.0 - theta) * q[n]
        rhs = qt + Hd * t_inf - A @ W
        d = np.where(fx, bar[n + 1] - T[n], 0.0)
        if len(free):
            d[free] = np.linalg.solve(Sff, rhs[free])
        T[n + 1] = np.where(fx, bar[n + 1], T[n] + d)
        Tt = T[n] + theta * d
        heat[n + 1, 0] = C @ (T[n + 1] - t_inf)
        heat[n + 1, 1] = heat[n, 1] + dt * qt[free].sum()
        heat[n + 1, 2] = heat[n, 2] + dt * (Hd @ (Tt - t_inf))
        heat[n + 1, 3] = heat[n, 3] + (C * d + dt * (A @ Tt - Hd * t_inf))[fx].sum()
    return {"T": T, "heat": heat, "bar": bar}


def transient_exact(beam_conn, node_count, g, C, t, fixed=None, t_bar=None, q=None, t0=None, H=None, t_inf=0.0):
    """(N,) the solution at time t of C dT/dt + (K_T + H) T = q + H t_inf on the free nodes with loads and boundary data constant
    in time (T = t_bar on the fixed nodes from t = 0 on, start field t0, None = t_inf), from the generalised eigen-decomposition
    (K_T + H) v = lam C v on the free nodes: each mode relaxes as exp(-lam t); a mode with lam = 0 (an insulated lattice) grows
    linearly with its load."""
    import scipy.linalg
    N = int(node_count)
    fx = np.zeros(N, bool) if fixed is None else (np.asarray(fixed).reshape(-1) != 0)
    free = np.flatnonzero(~fx)
    C = np.asarray(C, dtype=float).reshape(-1)
    Hd = np.zeros(N) if H is None else np.asarray(H, dtype=float).reshape(-1)
    A = laplacian(beam_conn, N, g) + np.diag(Hd)
    start = np.full(N, float(t_inf)) if t0 is None else np.asarray(t0, dtype=float).reshape(-1)
    T = np.zeros(N)
    if t_bar is not None:
        T[fx] = np.broadcast_to(np.asarray(t_bar, dtype=float).reshape(-1), (N,))[fx]
    b = Hd * t_inf - A @ T
    if q is not None:
        b = b + np.asarray(q, dtype=float).reshape(-1)
    if len(free):
        lam, V = scipy.linalg.eigh(A[np.ix_(free, free)], np.diag(C[free]))
        a0 = V.T @ (C[free] * start[free])
        beta = V.T @ b[free]
        lt = lam * t
        small = np.abs(lt) < 1e-12
        growth = np.where(small, t, -np.expm1(-lt) / np.where(small, 1.0, lam))
        T[free] = V @ (a0 * np.exp(-lt) + beta * growth)
    return T


def thermal_load_adjoint(rec, beam_conn, node_count, alpha, lam):
    """(N,) c = (d f_th / d dT)^T lam: every strut adds (1/2) alpha L ka t . (lam_u,B - lam_u,A) to both of its ends - the
    output of pl_thermal_load_adjoint.  alpha a scalar or (B,)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    lam = np.asarray(lam, dtype=float).reshape(-1, 6)
    d = rec[:, 5:8]
    term = 0.5 * np.asarray(alpha, dtype=float) * TH.axial_stiffness(rec) * SH._dot(d, lam[conn[:, 1], :3] - lam[conn[:, 0], :3])
    c = np.zeros(node_count)
    np.add.at(c, conn[:, 0], term)
    np.add.at(c, conn[:, 1], term)
    return c


def coupled_state(node_xyz, beam_conn, radius, seg_len, seg_nsub, material, mult, fixed_dof, f_ext, alpha, kappa, t_fixed,
                  t_bar, heat_in, reference=0.0, film=None, t_inf=0.0):
    """The thermo-elastic equilibrium on dense matrices: T of the conduction problem, f_th of T - reference, and u (N, 6) of
    K u = f_ext + f_th on the free dofs (zero on the fixed ones).  material = (E, nu, kappa_shear, pen).  Returns a dict."""
    import scipy.linalg
    from . import geometric_host as GH
    conn = np.asarray(beam_conn).reshape(-1, 2)
    N = len(np.asarray(node_xyz).reshape(-1, 3))
    rec = SH.records(node_xyz, conn, radius, seg_len, seg_nsub, *material, mult)
    g = conductance(node_xyz, conn, radius, kappa, mult)
    c = None if film is None else film_conductance(node_xyz, conn, radius, film, mult)
    H = None if c is None else convection_diag(conn, N, c)
    T = solve(conn, N, g, t_fixed, t_bar, heat_in, H, t_inf)
    delta = TH.elongation(node_xyz, conn, alpha, T - reference)
    f_th = TH.thermal_load(rec, conn, N, delta, mult)[0]
    K = GH.elastic_matrix(rec, conn, N)
    K = K.toarray() if hasattr(K, "toarray") else np.asarray(K)
    free = np.flatnonzero(~np.asarray(fixed_dof).astype(bool).ravel())
    Kff = K[np.ix_(free, free)]
    u = np.zeros(6 * N)
    u[free] = scipy.linalg.solve(Kff, (np.asarray(f_ext, dtype=float) + f_th).ravel()[free], assume_a="pos")
    return {"rec": rec, "g": g, "c": c, "H": H, "T": T, "delta": delta, "f_th": f_th, "u": u.reshape(N, 6), "K": K, "free": free}


def coupled_gradient(node_xyz, beam_conn, radius, seg_len, seg_nsub, material, mult, fixed_dof, f_ext, q, alpha, kappa,
                     t_fixed, t_bar, heat_in, reference=0.0, chain=True, film=None, t_inf=0.0):
    """(B,) d(q . u)/dr_b of the thermo-elastic equilibrium of coupled_state at fixed segment geometry - the whole chain on
    dense matrices: -lam^T (dK/dr) u + lam^T d f_th/dr at fixed T, and (chain) -(2 g / r)(mu_A - mu_B)(T_A - T_B) with
    K lam = q on the free dofs, c = thermal_load_adjoint(lam), K_T mu = c on the free thermal nodes.  t_bar and heat_in do not
    depend on r.  chain = False leaves the temperature's dependence on the radii out (the gradient that is silently wrong)."""
    import scipy.linalg
    from . import geometric_host as GH
    conn = np.asarray(beam_conn).reshape(-1, 2)
    st = coupled_state(node_xyz, conn, radius, seg_len, seg_nsub, material, mult, fixed_dof, f_ext, alpha, kappa, t_fixed,
                       t_bar, heat_in, reference, film, t_inf)
    N = len(st["T"])
    free = st["free"]
    lam = np.zeros(6 * N)
    lam[free] = scipy.linalg.solve(st["K"][np.ix_(free, free)], np.asarray(q, dtype=float).ravel()[free], assume_a="pos")
    lam = lam.reshape(N, 6)
    drec = SH.drecords_dr(node_xyz, conn, radius, seg_len, seg_nsub, *material, mult)
    grad = -GH._pairing(drec, conn, st["u"], lam) + TH.thermal_sens(st["rec"], conn, radius, st["delta"], lam)
    if chain:
        c = thermal_load_adjoint(st["rec"], conn, N, alpha, lam)
        tf = np.asarray(t_fixed).astype(bool).reshape(-1)
        mu = solve(conn, N, st["g"], tf, None, np.where(tf, 0.0, c), st["H"], 0.0)
        grad = grad - cond_sens(conn, radius, st["g"], st["T"], mu, st["c"], t_inf)
    return grad
