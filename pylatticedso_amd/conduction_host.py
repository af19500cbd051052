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


def spmv(beam_conn, node_count, g, x, fixed=None):
    """K_T x per strut, fixed not None: P K_T P x (what pl_cond_spmv returns)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    x = np.asarray(x, dtype=float).reshape(-1)
    if fixed is not None:
        x = np.where(np.asarray(fixed).astype(bool), 0.0, x)
    flow = np.asarray(g, dtype=float) * (x[conn[:, 0]] - x[conn[:, 1]])
    y = np.zeros(node_count)
    np.add.at(y, conn[:, 0], flow)
    np.add.at(y, conn[:, 1], -flow)
    return y if fixed is None else np.where(np.asarray(fixed).astype(bool), 0.0, y)


def solve(beam_conn, node_count, g, fixed, t_bar=None, q=None):
    """(N,) T of K_T T = q on the free nodes, T = t_bar on the fixed ones: a dense solve."""
    import scipy.linalg
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    if not fixed.any():
        raise ValueError("conduction_host.solve: the mask fixes no node")
    K = laplacian(beam_conn, node_count, g)
    T = np.zeros(node_count)
    if t_bar is not None:
        T[fixed] = np.broadcast_to(np.asarray(t_bar, dtype=float), (node_count,))[fixed]
    rhs = -K @ T
    if q is not None:
        rhs = rhs + np.asarray(q, dtype=float).reshape(-1)
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


def cond_sens(beam_conn, radius, g, T, mu):
    """(B,) mu^T (dK_T / dr_b) T = (2 g / r) (mu_A - mu_B) (T_A - T_B) - the output of pl_cond_sens."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    T = np.asarray(T, dtype=float).reshape(-1)
    mu = np.asarray(mu, dtype=float).reshape(-1)
    return (2.0 * np.asarray(g, dtype=float) / np.asarray(radius, dtype=float) *
            (mu[conn[:, 0]] - mu[conn[:, 1]]) * (T[conn[:, 0]] - T[conn[:, 1]]))


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
                  t_bar, heat_in, reference=0.0):
    """The thermo-elastic equilibrium on dense matrices: T of the conduction problem, f_th of T - reference, and u (N, 6) of
    K u = f_ext + f_th on the free dofs (zero on the fixed ones).  material = (E, nu, kappa_shear, pen).  Returns a dict."""
    import scipy.linalg
    from . import geometric_host as GH
    conn = np.asarray(beam_conn).reshape(-1, 2)
    N = len(np.asarray(node_xyz).reshape(-1, 3))
    rec = SH.records(node_xyz, conn, radius, seg_len, seg_nsub, *material, mult)
    g = conductance(node_xyz, conn, radius, kappa, mult)
    T = solve(conn, N, g, t_fixed, t_bar, heat_in)
    delta = TH.elongation(node_xyz, conn, alpha, T - reference)
    f_th = TH.thermal_load(rec, conn, N, delta, mult)[0]
    K = GH.elastic_matrix(rec, conn, N)
    K = K.toarray() if hasattr(K, "toarray") else np.asarray(K)
    free = np.flatnonzero(~np.asarray(fixed_dof).astype(bool).ravel())
    Kff = K[np.ix_(free, free)]
    u = np.zeros(6 * N)
    u[free] = scipy.linalg.solve(Kff, (np.asarray(f_ext, dtype=float) + f_th).ravel()[free], assume_a="pos")
    return {"rec": rec, "g": g, "T": T, "delta": delta, "f_th": f_th, "u": u.reshape(N, 6), "K": K, "free": free}


def coupled_gradient(node_xyz, beam_conn, radius, seg_len, seg_nsub, material, mult, fixed_dof, f_ext, q, alpha, kappa,
                     t_fixed, t_bar, heat_in, reference=0.0, chain=True):
    """(B,) d(q . u)/dr_b of the thermo-elastic equilibrium of coupled_state at fixed segment geometry - the whole chain on
    dense matrices: -lam^T (dK/dr) u + lam^T d f_th/dr at fixed T, and (chain) -(2 g / r)(mu_A - mu_B)(T_A - T_B) with
    K lam = q on the free dofs, c = thermal_load_adjoint(lam), K_T mu = c on the free thermal nodes.  t_bar and heat_in do not
    depend on r.  chain = False leaves the temperature's dependence on the radii out (the gradient that is silently wrong)."""
    import scipy.linalg
    from . import geometric_host as GH
    conn = np.asarray(beam_conn).reshape(-1, 2)
    st = coupled_state(node_xyz, conn, radius, seg_len, seg_nsub, material, mult, fixed_dof, f_ext, alpha, kappa, t_fixed,
                       t_bar, heat_in, reference)
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
        mu = solve(conn, N, st["g"], tf, None, np.where(tf, 0.0, c))
        grad = grad - cond_sens(conn, radius, st["g"], st["T"], mu)
    return grad
