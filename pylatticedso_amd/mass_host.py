"""Numpy / scipy restatement of the consistent strut mass and the natural-frequency analysis built on it
(include/pylattice_hip.h: pl_set_mass / pl_mass_spmv_multi / pl_vibration_modes / pl_vibration_modes_sens; csrc/pl_mass.h;
DESIGN.md section 10f), in the manner of geometric_host.py.  No device call.

Free vibration: K phi = omega^2 M phi on the free dofs, solved as the pencil M phi = mu K phi, omega^2 = 1 / mu.  Each strut
is ONE element between its two lattice nodes (the discretisation of K_g), a uniform circular section of the strut's plain
radius r over the node-to-node length L; penalised end zones stiffen K only.  For a strut of multiplicity k and density rho

    m = k rho pi r^2 L,   c = m / 420,   j = m r^2 / 12  (= rho J L / 6),   g = m r^2 / (120 L^2)  (= rho I / (30 L); 0 without
    rotary inertia)

and with t = d / L, P = I - t t^T, u_perp = P u, s = th x t the load on end B is

    f_B = (m / 6) (t.(u_A + 2 u_B)) t + c [54 u_A_perp + 156 u_B_perp + 13 L s_A - 22 L s_B]
          + g [36 (u_B_perp - u_A_perp) - 3 L (s_A + s_B)]
    m_B = j (t.(th_A + 2 th_B)) t + t x { c [-13 L u_A_perp - 22 L u_B_perp - 3 L^2 s_A + 4 L^2 s_B]
                                        + g [-3 L (u_B_perp - u_A_perp) + 4 L^2 s_B - L^2 s_A] }

- the textbook block rho A L / 420 [[156, 22 L, 54, -13 L], ...] in both bending planes, the axial and torsional blocks
[[2, 1], [1, 2]] and the Rayleigh rotary inertia of bending.  End A follows with the roles swapped and d -> -d.  A per-node
point mass adds node_mass_i u_i on the node's three translations.  Radius derivative at fixed segment geometry:
dM_e/dr = (2 / r) M_e[m / 6 and c terms] + (4 / r) M_e[j and g terms].
"""
from __future__ import annotations

import numpy as np
import scipy.linalg
import scipy.sparse as sp

from . import geometric_host as GH
from . import stress_host as SH


def coefficients(d, r, rho, mult=None, rotary=True):
    """(m6, c, j, g) = (m / 6, m / 420, m r^2 / 12, m r^2 / (120 L^2) or 0) of struts with spans d (..., 3), radii r (...,)."""
    d = np.asarray(d, dtype=float)
    r = np.asarray(r, dtype=float)
    k = 1.0 if mult is None else np.asarray(mult, dtype=float)
    L2 = SH._dot(d, d)
    m = k * rho * np.pi * r * r * np.sqrt(L2)
    g = m * r * r / (120.0 * L2) if rotary else np.zeros_like(m)
    return m / 6.0, m / 420.0, m * r * r / 12.0, g


def _blocks(d, m6, c, j, g):
    """(..., 12, 12) element matrix with dofs [u_A, th_A, u_B, th_B] in global axes from the four coefficients."""
    d = np.asarray(d, dtype=float)
    L = np.sqrt(SH._dot(d, d))
    t = d / L[..., None]
    m6, c, j, g = (np.asarray(v, dtype=float)[..., None, None] for v in (m6, c, j, g))
    L = L[..., None, None]
    X = GH._skew(t)                                    # X v = t x v;  th x t = -X th;  X P = X;  X X = -P
    T = t[..., :, None] * t[..., None, :]
    P = np.eye(3) - T
    M = np.zeros(d.shape[:-1] + (12, 12))
    uA, tA, uB, tB = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12)
    M[..., uB, uA] = m6 * T + (54.0 * c - 36.0 * g) * P
    M[..., uB, uB] = 2.0 * m6 * T + (156.0 * c + 36.0 * g) * P
    M[..., uB, tA] = (-13.0 * c + 3.0 * g) * L * X
    M[..., uB, tB] = (22.0 * c + 3.0 * g) * L * X
    M[..., tB, uA] = (-13.0 * c + 3.0 * g) * L * X
    M[..., tB, uB] = (-22.0 * c - 3.0 * g) * L * X
    M[..., tB, tA] = j * T + (-3.0 * c - g) * L * L * P
    M[..., tB, tB] = 2.0 * j * T + (4.0 * c + 4.0 * g) * L * L * P
    # end A: the roles swapped and d -> -d (X -> -X; T and P keep their sign)
    M[..., uA, uB] = M[..., uB, uA]
    M[..., uA, uA] = M[..., uB, uB]
    M[..., uA, tB] = -M[..., uB, tA]
    M[..., uA, tA] = -M[..., uB, tB]
    M[..., tA, uB] = -M[..., tB, uA]
    M[..., tA, uA] = -M[..., tB, uB]
    M[..., tA, tB] = M[..., tB, tA]
    M[..., tA, tA] = M[..., tB, tB]
    return M


def element_matrix(d, r, rho, mult=None, rotary=True):
    """(..., 12, 12) consistent mass of struts with span vectors d (..., 3), radii r (...,), density rho and multiplicities
    mult (None = 1), dofs [u_A, th_A, u_B, th_B] in global axes."""
    return _blocks(d, *coefficients(d, r, rho, mult, rotary))


def delement_matrix_dr(d, r, rho, mult=None, rotary=True):
    """(..., 12, 12) radius derivative of ``element_matrix`` at fixed span: (2 / r) of the m / 6 and c terms, (4 / r) of
    the j and g terms."""
    r = np.asarray(r, dtype=float)
    m6, c, j, g = coefficients(d, r, rho, mult, rotary)
    return _blocks(d, 2.0 / r * m6, 2.0 / r * c, 4.0 / r * j, 4.0 / r * g)


def _spans(node_xyz, beam_conn):
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    return xyz[conn[:, 1]] - xyz[conn[:, 0]], conn


def _point_mass(node_mass, n_nodes):
    nm = np.zeros(n_nodes) if node_mass is None else np.asarray(node_mass, dtype=float).reshape(-1)
    if nm.size != n_nodes:
        raise ValueError(f"node_mass must have {n_nodes} entries")
    if (nm < 0).any():
        raise ValueError("node_mass must not be negative")
    return nm


def mass_matrix(node_xyz, beam_conn, radius, rho, mult=None, rotary=True, node_mass=None):
    """sparse M (6N, 6N) of the lattice: the strut elements, plus node_mass (N,) on the translations."""
    d, conn = _spans(node_xyz, beam_conn)
    n = len(np.asarray(node_xyz).reshape(-1, 3))
    M = GH._scatter(element_matrix(d, radius, rho, mult, rotary), conn, n)
    diag = np.zeros((n, 6))
    diag[:, :3] = _point_mass(node_mass, n)[:, None]
    return (M + sp.diags(diag.ravel())).tocsr()


def mass_apply(node_xyz, beam_conn, radius, rho, X, mult=None, rotary=True, node_mass=None, fixed=None):
    """Y[j] = M X[j] by the force formula, struts vectorised: X (k, N, 6) -> (k, N, 6) (what k_mass_gather_multi computes).
    fixed (N, 6) bool: the masked product P M P (X zeroed on the fixed dofs first, Y zeroed there afterwards)."""
    d, conn = _spans(node_xyz, beam_conn)
    X = np.array(X, dtype=float)
    one = X.ndim == 2
    X = X[None] if one else X.reshape((-1,) + X.shape[-2:])
    if fixed is not None:
        fixed = np.asarray(fixed).reshape(-1, 6) != 0
        X = np.where(fixed[None], 0.0, X)
    nm = _point_mass(node_mass, X.shape[1])
    m6, c, j, g = (v[:, None] for v in coefficients(d, np.asarray(radius, dtype=float).reshape(-1), rho, mult, rotary))
    L = np.sqrt(SH._dot(d, d))[:, None]
    t = d / L
    A, B = conn[:, 0], conn[:, 1]

    def end(t, uo, to, us, ts):
        """load on the strut's end with values (us, ts), the other end's being (uo, to), t pointing to this end"""
        ax = lambda v: SH._dot(v, t)[:, None] * t
        uop, usp = uo - ax(uo), us - ax(us)
        so, ss = np.cross(to, t), np.cross(ts, t)
        f = m6 * ax(uo + 2.0 * us) + c * (54.0 * uop + 156.0 * usp + 13.0 * L * so - 22.0 * L * ss) \
            + g * (36.0 * (usp - uop) - 3.0 * L * (so + ss))
        mo = j * ax(to + 2.0 * ts) + np.cross(t, c * (-13.0 * L * uop - 22.0 * L * usp - 3.0 * L * L * so + 4.0 * L * L * ss)
                                              + g * (-3.0 * L * (usp - uop) + 4.0 * L * L * ss - L * L * so))
        return np.column_stack([f, mo])

    Y = np.zeros_like(X)
    for q in range(len(X)):
        x = X[q]
        np.add.at(Y[q], B, end(t, x[A, :3], x[A, 3:], x[B, :3], x[B, 3:]))
        np.add.at(Y[q], A, end(-t, x[B, :3], x[B, 3:], x[A, :3], x[A, 3:]))
        Y[q, :, :3] += nm[:, None] * x[:, :3]
    if fixed is not None:
        Y = np.where(fixed[None], 0.0, Y)
    return Y[0] if one else Y


def _finish(K, M, free, mu, V, n_modes):
    """dict of the outputs of pl_vibration_modes from Ritz pairs (mu = 1 / omega^2 descending, V K-orthonormal)."""
    n = K.shape[0]
    om2 = np.full(n_modes, np.nan)
    modes = np.full((n_modes, n // 6, 6), np.nan)
    res = np.full(n_modes, np.nan)
    found = 0
    for q in range(min(n_modes, len(mu))):
        if not mu[q] > 0.0:
            break
        om2[q] = 1.0 / mu[q]
        phi = np.zeros(n)
        phi[free] = V[:, q] * np.sqrt(om2[q])          # K-orthonormal -> M-orthonormal
        if phi[np.argmax(np.abs(phi))] < 0:
            phi = -phi
        kp, mp = (K @ phi)[free], (M @ phi)[free]
        res[q] = np.linalg.norm(kp - om2[q] * mp) / np.linalg.norm(kp)
        modes[q] = phi.reshape(-1, 6)
        found += 1
    return {"omega2": om2, "modes": modes, "residual": res, "n_found": found}


def vibration_modes_dense(K, M, fixed=None, n_modes=4):
    """The n_modes smallest omega^2 of K phi = omega^2 M phi on the free dofs by scipy.linalg.eigh of the pencil (K, M): dict
    omega2 (ascending), modes (n_modes, N, 6) with phi^T M phi = 1 and the largest component positive, residual
    |K phi - omega^2 M phi| / |K phi|, n_found, and omega2_all (every eigenvalue, ascending)."""
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    free = GH._free(fixed, K.shape[0])
    Kf = K[free][:, free].toarray()
    Mf = M[free][:, free].toarray()
    w, V = scipy.linalg.eigh(0.5 * (Kf + Kf.T), 0.5 * (Mf + Mf.T))
    out = _finish(K, M, free, 1.0 / w, V / np.sqrt(w)[None, :], n_modes)
    out["omega2_all"] = w
    return out


def vibration_modes_subspace(K, M, fixed=None, n_modes=4, n_sub=0, tol=1e-9, max_outer=200, seed=0, solve=None):
    """The algorithm of pl_vibration_modes with exact solves: geometric_host.buckling_modes_subspace on the pencil with
    K_g = -M (the shift stays 0: M is positive definite).  Returns the dict of ``vibration_modes_dense`` without omega2_all,
    plus outer_iterations and converged."""
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    sub = GH.buckling_modes_subspace(K, -M, fixed, n_modes, n_sub, tol, max_outer, seed, solve)
    free = GH._free(fixed, K.shape[0])
    found = sub["n_found"]
    mu = 1.0 / sub["load_factor"][:found]
    V = sub["modes"][:found].reshape(found, -1)[:, free].T
    out = _finish(K, M, free, mu, V, n_modes)
    out.update(outer_iterations=sub["outer_iterations"], converged=sub["converged"])
    return out


def vibration_sensitivity(node_xyz, beam_conn, radius, rho, drec_dr, fixed, omega2, modes, mult=None, rotary=True,
                          node_mass=None):
    """What pl_vibration_modes_sens computes: domega2_dr (n_modes, B), the derivatives of omega_i^2 to the strut radii at
    fixed segment geometry.  drec_dr: the radius derivative of the condensed records (stress_host.drecords_dr); fixed (N, 6)
    the Dirichlet mask; (omega2, modes) the eigenpairs (any scaling; the modes are read with the fixed dofs zeroed; a NaN
    omega2 gives a NaN row).  Per strut

        domega2_i/dr_b = (phi_e^T dK_e phi_e - omega_i^2 phi_e^T dM_e phi_e) / (phi_i^T M phi_i)

    with no adjoint solve: neither K nor M depends on a displacement field.  node_mass has no derivative.  The rows of an
    m-fold repeated frequency are not derivatives one by one; their sum over the cluster is the derivative of the sum."""
    d, conn = _spans(node_xyz, beam_conn)
    drec = np.asarray(drec_dr, dtype=float).reshape(-1, 8)
    om2 = np.asarray(omega2, dtype=float).reshape(-1)
    n = len(np.asarray(node_xyz).reshape(-1, 3))
    fixed = np.asarray(fixed).reshape(n, 6) != 0
    modes = np.where(fixed[None], 0.0, np.asarray(modes, dtype=float).reshape(len(om2), n, 6))
    M = mass_matrix(node_xyz, conn, radius, rho, mult, rotary, node_mass)
    dM = delement_matrix_dr(d, np.asarray(radius, dtype=float).reshape(-1), rho, mult, rotary)
    A, B = conn[:, 0], conn[:, 1]
    rows = np.full((len(om2), len(conn)), np.nan)
    for i in range(len(om2)):
        if np.isnan(om2[i]):
            continue
        phi = modes[i]
        mm = float(phi.reshape(-1) @ (M @ phi.reshape(-1)))
        pe = np.concatenate([phi[A], phi[B]], axis=1)
        rows[i] = (GH._pairing(drec, conn, phi, phi) - om2[i] * np.einsum("bi,bij,bj->b", pe, dM, pe)) / mm
    return rows


def frequency_aggregate(omega2, p):
    """(J, dJ_domega2): J = (sum_i (omega_i^2)^-p)^(1/p) >= 1 / omega_1^2 over the finite entries and its derivative
    (geometric_host.load_factor_aggregate: a symmetric function, differentiable through repeated frequencies)."""
    return GH.load_factor_aggregate(omega2, p)
