"""Numpy / scipy restatement of the geometric stiffness and the global linear buckling analysis
(include/pylattice_hip.h: pl_geom_spmv_multi / pl_buckling_modes / pl_buckling_modes_sens; csrc/pl_geom.h; DESIGN.md section
10d), in the manner of buckling_host.py.  No device call.

With u the equilibrium of the applied loads, the load factors are the smallest lambda > 0 with (K + lambda K_g(u)) phi = 0
on the free dofs.  Per strut, d = x_B - x_A, L = |d|, t = d / L and N = F.t the record's TOTAL axial force (tension > 0; a
record of multiplicity k already carries k copies).  The strut is ONE Hermite-cubic element between its two lattice nodes;
with g = N / (30 L), P = I - t t^T, delta = P (u_B - u_A), s_A = th_A x t, s_B = th_B x t:

    f_B = g [36 delta - 3 L (s_A + s_B)]                 f_A = -f_B
    m_A = t x g [-3 L delta + 4 L^2 s_A - L^2 s_B]       m_B = t x g [-3 L delta + 4 L^2 s_B - L^2 s_A]

- the textbook block N / (30 L) [[36, 3L, -36, 3L], [3L, 4L^2, -3L, -L^2], ...] in both bending planes, no axial and no
torsional terms.  A strut buckling between its own two joints is not represented (buckling_host.py covers that failure).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import stress_host as SH

ZERO_RITZ = 1e-10          # Ritz values below this share of the largest magnitude count as zero (as pl_buckling_modes)
DROP_PIVOT = 1e-12         # Cholesky pivots below this share of the largest diagonal entry are dropped


def _skew(v):
    v = np.asarray(v, dtype=float)
    out = np.zeros(v.shape[:-1] + (3, 3))
    out[..., 0, 1], out[..., 0, 2], out[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    out[..., 1, 2], out[..., 2, 0], out[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return out


def element_matrix(d, N):
    """(..., 12, 12) geometric stiffness of struts with span vectors d (..., 3) and axial forces N (...,), dofs
    [u_A, th_A, u_B, th_B] in global axes."""
    d = np.asarray(d, dtype=float)
    N = np.asarray(N, dtype=float)
    L = np.sqrt(SH._dot(d, d))
    t = d / L[..., None]
    g = (N / (30.0 * L))[..., None, None]
    L = L[..., None, None]
    X = _skew(t)                                       # X v = t x v;  th x t = -X th
    P = np.eye(3) - t[..., :, None] * t[..., None, :]
    K = np.zeros(d.shape[:-1] + (12, 12))
    uA, tA, uB, tB = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12)
    K[..., uB, uB] = 36.0 * P
    K[..., uB, uA] = -36.0 * P
    K[..., uB, tA] = 3.0 * L * X
    K[..., uB, tB] = 3.0 * L * X
    K[..., uA, :] = -K[..., uB, :]
    # t x (P v) = X v and t x (th x t) = P th
    K[..., tA, uA] = 3.0 * L * X
    K[..., tA, uB] = -3.0 * L * X
    K[..., tA, tA] = 4.0 * L * L * P
    K[..., tA, tB] = -L * L * P
    K[..., tB, uA] = 3.0 * L * X
    K[..., tB, uB] = -3.0 * L * X
    K[..., tB, tB] = 4.0 * L * L * P
    K[..., tB, tA] = -L * L * P
    return g * K


def axial_force(rec, beam_conn, u):
    """(B,) total axial force of every record, tension > 0 (the N of buckling_host times the multiplicity)."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    d = rec[:, 5:8]
    F, _ = SH.tip_force(rec, conn, u)
    return SH._dot(F, d / np.sqrt(SH._dot(d, d))[:, None])


def geometric_records(rec, beam_conn, u):
    """(B, 4) geometric records (g, dx, dy, dz), g = N / (30 L): what k_geom_records writes, in the caller's strut order."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    d = rec[:, 5:8]
    return np.column_stack([axial_force(rec, beam_conn, u) / (30.0 * np.sqrt(SH._dot(d, d))), d])


def _scatter(blocks, conn, n_nodes):
    """sparse (6N, 6N) sum of (B, 12, 12) element matrices with dofs [node A (6), node B (6)]."""
    conn = np.asarray(conn).reshape(-1, 2)
    dofs = (6 * conn[:, :, None] + np.arange(6)[None, None, :]).reshape(len(conn), 12)
    rows = np.repeat(dofs[:, :, None], 12, axis=2).ravel()
    cols = np.repeat(dofs[:, None, :], 12, axis=1).ravel()
    return sp.coo_matrix((blocks.ravel(), (rows, cols)), shape=(6 * n_nodes, 6 * n_nodes)).tocsr()


def geometric_matrix(rec, beam_conn, u, n_nodes):
    """sparse K_g(u) (6N, 6N) from the condensed records, the connectivity and the displacements."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    return _scatter(element_matrix(rec[:, 5:8], axial_force(rec, beam_conn, u)), beam_conn, n_nodes)


def elastic_matrix(rec, beam_conn, n_nodes):
    """sparse K (6N, 6N) of the condensed records (pl_device.h tip_blocks): the matrix pl_get_bsr returns."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    a, c, e1, e2, e3 = (rec[:, i] for i in range(5))
    d = rec[:, 5:8]
    L2 = SH._dot(d, d)

    def tip_blocks(a, c, e1, e2, e3, d):
        eye = np.eye(3)[None]
        dd = d[:, :, None] * d[:, None, :]
        D = _skew(d)
        Kss = np.zeros((len(a), 6, 6))
        Kss[:, :3, :3] = a[:, None, None] * eye + e1[:, None, None] * dd
        Kss[:, 3:, 3:] = c[:, None, None] * eye + e3[:, None, None] * dd
        Kss[:, :3, 3:] = e2[:, None, None] * D
        Kss[:, 3:, :3] = -e2[:, None, None] * D
        Rm = np.tile(np.eye(6), (len(a), 1, 1))
        Rm[:, :3, 3:] = -D
        return Kss, -Kss @ Rm

    Kbb, Kba = tip_blocks(a, c, e1, e2, e3, d)
    g = a - 2.0 * e2
    Kaa, _ = tip_blocks(a, c + L2 * g, e1, a - e2, e3 - g, -d)          # the record seen from end A (pl_device.h reversed)
    K = np.zeros((len(a), 12, 12))
    K[:, :6, :6], K[:, 6:, 6:], K[:, 6:, :6] = Kaa, Kbb, Kba
    K[:, :6, 6:] = np.swapaxes(Kba, 1, 2)
    return _scatter(K, beam_conn, n_nodes)


def geometric_apply(rec, beam_conn, u, X, fixed=None):
    """Y[j] = K_g(u) X[j] by the force formula, struts vectorised: X (k, N, 6) -> (k, N, 6).  fixed (N, 6) bool: the masked
    product P K_g P (X zeroed on the fixed dofs first, Y zeroed there afterwards)."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    X = np.array(X, dtype=float)
    one = X.ndim == 2
    X = X.reshape((-1,) + X.shape[-2:]) if not one else X[None]
    if fixed is not None:
        fixed = np.asarray(fixed).reshape(-1, 6) != 0
        X = np.where(fixed[None], 0.0, X)
    gr = geometric_records(rec, conn, u)
    g, d = gr[:, 0:1], gr[:, 1:4]
    L = np.sqrt(SH._dot(d, d))[:, None]
    t = d / L
    A, B = conn[:, 0], conn[:, 1]
    Y = np.zeros_like(X)
    for j in range(len(X)):
        x = X[j]
        du = x[B, :3] - x[A, :3]
        delta = du - SH._dot(du, t)[:, None] * t
        sA, sB = np.cross(x[A, 3:], t), np.cross(x[B, 3:], t)
        fB = g * (36.0 * delta - 3.0 * L * (sA + sB))
        mA = np.cross(t, g * (4.0 * L * L * sA - L * L * sB - 3.0 * L * delta))
        mB = np.cross(t, g * (4.0 * L * L * sB - L * L * sA - 3.0 * L * delta))
        np.add.at(Y[j], B, np.column_stack([fB, mB]))
        np.add.at(Y[j], A, np.column_stack([-fB, mA]))
    if fixed is not None:
        Y = np.where(fixed[None], 0.0, Y)
    return Y[0] if one else Y


def _free(fixed, n):
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed).reshape(-1) != 0
    if fixed.size != n:
        raise ValueError(f"fixed must have {n} entries")
    return np.flatnonzero(~fixed)


def _finish(K, Kg, free, mu, V, n_modes):
    """dict of the outputs of pl_buckling_modes from Ritz pairs (mu descending, V K-orthonormal on the free dofs)."""
    n = K.shape[0]
    scale = np.abs(mu).max() if len(mu) else 0.0
    lam = np.full(n_modes, np.nan)
    modes = np.full((n_modes, n // 6, 6), np.nan)
    res = np.full(n_modes, np.nan)
    found = 0
    for j in range(min(n_modes, len(mu))):
        if not mu[j] > ZERO_RITZ * scale:
            break
        phi = np.zeros(n)
        phi[free] = V[:, j]
        if phi[np.argmax(np.abs(phi))] < 0:
            phi = -phi
        lam[j] = 1.0 / mu[j]
        kp, gp = (K @ phi)[free], (Kg @ phi)[free]
        res[j] = np.linalg.norm(kp + lam[j] * gp) / np.linalg.norm(kp)
        modes[j] = phi.reshape(-1, 6)
        found += 1
    return {"load_factor": lam, "modes": modes, "residual": res, "n_found": found}


def buckling_modes_dense(K, Kg, fixed=None, n_modes=4):
    """The n_modes smallest positive load factors of (K + lambda K_g) phi = 0 on the free dofs by scipy.linalg.eigh of the
    pencil (-K_g, K): dict load_factor (ascending, NaN where none exists), modes (n_modes, N, 6) with phi^T K phi = 1 and
    the largest component positive, residual |K phi + lambda K_g phi| / |K phi|, n_found, and mu (every eigenvalue 1 / lambda
    of the pencil, descending)."""
    K, Kg = sp.csr_matrix(K), sp.csr_matrix(Kg)
    free = _free(fixed, K.shape[0])
    Kf = K[free][:, free].toarray()
    Gf = -Kg[free][:, free].toarray()
    mu, V = scipy.linalg.eigh(0.5 * (Gf + Gf.T), 0.5 * (Kf + Kf.T))
    mu, V = mu[::-1], V[:, ::-1]
    out = _finish(K, Kg, free, mu, V, n_modes)
    out["mu"] = mu
    return out


def ritz_step(Km, Gm):
    """Rayleigh-Ritz on projected matrices Km = Y^T K Y, Gm = Y^T G Y: Cholesky of Km with diagonal pivoting, directions
    whose pivot is negligible dropped, then the symmetric eigenproblem of L^-1 Gm L^-T.  Returns (mu descending (r,),
    C (n, r)) with C^T Km C = I, C^T Gm C = diag(mu)."""
    Km, Gm = 0.5 * (Km + Km.T), 0.5 * (Gm + Gm.T)
    n = len(Km)
    A = Km.copy()
    piv = np.arange(n)
    Lm = np.zeros((n, n))
    dmax = A.diagonal().max() if n else 0.0
    r = 0
    for k in range(n):
        best = k + int(np.argmax(A[piv[k:], piv[k:]]))
        p = A[piv[best], piv[best]]
        if not (p > DROP_PIVOT * dmax and p > 0.0):
            break
        piv[[k, best]] = piv[[best, k]]
        Lm[[k, best], :k] = Lm[[best, k], :k]
        Lm[k, k] = np.sqrt(p)
        rest = piv[k + 1:]
        Lm[k + 1:, k] = A[rest, piv[k]] / Lm[k, k]
        A[np.ix_(rest, rest)] -= np.outer(Lm[k + 1:, k], Lm[k + 1:, k])
        r = k + 1
    if r == 0:
        return np.zeros(0), np.zeros((n, 0))
    L1 = Lm[:r, :r]
    keep = piv[:r]
    T = scipy.linalg.solve_triangular(L1, Gm[np.ix_(keep, keep)], lower=True)
    Ar = scipy.linalg.solve_triangular(L1, T.T, lower=True).T
    mu, Q = np.linalg.eigh(0.5 * (Ar + Ar.T))
    mu, Q = mu[::-1], Q[:, ::-1]
    C = np.zeros((n, r))
    C[keep] = scipy.linalg.solve_triangular(L1.T, Q, lower=False)
    return mu, C


def buckling_modes_subspace(K, Kg, fixed=None, n_modes=4, n_sub=0, tol=1e-9, max_outer=200, seed=0, solve=None):
    """The algorithm of pl_buckling_modes with exact solves: shifted block subspace iteration on G phi = mu K phi, G = -K_g,
    lambda = 1 / mu.  Each outer step is Y = K^-1 (G X) + sigma X with sigma = max(0, -smallest Ritz value so far), then a
    Rayleigh-Ritz step on span(Y) with K Y and G Y actually applied; it stops when the n_modes largest Ritz values have
    changed by less than tol relatively.  solve(B) -> K_ff^-1 B replaces the sparse LU (an iterative inner solve, say).
    Returns the dict of ``buckling_modes_dense`` without mu, plus outer_iterations, converged and sigma (the largest shift)."""
    if n_sub == 0:
        n_sub = max(8, -(-2 * n_modes // 4) * 4)
    if n_sub % 4 or not 4 <= n_sub <= 32:
        raise ValueError("n_sub must be a multiple of 4 in 4 ... 32")
    if not 1 <= n_modes <= n_sub // 2:
        raise ValueError("n_modes must be 1 ... n_sub / 2")
    K, Kg = sp.csr_matrix(K), sp.csr_matrix(Kg)
    free = _free(fixed, K.shape[0])
    Kf = K[free][:, free].tocsc()
    Gf = -Kg[free][:, free].tocsr()
    if solve is None:
        solve = spla.splu(Kf).solve
    Y = np.random.default_rng(seed).uniform(-1.0, 1.0, (len(free), n_sub))
    cur = np.full(n_modes, -np.inf)
    mu_low, outer, converged, sigma_max = 0.0, 0, False, 0.0
    mu, X, GX = np.zeros(0), Y[:, :0], Y[:, :0]

    def ritz(Y):
        KY, GY = Kf @ Y, Gf @ Y
        mu, C = ritz_step(Y.T @ KY, Y.T @ GY)
        v = np.full(n_modes, -np.inf)
        m = min(n_modes, len(mu))
        scale = np.abs(mu).max() if len(mu) else 0.0
        v[:m] = np.where(np.abs(mu[:m]) <= ZERO_RITZ * scale, 0.0, mu[:m])
        return mu, Y @ C, GY @ C, v

    mu, X, GX, cur = ritz(Y)
    while len(mu) > 0 and outer < max_outer:
        if len(mu):
            mu_low = min(mu_low, mu[-1])
        sigma = max(0.0, -mu_low)
        sigma_max = max(sigma_max, sigma)
        prev = cur
        mu, X, GX, cur = ritz(solve(GX) + sigma * X)
        outer += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            change = np.where(cur == prev, 0.0, np.where((cur != 0) & np.isfinite(cur) & np.isfinite(prev),
                                                         np.abs(cur - prev) / np.abs(cur), np.inf))
        if change.max() < tol:
            converged = True
            break
    if len(mu) == 0:
        converged = True
    out = _finish(K, Kg, free, np.where(np.abs(mu) <= ZERO_RITZ * (np.abs(mu).max() if len(mu) else 0.0), 0.0, mu), X, n_modes)
    out.update(outer_iterations=outer, converged=converged, sigma=sigma_max)
    return out


def _pairing(rec, conn, x, y):
    """(B,) y_e^T K_e x_e for the elements of the records ``rec`` (pl_kernels.h strut_pairing): the tip force of x against
    the relative deformations of y."""
    conn = np.asarray(conn).reshape(-1, 2)
    y = np.asarray(y, dtype=float).reshape(-1, 6)
    F, M = SH.tip_force(rec, conn, x)
    A, B = conn[:, 0], conn[:, 1]
    return SH._dot(F, y[B, :3] - y[A, :3] + np.cross(rec[:, 5:8], y[A, 3:])) + SH._dot(M, y[B, 3:] - y[A, 3:])


def buckling_sensitivity(rec, drec_dr, beam_conn, u, fixed, load_factor, modes, solve=None):
    """What pl_buckling_modes_sens computes: (dlam_dr (n_modes, B), adj_load (n_modes, N, 6)), the derivatives of the load
    factors to the strut radii at fixed segment geometry, u following the radii through K u = f, and the loads w of the
    adjoint solves.  rec: the condensed records, drec_dr: their radius derivative (stress_host.drecords_dr), u (N, 6) the
    full equilibrium field, fixed (N, 6) the Dirichlet mask, (load_factor, modes) the eigenpairs (any scaling; the modes are
    read with the fixed dofs zeroed; a NaN factor gives NaN rows).  Per strut, with G_b = element_matrix(d_b, 1),
    ka = a + e1 L^2 (axial_force = ka t.(u_B - u_A)) and dK_e = dK_e/dr_b:

        kk = phi^T K phi,  q_b = phi_e^T G_b phi_e,  w = sum_b q_b ka_b (-t_b at u_A, +t_b at u_B),  K nu = -w (free dofs)
        dlambda/dr_b = (lambda / kk) [phi_e^T dK_e phi_e + lambda (q_b dka_b t_b.(u_B - u_A) + nu_e^T dK_e u_e)]

    The rows of an m-fold repeated factor are not derivatives one by one (the modes are an arbitrary basis of the eigenspace);
    their sum over the cluster is the derivative of the sum of those factors.  solve(b) -> K_ff^-1 b replaces the sparse LU."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    drec = np.asarray(drec_dr, dtype=float).reshape(-1, 8)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    u = np.asarray(u, dtype=float).reshape(-1, 6)
    n = len(u)
    lam = np.asarray(load_factor, dtype=float).reshape(-1)
    fixed = np.asarray(fixed).reshape(n, 6) != 0
    modes = np.where(fixed[None], 0.0, np.asarray(modes, dtype=float).reshape(len(lam), n, 6))
    free = _free(fixed, 6 * n)
    K = elastic_matrix(rec, conn, n)
    if solve is None:
        solve = spla.splu(K[free][:, free].tocsc()).solve
    d = rec[:, 5:8]
    L2 = SH._dot(d, d)
    t = d / np.sqrt(L2)[:, None]
    A, B = conn[:, 0], conn[:, 1]
    G = element_matrix(d, np.ones(len(d)))
    ka, dka = rec[:, 0] + rec[:, 2] * L2, drec[:, 0] + drec[:, 2] * L2
    stretch = SH._dot(t, u[B, :3] - u[A, :3])
    dlam = np.full((len(lam), len(rec)), np.nan)
    load = np.full((len(lam), n, 6), np.nan)
    for i in range(len(lam)):
        if np.isnan(lam[i]):
            continue
        phi = modes[i]
        kk = float(phi.reshape(-1) @ (K @ phi.reshape(-1)))
        pe = np.concatenate([phi[A], phi[B]], axis=1)
        q = np.einsum("bi,bij,bj->b", pe, G, pe)
        w = np.zeros((n, 6))
        np.add.at(w[:, :3], B, (q * ka)[:, None] * t)
        np.add.at(w[:, :3], A, -(q * ka)[:, None] * t)
        nu = np.zeros(6 * n)
        nu[free] = solve(-w.reshape(-1)[free])
        dlam[i] = lam[i] / kk * (_pairing(drec, conn, phi, phi) + lam[i] * (q * dka * stretch + _pairing(drec, conn, u, nu)))
        load[i] = w
    return dlam, load


def load_factor_aggregate(load_factor, p):
    """(J, dJ_dlambda): the p-norm J = (sum_i mu_i^p)^(1/p) of mu = 1 / lambda over the finite entries of load_factor,
    evaluated as mu_max (sum (mu / mu_max)^p)^(1/p), and its derivative (zero on the other entries).  J >= 1 / lambda_1, and J
    is a symmetric function of the factors: equal factors get equal weights, which the rows of a repeated factor need
    (buckling_sensitivity).  No finite entry: (0, zeros)."""
    lam = np.asarray(load_factor, dtype=float).reshape(-1)
    ok = np.isfinite(lam)
    dJ = np.zeros_like(lam)
    if not ok.any():
        return 0.0, dJ
    mu = 1.0 / lam[ok]
    mmax = mu.max()
    s = ((mu / mmax) ** p).sum()
    dJ[ok] = -(mu / mmax) ** (p - 1.0) * s ** (1.0 / p - 1.0) * mu * mu          # dJ/dmu dmu/dlambda
    return float(mmax * s ** (1.0 / p)), dJ
