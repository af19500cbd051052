"""Numpy restatement of the thermal loads of the struts (include/pylattice_hip.h: pl_set_thermal / pl_thermal_load /
pl_thermal_sens; csrc/pl_thermal.h), the counterpart of stress_host.py and buckling_host.py.

Vectorised over the struts, no device call.  Strut b joins A = beam_conn[b, 0] and B = beam_conn[b, 1], d = x_B - x_A,
L = |d|, t = d / L.  The temperature rise is given per node, linear along the strut and uniform over the section:

    delta_b = alpha_b L (dT_A + dT_B) / 2                 free elongation (no radius, no penalised segment)
    F_th,b  = ka_b delta_b,  ka_b = rec.a + rec.e1 L^2    restrained force of the record, multiplicity k included
    n_free_b = F_th,b / k                                 that of one copy
    f_th: +F_th t on the translations of B, -F_th t on those of A, no moments;  K u = f_ext + f_th.

The mechanical section force is K_tip (du, dth) - F_th t, so only N shifts: N = (F.t - F_th) / k.  At fixed segment
geometry d ka / dr = 2 ka / r, so lam^T d f_th / d r_b = (2 ka_b / r_b) delta_b t . (lam_u,B - lam_u,A).
"""
from __future__ import annotations

import numpy as np

from . import stress_host as SH


def elongation(node_xyz, beam_conn, alpha, node_dT):
    """(B,) free elongations delta_b; alpha a scalar or (B,), node_dT a scalar or (N,)."""
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    dT = np.broadcast_to(np.asarray(node_dT, dtype=float), (len(xyz),))
    d = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    return np.asarray(alpha, dtype=float) * np.sqrt(SH._dot(d, d)) * (0.5 * (dT[conn[:, 0]] + dT[conn[:, 1]]))


def axial_stiffness(rec):
    """(B,) condensed axial stiffness ka = a + e1 L^2 of the records (B, 8)."""
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    return rec[:, 0] + rec[:, 2] * SH._dot(rec[:, 5:8], rec[:, 5:8])


def restrained_force(rec, delta):
    """(B,) F_th = ka delta of the whole record: the ``f_th`` that stress_host and buckling_host take."""
    return axial_stiffness(rec) * np.asarray(delta, dtype=float)


def _tangent(rec):
    d = np.asarray(rec, dtype=float).reshape(-1, 8)[:, 5:8]
    return d / np.sqrt(SH._dot(d, d))[:, None]


def thermal_load(rec, beam_conn, node_count, delta, mult=None):
    """(f_th (N, 6), n_free (B,)) - the outputs of pl_thermal_load."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    fth = restrained_force(rec, delta)
    k = np.ones_like(fth) if mult is None else np.asarray(mult, dtype=float)
    ft = fth[:, None] * _tangent(rec)
    f = np.zeros((node_count, 6))
    np.add.at(f[:, :3], conn[:, 1], ft)
    np.add.at(f[:, :3], conn[:, 0], -ft)
    return f, fth / k


def thermal_sens(rec, beam_conn, radius, delta, lam):
    """(B,) lam^T d f_th / d r_b at fixed segment geometry - the output of pl_thermal_sens."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    lam = np.asarray(lam, dtype=float).reshape(-1, 6)
    dl = lam[conn[:, 1], :3] - lam[conn[:, 0], :3]
    return 2.0 * restrained_force(rec, delta) / np.asarray(radius, dtype=float) * SH._dot(_tangent(rec), dl)


def axial_force(rec, beam_conn, u, delta=None, mult=None):
    """(B,) signed mechanical axial force of one copy, N = (F.t - F_th) / k; delta = None: no thermal state."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    F, _ = SH.tip_force(rec, conn, u)
    N = SH._dot(F, _tangent(rec))
    if delta is not None:
        N = N - restrained_force(rec, delta)
    return N if mult is None else N / np.asarray(mult, dtype=float)


def periodic_total_fields(rec, beam_conn, node_xyz, cell_lo, cell_size):
    """(U (6, N, 6), K) of a one-cell lattice: the six total fields w_k + u_k of the unit macro strains under periodic
    fluctuations (what HomogenizedCell.solve_full_homogenization keeps in saveDataToExport), by a dense host solve, and
    the dense elastic matrix."""
    import scipy.linalg
    from . import geometric_host as GH
    from .homogenization_cell import imposed_displacement, periodic_masters
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    N = len(xyz)
    K = GH.elastic_matrix(rec, beam_conn, N)
    K = K.toarray() if hasattr(K, "toarray") else np.asarray(K)
    master, _ = periodic_masters(xyz, np.asarray(cell_lo, dtype=float), np.asarray(cell_size, dtype=float))
    masters = np.unique(master)
    slot = np.full(N, -1, np.int64)
    slot[masters] = np.arange(len(masters))
    cols = (6 * slot[master][:, None] + np.arange(6)).ravel()
    P = np.zeros((6 * N, 6 * len(masters)))
    P[np.arange(6 * N), cols] = 1.0
    free = np.setdiff1d(np.arange(P.shape[1]), np.arange(3))        # translations of the first master group anchored
    Kr = P.T @ K @ P
    factor = scipy.linalg.cho_factor(Kr[np.ix_(free, free)])
    U = []
    for case in range(1, 7):
        w = imposed_displacement(case, xyz).ravel()
        v = np.zeros(P.shape[1])
        v[free] = scipy.linalg.cho_solve(factor, -(P.T @ (K @ w))[free])
        U.append((w + P @ v).reshape(N, 6))
    return np.stack(U), K


def expansion_from_fields(U, KU, f_th):
    """alpha_hom (6,) = H^-1 tau with H_kl = u_k^T K u_l and tau_k = u_k^T f_th: U (6, N, 6) the total fields, KU (6, N, 6)
    = K U, f_th (N, 6) the thermal load at dT = 1.  Components in the order of the six macro strains (xx, yy, zz, xy, xz,
    yz; the shear amplitudes are tensorial strains, as the macro strains are)."""
    U = np.asarray(U, dtype=float).reshape(6, -1)
    H = U @ np.asarray(KU, dtype=float).reshape(6, -1).T
    tau = U @ np.asarray(f_th, dtype=float).reshape(-1)
    return np.linalg.solve(0.5 * (H + H.T), tau)


def homogenized_expansion(rec, beam_conn, node_xyz, cell_lo, cell_size, alpha):
    """alpha_hom (6,) of a one-cell periodic lattice, the strain of the stress-free cell per unit temperature: no extra
    solve beyond the six total fields of the homogenisation.  alpha a scalar or (B,)."""
    U, K = periodic_total_fields(rec, beam_conn, node_xyz, cell_lo, cell_size)
    N = U.shape[1]
    delta = elongation(node_xyz, beam_conn, alpha, 1.0)
    f_th, _ = thermal_load(rec, beam_conn, N, delta)
    KU = (K @ U.reshape(6, -1).T).T
    return expansion_from_fields(U, KU, f_th)
