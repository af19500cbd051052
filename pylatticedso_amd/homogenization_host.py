"""Numpy / scipy restatement of the periodic homogenisation of one cell and of its radius sensitivities
(include/pylattice_hip.h: pl_sens_gram; csrc/pl_sensgram.h; homogenization_cell.py), in the manner of
stress_host.py / geometric_host.py.  No device call.

The six total fields u_k = w_k + fluctuation_k of ``HomogenizedCell`` are in equilibrium against every periodic variation
(P^T K u_k = 0 on the free reduced dofs), and the macro stress of case l read against the macro strain of case k is a strain
energy product (Hill-Mandel, tests/test_homogenization_oracle.py):

    E_kl = u_k^T K u_l = scale_k H_raw[k, l],        scale = (1, 1, 1, 2, 2, 2)   (the shear cases are tensorial: gamma = 2)

``H_raw`` is the un-symmetrised matrix ``solve_full_homogenization`` builds, ``homogenizeMatrix = sym(H_raw)``.  A radius
changes K and, through the solves, the fluctuations; the variation of a fluctuation is itself periodic with the anchor fixed,
so K u_l does no work on it and the derivative needs NO adjoint solve:

    dE_kl / dr_b = u_k,e^T (dK_e / dr_b) u_l,e

- the per-strut Gram of the six fields in the strut's radius derivative (``sens_gram``, on the device pl_sens_gram), at fixed
segment geometry (the convention of pl_sens: exact when joint penalisation is off; with penalisation on, the change of the
penalised lengths with the radius is not included, exactly as in LatticeOpti's gradients).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg
import scipy.sparse as sp

from . import geometric_host as GH
from .homogenization_cell import _VOIGT, imposed_displacement, periodic_masters

SCALE = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])          # E_kl = SCALE[k] * H_raw[k, l]
CONSTANTS = ("Ex", "Ey", "Ez", "Gxy", "Gxz", "Gyz", "nuxy", "nuxz", "nuyz")


def _columns(X, n_nodes=None):
    X = np.asarray(X, dtype=float)
    if X.ndim == 2:
        X = X.reshape(X.shape[0], -1, 6)
    if X.ndim != 3 or X.shape[2] != 6 or (n_nodes is not None and X.shape[1] != n_nodes):
        raise ValueError(f"X must have shape (k, N, 6) or (k, 6 N), got {X.shape}")
    return X


def sens_gram(drec_dr, beam_conn, X):
    """(k, k, B): G[k, l, b] = X[k]_e^T (dK_e/dr_b) X[l]_e - what pl_sens_gram computes.  drec_dr: the radius derivative of
    the records (stress_host.drecords_dr), X (k, N, 6) or (k, 6 N).  Every entry is evaluated on its own (the tip force of
    X[l] against the deformations of X[k]), so the symmetry of the result is a property of the formula, not of the code."""
    drec = np.asarray(drec_dr, dtype=float).reshape(-1, 8)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    X = _columns(X)
    k = len(X)
    out = np.empty((k, k, len(drec)))
    for i in range(k):
        for j in range(k):
            out[i, j] = GH._pairing(drec, conn, X[j], X[i])
    return out


def homogenize(rec, beam_conn, node_xyz, lo, size):
    """(H_raw (6, 6), U_tot (6, N, 6)) of one periodic cell with the condensed records ``rec`` (stress_host.records), corner
    ``lo`` and edge lengths ``size``: the dense periodic solve of ``HomogenizedCell(solver="host")`` on
    geometric_host.elastic_matrix instead of the device's BSR - same periodic groups (periodic_masters), same anchor rule
    (the vertex at the cell centre, else the first master node), reactions summed over every boundary node."""
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    lo, size = np.asarray(lo, dtype=float), np.asarray(size, dtype=float)
    N = len(xyz)
    K = GH.elastic_matrix(rec, beam_conn, N)
    master, boundary = periodic_masters(xyz, lo, size)
    masters = np.unique(master)
    slot = np.full(N, -1, np.int64)
    slot[masters] = np.arange(len(masters))
    node_slot = slot[master]
    cols = (6 * node_slot[:, None] + np.arange(6)).ravel()
    P = sp.csr_matrix((np.ones(6 * N), (np.arange(6 * N), cols)), shape=(6 * N, 6 * len(masters)))
    Kr = (P.T @ K @ P).toarray()
    d = np.abs(xyz - (lo + 0.5 * size)).max(axis=1)
    centre = int(np.argmin(d))
    anchor = int(node_slot[centre]) if d[centre] <= 1e-6 else 0
    free = np.setdiff1d(np.arange(Kr.shape[0]), 6 * anchor + np.arange(3))
    try:
        factor = scipy.linalg.cho_factor(Kr[np.ix_(free, free)])
    except np.linalg.LinAlgError as err:
        raise RuntimeError("homogenisation: the periodic cell operator is singular (mechanism in the cell?)") from err
    H = np.empty((6, 6))
    U = np.empty((6, N, 6))
    for k in range(6):
        w = imposed_displacement(k + 1, xyz)
        ur = np.zeros(P.shape[1])
        ur[free] = scipy.linalg.cho_solve(factor, -(P.T @ (K @ w.ravel()))[free])
        U[k] = w + (P @ ur).reshape(N, 6)
        R = (K @ U[k].ravel()).reshape(N, 6)
        s = R[boundary, :3].T @ xyz[boundary]
        H[:, k] = [s[i][j] for i, j in _VOIGT]
    return H, U


def homogenized_sensitivity(drec_dr, beam_conn, U_tot):
    """dH_raw (6, 6, B): the derivative of every entry of H_raw to every strut radius at fixed segment geometry, from the six
    total fields U_tot (6, N, 6) of ``homogenize`` (or of HomogenizedCell.saveDataToExport): sens_gram / SCALE by rows."""
    U = _columns(U_tot)
    if len(U) != 6:
        raise ValueError("U_tot must hold the six total fields")
    return sens_gram(drec_dr, beam_conn, U) / SCALE[:, None, None]


def engineering_constants(H_raw):
    """(9,) Ex, Ey, Ez, Gxy, Gxz, Gyz, nuxy, nuxz, nuyz of HomogenizedCell._engineering_constants: from the inverse of the
    UN-symmetrised matrix, as the class (and the reference) computes them."""
    Hi = np.linalg.inv(np.asarray(H_raw, dtype=float))
    Ex, Ey, Ez = 1.0 / Hi[0, 0], 1.0 / Hi[1, 1], 1.0 / Hi[2, 2]
    return np.array([Ex, Ey, Ez, 1.0 / (2.0 * Hi[3, 3]), 1.0 / (2.0 * Hi[4, 4]), 1.0 / (2.0 * Hi[5, 5]),
                     -Hi[0, 1] * Ey, -Hi[0, 2] * Ez, -Hi[1, 2] * Ez])


def engineering_constants_sensitivity(H_raw, dH_raw):
    """(9, B) derivatives of ``engineering_constants`` for the derivatives dH_raw (6, 6, B) of the matrix:
    dHinv = -Hinv dH Hinv, then the quotient rule on the nine formulas."""
    Hi = np.linalg.inv(np.asarray(H_raw, dtype=float))
    dH = np.asarray(dH_raw, dtype=float)
    dHi = -np.einsum("ij,jkb,kl->ilb", Hi, dH, Hi)
    Ey, Ez = 1.0 / Hi[1, 1], 1.0 / Hi[2, 2]
    dE = [-dHi[i, i] / Hi[i, i] ** 2 for i in range(3)]
    dG = [-dHi[i, i] / (2.0 * Hi[i, i] ** 2) for i in range(3, 6)]
    dnu = [-dHi[0, 1] * Ey - Hi[0, 1] * dE[1], -dHi[0, 2] * Ez - Hi[0, 2] * dE[2], -dHi[1, 2] * Ez - Hi[1, 2] * dE[2]]
    return np.stack(dE + dG + dnu)


def per_radius(d_per_strut, beam_type, n_geometries):
    """Sum a per-strut derivative (..., B) over the struts of every geometry of the cell: (..., n_geometries), the
    derivative to the cell's ``radii`` entries (every strut of geometry g has the radius radii[g] times a fixed factor 1 in
    a one-cell lattice)."""
    d = np.asarray(d_per_strut, dtype=float)
    out = np.zeros(d.shape[:-1] + (int(n_geometries),))
    np.add.at(np.moveaxis(out, -1, 0), np.asarray(beam_type), np.moveaxis(d, -1, 0))
    return out
