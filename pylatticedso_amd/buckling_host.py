"""Numpy restatement of the strut buckling pass (include/pylattice_hip.h: pl_buckling / pl_buckling_pnorm; DESIGN.md
section 10c), the counterpart of stress_host.py.

Vectorised over the struts, no device call.  Per strut, with (F, M_B) the tip force of the condensed record and k its
multiplicity: N = F.t / k is the signed axial force of one copy (tension > 0), P = max(0, -N) its compressive part.  The
strut buckles as a column of the un-penalised radius r (I = pi r^4 / 4, S = pi r^2) and length l - the node-to-node length
(``length = 0``) or the middle segment (``length = 1``; a strut without one is absent: NaN, in no sum):

    N_E = pi^2 E I / (k_eff l)^2,      N_cr = N_E (``shear = 0``)  or  N_E / (1 + N_E / (kappa G S)) (``shear = 1``, Engesser)

Utilisation beta = P / N_cr; aggregate B_p = (sum beta^p)^(1/p) over the present struts.
"""
from __future__ import annotations

import numpy as np

from . import stress_host as SH


def critical_load(radius, ell, young, poisson, kappa=0.9, k_eff=1.0, shear=0):
    """(N_cr, q) per strut: Euler load of a column of length ``ell``, reduced by 1 + q with q = N_E / (kappa G S) when
    ``shear`` is 1 (q = 0 otherwise)."""
    if shear not in (0, 1):
        raise ValueError("shear must be 0 (Euler) or 1 (Engesser)")
    if not (k_eff > 0 and np.isfinite(k_eff)):
        raise ValueError("k_eff must be positive and finite")
    r = np.asarray(radius, dtype=float)
    with np.errstate(divide="ignore"):
        n_e = np.pi ** 2 * young * (0.25 * np.pi * r ** 4) / (k_eff * np.asarray(ell, dtype=float)) ** 2
    if not shear:
        return n_e, np.zeros_like(n_e)
    q = n_e / (kappa * young / (2.0 * (1.0 + poisson)) * np.pi * r ** 2)
    return n_e / (1.0 + q), q


def _evaluate(rec, conn, radius, seg_len, u, young, poisson, kappa, mult, length, k_eff, shear, f_th=None):
    if length not in (0, 1):
        raise ValueError("length must be 0 (node to node) or 1 (the middle segment)")
    conn = np.asarray(conn).reshape(-1, 2)
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    r = np.asarray(radius, dtype=float).reshape(-1)
    k = np.ones_like(r) if mult is None else np.asarray(mult, dtype=float)
    d = rec[:, 5:8]
    span = np.sqrt(SH._dot(d, d))
    t = d / span[:, None]
    F, _ = SH.tip_force(rec, conn, u)
    if f_th is not None:                                           # mechanical force under a thermal state: F - F_th t
        F = F - np.asarray(f_th, dtype=float)[:, None] * t
    mid = np.asarray(seg_len, dtype=float).reshape(-1, 3)[:, 1]
    on = np.ones(len(r), bool) if length == 0 else mid > 0
    ell = span if length == 0 else np.where(on, mid, 1.0)
    n_cr, q = critical_load(r, ell, young, poisson, kappa, k_eff, shear)
    N = SH._dot(F, t) / k
    beta = np.maximum(0.0, -N) / n_cr
    return dict(conn=conn, rec=rec, r=r, k=k, d=d, t=t, on=on, N=N, n_cr=n_cr, q=q, beta=beta)


def strut_buckling(rec, beam_conn, radius, seg_len, u, young, poisson, kappa=0.9, mult=None, length=1, k_eff=1.0, shear=0,
                   f_th=None):
    """dict util (beta), n_axial (signed N of one copy), n_crit (N_cr), each (B,), NaN on absent struts - the outputs of
    pl_buckling.  f_th (B,): the restrained thermal force of every record (stress_host.strut_stress); None: no thermal state."""
    ev = _evaluate(rec, beam_conn, radius, seg_len, u, young, poisson, kappa, mult, length, k_eff, shear, f_th)
    return {"util": np.where(ev["on"], ev["beta"], np.nan), "n_axial": np.where(ev["on"], ev["N"], np.nan),
            "n_crit": np.where(ev["on"], ev["n_cr"], np.nan)}


def pnorm(util, p):
    """(B_p, beta_max) of the present (non-NaN) entries without overflow: beta_max (sum (beta / beta_max)^p)^(1/p)."""
    return SH.pnorm(util, p)


def buckling_pnorm(rec, node_count, beam_conn, radius, seg_len, seg_nsub, u, p, young, poisson, kappa=0.9, pen_coef=1.5,
                   mult=None, length=1, k_eff=1.0, shear=0, want_grad=True, f_th=None):
    """(bp, util_max, dbp_du (N, 6), dbp_dr (B,)) - the outputs of pl_buckling_pnorm; dbp_dr at fixed u and segment geometry,
    through the record (its radius derivative) and through N_cr(r).  f_th: as in ``strut_buckling``; its radius derivative
    (2 / r) f_th t enters dbp_dr."""
    ev = _evaluate(rec, beam_conn, radius, seg_len, u, young, poisson, kappa, mult, length, k_eff, shear, f_th)
    on, beta = ev["on"], ev["beta"]
    bp, bmax = pnorm(np.where(on, beta, np.nan), p)
    if not want_grad:
        return bp, bmax, None, None
    nb = len(ev["conn"])
    if not bmax > 0.0:
        return bp, bmax, np.zeros((node_count, 6)), np.zeros(nb)
    live = on & (ev["N"] < 0)
    x = np.where(live, beta / bmax, 0.0)
    total = float((x ** p).sum())
    w = np.where(live, x ** (p - 1.0) * total ** (1.0 / p - 1.0), 0.0)            # dB / d beta_b
    gF = (-w / (ev["k"] * ev["n_cr"]))[:, None] * ev["t"]                          # dB / dF; dB / dM_B = 0
    conn, d = ev["conn"], ev["d"]
    du = SH.scatter_tip_gradient(ev["rec"], conn, node_count, gF, np.zeros_like(gF))
    f = SH.flexibility(ev["r"], seg_len, seg_nsub, young, poisson, kappa, pen_coef, mult)
    dF, _ = SH.tip_force(SH._record(SH._dscalars_dr(f, ev["r"]), d), conn, u)
    if f_th is not None:
        dF = dF - (2.0 * np.asarray(f_th, dtype=float) / ev["r"])[:, None] * ev["t"]
    q = ev["q"]
    dbeta = -beta * (4.0 - 2.0 * q / (1.0 + q)) / ev["r"]                          # at fixed P: N_E ~ r^4, q ~ r^2
    return bp, bmax, du, np.where(live, SH._dot(gF, dF) + w * dbeta, 0.0)
