"""Numpy restatement of the strut stress pass (include/pylattice_hip.h: pl_stress / pl_stress_pnorm).

Vectorised over the struts, no device call: it reads the condensed records (``HipLattice.records()`` or ``records``
below), the segment data and a displacement field.  The host tests and the device parity tests use it as the yardstick.

Per strut (F, M_B) = tip force of the record; N = F.t, V = |F - N t|, T = M_B.t are constant along the strut, the bending
moment at arclength s is Mb(s) = |P (M_B + (L - s) t x F)|, P = I - t t^T.  Stations ``[A, q1, q2, B]`` (``stations``),
stress of a circular section of radius R: sigma = |N| / S + Mb R / I, tau = |T| R / J, sigma_vm = sqrt(sigma^2 + 3 tau^2).
With a strut multiplicity k every value is that of one of the k parallel copies (F / k, M / k).
"""
from __future__ import annotations

import numpy as np

FIELDS = ("N", "V", "T", "Mb", "sigma_vm")


def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def flexibility(radius, seg_len, seg_nsub, young, poisson, kappa=0.9, pen_coef=1.5, mult=None):
    """Tip flexibility sums of the condensed strut split by their power of the radius (pl_device.h strut_flexibility):
    dict fa, ft, s11 (~ r^-2, r^-4, r^-2) and b11, b12, b22 (~ r^-4).  mult: k parallel copies = a k times stiffer material."""
    r = np.asarray(radius, dtype=float)
    sl = np.asarray(seg_len, dtype=float).reshape(-1, 3)
    ns = np.asarray(seg_nsub).reshape(-1, 3)
    k = np.ones_like(r) if mult is None else np.asarray(mult, dtype=float)
    E = young * k
    G = young / (2.0 * (1.0 + poisson)) * k
    L = sl.sum(axis=1)
    f = {n: np.zeros_like(r) for n in ("fa", "ft", "s11", "b11", "b12", "b22")}
    s = np.zeros_like(r)
    for i in range(3):
        l = sl[:, i]
        on = l > 0
        R = r if i == 1 else pen_coef * r
        S, I = np.pi * R * R, 0.25 * np.pi * R ** 4
        n = np.where(on, ns[:, i], 1).astype(float)
        g11s = l / (G * kappa * S)
        g11b = l ** 3 / (3.0 * E * I) * (1.0 - 1.0 / (4.0 * n * n))
        g12, g22 = l * l / (2.0 * E * I), l / (E * I)
        d = L - (s + l)
        for name, v in (("fa", l / (E * S)), ("ft", l / (G * 2.0 * I)), ("s11", g11s),
                        ("b11", g11b + 2.0 * d * g12 + d * d * g22), ("b12", g12 + d * g22), ("b22", g22)):
            f[name] = f[name] + np.where(on, v, 0.0)
        s = s + np.where(on, l, 0.0)
    return f


def _scalars(f):
    f11, f12, f22 = f["s11"] + f["b11"], f["b12"], f["b22"]
    det = f11 * f22 - f12 * f12
    return 1.0 / f["fa"], 1.0 / f["ft"], f22 / det, f12 / det, f11 / det        # ka, kt, a, b, c


def _dscalars_dr(f, r):
    """d(ka, kt, a, b, c)/dr at fixed segment geometry: dF = -(2 / r) F_shear - (4 / r) F_bend, dK = -K dF K."""
    ka, kt, a, b, c = _scalars(f)
    d11 = -(2.0 / r) * f["s11"] - (4.0 / r) * f["b11"]
    d12, d22 = -(4.0 / r) * f["b12"], -(4.0 / r) * f["b22"]
    K = np.stack([np.stack([a, -b], -1), np.stack([-b, c], -1)], -2)
    dF = np.stack([np.stack([d11, d12], -1), np.stack([d12, d22], -1)], -2)
    dK = -K @ dF @ K
    return ka * 2.0 / r, kt * 4.0 / r, dK[:, 0, 0], -dK[:, 0, 1], dK[:, 1, 1]


def _record(scalars, d):
    ka, kt, a, b, c = scalars
    L2 = _dot(d, d)
    return np.column_stack([a, c, (ka - a) / L2, b / np.sqrt(L2), (kt - c) / L2, d])


def records(node_xyz, beam_conn, radius, seg_len, seg_nsub, young, poisson, kappa=0.9, pen_coef=1.5, mult=None):
    """(B, 8) condensed records (a, c, e1, e2, e3, dx, dy, dz), what pl_get_records returns."""
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    d = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    return _record(_scalars(flexibility(radius, seg_len, seg_nsub, young, poisson, kappa, pen_coef, mult)), d)


def drecords_dr(node_xyz, beam_conn, radius, seg_len, seg_nsub, young, poisson, kappa=0.9, pen_coef=1.5, mult=None):
    """(B, 8) radius derivative of ``records`` at fixed segment geometry (pl_device.h dscalars_dr / make_record): the
    derivatives of (a, c, e1, e2, e3) in columns 0 ... 4 and the span d itself, not a derivative, in columns 5 ... 7, so the
    result is a record that ``tip_force`` reads: tip_force(drecords_dr(...), conn, u) = (dK_e/dr u_e) on end B."""
    xyz = np.asarray(node_xyz, dtype=float).reshape(-1, 3)
    conn = np.asarray(beam_conn).reshape(-1, 2)
    d = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    r = np.asarray(radius, dtype=float)
    return _record(_dscalars_dr(flexibility(r, seg_len, seg_nsub, young, poisson, kappa, pen_coef, mult), r), d)


def tip_force(rec, conn, u):
    """(F, M_B) (B, 3) each: what the strut applies to its end beam_conn[:, 1] (pl_device.h tip_force)."""
    u = np.asarray(u, dtype=float).reshape(-1, 6)
    a, c, e1, e2, e3 = (rec[:, i:i + 1] for i in range(5))
    d = rec[:, 5:8]
    A, B = conn[:, 0], conn[:, 1]
    du = u[B, :3] - u[A, :3] + np.cross(d, u[A, 3:])
    dth = u[B, 3:] - u[A, 3:]
    F = a * du + e1 * _dot(du, d)[:, None] * d + e2 * np.cross(d, dth)
    M = c * dth + e3 * _dot(dth, d)[:, None] * d - e2 * np.cross(d, du)
    return F, M


def stations(seg_len, L, pen_coef=1.5, where=0):
    """Per strut and station of [A, q1, q2, B]: lever arm c = L - s (B, 4), radius factor (R = fac * r) and presence."""
    if where not in (0, 1):
        raise ValueError("where must be 0 (all stations) or 1 (the middle segment's ends)")
    sl = np.asarray(seg_len, dtype=float).reshape(-1, 3)
    l1, l2 = sl[:, 0], sl[:, 1]
    h1, h2, h3 = sl[:, 0] > 0, sl[:, 1] > 0, sl[:, 2] > 0
    c = np.stack([L, L - l1, L - (l1 + l2), np.zeros_like(L)], axis=1)
    one, no = np.ones_like(L), np.zeros(len(L), bool)
    if where == 1:
        return c, np.stack([one] * 4, axis=1), np.stack([no, h2, h2, no], axis=1)
    thin = min(pen_coef, 1.0)
    fac = np.stack([np.where(h1, pen_coef, np.where(h2, 1.0, pen_coef)), np.where(h2, thin, pen_coef), thin * one,
                    np.where(h3, pen_coef, np.where(h2, 1.0, pen_coef))], axis=1)
    return c, fac, np.stack([~no, h1 & (h2 | h3), h2 & h3, ~no], axis=1)


def _evaluate(rec, conn, radius, seg_len, u, pen_coef, mult, where, f_th=None):
    conn = np.asarray(conn).reshape(-1, 2)
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    r = np.asarray(radius, dtype=float)
    k = np.ones_like(r) if mult is None else np.asarray(mult, dtype=float)
    F, M = tip_force(rec, conn, u)
    d = rec[:, 5:8]
    L = np.sqrt(_dot(d, d))
    t = d / L[:, None]
    if f_th is not None:                                           # mechanical force under a thermal state: F - F_th t
        F = F - np.asarray(f_th, dtype=float)[:, None] * t
    Ft, Mt = _dot(F, t), _dot(M, t)
    Fp, Mp, tF = F - Ft[:, None] * t, M - Mt[:, None] * t, np.cross(t, F)
    c, fac, on = stations(seg_len, L, pen_coef, where)
    m = Mp[:, None, :] + c[:, :, None] * tF[:, None, :]            # (B, 4, 3): P M(s_i) of the whole record
    mn = np.sqrt(_dot(m, m))
    R = fac * r[:, None]
    iS, RI = 1.0 / (np.pi * R * R), 4.0 / (np.pi * R ** 3)
    RJ = 0.5 * RI
    ev = dict(F=F, M=M, t=t, k=k, c=c, on=on, m=m, mn=mn, iS=iS, RI=RI, RJ=RJ, r=r,
              N=Ft / k, V=np.sqrt(_dot(Fp, Fp)) / k, T=Mt / k, Mb=mn / k[:, None])
    ev["sgN"], ev["sgB"] = np.abs(ev["N"])[:, None] * iS, ev["Mb"] * RI
    ev["tau"] = np.abs(ev["T"])[:, None] * RJ
    ev["vm"] = np.sqrt((ev["sgN"] + ev["sgB"]) ** 2 + 3.0 * ev["tau"] ** 2)
    return ev


def strut_stress(rec, beam_conn, radius, seg_len, u, pen_coef=1.5, mult=None, where=0, f_th=None):
    """dict N, V, T, Mb, sigma_vm (B, 4) (NaN at absent stations) and peak (B,) - the outputs of pl_stress.  f_th (B,): the
    restrained thermal force ka delta of every record (thermal_host.restrained_force), subtracted along t as the device does
    under pl_set_thermal; None: no thermal state."""
    ev = _evaluate(rec, beam_conn, radius, seg_len, u, pen_coef, mult, where, f_th)
    on = ev["on"]
    out = {n: np.where(on, np.broadcast_to(ev[n][:, None], on.shape), np.nan) for n in ("N", "V", "T")}
    out["Mb"] = np.where(on, ev["Mb"], np.nan)
    out["sigma_vm"] = np.where(on, ev["vm"], np.nan)
    out["peak"] = np.where(on, ev["vm"], 0.0).max(axis=1)
    return out


def pnorm(sigma_vm, p):
    """(Phi_p, sigma_max) of the present (non-NaN) entries, evaluated without overflow: sigma_max (sum (s / sigma_max)^p)^(1/p)."""
    if not p >= 1:
        raise ValueError("p must be >= 1")
    s = np.asarray(sigma_vm, dtype=float)
    s = s[~np.isnan(s)]
    smax = float(s.max()) if s.size else 0.0
    if not smax > 0.0:
        return 0.0, smax
    return smax * float(((s / smax) ** p).sum()) ** (1.0 / p), smax


def scatter_tip_gradient(rec, conn, node_count, gF, gM):
    """(N, 6) derivative with respect to u of a scalar whose derivatives with respect to the struts' (F, M_B) are (gF, gM):
    the symmetric tip block applied to (g_F, g_M), added to end B and, moved to end A with reversed sign, to end A."""
    a, c, e1, e2, e3 = (rec[:, i:i + 1] for i in range(5))
    d = rec[:, 5:8]
    Gu = a * gF + e1 * _dot(gF, d)[:, None] * d + e2 * np.cross(d, gM)
    Gth = c * gM + e3 * _dot(gM, d)[:, None] * d - e2 * np.cross(d, gF)
    du = np.zeros((node_count, 6))
    np.add.at(du, conn[:, 1], np.column_stack([Gu, Gth]))
    np.add.at(du, conn[:, 0], np.column_stack([-Gu, -Gth - np.cross(d, Gu)]))
    return du


def stress_pnorm(rec, node_count, beam_conn, radius, seg_len, seg_nsub, u, p, young, poisson, kappa=0.9, pen_coef=1.5,
                 mult=None, where=0, want_grad=True, f_th=None):
    """(phi, sigma_max, dphi_du (N, 6), dphi_dr (B,)) - the outputs of pl_stress_pnorm with the formulas of its kernels;
    dphi_dr at fixed u and segment geometry, through the record (dscalars_dr) and the section constants.  f_th: as in
    ``strut_stress``; its radius derivative (2 / r) f_th t enters dphi_dr."""
    conn = np.asarray(beam_conn).reshape(-1, 2)
    ev = _evaluate(rec, conn, radius, seg_len, u, pen_coef, mult, where, f_th)
    on, vm = ev["on"], ev["vm"]
    phi, smax = pnorm(np.where(on, vm, np.nan), p)
    if not want_grad:
        return phi, smax, None, None
    nb = len(conn)
    if not smax > 0.0:
        return phi, smax, np.zeros((node_count, 6)), np.zeros(nb)
    ssum = float(np.where(on, (vm / smax) ** p, 0.0).sum())
    live = on & (vm > 0)
    vs = np.where(live, vm, 1.0)
    w = np.where(live, (vs / smax) ** (p - 1.0) * ssum ** (1.0 / p - 1.0), 0.0)
    ws, wt = w * (ev["sgN"] + ev["sgB"]) / vs, w * 3.0 * ev["tau"] / vs
    t, ik = ev["t"], 1.0 / ev["k"]
    mh = ev["m"] / np.where(ev["mn"] > 0, ev["mn"], 1.0)[:, :, None]
    mh = np.where((ev["mn"] > 0)[:, :, None], mh, 0.0)
    sN, sT = np.sign(ev["N"]), np.sign(ev["T"])
    gF = ((ws * ev["iS"]).sum(axis=1) * sN * ik)[:, None] * t \
        + ((ws * ev["RI"] * ev["c"])[:, :, None] * np.cross(mh, t[:, None, :])).sum(axis=1) * ik[:, None]
    gM = ((ws * ev["RI"])[:, :, None] * mh).sum(axis=1) * ik[:, None] + ((wt * ev["RJ"]).sum(axis=1) * sT * ik)[:, None] * t
    dsec = -((ws * (2.0 * ev["sgN"] + 3.0 * ev["sgB"]) + wt * 3.0 * ev["tau"]).sum(axis=1)) / ev["r"]
    rec = np.asarray(rec, dtype=float).reshape(-1, 8)
    d = rec[:, 5:8]
    du = scatter_tip_gradient(rec, conn, node_count, gF, gM)
    f = flexibility(radius, seg_len, seg_nsub, young, poisson, kappa, pen_coef, mult)
    drec = _record(_dscalars_dr(f, ev["r"]), d)
    dF, dM = tip_force(drec, conn, u)
    if f_th is not None:
        dF = dF - (2.0 * np.asarray(f_th, dtype=float) / ev["r"])[:, None] * t
    return phi, smax, du, _dot(gF, dF) + _dot(gM, dM) + dsec
