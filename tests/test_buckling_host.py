"""Host side of the strut buckling pass (pl_buckling / pl_buckling_pnorm), no GPU: the numpy restatement
(pylatticedso_amd/buckling_host.py, the yardstick of the device parity tests) against a compressed column in closed form,
its axial force against the reference's own sub-meshed model, the sign properties of the utilisation, its derivatives
against central differences, the bounds of the aggregate, and the C ABI's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import timoshenko_oracle as O
from pylatticedso_amd import _capi
from pylatticedso_amd import buckling_host as BH
from pylatticedso_amd import stress_host as SH

E, NU, KAPPA, PEN = 1013.0, 0.3, 0.9, 1.5
EPS = np.finfo(float).eps


# ---------------------------------------------------------------------------------------------------------------------
# one strut in a skew direction, clamped at A, axial force at B
# ---------------------------------------------------------------------------------------------------------------------
SEGMENTS = {"three": ((0.11, 0.53, 0.07), (3, 9, 2)), "plain": ((0.0, 0.71, 0.0), (0, 12, 0))}


def _column(case, load, mult=None):
    """The strut's records and its displacements under the force ``load`` x t at B (negative = pushed)."""
    seg_len, seg_n = SEGMENTS[case]
    r, L = 0.04, sum(seg_len)
    t = np.array([2.0, -1.0, 0.5])
    t /= np.linalg.norm(t)
    xyz = np.array([[0.3, 0.1, -0.2], [0.3, 0.1, -0.2] + L * t])
    k = 1.0 if mult is None else mult
    Kbb = k * O.beam_matrix(O.condensed_beam(r, seg_len, seg_n, E, NU), xyz[1] - xyz[0])[6:, 6:]
    u = np.zeros((2, 6))
    u[1] = np.linalg.solve(Kbb, np.r_[load * t, 0, 0, 0])
    m = None if mult is None else [mult]
    rec = SH.records(xyz, [[0, 1]], [r], [seg_len], [seg_n], E, NU, KAPPA, PEN, m)
    tol = 100 * np.linalg.cond(Kbb) * EPS          # round-off of the 6 x 6 solve that produced u
    return dict(rec=rec, r=r, L=L, seg_len=seg_len, u=u, mult=m, tol=tol)


def _beta(c, length, k_eff, shear):
    return BH.strut_buckling(c["rec"], [[0, 1]], [c["r"]], [c["seg_len"]], c["u"], E, NU, KAPPA, c["mult"], length, k_eff, shear)


@pytest.mark.parametrize("shear", [0, 1])
@pytest.mark.parametrize("k_eff", [1.0, 0.5])
@pytest.mark.parametrize("length", [0, 1])
@pytest.mark.parametrize("case", sorted(SEGMENTS))
def test_column_closed_form(case, length, k_eff, shear):
    """beta = P (k_eff l)^2 / (pi^2 E I), times 1 + N_E / (kappa G S) with shear; l = |d| or the middle segment; two parallel
    copies carry half each; the same strut pulled has beta = 0 exactly."""
    P = 0.37
    c = _column(case, -P)
    r = c["r"]
    ell = c["L"] if length == 0 else c["seg_len"][1]
    I, S, G = 0.25 * np.pi * r ** 4, np.pi * r ** 2, E / (2 * (1 + NU))
    n_e = np.pi ** 2 * E * I / (k_eff * ell) ** 2
    want = P * (k_eff * ell) ** 2 / (np.pi ** 2 * E * I)
    n_cr = n_e
    if shear:
        n_cr = n_e / (1 + n_e / (KAPPA * G * S))
        want = P / n_cr
        assert want > P / n_e                                       # shear flexibility lowers the critical load
    out = _beta(c, length, k_eff, shear)
    assert np.isclose(out["util"][0], want, rtol=c["tol"], atol=0), (out["util"][0], want)
    assert np.isclose(out["n_axial"][0], -P, rtol=c["tol"], atol=0)
    assert np.isclose(out["n_crit"][0], n_cr, rtol=1e-14, atol=0)
    two = _column(case, -P, mult=2.0)
    out2 = _beta(two, length, k_eff, shear)
    assert np.isclose(out2["util"][0], 0.5 * want, rtol=two["tol"], atol=0)
    assert np.isclose(out2["n_axial"][0], -0.5 * P, rtol=two["tol"], atol=0) and out2["n_crit"][0] == out["n_crit"][0]
    pulled = _beta(_column(case, P), length, k_eff, shear)
    assert pulled["util"][0] == 0.0 and pulled["n_axial"][0] > 0


def test_no_middle_segment_is_absent_under_length_1():
    xyz = np.array([[0.0, 0, 0], [0.5, 0, 0]])
    sl, sn = [[0.2, 0.0, 0.3]], [[3, 0, 4]]
    rec = SH.records(xyz, [[0, 1]], [0.03], sl, sn, E, NU)
    u = np.zeros((2, 6))
    u[1, 0] = -1e-3                                                  # compressed
    out = BH.strut_buckling(rec, [[0, 1]], [0.03], sl, u, E, NU, length=1)
    assert all(np.isnan(out[k][0]) for k in ("util", "n_axial", "n_crit"))
    bp, bmax, du, dr = BH.buckling_pnorm(rec, 2, [[0, 1]], [0.03], sl, sn, u, 8, E, NU, length=1)
    assert (bp, bmax) == (0.0, 0.0) and not du.any() and not dr.any()
    assert BH.strut_buckling(rec, [[0, 1]], [0.03], sl, u, E, NU, length=0)["util"][0] > 0
    for bad in (dict(length=2), dict(shear=-1), dict(k_eff=0.0), dict(k_eff=float("inf"))):
        with pytest.raises(ValueError):
            BH.strut_buckling(rec, [[0, 1]], [0.03], sl, u, E, NU, **bad)


# ---------------------------------------------------------------------------------------------------------------------
# a small lattice
# ---------------------------------------------------------------------------------------------------------------------
def _lattice(cells=(2, 1, 1), geoms=("BCC",), radii=(0.05,)):
    from pylatticedso_amd.lattice_sim import LatticeSim
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                                    "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                                    "radii": list(radii), "geom_types": list(geoms)},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                       "boundary_conditions": {
                           "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                      "Value": [0, 0, 0, 0, 0, 0]}},
                           "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})


class _Problem:
    """Records and segment data of a lattice, a generic displacement field and the restatement's calls on them."""

    def __init__(self, L, seed, mult=False, vary_radii=False):
        lat, pen = L.lattice, L.penalized
        rng = np.random.default_rng(seed)
        self.xyz, self.conn, self.sl, self.sn = lat.node_xyz, lat.beam_conn, pen.seg_len, pen.seg_nsub
        self.nn, self.nb = lat.n_nodes, lat.n_beams
        self.mat = (L.young_modulus, L.poisson_ratio, KAPPA, L.penalization_coefficient)
        self.mult = rng.integers(1, 3, self.nb).astype(float) if mult else None
        self.rad = lat.beam_radius * (0.8 + 0.4 * rng.random(self.nb)) if vary_radii else np.array(lat.beam_radius, float)
        self.u = rng.standard_normal((self.nn, 6)) * np.array([1, 1, 1, 3, 3, 3]) * 1e-3

    def records(self, rad=None):
        Em, nu, kappa, pc = self.mat
        return SH.records(self.xyz, self.conn, self.rad if rad is None else rad, self.sl, self.sn, Em, nu, kappa, pc, self.mult)

    def struts(self, u=None, rad=None, **kw):
        Em, nu, kappa, _ = self.mat
        rad = self.rad if rad is None else rad
        return BH.strut_buckling(self.records(rad), self.conn, rad, self.sl, self.u if u is None else u, Em, nu, kappa,
                                 self.mult, **kw)

    def pnorm(self, p, u=None, rad=None, want_grad=True, **kw):
        Em, nu, kappa, pc = self.mat
        rad = self.rad if rad is None else rad
        return BH.buckling_pnorm(self.records(rad), self.nn, self.conn, rad, self.sl, self.sn, self.u if u is None else u, p,
                                 Em, nu, kappa, pc, self.mult, want_grad=want_grad, **kw)


def test_axial_force_of_the_submeshed_model():
    """n_axial of the restatement on the condensed displacements against the axial component of the nodal force K_e u_e of
    the first sub-element of every strut in the reference's sub-meshed model of the same problem (N is constant along a
    strut, so one sub-element per strut says it all).  The condensation is exact: the two differ by the round-off of two
    direct solves, bounded as in tests/test_stress_host.py by (relative difference of the two displacement fields at the
    lattice nodes + 8 eps) x (largest row sum of |K_e| x largest |u|)."""
    from pylatticedso_amd.views import _tables
    L = _lattice()
    lat, pen = L.lattice, L.penalized
    Em, nu = L.young_modulus, L.poisson_ratio
    assert L.is_penalized and (pen.seg_len[:, 0] > 0).any() and (pen.seg_len[:, 2] > 0).any()
    t = _tables(L)
    h = 0.05 * L.cell_size_x
    fixed = np.asarray(L.fixed_DOF, bool)
    f = np.where(fixed, 0.0, np.random.default_rng(3).standard_normal(fixed.shape) * np.array([1, 1, 1, 0.05, 0.05, 0.05]))
    sc = np.array([O.condensed_beam(r, l, n, Em, nu) for r, l, n in zip(lat.beam_radius, pen.seg_len, pen.seg_nsub)])
    Kc = O.assemble_condensed(lat.node_xyz, lat.beam_conn, sc)
    u_c = O.solve_dirichlet(Kc, fixed.ravel(), np.zeros(fixed.size), f.ravel()).reshape(-1, 6)
    K, nv = O.assemble_submeshed(t.node_xyz, t.beam_conn, t.beam_radius, Em, nu, h)
    fx, ff = np.zeros((nv, 6), bool), np.zeros((nv, 6))
    fx[:lat.n_nodes], ff[:lat.n_nodes] = fixed, f
    u_s = O.solve_dirichlet(K, fx.ravel(), np.zeros(fx.size), ff.ravel()).reshape(-1, 6)
    rel_u = np.abs(u_s[:lat.n_nodes] - u_c).max() / np.abs(u_c).max()
    V = O.submesh_vertices(t.node_xyz, t.beam_conn, h)
    first_new = np.r_[len(t.node_xyz), len(t.node_xyz) + np.cumsum(
        [O.gmsh_subdivisions(float(np.linalg.norm(t.node_xyz[b] - t.node_xyz[a])), h) - 1 for a, b in t.beam_conn])]
    assert first_new[-1] == nv
    ref, amp = np.empty(lat.n_beams), 0.0
    for b in range(lat.n_beams):
        A, Bn = lat.beam_conn[b]
        tb = lat.node_xyz[Bn] - lat.node_xyz[A]
        tb /= np.linalg.norm(tb)
        seg = next(s for s in np.flatnonzero(t.beam_parent == b) if A in t.beam_conn[s])      # the segment at end A
        ia, ib = t.beam_conn[seg]
        inner = list(range(first_new[seg], first_new[seg + 1]))
        ids = [ia] + inner + [ib]
        e = (ids[0], ids[1]) if ia == A else (ids[-2], ids[-1])                               # its sub-element at A
        Ke = O.sub_element_stiffness(V[e[0]], V[e[1]], O.section_constants(t.beam_radius[seg], Em, nu))
        g = Ke @ np.r_[u_s[e[0]], u_s[e[1]]]
        amp = max(amp, np.abs(Ke).sum(axis=1).max())
        ref[b] = -(g[:3] if ia == A else g[6:9]) @ tb             # what the rest of the strut transmits to this element
    rec = SH.records(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, Em, nu, pen_coef=L.penalization_coefficient)
    bound = (rel_u + 8 * EPS) * amp * np.abs(u_s).max()
    assert (ref < 0).any() and (ref > 0).any()
    for length in (0, 1):
        got = BH.strut_buckling(rec, lat.beam_conn, lat.beam_radius, pen.seg_len, u_c, Em, nu, length=length)
        here = ~np.isnan(got["n_axial"])
        assert np.array_equal(here, np.ones(lat.n_beams, bool) if length == 0 else pen.seg_len[:, 1] > 0)
        diff = np.abs(got["n_axial"][here] - ref[here]).max()
        print(f"\nlength {length}: displacement difference {rel_u:.2e}, axial force difference {diff:.2e} "
              f"of max|N| {np.abs(ref).max():.2e}, bound {bound:.2e} (absolute)")
        assert diff <= bound
        assert np.array_equal(got["util"][here] > 0, ref[here] < 0)


@pytest.mark.parametrize("shear", [0, 1])
@pytest.mark.parametrize("length", [0, 1])
def test_sign_properties(length, shear):
    """a strut buckles under u or under -u, never both; together they give |N| / N_cr; beta is homogeneous of degree one."""
    P = _Problem(_lattice((2, 2, 1), ("BCC", "Hybrid1"), (0.05, 0.04)), 4, mult=True)
    kw = dict(length=length, k_eff=0.7, shear=shear)
    a, b = P.struts(**kw), P.struts(-P.u, **kw)
    assert np.array_equal(np.isnan(a["util"]), np.isnan(b["util"]))
    here = ~np.isnan(a["util"])
    assert here.any() and (a["util"][here] > 0).any() and (b["util"][here] > 0).any()
    assert np.all(a["util"][here] * b["util"][here] == 0.0)
    assert np.array_equal(a["util"][here] + b["util"][here], np.abs(a["n_axial"][here]) / a["n_crit"][here])
    assert np.array_equal(a["n_axial"][here], -b["n_axial"][here]) and np.array_equal(a["n_crit"][here], b["n_crit"][here])
    alpha = 3.7
    c = P.struts(alpha * P.u, **kw)
    assert np.allclose(c["util"][here], alpha * a["util"][here], rtol=64 * EPS, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# derivatives of the restatement (the formulas the kernels implement) against central differences
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shear", [0, 1])
@pytest.mark.parametrize("length", [0, 1])
@pytest.mark.parametrize("p", [1, 2, 8])
def test_derivatives_against_central_differences(p, length, shear):
    """steps and bound of the stress pass's check (tests/test_stress_host.py): 1e-6 of max|u| in a random direction of u,
    1e-4 of the radii, 2e-3 of the difference quotient.  B_p has a kink where a strut's N changes sign: before every
    difference the test asserts that each strut's |N| is more than 100 times what the step changes it by."""
    P = _Problem(_lattice((2, 2, 1), ("BCC", "Hybrid1"), (0.05, 0.04)), 11, mult=True, vary_radii=True)
    kw = dict(length=length, k_eff=0.8, shear=shear)
    rng = np.random.default_rng(17)
    u, rad = P.u, P.rad
    val, bmax, du, dr = P.pnorm(p, **kw)
    assert val == P.pnorm(p, want_grad=False, **kw)[0] and 0 < bmax <= val
    N0 = P.struts(length=0)["n_axial"]
    h, hu = 1e-4, 1e-6
    for k in range(8):
        d = rng.standard_normal(u.shape) * np.abs(u).max()
        assert np.all(np.abs(N0) > 100 * np.abs(P.struts(u + hu * d, length=0)["n_axial"] - N0)), "a strut crosses the kink (u)"
        fd = (P.pnorm(p, u + hu * d, want_grad=False, **kw)[0] - P.pnorm(p, u - hu * d, want_grad=False, **kw)[0]) / (2 * hu)
        an = float((du * d).sum())
        assert abs(an - fd) <= 2e-3 * abs(fd), ("u", p, length, shear, k, an, fd)
        e = rng.standard_normal(P.nb) * rad
        assert np.all(np.abs(N0) > 100 * np.abs(P.struts(rad=rad + h * e, length=0)["n_axial"] - N0)), "a strut crosses the kink (r)"
        fd = (P.pnorm(p, rad=rad + h * e, want_grad=False, **kw)[0] - P.pnorm(p, rad=rad - h * e, want_grad=False, **kw)[0]) / (2 * h)
        an = float(dr @ e)
        assert abs(an - fd) <= 2e-3 * abs(fd), ("r", p, length, shear, k, an, fd)


def test_aggregate_bounds_and_degenerate_cases():
    P = _Problem(_lattice((2, 2, 1), ("BCC", "Hybrid1"), (0.05, 0.04)), 6)
    for length in (0, 1):
        util = P.struts(length=length)["util"]
        n = int((~np.isnan(util)).sum())
        prev = np.inf
        for p in (1, 2, 8, 64, 300):
            bp, bmax, du, dr = P.pnorm(p, length=length)
            assert bmax == np.nanmax(util) > 0
            assert bmax <= bp <= n ** (1.0 / p) * bmax * (1 + 1e-14) and bp <= prev * (1 + 1e-14)
            assert np.isfinite(du).all() and np.isfinite(dr).all()
            prev = bp
        big = P.pnorm(300, 1e150 * P.u, length=length)                  # beta^300 would overflow; the scaled sum does not
        assert np.isfinite(big[0]) and abs(big[0] - 1e150 * prev) <= 1e-12 * big[0]
        assert np.isfinite(big[2]).all() and np.isfinite(big[3]).all()
    with pytest.raises(ValueError):
        P.pnorm(0.5)
    # a uniform dilation stretches every strut: nothing is compressed
    dil = np.zeros((P.nn, 6))
    dil[:, :3] = 1e-3 * np.asarray(P.xyz)
    out = P.struts(dil, length=0)
    assert (out["n_axial"] > 0).all() and not out["util"].any()
    bp, bmax, du, dr = P.pnorm(8, dil, length=0)
    assert bp == 0.0 and bmax == 0.0 and not du.any() and not dr.any()
    assert P.pnorm(8, -dil, length=0)[0] > 0                            # and the contraction compresses all of them


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _library():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.load_library()


def test_c_abi_declarations_and_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pylattice_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    ctype = {"pl_handle": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}
    lib = _library()
    for name, n_args in (("pl_buckling", 8), ("pl_buckling_pnorm", 10)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args
        want = [C.c_void_p if "*" in a else ctype[a.replace("const", "").split()[0]] for a in args]
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == want, (name, args)
    assert re.search(r"#define\s+PL_ABI_VERSION\s+6u", text)           # additive: no ABI bump
    # the argument checks that need no device
    assert lib.pl_buckling(None, None, 1, 1.0, 0, None, None, None) == _capi.PL_ERR_ARG
    assert lib.pl_buckling_pnorm(None, None, 1, 1.0, 0, 8.0, None, None, None, None) == _capi.PL_ERR_ARG
