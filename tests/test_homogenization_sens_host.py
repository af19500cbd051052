"""The numpy / scipy restatement of the homogenised-stiffness sensitivities (pylatticedso_amd/homogenization_host.py; DESIGN.md
section 10e) against central differences of the whole host homogenisation, a closed form, the chain to the cell's radii and
an inverse design.  No device.

The identity under test: with the six total fields u_k of the periodic homogenisation, E_kl = u_k^T K u_l = scale_k
H_raw[k, l] (Hill-Mandel) and dE_kl/dr_b = u_k,e^T (dK_e/dr_b) u_l,e at fixed segment geometry - no adjoint solve.

Measured on the host code (bcc / hybrid1 / bcchybrid1 goldens, radii scaled by U(1, 1.4) from default_rng(11), four struts
each, errors relative to max|d . / dr_b| over the entries resp. to each constant's largest derivative over the struts):

    step        dH_raw vs differences      engineering constants vs differences
    1e-4 r      2.3e-9 / 8.5e-9 / 6.6e-9   8.0e-9 / 8.5e-9 / 5.7e-9
    1e-5 r      6.7e-11 / 8.8e-10 / 1.2e-9 1.7e-9 / 1.2e-9 / 2.1e-9

At 1e-4 r the error is the truncation of the differences (~ h^2); a ten times smaller step lowers it until the rounding of
the differences (~ 1e-16 / h times the conditioning of the dense solve) takes over near 1e-9.  Both stay two orders below
the tolerance of 1e-6 the tests hold at step 1e-4 r; the margin absorbs another BLAS.  The chain to the cell radii measured
1.1e-11, the inverse design 6 evaluations with a Jacobian of condition number 1.8."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from pylatticedso_amd import geometric_host as GH
from pylatticedso_amd import homogenization_host as HH
from pylatticedso_amd import lattice_arrays as LA
from pylatticedso_amd import stress_host as SH
from pylatticedso_amd.lattice_sim import LatticeSim

E, NU, KAPPA, PEN = 1013.0, 0.3, 0.9, 1.5
CELLS = ("bcc", "hybrid1", "bcchybrid1")
STEP, TOL = 1e-4, 1e-6


class Cell:
    """One golden cell with penalised segments and perturbed radii; ``solve(radius)`` is the whole host homogenisation."""

    def __init__(self, golden_dir, name):
        g = np.load(os.path.join(golden_dir, f"lattice_{name}_1x1x1_periodic.npz"))
        self.xyz, self.conn = np.asarray(g["base_node_xyz"], float), np.asarray(g["base_beam_conn"])
        pen = LA.penalize(SimpleNamespace(node_xyz=self.xyz, beam_conn=self.conn, cell_size_nominal=(1.0, 1.0, 1.0)),
                          np.asarray(g["base_beam_lzone"], float), mesh_size=0.05, backend="numpy")
        self.seg_len, self.seg_nsub = pen.seg_len, pen.seg_nsub
        assert (self.seg_len[:, [0, 2]] > 0).any()                       # joints are penalised
        self.lo, self.size = np.asarray(g["cell_coord"][0], float), np.ones(3)
        rng = np.random.default_rng(11)
        self.radius = np.asarray(g["base_beam_radius"], float) * rng.uniform(1.0, 1.4, len(self.conn))
        self.struts = rng.choice(len(self.conn), 4, replace=False)
        self.H, self.U, self.drec = self.solve(self.radius, want_drec=True)
        self.dH = HH.homogenized_sensitivity(self.drec, self.conn, self.U)

    def _args(self, radius):
        return self.xyz, self.conn, radius, self.seg_len, self.seg_nsub, E, NU, KAPPA, PEN

    def solve(self, radius, want_drec=False):
        H, U = HH.homogenize(SH.records(*self._args(radius)), self.conn, self.xyz, self.lo, self.size)
        return (H, U, SH.drecords_dr(*self._args(radius))) if want_drec else H

    def differences(self, fn, h=STEP):
        """central differences of fn(H_raw) to the radii of ``struts``, step h r_b: stacked on a last axis"""
        out = []
        for b in self.struts:
            step = np.zeros(len(self.radius))
            step[b] = h * self.radius[b]
            out.append((fn(self.solve(self.radius + step)) - fn(self.solve(self.radius - step))) / (2.0 * step[b]))
        return np.stack(out, axis=-1)


_cells = {}


def cell(golden_dir, name):
    if name not in _cells:
        _cells[name] = Cell(golden_dir, name)
    return _cells[name]


@pytest.mark.parametrize("name", CELLS)
def test_matrix_sensitivity_matches_central_differences(golden_dir, name):
    c = cell(golden_dir, name)
    H = c.H
    # the perturbed radii break the cubic symmetry: the raw matrix is unsymmetric and normal strains load the shear rows
    asym = np.linalg.norm(H - H.T) / np.linalg.norm(H)
    coupling = np.abs(H[:3, 3:]).max() / np.abs(H).max()
    print(name, "asymmetry", asym, "normal-shear coupling", coupling)
    assert asym > 1e-3 and coupling > 1e-4
    fd = c.differences(lambda M: M)
    for i, b in enumerate(c.struts):
        err = np.abs(c.dH[:, :, b] - fd[:, :, i]).max() / np.abs(c.dH[:, :, b]).max()
        print(name, "strut", b, "dH_raw vs differences", err)
        assert err < TOL


@pytest.mark.parametrize("name", CELLS)
def test_engineering_constants_sensitivity_matches_central_differences(golden_dir, name):
    c = cell(golden_dir, name)
    d = HH.engineering_constants_sensitivity(c.H, c.dH)                  # (9, B)
    assert d.shape == (9, len(c.conn))
    fd = c.differences(HH.engineering_constants)                         # (9, 4)
    scale = np.abs(d).max(axis=1)                                        # each constant's own derivative scale
    assert (scale > 0).all()
    err = np.abs(d[:, c.struts] - fd) / scale[:, None]
    print(name, "engineering constants vs differences", dict(zip(HH.CONSTANTS, err.max(axis=1))))
    assert err.max() < TOL
    # the constants themselves are those of the class: inverse of the UN-symmetrised matrix
    Hi = np.linalg.inv(c.H)
    v = HH.engineering_constants(c.H)
    assert np.isclose(v[0], 1 / Hi[0, 0]) and np.isclose(v[3], 1 / (2 * Hi[3, 3])) and np.isclose(v[6], -Hi[0, 1] / Hi[1, 1])


@pytest.mark.parametrize("name", CELLS)
def test_gram_is_symmetric_and_equals_the_pairing_and_hill_mandel_holds(golden_dir, name):
    c = cell(golden_dir, name)
    G = HH.sens_gram(c.drec, c.conn, c.U)
    assert G.shape == (6, 6, len(c.conn))
    assert np.abs(G - G.transpose(1, 0, 2)).max() < 1e-13 * np.abs(G).max()
    assert np.array_equal(HH.sens_gram(c.drec, c.conn, c.U[2:3])[0, 0], GH._pairing(c.drec, c.conn, c.U[2], c.U[2]))
    assert np.array_equal(HH.sens_gram(c.drec, c.conn, c.U.reshape(6, -1)), G)           # (k, 6 N) columns
    K = GH.elastic_matrix(SH.records(*c._args(c.radius)), c.conn, len(c.xyz))
    En = np.array([[c.U[k].ravel() @ (K @ c.U[l].ravel()) for l in range(6)] for k in range(6)])
    assert np.abs(En - HH.SCALE[:, None] * c.H).max() < 1e-12 * np.abs(c.H).max()
    assert np.allclose(c.dH, G / HH.SCALE[:, None, None], rtol=0, atol=0)
    with pytest.raises(ValueError):
        HH.homogenized_sensitivity(c.drec, c.conn, c.U[:5])


def test_simple_cubic_cell_closed_form():
    """12 edge struts of radius r, un-penalised: H[0, 0] = 4 E pi r^2 (tests/test_homogenization_oracle.py), so each of the
    four x-struts contributes 2 E pi r to dH[0, 0]/dr and every other strut nothing."""
    r = 0.04
    corners = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    conn = np.array([(a, b) for a in range(8) for b in range(a + 1, 8) if np.abs(corners[a] - corners[b]).sum() == 1.0])
    assert len(conn) == 12
    seg_len, seg_nsub = np.zeros((12, 3)), np.zeros((12, 3), np.int32)
    seg_len[:, 1], seg_nsub[:, 1] = 1.0, 20
    args = (corners, conn, np.full(12, r), seg_len, seg_nsub, E, NU, KAPPA, PEN)
    H, U = HH.homogenize(SH.records(*args), conn, corners, np.zeros(3), np.ones(3))
    assert np.isclose(H[0, 0], 4 * E * np.pi * r ** 2, rtol=1e-11)
    dH = HH.homogenized_sensitivity(SH.drecords_dr(*args), conn, U)
    along_x = np.abs(corners[conn[:, 1]] - corners[conn[:, 0]])[:, 0] == 1.0
    assert along_x.sum() == 4
    unit = 2 * E * np.pi * r
    assert np.abs(dH[0, 0, along_x] - unit).max() < 1e-10 * unit
    assert np.abs(dH[0, 0, ~along_x]).max() < 1e-10 * unit


def preset(radii):
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                         "radii": [float(r) for r in radii], "geom_types": ["BCC", "Cubic"]},
            "simulation_parameters": {"enable": False, "material": "VeroClear", "periodicity": True}}


def hybrid(radii, want_derivative=False):
    """(H_raw, dH_raw/d radii (6, 6, 2) or None) of the BCC + Cubic cell at the given radii, all on the host."""
    L = LatticeSim(preset(radii))
    lat, pen = L.lattice, L.penalized
    args = (lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, L.young_modulus, L.poisson_ratio,
            KAPPA, L.penalization_coefficient, L.beam_mult)
    H, U = HH.homogenize(SH.records(*args), lat.beam_conn, lat.node_xyz, lat.cell_coord[0], lat.cell_size[0])
    if not want_derivative:
        return H, None
    dH = HH.homogenized_sensitivity(SH.drecords_dr(*args), lat.beam_conn, U)
    assert set(np.unique(lat.beam_type)) == {0, 1}
    return H, HH.per_radius(dH, lat.beam_type, 2)


def test_chain_to_the_cell_radii_matches_differences_of_the_whole_homogenisation():
    """Joint penalisation off: the fixed-segment derivative is the exact one, and every strut of geometry g has the radius
    radii[g], so the sum over beam_type is dH/d radii[g].  Measured: 1.1e-11."""
    r0, h = np.array([0.05, 0.05]), 1e-6
    _, dH = hybrid(r0, want_derivative=True)
    assert dH.shape == (6, 6, 2)
    for g in range(2):
        e = np.zeros(2)
        e[g] = h
        fd = (hybrid(r0 + e)[0] - hybrid(r0 - e)[0]) / (2 * h)
        err = np.abs(dH[:, :, g] - fd).max() / np.abs(dH[:, :, g]).max()
        print("radius", g, "chain vs differences", err)
        assert err < 1e-7


def test_inverse_design_recovers_the_radii_on_the_host_path():
    """Gauss-Newton (scipy least_squares with the analytic Jacobian) on the 21 entries of the symmetrised matrix: from
    (0.05, 0.05) to the cell of radii (0.06, 0.04).  Measured: 6 evaluations, Jacobian condition number 1.8 (columns scaled by the target's norm)."""
    from scipy.optimize import least_squares
    want = np.array([0.06, 0.04])
    iu = np.triu_indices(6)
    sym = lambda M: 0.5 * (M + np.swapaxes(M, 0, 1))                       # noqa: E731
    target = sym(hybrid(want)[0])[iu]
    norm = np.linalg.norm(target)
    cache = {}

    def both(x):
        key = tuple(x)
        if key not in cache:
            H, dH = hybrid(x, want_derivative=True)
            cache[key] = (sym(H)[iu] - target) / norm, sym(dH)[iu] / norm
        return cache[key]

    res = least_squares(lambda x: both(x)[0], [0.05, 0.05], jac=lambda x: both(x)[1], xtol=1e-12, ftol=None, gtol=None)
    print("nfev", res.nfev, "cond(J)", np.linalg.cond(res.jac), "x", res.x)
    assert np.abs(res.x - want).max() < 1e-8 * want.min()
    assert res.nfev <= 12
