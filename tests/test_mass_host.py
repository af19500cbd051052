"""The numpy / scipy restatement of the consistent strut mass and the natural-frequency analysis (mass_host.py): the element
against the textbook blocks, its invariances and rigid-body inertia, the force formula against the sparse matrix, a pinned
column against the Timoshenko beam, the subspace iteration against the dense eigen-solution, and the radius sensitivities
against central differences.  No device."""
import numpy as np
import pytest
import scipy.linalg

from pylatticedso_amd import geometric_host as GH
from pylatticedso_amd import mass_host as MH
from pylatticedso_amd import stress_host as SH
from pylatticedso_amd.lattice_sim import LatticeSim

E, NU, KAPPA, PEN = 1013.0, 0.3, 0.9, 1.5
RHO = 1.3


# ---------------------------------------------------------------------------------------------------------------------
# 1. the element
# ---------------------------------------------------------------------------------------------------------------------
def _bending(c, L):
    return c * np.array([[156, 22 * L, 54, -13 * L], [22 * L, 4 * L * L, 13 * L, -3 * L * L],
                         [54, 13 * L, 156, -22 * L], [-13 * L, -3 * L * L, -22 * L, 4 * L * L]], float)


def _rotary(g, L):
    return g * np.array([[36, 3 * L, -36, 3 * L], [3 * L, 4 * L * L, -3 * L, -L * L],
                         [-36, -3 * L, 36, -3 * L], [3 * L, -L * L, -3 * L, 4 * L * L]], float)


@pytest.mark.parametrize("rotary", [False, True])
def test_element_of_a_strut_along_x_is_the_textbook_blocks(rotary):
    L, r, k = 0.7, 0.06, 2.0
    M = MH.element_matrix(np.array([L, 0.0, 0.0]), r, RHO, k, rotary)
    S, I = np.pi * r * r, 0.25 * np.pi * r ** 4
    m = k * RHO * S * L
    T = _bending(m / 420.0, L) + (_rotary(k * RHO * I / (30.0 * L), L) if rotary else 0.0)
    # plane x-y: deflection u_y, slope th_z;  plane x-z: deflection u_z, slope -th_y
    xy, xz = [1, 5, 7, 11], [2, 4, 8, 10]
    sign = np.array([1.0, -1.0, 1.0, -1.0])
    two = np.array([[2.0, 1.0], [1.0, 2.0]])
    scale = np.abs(M).max()
    assert np.abs(M[np.ix_(xy, xy)] - T).max() <= 4e-16 * scale
    assert np.abs(M[np.ix_(xz, xz)] - sign[:, None] * T * sign[None, :]).max() <= 4e-16 * scale
    assert np.abs(M[np.ix_([0, 6], [0, 6])] - m / 6.0 * two).max() <= 4e-16 * scale                  # axial
    assert np.abs(M[np.ix_([3, 9], [3, 9])] - k * RHO * 2.0 * I * L / 6.0 * two).max() <= 4e-16 * scale   # torsional
    rest = np.ones((12, 12), bool)
    for idx in (xy, xz, [0, 6], [3, 9]):
        rest[np.ix_(idx, idx)] = False
    assert not M[rest].any()


def test_element_is_symmetric_positive_definite_rotates_and_batches():
    rng = np.random.default_rng(5)
    d, r = rng.standard_normal(3), 0.11
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    T = np.kron(np.eye(4), R)
    for rotary in (False, True):
        M, Mr = MH.element_matrix(d, r, RHO, None, rotary), MH.element_matrix(R @ d, r, RHO, None, rotary)
        scale = np.abs(M).max()
        assert np.abs(Mr - T @ M @ T.T).max() <= 1e-14 * scale
        assert np.abs(M - M.T).max() <= 1e-15 * scale
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0
    ds, rs, ks = rng.standard_normal((4, 3)), 0.05 + 0.1 * rng.random(4), np.array([1.0, 2.0, 1.0, 3.0])
    batch = MH.element_matrix(ds, rs, RHO, ks, True)
    assert all(np.array_equal(batch[i], MH.element_matrix(ds[i], rs[i], RHO, ks[i], True)) for i in range(4))
    # the radius derivative against a central difference
    h = 1e-6
    fd = (MH.element_matrix(ds, rs + h, RHO, ks, True) - MH.element_matrix(ds, rs - h, RHO, ks, True)) / (2 * h)
    dM = MH.delement_matrix_dr(ds, rs, RHO, ks, True)
    assert np.abs(fd - dM).max() <= 1e-8 * np.abs(dM).max()


@pytest.mark.parametrize("rotary", [False, True])
def test_rigid_motions_carry_the_mass_and_the_moment_of_inertia(rotary):
    rng = np.random.default_rng(8)
    d, r, k = rng.standard_normal(3), 0.09, 2.0
    L = np.linalg.norm(d)
    m = k * RHO * np.pi * r * r * L
    M = MH.element_matrix(d, r, RHO, k, rotary)
    for axis in range(3):
        x = np.zeros(12)
        x[axis] = x[6 + axis] = 1.0
        assert abs(x @ M @ x - m) <= 1e-14 * m
    # rotation about end A with a unit rate w normal to the strut: u_B = w x d, th_A = th_B = w
    w = np.cross(d, rng.standard_normal(3))
    w /= np.linalg.norm(w)
    x = np.concatenate([np.zeros(3), w, np.cross(w, d), w])
    want = m * L * L / 3.0 + (m * r * r / 4.0 if rotary else 0.0)
    assert abs(x @ M @ x - want) <= 1e-13 * want
    # spin about the strut's own axis: the polar inertia m r^2 / 2
    t = d / L
    x = np.concatenate([np.zeros(3), t, np.zeros(3), t])
    assert abs(x @ M @ x - 0.5 * m * r * r) <= 1e-14 * m * r * r


# ---------------------------------------------------------------------------------------------------------------------
# 2. lattices A (graded, penalised BCC tower), B (uniform plain tower), C (graded plain Octet)
# ---------------------------------------------------------------------------------------------------------------------
def _preset(geom, cells, radius=0.05):
    return {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1},
                         "number_of_cells": {"x": cells[0], "y": cells[1], "z": cells[2]},
                         "radii": [radius], "geom_types": [geom]},
            "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
            "boundary_conditions": {
                "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                           "Value": [0, 0, 0, 0, 0, 0]}},
                "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["Z"], "Value": [-0.1]}}}}


class Case:
    """One test lattice: geometry, graded radii, one strut of multiplicity 2, a point mass on the top face."""

    def __init__(self, geom, cells, graded, penalised):
        L = LatticeSim(_preset(geom, cells))
        lat, pen = L.lattice, L.penalized
        self.xyz, self.conn = np.asarray(lat.node_xyz, float), np.asarray(lat.beam_conn)
        self.n, self.B = lat.n_nodes, lat.n_beams
        if penalised:
            self.sl, self.sn = pen.seg_len.copy(), pen.seg_nsub.copy()
        else:
            self.sl = np.zeros_like(pen.seg_len)
            self.sl[:, 1] = pen.seg_len.sum(axis=1)
            self.sn = np.zeros_like(pen.seg_nsub)
            self.sn[:, 1] = np.maximum(pen.seg_nsub.sum(axis=1), 1)
        mid = 0.5 * (self.xyz[self.conn[:, 0]] + self.xyz[self.conn[:, 1]])
        self.radius = np.full(self.B, 0.05)
        self.mult, self.node_mass = None, None
        if graded:       # a smooth function of the strut midpoint without any symmetry: simple eigenvalues
            self.radius = 0.05 * (1.0 + 0.25 * np.sin(1.3 * mid[:, 0] + 0.4) + 0.2 * np.cos(0.9 * mid[:, 1] - 0.3)
                                  + 0.08 * mid[:, 2])
            self.mult = np.ones(self.B)
            self.mult[3] = 2.0
            self.node_mass = np.where(self.xyz[:, 2] > self.xyz[:, 2].max() - 1e-9, 0.02, 0.0)
        self.fixed = np.asarray(L.fixed_DOF).reshape(self.n, 6) != 0

    def rec(self, radius=None):
        return SH.records(self.xyz, self.conn, self.radius if radius is None else radius, self.sl, self.sn, E, NU, KAPPA,
                          PEN, self.mult)

    def drec(self):
        return SH.drecords_dr(self.xyz, self.conn, self.radius, self.sl, self.sn, E, NU, KAPPA, PEN, self.mult)

    def K(self, radius=None):
        return GH.elastic_matrix(self.rec(radius), self.conn, self.n)

    def M(self, radius=None, rotary=True):
        return MH.mass_matrix(self.xyz, self.conn, self.radius if radius is None else radius, RHO, self.mult, rotary,
                              self.node_mass)


CASES = {"A": ("BCC", (2, 2, 3), True, True), "B": ("BCC", (2, 2, 3), False, False), "C": ("Octet", (2, 2, 2), True, False)}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = Case(*CASES[name])
    return _cache[name]


def test_lattice_sizes():
    assert (case("A").n, case("A").B) == (48, 96)
    assert (case("C").n, case("C").B) == (63, 240)


@pytest.mark.parametrize("name", ["A", "C"])
def test_mass_apply_equals_the_sparse_product(name):
    c = case(name)
    X = np.random.default_rng(2).standard_normal((3, c.n, 6))
    for rotary in (False, True):
        M = c.M(rotary=rotary)
        assert abs(M - M.T).max() <= 1e-15 * abs(M).max()
        ref = (M @ X.reshape(3, -1).T).T.reshape(3, c.n, 6)
        got = MH.mass_apply(c.xyz, c.conn, c.radius, RHO, X, c.mult, rotary, c.node_mass)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.array_equal(MH.mass_apply(c.xyz, c.conn, c.radius, RHO, X[1], c.mult, rotary, c.node_mass), got[1])
        Xm = np.where(c.fixed[None], 0.0, X)
        refm = np.where(c.fixed[None], 0.0, (M @ Xm.reshape(3, -1).T).T.reshape(3, c.n, 6))
        gotm = MH.mass_apply(c.xyz, c.conn, c.radius, RHO, X, c.mult, rotary, c.node_mass, fixed=c.fixed)
        assert np.abs(gotm - refm).max() <= 1e-13 * np.abs(refm).max()
    # a rigid translation of the whole lattice carries the total mass
    x = np.zeros((c.n, 6))
    x[:, 0] = 1.0
    d = c.xyz[c.conn[:, 1]] - c.xyz[c.conn[:, 0]]
    total = (c.mult * RHO * np.pi * c.radius ** 2 * np.linalg.norm(d, axis=1)).sum() + c.node_mass.sum()
    assert abs(x.reshape(-1) @ (c.M() @ x.reshape(-1)) - total) <= 1e-13 * total
    with pytest.raises(ValueError):
        MH.mass_matrix(c.xyz, c.conn, c.radius, RHO, node_mass=-np.ones(c.n))


def test_pinned_column_against_the_timoshenko_beam():
    """16 collinear plain struts, pinned - roller: omega_1^2 within 1 % of the Timoshenko value
    omega_EB^2 / (1 + (pi / L)^2 (I / S) (1 + E / (kappa G))).  The deviation is K's one-sub-element discretisation."""
    ns, radius = 16, 0.05
    n = ns + 1
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.arange(n)
    conn = np.column_stack([np.arange(ns), np.arange(1, n)])
    sl = np.zeros((ns, 3))
    sl[:, 1] = 1.0
    sn = np.zeros((ns, 3), int)
    sn[:, 1] = 1
    fixed = np.zeros((n, 6), bool)
    fixed[0, [0, 1, 2, 3]] = True
    fixed[-1, [1, 2]] = True
    r = np.full(ns, radius)
    K = GH.elastic_matrix(SH.records(xyz, conn, r, sl, sn, E, NU, KAPPA), conn, n)
    M = MH.mass_matrix(xyz, conn, r, RHO)
    S, I, G = np.pi * radius ** 2, 0.25 * np.pi * radius ** 4, E / (2.0 * (1.0 + NU))
    kk = (np.pi / ns) ** 2
    timo = kk * kk * E * I / (RHO * S) / (1.0 + kk * (I / S) * (1.0 + E / (KAPPA * G)))
    got = MH.vibration_modes_dense(K, M, fixed, 2)["omega2"]
    print("omega_1^2 / Timoshenko:", got[0] / timo)
    assert abs(got[0] / timo - 1.0) <= 0.01
    assert abs(got[1] / got[0] - 1.0) <= 1e-9                  # the same mode in the other bending plane


@pytest.mark.parametrize("name,n_modes,n_sub", [("A", 4, 8), ("A", 4, 12), ("B", 5, 12), ("C", 4, 8)])
def test_subspace_iteration_agrees_with_eigh(name, n_modes, n_sub):
    c = case(name)
    K, M = c.K(), c.M()
    ref = MH.vibration_modes_dense(K, M, c.fixed, n_modes)
    got = MH.vibration_modes_subspace(K, M, c.fixed, n_modes, n_sub, tol=1e-10)
    print(name, n_sub, "outer steps", got["outer_iterations"], "omega2", ref["omega2"])
    assert got["converged"] and got["n_found"] == ref["n_found"] == n_modes
    assert np.abs(got["omega2"] / ref["omega2"] - 1.0).max() <= 1e-6
    assert got["residual"].max() <= 1e-4 and ref["residual"].max() <= 1e-8
    for out in (got, ref):                                       # M-orthonormal, largest component positive
        V = out["modes"].reshape(n_modes, -1)
        assert np.abs(V @ (M @ V.T) - np.eye(n_modes)).max() <= 1e-8
        assert all(v[np.argmax(np.abs(v))] > 0 for v in V)


def _fd_rows(c, n_modes, h=1e-6):
    """central differences of the dense omega^2 to every radius.  One radius changes one element: the dense K and M of the
    free dofs are formed once and the element's change is added to them."""
    free = GH._free(c.fixed, 6 * c.n)
    pos = np.full(6 * c.n, -1)
    pos[free] = np.arange(len(free))
    K0, M0 = c.K()[free][:, free].toarray(), c.M()[free][:, free].toarray()
    pair = np.array([[0, 1]])

    def element(b, r):
        mult = None if c.mult is None else c.mult[b:b + 1]
        rec = SH.records(c.xyz[c.conn[b]], pair, np.array([r]), c.sl[b:b + 1], c.sn[b:b + 1], E, NU, KAPPA, PEN, mult)
        Me = MH.element_matrix(c.xyz[c.conn[b, 1]] - c.xyz[c.conn[b, 0]], r, RHO, None if mult is None else mult[0], True)
        return GH.elastic_matrix(rec, pair, 2).toarray(), Me

    rows = np.zeros((n_modes, c.B))
    for b in range(c.B):
        dofs = pos[np.concatenate([6 * c.conn[b, 0] + np.arange(6), 6 * c.conn[b, 1] + np.arange(6)])]
        keep = dofs >= 0
        at = np.ix_(dofs[keep], dofs[keep])
        Ke0, Me0 = element(b, c.radius[b])
        w = []
        for s in (+1.0, -1.0):
            Ke, Me = element(b, c.radius[b] + s * h)
            K, M = K0.copy(), M0.copy()
            K[at] += (Ke - Ke0)[np.ix_(keep, keep)]
            M[at] += (Me - Me0)[np.ix_(keep, keep)]
            w.append(scipy.linalg.eigh(K, M, eigvals_only=True, subset_by_index=[0, n_modes - 1]))
        rows[:, b] = (w[0] - w[1]) / (2.0 * h)
    return rows


@pytest.mark.parametrize("name", ["A", "C"])
def test_sensitivity_rows_agree_with_central_differences(name):
    c = case(name)
    n_modes = 4
    ref = MH.vibration_modes_dense(c.K(), c.M(), c.fixed, n_modes)
    rows = MH.vibration_sensitivity(c.xyz, c.conn, c.radius, RHO, c.drec(), c.fixed, ref["omega2"], ref["modes"], c.mult,
                                    True, c.node_mass)
    fd = _fd_rows(c, n_modes)
    err = np.abs(rows - fd).max(axis=1) / np.abs(fd).max(axis=1)
    print(name, "rows against central differences:", err)
    assert err.max() <= 1e-5
    # a scaled mode keeps its row; a NaN omega^2 gives a NaN row
    om2 = ref["omega2"].copy()
    om2[2] = np.nan
    modes = ref["modes"].copy()
    modes[1] *= 3.0
    again = MH.vibration_sensitivity(c.xyz, c.conn, c.radius, RHO, c.drec(), c.fixed, om2, modes, c.mult, True, c.node_mass)
    assert np.isnan(again[2]).all()
    assert np.abs(again[[0, 1, 3]] - rows[[0, 1, 3]]).max() <= 1e-12 * np.abs(rows).max()


def test_rows_of_a_double_frequency_miss_one_by_one_and_agree_in_their_sum():
    c = case("B")
    n_modes = 3                                                   # the double first frequency and the simple third
    ref = MH.vibration_modes_dense(c.K(), c.M(), c.fixed, n_modes)
    om2 = ref["omega2"]
    print("B omega2", MH.vibration_modes_dense(c.K(), c.M(), c.fixed, 5)["omega2"])
    assert abs(om2[1] / om2[0] - 1.0) <= 1e-9 and om2[2] / om2[1] > 1.5
    rows = MH.vibration_sensitivity(c.xyz, c.conn, c.radius, RHO, c.drec(), c.fixed, om2, ref["modes"])
    fd = _fd_rows(c, n_modes)
    scale = np.abs(fd).max(axis=1)
    assert np.abs(rows[0] - fd[0]).max() > 1e-3 * scale[0] and np.abs(rows[1] - fd[1]).max() > 1e-3 * scale[1]
    assert np.abs(rows[0] + rows[1] - fd[0] - fd[1]).max() <= 1e-5 * np.abs(fd[0] + fd[1]).max()
    assert np.abs(rows[2] - fd[2]).max() <= 1e-5 * scale[2]
    # the aggregate over whole clusters is differentiable: its gradient against differences of the aggregate itself
    J, dJ = MH.frequency_aggregate(om2, 8.0)
    g = dJ @ rows
    dr = np.random.default_rng(3).standard_normal(c.B) * 1e-3
    h = 1e-4
    Jp = MH.frequency_aggregate(MH.vibration_modes_dense(c.K(c.radius + h * dr), c.M(c.radius + h * dr), c.fixed, 3)["omega2"], 8.0)[0]
    Jm = MH.frequency_aggregate(MH.vibration_modes_dense(c.K(c.radius - h * dr), c.M(c.radius - h * dr), c.fixed, 3)["omega2"], 8.0)[0]
    assert abs((Jp - Jm) / (2 * h) - g @ dr) <= 1e-5 * np.abs(g * dr).sum()
