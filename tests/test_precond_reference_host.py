"""The host restatement of the preconditioners (oracle/precond_oracle.py) has to be worth comparing against before
tests/test_gpu_precond.py holds the device to it: M^-1 symmetric, positive semi-definite and zero on fixed dofs, every
level exact on its own span, independent of the modes' reference points, the PCG under it converging to the oracle's
direct solve (node elimination included) - and SENSITIVE: the iterates must move, under every planted defect, by at
least ten times what the GPU test tolerates.  No GPU; the partition is the library's own, recorded in
tests/golden/precond_partition.npz (the GPU test asserts that the library still cuts it)."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import precond_cases as C, precond_oracle as P
from oracle import timoshenko_oracle as O
from pylatticedso_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, b) for n in C.LATTICES for b in C.BOUNDARY_SETS]


@functools.lru_cache(maxsize=None)
def _lattice(name):
    return C.Lattice(name)


@functools.lru_cache(maxsize=None)
def _setup(name, bset, modes, precond=3):
    lat = _lattice(name)
    part = C.recorded_partition(name, modes[1])
    fixed, ubar, f, info = C.boundary_set(bset, lat, part)
    return lat, part, fixed, ubar, f, info, P.Levels(lat.K, fixed, lat.xyz, part, precond, *modes)


def test_partition_hook_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "pylattice_hip.h")).read()
    assert re.search(r"int pl_debug_partition\(pl_handle h, int32_t \*tile_of_node, int32_t \*agg_of_node, "
                     r"int32_t \*local_agg_of_node,\s+uint8_t \*eliminated\);", text)
    assert re.search(r"#define\s+PL_ABI_VERSION\s+6u", text)           # additive: no ABI bump
    assert "pl_debug_partition" in _capi.EXPORTS and hasattr(_capi.HipLattice, "partition")


@pytest.mark.parametrize("name", C.LATTICES)
def test_recorded_partitions_cannot_go_vacuous(name):
    lat = _lattice(name)
    for cm in (6, 12):
        part = C.recorded_partition(name, cm)
        assert part["tile"].shape == part["agg"].shape == (lat.n_nodes,)
        assert len(np.unique(part["tile"])) >= 4 and len(np.unique(part["agg"])) >= 2
        for t in np.unique(part["tile"]):
            assert len(np.unique(part["agg"][part["tile"] == t])) == 1
    # the boundary sets are what they claim to be
    part = C.recorded_partition(name, 6)
    fixed, _, _, info = C.boundary_set("b", lat, part)
    partial = fixed.any(axis=1) & ~fixed.all(axis=1)
    assert partial.sum() >= 2
    fixed, _, _, info = C.boundary_set("c", lat, part)
    i = info["inside"]
    nb = np.r_[lat.conn[lat.conn[:, 0] == i, 1], lat.conn[lat.conn[:, 1] == i, 0]]
    assert fixed[i].all() and (part["tile"][nb] == part["tile"][i]).all() and not fixed[nb].any()
    assert len(P.fix_list_struts(lat.conn, fixed, part["agg"])) > 0
    fixed, _, _, info = C.boundary_set("d", lat, part)
    nodes = np.flatnonzero(part["tile"] == info["tile"])
    assert (~fixed[nodes].all(axis=1)).sum() == 1 and not fixed[info["free_node"]].any()


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("name,bset", CASES)
def test_reference_preconditioner_is_spsd_zero_on_fixed_dofs_and_exact_on_its_spans(name, bset, modes):
    lat, part, fixed, ubar, f, info, L = _setup(name, bset, modes)
    fx = fixed.ravel() != 0
    scale = np.abs(L.M).max()
    assert np.abs(L.M - L.M.T).max() == 0.0
    assert np.abs(L.M[fx]).max() == 0.0 and np.abs(L.M[:, fx]).max() == 0.0
    assert np.linalg.eigvalsh(L.M).min() > -1e-12 * scale
    # positive DEFINITE on the free dofs (a preconditioner CG may use)
    free = np.flatnonzero(~fx)
    assert np.linalg.eigvalsh(L.M[np.ix_(free, free)]).min() > 0.0
    # each level reproduces its own span: Z (Z^T A Z)^-1 Z^T A Z c = Z c
    c = np.random.default_rng(1).standard_normal(L.Z.shape[1])
    v = L.Z @ c
    assert P.rel(L.terms["dense"] @ (L.A @ v), v) < 1e-9
    for t, (Zt, Binv, kept) in L.tile_factors.items():
        v = Zt[:, kept] @ np.random.default_rng(int(t)).standard_normal(len(kept))
        assert P.rel(Zt @ (Binv @ (Zt.T @ (L.A @ v))), v) < 1e-9
    if bset == "d":      # one free node under 6 / 12 tile modes: the rigid modes span its six dofs, the strains are dropped
        assert L.kept[info["tile"]] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("name,bset", CASES)
def test_reference_does_not_depend_on_the_reference_points_of_the_modes(name, bset, modes):
    """The library's reference points (centres of boxes of bricks) are not part of the partition hook; they need not be:
    moving every reference point leaves the iterates where they are, rank-deficient tile included."""
    lat, part, fixed, ubar, f, info, L = _setup(name, bset, modes)
    L2 = P.Levels(lat.K, fixed, lat.xyz, part, 3, *modes, centre_shift=[0.37, -0.21, 0.11])
    a = P.solve_iterates(lat.K, fixed, ubar, f, L.M, 3)
    b = P.solve_iterates(lat.K, fixed, ubar, f, L2.M, 3)
    assert max(P.rel(x, y) for x, y in zip(b, a)) < 1e-11


def test_block_inverse_of_a_rank_deficient_block():
    rng = np.random.default_rng(0)
    for n in (6, 12):
        Q = rng.standard_normal((n, 4))
        B = Q @ Q.T                                   # rank 4
        inv, kept = P.greedy_block_inverse(B, n)
        assert kept == [0, 1, 2, 3]
        assert np.abs(inv - inv.T).max() == 0.0 and np.linalg.eigvalsh(inv).min() > -1e-12 * np.abs(inv).max()
        assert np.allclose(inv[:4, :4] @ B[:4, :4], np.eye(4), atol=1e-9) and not inv[4:].any() and not inv[:, 4:].any()
        inv0, kept0 = P.greedy_block_inverse(np.zeros((n, n)), n)
        assert kept0 == [] and not inv0.any()
        full = B + np.eye(n)
        inv1, kept1 = P.greedy_block_inverse(full, n)
        assert kept1 == list(range(n)) and np.allclose(inv1, np.linalg.inv(full))


@pytest.mark.parametrize("name", C.LATTICES)
def test_reference_pcg_converges_to_the_direct_solve_with_and_without_node_elimination(name):
    lat, part, fixed, ubar, f, info, L = _setup(name, "b", (12, 6))
    uref = O.solve_dirichlet(O.assemble_condensed(lat.xyz, lat.conn, lat.scalars), fixed != 0,
                             np.where(fixed != 0, ubar, 0.0), f).reshape(-1, 6)
    # an independent set without Dirichlet dofs, greedily (the library chooses its own; any such set must do)
    taken = np.zeros(lat.n_nodes, bool)
    blocked = fixed.any(axis=1).copy()
    nbr = [[] for _ in range(lat.n_nodes)]
    for ia, ib in lat.conn:
        nbr[ia].append(ib)
        nbr[ib].append(ia)
    for i in range(lat.n_nodes):
        if not blocked[i]:
            taken[i] = True
            blocked[nbr[i]] = True
    assert taken.sum() > lat.n_nodes // 8
    for elim in (None, taken):
        its = P.solve_iterates(lat.K, fixed, ubar, f, L.M, 400, elim)
        assert P.rel(its[-1], uref) < 1e-9
        assert P.rel(its[2], uref) > 1e-3          # ... and the early iterates are not the solution yet
    M5 = np.zeros_like(L.A)
    free = np.flatnonzero(L.free)
    M5[np.ix_(free, free)] = np.linalg.inv(L.A[np.ix_(free, free)])
    assert P.rel(P.solve_iterates(lat.K, fixed, ubar, f, M5, 1)[0], uref) < 1e-10      # precond = 5


@functools.lru_cache(maxsize=None)
def defect_distances(name, bset, modes):
    """{defect: relative move of (u_1, u_2, u_3)}.  Every mode of the aggregate and of the tile that hold the interior load is
    dropped in turn and the SMALLEST move per iterate counts (a strain mode of a small tile matters least); the rollers
    unmasked (boundary set b, the only one with rollers); the in-aggregate struts at Dirichlet dofs left out of the dense
    operator."""
    lat, part, fixed, ubar, f, info, L = _setup(name, bset, modes)
    base = P.solve_iterates(lat.K, fixed, ubar, f, L.M, 3)

    def moved(defect, **kw):
        M = P.Levels(lat.K, fixed, lat.xyz, part, 3, *modes, defect=defect, **kw).M
        return np.array([P.rel(x, y) for x, y in zip(P.solve_iterates(lat.K, fixed, ubar, f, M, 3), base)])

    a, t = int(part["agg"][info["inner"]]), int(part["tile"][info["inner"]])
    out = {"agg_mode": np.min([moved(("agg_mode", a, m)) for m in range(modes[1])], axis=0),
           "tile_mode": np.min([moved(("tile_mode", t, m)) for m in range(modes[0])], axis=0)}
    if bset == "b":
        out["roller_unmasked"] = moved(("roller_unmasked",))
    struts = P.fix_list_struts(lat.conn, fixed, part["agg"])
    out["fix_list"] = moved(("fix_list",), K_fix_list=P.strut_matrix(lat.xyz, lat.conn, lat.scalars, struts))
    return out


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("name,bset", CASES)
def test_sensitivity_floor(name, bset, modes):
    """Per iterate k = 1, 2, 3 (rounding accumulates with k, and so does what a defect does): every planted defect moves u_k
    by at least FLOOR_FACTOR times the bound the GPU test puts on u_k, for every group of forms that runs this input
    (oracle.precond_cases.GROUP_CASES; the Jacobi group has no level to get wrong and the smallest bounds)."""
    d = defect_distances(name, bset, modes)
    floor = np.min(list(d.values()), axis=0)
    print(f"PRECOND_FLOOR lattice={name} set={bset} modes={modes} floor={floor} "
          + " ".join(f"{k}={np.array2string(v, precision=2)}" for k, v in d.items()))
    for group, cases in C.GROUP_CASES.items():
        if (name, bset) in cases:
            assert (floor >= P.FLOOR_FACTOR * np.array(P.GPU_TOL[group])).all(), (group, floor, P.GPU_TOL[group])
    assert (np.array(P.GPU_TOL["jacobi"]) <= np.array(P.GPU_TOL["fp64"])).all()
