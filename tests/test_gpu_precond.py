"""The PCG preconditioner levels against a dense fp64 host restatement (oracle/precond_oracle.py), iterate by iterate.

CG converges to the right displacements under ANY symmetric positive definite preconditioner, so the solve-level tests of
tests/test_gpu_parity.py cannot see a wrong M^-1.  Here every solver form is stopped after k = 1, 2, 3 iterations
(pl_solve(max_iter = k) still writes the solution) from x_0 = 0 on a fresh handle, and u_k is compared with the reference
PCG under the restated M^-1: x_1 = alpha_0 M^-1 b reads the preconditioner itself, x_2 and x_3 also the residual update,
the restriction, the dense solve, the tile solves, beta and the new direction of the form under test.

Inputs: oracle/precond_cases.py (three lattices, tile_nodes = 32 or 16, boundary sets a - d built from the solver's own partition,
HipLattice.partition()).  coarse_storage = 32 throughout (bfloat16 rounding cannot be restated).

Tolerances (oracle.precond_oracle.GPU_TOL, relative L2 of u_1, u_2, u_3): ten times the largest deviation MEASURED on an
MI355X per group of forms, to allow for the order of the atomic sums, per iterate (rounding accumulates with k, and so does
the effect of a defect); tests/test_precond_reference_host.py holds each to a tenth of the sensitivity floor of the same
iterate - the smallest move of u_k under a planted defect of the reference: 1.0e-5, 3.7e-5, 6.3e-5 over all inputs.
    group    forms                                                   measured u_1, u_2, u_3        bound
    fp64     precond 2 / 3 in the ordinary, short, persistent and
             single-reduction forms, node elimination, loopback      4.1e-8   3.9e-8   1.4e-7      4.2e-7  3.9e-7  1.5e-6
             (DDM precond 4: 3.2e-9; precond 5 and DDM 2 / 3: < 2e-12)
    fp32     precision 1 and 2 (fp32-stored vectors)                 5.1e-8   8.0e-8   8.7e-8      5.2e-7  8.1e-7  8.8e-7
    jacobi   precond 1                                               3.8e-15  4.2e-15  4.7e-15     3.9e-14 4.3e-14 4.7e-14
What the fp64 group deviates by is the fp32 copy of D^-1 and the fp32 inverse factor / explicit inverse of the dense level.
Not bounded: precision = 1 WITH node elimination (1.7e-6 ... 4.0e-6 measured, see test_fp32_stored_vectors).
Every test prints its figures (pytest -s) before it asserts."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import precond_cases as C, precond_oracle as P      # noqa: E402
from oracle import timoshenko_oracle as O                       # noqa: E402

KS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _lattice(name):
    return C.Lattice(name)


@functools.lru_cache(maxsize=None)
def _case(name, cm, bset):
    return C.boundary_set(bset, _lattice(name), C.recorded_partition(name, cm))


@functools.lru_cache(maxsize=None)
def _levels(name, bset, precond, tm, cm):
    lat = _lattice(name)
    fixed = _case(name, cm, bset)[0]
    return P.Levels(lat.K, fixed, lat.xyz, C.recorded_partition(name, cm), precond, tm, cm)


def _opts(precond, tm, cm, **kw):
    o = dict(precond=precond, coarse_max_dofs=C.COARSE_MAX_DOFS[cm], tile_modes=tm,
             coarse_modes=cm, coarse_storage=32, condense=-1, short_iteration=-1, warm_start=0)
    o.update(kw)
    return o


def _device_iterates(name, cm, bset, opts, ks=KS):
    """[(u_k, stats)] for k in ks, each from a fresh handle, and the handle's partition."""
    lat = _lattice(name)
    if opts.get("precond", 1) in (2, 3):
        opts = dict(opts, tile_nodes=C.TILE_NODES[name])
    fixed, ubar, f, _ = _case(name, cm, bset)
    out, part = [], None
    for k in ks:
        with lat.device(**opts) as dev:
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            u, st = dev.solve(rtol=1e-30, max_iter=k, raise_on_noconv=False)
            part = dev.partition()
        out.append((u, st))
    return out, part


def _check_partition(name, cm, part, min_tiles=4, min_aggs=2):
    rec = C.recorded_partition(name, cm)
    assert np.array_equal(part["tile"], rec["tile"]) and np.array_equal(part["agg"], rec["agg"]), \
        "the library cuts another partition than tests/golden/precond_partition.npz records"
    assert len(np.unique(part["tile"])) >= min_tiles and len(np.unique(part["agg"])) >= min_aggs


def _compare(tag, group, name, bset, precond, tm, cm, opts, expect=None, ks=KS):
    """Run the device form, check what ran, compare u_k with the reference; returns the deviations."""
    lat = _lattice(name)
    fixed, ubar, f, _ = _case(name, cm, bset)
    runs, part = _device_iterates(name, cm, bset, opts, ks)
    if precond >= 2:
        _check_partition(name, cm, part)
    M = _levels(name, bset, precond, tm, cm).M if precond >= 2 else np.diag(_levels(name, bset, 1, 6, cm).Dinv)
    elim = part["eliminated"] if opts.get("condense", -1) > 0 else None
    ref = P.solve_iterates(lat.K, fixed, ubar, f, M, max(ks), elim)
    devs = []
    for k, (u, st) in zip(ks, runs):
        assert st["iterations"] == k, (tag, k, st["iterations"])
        assert int(st["precond_used"]) == precond, (tag, st["precond_used"])
        for key, val in (expect or {}).items():
            if key == "condensed":
                assert (st["condensed_nodes"] > 0) == val and (elim is not None and elim.sum() == st["condensed_nodes"]
                                                              if val else True), (tag, st["condensed_nodes"])
            else:
                assert int(st[key]) == val, (tag, key, st[key])
        devs.append(P.rel(u, ref[k - 1]))
    print(f"PRECOND_DEV group={group} form={tag} lattice={name} set={bset} modes=({tm},{cm}) precond={precond} "
          f"dev={' '.join(f'{d:.3e}' for d in devs)}")
    assert all(d < P.GPU_TOL[group][k - 1] for k, d in zip(ks, devs)), (tag, devs)
    return devs


@pytest.mark.parametrize("cm", [6, 12])
@pytest.mark.parametrize("name", C.LATTICES)
def test_partition_hook_reports_the_recorded_partition(name, cm):
    """pl_debug_partition: tiles and aggregates as recorded for the host test, every node in exactly one of each, a tile
    inside one aggregate; the eliminated set is independent, free of Dirichlet dofs and the size pl_solve reports."""
    lat = _lattice(name)
    fixed, ubar, f, _ = _case(name, cm, "b")
    tm = 12 if cm == 12 else 6
    with lat.device(**_opts(3, tm, cm, condense=1, tile_nodes=C.TILE_NODES[name])) as dev:
        dev.set_bc(fixed, ubar, f)
        dev.assemble()
        part = dev.partition()
        _, st = dev.solve(rtol=1e-8)
    _check_partition(name, cm, part)
    assert part["tile"].min() >= 0 and part["agg"].min() >= 0 and (part["local_agg"] == -1).all()
    for t in np.unique(part["tile"]):
        assert len(np.unique(part["agg"][part["tile"] == t])) == 1
    e = part["eliminated"]
    assert e.sum() == st["condensed_nodes"] > 0
    assert not (fixed[e] != 0).any() and not (e[lat.conn[:, 0]] & e[lat.conn[:, 1]]).any()
    with lat.device(precond=1) as dev:
        part1 = dev.partition()
    assert part1["tile"].min() >= 0 and (part1["agg"] == -1).all() and not part1["eliminated"].any()


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("bset", C.BOUNDARY_SETS)
@pytest.mark.parametrize("name", C.LATTICES)
def test_ordinary_form_three_levels(name, bset, modes):
    """precond = 3, the ordinary five-launch iteration, on every lattice, boundary set and mode pair."""
    tm, cm = modes
    _compare("ordinary", "fp64", name, bset, 3, tm, cm, _opts(3, tm, cm),
             expect={"short_iteration_used": 0, "cg_form_used": 0, "condensed": False})


@pytest.mark.parametrize("bset", ["b", "c"])
@pytest.mark.parametrize("name", C.LATTICES)
def test_two_level_and_jacobi(name, bset):
    """precond = 2 (Jacobi + dense level, no tile level) and precond = 1 (Jacobi alone)."""
    _compare("two-level", "fp64", name, bset, 2, 6, 6, _opts(2, 6, 6))
    _compare("jacobi", "jacobi", name, bset, 1, 6, 6, dict(precond=1))


FORMS = {
    "short": (dict(short_iteration=1, palette=1), {"short_iteration_used": 1, "condensed": False}),
    "persistent": (dict(short_iteration=2, palette=1), {"short_iteration_used": 2, "condensed": False}),
    "single-reduction": (dict(cg_form=1), {"cg_form_used": 1, "condensed": False}),
    "condensed": (dict(condense=1), {"short_iteration_used": 0, "condensed": True}),
    "condensed-short": (dict(condense=1, short_iteration=1, palette=1), {"short_iteration_used": 1, "condensed": True}),
}


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("bset", ["b", "c", "d"])
@pytest.mark.parametrize("form", list(FORMS))
def test_fp64_forms(form, bset, modes):
    """The short (three-launch), persistent and single-reduction forms and node elimination, fp64, precond = 3: the same
    iterates as the reference - hence as the ordinary form - at k = 1, 2, 3."""
    tm, cm = modes
    extra, expect = FORMS[form]
    _compare(form, "fp64", "bcc_6x3x3", bset, 3, tm, cm, _opts(3, tm, cm, **extra), expect=expect)


@pytest.mark.parametrize("form", ["short", "single-reduction", "condensed"])
@pytest.mark.parametrize("name", ["octet_4x3x3", "bcchybrid1hybrid4_3x2x1_size"])
def test_fp64_forms_on_the_other_lattices(name, form):
    extra, expect = FORMS[form]
    for bset in ("b", "c"):
        _compare(form, "fp64", name, bset, 3, 12, 6, _opts(3, 12, 6, **extra), expect=expect)


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("bset", ["b", "c"])
@pytest.mark.parametrize("precision", [1, 2])
def test_fp32_stored_vectors(precision, bset, modes):
    """opts.precision = 1 (all PCG vectors in fp32) and 2 (p and K*p in fp32).  (Not with node elimination: precision = 1
    then runs the elimination's prologue and back-substitution on fp32-stored vectors as well, and u_k of an inner solve
    that the fp64 refinement has not yet visited is 2e-6 ... 4e-6 off - measured - which no bound under the sensitivity
    floor admits.)"""
    tm, cm = modes
    assert ("bcc_6x3x3", bset) in C.GROUP_CASES["fp32"]
    _compare(f"precision{precision}", "fp32", "bcc_6x3x3", bset, 3, tm, cm, _opts(3, tm, cm, precision=precision),
             expect={"precision_used": precision, "condensed": False})


@pytest.mark.parametrize("bset", ["b", "c"])
@pytest.mark.parametrize("name", C.LATTICES)
def test_dense_factor_reaches_the_direct_solution_in_one_iteration(name, bset):
    """precond = 5: M^-1 = (P K P)^-1, so x_1 is the solution of the oracle's direct solve."""
    lat = _lattice(name)
    fixed, ubar, f, _ = _case(name, 6, bset)
    uref = O.solve_dirichlet(O.assemble_condensed(lat.xyz, lat.conn, lat.scalars), fixed != 0,
                             np.where(fixed != 0, ubar, 0.0), f).reshape(-1, 6)
    (u, st), = _device_iterates(name, 6, bset, dict(precond=5), ks=(1,))[0]
    dev = P.rel(u, uref)
    print(f"PRECOND_DEV group=fp64 form=dense-factor lattice={name} set={bset} precond=5 dev={dev:.3e}")
    assert st["iterations"] == 1 and int(st["precond_used"]) == 5
    assert dev < P.GPU_TOL["fp64"][0]


@pytest.mark.parametrize("modes", C.MODE_PAIRS)
@pytest.mark.parametrize("form", ["ordinary", "short", "single-reduction", "precision1"])
def test_preconditioner_is_symmetric_on_the_device(form, modes):
    """b2 . M^-1 b1 = b1 . M^-1 b2 without any reference.  x_1(b) = alpha(b) M^-1 b, and alpha cannot be read from x_1 alone
    (x_1 minimises the energy along its own direction whatever its length), so a third solve with b1 + b2 supplies it:
    x_1(b1 + b2) = c1 x_1(b1) + c2 x_1(b2) with c_i = alpha_12 / alpha_i by linearity of M^-1, hence
    (b2 . x_1(b1)) c1 = (b1 . x_1(b2)) c2 for a symmetric M^-1.  The fit also checks the linearity."""
    tm, cm = modes
    name, bset = "bcc_6x3x3", "b"
    lat = _lattice(name)
    fixed, _, f, info = _case(name, cm, bset)
    extra = {"ordinary": {}, "precision1": dict(precision=1)}.get(form) or FORMS.get(form, ({},))[0]
    b1 = f.copy()
    b2 = np.zeros_like(f)
    rng = np.random.default_rng(3)
    b2[rng.choice(lat.n_nodes, 12, replace=False)] = 0.05 * rng.standard_normal((12, 6))
    b2 = np.where(fixed != 0, 0.0, b2)
    xs = []
    for b in (b1, b2, b1 + b2):
        with lat.device(**_opts(3, tm, cm, tile_nodes=C.TILE_NODES[name], **extra)) as dev:
            dev.set_bc(fixed, None, b)
            dev.assemble()
            u, st = dev.solve(rtol=1e-30, max_iter=1, raise_on_noconv=False)
        assert st["iterations"] == 1
        xs.append(u.ravel())
    X = np.array(xs[:2]).T
    c = np.linalg.lstsq(X, xs[2], rcond=None)[0]
    fit = np.linalg.norm(X @ c - xs[2]) / np.linalg.norm(xs[2])
    lhs, rhs = (b2.ravel() @ xs[0]) * c[0], (b1.ravel() @ xs[1]) * c[1]
    # |lhs - rhs| against what the two sides can be at most (Cauchy-Schwarz): an error eps in every x_1 moves either side by
    # eps times its bound, and c by eps times the conditioning of the fit (columns scaled to unit length)
    size = abs(c[0]) * np.linalg.norm(b2) * np.linalg.norm(xs[0]) + abs(c[1]) * np.linalg.norm(b1) * np.linalg.norm(xs[1])
    kappa = np.linalg.cond(X / np.linalg.norm(X, axis=0))
    asym = abs(lhs - rhs) / size
    print(f"PRECOND_SYM form={form} modes=({tm},{cm}) linearity={fit:.3e} asymmetry={asym:.3e} kappa={kappa:.2f}")
    tol = P.GPU_TOL["fp32" if form == "precision1" else "fp64"][0]
    assert fit < 2 * tol and asym < (1 + kappa) * tol

def _ddm_problem(golden_dir):
    """The 6 x 3 x 3 BCC cells of tests/test_gpu_ddm.py as arrays: cell matrices, cell -> boundary-node table, positions;
    boundary sets b and c in one - a clamped face, rollers with prescribed values, one fully fixed node inside, two loads."""
    import json
    import os
    from pylatticedso_amd.lattice_sim import LatticeSim
    g = np.load(os.path.join(golden_dir, "ddm_bcc_6x3x3.npz"))
    L = LatticeSim(json.loads(str(g["preset_json"])), enable_domain_decomposition_solver=True, data_roots=[golden_dir])
    cb = L.cell_boundary_nodes()
    n = L.max_index_boundary + 1
    cell_nodes = np.array([L.index_boundary[cb[c]] for c in range(L.lattice.n_cells)], np.int32)
    bn = np.asarray(L._boundary_nodes_by_index())
    xyz = np.asarray(L.lattice.node_xyz)[bn]
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    fixed = np.zeros((n, 6), np.uint8)
    ubar = np.zeros((n, 6))
    face = xyz[:, 0] == lo[0]
    fixed[face] = 1
    ubar[face, 2] = 1e-3
    floor = np.flatnonzero((xyz[:, 1] == lo[1]) & ~face)[::2]
    fixed[floor, 1] = 1
    ubar[floor, 1] = -2e-3
    inside = int(np.argmin(((xyz - 0.5 * (lo + hi) - [0.4, 0.1, 0.2]) ** 2).sum(axis=1)))
    fixed[inside] = 1
    f = np.zeros((n, 6))
    far = np.flatnonzero(xyz[:, 0] == hi[0])
    f[far[-1]] = [0.03, -0.02, -0.1, 0.002, 0.005, -0.003]
    f[int(np.argmin(((xyz - 0.5 * (lo + hi) + [1.1, 0.4, 0.6]) ** 2).sum(axis=1)))] = [-0.04, 0.05, 0.03, -0.004, 0.001, 0.006]
    f = np.where(fixed != 0, 0.0, f)
    return n, cell_nodes, np.asarray(L.schur_complements), np.asarray(L.cell_schur_index, np.int32), xyz, fixed, ubar, f


@pytest.mark.parametrize("precond", [2, 3, 4])
def test_ddm_preconditioners(golden_dir, precond):
    """DDM handles: 2 = the factorised assembled matrix (x_1 is the solution), 3 = inverted node blocks, 4 = node blocks +
    twelve modes per aggregate of pl_ddm_set_geometry (aggregates from partition())."""
    from pylatticedso_amd import _capi
    n, cell_nodes, S, cell_S, xyz, fixed, ubar, f = _ddm_problem(golden_dir)
    G = P.ddm_matrix(n, cell_nodes, S, cell_S)
    G = 0.5 * (G + G.T)
    runs, agg = [], None
    for k in KS:
        with _capi.HipLattice.ddm(n, cell_nodes, S, cell_S, alpha_max=0.0, precond=precond,
                                  node_xyz=xyz if precond == 4 else None, coarse_max_dofs=48 if precond == 4 else 0) as dev:
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            runs.append(dev.solve(rtol=1e-30, max_iter=k, raise_on_noconv=False))
            agg = dev.partition()["agg"]
    if precond == 4:
        assert agg.min() >= 0 and len(np.unique(agg)) >= 2
    else:
        assert (agg == -1).all()
    ref = P.solve_iterates(G, fixed, ubar, f, P.ddm_minv(G, fixed, precond, xyz, agg), max(KS))
    devs = []
    for k, (u, st) in zip(KS, runs):
        assert st["iterations"] == k and int(st["precond_used"]) == precond, st
        devs.append(P.rel(u, ref[k - 1]))
    print(f"PRECOND_DEV group=fp64 form=ddm precond={precond} dev={' '.join(f'{d:.3e}' for d in devs)}")
    assert all(d < t for d, t in zip(devs, P.GPU_TOL["fp64"])), devs


def test_loopback_two_ranks_share_the_dense_level():
    """world = 2 on one device (loopback transport), precond = 2: Jacobi + the all-reduced dense level.  The iterates of the
    partitioned solve are those of the same reference, built on the aggregates the two ranks report."""
    from pylatticedso_amd.loopback import LoopbackGroup
    name = "bcc_6x3x3"
    lat = _lattice(name)
    fixed, ubar, f, _ = _case(name, 6, "b")
    devs = []
    ref = None
    for k in KS:
        with LoopbackGroup((1, 1, 1), (6, 3, 3), ["BCC"], [0.05], 2, axis=0, young=C.E, poisson=C.NU,
                           **_opts(2, 6, 6, tile_nodes=C.TILE_NODES[name])) as g:
            g.set_bc(g.scatter(lat.xyz, fixed), g.scatter(lat.xyz, ubar), g.scatter(lat.xyz, f))
            g.assemble()
            res = g.solve(rtol=1e-30, max_iter=k, raise_on_noconv=False)
            parts = g.each(lambda r: g.devs[r].partition())
        agg = g.gather(lat.xyz, [np.repeat(p["agg"][:, None].astype(float), 6, axis=1) for p in parts])[:, 0].astype(int)
        assert len(np.unique(agg)) >= 2
        assert all(st["iterations"] == k and int(st["precond_used"]) == 2 and int(st["comm_world"]) == 2 for _, st in res)
        if ref is None:
            M = P.Levels(lat.K, fixed, lat.xyz, {"agg": agg, "tile": agg}, 2, 6, 6).M
            ref = P.solve_iterates(lat.K, fixed, ubar, f, M, max(KS))
        devs.append(P.rel(g.gather(lat.xyz, [u for u, _ in res]), ref[k - 1]))
    print(f"PRECOND_DEV group=fp64 form=loopback2 dev={' '.join(f'{d:.3e}' for d in devs)}")
    assert all(d < t for d, t in zip(devs, P.GPU_TOL["fp64"])), devs
