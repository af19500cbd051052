"""The two vector kernels of the PCG iteration (k_pcg_update_tile, k_pcg_direction_flat in pl_coarse.h) at tile shapes the other
suites do not reach.  tests/test_gpu_precond.py and tests/test_gpu_node_words.py cut tiles of 16 and 32 nodes, smaller than a
wave's 21 nodes of the direction kernel; the benchmark's tiles hold about 152.  Here:

    case                                        what it reaches
    Octet 12 x 3 x 3 (613 nodes),               tiles of about 120 and about 200 nodes in three and two aggregates: three lanes
      tile_nodes = 96 and 300                   per node is no multiple of 64; waves inside one tile next to waves that straddle
                                                two tiles and two aggregates; the last block of the flat grid partly filled; more
                                                pairs per tile than the workgroup has lanes
    BCC 16 x 3 x 3 (416 nodes), condense = 1,   the keep list of the direction kernel, skipped rows of the update kernel, tiles
      tile_nodes = 96                           of about 80 nodes in three aggregates
    Octet 4 x 4 x 4 (365 nodes),                eight tiles of 32 to 63 nodes; ONE tile of 365 nodes, longer than the workgroup:
      tile_nodes = 96 and 200                   more than three passes of pairs, two nodes per lane (one aggregate each: the brick
    BCC 5 x 5 x 5 (341 nodes), condense = 1,    edge follows from tile_nodes and an aggregate spans at least 1.5 bricks per axis,
      tile_nodes = 96                           so a cube this small cannot have tiles of 90 nodes AND two aggregates)
    all with tile_modes / coarse_modes          every instantiation a solve can pick
      (6, 6), (12, 6), (12, 12), precision 0, 1
    Octet 4 x 4 x 4, cell size 0.7              lever arms from positions minus reference point (no node-word bytes, no rel32)
    boundary set d (oracle/precond_cases.py)    a tile of about 120 nodes with a single free node

Each case stops the solve after k = 1, 2, 3 iterations (max_iter = k, fresh handle) and compares u_k with the PCG under the
dense fp64 restatement of the preconditioner on the handle's own partition (oracle/precond_oracle.py), as
tests/test_gpu_precond.py does; a full solve to rtol 1e-11 is held to 1e-8 against the C oracle, the bar of
tests/test_gpu_parity.py.

Bounds on u_1, u_2, u_3 (relative L2): ten times the largest deviation from the oracle MEASURED with the build before
k_pcg_direction_flat was rewritten (MI355X; `PYTHONPATH=. python tests/test_gpu_tail_kernels.py` prints every case), per group and per k - what deviates
is the fp32 copy of D^-1 and of the dense level, not these kernels:
    group                                   measured u_1, u_2, u_3          bound
    fp64   precision 0                      4.3e-8   3.2e-7   1.3e-7          4.276e-7  3.211e-6  1.273e-6
    fp32   precision 1                      6.7e-8   1.1e-7   1.1e-7          6.676e-7  1.055e-6  1.122e-6
    fp32e  precision 1 with condense = 1    1.1e-6   1.5e-5   3.9e-5          1.092e-5  1.477e-4  3.885e-4
(profiles/r17_tail_kernels_oracle_dev_parent.txt; with the rewritten kernel: profiles/r17_tail_kernels_oracle_dev.txt - the same
figures to three digits, the largest full-solve error 1.9e-11.)  The fp64 figure is set by the node-elimination cases (without
them 1.4e-8, 3.1e-8, 3.7e-8).  precision = 1 with node elimination runs the elimination's prologue and back-substitution on
fp32-stored vectors and is 1e-6 ... 4e-5 off before the fp64 refinement has visited the inner solve (tests/test_gpu_precond.py
leaves it unbounded for that reason) and moves from run to run with the order of the atomic sums (u_2 of the parent build:
1.48e-5 in the recorded run, 1.56e-5 in profiles/r17_tail_kernels_oracle_dev_parent_other_run.txt; the bound is from the smaller): that group guards against a gross error only, the fp64 legs of the same
cases are the sharp check.
Every test prints its figures (pytest -s) before it asserts."""
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle, precond_cases as C, precond_oracle as P, timoshenko_oracle as O   # noqa: E402
from pylatticedso_amd import _capi, lattice_arrays as LA   # noqa: E402

KS = (1, 2, 3)
# ten times the deviation measured with the build before the rewrite (module docstring)
BOUND = {"fp64": (4.276e-7, 3.211e-6, 1.273e-6), "fp32": (6.676e-7, 1.055e-6, 1.122e-6), "fp32e": (1.092e-5, 1.477e-4, 3.885e-4)}
#         lattice: geometry, radii, cells, cell size, condense
LATTICES = {"octet_long": (["Octet"], [0.03], (12, 3, 3), 1.0, -1), "bcc_long_elim": (["BCC"], [0.05], (16, 3, 3), 1.0, 1),
            "octet": (["Octet"], [0.03], (4, 4, 4), 1.0, -1), "bcc_elim": (["BCC"], [0.05], (5, 5, 5), 1.0, 1),
            "octet07": (["Octet"], [0.03], (4, 4, 4), 0.7, -1)}
# the lattices long enough for tiles beyond a wave AND several aggregates: (fewest tiles, shortest longest tile, fewest aggregates)
LONG = {("octet_long", 96): (4, 100, 3), ("octet_long", 300): (3, 180, 2), ("bcc_long_elim", 96): (4, 70, 3)}
#        (lattice, tile_nodes, boundary set)
SHAPES = [("octet_long", 96, "b"), ("octet_long", 300, "b"), ("bcc_long_elim", 96, "b"), ("octet", 96, "b"), ("octet", 200, "b"),
          ("bcc_elim", 96, "b")]
CASES = [(n, tn, b, tm, cm, p) for n, tn, b in SHAPES for tm, cm in C.MODE_PAIRS for p in (0, 1)]
CASES += [("octet07", 96, "b", 12, 6, 0), ("octet07", 96, "b", 12, 6, 1), ("octet_long", 96, "d", 12, 6, 0),
          ("octet_long", 96, "d", 6, 6, 1), ("bcc_long_elim", 96, "d", 12, 12, 0)]


@functools.lru_cache(maxsize=None)
def _lattice(name):
    geom, radii, cells, size, _ = LATTICES[name]
    lat = LA.generate((size, size, size), cells, geom, radii)
    pen = LA.penalize(lat, LA.compute_lzone(lat))
    ns = types.SimpleNamespace(xyz=np.ascontiguousarray(lat.node_xyz, float), conn=np.ascontiguousarray(lat.beam_conn, np.int32),
                               radius=np.ascontiguousarray(lat.beam_radius, float), seg_len=np.asarray(pen.seg_len),
                               seg_nsub=np.asarray(pen.seg_nsub), n_nodes=lat.n_nodes)
    ns.scalars = c_oracle.condense_unique(ns.radius, ns.seg_len, ns.seg_nsub, C.E, C.NU)
    sc = np.array([O.condensed_beam(r, l, n, C.E, C.NU) for r, l, n in zip(ns.radius, ns.seg_len, ns.seg_nsub)])
    ns.K = O.assemble_condensed(ns.xyz, ns.conn, sc).toarray()
    return ns


def _opts(name, tile_nodes, tm, cm, precision):
    return dict(precond=3, tile_nodes=tile_nodes, coarse_max_dofs=C.COARSE_MAX_DOFS[cm], tile_modes=tm, coarse_modes=cm,
                coarse_storage=32, condense=LATTICES[name][4], short_iteration=-1, warm_start=0, precision=precision)


def _device(lat, **opts):
    return _capi.HipLattice(lat.xyz, lat.conn, lat.radius, lat.seg_len, lat.seg_nsub, C.E, C.NU, **opts)


@functools.lru_cache(maxsize=None)
def _partition(name, tile_nodes, cm):
    with _device(_lattice(name), **_opts(name, tile_nodes, 6 if cm == 6 else 12, cm, 0)) as dev:
        return dev.partition()


@functools.lru_cache(maxsize=None)
def _bc(name, tile_nodes, cm, bset):
    return C.boundary_set(bset, _lattice(name), _partition(name, tile_nodes, cm))


@functools.lru_cache(maxsize=None)
def _reference(name, tile_nodes, bset, tm, cm):
    """u_1, u_2, u_3 of the PCG under the restated preconditioner (shared by the two precisions of a case)."""
    lat, part = _lattice(name), _partition(name, tile_nodes, cm)
    fixed, ubar, f, _ = _bc(name, tile_nodes, cm, bset)
    M = P.Levels(lat.K, fixed, lat.xyz, part, 3, tm, cm).M
    elim = None
    if LATTICES[name][4] > 0:      # the eliminated set avoids the Dirichlet nodes: known once the boundary set is in place
        with _device(lat, **_opts(name, tile_nodes, tm, cm, 0)) as dev:
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            dev.solve(rtol=1e-30, max_iter=1, raise_on_noconv=False)
            elim = dev.partition()["eliminated"]
        assert elim.any() and not (fixed[elim] != 0).any()
    return P.solve_iterates(lat.K, fixed, ubar, f, M, max(KS), elim)


@functools.lru_cache(maxsize=None)
def _c_oracle(name, tile_nodes, cm, bset):
    lat = _lattice(name)
    fixed, ubar, f, _ = _bc(name, tile_nodes, cm, bset)
    return c_oracle.pcg(lat.xyz, lat.conn, lat.scalars, fixed, ubar, f, rtol=1e-13)[0]


def _group(name, precision):
    return "fp64" if precision == 0 else ("fp32e" if LATTICES[name][4] > 0 else "fp32")


def _run(name, tile_nodes, bset, tm, cm, precision):
    """(deviations of u_1, u_2, u_3 from the reference, error of the full solve against the C oracle, description)."""
    lat, part = _lattice(name), _partition(name, tile_nodes, cm)
    fixed, ubar, f, info = _bc(name, tile_nodes, cm, bset)
    opts = _opts(name, tile_nodes, tm, cm, precision)
    sizes = np.bincount(part["tile"])
    if (name, tile_nodes) in LONG:      # the shapes this file is about
        tiles, longest, aggs = LONG[(name, tile_nodes)]
        assert len(sizes) >= tiles and sizes.max() >= longest and len(np.unique(part["agg"])) >= aggs, (sizes, np.unique(part["agg"]))
    ref = _reference(name, tile_nodes, bset, tm, cm)
    devs = []
    for k in KS:
        with _device(lat, **opts) as dev:
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            u, st = dev.solve(rtol=1e-30, max_iter=k, raise_on_noconv=False)
            words = dev.node_words_info()
            assert np.array_equal(dev.partition()["tile"], part["tile"])
        assert st["iterations"] == k and int(st["precond_used"]) == 3 and int(st["precision_used"]) == precision
        assert int(st["short_iteration_used"]) == 0 and (st["condensed_nodes"] > 0) == (LATTICES[name][4] > 0)
        devs.append(P.rel(u, ref[k - 1]))
    with _device(lat, **opts) as dev:
        dev.set_bc(fixed, ubar, f)
        dev.assemble()
        u, st = dev.solve(rtol=1e-11, max_iter=20000)
    assert st["converged"] == 1
    err = P.rel(u, _c_oracle(name, tile_nodes, cm, bset))
    what = (f"tiles={len(sizes)} longest={sizes.max()} shortest={sizes.min()} aggs={len(np.unique(part['agg']))} "
            f"bytes={int(words['bytes'])} classes={int(words['classes'])}")
    if bset == "d":
        assert info["tile_nodes"] > 64
        what += f" single_free_node_tile={info['tile_nodes']}"
    return devs, err, what


@pytest.mark.parametrize("name,tile_nodes,bset,tm,cm,precision", CASES)
def test_iterates_and_full_solve(name, tile_nodes, bset, tm, cm, precision):
    devs, err, what = _run(name, tile_nodes, bset, tm, cm, precision)
    group = _group(name, precision)
    print(f"TAIL_DEV group={group} lattice={name} tile_nodes={tile_nodes} set={bset} modes=({tm},{cm}) precision={precision} "
          f"dev={' '.join(f'{d:.3e}' for d in devs)} full={err:.3e} {what}")
    if name == "octet07":      # neither bytes nor exact floats: the kernels read positions and reference points
        assert "bytes=0" in what
    assert all(d < b for d, b in zip(devs, BOUND[group])), (group, devs, BOUND[group])
    assert err < 1e-8, err


if __name__ == "__main__":      # the figures behind BOUND: every case, nothing asserted on the deviations
    worst = {}
    for case in CASES:
        devs, err, what = _run(*case)
        g = _group(case[0], case[5])
        worst[g] = [max(a, b) for a, b in zip(worst.get(g, [0.0] * 4), devs + [err])]
        print(f"TAIL_DEV group={g} case={case} dev={' '.join(f'{d:.3e}' for d in devs)} full={err:.3e} {what}", flush=True)
    for g, w in worst.items():
        print(f"TAIL_WORST group={g} u1={w[0]:.3e} u2={w[1]:.3e} u3={w[2]:.3e} full={w[3]:.3e}")
