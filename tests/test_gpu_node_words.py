"""Node words of the PCG vector kernels: one 4-byte word {rx, ry, rz, class} per node instead of the node's 24 bytes of
Jacobi weights, 12 bytes of lever arm and its Dirichlet bits (pl_nodeword.h, k_dcl_* and the three vector kernels in
pl_coarse.h).  PL_NODE_WORDS=0 at pl_create restores the arrays; HipLattice.node_words_info() says what a handle does.

The class row and the bytes give the kernels the SAME numbers bit for bit, so switching them on may change a solve only through
the order of the atomic sums (restriction, dot products), exactly as two runs of one path differ from each other.

Iterate equality (test_iterates_equal_with_and_without_words): u_k for k = 1, 2, 3 (max_iter = k) and a full solve to rtol
1e-8, switch on against switch off, on three 4 x 4 x 4 lattices (Octet; BCC with node elimination, i.e. keep lists; BCC +
Octet), fp64 and precision = 1, 6- and 12-mode tile levels, boundary sets a - d of oracle/precond_cases.py (clamped face;
rollers with prescribed values; set a plus an interior node with four of its six dofs fixed - a class whose row is partly zero,
_set_c; a tile with a single free node).  tile_nodes is set low: 27 or 64 tiles in 2 x 2 x 2 aggregates (asserted), with the
lever arms as bytes on two of the lattices and as before on the third (TILE_NODES).

Bound: ten times the largest deviation MEASURED between two runs of the switch-off path on the same case (relative L2 of u,
MI355X, over all cases of a group; tools/measure_node_words.py prints them):
    group   measured off / off  u_1      u_2      u_3      full        bound u_1 u_2 u_3 full
    fp64    (precision 0)       4.9e-17  8.6e-16  6.7e-16  1.9e-9      4.931e-16 8.561e-15 6.711e-15 1.905e-8
    fp32    (precision 1)       0        0        0        0           0 (the runs are bit-identical: equality is asserted)
(three repetitions of the pair on each of the 48 cases; on against off in the same run: 3.6e-17, 5.3e-16, 4.1e-16, 5.5e-10 and
0, 0, 0, 0.  The full fp64 solves stop on the first iterate below rtol, and two runs whose residuals differ in the last bits
can stop one iteration apart: 1.9e-9 is that step, not rounding.)
The deviations of on against off measured in the same run are listed beside them in DESIGN.md section 7.
Iteration counts of the full solves agree within the +- 3 the suite allows between two handles.

Oracle parity (test_full_solves_match_oracle): the same full solves, switch on, against oracle/c_oracle.py (Jacobi PCG in C on
the condensed struts, rtol 1e-13) at 1e-8 relative L2, the bar tests/test_gpu_parity.py sets for a multi-level solve against
the oracle (test_strain_mode_levels_match_oracle, test_condensed_pcg_matches_oracle), both on the full solves of the
equality test (rtol 1e-8) and on the same solves taken to rtol 1e-11, as those tests solve.  Measured, largest of the 48 cases:
    rtol 1e-8    2.0e-9 (fp64)   2.0e-9 (precision 1)        rtol 1e-11   1.1e-12 (fp64)   1.6e-12 (precision 1)
The fall-back and stale-class tests solve to rtol 1e-11 and hold 1e-8 against a sparse-direct solve of the oracle's matrix
(measured 3e-14 ... 6e-13).  The 140 x 2 x 2 cantilever is the exception, see test_lever_arms_longer_than_a_byte.

Fall-backs and stale classes: see the tests.  Every test prints its figures (pytest -s) before it asserts."""
import contextlib
import functools
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle, precond_cases as C, timoshenko_oracle as O      # noqa: E402
from pylatticedso_amd import _capi, lattice_arrays as LA   # noqa: E402

E, NU = 1013.0, 0.3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = {"octet": (["Octet"], [0.03], -1), "bcc_elim": (["BCC"], [0.05], 1), "hybrid": (["BCC", "Octet"], [0.04, 0.03], -1)}
# opts.tile_nodes and whether the lever arms then fit bytes.  The brick edge follows from tile_nodes (pl_tile.h): 16 cuts the
# Octet lattice into 3 bricks per axis, whose aggregate centres are multiples of 2/3 - no bytes, classes only; 3 and 7 cut the
# other two into 4 bricks per axis (one cell each, 64 tiles, 2 x 2 x 2 aggregates): lever arms in half cells, e = 1
TILE_NODES = {"octet": 16, "bcc_elim": 3, "hybrid": 7}
BYTE_EXP = {"octet": -1, "bcc_elim": 1, "hybrid": 1}
KS = (1, 2, 3)
# relative L2 of u_1, u_2, u_3 and of the full solve: 10 x the largest off / off deviation measured (module docstring)
BOUND = {0: (4.931e-16, 8.561e-15, 6.711e-15, 1.905e-8), 1: (0.0, 0.0, 0.0, 0.0)}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _lattice(name, cells=(4, 4, 4), size=1.0):
    geom, radii, _ = LATTICES[name]
    lat = LA.generate((size, size, size), cells, geom, radii)
    pen = LA.penalize(lat, LA.compute_lzone(lat))
    return types.SimpleNamespace(xyz=np.ascontiguousarray(lat.node_xyz, float), conn=np.ascontiguousarray(lat.beam_conn, np.int32),
                                 radius=np.ascontiguousarray(lat.beam_radius, float), seg_len=np.asarray(pen.seg_len),
                                 seg_nsub=np.asarray(pen.seg_nsub), n_nodes=lat.n_nodes, lat=lat)


@contextlib.contextmanager
def _switch(words):
    old = os.environ.get("PL_NODE_WORDS")
    os.environ["PL_NODE_WORDS"] = "1" if words else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["PL_NODE_WORDS"]
        else:
            os.environ["PL_NODE_WORDS"] = old


def _device(lat, words, radius=None, **kw):
    """A handle created with the switch on or off (the library reads it in pl_create)."""
    with _switch(words):
        return _capi.HipLattice(lat.xyz, lat.conn, lat.radius if radius is None else radius, lat.seg_len, lat.seg_nsub, E, NU, **kw)


def _opts(name, precision, tm, **kw):
    o = dict(precond=3, tile_nodes=TILE_NODES[name], coarse_max_dofs=600, tile_modes=tm, coarse_modes=6, coarse_storage=32, palette=1,
             condense=LATTICES[name][2], short_iteration=-1, warm_start=0, precision=precision)
    o.update(kw)
    return o


@functools.lru_cache(maxsize=None)
def _partition(name):
    lat = _lattice(name)
    with _device(lat, True, **_opts(name, 0, 6)) as dev:
        part = dev.partition()
    assert len(np.unique(part["tile"])) >= 4 and len(np.unique(part["agg"])) >= 2, "TILE_NODES must cut several tiles and two aggregates"
    return part


def _set_c(lat, part):
    """Boundary set a plus ONE node inside the lattice with four of its six dofs fixed at non-zero values: a class whose row
    is partly zero.  Strictly inside a tile where the partition has such a node (every strut at it stays in its tile; the
    one-cell tiles of TILE_NODES have none): the node with the largest share of its neighbours in its own tile."""
    fixed, ubar, f, info = C.boundary_set("a", lat, part)
    tile = np.asarray(part["tile"])
    lo, hi = lat.xyz.min(axis=0), lat.xyz.max(axis=0)
    inside = np.all((lat.xyz > lo) & (lat.xyz < hi), axis=1)
    same, deg = np.zeros(lat.n_nodes), np.zeros(lat.n_nodes)
    for ia, ib in lat.conn:
        deg[ia] += 1
        deg[ib] += 1
        if tile[ia] == tile[ib]:
            same[ia] += 1
            same[ib] += 1
    ok = inside & (deg >= 3)
    ok[[info["tip"], info["inner"]]] = False
    assert ok.any()
    score = np.where(ok, same / np.maximum(deg, 1), -1.0)
    i = int(np.argmax(score))
    fixed[i, [0, 1, 2, 4]] = 1
    ubar[i, [0, 1, 2, 4]] = [1e-3, -5e-4, 2e-4, 1e-3]
    return fixed, ubar, np.where(fixed != 0, 0.0, f), dict(info, inside=i, strictly_inside=bool(same[i] == deg[i]))


@functools.lru_cache(maxsize=None)
def _bc(name, bset):
    if bset == "c":
        return _set_c(_lattice(name), _partition(name))
    return C.boundary_set(bset, _lattice(name), _partition(name))


@functools.lru_cache(maxsize=None)
def _oracle(name, bset):
    lat = _lattice(name)
    fixed, ubar, f, _ = _bc(name, bset)
    sc = c_oracle.condense_unique(lat.radius, lat.seg_len, lat.seg_nsub, E, NU)
    u, _, _ = c_oracle.pcg(lat.xyz, lat.conn, sc, fixed, ubar, f, rtol=1e-13)
    return u


def _solves(name, precision, tm, bset, words):
    """u_1, u_2, u_3 and the full solve, each from a fresh handle: [(u, stats, info)] (not cached: run-to-run deviation)."""
    lat = _lattice(name)
    fixed, ubar, f, _ = _bc(name, bset)
    out = []
    for k in KS + (None,):
        with _device(lat, words, **_opts(name, precision, tm)) as dev:
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            if k is None:
                u, st = dev.solve(rtol=1e-8, max_iter=20000)
                assert st["converged"] == 1
            else:
                u, st = dev.solve(rtol=1e-30, max_iter=k, raise_on_noconv=False)
                assert st["iterations"] == k
            assert int(st["precond_used"]) == 3 and int(st["precision_used"]) == precision
            assert (st["condensed_nodes"] > 0) == (LATTICES[name][2] > 0)
            out.append((u, st, dev.node_words_info()))
    return out


@functools.lru_cache(maxsize=None)
def _on_off(name, precision, tm, bset):
    """The switch-on and switch-off runs of one case, shared by the tests below."""
    return _solves(name, precision, tm, bset, True), _solves(name, precision, tm, bset, False)


CASES = [(n, p, tm) for n in LATTICES for p in (0, 1) for tm in (6, 12)]


@pytest.mark.parametrize("name,precision,tm", CASES)
def test_iterates_equal_with_and_without_words(name, precision, tm):
    for bset in C.BOUNDARY_SETS:
        on, off = _on_off(name, precision, tm, bset)
        if name == "octet" and bset == "c":      # here the partly fixed node IS strictly inside its tile (12 of 12 struts)
            assert _bc(name, bset)[3]["strictly_inside"]
        devs = [_rel(a[0], b[0]) for a, b in zip(on, off)]
        print(f"NODE_WORDS_DEV lattice={name} precision={precision} tile_modes={tm} set={bset} "
              f"dev={' '.join(f'{d:.3e}' for d in devs)} its={on[-1][1]['iterations']}/{off[-1][1]['iterations']} "
              f"classes={on[0][2]['n_classes']} e={on[0][2]['byte_exp']}")
        for (_, _, info_on), (_, _, info_off) in zip(on, off):
            assert info_on["classes"] and 1 <= info_on["n_classes"] <= 256
            assert info_on["byte_exp"] == BYTE_EXP[name] and info_on["bytes"] == (BYTE_EXP[name] >= 0)
            assert info_off == {"classes": False, "n_classes": 0, "bytes": False, "byte_exp": -1}
        assert all(d <= b for d, b in zip(devs, BOUND[precision])), (name, precision, tm, bset, devs)
        assert abs(on[-1][1]["iterations"] - off[-1][1]["iterations"]) <= 3


@pytest.mark.parametrize("name,precision,tm", CASES)
def test_full_solves_match_oracle(name, precision, tm):
    lat = _lattice(name)
    for bset in C.BOUNDARY_SETS:
        on, _ = _on_off(name, precision, tm, bset)
        fixed, ubar, f, _ = _bc(name, bset)
        with _device(lat, True, **_opts(name, precision, tm)) as dev:      # the parity leg: the same solve to rtol 1e-11
            dev.set_bc(fixed, ubar, f)
            dev.assemble()
            u, st = dev.solve(rtol=1e-11, max_iter=20000)
            assert st["converged"] == 1 and dev.node_words_info()["classes"]
        err8, err = _rel(on[-1][0], _oracle(name, bset)), _rel(u, _oracle(name, bset))
        print(f"NODE_WORDS_ORACLE lattice={name} precision={precision} tile_modes={tm} set={bset} "
              f"err(rtol 1e-8)={err8:.3e} err(rtol 1e-11)={err:.3e}")
        assert err8 < 1e-8 and err < 1e-8, (name, precision, tm, bset, err8, err)
        assert np.array_equal(u[fixed != 0], ubar[fixed != 0]) and np.array_equal(on[-1][0][fixed != 0], ubar[fixed != 0])


def _cantilever(lat):
    fixed = np.zeros((lat.n_nodes, 6), np.uint8)
    fixed[lat.xyz[:, 0] == lat.xyz[:, 0].min()] = 1
    f = np.zeros((lat.n_nodes, 6))
    tip = lat.xyz[:, 0] == lat.xyz[:, 0].max()
    f[tip, 2] = -0.1 / tip.sum()
    return fixed, f


def _oracle_solve(lat, radius, fixed, f):
    """Sparse-direct solve of the oracle's assembled matrix (the slender lattices here are too ill-conditioned for the
    Jacobi PCG of c_oracle to be the more accurate side)."""
    sc = c_oracle.condense_unique(radius, lat.seg_len, lat.seg_nsub, E, NU)
    K = O.assemble_condensed(lat.xyz, lat.conn, sc)
    return O.solve_dirichlet(K, fixed != 0, np.zeros_like(f), f).reshape(-1, 6)


def test_more_than_256_classes_fall_back_and_come_back():
    """7 x 7 x 7 BCC with its own radius in every cell: 343 cell centres with 343 different diagonals, so the classes are
    refused and the kernels read dinv32.  Back at one radius the next assembly makes no attempt
    (back-off, as the record palette's), the one after it does, and the classes are in use again."""
    n = 7
    rc = 0.03 + 1e-4 * np.arange(n ** 3)
    g = LA.generate((1, 1, 1), (n, n, n), ["BCC"], [0.05], cell_radii_override=rc.reshape(-1, 1))
    pen = LA.penalize(g, LA.compute_lzone(g))
    lat = types.SimpleNamespace(xyz=np.ascontiguousarray(g.node_xyz, float), conn=np.ascontiguousarray(g.beam_conn, np.int32),
                                radius=np.ascontiguousarray(g.beam_radius, float), seg_len=np.asarray(pen.seg_len),
                                seg_nsub=np.asarray(pen.seg_nsub), n_nodes=g.n_nodes)
    fixed, f = _cantilever(lat)
    # one radius again: the radii AND the penalised segments that follow from them (the graded ones alone keep the records apart)
    gu = LA.generate((1, 1, 1), (n, n, n), ["BCC"], [0.05])
    pen_u = LA.penalize(gu, LA.compute_lzone(gu))
    assert np.array_equal(gu.beam_conn, g.beam_conn)
    uniform = np.ascontiguousarray(gu.beam_radius, float)
    lat_u = types.SimpleNamespace(xyz=lat.xyz, conn=lat.conn, seg_len=np.asarray(pen_u.seg_len), seg_nsub=np.asarray(pen_u.seg_nsub))
    # tile_nodes = 3: 8 bricks per axis of 7/8 of a cell in 4 aggregates per axis - lever arms in sixteenths or coarser,
    # so the BYTES are in use while the classes are not: the kernels read the word for the lever arm and dinv32 for D^-1
    with _device(lat, True, **_opts("octet", 0, 6, tile_nodes=3)) as dev:
        dev.set_bc(fixed, None, f)
        dev.assemble()
        info = dev.node_words_info()
        print("NODE_WORDS_FALLBACK graded:", info)
        assert not info["classes"] and info["n_classes"] > 256 and info["bytes"] and 0 <= info["byte_exp"] <= 8
        u, st = dev.solve(rtol=1e-11, max_iter=20000)
        err = _rel(u, _oracle_solve(lat, lat.radius, fixed, f))
        print(f"NODE_WORDS_FALLBACK graded: err={err:.3e}")
        assert st["converged"] == 1 and err < 1e-8
        uref = _oracle_solve(lat_u, uniform, fixed, f)
        seen = []
        for _ in range(2):
            dev.update_radii(uniform)
            dev.update_segments(lat_u.seg_len, lat_u.seg_nsub)
            assert not dev.node_words_info()["classes"]            # stale until the next assembly
            dev.assemble()
            seen.append(dev.node_words_info())
            u, st = dev.solve(rtol=1e-11, max_iter=20000)
            print(f"NODE_WORDS_FALLBACK uniform again: err={_rel(u, uref):.3e}")
            assert st["converged"] == 1 and _rel(u, uref) < 1e-8
        print("NODE_WORDS_FALLBACK uniform again:", seen)
        assert not seen[0]["classes"] and seen[0]["n_classes"] == 0      # one assembly without an attempt
        assert seen[1]["classes"] and 1 <= seen[1]["n_classes"] <= 256


def test_cell_size_that_is_not_dyadic_keeps_the_lever_arms():
    """Cells of 0.7: no lever arm is a multiple of 2^-8, so the bytes are off (the kernels subtract the reference point as
    before) while the classes are on."""
    geom, radii, _ = LATTICES["bcc_elim"]
    g = LA.generate((0.7, 0.7, 0.7), (4, 4, 4), geom, [0.035])
    pen = LA.penalize(g, LA.compute_lzone(g))
    lat = types.SimpleNamespace(xyz=np.ascontiguousarray(g.node_xyz, float), conn=np.ascontiguousarray(g.beam_conn, np.int32),
                                radius=np.ascontiguousarray(g.beam_radius, float), seg_len=np.asarray(pen.seg_len),
                                seg_nsub=np.asarray(pen.seg_nsub), n_nodes=g.n_nodes)
    fixed, f = _cantilever(lat)
    uref = _oracle_solve(lat, lat.radius, fixed, f)
    for precision in (0, 1):
        with _device(lat, True, **_opts("octet", precision, 6, tile_nodes=3)) as dev:
            dev.set_bc(fixed, None, f)
            dev.assemble()
            info = dev.node_words_info()
            print("NODE_WORDS_FALLBACK cell 0.7:", info)
            assert info["classes"] and not info["bytes"] and info["byte_exp"] == -1
            u, st = dev.solve(rtol=1e-11, max_iter=20000)
            print(f"NODE_WORDS_FALLBACK cell 0.7: precision={precision} err={_rel(u, uref):.3e}")
            assert st["converged"] == 1 and _rel(u, uref) < 1e-8


def test_lever_arms_longer_than_a_byte(tmp_path):
    """One aggregate along a 140 x 2 x 2 lattice: lever arms of up to 70 cells = 140 half cells, beyond the 127 units a byte
    holds.  (The issue proposed 40 x 2 x 2; the packing header says that one fits - 40 half cells - and that 140 does not.)

    Bound of the solution: the free-free block of this cantilever has a condition number of 3.6e10 (4.2e10 after Jacobi scaling),
    and the sparse-direct reference is itself no better than about 1e-7 - its relative residual is 1.2e-6 in fp64, and two steps
    of iterative refinement move it by 6e-8 and 1e-7 without settling.  The bound is ten times that error of the reference,
    1e-6; the device solve to rtol 1e-12 was measured 1.5e-7 away from it."""
    exe = str(tmp_path / "nodeword_main")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "nodeword_main.cpp"), "-o", exe], check=True)
    assert subprocess.run([exe, "overflow", "40", "2", "2", "1.0"], capture_output=True, text=True).stdout.strip() == "fits 1"
    long_ = subprocess.run([exe, "overflow", "140", "2", "2", "1.0"], capture_output=True, text=True)
    assert long_.returncode == 0 and long_.stdout.strip() == "overflow"
    lat = _lattice("bcc_elim", (140, 2, 2))
    fixed, f = _cantilever(lat)
    f *= 1e-3
    with _device(lat, True, **_opts("octet", 0, 6, tile_nodes=16, coarse_max_dofs=6)) as dev:
        part = dev.partition()
        assert len(np.unique(part["agg"])) == 1 and len(np.unique(part["tile"])) >= 4
        dev.set_bc(fixed, None, f)
        dev.assemble()
        info = dev.node_words_info()
        print("NODE_WORDS_FALLBACK 140 x 2 x 2:", info)
        assert info["classes"] and not info["bytes"] and info["byte_exp"] == -1
        u, st = dev.solve(rtol=1e-12, max_iter=100000)
        err = _rel(u, _oracle_solve(lat, lat.radius, fixed, f))
        print(f"NODE_WORDS_FALLBACK 140 x 2 x 2: err={err:.3e}")
        assert st["converged"] == 1 and err < 1e-6        # (ten times the reference's own error: docstring)


@pytest.mark.parametrize("precision", [0, 1])
def test_classes_follow_new_radii_and_a_new_dirichlet_set(precision):
    """Stale classes: after pl_update_radii (other uniform radii) and after pl_set_bc with another Dirichlet set the solve
    is the oracle's for the NEW system - the class table is rebuilt with dinv32, not kept."""
    lat = _lattice("hybrid")
    fixed, f = _cantilever(lat)
    r2 = lat.radius * 1.25                                             # (two uniform radii again: BCC and Octet struts)
    fixed2 = np.zeros_like(fixed)
    fixed2[lat.xyz[:, 0] == lat.xyz[:, 0].max()] = 1                 # the other face clamped, rollers on the floor
    fixed2[(lat.xyz[:, 2] == 0.0) & (lat.xyz[:, 0] < 2.0), 2] = 1
    f2 = np.zeros_like(f)
    f2[lat.xyz[:, 0] == 0.0, 1] = 1e-3
    f2 = np.where(fixed2 != 0, 0.0, f2)
    with _device(lat, True, **_opts("hybrid", precision, 12)) as dev:
        dev.set_bc(fixed, None, f)
        dev.assemble()
        u1, st1 = dev.solve(rtol=1e-11, max_iter=20000)
        i1 = dev.node_words_info()
        dev.update_radii(r2)
        assert not dev.node_words_info()["classes"]
        dev.assemble()
        u2, st2 = dev.solve(rtol=1e-11, max_iter=20000)
        i2 = dev.node_words_info()
        dev.set_bc(fixed2, None, f2)                                     # (an assembled handle rebuilds what the mask changes)
        i3 = dev.node_words_info()
        u3, st3 = dev.solve(rtol=1e-11, max_iter=20000)
    errs = [_rel(u1, _oracle_solve(lat, lat.radius, fixed, f)), _rel(u2, _oracle_solve(lat, r2, fixed, f)),
            _rel(u3, _oracle_solve(lat, r2, fixed2, f2))]
    print(f"NODE_WORDS_STALE precision={precision} errs={' '.join(f'{e:.3e}' for e in errs)} info={i1} {i2} {i3}")
    assert all(s["converged"] == 1 for s in (st1, st2, st3))
    assert i1["classes"] and i2["classes"] and i3["classes"] and i1["bytes"] and i3["bytes"]
    assert _rel(u2, u1) > 1e-2                                            # the radii did change the answer
    assert all(e < 1e-8 for e in errs), errs
    assert np.all(u3[fixed2 != 0] == 0.0)
