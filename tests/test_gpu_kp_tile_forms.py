"""The tail loops of the LDS-resident K*p (tile_lds_body in pl_tile.h) at the largest tile the plan cuts, tile_nodes = 512.

The other suites run the LDS-resident forms with tiles of 16 to 64 nodes: a thread then never gets past the kLdsPre = 3 interior
visits whose words it fetched before the barrier, and never makes a second crossing visit.  A tile with more than
kLdsPre * kLdsBlock = 1536 interior visits runs the loop behind the pre-fetched visits, one with more than kLdsBlock = 512
crossing visits the second round of the crossing loop (its prefetch of the next visit's words, row and record).  Every test
counts both on the host, from the handle's own partition and the connectivity (interior: both ends in the tile; crossing:
exactly one), and asserts them, so that a change of the tiling cannot silently empty it.

    lattice                         tiles (nodes)    most interior / crossing visits of a tile
    Octet 6 x 6 x 6, 1 099 nodes    3 (366 - 367)    1 660 / 648     the smallest cube with both (5 x 5 x 5: 1 535 / 230)
    BCC 13 x 13 x 13, 4 941 nodes   16 (279 - 343)   1 014 / 554     the smallest cube with more than 512 crossing visits; no BCC
      condense = 1                                                   cube up to 11 x 11 x 11 (3 059 nodes) has a tile with more
                                                                     than 1 536 interior visits (the most: 1 331), so that loop
                                                                     is the Octet cube's

Forms: palette = 1 (kp_form 1, k_spmv_tile_lds) and palette = 0 (kp_form 2, the streaming k_spmv_tile_lds_t), the two passes of
the condensed operator (BCC, with the one-eliminated-end shortcut of the palette form), the deferred form of the short
iteration on both lattices, and precision = 1 for the float instantiations.

Bars: K x and the masked product against the oracle's sparse K at 1e-11 with the palette (records compared on 40 mantissa bits)
and 1e-13 without, as tests/test_gpu_parity.py holds these two forms; full solves (rtol 1e-11) at 1e-8 against the oracle's
direct solve, the bar of tests/test_gpu_tail_kernels.py; precision = 1 at the bar of test_fp32_solver_modes_match_oracle.
The fused dot p.Kp: after ONE iteration from u = 0, u_1 = alpha p_0 with alpha = r.z / p.Kp, and z = p_0 in that iteration, so
u_1.f = u_1.(K u_1) on the free rows whatever the preconditioner.  A K*p that is off by `bar` relative to |K p| moves p.Kp by at
most bar |p| |K p|, hence the bound bar * |u_1| |K u_1| on the difference, with the bar of the form's product.
Every test prints its figures (pytest -s) before it asserts."""
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import timoshenko_oracle as O   # noqa: E402
from pylatticedso_amd import _capi, lattice_arrays as LA   # noqa: E402

E, NU = 1013.0, 0.3
LDS_PRE, LDS_BLOCK = 3, 512      # kLdsPre, kLdsBlock (pl_tile.h)
#           geometry, radius, cells per edge, condense, (interior, crossing) visits some tile must exceed
LATTICES = {"octet": ("Octet", 0.03, 6, -1, (LDS_PRE * LDS_BLOCK, LDS_BLOCK)), "bcc": ("BCC", 0.05, 13, 1, (0, LDS_BLOCK))}
BAR = {1: 1e-11, 0: 1e-13}       # K x against the oracle: palette form / streaming form
KP_FORM = {1: 1, 0: 2}


def _rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


@functools.lru_cache(maxsize=None)
def _lattice(name):
    geom, radius, n, _, _ = LATTICES[name]
    lat = LA.generate((1.0, 1.0, 1.0), (n, n, n), [geom], [radius])
    pen = LA.penalize(lat, LA.compute_lzone(lat))
    ns = types.SimpleNamespace(xyz=np.ascontiguousarray(lat.node_xyz, float), conn=np.ascontiguousarray(lat.beam_conn, np.int32),
                               radius=np.ascontiguousarray(lat.beam_radius, float), seg_len=np.asarray(pen.seg_len),
                               seg_nsub=np.asarray(pen.seg_nsub), n_nodes=lat.n_nodes)
    key = np.c_[ns.radius, ns.seg_len.reshape(-1, 3), ns.seg_nsub.reshape(-1, 3)]
    uq, inv = np.unique(key, axis=0, return_inverse=True)      # the oracle's condensation, once per distinct strut
    sc = np.array([O.condensed_beam(k[0], k[1:4], k[4:7].astype(int), E, NU) for k in uq])[inv.ravel()]
    ns.K = O.assemble_condensed(ns.xyz, ns.conn, sc)
    rng = np.random.default_rng(31)
    ns.x = rng.standard_normal(6 * ns.n_nodes)
    ns.mask = rng.random((ns.n_nodes, 6)) < 0.2
    ns.fixed = np.zeros((ns.n_nodes, 6), np.uint8)
    ns.fixed[ns.xyz[:, 0] == ns.xyz[:, 0].min()] = 1
    ns.f = np.zeros((ns.n_nodes, 6))
    ns.f[ns.xyz[:, 0] == ns.xyz[:, 0].max(), 2] = -1e-3
    ns.f[ns.n_nodes // 2, :3] += [1e-3, -2e-3, 5e-4]
    ns.f[ns.fixed != 0] = 0.0
    return ns


@functools.lru_cache(maxsize=None)
def _direct(name):
    lat = _lattice(name)
    return O.solve_dirichlet(lat.K, lat.fixed, np.zeros_like(lat.f), lat.f).reshape(-1, 6)


def _device(name, **opts):
    lat = _lattice(name)
    return _capi.HipLattice(lat.xyz, lat.conn, lat.radius, lat.seg_len, lat.seg_nsub, E, NU, tile_nodes=512, precond=3,
                            spmv_kernel=3, condense=LATTICES[name][3], warm_start=0, **opts)


def _assert_tail_loops(name, dev):
    """Some tile has more interior / crossing visits than the pre-fetched ones cover (module docstring)."""
    lat, tile = _lattice(name), dev.partition()["tile"]
    ta, tb = tile[lat.conn[:, 0]], tile[lat.conn[:, 1]]
    n_tiles = int(tile.max()) + 1
    interior = np.bincount(ta[ta == tb], minlength=n_tiles)
    crossing = np.bincount(ta[ta != tb], minlength=n_tiles) + np.bincount(tb[ta != tb], minlength=n_tiles)
    print(f"{name}: {n_tiles} tiles of {np.bincount(tile).min()} - {np.bincount(tile).max()} nodes, most interior visits "
          f"{interior.max()}, most crossing visits {crossing.max()}")
    need_int, need_cross = LATTICES[name][4]
    assert interior.max() > need_int and crossing.max() > need_cross, (interior, crossing)


@functools.lru_cache(maxsize=None)
def _ordinary(name, palette):
    """(u, stats) of the ordinary iteration's full solve: checked against the oracle by its own test, the deferred form's
    reference."""
    lat = _lattice(name)
    with _device(name, palette=palette, short_iteration=-1) as dev:
        _assert_tail_loops(name, dev)
        dev.set_bc(lat.fixed, None, lat.f)
        dev.assemble()
        u, st = dev.solve(rtol=1e-11, max_iter=20000)
    u.setflags(write=False)
    return u, dict((k, st[k]) for k in ("converged", "iterations", "kp_form", "condensed_nodes", "short_iteration_used"))


@pytest.mark.parametrize("palette", [1, 0])
def test_products_and_fused_dot_on_large_tiles(palette):
    """Octet cube: K x, the masked product under a random 20 % mask, and the fused dot through a one-iteration solve."""
    lat, bar = _lattice("octet"), BAR[palette]
    K, x = lat.K, lat.x
    m = (~lat.mask).ravel().astype(float)
    with _device("octet", palette=palette, short_iteration=-1) as dev:
        _assert_tail_loops("octet", dev)
        dev.assemble()
        e_plain = _rel(dev.spmv(x), K @ x)
        dev.set_bc(lat.mask)
        e_masked = _rel(dev.spmv_free(x), m * (K @ (m * x)))
        print(f"palette {palette}: K x {e_plain:.2e}, masked {e_masked:.2e} (bar {bar:.0e})")
        assert e_plain < bar and e_masked < bar
        dev.set_bc(lat.fixed, None, lat.f)
        dev.assemble()
        u1, st = dev.solve(rtol=1e-30, max_iter=1, raise_on_noconv=False)
    assert int(st["kp_form"]) == KP_FORM[palette] and int(st["iterations"]) == 1
    u1 = u1.ravel()
    Ku = np.where(lat.fixed.ravel() != 0, 0.0, K @ u1)
    gap, scale = abs(u1 @ lat.f.ravel() - u1 @ Ku), np.linalg.norm(u1) * np.linalg.norm(Ku)
    print(f"palette {palette}: |u_1.f - u_1.K u_1| = {gap:.3e}, |u_1| |K u_1| = {scale:.3e}, ratio {gap / scale:.2e}")
    assert np.linalg.norm(u1) > 0 and gap <= bar * scale


@pytest.mark.parametrize("palette", [1, 0])
@pytest.mark.parametrize("name", ["octet", "bcc"])
def test_full_solve_on_large_tiles_matches_oracle(name, palette):
    """Ordinary iteration to rtol 1e-11 against the oracle's direct solve; on the BCC cube with node elimination, both passes
    of the condensed operator."""
    u, st = _ordinary(name, palette)
    err = _rel(u, _direct(name))
    print(f"{name} palette {palette}: {st['iterations']:.0f} iterations, {st['condensed_nodes']:.0f} condensed nodes, "
          f"kp_form {st['kp_form']:.0f}, error {err:.2e}")
    assert st["converged"] == 1 and int(st["kp_form"]) == KP_FORM[palette] and int(st["short_iteration_used"]) == 0
    assert (st["condensed_nodes"] > 0) == (name == "bcc")
    assert err < 1e-8


@pytest.mark.parametrize("palette", [1, 0])
@pytest.mark.parametrize("name", ["octet", "bcc"])
def test_deferred_form_on_large_tiles_matches_ordinary_form(name, palette):
    """The short iteration forced: the operand formed inside the K*p launch (the deferred form), against the ordinary form's
    solution."""
    lat = _lattice(name)
    u_ref, _ = _ordinary(name, palette)
    with _device(name, palette=palette, short_iteration=1) as dev:
        dev.set_bc(lat.fixed, None, lat.f)
        dev.assemble()
        u, st = dev.solve(rtol=1e-11, max_iter=20000)
    err = _rel(u, u_ref)
    print(f"{name} palette {palette}: {st['iterations']:.0f} iterations, kp_form {st['kp_form']:.0f}, against the ordinary form "
          f"{err:.2e}")
    assert st["converged"] == 1 and int(st["short_iteration_used"]) == 1 and int(st["kp_form"]) == KP_FORM[palette]
    assert (st["condensed_nodes"] > 0) == (name == "bcc")
    assert err < 1e-8


@pytest.mark.parametrize("palette", [1, 0])
def test_fp32_inner_solve_on_large_tiles(palette):
    """precision = 1 on the Octet cube: the float instantiations, at the bar of test_fp32_solver_modes_match_oracle."""
    lat = _lattice("octet")
    with _device("octet", palette=palette, short_iteration=-1, precision=1) as dev:
        dev.set_bc(lat.fixed, None, lat.f)
        dev.assemble()
        u, st = dev.solve(rtol=1e-9, max_iter=20000)
        res = np.where(lat.fixed != 0, 0.0, lat.f - dev.spmv(u))
    err, rres = _rel(u, _direct("octet")), np.linalg.norm(res) / np.linalg.norm(lat.f)
    print(f"palette {palette}: {st['iterations']:.0f} iterations, error {err:.2e}, true residual {rres:.2e}")
    assert st["converged"] == 1 and int(st["precision_used"]) == 1 and int(st["kp_form"]) == KP_FORM[palette]
    assert err < 1e-6 and rres <= 2e-9
