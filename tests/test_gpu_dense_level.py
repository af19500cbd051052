"""The dense coarse level, path by path, against a long-double host reference (oracle/dense_oracle.py).

PCG converges to the right displacements under ANY symmetric positive definite preconditioner, so a dense level that drops
the band-edge product, reads a ring slot one lap late or misses a parked slice costs a few iterations and nothing else.
pl_debug_dense_level runs the calls of the assembly and of the preconditioner (csrc/pl_dense.h, the explicit inverse of
csrc/pl_small.h, the band transfer of csrc/pl_coarse.h) with their production switches on a matrix of the test's:

    case  nb  bw     n  walk   what it reaches
    a      5   2   320  ring   band truncation in chain and walk; trtri_rows = 3 cuts [0, 3) and [3, 5)
    b      5   2   300  ring   the same with identity padding
    c     16   5  1024  ring   nb > kRing: the slot index wraps; six ranges
    d     14  11   896  ring   bw + 1 = kRing: the ring at its limit
    e     15  12   960  mfma   the banded matrix-pipe walk; a later range re-reads the stored slices
    f     32   6  2048  ring   kOneGemvMaxDofs: the largest explicit inverse (bfloat16, trtri_rows = 3 only)

a - e: storage 64, 32, 16 and trtri_rows 0, 1, 3; a and c also with the band packed and unpacked (k_band_pack / k_band_unpack)
in front of the factorisation.  The persistent chain k_chol_chain (opts.chol_persistent, off everywhere) is NOT covered: it
spins on a grid barrier and is not launched from a test.

What is asserted, per case and storage:
  1  info == 0, W exactly zero above the diagonal, Wt == W^T bit for bit;
  2  W bit-identical across the schedules (where the walk is cut, band transfer);
  3  ring form: W_32 == float32(W_64) and W_16 == round_storage(W_64, 16) exactly (ring and parked slices are fp64); the
     matrix-pipe form re-reads its slices as stored, there this holds for the diagonal blocks;
  4  the worst 64 x 64 block of W (relative Frobenius error against the long-double L^-1) is at most MARGIN[storage] = 16 / 4
     / 4 times the same figure of the fp64 restatement of the walk (ring: fp64 slices, mfma: re-read as stored);
  5  t = W r, y = W^T t and the slot sum t.t + sum(add0) against long double from W AS DOWNLOADED, to the dot-product bounds
     2 n 2^-53 |W| |r| etc. (nothing measured);
  6  Ainv == Ainv^T bit for bit, |Ainv - W^T W| <= 2^-24 |W^T W| + 2 n 2^-53 |W|^T |W| (long double, W as downloaded; at
     n = 2 048 on 128 whole rows - four of every 64, in both 16-row halves of both 32 x 32 tiles of the block row, so every
     tile of the triangle and, through the exact symmetry, its mirror image is read);
  7  the one-GEMV form: y = Ainv r and r.y + sum(add0), dot-product bounds, Ainv as downloaded;
  8  end to end: y against the long-double A^-1 r, relative L2 at most MARGIN times the restatement's.

Measured on an MI355X:
    case walk storage   worst block of W, device / restatement   y end to end, device / restatement
    a    ring   64      3.4e-15 / 2.4e-14                         1.7e-15 / 9.8e-15
    a    ring   32      2.6e-08 / 2.6e-08                         2.6e-08 / 2.6e-08
    a    ring   16      1.8e-03 / 1.8e-03                         1.6e-03 / 1.6e-03
    b    ring   64      3.4e-15 / 1.4e-14                         1.4e-15 / 4.2e-15
    b    ring   32      2.7e-08 / 2.7e-08                         2.8e-08 / 2.8e-08
    b    ring   16      1.7e-03 / 1.7e-03                         1.4e-03 / 1.4e-03
    c    ring   64      5.5e-15 / 2.7e-14                         2.6e-15 / 1.2e-14
    c    ring   32      2.9e-08 / 2.9e-08                         2.3e-08 / 2.3e-08
    c    ring   16      2.0e-03 / 2.0e-03                         1.6e-03 / 1.6e-03
    d    ring   64      5.8e-15 / 1.5e-13                         3.4e-15 / 2.8e-14
    d    ring   32      3.0e-08 / 3.0e-08                         2.2e-08 / 2.2e-08
    d    ring   16      1.9e-03 / 1.9e-03                         1.4e-03 / 1.4e-03
    e    mfma   64      6.2e-15 / 1.4e-13                         3.4e-15 / 3.3e-14
    e    mfma   32      7.3e-08 / 7.3e-08                         4.8e-08 / 4.8e-08
    e    mfma   16      4.8e-03 / 4.8e-03                         3.0e-03 / 3.0e-03
    f    ring   16      2.0e-03 / 2.0e-03                         1.4e-03 / 1.4e-03
(in fp32 and bfloat16 the stored rounding is all there is: device and restatement agree to four digits; in fp64 the device is
the closer of the two).  Every schedule gave the same W bit for bit; the ring form's W_32 and W_16 had 0 entries off the
rounded W_64, the matrix-pipe form's ~220 000, half of the triangle (diagonal blocks equal); the GEMVs and slot sums used at most
7.1e-3 of their dot-product bounds, the explicit inverse up to 1.000 of its bound (the fp32 rounding term is sharp).
tests/test_dense_reference_host.py shows that each planted defect of the oracle moves the figure of item 4 by at least ten
times its bound.  Every test prints its figures (pytest -s) before it asserts."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense_oracle as D                                # noqa: E402

LD = np.longdouble
U = 2.0 ** -53
CASE_STORAGE = [(c, s) for c in D.CASES for s in D.STORAGES[c]]
ONE_GEMV = [(c, s) for c, s in CASE_STORAGE if s != 64]


def _schedules(name):
    """(trtri_rows, band_roundtrip); the first one is the assembly's."""
    if name == "f":
        return [(3, False)]
    return [(3, False), (0, False), (1, False)] + ([(3, True)] if name in "ac" else [])


@functools.lru_cache(maxsize=None)
def _run(name, storage, rows, band):
    from pylatticedso_amd import _capi
    c = D.case(name)
    out = _capi.debug_dense_level(c.A, c.r, c.bw, storage, trtri_rows=rows, band_roundtrip=band, add0=c.add0)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _main(name, storage):
    return _run(name, storage, *_schedules(name)[0])


@functools.lru_cache(maxsize=None)
def _applied(name, storage):
    """t* = W r, y* = W^T t* and their scales |W| |r|, |W|^T |t*| in long double, W as downloaded."""
    c = D.case(name)
    W = _main(name, storage)["W"].astype(LD)
    r = c.rp.astype(LD)
    t = W @ r
    return t, W.T @ t, np.abs(W) @ np.abs(r), np.abs(W).T @ np.abs(t)


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_structure_and_schedules(name, storage):
    """Items 1 and 2."""
    c = D.case(name)
    first = None
    for rows, band in _schedules(name):
        out = _run(name, storage, rows, band)
        W, Wt = out["W"], out["Wt"]
        same = first is None or np.array_equal(W, first)
        print(f"DENSE_SCHED case={name} form={c.form} storage={storage} rows={rows} band={int(band)} "
              f"ranges={len(D.ranges(c.nb, rows))} info={out['info'].tolist()} upper_nonzero={int(np.triu(W, 1).any())} "
              f"Wt_is_transpose={int(np.array_equal(Wt, W.T))} same_as_first={int(same)}")
        assert W.shape == (c.np, c.np) and out["info"].tolist() == [0, 0]
        assert not np.triu(W, 1).any()
        assert np.array_equal(Wt, W.T)
        assert np.isfinite(W).all()
        assert same, (rows, band, int((W != first).sum()))
        first = W if first is None else first
        assert out["one_gemv"] == (storage != 64 and c.np <= D.ONE_GEMV_MAX_DOFS)
    if c.np > c.n:                      # identity padding couples to nothing
        pad = np.arange(c.n, c.np)
        assert not first[pad][:, :c.n].any() and (np.diag(first)[pad] > 0).all()


@pytest.mark.parametrize("name", [c for c in D.CASES if 64 in D.STORAGES[c]])
def test_storage_is_one_rounding_of_the_fp64_walk(name):
    """Item 3."""
    c = D.case(name)
    W64 = _main(name, 64)["W"]
    for storage in (32, 16):
        W = _main(name, storage)["W"]
        want = D.round_storage(W64, storage)
        diag = all(np.array_equal(D._blk(W, k, k), D._blk(want, k, k)) for k in range(c.nb))
        moved = int((W != want).sum())
        print(f"DENSE_ROUND case={name} form={c.form} storage={storage} entries_off={moved} diagonal_blocks_equal={int(diag)}")
        assert diag
        if c.form == "ring":
            assert moved == 0
        else:
            assert moved > 0            # (re-read as stored: if this were equal the case would not be the matrix-pipe walk)


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_inverse_factor_against_long_double(name, storage):
    """Item 4."""
    c = D.case(name)
    err = D.block_errors(_main(name, storage)["W"], c.W)
    ref = c.figures(storage)[0]
    bound = c.bounds(storage)[0]
    i, k = np.unravel_index(np.argmax(err), err.shape)
    print(f"DENSE_W case={name} form={c.form} storage={storage} worst_block={err.max():.3e} at=({i},{k}) "
          f"restatement={ref:.3e} bound={bound:.3e}")
    assert err.max() <= bound


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_triangular_gemvs(name, storage):
    """Item 5, every schedule."""
    c = D.case(name)
    n = c.np
    t, y, st, sy = _applied(name, storage)
    q = t @ t + c.add0.astype(LD).sum()
    sq = np.abs(t) @ np.abs(t) + np.abs(c.add0).sum()
    for rows, band in _schedules(name):
        out = _run(name, storage, rows, band)
        dt, dy, dq = np.abs(out["t"] - t), np.abs(out["y"] - y), abs(out["quad"] - q)
        bt, by, bq = 2 * n * U * st, 2 * n * U * sy, 2 * n * U * sq
        print(f"DENSE_GEMV case={name} storage={storage} rows={rows} band={int(band)} "
              f"t={float((dt / np.where(bt > 0, bt, 1)).max()):.2e} y={float((dy / np.where(by > 0, by, 1)).max()):.2e} "
              f"quad={float(dq / bq):.2e} (fractions of the bounds)")
        assert (dt <= bt).all() and (dy <= by).all() and dq <= bq
        assert np.linalg.norm(out["t"]) > 0 and np.linalg.norm(out["y"]) > 0


@functools.lru_cache(maxsize=None)
def _gram(name, storage):
    """(rows or None, W^T W in long double, |W|^T |W|) from W as downloaded."""
    c = D.case(name)
    W = _main(name, storage)["W"]
    rows = None
    if c.np > 1024:
        rows = np.array([D.NB * b + o for b in range(c.nb) for o in ((5 * b) % 16, 16 + (7 * b + 3) % 16,
                                                                       32 + (11 * b + 6) % 16, 48 + (13 * b + 9) % 16)])
    G = D.gram_ld(W, rows)
    Wa = np.abs(W)
    Ga = Wa.T @ Wa if rows is None else Wa[:, rows].T @ Wa      # (the scale of a bound: fp64 is enough)
    return rows, G, Ga


@pytest.mark.parametrize("name,storage", ONE_GEMV)
def test_explicit_inverse(name, storage):
    """Item 6."""
    c = D.case(name)
    n = c.np
    out = _main(name, storage)
    assert out["one_gemv"]
    Ainv = out["Ainv"]
    assert Ainv.dtype == np.float32 and np.array_equal(Ainv, Ainv.T) and np.isfinite(Ainv).all()
    rows, G, Ga = _gram(name, storage)
    got = Ainv.astype(LD) if rows is None else Ainv[rows].astype(LD)
    bound = 2.0 ** -24 * np.abs(G) + 2 * n * U * Ga
    frac = np.abs(got - G) / np.where(bound > 0, bound, 1)
    print(f"DENSE_AINV case={name} storage={storage} rows_checked={n if rows is None else len(rows)} "
          f"worst={float(frac.max()):.3f} of the bound, symmetric=1")
    assert (np.abs(got - G) <= bound).all()
    assert (np.diag(Ainv) > 0).all()


@pytest.mark.parametrize("name,storage", ONE_GEMV)
def test_one_gemv_form(name, storage):
    """Item 7."""
    c = D.case(name)
    n = c.np
    out = _main(name, storage)
    G, r = out["Ainv"].astype(LD), c.rp.astype(LD)
    y = G @ r
    sy = np.abs(G) @ np.abs(r)
    q = r @ y + c.add0.astype(LD).sum()
    sq = np.abs(r) @ np.abs(y) + np.abs(c.add0).sum()
    dy, dq = np.abs(out["y_one"] - y), abs(out["quad_one"] - q)
    by, bq = 2 * n * U * sy, 2 * n * U * sq
    print(f"DENSE_ONE case={name} storage={storage} y={float((dy / np.where(by > 0, by, 1)).max()):.2e} "
          f"quad={float(dq / bq):.2e} (fractions of the bounds)")
    assert (dy <= by).all() and dq <= bq
    assert np.linalg.norm(out["y_one"]) > 0


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_end_to_end_against_long_double(name, storage):
    """Item 8."""
    c = D.case(name)
    out = _main(name, storage)
    dev = D.rel_l2(out["y"], c.y)
    ref, bound = c.figures(storage)[1], c.bounds(storage)[1]
    print(f"DENSE_Y case={name} form={c.form} storage={storage} y={dev:.3e} restatement={ref:.3e} bound={bound:.3e}")
    assert dev <= bound
