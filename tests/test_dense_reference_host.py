"""The host reference of the dense level (oracle/dense_oracle.py) has to be worth comparing against before
tests/test_gpu_dense_level.py holds the device to it: the test matrices are what they claim to be (banded, a band edge that
counts, ill-conditioned), the fp64 restatement of the blocked factorisation and of the walk agrees with the long-double truth
to rounding, bfloat16 is rounded the way an independent implementation rounds it - and the comparison is SENSITIVE: under
every planted defect the quantity the GPU test measures moves by at least FLOOR_FACTOR = 10 times the bound the GPU test puts
on it.  No GPU.

The quantity is the worst 64 x 64 block of W (relative Frobenius error against the truth), bounded on the device by
MARGIN[storage] times the same figure of the restatement.  Two defects are judged otherwise, and say so when they print:
a band-edge row left out of the trailing update usually leaves a pivot that is not positive (the device reports info != 0,
which the GPU test asserts first; move = inf), and truncation instead of rounding to bfloat16 moves the block error by a
factor of two only - it is what the GPU test's EXACT comparison W_16 == round_storage(W_64, 16) is for (every block in the
ring form; the diagonal blocks, which do not depend on the storage type, in the matrix-pipe form), bound 0: any entry moved
is a failure there."""
import os
import re

import numpy as np
import pytest

from oracle import dense_oracle as D
from pylatticedso_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_STORAGE = [(c, s) for c in D.CASES for s in D.STORAGES[c]]


def test_dense_level_hook_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "pylattice_hip.h")).read()
    assert re.search(r"int pl_debug_dense_level\(int device, int32_t n, const double \*A, int32_t bw_blocks, int32_t storage, "
                     r"int32_t trtri_rows,\s+int32_t band_roundtrip, const double \*r, const double \*add0,", text)
    assert re.search(r"#define\s+PL_ABI_VERSION\s+6u", text)           # additive: no ABI bump
    assert "pl_debug_dense_level" in _capi.EXPORTS and callable(_capi.debug_dense_level)
    assert "pl_debug_spd_solve" in _capi.EXPORTS                       # the older hook stays
    assert D.SLOTS == 64 and D.NB == 64


def test_the_cases_reach_the_paths_they_are_named_for():
    forms = {c: D.form_of(*D.CASES[c][:2]) for c in D.CASES}
    assert forms == {"a": "ring", "b": "ring", "c": "ring", "d": "ring", "e": "mfma", "f": "ring"}
    assert D.ranges(5, 0) == [(0, 5)] and D.ranges(5, 3) == [(0, 3), (3, 5)]
    assert D.ranges(5, 1) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    for c, (nb, bw, n, _) in D.CASES.items():
        assert (n + 63) // 64 == nb and 2 <= bw < nb                   # banded: the truncations are active
        assert len(D.ranges(nb, 3)) >= 2 and len(D.ranges(nb, 1)) > len(D.ranges(nb, 3))
        r3 = D.ranges(nb, 3)
        assert r3[0][0] == 0 and r3[-1][1] == nb and all(a[1] == b[0] for a, b in zip(r3, r3[1:]))
    assert D.CASES["b"][2] % 64 != 0                                   # identity padding
    assert D.CASES["c"][0] > D.K_RING and D.CASES["f"][0] > D.K_RING   # the slot index wraps
    assert D.CASES["d"][1] + 1 == D.K_RING and D.CASES["e"][1] + 1 == D.K_RING + 1     # either side of the switch
    assert D.CASES["f"][2] == D.ONE_GEMV_MAX_DOFS
    # a later range of the ring form needs a parked slice that is not the diagonal one
    for c in "abcdf":
        nb, bw = D.CASES[c][:2]
        assert any(r0 - bw >= 1 for r0, _ in D.ranges(nb, 3)[1:]), c


@pytest.mark.parametrize("name", ["a", "c", "e"])
def test_test_matrix_is_banded_spd_with_a_band_edge_that_counts(name):
    c = D.case(name)
    nb, bw = c.nb, c.bw
    A = D.banded_spd(nb, bw, D.CASES[name][3])
    assert np.array_equal(A, A.T)
    for i in range(nb):
        for j in range(nb):
            if abs(i - j) > bw:
                assert not D._blk(A, i, j).any()
            else:
                assert D._blk(A, i, j).any()
    L = np.asarray(c.L, np.float64)
    edge = [np.linalg.norm(D._blk(L, k + bw, k)) / np.linalg.norm(D._blk(L, k, k)) for k in range(nb - bw)]
    cond = np.linalg.cond(c.Ap)
    print(f"DENSE_MATRIX case={name} band_edge_of_L={min(edge):.3f}..{max(edge):.3f} cond={cond:.2e}")
    assert min(edge) > 0.2 and cond > 3e7
    # the truth is a factorisation of the matrix, and banded like it
    V = np.random.default_rng(5).standard_normal((c.np, 4)).astype(D.LD)
    Ald = c.Ap.astype(D.LD)
    assert float(np.abs(c.L @ (c.L.T @ V) - Ald @ V).max() / np.abs(Ald @ V).max()) < 1e-17
    LV = c.L @ V
    assert float(np.abs(c.W @ LV - V).max() / np.abs(V).max()) < 1e-10     # (cond(L) ~ 1e4 at 2^-64)
    assert D.rel_l2(Ald @ c.y, c.rp) < 1e-10
    for i in range(nb):
        for j in range(nb):
            if i - j > bw or j > i:
                assert not D._blk(c.L, i, j).any()


def test_round_storage_rounds_to_nearest_even():
    import torch
    rng = np.random.default_rng(3)
    x = np.r_[rng.standard_normal(4096) * 10.0 ** rng.uniform(-12, 6, 4096), 0.0, -0.0,
              1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -30, 2.0 - 2.0 ** -9]
    want = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(D.round_storage(x, 16), want)
    assert D.round_storage(np.array([1.0 + 2.0 ** -8]), 16)[0] == 1.0              # tie: to even
    assert D.round_storage(np.array([1.0 + 3 * 2.0 ** -8]), 16)[0] == 1.0 + 2.0 ** -6
    assert D.round_storage(np.array([1.0 + 3 * 2.0 ** -8]), 16, truncate=True)[0] == 1.0 + 2.0 ** -7
    assert np.array_equal(D.round_storage(x, 32), x.astype(np.float32).astype(np.float64))
    assert np.array_equal(D.round_storage(x, 64), x)


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_restatement_against_the_long_double_truth(name, storage):
    c = D.case(name)
    w, y = c.figures(storage)
    print(f"DENSE_REF case={name} form={c.form} storage={storage} worst_block={w:.3e} y={y:.3e}")
    W = c.restated(storage)
    assert not np.triu(W, 1).any()
    assert c.figures(64)[0] < 1e-12
    unit = {64: 0.0, 32: 2.0 ** -24, 16: 2.0 ** -8}[storage]        # unit roundoff: 24 and 8 significant bits
    if c.form == "ring":        # the slices of the sums are fp64: what is stored is one rounding away from the fp64 walk
        assert w <= unit * (1.0 + 2.0 ** -23) + 1e-12
        if storage != 64:
            assert np.array_equal(W, D.round_storage(c.restated(64), storage))
    else:                       # re-read as stored: the roundings travel down the column
        assert w <= 4.0 * unit + 1e-12
        if storage != 64:
            assert not np.array_equal(W, D.round_storage(c.restated(64), storage))
            nb = c.nb
            for k in range(nb):
                assert np.array_equal(D._blk(W, k, k), D.round_storage(D._blk(c.restated(64), k, k), storage))
    # where the walk is cut is no part of a correct result
    if name in "ae":
        assert np.array_equal(c.restated(storage, None, 0), c.restated(storage, None, 3))


def _applies(defect, c):
    if defect in ("jlo", "chain_edge"):
        return True
    if defect == "ring_lap":
        return c.form == "ring" and c.nb > D.K_RING
    if defect == "parked":
        return c.form == "ring"
    return False


@pytest.mark.parametrize("name,storage", CASE_STORAGE)
def test_sensitivity_floor(name, storage):
    """Every planted defect moves the worst block of W by at least FLOOR_FACTOR times what the GPU test allows it."""
    c = D.case(name)
    good = c.figures(storage)[0]
    bound = c.bounds(storage)[0]
    seen = 0
    for defect in D.DEFECTS:
        if not _applies(defect, c):
            continue
        move = c.figures(storage, defect)[0] - good
        print(f"DENSE_FLOOR case={name} form={c.form} storage={storage} defect={defect} move={move:.3e} bound={bound:.3e} "
              f"ratio={move / bound:.3e}" + (" (pivot not positive: info != 0)" if np.isinf(move) else ""))
        assert move >= D.FLOOR_FACTOR * bound, (defect, move, bound)
        seen += 1
    assert seen >= (4 if c.form == "ring" and c.nb > D.K_RING else 3 if c.form == "ring" else 2)
    if storage == 16:           # truncation: judged by the exact comparison (bound 0), see the module docstring
        W = c.restated(16)
        Wt = c.restated(16, "bf16_truncate")
        if c.form == "ring":
            moved = int((Wt != D.round_storage(c.restated(64), 16)).sum())
        else:
            moved = sum(int((D._blk(Wt, k, k) != D._blk(W, k, k)).sum()) for k in range(c.nb))
        print(f"DENSE_FLOOR case={name} form={c.form} storage=16 defect=bf16_truncate entries_moved={moved} bound=0 (exact)")
        assert moved > 1000
