"""Host reference of the dense coarse level (csrc/pl_dense.h, the explicit inverse of csrc/pl_small.h): plain numpy.

What tests/test_gpu_dense_level.py holds the device to, and what tests/test_dense_reference_host.py holds this file to:

  * banded_spd(nb, bw, seed): the test matrix.  A = G G^T + 0.05 I with G block lower triangular of block bandwidth bw
    (64 x 64 blocks; diagonal blocks N(0, 1/64), the others 0.35 times that), then D A D with D = 10^3 on dofs 3, 4, 5 of
    every six - the spread between translational and rotational modes of a coarse operator.  Blocks outside the band are
    exactly zero, the band-edge block of L has 0.24 ... 0.32 of the diagonal block's norm, cond(A) = 6e7 ... 1e8.
  * truth(): Cholesky factor L, W = L^-1 and A^-1 r in np.longdouble (column-wise, band-aware: the zeros stay zeros).
  * the RESTATEMENT of what the device computes, in fp64: block_cholesky() (right-looking over 64 x 64 blocks, the fill kept
    inside the band, L_ik = A_ik Dinv_k^T with the explicit inverse of the diagonal block) and walk(), the block recurrence
        W_kk = Dinv_k ,   W_ik = -Dinv_i  sum_{j = max(k, i - bw)}^{i-1}  L_ij W_jk
    with the slices W_jk either kept in fp64 (the LDS-ring form: `ring`) or re-read as stored (the matrix-pipe form: `mfma`),
    and round_storage(x, 64 | 32 | 16) - 16 = fp32, then round-to-nearest-even on the upper 16 bits.
    Its own distance to the truth is the yardstick of the GPU test: the device, which sums in another order, may be
    MARGIN[storage] times as far from the truth as the restatement and no further.
  * planted defects (DEFECTS), each one thing a kernel could get wrong while every PCG solve still converges.
"""
from __future__ import annotations

import functools

import numpy as np

NB = 64                      # block size (kNB)
K_RING = 12                  # slices the LDS ring holds (kRing): the ring form runs while bw + 1 <= K_RING
ONE_GEMV_MAX_DOFS = 2048     # levels up to this size also get the explicit inverse (kOneGemvMaxDofs)
SLOTS = 64                   # a slotted scalar (kSlots)
LD = np.longdouble

# The device may be this many times as far from the long-double truth as the restatement is.  Storage 64: the sums of the
# device run in another order and its diagonal blocks are inverted by another algorithm; 32 / 16: the rounding of the stored
# value dominates both, only ties and near-ties can fall the other way.
MARGIN = {64: 16.0, 32: 4.0, 16: 4.0}
FLOOR_FACTOR = 10.0          # every planted defect moves a measured quantity by at least this many times its bound
DEFECTS = ("jlo", "ring_lap", "parked", "chain_edge", "bf16_truncate")

# name: (nb, bw, n, seed).  The smallest shapes at which each path of the level can go wrong (tests/test_gpu_dense_level.py).
CASES = {"a": (5, 2, 320, 11), "b": (5, 2, 300, 12), "c": (16, 5, 1024, 13), "d": (14, 11, 896, 14),
         "e": (15, 12, 960, 15), "f": (32, 6, 2048, 16)}
STORAGES = {"a": (64, 32, 16), "b": (64, 32, 16), "c": (64, 32, 16), "d": (64, 32, 16), "e": (64, 32, 16), "f": (16,)}


def form_of(nb, bw):
    """Which walk dense_factor_inverse launches."""
    bw = bw if 0 < bw <= nb else nb
    return "ring" if bw + 1 <= K_RING else "mfma"


def ranges(nb, rows):
    """Row ranges [row0, row1) of the inverse factor as dense_factor_inverse cuts them: a range is launched behind link k of
    the chain once `rows` block rows are final and at least rows / 2 are left for the last one."""
    out, done = [], 0
    if rows > 0:
        for k in range(nb - 1):
            if k + 2 < nb and k + 2 - done >= rows and nb - (k + 2) >= rows // 2:
                out.append((done, k + 2))
                done = k + 2
    return out + [(done, nb)]


def banded_spd(nb, bw, seed):
    rng = np.random.default_rng(seed)
    n = nb * NB
    G = np.zeros((n, n))
    for i in range(nb):
        for j in range(max(0, i - bw), i + 1):
            blk = rng.standard_normal((NB, NB)) / 8.0
            G[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB] = blk if i == j else 0.35 * blk
    A = G @ G.T + 0.05 * np.eye(n)
    d = np.where(np.arange(n) % 6 >= 3, 1.0e3, 1.0)
    A = A * d[:, None] * d[None, :]
    return np.tril(A) + np.tril(A, -1).T                       # exactly symmetric


def padded(A):
    """To the next multiple of 64 with an identity diagonal, as the library pads."""
    n = len(A)
    m = (n + NB - 1) // NB * NB
    out = np.eye(m)
    out[:n, :n] = A
    return out


def round_storage(x, bits, truncate=False):
    """x (float64) as the inverse factor stores it, widened back to float64 exactly."""
    x = np.asarray(x, np.float64)
    if bits == 64:
        return x.copy()
    f = x.astype(np.float32)
    if bits == 32:
        return f.astype(np.float64)
    assert bits == 16
    u = f.view(np.uint32)
    if truncate:
        u = u & np.uint32(0xFFFF0000)
    else:
        u = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return u.view(np.float32).astype(np.float64)


# ---- the truth ------------------------------------------------------------------------------------------------------------
def truth(Ap, bw):
    """(L, W = L^-1) of the padded matrix in long double; bw = block bandwidth (entries outside it are never touched)."""
    n = len(Ap)
    A = Ap.astype(LD)
    L = np.zeros((n, n), LD)
    lo_of = [max(0, (j // NB - bw) * NB) for j in range(n)]
    for j in range(n):
        lo, hi = lo_of[j], min(n, (j // NB + bw + 1) * NB)
        c = A[j:hi, j] - L[j:hi, lo:j] @ L[j, lo:j]
        L[j, j] = np.sqrt(c[0])
        L[j + 1:hi, j] = c[1:] / L[j, j]
    W = np.zeros((n, n), LD)
    for i in range(n):
        lo = lo_of[i]
        W[i, :i] = -(L[i, lo:i] @ W[lo:i, :i]) / L[i, i]
        W[i, i] = LD(1) / L[i, i]
    return L, W


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _blk(M, i, j):
    return M[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]


def block_cholesky(Ap, bw, defect=None):
    """Blocked right-looking Cholesky in fp64 as the chain of k_chol_step runs it.  Returns (L, [Dinv_k])."""
    n = len(Ap)
    nb = n // NB
    bw = bw if 0 < bw <= nb else nb
    A = np.tril(Ap)
    L = np.zeros((n, n))
    Dinv = []
    for k in range(nb):
        Lkk = np.linalg.cholesky(_blk(A, k, k) + np.tril(_blk(A, k, k), -1).T)
        _blk(L, k, k)[:] = Lkk
        Dinv.append(np.tril(np.linalg.solve(Lkk, np.eye(NB))))
        rest = min(nb - k - 1, bw)
        for i in range(k + 1, k + 1 + rest):
            _blk(L, i, k)[:] = _blk(A, i, k) @ Dinv[k].T
        for i in range(k + 1, k + 1 + rest):
            if defect == "chain_edge" and i == k + bw:          # the band-edge row of the trailing update left out
                continue
            for j in range(k + 1, i + 1):
                _blk(A, i, j)[:] -= _blk(L, i, k) @ _blk(L, j, k).T
    return L, Dinv


def walk(L, Dinv, bw, storage, form, defect=None, rows=0, Ap=None):
    """The inverse factor as stored (widened to float64), by the block recurrence.  form = 'ring': the slices of the sum
    are the fp64 values; 'mfma': they are re-read as stored.  `rows` and `Ap` matter to the defect 'parked' alone (the
    result of a correct walk does not depend on where it was cut)."""
    n = len(L)
    nb = n // NB
    bw = bw if 0 < bw <= nb else nb
    trunc = defect == "bf16_truncate"
    Ws = np.zeros((n, n))
    starts = {r0 for r0, _ in ranges(nb, rows) if r0 > 0}
    for k in range(nb):
        Wd = {k: Dinv[k]}
        _blk(Ws, k, k)[:] = round_storage(Dinv[k], storage, trunc)
        for i in range(k + 1, nb):
            jlo = max(k, i - bw + (1 if defect == "jlo" else 0))
            acc = np.zeros((NB, NB))
            for j in range(jlo, i):
                src = j
                if defect == "ring_lap" and form == "ring" and j - K_RING >= k:
                    src = j - K_RING                             # the slot still holds the slice of the lap before
                w = Wd[src] if form == "ring" else _blk(Ws, src, k)
                if defect == "parked" and form == "ring" and i in starts and j == i - bw and j > k:
                    w = _blk(Ap, j, k)                           # never parked: the range reads what the matrix held there
                acc += _blk(L, i, j) @ w
            o = -(Dinv[i] @ acc)
            Wd[i] = o
            _blk(Ws, i, k)[:] = round_storage(o, storage, trunc)
    return Ws


# ---- measures -------------------------------------------------------------------------------------------------------------
def block_errors(W, Wtrue):
    """(nb, nb): relative Frobenius error of every 64 x 64 block of the lower triangle against the truth (0 above it)."""
    nb = len(W) // NB
    d = (np.asarray(W, LD) - Wtrue) ** 2
    t = Wtrue ** 2
    d = d.reshape(nb, NB, nb, NB).sum(axis=(1, 3))
    t = t.reshape(nb, NB, nb, NB).sum(axis=(1, 3))
    out = np.zeros((nb, nb))
    lower = np.tril(np.ones((nb, nb), bool))
    out[lower] = np.sqrt((d[lower] / t[lower]).astype(np.float64))
    return out


def apply_ld(W, r):
    """(t, y) = (W r, W^T t) in long double."""
    W = np.asarray(W, LD)
    t = W @ np.asarray(r, LD)
    return t, W.T @ t


def rel_l2(x, ref):
    x, ref = np.asarray(x, LD), np.asarray(ref, LD)
    return float(np.sqrt(((x - ref) ** 2).sum() / (ref ** 2).sum()))


def gram_ld(W, rows=None):
    """W^T W in long double, rows `rows` of it (all by default).  W is lower triangular: entry (a, b) sums over
    k >= max(a, b) only, so the product is taken block column by block column."""
    n = len(W)
    Wl = np.asarray(W, LD)
    if rows is not None:
        rows = np.asarray(rows)
        out = np.zeros((len(rows), n), LD)
        for b0 in np.unique(rows // NB * NB):                    # rows a of one block: k >= a >= b0
            sel = np.flatnonzero(rows // NB * NB == b0)
            out[sel] = Wl[b0:, rows[sel]].T @ Wl[b0:]
        return out
    G = np.zeros((n, n), LD)
    for b0 in range(0, n, NB):                                   # columns [b0, b0 + NB), rows a >= b0: k >= a >= b0
        G[b0:, b0:b0 + NB] = Wl[b0:, b0:].T @ Wl[b0:, b0:b0 + NB]
    iu = np.triu_indices(n, 1)
    G[iu] = G.T[iu]
    return G


# ---- the cases, computed once -----------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name):
        self.name = name
        self.nb, self.bw, self.n, seed = CASES[name]
        self.form = form_of(self.nb, self.bw)
        self.A = np.ascontiguousarray(banded_spd(self.nb, self.bw, seed)[:self.n, :self.n])
        self.Ap = padded(self.A)
        self.np = len(self.Ap)
        rng = np.random.default_rng(1000 + seed)
        self.r = rng.standard_normal(self.n)
        self.rp = np.r_[self.r, np.zeros(self.np - self.n)]
        self.add0 = rng.standard_normal(SLOTS)
        self.L, self.W = truth(self.Ap, self.bw)
        self.t, self.y = apply_ld(self.W, self.rp)

    @functools.lru_cache(maxsize=None)
    def factor(self, defect=None):
        return block_cholesky(self.Ap, self.bw, defect if defect == "chain_edge" else None)

    @functools.lru_cache(maxsize=None)
    def restated(self, storage, defect=None, rows=3):
        L, Dinv = self.factor(defect)
        W = walk(L, Dinv, self.bw, storage, self.form, defect, rows, self.Ap)
        W.setflags(write=False)
        return W

    @functools.lru_cache(maxsize=None)
    def figures(self, storage, defect=None, rows=3):
        """(worst block error of W, relative L2 error of y = W^T W r) of the restatement against the truth; (inf, inf)
        where a defect leaves a pivot that is not positive (the device then reports info != 0)."""
        try:
            W = self.restated(storage, defect, rows)
        except np.linalg.LinAlgError:
            return float("inf"), float("inf")
        return float(block_errors(W, self.W).max()), rel_l2(apply_ld(W, self.rp)[1], self.y)

    def bounds(self, storage):
        """What the GPU test allows the device: (worst block error of W, relative L2 error of y)."""
        w, y = self.figures(storage)
        return MARGIN[storage] * w, MARGIN[storage] * y


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
