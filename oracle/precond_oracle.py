"""Dense numpy restatement of the PCG preconditioners of libpylattice_hip, and of the first PCG iterates under them.

Test infrastructure only (tests/test_precond_reference_host.py, tests/test_gpu_precond.py).  CG reaches the right
displacements with ANY symmetric positive definite preconditioner, so a converged solve says nothing about M^-1; the
iterates after one, two and three iterations do (x_1 = alpha_0 M^-1 b).  This module computes them in fp64 from the
definition the library states for itself (csrc/pl_coarse.h, DESIGN.md section 7, csrc/pl_ddm.h):

    M^-1 = D^-1 + sum_t Z_t (Z_t^T A Z_t)^-1 Z_t^T + Z (Z^T A Z)^-1 Z^T ,   A = P K P

* K: the assembled stiffness of the condensed struts (timoshenko_oracle.assemble_condensed); P projects on the free dofs.
* D = diag(K) on the free dofs (Jacobi level; precond = 1 is this level alone).
* Z (dense level, precond >= 2): per AGGREGATE of nodes the six rigid-body modes about a reference point c
  (u = U + W x (x - c), theta = W) or, with coarse_modes = 12, those plus the six uniform strains (u = eps (x - c),
  theta = 0; order xx, yy, zz, xy, yz, xz with the engineering halves of pl_coarse.h strain_disp), restricted to the
  aggregate's nodes and to the free dofs.
* Z_t (tile level, precond = 3): the same 6 or 12 (tile_modes) modes per K*p TILE.
  Which node lies in which tile / aggregate is the library's own partition (HipLattice.partition()), never re-derived.

The span of the modes does not depend on the reference point, so a full-rank block gives the same operator for any c; the
library uses the centre of the aggregate's box of bricks, this module the mean of the aggregate's nodes.

Rank-deficient blocks, as the library treats them:
* tile block, 6 modes (pl_coarse.h spd6_inverse): Cholesky in mode order; a mode whose pivot is not above 1e-12 of the largest
  diagonal entry is dropped, the block's inverse is the inverse of the kept principal sub-matrix, zero elsewhere.
* tile block, 12 modes (k_tile_invert12): the same sweep, a mode is dropped when its pivot is not above 1e-10 of its OWN
  diagonal entry (or that entry is not positive).
  Both are Z_k (Z_k^T A Z_k)^-1 Z_k^T on the kept modes k: symmetric positive semi-definite.  Where the kept modes span what
  all modes span (a tile with one free node: the rigid modes span its six dofs, every strain mode is dropped) the result
  is again independent of the reference point (Levels(centre_shift=...) lets the host test measure that).
* dense level (k_coarse_regularize): a mode with an exactly zero diagonal entry (no free support) becomes an identity
  row / column - its prolongation is zero, so it drops out; any other deficiency makes the Cholesky factorisation fail and
  the library falls back to Jacobi (pl_stats_t.precond_used = 1, which the tests assert).  Restated as the inverse on the
  span of the modes (span_inverse).

Node elimination (opts.condense, csrc/pl_coarse.h k_node_block_inverse ..., csrc/pl_solver.h pcg_solve): CG runs on the
Schur complement S = A_kk - A_ke A_ee^-1 A_ek of the kept nodes k (e: eliminated, an independent set without Dirichlet
dofs) with b' = b_k - A_ke A_ee^-1 b_e.  The levels are NOT rebuilt for S: D stays diag(K), the tile blocks and the dense
operator stay Z^T A Z of the FULL operator A with the modes on all nodes (eliminated ones included; build_coarse_level
takes the Dirichlet mask, not the elimination mask), and the vector kernels skip the eliminated rows in the restriction
and in the prolongation.  So the preconditioner of the condensed CG is the kept-rows principal block of the ordinary one,
M_c^-1 = (M^-1)_kk.  pl_solve returns the iterate on the kept nodes and x_e = A_ee^-1 (b_e - A_ek x_k) on the others.

DDM handles (csrc/pl_ddm.h), G = sum_c B_c^T S_c B_c: precond = 2 is (P G P)^-1, precond = 3 the inverted 6 x 6 node
blocks of G (constrained dofs taken out of the block first), precond = 4 the node blocks plus Z A_c^-1 Z^T with twelve
modes per aggregate.  precond = 5 of a strut handle is (P K P)^-1: the first iterate is the solution.

Planted defects (``Levels(defect=...)``) model mistakes the library could make without any converged solve noticing; the
host test measures how far they move the iterates (the sensitivity floor the GPU tolerance is held against).
"""
from __future__ import annotations

import numpy as np

from . import timoshenko_oracle as O

# Bounds on the relative L2 deviation of the device iterates (u_1, u_2, u_3) from this module's, per group of solver forms:
# ten times the largest deviation measured on an MI355X (tests/test_gpu_precond.py lists the measurements), to allow for
# the order of the atomic sums.  Per iterate: rounding accumulates with k, and so does what a defect does.  Each is held to
# a tenth of the sensitivity floor of the same iterate by tests/test_precond_reference_host.py.
GPU_TOL = {"fp64": (4.2e-7, 3.9e-7, 1.5e-6), "fp32": (5.2e-7, 8.1e-7, 8.8e-7), "jacobi": (3.9e-14, 4.3e-14, 4.7e-14)}
FLOOR_FACTOR = 10.0


def mode_matrix(xyz, nodes, centre, n_modes):
    """Z [6 N, n_modes]: the rigid-body (and uniform-strain) modes of ``nodes`` about ``centre``, zero on other nodes."""
    Z = np.zeros((6 * len(xyz), n_modes))
    for i in nodes:
        rx, ry, rz = xyz[i] - centre
        u = np.zeros((3, n_modes))
        th = np.zeros((3, n_modes))
        u[0, 0] = u[1, 1] = u[2, 2] = 1.0
        u[:, 3] = [0.0, -rz, ry]          # e_x x r
        u[:, 4] = [rz, 0.0, -rx]
        u[:, 5] = [-ry, rx, 0.0]
        th[0, 3] = th[1, 4] = th[2, 5] = 1.0
        if n_modes == 12:
            u[:, 6] = [rx, 0.0, 0.0]
            u[:, 7] = [0.0, ry, 0.0]
            u[:, 8] = [0.0, 0.0, rz]
            u[:, 9] = [0.5 * ry, 0.5 * rx, 0.0]
            u[:, 10] = [0.0, 0.5 * rz, 0.5 * ry]
            u[:, 11] = [0.5 * rz, 0.0, 0.5 * rx]
        Z[6 * i:6 * i + 3] = u
        Z[6 * i + 3:6 * i + 6] = th
    return Z


def greedy_block_inverse(B, n_modes):
    """(Z_t^T A Z_t)^-1 as the library forms it for a tile block that may be rank-deficient (module docstring).
    Returns (inverse, kept mode indices)."""
    B = 0.5 * (B + B.T)
    n = len(B)
    dmax = max(0.0, float(np.max(np.diag(B)))) if n else 0.0
    kept = []
    for k in range(n):
        s = B[k, k]
        if kept:
            s = s - B[k, kept] @ np.linalg.solve(B[np.ix_(kept, kept)], B[kept, k])
        ok = s > 1e-12 * dmax if n_modes == 6 else (B[k, k] > 0.0 and s > 1e-10 * B[k, k])
        if ok:
            kept.append(k)
    inv = np.zeros_like(B)
    if kept:
        sub = np.linalg.inv(B[np.ix_(kept, kept)])
        inv[np.ix_(kept, kept)] = 0.5 * (sub + sub.T)
    return inv, kept


def span_inverse(Ac):
    """(Z^T A Z)^-1 of the dense level on the span of its modes.  The library's modes are independent wherever its
    factorisation succeeds (it drops the modes without free support, which have an exactly zero row, and falls back to
    Jacobi on any other deficiency: the tests assert pl_stats_t.precond_used); then this is the plain inverse.  About this
    module's reference points a mode can repeat another one on a degenerate support (an aggregate whose free nodes lie in
    one plane: a uniform strain across the plane is a multiple of the translation), so the inverse is taken on the span -
    the same operator, whatever the reference point."""
    w, V = np.linalg.eigh(Ac)
    keep = w > 1e-11 * max(float(w.max()), 0.0)
    return (V[:, keep] / w[keep]) @ V[:, keep].T


def _groups(ids):
    ids = np.asarray(ids)
    return [(int(g), np.flatnonzero(ids == g)) for g in np.unique(ids[ids >= 0])]


def strut_matrix(xyz, conn, scalars, struts):
    """Dense sum of the 12 x 12 matrices of the listed struts."""
    K = np.zeros((6 * len(xyz), 6 * len(xyz)))
    for b in struts:
        ia, ib = conn[b]
        dofs = np.r_[6 * ia + np.arange(6), 6 * ib + np.arange(6)]
        K[np.ix_(dofs, dofs)] += O.beam_matrix(scalars[b], xyz[ib] - xyz[ia])
    return K


class Levels:
    """M^-1 of one handle configuration as a dense [6 N, 6 N] matrix on all dofs (zero on fixed ones).

    K dense [6N, 6N]; fixed (N, 6) bool; part = HipLattice.partition(); precond 1 / 2 / 3; defect: None or
      ("agg_mode", aggregate, mode)   that mode left out of the dense level,
      ("tile_mode", tile, mode)       that mode left out of one tile block,
      ("roller_unmasked",)            the Galerkin blocks built as if the single fixed dofs of roller nodes (nodes with some
                                      but not all dofs fixed) were free - the mask forgotten in the assembly kernels,
      ("fix_list", struts)            the listed struts (inside one aggregate, touching a Dirichlet dof) left out of
                                      Z^T A Z of the dense level; ``fix_list_struts`` finds them.
    centre_shift moves every reference point (reference_point_invariance)."""

    def __init__(self, K, fixed, xyz, part, precond, tile_modes=6, coarse_modes=6, defect=None, centre_shift=None,
                 K_fix_list=None):
        self.xyz = np.asarray(xyz, float)
        N = len(self.xyz)
        self.fixed = np.asarray(fixed).reshape(N, 6) != 0
        free = ~self.fixed.ravel()
        K = np.asarray(K)
        self.free = free
        self.A = K * np.outer(free, free)
        d = np.diag(K)
        self.Dinv = np.where(free & (d != 0.0), 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
        self.precond = precond
        self.defect = defect or (None,)
        shift = np.zeros(3) if centre_shift is None else np.asarray(centre_shift, float)
        # the operator and the mask the Galerkin blocks are built with (they differ from A / free only under a defect)
        gfree = free.copy()
        if self.defect[0] == "roller_unmasked":
            roller = self.fixed.any(axis=1) & ~self.fixed.all(axis=1)
            gfree |= np.repeat(roller, 6)
        Ag = K * np.outer(gfree, gfree)
        self.terms = {"jacobi": np.diag(self.Dinv)}
        self.kept, self.tile_factors = {}, {}
        agg, tile = np.asarray(part["agg"]), np.asarray(part["tile"])
        cen = {a: self.xyz[nodes].mean(axis=0) + shift for a, nodes in _groups(agg)}
        if precond >= 3:
            T = np.zeros_like(self.A)
            for t, nodes in _groups(tile):
                a = int(agg[nodes[0]])
                assert (agg[nodes] == a).all(), "a tile lies in one aggregate"
                Zg = mode_matrix(self.xyz, nodes, cen[a], tile_modes)
                Z = Zg * free[:, None]
                Zg = Zg * gfree[:, None]
                cols = list(range(tile_modes))
                if self.defect[0] == "tile_mode" and self.defect[1] == t:
                    cols.remove(self.defect[2])
                Binv, kept = greedy_block_inverse(Zg[:, cols].T @ Ag @ Zg[:, cols], tile_modes)
                self.kept[t] = [cols[k] for k in kept]
                self.tile_factors[t] = (Z[:, cols], Binv, kept)
                T += Z[:, cols] @ Binv @ Z[:, cols].T
            self.terms["tile"] = T
        if precond >= 2:
            cols_Z, cols_G = [], []
            for a, nodes in _groups(agg):
                Zg = mode_matrix(self.xyz, nodes, cen[a], coarse_modes)
                for m in range(coarse_modes):
                    if self.defect[0] == "agg_mode" and self.defect[1:] == (a, m):
                        continue
                    cols_Z.append(Zg[:, m] * free)
                    cols_G.append(Zg[:, m] * gfree)
            Z, Zg = np.array(cols_Z).T, np.array(cols_G).T
            Ad = Ag
            if self.defect[0] == "fix_list":
                Ad = Ag - K_fix_list * np.outer(gfree, gfree)
            Ac = Zg.T @ Ad @ Zg
            self.Ac, self.Z = 0.5 * (Ac + Ac.T), Z
            self.terms["dense"] = Z @ span_inverse(self.Ac) @ Z.T
        M = sum(self.terms.values())
        self.M = 0.5 * (M + M.T)


def fix_list_struts(conn, fixed, agg):
    """Struts with both ends in one aggregate that touch a Dirichlet dof (Coarse::fix_list)."""
    fx = (np.asarray(fixed).reshape(-1, 6) != 0).any(axis=1)
    conn = np.asarray(conn)
    return [b for b, (ia, ib) in enumerate(conn) if agg[ia] == agg[ib] and (fx[ia] or fx[ib])]


def pcg_iterates(A, M, b, k):
    """x_1 ... x_k of preconditioned CG from x_0 = 0 on A x = b with z = M r (dense matrices)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = M @ r
    p = z.copy()
    rz = r @ z
    out = []
    for _ in range(k):
        Ap = A @ p
        pAp = p @ Ap
        alpha = rz / pAp if pAp != 0.0 else 0.0
        x = x + alpha * p
        r = r - alpha * Ap
        z = M @ r
        rz_new = r @ z
        beta = rz_new / rz if rz != 0.0 else 0.0
        p = z + beta * p
        rz = rz_new
        out.append(x.copy())
    return out


def solve_iterates(K, fixed, ubar, f, M, k, eliminated=None):
    """What pl_solve(max_iter = j) returns for j = 1 ... k, (N, 6) each: prescribed values on fixed dofs, the PCG iterate
    of A x = P (f - K ubar) on the others; with node elimination the iterate of the condensed system on the kept nodes and
    the back-substituted eliminated ones (module docstring).  M: dense [6N, 6N] preconditioner on all dofs."""
    K = np.asarray(K)
    fx = (np.asarray(fixed).reshape(-1) != 0)
    free = ~fx
    ub = np.where(fx, np.asarray(ubar, float).reshape(-1), 0.0)
    b = np.where(fx, 0.0, np.asarray(f, float).reshape(-1) - K @ ub)
    A = K * np.outer(free, free)
    n = len(b)
    if eliminated is None or not np.any(eliminated):
        its = pcg_iterates(A, M, b, k)
    else:
        e = np.repeat(np.asarray(eliminated, bool), 6)
        assert not (e & fx).any(), "an eliminated node carries no Dirichlet dof"
        kk = ~e
        Aee_inv = np.linalg.inv(A[np.ix_(e, e)])
        S = A[np.ix_(kk, kk)] - A[np.ix_(kk, e)] @ Aee_inv @ A[np.ix_(e, kk)]
        bk = b[kk] - A[np.ix_(kk, e)] @ (Aee_inv @ b[e])
        its = []
        for xk in pcg_iterates(S, M[np.ix_(kk, kk)], bk, k):
            x = np.zeros(n)
            x[kk] = xk
            x[e] = Aee_inv @ (b[e] - A[np.ix_(e, kk)] @ xk)
            its.append(x)
    return [np.where(fx, ub, x).reshape(-1, 6) for x in its]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------------------------------
# DDM handles
# ---------------------------------------------------------------------------------------------------------------------
def ddm_matrix(n_nodes, cell_nodes, S, cell_S):
    """G = sum_c B_c^T S_c B_c, dense [6 N, 6 N]."""
    G = np.zeros((6 * n_nodes, 6 * n_nodes))
    for c, nodes in enumerate(np.asarray(cell_nodes)):
        dofs = (6 * np.asarray(nodes)[:, None] + np.arange(6)[None, :]).ravel()
        G[np.ix_(dofs, dofs)] += S[cell_S[c]]
    return G


def ddm_minv(G, fixed, precond, xyz=None, agg=None):
    """M^-1 of a DDM handle: precond 2 (P G P)^-1, 3 inverted node blocks, 4 node blocks + twelve modes per aggregate."""
    fx = np.asarray(fixed).reshape(-1) != 0
    free = ~fx
    n = len(fx)
    A = G * np.outer(free, free)
    M = np.zeros_like(A)
    if precond == 2:
        idx = np.flatnonzero(free)
        M[np.ix_(idx, idx)] = np.linalg.inv(A[np.ix_(idx, idx)])
        return M
    for i in range(n // 6):
        d = np.arange(6 * i, 6 * i + 6)
        inv, _ = greedy_block_inverse(A[np.ix_(d, d)], 6)
        M[np.ix_(d, d)] = inv
    if precond == 4:
        xyz = np.asarray(xyz, float)
        cols = []
        for a, nodes in _groups(agg):
            Z = mode_matrix(xyz, nodes, xyz[nodes].mean(axis=0), 12)
            cols.extend((Z * free[:, None]).T)
        Z = np.array(cols).T
        Ac = Z.T @ A @ Z
        M = M + Z @ span_inverse(0.5 * (Ac + Ac.T)) @ Z.T
    return 0.5 * (M + M.T)
