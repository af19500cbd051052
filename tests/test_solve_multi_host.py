"""Host side of the multi-column solver (no GPU): header / EXPORTS / argtypes of the three entry points, the shape checks of
HipLattice.spmv_multi / solve_multi, and the host plumbing of the two opt-in callers - the batched homogenisation and the
paired adjoint - against a stub device whose spmv_multi / solve_multi are numpy on the oracle's K."""
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import timoshenko_oracle as O
from pylatticedso_amd import _capi
from pylatticedso_amd.homogenization_cell import HomogenizedCell
from pylatticedso_amd.lattice_opti import LatticeOpti
from pylatticedso_amd.lattice_sim import LatticeSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NU = 1013.0, 0.3
NAMES = ("pl_spmv_multi", "pl_solve_multi", "pl_schur_block")


def test_header_exports_and_argtypes_agree():
    text = open(os.path.join(ROOT, "include", "pylattice_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+PL_MULTI_MAX\s+(\d+)", text).group(1) == str(_capi.MULTI_MAX)
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.load_library()
    for name in NAMES:
        assert name in _capi.EXPORTS
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert proto, name
        params = [p.strip() for p in proto.group(1).split(",")]
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            if "*" in p or p.startswith("pl_handle"):
                assert t is _capi.C.c_void_p, (name, p)
            elif p.startswith("double"):
                assert t is _capi.C.c_double, (name, p)
            else:
                assert t is _capi.C.c_int32, (name, p)


def test_shapes_are_rejected_before_the_library_is_touched():
    dev = _capi.HipLattice.__new__(_capi.HipLattice)
    dev.n_nodes, dev._lib, dev._h = 5, None, None                # any call into the library would raise AttributeError
    for bad in (np.zeros((2, 5, 5)), np.zeros((2, 31)), np.zeros((0, 5, 6)), np.zeros((_capi.MULTI_MAX + 1, 30)),
                np.zeros((2, 2, 5, 6))):
        with pytest.raises(ValueError):
            dev.spmv_multi(bad)
        with pytest.raises(ValueError):
            dev.solve_multi(None, bad)
        with pytest.raises(ValueError):
            dev.solve_multi(bad, None)
    with pytest.raises(ValueError):
        dev.solve_multi(None, None)
    with pytest.raises(ValueError):
        dev.solve_multi(np.zeros((2, 5, 6)), np.zeros((3, 5, 6)))       # column counts differ
    assert dev._columns("x", np.zeros((5, 6))).shape == (1, 30) and dev._columns("x", np.zeros((3, 30))).shape == (3, 30)


class StubDevice:
    """What HomogenizedCell / LatticeOpti ask of a HipLattice, in numpy on a dense K."""

    def __init__(self, K):
        self.K = K
        self.n_nodes = K.shape[0] // 6
        self.master = None
        self.fixed = np.zeros((self.n_nodes, 6), bool)
        self.calls = {"solve": 0, "solve_multi": 0, "spmv": 0, "spmv_multi": 0}

    def set_bc(self, fixed, ubar=None, f=None):
        self.fixed = np.asarray(fixed, bool).reshape(self.n_nodes, 6).copy()

    def assemble(self):
        pass

    def assemble_bsr(self, with_bc=False):
        pass

    def get_bsr(self):
        B = sp.bsr_matrix(sp.csr_matrix(self.K), blocksize=(6, 6))
        B.sort_indices()
        return B.indptr.astype(np.int64), B.indices.astype(np.int32), B.data

    def set_periodic(self, master):
        self.master = None if master is None else np.asarray(master)

    def spmv(self, x):
        self.calls["spmv"] += 1
        return (self.K @ np.asarray(x).ravel()).reshape(-1, 6)

    def spmv_multi(self, X, masked=False):
        self.calls["spmv_multi"] += 1
        X = np.asarray(X).reshape(len(X), -1)
        return (self.K @ X.T).T.reshape(len(X), -1, 6)

    def solve(self, *a, **kw):
        self.calls["solve"] += 1
        raise AssertionError("the batched paths must not call solve()")

    def solve_multi(self, ubar=None, f=None, rtol=1e-8, max_iter=20000, raise_on_noconv=True):
        self.calls["solve_multi"] += 1
        k = len(ubar if ubar is not None else f)
        n6 = 6 * self.n_nodes
        ub = np.zeros((k, n6)) if ubar is None else np.asarray(ubar).reshape(k, n6)
        ff = np.zeros((k, n6)) if f is None else np.asarray(f).reshape(k, n6)
        fx = self.fixed.ravel()
        U = np.zeros((k, n6))
        if self.master is None:
            Kff = self.K[np.ix_(~fx, ~fx)]
            for j in range(k):
                u = np.where(fx, ub[j], 0.0)
                u[~fx] = np.linalg.solve(Kff, (ff[j] - self.K @ u)[~fx])
                U[j] = u
        else:      # periodic groups share their dofs: reduce to the masters, drop the fixed ones
            masters = np.unique(self.master)
            slot = np.full(self.n_nodes, -1)
            slot[masters] = np.arange(len(masters))
            cols = (6 * slot[self.master][:, None] + np.arange(6)).ravel()
            P = sp.csr_matrix((np.ones(n6), (np.arange(n6), cols)), shape=(n6, 6 * len(masters)))
            Kr = (P.T @ sp.csr_matrix(self.K) @ P).toarray()
            free = np.flatnonzero((P.T @ fx.astype(float)) == 0)
            for j in range(k):
                ur = np.zeros(Kr.shape[0])
                ur[free] = np.linalg.solve(Kr[np.ix_(free, free)], (P.T @ ff[j])[free])
                U[j] = P @ ur
        stats = [{"iterations": 1, "converged": 1} for _ in range(k)]
        return U.reshape(k, -1, 6), stats


def _oracle_K(L):
    lat, pen = L.lattice, L.penalized
    sc = np.array([O.condensed_beam(r, l, n, E, NU) for r, l, n in zip(lat.beam_radius, pen.seg_len, pen.seg_nsub)])
    return np.asarray(O.assemble_condensed(lat.node_xyz, lat.beam_conn, sc).todense())


@pytest.mark.parametrize("geoms,radii", [(["BCC"], [0.05]), (["Octet"], [0.04]), (["BCC", "Hybrid1"], [0.05, 0.03])])
def test_batched_homogenisation_plumbing(geoms, radii):
    """Column packing, anchor mask, group average and Voigt order of HomogenizedCell(batched=True) against the unbatched
    host path (solver="host"): matrix and fields to 1e-9."""
    preset = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                           "radii": radii, "geom_types": geoms},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": True}}
    L = LatticeSim(preset)
    K = _oracle_K(L)
    out = {}
    for mode in ("batched", "host"):
        dev = StubDevice(K)
        a = HomogenizedCell(L, device=dev, solver="device" if mode == "batched" else "host", batched=mode == "batched")
        a.prepare_simulation()
        a.apply_dirichlet_for_homogenization()
        a.periodic_boundary_condition()
        out[mode] = (a.solve_full_homogenization(), a.saveDataToExport, dev.calls, a.orthotropicMatrix)
    Hb, Hh = out["batched"][0], out["host"][0]
    assert out["batched"][2] == {"solve": 0, "solve_multi": 1, "spmv": 0, "spmv_multi": 2}
    assert np.linalg.norm(Hb - Hh) < 1e-9 * np.linalg.norm(Hh)
    assert np.linalg.norm(out["batched"][3] - out["host"][3]) < 1e-9 * np.linalg.norm(out["host"][3])
    for ub, uh in zip(out["batched"][1], out["host"][1]):
        assert ub.shape == uh.shape and np.linalg.norm(ub - uh) < 1e-9 * np.linalg.norm(uh)


def test_paired_adjoint_plumbing():
    """_paired_state_adjoints: column 0 is the equilibrium (prescribed values and loads), the others K_ff^-1 q with zero
    values on the constrained dofs."""
    preset = {"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 2, "y": 1, "z": 1},
                           "radii": [0.05], "geom_types": ["BCC"]},
              "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False}}
    L = LatticeSim(preset)
    K = _oracle_K(L)
    n = L.lattice.n_nodes
    rng = np.random.default_rng(8)
    fixed = np.zeros((n, 6), bool)
    fixed[L.lattice.node_xyz[:, 0] == 0.0] = True
    ubar = np.where(fixed, 1e-3 * rng.standard_normal((n, 6)), 0.0)
    f = np.where(fixed, 0.0, rng.standard_normal((n, 6)))
    qs = [rng.standard_normal((n, 6)), rng.standard_normal((n, 6))]
    dev = StubDevice(K)
    dev.set_bc(fixed)
    fake = types.SimpleNamespace(device_model=lambda: dev, _model=types.SimpleNamespace(_fixed=fixed, _ubar=ubar, _f=f))
    u, lams = LatticeOpti._paired_state_adjoints(fake, qs)
    assert dev.calls["solve_multi"] == 1 and len(lams) == 2
    fx = fixed.ravel()
    Kff = K[np.ix_(~fx, ~fx)]
    ref = ubar.ravel().copy()
    ref[~fx] = np.linalg.solve(Kff, (f.ravel() - K @ ubar.ravel())[~fx])
    assert np.linalg.norm(u.ravel() - ref) < 1e-9 * np.linalg.norm(ref)
    for lam, q in zip(lams, qs):
        assert not lam[fixed].any()
        ref = np.linalg.solve(Kff, q.ravel()[~fx])
        assert np.linalg.norm(lam.ravel()[~fx] - ref) < 1e-9 * np.linalg.norm(ref)
