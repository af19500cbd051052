"""ctypes binding of libpylattice_hip.so (C ABI: include/pylattice_hip.h).

There is NO CPU fallback: if the shared library is missing or no MI355X is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .timing import timing as _timing

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYLATTICE_HIP_LIB: load another build of the library (kernel experiments: tools/exp_variants.sh)
LIB_PATH = os.environ.get("PYLATTICE_HIP_LIB") or os.path.join(_HERE, "libpylattice_hip.so")

PL_OK, PL_ERR_ARG, PL_ERR_HIP, PL_ERR_STATE, PL_ERR_NOCONV, PL_ERR_NAN, PL_ERR_NODEVICE = 0, -1, -2, -3, -4, -5, -6

# every symbol include/pylattice_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = ["pl_default_opts", "pl_opts_size", "pl_stats_size", "pl_abi_version", "pl_last_error", "pl_version", "pl_lzone", "pl_create", "pl_create_ddm",
           "pl_ddm_set_preconditioner", "pl_ddm_set_geometry", "pl_ddm_update_matrices", "pl_destroy", "pl_set_bc", "pl_set_periodic",
           "pl_update_radii", "pl_set_multiplicity", "pl_update_segments", "pl_assemble", "pl_assemble_bsr", "pl_get_bsr", "pl_spmv",
           "pl_spmv_free", "pl_spmv_bsr", "pl_solve", "pl_reactions", "pl_sens", "pl_sens_gram", "pl_energy", "pl_node_mod", "pl_schur",
           "pl_stress", "pl_stress_pnorm", "pl_buckling", "pl_buckling_pnorm",
           "pl_set_thermal", "pl_thermal_load", "pl_thermal_sens",
           "pl_set_conduction", "pl_cond_spmv", "pl_cond_solve", "pl_cond_flux", "pl_cond_sens", "pl_thermal_load_adjoint",
           "pl_set_convection", "pl_cond_solve_adjoint", "pl_cond_film", "pl_temp_pnorm",
           "pl_set_heat_capacity", "pl_cond_transient",
           "pl_spmv_multi", "pl_solve_multi", "pl_schur_block", "pl_geom_spmv_multi", "pl_buckling_modes", "pl_buckling_modes_sens",
           "pl_set_mass", "pl_mass_spmv_multi", "pl_vibration_modes", "pl_vibration_modes_sens",
           "pl_dyn_spmv_multi", "pl_transient", "pl_transient_sens", "pl_harm_spmv", "pl_harmonic", "pl_harmonic_sens",
           "pl_schur_cells", "pl_cells_recover", "pl_get_records", "pl_debug_partition", "pl_time_kernel", "pl_algorithmic_bytes", "pl_node_words_info", "pl_forget_history", "pl_debug_spd_solve", "pl_debug_dense_level", "pl_dist_unique_id_bytes",
           "pl_dist_unique_id", "pl_dist_loopback_id", "pl_dist_abort", "pl_dist_init", "pl_dist_set_peers", "pl_generate_lattice", "pl_lattice_fetch",
           "pl_lattice_free", "pl_penalize", "pl_boundary_index", "pl_boundary_index_rows"]


class PlMesh(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("n_beams", C.c_int64), ("node_xyz", C.c_void_p),
                ("beam_conn", C.c_void_p), ("beam_radius", C.c_void_p), ("seg_len", C.c_void_p),
                ("seg_nsub", C.c_void_p)]


class PlOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
                ("young", C.c_double), ("poisson", C.c_double), ("kappa", C.c_double), ("pen_coef", C.c_double),
                ("device", C.c_int32), ("spmv_kernel", C.c_int32), ("precond", C.c_int32), ("reorder", C.c_int32),
                ("check_every", C.c_int32), ("lanes_per_node", C.c_int32),
                ("tile_nodes", C.c_int32), ("coarse_max_dofs", C.c_int32), ("palette", C.c_int32),
                ("local_max_dofs", C.c_int32), ("precision", C.c_int32), ("restart_every", C.c_int32),
                ("alpha_max", C.c_double), ("grid_lo", C.c_double * 3), ("grid_hi", C.c_double * 3),
                ("grid_nodes", C.c_int64), ("mintol", C.c_double), ("compact_records", C.c_int32),
                ("condense", C.c_int32), ("chol_persistent", C.c_int32), ("cg_form", C.c_int32),
                ("tile_modes", C.c_int32), ("coarse_modes", C.c_int32), ("overlap", C.c_int32),
                ("coarse_storage", C.c_int32), ("warm_start", C.c_int32), ("short_iteration", C.c_int32)]


class PlStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("reserved_i", C.c_int32), ("rel_residual", C.c_double),
                ("b_norm", C.c_double), ("ms_assembly", C.c_double), ("ms_solve", C.c_double),
                ("ms_spmv_avg", C.c_double), ("precond_used", C.c_double), ("restarts", C.c_double),
                ("precision_used", C.c_double), ("info", C.c_double), ("stop_reason", C.c_double),
                ("condensed_nodes", C.c_double), ("cg_form_used", C.c_double), ("kp_form", C.c_double),
                ("comm_world", C.c_double), ("comm_rank", C.c_double), ("short_iteration_used", C.c_double),
                ("reserved", C.c_double * 2)]


class PlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libpylattice_hip error {code}: {msg}")
        self.code = code


_lib = None


def load_library(path: str | None = None):
    """dlopen libpylattice_hip.so (built in-tree by pylatticedso_amd/csrc/Makefile or __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not found - build it with `make -C pylatticedso_amd/csrc` "
                                "(the HIP path has no CPU fallback)")
    lib = C.CDLL(p)
    lib.pl_last_error.restype = C.c_char_p
    lib.pl_version.restype = C.c_char_p
    lib.pl_destroy.restype = None
    for name in ("pl_opts_size", "pl_stats_size", "pl_abi_version"):
        getattr(lib, name).restype = C.c_uint32
    lib.pl_lattice_free.restype = None
    V, I32, I64, D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    sig = {"pl_default_opts": [V, C.c_uint32], "pl_opts_size": [], "pl_stats_size": [], "pl_abi_version": [], "pl_lzone": [I32, I64, I64, V, V, V, V], "pl_create": [V, V, V], "pl_create_ddm": [I64, I64, I32, V, I32, V, V, V, V],
           "pl_ddm_set_preconditioner": [V, I32, V, V], "pl_ddm_set_geometry": [V, V], "pl_ddm_update_matrices": [V, I32, V, V], "pl_destroy": [V], "pl_set_bc": [V, V, V, V], "pl_set_periodic": [V, V],
           "pl_update_radii": [V, V], "pl_set_multiplicity": [V, V], "pl_update_segments": [V, V, V], "pl_assemble": [V],
           "pl_assemble_bsr": [V, I32, V, V], "pl_get_bsr": [V, V, V, V], "pl_spmv": [V, V, V],
           "pl_spmv_free": [V, V, V], "pl_spmv_bsr": [V, V, V], "pl_solve": [V, D, I32, V, V],
           "pl_reactions": [V, V, V], "pl_sens": [V, V, V, V], "pl_sens_gram": [V, I32, V, V], "pl_energy": [V, V, V], "pl_node_mod": [V, V, V],
           "pl_stress": [V, V, I32, V, V], "pl_stress_pnorm": [V, V, I32, D, V, V, V, V],
           "pl_buckling": [V, V, I32, D, I32, V, V, V], "pl_buckling_pnorm": [V, V, I32, D, I32, D, V, V, V, V],
           "pl_set_thermal": [V, D, V, V], "pl_thermal_load": [V, V, V], "pl_thermal_sens": [V, V, V],
           "pl_set_conduction": [V, D, V], "pl_cond_spmv": [V, I32, V, V, V], "pl_cond_solve": [V, V, V, V, D, I32, V, V],
           "pl_cond_flux": [V, V, V], "pl_cond_sens": [V, V, V, V], "pl_thermal_load_adjoint": [V, V, V],
           "pl_set_convection": [V, D, V, D], "pl_cond_solve_adjoint": [V, V, V, D, I32, V, V], "pl_cond_film": [V, V, V, V], "pl_temp_pnorm": [V, V, V, D, D, V, V],
           "pl_set_heat_capacity": [V, D, V, V],
           "pl_cond_transient": [V, I32, D, D, V, V, V, I32, V, V, V, D, I32, I32, V, V, V, I32, V, V, V],
           "pl_schur": [V, V, I32, D, I32, V], "pl_spmv_multi": [V, I32, I32, V, V],
           "pl_solve_multi": [V, I32, V, V, D, I32, V, V], "pl_schur_block": [V, V, I32, D, I32, I32, V],
           "pl_geom_spmv_multi": [V, V, I32, I32, V, V],
           "pl_buckling_modes": [V, V, I32, I32, D, I32, D, I32, V, V, V, V, V],
           "pl_buckling_modes_sens": [V, V, I32, V, V, D, I32, V, V, V, V],
           "pl_set_mass": [V, D, I32, V], "pl_mass_spmv_multi": [V, I32, I32, V, V],
           "pl_vibration_modes": [V, I32, I32, D, I32, D, I32, V, V, V, V, V],
           "pl_vibration_modes_sens": [V, I32, V, V, V, V, V],
           "pl_dyn_spmv_multi": [V, D, D, I32, I32, V, V],
           "pl_transient": [V, I32, D, D, D, D, D, I32, V, V, V, V, D, I32, I32, V, V, V, I32, V, V, V],
           "pl_transient_sens": [V, I32, D, D, D, D, D, I32, V, V, V, V, V, V, D, I32, V, I32, D, V, V, V, V, V],
           "pl_harm_spmv": [V, I32, V, I32, V, V],
           "pl_harmonic": [V, I32, V, D, D, V, V, I32, V, D, I32, I32, V, V, V, V, V, V],
           "pl_harmonic_sens": [V, I32, V, D, D, V, V, V, V, I32, D, V, D, I32, I32, V, V, V, V, V, V],
           "pl_schur_cells": [V, I32, I32, I32, V, I32, V, V, V, V, V, V, V],
           "pl_cells_recover": [V, I32, I32, I32, V, I32, V, V, V, V, V, V, V, V, V, V, V],
           "pl_get_records": [V, V], "pl_debug_partition": [V, V, V, V, V], "pl_time_kernel": [V, I32, I32, V],
           "pl_algorithmic_bytes": [V, V], "pl_node_words_info": [V, V, V, V, V], "pl_forget_history": [V], "pl_debug_spd_solve": [I32, I32, V, V, V, V, I32],
           "pl_debug_dense_level": [I32, I32, V, I32, I32, I32, I32] + [V] * 12, "pl_dist_unique_id_bytes": [], "pl_dist_unique_id": [V], "pl_dist_loopback_id": [V], "pl_dist_abort": [V],
           "pl_dist_init": [V, I32, I32, V, V, V, I32, I32], "pl_dist_set_peers": [V, V],
           "pl_generate_lattice": [I64, V, V, V, I32, I32, V, V, V, V], "pl_lattice_fetch": [V] * 12,
           "pl_lattice_free": [V], "pl_penalize": [I64, V, V, V, D, V, V, V],
           "pl_boundary_index": [I64, V, V, I64, V, V, V, V, V, V],
           "pl_boundary_index_rows": [I64, V, V, I64, V, V, V, V, V, V]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
    # ABI handshake (include/pylattice_hip.h): this binding's struct layouts must be the library's
    if lib.pl_opts_size() != C.sizeof(PlOpts) or lib.pl_stats_size() != C.sizeof(PlStats):
        raise ImportError(f"{p}: pl_opts_t / pl_stats_t are {lib.pl_opts_size()} / {lib.pl_stats_size()} bytes in the "
                          f"library, {C.sizeof(PlOpts)} / {C.sizeof(PlStats)} in this binding (ABI version "
                          f"{lib.pl_abi_version()}): rebuild libpylattice_hip.so")
    _lib = lib
    return lib


def default_opts(lib=None) -> "PlOpts":
    """A pl_opts_t stamped by pl_default_opts (struct size + ABI version checked by the library)."""
    lib = lib or load_library()
    opts = PlOpts()
    _check(lib, lib.pl_default_opts(C.byref(opts), C.sizeof(PlOpts)))
    return opts


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def _check(lib, rc, allow=()):
    if rc != PL_OK and rc not in allow:
        raise PlError(rc, lib.pl_last_error().decode())
    return rc


def lzone(node_xyz, beam_conn, beam_radius, device=0):
    """(B, 2) joint-penalisation lengths of a non-periodic lattice on the device (pl_lzone)."""
    lib = load_library()
    xyz = _f64(np.asarray(node_xyz).reshape(-1))
    conn = np.ascontiguousarray(beam_conn, dtype=np.int32).reshape(-1)
    rad = _f64(np.asarray(beam_radius).reshape(-1), len(conn) // 2)
    out = np.empty(len(conn), np.float64)
    _check(lib, lib.pl_lzone(int(device), len(xyz) // 3, len(conn) // 2, _ptr(xyz), _ptr(conn), _ptr(rad), _ptr(out)))
    return out.reshape(-1, 2)


def debug_spd_solve(A, b, device=0, fp32_factor=False):
    """Device dense SPD solve (test hook of the coarse solver): returns (x, b^T A^-1 b).  fp32_factor stores the
    inverse Cholesky factor in fp32, as the preconditioner does."""
    lib = load_library()
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.empty_like(b)
    q = C.c_double()
    _check(lib, lib.pl_debug_spd_solve(device, len(b), _ptr(A), _ptr(b), _ptr(x), C.byref(q), int(bool(fp32_factor))))
    return x, q.value


def debug_dense_level(A, r, bw_blocks, storage, trtri_rows=0, band_roundtrip=False, add0=None, device=0):
    """The dense level as the assembly and the preconditioner run it (pl_debug_dense_level): block band, storage of the
    inverse factor (64, 32 or 16 bits), row ranges on a second stream, band transfer, both forms of the apply.  Returns a
    dict of arrays of the padded size np (next multiple of 64): W, Wt (np, np) as stored, widened to float64; t, y (np,);
    quad; info (2,); and - where the one-GEMV form ran (``one_gemv``) - Ainv (np, np) float32, y_one, quad_one."""
    lib = load_library()
    r = _f64(r)
    n = len(r)
    A = _f64(A, n * n)
    add0 = np.zeros(64) if add0 is None else _f64(add0, 64)
    m = (n + 63) // 64 * 64
    W, Wt, Ainv = np.empty((m, m)), np.empty((m, m)), np.zeros((m, m), np.float32)
    t, y, y_one = np.empty(m), np.empty(m), np.zeros(m)
    quad, quad_one, one = C.c_double(), C.c_double(), C.c_int32()
    info = np.zeros(2, np.int32)
    _check(lib, lib.pl_debug_dense_level(int(device), n, _ptr(A), int(bw_blocks), int(storage), int(trtri_rows),
                                         int(bool(band_roundtrip)), _ptr(r), _ptr(add0), _ptr(W), _ptr(Wt), _ptr(Ainv),
                                         _ptr(t), _ptr(y), C.byref(quad), _ptr(y_one), C.byref(quad_one), C.byref(one),
                                         _ptr(info)))
    out = {"W": W, "Wt": Wt, "t": t, "y": y, "quad": quad.value, "info": info, "one_gemv": bool(one.value)}
    if one.value:
        out.update(Ainv=Ainv, y_one=y_one, quad_one=quad_one.value)
    return out


# columns one pl_spmv_multi / pl_solve_multi call takes (PL_MULTI_MAX of include/pylattice_hip.h)
MULTI_MAX = 64
# columns of one pl_sens_gram call (PL_SENS_GRAM_MAX)
SENS_GRAM_MAX = 8
# rows of the adjoint one pl_transient_sens contraction launch takes (PL_TRANSIENT_SENS_CHUNK)
TRANSIENT_SENS_CHUNK = 32

# what one workgroup of pl_schur_cells holds (include/pylattice_hip.h): larger cells go through pl_schur
SCHUR_CELLS_MAX_BOUNDARY, SCHUR_CELLS_MAX_INTERIOR, SCHUR_CELLS_MAX_BEAMS = 32, 16, 512


def schur_cells_fits(n_nodes, n_beams, n_boundary):
    """Whether pl_schur_cells condenses a cell of this size."""
    return (0 < n_boundary <= SCHUR_CELLS_MAX_BOUNDARY and n_nodes - n_boundary <= SCHUR_CELLS_MAX_INTERIOR
            and 0 < n_beams <= SCHUR_CELLS_MAX_BEAMS)


def _per_instance(name, a, tail, n_inst):
    """a of shape tail (shared by every instance) or (n_inst,) + tail, as a contiguous (n_inst,) + tail array."""
    if a.shape == tail:
        a = np.broadcast_to(a, (n_inst,) + tail)
    elif a.shape != (n_inst,) + tail:
        raise ValueError(f"{name} must have shape {tail} or {(n_inst,) + tail}, got {a.shape}")
    return np.ascontiguousarray(a)


def schur_cells(node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, young, poisson, kappa=0.9,
                pen_coef=1.5, device=0, n_inst=None):
    """Exact Schur complements of n_inst instances of one cell topology in one launch (pl_schur_cells).

    beam_conn (B, 2) and boundary_nodes (n_b,) are shared; node_xyz (N, 3), beam_radius (B,), seg_len (B, 3) and
    seg_nsub (B, 3) are either shared or given per instance with a leading n_inst axis.  Returns (S (n_inst, 6 n_b, 6 n_b),
    info (n_inst,) int32): info 0 = ok, k > 0 = Cholesky pivot k of K_II not positive, -1 = bad radius / segment data
    (S of such an instance is NaN)."""
    xyz, conn, bn, rad, slen, nsub, n_inst = _cell_batch_arrays(node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len,
                                                                seg_nsub, n_inst)
    B, N = len(conn), xyz.shape[1]
    lib = load_library()
    opts = default_opts(lib)
    opts.young, opts.poisson, opts.kappa, opts.pen_coef, opts.device = young, poisson, kappa, pen_coef, device
    m = 6 * len(bn)
    S = np.empty((n_inst, m, m), np.float64)
    info = np.empty(n_inst, np.int32)
    _check(lib, lib.pl_schur_cells(C.byref(opts), n_inst, N, B, _ptr(conn), len(bn), _ptr(bn), _ptr(xyz), _ptr(rad),
                                   _ptr(slen), _ptr(nsub), _ptr(S), _ptr(info)))
    return S, info


def _cell_batch_arrays(node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, n_inst, extra_lead=()):
    """The checked, broadcast arguments schur_cells and cells_recover share: (xyz, conn, bn, rad, slen, nsub, n_inst)."""
    conn = np.asarray(beam_conn)
    bn = np.asarray(boundary_nodes)
    if conn.ndim != 2 or conn.shape[1] != 2 or not np.issubdtype(conn.dtype, np.integer):
        raise ValueError("beam_conn must be an integer (B, 2) array")
    if bn.ndim != 1 or not np.issubdtype(bn.dtype, np.integer):
        raise ValueError("boundary_nodes must be a 1-D integer array")
    xyz, rad = np.asarray(node_xyz, dtype=np.float64), np.asarray(beam_radius, dtype=np.float64)
    slen, nsub = np.asarray(seg_len, dtype=np.float64), np.asarray(seg_nsub)
    if not np.issubdtype(nsub.dtype, np.integer):
        raise ValueError("seg_nsub must be an integer array")
    if xyz.ndim not in (2, 3) or xyz.shape[-1] != 3:
        raise ValueError("node_xyz must be (N, 3) or (n_inst, N, 3)")
    B, N = len(conn), xyz.shape[-2]
    lead = [a.shape[0] for a, nd in ((xyz, 3), (rad, 2), (slen, 3), (nsub, 3)) if a.ndim == nd] + list(extra_lead)
    if n_inst is None:
        n_inst = max(lead) if lead else 1
    n_inst = int(n_inst)
    if n_inst < 1:
        raise ValueError("n_inst must be >= 1")
    xyz = _per_instance("node_xyz", xyz, (N, 3), n_inst)
    rad = _per_instance("beam_radius", rad, (B,), n_inst)
    slen = _per_instance("seg_len", slen, (B, 3), n_inst)
    nsub = _per_instance("seg_nsub", nsub.astype(np.int32, copy=False), (B, 3), n_inst)
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    bn = np.ascontiguousarray(bn, dtype=np.int32)
    return xyz, conn, bn, rad, slen, nsub, n_inst


def cells_recover(node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len, seg_nsub, u_b, young, poisson, lam_b=None,
                  want=("u", "lam", "sens"), kappa=0.9, pen_coef=1.5, device=0):
    """Cell interiors and exact strut sensitivities from boundary values, n_inst instances of one cell topology in one
    launch (pl_cells_recover).

    Geometry arguments as ``schur_cells``.  u_b (6 n_b,) / (n_b, 6) or with a leading n_inst axis, rows in
    boundary_nodes order; lam_b likewise, None: lam = u.  ``want`` chooses among "u" (u_full (n_inst, N, 6): u_b on the
    boundary nodes, -K_II^-1 K_IB u_b on the others, in the cell's node order), "lam" (the same for lam_b) and "sens"
    ((n_inst, B): lam_e^T (dK_e/dr_b) u_e).  Returns a dict with the wanted keys and "info" ((n_inst,) int32, codes of
    ``schur_cells``; the outputs of a failed instance are NaN)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("u", "lam", "sens") for w in want):
        raise ValueError('want must be a non-empty subset of ("u", "lam", "sens")')
    bn = np.asarray(boundary_nodes)
    m = 6 * (len(bn) if bn.ndim == 1 else 0)

    def boundary_values(name, v):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim >= 2 and v.shape[-2:] == (m // 6, 6):
            v = v.reshape(v.shape[:-2] + (m,))
        if v.ndim not in (1, 2) or v.shape[-1] != m:
            raise ValueError(f"{name} must have {m} values per instance, got shape {v.shape}")
        return v

    ub = boundary_values("u_b", u_b)
    lb = None if lam_b is None else boundary_values("lam_b", lam_b)
    lead = [v.shape[0] for v in (ub, lb) if v is not None and v.ndim == 2]
    xyz, conn, bn, rad, slen, nsub, n_inst = _cell_batch_arrays(node_xyz, beam_conn, boundary_nodes, beam_radius, seg_len,
                                                                seg_nsub, None, lead)
    ub = _per_instance("u_b", ub, (m,), n_inst)
    lb = None if lb is None else _per_instance("lam_b", lb, (m,), n_inst)
    B, N = len(conn), xyz.shape[1]
    lib = load_library()
    opts = default_opts(lib)
    opts.young, opts.poisson, opts.kappa, opts.pen_coef, opts.device = young, poisson, kappa, pen_coef, device
    out = {"info": np.empty(n_inst, np.int32)}
    if "u" in want:
        out["u"] = np.empty((n_inst, N, 6), np.float64)
    if "lam" in want:
        out["lam"] = np.empty((n_inst, N, 6), np.float64)
    if "sens" in want:
        out["sens"] = np.empty((n_inst, B), np.float64)
    _check(lib, lib.pl_cells_recover(C.byref(opts), n_inst, N, B, _ptr(conn), len(bn), _ptr(bn), _ptr(xyz), _ptr(rad),
                                     _ptr(slen), _ptr(nsub), _ptr(ub), _ptr(lb), _ptr(out.get("u")), _ptr(out.get("lam")),
                                     _ptr(out.get("sens")), _ptr(out["info"])))
    return out


class PlLatticeInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("n_beams", C.c_int64), ("n_cell_beam", C.c_int64), ("n_cell_node", C.c_int64),
                ("n_created", C.c_int64)]


def generate_lattice(cell_coord, cell_size, cell_radii, tmpl, tmpl_type, want_created=False):
    """pl_generate_lattice: the multi-threaded host generator.  Returns a dict of arrays, or None when the library
    declines (lattice too irregular for its node table) and the numpy path has to be taken."""
    lib = load_library()
    cc, cs = _f64(cell_coord).reshape(-1, 3), _f64(cell_size).reshape(-1, 3)
    cr = _f64(cell_radii).reshape(len(cc), -1)
    tm = _f64(tmpl).reshape(-1, 6)
    tt = np.ascontiguousarray(tmpl_type, dtype=np.int32)
    h = C.c_void_p()
    info = PlLatticeInfo()
    rc = lib.pl_generate_lattice(len(cc), _ptr(cc), _ptr(cs), _ptr(cr), cr.shape[1], len(tm), _ptr(tm), _ptr(tt),
                                 C.byref(h), C.byref(info))
    if rc == PL_ERR_STATE:
        return None
    if rc != PL_OK:
        raise PlError(rc, "pl_generate_lattice: bad argument")
    try:
        Cn = len(cc)
        out = {"node_xyz": np.empty((info.n_nodes, 3)), "beam_conn": np.empty((info.n_beams, 2), np.int32),
               "beam_radius": np.empty(info.n_beams), "beam_type": np.empty(info.n_beams, np.int32),
               "beam_cell0": np.empty(info.n_beams, np.int32), "cell_beam_ptr": np.empty(Cn + 1, np.int64),
               "cell_beam_idx": np.empty(info.n_cell_beam, np.int64), "cell_node_ptr": np.empty(Cn + 1, np.int64),
               "cell_node_idx": np.empty(info.n_cell_node, np.int64)}
        if want_created:
            out["pid"] = np.empty((Cn, len(tm), 2), np.int32)
            out["bid"] = np.empty(Cn * len(tm), np.int32)
        order = ["node_xyz", "beam_conn", "beam_radius", "beam_type", "beam_cell0", "cell_beam_ptr", "cell_beam_idx",
                 "cell_node_ptr", "cell_node_idx", "pid", "bid"]
        lib.pl_lattice_fetch(h, *[_ptr(out.get(k)) for k in order])
    finally:
        lib.pl_lattice_free(h)
    return out


def penalize_arrays(node_xyz, beam_conn, lzone, mesh_size):
    """pl_penalize: (seg_len (B,3), seg_nsub (B,3) i32, pen_xyz (B,2,3))."""
    lib = load_library()
    xyz = _f64(node_xyz).reshape(-1, 3)
    conn = np.ascontiguousarray(beam_conn, dtype=np.int32).reshape(-1, 2)
    lz = None if lzone is None else _f64(lzone, 2 * len(conn))
    B = len(conn)
    seg_len, seg_nsub, pen = np.empty((B, 3)), np.empty((B, 3), np.int32), np.empty((B, 2, 3))
    _check(lib, lib.pl_penalize(B, _ptr(xyz), _ptr(conn), _ptr(lz), float(mesh_size), _ptr(seg_len), _ptr(seg_nsub),
                                _ptr(pen)))
    return seg_len, seg_nsub, pen


def boundary_index(cell_node_ptr, cell_node_idx, node_xyz, cell_coord, cell_size, by_coordinates=False):
    """pl_boundary_index: (index_boundary (N,) int64 with -1 off the cell boxes, nodes in visit order).
    by_coordinates: pl_boundary_index_rows - rows of a cell visited in rounded-coordinate order (reference_compat rows)."""
    lib = load_library()
    ptr = np.ascontiguousarray(cell_node_ptr, dtype=np.int64)
    idx = np.ascontiguousarray(cell_node_idx, dtype=np.int64)
    xyz = _f64(node_xyz).reshape(-1, 3)
    cc, cs = _f64(cell_coord).reshape(-1, 3), _f64(cell_size).reshape(-1, 3)
    ib = np.empty(len(xyz), np.int64)
    visit = np.empty(len(xyz), np.int64)
    nv = C.c_int64()
    fn = lib.pl_boundary_index_rows if by_coordinates else lib.pl_boundary_index
    _check(lib, fn(len(cc), _ptr(ptr), _ptr(idx), len(xyz), _ptr(xyz), _ptr(cc), _ptr(cs), _ptr(ib), _ptr(visit), C.byref(nv)))
    return ib, visit[:nv.value].copy()


class HipLattice:
    """Owner of one device handle: the condensed lattice operator + its PCG on one MI355X."""

    def __init__(self, node_xyz, beam_conn, beam_radius, seg_len, seg_nsub, young, poisson, kappa=0.9,
                 pen_coef=1.5, device=0, spmv_kernel=0, reorder=1, check_every=0, lanes_per_node=0, tile_nodes=0, precond=1,
                 coarse_max_dofs=0, grid=None, palette=0, local_max_dofs=0, precision=0, compact_records=0, condense=0, chol_persistent=0,
                 cg_form=0, tile_modes=0, coarse_modes=0, overlap=0, coarse_storage=0, warm_start=0, beam_mult=None, short_iteration=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.node_xyz = _f64(node_xyz).reshape(-1, 3)
        self.beam_conn = np.ascontiguousarray(beam_conn, dtype=np.int32).reshape(-1, 2)
        self.n_nodes, self.n_beams = len(self.node_xyz), len(self.beam_conn)
        self._radius = _f64(beam_radius, self.n_beams)
        self._seg_len = _f64(seg_len, 3 * self.n_beams)
        self._seg_nsub = np.ascontiguousarray(seg_nsub, dtype=np.int32).reshape(-1)
        self._material = (float(young), float(poisson), float(kappa), float(pen_coef))
        mesh = PlMesh(self.n_nodes, self.n_beams, _ptr(self.node_xyz), _ptr(self.beam_conn), _ptr(self._radius),
                      _ptr(self._seg_len), _ptr(self._seg_nsub))
        opts = default_opts(self._lib)
        opts.young, opts.poisson, opts.kappa, opts.pen_coef = young, poisson, kappa, pen_coef
        opts.device, opts.spmv_kernel, opts.reorder, opts.check_every = device, spmv_kernel, reorder, check_every
        opts.lanes_per_node = lanes_per_node
        opts.tile_nodes = tile_nodes
        opts.precond, opts.coarse_max_dofs = precond, coarse_max_dofs
        opts.local_max_dofs = local_max_dofs
        opts.palette = palette
        opts.compact_records = compact_records
        opts.condense = condense
        opts.chol_persistent = chol_persistent
        opts.cg_form = cg_form
        opts.tile_modes = tile_modes
        opts.coarse_modes = coarse_modes
        opts.overlap = overlap
        opts.coarse_storage = coarse_storage
        opts.warm_start = warm_start
        opts.short_iteration = short_iteration
        opts.precision = precision            # 0 fp64, 1 fp32 inner PCG + fp64 refinement, 2 fp32 p / K*p only
        if grid is not None:                       # (lo[3], hi[3], n_nodes) of the whole lattice (multi-GPU)
            lo, hi, nn = grid
            for k in range(3):
                opts.grid_lo[k], opts.grid_hi[k] = float(lo[k]), float(hi[k])
            opts.grid_nodes = int(nn)
        _check(self._lib, self._lib.pl_create(C.byref(mesh), C.byref(opts), C.byref(self._h)))
        self.last_stats = None
        self._mult = None
        self._thermal = None
        self._conduction = None
        self._convection = None
        self._heat_capacity = None
        self._assembled = False
        if beam_mult is not None:
            self.set_multiplicity(beam_mult)

    @classmethod
    def ddm(cls, n_nodes, cell_nodes, S, cell_S, device=0, alpha_max=100.0, check_every=0, precond=0, mintol=0.0,
            restart_every=0, node_xyz=None, coarse_max_dofs=0):
        """Handle for the domain-decomposition operator sum_c B^T S B (pl_create_ddm).  precond = 0: plain CG as the
        reference's default; 1: Jacobi on the assembled diagonal; 2: the reference's factorised assembled matrix
        (of the operator's own cell matrices unless ``set_ddm_preconditioner`` installs others); 3: its 6 x 6 node blocks;
        4: node blocks + a dense level of 12 modes per aggregate of nodes (needs ``node_xyz``, pl_ddm_set_geometry).
        check_every = 0: the host looks at the residual history every few dozen iterations; the device applies the
        reference's stopping rules itself and freezes the iterate at the iteration that meets them (k_pcg_direction), so the
        result is the reference's iterate whatever the host had queued (until round 5 the default was a look - and a drained
        stream - after every iteration)."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = C.c_void_p()
        cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
        Sm = np.ascontiguousarray(S, dtype=np.float64)
        if Sm.ndim == 2:
            Sm = Sm[None]
        cs = np.ascontiguousarray(cell_S, dtype=np.int32)
        self.n_nodes, self.n_beams = int(n_nodes), 0
        opts = default_opts(self._lib)
        opts.device, opts.alpha_max, opts.check_every = device, alpha_max, check_every
        opts.precond = precond
        opts.coarse_max_dofs = int(coarse_max_dofs)
        opts.mintol, opts.restart_every = float(mintol), int(restart_every)   # conjugate_gradient_solver.py:96-109
        if precond == 4 and node_xyz is None:
            raise ValueError("precond = 4 on a DDM handle needs node_xyz (the modes of its dense level)")
        _check(self._lib, self._lib.pl_create_ddm(self.n_nodes, cn.shape[0], cn.shape[1], _ptr(cn), Sm.shape[0],
                                                  _ptr(Sm), _ptr(cs), C.byref(opts), C.byref(self._h)))
        self.last_stats = None
        self._n_cells, self._m = cn.shape[0], 6 * cn.shape[1]
        if node_xyz is not None:
            self.set_ddm_geometry(node_xyz)
        return self

    def update_ddm_matrices(self, S, cell_S):
        """New cell matrices on this DDM handle (pl_ddm_update_matrices): same cells and nodes, other S_c; assemble() again
        before the next solve."""
        Sm = np.ascontiguousarray(S, dtype=np.float64)
        if Sm.ndim == 2:
            Sm = Sm[None]
        if Sm.shape[1:] != (self._m, self._m):
            raise ValueError(f"cell matrices must be {self._m} x {self._m}, got {Sm.shape[1:]}")
        cs = np.ascontiguousarray(cell_S, dtype=np.int32)
        if cs.shape != (self._n_cells,):
            raise ValueError("one matrix index per cell expected")
        _check(self._lib, self._lib.pl_ddm_update_matrices(self._h, Sm.shape[0], _ptr(Sm), _ptr(cs)))

    def set_ddm_geometry(self, node_xyz):
        """Node positions of a DDM handle (pl_ddm_set_geometry): aggregates and modes of the dense level of precond = 4."""
        xyz = np.ascontiguousarray(node_xyz, dtype=np.float64)
        if xyz.shape != (self.n_nodes, 3):
            raise ValueError(f"node_xyz must be ({self.n_nodes}, 3), got {xyz.shape}")
        _check(self._lib, self._lib.pl_ddm_set_geometry(self._h, _ptr(xyz)))

    def set_ddm_preconditioner(self, S=None, cell_S=None):
        """Cell matrices of the assembled-Schur preconditioner (pl_ddm_set_preconditioner); None = the operator's."""
        if S is None:
            _check(self._lib, self._lib.pl_ddm_set_preconditioner(self._h, 0, None, None))
            return
        Sm = np.ascontiguousarray(S, dtype=np.float64)
        if Sm.ndim == 2:
            Sm = Sm[None]
        if Sm.shape[1:] != (self._m, self._m):
            raise ValueError(f"preconditioner matrices must be {self._m} x {self._m}, got {Sm.shape[1:]}")
        cs = (np.zeros(self._n_cells, np.int32) if cell_S is None else np.ascontiguousarray(cell_S, dtype=np.int32))
        if cs.shape != (self._n_cells,):
            raise ValueError("one preconditioner matrix index per cell expected")
        _check(self._lib, self._lib.pl_ddm_set_preconditioner(self._h, Sm.shape[0], _ptr(Sm), _ptr(cs)))

    # -- lifetime ---------------------------------------------------------------------------------------
    def _changing(self, why):
        self._assembled = False               # (update_radii / set_multiplicity / update_segments clear the library's flag)
        cb = getattr(self, "_before_change", None)
        if cb is not None:
            self._before_change = None
            cb(why)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._changing("handle closed")
            self._lib.pl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- data -------------------------------------------------------------------------------------------
    def _opt_vec6(self, a):
        """An optional nodal vector ((N, 6) or (6 N,)) as contiguous float64; None stays None (the library's NULL)."""
        return None if a is None else _f64(np.asarray(a).reshape(-1), 6 * self.n_nodes)

    def _pnorm(self, call, u, want_grad, *args):
        """(value, max, d/du (N, 6) or None, d/dr (B,) or None) of a pl_*_pnorm entry point, which takes (handle, u, *args,
        &value, &max, du, dr)."""
        val, vmax = C.c_double(), C.c_double()
        du = np.empty((self.n_nodes, 6), np.float64) if want_grad else None
        dr = np.empty(self.n_beams, np.float64) if want_grad else None
        _check(self._lib, call(self._h, _ptr(self._opt_vec6(u)), *args, C.byref(val), C.byref(vmax), _ptr(du), _ptr(dr)))
        return val.value, vmax.value, du, dr

    def set_bc(self, fixed, ubar=None, f=None):
        n6 = 6 * self.n_nodes
        fx = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
        if fx.size != n6:
            raise ValueError("fixed must have 6*n_nodes entries")
        ub = self._opt_vec6(ubar)
        ff = self._opt_vec6(f)
        _check(self._lib, self._lib.pl_set_bc(self._h, _ptr(fx), _ptr(ub), _ptr(ff)))

    def update_radii(self, radius):
        self._changing("update_radii")
        self._radius = _f64(radius, self.n_beams)
        _check(self._lib, self._lib.pl_update_radii(self._h, _ptr(self._radius)))

    def set_multiplicity(self, beam_mult):
        """Strut b counts as beam_mult[b] identical struts in parallel (pl_set_multiplicity); None = 1 everywhere."""
        self._changing("set_multiplicity")
        self._mult = None if beam_mult is None else _f64(beam_mult, self.n_beams)
        _check(self._lib, self._lib.pl_set_multiplicity(self._h, _ptr(self._mult)))

    def update_segments(self, seg_len, seg_nsub):
        self._changing("update_segments")
        self._seg_len = _f64(seg_len, 3 * self.n_beams)
        self._seg_nsub = np.ascontiguousarray(seg_nsub, dtype=np.int32).reshape(-1)
        _check(self._lib, self._lib.pl_update_segments(self._h, _ptr(self._seg_len), _ptr(self._seg_nsub)))

    def assemble(self):
        _check(self._lib, self._lib.pl_assemble(self._h))
        self._assembled = True

    def assemble_bsr(self, with_bc=False):
        nr, nb = C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.pl_assemble_bsr(self._h, int(bool(with_bc)), C.byref(nr), C.byref(nb)))
        return nr.value, nb.value

    def get_bsr(self):
        nr, nb = self.n_nodes, self.n_nodes + 2 * self.n_beams
        rowptr = np.empty(nr + 1, np.int64)
        col = np.empty(nb, np.int32)
        vals = np.empty((nb, 6, 6), np.float64)
        _check(self._lib, self._lib.pl_get_bsr(self._h, _ptr(rowptr), _ptr(col), _ptr(vals)))
        return rowptr, col, vals

    def records(self):
        rec = np.empty((self.n_beams, 8), np.float64)
        _check(self._lib, self._lib.pl_get_records(self._h, _ptr(rec)))
        return rec

    def partition(self):
        """The solver's partition in the caller's node numbering (pl_debug_partition): dict of (N,) arrays - ``tile`` (K*p
        tile = block of the tile level), ``agg`` (aggregate of the dense level), ``local_agg`` (aggregate of the rank-local
        level of precond = 4), int32 with -1 where the handle has no such level, and ``eliminated`` (bool: nodes that
        opts.condense takes out of the CG; after assemble()).  A DDM handle with node positions reports the aggregates of
        its precond = 4 in ``agg``."""
        n = self.n_nodes
        tile, agg, loc = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        elim = np.empty(n, np.uint8)
        _check(self._lib, self._lib.pl_debug_partition(self._h, _ptr(tile), _ptr(agg), _ptr(loc), _ptr(elim)))
        return {"tile": tile, "agg": agg, "local_agg": loc, "eliminated": elim.astype(bool)}

    # -- operator ---------------------------------------------------------------------------------------
    def _vec_op(self, fn, x):
        x = _f64(np.asarray(x).reshape(-1), 6 * self.n_nodes)
        y = np.empty_like(x)
        _check(self._lib, fn(self._h, _ptr(x), _ptr(y)))
        return y.reshape(self.n_nodes, 6)

    def spmv(self, x):
        return self._vec_op(self._lib.pl_spmv, x)

    def spmv_free(self, x):
        return self._vec_op(self._lib.pl_spmv_free, x)

    def spmv_bsr(self, x):
        return self._vec_op(self._lib.pl_spmv_bsr, x)

    def reactions(self, u):
        return self._vec_op(self._lib.pl_reactions, u)

    def solve(self, rtol=1e-8, max_iter=20000, raise_on_noconv=True, download=True):
        """PCG solve; returns (u[N,6], stats).  download=False leaves u on the device and returns stats only."""
        u = np.empty(6 * self.n_nodes, np.float64) if download else None
        st = PlStats()
        st.struct_size = C.sizeof(PlStats)
        rc = self._lib.pl_solve(self._h, float(rtol), int(max_iter), _ptr(u), C.byref(st))
        self.last_stats = {k: getattr(st, k) for k, _ in PlStats._fields_ if k not in ("reserved", "reserved_i", "struct_size")}
        _timing.device("pl_solve: PCG (HIP events)", st.ms_solve)
        if st.ms_assembly > 0.0:
            _timing.device("pl_assemble of this solve (HIP events)", st.ms_assembly)
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        if not download:
            return self.last_stats
        return u.reshape(self.n_nodes, 6), self.last_stats

    def sens(self, u, lam=None):
        """Per-strut sensitivities lam^T (dK_e/dr) u (pl_sens).  u = None: the solution of the last solve() of this handle,
        still on the device (no upload)."""
        u = self._opt_vec6(u)
        lam_a = self._opt_vec6(lam)
        out = np.empty(self.n_beams, np.float64)
        _check(self._lib, self._lib.pl_sens(self._h, _ptr(u), _ptr(lam_a), _ptr(out)))
        return out

    def sens_gram(self, X):
        """G[k, l, b] = X[k]_e^T (dK_e/dr_b) X[l]_e for every pair of the k columns of X in one pass over the struts
        (pl_sens_gram): X (k, N, 6) or (k, 6 N), k = 1 ... SENS_GRAM_MAX (the library checks it); returns the full symmetric
        (k, k, B) array - the library computes the upper triangle, the lower one is its mirror.  The same dK_e/dr as
        ``sens``: fixed segment geometry."""
        x = np.asarray(X, dtype=np.float64)
        n6 = 6 * self.n_nodes
        if x.ndim == 3 and x.shape[1:] == (self.n_nodes, 6):
            x = x.reshape(x.shape[0], n6)
        elif not (x.ndim == 2 and x.shape[1] == n6):
            raise ValueError(f"X must have shape (k, {self.n_nodes}, 6) or (k, {n6}), got {x.shape}")
        x = np.ascontiguousarray(x)
        k = x.shape[0]
        tri = np.empty((max(k * (k + 1) // 2, 1), self.n_beams), np.float64)
        _check(self._lib, self._lib.pl_sens_gram(self._h, k, _ptr(x), _ptr(tri)))
        iu = np.triu_indices(k)
        out = np.empty((k, k, self.n_beams), np.float64)
        out[iu] = tri
        out[iu[1], iu[0]] = tri
        return out

    def node_mod(self, u):
        """(B, 2, 6) displacements of the two penalisation points of every strut (pl_node_mod)."""
        u = _f64(np.asarray(u).reshape(-1), 6 * self.n_nodes)
        out = np.empty((self.n_beams, 2, 6), np.float64)
        _check(self._lib, self._lib.pl_node_mod(self._h, _ptr(u), _ptr(out)))
        return out

    def stress(self, u=None, where=0):
        """Section forces and von Mises stress at the stations [A, q1, q2, B] of every strut (pl_stress): dict with N, V, T,
        Mb, sigma_vm of shape (B, 4) (NaN at absent stations) and peak (B,).  u = None: the solution of the last solve().
        where = 0: all stations, 1: the two ends of the middle segment only."""
        u = self._opt_vec6(u)
        st = np.empty((self.n_beams, 4, 5), np.float64)
        peak = np.empty(self.n_beams, np.float64)
        _check(self._lib, self._lib.pl_stress(self._h, _ptr(u), int(where), _ptr(st), _ptr(peak)))
        out = {name: st[:, :, i] for i, name in enumerate(("N", "V", "T", "Mb", "sigma_vm"))}
        out["peak"] = peak
        return out

    def stress_pnorm(self, p, u=None, where=0, want_grad=True):
        """(phi, sigma_max, dphi_du (N, 6), dphi_dr (B,)) of the p-norm aggregate of sigma_vm over the stations
        (pl_stress_pnorm); the two derivatives are None with want_grad=False.  dphi_dr: at fixed u and segment geometry."""
        return self._pnorm(self._lib.pl_stress_pnorm, u, want_grad, int(where), float(p))

    def stress_host(self, u, where=0):
        """The numpy restatement of ``stress`` (stress_host.strut_stress) on this handle's records and segment data."""
        from . import stress_host as SH
        rec = self.records()
        return SH.strut_stress(rec, self.beam_conn, self._radius, self._seg_len, u, self._material[3], self._mult, where,
                               self._f_th_host(rec))

    def stress_pnorm_host(self, p, u, where=0, want_grad=True):
        """The numpy restatement of ``stress_pnorm`` (stress_host.stress_pnorm)."""
        from . import stress_host as SH
        E, nu, kappa, pen = self._material
        rec = self.records()
        return SH.stress_pnorm(rec, self.n_nodes, self.beam_conn, self._radius, self._seg_len, self._seg_nsub,
                               u, p, E, nu, kappa, pen, self._mult, where, want_grad, self._f_th_host(rec))

    def buckling(self, u=None, length=1, k_eff=1.0, shear=0):
        """Euler buckling utilisation of every strut (pl_buckling): dict with util = max(0, -N) / N_cr, n_axial (signed N of
        one copy) and n_crit, each (B,).  u = None: the solution of the last solve().  length = 0: node-to-node buckling
        length, 1: the middle segment (NaN on a strut without one); k_eff: effective-length factor; shear = 1: Engesser."""
        u = self._opt_vec6(u)
        out = {name: np.empty(self.n_beams, np.float64) for name in ("util", "n_axial", "n_crit")}
        _check(self._lib, self._lib.pl_buckling(self._h, _ptr(u), int(length), float(k_eff), int(shear), _ptr(out["util"]),
                                                _ptr(out["n_axial"]), _ptr(out["n_crit"])))
        return out

    def buckling_pnorm(self, p, u=None, length=1, k_eff=1.0, shear=0, want_grad=True):
        """(bp, util_max, dbp_du (N, 6), dbp_dr (B,)) of the p-norm aggregate of the utilisations (pl_buckling_pnorm); the
        two derivatives are None with want_grad=False.  dbp_dr: at fixed u and segment geometry."""
        return self._pnorm(self._lib.pl_buckling_pnorm, u, want_grad, int(length), float(k_eff), int(shear), float(p))

    def buckling_host(self, u, length=1, k_eff=1.0, shear=0):
        """The numpy restatement of ``buckling`` (buckling_host.strut_buckling) on this handle's records and segment data."""
        from . import buckling_host as BH
        E, nu, kappa, _ = self._material
        rec = self.records()
        return BH.strut_buckling(rec, self.beam_conn, self._radius, self._seg_len, u, E, nu, kappa, self._mult,
                                 length, k_eff, shear, self._f_th_host(rec))

    def buckling_pnorm_host(self, p, u, length=1, k_eff=1.0, shear=0, want_grad=True):
        """The numpy restatement of ``buckling_pnorm`` (buckling_host.buckling_pnorm)."""
        from . import buckling_host as BH
        E, nu, kappa, pen = self._material
        rec = self.records()
        return BH.buckling_pnorm(rec, self.n_nodes, self.beam_conn, self._radius, self._seg_len, self._seg_nsub,
                                 u, p, E, nu, kappa, pen, self._mult, length, k_eff, shear, want_grad, self._f_th_host(rec))

    # -- thermal loads ------------------------------------------------------------------------------------
    def set_thermal(self, alpha, node_dT, beam_alpha=None):
        """Thermal state of the handle (pl_set_thermal): expansion coefficient ``alpha`` of every strut, or beam_alpha (B,)
        per strut, and the temperature rise node_dT (N,) of every node.  While it is set, ``stress``, ``stress_pnorm``,
        ``buckling`` and ``buckling_pnorm`` evaluate the mechanical section force K_tip (du, dth) - ka delta t, and
        ``buckling_modes`` / ``geom_spmv_multi`` refuse.  It survives update_radii / update_segments / assemble."""
        dT = _f64(np.asarray(node_dT).reshape(-1), self.n_nodes)
        ba = None if beam_alpha is None else _f64(np.asarray(beam_alpha).reshape(-1), self.n_beams)
        _check(self._lib, self._lib.pl_set_thermal(self._h, float(alpha), _ptr(ba), _ptr(dT)))
        self._thermal = (ba if ba is not None else float(alpha), dT)

    def clear_thermal(self):
        """Removes the thermal state (pl_set_thermal with node_dT = NULL)."""
        _check(self._lib, self._lib.pl_set_thermal(self._h, 0.0, None, None))
        self._thermal = None

    def thermal_load(self):
        """(f_th (N, 6), n_free (B,)) of the thermal state on the records of the last assemble() (pl_thermal_load): the
        equivalent nodal loads, K u = f_ext + f_th, and the restrained force of one copy of every strut."""
        f = np.empty((self.n_nodes, 6), np.float64)
        n_free = np.empty(self.n_beams, np.float64)
        _check(self._lib, self._lib.pl_thermal_load(self._h, _ptr(f), _ptr(n_free)))
        return f, n_free

    def thermal_sens(self, lam=None):
        """(B,) lam^T d f_th / d r_b at fixed segment geometry (pl_thermal_sens); lam = None: the solution of the last
        solve(), still on the device."""
        out = np.empty(self.n_beams, np.float64)
        _check(self._lib, self._lib.pl_thermal_sens(self._h, _ptr(self._opt_vec6(lam)), _ptr(out)))
        return out

    def _delta_host(self):
        from . import thermal_host as TH
        if getattr(self, "_thermal", None) is None:
            return None
        return TH.elongation(self.node_xyz, self.beam_conn, *self._thermal)

    def _f_th_host(self, rec):
        """Restrained thermal force of every record (thermal_host.restrained_force), None without a thermal state."""
        from . import thermal_host as TH
        delta = self._delta_host()
        return None if delta is None else TH.restrained_force(rec, delta)

    def thermal_load_host(self):
        """The numpy restatement of ``thermal_load`` (thermal_host.thermal_load) on this handle's records."""
        from . import thermal_host as TH
        if self._thermal is None:
            raise RuntimeError("thermal_load_host: call set_thermal first")
        return TH.thermal_load(self.records(), self.beam_conn, self.n_nodes, self._delta_host(), self._mult)

    def thermal_sens_host(self, lam):
        """The numpy restatement of ``thermal_sens`` (thermal_host.thermal_sens)."""
        from . import thermal_host as TH
        if self._thermal is None:
            raise RuntimeError("thermal_sens_host: call set_thermal first")
        return TH.thermal_sens(self.records(), self.beam_conn, self._radius, self._delta_host(), lam)

    # -- steady heat conduction on the strut graph -----------------------------------------------------------
    def set_conduction(self, kappa, beam_kappa=None):
        """Conduction state of the handle (pl_set_conduction): conductivity ``kappa`` of every strut, or beam_kappa (B,) per
        strut; each strut conducts with g = k kappa pi r^2 / L between its nodes.  It survives update_radii / update_segments /
        assemble, and the conductances follow the radii."""
        bk = None if beam_kappa is None else _f64(np.asarray(beam_kappa).reshape(-1), self.n_beams)
        _check(self._lib, self._lib.pl_set_conduction(self._h, float(kappa), _ptr(bk)))
        self._conduction = bk if bk is not None else float(kappa)
        self._convection = None      # (the convection state lives in the conduction state)
        self._heat_capacity = None   # (and so does the heat capacity)

    def clear_conduction(self):
        """Removes the conduction state (pl_set_conduction with kappa = 0 and no beam_kappa)."""
        _check(self._lib, self._lib.pl_set_conduction(self._h, 0.0, None))
        self._conduction = None
        self._convection = None
        self._heat_capacity = None

    def set_convection(self, film, ambient, beam_film=None):
        """Convection state of the handle (pl_set_convection): film coefficient ``film`` of every strut, or beam_film (B,) per
        strut, to an ambient at ``ambient``; each strut end exchanges through c = k h pi r L.  Needs a conduction state and is
        dropped with it (set_conduction included); it survives update_radii / update_segments / assemble.  cond_spmv,
        cond_solve and cond_sens then act on the convective problem."""
        bf = None if beam_film is None else _f64(np.asarray(beam_film).reshape(-1), self.n_beams)
        _check(self._lib, self._lib.pl_set_convection(self._h, float(film), _ptr(bf), float(ambient)))
        self._convection = (bf if bf is not None else float(film), float(ambient))

    def clear_convection(self):
        """Removes the convection state (pl_set_convection with film = 0 and no beam_film)."""
        _check(self._lib, self._lib.pl_set_convection(self._h, 0.0, None, 0.0))
        self._convection = None

    def _mask_n(self, fixed):
        fx = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
        if fx.size != self.n_nodes:
            raise ValueError("the thermal mask must have n_nodes entries")
        return fx

    def cond_spmv(self, x, fixed=None):
        """(N,) K_T x (pl_cond_spmv); fixed (N,) given: P K_T P x under that mask of one flag per node."""
        x = _f64(np.asarray(x).reshape(-1), self.n_nodes)
        fx = None if fixed is None else self._mask_n(fixed)
        y = np.empty(self.n_nodes, np.float64)
        _check(self._lib, self._lib.pl_cond_spmv(self._h, int(fx is not None), _ptr(fx), _ptr(x), _ptr(y)))
        return y

    def cond_solve(self, fixed, t_bar=None, q=None, rtol=1e-10, max_iter=200000, raise_on_noconv=True, adjoint=False):
        """(T (N,), stats) of K_T T = q on the free nodes, T = t_bar on the nodes of ``fixed`` (pl_cond_solve): a Jacobi PCG
        from zero on the device.  t_bar None = 0, q None = no inflow.  The handle's mechanical state is not touched.  Under a
        convection state: (K_T + H) T = q + H T_inf, and a mask that fixes no node is valid.  adjoint = True
        (pl_cond_solve_adjoint): (K_T + H) mu = q with mu = 0 on the fixed nodes, no ambient term."""
        fx = self._mask_n(fixed)
        tb = None if t_bar is None else _f64(np.broadcast_to(np.asarray(t_bar, dtype=float).reshape(-1), (self.n_nodes,)))
        qq = None if q is None else _f64(np.asarray(q).reshape(-1), self.n_nodes)
        T = np.empty(self.n_nodes, np.float64)
        st = PlStats()
        st.struct_size = C.sizeof(PlStats)
        if adjoint:
            if qq is None or tb is not None:
                raise ValueError("cond_solve(adjoint=True) takes a right-hand side q and no t_bar")
            rc = self._lib.pl_cond_solve_adjoint(self._h, _ptr(fx), _ptr(qq), float(rtol), int(max_iter), _ptr(T), C.byref(st))
        else:
            rc = self._lib.pl_cond_solve(self._h, _ptr(fx), _ptr(tb), _ptr(qq), float(rtol), int(max_iter), _ptr(T), C.byref(st))
        keys = [n for n, _ in PlStats._fields_ if n not in ("reserved", "reserved_i", "struct_size")]
        stats = {n: getattr(st, n) for n in keys}
        if rc in (PL_OK, PL_ERR_NOCONV):
            _timing.device("pl_cond_solve: PCG (HIP events)", st.ms_solve)
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        return T, stats

    def cond_flux(self, T):
        """(B,) heat flow Q_b = g (T_A - T_B) / k of one copy of every strut from A to B (pl_cond_flux)."""
        T = _f64(np.asarray(T).reshape(-1), self.n_nodes)
        Q = np.empty(self.n_beams, np.float64)
        _check(self._lib, self._lib.pl_cond_flux(self._h, _ptr(T), _ptr(Q)))
        return Q

    def cond_sens(self, T, mu, convective=True):
        """(B,) mu^T (dK_T / dr_b) T = (2 g / r)(mu_A - mu_B)(T_A - T_B) (pl_cond_sens); under a convection state plus
        (c / r)[mu_A (T_A - T_inf) + mu_B (T_B - T_inf)].  convective = False leaves that bracket out (the convection state
        is lifted for the call): the switch of the tests that show what the term is worth."""
        T = _f64(np.asarray(T).reshape(-1), self.n_nodes)
        mu = _f64(np.asarray(mu).reshape(-1), self.n_nodes)
        out = np.empty(self.n_beams, np.float64)
        cv = self._convection if not convective else None
        if cv is not None:
            self.clear_convection()
        try:
            _check(self._lib, self._lib.pl_cond_sens(self._h, _ptr(T), _ptr(mu), _ptr(out)))
        finally:
            if cv is not None:
                self.set_convection(0.0 if isinstance(cv[0], np.ndarray) else cv[0], cv[1],
                                    cv[0] if isinstance(cv[0], np.ndarray) else None)
        return out

    def cond_film(self, T, total=False):
        """(B,) convective loss Qc_b = c [(T_A - T_inf) + (T_B - T_inf)] / k of one copy of every strut (pl_cond_film);
        total = True: (Qc, P) with the dissipated power P = sum k Qc folded on the device in a fixed order."""
        T = _f64(np.asarray(T).reshape(-1), self.n_nodes)
        Qc = np.empty(self.n_beams, np.float64)
        P = np.zeros(1, np.float64)
        _check(self._lib, self._lib.pl_cond_film(self._h, _ptr(T), _ptr(Qc), _ptr(P) if total else None))
        return (Qc, float(P[0])) if total else Qc

    def temp_pnorm(self, T, p=8.0, reference=0.0, nodes=None, gradient=False):
        """{"phi", "max", "sum"} of the temperature p-norm (sum over the nodes of ``nodes`` (N,) flags, None = all, of
        max(T - reference, 0)^p)^(1/p) (pl_temp_pnorm); gradient = True adds "dphi_dT" (N,)."""
        T = _f64(np.asarray(T).reshape(-1), self.n_nodes)
        nd = None if nodes is None else self._mask_n(nodes)
        out = np.zeros(3, np.float64)
        g = np.empty(self.n_nodes, np.float64) if gradient else None
        _check(self._lib, self._lib.pl_temp_pnorm(self._h, _ptr(T), _ptr(nd), float(reference), float(p), _ptr(out), _ptr(g)))
        res = {"phi": float(out[0]), "max": float(out[1]), "sum": float(out[2])}
        if gradient:
            res["dphi_dT"] = g
        return res

    def thermal_load_adjoint(self, lam):
        """(N,) c = (d f_th / d dT)^T lam of the thermal state's expansion coefficients (pl_thermal_load_adjoint)."""
        lam = _f64(np.asarray(lam).reshape(-1), 6 * self.n_nodes)
        out = np.empty(self.n_nodes, np.float64)
        _check(self._lib, self._lib.pl_thermal_load_adjoint(self._h, _ptr(lam), _ptr(out)))
        return out

    # -- transient heat conduction ----------------------------------------------------------------------------
    def set_heat_capacity(self, rho_c, beam_rho_c=None, node_capacity=None):
        """Heat capacity of the handle (pl_set_heat_capacity): volumetric heat capacity ``rho_c`` of every strut, or beam_rho_c
        (B,) per strut, lumped to the nodes as C_i = sum (1/2) k rho_c pi r^2 L + node_capacity_i (node_capacity (N,) >= 0 or
        None).  Needs a conduction state and is dropped with it (set_conduction included); it survives update_radii /
        update_segments / assemble, and C follows the radii."""
        br = None if beam_rho_c is None else _f64(np.asarray(beam_rho_c).reshape(-1), self.n_beams)
        nc = None if node_capacity is None else _f64(np.asarray(node_capacity).reshape(-1), self.n_nodes)
        _check(self._lib, self._lib.pl_set_heat_capacity(self._h, float(rho_c), _ptr(br), _ptr(nc)))
        self._heat_capacity = (br if br is not None else float(rho_c), nc)

    def clear_heat_capacity(self):
        """Removes the heat capacity (pl_set_heat_capacity with rho_c = 0 and no beam_rho_c)."""
        _check(self._lib, self._lib.pl_set_heat_capacity(self._h, 0.0, None, None))
        self._heat_capacity = None

    def _transient_args(self, n_steps, patterns, amp, bar_amp):
        n_steps = int(n_steps)
        rows = max(n_steps, 0) + 1
        pat = am = None
        n_pat = 0
        if patterns is not None:
            pat = np.ascontiguousarray(np.asarray(patterns, dtype=np.float64)).reshape(-1, self.n_nodes)
            n_pat = pat.shape[0]
            am = np.ascontiguousarray(np.asarray(amp, dtype=np.float64).reshape(-1))
            if am.size != rows * n_pat:
                raise ValueError(f"amp must have shape ({rows}, {n_pat})")
        ba = None if bar_amp is None else _f64(np.asarray(bar_amp).reshape(-1), rows)
        return n_steps, rows, n_pat, pat, am, ba

    def cond_transient(self, dt, n_steps, theta=1.0, fixed=None, t_bar=None, bar_amp=None, patterns=None, amp=None, t0=None,
                       rtol=1e-10, max_iter=100000, probes=None, snap_every=0, want_state=True):
        """n_steps implicit theta steps of C dT/dt + (K_T + H) T = amp[n] @ patterns + H T_inf on the free nodes of ``fixed``
        (N,) flags (None = none), T = t0 + bar_amp[n] (t_bar - t0) on the fixed ones (pl_cond_transient).  patterns (n_pat, N),
        n_pat <= 4, amp (n_steps + 1, n_pat); bar_amp (n_steps + 1,) or None = 1; t0 (N,) or None = the ambient; probes: node
        indices.  Returns a dict: times (n_steps + 1,), probe (n_steps + 1, n_probe), heat (n_steps + 1, 4) = stored heat U and
        the cumulative Q_in, Q_c, Q_R (U_n - U_0 = Q_in + Q_R - Q_c), iters (n_steps + 1,), state (N,) = the last row (a call
        started from it continues the history), and snaps (n_steps // snap_every, N) if snap_every > 0."""
        n_steps, rows, n_pat, pat, am, ba = self._transient_args(n_steps, patterns, amp, bar_amp)
        fx = None if fixed is None else self._mask_n(fixed)
        tb = None if t_bar is None else _f64(np.broadcast_to(np.asarray(t_bar, dtype=float).reshape(-1), (self.n_nodes,)))
        tt0 = None if t0 is None else _f64(np.broadcast_to(np.asarray(t0, dtype=float).reshape(-1), (self.n_nodes,)))
        pr = np.zeros(0, np.int32) if probes is None else np.ascontiguousarray(np.asarray(probes).reshape(-1), dtype=np.int32)
        probe = np.zeros((rows, pr.size), np.float64)
        heat = np.zeros((rows, 4), np.float64)
        iters = np.zeros(rows, np.int32)
        snap_every = int(snap_every)
        snaps = np.zeros((n_steps // snap_every, self.n_nodes), np.float64) if snap_every > 0 and n_steps > 0 else None
        state = np.zeros(self.n_nodes, np.float64) if want_state else None
        _check(self._lib, self._lib.pl_cond_transient(self._h, n_steps, float(dt), float(theta), _ptr(fx), _ptr(tb), _ptr(ba),
                                                      n_pat, _ptr(pat), _ptr(am), _ptr(tt0), float(rtol), int(max_iter), pr.size,
                                                      _ptr(pr) if pr.size else None, _ptr(probe) if pr.size else None,
                                                      _ptr(heat), snap_every, _ptr(snaps), _ptr(state), _ptr(iters)))
        out = {"times": float(dt) * np.arange(rows), "probe": probe, "heat": heat, "iters": iters}
        if want_state:
            out["state"] = state
        if snaps is not None:
            out["snaps"] = snaps
        return out

    def heat_capacity_host(self):
        """(N,) the lumped heat capacity C of the current radii (conduction_host.heat_capacity)."""
        from . import conduction_host as CH
        hc = getattr(self, "_heat_capacity", None)
        if hc is None:
            raise RuntimeError("call set_heat_capacity first")
        return CH.heat_capacity(self.node_xyz, self.beam_conn, self._radius, hc[0], self._mult, hc[1])

    def cond_transient_host(self, dt, n_steps, theta=1.0, fixed=None, t_bar=None, bar_amp=None, patterns=None, amp=None, t0=None,
                            probes=None, snap_every=0):
        """The dense numpy restatement of ``cond_transient`` (conduction_host.transient), the same dict without iters; "T"
        (n_steps + 1, N) holds every row."""
        from . import conduction_host as CH
        H, t_inf = self._H_host()
        res = CH.transient(self.beam_conn, self.n_nodes, self._g_host(), self.heat_capacity_host(), dt, n_steps, theta, fixed,
                           t_bar, bar_amp, patterns, amp, t0, H, t_inf)
        T = res["T"]
        pr = np.zeros(0, np.int64) if probes is None else np.asarray(probes).reshape(-1)
        out = {"times": float(dt) * np.arange(int(n_steps) + 1), "probe": T[:, pr], "heat": res["heat"], "state": T[-1].copy(),
               "T": T, "bar": res["bar"]}
        if snap_every > 0:
            out["snaps"] = T[snap_every::snap_every][:int(n_steps) // snap_every].copy()
        return out

    def _g_host(self):
        from . import conduction_host as CH
        if getattr(self, "_conduction", None) is None:
            raise RuntimeError("call set_conduction first")
        return CH.conductance(self.node_xyz, self.beam_conn, self._radius, self._conduction, self._mult)

    def _c_host(self):
        """(c (B,), T_inf) of the convection state, (None, 0.0) without one."""
        from . import conduction_host as CH
        cv = getattr(self, "_convection", None)
        if cv is None:
            return None, 0.0
        return CH.film_conductance(self.node_xyz, self.beam_conn, self._radius, cv[0], self._mult), cv[1]

    def _H_host(self):
        from . import conduction_host as CH
        c, t_inf = self._c_host()
        return (None if c is None else CH.convection_diag(self.beam_conn, self.n_nodes, c)), t_inf

    def cond_spmv_host(self, x, fixed=None):
        """The numpy restatement of ``cond_spmv`` (conduction_host.spmv)."""
        from . import conduction_host as CH
        return CH.spmv(self.beam_conn, self.n_nodes, self._g_host(), x, fixed, self._H_host()[0])

    def cond_solve_host(self, fixed, t_bar=None, q=None, adjoint=False):
        """The dense host solve of the problem of ``cond_solve`` (conduction_host.solve)."""
        from . import conduction_host as CH
        qq = None if q is None else np.where(np.asarray(fixed).reshape(-1) != 0, 0.0, np.asarray(q, dtype=float).reshape(-1))
        H, t_inf = self._H_host()
        return CH.solve(self.beam_conn, self.n_nodes, self._g_host(), fixed, t_bar, qq, H, 0.0 if adjoint else t_inf)

    def cond_flux_host(self, T):
        """The numpy restatement of ``cond_flux`` (conduction_host.flux)."""
        from . import conduction_host as CH
        return CH.flux(self.beam_conn, self._g_host(), T, self._mult)

    def cond_sens_host(self, T, mu):
        """The numpy restatement of ``cond_sens`` (conduction_host.cond_sens)."""
        from . import conduction_host as CH
        c, t_inf = self._c_host()
        return CH.cond_sens(self.beam_conn, self._radius, self._g_host(), T, mu, c, t_inf)

    def cond_film_host(self, T, total=False):
        """The numpy restatement of ``cond_film`` (conduction_host.film_loss)."""
        from . import conduction_host as CH
        c, t_inf = self._c_host()
        if c is None:
            raise RuntimeError("cond_film_host: call set_convection first")
        Qc = CH.film_loss(self.beam_conn, c, T, t_inf, self._mult)
        k = 1.0 if self._mult is None else np.asarray(self._mult, dtype=float)
        return (Qc, float((k * Qc).sum())) if total else Qc

    def temp_pnorm_host(self, T, p=8.0, reference=0.0, nodes=None, gradient=False):
        """The numpy restatement of ``temp_pnorm`` (conduction_host.temp_pnorm)."""
        from . import conduction_host as CH
        phi, vmax, ssum, g = CH.temp_pnorm(T, p, reference, nodes)
        res = {"phi": phi, "max": vmax, "sum": ssum}
        if gradient:
            res["dphi_dT"] = g
        return res

    def thermal_load_adjoint_host(self, lam):
        """The numpy restatement of ``thermal_load_adjoint`` (conduction_host.thermal_load_adjoint)."""
        from . import conduction_host as CH
        if self._thermal is None:
            raise RuntimeError("thermal_load_adjoint_host: call set_thermal first")
        return CH.thermal_load_adjoint(self.records(), self.beam_conn, self.n_nodes, self._thermal[0], lam)

    def energy(self, u):
        u = _f64(np.asarray(u).reshape(-1), 6 * self.n_nodes)
        e = C.c_double()
        _check(self._lib, self._lib.pl_energy(self._h, _ptr(u), C.byref(e)))
        return e.value

    def schur(self, boundary_nodes, rtol=1e-12, max_iter=20000, block=None):
        """Schur complement on the listed nodes.  block = None: pl_schur, one solve per boundary dof; an int: pl_schur_block,
        `block` columns per PCG pass, generated and contracted on the device (0 = the library's choice)."""
        bn = np.ascontiguousarray(boundary_nodes, dtype=np.int32)
        S = np.empty((6 * len(bn), 6 * len(bn)), np.float64)
        if block is None:
            _check(self._lib, self._lib.pl_schur(self._h, _ptr(bn), len(bn), float(rtol), int(max_iter), _ptr(S)))
        else:
            _check(self._lib, self._lib.pl_schur_block(self._h, _ptr(bn), len(bn), float(rtol), int(max_iter), int(block),
                                                       _ptr(S)))
        return S

    # -- several right-hand sides in one pass -------------------------------------------------------------
    def _columns(self, name, a, k=None):
        """a as a contiguous (k, 6 N) array: (k, N, 6), (k, 6 N), or one column (N, 6) / (6 N,)."""
        n6 = 6 * self.n_nodes
        a = np.asarray(a, dtype=np.float64)
        if a.shape in ((self.n_nodes, 6), (n6,)):
            a = a.reshape(1, n6)
        elif a.ndim == 3 and a.shape[1:] == (self.n_nodes, 6):
            a = a.reshape(a.shape[0], n6)
        elif not (a.ndim == 2 and a.shape[1] == n6):
            raise ValueError(f"{name} must have shape (k, {self.n_nodes}, 6) or (k, {n6}), got {a.shape}")
        if not 1 <= a.shape[0] <= MULTI_MAX:
            raise ValueError(f"{name}: 1 ... {MULTI_MAX} columns per call, got {a.shape[0]}")
        if k is not None and a.shape[0] != k:
            raise ValueError(f"{name} has {a.shape[0]} columns, {k} expected")
        return np.ascontiguousarray(a)

    def spmv_multi(self, X, masked=False):
        """Y[j] = K X[j] for k columns in one launch (pl_spmv_multi); masked: P K P X[j] under the mask of set_bc.
        X (k, N, 6) or (k, 6 N); returns (k, N, 6)."""
        x = self._columns("X", X)
        y = np.empty_like(x)
        _check(self._lib, self._lib.pl_spmv_multi(self._h, x.shape[0], int(bool(masked)), _ptr(x), _ptr(y)))
        return y.reshape(x.shape[0], self.n_nodes, 6)

    def solve_multi(self, ubar=None, f=None, rtol=1e-8, max_iter=20000, raise_on_noconv=True):
        """K u_j = f_j for k columns in one Jacobi-PCG pass under the Dirichlet mask of the last set_bc (pl_solve_multi):
        ubar (k, N, 6) prescribed values (read where fixed; None = 0), f (k, N, 6) loads (None = 0), at least one of them.
        Returns (U (k, N, 6), [stats of every column]).  The handle's single-column state is not touched."""
        if ubar is None and f is None:
            raise ValueError("solve_multi needs ubar or f (they give the number of columns)")
        ub = None if ubar is None else self._columns("ubar", ubar)
        ff = None if f is None else self._columns("f", f, None if ub is None else ub.shape[0])
        k = (ub if ub is not None else ff).shape[0]
        u = np.empty((k, 6 * self.n_nodes), np.float64)
        st = (PlStats * k)()
        for s in st:
            s.struct_size = C.sizeof(PlStats)
        rc = self._lib.pl_solve_multi(self._h, k, _ptr(ub), _ptr(ff), float(rtol), int(max_iter), _ptr(u), st)
        keys = [n for n, _ in PlStats._fields_ if n not in ("reserved", "reserved_i", "struct_size")]
        stats = [{n: getattr(s, n) for n in keys} for s in st]
        if rc in (PL_OK, PL_ERR_NOCONV):
            _timing.device("pl_solve_multi: PCG (HIP events)", st[0].ms_solve)
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        return u.reshape(k, self.n_nodes, 6), stats

    # -- global linear buckling ---------------------------------------------------------------------------
    def geom_spmv_multi(self, X, u=None, masked=False):
        """Y[j] = K_g(u) X[j] for k columns in one launch (pl_geom_spmv_multi), K_g the geometric stiffness of the struts'
        axial forces in u (None: the solution of the last solve()); masked: P K_g P X[j] under the mask of set_bc.
        X (k, N, 6) or (k, 6 N); returns (k, N, 6)."""
        x = self._columns("X", X)
        u = self._opt_vec6(u)
        y = np.empty_like(x)
        _check(self._lib, self._lib.pl_geom_spmv_multi(self._h, _ptr(u), x.shape[0], int(bool(masked)), _ptr(x), _ptr(y)))
        return y.reshape(x.shape[0], self.n_nodes, 6)

    def buckling_modes(self, n_modes=4, u=None, n_sub=0, rtol=1e-10, max_iter=200000, tol=1e-9, max_outer=200,
                       raise_on_noconv=True):
        """The n_modes smallest positive load factors of (K + lambda K_g(u)) phi = 0 on the free dofs of set_bc and their
        modes (pl_buckling_modes): dict with load_factor (n_modes,) ascending, modes (n_modes, N, 6) (phi^T K phi = 1,
        largest component positive), residual (n_modes,), n_found and outer_iterations; entries beyond n_found are NaN.
        u = None: the solution of the last solve().  n_sub: columns of the subspace iteration (0 = the library's choice);
        rtol, max_iter: its inner PCG; tol, max_outer: its stopping rule."""
        u = self._opt_vec6(u)
        n_modes = int(n_modes)
        lam = np.empty(max(n_modes, 0), np.float64)
        modes = np.empty((max(n_modes, 0), self.n_nodes, 6), np.float64)
        res = np.empty(max(n_modes, 0), np.float64)
        found, outer = C.c_int32(), C.c_int32()
        rc = self._lib.pl_buckling_modes(self._h, _ptr(u), n_modes, int(n_sub), float(rtol), int(max_iter), float(tol),
                                         int(max_outer), _ptr(lam), _ptr(modes), _ptr(res), C.byref(found), C.byref(outer))
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        return {"load_factor": lam, "modes": modes, "residual": res, "n_found": found.value,
                "outer_iterations": outer.value}

    def buckling_modes_sens(self, load_factor, modes, u=None, rtol=1e-12, max_iter=200000, weights=None, want_rows=True,
                            want_load=False, raise_on_noconv=True):
        """Sensitivities of the load factors of ``buckling_modes`` to the strut radii (pl_buckling_modes_sens), total: the
        adjoint solves for u(r) run inside the call, all modes in one PCG pass (rtol, max_iter).  load_factor (n_modes,) and
        modes (n_modes, N, 6) as ``buckling_modes`` returns them (any scaling; a NaN factor marks a mode to skip).  Returns a
        dict with dlam_dr (n_modes, B) if want_rows, dsum_dr (B,) = weights @ dlam_dr formed on the device if weights is
        given, adj_load (n_modes, N, 6) = d(phi^T K_g(u) phi)/du if want_load.  Rows of a repeated factor are not derivatives
        one by one; a sum with equal weights over the whole cluster is.  u = None: the solution of the last solve()."""
        lam = np.ascontiguousarray(np.asarray(load_factor, dtype=np.float64).reshape(-1))
        k = lam.size
        phi = np.ascontiguousarray(np.asarray(modes, dtype=np.float64)).reshape(-1)
        if phi.size != k * 6 * self.n_nodes:
            raise ValueError(f"modes must have shape ({k}, {self.n_nodes}, 6)")
        u = self._opt_vec6(u)
        wts = None if weights is None else _f64(np.asarray(weights).reshape(-1), k)
        rows = np.empty((k, self.n_beams), np.float64) if want_rows else None
        dsum = np.empty(self.n_beams, np.float64) if wts is not None else None
        load = np.empty((k, self.n_nodes, 6), np.float64) if want_load else None
        rc = self._lib.pl_buckling_modes_sens(self._h, _ptr(u), k, _ptr(lam), _ptr(phi), float(rtol), int(max_iter), _ptr(wts),
                                              _ptr(rows), _ptr(dsum), _ptr(load))
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        out = {}
        if want_rows:
            out["dlam_dr"] = rows
        if wts is not None:
            out["dsum_dr"] = dsum
        if want_load:
            out["adj_load"] = load
        return out

    def geom_spmv_multi_host(self, X, u, masked=False, fixed=None):
        """The numpy restatement of ``geom_spmv_multi`` (geometric_host.geometric_apply) on this handle's records; the
        masked product needs the mask ``fixed`` (N, 6) that was given to set_bc."""
        from . import geometric_host as GH
        if masked and fixed is None:
            raise ValueError("the masked product needs the mask given to set_bc")
        x = self._columns("X", X).reshape(-1, self.n_nodes, 6)
        return GH.geometric_apply(self.records(), self.beam_conn, u, x, fixed if masked else None)

    def buckling_modes_host(self, u, fixed, n_modes=4, n_sub=0, tol=1e-9, max_outer=200, dense=False):
        """The scipy restatement of ``buckling_modes`` on this handle's records: geometric_host.buckling_modes_subspace
        (exact solves), or buckling_modes_dense with dense=True.  fixed (N, 6): the mask that was given to set_bc."""
        from . import geometric_host as GH
        rec = self.records()
        K = GH.elastic_matrix(rec, self.beam_conn, self.n_nodes)
        Kg = GH.geometric_matrix(rec, self.beam_conn, u, self.n_nodes)
        if dense:
            return GH.buckling_modes_dense(K, Kg, fixed, n_modes)
        return GH.buckling_modes_subspace(K, Kg, fixed, n_modes, n_sub, tol, max_outer)

    # -- natural frequencies ------------------------------------------------------------------------------
    def set_mass(self, density, rotary=True, node_mass=None):
        """Mass model of the handle (pl_set_mass): the consistent mass of the struts at ``density``, with the rotary inertia
        of bending if ``rotary``, plus optional translational point masses node_mass (N,) >= 0.  The strut masses follow
        later update_radii / set_multiplicity calls by themselves."""
        nm = None if node_mass is None else _f64(np.asarray(node_mass).reshape(-1), self.n_nodes)
        _check(self._lib, self._lib.pl_set_mass(self._h, float(density), int(bool(rotary)), _ptr(nm)))
        self._mass = (float(density), bool(rotary), nm)

    def mass_spmv_multi(self, X, masked=False):
        """Y[j] = M X[j] for k columns in one launch (pl_mass_spmv_multi), M the consistent mass of ``set_mass``; masked:
        P M P X[j] under the mask of set_bc.  X (k, N, 6) or (k, 6 N); returns (k, N, 6)."""
        x = self._columns("X", X)
        y = np.empty_like(x)
        _check(self._lib, self._lib.pl_mass_spmv_multi(self._h, x.shape[0], int(bool(masked)), _ptr(x), _ptr(y)))
        return y.reshape(x.shape[0], self.n_nodes, 6)

    def vibration_modes(self, n_modes=4, n_sub=0, rtol=1e-10, max_iter=200000, tol=1e-9, max_outer=200,
                        raise_on_noconv=True):
        """The n_modes smallest omega^2 of K phi = omega^2 M phi on the free dofs of set_bc and their modes
        (pl_vibration_modes): dict with omega2 (n_modes,) ascending, modes (n_modes, N, 6) (phi^T M phi = 1, largest
        component positive), residual (n_modes,), n_found and outer_iterations; entries beyond n_found are NaN.  n_sub:
        columns of the subspace iteration (0 = the library's choice); rtol, max_iter: its inner PCG; tol, max_outer: its
        stopping rule."""
        n_modes = int(n_modes)
        om2 = np.empty(max(n_modes, 0), np.float64)
        modes = np.empty((max(n_modes, 0), self.n_nodes, 6), np.float64)
        res = np.empty(max(n_modes, 0), np.float64)
        found, outer = C.c_int32(), C.c_int32()
        rc = self._lib.pl_vibration_modes(self._h, n_modes, int(n_sub), float(rtol), int(max_iter), float(tol), int(max_outer),
                                          _ptr(om2), _ptr(modes), _ptr(res), C.byref(found), C.byref(outer))
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        return {"omega2": om2, "modes": modes, "residual": res, "n_found": found.value, "outer_iterations": outer.value}

    def vibration_modes_sens(self, omega2, modes, weights=None, want_rows=True):
        """Sensitivities of the omega^2 of ``vibration_modes`` to the strut radii (pl_vibration_modes_sens), one pass over
        the struts and no solve.  omega2 (n_modes,) and modes (n_modes, N, 6) as ``vibration_modes`` returns them (any
        scaling; a NaN omega2 marks a mode to skip).  Returns a dict with domega2_dr (n_modes, B) if want_rows and dsum_dr
        (B,) = weights @ domega2_dr formed on the device if weights is given.  Rows of a repeated frequency are not
        derivatives one by one; a sum with equal weights over the whole cluster is."""
        om2 = np.ascontiguousarray(np.asarray(omega2, dtype=np.float64).reshape(-1))
        k = om2.size
        phi = np.ascontiguousarray(np.asarray(modes, dtype=np.float64)).reshape(-1)
        if phi.size != k * 6 * self.n_nodes:
            raise ValueError(f"modes must have shape ({k}, {self.n_nodes}, 6)")
        wts = None if weights is None else _f64(np.asarray(weights).reshape(-1), k)
        rows = np.empty((k, self.n_beams), np.float64) if want_rows else None
        dsum = np.empty(self.n_beams, np.float64) if wts is not None else None
        _check(self._lib, self._lib.pl_vibration_modes_sens(self._h, k, _ptr(om2), _ptr(phi), _ptr(wts), _ptr(rows), _ptr(dsum)))
        out = {}
        if want_rows:
            out["domega2_dr"] = rows
        if wts is not None:
            out["dsum_dr"] = dsum
        return out

    def _mass_model(self):
        if getattr(self, "_mass", None) is None:
            raise ValueError("call set_mass first")
        return self._mass

    def mass_spmv_multi_host(self, X, masked=False, fixed=None):
        """The numpy restatement of ``mass_spmv_multi`` (mass_host.mass_apply) on this handle's geometry, radii and
        multiplicities; the masked product needs the mask ``fixed`` (N, 6) that was given to set_bc."""
        from . import mass_host as MH
        if masked and fixed is None:
            raise ValueError("the masked product needs the mask given to set_bc")
        rho, rotary, nm = self._mass_model()
        x = self._columns("X", X).reshape(-1, self.n_nodes, 6)
        return MH.mass_apply(self.node_xyz, self.beam_conn, self._radius, rho, x, self._mult, rotary, nm,
                             fixed if masked else None)

    def mass_matrix_host(self):
        """The sparse restated M (mass_host.mass_matrix) of this handle's geometry, radii, multiplicities and mass model."""
        from . import mass_host as MH
        rho, rotary, nm = self._mass_model()
        return MH.mass_matrix(self.node_xyz, self.beam_conn, self._radius, rho, self._mult, rotary, nm)

    def vibration_modes_host(self, fixed, n_modes=4, n_sub=0, tol=1e-9, max_outer=200, dense=False):
        """The scipy restatement of ``vibration_modes`` on this handle's records: mass_host.vibration_modes_subspace (exact
        solves), or vibration_modes_dense with dense=True.  fixed (N, 6): the mask that was given to set_bc."""
        from . import geometric_host as GH
        from . import mass_host as MH
        K = GH.elastic_matrix(self.records(), self.beam_conn, self.n_nodes)
        M = self.mass_matrix_host()
        if dense:
            return MH.vibration_modes_dense(K, M, fixed, n_modes)
        return MH.vibration_modes_subspace(K, M, fixed, n_modes, n_sub, tol, max_outer)

    def vibration_modes_sens_host(self, omega2, modes, fixed):
        """The numpy restatement of ``vibration_modes_sens`` (mass_host.vibration_sensitivity)."""
        from . import mass_host as MH
        from . import stress_host as SH
        rho, rotary, nm = self._mass_model()
        E, nu, kappa, pen = self._material
        drec = SH.drecords_dr(self.node_xyz, self.beam_conn, self._radius, self._seg_len, self._seg_nsub, E, nu, kappa, pen,
                              self._mult)
        return MH.vibration_sensitivity(self.node_xyz, self.beam_conn, self._radius, rho, drec, fixed, omega2, modes,
                                        self._mult, rotary, nm)

    # -- transient response -------------------------------------------------------------------------------
    def dyn_spmv_multi(self, c_K, c_M, X, masked=False):
        """Y[j] = c_K K X[j] + c_M M X[j] for k columns in one fused gather (pl_dyn_spmv_multi), M the consistent mass of
        ``set_mass``; masked: P (...) P X[j] under the mask of set_bc.  X (k, N, 6) or (k, 6 N); returns (k, N, 6)."""
        x = self._columns("X", X)
        y = np.empty_like(x)
        _check(self._lib, self._lib.pl_dyn_spmv_multi(self._h, float(c_K), float(c_M), x.shape[0], int(bool(masked)), _ptr(x),
                                                      _ptr(y)))
        return y.reshape(x.shape[0], self.n_nodes, 6)

    def transient(self, dt, n_steps, patterns=None, amp=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0, ray_k=0.0,
                  rtol=1e-10, max_iter=100000, probes=None, snap_every=0, want_state=True):
        """n_steps implicit Newmark steps of M a + (ray_m M + ray_k K) v + K u = amp[n] @ patterns on the free dofs of
        set_bc (pl_transient).  patterns (n_pat, N, 6), n_pat <= 4, amp (n_steps + 1, n_pat); u0, v0 (N, 6) or None = 0;
        probes: node indices.  Returns a dict: time (n_steps + 1,), probe (n_steps + 1, 3, n_probe, 6) = u, v, a of the
        probed nodes, energy (n_steps + 1, 3) = kinetic, strain, external work, iters (n_steps + 1,), state (3, N, 6) = the
        last u, v, a, and snaps (n_steps // snap_every, N, 6) if snap_every > 0."""
        n_steps, n6 = int(n_steps), 6 * self.n_nodes
        rows = max(n_steps, 0) + 1
        pat = am = None
        n_pat = 0
        if patterns is not None:
            pat = np.ascontiguousarray(np.asarray(patterns, dtype=np.float64)).reshape(-1, n6)
            n_pat = pat.shape[0]
            am = np.ascontiguousarray(np.asarray(amp, dtype=np.float64).reshape(-1))
            if am.size != rows * n_pat:
                raise ValueError(f"amp must have shape ({rows}, {n_pat})")
        uu = self._opt_vec6(u0)
        vv = self._opt_vec6(v0)
        pr = np.zeros(0, np.int32) if probes is None else np.ascontiguousarray(np.asarray(probes).reshape(-1), dtype=np.int32)
        probe = np.zeros((rows, 3, pr.size, 6), np.float64)
        energy = np.zeros((rows, 3), np.float64)
        iters = np.zeros(rows, np.int32)
        snap_every = int(snap_every)
        snaps = np.zeros((n_steps // snap_every, self.n_nodes, 6), np.float64) if snap_every > 0 and n_steps > 0 else None
        state = np.zeros((3, self.n_nodes, 6), np.float64) if want_state else None
        _check(self._lib, self._lib.pl_transient(self._h, n_steps, float(dt), float(beta), float(gamma), float(ray_m),
                                                 float(ray_k), n_pat, _ptr(pat), _ptr(am), _ptr(uu), _ptr(vv), float(rtol),
                                                 int(max_iter), pr.size, _ptr(pr) if pr.size else None,
                                                 _ptr(probe) if pr.size else None, _ptr(energy), snap_every, _ptr(snaps),
                                                 _ptr(state), _ptr(iters)))
        out = {"time": float(dt) * np.arange(rows), "probe": probe, "energy": energy, "iters": iters}
        if want_state:
            out["state"] = state
        if snaps is not None:
            out["snaps"] = snaps
        return out

    def transient_host(self, fixed, dt, n_steps, patterns=None, amp=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0,
                       ray_k=0.0, solve=None, probes=None, snap_every=0):
        """The numpy / scipy restatement of ``transient`` (dynamics_host.newmark) on this handle's own BSR K and the restated
        M of its mass model.  fixed (N, 6): the mask that was given to set_bc."""
        import scipy.sparse as sp
        from . import dynamics_host as DH
        self.assemble_bsr(False)
        rowptr, col, vals = self.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * self.n_nodes, 6 * self.n_nodes)).tocsr()
        K.sum_duplicates()
        return DH.newmark(K, self.mass_matrix_host(), fixed, dt, n_steps, patterns, amp, u0, v0, beta, gamma, ray_m, ray_k,
                          solve, probes, snap_every)

    def transient_sens(self, dt, n_steps, out_vec, kind=2, p=8.0, weight=None, patterns=None, amp=None, base_dir=None,
                       base_acc=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0, ray_k=0.0, rtol=1e-10,
                       max_iter=100000):
        """The run of ``transient`` with one output per row y_n = out_vec . u_n, the objective J of the outputs (kind 0:
        sum w y, 1: 1/2 sum w y^2, 2: (sum w |y|^p)^(1/p); weight (n_steps + 1,) >= 0 or None = 1) and dJ/dr for every
        strut radius by the discrete adjoint of the scheme (pl_transient_sens).  out_vec (N, 6), read with the fixed dofs
        zeroed; base_dir (3,) with base_acc (n_steps + 1,) adds the load -base_acc[n] M e_dir, which follows the design.
        Returns a dict: J, y (n_steps + 1,), dJ_dr (B,), iters (2, n_steps + 1) = forward, adjoint."""
        n_steps, n6 = int(n_steps), 6 * self.n_nodes
        rows = max(n_steps, 0) + 1
        pat = am = None
        n_pat = 0
        if patterns is not None:
            pat = np.ascontiguousarray(np.asarray(patterns, dtype=np.float64)).reshape(-1, n6)
            n_pat = pat.shape[0]
            am = np.ascontiguousarray(np.asarray(amp, dtype=np.float64).reshape(-1))
            if am.size != rows * n_pat:
                raise ValueError(f"amp must have shape ({rows}, {n_pat})")
        bd = None if base_dir is None else _f64(np.asarray(base_dir).reshape(-1), 3)
        ba = None if base_acc is None else _f64(np.asarray(base_acc).reshape(-1), rows)
        uu = self._opt_vec6(u0)
        vv = self._opt_vec6(v0)
        lv = _f64(np.asarray(out_vec).reshape(-1), n6)
        wt = None if weight is None else _f64(np.asarray(weight).reshape(-1), rows)
        J = C.c_double()
        y = np.zeros(rows, np.float64)
        grad = np.zeros(self.n_beams, np.float64)
        iters = np.zeros((2, rows), np.int32)
        _check(self._lib, self._lib.pl_transient_sens(self._h, n_steps, float(dt), float(beta), float(gamma), float(ray_m),
                                                      float(ray_k), n_pat, _ptr(pat), _ptr(am), _ptr(bd), _ptr(ba), _ptr(uu),
                                                      _ptr(vv), float(rtol), int(max_iter), _ptr(lv), int(kind), float(p),
                                                      _ptr(wt), C.byref(J), _ptr(y), _ptr(grad), _ptr(iters)))
        return {"J": J.value, "y": y, "dJ_dr": grad, "iters": iters}

    def transient_sens_host(self, fixed, dt, n_steps, out_vec, kind=2, p=8.0, weight=None, patterns=None, amp=None,
                            base_dir=None, base_acc=None, u0=None, v0=None, beta=0.25, gamma=0.5, ray_m=0.0, ray_k=0.0,
                            solve=None):
        """The numpy / scipy restatement of ``transient_sens`` (dynamics_host.newmark_sensitivity) on this handle's own BSR
        K, the restated M of its mass model and the restated record and mass derivatives.  fixed (N, 6): the mask that was
        given to set_bc."""
        import scipy.sparse as sp
        from . import dynamics_host as DH
        from . import mass_host as MH
        from . import stress_host as SH
        self.assemble_bsr(False)
        rowptr, col, vals = self.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * self.n_nodes, 6 * self.n_nodes)).tocsr()
        K.sum_duplicates()
        rho, rotary, nm = self._mass_model()
        E, nu, kappa, pen = self._material
        drec = SH.drecords_dr(self.node_xyz, self.beam_conn, self._radius, self._seg_len, self._seg_nsub, E, nu, kappa, pen,
                              self._mult)
        conn = np.asarray(self.beam_conn).reshape(-1, 2)
        xyz = np.asarray(self.node_xyz, dtype=np.float64).reshape(-1, 3)
        dM = MH.delement_matrix_dr(xyz[conn[:, 1]] - xyz[conn[:, 0]], np.asarray(self._radius, dtype=np.float64).reshape(-1),
                                   rho, self._mult, rotary)
        return DH.newmark_sensitivity(K, self.mass_matrix_host(), fixed, conn, drec, dM, dt, n_steps, out_vec, kind, p, weight,
                                      patterns, amp, base_dir, base_acc, u0, v0, beta, gamma, ray_m, ray_k, solve)

    # -- measurement ------------------------------------------------------------------------------------
    # -- frequency response -------------------------------------------------------------------------------
    def harm_spmv(self, coef, X, masked=False):
        """Y[k] = (cK[k] K + cM[k] M) X[k] for k complex vectors in one fused gather (pl_harm_spmv).  coef (k, 2) complex =
        (cK, cM) per vector, or (k, 4) real = Re cK, Im cK, Re cM, Im cM; X (k, N, 6) or (k, 6 N) complex; masked: P (...) P X[k]
        under the mask of set_bc.  Returns (k, N, 6) complex."""
        n6 = 6 * self.n_nodes
        x = np.ascontiguousarray(np.asarray(X, dtype=np.complex128)).reshape(-1, n6)
        k = x.shape[0]
        c = np.asarray(coef)
        c = (np.ascontiguousarray(c, dtype=np.complex128).reshape(k, 2).view(np.float64) if np.iscomplexobj(c)
             else np.ascontiguousarray(c, dtype=np.float64))
        if c.size != 4 * k:
            raise ValueError(f"coef must have shape ({k}, 2) complex or ({k}, 4) real")
        c = np.ascontiguousarray(c.reshape(k, 4))
        y = np.empty_like(x)
        _check(self._lib, self._lib.pl_harm_spmv(self._h, k, _ptr(c), int(bool(masked)), _ptr(x), _ptr(y)))
        return y.reshape(k, self.n_nodes, 6)

    def harmonic(self, omegas, load, ray_m=0.0, ray_k=0.0, probes=None, fields=False, rtol=1e-10, max_iter=20000, block=0,
                 raise_on_noconv=True):
        """The steady state u e^{iwt} under load e^{iwt} for every w of ``omegas`` (pl_harmonic):
        ((1 + i w ray_k) K + (i w ray_m - w^2) M) u = load on the free dofs of set_bc, one Jacobi-preconditioned COCG solve per
        frequency, ``block`` frequencies in lock step per pass (0 = 32).  load (N, 6) real or complex; probes: node indices.
        Returns a dict: omega (n_freq,), probe (n_freq, n_probe, 6) complex, power (n_freq, 4) = Re f^T u, Im f^T u, u^H K u,
        u^H M u, iters, relres and status (n_freq,; 0 converged, 1 max_iter, 2 breakdown), and fields (n_freq, N, 6) complex if
        ``fields``.  Without raise_on_noconv a frequency that did not converge only shows in status."""
        w = np.ascontiguousarray(np.atleast_1d(np.asarray(omegas, dtype=np.float64)).reshape(-1))
        nf, n6 = w.size, 6 * self.n_nodes
        ld = np.asarray(load)
        if ld.size != n6:
            raise ValueError(f"load must have shape ({self.n_nodes}, 6)")
        lre = np.ascontiguousarray(ld.real, dtype=np.float64).reshape(-1)
        lim = np.ascontiguousarray(ld.imag, dtype=np.float64).reshape(-1) if np.iscomplexobj(ld) else None
        pr = np.zeros(0, np.int32) if probes is None else np.ascontiguousarray(np.asarray(probes).reshape(-1), dtype=np.int32)
        probe = np.zeros((nf, pr.size, 6), np.complex128)
        fld = np.zeros((nf, self.n_nodes, 6), np.complex128) if fields else None
        power = np.zeros((nf, 4), np.float64)
        iters = np.zeros(nf, np.int32)
        relres = np.zeros(nf, np.float64)
        status = np.zeros(nf, np.int32)
        rc = self._lib.pl_harmonic(self._h, nf, _ptr(w), float(ray_m), float(ray_k), _ptr(lre), _ptr(lim), pr.size,
                                   _ptr(pr) if pr.size else None, float(rtol), int(max_iter), int(block),
                                   _ptr(probe) if pr.size else None, _ptr(fld), _ptr(power), _ptr(iters), _ptr(relres),
                                   _ptr(status))
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        out = {"omega": w, "probe": probe, "power": power, "iters": iters, "relres": relres, "status": status}
        if fields:
            out["fields"] = fld
        return out

    def harmonic_host(self, fixed, omegas, load, ray_m=0.0, ray_k=0.0, solver=None):
        """The numpy / scipy restatement of ``harmonic`` (dynamics_host.harmonic) on this handle's own BSR K and the restated M
        of its mass model.  fixed (N, 6): the mask that was given to set_bc."""
        import scipy.sparse as sp
        from . import dynamics_host as DH
        self.assemble_bsr(False)
        rowptr, col, vals = self.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * self.n_nodes, 6 * self.n_nodes)).tocsr()
        K.sum_duplicates()
        return DH.harmonic(K, self.mass_matrix_host(), fixed, omegas, load, ray_m, ray_k, solver)

    def harmonic_sens(self, omegas, load, out_vec=None, kind=2, p=8.0, weight=None, base_dir=None, ray_m=0.0, ray_k=0.0,
                      rtol=1e-10, max_iter=20000, block=0, raise_on_noconv=True):
        """The solves of ``harmonic`` with one complex output per frequency y_k = out_vec^T u_k (unconjugated), the objective J
        of the outputs (kind 0: -sum w Im y, 1: 1/2 sum w |y|^2, 2: (sum w |y|^p)^(1/p); weight (n_freq,) >= 0 or None = 1)
        and dJ/dr for every strut radius (pl_harmonic_sens).  load (N, 6) real or complex, or None with base_dir; base_dir
        (3,) adds the load -M e_dir of a base shaken with unit acceleration, which follows the design; out_vec (N, 6) real,
        read with the fixed dofs zeroed, or None: the whole load (no second solve).  ``block`` frequencies per pass (0 = the
        most: 16, or 32 with out_vec = None).  Returns a dict: omega, J, y (n_freq,) complex, dJ_dr (B,), iters, relres and
        status (2, n_freq) = forward, adjoint.  Without raise_on_noconv a solve that did not converge only shows in status,
        and J, y, dJ_dr are None."""
        w = np.ascontiguousarray(np.atleast_1d(np.asarray(omegas, dtype=np.float64)).reshape(-1))
        nf, n6 = w.size, 6 * self.n_nodes
        lre = lim = None
        if load is not None:
            ld = np.asarray(load)
            if ld.size != n6:
                raise ValueError(f"load must have shape ({self.n_nodes}, 6)")
            lre = np.ascontiguousarray(ld.real, dtype=np.float64).reshape(-1)
            lim = np.ascontiguousarray(ld.imag, dtype=np.float64).reshape(-1) if np.iscomplexobj(ld) else None
        bd = None if base_dir is None else _f64(np.asarray(base_dir).reshape(-1), 3)
        lv = None if out_vec is None else _f64(np.asarray(out_vec).reshape(-1), n6)
        wt = None if weight is None else _f64(np.asarray(weight).reshape(-1), nf)
        J = C.c_double()
        y = np.zeros(nf, np.complex128)
        grad = np.zeros(self.n_beams, np.float64)
        iters = np.zeros((2, nf), np.int32)
        relres = np.zeros((2, nf), np.float64)
        status = np.zeros((2, nf), np.int32)
        rc = self._lib.pl_harmonic_sens(self._h, nf, _ptr(w), float(ray_m), float(ray_k), _ptr(lre), _ptr(lim), _ptr(bd),
                                        _ptr(lv), int(kind), float(p), _ptr(wt), float(rtol), int(max_iter), int(block),
                                        C.byref(J), _ptr(y), _ptr(grad), _ptr(iters), _ptr(relres), _ptr(status))
        _check(self._lib, rc, allow=() if raise_on_noconv else (PL_ERR_NOCONV,))
        ok = rc == PL_OK
        return {"omega": w, "J": J.value if ok else None, "y": y if ok else None, "dJ_dr": grad if ok else None,
                "iters": iters, "relres": relres, "status": status}

    def harmonic_sens_host(self, fixed, omegas, load, out_vec=None, kind=2, p=8.0, weight=None, base_dir=None, ray_m=0.0,
                           ray_k=0.0, solver=None):
        """The numpy / scipy restatement of ``harmonic_sens`` (dynamics_host.harmonic_sensitivity) on this handle's own BSR K,
        the restated M of its mass model and the restated record and mass derivatives.  fixed (N, 6): the mask that was given
        to set_bc."""
        import scipy.sparse as sp
        from . import dynamics_host as DH
        from . import mass_host as MH
        from . import stress_host as SH
        self.assemble_bsr(False)
        rowptr, col, vals = self.get_bsr()
        K = sp.bsr_matrix((vals, col, rowptr), shape=(6 * self.n_nodes, 6 * self.n_nodes)).tocsr()
        K.sum_duplicates()
        rho, rotary, nm = self._mass_model()
        E, nu, kappa, pen = self._material
        drec = SH.drecords_dr(self.node_xyz, self.beam_conn, self._radius, self._seg_len, self._seg_nsub, E, nu, kappa, pen,
                              self._mult)
        conn = np.asarray(self.beam_conn).reshape(-1, 2)
        xyz = np.asarray(self.node_xyz, dtype=np.float64).reshape(-1, 3)
        dM = MH.delement_matrix_dr(xyz[conn[:, 1]] - xyz[conn[:, 0]], np.asarray(self._radius, dtype=np.float64).reshape(-1),
                                   rho, self._mult, rotary)
        return DH.harmonic_sensitivity(K, self.mass_matrix_host(), fixed, conn, drec, dM, omegas, load, out_vec, kind, p,
                                       weight, base_dir, ray_m, ray_k, solver)

    def time_kernel(self, which, reps=20):
        ms = C.c_double()
        _check(self._lib, self._lib.pl_time_kernel(self._h, int(which), int(reps), C.byref(ms)))
        return ms.value

    def node_words_info(self):
        """What the PCG vector kernels read per node on this handle: {"classes": bool, "n_classes": int, "bytes": bool,
        "byte_exp": int} (pl_node_words_info)."""
        v = [C.c_int() for _ in range(4)]
        _check(self._lib, self._lib.pl_node_words_info(self._h, *[C.byref(x) for x in v]))
        return {"classes": bool(v[0].value), "n_classes": v[1].value, "bytes": bool(v[2].value), "byte_exp": v[3].value}

    def algorithmic_bytes(self):
        out = (C.c_double * 3)()
        _check(self._lib, self._lib.pl_algorithmic_bytes(self._h, out))
        return {"spmv": out[0], "pcg_iter": out[1], "bsr": out[2]}

    def set_periodic(self, master):
        """Periodic constraints: master[i] = node whose six dofs node i shares (pl_set_periodic); None removes them."""
        m = None if master is None else np.ascontiguousarray(master, dtype=np.int32)
        if m is not None and m.size != self.n_nodes:
            raise ValueError(f"expected {self.n_nodes} entries, got {m.size}")
        _check(self._lib, self._lib.pl_set_periodic(self._h, _ptr(m)))

    def forget_history(self):
        """Drop the previous solve's iteration count (first look at the residual history) and the warm-start solution."""
        _check(self._lib, self._lib.pl_forget_history(self._h))

    # -- multi-GPU --------------------------------------------------------------------------------------
    @staticmethod
    def dist_unique_id() -> bytes:
        lib = load_library()
        n = lib.pl_dist_unique_id_bytes()
        buf = C.create_string_buffer(n)
        _check(lib, lib.pl_dist_unique_id(buf))
        return buf.raw

    @staticmethod
    def dist_loopback_id() -> bytes:
        """Id of a new in-process loopback group (pl_dist_loopback_id): `world` handles on one device, one host thread
        per rank - see ``pylatticedso_amd.loopback.LoopbackGroup``."""
        lib = load_library()
        buf = C.create_string_buffer(lib.pl_dist_unique_id_bytes())
        _check(lib, lib.pl_dist_loopback_id(buf))
        return buf.raw

    def dist_abort(self):
        """Break this handle's loopback group (ranks waiting at a collective return an error at once)."""
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.pl_dist_abort(self._h)

    def dist_init(self, rank, world, unique_id: bytes, shared_local, shared_global, n_shared_global, shared_peer=None):
        """Attach the handle to the RCCL communicator; ``shared_peer`` (rank on the other side of every shared entry)
        switches the interface rows from the all-planes all-reduce to the neighbour exchange (pl_dist_set_peers)."""
        sl = np.ascontiguousarray(shared_local, dtype=np.int32)
        sg = np.ascontiguousarray(shared_global, dtype=np.int32)
        buf = C.create_string_buffer(unique_id, len(unique_id))
        _check(self._lib, self._lib.pl_dist_init(self._h, int(rank), int(world), buf, _ptr(sl), _ptr(sg),
                                                 int(len(sl)), int(n_shared_global)))
        if shared_peer is not None:
            sp = np.ascontiguousarray(shared_peer, dtype=np.int32)
            if sp.shape != sl.shape:
                raise ValueError("one peer rank per shared entry expected")
            _check(self._lib, self._lib.pl_dist_set_peers(self._h, _ptr(sp)))


# the reference wraps every hot-path method in @timing.category(..) @timing.timeit; here the
# C-ABI calls are the hot path: host wall clock per call, plus the device's own HIP-event times (see solve)
for _name in ("assemble", "assemble_bsr", "get_bsr", "solve", "set_bc", "spmv", "spmv_free", "spmv_bsr", "reactions",
              "sens", "stress", "stress_pnorm", "buckling", "buckling_pnorm", "energy", "schur", "spmv_multi", "solve_multi", "geom_spmv_multi", "buckling_modes", "buckling_modes_sens", "mass_spmv_multi", "vibration_modes", "vibration_modes_sens", "dyn_spmv_multi", "transient", "update_radii", "update_segments", "records"):
    _f = getattr(HipLattice, _name, None)
    if _f is not None:
        _f._timing_category = "hip"
        setattr(HipLattice, _name, _timing.timeit(_f))
