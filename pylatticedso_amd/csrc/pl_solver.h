// PCG solvers of libpylattice_hip: ordinary multi-level / Jacobi / reference-CG loop, single-reduction form
// (Chronopoulos-Gear), fp32 solver modes.
#pragma once
#include <type_traits>

#include "pl_assembly.h"
#include "pl_schedule.h"
#include "pl_warm.h"

namespace {

int read_slots(pl_context *c, const double *dev, double *sum) {
  double h[pl::kSlots];
  PL_HIP(hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  *sum = 0.0;
  for (int k = 0; k < pl::kSlots; ++k) *sum += h[k];
  return PL_OK;
}

// Start of every solve: ||b||^2 from its slots, the stats of a solve that has not iterated yet.  *zero: the right-hand side
// is zero (or NaN) - the solve is over and the return value is its result.
int solve_begin(pl_context *c, const double *bb_slots, pl_stats_t *st, double *bb, bool *zero) {
  *zero = false;
  const int rc = read_slots(c, bb_slots, bb);
  if (rc) return rc;
  st->b_norm = std::sqrt(*bb);
  st->iterations = 0;
  st->converged = 0;
  st->rel_residual = 0.0;
  if (*bb > 0.0) return PL_OK;
  *zero = true;
  st->converged = 1;
  return std::isnan(*bb) ? fail(PL_ERR_NAN, "NaN in the right-hand side") : PL_OK;
}

inline void converged_at(pl_stats_t *st, int iterations, double stop_reason) {
  st->converged = 1;
  st->iterations = iterations;
  st->info = 0.0;
  st->stop_reason = stop_reason;
}

// ----------------------------------------------------------------------------------------------------------
// Launches of the iteration's tail kernels: every kernel's argument list is written once, in its launch_* function, and the
// compile-time variant is chosen by a dispatcher (pl_dispatch.h and the two below), which hands it to a generic lambda as
// constants.
// ----------------------------------------------------------------------------------------------------------
using pl::Int;
using pl::with_flag;

// f(tm): modes of the tile level, 6 or 12
template <typename F>
inline void with_tile_modes(const pl_context *c, F &&f) {
  if (tile_modes_now(c) == 12) f(Int<12>{});
  else f(Int<6>{});
}
// f(tm, multi, local): MULTI = several ranks or a rank-local dense level, LOCAL = the rank-local level (k_pcg_update_tile)
template <typename F>
inline void with_tail_variant(const pl_context *c, F &&f) {
  with_tile_modes(c, [&](auto tm) {
    if (c->coarseL.ready) f(tm, std::true_type{}, std::true_type{});
    else if (c->dist.active) f(tm, std::true_type{}, std::false_type{});
    else f(tm, std::false_type{}, std::false_type{});
  });
}

// Lever arms as exact floats where the lattice allows it (Coarse::rel32) and the node words (Coarse::nword): the class table
// of the Jacobi weights and / or the lever arms as bytes, whichever this handle has; neither (or PL_NODE_WORDS=0 at
// pl_create: no words): null, and the kernels read what they always read
struct NodeWords {
  const float *rel32;
  const uint32_t *nword, *dtab;
  double rscale;
};
inline NodeWords node_words_of(const pl_context *c) {
  const pl::Coarse &cs = c->coarse;
  const bool words = node_words_apply(c);
  NodeWords nw;
  nw.rel32 = cs.rel_exact ? (const float *)cs.rel32.p : (const float *)nullptr;
  nw.dtab = words && cs.dcl_ready ? (const uint32_t *)cs.dcl_table : (const uint32_t *)nullptr;
  nw.rscale = words && cs.rel_e >= 0 ? std::ldexp(1.0, -cs.rel_e) : 0.0;
  nw.nword = (nw.dtab || nw.rscale != 0.0) ? (const uint32_t *)cs.nword.p : (const uint32_t *)nullptr;
  return nw;
}

// r -= alpha Ap with the scalars of `scal`, restriction into rc_out, tile solve (the rank-local level has its own reference
// points)
template <typename PT, typename RT, int TM, bool MULTI, bool LOCAL>
void launch_update_tile(pl_context *c, Int<TM>, std::bool_constant<MULTI>, std::bool_constant<LOCAL>, const PT *Ap, RT *r,
                        double *scal, double *rc_out, const NodeWords &nw) {
  pl::Coarse &cs = c->coarse, &cl = c->coarseL;
  hipLaunchKernelGGL((pl::k_pcg_update_tile<PT, RT, TM, MULTI, LOCAL>), dim3((unsigned)cs.n_tiles), dim3(cs.vblock), 0,
                     c->stream, c->tile.tile_start.p, cs.agg_of_tile.p, cs.cen.p, c->xyz.p, Ap, cs.dinv32,
                     c->dist.active ? (const double *)c->dist.weight.p : (const double *)nullptr, r, scal, rc_out,
                     cs.tile_level ? (const double *)cs.Bt_inv : (const double *)nullptr, cs.yt,
                     LOCAL ? (const int32_t *)cl.agg_of_tile.p : (const int32_t *)nullptr,
                     LOCAL ? (const double *)cl.cen.p : (const double *)nullptr,
                     MULTI ? (const uint8_t *)c->sharedbits.p : (const uint8_t *)nullptr, LOCAL ? cl.rc : (double *)nullptr,
                     cs.ncp, c->cond_use ? (const uint8_t *)c->cflag.p : (const uint8_t *)nullptr, cs.cm, nw.rel32, nw.nword,
                     nw.dtab, nw.rscale);
}
template <typename PT, typename RT, int TM, bool MULTI, bool LOCAL>
void launch_direction_coarse(pl_context *c, Int<TM>, std::bool_constant<MULTI>, std::bool_constant<LOCAL>, PT *p, RT *x,
                             const RT *r, double *cur, double *nxt, int hist_slot, const NodeWords &nw) {
  pl::Coarse &cs = c->coarse, &cl = c->coarseL;
  hipLaunchKernelGGL((pl::k_pcg_direction_coarse<PT, RT, TM, MULTI, LOCAL>), dim3((unsigned)cs.n_tiles), dim3(cs.vblock), 0,
                     c->stream, c->tile.tile_start.p, r, cs.dinv32, c->xyz.p, cs.agg_of_tile.p, cs.cen.p, cs.yc,
                     cs.tile_level ? (const double *)cs.yt : (const double *)nullptr, c->fixedbits.p, p, x, cur, nxt,
                     c->hist.p, hist_slot, cs.rc, cs.ncp,
                     LOCAL ? (const int32_t *)cl.agg_of_tile.p : (const int32_t *)nullptr,
                     LOCAL ? (const double *)cl.cen.p : (const double *)nullptr,
                     LOCAL ? (const double *)cl.yc : (const double *)nullptr,
                     MULTI ? (const uint8_t *)c->sharedbits.p : (const uint8_t *)nullptr, LOCAL ? cl.rc : (double *)nullptr,
                     LOCAL ? cl.ncp : 0, c->cond_use ? (const uint8_t *)c->cflag.p : (const uint8_t *)nullptr, cs.cm,
                     nw.rel32, nw.nword, nw.dtab, nw.rscale);
}
// the same direction on a flat mapping, contiguous per wave (no rank-local level)
template <typename PT, typename RT, int TM>
void launch_direction_flat(pl_context *c, Int<TM>, PT *p, RT *x, const RT *r, double *cur, double *nxt, int hist_slot,
                           const NodeWords &nw) {
  pl::Coarse &cs = c->coarse;
  const int64_t n_flat = c->cond_use ? c->N - c->n_cond : c->N;       // nodes that are unknowns of this CG
  // what is fixed for the handle is compiled in: where the lever arms come from, the class table, the tile level, node
  // elimination, several ranks
  auto go = [&](auto arms, auto dt, auto yt, auto keep, auto sh) {
    hipLaunchKernelGGL((pl::k_pcg_direction_flat<PT, RT, TM, decltype(arms)::value, decltype(dt)::value, decltype(yt)::value,
                                                 decltype(keep)::value, decltype(sh)::value>),
                       dim3((unsigned)((3 * n_flat + pl::kBlock - 1) / pl::kBlock)), dim3(pl::kBlock), 0, c->stream, n_flat,
                       cs.tile_of_node.p, r, cs.dinv32, c->xyz.p, cs.agg_of_tile.p, cs.cen.p, cs.yc,
                       cs.tile_level ? (const double *)cs.yt : (const double *)nullptr, c->fixedbits.p, p, x, cur, nxt,
                       c->hist.p, hist_slot, cs.rc, cs.ncp,
                       c->cond_use ? (const int32_t *)c->ckeep.p : (const int32_t *)nullptr, cs.cm,
                       c->dist.active ? (const uint8_t *)c->sharedbits.p : (const uint8_t *)nullptr, nw.rel32, nw.nword,
                       nw.dtab, nw.rscale);
  };
  auto with_arms = [&](auto &&f) {
    if (nw.rscale != 0.0) f(Int<pl::kArmsBytes>{});
    else if (nw.rel32) f(Int<pl::kArmsRel32>{});
    else f(Int<pl::kArmsXyz>{});
  };
  with_arms([&](auto arms) {
    with_flag(nw.dtab != nullptr, [&](auto dt) {
      with_flag(cs.tile_level, [&](auto yt) {
        with_flag(c->cond_use, [&](auto keep) {
          with_flag(c->dist.active, [&](auto sh) { go(arms, dt, yt, keep, sh); });
        });
      });
    });
  });
}

// Everything of a two-level PCG iteration after K*p: update + restriction, coarse solve, new direction.
template <typename PT, typename RT>
int pcg_tail_coarse_t(pl_context *c, double *cur, double *nxt, int hist_slot, PT *p, const PT *Ap, RT *x, RT *r) {
  pl::Coarse &cs = c->coarse, &cl = c->coarseL;
  const bool useL = cl.ready;
  const NodeWords nw = node_words_of(c);
  with_tail_variant(c, [&](auto tm, auto multi, auto local) { launch_update_tile(c, tm, multi, local, Ap, r, cur, cs.rc, nw); });
  if (useL)   // rank-local level: y_L is never communicated, but its share of r.z, r_L . A_L^-1 r_L, is a per-rank
              // partial sum: it joins the r.D^-1 r slots BEFORE they travel in the collective below
    pl::coarse_apply(cl, cl.rc, cl.tv, cl.yc, cs.rc + cs.ncp + pl::kSlots, (const double *)nullptr, c->stream);
  if (c->dist.active) {   // one collective: [Z^T r | r.r slots | r.D^-1 r slots]; the coarse solve is then redundant per rank
    if (pl::dist_sum_scalars(c->dist, cs.rc, cs.ncp + 2 * pl::kSlots, c->stream))
      return fail(PL_ERR_HIP, "RCCL all-reduce of the coarse residual failed");
  }
  pl::coarse_apply(cs, cs.rc, cs.tv, cs.yc, cur + pl::S_RZ_NEW * pl::kSlots, cs.rc + cs.ncp + pl::kSlots, c->stream);
  // flat mapping: fp64 p without a rank-local level (measured on one box, 50^3 Octet: 26.2 -> 24.5 us;
  // fp32 p / fp64 r the same either way, fp32 p / fp32 r 19.0 -> 22.0 us - 8-byte loads per lane are too few in flight)
  bool flat = false;
  if constexpr (sizeof(PT) == 8) {
    if (!useL) {
      flat = true;
      with_tile_modes(c, [&](auto tm) { launch_direction_flat(c, tm, p, x, (const RT *)r, cur, nxt, hist_slot, nw); });
    }
  }
  if (!flat)
    with_tail_variant(c, [&](auto tm, auto multi, auto local) {
      launch_direction_coarse(c, tm, multi, local, p, x, (const RT *)r, cur, nxt, hist_slot, nw);
    });
  PL_HIP(hipGetLastError());
  return PL_OK;
}

int pcg_tail_coarse(pl_context *c, double *cur, double *nxt, int hist_slot) {
  return pcg_tail_coarse_t<double, double>(c, cur, nxt, hist_slot, c->p.p, (const double *)c->Ap.p, c->x.p, c->r.p);
}

// z = G^-1 r of a DDM handle (dense factor of the assembled matrix, or its inverted node blocks); dot[kSlots] += r.z
// (restricted = true: r_c already holds Z^T r - the iteration's fused update has summed it, k_ddm_update_restrict)
inline void ddm_precondition(pl_context *c, double *dot, bool restricted = false) {
  if (c->dd2_ready) {   // two-level: r_c = Z^T r, y_c = A_c^-1 r_c (dot += r_c . y_c), z = B^-1 r + P Z y_c (dot += r . B^-1 r)
    pl::Coarse &cs = c->dd2;
    const uint8_t *fx = c->have_bc ? (const uint8_t *)c->fixed.p : (const uint8_t *)nullptr;
    if (!restricted)
      hipLaunchKernelGGL(pl::k_ddm_restrict, dim3((unsigned)c->dd2_n_agg), dim3(pl::kBlock), 0, c->stream, c->dd2_ptr.p,
                         c->dd2_nodes.p, (const double *)c->dd2_cen.p, (const double *)c->dd2_xyz.p, fx,
                         (const double *)c->r.p, cs.rc);
    pl::coarse_apply(cs, cs.rc, cs.tv, cs.yc, dot, (const double *)nullptr, c->stream);
    hipLaunchKernelGGL(pl::k_ddm_two_level_apply, dim3(grid_for(c->N * 6)), dim3(pl::kBlock), 0, c->stream, c->N,
                       (const double *)c->dd_B.p, c->dd2_agg.p, (const double *)c->dd2_cen.p, (const double *)c->dd2_xyz.p, fx,
                       (const double *)cs.yc, (const double *)c->r.p, c->z.p, dot, cs.rc, cs.ncp);
    return;
  }
  if (c->dd_ready)
    pl::dense_apply(c->dd_W.p, c->dd_Wt.p, c->dd_n, c->dd_n, c->r.p, c->dd_tv.p, c->z.p, dot, (const double *)nullptr,
                    c->stream);
  else
    hipLaunchKernelGGL(pl::k_ddm_node_blocks_apply, dim3(grid_for(c->N * 6)), dim3(pl::kBlock), 0, c->stream, c->N,
                       (const double *)c->dd_B.p, (const double *)c->r.p, c->z.p, dot);
}

// ----------------------------------------------------------------------------------------------------------
// Short form of the iteration (pl_small.h): K*p with the direction formed in the kernel, update, z-kernel.
// ----------------------------------------------------------------------------------------------------------
inline int small_set_size() { return pl::S_COUNT * pl::kSlots; }
inline double *small_set(pl_context *c, int k) { return c->small_scal.p + (size_t)((k + 4) & 3) * small_set_size(); }
inline double *small_rc(pl_context *c, int parity) { return c->small_rc.p + (size_t)(parity & 1) * (c->coarse.ncp + 2 * pl::kSlots); }

// buffers of the short form, zeroed: scalar ring, both r_c buffers, p_old of iteration 0
int small_prepare(pl_context *c) {
  const int64_t n6 = c->N * 6;
  const size_t nrc = 2 * (size_t)(c->coarse.ncp + 2 * pl::kSlots);
  if (!c->p2.p || c->p2.n < (size_t)n6) PL_HIP(c->p2.alloc((size_t)n6));
  if (!c->small_scal.p) PL_HIP(c->small_scal.alloc(4 * (size_t)small_set_size()));
  if (!c->small_rc.p || c->small_rc.n < nrc) PL_HIP(c->small_rc.alloc(nrc));
  PL_HIP(hipMemsetAsync(c->small_scal.p, 0, 4 * (size_t)small_set_size() * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->small_rc.p, 0, nrc * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->p.p, 0, n6 * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->p2.p, 0, n6 * sizeof(double), c->stream));
  return PL_OK;
}

// update (r -= alpha Ap with the scalars of set k, restriction into the r_c buffer of parity k + 1, tile solve) and the
// z-kernel of iteration k (k = -1: the pass that prepares iteration 0, alpha = 0; its history entry goes to hist_slot)
template <int TM>
void launch_small_z(pl_context *c, Int<TM>, int k, int hist_slot) {
  pl::Coarse &cs = c->coarse;
  hipLaunchKernelGGL((pl::k_small_z<TM>), dim3((unsigned)cs.n_tiles), dim3(cs.vblock), 0, c->stream, c->tile.tile_start.p,
                     cs.agg_of_tile.p, cs.cen.p, c->xyz.p, (const double *)c->r.p, cs.dinv32, c->fixedbits.p,
                     c->cond_use ? (const uint8_t *)c->cflag.p : (const uint8_t *)nullptr, (const float *)cs.Ainv, cs.ncp, cs.cm,
                     (const double *)small_rc(c, k + 1), small_rc(c, k),
                     cs.tile_level ? (const double *)cs.yt : (const double *)nullptr, c->z.p, small_set(c, k + 1),
                     small_set(c, k + 2), c->hist.p, hist_slot);
}
int small_tail(pl_context *c, int k, int hist_slot) {
  // (one rank, no rank-local level: small_wanted; the short form reads neither exact lever arms nor node words)
  const NodeWords none = {(const float *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0.0};
  with_tile_modes(c, [&](auto tm) {
    launch_update_tile(c, tm, std::false_type{}, std::false_type{}, (const double *)c->Ap.p, c->r.p, small_set(c, k),
                       small_rc(c, k + 1), none);
    launch_small_z(c, tm, k, hist_slot);
  });
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// p_k = z_k + beta p_{k-1} is formed by the K*p launch of iteration k and stored in buffer k & 1 (p_{k-1} in the other one)
inline double *small_p_of(pl_context *c, int k) { return (k & 1) ? c->p2.p : c->p.p; }

int small_iteration(pl_context *c, int k) {
  pl::Defer df;
  df.z = c->z.p;
  df.p_old = small_p_of(c, k - 1);
  df.p_new = small_p_of(c, k);
  df.xsol = c->x.p;
  df.sc_prev = small_set(c, k - 1);
  df.sc_cur = small_set(c, k);
  double *dot = small_set(c, k) + pl::S_PAP * pl::kSlots;
  const bool stream_form = !c->pal_lds;
  const uint32_t *vw = stream_form ? c->vword_dir.p : c->vword.p;
  const void *tab = stream_form ? (const void *)c->tile.dir_table.p : (const void *)c->pal_dense.p;
  const int n_tab = stream_form ? c->tile.n_dir : c->pal_entries;
  const pl::Rec5 *r5 = stream_form ? reinterpret_cast<const pl::Rec5 *>(c->rec5.p) : (const pl::Rec5 *)nullptr;
  if (c->cond_use) {   // (the first pass of S p with the direction formed in the kernel, the second as in apply_operator)
    const pl::CondSolve cs = cond_solve(c, pl::kEndsCondensedSolve);
    if (!pl::launch_tile_spmv_lds<double>(c->tile, vw, tab, n_tab, r5, nullptr, nullptr, df.p_new, nullptr, c->stream,
                                          pl::kEndsCondensedSolve, c->cflag.p, cs, nullptr, 0, &df))
      return fail(PL_ERR_STATE, "short iteration: the LDS-resident K*p does not fit this lattice");
    int rc = launch_spmv(c, df.p_new, c->Ap.p, true, dot, c->maskC.p, pl::kEndsOthers);
    if (rc) return rc;
  } else {
    if (!pl::launch_tile_spmv_lds<double>(c->tile, vw, tab, n_tab, r5, c->fixedbits.p, nullptr, c->Ap.p, dot, c->stream,
                                          pl::kEndsAll, nullptr, pl::CondSolve(), nullptr, 0, &df))
      return fail(PL_ERR_STATE, "short iteration: the LDS-resident K*p does not fit this lattice");
  }
  return small_tail(c, k, k);
}

// x += alpha_{K-1} p_{K-1} after K iterations (the K*p launch of iteration K would have made it)
int small_finish(pl_context *c, int K) {
  if (K <= 0) return PL_OK;
  hipLaunchKernelGGL(pl::k_small_final_x, dim3(grid_stream(c->N * 6)), dim3(pl::kBlock), 0, c->stream, c->N,
                     c->cond_use ? (const uint8_t *)c->cflag.p : (const uint8_t *)nullptr,
                     (const double *)small_p_of(c, K - 1), (const double *)small_set(c, K - 1), c->x.p);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// v <- Q v (periodic constraints, pl_set_periodic)
inline void periodic_average(pl_context *c, double *v) {
  if (c->n_per_groups > 0)
    hipLaunchKernelGGL(pl::k_periodic_average, dim3(grid_for(6 * c->n_per_groups)), dim3(pl::kBlock), 0, c->stream,
                       c->n_per_groups, c->per_ptr.p, c->per_nodes.p, v);
}

// One PCG iteration (k = iteration index: selects the scalar set by parity and the residual-history slot).
int pcg_iteration(pl_context *c, int k) {
  if (c->small_use) return small_iteration(c, k);
  const int64_t n6 = c->N * 6;
  const int set = pl::S_COUNT * pl::kSlots;
  double *cur = c->scal.p + (k & 1) * set, *nxt = c->scal.p + ((k + 1) & 1) * set;
  int rc = apply_operator(c, c->p.p, c->Ap.p, cur + pl::S_PAP * pl::kSlots);
  if (rc) return rc;
  if (c->coarse.ready) return pcg_tail_coarse(c, cur, nxt, k);      // (node elimination: with the multi-level PCG only)
  periodic_average(c, c->Ap.p);        // (periodic constraints: the operator is Q K Q; p.Kp above is already p.QKQp)
  // reference-CG mode (conjugate_gradient_solver.py:79-109): every restart_every-th iteration the direction is rebuilt
  // on the PREVIOUS z (with a preconditioner; kept in tmp) or on the updated residual (without one: z aliases r there)
  const bool ref = ref_cg(c) && !c->dist.active;
  const bool restart = ref && c->opt.restart_every > 0 && k > 0 && (k % c->opt.restart_every) == 0;
  const bool has_M = c->dd_ready || c->dd_blocks || c->opt.precond >= 1;
  const double *pn = c->p.p, *psrc = nullptr;
  if (restart) {
    if (has_M) {
      PL_HIP(hipMemcpyAsync(c->tmp.p, c->z.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      pn = psrc = c->tmp.p;
    } else {
      pn = nullptr;        // ||r_new||
      psrc = c->z.p;       // = r_new once the update kernel has run (dinv = 1 on free dofs)
    }
  }
  const int hcap = ref ? c->hist_cap : 0;
  int *stop = c->stop_use ? c->stop_flag.p : (int *)nullptr;     // (DDM handles: the device stops itself, k_pcg_direction)
  const double stop_mintol = ref ? c->opt.mintol : 0.0;
  const double *pn_upd = ref ? pn : (const double *)nullptr;
  const auto update = [&] {            // x += alpha p, r -= alpha Ap, z = D^-1 r (DDM: dinv = 0 leaves z = 0, r.z = 0)
    const auto kern = ref ? pl::k_pcg_update<true> : pl::k_pcg_update<false>;
    hipLaunchKernelGGL(kern, dim3(grid_stream(n6 / 2)), dim3(pl::kBlock), 0, c->stream, n6, c->p.p, c->Ap.p, c->dinv.p,
                       c->x.p, c->r.p, c->z.p, cur, c->opt.alpha_max, pn_upd, (const int *)stop);
  };
  const auto direction = [&]() -> int {
    hipLaunchKernelGGL(pl::k_pcg_direction, dim3(grid_stream(n6 / 2)), dim3(pl::kBlock), 0, c->stream, n6, c->z.p,
                       c->p.p, cur, nxt, c->hist.p, k, psrc, hcap, stop, c->stop_thresh, stop_mintol);
    PL_HIP(hipGetLastError());
    return PL_OK;
  };
  if (c->dd2_ready) {                  // two-level DDM preconditioner: update and restriction in one pass over the aggregates
    const uint8_t *fx = c->have_bc ? (const uint8_t *)c->fixed.p : (const uint8_t *)nullptr;
    const auto kern = ref ? pl::k_ddm_update_restrict<true> : pl::k_ddm_update_restrict<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(c->dd2_n_agg * pl::kDdmSplit)), dim3(pl::kBlock), 0, c->stream, c->dd2_ptr.p,
                       c->dd2_nodes.p, (const double *)c->dd2_cen.p, (const double *)c->dd2_xyz.p, fx, (const double *)c->p.p,
                       (const double *)c->Ap.p, c->x.p, c->r.p, cur, c->opt.alpha_max, pn_upd, (const int *)stop, c->dd2.rc);
    ddm_precondition(c, cur + pl::S_RZ_NEW * pl::kSlots, true);
    return direction();
  }
  if (c->dd_ready || c->dd_blocks) {   // DDM with the factorised assembled matrix / its node blocks: then z = G^-1 r
    update();
    ddm_precondition(c, cur + pl::S_RZ_NEW * pl::kSlots);
    return direction();
  }
  if (c->dist.active) {
    pl::launch_pcg_update_weighted(n6, c->p.p, c->Ap.p, c->dinv.p, c->dist.weight.p, c->x.p, c->r.p, c->z.p, cur,
                                   c->stream);
    if (pl::dist_sum_scalars(c->dist, cur + pl::S_RZ_NEW * pl::kSlots, 2 * pl::kSlots, c->stream))
      return fail(PL_ERR_HIP, "RCCL all-reduce of the PCG scalars failed");
  } else {
    update();
  }
  periodic_average(c, c->z.p);         // z = Q D^-1 r (r.z was summed with the un-averaged D^-1 r: the same number, r = Q r)
  return direction();
}

// The PCG loop as one persistent launch (pl_persist.h): x, r hold the initial iterate and residual on entry, the result on exit.
int persist_solve(pl_context *c, double thresh, double bb, int max_iter, pl_stats_t *st) {
  pl::Coarse &cs = c->coarse;
  const int64_t n6 = c->N * 6;
  const int G = (int)c->tile.n_tiles;
  if (!c->ps_Ug.p) {
    PL_HIP(c->ps_Ug.alloc((size_t)n6));
    PL_HIP(c->ps_red.alloc((size_t)G * pl::kPersistRed));
    PL_HIP(c->ps_flags.alloc((size_t)2 * G + 4));
    PL_HIP(c->ps_dbg.alloc(8));
    // aggregate -> its tiles
    std::vector<int32_t> aot((size_t)G);
    PL_HIP(hipMemcpy(aot.data(), cs.agg_of_tile.p, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost));
    int n_agg = 0;
    for (int32_t v : aot) n_agg = std::max(n_agg, v + 1);
    std::vector<int32_t> ptr((size_t)n_agg + 1, 0), idx((size_t)G);
    for (int32_t v : aot) ptr[(size_t)v + 1]++;
    for (int g = 0; g < n_agg; ++g) ptr[(size_t)g + 1] += ptr[(size_t)g];
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int t = 0; t < G; ++t) idx[(size_t)fill[(size_t)aot[(size_t)t]]++] = t;
    PL_HIP(c->ps_agg_ptr.alloc(ptr.size()));
    PL_HIP(c->ps_agg_idx.alloc(idx.size()));
    PL_HIP(hipMemcpy(c->ps_agg_ptr.p, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    PL_HIP(hipMemcpy(c->ps_agg_idx.p, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    c->ps_n_agg = n_agg;
  }
  if ((int64_t)c->ps_n_agg * cs.cm > cs.ncp) return fail(PL_ERR_STATE, "persistent PCG: aggregate table does not match the dense level");
  PL_HIP(hipMemsetAsync(c->ps_flags.p, 0, ((size_t)2 * G + 4) * sizeof(unsigned), c->stream));
  const bool stream_form = !c->pal_lds;
  pl::PersistArgs a;
  a.tdesc = c->tile.tdesc.p;
  a.vword = stream_form ? c->vword_dir.p : c->vword.p;
  a.vother = c->tile.vother.p;
  a.tab = static_cast<const double2 *>(stream_form ? (const void *)c->tile.dir_table.p : (const void *)c->pal_dense.p);
  a.n_tab = stream_form ? c->tile.n_dir : c->pal_entries;
  a.rec5 = stream_form ? reinterpret_cast<const pl::Rec5 *>(c->rec5.p) : (const pl::Rec5 *)nullptr;
  a.foreign_idx = c->tile.foreign_idx.p;
  a.fixedbits = c->fixedbits.p;
  a.stride = c->tile.max_nodes | 1;
  a.agg_of_tile = cs.agg_of_tile.p;
  a.cen = cs.cen.p;
  a.xyz = c->xyz.p;
  a.dinv32 = cs.dinv32;
  a.Bt_inv = cs.tile_level ? (const double *)cs.Bt_inv : (const double *)nullptr;
  a.Ainv = cs.Ainv;
  a.agg_tile_ptr = c->ps_agg_ptr.p;
  a.agg_tile_idx = c->ps_agg_idx.p;
  a.ncp = cs.ncp;
  a.cm = cs.cm;
  a.n_agg = c->ps_n_agg;
  a.x = c->x.p;
  a.r = c->r.p;
  a.Ug = c->ps_Ug.p;
  a.red = c->ps_red.p;
  a.flagU = c->ps_flags.p;
  a.flagR = c->ps_flags.p + G;
  a.err = c->ps_flags.p + 2 * G;
  a.hist = c->hist.p;
  a.max_iter = max_iter;
  a.thresh = thresh;
  a.iters_out = reinterpret_cast<int *>(c->ps_flags.p + 2 * G + 1);
  a.dbg = c->ps_dbg.p;
  const size_t lds = ((size_t)12 * a.stride + (size_t)2 * a.n_tab * (stream_form ? 2 : pl::kPalLdsChunks) + (size_t)2 * cs.ncp +
                      (size_t)G * pl::kPersistRed) * sizeof(double) + ((size_t)c->ps_n_agg + 1 + G + 2) * sizeof(int32_t);
  if (lds > 150 * 1024) return fail(PL_ERR_STATE, "persistent PCG: the tile state does not fit the LDS");
  hipError_t attr = hipSuccess;
  const auto launch = [&](auto rec, auto tm, auto nc) {
    const auto kern = &pl::k_persist_cg1<decltype(rec)::value, decltype(tm)::value, decltype(nc)::value>;
    attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr == hipSuccess) hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(pl::kPersistBlock), lds, c->stream, a);
  };
  with_tile_modes(c, [&](auto tm) {
    const auto columns = [&](auto rec) {      // columns of A_c^-1 per thread
      if (cs.ncp <= 2 * pl::kPersistBlock) launch(rec, tm, Int<2>{});
      else if (cs.ncp <= 3 * pl::kPersistBlock) launch(rec, tm, Int<3>{});
      else launch(rec, tm, Int<4>{});
    };
    if (stream_form) columns(Int<pl::kRecCompact>{});
    else columns(Int<pl::kRecPalette>{});
  });
  PL_HIP(attr);
  PL_HIP(hipGetLastError());
  unsigned tail[3] = {0, 0, 0};
  PL_HIP(hipMemcpyAsync(tail, c->ps_flags.p + 2 * G, sizeof(tail), hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  if (tail[0] != 0) return fail(PL_ERR_HIP, "persistent PCG: a hand-off between workgroups timed out");
  if (const char *e = std::getenv("PL_PERSIST_DEBUG"); e && e[0] == '1') {
    unsigned long long ph[8];
    PL_HIP(hipMemcpy(ph, c->ps_dbg.p, sizeof(ph), hipMemcpyDeviceToHost));
    const double it = std::max(1u, tail[1]);
    std::fprintf(stderr, "[persist] %u iterations; us per iteration in workgroup 0: u + publish %.2f | wait u %.2f | K u %.2f | sums + publish "
                 "%.2f | wait + gather %.2f | scalars + recurrences %.2f\n", tail[1], ph[0] * 0.01 / it, ph[1] * 0.01 / it,
                 ph[2] * 0.01 / it, ph[3] * 0.01 / it, ph[4] * 0.01 / it, ph[5] * 0.01 / it);
  }
  const int its = (int)tail[1];
  st->iterations = its;
  st->converged = (int)tail[2];
  st->info = st->converged ? 0.0 : 1.0;
  st->short_iteration_used = 2.0;
  if (its >= 0 && its < c->hist_cap) {
    double rr = 0.0;
    PL_HIP(hipMemcpy(&rr, c->hist.p + std::min(its, max_iter - 1), sizeof(double), hipMemcpyDeviceToHost));
    if (std::isnan(rr) || std::isinf(rr)) return fail(PL_ERR_NAN, "NaN/Inf in the PCG residual");
    st->rel_residual = std::sqrt(rr / bb);
  }
  return PL_OK;
}

// r0 = P (f - K ubar), x = 0, z0 = p0 = D^-1 r0 (G^-1 r0 on DDM handles), ||b||^2 and r0.z0 into scalar set 0
int pcg_init(pl_context *c, const double *f_dev, const double *Kubar_dev, bool sum_rz) {
  const int64_t n6 = c->N * 6;
  PL_HIP(hipMemsetAsync(c->scal.p, 0, 2 * pl::S_COUNT * pl::kSlots * sizeof(double), c->stream));
  if (c->dist.active)
    pl::launch_pcg_init_weighted(n6, f_dev, Kubar_dev, c->fixed.p, c->dinv.p, c->dist.weight.p, c->x.p, c->r.p,
                                 c->z.p, c->p.p, c->scal.p, c->stream);
  else
    hipLaunchKernelGGL(pl::k_pcg_init, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, c->stream, n6, f_dev, Kubar_dev,
                       c->fixed.p, c->dinv.p, c->x.p, c->r.p, c->z.p, c->p.p, c->scal.p);
  PL_HIP(hipGetLastError());
  if (c->dist.active) {
    if ((sum_rz && pl::dist_sum_scalars(c->dist, c->scal.p + pl::S_RZ_OLD * pl::kSlots, pl::kSlots, c->stream)) ||
        pl::dist_sum_scalars(c->dist, c->scal.p + pl::S_BB * pl::kSlots, pl::kSlots, c->stream))
      return fail(PL_ERR_HIP, "RCCL all-reduce of the initial PCG scalars failed");
  }
  return PL_OK;
}

// Node elimination, before the loop: start from the iterate whose eliminated nodes are in equilibrium.  t_c = K_cc^-1 b_c
// (rows of the zeroed t, zero elsewhere), r_v -= (K t)_v: the load the eliminated nodes pass on.  Their own rows of r keep
// b_c (every later step keeps them in equilibrium), their rows of x stay 0 until the back-substitution after the loop.
template <typename T>
int condense_prologue(pl_context *c, T *r, T *t, T *Kt) {
  hipLaunchKernelGGL(pl::k_condense_solve<T>, dim3(grid_for(c->n_cond * 6)), dim3(pl::kBlock), 0, c->stream, c->n_cond,
                     c->cnodes.p, cinv(c), ccls(c), (const T *)r, t, 1.0);
  const int rc = spmv_as_stored<T>(c, t, Kt, true, nullptr, c->maskC.p, pl::kEndsOthers);
  if (rc) return rc;
  hipLaunchKernelGGL(pl::k_condense_subtract<T>, dim3(grid_for(c->N * 6)), dim3(pl::kBlock), 0, c->stream, c->N, c->cflag.p,
                     (const T *)Kt, r);
  PL_HIP(hipGetLastError());
  return PL_OK;
}
// ... and after it: x_c = K_cc^-1 (b_c - (K [x_v ; 0])_c)
template <typename T>
int condense_backsubst(pl_context *c, T *x, const T *r, T *Kx) {
  const int rc = spmv_as_stored<T>(c, x, Kx, false, nullptr, nullptr, pl::kEndsCondensed);
  if (rc) return rc;
  hipLaunchKernelGGL(pl::k_condense_backsubst<T>, dim3(grid_for(c->n_cond * 6)), dim3(pl::kBlock), 0, c->stream, c->n_cond,
                     c->cnodes.p, cinv(c), ccls(c), r, (const T *)Kx, x);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// z0 = M^-1 r0 and r0.z0 of the multi-level forms, through the tail of an iteration "-1" (alpha = 0); its history entry
// goes to slot max_iter.  (The persistent launch builds u0 = M^-1 r0 itself.)
int pcg_first_direction(pl_context *c, int max_iter) {
  const int64_t n6 = c->N * 6;
  if (c->persist_use || !(c->small_use || c->coarse.ready)) return PL_OK;
  if (c->small_use) {   // set -1 of the ring is zero; iteration 0 then forms p0 = z0 + 0 p_old in its K*p launch
    const int rc = small_prepare(c);
    if (rc) return rc;
    PL_HIP(hipMemsetAsync(c->Ap.p, 0, n6 * sizeof(double), c->stream));
    return small_tail(c, -1, max_iter);
  }
  // p = 0 (p.Ap = 0) on scalar set 1: the direction kernel leaves p = z0 and rz_old = r0.z0 in set 0, where iteration 0 starts
  PL_HIP(hipMemsetAsync(c->p.p, 0, n6 * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->Ap.p, 0, n6 * sizeof(double), c->stream));
  return pcg_tail_coarse(c, c->scal.p + pl::S_COUNT * pl::kSlots, c->scal.p, max_iter);
}

// The iterations of pcg_solve: chunks of the look schedule (pl_schedule.h), the residual history read after each.
// *done: iterations the device has run.
int pcg_loop(pl_context *c, double thresh, double bb, int max_iter, pl_stats_t *st, int *done) {
  const bool ref = ref_cg(c) && !c->dist.active && !c->coarse.ready;
  const int hcap = c->hist_cap;
  // DDM handles: the device applies the stopping rules itself and freezes the iterate (k_pcg_direction), so the host may
  // queue as many iterations as it likes between two looks at the history and still hands back the reference's iterate
  c->stop_use = c->opkind == 1 && !c->dist.active && !c->coarse.ready && !c->small_use;
  if (c->stop_use) {
    if (!c->stop_flag.p) PL_HIP(c->stop_flag.alloc(1));
    PL_HIP(hipMemsetAsync(c->stop_flag.p, 0, sizeof(int), c->stream));
    c->stop_thresh = thresh;
  }
  pl::LookParams lp{c->opt.check_every, max_iter, thresh, bb};
  lp.dd_ready = c->dd_ready;
  lp.ref_cg = ref;
  lp.last_iterations = c->last_iterations;
  pl::LookSchedule look(lp);
  const int hbuf = look.max_chunk();
  std::vector<double> h_hist(hbuf), h_pp(ref ? hbuf : 0), h_xx(ref ? hbuf : 0), h_al(ref ? hbuf : 0);
  st->info = 1.0;
  int k = 0;
  while (k < max_iter) {
    const int todo = look.todo(k);
    for (int j = 0; j < todo; ++j) {
      const int rc = pcg_iteration(c, k + j);
      if (rc) return rc;
    }
    PL_HIP(hipMemcpyAsync(h_hist.data(), c->hist.p + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ref) {
      PL_HIP(hipMemcpyAsync(h_pp.data(), c->hist.p + hcap + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      PL_HIP(hipMemcpyAsync(h_xx.data(), c->hist.p + 2 * (size_t)hcap + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      PL_HIP(hipMemcpyAsync(h_al.data(), c->hist.p + 3 * (size_t)hcap + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    PL_HIP(hipStreamSynchronize(c->stream));
    for (int j = 0; j < todo; ++j) {
      const double rr = h_hist[j];
      if (std::isnan(rr) || std::isinf(rr)) return fail(PL_ERR_NAN, "NaN/Inf in the PCG residual");
      if (!st->converged) st->rel_residual = std::sqrt(rr / bb);
      if (rr <= thresh && !st->converged) converged_at(st, k + j + 1, 0.0);
      if (ref && !st->converged) {
        // conjugate_gradient_solver.py:102-109, in its order: the direction-norm stop, then the "tiny step" flag
        if (c->opt.mintol > 0.0 && std::sqrt(h_pp[j]) < c->opt.mintol * (std::sqrt(h_xx[j]) + 1e-12)) converged_at(st, k + j + 1, 1.0);
        else if (h_al[j] < 1e-6) st->info = 2.0;
      }
      if (st->converged && c->stop_use) break;     // (the device stopped there too: later slots of the history are not written)
    }
    k += todo;
    if (st->converged) break;
    look.missed(k, h_hist[todo - 1]);
  }
  if (!st->converged) st->iterations = k;
  *done = k;
  return PL_OK;
}

// Solve P K P x = rhs (device rhs already masked), x0 = 0.  Result in c->x.  Returns iterations through stats.
int pcg_solve(pl_context *c, const double *f_dev, const double *Kubar_dev, double rtol, int max_iter,
              pl_stats_t *st) {
  const int64_t n6 = c->N * 6;
  int rc = ensure_hist(c, max_iter + 1);
  if (rc) return rc;
  rc = pcg_init(c, f_dev, Kubar_dev, true);
  if (rc) return rc;
  if (c->n_per_groups > 0) {   // periodic constraints: b is Q b (the caller's part), z0 = Q D^-1 r0, p0 = z0
    periodic_average(c, c->z.p);
    PL_HIP(hipMemcpyAsync(c->p.p, c->z.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  if (c->dd_ready || c->dd_blocks) {   // z0 = p0 = G^-1 r0, rz_old = r0.z0 (k_pcg_init ran with dinv = 0)
    ddm_precondition(c, c->scal.p + pl::S_RZ_OLD * pl::kSlots);
    PL_HIP(hipMemcpyAsync(c->p.p, c->z.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  if (c->cond_use) {   // (decided by solver_plan: never with a K*p kernel that ignores the elimination masks)
    PL_HIP(hipMemsetAsync(c->z.p, 0, n6 * sizeof(double), c->stream));
    rc = condense_prologue<double>(c, c->r.p, c->z.p, c->tmp2.p);
    if (rc) return rc;
  }
  const bool warm = c->opt.warm_start >= 1 && c->coarse.ready && !c->dist.active;
  if (warm && c->xprev.p && c->xprev_valid) {
    rc = warm_start_apply(c);
    if (rc) return rc;
  }
  rc = pcg_first_direction(c, max_iter);
  if (rc) return rc;
  double bb = 0.0;
  bool zero = false;
  rc = solve_begin(c, c->scal.p + pl::S_BB * pl::kSlots, st, &bb, &zero);
  if (zero) {   // zero right-hand side -> zero solution (a warm start above may have put the previous one into x)
    PL_HIP(hipMemsetAsync(c->x.p, 0, n6 * sizeof(double), c->stream));
    PL_HIP(hipStreamSynchronize(c->stream));
  }
  if (rc || zero) return rc;
  const double thresh = rtol * rtol * bb;
  if (c->persist_use) {
    rc = persist_solve(c, thresh, bb, max_iter, st);
    if (rc) return rc;
    c->last_iterations = st->converged ? st->iterations : 0;
    // (as found: only warm_start = 1 keeps the solution here, although 2 to 4 reach this branch as well)
    return c->opt.warm_start == 1 && st->converged ? warm_retain(c, false) : PL_OK;
  }
  int k = 0;
  rc = pcg_loop(c, thresh, bb, max_iter, st, &k);
  if (rc) return rc;
  c->last_iterations = st->converged ? st->iterations : 0;
  if (c->small_use) {
    rc = small_finish(c, k);
    if (rc) return rc;
    st->short_iteration_used = 1.0;
  }
  if (c->cond_use) {
    rc = condense_backsubst<double>(c, c->x.p, (const double *)c->r.p, c->tmp2.p);
    if (rc) return rc;
  }
  return warm && st->converged ? warm_retain(c, true) : PL_OK;
}

// ----------------------------------------------------------------------------------------------------------
// Single-reduction PCG (opts.cg_form = 1; pl_cg1.h): u -> z, w -> Ap, s -> tmp2.
// ----------------------------------------------------------------------------------------------------------
// Which solver the next pl_solve runs, decided in ONE place (pl_solve and pl_time_kernel both ask): the fp32 modes and
// the node elimination need the multi-level preconditioner on the LDS-tile kernel; the elimination is off in the
// single-reduction form and in precision = 2.  Sets c->cond_use.
inline bool mp_applies(const pl_context *c) {
  return c->opt.precision != 0 && c->opkind == 0 && c->coarse.ready && choose_kernel(c) == 3 && c->tile.ready;
}
inline void solver_plan(pl_context *c) {
  const bool mp = mp_applies(c);
  c->cond_use = c->cond_ready && c->coarse.ready && c->opkind == 0 && choose_kernel(c) == 3 && c->tile.ready &&
                (!mp || c->opt.precision == 1) && c->opt.cg_form != 1;
  // short form of the iteration (pl_small.h): the fp64 ordinary form on the LDS-resident K*p, explicit A_c^-1 at hand
  const int form = kp_form_of(c);
  c->small_use = !mp && small_wanted(c) && c->coarse.ready && !c->coarseL.ready && c->coarse.ainv_ready &&
                 (form == 1 || form == 2) && c->tile.vis_ready;
  // ... or, opt-in, the whole loop as one persistent launch (pl_persist.h): single-reduction CG without node elimination,
  // one workgroup per tile, all co-resident
  c->persist_use = c->small_use && c->opt.short_iteration == 2 && c->tile.n_tiles <= 256 &&
                   c->coarse.ncp <= pl::kPersistBlock * pl::kPersistMaxCols && c->tile.max_nodes <= pl::kPersistBlock;
  if (c->persist_use) {
    c->cond_use = false;
    c->small_use = false;
  }
}
inline bool cg1_applies(const pl_context *c) {
  return c->opt.cg_form == 1 && c->coarse.ready && !c->coarseL.ready && !c->cond_use && c->opt.precision == 0 &&
         c->opkind == 0 && c->tile.ready && choose_kernel(c) == 3;
}

int pcg_solve_cg1(pl_context *c, const double *f_dev, const double *Kubar_dev, double rtol, int max_iter,
                  pl_stats_t *st) {
  const int64_t n6 = c->N * 6;
  pl::Coarse &cs = c->coarse;
  const int ncp = cs.ncp, bs = pl::cg1_block_size(ncp);
  int rc = ensure_hist(c, max_iter + 2);
  if (rc) return rc;
  const size_t need = 2 * (size_t)bs + 2 * pl::kSlots + 4 + (size_t)ncp;
  if (!c->cg1.p || c->cg1.n < need) PL_HIP(c->cg1.alloc(need));
  double *blk[2] = {c->cg1.p, c->cg1.p + bs};
  double *gc[2] = {c->cg1.p + 2 * bs, c->cg1.p + 2 * bs + pl::kSlots};
  double *stt[2] = {c->cg1.p + 2 * bs + 2 * pl::kSlots, c->cg1.p + 2 * bs + 2 * pl::kSlots + 2};
  double *sc = c->cg1.p + 2 * bs + 2 * pl::kSlots + 4;
  double *u = c->z.p, *w = c->Ap.p, *s = c->tmp2.p;
  const double *wt = c->dist.active ? (const double *)c->dist.weight.p : (const double *)nullptr;
  const uint8_t *shared = c->dist.active ? (const uint8_t *)c->sharedbits.p : (const uint8_t *)nullptr;
  const double *Bt = cs.tile_level ? (const double *)cs.Bt_inv : (const double *)nullptr;
  const double *yt = cs.tile_level ? (const double *)cs.yt : (const double *)nullptr;
  const dim3 gt((unsigned)cs.n_tiles), blkdim(cs.vblock);
  const bool cm12 = cs.cm == 12;     // (a 12-mode dense level needs the 12-mode tile level)
  const auto restrict_to = [&](const double *v, double *out) {
    const auto kern = cm12 ? pl::k_cg1_restrict<12> : pl::k_cg1_restrict<6>;
    hipLaunchKernelGGL(kern, gt, blkdim, 0, c->stream, c->tile.tile_start.p, cs.agg_of_tile.p, cs.cen.p, c->xyz.p, v, wt, out);
  };
  // x += alpha p, r -= alpha s with the recurrences of iteration `it` (INIT: the pass before iteration 0)
  const auto update = [&](auto init, int cur, int nxt, int it) {
    with_tile_modes(c, [&](auto tm) {
      hipLaunchKernelGGL((pl::k_cg1_update<decltype(init)::value, decltype(tm)::value>), gt, blkdim, 0, c->stream,
                         c->tile.tile_start.p, cs.agg_of_tile.p, cs.cen.p, c->xyz.p, (const double *)u, (const double *)w,
                         cs.dinv32, wt, c->p.p, s, c->x.p, c->r.p, (const double *)blk[cur], (const double *)gc[cur],
                         (const double *)stt[cur], stt[nxt], blk[nxt], Bt, cs.yt, shared, cs.rc, sc, ncp, c->hist.p, it);
    });
  };

  rc = pcg_init(c, f_dev, Kubar_dev, false);      // (the z / p the init kernel also writes are overwritten below)
  if (rc) return rc;
  PL_HIP(hipMemsetAsync(c->cg1.p, 0, need * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->p.p, 0, n6 * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(s, 0, n6 * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(cs.rc, 0, (size_t)ncp * sizeof(double), c->stream));

  // u = M^-1 r, w = K u and the reduction block of iteration k (k = -1: the pass that prepares iteration 0)
  auto second_half = [&](int k) -> int {
    const int cur = k & 1, nxt = (k + 1) & 1;
    pl::coarse_apply(cs, cs.rc, cs.tv, cs.yc, gc[nxt], (const double *)nullptr, c->stream);
    with_tile_modes(c, [&](auto tm) {
      hipLaunchKernelGGL(pl::k_cg1_precond<decltype(tm)::value>, gt, blkdim, 0, c->stream, c->tile.tile_start.p,
                         (const double *)c->r.p, cs.dinv32, c->xyz.p, cs.agg_of_tile.p, cs.cen.p, cs.yc, yt, c->fixedbits.p,
                         shared, u, k >= 0 ? blk[cur] : (double *)nullptr, bs, k >= 0 ? gc[cur] : (double *)nullptr, cs.cm);
    });
    int r2 = launch_spmv(c, u, w, true, blk[nxt] + ncp, nullptr, pl::kEndsAll, false);
    if (r2) return r2;
    restrict_to((const double *)w, blk[nxt]);
    if (c->dist.active && pl::dist_sum_scalars(c->dist, blk[nxt], bs, c->stream))
      return fail(PL_ERR_HIP, "RCCL all-reduce of the single-reduction PCG failed");
    PL_HIP(hipGetLastError());
    return PL_OK;
  };
  // Z^T r0 (summed over ranks once), tile level and partial sums of r0 into block 0, then u0, w0
  restrict_to((const double *)c->r.p, cs.rc);
  if (c->dist.active && pl::dist_sum_scalars(c->dist, cs.rc, ncp, c->stream))
    return fail(PL_ERR_HIP, "RCCL all-reduce of the initial coarse residual failed");
  update(std::true_type{}, 1, 0, -1);
  rc = second_half(-1);
  if (rc) return rc;

  double bb = 0.0;
  bool zero = false;
  st->info = 1.0;
  rc = solve_begin(c, c->scal.p + pl::S_BB * pl::kSlots, st, &bb, &zero);
  if (rc || zero) return rc;
  const double thresh = rtol * rtol * bb;
  pl::LookParams lp{c->opt.check_every, max_iter, thresh, bb};
  lp.extra = 1;      // (the history lags one update behind)
  pl::LookSchedule look(lp);
  std::vector<double> h_hist(look.max_chunk());
  int k = 0;
  // hist[k] = ||r_k||^2, the residual BEFORE update k (it is reduced together with that iteration's other sums).  Exactly
  // max_iter updates are applied: the residual after the last one is read from the block the next update would have used
  // (until this was counted right the loop ran max_iter + 1 updates to learn it, and a solve that hit max_iter handed back
  // x_(max_iter + 1) under iterations = max_iter: tests/test_gpu_precond.py)
  while (k < max_iter) {
    const int todo = look.todo(k);
    for (int j = 0; j < todo; ++j) {
      const int it = k + j;
      update(std::false_type{}, it & 1, (it + 1) & 1, it);
      rc = second_half(it);
      if (rc) return rc;
    }
    PL_HIP(hipMemcpyAsync(h_hist.data(), c->hist.p + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PL_HIP(hipStreamSynchronize(c->stream));
    for (int j = 0; j < todo; ++j) {
      const double rr = h_hist[j];
      if (std::isnan(rr) || std::isinf(rr)) return fail(PL_ERR_NAN, "NaN/Inf in the PCG residual");
      if (!st->converged) st->rel_residual = std::sqrt(rr / bb);
      // (iterations: updates applied when this residual was reached - x has had a few more since)
      if (rr <= thresh && !st->converged) converged_at(st, k + j, 0.0);
    }
    k += todo;
    if (st->converged) break;
    look.missed(k, h_hist[todo - 1]);
  }
  if (!st->converged) {
    double h_rr[pl::kSlots], rr = 0.0;       // ||r_k||^2 after update k - 1: slot 2 of the reduced block of iteration k
    PL_HIP(hipMemcpyAsync(h_rr, blk[k & 1] + ncp + 2 * pl::kSlots, sizeof(h_rr), hipMemcpyDeviceToHost, c->stream));
    PL_HIP(hipStreamSynchronize(c->stream));
    for (int q = 0; q < pl::kSlots; ++q) rr += h_rr[q];
    if (std::isnan(rr) || std::isinf(rr)) return fail(PL_ERR_NAN, "NaN/Inf in the PCG residual");
    st->rel_residual = std::sqrt(rr / bb);
    st->iterations = k;
    if (rr <= thresh) converged_at(st, k, 0.0);
  }
  return PL_OK;
}

// ----------------------------------------------------------------------------------------------------------
// fp32 solver modes (opts.precision; multi-level PCG on the tile kernel only):
//   1  inner PCG on fp32-stored x, r, p, Ap; the fp64 solution accumulates the inner corrections and every restart
//      begins from the TRUE fp64 residual P(f - K(ubar + x)) (classical iterative refinement);
//   2  only the search direction p and K*p are stored in fp32, x and the residual recurrence stay fp64: no restart
//      is needed to reach fp64 accuracy, the true residual is verified once the recurrence says "converged" (the
//      fp32 rounding of K*p lets the two drift apart by ~6e-8 of the accumulated steps).
// In both modes every product and sum is evaluated in fp64 (pl_tile.h, pl_coarse.h): fp32 only halves the bytes.
// ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(pl::kBlock) void k_mp_true_residual(int64_t n6, const double *__restrict__ f,
                                                                const double *__restrict__ Kubar,
                                                                const double *__restrict__ Kx /* may be null */,
                                                                const uint8_t *__restrict__ fixed,
                                                                const double *__restrict__ w /* may be null */,
                                                                double *__restrict__ r, double *__restrict__ rr_slots) {
  __shared__ double red[pl::kBlock / pl::kWave];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * pl::kBlock + threadIdx.x; i < n6; i += (int64_t)gridDim.x * pl::kBlock) {
    const double v = fixed[i] ? 0.0 : f[i] - Kubar[i] - (Kx ? Kx[i] : 0.0);
    r[i] = v;
    acc += (w ? w[i] : 1.0) * v * v;
  }
  const double t = pl::block_sum(acc, red);
  if (threadIdx.x == 0) unsafeAtomicAdd(rr_slots + (blockIdx.x & (pl::kSlots - 1)), t);
}
// start of an fp32 inner solve: r32 = r, x32 = 0
__global__ __launch_bounds__(pl::kBlock) void k_mp_restart(int64_t n6, const double *__restrict__ r,
                                                          float *__restrict__ r32, float *__restrict__ x32) {
  for (int64_t i = (int64_t)blockIdx.x * pl::kBlock + threadIdx.x; i < n6; i += (int64_t)gridDim.x * pl::kBlock) {
    r32[i] = (float)r[i];
    x32[i] = 0.f;
  }
}
__global__ __launch_bounds__(pl::kBlock) void k_mp_accumulate(int64_t n6, const float *__restrict__ x32,
                                                             double *__restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * pl::kBlock + threadIdx.x; i < n6; i += (int64_t)gridDim.x * pl::kBlock)
    x[i] += (double)x32[i];
}

// One iteration of the inner PCG of the fp32 modes: the operator as the solve applies it, then the multi-level tail.  j:
// iteration of this inner solve (parity of the scalar sets).  (precision = 2 never eliminates nodes: solver_plan leaves
// cond_use false there.)
template <typename RT>
int mp_iteration(pl_context *c, int j, int hist_slot, float *p32, float *Ap32, RT *x, RT *r) {
  const int set = pl::S_COUNT * pl::kSlots;
  double *cur = c->scal.p + (j & 1) * set, *nxt = c->scal.p + ((j + 1) & 1) * set;
  const int rc = apply_operator<float>(c, p32, Ap32, cur + pl::S_PAP * pl::kSlots);
  return rc ? rc : pcg_tail_coarse_t<float, RT>(c, cur, nxt, hist_slot, p32, (const float *)Ap32, x, r);
}

template <typename RT>
int pcg_solve_mp_t(pl_context *c, const double *f_dev, const double *Kubar_dev, double rtol, int max_iter,
                   pl_stats_t *st) {
  constexpr bool kAll32 = sizeof(RT) == 4;
  const int64_t n6 = c->N * 6;
  const int set = pl::S_COUNT * pl::kSlots;
  int rc = ensure_hist(c, max_iter + 2);
  if (rc) return rc;
  float *p32 = reinterpret_cast<float *>(c->p.p), *Ap32 = reinterpret_cast<float *>(c->Ap.p);
  // mode 1: the inner iterate / residual live in the (otherwise unused) z buffer
  RT *xi = kAll32 ? reinterpret_cast<RT *>(c->z.p) : reinterpret_cast<RT *>(c->x.p);
  RT *ri = kAll32 ? reinterpret_cast<RT *>(c->z.p) + n6 : reinterpret_cast<RT *>(c->r.p);
  const double *w = c->dist.active ? (const double *)c->dist.weight.p : (const double *)nullptr;
  double *aux = c->scal.p + pl::S_AUX * pl::kSlots;   // slots outside the two per-parity sets' live entries
  PL_HIP(hipMemsetAsync(c->scal.p, 0, 2 * set * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(c->x.p, 0, n6 * sizeof(double), c->stream));
  hipLaunchKernelGGL(k_mp_true_residual, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, c->stream, n6, f_dev, Kubar_dev,
                     (const double *)nullptr, c->fixed.p, w, c->r.p, aux);
  PL_HIP(hipGetLastError());
  if (c->dist.active && pl::dist_sum_scalars(c->dist, aux, pl::kSlots, c->stream))
    return fail(PL_ERR_HIP, "RCCL all-reduce of ||b||^2 failed");
  double bb = 0.0;
  bool zero = false;
  rc = solve_begin(c, aux, st, &bb, &zero);
  if (rc || zero) return rc;
  const double thresh = rtol * rtol * bb;
  // an fp32 residual recurrence is trustworthy over ~4 decades: restart from the true residual after that
  static const double drop_env = [] { const char *e = std::getenv("PL_MP_DROP"); return e ? std::atof(e) : 0.0; }();
  const double inner_drop = kAll32 ? (drop_env > 0.0 ? drop_env : 1e-8) : 0.0;      // on ||r||^2
  // (measured, tools/experiments/mp_drop_sweep.sh, iterations at 50^3 Octet / 100^3 Octet / configs[2] / configs[4]:
  //  fixed 8 decades per stage 141 / 151 / 392 / 324;  equal stages of at most 5: 136 / 146 / 352 / 293,  6: 130 / 144 / 358 / 298,
  //  7: 130 / 144 / 357 / 298,  8: 130 / 147 / 393 / 354;  fp64: 120 / 137 / 335 / -)
  static const double stage_max = [] { const char *e = std::getenv("PL_MP_STAGE"); return e ? std::atof(e) : 6.0; }();
  double rr_true = bb;
  // r = P (f - K (ubar + x)) in fp64, rr_true = its squared norm (summed over the ranks; a warm start has one rank)
  const auto true_residual = [&](const char *nan_message) -> int {
    const int r2 = launch_spmv(c, c->x.p, c->tmp2.p, true, nullptr);
    if (r2) return r2;
    PL_HIP(hipMemsetAsync(aux, 0, pl::kSlots * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_mp_true_residual, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, c->stream, n6, f_dev, Kubar_dev,
                       (const double *)c->tmp2.p, c->fixed.p, w, c->r.p, aux);
    PL_HIP(hipGetLastError());
    if (c->dist.active && pl::dist_sum_scalars(c->dist, aux, pl::kSlots, c->stream))
      return fail(PL_ERR_HIP, "RCCL all-reduce of the true residual failed");
    const int r3 = read_slots(c, aux, &rr_true);
    if (r3) return r3;
    if (std::isnan(rr_true) || std::isinf(rr_true)) return fail(PL_ERR_NAN, nan_message);
    st->rel_residual = std::sqrt(rr_true / bb);
    return PL_OK;
  };
  // warm start (mode 1, as pcg_solve): the refinement begins at the previous solution of this handle, masked with the
  // CURRENT Dirichlet set - the first inner solve then works on its true residual like every later one
  const bool warm = kAll32 && c->opt.warm_start >= 1 && !c->dist.active;     // (2 / 3: the previous solution here, no extrapolation)
  if (warm && c->xprev.p && c->xprev_valid) {
    PL_HIP(hipMemcpyAsync(c->x.p, c->xprev.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_warm_mask, dim3(grid_for(n6)), dim3(pl::kBlock), 0, c->stream, c->N, (const uint8_t *)nullptr,
                       (const uint8_t *)c->fixed.p, c->x.p);
    rc = true_residual("NaN/Inf in the warm-start residual");
    if (rc) return rc;
    if (rr_true <= thresh) {       // (the previous solution already solves this system)
      st->converged = 1;
      return PL_OK;
    }
  }
  int k = 0;                      // iterations over all inner solves
  std::vector<double> h_hist;
  for (int outer = 0; outer < 40 && k < max_iter; ++outer) {
    // ---- (re)start: p = M^-1 r through the tail of an iteration "-1" (alpha = 0) on scalar set 1
    PL_HIP(hipMemsetAsync(c->scal.p, 0, 2 * set * sizeof(double), c->stream));
    if (kAll32)
      hipLaunchKernelGGL(k_mp_restart, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, c->stream, n6, c->r.p,
                         reinterpret_cast<float *>(ri), reinterpret_cast<float *>(xi));
    PL_HIP(hipMemsetAsync(p32, 0, n6 * sizeof(float), c->stream));
    if (c->cond_use) {   // node elimination inside the inner solve (as in pcg_solve; precision = 1 only: solver_plan)
      rc = condense_prologue<float>(c, reinterpret_cast<float *>(ri), p32, Ap32);
      if (rc) return rc;
      PL_HIP(hipMemsetAsync(p32, 0, n6 * sizeof(float), c->stream));
    }
    PL_HIP(hipMemsetAsync(Ap32, 0, n6 * sizeof(float), c->stream));
    rc = pcg_tail_coarse_t<float, RT>(c, c->scal.p + set, c->scal.p, max_iter + 1, p32, (const float *)Ap32, xi, ri);
    if (rc) return rc;
    // Stages of EQUAL depth: what is left to the threshold (on ||r||^2) is cut into the fewest stages of at most
    // `stage_max` decades - an fp32 residual recurrence that has dropped further has drifted from the true residual, and the
    // iterations of a stage that ends below the threshold by accident are wasted (PL_MP_DROP: a fixed drop per stage instead)
    double stop = std::max(thresh, inner_drop * rr_true);
    if (kAll32 && !(drop_env > 0.0) && rr_true > thresh) {
      const double left = std::log10(rr_true / thresh);
      const int stages = std::max(1, (int)std::ceil(left / stage_max));
      stop = stages == 1 ? thresh : std::max(thresh, rr_true * std::pow(10.0, -left / stages));
    }
    pl::LookSchedule look(pl::LookParams{0, max_iter, stop, rr_true, k});     // (always adaptive, whatever opts.check_every says)
    h_hist.resize(look.max_chunk());
    const int k0 = k;
    bool inner_done = false;
    while (!inner_done && k < max_iter) {
      const int todo = look.todo(k);
      for (int q = 0; q < todo; ++q) {
        rc = mp_iteration<RT>(c, k - k0 + q, k + q, p32, Ap32, xi, ri);
        if (rc) return rc;
      }
      PL_HIP(hipMemcpyAsync(h_hist.data(), c->hist.p + k, todo * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      PL_HIP(hipStreamSynchronize(c->stream));
      for (int q = 0; q < todo && !inner_done; ++q) {
        const double rr = h_hist[q];
        if (std::isnan(rr) || std::isinf(rr)) return fail(PL_ERR_NAN, "NaN/Inf in the PCG residual");
        inner_done = rr <= stop;
      }
      // (the device has run the whole chunk: x holds the iterate after `todo` iterations, which is what is kept)
      k += todo;
      if (!inner_done) look.missed(k, h_hist[todo - 1]);
    }
    // ---- true residual of the accumulated solution
    if (c->cond_use) {   // the eliminated nodes of this inner solve
      rc = condense_backsubst<float>(c, reinterpret_cast<float *>(xi), reinterpret_cast<const float *>(ri), Ap32);
      if (rc) return rc;
    }
    if (kAll32)
      hipLaunchKernelGGL(k_mp_accumulate, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, c->stream, n6,
                         reinterpret_cast<const float *>(xi), c->x.p);
    rc = true_residual("NaN/Inf in the true residual");
    if (rc) return rc;
    st->restarts = (double)(outer + 1);     // restarts (inner solves) taken
    if (rr_true <= thresh * 1.0000001) {
      st->converged = 1;
      break;
    }
  }
  st->iterations = k;
  // (as found: every warm_start >= 1 is 1 here - no older solutions are kept)
  return warm && st->converged ? warm_retain(c, false) : PL_OK;
}

}  // namespace
