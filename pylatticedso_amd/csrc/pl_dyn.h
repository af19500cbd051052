// Transient response by implicit Newmark time stepping (pl_dyn_spmv_multi / pl_transient).  gfx950 only.
//
// Linear structural dynamics M a + C v + K u = f(t) on the free dofs of pl_set_bc (supports held at zero), K the strut
// operator, M the consistent mass of pl_set_mass, C = ray_m M + ray_k K (Rayleigh).  Acceleration form of the Newmark family
// (beta, gamma), step n -> n + 1 with dt:
//     ut = u_n + dt v_n + dt^2 (1/2 - beta) a_n,   vt = v_n + dt (1 - gamma) a_n                                (predict)
//     (M (1 + gamma dt ray_m) + K (beta dt^2 + gamma dt ray_k)) a_{n+1} = f_{n+1} - K ut - C vt                  (solve)
//     u_{n+1} = ut + beta dt^2 a_{n+1},   v_{n+1} = vt + gamma dt a_{n+1}                                       (correct)
// a_0 is the same three stages with dt = 0: M a_0 = f_0 - K u_0 - C v_0.  The matrix of the solve is S = c_K K + c_M M, SPD for
// c_K >= 0, c_M > 0; the solver is the multi-column Jacobi PCG of pl_multi.h on one column with S in the place of K.
//
// S x is ONE gather (k_gather_multi with DynTerm): the node -> strut walk of the K and M products, the ELL entry
// and the neighbour's row read once, the stiffness record and the mass record read at the same strut index, both closed
// forms summed into the same registers.  The linear scalars of the stiffness record (a, c, e1, e2, e3) carry c_K and the four
// mass scalars (m / 6, c, j, g) carry c_M, so the sum costs no multiplication per dof.
//
// Per step the state [u | v | a | 0] lives in one column block of four, and K and M are applied to it once each: by
// linearity that gives K ut, K vt and M vt of the right-hand side AND the energies 1/2 v.M v, 1/2 u.K u of the state.
//
// Every product has a fixed order and no floating-point atomics; the energy sums go through the slot reductions of pl_multi.h.
#pragma once
#include "pl_mass.h"

namespace pl {

__device__ __forceinline__ Record scaled_record(const Record &r, double s) {
  return {s * r.a, s * r.c, s * r.e1, s * r.e2, s * r.e3, r.dx, r.dy, r.dz};
}

// Diagonal of the own-end 6x6 block of the mass element (mass_force with the other end at rest, one dof at a time):
//     translations 2 (m / 6) t_d^2 + (156 c + 36 g) (1 - t_d^2),   rotations 2 j t_d^2 + 4 L^2 (c + g) (1 - t_d^2)
__device__ __forceinline__ void mass_diag(const MassCoef &q, V3 d, double *dg) {
  const double L2 = dot(d, d);
  const double tt[3] = {d.x * d.x / L2, d.y * d.y / L2, d.z * d.z / L2};
  const double pu = 156.0 * q.c + 36.0 * q.g, pt = 4.0 * L2 * (q.c + q.g);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dg[k] = 2.0 * q.m6 * tt[k] + pu * (1.0 - tt[k]);
    dg[3 + k] = 2.0 * q.j * tt[k] + pt * (1.0 - tt[k]);
  }
}

// c_K K + c_M M in k_gather_multi (pl_multi.h): per entry the stiffness record is loaded, reversed, scaled and used up before
// the mass record is loaded, so only one of the two is live at a time - that is why the fused product fits in the registers of
// the mass product.  Built for column blocks of 1 and 2: at 4 it would need scratch.
struct DynTerm {
  static constexpr int kMaxKB = 2;
  const Record *__restrict__ rec;
  MassTerm mass;
  double c_K, c_M;
  template <int KB>
  __device__ __forceinline__ void entry(int64_t strut, bool point1, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                        double (&out)[6 * KB]) const {
    {
      Record r = load_record(rec, strut);
      if (point1) r = reversed(r);
      r = scaled_record(r, c_K);
      add_tip_forces<KB>(r, xo, xs, out);
    }
    {
      const MassRecord r = load_mass(mass.rec, strut);
      MassCoef c = mass_coef(r, mass.rotary);
      c = {c_M * c.m6, c_M * c.c, c_M * c.j, c_M * c.g};
      const double sg = point1 ? -1.0 : 1.0;                     // point1: d -> -d
      const V3 d = {sg * r.dx, sg * r.dy, sg * r.dz};
      add_mass_forces<KB>(c, d, xo, xs, out);
    }
  }
  template <int KB>
  __device__ __forceinline__ void node(int64_t i, const double (&xs)[6 * KB], double (&out)[6 * KB]) const {
    if (mass.node_mass) {               // kernel-uniform
      const double nm = c_M * mass.node_mass[i];
#pragma unroll
      for (int q = 0; q < 3 * KB; ++q) out[q] += nm * xs[q];
    }
  }
};

// diag(c_K K + c_M M) and its inverse on the free dofs (0 on fixed dofs and where the diagonal vanishes), as k_diag_gather
template <int LPN>
__global__ __launch_bounds__(kBlock) void k_dyn_diag_gather(int64_t N, const int64_t *__restrict__ slice_ptr,
                                                            const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                            const MassRecord *__restrict__ mrec, int rotary,
                                                            const double *__restrict__ node_mass, double c_K, double c_M,
                                                            const uint8_t *__restrict__ fixedbits,
                                                            double *__restrict__ diag, double *__restrict__ dinv) {
  constexpr int kSliceNodes = kWave / LPN;
  const int lane = threadIdx.x & 63, sub = lane / kSliceNodes;
  const int64_t slice = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const int64_t i = slice * kSliceNodes + (lane & (kSliceNodes - 1));
  if (slice * kSliceNodes >= N) return;
  double dg[6] = {0, 0, 0, 0, 0, 0};
  const int64_t p0 = slice_ptr[slice], p1 = slice_ptr[slice + 1];
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const int2 e = ent[p];
    if (e.x >= 0) {
      const int64_t b = e.y & 0x7fffffff;
      Record r = load_record(rec, b);
      if (e.y < 0) r = reversed(r);
      const MassRecord q = load_mass(mrec, b);
      double t[6], tm[6];
      tip_diag(r, t);
      mass_diag(mass_coef(q, rotary), {q.dx, q.dy, q.dz}, tm);
#pragma unroll
      for (int k = 0; k < 6; ++k) dg[k] += c_K * t[k] + c_M * tm[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) dg[k] = lpn_sum<LPN>(dg[k]);
  if (i < N && sub == 0) {
    const unsigned fb = fixedbits ? fixedbits[i] : 0u;
    const double nm = node_mass ? c_M * node_mass[i] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double v = dg[k] + (k < 3 ? nm : 0.0);
      diag[6 * i + k] = v;
      if (dinv) dinv[6 * i + k] = (((fb >> k) & 1u) || v == 0.0) ? 0.0 : 1.0 / v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Step kernels: one thread per dof.  st, Ks, Ms are column blocks of four, [u | v | a | 0] and K, M applied to it (two 16-byte
// accesses per dof); everything else is a plain [6N] vector.
// ---------------------------------------------------------------------------------------------------------
enum { DYN_E_KIN = 0, DYN_E_STRAIN = 1, DYN_E_WORK = 2, DYN_E_COUNT = 3 };

struct NewmarkCoef {
  double dt, beta, gamma, ray_m, ray_k;
};

// Energies of the state (erow >= 0): 1/2 v.M v and 1/2 u.K u into the slots of row erow.  form != 0: the predictors ut, vt,
// the load f = sum_p amp[p] F_p (0 on fixed dofs) and the right-hand side r = f - K ut - ray_m M vt - ray_k K vt.
__global__ __launch_bounds__(kBlock) void k_newmark_predict(int64_t n6, const double *__restrict__ st,
                                                            const double *__restrict__ Ks, const double *__restrict__ Ms,
                                                            const uint8_t *__restrict__ fixedbits, NewmarkCoef q, int form,
                                                            int n_pat, const double *__restrict__ pattern,
                                                            const double *__restrict__ amp, double *__restrict__ ut,
                                                            double *__restrict__ vt, double *__restrict__ f,
                                                            double *__restrict__ r, double *__restrict__ energy, int erow) {
  __shared__ double red[2][kBlock / kWave];
  double s[2] = {0.0, 0.0};
  const double c1 = q.dt, c2 = q.dt * q.dt * (0.5 - q.beta), c3 = q.dt * (1.0 - q.gamma);
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const double2 *sp = reinterpret_cast<const double2 *>(st + 4 * e);
    const double2 *kp = reinterpret_cast<const double2 *>(Ks + 4 * e);
    const double2 *mp = reinterpret_cast<const double2 *>(Ms + 4 * e);
    const double2 s0 = sp[0], s1 = sp[1], k0 = kp[0], k1 = kp[1], m0 = mp[0], m1 = mp[1];
    const double u = s0.x, v = s0.y, a = s1.x;
    s[0] += 0.5 * v * m0.y;
    s[1] += 0.5 * u * k0.x;
    if (form) {
      const double Kut = k0.x + c1 * k0.y + c2 * k1.x, Kvt = k0.y + c3 * k1.x, Mvt = m0.y + c3 * m1.x;
      double fv = 0.0;
      if (!dof_fixed(fixedbits, e))
        for (int p = 0; p < n_pat; ++p) fv += amp[p] * pattern[(size_t)p * n6 + e];
      ut[e] = u + c1 * v + c2 * a;
      vt[e] = v + c3 * a;
      f[e] = fv;
      r[e] = fv - Kut - q.ray_m * Mvt - q.ray_k * Kvt;
    }
  }
  if (erow >= 0) {   // kernel-uniform
    double *dst[2] = {energy + ((size_t)erow * DYN_E_COUNT + DYN_E_KIN) * kSlots,
                      energy + ((size_t)erow * DYN_E_COUNT + DYN_E_STRAIN) * kSlots};
    block_add_slots<2>(s, red, dst);
  }
}

// u = ut + beta dt^2 a, v = vt + gamma dt a into the state; the trapezoid 1/2 (f_prev + f_cur).(u - u_old) into the work slots of
// `row`; the u, v, a rows of the probed nodes (probe_slot[node] >= 0) into probe[row]; u into snap if asked for.
__global__ __launch_bounds__(kBlock) void k_newmark_correct(int64_t n6, const double *__restrict__ ut,
                                                            const double *__restrict__ vt, const double *__restrict__ a_new,
                                                            const double *__restrict__ f_prev, const double *__restrict__ f_cur,
                                                            NewmarkCoef q, double *__restrict__ st,
                                                            const int32_t *__restrict__ probe_slot, int n_probe,
                                                            double *__restrict__ probe, double *__restrict__ snap,
                                                            double *__restrict__ energy, int row) {
  __shared__ double red[1][kBlock / kWave];
  double s[1] = {0.0};
  const double cu = q.beta * q.dt * q.dt, cv = q.gamma * q.dt;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    double2 *sp = reinterpret_cast<double2 *>(st + 4 * e);
    const double a = a_new[e], u_old = sp[0].x;
    const double u = ut[e] + cu * a, v = vt[e] + cv * a;
    s[0] += 0.5 * (f_prev[e] + f_cur[e]) * (u - u_old);
    sp[0] = {u, v};
    sp[1] = {a, 0.0};
    const int64_t node = e / 6;
    const int slot = probe_slot[node];
    if (slot >= 0) {
      double *o = probe + ((size_t)row * 3 * n_probe + slot) * 6 + (e - 6 * node);
      o[0] = u;
      o[(size_t)6 * n_probe] = v;
      o[(size_t)12 * n_probe] = a;
    }
    if (snap) snap[e] = u;
  }
  double *dst[1] = {energy + ((size_t)row * DYN_E_COUNT + DYN_E_WORK) * kSlots};
  block_add_slots<1>(s, red, dst);
}

}  // namespace pl

namespace {

// widest column block the fused gather is built for (make resource-usage: no scratch at 1 and 2)
constexpr int kDynKB = pl::DynTerm::kMaxKB;

// column blocks of the fused product: KB = min(n_rhs, kDynKB)
inline MultiShape dyn_shape(const pl_context *c, int n_rhs) {
  MultiShape s;
  s.n_rhs = n_rhs;
  s.KB = std::min(n_rhs, kDynKB);
  s.ncb = (n_rhs + s.KB - 1) / s.KB;
  s.ncol = s.ncb * s.KB;
  s.stride = c->N * 6 * s.KB;
  return s;
}

// y_j = (c_K K + c_M M) x_j (masked: P (...)) for every column of the shape, one launch; the mass records must be current
int launch_dyn_multi(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x, double *y,
                     bool masked, double *dot_dev) {
  if (s.KB > kDynKB) return fail(PL_ERR_ARG, "the fused K, M product is built for column blocks of 1 and 2");   // a missing kernel is an error
  return launch_gather_multi(c, s, pl::DynTerm{c->rec.p, mass_term(op.mass), op.c_K, op.c_M}, fixedbits, x, y, masked, dot_dev);
}

int launch_dyn_diag(pl_context *c, const MultiOp &op, const uint8_t *fixedbits, double *diag, double *dinv) {
  const unsigned g = grid_for(c->n_slices, pl::kBlock / pl::kWave);
  const MassWs *m = op.mass;
#define PL_D(L)                                                                                                            \
  hipLaunchKernelGGL((pl::k_dyn_diag_gather<L>), dim3(g), dim3(pl::kBlock), 0, c->stream, c->N, c->slice_ptr.p, c->ent.p, \
                     (const pl::Record *)c->rec.p, (const pl::MassRecord *)m->rec.p, m->rotary, m->nm(), op.c_K, op.c_M,  \
                     fixedbits, diag, dinv)
  switch (c->lpn) { case 1: PL_D(1); break; case 2: PL_D(2); break; case 4: PL_D(4); break; case 8: PL_D(8); break;
                    default: PL_D(16); }
#undef PL_D
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// Device data of one pl_transient call, owned by the handle (pl_context::dyn_ws), grown on demand.
struct DynWs {
  DevBuf<double> st, Ks, Ms;       // [6N][4]: the state [u | v | a | 0] and K, M applied to it
  DevBuf<double> ut, vt, f2;       // predictors [6N], the loads of the two last rows [2][6N]
  DevBuf<double> pattern, amp;     // [n_pat][6N] (device numbering, 0 on fixed dofs), [rows][n_pat]
  DevBuf<int32_t> probe_slot;      // [N]: row of the node in the probe block, -1 = not probed
  DevBuf<double> probe, energy;    // [rows][3][n_slot][6], [rows][DYN_E_COUNT][kSlots]
  DevBuf<double> snaps;            // [n_snap][6N]
};

template <typename T>
hipError_t dyn_grow(DevBuf<T> &b, size_t n) {
  return b.n < n ? b.alloc(n) : hipSuccess;
}

// ---- what the response calls (pl_transient, pl_harmonic, their _sens) share; first a PL_TIMING line (tools/time_*.py read it) ----
inline void timing_ms(const char *who, const char *label, double ms) { std::fprintf(stderr, "[%s] %-28s %10.4f ms\n", who, label, ms); }
inline void timing_count(const char *who, const char *label, int n) { std::fprintf(stderr, "[%s] %-28s %10d\n", who, label, n); }
inline void timing_mean(const char *who, const char *label, double v, const char *unit = "") {
  std::fprintf(stderr, "[%s] %-28s %10.2f%s\n", who, label, v, unit);
}
inline int check_rayleigh(const std::string &who, double ray_m, double ray_k) {
  if (!(ray_m >= 0.0) || !(ray_k >= 0.0) || !std::isfinite(ray_m) || !std::isfinite(ray_k))
    return fail(PL_ERR_ARG, who + ": the Rayleigh coefficients must be finite and not negative");
  return PL_OK;
}
inline int check_solve(const std::string &who, double rtol, int32_t max_iter) {
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, who + ": rtol and max_iter must be positive");
  return PL_OK;
}
inline int check_omega(const std::string &who, int32_t n_freq, const double *omega) {
  if (n_freq < 1) return fail(PL_ERR_ARG, who + ": n_freq must be at least 1");
  for (int i = 0; i < n_freq; ++i)
    if (!(omega[i] >= 0.0) || !std::isfinite(omega[i])) return fail(PL_ERR_ARG, who + ": omega must be finite and not negative");
  return PL_OK;
}
inline int check_kind(const std::string &who, int32_t kind, double p) {
  if (kind < 0 || kind > 2) return fail(PL_ERR_ARG, who + ": kind must be 0, 1 or 2");
  if (kind == 2 && !(p >= 2.0 && std::isfinite(p))) return fail(PL_ERR_ARG, who + ": p must be at least 2 (and finite)");
  return PL_OK;
}
inline int check_weights(const std::string &who, const double *weight, int rows) {
  for (int n = 0; weight && n < rows; ++n)
    if (!(weight[n] >= 0.0) || !std::isfinite(weight[n])) return fail(PL_ERR_ARG, who + ": the weights must be finite and not negative");
  return PL_OK;
}
inline int check_probes(const std::string &who, int32_t n_probe, const int32_t *probe_nodes, int64_t N) {
  for (int i = 0; i < n_probe; ++i)
    if (probe_nodes[i] < 0 || probe_nodes[i] >= N) return fail(PL_ERR_ARG, who + ": probe node index out of range");
  return PL_OK;
}

// The probed nodes, each once: their rows in the device's probe block by device node (-1: not probed) and by probe; returns the rows
inline int probe_map(const pl_context *c, int32_t n_probe, const int32_t *probe_nodes, std::vector<int32_t> &slot_of,
                     std::vector<int32_t> &probe_to_slot) {
  int n_slot = 0;
  slot_of.assign((size_t)c->N, -1);
  probe_to_slot.resize((size_t)n_probe);
  for (int i = 0; i < n_probe; ++i) {
    const int64_t di = c->iperm[probe_nodes[i]];
    if (slot_of[(size_t)di] < 0) slot_of[(size_t)di] = n_slot++;
    probe_to_slot[(size_t)i] = slot_of[(size_t)di];
  }
  return n_slot;
}

// sum[r] of `rows` reduction scalars on the device: their kSlots partial sums added in ascending order (the sums keep their bits)
inline int download_slot_sums(pl_context *c, const double *slots_dev, size_t rows, double *sum) {
  std::vector<double> sl(rows * pl::kSlots);
  PL_HIP(hipMemcpyAsync(sl.data(), slots_dev, sl.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  for (size_t r = 0; r < rows; ++r) sum[r] = std::accumulate(&sl[r * pl::kSlots], &sl[r * pl::kSlots] + pl::kSlots, 0.0);
  return PL_OK;
}

// e_dir, the rigid translation of ALL nodes along dir[3] (supports included), into edir_dev and P M e_dir into out_dev
inline int base_load(pl_context *c, MultiWs *w, const MassWs *m, const double *dir, double *edir_dev, double *out_dev) {
  const MultiShape s1 = multi_shape(c, 1);
  std::vector<double> e((size_t)c->N * 6, 0.0);
  for (int64_t i = 0; i < c->N; ++i)
    for (int k = 0; k < 3; ++k) e[(size_t)(6 * i + k)] = dir[k];
  if (int rc = multi_upload(c, w, s1, e.data(), edir_dev, 0)) return rc;
  return launch_mass_multi(c, m, s1, edir_dev, out_dev, true);
}

// One solve of a transient row, (c_K K + c_M M) w->U = w->F.  `what` names it where it misses rtol ("the [forward | adjoint ]solve
// of step"); where a norm is not a number only the adjoint is named in full.  *ms gains the host time of the solve.
inline int transient_solve(pl_context *c, MultiWs *w, const MultiOp &op, double rtol, int32_t max_iter, const std::string &who,
                           const char *what, int row, int *iters, double *ms) {
  const MultiShape s1 = multi_shape(c, 1);
  std::vector<double> status((size_t)pl::M_ST_COUNT * s1.ncol);
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = pcg_solve_multi(c, w, s1, c->fixedbits.p, w->F.p, rtol, max_iter, status.data(), op)) return rc;
  *ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const double rr = status[pl::M_ST_RR * s1.ncol], bb = status[pl::M_ST_BB * s1.ncol];
  *iters = (int)status[pl::M_ST_ITER * s1.ncol];
  if (!std::isfinite(rr) || !std::isfinite(bb))
    return fail(PL_ERR_NAN, who + ": NaN/Inf in a residual norm of " + (std::strstr(what, "adjoint") ? what : "step") + " " +
                                std::to_string(row));
  if (!(rr <= rtol * rtol * bb))
    return fail(PL_ERR_NOCONV, who + ": " + what + " " + std::to_string(row) + " did not reach rtol within max_iter");
  return PL_OK;
}

}  // namespace
