// Steady heat conduction on the strut graph: conductances, the scalar graph Laplacian K_T and its Jacobi PCG, strut heat flows
// and the two contractions that close the thermo-elastic adjoint chain (pl_set_conduction / pl_cond_spmv / pl_cond_solve /
// pl_cond_flux / pl_cond_sens / pl_thermal_load_adjoint).  gfx950 only, fp64, wave 64.
//
// Strut b joins A = conn[2b] and B = conn[2b+1], d = x_B - x_A, L = |d|.  Each strut is ONE two-node conductor of uniform
// circular section of the plain radius r over the node-to-node length (the convention of K_g and M): penalised end zones and the
// overlap at the joints are ignored, a multiplicity k counts k times.
//     g_b = k_b kappa_b pi r_b^2 / L_b                     conductance,  d g_b / d r_b = 2 g_b / r_b
//     (K_T T)_i = sum over struts b at i of g_b (T_i - T_other)
//     K_T T = q on the free nodes, T = T_bar on the nodes of a one-byte-per-node mask (not the mechanical mask of pl_set_bc)
//     Q_b = g_b (T_A - T_B) / k_b                          heat flow of ONE copy of the strut from A to B
// Coupling to the thermal loads (pl_thermal.h): with dT = T - T_ref, the transpose of d f_th / d dT applied to a field lam is
//     c_i = sum over struts b at i of (1/2) alpha_b ka_b d_b . (lam_u,B - lam_u,A),   ka_b = rec.a + rec.e1 L^2
// (both ends of a strut receive the same term; L t = d), and with K_T mu = c on the free thermal nodes, mu = 0 on the others,
//     dq/dr_b += - mu^T (dK_T / dr_b) T = - (2 g_b / r_b) (mu_A - mu_B) (T_A - T_B).
//
// k_cond_gather, k_cond_diag and k_thermal_load_adjoint are per-node gathers over the sliced-ELL incidence in its stored order
// (the lane mapping of k_thermal_load): no floating-point atomics in the product, no [B] intermediate besides g, equal inputs
// give equal bits.  The PCG's vector kernels are the KB = 1 kernels of pl_multi.h on N scalars; their reduction scalars and the
// p . K_T p of k_cond_gather are summed by atomics over 64 slots, so the SOLVE is not bitwise reproducible once the grid has
// more than 64 blocks.
#pragma once
#include "pl_context.h"
#include "pl_multi.h"
#include "pl_thermal.h"

namespace pl {

// One thread per strut: g[b] = k kappa pi r^2 / L from the current radius and record.
__global__ __launch_bounds__(kBlock) void k_cond_strut(int64_t B, const Record *__restrict__ rec,
                                                       const double *__restrict__ radius, const double *__restrict__ mult,
                                                       const double *__restrict__ kappa, double *__restrict__ g) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double2 *q = reinterpret_cast<const double2 *>(rec + b);
  const double2 q2 = q[2], q3 = q[3];
  const double L2 = q2.y * q2.y + q3.x * q3.x + q3.y * q3.y;
  const double r = radius[b];
  g[b] = (mult ? mult[b] : 1.0) * kappa[b] * (3.14159265358979323846 * r * r) / sqrt(L2);
}

// One thread per node, its struts in their stored order: y_i = sum g_b (x_i - x_other); MASK: y_i = 0 on a fixed node and x is
// taken as 0 there by the caller (P K_T P x).  dot_out != null: x . y is added to the 64 slots of dot_out (the p . K_T p of the PCG).
template <bool MASK>
__global__ __launch_bounds__(kBlock) void k_cond_gather(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                        const int2 *__restrict__ ent, const double *__restrict__ g,
                                                        const uint8_t *__restrict__ fixed, const double *__restrict__ x,
                                                        double *__restrict__ y, double *__restrict__ dot_out) {
  __shared__ double red[1][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[1] = {0.0};
  if (i < N) {
    const int64_t s = i / SN, n = i - s * SN;
    const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
    const double xs = x[i];
    double out = 0.0;
    for (int64_t j = 0; j < width; ++j) {
      const int2 e = ent[p0 + j * SN + n];
      if (e.x < 0) continue;
      out += g[e.y & 0x7fffffff] * (xs - x[e.x]);
    }
    if (MASK && fixed[i]) out = 0.0;
    y[i] = out;
    acc[0] = xs * out;
  }
  if (dot_out) {   // kernel-uniform
    double *dst[1] = {dot_out};
    block_add_slots<1>(acc, red, dst);
  }
}

// The Jacobi diagonal of K_T by the same walk: diag_i = sum g_b, dinv_i = 1 / diag_i on a free node and 0 on a fixed one.
__global__ __launch_bounds__(kBlock) void k_cond_diag(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                      const int2 *__restrict__ ent, const double *__restrict__ g,
                                                      const uint8_t *__restrict__ fixed, double *__restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  double dg = 0.0;
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x >= 0) dg += g[e.y & 0x7fffffff];
  }
  dinv[i] = (fixed[i] || !(dg > 0.0)) ? 0.0 : 1.0 / dg;
}

// Scalar twin of k_multi_init<1> (one mask byte per node instead of six bits):
// r = P (q - K_T T_bar) ; z = dinv r ; p = z ; x = 0 ; rz_old = r.z ; bb = r.r        (q == null: no inflow)
__global__ __launch_bounds__(kBlock) void k_cond_init(int64_t N, const double *__restrict__ q, const double *__restrict__ Kt,
                                                      const uint8_t *__restrict__ fixed, const double *__restrict__ dinv,
                                                      double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                      double *__restrict__ p, double *__restrict__ set0,
                                                      double *__restrict__ bb) {
  __shared__ double red[2][kBlock / kWave];
  double s[2] = {0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < N; e += (int64_t)gridDim.x * kBlock) {
    const double rv = fixed[e] ? 0.0 : ((q ? q[e] : 0.0) - Kt[e]);
    const double zv = dinv[e] * rv;
    s[0] += rv * zv;
    s[1] += rv * rv;
    x[e] = 0.0;
    r[e] = rv;
    z[e] = zv;
    p[e] = zv;
  }
  double *dst[2] = {slots_of(set0, M_RZ_OLD, 1, 0), bb};
  block_add_slots<2>(s, red, dst);
}

// Scalar twin of k_multi_compose<1>: T = fixed ? T_bar : x
__global__ __launch_bounds__(kBlock) void k_cond_compose(int64_t N, const uint8_t *__restrict__ fixed,
                                                         const double *__restrict__ tbar, const double *__restrict__ x,
                                                         double *__restrict__ T) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < N; e += (int64_t)gridDim.x * kBlock)
    T[e] = fixed[e] ? tbar[e] : x[e];
}

// One thread per strut, no scatter: Q[b] = g (T_A - T_B) / k, the heat flow of one copy from A to B.
__global__ __launch_bounds__(kBlock) void k_cond_flux(int64_t B, const int32_t *__restrict__ conn,
                                                      const double *__restrict__ mult, const double *__restrict__ g,
                                                      const double *__restrict__ T, double *__restrict__ Q) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  Q[b] = g[b] * (T[ia] - T[ib]) / (mult ? mult[b] : 1.0);
}

// One thread per strut, no scatter: out[b] = (2 g / r) (mu_A - mu_B) (T_A - T_B) = mu^T (dK_T / dr_b) T.
__global__ __launch_bounds__(kBlock) void k_cond_sens(int64_t B, const int32_t *__restrict__ conn,
                                                      const double *__restrict__ radius, const double *__restrict__ g,
                                                      const double *__restrict__ T, const double *__restrict__ mu,
                                                      double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  out[b] = (2.0 * g[b] / radius[b]) * (mu[ia] - mu[ib]) * (T[ia] - T[ib]);
}

// One thread per node, its struts in their stored order (the lane mapping of k_thermal_load): c_i = sum of
// (1/2) alpha ka d . (lam_u,B - lam_u,A).  The node is the strut's end B unless bit 31 of the entry is set.
__global__ __launch_bounds__(kBlock) void k_thermal_load_adjoint(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                                 const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                                 const double *__restrict__ alpha,
                                                                 const double *__restrict__ lam, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  V3 ls, ms;
  load6(lam + 6 * i, ls, ms);
  double c = 0.0;
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x < 0) continue;
    const int64_t b = e.y & 0x7fffffff;
    const double2 *q = reinterpret_cast<const double2 *>(rec + b);
    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const V3 d = {q2.y, q3.x, q3.y};
    V3 lo, mo;
    load6(lam + 6 * (int64_t)e.x, lo, mo);
    const V3 dl = e.y < 0 ? lo - ls : ls - lo;     // lam_u,B - lam_u,A
    c += (0.5 * alpha[b] * (q0.x + q1.x * dot(d, d))) * dot(d, dl);
  }
  out[i] = c;
}

}  // namespace pl

namespace {

// Conduction state of the handle (pl_context::cond_ws), set by pl_set_conduction, device numbering: kappa[B]; g[B] is rebuilt
// from the current radii and records by every call that reads it; the rest is the workspace of the calls (N scalars each).
struct CondWs {
  DevBuf<double> kappa, g, out;                          // [B]
  DevBuf<double> X, R, Z, P, AP, KT, TB, QF, T, MU, dinv, lam6;   // [N] (lam6: [6N], first pl_thermal_load_adjoint)
  DevBuf<uint8_t> fixed;                                 // [N]
  DevBuf<double> scal;   // [2 sets][M_COUNT][kSlots] | bb [kSlots] | thresh | status [M_ST_COUNT]   (one column)
  DevBuf<int> flags;     // [2]
};

inline MultiScal cond_scal(CondWs *w) {
  MultiScal m;
  const size_t set = (size_t)pl::M_COUNT * pl::kSlots;
  m.set[0] = w->scal.p;
  m.set[1] = m.set[0] + set;
  m.bb = m.set[1] + set;
  m.thresh = m.bb + pl::kSlots;
  m.status = m.thresh + 1;
  m.flag[0] = w->flags.p;
  m.flag[1] = w->flags.p + 1;
  return m;
}
constexpr size_t kCondScal = (size_t)(2 * pl::M_COUNT + 1) * pl::kSlots + 1 + pl::M_ST_COUNT;

// N scalars between the caller's node numbering and the device's (host == null: zeros; zero_fixed: 0 on the nodes of `fixed`,
// caller's numbering - the operand of the masked product)
int cond_upload(pl_context *c, const double *host, double *dev, const uint8_t *zero_fixed = nullptr) {
  const size_t N = (size_t)c->N;
  if (!host) {
    PL_HIP(hipMemsetAsync(dev, 0, N * sizeof(double), c->stream));
    return PL_OK;
  }
  std::vector<double> st(N);
  for (size_t i = 0; i < N; ++i) {
    const size_t src = (size_t)c->perm[i];
    st[i] = (zero_fixed && zero_fixed[src]) ? 0.0 : host[src];
  }
  PL_HIP(hipMemcpyAsync(dev, st.data(), N * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  return PL_OK;
}
int cond_upload_mask(pl_context *c, const uint8_t *host, uint8_t *dev) {
  const size_t N = (size_t)c->N;
  std::vector<uint8_t> st(N);
  for (size_t i = 0; i < N; ++i) st[i] = host[(size_t)c->perm[i]] ? 1 : 0;
  PL_HIP(hipMemcpyAsync(dev, st.data(), N, hipMemcpyHostToDevice, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  return PL_OK;
}
int cond_download(pl_context *c, const double *dev, double *host) {
  const size_t N = (size_t)c->N;
  std::vector<double> st(N);
  PL_HIP(hipMemcpyAsync(st.data(), dev, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < N; ++i) host[(size_t)c->perm[i]] = st[i];
  return PL_OK;
}

// y = K_T x (masked: P K_T x, x zero on the fixed nodes); dot_dev != null: x . y into its 64 slots
inline void launch_cond_gather(pl_context *c, CondWs *w, bool masked, const double *x, double *y, double *dot_dev) {
  const auto kernel = masked ? pl::k_cond_gather<true> : pl::k_cond_gather<false>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(c->N)), dim3(pl::kBlock), 0, c->stream, c->N, pl::kWave / c->lpn,
                     (const int64_t *)c->slice_ptr.p, (const int2 *)c->ent.p, (const double *)w->g.p,
                     (const uint8_t *)w->fixed.p, x, y, dot_dev);
}

// K_T x = q on the free nodes of w->fixed, x = T_bar on the others: w->TB (T_bar, zero on the free nodes) and q_dev (null: no
// inflow) hold the data, `out` receives the full field.  Jacobi PCG from x0 = 0 in the manner of pcg_solve_multi with one
// column: three launches per iteration (k_cond_gather with p . K_T p, k_multi_update<1>, k_multi_direction<1>), stopped on the
// device by ||r|| <= rtol ||b||; the host looks at the status block every check_every iterations.
int cond_pcg(pl_context *c, CondWs *w, const double *q_dev, double rtol, int max_iter, double *out, double *status_host) {
  const int64_t N = c->N;
  const MultiScal m = cond_scal(w);
  PL_HIP(hipMemsetAsync(w->scal.p, 0, kCondScal * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(w->flags.p, 0, 2 * sizeof(int), c->stream));
  hipLaunchKernelGGL(pl::k_cond_diag, dim3(grid_for(N)), dim3(pl::kBlock), 0, c->stream, N, pl::kWave / c->lpn,
                     (const int64_t *)c->slice_ptr.p, (const int2 *)c->ent.p, (const double *)w->g.p,
                     (const uint8_t *)w->fixed.p, w->dinv.p);
  launch_cond_gather(c, w, false, w->TB.p, w->KT.p, nullptr);   // lifting: K_T T_bar
  const dim3 g(grid_stream(N));
  hipLaunchKernelGGL(pl::k_cond_init, g, dim3(pl::kBlock), 0, c->stream, N, q_dev, (const double *)w->KT.p,
                     (const uint8_t *)w->fixed.p, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, w->P.p, m.set[0], m.bb);
  hipLaunchKernelGGL(pl::k_multi_begin, dim3(1), dim3(pl::kWave), 0, c->stream, 1, rtol, (const double *)m.bb, m.thresh,
                     m.status, m.flag[0]);
  PL_HIP(hipGetLastError());
  const int every = c->opt.check_every > 0 ? c->opt.check_every : 16;
  const size_t st_bytes = (size_t)pl::M_ST_COUNT * sizeof(double);
  auto look = [&]() -> int {     // 1: the column is frozen
    if (hipMemcpyAsync(status_host, m.status, st_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return -1;
    return status_host[pl::M_ST_FROZEN] == 0.0 ? 0 : 1;
  };
  int it = 0, all = look();
  while (all == 0 && it < max_iter) {
    const int stop = std::min(max_iter, it + every);
    for (; it < stop; ++it) {
      const int a = it & 1, b = a ^ 1;
      launch_cond_gather(c, w, true, w->P.p, w->AP.p, m.set[a] + (size_t)pl::M_PAP * pl::kSlots);
      hipLaunchKernelGGL((pl::k_multi_update<1>), g, dim3(pl::kBlock), 0, c->stream, N, (const double *)w->P.p,
                         (const double *)w->AP.p, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, m.set[a],
                         (const int *)m.flag[a], 1, N);
      hipLaunchKernelGGL((pl::k_multi_direction<1>), g, dim3(pl::kBlock), 0, c->stream, N, (const double *)w->Z.p, w->P.p,
                         (const double *)m.set[a], m.set[b], (const int *)m.flag[a], m.flag[b], (const double *)m.thresh,
                         m.status, it, 1, N);
    }
    PL_HIP(hipGetLastError());
    all = look();
  }
  if (all < 0) return fail(PL_ERR_HIP, "pl_cond_solve: download of the status block failed");
  hipLaunchKernelGGL(pl::k_cond_compose, g, dim3(pl::kBlock), 0, c->stream, N, (const uint8_t *)w->fixed.p,
                     (const double *)w->TB.p, (const double *)w->X.p, out);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

}  // namespace
