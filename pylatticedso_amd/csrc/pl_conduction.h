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
// Lumped strut-surface convection (pl_set_convection): each end of strut b exchanges with an ambient at
// T_inf through the film conductance c_b = k_b h_b pi r_b L_b (half the lateral surface of every copy), d c_b / d r_b = c_b / r_b:
//     H_i = sum over struts b at i of c_b,   (K_T + diag H) T = q + H T_inf on the free nodes,
//     Qc_b = c_b [(T_A - T_inf) + (T_B - T_inf)] / k_b     convective loss of ONE copy,   P = sum_b k_b Qc_b
//     mu^T d[(K_T + H) T - H T_inf]/dr_b = (2 g_b / r_b)(mu_A - mu_B)(T_A - T_B) + (c_b / r_b)[mu_A (T_A - T_inf) + mu_B (T_B - T_inf)].
// The CONV instantiations carry it; without a convection state the plain ones are launched, as before.
// Temperature p-norm (pl_temp_pnorm): Phi_p = (sum over a node set of max(T_i - T_ref, 0)^p)^(1/p) in the four steps of the
// stress p-norm (values + block maxima, fold, p-sum, fold) and dPhi/dT per node; P and Phi_p fold in two fixed-order stages.
//
// k_cond_gather, k_cond_diag and k_thermal_load_adjoint are per-node gathers over the sliced-ELL incidence in its stored order
// (the lane mapping of k_thermal_load): no floating-point atomics in the product, no [B] intermediate besides g, equal inputs
// give equal bits.  The PCG's vector kernels are the KB = 1 kernels of pl_multi.h on N scalars; their reduction scalars and the
// p . K_T p of k_cond_gather are summed by atomics over 64 slots, so the SOLVE is not bitwise reproducible once the grid has
// more than 64 blocks.
#pragma once
#include "pl_context.h"
#include "pl_multi.h"
#include "pl_stress.h"
#include "pl_thermal.h"

namespace pl {

// What the strut passes share (k_cond_strut, k_heat_strut of pl_heat.h), so that every call forms the same bits: the squared
// node-to-node length of the record, g = k kappa pi r^2 / L and c = k h pi r L.
__device__ __forceinline__ double strut_length2(const Record *__restrict__ rec, int64_t b) {
  const double2 *q = reinterpret_cast<const double2 *>(rec + b);
  const double2 q2 = q[2], q3 = q[3];
  return q2.y * q2.y + q3.x * q3.x + q3.y * q3.y;
}
__device__ __forceinline__ double strut_conductance(const double *__restrict__ mult, const double *__restrict__ kappa, int64_t b,
                                                    double r, double L2) {
  return (mult ? mult[b] : 1.0) * kappa[b] * (3.14159265358979323846 * r * r) / sqrt(L2);
}
__device__ __forceinline__ double strut_film(const double *__restrict__ mult, const double *__restrict__ film, int64_t b, double r,
                                             double L2) {
  return (mult ? mult[b] : 1.0) * film[b] * (3.14159265358979323846 * r) * sqrt(L2);
}

// One thread per strut: g[b] = k kappa pi r^2 / L from the current radius and record; CONV: also c[b] = k h pi r L.
template <bool CONV = false>
__global__ __launch_bounds__(kBlock) void k_cond_strut(int64_t B, const Record *__restrict__ rec,
                                                       const double *__restrict__ radius, const double *__restrict__ mult,
                                                       const double *__restrict__ kappa, double *__restrict__ g,
                                                       const double *__restrict__ film, double *__restrict__ c) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double L2 = strut_length2(rec, b);
  const double r = radius[b];
  g[b] = strut_conductance(mult, kappa, b, r, L2);
  if (CONV) c[b] = strut_film(mult, film, b, r, L2);
}

// CONV only, one thread per node, its struts in their stored order: H_i = sum c_b.
__global__ __launch_bounds__(kBlock) void k_cond_hdiag(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                       const int2 *__restrict__ ent, const double *__restrict__ c,
                                                       double *__restrict__ H) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  double hs = 0.0;
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x >= 0) hs += c[e.y & 0x7fffffff];
  }
  H[i] = hs;
}

// One thread per node, its struts in their stored order: y_i = sum g_b (x_i - x_other); MASK: y_i = 0 on a fixed node and x is
// taken as 0 there by the caller (P K_T P x).  dot_out != null: x . y is added to the 64 slots of dot_out (the p . K_T p of the PCG).
// CONV: y_i += H_i x_i, one more 8-byte load per node (H is not read without it).
template <bool MASK, bool CONV = false>
__global__ __launch_bounds__(kBlock) void k_cond_gather(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                        const int2 *__restrict__ ent, const double *__restrict__ g,
                                                        const uint8_t *__restrict__ fixed, const double *__restrict__ x,
                                                        double *__restrict__ y, double *__restrict__ dot_out,
                                                        const double *__restrict__ H) {
  __shared__ double red[1][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[1] = {0.0};
  if (i < N) {
    const int64_t s = i / SN, n = i - s * SN;
    const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
    const double xs = x[i];
    double hs = 0.0;
    if (CONV) hs = H[i];
    double out = 0.0;
    for (int64_t j = 0; j < width; ++j) {
      const int2 e = ent[p0 + j * SN + n];
      if (e.x < 0) continue;
      out += g[e.y & 0x7fffffff] * (xs - x[e.x]);
    }
    if (CONV) out += hs * xs;
    if (MASK && fixed[i]) out = 0.0;
    y[i] = out;
    acc[0] = xs * out;
  }
  if (dot_out) {   // kernel-uniform
    double *dst[1] = {dot_out};
    block_add_slots<1>(acc, red, dst);
  }
}

// The Jacobi diagonal of K_T by the same walk: diag_i = sum g_b (CONV: + H_i), dinv_i = 1 / diag_i on a free node and 0 on a
// fixed one.
template <bool CONV = false>
__global__ __launch_bounds__(kBlock) void k_cond_diag(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                      const int2 *__restrict__ ent, const double *__restrict__ g,
                                                      const uint8_t *__restrict__ fixed, double *__restrict__ dinv,
                                                      const double *__restrict__ H) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  double dg = 0.0;
  if (CONV) dg = H[i];
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x >= 0) dg += g[e.y & 0x7fffffff];
  }
  dinv[i] = (fixed[i] || !(dg > 0.0)) ? 0.0 : 1.0 / dg;
}

// Scalar twin of k_multi_init<1> (one mask byte per node instead of six bits):
// r = P (q - K_T T_bar) ; z = dinv r ; p = z ; x = 0 ; rz_old = r.z ; bb = r.r        (q == null: no inflow)
// H != null (convection): Kt = (K_T + H) T_bar and the right-hand side gains H T_inf.
__global__ __launch_bounds__(kBlock) void k_cond_init(int64_t N, const double *__restrict__ q, const double *__restrict__ Kt,
                                                      const uint8_t *__restrict__ fixed, const double *__restrict__ dinv,
                                                      double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                      double *__restrict__ p, double *__restrict__ set0,
                                                      double *__restrict__ bb, const double *__restrict__ H, double T_inf) {
  __shared__ double red[2][kBlock / kWave];
  double s[2] = {0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < N; e += (int64_t)gridDim.x * kBlock) {
    const double rv = fixed[e] ? 0.0 : ((q ? q[e] : 0.0) + (H ? H[e] * T_inf : 0.0) - Kt[e]);
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
// CONV: + (c / r) [mu_A (T_A - T_inf) + mu_B (T_B - T_inf)] = mu^T d(H (T - T_inf)) / dr_b.
template <bool CONV = false>
__global__ __launch_bounds__(kBlock) void k_cond_sens(int64_t B, const int32_t *__restrict__ conn,
                                                      const double *__restrict__ radius, const double *__restrict__ g,
                                                      const double *__restrict__ T, const double *__restrict__ mu,
                                                      double *__restrict__ out, const double *__restrict__ c, double T_inf) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const double r = radius[b], ta = T[ia], tb = T[ib], ma = mu[ia], mb = mu[ib];
  double o = (2.0 * g[b] / r) * (ma - mb) * (ta - tb);
  if (CONV) o += (c[b] / r) * (ma * (ta - T_inf) + mb * (tb - T_inf));
  out[b] = o;
}

// One thread per strut, no scatter: Qc[b] = c [(T_A - T_inf) + (T_B - T_inf)] / k, the convective loss of one copy; part != null:
// the block's sum of k Qc in the fixed tree, one partial per block (first stage of P).
__global__ __launch_bounds__(kBlock) void k_cond_film(int64_t B, const int32_t *__restrict__ conn,
                                                      const double *__restrict__ mult, const double *__restrict__ c,
                                                      const double *__restrict__ T, double T_inf, double *__restrict__ Qc,
                                                      double *__restrict__ part) {
  __shared__ double smem[kBlock];
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double loss = 0.0;
  if (b < B) {
    const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
    loss = c[b] * ((T[ia] - T_inf) + (T[ib] - T_inf));
    if (Qc) Qc[b] = loss / (mult ? mult[b] : 1.0);
  }
  if (part) {   // kernel-uniform
    const double t = stress_block_fold<false>(loss, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}

// Second stage of P: ONE block walks the n partials in a fixed stride and folds them in the fixed tree (k_stress_fold's order).
__global__ __launch_bounds__(kBlock) void k_cond_film_fold(int64_t n, const double *__restrict__ part, double *__restrict__ total) {
  __shared__ double smem[kBlock];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) v += part[i];
  v = stress_block_fold<false>(v, smem);
  if (threadIdx.x == 0) total[0] = v;
}

// Temperature p-norm, node pass: v_i = max(T_i - T_ref, 0) on the nodes of the set (nodes == null: all), 0 elsewhere and for a
// NaN; the block maxima go to part_max (k_stress_stations' first stage).
__global__ __launch_bounds__(kBlock) void k_temp_values(int64_t N, const double *__restrict__ T, const uint8_t *__restrict__ nodes,
                                                        double T_ref, double *__restrict__ v, double *__restrict__ part_max) {
  __shared__ double smem[kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double val = 0.0;
  if (i < N) {
    const double d = T[i] - T_ref;
    if ((!nodes || nodes[i]) && d > 0.0) val = d;
    v[i] = val;
  }
  const double m = stress_block_fold<true>(val, smem);
  if (threadIdx.x == 0) part_max[blockIdx.x] = m;
}

// One thread per node: dPhi/dT_i = (v_i / v_max)^(p-1) (sum)^(1/p - 1) where v_i > 0, else 0; red = (v_max, sum, Phi_p).
__global__ __launch_bounds__(kBlock) void k_temp_pnorm_grad(int64_t N, const double *__restrict__ v,
                                                            const double *__restrict__ red, double p, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const double vmax = red[0], vi = v[i];
  out[i] = (vmax > 0.0 && vi > 0.0) ? pow(vi / vmax, p - 1.0) * pow(red[1], 1.0 / p - 1.0) : 0.0;
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
  DevBuf<double> film, c, H, part, total;                // convection (pl_set_convection): h [B], c [B], H [N], fold scratch
  bool conv = false;                                     // a convection state is set: the CONV kernels run
  double T_inf = 0.0;
  DevBuf<double> X, R, Z, P, AP, KT, TB, QF, T, MU, dinv, lam6;   // [N] (lam6: [6N], first pl_thermal_load_adjoint)
  DevBuf<uint8_t> fixed;                                 // [N]
  DevBuf<double> scal;   // [2 sets][M_COUNT][kSlots] | bb [kSlots] | thresh | status [M_ST_COUNT]   (one column)
  DevBuf<int> flags;     // [2]
  std::shared_ptr<void> heat;   // heat capacity and the device data of pl_cond_transient (pl_heat.h), set by pl_set_heat_capacity
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

// y = K_T x (masked: P K_T x, x zero on the fixed nodes; under a convection state K_T + H); dot_dev != null: x . y into its 64 slots
inline void launch_cond_gather(pl_context *c, CondWs *w, bool masked, const double *x, double *y, double *dot_dev) {
  const auto kernel = w->conv ? (masked ? pl::k_cond_gather<true, true> : pl::k_cond_gather<false, true>)
                              : (masked ? pl::k_cond_gather<true> : pl::k_cond_gather<false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(c->N)), dim3(pl::kBlock), 0, c->stream, c->N, pl::kWave / c->lpn,
                     (const int64_t *)c->slice_ptr.p, (const int2 *)c->ent.p, (const double *)w->g.p,
                     (const uint8_t *)w->fixed.p, x, y, dot_dev, w->conv ? (const double *)w->H.p : (const double *)nullptr);
}

// K_T x = q (under a convection state (K_T + H) x = q + H T_inf) on the free nodes of w->fixed, x = T_bar on the others: w->TB (T_bar, zero on the free nodes) and q_dev (null: no
// inflow) hold the data, `out` receives the full field.  Jacobi PCG from x0 = 0 in the manner of pcg_solve_multi with one
// column: three launches per iteration (k_cond_gather with p . K_T p, k_multi_update<1>, k_multi_direction<1>), stopped on the
// device by ||r|| <= rtol ||b||; the host looks at the status block every check_every iterations.
// ambient = false: the right-hand side is q alone (the adjoint problem (K_T + H) mu = q).
int cond_pcg(pl_context *c, CondWs *w, const double *q_dev, double rtol, int max_iter, double *out, double *status_host,
             bool ambient = true) {
  const int64_t N = c->N;
  const MultiScal m = cond_scal(w);
  PL_HIP(hipMemsetAsync(w->scal.p, 0, kCondScal * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(w->flags.p, 0, 2 * sizeof(int), c->stream));
  const double *H = w->conv ? (const double *)w->H.p : (const double *)nullptr;
  hipLaunchKernelGGL(w->conv ? pl::k_cond_diag<true> : pl::k_cond_diag<false>, dim3(grid_for(N)), dim3(pl::kBlock), 0, c->stream,
                     N, pl::kWave / c->lpn, (const int64_t *)c->slice_ptr.p, (const int2 *)c->ent.p, (const double *)w->g.p,
                     (const uint8_t *)w->fixed.p, w->dinv.p, H);
  launch_cond_gather(c, w, false, w->TB.p, w->KT.p, nullptr);   // lifting: K_T T_bar (convection: (K_T + H) T_bar)
  const dim3 g(grid_stream(N));
  hipLaunchKernelGGL(pl::k_cond_init, g, dim3(pl::kBlock), 0, c->stream, N, q_dev, (const double *)w->KT.p,
                     (const uint8_t *)w->fixed.p, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, w->P.p, m.set[0], m.bb,
                     ambient ? H : (const double *)nullptr, w->T_inf);
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
