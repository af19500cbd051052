// Euler buckling utilisation of every strut and its p-norm aggregate with derivatives (pl_buckling / pl_buckling_pnorm;
// DESIGN.md section 10c).  gfx950 only.  The sibling of the stress pass (pl_stress.h), whose axial force it reads.
//
// Per strut b, with (F, M_B) = tip_force(record, u) - under a thermal state of the handle (pl_set_thermal) the mechanical
// force F - ka delta t of load_strut<true>, the TH instantiation of both kernels - and the multiplicity k of pl_set_multiplicity:
//     N = F.t / k          signed axial force of ONE copy (tension > 0) - exactly the N of pl_stress (stress_strut)
//     P = max(0, -N)       compressive force
// Buckling length l:   length = 0: the node-to-node length |d|;
//                      length = 1: the middle segment seg_len[3b+1] (the penalised joint zones are rigid ends, the view
//                                  where = 1 takes for stresses); a strut without a middle segment is ABSENT: NaN in the
//                                  per-strut outputs, and it enters no sum.
// Critical load with the un-penalised radius r, I = pi r^4 / 4, S = pi r^2:
//     N_E  = pi^2 E I / (k_eff l)^2        Euler; k_eff = 1 pinned-pinned, 0.5 clamped-clamped
//     shear = 0: N_cr = N_E
//     shear = 1: N_cr = N_E / (1 + q),  q = N_E / (kappa G S)      Engesser load of a Timoshenko column
// Utilisation beta = P / N_cr >= 0: buckling is predicted at beta >= 1, a strut in tension has beta = 0 exactly.
//
// Aggregate B_p = (sum over present struts of beta^p)^(1/p), p >= 1, evaluated as beta_max (sum (beta / beta_max)^p)^(1/p);
// B_p = 0 and zero derivatives when beta_max = 0; the derivative of max(0, -N) at N = 0 is taken as zero.
// With w = dB/dbeta_b = (beta_b / beta_max)^(p-1) (sum (beta / beta_max)^p)^(1/p - 1) on compressed struts (0 elsewhere):
//     g_F = dB/dF = -w t / (k N_cr),  dB/dM_B = 0,   (G_u, G_th) = tip_force(record; 0, 0, g_F, 0)  -> G[b][6],
//     scattered to the two ends by k_stress_gather: end B receives (G_u, G_th), end A (-G_u, -G_th - d x G_u);
//     dB/dr_b at fixed u and segment geometry = g_F . dF/dr (record derivative, dscalars_dr) + w dbeta/dr|_P,
//     dbeta/dr|_P = -4 beta / r (Euler),  -beta (4 - 2 q / (1 + q)) / r (Engesser: N_E ~ r^4, q ~ r^2).
//
// Both reductions run in the two fixed-order stages of the stress pass (stress_block_fold, k_stress_fold), the nodal
// accumulation is its per-node gather: no floating-point atomics anywhere, so equal inputs give equal bits.
#pragma once
#include "pl_stress.h"

namespace pl {

// Critical load of a strut of radius r and buckling length l; q = N_E / (kappa G S) with shear, else 0.
__device__ __forceinline__ double buckling_ncr(double r, double l, double k_eff, int shear, const Material &m, double &q) {
  const double PI = 3.14159265358979323846;
  const double r2 = r * r, kl = k_eff * l;
  const double NE = PI * PI * m.E * (0.25 * PI * r2 * r2) / (kl * kl);
  q = shear ? NE / (m.kappa * m.G * (PI * r2)) : 0.0;
  return NE / (1.0 + q);
}

// ---------------------------------------------------------------------------------------------------------
// Utilisation pass: one thread per strut, no scatter.  util[b] = beta, n_axial[b] = N of one copy (signed), n_crit[b] =
// N_cr (all three NaN on an absent strut), part_max[block] = block maximum of beta.  Any output may be null.
// ---------------------------------------------------------------------------------------------------------
template <bool TH>
__global__ __launch_bounds__(kBlock) void k_buckling_util(int64_t B, const int32_t *__restrict__ conn,
                                                          const Record *__restrict__ rec,
                                                          const double *__restrict__ radius,
                                                          const double *__restrict__ seg_len,
                                                          const double *__restrict__ mult, Material mat, int length,
                                                          double k_eff, int shear, const double *__restrict__ u,
                                                          double *__restrict__ util, double *__restrict__ n_axial,
                                                          double *__restrict__ n_crit, double *__restrict__ part_max,
                                                          const double *__restrict__ delta) {
  __shared__ double smem[kBlock];
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double pk = 0.0;
  if (b < B) {
    const StressStrut s = load_strut<TH>(b, conn, rec, mult, u, delta).q;
    const double l2 = seg_len[3 * b + 1];
    const bool on = length == 0 || l2 > 0.0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double q;
    const double ncr = buckling_ncr(radius[b], length == 0 ? s.L : l2, k_eff, shear, mat, q);
    const double beta = s.N < 0.0 ? -s.N / ncr : 0.0;
    if (on) pk = beta;
    if (util) util[b] = on ? beta : nan;
    if (n_axial) n_axial[b] = on ? s.N : nan;
    if (n_crit) n_crit[b] = on ? ncr : nan;
  }
  if (part_max) {
    const double m = stress_block_fold<true>(pk, smem);
    if (threadIdx.x == 0) part_max[blockIdx.x] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Derivatives of B_p, one thread per strut, no scatter (header comment): G[b][6] and, with DR, dbp_dr[b].
// red = (beta_max, sum (beta / beta_max)^p, B_p) of k_stress_fold.
// ---------------------------------------------------------------------------------------------------------
template <bool DR, bool TH>
__global__ __launch_bounds__(kBlock) void k_buckling_grad(int64_t B, const int32_t *__restrict__ conn,
                                                          const Record *__restrict__ rec,
                                                          const double *__restrict__ radius,
                                                          const double *__restrict__ seg_len,
                                                          const int32_t *__restrict__ seg_nsub,
                                                          const double *__restrict__ mult, Material mat, int length,
                                                          double k_eff, int shear, double p,
                                                          const double *__restrict__ u, const double *__restrict__ red,
                                                          double *__restrict__ G, double *__restrict__ dbp_dr,
                                                          const double *__restrict__ delta) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double bmax = red[0], bsum = red[1];
  const StrutState st = load_strut<TH>(b, conn, rec, mult, u, delta);
  const StressStrut &s = st.q;
  const double len[3] = {seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2]};
  const bool on = length == 0 || len[1] > 0.0;
  const double rr = radius[b];
  double q;
  const double ncr = buckling_ncr(rr, length == 0 ? s.L : len[1], k_eff, shear, mat, q);
  const bool live = on && s.N < 0.0 && bmax > 0.0;
  const double beta = live ? -s.N / ncr : 0.0;
  const double w = live ? pow(beta / bmax, p - 1.0) * pow(bsum, 1.0 / p - 1.0) : 0.0;
  const V3 gF = (live ? -w * s.invk / ncr : 0.0) * s.t;
  V3 dF, dM;
  grad_epilogue<DR, TH>(st, b, rr, len, seg_nsub, mat, gF, V3{0, 0, 0}, G, dF, dM);
  if (DR) dbp_dr[b] = live ? dot(gF, dF) - w * beta * (4.0 - 2.0 * q / (1.0 + q)) / rr : 0.0;
}

}  // namespace pl
