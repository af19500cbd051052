// Thermal loads of the struts: free elongation, equivalent nodal loads and their radius derivative (pl_set_thermal /
// pl_thermal_load / pl_thermal_sens).  gfx950 only.
//
// Strut b joins A = conn[2b] and B = conn[2b+1], d = x_B - x_A, L = |d|, t = d / L.  The temperature rise is linear along
// the strut between the nodal values and uniform over the section (no thermal curvature):
//     delta_b = alpha_b L (dT_A + dT_B) / 2          free elongation; no radius, no penalised segment enters
//     F_th,b  = ka_b delta_b,  ka_b = rec.a + rec.e1 L^2   restrained force of the record (multiplicity k included),
//     n_free_b = F_th,b / k                                that of ONE copy
//     f_th: +F_th t on the translations of B, -F_th t on those of A, no moments;  K u = f_ext + f_th.
// The mechanical section force is F = K_tip (du, dth) - F_th t (load_strut<true> in pl_stress.h): only N shifts.
// d ka / dr = 2 ka / r at fixed segment geometry (dscalars_dr), so for any field lam
//     lam^T d f_th / d r_b = (2 ka_b / r_b) delta_b t . (lam_u,B - lam_u,A).
//
// k_thermal_load is a per-node gather over the sliced-ELL incidence in its stored order (the lane mapping of
// k_stress_gather): no floating-point atomics, no [B][6] intermediate, equal inputs give equal bits.
#pragma once
#include "pl_context.h"
#include "pl_stress.h"

namespace pl {

// One thread per strut: delta[b] and, if asked for, n_free[b] (of one copy).
__global__ __launch_bounds__(kBlock) void k_thermal_strut(int64_t B, const int32_t *__restrict__ conn,
                                                          const Record *__restrict__ rec,
                                                          const double *__restrict__ mult,
                                                          const double *__restrict__ alpha,
                                                          const double *__restrict__ dT, double *__restrict__ delta,
                                                          double *__restrict__ n_free) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const Record r = load_record(rec, b);
  const double L2 = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
  const double dl = alpha[b] * sqrt(L2) * (0.5 * (dT[ia] + dT[ib]));
  delta[b] = dl;
  if (n_free) n_free[b] = (r.a + r.e1 * L2) * dl / (mult ? mult[b] : 1.0);
}

// One thread per node, its struts in their stored order: out[i][0..2] = sum of +-ka delta t, out[i][3..5] = 0.  The node is
// the strut's end B unless bit 31 of the entry is set.
__global__ __launch_bounds__(kBlock) void k_thermal_load(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                         const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                         const double *__restrict__ delta, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  V3 au = {0, 0, 0};
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x < 0) continue;
    const int64_t b = e.y & 0x7fffffff;
    const double2 *q = reinterpret_cast<const double2 *>(rec + b);
    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const V3 d = {q2.y, q3.x, q3.y};
    const double L2 = dot(d, d);
    const V3 f = ((q0.x + q1.x * L2) * delta[b] / sqrt(L2)) * d;
    au = e.y < 0 ? au - f : au + f;
  }
  store6(out + 6 * i, au, V3{0, 0, 0});
}

// One thread per strut, no scatter: out[b] = (2 ka / r) delta t . (lam_u,B - lam_u,A).
__global__ __launch_bounds__(kBlock) void k_thermal_sens(int64_t B, const int32_t *__restrict__ conn,
                                                         const Record *__restrict__ rec,
                                                         const double *__restrict__ radius,
                                                         const double *__restrict__ delta,
                                                         const double *__restrict__ lam, double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const Record r = load_record(rec, b);
  V3 lA, mA, lB, mB;
  load6(lam + 6 * ia, lA, mA);
  load6(lam + 6 * ib, lB, mB);
  const V3 d = {r.dx, r.dy, r.dz};
  const double L2 = dot(d, d);
  out[b] = (2.0 * (r.a + r.e1 * L2) / radius[b]) * delta[b] * (dot(d, lB - lA) / sqrt(L2));
}

}  // namespace pl

namespace {

// Thermal state of the handle (pl_context::thermal_ws), set by pl_set_thermal, device numbering: alpha[B], dT[N]; delta[B] is
// rebuilt from the current records by every call that reads it, n_free[B] and out[B] hold the per-strut outputs.
struct ThermalWs {
  DevBuf<double> alpha, dT, delta, n_free, out;
};

}  // namespace
