// Strut section forces, peak von Mises stress and its p-norm aggregate with derivatives (pl_stress / pl_stress_pnorm;
// DESIGN.md section 12).  gfx950 only.
//
// A strut carries no span load: with (F, M_B) = tip_force(record, u) the section force is F everywhere and the moment
// about the point at arclength s (from end A) is M(s) = M_B + (L - s) t x F, t = d / L (the fact k_node_mod uses).  So
//     N = F.t,  V = |F - N t|,  T = M_B.t         are constant along the strut, and
//     Mb(s) = |M(s) - T t| = |P M_B + (L - s) t x F|,  P = I - t t^T
// is the norm of a linear function of s: over a segment it peaks at one of the segment's ends.  The stations are therefore
// the strut's ends and the junctions of its segments, [A, q1, q2, B]:
//     where = 0   A: s = 0, radius of the first present segment;  q1: s = l1 (present when the penalised segment at A and
//                 a segment behind it exist);  q2: s = l1 + l2 (middle and penalised segment at B exist);  B: s = L, radius
//                 of the last present segment.  A junction takes the smaller of its two segments' radii.
//     where = 1   slots 1 and 2 = the two ends of the middle segment (s = l1 and s = l1 + l2), radius r; slots 0 and 3 absent;
//                 a strut without a middle segment has no station.
// Stress of a circular section of radius R (S = pi R^2, I = pi R^4 / 4, J = 2 I):
//     sigma = |N| / S + Mb R / I,   tau = |T| R / J,   sigma_vm = sqrt(sigma^2 + 3 tau^2).
// A record of multiplicity k (pl_set_multiplicity) stands for k parallel copies: every copy carries F / k, M / k; all
// values are those of ONE copy and a copy counts once in the aggregate.
//
// Aggregate Phi_p = (sum over present stations of sigma_vm^p)^(1/p), evaluated as sigma_max (sum (sigma_vm / sigma_max)^p)^(1/p).
// Both reductions run in two stages with a fixed order (one partial per block in block order, then one block that walks the
// partials in a fixed stride and folds them in a fixed LDS tree), the nodal accumulation of dPhi/du is a per-node gather over
// the sliced-ELL incidence in its stored order: no floating-point atomics anywhere, so equal inputs give equal bits.
#pragma once
#include "pl_kernels.h"

namespace pl {

// Fold over the block in a fixed tree (LDS), result in every thread.  MAX: maximum, else sum.
template <bool MAX>
__device__ __forceinline__ double stress_block_fold(double v, double *smem /*[kBlock]*/) {
  smem[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double a = smem[threadIdx.x], b = smem[threadIdx.x + o];
      smem[threadIdx.x] = MAX ? fmax(a, b) : a + b;
    }
    __syncthreads();
  }
  const double r = smem[0];
  __syncthreads();
  return r;
}

// What every station of one strut shares.
struct StressStrut {
  V3 t, Mp, tF;        // unit tangent, P M_B, t x F  (F, M_B of the whole record)
  double L, invk;      // length, 1 / multiplicity
  double N, V, T;      // of one copy
};

// Station i of [A, q1, q2, B]: lever arm c = L - s, radius factor (R = fac r), presence.
struct StressStations {
  double c[4], fac[4];
  bool on[4];
};

__device__ __forceinline__ StressStations stress_stations(double l1, double l2, double l3, double L, double pen, int where) {
  StressStations s;
  const bool h1 = l1 > 0.0, h2 = l2 > 0.0, h3 = l3 > 0.0;
  const double thin = fmin(pen, 1.0);
  s.c[0] = L; s.c[1] = L - l1; s.c[2] = L - (l1 + l2); s.c[3] = 0.0;
  if (where == 1) {
    s.on[0] = false; s.on[1] = h2; s.on[2] = h2; s.on[3] = false;
    s.fac[0] = s.fac[1] = s.fac[2] = s.fac[3] = 1.0;
  } else {
    s.on[0] = true;
    s.on[1] = h1 && (h2 || h3);
    s.on[2] = h2 && h3;
    s.on[3] = true;
    s.fac[0] = h1 ? pen : (h2 ? 1.0 : pen);
    s.fac[1] = h2 ? thin : pen;
    s.fac[2] = thin;
    s.fac[3] = h3 ? pen : (h2 ? 1.0 : pen);
  }
  return s;
}

__device__ __forceinline__ StressStrut stress_strut(const Record &r, double k, V3 F, V3 M) {
  StressStrut q;
  const V3 d = {r.dx, r.dy, r.dz};
  q.L = sqrt(dot(d, d));
  q.t = (1.0 / q.L) * d;
  q.invk = 1.0 / k;
  const double Ft = dot(F, q.t), Mt = dot(M, q.t);
  const V3 Fp = F - Ft * q.t;
  q.Mp = M - Mt * q.t;
  q.tF = cross(q.t, F);
  q.N = Ft * q.invk;
  q.V = sqrt(dot(Fp, Fp)) * q.invk;
  q.T = Mt * q.invk;
  return q;
}

// Strut b under the field u: record, end vectors, (F, M_B) = tip_force(record, u), multiplicity k, and what its stations share.
struct StrutState {
  Record r;
  V3 uA, tA, uB, tB, F, M;
  double k;
  double fth;          // TH only: restrained thermal force ka delta of the record (pl_thermal.h)
  StressStrut q;
};

// TH: the handle has a thermal state (pl_set_thermal) and delta[b] is the strut's free elongation; F becomes the MECHANICAL
// section force K_tip (du, dth) - ka delta t.  Without TH delta is not read and the arithmetic is that of the plain pass.
template <bool TH>
__device__ __forceinline__ StrutState load_strut(int64_t b, const int32_t *__restrict__ conn, const Record *__restrict__ rec,
                                                 const double *__restrict__ mult, const double *__restrict__ u,
                                                 const double *__restrict__ delta) {
  StrutState s;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  s.r = load_record(rec, b);
  load6(u + 6 * ia, s.uA, s.tA);
  load6(u + 6 * ib, s.uB, s.tB);
  tip_force(s.r, s.uA, s.tA, s.uB, s.tB, s.F, s.M);
  if (TH) {
    const V3 d = {s.r.dx, s.r.dy, s.r.dz};
    const double L2 = dot(d, d);
    s.fth = (s.r.a + s.r.e1 * L2) * delta[b];
    s.F = s.F - (s.fth / sqrt(L2)) * d;
  }
  s.k = mult ? mult[b] : 1.0;
  s.q = stress_strut(s.r, s.k, s.F, s.M);
  return s;
}

// Close of a p-norm grad kernel (k_stress_grad, k_buckling_grad): G[b][6] = K_tip (g_F, g_M), the tip block applied to the
// aggregate's derivative with respect to (F, M_B).  With DR also (dF, dM) = d(F, M_B)/dr at fixed u and segment geometry, so
// that the caller's d/dr = g_F.dF + g_M.dM + its own section term; with TH the thermal shift of F is part of dF.
template <bool DR, bool TH>
__device__ __forceinline__ void grad_epilogue(const StrutState &s, int64_t b, double rr, const double *len,
                                              const int32_t *__restrict__ seg_nsub, const Material &mat, V3 gF, V3 gM,
                                              double *__restrict__ G, V3 &dF, V3 &dM) {
  const V3 zero = {0, 0, 0};
  V3 Gu, Gth;
  tip_force(s.r, zero, zero, gF, gM, Gu, Gth);
  store6(G + 6 * b, Gu, Gth);
  if (DR) {
    const int ns[3] = {seg_nsub[3 * b], seg_nsub[3 * b + 1], seg_nsub[3 * b + 2]};
    const V3 d = {s.r.dx, s.r.dy, s.r.dz};
    const Record dr = strut_drecord(rr, len, ns, scaled(mat, s.k), d);
    tip_force(dr, s.uA, s.tA, s.uB, s.tB, dF, dM);
    if (TH) dF = dF - (2.0 * s.fth / rr / sqrt(dot(d, d))) * d;   // d(ka delta t)/dr = (2 ka / r) delta t
  }
}

// Section constants of radius R: 1 / S, R / I, R / J.
__device__ __forceinline__ void stress_section(double R, double &iS, double &RI, double &RJ) {
  const double PI = 3.14159265358979323846;
  const double R2 = R * R;
  iS = 1.0 / (PI * R2);
  RI = 4.0 / (PI * R2 * R);
  RJ = 0.5 * RI;
}

// ---------------------------------------------------------------------------------------------------------
// Station pass: one thread per strut, no scatter.  station[b][4][5] = N, V, T, Mb, sigma_vm (NaN where absent), peak[b] =
// max sigma_vm (0 without a station), vm4[b][4] = sigma_vm per station (NaN where absent), part_max[block] = block maximum.
// Any output may be null.  TH: the mechanical force under the handle's thermal state (load_strut).
// ---------------------------------------------------------------------------------------------------------
template <bool TH>
__global__ __launch_bounds__(kBlock) void k_stress_stations(int64_t B, const int32_t *__restrict__ conn,
                                                            const Record *__restrict__ rec,
                                                            const double *__restrict__ radius,
                                                            const double *__restrict__ seg_len,
                                                            const double *__restrict__ mult, double pen, int where,
                                                            const double *__restrict__ u, double *__restrict__ station,
                                                            double *__restrict__ peak, double *__restrict__ vm4,
                                                            double *__restrict__ part_max,
                                                            const double *__restrict__ delta) {
  __shared__ double smem[kBlock];
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double pk = 0.0;
  if (b < B) {
    const StressStrut q = load_strut<TH>(b, conn, rec, mult, u, delta).q;
    const StressStations s = stress_stations(seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2], q.L, pen, where);
    const double rr = radius[b];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double vm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const V3 m = q.Mp + s.c[i] * q.tF;
      const double Mb = sqrt(dot(m, m)) * q.invk;
      double iS, RI, RJ;
      stress_section(s.fac[i] * rr, iS, RI, RJ);
      const double sg = fabs(q.N) * iS + Mb * RI, ta = fabs(q.T) * RJ;
      const double v = sqrt(sg * sg + 3.0 * ta * ta);
      vm[i] = s.on[i] ? v : nan;
      if (s.on[i]) pk = fmax(pk, v);
      if (station) {
        double *o = station + 20 * b + 5 * i;
        o[0] = s.on[i] ? q.N : nan;
        o[1] = s.on[i] ? q.V : nan;
        o[2] = s.on[i] ? q.T : nan;
        o[3] = s.on[i] ? Mb : nan;
        o[4] = vm[i];
      }
    }
    if (peak) peak[b] = pk;
    if (vm4) {
      double2 *o = reinterpret_cast<double2 *>(vm4 + 4 * b);
      o[0] = {vm[0], vm[1]};
      o[1] = {vm[2], vm[3]};
    }
  }
  if (part_max) {
    const double m = stress_block_fold<true>(pk, smem);
    if (threadIdx.x == 0) part_max[blockIdx.x] = m;
  }
}

// Second stage of both reductions: ONE block walks the n partials in a fixed stride and folds them in the fixed tree.
// MAX: red[0] = sigma_max.  Otherwise: red[1] = sum (sigma_vm / sigma_max)^p, red[2] = Phi_p (0 when sigma_max = 0).
template <bool MAX>
__global__ __launch_bounds__(kBlock) void k_stress_fold(int64_t n, const double *__restrict__ part, double p,
                                                        double *__restrict__ red) {
  __shared__ double smem[kBlock];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) v = MAX ? fmax(v, part[i]) : v + part[i];
  v = stress_block_fold<MAX>(v, smem);
  if (threadIdx.x == 0) {
    if (MAX) {
      red[0] = v;
    } else {
      red[1] = v;
      red[2] = red[0] > 0.0 ? red[0] * pow(v, 1.0 / p) : 0.0;
    }
  }
}

// First stage of the p-sum: per strut the sum over its W values (stress: 4 stations, buckling: 1 utilisation) of
// (v / v_max)^p, one partial per block; red[0] = v_max.  NaN marks an absent value, and like a zero it adds nothing.
// RECIP: the ratio is formed as v * (1 / v_max) (the stress pass), else as v / v_max (the buckling pass) - each as its grad
// kernel forms it.
template <int W, bool RECIP>
__global__ __launch_bounds__(kBlock) void k_pnorm_psum(int64_t B, const double *__restrict__ val /*[B][W]*/,
                                                       const double *__restrict__ red, double p,
                                                       double *__restrict__ part_sum) {
  __shared__ double smem[kBlock];
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double vmax = red[0];
  double acc = 0.0;
  if (b < B && vmax > 0.0) {
    double v[W];
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = val[W * b + i];
    const double inv = 1.0 / vmax;
#pragma unroll
    for (int i = 0; i < W; ++i)
      if (v[i] > 0.0) acc += pow(RECIP ? v[i] * inv : v[i] / vmax, p);
  }
  const double t = stress_block_fold<false>(acc, smem);
  if (threadIdx.x == 0) part_sum[blockIdx.x] = t;
}

// ---------------------------------------------------------------------------------------------------------
// Derivatives of Phi_p, one thread per strut, no scatter.  With w_i = dPhi / d sigma_vm,i = (sigma_vm,i / sigma_max)^(p-1)
// (sum (sigma_vm / sigma_max)^p)^(1/p - 1):
//   g_F = dPhi/dF = sum_i w_i [ (sigma/sigma_vm) (sgn N / S) t + (sigma/sigma_vm) (R/I) (L - s_i) (m_i x t) ] / k
//   g_M = dPhi/dM_B = sum_i w_i [ (sigma/sigma_vm) (R/I) m_i + 3 (tau/sigma_vm) (R/J) sgn T t ] / k,   m_i = unit vector of P M(s_i)
// (F, M_B) = K_tip (du, dth) with the symmetric tip block, so dPhi/d(du, dth) = K_tip (g_F, g_M) = tip_force(record; g_F, g_M at
// the tip) =: (G_u, G_th), written to G[b][6]: end B receives (G_u, G_th), end A (-G_u, -G_th - d x G_u) (k_stress_gather).
// dphi_dr[b] at fixed u and segment geometry = g_F.dF/dr + g_M.dM_B/dr with the record's derivative (dscalars_dr) plus the
// section constants' own dependence on R = fac r:  d sigma/dr = -(2 |N|/S + 3 Mb R/I) / r,  d tau/dr = -3 tau / r.
// Derivatives of |N|, |T|, Mb at exactly zero are taken as zero.
// ---------------------------------------------------------------------------------------------------------
template <bool DR, bool TH>
__global__ __launch_bounds__(kBlock) void k_stress_grad(int64_t B, const int32_t *__restrict__ conn,
                                                        const Record *__restrict__ rec,
                                                        const double *__restrict__ radius,
                                                        const double *__restrict__ seg_len,
                                                        const int32_t *__restrict__ seg_nsub,
                                                        const double *__restrict__ mult, Material mat, int where, double p,
                                                        const double *__restrict__ u, const double *__restrict__ red,
                                                        double *__restrict__ G, double *__restrict__ dphi_dr,
                                                        const double *__restrict__ delta) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double smax = red[0], ssum = red[1];
  const StrutState st = load_strut<TH>(b, conn, rec, mult, u, delta);
  const StressStrut &q = st.q;
  const double len[3] = {seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2]};
  const StressStations s = stress_stations(len[0], len[1], len[2], q.L, mat.pen, where);
  const double rr = radius[b];
  const double outer = smax > 0.0 ? pow(ssum, 1.0 / p - 1.0) : 0.0, inv = smax > 0.0 ? 1.0 / smax : 0.0;
  const double sN = q.N > 0.0 ? 1.0 : (q.N < 0.0 ? -1.0 : 0.0), sT = q.T > 0.0 ? 1.0 : (q.T < 0.0 ? -1.0 : 0.0);
  V3 gF = {0, 0, 0}, gM = {0, 0, 0};
  double dsec = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const V3 m = q.Mp + s.c[i] * q.tF;
    const double mn = sqrt(dot(m, m));
    const double Mb = mn * q.invk;
    double iS, RI, RJ;
    stress_section(s.fac[i] * rr, iS, RI, RJ);
    const double sgN = fabs(q.N) * iS, sgB = Mb * RI, sg = sgN + sgB, ta = fabs(q.T) * RJ;
    const double v = sqrt(sg * sg + 3.0 * ta * ta);
    if (s.on[i] && v > 0.0) {
      const double w = pow(v * inv, p - 1.0) * outer;
      const double ws = w * sg / v, wt = w * 3.0 * ta / v;      // dPhi/d sigma, dPhi/d tau of this station
      const V3 mh = mn > 0.0 ? (1.0 / mn) * m : V3{0, 0, 0};
      gF = gF + (ws * sN * iS * q.invk) * q.t + (ws * RI * s.c[i] * q.invk) * cross(mh, q.t);
      gM = gM + (ws * RI * q.invk) * mh + (wt * RJ * sT * q.invk) * q.t;
      dsec -= (ws * (2.0 * sgN + 3.0 * sgB) + wt * 3.0 * ta) / rr;
    }
  }
  V3 dF, dM;
  grad_epilogue<DR, TH>(st, b, rr, len, seg_nsub, mat, gF, gM, G, dF, dM);
  if (DR) dphi_dr[b] = dot(gF, dF) + dot(gM, dM) + dsec;
}

// dPhi/du by a per-node gather over the sliced-ELL incidence of k_spmv_gather (SN = 64 / lanes-per-node nodes per slice,
// ent[slice_ptr[s] + j SN + n] = j-th strut of node s SN + n as (other node, strut | end << 31), other < 0 = padding): one
// thread per node, its struts in their stored order.  The node is the strut's tip (end B) unless bit 31 is set.
__global__ __launch_bounds__(kBlock) void k_stress_gather(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                          const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                          const double *__restrict__ G, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  V3 au = {0, 0, 0}, at = {0, 0, 0};
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x < 0) continue;
    const int64_t b = e.y & 0x7fffffff;
    V3 gu, gt;
    load6(G + 6 * b, gu, gt);
    if (e.y < 0) {   // this node is the strut's point1
      const double2 *q = reinterpret_cast<const double2 *>(rec + b);
      const double2 c = q[2], dd = q[3];
      const V3 d = {c.y, dd.x, dd.y};
      au = au - gu;
      at = at - gt - cross(d, gu);
    } else {
      au = au + gu;
      at = at + gt;
    }
  }
  store6(out + 6 * i, au, at);
}

}  // namespace pl
