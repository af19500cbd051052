// Transient heat conduction on the strut graph: a lumped heat capacity and implicit one-step theta stepping on the device
// (pl_set_heat_capacity / pl_cond_transient).  gfx950 only, fp64, wave 64.  Conventions of pl_conduction.h.
//
//     C_i = sum over struts b at i of cap_b + node_capacity_i,   cap_b = (1/2) k_b (rho c)_b pi r_b^2 L_b
//     C dT/dt + (K_T + H) T = q(t) + H T_inf on the free nodes, T = T_bar(t) on the masked ones (H = 0 without convection)
// One step in increment form, dT = T_{n+1} - T_n, 1/2 <= theta <= 1:
//     (C/dt + theta (K_T + H)) dT = q_theta + H T_inf - (K_T + H) W on the free rows
//     W_j = T_n,j on a free node, (1 - theta) T_n,j + theta T_bar,n+1,j on a fixed one;  q_theta = theta q_{n+1} + (1 - theta) q_n
// The capacity terms cancel on the right-hand side: a field at rest gives b = 0 and k_multi_begin freezes the column with dT = 0.
// The prescribed temperature of row n on a fixed node is T0_i + s_n (T_bar_i - T0_i) (heat_row_value, not contracted into an fma,
// so that a host restatement gives the same bits).
// Heat balance, increments per row summed over 64 slots: U = sum C (T - T_inf); dQ_in = dt sum_free q_theta;
//     dQ_c = dt sum_all H (T_theta - T_inf);  dQ_R = dt sum_fixed [C dT/dt + ((K_T + H) T_theta)_i - H_i T_inf],  T_theta = T_n + theta dT.
//
// Per step: k_heat_begin (lifting gather + PCG init), k_multi_begin, per iteration k_heat_gather + k_multi_update<1> +
// k_multi_direction<1>, then k_heat_end (new temperatures, probes, snapshot, balance).  All per-node walks go over the sliced-ELL
// incidence in its stored order with the lane mapping of k_cond_gather: no floating-point atomics outside the slot sums.
#pragma once
#include "pl_conduction.h"

namespace pl {

enum { HEAT_U = 0, HEAT_QIN = 1, HEAT_QC = 2, HEAT_QR = 3, HEAT_COUNT = 4 };
constexpr int kHeatMaxPat = 4;

// What the step kernels share: the scheme, the two boundary arrays, the loads.  amp: [rows][n_pat], bar_amp: [rows] or null (s = 1).
struct HeatStep {
  double dt, theta, T_inf;
  int n_pat;
  const uint8_t *fixed;      // [N]
  const double *T0, *Tbar;   // [N]: the start field and the prescribed end values
  const double *bar_amp;     // [rows] or null
  const double *pattern;     // [n_pat][N]
  const double *amp;         // [rows][n_pat]
};

__device__ __forceinline__ double heat_row_value(double t0, double tb, double s) {
#pragma clang fp contract(off)
  const double d = tb - t0;
  const double sd = s * d;
  return t0 + sd;
}
// the prescribed temperature of a fixed node in row `row`
__device__ __forceinline__ double heat_bar(const HeatStep &q, int row, int64_t i) {
  return heat_row_value(q.T0[i], q.Tbar[i], q.bar_amp ? q.bar_amp[row] : 1.0);
}
// q_theta of the step that ends in row `row` at node i
__device__ __forceinline__ double heat_load(const HeatStep &q, int row, int64_t N, int64_t i) {
  double v = 0.0;
  for (int p = 0; p < q.n_pat; ++p) {
    const double a = q.theta * q.amp[(size_t)row * q.n_pat + p] + (1.0 - q.theta) * q.amp[(size_t)(row - 1) * q.n_pat + p];
    v += a * q.pattern[(size_t)p * N + i];
  }
  return v;
}

// One thread per strut, the pass of k_cond_strut with the half capacity: g[b], CONV: c[b], and cap[b] = (1/2) k rho_c pi r^2 L.
template <bool CONV>
__global__ __launch_bounds__(kBlock) void k_heat_strut(int64_t B, const Record *__restrict__ rec, const double *__restrict__ radius,
                                                       const double *__restrict__ mult, const double *__restrict__ kappa,
                                                       double *__restrict__ g, const double *__restrict__ film,
                                                       double *__restrict__ c, const double *__restrict__ rho_c,
                                                       double *__restrict__ cap) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double L2 = strut_length2(rec, b);
  const double r = radius[b];
  g[b] = strut_conductance(mult, kappa, b, r, L2);       // (the expressions of k_cond_strut: the same bits)
  if (CONV) c[b] = strut_film(mult, film, b, r, L2);
  cap[b] = 0.5 * (mult ? mult[b] : 1.0) * rho_c[b] * (3.14159265358979323846 * r * r) * sqrt(L2);
}

// One thread per node, ONE walk over its struts in their stored order: C_i = sum cap_b + node_cap_i, CONV: H_i = sum c_b,
// the step diagonal S_i = C_i / dt + theta H_i and dinv_i = 1 / (S_i + theta sum g_b) on a free node, 0 on a fixed one.
template <bool CONV>
__global__ __launch_bounds__(kBlock) void k_heat_diag(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                      const int2 *__restrict__ ent, const double *__restrict__ g,
                                                      const double *__restrict__ c, const double *__restrict__ cap,
                                                      const double *__restrict__ node_cap, const uint8_t *__restrict__ fixed,
                                                      double dt, double theta, double *__restrict__ H, double *__restrict__ C,
                                                      double *__restrict__ S, double *__restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t s = i / SN, n = i - s * SN;
  const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
  double gs = 0.0, hs = 0.0, cs = 0.0;
  for (int64_t j = 0; j < width; ++j) {
    const int2 e = ent[p0 + j * SN + n];
    if (e.x < 0) continue;
    const int64_t b = e.y & 0x7fffffff;
    gs += g[b];
    cs += cap[b];
    if (CONV) hs += c[b];
  }
  cs += node_cap[i];
  const double sd = cs / dt + theta * hs, dg = sd + theta * gs;
  if (CONV) H[i] = hs;
  C[i] = cs;
  S[i] = sd;
  dinv[i] = (fixed[i] || !(dg > 0.0)) ? 0.0 : 1.0 / dg;
}

// Row 0, one thread per node: T_0 = T0 with the fixed nodes at their row-0 value, its probes, and U_0 into the slots of row 0.
__global__ __launch_bounds__(kBlock) void k_heat_start(int64_t N, HeatStep q, const double *__restrict__ C,
                                                       double *__restrict__ T, const int32_t *__restrict__ probe_slot,
                                                       int n_slot, double *__restrict__ probe, double *__restrict__ heat) {
  __shared__ double red[1][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[1] = {0.0};
  if (i < N) {
    const double t = q.fixed[i] ? heat_bar(q, 0, i) : q.T0[i];
    T[i] = t;
    const int slot = probe_slot[i];
    if (slot >= 0) probe[slot] = t;
    acc[0] = C[i] * (t - q.T_inf);
  }
  double *dst[1] = {heat + (size_t)HEAT_U * kSlots};
  block_add_slots<1>(acc, red, dst);
}

// The lifting gather and the PCG init of the step that ends in row `row`, one thread per node:
//   r_i = q_theta,i + H_i (T_inf - T_n,i) - sum g_b (T_n,i - W_other) on a free node, 0 on a fixed one (W formed on the fly),
//   z = dinv r ; p = z ; x = 0 ; rz_old += r.z ; bb += r.r
template <bool CONV>
__global__ __launch_bounds__(kBlock) void k_heat_begin(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                       const int2 *__restrict__ ent, const double *__restrict__ g,
                                                       const double *__restrict__ H, HeatStep q, int row,
                                                       const double *__restrict__ Tn, const double *__restrict__ dinv,
                                                       double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                       double *__restrict__ p, double *__restrict__ set0,
                                                       double *__restrict__ bb) {
  __shared__ double red[2][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (i < N) {
    double rv = 0.0;
    if (!q.fixed[i]) {
      const int64_t s = i / SN, n = i - s * SN;
      const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
      const double ts = Tn[i];
      double flow = 0.0;
      for (int64_t j = 0; j < width; ++j) {
        const int2 e = ent[p0 + j * SN + n];
        if (e.x < 0) continue;
        double wo = Tn[e.x];
        if (q.fixed[e.x]) wo = (1.0 - q.theta) * wo + q.theta * heat_bar(q, row, e.x);
        flow += g[e.y & 0x7fffffff] * (ts - wo);
      }
      rv = heat_load(q, row, N, i) - flow;
      if (CONV) rv += H[i] * (q.T_inf - ts);
    }
    const double zv = dinv[i] * rv;
    x[i] = 0.0;
    r[i] = rv;
    z[i] = zv;
    p[i] = zv;
    acc[0] = rv * zv;
    acc[1] = rv * rv;
  }
  double *dst[2] = {slots_of(set0, M_RZ_OLD, 1, 0), bb};
  block_add_slots<2>(acc, red, dst);
}

// The operator of the iteration, the lane mapping and stored order of k_cond_gather: y_i = theta sum g_b (x_i - x_other) + S_i x_i,
// 0 on a fixed node (x is 0 there), and x . y into the 64 slots of dot_out.
__global__ __launch_bounds__(kBlock) void k_heat_gather(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                        const int2 *__restrict__ ent, const double *__restrict__ g,
                                                        const double *__restrict__ S, const uint8_t *__restrict__ fixed,
                                                        double theta, const double *__restrict__ x, double *__restrict__ y,
                                                        double *__restrict__ dot_out) {
  __shared__ double red[1][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[1] = {0.0};
  if (i < N) {
    const int64_t s = i / SN, n = i - s * SN;
    const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
    const double xs = x[i], sd = S[i];
    double out = 0.0;
    for (int64_t j = 0; j < width; ++j) {
      const int2 e = ent[p0 + j * SN + n];
      if (e.x < 0) continue;
      out += g[e.y & 0x7fffffff] * (xs - x[e.x]);
    }
    out = theta * out + sd * xs;
    if (fixed[i]) out = 0.0;
    y[i] = out;
    acc[0] = xs * out;
  }
  double *dst[1] = {dot_out};
  block_add_slots<1>(acc, red, dst);
}

// The end of the step that ends in row `row`, one thread per node: T_{n+1} = T_n + dT (a fixed node gets its row value), the
// probed nodes, the snapshot (snap != null), and the four balance terms of the row into the slots of heat [HEAT_COUNT][kSlots].
// Only a fixed node walks its struts, for (K_T T_theta)_i; the neighbours' increments are formed on the fly.
template <bool CONV>
__global__ __launch_bounds__(kBlock) void k_heat_end(int64_t N, int SN, const int64_t *__restrict__ slice_ptr,
                                                     const int2 *__restrict__ ent, const double *__restrict__ g,
                                                     const double *__restrict__ H, const double *__restrict__ C, HeatStep q,
                                                     int row, const double *__restrict__ Tn, const double *__restrict__ x,
                                                     double *__restrict__ Tnew, const int32_t *__restrict__ probe_slot,
                                                     double *__restrict__ probe_row, double *__restrict__ snap,
                                                     double *__restrict__ heat) {
  __shared__ double red[HEAT_COUNT][kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[HEAT_COUNT] = {0.0, 0.0, 0.0, 0.0};
  if (i < N) {
    const bool fx = q.fixed[i] != 0;
    const double ts = Tn[i];
    const double tn = fx ? heat_bar(q, row, i) : ts + x[i];
    const double d = fx ? tn - ts : x[i];
    const double tt = ts + q.theta * d;
    const double ci = C[i];
    double hi = 0.0;
    if (CONV) hi = H[i];
    Tnew[i] = tn;
    const int slot = probe_slot[i];
    if (slot >= 0) probe_row[slot] = tn;
    if (snap) snap[i] = tn;
    acc[HEAT_U] = ci * (tn - q.T_inf);
    acc[HEAT_QC] = q.dt * (hi * (tt - q.T_inf));
    if (fx) {
      const int64_t s = i / SN, n = i - s * SN;
      const int64_t p0 = slice_ptr[s], width = (slice_ptr[s + 1] - p0) / SN;
      double flow = 0.0;
      for (int64_t j = 0; j < width; ++j) {
        const int2 e = ent[p0 + j * SN + n];
        if (e.x < 0) continue;
        const double to = Tn[e.x];
        const double dd = q.fixed[e.x] ? heat_bar(q, row, e.x) - to : x[e.x];
        flow += g[e.y & 0x7fffffff] * (tt - (to + q.theta * dd));
      }
      acc[HEAT_QR] = ci * d + q.dt * (flow + hi * (tt - q.T_inf));
    } else {
      acc[HEAT_QIN] = q.dt * heat_load(q, row, N, i);
    }
  }
  double *dst[HEAT_COUNT];
#pragma unroll
  for (int v = 0; v < HEAT_COUNT; ++v) dst[v] = heat + (size_t)v * kSlots;
  block_add_slots<HEAT_COUNT>(acc, red, dst);
}

}  // namespace pl

namespace {

// Heat capacity of the handle and the device data of pl_cond_transient, owned by the conduction state (CondWs::heat): set by
// pl_set_heat_capacity, dropped with the conduction state.  The PCG vectors, the mask and the scalar block are the conduction
// state's own (every call that uses them writes them first).
struct HeatWs {
  DevBuf<double> rho_c, cap;             // [B]
  DevBuf<double> node_cap, C, S;         // [N]
  DevBuf<double> T2, T0, Tbar;           // the two temperature fields of the ping-pong [2][N], the start field, the end values
  DevBuf<double> pattern, amp, bar_amp;  // [n_pat][N], [rows][n_pat], [rows]
  DevBuf<int32_t> probe_slot;            // [N]: column of the node in the probe block, -1 = not probed
  DevBuf<double> probe, heat, snaps;     // [rows][n_slot], [rows][HEAT_COUNT][kSlots], [n_snap][N]; probe and snaps are
                                         // released after the download of every call, the rest stays at its largest size
};

template <typename T>
hipError_t heat_grow(DevBuf<T> &b, size_t n) {
  return b.n < n ? b.alloc(n) : hipSuccess;
}

}  // namespace
