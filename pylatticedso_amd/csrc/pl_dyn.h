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
// S x is ONE gather (k_dyn_gather_multi): the node -> strut walk of k_spmv_gather_multi / k_mass_gather_multi, the ELL entry
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

// ---------------------------------------------------------------------------------------------------------
// y_k = c_K K x_k + c_M M x_k (MASK: P (...), x_k assumed 0 on fixed dofs) for the KB columns of column block blockIdx.y.
// Lane mapping, sliced ELL, xcd_block, lpn_sum, masked store, thirds-of-a-row store and the dot_out slots are those of
// k_spmv_gather_multi.  Per entry: one ent[p], one load_row of the neighbour; the stiffness record is loaded, reversed, scaled
// and used up before the mass record is loaded, so only one of the two is live at a time.
// ---------------------------------------------------------------------------------------------------------
template <int LPN, int KB, bool MASK>
__global__ __launch_bounds__(kBlock) void k_dyn_gather_multi(int64_t N, const int64_t *__restrict__ slice_ptr,
                                                             const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                             const MassRecord *__restrict__ mrec, int rotary,
                                                             const double *__restrict__ node_mass, double c_K, double c_M,
                                                             const uint8_t *__restrict__ fixedbits,
                                                             const double *__restrict__ x, double *__restrict__ y,
                                                             double *__restrict__ dot_out, int64_t stride) {
  __shared__ double red[KB][kBlock / kWave];
  const unsigned blk = xcd_block(blockIdx.x, gridDim.x);
  const int cb = blockIdx.y;
  x += (size_t)cb * stride;
  y += (size_t)cb * stride;
  constexpr int kSliceNodes = kWave / LPN;
  const int lane = threadIdx.x & 63, sub = lane / kSliceNodes;
  const int64_t slice = (int64_t)blk * (kBlock / kWave) + (threadIdx.x >> 6);
  const int64_t i = slice * kSliceNodes + (lane & (kSliceNodes - 1));
  double acc[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) acc[k] = 0.0;
  if (slice * kSliceNodes < N) {          // wave-uniform
    const bool live = i < N;
    double xs[6 * KB], out[6 * KB];
#pragma unroll
    for (int q = 0; q < 6 * KB; ++q) { xs[q] = 0.0; out[q] = 0.0; }
    if (live) load_row<KB>(x, i, xs);
    const int64_t p0 = slice_ptr[slice], p1 = slice_ptr[slice + 1];
#pragma unroll 1
    for (int64_t p = p0 + lane; p < p1; p += 64) {
      const int2 e = ent[p];
      if (e.x >= 0) {
        const int64_t b = e.y & 0x7fffffff;
        double xo[6 * KB];
        load_row<KB>(x, (int64_t)e.x, xo);
        {
          Record r = load_record(rec, b);
          if (e.y < 0) r = reversed(r);   // this node is the strut's point1
          r = scaled_record(r, c_K);
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            V3 uo, to, us, ts, f, m;
            column_of<KB>(xo, k, uo, to);
            column_of<KB>(xs, k, us, ts);
            tip_force(r, uo, to, us, ts, f, m);
            out[0 * KB + k] += f.x; out[1 * KB + k] += f.y; out[2 * KB + k] += f.z;
            out[3 * KB + k] += m.x; out[4 * KB + k] += m.y; out[5 * KB + k] += m.z;
          }
        }
        {
          const MassRecord r = load_mass(mrec, b);
          MassCoef c = mass_coef(r, rotary);
          c = {c_M * c.m6, c_M * c.c, c_M * c.j, c_M * c.g};
          const double sg = e.y < 0 ? -1.0 : 1.0;                     // point1: d -> -d
          const V3 d = {sg * r.dx, sg * r.dy, sg * r.dz};
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            V3 uo, to, us, ts, f, m;
            column_of<KB>(xo, k, uo, to);
            column_of<KB>(xs, k, us, ts);
            mass_force(c, d, uo, to, us, ts, f, m);
            out[0 * KB + k] += f.x; out[1 * KB + k] += f.y; out[2 * KB + k] += f.z;
            out[3 * KB + k] += m.x; out[4 * KB + k] += m.y; out[5 * KB + k] += m.z;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 6 * KB; ++q) out[q] = lpn_sum<LPN>(out[q]);
    if (live) {
      if (node_mass) {                    // kernel-uniform; every lane of the node holds the whole row by now
        const double nm = c_M * node_mass[i];
#pragma unroll
        for (int q = 0; q < 3 * KB; ++q) out[q] += nm * xs[q];
      }
      if (MASK) {
        const unsigned fb = fixedbits[i];
#pragma unroll
        for (int d = 0; d < 6; ++d)
          if (fb & (1u << d)) {
#pragma unroll
            for (int k = 0; k < KB; ++k) out[d * KB + k] = 0.0;
          }
      }
      double2 *q = reinterpret_cast<double2 *>(y + 6 * KB * i);
      if (LPN >= 4) {   // lanes sub = 0, 1, 2 of a node store one third of its row each (2 dofs x KB columns, contiguous)
        if (sub == 0) {
#pragma unroll
          for (int j = 0; j < KB; ++j) q[j] = {out[2 * j], out[2 * j + 1]};
        } else if (sub == 1) {
#pragma unroll
          for (int j = KB; j < 2 * KB; ++j) q[j] = {out[2 * j], out[2 * j + 1]};
        } else if (sub == 2) {
#pragma unroll
          for (int j = 2 * KB; j < 3 * KB; ++j) q[j] = {out[2 * j], out[2 * j + 1]};
        }
      } else if (sub == 0) {
#pragma unroll
        for (int j = 0; j < 3 * KB; ++j) q[j] = {out[2 * j], out[2 * j + 1]};
      }
      if (dot_out && sub == 0) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
          acc[k] = xs[0 * KB + k] * out[0 * KB + k] + xs[1 * KB + k] * out[1 * KB + k] + xs[2 * KB + k] * out[2 * KB + k] +
                   xs[3 * KB + k] * out[3 * KB + k] + xs[4 * KB + k] * out[4 * KB + k] + xs[5 * KB + k] * out[5 * KB + k];
      }
    }
  }
  if (dot_out) {   // kernel-uniform
    double *dst[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) dst[k] = dot_out + (size_t)(cb * KB + k) * kSlots;
    block_add_slots<KB>(acc, red, dst);
  }
}

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
constexpr int kDynKB = 2;

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

template <int LPN, int KB>
void launch_dyn_multi_t(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x,
                        double *y, bool masked, double *dot_dev) {
  const dim3 grid(grid_for(c->n_slices, pl::kBlock / pl::kWave), (unsigned)s.ncb);   // one wave per ELL slice and column block
  const MassWs *m = op.mass;
  if (masked)
    hipLaunchKernelGGL((pl::k_dyn_gather_multi<LPN, KB, true>), grid, dim3(pl::kBlock), 0, c->stream, c->N, c->slice_ptr.p,
                       c->ent.p, (const pl::Record *)c->rec.p, (const pl::MassRecord *)m->rec.p, m->rotary, m->nm(), op.c_K,
                       op.c_M, fixedbits, x, y, dot_dev, s.stride);
  else
    hipLaunchKernelGGL((pl::k_dyn_gather_multi<LPN, KB, false>), grid, dim3(pl::kBlock), 0, c->stream, c->N, c->slice_ptr.p,
                       c->ent.p, (const pl::Record *)c->rec.p, (const pl::MassRecord *)m->rec.p, m->rotary, m->nm(), op.c_K,
                       op.c_M, fixedbits, x, y, dot_dev, s.stride);
}
template <int LPN>
int launch_dyn_multi_lpn(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x,
                         double *y, bool masked, double *dot_dev) {
  if (s.KB == 1) launch_dyn_multi_t<LPN, 1>(c, op, s, fixedbits, x, y, masked, dot_dev);
  else if (s.KB == 2) launch_dyn_multi_t<LPN, 2>(c, op, s, fixedbits, x, y, masked, dot_dev);
  else return fail(PL_ERR_ARG, "the fused K, M product is built for column blocks of 1 and 2");   // a missing kernel is an error
  return PL_OK;
}
// y_j = (c_K K + c_M M) x_j (masked: P (...)) for every column of the shape, one launch; the mass records must be current
int launch_dyn_multi(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x, double *y,
                     bool masked, double *dot_dev) {
  int rc = PL_OK;
  switch (c->lpn) {
    case 1: rc = launch_dyn_multi_lpn<1>(c, op, s, fixedbits, x, y, masked, dot_dev); break;
    case 2: rc = launch_dyn_multi_lpn<2>(c, op, s, fixedbits, x, y, masked, dot_dev); break;
    case 4: rc = launch_dyn_multi_lpn<4>(c, op, s, fixedbits, x, y, masked, dot_dev); break;
    case 8: rc = launch_dyn_multi_lpn<8>(c, op, s, fixedbits, x, y, masked, dot_dev); break;
    case 16: rc = launch_dyn_multi_lpn<16>(c, op, s, fixedbits, x, y, masked, dot_dev); break;
    default: return fail(PL_ERR_ARG, "lanes per node must be 1, 2, 4, 8 or 16");
  }
  if (rc) return rc;
  PL_HIP(hipGetLastError());
  return PL_OK;
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

}  // namespace
