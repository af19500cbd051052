// Radius sensitivities of the transient response by the discrete adjoint of the Newmark scheme (pl_transient_sens; DESIGN.md
// section 10h).  gfx950 only.
//
// Objective: one scalar output per row, y_n = l . u_n (l zero on the fixed dofs), J = sum w_n y_n | 1/2 sum w_n y_n^2 |
// (sum w_n |y_n|^p)^(1/p), c_n = dJ/dy_n formed on the host between the passes.  With c2 = dt^2 (1/2 - beta), c3 = dt (1 - gamma),
// cu = beta dt^2, cv = gamma dt the scheme of pl_dyn.h is, on the free dofs, equilibrium at every row plus
//     u_n = u_{n-1} + dt v_{n-1} + c2 a_{n-1} + cu a_n,   v_n = v_{n-1} + c3 a_{n-1} + cv a_n          (n >= 1)
// and its adjoint runs backwards from mu = nu = 0, for n = N ... 1:
//     S lam_n = (cu + cv dt + c2) mu + (cv + c3) nu - cu c_n l          (the S, the Jacobi PCG and the zero start of the forward step)
//     mu' = mu - c_n l - K lam_n,   nu' = nu + dt mu - C lam_n          (the OLD mu on the right)
// closed by M lam_0 = c2 mu + c3 nu (the matrix of the a_0 solve).  At fixed segment geometry (the convention of pl_sens)
//     dJ/dr_b = sum_{n=0}^{N} lam_n,e^T dK_e (u_n + ray_k v_n)_e + lam_n,e^T dM_e (a_n + ray_m v_n + a_g[n] e_dir)_e
// - dead loads have no derivative, the base-acceleration load -a_g[n] M e_dir has (e_dir: the rigid translation of ALL nodes,
// supports included), point masses have none.
//
// Histories.  The forward pass (the row loop of pl_transient, shared with that call) keeps wK_n = u_n + ray_k v_n and
// wM_n = a_n + ray_m v_n + a_g[n] e_dir on the device, [n_steps + 1][6N] each: 2 * 48 N (n_steps + 1) bytes - about 170 MB for
// the 20^3 Octet column at 50 steps.  No checkpointing.  lam is kept for a chunk of kSensChunk rows only ([kSensChunk][6N]):
// k_transient_sens runs once per chunk, so the strut's derivative records are built once per kSensChunk / kSensGroups rows.
//
// Every sum has a fixed order and there is no floating-point atomic in the contraction: each (row group, strut) cell of the
// accumulator belongs to one thread in every launch, and k_transient_sens_sum adds the groups in their order.
#pragma once
#include "pl_dyn.h"

namespace pl {

constexpr int kSensChunk = PL_TRANSIENT_SENS_CHUNK;   // rows of lam kept on the device; one k_transient_sens launch per chunk
constexpr int kSensGroups = 4;                        // row groups of a launch: a 96-strut lattice still fills a workgroup

// After the corrector of row `row`: wK = u + ray_k v, wM = a + ray_m v + ag e_dir (edir == null: no base acceleration) into the
// histories' row, and l . u into the slots of the row.
__global__ __launch_bounds__(kBlock) void k_newmark_history(int64_t n6, const double *__restrict__ st,
                                                            const double *__restrict__ l, const double *__restrict__ edir,
                                                            double ag, double ray_m, double ray_k, double *__restrict__ wK,
                                                            double *__restrict__ wM, double *__restrict__ yslots) {
  __shared__ double red[1][kBlock / kWave];
  double s[1] = {0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const double2 *sp = reinterpret_cast<const double2 *>(st + 4 * e);
    const double2 s0 = sp[0], s1 = sp[1];
    const double u = s0.x, v = s0.y, a = s1.x;
    wK[e] = u + ray_k * v;
    wM[e] = a + ray_m * v + (edir ? ag * edir[e] : 0.0);
    s[0] += l[e] * u;
  }
  double *dst[1] = {yslots};
  block_add_slots<1>(s, red, dst);
}

// One thread per dof, row n of the backward sweep after its solve: lam = lam_n, Kl = P K lam_n, Ml = P M lam_n.
//     mu' = mu - c_cur l - Kl,   nu' = nu + dt mu - ray_m Ml - ray_k Kl,   rhs = ca mu' + cb nu' - cl_next l
// - the right-hand side of the next solve: (ca, cb, cl_next) = (cu + cv dt + c2, cv + c3, cu c_{n-1}) before a step row,
// (c2, c3, 0) before row 0.  lam goes into its row of the chunk.  lam == null opens the sweep: mu = nu = 0, rhs = -cl_next l.
__global__ __launch_bounds__(kBlock) void k_newmark_adjoint(int64_t n6, const double *__restrict__ lam,
                                                            const double *__restrict__ Kl, const double *__restrict__ Ml,
                                                            const double *__restrict__ l, double dt, double ray_m, double ray_k,
                                                            double c_cur, double ca, double cb, double cl_next,
                                                            double *__restrict__ mu, double *__restrict__ nu,
                                                            double *__restrict__ rhs, double *__restrict__ lam_row) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const double lv = l[e];
    double m = 0.0, n = 0.0;
    if (lam) {   // kernel-uniform
      const double k = Kl[e], mm = Ml[e], m_old = mu[e];
      m = m_old - c_cur * lv - k;
      n = nu[e] + dt * m_old - ray_m * mm - ray_k * k;
      lam_row[e] = lam[e];
    }
    mu[e] = m;
    nu[e] = n;
    rhs[e] = ca * m + cb * n - cl_next * lv;
  }
}

// The contraction, one thread per (strut, row group): the strut's dK_e/dr record and dM_e/dr coefficients once, then for the
// rows g, g + kSensGroups, ... of the chunk (lam, wK, wM: the chunk's first row, plain [6N] rows)
//     lam_e^T dK_e wK_e   (tip_force of wK paired with the relative deformations of lam, strut_pairing)
//   + lam_e^T dM_e wM_e   (mass_force of wM with the derivative coefficients, on both ends, against lam)
// added to acc[g][b] - this thread's own cell in every launch of the call.
__global__ __launch_bounds__(kBlock) void k_transient_sens(int64_t B, const int32_t *__restrict__ conn,
                                                           const MassRecord *__restrict__ mrec, int rotary,
                                                           const double *__restrict__ radius, const double *__restrict__ seg_len,
                                                           const int32_t *__restrict__ seg_nsub, const double *__restrict__ mult,
                                                           Material m, const double *__restrict__ lam,
                                                           const double *__restrict__ wK, const double *__restrict__ wM,
                                                           int64_t n6, int nrows, double *__restrict__ acc) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int g = blockIdx.y;
  if (b >= B) return;
  if (mult) m = scaled(m, mult[b]);
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const MassRecord q = load_mass(mrec, b);
  const V3 d = {q.dx, q.dy, q.dz}, dn = {-q.dx, -q.dy, -q.dz};
  const double rad = radius[b];
  const double len[3] = {seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2]};
  const int ns[3] = {seg_nsub[3 * b], seg_nsub[3 * b + 1], seg_nsub[3 * b + 2]};
  const Record dr = strut_drecord(rad, len, ns, m, d);
  const MassCoef c0 = mass_coef(q, rotary);
  const MassCoef dc = {2.0 / rad * c0.m6, 2.0 / rad * c0.c, 4.0 / rad * c0.j, 4.0 / rad * c0.g};
  double sum = 0.0;
  for (int r = g; r < nrows; r += kSensGroups) {
    const size_t off = (size_t)r * (size_t)n6;
    V3 lA, mA, lB, mB, pA, rA, pB, rB, F, M, fA, tA, fB, tB;
    load6(lam + off + 6 * ia, lA, mA);
    load6(lam + off + 6 * ib, lB, mB);
    load6(wK + off + 6 * ia, pA, rA);
    load6(wK + off + 6 * ib, pB, rB);
    tip_force(dr, pA, rA, pB, rB, F, M);
    const double qk = strut_pairing(d, F, M, lA, mA, lB, mB);
    load6(wM + off + 6 * ia, pA, rA);
    load6(wM + off + 6 * ib, pB, rB);
    mass_force(dc, d, pA, rA, pB, rB, fB, tB);
    mass_force(dc, dn, pB, rB, pA, rA, fA, tA);
    const double qm = dot(lA, fA) + dot(mA, tA) + dot(lB, fB) + dot(mB, tB);
    sum += qk + qm;
  }
  acc[(size_t)g * B + b] += sum;
}

// out[b] = acc[0][b] + acc[1][b] + ... in the order of the groups
__global__ __launch_bounds__(kBlock) void k_transient_sens_sum(int64_t B, const double *__restrict__ acc, double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
#pragma unroll
  for (int g = 0; g < kSensGroups; ++g) s += acc[(size_t)g * B + b];
  out[b] = s;
}

}  // namespace pl

namespace {

// Device data of one pl_transient_sens call beside the DynWs of its forward pass, owned by the handle
// (pl_context::dyn_sens_ws), grown on demand.
struct DynSensWs {
  DevBuf<double> wK, wM;           // [rows][6N] histories
  DevBuf<double> lam;              // [kSensChunk][6N]
  DevBuf<double> mu, nu, Kl, Ml;   // [6N]
  DevBuf<double> l, edir;          // [6N]: the output vector (0 on fixed dofs), the rigid translation of every node
  DevBuf<double> yslots;           // [rows][kSlots]
  DevBuf<double> acc, grad;        // [kSensGroups][B], [B]
};

// What the sensitivity call adds to the forward pass (transient_forward): null for pl_transient.
struct DynHistory {
  DynSensWs *s = nullptr;
  const double *l_host = nullptr;     // [6N] host, caller numbering: the output vector
  const double *base_dir = nullptr;   // [3] host, with base_acc [rows] host: the pattern P M e_dir goes behind the caller's
  const double *base_acc = nullptr;
};

int launch_transient_sens(pl_context *c, const MassWs *m, DynSensWs *s, int64_t row0, int nrows) {
  const size_t n6 = (size_t)c->N * 6;
  hipLaunchKernelGGL(pl::k_transient_sens, dim3(grid_for(c->B), pl::kSensGroups), dim3(pl::kBlock), 0, c->stream, c->B,
                     (const int32_t *)c->conn.p, (const pl::MassRecord *)m->rec.p, m->rotary, (const double *)c->radius.p,
                     (const double *)c->seg_len.p, (const int32_t *)c->seg_nsub.p, (const double *)c->mult.p, c->mat,
                     (const double *)s->lam.p, (const double *)s->wK.p + (size_t)row0 * n6,
                     (const double *)s->wM.p + (size_t)row0 * n6, (int64_t)n6, nrows, s->acc.p);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

}  // namespace
