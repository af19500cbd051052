// Radius sensitivities of the frequency response (pl_harmonic_sens).  gfx950 only.
//
// Per frequency w_k the system of pl_harm.h, A_k u_k = f with A_k = c_K K + c_M M, and one complex output y_k = l^T u_k
// (unconjugated; l zero on the fixed dofs).  A_k is complex SYMMETRIC, so the adjoint field solves the same matrix,
//     A_k lam_k = l,
// with no transpose and no conjugate, and does not depend on the objective: it is solved together with u_k, as column block
// nf + j of a pass of nf frequencies (block j is u_j; both carry the coefficients of frequency j).  At fixed segment geometry
// (the convention of pl_sens), for strut b with end rows e,
//     dy_k/dr_b = -[ c_K lam_e^T dK_e u_e + c_M lam_e^T dM_e u_e + s lam_e^T dM_e e_dir,e ]
// - dead loads have no derivative, the load -P M e_dir of a base shaken with unit acceleration has (s = 1; e_dir: the rigid
// translation of ALL nodes, supports included), point masses have none.  With l = f (out_vec = NULL) lam_k = u_k, there is no
// second solve, and with a base l follows the design too: s = 2.  For a real objective J of the outputs with g_k = dJ/dy_k
// (formed on the host from the downloaded y_k: the one host look between the solves and the contraction)
//     dJ/dr_b = sum_k Re(g_k dy_k/dr_b).
//
// Kept fields.  U[n_freq][12 N] and L[n_freq][12 N] (complex rows as in pl_harm.h) stay on the device for the call:
// 2 * 96 N n_freq bytes, half of it when l = f.  No checkpointing.
//
// Every sum has a fixed order and there is no floating-point atomic in the contraction: each (frequency group, strut) cell of
// the accumulator belongs to one thread of the one launch, and k_transient_sens_sum adds the groups in their order.
#pragma once
#include "pl_dyn_sens.h"
#include "pl_harm.h"

namespace pl {

constexpr int kHarmSensGroups = 4;   // frequency groups of the launch: a 96-strut lattice still fills a workgroup
static_assert(kHarmSensGroups == kSensGroups, "k_transient_sens_sum adds the groups");

// f -= Me on the real parts: the load of a base shaken with unit acceleration, Me = P M e_dir [6N] real
__global__ __launch_bounds__(kBlock) void k_harm_base_load(int64_t n6, const double *__restrict__ Me, double *__restrict__ f) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) f[2 * e] -= Me[e];
}

// y_k = l^T u_k (unconjugated) into yslots[k][2][kSlots]; grid.x (at most kSlots blocks) strides over the dofs, grid.y = k
__global__ __launch_bounds__(kBlock) void k_harm_output(int64_t n6, const double *__restrict__ l, const double *__restrict__ U,
                                                        double *__restrict__ yslots) {
  __shared__ double red[2][kBlock / kWave];
  const int k = blockIdx.y;
  const double *u = U + (size_t)k * 2 * (size_t)n6;
  double s[2] = {0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const Cplx t = cmul(load_c(l, e), load_c(u, e));
    s[0] += t.re;
    s[1] += t.im;
  }
  double *dst[2] = {yslots + (size_t)(2 * k) * kSlots, yslots + (size_t)(2 * k + 1) * kSlots};
  block_add_slots<2>(s, red, dst);
}

// the six complex dofs of node i as two real rows
__device__ __forceinline__ void load6c(const double *__restrict__ x, int64_t i, V3 &ur, V3 &tr, V3 &ui, V3 &ti) {
  const double2 *q = reinterpret_cast<const double2 *>(x + 12 * i);
  const double2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
  ur = {a.x, b.x, c.x};
  ui = {a.y, b.y, c.y};
  tr = {d.x, e.x, f.x};
  ti = {d.y, e.y, f.y};
}

// The contraction, one thread per (strut, frequency group): the strut's dK_e/dr record, its dM_e/dr coefficients and (s != 0)
// the mass force of e_dir on both ends once, then for the frequencies k = g, g + kHarmSensGroups, ...
//     q_K = lam_e^T dK_e u_e   (tip_force of Re u and of Im u, each paired with Re lam and Im lam: strut_pairing)
//     q_M = lam_e^T dM_e u_e   (mass_force of Re u and of Im u on both ends, against Re lam and Im lam)
//     q_E = lam_e^T dM_e e_dir,e
//     t = c_K q_K + c_M q_M + s q_E,   sum -= Re(g_k t)
// into acc[g][b], this thread's own cell.  U, L: [n_freq][12 N] (L == U when l = f); coef[k][4], g[k][2] read uniformly.
__global__ __launch_bounds__(kBlock) void k_harmonic_sens(int64_t B, const int32_t *__restrict__ conn,
                                                          const MassRecord *__restrict__ mrec, int rotary,
                                                          const double *__restrict__ radius, const double *__restrict__ seg_len,
                                                          const int32_t *__restrict__ seg_nsub, const double *__restrict__ mult,
                                                          Material m, const double *__restrict__ U, const double *__restrict__ L,
                                                          const double *__restrict__ coef, const double *__restrict__ gk,
                                                          int64_t n12, int n_freq, double s, V3 edir, double *__restrict__ acc) {
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
  const V3 zero = {0.0, 0.0, 0.0};
  V3 eFA = zero, eTA = zero, eFB = zero, eTB = zero;
  if (s != 0.0) {   // kernel-uniform
    mass_force(dc, d, edir, zero, edir, zero, eFB, eTB);
    mass_force(dc, dn, edir, zero, edir, zero, eFA, eTA);
  }
  double sum = 0.0;
  for (int k = g; k < n_freq; k += kHarmSensGroups) {
    const double *u = U + (size_t)k * (size_t)n12, *l = L + (size_t)k * (size_t)n12;
    V3 lAr, mAr, lAi, mAi, lBr, mBr, lBi, mBi, pA, rA, pB, rB, xA, yA, xB, yB, F, M, fA, tA, fB, tB;
    load6c(l, ia, lAr, mAr, lAi, mAi);
    load6c(l, ib, lBr, mBr, lBi, mBi);
    load6c(u, ia, pA, rA, xA, yA);
    load6c(u, ib, pB, rB, xB, yB);
    // Re u
    tip_force(dr, pA, rA, pB, rB, F, M);
    double qKr = strut_pairing(d, F, M, lAr, mAr, lBr, mBr);
    double qKi = strut_pairing(d, F, M, lAi, mAi, lBi, mBi);
    mass_force(dc, d, pA, rA, pB, rB, fB, tB);
    mass_force(dc, dn, pB, rB, pA, rA, fA, tA);
    double qMr = dot(lAr, fA) + dot(mAr, tA) + dot(lBr, fB) + dot(mBr, tB);
    double qMi = dot(lAi, fA) + dot(mAi, tA) + dot(lBi, fB) + dot(mBi, tB);
    // Im u
    tip_force(dr, xA, yA, xB, yB, F, M);
    qKr -= strut_pairing(d, F, M, lAi, mAi, lBi, mBi);
    qKi += strut_pairing(d, F, M, lAr, mAr, lBr, mBr);
    mass_force(dc, d, xA, yA, xB, yB, fB, tB);
    mass_force(dc, dn, xB, yB, xA, yA, fA, tA);
    qMr -= dot(lAi, fA) + dot(mAi, tA) + dot(lBi, fB) + dot(mBi, tB);
    qMi += dot(lAr, fA) + dot(mAr, tA) + dot(lBr, fB) + dot(mBr, tB);
    const double qEr = dot(lAr, eFA) + dot(mAr, eTA) + dot(lBr, eFB) + dot(mBr, eTB);
    const double qEi = dot(lAi, eFA) + dot(mAi, eTA) + dot(lBi, eFB) + dot(mBi, eTB);
    const double *c = coef + 4 * k;
    const Cplx cK = {c[0], c[1]}, cM = {c[2], c[3]}, gv = {gk[2 * k], gk[2 * k + 1]};
    const Cplx a = cmul(cK, {qKr, qKi}), bq = cmul(cM, {qMr, qMi});
    const Cplx t = {a.re + bq.re + s * qEr, a.im + bq.im + s * qEi};
    sum -= gv.re * t.re - gv.im * t.im;
  }
  acc[(size_t)g * B + b] = sum;
}

}  // namespace pl

namespace {

constexpr int kHarmSensMaxFreq = PL_MULTI_MAX / 4;   // frequencies per pass with an adjoint block beside every field

// Device data of one pl_harmonic_sens call beside the workspaces of pl_harmonic, owned by the handle
// (pl_context::harm_sens_ws), grown on demand.
struct HarmSensWs {
  DevBuf<double> U, L;             // [n_freq][12N] kept fields (L unused when l = f)
  DevBuf<double> fl;               // [2][12N]: the load f and the output vector l, complex, 0 on fixed dofs
  DevBuf<double> edir, Me;         // [6N]: the rigid translation of every node, P M e_dir
  DevBuf<double> coef, g;          // [n_freq][4], [n_freq][2]
  DevBuf<double> yslots;           // [n_freq][2][kSlots]
  DevBuf<double> acc, grad;        // [kHarmSensGroups][B], [B]
};

int launch_harmonic_sens(pl_context *c, const MassWs *m, HarmSensWs *s, bool self_adjoint, int n_freq, double sfac,
                         const double *base_dir) {
  const pl::V3 e = base_dir ? pl::V3{base_dir[0], base_dir[1], base_dir[2]} : pl::V3{0.0, 0.0, 0.0};
  hipLaunchKernelGGL(pl::k_harmonic_sens, dim3(grid_for(c->B), pl::kHarmSensGroups), dim3(pl::kBlock), 0, c->stream, c->B,
                     (const int32_t *)c->conn.p, (const pl::MassRecord *)m->rec.p, m->rotary, (const double *)c->radius.p,
                     (const double *)c->seg_len.p, (const int32_t *)c->seg_nsub.p, (const double *)c->mult.p, c->mat,
                     (const double *)s->U.p, (const double *)(self_adjoint ? s->U.p : s->L.p), (const double *)s->coef.p,
                     (const double *)s->g.p, (int64_t)c->N * 12, n_freq, sfac, e, s->acc.p);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

}  // namespace
