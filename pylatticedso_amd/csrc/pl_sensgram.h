// Per-strut Gram of several fields in the strut's radius derivative (pl_sens_gram):
//     gram[p(k, l)][b] = x_k,e^T (dK_e/dr_b) x_l,e,   k <= l < NR,   p(k, l) = k NR - k (k - 1) / 2 + (l - k),
// at fixed segment geometry - the quantity of k_sens for every pair of NR columns in ONE pass over the struts.
//
// What k_sens pays for is the record: strut_flexibility -> dscalars_dr -> make_record is a few dozen divisions, against six
// fused multiply-adds per pairing.  Here it is built once per strut.  dK_e is symmetric and acts on the strut's six relative
// deformations only (pl_device.h tip_force: du = uB - uA + d x thA, dth = thB - thA), so with delta_l = (du_l, dth_l) and
// (F_k, M_k) = dK_e delta_k the Gram is G_kl = F_k . du_l + M_k . dth_l (pl_kernels.h strut_pairing), needed for k <= l only.
//
// One thread per strut, no scatter, no atomics.  NR is compiled in: the 6 NR deformations stay in registers (12 VGPRs per
// column), and the loops are ordered so that beside them only the force of the CURRENT column k is live - it is formed,
// contracted with the deformations of the columns l >= k, and dropped.  The rows of the output are [pair][B]: lane i of a
// wave writes strut b0 + i, so every pair is one store of 64 consecutive doubles.  The columns are read by gather through
// conn (12 doubles per column and strut, as three 16-byte loads per end).  Struts are in the library's internal order; the
// caller's numbering is restored on the host (pl_api.hip pl_sens_gram), as for pl_sens.
#pragma once
#include "pl_kernels.h"
#include "pl_context.h"

static_assert(PL_SENS_GRAM_MAX == 8, "launch_sens_gram dispatches the column counts 1 ... 8");

namespace pl {

// (F, M) = (dK_e or K_e) applied to the relative deformations (du, dth): the last two lines of tip_force
__device__ __forceinline__ void rel_force(const Record &r, V3 d, V3 du, V3 dth, V3 &F, V3 &M) {
  F = r.a * du + (r.e1 * dot(du, d)) * d + r.e2 * cross(d, dth);
  M = r.c * dth + (r.e3 * dot(dth, d)) * d - r.e2 * cross(d, du);
}

template <int NR>
__global__ __launch_bounds__(kBlock) void k_sens_gram(int64_t B, int64_t n6, const double *__restrict__ xyz,
                                                      const int32_t *__restrict__ conn, const double *__restrict__ radius,
                                                      const double *__restrict__ seg_len,
                                                      const int32_t *__restrict__ seg_nsub,
                                                      const double *__restrict__ mult, Material m,
                                                      const double *__restrict__ x, double *__restrict__ gram) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  if (mult) m = scaled(m, mult[b]);
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const V3 d = {xyz[3 * ib] - xyz[3 * ia], xyz[3 * ib + 1] - xyz[3 * ia + 1], xyz[3 * ib + 2] - xyz[3 * ia + 2]};
  // the record first: its divisions need about 90 VGPRs for a moment and leave 8 doubles.  (With the gathers in front of
  // it the compiler keeps all 24 NR loaded registers beside that peak: 231 VGPRs for six columns, and the eight-column
  // kernel fills the file and runs one wave per SIMD.  In this order: 140 VGPRs / 3 waves for six, 184 / 2 for eight.)
  const double len[3] = {seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2]};
  const int ns[3] = {seg_nsub[3 * b], seg_nsub[3 * b + 1], seg_nsub[3 * b + 2]};
  const Record dr = strut_drecord(radius[b], len, ns, m, d);       // once per strut
  // the deformations of every column
  V3 du[NR], dth[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const double *xk = x + (int64_t)k * n6;
    V3 uA, tA, uB, tB;
    load6(xk + 6 * ia, uA, tA);
    load6(xk + 6 * ib, uB, tB);
    du[k] = uB - uA + cross(d, tA);
    dth[k] = tB - tA;
  }
  double *out = gram + b;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    V3 F, M;
    rel_force(dr, d, du[k], dth[k], F, M);
#pragma unroll
    for (int l = k; l < NR; ++l) {
      *out = dot(F, du[l]) + dot(M, dth[l]);
      out += B;
    }
  }
}

}  // namespace pl

namespace {

template <int NR>
void launch_sens_gram_t(pl_context *c, const double *x, double *gram) {
  hipLaunchKernelGGL((pl::k_sens_gram<NR>), dim3(grid_for(c->B)), dim3(pl::kBlock), 0, c->stream, c->B, c->N * 6,
                     (const double *)c->xyz.p, (const int32_t *)c->conn.p, (const double *)c->radius.p,
                     (const double *)c->seg_len.p, (const int32_t *)c->seg_nsub.p, (const double *)c->mult.p, c->mat, x, gram);
}

// x: [n_rhs][6N] and gram: [n_rhs (n_rhs + 1) / 2][B] on the device, device numbering; 1 <= n_rhs <= PL_SENS_GRAM_MAX
int launch_sens_gram(pl_context *c, int n_rhs, const double *x, double *gram) {
  switch (n_rhs) {
    case 1: launch_sens_gram_t<1>(c, x, gram); break;
    case 2: launch_sens_gram_t<2>(c, x, gram); break;
    case 3: launch_sens_gram_t<3>(c, x, gram); break;
    case 4: launch_sens_gram_t<4>(c, x, gram); break;
    case 5: launch_sens_gram_t<5>(c, x, gram); break;
    case 6: launch_sens_gram_t<6>(c, x, gram); break;
    case 7: launch_sens_gram_t<7>(c, x, gram); break;
    case 8: launch_sens_gram_t<8>(c, x, gram); break;
    default: return fail(PL_ERR_ARG, "pl_sens_gram: n_rhs must be 1 ... PL_SENS_GRAM_MAX");
  }
  PL_HIP(hipGetLastError());
  return PL_OK;
}

}  // namespace
