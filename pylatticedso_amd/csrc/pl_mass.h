// Consistent mass M of the lattice and the pieces of the natural-frequency analysis built on it (pl_set_mass /
// pl_mass_spmv_multi / pl_vibration_modes / pl_vibration_modes_sens).  gfx950 only.
//
// Free vibration: K phi = omega^2 M phi on the free dofs of pl_set_bc, solved as the pencil M phi = mu K phi with the block
// subspace iteration of pl_buckling_modes (M in the place of G = -K_g; M is positive definite, so the shift stays 0 and
// omega^2 = 1 / mu).  Per strut, d = x_B - x_A, L = |d|, t = d / L.  The strut is ONE element between its two lattice nodes,
// as in K_g: a uniform circular section of the strut's plain radius r over the whole length L (penalised end zones stiffen
// K only, strut overlap at the nodes is ignored).  With the density rho of pl_set_mass and the multiplicity k,
//     m = k rho pi r^2 L,  c = m / 420,  j = m r^2 / 12 (= rho J L / 6),  g = m r^2 / (120 L^2) (= rho I / (30 L); 0: rotary = 0)
// and P = I - t t^T, u_perp = P u, s = th x t, the load on end B is
//     f_B = (m / 6) (t.(u_A + 2 u_B)) t + c [54 u_A_perp + 156 u_B_perp + 13 L s_A - 22 L s_B]
//           + g [36 (u_B_perp - u_A_perp) - 3 L (s_A + s_B)]
//     m_B = j (t.(th_A + 2 th_B)) t + t x { c [-13 L u_A_perp - 22 L u_B_perp - 3 L^2 s_A + 4 L^2 s_B]
//                                         + g [-3 L (u_B_perp - u_A_perp) + 4 L^2 s_B - L^2 s_A] }
// - the textbook block rho A L / 420 [[156, 22 L, 54, -13 L], ...] in both bending planes, the axial and torsional blocks
// [[2, 1], [1, 2]] and the Rayleigh rotary inertia of bending.  Seen from the other end the same formula holds with the
// roles swapped and d -> -d.  A point mass node_mass_i adds node_mass_i u_i on the three translations of node i.
// Radius derivative at fixed segment geometry: dM_e/dr = (2 / r) M_e[m / 6 and c terms] + (4 / r) M_e[j and g terms].
//
// Limits: those of pl_geom.h - one element per strut (a strut vibrating between its own joints is over-stiff), single-GPU
// FEM handles, the Jacobi inner solve, clustered spectra need n_sub past the cluster.
//
// Every product and reduction here has a fixed order and no floating-point atomics: equal inputs give equal bits.
#pragma once
#include "pl_geom.h"

namespace pl {

// Mass record the product reads: 48 B per strut, in the device's strut order.
struct __attribute__((aligned(16))) MassRecord {
  double m, r2, dx, dy, dz, pad;
};
__device__ __forceinline__ MassRecord load_mass(const MassRecord *__restrict__ rec, int64_t i) {
  const double2 *q = reinterpret_cast<const double2 *>(rec + i);
  const double2 a = q[0], b = q[1], c = q[2];
  return {a.x, a.y, b.x, b.y, c.x, 0.0};
}

// the four scalars of the element: m / 6, c, j, g
struct MassCoef {
  double m6, c, j, g;
};
__device__ __forceinline__ MassCoef mass_coef(const MassRecord &q, int rotary) {
  const double L2 = q.dx * q.dx + q.dy * q.dy + q.dz * q.dz;
  return {q.m / 6.0, q.m / 420.0, q.m * q.r2 / 12.0, rotary ? q.m * q.r2 / (120.0 * L2) : 0.0};
}

// Force / moment of the element on the strut's end B (span d from A to B) for end values (uA, thA) and (uB, thB).
__device__ __forceinline__ void mass_force(const MassCoef &q, V3 d, V3 uA, V3 thA, V3 uB, V3 thB, V3 &F, V3 &M) {
  const double L2 = dot(d, d), L = sqrt(L2);
  const V3 t = (1.0 / L) * d;
  const V3 pA = uA - dot(uA, t) * t, pB = uB - dot(uB, t) * t;
  const V3 sA = cross(thA, t), sB = cross(thB, t);
  const V3 dp = pB - pA;
  F = (q.m6 * dot(t, uA + 2.0 * uB)) * t + q.c * (54.0 * pA + 156.0 * pB + (13.0 * L) * sA - (22.0 * L) * sB) +
      q.g * (36.0 * dp - (3.0 * L) * (sA + sB));
  M = (q.j * dot(t, thA + 2.0 * thB)) * t +
      cross(t, q.c * ((4.0 * L2) * sB - (3.0 * L2) * sA - (13.0 * L) * pA - (22.0 * L) * pB) +
                   q.g * ((4.0 * L2) * sB - L2 * sA - (3.0 * L) * dp));
}

// One mass record per strut from the handle's current radii, multiplicities and span vectors (the spans of the condensed
// records): rebuilt inside every call, so pl_update_radii / pl_set_multiplicity need no hook.
__global__ __launch_bounds__(kBlock) void k_mass_records(int64_t B, const Record *__restrict__ rec,
                                                         const double *__restrict__ radius, const double *__restrict__ mult,
                                                         double density, MassRecord *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const Record r = load_record(rec, b);
  const double PI = 3.14159265358979323846;
  const double rad = radius[b], r2 = rad * rad;
  const double L = sqrt(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
  const double k = mult ? mult[b] : 1.0;
  double2 *o = reinterpret_cast<double2 *>(out + b);
  o[0] = {k * density * PI * r2 * L, r2};
  o[1] = {r.dx, r.dy};
  o[2] = {r.dz, 0.0};
}

// the mass forces of the element (coefficients c, span d as seen from this node) for the KB columns
template <int KB>
__device__ __forceinline__ void add_mass_forces(const MassCoef &c, V3 d, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                                double (&out)[6 * KB]) {
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    V3 uo, to, us, ts, f, m;
    column_of<KB>(xo, k, uo, to);
    column_of<KB>(xs, k, us, ts);
    mass_force(c, d, uo, to, us, ts, f, m);
    add_column<KB>(out, k, f, m);
  }
}

// M in k_gather_multi (pl_multi.h): the mass record loaded once per entry and negated in d for a strut's point1.
// node_mass != null: the node's point mass times its own translations is added once per node, after the sum over the lanes.
struct MassTerm {
  static constexpr int kMaxKB = 4;
  const MassRecord *__restrict__ rec;
  int rotary;
  const double *__restrict__ node_mass;
  template <int KB>
  __device__ __forceinline__ void entry(int64_t strut, bool point1, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                        double (&out)[6 * KB]) const {
    const MassRecord r = load_mass(rec, strut);
    const MassCoef c = mass_coef(r, rotary);
    const double sg = point1 ? -1.0 : 1.0;                       // this node is the strut's point1: d -> -d
    const V3 d = {sg * r.dx, sg * r.dy, sg * r.dz};
    add_mass_forces<KB>(c, d, xo, xs, out);
  }
  template <int KB>
  __device__ __forceinline__ void node(int64_t i, const double (&xs)[6 * KB], double (&out)[6 * KB]) const {
    if (node_mass) {                    // kernel-uniform
      const double nm = node_mass[i];
#pragma unroll
      for (int q = 0; q < 3 * KB; ++q) out[q] += nm * xs[q];
    }
  }
};

// ---------------------------------------------------------------------------------------------------------
// Sensitivities of omega^2 to the strut radii (pl_vibration_modes_sens).  For an eigenpair
// (omega^2, phi), phi = 0 on the fixed dofs, any scaling, at fixed segment geometry (the convention of pl_sens):
//     domega2/dr_b = (phi_e^T dK_e phi_e - omega^2 phi_e^T dM_e phi_e) / (phi^T M phi)
// - no adjoint solve: neither matrix depends on a displacement field.  One thread per strut loops over all column blocks,
// no scatter.  dK_e is the record derivative of k_sens (strut_drecord, strut_pairing), dM_e the closed form above.
// mm_col = gram[col * ncol + col] (k_multi_gram of phi and M phi), coef = [omega^2 (ncol) | weight (ncol)].  dom[col][b] for
// the n_live columns and dsum[b] = sum_col weight_col dom[col][b] in the order of the columns (either may be null).
// ---------------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kBlock) void k_mass_sens(int64_t B, const int32_t *__restrict__ conn,
                                                      const MassRecord *__restrict__ mrec, int rotary,
                                                      const double *__restrict__ radius, const double *__restrict__ seg_len,
                                                      const int32_t *__restrict__ seg_nsub, const double *__restrict__ mult,
                                                      Material m, const double *__restrict__ phi,
                                                      const double *__restrict__ gram, const double *__restrict__ coef,
                                                      int n_live, int ncb, int64_t stride, double *__restrict__ dom,
                                                      double *__restrict__ dsum) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
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
  const int ncol = ncb * KB;
  double sum = 0.0;
  for (int cb = 0; cb < ncb; ++cb) {
    double xa[6 * KB], xb[6 * KB];
    load_row<KB>(phi + (size_t)cb * stride, ia, xa);
    load_row<KB>(phi + (size_t)cb * stride, ib, xb);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      V3 pA, rA, pB, rB, F, M, fA, mA, fB, mB;
      column_of<KB>(xa, k, pA, rA);
      column_of<KB>(xb, k, pB, rB);
      tip_force(dr, pA, rA, pB, rB, F, M);
      const double qk = strut_pairing(d, F, M, pA, rA, pB, rB);
      mass_force(dc, d, pA, rA, pB, rB, fB, mB);
      mass_force(dc, dn, pB, rB, pA, rA, fA, mA);
      const double qm = dot(pA, fA) + dot(rA, mA) + dot(pB, fB) + dot(rB, mB);
      const int col = cb * KB + k;
      if (col < n_live) {
        const double om2 = coef[col];
        const double v = (qk - om2 * qm) / gram[(size_t)col * ncol + col];
        if (dom) dom[(size_t)col * B + b] = v;
        sum += coef[ncol + col] * v;
      }
    }
  }
  if (dsum) dsum[b] = sum;
}

}  // namespace pl

namespace {

// Mass data of the handle (pl_context::mass_ws), set by pl_set_mass; the records are rebuilt by every call.
struct MassWs {
  double density = 0.0;
  int rotary = 1;
  bool have_nm = false;
  DevBuf<double> node_mass;        // [N], device numbering
  DevBuf<pl::MassRecord> rec;      // [B]
  const double *nm() const { return have_nm ? node_mass.p : nullptr; }
};

int launch_mass_records(pl_context *c, MassWs *m) {
  if (m->rec.n < (size_t)c->B) PL_HIP(m->rec.alloc((size_t)c->B));
  hipLaunchKernelGGL(pl::k_mass_records, dim3(grid_for(c->B)), dim3(pl::kBlock), 0, c->stream, c->B, (const pl::Record *)c->rec.p,
                     (const double *)c->radius.p, (const double *)c->mult.p, m->density, m->rec.p);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

inline pl::MassTerm mass_term(const MassWs *m) { return {m->rec.p, m->rotary, m->nm()}; }
// y_j = M x_j (masked: P M x_j) for every column of the shape, one launch
inline int launch_mass_multi(pl_context *c, const MassWs *m, const MultiShape &s, const double *x, double *y, bool masked) {
  return launch_gather_multi(c, s, mass_term(m), c->fixedbits.p, x, y, masked, nullptr);
}

// rows of domega^2/dr (dom may be null) and their weighted sum (dsum may be null) from phi, g->M and g->scoef
template <int KB>
void launch_mass_sens_t(pl_context *c, const GeomWs *g, const MassWs *m, const MultiShape &s, const double *phi, double *dom,
                        double *dsum) {
  hipLaunchKernelGGL((pl::k_mass_sens<KB>), dim3(grid_for(c->B)), dim3(pl::kBlock), 0, c->stream, c->B, (const int32_t *)c->conn.p,
                     (const pl::MassRecord *)m->rec.p, m->rotary, (const double *)c->radius.p, (const double *)c->seg_len.p,
                     (const int32_t *)c->seg_nsub.p, (const double *)c->mult.p, c->mat, phi, (const double *)g->M.p,
                     (const double *)g->scoef.p, s.n_rhs, s.ncb, s.stride, dom, dsum);
}
int launch_mass_sens(pl_context *c, const GeomWs *g, const MassWs *m, const MultiShape &s, const double *phi, double *dom,
                     double *dsum) {
  if (s.KB == 1) launch_mass_sens_t<1>(c, g, m, s, phi, dom, dsum);
  else if (s.KB == 2) launch_mass_sens_t<2>(c, g, m, s, phi, dom, dsum);
  else launch_mass_sens_t<4>(c, g, m, s, phi, dom, dsum);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

}  // namespace
