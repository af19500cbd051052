// Geometric stiffness K_g(u) of the lattice and the pieces of the global linear buckling analysis built on it
// (pl_geom_spmv_multi / pl_buckling_modes / pl_buckling_modes_sens).  gfx950 only.
//
// Linearised buckling: with u the equilibrium of the applied loads, find the smallest lambda > 0 with
//     (K + lambda K_g(u)) phi = 0            on the free dofs of pl_set_bc,
// K_g the geometric stiffness of the axial forces N in u.  Per strut, d = x_B - x_A, L = |d|, t = d / L and N = F.t the
// record's TOTAL axial force (tip_force, tension > 0; a record of multiplicity k stands for k copies that carry N / k each,
// so K_g takes the total).  The strut is ONE Hermite-cubic element between its two lattice nodes; with g = N / (30 L),
// P = I - t t^T, delta = P (u_B - u_A), s_A = th_A x t, s_B = th_B x t:
//     f_B = g [36 delta - 3 L (s_A + s_B)]                 f_A = -f_B
//     m_A = t x g [-3 L delta + 4 L^2 s_A - L^2 s_B]       m_B = t x g [-3 L delta + 4 L^2 s_B - L^2 s_A]
// - the textbook block N / (30 L) [[36, 3L, -36, 3L], [3L, 4L^2, -3L, -L^2], ...] in both bending planes, no axial and no
// torsional terms.  Seen from the other end the same formula holds with d -> -d.
//
// Limits: single-GPU FEM handles only.  ONE element per strut in K_g: penalised end zones and sub-element counts do not
// enter, a strut buckling between its own two joints cannot be represented and is over-estimated (pl_buckling covers that
// failure).  Linearised prebuckling only.  A spectrum dominated by tension (|mu_min| >> mu_max, mu = 1 / lambda) converges
// slowly under the shift of the eigen-iteration; it stays correct, and max_outer bounds it.
//
// Every product and reduction here has a fixed order and no floating-point atomics: equal inputs give equal bits.
#pragma once
#include <algorithm>
#include <chrono>
#include <limits>
#include <vector>

#include "pl_buckling.h"
#include "pl_multi.h"

namespace pl {

// Geometric record the product reads: 4 doubles = 32 B per strut, in the device's strut order.
struct __attribute__((aligned(16))) GeomRecord {
  double g, dx, dy, dz;
};
__device__ __forceinline__ GeomRecord load_geom(const GeomRecord *__restrict__ rec, int64_t i) {
  const double2 *q = reinterpret_cast<const double2 *>(rec + i);
  const double2 a = q[0], b = q[1];
  return {a.x, a.y, b.x, b.y};
}

// Force / moment of K_g on the strut's end B for end values (uA, thA) and (uB, thB).
__device__ __forceinline__ void geom_force(const GeomRecord &q, V3 uA, V3 thA, V3 uB, V3 thB, V3 &F, V3 &M) {
  const V3 d = {q.dx, q.dy, q.dz};
  const double L2 = dot(d, d), L = sqrt(L2);
  const V3 t = (1.0 / L) * d;
  const V3 du = uB - uA;
  const V3 delta = du - dot(du, t) * t;
  const V3 sA = cross(thA, t), sB = cross(thB, t);
  F = q.g * (36.0 * delta - (3.0 * L) * (sA + sB));
  M = cross(t, q.g * ((4.0 * L2) * sB - L2 * sA - (3.0 * L) * delta));
}

// One geometric record per strut from the displacements u (device numbering): N with the arithmetic of k_buckling_util
// (tip_force, stress_strut), taken for the whole record (multiplicity 1).
__global__ __launch_bounds__(kBlock) void k_geom_records(int64_t B, const int32_t *__restrict__ conn,
                                                         const Record *__restrict__ rec, const double *__restrict__ u,
                                                         GeomRecord *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const Record r = load_record(rec, b);
  V3 uA, tA, uB, tB, F, M;
  load6(u + 6 * ia, uA, tA);
  load6(u + 6 * ib, uB, tB);
  tip_force(r, uA, tA, uB, tB, F, M);
  const StressStrut s = stress_strut(r, 1.0, F, M);
  double2 *o = reinterpret_cast<double2 *>(out + b);
  o[0] = {s.N / (30.0 * s.L), r.dx};
  o[1] = {r.dy, r.dz};
}

// K_g in k_gather_multi (pl_multi.h): the geometric record loaded once per entry and negated in d for a strut's point1
struct GeomTerm {
  static constexpr int kMaxKB = 4;
  const GeomRecord *__restrict__ rec;
  template <int KB>
  __device__ __forceinline__ void entry(int64_t strut, bool point1, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                        double (&out)[6 * KB]) const {
    GeomRecord r = load_geom(rec, strut);
    if (point1) { r.dx = -r.dx; r.dy = -r.dy; r.dz = -r.dz; }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      V3 uo, to, us, ts, f, m;
      column_of<KB>(xo, k, uo, to);
      column_of<KB>(xs, k, us, ts);
      geom_force(r, uo, to, us, ts, f, m);
      add_column<KB>(out, k, f, m);
    }
  }
  template <int KB>
  __device__ __forceinline__ void node(int64_t, const double (&)[6 * KB], double (&)[6 * KB]) const {}
};

// ---------------------------------------------------------------------------------------------------------
// All ncol x ncol dot products M[i][j] = A_i . B_j of two arrays in the column-block layout, in two stages of a fixed
// order.  Stage 1: grid.y = (column block of A, column block of B), grid.x = chunks of a grid-stride walk over the 6N
// dofs; a thread keeps the KB x KB products of its dofs, the block folds them (wave_sum, then its waves in order) into
// part[(pair KB KB + q) * gridDim.x + chunk].  Stage 2 (k_multi_gram_fold): one block per entry walks its partials in a
// fixed stride and folds them in the fixed LDS tree of the stress pass.
// ---------------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_gram(int64_t n6, const double *__restrict__ A, const double *__restrict__ Bv,
                                                       double *__restrict__ part, int ncb, int64_t stride) {
  __shared__ double red[KB * KB][kBlock / kWave];
  const int pair = blockIdx.y, ca = pair / ncb, cbb = pair - ca * ncb;
  const double *a = A + (size_t)ca * stride, *b = Bv + (size_t)cbb * stride;
  double acc[KB * KB];
#pragma unroll
  for (int q = 0; q < KB * KB; ++q) acc[q] = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    double av[KB], bv[KB];
    load_cols<KB>(a, e, av);
    load_cols<KB>(b, e, bv);
#pragma unroll
    for (int i = 0; i < KB; ++i)
#pragma unroll
      for (int j = 0; j < KB; ++j) acc[i * KB + j] += av[i] * bv[j];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < KB * KB; ++q) {
    const double t = wave_sum(acc[q]);
    if (lane == 0) red[q][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < KB * KB) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kBlock / kWave; ++i) t += red[threadIdx.x][i];
    part[((size_t)pair * KB * KB + threadIdx.x) * gridDim.x + blockIdx.x] = t;
  }
}

// M[(ca KB + i) * ncol + cb KB + j] = sum of the nchunk partials of entry blockIdx.x = (pair KB + i) KB + j
__global__ __launch_bounds__(kBlock) void k_multi_gram_fold(int nchunk, const double *__restrict__ part, double *__restrict__ M,
                                                            int KB, int ncb) {
  __shared__ double smem[kBlock];
  const int q = blockIdx.x;
  const double *p = part + (size_t)q * nchunk;
  double v = 0.0;
  for (int i = threadIdx.x; i < nchunk; i += kBlock) v += p[i];
  v = stress_block_fold<false>(v, smem);
  if (threadIdx.x == 0) {
    const int pair = q / (KB * KB), ij = q - pair * KB * KB;
    const int ca = pair / ncb, cbb = pair - ca * ncb;
    M[(size_t)(ca * KB + ij / KB) * (ncb * KB) + cbb * KB + ij % KB] = v;
  }
}

// Z = Y C for a small C[ncol][ncol] (row-major, held in LDS); grid.y = column block of Z.  Z must not alias Y.
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_combine(int64_t n6, const double *__restrict__ Y, const double *__restrict__ Cm,
                                                          double *__restrict__ Z, int ncb, int64_t stride) {
  __shared__ double Cs[PL_MULTI_MAX * KB];     // Cs[i * KB + k] = C[i][cbo KB + k]
  const int cbo = blockIdx.y, ncol = ncb * KB;
  for (int q = threadIdx.x; q < ncol * KB; q += kBlock) Cs[q] = Cm[(size_t)(q / KB) * ncol + cbo * KB + q % KB];
  __syncthreads();
  double *z = Z + (size_t)cbo * stride;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    double out[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) out[k] = 0.0;
    for (int cbi = 0; cbi < ncb; ++cbi) {
      double yv[KB];
      load_cols<KB>(Y + (size_t)cbi * stride, e, yv);
#pragma unroll
      for (int i = 0; i < KB; ++i)
#pragma unroll
        for (int k = 0; k < KB; ++k) out[k] += yv[i] * Cs[(cbi * KB + i) * KB + k];
    }
    store_cols<KB>(z, e, out);
  }
}

// out = a x + b y over n2 pairs of doubles (any layout); out may alias x or y
__global__ __launch_bounds__(kBlock) void k_multi_axpby(int64_t n2, double a, const double *x, double b, const double *y,
                                                        double *out) {
  const double2 *xq = reinterpret_cast<const double2 *>(x), *yq = reinterpret_cast<const double2 *>(y);
  double2 *oq = reinterpret_cast<double2 *>(out);
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n2; e += (int64_t)gridDim.x * kBlock) {
    const double2 u = xq[e], v = yq[e];
    oq[e] = {a * u.x + b * v.x, a * u.y + b * v.y};
  }
}

// Start vectors of the eigen-iteration: a fixed hash of (caller node, dof, column) in (-1, 1), zero on fixed dofs.
__device__ __forceinline__ double geom_hash(uint64_t dof, uint64_t col) {
  uint64_t z = (dof * 64u + col + 1u) * 0x9E3779B97F4A7C15ull;     // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
template <int KB>
__global__ __launch_bounds__(kBlock) void k_geom_start(int64_t n6, const int32_t *__restrict__ perm,
                                                       const uint8_t *__restrict__ fixedbits, double *__restrict__ X,
                                                       int64_t stride) {
  const int cb = blockIdx.y;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const int64_t node = e / 6;
    const uint64_t dof = (uint64_t)perm[node] * 6u + (uint64_t)(e - 6 * node);
    const bool fx = dof_fixed(fixedbits, e);
    double v[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) v[k] = fx ? 0.0 : geom_hash(dof, (uint64_t)(cb * KB + k));
    store_cols<KB>(X + (size_t)cb * stride, e, v);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Sensitivities of the load factors to the strut radii (pl_buckling_modes_sens).  For an eigenpair
// (lambda, phi), phi = 0 on the fixed dofs, any scaling, at fixed segment geometry (the convention of pl_sens):
//     kk   = phi^T K phi,   q_b = phi_e^T G_b phi_e   (G_b: the strut's geometric element matrix for N = 1)
//     w    = d(phi^T K_g(u) phi)/du = sum_b q_b ka_b (-t_b at u_A, +t_b at u_B),  ka = a + e1 L^2   (N_b = ka_b t_b.(u_B - u_A))
//     K nu = -w on the free dofs, nu = 0 on the fixed ones                       (u depends on r through K u = f)
//     dlambda/dr_b = (lambda / kk) [phi_e^T dK_e phi_e + lambda (q_b dka_b t_b.(u_B - u_A) + nu_e^T dK_e u_e)],  dK_e = dK_e/dr_b
// Every kernel carries all modes in one launch, in the column-block layout of pl_multi.h.
// ---------------------------------------------------------------------------------------------------------
// q[cb][b * KB + k] = phi_e^T G_b phi_e of column cb KB + k: one thread per strut and column block, no scatter.  Of the
// geometric record only the span d is read.
template <int KB>
__global__ __launch_bounds__(kBlock) void k_geom_quad(int64_t B, const int32_t *__restrict__ conn,
                                                      const GeomRecord *__restrict__ rec, const double *__restrict__ phi,
                                                      double *__restrict__ Q, int64_t stride) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int cb = blockIdx.y;
  phi += (size_t)cb * stride;
  GeomRecord fwd = load_geom(rec, b);
  fwd.g = 1.0 / (30.0 * sqrt(fwd.dx * fwd.dx + fwd.dy * fwd.dy + fwd.dz * fwd.dz));
  const GeomRecord rev = {fwd.g, -fwd.dx, -fwd.dy, -fwd.dz};     // the strut seen from its point1
  double xa[6 * KB], xb[6 * KB], q[KB];
  load_row<KB>(phi, (int64_t)conn[2 * b], xa);
  load_row<KB>(phi, (int64_t)conn[2 * b + 1], xb);
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    V3 uA, tA, uB, tB, fA, mA, fB, mB;
    column_of<KB>(xa, k, uA, tA);
    column_of<KB>(xb, k, uB, tB);
    geom_force(fwd, uA, tA, uB, tB, fB, mB);
    geom_force(rev, uB, tB, uA, tA, fA, mA);
    q[k] = dot(uA, fA) + dot(tA, mA) + dot(uB, fB) + dot(tB, mB);
  }
  store_cols<KB>(Q + (size_t)cb * B * KB, b, q);
}

// y_k = -w_k, the load of the adjoint solve, for the KB columns of column block blockIdx.y: the per-node gather of
// k_gather_multi (same sliced ELL and lane mapping, same lpn_sum, same order of the sum over a node's struts, no
// atomics).  An entry adds -(+-) q_{b,k} ka_b t_b to the node's three translations, + at the strut's point2 and - at its
// point1; the rotations get zero.  Nothing is masked here: the solve masks its loads itself.
template <int LPN, int KB>
__global__ __launch_bounds__(kBlock) void k_geom_adjoint_load(int64_t N, int64_t B, const int64_t *__restrict__ slice_ptr,
                                                              const int2 *__restrict__ ent, const Record *__restrict__ rec,
                                                              const double *__restrict__ Q, double *__restrict__ y,
                                                              int64_t stride) {
  const unsigned blk = xcd_block(blockIdx.x, gridDim.x);
  const int cb = blockIdx.y;
  Q += (size_t)cb * B * KB;
  y += (size_t)cb * stride;
  constexpr int kSliceNodes = kWave / LPN;
  const int lane = threadIdx.x & 63, sub = lane / kSliceNodes;
  const int64_t slice = (int64_t)blk * (kBlock / kWave) + (threadIdx.x >> 6);
  const int64_t i = slice * kSliceNodes + (lane & (kSliceNodes - 1));
  if (slice * kSliceNodes >= N) return;   // wave-uniform
  double out[6 * KB];                    // the node's row; its rotations stay zero
#pragma unroll
  for (int q = 0; q < 6 * KB; ++q) out[q] = 0.0;
  const int64_t p0 = slice_ptr[slice], p1 = slice_ptr[slice + 1];
#pragma unroll 1
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const int2 e = ent[p];
    if (e.x >= 0) {
      const int64_t s = e.y & 0x7fffffff;
      const Record r = load_record(rec, s);
      double qv[KB];
      load_cols<KB>(Q, s, qv);
      const double L2 = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
      const double c = (r.a + r.e1 * L2) / sqrt(L2);              // ka / L: ka t = c d
      const double sc = e.y < 0 ? c : -c;                         // -w: + at the strut's point1 (this node), - at point2
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const double v = sc * qv[k];
        out[0 * KB + k] += v * r.dx; out[1 * KB + k] += v * r.dy; out[2 * KB + k] += v * r.dz;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 3 * KB; ++q) out[q] = lpn_sum<LPN>(out[q]);
  if (i < N && sub == 0) {
    double2 *q = reinterpret_cast<double2 *>(y + 6 * KB * i);
#pragma unroll
    for (int j = 0; j < 3 * KB; ++j) q[j] = {out[2 * j], out[2 * j + 1]};
  }
}

// dlam[col][b] = dlambda_col / dr_b for the n_live columns, and dsum[b] = sum_col weight_col dlam[col][b] in the order of
// the columns (either output may be null): one thread per strut, no scatter.  The radius derivative of the record is that
// of k_sens and k_buckling_grad (strut_drecord); nu solves K nu = -w.  kk_col = gram[col * ncol + col] (k_multi_gram of
// phi and K phi), coef = [lambda (ncol) | weight (ncol)].
template <int KB>
__global__ __launch_bounds__(kBlock) void k_geom_sens(int64_t B, const int32_t *__restrict__ conn,
                                                      const GeomRecord *__restrict__ grec, const double *__restrict__ radius,
                                                      const double *__restrict__ seg_len, const int32_t *__restrict__ seg_nsub,
                                                      const double *__restrict__ mult, Material m,
                                                      const double *__restrict__ u, const double *__restrict__ phi,
                                                      const double *__restrict__ nu, const double *__restrict__ Q,
                                                      const double *__restrict__ gram, const double *__restrict__ coef,
                                                      int n_live, int ncb, int64_t stride, double *__restrict__ dlam,
                                                      double *__restrict__ dsum) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  if (mult) m = scaled(m, mult[b]);
  const int64_t ia = conn[2 * b], ib = conn[2 * b + 1];
  const GeomRecord g = load_geom(grec, b);
  const V3 d = {g.dx, g.dy, g.dz};
  const double len[3] = {seg_len[3 * b], seg_len[3 * b + 1], seg_len[3 * b + 2]};
  const int ns[3] = {seg_nsub[3 * b], seg_nsub[3 * b + 1], seg_nsub[3 * b + 2]};
  const Record dr = strut_drecord(radius[b], len, ns, m, d);
  V3 uA, tA, uB, tB, Fu, Mu;
  load6(u + 6 * ia, uA, tA);
  load6(u + 6 * ib, uB, tB);
  tip_force(dr, uA, tA, uB, tB, Fu, Mu);                           // (dK_e u_e) on end B
  const double L2 = dot(d, d);
  const double dN = (dr.a + dr.e1 * L2) * dot(d, uB - uA) / sqrt(L2);   // dka t.(u_B - u_A)
  const int ncol = ncb * KB;
  double sum = 0.0;
  for (int cb = 0; cb < ncb; ++cb) {
    double xa[6 * KB], xb[6 * KB], t1[KB], t3[KB], qv[KB];
    load_row<KB>(phi + (size_t)cb * stride, ia, xa);
    load_row<KB>(phi + (size_t)cb * stride, ib, xb);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      V3 pA, rA, pB, rB, F, M;
      column_of<KB>(xa, k, pA, rA);
      column_of<KB>(xb, k, pB, rB);
      tip_force(dr, pA, rA, pB, rB, F, M);
      t1[k] = strut_pairing(d, F, M, pA, rA, pB, rB);
    }
    load_row<KB>(nu + (size_t)cb * stride, ia, xa);
    load_row<KB>(nu + (size_t)cb * stride, ib, xb);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      V3 pA, rA, pB, rB;
      column_of<KB>(xa, k, pA, rA);
      column_of<KB>(xb, k, pB, rB);
      t3[k] = strut_pairing(d, Fu, Mu, pA, rA, pB, rB);
    }
    load_cols<KB>(Q + (size_t)cb * B * KB, b, qv);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int col = cb * KB + k;
      if (col < n_live) {
        const double lam = coef[col];
        const double v = lam / gram[(size_t)col * ncol + col] * (t1[k] + lam * (qv[k] * dN + t3[k]));
        if (dlam) dlam[(size_t)col * B + b] = v;
        sum += coef[ncol + col] * v;
      }
    }
  }
  if (dsum) dsum[b] = sum;
}

}  // namespace pl

namespace {

// Workspace of the geometric calls, owned by the handle (pl_context::geom_ws), grown on demand.
struct GeomWs {
  DevBuf<pl::GeomRecord> rec;      // [B]
  int64_t cap = 0;                 // doubles per block vector
  DevBuf<double> Y, KY, GY, X, KX, GX;
  DevBuf<double> part, M, C;       // gram partials, two gram matrices, the combination matrix
  DevBuf<int32_t> perm;            // device node -> caller node
  DevBuf<double> sq, sdlam, scoef; // pl_buckling_modes_sens: q [ncol][B], dlam [n_modes][B] + dsum [B], lambda | weight
};

int geom_ws(pl_context *c, GeomWs **out) {
  if (!c->geom_ws) c->geom_ws = std::make_shared<GeomWs>();
  GeomWs *g = static_cast<GeomWs *>(c->geom_ws.get());
  if (g->rec.n < (size_t)c->B) PL_HIP(g->rec.alloc((size_t)c->B));
  *out = g;
  return PL_OK;
}

// the block vectors and small matrices of pl_buckling_modes for the shape s
int geom_ws_modes(pl_context *c, GeomWs *g, const MultiShape &s, unsigned nchunk) {
  const int64_t need = (int64_t)s.ncb * s.stride;
  if (g->cap < need) {
    for (DevBuf<double> *b : {&g->Y, &g->KY, &g->GY, &g->X, &g->KX, &g->GX}) PL_HIP(b->alloc((size_t)need));
    g->cap = need;
  }
  const size_t np = (size_t)s.ncol * s.ncol * nchunk;
  if (g->part.n < np) PL_HIP(g->part.alloc(np));
  if (!g->M.p) {
    PL_HIP(g->M.alloc((size_t)2 * PL_MULTI_MAX * PL_MULTI_MAX));
    PL_HIP(g->C.alloc((size_t)PL_MULTI_MAX * PL_MULTI_MAX));
  }
  if (g->perm.n < (size_t)c->N) PL_HIP(g->perm.alloc((size_t)c->N));
  return PL_OK;
}

int launch_geom_records(pl_context *c, GeomWs *g, const double *u_dev) {
  hipLaunchKernelGGL(pl::k_geom_records, dim3(grid_for(c->B)), dim3(pl::kBlock), 0, c->stream, c->B, c->conn.p, c->rec.p, u_dev,
                     g->rec.p);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// y_j = K_g x_j (masked: P K_g x_j) for every column of the shape, one launch
inline int launch_geom_multi(pl_context *c, const GeomWs *g, const MultiShape &s, const double *x, double *y, bool masked) {
  return launch_gather_multi(c, s, pl::GeomTerm{g->rec.p}, c->fixedbits.p, x, y, masked, nullptr);
}

// M[i][j] = A_i . B_j (ncol x ncol, row-major, on the device)
int launch_gram(pl_context *c, GeomWs *g, const MultiShape &s, unsigned nchunk, const double *A, const double *Bv, double *M) {
  const int64_t n6 = c->N * 6;
  const dim3 grid(nchunk, (unsigned)(s.ncb * s.ncb));
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_gram<KB>), grid, dim3(pl::kBlock), 0, c->stream, n6, A, Bv, g->part.p, s.ncb,
                                       s.stride));
  hipLaunchKernelGGL(pl::k_multi_gram_fold, dim3((unsigned)(s.ncol * s.ncol)), dim3(pl::kBlock), 0, c->stream, (int)nchunk,
                     (const double *)g->part.p, M, s.KB, s.ncb);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// Z = Y C with C = g->C
int launch_combine(pl_context *c, GeomWs *g, const MultiShape &s, const double *Y, double *Z) {
  const int64_t n6 = c->N * 6;
  const dim3 grid(grid_stream(n6), (unsigned)s.ncb);
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_combine<KB>), grid, dim3(pl::kBlock), 0, c->stream, n6, Y,
                                       (const double *)g->C.p, Z, s.ncb, s.stride));
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// the per-strut arrays of the mode-sensitivity calls for the shape s and n_modes rows of output (quad: q of k_geom_quad too)
int geom_ws_sens(pl_context *c, GeomWs *g, const MultiShape &s, bool quad) {
  const size_t B = (size_t)c->B;
  if (quad && g->sq.n < (size_t)s.ncol * B) PL_HIP(g->sq.alloc((size_t)s.ncol * B));
  if (g->sdlam.n < (size_t)(s.n_rhs + 1) * B) PL_HIP(g->sdlam.alloc((size_t)(s.n_rhs + 1) * B));
  if (!g->scoef.p) PL_HIP(g->scoef.alloc((size_t)2 * PL_MULTI_MAX));
  return PL_OK;
}

// Q[cb][b KB + k] = phi_e^T G_b phi_e for every strut and column, one launch
template <int KB>
void launch_geom_quad_t(pl_context *c, const GeomWs *g, const MultiShape &s, const double *phi) {
  hipLaunchKernelGGL((pl::k_geom_quad<KB>), dim3(grid_for(c->B), (unsigned)s.ncb), dim3(pl::kBlock), 0, c->stream, c->B,
                     (const int32_t *)c->conn.p, (const pl::GeomRecord *)g->rec.p, phi, g->sq.p, s.stride);
}
int launch_geom_quad(pl_context *c, const GeomWs *g, const MultiShape &s, const double *phi) {
  if (s.KB == 1) launch_geom_quad_t<1>(c, g, s, phi);
  else if (s.KB == 2) launch_geom_quad_t<2>(c, g, s, phi);
  else launch_geom_quad_t<4>(c, g, s, phi);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

template <int LPN, int KB>
void launch_adjoint_load_t(pl_context *c, const GeomWs *g, const MultiShape &s, double *y) {
  const dim3 grid(grid_for(c->n_slices, pl::kBlock / pl::kWave), (unsigned)s.ncb);   // one wave per ELL slice and column block
  hipLaunchKernelGGL((pl::k_geom_adjoint_load<LPN, KB>), grid, dim3(pl::kBlock), 0, c->stream, c->N, c->B, c->slice_ptr.p,
                     c->ent.p, c->rec.p, (const double *)g->sq.p, y, s.stride);
}
template <int LPN>
void launch_adjoint_load_lpn(pl_context *c, const GeomWs *g, const MultiShape &s, double *y) {
  if (s.KB == 1) launch_adjoint_load_t<LPN, 1>(c, g, s, y);
  else if (s.KB == 2) launch_adjoint_load_t<LPN, 2>(c, g, s, y);
  else launch_adjoint_load_t<LPN, 4>(c, g, s, y);
}
// y_j = -w_j from g->sq for every column of the shape, one launch
int launch_adjoint_load(pl_context *c, const GeomWs *g, const MultiShape &s, double *y) {
  switch (c->lpn) {
    case 1: launch_adjoint_load_lpn<1>(c, g, s, y); break;
    case 2: launch_adjoint_load_lpn<2>(c, g, s, y); break;
    case 4: launch_adjoint_load_lpn<4>(c, g, s, y); break;
    case 8: launch_adjoint_load_lpn<8>(c, g, s, y); break;
    case 16: launch_adjoint_load_lpn<16>(c, g, s, y); break;
    default: return fail(PL_ERR_ARG, "lanes per node must be 1, 2, 4, 8 or 16");
  }
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// rows of dlambda/dr (dlam may be null) and their weighted sum (dsum may be null) from phi, nu, g->sq, g->M and g->scoef
template <int KB>
void launch_geom_sens_t(pl_context *c, const GeomWs *g, const MultiShape &s, const double *u, const double *phi, const double *nu,
                        double *dlam, double *dsum) {
  hipLaunchKernelGGL((pl::k_geom_sens<KB>), dim3(grid_for(c->B)), dim3(pl::kBlock), 0, c->stream, c->B, (const int32_t *)c->conn.p,
                     (const pl::GeomRecord *)g->rec.p, (const double *)c->radius.p, (const double *)c->seg_len.p,
                     (const int32_t *)c->seg_nsub.p, (const double *)c->mult.p, c->mat, u, phi, nu, (const double *)g->sq.p,
                     (const double *)g->M.p, (const double *)g->scoef.p, s.n_rhs, s.ncb, s.stride, dlam, dsum);
}
int launch_geom_sens(pl_context *c, const GeomWs *g, const MultiShape &s, const double *u, const double *phi, const double *nu,
                     double *dlam, double *dsum) {
  if (s.KB == 1) launch_geom_sens_t<1>(c, g, s, u, phi, nu, dlam, dsum);
  else if (s.KB == 2) launch_geom_sens_t<2>(c, g, s, u, phi, nu, dlam, dsum);
  else launch_geom_sens_t<4>(c, g, s, u, phi, nu, dlam, dsum);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Rayleigh-Ritz on the host, plain C++: Km = Y^T K Y, Gm = Y^T G Y (n x n, row-major, symmetrised here).  Cholesky of Km
// with diagonal pivoting; directions whose pivot is negligible against the largest diagonal entry are dropped.  The
// reduced problem L^-1 Gm L^-T is diagonalised by cyclic Jacobi.  Returns the rank r; mu[0 .. r) descending, C (n x n,
// row-major) with C^T Km C = I and C^T Gm C = diag(mu) in its first r columns, zero in the others.
// ---------------------------------------------------------------------------------------------------------
int ritz_host(int n, std::vector<double> Km, std::vector<double> Gm, std::vector<double> &mu, std::vector<double> &C) {
  auto sym = [n](std::vector<double> &A) {
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) A[i * n + j] = A[j * n + i] = 0.5 * (A[i * n + j] + A[j * n + i]);
  };
  sym(Km);
  sym(Gm);
  std::vector<int> piv(n);
  for (int i = 0; i < n; ++i) piv[i] = i;
  double dmax = 0.0;
  for (int i = 0; i < n; ++i) dmax = std::max(dmax, Km[i * n + i]);
  std::vector<double> Lm((size_t)n * n, 0.0);      // L of the permuted matrix
  int r = 0;
  for (int k = 0; k < n; ++k) {
    int best = k;
    for (int i = k + 1; i < n; ++i)
      if (Km[piv[i] * n + piv[i]] > Km[piv[best] * n + piv[best]]) best = i;
    const double p = Km[piv[best] * n + piv[best]];
    if (!(p > 1e-12 * dmax) || !(p > 0.0)) break;
    std::swap(piv[k], piv[best]);
    for (int j = 0; j < k; ++j) std::swap(Lm[k * n + j], Lm[best * n + j]);
    const double lkk = std::sqrt(p);
    Lm[k * n + k] = lkk;
    for (int i = k + 1; i < n; ++i) Lm[i * n + k] = Km[piv[i] * n + piv[k]] / lkk;
    for (int i = k + 1; i < n; ++i)
      for (int j = k + 1; j < n; ++j) Km[piv[i] * n + piv[j]] -= Lm[i * n + k] * Lm[j * n + k];
    r = k + 1;
  }
  mu.assign(n, -std::numeric_limits<double>::infinity());
  C.assign((size_t)n * n, 0.0);
  if (r == 0) return 0;
  // A = L1^-1 Gm(piv, piv) L1^-T on the leading r x r block
  std::vector<double> A((size_t)r * r), T((size_t)r * r);
  for (int j = 0; j < r; ++j)          // T = L1^-1 Gp
    for (int i = 0; i < r; ++i) {
      double v = Gm[piv[i] * n + piv[j]];
      for (int q = 0; q < i; ++q) v -= Lm[i * n + q] * T[q * r + j];
      T[i * r + j] = v / Lm[i * n + i];
    }
  for (int i = 0; i < r; ++i)          // A = T L1^-T: row i of A solves L1 a^T = T[i]^T
    for (int j = 0; j < r; ++j) {
      double v = T[i * r + j];
      for (int q = 0; q < j; ++q) v -= Lm[j * n + q] * A[i * r + q];
      A[i * r + j] = v / Lm[j * n + j];
    }
  for (int i = 0; i < r; ++i)
    for (int j = i + 1; j < r; ++j) A[i * r + j] = A[j * r + i] = 0.5 * (A[i * r + j] + A[j * r + i]);
  std::vector<double> Q((size_t)r * r, 0.0);
  for (int i = 0; i < r; ++i) Q[i * r + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) (i == j ? diag : off) += A[i * r + j] * A[i * r + j];
    if (!(off > 1e-34 * diag)) break;
    for (int p = 0; p < r - 1; ++p)
      for (int q = p + 1; q < r; ++q) {
        const double apq = A[p * r + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * r + q] - A[p * r + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < r; ++k) {
          const double akp = A[k * r + p], akq = A[k * r + q];
          A[k * r + p] = cs * akp - sn * akq;
          A[k * r + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < r; ++k) {
          const double apk = A[p * r + k], aqk = A[q * r + k];
          A[p * r + k] = cs * apk - sn * aqk;
          A[q * r + k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < r; ++k) {
          const double qkp = Q[k * r + p], qkq = Q[k * r + q];
          Q[k * r + p] = cs * qkp - sn * qkq;
          Q[k * r + q] = sn * qkp + cs * qkq;
        }
      }
  }
  std::vector<int> order(r);
  for (int i = 0; i < r; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[a * r + a] > A[b * r + b]; });
  for (int j = 0; j < r; ++j) {
    const int src = order[j];
    mu[j] = A[src * r + src];
    std::vector<double> z(r);          // L1^T z = Q[:, src]
    for (int i = r - 1; i >= 0; --i) {
      double v = Q[i * r + src];
      for (int q = i + 1; q < r; ++q) v -= Lm[q * n + i] * z[q];
      z[i] = v / Lm[i * n + i];
    }
    for (int i = 0; i < r; ++i) C[(size_t)piv[i] * n + j] = z[i];
  }
  return r;
}

}  // namespace
