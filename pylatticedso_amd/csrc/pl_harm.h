// Frequency response: the steady state under a harmonic load (pl_harm_spmv / pl_harmonic).  gfx950 only.
//
// f e^{iwt} on the free dofs of pl_set_bc (supports held at zero), K the strut operator, M the consistent mass of pl_set_mass,
// C = ray_m M + ray_k K: u e^{iwt} with
//     A(w) u = f,   A(w) = c_K K + c_M M,   c_K = 1 + i w ray_k,   c_M = i w ray_m - w^2
// A is complex SYMMETRIC (not Hermitian) and, above the first resonance, indefinite in its real part.  The solver is the
// conjugate orthogonal CG (COCG): CG with the unconjugated form x^T y in the place of the inner product, one operator
// application per iteration, Jacobi-preconditioned with the complex diagonal d = c_K diag K + c_M diag M:
//     r = f, z = r / d, p = z, rho = r^T z;   sigma = p^T A p, alpha = rho / sigma, x += alpha p, r -= alpha A p, z = r / d,
//     rho' = r^T z, beta = rho' / rho, p = z + beta p
// It has no convergence guarantee: sigma or rho may vanish on a vector that is not zero (a breakdown), and ||r|| is not
// monotone.
//
// A complex vector is a column block of two, X[cb][(6 i + d) * 2 + k] with k = 0 the real and k = 1 the imaginary part - bit
// for bit a complex128 array -, so one column block is one frequency and blockIdx.y carries the frequencies of a pass through
// every launch.  A x is ONE gather (k_gather_multi with HarmTerm).  The frequencies iterate in lock step with the freeze rule of
// pl_multi.h: a decision is taken from numbers that are final in the launch and written to the flags of the other parity.
//
// Every product and reduction here has a fixed order: the vector kernels run at most kSlots blocks per frequency, so every slot
// of a reduction scalar receives ONE block total, and a frequency's numbers do not depend on the others in its pass.
#pragma once
#include "pl_dyn.h"

namespace pl {

struct Cplx {
  double re, im;
};
__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cplx cdiv(Cplx a, Cplx b) {
  const double q = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / q, (a.im * b.re - a.re * b.im) / q};
}
// zero, or not a number: a scalar COCG cannot divide by
__device__ __forceinline__ bool cbad(Cplx a) {
  return !(fabs(a.re) <= 1.7e308 && fabs(a.im) <= 1.7e308) || (a.re == 0.0 && a.im == 0.0);
}

// y = c x for the six complex dofs of a node's row (column block of two)
__device__ __forceinline__ void rotate_row(Cplx c, const double (&x)[12], double (&y)[12]) {
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    y[2 * d] = c.re * x[2 * d] - c.im * x[2 * d + 1];
    y[2 * d + 1] = c.re * x[2 * d + 1] + c.im * x[2 * d];
  }
}

// c_K[cb] K + c_M[cb] M on complex operands in k_gather_multi (pl_multi.h), the coefficients {Re c_K, Im c_K, Re c_M, Im c_M} of
// column block cb = blockIdx.y from a device array.  K and M are real, so the operands are rotated and not the records: the
// stiffness forces of the pair c_K x, then the mass forces of the pair c_M x, into the same row; as in DynTerm one record is live
// at a time.  Column blocks of two only.
struct HarmTerm {
  static constexpr int kMaxKB = 2, kMinKB = 2;
  const Record *__restrict__ rec;
  MassTerm mass;
  const double *__restrict__ coef;   // [gridDim.y][4]
  template <int KB>
  __device__ __forceinline__ void entry(int64_t strut, bool point1, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                        double (&out)[6 * KB]) const {
    static_assert(KB == 2, "a complex vector is a column block of two");
    const double *q = coef + 4 * blockIdx.y;
    {
      const Cplx cK = {q[0], q[1]};
      double yo[12], ys[12];
      rotate_row(cK, xo, yo);
      rotate_row(cK, xs, ys);
      Record r = load_record(rec, strut);
      if (point1) r = reversed(r);
      add_tip_forces<2>(r, yo, ys, out);
    }
    {
      const Cplx cM = {q[2], q[3]};
      double yo[12], ys[12];
      rotate_row(cM, xo, yo);
      rotate_row(cM, xs, ys);
      const MassRecord r = load_mass(mass.rec, strut);
      const MassCoef c = mass_coef(r, mass.rotary);
      const double sg = point1 ? -1.0 : 1.0;                     // point1: d -> -d
      const V3 d = {sg * r.dx, sg * r.dy, sg * r.dz};
      add_mass_forces<2>(c, d, yo, ys, out);
    }
  }
  template <int KB>
  __device__ __forceinline__ void node(int64_t i, const double (&xs)[6 * KB], double (&out)[6 * KB]) const {
    static_assert(KB == 2, "a complex vector is a column block of two");
    if (mass.node_mass) {               // kernel-uniform
      const double *q = coef + 4 * blockIdx.y;
      const double nm = mass.node_mass[i];
      const Cplx c = {nm * q[2], nm * q[3]};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        out[2 * d] += c.re * xs[2 * d] - c.im * xs[2 * d + 1];
        out[2 * d + 1] += c.re * xs[2 * d + 1] + c.im * xs[2 * d];
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------------------
// COCG vector kernels: grid.x (at most kSlots blocks) strides over the 6N complex dofs, grid.y = frequency.  Reduction scalars
// per frequency: set[which][frequency][kSlots], two sets by iteration parity, as in pl_multi.h.
// ---------------------------------------------------------------------------------------------------------
enum { H_RHO_OLD = 0, H_SIGMA = 2, H_RHO_NEW = 4, H_RR = 6, H_COUNT = 7 };   // complex scalars take two rows: re, im
// status block the host downloads in one piece: [H_ST_COUNT][n_freq]; state: 0 iterating, 1 converged, 2 breakdown
enum { H_ST_RR = 0, H_ST_BB = 1, H_ST_ITER = 2, H_ST_STATE = 3, H_ST_COUNT = 4 };
enum { H_PW_FU = 0, H_PW_UKU = 2, H_PW_UMU = 3, H_PW_COUNT = 4 };

__device__ __forceinline__ Cplx load_c(const double *__restrict__ p, int64_t e) {
  const double2 a = reinterpret_cast<const double2 *>(p)[e];
  return {a.x, a.y};
}
__device__ __forceinline__ void store_c(double *__restrict__ p, int64_t e, Cplx v) {
  reinterpret_cast<double2 *>(p)[e] = {v.re, v.im};
}
__device__ __forceinline__ Cplx slots_read_c(const double *set, int which, int nf, int cb) {
  return {slots_read_v(set, which, nf, cb), slots_read_v(set, which + 1, nf, cb)};
}
// 1 / d of dof e, d = c_K diag K + c_M diag M; 0 on fixed dofs and where d vanishes
__device__ __forceinline__ Cplx harm_dinv(const double *__restrict__ diagK, const double *__restrict__ diagM, Cplx cK, Cplx cM,
                                          bool fixed, int64_t e) {
  const double k = diagK[e], m = diagM[e];
  const Cplx d = {cK.re * k + cM.re * m, cK.im * k + cM.im * m};
  if (fixed || (d.re == 0.0 && d.im == 0.0)) return {0.0, 0.0};
  return cdiv({1.0, 0.0}, d);
}

// r = P f ; z = r / d ; p = z ; x = 0 ; rho = r^T z ; bb = ||r||^2.  The load of column block cb is f + cb * fstride, [6N] complex:
// fstride = 0 gives every frequency the same load (pl_harmonic), pl_harmonic_sens gives every block its own.
__global__ __launch_bounds__(kBlock) void k_harm_init(int64_t n6, const double *__restrict__ f,
                                                      const uint8_t *__restrict__ fixedbits,
                                                      const double *__restrict__ diagK, const double *__restrict__ diagM,
                                                      const double *__restrict__ coef, double *__restrict__ x,
                                                      double *__restrict__ r, double *__restrict__ z, double *__restrict__ p,
                                                      double *__restrict__ set0, double *__restrict__ bb, int nf, int64_t stride,
                                                      int64_t fstride) {
  __shared__ double red[3][kBlock / kWave];
  const int cb = blockIdx.y;
  const size_t off = (size_t)cb * stride;
  f += (size_t)cb * fstride;
  const Cplx cK = {coef[4 * cb], coef[4 * cb + 1]}, cM = {coef[4 * cb + 2], coef[4 * cb + 3]};
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const bool fx = dof_fixed(fixedbits, e);
    Cplx rv = load_c(f, e);
    if (fx) rv = {0.0, 0.0};
    const Cplx zv = cmul(rv, harm_dinv(diagK, diagM, cK, cM, fx, e));
    const Cplx rz = cmul(rv, zv);
    s[0] += rz.re;
    s[1] += rz.im;
    s[2] += rv.re * rv.re + rv.im * rv.im;
    store_c(x + off, e, {0.0, 0.0});
    store_c(r + off, e, rv);
    store_c(z + off, e, zv);
    store_c(p + off, e, zv);
  }
  double *dst[3] = {slots_of(set0, H_RHO_OLD, nf, cb), slots_of(set0, H_RHO_OLD + 1, nf, cb), bb + (size_t)cb * kSlots};
  block_add_slots<3>(s, red, dst);
}

// One wave per frequency, after k_harm_init: ||b||^2, the stopping threshold and the flags of iteration 0 - a zero load (or one
// that is not a number) never moves: it is converged at iteration 0.
__global__ __launch_bounds__(kWave) void k_harm_begin(int nf, double rtol, const double *__restrict__ bb,
                                                      double *__restrict__ thresh, double *__restrict__ status,
                                                      int *__restrict__ flag0) {
  const int cb = blockIdx.x;
  const double b = wave_sum(bb[(size_t)cb * kSlots + threadIdx.x]);
  if (threadIdx.x == 0) {
    const bool stay = !(b > 0.0) || b > 1.7e308;
    thresh[cb] = rtol * rtol * b;
    status[H_ST_RR * nf + cb] = b;
    status[H_ST_BB * nf + cb] = b;
    status[H_ST_ITER * nf + cb] = 0.0;
    status[H_ST_STATE * nf + cb] = stay ? 1.0 : 0.0;
    flag0[cb] = stay ? 1 : 0;
  }
}

// sigma = p^T A p, unconjugated.  (The x . y slots of the gather hold Re p . Re Ap and Im p . Im Ap only: the cross terms of the
// imaginary part are not among them, and alpha needs the whole sum before the update starts.)
__global__ __launch_bounds__(kBlock) void k_harm_sigma(int64_t n6, const double *__restrict__ p, const double *__restrict__ Ap,
                                                       double *__restrict__ cur, const int *__restrict__ flag_cur, int nf,
                                                       int64_t stride) {
  __shared__ double red[2][kBlock / kWave];
  const int cb = blockIdx.y;
  if (flag_cur[cb] != 0) return;   // block-uniform: a frozen frequency
  const size_t off = (size_t)cb * stride;
  double s[2] = {0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const Cplx t = cmul(load_c(p + off, e), load_c(Ap + off, e));
    s[0] += t.re;
    s[1] += t.im;
  }
  double *dst[2] = {slots_of(cur, H_SIGMA, nf, cb), slots_of(cur, H_SIGMA + 1, nf, cb)};
  block_add_slots<2>(s, red, dst);
}

// x += alpha p ; r -= alpha Ap ; z = r / d ; rho' += r^T z ; rr += ||r||^2       alpha = rho / sigma, 0 at a breakdown
__global__ __launch_bounds__(kBlock) void k_harm_update(int64_t n6, const double *__restrict__ p, const double *__restrict__ Ap,
                                                        const uint8_t *__restrict__ fixedbits,
                                                        const double *__restrict__ diagK, const double *__restrict__ diagM,
                                                        const double *__restrict__ coef, double *__restrict__ x,
                                                        double *__restrict__ r, double *__restrict__ z, double *__restrict__ cur,
                                                        const int *__restrict__ flag_cur, int nf, int64_t stride) {
  __shared__ double red[3][kBlock / kWave];
  const int cb = blockIdx.y;
  if (flag_cur[cb] != 0) return;   // block-uniform: x and r of a frozen frequency no longer change
  const size_t off = (size_t)cb * stride;
  const Cplx cK = {coef[4 * cb], coef[4 * cb + 1]}, cM = {coef[4 * cb + 2], coef[4 * cb + 3]};
  const Cplx rho = slots_read_c(cur, H_RHO_OLD, nf, cb), sigma = slots_read_c(cur, H_SIGMA, nf, cb);
  const Cplx alpha = (cbad(rho) || cbad(sigma)) ? Cplx{0.0, 0.0} : cdiv(rho, sigma);
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const Cplx pv = load_c(p + off, e), av = load_c(Ap + off, e);
    Cplx xv = load_c(x + off, e), rv = load_c(r + off, e);
    const Cplx ap = cmul(alpha, pv), aa = cmul(alpha, av);
    xv = {xv.re + ap.re, xv.im + ap.im};
    rv = {rv.re - aa.re, rv.im - aa.im};
    const Cplx zv = cmul(rv, harm_dinv(diagK, diagM, cK, cM, dof_fixed(fixedbits, e), e));
    const Cplx rz = cmul(rv, zv);
    s[0] += rz.re;
    s[1] += rz.im;
    s[2] += rv.re * rv.re + rv.im * rv.im;
    store_c(x + off, e, xv);
    store_c(r + off, e, rv);
    store_c(z + off, e, zv);
  }
  double *dst[3] = {slots_of(cur, H_RHO_NEW, nf, cb), slots_of(cur, H_RHO_NEW + 1, nf, cb), slots_of(cur, H_RR, nf, cb)};
  block_add_slots<3>(s, red, dst);
}

// p = z + beta p (beta = rho' / rho) and the bookkeeping at the end of iteration `it`: every block takes the freeze decision of
// its frequency from numbers that are final in this launch; block 0 of the frequency records it in the flags of the OTHER
// parity, writes the status block and prepares the next scalar set.  Converged: ||r||^2 <= thresh.  Breakdown: sigma, rho or
// rho' zero or not a number while the residual is above the threshold.
__global__ __launch_bounds__(kBlock) void k_harm_direction(int64_t n6, const double *__restrict__ z, double *__restrict__ p,
                                                           const double *__restrict__ cur, double *__restrict__ nxt,
                                                           const int *__restrict__ flag_cur, int *__restrict__ flag_nxt,
                                                           const double *__restrict__ thresh, double *__restrict__ status,
                                                           int it, int nf, int64_t stride) {
  const int cb = blockIdx.y;
  if (flag_cur[cb] != 0) {   // block-uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) flag_nxt[cb] = 1;
    return;
  }
  const Cplx old = slots_read_c(cur, H_RHO_OLD, nf, cb), nw = slots_read_c(cur, H_RHO_NEW, nf, cb);
  const Cplx sigma = slots_read_c(cur, H_SIGMA, nf, cb);
  const double rr = slots_read_v(cur, H_RR, nf, cb);
  const bool conv = rr <= thresh[cb];
  const bool brk = !conv && (cbad(sigma) || cbad(old) || cbad(nw) || !(rr <= 1.7e308));
  if (blockIdx.x == 0 && threadIdx.x < kWave) {
    const int lane = threadIdx.x;
    if (lane == 0) {
      flag_nxt[cb] = (conv || brk) ? 1 : 0;
      status[H_ST_RR * nf + cb] = rr;
      status[H_ST_ITER * nf + cb] = (double)(it + 1);
      status[H_ST_STATE * nf + cb] = conv ? 1.0 : (brk ? 2.0 : 0.0);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      nxt[((size_t)(H_RHO_OLD + q) * nf + cb) * kSlots + lane] = cur[((size_t)(H_RHO_NEW + q) * nf + cb) * kSlots + lane];
      nxt[((size_t)(H_RHO_NEW + q) * nf + cb) * kSlots + lane] = 0.0;
      nxt[((size_t)(H_SIGMA + q) * nf + cb) * kSlots + lane] = 0.0;
    }
    nxt[((size_t)H_RR * nf + cb) * kSlots + lane] = 0.0;
  }
  if (conv || brk) return;   // block-uniform: frozen from the next iteration on
  const size_t off = (size_t)cb * stride;
  const Cplx beta = cdiv(nw, old);
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const Cplx zv = load_c(z + off, e), bp = cmul(beta, load_c(p + off, e));
    store_c(p + off, e, {zv.re + bp.re, zv.im + bp.im});
  }
}

// After the solve: the six complex dofs of the probed nodes (probe_slot[node] >= 0) into probe[frequency][slot][6], and the
// slots of f^T u (unconjugated), u^H K u and u^H M u (real: K and M are real symmetric) of every frequency.
__global__ __launch_bounds__(kBlock) void k_harm_epilogue(int64_t n6, const double *__restrict__ f, const double *__restrict__ u,
                                                          const double *__restrict__ Ku, const double *__restrict__ Mu,
                                                          const int32_t *__restrict__ probe_slot, int n_slot,
                                                          double *__restrict__ probe, double *__restrict__ power, int64_t stride) {
  __shared__ double red[4][kBlock / kWave];
  const int cb = blockIdx.y;
  const size_t off = (size_t)cb * stride;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const Cplx uv = load_c(u + off, e), kv = load_c(Ku + off, e), mv = load_c(Mu + off, e);
    const Cplx fu = cmul(load_c(f, e), uv);
    s[0] += fu.re;
    s[1] += fu.im;
    s[2] += uv.re * kv.re + uv.im * kv.im;
    s[3] += uv.re * mv.re + uv.im * mv.im;
    const int64_t node = e / 6;
    const int slot = probe_slot[node];
    if (slot >= 0) store_c(probe, ((int64_t)cb * n_slot + slot) * 6 + (e - 6 * node), uv);
  }
  double *dst[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = power + ((size_t)cb * H_PW_COUNT + q) * kSlots;
  block_add_slots<4>(s, red, dst);
}

}  // namespace pl

namespace {

constexpr int kHarmMaxFreq = PL_MULTI_MAX / 2;   // frequencies per pass: column blocks of two in the multi-column workspace

// one complex vector per frequency: n_freq column blocks of two
inline MultiShape harm_shape(const pl_context *c, int n_freq) {
  MultiShape s;
  s.n_rhs = 2 * n_freq;
  s.KB = 2;
  s.ncb = n_freq;
  s.ncol = 2 * n_freq;
  s.stride = c->N * 12;
  return s;
}

// grid.x of the COCG vector kernels: one block per slot at the most, so that every reduction has a fixed order
inline unsigned harm_grid(int64_t n6) { return std::min<unsigned>(grid_stream(n6), (unsigned)pl::kSlots); }

// Device data of the harmonic calls beside the multi-column workspace, owned by the handle (pl_context::harm_ws).
struct HarmWs {
  DevBuf<double> diagK, diagM;     // [6N] real
  DevBuf<double> coef;             // [kHarmMaxFreq][4]
  DevBuf<double> scal;             // [2 sets][H_COUNT][nf][kSlots] | bb [nf][kSlots] | thresh [nf] | status [H_ST_COUNT][nf]
  DevBuf<int> flags;               // [2][nf]
  DevBuf<int32_t> probe_slot;      // [N]
  DevBuf<double> probe, power;     // [nf][n_slot][6] complex, [nf][H_PW_COUNT][kSlots]
};

struct HarmScal {
  double *set[2], *bb, *thresh, *status;
  int *flag[2];
};
constexpr size_t kHarmScalPer = (size_t)(2 * pl::H_COUNT + 1) * pl::kSlots + 1 + pl::H_ST_COUNT;
inline HarmScal harm_scal(HarmWs *hw, int nf) {
  HarmScal m;
  const size_t set = (size_t)pl::H_COUNT * nf * pl::kSlots;
  m.set[0] = hw->scal.p;
  m.set[1] = m.set[0] + set;
  m.bb = m.set[1] + set;
  m.thresh = m.bb + (size_t)nf * pl::kSlots;
  m.status = m.thresh + nf;
  m.flag[0] = hw->flags.p;
  m.flag[1] = hw->flags.p + nf;
  return m;
}

int harm_ws(pl_context *c, HarmWs **out) {
  if (!c->harm_ws) c->harm_ws = std::make_shared<HarmWs>();
  HarmWs *hw = static_cast<HarmWs *>(c->harm_ws.get());
  PL_HIP(dyn_grow(hw->coef, (size_t)kHarmMaxFreq * 4));
  PL_HIP(dyn_grow(hw->diagK, (size_t)c->N * 6));
  PL_HIP(dyn_grow(hw->diagM, (size_t)c->N * 6));
  PL_HIP(dyn_grow(hw->scal, kHarmScalPer * kHarmMaxFreq));
  PL_HIP(dyn_grow(hw->flags, (size_t)2 * kHarmMaxFreq));
  PL_HIP(dyn_grow(hw->probe_slot, (size_t)c->N));
  PL_HIP(dyn_grow(hw->power, (size_t)kHarmMaxFreq * pl::H_PW_COUNT * pl::kSlots));
  *out = hw;
  return PL_OK;
}

// host complex vectors (caller numbering) -> device column blocks, ONE transfer.  a = [nf][6N] complex128, or (b_split) the real
// parts a [6N] and the imaginary parts b [6N] (null: 0) of one vector.  keep: 0 = every dof, -1 = free dofs only.
int harm_upload(pl_context *c, MultiWs *w, int nf, const double *a, const double *b, bool b_split, double *dev, int keep) {
  const size_t n6 = (size_t)c->N * 6, stride = 2 * n6;
  double *st = w->pin;
  pl::parallel_for(c->N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int cb = 0; cb < nf; ++cb)
      for (int64_t i = i0; i < i1; ++i) {
        const size_t src = 6 * (size_t)c->perm[i];
        const unsigned fb = keep ? c->h_fixedbits[(size_t)i] : 0u;
        double *row = st + (size_t)cb * stride + (size_t)12 * i;
        for (int d = 0; d < 6; ++d) {
          const bool take = !((fb >> d) & 1u);
          double re, im;
          if (b_split) {
            re = a[src + d];
            im = b ? b[src + d] : 0.0;
          } else {
            re = a[2 * ((size_t)cb * n6 + src + d)];
            im = a[2 * ((size_t)cb * n6 + src + d) + 1];
          }
          row[2 * d] = take ? re : 0.0;
          row[2 * d + 1] = take ? im : 0.0;
        }
      }
  }, 1 << 13);
  PL_HIP(hipMemcpyAsync(dev, st, (size_t)nf * stride * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));     // the staging buffer is reused by the next transfer
  return PL_OK;
}

// device column blocks -> host [nf][6N] complex128 (caller numbering)
int harm_download(pl_context *c, MultiWs *w, int nf, const double *dev, double *host) {
  const size_t n6 = (size_t)c->N * 6, stride = 2 * n6;
  double *st = w->pin;
  PL_HIP(hipMemcpyAsync(st, dev, (size_t)nf * stride * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  pl::parallel_for(c->N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int cb = 0; cb < nf; ++cb)
      for (int64_t i = i0; i < i1; ++i)
        std::memcpy(host + 2 * ((size_t)cb * n6 + 6 * (size_t)c->perm[i]), st + (size_t)cb * stride + (size_t)12 * i,
                    12 * sizeof(double));
  }, 1 << 13);
  return PL_OK;
}

// y_cb = (c_K[cb] K + c_M[cb] M) x_cb (masked: P (...)) for the frequencies of the shape, one launch; coef_dev [ncb][4]
inline int launch_harm_multi(pl_context *c, const MassWs *m, const MultiShape &s, const double *coef_dev, const double *x, double *y,
                             bool masked) {
  return launch_gather_multi(c, s, pl::HarmTerm{c->rec.p, mass_term(m), coef_dev}, c->fixedbits.p, x, y, masked, nullptr);
}

// One COCG iteration of every frequency of the pass (it selects the scalar / flag set by parity): four launches.
int harm_iteration(pl_context *c, MultiWs *w, HarmWs *hw, const MassWs *m, const MultiShape &s, const HarmScal &q, int it) {
  const int64_t n6 = c->N * 6;
  const int a = it & 1, b = a ^ 1, nf = s.ncb;
  if (int rc = launch_harm_multi(c, m, s, hw->coef.p, w->P.p, w->AP.p, true)) return rc;
  const dim3 g(harm_grid(n6), (unsigned)nf);
  hipLaunchKernelGGL(pl::k_harm_sigma, g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->P.p, (const double *)w->AP.p,
                     q.set[a], (const int *)q.flag[a], nf, s.stride);
  hipLaunchKernelGGL(pl::k_harm_update, g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->P.p, (const double *)w->AP.p,
                     (const uint8_t *)c->fixedbits.p, (const double *)hw->diagK.p, (const double *)hw->diagM.p,
                     (const double *)hw->coef.p, w->X.p, w->R.p, w->Z.p, q.set[a], (const int *)q.flag[a], nf, s.stride);
  hipLaunchKernelGGL(pl::k_harm_direction, g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->Z.p, w->P.p,
                     (const double *)q.set[a], q.set[b], (const int *)q.flag[a], q.flag[b], (const double *)q.thresh, q.status, it,
                     nf, s.stride);
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// A(w_cb) u_cb = f on the free dofs for the frequencies of the pass: hw->coef holds their coefficients, hw->diagK / diagM the
// real diagonals, w->F the load (0 on fixed dofs: one complex vector with fstride = 0, one per column block with fstride =
// s.stride); w->X receives the fields (0 on fixed dofs).
// status_host[H_ST_COUNT][ncb].  The host looks at the status block every check_every iterations; nothing else drains the stream.
int cocg_solve(pl_context *c, MultiWs *w, HarmWs *hw, const MassWs *m, const MultiShape &s, double rtol, int max_iter,
               double *status_host, int *launched, int64_t fstride = 0) {
  const int64_t n6 = c->N * 6;
  const int nf = s.ncb;
  const HarmScal q = harm_scal(hw, nf);
  PL_HIP(hipMemsetAsync(hw->scal.p, 0, kHarmScalPer * nf * sizeof(double), c->stream));
  PL_HIP(hipMemsetAsync(hw->flags.p, 0, (size_t)2 * nf * sizeof(int), c->stream));
  const dim3 g(harm_grid(n6), (unsigned)nf);
  hipLaunchKernelGGL(pl::k_harm_init, g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->F.p, (const uint8_t *)c->fixedbits.p,
                     (const double *)hw->diagK.p, (const double *)hw->diagM.p, (const double *)hw->coef.p, w->X.p, w->R.p, w->Z.p,
                     w->P.p, q.set[0], q.bb, nf, s.stride, fstride);
  hipLaunchKernelGGL(pl::k_harm_begin, dim3((unsigned)nf), dim3(pl::kWave), 0, c->stream, nf, rtol, (const double *)q.bb, q.thresh,
                     q.status, q.flag[0]);
  PL_HIP(hipGetLastError());
  const int every = c->opt.check_every > 0 ? c->opt.check_every : 16;
  const size_t st_bytes = (size_t)pl::H_ST_COUNT * nf * sizeof(double);
  auto look = [&]() -> int {     // 1: every frequency is frozen
    if (hipMemcpyAsync(status_host, q.status, st_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return -1;
    for (int j = 0; j < nf; ++j)
      if (status_host[pl::H_ST_STATE * nf + j] == 0.0) return 0;
    return 1;
  };
  int it = 0, all = look();
  while (all == 0 && it < max_iter) {
    const int stop = std::min(max_iter, it + every);
    for (; it < stop; ++it)
      if (int rc = harm_iteration(c, w, hw, m, s, q, it)) return rc;
    all = look();
  }
  if (all < 0) return fail(PL_ERR_HIP, "cocg_solve: download of the status block failed");
  *launched = it;
  return PL_OK;
}

// {Re c_K, Im c_K, Re c_M, Im c_M} of every frequency: c_K = 1 + i w ray_k, c_M = i w ray_m - w^2
inline std::vector<double> harm_coef(int n_freq, const double *omega, double ray_m, double ray_k) {
  std::vector<double> coef((size_t)4 * n_freq);
  for (int k = 0; k < n_freq; ++k) {
    const double wk = omega[k];
    coef[(size_t)4 * k] = 1.0;
    coef[(size_t)4 * k + 1] = wk * ray_k;
    coef[(size_t)4 * k + 2] = -wk * wk;
    coef[(size_t)4 * k + 3] = wk * ray_m;
  }
  return coef;
}

// The passes of pl_harmonic and pl_harmonic_sens: diag K and diag M (real, once per call), then nb frequencies per pass with
// `per` column blocks each (block q * nf + j: frequency j).  loads = null: w->F holds the one load of every block; else block
// q * nf + j reads loads[q], copied into w->F when the pass size changes.  iters / relres / status are [per][n_freq]; after the
// solves step(f0, nf) takes what the caller needs from w->X.  The labels name the PL_TIMING lines in which the two calls differ.
template <class Step>
int harm_passes(pl_context *c, MultiWs *w, HarmWs *hw, const MassWs *m, const char *who, int n_freq, const double *coef_all, int nb,
                int per, const double *const *loads, double rtol, int max_iter, const char *blocks_label,
                const char *iterations_label, int32_t *iters, double *relres, int32_t *status, int *bad,
                std::chrono::steady_clock::time_point *t_begin, Step step) {
  MultiOp op;
  op.mass = m;
  op.c_K = 1.0; op.c_M = 0.0;
  if (int rc = launch_dyn_diag(c, op, c->fixedbits.p, hw->diagK.p, nullptr)) return rc;
  op.c_K = 0.0; op.c_M = 1.0;
  if (int rc = launch_dyn_diag(c, op, c->fixedbits.p, hw->diagM.p, nullptr)) return rc;

  const bool timing = std::getenv("PL_TIMING") != nullptr;
  *t_begin = std::chrono::steady_clock::now();
  std::vector<double> coef((size_t)4 * per * nb), st((size_t)pl::H_ST_COUNT * per * nb);
  int filled = 0;
  for (int f0 = 0; f0 < n_freq; f0 += nb) {
    const int nf = std::min(nb, n_freq - f0), ncb = per * nf;
    const MultiShape s = harm_shape(c, ncb);
    if (loads && filled != nf) {
      for (int j = 0; j < ncb; ++j)
        PL_HIP(hipMemcpyAsync(w->F.p + (size_t)j * s.stride, loads[j / nf], (size_t)s.stride * sizeof(double),
                              hipMemcpyDeviceToDevice, c->stream));
      filled = nf;
    }
    for (int q = 0; q < per; ++q)
      std::memcpy(coef.data() + (size_t)4 * q * nf, coef_all + (size_t)4 * f0, (size_t)4 * nf * sizeof(double));
    PL_HIP(hipMemcpyAsync(hw->coef.p, coef.data(), (size_t)4 * ncb * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PL_HIP(hipStreamSynchronize(c->stream));         // (coef is pageable host memory, rewritten by the next pass)
    const auto t0 = std::chrono::steady_clock::now();
    int launched = 0;
    if (int rc = cocg_solve(c, w, hw, m, s, rtol, max_iter, st.data(), &launched, loads ? s.stride : 0)) return rc;
    const double ms_pass = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    long pass_iters = 0;
    for (int j = 0; j < ncb; ++j) {
      const double rr = st[(size_t)pl::H_ST_RR * ncb + j], bb = st[(size_t)pl::H_ST_BB * ncb + j];
      const int state = (int)st[(size_t)pl::H_ST_STATE * ncb + j];
      const size_t o = (size_t)(j / nf) * n_freq + f0 + (j % nf);
      iters[o] = (int32_t)st[(size_t)pl::H_ST_ITER * ncb + j];
      relres[o] = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
      status[o] = state == 1 ? 0 : (state == 2 ? 2 : 1);
      if (status[o] != 0) ++*bad;
      pass_iters += iters[o];
    }
    if (int rc = step(f0, nf)) return rc;
    if (timing) {
      timing_count(who, "pass_frequencies", nf);
      if (blocks_label) timing_count(who, blocks_label, ncb);
      timing_ms(who, "iteration_mean_host_clock", launched > 0 ? ms_pass / launched : 0.0);
      timing_mean(who, iterations_label, (double)pass_iters / ncb);
    }
  }
  return PL_OK;
}

}  // namespace
