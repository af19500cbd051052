// Several right-hand sides on ONE operator in one PCG pass (pl_spmv_multi / pl_solve_multi / pl_schur_block).
//
// Scope (enforced with PL_ERR_STATE by the entry points): single-GPU FEM handles (opkind == 0, no pl_dist_init), fp64,
// Jacobi-preconditioned CG from x0 = 0.  The handle's multi-level / dense preconditioner, node elimination and warm start
// are ignored; its single-column state (x, usol, warm-start history, `last` statistics, the vectors of pl_solve) is not
// touched - everything here lives in a workspace of its own - so a pl_solve after a multi call behaves exactly as before.
// Periodic constraints of pl_set_periodic are honoured (z and p averaged per group, as pcg_solve does).
//
// Device layout: the columns are cut into column blocks of KB in {1, 2, 4}; inside a block the column index is fastest,
//     X[cb][(6 i + d) * KB + k]            (node i, dof d, column cb * KB + k)
// so one node's row is 6 KB consecutive doubles, read with 16-byte loads, and one strut record serves KB operand pairs.
// Every kernel takes the column block from blockIdx.y: ONE launch carries all columns, whatever their number.
//
// Freeze rule: all columns iterate in lock step.  A column that has met ||r|| <= rtol ||b||, or whose p^T K p is not
// positive (NaN included), is frozen: alpha = beta = 0 from then on, its x and r no longer change.  The decision of
// iteration i is taken by k_multi_direction from the reduction scalars every block can see and written to the flag set of
// the OTHER parity, which only later launches read.
#pragma once
#include <memory>

#include "pl_solver.h"

namespace pl {

enum { M_RZ_OLD = 0, M_PAP = 1, M_RZ_NEW = 2, M_RR = 3, M_COUNT = 4 };
// status block the host downloads in one piece: [M_ST_COUNT][ncol]
enum { M_ST_RR = 0, M_ST_BB = 1, M_ST_ITER = 2, M_ST_FROZEN = 3, M_ST_COUNT = 4 };

// one node's row of a column block: v[d * KB + k]
template <int KB>
__device__ __forceinline__ void load_row(const double *__restrict__ x, int64_t node, double (&v)[6 * KB]) {
  const double2 *q = reinterpret_cast<const double2 *>(x + 6 * KB * node);
#pragma unroll
  for (int j = 0; j < 3 * KB; ++j) {
    const double2 a = q[j];
    v[2 * j] = a.x;
    v[2 * j + 1] = a.y;
  }
}
template <int KB>
__device__ __forceinline__ void column_of(const double (&v)[6 * KB], int k, V3 &u, V3 &t) {
  u = {v[0 * KB + k], v[1 * KB + k], v[2 * KB + k]};
  t = {v[3 * KB + k], v[4 * KB + k], v[5 * KB + k]};
}
// the KB values of one dof
template <int KB>
__device__ __forceinline__ void load_cols(const double *__restrict__ p, int64_t e, double (&v)[KB]) {
  if constexpr (KB == 1) {
    v[0] = p[e];
  } else {
    const double2 *q = reinterpret_cast<const double2 *>(p + KB * e);
#pragma unroll
    for (int j = 0; j < KB / 2; ++j) {
      const double2 a = q[j];
      v[2 * j] = a.x;
      v[2 * j + 1] = a.y;
    }
  }
}
template <int KB>
__device__ __forceinline__ void store_cols(double *__restrict__ p, int64_t e, const double (&v)[KB]) {
  if constexpr (KB == 1) {
    p[e] = v[0];
  } else {
    double2 *q = reinterpret_cast<double2 *>(p + KB * e);
#pragma unroll
    for (int j = 0; j < KB / 2; ++j) q[j] = {v[2 * j], v[2 * j + 1]};
  }
}
__device__ __forceinline__ bool dof_fixed(const uint8_t *__restrict__ fixedbits, int64_t e) {
  const int64_t node = e / 6;
  return (fixedbits[node] >> (int)(e - 6 * node)) & 1u;
}
// NV block totals into the slot arrays dst[v] (thread 0 adds); all threads of the block must call
template <int NV>
__device__ __forceinline__ void block_add_slots(double (&v)[NV], double (*smem)[kBlock / kWave], double *(&dst)[NV]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double t = wave_sum(v[q]);
    if (lane == 0) smem[q][w] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < kBlock / kWave; ++i) t += smem[q][i];
      unsafeAtomicAdd(dst[q] + (blockIdx.x & (kSlots - 1)), t);
    }
  }
}
__device__ __forceinline__ double *slots_of(double *set, int which, int ncol, int col) {
  return set + ((size_t)which * ncol + col) * kSlots;
}
__device__ __forceinline__ double slots_read(const double *set, int which, int ncol, int col) {
  const double v = set[((size_t)which * ncol + col) * kSlots + (threadIdx.x & 63)];
  return wave_sum(v);
}

// The same total from a butterfly of lane exchanges: it stays in vector registers (wave_sum hands its result over in
// scalar registers; k_multi_direction reads 4 KB totals at once and would spill them)
__device__ __forceinline__ double slots_read_v(const double *set, int which, int ncol, int col) {
  double v = set[((size_t)which * ncol + col) * kSlots + (threadIdx.x & 63)];
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------
// y_k = A x_k (MASK: P A x_k, x_k assumed 0 on fixed dofs) for the KB columns of column block blockIdx.y, A a sum of strut
// elements chosen by `term`: the per-node gather of k_spmv_gather (same lane mapping, same sliced ELL, same order of the sum
// over a node's struts and the same lpn_sum, so with the stiffness term every column is what the single-column kernel
// gives).  No atomics in the product, and every sum has a fixed order: equal inputs give equal bits.
// dot_out != null: x_k . y_k is added to dot_out[(cb KB + k) * kSlots + slot].
//
// A term is a small struct passed by value (its record pointers and scalars) with
//     entry<KB>(strut, point1, xo, xs, out)   one ELL entry: load the strut's record ONCE, orient it for point1 (this node is
//                                             the strut's point1), add the forces of the KB columns on this node to out;
//                                             xo is the row of the node at the other end, xs this node's own
//     node<KB>(i, xs, out)                    once per live node, after the sum over its lanes and before the mask
//     kMaxKB                                  the widest column block the term is built for
// K: StiffTerm below, K_g: GeomTerm (pl_geom.h), M: MassTerm (pl_mass.h), c_K K + c_M M: DynTerm (pl_dyn.h).
// ---------------------------------------------------------------------------------------------------------
template <int LPN, int KB, bool MASK, class Term>
__global__ __launch_bounds__(kBlock) void k_gather_multi(int64_t N, const int64_t *__restrict__ slice_ptr,
                                                         const int2 *__restrict__ ent, const Term term,
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
        double xo[6 * KB];
        load_row<KB>(x, (int64_t)e.x, xo);
        term.template entry<KB>((int64_t)(e.y & 0x7fffffff), e.y < 0, xo, xs, out);
      }
    }
#pragma unroll
    for (int q = 0; q < 6 * KB; ++q) out[q] = lpn_sum<LPN>(out[q]);
    if (live) {
      term.template node<KB>(i, xs, out);   // every lane of the node holds the whole row by now
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

// the force f and moment m of one entry on this node, column k, into the node's row
template <int KB>
__device__ __forceinline__ void add_column(double (&out)[6 * KB], int k, V3 f, V3 m) {
  out[0 * KB + k] += f.x; out[1 * KB + k] += f.y; out[2 * KB + k] += f.z;
  out[3 * KB + k] += m.x; out[4 * KB + k] += m.y; out[5 * KB + k] += m.z;
}

// the stiffness forces of the oriented record r for the KB columns (tip_force, pl_device.h)
template <int KB>
__device__ __forceinline__ void add_tip_forces(const Record &r, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                               double (&out)[6 * KB]) {
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    V3 uo, to, us, ts, f, m;
    column_of<KB>(xo, k, uo, to);
    column_of<KB>(xs, k, us, ts);
    tip_force(r, uo, to, us, ts, f, m);
    add_column<KB>(out, k, f, m);
  }
}

// K: the condensed strut record, reversed for a strut's point1
struct StiffTerm {
  static constexpr int kMaxKB = 4;
  const Record *__restrict__ rec;
  template <int KB>
  __device__ __forceinline__ void entry(int64_t strut, bool point1, const double (&xo)[6 * KB], const double (&xs)[6 * KB],
                                        double (&out)[6 * KB]) const {
    Record r = load_record(rec, strut);
    if (point1) r = reversed(r);
    add_tip_forces<KB>(r, xo, xs, out);
  }
  template <int KB>
  __device__ __forceinline__ void node(int64_t, const double (&)[6 * KB], double (&)[6 * KB]) const {}
};

// ---------------------------------------------------------------------------------------------------------
// Vector kernels: grid.x strides over the 6N dofs, grid.y = column block; a thread handles the KB columns of a dof.
// Reduction scalars per column: set[which][column][kSlots], two sets by iteration parity (as k_pcg_direction).
// ---------------------------------------------------------------------------------------------------------
// r = P (f - K ubar) ; z = dinv r ; p = z ; x = 0 ; rz_old = r.z ; bb = r.r        (f == null: zero loads)
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_init(int64_t n6, const double *__restrict__ f,
                                                       const double *__restrict__ Kubar,
                                                       const uint8_t *__restrict__ fixedbits,
                                                       const double *__restrict__ dinv, double *__restrict__ x,
                                                       double *__restrict__ r, double *__restrict__ z,
                                                       double *__restrict__ p, double *__restrict__ set0,
                                                       double *__restrict__ bb, int ncol, int64_t stride) {
  __shared__ double red[2 * KB][kBlock / kWave];
  const int cb = blockIdx.y;
  const size_t off = (size_t)cb * stride;
  double s[2 * KB];
#pragma unroll
  for (int q = 0; q < 2 * KB; ++q) s[q] = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const bool fx = dof_fixed(fixedbits, e);
    const double dv = dinv[e];
    double fv[KB], kv[KB], rv[KB], zv[KB], zero[KB];
    load_cols<KB>(Kubar + off, e, kv);
    if (f) load_cols<KB>(f + off, e, fv);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      rv[k] = fx ? 0.0 : ((f ? fv[k] : 0.0) - kv[k]);
      zv[k] = dv * rv[k];
      zero[k] = 0.0;
      s[k] += rv[k] * zv[k];
      s[KB + k] += rv[k] * rv[k];
    }
    store_cols<KB>(x + off, e, zero);
    store_cols<KB>(r + off, e, rv);
    store_cols<KB>(z + off, e, zv);
    store_cols<KB>(p + off, e, zv);
  }
  double *dst[2 * KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    dst[k] = slots_of(set0, M_RZ_OLD, ncol, cb * KB + k);
    dst[KB + k] = bb + (size_t)(cb * KB + k) * kSlots;
  }
  block_add_slots<2 * KB>(s, red, dst);
}

// One wave per column, after k_multi_init: ||b||^2, the stopping threshold, and the flags of iteration 0 - a column with
// b = 0 (or a b that is not a number) never moves: it is converged at iteration 0 and returns its lifting.
__global__ __launch_bounds__(kWave) void k_multi_begin(int ncol, double rtol, const double *__restrict__ bb,
                                                       double *__restrict__ thresh, double *__restrict__ status,
                                                       int *__restrict__ flag0) {
  const int col = blockIdx.x;
  const double b = wave_sum(bb[(size_t)col * kSlots + threadIdx.x]);
  if (threadIdx.x == 0) {
    const bool stay = !(b > 0.0) || b > 1.7e308;
    thresh[col] = rtol * rtol * b;
    status[M_ST_RR * ncol + col] = b;
    status[M_ST_BB * ncol + col] = b;
    status[M_ST_ITER * ncol + col] = 0.0;
    status[M_ST_FROZEN * ncol + col] = stay ? 1.0 : 0.0;
    flag0[col] = stay ? 1 : 0;
  }
}

// x += alpha p ; r -= alpha Ap ; z = dinv r ; rz_new += r.z ; rr += r.r       alpha = rz_old / pAp, 0 on a frozen column
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_update(int64_t n6, const double *__restrict__ p,
                                                         const double *__restrict__ Ap, const double *__restrict__ dinv,
                                                         double *__restrict__ x, double *__restrict__ r,
                                                         double *__restrict__ z, double *__restrict__ cur,
                                                         const int *__restrict__ flag_cur, int ncol, int64_t stride) {
  __shared__ double red[2 * KB][kBlock / kWave];
  const int cb = blockIdx.y;
  const size_t off = (size_t)cb * stride;
  double alpha[KB], s[2 * KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int col = cb * KB + k;
    const double pap = slots_read(cur, M_PAP, ncol, col), old = slots_read(cur, M_RZ_OLD, ncol, col);
    alpha[k] = (flag_cur[col] != 0 || !(pap > 0.0)) ? 0.0 : old / pap;
    s[k] = 0.0;
    s[KB + k] = 0.0;
  }
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    const double dv = dinv[e];
    double pv[KB], av[KB], xv[KB], rv[KB], zv[KB];
    load_cols<KB>(p + off, e, pv);
    load_cols<KB>(Ap + off, e, av);
    load_cols<KB>(x + off, e, xv);
    load_cols<KB>(r + off, e, rv);
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      xv[k] += alpha[k] * pv[k];
      rv[k] -= alpha[k] * av[k];
      zv[k] = dv * rv[k];
      s[k] += rv[k] * zv[k];
      s[KB + k] += rv[k] * rv[k];
    }
    store_cols<KB>(x + off, e, xv);
    store_cols<KB>(r + off, e, rv);
    store_cols<KB>(z + off, e, zv);
  }
  double *dst[2 * KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    dst[k] = slots_of(cur, M_RZ_NEW, ncol, cb * KB + k);
    dst[KB + k] = slots_of(cur, M_RR, ncol, cb * KB + k);
  }
  block_add_slots<2 * KB>(s, red, dst);
}

// p = z + beta p (beta = rz_new / rz_old, 0 on a frozen column) and the bookkeeping at the end of iteration `it`: every
// block takes the freeze decision of its columns from numbers that are final in this launch (the flags of this parity, the
// reduction scalars of the update and K*p launches before it); block 0 of the column block records it in the flags of the
// OTHER parity - read by the next iteration's launches only -, writes the status block and prepares the next scalar set.
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_direction(int64_t n6, const double *__restrict__ z, double *__restrict__ p,
                                                            const double *__restrict__ cur, double *__restrict__ nxt,
                                                            const int *__restrict__ flag_cur, int *__restrict__ flag_nxt,
                                                            const double *__restrict__ thresh, double *__restrict__ status,
                                                            int it, int ncol, int64_t stride) {
  const int cb = blockIdx.y;
  const size_t off = (size_t)cb * stride;
  double beta[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int col = cb * KB + k;
    const double old = slots_read_v(cur, M_RZ_OLD, ncol, col), nw = slots_read_v(cur, M_RZ_NEW, ncol, col);
    const double rr = slots_read_v(cur, M_RR, ncol, col), pap = slots_read_v(cur, M_PAP, ncol, col);
    const bool was = flag_cur[col] != 0;
    const bool now = was || rr <= thresh[col] || !(pap > 0.0) || !(rr == rr);
    beta[k] = (now || old == 0.0) ? 0.0 : nw / old;
    if (blockIdx.x == 0 && threadIdx.x < kWave) {
      const int lane = threadIdx.x;
      if (lane == 0) {
        flag_nxt[col] = now ? 1 : 0;
        if (!was) {
          status[M_ST_RR * ncol + col] = rr;
          status[M_ST_ITER * ncol + col] = (double)(it + 1);
          status[M_ST_FROZEN * ncol + col] = now ? 1.0 : 0.0;
        }
      }
      const size_t o_old = ((size_t)M_RZ_OLD * ncol + col) * kSlots + lane, o_new = ((size_t)M_RZ_NEW * ncol + col) * kSlots + lane;
      nxt[o_old] = cur[o_new];
      nxt[o_new] = 0.0;
      nxt[((size_t)M_RR * ncol + col) * kSlots + lane] = 0.0;
      nxt[((size_t)M_PAP * ncol + col) * kSlots + lane] = 0.0;
    }
  }
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    double zv[KB], pv[KB];
    load_cols<KB>(z + off, e, zv);
    load_cols<KB>(p + off, e, pv);
#pragma unroll
    for (int k = 0; k < KB; ++k) pv[k] = zv[k] + beta[k] * pv[k];
    store_cols<KB>(p + off, e, pv);
  }
}

// u = fixed ? ubar : x
template <int KB>
__global__ __launch_bounds__(kBlock) void k_multi_compose(int64_t n6, const uint8_t *__restrict__ fixedbits,
                                                          const double *__restrict__ ubar, const double *__restrict__ x,
                                                          double *__restrict__ u, int64_t stride) {
  const size_t off = (size_t)blockIdx.y * stride;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n6; e += (int64_t)gridDim.x * kBlock) {
    double v[KB];
    if (dof_fixed(fixedbits, e)) load_cols<KB>(ubar + off, e, v);
    else load_cols<KB>(x + off, e, v);
    store_cols<KB>(u + off, e, v);
  }
}

// v <- Q v per column (pl_set_periodic): one thread per (group, dof, column)
__global__ __launch_bounds__(kBlock) void k_multi_periodic_average(int64_t n_groups, const int32_t *__restrict__ gptr,
                                                                   const int32_t *__restrict__ gnodes, double *__restrict__ v,
                                                                   int KB, int64_t stride) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 6 * n_groups * KB) return;
  v += (size_t)blockIdx.y * stride;
  const int64_t g = t / (6 * KB);
  const int dk = (int)(t - 6 * KB * g);     // d * KB + k
  const int32_t b = gptr[g], e = gptr[g + 1];
  double s = 0.0;
  for (int32_t q = b; q < e; ++q) s += v[(int64_t)6 * KB * gnodes[q] + dk];
  s /= (double)(e - b);
  for (int32_t q = b; q < e; ++q) v[(int64_t)6 * KB * gnodes[q] + dk] = s;
}

// pl_schur_block: the unit boundary displacements of columns j0 .. j0 + n - 1 (ubar zeroed by the caller); column j has
// a 1 on dof (j0 + j) % 6 of boundary node (j0 + j) / 6
__global__ __launch_bounds__(kBlock) void k_multi_unit_ubar(int n, int j0, const int32_t *__restrict__ bnodes, double *__restrict__ ubar,
                                                            int KB, int64_t stride) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int dof = j0 + j;
  ubar[(size_t)(j / KB) * stride + ((int64_t)6 * bnodes[dof / 6] + dof % 6) * KB + (j % KB)] = 1.0;
}
// ... and the contraction of the reactions R_j = K u_j to S[i][j0 + j] = R_j[boundary dof i]
__global__ __launch_bounds__(kBlock) void k_multi_schur_rows(int m, int n, int j0, const int32_t *__restrict__ bnodes,
                                                             const double *__restrict__ R, double *__restrict__ S, int KB,
                                                             int64_t stride) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (int64_t)m * n) return;
  const int i = (int)(t / n), j = (int)(t - (int64_t)i * n);
  S[(size_t)i * m + j0 + j] = R[(size_t)(j / KB) * stride + ((int64_t)6 * bnodes[i / 6] + i % 6) * KB + (j % KB)];
}

}  // namespace pl

namespace {

// Workspace of the multi-column calls, owned by the handle (pl_context::multi_ws), grown on demand.
struct MultiWs {
  int64_t cap = 0;                 // doubles per vector
  DevBuf<double> X, R, Z, P, AP, KU, F, UB, U;
  DevBuf<double> diag, dinv;       // Jacobi inverse for the mask of the running call
  DevBuf<uint8_t> fixedbits;       // pl_schur_block: the boundary mask
  DevBuf<int32_t> bnodes;
  DevBuf<double> S;
  DevBuf<double> scal;             // [2 sets][M_COUNT][ncol][kSlots] | bb [ncol][kSlots] | thresh [ncol] | status [M_ST_COUNT][ncol]
  DevBuf<int> flags;               // [2][ncol]
  int scal_cols = 0;
  double *pin = nullptr;           // pinned staging of the k-column transfers
  size_t pin_n = 0;
  ~MultiWs() {
    if (pin) (void)hipHostFree(pin);
  }
};

// pl_schur_block(block = 0): columns per pass
constexpr int kSchurBlockDefault = 64;   // the measured best (profiles/r08_solve_multi.txt)

struct MultiShape {
  int n_rhs, KB, ncb, ncol;        // ncol = ncb * KB >= n_rhs (the padding columns are zero right-hand sides)
  int64_t stride;                  // 6 N KB doubles per column block
};

inline MultiShape multi_shape(const pl_context *c, int n_rhs) {
  MultiShape s;
  s.n_rhs = n_rhs;
  s.KB = n_rhs >= 3 ? 4 : n_rhs;
  s.ncb = (n_rhs + s.KB - 1) / s.KB;
  s.ncol = s.ncb * s.KB;
  s.stride = c->N * 6 * s.KB;
  return s;
}

int multi_ws(pl_context *c, const MultiShape &s, bool solver, MultiWs **out) {
  if (!c->multi_ws) c->multi_ws = std::make_shared<MultiWs>();
  MultiWs *w = static_cast<MultiWs *>(c->multi_ws.get());
  const int64_t need = (int64_t)s.ncb * s.stride;
  if (w->cap < need) {
    for (DevBuf<double> *b : {&w->X, &w->R, &w->Z, &w->P, &w->AP, &w->KU, &w->F, &w->UB, &w->U}) b->release();
    w->cap = need;
  }
  for (DevBuf<double> *b : {&w->F, &w->U})
    if (!b->p) PL_HIP(b->alloc((size_t)w->cap));
  if (solver) {
    for (DevBuf<double> *b : {&w->X, &w->R, &w->Z, &w->P, &w->AP, &w->KU, &w->UB})
      if (!b->p) PL_HIP(b->alloc((size_t)w->cap));
    if (!w->diag.p) {
      PL_HIP(w->diag.alloc((size_t)c->N * 6));
      PL_HIP(w->dinv.alloc((size_t)c->N * 6));
    }
    if (w->scal_cols < s.ncol) {
      const size_t per = (size_t)(2 * pl::M_COUNT + 1) * pl::kSlots + 1 + pl::M_ST_COUNT;
      PL_HIP(w->scal.alloc(per * PL_MULTI_MAX));
      PL_HIP(w->flags.alloc((size_t)2 * PL_MULTI_MAX));
      w->scal_cols = PL_MULTI_MAX;
    }
  }
  if (w->pin_n < (size_t)need) {
    if (w->pin) (void)hipHostFree(w->pin);
    w->pin = nullptr;
    w->pin_n = 0;
    void *p = nullptr;
    PL_HIP(hipHostMalloc(&p, (size_t)need * sizeof(double), hipHostMallocDefault));
    w->pin = static_cast<double *>(p);
    w->pin_n = (size_t)need;
  }
  *out = w;
  return PL_OK;
}

// host [n_rhs][6N] (caller numbering) -> device column blocks, ONE transfer.  keep: 0 = every dof, 1 = fixed dofs only (the
// others 0: prescribed values), -1 = free dofs only (operand of the masked product).  host == null: zeros.
int multi_upload(pl_context *c, MultiWs *w, const MultiShape &s, const double *host, double *dev, int keep) {
  const size_t bytes = (size_t)s.ncb * s.stride * sizeof(double);
  if (!host) {
    PL_HIP(hipMemsetAsync(dev, 0, bytes, c->stream));
    return PL_OK;
  }
  const size_t n6 = (size_t)c->N * 6;
  double *st = w->pin;
  const int KB = s.KB;
  pl::parallel_for(c->N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int cb = 0; cb < s.ncb; ++cb)
      for (int64_t i = i0; i < i1; ++i) {
        const size_t src = 6 * (size_t)c->perm[i];
        const unsigned fb = keep ? c->h_fixedbits[(size_t)i] : 0u;
        double *row = st + (size_t)cb * s.stride + (size_t)6 * KB * i;
        for (int d = 0; d < 6; ++d) {
          const bool fx = (fb >> d) & 1u;
          const bool take = keep == 0 || (keep > 0 ? fx : !fx);
          for (int k = 0; k < KB; ++k) {
            const int col = cb * KB + k;
            row[d * KB + k] = (take && col < s.n_rhs) ? host[(size_t)col * n6 + src + d] : 0.0;
          }
        }
      }
  }, 1 << 13);
  PL_HIP(hipMemcpyAsync(dev, st, bytes, hipMemcpyHostToDevice, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));     // the staging buffer is reused by the next transfer
  return PL_OK;
}

int multi_download(pl_context *c, MultiWs *w, const MultiShape &s, const double *dev, double *host) {
  const size_t bytes = (size_t)s.ncb * s.stride * sizeof(double);
  const size_t n6 = (size_t)c->N * 6;
  double *st = w->pin;
  PL_HIP(hipMemcpyAsync(st, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  PL_HIP(hipStreamSynchronize(c->stream));
  const int KB = s.KB;
  pl::parallel_for(c->N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int col = 0; col < s.n_rhs; ++col) {
      const int cb = col / KB, k = col % KB;
      for (int64_t i = i0; i < i1; ++i) {
        const double *row = st + (size_t)cb * s.stride + (size_t)6 * KB * i;
        double *dst = host + (size_t)col * n6 + 6 * (size_t)c->perm[i];
        for (int d = 0; d < 6; ++d) dst[d] = row[d * KB + k];
      }
    }
  }, 1 << 13);
  return PL_OK;
}

// y_j = A x_j (masked: P A x_j), A the operator of `term`, for every column of the shape: one launch of k_gather_multi at the
// handle's lanes per node, the shape's column block and the mask.  A column block wider than the term is built for is an
// error: there is no other path.
// the narrowest column block a term is built for: Term::kMinKB where it has one (HarmTerm, pl_harm.h), 1 otherwise
template <class Term, class = void>
struct term_min_kb : std::integral_constant<int, 1> {};
template <class Term>
struct term_min_kb<Term, std::void_t<decltype(Term::kMinKB)>> : std::integral_constant<int, Term::kMinKB> {};

template <class Term>
int launch_gather_multi(pl_context *c, const MultiShape &s, Term term, const uint8_t *fixedbits, const double *x, double *y,
                        bool masked, double *dot_dev) {
  constexpr int kMinKB = term_min_kb<Term>::value;
  if (s.KB > Term::kMaxKB || s.KB < kMinKB)
    return fail(PL_ERR_ARG, "the product is not built for column blocks of " + std::to_string(s.KB));
  const dim3 g(grid_for(c->n_slices, pl::kBlock / pl::kWave), (unsigned)s.ncb);   // one wave per ELL slice and column block
  auto go = [&](auto lpn, auto kb) {
    constexpr int LPN = decltype(lpn)::value, KB = decltype(kb)::value;
    if constexpr (KB <= Term::kMaxKB && KB >= term_min_kb<Term>::value) {
      const auto kernel = masked ? pl::k_gather_multi<LPN, KB, true, Term> : pl::k_gather_multi<LPN, KB, false, Term>;
      hipLaunchKernelGGL(kernel, g, dim3(pl::kBlock), 0, c->stream, c->N, (const int64_t *)c->slice_ptr.p, (const int2 *)c->ent.p,
                         term, fixedbits, x, y, dot_dev, s.stride);
    }
  };
  auto at = [&](auto lpn) {
    if (s.KB == 1) go(lpn, std::integral_constant<int, 1>());
    else if (s.KB == 2) go(lpn, std::integral_constant<int, 2>());
    else go(lpn, std::integral_constant<int, 4>());
  };
  switch (c->lpn) {
    case 1: at(std::integral_constant<int, 1>()); break;
    case 2: at(std::integral_constant<int, 2>()); break;
    case 4: at(std::integral_constant<int, 4>()); break;
    case 8: at(std::integral_constant<int, 8>()); break;
    case 16: at(std::integral_constant<int, 16>()); break;
    default: return fail(PL_ERR_ARG, "lanes per node must be 1, 2, 4, 8 or 16");
  }
  PL_HIP(hipGetLastError());
  return PL_OK;
}
// y_j = K x_j (masked: P K x_j)
inline int launch_spmv_multi(pl_context *c, const MultiShape &s, const uint8_t *fixedbits, const double *x, double *y, bool masked,
                             double *dot_dev) {
  return launch_gather_multi(c, s, pl::StiffTerm{c->rec.p}, fixedbits, x, y, masked, dot_dev);
}

inline void multi_periodic_average(pl_context *c, const MultiShape &s, double *v) {
  if (c->n_per_groups > 0)
    hipLaunchKernelGGL(pl::k_multi_periodic_average, dim3(grid_for(6 * c->n_per_groups * s.KB), (unsigned)s.ncb),
                       dim3(pl::kBlock), 0, c->stream, c->n_per_groups, c->per_ptr.p, c->per_nodes.p, v, s.KB, s.stride);
}

struct MultiScal {
  double *set[2], *bb, *thresh, *status;
  int *flag[2];
};
inline MultiScal multi_scal(MultiWs *w, int ncol) {
  MultiScal m;
  const size_t set = (size_t)pl::M_COUNT * ncol * pl::kSlots;
  m.set[0] = w->scal.p;
  m.set[1] = m.set[0] + set;
  m.bb = m.set[1] + set;
  m.thresh = m.bb + (size_t)ncol * pl::kSlots;
  m.status = m.thresh + ncol;
  m.flag[0] = w->flags.p;
  m.flag[1] = w->flags.p + ncol;
  return m;
}

// The SPD operator the k-column PCG works on: c_K K + c_M M (pl_dyn.h).  The default is K alone, applied and preconditioned by
// the launches of this file; any other operator needs the mass data of pl_set_mass and goes through the fused kernels.
struct MassWs;
struct MultiOp {
  double c_K = 1.0, c_M = 0.0;
  const MassWs *mass = nullptr;
  bool plain() const { return mass == nullptr; }
};
// (pl_dyn.h)
int launch_dyn_multi(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x, double *y,
                     bool masked, double *dot_dev);
int launch_dyn_diag(pl_context *c, const MultiOp &op, const uint8_t *fixedbits, double *diag, double *dinv);
// y_j = A x_j for the operator of the running solve
inline int multi_apply(pl_context *c, const MultiOp &op, const MultiShape &s, const uint8_t *fixedbits, const double *x, double *y,
                       bool masked, double *dot_dev) {
  return op.plain() ? launch_spmv_multi(c, s, fixedbits, x, y, masked, dot_dev)
                    : launch_dyn_multi(c, op, s, fixedbits, x, y, masked, dot_dev);
}

#define PL_MULTI_KB(KBV, CALL)                         \
  do {                                                 \
    if ((KBV) == 1) { constexpr int KB = 1; CALL; }    \
    else if ((KBV) == 2) { constexpr int KB = 2; CALL; } \
    else { constexpr int KB = 4; CALL; }               \
  } while (0)

// One iteration of the k-column Jacobi PCG (it selects the scalar / flag set by parity): four launches, whatever ncol.
int multi_iteration(pl_context *c, MultiWs *w, const MultiShape &s, const MultiScal &m, const uint8_t *fixedbits, int it,
                    const MultiOp &op = MultiOp()) {
  const int64_t n6 = c->N * 6;
  const int a = it & 1, b = a ^ 1;
  int rc = multi_apply(c, op, s, fixedbits, w->P.p, w->AP.p, true, m.set[a] + (size_t)pl::M_PAP * s.ncol * pl::kSlots);
  if (rc) return rc;
  multi_periodic_average(c, s, w->AP.p);   // the operator is Q K Q; p.Kp above is already p.QKQp (p = Q p)
  const dim3 g(grid_stream(n6), (unsigned)s.ncb);
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_update<KB>), g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->P.p,
                                       (const double *)w->AP.p, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, m.set[a],
                                       (const int *)m.flag[a], s.ncol, s.stride));
  multi_periodic_average(c, s, w->Z.p);    // z = Q D^-1 r (r.z was summed with the un-averaged D^-1 r: the same number)
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_direction<KB>), g, dim3(pl::kBlock), 0, c->stream, n6, (const double *)w->Z.p,
                                       w->P.p, (const double *)m.set[a], m.set[b], (const int *)m.flag[a], m.flag[b],
                                       (const double *)m.thresh, m.status, it, s.ncol, s.stride));
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// Jacobi diagonal and inverse for `fixedbits` into the workspace (the handle's own dinv belongs to its own preconditioner)
int multi_diag(pl_context *c, MultiWs *w, const uint8_t *fixedbits, const MultiOp &op = MultiOp()) {
  if (!op.plain()) return launch_dyn_diag(c, op, fixedbits, w->diag.p, w->dinv.p);
  const unsigned g = grid_for(c->n_slices, pl::kBlock / pl::kWave);
#define PL_D(L)                                                                                                        \
  hipLaunchKernelGGL((pl::k_diag_gather<L>), dim3(g), dim3(pl::kBlock), 0, c->stream, c->N, c->slice_ptr.p, c->ent.p, \
                     c->rec.p, fixedbits, w->diag.p, w->dinv.p)
  switch (c->lpn) { case 1: PL_D(1); break; case 2: PL_D(2); break; case 4: PL_D(4); break; case 8: PL_D(8); break;
                    default: PL_D(16); }
#undef PL_D
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// K u_j = f_j (with `op`: (c_K K + c_M M) u_j = f_j) on the free dofs of `fixedbits`, u_j = ubar_j on the others: w->UB (zero on
// free dofs) and w->F (f_dev == null: zero loads) hold the data in column blocks, w->U receives the full fields.  status_host[M_ST_COUNT][ncol] gets ||r||^2,
// ||b||^2, iterations and the frozen flag of every column.  The host looks at the status block every check_every
// iterations in one small download; nothing else drains the stream.
int pcg_solve_multi(pl_context *c, MultiWs *w, const MultiShape &s, const uint8_t *fixedbits, const double *f_dev, double rtol,
                    int max_iter, double *status_host, const MultiOp &op = MultiOp()) {
  const int64_t n6 = c->N * 6;
  const MultiScal m = multi_scal(w, s.ncol);
  const size_t scal_bytes = ((size_t)(2 * pl::M_COUNT + 1) * pl::kSlots + 1 + pl::M_ST_COUNT) * s.ncol * sizeof(double);
  PL_HIP(hipMemsetAsync(w->scal.p, 0, scal_bytes, c->stream));
  PL_HIP(hipMemsetAsync(w->flags.p, 0, (size_t)2 * s.ncol * sizeof(int), c->stream));
  int rc = multi_diag(c, w, fixedbits, op);
  if (rc) return rc;
  rc = multi_apply(c, op, s, fixedbits, w->UB.p, w->KU.p, false, nullptr);   // lifting: K ubar
  if (rc) return rc;
  const dim3 g(grid_stream(n6), (unsigned)s.ncb);
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_init<KB>), g, dim3(pl::kBlock), 0, c->stream, n6, f_dev, (const double *)w->KU.p,
                                       fixedbits, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, w->P.p, m.set[0], m.bb,
                                       s.ncol, s.stride));
  hipLaunchKernelGGL(pl::k_multi_begin, dim3((unsigned)s.ncol), dim3(pl::kWave), 0, c->stream, s.ncol, rtol, (const double *)m.bb,
                     m.thresh, m.status, m.flag[0]);
  PL_HIP(hipGetLastError());
  if (c->n_per_groups > 0) {   // periodic constraints: b is Q b (the caller's part), z0 = Q D^-1 r0, p0 = z0
    multi_periodic_average(c, s, w->Z.p);
    PL_HIP(hipMemcpyAsync(w->P.p, w->Z.p, (size_t)s.ncb * s.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  const int every = c->opt.check_every > 0 ? c->opt.check_every : 16;
  const size_t st_bytes = (size_t)pl::M_ST_COUNT * s.ncol * sizeof(double);
  auto look = [&]() -> int {     // 1: every column is frozen
    if (hipMemcpyAsync(status_host, m.status, st_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return -1;
    for (int j = 0; j < s.ncol; ++j)
      if (status_host[pl::M_ST_FROZEN * s.ncol + j] == 0.0) return 0;
    return 1;
  };
  int it = 0, all = look();
  while (all == 0 && it < max_iter) {
    const int stop = std::min(max_iter, it + every);
    for (; it < stop; ++it) {
      rc = multi_iteration(c, w, s, m, fixedbits, it, op);
      if (rc) return rc;
    }
    all = look();
  }
  if (all < 0) return fail(PL_ERR_HIP, "pcg_solve_multi: download of the status block failed");
  PL_MULTI_KB(s.KB, hipLaunchKernelGGL((pl::k_multi_compose<KB>), g, dim3(pl::kBlock), 0, c->stream, n6, fixedbits,
                                       (const double *)w->UB.p, (const double *)w->X.p, w->U.p, s.stride));
  PL_HIP(hipGetLastError());
  return PL_OK;
}

// entry-point checks shared by the three calls
int multi_check_handle(pl_context *h, const char *who, bool need_bc) {
  if (h->opkind != 0) return fail(PL_ERR_STATE, std::string(who) + ": not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, std::string(who) + ": single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->assembled) return fail(PL_ERR_STATE, std::string(who) + ": call pl_assemble first");
  if (need_bc && !h->have_bc) return fail(PL_ERR_STATE, std::string(who) + ": call pl_set_bc first");
  return PL_OK;
}

}  // namespace
