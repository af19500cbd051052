// Batched exact static condensation of unit cells (pl_schur_cells): S = K_BB - K_BI K_II^-1 K_IB for many small
// lattices of ONE topology, one workgroup per instance (one cell with one radius set), fp64 throughout.
//
// Per workgroup:
//   1. the strut records from the instance's radii and penalised segments (strut_flexibility / scalars_from_flex /
//      make_record of pl_device.h - the element formula every other kernel uses), into LDS;
//   2. K_II (lower triangle) in LDS: one thread owns one 6 x 6 node-pair block and sums the incident struts in strut
//      order (tip_blocks) - no atomics, so S does not depend on where the instance sits in the batch;
//   3. Cholesky K_II = L L^T in LDS (right-looking, one column per step);
//   4. per column panel of boundary nodes: K_IB panel assembled as in 2, V = L^-1 K_IB by forward substitution
//      (one thread per column);
//   5. S = K_BB - V_I^T V_J for the node-pair blocks of the panel pair, K_BB summed from the records by the block's
//      owning thread; upper triangle computed, the lower one mirrored, so that S is exactly symmetric.
// A bad instance (info != 0) writes NaN into its S and leaves the others alone.
//
// pl_cells_recover (k_cells_recover) is the backward half on the same factor: steps 1 - 3, then
//   4'. g = K_IB u_b per interior node by its owning thread (the incident struts in strut order, tip_force);
//   5'. L L^T w = -g, one wave per right-hand side (u, and lam when given), the vector in registers;
//   6'. per strut lam_e^T (dK_e/dr) u_e on the recovered fields (strut_sens, the arithmetic of k_sens).
// It holds no V panel: records + factor in LDS, the boundary values are read from global memory.
#pragma once
#include "pl_kernels.h"

namespace pl {

constexpr int kCondBlock = 256;
constexpr int kCondMaxBoundary = 32;      // boundary nodes: S is at most 192 x 192
constexpr int kCondMaxInterior = 16;      // interior nodes: K_II is at most 96 x 96
constexpr int kCondMaxBeams = 512;        // struts (their records stay in LDS: 32 KiB)

struct CondenseArgs {
  int32_t n_nodes, n_beams, nb, ni;
  int32_t pw;                    // boundary nodes per column panel (pw >= nb: one panel)
  const int32_t *conn;           // [2 B] shared
  const int32_t *end_slot;       // [2 B] slot of each strut end: boundary position (>= 0) or -1 - interior index
  const double *xyz;             // [n_inst][3 n_nodes]
  const double *radius;          // [n_inst][B]
  const double *seg_len;         // [n_inst][3 B]
  const int32_t *seg_nsub;       // [n_inst][3 B]
  Material m;
  double *S;                     // [n_inst][6 nb][6 nb]
  int32_t *info;                 // [n_inst]
};

// LDS of one workgroup in doubles: records, K_II / its factor, one or two V panels (row stride 6 pw)
__host__ __device__ inline size_t condense_lds_doubles(int n_beams, int ni, int pw, int panels) {
  const size_t n6 = 6 * (size_t)ni;
  return 8 * (size_t)n_beams + n6 * n6 + (size_t)(panels > 1 ? 2 : 1) * n6 * 6 * (size_t)pw;
}

// 6 x 6 block (row node with slot sp, column node with slot sq) of the instance's stiffness, row-major: the struts in
// index order.  K_aa / K_ab come from the reversed record, K_bb / K_ba from the record itself (as in pl_coarse.h).
__device__ __forceinline__ void cond_node_block(const Record *rec, const int32_t *es, int B, int sp, int sq,
                                                double *K) {
#pragma unroll
  for (int e = 0; e < 36; ++e) K[e] = 0.0;
  const bool diag = sp == sq;
  double Kss[36], Kso[36];
  for (int b = 0; b < B; ++b) {
    const int sa = es[2 * b], sb = es[2 * b + 1];
    for (int end = 0; end < 2; ++end) {
      // end 0: the row node is end B (K_bb or K_ba); end 1: it is end A (K_aa or K_ab)
      const int s_row = end == 0 ? sb : sa, s_other = end == 0 ? sa : sb;
      if (s_row != sp || !(diag || s_other == sq)) continue;
      tip_blocks(end == 0 ? rec[b] : reversed(rec[b]), Kss, Kso);
      if (diag) {
#pragma unroll
        for (int e = 0; e < 36; ++e) K[e] += Kss[e];
      } else {
#pragma unroll
        for (int e = 0; e < 36; ++e) K[e] += Kso[e];
      }
    }
  }
}

// V[0:n6][0:6 np] = L^-1 K_IB[:, boundary nodes q0 .. q0 + np) (row stride W)
__device__ __forceinline__ void cond_panel(const CondenseArgs &a, const Record *rec, const double *L, double *V, int W,
                                           int q0, int np) {
  const int ni = a.ni, n6 = 6 * ni, w = 6 * np;
  for (int t = threadIdx.x; t < ni * np; t += blockDim.x) {
    const int p = t / np, q = t - p * np;
    double K[36];
    cond_node_block(rec, a.end_slot, a.n_beams, -1 - p, q0 + q, K);
#pragma unroll
    for (int e = 0; e < 36; ++e) V[(size_t)(6 * p + e / 6) * W + 6 * q + e % 6] = K[e];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < w; c += blockDim.x) {
    for (int k = 0; k < n6; ++k) {
      double x = V[(size_t)k * W + c];
      for (int l = 0; l < k; ++l) x -= L[(size_t)k * n6 + l] * V[(size_t)l * W + c];
      V[(size_t)k * W + c] = x / L[(size_t)k * n6 + k];
    }
  }
  __syncthreads();
}

// Step 1: the strut records of instance inst into rec; *status = -1 for a non-positive radius or segment count (or a
// strut without length).  The caller synchronises.
__device__ __forceinline__ void cond_records(const int32_t *conn, const double *xyz_all, const double *radius,
                                             const double *seg_len, const int32_t *seg_nsub, const Material &m,
                                             int64_t inst, int N, int B, Record *rec, int *status) {
  const double *xyz = xyz_all + inst * 3 * (size_t)N;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const double r = radius[inst * B + b];
    double len[3];
    int ns[3];
    bool ok = r > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      len[k] = seg_len[inst * 3 * B + 3 * b + k];
      ns[k] = seg_nsub[inst * 3 * B + 3 * b + k];
      ok = ok && len[k] >= 0.0 && (len[k] == 0.0 || ns[k] >= 1);
    }
    const int ia = conn[2 * b], ib = conn[2 * b + 1];
    const V3 d = {xyz[3 * ib] - xyz[3 * ia], xyz[3 * ib + 1] - xyz[3 * ia + 1], xyz[3 * ib + 2] - xyz[3 * ia + 2]};
    ok = ok && (len[0] + len[1] + len[2]) > 0.0 && dot(d, d) > 0.0;
    if (ok)
      rec[b] = make_record(scalars_from_flex(strut_flexibility(r, len, ns, m)), d);
    else
      *status = -1;
  }
}

// Steps 2 and 3 (st == 0 on entry, else nothing is done): lower triangle of K_II into L, its Cholesky factor in place.
// Returns the status: 0, or pivot k + 1 when it is not positive (a mechanism, a floating interior node).
__device__ __forceinline__ int cond_factor(const Record *rec, const int32_t *end_slot, int B, int ni, double *L,
                                           double *diag0, int *status, int st) {
  const int n6 = 6 * ni;
  // 2. lower triangle of K_II (block rows p >= q)
  if (st == 0) {
    for (int t = threadIdx.x; t < ni * ni; t += blockDim.x) {
      const int p = t / ni, q = t - p * ni;
      if (q > p) continue;
      double K[36];
      cond_node_block(rec, end_slot, B, -1 - p, -1 - q, K);
#pragma unroll
      for (int e = 0; e < 36; ++e) {
        const int i = 6 * p + e / 6, j = 6 * q + e % 6;
        if (j <= i) L[(size_t)i * n6 + j] = K[e];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n6; i += blockDim.x) diag0[i] = L[(size_t)i * n6 + i];
    __syncthreads();

    // 3. Cholesky; pivot k + 1 reported when it is not positive (a mechanism, a floating interior node)
    for (int k = 0; k < n6; ++k) {
      if (threadIdx.x == 0) {
        const double d = L[(size_t)k * n6 + k];
        if (!(diag0[k] > 0.0) || !(d > 1e-14 * diag0[k]))
          *status = k + 1;
        else
          L[(size_t)k * n6 + k] = sqrt(d);
      }
      __syncthreads();
      st = *status;
      if (st != 0) break;
      const double lkk = L[(size_t)k * n6 + k];
      for (int i = k + 1 + threadIdx.x; i < n6; i += blockDim.x) L[(size_t)i * n6 + k] /= lkk;
      __syncthreads();
      const int r = n6 - k - 1;
      for (int t = threadIdx.x; t < r * r; t += blockDim.x) {
        const int i = k + 1 + t / r, j = k + 1 + t % r;
        if (j <= i) L[(size_t)i * n6 + j] -= L[(size_t)i * n6 + k] * L[(size_t)j * n6 + k];
      }
      __syncthreads();
    }
  }
  return st;
}

__global__ __launch_bounds__(kCondBlock) void k_schur_cells(CondenseArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cond_lds[];
  __shared__ double diag0[6 * kCondMaxInterior];
  __shared__ int status;
  const int64_t inst = blockIdx.x;
  const int B = a.n_beams, N = a.n_nodes, ni = a.ni, n6 = 6 * ni, m = 6 * a.nb;
  const int npan = (a.nb + a.pw - 1) / a.pw, W = 6 * a.pw;
  Record *rec = reinterpret_cast<Record *>(cond_lds);
  double *L = cond_lds + 8 * (size_t)B;
  double *VJ = L + (size_t)n6 * n6;
  double *VI = npan > 1 ? VJ + (size_t)n6 * W : VJ;
  double *S = a.S + inst * (size_t)m * m;
  if (threadIdx.x == 0) status = 0;
  __syncthreads();

  // 1. - 3. records, K_II, its Cholesky factor
  cond_records(a.conn, a.xyz, a.radius, a.seg_len, a.seg_nsub, a.m, inst, N, B, rec, &status);
  __syncthreads();
  const int st = cond_factor(rec, a.end_slot, B, ni, L, diag0, &status, status);
  if (threadIdx.x == 0) a.info[inst] = st;
  if (st != 0) {
    const double nan = __builtin_nan("");
    for (int t = threadIdx.x; t < m * m; t += blockDim.x) S[t] = nan;
    return;
  }

  // 4. / 5. panels of boundary nodes: S_IJ = K_BB,IJ - V_I^T V_J for I <= J
  for (int J = 0; J < npan; ++J) {
    const int j0 = J * a.pw, nj = min(a.pw, a.nb - j0);
    cond_panel(a, rec, L, VJ, W, j0, nj);
    for (int I = 0; I <= J; ++I) {
      const int i0 = I * a.pw, nI = min(a.pw, a.nb - i0);
      if (I < J) cond_panel(a, rec, L, VI, W, i0, nI);
      const double *Vi = (I < J) ? VI : VJ;
      for (int t = threadIdx.x; t < nI * nj; t += blockDim.x) {
        const int P = i0 + t / nj, Q = j0 + t % nj;
        if (P > Q) continue;
        double K[36];
        cond_node_block(rec, a.end_slot, B, P, Q, K);
        const int ci = 6 * (P - i0), cj = 6 * (Q - j0);
#pragma unroll
        for (int e = 0; e < 36; ++e) {
          const int x = e / 6, y = e % 6;
          if (P == Q && y < x) continue;
          double s = K[e];
          for (int k = 0; k < n6; ++k) s -= Vi[(size_t)k * W + ci + x] * VJ[(size_t)k * W + cj + y];
          S[(size_t)(6 * P + x) * m + 6 * Q + y] = s;
          S[(size_t)(6 * Q + y) * m + 6 * P + x] = s;
        }
      }
      __syncthreads();   // VI is refilled by the next panel
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// pl_cells_recover
// ---------------------------------------------------------------------------------------------------------
struct RecoverArgs {
  int32_t n_nodes, n_beams, nb, ni;
  const int32_t *conn;           // [2 B] shared
  const int32_t *end_slot;       // [2 B] as CondenseArgs
  const int32_t *node_slot;      // [n_nodes] slot of every node
  const double *xyz, *radius, *seg_len;
  const int32_t *seg_nsub;
  Material m;
  const double *u_b, *lam_b;     // [n_inst][6 nb]; lam_b may be null (lam = u)
  double *u_full, *lam_full;     // [n_inst][6 n_nodes] or null
  double *sens;                  // [n_inst][B] or null
  int32_t *info;                 // [n_inst]
};

// LDS of one workgroup in doubles: records and K_II / its factor
__host__ __device__ inline size_t recover_lds_doubles(int n_beams, int ni) {
  return 8 * (size_t)n_beams + 36 * (size_t)ni * ni;
}

// Workgroup size: the widest loops are the trailing update of the factor ((6 ni)^2 entries) and the struts
inline int recover_block(int n_beams, int ni) {
  const int work = n_beams > 9 * ni * ni ? n_beams : 9 * ni * ni;
  return work <= 64 ? 64 : work <= 128 ? 128 : kCondBlock;
}

// Values of the node with slot s: boundary values from vb, interior ones from w (zero when w is null)
__device__ __forceinline__ void cond_node_values(int s, const double *vb, const double *w, V3 &u, V3 &t) {
  if (s >= 0)
    load6(vb + 6 * s, u, t);
  else if (w)
    load6(w + 6 * (-1 - s), u, t);
  else
    u = t = V3{0.0, 0.0, 0.0};
}

__global__ __launch_bounds__(kCondBlock) void k_cells_recover(RecoverArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cond_lds[];
  __shared__ double diag0[6 * kCondMaxInterior];
  __shared__ __attribute__((aligned(16))) double W[2][6 * kCondMaxInterior];
  __shared__ int status;
  const int64_t inst = blockIdx.x;
  const int B = a.n_beams, N = a.n_nodes, ni = a.ni, n6 = 6 * ni, m = 6 * a.nb;
  const int nrhs = a.lam_b ? 2 : 1;
  Record *rec = reinterpret_cast<Record *>(cond_lds);
  double *L = cond_lds + 8 * (size_t)B;
  if (threadIdx.x == 0) status = 0;
  __syncthreads();
  cond_records(a.conn, a.xyz, a.radius, a.seg_len, a.seg_nsub, a.m, inst, N, B, rec, &status);
  __syncthreads();
  const int st = cond_factor(rec, a.end_slot, B, ni, L, diag0, &status, status);
  if (threadIdx.x == 0) a.info[inst] = st;
  double *uf = a.u_full ? a.u_full + inst * 6 * (size_t)N : nullptr;
  double *lf = a.lam_full ? a.lam_full + inst * 6 * (size_t)N : nullptr;
  double *sens = a.sens ? a.sens + inst * (size_t)B : nullptr;
  if (st != 0) {
    const double nan = __builtin_nan("");
    for (int t = threadIdx.x; t < 6 * N; t += blockDim.x) {
      if (uf) uf[t] = nan;
      if (lf) lf[t] = nan;
    }
    if (sens)
      for (int b = threadIdx.x; b < B; b += blockDim.x) sens[b] = nan;
    return;
  }
  const double *vb[2] = {a.u_b + inst * (size_t)m, a.lam_b ? a.lam_b + inst * (size_t)m : nullptr};

  // 4'. W = -K_IB v_b: the owning thread of (right-hand side, interior node) sums the incident struts in strut order
  for (int t = threadIdx.x; t < nrhs * ni; t += blockDim.x) {
    const int r = t / ni, p = t - r * ni;
    V3 gF = {0.0, 0.0, 0.0}, gM = {0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b) {
      const int sa = a.end_slot[2 * b], sb = a.end_slot[2 * b + 1];
      if (sa != -1 - p && sb != -1 - p) continue;
      V3 uA, tA, uB, tB, F, M;
      cond_node_values(sa, vb[r], nullptr, uA, tA);
      cond_node_values(sb, vb[r], nullptr, uB, tB);
      if (sb == -1 - p)
        tip_force(rec[b], uA, tA, uB, tB, F, M);
      else
        tip_force(reversed(rec[b]), uB, tB, uA, tA, F, M);
      gF = gF + F;
      gM = gM + M;
    }
    double *w = W[r] + 6 * p;
    w[0] = -gF.x; w[1] = -gF.y; w[2] = -gF.z;
    w[3] = -gM.x; w[4] = -gM.y; w[5] = -gM.z;
  }
  __syncthreads();

  // 5'. L L^T w = W: one wave per right-hand side, entries k and k + 64 of the vector in the registers of lane k
  if (n6 > 0) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwave = blockDim.x / kWave;
    for (int r = wave; r < nrhs; r += nwave) {
      double *w = W[r];
      double x0 = lane < n6 ? w[lane] : 0.0, x1 = lane + kWave < n6 ? w[lane + kWave] : 0.0;
      for (int k = 0; k < n6; ++k) {             // L y = w by rows: y_k = (w_k - L[k, :k] . y[:k]) / L_kk
        const double *Lk = L + (size_t)k * n6;
        double part = 0.0;
        if (lane < k) part = Lk[lane] * x0;
        if (lane + kWave < k) part += Lk[lane + kWave] * x1;
        const double s = wave_sum(part);
        if (lane == (k & (kWave - 1))) {
          if (k < kWave) x0 = (x0 - s) / Lk[k];
          else x1 = (x1 - s) / Lk[k];
        }
      }
      for (int k = n6 - 1; k >= 0; --k) {        // L^T x = y by columns of L^T = rows of L
        const double *Lk = L + (size_t)k * n6;
        const double xk = __shfl(k < kWave ? x0 : x1, k & (kWave - 1)) / Lk[k];
        if (lane == (k & (kWave - 1))) {
          if (k < kWave) x0 = xk;
          else x1 = xk;
        }
        if (lane < k) x0 -= Lk[lane] * xk;
        if (lane + kWave < k) x1 -= Lk[lane + kWave] * xk;
      }
      if (lane < n6) w[lane] = x0;
      if (lane + kWave < n6) w[lane + kWave] = x1;
    }
  }
  __syncthreads();

  // the whole fields, cell-local node order
  for (int t = threadIdx.x; t < 6 * N; t += blockDim.x) {
    const int s = a.node_slot[t / 6], k = t % 6;
    if (uf) uf[t] = s >= 0 ? vb[0][6 * s + k] : W[0][6 * (-1 - s) + k];
    if (lf) lf[t] = s >= 0 ? vb[nrhs - 1][6 * s + k] : W[nrhs - 1][6 * (-1 - s) + k];
  }

  // 6'. per-strut sensitivities on the recovered fields
  if (sens) {
    const double *xyz = a.xyz + inst * 3 * (size_t)N;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const int ia = a.conn[2 * b], ib = a.conn[2 * b + 1];
      const int sa = a.end_slot[2 * b], sb = a.end_slot[2 * b + 1];
      const V3 d = {xyz[3 * ib] - xyz[3 * ia], xyz[3 * ib + 1] - xyz[3 * ia + 1], xyz[3 * ib + 2] - xyz[3 * ia + 2]};
      double len[3];
      int ns[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        len[k] = a.seg_len[inst * 3 * B + 3 * b + k];
        ns[k] = a.seg_nsub[inst * 3 * B + 3 * b + k];
      }
      V3 uA, tA, uB, tB, lA, mA, lB, mB;
      cond_node_values(sa, vb[0], W[0], uA, tA);
      cond_node_values(sb, vb[0], W[0], uB, tB);
      cond_node_values(sa, vb[nrhs - 1], W[nrhs - 1], lA, mA);
      cond_node_values(sb, vb[nrhs - 1], W[nrhs - 1], lB, mB);
      sens[b] = strut_sens(a.radius[inst * B + b], len, ns, a.m, d, uA, tA, uB, tB, lA, mA, lB, mB);
    }
  }
}

}  // namespace pl
