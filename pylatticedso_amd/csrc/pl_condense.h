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
#pragma once
#include "pl_device.h"

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

  // 1. records; -1 for a non-positive radius or segment count (or a strut without length)
  const double *xyz = a.xyz + inst * 3 * (size_t)N;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const double r = a.radius[inst * B + b];
    double len[3];
    int ns[3];
    bool ok = r > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      len[k] = a.seg_len[inst * 3 * B + 3 * b + k];
      ns[k] = a.seg_nsub[inst * 3 * B + 3 * b + k];
      ok = ok && len[k] >= 0.0 && (len[k] == 0.0 || ns[k] >= 1);
    }
    const int ia = a.conn[2 * b], ib = a.conn[2 * b + 1];
    const V3 d = {xyz[3 * ib] - xyz[3 * ia], xyz[3 * ib + 1] - xyz[3 * ia + 1], xyz[3 * ib + 2] - xyz[3 * ia + 2]};
    ok = ok && (len[0] + len[1] + len[2]) > 0.0 && dot(d, d) > 0.0;
    if (ok)
      rec[b] = make_record(scalars_from_flex(strut_flexibility(r, len, ns, a.m)), d);
    else
      status = -1;
  }
  __syncthreads();
  int st = status;

  // 2. lower triangle of K_II (block rows p >= q)
  if (st == 0) {
    for (int t = threadIdx.x; t < ni * ni; t += blockDim.x) {
      const int p = t / ni, q = t - p * ni;
      if (q > p) continue;
      double K[36];
      cond_node_block(rec, a.end_slot, B, -1 - p, -1 - q, K);
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
          status = k + 1;
        else
          L[(size_t)k * n6 + k] = sqrt(d);
      }
      __syncthreads();
      st = status;
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

}  // namespace pl
