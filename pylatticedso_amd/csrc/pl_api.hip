// libpylattice_hip.so - the C ABI declared in include/pylattice_hip.h (gfx950 / MI355X).  One translation unit:
// pl_context.h (handle state) <- pl_ops.h (operator launches) <- pl_assembly.h <- pl_solver.h (+ pl_warm.h, pl_schedule.h) <- this file.
#include <functional>

#include "pl_solver.h"
#include "pl_condense.h"
#include "pl_multi.h"
#include "pl_stress.h"
#include "pl_buckling.h"
#include "pl_thermal.h"
#include "pl_conduction.h"
#include "pl_heat.h"
#include "pl_geom.h"
#include "pl_mass.h"
#include "pl_dyn.h"
#include "pl_harm.h"
#include "pl_dyn_sens.h"
#include "pl_harm_sens.h"
#include "pl_objective.h"
#include "pl_sensgram.h"


// ==========================================================================================================
// C ABI
// ==========================================================================================================
namespace {
template <typename WT>
int debug_spd_solve_t(int device, int32_t n, const double *A, const double *b, double *x, double *quad) {
  if (n <= 0 || !A || !b || !x) return fail(PL_ERR_ARG, "pl_debug_spd_solve: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PL_ERR_NODEVICE, "no HIP device visible");
  PL_HIP(hipSetDevice(device));
  const int np = (n + pl::kNB - 1) / pl::kNB * pl::kNB;
  std::vector<double> Ap((size_t)np * np, 0.0), bp(np, 0.0);
  for (int i = 0; i < np; ++i) {
    if (i < n) {
      std::memcpy(&Ap[(size_t)i * np], A + (size_t)i * n, n * sizeof(double));
      bp[i] = b[i];
    } else {
      Ap[(size_t)i * np + i] = 1.0;
    }
  }
  DevBuf<double> dA, dL, dD, db, dt, dy, dq;
  DevBuf<WT> dW, dWt;
  DevBuf<int> dinfo;
  PL_HIP(dA.alloc(Ap.size()));
  PL_HIP(dW.alloc(Ap.size()));
  PL_HIP(dL.alloc(Ap.size()));
  PL_HIP(dWt.alloc(Ap.size()));
  PL_HIP(hipMemset(dWt.p, 0, Ap.size() * sizeof(WT)));
  PL_HIP(dD.alloc((size_t)np * pl::kNB));
  PL_HIP(db.alloc(np));
  PL_HIP(dt.alloc(np));
  PL_HIP(dy.alloc(np));
  PL_HIP(dq.alloc(pl::kSlots));
  PL_HIP(dinfo.alloc(2));
  PL_HIP(hipMemcpy(dA.p, Ap.data(), Ap.size() * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(db.p, bp.data(), np * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemset(dW.p, 0, Ap.size() * sizeof(WT)));
  PL_HIP(hipMemset(dq.p, 0, pl::kSlots * sizeof(double)));
  PL_HIP(hipMemset(dinfo.p, 0, 2 * sizeof(int)));
  pl::dense_factor_inverse(dA.p, dL.p, dW.p, dWt.p, dD.p, np, np, dinfo.p, 0, nullptr);
  pl::dense_apply(dW.p, dWt.p, np, np, db.p, dt.p, dy.p, dq.p, nullptr, nullptr);
  PL_HIP(hipGetLastError());
  PL_HIP(hipDeviceSynchronize());
  int info[2];
  PL_HIP(hipMemcpy(info, dinfo.p, sizeof(info), hipMemcpyDeviceToHost));
  if (info[0] != 0) return fail(PL_ERR_ARG, "pl_debug_spd_solve: matrix is not positive definite");
  std::vector<double> y(np), q(pl::kSlots);
  PL_HIP(hipMemcpy(y.data(), dy.p, np * sizeof(double), hipMemcpyDeviceToHost));
  PL_HIP(hipMemcpy(q.data(), dq.p, pl::kSlots * sizeof(double), hipMemcpyDeviceToHost));
  std::memcpy(x, y.data(), n * sizeof(double));
  if (quad) {
    *quad = 0.0;
    for (double v : q) *quad += v;
  }
  return PL_OK;
}

// pl_debug_dense_level: the dense level as build_coarse_level and coarse_apply run it - the band, the row ranges of the
// inverse factor on a second stream, the storage type, both forms of the apply - on a matrix of the caller's.
inline double widen(double v) { return v; }
inline double widen(float v) { return (double)v; }
inline double widen(pl::bf16_t v) {
  const uint32_t u = (uint32_t)v.v << 16;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return (double)f;
}
struct DebugStreams {
  hipStream_t main = nullptr, side = nullptr;
  hipEvent_t go = nullptr, done = nullptr;
  ~DebugStreams() {
    if (go) (void)hipEventDestroy(go);
    if (done) (void)hipEventDestroy(done);
    if (side) (void)hipStreamDestroy(side);
    if (main) (void)hipStreamDestroy(main);
  }
};
template <typename WT>
int debug_dense_level_t(int device, int32_t n, const double *A, int32_t bw_blocks, int32_t trtri_rows,
                        int32_t band_roundtrip, const double *r, const double *add0, double *W_out, double *Wt_out,
                        float *Ainv_out, double *t_out, double *y_out, double *quad, double *y_one, double *quad_one,
                        int32_t *one_gemv, int32_t *info_out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PL_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PL_ERR_ARG, "pl_debug_dense_level: bad device ordinal");
  PL_HIP(hipSetDevice(device));
  const int np = (n + pl::kNB - 1) / pl::kNB * pl::kNB, nb = np / pl::kNB;
  if (band_roundtrip && !(bw_blocks > 0 && bw_blocks + 1 < nb))
    return fail(PL_ERR_ARG, "pl_debug_dense_level: the band transfer needs 0 < bw_blocks < n / 64 - 1");
  const size_t n2 = (size_t)np * np;
  const bool one = !std::is_same<WT, double>::value && np <= pl::kOneGemvMaxDofs;
  std::vector<double> Ap(n2, 0.0), rp(np, 0.0);
  for (int i = 0; i < np; ++i) {
    if (i < n) {
      std::memcpy(&Ap[(size_t)i * np], A + (size_t)i * n, n * sizeof(double));
      rp[i] = r[i];
    } else {
      Ap[(size_t)i * np + i] = 1.0;
    }
  }
  DevBuf<double> dA, dL, dD, dr, dt, dy, dy1, dq, dq1, dadd;
  DevBuf<WT> dW, dWt;
  DevBuf<float> dG;
  DevBuf<int> dinfo;
  PL_HIP(dA.alloc(n2));
  PL_HIP(dL.alloc(n2));
  PL_HIP(dW.alloc(n2));
  PL_HIP(dWt.alloc(n2));
  PL_HIP(dD.alloc((size_t)np * pl::kNB));
  PL_HIP(dr.alloc(np));
  PL_HIP(dt.alloc(np));
  PL_HIP(dy.alloc(np));
  PL_HIP(dy1.alloc(np));
  PL_HIP(dq.alloc(pl::kSlots));
  PL_HIP(dq1.alloc(pl::kSlots));
  PL_HIP(dadd.alloc(pl::kSlots));
  PL_HIP(dinfo.alloc(2));
  if (one) PL_HIP(dG.alloc(n2));
  PL_HIP(hipMemcpy(dA.p, Ap.data(), n2 * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dr.p, rp.data(), np * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dadd.p, add0, pl::kSlots * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemset(dL.p, 0, n2 * sizeof(double)));
  PL_HIP(hipMemset(dW.p, 0, n2 * sizeof(WT)));
  PL_HIP(hipMemset(dWt.p, 0, n2 * sizeof(WT)));
  PL_HIP(hipMemset(dt.p, 0, np * sizeof(double)));
  PL_HIP(hipMemset(dy.p, 0, np * sizeof(double)));
  PL_HIP(hipMemset(dy1.p, 0, np * sizeof(double)));
  PL_HIP(hipMemset(dq.p, 0, pl::kSlots * sizeof(double)));
  PL_HIP(hipMemset(dq1.p, 0, pl::kSlots * sizeof(double)));
  PL_HIP(hipMemset(dinfo.p, 0, 2 * sizeof(int)));
  if (one) PL_HIP(hipMemset(dG.p, 0, n2 * sizeof(float)));
  PL_HIP(hipDeviceSynchronize());                    // (the streams below do not wait for the null stream)
  DebugStreams st;
  PL_HIP(hipStreamCreateWithFlags(&st.main, hipStreamNonBlocking));
  pl::TrtriPhases ph;
  if (trtri_rows > 0) {
    PL_HIP(hipStreamCreateWithFlags(&st.side, hipStreamNonBlocking));
    PL_HIP(hipEventCreateWithFlags(&st.go, hipEventDisableTiming));
    PL_HIP(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    ph.rows = trtri_rows;
    ph.stream = st.side;
    ph.ev_go = st.go;
    ph.ev_done = st.done;
  }
  if (band_roundtrip) {
    pl::band_pack(np, np, bw_blocks, dA.p, dL.p, st.main);
    pl::band_unpack(np, np, bw_blocks, dL.p, dA.p, st.main);
  }
  pl::dense_factor_inverse(dA.p, dL.p, dW.p, dWt.p, dD.p, np, np, dinfo.p, bw_blocks, st.main, nullptr, (unsigned *)nullptr,
                           ph);
  pl::dense_apply(dW.p, dWt.p, np, np, dr.p, dt.p, dy.p, dq.p, dadd.p, st.main);
  if constexpr (!std::is_same<WT, double>::value) {
    if (one) {
      pl::dense_explicit_inverse(np, (const WT *)dW.p, np, dG.p, st.main);
      pl::dense_apply_one_gemv(dG.p, np, np, dr.p, dy1.p, dq1.p, dadd.p, st.main);
    }
  }
  PL_HIP(hipGetLastError());
  PL_HIP(hipStreamSynchronize(st.main));
  if (st.side) PL_HIP(hipStreamSynchronize(st.side));
  int info[2];
  PL_HIP(hipMemcpy(info, dinfo.p, sizeof(info), hipMemcpyDeviceToHost));
  info_out[0] = info[0];
  info_out[1] = info[1];
  {
    std::vector<WT> w(n2);
    PL_HIP(hipMemcpy(w.data(), dW.p, n2 * sizeof(WT), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n2; ++e) W_out[e] = widen(w[e]);
    PL_HIP(hipMemcpy(w.data(), dWt.p, n2 * sizeof(WT), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n2; ++e) Wt_out[e] = widen(w[e]);
  }
  std::vector<double> q(pl::kSlots);
  PL_HIP(hipMemcpy(t_out, dt.p, np * sizeof(double), hipMemcpyDeviceToHost));
  PL_HIP(hipMemcpy(y_out, dy.p, np * sizeof(double), hipMemcpyDeviceToHost));
  PL_HIP(hipMemcpy(q.data(), dq.p, pl::kSlots * sizeof(double), hipMemcpyDeviceToHost));
  *quad = 0.0;
  for (double v : q) *quad += v;
  *one_gemv = one ? 1 : 0;
  if (one) {
    PL_HIP(hipMemcpy(Ainv_out, dG.p, n2 * sizeof(float), hipMemcpyDeviceToHost));
    PL_HIP(hipMemcpy(y_one, dy1.p, np * sizeof(double), hipMemcpyDeviceToHost));
    PL_HIP(hipMemcpy(q.data(), dq1.p, pl::kSlots * sizeof(double), hipMemcpyDeviceToHost));
    *quad_one = 0.0;
    for (double v : q) *quad_one += v;
  }
  return PL_OK;
}

// ---- multi-GPU ------------------------------------------------------------------------------------------
}  // namespace

extern "C" {

const char *pl_last_error(void) { return g_err.c_str(); }
#ifndef PL_KP_HASH
#define PL_KP_HASH "unknown"
#endif
const char *pl_version(void) { return "pylattice_hip 0.2 (gfx950) kp=" PL_KP_HASH; }

uint32_t pl_opts_size(void) { return (uint32_t)sizeof(pl_opts_t); }
uint32_t pl_stats_size(void) { return (uint32_t)sizeof(pl_stats_t); }
uint32_t pl_abi_version(void) { return PL_ABI_VERSION; }

int pl_default_opts(pl_opts_t *o, uint32_t struct_size) {
  if (!o) return fail(PL_ERR_ARG, "pl_default_opts: null argument");
  if (struct_size != sizeof(pl_opts_t))
    return fail(PL_ERR_ARG, "pl_default_opts: the caller's pl_opts_t has " + std::to_string(struct_size) +
                                " bytes, this library's " + std::to_string(sizeof(pl_opts_t)) +
                                " (ABI version " + std::to_string(PL_ABI_VERSION) + "): rebuild the binding against include/pylattice_hip.h");
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (uint32_t)sizeof(pl_opts_t);
  o->abi_version = PL_ABI_VERSION;
  o->young = 1013.0;   // VeroClear
  o->poisson = 0.3;
  o->kappa = 0.9;
  o->pen_coef = 1.5;
  o->device = 0;
  o->spmv_kernel = 0;
  o->precond = 1;
  o->reorder = 1;
  o->check_every = 0;   // adaptive
  return PL_OK;
}

namespace {
// pl_opts_t must carry the stamp of pl_default_opts of THIS library (include/pylattice_hip.h, "ABI handshake")
int check_opts_abi(const pl_opts_t *o, const char *who) {
  if (o->struct_size != sizeof(pl_opts_t) || o->abi_version != PL_ABI_VERSION)
    return fail(PL_ERR_ARG, std::string(who) + ": pl_opts_t was not initialised by pl_default_opts of this library (struct_size " +
                                std::to_string(o->struct_size) + " / abi " + std::to_string(o->abi_version) + ", expected " +
                                std::to_string(sizeof(pl_opts_t)) + " / " + std::to_string(PL_ABI_VERSION) + ")");
  return PL_OK;
}
inline bool multi_rank_handle(const pl_opts_t *o) { return o->grid_nodes > 0; }
// modes per aggregate of the dense level: 12 (rigid + strains) needs the 12-mode tile level, i.e. precond = 3 (either CG form)
inline int coarse_modes_of(const pl_opts_t *o, int64_t N = -1) {
  const bool tile12 = o->precond == 3 && o->tile_modes != 6;
  if (!tile12 || o->coarse_modes == 6) return 6;
  if (multi_rank_handle(o)) N = o->grid_nodes;       // every rank must decide alike: the node count of the whole lattice
  // automatic: from a quarter of a million nodes on (below, the longer set-up of the richer level costs what its
  // iterations save: 32^3 Octet 178 M beams/s with 6 modes, 169 M with 12)
  return (o->coarse_modes == 12 || N < 0 || N >= 250000) ? 12 : 6;
}
// dofs the dense level may have (see the comment at its set-up in pl_create)
inline int coarse_budget(const pl_opts_t *o, int64_t N) {
  const bool multi_rank = o->grid_nodes > 0;
  if (o->coarse_max_dofs > 0) return o->coarse_max_dofs;
  // 12 modes per aggregate: 5^3 aggregates (1 500 dofs) beat 7^3 x 6 (2 058) below a million nodes - 120 against 126
  // iterations at 50^3 Octet, 24 chain links instead of 33 (measured: 1 536 -> 203, 2 600 -> 200, 800 -> 193 M beams/s)
  // (the level's cost does not grow with the lattice, its benefit does: 100^3 BCC 3 072 -> 59.7, 6 144 -> 61.4 M beams/s;
  // 200 x 200 x 50 BCC + Octet 3 072 -> 104.9, 6 144 -> 136.4 M beams/s)
  // several GPUs: replicated on every rank and all-reduced per assembly, decided on the node count of the WHOLE lattice so
  // that every rank decides alike.  Emulated 4 / 8 ranks (50 x 50N x 50 Octet): 161 / 179 iterations with 6 modes and 3 072
  // dofs, 139 / 174 with 12 modes and 3 072, 120 / 139 with 12 modes and 6 144
  if (multi_rank) return (coarse_modes_of(o, N) == 12 && o->grid_nodes >= 2000000) ? 6144 : 3072;
  if (coarse_modes_of(o, N) == 12) return N >= 2000000 ? 6144 : (N >= 1000000 ? 3072 : (N >= 250000 ? 1536 : 768));
  return N >= 1000000 ? 3072 : 2100;
}
}  // namespace

int pl_create(const pl_mesh_t *m, const pl_opts_t *o, pl_handle *out) {
  if (!m || !o || !out) return fail(PL_ERR_ARG, "pl_create: null argument");
  if (int rc_abi = check_opts_abi(o, "pl_create")) return rc_abi;
  StageTimer stage("pl_create");
  if (m->n_nodes <= 0 || m->n_beams <= 0) return fail(PL_ERR_ARG, "pl_create: empty mesh");
  if (m->n_nodes >= (1LL << 31) - 64 || m->n_beams >= (1LL << 31) - 64)
    return fail(PL_ERR_ARG, "pl_create: more than 2^31 nodes/struts per handle");
  if (!m->node_xyz || !m->beam_conn || !m->beam_radius || !m->seg_len || !m->seg_nsub)
    return fail(PL_ERR_ARG, "pl_create: null mesh array");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PL_ERR_NODEVICE, "pl_create: no HIP device visible (libpylattice_hip has no CPU fallback)");
  if (o->device < 0 || o->device >= ndev) return fail(PL_ERR_ARG, "pl_create: bad device ordinal");
  if (o->precond == 5 && 6 * m->n_nodes > PL_DDM_DENSE_MAX)
    return fail(PL_ERR_ARG, "pl_create: precond = 5 (dense factorisation) serves at most PL_DDM_DENSE_MAX dofs");
  const int64_t N = m->n_nodes, B = m->n_beams;
  {
    std::atomic<int64_t> bad_ends{-1}, bad_radius{-1}, bad_len{-1}, bad_seg{-1};
    pl::parallel_for(B, [&](int64_t b0, int64_t b1, unsigned) {
      for (int64_t b = b0; b < b1; ++b) {
        const int32_t a = m->beam_conn[2 * b], d = m->beam_conn[2 * b + 1];
        if (a < 0 || d < 0 || a >= N || d >= N || a == d) bad_ends = b;
        if (!(m->beam_radius[b] > 0.0)) bad_radius = b;
        const double L = m->seg_len[3 * b] + m->seg_len[3 * b + 1] + m->seg_len[3 * b + 2];
        if (!(L > 0.0)) bad_len = b;
        for (int k = 0; k < 3; ++k)
          if (m->seg_len[3 * b + k] < 0.0 || (m->seg_len[3 * b + k] > 0.0 && m->seg_nsub[3 * b + k] < 1)) bad_seg = b;
      }
    });
    if (bad_ends >= 0)
      return fail(PL_ERR_ARG, "pl_create: strut " + std::to_string(bad_ends.load()) + " has invalid end nodes");
    if (bad_radius >= 0) return fail(PL_ERR_ARG, "pl_create: non-positive radius");
    if (bad_len >= 0) return fail(PL_ERR_ARG, "pl_create: strut with zero length");
    if (bad_seg >= 0) return fail(PL_ERR_ARG, "pl_create: bad segment data on strut " + std::to_string(bad_seg.load()));
  }
  stage.mark("validate");
  PL_HIP(hipSetDevice(o->device));
  pl_context *c = new pl_context();
  c->opt = *o;
  c->N = N;
  c->B = B;
  c->mat = {o->young, o->young / (2.0 * (1.0 + o->poisson)), o->kappa, o->pen_coef};
  c->lpn = o->lanes_per_node > 0 ? o->lanes_per_node : pl::kDefaultLPN;
  if (c->lpn != 1 && c->lpn != 2 && c->lpn != 4 && c->lpn != 8 && c->lpn != 16) {
    delete c;
    return fail(PL_ERR_ARG, "pl_create: lanes_per_node must be 0 (default), 1, 2, 4, 8 or 16");
  }
  auto bail = [&](int rc) {
    delete c;
    return rc;
  };
#define PL_TRY(expr)              \
  do {                            \
    int _rc = (expr);             \
    if (_rc) return bail(_rc);    \
  } while (0)
#define PL_HIPC(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return bail(fail(PL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
  } while (0)
  {   // the main stream carries the latency-bound chains (dense factorisation, PCG): it goes ahead of the bulk fills
    int prio_low = 0, prio_high = 0;
    PL_HIPC(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    PL_HIPC(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_high));
    PL_HIPC(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_low));
  }
  PL_HIPC(hipEventCreate(&c->ev0));
  PL_HIPC(hipEventCreate(&c->ev1));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_chol, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_t0, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_t1, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_p0, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_p1, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_fill1, hipEventDisableTiming));
  PL_HIPC(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
  {
    // The explicit K (2.5 GB of traffic) is filled BESIDE the latency-bound factorisation chain, on a stream whose CU mask
    // leaves k of every 8 CUs to the chain (next to an unmasked fill every link of the chain went from 44 to 57 us, which is
    // why the fill used to wait for the chain's end: assembly 2.20 -> 1.93 ms at 50^3 Octet with k = 4 or 5, 1.97 with 1,
    // 2.03 with 6).  The CUs are left out on a diagonal - bit i when (i / 8 + i) % 8 < k - which is k CUs of every XCD
    // whether the mask bits run XCD-major or round-robin over the XCDs.  PL_BSR_CUMASK=0: the old order.
    // The mask (8 words = 256 CUs in 8 XCDs) and the two rates of the split heuristic in pl_assemble were tuned on MI355X:
    // on a device with another CU count the masked stream is not created and the fill keeps the old order.
    const char *e = std::getenv("PL_BSR_CUMASK");
    const int k = e ? std::atoi(e) : 4;
    hipDeviceProp_t prop;
    const bool tuned_layout = hipGetDeviceProperties(&prop, o->device) == hipSuccess && prop.multiProcessorCount == 256;
    if (k > 0 && k < 8 && tuned_layout) {
      uint32_t mask[8];
      for (int w = 0; w < 8; ++w) {
        mask[w] = 0u;
        for (int b = 0; b < 32; ++b) {
          const int i = 32 * w + b;
          if ((i / 8 + i) % 8 >= k) mask[w] |= 1u << b;
        }
      }
      if (hipExtStreamCreateWithCUMask(&c->side_cu, 8, mask) != hipSuccess) {   // (no CU masks here: the old order)
        (void)hipGetLastError();
        c->side_cu = nullptr;
      }
    }
  }

  // node ordering on the device
  const double global_grid[7] = {o->grid_lo[0], o->grid_lo[1], o->grid_lo[2], o->grid_hi[0], o->grid_hi[1],
                                 o->grid_hi[2], (double)o->grid_nodes};
  c->perm.resize(N);
  std::iota(c->perm.begin(), c->perm.end(), 0);
  std::vector<int32_t> tile_start, tile_of;
  std::vector<int64_t> tile_brick;
  pl::BrickGrid grid;
  if (o->reorder == 1) {
    pl::spatial_order(m->node_xyz, N, c->perm, tile_start,
                      (double)(o->tile_nodes > 0 ? std::min(o->tile_nodes, pl::kTileMaxNodes) : 256), tile_brick,
                      grid, o->grid_nodes > 0 ? global_grid : nullptr,
                      (o->precond >= 2 && o->precond <= 4) ? coarse_budget(o, N) * 6 / coarse_modes_of(o, N) : 0);
    c->reordered = true;
    // Inside a tile: nodes of one KIND together (kind = the set of directions of a node's struts: in a periodic lattice
    // the corner nodes, the face centres of each orientation, ...; original order within a kind).  Struts of one
    // direction then join consecutive rows on both ends, which is what keeps the LDS-resident K*p (pl_tile.h) free of
    // bank conflicts; the other kernels do not care about the order inside a tile.
    {
      std::vector<uint64_t> kind((size_t)N, 0);
      pl::parallel_for(B, [&](int64_t b0, int64_t b1, unsigned) {
        for (int64_t b = b0; b < b1; ++b) {
          const int32_t u = m->beam_conn[2 * b], v = m->beam_conn[2 * b + 1];
          uint64_t d = 0;
          for (int k = 0; k < 3; ++k) {
            const int64_t q = (int64_t)std::llround((m->node_xyz[3 * (size_t)v + k] - m->node_xyz[3 * (size_t)u + k]) * 4096.0);
            d = d * 0x9E3779B97F4A7C15ull + (uint64_t)(q + (1 << 20));
          }
          auto mix = [](uint64_t h) { h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; return h; };
          __atomic_fetch_add(&kind[u], mix(d), __ATOMIC_RELAXED);
          __atomic_fetch_add(&kind[v], mix(~d), __ATOMIC_RELAXED);
        }
      }, 1 << 16);
      const int64_t T = (int64_t)tile_start.size() - 1;
      pl::parallel_for(T, [&](int64_t t0, int64_t t1, unsigned) {
        for (int64_t t = t0; t < t1; ++t)
          std::stable_sort(c->perm.begin() + tile_start[t], c->perm.begin() + tile_start[t + 1],
                           [&](int32_t l, int32_t r) { return kind[l] < kind[r]; });
      }, 16);
    }
  } else {
    pl::chunk_tiles(N, tile_start);
  }
  stage.mark("spatial order");
  c->iperm.resize(N);
  pl::parallel_for(N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int64_t i = i0; i < i1; ++i) c->iperm[c->perm[i]] = (int32_t)i;
  }, 1 << 16);
  if (o->condense >= 0 && o->precond >= 2 && o->precond <= 4 && o->precision != 2 && o->reorder == 1) {
    // Candidates for exact elimination inside the PCG (opts.condense): a greedy maximal independent set of the node
    // graph (no two share a strut; at least three struts each).  Inside every tile they are numbered LAST, so that the
    // vector kernels, which skip them, skip one contiguous run of rows per tile.
    std::vector<int64_t> aptr((size_t)N + 1, 0);
    pl::parallel_for(2 * B, [&](int64_t k0, int64_t k1, unsigned) {
      for (int64_t k = k0; k < k1; ++k)
        __atomic_fetch_add(&aptr[c->iperm[m->beam_conn[k]] + 1], (int64_t)1, __ATOMIC_RELAXED);
    }, 1 << 16);
    for (int64_t i = 0; i < N; ++i) aptr[i + 1] += aptr[i];
    std::vector<int32_t> adj((size_t)2 * B);
    {   // neighbour lists in any order: the greedy passes below only ask whether a neighbour is taken
      std::vector<int64_t> fill(aptr.begin(), aptr.end() - 1);
      pl::parallel_for(B, [&](int64_t b0, int64_t b1, unsigned) {
        for (int64_t b = b0; b < b1; ++b) {
          const int32_t u = c->iperm[m->beam_conn[2 * b]], v = c->iperm[m->beam_conn[2 * b + 1]];
          adj[__atomic_fetch_add(&fill[u], (int64_t)1, __ATOMIC_RELAXED)] = v;
          adj[__atomic_fetch_add(&fill[v], (int64_t)1, __ATOMIC_RELAXED)] = u;
        }
      }, 1 << 16);
    }
    // two greedy passes: nodes strictly inside the bounding box first, then the ones on it.  Boundary conditions sit
    // on the faces (a node with a Dirichlet dof cannot be eliminated) and face nodes have fewer struts; on BCC this
    // picks the cell centres rather than the corners (measured: 702 -> 468 iterations at 50^3 against 575 the other way)
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(lo[k], m->node_xyz[3 * i + k]);
        hi[k] = std::max(hi[k], m->node_xyz[3 * i + k]);
      }
    std::vector<uint8_t> state((size_t)N, 0);
    for (int pass = 0; pass < 2; ++pass)
      for (int64_t i = 0; i < N; ++i) {
        if (state[i] || aptr[i + 1] - aptr[i] < 3) continue;
        const double *q3 = m->node_xyz + 3 * (size_t)c->perm[i];
        const bool on_box = q3[0] <= lo[0] || q3[0] >= hi[0] || q3[1] <= lo[1] || q3[1] >= hi[1] || q3[2] <= lo[2] ||
                            q3[2] >= hi[2];
        if (on_box != (pass == 1)) continue;
        state[i] = 1;
        for (int64_t q = aptr[i]; q < aptr[i + 1]; ++q)
          if (!state[adj[q]]) state[adj[q]] = 2;
      }
    int64_t n_cand = 0;
    for (int64_t i = 0; i < N; ++i) n_cand += state[i] == 1;
    // automatic mode: only when close to half of the unknowns can go (bipartite node graphs such as BCC: measured
    // 1.1-1.2 x faster solves; Octet, a quarter of the nodes: 1.2 x slower - every iteration pays a second K*p)
    const bool use = o->condense > 0 || (double)n_cand >= 0.45 * (double)N;
    const int64_t T = use ? (int64_t)tile_start.size() - 1 : 0;
    std::vector<int32_t> np(c->perm.size());
    if (use) c->h_cand.assign((size_t)N, 0);
    for (int64_t t = 0; t < T; ++t) {
      int64_t w = tile_start[t];
      for (int pass = 0; pass < 2; ++pass)
        for (int64_t i = tile_start[t]; i < tile_start[t + 1]; ++i)
          if ((state[i] == 1) == (pass == 1)) {
            c->h_cand[w] = (uint8_t)pass;
            np[w++] = c->perm[i];
          }
    }
    if (use) {
      c->perm.swap(np);
      for (int64_t i = 0; i < N; ++i) c->iperm[c->perm[i]] = (int32_t)i;
    }
  }

  stage.mark("candidates");
  std::vector<double> xyz((size_t)N * 3);
  pl::parallel_for(N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int64_t i = i0; i < i1; ++i)
      std::memcpy(&xyz[3 * i], m->node_xyz + 3 * (size_t)c->perm[i], 3 * sizeof(double));
  });
  std::vector<int32_t> conn((size_t)B * 2);
  {
    std::vector<int32_t> conn0((size_t)B * 2);
    pl::parallel_for(2 * B, [&](int64_t k0, int64_t k1, unsigned) {
      for (int64_t k = k0; k < k1; ++k) conn0[k] = c->iperm[m->beam_conn[k]];
    });
    pl::tile_strut_order(conn0, N, B, tile_start, tile_of, c->bperm, xyz.data());
    pl::parallel_for(B, [&](int64_t b0, int64_t b1, unsigned) {
      for (int64_t b = b0; b < b1; ++b) {
        conn[2 * b] = conn0[2 * (size_t)c->bperm[b]];
        conn[2 * b + 1] = conn0[2 * (size_t)c->bperm[b] + 1];
      }
    });
  }
  stage.mark("strut order");
  std::vector<double> radius(B), seg_len((size_t)B * 3);
  std::vector<int32_t> seg_nsub((size_t)B * 3);
  pl::parallel_for(B, [&](int64_t b0, int64_t b1, unsigned) {
    for (int64_t b = b0; b < b1; ++b) {
      const size_t ob = (size_t)c->bperm[b];
      radius[b] = m->beam_radius[ob];
      for (int k = 0; k < 3; ++k) {
        seg_len[3 * b + k] = m->seg_len[3 * ob + k];
        seg_nsub[3 * b + k] = m->seg_nsub[3 * ob + k];
      }
    }
  });

  PL_HIPC(c->xyz.alloc(N * 3));
  PL_HIPC(c->conn.alloc(B * 2));
  PL_HIPC(c->radius.alloc(B));
  PL_HIPC(c->seg_len.alloc(B * 3));
  PL_HIPC(c->seg_nsub.alloc(B * 3));
  PL_HIPC(c->rec.alloc(B));
  // opts.compact_records (default on): the tile K*p streams 40-byte records when no palette applies
  if (o->compact_records >= 0 && (o->spmv_kernel == 0 || o->spmv_kernel == 3)) PL_HIPC(c->rec5.alloc((size_t)B * 5));
  PL_HIPC(hipMemcpy(c->xyz.p, xyz.data(), xyz.size() * sizeof(double), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->conn.p, conn.data(), conn.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->radius.p, radius.data(), B * sizeof(double), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->seg_len.p, seg_len.data(), 3 * B * sizeof(double), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->seg_nsub.p, seg_nsub.data(), 3 * B * sizeof(int32_t), hipMemcpyHostToDevice));
  stage.mark("permute + upload");
  PL_TRY(build_incidence(c, conn));
  stage.mark("incidence + BSR pattern");
  {
    int rc = pl::build_tile_plan(c->tile, conn, N, B, tile_start, tile_of, xyz.data());
    if (rc) return bail(fail(PL_ERR_HIP, "pl_create: building the LDS tile plan failed (" + std::to_string(rc) + ")"));
  }
  if (o->palette && c->tile.vis_ready && std::getenv("PL_ROWS")) {   // K*p by rows (pl_rows.h, opt-in): palette form only
    int rc = pl::build_row_plan(c->rows, conn, N, B, tile_start, xyz.data());
    if (rc) return bail(fail(PL_ERR_HIP, "pl_create: building the row plan failed (" + std::to_string(rc) + ")"));
  }
  c->h_tile_start = tile_start;
  stage.mark("tile + row plan");
  if (o->precond >= 2 && o->precond <= 4) {
    if (!c->reordered) return bail(fail(PL_ERR_ARG, "pl_create: precond = 2/3/4 (multi-level) needs reorder = 1"));
    c->coarse.tile_level = (o->precond >= 3);
    // 12-mode tile level (rigid + uniform strains): single-GPU handles in the ordinary CG form; opts.tile_modes = 6 keeps
    // the rigid-body blocks
    c->coarse.tile_modes = (o->tile_modes == 6 || o->precond == 4) ? 6 : 12;
    // default size of the dense level: its factorisation is a ~45 us-per-64-dofs latency chain in every assembly, its
    // benefit grows with the cost of an iteration - up to 1 M nodes on one GPU the optimum is ~2 000 dofs (measured on
    // 50^3 Octet: 7^3 aggregates 18.9 ms per step, 8^3 20.7 ms), beyond that and in multi-rank runs (collectives in
    // every iteration) the full 3 072
    const bool multi_rank = o->grid_nodes > 0;
    const int max_dofs = coarse_budget(o, N);
    int rc = pl::coarse_setup(c->coarse, tile_start, tile_brick, grid, xyz.data(), N, max_dofs, conn, false, multi_rank,
                              coarse_modes_of(o, N));
    if (rc == 4)
      return bail(fail(PL_ERR_ARG, "pl_create: a strut spans more than neighbouring aggregates; the band-packed "
                                   "all-reduce of the coarse operator of a multi-GPU handle cannot hold it (use "
                                   "precond = 1 or a smaller coarse_max_dofs)"));
    if (rc) return bail(fail(PL_ERR_HIP, "pl_create: coarse-space setup failed (" + std::to_string(rc) + ")"));
    if (o->coarse_storage != 0 && o->coarse_storage != 16 && o->coarse_storage != 32)
      return bail(fail(PL_ERR_ARG, "pl_create: coarse_storage must be 0 (automatic), 16 (bfloat16) or 32 (fp32)"));
    c->coarse.w16 = o->coarse_storage == 16 || (o->coarse_storage == 0 && c->coarse.ncp >= 1024);
    PL_HIPC(c->sharedbits.alloc(N));
    PL_HIPC(c->maskL.alloc(N));
    PL_HIPC(hipMemset(c->sharedbits.p, 0, N));
    if (o->precond == 4) {
      const int maxL = o->local_max_dofs > 0 ? o->local_max_dofs : 3072;
      rc = pl::coarse_setup(c->coarseL, tile_start, tile_brick, grid, xyz.data(), N, maxL, conn, true);
      if (rc) return bail(fail(PL_ERR_HIP, "pl_create: local coarse-space setup failed (" + std::to_string(rc) + ")"));
      c->coarseL.tile_level = false;
      c->coarseL.w16 = o->coarse_storage == 16 || (o->coarse_storage == 0 && c->coarseL.ncp >= 1024);
    }
  }

  stage.mark("coarse setup");
  const size_t n6 = (size_t)N * 6;
  PL_HIPC(c->fixed.alloc(n6));
  PL_HIPC(c->fixedbits.alloc(N));
  PL_HIPC(c->ubar.alloc(n6));
  PL_HIPC(c->f.alloc(n6));
  // (precond = 5: padded to the block size of the dense solver and zeroed - its GEMVs read / write whole blocks)
  const size_t vpad = o->precond == 5 ? (size_t)pl::kNB : 0;
  for (DevBuf<double> *v : {&c->diag, &c->dinv, &c->x, &c->r, &c->z, &c->p, &c->Ap, &c->tmp, &c->tmp2}) {
    PL_HIPC(v->alloc(n6 + vpad));
    if (vpad) PL_HIPC(hipMemset(v->p, 0, (n6 + vpad) * sizeof(double)));
  }
  PL_HIPC(c->scal.alloc(2 * pl::S_COUNT * pl::kSlots));   // two sets, selected by iteration parity
  PL_HIPC(hipMemset(c->fixed.p, 0, n6));
  PL_HIPC(hipMemset(c->fixedbits.p, 0, N));
  PL_HIPC(hipMemset(c->ubar.p, 0, n6 * sizeof(double)));
  PL_HIPC(hipMemset(c->f.p, 0, n6 * sizeof(double)));
  PL_HIPC(hipDeviceSynchronize());
#undef PL_TRY
#undef PL_HIPC
  stage.mark("vector buffers");
  *out = c;
  return PL_OK;
}

// Everything of a DDM handle that depends on WHICH matrix a cell uses (not on the matrix values): the cells sorted by matrix
// id (k_ddm_cell_product_lds), and the tiles of 16 cells of one class with their gather positions (k_ddm_cell_product_mfma).
static int ddm_build_classes(pl_context *c) {
  const int64_t n_cells = c->ddm_cells;
  const int nb = c->ddm_nb, m = 6 * nb;
  const int32_t *cell_S = c->h_ddm_cell_S.data(), *cell_nodes = c->h_ddm_cell_nodes.data();
  std::vector<int32_t> order((size_t)n_cells);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t l, int32_t r) { return cell_S[l] < cell_S[r]; });
  PL_HIP(c->ddm_order.alloc(order.size()));
  PL_HIP(hipMemcpy(c->ddm_order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  // tiles of 16 cells of one matrix class for the matrix-pipe product (k_ddm_cell_product_mfma)
  std::vector<int32_t> tiles, tile_S;
  for (size_t q = 0; q < order.size();) {
    const int32_t id = cell_S[order[q]];
    size_t e = q;
    while (e < order.size() && cell_S[order[e]] == id) ++e;
    for (size_t a = q; a < e; a += 16) {
      for (size_t k = 0; k < 16; ++k) tiles.push_back(a + k < e ? order[a + k] : -1);
      tile_S.push_back(id);
    }
    q = e;
  }
  c->ddm_n_tiles = (int64_t)tile_S.size();
  if (m <= 192) {
    const int KS = pl::ddm_mfma_ks(m);
    std::vector<int32_t> gidx((size_t)c->ddm_n_tiles * KS * 64, -1);
    for (int64_t t = 0; t < c->ddm_n_tiles; ++t)
      for (int kk = 0; kk < KS; ++kk)
        for (int lane = 0; lane < 64; ++lane) {
          const int32_t cell = tiles[16 * t + (lane & 15)];
          const int k = 4 * kk + (lane >> 4);
          if (cell >= 0 && k < m)
            gidx[((size_t)t * KS + kk) * 64 + lane] = 6 * cell_nodes[(int64_t)cell * nb + k / 6] + k % 6;
        }
    PL_HIP(c->ddm_tile_gidx.alloc(std::max<size_t>(1, gidx.size())));
    if (!gidx.empty())
      PL_HIP(hipMemcpy(c->ddm_tile_gidx.p, gidx.data(), gidx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  PL_HIP(c->ddm_tiles.alloc(std::max<size_t>(1, tiles.size())));
  PL_HIP(c->ddm_tile_S.alloc(std::max<size_t>(1, tile_S.size())));
  if (!tiles.empty()) {
    PL_HIP(hipMemcpy(c->ddm_tiles.p, tiles.data(), tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    PL_HIP(hipMemcpy(c->ddm_tile_S.p, tile_S.data(), tile_S.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return PL_OK;
}

// New cell matrices on an existing DDM handle (a design loop changes the radii, hence every S_c, between two solves; the
// topology - which nodes a cell couples - stays): uploads the palette again and, only when the cells' matrix ids changed,
// re-cuts the class tiles.  What it saves is pl_destroy + pl_create_ddm per design iteration (streams, events, a dozen
// allocations, the node -> cell incidence).  The preconditioner data of the handle is dropped: pl_assemble before pl_solve.
int pl_ddm_update_matrices(pl_handle h, int32_t n_S, const double *S, const int32_t *cell_S) {
  if (!valid(h) || !S || !cell_S || n_S <= 0) return fail(PL_ERR_ARG, "pl_ddm_update_matrices: bad argument");
  if (h->opkind != 1) return fail(PL_ERR_STATE, "pl_ddm_update_matrices: not a DDM handle");
  for (int64_t c = 0; c < h->ddm_cells; ++c)
    if (cell_S[c] < 0 || cell_S[c] >= n_S) return fail(PL_ERR_ARG, "pl_ddm_update_matrices: matrix id out of range");
  PL_HIP(hipSetDevice(h->opt.device));
  PL_HIP(hipStreamSynchronize(h->stream));
  const int m = 6 * h->ddm_nb;
  const size_t cnt = (size_t)n_S * m * m;
  if (h->ddm_St.n != cnt) PL_HIP(h->ddm_St.alloc(cnt));
  if (h->ddm_Sraw.n < cnt) PL_HIP(h->ddm_Sraw.alloc(cnt));
  PL_HIP(hipMemcpyAsync(h->ddm_Sraw.p, S, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(pl::k_ddm_transpose_palette, dim3(grid_for((int64_t)cnt)), dim3(pl::kBlock), 0, h->stream, (int64_t)n_S, m,
                     (const double *)h->ddm_Sraw.p, h->ddm_St.p);
  PL_HIP(hipStreamSynchronize(h->stream));
  PL_HIP(hipGetLastError());
  h->ddm_n_S = n_S;
  if (!std::equal(h->h_ddm_cell_S.begin(), h->h_ddm_cell_S.end(), cell_S)) {
    h->h_ddm_cell_S.assign(cell_S, cell_S + h->ddm_cells);
    PL_HIP(hipMemcpy(h->ddm_cell_S.p, cell_S, h->ddm_cells * sizeof(int32_t), hipMemcpyHostToDevice));
    int rc = ddm_build_classes(h);
    if (rc) return rc;
  }
  h->assembled = false;
  h->dd_ready = false;
  h->dd_blocks = false;
  h->dd2_ready = false;
  return PL_OK;
}

int pl_create_ddm(int64_t n_nodes, int64_t n_cells, int32_t nb, const int32_t *cell_nodes, int32_t n_S,
                  const double *S, const int32_t *cell_S, const pl_opts_t *o, pl_handle *out) {
  if (!cell_nodes || !S || !cell_S || !o || !out) return fail(PL_ERR_ARG, "pl_create_ddm: null argument");
  if (int rc_abi = check_opts_abi(o, "pl_create_ddm")) return rc_abi;
  if (n_nodes <= 0 || n_cells <= 0 || nb <= 0 || n_S <= 0) return fail(PL_ERR_ARG, "pl_create_ddm: empty problem");
  if (6 * nb > pl::kDdmMaxM) return fail(PL_ERR_ARG, "pl_create_ddm: more than 27 boundary nodes per cell");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PL_ERR_NODEVICE, "pl_create_ddm: no HIP device visible (libpylattice_hip has no CPU fallback)");
  if (o->device < 0 || o->device >= ndev) return fail(PL_ERR_ARG, "pl_create_ddm: bad device ordinal");
  for (int64_t k = 0; k < n_cells * nb; ++k)
    if (cell_nodes[k] < 0 || cell_nodes[k] >= n_nodes) return fail(PL_ERR_ARG, "pl_create_ddm: node id out of range");
  for (int64_t c = 0; c < n_cells; ++c)
    if (cell_S[c] < 0 || cell_S[c] >= n_S) return fail(PL_ERR_ARG, "pl_create_ddm: matrix id out of range");
  PL_HIP(hipSetDevice(o->device));
  pl_context *c = new pl_context();
  c->opt = *o;
  // 0: the reference's plain CG; 1: Jacobi on the assembled Schur diagonal; 2: the reference's own preconditioner, the
  // factorised assembled Schur matrix (dense Cholesky on the device, hence the size limit)
  c->opt.precond = (o->precond >= 1 && o->precond <= 4) ? o->precond : 0;     // 3: node-block Jacobi (6 x 6 blocks of G);
                                                                              // 4: + a dense level on node aggregates (pl_ddm_set_geometry)
  if (c->opt.precond == 2 && 6 * n_nodes > PL_DDM_DENSE_MAX) {
    delete c;
    return fail(PL_ERR_ARG, "pl_create_ddm: precond = 2 factorises a dense (6 n_nodes)^2 matrix; limit is " +
                                std::to_string(PL_DDM_DENSE_MAX) + " dofs (use precond = 3 or 1)");
  }
  c->opkind = 1;
  c->N = n_nodes;
  c->B = 0;
  c->ddm_cells = n_cells;
  c->ddm_nb = nb;
  {   // dofs coupled by a cell are at most 6 * (max - min node id) + 5 apart: the band of the assembled matrix
    int64_t span = 0;
    for (int64_t cc = 0; cc < n_cells; ++cc) {
      const int32_t *nd = cell_nodes + cc * nb;
      span = std::max<int64_t>(span, *std::max_element(nd, nd + nb) - *std::min_element(nd, nd + nb));
    }
    c->dd_bw = (int)((6 * span + 5) / pl::kNB + 1);
  }
  auto bail = [&](int rc) {
    delete c;
    return rc;
  };
#define PL_HIPC(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return bail(fail(PL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
  } while (0)
  {   // the main stream carries the latency-bound chains (dense factorisation, PCG): it goes ahead of the bulk fills
    int prio_low = 0, prio_high = 0;
    PL_HIPC(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    PL_HIPC(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_high));
    PL_HIPC(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_low));
  }
  PL_HIPC(hipEventCreate(&c->ev0));
  PL_HIPC(hipEventCreate(&c->ev1));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_chol, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_t0, hipEventDisableTiming));
  PL_HIPC(hipEventCreateWithFlags(&c->ev_t1, hipEventDisableTiming));
  PL_HIPC(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
  c->perm.resize(n_nodes);
  std::iota(c->perm.begin(), c->perm.end(), 0);
  c->iperm = c->perm;
  const int m = 6 * nb;
  std::vector<double> St((size_t)n_S * m * m);
  for (int s = 0; s < n_S; ++s)
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) St[((size_t)s * m + j) * m + i] = S[((size_t)s * m + i) * m + j];
  PL_HIPC(c->ddm_cell_nodes.alloc((size_t)n_cells * nb));
  PL_HIPC(c->ddm_cell_S.alloc(n_cells));
  PL_HIPC(c->ddm_St.alloc(St.size()));
  PL_HIPC(hipMemcpy(c->ddm_cell_nodes.p, cell_nodes, (size_t)n_cells * nb * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->ddm_cell_S.p, cell_S, n_cells * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIPC(hipMemcpy(c->ddm_St.p, St.data(), St.size() * sizeof(double), hipMemcpyHostToDevice));
  {
    if (n_cells * nb >= (1LL << 31)) return bail(fail(PL_ERR_ARG, "pl_create_ddm: more than 2^31 cell-node entries"));
    std::vector<int64_t> nptr((size_t)n_nodes + 1, 0);
    for (int64_t k = 0; k < n_cells * nb; ++k) nptr[cell_nodes[k] + 1]++;
    for (int64_t i = 0; i < n_nodes; ++i) nptr[i + 1] += nptr[i];
    std::vector<int32_t> nent((size_t)n_cells * nb);
    std::vector<int64_t> fill(nptr.begin(), nptr.end() - 1);
    for (int64_t k = 0; k < n_cells * nb; ++k) nent[fill[cell_nodes[k]]++] = (int32_t)k;   // cell-major: fixed sum order
    PL_HIPC(c->ddm_node_ptr.alloc(nptr.size()));
    PL_HIPC(c->ddm_node_ent.alloc(nent.size()));
    PL_HIPC(c->ddm_stage.alloc((size_t)n_cells * m));
    PL_HIPC(hipMemcpy(c->ddm_node_ptr.p, nptr.data(), nptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    PL_HIPC(hipMemcpy(c->ddm_node_ent.p, nent.data(), nent.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    c->h_ddm_cell_nodes.assign(cell_nodes, cell_nodes + n_cells * nb);
    c->h_ddm_cell_S.assign(cell_S, cell_S + n_cells);
    c->ddm_n_S = n_S;
    {
      int rcc = ddm_build_classes(c);
      if (rcc) return bail(rcc);
    }
  }
  const size_t n6 = (size_t)n_nodes * 6;
  PL_HIPC(c->fixed.alloc(n6));
  PL_HIPC(c->fixedbits.alloc(n_nodes));
  PL_HIPC(c->ubar.alloc(n6));
  PL_HIPC(c->f.alloc(n6));
  // (vectors padded to the block size of the dense solver and zeroed: its GEMVs read / write whole blocks)
  for (DevBuf<double> *v : {&c->diag, &c->dinv, &c->x, &c->r, &c->z, &c->p, &c->Ap, &c->tmp, &c->tmp2}) {
    PL_HIPC(v->alloc(n6 + pl::kNB));
    PL_HIPC(hipMemset(v->p, 0, (n6 + pl::kNB) * sizeof(double)));
  }
  PL_HIPC(c->scal.alloc(2 * pl::S_COUNT * pl::kSlots));
  PL_HIPC(hipMemset(c->fixed.p, 0, n6));
  PL_HIPC(hipMemset(c->fixedbits.p, 0, n_nodes));
  PL_HIPC(hipMemset(c->ubar.p, 0, n6 * sizeof(double)));
  PL_HIPC(hipMemset(c->f.p, 0, n6 * sizeof(double)));
  PL_HIPC(hipDeviceSynchronize());
#undef PL_HIPC
  *out = c;
  return PL_OK;
}

// Node positions of a DDM handle -> aggregates of the two-level preconditioner (opts.precond = 4): boxes of a regular grid over
// the bounding box, as many as opts.coarse_max_dofs / 12 allows (default 1 536 dofs = 128 aggregates) but at least ~27 nodes
// each, numbered with the longest axis slowest (narrow band of A_c); the band is taken from the cells themselves.
int pl_ddm_set_geometry(pl_handle h, const double *node_xyz) {
  if (!valid(h) || !node_xyz) return fail(PL_ERR_ARG, "pl_ddm_set_geometry: null argument");
  if (h->opkind != 1) return fail(PL_ERR_STATE, "pl_ddm_set_geometry: not a DDM handle");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  h->dd2_plan = false;
  h->dd2_ready = false;
  h->assembled = false;
  double lo[3], hi[3];
  for (int k = 0; k < 3; ++k) lo[k] = hi[k] = node_xyz[k];
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < 3; ++k) {
      const double v = node_xyz[3 * i + k];
      if (!std::isfinite(v)) return fail(PL_ERR_ARG, "pl_ddm_set_geometry: non-finite coordinate");
      lo[k] = std::min(lo[k], v);
      hi[k] = std::max(hi[k], v);
    }
  const int budget = h->opt.coarse_max_dofs > 0 ? h->opt.coarse_max_dofs : 1536;
  const int64_t n_target = std::max<int64_t>(1, std::min<int64_t>(budget / pl::kDdmModes, N / 27));
  double ext[3];
  for (int k = 0; k < 3; ++k) ext[k] = hi[k] - lo[k];
  const double emax = std::max(ext[0], std::max(ext[1], ext[2]));
  int64_t na[3] = {1, 1, 1};
  if (emax > 0.0) {     // boxes as close to cubes as the count allows: na_k ~ ext_k / side, side shrunk while the product fits
    double side = emax;
    for (int it = 0; it < 200; ++it) {
      int64_t t[3];
      for (int k = 0; k < 3; ++k) t[k] = std::max<int64_t>(1, (int64_t)std::floor(ext[k] / (side * 0.96) + 0.5));
      if (t[0] * t[1] * t[2] > n_target) break;
      for (int k = 0; k < 3; ++k) na[k] = t[k];
      side *= 0.96;
    }
  }
  const int n_agg = (int)(na[0] * na[1] * na[2]);
  int ax[3] = {0, 1, 2};
  std::stable_sort(ax, ax + 3, [&](int l, int r) { return na[l] > na[r]; });
  std::vector<int32_t> agg((size_t)N), ptr((size_t)n_agg + 1, 0), nodes((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    int64_t b[3];
    for (int k = 0; k < 3; ++k) {
      b[k] = ext[k] > 0.0 ? (int64_t)std::floor((node_xyz[3 * i + k] - lo[k]) / ext[k] * (double)na[k]) : 0;
      b[k] = std::min<int64_t>(std::max<int64_t>(b[k], 0), na[k] - 1);
    }
    agg[(size_t)i] = (int32_t)((b[ax[0]] * na[ax[1]] + b[ax[1]]) * na[ax[2]] + b[ax[2]]);
    ptr[(size_t)agg[(size_t)i] + 1]++;
  }
  for (int a = 0; a < n_agg; ++a) ptr[(size_t)a + 1] += ptr[(size_t)a];
  {
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t i = 0; i < N; ++i) nodes[(size_t)fill[(size_t)agg[(size_t)i]]++] = (int32_t)i;
  }
  std::vector<double> cen((size_t)n_agg * 3);
  for (int a = 0; a < n_agg; ++a) {
    int64_t b[3];
    b[ax[0]] = a / (na[ax[1]] * na[ax[2]]);
    b[ax[1]] = (a / na[ax[2]]) % na[ax[1]];
    b[ax[2]] = a % na[ax[2]];
    for (int k = 0; k < 3; ++k) cen[3 * (size_t)a + k] = lo[k] + ((double)b[k] + 0.5) * ext[k] / (double)na[k];
  }
  // band of A_c: the largest difference of aggregate numbers inside one cell
  std::vector<int32_t> cn((size_t)h->ddm_cells * h->ddm_nb);
  PL_HIP(hipMemcpy(cn.data(), h->ddm_cell_nodes.p, cn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t max_diff = 0;
  for (int64_t c = 0; c < h->ddm_cells; ++c) {
    int32_t amin = n_agg, amax = -1;
    for (int i = 0; i < h->ddm_nb; ++i) {
      const int32_t a = agg[(size_t)cn[(size_t)c * h->ddm_nb + i]];
      amin = std::min(amin, a);
      amax = std::max(amax, a);
    }
    max_diff = std::max<int64_t>(max_diff, amax - amin);
  }
  pl::Coarse &cs = h->dd2;
  const int nc = pl::kDdmModes * n_agg, ncp = (nc + pl::kNB - 1) / pl::kNB * pl::kNB;
  if (cs.ncp != ncp) {
    for (void **q : {(void **)&cs.Ac, (void **)&cs.Lf, (void **)&cs.W, (void **)&cs.Wt, (void **)&cs.Dinv, (void **)&cs.rc,
                     (void **)&cs.yc, (void **)&cs.tv, (void **)&cs.info, (void **)&cs.bar, (void **)&cs.Ainv})
      if (*q) {
        (void)hipFree(*q);
        *q = nullptr;
      }
    const size_t n2 = (size_t)ncp * ncp;
    PL_HIP(hipMalloc((void **)&cs.Ac, n2 * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.Lf, n2 * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.W, n2 * sizeof(float)));
    PL_HIP(hipMalloc((void **)&cs.Wt, n2 * sizeof(float)));
    PL_HIP(hipMalloc((void **)&cs.Dinv, (size_t)ncp * pl::kNB * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.rc, (size_t)(ncp + 2 * pl::kSlots) * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.yc, (size_t)ncp * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.tv, (size_t)ncp * sizeof(double)));
    PL_HIP(hipMalloc((void **)&cs.info, 2 * sizeof(int)));
    PL_HIP(hipMalloc((void **)&cs.bar, sizeof(unsigned)));
    if (ncp <= pl::kOneGemvMaxDofs) PL_HIP(hipMalloc((void **)&cs.Ainv, n2 * sizeof(float)));
    PL_HIP(hipMemset(cs.Lf, 0, n2 * sizeof(double)));
    PL_HIP(hipMemset(cs.W, 0, n2 * sizeof(float)));
    PL_HIP(hipMemset(cs.Wt, 0, n2 * sizeof(float)));
    PL_HIP(hipMemset(cs.rc, 0, (size_t)(ncp + 2 * pl::kSlots) * sizeof(double)));
    PL_HIP(hipMemset(cs.yc, 0, (size_t)ncp * sizeof(double)));
  }
  cs.n_agg = n_agg;
  cs.nc = nc;
  cs.ncp = ncp;
  cs.cm = pl::kDdmModes;
  cs.bw_blocks = (int)((pl::kDdmModes * (max_diff + 1) + pl::kNB - 1) / pl::kNB + 1);
  cs.w16 = h->opt.coarse_storage == 16 || (h->opt.coarse_storage == 0 && ncp >= 1024);
  cs.ainv_ready = false;
  h->dd2_n_agg = n_agg;
  PL_HIP(h->dd2_xyz.alloc((size_t)N * 3));
  PL_HIP(h->dd2_cen.alloc(cen.size()));
  PL_HIP(h->dd2_agg.alloc(agg.size()));
  PL_HIP(h->dd2_ptr.alloc(ptr.size()));
  PL_HIP(h->dd2_nodes.alloc(nodes.size()));
  PL_HIP(hipMemcpy(h->dd2_xyz.p, node_xyz, (size_t)N * 3 * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->dd2_cen.p, cen.data(), cen.size() * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->dd2_agg.p, agg.data(), agg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->dd2_ptr.p, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->dd2_nodes.p, nodes.data(), nodes.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  h->dd2_plan = true;
  return PL_OK;
}

int pl_ddm_set_preconditioner(pl_handle h, int32_t n_S, const double *S, const int32_t *cell_S) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_ddm_set_preconditioner: null handle");
  if (h->opkind != 1) return fail(PL_ERR_STATE, "pl_ddm_set_preconditioner: not a DDM handle");
  PL_HIP(hipSetDevice(h->opt.device));
  h->assembled = false;
  if (!S) {   // back to the operator's own matrices
    h->ddm_have_P = false;
    return PL_OK;
  }
  if (n_S <= 0 || !cell_S) return fail(PL_ERR_ARG, "pl_ddm_set_preconditioner: bad argument");
  for (int64_t c = 0; c < h->ddm_cells; ++c)
    if (cell_S[c] < 0 || cell_S[c] >= n_S) return fail(PL_ERR_ARG, "pl_ddm_set_preconditioner: matrix id out of range");
  const int m = 6 * h->ddm_nb;
  std::vector<double> Pt((size_t)n_S * m * m);
  for (int s = 0; s < n_S; ++s)
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) Pt[((size_t)s * m + j) * m + i] = S[((size_t)s * m + i) * m + j];
  PL_HIP(h->ddm_Pt.alloc(Pt.size()));
  PL_HIP(h->ddm_cell_P.alloc(h->ddm_cells));
  PL_HIP(hipMemcpy(h->ddm_Pt.p, Pt.data(), Pt.size() * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->ddm_cell_P.p, cell_S, h->ddm_cells * sizeof(int32_t), hipMemcpyHostToDevice));
  h->ddm_have_P = true;
  return PL_OK;
}

// G = sum_c B^T Shat B on the free dofs (unit diagonal elsewhere), Cholesky + explicit inverse factor on the device.
static int ensure_bsr_buffers(pl_context *h) {
  if (h->bsr_vals.p) return PL_OK;
  PL_HIP(h->bsr_rowptr.alloc(h->N + 1));
  PL_HIP(h->bsr_col.alloc(h->nblk));
  PL_HIP(h->bsr_vals.alloc((size_t)h->nblk * 36));
  PL_HIP(hipMemcpy(h->bsr_rowptr.p, h->h_rowptr.data(), (h->N + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->bsr_col.p, h->h_col.data(), h->nblk * sizeof(int32_t), hipMemcpyHostToDevice));
  return PL_OK;
}

static int ddm_factor_preconditioner(pl_context *h) {
  const int64_t n6 = h->N * 6;
  const int np = (int)((n6 + pl::kNB - 1) / pl::kNB * pl::kNB);
  if (h->dd_n != np) {
    const size_t nn = (size_t)np * np;
    PL_HIP(h->dd_A.alloc(nn));
    PL_HIP(h->dd_Lf.alloc(nn));
    PL_HIP(h->dd_W.alloc(nn));
    PL_HIP(h->dd_Wt.alloc(nn));
    PL_HIP(h->dd_Dinv.alloc((size_t)np * pl::kNB));
    PL_HIP(h->dd_tv.alloc(np));
    PL_HIP(h->dd_info.alloc(2));
    PL_HIP(hipMemsetAsync(h->dd_W.p, 0, nn * sizeof(double), h->stream));
    PL_HIP(hipMemsetAsync(h->dd_Wt.p, 0, nn * sizeof(double), h->stream));
    h->dd_n = np;
  }
  h->dd_ready = false;
  PL_HIP(hipMemsetAsync(h->dd_A.p, 0, (size_t)np * np * sizeof(double), h->stream));
  PL_HIP(hipMemsetAsync(h->dd_info.p, 0, 2 * sizeof(int), h->stream));
  const int m = 6 * h->ddm_nb;
  const int64_t ne = h->ddm_cells * m * m;
  const uint8_t *fx = h->have_bc ? h->fixed.p : (const uint8_t *)nullptr;
  hipLaunchKernelGGL(pl::k_ddm_dense_assemble, dim3(grid_for(ne)), dim3(pl::kBlock), 0, h->stream, h->ddm_cells,
                     h->ddm_nb, h->ddm_cell_nodes.p, h->ddm_have_P ? h->ddm_cell_P.p : h->ddm_cell_S.p,
                     h->ddm_have_P ? h->ddm_Pt.p : h->ddm_St.p, fx, np, h->dd_A.p);
  hipLaunchKernelGGL(pl::k_ddm_dense_unit, dim3((np + 255) / 256), dim3(256), 0, h->stream, n6, np, fx, h->dd_A.p);
  pl::dense_factor_inverse(h->dd_A.p, h->dd_Lf.p, h->dd_W.p, h->dd_Wt.p, h->dd_Dinv.p, np, np, h->dd_info.p,
                           h->dd_bw, h->stream);
  PL_HIP(hipGetLastError());
  int info[2] = {0, 0};
  PL_HIP(hipMemcpyAsync(info, h->dd_info.p, sizeof(info), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  h->dd_ready = (info[0] == 0);   // not positive definite (e.g. an indefinite surrogate matrix): caller falls back
  return PL_OK;
}

// precond = 5 on a strut-operator handle: P K P + (I - P) as a dense matrix from the BSR(6 x 6) blocks, factorised by the same
// device Cholesky as the DDM path's assembled Schur matrix (fp64 inverse factor); the PCG then converges in one or two
// iterations.  What PETSc's preonly / LU is to the reference (simulation_base.py:501-511), for lattices of a few hundred
// nodes - the sizes of the reference's own presets - where hundreds of PCG iterations cost more than the factorisation.
static int fem_factor_dense(pl_context *h) {
  const int64_t n6 = h->N * 6;
  const int np = (int)((n6 + pl::kNB - 1) / pl::kNB * pl::kNB);
  if (h->dd_n != np) {
    const size_t nn = (size_t)np * np;
    PL_HIP(h->dd_A.alloc(nn));
    PL_HIP(h->dd_Lf.alloc(nn));
    PL_HIP(h->dd_W.alloc(nn));
    PL_HIP(h->dd_Wt.alloc(nn));
    PL_HIP(h->dd_Dinv.alloc((size_t)np * pl::kNB));
    PL_HIP(h->dd_tv.alloc(np));
    PL_HIP(h->dd_info.alloc(2));
    PL_HIP(hipMemsetAsync(h->dd_W.p, 0, nn * sizeof(double), h->stream));
    PL_HIP(hipMemsetAsync(h->dd_Wt.p, 0, nn * sizeof(double), h->stream));
    h->dd_n = np;
    // block bandwidth of K in the device numbering (spatial tiles: a banded matrix)
    int64_t band = 0;
    for (int64_t i = 0; i < h->N; ++i)
      for (int64_t q = h->h_rowptr[i]; q < h->h_rowptr[i + 1]; ++q) band = std::max<int64_t>(band, std::llabs((long long)(h->h_col[q] - i)));
    h->dd_bw = (int)((6 * (band + 1) + pl::kNB - 1) / pl::kNB + 1);
  }
  h->dd_ready = false;
  int rc = ensure_bsr_buffers(h);
  if (rc) return rc;
  PL_HIP(hipMemsetAsync(h->dd_A.p, 0, (size_t)np * np * sizeof(double), h->stream));
  PL_HIP(hipMemsetAsync(h->dd_info.p, 0, 2 * sizeof(int), h->stream));
  rc = launch_bsr_fill(h, 1, h->stream);            // dolfinx's Dirichlet treatment: constrained rows / columns zero, unit diagonal
  if (rc) return rc;
  h->have_bsr = false;                              // (the caller's explicit matrix, if any, is refreshed by pl_assemble)
  hipLaunchKernelGGL(pl::k_bsr_to_dense, dim3(grid_for(h->nblk * 36)), dim3(pl::kBlock), 0, h->stream, h->N, h->nblk,
                     h->bsr_rowptr.p, h->bsr_col.p, (const double *)h->bsr_vals.p, np, h->dd_A.p);
  hipLaunchKernelGGL(pl::k_ddm_dense_unit, dim3((np + 255) / 256), dim3(256), 0, h->stream, n6, np, (const uint8_t *)nullptr,
                     h->dd_A.p);
  pl::dense_factor_inverse(h->dd_A.p, h->dd_Lf.p, h->dd_W.p, h->dd_Wt.p, h->dd_Dinv.p, np, np, h->dd_info.p, h->dd_bw,
                           h->stream);
  PL_HIP(hipGetLastError());
  int info[2] = {0, 0};
  PL_HIP(hipMemcpyAsync(info, h->dd_info.p, sizeof(info), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  h->dd_ready = (info[0] == 0);   // not positive definite (a mechanism): the solve falls back to Jacobi
  if (h->dd_ready) PL_HIP(hipMemsetAsync(h->dinv.p, 0, n6 * sizeof(double), h->stream));     // z comes from the dense solve
  return PL_OK;
}

void pl_destroy(pl_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->opt.device);
  (void)hipStreamSynchronize(h->stream);
  if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
  pl::dist_destroy(h->dist);
  if (h->pal_host_flags != h->pal_fallback_flags) (void)hipHostFree(h->pal_host_flags);
  if (h->cls_host_flag) (void)hipHostFree(h->cls_host_flag);
  if (h->dcl_host_flags) (void)hipHostFree(h->dcl_host_flags);
  delete h;
}

int pl_set_bc(pl_handle h, const uint8_t *fixed, const double *ubar, const double *f) {
  if (!valid(h) || !fixed) return fail(PL_ERR_ARG, "pl_set_bc: null argument");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  const size_t n6 = (size_t)N * 6;
  std::vector<uint8_t> fx(n6), bits(N);
  double *st = nullptr;          // ubar, then f, through the handle's pinned staging buffer
  if (int rcs = staging(h, &st)) return rcs;
  pl::parallel_for(N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int64_t i = i0; i < i1; ++i) {
      const size_t src = 6 * (size_t)h->perm[i];
      uint8_t b = 0;
      for (int k = 0; k < 6; ++k) {
        const uint8_t v = fixed[src + k] ? 1 : 0;
        fx[6 * i + k] = v;
        b |= (uint8_t)(v << k);
        st[6 * i + k] = (ubar && v) ? ubar[src + k] : 0.0;
      }
      bits[i] = b;
    }
  }, 1 << 15);
  PL_HIP(hipMemcpyAsync(h->ubar.p, st, n6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipMemcpyAsync(h->fixed.p, fx.data(), n6, hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipMemcpyAsync(h->fixedbits.p, bits.data(), N, hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  pl::parallel_for(N, [&](int64_t i0, int64_t i1, unsigned) {
    for (int64_t i = i0; i < i1; ++i) {
      const size_t src = 6 * (size_t)h->perm[i];
      for (int k = 0; k < 6; ++k) st[6 * i + k] = f ? f[src + k] : 0.0;
    }
  }, 1 << 15);
  PL_HIP(hipMemcpyAsync(h->f.p, st, n6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  // The same Dirichlet set as before (only prescribed values / loads changed - the columns of pl_schur, the adjoint solves of
  // a design loop): everything that depends on the mask (Jacobi inverse, coarse levels, eliminated nodes, dense factor) stands
  const bool same_mask = h->have_bc && !h->dist.active && h->h_fixedbits == bits;
  h->h_fixedbits = bits;
  if (same_mask) return PL_OK;
  h->have_bc = true;
  h->coarse.n_fix = -1;
  h->coarseL.n_fix = -1;
  h->coarse.dcl_ready = false;     // (the classes of the Jacobi weights carry the mask: rebuilt with dinv32 below / in pl_assemble)
  {
    int rcs = select_condensed(h, bits);
    if (rcs) return rcs;
  }
  if (h->assembled && h->opkind == 1) {
    if (h->opt.precond >= 2 && h->opt.precond <= 4) {
      // the factorised G / the node blocks (and the dense level on top of them) were built for the old Dirichlet mask (and
      // dinv must stay 0 next to them): build them again
      h->assembled = false;
      h->dd_ready = false;
      h->dd_blocks = false;
      h->dd2_ready = false;
    } else {
      pl::launch_invert_diag(h->N * 6, h->diag.p, h->fixed.p, h->dinv.p, h->stream);
      PL_HIP(hipStreamSynchronize(h->stream));
    }
  } else if (h->assembled) {   // the Jacobi inverse and the coarse operator depend on the mask
    int rc = launch_diag(h, h->stream);
    if (rc) return rc;
    rc = finish_diag_dist(h);
    if (rc) return rc;
    rc = launch_local_mask(h);
    if (rc) return rc;
    rc = launch_tile_blocks(h, h->stream);
    if (rc) return rc;
    rc = build_coarse(h);
    if (rc) return rc;
    rc = launch_dinv32(h);
    if (rc) return rc;
    rc = launch_node_classes(h, h->stream, false);      // (dinv32 was written just above)
    if (rc) return rc;
    rc = agree_condensed(h);
    if (rc) return rc;
    rc = launch_condensed_blocks(h, h->stream);
    if (rc) return rc;
    PL_HIP(hipStreamSynchronize(h->stream));
    finish_node_classes(h);
    {
      const bool keep = h->pal_ready;        // (the record palette is untouched by a new mask)
      finish_condensed_classes(h);
      (void)keep;
    }
    if (h->bsr_with_bc) h->have_bsr = false;   // an explicit matrix built with the old mask is stale
    if (h->opt.precond == 5 && !h->dist.active) {   // the dense factor depends on the mask
      rc = fem_factor_dense(h);
      if (rc) return rc;
    }
  }
  return PL_OK;
}

int pl_set_periodic(pl_handle h, const int32_t *master) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_periodic: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_periodic: not available on a DDM handle");
  h->n_per_groups = 0;
  if (!master) return PL_OK;
  if (h->opt.precond != 1 || h->dist.active)
    return fail(PL_ERR_STATE, "pl_set_periodic: periodic constraints are served by the Jacobi PCG of a single-GPU handle (opts.precond = 1)");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  std::vector<int32_t> inv((size_t)N);
  for (int64_t i = 0; i < N; ++i) inv[(size_t)h->perm[i]] = (int32_t)i;          // caller node -> device node
  std::vector<int32_t> cnt((size_t)N, 0);
  for (int64_t i = 0; i < N; ++i) {
    const int32_t m = master[i];
    if (m < 0 || m >= N || master[m] != m) return fail(PL_ERR_ARG, "pl_set_periodic: master[i] must name a node that is its own master");
    cnt[(size_t)m]++;
  }
  std::vector<int32_t> ptr(1, 0), nodes, start((size_t)N, -1);
  for (int64_t m = 0; m < N; ++m)
    if (cnt[(size_t)m] >= 2) {
      start[(size_t)m] = (int32_t)ptr.size() - 1;
      ptr.push_back(ptr.back() + cnt[(size_t)m]);
    }
  nodes.resize((size_t)ptr.back());
  std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (int64_t i = 0; i < N; ++i) {
    const int32_t g = start[(size_t)master[i]];
    if (g >= 0) nodes[(size_t)fill[(size_t)g]++] = inv[(size_t)i];
  }
  const int64_t ng = (int64_t)ptr.size() - 1;
  if (ng == 0) return PL_OK;
  PL_HIP(h->per_ptr.alloc(ptr.size()));
  PL_HIP(h->per_nodes.alloc(nodes.size()));
  PL_HIP(hipMemcpy(h->per_ptr.p, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->per_nodes.p, nodes.data(), nodes.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  h->n_per_groups = ng;
  return PL_OK;
}

int pl_update_radii(pl_handle h, const double *beam_radius) {
  if (!valid(h) || !beam_radius) return fail(PL_ERR_ARG, "pl_update_radii: null argument");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_update_radii: not available on a DDM handle");
  for (int64_t b = 0; b < h->B; ++b)
    if (!(beam_radius[b] > 0.0)) return fail(PL_ERR_ARG, "pl_update_radii: non-positive radius");
  PL_HIP(hipSetDevice(h->opt.device));
  double *stg = nullptr;
  int rc = stagingB(h, &stg);
  if (rc) return rc;
  pl::parallel_for(h->B, [&](int64_t b0, int64_t b1, unsigned) {
    for (int64_t b = b0; b < b1; ++b) stg[b] = beam_radius[h->bperm[b]];
  }, 1 << 16);
  PL_HIP(hipMemcpyAsync(h->radius.p, stg, h->B * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  h->assembled = false;
  h->coarse.dcl_ready = false;     // the Jacobi weights are stale, and their classes with them
  h->have_bsr = false;
  return PL_OK;
}

int pl_set_multiplicity(pl_handle h, const double *beam_mult) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_multiplicity: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_multiplicity: not available on a DDM handle");
  PL_HIP(hipSetDevice(h->opt.device));
  if (!beam_mult) {
    h->mult.release();
  } else {
    for (int64_t b = 0; b < h->B; ++b)
      if (!(beam_mult[b] > 0.0)) return fail(PL_ERR_ARG, "pl_set_multiplicity: non-positive multiplicity");
    std::vector<double> m(h->B);
    for (int64_t b = 0; b < h->B; ++b) m[b] = beam_mult[h->bperm[b]];
    if (!h->mult.p) PL_HIP(h->mult.alloc(h->B));
    PL_HIP(hipMemcpy(h->mult.p, m.data(), h->B * sizeof(double), hipMemcpyHostToDevice));
  }
  h->assembled = false;
  h->coarse.dcl_ready = false;     // the Jacobi weights are stale, and their classes with them
  h->have_bsr = false;
  return PL_OK;
}

int pl_update_segments(pl_handle h, const double *seg_len, const int32_t *seg_nsub) {
  if (!valid(h) || !seg_len || !seg_nsub) return fail(PL_ERR_ARG, "pl_update_segments: null argument");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<double> sl((size_t)h->B * 3);
  std::vector<int32_t> sn((size_t)h->B * 3);
  for (int64_t b = 0; b < h->B; ++b)
    for (int k = 0; k < 3; ++k) {
      sl[3 * b + k] = seg_len[3 * (size_t)h->bperm[b] + k];
      sn[3 * b + k] = seg_nsub[3 * (size_t)h->bperm[b] + k];
    }
  PL_HIP(hipMemcpy(h->seg_len.p, sl.data(), 3 * h->B * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(h->seg_nsub.p, sn.data(), 3 * h->B * sizeof(int32_t), hipMemcpyHostToDevice));
  h->assembled = false;
  h->coarse.dcl_ready = false;     // the Jacobi weights are stale, and their classes with them
  h->have_bsr = false;
  return PL_OK;
}

int pl_assemble(pl_handle h) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_assemble: null handle");
  PL_HIP(hipSetDevice(h->opt.device));
  if (h->opkind == 1) {   // DDM operator: nothing to build; plain CG as the reference, Jacobi, or the factorised matrix
    // (everything that changes what is built here - pl_set_bc with another Dirichlet set, pl_ddm_update_matrices,
    //  pl_ddm_set_preconditioner, pl_ddm_set_geometry - clears `assembled`: a second call on an unchanged handle, e.g. solve_DDM
    //  for another load case, has nothing to do.  32^3 cells: 1.6 of the 9.5 ms of a repeated solve_DDM)
    if (h->assembled && (h->opt.precond == 0 || (h->opt.precond == 1 && !h->dd_ready && !h->dd_blocks) || h->dd_ready || h->dd_blocks)) {
      h->ms_assembly = 0.0;
      return PL_OK;
    }
    h->dd_ready = false;
    h->dd_blocks = false;
    h->dd2_ready = false;
    if (h->opt.precond == 4 && !h->dd2_plan)
      return fail(PL_ERR_STATE, "pl_assemble: precond = 4 on a DDM handle needs the node positions (pl_ddm_set_geometry)");
    if (h->opt.precond == 3 || h->opt.precond == 4) {      // node-block Jacobi: the 6 x 6 diagonal blocks of the assembled matrix, inverted
      PL_HIP(hipEventRecord(h->ev0, h->stream));
      if (!h->dd_B.p) PL_HIP(h->dd_B.alloc((size_t)h->N * 36));
      PL_HIP(hipMemsetAsync(h->dd_B.p, 0, (size_t)h->N * 36 * sizeof(double), h->stream));
      const int64_t ne = (int64_t)h->ddm_cells * h->ddm_nb * 36;
      hipLaunchKernelGGL(pl::k_ddm_node_blocks, dim3(grid_for(ne)), dim3(pl::kBlock), 0, h->stream, h->ddm_cells, h->ddm_nb,
                         h->ddm_cell_nodes.p, h->ddm_have_P ? h->ddm_cell_P.p : h->ddm_cell_S.p,
                         h->ddm_have_P ? h->ddm_Pt.p : h->ddm_St.p, h->dd_B.p);
      hipLaunchKernelGGL(pl::k_ddm_node_blocks_invert, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N,
                         h->have_bc ? (const uint8_t *)h->fixed.p : (const uint8_t *)nullptr, h->dd_B.p);
      PL_HIP(hipMemsetAsync(h->dinv.p, 0, h->N * 6 * sizeof(double), h->stream));      // z comes from the node blocks
      int info2[2] = {0, 0};
      if (h->opt.precond == 4) {    // + the dense level: A_c = Z^T P G P Z cell by cell, Cholesky + inverse factor (pl_dense.h)
        pl::Coarse &cs = h->dd2;
        const int n = cs.ncp, m = 6 * h->ddm_nb;
        PL_HIP(hipMemsetAsync(cs.Ac, 0, (size_t)n * n * sizeof(double), h->stream));
        PL_HIP(hipMemsetAsync(cs.info, 0, 2 * sizeof(int), h->stream));
        hipLaunchKernelGGL(pl::k_ddm_coarse_cells, dim3((unsigned)h->ddm_cells), dim3(pl::kWave),
                           (size_t)2 * m * pl::kDdmModes * sizeof(double), h->stream, h->ddm_cells, h->ddm_nb,
                           h->ddm_cell_nodes.p, h->ddm_have_P ? h->ddm_cell_P.p : h->ddm_cell_S.p,
                           h->ddm_have_P ? h->ddm_Pt.p : h->ddm_St.p, h->dd2_agg.p, h->dd2_cen.p, h->dd2_xyz.p,
                           h->have_bc ? (const uint8_t *)h->fixed.p : (const uint8_t *)nullptr, n, cs.Ac);
        hipLaunchKernelGGL(pl::k_coarse_regularize, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, cs.Ac);
        pl::TrtriPhases ph;          // the inverse factor in row ranges on a second stream, behind the chain (as pl_assembly.h)
        ph.rows = 3;
        ph.stream = h->side2;
        ph.ev_go = h->ev_t0;
        ph.ev_done = h->ev_t1;
        pl::coarse_factor(cs, n, h->stream, nullptr, (unsigned *)nullptr, ph);
        cs.ainv_ready = false;
        if (cs.Ainv) {
          if (cs.w16) pl::dense_explicit_inverse(n, reinterpret_cast<const pl::bf16_t *>(cs.W), n, cs.Ainv, h->stream);
          else pl::dense_explicit_inverse(n, (const float *)cs.W, n, cs.Ainv, h->stream);
          cs.ainv_ready = true;
        }
        PL_HIP(hipMemcpyAsync(info2, cs.info, sizeof(info2), hipMemcpyDeviceToHost, h->stream));
      }
      PL_HIP(hipEventRecord(h->ev1, h->stream));
      PL_HIP(hipEventSynchronize(h->ev1));
      PL_HIP(hipGetLastError());
      float ms = 0.f;
      PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
      h->ms_assembly = ms;
      h->dd2_ready = h->opt.precond == 4 && info2[0] == 0;     // (A_c not positive definite: the node blocks alone; precond_used = 3)
      h->dd_blocks = true;
      h->assembled = true;
      return PL_OK;
    }
    if (h->opt.precond == 2) {
      PL_HIP(hipEventRecord(h->ev0, h->stream));
      int rcp = ddm_factor_preconditioner(h);
      if (rcp) return rcp;
      if (h->dd_ready) {
        PL_HIP(hipMemsetAsync(h->dinv.p, 0, h->N * 6 * sizeof(double), h->stream));   // z comes from the dense solve
        PL_HIP(hipEventRecord(h->ev1, h->stream));
        PL_HIP(hipEventSynchronize(h->ev1));
        float ms = 0.f;
        PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        h->ms_assembly = ms;
        h->assembled = true;
        return PL_OK;
      }
      // G is not positive definite (the reference falls back from LU to ILU when its factorisation fails,
      // lattice_sim.py:1406-1413): Jacobi on the assembled diagonal; pl_stats_t.precond_used tells the caller
    }
    if (h->opt.precond >= 1) {
      PL_HIP(hipMemsetAsync(h->diag.p, 0, h->N * 6 * sizeof(double), h->stream));
      const int64_t m = (int64_t)h->ddm_cells * h->ddm_nb * 6;
      hipLaunchKernelGGL(pl::k_ddm_diag, dim3(grid_for(m)), dim3(pl::kBlock), 0, h->stream, h->ddm_cells, h->ddm_nb,
                         h->ddm_cell_nodes.p, h->ddm_cell_S.p, h->ddm_St.p, h->diag.p);
    } else {
      pl::launch_fill(h->N * 6, 1.0, h->diag.p, h->stream);
    }
    pl::launch_invert_diag(h->N * 6, h->diag.p, h->have_bc ? h->fixed.p : nullptr, h->dinv.p, h->stream);
    PL_HIP(hipStreamSynchronize(h->stream));
    h->ms_assembly = 0.0;
    h->assembled = true;
    return PL_OK;
  }
  int rc = agree_condensed(h);      // (multi-GPU, first assembly after a pl_set_bc: a host round trip, outside the timing)
  if (rc) return rc;
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  rc = launch_records(h);
  if (rc) return rc;
  rc = launch_local_mask(h);
  if (rc) return rc;
  // fork: everything that only streams the records runs on the side stream while the main stream walks the
  // latency-bound chain of the coarse factorisation
  PL_HIP(hipEventRecord(h->ev_fork, h->stream));
  PL_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  rc = launch_palette(h, h->side);
  if (rc) return rc;
  rc = launch_diag(h, h->dist.active ? h->stream : h->side);
  if (rc) return rc;
  rc = finish_diag_dist(h);
  if (rc) return rc;
  rc = launch_tile_blocks(h, h->side);
  if (rc) return rc;
  rc = launch_condensed_blocks(h, h->side);
  if (rc) return rc;
  const bool refresh_bsr = h->want_bsr && (!h->bsr_with_bc || h->have_bc);
  // The explicit K is the one bulk item of the assembly (2.5 GB of traffic): next to the Cholesky chain it slows every
  // link of that latency-bound chain (44 -> 57 us), so it starts when the chain's last link is queued and runs beside
  // the single-launch inverse factor instead.
  int rc_fill = PL_OK;
  bool fill_queued = false;
  // How much of the fill fits beside the chain: the masked stream fills 7 - 9 M blocks per millisecond (50^3 Octet: 6.6 M blocks in
  // 0.72 ms; 100^3 BCC: 18 M in 2.6 ms), a link of the chain takes ~40 us.  What does not fit (200 x 200 x 50 BCC + Octet:
  // 138 M blocks against a 3.8-ms chain - all of it on the masked half of the chip cost 7 ms) runs behind the chain on the
  // plain side stream, on the whole chip, as until round 4.
  int64_t split = 0;            // slices [0, split) beside the chain
  if (refresh_bsr && h->side_cu && h->coarse.enabled && h->have_bc) {
    // (PL_CHAIN_LINK_MS / PL_FILL_BLOCKS_PER_MS: the two measured rates, for A/B runs on another box)
    static const double kChainLinkMs = [] { const char *e = std::getenv("PL_CHAIN_LINK_MS"); return e ? std::atof(e) : 0.04; }();
    static const double kFillBlocksPerMs = [] { const char *e = std::getenv("PL_FILL_BLOCKS_PER_MS"); return e ? std::atof(e) : 8.5e6; }();
    const double chain_ms = kChainLinkMs * std::max(0, h->coarse.ncp / pl::kNB - 1);
    const double fit = chain_ms * kFillBlocksPerMs / std::max<double>(1.0, (double)h->nblk);
    split = fit >= 1.0 ? h->n_slices : (int64_t)(fit * (double)h->n_slices);
    if (split < h->n_slices / 16) split = 0;         // (not worth a launch)
  }
  bool part1_queued = false;
  auto queue_fill = [&](int phase) {
    if (!refresh_bsr || fill_queued) return;
    if (phase == 0) {              // head of the chain: the part that fits beside it, on the stream that leaves it CUs
      if (split <= 0 || part1_queued) return;
      part1_queued = true;
      if (hipEventRecord(h->ev_chol, h->stream) != hipSuccess || hipStreamWaitEvent(h->side_cu, h->ev_chol, 0) != hipSuccess ||
          hipStreamWaitEvent(h->side_cu, h->ev_join, 0) != hipSuccess) {
        rc_fill = fail(PL_ERR_HIP, "pl_assemble: could not order the BSR fill beside the factorisation");
        return;
      }
      rc_fill = launch_bsr_fill(h, h->bsr_with_bc, h->side_cu, 0, split);
      if (hipEventRecord(h->ev_fill1, h->side_cu) != hipSuccess) rc_fill = fail(PL_ERR_HIP, "pl_assemble: event record failed");
      return;
    }
    fill_queued = true;            // behind the chain: the rest (everything without a masked stream), on the whole chip
    if (hipEventRecord(h->ev_chol, h->stream) != hipSuccess || hipStreamWaitEvent(h->side, h->ev_chol, 0) != hipSuccess) {
      rc_fill = fail(PL_ERR_HIP, "pl_assemble: could not order the BSR fill behind the factorisation");
      return;
    }
    if (!rc_fill) rc_fill = launch_bsr_fill(h, h->bsr_with_bc, h->side, part1_queued ? split : 0, -1);
    if (part1_queued && hipStreamWaitEvent(h->side, h->ev_fill1, 0) != hipSuccess)
      rc_fill = fail(PL_ERR_HIP, "pl_assemble: event wait failed");
    if (hipEventRecord(h->ev_join, h->side) != hipSuccess) rc_fill = fail(PL_ERR_HIP, "pl_assemble: event record failed");
  };
  // (round 3, tried: the fill queued HERE, beside the tile-block front of the assembly instead of behind the chain's last
  // link: assembly 2.27 -> 2.46 ms in two alternating pairs of runs - it slows the front and the first links)
  PL_HIP(hipEventRecord(h->ev_join, h->side));
  h->dd_ready = false;
  if (h->opt.precond == 5 && h->have_bc && !h->dist.active) {
    PL_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));       // (the Jacobi diagonal first: the fallback, and dinv is cleared after)
    rc = fem_factor_dense(h);
    if (rc) return rc;
  }
  // The classes of the Jacobi weights (node words) run on the side stream, behind the diagonal - but their launches are
  // QUEUED only here, from the callback at the head of the chain, when the front of the chain is already queued on the main
  // stream: queued ahead of it they held the host back and the chain started 100 us later (profiles/README.md,
  // r12_node_words_timeline).  ev_join moves behind them, so that everything that waits for the side stream waits for them.
  bool dcl_queued = false;
  int rc_dcl = PL_OK;
  auto beside_chain = [&](int phase) {
    if (!dcl_queued) {
      dcl_queued = true;
      rc_dcl = launch_node_classes(h, h->side, true);
      if (!rc_dcl && hipEventRecord(h->ev_join, h->side) != hipSuccess)
        rc_dcl = fail(PL_ERR_HIP, "pl_assemble: event record failed");
    }
    queue_fill(phase);
  };
  rc = build_coarse(h, h->coarse.enabled && h->have_bc ? std::function<void(int)>(beside_chain) : std::function<void(int)>());
  if (rc) return rc;
  if (rc_dcl) return rc_dcl;
  queue_fill(1);                                 // (no dense level: queue it now)
  if (rc_fill) return rc_fill;
  PL_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  if (!h->dcl_pending) {      // (a queued classification has written dinv32 itself, on the side stream, and verified against it)
    rc = launch_dinv32(h);
    if (rc) return rc;
  }
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  finish_palette(h);
  finish_condensed_classes(h);
  finish_node_classes(h);
  // the factorisation has consumed A_c: zero it now, behind the caller's back, instead of at the head of the next
  // assembly's critical chain (34 MB; it would sit in front of the coarse assembly there)
  for (pl::Coarse *cs : {&h->coarse, &h->coarseL})
    if (cs->ready && cs->Ac) {
      PL_HIP(hipMemsetAsync(cs->Ac, 0, (size_t)cs->ncp * cs->ncp * sizeof(double), h->stream));
      cs->ac_clean = true;
    }
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->ms_assembly = ms;
  h->assembled = true;
  h->have_bsr = refresh_bsr;
  return PL_OK;
}

int pl_assemble_bsr(pl_handle h, int with_bc, int64_t *n_block_rows, int64_t *n_blocks) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_assemble_bsr: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_assemble_bsr: not available on a DDM handle");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_assemble_bsr: call pl_assemble first");
  if (with_bc && !h->have_bc) return fail(PL_ERR_STATE, "pl_assemble_bsr: with_bc needs pl_set_bc");
  PL_HIP(hipSetDevice(h->opt.device));
  if (int rcb = ensure_bsr_buffers(h)) return rcb;
  const bool fresh = h->have_bsr && h->want_bsr && h->bsr_with_bc == (with_bc ? 1 : 0);
  h->want_bsr = true;
  h->bsr_with_bc = with_bc ? 1 : 0;
  if (fresh) {   // pl_assemble already rebuilt it (overlapped with the coarse factorisation)
    if (n_block_rows) *n_block_rows = h->N;
    if (n_blocks) *n_blocks = h->nblk;
    return PL_OK;
  }
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  int rc = launch_bsr_fill(h, with_bc, h->stream);
  if (rc) return rc;
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->ms_assembly += ms;
  h->have_bsr = true;
  if (n_block_rows) *n_block_rows = h->N;
  if (n_blocks) *n_blocks = h->nblk;
  return PL_OK;
}

int pl_get_bsr(pl_handle h, int64_t *rowptr, int32_t *colidx, double *vals) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_get_bsr: null handle");
  if (!h->have_bsr) return fail(PL_ERR_STATE, "pl_get_bsr: call pl_assemble_bsr first");
  PL_HIP(hipSetDevice(h->opt.device));
  // returned in CALLER numbering: row i of the device matrix is caller node perm[i]
  std::vector<double> v((size_t)h->nblk * 36);
  PL_HIP(hipMemcpy(v.data(), h->bsr_vals.p, v.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (!h->reordered) {
    if (rowptr) std::memcpy(rowptr, h->h_rowptr.data(), (h->N + 1) * sizeof(int64_t));
    if (colidx) std::memcpy(colidx, h->h_col.data(), h->nblk * sizeof(int32_t));
    if (vals) std::memcpy(vals, v.data(), v.size() * sizeof(double));
    return PL_OK;
  }
  // permuted: rebuild rows in caller order, columns re-sorted
  std::vector<int64_t> rp(h->N + 1, 0);
  for (int64_t ci = 0; ci < h->N; ++ci) {
    const int64_t di = h->iperm[ci];
    rp[ci + 1] = rp[ci] + (h->h_rowptr[di + 1] - h->h_rowptr[di]);
  }
  if (rowptr) std::memcpy(rowptr, rp.data(), (h->N + 1) * sizeof(int64_t));
  std::vector<std::pair<int32_t, int64_t>> row;
  for (int64_t ci = 0; ci < h->N; ++ci) {
    const int64_t di = h->iperm[ci];
    row.clear();
    for (int64_t p = h->h_rowptr[di]; p < h->h_rowptr[di + 1]; ++p) row.push_back({h->perm[h->h_col[p]], p});
    std::stable_sort(row.begin(), row.end(), [](auto &l, auto &r) { return l.first < r.first; });
    for (size_t k = 0; k < row.size(); ++k) {
      if (colidx) colidx[rp[ci] + k] = row[k].first;
      if (vals) std::memcpy(vals + 36 * (rp[ci] + k), &v[36 * row[k].second], 36 * sizeof(double));
    }
  }
  return PL_OK;
}

static int spmv_common(pl_handle h, const double *x, double *y, bool masked, const char *who) {
  if (!valid(h) || !x || !y) return fail(PL_ERR_ARG, std::string(who) + ": null argument");
  if (!h->assembled) return fail(PL_ERR_STATE, std::string(who) + ": call pl_assemble first");
  if (masked && !h->have_bc) return fail(PL_ERR_STATE, std::string(who) + ": call pl_set_bc first");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<double> stage;
  int rc = upload6(h, x, h->tmp.p, stage);
  if (rc) return rc;
  if (masked) {
    // enforce the contract "x is zero on fixed dofs" for arbitrary caller input
    hipLaunchKernelGGL(pl::k_mask_dot, dim3(grid_stream(h->N * 6)), dim3(pl::kBlock), 0, h->stream, h->N * 6,
                       h->fixed.p, h->tmp.p, h->tmp.p, (double *)nullptr);
  }
  rc = launch_spmv(h, h->tmp.p, h->tmp2.p, masked, nullptr);
  if (rc) return rc;
  return download6(h, h->tmp2.p, y);
}

int pl_spmv(pl_handle h, const double *x, double *y) { return spmv_common(h, x, y, false, "pl_spmv"); }
int pl_spmv_free(pl_handle h, const double *x, double *y) { return spmv_common(h, x, y, true, "pl_spmv_free"); }

int pl_spmv_bsr(pl_handle h, const double *x, double *y) {
  if (!valid(h) || !x || !y) return fail(PL_ERR_ARG, "pl_spmv_bsr: null argument");
  if (!h->have_bsr) return fail(PL_ERR_STATE, "pl_spmv_bsr: call pl_assemble_bsr first");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<double> stage;
  int rc = upload6(h, x, h->tmp.p, stage);
  if (rc) return rc;
  hipLaunchKernelGGL(pl::k_bsr_spmv, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N, h->bsr_rowptr.p,
                     h->bsr_col.p, h->bsr_vals.p, h->tmp.p, h->tmp2.p);
  PL_HIP(hipGetLastError());
  return download6(h, h->tmp2.p, y);
}

int pl_solve(pl_handle h, double rtol, int32_t max_iter, double *u, pl_stats_t *stats) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_solve: null handle");   // u == NULL: leave the solution on the device
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_solve: call pl_assemble first");
  if (!h->have_bc) return fail(PL_ERR_STATE, "pl_solve: call pl_set_bc first");
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, "pl_solve: rtol and max_iter must be positive");
  if (stats && stats->struct_size != sizeof(pl_stats_t))
    return fail(PL_ERR_ARG, "pl_solve: stats->struct_size is " + std::to_string(stats->struct_size) + ", this library's pl_stats_t has " +
                                std::to_string(sizeof(pl_stats_t)) + " bytes (set it to sizeof(pl_stats_t) before the call)");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t n6 = h->N * 6;
  pl_stats_t st{};
  st.struct_size = (uint32_t)sizeof(pl_stats_t);
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  // lifting: tmp = K ubar (ubar is zero on free dofs)
  int rc = launch_spmv(h, h->ubar.p, h->tmp.p, false, nullptr);
  if (rc) return rc;
  if (h->n_per_groups > 0 && (h->coarse.ready || ref_cg(h) || h->dist.active))
    return fail(PL_ERR_STATE, "pl_solve: periodic constraints (pl_set_periodic) need the plain Jacobi PCG");
  // fp32 solver modes need the multi-level preconditioner on the tile kernel; anything else runs the fp64 PCG
  const bool mp = mp_applies(h);
  solver_plan(h);
  const bool cg1 = !mp && cg1_applies(h);
  st.cg_form_used = cg1 ? 1.0 : 0.0;
  if (cg1) rc = pcg_solve_cg1(h, h->f.p, h->tmp.p, rtol, max_iter, &st);
  else if (mp && h->opt.precision == 1) rc = pcg_solve_mp_t<float>(h, h->f.p, h->tmp.p, rtol, max_iter, &st);
  else if (mp) rc = pcg_solve_mp_t<double>(h, h->f.p, h->tmp.p, rtol, max_iter, &st);
  else rc = pcg_solve(h, h->f.p, h->tmp.p, rtol, max_iter, &st);
  if (rc) return rc;
  st.precision_used = mp ? (double)h->opt.precision : 0.0;
  st.kp_form = (double)kp_form_of(h);
  st.comm_world = h->dist.active ? (double)h->dist.comm_count : 0.0;
  st.comm_rank = h->dist.active ? (double)h->dist.comm_user_rank : 0.0;
  st.condensed_nodes = h->cond_use ? (double)h->n_cond : 0.0;
  if (st.converged) st.info = 0.0;
  else if (st.info != 2.0) st.info = 1.0;     // precision mode the solve ran in
  if (!h->usol.p) PL_HIP(h->usol.alloc((size_t)n6));
  h->usol_valid = false;
  hipLaunchKernelGGL(pl::k_compose_solution, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, h->stream, n6, h->fixed.p,
                     h->ubar.p, h->x.p, h->usol.p);
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  st.ms_solve = ms;
  st.ms_assembly = h->ms_assembly;
  st.precond_used = h->opkind == 1 ? (h->dd_ready ? 2 : h->dd2_ready ? 4 : h->dd_blocks ? 3 : h->opt.precond >= 1 ? 1 : 0)
                                   : (h->coarse.ready ? h->opt.precond : (h->dd_ready ? 5 : 1));
  h->usol_valid = true;
  if (u) {
    rc = download6(h, h->usol.p, u);
    if (rc) return rc;
  }
  h->last = st;
  if (stats) *stats = st;
  if (!st.converged) return fail(PL_ERR_NOCONV, "pl_solve: PCG did not reach rtol within max_iter");
  return PL_OK;
}

int pl_reactions(pl_handle h, const double *u, double *R) { return spmv_common(h, u, R, false, "pl_reactions"); }

int pl_sens(pl_handle h, const double *u, const double *lam, double *dCdr) {
  if (!valid(h) || !dCdr) return fail(PL_ERR_ARG, "pl_sens: null argument");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_sens: not available on a DDM handle");
  const double *u_dev = nullptr;
  if (int rc = state_on_device(h, "pl_sens", u, &u_dev)) return rc;
  const double *lam_dev = u_dev;
  if (lam) {
    std::vector<double> stage;
    if (int rc = upload6(h, lam, h->tmp2.p, stage)) return rc;
    lam_dev = h->tmp2.p;
  }
  if (!h->sens_out.p) PL_HIP(h->sens_out.alloc(h->B));
  hipLaunchKernelGGL(pl::k_sens, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, h->xyz.p, h->conn.p,
                     h->radius.p, h->seg_len.p, h->seg_nsub.p, h->mult.p, h->mat, u_dev, lam_dev, h->sens_out.p);
  PL_HIP(hipGetLastError());
  return download_struts(h, h->sens_out.p, dCdr);
}

int pl_sens_gram(pl_handle h, int32_t n_rhs, const double *x, double *gram) {
  if (!valid(h) || !x || !gram) return fail(PL_ERR_ARG, "pl_sens_gram: null argument");
  if (n_rhs < 1 || n_rhs > PL_SENS_GRAM_MAX) return fail(PL_ERR_ARG, "pl_sens_gram: n_rhs must be 1 ... PL_SENS_GRAM_MAX");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_sens_gram: not available on a DDM handle");
  if (h->dist.active) return fail(PL_ERR_STATE, "pl_sens_gram: not available on a multi-GPU handle");
  PL_HIP(hipSetDevice(h->opt.device));
  const size_t n6 = (size_t)h->N * 6, B = (size_t)h->B, pairs = (size_t)n_rhs * (n_rhs + 1) / 2;
  if (h->gram_x.n < n_rhs * n6) PL_HIP(h->gram_x.alloc(n_rhs * n6));
  if (h->gram_out.n < pairs * B) PL_HIP(h->gram_out.alloc(pairs * B));
  if (h->pinG_n < pairs * B) {
    if (h->pinG) (void)hipHostFree(h->pinG);
    h->pinG = nullptr;
    h->pinG_n = 0;
    void *p = nullptr;
    PL_HIP(hipHostMalloc(&p, pairs * B * sizeof(double), hipHostMallocDefault));
    h->pinG = static_cast<double *>(p);
    h->pinG_n = pairs * B;
  }
  h->gram_cols = 0;
  std::vector<double> stage;
  int rc = PL_OK;
  for (int32_t k = 0; k < n_rhs; ++k) {
    rc = upload6(h, x + k * n6, h->gram_x.p + k * n6, stage);
    if (rc) return rc;
  }
  rc = launch_sens_gram(h, n_rhs, h->gram_x.p, h->gram_out.p);
  if (rc) return rc;
  h->gram_cols = n_rhs;
  PL_HIP(hipMemcpyAsync(h->pinG, h->gram_out.p, pairs * B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  for (size_t p = 0; p < pairs; ++p) struts_to_caller(h, h->pinG + p * B, gram + p * B);   // rows [pairs][B], one transfer
  return PL_OK;
}

int pl_node_mod(pl_handle h, const double *u, double *out) {
  if (!valid(h) || !u || !out) return fail(PL_ERR_ARG, "pl_node_mod: null argument");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_node_mod: not available on a DDM handle");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_node_mod: call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<double> stage;
  int rc = upload6(h, u, h->tmp.p, stage);
  if (rc) return rc;
  DevBuf<double> dev;
  PL_HIP(dev.alloc((size_t)h->B * 12));
  hipLaunchKernelGGL(pl::k_node_mod, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, h->xyz.p, h->conn.p,
                     h->radius.p, h->seg_len.p, h->seg_nsub.p, h->mult.p, h->mat, h->rec.p, h->tmp.p, dev.p);
  PL_HIP(hipGetLastError());
  return download_struts(h, dev.p, out, 12);
}

namespace {
// what pl_stress and pl_stress_pnorm share: the checks, and u on the device (tmp, or the last solution)
int stress_begin(pl_handle h, const char *who, const double *u, int32_t where, const double **u_dev) {
  if (!valid(h)) return fail(PL_ERR_ARG, std::string(who) + ": null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, std::string(who) + ": not available on a DDM handle");
  if (h->dist.active) return fail(PL_ERR_STATE, std::string(who) + ": not available on a multi-GPU handle");
  if (!h->assembled) return fail(PL_ERR_STATE, std::string(who) + ": call pl_assemble first");
  if (where != 0 && where != 1) return fail(PL_ERR_ARG, std::string(who) + ": where must be 0 (all stations) or 1 (middle segment)");
  return state_on_device(h, who, u, u_dev);
}
// PL_TIMING in the environment: HIP-event times of a call's device stages on stderr, "[<who>] <stage> <ms> ms" with four
// decimals (tools/time_*.py read this format).  mark(stage) records an event on the stream; a stage runs from its mark to the
// next one, so the last mark only closes the stage before it.  report() waits for the last mark and prints every stage.
struct EventTimer {
  static constexpr int kMaxMarks = 8;
  const char *who;
  hipStream_t stream;
  bool on;
  hipEvent_t ev[kMaxMarks] = {};
  const char *stage[kMaxMarks] = {};
  int n = 0;
  // first != null: the timer starts with mark(first)
  EventTimer(const char *w, hipStream_t s, const char *first = nullptr) : who(w), stream(s), on(std::getenv("PL_TIMING") != nullptr) {
    if (first) mark(first);
  }
  EventTimer(const EventTimer &) = delete;
  void mark(const char *name = nullptr) {
    if (!on || n == kMaxMarks || hipEventCreate(&ev[n]) != hipSuccess) return;
    stage[n] = name;
    (void)hipEventRecord(ev[n++], stream);
  }
  void report() {
    if (n < 2 || hipEventSynchronize(ev[n - 1]) != hipSuccess) return;
    for (int i = 0; i + 1 < n; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) timing_ms(who, stage[i], (double)ms);
    }
  }
  void stop() {   // closes the running stage and prints
    mark();
    report();
  }
  double lap() {  // closes the running stage and returns its time, for a caller that adds laps up and prints the sum itself
    mark();
    float ms = 0.f;
    if (n >= 2 && hipEventSynchronize(ev[n - 1]) == hipSuccess) (void)hipEventElapsedTime(&ms, ev[n - 2], ev[n - 1]);
    return ms;
  }
  ~EventTimer() {
    for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
  }
};

// Thermal state of the handle (pl_set_thermal): *t = null without one.  With one, delta[B] (and n_free[B] when asked for) is
// rebuilt from the current records - k_thermal_strut, one thread per strut - so the state follows every pl_assemble.
int thermal_refresh(pl_handle h, const char *who, bool want_n_free, ThermalWs **t) {
  *t = static_cast<ThermalWs *>(h->thermal_ws.get());
  if (!*t) return PL_OK;
  EventTimer timer(who, h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_thermal_strut, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, h->conn.p, h->rec.p,
                     h->mult.p, (*t)->alpha.p, (*t)->dT.p, (*t)->delta.p, want_n_free ? (*t)->n_free.p : (double *)nullptr);
  PL_HIP(hipGetLastError());
  timer.stop();
  return PL_OK;
}
// the free elongations the stress and buckling passes subtract: *delta = null without a thermal state (the plain kernels run)
int thermal_delta(pl_handle h, const char *who, const double **delta) {
  ThermalWs *t = nullptr;
  if (int rc = thermal_refresh(h, who, false, &t)) return rc;
  *delta = t ? t->delta.p : nullptr;
  return PL_OK;
}
// runs launch(std::bool_constant<TH>): the thermal instantiation of a strut kernel exactly when delta is set
extern "C++" {   // (a template)
template <class Launch>
void thermal_dispatch(const double *delta, Launch launch) {
  if (delta) launch(std::true_type{});
  else launch(std::false_type{});
}
}  // extern "C++"
}  // namespace

int pl_stress(pl_handle h, const double *u, int32_t where, double *station, double *peak) {
  const double *u_dev = nullptr;
  if (int rc = stress_begin(h, "pl_stress", u, where, &u_dev)) return rc;
  if (!station && !peak) return fail(PL_ERR_ARG, "pl_stress: every output pointer is NULL");
  const int64_t B = h->B;
  DevBuf<double> d_station;
  if (station) PL_HIP(d_station.alloc((size_t)B * 20));
  if (peak && !h->st_dr.p) PL_HIP(h->st_dr.alloc((size_t)B));
  const double *delta = nullptr;
  if (int rc = thermal_delta(h, "pl_stress", &delta)) return rc;
  EventTimer timer("pl_stress", h->stream, "kernel_hip_event");
  thermal_dispatch(delta, [&](auto th) {
    hipLaunchKernelGGL(pl::k_stress_stations<decltype(th)::value>, dim3(grid_for(B)), dim3(pl::kBlock), 0, h->stream, B,
                       h->conn.p, h->rec.p, h->radius.p, h->seg_len.p, h->mult.p, h->mat.pen, (int)where, u_dev, d_station.p,
                       peak ? h->st_dr.p : (double *)nullptr, (double *)nullptr, (double *)nullptr, delta);
  });
  PL_HIP(hipGetLastError());
  timer.stop();
  if (station)
    if (int rc = download_struts(h, d_station.p, station, 20)) return rc;
  if (peak)
    if (int rc = download_struts(h, h->st_dr.p, peak)) return rc;
  return PL_OK;
}

extern "C++" {   // (a template)
namespace {
// What pl_stress_pnorm and pl_buckling_pnorm share after their own checks: the checks of p and the outputs, the work arrays
// (st_vm4 = the measure's per-strut values, one stream, every call ends with its downloads), the passes
//     values -> fold<max> -> p-sum -> fold<sum> [-> grad<DR> [-> k_stress_gather]]
// between the marks of the PL_TIMING line, red = (max, p-sum, p-norm) and the downloads.  The measure gives its three
// launches: values(grid) fills st_vm4 and the block maxima in st_part, psum(grid) the block sums in st_part, and
// grad(grid, std::bool_constant<DR>) G[b][6] in st_G and, with DR, d/dr in st_dr.  A new per-strut aggregate is one such triple.
template <class Values, class Psum, class Grad>
int pnorm_call(pl_handle h, const char *who, double p, double *value, double *value_max, double *d_du, double *d_dr,
               Values values, Psum psum, Grad grad) {
  if (!(p >= 1.0) || !std::isfinite(p)) return fail(PL_ERR_ARG, std::string(who) + ": p must be >= 1");
  if (!value && !value_max && !d_du && !d_dr) return fail(PL_ERR_ARG, std::string(who) + ": every output pointer is NULL");
  const int64_t B = h->B, N = h->N;
  const unsigned grid = grid_for(B);
  if (!h->st_vm4.p) PL_HIP(h->st_vm4.alloc((size_t)B * 4));
  if (!h->st_part.p) PL_HIP(h->st_part.alloc(std::max<size_t>(grid, 1)));
  if (!h->st_red.p) PL_HIP(h->st_red.alloc(4));
  if ((d_du || d_dr) && !h->st_G.p) PL_HIP(h->st_G.alloc((size_t)B * 6));
  if (d_dr && !h->st_dr.p) PL_HIP(h->st_dr.alloc((size_t)B));
  EventTimer timer(who, h->stream, "kernel_hip_event");
  values(grid);
  hipLaunchKernelGGL(pl::k_stress_fold<true>, dim3(1), dim3(pl::kBlock), 0, h->stream, (int64_t)grid, h->st_part.p, p,
                     h->st_red.p);
  psum(grid);
  hipLaunchKernelGGL(pl::k_stress_fold<false>, dim3(1), dim3(pl::kBlock), 0, h->stream, (int64_t)grid, h->st_part.p, p,
                     h->st_red.p);
  if (d_dr) grad(grid, std::true_type{});
  else if (d_du) grad(grid, std::false_type{});
  if (d_du)   // (tmp2 is free: u sits in tmp or usol)
    hipLaunchKernelGGL(pl::k_stress_gather, dim3(grid_for(N)), dim3(pl::kBlock), 0, h->stream, N, pl::kWave / h->lpn,
                       h->slice_ptr.p, h->ent.p, h->rec.p, h->st_G.p, h->tmp2.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  double red[3] = {0, 0, 0};
  PL_HIP(hipMemcpyAsync(red, h->st_red.p, sizeof(red), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  if (value_max) *value_max = red[0];
  if (value) *value = red[2];
  if (d_du)
    if (int rc = download6(h, h->tmp2.p, d_du)) return rc;
  if (d_dr)
    if (int rc = download_struts(h, h->st_dr.p, d_dr)) return rc;
  return PL_OK;
}
}  // namespace
}  // extern "C++"

int pl_stress_pnorm(pl_handle h, const double *u, int32_t where, double p, double *phi, double *sigma_max, double *dphi_du,
                    double *dphi_dr) {
  const double *u_dev = nullptr;
  if (int rc = stress_begin(h, "pl_stress_pnorm", u, where, &u_dev)) return rc;
  const int64_t B = h->B;
  const double *delta = nullptr;
  if (int rc = thermal_delta(h, "pl_stress_pnorm", &delta)) return rc;
  return pnorm_call(h, "pl_stress_pnorm", p, phi, sigma_max, dphi_du, dphi_dr, [&](unsigned grid) {
    thermal_dispatch(delta, [&](auto th) {
      hipLaunchKernelGGL(pl::k_stress_stations<decltype(th)::value>, dim3(grid), dim3(pl::kBlock), 0, h->stream, B, h->conn.p,
                         h->rec.p, h->radius.p, h->seg_len.p, h->mult.p, h->mat.pen, (int)where, u_dev, (double *)nullptr,
                         (double *)nullptr, h->st_vm4.p, h->st_part.p, delta);
    });
  }, [&](unsigned grid) {
    hipLaunchKernelGGL((pl::k_pnorm_psum<4, true>), dim3(grid), dim3(pl::kBlock), 0, h->stream, B, h->st_vm4.p, h->st_red.p, p,
                       h->st_part.p);
  }, [&](unsigned grid, auto dr) {
    thermal_dispatch(delta, [&](auto th) {
      hipLaunchKernelGGL((pl::k_stress_grad<decltype(dr)::value, decltype(th)::value>), dim3(grid), dim3(pl::kBlock), 0,
                         h->stream, B, h->conn.p, h->rec.p, h->radius.p, h->seg_len.p, h->seg_nsub.p, h->mult.p, h->mat,
                         (int)where, p, u_dev, h->st_red.p, h->st_G.p, dr ? h->st_dr.p : (double *)nullptr, delta);
    });
  });
}

namespace {
// what pl_buckling and pl_buckling_pnorm share: the argument checks, then those of the stress pass and u on the device
int buckling_begin(pl_handle h, const char *who, const double *u, int32_t length, double k_eff, int32_t shear,
                   const double **u_dev) {
  if (!valid(h)) return fail(PL_ERR_ARG, std::string(who) + ": null handle");
  if (length != 0 && length != 1)
    return fail(PL_ERR_ARG, std::string(who) + ": length must be 0 (node to node) or 1 (middle segment)");
  if (shear != 0 && shear != 1) return fail(PL_ERR_ARG, std::string(who) + ": shear must be 0 (Euler) or 1 (Engesser)");
  if (!(k_eff > 0.0) || !std::isfinite(k_eff)) return fail(PL_ERR_ARG, std::string(who) + ": k_eff must be positive and finite");
  return stress_begin(h, who, u, 0, u_dev);
}
}  // namespace

int pl_buckling(pl_handle h, const double *u, int32_t length, double k_eff, int32_t shear, double *util, double *n_axial,
                double *n_crit) {
  const double *u_dev = nullptr;
  if (int rc = buckling_begin(h, "pl_buckling", u, length, k_eff, shear, &u_dev)) return rc;
  if (!util && !n_axial && !n_crit) return fail(PL_ERR_ARG, "pl_buckling: every output pointer is NULL");
  const int64_t B = h->B;
  if (!h->st_vm4.p) PL_HIP(h->st_vm4.alloc((size_t)B * 4));   // rows 0..2 of [4][B]: beta, N, N_cr
  double *d_util = h->st_vm4.p, *d_n = h->st_vm4.p + B, *d_cr = h->st_vm4.p + 2 * B;
  const double *delta = nullptr;
  if (int rc = thermal_delta(h, "pl_buckling", &delta)) return rc;
  EventTimer timer("pl_buckling", h->stream, "kernel_hip_event");
  thermal_dispatch(delta, [&](auto th) {
    hipLaunchKernelGGL(pl::k_buckling_util<decltype(th)::value>, dim3(grid_for(B)), dim3(pl::kBlock), 0, h->stream, B,
                       h->conn.p, h->rec.p, h->radius.p, h->seg_len.p, h->mult.p, h->mat, (int)length, k_eff, (int)shear, u_dev,
                       util ? d_util : (double *)nullptr, n_axial ? d_n : (double *)nullptr,
                       n_crit ? d_cr : (double *)nullptr, (double *)nullptr, delta);
  });
  PL_HIP(hipGetLastError());
  timer.stop();
  if (util)
    if (int rc = download_struts(h, d_util, util)) return rc;
  if (n_axial)
    if (int rc = download_struts(h, d_n, n_axial)) return rc;
  if (n_crit)
    if (int rc = download_struts(h, d_cr, n_crit)) return rc;
  return PL_OK;
}

int pl_buckling_pnorm(pl_handle h, const double *u, int32_t length, double k_eff, int32_t shear, double p, double *bp,
                      double *util_max, double *dbp_du, double *dbp_dr) {
  const double *u_dev = nullptr;
  if (int rc = buckling_begin(h, "pl_buckling_pnorm", u, length, k_eff, shear, &u_dev)) return rc;
  const int64_t B = h->B;
  const double *delta = nullptr;
  if (int rc = thermal_delta(h, "pl_buckling_pnorm", &delta)) return rc;
  return pnorm_call(h, "pl_buckling_pnorm", p, bp, util_max, dbp_du, dbp_dr, [&](unsigned grid) {   // beta in st_vm4
    thermal_dispatch(delta, [&](auto th) {
      hipLaunchKernelGGL(pl::k_buckling_util<decltype(th)::value>, dim3(grid), dim3(pl::kBlock), 0, h->stream, B, h->conn.p,
                         h->rec.p, h->radius.p, h->seg_len.p, h->mult.p, h->mat, (int)length, k_eff, (int)shear, u_dev,
                         h->st_vm4.p, (double *)nullptr, (double *)nullptr, h->st_part.p, delta);
    });
  }, [&](unsigned grid) {
    hipLaunchKernelGGL((pl::k_pnorm_psum<1, false>), dim3(grid), dim3(pl::kBlock), 0, h->stream, B, h->st_vm4.p, h->st_red.p, p,
                       h->st_part.p);
  }, [&](unsigned grid, auto dr) {
    thermal_dispatch(delta, [&](auto th) {
      hipLaunchKernelGGL((pl::k_buckling_grad<decltype(dr)::value, decltype(th)::value>), dim3(grid), dim3(pl::kBlock), 0,
                         h->stream, B, h->conn.p, h->rec.p, h->radius.p, h->seg_len.p, h->seg_nsub.p, h->mult.p, h->mat,
                         (int)length, k_eff, (int)shear, p, u_dev, h->st_red.p, h->st_G.p, dr ? h->st_dr.p : (double *)nullptr,
                         delta);
    });
  });
}

// ---- thermal loads (pl_thermal.h) ----------------------------------------------------------------------------------------
int pl_set_thermal(pl_handle h, double alpha, const double *beam_alpha, const double *node_dT) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_thermal: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_thermal: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_set_thermal: single-GPU handles only (this one belongs to a multi-rank run)");
  if (!node_dT) {
    h->thermal_ws.reset();
    return PL_OK;
  }
  if (!beam_alpha && !std::isfinite(alpha)) return fail(PL_ERR_ARG, "pl_set_thermal: alpha must be finite");
  if (beam_alpha)
    for (int64_t b = 0; b < h->B; ++b)
      if (!std::isfinite(beam_alpha[b])) return fail(PL_ERR_ARG, "pl_set_thermal: beam_alpha must be finite");
  for (int64_t i = 0; i < h->N; ++i)
    if (!std::isfinite(node_dT[i])) return fail(PL_ERR_ARG, "pl_set_thermal: node_dT must be finite");
  PL_HIP(hipSetDevice(h->opt.device));
  const size_t B = (size_t)h->B, N = (size_t)h->N;
  auto t = std::make_shared<ThermalWs>();
  PL_HIP(t->alpha.alloc(B));
  PL_HIP(t->dT.alloc(N));
  PL_HIP(t->delta.alloc(B));
  PL_HIP(t->n_free.alloc(B));
  PL_HIP(t->out.alloc(B));
  std::vector<double> al(B), dt(N);
  for (size_t b = 0; b < B; ++b) al[b] = beam_alpha ? beam_alpha[h->bperm[b]] : alpha;
  for (size_t i = 0; i < N; ++i) dt[i] = node_dT[h->perm[i]];
  PL_HIP(hipMemcpy(t->alpha.p, al.data(), B * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(t->dT.p, dt.data(), N * sizeof(double), hipMemcpyHostToDevice));
  h->thermal_ws = t;
  return PL_OK;
}

namespace {
// what pl_thermal_load and pl_thermal_sens share: the handle checks and the refreshed elongations
int thermal_begin(pl_handle h, const char *who, bool want_n_free, ThermalWs **t) {
  if (!valid(h)) return fail(PL_ERR_ARG, std::string(who) + ": null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, std::string(who) + ": not available on a DDM handle");
  if (h->dist.active) return fail(PL_ERR_STATE, std::string(who) + ": not available on a multi-GPU handle");
  if (!h->thermal_ws) return fail(PL_ERR_STATE, std::string(who) + ": call pl_set_thermal first");
  if (!h->assembled) return fail(PL_ERR_STATE, std::string(who) + ": call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  return thermal_refresh(h, who, want_n_free, t);
}
}  // namespace

int pl_thermal_load(pl_handle h, double *f, double *n_free) {
  if (valid(h) && !f && !n_free) return fail(PL_ERR_ARG, "pl_thermal_load: every output pointer is NULL");
  ThermalWs *t = nullptr;
  if (int rc = thermal_begin(h, "pl_thermal_load", n_free != nullptr, &t)) return rc;
  if (f) {   // (tmp2 is a work vector of the derived-quantity calls: pnorm_call gathers into it too)
    EventTimer timer("pl_thermal_load", h->stream, "kernel_hip_event");
    hipLaunchKernelGGL(pl::k_thermal_load, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N, pl::kWave / h->lpn,
                       h->slice_ptr.p, h->ent.p, h->rec.p, t->delta.p, h->tmp2.p);
    PL_HIP(hipGetLastError());
    timer.stop();
    if (int rc = download6(h, h->tmp2.p, f)) return rc;
  }
  if (n_free)
    if (int rc = download_struts(h, t->n_free.p, n_free)) return rc;
  return PL_OK;
}

int pl_thermal_sens(pl_handle h, const double *lam, double *out) {
  if (valid(h) && !out) return fail(PL_ERR_ARG, "pl_thermal_sens: null argument");
  ThermalWs *t = nullptr;
  if (int rc = thermal_begin(h, "pl_thermal_sens", false, &t)) return rc;
  const double *lam_dev = nullptr;
  if (int rc = state_on_device(h, "pl_thermal_sens", lam, &lam_dev)) return rc;
  EventTimer timer("pl_thermal_sens", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_thermal_sens, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, h->conn.p, h->rec.p,
                     h->radius.p, t->delta.p, lam_dev, t->out.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  return download_struts(h, t->out.p, out);
}

int pl_energy(pl_handle h, const double *u, double *energy) {
  if (!valid(h) || !u || !energy) return fail(PL_ERR_ARG, "pl_energy: null argument");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_energy: not available on a DDM handle");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_energy: call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<double> stage;
  int rc = upload6(h, u, h->tmp.p, stage);
  if (rc) return rc;
  double *aux = h->scal.p + pl::S_AUX * pl::kSlots;
  double h_aux[pl::kSlots];
  PL_HIP(hipMemsetAsync(aux, 0, sizeof(h_aux), h->stream));
  hipLaunchKernelGGL(pl::k_energy, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, h->conn.p, h->rec.p,
                     h->tmp.p, aux);
  PL_HIP(hipGetLastError());
  PL_HIP(hipMemcpyAsync(h_aux, aux, sizeof(h_aux), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  *energy = 0.0;
  for (int k = 0; k < pl::kSlots; ++k) *energy += h_aux[k];
  return PL_OK;
}

int pl_schur(pl_handle h, const int32_t *boundary_nodes, int32_t nb, double rtol, int32_t max_iter, double *S) {
  if (!valid(h) || !boundary_nodes || !S || nb <= 0) return fail(PL_ERR_ARG, "pl_schur: bad argument");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_schur: call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  const size_t n6 = (size_t)N * 6;
  for (int i = 0; i < nb; ++i)
    if (boundary_nodes[i] < 0 || boundary_nodes[i] >= N) return fail(PL_ERR_ARG, "pl_schur: node index out of range");
  // Column j of S = reaction on the boundary dofs when boundary dof j = 1, the other boundary dofs = 0 and the
  // interior is in equilibrium: exactly S = K_BB - K_BI K_II^-1 K_IB.
  std::vector<uint8_t> fixed(n6, 0);
  for (int i = 0; i < nb; ++i)
    for (int k = 0; k < 6; ++k) fixed[6 * (size_t)boundary_nodes[i] + k] = 1;
  std::vector<double> ubar(n6, 0.0), u(n6), R(n6);
  const int m = nb * 6;
  for (int j = 0; j < m; ++j) {
    const size_t dofj = 6 * (size_t)boundary_nodes[j / 6] + (j % 6);
    ubar[dofj] = 1.0;
    int rc = pl_set_bc(h, fixed.data(), ubar.data(), nullptr);
    if (rc) return rc;
    pl_stats_t st;
    st.struct_size = (uint32_t)sizeof(pl_stats_t);
    rc = pl_solve(h, rtol, max_iter, u.data(), &st);
    if (rc) return rc;
    rc = pl_reactions(h, u.data(), R.data());
    if (rc) return rc;
    for (int i = 0; i < m; ++i) S[(size_t)i * m + j] = R[6 * (size_t)boundary_nodes[i / 6] + (i % 6)];
    ubar[dofj] = 0.0;
  }
  return PL_OK;
}

// ---- several right-hand sides in one pass (pl_multi.h) ---------------------------------------------------------------
extern "C++" {   // (a template)
namespace {
// What the four pl_*_spmv_multi calls share: the checks of x, y and n_rhs, the workspace, the upload (masked: the free dofs
// only), one launch of k_gather_multi between the marks of the PL_TIMING line, and the download.  begin() makes the call's own
// checks and preparations (0 = go on); term() then gives the operator, shape(h, n_rhs) its column blocks.
template <class Begin, class TermOf>
int spmv_multi_call(pl_handle h, const char *who, MultiShape (*shape)(const pl_context *, int), int32_t n_rhs, int masked,
                    const double *x, double *y, Begin begin, TermOf term) {
  if (!valid(h) || !x || !y) return fail(PL_ERR_ARG, std::string(who) + ": null argument");
  if (n_rhs < 1 || n_rhs > PL_MULTI_MAX) return fail(PL_ERR_ARG, std::string(who) + ": n_rhs must be 1 ... PL_MULTI_MAX");
  if (int rc = begin()) return rc;
  const MultiShape s = shape(h, n_rhs);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s, false, &w)) return rc;
  if (int rc = multi_upload(h, w, s, x, w->F.p, masked ? -1 : 0)) return rc;
  EventTimer timer(who, h->stream, "kernel_hip_event");
  if (int rc = launch_gather_multi(h, s, term(), h->fixedbits.p, w->F.p, w->U.p, masked != 0, nullptr)) return rc;
  timer.stop();
  return multi_download(h, w, s, w->U.p, y);
}
}  // namespace
}  // extern "C++"

int pl_spmv_multi(pl_handle h, int32_t n_rhs, int masked, const double *x, double *y) {
  return spmv_multi_call(h, "pl_spmv_multi", multi_shape, n_rhs, masked, x, y, [&]() -> int {
    if (int rc = multi_check_handle(h, "pl_spmv_multi", masked != 0)) return rc;
    PL_HIP(hipSetDevice(h->opt.device));
    return PL_OK;
  }, [&] { return pl::StiffTerm{h->rec.p}; });
}

namespace {
// per-column statistics from the status block of pcg_solve_multi; returns the number of columns that missed rtol
int multi_stats(const MultiShape &s, const double *status, double rtol, double ms, pl_stats_t *stats, bool *bad_number) {
  int missed = 0;
  for (int j = 0; j < s.n_rhs; ++j) {
    const double rr = status[pl::M_ST_RR * s.ncol + j], bb = status[pl::M_ST_BB * s.ncol + j];
    const bool conv = rr <= rtol * rtol * bb;
    if (!std::isfinite(rr) || !std::isfinite(bb)) *bad_number = true;
    if (!conv) ++missed;
    if (stats) {
      pl_stats_t st{};
      st.struct_size = (uint32_t)sizeof(pl_stats_t);
      st.iterations = (int32_t)status[pl::M_ST_ITER * s.ncol + j];
      st.converged = conv ? 1 : 0;
      st.rel_residual = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
      st.b_norm = std::sqrt(bb);
      st.ms_solve = ms;
      st.precond_used = 1.0;
      st.kp_form = 5.0;
      st.info = conv ? 0.0 : 1.0;
      stats[j] = st;
    }
  }
  return missed;
}
}  // namespace

int pl_solve_multi(pl_handle h, int32_t n_rhs, const double *ubar, const double *f, double rtol, int32_t max_iter, double *u,
                   pl_stats_t *stats) {
  if (!valid(h) || !u) return fail(PL_ERR_ARG, "pl_solve_multi: null argument");
  if (n_rhs < 1 || n_rhs > PL_MULTI_MAX) return fail(PL_ERR_ARG, "pl_solve_multi: n_rhs must be 1 ... PL_MULTI_MAX");
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, "pl_solve_multi: rtol and max_iter must be positive");
  if (stats)
    for (int j = 0; j < n_rhs; ++j)
      if (stats[j].struct_size != sizeof(pl_stats_t))
        return fail(PL_ERR_ARG, "pl_solve_multi: stats[" + std::to_string(j) + "].struct_size is " + std::to_string(stats[j].struct_size) +
                                    ", this library's pl_stats_t has " + std::to_string(sizeof(pl_stats_t)) + " bytes");
  if (int rc = multi_check_handle(h, "pl_solve_multi", true)) return rc;
  PL_HIP(hipSetDevice(h->opt.device));
  const MultiShape s = multi_shape(h, n_rhs);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s, true, &w)) return rc;
  if (int rc = multi_upload(h, w, s, ubar, w->UB.p, 1)) return rc;
  if (f)
    if (int rc = multi_upload(h, w, s, f, w->F.p, 0)) return rc;
  std::vector<double> status((size_t)pl::M_ST_COUNT * s.ncol);
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  if (int rc = pcg_solve_multi(h, w, s, h->fixedbits.p, f ? (const double *)w->F.p : (const double *)nullptr, rtol, max_iter,
                               status.data()))
    return rc;
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (int rc = multi_download(h, w, s, w->U.p, u)) return rc;
  bool bad = false;
  const int missed = multi_stats(s, status.data(), rtol, ms, stats, &bad);
  if (bad) return fail(PL_ERR_NAN, "pl_solve_multi: NaN/Inf in a residual norm");
  if (missed) return fail(PL_ERR_NOCONV, "pl_solve_multi: " + std::to_string(missed) + " column(s) did not reach rtol within max_iter");
  return PL_OK;
}

int pl_schur_block(pl_handle h, const int32_t *boundary_nodes, int32_t nb, double rtol, int32_t max_iter, int32_t block,
                   double *S) {
  if (!valid(h) || !boundary_nodes || !S || nb <= 0) return fail(PL_ERR_ARG, "pl_schur_block: bad argument");
  if (block < 0 || block > PL_MULTI_MAX) return fail(PL_ERR_ARG, "pl_schur_block: block must be 0 ... PL_MULTI_MAX");
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, "pl_schur_block: rtol and max_iter must be positive");
  if (int rc = multi_check_handle(h, "pl_schur_block", false)) return rc;
  const int64_t N = h->N;
  for (int i = 0; i < nb; ++i)
    if (boundary_nodes[i] < 0 || boundary_nodes[i] >= N) return fail(PL_ERR_ARG, "pl_schur_block: node index out of range");
  PL_HIP(hipSetDevice(h->opt.device));
  const int m = nb * 6;
  if (block == 0) block = kSchurBlockDefault;
  block = std::min(block, m);
  // The boundary mask, the unit displacements and the Jacobi inverse live in the workspace: the handle's own boundary data
  // (pl_set_bc) are never touched, so there is nothing to restore.
  std::vector<int32_t> inv((size_t)N), bdev((size_t)nb);
  for (int64_t i = 0; i < N; ++i) inv[(size_t)h->perm[i]] = (int32_t)i;          // caller node -> device node
  std::vector<uint8_t> bits((size_t)N, 0);
  for (int i = 0; i < nb; ++i) {
    bdev[(size_t)i] = inv[(size_t)boundary_nodes[i]];
    bits[(size_t)bdev[(size_t)i]] = 0x3f;
  }
  const MultiShape s0 = multi_shape(h, block);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s0, true, &w)) return rc;
  if (w->fixedbits.n < (size_t)N) PL_HIP(w->fixedbits.alloc((size_t)N));
  if (w->bnodes.n < (size_t)nb) PL_HIP(w->bnodes.alloc((size_t)nb));
  if (w->S.n < (size_t)m * m) PL_HIP(w->S.alloc((size_t)m * m));
  PL_HIP(hipMemcpyAsync(w->fixedbits.p, bits.data(), (size_t)N, hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipMemcpyAsync(w->bnodes.p, bdev.data(), (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));      // (bits / bdev are pageable host memory)
  // Column j of S = reaction on the boundary dofs when boundary dof j = 1, the other boundary dofs = 0 and the interior is
  // in equilibrium (as pl_schur)
  std::vector<double> status((size_t)pl::M_ST_COUNT * PL_MULTI_MAX);
  int rc = PL_OK, missed = 0;
  bool bad = false;
  for (int j0 = 0; j0 < m && rc == PL_OK; j0 += block) {
    const int n = std::min(block, m - j0);
    const MultiShape s = multi_shape(h, n);
    const size_t bytes = (size_t)s.ncb * s.stride * sizeof(double);
    if (hipMemsetAsync(w->UB.p, 0, bytes, h->stream) != hipSuccess) { rc = fail(PL_ERR_HIP, "pl_schur_block: memset failed"); break; }
    hipLaunchKernelGGL(pl::k_multi_unit_ubar, dim3(grid_for(n)), dim3(pl::kBlock), 0, h->stream, n, j0, (const int32_t *)w->bnodes.p,
                       w->UB.p, s.KB, s.stride);
    rc = pcg_solve_multi(h, w, s, w->fixedbits.p, nullptr, rtol, max_iter, status.data());
    if (rc) break;
    missed += multi_stats(s, status.data(), rtol, 0.0, nullptr, &bad);
    rc = launch_spmv_multi(h, s, w->fixedbits.p, w->U.p, w->AP.p, false, nullptr);     // reactions R_j = K u_j
    if (rc) break;
    hipLaunchKernelGGL(pl::k_multi_schur_rows, dim3(grid_for((int64_t)m * n)), dim3(pl::kBlock), 0, h->stream, m, n, j0,
                       (const int32_t *)w->bnodes.p, (const double *)w->AP.p, w->S.p, s.KB, s.stride);
  }
  if (rc) return rc;
  PL_HIP(hipGetLastError());
  PL_HIP(hipMemcpyAsync(S, w->S.p, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  if (bad) return fail(PL_ERR_NAN, "pl_schur_block: NaN/Inf in a residual norm");
  if (missed) return fail(PL_ERR_NOCONV, "pl_schur_block: " + std::to_string(missed) + " column(s) did not reach rtol within max_iter");
  return PL_OK;
}

// ---- steady heat conduction on the strut graph (pl_conduction.h) ---------------------------------------------------------
int pl_set_conduction(pl_handle h, double kappa, const double *beam_kappa) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_conduction: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_conduction: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_set_conduction: single-GPU handles only (this one belongs to a multi-rank run)");
  if (kappa == 0.0 && !beam_kappa) {
    h->cond_ws.reset();
    return PL_OK;
  }
  if (!beam_kappa && !(kappa > 0.0 && std::isfinite(kappa)))
    return fail(PL_ERR_ARG, "pl_set_conduction: kappa must be positive and finite");
  if (beam_kappa)
    for (int64_t b = 0; b < h->B; ++b)
      if (!(beam_kappa[b] > 0.0 && std::isfinite(beam_kappa[b])))
        return fail(PL_ERR_ARG, "pl_set_conduction: beam_kappa must be positive and finite");
  PL_HIP(hipSetDevice(h->opt.device));
  const size_t B = (size_t)h->B, N = (size_t)h->N;
  auto w = std::make_shared<CondWs>();
  for (DevBuf<double> *b : {&w->kappa, &w->g, &w->out}) PL_HIP(b->alloc(B));
  for (DevBuf<double> *b : {&w->X, &w->R, &w->Z, &w->P, &w->AP, &w->KT, &w->TB, &w->QF, &w->T, &w->MU, &w->dinv})
    PL_HIP(b->alloc(N));
  PL_HIP(w->fixed.alloc(N));
  PL_HIP(w->scal.alloc(kCondScal));
  PL_HIP(w->flags.alloc(2));
  std::vector<double> ka(B);
  for (size_t b = 0; b < B; ++b) ka[b] = beam_kappa ? beam_kappa[h->bperm[b]] : kappa;
  PL_HIP(hipMemcpy(w->kappa.p, ka.data(), B * sizeof(double), hipMemcpyHostToDevice));
  h->cond_ws = w;
  return PL_OK;
}

namespace {
// what the conduction calls share: the handle checks and the conductances of the current radii and records - k_cond_strut, one
// thread per strut - so the state follows every pl_update_radii and pl_assemble without a flag
int cond_begin(pl_handle h, const char *who, CondWs **w) {
  if (!valid(h)) return fail(PL_ERR_ARG, std::string(who) + ": null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, std::string(who) + ": not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, std::string(who) + ": single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->cond_ws) return fail(PL_ERR_STATE, std::string(who) + ": call pl_set_conduction first");
  if (!h->assembled) return fail(PL_ERR_STATE, std::string(who) + ": call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  *w = static_cast<CondWs *>(h->cond_ws.get());
  EventTimer timer(who, h->stream, "kernel_hip_event");
  if ((*w)->conv) {   // the film conductances and their nodal sums follow the radii in the same pass
    hipLaunchKernelGGL(pl::k_cond_strut<true>, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B,
                       (const pl::Record *)h->rec.p, (const double *)h->radius.p, (const double *)h->mult.p,
                       (const double *)(*w)->kappa.p, (*w)->g.p, (const double *)(*w)->film.p, (*w)->c.p);
    hipLaunchKernelGGL(pl::k_cond_hdiag, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N, pl::kWave / h->lpn,
                       (const int64_t *)h->slice_ptr.p, (const int2 *)h->ent.p, (const double *)(*w)->c.p, (*w)->H.p);
  } else {
    hipLaunchKernelGGL(pl::k_cond_strut<false>, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B,
                       (const pl::Record *)h->rec.p, (const double *)h->radius.p, (const double *)h->mult.p,
                       (const double *)(*w)->kappa.p, (*w)->g.p, (const double *)nullptr, (double *)nullptr);
  }
  PL_HIP(hipGetLastError());
  timer.stop();
  return PL_OK;
}
}  // namespace

int pl_set_convection(pl_handle h, double film, const double *beam_film, double T_inf) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_convection: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_convection: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_set_convection: single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->cond_ws) return fail(PL_ERR_STATE, "pl_set_convection: call pl_set_conduction first");
  CondWs *w = static_cast<CondWs *>(h->cond_ws.get());
  if (film == 0.0 && !beam_film) {
    w->conv = false;
    return PL_OK;
  }
  if (!beam_film && !(film > 0.0 && std::isfinite(film)))
    return fail(PL_ERR_ARG, "pl_set_convection: film must be positive and finite");
  if (!std::isfinite(T_inf)) return fail(PL_ERR_ARG, "pl_set_convection: T_inf must be finite");
  if (beam_film) {
    bool any = false;
    for (int64_t b = 0; b < h->B; ++b) {
      if (!(beam_film[b] >= 0.0 && std::isfinite(beam_film[b])))
        return fail(PL_ERR_ARG, "pl_set_convection: beam_film must be non-negative and finite");
      any = any || beam_film[b] > 0.0;
    }
    if (!any) return fail(PL_ERR_ARG, "pl_set_convection: every film coefficient is zero");
  }
  PL_HIP(hipSetDevice(h->opt.device));
  const size_t B = (size_t)h->B, N = (size_t)h->N;
  if (!w->film.p) {
    PL_HIP(w->film.alloc(B));
    PL_HIP(w->c.alloc(B));
    PL_HIP(w->H.alloc(N));
    PL_HIP(w->part.alloc(std::max<size_t>(grid_for(h->B), 1)));
    PL_HIP(w->total.alloc(1));
  }
  std::vector<double> hf(B);
  for (size_t b = 0; b < B; ++b) hf[b] = beam_film ? beam_film[h->bperm[b]] : film;
  PL_HIP(hipMemcpy(w->film.p, hf.data(), B * sizeof(double), hipMemcpyHostToDevice));
  w->T_inf = T_inf;
  w->conv = true;
  return PL_OK;
}

int pl_cond_spmv(pl_handle h, int32_t masked, const uint8_t *fixed, const double *x, double *y) {
  if (valid(h) && (!x || !y || (masked && !fixed))) return fail(PL_ERR_ARG, "pl_cond_spmv: null argument");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, "pl_cond_spmv", &w)) return rc;
  if (masked)
    if (int rc = cond_upload_mask(h, fixed, w->fixed.p)) return rc;
  if (int rc = cond_upload(h, x, w->X.p, masked ? fixed : nullptr)) return rc;
  EventTimer timer("pl_cond_spmv", h->stream, "kernel_hip_event");
  launch_cond_gather(h, w, masked != 0, w->X.p, w->AP.p, nullptr);
  PL_HIP(hipGetLastError());
  timer.stop();
  return cond_download(h, w->AP.p, y);
}

namespace {
// pl_cond_solve and pl_cond_solve_adjoint (ambient = false: no H T_inf on the right-hand side, and T_bar is NULL)
int cond_solve_call(pl_handle h, const std::string &who, const uint8_t *fixed, const double *T_bar, const double *q, double rtol,
                    int32_t max_iter, double *T, pl_stats_t *stats, bool ambient) {
  if (valid(h) && (!fixed || !T)) return fail(PL_ERR_ARG, who + ": null argument");
  if (valid(h) && (!(rtol > 0.0) || max_iter <= 0)) return fail(PL_ERR_ARG, who + ": rtol and max_iter must be positive");
  if (valid(h) && stats && stats->struct_size != sizeof(pl_stats_t))
    return fail(PL_ERR_ARG, who + ": stats->struct_size is " + std::to_string(stats->struct_size) +
                                ", this library's pl_stats_t has " + std::to_string(sizeof(pl_stats_t)) + " bytes");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, who.c_str(), &w)) return rc;
  bool any = false;
  for (int64_t i = 0; i < h->N && !any; ++i) any = fixed[i] != 0;
  if (!any && !w->conv)   // (with convection K_T + H is positive definite on its own)
    return fail(PL_ERR_ARG, who + ": the mask fixes no node (K_T is singular without a prescribed temperature)");
  if (int rc = cond_upload_mask(h, fixed, w->fixed.p)) return rc;
  {   // T_bar on the fixed nodes only, zero on the free ones (the lifting K_T T_bar must not see free values)
    std::vector<double> tb((size_t)h->N, 0.0);
    if (T_bar)
      for (int64_t i = 0; i < h->N; ++i)
        if (fixed[i]) tb[(size_t)i] = T_bar[i];
    if (int rc = cond_upload(h, tb.data(), w->TB.p)) return rc;
  }
  if (q)
    if (int rc = cond_upload(h, q, w->QF.p)) return rc;
  double status[pl::M_ST_COUNT] = {};
  EventTimer timer(who.c_str(), h->stream, "kernel_hip_event");
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  if (int rc = cond_pcg(h, w, q ? (const double *)w->QF.p : (const double *)nullptr, rtol, max_iter, w->T.p, status, ambient))
    return rc;
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  timer.stop();
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (int rc = cond_download(h, w->T.p, T)) return rc;
  MultiShape s{1, 1, 1, 1, h->N};
  bool bad = false;
  const int missed = multi_stats(s, status, rtol, ms, stats, &bad);
  if (bad) return fail(PL_ERR_NAN, who + ": NaN/Inf in a residual norm");
  if (missed) return fail(PL_ERR_NOCONV, who + ": rtol not reached within max_iter");
  return PL_OK;
}
}  // namespace

int pl_cond_solve(pl_handle h, const uint8_t *fixed, const double *T_bar, const double *q, double rtol, int32_t max_iter,
                  double *T, pl_stats_t *stats) {
  return cond_solve_call(h, "pl_cond_solve", fixed, T_bar, q, rtol, max_iter, T, stats, true);
}

int pl_cond_solve_adjoint(pl_handle h, const uint8_t *fixed, const double *rhs, double rtol, int32_t max_iter, double *mu,
                          pl_stats_t *stats) {
  if (valid(h) && !rhs) return fail(PL_ERR_ARG, "pl_cond_solve_adjoint: null argument");
  return cond_solve_call(h, "pl_cond_solve_adjoint", fixed, nullptr, rhs, rtol, max_iter, mu, stats, false);
}

int pl_cond_flux(pl_handle h, const double *T, double *Q) {
  if (valid(h) && (!T || !Q)) return fail(PL_ERR_ARG, "pl_cond_flux: null argument");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, "pl_cond_flux", &w)) return rc;
  if (int rc = cond_upload(h, T, w->T.p)) return rc;
  EventTimer timer("pl_cond_flux", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_cond_flux, dim3(grid_for(h->B)), dim3(pl::kBlock), 0, h->stream, h->B, (const int32_t *)h->conn.p,
                     (const double *)h->mult.p, (const double *)w->g.p, (const double *)w->T.p, w->out.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  return download_struts(h, w->out.p, Q);
}

int pl_cond_sens(pl_handle h, const double *T, const double *mu, double *out) {
  if (valid(h) && (!T || !mu || !out)) return fail(PL_ERR_ARG, "pl_cond_sens: null argument");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, "pl_cond_sens", &w)) return rc;
  if (int rc = cond_upload(h, T, w->T.p)) return rc;
  if (int rc = cond_upload(h, mu, w->MU.p)) return rc;
  EventTimer timer("pl_cond_sens", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(w->conv ? pl::k_cond_sens<true> : pl::k_cond_sens<false>, dim3(grid_for(h->B)), dim3(pl::kBlock), 0,
                     h->stream, h->B, (const int32_t *)h->conn.p, (const double *)h->radius.p, (const double *)w->g.p,
                     (const double *)w->T.p, (const double *)w->MU.p, w->out.p,
                     w->conv ? (const double *)w->c.p : (const double *)nullptr, w->T_inf);
  PL_HIP(hipGetLastError());
  timer.stop();
  return download_struts(h, w->out.p, out);
}

int pl_cond_film(pl_handle h, const double *T, double *Qc, double *total) {
  if (valid(h) && (!T || (!Qc && !total))) return fail(PL_ERR_ARG, "pl_cond_film: null argument");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, "pl_cond_film", &w)) return rc;
  if (!w->conv) return fail(PL_ERR_STATE, "pl_cond_film: call pl_set_convection first");
  if (int rc = cond_upload(h, T, w->T.p)) return rc;
  const unsigned grid = grid_for(h->B);
  EventTimer timer("pl_cond_film", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_cond_film, dim3(grid), dim3(pl::kBlock), 0, h->stream, h->B, (const int32_t *)h->conn.p,
                     (const double *)h->mult.p, (const double *)w->c.p, (const double *)w->T.p, w->T_inf,
                     Qc ? w->out.p : (double *)nullptr, total ? w->part.p : (double *)nullptr);
  if (total)
    hipLaunchKernelGGL(pl::k_cond_film_fold, dim3(1), dim3(pl::kBlock), 0, h->stream, (int64_t)grid, (const double *)w->part.p,
                       w->total.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  if (total) {
    PL_HIP(hipMemcpyAsync(total, w->total.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));
  }
  if (Qc) return download_struts(h, w->out.p, Qc);
  return PL_OK;
}

namespace {
// work arrays of pl_temp_pnorm (pl_context::temp_ws), allocated by the first call
struct TempWs {
  DevBuf<double> T, V, G, part, red;   // [N] [N] [N] [blocks] [4]
  DevBuf<uint8_t> nodes;               // [N]
};
}  // namespace

int pl_temp_pnorm(pl_handle h, const double *T, const uint8_t *nodes, double T_ref, double p, double *out, double *dphi_dT) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_temp_pnorm: null handle");
  if (!T || (!out && !dphi_dT)) return fail(PL_ERR_ARG, "pl_temp_pnorm: null argument");
  if (!(p >= 1.0) || !std::isfinite(p)) return fail(PL_ERR_ARG, "pl_temp_pnorm: p must be >= 1 and finite");
  if (!std::isfinite(T_ref)) return fail(PL_ERR_ARG, "pl_temp_pnorm: T_ref must be finite");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_temp_pnorm: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_temp_pnorm: single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_temp_pnorm: call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  const unsigned grid = grid_for(N);
  if (!h->temp_ws) {
    auto t = std::make_shared<TempWs>();
    for (DevBuf<double> *b : {&t->T, &t->V, &t->G}) PL_HIP(b->alloc((size_t)N));
    PL_HIP(t->part.alloc(std::max<size_t>(grid, 1)));
    PL_HIP(t->red.alloc(4));
    PL_HIP(t->nodes.alloc((size_t)N));
    h->temp_ws = t;
  }
  TempWs *t = static_cast<TempWs *>(h->temp_ws.get());
  if (int rc = cond_upload(h, T, t->T.p)) return rc;
  if (nodes)
    if (int rc = cond_upload_mask(h, nodes, t->nodes.p)) return rc;
  EventTimer timer("pl_temp_pnorm", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_temp_values, dim3(grid), dim3(pl::kBlock), 0, h->stream, N, (const double *)t->T.p,
                     nodes ? (const uint8_t *)t->nodes.p : (const uint8_t *)nullptr, T_ref, t->V.p, t->part.p);
  hipLaunchKernelGGL(pl::k_stress_fold<true>, dim3(1), dim3(pl::kBlock), 0, h->stream, (int64_t)grid, t->part.p, p, t->red.p);
  hipLaunchKernelGGL((pl::k_pnorm_psum<1, false>), dim3(grid), dim3(pl::kBlock), 0, h->stream, N, t->V.p, t->red.p, p, t->part.p);
  hipLaunchKernelGGL(pl::k_stress_fold<false>, dim3(1), dim3(pl::kBlock), 0, h->stream, (int64_t)grid, t->part.p, p, t->red.p);
  if (dphi_dT)
    hipLaunchKernelGGL(pl::k_temp_pnorm_grad, dim3(grid), dim3(pl::kBlock), 0, h->stream, N, (const double *)t->V.p,
                       (const double *)t->red.p, p, t->G.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  if (out) {
    double red[3] = {0, 0, 0};
    PL_HIP(hipMemcpyAsync(red, t->red.p, sizeof(red), hipMemcpyDeviceToHost, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));
    out[0] = red[2];
    out[1] = red[0];
    out[2] = red[1];
  }
  if (dphi_dT) return cond_download(h, t->G.p, dphi_dT);
  return PL_OK;
}

int pl_thermal_load_adjoint(pl_handle h, const double *lam, double *out) {
  if (valid(h) && (!lam || !out)) return fail(PL_ERR_ARG, "pl_thermal_load_adjoint: null argument");
  CondWs *w = nullptr;
  if (int rc = cond_begin(h, "pl_thermal_load_adjoint", &w)) return rc;
  ThermalWs *t = static_cast<ThermalWs *>(h->thermal_ws.get());
  if (!t) return fail(PL_ERR_STATE, "pl_thermal_load_adjoint: call pl_set_thermal first (the expansion coefficients)");
  if (!w->lam6.p) PL_HIP(w->lam6.alloc((size_t)h->N * 6));
  std::vector<double> stage;
  if (int rc = upload6(h, lam, w->lam6.p, stage)) return rc;
  EventTimer timer("pl_thermal_load_adjoint", h->stream, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_thermal_load_adjoint, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N,
                     pl::kWave / h->lpn, (const int64_t *)h->slice_ptr.p, (const int2 *)h->ent.p, (const pl::Record *)h->rec.p,
                     (const double *)t->alpha.p, (const double *)w->lam6.p, w->MU.p);
  PL_HIP(hipGetLastError());
  timer.stop();
  return cond_download(h, w->MU.p, out);
}

// ---- global linear buckling (pl_geom.h) --------------------------------------------------------------------------------
namespace {
// what the two geometric calls share after their argument checks: the handle checks and the geometric records of u
int geom_begin(pl_handle h, const char *who, const double *u, bool need_bc, GeomWs **g) {
  if (int rc = multi_check_handle(h, who, need_bc)) return rc;
  if (h->thermal_ws)
    return fail(PL_ERR_STATE, std::string(who) + ": K_g is built from K_e u_e and would ignore the thermal prestress of "
                                                 "pl_set_thermal; clear the thermal state first");
  const double *u_dev = nullptr;
  if (int rc = state_on_device(h, who, u, &u_dev)) return rc;
  if (int rc = geom_ws(h, g)) return rc;
  return launch_geom_records(h, *g, u_dev);
}
}  // namespace

int pl_geom_spmv_multi(pl_handle h, const double *u, int32_t n_rhs, int masked, const double *x, double *y) {
  GeomWs *g = nullptr;
  return spmv_multi_call(h, "pl_geom_spmv_multi", multi_shape, n_rhs, masked, x, y,
                         [&] { return geom_begin(h, "pl_geom_spmv_multi", u, masked != 0, &g); },
                         [&] { return pl::GeomTerm{g->rec.p}; });
}

namespace {
// The pencil G phi = mu K phi of the block subspace iteration: G = sign * A, A the second operator beside K.
//   pl_buckling_modes:   A = K_g(u), sign = -1, value lambda = 1 / mu, shifted by the most negative Ritz value seen,
//                        modes K-orthonormal, residual |K phi + lambda K_g phi| / |K phi|
//   pl_vibration_modes:  A = M,      sign = +1, value omega^2 = 1 / mu, no shift (M is positive definite),
//                        modes scaled by omega to phi^T M phi = 1, residual |K phi - omega^2 M phi| / |K phi|
struct Pencil {
  const char *who;
  double sign;
  bool shifted, second_normalised;
  std::function<int(const MultiShape &, const double *, double *)> apply;     // y = P A x for every column of the shape
};

// argument checks the two eigen-calls share; n_sub = 0 becomes the library's choice
int pencil_check(pl_handle h, const char *who, int32_t n_modes, int32_t &n_sub, double rtol, int32_t max_iter, double tol,
                 int32_t max_outer, const double *value, const int32_t *n_found, const int32_t *outer_iterations) {
  const std::string w(who);
  if (!valid(h) || !value || !n_found || !outer_iterations) return fail(PL_ERR_ARG, w + ": null argument");
  if (n_sub == 0) n_sub = std::max(8, (2 * std::max(n_modes, 1) + 3) / 4 * 4);
  if (n_sub < 4 || n_sub > 32 || n_sub % 4 != 0) return fail(PL_ERR_ARG, w + ": n_sub must be a multiple of 4 in 4 ... 32 (or 0)");
  if (n_modes < 1 || n_modes > n_sub / 2) return fail(PL_ERR_ARG, w + ": n_modes must be 1 ... n_sub / 2");
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, w + ": rtol and max_iter must be positive");
  if (!(tol > 0.0) || max_outer <= 0) return fail(PL_ERR_ARG, w + ": tol and max_outer must be positive");
  if (valid(h) && h->n_per_groups > 0)
    return fail(PL_ERR_STATE, w + ": not available with periodic constraints (pl_set_periodic)");
  return PL_OK;
}

// The n_modes largest mu > 0 of the pencil by block subspace iteration around pcg_solve_multi, value[j] = 1 / mu_j
// ascending: second operator, solve, Rayleigh-Ritz, combine.  The handle checks are the caller's.
int pencil_modes(pl_handle h, GeomWs *g, const Pencil &pc, int32_t n_modes, int32_t n_sub, double rtol, int32_t max_iter,
                 double tol, int32_t max_outer, double *value, double *modes, double *residual, int32_t *n_found,
                 int32_t *outer_iterations) {
  const std::string who(pc.who);
  const int64_t N = h->N, n6 = N * 6;
  const MultiShape s = multi_shape(h, n_sub);     // KB = 4, ncol = n_sub
  const int n = s.ncol;
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s, true, &w)) return rc;
  const unsigned nchunk = std::min(grid_stream(n6), 512u);
  if (int rc = geom_ws_modes(h, g, s, nchunk)) return rc;
  const size_t vec_bytes = (size_t)s.ncb * s.stride * sizeof(double);
  const bool timing = std::getenv("PL_TIMING") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  PL_HIP(hipMemcpyAsync(g->perm.p, h->perm.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));       // (perm is pageable host memory)
  PL_HIP(hipMemsetAsync(w->UB.p, 0, vec_bytes, h->stream));     // zero prescribed values in every solve
  const dim3 gs(grid_stream(n6), (unsigned)s.ncb);
  hipLaunchKernelGGL((pl::k_geom_start<4>), gs, dim3(pl::kBlock), 0, h->stream, n6, (const int32_t *)g->perm.p,
                     (const uint8_t *)h->fixedbits.p, g->Y.p, s.stride);
  PL_HIP(hipGetLastError());

  const double ninf = -std::numeric_limits<double>::infinity();
  std::vector<double> Mh((size_t)2 * n * n), mu, Cm, cur(n_modes, ninf), prev(n_modes, ninf);
  std::vector<double> status((size_t)pl::M_ST_COUNT * s.ncol);
  double mu_low = 0.0, ztol = 0.0, ms_solve = 0.0;
  int rank = 0, outer = 0;
  bool converged = false;
  // Rayleigh-Ritz on span(Y) with products that are applied: X <- Y C, K X <- (K Y) C, A X <- (A Y) C
  auto ritz = [&]() -> int {
    if (int rc = launch_spmv_multi(h, s, h->fixedbits.p, g->Y.p, g->KY.p, true, nullptr)) return rc;
    if (int rc = pc.apply(s, g->Y.p, g->GY.p)) return rc;
    if (int rc = launch_gram(h, g, s, nchunk, g->Y.p, g->KY.p, g->M.p)) return rc;
    if (int rc = launch_gram(h, g, s, nchunk, g->Y.p, g->GY.p, g->M.p + (size_t)n * n)) return rc;
    PL_HIP(hipMemcpyAsync(Mh.data(), g->M.p, Mh.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));
    for (double v : Mh)
      if (!std::isfinite(v)) return fail(PL_ERR_NAN, who + ": NaN/Inf in a projected matrix");
    std::vector<double> Km(Mh.begin(), Mh.begin() + (size_t)n * n), Gm((size_t)n * n);
    for (size_t q = 0; q < Gm.size(); ++q) Gm[q] = pc.sign * Mh[(size_t)n * n + q];      // G = sign A
    rank = ritz_host(n, Km, Gm, mu, Cm);
    PL_HIP(hipMemcpyAsync(g->C.p, Cm.data(), Cm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));     // (Cm is pageable host memory)
    if (int rc = launch_combine(h, g, s, g->Y.p, g->X.p)) return rc;
    if (int rc = launch_combine(h, g, s, g->KY.p, g->KX.p)) return rc;
    if (int rc = launch_combine(h, g, s, g->GY.p, g->GX.p)) return rc;
    double scale = 0.0;
    for (int j = 0; j < rank; ++j) scale = std::max(scale, std::fabs(mu[j]));
    ztol = 1e-10 * scale;
    prev = cur;
    for (int j = 0; j < n_modes; ++j) cur[j] = j < rank ? (std::fabs(mu[j]) <= ztol ? 0.0 : mu[j]) : ninf;
    if (rank > 0) mu_low = std::min(mu_low, mu[rank - 1]);
    return PL_OK;
  };
  if (int rc = ritz()) return rc;                 // K-orthonormalises the start vectors
  while (rank > 0) {
    if (outer == max_outer) break;
    const double sigma = pc.shifted ? std::max(0.0, -mu_low) : 0.0;
    // Y = K^-1 (G X) + sigma X: one multi-column solve with A X as loads, W = K^-1 A X = sign K^-1 G X
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = pcg_solve_multi(h, w, s, h->fixedbits.p, g->GX.p, rtol, max_iter, status.data())) return rc;
    ms_solve += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    hipLaunchKernelGGL(pl::k_multi_axpby, dim3(grid_stream((int64_t)s.ncb * s.stride / 2)), dim3(pl::kBlock), 0, h->stream,
                       (int64_t)s.ncb * s.stride / 2, pc.sign, (const double *)w->U.p, sigma, (const double *)g->X.p, g->Y.p);
    PL_HIP(hipGetLastError());
    if (int rc = ritz()) return rc;
    ++outer;
    double change = 0.0;
    for (int j = 0; j < n_modes; ++j) {
      if (cur[j] == prev[j]) continue;
      change = std::max(change, (cur[j] != 0.0 && std::isfinite(cur[j]) && std::isfinite(prev[j]))
                                    ? std::fabs(cur[j] - prev[j]) / std::fabs(cur[j])
                                    : std::numeric_limits<double>::infinity());
    }
    if (change < tol) { converged = true; break; }
  }
  if (rank == 0) converged = true;                // G vanishes on the free dofs: no value exists
  int found = 0;
  while (found < n_modes && cur[found] > 0.0) ++found;
  *n_found = found;
  *outer_iterations = outer;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int j = 0; j < n_modes; ++j) value[j] = j < found ? 1.0 / cur[j] : nan;
  if (residual)
    for (int j = 0; j < n_modes; ++j) residual[j] = nan;
  if (modes) std::fill(modes, modes + (size_t)n_modes * n6, nan);
  if (found > 0 && (modes || residual)) {
    MultiShape sd = s;                            // the column blocks that hold the found modes
    sd.n_rhs = found;
    sd.ncb = (found + s.KB - 1) / s.KB;
    std::vector<double> own;
    double *phi = modes;
    if (!phi) {
      own.resize((size_t)found * n6);
      phi = own.data();
    }
    if (int rc = multi_download(h, w, sd, g->X.p, phi)) return rc;
    if (residual) {
      std::vector<double> Kp((size_t)found * n6), Gp((size_t)found * n6);
      if (int rc = multi_download(h, w, sd, g->KX.p, Kp.data())) return rc;
      if (int rc = multi_download(h, w, sd, g->GX.p, Gp.data())) return rc;
      for (int j = 0; j < found; ++j) {
        double rr = 0.0, kk = 0.0;
        const double lam = -pc.sign * value[j];      // K phi - value G phi
        for (int64_t e = 0; e < n6; ++e) {
          const double k = Kp[(size_t)j * n6 + e], r = k + lam * Gp[(size_t)j * n6 + e];
          rr += r * r;
          kk += k * k;
        }
        residual[j] = std::sqrt(rr / kk);
      }
    }
    if (modes)
      for (int j = 0; j < found; ++j) {           // largest component positive
        double *p = modes + (size_t)j * n6;
        int64_t big = 0;
        for (int64_t e = 1; e < n6; ++e)
          if (std::fabs(p[e]) > std::fabs(p[big])) big = e;
        if (p[big] < 0.0)
          for (int64_t e = 0; e < n6; ++e) p[e] = -p[e];
        if (pc.second_normalised) {               // phi^T K phi = 1 and phi^T G phi = mu: scale by 1 / sqrt(mu)
          const double sc = std::sqrt(value[j]);
          for (int64_t e = 0; e < n6; ++e) p[e] *= sc;
        }
      }
  }
  if (timing) {
    PL_HIP(hipStreamSynchronize(h->stream));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "[%s] %-28s %10.4f ms\n", pc.who, "whole_call_host_clock", ms);
    std::fprintf(stderr, "[%s] %-28s %10d\n", pc.who, "outer_steps", outer);
    if (outer > 0) {
      std::fprintf(stderr, "[%s] %-28s %10.4f ms\n", pc.who, "outer_step_mean_host_clock", ms / outer);
      std::fprintf(stderr, "[%s] %-28s %10.4f ms\n", pc.who, "inner_solve_mean_host_clock", ms_solve / outer);
    }
  }
  if (!converged) return fail(PL_ERR_NOCONV, who + ": max_outer reached before the Ritz values settled");
  return PL_OK;
}
}  // namespace

int pl_buckling_modes(pl_handle h, const double *u, int32_t n_modes, int32_t n_sub, double rtol, int32_t max_iter, double tol,
                      int32_t max_outer, double *load_factor, double *modes, double *residual, int32_t *n_found,
                      int32_t *outer_iterations) {
  if (int rc = pencil_check(h, "pl_buckling_modes", n_modes, n_sub, rtol, max_iter, tol, max_outer, load_factor, n_found,
                            outer_iterations))
    return rc;
  GeomWs *g = nullptr;
  if (int rc = geom_begin(h, "pl_buckling_modes", u, true, &g)) return rc;
  const Pencil pc = {"pl_buckling_modes", -1.0, true, false, [h, g](const MultiShape &s, const double *x, double *y) {
                       return launch_geom_multi(h, g, s, x, y, true);
                     }};
  return pencil_modes(h, g, pc, n_modes, n_sub, rtol, max_iter, tol, max_outer, load_factor, modes, residual, n_found,
                      outer_iterations);
}

namespace {
// What the two mode-sensitivity calls share around their kernels.  A mode whose value is NaN (beyond n_found of the modes call)
// is skipped: the live ones are the columns.
struct ModeSens {
  std::vector<int> live;           // column -> mode
  MultiShape s;
  MultiWs *w = nullptr;
  unsigned nchunk = 0;
};
// Fills the rows of the skipped modes with NaN, packs the live modes into g->X (zero on the fixed dofs), uploads [value | weight]
// to g->scoef and sizes the workspaces (solver: those of pcg_solve_multi too; quad: g->sq).  No live mode: dsum = 0 and
// ms->live stays empty - the caller returns PL_OK.
int mode_sens_begin(pl_handle h, GeomWs *g, int32_t n_modes, const double *value, const double *modes, const double *weights,
                    bool solver, bool quad, double *rows, double *dsum, ModeSens *ms) {
  const int64_t B = h->B, n6 = h->N * 6;
  for (int j = 0; j < n_modes; ++j)
    if (!std::isnan(value[j])) ms->live.push_back(j);
  const int nl = (int)ms->live.size();
  if (rows) std::fill(rows, rows + (size_t)n_modes * B, std::numeric_limits<double>::quiet_NaN());
  if (nl == 0) {
    if (dsum) std::fill(dsum, dsum + B, 0.0);
    return PL_OK;
  }
  std::vector<double> packed;
  const double *phi_host = modes;
  if (nl < n_modes) {
    packed.resize((size_t)nl * n6);
    for (int j = 0; j < nl; ++j)
      std::memcpy(&packed[(size_t)j * n6], modes + (size_t)ms->live[j] * n6, (size_t)n6 * sizeof(double));
    phi_host = packed.data();
  }
  const MultiShape s = ms->s = multi_shape(h, nl);
  if (int rc = multi_ws(h, s, solver, &ms->w)) return rc;
  ms->nchunk = std::min(grid_stream(n6), 512u);
  if (int rc = geom_ws_modes(h, g, s, ms->nchunk)) return rc;
  if (int rc = geom_ws_sens(h, g, s, quad)) return rc;
  std::vector<double> coef((size_t)2 * s.ncol, 0.0);
  for (int j = 0; j < nl; ++j) {
    coef[(size_t)j] = value[ms->live[j]];
    coef[(size_t)s.ncol + j] = weights ? weights[ms->live[j]] : 0.0;
  }
  PL_HIP(hipMemcpyAsync(g->scoef.p, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));        // (coef is pageable host memory)
  return multi_upload(h, ms->w, s, phi_host, g->X.p, -1);
}
// the per-strut rows g->sdlam[column] back to the rows of their modes, and the weighted sum behind them
int mode_sens_end(pl_handle h, GeomWs *g, const ModeSens &ms, double *rows, double *dsum) {
  const size_t B = (size_t)h->B, nl = ms.live.size();
  if (rows)
    for (size_t j = 0; j < nl; ++j)
      if (int rc = download_struts(h, g->sdlam.p + j * B, rows + (size_t)ms.live[j] * B)) return rc;
  if (dsum)
    if (int rc = download_struts(h, g->sdlam.p + nl * B, dsum)) return rc;
  return PL_OK;
}
}  // namespace

int pl_buckling_modes_sens(pl_handle h, const double *u, int32_t n_modes, const double *load_factor, const double *modes,
                           double rtol, int32_t max_iter, const double *weights, double *dlam_dr, double *dsum_dr,
                           double *adj_load) {
  const char *who = "pl_buckling_modes_sens";
  if (!valid(h) || !load_factor || !modes) return fail(PL_ERR_ARG, "pl_buckling_modes_sens: null argument");
  if (n_modes < 1 || n_modes > 16) return fail(PL_ERR_ARG, "pl_buckling_modes_sens: n_modes must be 1 ... 16");
  if (!dlam_dr && !dsum_dr && !adj_load) return fail(PL_ERR_ARG, "pl_buckling_modes_sens: every output pointer is NULL");
  if (dsum_dr && !weights) return fail(PL_ERR_ARG, "pl_buckling_modes_sens: dsum_dr needs weights");
  if (!(rtol > 0.0) || max_iter <= 0) return fail(PL_ERR_ARG, "pl_buckling_modes_sens: rtol and max_iter must be positive");
  if (h->n_per_groups > 0)
    return fail(PL_ERR_STATE, "pl_buckling_modes_sens: not available with periodic constraints (pl_set_periodic)");
  GeomWs *g = nullptr;
  if (int rc = geom_begin(h, who, u, true, &g)) return rc;
  const double *u_dev = u ? h->tmp.p : h->usol.p;
  const int64_t B = h->B, n6 = h->N * 6;
  if (adj_load) std::fill(adj_load, adj_load + (size_t)n_modes * n6, std::numeric_limits<double>::quiet_NaN());
  ModeSens ms;
  if (int rc = mode_sens_begin(h, g, n_modes, load_factor, modes, weights, true, true, dlam_dr, dsum_dr, &ms)) return rc;
  if (ms.live.empty()) return PL_OK;
  const std::vector<int> &live = ms.live;
  const int nl = (int)live.size();
  const MultiShape s = ms.s;
  MultiWs *w = ms.w;
  EventTimer timer(who, h->stream);
  int rc = PL_OK, missed = 0;
  bool bad = false;
  std::vector<double> status((size_t)pl::M_ST_COUNT * s.ncol);
  do {
    timer.mark("k_geom_quad");
    if ((rc = launch_geom_quad(h, g, s, g->X.p))) break;
    timer.mark("k_geom_adjoint_load");
    if ((rc = launch_adjoint_load(h, g, s, w->F.p))) break;                  // loads -w_i
    timer.mark("K phi and kk (gram)");
    if (dlam_dr || dsum_dr) {
      if ((rc = launch_spmv_multi(h, s, h->fixedbits.p, g->X.p, g->KX.p, true, nullptr))) break;
      if ((rc = launch_gram(h, g, s, ms.nchunk, g->X.p, g->KX.p, g->M.p))) break;    // kk_i on its diagonal
      timer.mark("adjoint pcg_solve_multi");
      if (hipMemsetAsync(w->UB.p, 0, (size_t)s.ncb * s.stride * sizeof(double), h->stream) != hipSuccess) {
        rc = fail(PL_ERR_HIP, "pl_buckling_modes_sens: memset failed");
        break;
      }
      if ((rc = pcg_solve_multi(h, w, s, h->fixedbits.p, w->F.p, rtol, max_iter, status.data()))) break;   // nu_i in w->U
      missed = multi_stats(s, status.data(), rtol, 0.0, nullptr, &bad);
      timer.mark("k_geom_sens");
      if ((rc = launch_geom_sens(h, g, s, u_dev, g->X.p, w->U.p, dlam_dr ? g->sdlam.p : (double *)nullptr,
                                 dsum_dr ? g->sdlam.p + (size_t)nl * B : (double *)nullptr)))
        break;
      timer.mark();
    }
  } while (false);
  if (rc) return rc;
  timer.report();
  if (adj_load) {                                 // w_i = -(the load of the adjoint solve), unmasked
    std::vector<double> wl((size_t)nl * n6);
    if ((rc = multi_download(h, w, s, w->F.p, wl.data()))) return rc;
    for (int j = 0; j < nl; ++j) {
      double *dst = adj_load + (size_t)live[j] * n6;
      for (int64_t e = 0; e < n6; ++e) dst[e] = -wl[(size_t)j * n6 + e];
    }
  }
  if ((rc = mode_sens_end(h, g, ms, dlam_dr, dsum_dr))) return rc;
  if (bad) return fail(PL_ERR_NAN, "pl_buckling_modes_sens: NaN/Inf in a residual norm of the adjoint solve");
  if (missed)
    return fail(PL_ERR_NOCONV, "pl_buckling_modes_sens: " + std::to_string(missed) + " adjoint column(s) did not reach rtol within max_iter");
  return PL_OK;
}

// ---- natural frequencies (pl_mass.h) -----------------------------------------------------------------------------------
namespace {
// what the three mass calls share after their argument checks: the handle checks and the mass records of the current radii
int mass_begin(pl_handle h, const char *who, bool need_bc, MassWs **m) {
  if (int rc = multi_check_handle(h, who, need_bc)) return rc;
  if (h->n_per_groups > 0)
    return fail(PL_ERR_STATE, std::string(who) + ": not available with periodic constraints (pl_set_periodic)");
  if (!h->mass_ws) return fail(PL_ERR_STATE, std::string(who) + ": call pl_set_mass first");
  PL_HIP(hipSetDevice(h->opt.device));
  *m = static_cast<MassWs *>(h->mass_ws.get());
  return launch_mass_records(h, *m);
}
}  // namespace

int pl_set_mass(pl_handle h, double density, int32_t rotary, const double *node_mass) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_mass: null handle");
  if (!(density > 0.0) || !std::isfinite(density)) return fail(PL_ERR_ARG, "pl_set_mass: density must be positive and finite");
  if (rotary != 0 && rotary != 1) return fail(PL_ERR_ARG, "pl_set_mass: rotary must be 0 or 1");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_mass: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_set_mass: single-GPU handles only (this one belongs to a multi-rank run)");
  if (node_mass)
    for (int64_t i = 0; i < h->N; ++i)
      if (!(node_mass[i] >= 0.0) || !std::isfinite(node_mass[i]))
        return fail(PL_ERR_ARG, "pl_set_mass: node_mass must be finite and not negative");
  PL_HIP(hipSetDevice(h->opt.device));
  if (!h->mass_ws) h->mass_ws = std::make_shared<MassWs>();
  MassWs *m = static_cast<MassWs *>(h->mass_ws.get());
  m->density = density;
  m->rotary = rotary;
  m->have_nm = node_mass != nullptr;
  if (node_mass) {
    std::vector<double> nm((size_t)h->N);
    for (int64_t i = 0; i < h->N; ++i) nm[(size_t)i] = node_mass[h->perm[i]];
    if (m->node_mass.n < (size_t)h->N) PL_HIP(m->node_mass.alloc((size_t)h->N));
    PL_HIP(hipMemcpy(m->node_mass.p, nm.data(), (size_t)h->N * sizeof(double), hipMemcpyHostToDevice));
  }
  return PL_OK;
}

int pl_mass_spmv_multi(pl_handle h, int32_t n_rhs, int masked, const double *x, double *y) {
  MassWs *m = nullptr;
  return spmv_multi_call(h, "pl_mass_spmv_multi", multi_shape, n_rhs, masked, x, y,
                         [&] { return mass_begin(h, "pl_mass_spmv_multi", masked != 0, &m); }, [&] { return mass_term(m); });
}

int pl_vibration_modes(pl_handle h, int32_t n_modes, int32_t n_sub, double rtol, int32_t max_iter, double tol,
                       int32_t max_outer, double *omega2, double *modes, double *residual, int32_t *n_found,
                       int32_t *outer_iterations) {
  if (int rc = pencil_check(h, "pl_vibration_modes", n_modes, n_sub, rtol, max_iter, tol, max_outer, omega2, n_found,
                            outer_iterations))
    return rc;
  MassWs *m = nullptr;
  if (int rc = mass_begin(h, "pl_vibration_modes", true, &m)) return rc;
  GeomWs *g = nullptr;
  if (int rc = geom_ws(h, &g)) return rc;
  const Pencil pc = {"pl_vibration_modes", 1.0, false, true, [h, m](const MultiShape &s, const double *x, double *y) {
                       return launch_mass_multi(h, m, s, x, y, true);
                     }};
  return pencil_modes(h, g, pc, n_modes, n_sub, rtol, max_iter, tol, max_outer, omega2, modes, residual, n_found,
                      outer_iterations);
}

int pl_vibration_modes_sens(pl_handle h, int32_t n_modes, const double *omega2, const double *modes, const double *weights,
                            double *domega2_dr, double *dsum_dr) {
  const char *who = "pl_vibration_modes_sens";
  if (!valid(h) || !omega2 || !modes) return fail(PL_ERR_ARG, "pl_vibration_modes_sens: null argument");
  if (n_modes < 1 || n_modes > 16) return fail(PL_ERR_ARG, "pl_vibration_modes_sens: n_modes must be 1 ... 16");
  if (!domega2_dr && !dsum_dr) return fail(PL_ERR_ARG, "pl_vibration_modes_sens: every output pointer is NULL");
  if (dsum_dr && !weights) return fail(PL_ERR_ARG, "pl_vibration_modes_sens: dsum_dr needs weights");
  MassWs *m = nullptr;
  if (int rc = mass_begin(h, who, true, &m)) return rc;
  GeomWs *g = nullptr;
  if (int rc = geom_ws(h, &g)) return rc;
  const int64_t B = h->B;
  ModeSens ms;
  if (int rc = mode_sens_begin(h, g, n_modes, omega2, modes, weights, false, false, domega2_dr, dsum_dr, &ms)) return rc;
  if (ms.live.empty()) return PL_OK;
  const size_t nl = ms.live.size();
  EventTimer timer(who, h->stream, "M phi and mm (gram)");
  if (int rc = launch_mass_multi(h, m, ms.s, g->X.p, g->GX.p, true)) return rc;
  if (int rc = launch_gram(h, g, ms.s, ms.nchunk, g->X.p, g->GX.p, g->M.p)) return rc;     // mm_i = phi_i^T M phi_i on its diagonal
  timer.mark("k_mass_sens");
  if (int rc = launch_mass_sens(h, g, m, ms.s, g->X.p, domega2_dr ? g->sdlam.p : (double *)nullptr,
                                dsum_dr ? g->sdlam.p + nl * B : (double *)nullptr))
    return rc;
  timer.stop();
  return mode_sens_end(h, g, ms, domega2_dr, dsum_dr);
}

// ---- transient heat conduction: implicit theta steps on the strut graph (pl_heat.h) --------------------------------------
int pl_set_heat_capacity(pl_handle h, double rho_c, const double *beam_rho_c, const double *node_capacity) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_set_heat_capacity: null handle");
  if (h->opkind != 0) return fail(PL_ERR_STATE, "pl_set_heat_capacity: not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, "pl_set_heat_capacity: single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->cond_ws) return fail(PL_ERR_STATE, "pl_set_heat_capacity: call pl_set_conduction first");
  CondWs *w = static_cast<CondWs *>(h->cond_ws.get());
  if (rho_c == 0.0 && !beam_rho_c) {
    w->heat.reset();
    return PL_OK;
  }
  if (!beam_rho_c && !(rho_c > 0.0 && std::isfinite(rho_c)))
    return fail(PL_ERR_ARG, "pl_set_heat_capacity: rho_c must be positive and finite");
  if (beam_rho_c)
    for (int64_t b = 0; b < h->B; ++b)
      if (!(beam_rho_c[b] > 0.0 && std::isfinite(beam_rho_c[b])))
        return fail(PL_ERR_ARG, "pl_set_heat_capacity: beam_rho_c must be positive and finite");
  if (node_capacity)
    for (int64_t i = 0; i < h->N; ++i)
      if (!(node_capacity[i] >= 0.0 && std::isfinite(node_capacity[i])))
        return fail(PL_ERR_ARG, "pl_set_heat_capacity: node_capacity must be non-negative and finite");
  PL_HIP(hipSetDevice(h->opt.device));
  const size_t B = (size_t)h->B, N = (size_t)h->N;
  auto hw = std::make_shared<HeatWs>();
  for (DevBuf<double> *b : {&hw->rho_c, &hw->cap}) PL_HIP(b->alloc(B));
  for (DevBuf<double> *b : {&hw->node_cap, &hw->C, &hw->S}) PL_HIP(b->alloc(N));
  std::vector<double> rc(B);
  for (size_t b = 0; b < B; ++b) rc[b] = beam_rho_c ? beam_rho_c[h->bperm[b]] : rho_c;
  PL_HIP(hipMemcpy(hw->rho_c.p, rc.data(), B * sizeof(double), hipMemcpyHostToDevice));
  if (int rcode = cond_upload(h, node_capacity, hw->node_cap.p)) return rcode;
  PL_HIP(hipStreamSynchronize(h->stream));
  w->heat = hw;
  return PL_OK;
}

int pl_cond_transient(pl_handle h, int32_t n_steps, double dt, double theta, const uint8_t *fixed, const double *T_bar,
                      const double *bar_amp, int32_t n_pat, const double *pattern, const double *amp, const double *T0, double rtol,
                      int32_t max_iter, int32_t n_probe, const int32_t *probe_nodes, double *probe, double *heat, int32_t snap_every,
                      double *snaps, double *state, int32_t *iters) {
  const char *who = "pl_cond_transient";
  const std::string whos = who;
  // every check on the host, before any launch
  if (!valid(h)) return fail(PL_ERR_ARG, whos + ": null handle");
  if (n_steps < 1) return fail(PL_ERR_ARG, whos + ": n_steps must be at least 1");
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(PL_ERR_ARG, whos + ": dt must be positive and finite");
  if (!(theta >= 0.5 && theta <= 1.0)) return fail(PL_ERR_ARG, whos + ": theta must lie in [1/2, 1] (unconditionally stable schemes only)");
  if (n_pat < 0 || n_pat > pl::kHeatMaxPat) return fail(PL_ERR_ARG, whos + ": n_pat must be 0 ... 4");
  if (n_pat > 0 && (!pattern || !amp)) return fail(PL_ERR_ARG, whos + ": n_pat > 0 needs pattern and amp");
  if (n_probe < 0 || (n_probe > 0 && (!probe_nodes || !probe))) return fail(PL_ERR_ARG, whos + ": n_probe > 0 needs probe_nodes and probe");
  if (snap_every < 0 || (snaps && snap_every < 1)) return fail(PL_ERR_ARG, whos + ": snaps needs snap_every >= 1");
  if (int rc = check_solve(whos, rtol, max_iter)) return rc;
  if (int rc = check_probes(whos, n_probe, probe_nodes, h->N)) return rc;
  {   // a NaN in the data would otherwise surface as a missed solve, or silently through a fixed node's row value
    const size_t Nh = (size_t)h->N, rows_h = (size_t)n_steps + 1;
    auto finite = [](const double *v, size_t n) {
      for (size_t i = 0; v && i < n; ++i)
        if (!std::isfinite(v[i])) return false;
      return true;
    };
    if (!finite(T0, Nh) || !finite(T_bar, Nh) || !finite(bar_amp, rows_h) || !finite(pattern, Nh * (size_t)n_pat) ||
        !finite(n_pat > 0 ? amp : nullptr, rows_h * (size_t)n_pat))
      return fail(PL_ERR_ARG, whos + ": T0, T_bar, bar_amp, pattern and amp must be finite");
  }
  if (h->opkind != 0) return fail(PL_ERR_STATE, whos + ": not available on a DDM handle");
  if (h->dist.active || h->opt.grid_nodes > 0)
    return fail(PL_ERR_STATE, whos + ": single-GPU handles only (this one belongs to a multi-rank run)");
  if (!h->cond_ws) return fail(PL_ERR_STATE, whos + ": call pl_set_conduction first");
  CondWs *w = static_cast<CondWs *>(h->cond_ws.get());
  if (!w->heat) return fail(PL_ERR_STATE, whos + ": call pl_set_heat_capacity first");
  if (!h->assembled) return fail(PL_ERR_STATE, whos + ": call pl_assemble first");
  HeatWs *hw = static_cast<HeatWs *>(w->heat.get());
  PL_HIP(hipSetDevice(h->opt.device));
  // the two blocks that grow with the length of the history do not outlive the call, however it returns
  struct HistoryRelease {
    HeatWs *hw;
    ~HistoryRelease() {
      hw->probe.release();
      hw->snaps.release();
    }
  } history_release{hw};

  const int64_t N = h->N;
  const size_t Ns = (size_t)N;
  const int rows = n_steps + 1;
  const int n_snap = snaps ? n_steps / snap_every : 0;
  const double T_inf = w->conv ? w->T_inf : 0.0;
  std::vector<int32_t> slot_of, probe_to_slot;
  const int n_slot = probe_map(h, n_probe, probe_nodes, slot_of, probe_to_slot);
  PL_HIP(heat_grow(hw->T2, 2 * Ns));
  PL_HIP(heat_grow(hw->T0, Ns));
  PL_HIP(heat_grow(hw->Tbar, Ns));
  PL_HIP(heat_grow(hw->pattern, Ns * (size_t)std::max(n_pat, 1)));
  PL_HIP(heat_grow(hw->amp, (size_t)rows * std::max(n_pat, 1)));
  PL_HIP(heat_grow(hw->bar_amp, (size_t)rows));
  PL_HIP(heat_grow(hw->probe_slot, Ns));
  PL_HIP(heat_grow(hw->probe, (size_t)rows * std::max(n_slot, 1)));
  PL_HIP(heat_grow(hw->heat, (size_t)rows * pl::HEAT_COUNT * pl::kSlots));
  if (n_snap > 0) PL_HIP(heat_grow(hw->snaps, (size_t)n_snap * Ns));
  if (w->conv && !w->H.p) return fail(PL_ERR_STATE, whos + ": the convection state holds no film sums");
  // uploads, once per call: the mask, the start field, the end values, the patterns, the two tables and the probe map
  if (fixed) {
    if (int rc = cond_upload_mask(h, fixed, w->fixed.p)) return rc;
  } else {
    PL_HIP(hipMemsetAsync(w->fixed.p, 0, Ns, h->stream));
  }
  {
    std::vector<double> t0(Ns, T_inf);
    if (T0) std::memcpy(t0.data(), T0, Ns * sizeof(double));
    if (int rc = cond_upload(h, t0.data(), hw->T0.p)) return rc;
  }
  if (int rc = cond_upload(h, T_bar, hw->Tbar.p)) return rc;
  for (int p = 0; p < n_pat; ++p)
    if (int rc = cond_upload(h, pattern + (size_t)p * Ns, hw->pattern.p + (size_t)p * Ns)) return rc;
  if (n_pat > 0)
    PL_HIP(hipMemcpyAsync(hw->amp.p, amp, (size_t)rows * n_pat * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (bar_amp) PL_HIP(hipMemcpyAsync(hw->bar_amp.p, bar_amp, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipMemcpyAsync(hw->probe_slot.p, slot_of.data(), Ns * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));         // (the tables and slot_of are pageable host memory)
  PL_HIP(hipMemsetAsync(hw->heat.p, 0, (size_t)rows * pl::HEAT_COUNT * pl::kSlots * sizeof(double), h->stream));

  const pl::HeatStep q = {dt, theta, T_inf, n_pat, (const uint8_t *)w->fixed.p, (const double *)hw->T0.p,
                          (const double *)hw->Tbar.p, bar_amp ? (const double *)hw->bar_amp.p : (const double *)nullptr,
                          (const double *)hw->pattern.p, (const double *)hw->amp.p};
  const int SN = pl::kWave / h->lpn;
  const int64_t *sp = (const int64_t *)h->slice_ptr.p;
  const int2 *ent = (const int2 *)h->ent.p;
  const double *g = (const double *)w->g.p;
  const double *H = w->conv ? (const double *)w->H.p : (const double *)nullptr;
  const dim3 gn(grid_for(N)), gs(grid_stream(N)), blk(pl::kBlock);
  const bool timing = std::getenv("PL_TIMING") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  EventTimer timer(who, h->stream, "refresh_hip_event");
  // refresh: g, c and cap of the current radii, then ONE per-node walk for C, H, the step diagonal and the Jacobi diagonal
  if (w->conv) {
    hipLaunchKernelGGL(pl::k_heat_strut<true>, dim3(grid_for(h->B)), blk, 0, h->stream, h->B, (const pl::Record *)h->rec.p,
                       (const double *)h->radius.p, (const double *)h->mult.p, (const double *)w->kappa.p, w->g.p,
                       (const double *)w->film.p, w->c.p, (const double *)hw->rho_c.p, hw->cap.p);
    hipLaunchKernelGGL(pl::k_heat_diag<true>, gn, blk, 0, h->stream, N, SN, sp, ent, g, (const double *)w->c.p,
                       (const double *)hw->cap.p, (const double *)hw->node_cap.p, (const uint8_t *)w->fixed.p, dt, theta, w->H.p,
                       hw->C.p, hw->S.p, w->dinv.p);
  } else {
    hipLaunchKernelGGL(pl::k_heat_strut<false>, dim3(grid_for(h->B)), blk, 0, h->stream, h->B, (const pl::Record *)h->rec.p,
                       (const double *)h->radius.p, (const double *)h->mult.p, (const double *)w->kappa.p, w->g.p,
                       (const double *)nullptr, (double *)nullptr, (const double *)hw->rho_c.p, hw->cap.p);
    hipLaunchKernelGGL(pl::k_heat_diag<false>, gn, blk, 0, h->stream, N, SN, sp, ent, g, (const double *)nullptr,
                       (const double *)hw->cap.p, (const double *)hw->node_cap.p, (const uint8_t *)w->fixed.p, dt, theta,
                       (double *)nullptr, hw->C.p, hw->S.p, w->dinv.p);
  }
  hipLaunchKernelGGL(pl::k_heat_start, gn, blk, 0, h->stream, N, q, (const double *)hw->C.p, hw->T2.p,
                     (const int32_t *)hw->probe_slot.p, n_slot, hw->probe.p, hw->heat.p);
  PL_HIP(hipGetLastError());
  timer.mark("time_loop_hip_event");

  // the time loop: nothing comes down but the status block, once per look
  const MultiScal m = cond_scal(w);
  const int every = h->opt.check_every > 0 ? h->opt.check_every : 16;
  const size_t st_bytes = (size_t)pl::M_ST_COUNT * sizeof(double);
  double status[pl::M_ST_COUNT] = {};
  std::vector<int32_t> its((size_t)rows, 0);
  long looks = 0, total_iters = 0;
  double ms_begin = 0.0, ms_end = 0.0;
  for (int row = 1; row <= n_steps; ++row) {
    const double *Tn = hw->T2.p + (size_t)((row - 1) & 1) * Ns;
    double *Tnew = hw->T2.p + (size_t)(row & 1) * Ns;
    const bool time_row = timing && row == n_steps;   // the two fused kernels of the last step, timed on their own
    PL_HIP(hipMemsetAsync(w->scal.p, 0, kCondScal * sizeof(double), h->stream));
    PL_HIP(hipMemsetAsync(w->flags.p, 0, 2 * sizeof(int), h->stream));
    {
      EventTimer tk(who, h->stream);
      if (time_row) tk.mark("k_heat_begin");
      hipLaunchKernelGGL(w->conv ? pl::k_heat_begin<true> : pl::k_heat_begin<false>, gn, blk, 0, h->stream, N, SN, sp, ent, g, H, q,
                         row, Tn, (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, w->P.p, m.set[0], m.bb);
      if (time_row) ms_begin = tk.lap();
    }
    hipLaunchKernelGGL(pl::k_multi_begin, dim3(1), dim3(pl::kWave), 0, h->stream, 1, rtol, (const double *)m.bb, m.thresh,
                       m.status, m.flag[0]);
    int it = 0, all = 0;
    do {   // the first look comes after min(check_every, max_iter) iterations: past convergence they are no-ops
      const int stop = std::min((int)max_iter, it + every);
      for (; it < stop; ++it) {
        const int a = it & 1, b = a ^ 1;
        hipLaunchKernelGGL(pl::k_heat_gather, gn, blk, 0, h->stream, N, SN, sp, ent, g, (const double *)hw->S.p,
                           (const uint8_t *)w->fixed.p, theta, (const double *)w->P.p, w->AP.p,
                           m.set[a] + (size_t)pl::M_PAP * pl::kSlots);
        hipLaunchKernelGGL((pl::k_multi_update<1>), gs, blk, 0, h->stream, N, (const double *)w->P.p, (const double *)w->AP.p,
                           (const double *)w->dinv.p, w->X.p, w->R.p, w->Z.p, m.set[a], (const int *)m.flag[a], 1, N);
        hipLaunchKernelGGL((pl::k_multi_direction<1>), gs, blk, 0, h->stream, N, (const double *)w->Z.p, w->P.p,
                           (const double *)m.set[a], m.set[b], (const int *)m.flag[a], m.flag[b], (const double *)m.thresh,
                           m.status, it, 1, N);
      }
      PL_HIP(hipGetLastError());
      if (hipMemcpyAsync(status, m.status, st_bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
          hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(PL_ERR_HIP, whos + ": download of the status block failed");
      ++looks;
      all = status[pl::M_ST_FROZEN] == 0.0 ? 0 : 1;
    } while (all == 0 && it < max_iter);
    const double rr = status[pl::M_ST_RR], bb = status[pl::M_ST_BB];
    if (!std::isfinite(rr) || !std::isfinite(bb))
      return fail(PL_ERR_NAN, whos + ": NaN/Inf in a residual norm of step " + std::to_string(row));
    if (!(rr <= rtol * rtol * bb))
      return fail(PL_ERR_NOCONV, whos + ": the solve of step " + std::to_string(row) + " did not reach rtol within max_iter");
    its[(size_t)row] = (int32_t)status[pl::M_ST_ITER];
    total_iters += its[(size_t)row];
    double *snap = nullptr;
    if (n_snap > 0 && row % snap_every == 0) snap = hw->snaps.p + (size_t)(row / snap_every - 1) * Ns;
    {
      EventTimer tk(who, h->stream);
      if (time_row) tk.mark("k_heat_end");
      hipLaunchKernelGGL(w->conv ? pl::k_heat_end<true> : pl::k_heat_end<false>, gn, blk, 0, h->stream, N, SN, sp, ent, g, H,
                         (const double *)hw->C.p, q, row, Tn, (const double *)w->X.p, Tnew, (const int32_t *)hw->probe_slot.p,
                         hw->probe.p + (size_t)row * std::max(n_slot, 1), snap,
                         hw->heat.p + (size_t)row * pl::HEAT_COUNT * pl::kSlots);
      if (time_row) ms_end = tk.lap();
    }
    PL_HIP(hipGetLastError());
  }
  timer.stop();

  // the histories come down once
  if (heat) {
    if (int rc = download_slot_sums(h, hw->heat.p, (size_t)rows * pl::HEAT_COUNT, heat)) return rc;
    for (int r = 1; r < rows; ++r)     // the three exchanged heats are cumulative
      for (int v : {pl::HEAT_QIN, pl::HEAT_QC, pl::HEAT_QR}) heat[r * pl::HEAT_COUNT + v] += heat[(r - 1) * pl::HEAT_COUNT + v];
  }
  if (n_probe > 0) {
    const size_t ld = (size_t)std::max(n_slot, 1);
    std::vector<double> ph((size_t)rows * ld);
    PL_HIP(hipMemcpyAsync(ph.data(), hw->probe.p, ph.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));
    for (size_t r = 0; r < (size_t)rows; ++r)
      for (int i = 0; i < n_probe; ++i) probe[r * n_probe + i] = ph[r * ld + probe_to_slot[(size_t)i]];
  }
  for (int k = 0; k < n_snap; ++k)
    if (int rc = cond_download(h, hw->snaps.p + (size_t)k * Ns, snaps + (size_t)k * Ns)) return rc;
  if (state)
    if (int rc = cond_download(h, hw->T2.p + (size_t)(n_steps & 1) * Ns, state)) return rc;
  if (iters) std::memcpy(iters, its.data(), (size_t)rows * sizeof(int32_t));
  if (timing) {
    PL_HIP(hipStreamSynchronize(h->stream));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    timing_ms(who, "whole_call_host_clock", ms);
    timing_count(who, "steps", (int)n_steps);
    timing_ms(who, "k_heat_begin_last_step", ms_begin);
    timing_ms(who, "k_heat_end_last_step", ms_end);
    timing_mean(who, "iterations_per_step", (double)total_iters / n_steps);
    timing_mean(who, "host_syncs_per_step", (double)looks / n_steps);
  }
  return PL_OK;
}

// ---- transient response (pl_dyn.h) -------------------------------------------------------------------------------------
int pl_dyn_spmv_multi(pl_handle h, double c_K, double c_M, int32_t n_rhs, int masked, const double *x, double *y) {
  MassWs *m = nullptr;
  return spmv_multi_call(h, "pl_dyn_spmv_multi", dyn_shape, n_rhs, masked, x, y, [&]() -> int {
    if (!std::isfinite(c_K) || !std::isfinite(c_M)) return fail(PL_ERR_ARG, "pl_dyn_spmv_multi: c_K and c_M must be finite");
    return mass_begin(h, "pl_dyn_spmv_multi", masked != 0, &m);
  }, [&] { return pl::DynTerm{h->rec.p, mass_term(m), c_K, c_M}; });
}

namespace {
// The run that pl_transient and pl_transient_sens share: its arguments, their checks and the forward pass.
struct TransientRun {
  int32_t n_steps;
  double dt, beta, gamma, ray_m, ray_k;
  int32_t n_pat;                     // the caller's patterns [n_pat][6N] (host)
  const double *pattern, *amp;       // amp: [n_steps + 1][n_pat_dev] for the device's patterns (the caller's, then the base load)
  const double *u0, *v0;
  double rtol;
  int32_t max_iter;
};

int transient_check(pl_handle h, const std::string &who, const TransientRun &a) {
  if (!valid(h)) return fail(PL_ERR_ARG, who + ": null handle");
  if (a.n_steps < 1) return fail(PL_ERR_ARG, who + ": n_steps must be at least 1");
  if (!(a.dt > 0.0) || !std::isfinite(a.dt)) return fail(PL_ERR_ARG, who + ": dt must be positive and finite");
  if (!(a.gamma >= 0.5) || !std::isfinite(a.gamma)) return fail(PL_ERR_ARG, who + ": gamma must be at least 1/2");
  if (!(a.beta >= 0.25 * (0.5 + a.gamma) * (0.5 + a.gamma)) || !std::isfinite(a.beta))
    return fail(PL_ERR_ARG, who + ": beta must be at least (1/2 + gamma)^2 / 4 (unconditionally stable schemes only)");
  if (int rc = check_rayleigh(who, a.ray_m, a.ray_k)) return rc;
  if (a.n_pat < 0 || a.n_pat > 4) return fail(PL_ERR_ARG, who + ": n_pat must be 0 ... 4");
  if (a.n_pat > 0 && (!a.pattern || !a.amp)) return fail(PL_ERR_ARG, who + ": n_pat > 0 needs pattern and amp");
  return check_solve(who, a.rtol, a.max_iter);
}

// the handle checks, the mass records of the current radii, and supports held at zero: prescribed values are refused
int transient_begin(pl_handle h, const char *who, MassWs **m) {
  if (int rc = mass_begin(h, who, true, m)) return rc;
  const int64_t n6 = h->N * 6;
  std::vector<double> ub((size_t)n6);
  PL_HIP(hipMemcpyAsync(ub.data(), h->ubar.p, (size_t)n6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  for (double v : ub)
    if (v != 0.0) return fail(PL_ERR_STATE, std::string(who) + ": the handle carries non-zero prescribed displacements (pl_set_bc)");
  return PL_OK;
}

// The row loop: the initial acceleration and n_steps steps, with the probe block, the energies and the snapshots left on the
// device (DynWs) and the last state in d->st.  hist != null (pl_transient_sens): the base-acceleration pattern P M e_dir is
// formed behind the caller's patterns, and every row leaves wK, wM and the slots of l . u (pl_dyn_sens.h).
struct TransientClock {              // what the PL_TIMING lines of the callers need
  std::chrono::steady_clock::time_point t_begin;
  double ms_solve = 0.0;
  long total_iters = 0;
};
int transient_forward(pl_handle h, const char *who, MassWs *m, const TransientRun &a, const std::vector<int32_t> &slot_of,
                      int n_slot, int snap_every, int n_snap, int32_t *iters, const DynHistory *hist, MultiWs **w_out,
                      DynWs **d_out, TransientClock *clk) {
  const int32_t n_steps = a.n_steps, n_pat = a.n_pat;
  const double dt = a.dt, beta = a.beta, gamma = a.gamma, ray_m = a.ray_m, ray_k = a.ray_k;
  const double *pattern = a.pattern, *amp = a.amp, *u0 = a.u0, *v0 = a.v0;
  const int64_t N = h->N, n6 = N * 6;
  const int rows = n_steps + 1;
  const bool base = hist && hist->base_dir;
  const int n_pat_dev = n_pat + (base ? 1 : 0);
  // workspaces: the column block of four first (it sets the capacity), then the single column of the solves
  MultiShape s4;
  s4.n_rhs = 3; s4.KB = 4; s4.ncb = 1; s4.ncol = 4; s4.stride = n6 * 4;
  MultiShape sp;                                   // the patterns: n_pat single columns
  sp.n_rhs = n_pat; sp.KB = 1; sp.ncb = n_pat; sp.ncol = n_pat; sp.stride = n6;
  const MultiShape s1 = multi_shape(h, 1);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s4, true, &w)) return rc;
  if (int rc = multi_ws(h, s1, true, &w)) return rc;
  if (!h->dyn_ws) h->dyn_ws = std::make_shared<DynWs>();
  DynWs *d = static_cast<DynWs *>(h->dyn_ws.get());
  PL_HIP(dyn_grow(d->st, (size_t)n6 * 4));
  PL_HIP(dyn_grow(d->Ks, (size_t)n6 * 4));
  PL_HIP(dyn_grow(d->Ms, (size_t)n6 * 4));
  PL_HIP(dyn_grow(d->ut, (size_t)n6));
  PL_HIP(dyn_grow(d->vt, (size_t)n6));
  PL_HIP(dyn_grow(d->f2, (size_t)n6 * 2));
  PL_HIP(dyn_grow(d->pattern, (size_t)n6 * std::max(n_pat_dev, 1)));
  PL_HIP(dyn_grow(d->amp, (size_t)rows * std::max(n_pat_dev, 1)));
  PL_HIP(dyn_grow(d->probe_slot, (size_t)N));
  PL_HIP(dyn_grow(d->probe, (size_t)rows * 18 * std::max(n_slot, 1)));
  PL_HIP(dyn_grow(d->energy, (size_t)rows * pl::DYN_E_COUNT * pl::kSlots));
  if (n_snap > 0) PL_HIP(dyn_grow(d->snaps, (size_t)n_snap * n6));
  // uploads: the start state (free dofs only), the patterns (free dofs only), the amplitudes, the probe map
  {
    std::vector<double> s0((size_t)3 * n6, 0.0);
    if (u0) std::memcpy(s0.data(), u0, (size_t)n6 * sizeof(double));
    if (v0) std::memcpy(s0.data() + n6, v0, (size_t)n6 * sizeof(double));
    if (int rc = multi_upload(h, w, s4, s0.data(), d->st.p, -1)) return rc;
  }
  if (n_pat > 0)
    if (int rc = multi_upload(h, w, sp, pattern, d->pattern.p, -1)) return rc;
  if (base)     // P M e_dir behind the caller's patterns; its amplitude column carries -a_g
    if (int rc = base_load(h, w, m, hist->base_dir, hist->s->edir.p, d->pattern.p + (size_t)n_pat * n6)) return rc;
  if (n_pat_dev > 0)
    PL_HIP(hipMemcpyAsync(d->amp.p, amp, (size_t)rows * n_pat_dev * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (hist) {
    if (int rc = multi_upload(h, w, s1, hist->l_host, hist->s->l.p, -1)) return rc;
    PL_HIP(hipMemsetAsync(hist->s->yslots.p, 0, (size_t)rows * pl::kSlots * sizeof(double), h->stream));
  }
  PL_HIP(hipMemcpyAsync(d->probe_slot.p, slot_of.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));         // (amp and slot_of are pageable host memory)
  PL_HIP(hipMemsetAsync(d->f2.p, 0, (size_t)n6 * 2 * sizeof(double), h->stream));
  PL_HIP(hipMemsetAsync(d->energy.p, 0, (size_t)rows * pl::DYN_E_COUNT * pl::kSlots * sizeof(double), h->stream));
  PL_HIP(hipMemsetAsync(w->UB.p, 0, (size_t)n6 * sizeof(double), h->stream));      // zero prescribed values in every solve

  clk->t_begin = std::chrono::steady_clock::now();
  const dim3 gs(grid_stream(n6));
  MultiOp op;
  op.mass = m;
  // K and M on the state, then the energies of row erow; form: the predictors, the load of row erow + 1 and the right-hand side
  auto products_and_predict = [&](const pl::NewmarkCoef &q, bool form, int erow) -> int {
    if (int rc = launch_spmv_multi(h, s4, h->fixedbits.p, d->st.p, d->Ks.p, true, nullptr)) return rc;
    if (int rc = launch_mass_multi(h, m, s4, d->st.p, d->Ms.p, true)) return rc;
    const int row = erow + 1;
    hipLaunchKernelGGL(pl::k_newmark_predict, gs, dim3(pl::kBlock), 0, h->stream, n6, (const double *)d->st.p,
                       (const double *)d->Ks.p, (const double *)d->Ms.p, (const uint8_t *)h->fixedbits.p, q, form ? 1 : 0,
                       n_pat_dev, (const double *)d->pattern.p, (const double *)d->amp.p + (size_t)(form ? row : 0) * n_pat_dev,
                       d->ut.p, d->vt.p, d->f2.p + (size_t)(row & 1) * n6, w->F.p, d->energy.p, erow);
    PL_HIP(hipGetLastError());
    return PL_OK;
  };
  for (int row = 0; row <= n_steps; ++row) {       // row 0: the initial acceleration, the same three stages with dt = 0
    const pl::NewmarkCoef q = {row == 0 ? 0.0 : dt, beta, gamma, ray_m, ray_k};
    op.c_M = 1.0 + gamma * q.dt * ray_m;
    op.c_K = beta * q.dt * q.dt + gamma * q.dt * ray_k;
    if (int rc = products_and_predict(q, true, row - 1)) return rc;
    int its = 0;
    const int rc = transient_solve(h, w, op, a.rtol, a.max_iter, who, hist ? "the forward solve of step" : "the solve of step", row,
                                   &its, &clk->ms_solve);
    clk->total_iters += its;
    if (iters) iters[row] = its;
    if (rc) return rc;
    double *snap = nullptr;
    if (n_snap > 0 && row > 0 && row % snap_every == 0) snap = d->snaps.p + (size_t)(row / snap_every - 1) * n6;
    hipLaunchKernelGGL(pl::k_newmark_correct, gs, dim3(pl::kBlock), 0, h->stream, n6, (const double *)d->ut.p,
                       (const double *)d->vt.p, (const double *)w->U.p, (const double *)d->f2.p + (size_t)((row & 1) ^ 1) * n6,
                       (const double *)d->f2.p + (size_t)(row & 1) * n6, q, d->st.p, (const int32_t *)d->probe_slot.p, n_slot,
                       d->probe.p, snap, d->energy.p, row);
    if (hist) {
      DynSensWs *s = hist->s;
      hipLaunchKernelGGL(pl::k_newmark_history, gs, dim3(pl::kBlock), 0, h->stream, n6, (const double *)d->st.p,
                         (const double *)s->l.p, base ? (const double *)s->edir.p : (const double *)nullptr,
                         base ? hist->base_acc[row] : 0.0, ray_m, ray_k, s->wK.p + (size_t)row * n6, s->wM.p + (size_t)row * n6,
                         s->yslots.p + (size_t)row * pl::kSlots);
    }
    PL_HIP(hipGetLastError());
  }
  if (!hist) {   // the energies of the last row
    const pl::NewmarkCoef q = {dt, beta, gamma, ray_m, ray_k};
    if (int rc = products_and_predict(q, false, n_steps)) return rc;
  }
  *w_out = w;
  *d_out = d;
  return PL_OK;
}
}  // namespace

int pl_transient(pl_handle h, int32_t n_steps, double dt, double beta, double gamma, double ray_m, double ray_k, int32_t n_pat,
                 const double *pattern, const double *amp, const double *u0, const double *v0, double rtol, int32_t max_iter,
                 int32_t n_probe, const int32_t *probe_nodes, double *probe, double *energy, int32_t snap_every, double *snaps,
                 double *state, int32_t *iters) {
  const char *who = "pl_transient";
  const TransientRun a = {n_steps, dt, beta, gamma, ray_m, ray_k, n_pat, pattern, amp, u0, v0, rtol, max_iter};
  if (int rc = transient_check(h, who, a)) return rc;
  if (n_probe < 0 || (n_probe > 0 && (!probe_nodes || !probe))) return fail(PL_ERR_ARG, "pl_transient: n_probe > 0 needs probe_nodes and probe");
  if (snap_every < 0 || (snaps && snap_every < 1)) return fail(PL_ERR_ARG, "pl_transient: snaps needs snap_every >= 1");
  if (int rc = check_probes(who, n_probe, probe_nodes, h->N)) return rc;
  MassWs *m = nullptr;
  if (int rc = transient_begin(h, who, &m)) return rc;
  const int64_t n6 = h->N * 6;
  std::vector<int32_t> slot_of, probe_to_slot;
  const int rows = n_steps + 1, n_slot = probe_map(h, n_probe, probe_nodes, slot_of, probe_to_slot);
  const int n_snap = snaps ? n_steps / snap_every : 0;
  MultiWs *w = nullptr;
  DynWs *d = nullptr;
  TransientClock clk;
  if (int rc = transient_forward(h, who, m, a, slot_of, n_slot, snap_every, n_snap, iters, nullptr, &w, &d, &clk)) return rc;
  const MultiShape s4 = {3, 4, 1, 4, n6 * 4};
  // histories come down once
  if (energy) {
    const size_t ne = pl::DYN_E_COUNT;
    if (int rc = download_slot_sums(h, d->energy.p, rows * ne, energy)) return rc;
    for (int r = 1; r < rows; ++r) energy[r * ne + pl::DYN_E_WORK] += energy[(r - 1) * ne + pl::DYN_E_WORK];   // the work done so far
  }
  if (n_probe > 0) {
    std::vector<double> ph((size_t)rows * 18 * n_slot);
    PL_HIP(hipMemcpyAsync(ph.data(), d->probe.p, ph.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PL_HIP(hipStreamSynchronize(h->stream));
    for (size_t rq = 0; rq < (size_t)rows * 3; ++rq)
      for (int i = 0; i < n_probe; ++i)
        std::memcpy(probe + (rq * n_probe + i) * 6, ph.data() + (rq * n_slot + probe_to_slot[(size_t)i]) * 6, 6 * sizeof(double));
  }
  for (int k = 0; k < n_snap; ++k)
    if (int rc = download6(h, d->snaps.p + (size_t)k * n6, snaps + (size_t)k * n6)) return rc;
  if (state)
    if (int rc = multi_download(h, w, s4, d->st.p, state)) return rc;
  if (std::getenv("PL_TIMING") != nullptr) {
    PL_HIP(hipStreamSynchronize(h->stream));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk.t_begin).count();
    timing_ms(who, "whole_call_host_clock", ms);
    timing_count(who, "steps", (int)n_steps);
    timing_ms(who, "step_mean_host_clock", ms / rows);
    timing_ms(who, "inner_solve_mean_host_clock", clk.ms_solve / rows);
    timing_mean(who, "iterations_per_step", (double)clk.total_iters / rows);
  }
  return PL_OK;
}

int pl_transient_sens(pl_handle h, int32_t n_steps, double dt, double beta, double gamma, double ray_m, double ray_k,
                      int32_t n_pat, const double *pattern, const double *amp, const double *base_dir, const double *base_acc,
                      const double *u0, const double *v0, double rtol, int32_t max_iter, const double *out_vec, int32_t kind,
                      double p, const double *weight, double *J, double *y, double *dJ_dr, int32_t *iters) {
  const char *who = "pl_transient_sens";
  TransientRun a = {n_steps, dt, beta, gamma, ray_m, ray_k, n_pat, pattern, amp, u0, v0, rtol, max_iter};
  if (int rc = transient_check(h, who, a)) return rc;
  if (!out_vec || !J || !dJ_dr) return fail(PL_ERR_ARG, "pl_transient_sens: out_vec, J and dJ_dr must not be NULL");
  if (int rc = check_kind(who, kind, p)) return rc;
  if (base_dir && !base_acc) return fail(PL_ERR_ARG, "pl_transient_sens: base_dir needs base_acc");
  const int rows = n_steps + 1;
  if (int rc = check_weights(who, weight, rows)) return rc;
  MassWs *m = nullptr;
  if (int rc = transient_begin(h, who, &m)) return rc;
  const int64_t n6 = h->N * 6, B = h->B;
  if (!h->dyn_sens_ws) h->dyn_sens_ws = std::make_shared<DynSensWs>();
  DynSensWs *s = static_cast<DynSensWs *>(h->dyn_sens_ws.get());
  PL_HIP(dyn_grow(s->wK, (size_t)rows * n6));
  PL_HIP(dyn_grow(s->wM, (size_t)rows * n6));
  PL_HIP(dyn_grow(s->lam, (size_t)pl::kSensChunk * n6));
  for (DevBuf<double> *b : {&s->mu, &s->nu, &s->Kl, &s->Ml, &s->l, &s->edir}) PL_HIP(dyn_grow(*b, (size_t)n6));
  PL_HIP(dyn_grow(s->yslots, (size_t)rows * pl::kSlots));
  PL_HIP(dyn_grow(s->acc, (size_t)pl::kSensGroups * B));
  PL_HIP(dyn_grow(s->grad, (size_t)B));
  // the amplitudes of the device's patterns: the caller's columns, then -a_g for P M e_dir
  const int n_pat_dev = n_pat + (base_dir ? 1 : 0);
  std::vector<double> amp_dev((size_t)rows * std::max(n_pat_dev, 1), 0.0);
  for (int n = 0; n < rows; ++n) {
    for (int q = 0; q < n_pat; ++q) amp_dev[(size_t)n * n_pat_dev + q] = amp[(size_t)n * n_pat + q];
    if (base_dir) amp_dev[(size_t)n * n_pat_dev + n_pat] = -base_acc[n];
  }
  a.amp = amp_dev.data();
  const DynHistory hist = {s, out_vec, base_dir, base_acc};
  std::vector<int32_t> its((size_t)2 * rows, 0);
  MultiWs *w = nullptr;
  DynWs *d = nullptr;
  TransientClock clk;
  const std::vector<int32_t> no_probe((size_t)h->N, -1);
  if (int rc = transient_forward(h, who, m, a, no_probe, 0, 0, 0, its.data(), &hist, &w, &d, &clk)) return rc;
  // the one host look between the passes: y_n from its slots, J and c_n = dJ/dy_n
  std::vector<double> yh((size_t)rows), c((size_t)rows);
  if (int rc = download_slot_sums(h, s->yslots.p, (size_t)rows, yh.data())) return rc;
  const double ms_forward = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk.t_begin).count();
  const double Jv = objective_real(rows, yh.data(), kind, p, weight, c.data());
  if (!std::isfinite(Jv)) return fail(PL_ERR_NAN, "pl_transient_sens: the objective is not finite");
  // the backward sweep
  const double c2 = dt * dt * (0.5 - beta), c3 = dt * (1.0 - gamma), cu = beta * dt * dt, cv = gamma * dt;
  const double ca = cu + cv * dt + c2, cb = cv + c3;
  const dim3 gs(grid_stream(n6));
  const MultiShape s1 = multi_shape(h, 1);
  MultiOp op;
  op.mass = m;
  const bool timing = std::getenv("PL_TIMING") != nullptr;
  double ms_solve = 0.0, ms_sens = 0.0;
  long adj_iters = 0;
  PL_HIP(hipMemsetAsync(s->acc.p, 0, (size_t)pl::kSensGroups * B * sizeof(double), h->stream));
  auto adjoint = [&](const double *lam, double c_cur, double a_, double b_, double cl_next, int row) {
    hipLaunchKernelGGL(pl::k_newmark_adjoint, gs, dim3(pl::kBlock), 0, h->stream, n6, lam, (const double *)s->Kl.p,
                       (const double *)s->Ml.p, (const double *)s->l.p, dt, ray_m, ray_k, c_cur, a_, b_, cl_next, s->mu.p,
                       s->nu.p, w->F.p, s->lam.p + (size_t)(row % pl::kSensChunk) * n6);
  };
  adjoint(nullptr, 0.0, ca, cb, cu * c[(size_t)n_steps], 0);     // mu = nu = 0 and the right-hand side of row n_steps
  PL_HIP(hipGetLastError());
  for (int row = n_steps; row >= 0; --row) {
    const double qdt = row == 0 ? 0.0 : dt;
    op.c_M = 1.0 + gamma * qdt * ray_m;
    op.c_K = beta * qdt * qdt + gamma * qdt * ray_k;
    if (int rc = transient_solve(h, w, op, rtol, max_iter, who, "the adjoint solve of step", row, &its[(size_t)rows + row], &ms_solve))
      return rc;
    adj_iters += its[(size_t)rows + row];
    if (row > 0) {
      if (int rc = launch_spmv_multi(h, s1, h->fixedbits.p, w->U.p, s->Kl.p, true, nullptr)) return rc;
      if (int rc = launch_mass_multi(h, m, s1, w->U.p, s->Ml.p, true)) return rc;
      if (row > 1) adjoint(w->U.p, c[(size_t)row], ca, cb, cu * c[(size_t)row - 1], row);
      else adjoint(w->U.p, c[(size_t)row], c2, c3, 0.0, row);     // the right-hand side of M lam_0
      PL_HIP(hipGetLastError());
    } else {
      PL_HIP(hipMemcpyAsync(s->lam.p, w->U.p, (size_t)n6 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    if (row % pl::kSensChunk == 0) {   // the chunk whose first row this is
      EventTimer timer(who, h->stream, "k_transient_sens");
      if (int rc = launch_transient_sens(h, m, s, row, std::min(pl::kSensChunk, rows - row))) return rc;
      ms_sens += timer.lap();
    }
  }
  hipLaunchKernelGGL(pl::k_transient_sens_sum, dim3(grid_for(B)), dim3(pl::kBlock), 0, h->stream, B, (const double *)s->acc.p,
                     s->grad.p);
  PL_HIP(hipGetLastError());
  if (int rc = download_struts(h, s->grad.p, dJ_dr)) return rc;
  *J = Jv;
  if (y) std::memcpy(y, yh.data(), (size_t)rows * sizeof(double));
  if (iters) std::memcpy(iters, its.data(), its.size() * sizeof(int32_t));
  if (timing) {
    PL_HIP(hipStreamSynchronize(h->stream));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk.t_begin).count();
    timing_ms(who, "whole_call_host_clock", ms);
    timing_count(who, "steps", (int)n_steps);
    timing_ms(who, "forward_pass_host_clock", ms_forward);
    timing_ms(who, "adjoint_pass_host_clock", ms - ms_forward);
    timing_ms(who, "inner_solve_mean_host_clock", (clk.ms_solve + ms_solve) / (2 * rows));
    timing_mean(who, "forward_iterations_per_step", (double)clk.total_iters / rows);
    timing_mean(who, "adjoint_iterations_per_step", (double)adj_iters / rows);
    timing_ms(who, "k_transient_sens", ms_sens);
    timing_mean(who, "k_transient_sens_share", 100.0 * ms_sens / ms, " %");
  }
  return PL_OK;
}

// ---- frequency response (pl_harm.h) ------------------------------------------------------------------------------------
int pl_harm_spmv(pl_handle h, int32_t n_freq, const double *coef, int masked, const double *x, double *y) {
  const char *who = "pl_harm_spmv";
  if (!valid(h) || !coef || !x || !y) return fail(PL_ERR_ARG, "pl_harm_spmv: null argument");
  if (n_freq < 1 || n_freq > kHarmMaxFreq) return fail(PL_ERR_ARG, "pl_harm_spmv: n_freq must be 1 ... PL_MULTI_MAX / 2");
  for (int i = 0; i < 4 * n_freq; ++i)
    if (!std::isfinite(coef[i])) return fail(PL_ERR_ARG, "pl_harm_spmv: the coefficients must be finite");
  MassWs *m = nullptr;
  if (int rc = mass_begin(h, who, masked != 0, &m)) return rc;
  const MultiShape s = harm_shape(h, n_freq);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, s, false, &w)) return rc;
  HarmWs *hw = nullptr;
  if (int rc = harm_ws(h, &hw)) return rc;
  PL_HIP(hipMemcpyAsync(hw->coef.p, coef, (size_t)4 * n_freq * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (int rc = harm_upload(h, w, n_freq, x, nullptr, false, w->F.p, masked ? -1 : 0)) return rc;
  EventTimer timer(who, h->stream, "kernel_hip_event");
  if (int rc = launch_harm_multi(h, m, s, hw->coef.p, w->F.p, w->U.p, masked != 0)) return rc;
  timer.stop();
  return harm_download(h, w, n_freq, w->U.p, y);
}

int pl_harmonic(pl_handle h, int32_t n_freq, const double *omega, double ray_m, double ray_k, const double *load_re,
                const double *load_im, int32_t n_probe, const int32_t *probe_nodes, double rtol, int32_t max_iter, int32_t block,
                double *probe_out, double *fields, double *power, int32_t *iters, double *relres, int32_t *status) {
  const char *who = "pl_harmonic";
  if (!valid(h) || !omega || !load_re || !iters || !relres || !status) return fail(PL_ERR_ARG, "pl_harmonic: null argument");
  if (int rc = check_omega(who, n_freq, omega)) return rc;
  if (int rc = check_rayleigh(who, ray_m, ray_k)) return rc;
  if (int rc = check_solve(who, rtol, max_iter)) return rc;
  if (block < 0 || block > kHarmMaxFreq) return fail(PL_ERR_ARG, "pl_harmonic: block must be 0 ... PL_MULTI_MAX / 2");
  if (n_probe < 0 || (n_probe > 0 && (!probe_nodes || !probe_out)))
    return fail(PL_ERR_ARG, "pl_harmonic: n_probe > 0 needs probe_nodes and probe_out");
  if (int rc = check_probes(who, n_probe, probe_nodes, h->N)) return rc;
  MassWs *m = nullptr;
  if (int rc = transient_begin(h, who, &m)) return rc;
  const int64_t N = h->N, n6 = N * 6;
  const int nb = std::min<int>(block == 0 ? kHarmMaxFreq : block, n_freq);
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, harm_shape(h, nb), true, &w)) return rc;
  HarmWs *hw = nullptr;
  if (int rc = harm_ws(h, &hw)) return rc;
  std::vector<int32_t> slot_of, probe_to_slot;
  const int n_slot = probe_map(h, n_probe, probe_nodes, slot_of, probe_to_slot);
  PL_HIP(dyn_grow(hw->probe, (size_t)nb * std::max(n_slot, 1) * 12));
  PL_HIP(hipMemcpyAsync(hw->probe_slot.p, slot_of.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  if (int rc = harm_upload(h, w, 1, load_re, load_im, true, w->F.p, -1)) return rc;   // (its wait covers slot_of too)

  const dim3 gs(harm_grid(n6));
  std::vector<double> ph((size_t)nb * std::max(n_slot, 1) * 12);
  const std::vector<double> coef = harm_coef(n_freq, omega, ray_m, ray_k);
  int bad = 0;
  std::chrono::steady_clock::time_point t_begin;
  // after the solves of a pass: K u and M u of the fields, then the probes and the power sums
  auto products_and_outputs = [&](int f0, int nf) -> int {
    const MultiShape s = harm_shape(h, nf);
    if (int rc = launch_spmv_multi(h, s, h->fixedbits.p, w->X.p, w->KU.p, true, nullptr)) return rc;
    if (int rc = launch_mass_multi(h, m, s, w->X.p, w->AP.p, true)) return rc;
    PL_HIP(hipMemsetAsync(hw->power.p, 0, (size_t)nf * pl::H_PW_COUNT * pl::kSlots * sizeof(double), h->stream));
    hipLaunchKernelGGL(pl::k_harm_epilogue, dim3(gs.x, (unsigned)nf), dim3(pl::kBlock), 0, h->stream, n6, (const double *)w->F.p,
                       (const double *)w->X.p, (const double *)w->KU.p, (const double *)w->AP.p,
                       (const int32_t *)hw->probe_slot.p, n_slot, hw->probe.p, hw->power.p, s.stride);
    PL_HIP(hipGetLastError());
    if (n_slot > 0)
      PL_HIP(hipMemcpyAsync(ph.data(), hw->probe.p, (size_t)nf * n_slot * 12 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (power) {   // (its wait covers ph too)
      if (int rc = download_slot_sums(h, hw->power.p, (size_t)nf * pl::H_PW_COUNT, power + (size_t)f0 * pl::H_PW_COUNT)) return rc;
    } else {
      PL_HIP(hipStreamSynchronize(h->stream));
    }
    for (int j = 0; j < nf; ++j)
      for (int i = 0; i < n_probe; ++i)
        std::memcpy(probe_out + ((size_t)(f0 + j) * n_probe + i) * 12,
                    ph.data() + ((size_t)j * n_slot + probe_to_slot[(size_t)i]) * 12, 12 * sizeof(double));
    return fields ? harm_download(h, w, nf, w->X.p, fields + (size_t)f0 * 2 * n6) : PL_OK;
  };
  if (int rc = harm_passes(h, w, hw, m, who, n_freq, coef.data(), nb, 1, nullptr, rtol, max_iter, nullptr, "iterations_per_frequency",
                           iters, relres, status, &bad, &t_begin, products_and_outputs))
    return rc;
  if (std::getenv("PL_TIMING") != nullptr)
    timing_ms(who, "whole_call_host_clock", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  if (bad)
    return fail(PL_ERR_NOCONV, "pl_harmonic: " + std::to_string(bad) + " frequencies ended without convergence (see status)");
  return PL_OK;
}

// ---- frequency response sensitivities (pl_harm_sens.h) -------------------------------------------------------------------
int pl_harmonic_sens(pl_handle h, int32_t n_freq, const double *omega, double ray_m, double ray_k, const double *load_re,
                     const double *load_im, const double *base_dir, const double *out_vec, int32_t kind, double p,
                     const double *weight, double rtol, int32_t max_iter, int32_t block, double *J, double *y, double *dJ_dr,
                     int32_t *iters, double *relres, int32_t *status) {
  const char *who = "pl_harmonic_sens";
  if (!valid(h) || !omega) return fail(PL_ERR_ARG, "pl_harmonic_sens: null argument");
  if (!J || !dJ_dr) return fail(PL_ERR_ARG, "pl_harmonic_sens: J and dJ_dr must not be NULL");
  if (!load_re && !base_dir) return fail(PL_ERR_ARG, "pl_harmonic_sens: neither a load nor base_dir");
  if (load_im && !load_re) return fail(PL_ERR_ARG, "pl_harmonic_sens: load_im needs load_re");
  if (int rc = check_omega(who, n_freq, omega)) return rc;
  if (int rc = check_rayleigh(who, ray_m, ray_k)) return rc;
  if (int rc = check_solve(who, rtol, max_iter)) return rc;
  const bool self_adjoint = out_vec == nullptr;
  const int pass_max = self_adjoint ? kHarmMaxFreq : kHarmSensMaxFreq;
  if (block < 0 || block > pass_max)
    return fail(PL_ERR_ARG, "pl_harmonic_sens: block must be 0 ... PL_MULTI_MAX / 4 (PL_MULTI_MAX / 2 with out_vec = NULL)");
  if (int rc = check_kind(who, kind, p)) return rc;
  if (base_dir)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(base_dir[k])) return fail(PL_ERR_ARG, "pl_harmonic_sens: base_dir must be finite");
  if (int rc = check_weights(who, weight, n_freq)) return rc;
  MassWs *m = nullptr;
  if (int rc = transient_begin(h, who, &m)) return rc;
  const int64_t n6 = h->N * 6, n12 = h->N * 12, B = h->B;
  const int nb = std::min<int>(block == 0 ? pass_max : block, n_freq);     // frequencies per pass
  const int per = self_adjoint ? 1 : 2;                                   // column blocks per frequency
  MultiWs *w = nullptr;
  if (int rc = multi_ws(h, harm_shape(h, per * nb), true, &w)) return rc;
  HarmWs *hw = nullptr;
  if (int rc = harm_ws(h, &hw)) return rc;
  if (!h->harm_sens_ws) h->harm_sens_ws = std::make_shared<HarmSensWs>();
  HarmSensWs *s = static_cast<HarmSensWs *>(h->harm_sens_ws.get());
  PL_HIP(dyn_grow(s->U, (size_t)n_freq * n12));
  if (!self_adjoint) PL_HIP(dyn_grow(s->L, (size_t)n_freq * n12));
  PL_HIP(dyn_grow(s->fl, (size_t)2 * n12));
  PL_HIP(dyn_grow(s->edir, (size_t)n6));
  PL_HIP(dyn_grow(s->Me, (size_t)n6));
  PL_HIP(dyn_grow(s->coef, (size_t)4 * n_freq));
  PL_HIP(dyn_grow(s->g, (size_t)2 * n_freq));
  PL_HIP(dyn_grow(s->yslots, (size_t)2 * n_freq * pl::kSlots));
  PL_HIP(dyn_grow(s->acc, (size_t)pl::kHarmSensGroups * B));
  PL_HIP(dyn_grow(s->grad, (size_t)B));
  // the load f (0 on fixed dofs), with a base minus P M e_dir, and the output vector l
  double *f_dev = s->fl.p, *l_dev = self_adjoint ? s->fl.p : s->fl.p + n12;
  if (load_re) {
    if (int rc = harm_upload(h, w, 1, load_re, load_im, true, f_dev, -1)) return rc;
  } else {
    PL_HIP(hipMemsetAsync(f_dev, 0, (size_t)n12 * sizeof(double), h->stream));
  }
  if (base_dir) {
    if (int rc = base_load(h, w, m, base_dir, s->edir.p, s->Me.p)) return rc;
    hipLaunchKernelGGL(pl::k_harm_base_load, dim3(grid_stream(n6)), dim3(pl::kBlock), 0, h->stream, n6, (const double *)s->Me.p,
                       f_dev);
    PL_HIP(hipGetLastError());
  }
  if (!self_adjoint)
    if (int rc = harm_upload(h, w, 1, out_vec, nullptr, true, l_dev, -1)) return rc;

  const std::vector<double> coef_all = harm_coef(n_freq, omega, ray_m, ray_k);
  std::vector<int32_t> its((size_t)2 * n_freq, 0), stat((size_t)2 * n_freq, 0);
  std::vector<double> rres((size_t)2 * n_freq, 0.0);
  const double *loads[2] = {f_dev, l_dev};   // every column block reads its own load: f for the fields, l for the adjoint fields
  int bad = 0;
  std::chrono::steady_clock::time_point t_begin;
  auto keep_fields = [&](int f0, int nf) -> int {
    PL_HIP(hipMemcpyAsync(s->U.p + (size_t)f0 * n12, w->X.p, (size_t)nf * n12 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (!self_adjoint)
      PL_HIP(hipMemcpyAsync(s->L.p + (size_t)f0 * n12, w->X.p + (size_t)nf * n12, (size_t)nf * n12 * sizeof(double),
                            hipMemcpyDeviceToDevice, h->stream));
    return PL_OK;
  };
  if (int rc = harm_passes(h, w, hw, m, who, n_freq, coef_all.data(), nb, per, loads, rtol, max_iter, "pass_column_blocks",
                           "iterations_per_solve", its.data(), rres.data(), stat.data(), &bad, &t_begin, keep_fields))
    return rc;
  if (iters) std::memcpy(iters, its.data(), its.size() * sizeof(int32_t));
  if (relres) std::memcpy(relres, rres.data(), rres.size() * sizeof(double));
  if (status) std::memcpy(status, stat.data(), stat.size() * sizeof(int32_t));
  if (bad) {
    PL_HIP(hipStreamSynchronize(h->stream));
    return fail(PL_ERR_NOCONV, "pl_harmonic_sens: " + std::to_string(bad) + " solves ended without convergence (see status)");
  }
  // the one host look between the solves and the contraction: y_k from its slots, J and g_k = dJ/dy_k
  PL_HIP(hipMemsetAsync(s->yslots.p, 0, (size_t)2 * n_freq * pl::kSlots * sizeof(double), h->stream));
  hipLaunchKernelGGL(pl::k_harm_output, dim3(harm_grid(n6), (unsigned)n_freq), dim3(pl::kBlock), 0, h->stream, n6,
                     (const double *)l_dev, (const double *)s->U.p, s->yslots.p);
  PL_HIP(hipGetLastError());
  std::vector<double> yh((size_t)2 * n_freq), g((size_t)2 * n_freq);
  if (int rc = download_slot_sums(h, s->yslots.p, (size_t)2 * n_freq, yh.data())) return rc;
  const double Jv = objective_complex(n_freq, yh.data(), kind, p, weight, g.data());
  if (!std::isfinite(Jv)) return fail(PL_ERR_NAN, "pl_harmonic_sens: the objective is not finite");
  for (double v : g)
    if (!std::isfinite(v)) return fail(PL_ERR_NAN, "pl_harmonic_sens: the objective's derivative is not finite");
  PL_HIP(hipMemcpyAsync(s->coef.p, coef_all.data(), coef_all.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PL_HIP(hipMemcpyAsync(s->g.p, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  EventTimer sens_timer(who, h->stream, "k_harmonic_sens");
  const double sfac = base_dir ? (self_adjoint ? 2.0 : 1.0) : 0.0;
  if (int rc = launch_harmonic_sens(h, m, s, self_adjoint, n_freq, sfac, base_dir)) return rc;
  const double ms_sens = sens_timer.lap();
  hipLaunchKernelGGL(pl::k_transient_sens_sum, dim3(grid_for(B)), dim3(pl::kBlock), 0, h->stream, B, (const double *)s->acc.p,
                     s->grad.p);
  PL_HIP(hipGetLastError());
  if (int rc = download_struts(h, s->grad.p, dJ_dr)) return rc;   // (its wait covers coef_all and g too)
  *J = Jv;
  if (y) std::memcpy(y, yh.data(), yh.size() * sizeof(double));
  if (sens_timer.on) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    timing_ms(who, "whole_call_host_clock", ms);
    timing_ms(who, "k_harmonic_sens", ms_sens);
    timing_mean(who, "k_harmonic_sens_share", 100.0 * ms_sens / ms, " %");
  }
  return PL_OK;
}

int pl_schur_cells(const pl_opts_t *o, int32_t n_inst, int32_t n_nodes, int32_t n_beams, const int32_t *beam_conn,
                   int32_t nb, const int32_t *boundary_nodes, const double *node_xyz, const double *beam_radius,
                   const double *seg_len, const int32_t *seg_nsub, double *S, int32_t *info) {
  if (!o || !beam_conn || !boundary_nodes || !node_xyz || !beam_radius || !seg_len || !seg_nsub || !S || !info)
    return fail(PL_ERR_ARG, "pl_schur_cells: null argument");
  if (int rc_abi = check_opts_abi(o, "pl_schur_cells")) return rc_abi;
  if (n_inst <= 0 || n_nodes <= 0 || n_beams <= 0 || nb <= 0 || nb > n_nodes)
    return fail(PL_ERR_ARG, "pl_schur_cells: bad sizes");
  const int32_t ni = n_nodes - nb;
  if (nb > pl::kCondMaxBoundary || ni > pl::kCondMaxInterior || n_beams > pl::kCondMaxBeams)
    return fail(PL_ERR_ARG, "pl_schur_cells: cell too large for the batched condensation (" + std::to_string(nb) +
                                " boundary nodes, " + std::to_string(ni) + " interior nodes, " + std::to_string(n_beams) +
                                " struts; at most " + std::to_string(pl::kCondMaxBoundary) + " / " +
                                std::to_string(pl::kCondMaxInterior) + " / " + std::to_string(pl::kCondMaxBeams) + ")");
  if (!(o->young > 0.0) || !(o->poisson > -1.0) || !(o->kappa > 0.0) || !(o->pen_coef > 0.0))
    return fail(PL_ERR_ARG, "pl_schur_cells: bad material");
  StageTimer stage("pl_schur_cells");
  // slot of every node: its position in boundary_nodes (the row order of S), or -1 - its rank among the other nodes
  std::vector<int32_t> slot((size_t)n_nodes, INT32_MIN);
  for (int i = 0; i < nb; ++i) {
    const int32_t v = boundary_nodes[i];
    if (v < 0 || v >= n_nodes) return fail(PL_ERR_ARG, "pl_schur_cells: boundary node out of range");
    if (slot[v] != INT32_MIN) return fail(PL_ERR_ARG, "pl_schur_cells: boundary node listed twice");
    slot[v] = i;
  }
  for (int32_t v = 0, k = 0; v < n_nodes; ++v)
    if (slot[v] == INT32_MIN) slot[v] = -1 - k++;
  std::vector<int32_t> end_slot(2 * (size_t)n_beams);
  for (int64_t h = 0; h < 2 * (int64_t)n_beams; ++h) {
    const int32_t v = beam_conn[h];
    if (v < 0 || v >= n_nodes) return fail(PL_ERR_ARG, "pl_schur_cells: strut end out of range");
    if ((h & 1) && v == beam_conn[h - 1]) return fail(PL_ERR_ARG, "pl_schur_cells: strut with both ends on one node");
    end_slot[h] = slot[v];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PL_ERR_NODEVICE, "pl_schur_cells: no HIP device visible (libpylattice_hip has no CPU fallback)");
  if (o->device < 0 || o->device >= ndev) return fail(PL_ERR_ARG, "pl_schur_cells: bad device ordinal");
  // one panel when K_II and the whole of V fit 64 KiB (two workgroups per CU); otherwise the widest pair of panels that
  // fits 64 KiB, then 150 KiB (the largest supported cell: 96 x 96 factor, 32 KiB of records, panels of 5 nodes)
  int pw = nb, panels = 1;
  size_t lds = pl::condense_lds_doubles(n_beams, ni, nb, 1) * sizeof(double);
  if (lds > 64 * 1024) {
    pw = 0;
    for (size_t budget : {(size_t)64 * 1024, (size_t)150 * 1024}) {
      for (int w = nb - 1; w >= 1 && pw == 0; --w)
        if (pl::condense_lds_doubles(n_beams, ni, w, 2) * sizeof(double) <= budget) pw = w;
      if (pw) break;
    }
    if (pw == 0) return fail(PL_ERR_ARG, "pl_schur_cells: the cell does not fit the LDS");
    panels = (nb + pw - 1) / pw;
    lds = pl::condense_lds_doubles(n_beams, ni, pw, panels) * sizeof(double);
  }
  stage.mark("validate");
  PL_HIP(hipSetDevice(o->device));
  const size_t m = 6 * (size_t)nb, ninst = (size_t)n_inst;
  DevBuf<int32_t> dconn, dslot, dnsub, dinfo;
  DevBuf<double> dxyz, drad, dlen, dS;
  PL_HIP(dconn.alloc(2 * (size_t)n_beams));
  PL_HIP(dslot.alloc(2 * (size_t)n_beams));
  PL_HIP(dxyz.alloc(ninst * 3 * n_nodes));
  PL_HIP(drad.alloc(ninst * n_beams));
  PL_HIP(dlen.alloc(ninst * 3 * n_beams));
  PL_HIP(dnsub.alloc(ninst * 3 * n_beams));
  PL_HIP(dS.alloc(ninst * m * m));
  PL_HIP(dinfo.alloc(ninst));
  PL_HIP(hipMemcpy(dconn.p, beam_conn, dconn.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dslot.p, end_slot.data(), dslot.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dxyz.p, node_xyz, dxyz.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(drad.p, beam_radius, drad.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dlen.p, seg_len, dlen.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dnsub.p, seg_nsub, dnsub.n * sizeof(int32_t), hipMemcpyHostToDevice));
  stage.mark("upload");
  pl::CondenseArgs a;
  a.n_nodes = n_nodes;
  a.n_beams = n_beams;
  a.nb = nb;
  a.ni = ni;
  a.pw = pw;
  a.conn = dconn.p;
  a.end_slot = dslot.p;
  a.xyz = dxyz.p;
  a.radius = drad.p;
  a.seg_len = dlen.p;
  a.seg_nsub = dnsub.p;
  a.m = {o->young, o->young / (2.0 * (1.0 + o->poisson)), o->kappa, o->pen_coef};
  a.S = dS.p;
  a.info = dinfo.p;
  if (lds > 64 * 1024)
    PL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pl::k_schur_cells),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  EventTimer kernel_time("pl_schur_cells", nullptr, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_schur_cells, dim3((unsigned)n_inst), dim3(pl::kCondBlock), lds, nullptr, a);
  kernel_time.mark();
  PL_HIP(hipGetLastError());
  PL_HIP(hipDeviceSynchronize());
  kernel_time.report();
  stage.mark("kernel");
  PL_HIP(hipMemcpy(S, dS.p, dS.n * sizeof(double), hipMemcpyDeviceToHost));
  PL_HIP(hipMemcpy(info, dinfo.p, ninst * sizeof(int32_t), hipMemcpyDeviceToHost));
  stage.mark("download");
  return PL_OK;
}

int pl_cells_recover(const pl_opts_t *o, int32_t n_inst, int32_t n_nodes, int32_t n_beams, const int32_t *beam_conn,
                     int32_t nb, const int32_t *boundary_nodes, const double *node_xyz, const double *beam_radius,
                     const double *seg_len, const int32_t *seg_nsub, const double *u_b, const double *lam_b,
                     double *u_full, double *lam_full, double *sens, int32_t *info) {
  if (!o || !beam_conn || !boundary_nodes || !node_xyz || !beam_radius || !seg_len || !seg_nsub || !u_b || !info)
    return fail(PL_ERR_ARG, "pl_cells_recover: null argument");
  if (!u_full && !lam_full && !sens) return fail(PL_ERR_ARG, "pl_cells_recover: no output asked for");
  if (int rc_abi = check_opts_abi(o, "pl_cells_recover")) return rc_abi;
  if (n_inst <= 0 || n_nodes <= 0 || n_beams <= 0 || nb <= 0 || nb > n_nodes)
    return fail(PL_ERR_ARG, "pl_cells_recover: bad sizes");
  const int32_t ni = n_nodes - nb;
  if (nb > pl::kCondMaxBoundary || ni > pl::kCondMaxInterior || n_beams > pl::kCondMaxBeams)
    return fail(PL_ERR_ARG, "pl_cells_recover: cell too large for the batched recovery (" + std::to_string(nb) +
                                " boundary nodes, " + std::to_string(ni) + " interior nodes, " + std::to_string(n_beams) +
                                " struts; at most " + std::to_string(pl::kCondMaxBoundary) + " / " +
                                std::to_string(pl::kCondMaxInterior) + " / " + std::to_string(pl::kCondMaxBeams) + ")");
  if (!(o->young > 0.0) || !(o->poisson > -1.0) || !(o->kappa > 0.0) || !(o->pen_coef > 0.0))
    return fail(PL_ERR_ARG, "pl_cells_recover: bad material");
  StageTimer stage("pl_cells_recover");
  // slots as in pl_schur_cells: position in boundary_nodes, or -1 - rank among the other nodes (ascending node index)
  std::vector<int32_t> slot((size_t)n_nodes, INT32_MIN);
  for (int i = 0; i < nb; ++i) {
    const int32_t v = boundary_nodes[i];
    if (v < 0 || v >= n_nodes) return fail(PL_ERR_ARG, "pl_cells_recover: boundary node out of range");
    if (slot[v] != INT32_MIN) return fail(PL_ERR_ARG, "pl_cells_recover: boundary node listed twice");
    slot[v] = i;
  }
  for (int32_t v = 0, k = 0; v < n_nodes; ++v)
    if (slot[v] == INT32_MIN) slot[v] = -1 - k++;
  std::vector<int32_t> end_slot(2 * (size_t)n_beams);
  for (int64_t h = 0; h < 2 * (int64_t)n_beams; ++h) {
    const int32_t v = beam_conn[h];
    if (v < 0 || v >= n_nodes) return fail(PL_ERR_ARG, "pl_cells_recover: strut end out of range");
    if ((h & 1) && v == beam_conn[h - 1]) return fail(PL_ERR_ARG, "pl_cells_recover: strut with both ends on one node");
    end_slot[h] = slot[v];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PL_ERR_NODEVICE, "pl_cells_recover: no HIP device visible (libpylattice_hip has no CPU fallback)");
  if (o->device < 0 || o->device >= ndev) return fail(PL_ERR_ARG, "pl_cells_recover: bad device ordinal");
  const size_t lds = pl::recover_lds_doubles(n_beams, ni) * sizeof(double);   // at most 32 + 72 KiB
  const int block = pl::recover_block(n_beams, ni);
  stage.mark("validate");
  PL_HIP(hipSetDevice(o->device));
  const size_t m = 6 * (size_t)nb, n6 = 6 * (size_t)n_nodes, ninst = (size_t)n_inst;
  DevBuf<int32_t> dconn, dslot, dnslot, dnsub, dinfo;
  DevBuf<double> dxyz, drad, dlen, dub, dlb, duf, dlf, dsens;
  PL_HIP(dconn.alloc(2 * (size_t)n_beams));
  PL_HIP(dslot.alloc(2 * (size_t)n_beams));
  PL_HIP(dnslot.alloc((size_t)n_nodes));
  PL_HIP(dxyz.alloc(ninst * 3 * n_nodes));
  PL_HIP(drad.alloc(ninst * n_beams));
  PL_HIP(dlen.alloc(ninst * 3 * n_beams));
  PL_HIP(dnsub.alloc(ninst * 3 * n_beams));
  PL_HIP(dub.alloc(ninst * m));
  if (lam_b) PL_HIP(dlb.alloc(ninst * m));
  if (u_full) PL_HIP(duf.alloc(ninst * n6));
  if (lam_full) PL_HIP(dlf.alloc(ninst * n6));
  if (sens) PL_HIP(dsens.alloc(ninst * n_beams));
  PL_HIP(dinfo.alloc(ninst));
  PL_HIP(hipMemcpy(dconn.p, beam_conn, dconn.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dslot.p, end_slot.data(), dslot.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dnslot.p, slot.data(), dnslot.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dxyz.p, node_xyz, dxyz.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(drad.p, beam_radius, drad.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dlen.p, seg_len, dlen.n * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dnsub.p, seg_nsub, dnsub.n * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dub.p, u_b, dub.n * sizeof(double), hipMemcpyHostToDevice));
  if (lam_b) PL_HIP(hipMemcpy(dlb.p, lam_b, dlb.n * sizeof(double), hipMemcpyHostToDevice));
  stage.mark("upload");
  pl::RecoverArgs a;
  a.n_nodes = n_nodes;
  a.n_beams = n_beams;
  a.nb = nb;
  a.ni = ni;
  a.conn = dconn.p;
  a.end_slot = dslot.p;
  a.node_slot = dnslot.p;
  a.xyz = dxyz.p;
  a.radius = drad.p;
  a.seg_len = dlen.p;
  a.seg_nsub = dnsub.p;
  a.m = {o->young, o->young / (2.0 * (1.0 + o->poisson)), o->kappa, o->pen_coef};
  a.u_b = dub.p;
  a.lam_b = lam_b ? dlb.p : nullptr;
  a.u_full = u_full ? duf.p : nullptr;
  a.lam_full = lam_full ? dlf.p : nullptr;
  a.sens = sens ? dsens.p : nullptr;
  a.info = dinfo.p;
  if (lds > 64 * 1024)
    PL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pl::k_cells_recover),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  EventTimer kernel_time("pl_cells_recover", nullptr, "kernel_hip_event");
  hipLaunchKernelGGL(pl::k_cells_recover, dim3((unsigned)n_inst), dim3((unsigned)block), lds, nullptr, a);
  kernel_time.mark();
  PL_HIP(hipGetLastError());
  PL_HIP(hipDeviceSynchronize());
  kernel_time.report();
  stage.mark("kernel");
  if (u_full) PL_HIP(hipMemcpy(u_full, duf.p, duf.n * sizeof(double), hipMemcpyDeviceToHost));
  if (lam_full) PL_HIP(hipMemcpy(lam_full, dlf.p, dlf.n * sizeof(double), hipMemcpyDeviceToHost));
  if (sens) PL_HIP(hipMemcpy(sens, dsens.p, dsens.n * sizeof(double), hipMemcpyDeviceToHost));
  PL_HIP(hipMemcpy(info, dinfo.p, ninst * sizeof(int32_t), hipMemcpyDeviceToHost));
  stage.mark("download");
  return PL_OK;
}

int pl_get_records(pl_handle h, double *rec) {
  if (!valid(h) || !rec) return fail(PL_ERR_ARG, "pl_get_records: null argument");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_get_records: call pl_assemble first");
  PL_HIP(hipSetDevice(h->opt.device));
  static_assert(sizeof(pl::Record) == 8 * sizeof(double), "a record is a row of eight doubles");
  return download_struts(h, reinterpret_cast<const double *>(h->rec.p), rec, 8);
}

int pl_debug_partition(pl_handle h, int32_t *tile_of_node, int32_t *agg_of_node, int32_t *local_agg_of_node,
                       uint8_t *eliminated) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_debug_partition: null handle");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t N = h->N;
  std::vector<int32_t> tmp((size_t)N);
  // device array (device numbering) -> caller numbering; absent: -1 everywhere
  auto fetch = [&](const int32_t *dev, int32_t *out) -> int {
    if (!out) return PL_OK;
    if (!dev) {
      std::fill(out, out + N, -1);
      return PL_OK;
    }
    PL_HIP(hipMemcpy(tmp.data(), dev, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < N; ++i) out[h->perm[i]] = tmp[(size_t)i];
    return PL_OK;
  };
  if (tile_of_node) {
    std::fill(tile_of_node, tile_of_node + N, -1);
    if (h->opkind == 0)
      for (size_t t = 0; t + 1 < h->h_tile_start.size(); ++t)
        for (int32_t i = h->h_tile_start[t]; i < h->h_tile_start[t + 1]; ++i) tile_of_node[h->perm[i]] = (int32_t)t;
  }
  int rc = fetch(h->opkind == 1 ? (h->dd2_plan ? (const int32_t *)h->dd2_agg.p : (const int32_t *)nullptr)
                                : (h->coarse.enabled ? (const int32_t *)h->coarse.agg_of_node.p : (const int32_t *)nullptr),
                 agg_of_node);
  if (rc) return rc;
  rc = fetch(h->coarseL.enabled ? (const int32_t *)h->coarseL.agg_of_node.p : (const int32_t *)nullptr, local_agg_of_node);
  if (rc) return rc;
  if (eliminated) {
    std::fill(eliminated, eliminated + N, (uint8_t)0);
    if (h->n_cond > 0 && h->cond_ready && h->cflag.p) {
      std::vector<uint8_t> flag((size_t)N);
      PL_HIP(hipMemcpy(flag.data(), h->cflag.p, (size_t)N, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < N; ++i) eliminated[h->perm[i]] = flag[(size_t)i];
    }
  }
  return PL_OK;
}

int pl_algorithmic_bytes(pl_handle h, double *out3) {
  if (!valid(h) || !out3) return fail(PL_ERR_ARG, "pl_algorithmic_bytes: null argument");
  // SURVEY.md 8(d) with the storage widths the next pl_solve really uses: records are fp64 in every mode (w = 8); the PCG
  // vectors are fp32-stored in precision = 1 (x, r, p, K*p: wv = 4) and, for p and K*p only, in precision = 2.
  const double w = 8.0, B = (double)h->B, N = (double)h->N;
  const bool mp = h->assembled && mp_applies(h);
  const double wv = mp ? 4.0 : 8.0;                                    // p and K*p
  const double wx = (mp && h->opt.precision == 1) ? 4.0 : 8.0;         // x, r (and the other vector passes)
  out3[0] = B * (8.0 + 8.0 * w) + N * 6.0 * wv * 2.0;       // bytes_spmv
  out3[1] = out3[0] + 10.0 * (6.0 * N * wx);                // bytes_pcg_iter
  out3[2] = B * (8.0 + 8.0 * w) + (N + 2.0 * B) * (36.0 * w + 4.0);   // bytes_assembly_bsr (the explicit K is fp64)
  return PL_OK;
}

int pl_forget_history(pl_handle h) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_forget_history: null handle");
  h->last_iterations = 0;       // the next solve looks at the residual history every 32 iterations again
  h->xprev_valid = false;       // and starts from zero even with opts.warm_start
  h->xprev2_valid = false;
  h->xprev3_valid = false;
  h->gh_count = 0;
  return PL_OK;
}

int pl_time_kernel(pl_handle h, int which, int reps, double *avg_ms) {
  if (!valid(h) || !avg_ms || reps <= 0) return fail(PL_ERR_ARG, "pl_time_kernel: bad argument");
  if (h->opkind != 0 && which != 0 && which != 3 && which != 10 && which != 11) return fail(PL_ERR_STATE, "pl_time_kernel: DDM handles time K*p / PCG only");
  if (!h->assembled) return fail(PL_ERR_STATE, "pl_time_kernel: call pl_assemble first");
  if ((which == 0 || which == 3 || which == 10 || which == 11) && !h->have_bc) return fail(PL_ERR_STATE, "pl_time_kernel: call pl_set_bc first");
  if ((which == 2 || which == 4) && !h->have_bsr) return fail(PL_ERR_STATE, "pl_time_kernel: needs pl_assemble_bsr");
  PL_HIP(hipSetDevice(h->opt.device));
  const int64_t n6 = h->N * 6;
  int rc = ensure_hist(h, reps + 1);
  if (rc) return rc;
  solver_plan(h);   // which == 3 times the iteration the next pl_solve would run, whatever was called before
  h->stop_use = false;   // (a finished solve has stopped itself on the device: time the iteration, not its early return)
  if (h->small_use && (which == 3 || which == 11)) {     // short form: its buffers (zeroed operands: the timing does not care)
    rc = small_prepare(h);
    if (rc) return rc;
  }
  // a well-defined operand: p = dinv (free dofs) -> nonzero everywhere that matters
  PL_HIP(hipMemcpyAsync(h->p.p, h->dinv.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (which >= 7 && which <= 11) {   // the same operand, fp32-stored, in the z buffer; zeroed fp32 x / r in tmp
    hipLaunchKernelGGL(pl::k_to_float, dim3(grid_for(n6)), dim3(pl::kBlock), 0, h->stream, n6, h->dinv.p,
                       reinterpret_cast<float *>(h->z.p));
    PL_HIP(hipMemsetAsync(h->tmp.p, 0, n6 * sizeof(double), h->stream));
  }
  float *p32 = reinterpret_cast<float *>(h->z.p), *Ap32 = p32 + n6;             // (ids 7 to 11)
  float *x32 = reinterpret_cast<float *>(h->tmp.p), *r32 = x32 + n6;
  auto one = [&](int k) -> int {
    switch (which) {
      case 0: return launch_spmv(h, h->p.p, h->Ap.p, true, h->scal.p + pl::S_PAP * pl::kSlots);
      case 1: {
        int r1 = launch_records(h);
        return r1 ? r1 : build_palette(h);
      }
      case 2: return launch_bsr_fill(h, 0, h->stream);
      case 3: return pcg_iteration(h, k);
      case 4:
        hipLaunchKernelGGL(pl::k_bsr_spmv, dim3(grid_for(h->N)), dim3(pl::kBlock), 0, h->stream, h->N,
                           h->bsr_rowptr.p, h->bsr_col.p, h->bsr_vals.p, h->p.p, h->Ap.p);
        return PL_OK;
      case 5:   // multi-GPU: the interface all-reduce of a K*p alone (pack, RCCL, unpack) - collective call
        if (!h->dist.active) return fail(PL_ERR_STATE, "pl_time_kernel: 5/6 need pl_dist_init");
        return pl::dist_sum_shared(h->dist, h->Ap.p, h->stream, h->scal.p + pl::S_PAP * pl::kSlots, pl::kSlots)
                   ? fail(PL_ERR_HIP, "RCCL all-reduce failed") : PL_OK;
      case 6:   // multi-GPU: the coarse-residual all-reduce alone - collective call
        if (!h->dist.active || !h->coarse.ready) return fail(PL_ERR_STATE, "pl_time_kernel: 6 needs a coarse level");
        return pl::dist_sum_scalars(h->dist, h->coarse.tv, h->coarse.ncp, h->stream)
                   ? fail(PL_ERR_HIP, "RCCL all-reduce failed") : PL_OK;
      case 7:   // K*p on fp32-stored vectors (the operator of opts.precision = 1 / 2), without node elimination
      case 8:   // one whole iteration of the fp32 inner PCG (precision = 1)
      case 9:   // one whole iteration of the mixed PCG (precision = 2: p, K*p fp32; x, r fp64)
        if (!(h->coarse.ready && h->tile.ready && choose_kernel(h) == 3))
          return fail(PL_ERR_STATE, "pl_time_kernel: 7/8/9 need the multi-level PCG on the tile kernel");
        if (which == 7) return launch_spmv_f32(h, p32, Ap32, true, h->scal.p + pl::S_PAP * pl::kSlots);
        return which == 8 ? mp_iteration<float>(h, k, k, p32, Ap32, x32, r32)
                          : mp_iteration<double>(h, k, k, p32, Ap32, h->x.p, h->r.p);
      case 10:   // the operator exactly as the next pl_solve applies it: both passes under node elimination, fp32-stored
                 // operands in the fp32 solver modes
        return mp_applies(h) ? apply_operator<float>(h, p32, Ap32, h->scal.p + pl::S_PAP * pl::kSlots)
                             : apply_operator<double>(h, h->p.p, h->Ap.p, h->scal.p + pl::S_PAP * pl::kSlots);
      case 11:   // one whole iteration exactly as the next pl_solve runs it (storage width and node elimination of its plan)
        return mp_applies(h) && h->opt.precision == 1 ? mp_iteration<float>(h, k, k, p32, Ap32, x32, r32) : pcg_iteration(h, k);
      case 12:   // the kernel of pl_sens_gram on the columns its last call left on the device
        if (h->gram_cols < 1) return fail(PL_ERR_STATE, "pl_time_kernel: 12 needs a pl_sens_gram call on this handle first");
        return launch_sens_gram(h, h->gram_cols, h->gram_x.p, h->gram_out.p);
      default: return fail(PL_ERR_ARG, "pl_time_kernel: unknown kernel id");
    }
  };
  for (int k = 0; k < 3; ++k) {   // warm-up
    rc = one(0);
    if (rc) return rc;
  }
  PL_HIP(hipEventRecord(h->ev0, h->stream));
  for (int k = 0; k < reps; ++k) {
    rc = one(k);
    if (rc) return rc;
  }
  PL_HIP(hipEventRecord(h->ev1, h->stream));
  PL_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  PL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *avg_ms = (double)ms / reps;
  return PL_OK;
}

int pl_node_words_info(pl_handle h, int *classes_on, int *n_classes, int *bytes_on, int *byte_exp) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_node_words_info: null handle");
  const pl::Coarse &cs = h->coarse;
  const bool words = node_words_apply(h);      // (the predicate of the solver's launch helper)
  const bool cls = words && h->assembled && cs.dcl_ready;
  const bool bytes = words && cs.rel_e >= 0;
  if (classes_on) *classes_on = cls ? 1 : 0;
  if (n_classes) *n_classes = h->assembled ? cs.dcl_classes : 0;
  if (bytes_on) *bytes_on = bytes ? 1 : 0;
  if (byte_exp) *byte_exp = bytes ? cs.rel_e : -1;
  return PL_OK;
}

int pl_debug_spd_solve(int device, int32_t n, const double *A, const double *b, double *x, double *quad,
                       int32_t fp32_factor) {
  return fp32_factor ? debug_spd_solve_t<float>(device, n, A, b, x, quad)
                     : debug_spd_solve_t<double>(device, n, A, b, x, quad);
}

int pl_debug_dense_level(int device, int32_t n, const double *A, int32_t bw_blocks, int32_t storage, int32_t trtri_rows,
                         int32_t band_roundtrip, const double *r, const double *add0, double *W, double *Wt, float *Ainv,
                         double *t, double *y, double *quad, double *y_one, double *quad_one, int32_t *one_gemv,
                         int32_t *info) {
  if (n <= 0 || !A || !r || !add0 || !W || !Wt || !Ainv || !t || !y || !quad || !y_one || !quad_one || !one_gemv || !info ||
      bw_blocks < 0 || trtri_rows < 0)
    return fail(PL_ERR_ARG, "pl_debug_dense_level: bad argument");
  switch (storage) {
    case 64:
      return debug_dense_level_t<double>(device, n, A, bw_blocks, trtri_rows, band_roundtrip, r, add0, W, Wt, Ainv, t, y,
                                         quad, y_one, quad_one, one_gemv, info);
    case 32:
      return debug_dense_level_t<float>(device, n, A, bw_blocks, trtri_rows, band_roundtrip, r, add0, W, Wt, Ainv, t, y,
                                        quad, y_one, quad_one, one_gemv, info);
    case 16:
      return debug_dense_level_t<pl::bf16_t>(device, n, A, bw_blocks, trtri_rows, band_roundtrip, r, add0, W, Wt, Ainv, t,
                                             y, quad, y_one, quad_one, one_gemv, info);
  }
  return fail(PL_ERR_ARG, "pl_debug_dense_level: storage must be 64, 32 or 16");
}

int pl_lzone(int device, int64_t n_nodes, int64_t n_beams, const double *node_xyz, const int32_t *beam_conn,
             const double *beam_radius, double *lzone) {
  if (n_nodes <= 0 || n_beams <= 0 || !node_xyz || !beam_conn || !beam_radius || !lzone)
    return fail(PL_ERR_ARG, "pl_lzone: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PL_ERR_NODEVICE, "pl_lzone: no HIP device visible (libpylattice_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PL_ERR_ARG, "pl_lzone: bad device ordinal");
  const int64_t nh = 2 * n_beams;
  std::vector<int64_t> ptr((size_t)n_nodes + 1, 0);
  for (int64_t h = 0; h < nh; ++h) {
    const int32_t v = beam_conn[h];
    if (v < 0 || v >= n_nodes) return fail(PL_ERR_ARG, "pl_lzone: node id out of range");
    ptr[(size_t)v + 1]++;
  }
  for (int64_t i = 0; i < n_nodes; ++i) ptr[i + 1] += ptr[i];
  std::vector<int32_t> half((size_t)nh);
  {
    std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t h = 0; h < nh; ++h) half[(size_t)fill[beam_conn[h]]++] = (int32_t)h;
  }
  PL_HIP(hipSetDevice(device));
  DevBuf<double> dx, dr, dl;
  DevBuf<int32_t> dc, dh;
  DevBuf<int64_t> dp;
  PL_HIP(dx.alloc((size_t)n_nodes * 3));
  PL_HIP(dr.alloc(n_beams));
  PL_HIP(dl.alloc(nh));
  PL_HIP(dc.alloc(nh));
  PL_HIP(dh.alloc(nh));
  PL_HIP(dp.alloc(n_nodes + 1));
  PL_HIP(hipMemcpy(dx.p, node_xyz, (size_t)n_nodes * 3 * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dr.p, beam_radius, n_beams * sizeof(double), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dc.p, beam_conn, nh * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dh.p, half.data(), nh * sizeof(int32_t), hipMemcpyHostToDevice));
  PL_HIP(hipMemcpy(dp.p, ptr.data(), (n_nodes + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pl::k_lzone, dim3(grid_for(nh)), dim3(pl::kBlock), 0, nullptr, nh, dx.p, dc.p, dr.p, dp.p, dh.p,
                     dl.p);
  PL_HIP(hipGetLastError());
  PL_HIP(hipMemcpy(lzone, dl.p, nh * sizeof(double), hipMemcpyDeviceToHost));
  return PL_OK;
}

#ifdef PL_TILE_STAMPS
// experiment builds only (not in the header): the clock stamps of the last tile K*p launch, out[8 * 4096]
int pl_debug_tile_stamps(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(pl::g_tile_stamps), sizeof(unsigned long long) * 8 * 4096) == hipSuccess ? 0 : -2;
}
#endif

int pl_dist_unique_id_bytes(void) { return pl::dist_unique_id_bytes(); }
int pl_dist_unique_id(void *id_out) {
  if (!id_out) return fail(PL_ERR_ARG, "pl_dist_unique_id: null argument");
  return pl::dist_unique_id(id_out) ? fail(PL_ERR_HIP, "ncclGetUniqueId failed") : PL_OK;
}
int pl_dist_loopback_id(void *id_out) {
  if (!id_out) return fail(PL_ERR_ARG, "pl_dist_loopback_id: null argument");
  pl::dist_loopback_id(id_out);
  return PL_OK;
}
int pl_dist_init(pl_handle h, int rank, int world, const void *unique_id, const int32_t *shared_local,
                 const int32_t *shared_global, int32_t n_shared, int32_t n_shared_global) {
  if (!valid(h) || !unique_id || world < 1 || rank < 0 || rank >= world || n_shared < 0)
    return fail(PL_ERR_ARG, "pl_dist_init: bad argument");
  if (n_shared > 0 && (!shared_local || !shared_global)) return fail(PL_ERR_ARG, "pl_dist_init: null index array");
  PL_HIP(hipSetDevice(h->opt.device));
  std::vector<int32_t> loc(n_shared);
  for (int i = 0; i < n_shared; ++i) {
    if (shared_local[i] < 0 || shared_local[i] >= h->N || shared_global[i] < 0 || shared_global[i] >= n_shared_global)
      return fail(PL_ERR_ARG, "pl_dist_init: shared node index out of range");
    loc[i] = h->iperm[shared_local[i]];
  }
  int rc = pl::dist_init(h->dist, rank, world, unique_id, loc.data(), shared_global, n_shared, n_shared_global, h->N,
                         h->stream);
  if (rc == 6)
    return fail(PL_ERR_ARG, "pl_dist_init: loopback group mismatch (all ranks of a loopback id must share one device and one "
                            "world size <= " + std::to_string(pl::kLoopMaxWorld) + ", each rank attaches once)");
  if (rc) return fail(PL_ERR_HIP, "pl_dist_init: communicator setup failed (" + std::to_string(rc) + ")");
  h->h_shared.assign((size_t)h->N, 0);
  for (int i = 0; i < n_shared; ++i) h->h_shared[loc[i]] = 1;
  h->ov_ready = false;
  if (h->coarse.enabled) {   // the tile level and the rank-local dense level leave shared nodes out
    h->cond_ready = false;   // (re-selected at the next pl_set_bc; until then nothing is condensed)
    h->n_cond = 0;
    h->cond_agree = -1;
    PL_HIP(hipMemcpy(h->sharedbits.p, h->h_shared.data(), h->h_shared.size(), hipMemcpyHostToDevice));
    h->coarseL.n_fix = -1;
  }
  h->assembled = false;
  return PL_OK;
}

int pl_dist_abort(pl_handle h) {
  if (!valid(h)) return fail(PL_ERR_ARG, "pl_dist_abort: null handle");
  if (h->dist.loop) {
    std::lock_guard<std::mutex> lk(h->dist.loop->m);
    h->dist.loop->broken = true;
    h->dist.loop->cv.notify_all();
  }
  return PL_OK;
}

int pl_dist_set_peers(pl_handle h, const int32_t *shared_peer) {
  if (!valid(h) || !shared_peer) return fail(PL_ERR_ARG, "pl_dist_set_peers: null argument");
  if (!h->dist.active) return fail(PL_ERR_STATE, "pl_dist_set_peers: call pl_dist_init first");
  PL_HIP(hipSetDevice(h->opt.device));
  int rc = pl::dist_set_peers(h->dist, shared_peer);
  if (rc) return fail(rc == 2 ? PL_ERR_ARG : PL_ERR_HIP, "pl_dist_set_peers: setup failed (" + std::to_string(rc) + ")");
  h->assembled = false;
  // exchange / compute overlap of the tile K*p: which tiles own interface rows
  h->ov_ready = false;
  if (h->opt.overlap >= 0 && h->tile.ready && h->opkind == 0 && !h->h_tile_start.empty()) {
    const int64_t T = (int64_t)h->h_tile_start.size() - 1;
    std::vector<int32_t> iface, inner;
    for (int64_t t = 0; t < T; ++t) {
      bool has = false;
      for (int32_t i = h->h_tile_start[t]; i < h->h_tile_start[t + 1] && !has; ++i) has = h->h_shared[i] != 0;
      (has ? iface : inner).push_back((int32_t)t);
    }
    if (!iface.empty() && !inner.empty()) {
      PL_HIP(h->ov_iface.alloc(iface.size()));
      PL_HIP(h->ov_inner.alloc(inner.size()));
      PL_HIP(hipMemcpy(h->ov_iface.p, iface.data(), iface.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      PL_HIP(hipMemcpy(h->ov_inner.p, inner.data(), inner.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      h->n_ov_iface = (int64_t)iface.size();
      h->n_ov_inner = (int64_t)inner.size();
      if (!h->comm_stream) {
        int prio_low = 0, prio_high = 0;
        PL_HIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        PL_HIP(hipStreamCreateWithPriority(&h->comm_stream, hipStreamNonBlocking, prio_high));
        PL_HIP(hipEventCreateWithFlags(&h->ev_ov_a, hipEventDisableTiming));
        PL_HIP(hipEventCreateWithFlags(&h->ev_ov_x, hipEventDisableTiming));
      }
      h->ov_ready = true;
    }
  }
  return PL_OK;
}

}  // extern "C"
