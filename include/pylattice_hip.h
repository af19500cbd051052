/*
 * pylattice_hip.h — C ABI of libpylattice_hip.so (MI355X / gfx950).
 *
 * The reference (Tcadart/pyLatticeDSO, 100 % Python) has no FFI of its own; the seam this library sits behind is
 * the dolfinx/PETSc work done inside
 *     solve_FEM_FenicsX            src/pyLatticeSim/utils_simulation.py:21-56
 *     SimulationBase.solve_problem src/pyLatticeSim/simulation_base.py:465-514   (assemble K, lifting, LU solve)
 *     get_schur_complement         src/pyLatticeSim/utils_schur.py:22-53
 *     LatticeOpti.calculate_gradient src/pyLatticeOpti/lattice_opti.py:735-907   (u^T dK/dr u, adjoint form)
 * Each entry point below cites the reference code it replaces.  All pointers are caller-owned HOST buffers
 * (C-contiguous) unless the name ends in _dev; device state is owned by the handle.  Every function returns
 * 0 on success or a negative pl_status; pl_last_error() gives the message.  No C++ exceptions cross the ABI.
 * Handles are not thread-safe; distinct handles are independent.
 *
 * Unknown ordering everywhere: node-major, 6 values per node [ux, uy, uz, thx, thy, thz]
 * (mixed P1xP1 space of simulation_base.py:201-213).
 */
#ifndef PYLATTICE_HIP_H
#define PYLATTICE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pl_context *pl_handle;

typedef enum {
  PL_OK = 0,
  PL_ERR_ARG = -1,       /* bad argument (null pointer, negative size, index out of range) */
  PL_ERR_HIP = -2,       /* HIP runtime error (message has the hipError string) */
  PL_ERR_STATE = -3,     /* call order violated (e.g. solve before set_bc) */
  PL_ERR_NOCONV = -4,    /* PCG hit max iterations (solution and stats are still written) */
  PL_ERR_NAN = -5,       /* NaN/Inf detected in the residual */
  PL_ERR_NODEVICE = -6   /* no HIP device visible */
} pl_status;

/* The lattice the FEM mesh is built from.  One entry per DESIGN strut (before joint penalisation); the
 * penalised end segments (LatticeSim.set_penalized_beams, lattice_sim.py:245-308) and the gmsh sub-mesh
 * (latticeGeneration.mesh_lattice_cells, lattice_generation.py:64-101) are described per strut by seg_len/seg_nsub
 * and condensed in closed form on the device. */
typedef struct {
  int64_t n_nodes;
  int64_t n_beams;
  const double *node_xyz;     /* [3*n_nodes] */
  const int32_t *beam_conn;   /* [2*n_beams] point1, point2 */
  const double *beam_radius;  /* [n_beams]   un-penalised radius r (end segments use pen_coef*r) */
  const double *seg_len;      /* [3*n_beams] geometric length of [pen@point1, middle, pen@point2], 0 = absent */
  const int32_t *seg_nsub;    /* [3*n_beams] number of equal P1 sub-elements per segment (>=1 where len>0) */
} pl_mesh_t;

/* ABI handshake.  pl_opts_t and pl_stats_t grow from release to release; a caller compiled (or a ctypes binding written)
 * against another header must fail with PL_ERR_ARG instead of having memory overrun.  Both structs therefore START with
 * the size the CALLER believes they have: pl_default_opts(&o, sizeof o) refuses any other size than the library's and
 * stamps struct_size / abi_version, pl_create / pl_create_ddm check the stamp, and pl_solve checks stats->struct_size,
 * which the caller sets (= sizeof(pl_stats_t)) before the call.  pl_opts_size() / pl_stats_size() / pl_abi_version()
 * let a binding assert its layout when it loads the library. */
#define PL_ABI_VERSION 6u

typedef struct {
  uint32_t struct_size;  /* sizeof(pl_opts_t) as the caller sees it; written by pl_default_opts, checked by pl_create */
  uint32_t abi_version;  /* PL_ABI_VERSION, written by pl_default_opts */
  double young;          /* E   (materials/<name>.json Young_modulus) */
  double poisson;        /* nu */
  double kappa;          /* shear correction, 0.9 in material_definition.py:45 */
  double pen_coef;       /* radius multiplier of penalised segments, 1.5 (beam.py:71) */
  int32_t device;        /* HIP device ordinal */
  int32_t spmv_kernel;   /* 0 = auto (3 if reorder else 2), 1 = per-strut + f64 global atomics, 2 = per-node gather
                            (sliced ELL), 3 = per-strut with LDS tile accumulators (in its LDS-resident form - a tile's rows
                            of x and the record / direction palette in LDS, one 32-bit word per strut visit - whenever the
                            lattice has <= 256 distinct records or strut vectors; environment PL_TILE_LDS=0 keeps the form
                            that gathers from global memory, for A/B runs) */
  int32_t precond;       /* 1 = Jacobi (diagonal); 2 = two-level: Jacobi + rigid-body-mode coarse space on brick
                            aggregates, dense solve; 3 = 2 plus a tile level (rigid-body modes of every K*p tile,
                            6 x 6 block solves); 4 = 3 plus a rank-LOCAL dense level (aggregates of this handle only,
                            nodes shared with other ranks left out, no communication) under the global one: for
                            multi-GPU runs, where the all-reduced global level has to coarsen with the rank count.
                            2, 3 and 4 need reorder = 1;
                            5 = the dense Cholesky factor of P K P + (I - P) itself (6 n_nodes <= PL_DDM_DENSE_MAX; built by
                            pl_assemble from the BSR blocks, fp64 inverse factor): the PCG converges in one or two steps - what
                            PETSc's preonly / LU is to the reference, for lattices of a few hundred nodes (its own presets) where
                            hundreds of PCG iterations cost more than a factorisation; pl_stats_t.precond_used = 5, or 1 (Jacobi)
                            when the matrix is not positive definite (a mechanism).  Single-GPU handles */
  int32_t reorder;       /* 0 = keep caller's node numbering on the device, 1 = spatial tile reordering */
  int32_t check_every;   /* PCG: iterations between host-side convergence checks; 0 = adaptive (32 while far from
                            the threshold, then what the observed decay rate predicts is still needed) */
  int32_t lanes_per_node;/* gather kernels: wave lanes sharing one node, 1/2/4/8/16 (0 -> 4) */
  int32_t tile_nodes;    /* target nodes per brick/tile of the spatial reordering, <= 512 (0 -> 256) */
  int32_t coarse_max_dofs; /* precond = 2/3: upper bound on 6 * (number of aggregates) (0 -> 2100 below 10^6 nodes
                              on one GPU, 3072 otherwise) */
  int32_t palette;       /* 1: K*p (LDS-tile kernel) reads 2-byte palette ids instead of 64-byte records when the lattice
                            has <= ~30 000 distinct records (compared on 40 mantissa bits, i.e. to 1e-12) */
  int32_t local_max_dofs;  /* precond = 4: upper bound on 6 * (aggregates of the rank-local level) (0 -> 3072) */
  int32_t precision;     /* storage precision of the PCG vectors (multi-level PCG on the LDS-tile kernel, i.e. precond >=
                            2 with reorder = 1; any other configuration runs fp64).  0 = fp64.  1 = fp32 inner PCG with
                            fp64 refinement: x, r, p, K*p stored in fp32, restart from the TRUE fp64 residual
                            P(f - K u) every ~4 decades.  2 = only p and K*p stored in fp32, x and the residual
                            recurrence in fp64, true residual verified at the end.  All products and sums are evaluated
                            in fp64 in every mode; rtol always refers to the true fp64 residual in modes 1 and 2 */
  int32_t restart_every; /* > 0: every restart_every-th iteration rebuilds the search direction as the reference's CG does
                            (conjugate_gradient_solver.py:96-97; solve_DDM passes 500000).  Jacobi / DDM paths */
  double alpha_max;      /* > 0: clamp the CG step like conjugate_gradient_solver.py:79 (DDM solves use 100) */
  /* Multi-GPU only: bounding box and node count of the WHOLE lattice, so that every rank cuts the same brick /
   * aggregate grid (all zero -> derived from this handle's own nodes). */
  double grid_lo[3];
  double grid_hi[3];
  int64_t grid_nodes;
  double mintol;         /* > 0: also stop (converged, pl_stats_t.stop_reason = 1) when ||p|| < mintol (||x|| + 1e-12), the
                            reference's "direction norm" test (conjugate_gradient_solver.py:102-105; solve_DDM passes
                            1e-12), and report info = 2 when a step length fell below 1e-6 (:107-109).  These tests need
                            the host to see every iteration: use check_every = 1.  Jacobi / DDM paths */
  int32_t compact_records; /* LDS-tile K*p without a palette (graded / optimised lattices): 0 or 1 = stream 40-byte records
                              (the 5 stiffness scalars; the strut vector is recomputed from the node coordinates),
                              -1 = stream the 64-byte records */
  int32_t condense;      /* multi-level PCG (precond >= 2; fp64 and precision = 1; one or several GPUs - nodes shared with another
                            rank are never eliminated, and either every rank eliminates or none does): exact elimination of an independent set of nodes (no
                            two share a strut, none carries a Dirichlet dof; chosen at pl_create, interior nodes first)
                            inside the solver - CG runs on the Schur complement of the other nodes, the vector kernels skip
                            the eliminated rows, every iteration pays a second K*p, x still receives every node.
                            0 = automatic: when >= 45 % of the nodes can go (bipartite node graphs such as BCC: 793 -> 503
                            iterations and 275 -> 228 ms at 100^3), 1 = whenever candidates exist, -1 = never */
  int32_t chol_persistent; /* 1: factor the dense coarse operator in ONE persistent launch with a grid barrier per block
                              column instead of one launch per block column.  Measured slower (2.94 vs 2.86 ms per
                              assembly at 50^3 Octet): the release / acquire fences of a barrier across the 8 XCDs cost
                              what the kernel boundary costs - kept as an experiment switch */
  int32_t cg_form;       /* multi-level PCG (precond 2 / 3, fp64, no node elimination): 1 = single-reduction form (Chronopoulos-
                          * Gear recurrences, the dense level's residual carried by recurrence): ONE all-reduce per iteration on
                          * several GPUs instead of three exchanges, for three more stored vectors.  0 = ordinary form. */
  int32_t tile_modes;    /* tile level of the multi-level PCG: 0 / 12 = rigid-body + uniform-strain modes per tile (12 x 12 blocks;
                          * both CG forms, one or several GPUs), 6 = rigid-body modes only */
  int32_t coarse_modes;  /* dense level of the multi-level PCG: 0 = automatic (12 from 250 k nodes of the whole lattice), 12 =
                          * rigid-body + uniform-strain modes per aggregate (needs tile_modes = 12; fewer, larger aggregates),
                          * 6 = rigid-body modes */
  int32_t overlap;       /* multi-GPU handles with the neighbour exchange (pl_dist_set_peers), LDS-tile K*p: 0 / 1 = the tiles
                          * that own interface rows run first and their rows travel (pack, send / recv, add) on a second
                          * stream while the interior tiles run, -1 = one launch, then the exchange */
  int32_t coarse_storage; /* storage of the dense level's inverse factor W (the two triangular GEMVs of every iteration read it):
                           * 32 = fp32, 16 = bfloat16 (half the bytes; W16^T W16 is still symmetric positive definite and
                           * fixed - measured iteration counts unchanged), 0 = automatic: bfloat16 from 1 024 dofs on (round 4; from
                           * 3 072 until then: 100^3 BCC 2 x 22 us of a 354-us iteration; at 1 536 dofs the GEMVs are
                           * latency-bound and the step gains 1 - 2 %, iteration counts of five lattice types unchanged) */
  int32_t warm_start;    /* design loops (LatticeOpti.objective / gradient call the solver over and over on a slowly changing
                          * lattice, lattice_opti.py:569-570): 1 = pl_solve starts from the previous CONVERGED solution of this
                          * handle instead of from zero (one extra K*x; the stopping test is unchanged: ||r|| <= rtol ||b|| of the
                          * current right-hand side).  Multi-level PCG in fp64, ordinary form, single-GPU handles; ignored
                          * elsewhere.  0 = every solve starts from zero (what bench.py times on configs[1] / [2] / [4]: a loop of
                          * IDENTICAL solves must not start from its own answer).  2 (round 5) = start from 2 x_prev - x_prev2,
                          * the linear extrapolation of the handle's last two solutions - a design loop moves along a smooth path
                          * (configs[3]: 249 -> 208 iterations per solve on average); 3 = quadratic extrapolation of the last three
                          * (193; amplifies a jagged path threefold - opt-in); 4 = the GALERKIN start: x0 = the combination of the
                          * handle's last six solutions (environment PL_WARM_VECTORS, 2 ... 8) that is nearest to the solution of the
                          * CURRENT system in its energy norm, (V^T K V) c = V^T b - one operator application and a handful of dot
                          * products per stored vector, one 6 x 6 solve on the host.  A projection: it contains the candidates of 1, 2
                          * and 3 and can do no worse than any of them (configs[3]: 160 iterations per solve).  With the fp32 inner
                          * solver (precision = 1) 2, 3 and 4 act as 1. */
  int32_t short_iteration; /* small lattices (few K*p tiles: the dense level's explicit inverse can be read once per tile and
                          * iteration): 1 = the SHORT form of the multi-level PCG iteration (pl_small.h) - the dense level's
                          * solve and the prolongation fused into one launch that writes z = M^-1 r and r.z, the search
                          * direction p = z + beta p formed inside the next K*p launch: 3 dependent launches per iteration
                          * instead of 5 (4 instead of 6 under node elimination); 0 = automatic (on where it applies: fp64,
                          * ordinary CG form, single-GPU handle, n_tiles x modes x dense dofs small), -1 = never;
                          * 2 = EXPERIMENTAL: the whole loop as ONE persistent launch (pl_persist.h: single-reduction CG without
                          * node elimination, one workgroup per tile, hand-offs through write-through stores and flags; at most
                          * 256 tiles of <= 512 nodes, dense level <= 2 048 dofs) - measured slower than 1, kept for
                          * the record; pl_stats_t.short_iteration_used = 2.
                          * pl_stats_t.short_iteration_used says what ran */
} pl_opts_t;

typedef struct {
  uint32_t struct_size;    /* IN: sizeof(pl_stats_t) as the caller sees it (pl_solve returns PL_ERR_ARG on any other value) */
  int32_t iterations;
  int32_t converged;       /* 1 if ||r|| <= rtol*||b|| */
  int32_t reserved_i;
  double rel_residual;     /* ||r||/||b|| of the recurrence at exit */
  double b_norm;
  double ms_assembly;      /* last pl_assemble (+ pl_assemble_bsr) on the device, HIP events */
  double ms_solve;         /* last pl_solve, HIP events around the PCG loop */
  double ms_spmv_avg;      /* average K*x kernel time inside the last pl_solve (HIP events, sampled) */
  double precond_used;     /* preconditioner the solve actually ran with (opts->precond numbering): differs from the
                              request when a dense level was not positive definite and the solve fell back to Jacobi */
  double restarts;         /* precision = 1 / 2: inner solves taken (each ends with a true-residual evaluation) */
  double precision_used;   /* precision mode the solve ran in (0 when the request did not apply) */
  double info;             /* the reference CG's return code (conjugate_gradient_solver.py:75,99-109): 0 converged,
                              1 not converged, 2 not converged and a step length fell below 1e-6 */
  double stop_reason;      /* which test ended a converged solve: 0 ||r|| <= rtol ||b||, 1 direction norm (mintol) */
  double condensed_nodes;  /* nodes eliminated exactly inside the solve (opts.condense) */
  double cg_form_used;     /* 1: the solve ran in the single-reduction form (opts.cg_form) */
  double kp_form;          /* which K*p the solve applied: 1 = LDS-resident tile kernel with the record palette (k_spmv_tile_lds),
                              2 = LDS-resident tile kernel streaming 40-byte records (k_spmv_tile_lds_t), 3 = tile kernel gathering
                              from global memory (k_spmv_tile), 4 = row form (k_spmv_rows), 5 = per-node gather, 6 = global
                              atomics, 7 = DDM cell product */
  double comm_world;       /* multi-GPU handles: ranks of the communicator as the COMMUNICATOR reports them (ncclCommCount, or
                              the loopback group's size) - not what the launcher's environment says; 0 on a single-GPU handle */
  double comm_rank;        /* this handle's rank in it (ncclCommUserRank) */
  double short_iteration_used;  /* 1: the solve ran the short form of the iteration (opts.short_iteration) */
  double reserved[2];
} pl_stats_t;

/* Fills *o with the defaults.  struct_size = sizeof(pl_opts_t) of the caller's header; PL_ERR_ARG (and *o untouched)
 * when it differs from the library's. */
int pl_default_opts(pl_opts_t *o, uint32_t struct_size);
uint32_t pl_opts_size(void);
uint32_t pl_stats_size(void);
uint32_t pl_abi_version(void);
const char *pl_last_error(void);
const char *pl_version(void);

/* Joint-penalisation length L_zone at both ends of every strut of a NON-periodic lattice, lzone[2*b + end] (end 0 =
 * beam_conn[2b]): over the other struts meeting at that node, the largest r_other / tan(angle / 2); 1e-7 where the
 * angle exceeds 170 degrees, 0 where no other strut meets the node.  Replaces the per-node double loop of
 * Lattice.define_angles_between_beams (lattice.py:871-904) with Beam.get_angle_between_beams (beam.py:204-277) and
 * function_penalization_Lzone (utils.py:432-453).  Stand-alone (no handle): the result decides seg_len / seg_nsub of
 * pl_mesh_t.  Periodic single cells (Schur datasets) keep the host restatement. */
int pl_lzone(int device, int64_t n_nodes, int64_t n_beams, const double *node_xyz, const int32_t *beam_conn,
             const double *beam_radius, double *lzone);

/* Upload topology + geometry; builds the node->strut incidence.  Replaces BeamModel.__init__ /
 * latticeGeneration (beam_model.py:57-105, lattice_generation.py:64-175). */
int pl_create(const pl_mesh_t *mesh, const pl_opts_t *opts, pl_handle *out);
void pl_destroy(pl_handle h);

/* Domain-decomposition operator (LatticeSim.solve_DDM, lattice_sim.py:1111-1252): unknowns are the n_nodes
 * cell-boundary nodes; every cell c couples its nb boundary nodes cell_nodes[c*nb..] (order of
 * Cell.define_node_order_to_simulate, cell.py:611-680) through the dense Schur complement S[cell_S[c]] ((6nb)^2,
 * row-major).  The handle then serves pl_set_bc / pl_assemble / pl_spmv / pl_spmv_free / pl_solve / pl_reactions with
 * K := sum_c B_c^T S_c B_c; pl_solve runs plain CG (opts->precond = 0, as the reference's default), Jacobi-CG
 * (opts->precond = 1), CG preconditioned by the factorised assembled matrix (opts->precond = 2, below), by the inverted
 * 6 x 6 node blocks of the assembled matrix (opts->precond = 3: any size; built by pl_assemble for the current Dirichlet
 * mask from the same matrices as precond = 2) or by the node blocks plus a dense level on aggregates of nodes
 * (opts->precond = 4, pl_ddm_set_geometry below), with opts->alpha_max. */
int pl_create_ddm(int64_t n_nodes, int64_t n_cells, int32_t nb, const int32_t *cell_nodes, int32_t n_S, const double *S,
                  const int32_t *cell_S, const pl_opts_t *opts, pl_handle *out);

/* The reference's preconditioner of the DDM solve (LatticeSim.define_preconditioner / build_preconditioner,
 * lattice_sim.py:1333-1415; Cell.build_coupling_operator / build_local_preconditioner, cell.py:754-827):
 * G = sum_c B_c^T Shat_c B_c on the free dofs, factorised once (SuperLU there; dense Cholesky + explicit inverse
 * factor on the device here, so 6 n_nodes <= PL_DDM_DENSE_MAX), z = G^-1 r per iteration.  Selected by
 * opts->precond = 2 at pl_create_ddm; pl_assemble builds and factorises G for the current Dirichlet mask.
 * Shat_c defaults to the operator's own matrices (preconditioner_type "exact": CG converges in one step); this call
 * installs another palette - one mean matrix ("mean"), or the dataset matrices with the nearest-radius index per
 * cell ("nearest_reference").  pl_set_bc on an assembled precond = 2 handle invalidates the factorisation (it
 * depends on the Dirichlet mask): call pl_assemble again before pl_solve.  S = NULL goes back to the default.  When G is not positive definite (an indefinite
 * surrogate matrix) pl_assemble falls back to Jacobi (the reference: LU -> ILU) and pl_stats_t.precond_used says 1. */
#define PL_DDM_DENSE_MAX 16384
int pl_ddm_set_preconditioner(pl_handle h, int32_t n_S, const double *S /*[n_S][6nb][6nb]*/,
                              const int32_t *cell_S /*[n_cells]*/);

/* New cell matrices on an existing DDM handle (round 5): a design loop changes every S_c between two solves
 * (LatticeOpti.set_optimization_parameters -> reset_cell_with_new_radii, lattice_opti.py:467-560, lattice_sim.py:1421-1497) while
 * the cells keep their nodes.  S / cell_S as in pl_create_ddm (same nb; n_S may differ).  The handle's preconditioner data is
 * dropped: pl_assemble before the next pl_solve.  A palette installed by pl_ddm_set_preconditioner stays. */
int pl_ddm_update_matrices(pl_handle h, int32_t n_S, const double *S /*[n_S][6nb][6nb]*/, const int32_t *cell_S /*[n_cells]*/);

/* Beyond PL_DDM_DENSE_MAX dofs (round 5): opts->precond = 4 on a DDM handle = the node blocks of precond = 3 plus a dense
 * level, M^-1 = B^-1 + Z A_c^-1 Z^T with A_c = Z^T P G P Z - twelve modes (six rigid-body motions, six uniform strains) per
 * aggregate of boundary nodes, aggregates = boxes of a regular grid over the nodes' bounding box, as many as
 * opts->coarse_max_dofs / 12 allows (0: 1 536 dofs).  It stands where the reference factorises the assembled matrix
 * (build_preconditioner, lattice_sim.py:1351-1415): not a direct solve, but an iteration count that no longer grows with the
 * lattice (32^3 BCC cells: 2.2 x fewer iterations than the node blocks).  The modes need the node positions, which
 * pl_create_ddm does not take: this call hands them over (before pl_assemble; calling it again re-cuts the aggregates).
 * pl_assemble builds the node blocks, A_c from the cell matrices (the palette of pl_ddm_set_preconditioner if one is set)
 * and its Cholesky / inverse factor; when A_c is not positive definite the node blocks alone are used and
 * pl_stats_t.precond_used says 3. */
int pl_ddm_set_geometry(pl_handle h, const double *node_xyz /*[3 n_nodes]*/);

/* Dirichlet / load data per dof.  fixed[6N] (0/1), ubar[6N] prescribed values (read where fixed), f[6N] nodal
 * loads.  Replaces apply_displacement_all_nodes_with_lattice_data / apply_force_on_all_nodes_with_lattice_data
 * (full_scale_lattice_simulation.py:39-73,124-153).  Any of ubar/f may be NULL (= zeros). */
int pl_set_bc(pl_handle h, const uint8_t *fixed, const double *ubar, const double *f);

/* Periodic constraints for one-cell homogenisation (HomogenizedCell.periodic_boundary_condition,
 * homogenization_cell.py:210-252: dolfinx_mpc ties all six dofs of opposite corner / edge / face nodes): master[i] = the node
 * whose dofs node i shares (master[master[i]] == master[i]; i itself for an unconstrained node).  pl_solve then solves
 * P^T K P v = P^T f, u = P v, as CG on Q K Q with Q the orthogonal projector "average over each group" - f must be periodic
 * (the caller averages it over the groups) and the Dirichlet flags equal on all members of a group.  Jacobi PCG of a
 * single-GPU handle (opts.precond = 1).  master = NULL: no constraints. */
int pl_set_periodic(pl_handle h, const int32_t *master /*[n_nodes] or NULL*/);

/* New radii, same topology/segment geometry (optimisation loop; Cell.change_beam_radius cell.py:896-917). */
int pl_update_radii(pl_handle h, const double *beam_radius);
/* Per-strut multiplicity: strut b stands for beam_mult[b] identical struts in parallel between its two nodes (its record,
 * sensitivity and energy scale with it; the back-substitution of pl_node_mod gives every copy its share of the section
 * force).  This is what the reference's own model is on lattices whose struts lie in cell faces or on cell edges (Octet,
 * Cubic, Kelvin ...): LatticeSim.set_penalized_beams splits a strut shared by k cells once PER CELL and keeps every copy
 * (lattice_sim.py:250-303; Beam hashes by identity, beam.py:78-82; the mesher de-duplicates by object,
 * lattice_generation.py:152-160), and Lattice.check_hybrid_collision does the same to struts cut by another geometry's
 * node (lattice.py:1111-1215).  NULL = 1 everywhere (the default).  The next pl_assemble picks it up. */
int pl_set_multiplicity(pl_handle h, const double *beam_mult /*[n_beams] > 0, or NULL*/);
/* New penalised-segment geometry (when the caller re-runs the angle search, lattice_sim.py:1421-1497). */
int pl_update_segments(pl_handle h, const double *seg_len, const int32_t *seg_nsub);

/* Per-strut stiffness build ("assembly" of the matrix-free operator): condensed element records + the
 * preconditioner.  Replaces Material.compute_mechanical_properties + the FFCx element kernel
 * (material_definition.py:142-156, simulation_base.py:220-225).
 * Once pl_assemble_bsr has been called on the handle, pl_assemble also refreshes that explicit matrix (same with_bc):
 * the fill runs on a second stream next to the factorisation of the coarse operator.  Collective on a multi-GPU
 * handle (pl_dist_init): every rank must call it. */
int pl_assemble(pl_handle h);

/* Explicit global K as BSR(6x6) on the device (dolfinx assemble_matrix, simulation_base.py:473-476).
 * with_bc != 0 applies dolfinx's Dirichlet treatment (constrained rows/cols zeroed, unit diagonal). */
int pl_assemble_bsr(pl_handle h, int with_bc, int64_t *n_block_rows, int64_t *n_blocks);
int pl_get_bsr(pl_handle h, int64_t *rowptr /*[N+1]*/, int32_t *colidx /*[nblk]*/, double *vals /*[36*nblk]*/);

/* y = K x with the full (unconstrained) operator; test hook and building block of reactions. */
int pl_spmv(pl_handle h, const double *x, double *y);
/* y = P K P x with P the projector on free dofs (the PCG operator). */
int pl_spmv_free(pl_handle h, const double *x, double *y);
/* y = BSR * x using the explicitly assembled matrix (cross-check of the two paths). */
int pl_spmv_bsr(pl_handle h, const double *x, double *y);

/* Solve K u = f with the Dirichlet data of pl_set_bc by Jacobi-PCG on the matrix-free operator.
 * Replaces the PETSc KSP(preonly)+PC(LU) solve of simulation_base.py:501-511.  u[6N] gets the full field
 * (prescribed values on constrained dofs; u == NULL keeps it on the device only).  rtol is on ||r||/||b||. */
int pl_solve(pl_handle h, double rtol, int32_t max_iter, double *u, pl_stats_t *stats);

/* R = K u on every dof (caller keeps the constrained ones).  Replaces
 * calculate_reaction_force_and_moment_at_position (simulation_base.py:582-645). */
int pl_reactions(pl_handle h, const double *u, double *R);

/* Per-strut sensitivity s_b = lam_e^T (dK_e/dr_b) u_e at fixed segment geometry (lam == NULL -> lam = u; u == NULL -> the
 * solution of the last pl_solve of this handle, which is still on the device: a design loop need not upload it again).
 * Replaces the dS/dr contraction of LatticeOpti.calculate_gradient (lattice_opti.py:746-902) and the dormant
 * Material.compute_gradient (material_definition.py:163-231). */
int pl_sens(pl_handle h, const double *u, const double *lam, double *dCdr);

/* The same contraction for every pair of several fields in one pass (csrc/pl_sensgram.h): the strut's
 * dK_e/dr record - the expensive part of pl_sens - is built once per strut instead of once per pair.  A building block
 * beside pl_sens and pl_spmv_multi: the diagonal holds the compliance sensitivities of n_rhs load cases, an off-diagonal
 * entry a state x adjoint pair, and with the six total fields of a periodic homogenisation the whole Gram is the radius
 * derivative of the homogenised stiffness (u_k^T K u_l = scale_k H[k][l], no adjoint solve). */
#define PL_SENS_GRAM_MAX 8
/* gram[p][b] = x_k,e^T (dK_e/dr_b) x_l,e at fixed segment geometry for every pair k <= l < n_rhs,
 * p = k*n_rhs - k*(k-1)/2 + (l - k)  (rows of the upper triangle, row-major); x: [n_rhs][6N] host, gram: [n_rhs(n_rhs+1)/2][B]
 * host, caller's strut numbering.  Same dK_e/dr as pl_sens (radius, segments, multiplicity, material of the handle).
 * Single-GPU FEM handles (PL_ERR_STATE on pl_create_ddm / pl_dist_init handles); n_rhs < 1 or > PL_SENS_GRAM_MAX, NULL: PL_ERR_ARG.
 * Purely per strut: Dirichlet data and periodic constraints of the handle do not enter.  Leaves the handle's solver state untouched. */
int pl_sens_gram(pl_handle h, int32_t n_rhs, const double *x, double *gram);

/* Displacements of the penalisation points ("node_mod" points: the junctions between the penalised end segments and the
 * middle segment of every strut, LatticeSim.set_penalized_beams lattice_sim.py:245-308, which the reference meshes as
 * FE vertices and reads back in set_result_diplacement_on_lattice_object, full_scale_lattice_simulation.py:77-107).
 * They are interior points of the condensed strut: recovered in closed form from the end displacements u[6N].
 * out[12*b ..] = [u(q1)(3) th(q1)(3) u(q2)(3) th(q2)(3)], q1 next to beam_conn[2b], q2 next to beam_conn[2b+1]; an absent
 * segment gives the end node's own values. */
int pl_node_mod(pl_handle h, const double *u, double *out);

/* ---- strut section forces, von Mises stress and its p-norm aggregate (round 9) ---------------------------------------------
 * Replaces generalized_stress = C eps (simulation_base.py:116-125), calculate_forces / calculate_moments and
 * extract_stress_field (simulation_base.py:776-806), which prints the maximum.  Single-GPU FEM handles after pl_assemble
 * (PL_ERR_STATE on pl_create_ddm / pl_dist_init handles and before assembly).  u[6N]; NULL = the solution of the last
 * pl_solve of this handle, still on the device (as pl_sens).  All outputs in the caller's strut and node numbering.
 *
 * A strut carries no span load: the axial force N = F.t, the shear force V = |F - N t| and the torque T = M.t are constant
 * along it, the bending moment Mb(s) = |M(s) - T t| is the norm of a linear function of the arclength and peaks at a
 * segment end.  Stations per strut, in the direction beam_conn[2b] -> beam_conn[2b+1], laid out [A, q1, q2, B]:
 *   where = 0: A = end beam_conn[2b] (radius of the first present segment of seg_len), q1 / q2 = the junctions behind the
 *              penalised segment at point1 / in front of the one at point2 (radius: the smaller of the two adjacent segments',
 *              i.e. r), B = end beam_conn[2b+1] (radius of the last present segment).  A junction whose segment is absent
 *              is absent.  Penalised segments have radius pen_coef * r, the middle one r.
 *   where = 1: slots 1 and 2 = the two ends of the MIDDLE segment, both with radius r (the penalised joint zones are a
 *              stiffness device, not a place to read stresses); slots 0 and 3 absent; no station on a strut without a middle
 *              segment.
 * An absent station is NaN in `station` and contributes to no sum.  Circular section of radius R (S = pi R^2, I = pi R^4 / 4,
 * J = 2 I):  sigma = |N| / S + Mb R / I,  tau = |T| R / J,  sigma_vm = sqrt(sigma^2 + 3 tau^2); V is reported but does not
 * enter (the transverse shear stress vanishes at the fibre where bending peaks).
 * Multiplicity (pl_set_multiplicity): the record's force is shared by its k parallel copies - N, V, T, Mb and the stresses are
 * those of ONE copy (F / k, M / k), and a copy counts once in the aggregate below, not k times.
 * PL_ERR_ARG: where not 0 / 1, every output pointer NULL. */
int pl_stress(pl_handle h, const double *u /*[6N] or NULL*/, int32_t where,
              double *station /*[B][4][5] = N, V, T, Mb, sigma_vm per station, or NULL*/,
              double *peak /*[B] max sigma_vm over the strut's stations (0 if none), or NULL*/);
/* Phi_p = (sum over the present stations of sigma_vm^p)^(1/p), p >= 1 (PL_ERR_ARG below 1): an upper bound of
 * sigma_max = max sigma_vm that tends to it with p; evaluated as sigma_max (sum (sigma_vm / sigma_max)^p)^(1/p), so no power
 * overflows; Phi = 0 and zero derivatives when sigma_max = 0.  dphi_du[6N] = dPhi/du at fixed radii, dphi_dr[B] = dPhi/dr_b at
 * fixed u and segment geometry - through the strut record AND through the section constants S, I, J (R = r or pen_coef r).
 * Derivatives of |N|, |T|, Mb at exactly zero are taken as zero.  Both reductions run in two stages in a fixed order and
 * dphi_du is gathered per node without atomics: two calls with the same inputs return the same bits in every output.
 * Any output may be NULL, not all. */
int pl_stress_pnorm(pl_handle h, const double *u /*[6N] or NULL*/, int32_t where, double p, double *phi, double *sigma_max,
                    double *dphi_du /*[6N] or NULL*/, double *dphi_dr /*[B] or NULL*/);

/* ---- Euler buckling utilisation of the struts and its p-norm aggregate (round 10) -------------------------------------------
 * The other way a slender strut fails.  Same handles, same u (NULL = last pl_solve) and same numbering rules as pl_stress.
 * Per strut b: N = F.t / k, the signed axial force of ONE copy (tension > 0) - exactly the N of pl_stress, k the multiplicity
 * of pl_set_multiplicity; compressive force P = max(0, -N).
 * Buckling length l:  length = 0: the node-to-node length |d|;  length = 1: the middle segment seg_len[3b+1] (the penalised
 * joint zones are rigid ends, the view where = 1 takes for stresses) - a strut without a middle segment is then absent: NaN in
 * util, n_axial and n_crit, and it enters no sum.
 * Critical load with the un-penalised radius r, I = pi r^4 / 4, S = pi r^2:  N_E = pi^2 E I / (k_eff l)^2 (k_eff = 1
 * pinned-pinned, 0.5 clamped-clamped);  shear = 0: N_cr = N_E;  shear = 1: the Engesser load of a Timoshenko column,
 * N_cr = N_E / (1 + N_E / (kappa G S)), G = E / (2 (1 + nu)); E, nu, kappa of the handle.
 * Utilisation util = beta = P / N_cr >= 0: buckling is predicted at beta >= 1; a strut in tension has beta = 0 exactly.
 * PL_ERR_ARG: length not 0 / 1, shear not 0 / 1, k_eff <= 0 or not finite, every output pointer NULL. */
int pl_buckling(pl_handle h, const double *u /*[6N] or NULL*/, int32_t length, double k_eff, int32_t shear,
                double *util /*[B] or NULL*/, double *n_axial /*[B] signed, one copy, or NULL*/, double *n_crit /*[B] or NULL*/);
/* B_p = (sum over the present struts of beta^p)^(1/p), p >= 1 (PL_ERR_ARG below 1), evaluated as
 * beta_max (sum (beta / beta_max)^p)^(1/p) so that no power overflows; util_max = beta_max; B_p = 0 and zero derivatives when
 * beta_max = 0; the derivative of max(0, -N) at N = 0 is taken as zero.  dbp_du[6N] = dB/du at fixed radii, dbp_dr[B] = dB/dr_b
 * at fixed u and segment geometry - through the strut record AND through N_cr(r).  Two-stage reductions in a fixed order and a
 * per-node gather without atomics: two calls with the same inputs return the same bits in every output.
 * Any output may be NULL, not all. */
int pl_buckling_pnorm(pl_handle h, const double *u /*[6N] or NULL*/, int32_t length, double k_eff, int32_t shear, double p,
                      double *bp, double *util_max, double *dbp_du /*[6N] or NULL*/, double *dbp_dr /*[B] or NULL*/);

/* ---- thermal loads: strut expansion forces, thermal stress and buckling, gradients -------------------------------------------
 * The temperature rise is GIVEN per node (no heat conduction here), linear along a strut between its end values and uniform
 * over the section (no thermal curvature).  Strut b = (A, B), d = x_B - x_A, L = |d|, t = d / L, expansion coefficient alpha_b:
 *   free elongation     delta_b = alpha_b L (dT_A + dT_B) / 2    (no radius and no penalised segment enters)
 *   restrained force    F_th,b = ka_b delta_b, ka_b = rec.a + rec.e1 L^2 the condensed axial stiffness of the record
 *                       (multiplicity k of pl_set_multiplicity included); n_free_b = F_th,b / k is that of ONE copy
 *   equivalent loads    f_th: +F_th t on the translations of B, -F_th t on those of A, no moments.  Equilibrium under a thermal
 *                       load is K u = f_ext + f_th: the caller adds f_th to the f of pl_set_bc.
 * While a thermal state is set, pl_stress, pl_stress_pnorm, pl_buckling and pl_buckling_pnorm evaluate the MECHANICAL section
 * force F = K_tip (du, dth) - F_th t: N = (F.t - F_th) / k, while V, T, Mb are unchanged; dphi_du / dbp_du keep their form and
 * dphi_dr / dbp_dr gain g_F . (-(2 ka / r) delta t) (d ka / dr = 2 ka / r at fixed segment geometry).  Without a thermal state
 * these calls run the kernels and the arithmetic they ran before.  pl_buckling_modes, pl_buckling_modes_sens and
 * pl_geom_spmv_multi build K_g from K_e u_e, which would ignore the thermal prestress: PL_ERR_STATE while a thermal state is set.
 * pl_energy, pl_reactions, pl_node_mod, pl_sens and the dynamic calls do not read the thermal state.
 *
 * alpha_b = beam_alpha ? beam_alpha[b] : alpha; node_dT[N] in the caller's node numbering; node_dT == NULL clears the
 * thermal state of the handle.  Non-finite values: PL_ERR_ARG.  Single-GPU FEM handles only (PL_ERR_STATE on
 * pl_create_ddm / pl_dist_init handles, as pl_set_mass).  Survives pl_update_radii / pl_update_segments / pl_assemble. */
int pl_set_thermal(pl_handle h, double alpha, const double *beam_alpha /*[B] or NULL*/, const double *node_dT /*[N] or NULL*/);
/* f_th[6N] (caller's numbering) and/or n_free[B] = restrained force of ONE copy, from the records of the last pl_assemble.
 * f_th is gathered per node without atomics: two calls return the same bits.
 * PL_ERR_STATE before pl_set_thermal or before assembly; both outputs NULL: PL_ERR_ARG. */
int pl_thermal_load(pl_handle h, double *f /*[6N] or NULL*/, double *n_free /*[B] or NULL*/);
/* out[b] = lam^T d f_th / d r_b = (2 ka_b / r_b) delta_b t . (lam_u,B - lam_u,A) at fixed segment geometry; lam == NULL -> the
 * solution of the last pl_solve (as pl_sens).  For a scalar q(u(r), r) with K lam = dq/du on the free dofs,
 * dq/dr_b = dq/dr_b at fixed u - lam^T (dK/dr_b) u + lam^T d f_th / d r_b.  Errors as pl_thermal_load; out == NULL: PL_ERR_ARG. */
int pl_thermal_sens(pl_handle h, const double *lam /*[6N] or NULL*/, double *out /*[B]*/);

/* ---- steady heat conduction on the strut graph: temperatures, strut heat flows, the thermo-elastic adjoint chain ----------------
 * Each strut is ONE two-node conductor between its lattice nodes (the convention of K_g and M): a uniform circular section of
 * the plain radius r over the node-to-node length L = |d|; penalised end zones and the overlap at the joints are ignored, a
 * multiplicity k of pl_set_multiplicity counts k times.
 *   conductance   g_b = k_b kappa_b pi r_b^2 / L_b,  kappa_b = beam_kappa ? beam_kappa[b] : kappa;  d g_b / d r_b = 2 g_b / r_b
 *   operator      (K_T T)_i = sum over struts b at i of g_b (T_i - T_other)
 *   problem       K_T T = q on the free nodes (q the nodal heat inflow), T = T_bar on the nodes of a mask of one byte per node,
 *                 which is independent of the mechanical mask of pl_set_bc
 *   heat flow     Q_b = g_b (T_A - T_B) / k_b of ONE copy of strut b from A to B
 * Coupling to the thermal loads: the solved T minus a reference temperature is the node_dT of pl_set_thermal.  For a mechanical
 * field lam the transpose of d f_th / d dT is c_i = sum over struts b at i of (1/2) alpha_b L_b ka_b t_b . (lam_u,B - lam_u,A)
 * (pl_thermal_load_adjoint).  With K_T mu = c on the free thermal nodes and mu = 0 on the others, a scalar q(u(T(r), r), r)
 * with K lam = dq/du gains dq/dr_b += - mu^T (dK_T/dr_b) T = - (2 g_b / r_b) (mu_A - mu_B) (T_A - T_B) (pl_cond_sens gives the
 * product without the sign), for heat inflows and T_bar that do not depend on r.
 *
 * All calls: the caller's node and strut numbering; single-GPU FEM handles only (PL_ERR_STATE on pl_create_ddm / pl_dist_init
 * handles); PL_ERR_STATE before pl_set_conduction (the five below) and before pl_assemble; NULL where an array is required:
 * PL_ERR_ARG.  g is rebuilt from the current radii and records by every call, so the state follows pl_update_radii and
 * pl_assemble.  The handle's mechanical state (boundary conditions, last solution, warm start, statistics) is not touched.
 * The per-node and per-strut products have a fixed order of summation and no atomics: two calls return the same bits.  The
 * solve sums its scalar products with atomics and is NOT bitwise reproducible. */
/* kappa == 0 && !beam_kappa clears the state; non-positive or non-finite values: PL_ERR_ARG.  Survives pl_update_radii /
 * pl_update_segments / pl_assemble. */
int pl_set_conduction(pl_handle h, double kappa, const double *beam_kappa /*[B] or NULL*/);
/* y = K_T x; masked: y = P K_T P x for the mask `fixed` (P zeroes the fixed nodes; fixed may be NULL when masked == 0). */
int pl_cond_spmv(pl_handle h, int32_t masked, const uint8_t *fixed /*[N] or NULL*/, const double *x /*[N]*/, double *y /*[N]*/);
/* Jacobi-preconditioned CG from x0 = 0 on the free nodes, stopped on the device by ||r|| <= rtol ||b||, b = P (q - K_T T_bar).
 * T_bar == NULL: zeros (only its values on fixed nodes are read, and they come back bit-equal); q == NULL: no inflow (values
 * of q on fixed nodes are ignored).  A mask without a fixed node: PL_ERR_ARG.  stats as pl_solve_multi fills them.
 * PL_ERR_NOCONV when rtol is missed within max_iter (T and stats are still written). */
int pl_cond_solve(pl_handle h, const uint8_t *fixed /*[N]*/, const double *T_bar /*[N] or NULL*/, const double *q /*[N] or NULL*/,
                  double rtol, int32_t max_iter, double *T /*[N]*/, pl_stats_t *stats);
/* Q[b] = g_b (T_A - T_B) / k_b. */
int pl_cond_flux(pl_handle h, const double *T /*[N]*/, double *Q /*[B]*/);
/* out[b] = (2 g_b / r_b) (mu_A - mu_B) (T_A - T_B) = mu^T (dK_T / dr_b) T. */
int pl_cond_sens(pl_handle h, const double *T /*[N]*/, const double *mu /*[N]*/, double *out /*[B]*/);
/* out[i] = c_i above for the field lam.  Needs the alpha of a thermal state: PL_ERR_STATE before pl_set_thermal. */
int pl_thermal_load_adjoint(pl_handle h, const double *lam /*[6N]*/, double *out /*[N]*/);

/* ---- lumped strut-surface convection and thermal aggregates ---------------------------------------------
 * Every end of strut b exchanges heat with an ambient at T_inf through the film conductance
 *   c_b = k_b h_b pi r_b L_b   (half the lateral surface 2 pi r L of every copy times the film coefficient),  d c_b / d r_b = c_b / r_b,
 *   h_b = beam_film ? beam_film[b] : film.  With H_i = sum over struts b at i of c_b the operator becomes K_T + diag(H) and the
 * problem (K_T + H) T = q + H T_inf on the free nodes, T = T_bar on the masked ones.  The form is lumped: the operator stays
 * an M-matrix.  With a positive c_b on every connected component no Dirichlet node is needed.
 *   loss of one copy   Qc_b = c_b [(T_A - T_inf) + (T_B - T_inf)] / k_b,   dissipated power P = sum_b k_b Qc_b = sum_i H_i (T_i - T_inf)
 * Under a convection state pl_cond_spmv, pl_cond_solve and pl_cond_sens act on the convective problem: the product gains H x,
 * pl_cond_solve accepts a mask without a fixed node, and pl_cond_sens gains (c_b / r_b) [mu_A (T_A - T_inf) + mu_B (T_B - T_inf)].
 *
 * pl_set_convection needs a conduction state (PL_ERR_STATE) and lives in it: pl_set_conduction - setting, replacing or clearing -
 * drops it.  film == 0 and beam_film == NULL clears it.  PL_ERR_ARG: a negative or non-finite film, a non-finite T_inf, every
 * film zero.  The state survives pl_update_radii / pl_update_segments / pl_assemble; handle restrictions as pl_set_conduction. */
int pl_set_convection(pl_handle h, double film, const double *beam_film /*[B] or NULL*/, double T_inf);
/* The adjoint problem of a functional J(T): (K_T + H) mu = rhs on the free nodes, mu = 0 on the fixed ones - pl_cond_solve without
 * T_bar and without the ambient term H T_inf (without a convection state it equals pl_cond_solve(h, fixed, NULL, rhs, ...)). */
int pl_cond_solve_adjoint(pl_handle h, const uint8_t *fixed /*[N]*/, const double *rhs /*[N]*/, double rtol, int32_t max_iter,
                          double *mu /*[N]*/, pl_stats_t *stats);
/* Qc[b] above and total[0] = P, folded in two stages of a fixed order (equal inputs give equal bits).  Either may be NULL, not
 * both.  PL_ERR_STATE without a convection state. */
int pl_cond_film(pl_handle h, const double *T /*[N]*/, double *Qc /*[B] or NULL*/, double *total /*[1] or NULL*/);
/* Phi_p = (sum over the nodes of the set of max(T_i - T_ref, 0)^p)^(1/p), evaluated as v_max (sum (v / v_max)^p)^(1/p) in the
 * fixed-order stages of pl_stress_pnorm.  nodes: one byte per node, NULL = all; a NaN in T adds nothing.
 * out = (Phi_p, v_max, sum (v / v_max)^p), dphi_dT[i] = (v_i / v_max)^(p-1) (sum)^(1/p - 1) where v_i > 0, else 0.  Either
 * output may be NULL, not both.  p < 1 or non-finite: PL_ERR_ARG.  Needs an assembled single-GPU FEM handle, no conduction state. */
int pl_temp_pnorm(pl_handle h, const double *T /*[N]*/, const uint8_t *nodes /*[N] or NULL*/, double T_ref, double p,
                  double *out /*[3] or NULL*/, double *dphi_dT /*[N] or NULL*/);

/* ---- transient heat conduction: implicit theta steps on the strut graph ---------------------------------
 * Lumped heat capacity, conventions of the conductance (plain radius r, node-to-node length L, multiplicity k):
 *   C_i = sum over struts b at i of (1/2) k_b (rho c)_b pi r_b^2 L_b + node_capacity_i,  (rho c)_b = beam_rho_c ? beam_rho_c[b] : rho_c
 * (half of every copy's volume to each end times the volumetric heat capacity), rebuilt from the current radii by every call.
 *   problem   C dT/dt + (K_T + H) T = q(t) + H T_inf on the free nodes, T = T_bar(t) on the masked ones (H = 0 without convection)
 *   step      (C/dt + theta (K_T + H)) dT = q_theta + H T_inf - (K_T + H) W on the free rows, dT = T_{n+1} - T_n, 1/2 <= theta <= 1,
 *             W_j = T_n,j on a free node and (1 - theta) T_n,j + theta T_bar,n+1,j on a fixed one, q_theta = theta q_{n+1} + (1 - theta) q_n
 * The capacity matrix is diagonal on purpose: the step matrix is an M-matrix and backward Euler (theta = 1) cannot undershoot.
 * Every strut has rho c > 0, so the step matrix is positive definite for any mask, an all-zero mask without convection (an
 * insulated lattice) included.
 *
 * pl_set_heat_capacity needs a conduction state (PL_ERR_STATE) and lives in it, as pl_set_convection does: pl_set_conduction
 * drops it.  rho_c == 0 and beam_rho_c == NULL clears it.  PL_ERR_ARG: a non-positive or non-finite strut value, a negative or
 * non-finite node_capacity.  Survives pl_update_radii / pl_update_segments / pl_assemble; handle restrictions as pl_set_conduction. */
int pl_set_heat_capacity(pl_handle h, double rho_c, const double *beam_rho_c /*[B] or NULL*/, const double *node_capacity /*[N] >= 0 or NULL*/);
/* n_steps steps of size dt from the initial state T0 (NULL: T_inf everywhere, 0 without a convection state) with the fixed nodes
 * at their row-0 value.  Caller's node numbering throughout.
 *   loads      q_n = sum_p amp[n][p] pattern[p], n_pat <= 4 (values on fixed nodes are ignored)
 *   mask       fixed: one byte per node, NULL = no fixed node.  The prescribed temperature of row n on a fixed node i is
 *              T0_i + s_n (T_bar_i - T0_i), evaluated in this order without a fused multiply-add; s = bar_amp, NULL: s_n = 1.
 *              T_bar == NULL: zeros.
 *   probe      [n_steps + 1][n_probe]: the temperature of the probed nodes in every row
 *   heat       [n_steps + 1][4]: U_n = sum_i C_i (T_i - T_inf), the stored heat, and three cumulative heats that are zero in row 0:
 *              Q_in += dt sum_free q_theta,i;  Q_c += dt sum over ALL nodes of H_i (T_theta,i - T_inf);
 *              Q_R += dt sum_fixed [C_i dT_i/dt + ((K_T + H) T_theta)_i - H_i T_inf], the heat the prescribed nodes supply, with
 *              T_theta = T_n + theta dT.  U_n - U_0 = Q_in + Q_R - Q_c up to the PCG residuals.
 *   snaps      row k * snap_every lands in snaps[k - 1], k = 1 ... n_steps / snap_every
 *   state      the last row; a later call with T0 = state (and the same data) continues the history
 *   iters      PCG iterations of every step, iters[0] = 0
 * Every step is one Jacobi PCG solve from dT = 0 on the device, stopped by ||r|| <= rtol ||b||; a field at rest takes no
 * iteration.  The whole history stays on the device and comes down once at the end.
 * PL_ERR_ARG: dt <= 0, n_steps < 1, theta outside [1/2, 1], n_pat outside 0 ... 4, a probe index out of range, a non-positive
 * rtol or max_iter, a value of T0, T_bar, bar_amp, pattern or amp that is not finite.  PL_ERR_STATE: before pl_set_heat_capacity, before pl_assemble, on a pl_create_ddm or pl_dist_init handle.
 * PL_ERR_NOCONV names the step whose solve missed rtol; the outputs are then not written.  The handle's mechanical state is not
 * touched, and neither is steady conduction: pl_cond_solve before and after gives the same result.  Device memory: the probe
 * block and the snapshots are released when the call returns; its other buffers (a few arrays of N, the patterns and tables)
 * stay in the heat-capacity state at the largest size asked for so far, until that state is dropped. */
int pl_cond_transient(pl_handle h, int32_t n_steps, double dt, double theta, const uint8_t *fixed /*[N] or NULL*/,
                      const double *T_bar /*[N] or NULL*/, const double *bar_amp /*[n_steps+1] or NULL*/, int32_t n_pat,
                      const double *pattern /*[n_pat][N] or NULL*/, const double *amp /*[n_steps+1][n_pat]*/,
                      const double *T0 /*[N] or NULL*/, double rtol, int32_t max_iter, int32_t n_probe,
                      const int32_t *probe_nodes, double *probe /*[n_steps+1][n_probe]*/, double *heat /*[n_steps+1][4] or NULL*/,
                      int32_t snap_every, double *snaps /*[n_steps/snap_every][N] or NULL*/, double *state /*[N] or NULL*/,
                      int32_t *iters /*[n_steps+1] or NULL*/);

/* Strain energy 1/2 u^T K u (LatticeOpti.compute_compliance, lattice_opti.py:645-663 uses u^T K u). */
int pl_energy(pl_handle h, const double *u, double *energy);

/* Dense condensation of a node subset: S = K_BB - K_BI K_II^-1 K_IB for the boundary nodes listed, computed
 * column by column with the device PCG.  Replaces SchurComplement.calculate_schur_complement
 * (schur_complement.py:75-147).  S is [6*nb x 6*nb] row-major. */
int pl_schur(pl_handle h, const int32_t *boundary_nodes, int32_t nb, double rtol, int32_t max_iter, double *S);

/* ---- several right-hand sides on one operator, one Jacobi-PCG pass (round 8) -------------------------------------------
 * The reference factorises once and back-substitutes per column (PETSc LU: simulation_base.py:501-511,
 * schur_complement.py:75-147, homogenization_cell.py:256-331); here all columns iterate in lock step and every launch
 * carries all of them.  Single-GPU FEM handles (not pl_create_ddm, not pl_dist_init), fp64, Jacobi preconditioner, x0 = 0:
 * the handle's multi-level / dense preconditioner, node elimination and warm start are ignored, and its single-column state
 * (solution of the last pl_solve, warm-start history, statistics) is left untouched.  Periodic constraints of
 * pl_set_periodic are honoured.  A column that has converged, or whose p^T K p is not positive, is frozen while the
 * others go on.  n_rhs < 1 or > PL_MULTI_MAX is PL_ERR_ARG. */
#define PL_MULTI_MAX 64
/* y_j = K x_j (masked != 0: P K P x_j, x_j zeroed on fixed dofs first), j < n_rhs; x, y: [n_rhs][6N] host arrays. */
int pl_spmv_multi(pl_handle h, int32_t n_rhs, int masked, const double *x, double *y);
/* K u_j = f_j under the Dirichlet MASK of the last pl_set_bc, with per-column prescribed values ubar[n_rhs][6N]
 * (read where fixed; NULL = 0) and loads f[n_rhs][6N] (NULL = 0).  u[n_rhs][6N] gets the full fields.
 * stats: NULL or n_rhs entries, struct_size set by the caller in each; iterations / converged / rel_residual / b_norm
 * per column, ms_solve = the whole call.  PL_ERR_NOCONV when any column missed rtol (all outputs still written). */
int pl_solve_multi(pl_handle h, int32_t n_rhs, const double *ubar, const double *f, double rtol, int32_t max_iter,
                   double *u, pl_stats_t *stats);
/* pl_schur by column blocks: the unit boundary displacements are generated, solved (the loop of pl_solve_multi) and
 * contracted to S on the device, `block` columns at a time (0 = the library's choice, <= PL_MULTI_MAX); only S comes
 * back.  Same S, row order and meaning of rtol / max_iter as pl_schur.  The handle's boundary data (pl_set_bc) are not
 * touched: the boundary mask of the condensation lives in the call's own workspace. */
int pl_schur_block(pl_handle h, const int32_t *boundary_nodes, int32_t nb, double rtol, int32_t max_iter,
                   int32_t block, double *S);

/* ---- global linear buckling (csrc/pl_geom.h) --------------------------------------------------------
 * With u the equilibrium of the applied loads: the smallest lambda > 0 with (K + lambda K_g(u)) phi = 0, K_g the geometric
 * stiffness of the struts' axial forces in u - the load factor at which cells or the whole lattice buckle together, which the
 * per-strut check of pl_buckling does not see.  Limits: single-GPU FEM handles only (the cases of pl_spmv_multi).  K_g takes
 * each strut as ONE Hermite-cubic element between its two lattice nodes, loaded by the record's total axial force: penalised
 * end zones and sub-element counts do not enter, a strut buckling between its own two joints cannot be represented and is
 * over-estimated (pl_buckling covers that failure).  Linearised prebuckling only.  A spectrum dominated by tension
 * (|mu_min| >> mu_max, mu = 1 / lambda) converges slowly under the shift of the iteration; it stays correct, and max_outer
 * bounds it. */
/* y_j = K_g(u) x_j (masked != 0: P K_g P x_j), j < n_rhs <= PL_MULTI_MAX; u[6N] or NULL = solution of the last
 * pl_solve; x, y: [n_rhs][6N] host arrays.  Test hook and building block. */
int pl_geom_spmv_multi(pl_handle h, const double *u, int32_t n_rhs, int masked, const double *x, double *y);
/* The n_modes smallest POSITIVE load factors of (K + lambda K_g(u)) phi = 0 on the free dofs of the last pl_set_bc,
 * ascending, and their modes (0 on fixed dofs, phi_i^T K phi_j = delta_ij, largest component positive).
 * Shifted block subspace iteration on G phi = mu K phi, G = -K_g, with n_sub columns (a multiple of 4 in 4 ... 32; 0 =
 * max(8, 2 n_modes rounded up to a multiple of 4)), 1 <= n_modes <= n_sub / 2; every outer step solves its n_sub columns in
 * one Jacobi-PCG pass (rtol, max_iter as pl_solve_multi) and ends with a Rayleigh-Ritz step on products that are applied,
 * so the Ritz values are true Rayleigh quotients.  It stops when the n_modes largest Ritz values have changed by less than
 * tol relatively between two steps (values below 1e-10 of the largest magnitude count as zero).
 * Fewer than n_modes positive factors may exist (every strut in tension, u = 0): n_found says how many were found, the rest
 * of every output is NaN, and the call returns PL_OK.  PL_ERR_NOCONV when max_outer is reached (outputs still written).
 * PL_ERR_STATE in the cases of pl_spmv_multi, on a handle with pl_set_periodic constraints, before pl_set_bc, and for
 * u = NULL without a pl_solve; PL_ERR_ARG for bad sizes or null outputs.  The handle's single-column state (last solution,
 * warm-start history, statistics) is left untouched. */
int pl_buckling_modes(pl_handle h, const double *u /*[6N] or NULL*/, int32_t n_modes, int32_t n_sub,
                      double rtol, int32_t max_iter,      /* inner PCG, as pl_solve_multi */
                      double tol, int32_t max_outer,      /* outer: largest relative change of the wanted Ritz values */
                      double *load_factor /*[n_modes]*/, double *modes /*[n_modes][6N] or NULL*/,
                      double *residual /*[n_modes] or NULL: |K phi + lambda K_g phi| / |K phi|, free dofs*/,
                      int32_t *n_found, int32_t *outer_iterations);
/* Sensitivities of those load factors to the strut radii, at fixed segment geometry (the convention of pl_sens) and with u
 * following the radii through K u = f: for every eigenpair (load_factor[i], modes[i]) - any scaling, read with the fixed
 * dofs zeroed -, with kk = phi^T K phi, q_b = phi_e^T G_b phi_e (G_b the strut's geometric element matrix for N = 1),
 * ka = a + e1 L^2 and dK_e = dK_e/dr_b,
 *     w = d(phi^T K_g(u) phi)/du = sum_b q_b ka_b (-t_b at u_A, +t_b at u_B),   K nu = -w on the free dofs, nu = 0 elsewhere,
 *     dlambda/dr_b = (lambda / kk) [phi_e^T dK_e phi_e + lambda (q_b (dka_b/dr_b) t_b.(u_B - u_A) + nu_e^T dK_e u_e)].
 * The adjoint solves of all modes run in ONE Jacobi-PCG pass (rtol, max_iter as pl_solve_multi), so the rows are total
 * derivatives.  For an m-fold repeated factor the single rows are NOT derivatives (the modes are an arbitrary basis of the
 * eigenspace); their sum over the whole cluster is the derivative of the sum of those factors, and so is any combination with
 * equal weights inside the cluster - dsum_dr with such weights is what a design loop should use.
 * 1 <= n_modes <= 16.  A mode whose load_factor is NaN (what pl_buckling_modes writes beyond n_found) is skipped: its rows of
 * dlam_dr and adj_load are NaN and it adds nothing to dsum_dr.  dsum_dr needs weights.  Outputs in the caller's strut
 * numbering.  PL_ERR_ARG for bad sizes, null inputs and when all three outputs are NULL; PL_ERR_STATE in the cases of
 * pl_buckling_modes; PL_ERR_NOCONV when an adjoint column missed rtol (outputs still written).  The handle's single-column
 * state is left untouched. */
int pl_buckling_modes_sens(pl_handle h, const double *u /*[6N] or NULL = last pl_solve*/, int32_t n_modes,
                           const double *load_factor /*[n_modes]*/, const double *modes /*[n_modes][6N]*/,
                           double rtol, int32_t max_iter,            /* adjoint solve, as pl_solve_multi */
                           const double *weights /*[n_modes] or NULL*/,
                           double *dlam_dr  /*[n_modes][B] or NULL*/,
                           double *dsum_dr  /*[B] or NULL: sum_i weights[i] dlam_i/dr_b, formed on the device*/,
                           double *adj_load /*[n_modes][6N] or NULL: w_i, unmasked - test hook*/);

/* ---- natural frequencies (csrc/pl_mass.h) -----------------------------------------------------------
 * Free vibration K phi = omega^2 M phi on the free dofs of pl_set_bc, M the CONSISTENT mass of the struts: each strut is ONE
 * element between its two lattice nodes (the discretisation of K_g), a uniform circular section of its plain radius r over
 * the node-to-node length L - the textbook rho A L / 420 [[156, 22 L, 54, -13 L], ...] in both bending planes, the axial and
 * torsional blocks [[2, 1], [1, 2]] and, with rotary != 0, the Rayleigh rotary inertia of bending rho I / (30 L) [[36, 3 L, ...
 * Penalised end zones stiffen K only, strut overlap at the nodes is ignored, a multiplicity k counts k times.  Limits: those
 * of the buckling calls - a strut vibrating between its own joints is over-stiff, single-GPU FEM handles, the Jacobi inner
 * solve, clustered spectra need n_sub past the cluster.
 * All four calls: PL_ERR_STATE on DDM and multi-rank handles; the last three also before pl_set_mass, before pl_assemble and
 * with pl_set_periodic constraints.  The handle's single-column state is left untouched. */
/* Density (> 0), rotary inertia of bending on / off (1 / 0) and optional translational point masses node_mass[N] >= 0 (NULL:
 * none) in the caller's node numbering.  The strut masses follow the handle's current radii and multiplicities in every later
 * call without further notice.  PL_ERR_ARG for a density that is not positive and a negative node_mass. */
int pl_set_mass(pl_handle h, double density, int32_t rotary, const double *node_mass /*[N] >= 0 or NULL*/);
/* y_j = M x_j (masked != 0: P M P x_j, needs pl_set_bc), j < n_rhs <= PL_MULTI_MAX; x, y: [n_rhs][6N] host arrays. */
int pl_mass_spmv_multi(pl_handle h, int32_t n_rhs, int masked, const double *x, double *y);
/* The n_modes smallest omega^2, ascending, and their modes (0 on fixed dofs, phi_i^T M phi_j = delta_ij, largest component
 * positive): the block subspace iteration of pl_buckling_modes on M phi = mu K phi, omega^2 = 1 / mu, without a shift (M is
 * positive definite).  n_sub, rtol, max_iter, tol, max_outer, n_found and PL_ERR_NOCONV as there; PL_ERR_STATE also before
 * pl_set_bc. */
int pl_vibration_modes(pl_handle h, int32_t n_modes, int32_t n_sub, double rtol, int32_t max_iter, double tol,
                       int32_t max_outer, double *omega2 /*[n_modes]*/, double *modes /*[n_modes][6N] or NULL*/,
                       double *residual /*[n_modes] or NULL: |K phi - omega^2 M phi| / |K phi|, free dofs*/,
                       int32_t *n_found, int32_t *outer_iterations);
/* Sensitivities of omega^2 to the strut radii at fixed segment geometry (the convention of pl_sens): for every eigenpair
 * (omega2[i], modes[i]) - any scaling, read with the fixed dofs zeroed -
 *     domega2_i/dr_b = (phi_e^T (dK_e/dr_b) phi_e - omega_i^2 phi_e^T (dM_e/dr_b) phi_e) / (phi_i^T M phi_i),
 * dM_e/dr = (2 / r) M_e[axial and transverse terms] + (4 / r) M_e[torsional and rotary terms]; the point masses have no
 * derivative.  No solve: one pass over the struts.  Rows of a repeated frequency are not derivatives one by one; a sum with
 * equal weights over the whole cluster is (pl_buckling_modes_sens).  1 <= n_modes <= 16; a NaN omega2[i] marks a mode to
 * skip: its row is NaN and it adds nothing to dsum_dr.  dsum_dr needs weights.  Outputs in the caller's strut numbering.
 * PL_ERR_ARG for bad sizes, null inputs and when both outputs are NULL. */
int pl_vibration_modes_sens(pl_handle h, int32_t n_modes, const double *omega2 /*[n_modes]*/,
                            const double *modes /*[n_modes][6N]*/, const double *weights /*[n_modes] or NULL*/,
                            double *domega2_dr /*[n_modes][B] or NULL*/,
                            double *dsum_dr /*[B] or NULL: sum_i weights[i] domega2_i/dr_b, formed on the device*/);

/* ---- transient response (csrc/pl_dyn.h) -------------------------------------------------------------
 * M a + C v + K u = f(t) on the free dofs of pl_set_bc, the supports held at zero: K the strut operator, M the consistent
 * mass of pl_set_mass, C = ray_m M + ray_k K (Rayleigh damping), integrated by the implicit Newmark scheme (beta, gamma) in
 * acceleration form.  Both calls: PL_ERR_STATE on DDM and multi-rank handles, before pl_set_mass, before pl_assemble and with
 * pl_set_periodic constraints.  The handle's single-column state is left untouched. */
/* y_j = c_K K x_j + c_M M x_j in ONE gather (masked != 0: P (...) P x_j, needs pl_set_bc), j < n_rhs <= PL_MULTI_MAX; x, y:
 * [n_rhs][6N] host arrays.  This is the operator of the time step's solve. */
int pl_dyn_spmv_multi(pl_handle h, double c_K, double c_M, int32_t n_rhs, int masked, const double *x, double *y);
/* n_steps steps of size dt from (u0, v0) under the load f_n = sum_p amp[n][p] pattern[p], n = 0 ... n_steps.  a_0 solves
 * M a_0 = f_0 - K u_0 - C v_0; every step solves (M (1 + gamma dt ray_m) + K (beta dt^2 + gamma dt ray_k)) a_{n+1} =
 * f_{n+1} - K ut - C vt for the predictors ut, vt, one column, zero start, Jacobi PCG to rtol within max_iter.  u0, v0 and the
 * patterns are read with the fixed dofs zeroed.  Row n of the outputs is time n dt: probe holds u, v, a of the probe_nodes
 * (caller numbering), energy the kinetic energy 1/2 v.M v, the strain energy 1/2 u.K u and the external work by the trapezoid
 * W_{n+1} = W_n + 1/2 (f_n + f_{n+1}).(u_{n+1} - u_n), snaps[k] is u of row (k + 1) snap_every, state the last u, v, a (a
 * later call started from state's u and v continues the history), iters[n] the PCG iterations of row n's solve.
 * PL_ERR_ARG: dt <= 0, n_steps < 1, gamma < 1/2, beta < (1/2 + gamma)^2 / 4 (unconditionally stable schemes only), a negative
 * Rayleigh coefficient, n_pat > 4, a probe index out of range.  PL_ERR_STATE also before pl_set_bc and when the handle holds
 * non-zero prescribed displacements.  PL_ERR_NOCONV names the step whose solve missed rtol; the outputs are then not written. */
int pl_transient(pl_handle h, int32_t n_steps, double dt, double beta, double gamma, double ray_m, double ray_k,
                 int32_t n_pat, const double *pattern /*[n_pat][6N] or NULL*/, const double *amp /*[n_steps+1][n_pat]*/,
                 const double *u0, const double *v0 /*[6N] or NULL = 0*/, double rtol, int32_t max_iter,
                 int32_t n_probe, const int32_t *probe_nodes, double *probe /*[n_steps+1][3][n_probe][6]: u, v, a*/,
                 double *energy /*[n_steps+1][3]: kinetic, strain, external work*/,
                 int32_t snap_every, double *snaps /*[n_steps/snap_every][6N] u, or NULL*/,
                 double *state /*[3][6N]: final u, v, a, or NULL*/, int32_t *iters /*[n_steps+1] or NULL*/);

/* ---- transient sensitivities (csrc/pl_dyn_sens.h) ----------------------------------------------------
 * The run of pl_transient (same scheme, same solver, same preconditions and error codes), one scalar output per row
 * y_n = l . u_n (out_vec = l, read with the fixed dofs zeroed), an objective of the outputs with weights w_n >= 0 (NULL = 1)
 *     kind 0: J = sum w_n y_n,   kind 1: J = 1/2 sum w_n y_n^2,   kind 2: J = (sum w_n |y_n|^p)^(1/p), p >= 2
 * and dJ/dr_b for every strut radius at fixed segment geometry (the convention of pl_sens) by the discrete adjoint of the
 * scheme: one backward sweep of n_steps + 1 solves with the matrices of the forward steps.  A base acceleration is an argument
 * here: base_dir with base_acc adds the load -base_acc[n] P M e_dir (e_dir: the rigid translation base_dir of ALL nodes), the
 * only load that follows the design; the patterns are dead loads.  n_pat = 0 is legal with a base acceleration.  The histories
 * u + ray_k v and a + ray_m v + a_g e_dir stay on the device for the call: 2 * 48 N (n_steps + 1) bytes; the adjoint is kept for
 * PL_TRANSIENT_SENS_CHUNK rows at a time.  No floating-point atomics in the contraction: two calls return the same bits.
 * PL_ERR_ARG also: kind outside 0 ... 2, p < 2 with kind 2, a negative weight, a NULL out_vec, J or dJ_dr, base_dir without
 * base_acc.  PL_ERR_NOCONV names the row and the pass (forward / adjoint) whose solve missed rtol; no output is then written.
 * The handle's single-column state and its earlier results are left untouched. */
#define PL_TRANSIENT_SENS_CHUNK 32
int pl_transient_sens(pl_handle h, int32_t n_steps, double dt, double beta, double gamma, double ray_m, double ray_k,
                      int32_t n_pat, const double *pattern /*[n_pat][6N] or NULL*/, const double *amp /*[n_steps+1][n_pat]*/,
                      const double *base_dir /*[3] or NULL*/, const double *base_acc /*[n_steps+1], with base_dir*/,
                      const double *u0, const double *v0 /*[6N] or NULL = 0*/, double rtol, int32_t max_iter,
                      const double *out_vec /*[6N]: l*/, int32_t kind, double p, const double *weight /*[n_steps+1] or NULL = 1*/,
                      double *J, double *y /*[n_steps+1] or NULL*/, double *dJ_dr /*[B], caller's strut numbering*/,
                      int32_t *iters /*[2][n_steps+1] or NULL: forward, adjoint*/);

/* ---- frequency response (csrc/pl_harm.h) -------------------------------------------------------------
 * The steady state u e^{iwt} under the load f e^{iwt} on the free dofs of pl_set_bc, the supports held at zero:
 *     A(w) u = f,   A(w) = c_K K + c_M M,   c_K = 1 + i w ray_k,   c_M = i w ray_m - w^2
 * with K, M and the Rayleigh damping of pl_transient.  A is complex symmetric; each frequency is solved by the conjugate
 * orthogonal CG (unconjugated bilinear form, Jacobi-preconditioned with the complex diagonal, zero start), the frequencies of a
 * pass in lock step, one fused gather per iteration.  Complex arrays are complex128: (re, im) pairs.  COCG has no convergence
 * guarantee: lightly damped systems slow down or fail at frequencies with many modes below them, and at an undamped resonance
 * the system is singular - status tells which frequency.  Both calls: PL_ERR_STATE on DDM and multi-rank handles, before
 * pl_set_mass, before pl_assemble and with pl_set_periodic constraints.  The handle's single-column state is left untouched. */
/* y_k = (cK_k K + cM_k M) x_k in ONE gather (masked != 0: P (...) P x_k, needs pl_set_bc), k < n_freq <= PL_MULTI_MAX / 2;
 * coef[n_freq][4] = Re cK, Im cK, Re cM, Im cM; x, y: [n_freq][6N] complex128 host arrays. */
int pl_harm_spmv(pl_handle h, int32_t n_freq, const double *coef, int masked, const double *x, double *y);
/* One solve per omega[k] >= 0 (0: the static solve), k < n_freq, in passes of `block` frequencies (0 = PL_MULTI_MAX / 2, the
 * most).  The load load_re + i load_im is read with the fixed dofs zeroed.  A frequency stops when ||r|| <= rtol ||f||
 * (status 0), at max_iter (1), or at a breakdown - a zero or non-finite p^T A p or r^T z (2).  probe_out: the six complex
 * dofs of the probe_nodes (caller numbering); fields: the whole complex fields; power: Re f^T u, Im f^T u (unconjugated),
 * u^H K u, u^H M u, so that Re f^T u = u^H K u - w^2 u^H M u and -Im f^T u = w (ray_m u^H M u + ray_k u^H K u) is twice the
 * dissipated power over w.  PL_ERR_ARG: n_freq < 1, a negative omega or Rayleigh coefficient, rtol or max_iter not positive,
 * block outside 0 ... PL_MULTI_MAX / 2, a probe index out of range, a NULL omega, load_re, iters, relres or status.
 * PL_ERR_STATE also before pl_set_bc and when the handle holds non-zero prescribed displacements.  PL_ERR_NOCONV when any
 * frequency ends with status != 0; every output is still written. */
int pl_harmonic(pl_handle h, int32_t n_freq, const double *omega /*[n_freq]*/, double ray_m, double ray_k,
                const double *load_re /*[6N]*/, const double *load_im /*[6N] or NULL = 0*/, int32_t n_probe,
                const int32_t *probe_nodes /*[n_probe]*/, double rtol, int32_t max_iter, int32_t block,
                double *probe_out /*[n_freq][n_probe][6] complex*/, double *fields /*[n_freq][6N] complex, or NULL*/,
                double *power /*[n_freq][4], or NULL*/, int32_t *iters /*[n_freq]*/, double *relres /*[n_freq]*/,
                int32_t *status /*[n_freq]: 0 ok, 1 max_iter, 2 breakdown*/);

/* ---- frequency response sensitivities (csrc/pl_harm_sens.h) ------------------------------------------
 * The solves of pl_harmonic (same systems, same solver, same preconditions and error codes; the fields are its bits), one
 * complex output per frequency y_k = l^T u_k (unconjugated; out_vec = l real, read with the fixed dofs zeroed), a real
 * objective of the outputs with weights w_k >= 0 (NULL = 1)
 *     kind 0: J = -sum w_k Im y_k,   kind 1: J = 1/2 sum w_k |y_k|^2,   kind 2: J = (sum w_k |y_k|^p)^(1/p), p >= 2
 * and dJ/dr_b for every strut radius at fixed segment geometry (the convention of pl_sens).  A(w) is complex symmetric, so
 * the adjoint field solves A(w_k) lam_k = l with the matrix of the forward solve; it rides in the same pass as u_k, which
 * therefore takes PL_MULTI_MAX / 4 frequencies at the most.  The load is load_re + i load_im (a dead load) plus, with
 * base_dir, the load -P M e_dir of a base shaken with unit acceleration (e_dir: the rigid translation base_dir of ALL nodes),
 * the only load that follows the design; load_re = NULL is legal with base_dir.  out_vec = NULL: l is the whole load, lam = u,
 * no second solve (the dynamic compliance; with kind 0 and w_k = omega_k / 2 the mean dissipated power), and a pass takes
 * PL_MULTI_MAX / 2 frequencies.  The fields of every frequency stay on the device for the call: 2 * 96 N n_freq bytes, half
 * of it with out_vec = NULL.  No floating-point atomics in the contraction: two calls return the same bits, whatever `block`.
 * iters, relres, status: row 0 the forward solves, row 1 the adjoint ones (zeros with out_vec = NULL).
 * PL_ERR_ARG: the checks of pl_harmonic, kind outside 0 ... 2, p < 2 with kind 2, a negative or non-finite weight, a NULL J
 * or dJ_dr, neither a load nor base_dir, block above the pass limit.  PL_ERR_STATE as pl_harmonic.  PL_ERR_NOCONV when any
 * solve ends with status != 0: iters, relres and status are written, J, y and dJ_dr are not.  PL_ERR_NAN: the objective is
 * not finite.  The handle's single-column state and its earlier results are left untouched. */
int pl_harmonic_sens(pl_handle h, int32_t n_freq, const double *omega /*[n_freq]*/, double ray_m, double ray_k,
                     const double *load_re /*[6N] or NULL with base_dir*/, const double *load_im /*[6N] or NULL = 0*/,
                     const double *base_dir /*[3] or NULL*/, const double *out_vec /*[6N] real, or NULL = the load*/,
                     int32_t kind, double p, const double *weight /*[n_freq] or NULL = 1*/, double rtol, int32_t max_iter,
                     int32_t block /*0 = the most*/, double *J, double *y /*[n_freq] complex or NULL*/,
                     double *dJ_dr /*[B], caller's strut numbering*/, int32_t *iters, double *relres,
                     int32_t *status /*[2][n_freq]: forward, adjoint; or NULL*/);

/* The same condensation, exact and batched, without a handle: n_inst small lattices of ONE topology (a unit cell at
 * several radius sets - the exact DDM mode, Schur datasets), each condensed by a dense Cholesky of K_II in one workgroup
 * of a single launch.  Material, pen_coef and device come from o (stamped by pl_default_opts; the solver fields are
 * ignored).  beam_conn and boundary_nodes are shared by every instance; boundary_nodes gives the row order of S (6 dofs
 * per node, as pl_schur), every other node is interior.  Per instance: node_xyz[3 n_nodes], beam_radius[n_beams],
 * seg_len / seg_nsub[3 n_beams] (pl_mesh_t), S[6nb][6nb] row-major, exactly symmetric, and info: 0 = ok, k > 0 = pivot k
 * of the Cholesky factor of K_II not positive (a mechanism, a floating interior node), -1 = a non-positive radius or
 * segment count; S of a failed instance is NaN, the others are unaffected.  Supported: nb <= 32 boundary nodes,
 * n_nodes - nb <= 16 interior nodes, n_beams <= 512 (PL_ERR_ARG beyond). */
int pl_schur_cells(const pl_opts_t *o, int32_t n_inst, int32_t n_nodes, int32_t n_beams,
                   const int32_t *beam_conn /*[2*n_beams], shared*/, int32_t nb,
                   const int32_t *boundary_nodes /*[nb], shared: the row order of S*/,
                   const double *node_xyz /*[n_inst][3*n_nodes]*/, const double *beam_radius /*[n_inst][n_beams]*/,
                   const double *seg_len /*[n_inst][3*n_beams]*/, const int32_t *seg_nsub /*[n_inst][3*n_beams]*/,
                   double *S /*[n_inst][6nb][6nb]*/, int32_t *info /*[n_inst]*/);

/* The backward half of pl_schur_cells, same conventions (opts, shared beam_conn / boundary_nodes, per-instance geometry,
 * info codes, size limits): from the boundary values u_b of every instance the displacement of the whole cell -
 * u_full repeats u_b on the boundary nodes and holds -K_II^-1 K_IB u_b on the others (no load and no Dirichlet dof on
 * interior nodes, as the DDM assumes) - the same for an adjoint field lam_b (NULL: lam = u), and per strut
 * sens[b] = lam_e^T (dK_e/dr_b) u_e on the recovered fields (the quantity of pl_sens).  Summed over the struts of one
 * radius parameter this is lam_b^T (dS/dr) u_b exactly, at fixed segment geometry.  u_b / lam_b rows follow
 * boundary_nodes; u_full / lam_full are in the cell's own node order.  Any of u_full, lam_full, sens may be NULL (not
 * all).  A cell without interior nodes is legal.  A failed instance (info != 0) gets NaN in its own outputs only. */
int pl_cells_recover(const pl_opts_t *o, int32_t n_inst, int32_t n_nodes, int32_t n_beams,
                     const int32_t *beam_conn /*[2*n_beams], shared*/, int32_t nb,
                     const int32_t *boundary_nodes /*[nb], shared*/,
                     const double *node_xyz /*[n_inst][3*n_nodes]*/, const double *beam_radius /*[n_inst][n_beams]*/,
                     const double *seg_len /*[n_inst][3*n_beams]*/, const int32_t *seg_nsub /*[n_inst][3*n_beams]*/,
                     const double *u_b /*[n_inst][6nb], boundary_nodes order*/,
                     const double *lam_b /*[n_inst][6nb] or NULL: lam = u*/,
                     double *u_full /*[n_inst][6*n_nodes], cell-local node order, or NULL*/,
                     double *lam_full /*[n_inst][6*n_nodes] or NULL*/,
                     double *sens /*[n_inst][n_beams]: lam_e^T (dK_e/dr_b) u_e, or NULL*/,
                     int32_t *info /*[n_inst]*/);

/* Debug / test access to the condensed per-strut records: rec[8*B] = (a, c, e1, e2, e3, dx, dy, dz). */
int pl_get_records(pl_handle h, double *rec);

/* Debug / test access to the solver's partition, caller's node numbering; any pointer may be NULL; -1 where absent.
 * The spans of the preconditioner's modes are sets of nodes, so a host restatement of M^-1 (oracle/precond_oracle.py) needs
 * exactly this and nothing else of the solver's state.  [n_nodes] each.
 * FEM handles: tile_of_node = the K*p tile (the tile level's blocks), agg_of_node = the aggregate of the dense level
 * (precond 2 / 3 / 4), local_agg_of_node = the aggregate of the rank-local level (precond 4), eliminated = 1 on the nodes
 * opts.condense takes out of the CG (chosen by pl_set_bc, valid after pl_assemble; which solver forms honour it:
 * pl_stats_t.condensed_nodes).  DDM handles after pl_ddm_set_geometry: agg_of_node = the aggregate of precond = 4. */
int pl_debug_partition(pl_handle h, int32_t *tile_of_node, int32_t *agg_of_node, int32_t *local_agg_of_node,
                       uint8_t *eliminated);

/* Measurement hooks (bench.py): run `reps` launches of one kernel on the handle's stream between two HIP
 * events and return the average milliseconds.  which: 0 = K*p (PCG operator), 1 = record build,
 * 2 = BSR fill, 3 = one full PCG iteration, 4 = BSR SpMV; on a multi-GPU handle also 5 = the interface all-reduce of
 * one K*p (staging kernels + RCCL) and 6 = the coarse-residual all-reduce - collective calls, every rank must make them.
 * With the multi-level PCG: 7 = K*p on fp32-stored vectors, 8 = one iteration of the fp32 inner PCG (precision 1),
 * 9 = one iteration of the mixed PCG (precision 2) - 8 and 9 call the solver's own iteration, so they apply the operator
 * as the handle's plan does (both passes where it eliminates nodes); 10 = the operator exactly as the next pl_solve applies it (BOTH passes
 * under node elimination, fp32-stored operands in the fp32 solver modes) - what a roofline of "K*p" must be priced with;
 * 11 = one whole PCG iteration exactly as the next pl_solve runs it (storage width and node elimination of its plan);
 * 12 = the kernel of pl_sens_gram alone, on the columns (and with the column count) of the last pl_sens_gram call of this
 * handle, which stay on the device (PL_ERR_STATE without such a call). */
int pl_time_kernel(pl_handle h, int which, int reps, double *avg_ms);
/* Algorithmic byte counts of SURVEY.md section 8(d) for this handle: out[0]=spmv, out[1]=pcg_iter, out[2]=bsr - with the
 * storage widths the next pl_solve uses: strut records and the explicit K are fp64 in every mode, the PCG vectors are 4 bytes
 * wide where opts.precision stores them in fp32 (precision 1: all of them; 2: p and K*p). */
int pl_algorithmic_bytes(pl_handle h, double *out3);
/* What the vector kernels of the multi-level PCG read per node on this handle (node words): instead of
 * 24 bytes of Jacobi weights, 12 bytes of lever arm and the Dirichlet bits, one 4-byte word {rx, ry, rz, class} where the
 * lattice allows it.  The two halves are independent:
 *   classes_on  1 if the last pl_assemble found at most 256 distinct rows {six fp32 weights, Dirichlet bits} and every node
 *               matched its row bit for bit (0: too many, an attempt skipped after earlier failures, no assembly yet)
 *   n_classes   rows counted by the last attempt (may exceed 256 when classes_on = 0; 0 when no attempt was made)
 *   bytes_on    1 if every lever arm is a signed byte in units of 2^-byte_exp, exactly (decided at pl_create)
 *   byte_exp    that exponent, 0 .. 8; -1 when bytes_on = 0
 * Any pointer may be null.  Everything is 0 / -1 with PL_NODE_WORDS=0, on multi-GPU handles and with precond = 4. */
int pl_node_words_info(pl_handle h, int *classes_on, int *n_classes, int *bytes_on, int *byte_exp);
/* Forget what earlier solves taught this handle: the iteration count that places the first look at the residual history of
 * the next solve (pl_solve) and the previous solution a warm start would begin from.  bench.py uses it
 * to report the cold value of a loop of identical solves beside the ordinary one. */
int pl_forget_history(pl_handle h);

/* Test hook for the device dense SPD solver behind the two-level preconditioner (blocked Cholesky + inverse factor):
 * solves A x = b for a host SPD matrix A[n*n] (row-major) on `device`; quad (may be NULL) gets b^T A^-1 b.
 * fp32_factor != 0 stores the inverse factor W = L^-1 in fp32, as the preconditioner does (x is then W32^T W32 b:
 * accurate to ~1e-6 cond(A)^(1/2), which is all a preconditioner needs); 0 keeps it in fp64.
 * Returns PL_ERR_ARG if A is not positive definite. */
int pl_debug_spd_solve(int device, int32_t n, const double *A, const double *b, double *x, double *quad,
                       int32_t fp32_factor);

/* Test hook for the dense level with the switches of production (tests/test_gpu_dense_level.py): factors the host SPD matrix
 * A[n*n] (row-major; padded to np = the next multiple of 64 with an identity diagonal) with block bandwidth bw_blocks
 * (blocks (i, j), i - j > bw_blocks, must be zero; 0 = full), builds the inverse factor W = L^-1 in `storage` = 64, 32 or 16
 * bits (fp64, fp32, bfloat16) - in one launch after the factorisation chain (trtri_rows = 0) or in ranges of at least
 * trtri_rows block rows on a second stream behind it, as the assembly does with 3 - and applies it to r[n]:
 * t = W r, y = W^T t, quad = t.t + the sum of add0[64] (a slotted scalar, as the PCG passes r.D^-1 r).  For storage 32 and
 * 16 and np <= 2 048, also the explicit inverse Ainv = W^T W in fp32 and the one-GEMV form y_one = Ainv r,
 * quad_one = r.y_one + sum(add0); *one_gemv says whether that ran (Ainv, y_one, quad_one are untouched otherwise).
 * band_roundtrip != 0 first packs the block band of A and unpacks it again, as the multi-GPU assembly does around its
 * all-reduce (needs 0 < bw_blocks < np / 64 - 1).  The calls are the assembly's and the preconditioner's own.
 * W, Wt (= W^T as stored): [np*np], widened exactly to double; Ainv: [np*np]; t, y, y_one: [np]; info[2]: info[0] != 0 if a
 * pivot was not positive (the outputs are then meaningless; the call still returns PL_OK). */
int pl_debug_dense_level(int device, int32_t n, const double *A, int32_t bw_blocks, int32_t storage, int32_t trtri_rows,
                         int32_t band_roundtrip, const double *r, const double *add0, double *W, double *Wt, float *Ainv,
                         double *t, double *y, double *quad, double *y_one, double *quad_one, int32_t *one_gemv,
                         int32_t *info);

/* ---- multi-GPU (slab partition, RCCL) ---------------------------------------------------------------- */
/* Size of the opaque RCCL unique id the ranks must share (rank 0 fills it with pl_dist_unique_id). */
int pl_dist_unique_id_bytes(void);
int pl_dist_unique_id(void *id_out);
/* Loopback transport: an id (same size as the RCCL one) that makes pl_dist_init attach the handle to an IN-PROCESS group
 * instead of an RCCL communicator - `world` handles of one process on one device, every collective of the multi-GPU path
 * (interface rows, scalar blocks, coarse operator band) summed through device buffers.  Each rank must then be driven by
 * its own host thread (collective calls meet at a host barrier: pl_dist_init, pl_set_bc on an assembled handle,
 * pl_assemble, pl_solve, pl_spmv*, pl_reactions, pl_time_kernel), exactly as each rank of an RCCL run is driven by its
 * own process.  This is how the whole multi-rank solver path runs with world = 2 ... 16 on a one-GPU box (tests/
 * test_gpu_loopback.py); it also serves to run several sub-domains on one GPU.  A rank that never arrives at a
 * collective makes the others fail with PL_ERR_HIP after 120 s instead of hanging. */
int pl_dist_loopback_id(void *id_out);
/* Loopback groups only (no-op otherwise): declare the group broken, so that ranks waiting at a collective return
 * PL_ERR_HIP at once - what a driver calls when one of its rank threads failed outside a collective. */
int pl_dist_abort(pl_handle h);
/* Attach this handle (one per rank/GPU) to a communicator.  shared_nodes lists, for each node of THIS rank's
 * sub-lattice that also exists on other ranks, its local index and a global id (dense 0..n_shared_global-1);
 * partial forces on those nodes are summed across ranks after every local K*x. */
int pl_dist_init(pl_handle h, int rank, int world, const void *unique_id, const int32_t *shared_local,
                 const int32_t *shared_global, int32_t n_shared, int32_t n_shared_global);

/* ---- host-side lattice generation (no GPU involved) -------------------------------------------------------- */
/* Lattice.generate_lattice + Cell.generate_beams + define_beam_node_index (lattice.py:421-483,665-698,
 * cell.py:293-382) on flat arrays, multi-threaded: for every cell c and template strut s the two end points
 * tmpl[6s + 3e + k] * cell_size[3c + k] + cell_coord[3c + k]; nodes and struts de-duplicated through coordinates
 * rounded to 9 decimals (first creator wins); nodes numbered in (x, y, z) order, struts in (lower end, upper end) order.
 * cell_radii[c * n_geom + g] is the radius the struts of geometry g get in cell c (gradient already applied),
 * tmpl_type[s] the geometry of template strut s.  The result lives in a library-owned object: read the sizes from
 * *info, fetch into caller arrays of those sizes (any pointer may be NULL), free.  created_nodes[2 (c n_tmpl + s) + e] /
 * created_beam[c n_tmpl + s] give node and strut of every CREATED strut end (the hybrid-collision pass needs them).
 * Returns PL_ERR_STATE when the lattice is too irregular for the direct-address node table (caller falls back). */
typedef struct pl_lattice pl_lattice;
typedef struct {
  int64_t n_nodes, n_beams, n_cell_beam, n_cell_node, n_created;
} pl_lattice_info_t;
int pl_generate_lattice(int64_t n_cells, const double *cell_coord, const double *cell_size, const double *cell_radii,
                        int32_t n_geom, int32_t n_tmpl, const double *tmpl, const int32_t *tmpl_type,
                        pl_lattice **out, pl_lattice_info_t *info);
int pl_lattice_fetch(const pl_lattice *L, double *node_xyz, int32_t *beam_conn, double *beam_radius, int32_t *beam_type,
                     int32_t *beam_cell0, int64_t *cell_beam_ptr /*[n_cells+1]*/, int64_t *cell_beam_idx,
                     int64_t *cell_node_ptr /*[n_cells+1]*/, int64_t *cell_node_idx, int32_t *created_nodes,
                     int32_t *created_beam);
void pl_lattice_free(pl_lattice *L);

/* LatticeSim.set_penalized_beams (lattice_sim.py:245-308) on arrays: every strut becomes [pen(L_zone at point1) | middle
 * | pen(L_zone at point2)]; new points at end + (other - end) / round(length, 4) * L_zone (beam.py:135,300-312).  Outputs
 * per strut: the three geometric segment lengths (0 = absent), gmsh's element count int(len / mesh_size + 0.99) per
 * segment (lattice_generation.py:50-64) and the two penalisation points (NaN where absent).  lzone = NULL: no
 * penalisation (one segment per strut).  Host code, multi-threaded. */
int pl_penalize(int64_t n_beams, const double *node_xyz, const int32_t *beam_conn, const double *lzone /*[2B] or NULL*/,
                double mesh_size, double *seg_len /*[3B]*/, int32_t *seg_nsub /*[3B]*/, double *pen_xyz /*[6B]*/);

/* LatticeSim.define_node_index_boundary (lattice_sim.py:546-563) with the visit order of get_global_displacement
 * (:502-542) on arrays: a node gets a boundary index when it lies on the box of one of its cells (exact coordinate
 * comparison with the cell's origin / origin + size); indices are handed out in the order cells (ascending) then nodes of
 * the cell (ascending node index = coordinate order) first meet them.  index_boundary[n_nodes] (-1 elsewhere),
 * visit[<= n_nodes] = the nodes in that order, *n_visit their number.  Host code, multi-threaded. */
int pl_boundary_index(int64_t n_cells, const int64_t *cell_node_ptr, const int64_t *cell_node_idx, int64_t n_nodes,
                      const double *node_xyz, const double *cell_coord, const double *cell_size, int64_t *index_boundary,
                      int64_t *visit, int64_t *n_visit);

/* The same for the reference's own rows (LatticeSim(reference_compat=True): the rows of a cell are its design nodes AND the
 * penalisation points of its struts, visited in (round(x, 9), round(y, 9), round(z, 9), index) order - _sorted_nodes,
 * lattice_sim.py:193-199): every cell's rows are sorted by that key here, all cells in parallel. */
int pl_boundary_index_rows(int64_t n_cells, const int64_t *cell_node_ptr, const int64_t *cell_node_idx, int64_t n_nodes,
                           const double *node_xyz, const double *cell_coord, const double *cell_size,
                           int64_t *index_boundary, int64_t *visit, int64_t *n_visit);

/* Neighbour halo exchange ("sum of interface-node partial forces with the two neighbouring
 * slabs"): shared_peer[i] = the rank that holds the other copy of shared entry i of pl_dist_init (a node shared with
 * several ranks is listed once per peer there).  After this call the interface rows of every K*x travel by grouped
 * ncclSend / ncclRecv between neighbours - each rank moves its own planes only, concurrently - instead of the all-reduce
 * over all planes; the dot-product slots take a small all-reduce of their own.  Both ranks of a pair order their
 * common nodes by global interface id, so no further handshake is needed.  Collective: every rank must call it. */
int pl_dist_set_peers(pl_handle h, const int32_t *shared_peer /*[n_shared]*/);

#ifdef __cplusplus
}
#endif
#endif /* PYLATTICE_HIP_H */
