/*
 * mgmc.h -- C-ABI boundary of the MI355X-native Multigrid Monte Carlo (MGMC) sampler.
 *
 * This is the drop-in boundary for the reference's `driver_mgmc` hot path
 * (nilsfriess/MultigridMC, all citations relative to its src/ directory):
 *
 *   Sampler::apply(f, x)                     sampler/sampler.hh:41           -> mgmc_apply / mgmc_sample
 *   Sampler::fix_rhs(f)                      sampler/sampler.hh:56           -> mgmc_set_rhs
 *   MultigridMCSampler ctor                  sampler/multigridmc_sampler.cc:8-100 -> mgmc_create
 *   MultigridMCSampler::sample(level)        sampler/multigridmc_sampler.cc:103-130 (one V/W-cycle per sample)
 *   SORSampler::apply                        sampler/sor_sampler.cc:37-59    -> mgmc_sor_sampler_apply
 *   SORSmoother::apply_sparse                smoother/sor_smoother.cc:56-78  -> mgmc_smoother_apply
 *   LinearOperator::apply                    linear_operator/linear_operator.hh:66-76 -> mgmc_operator_apply
 *   IntergridOperator::restrict              intergrid/intergrid_operator.hh:74-88    -> mgmc_restrict
 *   IntergridOperator::prolongate_add        intergrid/intergrid_operator.hh:106-120  -> mgmc_prolongate_add
 *   LinearOperator::coarsen (Galerkin RAP)   linear_operator/linear_operator.cc:10-23 -> mgmc_describe (stencils)
 *   measure_sampling_time QoI loop           driver_mgmc.cc:66-94            -> mgmc_sample + mgmc_qoi_moments
 *
 * Every function returns MGMC_OK (0) or a negative MGMC_E* code; the text of the last
 * error is available from mgmc_last_error(handle) (or mgmc_last_error(NULL) for errors
 * raised before a handle exists).  The reference prints and exit(-1)s instead
 * (e.g. sampler/multigridmc_sampler.cc:47-49); the C++ wrapper in mgmc_sampler.hh restores
 * that behaviour at the driver level.
 *
 * Vectors crossing this boundary as host pointers use the reference's layout: one double per
 * interior lattice vertex, numbered lexicographically with x fastest
 * (lattice/lattice3d.hh:126-135, lattice/lattice2d.hh:95-103).  Device-resident state uses
 * a padded zero-halo layout ("Data layout in HBM") and never leaves HBM unless a
 * get/apply call asks for it.
 */
#ifndef MGMC_H
#define MGMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGMC_ABI_VERSION 5

/* error codes */
#define MGMC_OK 0
#define MGMC_E_INVALID -1   /* invalid argument / configuration           */
#define MGMC_E_HIP -2       /* HIP runtime error (incl. no device)        */
#define MGMC_E_NOMEM -3     /* device allocation failed                   */
#define MGMC_E_UNSUPPORTED -4 /* feature not (yet) on the device path     */
#define MGMC_E_NONFINITE -5 /* the chain state became NaN / Inf (guard on the QoI vertex, or the
                               lattice centre without a QoI, checked after every cycle); the flag
                               stays set until mgmc_set_state */

/* smoother kinds (parameters.hh:145-174 MultigridParameters::smoother) */
#define MGMC_SMOOTHER_SOR 0   /* forward SOR pre-sampler, backward SOR post-sampler */
#define MGMC_SMOOTHER_SSOR 1  /* SSOR (forward+backward) pre- and post-sampler      */

/* coarse solvers (MultigridParameters::coarse_solver) */
#define MGMC_COARSE_SSOR 0
#define MGMC_COARSE_CHOLESKY 1 /* Cholesky factors of the coarsest level (cholesky_sampler.cc:9-41): dense inverses up to
                                  8192 unknowns, blocked banded solves above (rows of at most 4096 unknowns) */

/* fine-level operators (driver_mgmc.cc:414-425, PriorParameters::pde_model) */
#define MGMC_OPERATOR_FD 0  /* ShiftedLaplaceFDOperator: 5/7-point (shiftedlaplace_fd_operator.cc:9-57) */
#define MGMC_OPERATOR_FEM 1 /* ShiftedLaplaceFEMOperator: Q1 elements, 9/27-point
                               (shiftedlaplace_fem_operator.cc:9-145) */
#define MGMC_OPERATOR_SQUARED_FD 2 /* SquaredShiftedLaplaceFDOperator, 2D 13-point
                                      (squared_shiftedlaplace_fd_operator.cc:9-96); CSR path only */

/* correlation-length models (linear_operator/correlationlength_model.hh:45-112) */
#define MGMC_KAPPA_CONSTANT 0 /* kappa^2 = 1 / Lambda^2 */
#define MGMC_KAPPA_PERIODIC 1 /* Lambda(x) = L1 + L2 prod_d cos(pi x_d), L1/2 = (Lambda_max +/- Lambda_min)/2 */
#define MGMC_KAPPA_GIVEN 2    /* constant kappa^2 given directly (mgmc_config.kappa_sq's convention) */

/* sweep directions (smoother/sor_smoother.hh:14-18) */
#define MGMC_FORWARD 1
#define MGMC_BACKWARD 2

/* Plain-old-data configuration; mirrors the MultigridParameters / LatticeParameters /
 * ConstantCorrelationLengthModelParameters / PriorParameters fields of auxilliary/parameters.hh
 * that reach the hot path.  The fine operator is ShiftedLaplaceFDOperator or
 * ShiftedLaplaceFEMOperator with constant kappa^2 = 1/Lambda^2
 * (linear_operator/shiftedlaplace_fd_operator.cc:9-57, shiftedlaplace_fem_operator.cc:9-145,
 * correlationlength_model.hh:45-66).  Zero-initialise and set the fields: 0 in fine_operator is
 * the FD operator. */
typedef struct mgmc_config {
    int dim;            /* 2 or 3 */
    int nx, ny, nz;     /* cells per direction (nz ignored for dim=2) */
    int nlevel;         /* number of multigrid levels (>=1) */
    int cycle;          /* 1 = V-cycle, 2 = W-cycle, ... (applies below level 0) */
    int npresmooth;
    int npostsmooth;
    int ncoarsesmooth;
    int smoother;       /* MGMC_SMOOTHER_* */
    int coarse_solver;  /* MGMC_COARSE_* */
    int verbose;
    double omega;          /* overrelaxation factor of the Gibbs samplers */
    double coarse_scaling; /* factor on the prolongated coarse correction */
    double kappa_sq;       /* 1/Lambda^2 */
    int fine_operator;     /* MGMC_OPERATOR_* (ABI 2) */
    int pad_;
} mgmc_config;

/* Host-side description of one multigrid level (no device needed). */
typedef struct mgmc_level_desc {
    int nx, ny, nz;       /* cells per direction on this level (nz = 0 for 2D) */
    int npoints;          /* stencil points: 5/7 (fine FD) or 9/27 (fine FEM, Galerkin) */
    int ncolours;         /* colours of the Gibbs sweep: 2 (5/7-point) or 2^dim (9/27-point) */
    int varcoef;          /* 1: per-vertex coefficients (mgmc_create_csr); stencil = the centre row */
    uint64_t ndof;        /* number of interior unknowns */
    /* stencil coefficients indexed by offset (dz+1)*9 + (dy+1)*3 + (dx+1) (3D) or
     * (dy+1)*3 + (dx+1) (2D); entries outside the stencil are 0 */
    double stencil[27];
} mgmc_level_desc;

typedef struct mgmc_handle mgmc_handle;

/* ---- host-only helpers (no GPU touched) ---- */
int mgmc_abi_version(void);
/* Handles created and not yet destroyed in this process (any mgmc_create* variant).  A host
 * integration checks with it that its owners release their device state (the reference's
 * shared_ptr ownership). */
int mgmc_live_handles(void);
/* Validate cfg and fill out[0..nlevel-1] with the level hierarchy and Galerkin stencils.
 * Returns the number of levels (> 0) or a negative MGMC_E* code. */
int mgmc_describe(const mgmc_config* cfg, mgmc_level_desc* out, int max_levels);
const char* mgmc_last_error(const mgmc_handle* h);

/* ---- fine operators as matrices (ABI 3; host only, no GPU touched) ----
 * The reference's LinearOperator subclasses with any correlation-length model
 * (ShiftedLaplaceFDOperator shiftedlaplace_fd_operator.cc:9-57, ShiftedLaplaceFEMOperator
 * shiftedlaplace_fem_operator.cc:9-145, SquaredShiftedLaplaceFDOperator
 * squared_shiftedlaplace_fd_operator.cc:9-96; PeriodicCorrelationLengthModel
 * correlationlength_model.hh:68-112) assembled as their A_sparse: CSR, rows = interior vertices in
 * the lattice order (x fastest), columns ascending, entries summed as the reference sums them. */
typedef struct mgmc_operator_desc {
    int dim, nx, ny, nz;       /* lattice (nz ignored for dim = 2) */
    int pde;                   /* MGMC_OPERATOR_FD / _FEM / _SQUARED_FD */
    int kappa_model;           /* MGMC_KAPPA_CONSTANT / _PERIODIC */
    double Lambda;             /* constant model */
    double Lambda_min, Lambda_max; /* periodic model */
    double kappa_sq;           /* MGMC_KAPPA_GIVEN */
} mgmc_operator_desc;
/* rows and stored entries of the assembled matrix */
int mgmc_operator_csr_size(const mgmc_operator_desc* d, int64_t* nrow, int64_t* nnz);
/* fill rowptr[nrow + 1], col[nnz], val[nnz] */
int mgmc_operator_csr(const mgmc_operator_desc* d, int64_t* rowptr, int32_t* col, double* val);

/* The colouring mgmc_create_csr gives a level with this matrix (ABI 5; host only): 2 (red-black, a
 * fine level whose couplings are all axis neighbours), 4 / 8 (coordinate parities, other reach-1
 * levels) or 9 / 27 (coordinates mod 3, reach-2 levels).  cfg gives the level's lattice; level 0 is
 * the fine level.  Same validation as mgmc_create_csr. */
int mgmc_csr_colour_scheme(const mgmc_config* cfg, int level, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                           int* scheme);

/* The constant stencil of a matrix (ABI 5; host only): MGMC_OK and stencil[27] (offset order of
 * mgmc_level_desc) if every row of the CSR is that 3^d stencil truncated at the lattice boundary, in
 * ascending column order with bitwise equal values -- the matrix of a constant-coefficient operator
 * such as ShiftedLaplaceFDOperator / ShiftedLaplaceFEMOperator with a constant correlation length;
 * MGMC_E_UNSUPPORTED otherwise (use mgmc_create_csr).  A reference-side adapter calls this on
 * LinearOperator::get_sparse() (linear_operator.hh:93) to pick the stencil fast path. */
int mgmc_stencil_of_csr(const mgmc_config* cfg, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                        const double* val, double* stencil);

/* A constant stencil plus a diagonal field (ABI 5; host only): MGMC_OK and stencil[27] (offset order of
 * mgmc_level_desc, stencil[13] = 0.0) if the CSR on cfg's 3D lattice is a constant, symmetric axis-neighbour
 * stencil truncated at the boundary plus an arbitrary positive finite diagonal: every stored off-diagonal is an
 * axis neighbour, all entries of one offset are bitwise equal, -x/+x, -y/+y, -z/+z are equal, no interior
 * coupling is missing -- the matrix of ShiftedLaplaceFDOperator with any correlation-length model (kappa^2
 * enters its diagonal only).  MGMC_E_UNSUPPORTED otherwise; same argument validation as mgmc_create_csr.
 * mgmc_create_csr runs this check on its fine matrix: a level that passes (a constant diagonal included) and
 * has the z-sweep's shape (3D, nx a multiple of 64, a coarser level) is swept and restricted by the z-marching
 * kernels with the diagonal streamed per vertex (mgmc_level_kernels: diag=field), bitwise equal to the field
 * kernels it replaces; MGMC_DISABLE=zsweep keeps those. */
int mgmc_vardiag_of_csr(const mgmc_config* cfg, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                        const double* val, double* stencil);

/* Host-side bounds check of one level's padded layout (ABI 5; host only; mgmc_create runs it on
 * every level of every handle).  families: MGMC_LAYOUT_* bits of the kernels that address the level;
 * reach: 1 (3^d couplings) or 2 (the squared FD operator's levels); zrestrict_cx: coarse points per
 * tile of the z-marching residual + restriction on this level (0: none).  legacy: bit 0 builds the
 * round-2 reach-2 layout without its margin rows / planes, bit 1 the unclamped restriction columns,
 * bit 2 a j-sweep grid 8 workgroups short (all wrong: kept so the test shows the check catches them).  MGMC_OK, or MGMC_E_INVALID
 * with the offending offset range in mgmc_last_error(NULL). */
#define MGMC_LAYOUT_POINT 1u
#define MGMC_LAYOUT_PAIRS 2u
#define MGMC_LAYOUT_ZSWEEP 4u
#define MGMC_LAYOUT_ZSWEEP_COARSE 8u
#define MGMC_LAYOUT_ZRESTRICT 16u
#define MGMC_LAYOUT_RB2D 32u
#define MGMC_LAYOUT_JSWEEP 64u     /* + a replay of the j-marching half-sweeps' whole grid (256 CUs) */
#define MGMC_LAYOUT_QRESTRICT 128u /* 2D fused last pre-sweep + residual + restriction */
int mgmc_check_layout(int dim, const int* n, int reach, unsigned families, int zrestrict_cx, int legacy);

/* ---- lifetime ---- */
/* (seed, chain_id) name the noise stream: every normal is Philox4x32-10 under the 64-bit key
 * (lo32(seed), lo32(chain_id) ^ hi32(seed)) with the counter (pair id, sweep tag, lo32(sample), hi32(sample)).
 * The seed and the sample index are full 64-bit words.  The chain id is taken modulo 2^32 in the key, so
 * every mgmc_create* variant returns MGMC_E_INVALID unless chain_id + nchains - 1 < 2^32 (nchains = 1
 * here): ids 2^32 apart would draw one stream.  128 bits go into a 64-bit key, so
 * (seed ^ (d << 32), chain_id ^ d) names the same stream as (seed, chain_id) for every 32-bit d: that
 * alias is by construction and is not rejected. */
int mgmc_create(const mgmc_config* cfg, int device, uint64_t seed, uint64_t chain_id, mgmc_handle** out);
/* A sampler on a fine operator given as a matrix (LinearOperator::A_sparse, linear_operator.hh:187):
 * CSR on cfg's lattice (rows = interior vertices, columns strictly ascending, a positive diagonal,
 * couplings at most 2 vertices apart per direction).  Every coarse level is the Galerkin product
 * R A R^T (linear_operator.cc:10-23) formed on the host; every level is swept with its own per-vertex
 * coefficients (2 colours for a 5/7-point fine level, 2^d for reach-1 levels, 3^d for reach-2
 * levels such as the squared FD operator's).  cfg.kappa_sq and cfg.fine_operator are ignored. */
int mgmc_create_csr(const mgmc_config* cfg, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                    const double* val, int device, uint64_t seed, uint64_t chain_id, mgmc_handle** out);
/* Batched chains (ABI 4): nchains (1..16) independent chains chain0, chain0+1, ... in one handle.
 * They share the hierarchy, the stencils and the low-rank data (B, B_bar); each keeps its own state
 * and right-hand side in HBM and its own Philox key make_key(seed, chain0 + c), so chain c draws
 * exactly what a single-chain handle with chain_id = chain0 + c draws (bitwise); chain0 + nchains - 1
 * must be below 2^32 (the key's contract, at mgmc_create).  Every kernel of
 * the cycle covers all chains in one launch; the low-rank fix reads B_bar once per row for all
 * chains (x -= B_bar W, W = B^T X: the (N x m)(m x C) product of the batch, sor_smoother.cc:47-51).
 * The entry points below without _chain act on every chain (set_rhs, set_state: the same vector)
 * or on chain 0 (get_state, get_series, qoi_moments).  Replaces running several
 * MultigridMCSampler objects (driver_mgmc.cc:188-314 measure_convergence's chains). */
int mgmc_create_batch(const mgmc_config* cfg, int device, uint64_t seed, uint64_t chain0, int nchains,
                      mgmc_handle** out);
int mgmc_create_csr_batch(const mgmc_config* cfg, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                          const double* val, int device, uint64_t seed, uint64_t chain0, int nchains,
                          mgmc_handle** out);
/* A sampler whose fine level is the constant stencil fine_stencil[27] (ABI 5; e.g. from
 * mgmc_stencil_of_csr): the stencil hierarchy of mgmc_create (Galerkin levels by stencil RAP, the
 * fused z-marching / pair-pass kernels) without a kappa^2.  Couplings only to axis neighbours:
 * red-black fine sweeps; otherwise 2^d colours.  cfg.kappa_sq and cfg.fine_operator are ignored. */
int mgmc_create_stencil_batch(const mgmc_config* cfg, const double* fine_stencil, int device, uint64_t seed,
                              uint64_t chain0, int nchains, mgmc_handle** out);
int mgmc_nchains(const mgmc_handle* h);
int mgmc_destroy(mgmc_handle* h);
int mgmc_level_desc_get(const mgmc_handle* h, int level, mgmc_level_desc* out);
/* The kernels this handle runs on a level (ABI 5), as text "sweep=<kernel>[;post_sweep=<kernel>]
 * [;noise=<source>][;residual_restrict=<kernel>][;rhs=zero][;diag=field][;lowrank=<path>][;quads=window]", the keys in this
 * order -- for labels (bench.py) and profiles;
 * quads=window: a 3D k_sweep_quads<3> level whose rows (nx/2 pairs, not a divisor of 64) run the three-load
 * window instances; without the key such a level runs the lane-shift instances;
 * <source>: restriction | tail | restriction+tail -- sweeps of the level read Box-Muller pairs drawn by the
 * restriction launch before the first pre-sweep and / or a tail launch's spare workgroups;
 * rhs=zero, on level 0 only: the level's right-hand side is all +0.0 (prior sampling: as created, or after a
 * mgmc_set_rhs / mgmc_apply of zeros; -0.0, denormals and NaN are not zero) and the cycle's z-marching
 * sweeps and residual + restriction named above run their instances that take it as a constant instead of
 * reading it -- same bits; absent on every other level, with a low-rank part, and on the general kernels;
 * diag=field, on level 0 of a matrix handle only: the fine matrix is a constant stencil plus a diagonal field
 * (mgmc_vardiag_of_csr) and the level runs k_zsweep_rb7<...,VD> and, unless MGMC_DISABLE=zrestrict,
 * k_zresrestrict<7,64,4|8>, their instances that stream the diagonal per vertex; such a level has no post_sweep
 * (the prolongation is a launch of its own) and never rhs=zero; mgmc_level_desc.varcoef stays 1;
 * <path> on a posterior level: small | rows | dense | dense,rhs_inplace */
int mgmc_level_kernels(const mgmc_handle* h, int level, char* out, size_t n);

/* ---- posterior operator Q = A + B Sigma^{-1} B^T (MeasuredOperator) ----
 * Replaces MeasuredOperator's B / Sigma (linear_operator/measured_operator.cc:9-49,
 * LinearOperator::get_B / get_Sigma, linear_operator.hh:187-197).  B is N x m in CSC form:
 * column k holds rows[colptr[k] .. colptr[k+1]) (reference vertex indices, strictly ascending)
 * with values vals[...]; sigma[k] > 0 is the diagonal of Sigma.  A column listing all N rows is a
 * dense column (the global average measurement).  Coarse levels get B_c = R B, Sigma_c = Sigma
 * (linear_operator.cc:10-23); every SOR smoother sets up its B_bar (sor_smoother.cc:17-37) here,
 * so the call costs 2 m noise-free sweeps per level.  From then on every sweep applies the
 * low-rank fix and noise, and residuals / operator applications include B Sigma^{-1} B^T.
 * m = 0 restores the prior operator.  1 <= m <= 64.  Invalid arguments (MGMC_E_INVALID from the
 * checks of m, colptr, rows, vals, sigma) leave the handle unchanged; a failure after them (a coarse
 * band the blocked Cholesky cannot take, the host work limit, an allocation) leaves the prior operator
 * (no low-rank part on any level, the prior's coarse factors) and returns the error code. */
int mgmc_set_lowrank(mgmc_handle* h, int m, const int64_t* colptr, const int64_t* rows, const double* vals,
                     const double* sigma);
/* m of the current low-rank part (LinearOperator::get_m_lowrank); *nrows_bbar = rows stored for
 * B_bar of (level, direction) */
int mgmc_lowrank_info(const mgmc_handle* h, int level, int direction, int* m, int64_t* nrows_bbar);
/* testing hook: the handle's next n builds of the coarse Cholesky factor fail with MGMC_E_NOMEM, so
 * tests can drive mgmc_set_lowrank's rollback (a failed restore leaves the handle refusing the cycle
 * and solver calls until a later mgmc_set_lowrank succeeds).  n = 0 clears it. */
int mgmc_debug_fail_coarse_factor(mgmc_handle* h, int n);
/* testing hook: measures the LDS poison of MGMC_POISON=1 (the NaN fill launched before every op of the cycle
 * graph and every LDS-using launch of the per-level calls).  Launches that fill (nothing without
 * MGMC_POISON), then *nwg = 2 x (compute units) probe workgroups of the fill's footprint (80 KB of LDS), which
 * read every word of their LDS without writing any.  *nwg_all_nan = the probe workgroups that read NaN in
 * every word, *min_nan_fraction = the smallest fraction of NaN words any of them read.  Full coverage is
 * *nwg_all_nan == *nwg; without MGMC_POISON the call returns MGMC_OK and the counts say what the LDS held. */
int mgmc_debug_lds_probe(mgmc_handle* h, int64_t* nwg, int64_t* nwg_all_nan, double* min_nan_fraction);

/* ---- Sampler interface (host buffers, reference layout) ---- */
int mgmc_set_rhs(mgmc_handle* h, const double* f, size_t n);       /* fix_rhs: f stays in HBM */
int mgmc_set_state(mgmc_handle* h, const double* x, size_t n);
int mgmc_get_state(mgmc_handle* h, double* x, size_t n);
int mgmc_set_state_chain(mgmc_handle* h, int chain, const double* x, size_t n);
int mgmc_get_state_chain(mgmc_handle* h, int chain, double* x, size_t n);
/* Sampler::apply(f, x): upload f and x, run one MGMC cycle, download x (PCIe inclusive). */
int mgmc_apply(mgmc_handle* h, const double* f, double* x, size_t n);

/* ---- device-resident sampling loop (the hot path) ----
 * Run nsteps MGMC cycles on the device-resident state.  After every cycle the QoI
 * z = x[qoi_index] (reference index, radius-0 measurement vector,
 * linear_operator/measured_operator.cc:74-91) is appended to a device time series and folded
 * into device-side running moments.  If qoi_out != NULL the nsteps values are copied back. */
int mgmc_sample(mgmc_handle* h, int nsteps, int64_t qoi_index, double* qoi_out);
/* qoi_index = MGMC_QOI_VECTOR records z = b^T x with the vector b of mgmc_set_qoi_vector (ABI 5). */
#define MGMC_QOI_VECTOR (-2)
/* The QoI vector b for qoi_index = MGMC_QOI_VECTOR: the radius > 0 measurement vector of
 * MeasuredOperator::measurement_vector (linear_operator/measured_operator.cc:92-171) that
 * driver_mgmc.cc:58-59, :76 dots with every sample.  nnz entries, rows strictly ascending (reference
 * vertex indices), values; nnz = 0 removes it.  The dot runs in the cycle graph in a fixed order
 * (4096-entry blocks, lane-strided sums, xor butterflies -- the low-rank dots' order): the state
 * stays in HBM.  Rebuilds the handle's graphs. */
int mgmc_set_qoi_vector(mgmc_handle* h, int64_t nnz, const int64_t* rows, const double* vals);
/* Enqueue nsteps cycles on the handle's stream without synchronising or copying back. */
int mgmc_sample_async(mgmc_handle* h, int nsteps, int64_t qoi_index);
int mgmc_synchronize(mgmc_handle* h);
/* out[0] = n, out[1] = mean, out[2] = M2 (sum of squared deviations) of the recorded QoI */
int mgmc_qoi_moments(mgmc_handle* h, double out[3]);
int mgmc_qoi_moments_chain(mgmc_handle* h, int chain, double out[3]);
int mgmc_reset_moments(mgmc_handle* h);
int mgmc_set_sample_index(mgmc_handle* h, uint64_t index);
int mgmc_get_sample_index(mgmc_handle* h, uint64_t* index);
/* Copy the QoI series recorded by the last mgmc_sample / mgmc_sample_async call (n values; waits
 * for the handle's stream).  With mgmc_sample_async on several handles this collects the series of
 * chains that ran concurrently (measure_convergence's batched chains, driver_mgmc.cc:188-314). */
int mgmc_get_series(mgmc_handle* h, double* out, size_t n);
int mgmc_get_series_chain(mgmc_handle* h, int chain, double* out, size_t n);
/* HIP stream (hipStream_t) the handle enqueues on */
int mgmc_get_stream(mgmc_handle* h, void** stream);

/* ---- pointwise field statistics (posterior_statistics, driver_mgmc.cc:118-171) ----
 * The sample mean and the pointwise variance of the whole field, accumulated on the device: while
 * enabled, every stride-th cycle of the handle (numbered 1, 2, ... from the enable / reset on; whichever
 * of mgmc_sample, mgmc_sample_async, mgmc_sample_timed* or mgmc_apply ran it) folds the level-0 state of
 * every chain, chains in the order 0 .. nchains-1, into one running (mean, M2) pair per vertex with the
 * Welford update of the QoI moments (mgmc_qoi_moments):
 *     delta = x - mean;  mean += delta / cnt;  M2 += delta * (x - mean),  cnt = states folded in + 1.
 * One mean and one M2 field per handle whatever nchains is (the chains sample the same distribution);
 * the reference's variance E[x^2] - mean^2 is M2 / nrecorded.  The fields stay in HBM (two vectors in the
 * fine level's padded layout) until mgmc_field_stats_get.  mgmc_set_state, mgmc_set_rhs and
 * mgmc_set_sample_index do not reset them; mgmc_set_lowrank and mgmc_set_qoi_vector keep them recording
 * (mgmc_set_lowrank resets them in the Rao-Blackwellised mode below).
 * Disabled (the default) the cycle and its graphs are those of a handle that never enabled them.
 * MGMC_E_INVALID: a NULL handle, stride < 1, a wrong n, get / reset while disabled; MGMC_E_NOMEM: the
 * fields could not be allocated (the handle stays disabled and otherwise intact). */
int mgmc_field_stats_enable(mgmc_handle* h, int stride);  /* stride >= 1; allocates + zeroes, rebuilds graphs;
                                                             on an enabled handle: reset with the new stride */
int mgmc_field_stats_disable(mgmc_handle* h);             /* frees, rebuilds graphs; no-op when disabled */
int mgmc_field_stats_reset(mgmc_handle* h);               /* zero fields and both counters; no graph rebuild */
int mgmc_field_stats_info(const mgmc_handle* h, int* enabled, int* stride, uint64_t* nrecorded);
                                                          /* nrecorded = states folded in (recorded cycles x nchains) */
int mgmc_field_stats_get(mgmc_handle* h, double* mean, double* m2, size_t n);
                                                          /* reference layout, n = ndof; either pointer may be NULL;
                                                             waits for the handle's stream */
/* Batch means: the Monte Carlo error of the mean field and the integrated autocorrelation time per vertex
 * (the reference's Statistics class estimates tau_int of one series from its autocovariances,
 * auxilliary/statistics.cc).  With batch length B, in recorded cycles r = 1, 2, ... since the enable / reset,
 * three more fields: bsum, the sum of the current batch, and bmean / bM2, the Welford mean and M2 of the
 * completed batches' means.  On recorded cycle r, besides the update above and with its chain order:
 *     bsum += x_c (c = 0 .. nchains-1);  if r % B == 0:  bm = bsum / (double)(B * nchains);  nb = r / B;
 *     d = bm - bmean;  bmean += d / nb;  bM2 += d * (bm - bmean);  bsum = +0.0.
 * A batch pools the chains of its B cycles.  With nb completed batches the standard error of the mean field
 * is sqrt(bM2 / (nb - 1) / nb) and tau = B * nchains * (bM2 / (nb - 1)) / (M2 / (nrecorded - 1)).  mean and
 * M2 are bitwise what they are without batching.  mgmc_field_stats_reset zeroes the three fields too and
 * drops a partial batch; mgmc_set_lowrank and mgmc_set_qoi_vector keep a partial batch; disable, info and
 * get work as above.  mgmc_field_stats_enable on a batched handle frees the three fields, rebuilds the
 * graphs and resets.  MGMC_E_INVALID: stride < 1, batch < 1, a wrong n, get_batch while batching is off;
 * MGMC_E_NOMEM: the fields could not be allocated (the handle stays as it was before the call). */
int mgmc_field_stats_enable_batched(mgmc_handle* h, int stride, int batch);
                                                          /* stride, batch >= 1; allocates + zeroes five fields,
                                                             rebuilds graphs; on a batched handle: reset with the
                                                             new stride and batch (same graphs) */
int mgmc_field_stats_batch_info(const mgmc_handle* h, int* batch, uint64_t* nbatches);
                                                          /* batch = 0 without batching or disabled; nbatches =
                                                             completed batches */
int mgmc_field_stats_get_batch(mgmc_handle* h, double* bmean, double* bm2, size_t n);
                                                          /* reference layout, n = ndof; either pointer may be NULL;
                                                             waits for the handle's stream */
/* Rao-Blackwellised statistics: for x ~ N(Q^{-1} f, Q^{-1}) the law of one vertex given the rest is
 * N(c_i, 1 / d_i) with d_i = Q_ii and c = x + D^{-1} (f - Q x), one Jacobi step applied to the sample.
 * E[c] = Q^{-1} f and diag Cov(c) = diag(Q^{-1}) - D^{-1}: mean(c) estimates the posterior mean and
 * 1 / d_i + var(c_i) the marginal variance, with only the smaller part of the variance left to Monte Carlo.
 * The identity needs only that every state has the target law, so it holds along a correlated chain.
 * In this mode the fields above (and the batch fields when batch >= 1) fold c in place of x, with the same
 * statements and chain order.  Per recorded state, at every interior vertex of level 0, in plain IEEE double:
 *     y_i = (Q x)_i   the bits of mgmc_operator_apply(h, 0, x) (the low-rank patch included),
 *     c_i = x_i + (f_i - y_i) / d_i,   f the vector of mgmc_set_rhs (+0.0 while it is all +0.0),
 *     d_i = a_ii, then for k = 0 .. m-1 ascending with B_ik stored:  d_i = d_i + (B_ik * B_ik) / Sigma_k.
 * Two paths compute the same bits: one fused z-marching kernel (one chain on a level that runs the z-sweep
 * with a constant stencil and no low-rank part), and everywhere else two passes (c into a buffer of
 * nchains x nstore doubles, then the plain fold).  MGMC_FIELD_COND_TWO_PASS takes the two passes where the
 * plan would fuse (how the two are compared).  disable, reset, info, get, batch_info and get_batch work as
 * above; mgmc_field_stats_enable / _enable_batched on a conditional handle switch back to plain statistics
 * (a reset).  mgmc_set_rhs, mgmc_set_state, mgmc_set_sample_index and mgmc_set_qoi_vector do not reset.
 * mgmc_set_lowrank changes d and Q: on a conditional handle it plans the path again, rebuilds d and RESETS
 * the statistics (n = 0, a partial batch dropped); if that needs an allocation which fails, the statistics
 * are left disabled and the call returns the error code.
 * MGMC_E_INVALID: a NULL handle, stride < 1, batch < 0, unknown flag bits, a wrong n, get_cond_precision while
 * the mode is off; MGMC_E_NOMEM: an allocation failed (the handle stays as it was before the call). */
#define MGMC_FIELD_COND_TWO_PASS 1u
int mgmc_field_stats_enable_cond(mgmc_handle* h, int stride, int batch, unsigned flags);
                                                          /* batch 0: no batch means.  On an enabled handle: a
                                                             reset, with a graph rebuild where the mode or the
                                                             instance changes */
int mgmc_field_stats_cond_info(const mgmc_handle* h, int* enabled, int* path);
                                                          /* path: 0 off / plain, 1 fused z-march, 2 two-pass */
int mgmc_field_stats_get_cond_precision(mgmc_handle* h, double* d, size_t n);
                                                          /* d in the reference layout, n = ndof */

/* ---- whole-field energy: x^T Q x and f^T x of the level-0 state, reduced on the device ----
 * Per chain two doubles:
 *     xqx = x^T A x + sum_k (B_k^T x)^2 / Sigma_k   (the second term once mgmc_set_lowrank ran),
 *     fx  = f^T x, f the vector of mgmc_set_rhs (never a low-rank-patched copy); +0.0 while f is all +0.0.
 * At stationarity E = xqx - 2 fx + f^T Q^{-1} f is chi-square with ndof degrees of freedom (mean ndof,
 * variance 2 ndof), and -xqx / 2 + fx is the Gaussian log-density of the state up to a constant.  The sums run
 * in a fixed order (no atomics): a chain's values do not depend on scheduling, on the
 * other chains of its batch or on MGMC_GRAPH_UNROLL.
 * mgmc_energy evaluates the current device state, nchains values each; nothing is recorded and the state is
 * untouched.  flags: MGMC_ENERGY_GENERAL takes the general kernel where the level would take the z-marching
 * one (the two agree to rounding, not bitwise). */
#define MGMC_ENERGY_GENERAL 1u
int mgmc_energy(mgmc_handle* h, unsigned flags, double* xqx, double* fx);
/* Recording: while enabled, every stride-th cycle of the handle (numbered 1, 2, ... from the enable / reset on,
 * whichever call ran it) appends (xqx, fx) of every chain to a series that keeps the first `capacity` records,
 * and folds E = xqx - 2 fx into per-chain Welford moments (the update of mgmc_qoi_moments), which keep counting
 * past the capacity.  The op sits after the QoI record and before the field statistics, in the timed cycle's
 * last segment; on a cycle that is not recorded its kernels leave at once.  mgmc_set_state, mgmc_set_rhs and
 * mgmc_set_sample_index do not reset the record; mgmc_set_lowrank and mgmc_set_qoi_vector keep it going.
 * Disabled (the default) the cycle and its graphs are those of a handle that never enabled it.
 * MGMC_E_INVALID: a NULL handle or pointer, stride < 1, capacity < 1, a chain out of range, get_series / moments
 * / reset while disabled, n beyond the records kept; MGMC_E_NOMEM: the buffers could not be allocated (the
 * handle stays as it was). */
int mgmc_energy_record_enable(mgmc_handle* h, int stride, int64_t capacity);
                                                          /* allocates + zeroes, rebuilds graphs; on an enabled
                                                             handle: a reset with the new stride (and capacity) */
int mgmc_energy_record_disable(mgmc_handle* h);           /* frees, rebuilds graphs; no-op when disabled */
int mgmc_energy_record_reset(mgmc_handle* h);             /* zero moments and both counters; no graph rebuild */
int mgmc_energy_record_info(const mgmc_handle* h, int* enabled, int* stride, uint64_t* ncycles, uint64_t* nrecorded);
                                                          /* cycles seen and cycles recorded since enable / reset */
int mgmc_energy_get_series(mgmc_handle* h, int chain, double* xqx, double* fx, size_t n);
                                                          /* the first n records, n <= min(nrecorded, capacity);
                                                             either pointer may be NULL; waits for the stream */
int mgmc_energy_moments(mgmc_handle* h, int chain, double out[3]);
                                                          /* (n, mean, M2) of E = xqx - 2 fx */

/* ---- QoI panel: K linear functionals z_k = b_k^T x per cycle and their joint statistics, on the device ----
 * The reference's Statistics (src/auxilliary/statistics.hh, statistics.cc) for a vector-valued observable: the
 * running average and covariance (statistics.cc:5-18, :41-51), the autocovariance over a window (:19-38, :54-62)
 * and from it tau_int (:65-80).  The natural panel of a posterior run is the predicted data B^T x at the
 * measurement sites plus the driver's QoI.
 * A panel is K <= 64 columns in CSC form, mgmc_set_lowrank's format: colptr[K + 1], rows = reference vertex
 * indices strictly ascending per column, vals.  A column that lists all N vertices is a dense column: dense
 * columns are read in groups that load each x once, and one whose values are all the same bits needs no value
 * array.  Column k is summed in mgmc_set_qoi_vector's order (4096-entry blocks, lane-strided, xor butterfly;
 * DESIGN.md section 3l), so it equals bit for bit what MGMC_QOI_VECTOR records for that vector.  K = 0 removes
 * the panel (and ends its recording).  mgmc_qoi_panel_set on a recording handle starts the records again.
 * mgmc_set_lowrank, mgmc_set_rhs, mgmc_set_state, mgmc_set_qoi_vector and mgmc_reset_moments do not touch the
 * panel or its records; the scalar QoI (series, moments) keeps its bits whether or not a panel records.
 * MGMC_E_INVALID (handle and installed panel unchanged): K outside [0, 64], colptr[0] != 0 or decreasing, an
 * empty column, rows out of range or not strictly ascending, a non-finite value.  MGMC_E_NOMEM: likewise unchanged.
 * A HIP failure while a recording handle takes its new panel leaves the new panel installed and the recording
 * off (the cycle without the op), as a failed mgmc_qoi_panel_record_enable does. */
int mgmc_qoi_panel_set(mgmc_handle* h, int K, const int64_t* colptr, const int64_t* rows, const double* vals);
int mgmc_qoi_panel_eval(mgmc_handle* h, double* out);     /* out[chain * K + k] = b_k^T x of the current state;
                                                             nothing is recorded */
/* Recording: while enabled, every stride-th cycle (numbered 1, 2, ... from the enable / reset on) records z of
 * every chain from an op right after the QoI record: the series keeps the first `capacity` records; the mean and
 * the co-moments C (cnt = n + 1; delta_k = z_k - mean_k; mean_k += delta_k / cnt; C[k][l] += delta_k (z_l -
 * mean_l), all deltas from the old means, all means updated first: the diagonal is mgmc_qoi_moments' M2 update)
 * and, per column, S[j] for lags j < window, 1 <= window <= 256 (statistics.cc:19-38: N_j = records - j,
 * S[j] = z_now z_lag if N_j == 1, else S[j] += (z_now z_lag - S[j]) / N_j) keep counting.  Disabled (the default)
 * the cycle and its graphs are those of a handle without a panel.  MGMC_E_INVALID: no panel installed, stride < 1,
 * window outside [1, 256], capacity < 1, a chain out of range, get_series / moments / autocov / reset while
 * disabled, n beyond the records kept; MGMC_E_NOMEM leaves the handle as it was. */
int mgmc_qoi_panel_record_enable(mgmc_handle* h, int stride, int window, int64_t capacity);
                                                          /* allocates + zeroes, rebuilds graphs; on an enabled handle
                                                             with the same window and capacity: a reset */
int mgmc_qoi_panel_record_disable(mgmc_handle* h);        /* frees, rebuilds graphs; no-op when disabled */
int mgmc_qoi_panel_record_reset(mgmc_handle* h);          /* zero moments, S and the counters; no graph rebuild */
int mgmc_qoi_panel_info(const mgmc_handle* h, int* K, int* enabled, int* stride, int* window, uint64_t* ncycles,
                        uint64_t* nrecorded);
int mgmc_qoi_panel_get_series(mgmc_handle* h, int chain, double* out, size_t n);
                                                          /* out[r * K + k], the first n records,
                                                             n <= min(nrecorded, capacity) */
int mgmc_qoi_panel_moments(mgmc_handle* h, int chain, double* count, double* mean, double* comoment);
                                                          /* mean[K]; comoment[K * K] = C, the upper triangle the
                                                             device keeps mirrored; the reference's covariance()
                                                             (statistics.cc:41-45) is C / (count - 1) */
int mgmc_qoi_panel_autocov(mgmc_handle* h, int chain, double* S, int* nlags);
                                                          /* S[k * window + j]; *nlags = min(window, nrecorded)
                                                             lags hold values; C_k(j) = S[k][j] - mean_k^2 */

/* ---- component entry points (host buffers, reference layout) used by the parity tests ---- */
/* y = Q_level x  (LinearOperator::apply; Q = A + B Sigma^{-1} B^T once mgmc_set_lowrank ran) */
int mgmc_operator_apply(mgmc_handle* h, int level, const double* x, double* y);
/* deterministic multicolour SOR sweeps (SORSmoother::apply, no noise; with the B_bar fix) */
int mgmc_smoother_apply(mgmc_handle* h, int level, int direction, int nsweeps,
                        const double* b, double* x);
/* The Smoother drop-ins (include/reference_adapter/hip_sor_smoother.hh), noise-free multicolour sweeps:
 * SORSmoother::apply exactly as the reference nests it -- nsmooth x (nsmooth sweeps of apply_sparse,
 * then the B_bar fix once), smoother/sor_smoother.cc:41-53 over :56-78 -- so nsmooth^2 sweeps;
 * 0 <= nsmooth <= 1024, else MGMC_E_INVALID ... */
int mgmc_sor_smoother_apply(mgmc_handle* h, int level, int direction, int nsmooth, const double* b, double* x);
/* ... and SSORSmoother::apply (smoother/ssor_smoother.cc:9-15): nsmooth x (forward sweep + fix,
 * backward sweep + fix) */
int mgmc_ssor_smoother_apply(mgmc_handle* h, int level, int nsmooth, const double* b, double* x);
/* one noisy multicolour SOR Gibbs sweep with explicit RNG counter (SORSampler::apply, nsmooth=1) */
int mgmc_sor_sampler_apply(mgmc_handle* h, int level, int direction, uint32_t sweep_tag,
                           uint64_t sample_index, const double* f, double* x);
/* coarse = R r  (restrict, level -> level+1) */
int mgmc_restrict(mgmc_handle* h, int level, const double* r, double* rc);
/* x += alpha * P xc  (prolongate_add, level+1 -> level) */
int mgmc_prolongate_add(mgmc_handle* h, int level, double alpha, const double* xc, double* x);
/* fc = R (f - Q x)  (fused residual + restriction of multigridmc_sampler.cc:118-120) */
int mgmc_residual_restrict(mgmc_handle* h, int level, const double* f, const double* x, double* fc);
/* ---- exact-statistics engine (linear_operator.hh:119-174 targets at any lattice size) ----
 * x = Q^{-1} b with the multigrid preconditioner of MultigridPreconditioner
 * (preconditioner/multigrid_preconditioner.cc:74-109): one deterministic cycle of the handle's
 * hierarchy from x = 0 (its smoothers without noise, with the B_bar fix).  The coarsest level is
 * solved exactly with its Cholesky factors, as the reference's CholeskySolver, when the handle has
 * them (coarse_solver Cholesky, or a coarsest level of at most 2048 unknowns); otherwise it takes
 * ncoarsesmooth SSOR sweeps.  method MGMC_SOLVER_LOOP is the
 * reference's LoopSolver (solver/loop_solver.cc:9-53, x -= M(Qx - b)); MGMC_SOLVER_CG wraps the
 * same (symmetric) cycle in conjugate gradients.  Stops when ||r||/||b|| < rtol and ||r|| < atol
 * (the reference's test) or after maxiter iterations; *iters and *rnorm report the outcome.
 * Host buffers, reference layout; the chain state is untouched. */
#define MGMC_SOLVER_LOOP 0
#define MGMC_SOLVER_CG 1
int mgmc_solve(mgmc_handle* h, int method, const double* b, double* x, double rtol, double atol, int maxiter,
               int* iters, double* rnorm);
/* n standard normals of pair ids [pair0, pair0+n/2) for (sweep_tag, sample_index):
 * out[2p] = cos branch, out[2p+1] = sin branch of the Box-Muller pair p */
int mgmc_normals(mgmc_handle* h, uint64_t pair0, size_t n, uint32_t sweep_tag, uint64_t sample_index,
                 double* out);

/* ---- timing hooks for the roofline measurement (bench.py) ----
 * Run `nsweeps` noisy fine-level (level 0) Gibbs sweeps on the device state, bracketed by
 * HIP events recorded on the handle's own stream; *ms = elapsed milliseconds. */
int mgmc_time_fine_sweeps(mgmc_handle* h, int nsweeps, float* ms);
/* Same as mgmc_sample_async + synchronize, but each cycle is replayed as three graph segments
 * [fine pre-sampler | coarse-grid correction | fine post-sampler + QoI record] with HIP events
 * recorded between them on the handle's stream.  *total_ms = first-to-last event time of the nsteps
 * cycles; *pre_ms / *post_ms = summed time of the fine-level (level 0) pre- / post-sampler segments
 * (the post segment holds the sweep with the fused prolongation and the ~4 us QoI record);
 * *npre / *npost = number of fine-level sweeps they contain. */
int mgmc_sample_timed(mgmc_handle* h, int nsteps, int64_t qoi_index, double* total_ms, double* pre_ms, int* npre,
                      double* post_ms, int* npost);
/* The same with the segments timed on every stride-th cycle only (and the last); the other cycles
 * replay the plain cycle graph (ABI 5).  *npre / *npost count the timed sweeps. */
int mgmc_sample_timed_stride(mgmc_handle* h, int nsteps, int stride, int64_t qoi_index, double* total_ms,
                             double* pre_ms, int* npre, double* post_ms, int* npost);

/* ---- multi-GPU: one chain per rank, RCCL over xGMI for the final QoI reduction ----
 * (the reference is single-process; this is the only collective of the path) */
#define MGMC_UNIQUE_ID_BYTES 128
/* rank 0 creates the id and ships it to the other ranks (any host channel) */
int mgmc_comm_unique_id(unsigned char out[MGMC_UNIQUE_ID_BYTES]);
int mgmc_comm_init(mgmc_handle* h, int nranks, int rank, const unsigned char id[MGMC_UNIQUE_ID_BYTES]);
/* all ranks: out[3*(r*nchains + c) .. +2] = (n, mean, M2) of chain c of rank r's handle (device-side
 * QoI moments; 3 * nranks * mgmc_nchains(h) doubles) */
int mgmc_comm_allgather_moments(mgmc_handle* h, double* out);
/* all ranks: *value <- max over ranks (used for the max-over-ranks benchmark time) */
int mgmc_comm_allreduce_max(mgmc_handle* h, double* value);
/* device-side barrier over the communicator, followed by a stream synchronisation */
int mgmc_comm_barrier(mgmc_handle* h);
int mgmc_comm_destroy(mgmc_handle* h);
/* what the communicator really spans: *rccl_ranks = ncclCommCount (0 without a communicator),
 * *rccl_rank = ncclCommUserRank (-1 without one), *pci_bus_id = PCI bus id of the handle's device
 * (ranks that report the same id share one GPU, where RCCL cannot run). */
int mgmc_comm_info(const mgmc_handle* h, int* rccl_ranks, int* rccl_rank, int* pci_bus_id);

#ifdef __cplusplus
}
#endif

#endif /* MGMC_H */
