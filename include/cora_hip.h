/*
 * cora_hip.h -- C ABI of the MI355X-native CORA solver core (libcora_hip.so).
 *
 * The reference (MarineRoboticsGroup/cora) has no FFI seam: its hot path is the
 * set of `const` methods of `CORA::Problem` that `solveCORA` wraps in
 * std::function closures for the TNT optimizer (src/CORA.cpp:52-92,119-122)
 * and for LOBPCG (src/CORA_utils.cpp:83).  Each entry point below replaces one
 * of those methods; the citation is the reference file:line it stands in for.
 *
 * Conventions
 *   - every call returns a cora_status (0 = ok); no exception crosses the ABI;
 *     cora_last_error() gives the message (replaces MatrixShapeException /
 *     std::runtime_error, include/CORA/CORA_types.h:23-39).
 *   - host matrices are column-major double with an explicit leading dimension
 *     (zero-copy from Eigen::MatrixXd::data(), include/CORA/CORA_types.h:48);
 *     Q is row-major CSR with int32 indices (Eigen::SparseMatrix<double,
 *     RowMajor,int> outerIndexPtr/innerIndexPtr/valuePtr after makeCompressed(),
 *     include/CORA/CORA_types.h:70).
 *   - variable layout (include/CORA/CORA_problem.h:151-157): rows [0,d*n) are n
 *     stacked d x p Stiefel blocks, rows [d*n, d*n+r) are r unit rows, rows
 *     [d*n+r, N) are the n+l translations;  N = n(d+1) + l + r.
 *   - the caller owns host buffers; the library owns all device memory tied to
 *     the handle.  One handle = one HIP stream; a handle is not thread-safe,
 *     independent handles are.
 *   - `_dev` entry points take DEVICE pointers to the library's resident layout:
 *     row-major  rows x ld  doubles with ld = cora_ld(ctx) = cora_ld_for(k) = the number of
 *     columns k itself for every k in 2..24 (no padding columns; ld = 2 for k = 1) -- ask, do not
 *     assume -- and rows = cora_rows(ctx) in the library's internal row order (a permutation even
 *     on one GPU: cora_row_map).  Use cora_upload / cora_download to convert from / to the host layout.
 *   - there is no CPU fallback: every compute entry point fails with
 *     CORA_ERR_HIP when no gfx950 device is usable.
 */
#ifndef CORA_HIP_H_
#define CORA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cora_ctx cora_ctx;

typedef enum {
  CORA_OK = 0,
  CORA_ERR_SHAPE = 1,     /* checkMatrixShape failure */
  CORA_ERR_NOT_READY = 2, /* set_point / precond_setup missing (checkUpToDate) */
  CORA_ERR_NAN = 3,       /* NaN guard, src/CORA_problem.cpp:898-901 */
  CORA_ERR_HIP = 4,
  CORA_ERR_ARG = 5,
  CORA_ERR_NOMEM = 6
} cora_status;

/* Preconditioner kinds, include/CORA/CORA_types.h:77 */
typedef enum {
  CORA_PRECOND_NONE = 0,
  CORA_PRECOND_JACOBI = 1,
  CORA_PRECOND_BLOCK_CHOLESKY = 2,
  CORA_PRECOND_REGULARIZED_CHOLESKY = 3
} cora_precond_kind;

/* ---------------------------------------------------------------- handle */

/* Builds a device-resident problem from the assembled data matrix
 * (`Problem::data_matrix_` after updateProblemData(), src/CORA_problem.cpp:
 * 500-510, 625-712).  n_trans = n_poses + n_landmarks. */
int cora_ctx_create(int device, int d, int n_poses, int n_ranges, int n_trans,
                    const int32_t *rowptr, const int32_t *colidx,
                    const double *vals, cora_ctx **out);

/* Same, but the handle owns only the rows of partition `rank` of `world`
 * (pose-aligned, nnz-balanced row partition).  All ranks must pass
 * the same full matrix.  world == 1 is identical to cora_ctx_create. */
int cora_ctx_create_part(int device, int d, int n_poses, int n_ranges,
                         int n_trans, const int32_t *rowptr,
                         const int32_t *colidx, const double *vals, int rank,
                         int world, cora_ctx **out);
/* The same with options.  CORA_PART_WHOLE_LONG_ROWS: keep the long (landmark) rows whole on their owner, as rounds 1-2
 * did -- the owner then reads ~10^4 remote rows of X per landmark (cora_remote_rows), but a handle WITHOUT communication
 * computes complete rows of its shard by itself (the caller keeps the remote rows current).  Default (flags = 0): the
 * long rows are distributed (cora_long_rows) and need the all-reduce of cora_comm_create_* / cora_set_comm. */
#define CORA_PART_WHOLE_LONG_ROWS 1u
int cora_ctx_create_part_opts(int device, int d, int n_poses, int n_ranges, int n_trans, const int32_t *rowptr,
                              const int32_t *colidx, const double *vals, int rank, int world, unsigned flags,
                              cora_ctx **out);

void cora_ctx_destroy(cora_ctx *ctx);

/* Message of the last failed call on `ctx` (ctx may be NULL for create). */
const char *cora_last_error(const cora_ctx *ctx);

/* Problem::setRank / incrementRank, include/CORA/CORA_problem.h:327-334.
 * Invalidates the current point and the preconditioner state. */
int cora_set_rank(cora_ctx *ctx, int p);
int cora_get_rank(const cora_ctx *ctx);

/* Use an externally created hipStream_t (e.g. torch's current stream) for everything the handle enqueues from now on.
 * The contract, pinned on the GPU by tests/test_gpu_streams.py:
 *   - the call first waits on the host for the handle's old stream, so work pending there has finished when it returns and
 *     a later call on the new stream may read its results; the handle's own stream (the one it was created with) is
 *     destroyed then, a caller's stream never is -- not by a later cora_set_stream, not by cora_ctx_destroy, which waits
 *     for the handle's pending work and leaves the stream usable.  The caller keeps the stream alive while the handle
 *     uses it.  On a handle without a device: CORA_ERR_HIP.
 *   - hip_stream = NULL, the legacy default stream 0, is allowed (it is what torch's default current stream is).
 *   - ordering: whatever a call enqueues is ordered AFTER the work already on that stream when the call is made (the
 *     caller's own kernels and copies included: operands may still be in the making, with no host wait) and BEFORE the work
 *     the caller enqueues after the call returns.  That covers the handle's state: the current point, a kept trial product,
 *     scratch, and vectors of cora_dev_alloc (zeroed on the stream, also when recycled) -- all survive a move.
 *   - which calls wait on the host: those that return values to the host -- cora_dots_dev, cora_dot_dev, cora_gram_dev,
 *     cora_gram_batch_dev, cora_objective_dev, cora_tnt_trial_dev, cora_tnt_accept_dev, cora_stpcg_dev and its warm form,
 *     cora_set_point_dev (the cost), cora_gnc_weights_dev, the evaluation calls and the initialisers, cora_upload,
 *     cora_download, cora_timer_stop_ms, cora_sync -- return when the stream has reached them, so they also wait for the
 *     caller's earlier work on it.  Calls that only write device vectors (products, row operations, the projected
 *     preconditioner, cora_copy_dev, cora_fill_random_dev) return as soon as their work is enqueued.
 *   - not supported: the opt-in graph replay of the inner solve (CORA_STPCG_GRAPH) on stream 0 -- a stream capture on the
 *     legacy default stream is not legal HIP.  Use a created stream with it. */
int cora_set_stream(cora_ctx *ctx, void *hip_stream);

/* Layout queries for the `_dev` API. */
int cora_ld(const cora_ctx *ctx);            /* row stride (doubles) */
int cora_ld_for(int k);                      /* row stride used for k columns */
int64_t cora_rows(const cora_ctx *ctx);      /* rows of a resident vector */
int64_t cora_shard_rows(const cora_ctx *ctx);  /* rows owned per rank (padded) */
int64_t cora_shard_begin(const cora_ctx *ctx); /* first owned internal row */
int64_t cora_nnz(const cora_ctx *ctx);
int64_t cora_dim(const cora_ctx *ctx);       /* N */
/* Row permutation: internal row of API row i (length N, int32). */
int cora_row_map(const cora_ctx *ctx, int32_t *api_to_internal);
/* Partitioned handles: the internal rows OUTSIDE this rank's shard that its rows of Q reference, ascending
 * (the halo of the pose chain plus whatever couples to remote landmarks).  Only these rows of an operand
 * have to arrive before a product, so the exchange step can all-gather them instead of whole shards
 * (cora_amd/dist.py).  rows may be NULL to query the count. */
int cora_remote_rows(const cora_ctx *ctx, int32_t *rows, int64_t *count);
/* Partitioned handles: the DISTRIBUTED long rows (API row indices, the same list on every rank; empty on one GPU).
 * The columns of such a row -- a landmark's translation row -- span every rank, so every rank multiplies the part of
 * the row on the columns it owns and the partial sums are added over the ranks after the product (by the library with
 * cora_comm_create_* / cora_set_comm); the row's owner then holds the result.  A rank therefore asks for no remote rows
 * of X on behalf of these rows: cora_remote_rows() is the chain halo plus the landmarks' own rows. */
int cora_long_rows(const cora_ctx *ctx, int32_t *api_rows, int64_t *count);

/* Statistics of the device format: [0] slices, [1] padded nnz stored in
 * slices, [2] nnz in long rows, [3] long rows, [4] long-row chunks,
 * [5] local rows, [6] local nnz, [7] max slice width. */
int cora_format_stats(const cora_ctx *ctx, int64_t stats[8]);

/* Bytes of the device format of this handle's share of Q -- what ONE product reads of the matrix whatever the operand:
 * [0] values, [1] column indices and per-lane descriptors, [2] slice / chunk descriptors, row lists and head blocks,
 * [3] their sum.  (The reference's CSR, src/CORA_problem.cpp:742-746, is 12 nnz + 4 (N + 1) bytes.) */
int cora_format_bytes(const cora_ctx *ctx, int64_t bytes[4]);

/* ------------------------------------------- host-pointer operator API */

/* Problem::dataMatrixProduct (Explicit), src/CORA_problem.cpp:742-746.
 * X, out: N x k. */
int cora_data_matrix_product(cora_ctx *ctx, const double *X, int ldx, int k,
                             double *out, int ldo);

/* Problem::evaluateObjective, src/CORA_problem.cpp:759-762. Y: N x p. */
int cora_evaluate_objective(cora_ctx *ctx, const double *Y, int ldy, double *f);

/* Problem::Euclidean_gradient, src/CORA_problem.cpp:764-770. */
int cora_euclidean_gradient(cora_ctx *ctx, const double *Y, int ldy,
                            double *out, int ldo);

/* Problem::Riemannian_gradient(Y), src/CORA_problem.cpp:772-780. */
int cora_riemannian_gradient(cora_ctx *ctx, const double *Y, int ldy,
                             double *out, int ldo);

/* Problem::tangent_space_projection(Y, Ydot), src/CORA_problem.cpp:782-820. */
int cora_tangent_space_projection(cora_ctx *ctx, const double *Y, int ldy,
                                  const double *V, int ldv, double *out,
                                  int ldo);

/* Problem::Riemannian_Hessian_vector_product(Y, nablaF_Y, dotY),
 * src/CORA_problem.cpp:822-867. */
int cora_riemannian_hessian_vector_product(cora_ctx *ctx, const double *Y,
                                           int ldy, const double *nablaF_Y,
                                           int ldg, const double *dotY,
                                           int ldd, double *out, int ldo);

/* Problem::projectToManifold, src/CORA_problem.cpp:905-934: polar factor of every pose block, unit range rows,
 * translation rows unchanged.  This call, cora_retract, cora_retract_dev and cora_project_to_manifold_dev run the same
 * kernel and return the same bits for the same input.
 * SCALE.  Any finite non-zero scale is accepted: a block (a range row) whose largest |entry| lies outside
 * [2^-250, 2^250] is multiplied by an exact power of two first; ordinary input takes the same arithmetic as before.
 * RANK-DEFICIENT pose blocks are NOT completed to an orthonormal frame as the reference's SVD route does: a zero block
 * returns zero, a zero row stays zero next to orthonormal others, and of two identical rows one comes back without
 * meaning (zero or a normalised rounding residue).  A zero range row stays zero.  The output is finite in every case. */
int cora_project_to_manifold(cora_ctx *ctx, const double *A, int lda,
                             double *out, int ldo);

/* Problem::retract(Y, V), src/CORA_problem.cpp:936-938. */
int cora_retract(cora_ctx *ctx, const double *Y, int ldy, const double *V,
                 int ldv, double *out, int ldo);

/* Problem::updatePreconditioner, src/CORA_problem.cpp:512-623.
 *  JACOBI: diag(Q)^-1 (:616-618), built on device.
 *  *_CHOLESKY: `factor` is an opaque host factorization installed with
 *  cora_precond_set_cholesky (host LL^T + device triangular solves). */
int cora_precond_setup(cora_ctx *ctx, int kind);

/* Install a sparse Cholesky factor L (CSC, int32, diagonal first in each
 * column) of P (Q + lambda I)[0:m,0:m] P^T with m = N or N-1
 * (pin_last_translation, src/CORA_problem.cpp:602-609); perm is new->old. */
int cora_precond_set_cholesky(cora_ctx *ctx, int m, const int32_t *Lp,
                              const int32_t *Li, const double *Lx,
                              const int32_t *perm);

/* Device solve plan of the installed factor: [0] stages (a solve is 4*stages - 2 sparse products),
 * [1] entries of the explicit block inverses, [2] nnz(L), [3] rows of the last stage. */
int cora_precond_stats(const cora_ctx *ctx, int64_t stats[4]);
/* Entries the preconditioner's device solve plan stores: [0] / [1] the last stage's forward / backward product,
 * [2] / [3] entry slots of the substitution blocks' forward / backward sweep (null padding included), [4] substitution
 * blocks, [5] aux rows.  (Measurement: bench.py's bytes per STPCG iteration.) */
int cora_precond_entries(const cora_ctx *ctx, int64_t s[6]);

/* Translation-implicit formulation (Formulation::Implicit, src/CORA_problem.cpp:714-753):
 *   dataMatrixProduct(Y) = Qmain Y - B L^-1 B^T Y,  L L^T = Q33[0:nt-1, 0:nt-1].
 * cora_implicit_set_cholesky installs that factor (CSC, diagonal first per column; perm is
 * new -> old index inside the translation block); cora_set_formulation(ctx, 1) then switches every
 * product (spmm / objective / set_point / hvp) to the implicit operator.  Vectors keep N rows:
 * translation rows of inputs are ignored, translation rows of outputs are zero (callers pass and
 * read the leading d*n + r rows).  cora_certificate_product* always applies the explicit S, like
 * the reference's certify_solution (:1054-1058).  cora_translation_explicit_dev =
 * getTranslationExplicitSolution (:1168-1197): out = [Y; -L^-1 B^T Y; 0].
 * Partitioned handle: every rank installs the WHOLE factor; the two products of an implicit product are partitioned
 * products and the solve between them is replicated (the right-hand side is all-gathered, cora_allgather_fn). */
int cora_implicit_set_cholesky(cora_ctx *ctx, int m, const int32_t *Lp, const int32_t *Li,
                               const double *Lx, const int32_t *perm);
int cora_set_formulation(cora_ctx *ctx, int implicit);
int cora_translation_explicit_dev(cora_ctx *ctx, const double *dY, int k, double *dOut);

/* Problem::precondition(V), src/CORA_problem.cpp:869-903 (no projection;
 * last row zeroed when the factor has N-1 rows, src/CORA_preconditioners.cpp:
 * 78-79; NaN guard -> CORA_ERR_NAN). */
int cora_precondition(cora_ctx *ctx, const double *V, int ldv, double *out,
                      int ldo);

/* Problem::compute_Lambda_blocks(Y), src/CORA_problem.cpp:1105-1131.
 * stiefel: d x (d*n) column-major (ld = d); oblique: r. */
int cora_compute_lambda_blocks(cora_ctx *ctx, const double *Y, int ldy,
                               double *stiefel, double *oblique);

/* Certificate operator  out = (Q - Lambda(Y)) X  for an N x k block, i.e.
 * Problem::get_certificate_matrix(Y) (src/CORA_problem.cpp:1162-1166) applied
 * as the LOBPCG operator (src/CORA_utils.cpp:83).  Uses the Lambda of the
 * current point (cora_set_point). */
int cora_certificate_product(cora_ctx *ctx, const double *X, int ldx, int k,
                             double *out, int ldo);

/* Metric closure <V1, V2> = trace(V1^T V2), src/CORA.cpp:119-122. */
int cora_inner_product(cora_ctx *ctx, const double *A, int lda,
                       const double *B, int ldb, int k, double *out);

/* --------------------------------------------- resident (device) API */

/* Allocate / free a resident vector of cora_rows(ctx) x cora_ld_for(k). */
int cora_dev_alloc(cora_ctx *ctx, int k, double **dptr);
int cora_dev_free(cora_ctx *ctx, double *dptr);

/* Host column-major N x k  <->  resident row-major layout. */
int cora_upload(cora_ctx *ctx, const double *host, int ld, int k, double *dptr);
int cora_download(cora_ctx *ctx, const double *dptr, int k, double *host,
                  int ld);

/* Make Y the current point: caches Y, nablaF = Q Y, f = 1/2 <Y, Q Y>,
 * Lambda(Y) and grad = Proj_Y(nablaF) on the device (the QuadraticModel
 * closure of src/CORA.cpp:58-75 + the objective of :52-55 in one pass). */
int cora_set_point(cora_ctx *ctx, const double *Y, int ldy);
int cora_set_point_dev(cora_ctx *ctx, const double *dY);

/* f(Y) = 1/2 <Y, Q Y> for a resident Y WITHOUT changing the current point (the
 * Objective closure of src/CORA.cpp:52-55, used for trial points). Synchronises. */
int cora_objective_dev(cora_ctx *ctx, const double *dY, double *f);

/* One trust-region trial step of Optimization::Riemannian::TNT (the solver src/CORA.cpp:139-140 calls; its sources
 * are a dependency absent from the reference tree) in ONE wait: dHs = Hess(s), dXprop = Retr_Y(s), and
 * out = { <grad, s>, <s, Hess s>, <s, s>, f(Xprop) }.  Same kernels and values as cora_hvp_dev + cora_dots_dev +
 * cora_retract_dev + cora_objective_dev; the product Q Xprop stays on the handle for cora_tnt_accept_dev. */
int cora_tnt_trial_dev(cora_ctx *ctx, const double *dS, double *dHs, double *dXprop, double out[4]);
/* Make dX the current point (cora_set_point_dev), dPg = precondition(grad) projected, and
 * out = { f, <grad, grad>, <Pg, Pg>, <grad, Pg> } in one wait.  When dX is the vector the last cora_tnt_trial_dev
 * filled (one GPU), Q X is taken from that call: the pointer cora_point_egrad_dev returns changes.
 * CONTRACT of the reuse: the kept product belongs to the CONTENTS dXprop had when cora_tnt_trial_dev returned.  Every entry
 * point of this header that writes a caller's vector (cora_upload, the outputs of every *_dev operation, cora_stpcg_*_dev's
 * work vectors) or can hand its address out again (cora_dev_free / cora_dev_alloc) drops it when that vector is dXprop, and
 * the accept then forms Q X again.  A write the library cannot see (the caller's own kernel, hipMemcpy into dXprop) must be
 * followed by cora_set_point_dev instead of this call. */
int cora_tnt_accept_dev(cora_ctx *ctx, const double *dX, double *dPg, double out[4]);

/* f at the current point (local shard contribution when partitioned). */
int cora_point_cost(cora_ctx *ctx, double *f);
/* Device pointers to the cached point data (valid until the next point is set: cora_set_point*, cora_tnt_accept_dev). */
const double *cora_point_Y_dev(const cora_ctx *ctx);
const double *cora_point_egrad_dev(const cora_ctx *ctx);
const double *cora_point_rgrad_dev(const cora_ctx *ctx);

/* out = Q X (k columns; ld = cora_ld_for(k)). */
int cora_spmm_dev(cora_ctx *ctx, const double *dX, int k, double *dOut);
/* out = Proj_Y((Q - Lambda) X) at the current point: the Hessian-vector
 * product of src/CORA_problem.cpp:822-867 with cached Lambda. */
int cora_hvp_dev(cora_ctx *ctx, const double *dX, double *dOut);
/* out = (Q - Lambda) X, k columns. */
int cora_certificate_product_dev(cora_ctx *ctx, const double *dX, int k,
                                 double *dOut);
/* out = Proj_Y(V) at the current point. */
int cora_tangent_space_projection_dev(cora_ctx *ctx, const double *dV,
                                      double *dOut);
/* out = Proj_Y(precondition(V)): the `precon` closure, src/CORA.cpp:86-92. */
int cora_precondition_projected_dev(cora_ctx *ctx, const double *dV,
                                    double *dOut);
/* out = projectToManifold(Y + alpha V) with Y the current point. */
int cora_retract_dev(cora_ctx *ctx, const double *dV, double alpha,
                     double *dOut);
int cora_project_to_manifold_dev(cora_ctx *ctx, const double *dA, double *dOut);
/* Vector ops on resident N x p vectors (local shard rows when partitioned). */
int cora_axpby_dev(cora_ctx *ctx, double a, const double *dX, double b,
                   double *dY); /* Y = a X + b Y */
/* Y1 += a1 X1 and Y2 += a2 X2 in one launch: the step and residual updates of an STPCG iteration
 * (s += alpha p, r += alpha Hp inside Optimization::Riemannian::TNT, called from src/CORA.cpp:139). */
int cora_axpy2_dev(cora_ctx *ctx, double a1, const double *dX1, double *dY1, double a2, const double *dX2,
                   double *dY2);
/* The inner solver of the trust-region method -- Steihaug-Toint truncated preconditioned CG on
 *   min <grad, s> + 1/2 <s, Hess s>   subject to ||s||_M <= Delta
 * (Optimization::Riemannian::TNT's STPCG, reached from src/CORA.cpp:139-140 with the closures of
 * :58-92,119-122) -- run entirely on the device at the current point: Hess = cora_hvp_dev, M^-1 =
 * cora_precondition_projected_dev, inner products and the scalar recurrences in device memory.  Stops
 * when ||r|| <= ||r0|| min(kappa_fgr, ||r0||^theta), on negative curvature or the trust-region boundary
 * (step to the boundary), or after max_iters Hessian-vector products.  dS receives the step; dR, dV,
 * dP, dHp are work vectors (cora_dev_alloc(ctx, p, ..)).  iters = Hessian-vector products used,
 * step_M_norm = ||s||_M. */
int cora_stpcg_dev(cora_ctx *ctx, const double *dGrad, double Delta, double kappa_fgr, double theta,
                   int max_iters, double *dS, double *dR, double *dV, double *dP, double *dHp, int *iters,
                   double *step_M_norm);
/* The same solve started from a preconditioned gradient the caller already holds: dPg = M^-1 grad (projected, i.e.
 * cora_precondition_projected_dev(grad)), g_g = <grad, grad>, g_Pg = <grad, dPg>.  The trust-region loop computes all
 * three for its stopping tests at every accepted point, so the inner solve needs neither a preconditioner apply nor a
 * reduction of its own to start.  dPg is read only. */
int cora_stpcg_warm_dev(cora_ctx *ctx, const double *dGrad, const double *dPg, double g_g, double g_Pg, double Delta,
                        double kappa_fgr, double theta, int max_iters, double *dS, double *dR, double *dV, double *dP,
                        double *dHp, int *iters, double *step_M_norm);
/* Same for vectors allocated with k columns (cora_dev_alloc(ctx, k, ..)). */
int cora_axpby_cols_dev(cora_ctx *ctx, int k, double a, const double *dX, double b, double *dY);
/* dX (k columns, resident layout) = numbers in (-1, 1) that depend on (seed, variable, column) only -- the same block on
 * every partition of the problem --: a start block for the eigensolver made on the device (the norm estimate of src/CORA_problem.cpp:556-578 starts from Matrix::Random). */
int cora_fill_random_dev(cora_ctx *ctx, int k, unsigned long long seed, double *dX);
int cora_copy_dev(cora_ctx *ctx, const double *dX, int k, double *dY);
int cora_dot_dev(cora_ctx *ctx, const double *dA, const double *dB, int k,
                 double *out); /* synchronises the stream */
/* Up to 4 inner products in one pass / one synchronisation. */
int cora_dots_dev(cora_ctx *ctx, int count, const double *const *dA,
                  const double *const *dB, double *out);

/* Tall-skinny block operations for the eigensolver (Rayleigh-Ritz of LOBPCG, which the reference
 * takes from libs/Optimization: src/CORA_utils.cpp:113-119).  Blocks are resident vectors with ka /
 * kb <= 24 columns.
 *   gram:    G = A^T B -> host, column-major ka x kb (synchronises)
 *   combine: Out = sum_{i<n} X_i C_i, C_i host column-major k_i x kout (ld k_i), n <= 4;
 *            Out must not alias an input. */
int cora_gram_dev(cora_ctx *ctx, const double *dA, int ka, const double *dB, int kb, double *G);
/* n <= 16 products G[e] = A_e^T B_e with one synchronisation: the numbers of n cora_gram_dev calls (same kernel, one
 * piece of the reduction buffer each) -- the twelve Gram blocks of one Rayleigh-Ritz step. */
int cora_gram_batch_dev(cora_ctx *ctx, int n, const double *const *dA, const int *ka, const double *const *dB,
                        const int *kb, double *const *G);
int cora_combine_dev(cora_ctx *ctx, int n, const double *const *dX, const int *k, const double *const *C,
                     int kout, double *dOut);

/* ------------------------------------------------ per-measurement residuals
 *
 * An EXTENSION beyond the reference, whose Problem keeps the measurements only until fillDataMatrix() has summed them
 * into Q (src/CORA_problem.cpp:625-712) and can therefore report one number, f = 1/2 <X, Q X>.  The handle keeps a table
 * of the measurements themselves and evaluates every one of them at a resident X in one gather pass.  With X_a the
 * d x k block of pose a's rotation rows, x_t(s) the translation row of symbol s and x_rho(m) the unit row of range m:
 *   edge  (a, b, R, t, kappa, tau) -- relative poses, pose priors (a = the origin pose), pose-landmark measurements and
 *         landmark priors (a = the origin pose, t = the prior position), in the row order of fillRelPoseSubmatrices
 *         (src/CORA_problem.cpp:149-295):
 *             rot   = kappa |X_b - R^T X_a|_F^2          (0, and R not read, when b has no rotation: second row -1)
 *             trans = tau |x_t(b) - x_t(a) - sum_c t_c X_a[c, :]|^2
 *   range (a, b, r, omega):  res = omega |x_t(b) - x_t(a) + r x_rho(m)|^2
 * NO factor 1/2 goes into the per-measurement values.  With Q as fillDataMatrix() builds it,
 *   1/2 (sum rot + sum trans + sum res) = f(X)  for ANY X (on the manifold or not; R is orthogonal),
 * and at a good solution the residual form keeps the digits the quadratic form cancels.
 *
 * cora_set_measurements: the table, in API rows (variable layout above).
 *   edge_rows  [n_edges][4] int32: first rotation row of a, first rotation row of b or -1, translation row of a, of b
 *   edge_data  [n_edges][d*d + d + 2]: R row-major, t, kappa, tau
 *   range_rows [n_ranges][3]: range row, translation row of a, translation row of b
 *   range_data [n_ranges][2]: r, omega
 * CORA_ERR_ARG with a message: a rotation row that is not a multiple of d below d*n, a range row outside [d*n, d*n + r),
 * a translation row outside [d*n + r, N), non-finite data, a partitioned handle (world > 1: not supported yet).  Every
 * row is translated to the internal order once (cora_row_map); a pose's rotation block is kept by its first internal
 * row, and a layout in which its d rows are not consecutive is an error, not a wrong number.  The device copy is
 * structure-of-arrays ([field][measurement]) in the order given -- keep Problem order: odometry edges then touch
 * neighbouring internal rows.  A second call replaces the table.  Works on a plan-only handle (device < 0): everything
 * except the upload.
 * cora_measurement_counts: out = { edges, ranges } of the current table (0, 0 without one).
 * cora_measurement_residuals_dev: dX is a resident vector of k columns, 1 <= k <= 24 (ld = cora_ld_for(k)), k independent
 *   of the handle's rank as in cora_spmm_dev (the relaxed and the rounded solution are both served).  edge_rot,
 *   edge_trans [n_edges] and range_res [n_ranges] are HOST pointers, each may be NULL; sums[3] = { sum rot, sum trans,
 *   sum res } (may be NULL).  Synchronises.  CORA_ERR_NOT_READY before a table is set.  A measurement's value has the
 *   same bits wherever it stands in the table, and two calls give the same bits (fixed summation orders, no atomics).
 * cora_measurement_residuals: the host-pointer form (X: N x k column-major, uploaded first). */
int cora_set_measurements(cora_ctx *ctx, int64_t n_edges, const int32_t *edge_rows, const double *edge_data,
                          int64_t n_ranges, const int32_t *range_rows, const double *range_data);
int cora_measurement_counts(const cora_ctx *ctx, int64_t out[2]);
int cora_measurement_residuals_dev(cora_ctx *ctx, const double *dX, int k, double *edge_rot, double *edge_trans,
                                   double *range_res, double sums[3]);
int cora_measurement_residuals(cora_ctx *ctx, const double *X, int ldx, int k, double *edge_rot, double *edge_trans,
                               double *range_res, double sums[3]);
/* Test hook: the TRANSLATED table executed on the host on X permuted into the internal order (the analogue of
 * cora_debug_format_spmm_host): table building and row translation can be tested where no GPU exists.  Never used by
 * any compute entry point. */
int cora_debug_measurement_residuals_host(cora_ctx *ctx, const double *X, int ldx, int k, double *edge_rot,
                                          double *edge_trans, double *range_res, double sums[3]);

/* ---- New VALUES of Q on a live handle (same sparsity pattern) ----------------------------------------------------------
 * Re-weighting measurements changes numbers of Q, never its pattern, and everything a handle derives from the pattern --
 * the row order, the slices, the column indices, the partition, the exchange lists -- stays.  These calls move the
 * values only: a gather pass per value array through a SOURCE MAP (for every stored value, the CSR position it comes
 * from).  The stored bits are exactly the ones a handle created from the same CSR holds.
 *
 * cora_values_map_build   builds the map from (rowptr, colidx), which must be the pattern the handle was created with:
 *                         the structure is recomputed and compared with the handle's own (CORA_ERR_ARG when it
 *                         differs), and a 64-bit hash of the pattern is kept and checked by every later update.  Lazy:
 *                         a handle that is never updated pays nothing; cora_update_values builds the map on its first
 *                         call.  Costs about one format build and 4 bytes per stored value (host and device), plus a
 *                         device staging buffer of nnz doubles.
 * cora_update_values      vals: the new values on the HOST, CSR order, with the pattern passed again.  Also works on a
 *                         plan-only handle (device < 0): the host format is refreshed through the same map.
 * cora_update_values_dev  d_vals: nnz doubles in CSR order ON THE DEVICE (cora_assemble_values_dev below forms Q(w)
 *                         there; any other values are the caller's).  Needs the map
 *                         (CORA_ERR_NOT_READY before).  The host copy of the format is NOT refreshed:
 *                         cora_debug_format_spmm_host answers CORA_ERR_NOT_READY until the next cora_update_values.
 * Partitioned handles: every rank passes the WHOLE matrix, as to cora_ctx_create_part; the map is per rank and the call
 * is not collective (but the ranks' products only agree again once every rank has been updated).
 *
 * SYMMETRY.  A pose slice in the chain layout stores Q(rot(P), t_P), the couplings of neighbouring poses and
 * Q(t_P, t_{P+1}) ONCE and reads the transposed entries from there; creation checks that the two copies are equal and
 * falls back to a plain slice otherwise.  An update cannot change the layout, so it REQUIRES the same equalities of the
 * new values (compared as numbers, entry against entry) and refuses values that break one.  A symmetric Q -- what
 * CORA::Problem assembles -- always passes.
 * DUPLICATES.  A row that repeats a column index is accepted by creation (the entries are summed) but has no source map:
 * both map-building calls refuse it with CORA_ERR_ARG.  Merge duplicates before creating a handle that is to be updated.
 *
 * STATE after a successful update -- that of a handle freshly created from the new values, at the same rank:
 *   gone     the current point and a kept trial product (CORA_ERR_NOT_READY until the next cora_set_point*), the
 *            preconditioner (cora_precond_setup again; Jacobi then uses the new diagonal; an installed Cholesky factor
 *            belongs to the old values and must be installed again), the implicit factor; the formulation is explicit.
 *   survives the rank, the stream, every vector of cora_dev_alloc with its contents, scratch memory, the communicator,
 *            the aux factor (cora_aux_set_cholesky: the caller's own matrix) and the measurement table -- whose kappa,
 *            tau and omega describe the OLD weights until the caller sets a new table (cora_set_measurements).
 * ERRORS.  CORA_ERR_ARG: another pattern or number of nonzeros, a broken equality, a value that is not finite, a null
 * pointer, duplicates.  Values are checked (on the device by a kernel of their own) BEFORE anything is written: a
 * refused update leaves the handle exactly as it was.  cora_last_error says which.
 *
 * cora_update_values_times: wall-clock milliseconds of the last update's phases -- [0] map build (first call only),
 * [1] host check, [2] upload of the values, [3] device check + gather passes, [4] refresh of the host format. */
int cora_values_map_build(cora_ctx *ctx, const int32_t *rowptr, const int32_t *colidx);
int cora_update_values(cora_ctx *ctx, const int32_t *rowptr, const int32_t *colidx, const double *vals);
int cora_update_values_dev(cora_ctx *ctx, const double *d_vals);
int cora_update_values_times(const cora_ctx *ctx, double ms[5]);

/* ---- Q(w): the values of Q ASSEMBLED ON THE DEVICE from per-measurement weights ------------------------------------------
 * Q is linear in the weights of the measurements.  With the table of cora_set_measurements -- rows (ra, rb, ta, tb) and
 * data (R, t, kappa, tau) of an edge, rows (q, ta, tb) and data (r, omega) of a range -- every stored entry of Q is a
 * fixed sum of terms coef * w[i], the ones the reference's assembly produces (src/CORA_problem.cpp:115-377, 625-712):
 *   rotation of edge e (rb >= 0), weight e:    kappa at (ra+k, ra+k) and (rb+k, rb+k), k < d;
 *                                              -kappa R[a,c] at (ra+a, rb+c) and at (rb+c, ra+a)
 *   translation of edge e, weight n_edges + e: tau v_i v_j at every pair of the rows (ra .. ra+d-1, ta, tb), v = (-t, -1, +1)
 *   range m, weight 2 n_edges + m:             omega v_i v_j at every pair of the rows (q, ta, tb), v = (r, -1, +1)
 * (the rotation part is the connection Laplacian as the reference forms it, kappa on the diagonals -- not the expansion
 * of the residual, which differs wherever R is not exactly orthonormal).
 * WEIGHTS: 2 n_edges + n_ranges doubles, [rot of every edge | trans of every edge | range], the layout of the residuals
 * of cora_measurement_residuals_dev, so that a re-weighting loop reads residuals and writes weights at the same index.
 * Every weight must be finite and >= 0.  The rot weight of an edge without a rotation part (rb = -1) multiplies nothing
 * but is validated like the others.  A weight MULTIPLIES the precision the table held when the map was built: build with
 * the unweighted precisions and w = 1 reproduces Q.
 *
 * cora_assembly_build    (rowptr, colidx): the pattern the handle was created with (checked as cora_values_map_build
 *                        checks it; the source map of cora_update_values is built too when it is absent).  Builds the
 *                        TERM MAP -- for every CSR entry the list of (weight index, coefficient) -- and uploads it:
 *                        12 bytes per term and 4 per entry.  Needs a measurement table (CORA_ERR_NOT_READY).  Works on a
 *                        plan-only handle (device < 0).  CORA_ERR_ARG: a term with a nonzero coefficient outside the
 *                        pattern (the message names the measurement; terms whose coefficient is exactly 0.0 are
 *                        dropped), a row that repeats a column, 2^31 terms or more, a partitioned handle.
 *                        A later cora_set_measurements drops the map.
 * cora_assemble_values   w: the weights on the HOST.  vals_out: NULL or nnz host doubles that receive the assembled CSR
 *                        values (the bits the handle now holds).  The host copy of the format and the host copy of the
 *                        table are refreshed; on a plan-only handle the map is executed on the host.
 * cora_assemble_values_dev  d_w: the weights ON THE DEVICE; d_vals_out: NULL or nnz device doubles.  No host memory is
 *                        touched: the host copy of the format is stale as after cora_update_values_dev, and so is the
 *                        host copy of the table (cora_debug_measurement_residuals_host answers CORA_ERR_NOT_READY).
 * cora_debug_assemble_values_host  test hook: the map executed on the host in the device's order.  Never used by a compute
 *                        entry point; changes nothing of the handle.
 * cora_assembly_info     out = { number of weights, number of terms, long entries, most terms of one entry };
 *                        CORA_ERR_NOT_READY without a map.
 * cora_assemble_times    milliseconds of the last calls: [0] term map build, [1] weight check, [2] the assembly kernels
 *                        (events), [3] cora_update_values_dev's passes, [4] copies and host refresh.
 *
 * SUMMATION ORDER.  An entry's terms are ordered by ascending weight index and, for one measurement, as listed above
 * (diagonals of a, of b, the block (a, b) row by row, the block (b, a) in the same (a, c) order; pairs (i, j) row by
 * row).  An entry of at most 128 terms is summed by one thread: acc = fma(coef, w, acc) from +0.0 in that order.  A
 * longer one (a landmark's diagonal collects a term per measurement) by one wavefront: lane l sums terms l, l + 64, ...
 * the same way, then lane l += lane l + off for off = 32, 16, 8, 4, 2, 1, and lane 0 holds the entry.  No atomics: the
 * values are a function of the map and the weights, two calls give the same bits, and the host mirror gives the
 * device's bits.  An entry no term reaches is +0.0.  v_i v_j is formed before the precision multiplies it, so Q(w) is
 * bitwise symmetric and passes the symmetry check of an update.
 *
 * STATE after a successful call: that of cora_update_values* (above) -- the values go through the same check and gather
 * passes -- except that the measurement table FOLLOWS the weights: kappa, tau and omega become base * w (device copy
 * always, host copy by cora_assemble_values), so cora_measurement_residuals* return weighted residuals and 1/2 of their
 * sum stays the cost.  A refused call (a bad weight, no map, values the update refuses) leaves the handle as it was. */
int cora_assembly_build(cora_ctx *ctx, const int32_t *rowptr, const int32_t *colidx);
int cora_assemble_values(cora_ctx *ctx, const double *w, double *vals_out);
int cora_assemble_values_dev(cora_ctx *ctx, const double *d_w, double *d_vals_out);
int cora_debug_assemble_values_host(cora_ctx *ctx, const double *w, double *vals_out);
int cora_assembly_info(const cora_ctx *ctx, int64_t out[4]);
int cora_assemble_times(const cora_ctx *ctx, double ms[5]);

/* ---- The WEIGHT STEP of a robust-cost loop (graduated non-convexity) on the device -------------------------------------
 * One pass over the measurement table at a point X: the UNWEIGHTED residual r2 of every slot, its ratio rho = r2 / barc2 to
 * a threshold, the weight w(rho, mu) of the chosen cost, and the statistics a GNC schedule needs.  All vectors have the
 * weight layout of cora_assemble_values -- n_w = 2 n_edges + n_ranges doubles, [rot of every edge | trans of every edge |
 * range] -- so d_w_out is directly an argument of cora_assemble_values_dev and the loop never leaves the device.
 *   r2     the value cora_measurement_residuals* returns for the slot when the table holds the BASE precisions (the ones
 *          it held at cora_assembly_build): read from the term map, not from the table, whose kappa, tau and omega are
 *          base * w after a re-weighting -- a weight of 0 could never be undone from those.  It does not depend on the
 *          current weights, and has the bits of the residual kernels.  The rot slot of an edge without a rotation part is 0.
 *   barc2  one threshold per slot: finite and > 0, or +inf = trusted (rho = 0, w = 1).
 *   cost   CORA_GNC_NONE  w = 1, mu ignored (the statistics for mu_0)
 *          CORA_GNC_TLS   w = 1 for rho <= mu / (mu + 1);  0 for rho >= (mu + 1) / mu;  else sqrt(mu (mu + 1) / rho) - mu
 *          CORA_GNC_GM    t = mu / (rho + mu), w = t t
 *          each operation one plain fp64 operation in the order written (no contraction); the middle band of TLS is
 *          clamped to [0, 1], which rounding can leave by an ulp.
 *   couple_edges != 0: an edge is ONE measurement, r2 = rot + trans (one addition), its threshold is the one of its TRANS
 *          slot (the rot slots of barc2 are not read), and the same w goes to both slots.  Ranges are unaffected.
 *   stats  12 host doubles [3][4] for the segments rot, trans, range: { sum of w r2, largest rho (0 for an empty segment),
 *          number of 0 < w < 1, number of w < 0.5 }; counts are exact.  Coupled: an edge is counted and maximised in the
 *          trans segment only, the rot segment carries only its sum.  May be NULL.
 * cora_gnc_weights_dev  dX: a resident vector of k columns (1 <= k <= 24); d_barc2, d_w_out: n_w device doubles;
 *          d_r2_out: NULL or n_w device doubles.  Synchronises.
 * cora_gnc_weights      the host-pointer form (X: N x k column-major, uploaded first).
 * cora_debug_gnc_weights_host  test hook: the same sequence of operations on the host (no GPU needed): r2 and w have the
 *          device's bits; the statistics' sums are added in measurement order instead of per block.
 * No atomics on the outputs: block partials in fixed slots, one block adds them (the maxima likewise), so two calls give
 * the same bits, statistics included.
 * ERRORS.  CORA_ERR_NOT_READY without a table or without a term map (cora_assembly_build).  CORA_ERR_SHAPE for k outside
 * 1..24.  CORA_ERR_ARG: a null pointer, an unknown cost, mu not finite or <= 0 with a cost other than NONE, a threshold
 * that is NaN or <= 0, a partitioned handle.  CORA_ERR_NAN: a residual that is not finite.  On an error the contents of
 * the outputs are unspecified.
 * STATE.  The call never changes the handle: the current point, the preconditioner, the values, the table and the
 * staleness flags stay as they were. */
enum { CORA_GNC_NONE = 0, CORA_GNC_TLS = 1, CORA_GNC_GM = 2 };
int cora_gnc_weights_dev(cora_ctx *ctx, const double *dX, int k, const double *d_barc2, int cost, int couple_edges,
                         double mu, double *d_w_out, double *d_r2_out, double stats[12]);
int cora_gnc_weights(cora_ctx *ctx, const double *X, int ldx, int k, const double *barc2, int cost, int couple_edges,
                     double mu, double *w_out, double *r2_out, double stats[12]);
int cora_debug_gnc_weights_host(cora_ctx *ctx, const double *X, int ldx, int k, const double *barc2, int cost,
                                int couple_edges, double mu, double *w_out, double *r2_out, double stats[12]);

/* ---- TRAJECTORY ERROR against a reference (normally ground truth), aligned on the device ------------------------------
 * Compares a resident estimate X (k columns) with a resident reference Ref (kr <= k columns, normally kr = d).  A relaxed
 * solution is defined up to X -> X G, G in O(p), and a common shift of the translation rows, a rounded one up to a rigid
 * motion, so the two are aligned first: orthogonal Procrustes (Kabsch) on the selected poses' positions.
 * DEFINITIONS.  n poses, l = n_trans - n landmarks, dimension d.  For pose i: x_i in R^k its translation row of X, g_i in
 * R^kr its translation row of Ref, X_i (d x k) and G_i (d x kr) its rotation blocks.
 *   select   host array of n_trans bytes in API order (poses, then landmarks); NULL = all ones.  P = the selected poses,
 *            m = |P|; m = 0 is CORA_ERR_ARG.
 *   means    xbar = (1/m) sum_P x_i, gbar likewise.
 *   H        = sum_P (x_i - xbar)^T (g_i - gbar), k x kr, formed from CENTRED rows in two passes (the one-pass form cancels
 *            for a trajectory far from the origin).
 *   A        = U D V^T of the thin SVD H = U Sigma V^T (host, fp64, one-sided Jacobi), D = I; with CORA_COMPARE_PROPER
 *            (needs k == kr) D = diag(1, .., 1, det(U V^T)), so det A = +1 and a rounded solution is not matched by a
 *            reflection.  A minimises sum_P |(x_i - xbar) A - (g_i - gbar)|^2 over A^T A = I.  Where H is rank deficient
 *            (one pose; a collinear walk in 3-D) A is any such minimiser; the singular values are returned so that the
 *            caller can see it; it is not an error.
 *   et_i     = |(x_i - xbar) A - (g_i - gbar)|_2 per selected pose
 *   er_i     = |X_i A - G_i|_F per selected pose: the chordal distance; for kr = d the angle is 2 asin(er_i / (2 sqrt 2)).
 *   el_j     = the same as et with the rows of landmark j, per selected landmark.  Landmarks never enter xbar, gbar or H.
 *   Entries of the three arrays that are not selected are 0.0.
 *   out      8 + kr + k + kr + k kr host doubles: m, sum et^2, max et, sum er^2, max er, number of selected landmarks,
 *            sum el^2, max el | the kr singular values, descending | xbar | gbar | A column-major (k x kr).
 *   dAligned optional resident vector of kr columns, EVERY row whatever the selection: rotation and range rows times A,
 *            translation rows (x - xbar) A + gbar; padding rows are zero.  Must not overlap dX or dRef (checked).
 * cora_compare_dev   dX, dRef (and dAligned) resident vectors; pose_trans_err, pose_rot_err (n) and landmark_err (l) host
 *            arrays, each may be NULL.  Three device steps -- column sums, centred rows and H (the Gram kernel), errors --
 *            with the SVD on the host between the second and the third.  Synchronises.
 * cora_compare       the host-pointer form: X is N x k, Ref N x kr, Aligned (may be NULL) N x kr, column-major with leading
 *            dimensions; uploaded first.
 * cora_debug_compare_host  the same operations on the host; works on a plan-only handle (device < 0).  It does NOT mirror
 *            the device's lane order, so its sums, its H and with H its A have other last bits.  What holds for EACH form,
 *            against exact arithmetic on the same inputs, wherever D = I and H has full column rank:
 *              means   |xbar_c - exact| <= eps sum_P |x_ic|, gbar likewise
 *              H       |H_ab - exact| <= tol_ab = (m + 4) eps sum_P |x_ia - xbar_a| |g_ib - gbar_b|
 *              A       |A - exact|_F <= dA = 4 |tol|_F / sigma_min(H) + 64 k eps   (perturbation of the polar factor)
 *              entry   within 8 (k + kr) eps (|x_i - xbar| + |g_i - gbar| + |xbar| + |gbar|) of the exact error for ITS A,
 *                      xbar, gbar.
 *            Hence the two forms' A differ by at most 2 dA in the Frobenius norm, and an entry of the two by at most
 *            twice the entry bound plus |x_i - xbar| 2 dA + dm for a position (dm = twice the norms of the two vectors of
 *            mean bounds), sqrt(d) 2 dA for a rotation block -- bounds fixed by the inputs, not bit for bit.
 * No atomics on doubles: block partials in fixed slots, one block finishes them, so two calls give the same bits.
 * ERRORS.  CORA_ERR_SHAPE: k or kr outside 1..24, kr > k, a leading dimension below N.  CORA_ERR_ARG: a null dX, dRef or out,
 * an unknown flag, CORA_COMPARE_PROPER with k != kr, m = 0, an aligned vector that overlaps an input, a partitioned handle,
 * a handle whose row order does not keep a pose's d rotation rows consecutive.  CORA_ERR_NAN: a mean, H or an error that is
 * not finite.  On an error the contents of the outputs are unspecified.
 * STATE.  The call never changes what the handle computes with: the current point, the preconditioner, the values, the
 * tables and the staleness flags stay as they were.  Kept on the handle until it is destroyed: the pose table, the
 * per-entry error arrays, and the two centred vectors of cora_compare_dev (rows x k and rows x kr doubles, grown to the
 * widest k and kr seen) while they are at most 256 MiB each -- a larger one (10^6 poses at 24 columns: 0.86 GB) is
 * released before the call returns and allocated again by the next; cora_compare releases its three upload / download
 * vectors before it returns.  Every form also keeps H of its last call (k kr doubles) for cora_debug_compare_H. */
enum { CORA_COMPARE_PROPER = 1 };
int cora_compare_dev(cora_ctx *ctx, const double *dX, int k, const double *dRef, int kr, const unsigned char *select,
                     int flags, double *pose_trans_err, double *pose_rot_err, double *landmark_err, double *dAligned,
                     double *out);
int cora_compare(cora_ctx *ctx, const double *X, int ldx, int k, const double *Ref, int ldref, int kr,
                 const unsigned char *select, int flags, double *pose_trans_err, double *pose_rot_err, double *landmark_err,
                 double *Aligned, int ldal, double *out);
int cora_debug_compare_host(cora_ctx *ctx, const double *X, int ldx, int k, const double *Ref, int ldref, int kr,
                            const unsigned char *select, int flags, double *pose_trans_err, double *pose_rot_err,
                            double *landmark_err, double *Aligned, int ldal, double *out);
/* Test hook: H of the handle's last comparison (any of the three forms) with these k, kr; k x kr column-major. */
int cora_debug_compare_H(const cora_ctx *ctx, int k, int kr, double *H);

/* ---- RELATIVE POSE ERROR against a reference (normally ground truth), evaluated on the device ---------------------------
 * The error of the MOTION between two poses i -> j, for a table of pairs kept on the handle.  It needs no alignment: with
 * X_i the d x k rotation block of pose i and x_i its translation row, X_i X_j^T and X_i (x_j - x_i)^T are invariant under
 * X -> X G, G in O(k), and under a common shift of the translation rows.  So the estimate X (k columns) and the reference
 * Ref (kr columns) may have ANY column counts 1 <= k, kr <= 24, independent of each other and of the handle's rank: a
 * relaxed level of the staircase is compared with a d-column ground truth directly.
 * DEFINITIONS.  n poses, dimension d.  For pose i: X_i (d x k), x_i in R^k from X; G_i (d x kr), g_i in R^kr from Ref.
 * For a pair (i, j) of pose indices in API pose order, 0 <= i, j < n:
 *   E_ij = X_i X_j^T (d x d)        u_ij = X_i (x_j - x_i)^T (d)
 *   S_ij = G_i G_j^T                v_ij = G_i (g_j - g_i)^T
 *   et_ij = |u_ij - v_ij|_2         er_ij = |E_ij - S_ij|_F
 * er is the chordal distance cora_compare reports for a pose; for on-manifold d-column inputs the angle of the error
 * rotation is 2 asin(er / (2 sqrt 2)), and et is the length of the translation part of (S, v)^-1 (E, u), the usual RPE.
 * Any pair is allowed: i > j, repeated pairs, pairs across robots.  i == j is the identity motion in both vectors and
 * both errors are exactly 0.0 (the rows are not looked at: off the manifold X_i X_i^T and G_i G_i^T differ).  Landmarks
 * have no rotation and are not pairable.
 *   out      6 host doubles: m, sum et^2, max et, sum er^2, max er, the index of the first pair that attains max et.
 * SUMMATION ORDER.  A pair belongs to a group of 8 lanes.  A dot product over the columns of a vector is split over the
 * lanes in pieces of 16 bytes (8 at an odd row stride, i.e. an odd column count of 3 or more), piece v going to lane
 * v mod 8; a lane adds its pieces in column order with one fma per term from +0.0 (x_j - x_i is one subtraction per
 * column); the lanes are added by the butterfly over the distances 4, 2, 1, X and Ref separately; the d^2 + d differences
 * are taken afterwards, squared and added with one fma each in row-major order, E before u.  A pair's errors are a function
 * of its 2 d + 2 rows of each vector alone: the same bits on every call and at every place in the table.  No atomics on
 * doubles: block totals in fixed slots, one block finishes the sums, the maxima and the first maximum.
 * cora_set_pose_pairs   pairs: m x 2 int32 (i, j).  Validates, translates through the pose table the comparison keeps
 *            (first internal rotation row, translation row) and uploads structure-of-arrays.  A second call replaces the
 *            table; m = 0 clears it.  Works on a plan-only handle (device < 0) except for the upload.  A refused call
 *            leaves the table as it was.
 * cora_pose_pairs_count m of the table (0 without one).
 * cora_pose_pairs_equal *equal = 1 when the table holds exactly these m pairs in this order (m = 0: no table), else 0: a
 *            caller that evaluates in a loop installs a table only when it changed.
 * cora_rpe_dev          dX, dRef resident vectors of k and kr columns; trans_err, rot_err: host arrays of m doubles, each
 *            may be NULL -- with both NULL only `out` is read back.  Synchronises.
 * cora_rpe              the host-pointer form: X is N x k, Ref N x kr, column-major with leading dimensions; uploaded
 *            first, and the two vectors are released before it returns.
 * cora_debug_rpe_host   the same definitions on the host through the translated table; works on a plan-only handle.  It
 *            MIRRORS the lane pieces, the fma order and the butterfly: trans_err and rot_err have the device's bits, and
 *            with them the two maxima and the first maximum.  The two sums of squares are added in pair order, not in the
 *            device's block order: they agree with the device's within m eps times the sum, not bit for bit.
 * ROUNDING.  With a = |X_i|_F |x_j - x_i|, b = |G_i|_F |g_j - g_i|, A = |X_i|_F |X_j|_F, B = |G_i|_F |G_j|_F, eps = 2^-52,
 * exact double inputs, and any summation order of a length-k dot product within (k + 1) eps sum |p| |q|:
 *   |et - exact| <= 2 (k + kr + d + 8) eps (a + b)        |er - exact| <= 2 (k + kr + d + 8) eps (A + B)
 * x_j - x_i carries one relative eps, so a trajectory far from the origin does not cancel beyond it; the norm of an error
 * vector is bounded through the triangle inequality, so the bounds hold at et = 0 and er = 0 too; the factor 2 covers the
 * second-order terms and the final square root.  Both forms stay inside them against exact arithmetic.
 * ERRORS.  cora_set_pose_pairs: CORA_ERR_ARG for m < 0 or above 2^30, a null table with m > 0, an index outside [0, n) (the
 * message names the first bad pair), a partitioned handle, a handle whose row order does not keep a pose's d rotation rows
 * consecutive.  The three forms: CORA_ERR_ARG for a partitioned handle or a null X, Ref or out; CORA_ERR_SHAPE for k or kr
 * outside 1..24 or a leading dimension below N; CORA_ERR_NOT_READY without a table; CORA_ERR_NAN for an error or a sum that
 * is not finite.  On an error the contents of the outputs are unspecified.
 * STATE.  The calls never change what the handle computes with: the current point, the values, the preconditioner, the
 * measurement table, the term map and the staleness flags stay as they were.  Kept on the handle until replaced or
 * destroyed: the pair table (as given and translated, 24 bytes per pair on the host, 16 on the device) and two error
 * arrays of m doubles on the device. */
int cora_set_pose_pairs(cora_ctx *ctx, int64_t m, const int32_t *pairs /* [m][2] */);
int cora_pose_pairs_count(const cora_ctx *ctx, int64_t *m);
int cora_pose_pairs_equal(const cora_ctx *ctx, int64_t m, const int32_t *pairs, int *equal);
int cora_rpe_dev(cora_ctx *ctx, const double *dX, int k, const double *dRef, int kr, double *trans_err, double *rot_err,
                 double out[6]);
int cora_rpe(cora_ctx *ctx, const double *X, int ldx, int k, const double *Ref, int ldref, int kr, double *trans_err,
             double *rot_err, double out[6]);
int cora_debug_rpe_host(cora_ctx *ctx, const double *X, int ldx, int k, const double *Ref, int ldref, int kr,
                        double *trans_err, double *rot_err, double out[6]);

/* ---- ROUNDING of a relaxed point to SE(d), on the device -------------------------------------------------------------------
 * The step between a certified point of rank k and the rank-d estimate (projectSolution on the host): the input is a
 * resident vector Y of k columns, d <= k <= 24; the output a resident vector of d columns at stride cora_ld_for(d).  The
 * two must not overlap.
 * 1. BASIS.  G = Y^T Y over all rows (the Gram kernel of cora_gram_dev).  The k x k symmetric eigenproblem runs on the host
 *    (the comparison's one-sided Jacobi).  Vd (k x d): the eigenvectors of the d largest eigenvalues in descending order, each signed so that
 *    its entry of largest magnitude is positive (the first such entry on a tie).  Singular values: sqrt(max(lambda, 0)),
 *    descending, all k of them.
 * 2. COUNT.  M_i = Y_i Vd (d x d) for every pose block; count = the number of blocks with det(M_i) > 0.  When
 *    count < n / 2 (integer division; the host's rule) the last column of Y Vd is negated for every row of every kind.
 * 3. APPLY, one unit at a time:
 *    pose block        the R in SO(d) that maximises tr(R^T M_i): with M_i = U Sigma V^T it is U diag(1, .., 1, det(U V^T)) V^T,
 *                      the correction on the smallest singular value.  One-sided Jacobi on the block itself (no Gram matrix
 *                      of the block).  The result is a rotation -- orthonormal, determinant +1 -- for EVERY finite input: a
 *                      rank-deficient block is completed to a frame (the perpendicular at d = 2, cross products at d = 3),
 *                      a zero block gives exactly the identity.
 *    range row         y Vd normalised to unit length; a zero row stays zero.
 *    translation row   y Vd (poses and landmarks).
 *    A block or row at an extreme scale is brought into range by an exact power of two first, as the retraction does.  An
 *    input whose squares leave the range of a double altogether (|y| beyond about 1e+-150) has its Gram matrix formed from
 *    a copy scaled by a power of two, in a second pass that ordinary inputs never take.
 *   out      CORA_ROUND_OUT_LEN(k, d) <= CORA_ROUND_OUT_MAX host doubles: the count, flipped (0 / 1), the k singular values,
 *            Vd column-major (k x d).
 * ARITHMETIC.  A product y Vd is one fma per term from +0.0 in column order; every later operation of a unit is a single
 * correctly rounded one in a fixed order, never contracted.  A unit's output is a function of its own rows, Vd and the flip:
 * the same bits on every call.  The count is a sum of integers.  No atomics on doubles.
 * cora_round_dev        dY: k columns, dOut: d columns (cora_dev_alloc(ctx, d, ..)).  Synchronises (twice: the basis is
 *            formed on the host; count, its finish and the apply pass follow each other on the stream without a host step).
 * cora_round            the host-pointer form: Y is N x k, Out N x d, column-major with leading dimensions; its two vectors
 *            are released before it returns.
 * cora_debug_round_host the same on the host; works on a plan-only handle.  basis == NULL: Vd from this form's own Gram
 *            matrix (plain sums in row order).  basis != NULL (k x d column-major, e.g. the Vd a device call returned): the
 *            units run through the very functions the kernels call, so every output row, the count and the flip have the
 *            device's bits.  The singular values in `out` are this form's own in both cases.
 * ACCURACY.  A pose block against exact arithmetic on the same Vd: within a small multiple of eps kappa, kappa =
 * 2 sigma_1 / (sigma_{d-1} + s sigma_d) of M_i with s the sign of det(M_i), plus the forward error (k + 2) eps |Y_i| |Vd| of
 * the product scaled by kappa / sigma_1 (tests/round_ref.py calibrates the multiple on a float64 SVD; profiles/round.md).
 * ERRORS.  CORA_ERR_ARG: a partitioned handle, a null pointer, an output that overlaps the input; CORA_ERR_SHAPE: k < d or
 * k > 24, a leading dimension below N; CORA_ERR_NAN: an input entry or a product that is not finite (the device forms report
 * it through the handle's flag word).  On an error the contents of the outputs are unspecified.
 * STATE.  The calls never change what the handle computes with.  Nothing is kept on the handle between calls. */
#define CORA_ROUND_OUT_LEN(k, d) (2 + (k) + (k) * (d))
#define CORA_ROUND_OUT_MAX 98 /* k = 24, d = 3 */
int cora_round_dev(cora_ctx *ctx, const double *dY, int k, double *dOut, double *out);
int cora_round(cora_ctx *ctx, const double *Y, int ldy, int k, double *Out, int ldo, double *out);
int cora_debug_round_host(cora_ctx *ctx, const double *Y, int ldy, int k, const double *basis, double *Out, int ldo,
                          double *out);

/* ---- ODOMETRY INITIALISATION, on the device -------------------------------------------------------------------------------
 * The start the reference's experiments use by default ("init_type": "Odom"): every robot's odometry composed from a start
 * position, as a resident vector of d columns (cora_dev_alloc(ctx, d, ..), stride cora_ld_for(d)).  The lift to p columns
 * is cora_combine_dev with the first d rows of a p x p rotation.  Needs a measurement table (cora_set_measurements).
 * DEFINITIONS.
 *   chain            relative-pose edges e_1 .. e_m (m >= 1) of the measurement table, pose b of e_k being pose a of
 *                    e_{k+1}, with a start translation s of d numbers.  The head (pose a of e_1) gets (I, s); pose b of
 *                    e_k gets T_k = T_{k-1} o (R_k, t_k), that is R <- R R_k, t <- t + R t_k.
 *   rows of (R, t)   the rotation block holds R^T (row a, column b = R(b, a)), the translation row holds t.
 *   poses in no chain  an identity block and a zero translation.
 *   landmarks        the caller's landmarks[l][d]; NULL: zeros.
 *   range row m      (x_t(b) - x_t(a)) / |x_t(b) - x_t(a)| of the OUTPUT's translation rows, through the table's range
 *                    measurement m.  Where the norm is below 1e-5 the row stays zero and is reported as degenerate: the
 *                    caller supplies a direction afterwards (cora_odometry_set_range_rows_dev).  A range row no
 *                    measurement of the table names stays zero.
 * cora_set_odometry_chains   chain c is chain_edges[chain_ptr[c] .. chain_ptr[c + 1]), indices into the edge table.
 *            Validates, translates to position tables (chain c contributes its head, then its edges: P = edges + chains
 *            positions <= n) and uploads them; they stay on the handle until replaced, until the measurement table is
 *            replaced or until the handle is destroyed.  n_chains = 0 clears them (every pose is then in no chain; a handle
 *            that was never given chains behaves the same).  Works on a plan-only handle, except for the upload.  A refused
 *            call leaves the tables as they were.
 * cora_odometry_chains_count   out = {chains, positions}.
 * cora_odometry_scan_shape     out = {positions per tile, tile totals per sweep of the middle pass}: the shape the bracket
 *            order below depends on.
 * cora_odometry_init_dev   starts: host [n_chains][d]; landmarks: host [nt - n][d] or NULL; dOut: d columns; out (host):
 *            {poses written by chains, degenerate range rows}; degenerate: host bytes, one per range measurement of the
 *            table (1: degenerate), or NULL.  Rows: the poses in no chain and the landmarks, then the scan -- per-tile
 *            totals, one workgroup over the totals (in sweeps, carrying across them), per-tile scan with the carry-in, which
 *            writes the pose rows -- then the range rows.  Everything on the handle's stream; synchronises once, at the end.
 * cora_odometry_init       the host-pointer form: Out is N x d column-major with leading dimension ldo; its vector is
 *            released before it returns.
 * cora_odometry_set_range_rows_dev   writes dirs[i] / |dirs[i]| (host [m][d]) into the row of range measurement
 *            range_idx[i] of dOut, i < m: the rare path for the degenerate rows.  Synchronises.
 * cora_debug_odometry_init_host      the same on the host through the translated tables, in the device's bracket order and
 *            through the function the kernels compose with: Out has the device's bits.  Works on a plan-only handle.
 * ARITHMETIC.  A composition is one fma per term: an entry of R R_k from +0.0, an entry of t + R t_k from t, the inner index
 * ascending; never contracted.  The scan is segmented (a head resets the product) and brackets the factors of a chain as a
 * function of (P, the scan shape) alone: within a wavefront of 64 positions Kogge-Stone with offsets 1, 2, .., 32; within a
 * tile the totals of the wavefronts before are folded from the left and applied from the left; the same for the totals of the
 * tiles (one wavefront per sweep) and for the carry into a tile.  The same bits on every call.  A range row is the
 * difference, its squares summed by fma from +0.0, one square root, one division per entry.  The count of degenerate rows is
 * a sum of integers in fixed slots.  No atomics on doubles.
 * ACCURACY.  Against exact arithmetic, at position k of a chain (k factors of spectral norm 1, in any bracket order), to
 * first order: rotation block within k d^2 eps in Frobenius norm, translation row within k d^2 eps (|s| + sum |t_m|).
 * ERRORS.  CORA_ERR_NOT_READY: no measurement table.  CORA_ERR_ARG: a partitioned handle; a null pointer; an edge index
 * outside the table; an edge without a rotation part (second rotation row -1); an empty chain; two consecutive edges that do
 * not share the pose; a pose two positions would write (the message names the first offender); two range measurements of the
 * table that name one range row; a start, a landmark or a direction that is not finite, a direction without length.
 * CORA_ERR_SHAPE: a leading dimension below N.  CORA_ERR_NAN: a product that is not finite (the device forms report it
 * through the handle's flag word).  CORA_ERR_HIP: a device form on a plan-only handle.
 * STATE.  Nothing the handle computes with changes.  The handle keeps the position tables, the staging of the starts and
 * the landmarks, the scan's tile totals and the flag bytes. */
int cora_set_odometry_chains(cora_ctx *ctx, int64_t n_chains, const int64_t *chain_ptr /* [n_chains + 1] */,
                             const int32_t *chain_edges);
int cora_odometry_chains_count(const cora_ctx *ctx, int64_t out[2]);
int cora_odometry_scan_shape(const cora_ctx *ctx, int64_t out[2]);
int cora_odometry_init_dev(cora_ctx *ctx, const double *starts, const double *landmarks, double *dOut, int64_t out[2],
                           unsigned char *degenerate);
int cora_odometry_init(cora_ctx *ctx, const double *starts, const double *landmarks, double *Out, int ldo, int64_t out[2],
                       unsigned char *degenerate);
int cora_odometry_set_range_rows_dev(cora_ctx *ctx, int64_t m, const int32_t *range_idx, const double *dirs, double *dOut);
int cora_debug_odometry_init_host(cora_ctx *ctx, const double *starts, const double *landmarks, double *Out, int ldo,
                                  int64_t out[2], unsigned char *degenerate);

/* ---- LANDMARK INITIALISATION FROM RANGES: MULTILATERATION, on the device -----------------------------------------------
 * Places the landmarks of a resident vector of d columns (the output of cora_odometry_init_dev, stride cora_ld_for(d))
 * from the range table of the measurement table and the pose translations the vector holds, in place.  Needs a
 * measurement table (cora_set_measurements) and the tables of cora_set_multilateration.
 * DEFINITIONS.
 *   usable range     a range measurement of the table one endpoint of which is a landmark (a translation row past the n
 *                    poses' translation rows) and the other a pose, in either order.  Pose-pose and landmark-landmark
 *                    ranges are skipped and counted.
 *   anchor           the pose endpoint t_i of a usable range, with the distance r_i and the precision omega_i.
 *   list of l        the usable ranges of landmark l in table order, after the masks: pose_ok[n] keeps the anchors whose
 *                    pose is flagged (NULL: all), landmark_on[nl] the landmarks that are solved (NULL: all), nl = nt - n.
 *   chunk            kMlChunk = 256 consecutive entries of one list; a chunk never spans two lists.
 *   origin           the first anchor t_0 of a list; u_i = t_i - t_0, and the landmark is kept as y = x - t_0: the digits
 *                    stay when the trajectory is far from zero.
 *   linear stage     sums of omega, omega u, omega u u^T, omega b, omega b u with b = r^2 - |u|^2; the normal equations of
 *                    |y|^2 - 2 u^T y = b in (y, s), lengths scaled by the ONE scale L = sqrt(sum omega |u|^2 / sum omega),
 *                    divided by sum omega, factored by a (d + 1) x (d + 1) Cholesky without pivoting.
 *   status           0 solved | 1 fewer than d + 1 entries | 2 degenerate geometry: sum omega <= 0, L == 0 or a pivot
 *                    <= 1e-8 (anchors on a line in 2-D, in a plane in 3-D, coincident anchors) | 3 masked, or an empty
 *                    list.  A landmark whose status is not 0 keeps the row the caller wrote.
 *   Gauss-Newton     gn_steps in [0, 16] steps y <- y - H^-1 g with D_i = y - u_i, J_i = D_i / |D_i| (0 where |D_i| == 0),
 *                    e_i = |D_i| - r_i, H = sum omega J J^T / sum omega, g = sum omega J e / sum omega, by a d x d
 *                    Cholesky.  A landmark stops stepping, and keeps its point, at a pivot <= 1e-12 or a step that is not
 *                    finite.  The visited points are 0 (the linear solution), 1, 2, ..; the cost sum omega e^2 is
 *                    evaluated at every one, the last included, and the row written is t_0 + the visited point of least
 *                    cost, the earliest on ties (chosen): never worse than the linear solution on the range cost.
 *   range rows       afterwards the unit range rows of ALL range measurements are recomputed from the translation rows by
 *                    the range-row step of the odometry initialisation, its rules unchanged (below 1e-5: a zero row,
 *                    reported degenerate; the caller supplies directions with cora_odometry_set_range_rows_dev), with
 *                    the endpoints exchanged: row m = (x_t(a) - x_t(b)) / |x_t(a) - x_t(b)|, the direction at which the
 *                    residual |x_t(b) - x_t(a) + r x_rho|^2 of the table is (|x_t(b) - x_t(a)| - r)^2, so that the range
 *                    residuals of the result ARE the range cost the landmarks were placed by.  (cora_odometry_init_dev
 *                    writes the opposite direction, as the host function it mirrors does.)
 * cora_set_multilateration   validates, groups, translates to internal rows once and uploads the chunk table.  The tables
 *            stay on the handle until replaced, until the measurement table is replaced or until the handle is destroyed.
 *            Works on a plan-only handle, except for the upload.  A refused call leaves the tables as they were.
 * cora_multilateration_counts   out = {landmarks with a non-empty list, usable ranges (before the masks), skipped ranges,
 *            chunks}.
 * cora_multilaterate_dev   out (host) = {landmarks solved, landmarks not solved, degenerate range rows, Gauss-Newton steps
 *            taken, summed over the landmarks}; status, cost_linear, cost_final, chosen: host arrays of nl entries or NULL
 *            (costs 0 and chosen -1 where the status is not 0); degenerate: host bytes, one per range measurement, or NULL.
 *            2 (gn_steps + 2) launches -- per stage one pass over the chunks and one fold per landmark -- and the range
 *            rows.  Everything on the handle's stream; synchronises once, at the end.
 * cora_multilaterate       the host-pointer form, in place: X is N x d column-major with leading dimension ldx.
 * cora_debug_multilaterate_host   the same on the host through the translated tables, in the device's bracket order and
 *            through the functions the kernels call: X has the device's bits.  Works on a plan-only handle.  (It reads the
 *            host's copy of the range table: after cora_assemble_values_dev rescaled the device's precisions the two differ.)
 * ARITHMETIC.  Single correctly rounded fp64 operations in the order written, never contracted: u by subtraction, |u|^2
 * by fma from +0.0, b = fma(r, r, -|u|^2), every term a chain of products from the left (omega u_a, then times u_b; omega
 * b, then times u_a; omega J_a, then times J_b or e; omega e, then e).  The sums are additions bracketed as a function of the
 * list's length and kMlChunk alone: within a wavefront of 64 entries a butterfly over lane exchanges with offsets 1, 2, ..,
 * 32 (the balanced tree over neighbouring lanes; a lane without an entry holds +0.0); the four wavefronts of a chunk from the
 * left; chunk sums as [sum][chunk]; one wavefront per landmark in which lane j adds chunks j, j + 64, .. of the list from the
 * left to +0.0, then the same butterfly.  The solves use fma with the inner index ascending, one square root per pivot, one
 * division per entry.  The same bits on every call.  No atomics on doubles.
 * ACCURACY.  The linear solution is that of a least-squares problem in the squared ranges: its error against exact
 * arithmetic is of the order eps kappa(M) (|y| + L) with M the scaled normal matrix, and on noisy ranges it is not the
 * minimiser of the range cost, which the Gauss-Newton steps approach; their error is of the order eps kappa(H) (|y| + L).
 * ERRORS.  CORA_ERR_NOT_READY: no measurement table, or no multilateration tables.  CORA_ERR_ARG: a partitioned handle;
 * gn_steps outside [0, 16]; a null X or out; two range measurements of the table that name one range row.  CORA_ERR_SHAPE: a
 * leading dimension below N.  CORA_ERR_NAN: a sum or a range row that is not finite (the device forms report it through
 * the handle's flag word).  CORA_ERR_HIP: a device form on a plan-only handle.
 * STATE.  Nothing the handle computes with changes.  The handle keeps the list and chunk tables, the chunks' partial sums,
 * the landmarks' state and the flag bytes. */
int cora_set_multilateration(cora_ctx *ctx, const unsigned char *pose_ok /* [n] or NULL */,
                             const unsigned char *landmark_on /* [nt - n] or NULL */);
int cora_multilateration_counts(const cora_ctx *ctx, int64_t out[4]);
int cora_multilaterate_dev(cora_ctx *ctx, double *dX, int gn_steps, int64_t out[4], unsigned char *status, double *cost_linear,
                           double *cost_final, int32_t *chosen, unsigned char *degenerate);
int cora_multilaterate(cora_ctx *ctx, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status,
                       double *cost_linear, double *cost_final, int32_t *chosen, unsigned char *degenerate);
int cora_debug_multilaterate_host(cora_ctx *ctx, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status,
                                  double *cost_linear, double *cost_final, int32_t *chosen, unsigned char *degenerate);

/* Outlier-robust multilateration: a consensus vote over minimal samples of d + 1 ranges in front of the fit.  A
 * range that is grossly long (NLOS, multipath) drags the linear stage, which works in SQUARED ranges, far off, and the
 * Gauss-Newton steps then descend the contaminated cost.  Tables, lists, chunks, origin, masks, the range-row step and the
 * meaning of gn_steps are exactly those above: there is no new set call.  Per list of a landmark that is to be solved (L >= d
 * + 1 entries e = 0 .. L - 1 in table order; origin t_0 the first anchor, whether or not it turns out an inlier; u_j = t_j - t_0):
 *   sample of h      the entries (h + k s) mod L, k = 0 .. d, s = max(1, L / (d + 1)) (integer division): d + 1 distinct
 *                    entries (d s < L) spread over the list instead of d + 1 consecutive, nearly collinear poses; a function
 *                    of (h, L, d) alone: no random number, the same bits on every call and in the mirror.
 *   hypothesis       y_h: the linear stage's terms of the sample's entries (their own omega, relative to t_0) added from the
 *                    left in the order k = 0 .. d starting from +0.0, then the linear stage's solve.  VALID where that solve
 *                    has status 0 (pivots > 1e-8, a finite result: the plain fit's rule filters a near-degenerate sample); an
 *                    invalid hypothesis has vote 0 and y = 0 and sets no flag.
 *   score            r(h, j) = (omega_j e) e, e = |y_h - u_j| - r_j: the difference, fma from +0.0, one square root -- the
 *                    operations and order of the Gauss-Newton cost term: the weighted squared range residual that
 *                    cora_gnc_weights thresholds, no 1/2.
 *   vote             vote(h) = #{ j : r(h, j) <= barc2 } over EVERY entry of the list, the sample's own included; a NaN is no
 *                    vote.  A valid hypothesis therefore starts with about d + 1 votes of its own: A CONSENSUS MEANS SOMETHING
 *                    ONLY ABOVE d + 1.  barc2: one finite scalar > 0.
 *   election         h* = the entry of largest vote, among equal votes the lowest entry; consensus = vote(h*).  A list without
 *                    a valid hypothesis elects entry 0 with consensus 0.  consensus < min_consensus (min_consensus >= 1):
 *                    status 5, "no consensus": the landmark keeps the row the caller wrote and counts as not solved.  (4 is
 *                    not used by the multilateration.)
 *   inliers          I = { j : r(h*, j) <= barc2 }, the same function and bits as the vote; empty at consensus 0.
 *   refit            the plain fit over I only: one linear stage (status 2 is still possible), gn_steps Gauss-Newton stages, the
 *                    last evaluation, the visited point of least cost, the earliest on ties.  AN ENTRY OUTSIDE I ADDS +0.0 FOR
 *                    EACH OF ITS TERMS (it is not skipped: the bracket order of every sum is the plain call's, a lane beyond a
 *                    chunk's end adds the same +0.0).  cost_linear and cost_final are sums over I.  One election, one refit.
 *   cost             L^2 scores per list of L entries, by design: every entry is a hypothesis.
 *   limit            one hypothesis per entry, and a hypothesis is clean only where all d + 1 entries of its sample are
 *                    inliers: a fraction (1 - eps)^(d + 1) of the L hypotheses at an outlier fraction eps.  Short lists with
 *                    many outliers do not reach a consensus (status 5) or elect a contaminated hypothesis.
 * out = the plain call's four fields, then {landmarks without consensus (status 5; they are among out[1]), ranges excluded: the
 * inlier bytes equal to 0}.  status, cost_linear, cost_final, chosen, degenerate: as the plain call's.  elected [nl]: h*, -1
 * where the landmark's list is not voted on (status 1 or 3);  consensus [nl]: 0 there;  list_len [nl]: the entries of the
 * landmark's list;  inlier [n_ranges]: 1 in I | 0 in a list that is voted on, outside I (every entry of a list with consensus 0)
 * | 2 in no such list (pose-pose, landmark-landmark, masked, a list that is too short).  Every array may be NULL.
 * 2 + 2 (gn_steps + 2) launches (vote, elect, then the stages with masked passes), then the range rows.
 * cora_multilaterate_robust: the host-pointer form.  cora_debug_multilaterate_robust_host: the mirror, the same functions in the
 * same bracket order: the device's bits; works on a plan-only handle.
 * ERRORS.  The plain call's; CORA_ERR_ARG also for barc2 not finite or <= 0 and for min_consensus < 1; CORA_ERR_NAN also for an
 * elected hypothesis that is not finite.  STATE.  Nothing the handle computes with changes, nor its tables. */
int cora_multilaterate_robust_dev(cora_ctx *ctx, double *dX, int gn_steps, double barc2, int min_consensus, int64_t out[6],
                                  unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected,
                                  int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate);
int cora_multilaterate_robust(cora_ctx *ctx, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[6],
                              unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected,
                              int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate);
int cora_debug_multilaterate_robust_host(cora_ctx *ctx, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[6],
                                         unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected,
                                         int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate);

/* ---- CHAIN PLACEMENT FROM INTER-ROBOT RANGES, on the device ---------------------------------------------------------------
 * Moves whole odometry chains of a resident vector of d columns (the output of cora_odometry_init_dev: every chain
 * composed in its own frame) rigidly into the frame of the chains that are fixed, from the pose-pose ranges between
 * chains, in place.  Needs a measurement table (cora_set_measurements), chain tables (cora_set_odometry_chains) and the
 * tables of cora_set_chain_placement.  The multilateration with an element of SE(d) per chain in place of a point.
 * DEFINITIONS.
 *   entry            a range measurement one end of which is the translation row of a position of chain c and the other
 *                    the translation row of a position of another chain c', in either order; duplicates count twice.
 *                    Every other range (an end in a free pose or a landmark, both ends in one chain) is skipped and counted.
 *   order            placed = the chains of chain_fixed (NULL: chain 0).  Repeatedly the unplaced chain with the most
 *                    entries against placed chains is taken (ties: the lowest index) until that count is below min_ranges;
 *                    a chain taken is a STAGE and counts as placed from then on.  min_ranges >= 8 (d = 2), 17 (d = 3).
 *   stage's list     the entries of the stage's chain against the chains placed before it, in table order, as (row of the
 *                    chain's position q, row of the anchor a, measurement), cut into chunks of 256; no chunk spans two stages.
 *   status           0 placed | 1 never taken, fewer than min_ranges entries against placed chains | 2 placed, the linear
 *                    stage refused (sum omega <= 0, no length scale, a pivot <= 1e-8 of the scaled normal matrix: positions
 *                    on a line in 2-D or in a plane in 3-D, coincident points): the Gauss-Newton steps start from the
 *                    identity | 3 never taken, no entry against any chain | 4 fixed.
 *   a stage          finds g = (R, t) that minimises sum omega (|R q + t - a| - r)^2 over its list, q and a as the vector
 *                    holds them (a was written by an earlier stage or belongs to a fixed chain).  Coordinates are relative to
 *                    the first entry: q' = q - q_0, a' = a - a_0, t' = R q_0 + t - a_0.
 *                    Visited point 0 is the identity (cost_start).  Point 1 is the linear stage in the squared ranges,
 *                    |q'|^2 + |a'|^2 + s + 2 q'.v - 2 a'^T M q' - 2 a'.t' = r^2 in the unknowns s, v, M, t' (7 at d = 2 with
 *                    M = (cos, sin); 16 at d = 3), lengths scaled by L = sqrt(sum omega (|q'|^2 + |a'|^2) / (2 sum omega)),
 *                    the normal equations divided by sum omega and factored by Cholesky without pivoting, M projected to
 *                    SO(d) (cost_linear; the identity again where the stage is refused).  Points 2 .. gn_steps + 1 follow by
 *                    Gauss-Newton steps on the d (d + 1) / 2 degrees of freedom (rotation in units of L, then translation):
 *                    with u = R q', p = u + t' - a', n = p / |p|, e = |p| - r and J = ((u x n) / L | n), delta = -H^-1 g,
 *                    R <- round(Cayley(delta_rot / L) R), t' <- t' + delta_t; a stage stops stepping at a pivot <= 1e-12
 *                    of H / sum omega or a step that is not finite.  The transform written is the visited point of least
 *                    cost, the earliest on ties (chosen; cost_final): a stage never raises the range cost over its own
 *                    entries.  Where point 0 wins the chain's rows are not touched.
 *   apply            t_i <- R t_i + t and the stored block R_i^T <- R_i^T R^T for every position of the chain.
 *   range rows       afterwards the unit range rows of ALL range measurements are recomputed in the direction of least
 *                    residual, as cora_multilaterate_dev does, with its degenerate bytes and count.
 * cora_set_chain_placement   decides the order, builds and uploads the tables.  They stay on the handle until replaced,
 *            until the measurement table or the chain tables are replaced or until the handle is destroyed.  Works on a
 *            plan-only handle, except for the upload.  A refused call leaves the tables as they were.
 * cora_chain_placement_counts   out = {stages, entries, chunks, skipped ranges}.
 * cora_chain_placement_order    stage_chain[stages] = the chain of every stage, in the order of the stages.
 * cora_place_chains_dev   out (host) = {chains placed, chains not placed, Gauss-Newton steps taken, degenerate range rows,
 *            stages}; status, cost_start, cost_linear, cost_final, chosen: host arrays with one entry per chain or NULL
 *            (costs 0 and chosen -1 where the chain is no stage); transforms: [chains][d * d + d], R row-major then t as
 *            written, the identity where the chain is no stage or point 0 won; degenerate: host bytes, one per range
 *            measurement, or NULL.  Per stage 2 (gn_steps + 3) + 1 launches, one stage after the other, then the range
 *            rows.  Everything on the handle's stream; synchronises once, at the end.
 * cora_place_chains       the host-pointer form, in place: X is N x d column-major with leading dimension ldx.
 * cora_debug_place_chains_host   the same on the host in the device's bracket order and through the functions the kernels
 *            call: X has the device's bits.  Works on a plan-only handle.
 * ARITHMETIC.  No transcendental function: + - x / and sqrt only, single correctly rounded fp64 operations in the order
 * written, never contracted.  Linear stage: the entry's terms and weight are staged per chunk and pair product (i, j) is
 * summed over the chunk's entries from the left as (omega c_i) c_j from +0.0; Gauss-Newton sums as the multilateration's;
 * chunk sums as [sum][chunk]; one wavefront in which lane j adds chunks j, j + 64, .. of the stage from the left to +0.0,
 * then the butterfly.  The same bits on every call.  No atomics on doubles.
 * ERRORS.  CORA_ERR_NOT_READY: no measurement table, no chain tables, or no placement tables.  CORA_ERR_ARG: a partitioned
 * handle; min_ranges below the linear stage's unknowns + 1; a mask that fixes no chain; gn_steps outside [0, 16]; a null
 * X or out; two range measurements that name one range row.  CORA_ERR_SHAPE: a leading dimension below N.  CORA_ERR_NAN: a
 * sum or a range row that is not finite (the device forms report it through the handle's flag word).  CORA_ERR_HIP: a
 * device form on a plan-only handle.
 * STATE.  Nothing the handle computes with changes. */
int cora_set_chain_placement(cora_ctx *ctx, const unsigned char *chain_fixed /* [chains] or NULL */, int min_ranges);
int cora_chain_placement_counts(const cora_ctx *ctx, int64_t out[4]);
int cora_chain_placement_order(const cora_ctx *ctx, int32_t *stage_chain);
int cora_place_chains_dev(cora_ctx *ctx, double *dX, int gn_steps, int64_t out[5], unsigned char *status, double *cost_start,
                          double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate);
int cora_place_chains(cora_ctx *ctx, double *X, int ldx, int gn_steps, int64_t out[5], unsigned char *status, double *cost_start,
                      double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate);
int cora_debug_place_chains_host(cora_ctx *ctx, double *X, int ldx, int gn_steps, int64_t out[5], unsigned char *status,
                                 double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen, double *transforms,
                                 unsigned char *degenerate);

/* ---- CHAIN PLACEMENT FROM INTER-ROBOT RANGES: LEVELS, and a level's chains placed together ----------------------------------
 * A second, opt-in order of the stages of the chain placement above and the batched launches it makes possible.  The greedy
 * order, cora_set_chain_placement, cora_place_chains_dev and their bits are unchanged.
 * DEFINITIONS.
 *   level order      level 0 = the chains of chain_fixed (NULL: chain 0).  Level k >= 1 = every chain not yet placed whose
 *                    entries against chains of levels < k number at least min_ranges; its stages stand in ascending chain
 *                    index.  A stage's list: the chain's entries against chains of levels < k ONLY, in table order -- an
 *                    entry against a chain of the same level is NOT in the list, which is what makes the stages of a level
 *                    independent of each other.  The order ends where a level would be empty; the chains left over have
 *                    status 1 or 3 by the rule above.  From structure alone, like the greedy order.
 *   THE LIMIT        a chain is placed from FEWER ranges than under the greedy order wherever chains of its own level range
 *                    against it: those ranges are ignored (under the greedy order the later of the two chains uses them).
 *                    Where every chain ranges only against earlier levels (a star, a relay) the lists and the bits coincide.
 *                    Measured on the shipped data sets: profiles/chain_placement_levels.md.  The promise is the one above: a
 *                    stage never raises the range cost over its own entries.
 *   greedy as levels the greedy order stores every stage as a level of its own, so every call below serves both orders.
 * cora_set_chain_placement_order   cora_set_chain_placement with the order chosen: CORA_PL_ORDER_GREEDY gives its tables
 *            exactly, CORA_PL_ORDER_LEVELS the level order.  Counts, the order of the stages, the plain device forms and the
 *            host mirror run on either tables, one stage after the other in table order -- a legal dependent order, so they
 *            are the reference and the mirror of the batched call.
 * cora_chain_placement_levels   stage_level[stages] = the level k >= 1 of every stage, in the order of the stages
 *            (ascending; level 0, the fixed chains, has no stage).  The number of levels is the last entry.
 * cora_place_chains_batched_dev   cora_place_chains_dev with every launch serving ALL stages of one level: the passes one
 *            workgroup per chunk of the level, the folds one wavefront per stage, the apply one workgroup per 256 positions
 *            of one chain.  2 (gn_steps + 3) + 1 launches per LEVEL, then the range rows.  out (host) = the five fields of
 *            cora_place_chains_dev, then the number of levels.  Every other argument, every error and the state are
 *            cora_place_chains_dev's; X, the per-chain outputs, the degenerate bytes and out[0..4] have its bits on the same
 *            tables (the terms, the chunk sums and the fold's bracket order over a stage's own chunks are the same).
 * cora_place_chains_batched       the host-pointer form. */
enum { CORA_PL_ORDER_GREEDY = 0, CORA_PL_ORDER_LEVELS = 1 };
int cora_set_chain_placement_order(cora_ctx *ctx, const unsigned char *chain_fixed /* [chains] or NULL */, int min_ranges, int order);
int cora_chain_placement_levels(const cora_ctx *ctx, int32_t *stage_level);
int cora_place_chains_batched_dev(cora_ctx *ctx, double *dX, int gn_steps, int64_t out[6], unsigned char *status, double *cost_start,
                                  double *cost_linear, double *cost_final, int32_t *chosen, double *transforms,
                                  unsigned char *degenerate);
int cora_place_chains_batched(cora_ctx *ctx, double *X, int ldx, int gn_steps, int64_t out[6], unsigned char *status, double *cost_start,
                              double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate);

/* Outlier-robust chain placement: a consensus vote over samples of m ranges in front of the batched fit.  The first
 * visited point of a stage is a linear stage in the SQUARED ranges with 7 (d = 2) or 16 (d = 3) unknowns: one NLOS or multipath
 * range lengthened by 10 m enters with its square and drags all of them, the Gauss-Newton steps then descend the contaminated
 * cost, and every later stage and the landmark multilateration inherit the misplaced chain.  Tables, order (greedy or levels),
 * lists, chunks, origin, the range-row step and the meaning of gn_steps are those of cora_set_chain_placement_order: there is no
 * new set call.  Per stage list of L entries e = 0 .. L - 1 in table order (origin q_0, a_0 of the first entry, whether or not
 * it turns out an inlier; q' = q - q_0, a' = a - a_0; the stage carries g = (R, t')), with m = unknowns + 1 = 8 at d = 2 and
 * 17 at d = 3, the least min_ranges the set call accepts, so L >= m:
 *   sample of h      the entries (h + k s) mod L, k = 0 .. m - 1, s = max(1, L / m) (integer division): m distinct entries
 *                    spread over the list, a function of (h, L, d) alone: no random number, the same bits on every call and
 *                    in the mirror.
 *   hypothesis       g_h: the linear stage's terms and weights of the sample's entries, every pair product added from the left
 *                    in the order k = 0 .. m - 1 starting from +0.0, then the linear stage's solve.  VALID only where that
 *                    solve has status 0.  A valid hypothesis then takes 3 Gauss-Newton steps ON THE SAMPLE'S OWN m ENTRIES
 *                    (the Gauss-Newton terms added from the left in the order k from +0.0; the step with the sample's length
 *                    scale and sum omega); a refused step keeps the point and ends the stepping, the hypothesis stays valid.
 *                    The linear stage from 17 noisy ranges is badly conditioned at d = 3; the 17 ranges over-determine the 6
 *                    degrees of freedom well once it has found the basin.  An invalid hypothesis has g = the identity and
 *                    vote 0 and sets no flag.
 *   score            r(h, j) = (omega_j e) e, e = |R_h q'_j + t'_h - a'_j| - r_j: the operations and order of the Gauss-Newton
 *                    cost term: the weighted squared range residual that cora_gnc_weights thresholds, no 1/2.
 *   vote             vote(h) = #{ j : r(h, j) <= barc2 } over EVERY entry of the list, the sample's own included; a NaN is no
 *                    vote.  A CONSENSUS MEANS SOMETHING ONLY ABOVE m.  barc2: one finite scalar > 0.
 *   election         h* = the entry of largest vote, among equal votes the lowest entry; consensus = vote(h*).  A list without
 *                    a valid hypothesis elects entry 0 with consensus 0.  consensus < min_consensus (min_consensus >= 1):
 *                    status 5, "no consensus": the chain's rows are not touched and the chain counts as not placed; later
 *                    stages still read its rows, as they do after a stage where point 0 won.
 *   inliers          I = { j : r(h*, j) <= barc2 }, the same function and bits as the vote; empty at consensus 0.
 *   refit            the plain stages over I only: the identity's cost, the linear stage (status 2 is still possible), the
 *                    gn_steps Gauss-Newton steps, the last evaluation; the visited point of least cost is written, the
 *                    earliest on ties.  AN ENTRY OUTSIDE I ADDS +0.0 FOR EACH OF ITS TERMS, in the pair products of the linear
 *                    pass and in the sums of the Gauss-Newton pass (it is not skipped: the bracket order of every sum is the
 *                    plain call's).  A list without outliers therefore has cora_place_chains_batched_dev's bits.  cost_start,
 *                    cost_linear and cost_final are sums over I.  One election, one refit.
 *   cost             L^2 scores per list of L entries, by design: every entry is a hypothesis.
 *   limit            a hypothesis is clean only where all m entries of its sample are inliers: a share (1 - eps)^m of the
 *                    hypotheses at an outlier share eps -- 0.43 / 0.17 at eps = 0.1 for d = 2 / 3, 0.17 / 0.02 at eps = 0.2.
 *                    Strided samples overlap (sample h and sample h + s share m - 1 entries), so clean samples come in runs.
 *                    Short lists with many outliers end in status 5 or elect a contaminated hypothesis.
 * out = the six fields of cora_place_chains_batched_dev (a stage without consensus is among out[1], not placed, and not among
 * out[0], placed; out[4] counts it as a stage), then {stages without
 * consensus, ranges excluded: the inlier bytes equal to 0}.  status, cost_start, cost_linear, cost_final, chosen, transforms,
 * degenerate: as the batched call's (costs 0, chosen -1, the identity at status 5).  elected [chains]: h*, -1 where the chain is
 * no stage;  consensus [chains]: 0 there;  list_len [chains]: the entries of the chain's stage list, 0 there;  inlier [n_ranges]:
 * 1 in I | 0 in a stage list, outside I (every entry of a list with consensus 0) | 2 in no stage list.  Every array may be NULL.
 * Per LEVEL 3 launches (hypotheses, vote, election), then the 2 (gn_steps + 3) + 1 of the batched call with masked passes; then
 * the range rows.  Everything on the handle's stream; synchronises once, at the end.  The vote's workspaces are made at the
 * first robust call on the tables and freed with them.
 * cora_place_chains_robust: the host-pointer form.  cora_debug_place_chains_robust_host: the mirror, the same functions in the
 * same bracket order: the device's bits; works on a plan-only handle.
 * ERRORS.  The plain call's; CORA_ERR_ARG also for barc2 not finite or <= 0 and for min_consensus < 1; CORA_ERR_NAN also for an
 * elected hypothesis that is not finite.  STATE.  Nothing the handle computes with changes, nor its tables. */
int cora_place_chains_robust_dev(cora_ctx *ctx, double *dX, int gn_steps, double barc2, int min_consensus, int64_t out[8],
                                 unsigned char *status, double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen,
                                 double *transforms, int32_t *elected, int32_t *consensus, int32_t *list_len, unsigned char *inlier,
                                 unsigned char *degenerate);
int cora_place_chains_robust(cora_ctx *ctx, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[8],
                             unsigned char *status, double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen,
                             double *transforms, int32_t *elected, int32_t *consensus, int32_t *list_len, unsigned char *inlier,
                             unsigned char *degenerate);
int cora_debug_place_chains_robust_host(cora_ctx *ctx, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[8],
                                        unsigned char *status, double *cost_start, double *cost_linear, double *cost_final,
                                        int32_t *chosen, double *transforms, int32_t *elected, int32_t *consensus, int32_t *list_len,
                                        unsigned char *inlier, unsigned char *degenerate);

/* ---- PLACEMENT FROM POSE-LANDMARK SIGHTINGS, on the device ----------------------------------------------------------------
 * Places landmarks and whole odometry chains of a resident vector of d columns (the output of cora_odometry_init_dev)
 * from the pose-landmark sightings of the measurement table, in place; both solves are closed-form.  Needs a measurement
 * table (cora_set_measurements), chain tables (cora_set_odometry_chains) and the tables of cora_set_sighting_placement.
 * DEFINITIONS.
 *   sighting         an edge of the measurement table whose second rotation row is -1, whose first translation row is the
 *                    translation row of a position of an odometry chain and whose second translation row is a landmark's
 *                    row (past the n poses' translation rows).  Every other edge without a second rotation (a landmark
 *                    prior, a sighting from a free pose) is skipped and counted.  Its data: pose a, landmark l, t and tau as
 *                    the table holds them.
 *   prediction       p = x_t(a) + sum_c t_c X_a[c, :] from the vector as it stands: the point at which the table's
 *                    translation residual of the edge is zero.
 *   sighting cost    of a set of sightings: sum tau |x_t(l) - p|^2, the table's own residual.
 *   order            decided on the host from structure alone.  The placed chains start as chain_fixed (NULL: chain 0), the
 *                    placed landmarks as landmark_fixed (NULL: none).  Then an L-stage and a C-stage alternate until
 *                    neither takes anything; then one REFIT stage follows.  A stage that takes nothing is no stage.
 *   L-stage          every unplaced landmark with at least one sighting from a position of a placed chain; its list is
 *                    those sightings in table order; it counts as placed from then on.
 *   C-stage          EVERY unplaced chain with at least min_sightings sightings of placed landmarks, among them at least d
 *                    distinct landmarks: all of them in the same stage, solved side by side in the same launches.  A chain's
 *                    list is those sightings in table order.  min_sightings >= d.
 *   REFIT            every landmark outside landmark_fixed with a sighting from any placed chain is set again, from ALL its
 *                    sightings by placed chains.
 *   lists            cut into chunks of 256; no chunk spans two lists.  Coordinates are relative to the first entry of the
 *                    list: p' = p - p_0, l' = x_t(l) - l_0.
 *   landmark         x_t(l) = p_0 + (sum tau (p_i - p_0)) / sum tau.  landmark_status: 0 placed | 1 no sighting from a placed
 *                    chain | 2 sum tau <= 0 (the row is not touched) | 3 fixed.  The status and landmark_cost (the sighting
 *                    cost of the REFIT's list at the row written; 0 without a list) are the REFIT's.
 *   chain            g = (R, t) that minimises sum tau |R p_i + t - x_t(l_i)|^2 over the list.  From the sums of tau, tau p',
 *                    tau l', tau l' p'^T, tau |p'|^2, tau |l'|^2 (11 at d = 2, 18 at d = 3):  W = sum tau,
 *                    H = sum tau l' p'^T - (sum tau l')(sum tau p')^T / W,  R = the rotation that maximises tr(R^T H)
 *                    (one-sided Jacobi with the determinant correction on the smallest singular value),  t' = (sum tau l')
 *                    / W - R (sum tau p') / W,  t = t' + l_0 - R p_0.  A second pass evaluates the sighting cost of the list
 *                    at the identity (cost_start) and at g (as tau |R p' + t' - l'|^2).  g is applied only where its
 *                    cost is below cost_start (chosen 1, cost_final = the cost at g); otherwise the chain's rows are not
 *                    touched (chosen 0, cost_final = cost_start): cost_final <= cost_start as doubles, always.
 *                    status: 0 placed | 1 never taken (too few sightings of placed landmarks or too few distinct ones) |
 *                    2 taken but refused by the device | 3 no sighting at all | 4 fixed.
 *   refusal          a function of the sums alone.  With the centred spreads s_p = sum tau |p'|^2 - |sum tau p'|^2 / W and
 *                    s_l likewise, and k = 1e-6 (a length ratio): refused where W <= 0, s_p <= 0 or s_l <= 0 (no spread), or
 *                    d = 2: |H|_F^2 <= k^2 s_p s_l;  d = 3: |cof(H)|_F^2 <= k^4 (s_p s_l)^2, the sum of the squared 2 x 2
 *                    minors (rank below d - 1: all sighted landmarks at one point, at d = 3 all on one line).  A NaN refuses.
 *                    A refused chain keeps its rows (cost_final = cost_start, chosen 0); by the structural order it STILL
 *                    COUNTS AS PLACED for the stages after it: its sightings enter the later L-stages and the REFIT.
 *   apply            t_i <- R t_i + t and the stored block R_i^T <- R_i^T R^T for every position of the stage's chains.
 *   range rows       afterwards the unit range rows of ALL range measurements are recomputed in the direction of least
 *                    residual, as cora_place_chains_dev does, with its degenerate bytes and count.
 * cora_set_sighting_placement   validates, decides the order, translates the rows once and uploads.  The tables stay on the
 *            handle until replaced, until the measurement table or the chain tables are replaced or until the handle is
 *            destroyed.  Works on a plan-only handle, except for the upload.  A refused call leaves the tables as they were.
 * cora_sighting_placement_counts   out = {stages, sightings used (entries of all lists), chunks, skipped edges}.
 * cora_sighting_placement_order    stage_kind[stages]: 0 L | 1 C | 2 REFIT;  stage_ptr[stages + 1];  items[stage_ptr[stages]]:
 *            the landmarks (L, REFIT) or chains (C) of stage s at items[stage_ptr[s] .. stage_ptr[s + 1]), ascending; one
 *            item per list, and a list has at least one chunk: `chunks` entries always suffice.
 * cora_place_by_sightings_dev   out (host) = {chains placed (status 0), chains not placed (1, 2, 3), landmarks placed (0),
 *            landmarks not placed (1, 2), degenerate range rows, stages};  status, cost_start, cost_final, chosen: host
 *            arrays with one entry per chain or NULL (costs 0 and chosen -1 where the chain has no list);  transforms:
 *            [chains][d * d + d], R row-major then t as applied, the identity where nothing was applied;
 *            landmark_status, landmark_cost: one entry per landmark or NULL;  degenerate: host bytes, one per range
 *            measurement, or NULL.  Launches per stage: L-stage 2, C-stage 5, REFIT 2 + 2 for the landmarks' cost; then the
 *            range rows.  Everything on the handle's stream; synchronises once, at the end.
 * cora_place_by_sightings       the host-pointer form, in place: X is N x d column-major with leading dimension ldx.
 * cora_debug_place_by_sightings_host   the same on the host in the device's bracket order and through the functions the
 *            kernels call: X has the device's bits.  Works on a plan-only handle.
 * ARITHMETIC.  No transcendental function: + - x / and sqrt only, single correctly rounded fp64 operations in the order
 * written, never contracted.  Sums: the butterfly within a wavefront (lanes without an entry hold +0.0), the four
 * wavefronts of a chunk from the left, chunk sums as [sum][chunk]; one wavefront per list in which lane j adds chunks
 * j, j + 64, .. of the list from the left to +0.0, then the butterfly.  The same bits on every call.  No atomics on doubles.
 * ERRORS.  CORA_ERR_NOT_READY: no measurement table, no chain tables, or no sighting tables.  CORA_ERR_ARG: a partitioned
 * handle; min_sightings < d; a mask that fixes no chain; a null X or out; two range measurements that name one range row.
 * CORA_ERR_SHAPE: a leading dimension below N.  CORA_ERR_NAN: a sum or a range row that is not finite (the device forms
 * report it through the handle's flag word).  CORA_ERR_HIP: a device form on a plan-only handle.
 * STATE.  Nothing the handle computes with changes. */
int cora_set_sighting_placement(cora_ctx *ctx, const unsigned char *chain_fixed /* [chains] or NULL */,
                                const unsigned char *landmark_fixed /* [landmarks] or NULL */, int min_sightings);
int cora_sighting_placement_counts(const cora_ctx *ctx, int64_t out[4]);
int cora_sighting_placement_order(const cora_ctx *ctx, int32_t *stage_kind, int32_t *stage_ptr, int32_t *items);
int cora_place_by_sightings_dev(cora_ctx *ctx, double *dX, int64_t out[6], unsigned char *status, double *cost_start, double *cost_final,
                                int32_t *chosen, double *transforms, unsigned char *landmark_status, double *landmark_cost,
                                unsigned char *degenerate);
int cora_place_by_sightings(cora_ctx *ctx, double *X, int ldx, int64_t out[6], unsigned char *status, double *cost_start,
                            double *cost_final, int32_t *chosen, double *transforms, unsigned char *landmark_status,
                            double *landmark_cost, unsigned char *degenerate);
int cora_debug_place_by_sightings_host(cora_ctx *ctx, double *X, int ldx, int64_t out[6], unsigned char *status, double *cost_start,
                                       double *cost_final, int32_t *chosen, double *transforms, unsigned char *landmark_status,
                                       double *landmark_cost, unsigned char *degenerate);

/* ---- OUTLIER-ROBUST PLACEMENT FROM SIGHTINGS: a consensus vote in front of every fit ---------------------------------------
 * cora_place_by_sightings_dev with a vote that keeps a sighting credited to the wrong landmark (the data-association
 * outlier) out of the landmark means and out of the chains' rigid alignments.  Tables, stages (L / C / REFIT), lists,
 * 256-entry chunks, the origin (the list's first entry, inlier or not), the refusal rule, "cost must fall", the apply and
 * the range-row step are exactly those of cora_set_sighting_placement: there is no new set call, and the order still
 * depends on structure alone.  One finite barc2 > 0 is given: the threshold on tau |.|^2, the quantity cora_gnc_weights
 * thresholds for a sighting (no 1/2).
 * LANDMARK LISTS (L-stages and the REFIT).
 *   hypothesis       entry h proposes the landmark at its own prediction, y_h = p'_h = p_h - p_0.  Every entry is valid.
 *   score            r(h, j) = tau_j |y_h - p'_j|^2, the operations and order of the sighting cost of one entry.
 *   vote             vote(h) = #{ j : r(h, j) <= barc2 }.  A NaN is no vote.
 *   election         h* is the entry of largest vote, the lowest entry among equal votes.  consensus = vote(h*).
 *   no consensus     consensus < min_landmark_consensus (>= 1): landmark status 5.  The row is not touched.  By the
 *                    structural order the landmark STILL COUNTS AS PLACED for later C-stages, as a refused chain does: its
 *                    sightings then enter those lists as gross outliers, and the chains' vote is what excludes them.
 *   refit            inliers I = { j : r(h*, j) <= barc2 }, the vote's function and bits.  The plain mean is taken over I:
 *                    an entry outside I adds +0.0 for each of its terms, so the bracket order is the plain call's.
 *                    landmark_cost is summed over I.
 * CHAIN LISTS (C-stages), a list of L entries.
 *   sample           the sample of h is the entries (h + k s) mod L, k = 0 .. d-1, s = max(1, L / d): d distinct entries,
 *                    because L >= min_sightings >= d; a function of (h, L, d) alone.
 *   hypothesis       g_h = (R_h, t'_h): the sample's terms of the alignment's sums (their own tau, relative to the list's
 *                    origin) are added from the left in the order k = 0 .. d-1, starting from +0.0; then the plain chain
 *                    solve runs, refusal rule included.  VALID where that solve is not refused and the result is finite.
 *                    Two sample entries that sight one landmark, or at d = 3 three landmarks on a line, are filtered by the
 *                    plain rule.  An invalid hypothesis has vote 0 and sets no flag.
 *   score            r(h, j) = tau_j |R_h p'_j + t'_h - l'_j|^2, the function and bits of the plain call's cost at g.
 *   vote, election, inliers   as above.  A list without a valid hypothesis elects entry 0 with consensus 0.
 *   no consensus     consensus < min_chain_consensus (>= 1): chain status 5, "taken, no consensus".  The chain keeps its
 *                    rows (chosen 0, the identity).  It counts as placed for later stages, as status 2 does.
 *   refit            the plain sums, solve (status 2 still possible) and the two costs over I only, with the same +0.0 rule.
 *                    The chain moves only where the cost over I falls.  One election, one refit.
 * LIMIT.  There is one hypothesis per entry.  It is clean only where all d entries of its sample are, a share (1 - eps)^d
 * of the hypotheses at an outlier fraction eps: the vote finds the consensus as long as ONE clean sample exists, but with
 * L (1 - eps)^d below about 1 no hypothesis may be clean and the list ends without consensus (status 5) or, worse, elects a
 * hypothesis a group of consistent outliers supports.  Landmark lists have d = 1 in this count.
 * cora_place_by_sightings_robust_dev   the arguments of cora_place_by_sightings_dev plus barc2, min_chain_consensus and
 *            min_landmark_consensus.  out (host, 10 fields) = the plain call's six, then {chains without consensus (status 5;
 *            not among "not placed"), landmarks without consensus in the REFIT, C-list entries outside I, REFIT entries
 *            outside I}.  New arrays, each NULL-allowed:  chain_consensus, chain_list_len [chains] (0 without a list);
 *            landmark_consensus, landmark_list_len [landmarks], the REFIT's;  inlier_chain [n_edges]: 1 in I of its C list,
 *            0 in a C list outside I, 2 in no C list;  inlier_landmark [n_edges]: the same for the REFIT lists (the L-stages'
 *            flags are superseded by the REFIT's: an L-stage's list is a part of the REFIT's list of the same landmark).  A
 *            list of status 5 reports the inliers of its elected hypothesis all the same.
 *            Launches per stage: L-stage 4 (vote, elect, masked pass and fold), REFIT 4 + 2 for the landmarks' cost, C-stage 8
 *            (hypotheses, vote, elect, masked pass and fold of the sums and of the costs, apply); then the range rows.  The
 *            chain hypotheses are a launch of their own into a workspace the vote reads.  The votes, the hypotheses, the
 *            elected hypotheses and the inlier bytes are scratch of the tables, allocated with them.  Everything on the
 *            handle's stream; synchronises once, at the end.
 * cora_place_by_sightings_robust       the host-pointer form.
 * cora_debug_place_by_sightings_robust_host   the mirror: the device's bits, on a plan-only handle too.
 * ARITHMETIC.  The plain section's: + - x / and sqrt only, never contracted; the votes are integers; no atomics on doubles;
 * the launches are the only synchronisation between workgroups.  A list in which every entry is an inlier has the plain
 * call's bits.
 * ERRORS.  The plain call's, plus CORA_ERR_ARG: barc2 not finite or <= 0, a minimum < 1;  CORA_ERR_NAN: an elected hypothesis
 * that is not finite.
 * STATE.  Nothing the handle computes with changes, nor its tables. */
int cora_place_by_sightings_robust_dev(cora_ctx *ctx, double *dX, double barc2, int min_chain_consensus, int min_landmark_consensus,
                                       int64_t out[10], unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen,
                                       double *transforms, unsigned char *landmark_status, double *landmark_cost, unsigned char *degenerate,
                                       int32_t *chain_consensus, int32_t *chain_list_len, int32_t *landmark_consensus,
                                       int32_t *landmark_list_len, unsigned char *inlier_chain, unsigned char *inlier_landmark);
int cora_place_by_sightings_robust(cora_ctx *ctx, double *X, int ldx, double barc2, int min_chain_consensus, int min_landmark_consensus,
                                   int64_t out[10], unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen,
                                   double *transforms, unsigned char *landmark_status, double *landmark_cost, unsigned char *degenerate,
                                   int32_t *chain_consensus, int32_t *chain_list_len, int32_t *landmark_consensus,
                                   int32_t *landmark_list_len, unsigned char *inlier_chain, unsigned char *inlier_landmark);
int cora_debug_place_by_sightings_robust_host(cora_ctx *ctx, double *X, int ldx, double barc2, int min_chain_consensus,
                                              int min_landmark_consensus, int64_t out[10], unsigned char *status, double *cost_start,
                                              double *cost_final, int32_t *chosen, double *transforms, unsigned char *landmark_status,
                                              double *landmark_cost, unsigned char *degenerate, int32_t *chain_consensus,
                                              int32_t *chain_list_len, int32_t *landmark_consensus, int32_t *landmark_list_len,
                                              unsigned char *inlier_chain, unsigned char *inlier_landmark);

/* ---- PLACEMENT FROM INTER-CHAIN RELATIVE-POSE EDGES (closures), on the device ------------------------------------------------
 * Moves whole odometry chains by one rigid motion each so that the relative-pose edges BETWEEN chains (inter-robot loop
 * closures, rendezvous, closures across a gap in one robot's odometry) are met, in place; the solve is closed-form and
 * the global minimiser of the list's cost.  Needs a measurement table (cora_set_measurements), chain tables
 * (cora_set_odometry_chains) and the tables of cora_set_closure_placement.
 * DEFINITIONS.
 *   closure          an edge of the measurement table with a rotation part (second rotation row >= 0) that is no edge of an
 *                    odometry chain and whose two poses are positions of two DIFFERENT chains.  Every other non-chain edge
 *                    with a rotation part (both ends in one chain, an end in a free pose) is skipped and counted; edges
 *                    without a rotation part (sightings, priors on a position) are no relative-pose edges and are not counted.
 *   motion           g = (G, s) of a chain: t_i <- G t_i + s, R_i <- G R_i, the stored block X_i <- X_i G^T.
 *   P, q, l          of a closure between a placed and the moving chain, from the vector as it stands:
 *                      a placed, b moving:  P = X_a^T R X_b,      q = x_t(b),            l = x_t(a) + R_a t
 *                      a moving, b placed:  P = X_b^T R^T X_a,    q = x_t(a) + R_a t,    l = x_t(b)
 *                    so that the edge's residuals after the motion are kappa |G - P|_F^2 and tau |G q + s - l|^2.
 *   closure cost     of a list: J(G, s) = sum kappa |G - P|_F^2 + sum tau |G q + s - l|^2.
 *   order            decided once on the host from structure alone.  Placed: chain_fixed, NULL: chain 0.  Stage k takes
 *                    EVERY unplaced chain with at least min_closures closures against chains placed BEFORE stage k; its list
 *                    is those closures in table order, cut into chunks of 256, none across two lists; all lists of a stage
 *                    share its launches; repeated until a stage takes nothing.  Closures between two chains taken in the
 *                    same stage, or to a chain never placed, are unused and counted.  min_closures >= 1.
 *   solve            relative to the list's first entry, q' = q - q_0, l' = l - l_0, W = sum tau, K = sum kappa:
 *                    H = sum kappa P + sum tau l' q'^T - (sum tau l')(sum tau q')^T / W (the last two dropped where W <= 0),
 *                    G = round_rotation(H) (maximises tr(G^T H)), s' = (sum tau l') / W - G (sum tau q') / W (0 where
 *                    W <= 0), s = s' + l_0 - G q_0.  A second pass evaluates the cost at the identity (cost_start: the sum
 *                    of the table's own rot + trans residuals of the list's edges) and at g (kappa |G - P|^2 + tau |G q' +
 *                    s' - l'|^2); g is applied only where its cost is below cost_start (chosen 1, cost_final the cost at g);
 *                    otherwise the rows are not touched (chosen 0, cost_final = cost_start).  cost_final <= cost_start.
 *   status           0 placed | 1 never taken (inter-chain closures, but too few against placed chains) | 2 taken, refused
 *                    by the device | 3 no inter-chain closure at all | 4 fixed.
 *   refusal          a function of the sums alone; a NaN refuses.  With the centred spreads s_q = sum tau |q'|^2 - |sum tau
 *                    q'|^2 / W and s_l likewise (0 where W <= 0), S = K sqrt(d) + sqrt(max(s_q, 0) max(s_l, 0)) (an upper
 *                    bound of |H|_F) and k = 1e-6: refused where K <= 0 and W <= 0; where K <= 0 and s_q <= 0 or s_l <= 0;
 *                    d = 2: |H|_F^2 <= k^2 S^2;  d = 3: |cof(H)|_F^2 <= k^4 S^4.  A refused chain keeps its rows; by the
 *                    structural order it STILL COUNTS AS PLACED for the stages after it.
 *   range rows       afterwards the unit range rows of ALL range measurements are recomputed in the direction of least
 *                    residual, as cora_place_by_sightings_dev does, with its degenerate bytes and count.
 * cora_set_closure_placement   validates, decides the order and uploads.  The tables stay on the handle until replaced, until
 *            the measurement table or the chain tables are replaced or until the handle is destroyed.  Works on a plan-only
 *            handle, except for the upload.  A refused call leaves the tables as they were.
 * cora_closure_placement_counts   out = {stages, closures used (entries of all lists), chunks, skipped + unused edges}.
 * cora_closure_placement_order    stage_ptr[stages + 1];  items[stage_ptr[stages]]: the chains of stage s at
 *            items[stage_ptr[s] .. stage_ptr[s + 1]), ascending; `chunks` entries always suffice.
 * cora_place_by_closures_dev   out (host) = {chains placed (status 0), chains not placed (1, 2, 3), degenerate range rows,
 *            stages, chains refused (2)};  status, cost_start, cost_final, chosen: host arrays with one entry per chain or
 *            NULL (costs 0 and chosen -1 where the chain has no list);  transforms: [chains][d * d + d], G row-major then s
 *            as applied, the identity where nothing was applied;  degenerate: host bytes, one per range measurement, or
 *            NULL.  5 launches per stage whatever the number of chains in it, then 2 for the range rows.  Everything on the
 *            handle's stream; synchronises once, at the end.
 * cora_place_by_closures       the host-pointer form, in place: X is N x d column-major with leading dimension ldx.
 * cora_debug_place_by_closures_host   the same on the host in the device's bracket order and through the functions the
 *            kernels call: X has the device's bits.  Works on a plan-only handle.
 * ARITHMETIC.  As the sighting placement's: + - x / and sqrt only, single correctly rounded fp64 operations in the order
 * written, never contracted; the same order of the sums; the same bits on every call; no atomics on doubles.
 * ERRORS.  CORA_ERR_NOT_READY: no measurement table, no chain tables, or no closure tables.  CORA_ERR_ARG: a partitioned
 * handle; min_closures < 1; a mask that fixes no chain; a null X or out; two range measurements that name one range row.
 * CORA_ERR_SHAPE: a leading dimension below N.  CORA_ERR_NAN: a sum or a range row that is not finite (the device forms
 * report it through the handle's flag word).  CORA_ERR_HIP: a device form on a plan-only handle.
 * STATE.  Nothing the handle computes with changes. */
int cora_set_closure_placement(cora_ctx *ctx, const unsigned char *chain_fixed /* [chains] or NULL */, int min_closures);
int cora_closure_placement_counts(const cora_ctx *ctx, int64_t out[4]);
int cora_closure_placement_order(const cora_ctx *ctx, int32_t *stage_ptr, int32_t *items);
int cora_place_by_closures_dev(cora_ctx *ctx, double *dX, int64_t out[5], unsigned char *status, double *cost_start, double *cost_final,
                               int32_t *chosen, double *transforms, unsigned char *degenerate);
int cora_place_by_closures(cora_ctx *ctx, double *X, int ldx, int64_t out[5], unsigned char *status, double *cost_start,
                           double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate);
int cora_debug_place_by_closures_host(cora_ctx *ctx, double *X, int ldx, int64_t out[5], unsigned char *status, double *cost_start,
                                      double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate);

/* Outlier-robust placement from closures: a consensus vote over minimal hypotheses in front of the closed-form fit (DESIGN
 * 7o).  Closures are the measurement kind most likely to be grossly wrong (perceptual aliasing), and one wrong closure among
 * ten drags the least-squares fit of cora_place_by_closures_dev away from all ten.  The tables, the stages, the lists and the
 * 256-entry chunks are exactly those of cora_set_closure_placement: there is no new set call, and the order still depends on
 * structure alone.  Per list of a stage, with (q_0, l_0) the list's first entry's (an origin only, whether or not that entry
 * turns out to be an inlier):
 *   hypothesis       entry h is VALID where kappa_h > 0 and then proposes g_h = (G_h, s_h): G_h = P_h as computed from the rows
 *                    (not rounded: a product of three orthogonal blocks), s'_h[a] = (l_h[a] - l_0[a]) - sum_k G_h[a][k]
 *                    (q_h[k] - q_0[k]) (k ascending from +0.0), s_h = (s'_h + l_0) - G_h q_0.
 *   residual         r(h, j) = kappa_j |G_h - P_j|_F^2 + tau_j |G_h q'_j + s'_h - l'_j|^2: the coupled rot + trans residual of
 *                    edge j after the motion g_h, the quantity cora_gnc_weights thresholds for a coupled edge (no 1/2); the
 *                    function and the bits of the plain placement's cost at g.
 *   vote             vote(h) = #{ j in the list : r(h, j) <= barc2 }; a NaN is no vote; an invalid h has vote 0; an entry
 *                    with kappa = 0 still votes for others where its translation part agrees.  barc2: one finite scalar > 0.
 *   election         h* = the entry of largest vote, among equal votes the lowest entry of the list; consensus = vote(h*).
 *                    consensus < min_consensus (min_consensus >= 1): status 5, "taken, no consensus"; the chain keeps its
 *                    rows (chosen 0, the identity) and, like a refused chain, STILL COUNTS AS PLACED for later stages.
 *   inliers          I = { j : r(h*, j) <= barc2 }, the same function and bits as the vote.
 *   refit            the plain placement's sums, solve (its refusal rule unchanged: status 2 is still possible), and two costs
 *                    over the entries of I only.  AN ENTRY OUTSIDE I ADDS +0.0 FOR EACH OF ITS TERMS (it is not skipped: the
 *                    bracket order of every sum is the plain placement's, a lane beyond a chunk's end adds the same +0.0).
 *                    The chain moves only where the cost over I falls; cost_start and cost_final are over I.  One refit, no
 *                    re-election.
 *   cost             L^2 residual evaluations per list of L entries, by design: every entry is a hypothesis.
 * out = the plain call's five fields, then {chains without consensus (status 5; they are not among out[1]), entries outside I
 * summed over all lists}.  status, cost_start, cost_final, chosen, transforms: as the plain call's, NULL allowed.  consensus
 * [chains]: the vote of the elected entry, 0 where the chain was not taken;  list_len [chains]: the entries of the chain's
 * list, 0 without one;  inlier [n_edges]: 1 in I of its list | 0 in a list, outside I | 2 in no list;  each NULL allowed.  7
 * launches per stage (vote, elect, pass, fold, pass, fold, apply), then 2 for the range rows (their degenerate count is
 * out[2]).  cora_place_by_closures_robust: the host-pointer form.  cora_debug_place_by_closures_robust_host: the mirror, the
 * same functions in the same bracket order: the device's bits; works on a plan-only handle.
 * ERRORS.  The plain call's; CORA_ERR_ARG also for barc2 not finite or <= 0 and for min_consensus < 1; CORA_ERR_NAN also for a
 * valid or elected hypothesis that is not finite.  STATE.  Nothing the handle computes with changes, nor its tables. */
int cora_place_by_closures_robust_dev(cora_ctx *ctx, double *dX, double barc2, int min_consensus, int64_t out[7], unsigned char *status,
                                      double *cost_start, double *cost_final, int32_t *chosen, double *transforms, int32_t *consensus,
                                      int32_t *list_len, unsigned char *inlier);
int cora_place_by_closures_robust(cora_ctx *ctx, double *X, int ldx, double barc2, int min_consensus, int64_t out[7], unsigned char *status,
                                  double *cost_start, double *cost_final, int32_t *chosen, double *transforms, int32_t *consensus,
                                  int32_t *list_len, unsigned char *inlier);
int cora_debug_place_by_closures_robust_host(cora_ctx *ctx, double *X, int ldx, double barc2, int min_consensus, int64_t out[7],
                                             unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms,
                                             int32_t *consensus, int32_t *list_len, unsigned char *inlier);

/* Timing helpers: HIP events on the handle's stream. */
int cora_timer_start(cora_ctx *ctx);
int cora_timer_stop_ms(cora_ctx *ctx, float *ms); /* synchronises */
int cora_sync(cora_ctx *ctx);

/* Test hook: executes the handle's device FORMAT (slices + long rows) on the
 * host, to validate the format conversion where no GPU exists.  Never used by
 * any compute entry point. */
/* A factor of the caller's own for the handle's vectors: (L L^T)^-1 with L (CSC, diagonal first) the Cholesky-form
 * factor of P A P^T, N rows, perm new -> old in API row order.  It may be INCOMPLETE (dropped entries).  Used by
 * fast_verification for the preconditioner of src/CORA_utils.cpp:140-156 (ILDL with pos_def_mod: L |D|^(1/2)).
 * cora_aux_solve_dev: dX = (P^T L L^T P)^-1 dB on k-column resident vectors, dB != dX.
 * Partitioned handle: the factor of the RANK'S OWN rows (m = its row count, perm holds its API rows): the solve is
 * block Jacobi over the ranks, like cora_precond_set_cholesky, and touches the rank's rows only. */
int cora_aux_set_cholesky(cora_ctx *ctx, int m, const int32_t *Lp, const int32_t *Li, const double *Lx,
                          const int32_t *perm);
int cora_aux_solve_dev(cora_ctx *ctx, const double *dB, int k, double *dX);

/* ------------------------------------------------ multi-GPU: injected communication
 *
 * A partitioned handle (cora_ctx_create_part, world > 1) owns the rows of its shard; every resident vector still
 * has cora_rows() rows, of which only the shard is kept current.  The library links no collective library: the
 * three steps that need other ranks are callbacks (RCCL through torch.distributed in bench.py, gloo or threads in
 * the tests).  With them installed every entry point of the resident API is collective -- all ranks call the same
 * sequence -- and the C++ host above (TNT, LOBPCG, solveCORA) runs unchanged, one process per GPU:
 *   exchange : make the rows of dX that this rank's part of Q reads (cora_remote_rows) current; called before
 *              every product (src/CORA_problem.cpp:742-746 and its callers), on the handle's stream
 *   allreduce: sum n host doubles over the ranks in place (inner products src/CORA.cpp:119-122, the cost
 *              src/CORA_problem.cpp:759-762, Gram matrices of LOBPCG); must return the SAME bits on every rank
 *   allgather: make every row of dX current on every rank (before a download)
 * Without callbacks a partitioned handle leaves both to the caller (operands current where read, results are
 * per-rank partial sums).  Each returns 0 on success.  Work they enqueue must be ordered after the work already on the handle's stream
 * (they may synchronise it) and complete, or be ordered on that stream, when they return. */
typedef int (*cora_exchange_fn)(void *user, double *dX, int ld);
typedef int (*cora_allreduce_fn)(void *user, double *vals, int n);
typedef int (*cora_allgather_fn)(void *user, double *dX, int ld);
int cora_set_comm(cora_ctx *ctx, cora_exchange_fn exchange, cora_allreduce_fn allreduce, cora_allgather_fn allgather,
                  void *user);
/* on != 0: a collective step on this (partitioned) handle without communication installed fails with
 * CORA_ERR_NOT_READY instead of being left to the caller.  CORA::Problem sets it on the handles it creates for a
 * partition, so that a rebuilt handle cannot silently compute per-rank partial results. */
int cora_require_comm(cora_ctx *ctx, int on);
/* 1 if cora_stpcg_dev / cora_stpcg_warm_dev can run on this handle: always on one GPU; on a partitioned handle with
 * the library's own communication as the ACTIVE transport (cora_comm_create_*: the inner products are all-reduced on
 * the device, no host round trip), the explicit formulation and up to 12 columns.  Preconditioners on a partitioned
 * handle: none, Jacobi, or a Cholesky factor of the rank's OWN diagonal block of Q + lambda I installed with
 * cora_precond_set_cholesky -- block Jacobi over the ranks with exact blocks, NOT the reference's one global factor
 * (a sequential solve does not shard; expect more inner iterations than on one GPU). */
int cora_stpcg_device_ok(const cora_ctx *ctx);
/* The library's OWN communication for a partitioned handle: the three steps above implemented natively, so that no
 * callback (and no Python) sits on the data path.  Two transports:
 *   RCCL : one process per GPU.  Rank 0 calls cora_rccl_unique_id (128 bytes), the launcher hands the bytes to every
 *          rank (torch.distributed broadcast in bench.py, MPI_Bcast, a file), every rank calls cora_comm_create_rccl:
 *          collective.  The exchange is pack kernel -> ncclAllGather -> scatter kernel, the reductions ncclAllReduce,
 *          all on the handle's stream.  librccl.so is opened at run time: single-GPU users do not depend on it.
 *   local: every rank a thread of one process with its own handle (tests on a one-GPU box; several GPUs of one process):
 *          cora_local_group_create(world) once, cora_comm_create_local(handle, group) from every rank's thread.
 * Both replace whatever cora_set_comm installed; the communicator is destroyed with the handle.
 * cora_comm_exchanged_rows: rows a rank receives per exchange (world x the longest export list). */
typedef struct cora_local_group cora_local_group;
int cora_rccl_unique_id(void *id128);
int cora_comm_create_rccl(cora_ctx *ctx, const void *id128);
cora_local_group *cora_local_group_create(int world);
void cora_local_group_destroy(cora_local_group *group);
void cora_local_group_abort(cora_local_group *group); /* a rank failed outside the library: release the others */
int cora_comm_create_local(cora_ctx *ctx, cora_local_group *group);
/* Third transport (round 6; SURVEY 8e mitigation 3: "one-shot direct all-gather"): DEVICE-SIDE collectives over peer-mapped
 * mailboxes, no RCCL and no host on the data path (cora_amd/csrc/p2p.h).  The exchange of a product is under 1 KB per rank
 * and the reductions of an STPCG iteration are 1-3 doubles, so a collective is ONE small kernel on the handle's stream: it
 * writes its payload into every peer's mailbox (stores over xGMI; the mailbox is exported with hipIpcGetMemHandle and mapped
 * by the peers, or shared by pointer between threads of one process), sets a per-(receiver, sender) sequence flag with
 * release at system scope, spins on the flags of its OWN mailbox (with a wall-clock timeout, CORA_P2P_TIMEOUT_S, default 60:
 * a dead peer raises an error count instead of hanging the GPU, and every later collective call of that rank fails with
 * CORA_ERR_HIP instead of computing on what the timed-out one delivered) and delivers -- all-reduces add in rank order, the same bits
 * as the other transports.  Ranks: one process per GPU, several processes sharing a GPU (tests), or threads.
 *   cora_comm_p2p_handle(ctx, blob)   -> creates this rank's mailbox, blob = CORA_P2P_HANDLE_BYTES to hand to the peers
 *   (launcher: all-gather of the blobs in rank order -- torch.distributed, MPI, a file; like the RCCL id)
 *   cora_comm_create_p2p(ctx, blobs)  -> collective: maps the peers, plans the exchange
 * cora_comm_counters stays at 0 + 0 on this transport (no library collective is issued); cora_comm_p2p_status:
 * out[0] collectives, [1] kernels launched for them, [2] timeouts raised, [3] mailbox memory (0 uncached, 1 fine-grained,
 * 2 ordinary; -1 no p2p transport), [4] all-gathers, [5] all-reduces. */
#define CORA_P2P_HANDLE_BYTES 128
int cora_comm_p2p_handle(cora_ctx *ctx, void *blob);
int cora_comm_create_p2p(cora_ctx *ctx, const void *blobs);
int cora_comm_p2p_status(const cora_ctx *ctx, long out[6]);
int64_t cora_comm_exchanged_rows(const cora_ctx *ctx);
/* Rows of resident vectors received through all-gathers of whole shards or of packed pieces so far (library's own
 * communication): the implicit formulation's replicated translation solve gathers the translation rows alone
 * (world x the longest shard's translation rows per product), not whole shards. */
long long cora_comm_gathered_rows(const cora_ctx *ctx);
/* What the handle's RCCL communicator itself reports: out[0] = ncclCommCount, out[1] = ncclCommUserRank (-1, -1 without an
 * RCCL communicator).  cora_comm_create_rccl fails when they differ from the handle's partition. */
int cora_comm_rccl_ranks(const cora_ctx *ctx, int out[2]);
/* Measurement switch: on = 0 leaves the collective steps to the caller again (a product then runs on whatever the
 * remote rows hold: bench.py times the kernel alone this way), on = 1 re-installs the native communication. */
int cora_comm_native_enable(cora_ctx *ctx, int on);
/* Collectives the library's own communication has issued on this handle so far: out[0] all-gathers, out[1] all-reduces.
 * A product is ONE all-gather (the exported rows of the operand and the distributed long rows' partial sums travel
 * together; the owners add the sums up in rank order); an iteration of the device-resident STPCG is that plus two
 * all-reduces (kappa; <r,r> and <r,v>): the two synchronisation points of preconditioned CG. */
int cora_comm_counters(const cora_ctx *ctx, long out[2]);

/* The phases of a partitioned handle's product, timed with HIP events on the handle's stream (library's own
 * communication, serial order; collective: every rank calls it): us[0] pack of the exported rows, [1] the distributed
 * long rows' chunks, [2] the all-gather, [3] unpack (rows scattered, long rows summed), [4] the slices.  epi: 0 Q X,
 * 1 (Q - Lambda) X, 2 the Hessian-vector product.  What a first run on several GPUs is read with (bench.py --gpus N). */
int cora_debug_product_phases(cora_ctx *ctx, const double *dX, double *dOut, int epi, int reps, double us[5]);

/* Test hook (process-wide): the pose slices of a product read X through their LDS windows from this many slices on
 * (default 2 048 = the wavefronts resident at once; below, every wavefront is resident and gathers directly).  Returns
 * the previous value; a negative argument only queries.  Results do not depend on it. */
int cora_debug_spmm_window_min_slices(int min_slices);
/* Test hooks (process-wide) of the staggered start of the window form: a pose slice that is the second wavefront on its
 * SIMD issues its first load `ticks` x 10 ns late (CORA_SPMM_STAGGER_TICKS; stored clamped to 0 .. 2 000, 0 = off).
 * The library applies the delay only to launches of the size and the row strides it was measured at; on = 1 applies
 * it to every window-form launch, on = 2 also makes EVERY pose slice wait (a small launch leaves no SIMD with two).
 * Each returns the previous value; a negative argument only queries.  Results do not depend on either. */
int cora_debug_spmm_stagger_ticks(int ticks);
int cora_debug_spmm_stagger_force(int on);

/* Timing hook: with on != 0 the products of a partitioned handle skip every collective step (the operand's remote rows
 * are whatever they are, the distributed long rows stay partial sums) -- the kernel alone, for bench.py's roofline leg. */
int cora_debug_local_products(cora_ctx *ctx, int on);

/* With the native communication a product of a partitioned handle overlaps the exchange of its operand with the
 * slices that read this rank's own rows only: exchange (pack, all-gather, scatter) on a second stream, interior
 * slices + long-row chunks at the same time on the handle's stream, boundary slices when the exchange has landed.
 * on = 0: always the serial order (exchange, then one launch); on = 1 (default): the split from 2 048 interior slices
 * per rank on (CORA_EXCHANGE_OVERLAP_MIN_SLICES) -- below, a second launch and two cross-stream dependencies cost more
 * than the interior slices take; on = 2: always the split.  The results are the same numbers either way.
 * cora_comm_overlap_active: 1 when products of this handle take the overlapped form. */
int cora_comm_overlap_enable(cora_ctx *ctx, int on);
int cora_comm_overlap_active(const cora_ctx *ctx);
/* Building blocks of an exchange, on the handle's stream: dPacked[k] = dX[rows[k]], dX[rows[k]] = dPacked[k],
 * dDst[rows[k]] = dSrc[rows[k]] (rows: device array of n internal rows; ld = row stride in doubles). */
int cora_pack_rows_dev(cora_ctx *ctx, const double *dX, int ld, const int32_t *d_rows, int64_t n, double *dPacked);
int cora_scatter_rows_dev(cora_ctx *ctx, const double *dPacked, int ld, const int32_t *d_rows, int64_t n, double *dX);
int cora_copy_rows_dev(cora_ctx *ctx, const double *dSrc, int ld, const int32_t *d_rows, int64_t n, double *dDst);
/* dDst[rows of shard `shard`] = dSrc[the same rows] (one contiguous block of cora_shard_rows() rows) */
int cora_copy_shard_dev(cora_ctx *ctx, const double *dSrc, int ld, int shard, double *dDst);
int cora_rank(const cora_ctx *ctx);
int cora_world(const cora_ctx *ctx);

/* Measurement hook (bench.py): HIP event pairs around the Hessian-vector product of every iteration of
 * cora_stpcg_dev, i.e. the product as it runs INSIDE the solver loop, with the preconditioner's traffic between
 * two of them (the back-to-back figure keeps Q in the Infinity Cache). */
int cora_debug_profile_stpcg(cora_ctx *ctx, int on);
int cora_debug_stpcg_hvp_us(cora_ctx *ctx, double *mean_us, int *count);
/* on = 2: events around EVERY launch of the sweep-fused iteration (one GPU).  us[k], mean over the iterations of the
 * last cora_stpcg_dev that ran: 0 product with the kappa partials | 1 kappa | 2 forward sweep | 3, 4 the last stage's
 * two products | 5 backward sweep | 6 two events in a row with nothing between them (what an event costs the stream:
 * every figure carries it); -1 where nothing was recorded.  us[7] = 1 when kappa had no launch of its own (folded into the
 * forward sweep: us[1] is then another measurement of the event's cost). */
int cora_debug_stpcg_phase_us(cora_ctx *ctx, double us[8]);
/* Form of the iteration the last cora_stpcg_dev ran: 0 one pass per operation, 1 fused vector passes, 2 vector passes
 * fused into the sweeps of the Cholesky solve (tests pin which form they compare). */
int cora_debug_stpcg_path(const cora_ctx *ctx);
/* OPT-IN (CORA_STPCG_GRAPH=1; off by default -- measured slower on this part, see stpcg_run in capi.hip): batches of
 * device-resident STPCG iterations captured once as a hipGraph and replayed (one GPU, fused forms).
 * out[0] = graphs captured so far, out[1] = batches replayed (both 0 unless the switch is on). */
int cora_debug_stpcg_graph(const cora_ctx *ctx, long out[2]);
/* Test hook: device and pinned blocks the handles of this process hold now (allocated and not yet freed), the native
 * transports' own blocks apart.  Process-wide; 0 once every handle is destroyed. */
int64_t cora_debug_live_allocations(void);
/* EVERY environment variable the library reads: the table of cora_amd/csrc/config.h, the only place that reads them
 * (tests/test_config_cpu.py checks that this list names the same variables).  NONE changes what is computed beyond the
 * rounding of a different (equally valid) order of operations.  A switch ("=1") is on when the variable is set to a
 * non-empty value that does not start with 0; numbers are clamped to their range.  [once]: read at first use and kept for
 * the life of the process; every other variable is read each time a call needs it.
 *
 * Forms of the STPCG iteration (all tested against each other, tests/test_gpu_solver.py):
 *   CORA_NO_FUSE=1            one pass per operation instead of the fused vector passes
 *   CORA_NO_SWEEP_FUSE=1      vector passes are not folded into the sweeps of the two-stage Cholesky solve
 *   CORA_NO_INVERSE_FUSE=1    ... nor into the two products of a one-explicit-inverse plan
 *   CORA_NO_RESIDUAL_SLOTS=1  [once] the one-explicit-inverse iteration finishes <r, r> with a ticket in its residual pass
 *   CORA_NO_KAPPA_FOLD=1, CORA_KAPPA_FOLD_MAX=n (4096) [once]   kappa = <p, Hp> gets a launch of its own (always | above n
 *                             partials)
 *   CORA_NO_TNT_FUSE=1        cora_tnt_accept_dev forms Q X again instead of taking the trial's
 * Host loop of cora_stpcg_dev (same numbers, tests run one problem under each):
 *   CORA_STPCG_DEPTH=0|1      the host waits for every iteration | runs one whole iteration ahead (default: the next
 *                             iteration's product ahead on small problems, 0 at 10^5 poses and above)
 *   CORA_STPCG_AHEAD=0|1      forces the product-ahead form off | on
 *   CORA_STPCG_BATCH=n        n iterations enqueued, all waited for (the form partitioned handles always use)
 *   CORA_STPCG_GRAPH=1        opt-in hipGraph replay of batches (measured slower on this part)
 * Partitioned handles:
 *   CORA_NO_EXCHANGE_OVERLAP=1, CORA_EXCHANGE_OVERLAP_MIN_SLICES=n (2048) [once]   interior slices beside the exchange:
 *                             never | from n interior slices per rank
 *   CORA_IMPLICIT_WHOLE_GATHER=1   the implicit formulation gathers whole shards instead of the packed translation rows
 *   CORA_P2P_TIMEOUT_S=x      seconds a collective of the device-side transport waits for its peers (60, at least 0.001)
 * Format of Q and the product's launch (same products to rounding; bit-identical where the order of sums is unchanged):
 *   CORA_CHAIN_SLICES=0       [once] pose slices in the plain layout (all columns explicit)
 *   CORA_SLICE_LJF=0          no longest-first order of the slices inside an XCD's range
 *   CORA_SPMM_WINDOW_MIN_SLICES=n (2048) [once]   k_spmm's LDS-window form from n slices on
 *                             (cora_debug_spmm_window_min_slices overrides it)
 *   CORA_SPMM_STAGGER_TICKS=n (300, 0..2000) [once]   a pose slice that is the second wavefront on its SIMD issues its first
 *                             load n x 10 ns late (window form with an epilogue, 65 536 to 131 072 poses, row stride 5:
 *                             where it was measured to win); 0: off (cora_debug_spmm_stagger_ticks overrides it;
 *                             bit-identical products)
 *   CORA_FORMAT_THREADS=n, CORA_FORMAT_TIMING=1   host threads of the format builder; its phase times on stderr
 * Solve plan of a Cholesky factor (trisolve_build.cpp; every plan solves the same system, tests/test_trisolve_cpu.py):
 *   CORA_TRI_SUB=0            the explicit-stage form instead of the substitution blocks
 *   CORA_TRI_SN_CAP=n         rows per supernode whose diagonal block is inverted, 1-32 (default: 4 or 8 by tree height)
 *   CORA_TRI_UNFOLD_MIN=n     aux sums folded into the last stage's first product below n extra entries (2000000)
 *   CORA_TRI_THREADS=n, CORA_TRI_CHECK_ETREE=1, CORA_TRI_TIMING=1   builder threads; elimination tree computed both ways
 *                             and compared; phase times of set-up on stderr
 *   CORA_SUB_IO_LISTS=1       row I/O of the sweeps from index lists instead of run tables
 *   [once] lab tunables of the plan, with their defaults and ranges (tools/plan_sweep.sh):
 *   CORA_TRI_TOP_INV=n (2500000, >= 0)   entries of an inverse of what is left that make it the last stage
 *   CORA_TRI_SHORT_ROW=n (64, 8..2^30), CORA_TRI_WAVE_ROW=n (1024, 64..2^30), CORA_TRI_CHUNK=n (512, 64..2^30)
 *                             row classes of a product: 8 lanes | a wavefront per row | chunks of n entries
 *   CORA_TRI_SUB_ROWS=n (512, 32..2048), CORA_TRI_SUB_ENT=n (5000, 100..2^30)   rows and entries of a substitution block
 *   CORA_TRI_LANE_ENTRIES=n (8, 1..8), CORA_TRI_LEVEL_LANES=n (256, 64..256)   entries per lane, lanes per level
 *   CORA_TRI_SPLIT_MIN_ROWS=n (2^20, 1..2^30)   level chunks closed early from n rows on
 * Host factorisation and ordering (sparse_cholesky.cpp, CORA_problem.cpp; bit-identical factors in every setting):
 *   CORA_CHOL_THREADS=n, CORA_SYMBOLIC_THREADS=n, CORA_CHOL_NO_SYMBOLIC_CACHE=1, CORA_CHOL_NO_TRAILING_GROUP=1
 *   CORA_ND_LEAF=n            poses per leaf of the nested dissection, >= 1 (2 for the preconditioner, 8 for the
 *                             translation factor of the implicit formulation)
 *   CORA_REG_CHOLESKY_MAX_COND=x   kappa_max of the regularised preconditioner (1e6, src/CORA_problem.cpp:551)
 * solveCORA (host/CORA.cpp, CORA_utils.cpp):
 *   CORA_NO_CERT_PREPARE=1    the first certification's pattern work is not prepared beside the first TNT solve
 *   CORA_NO_CERT_SPECULATION=1   the eigensolver's first stage does not run beside the host's PSD test
 *   CORA_NO_PIVOT_SEED=1      (round 6) fast_verification keeps the reference's plain order after a failed factorisation --
 *                             LOBPCG from the bootstrap block, then the ILDL branch (src/CORA_utils.cpp:112-167) -- instead of
 *                             seeding the block with the failed pivot's direction of non-positive curvature
 *   CORA_TRACE_BITS=1         [once] the bits of every stage of the staircase on stdout (determinism bisection) */
/* The effective value of every variable above, one "NAME=value" line each, " (default)" appended where the variable is
 * unset (switches print 1 | 0).  Reading a [once] variable here fixes it as its first use would.  Writes at most len bytes
 * including the terminating NUL; returns the length of the whole text (a larger buffer is needed when >= len). */
int cora_debug_config(char *buf, int len);

int cora_debug_format_spmm_host(const cora_ctx *ctx, const double *X, int ldx,
                                int k, double *out, int ldo);

/* Test hook: builds the device solve plan (stages, explicit block inverses) of a Cholesky factor
 * L (CSC, diagonal first per column, m x m) and executes its products on the host, in launch order:
 * X = (L L^T)^-1 B for k column-major right-hand sides.  stats: [0] stages, [1] entries of the
 * block inverses, [2] nnz(L), [3] dense stage-0 blocks.  Never used by any compute entry point. */
int cora_debug_factor_solve_host(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, int k,
                                 const double *B, double *X, int64_t stats[4]);

/* Test hook: the shape of the solve plan of an INSTALLED factor -- which: 0 the preconditioner's, 1 the implicit
 * formulation's, 2 the aux factor's (CORA_ERR_NOT_READY where none is installed).  Recorded at the install, before the
 * host plan is dropped; no kernel and no dispatch depends on it.
 *   [0] stages | [1] form of stage 0: 0 a plain stage of row products (one stage: one explicit inverse), 1 dense
 *   wavefront blocks, 2 substitution blocks | [2] blocks of stage 0 | [3] rows of its largest block |
 *   substitution blocks: [4] rows of the largest tile (block rows + coupled rows), [5] level headers of the longest
 *   block, [6] lanes of the widest level, [7] most entries per lane | [8] 1: row I/O from run tables, 0: from index
 *   lists | [9] 1: the STPCG passes can be fused into the sweeps | [10] aux rows | [11] 1: the aux sums are a product of
 *   their own | [12] rows of the last stage | [13] the internal row every solve zeroes (-1: none) |
 *   over all row products of the plan: [14] 8-lane rows, [15] wavefront rows, [16] long rows, [17] their chunks,
 *   [18] most chunks of one row | [19] dynamic LDS bytes of a substitution launch at a row stride of 24 |
 *   [20] nnz(L) | [21] entries of the explicit inverses | [22] row products with all three row classes |
 *   [23] installs on this factor so far.
 * cora_debug_factor_plan_host: the same for a factor that is not installed anywhere -- the plan alone is built (rows in
 * their own order; aux_ok != 0 allows the substitution form, as every install does); [8], [9] and [23] are -1. */
int cora_debug_factor_shape(const cora_ctx *ctx, int which, int64_t out[24]);
int cora_debug_factor_plan_host(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, int aux_ok,
                                int64_t out[24]);

/* Test hook: a digest of the WHOLE solve plan of a factor that is not installed anywhere (built as by
 * cora_debug_factor_plan_host; group: NULL or m ids, variables with the same id >= 0 are kept together, as a handle passes
 * the rotation rows of a pose).  FNV-1a, members in declaration order (cora_amd/csrc/trisolve.h), every array preceded by
 * its length: out[0] over every integer, boolean, index and header, out[1] over the bits of every double.  Equal digests:
 * the kernels see the same plan. */
int cora_debug_factor_plan_digest(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, const int32_t *group,
                                  int aux_ok, uint64_t out[2]);

/* Test hook: what an INSTALL of a factor uploads, for a factor that is installed nowhere (no GPU needed): the solve plan
 * as above plus its device image (cora_amd/csrc/trisolve_image.h: block descriptors, I/O lists, tile positions, run tables,
 * row units, packed block lanes, chunk rows, over-read tails), walked in upload order.  row_of: NULL (variable i lives in
 * row i) or m internal rows; group as above; rows: rows of a vector (0: m) -- the aux rows of a substitution plan start
 * there; zero_row: the pinned row or -1; d, [rot0, rot1): the rows that are the d rotation rows of a pose each (the fused
 * projection's row units; rot0 == rot1: none).  digest: FNV-1a, per array its element size, its length and its bytes --
 * [0] integers, indices, descriptors and the scalar members of the kernels' argument blocks, [1] the bits of the doubles.
 * shape: the 24 fields of cora_debug_factor_shape, [8] and [9] as an install decides them, [23] = -1.  An install with the
 * same factor, rows, groups and layout reports the same shape and uploads arrays with this digest. */
int cora_debug_factor_image(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, const int32_t *row_of,
                            const int32_t *group, int aux_ok, int64_t rows, int32_t zero_row, int d, int64_t rot0, int64_t rot1,
                            uint64_t digest[2], int64_t shape[24]);

/* Test hook: the shape of the handle's format of Q in numbers, read from the host copy of the format (no GPU needed; no
 * kernel and no dispatch depends on it) -- what a test asserts before it claims to have reached a path:
 *   pose slices [0] in the chain layout, [1] in the plain layout | over the chain slices: [2] most general slots of a
 *   lane, [3] most tail pairs T of a slice, [4] most tail pairs of a lane, [5] slices with T > 64, [6] tail pairs whose
 *   columns another rank owns (0 on one GPU) | long rows (one or more chunks on this handle) that are [7] a pose's,
 *   [8] a landmark's translation row | [9] most chunks of one long row | [10] lanes of chain slices whose tail pairs lie
 *   on both sides of a multiple of 64 pairs of their slice's tail (the wavefront gathers a tail 64 pairs at a time). */
int cora_debug_format_shape(const cora_ctx *ctx, int64_t out[11]);

/* Test hooks: digests of the handle's WHOLE format of Q and of its source map (cora_values_map_build), read from the host
 * copies (no GPU needed; plan-only handles too).  FNV-1a over 64-bit words, every array preceded by its length.
 * cora_debug_format_digest: out[0] over every integer -- the layout, the counters, the row maps, every slice and chunk
 * descriptor, the column indices, both work orders --, out[1] over the bits of every double (slice and long-row values,
 * head values, sym(Q_PP), the diagonal).  Equal digests: the kernels see the same format.
 * cora_debug_value_map_digest: out[0] over the sources of the five value arrays, out[1] over the mirror pairs;
 * CORA_ERR_NOT_READY while the handle has no map. */
int cora_debug_format_digest(const cora_ctx *ctx, uint64_t out[2]);
int cora_debug_value_map_digest(cora_ctx *ctx, uint64_t out[2]);

/* Test hook: the DEVICE IMAGE of the long rows -- what a handle uploads for the chunk blocks of the product kernel in
 * place of the format's chunks --, derived from the host copy of the format (no GPU needed; plan-only handles too).  On
 * one GPU every long row's entries are sorted by the XCD (blockIdx % 8) whose slices own the entry's row of X ("home"),
 * cut at every change of home and into parts of at most `piece` entries (<= 0: the library's piece size), and every piece
 * is launched on its home; partitioned handles keep the format's chunks (sizes[4] = 0).
 *   sizes[5]: [0] pieces, [1] launch positions (8 x the longest XCD list), [2] entries, [3] rows of a vector, [4] placed
 *   chunks[sizes[0]][8]: row, k0, k1, nchunks, first, slot, 0, 0 -- [k0, k1) in lval / lcol below
 *   chunk_order[sizes[1]]: XCD x runs the pieces at [x cper, (x + 1) cper), cper = sizes[1] / 8; -1 = padding
 *   lval, lcol, perm[sizes[2]]: lval[i] = (format's lval)[perm[i]];  lcol: INTERNAL rows (cora_row_map)
 *   home, home_pose_first[sizes[3]]: home XCD of every internal row under the two slice orders, -1 = none
 * Every array pointer may be null (call once for the sizes).  CORA_ERR_NOT_READY while the host values are stale. */
int cora_debug_long_image(const cora_ctx *ctx, int piece, int64_t sizes[5], int32_t *chunks, int32_t *chunk_order,
                          double *lval, int32_t *lcol, int32_t *perm, int8_t *home, int8_t *home_pose_first);

#ifdef __cplusplus
}
#endif
#endif /* CORA_HIP_H_ */
