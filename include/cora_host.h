/*
 * cora_host.h -- flat C view of the C++ host (cora_amd/csrc/host: CORA::Problem,
 * parsePyfgTextToProblem, solveCORA ...).  The C++ host mirrors the reference's
 * own C++ interface (include/CORA/CORA.h:19-37, include/CORA/CORA_problem.h:
 * 67-416, include/CORA/pyfg_text_parser.h:31); this header only exists so that
 * tests/ and bench.py can drive it through ctypes.  All matrices are
 * column-major double with an explicit leading dimension.  Every function
 * returns 0 on success; cora_host_last_error() holds the C++ exception text.
 */
#ifndef CORA_HOST_H_
#define CORA_HOST_H_

#include <stdint.h>

#include "cora_hip.h" /* cora_exchange_fn, cora_allreduce_fn, cora_allgather_fn */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cora_problem cora_problem;

const char *cora_host_last_error(void);

/* parsePyfgTextToProblem (src/pyfg_text_parser.cpp:112) */
int cora_problem_from_pyfg(const char *path, cora_problem **out);
/* Synthetic generator of SURVEY 8(d); pyfg_out may be NULL. precond: cora_precond_kind */
int cora_problem_synthetic(int dim, int n_poses, int n_landmarks, int n_ranges, int n_loops, uint64_t seed,
                           int precond, const char *pyfg_out, cora_problem **out);
/* Programmatic construction, one call per add* method of CORA::Problem
 * (include/CORA/CORA_problem.h:202-262; used like tests/test_construct_problem.cpp:21-99).  Symbols are the
 * reference's strings ("x1", "L3", ...).  Matrices are column-major: R d x d, t / pos d, cov (d + rotation
 * dim) square for poses (translation block first, include/CORA/Measurements.h:60-63) and d x d for landmarks. */
int cora_problem_new(int dim, int rank, int implicit, int precond, cora_problem **out);
int cora_problem_add_pose(cora_problem *p, const char *id);
int cora_problem_add_landmark(cora_problem *p, const char *id);
int cora_problem_add_range(cora_problem *p, const char *a, const char *b, double dist, double cov);
int cora_problem_add_rel_pose(cora_problem *p, const char *a, const char *b, const double *R, const double *t,
                              const double *cov);
int cora_problem_add_rel_pose_landmark(cora_problem *p, const char *a, const char *b, const double *t,
                                       const double *cov);
int cora_problem_add_pose_prior(cora_problem *p, const char *id, const double *R, const double *t, const double *cov);
int cora_problem_add_landmark_prior(cora_problem *p, const char *id, const double *pos, const double *cov);

/* Same generator with explicit noise levels sigmas = {sigma_t, sigma_R, sigma_range} (NULL: the
 * defaults 0.05, 0.01, 0.1) and, when x_gt != NULL, the ground truth as a column-major
 * ((dim+1) n + l + r) x dim point ([R_i^T]; range bearings; translations) -- zero cost when all
 * sigmas are zero, which gives the tests a known global optimum at any size. */
int cora_problem_synthetic_ex(int dim, int n_poses, int n_landmarks, int n_ranges, int n_loops, uint64_t seed,
                              int precond, const double *sigmas, const char *pyfg_out, double *x_gt,
                              cora_problem **out);
void cora_problem_destroy(cora_problem *p);

/* Problem::updateProblemData (src/CORA_problem.cpp:500-510): assembles Q on the host. */
int cora_problem_update(cora_problem *p);
/* dims: [0] d, [1] poses, [2] landmarks, [3] ranges, [4] N, [5] nnz(Q), [6] pose-pose
 * measurements, [7] relaxation rank */
int cora_problem_dims(const cora_problem *p, int64_t dims[8]);
/* Borrowed CSR pointers of a matrix by name: "DataMatrix", "Arange", "OmegaRange",
 * "RangeDistances", "Apose", "OmegaPose", "T", "RotConLaplacian". */
int cora_problem_matrix(cora_problem *p, const char *name, int64_t *rows, int64_t *cols, int64_t *nnz,
                        const int32_t **rowptr, const int32_t **colidx, const double **vals);
/* Problem::get_certificate_matrix(Y) (src/CORA_problem.cpp:1162-1166): S = Q - Lambda(Y) as CSR, Y column-major with the
 * current relaxation rank's columns; the arrays stay valid until the next call on this problem. */
int cora_problem_certificate_matrix(cora_problem *p, const double *Y, int ldy, int64_t *rows, int64_t *nnz,
                                    const int32_t **rowptr, const int32_t **colidx, const double **vals);

int cora_problem_set_rank(cora_problem *p, int rank);
int cora_problem_set_preconditioner(cora_problem *p, int kind);
int cora_problem_set_device(cora_problem *p, int device);
/* Problem::setPartition (this build's multi-GPU entry, cora_amd/csrc/host/CORA_problem.h): the process owns
 * partition `rank` of `world` and communicates through the callbacks of cora_set_comm (include/cora_hip.h). */
int cora_problem_set_partition(cora_problem *p, int rank, int world, cora_exchange_fn exchange,
                               cora_allreduce_fn allreduce, cora_allgather_fn allgather, void *user);
/* Problem::setFormulation (include/CORA/CORA_problem.h:338): implicit != 0 selects
 * Formulation::Implicit, where the variable is the leading d*n + r rows (rotations and ranges)
 * and the translations are eliminated analytically (src/CORA_problem.cpp:714-753). */
int cora_problem_set_formulation(cora_problem *p, int implicit);
/* Problem::getExpectedVariableSize (src/CORA_problem.cpp:944-952) */
int cora_problem_variable_size(cora_problem *p, int64_t *rows);

/* Operators of CORA::Problem, by name (all run on the GPU):
 *  "evaluateObjective"        A=Y                -> out[0] (scalar)
 *  "Euclidean_gradient"       A=Y                -> out N x p
 *  "Riemannian_gradient"      A=Y                -> out
 *  "tangent_space_projection" A=Y, B=Ydot        -> out
 *  "Riemannian_Hessian_vector_product" A=Y, B=nablaF_Y, C=Ydot -> out
 *  "precondition"             A=V                -> out
 *  "projectToManifold"        A                  -> out
 *  "retract"                  A=Y, B=V           -> out
 *  "getRandomInitialGuess"    (none)             -> out
 *  "getOdomInitialization"    (none)             -> out   (examples/paper_experiments.cpp:426-534)
 *  "odometryInitialization"   (none)             -> out   the same start composed on the device (Problem::odometryInitialization,
 *                                                        seed 7: getOdomInitialization's start up to rounding)
 *  "rangeAidedInitialization" (none)             -> out   odometryInitialization with the landmarks placed from the ranges
 *                                                        (Problem::rangeAidedInitialization, seed 7, 5 Gauss-Newton steps)
 *  "rangeAidedInitializationConsensus" (none)    -> out   the same with the multilateration's consensus vote (RangeConsensus{100, 0})
 *  "multiRobotInitialization" (none)             -> out   rangeAidedInitialization with the chains first placed from the ranges
 *                                                        between them (Problem::multiRobotInitialization, seed 7, 5 steps, default min_ranges)
 *  "sightingInitialization"   (none)             -> out   multiRobotInitialization with landmarks and chains first placed from the
 *                                                        pose-landmark sightings (Problem::sightingInitialization, seed 7, defaults)
 *  "sightingInitializationConsensus" (none)      -> out   the same with the sighting step's consensus vote (SightingConsensus{1, 0, 1})
 *  "closureInitialization"    (none)             -> out   sightingInitialization with the chains first placed from the relative-pose
 *                                                        edges between chains (Problem::closureInitialization, seed 7, defaults)
 *  "getTranslationExplicitSolution" A=Y (implicit) -> out (d+1)n + r + l rows (src/CORA_problem.cpp:1168)
 *  "alignEstimateToOrigin"    A=Y (rank d)       -> out (d+1)n + r + l rows (src/CORA_problem.cpp:1234)
 * Inputs are N x cols with leading dimension N = cora_problem_variable_size() (cols is checked
 * against the relaxation rank by the C++ methods, like the reference's checkMatrixShape); the
 * output is N x rank unless stated otherwise. */
int cora_problem_op(cora_problem *p, const char *op, int cols, const double *A, const double *B,
                    const double *C, double *out);
/* Problem::odometryChains (an extension beyond the reference): the chains getOdomInitialization composes, as indices into
 * the relative-pose measurements in the order they were added.  counts = { chains, edges of all chains }; chain_ptr
 * (chains + 1 entries) and chain_edges may both be NULL to ask for the counts alone. */
int cora_problem_odometry_chains(const cora_problem *p, int64_t counts[2], int64_t *chain_ptr, int32_t *chain_edges);
/* Problem::rangeAidedInitialization (an extension beyond the reference; include/cora_hip.h, "landmark initialisation from
 * ranges").  out: data-matrix-size x rank.  counts = { landmarks solved, not solved, degenerate range rows, Gauss-Newton
 * steps taken }; status, cost_linear, cost_final: one entry per landmark.  Every array but out may be NULL.  In the explicit
 * formulation the result is passed through checkVariablesAreValid (an error off the manifold). */
int cora_problem_range_aided_initialization(cora_problem *p, uint64_t seed, int gn_steps, double *out, int64_t counts[4],
                                            unsigned char *status, double *cost_linear, double *cost_final);
/* The same with the multilateration's consensus vote (RangeConsensus, CORA_problem.h; cora_multilaterate_robust_dev,
 * include/cora_hip.h): consensus_barc2 <= 0 is off and has cora_problem_range_aided_initialization's bits; > 0: every range of a
 * landmark's list proposes the point its sample of d + 1 ranges determines, the fit runs over the ranges that agree with the
 * elected proposal, and a landmark whose elected proposal has fewer than min_consensus (<= 0: d + 2) votes has status 5 and keeps
 * its random draw (it is among "not solved").  consensus_counts = { landmarks without consensus, ranges excluded };  consensus,
 * list_len: one entry per landmark;  inlier: one byte per range measurement as added (1 inlier | 0 in a voted list, not an
 * inlier | 2 in no voted list).  With the vote off the three arrays are not written.  Every array but out may be NULL. */
int cora_problem_range_aided_initialization_consensus(cora_problem *p, uint64_t seed, int gn_steps, double consensus_barc2, int min_consensus,
                                                      double *out, int64_t counts[4], unsigned char *status, double *cost_linear,
                                                      double *cost_final, int64_t consensus_counts[2], int32_t *consensus, int32_t *list_len,
                                                      unsigned char *inlier);
/* Problem::multiRobotInitialization (an extension beyond the reference; include/cora_hip.h, "chain placement from
 * inter-robot ranges").  min_ranges <= 0: the default.  out: data-matrix-size x rank.  counts = { chains placed, not placed,
 * Gauss-Newton steps taken, stages }; status, cost_start, cost_linear, cost_final: one entry per chain of
 * cora_problem_odometry_chains; transforms: d * d + d per chain.  landmark_counts and landmark_status as counts and status of
 * cora_problem_range_aided_initialization.  Every array but out may be NULL. */
int cora_problem_multi_robot_initialization(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, double *out, int64_t counts[4],
                                            unsigned char *status, double *cost_start, double *cost_linear, double *cost_final,
                                            double *transforms, int64_t landmark_counts[4], unsigned char *landmark_status);
/* The same with the order of the stages (ChainOrder, CORA_problem.h): 0 greedy -- the call above --, 1 levels, a level's
 * chains placed together (include/cora_hip.h, cora_place_chains_batched_dev).  counts has a fifth entry, the levels. */
int cora_problem_multi_robot_initialization_order(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int order, double *out,
                                                  int64_t counts[5], unsigned char *status, double *cost_start, double *cost_linear,
                                                  double *cost_final, double *transforms, int64_t landmark_counts[4],
                                                  unsigned char *landmark_status);
/* The same with the chain placement's consensus vote (ChainRangeConsensus, CORA_problem.h; cora_place_chains_robust_dev,
 * include/cora_hip.h), under either order: consensus_barc2 <= 0 is off and has the call above's bits; > 0: every range of a
 * chain's stage list proposes the motion its sample of m = 8 / 17 ranges determines, the fit runs over the ranges that agree
 * with the elected proposal, and a chain whose elected proposal has fewer than min_consensus (<= 0: 2 m) votes has status 5 and
 * keeps its random start (it is among "not placed").  consensus_counts = { chains without consensus, ranges excluded };
 * consensus, list_len: one entry per chain;  inlier: one byte per range measurement as added (1 inlier | 0 in a stage list, not
 * an inlier | 2 in no stage list).  With the vote off the three arrays are not written.  Every array but out may be NULL. */
int cora_problem_multi_robot_initialization_consensus(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int order, double consensus_barc2,
                                                      int min_consensus, double *out, int64_t counts[5], unsigned char *status, double *cost_start,
                                                      double *cost_linear, double *cost_final, double *transforms, int64_t landmark_counts[4],
                                                      unsigned char *landmark_status, int64_t consensus_counts[2], int32_t *consensus,
                                                      int32_t *list_len, unsigned char *inlier);
/* Problem::sightingInitialization (an extension beyond the reference; include/cora_hip.h, "placement from pose-landmark
 * sightings").  min_ranges, min_sightings <= 0: the defaults.  out: data-matrix-size x rank.  counts = { chains fixed, placed,
 * not placed, landmarks placed, not placed, stages } of the sighting step; status, cost_start, cost_final, chosen: one entry
 * per chain of cora_problem_odometry_chains; transforms: d * d + d per chain; landmark_status, landmark_cost: one entry per
 * landmark.  chain_counts and chain_status: counts and status of cora_problem_multi_robot_initialization for the range
 * placement of the chains the sightings left (all fixed where it was skipped); landmark_counts and range_landmark_status: as
 * counts and status of cora_problem_range_aided_initialization, for the landmarks the sightings did not place.  Every array
 * but out may be NULL. */
int cora_problem_sighting_initialization(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int min_sightings, double *out,
                                         int64_t counts[6], unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen,
                                         double *transforms, unsigned char *landmark_status, double *landmark_cost, int64_t chain_counts[4],
                                         unsigned char *chain_status, int64_t landmark_counts[4], unsigned char *range_landmark_status);
/* The same with the sighting step's consensus vote (SightingConsensus, CORA_problem.h; cora_place_by_sightings_robust_dev,
 * include/cora_hip.h): consensus_barc2 <= 0 is off and has cora_problem_sighting_initialization's bits; > 0: every sighting of
 * a list proposes, the proposal most sightings agree with (tau |.|^2 <= consensus_barc2) is elected and the fit runs over the
 * agreeing sightings; a chain below min_chain_consensus (<= 0: d + 1) or a landmark below min_landmark_consensus (>= 1) has
 * status 5 and is left to the steps that follow.  consensus_counts = { chains without consensus, landmarks without consensus,
 * C-list entries outside their inliers, REFIT entries outside their inliers };  chain_consensus, chain_list_len: per chain;
 * landmark_consensus, landmark_list_len: per landmark;  inlier_chain, inlier_landmark: one byte per edge of the measurement
 * table (relative poses first, as added), 1 | 0 | 2 in no list -- all empty / 0 without a vote.  Every array but out may be NULL. */
int cora_problem_sighting_initialization_consensus(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int min_sightings,
                                                   double consensus_barc2, int min_chain_consensus, int min_landmark_consensus, double *out,
                                                   int64_t counts[6], unsigned char *status, double *cost_start, double *cost_final,
                                                   int32_t *chosen, double *transforms, unsigned char *landmark_status, double *landmark_cost,
                                                   int64_t consensus_counts[4], int32_t *chain_consensus, int32_t *chain_list_len,
                                                   int32_t *landmark_consensus, int32_t *landmark_list_len, unsigned char *inlier_chain,
                                                   unsigned char *inlier_landmark, int64_t chain_counts[4], unsigned char *chain_status,
                                                   int64_t landmark_counts[4], unsigned char *range_landmark_status);
/* Problem::closureInitialization (an extension beyond the reference; include/cora_hip.h, "placement from inter-chain
 * relative-pose edges").  min_ranges, min_sightings, min_closures <= 0: the defaults.  out: data-matrix-size x rank.
 * counts = { chains fixed, placed, not placed, refused, stages, closures used, skipped + unused edges } of the closure step;
 * status, cost_start, cost_final, chosen: one entry per chain of cora_problem_odometry_chains; transforms: d * d + d per
 * chain.  sighting_counts, sighting_status, landmark_status: counts, status and landmark_status of
 * cora_problem_sighting_initialization for the sighting step that followed (its fixed chains: closure status 0 or 4); the
 * last four as there.  Every array but out may be NULL. */
int cora_problem_closure_initialization(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int min_sightings, int min_closures,
                                        double *out, int64_t counts[7], unsigned char *status, double *cost_start, double *cost_final,
                                        int32_t *chosen, double *transforms, int64_t sighting_counts[6], unsigned char *sighting_status,
                                        unsigned char *landmark_status, int64_t chain_counts[4], unsigned char *chain_status,
                                        int64_t landmark_counts[4], unsigned char *range_landmark_status);
/* The same with the closure step's consensus vote (ClosureConsensus, CORA_problem.h; cora_place_by_closures_robust_dev,
 * include/cora_hip.h): consensus_barc2 <= 0 is off and has cora_problem_closure_initialization's bits; > 0: every closure of
 * a list proposes a motion, the fit runs over the closures that agree with the elected one, and a chain whose elected closure
 * has fewer than min_consensus (>= 1) votes has status 5 and is handed on like a refused one.  consensus_counts = { chains
 * without consensus, closures excluded };  consensus, list_len: one entry per chain;  inlier: one byte per edge of the
 * measurement table, the relative poses, pose priors, pose-landmark measurements and landmark priors in this order, each as
 * added (cora_problem_measurement_counts [0] + .. + [3] bytes: 1 inlier | 0 in a list, not an inlier | 2 in no list).  With the vote off the
 * three arrays are not written.  Every array but out may be NULL. */
int cora_problem_closure_initialization_consensus(cora_problem *p, uint64_t seed, int gn_steps, int min_ranges, int min_sightings, int min_closures,
                                                  double consensus_barc2, int min_consensus, double *out, int64_t counts[7],
                                                  unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen,
                                                  double *transforms, int64_t consensus_counts[2], int32_t *consensus, int32_t *list_len,
                                                  unsigned char *inlier, int64_t sighting_counts[6], unsigned char *sighting_status,
                                                  unsigned char *landmark_status, int64_t chain_counts[4], unsigned char *chain_status,
                                                  int64_t landmark_counts[4], unsigned char *range_landmark_status);
/* compute_Lambda_blocks(Y): stiefel d x dn (ld d), oblique r */
int cora_problem_lambda_blocks(cora_problem *p, const double *Y, double *stiefel, double *oblique);
/* Problem::measurementResiduals (an extension beyond the reference; formulas in include/cora_hip.h, "per-measurement
 * residuals").  counts: [0] relative poses, [1] pose priors, [2] pose-landmark measurements, [3] landmark priors,
 * [4] ranges.  Y: getExpectedVariableSize() x cols, 1 <= cols <= 24.  Each output has the length of its kind's count, in
 * the order the measurements were added, and may be NULL; sums = { rotation, translation, range } (may be NULL). */
int cora_problem_measurement_counts(const cora_problem *p, int64_t counts[5]);
int cora_problem_measurement_residuals(cora_problem *p, const double *Y, int cols, double *rel_pose_rot,
                                       double *rel_pose_trans, double *pose_prior_rot, double *pose_prior_trans,
                                       double *pose_landmark, double *landmark_prior, double *range, double sums[3]);

/* Problem::setMeasurementWeights / getMeasurementWeights (an extension beyond the reference; CORA/CORA_problem.h,
 * struct MeasurementWeights).  Seven arrays in the order of cora_problem_measurement_residuals' outputs: rel_pose_rot,
 * rel_pose_trans, pose_prior_rot, pose_prior_trans, pose_landmark, landmark_prior, range.  set: a NULL array or a length
 * of 0 means all ones, otherwise lengths[k] must be the count of the kind and every weight finite and >= 0
 * (CORA_HOST_ERR_ARG otherwise, nothing changed).  Q is assembled again; a device handle that exists is updated in place
 * (cora_update_values) and stays the same handle.  Afterwards cora_problem_measurement_residuals returns WEIGHTED
 * residuals.  get: every non-NULL array receives the count of its kind (ones where none were set). */
int cora_problem_set_measurement_weights(cora_problem *p, const double *const weights[7], const int64_t lengths[7]);
/* Problem::reweight: the same arguments and the same result to rounding, with Q(w) assembled on the device through the
 * handle's term map (cora_assembly_build / cora_assemble_values, cora_hip.h) when a live unpartitioned handle exists:
 * the data matrix then holds the device's bits.  Without such a handle it is cora_problem_set_measurement_weights. */
int cora_problem_reweight(cora_problem *p, const double *const weights[7], const int64_t lengths[7]);
int cora_problem_get_measurement_weights(const cora_problem *p, double *const weights[7]);
/* Problem::gncWeights (an extension beyond the reference; CORA/CORA_problem.h): one weight step of a robust-cost (GNC)
 * loop on the device at Y (N x cols).  thresholds / lengths: barc2 per measurement in the seven arrays of
 * cora_problem_set_measurement_weights (NULL or length 0: the kind is trusted, weight 1).  cost: 0 none, 1 truncated
 * least squares, 2 Geman-McClure (cora_hip.h, CORA_GNC_*).  The residuals are UNWEIGHTED whatever the current weights.
 * couple_edges != 0: a relative pose / pose prior is one measurement judged against its *_trans threshold.
 * weights_out: every non-NULL array receives the count of its kind -- valid arguments of cora_problem_reweight.
 * stats: 12 doubles [rot | trans | range] x { sum w r2, max rho, n_mid, n_out } (may be NULL).
 * Needs a live, unpartitioned device handle (CORA_HOST_ERR otherwise). */
int cora_problem_gnc_weights(cora_problem *p, const double *Y, int cols, const double *const thresholds[7],
                             const int64_t lengths[7], int cost, double mu, int couple_edges, double *const weights_out[7],
                             double stats[12]);
/* parsePyfgGroundTruth (an extension beyond the reference; CORA/pyfg_text_parser.h): the VERTEX_* values of a PyFG file as
 * a point of the problem, N x d column-major with N = data-matrix size (rotation rows R_i^T, unit range rows, positions). */
int cora_problem_ground_truth(const cora_problem *p, const char *path, double *X_out);
/* Problem::compareToReference (an extension beyond the reference; CORA/CORA_problem.h; definitions: cora_hip.h,
 * cora_compare_dev): errors of Y (variable size x cols) against Ref (data-matrix size x ref_cols <= cols) after the
 * orthogonal alignment on the selected poses' positions.  select: NULL (every pose and landmark but the origin pose of a
 * problem with priors) or n_poses + n_landmarks bytes.  proper != 0 needs cols == ref_cols.  pose_trans_err, pose_rot_err
 * (n_poses), landmark_err (n_landmarks), aligned_out (data-matrix size x ref_cols) may be NULL.  out: 8 + ref_cols + cols
 * + ref_cols + cols * ref_cols doubles in the order of cora_compare_dev. */
int cora_problem_compare(const cora_problem *p, const double *Y, int cols, const double *Ref, int ref_cols,
                         const unsigned char *select, int proper, double *pose_trans_err, double *pose_rot_err,
                         double *landmark_err, double *aligned_out, double *out);
/* Problem::posePairsByStep (Ref == NULL: the pairs (c[a], c[a + step]) of every robot's chain) or
 * Problem::posePairsByDistance (Ref: data-matrix size x ref_cols; for every start the first later pose of the same robot at
 * least L along Ref's positions).  pairs_out: 2 * n_poses int32 (a start appears at most once), path_out: n_poses doubles;
 * *m_out: the number of pairs. */
int cora_problem_pose_pairs(const cora_problem *p, int step, const double *Ref, int ref_cols, double L, int32_t *pairs_out,
                            double *path_out, int64_t *m_out);
/* Problem::relativeError: the relative pose errors of Y (variable size x cols) against Ref (data-matrix size x ref_cols,
 * independent of cols) over m pairs (include/cora_hip.h, cora_rpe_dev).  trans_err, rot_err: m doubles or NULL.  out: m,
 * sum et^2, max et, sum er^2, max er, first pair that attains max et, mean of et / path_length, mean of er / path_length. */
int cora_problem_relative_error(cora_problem *p, const double *Y, int cols, const double *Ref, int ref_cols, int64_t m,
                                const int32_t *pairs, const double *path_length, double *trans_err, double *rot_err,
                                double out[8]);
/* Problem::roundSolution (an extension beyond the reference): projectSolution on the device (include/cora_hip.h,
 * cora_round).  Y: variable size x cols, d <= cols <= 24; y_out: variable size x d.  info: NULL or 2 + cols doubles -- the
 * pose blocks of positive determinant, flipped (0 / 1), the singular values of Y (descending). */
int cora_problem_round_solution(const cora_problem *p, const double *Y, int cols, double *y_out, double *info);
/* solveRobustCORA (an extension beyond the reference; CORA/CORA.h): graduated non-convexity over solveCORA from x0
 * (N x rank).  thresholds / lengths / cost (1 or 2) / couple_edges as above; mu_factor > 1; max_outer: cap on the rounds.
 * x_out: N x d.  stats: as cora_problem_solve, of the last solve.  robust: [0] rounds, [1] 1 = converged (0: the cap),
 * [2] number of weight steps recorded in the histories.  mu_hist / sum_wr2_hist: NULL or max_outer + 1 doubles each.
 * The problem is left weighted with the final weights (cora_problem_get_measurement_weights). */
int cora_problem_solve_robust(cora_problem *p, const double *x0, int max_rank, int verbose,
                              const double *const thresholds[7], const int64_t lengths[7], int cost, int couple_edges,
                              double mu_factor, int max_outer, double *x_out, double stats[11], double robust[3],
                              double *mu_hist, double *sum_wr2_hist);

/* Riemannian TNT (the call of src/CORA.cpp:139-140 with the parameters of :95-109) from x0
 * (N x rank).  opts (may be NULL): [0] max_iterations, [1] max_TPCG_iterations, [2] gradient
 * tolerance, [3] preconditioned gradient tolerance, [4] max seconds, [5] verbose, [6] non-zero: drive
 * the inner STPCG from the host instead of cora_stpcg_dev (7 entries; 0 keeps a default).
 * stats out: [0] f, [1] |grad|, [2] |P grad|, [3] outer iterations, [4] Hessian-vector products,
 * [5] status (TNTStatus), [6] seconds. */
int cora_problem_tnt(cora_problem *p, const double *x0, const double *opts, double *x_out, double stats[7]);
/* ONE outer iteration of the same solver from x with trust-region radius Delta (test hook: the iteration is compared
 * with the CPU restatement step by step, so that rounding differences cannot accumulate over a chaotic trajectory).
 * out: [0] f at x_out, [1] the radius after the update, [2] inner (STPCG) iterations, [3] gain ratio rho,
 * [4] 1 if the step was accepted (x_out = the new point, else x), [5] |h|, [6] |h|_M, [7] status as in cora_problem_tnt. */
int cora_problem_tnt_step(cora_problem *p, const double *x, double Delta, int host_stpcg, double *x_out, double out[8]);

/* Problem::certify_solution(Y, eta, nx, bootstrap = Y) (src/CORA_problem.cpp:1030-1103).
 * out: [0] is_certified, [1] theta, [2] LOBPCG iterations; x: N (direction of negative curvature or 0). */
int cora_problem_certify(cora_problem *p, const double *Y, double eta, int nx, double out[3], double *x);

/* Two certifications in a row at Y, the second started from the first one's Ritz block -- handed over through the host
 * (resident = 0: Problem::certify_solution, all_eigvecs as the next bootstrap, the reference's flow src/CORA.cpp:158-170)
 * or left on the device (resident = 1: Problem::certify_solution_resident, what this host's solveCORA does).
 * out: [0..2] is_certified, theta, iterations of the first; [3..5] of the second; x: the second's direction. */
int cora_problem_certify_chain(cora_problem *p, const double *Y, double eta, int nx, int resident, double out[6], double *x);

/* Test switches of the eigensolver stage of certify_solution (src/CORA_utils.cpp:129-167): run step 3 without the seed
 * that the failed factorisation yields and / or without the incomplete-LDL^T preconditioner; and whether the last
 * cora_problem_certify got as far as step 3 (the preconditioned stage). */
int cora_problem_set_verification_lab(cora_problem *p, int seed_negative_direction, int use_ildl);
int cora_problem_certification_reached_step3(cora_problem *p, int *reached);

/* The PSD test of fast_verification alone (src/CORA_utils.cpp:36-51), on the host, no device needed: LL^T of S + shift I
 * (S: CSR, n x n, the certificate matrix of a problem with d, n_poses, n_ranges, n_trans) in the elimination order
 * certify_solution uses.  out: [0] 1 when the factorisation succeeded, [1] the permuted index of the first non-positive
 * pivot (-1), [2] nnz(L). */
int cora_host_cholesky_test(int d, int n_poses, int n_ranges, int n_trans, int n, const int32_t *rowptr, const int32_t *colidx,
                            const double *vals, double shift, int leaf_poses, int64_t out[3]);

/* fast_verification(S, eta, X0) (src/CORA_utils.cpp:17-186) for an arbitrary symmetric sparse S
 * (CSR, n x n).  X0: n x nx or NULL for a random block.  out: [0] is_certified, [1] theta,
 * [2] iterations; x: n. */
int cora_host_fast_verification(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                double eta, const double *X0, int nx, int max_iters, double out[3], double *x);
/* The same with the start block handed over as two pieces (columns [0, split) and [split, nx)) that are put side by side
 * on the device -- the form certify_solution uses (previous eigenvectors | cached random columns); same numbers. */
int cora_host_fast_verification_pieces(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                       double eta, const double *X0, int nx, int split, int max_iters, double out[3],
                                       double *x);

/* The same with the knobs of step 3 (src/CORA_utils.cpp:129-167) exposed for the tests: opts = {max_fill_factor,
 * drop_tol, seed the block with the failed factorisation's direction (0/1), use the ILDL preconditioner (0/1)};
 * out[3] = 1 when step 3 ran. */
int cora_host_fast_verification_lab(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                    double eta, const double *X0, int nx, int max_iters, const double opts[4],
                                    double out[4], double *x);

/* The certification call of solveCORA's loop (src/CORA.cpp:156-170): first != 0 -- the point itself is the eigensolver's
 * bootstrap (first level); first == 0 -- it starts from the Ritz block the previous call left on the device (what this host's
 * solveCORA does instead of handing all_eigvecs through the host).  out / x as cora_problem_certify. */
int cora_problem_certify_resident(cora_problem *p, const double *Y, double eta, int nx, int first, double out[3], double *x);

/* saddleEscape (src/CORA.cpp:245-350): Y is N x (rank - 1), the problem's relaxation rank has been incremented by the
 * caller (cora_problem_set_rank) as solveCORA does before the call; theta, v: the certificate's curvature and direction.
 * y_out: N x rank.  info: [0] f at [Y 0], [1] f at y_out, [2] 1 when y_out differs from [Y 0] (a trial point was taken). */
int cora_problem_saddle_escape(cora_problem *p, const double *Y, double theta, const double *v, double grad_tol,
                               double pgrad_tol, double *y_out, double info[3]);

/* projectSolution (src/CORA.cpp:352-441): Y is N x rank (the problem's current rank), y_out N x d. */
int cora_problem_project_solution(cora_problem *p, const double *Y, double *y_out);

/* solveCORA (src/CORA.cpp:26-243) from x0 (N x rank): Riemannian staircase up to max_rank, final
 * projection to rank d and refinement.  x_out: N x d.  opts[0..4] as in cora_problem_tnt (may be NULL).
 * stats: [0] f, [1] |grad|, [2] certified (the returned, rounded and refined solution), [3] eta, [4] theta, [5] final rank,
 * [6] staircase levels, [7] Hessian-vector products, [8] seconds, [9] 1 when the staircase stopped because its last level
 * was certified (0: it reached max_rank), [10] the rank of that level. */
int cora_problem_solve(cora_problem *p, const double *x0, int max_rank, int verbose, const double *opts,
                       double *x_out, double stats[11]);
/* The same with flags: CORA_SOLVE_DEVICE_ROUNDING rounds the certified point with Problem::roundSolution (on the device)
 * in place of projectSolution (CoraSolveInfo::device_rounding); 0 is cora_problem_solve. */
#define CORA_SOLVE_DEVICE_ROUNDING 1
int cora_problem_solve_flags(cora_problem *p, const double *x0, int max_rank, int verbose, const double *opts, int flags,
                             double *x_out, double stats[11]);

/* After a preconditioned call: [0] regularisation lambda used, [1] nnz(L), [2] elimination-tree height. */
int cora_problem_precond_info(cora_problem *p, double info[3]);

/* Host sparse Cholesky of (Q + shift I)[0:m,0:m] in the CORA nested-dissection order (the
 * CHOLMOD stand-in, cora_amd/csrc/host/sparse_cholesky.h); m = N or N-1.  Solves for the k
 * right-hand sides in B (m x k, ld m) in place.  info: [0] ok (0/1), [1] nnz(L), [2] height of
 * the elimination tree. */
int cora_problem_cholesky_solve(cora_problem *p, int m, double shift, int leaf_poses, double *B, int k,
                                int64_t info[3]);
/* Test hook for the host factorisation itself: info = {ok, nnz(L), first failing column (permuted) or -1}, digest = two
 * order-dependent sums over the finished columns of L (bit-equal runs give bit-equal digests), negative_direction
 * (N doubles, optional) = the direction of non-positive curvature when the factorisation fails.  The subtree-parallel
 * factorisation (CORA_CHOL_THREADS) must reproduce the one-thread result exactly. */
int cora_problem_cholesky_probe(cora_problem *p, int m, double shift, int leaf_poses, int64_t info[3], double *digest,
                                double *negative_direction);
/* The same on a copy of Q whose diagonal entries bump_rows[b] (original numbering) have bump_vals[b] added: puts the
 * first non-positive pivot where a test wants it (e.g. inside the group of trailing landmark rows). */
int cora_problem_cholesky_probe_bumped(cora_problem *p, int m, double shift, int leaf_poses, int nbump,
                                       const int32_t *bump_rows, const double *bump_vals, int64_t info[3],
                                       double *digest, double *negative_direction);

/* Test / timing hook without a GPU: factor of (Q + shift I)[0:N-1] and the device solve plan built from it (the host part
 * of the preconditioner's set-up; CORA_TRI_TIMING=1 prints its phases).  info = {stages, nnz(L), substitution blocks,
 * rows of the top stage}. */
int cora_problem_plan_probe(cora_problem *p, double shift, int leaf_poses, int64_t info[4]);

/* getBlockCholeskyFactorization + blockCholeskySolve (include/CORA/CORA_preconditioners.h:40-44) on the host:
 * A symmetric CSR n x n, block sizes summing to n, B rhs_rows x k column-major with rhs_rows = n or n + 1
 * (then the last row of X is zero). */
int cora_host_block_cholesky_solve(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int nblocks,
                                   const int32_t *block_sizes, int rhs_rows, int k, const double *B, double *X);

/* The reference's manifold classes (include/CORA/StiefelProduct.h, ObliqueManifold.h, MatrixManifold.h) on the
 * GPU.  kind 0: StiefelProduct(k, p, n), points p x kn; kind 1: ObliqueManifold(p, n), points p x n
 * (column-major).  op: "projectToManifold" (A), "projectToTangentSpace" (A = Y, B = V), "retract" (A = Y, B = V),
 * "random_sample" (seed), "innerProduct" (A, B -> out[0]), "SymBlockDiagProduct" (A; B holds B then C back to
 * back). */
int cora_host_manifold_op(int kind, int k, int p, int n, const char *op, const double *A, const double *B,
                          uint64_t seed, double *out);

/* Problem::printProblem (src/CORA_problem.cpp:400-489): registry and measurements on stdout. */
int cora_problem_print(cora_problem *p);

/* saveSolnToTum / saveSolnToG20 (src/CORA_utils.cpp:235-346) for a rank-d solution of the explicit problem
 * (N x d, e.g. the output of "alignEstimateToOrigin"): one line per pose of robot `robot_chr` (the symbol
 * character, as getPoseSymbols(chr); 0 = every pose in index order), time stamp = position in that list. */
int cora_problem_save_trajectory(cora_problem *p, const double *X, int g2o, int robot_chr, const char *path);

/* The device handle (cora_ctx*, include/cora_hip.h) behind the problem's operators. */
void *cora_problem_context(cora_problem *p);

#ifdef __cplusplus
}
#endif
#endif /* CORA_HOST_H_ */
