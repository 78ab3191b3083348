// CORA::Problem -- host-side mirror of the reference's class
// (include/CORA/CORA_problem.h:67-416).  Ingestion, the variable registry and
// the data-matrix assembly run on the host (they define Q once per problem);
// every operator of the optimisation hot path is a call through the C ABI of
// include/cora_hip.h into HIP kernels.  There is no CPU implementation of the
// operators in this class: without a usable gfx950 device they throw.
#pragma once

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <set>
#include <utility>
#include <vector>

#include "CORA_types.h"
#include "sparse_cholesky.h"
#include "Measurements.h"
#include "Symbol.h"

struct cora_ctx;
// the injected communication steps of a partitioned handle (include/cora_hip.h, cora_set_comm)
extern "C" {
typedef int (*cora_exchange_fn)(void *user, double *dX, int ld);
typedef int (*cora_allreduce_fn)(void *user, double *vals, int n);
typedef int (*cora_allgather_fn)(void *user, double *dX, int ld);
}

namespace CORA {

/** include/CORA/CORA_problem.h:31-46 */
struct CoraDataSubmatrices {
  SparseMatrix range_incidence_matrix;
  SparseMatrix range_precision_matrix;
  SparseMatrix range_dist_matrix;
  SparseMatrix rel_pose_incidence_matrix;
  SparseMatrix rel_pose_translation_data_matrix;
  SparseMatrix rotation_conn_laplacian;
  SparseMatrix rel_pose_translation_precision_matrix;
  SparseMatrix rel_pose_rotation_precision_matrix;
};

/** EXTENSION beyond the reference's Problem (which can report only f = 1/2 <X, Q X>): the residual of every measurement at
 * a point, per kind and in the order the measurements were added.  With X_a the d x k rotation block of pose a, x_t(s) the
 * translation row of symbol s and x_rho the unit row of a range (include/cora_hip.h, "per-measurement residuals"):
 *   rotation part     kappa |X_b - R^T X_a|_F^2                           (relative poses, pose priors with a = the origin)
 *   translation part  tau |x_t(b) - x_t(a) - sum_c t_c X_a[c, :]|^2       (every kind but ranges; priors with a = the origin)
 *   range             omega |x_t(b) - x_t(a) + r x_rho|^2
 * No 1/2 in the values:  1/2 (rot_sum + trans_sum + range_sum) = evaluateObjective(X) for any X. */
struct MeasurementResiduals {
  std::vector<Scalar> rel_pose_rot, rel_pose_trans;      // getRPMs() order
  std::vector<Scalar> pose_prior_rot, pose_prior_trans;
  std::vector<Scalar> pose_landmark, landmark_prior;     // translation part (these kinds have no rotation part)
  std::vector<Scalar> range;                             // getRangeMeasurements() order
  Scalar rot_sum = 0, trans_sum = 0, range_sum = 0;      // over all kinds
};

/** EXTENSION beyond the reference: a weight per measurement, multiplied into the precision the data matrix is assembled
 * with (kappa and tau of a relative pose or pose prior, tau of a pose-landmark measurement or landmark prior, omega of a
 * range).  The same seven vectors as MeasurementResiduals, in the same order -- a robust-cost loop reads residuals and
 * writes weights kind by kind.  An EMPTY vector means all ones; otherwise its length must be the number of measurements of
 * the kind and every weight finite and >= 0.  A zero weight switches a measurement off without changing the sparsity
 * pattern of Q (its entries stay, as zeros). */
struct MeasurementWeights {
  std::vector<Scalar> rel_pose_rot, rel_pose_trans;
  std::vector<Scalar> pose_prior_rot, pose_prior_trans;
  std::vector<Scalar> pose_landmark, landmark_prior;
  std::vector<Scalar> range;
};

/** EXTENSION beyond the reference: the weight step of a graduated non-convexity (GNC) loop, Problem::gncWeights below.
 * The robust costs (include/cora_hip.h, cora_gnc_weights_dev): with rho = r2 / barc2 the ratio of a measurement's
 * UNWEIGHTED residual to its threshold,
 *   TruncatedLeastSquares  w = 1 for rho <= mu / (mu + 1), 0 for rho >= (mu + 1) / mu, sqrt(mu (mu + 1) / rho) - mu between
 *   GemanMcClure           w = (mu / (rho + mu))^2
 *   None                   w = 1 (only the statistics are of interest: the largest rho starts the schedule of mu). */
enum class GncCost { None = 0, TruncatedLeastSquares = 1, GemanMcClure = 2 };
/** Statistics of a weight step per segment (rotation parts, translation parts, ranges).  With coupled edges a relative
 * pose or pose prior is counted and maximised in `trans` only; `rot` then carries only its sum. */
struct GncStats {
  struct Segment {
    Scalar sum_wr2 = 0;  // sum of w r2
    Scalar max_rho = 0;  // largest ratio (0 for an empty segment)
    long n_mid = 0;      // measurements with 0 < w < 1
    long n_out = 0;      // measurements with w < 0.5
  } rot, trans, range;
  Scalar maxRho() const { return std::max(rot.max_rho, std::max(trans.max_rho, range.max_rho)); }
  Scalar sumWr2() const { return rot.sum_wr2 + trans.sum_wr2 + range.sum_wr2; }
  long nMid() const { return rot.n_mid + trans.n_mid + range.n_mid; }
};

/** EXTENSION beyond the reference: how far an estimate is from a reference point (normally the ground truth of
 * parsePyfgGroundTruth) after an orthogonal alignment on the selected poses' positions, Problem::compareToReference below
 * (definitions: include/cora_hip.h, cora_compare_dev).  Errors of entries that were not selected are 0. */
struct TrajectoryComparison {
  long num_poses = 0, num_landmarks = 0;  // selected
  std::vector<Scalar> pose_trans_err;     // |(x_i - xbar) A - (g_i - gbar)| per pose, pose order
  std::vector<Scalar> pose_rot_err;       // |X_i A - G_i|_F per pose (chordal; angle = 2 asin(e / (2 sqrt 2)) for a d-column reference)
  std::vector<Scalar> landmark_err;       // per landmark
  Scalar sum_trans_err2 = 0, max_trans_err = 0, sum_rot_err2 = 0, max_rot_err = 0, sum_landmark_err2 = 0, max_landmark_err = 0;
  std::vector<Scalar> singular_values;    // of H, descending: a small last one says the alignment is not determined
  Matrix A;                               // k x kr, A^T A = I
  Vector xbar, gbar;                      // the selected poses' mean positions
  Matrix aligned;                         // the estimate in the reference's frame (N x kr), empty unless asked for
  Scalar transRmse() const { return num_poses > 0 ? std::sqrt(sum_trans_err2 / static_cast<Scalar>(num_poses)) : 0; }
  Scalar rotRmse() const { return num_poses > 0 ? std::sqrt(sum_rot_err2 / static_cast<Scalar>(num_poses)) : 0; }
  Scalar landmarkRmse() const { return num_landmarks > 0 ? std::sqrt(sum_landmark_err2 / static_cast<Scalar>(num_landmarks)) : 0; }
};

/** EXTENSION beyond the reference: pairs of poses (i, j) in pose order for the relative pose error, Problem::relativeError
 * below, with the length of the path between the two.  posePairsByStep: the number of steps; posePairsByDistance: the
 * length along the reference's positions. */
struct PosePairs {
  std::vector<int32_t> pairs;       // (i, j) of every pair, one after the other
  std::vector<Scalar> path_length;  // one per pair
  size_t size() const { return path_length.size(); }
};

/** EXTENSION beyond the reference: the error of the motion between the two poses of every pair, estimate against
 * reference (definitions: include/cora_hip.h, cora_rpe_dev).  It needs no alignment and no common column count. */
struct RelativeError {
  long num_pairs = 0;
  std::vector<Scalar> trans_err;    // |X_i (x_j - x_i)^T - G_i (g_j - g_i)^T| per pair
  std::vector<Scalar> rot_err;      // |X_i X_j^T - G_i G_j^T|_F per pair (chordal; angle = 2 asin(e / (2 sqrt 2)) on the manifold)
  std::vector<Scalar> path_length;  // of the pairs the errors were computed for
  Scalar sum_trans_err2 = 0, max_trans_err = 0, sum_rot_err2 = 0, max_rot_err = 0;
  long argmax_trans_err = 0;  // the first pair that attains max_trans_err
  Scalar transRmse() const { return num_pairs > 0 ? std::sqrt(sum_trans_err2 / static_cast<Scalar>(num_pairs)) : 0; }
  Scalar rotRmse() const { return num_pairs > 0 ? std::sqrt(sum_rot_err2 / static_cast<Scalar>(num_pairs)) : 0; }
  /** mean of error / path_length over the pairs with a positive length (0 without one) */
  Scalar meanTransDrift() const { return meanDrift(trans_err); }
  Scalar meanRotDrift() const { return meanDrift(rot_err); }

 private:
  Scalar meanDrift(const std::vector<Scalar> &err) const {
    Scalar sum = 0;
    long count = 0;
    for (size_t p = 0; p < err.size() && p < path_length.size(); ++p)
      if (path_length[p] > 0) {
        sum += err[p] / path_length[p];
        ++count;
      }
    return count > 0 ? sum / static_cast<Scalar>(count) : 0;
  }
};

/** EXTENSION beyond the reference: what Problem::roundSolution reports beside the rounded point (include/cora_hip.h,
 * cora_round_dev). */
struct RoundingInfo {
  std::vector<Scalar> singular_values;  // of the relaxed point, descending, one per column
  long positive_determinants = 0;       // pose blocks of Y Vd with a positive determinant
  bool flipped = false;                 // fewer than half: the last column was negated
};

/** What Problem::rangeAidedInitialization reports (cora_multilaterate_dev, include/cora_hip.h). */
struct LandmarkInitInfo {
  long solved = 0, not_solved = 0;     // landmarks placed from their ranges | left at their random draw
  long gn_steps = 0;                   // Gauss-Newton steps taken, summed over the landmarks
  long degenerate_range_rows = 0;      // range rows that got a fallback direction
  std::vector<unsigned char> status;   // per landmark (0 solved, 1 too few ranges, 2 degenerate geometry, 3 no range)
  std::vector<Scalar> cost_linear, cost_final;  // per landmark: sum omega (|x - t| - r)^2 after the linear stage, at the point written
  // with a consensus vote (RangeConsensus; status 5: no consensus, counted in not_solved); empty / 0 without one
  long no_consensus = 0, ranges_excluded = 0;  // status 5; ranges of the voted lists outside their inliers
  std::vector<int32_t> consensus, list_len;    // per landmark: the vote of the elected hypothesis, the ranges of the landmark's list
  std::vector<unsigned char> inlier;   // per range measurement: 1 inlier | 0 in a voted list, not an inlier | 2 in no voted list
};

/** The consensus vote of the multilateration (cora_multilaterate_robust_dev, include/cora_hip.h).  barc2 <= 0: off, the plain
 * least-squares fit and its bits.  barc2 > 0: every range of a landmark's list proposes the point its sample of d + 1 ranges
 * determines, the proposal most ranges agree with (weighted squared range residual <= barc2, the quantity the GNC weights
 * threshold) is elected and the fit runs over the agreeing ranges only; a landmark whose elected proposal has fewer than
 * min_consensus votes (<= 0: d + 2 -- a proposal has about d + 1 votes of its own) keeps its random draw (status 5).  One
 * proposal per range, clean only where all d + 1 ranges of its sample are: short lists with many outliers reach no consensus. */
struct RangeConsensus {
  Scalar barc2 = 0;
  int min_consensus = 0;
};

/** The order of the stages of Problem::multiRobotInitialization (cora_set_chain_placement_order, include/cora_hip.h): Greedy,
 * one chain after the other; Levels, every chain that can be placed independently in one level, a level's chains placed
 * together (cora_place_chains_batched_dev) -- from fewer ranges where chains of one level range against each other. */
enum class ChainOrder { Greedy = 0, Levels = 1 };

/** What Problem::multiRobotInitialization reports about the chains (cora_place_chains_dev, include/cora_hip.h). */
struct ChainPlacementInfo {
  long placed = 0, not_placed = 0;     // chains moved onto the fixed ones | left at their random start
  long gn_steps = 0;                   // Gauss-Newton steps taken, summed over the stages
  long stages = 0;
  long levels = 0;                     // ChainOrder::Levels: the levels the stages stand in; Greedy: = stages
  std::vector<unsigned char> status;   // per chain (0 placed, 1 too few ranges, 2 placed without the linear stage, 3 no range, 4 fixed)
  std::vector<Scalar> cost_start, cost_linear, cost_final;  // per chain: sum omega (|R q + t - a| - r)^2 over the stage's entries
  std::vector<Scalar> transforms;      // per chain d * d + d: R row-major, then t, as written
  // with a consensus vote (ChainRangeConsensus; status 5: no consensus, counted in not_placed); empty / 0 without one
  long no_consensus = 0, ranges_excluded = 0;  // status 5; ranges of the stage lists outside their inliers
  std::vector<int32_t> consensus, list_len;    // per chain: the vote of the elected hypothesis, the ranges of the chain's stage list
  std::vector<unsigned char> inlier;   // per range measurement: 1 inlier | 0 in a stage list, not an inlier | 2 in no stage list
};

/** The consensus vote of the chain placement from ranges (cora_place_chains_robust_dev, include/cora_hip.h).  barc2 <= 0: off,
 * the plain fit and its bits.  barc2 > 0: every range of a chain's stage list proposes the motion its sample of m ranges
 * determines (m = 8 at d = 2, 17 at d = 3: the linear stage, then 3 Gauss-Newton steps on the sample), the proposal most ranges
 * agree with (weighted squared range residual <= barc2, the quantity the GNC weights threshold) is elected and the fit runs over
 * the agreeing ranges only; a chain whose elected proposal has fewer than min_consensus votes (<= 0: 2 m -- a proposal has about m
 * votes of its own) keeps its random start (status 5).  One proposal per range, clean only where all m ranges of its sample
 * are: short lists with many outliers reach no consensus. */
struct ChainRangeConsensus {
  Scalar barc2 = 0;
  int min_consensus = 0;
};

/** What Problem::sightingInitialization reports about the sighting step (cora_place_by_sightings_dev, include/cora_hip.h). */
struct SightingPlacementInfo {
  long chains_fixed = 0, chains_placed = 0, chains_not_placed = 0;  // status 4 | 0 | 1, 2, 3
  long landmarks_placed = 0, landmarks_not_placed = 0;              // status 0 | 1, 2
  long stages = 0;
  std::vector<unsigned char> status;   // per chain (0 placed, 1 never taken, 2 refused by the device, 3 no sighting, 4 fixed)
  std::vector<Scalar> cost_start, cost_final;  // per chain: sum tau |x_t(l) - p|^2 over its list, before and as applied
  std::vector<int32_t> chosen;         // per chain: 1 moved, 0 left where it stood, -1 no list
  std::vector<Scalar> transforms;      // per chain d * d + d: R row-major, then t, as applied
  std::vector<unsigned char> landmark_status;  // per landmark (0 placed, 1 no sighting from a placed chain, 2 sum tau <= 0, 3 fixed)
  std::vector<Scalar> landmark_cost;   // per landmark: the sighting cost of its REFIT list at the row written
  // with a consensus vote (SightingConsensus; status 5: no consensus, chain or landmark); empty / 0 without one
  long chains_no_consensus = 0, landmarks_no_consensus = 0;  // status 5 (the landmarks: in the REFIT)
  long chain_entries_excluded = 0, landmark_entries_excluded = 0;  // entries of the C-stage lists / the REFIT lists outside their inliers
  std::vector<int32_t> chain_consensus, chain_list_len;        // per chain: the vote of the elected hypothesis, the sightings of its list
  std::vector<int32_t> landmark_consensus, landmark_list_len;  // per landmark, the REFIT's
  std::vector<unsigned char> inlier_chain, inlier_landmark;    // per edge of the measurement table: 1 inlier | 0 in a list, not an inlier | 2 in no list
};

/** The consensus vote of the sighting step (cora_place_by_sightings_robust_dev, include/cora_hip.h).  barc2 <= 0: off, the plain
 * step and its bits.  barc2 > 0: the threshold on tau |.|^2 of a sighting (the quantity the GNC weights threshold).  Every
 * sighting of a landmark's list proposes the landmark at its own prediction, every sighting of a chain's list the alignment of
 * a sample of d sightings; the proposal most sightings agree with is elected and the fit runs over the agreeing sightings only.
 * A chain whose elected proposal has fewer than min_chain_consensus votes (<= 0: d + 1) keeps its rows (status 5) and is left to
 * the range placement like a refused one; a landmark below min_landmark_consensus keeps its row (status 5) and is left to the
 * multilateration.  One proposal per sighting, clean only where all d sightings of its sample are. */
struct SightingConsensus {
  Scalar barc2 = 0;
  int min_chain_consensus = 0;
  int min_landmark_consensus = 1;
};

/** What Problem::closureInitialization reports about the closure step (cora_place_by_closures_dev, include/cora_hip.h). */
struct ClosurePlacementInfo {
  long chains_fixed = 0, chains_placed = 0, chains_not_placed = 0, chains_refused = 0;  // status 4 | 0 | 1, 2, 3 | 2
  long stages = 0, closures_used = 0, edges_skipped = 0;  // entries of all lists; skipped + unused edges
  std::vector<unsigned char> status;   // per chain (0 placed, 1 never taken, 2 refused by the device, 3 no inter-chain closure, 4 fixed)
  std::vector<Scalar> cost_start, cost_final;  // per chain: the closure cost of its list, before and as applied
  std::vector<int32_t> chosen;         // per chain: 1 moved, 0 left where it stood, -1 no list
  std::vector<Scalar> transforms;      // per chain d * d + d: G row-major, then s, as applied
  // with a consensus vote (ClosureConsensus; status 5: taken, no consensus); empty / 0 without one
  long chains_no_consensus = 0, closures_excluded = 0;  // status 5; entries outside the inliers of their lists
  std::vector<int32_t> consensus, list_len;  // per chain: the vote of the elected closure, the closures of the chain's list
  std::vector<unsigned char> inlier;   // per edge of the measurement table: 1 inlier | 0 in a list, not an inlier | 2 in no list
};

/** The consensus vote of the closure step (cora_place_by_closures_robust_dev, include/cora_hip.h).  barc2 <= 0: off, the
 * plain least-squares placement and its bits.  barc2 > 0: every closure of a list proposes a motion, the one most closures
 * agree with (coupled rot + trans residual <= barc2, the quantity the GNC weights threshold) is elected and the fit runs over
 * the agreeing closures only; a chain whose elected closure has fewer than min_consensus votes keeps its rows (status 5) and
 * is handed to the later steps like a refused one. */
struct ClosureConsensus {
  Scalar barc2 = 0;
  int min_consensus = 2;
};

class Problem {
 private:
  int dim_;
  bool pin_last_translation_ = true;
  int relaxation_rank_;

  std::map<Symbol, int> pose_symbol_idxs_;
  std::map<Symbol, int> landmark_symbol_idxs_;
  std::vector<RangeMeasurement> range_measurements_;
  std::vector<RelativePoseMeasurement> rel_pose_pose_measurements_;
  std::vector<RelativePoseLandmarkMeasurement> rel_pose_landmark_measurements_;
  Symbol origin_symbol_;
  std::vector<PosePrior> pose_priors_;
  std::vector<LandmarkPrior> landmark_priors_;
  // The reference finds duplicates with std::find over the measurement vectors
  // (src/CORA_problem.cpp:42,56,69: O(m^2)); same semantics with a hash of the
  // unordered symbol pair in an ordered set, so that 10^5-edge graphs load in seconds.
  std::set<std::pair<Key, Key>> range_pairs_, rpm_pairs_, rplm_pairs_;
  std::set<Key> pose_prior_ids_, landmark_prior_ids_;

  Formulation formulation_;
  Preconditioner preconditioner_;
  CoraDataSubmatrices data_submatrices_;
  bool has_priors_ = false;
  bool problem_data_up_to_date_ = false;
  int device_ = 0;
  int part_rank_ = 0, part_world_ = 1;
  cora_exchange_fn comm_exchange_ = nullptr;
  cora_allreduce_fn comm_allreduce_ = nullptr;
  cora_allgather_fn comm_allgather_ = nullptr;
  void *comm_user_ = nullptr;
  mutable std::shared_ptr<cora_ctx> ctx_;
  void validateWeights(const MeasurementWeights &w) const;  // lengths and values, std::invalid_argument
  bool ensureTermMap(const char *who);  // unit-weight table + term map on the live handle; true when it installed them
  // the Ritz block of the last certify_solution_resident, on the device (declared after ctx_: released before the handle)
  mutable std::shared_ptr<class LOBPCGSolver> cert_block_;
  CertResults certifyImpl(const Matrix &Y, Scalar eta, size_t nx, const Matrix &eigvec_bootstrap, size_t max_LOBPCG_iters,
                          bool resident) const;
  mutable bool precond_ready_ = false;
  mutable bool implicit_ready_ = false;  // chol(Q33[0:nt-1]) installed on the handle
  mutable bool measurements_ready_ = false;  // measurement table installed on the handle (measurementResiduals)
  mutable Scalar precond_lambda_ = 0;   // regularisation actually used
  mutable long precond_nnz_ = 0;         // nnz(L)
  mutable int precond_levels_ = 0;       // height of the elimination tree
  // symbolic analyses of this problem's factorisations (preconditioner block, certificate matrix): kept with the
  // Problem and gone with it (shared between copies of one Problem: they factorise the same patterns)
  // The measurement weights (setMeasurementWeights) live in the same heap block, behind this pointer, and not in a member
  // of their own: the size of a Problem and the offsets of its members are part of the library's ABI -- a program built
  // against the header of one version runs with the library of the next -- so they are shared between copies too.
  mutable std::shared_ptr<SymbolicCache> symbolic_cache_ = newSharedState();
  static std::shared_ptr<SymbolicCache> newSharedState();
  MeasurementWeights &weights() const;
  // cert_* below is written by prepareCertification(), which solveCORA runs on a thread of its own beside the first TNT
  // solve, and read by certify_solution / get_certificate_matrix: every one of them holds this lock for its whole body
  // (round-4 advice; shared between copies like the cache above so that Problem stays copyable)
  mutable std::shared_ptr<std::recursive_mutex> cert_mutex_ = std::make_shared<std::recursive_mutex>();
  mutable std::vector<int32_t> cert_perm_;  // elimination order of the full certificate matrix (pattern-only: kept per data matrix)
  // S = Q - Lambda(Y) kept between certifications: its pattern is Q's plus the Lambda blocks, only the entries under
  // Lambda change with Y.  cert_lambda_pos_: position in cert_S_.values of every Lambda entry (pose-block entries row
  // by row, then the range diagonal); cert_lambda_q_: the position of the same entry in Q's values, -1 when Q has none
  mutable SparseMatrix cert_S_;
  mutable std::vector<int32_t> cert_lambda_pos_, cert_lambda_q_;
  mutable Matrix cert_random_;  // the random start columns of the eigensolver (fixed seed: the same numbers every time)
  // test switches of certify_solution's eigensolver stage (FastVerificationLab, CORA_utils.h) and what the last call did
  bool cert_lab_on_ = false, cert_lab_seed_ = true, cert_lab_ildl_ = true;
  mutable bool cert_reached_step3_ = false;
  const SparseMatrix &certificateMatrixCached(const Matrix &Y) const;
  const SparseMatrix &certificateMatrixFrom(const std::pair<Matrix, Vector> &lambda_blocks) const;

  void checkUpToDate() const;
  void addOriginPose();
  void fillRangeSubmatrices();
  void fillRelPoseSubmatrices();
  void fillRotConnLaplacian();
  void fillDataMatrix();
  void updatePreconditioner();
  Matrix dataMatrixProduct(const Matrix &Y) const;
  void ensureContext() const;
  void ensurePreconditioner() const;
  void ensureMeasurementTable() const;
  // gn_steps < 0: no multilateration; place: the chains are first placed from the ranges between them (min_ranges <= 0: the default)
  // closures: first of all, the chains are placed from the relative-pose edges between chains (min_closures <= 0: 1)
  // sightings: before that, landmarks and chains are placed from the pose-landmark sightings (min_sightings <= 0: the default)
  Matrix odometryStart(uint64_t seed, int gn_steps, LandmarkInitInfo *info, const char *where, bool place = false, int min_ranges = 0,
                       ChainPlacementInfo *chains_info = nullptr, bool sightings = false, int min_sightings = 0,
                       SightingPlacementInfo *sight_info = nullptr, bool closures = false, int min_closures = 0,
                       ClosurePlacementInfo *closure_info = nullptr, ClosureConsensus consensus = ClosureConsensus(),
                       RangeConsensus range_consensus = RangeConsensus(),
                       SightingConsensus sighting_consensus = SightingConsensus(), ChainOrder chain_order = ChainOrder::Greedy,
                       ChainRangeConsensus chain_consensus = ChainRangeConsensus()) const;
  void fillImplicitFormulationMatrices() const;
  [[noreturn]] void throwLast(int status, const char *where) const;

 public:
  Problem(int dim, int relaxation_rank, Formulation formulation = Formulation::Explicit,
          Preconditioner preconditioner = Preconditioner::RegularizedCholesky);

  void addPoseVariable(const Symbol &pose_id);
  void addPoseVariable(const std::string &pose_id) { addPoseVariable(Symbol(pose_id)); }
  void addLandmarkVariable(const Symbol &landmark_id);
  void addLandmarkVariable(const std::string &landmark_id) { addLandmarkVariable(Symbol(landmark_id)); }
  void addRangeMeasurement(const RangeMeasurement &range_measurement);
  void addRelativePoseMeasurement(const RelativePoseMeasurement &rel_pose_measure);
  void addRelativePoseLandmarkMeasurement(const RelativePoseLandmarkMeasurement &m);
  void addPosePrior(const PosePrior &pose_prior);
  void addLandmarkPrior(const LandmarkPrior &landmark_prior);

  Index getRotationIdx(const Symbol &pose_symbol) const;
  Index getRangeIdx(const SymbolPair &range_symbol_pair) const;
  Index getTranslationIdx(const Symbol &trans_symbol) const;

  const CoraDataSubmatrices &getDataSubmatrices() {
    if (!problem_data_up_to_date_) updateProblemData();
    return data_submatrices_;
  }
  Symbol getOriginSymbol() const { return origin_symbol_; }
  std::map<Symbol, int> getPoseSymbolMap() const { return pose_symbol_idxs_; }
  /** Poses of one robot (symbols with character chr) in symbol order, src/CORA_problem.cpp:954-962. */
  std::vector<Symbol> getPoseSymbols(unsigned char chr) const {
    std::vector<Symbol> s;
    for (const auto &kv : pose_symbol_idxs_)
      if (kv.first.chr() == chr) s.push_back(kv.first);
    return s;
  }
  std::map<Symbol, int> getLandmarkSymbolMap() const { return landmark_symbol_idxs_; }
  const std::vector<RangeMeasurement> &getRangeMeasurements() const { return range_measurements_; }
  const std::vector<RelativePoseMeasurement> &getRPMs() const { return rel_pose_pose_measurements_; }
  // (extensions: the other measurement kinds, for callers that label measurementResiduals' values)
  const std::vector<RelativePoseLandmarkMeasurement> &getRPLMs() const { return rel_pose_landmark_measurements_; }
  const std::vector<PosePrior> &getPosePriors() const { return pose_priors_; }
  const std::vector<LandmarkPrior> &getLandmarkPriors() const { return landmark_priors_; }

  SparseMatrix data_matrix_;

  void updateProblemData();
  const SparseMatrix &getDataMatrix();
  int getDataMatrixSize() const;
  int getExpectedVariableSize() const;

  Formulation getFormulation() const { return formulation_; }
  Preconditioner getPreconditioner() const { return preconditioner_; }
  int dim() const { return dim_; }
  int numPoses() const { return static_cast<int>(pose_symbol_idxs_.size()); }
  int numPosePoseMeasurements() const { return static_cast<int>(rel_pose_pose_measurements_.size()); }
  int numPoseLandmarkMeasurements() const { return static_cast<int>(rel_pose_landmark_measurements_.size()); }
  int numPosePriors() const { return static_cast<int>(pose_priors_.size()); }
  int numLandmarkPriors() const { return static_cast<int>(landmark_priors_.size()); }
  int getNumPosePriors() const { return numPosePriors(); }          // include/CORA/CORA_problem.h:231-232
  int getNumLandmarkPriors() const { return numLandmarkPriors(); }
  /** Human-readable dump of the registry and of every measurement (src/CORA_problem.cpp:400-489). */
  void printProblem() const;
  int numLandmarks() const { return static_cast<int>(landmark_symbol_idxs_.size()); }
  int numRangeMeasurements() const { return static_cast<int>(range_measurements_.size()); }
  int numTranslationalStates() const { return numPoses() + numLandmarks(); }
  int numPosesDim() const { return dim() * numPoses(); }
  int rotAndRangeMatrixSize() const { return numPosesDim() + numRangeMeasurements(); }

  /*****  Riemannian optimization functions (all on the GPU)  *******/
  size_t getRelaxationRank() const { return static_cast<size_t>(relaxation_rank_); }
  Matrix getRandomInitialGuess(uint64_t seed = 7) const;
  void incrementRank() { setRank(relaxation_rank_ + 1); }
  void setRank(int r);
  void setPreconditioner(Preconditioner p) {
    preconditioner_ = p;
    precond_ready_ = false;
  }
  void setFormulation(Formulation f) { formulation_ = f; }
  void setDevice(int device) { device_ = device; }
  // Multi-GPU (one process per GPU): this process owns partition `rank` of `world` of the rows of Q (pose-aligned,
  // nnz-balanced, include/cora_hip.h cora_ctx_create_part) and reaches the others through the library's own
  // communication (cora_comm_create_rccl / cora_comm_create_local on context(), after this call and after every
  // rebuild of the handle -- until then a collective step fails with CORA_ERR_NOT_READY) or through three injected
  // steps (cora_set_comm semantics; pass nullptr to install communication on the handle afterwards).  Every operator of
  // this class, TNT, LOBPCG, certify_solution and solveCORA then run on the partition, all ranks calling the same
  // sequence: the Lambda blocks of the certificate are gathered, every rank runs the PSD test (same decision), LOBPCG
  // runs on the sharded operator.  The Cholesky preconditioners become block Jacobi over the ranks with exact
  // blocks (every rank factorises the diagonal block of ITS rows of Q + lambda I: weaker than the reference's global
  // factor, more inner iterations).  Not sharded: the implicit formulation (use explicit) and the ILDL branch of
  // fast_verification (skipped).  Call before the first operator.
  SymbolicCache *symbolicCache() const { return symbolic_cache_.get(); }
  void setPartition(int rank, int world, cora_exchange_fn exchange, cora_allreduce_fn allreduce,
                    cora_allgather_fn allgather, void *user) {
    part_rank_ = rank;
    part_world_ = world;
    comm_exchange_ = exchange;
    comm_allreduce_ = allreduce;
    comm_allgather_ = allgather;
    comm_user_ = user;
    cert_block_.reset();
    ctx_.reset();
    measurements_ready_ = false;
    precond_ready_ = false;
  }
  int partitionWorld() const { return part_world_; }

  Scalar evaluateObjective(const Matrix &Y) const;
  Matrix Euclidean_gradient(const Matrix &Y) const;
  Matrix Riemannian_gradient(const Matrix &Y) const;
  Matrix Riemannian_gradient(const Matrix &Y, const Matrix &NablaF_Y) const;
  Matrix Riemannian_Hessian_vector_product(const Matrix &Y, const Matrix &NablaF_Y, const Matrix &Ydot) const;
  Matrix tangent_space_projection(const Matrix &Y, const Matrix &Ydot) const;
  Matrix precondition(const Matrix &V) const;
  Matrix projectToManifold(const Matrix &A) const;
  Matrix retract(const Matrix &Y, const Matrix &V) const;

  /** EXTENSION beyond the reference: per-measurement residuals at Y (struct MeasurementResiduals above), evaluated on the
   * device from a measurement table that is built from the measurement vectors on the first call and kept on the handle.
   * Y: getExpectedVariableSize() rows and any 1..24 columns (the relaxed and the rounded solution are both served); in the
   * implicit formulation it is completed with getTranslationExplicitSolution(Y) first.  Single-GPU handles only. */
  MeasurementResiduals measurementResiduals(const Matrix &Y) const;

  /** EXTENSION beyond the reference: re-weights the measurements (struct MeasurementWeights above) and assembles Q(w)
   * again on the host.  The stored measurements are not touched; the weights stay until they are set again (also across
   * updateProblemData()).  Unit weights give the data matrix of an unweighted problem bit for bit.
   *
   * A device handle that already exists is UPDATED IN PLACE (cora_update_values, include/cora_hip.h): the pattern of Q(w)
   * is the pattern of Q, so the format, the partition, the resident vectors and an installed communicator stay and only
   * the values move -- context() returns the same handle as before.  What depended on the values is redone on next use:
   * the preconditioner, the factor of the implicit formulation, the value caches of certification (their orderings and
   * symbolic analyses are kept).  Only if the pattern did change is the handle dropped and rebuilt, as
   * updateProblemData() does.
   * The measurement table follows the weights: measurementResiduals() then returns WEIGHTED residuals (w kappa, w tau,
   * w omega in the formulas above), so that 1/2 of their sum stays evaluateObjective().
   * Copies of one Problem share their weights (as they share the symbolic analyses): set them on one, and the others
   * assemble with them at their next updateProblemData().
   * Throws std::invalid_argument for a wrong length, a negative or a non-finite weight (nothing is changed then). */
  void setMeasurementWeights(const MeasurementWeights &w);
  const MeasurementWeights &getMeasurementWeights() const;
  /** EXTENSION beyond the reference: the same re-weighting with Q(w) ASSEMBLED ON THE DEVICE.  Same validation, same
   * stored weights and the same things redone on next use as setMeasurementWeights.  With a live, up-to-date,
   * unpartitioned handle the first call installs the measurement table with unit weights and builds the handle's term
   * map (cora_assembly_build, include/cora_hip.h); every call then flattens the seven kinds into table order (pose-pose,
   * pose priors, pose-landmark, landmark priors, then ranges) and runs cora_assemble_values: no host sparse algebra, and
   * getDataMatrix() holds the values the device computed, bit for bit.  Without such a handle it IS
   * setMeasurementWeights.
   * The two methods sum the same terms in different orders: their matrices agree to rounding (a few ulp of the sum of
   * the terms' magnitudes per entry), not to the bit.  reweight is reproducible in itself: the same weights give the same
   * bits on every call, on the device and in the host mirror of a plan-only handle. */
  void reweight(const MeasurementWeights &w);
  /** EXTENSION beyond the reference: one GNC weight step on the device (cora_gnc_weights, include/cora_hip.h) at Y
   * (getExpectedVariableSize() rows, 1..24 columns; completed first in the implicit formulation).  `thresholds` holds
   * barc2 per measurement in the seven vectors of MeasurementWeights: an EMPTY vector means trusted (+inf: weight 1),
   * otherwise its length must be the count of the kind and every value > 0 or +inf (std::invalid_argument /
   * std::runtime_error otherwise).  The residuals are UNWEIGHTED: they are formed with the measurements' own precisions
   * whatever the current weights are.  couple_edges: a relative pose or pose prior is one measurement (rot + trans
   * against its *_trans threshold, one weight for both parts; the *_rot thresholds are ignored).
   * Returns the weights, ready for reweight(), and the statistics.  The handle's state is untouched, except on the first
   * use per handle, which installs the unit-weight measurement table and the term map exactly as reweight does (and,
   * where weights had been set by setMeasurementWeights, re-assembles Q with them so that the table follows them).
   * Needs a live handle (one solve or operator call after updateProblemData): std::runtime_error without one, and with a
   * partitioned one, which has no measurement table. */
  std::pair<MeasurementWeights, GncStats> gncWeights(const Matrix &Y, const MeasurementWeights &thresholds, GncCost cost,
                                                     Scalar mu, bool couple_edges);

  /** EXTENSION beyond the reference: the errors of Y against Ref on the device (cora_compare, include/cora_hip.h).
   * Y: getExpectedVariableSize() rows, k = 1..24 columns (completed first in the implicit formulation); Ref:
   * getDataMatrixSize() rows, kr <= k columns.  select: one flag per translational state (poses, then landmarks); EMPTY
   * means every pose and landmark except the origin pose of a problem with priors.  proper (needs k == kr): det A = +1.
   * Changes nothing of the Problem or its handle.  Single-GPU handles only. */
  TrajectoryComparison compareToReference(const Matrix &Y, const Matrix &Ref, const std::vector<unsigned char> &select = {},
                                          bool proper = true, bool want_aligned = false) const;

  /** EXTENSION beyond the reference: the pairs (c[a], c[a + step]) of every robot's chain c (getPoseSymbols(chr), the
   * robots in the order of their characters), step >= 1; path_length = step.  A step of the chain's length or more gives
   * no pair of that robot. */
  PosePairs posePairsByStep(int step) const;
  /** For every start pose the first later pose of the same robot whose path length along Ref's positions -- the
   * cumulative sum of |g_{a+1} - g_a| over the chain, formed here on the host -- is at least L (> 0); starts that never
   * reach L are left out.  Ref: getDataMatrixSize() rows, any number of columns. */
  PosePairs posePairsByDistance(const Matrix &Ref, Scalar L) const;
  /** The relative pose errors of Y against Ref over the pairs, on the device (cora_rpe, include/cora_hip.h).  Y:
   * getExpectedVariableSize() rows, k = 1..24 columns (completed first in the implicit formulation); Ref:
   * getDataMatrixSize() rows, kr = 1..24 columns, independent of k.  The pair table is installed on the handle only when the
   * pairs differ from the ones the handle holds (cora_pose_pairs_equal; Problem keeps no copy and gains no member); nothing
   * else of the handle changes.  No pairs: zeros.  std::runtime_error on a
   * partitioned handle and without a live device handle (run a solve or an operator after updateProblemData first). */
  RelativeError relativeError(const Matrix &Y, const Matrix &Ref, const PosePairs &pairs);

  /** EXTENSION beyond the reference: projectSolution on the device (cora_round, include/cora_hip.h) -- the d dominant
   * singular directions of Y from its Gram matrix, the majority rule on the determinants, every pose block projected to
   * SO(d) by a one-sided Jacobi on the block itself, range rows normalised.  Y: getExpectedVariableSize() rows, d..24
   * columns (lifted to [Y; 0] and lowered again in the implicit formulation); returns the same rows, d columns, and ends
   * with checkVariablesAreValid.  Changes nothing of the handle; Problem gains no member.  std::runtime_error on a
   * partitioned handle. */
  Matrix roundSolution(const Matrix &Y, RoundingInfo *info = nullptr) const;

  /** EXTENSION beyond the reference: the odometry chains getOdomInitialization composes, as indices into getRPMs() (the
   * first block of the handle's measurement table): per robot character the measurements (c, k) -> (c, k + 1) in index
   * order, the last duplicate wins, a gap starts a new chain.  Chains in the host function's order. */
  std::vector<std::vector<int32_t>> odometryChains() const;
  /** EXTENSION beyond the reference: getOdomInitialization on the device (cora_odometry_init_dev, include/cora_hip.h): the
   * chains composed by a segmented scan of SE(d) over the handle's measurement table, the lift to the relaxation rank by
   * cora_combine_dev.  Draws from std::mt19937_64(seed) in the host function's order -- one start per chain after the
   * first, the landmarks in map order, the fallback directions of the degenerate range rows in range order, the p x p
   * rotation -- so that the same seed gives the host function's start up to rounding.  getDataMatrixSize() rows,
   * getRelaxationRank() columns.  Installs the measurement table and the chain tables on the handle where they are
   * missing; Problem gains no member.  std::runtime_error on a partitioned handle. */
  Matrix odometryInitialization(uint64_t seed = 7) const;
  /** EXTENSION beyond the reference: odometryInitialization with the landmarks placed from the ranges
   * (cora_multilaterate_dev): exactly the draws of odometryInitialization in the same order -- the random landmarks stay
   * as the fallback of the landmarks that are not solved --, then the multilateration over the poses a chain wrote
   * (pose_ok) with gn_steps Gauss-Newton steps, the range rows recomputed; a range row that is degenerate only now draws
   * its direction after everything else, in range order.  Pose rows and the rows of unsolved landmarks have
   * odometryInitialization's bits.  consensus: the outlier-robust multilateration (RangeConsensus; the default is off: the
   * same bits as without the argument); std::invalid_argument for a barc2 that is not finite.  std::runtime_error on a
   * partitioned handle. */
  Matrix rangeAidedInitialization(uint64_t seed = 7, int gn_steps = 5, LandmarkInitInfo *info = nullptr,
                                  RangeConsensus consensus = RangeConsensus()) const;
  /** EXTENSION beyond the reference: rangeAidedInitialization with every odometry chain after the first first moved rigidly
   * onto the chains placed before it, from the pose-pose ranges between chains (cora_place_chains_dev): exactly the draws
   * of odometryInitialization in the same order -- the random starts stay as the fallback of the chains that are not
   * placed --, then the placement, the multilateration over the poses a chain wrote, the range rows and the lift.  Rows of
   * chains that are not placed and of landmarks that are not solved have rangeAidedInitialization's bits.  min_ranges <= 0:
   * 4 x the unknowns of the linear stage (28 at d = 2, 64 at d = 3), a judgement (profiles/chain_placement.md).  A stage
   * never raises the range cost over its own entries; nothing else is promised.  std::runtime_error on a partitioned handle.
   * order: ChainOrder::Greedy (the default: the bits of the call without the argument) or ChainOrder::Levels, the level
   * order with a level's chains placed in the same launches (cora_place_chains_batched_dev): 17 launches per level at 5 steps
   * where the greedy order spends 17 per chain, at the price of ignoring the ranges between chains of one level
   * (profiles/chain_placement_levels.md).
   * consensus: the outlier-robust placement (ChainRangeConsensus; the default is off: the bits of the call without the argument),
   * under either order (cora_place_chains_robust_dev; profiles/chain_consensus.md).  std::invalid_argument for a threshold that
   * is not finite. */
  Matrix multiRobotInitialization(uint64_t seed = 7, int gn_steps = 5, int min_ranges = 0, ChainPlacementInfo *chains_info = nullptr,
                                  LandmarkInitInfo *info = nullptr, ChainOrder order = ChainOrder::Greedy,
                                  ChainRangeConsensus consensus = ChainRangeConsensus()) const;
  /** EXTENSION beyond the reference: multiRobotInitialization with landmarks and chains first placed from the
   * pose-landmark sightings (cora_place_by_sightings_dev), chain 0 fixed: exactly the draws of odometryInitialization in
   * the same order (the new step draws nothing), then the sighting placement, then cora_place_chains_dev for the chains
   * the sightings left (its fixed chains: every chain the sighting step fixed or placed; skipped when none is left), then
   * the multilateration for the landmarks the sightings did not place, the range rows and the lift.  On a problem without
   * sightings the result has multiRobotInitialization's bits.  A landmark that only a range-placed chain sights is not
   * revisited.  min_sightings <= 0: 4 d.  consensus: the outlier-robust sighting step (SightingConsensus; the default is off:
   * the same bits as without the argument); std::invalid_argument for a barc2 that is not finite or a minimum below 1.
   * std::runtime_error on a partitioned handle. */
  Matrix sightingInitialization(uint64_t seed = 7, int gn_steps = 5, int min_ranges = 0, int min_sightings = 0,
                                SightingPlacementInfo *sight_info = nullptr, ChainPlacementInfo *chains_info = nullptr,
                                LandmarkInitInfo *info = nullptr, SightingConsensus consensus = SightingConsensus()) const;
  /** EXTENSION beyond the reference: sightingInitialization with the chains first placed from the relative-pose edges
   * BETWEEN chains (cora_place_by_closures_dev), chain 0 fixed: exactly the draws of odometryInitialization in the same
   * order (the new step draws nothing), then the closure placement, then the sighting placement with every chain of
   * closure status 0 or 4 as its fixed set, then cora_place_chains_dev for the chains still left, the multilateration, the
   * range rows and the lift: one pipeline (odometryStart) with one more step.  On a problem without inter-chain closures
   * the result has sightingInitialization's bits.  min_closures <= 0: 1.  consensus: the outlier-robust closure step
   * (ClosureConsensus; the default is off: the same bits as without the argument); std::invalid_argument for a barc2 that is
   * not finite or a min_consensus below 1.  sighting_consensus: the vote of the sighting step that follows (SightingConsensus,
   * as in sightingInitialization).  std::runtime_error on a partitioned handle. */
  Matrix closureInitialization(uint64_t seed = 7, int gn_steps = 5, int min_ranges = 0, int min_sightings = 0, int min_closures = 0,
                               ClosurePlacementInfo *closure_info = nullptr, SightingPlacementInfo *sight_info = nullptr,
                               ChainPlacementInfo *chains_info = nullptr, LandmarkInitInfo *info = nullptr,
                               ClosureConsensus consensus = ClosureConsensus(),
                               SightingConsensus sighting_consensus = SightingConsensus()) const;

  /********** Certification **************/
  using LambdaBlocks = std::pair<Matrix, Vector>;
  LambdaBlocks compute_Lambda_blocks(const Matrix &Y) const;
  SparseMatrix compute_Lambda_from_Lambda_blocks(const LambdaBlocks &Lambda_blocks, const int &Lambda_size) const;
  SparseMatrix get_certificate_matrix(const Matrix &Y) const;
  /** Everything a first certification needs that does not depend on the point: the elimination order of the certificate
   * matrix, its pattern (Q's plus the Lambda blocks), the symbolic analysis of its factorisation with the factor's
   * storage touched once, and the random start columns of the eigensolver.  solveCORA runs it on a thread of its own
   * WHILE the first TNT solve keeps the device busy (none of it is read by TNT): at 10^5 poses 0.07 s of the first
   * certification's 0.12 s, at 10^6 poses 0.8 of 1.4 s.  Calling it is optional; certify_solution does whatever is missing. */
  void prepareCertification(Index num_eigvecs = 12) const;
  /** Test switches of the eigensolver stage of certify_solution (see FastVerificationLab): without the seed of the failed
   * factorisation and / or without the incomplete-LDL^T preconditioner; and whether the last call got as far as step 3. */
  void setVerificationLab(bool seed_negative_direction, bool use_ildl) {
    cert_lab_on_ = true;
    cert_lab_seed_ = seed_negative_direction;
    cert_lab_ildl_ = use_ildl;
  }
  bool lastCertificationReachedStep3() const { return cert_reached_step3_; }
  CertResults certify_solution(const Matrix &Y, Scalar eta, size_t nx, const Matrix &eigvec_bootstrap,
                               size_t max_LOBPCG_iters = 500) const;
  /** The same for a caller that only needs the decision, theta and the direction x (solveCORA): the eigensolver's Ritz
   * block stays on the device (all_eigvecs comes back EMPTY) and, handed an empty bootstrap, the next call starts from it
   * where it is -- no download and no upload of the N x 12 block per certification (9 + 2 ms at 10^5 poses, 0.1 s at 10^6). */
  CertResults certify_solution_resident(const Matrix &Y, Scalar eta, size_t nx, const Matrix &eigvec_bootstrap,
                                        size_t max_LOBPCG_iters = 500) const;

  /************** Utilities **********************/
  void checkVariablesAreValid(const Matrix &Y) const;
  Matrix alignEstimateToOrigin(const Matrix &Y) const;
  Matrix getTranslationExplicitSolution(const Matrix &Y) const;
  /** Host variable <-> device row count: identity when explicit; [M; 0] / leading rows when implicit. */
  const Matrix &lifted(const Matrix &M, Matrix &tmp) const;
  Matrix lowered(Matrix &&M) const;

  /** Device handle behind the operators (for the resident TNT / LOBPCG loops). */
  cora_ctx *context() const {
    ensureContext();
    return ctx_.get();
  }
  void ensurePreconditionerReady() const { ensurePreconditioner(); }
  Scalar preconditionerLambda() const { return precond_lambda_; }
  long preconditionerNnz() const { return precond_nnz_; }
  int preconditionerLevels() const { return precond_levels_; }
};

}  // namespace CORA
