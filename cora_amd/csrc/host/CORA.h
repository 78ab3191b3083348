// solveCORA / saddleEscape / projectSolution (reference include/CORA/CORA.h:19-37,
// src/CORA.cpp:26-441): the Riemannian staircase driver.  Host control flow over the
// device-resident TNT and certification.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "CORA_problem.h"
#include "CORA_types.h"
#include "CORA_utils.h"
#include "TNT.h"
#include "pyfg_text_parser.h"

namespace CORA {

using CoraTntResult = TNTResult;
using CoraResult = std::pair<CoraTntResult, std::vector<Matrix>>;

struct CoraSolveInfo {  // extra observability (the reference only prints these)
  bool certified = false;            // the returned (rounded and refined) solution's certificate
  bool relaxation_certified = false; // the staircase stopped because its last level was certified (not at the rank cap)
  int relaxation_rank = 0;           // the rank of that level
  Scalar eta = 0, theta = 0;
  int final_rank = 0;
  int staircase_levels = 0;
  long hessian_vector_products = 0;
  double tnt_seconds = 0, certify_seconds = 0, escape_seconds = 0;  // wall-clock split of the staircase
  // INPUT (the only one; everything above is written by solveCORA): round the certified point with
  // Problem::roundSolution -- on the device -- in place of projectSolution.  Without it nothing changes, down to the bit.
  bool device_rounding = false;
};

CoraResult solveCORA(Problem &problem, const Matrix &x0, int max_relaxation_rank = 20, bool verbose = false,
                     bool log_iterates = false, bool show_iterates = false, CoraSolveInfo *info = nullptr,
                     const TNTParams *params_override = nullptr);

/** EXTENSION beyond the reference: an outlier-robust solve by graduated non-convexity over solveCORA.  The weight step
 * runs on the device (Problem::gncWeights), Q(w) is assembled there (Problem::reweight), and every solve is a full
 * staircase warm-started from the solution before. */
struct GncParams {
  GncCost cost = GncCost::TruncatedLeastSquares;
  MeasurementWeights thresholds;  // barc2 per measurement (Problem::gncWeights); an empty kind is trusted
  bool couple_edges = true;       // a relative pose or pose prior is one measurement
  Scalar mu_factor = 1.4;         // TLS: mu grows by it, GM: mu shrinks by it (down to 1)
  int max_outer = 100;            // cap on the weight-step / solve rounds
};
struct RobustInfo {
  int outer_iterations = 0;                  // weight steps followed by a solve
  std::vector<Scalar> mu_history;            // mu of every weight step (the converging last one of TLS included)
  std::vector<Scalar> sum_wr2_history;       // sum of w r2 over all measurements at those steps
  MeasurementWeights weights;                // the final weights (the Problem is left weighted with them)
  CoraSolveInfo last_solve;                  // of the last solveCORA
  bool converged = false;                    // false: stopped at max_outer
};
/** 1. reweight to ones and solveCORA(x0);  2. statistics with cost None at the solution: rho_max <= 1 returns;
 * 3. mu_0 = 1 / (2 rho_max - 1) (TLS) or 2 rho_max (GM);  4. w = gncWeights(x, mu), reweight(w), solveCORA from x, then
 * mu *= mu_factor (TLS) or mu = max(1, mu / mu_factor) (GM);  TLS stops when a weight step has no weight strictly between
 * 0 and 1 and repeats the weights of the step before, GM after the solve at mu = 1, both at max_outer.
 * x0: as for solveCORA (the problem's current rank); the warm starts are the rank-d solutions. */
CoraResult solveRobustCORA(Problem &problem, const Matrix &x0, const GncParams &params, int max_relaxation_rank = 20,
                           bool verbose = false, RobustInfo *info = nullptr);

Matrix saddleEscape(const Problem &problem, const Matrix &Y, Scalar theta, const Vector &v,
                    Scalar gradient_tolerance, Scalar preconditioned_gradient_tolerance);

Matrix projectSolution(const Problem &problem, const Matrix &Y, bool verbose = false);

}  // namespace CORA
