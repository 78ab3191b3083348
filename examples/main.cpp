// Command-line driver with the flow of the reference's examples/main.cpp:
//   parse PyFG -> updateProblemData -> random initial guess -> solveCORA(max_rank 10)
//   -> alignEstimateToOrigin, then print the result and optionally save a TUM trajectory.
// Build:  hipcc -O2 -std=c++17 -Iinclude -Icora_amd/csrc/host examples/main.cpp \
//               -Lcora_amd/lib -lcora_hip -Wl,-rpath,$PWD/cora_amd/lib -o cora_main
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "CORA.h"
#include "io.h"
#include "odometry_init.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    std::cout << "Usage: " << argv[0] << " [input .pyfg file] [--jacobi] [--implicit] [--odom-init] [--tum out.tum] [--save-dir dir] [--max-rank r] [--residuals out.csv] [--weights in.csv] [--robust tls|gm --barc2 kind=value[,kind=value...] [--weights-out out.csv]] [--evaluate] [--aligned-tum out.tum] [--rpe step[,step...]] [--rpe-dist L[,L...]] [--device-rounding] [--device-init [--landmark-init [--range-consensus barc2 [--range-min-consensus k]]] [--place-chains [--chain-levels] [--chain-consensus barc2[,min]]] [--sightings [--sighting-consensus barc2 [--sighting-min-consensus k] [--sighting-min-landmark-consensus k]]] [--closures [--closure-consensus barc2 [--closure-min-consensus k]]] [--gn-steps k]]" << std::endl;
    return 1;
  }
  int max_rank = 10, gn_steps = 5;
  std::string tum, save_dir, residuals, weights, robust, barc2, weights_out, aligned_tum, rpe_steps, rpe_dists;
  CORA::ClosureConsensus closure_consensus;
  CORA::RangeConsensus range_consensus;
  CORA::SightingConsensus sighting_consensus;
  CORA::ChainRangeConsensus chain_consensus;
  bool chain_consensus_given = false;
  bool consensus_given = false, range_consensus_given = false, sighting_consensus_given = false;
  bool jacobi = false, implicit = false, odom = false, evaluate = false, device_rounding = false, device_init = false, landmark_init = false, place_chains = false, chain_levels = false, sightings = false, closures = false;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--jacobi") jacobi = true;
    else if (a == "--implicit") implicit = true;   // "formulation": "Implicit" of examples/config.json
    else if (a == "--odom-init") odom = true;      // "init_type": "Odom"
    else if (a == "--tum" && i + 1 < argc) tum = argv[++i];
    else if (a == "--save-dir" && i + 1 < argc) save_dir = argv[++i];  // cora_<robot>.tum / .g2o per robot, like saveSolutions
    else if (a == "--max-rank" && i + 1 < argc) max_rank = std::atoi(argv[++i]);
    // per-measurement residuals of the solution, one line each: kind,first,second,rotation,translation_or_range
    else if (a == "--residuals" && i + 1 < argc) residuals = argv[++i];
    // measurement weights, one line each: kind,index,weight -- kind one of rel_pose_rot, rel_pose_trans, pose_prior_rot,
    // pose_prior_trans, pose_landmark, landmark_prior, range; index in the order of the file's measurements of that kind
    else if (a == "--weights" && i + 1 < argc) weights = argv[++i];
    // outlier-robust solve (solveRobustCORA): the cost, one threshold barc2 per kind named as in --weights (kinds not
    // named are trusted), and a file for the final weights in the --weights format
    else if (a == "--robust" && i + 1 < argc) robust = argv[++i];
    else if (a == "--barc2" && i + 1 < argc) barc2 = argv[++i];
    else if (a == "--weights-out" && i + 1 < argc) weights_out = argv[++i];
    // error of the solution against the input file's own VERTEX_* values after the alignment on all poses' positions;
    // the estimate in the ground truth's frame as a TUM trajectory
    else if (a == "--evaluate") evaluate = true;
    else if (a == "--aligned-tum" && i + 1 < argc) aligned_tum = argv[++i];
    // relative pose error of the solution against the file's own VERTEX_* values (no alignment needed): pairs a fixed
    // number of steps apart, pairs at least a path length apart along the ground truth
    else if (a == "--rpe" && i + 1 < argc) rpe_steps = argv[++i];
    else if (a == "--rpe-dist" && i + 1 < argc) rpe_dists = argv[++i];
    // the certified point is rounded on the device (Problem::roundSolution) in place of projectSolution
    else if (a == "--device-rounding") device_rounding = true;
    // with --odom-init: the start is composed on the device (Problem::odometryInitialization) in place of getOdomInitialization
    else if (a == "--device-init") device_init = true;
    // with --odom-init --device-init: the landmarks of the start are placed from the ranges (Problem::rangeAidedInitialization)
    else if (a == "--landmark-init") landmark_init = true;
    // with --landmark-init: a consensus vote in front of each landmark's fit (RangeConsensus): the threshold on a range's weighted
    // squared residual, and the votes the elected proposal needs (0: d + 2)
    else if (a == "--range-consensus" && i + 1 < argc) range_consensus.barc2 = std::atof(argv[++i]), range_consensus_given = true;
    else if (a == "--range-min-consensus" && i + 1 < argc) range_consensus.min_consensus = std::atoi(argv[++i]), range_consensus_given = true;
    else if (a == "--gn-steps" && i + 1 < argc) gn_steps = std::atoi(argv[++i]);
    // with --odom-init --device-init: the chains after the first are first placed from the pose-pose ranges between chains
    // (Problem::multiRobotInitialization, which then places the landmarks as --landmark-init does)
    else if (a == "--place-chains") place_chains = true;
    // with --place-chains: the level order, a level's chains placed together (ChainOrder::Levels)
    else if (a == "--chain-levels") chain_levels = true;
    // with --place-chains: a consensus vote in front of each chain's fit (ChainRangeConsensus): barc2[,min], the threshold on a
    // range's weighted squared residual and the least consensus (default 2 m, m = 8 / 17)
    else if (a == "--chain-consensus" && i + 1 < argc) {
      const std::string v = argv[++i];
      const size_t comma = v.find(',');
      chain_consensus.barc2 = std::atof(v.substr(0, comma).c_str());
      if (comma != std::string::npos) chain_consensus.min_consensus = std::atoi(v.substr(comma + 1).c_str());
      chain_consensus_given = true;
    }
    // with --odom-init --device-init: landmarks and chains are first placed from the pose-landmark sightings, then the chains
    // that are left from the ranges and the landmarks that are left by multilateration (Problem::sightingInitialization)
    else if (a == "--sightings") sightings = true;
    // with --sightings: a consensus vote in front of every fit of the sighting step (SightingConsensus): the threshold on a
    // sighting's tau |.|^2, and the votes the elected proposal of a chain (0: d + 1) and of a landmark needs
    else if (a == "--sighting-consensus" && i + 1 < argc) sighting_consensus.barc2 = std::atof(argv[++i]), sighting_consensus_given = true;
    else if (a == "--sighting-min-consensus" && i + 1 < argc) sighting_consensus.min_chain_consensus = std::atoi(argv[++i]), sighting_consensus_given = true;
    else if (a == "--sighting-min-landmark-consensus" && i + 1 < argc) sighting_consensus.min_landmark_consensus = std::atoi(argv[++i]), sighting_consensus_given = true;
    // with --odom-init --device-init: the chains are first placed from the relative-pose edges between chains, then everything
    // --sightings does (Problem::closureInitialization)
    else if (a == "--closures") closures = true;
    // with --closures: a consensus vote in front of each chain's fit (ClosureConsensus): the threshold on a closure's coupled
    // rot + trans residual, and the votes the elected closure needs
    else if (a == "--closure-consensus" && i + 1 < argc) closure_consensus.barc2 = std::atof(argv[++i]), consensus_given = true;
    else if (a == "--closure-min-consensus" && i + 1 < argc) closure_consensus.min_consensus = std::atoi(argv[++i]), consensus_given = true;
  }
  using clk = std::chrono::steady_clock;
  auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  try {
    if (device_init && !odom) throw std::runtime_error("--device-init composes the odometry start on the device: it needs --odom-init");
    if (place_chains && !device_init) throw std::runtime_error("--place-chains places the chains of the device's odometry start: it needs --odom-init --device-init");
    if (chain_levels && !place_chains) throw std::runtime_error("--chain-levels chooses the order of --place-chains: it needs --place-chains");
    if (chain_consensus_given && !place_chains) throw std::runtime_error("--chain-consensus sets the vote of --place-chains: it needs --place-chains");
    if (chain_consensus_given && !(chain_consensus.barc2 > 0)) throw std::runtime_error("--chain-consensus: expected a threshold > 0");
    if (sightings && !device_init) throw std::runtime_error("--sightings places landmarks and chains of the device's odometry start: it needs --odom-init --device-init");
    if (closures && !device_init) throw std::runtime_error("--closures places the chains of the device's odometry start: it needs --odom-init --device-init");
    if (consensus_given && !closures) throw std::runtime_error("--closure-consensus and --closure-min-consensus set the vote of the closure step: they need --closures");
    if (consensus_given && !(closure_consensus.barc2 > 0)) throw std::runtime_error("--closure-consensus: expected a threshold > 0");
    if (sighting_consensus_given && !sightings) throw std::runtime_error("--sighting-consensus, --sighting-min-consensus and --sighting-min-landmark-consensus set the vote of the sighting step: they need --sightings");
    if (sighting_consensus_given && !(sighting_consensus.barc2 > 0)) throw std::runtime_error("--sighting-consensus: expected a threshold > 0");
    if (range_consensus_given && !landmark_init) throw std::runtime_error("--range-consensus and --range-min-consensus set the vote of the landmark step: they need --landmark-init");
    if (range_consensus_given && !(range_consensus.barc2 > 0)) throw std::runtime_error("--range-consensus: expected a threshold > 0");
    if (landmark_init && !device_init) throw std::runtime_error("--landmark-init places the landmarks of the device's odometry start: it needs --odom-init --device-init");
    const auto t_start = clk::now();
    CORA::Problem problem = CORA::parsePyfgTextToProblem(argv[1]);
    const auto t_parsed = clk::now();
    if (jacobi) problem.setPreconditioner(CORA::Preconditioner::Jacobi);
    if (implicit) problem.setFormulation(CORA::Formulation::Implicit);
    problem.updateProblemData();
    if (!weights.empty()) {  // (an extension beyond the reference: Problem::setMeasurementWeights)
      std::ifstream csv(weights);
      if (!csv) throw std::runtime_error("cannot read " + weights);
      CORA::MeasurementWeights w;
      const size_t npp = problem.getRPMs().size(), npr = problem.getPosePriors().size();
      const std::pair<const char *, std::pair<std::vector<CORA::Scalar> *, size_t>> kinds[] = {
          {"rel_pose_rot", {&w.rel_pose_rot, npp}},     {"rel_pose_trans", {&w.rel_pose_trans, npp}},
          {"pose_prior_rot", {&w.pose_prior_rot, npr}}, {"pose_prior_trans", {&w.pose_prior_trans, npr}},
          {"pose_landmark", {&w.pose_landmark, problem.getRPLMs().size()}},
          {"landmark_prior", {&w.landmark_prior, problem.getLandmarkPriors().size()}},
          {"range", {&w.range, problem.getRangeMeasurements().size()}}};
      std::string text;
      size_t lines = 0;
      while (std::getline(csv, text)) {
        if (text.empty() || text[0] == '#') continue;
        const size_t c1 = text.find(','), c2 = text.find(',', c1 == std::string::npos ? c1 : c1 + 1);
        if (c2 == std::string::npos) throw std::runtime_error(weights + ": expected kind,index,weight, got '" + text + "'");
        const std::string kind = text.substr(0, c1);
        const size_t index = std::stoul(text.substr(c1 + 1, c2 - c1 - 1));
        const double value = std::stod(text.substr(c2 + 1));
        bool known = false;
        for (const auto &k : kinds) {
          if (kind != k.first) continue;
          known = true;
          if (index >= k.second.second) throw std::runtime_error(weights + ": no " + kind + " measurement " + std::to_string(index));
          if (k.second.first->empty()) k.second.first->assign(k.second.second, 1.0);
          (*k.second.first)[index] = value;
        }
        if (!known) throw std::runtime_error(weights + ": unknown kind '" + kind + "'");
        ++lines;
      }
      problem.setMeasurementWeights(w);
      std::cout << "read " << weights << " (" << lines << " weights)" << std::endl;
    }
    const auto t_assembled = clk::now();
    problem.ensurePreconditionerReady();  // device copy of Q, Cholesky factor, solve plan
    const auto t_device = clk::now();
    std::printf("poses %d  landmarks %d  ranges %d  N %d  nnz(Q) %ld\n", problem.numPoses(), problem.numLandmarks(),
                problem.numRangeMeasurements(), problem.getDataMatrixSize(),
                static_cast<long>(problem.data_matrix_.nonZeros()));
    CORA::Matrix x0 = !odom ? problem.getRandomInitialGuess()
                      : device_init ? problem.odometryInitialization() : CORA::getOdomInitialization(problem);
    if (landmark_init) {  // (an extension beyond the reference: Problem::rangeAidedInitialization)
      CORA::LandmarkInitInfo lm;
      auto range_sum = [&](const CORA::Matrix &x) {  // (the implicit formulation's variable has no translation rows)
        return problem.measurementResiduals(implicit ? CORA::Matrix(x.block(0, 0, problem.rotAndRangeMatrixSize(), x.cols())) : x).range_sum;
      };
      const double without = range_sum(x0);
      x0 = problem.rangeAidedInitialization(7, gn_steps, &lm, range_consensus);
      std::printf("landmark init: %ld landmarks solved, %ld not solved (%ld Gauss-Newton steps); range residual sum at the start %.6e with it, %.6e without\n",
                  lm.solved, lm.not_solved, lm.gn_steps, range_sum(x0), without);
      if (range_consensus_given) {
        double least = 1.0;  // the smallest consensus / list length over the landmarks that were voted on
        for (size_t l = 0; l < lm.list_len.size(); ++l)
          if (lm.list_len[l] > 0 && (lm.status[l] == 0 || lm.status[l] == 2 || lm.status[l] == 5))
            least = std::min(least, static_cast<double>(lm.consensus[l]) / lm.list_len[l]);
        std::printf("range consensus: %ld landmarks without consensus, %ld ranges excluded; smallest consensus / list length %.4f\n",
                    lm.no_consensus, lm.ranges_excluded, least);
      }
    }
    if (place_chains) {  // (an extension beyond the reference: Problem::multiRobotInitialization)
      CORA::ChainPlacementInfo ci;
      auto range_sum = [&](const CORA::Matrix &x) {
        return problem.measurementResiduals(implicit ? CORA::Matrix(x.block(0, 0, problem.rotAndRangeMatrixSize(), x.cols())) : x).range_sum;
      };
      const double without = range_sum(x0);  // (the start as it stands: with the landmarks placed under --landmark-init)
      x0 = problem.multiRobotInitialization(7, gn_steps, 0, &ci, nullptr, chain_levels ? CORA::ChainOrder::Levels : CORA::ChainOrder::Greedy,
                                            chain_consensus);
      std::printf("chain placement: %ld chains placed, %ld not placed (%ld Gauss-Newton steps); range residual sum at the start %.6e with it, %.6e without\n",
                  ci.placed, ci.not_placed, ci.gn_steps, range_sum(x0), without);
      if (chain_levels) std::printf("chain placement: level order, %ld stages in %ld levels\n", ci.stages, ci.levels);
      if (chain_consensus_given) {
        double least = 1.0;  // the smallest consensus / list length over the stages
        for (size_t ch = 0; ch < ci.list_len.size(); ++ch)
          if (ci.list_len[ch] > 0) least = std::min(least, static_cast<double>(ci.consensus[ch]) / ci.list_len[ch]);
        std::printf("chain consensus: %ld chains without consensus, %ld ranges excluded; smallest consensus / list length %.4f\n", ci.no_consensus,
                    ci.ranges_excluded, least);
      }
    }
    if (sightings) {  // (an extension beyond the reference: Problem::sightingInitialization)
      CORA::SightingPlacementInfo si;
      auto sighting_sum = [&](const CORA::Matrix &x) {
        const CORA::MeasurementResiduals res =
            problem.measurementResiduals(implicit ? CORA::Matrix(x.block(0, 0, problem.rotAndRangeMatrixSize(), x.cols())) : x);
        double sum = 0;
        for (const double v : res.pose_landmark) sum += v;
        return sum;
      };
      const double without = sighting_sum(x0);  // (the start as it stands)
      x0 = problem.sightingInitialization(7, gn_steps, 0, 0, &si, nullptr, nullptr, sighting_consensus);
      std::printf("sighting placement: %ld chains fixed or placed, %ld not placed; %ld landmarks placed, %ld not placed (%ld stages); sighting cost at the start %.6e with it, %.6e without\n",
                  si.chains_fixed + si.chains_placed, si.chains_not_placed, si.landmarks_placed, si.landmarks_not_placed, si.stages,
                  sighting_sum(x0), without);
      if (sighting_consensus_given) {
        double least = 1.0;  // the smallest consensus / list length over the chains' lists and the REFIT's lists
        for (size_t ch = 0; ch < si.chain_list_len.size(); ++ch)
          if (si.chain_list_len[ch] > 0) least = std::min(least, static_cast<double>(si.chain_consensus[ch]) / si.chain_list_len[ch]);
        for (size_t l = 0; l < si.landmark_list_len.size(); ++l)
          if (si.landmark_list_len[l] > 0) least = std::min(least, static_cast<double>(si.landmark_consensus[l]) / si.landmark_list_len[l]);
        std::printf("sighting consensus: %ld chains without consensus, %ld landmarks without consensus, %ld chain sightings excluded, %ld landmark sightings excluded; smallest consensus / list length %.4f\n",
                    si.chains_no_consensus, si.landmarks_no_consensus, si.chain_entries_excluded, si.landmark_entries_excluded, least);
      }
    }
    if (closures) {  // (an extension beyond the reference: Problem::closureInitialization)
      CORA::ClosurePlacementInfo li;
      const CORA::Matrix without = problem.sightingInitialization(7, gn_steps);  // (the same pipeline without the step)
      x0 = problem.closureInitialization(7, gn_steps, 0, 0, 0, &li, nullptr, nullptr, nullptr, closure_consensus);
      // the closure cost: the table's own rot + trans residuals of the relative-pose edges that are no edge of a chain
      std::vector<char> in_chain(static_cast<size_t>(problem.numPosePoseMeasurements()), 0);
      for (const auto &ch : problem.odometryChains())
        for (const int32_t e : ch) in_chain[static_cast<size_t>(e)] = 1;
      auto closure_sum = [&](const CORA::Matrix &x) {
        const CORA::MeasurementResiduals res =
            problem.measurementResiduals(implicit ? CORA::Matrix(x.block(0, 0, problem.rotAndRangeMatrixSize(), x.cols())) : x);
        double sum = 0;
        for (size_t e = 0; e < in_chain.size(); ++e)
          if (!in_chain[e]) sum += res.rel_pose_rot[e] + res.rel_pose_trans[e];
        return sum;
      };
      std::printf("closure placement: %ld chains fixed or placed, %ld not placed, %ld refused (%ld stages, %ld closures used, %ld edges skipped or unused); closure cost at the start %.6e with it, %.6e without\n",
                  li.chains_fixed + li.chains_placed, li.chains_not_placed, li.chains_refused, li.stages, li.closures_used, li.edges_skipped,
                  closure_sum(x0), closure_sum(without));
      if (consensus_given) {
        double least = 1.0;  // the smallest consensus / list length over the taken chains
        for (size_t ch = 0; ch < li.list_len.size(); ++ch)
          if (li.list_len[ch] > 0) least = std::min(least, static_cast<double>(li.consensus[ch]) / li.list_len[ch]);
        std::printf("closure consensus: %ld chains without consensus, %ld closures excluded; smallest consensus / list length %.4f\n",
                    li.chains_no_consensus, li.closures_excluded, least);
      }
    }
    if (odom && implicit)  // examples/paper_experiments.cpp:623-625
      x0 = x0.block(0, 0, problem.rotAndRangeMatrixSize(), x0.cols());
    CORA::CoraSolveInfo info;
    info.device_rounding = device_rounding;  // (an extension beyond the reference: CoraSolveInfo::device_rounding)
    CORA::CoraResult soln;
    if (device_rounding && !robust.empty()) throw std::runtime_error("--device-rounding applies to the plain solve, not to --robust");
    if (robust.empty()) {
      if (!barc2.empty() || !weights_out.empty()) throw std::runtime_error("--barc2 and --weights-out need --robust tls|gm");
      soln = CORA::solveCORA(problem, x0, max_rank, /*verbose=*/true, false, false, &info);
    } else {  // (an extension beyond the reference: solveRobustCORA)
      CORA::GncParams gnc;
      if (robust == "tls") gnc.cost = CORA::GncCost::TruncatedLeastSquares;
      else if (robust == "gm") gnc.cost = CORA::GncCost::GemanMcClure;
      else throw std::runtime_error("--robust: expected tls or gm, got '" + robust + "'");
      const size_t npp = problem.getRPMs().size(), npr = problem.getPosePriors().size();
      const std::pair<const char *, std::pair<std::vector<CORA::Scalar> *, size_t>> kinds[] = {
          {"rel_pose_rot", {&gnc.thresholds.rel_pose_rot, npp}},     {"rel_pose_trans", {&gnc.thresholds.rel_pose_trans, npp}},
          {"pose_prior_rot", {&gnc.thresholds.pose_prior_rot, npr}}, {"pose_prior_trans", {&gnc.thresholds.pose_prior_trans, npr}},
          {"pose_landmark", {&gnc.thresholds.pose_landmark, problem.getRPLMs().size()}},
          {"landmark_prior", {&gnc.thresholds.landmark_prior, problem.getLandmarkPriors().size()}},
          {"range", {&gnc.thresholds.range, problem.getRangeMeasurements().size()}}};
      for (size_t at = 0; at < barc2.size();) {
        const size_t end = std::min(barc2.find(',', at), barc2.size()), eq = barc2.find('=', at);
        if (eq == std::string::npos || eq >= end) throw std::runtime_error("--barc2: expected kind=value, got '" + barc2.substr(at, end - at) + "'");
        const std::string kind = barc2.substr(at, eq - at);
        const double value = std::stod(barc2.substr(eq + 1, end - eq - 1));
        bool known = false;
        for (const auto &k : kinds)
          if (kind == k.first) {
            known = true;
            k.second.first->assign(k.second.second, value);
          }
        if (!known) throw std::runtime_error("--barc2: unknown kind '" + kind + "'");
        at = end + 1;
      }
      CORA::RobustInfo rinfo;
      soln = CORA::solveRobustCORA(problem, x0, gnc, max_rank, /*verbose=*/true, &rinfo);
      info = rinfo.last_solve;
      const CORA::MeasurementWeights &w = rinfo.weights;
      const std::pair<const char *, const std::vector<CORA::Scalar> *> out_kinds[] = {
          {"rel_pose_rot", &w.rel_pose_rot}, {"rel_pose_trans", &w.rel_pose_trans}, {"pose_prior_rot", &w.pose_prior_rot},
          {"pose_prior_trans", &w.pose_prior_trans}, {"pose_landmark", &w.pose_landmark}, {"landmark_prior", &w.landmark_prior},
          {"range", &w.range}};
      size_t below_half = 0, total = 0;
      for (const auto &k : out_kinds)
        for (const CORA::Scalar v : *k.second) {
          ++total;
          if (v < 0.5) ++below_half;
        }
      std::printf("robust solve (%s): %d rounds, %s, %zu of %zu weights below 1/2\n", robust.c_str(), rinfo.outer_iterations,
                  rinfo.converged ? "converged" : "stopped at the cap", below_half, total);
      if (!weights_out.empty()) {
        std::ofstream csv(weights_out);
        if (!csv) throw std::runtime_error("cannot write " + weights_out);
        csv.precision(17);
        for (const auto &k : out_kinds)
          for (size_t i = 0; i < k.second->size(); ++i) csv << k.first << ',' << i << ',' << (*k.second)[i] << '\n';
        std::cout << "wrote " << weights_out << " (" << total << " weights)" << std::endl;
      }
    }
    const auto t_solved = clk::now();
    const CORA::Matrix aligned = problem.alignEstimateToOrigin(soln.first.x);
    std::printf("final cost %.9g  |grad| %.3e  certified %d  theta %.3e  staircase levels %d  Hvps %ld  %.3f s\n",
                soln.first.f, soln.first.gradfx_norm, static_cast<int>(info.certified), info.theta,
                info.staircase_levels, info.hessian_vector_products, soln.first.elapsed_time);
    std::printf("wall clock: parse %.3f s | assemble Q %.3f s | device setup + preconditioner %.3f s | solve %.3f s "
                "(TNT %.3f, certification %.3f, saddle escape %.3f)\n",
                secs(t_start, t_parsed), secs(t_parsed, t_assembled), secs(t_assembled, t_device),
                secs(t_device, t_solved), info.tnt_seconds, info.certify_seconds, info.escape_seconds);
    if (!residuals.empty()) {  // (an extension beyond the reference: Problem::measurementResiduals)
      const CORA::MeasurementResiduals res = problem.measurementResiduals(soln.first.x);
      std::ofstream csv(residuals);
      if (!csv) throw std::runtime_error("cannot write " + residuals);
      csv.precision(17);
      const std::string origin = problem.getOriginSymbol().string();
      size_t lines = 0;
      auto line = [&](const char *kind, const std::string &first, const std::string &second, double rot, double other) {
        csv << kind << ',' << first << ',' << second << ',' << rot << ',' << other << '\n';
        ++lines;
      };
      for (size_t i = 0; i < problem.getRPMs().size(); ++i)
        line("rel_pose", problem.getRPMs()[i].first_id.string(), problem.getRPMs()[i].second_id.string(),
             res.rel_pose_rot[i], res.rel_pose_trans[i]);
      for (size_t i = 0; i < problem.getPosePriors().size(); ++i)
        line("pose_prior", origin, problem.getPosePriors()[i].id.string(), res.pose_prior_rot[i], res.pose_prior_trans[i]);
      for (size_t i = 0; i < problem.getRPLMs().size(); ++i)
        line("pose_landmark", problem.getRPLMs()[i].first_id.string(), problem.getRPLMs()[i].second_id.string(), 0.0,
             res.pose_landmark[i]);
      for (size_t i = 0; i < problem.getLandmarkPriors().size(); ++i)
        line("landmark_prior", origin, problem.getLandmarkPriors()[i].id.string(), 0.0, res.landmark_prior[i]);
      for (size_t i = 0; i < problem.getRangeMeasurements().size(); ++i)
        line("range", problem.getRangeMeasurements()[i].first_id.string(), problem.getRangeMeasurements()[i].second_id.string(),
             0.0, res.range[i]);
      std::printf("residuals: rotation %.9g  translation %.9g  range %.9g  half of their total %.9g  (final cost %.9g)\n",
                  res.rot_sum, res.trans_sum, res.range_sum, 0.5 * (res.rot_sum + res.trans_sum + res.range_sum), soln.first.f);
      std::cout << "wrote " << residuals << " (" << lines << " measurements)" << std::endl;
    }
    if (evaluate || !aligned_tum.empty()) {  // (an extension beyond the reference: Problem::compareToReference)
      const CORA::Matrix truth = CORA::parsePyfgGroundTruth(argv[1], problem);
      const CORA::TrajectoryComparison cmp = problem.compareToReference(soln.first.x, truth, {}, true, !aligned_tum.empty());
      // a pose's rotation error as an angle: 2 asin(e / (2 sqrt 2)) of its chordal error e; the RMSE is over these angles
      const auto degrees = [](double chordal) { return 2.0 * std::asin(std::min(1.0, chordal / (2.0 * std::sqrt(2.0)))) * 180.0 / 3.14159265358979323846; };
      if (evaluate) {
        // the origin pose that priors add is no pose of a robot (compareToReference leaves it out under the same condition)
        const bool has_origin = problem.getNumPosePriors() + problem.getNumLandmarkPriors() > 0;
        // one line from the per-pose errors of the poses with symbol character chr (0: all), under the joint alignment
        const auto line = [&](unsigned char chr) {
          double t2 = 0, a2 = 0, tmax = 0, amax = 0;
          long count = 0;
          for (const auto &kv : problem.getPoseSymbolMap()) {
            if ((chr && kv.first.chr() != chr) || (has_origin && kv.first == problem.getOriginSymbol())) continue;
            const double et = cmp.pose_trans_err[static_cast<size_t>(kv.second)];
            const double ang = degrees(cmp.pose_rot_err[static_cast<size_t>(kv.second)]);
            t2 += et * et;
            a2 += ang * ang;
            tmax = std::max(tmax, et);
            amax = std::max(amax, ang);
            ++count;
          }
          const double n = static_cast<double>(std::max(count, 1L));
          if (chr) std::printf("evaluate: robot '%c' ", chr);
          else std::printf("evaluate: ");
          std::printf("%ld poses  translation RMSE %.6g max %.6g  rotation RMSE %.6g deg max %.6g deg\n", count, std::sqrt(t2 / n), tmax,
                      std::sqrt(a2 / n), amax);
        };
        line(0);
        std::vector<unsigned char> robots;
        for (const auto &kv : problem.getPoseSymbolMap())
          if (!(has_origin && kv.first == problem.getOriginSymbol()) && std::find(robots.begin(), robots.end(), kv.first.chr()) == robots.end())
            robots.push_back(kv.first.chr());
        if (robots.size() > 1)
          for (const unsigned char chr : robots) line(chr);
        std::printf("evaluate: %ld landmarks  position RMSE %.6g max %.6g\n", cmp.num_landmarks, cmp.landmarkRmse(), cmp.max_landmark_err);
      }
      if (!aligned_tum.empty()) {
        CORA::saveSolnToTum(problem, cmp.aligned, aligned_tum);
        std::cout << "wrote " << aligned_tum << std::endl;
      }
    }
    if (!rpe_steps.empty() || !rpe_dists.empty()) {  // (an extension beyond the reference: Problem::relativeError)
      const CORA::Matrix truth = CORA::parsePyfgGroundTruth(argv[1], problem);
      const auto degrees = [](double chordal) { return 2.0 * std::asin(std::min(1.0, chordal / (2.0 * std::sqrt(2.0)))) * 180.0 / 3.14159265358979323846; };
      // the rotation RMSE is over the pairs' angles, as in --evaluate; the drift is the mean of error / path length
      const auto line = [&](const std::string &setting, const CORA::PosePairs &pairs) {
        const CORA::RelativeError e = problem.relativeError(soln.first.x, truth, pairs);
        double a2 = 0, amax = 0, adrift = 0;
        long with_length = 0;
        for (size_t p = 0; p < e.rot_err.size(); ++p) {
          const double ang = degrees(e.rot_err[p]);
          a2 += ang * ang;
          amax = std::max(amax, ang);
          if (e.path_length[p] > 0) {
            adrift += ang / e.path_length[p];
            ++with_length;
          }
        }
        const double n = static_cast<double>(std::max(e.num_pairs, 1L));
        std::printf("rpe: %s %ld pairs  translation RMSE %.6g max %.6g  rotation RMSE %.6g deg max %.6g deg  drift %.6g per unit %.6g deg per unit\n",
                    setting.c_str(), e.num_pairs, e.transRmse(), e.max_trans_err, std::sqrt(a2 / n), amax, e.meanTransDrift(),
                    with_length > 0 ? adrift / static_cast<double>(with_length) : 0.0);
      };
      const auto each = [](const std::string &list, const std::function<void(const std::string &)> &fn) {
        std::stringstream ss(list);
        std::string item;
        while (std::getline(ss, item, ','))
          if (!item.empty()) fn(item);
      };
      each(rpe_steps, [&](const std::string &v) { line("step " + v, problem.posePairsByStep(std::atoi(v.c_str()))); });
      each(rpe_dists, [&](const std::string &v) { line("distance " + v, problem.posePairsByDistance(truth, std::atof(v.c_str()))); });
    }
    if (!tum.empty()) {
      CORA::saveSolnToTum(problem, aligned, tum);
      std::cout << "wrote " << tum << std::endl;
    }
    if (!save_dir.empty()) {  // examples/paper_experiments.cpp:536-592: one trajectory file pair per robot chain
      std::vector<unsigned char> robots;
      for (const auto &kv : problem.getPoseSymbolMap())
        if (!(kv.first == problem.getOriginSymbol()) &&
            std::find(robots.begin(), robots.end(), kv.first.chr()) == robots.end())
          robots.push_back(kv.first.chr());
      for (size_t r = 0; r < robots.size(); ++r) {
        const auto chain = problem.getPoseSymbols(robots[r]);
        const std::string base = save_dir + "/cora_" + std::to_string(r);
        CORA::saveSolnToTum(chain, problem, aligned, base + ".tum");
        CORA::saveSolnToG20(chain, problem, aligned, base + ".g2o");
        std::cout << "wrote " << base << ".tum / .g2o (" << chain.size() << " poses of robot '" << robots[r] << "')" << std::endl;
      }
    }
  } catch (const std::exception &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
