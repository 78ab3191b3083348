// Odometry initialisation (reference examples/paper_experiments.cpp:375-534,
// getOdomChains / getOdomInitialization): poses by composing the odometry chain of
// each robot, landmarks random, sphere variables from the initial bearing.
#pragma once

#include <random>

#include "CORA_problem.h"

namespace CORA {

// What getOdomInitialization and Problem::odometryInitialization draw, in the order they draw it from
// std::mt19937_64(seed): one place per chain after the first, the landmarks in map order, the fallback directions of the
// degenerate range rows in range order, then the p x p rotation.
namespace odom_draws {
using Uniform = std::uniform_real_distribution<double>;
inline Uniform uniform() { return Uniform(-1.0, 1.0); }
/** d numbers 10 * U: the start of a later chain, a landmark (Random(1, d) * 10, :482-489) */
inline void drawPlace(std::mt19937_64 &g, Uniform &U, int d, double *out) {
  for (int c = 0; c < d; ++c) out[c] = 10.0 * U(g);
}
/** d numbers U: the direction of a range row whose endpoints coincide, before its normalisation */
inline void drawDirection(std::mt19937_64 &g, Uniform &U, int d, double *out) {
  for (int c = 0; c < d; ++c) out[c] = U(g);
}
/** random p x p rotation (:515-531): Gram-Schmidt of a random matrix, determinant fixed to +1 */
Matrix drawRotation(std::mt19937_64 &g, Uniform &U, Index p);
}  // namespace odom_draws

/** N x rank initial iterate (on the manifold). `seed` drives the random landmarks and the
 * random orthogonal mixing of the columns. */
Matrix getOdomInitialization(const Problem &problem, uint64_t seed = 7);

}  // namespace CORA
