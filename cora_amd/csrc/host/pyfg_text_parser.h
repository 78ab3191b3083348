// PyFG text ingestion (reference include/CORA/pyfg_text_parser.h:31,
// src/pyfg_text_parser.cpp:112-401).
#pragma once

#include <string>

#include "CORA_problem.h"

namespace CORA {

int getDimFromPyfgFirstLine(const std::string &filename);

/** Parses a PyFG text file into a Problem (defaults as in the reference:
 * Explicit formulation, RegularizedCholesky preconditioner, rank = dim). */
Problem parsePyfgTextToProblem(const std::string &filename);

/** EXTENSION beyond the reference, whose parser drops them: the values of the file's VERTEX_* records as a point of
 * `problem` (normally the Problem parsed from the same file) -- getDataMatrixSize() x d in the explicit layout and the
 * problem's variable order, the reference of Problem::compareToReference.
 *   rotation rows     R_i^T, R_i from the angle / quaternion by the conversion the measurement records use, then
 *                     projectToSOd, so that a quaternion printed to few digits still gives a valid point
 *   range row m       the unit vector (x_t(a) - x_t(b)) / |.| of measurement m's endpoints (a first), the convention of the
 *                     residual x_t(b) - x_t(a) + r x_rho; the first unit vector where the endpoints coincide
 *   translation rows  the records' positions, poses then landmarks
 *   the origin pose that priors add: identity / zero
 * Throws std::runtime_error when a pose or landmark of the problem has no record, std::invalid_argument when the file's
 * dimension is not the problem's. */
Matrix parsePyfgGroundTruth(const std::string &filename, const Problem &problem);

}  // namespace CORA
