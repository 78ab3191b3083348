// The term map of Q(w) (TermMap, cora_internal.h): which measurement weights every stored entry of Q is a sum over, and
// with which coefficients.  Host code; the kernels that execute the map are in kernels/assemble.inc.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <stdexcept>
#include <string>

#include "cora_internal.h"

namespace cora {

namespace {

// position of (row, col) in the CSR, -1 when the pattern does not have it.  `order` lists every row's positions by
// ascending column (the CSR's own order where the row is sorted already).
struct PatternIndex {
  const int32_t *rowptr, *col;
  std::vector<int32_t> order;
  PatternIndex(int64_t N, const int32_t *rp, const int32_t *ci) : rowptr(rp), col(ci) {
    if (rp[0] != 0) throw std::runtime_error("rowptr[0] must be 0");
    for (int64_t i = 0; i < N; ++i)
      if (rp[i + 1] < rp[i]) throw std::runtime_error("rowptr not monotone");
    order.resize(static_cast<size_t>(rp[N]));
    std::iota(order.begin(), order.end(), 0);
    for (int64_t i = 0; i < N; ++i) {
      int32_t *b = order.data() + rp[i], *e = order.data() + rp[i + 1];
      for (int32_t *p = b; p < e; ++p)
        if (ci[*p] < 0 || ci[*p] >= N) throw std::runtime_error("column index out of range");
      if (!std::is_sorted(b, e, [&](int32_t x, int32_t y) { return ci[x] < ci[y]; }))
        std::sort(b, e, [&](int32_t x, int32_t y) { return ci[x] < ci[y]; });
      for (int32_t *p = b; p + 1 < e; ++p)
        if (ci[p[0]] == ci[p[1]])
          throw std::runtime_error("row " + std::to_string(i) + " repeats a column index: such a matrix has no term map (merge the duplicates)");
    }
  }
  int32_t find(int32_t row, int32_t c) const {
    const int32_t *b = order.data() + rowptr[row], *e = order.data() + rowptr[row + 1];
    const int32_t *p = std::lower_bound(b, e, c, [&](int32_t x, int32_t cc) { return col[x] < cc; });
    return (p < e && col[*p] == c) ? *p : -1;
  }
};

}  // namespace

void build_term_map(int d, int64_t N, const int32_t *rowptr, const int32_t *col, int64_t n_edges, const int32_t *edge_rows,
                    const double *edge_data, int64_t n_ranges, const int32_t *range_rows, const double *range_data,
                    TermMap &M) {
  const PatternIndex P(N, rowptr, col);
  const int64_t nnz = rowptr[N], ne = n_edges, nr = n_ranges;
  auto field = [&](int f, int64_t e) { return edge_data[static_cast<size_t>(f) * ne + e]; };

  // every term in map order (ascending weight index, the documented enumeration inside a measurement)
  auto for_each_term = [&](auto &&emit) {
    for (int64_t e = 0; e < ne; ++e) {  // rotation parts: weight e
      const int32_t ra = edge_rows[4 * e], rb = edge_rows[4 * e + 1];
      if (rb < 0) continue;
      const double kappa = field(d * d + d, e);
      const int32_t w = static_cast<int32_t>(e);
      for (int k = 0; k < d; ++k) emit(ra + k, ra + k, w, kappa, "rotation part of edge", e);
      for (int k = 0; k < d; ++k) emit(rb + k, rb + k, w, kappa, "rotation part of edge", e);
      for (int a = 0; a < d; ++a)
        for (int c = 0; c < d; ++c) emit(ra + a, rb + c, w, -kappa * field(a * d + c, e), "rotation part of edge", e);
      for (int a = 0; a < d; ++a)
        for (int c = 0; c < d; ++c) emit(rb + c, ra + a, w, -kappa * field(a * d + c, e), "rotation part of edge", e);
    }
    for (int64_t e = 0; e < ne; ++e) {  // translation parts: weight n_edges + e
      int32_t u[5];
      double v[5];
      for (int k = 0; k < d; ++k) {
        u[k] = edge_rows[4 * e] + k;
        v[k] = -field(d * d + k, e);
      }
      u[d] = edge_rows[4 * e + 2];
      v[d] = -1.0;
      u[d + 1] = edge_rows[4 * e + 3];
      v[d + 1] = 1.0;
      const double tau = field(d * d + d + 1, e);
      const int32_t w = static_cast<int32_t>(ne + e);
      for (int i = 0; i < d + 2; ++i)
        for (int j = 0; j < d + 2; ++j) emit(u[i], u[j], w, tau * (v[i] * v[j]), "translation part of edge", e);
    }
    for (int64_t m = 0; m < nr; ++m) {  // ranges: weight 2 n_edges + m
      const int32_t u[3] = {range_rows[3 * m], range_rows[3 * m + 1], range_rows[3 * m + 2]};
      const double v[3] = {range_data[m], -1.0, 1.0}, omega = range_data[nr + m];
      const int32_t w = static_cast<int32_t>(2 * ne + m);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) emit(u[i], u[j], w, omega * (v[i] * v[j]), "range", m);
    }
  };

  if (d < 1 || d > 3) throw std::runtime_error("dimension must be 1, 2 or 3");
  if (2 * ne + nr >= (int64_t{1} << 31)) throw std::runtime_error("2^31 weights or more");
  TermMap T;
  T.nnz = nnz;
  T.n_edges = ne;
  T.n_ranges = nr;
  T.n_weights = 2 * ne + nr;
  // pass 1: the CSR position of every kept term (in map order) and the count per entry
  std::vector<int64_t> count(static_cast<size_t>(nnz) + 1, 0);
  std::vector<int32_t> where;
  where.reserve(static_cast<size_t>(ne) * (2 * d + 2 * d * d + (d + 2) * (d + 2)) + static_cast<size_t>(nr) * 9);
  int64_t total = 0;
  for_each_term([&](int32_t row, int32_t c, int32_t, double coef, const char *what, int64_t id) {
    const int32_t q = P.find(row, c);
    if (q < 0) {
      if (coef == 0.0) {  // (a structural zero the pattern does not keep)
        where.push_back(-1);
        return;
      }
      throw std::runtime_error(std::string("the ") + what + " " + std::to_string(id) + " has a nonzero term at (" +
                               std::to_string(row) + ", " + std::to_string(c) + "), which the sparsity pattern of the handle's matrix does not hold");
    }
    where.push_back(q);
    ++count[static_cast<size_t>(q)];
    ++total;
  });
  if (total >= (int64_t{1} << 31)) throw std::runtime_error("2^31 terms or more: the term map indexes them with 32 bits");
  T.n_terms = total;
  T.tptr.resize(static_cast<size_t>(nnz) + 1);
  int64_t at = 0;
  for (int64_t q = 0; q < nnz; ++q) {
    T.tptr[static_cast<size_t>(q)] = static_cast<int32_t>(at);
    T.max_terms = std::max(T.max_terms, count[static_cast<size_t>(q)]);
    if (count[static_cast<size_t>(q)] > kLongEntry) T.long_entries.push_back(static_cast<int32_t>(q));
    at += count[static_cast<size_t>(q)];
  }
  T.tptr[static_cast<size_t>(nnz)] = static_cast<int32_t>(at);
  // pass 2: the terms again in the same order, each behind the ones its entry already has (a stable counting sort)
  T.tweight.resize(static_cast<size_t>(total));
  T.tcoef.resize(static_cast<size_t>(total));
  std::vector<int32_t> fill(T.tptr.begin(), T.tptr.end() - 1);
  size_t seq = 0;
  for_each_term([&](int32_t, int32_t, int32_t w, double coef, const char *, int64_t) {
    const int32_t q = where[seq++];
    if (q < 0) return;
    const int32_t t = fill[static_cast<size_t>(q)]++;
    T.tweight[static_cast<size_t>(t)] = w;
    T.tcoef[static_cast<size_t>(t)] = coef;
  });
  T.base.resize(static_cast<size_t>(T.n_weights));
  for (int64_t e = 0; e < ne; ++e) {
    T.base[static_cast<size_t>(e)] = field(d * d + d, e);
    T.base[static_cast<size_t>(ne + e)] = field(d * d + d + 1, e);
  }
  for (int64_t m = 0; m < nr; ++m) T.base[static_cast<size_t>(2 * ne + m)] = range_data[nr + m];
  T.built = true;
  M = std::move(T);
}

void term_map_apply_host(const TermMap &M, const double *w, double *vals) {
  for (int64_t q = 0; q < M.nnz; ++q) {
    const int32_t t0 = M.tptr[static_cast<size_t>(q)], t1 = M.tptr[static_cast<size_t>(q) + 1];
    if (t1 - t0 <= kLongEntry) {
      double acc = 0.0;
      for (int32_t t = t0; t < t1; ++t) acc = std::fma(M.tcoef[static_cast<size_t>(t)], w[M.tweight[static_cast<size_t>(t)]], acc);
      vals[q] = acc;
      continue;
    }
    double lane[kWave];
    for (int l = 0; l < kWave; ++l) {
      double acc = 0.0;
      for (int32_t t = t0 + l; t < t1; t += kWave) acc = std::fma(M.tcoef[static_cast<size_t>(t)], w[M.tweight[static_cast<size_t>(t)]], acc);
      lane[l] = acc;
    }
    for (int off = kWave / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; ++l) lane[l] = lane[l] + lane[l + off];
    vals[q] = lane[0];
  }
}

}  // namespace cora
