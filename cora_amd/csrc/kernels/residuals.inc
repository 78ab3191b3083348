// Part of kernels.hip (included there, in this order, inside namespace cora).  per-measurement residuals: one gather pass over the measurement table (ResidualArgs, kernels.h).
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// per-measurement residuals
// ---------------------------------------------------------------------------
// A measurement belongs to a fixed group of kResidualLanes = 8 lanes that stride over the columns of X: a wave-instruction
// then reads 8 rows in pieces of 8 x 16 contiguous bytes (even row stride) or 8 x 8 bytes (odd), not 64 rows one double
// each.  The record of a measurement is read by all lanes of its group at the same address (one request per group; the
// groups of a wave read consecutive entries of a field).  The group's partial sums are added with a butterfly over the
// lane distances 4, 2, 1 -- one order whatever the group's place in the wave, the block or the table, so a measurement's
// value depends on its record and its rows of X alone.  Totals: one slot per block and output, no atomics.

// W columns of one row from column c0 on: W = 2 one 16-byte load (even row stride, c0 even), W = 1 one 8-byte load.
// Columns from k on are not data (the padding column of k = 1).
template <int W>
__device__ __forceinline__ void res_load(const double *__restrict__ X, int32_t row, int ld, int c0, int k, double (&v)[W]) {
  const double *p = X + static_cast<size_t>(row) * ld + c0;
  if constexpr (W == 2) {
    const double2 t = *reinterpret_cast<const double2 *>(p);
    v[0] = t.x;
    v[1] = c0 + 1 < k ? t.y : 0.0;
  } else {
    v[0] = *p;
  }
}

__device__ __forceinline__ double group_sum_8(double v) {
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

// What lane g of its group adds to the two sums of edge e (before the precisions):  rot += |X_b - R^T X_a|^2,
// trn += |x_t(b) - x_t(a) - sum_c t_c X_a[c, :]|^2 over the lane's pieces of the columns.  Shared with the robust-cost
// weight step (kernels/gnc.inc), whose residuals are these bits.
template <int D, int W>
__device__ __forceinline__ void edge_lane_sums(const ResidualArgs &A, int64_t n, int64_t e, int g, int pieces, bool &has_rot,
                                               double &rot, double &trn) {
  const int32_t ra = A.rows[e], rb = A.rows[n + e], ta = A.rows[2 * n + e], tb = A.rows[3 * n + e];
  has_rot = rb >= 0;
  double R[D][D] = {}, t[D];
#pragma unroll
  for (int c = 0; c < D; ++c) t[c] = A.data[static_cast<size_t>(D * D + c) * n + e];
  if (has_rot) {
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) R[a][b] = A.data[static_cast<size_t>(a * D + b) * n + e];
  }
  for (int v = g; v < pieces; v += kResidualLanes) {
    const int c0 = v * W;
    double xa[D][W], xta[W], xtb[W];
#pragma unroll
    for (int c = 0; c < D; ++c) res_load<W>(A.X, ra + c, A.ld, c0, A.k, xa[c]);
    res_load<W>(A.X, ta, A.ld, c0, A.k, xta);
    res_load<W>(A.X, tb, A.ld, c0, A.k, xtb);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      double diff = xtb[j] - xta[j];
#pragma unroll
      for (int c = 0; c < D; ++c) diff = fma(-t[c], xa[c][j], diff);
      trn = fma(diff, diff, trn);
    }
    if (has_rot) {
#pragma unroll
      for (int b = 0; b < D; ++b) {  // row b of X_b - R^T X_a
        double xb[W];
        res_load<W>(A.X, rb + b, A.ld, c0, A.k, xb);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          double diff = xb[j];
#pragma unroll
          for (int a = 0; a < D; ++a) diff = fma(-R[a][b], xa[a][j], diff);
          rot = fma(diff, diff, rot);
        }
      }
    }
  }
}

// the same for range m:  res += |x_t(b) - x_t(a) + r x_rho|^2
template <int W>
__device__ __forceinline__ void range_lane_sum(const ResidualArgs &A, int64_t n, int64_t m, int g, int pieces, double &res) {
  const int32_t rr = A.rows[m], ta = A.rows[n + m], tb = A.rows[2 * n + m];
  const double r = A.data[m];
  for (int v = g; v < pieces; v += kResidualLanes) {
    const int c0 = v * W;
    double xr[W], xta[W], xtb[W];
    res_load<W>(A.X, rr, A.ld, c0, A.k, xr);
    res_load<W>(A.X, ta, A.ld, c0, A.k, xta);
    res_load<W>(A.X, tb, A.ld, c0, A.k, xtb);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double diff = fma(r, xr[j], xtb[j] - xta[j]);
      res = fma(diff, diff, res);
    }
  }
}

// rot = kappa |X_b - R^T X_a|_F^2,  trans = tau |x_t(b) - x_t(a) - sum_c t_c X_a[c, :]|^2
template <int D, int W>
__global__ __launch_bounds__(256) void k_edge_residuals(ResidualArgs A) {
  __shared__ double sm[4];
  constexpr int G = kResidualLanes, PER_BLOCK = 256 / G;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int pieces = (A.k + W - 1) / W;
  const int64_t n = A.n;
  double sum_rot = 0.0, sum_trn = 0.0;
  // (the trip count is the same for every lane of the block: the shuffles below are executed by all of them)
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * PER_BLOCK; base < n; base += static_cast<int64_t>(gridDim.x) * PER_BLOCK) {
    const int64_t e = base + grp;
    const bool live = e < n;
    double rot = 0.0, trn = 0.0, kappa = 0.0, tau = 0.0;
    bool has_rot = false;
    if (live) {
      kappa = A.data[static_cast<size_t>(D * D + D) * n + e];
      tau = A.data[static_cast<size_t>(D * D + D + 1) * n + e];
      edge_lane_sums<D, W>(A, n, e, g, pieces, has_rot, rot, trn);
    }
    rot = group_sum_8(rot);
    trn = group_sum_8(trn);
    if (live && g == 0) {
      rot = has_rot ? kappa * rot : 0.0;
      trn = tau * trn;
      A.out0[e] = rot;
      A.out1[e] = trn;
      sum_rot += rot;
      sum_trn += trn;
    }
  }
  const double s0 = block_sum_256(sum_rot, sm);
  const double s1 = block_sum_256(sum_trn, sm);
  if (threadIdx.x == 0) {
    A.partial[blockIdx.x] = s0;
    A.partial[gridDim.x + blockIdx.x] = s1;
  }
}

// res = omega |x_t(b) - x_t(a) + r x_rho|^2
template <int W>
__global__ __launch_bounds__(256) void k_range_residuals(ResidualArgs A) {
  __shared__ double sm[4];
  constexpr int G = kResidualLanes, PER_BLOCK = 256 / G;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int pieces = (A.k + W - 1) / W;
  const int64_t n = A.n;
  double sum = 0.0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * PER_BLOCK; base < n; base += static_cast<int64_t>(gridDim.x) * PER_BLOCK) {
    const int64_t e = base + grp;
    const bool live = e < n;
    double res = 0.0, omega = 0.0;
    if (live) {
      omega = A.data[n + e];
      range_lane_sum<W>(A, n, e, g, pieces, res);
    }
    res = group_sum_8(res);
    if (live && g == 0) {
      res = omega * res;
      A.out0[e] = res;
      sum += res;
    }
  }
  const double s = block_sum_256(sum, sm);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = s;
}
#endif  // CORA_TU & 2
