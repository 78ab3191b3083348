// Part of kernels.hip (included there, in this order, inside namespace cora).  the weight step of a robust-cost (GNC) loop: unweighted residuals, ratios to the thresholds, weights and their statistics in one pass over the measurement table (GncArgs, kernels.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// GNC weight step
// ---------------------------------------------------------------------------
// The pass has the shape of the residual kernels (residuals.inc) and shares their per-lane bodies, so r^2 of a measurement
// has the bits k_edge_residuals / k_range_residuals give on a table that holds the base precisions.  The precisions come
// from the term map's base array ([kappa | tau] of the edges, omega of the ranges), never from the table, whose kappa, tau
// and omega are base * w after a re-weighting.  Lane 0 of a group forms r^2, rho and w (gnc_ratio / gnc_weight, kernels.h:
// the host mirror runs the same functions), stores them and keeps the block's share of the statistics; a block leaves its
// shares in fixed slots (launch_reduce_partials adds the sums, k_reduce_max_partials takes the maxima): no atomics, the
// same bits on every call.  Bad inputs are OR-ed into *flag by the one lane that saw them (bit 1: r^2 not finite, bit 2:
// threshold NaN or <= 0); the flag is only ever raised, so the order of the writes does not matter.

// Largest value over a 256-thread block of non-negative numbers; valid in thread 0.  `sm` holds >= 4 doubles.  (fmax
// drops a NaN operand: a NaN ratio has raised the flag already.)
__device__ __forceinline__ double block_max_256(double v, double *sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  return fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

// one segment's statistics of a lane
struct GncAcc {
  double wr2 = 0.0, mid = 0.0, out = 0.0, rho = 0.0;
  __device__ __forceinline__ void add_sum(double w, double r2) {
#pragma clang fp contract(off)
    const double t = w * r2;
    wr2 += t;
  }
  __device__ __forceinline__ void count(double w, double ratio) {
    if (w > 0.0 && w < 1.0) mid += 1.0;
    if (w < 0.5) out += 1.0;
    rho = fmax(rho, ratio);
  }
};

// rows [3 * seg .. 3 * seg + 2] of the sums and row n_seg * 3 + seg (the maxima) of partial[.][gridDim.x]
__device__ __forceinline__ void gnc_block_store(const GncAcc &a, int seg, int n_seg, double *partial, double *sm) {
  const double s0 = block_sum_256(a.wr2, sm);
  const double s1 = block_sum_256(a.mid, sm);
  const double s2 = block_sum_256(a.out, sm);
  const double mx = block_max_256(a.rho, sm);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    partial[(3 * seg + 0) * nb + blockIdx.x] = s0;
    partial[(3 * seg + 1) * nb + blockIdx.x] = s1;
    partial[(3 * seg + 2) * nb + blockIdx.x] = s2;
    partial[(3 * n_seg + seg) * nb + blockIdx.x] = mx;
  }
}

template <int D, int W>
__global__ __launch_bounds__(256) void k_gnc_edges(GncArgs A) {
  __shared__ double sm[4];
  constexpr int G = kResidualLanes, PER_BLOCK = 256 / G;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int pieces = (A.R.k + W - 1) / W;
  const int64_t n = A.R.n;
  GncAcc acc_rot, acc_trn;
  // (the trip count is the same for every lane of the block: the shuffles below are executed by all of them)
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * PER_BLOCK; base < n; base += static_cast<int64_t>(gridDim.x) * PER_BLOCK) {
    const int64_t e = base + grp;
    const bool live = e < n;
    double rot = 0.0, trn = 0.0;
    bool has_rot = false;
    if (live) edge_lane_sums<D, W>(A.R, n, e, g, pieces, has_rot, rot, trn);
    rot = group_sum_8(rot);
    trn = group_sum_8(trn);
    if (live && g == 0) {
      rot = has_rot ? A.base[e] * rot : 0.0;
      trn = A.base[n + e] * trn;
      int bad = 0;
      double w_rot, w_trn;
      if (A.couple) {
        const double ratio = gnc_ratio(gnc_coupled_r2(rot, trn), A.barc2[n + e], bad);
        w_rot = w_trn = gnc_weight(A.cost, A.mu, ratio);
        acc_trn.count(w_trn, ratio);
      } else {
        const double ratio_rot = gnc_ratio(rot, A.barc2[e], bad), ratio_trn = gnc_ratio(trn, A.barc2[n + e], bad);
        w_rot = gnc_weight(A.cost, A.mu, ratio_rot);
        w_trn = gnc_weight(A.cost, A.mu, ratio_trn);
        acc_rot.count(w_rot, ratio_rot);
        acc_trn.count(w_trn, ratio_trn);
      }
      acc_rot.add_sum(w_rot, rot);
      acc_trn.add_sum(w_trn, trn);
      A.w[e] = w_rot;
      A.w[n + e] = w_trn;
      if (A.r2) {
        A.r2[e] = rot;
        A.r2[n + e] = trn;
      }
      if (bad) atomicOr(A.flag, bad);
    }
  }
  gnc_block_store(acc_rot, 0, 2, A.partial, sm);
  gnc_block_store(acc_trn, 1, 2, A.partial, sm);
}

template <int W>
__global__ __launch_bounds__(256) void k_gnc_ranges(GncArgs A) {
  __shared__ double sm[4];
  constexpr int G = kResidualLanes, PER_BLOCK = 256 / G;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int pieces = (A.R.k + W - 1) / W;
  const int64_t n = A.R.n;
  GncAcc acc;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * PER_BLOCK; base < n; base += static_cast<int64_t>(gridDim.x) * PER_BLOCK) {
    const int64_t m = base + grp;
    const bool live = m < n;
    double res = 0.0;
    if (live) range_lane_sum<W>(A.R, n, m, g, pieces, res);
    res = group_sum_8(res);
    if (live && g == 0) {
      res = A.base[m] * res;
      int bad = 0;
      const double ratio = gnc_ratio(res, A.barc2[m], bad);
      const double w = gnc_weight(A.cost, A.mu, ratio);
      acc.count(w, ratio);
      acc.add_sum(w, res);
      A.w[m] = w;
      if (A.r2) A.r2[m] = res;
      if (bad) atomicOr(A.flag, bad);
    }
  }
  gnc_block_store(acc, 0, 1, A.partial, sm);
}

// out[j] = max_b partial[j * nblocks + b]   (one 256-thread block; the partials are >= 0)
__global__ __launch_bounds__(256) void k_reduce_max_partials(const double *__restrict__ partial, int nblocks, int count,
                                                             double *__restrict__ out) {
  __shared__ double sm[4];
  for (int j = 0; j < count; ++j) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s = fmax(s, partial[static_cast<size_t>(j) * nblocks + b]);
    const double t = block_max_256(s, sm);
    if (threadIdx.x == 0) out[j] = t;
  }
}
#endif  // CORA_TU & 2
