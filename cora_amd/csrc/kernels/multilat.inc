// Part of kernels.hip (included there, in this order, inside namespace cora).  landmark initialisation from ranges: per stage one pass over the chunks of the landmarks' range lists and one fold per landmark with the small dense solve (MlArgs, kernels.h); the outlier-robust form: the consensus vote over minimal samples of d + 1 ranges (one workgroup per chunk, the list's entries through an LDS tile), the election, and the same passes over the inliers (MlRobustArgs) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// multilateration
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's NS terms in registers (14 doubles at D = 3 in the linear stage, 10 in a
// Gauss-Newton stage).  The terms and everything the fold computes are functions of kernels.h the host mirror calls; the
// sums are taken in the order kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the
// launches are the only synchronisation between workgroups.

// the kernels' argument of the plain (MlArgs) and of the robust form (MlRobustArgs), and the plain part of either
template <bool ROBUST>
using MlKernelArgs = std::conditional_t<ROBUST, MlRobustArgs, MlArgs>;
__host__ __device__ inline const MlArgs &ml_plain(const MlArgs &A) { return A; }
__host__ __device__ inline const MlArgs &ml_plain(const MlRobustArgs &R) { return R.A; }

// ROBUST: over the inliers of the elected hypothesis (k_ml_vote, k_ml_elect below): each entry re-evaluates r(h*, j) <= barc2
// from cstate (the vote's function, the vote's bits); an entry outside I leaves its terms at +0.0.  The linear pass also
// writes the range's inlier byte, then leaves a list of status 5 alone.  The plain form loads none of that.
template <int D, int NS, bool LINEAR, bool ROBUST>
__device__ __forceinline__ void ml_pass(const MlKernelArgs<ROBUST> &K, double (*sm)[NS]) {
  const MlArgs &A = ml_plain(K);
  const int64_t chunk = blockIdx.x;
  const int32_t l = A.chunk_lm[chunk];
  if ((LINEAR ? static_cast<int>(A.lm_init[l]) : A.istate[static_cast<size_t>(l) * kMlInts]) != 0) return;  // (the whole workgroup)
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    const int32_t m = A.ent_m[e];
    const double *t0 = A.x + static_cast<size_t>(A.lm_origin[l]) * D, *ti = A.x + static_cast<size_t>(A.ent_row[e]) * D;
    const double r = A.range_data[m], w = A.range_data[A.n_ranges + m];
    bool in = true;
    if constexpr (ROBUST) {
      double yc[D], u[D];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        yc[c] = K.cstate[static_cast<size_t>(l) * kMlCState(D) + c];
        u[c] = ti[c] - t0[c];
      }
      in = K.cint[static_cast<size_t>(l) * kMlCInts + 1] > 0 && cl_agrees(ml_cost_at<D>(yc, u, r, w), K.barc2);
      if constexpr (LINEAR) K.inlier[m] = in ? 1 : 0;
    }
    if (LINEAR) {
      if (in) ml_linear_terms<D>(t0, ti, r, w, s);
    } else if (in) {
      double y[D];
#pragma unroll
      for (int c = 0; c < D; ++c) y[c] = A.state[static_cast<size_t>(l) * kMlState(D) + c];
      ml_gn_terms<D>(y, t0, ti, r, w, s);
    }
  }
  if constexpr (ROBUST && LINEAR) {
    if (A.istate[static_cast<size_t>(l) * kMlInts] == 5) return;  // (the whole workgroup; the fold reads no sum of this list)
  }
  chunk_sums<NS>(s, sm, A.partial, A.n_chunks, chunk);
}

template <int D, bool ROBUST = false>
__global__ __launch_bounds__(kMlChunk) void k_ml_pass_linear(const MlKernelArgs<ROBUST> K) {
  __shared__ double sm[kMlChunk / kWave][kMlSums(D)];
  ml_pass<D, kMlSums(D), true, ROBUST>(K, sm);
}
template <int D, bool ROBUST = false>
__global__ __launch_bounds__(kMlChunk) void k_ml_pass_gn(const MlKernelArgs<ROBUST> K) {
  __shared__ double sm[kMlChunk / kWave][kMlGnSums(D)];
  ml_pass<D, kMlGnSums(D), false, ROBUST>(K, sm);
}

// one wavefront per landmark: the sums of its chunks, ml_fold, and after the last stage the landmark's row.  ROBUST (the
// linear fold alone): a list k_ml_elect left at status 5 enters ml_fold with init 5, as a list that is not to be solved
template <int D, int NS, bool LINEAR, bool ROBUST = false>
__device__ __forceinline__ void ml_fold_lm(const MlArgs &A) {
  static_assert(LINEAR || !ROBUST, "the Gauss-Newton fold has one form");
  const int64_t l = blockIdx.x;
  const int lane = threadIdx.x;
  int32_t *ist = A.istate + static_cast<size_t>(l) * kMlInts;
  const int init = ROBUST && A.lm_init[l] == 0 && ist[0] == 5 ? 5 : static_cast<int>(A.lm_init[l]);
  double *st = A.state + static_cast<size_t>(l) * kMlState(D);
  if (LINEAR ? init != 0 : ist[0] != 0) {
    if (LINEAR && lane == 0) {
      const double none[NS] = {};
      ml_fold<D>(0, 0, none, st, ist, init);  // (reads no sum)
    }
    return;
  }
  double s[NS];
  list_sums<NS, int64_t>(s, A.partial, A.n_chunks, A.lm_chunk0[l], A.lm_chunk0[l + 1]);
  if (lane != 0) return;
  double lst[kMlState(D)];
  int32_t li[kMlInts];
#pragma unroll
  for (int i = 0; i < kMlState(D); ++i) lst[i] = st[i];
#pragma unroll
  for (int i = 0; i < kMlInts; ++i) li[i] = ist[i];
  if (!ml_fold<D>(A.stage, A.last, s, lst, li, init)) atomicOr(A.flag, 1);
#pragma unroll
  for (int i = 0; i < kMlState(D); ++i) st[i] = lst[i];
#pragma unroll
  for (int i = 0; i < kMlInts; ++i) ist[i] = li[i];
  if (A.last && li[0] == 0) {
    const double *t0 = A.x + static_cast<size_t>(A.lm_origin[l]) * D;
    double *row = A.x + static_cast<size_t>(A.lm_row[l]) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) row[c] = t0[c] + lst[D + c];
  }
}

template <int D, bool ROBUST = false>
__global__ __launch_bounds__(kWave) void k_ml_fold_linear(const MlArgs A) {
  ml_fold_lm<D, kMlSums(D), true, ROBUST>(A);
}
template <int D>
__global__ __launch_bounds__(kWave) void k_ml_fold_gn(const MlArgs A) {
  ml_fold_lm<D, kMlGnSums(D), false>(A);
}

// ---------------------------------------------------------------------------
// the consensus vote (MlRobustArgs, kernels.h)
// ---------------------------------------------------------------------------
// One workgroup per chunk of ALL lists; thread t owns the hypothesis of entry chunk_begin + t: it gathers its D + 1 sample
// entries from global memory (scattered, once) and keeps y_h and its validity in registers.  The workgroup then walks ALL
// chunks of its list: each step stages one chunk's u_j, r_j, omega_j in LDS (structure of arrays, D + 2 doubles per entry:
// 10 KB at D = 3, 8 KB at D = 2), and every thread scores its hypothesis against the tile.  In the inner loop all lanes read
// one LDS address: a broadcast, no bank conflict.  The vote is an integer: no order to keep.  Threads beyond chunk_len stage
// and own no hypothesis.  L^2 scores per list.
template <int D>
__global__ __launch_bounds__(kMlChunk) void k_ml_vote(const MlRobustArgs R) {
  __shared__ double tile[D + 2][kMlChunk];
  const MlArgs &A = R.A;
  const int64_t chunk = blockIdx.x;
  const int32_t l = A.chunk_lm[chunk];
  if (A.lm_init[l] != 0) return;  // (the whole workgroup)
  const int t = threadIdx.x;
  const bool own = t < A.chunk_len[chunk];
  const int32_t c0 = A.lm_chunk0[l], c1 = A.lm_chunk0[l + 1];
  const int32_t begin = A.chunk_begin[c0], len = A.chunk_begin[c1 - 1] + A.chunk_len[c1 - 1] - begin;
  double t0[D], y[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    t0[c] = A.x[static_cast<size_t>(A.lm_origin[l]) * D + c];
    y[c] = 0.0;
  }
  bool valid = false;
  if (own) {
    const int32_t h = A.chunk_begin[chunk] + t - begin;
    double ts[(D + 1) * D], rs[D + 1], ws[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) {
      const int64_t e = static_cast<int64_t>(begin) + ml_sample<D>(h, k, len);
      const int32_t m = A.ent_m[e];
      const double *ti = A.x + static_cast<size_t>(A.ent_row[e]) * D;
#pragma unroll
      for (int c = 0; c < D; ++c) ts[k * D + c] = ti[c];
      rs[k] = A.range_data[m];
      ws[k] = A.range_data[A.n_ranges + m];
    }
    valid = ml_hypothesis<D>(t0, ts, rs, ws, y);
  }
  int32_t vote = 0;
  for (int32_t c = c0; c < c1; ++c) {
    const int clen = A.chunk_len[c];
    __syncthreads();  // (the tile of the step before is read no more)
    if (t < clen) {
      const int64_t e = static_cast<int64_t>(A.chunk_begin[c]) + t;
      const int32_t m = A.ent_m[e];
      const double *ti = A.x + static_cast<size_t>(A.ent_row[e]) * D;
#pragma unroll
      for (int i = 0; i < D; ++i) tile[i][t] = ti[i] - t0[i];
      tile[D][t] = A.range_data[m];
      tile[D + 1][t] = A.range_data[A.n_ranges + m];
    }
    __syncthreads();
    if (own && valid) {
      for (int j = 0; j < clen; ++j) {
        double u[D];
#pragma unroll
        for (int i = 0; i < D; ++i) u[i] = tile[i][j];
        vote += cl_agrees(ml_cost_at<D>(y, u, tile[D][j], tile[D + 1][j]), R.barc2) ? 1 : 0;
      }
    }
  }
  if (own) R.votes[static_cast<int64_t>(A.chunk_begin[chunk]) + t] = vote;
}

// one wavefront per list: the entry of largest vote, the lowest entry among equal votes; lane 0 recomputes its hypothesis
// and sets status 5 where the consensus is below min_consensus (0 otherwise: the linear fold's solve overwrites it)
template <int D>
__global__ __launch_bounds__(kWave) void k_ml_elect(const MlRobustArgs R) {
  const MlArgs &A = R.A;
  const int64_t l = blockIdx.x;
  if (A.lm_init[l] != 0) return;
  const int lane = threadIdx.x;
  const int32_t c0 = A.lm_chunk0[l], c1 = A.lm_chunk0[l + 1];
  const int32_t begin = A.chunk_begin[c0], len = A.chunk_begin[c1 - 1] + A.chunk_len[c1 - 1] - begin;
  int32_t bv = -1, be = len;  // (every entry beats this)
  for (int32_t e = lane; e < len; e += kWave) {
    const int32_t v = R.votes[static_cast<int64_t>(begin) + e];
    if (cl_better(v, e, bv, be)) {
      bv = v;
      be = e;
    }
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int32_t v = __shfl_xor(bv, off, kWave), e = __shfl_xor(be, off, kWave);
    if (cl_better(v, e, bv, be)) {
      bv = v;
      be = e;
    }
  }
  if (lane != 0) return;
  double ts[(D + 1) * D], rs[D + 1], ws[D + 1], y[D];
#pragma unroll
  for (int k = 0; k <= D; ++k) {
    const int64_t e = static_cast<int64_t>(begin) + ml_sample<D>(be, k, len);
    const int32_t m = A.ent_m[e];
#pragma unroll
    for (int c = 0; c < D; ++c) ts[k * D + c] = A.x[static_cast<size_t>(A.ent_row[e]) * D + c];
    rs[k] = A.range_data[m];
    ws[k] = A.range_data[A.n_ranges + m];
  }
  ml_hypothesis<D>(A.x + static_cast<size_t>(A.lm_origin[l]) * D, ts, rs, ws, y);
#pragma unroll
  for (int c = 0; c < D; ++c) R.cstate[static_cast<size_t>(l) * kMlCState(D) + c] = y[c];
  R.cint[static_cast<size_t>(l) * kMlCInts] = be;
  R.cint[static_cast<size_t>(l) * kMlCInts + 1] = bv;
  A.istate[static_cast<size_t>(l) * kMlInts] = bv < R.min_consensus ? 5 : 0;
  if (!odom_finite(y, D)) atomicOr(A.flag, 1);
}
#endif  // CORA_TU & 2
