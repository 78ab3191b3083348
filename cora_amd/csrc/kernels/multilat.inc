// Part of kernels.hip (included there, in this order, inside namespace cora).  landmark initialisation from ranges: per stage one pass over the chunks of the landmarks' range lists and one fold per landmark with the small dense solve (MlArgs, kernels.h) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// multilateration
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's NS terms in registers (14 doubles at D = 3 in the linear stage, 10 in a
// Gauss-Newton stage).  The terms and everything the fold computes are functions of kernels.h the host mirror calls; the
// sums are taken in the order kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the
// launches are the only synchronisation between workgroups.

template <int D, int NS, bool LINEAR>
__device__ __forceinline__ void ml_pass(const MlArgs &A, double (*sm)[NS]) {
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
    if (LINEAR) {
      ml_linear_terms<D>(t0, ti, r, w, s);
    } else {
      double y[D];
#pragma unroll
      for (int c = 0; c < D; ++c) y[c] = A.state[static_cast<size_t>(l) * kMlState(D) + c];
      ml_gn_terms<D>(y, t0, ti, r, w, s);
    }
  }
  chunk_sums<NS>(s, sm, A.partial, A.n_chunks, chunk);
}

template <int D>
__global__ __launch_bounds__(kMlChunk) void k_ml_pass_linear(const MlArgs A) {
  __shared__ double sm[kMlChunk / kWave][kMlSums(D)];
  ml_pass<D, kMlSums(D), true>(A, sm);
}
template <int D>
__global__ __launch_bounds__(kMlChunk) void k_ml_pass_gn(const MlArgs A) {
  __shared__ double sm[kMlChunk / kWave][kMlGnSums(D)];
  ml_pass<D, kMlGnSums(D), false>(A, sm);
}

// one wavefront per landmark: the sums of its chunks, ml_fold, and after the last stage the landmark's row
template <int D, int NS, bool LINEAR>
__device__ __forceinline__ void ml_fold_lm(const MlArgs &A) {
  const int64_t l = blockIdx.x;
  const int lane = threadIdx.x;
  const int init = A.lm_init[l];
  int32_t *ist = A.istate + static_cast<size_t>(l) * kMlInts;
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

template <int D>
__global__ __launch_bounds__(kWave) void k_ml_fold_linear(const MlArgs A) {
  ml_fold_lm<D, kMlSums(D), true>(A);
}
template <int D>
__global__ __launch_bounds__(kWave) void k_ml_fold_gn(const MlArgs A) {
  ml_fold_lm<D, kMlGnSums(D), false>(A);
}
#endif  // CORA_TU & 2
