// Part of kernels.hip (included there, in this order, inside namespace cora).  landmark initialisation from ranges: per stage one pass over the chunks of the landmarks' range lists and one fold per landmark with the small dense solve (MlArgs, kernels.h) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// multilateration
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's NS terms in registers (14 doubles at D = 3 in the linear stage, 10 in a
// Gauss-Newton stage).  The terms and everything the fold computes are functions of kernels.h the host mirror calls; the
// sums are taken in the order kernels.h writes down.  No atomics on doubles; the launches are the only synchronisation
// between workgroups.

// the butterfly: afterwards every lane holds the wavefront's sum
template <int NS>
__device__ __forceinline__ void ml_wave_sum(double *s) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + __shfl_xor(s[i], off, kWave);
}

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
  ml_wave_sum<NS>(s);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) sm[w][i] = s[i];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = sm[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < kMlChunk / kWave; ++j) v = v + sm[j][threadIdx.x];
    A.partial[static_cast<size_t>(threadIdx.x) * A.n_chunks + chunk] = v;
  }
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
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  for (int64_t c = static_cast<int64_t>(A.lm_chunk0[l]) + lane; c < A.lm_chunk0[l + 1]; c += kWave)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + A.partial[static_cast<size_t>(i) * A.n_chunks + c];
  ml_wave_sum<NS>(s);
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
