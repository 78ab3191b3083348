// Part of kernels.hip (included there, in this order, inside namespace cora).  chain placement from inter-robot ranges: per stage the pass over the chunks of the stage's entry list and the fold with the small dense solve, for the linear stage and for a Gauss-Newton evaluation, then the rigid motion of the chain's positions (PlArgs, kernels.h) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// chain placement
// ---------------------------------------------------------------------------
// The terms and everything the folds compute are functions of kernels.h the host mirror calls; the sums are taken in the
// order kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the launches are the only
// synchronisation between workgroups.

// The linear stage has kPlSums(D) sums per chunk (153 at D = 3), more than a thread holds as accumulators: every entry's
// kPlTerms(D) terms and its weight are staged in LDS ((17 + 1) x 256 doubles = 36 KB at D = 3; the row stride of 17
// doubles is odd, so the staging stores meet no bank twice) and thread p sums the pair product p over the chunk.  All
// threads of that loop read the same entry at a time: two LDS addresses per wavefront and iteration.
template <int D>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_linear(const PlArgs A) {
  constexpr int NT = kPlTerms(D), NP = kPlSums(D);
  static_assert(NP <= kPlChunk, "one thread per pair product");
  __shared__ double term[kPlChunk * NT];
  __shared__ double wt[kPlChunk];
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int len = A.chunk_len[chunk], tid = threadIdx.x;
  if (tid < len) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + tid;
    const int32_t m = A.ent_m[e];
    double c[NT];
    pl_linear_terms<D>(A.x + static_cast<size_t>(A.origin_q) * D, A.x + static_cast<size_t>(A.origin_a) * D,
                       A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D, A.range_data[m], c);
#pragma unroll
    for (int i = 0; i < NT; ++i) term[tid * NT + i] = c[i];
    wt[tid] = A.range_data[A.n_ranges + m];
  }
  __syncthreads();
  if (tid < NP) {
    int i, j;
    pl_pair(NT, tid, &i, &j);
    A.partial[static_cast<size_t>(tid) * A.pstride + blockIdx.x] = pl_pair_sum(term, wt, len, NT, i, j);
  }
}

// B of a stage's sums at a time, from sum p0 (list_sums over the stage's chunks); lane 0 leaves them in S.  (B sums share a
// loop only to have their loads and exchanges in flight together: each sum's additions are its own, in the order kernels.h
// writes down.)
template <int B>
__device__ __forceinline__ void pl_fold_sums(const PlArgs &A, int p0, double *S) {
  double v[B];
  list_sums<B>(v, A.partial + static_cast<size_t>(p0) * A.pstride, A.pstride, 0, A.n_chunks);  // (n_chunks: an int)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < B; ++k) S[p0 + k] = v[k];
  }
}

// ONE wavefront: the stage's sums, nine at a time, into LDS, then lane 0 solves there (the 16 x 16 normal matrix
// and its factor never live in registers)
template <int D>
__global__ __launch_bounds__(kWave) void k_pl_fold_linear(const PlArgs A) {
  constexpr int NP = kPlSums(D), N = kPlUnknowns(D);
  __shared__ double S[NP];
  __shared__ double work[N * (N + 1)];
  static_assert(NP % 9 == 0, "36 and 153 sums");
  for (int p0 = 0; p0 < NP; p0 += 9) pl_fold_sums<9>(A, p0, S);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!pl_fold_linear<D>(S, work, A.state, A.istate, A.x + static_cast<size_t>(A.origin_q) * D, A.x + static_cast<size_t>(A.origin_a) * D))
    atomicOr(A.flag, 1);
}

// one thread per entry of a chunk, the entry's kPlGnSums(D) terms in registers (28 at D = 3)
template <int D>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_gn(const PlArgs A) {
  constexpr int NS = kPlGnSums(D), G = kPlG(D);
  __shared__ double sm[kPlChunk / kWave][NS];
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    const int32_t m = A.ent_m[e];
    const double *gp = A.state + (A.step == 0 ? G : 0);  // evaluation 0 is at the identity, which the linear fold left in `best`
    double g[G];
#pragma unroll
    for (int i = 0; i < G; ++i) g[i] = gp[i];
    pl_gn_terms<D>(g, A.state[3 * G + 4], A.x + static_cast<size_t>(A.origin_q) * D, A.x + static_cast<size_t>(A.origin_a) * D,
                   A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D, A.range_data[m],
                   A.range_data[A.n_ranges + m], s);
  }
  chunk_sums<NS>(s, sm, A.partial, A.pstride, blockIdx.x);
}

template <int D>
__global__ __launch_bounds__(kWave) void k_pl_fold_gn(const PlArgs A) {
  constexpr int NS = kPlGnSums(D);
  __shared__ double S[NS];
  pl_fold_sums<NS>(A, 0, S);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!pl_fold_gn<D>(A.step, A.last, S, A.state, A.istate, A.x + static_cast<size_t>(A.origin_q) * D, A.x + static_cast<size_t>(A.origin_a) * D))
    atomicOr(A.flag, 1);
}

// the chain's positions under the written transform; a stage whose least cost is at the identity writes nothing
template <int D>
__global__ __launch_bounds__(256) void k_pl_apply(const PlArgs A) {
  constexpr int G = kPlG(D);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= A.n_pos || A.istate[1] <= 0) return;
  double g[G];
#pragma unroll
  for (int k = 0; k < G; ++k) g[k] = A.state[2 * G + k];
  const int64_t pos = static_cast<int64_t>(A.pos0) + i;
  pl_apply<D>(g, A.x + static_cast<size_t>(A.pos_rot[pos]) * D, A.x + static_cast<size_t>(A.pos_trn[pos]) * D);
}
#endif  // CORA_TU & 2
