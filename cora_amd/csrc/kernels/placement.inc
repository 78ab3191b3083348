// Part of kernels.hip (included there, in this order, inside namespace cora).  chain placement from inter-robot ranges: per stage the pass over the chunks of the stage's entry list and the fold with the small dense solve, for the linear stage and for a Gauss-Newton evaluation, then the rigid motion of the chain's positions (PlArgs, kernels.h), for one stage (CORA_TU & 2) or, BATCHED (PlBatchArgs), for all stages of a level (CORA_TU & 8)
#if CORA_TU & (2 | 8)
// ---------------------------------------------------------------------------
// chain placement
// ---------------------------------------------------------------------------
// The terms and everything the folds compute are functions of kernels.h the host mirror calls; the sums are taken in the
// order kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the launches are the only
// synchronisation between workgroups.
//
// BATCHED (PlBatchArgs, kernels.h): the same bodies over ALL stages of one level -- independent of each other, since a stage's
// anchors lie in chains of earlier levels -- in one launch: a pass workgroup finds its chunk's stage in chunk_stage, a fold
// wavefront serves stage stage0 + blockIdx.x, an apply workgroup one tile of tile_stage / tile_off; origins, state and istate
// come from the per-stage arrays.  A chunk's partial sums stand at its index within the level, so a stage's chunks are
// consecutive there and the fold's bracket order is the plain one.
template <bool BATCHED>
using PlKernelArgs = std::conditional_t<BATCHED, PlBatchArgs, PlArgs>;
__host__ __device__ inline const PlArgs &pl_plain(const PlArgs &A) { return A; }
__host__ __device__ inline const PlArgs &pl_plain(const PlBatchArgs &B) { return B.A; }

// what a workgroup needs of the stage it serves
struct PlStageRef {
  const double *q0, *a0;  // rows of the first entry's position and anchor
  double *state;
  int32_t *istate;
};
template <int D>
__device__ __forceinline__ PlStageRef pl_stage_ref(const PlArgs &A, int32_t) {
  return {A.x + static_cast<size_t>(A.origin_q) * D, A.x + static_cast<size_t>(A.origin_a) * D, A.state, A.istate};
}
template <int D>
__device__ __forceinline__ PlStageRef pl_stage_ref(const PlBatchArgs &B, int32_t stage) {
  return {B.A.x + static_cast<size_t>(B.stage_origin_q[stage]) * D, B.A.x + static_cast<size_t>(B.stage_origin_a[stage]) * D,
          B.A.state + static_cast<size_t>(stage) * kPlState(D), B.A.istate + static_cast<size_t>(stage) * kPlInts};
}
// the stage of pass workgroup blockIdx.x (chunk A.chunk0 + blockIdx.x), of fold wavefront blockIdx.x
__device__ __forceinline__ int32_t pl_chunk_stage(const PlArgs &, int64_t) { return 0; }
__device__ __forceinline__ int32_t pl_chunk_stage(const PlBatchArgs &B, int64_t chunk) { return B.chunk_stage[chunk]; }
__device__ __forceinline__ int32_t pl_fold_stage(const PlArgs &) { return 0; }
__device__ __forceinline__ int32_t pl_fold_stage(const PlBatchArgs &B) { return B.stage0 + static_cast<int32_t>(blockIdx.x); }
// the stage's chunks [c0, c1) in the level's partial sums
__device__ __forceinline__ void pl_fold_chunks(const PlArgs &A, int32_t, int *c0, int *c1) {
  *c0 = 0;
  *c1 = A.n_chunks;
}
__device__ __forceinline__ void pl_fold_chunks(const PlBatchArgs &B, int32_t stage, int *c0, int *c1) {
  *c0 = B.stage_chunk0[stage] - B.A.chunk0;
  *c1 = B.stage_chunk0[stage + 1] - B.A.chunk0;
}

// The linear stage has kPlSums(D) sums per chunk (153 at D = 3), more than a thread holds as accumulators: every entry's
// kPlTerms(D) terms and its weight are staged in LDS ((17 + 1) x 256 doubles = 36 KB at D = 3; the row stride of 17
// doubles is odd, so the staging stores meet no bank twice) and thread p sums the pair product p over the chunk.  All
// threads of that loop read the same entry at a time: two LDS addresses per wavefront and iteration.
template <int D, bool BATCHED = false>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_linear(const PlKernelArgs<BATCHED> K) {
  constexpr int NT = kPlTerms(D), NP = kPlSums(D);
  static_assert(NP <= kPlChunk, "one thread per pair product");
  __shared__ double term[kPlChunk * NT];
  __shared__ double wt[kPlChunk];
  const PlArgs &A = pl_plain(K);
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int len = A.chunk_len[chunk], tid = threadIdx.x;
  if (tid < len) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + tid;
    const int32_t m = A.ent_m[e];
    const PlStageRef T = pl_stage_ref<D>(K, pl_chunk_stage(K, chunk));
    double c[NT];
    pl_linear_terms<D>(T.q0, T.a0, A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D, A.range_data[m], c);
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
__device__ __forceinline__ void pl_fold_sums(const PlArgs &A, int c0, int c1, int p0, double *S) {
  double v[B];
  list_sums<B>(v, A.partial + static_cast<size_t>(p0) * A.pstride, A.pstride, c0, c1);  // (chunks: an int)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < B; ++k) S[p0 + k] = v[k];
  }
}

// ONE wavefront per stage: the stage's sums, nine at a time, into LDS, then lane 0 solves there (the 16 x 16 normal matrix
// and its factor never live in registers)
template <int D, bool BATCHED = false>
__global__ __launch_bounds__(kWave) void k_pl_fold_linear(const PlKernelArgs<BATCHED> K) {
  constexpr int NP = kPlSums(D), N = kPlUnknowns(D);
  __shared__ double S[NP];
  __shared__ double work[N * (N + 1)];
  static_assert(NP % 9 == 0, "36 and 153 sums");
  const PlArgs &A = pl_plain(K);
  const int32_t stage = pl_fold_stage(K);
  int c0, c1;
  pl_fold_chunks(K, stage, &c0, &c1);
  for (int p0 = 0; p0 < NP; p0 += 9) pl_fold_sums<9>(A, c0, c1, p0, S);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const PlStageRef T = pl_stage_ref<D>(K, stage);
  if (!pl_fold_linear<D>(S, work, T.state, T.istate, T.q0, T.a0)) atomicOr(A.flag, 1);
}

// one thread per entry of a chunk, the entry's kPlGnSums(D) terms in registers (28 at D = 3)
template <int D, bool BATCHED = false>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_gn(const PlKernelArgs<BATCHED> K) {
  constexpr int NS = kPlGnSums(D), G = kPlG(D);
  __shared__ double sm[kPlChunk / kWave][NS];
  const PlArgs &A = pl_plain(K);
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    const int32_t m = A.ent_m[e];
    const PlStageRef T = pl_stage_ref<D>(K, pl_chunk_stage(K, chunk));
    const double *gp = T.state + (A.step == 0 ? G : 0);  // evaluation 0 is at the identity, which the linear fold left in `best`
    double g[G];
#pragma unroll
    for (int i = 0; i < G; ++i) g[i] = gp[i];
    pl_gn_terms<D>(g, T.state[3 * G + 4], T.q0, T.a0, A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D,
                   A.range_data[m], A.range_data[A.n_ranges + m], s);
  }
  chunk_sums<NS>(s, sm, A.partial, A.pstride, blockIdx.x);
}

// (BATCHED: a stage that stopped stepping, or was refused, is served like every other -- pl_fold_gn keeps its point)
template <int D, bool BATCHED = false>
__global__ __launch_bounds__(kWave) void k_pl_fold_gn(const PlKernelArgs<BATCHED> K) {
  constexpr int NS = kPlGnSums(D);
  __shared__ double S[NS];
  const PlArgs &A = pl_plain(K);
  const int32_t stage = pl_fold_stage(K);
  int c0, c1;
  pl_fold_chunks(K, stage, &c0, &c1);
  pl_fold_sums<NS>(A, c0, c1, 0, S);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const PlStageRef T = pl_stage_ref<D>(K, stage);
  if (!pl_fold_gn<D>(A.step, A.last, S, T.state, T.istate, T.q0, T.a0)) atomicOr(A.flag, 1);
}

// the chain's positions under the written transform; a stage whose least cost is at the identity writes nothing
// (BATCHED: workgroup blockIdx.x moves tile tile0 + blockIdx.x of the level: 256 positions of ONE chain from tile_off)
template <int D, bool BATCHED = false>
__global__ __launch_bounds__(256) void k_pl_apply(const PlKernelArgs<BATCHED> K) {
  constexpr int G = kPlG(D);
  const PlArgs &A = pl_plain(K);
  int64_t i, pos0, n_pos;
  const double *state = A.state;
  const int32_t *istate = A.istate;
  if constexpr (BATCHED) {
    const int64_t tile = static_cast<int64_t>(K.tile0) + blockIdx.x;
    const int32_t stage = K.tile_stage[tile];
    i = static_cast<int64_t>(K.tile_off[tile]) + threadIdx.x;
    pos0 = K.stage_pos0[stage];
    n_pos = K.stage_npos[stage];
    state += static_cast<size_t>(stage) * kPlState(D);
    istate += static_cast<size_t>(stage) * kPlInts;
  } else {
    i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    pos0 = A.pos0;
    n_pos = A.n_pos;
  }
  if (i >= n_pos || istate[1] <= 0) return;
  double g[G];
#pragma unroll
  for (int k = 0; k < G; ++k) g[k] = state[2 * G + k];
  const int64_t pos = pos0 + i;
  pl_apply<D>(g, A.x + static_cast<size_t>(A.pos_rot[pos]) * D, A.x + static_cast<size_t>(A.pos_trn[pos]) * D);
}
#endif  // CORA_TU & (2 | 8)
