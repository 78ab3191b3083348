// Part of kernels.hip (included there, in this order, inside namespace cora).  chain placement from inter-robot ranges: per stage the pass over the chunks of the stage's entry list and the fold with the small dense solve, for the linear stage and for a Gauss-Newton evaluation, then the rigid motion of the chain's positions (PlArgs, kernels.h), for one stage (CORA_TU & 2) or, BATCHED (PlBatchArgs), for all stages of a level (CORA_TU & 8); the outlier-robust form (PlRobustArgs): the hypotheses, the consensus vote and the election of a level's stages, and the batched bodies over the inliers, MASK (CORA_TU & 16)
#if CORA_TU & (2 | 8 | 16)
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
//
// MASK (PlRobustArgs, kernels.h; always BATCHED): over the inliers of the stage's elected hypothesis (k_pl_hyp, k_pl_vote,
// k_pl_elect below): each entry re-evaluates r(h*, j) <= barc2 from cstate (the vote's function, the vote's bits); an entry
// outside I adds +0.0 for each of its terms.  The linear pass also writes the range's inlier byte.  A stage of status 5 keeps
// the identity in its folds and writes nothing in the apply.  The other forms load none of that.
template <bool BATCHED, bool MASK = false>
using PlKernelArgs = std::conditional_t<MASK, PlRobustArgs, std::conditional_t<BATCHED, PlBatchArgs, PlArgs>>;
__host__ __device__ inline const PlArgs &pl_plain(const PlArgs &A) { return A; }
__host__ __device__ inline const PlArgs &pl_plain(const PlBatchArgs &B) { return B.A; }
__host__ __device__ inline const PlArgs &pl_plain(const PlRobustArgs &R) { return R.B.A; }
__host__ __device__ inline const PlBatchArgs &pl_batch(const PlBatchArgs &B) { return B; }
__host__ __device__ inline const PlBatchArgs &pl_batch(const PlRobustArgs &R) { return R.B; }

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
template <int D>
__device__ __forceinline__ PlStageRef pl_stage_ref(const PlRobustArgs &R, int32_t stage) { return pl_stage_ref<D>(R.B, stage); }
// the stage of pass workgroup blockIdx.x (chunk A.chunk0 + blockIdx.x), of fold wavefront blockIdx.x
__device__ __forceinline__ int32_t pl_chunk_stage(const PlArgs &, int64_t) { return 0; }
__device__ __forceinline__ int32_t pl_chunk_stage(const PlBatchArgs &B, int64_t chunk) { return B.chunk_stage[chunk]; }
__device__ __forceinline__ int32_t pl_chunk_stage(const PlRobustArgs &R, int64_t chunk) { return R.B.chunk_stage[chunk]; }
__device__ __forceinline__ int32_t pl_fold_stage(const PlArgs &) { return 0; }
__device__ __forceinline__ int32_t pl_fold_stage(const PlBatchArgs &B) { return B.stage0 + static_cast<int32_t>(blockIdx.x); }
__device__ __forceinline__ int32_t pl_fold_stage(const PlRobustArgs &R) { return pl_fold_stage(R.B); }
// the stage's chunks [c0, c1) in the level's partial sums
__device__ __forceinline__ void pl_fold_chunks(const PlArgs &A, int32_t, int *c0, int *c1) {
  *c0 = 0;
  *c1 = A.n_chunks;
}
__device__ __forceinline__ void pl_fold_chunks(const PlBatchArgs &B, int32_t stage, int *c0, int *c1) {
  *c0 = B.stage_chunk0[stage] - B.A.chunk0;
  *c1 = B.stage_chunk0[stage + 1] - B.A.chunk0;
}
__device__ __forceinline__ void pl_fold_chunks(const PlRobustArgs &R, int32_t stage, int *c0, int *c1) { pl_fold_chunks(R.B, stage, c0, c1); }
// MASK: whether the entry (rows q, a, range r, precision w) of `stage` is an inlier of the stage's elected hypothesis
template <int D>
__device__ __forceinline__ bool pl_inlier(const PlRobustArgs &R, int32_t stage, const PlStageRef &T, const double *q, const double *a, double r, double w) {
  constexpr int G = kPlCState(D);
  double g[G], qq[D], aa[D];
#pragma unroll
  for (int i = 0; i < G; ++i) g[i] = R.cstate[static_cast<size_t>(stage) * G + i];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    qq[k] = q[k] - T.q0[k];
    aa[k] = a[k] - T.a0[k];
  }
  return R.cint[static_cast<size_t>(stage) * kPlCInts + 1] > 0 && cl_agrees(pl_cost_at<D>(g, qq, aa, r, w), R.barc2);
}

// The linear stage has kPlSums(D) sums per chunk (153 at D = 3), more than a thread holds as accumulators: every entry's
// kPlTerms(D) terms and its weight are staged in LDS ((17 + 1) x 256 doubles = 36 KB at D = 3; the row stride of 17
// doubles is odd, so the staging stores meet no bank twice) and thread p sums the pair product p over the chunk.  All
// threads of that loop read the same entry at a time: two LDS addresses per wavefront and iteration.
template <int D, bool BATCHED = false, bool MASK = false>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_linear(const PlKernelArgs<BATCHED, MASK> K) {
  constexpr int NT = kPlTerms(D), NP = kPlSums(D);
  static_assert(NP <= kPlChunk, "one thread per pair product");
  __shared__ double term[kPlChunk * NT];
  __shared__ double wt[kPlChunk];
  __shared__ unsigned char in[MASK ? kPlChunk : 1];
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
    if constexpr (MASK) {
      in[tid] = pl_inlier<D>(K, pl_chunk_stage(K, chunk), T, A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D, A.range_data[m],
                             A.range_data[A.n_ranges + m]) ? 1 : 0;
      K.inlier[m] = in[tid];
    }
  }
  __syncthreads();
  if (tid < NP) {
    int i, j;
    pl_pair(NT, tid, &i, &j);
    if constexpr (MASK) {
      A.partial[static_cast<size_t>(tid) * A.pstride + blockIdx.x] = pl_pair_sum_masked(term, wt, in, len, NT, i, j);
    } else {
      A.partial[static_cast<size_t>(tid) * A.pstride + blockIdx.x] = pl_pair_sum(term, wt, len, NT, i, j);
    }
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
template <int D, bool BATCHED = false, bool MASK = false>
__global__ __launch_bounds__(kWave) void k_pl_fold_linear(const PlKernelArgs<BATCHED, MASK> K) {
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
  if (!(MASK ? pl_fold_linear_robust<D>(S, work, T.state, T.istate, T.q0, T.a0) : pl_fold_linear<D>(S, work, T.state, T.istate, T.q0, T.a0))) atomicOr(A.flag, 1);
}

// one thread per entry of a chunk, the entry's kPlGnSums(D) terms in registers (28 at D = 3)
template <int D, bool BATCHED = false, bool MASK = false>
__global__ __launch_bounds__(kPlChunk) void k_pl_pass_gn(const PlKernelArgs<BATCHED, MASK> K) {
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
    bool in = true;
    if constexpr (MASK)
      in = pl_inlier<D>(K, pl_chunk_stage(K, chunk), T, A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D, A.range_data[m],
                        A.range_data[A.n_ranges + m]);
    if (in)
      pl_gn_terms<D>(g, T.state[3 * G + 4], T.q0, T.a0, A.x + static_cast<size_t>(A.ent_q[e]) * D, A.x + static_cast<size_t>(A.ent_a[e]) * D,
                     A.range_data[m], A.range_data[A.n_ranges + m], s);
  }
  chunk_sums<NS>(s, sm, A.partial, A.pstride, blockIdx.x);
}

// (BATCHED: a stage that stopped stepping, or was refused, is served like every other -- pl_fold_gn keeps its point)
template <int D, bool BATCHED = false, bool MASK = false>
__global__ __launch_bounds__(kWave) void k_pl_fold_gn(const PlKernelArgs<BATCHED, MASK> K) {
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
  if (!(MASK ? pl_fold_gn_robust<D>(A.step, A.last, S, T.state, T.istate, T.q0, T.a0) : pl_fold_gn<D>(A.step, A.last, S, T.state, T.istate, T.q0, T.a0)))
    atomicOr(A.flag, 1);
}

// the chain's positions under the written transform; a stage whose least cost is at the identity writes nothing
// (BATCHED: workgroup blockIdx.x moves tile tile0 + blockIdx.x of the level: 256 positions of ONE chain from tile_off)
template <int D, bool BATCHED = false, bool MASK = false>
__global__ __launch_bounds__(256) void k_pl_apply(const PlKernelArgs<BATCHED, MASK> K) {
  constexpr int G = kPlG(D);
  const PlArgs &A = pl_plain(K);
  int64_t i, pos0, n_pos;
  const double *state = A.state;
  const int32_t *istate = A.istate;
  if constexpr (BATCHED) {
    const PlBatchArgs &B = pl_batch(K);
    const int64_t tile = static_cast<int64_t>(B.tile0) + blockIdx.x;
    const int32_t stage = B.tile_stage[tile];
    i = static_cast<int64_t>(B.tile_off[tile]) + threadIdx.x;
    pos0 = B.stage_pos0[stage];
    n_pos = B.stage_npos[stage];
    state += static_cast<size_t>(stage) * kPlState(D);
    istate += static_cast<size_t>(stage) * kPlInts;
  } else {
    i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    pos0 = A.pos0;
    n_pos = A.n_pos;
  }
  if (i >= n_pos || istate[1] <= 0) return;
  if constexpr (MASK) {
    if (istate[0] == 5) return;  // (no consensus: the chain keeps its rows)
  }
  double g[G];
#pragma unroll
  for (int k = 0; k < G; ++k) g[k] = state[2 * G + k];
  const int64_t pos = pos0 + i;
  pl_apply<D>(g, A.x + static_cast<size_t>(A.pos_rot[pos]) * D, A.x + static_cast<size_t>(A.pos_trn[pos]) * D);
}
#endif  // CORA_TU & (2 | 8 | 16)

#if CORA_TU & 16
// ---------------------------------------------------------------------------
// the consensus vote (PlRobustArgs, kernels.h)
// ---------------------------------------------------------------------------
// the first entry and the length of a stage's list
__device__ __forceinline__ void pl_list_span(const PlRobustArgs &R, int32_t stage, int32_t *begin, int32_t *len) {
  const PlArgs &A = R.B.A;
  const int32_t last = R.B.stage_chunk0[stage + 1] - 1;
  *begin = A.chunk_begin[R.B.stage_chunk0[stage]];
  *len = A.chunk_begin[last] + A.chunk_len[last] - *begin;
}

// The hypotheses of a level's lists.  ONE wavefront per entry, four per workgroup, a launch of its own: the 7 x 7 or 16 x 16
// factor never shares registers with the vote's inner loop.  Lane k < m stages entry k of the sample -- its kPlTerms(D) terms
// and its weight -- in LDS; lane p takes the pair sums p, p + 64, p + 128 (pl_pair_sum over the m staged entries: from the left
// in the order k); lane 0 then solves and polishes with the normal matrix, its factor and the sums in LDS (731 doubles per
// wavefront at D = 3, 23 KB per workgroup) and writes g_h into the workspace, structure of arrays, and the validity into the
// entry's vote word (0 | -1).  The entry's chunk, and so its stage, by bisection of the level's chunk_begin.
template <int D>
__global__ __launch_bounds__(256) void k_pl_hyp(const PlRobustArgs R) {
  constexpr int NT = kPlTerms(D), NP = kPlSums(D), N = kPlUnknowns(D), G = kPlG(D), W = 256 / kWave;
  __shared__ double term[W][NT * NT];
  __shared__ double wt[W][NT];
  __shared__ double S[W][NP];
  __shared__ double work[W][N * (N + 1)];
  const PlArgs &A = R.B.A;
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int64_t he = static_cast<int64_t>(blockIdx.x) * W + w;
  const bool active = he < R.n_ent;  // (the whole wavefront)
  int32_t begin = 0, len = NT, h = 0;
  int64_t e = 0;
  PlStageRef T{A.x, A.x, nullptr, nullptr};
  if (active) {
    e = static_cast<int64_t>(R.ent0) + he;
    int32_t lo = A.chunk0, hi = A.chunk0 + A.n_chunks - 1;  // the last chunk of the level that begins at or before e
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo + 1) / 2;
      if (A.chunk_begin[mid] <= e) lo = mid;
      else hi = mid - 1;
    }
    const int32_t stage = R.B.chunk_stage[lo];
    pl_list_span(R, stage, &begin, &len);
    h = static_cast<int32_t>(e - begin);
    T = pl_stage_ref<D>(R.B, stage);
    if (lane < NT) {
      const int64_t ek = static_cast<int64_t>(begin) + pl_sample<D>(h, lane, len);
      const int32_t m = A.ent_m[ek];
      double c[NT];
      pl_linear_terms<D>(T.q0, T.a0, A.x + static_cast<size_t>(A.ent_q[ek]) * D, A.x + static_cast<size_t>(A.ent_a[ek]) * D, A.range_data[m], c);
#pragma unroll
      for (int i = 0; i < NT; ++i) term[w][lane * NT + i] = c[i];
      wt[w][lane] = A.range_data[A.n_ranges + m];
    }
  }
  __syncthreads();
  if (active) {
    for (int p = lane; p < NP; p += kWave) {
      int i, j;
      pl_pair(NT, p, &i, &j);
      S[w][p] = pl_pair_sum(term[w], wt[w], NT, NT, i, j);
    }
  }
  __syncthreads();
  if (!active || lane != 0) return;
  double g[G];
  const bool valid = pl_hypothesis<D>(S[w], work[w], T.q0, T.a0,
                                      [&](int k, const double **q, const double **a, double *r, double *om) {
                                        const int64_t ek = static_cast<int64_t>(begin) + pl_sample<D>(h, k, len);
                                        const int32_t m = A.ent_m[ek];
                                        *q = A.x + static_cast<size_t>(A.ent_q[ek]) * D;
                                        *a = A.x + static_cast<size_t>(A.ent_a[ek]) * D;
                                        *r = A.range_data[m];
                                        *om = A.range_data[A.n_ranges + m];
                                      }, g);
#pragma unroll
  for (int i = 0; i < G; ++i) R.hyp[static_cast<int64_t>(i) * R.hstride + e] = g[i];
  R.votes[e] = valid ? 0 : -1;
}

// One workgroup per chunk of the level; thread t owns the hypothesis of entry chunk_begin + t in registers (D*D + D doubles).
// The workgroup walks ALL chunks of its stage's list: each step stages one chunk's entries in LDS -- what does not depend on
// the hypothesis: q' = q - q_0, a' = a - a_0, r, omega; 2D + 2 doubles each, structure of arrays, 16 KB at D = 3 -- and every
// thread scores its hypothesis against the tile.  In the inner loop all lanes read one LDS address: a broadcast, no bank
// conflict.  The vote is an integer written once per entry: no order to keep.  Threads beyond chunk_len stage and own nothing.
// L^2 scores per list.
template <int D>
__global__ __launch_bounds__(kPlChunk) void k_pl_vote(const PlRobustArgs R) {
  constexpr int NF = 2 * D + 2, G = kPlG(D);
  __shared__ double tile[NF][kPlChunk];
  const PlArgs &A = R.B.A;
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t stage = R.B.chunk_stage[chunk];
  const int t = threadIdx.x;
  const bool own = t < A.chunk_len[chunk];
  const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + t;
  const PlStageRef T = pl_stage_ref<D>(R.B, stage);
  double g[G], q0[D], a0[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    q0[i] = T.q0[i];
    a0[i] = T.a0[i];
  }
  bool valid = false;
#pragma unroll
  for (int i = 0; i < G; ++i) g[i] = 0.0;
  if (own) {
    valid = R.votes[e] >= 0;
#pragma unroll
    for (int i = 0; i < G; ++i) g[i] = R.hyp[static_cast<int64_t>(i) * R.hstride + e];
  }
  int32_t vote = 0;
  for (int32_t c = R.B.stage_chunk0[stage]; c < R.B.stage_chunk0[stage + 1]; ++c) {
    const int len = A.chunk_len[c];
    __syncthreads();  // (the tile of the step before is read no more)
    if (t < len) {
      const int64_t ej = static_cast<int64_t>(A.chunk_begin[c]) + t;
      const int32_t m = A.ent_m[ej];
      const double *q = A.x + static_cast<size_t>(A.ent_q[ej]) * D, *a = A.x + static_cast<size_t>(A.ent_a[ej]) * D;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        tile[i][t] = q[i] - q0[i];
        tile[D + i][t] = a[i] - a0[i];
      }
      tile[2 * D][t] = A.range_data[m];
      tile[2 * D + 1][t] = A.range_data[A.n_ranges + m];
    }
    __syncthreads();
    if (own && valid) {
      for (int j = 0; j < len; ++j) {
        double qq[D], aa[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          qq[i] = tile[i][j];
          aa[i] = tile[D + i][j];
        }
        vote += cl_agrees(pl_cost_at<D>(g, qq, aa, tile[2 * D][j], tile[2 * D + 1][j]), R.barc2) ? 1 : 0;
      }
    }
  }
  if (own) R.votes[e] = vote;
}

// one wavefront per stage of the level: the entry of largest vote, the lowest entry among equal votes; lane 0 writes its
// hypothesis (the workspace's, what the vote read) into cstate and sets status 5 where the consensus is below the minimum
// (0 otherwise: the linear fold's solve overwrites it)
template <int D>
__global__ __launch_bounds__(kWave) void k_pl_elect(const PlRobustArgs R) {
  constexpr int G = kPlCState(D);
  const PlArgs &A = R.B.A;
  const int32_t stage = R.B.stage0 + static_cast<int32_t>(blockIdx.x);
  const int lane = threadIdx.x;
  int32_t begin, len;
  pl_list_span(R, stage, &begin, &len);
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
  double g[G];
#pragma unroll
  for (int i = 0; i < G; ++i) g[i] = R.hyp[static_cast<int64_t>(i) * R.hstride + begin + be];
#pragma unroll
  for (int i = 0; i < G; ++i) R.cstate[static_cast<size_t>(stage) * G + i] = g[i];
  R.cint[static_cast<size_t>(stage) * kPlCInts] = be;
  R.cint[static_cast<size_t>(stage) * kPlCInts + 1] = bv;
  A.istate[static_cast<size_t>(stage) * kPlInts] = bv < R.min_consensus ? 5 : 0;
  A.istate[static_cast<size_t>(stage) * kPlInts + 1] = -1;
  if (!odom_finite(g, G)) atomicOr(A.flag, 1);
}
#endif  // CORA_TU & 16
