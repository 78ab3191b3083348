// Part of kernels.hip (included there, in this order, inside namespace cora).  placement from pose-landmark sightings: per stage one pass over the chunks of ALL the stage's lists and one fold per list with the closed-form solve (landmark sums, chain sums, chain costs, landmark costs), then the rigid motion of the stage's chains (SgArgs, kernels.h); the outlier-robust form: the chain hypotheses, the consensus vote (one workgroup per chunk, the list's entries through an LDS tile), the election, and the same pass and fold over the inliers (SgRobustArgs) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// placement from sightings
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's terms in registers (18 doubles at D = 3 for a chain's sums).  The terms
// and everything the fold computes are functions of kernels.h the host mirror calls; the sums are taken in the order
// kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the launches are the only
// synchronisation between workgroups.
template <int D, int MODE>
struct SgSums {
  static constexpr int value = MODE == 0 ? kSgLmSums(D) : (MODE == 1 ? kSgChainSums(D) : (MODE == 2 ? kSgCostSums : 1));
};

// the entry's data: its prediction, its edge's tau, the landmark's row
template <int D>
__device__ __forceinline__ double sg_entry(const SgArgs &A, int64_t e, double *p, const double **l) {
  const int32_t m = A.ent_e[e];
  double t[D];
#pragma unroll
  for (int c = 0; c < D; ++c) t[c] = A.edge_data[static_cast<size_t>(D * D + c) * A.n_edges + m];
  sg_predict<D>(A.x + static_cast<size_t>(A.ent_rot[e]) * D, A.x + static_cast<size_t>(A.ent_trn[e]) * D, t, p);
  *l = A.x + static_cast<size_t>(A.ent_lm[e]) * D;
  return A.edge_data[static_cast<size_t>(D * D + D + 1) * A.n_edges + m];
}

// the kernels' argument of the plain (SgArgs) and of the robust form (SgRobustArgs), and the plain part of either
template <bool ROBUST>
using SgKernelArgs = std::conditional_t<ROBUST, SgRobustArgs, SgArgs>;
__host__ __device__ inline const SgArgs &sg_plain(const SgArgs &A) { return A; }
__host__ __device__ inline const SgArgs &sg_plain(const SgRobustArgs &R) { return R.A; }

// ROBUST: over the inliers of the elected hypothesis (k_sg_vote, k_sg_elect below): each entry re-evaluates r(h*, j) <= barc2
// from cstate (the vote's function, the vote's bits); an entry outside I leaves its terms at +0.0.  Modes 0 and 1 also write
// the edge's flag byte (landmark lists, chain lists).  The plain form loads none of that.
template <int D, int MODE, bool ROBUST>
__global__ __launch_bounds__(kSgChunk) void k_sg_pass(const SgKernelArgs<ROBUST> K) {
  constexpr int NS = SgSums<D, MODE>::value;
  __shared__ double sm[kSgChunk / kWave][NS];
  const SgArgs &A = sg_plain(K);
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t list = A.chunk_list[chunk];
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    double p[D], p0[D];
    const double *l, *l0;
    const double tau = sg_entry<D>(A, e, p, &l);
    if constexpr (MODE != 3 || ROBUST) (void)sg_entry<D>(A, A.chunk_begin[A.list_chunk0[list]], p0, &l0);  // the list's first entry
    bool in = true;
    if constexpr (ROBUST) {
      constexpr int CS = MODE == 0 || MODE == 3 ? D : kSgCState(D);
      double h[CS], pp[D], ll[D];
#pragma unroll
      for (int i = 0; i < CS; ++i) h[i] = K.cstate[static_cast<size_t>(list) * kSgCState(D) + i];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        pp[c] = p[c] - p0[c];
        ll[c] = l[c] - l0[c];
      }
      if constexpr (MODE == 0 || MODE == 3) {
        in = cl_agrees(sg_lm_cost<D>(pp, h, tau), K.barc2);
      } else {
        in = cl_agrees(sg_cost_rel<D>(h, pp, ll, tau), K.barc2);
      }
      if constexpr (MODE == 0) K.inlier_landmark[A.ent_e[e]] = in ? 1 : 0;
      if constexpr (MODE == 1) K.inlier_chain[A.ent_e[e]] = in ? 1 : 0;
    }
    if (in) {
      if constexpr (MODE == 3) {
        s[0] = sg_lm_cost<D>(p, l, tau);
      } else if constexpr (MODE == 0) {
        sg_lm_terms<D>(p0, p, tau, s);
      } else if constexpr (MODE == 1) {
        sg_chain_terms<D>(p0, l0, p, l, tau, s);
      } else {
        constexpr int GS = kSgG(D) + D;
        double g[GS];
#pragma unroll
        for (int i = 0; i < GS; ++i) g[i] = A.state[static_cast<size_t>(list) * kSgState(D) + i];
        sg_cost_terms<D>(g, p0, l0, p, l, tau, s);
      }
    }
  }
  chunk_sums<NS>(s, sm, A.partial, A.pstride, chunk);
}

// one wavefront per list of the stage: the sums of its chunks, then lane 0 solves (sg_fold; ROBUST: sg_fold_robust, status 5
// passed through)
template <int D, int MODE, bool ROBUST>
__global__ __launch_bounds__(kWave) void k_sg_fold(const SgKernelArgs<ROBUST> K) {
  constexpr int NS = SgSums<D, MODE>::value;
  const SgArgs &A = sg_plain(K);
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  double s[NS];
  list_sums<NS, int64_t>(s, A.partial, A.pstride, A.list_chunk0[list], A.list_chunk0[list + 1]);
  if (threadIdx.x != 0) return;
  double p0[D];
  const double *l0;
  (void)sg_entry<D>(A, A.chunk_begin[A.list_chunk0[list]], p0, &l0);
  const int32_t row = A.list_row[list];
  double *st = A.state + static_cast<size_t>(list) * kSgState(D), *xr = row >= 0 ? A.x + static_cast<size_t>(row) * D : nullptr;
  int32_t *ist = A.istate + static_cast<size_t>(list) * kSgInts;
  if (!(ROBUST ? sg_fold_robust<D, MODE>(s, st, ist, p0, l0, xr) : sg_fold<D, MODE>(s, st, ist, p0, l0, xr))) atomicOr(A.flag, 1);
}

// The rigid motion of a stage's chains (k_sg_apply), for every placement whose lists' state begins with the motion (R
// row-major | t) and whose istate[1] is `chosen`: position i of the stage moves under the motion of its list where chosen > 0.
// The launchers fill it from the stage their own arguments describe (chain_apply, launch.inc); a list whose cost did not fall
// writes nothing.
struct SgApplyArgs {
  int d = 0;
  int32_t apply0 = 0, n_apply = 0;
  const int32_t *apply_pos = nullptr, *apply_list = nullptr, *pos_rot = nullptr, *pos_trn = nullptr;
  const double *state = nullptr;
  const int32_t *istate = nullptr;
  double *x = nullptr;
};
template <int D>
__global__ __launch_bounds__(256) void k_sg_apply(const SgApplyArgs A) {
  constexpr int G = kSgG(D);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= A.n_apply) return;
  const int32_t list = A.apply_list[A.apply0 + i];
  if (A.istate[static_cast<size_t>(list) * kSgInts + 1] <= 0) return;
  double g[G];
#pragma unroll
  for (int k = 0; k < G; ++k) g[k] = A.state[static_cast<size_t>(list) * kSgState(D) + k];
  const int64_t pos = A.apply_pos[A.apply0 + i];
  pl_apply<D>(g, A.x + static_cast<size_t>(A.pos_rot[pos]) * D, A.x + static_cast<size_t>(A.pos_trn[pos]) * D);
}

// ---------------------------------------------------------------------------
// the consensus vote (SgRobustArgs, kernels.h)
// ---------------------------------------------------------------------------
// the first entry and the length of a list
__device__ __forceinline__ void sg_list_span(const SgArgs &A, int64_t list, int32_t *begin, int32_t *len) {
  const int32_t last = A.list_chunk0[list + 1] - 1;
  *begin = A.chunk_begin[A.list_chunk0[list]];
  *len = A.chunk_begin[last] + A.chunk_len[last] - *begin;
}

// The hypotheses of a C-stage's lists: one thread per entry of a chunk runs the plain chain solve on the sums of its sample
// (sg_hypothesis: d entries of the list, read from the rows as they stand) and writes g_h into the workspace, structure of
// arrays, and the validity into the entry's vote word (0 | -1).  A launch of its own: the solve's one-sided Jacobi keeps its
// registers to itself, and the vote below holds only g_h.
template <int D>
__global__ __launch_bounds__(kSgChunk) void k_sg_hyp(const SgRobustArgs R) {
  constexpr int GS = kSgCState(D);
  const SgArgs &A = R.A;
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  if (static_cast<int>(threadIdx.x) >= A.chunk_len[chunk]) return;
  const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
  int32_t begin, len;
  sg_list_span(A, A.chunk_list[chunk], &begin, &len);
  double p0[D], g[GS];
  const double *l0;
  (void)sg_entry<D>(A, begin, p0, &l0);
  const bool valid = sg_hypothesis<D>(static_cast<int32_t>(e - begin), len, p0, l0,
                                      [&](int32_t j, double *p, const double **l) { return sg_entry<D>(A, static_cast<int64_t>(begin) + j, p, l); }, g);
#pragma unroll
  for (int i = 0; i < GS; ++i) R.hyp[static_cast<int64_t>(i) * R.hstride + e] = g[i];
  R.votes[e] = valid ? 0 : -1;
}

// One workgroup per chunk of the stage; thread t owns the hypothesis of entry chunk_begin + t in registers (KIND 0, a landmark
// list: y_h = p'_h, D doubles; KIND 1, a chain list: g_h from the workspace, D*D + 2D doubles).  The workgroup walks ALL chunks
// of its list: each step stages one chunk's entries in LDS -- what does not depend on the hypothesis: p' = p - p_0, for a chain
// l' = l - l_0, tau; D + 1 resp. 2D + 1 doubles each, structure of arrays, at most 14 KB -- with one sg_entry per thread, and
// every thread scores its hypothesis against the tile.  In the inner loop all lanes read one LDS address: a broadcast, no bank
// conflict.  The vote is an integer written once per entry: no order to keep.  Threads beyond chunk_len stage and own nothing.
template <int D, int KIND>
__global__ __launch_bounds__(kSgChunk) void k_sg_vote(const SgRobustArgs R) {
  constexpr int NF = KIND == 0 ? D + 1 : 2 * D + 1, GS = KIND == 0 ? D : kSgCState(D);
  __shared__ double tile[NF][kSgChunk];
  const SgArgs &A = R.A;
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t list = A.chunk_list[chunk];
  const int t = threadIdx.x;
  const bool own = t < A.chunk_len[chunk];
  const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + t;
  double g[GS], p0[D];
  const double *l0;
  (void)sg_entry<D>(A, A.chunk_begin[A.list_chunk0[list]], p0, &l0);  // the list's first entry
  bool valid = false;
#pragma unroll
  for (int i = 0; i < GS; ++i) g[i] = 0.0;
  if (own) {
    if constexpr (KIND == 0) {
      double p[D];
      const double *l;
      (void)sg_entry<D>(A, e, p, &l);
#pragma unroll
      for (int c = 0; c < D; ++c) g[c] = p[c] - p0[c];
      valid = true;
    } else {
      valid = R.votes[e] >= 0;
#pragma unroll
      for (int i = 0; i < GS; ++i) g[i] = R.hyp[static_cast<int64_t>(i) * R.hstride + e];
    }
  }
  int32_t vote = 0;
  for (int32_t c = A.list_chunk0[list]; c < A.list_chunk0[list + 1]; ++c) {
    const int len = A.chunk_len[c];
    __syncthreads();  // (the tile of the step before is read no more)
    if (t < len) {
      double p[D];
      const double *l;
      const double tau = sg_entry<D>(A, static_cast<int64_t>(A.chunk_begin[c]) + t, p, &l);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        tile[i][t] = p[i] - p0[i];
        if constexpr (KIND == 1) tile[D + i][t] = l[i] - l0[i];
      }
      tile[NF - 1][t] = tau;
    }
    __syncthreads();
    if (own && valid) {
      for (int j = 0; j < len; ++j) {
        double pp[D], ll[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          pp[i] = tile[i][j];
          if constexpr (KIND == 1) ll[i] = tile[D + i][j];
        }
        double r;
        if constexpr (KIND == 0) {
          r = sg_lm_cost<D>(pp, g, tile[NF - 1][j]);
        } else {
          r = sg_cost_rel<D>(g, pp, ll, tile[NF - 1][j]);
        }
        vote += cl_agrees(r, R.barc2) ? 1 : 0;
      }
    }
  }
  if (own) R.votes[e] = vote;
}

// one wavefront per list of the stage: the entry of largest vote, the lowest entry among equal votes; lane 0 writes its
// hypothesis (a landmark list: recomputed; a chain list: the workspace's, what the vote read) into cstate and sets status 5
// where the consensus is below the minimum of the list's kind (0 otherwise: the fold's solve overwrites it)
template <int D, int KIND>
__global__ __launch_bounds__(kWave) void k_sg_elect(const SgRobustArgs R) {
  constexpr int GS = KIND == 0 ? D : kSgCState(D);
  const SgArgs &A = R.A;
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  const int lane = threadIdx.x;
  int32_t begin, len;
  sg_list_span(A, list, &begin, &len);
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
  double g[GS];
  if constexpr (KIND == 0) {
    double p0[D], p[D];
    const double *l;
    (void)sg_entry<D>(A, begin, p0, &l);
    (void)sg_entry<D>(A, static_cast<int64_t>(begin) + be, p, &l);
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = p[c] - p0[c];
  } else {
#pragma unroll
    for (int i = 0; i < GS; ++i) g[i] = R.hyp[static_cast<int64_t>(i) * R.hstride + begin + be];
  }
#pragma unroll
  for (int i = 0; i < GS; ++i) R.cstate[static_cast<size_t>(list) * kSgCState(D) + i] = g[i];
  R.cint[static_cast<size_t>(list) * kSgCInts] = be;
  R.cint[static_cast<size_t>(list) * kSgCInts + 1] = bv;
  A.istate[static_cast<size_t>(list) * kSgInts] = bv < (KIND == 0 ? R.min_landmark_consensus : R.min_chain_consensus) ? 5 : 0;
  A.istate[static_cast<size_t>(list) * kSgInts + 1] = 0;
  if (!odom_finite(g, GS)) atomicOr(A.flag, 1);
}
#endif  // CORA_TU & 2
