// Part of kernels.hip (included there, in this order, inside namespace cora).  placement from inter-chain relative-pose edges: per stage one pass over the chunks of ALL the stage's lists and one fold per list (the sums with the closed-form solve, then the two costs); the rigid motion of the stage's chains is k_sg_apply (ClArgs, kernels.h); the outlier-robust form: the consensus vote (one workgroup per chunk, the list's entries through an LDS tile), the election, and the same pass and fold over the inliers (ClRobustArgs) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// placement from closures
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's terms in registers (28 doubles at D = 3 for the sums).  The terms and
// everything the fold computes are functions of kernels.h the host mirror calls; the sums are taken in the order
// kernels.h writes down (chunk_sums and list_sums, common.inc).  No atomics on doubles; the launches are the only
// synchronisation between workgroups.
template <int D, int MODE>
struct ClSums {
  static constexpr int value = MODE == 0 ? kClSums(D) : kClCostSums;
};

// the entry's data from the rows as they stand: P, q, l, the table's own residuals; kt: kappa | tau
template <int D>
__device__ __forceinline__ void cl_load(const ClArgs &A, int64_t e, double *P, double *q, double *l, double *res, double *kt) {
  constexpr int NF = D * D + D + 2;
  const int32_t m = A.ent_e[e];
  double f[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) f[i] = A.edge_data[static_cast<size_t>(i) * A.n_edges + m];
  cl_entry<D>(A.x + static_cast<size_t>(A.edge_rows[m]) * D, A.x + static_cast<size_t>(A.edge_rows[2 * A.n_edges + m]) * D,
              A.x + static_cast<size_t>(A.edge_rows[A.n_edges + m]) * D, A.x + static_cast<size_t>(A.edge_rows[3 * A.n_edges + m]) * D, f,
              A.ent_dir[e], P, q, l, res);
  kt[0] = f[D * D + D];
  kt[1] = f[D * D + D + 1];
}

// the kernels' argument of the plain (ClArgs) and of the robust form (ClRobustArgs), and the plain part of either
template <bool ROBUST>
using ClKernelArgs = std::conditional_t<ROBUST, ClRobustArgs, ClArgs>;
__host__ __device__ inline const ClArgs &cl_plain(const ClArgs &A) { return A; }
__host__ __device__ inline const ClArgs &cl_plain(const ClRobustArgs &R) { return R.A; }

// ROBUST: over the inliers of the elected hypothesis (k_cl_vote, k_cl_elect below): each entry re-evaluates r(h*, j) <= barc2
// from cstate (the vote's function, the vote's bits); an entry outside I leaves its terms at +0.0.  Mode 0 also writes the
// edge's flag byte.  The plain form loads none of that.
template <int D, int MODE, bool ROBUST>
__global__ __launch_bounds__(kClChunk) void k_cl_pass(const ClKernelArgs<ROBUST> K) {
  constexpr int NS = ClSums<D, MODE>::value, GS = kClCState(D);
  static_assert(GS == kSgG(D) + D, "the hypothesis has the layout of the state's G | s | s'");
  __shared__ double sm[kClChunk / kWave][NS];
  const ClArgs &A = cl_plain(K);
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t list = A.chunk_list[chunk];
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    double P[D * D], q[D], l[D], q0[D], l0[D], res, kt[2], g[GS];
    {
      double P0[D * D], res0, kt0[2];
      cl_load<D>(A, A.chunk_begin[A.list_chunk0[list]], P0, q0, l0, &res0, kt0);  // the list's first entry
    }
    cl_load<D>(A, e, P, q, l, &res, kt);
    bool in = true;
    if constexpr (ROBUST) {
#pragma unroll
      for (int i = 0; i < GS; ++i) g[i] = K.cstate[static_cast<size_t>(list) * GS + i];
      in = cl_agrees(cl_cost_at<D>(g, q0, l0, P, q, l, kt[0], kt[1]), K.barc2);
      if constexpr (MODE == 0) K.inlier[A.ent_e[e]] = in ? 1 : 0;
    }
    if constexpr (MODE == 0) {
      if (in) cl_terms<D>(q0, l0, P, q, l, kt[0], kt[1], s);
    } else if (in) {
#pragma unroll
      for (int i = 0; i < GS; ++i) g[i] = A.state[static_cast<size_t>(list) * kSgState(D) + i];
      s[0] = res;
      s[1] = cl_cost_at<D>(g, q0, l0, P, q, l, kt[0], kt[1]);
    }
  }
  chunk_sums<NS>(s, sm, A.partial, A.pstride, chunk);
}

// one wavefront per list of the stage: the sums of its chunks, then lane 0 solves or compares (cl_fold; ROBUST: cl_fold_robust,
// status 5 passed through)
template <int D, int MODE, bool ROBUST>
__global__ __launch_bounds__(kWave) void k_cl_fold(const ClKernelArgs<ROBUST> K) {
  constexpr int NS = ClSums<D, MODE>::value;
  const ClArgs &A = cl_plain(K);
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  double s[NS];
  list_sums<NS, int64_t>(s, A.partial, A.pstride, A.list_chunk0[list], A.list_chunk0[list + 1]);
  if (threadIdx.x != 0) return;
  double P0[D * D], q0[D], l0[D], res0, kt0[2];
  cl_load<D>(A, A.chunk_begin[A.list_chunk0[list]], P0, q0, l0, &res0, kt0);
  double *st = A.state + static_cast<size_t>(list) * kSgState(D);
  int32_t *ist = A.istate + static_cast<size_t>(list) * kSgInts;
  if (!(ROBUST ? cl_fold_robust<D, MODE>(s, st, ist, q0, l0) : cl_fold<D, MODE>(s, st, ist, q0, l0))) atomicOr(A.flag, 1);
}

// ---------------------------------------------------------------------------
// the consensus vote (ClRobustArgs, kernels.h)
// ---------------------------------------------------------------------------
// One workgroup per chunk of the stage; thread t owns the hypothesis of entry chunk_begin + t, g_h in registers.  The
// workgroup walks ALL chunks of its list: each step stages one chunk's entries (P, q' = q - q_0, l' = l - l_0, kappa, tau: what
// cl_cost_at forms of an entry whatever the hypothesis, so the score is cl_cost_rel with cl_cost_at's bits; D*D + 2D + 2 doubles each,
// structure of arrays, 34 KB at D = 3 and 20 KB at D = 2: the LDS admits four workgroups a CU; the registers:
// profiles/closure_consensus.md) with one cl_load per thread, and every thread scores its hypothesis against the tile.  In the inner loop all lanes read one LDS address: a broadcast, no bank
// conflict.  The vote is an integer: no order to keep.  Threads beyond chunk_len stage and own no hypothesis.
template <int D>
__global__ __launch_bounds__(kClChunk) void k_cl_vote(const ClRobustArgs R) {
  constexpr int NF = D * D + 2 * D + 2, GS = kClCState(D);
  __shared__ double tile[NF][kClChunk];
  const ClArgs &A = R.A;
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t list = A.chunk_list[chunk];
  const int t = threadIdx.x;
  const bool own = t < A.chunk_len[chunk];
  double g[GS], q0[D], l0[D];
  bool valid = false;
  {
    double P0[D * D], res0, kt0[2];
    cl_load<D>(A, A.chunk_begin[A.list_chunk0[list]], P0, q0, l0, &res0, kt0);  // the list's first entry
  }
#pragma unroll
  for (int i = 0; i < GS; ++i) g[i] = 0.0;
  if (own) {
    double P[D * D], q[D], l[D], res, kt[2];
    cl_load<D>(A, static_cast<int64_t>(A.chunk_begin[chunk]) + t, P, q, l, &res, kt);
    cl_hypothesis<D>(q0, l0, P, q, l, g);
    valid = kt[0] > 0.0;
    if (valid && !odom_finite(g, GS)) atomicOr(A.flag, 1);
  }
  int32_t vote = 0;
  for (int32_t c = A.list_chunk0[list]; c < A.list_chunk0[list + 1]; ++c) {
    const int len = A.chunk_len[c];
    __syncthreads();  // (the tile of the step before is read no more)
    if (t < len) {
      double P[D * D], q[D], l[D], res, kt[2];
      cl_load<D>(A, static_cast<int64_t>(A.chunk_begin[c]) + t, P, q, l, &res, kt);
#pragma unroll
      for (int i = 0; i < D * D; ++i) tile[i][t] = P[i];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        tile[D * D + i][t] = q[i] - q0[i];
        tile[D * D + D + i][t] = l[i] - l0[i];
      }
      tile[D * D + 2 * D][t] = kt[0];
      tile[D * D + 2 * D + 1][t] = kt[1];
    }
    __syncthreads();
    if (own && valid) {
      for (int j = 0; j < len; ++j) {
        double P[D * D], qq[D], ll[D];
#pragma unroll
        for (int i = 0; i < D * D; ++i) P[i] = tile[i][j];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          qq[i] = tile[D * D + i][j];
          ll[i] = tile[D * D + D + i][j];
        }
        vote += cl_agrees(cl_cost_rel<D>(g, P, qq, ll, tile[D * D + 2 * D][j], tile[D * D + 2 * D + 1][j]), R.barc2) ? 1 : 0;
      }
    }
  }
  if (own) R.votes[static_cast<int64_t>(A.chunk_begin[chunk]) + t] = vote;
}

// one wavefront per list of the stage: the entry of largest vote, the lowest entry among equal votes; lane 0 recomputes its
// hypothesis and sets status 5 where the consensus is below min_consensus (0 otherwise: the fold's solve overwrites it)
template <int D>
__global__ __launch_bounds__(kWave) void k_cl_elect(const ClRobustArgs R) {
  constexpr int GS = kClCState(D);
  const ClArgs &A = R.A;
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  const int lane = threadIdx.x;
  const int32_t last = A.list_chunk0[list + 1] - 1;
  const int32_t begin = A.chunk_begin[A.list_chunk0[list]], len = A.chunk_begin[last] + A.chunk_len[last] - begin;
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
  double P0[D * D], q0[D], l0[D], res0, kt0[2], P[D * D], q[D], l[D], res, kt[2], g[GS];
  cl_load<D>(A, begin, P0, q0, l0, &res0, kt0);
  cl_load<D>(A, static_cast<int64_t>(begin) + be, P, q, l, &res, kt);
  cl_hypothesis<D>(q0, l0, P, q, l, g);
#pragma unroll
  for (int i = 0; i < GS; ++i) R.cstate[static_cast<size_t>(list) * GS + i] = g[i];
  R.cint[static_cast<size_t>(list) * kClCInts] = be;
  R.cint[static_cast<size_t>(list) * kClCInts + 1] = bv;
  A.istate[static_cast<size_t>(list) * kSgInts] = bv < R.min_consensus ? 5 : 0;
  A.istate[static_cast<size_t>(list) * kSgInts + 1] = 0;
  if (!odom_finite(g, GS)) atomicOr(A.flag, 1);
}
#endif  // CORA_TU & 2
