// Part of kernels.hip (included there, in this order, inside namespace cora).  placement from pose-landmark sightings: per stage one pass over the chunks of ALL the stage's lists and one fold per list with the closed-form solve (landmark sums, chain sums, chain costs, landmark costs), then the rigid motion of the stage's chains (SgArgs, kernels.h) -- CORA_TU & 2
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

template <int D, int MODE>
__global__ __launch_bounds__(kSgChunk) void k_sg_pass(const SgArgs A) {
  constexpr int NS = SgSums<D, MODE>::value;
  __shared__ double sm[kSgChunk / kWave][NS];
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
    if constexpr (MODE == 3) {
      s[0] = sg_lm_cost<D>(p, l, tau);
    } else {
      (void)sg_entry<D>(A, A.chunk_begin[A.list_chunk0[list]], p0, &l0);  // the list's first entry
      if constexpr (MODE == 0) {
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

// one wavefront per list of the stage: the sums of its chunks, then lane 0 solves (sg_fold)
template <int D, int MODE>
__global__ __launch_bounds__(kWave) void k_sg_fold(const SgArgs A) {
  constexpr int NS = SgSums<D, MODE>::value;
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  double s[NS];
  list_sums<NS, int64_t>(s, A.partial, A.pstride, A.list_chunk0[list], A.list_chunk0[list + 1]);
  if (threadIdx.x != 0) return;
  double p0[D];
  const double *l0;
  (void)sg_entry<D>(A, A.chunk_begin[A.list_chunk0[list]], p0, &l0);
  const int32_t row = A.list_row[list];
  if (!sg_fold<D, MODE>(s, A.state + static_cast<size_t>(list) * kSgState(D), A.istate + static_cast<size_t>(list) * kSgInts, p0, l0,
                        row >= 0 ? A.x + static_cast<size_t>(row) * D : nullptr))
    atomicOr(A.flag, 1);
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
#endif  // CORA_TU & 2
