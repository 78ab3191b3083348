// Part of kernels.hip (included there, in this order, inside namespace cora).  placement from inter-chain relative-pose edges: per stage one pass over the chunks of ALL the stage's lists and one fold per list (the sums with the closed-form solve, then the two costs); the rigid motion of the stage's chains is k_sg_apply (ClArgs, kernels.h) -- CORA_TU & 2
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// placement from closures
// ---------------------------------------------------------------------------
// One thread per entry of a chunk, the entry's terms in registers (28 doubles at D = 3 for the sums).  The terms and
// everything the fold computes are functions of kernels.h the host mirror calls; the sums are taken in the order
// kernels.h writes down.  No atomics on doubles; the launches are the only synchronisation between workgroups.
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

template <int D, int MODE>
__global__ __launch_bounds__(kClChunk) void k_cl_pass(const ClArgs A) {
  constexpr int NS = ClSums<D, MODE>::value;
  __shared__ double sm[kClChunk / kWave][NS];
  const int64_t chunk = static_cast<int64_t>(A.chunk0) + blockIdx.x;
  const int32_t list = A.chunk_list[chunk];
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  if (static_cast<int>(threadIdx.x) < A.chunk_len[chunk]) {
    const int64_t e = static_cast<int64_t>(A.chunk_begin[chunk]) + threadIdx.x;
    double P[D * D], q[D], l[D], q0[D], l0[D], res, kt[2];
    {
      double P0[D * D], res0, kt0[2];
      cl_load<D>(A, A.chunk_begin[A.list_chunk0[list]], P0, q0, l0, &res0, kt0);  // the list's first entry
    }
    cl_load<D>(A, e, P, q, l, &res, kt);
    if constexpr (MODE == 0) {
      cl_terms<D>(q0, l0, P, q, l, kt[0], kt[1], s);
    } else {
      constexpr int GS = kSgG(D) + D;
      double g[GS];
#pragma unroll
      for (int i = 0; i < GS; ++i) g[i] = A.state[static_cast<size_t>(list) * kSgState(D) + i];
      s[0] = res;
      s[1] = cl_cost_at<D>(g, q0, l0, P, q, l, kt[0], kt[1]);
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
    for (int j = 1; j < kClChunk / kWave; ++j) v = v + sm[j][threadIdx.x];
    A.partial[static_cast<size_t>(threadIdx.x) * A.pstride + chunk] = v;
  }
}

// one wavefront per list of the stage: the sums of its chunks, then lane 0 solves or compares (cl_fold)
template <int D, int MODE>
__global__ __launch_bounds__(kWave) void k_cl_fold(const ClArgs A) {
  constexpr int NS = ClSums<D, MODE>::value;
  const int64_t list = static_cast<int64_t>(A.list0) + blockIdx.x;
  const int lane = threadIdx.x;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  for (int64_t c = static_cast<int64_t>(A.list_chunk0[list]) + lane; c < A.list_chunk0[list + 1]; c += kWave)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + A.partial[static_cast<size_t>(i) * A.pstride + c];
  ml_wave_sum<NS>(s);
  if (lane != 0) return;
  double P0[D * D], q0[D], l0[D], res0, kt0[2];
  cl_load<D>(A, A.chunk_begin[A.list_chunk0[list]], P0, q0, l0, &res0, kt0);
  if (!cl_fold<D, MODE>(s, A.state + static_cast<size_t>(list) * kSgState(D), A.istate + static_cast<size_t>(list) * kSgInts, q0, l0))
    atomicOr(A.flag, 1);
}
#endif  // CORA_TU & 2
