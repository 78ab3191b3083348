// Part of kernels.hip (included there, in this order, inside namespace cora).  relative pose error of a resident estimate against a resident reference over the handle's pair table (RpeArgs, kernels.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// relative pose error
// ---------------------------------------------------------------------------
// The pass has the shape of the residual and comparison kernels: a pair (i, j) belongs to a fixed group of kResidualLanes
// = 8 lanes, 32 pairs to a block, the grid is sized by the count.  The lanes stride over the COLUMNS of a vector in pieces
// of 16 bytes (even row stride) or 8 (odd), X and Ref each at its own stride and column count: a group reads the 2 d + 2
// rows of the pair (rotation rows and translation row of i and of j) and forms d^2 + d partial sums per vector,
//   E[a][b] += X_i[a][c] X_j[b][c],   u[a] += X_i[a][c] (x_j[c] - x_i[c]),
// one fma per term, a lane's pieces in column order.  The lanes are added by the butterfly over the distances 4, 2, 1, X
// and Ref separately (k != kr in general); the differences are taken after the butterflies, squared and added in
// row-major order.  A pair's errors depend on its rows alone: the same bits wherever it stands in the table.  i == j is
// the identity motion in both vectors: both errors are 0.0 without a look at the rows.  Block totals go to fixed slots
// (launch_reduce_partials / k_reduce_max_partials finish them, k_rpe_argmax the index): no atomics on doubles.

// One vector's d^2 + d sums of a pair, finished over the group, each left in ONE lane: sum q (q = a * D + b for E[a][b],
// D * D + a for u[a]) ends in lane q mod 8 of the group, in v0 for q < 8 and in v1 from 8 on; the other lanes keep 0.0.
// x_j - x_i of the lane's pieces is formed once; then the rows of pose i are taken one at a time (d + 1 sums in flight, the
// rows of pose j read again from the cache for every row), a lane's rounds one after the other: with all d^2 + d sums of
// both vectors at once the kernel takes 124 to 136 VGPRs at d = 3 (3 or 4 wavefronts per SIMD); this form takes 44 to 60
// at d = 2 and 56 at d = 3 with two odd strides (8 wavefronts), 70 to 76 at d = 3 where a vector is read in 16-byte pieces
// (6 or 7), without scratch.  Every lane of the block runs the shuffles, whether its group has work or not.
template <int D, int W>
__device__ __forceinline__ void rpe_vector_sums(const double *__restrict__ V, int ld, int k, int32_t ri, int32_t ti, int32_t rj,
                                                int32_t tj, int g, bool work, double &v0, double &v1) {
#pragma clang fp contract(off)
  constexpr int G = kResidualLanes;
  const int pieces = (k + W - 1) / W;
  v0 = v1 = 0.0;
  constexpr int ROUNDS = (kMaxLD + W * G - 1) / (W * G);
  // x_j - x_i of the lane's pieces, once for all rows of pose i (one subtraction per column)
  double dx[ROUNDS][W];
#pragma unroll
  for (int it = 0; it < ROUNDS; ++it) {
    const int v = g + it * G;
#pragma unroll
    for (int c = 0; c < W; ++c) dx[it][c] = 0.0;
    if (work && v < pieces) {
      double xi[W], xj[W];
      res_load<W>(V, ti, ld, v * W, k, xi);
      res_load<W>(V, tj, ld, v * W, k, xj);
#pragma unroll
      for (int c = 0; c < W; ++c) dx[it][c] = xj[c] - xi[c];
    }
  }
#pragma unroll 1
  for (int a = 0; a < D; ++a) {
    double s[D + 1];
#pragma unroll
    for (int b = 0; b <= D; ++b) s[b] = 0.0;
    if (work) {
#pragma unroll
      for (int it = 0; it < ROUNDS; ++it) {
        const int v = g + it * G;
        if (v >= pieces) break;
        const int c0 = v * W;
        double vi[W], vj[D][W];
        res_load<W>(V, ri + a, ld, c0, k, vi);
#pragma unroll
        for (int b = 0; b < D; ++b) res_load<W>(V, rj + b, ld, c0, k, vj[b]);
#pragma unroll
        for (int c = 0; c < W; ++c) {
#pragma unroll
          for (int b = 0; b < D; ++b) s[b] = fma(vi[c], vj[b][c], s[b]);
          s[D] = fma(vi[c], dx[it][c], s[D]);
        }
        asm volatile("" ::: "memory");  // (a round's loads stay behind the round before)
      }
    }
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      const double t = group_sum_8(s[b]);
      const int q = b < D ? a * D + b : D * D + a;
      if ((q & (G - 1)) == g) {
        if (q < G) v0 = t;
        else v1 = t;
      }
    }
  }
}

// rows: [4][m] = first rotation row of i | translation row of i | first rotation row of j | translation row of j
// (internal rows).  partial[5][gridDim.x] = sum et^2, sum er^2 | max et, max er | m - (first pair of the block that
// attains the block's max et) -- the last as a double: a larger value is an earlier pair, so the finish is a maximum too.
template <int D, int WX, int WR>
__global__ __launch_bounds__(256) void k_rpe(RpeArgs A) {
#pragma clang fp contract(off)
  __shared__ double sm[4];
  constexpr int G = kResidualLanes, NS = D * D + D;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int64_t m = A.m, p = static_cast<int64_t>(blockIdx.x) * (256 / G) + grp;
  const bool live = p < m;
  int32_t ri = 0, ti = 0, rj = 0, tj = 0;
  if (live) {
    ri = A.rows[p];
    ti = A.rows[m + p];
    rj = A.rows[2 * m + p];
    tj = A.rows[3 * m + p];
  }
  const bool work = live && ri != rj;
  // X and Ref separately (k != kr in general); the differences after the butterflies, in the lane that holds the sums
  double r0, r1, x0, x1;
  rpe_vector_sums<D, WR>(A.Ref, A.ldr, A.kr, ri, ti, rj, tj, g, work, r0, r1);
  rpe_vector_sums<D, WX>(A.X, A.ldx, A.k, ri, ti, rj, tj, g, work, x0, x1);
  const double d0 = x0 - r0, d1 = x1 - r1;
  // the differences back to every lane of the group in row-major order, E before u
  const int lane0 = (threadIdx.x & 63) & ~(G - 1);
  double r2 = 0.0, t2 = 0.0;
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const double diff = __shfl(q < G ? d0 : d1, lane0 + (q & (G - 1)), 64);
    if (q < D * D) r2 = fma(diff, diff, r2);
    else t2 = fma(diff, diff, t2);
  }
  double et = 0.0, er = 0.0;
  if (work && g == 0) {
    et = sqrt(t2);
    er = sqrt(r2);
    if (!(fabs(et) <= 1.79769313486231570815e308) || !(fabs(er) <= 1.79769313486231570815e308)) atomicOr(A.flag, 1);
  }
  if (live && g == 0) {
    A.et[p] = et;
    A.er[p] = er;
  }
  const double s0 = block_sum_256(et * et, sm);
  const double s1 = block_sum_256(er * er, sm);
  const double m0 = block_max_256(et, sm);  // (the same value in every thread: all of them read the four wave maxima)
  const double m1 = block_max_256(er, sm);
  const double first = block_max_256(live && g == 0 && et == m0 ? static_cast<double>(m - p) : 0.0, sm);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    A.partial[0 * nb + blockIdx.x] = s0;
    A.partial[1 * nb + blockIdx.x] = s1;
    A.partial[2 * nb + blockIdx.x] = m0;
    A.partial[3 * nb + blockIdx.x] = m1;
    A.partial[4 * nb + blockIdx.x] = first;
  }
}

// out[0] = the first pair that attains the largest et: block_max[nblocks] the blocks' maxima, block_first[nblocks] their
// m - (first pair), *max_et the finished maximum.  One 256-thread block, fixed order.
__global__ __launch_bounds__(256) void k_rpe_argmax(const double *__restrict__ block_max, const double *__restrict__ block_first,
                                                     int nblocks, const double *__restrict__ max_et, double m,
                                                     double *__restrict__ out) {
  __shared__ double sm[4];
  const double top = *max_et;
  double best = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256)
    if (block_max[b] == top) best = fmax(best, block_first[b]);
  const double t = block_max_256(best, sm);
  if (threadIdx.x == 0) out[0] = m - t;
}
#endif  // CORA_TU & 2
