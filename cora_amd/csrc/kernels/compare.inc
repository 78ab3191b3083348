// Part of kernels.hip (included there, in this order, inside namespace cora).  comparison of a resident estimate with a resident reference after an orthogonal alignment on the selected poses' positions (CompareArgs, kernels.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// trajectory comparison
// ---------------------------------------------------------------------------
// The pass has the shape of the residual kernels (residuals.inc): an entity belongs to a fixed group of kResidualLanes = 8
// lanes, 32 entities to a block.  In the first two steps the lanes stride over the columns of the entity's translation
// row in pieces of 16 bytes (even row stride) or 8 (odd), X and Ref each at its own stride.  In the third the lanes
// stride over the kr OUTPUT columns in such pieces (the row of Ref is read and the row of the aligned vector written
// that way) and every lane walks the whole row of X, which its group reads at one address; a column's sum runs over
// a = 0 .. k - 1 in that order with one fma per term, the squares of a lane's columns are added in column order, and the
// lanes by the butterfly over the distances 4, 2, 1: an entity's errors depend on its rows, the means and A alone.  Block
// totals go to fixed slots (launch_reduce_partials / k_reduce_max_partials finish them): no atomics on doubles.

constexpr int kCompareGroups = 256 / kResidualLanes;

// column sums of X | Ref over the selected poses' translation rows: partial[k + kr][gridDim.x]
template <int WX, int WR>
__global__ __launch_bounds__(256) void k_compare_sums(CompareArgs A) {
  __shared__ double sm[2 * kMaxLD][kCompareGroups + 1];
  constexpr int G = kResidualLanes;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int i = blockIdx.x * kCompareGroups + grp;
  const bool live = i < A.n && A.sel[i] != 0;
  const int32_t row = i < A.n ? A.trn_row[i] : 0;
  for (int v = g; v * WX < A.k; v += G) {
    double x[WX] = {};
    if (live) res_load<WX>(A.X, row, A.ldx, v * WX, A.k, x);
#pragma unroll
    for (int j = 0; j < WX; ++j)
      if (v * WX + j < A.k) sm[v * WX + j][grp] = x[j];
  }
  for (int v = g; v * WR < A.kr; v += G) {
    double x[WR] = {};
    if (live) res_load<WR>(A.Ref, row, A.ldr, v * WR, A.kr, x);
#pragma unroll
    for (int j = 0; j < WR; ++j)
      if (v * WR + j < A.kr) sm[A.k + v * WR + j][grp] = x[j];
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < A.k + A.kr) {
    double s = 0.0;
    for (int q = 0; q < kCompareGroups; ++q) s += sm[t][q];
    A.partial[static_cast<size_t>(t) * gridDim.x + blockIdx.x] = s;
  }
}

// Xc[t_i] = x_i - mean(x), Gc[t_i] = g_i - mean(g) for the selected poses (every other row stays as the caller zeroed it)
template <int WX, int WR>
__global__ __launch_bounds__(256) void k_compare_centre(CompareArgs A) {
#pragma clang fp contract(off)
  constexpr int G = kResidualLanes;
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int i = blockIdx.x * kCompareGroups + grp;
  if (i >= A.n || A.sel[i] == 0) return;
  const int32_t row = A.trn_row[i];
  for (int v = g; v * WX < A.k; v += G) {
    double x[WX];
    res_load<WX>(A.X, row, A.ldx, v * WX, A.k, x);
#pragma unroll
    for (int j = 0; j < WX; ++j)
      if (v * WX + j < A.k) A.Xc[static_cast<size_t>(row) * A.ldx + v * WX + j] = x[j] - A.sums[v * WX + j] / A.m;
  }
  for (int v = g; v * WR < A.kr; v += G) {
    double x[WR];
    res_load<WR>(A.Ref, row, A.ldr, v * WR, A.kr, x);
#pragma unroll
    for (int j = 0; j < WR; ++j)
      if (v * WR + j < A.kr) A.Gc[static_cast<size_t>(row) * A.ldr + v * WR + j] = x[j] - A.sums[A.k + v * WR + j] / A.m;
  }
}

// One row of X through A for the lane's output columns: acc[q] = sum_a (x_a - shift_a) A[a][col_q]  (shift == nullptr: 0),
// then what the row contributes to the squared error against the row of Ref (minus gshift), and the aligned row
// (acc + gshift).  NP pieces of W columns per lane: piece p is number g + 8 p.
template <int W>
struct CompareRow {
  static constexpr int NP = W == 2 ? 2 : 3, NC = NP * W;  // covers kMaxLD = 24 columns over 8 lanes
  template <bool CENTRED>
  static __device__ __forceinline__ double run(const CompareArgs &A, const double *sA, const double *sx, const double *sg, int32_t row,
                                               int g, bool want_err) {
#pragma clang fp contract(off)
    double acc[NC] = {};
    const double *x = A.X + static_cast<size_t>(row) * A.ldx;
    for (int a = 0; a < A.k; ++a) {
      const double xa = CENTRED ? x[a] - sx[a] : x[a];
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const int col = (g + kResidualLanes * (q / W)) * W + q % W;
        if (col < A.kr) acc[q] = fma(xa, sA[a * A.kr + col], acc[q]);
      }
    }
    double sq = 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c0 = (g + kResidualLanes * p) * W;
      if (c0 >= A.kr) continue;
      if (want_err) {
        double ref[W];
        res_load<W>(A.Ref, row, A.ldr, c0, A.kr, ref);
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (c0 + j < A.kr) {
            const double diff = CENTRED ? acc[p * W + j] - (ref[j] - sg[c0 + j]) : acc[p * W + j] - ref[j];
            sq = fma(diff, diff, sq);
          }
      }
      if (A.aligned) {
        double *o = A.aligned + static_cast<size_t>(row) * A.ldr + c0;
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (c0 + j < A.kr) o[j] = CENTRED ? acc[p * W + j] + sg[c0 + j] : acc[p * W + j];
      }
    }
    return sq;
  }
};

template <int D, int W>
__global__ __launch_bounds__(256) void k_compare_errors(CompareArgs A) {
#pragma clang fp contract(off)
  __shared__ double sA[kMaxLD * kMaxLD], sx[kMaxLD], sg[kMaxLD], sm[4];
  constexpr int G = kResidualLanes;
  for (int t = threadIdx.x; t < A.k * A.kr; t += 256) sA[t] = A.A[t];
  if (threadIdx.x < A.k) sx[threadIdx.x] = A.sums[threadIdx.x] / A.m;
  if (threadIdx.x < A.kr) sg[threadIdx.x] = A.sums[A.k + threadIdx.x] / A.m;
  __syncthreads();
  const int g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int e = blockIdx.x * kCompareGroups + grp;
  const int total = A.nt + (A.aligned ? A.nr : 0);
  double trn = 0.0, rot = 0.0;
  const bool is_trans = e < A.nt, is_pose = e < A.n;
  const bool selected = is_trans && A.sel[e] != 0;
  if (is_trans && (selected || A.aligned)) {
    trn = CompareRow<W>::template run<true>(A, sA, sx, sg, A.trn_row[e], g, selected);
    if (is_pose) {
      const int32_t r0 = A.rot_row[e];
#pragma unroll
      for (int c = 0; c < D; ++c) rot += CompareRow<W>::template run<false>(A, sA, sx, sg, r0 + c, g, selected);
    }
  } else if (!is_trans && e < total) {
    (void)CompareRow<W>::template run<false>(A, sA, sx, sg, A.rng_row[e - A.nt], g, false);
  }
  trn = group_sum_8(trn);
  rot = group_sum_8(rot);
  double t2 = 0.0, r2 = 0.0, l2 = 0.0, tmax = 0.0, rmax = 0.0, lmax = 0.0;
  if (is_trans && g == 0) {
    const double et = selected ? sqrt(trn) : 0.0, er = selected ? sqrt(rot) : 0.0;
    if (!(fabs(et) <= 1.79769313486231570815e308) || !(fabs(er) <= 1.79769313486231570815e308)) atomicOr(A.flag, 1);
    if (is_pose) {
      A.et[e] = et;
      A.er[e] = er;
      t2 = et * et;
      r2 = er * er;
      tmax = et;
      rmax = er;
    } else {
      A.el[e - A.n] = et;
      l2 = et * et;
      lmax = et;
    }
  }
  const double s0 = block_sum_256(t2, sm);
  const double s1 = block_sum_256(r2, sm);
  const double s2 = block_sum_256(l2, sm);
  const double m0 = block_max_256(tmax, sm);
  const double m1 = block_max_256(rmax, sm);
  const double m2 = block_max_256(lmax, sm);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    A.partial[0 * nb + blockIdx.x] = s0;
    A.partial[1 * nb + blockIdx.x] = s1;
    A.partial[2 * nb + blockIdx.x] = s2;
    A.partial[3 * nb + blockIdx.x] = m0;
    A.partial[4 * nb + blockIdx.x] = m1;
    A.partial[5 * nb + blockIdx.x] = m2;
  }
}
#endif  // CORA_TU & 2
