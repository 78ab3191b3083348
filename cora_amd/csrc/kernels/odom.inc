// Part of kernels.hip (included there, in this order, inside namespace cora).  odometry initialisation: the segmented scan of SE(d) over the chain positions (tile totals, their scan, the tiles' scan with the pose rows) and the fill of the other rows (OdomArgs, OdomFillArgs, kernels.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// odometry initialisation
// ---------------------------------------------------------------------------
// One thread per chain position, one element (flag, R, t) per thread in registers: 6 doubles at D = 2, 12 at D = 3, twice
// that during a step (the neighbour's element) plus the product.  The composition is odom_compose (kernels.h), the function
// the host mirror calls, applied in the order kernels.h writes down: every output row is a function of the tables, the
// starts and the tile shape alone.  The three launches are the only synchronisation between workgroups.

// the element of a position (past P: the head of nothing)
template <int D>
__device__ __forceinline__ void odom_load(const OdomArgs &A, int64_t pos, OdomEl<D> &e) {
  odom_head<D>(e);
  if (pos >= A.P) return;
  const int32_t ed = A.pos_edge[pos];
  if (ed < 0) {
    const double *s = A.starts + static_cast<size_t>(A.pos_chain[pos]) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) e.v[D * D + c] = s[c];
  } else {
#pragma unroll
    for (int f = 0; f < D * D + D; ++f) e.v[f] = A.edge_data[static_cast<size_t>(f) * A.n_edges + ed];
    e.flag = 0;
  }
}
// an element of a [field][ntiles] array
template <int D>
__device__ __forceinline__ void odom_get(const double *__restrict__ arr, int ntiles, int tile, OdomEl<D> &e) {
  e.flag = arr[tile] != 0.0 ? 1 : 0;
#pragma unroll
  for (int f = 0; f < D * D + D; ++f) e.v[f] = arr[static_cast<size_t>(f + 1) * ntiles + tile];
}
template <int D>
__device__ __forceinline__ void odom_put(double *__restrict__ arr, int ntiles, int tile, const OdomEl<D> &e) {
  arr[tile] = e.flag ? 1.0 : 0.0;
#pragma unroll
  for (int f = 0; f < D * D + D; ++f) arr[static_cast<size_t>(f + 1) * ntiles + tile] = e.v[f];
}

// inclusive scan of one element per lane over a wavefront: Kogge-Stone over lane shifts
template <int D>
__device__ __forceinline__ void odom_wave_scan(OdomEl<D> &e, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    OdomEl<D> o;
#pragma unroll
    for (int f = 0; f < D * D + D; ++f) o.v[f] = __shfl_up(e.v[f], off, kWave);
    o.flag = __shfl_up(e.flag, off, kWave);
    if (lane >= off) odom_compose<D>(o, e);
  }
}

// inclusive scan over a tile: the wavefronts' scans, their totals through LDS, the fold of the totals before a wave
template <int D>
__device__ __forceinline__ void odom_tile_scan(OdomEl<D> &e, double (*sm)[D * D + D + 1]) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  odom_wave_scan<D>(e, lane);
  if (lane == kWave - 1) {
    sm[w][0] = e.flag ? 1.0 : 0.0;
#pragma unroll
    for (int f = 0; f < D * D + D; ++f) sm[w][f + 1] = e.v[f];
  }
  __syncthreads();
  if (w > 0) {
    OdomEl<D> acc;
    odom_get<D>(&sm[0][0], 1, 0, acc);  // (sm[j] is a [field][1] array)
    for (int j = 1; j < w; ++j) {
      OdomEl<D> nxt;
      odom_get<D>(&sm[j][0], 1, 0, nxt);
      odom_compose<D>(acc, nxt);
      acc = nxt;
    }
    odom_compose<D>(acc, e);
  }
}

template <int D>
__global__ __launch_bounds__(kOdomTile) void k_odom_totals(const OdomArgs A) {
  __shared__ double sm[kOdomTile / kWave][D * D + D + 1];
  OdomEl<D> e;
  odom_load<D>(A, static_cast<int64_t>(blockIdx.x) * kOdomTile + threadIdx.x, e);
  odom_tile_scan<D>(e, sm);
  if (threadIdx.x == kOdomTile - 1) odom_put<D>(A.totals, A.ntiles, blockIdx.x, e);
}

// one wavefront: carry[tile] = totals[0] o .. o totals[tile], kOdomSweep tiles per sweep
template <int D>
__global__ __launch_bounds__(kOdomSweep) void k_odom_middle(const OdomArgs A) {
  static_assert(kOdomSweep == kWave, "the middle pass is one wavefront");
  const int lane = threadIdx.x;
  OdomEl<D> before;
  odom_head<D>(before);
  for (int base = 0; base < A.ntiles; base += kOdomSweep) {
    const int tile = base + lane;
    OdomEl<D> e;
    odom_head<D>(e);
    if (tile < A.ntiles) odom_get<D>(A.totals, A.ntiles, tile, e);
    odom_wave_scan<D>(e, lane);
    if (base > 0) odom_compose<D>(before, e);
    if (tile < A.ntiles) odom_put<D>(A.carry, A.ntiles, tile, e);
#pragma unroll
    for (int f = 0; f < D * D + D; ++f) before.v[f] = __shfl(e.v[f], kWave - 1, kWave);
    before.flag = __shfl(e.flag, kWave - 1, kWave);
  }
}

template <int D>
__global__ __launch_bounds__(kOdomTile) void k_odom_scan(const OdomArgs A) {
  __shared__ double sm[kOdomTile / kWave][D * D + D + 1];
  const int64_t pos = static_cast<int64_t>(blockIdx.x) * kOdomTile + threadIdx.x;
  OdomEl<D> e;
  odom_load<D>(A, pos, e);
  odom_tile_scan<D>(e, sm);
  if (blockIdx.x > 0) {
    OdomEl<D> before;
    odom_get<D>(A.carry, A.ntiles, static_cast<int>(blockIdx.x) - 1, before);
    odom_compose<D>(before, e);
  }
  if (pos >= A.P) return;
  // the rows of a pose (R, t): the block holds R^T, the translation row t
  double *rot = A.out + static_cast<size_t>(A.pos_rot[pos]) * D, *trn = A.out + static_cast<size_t>(A.pos_trn[pos]) * D;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) rot[a * D + b] = e.v[b * D + a];
#pragma unroll
  for (int c = 0; c < D; ++c) trn[c] = e.v[D * D + c];
  if (!odom_finite(e.v, D * D + D)) atomicOr(A.flag, 1);
}

// poses in no chain: identity block, zero translation; landmarks: the caller's rows (or zeros)
template <int D>
__global__ __launch_bounds__(256) void k_odom_fill(const OdomFillArgs A) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u < A.n_free) {
    double *rot = A.out + static_cast<size_t>(A.free_rot[u]) * D, *trn = A.out + static_cast<size_t>(A.free_trn[u]) * D;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) rot[a * D + b] = a == b ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) trn[c] = 0.0;
  } else if (u < A.n_free + A.n_lm) {
    const int64_t l = u - A.n_free;
    double *row = A.out + static_cast<size_t>(A.lm_row[l]) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) row[c] = A.lm ? A.lm[l * D + c] : 0.0;
  }
}

// range rows: one wavefront per block, the count of degenerate rows is the population of a ballot -- an integer in a
// fixed slot (summed by k_round_finish, round.inc)
template <int D>
__global__ __launch_bounds__(kWave) void k_odom_ranges(const OdomFillArgs A) {
  const int64_t m = static_cast<int64_t>(blockIdx.x) * kWave + threadIdx.x;
  bool degenerate = false;
  if (m < A.n_ranges) {
    const size_t rr = static_cast<size_t>(A.range_rows[m]), ta = static_cast<size_t>(A.range_rows[A.n_ranges + m]),
                 tb = static_cast<size_t>(A.range_rows[2 * A.n_ranges + m]);
    double row[D];
    degenerate = odom_range_row<D>(A.out + ta * D, A.out + tb * D, row);
#pragma unroll
    for (int c = 0; c < D; ++c) A.out[rr * D + c] = row[c];
    A.deg[m] = degenerate ? 1 : 0;
    if (!odom_finite(row, D)) atomicOr(A.flag, 1);
  }
  const unsigned long long votes = __ballot(degenerate);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = __popcll(votes);
}
#endif  // CORA_TU & 2
