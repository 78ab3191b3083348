// Part of kernels.hip (included there, in this order, inside namespace cora).  rounding of a resident vector to SE(d): count of the pose blocks of positive determinant, its finish, the per-unit pass (RoundArgs, kernels.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// rounding to SE(d)
// ---------------------------------------------------------------------------
// One thread per unit (unit_of, rows.inc), as in k_project_manifold.  The arithmetic of a unit is round_pose / round_row and their parts
// (kernels.h), the same functions the host mirror calls: a unit's output is a function of its rows, the basis and the flip
// alone.  The basis sits in the kernel arguments (RoundArgs::vd, vd_dir): the loop over the k columns reads it through
// scalar loads at a uniform index, a thread holds D accumulators per row and never a whole k-wide row.  Templates on D
// only; k and the row stride are loop bounds.  The apply pass forms Y Vd AGAIN instead of finishing products the count
// pass stored: the product is k fma per entry against 8 bytes of traffic, the output is written exactly once, and no
// pass reads what another wrote except the two words of the finish.

// partial[blockIdx.x] = number of the block's poses with det(Y_i Vd) > 0: one wavefront per block, the count is the
// population of a ballot -- an integer in a fixed slot
template <int D>
__global__ __launch_bounds__(kRoundCountBlock) void k_round_count(const RoundArgs A) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kRoundCountBlock + threadIdx.x;
  bool positive = false;
  if (u < A.R.nl_poses) {
    const double *row = A.Y + (A.R.rot_base + static_cast<size_t>(u) * D) * A.ldy;
    double m[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i) round_product<D>(row + static_cast<size_t>(i) * A.ldy, A.k, A.vd_dir, m[i]);
    positive = round_det_positive<D>(m);
  }
  const unsigned long long votes = __ballot(positive);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = __popcll(votes);
}

// words[0] = sum of the partials, words[1] = 1 when it is below n / 2 (integer division): one wavefront, rounds of 64
__global__ __launch_bounds__(64) void k_round_finish(const int *__restrict__ partial, int nblocks, int n, int *__restrict__ words) {
  int s = 0;
  for (int b = threadIdx.x; b < nblocks; b += 64) s += partial[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) {
    words[0] = s;
    words[1] = s < n / 2 ? 1 : 0;
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_round_apply(const RoundArgs A) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(A.R, u);
  if (un.kind < 0) return;
  const bool flip = A.words[1] != 0;
  const double *row = A.Y + un.row * A.ldy;
  double *out = A.out + un.row * D;  // (the output's stride is ld_for(D) = D)
  bool finite;
  if (un.kind == 0) {
    double m[D][D];
    finite = round_pose<D>(row, A.ldy, A.k, A.vd_dir, flip, m);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int c = 0; c < D; ++c) out[i * D + c] = m[i][c];
  } else {
    double m[D];
    finite = un.kind == 1 ? round_row<D>(true, row, A.k, A.vd_dir, flip, m) : round_row<D>(false, row, A.k, A.vd, flip, m);
#pragma unroll
    for (int c = 0; c < D; ++c) out[c] = m[c];
  }
  if (!finite) atomicOr(A.flag, 1);
}

// the rare path (an input whose Gram matrix leaves the range): the largest |entry| and whether every entry is finite
__global__ __launch_bounds__(256) void k_round_amax(int64_t n, const double *__restrict__ y, double *__restrict__ partial,
                                                    int *flag) {
  __shared__ double sm[4];
  double amax = 0.0;
  bool bad = false;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    const double v = fabs(y[i]);
    bad = bad || !(v <= 1.79769313486231570815e308);
    amax = fmax(amax, v);
  }
  if (bad) atomicOr(flag, 1);
  const double t = block_max_256(amax, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void k_round_scale(int64_t n, const double *__restrict__ y, int e, double *__restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
    out[i] = ldexp(y[i], e);
}
#endif  // CORA_TU & 2
