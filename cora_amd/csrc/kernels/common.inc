// Part of kernels.hip (included there, in this order, inside namespace cora).  helpers every kernel family shares: row loads / stores, wave reductions, the chunk and list sums of the placement initialisers, the STPCG state's scalar steps.

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
// 16-byte accesses that only promise 8-byte alignment: gfx950 global loads / stores need dword alignment only, and
// the L1 / texture-address path is charged per instruction and cache line, so a 40-byte row is three accesses
// (x4, x4, x2) instead of five
struct __attribute__((aligned(8))) Pair8 { double x, y; };
#ifndef CORA_WIDE_ROWS
#define CORA_WIDE_ROWS 1
#endif

template <int LD>
__device__ __forceinline__ void load_row(const double *__restrict__ p, double (&x)[LD]) {
  if constexpr (LD % 2 == 0) {  // 16-byte aligned rows: dwordx4
    const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
    for (int j = 0; j < LD / 2; ++j) {
      const double2 t = q[j];
      x[2 * j] = t.x;
      x[2 * j + 1] = t.y;
    }
  } else if constexpr (CORA_WIDE_ROWS) {  // odd row stride: rows are only 8-byte aligned
    const Pair8 *q = reinterpret_cast<const Pair8 *>(p);
#pragma unroll
    for (int j = 0; j < LD / 2; ++j) {
      const Pair8 t = q[j];
      x[2 * j] = t.x;
      x[2 * j + 1] = t.y;
    }
    x[LD - 1] = p[LD - 1];
  } else {
#pragma unroll
    for (int j = 0; j < LD; ++j) x[j] = p[j];
  }
}

template <int LD>
__device__ __forceinline__ void store_row(double *__restrict__ p, const double (&x)[LD]) {
  if constexpr (LD % 2 == 0) {
    double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
    for (int j = 0; j < LD / 2; ++j) q[j] = make_double2(x[2 * j], x[2 * j + 1]);
  } else if constexpr (CORA_WIDE_ROWS) {
    Pair8 *q = reinterpret_cast<Pair8 *>(p);
#pragma unroll
    for (int j = 0; j < LD / 2; ++j) q[j] = Pair8{x[2 * j], x[2 * j + 1]};
    p[LD - 1] = x[LD - 1];
  } else {
#pragma unroll
    for (int j = 0; j < LD; ++j) p[j] = x[j];
  }
}

template <int LD>
__device__ __forceinline__ double dot_row(const double (&a)[LD], const double (&b)[LD]) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < LD; ++j) s = fma(a[j], b[j], s);
  return s;
}

// Q's value / index streams are read exactly once per product: mark them
// non-temporal so they do not evict the X rows the gathers re-use from L1/L2.
#ifndef CORA_STREAM_NT
#define CORA_STREAM_NT 0
#endif
#ifndef CORA_POSE_UNROLL
#define CORA_POSE_UNROLL 3
#endif
template <typename T>
__device__ __forceinline__ T stream_load(const T *p) {
#if CORA_STREAM_NT == 1
  return __builtin_nontemporal_load(p);
#elif CORA_STREAM_NT == 2  // sc1: served by L2, does not allocate in the CU's L1
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sum over a 256-thread block; result valid in thread 0. `sm` holds >= 4 doubles.
__device__ __forceinline__ double block_sum_256(double v, double *sm) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// Sum of the per-block partials of kappa = <p, Hp> by a block of 256 threads: ONE order of additions wherever it is
// formed (k_kappa_finish, every block of a fused forward sweep, the tail block of the last stage), so the same bits.
// (10^6 poses: 40 k partials on one block -- keep 32 loads per lane in flight.)
__device__ __forceinline__ double kappa_sum_256(const double *__restrict__ partial, int n, double *sm) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int b = threadIdx.x;
#pragma unroll 8
  for (; b + 768 < n; b += 1024) {
    s0 += partial[b];
    s1 += partial[b + 256];
    s2 += partial[b + 512];
    s3 += partial[b + 768];
  }
  for (; b < n; b += 256) s0 += partial[b];
  return block_sum_256((s0 + s1) + (s2 + s3), sm);
}

// ---------------------------------------------------------------------------
// the sums of the placement initialisers (multilat, placement, sighting, closure .inc), in the bracket order kernels.h
// writes down: every pass ends in chunk_sums, every fold begins with list_sums
// ---------------------------------------------------------------------------
// the butterfly: afterwards every lane holds the wavefront's sum
template <int NS>
__device__ __forceinline__ void ml_wave_sum(double *s) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + __shfl_xor(s[i], off, kWave);
}

// The end of a pass: every thread's NS terms (+0.0 without an entry) summed over the workgroup's chunk -- the butterfly per
// wavefront, the wavefronts' rows sm[w] from the left -- into partial[i * pstride + chunk].  The whole workgroup calls.
template <int NS>
__device__ __forceinline__ void chunk_sums(double (&s)[NS], double (*sm)[NS], double *partial, int64_t pstride, int64_t chunk) {
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
    for (int j = 1; j < kSumChunk / kWave; ++j) v = v + sm[j][threadIdx.x];
    partial[static_cast<size_t>(threadIdx.x) * pstride + chunk] = v;
  }
}

// The start of a fold by ONE wavefront: lane j takes 0.0 + chunk (c0 + j) + chunk (c0 + j + 64) + .. below c1 from the left,
// then the butterfly; afterwards every lane holds the NS sums of the list in s.  (Index: the width the caller counts chunks in.)
template <int NS, class Index>
__device__ __forceinline__ void list_sums(double (&s)[NS], const double *partial, int64_t pstride, Index c0, Index c1) {
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  for (Index c = c0 + static_cast<Index>(threadIdx.x); c < c1; c += kWave)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + partial[static_cast<size_t>(i) * pstride + c];
  ml_wave_sum<NS>(s);
}

// Scalar recurrences of the device-resident Steihaug-Toint PCG (StpcgState, kernels.h), run by ONE thread of the
// kernel that finished the inner product they need.
__device__ __forceinline__ void stpcg_after_kappa(StpcgState &S, double kappa) {  // after Hp = H p:  kappa = <p, Hp>
  if (S.status == 0 && S.iters >= S.max_iters) S.status = 3;
  if (S.status != 0) {
    S.coef_s = 0.0;
    S.coef_r = 0.0;
    return;
  }
  S.iters++;
  S.kappa = kappa;
  const double alpha = S.r_v / kappa;
  const double sigma_next = S.sigma_M2 + 2 * alpha * S.s_Mp + alpha * alpha * S.p_M2;
  if (!(kappa > 0.0) || sigma_next >= S.Delta2) {  // negative curvature / leaves the trust region
    S.coef_s = (-S.s_Mp + sqrt(S.s_Mp * S.s_Mp + S.p_M2 * (S.Delta2 - S.sigma_M2))) / S.p_M2;
    S.coef_r = 0.0;
    S.status = 2;
    S.step_M_norm = sqrt(S.Delta2);
  } else {
    S.alpha = alpha;
    S.coef_s = alpha;
    S.coef_r = alpha;
    S.sigma_M2 = sigma_next;
    S.step_M_norm = sqrt(sigma_next);
  }
}
// coef_r of the step above without touching the state: what a block of the fused forward sweep needs when kappa has no
// launch of its own (the same expressions, so the same bits as stpcg_after_kappa leaves in S.coef_r)
__device__ __forceinline__ double stpcg_coef_r_after_kappa(const StpcgState *__restrict__ S, double kappa) {
  if (S->status != 0 || S->iters >= S->max_iters) return 0.0;
  const double alpha = S->r_v / kappa;
  const double sigma_next = S->sigma_M2 + 2 * alpha * S->s_Mp + alpha * alpha * S->p_M2;
  return (!(kappa > 0.0) || sigma_next >= S->Delta2) ? 0.0 : alpha;
}
__device__ __forceinline__ void stpcg_after_rr(StpcgState &S, double rr) {  // after r += alpha Hp:  <r, r>
  if (S.status == 0) {
    S.rr = rr;
    if (sqrt(rr) <= S.target) S.status = 1;
  }
}
__device__ __forceinline__ void stpcg_after_rv(StpcgState &S, double rv) {  // after v = P r:  <r, v>
  if (S.status != 0) {
    S.coef_v = 0.0;
    S.coef_beta = 1.0;
    return;
  }
  const double beta = rv / S.r_v;
  S.r_v = rv;
  S.coef_v = -1.0;
  S.coef_beta = beta;
  S.s_Mp = beta * (S.s_Mp + S.alpha * S.p_M2);
  S.p_M2 = S.r_v + beta * beta * S.p_M2;
}
