// Part of kernels.hip (included there, in this order, inside namespace cora).  in-place update of Q's values: the check of the new values and the gather passes that refill the handle's value arrays (ValueMap, cora_internal.h) -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// update of Q's values on a live handle
// ---------------------------------------------------------------------------
// Every slot of a value array has at most one source in the CSR (sym(Q_PP): two), so a slot is written by one thread
// from one or two loads: no sums across threads, no atomics, and the bits are the ones build_format produces on the
// host.  Memory-bound: per slot a 4-byte source, an 8-byte gather and an 8-byte store.  A thread takes TWO consecutive
// slots -- one 8-byte load of sources, one 16-byte store -- so a wave-instruction stores 1 KiB contiguously; the gathers
// stay 8 bytes wide because the [slot][lane] order of the slices puts consecutive ROWS, not consecutive CSR positions,
// in consecutive lanes.  Grid: capped and grid-strided (launch.inc, grid_for).

// the new value of a slot: 0 without a source; kSourceAdd0: the entry added to +0.0 (v for every finite v but -0.0)
__device__ __forceinline__ double value_of(const double *__restrict__ vals, int32_t s) {
  if (s == kNoSource) return 0.0;
  const double v = vals[s & INT32_MAX];
  return (s < 0 && v == 0.0) ? 0.0 : v;
}

// flag |= 1: a value that is not finite;  flag |= 2: a mirror pair whose two values differ (compared as build_format
// compares them: as numbers, so +0.0 equals -0.0).  Runs before any array is written; the host reads the flag.
__global__ __launch_bounds__(256) void k_values_check(int64_t nnz, const double *__restrict__ vals, int64_t n_pairs,
                                                      const int32_t *__restrict__ mirror, int *__restrict__ flag) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  int bad = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < nnz; i += stride)
    if (!isfinite(vals[i])) bad |= 1;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; j < n_pairs; j += stride) {
    const int2 s = reinterpret_cast<const int2 *>(mirror)[j];
    const double a = s.x == kNoSource ? 0.0 : vals[s.x], b = s.y == kNoSource ? 0.0 : vals[s.y];
    if (a != b) bad |= 2;
  }
  if (bad) atomicOr(flag, bad);
}

template <bool RECIPROCAL>
__global__ __launch_bounds__(256) void k_values_gather(int64_t n, const int32_t *__restrict__ src, const double *__restrict__ vals,
                                                       double *__restrict__ dst) {
  const int64_t n2 = n >> 1, stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (int64_t i = t0; i < n2; i += stride) {
    const int2 s = reinterpret_cast<const int2 *>(src)[i];
    double2 o;
    o.x = value_of(vals, s.x);
    o.y = value_of(vals, s.y);
    if (RECIPROCAL) {
      o.x = 1.0 / o.x;
      o.y = 1.0 / o.y;
    }
    reinterpret_cast<double2 *>(dst)[i] = o;
  }
  if ((n & 1) && t0 == 0) {
    const double v = value_of(vals, src[n - 1]);
    dst[n - 1] = RECIPROCAL ? 1.0 / v : v;
  }
}

// sym(Q_PP) into the array k_point_finish reads and into S (Lambda is zero until the next point)
__global__ __launch_bounds__(256) void k_values_gather_sym(int64_t n, const int32_t *__restrict__ src, const double *__restrict__ vals,
                                                           double *__restrict__ dst0, double *__restrict__ dst1) {
  const int64_t n2 = n >> 1, stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (int64_t i = t0; i < n2; i += stride) {
    const int4 s = reinterpret_cast<const int4 *>(src)[i];
    double2 o;
    o.x = 0.5 * (value_of(vals, s.x) + value_of(vals, s.y));
    o.y = 0.5 * (value_of(vals, s.z) + value_of(vals, s.w));
    reinterpret_cast<double2 *>(dst0)[i] = o;
    reinterpret_cast<double2 *>(dst1)[i] = o;
  }
  if ((n & 1) && t0 == 0) {
    const double v = 0.5 * (value_of(vals, src[2 * (n - 1)]) + value_of(vals, src[2 * (n - 1) + 1]));
    dst0[n - 1] = v;
    dst1[n - 1] = v;
  }
}
#endif  // CORA_TU & 2
