// Part of kernels.hip (included there, in this order, inside namespace cora).  assembly of Q(w) from per-measurement weights through the term map (TermMap, cora_internal.h): weight check, short and long entries, rescale of the measurement table -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// Q(w) from a weight vector
// ---------------------------------------------------------------------------
// Every CSR entry is written by one thread (short entries) or by lane 0 of one wavefront (long entries) from a fixed
// sequence of fma's and, for long entries, one fixed tree: no atomics, and the bits are a function of the map and the
// weights alone (term_map_apply_host executes the same sequence on the host).  Memory-bound: 12 bytes per term (a
// 4-byte weight index, an 8-byte coefficient; the weights themselves stay in cache) and 4 + 8 bytes per entry.

// flag |= 1: a weight that is not finite or is negative.  Runs before anything is written; the host reads the flag.
__global__ __launch_bounds__(256) void k_weights_check(int64_t n, const double *__restrict__ w, int *__restrict__ flag) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  int bad = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    if (!(isfinite(w[i]) && w[i] >= 0.0)) bad = 1;
  if (bad) atomicOr(flag, bad);
}

// the sum of a short entry, in map order; a long entry is left to k_assemble_long, which runs afterwards (0 until then)
__device__ __forceinline__ double assemble_entry(const int32_t t0, const int32_t t1, const int32_t *__restrict__ tweight,
                                                 const double *__restrict__ tcoef, const double *__restrict__ w) {
  double acc = 0.0;
  if (t1 - t0 > kLongEntry) return acc;
  for (int32_t t = t0; t < t1; ++t) acc = fma(tcoef[t], w[tweight[t]], acc);
  return acc;
}

// A thread takes TWO consecutive entries -- one 16-byte store, 1 KiB contiguous per wave-instruction, as the gather
// kernels of update_values.inc store; `vals` is a hipMalloc'ed array (16-byte aligned), the odd last entry goes alone.
__global__ __launch_bounds__(256) void k_assemble_short(int64_t nnz, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tweight,
                                                        const double *__restrict__ tcoef, const double *__restrict__ w,
                                                        double *__restrict__ vals) {
  const int64_t n2 = nnz >> 1, stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (int64_t i = i0; i < n2; i += stride) {
    const int32_t ta = tptr[2 * i], tb = tptr[2 * i + 1], tc = tptr[2 * i + 2];
    double2 o;
    o.x = assemble_entry(ta, tb, tweight, tcoef, w);
    o.y = assemble_entry(tb, tc, tweight, tcoef, w);
    reinterpret_cast<double2 *>(vals)[i] = o;
  }
  if ((nnz & 1) && i0 == 0) vals[nnz - 1] = assemble_entry(tptr[nnz - 1], tptr[nnz], tweight, tcoef, w);
}

// One wavefront per long entry (4 per block): lane l sums terms l, l + 64, ... in order, then the lanes are added in a
// fixed tree (lane l += lane l + off for off = 32 .. 1: the lanes the entry's value depends on are l < off) and lane 0
// stores.  The term loads of a wave are contiguous (768 bytes per round).
__global__ __launch_bounds__(256) void k_assemble_long(int n_long, const int32_t *__restrict__ entries, const int32_t *__restrict__ tptr,
                                                       const int32_t *__restrict__ tweight, const double *__restrict__ tcoef,
                                                       const double *__restrict__ w, double *__restrict__ vals) {
  const int lane = threadIdx.x & (kWave - 1);
  const int waves = static_cast<int>(gridDim.x) * (256 / kWave);
  for (int j = static_cast<int>(blockIdx.x) * (256 / kWave) + (threadIdx.x / kWave); j < n_long; j += waves) {
    const int32_t q = entries[j];
    const int32_t t1 = tptr[q + 1];
    double acc = 0.0;
    for (int32_t t = tptr[q] + lane; t < t1; t += kWave) acc = fma(tcoef[t], w[tweight[t]], acc);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, kWave);
    if (lane == 0) vals[q] = acc;
  }
}

// dst[i] = base[i] * w[i]: the precision fields of the measurement table (kappa | tau contiguous in the edge data, omega
// in the range data) follow the weights
__global__ __launch_bounds__(256) void k_scale_precisions(int64_t n, const double *__restrict__ base, const double *__restrict__ w,
                                                          double *__restrict__ dst) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) dst[i] = base[i] * w[i];
}
#endif  // CORA_TU & 2
