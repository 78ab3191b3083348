// Part of kernels.hip (included there, in this order, inside namespace cora).  row-unit, vector, reduction, exchange and LOBPCG block kernels -- CORA_TU & 2.
#if CORA_TU & 2
// ---------------------------------------------------------------------------
// Row-unit kernels: one thread per pose (d x LD block), per range row or per
// translation row of the LOCAL shard.
// ---------------------------------------------------------------------------
struct Unit {
  int kind;      // 0 pose, 1 range, 2 translation, -1 none
  int idx;       // local index within its kind
  size_t row;    // internal row of the unit's first row
};

__device__ __forceinline__ Unit unit_of(const RowArgs &R, int64_t u) {
  Unit x;
  if (u < R.nl_poses) { x.kind = 0; x.idx = static_cast<int>(u); x.row = R.rot_base + static_cast<size_t>(u) * R.d; }
  else if (u < R.nl_poses + R.nl_ranges) { x.kind = 1; x.idx = static_cast<int>(u - R.nl_poses); x.row = R.rng_base + x.idx; }
  else if (u < R.nl_poses + R.nl_ranges + R.nl_trans) { x.kind = 2; x.idx = static_cast<int>(u - R.nl_poses - R.nl_ranges); x.row = R.trn_base + x.idx; }
  else { x.kind = -1; x.idx = 0; x.row = 0; }
  return x;
}

// After G = Q Y:  Lambda blocks (:1105-1131), grad = Proj_Y(G) (:772-780) and
// the partial sums of f = 1/2 <Y, G> (:759-762).
template <int LD, int D>
__global__ __launch_bounds__(256) void k_point_finish(const RowArgs R, const double *__restrict__ Y,
                                                      const double *__restrict__ G,
                                                      double *__restrict__ rgrad,
                                                      double *__restrict__ lam_st,
                                                      double *__restrict__ lam_ob,
                                                      const double *__restrict__ own_sym,
                                                      double *__restrict__ S,
                                                      double *__restrict__ partial) {
  __shared__ double sm[4];
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(R, u);
  double f = 0.0;
  if (un.kind == 0) {
    double y[D][LD], g[D][LD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(Y + (un.row + a) * LD, y[a]);
      load_row<LD>(G + (un.row + a) * LD, g[a]);
      f += dot_row<LD>(y[a], g[a]);
    }
    double m[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) m[a][b] = dot_row<LD>(g[a], y[b]);
    double *L = lam_st + static_cast<size_t>(un.idx) * (D * D);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const double s = 0.5 * (m[a][b] + m[b][a]);
        L[a * D + b] = s;
#pragma unroll
        for (int c = 0; c < LD; ++c) g[a][c] = fma(-s, y[b][c], g[a][c]);
      }
    // note: g[a] is updated with y only, so the in-place update above is exact
    // S_P = sym(Q_PP) - Lambda_P, the block the pose slices' epilogues read for the pose's own columns (coalesced:
    // consecutive poses are consecutive doubles of a slot)
    const size_t so = static_cast<size_t>(un.idx / kWave) * kSymEl(D) * kWave + static_cast<size_t>(un.idx % kWave);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a; b < D; ++b) {
        const size_t k = so + static_cast<size_t>(kSymSlot(a, b, D)) * kWave;
        S[k] = own_sym[k] - 0.5 * (m[a][b] + m[b][a]);
      }
#pragma unroll
    for (int a = 0; a < D; ++a) store_row<LD>(rgrad + (un.row + a) * LD, g[a]);
  } else if (un.kind == 1) {
    double y[LD], g[LD];
    load_row<LD>(Y + un.row * LD, y);
    load_row<LD>(G + un.row * LD, g);
    const double lam = dot_row<LD>(y, g);
    f += lam;
    lam_ob[un.idx] = lam;
#pragma unroll
    for (int c = 0; c < LD; ++c) g[c] = fma(-lam, y[c], g[c]);
    store_row<LD>(rgrad + un.row * LD, g);
  } else if (un.kind == 2) {
    double y[LD], g[LD];
    load_row<LD>(Y + un.row * LD, y);
    load_row<LD>(G + un.row * LD, g);
    f += dot_row<LD>(y, g);
    store_row<LD>(rgrad + un.row * LD, g);
  }
  const double tot = block_sum_256(f, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = 0.5 * tot;
}

// out = Proj_Y(scale .* V)   (scale == nullptr -> 1): tangent_space_projection
// (:782-820) and the Jacobi `precon` closure (:888-889 + src/CORA.cpp:86-92).
template <int LD, int D>
__global__ __launch_bounds__(256) void k_tangent_project(const RowArgs R, const double *__restrict__ Y,
                                                         const double *__restrict__ V,
                                                         const double *__restrict__ scale,
                                                         double *__restrict__ out) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(R, u);
  if (un.kind == 0) {
    double y[D][LD], v[D][LD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(Y + (un.row + a) * LD, y[a]);
      load_row<LD>(V + (un.row + a) * LD, v[a]);
      if (scale) {
        const double sc = scale[un.row + a - R.base];
#pragma unroll
        for (int c = 0; c < LD; ++c) v[a][c] *= sc;
      }
    }
    stiefel_project_thread<LD, D>(y, v);
#pragma unroll
    for (int a = 0; a < D; ++a) store_row<LD>(out + (un.row + a) * LD, v[a]);
  } else if (un.kind == 1) {
    double y[LD], v[LD];
    load_row<LD>(Y + un.row * LD, y);
    load_row<LD>(V + un.row * LD, v);
    if (scale) {
      const double sc = scale[un.row - R.base];
#pragma unroll
      for (int c = 0; c < LD; ++c) v[c] *= sc;
    }
    const double ip = dot_row<LD>(y, v);
#pragma unroll
    for (int c = 0; c < LD; ++c) v[c] = fma(-ip, y[c], v[c]);
    store_row<LD>(out + un.row * LD, v);
  } else if (un.kind == 2) {
    double v[LD];
    load_row<LD>(V + un.row * LD, v);
    if (scale) {
      const double sc = scale[un.row - R.base];
#pragma unroll
      for (int c = 0; c < LD; ++c) v[c] *= sc;
    }
    store_row<LD>(out + un.row * LD, v);
  }
}

// (the scale guard of the normalisations below, rescale_exponent, lives in kernels.h: the rounding and its host mirror use it too)

// Polar factor of a d x LD block by one-sided (Hestenes) Jacobi on its rows:
// rotations J with (J A) having orthogonal rows;  A = J^T Sigma U  =>  polar = J^T U.
// Works on A directly (no Gram matrix), so it is as accurate as the reference's
// Eigen::JacobiSVD route (src/StiefelProduct.cpp:8-36: U V^T of the thin SVD): within 2 x the error of a
// float64 thin SVD in units of eps * (condition number of the polar factor), at every finite non-zero scale
// (tests/test_gpu_rowops.py; measured figures in profiles/rowops.md).
// RANK-DEFICIENT blocks are NOT completed to a frame as the reference's SVD route does.  A zero row takes part in no
// rotation and is normalised to zero: a zero block returns zero, a block with one zero row returns that row zero and the
// others orthonormal.  Two identical rows cancel in their first rotation; what is left of the second direction is zero
// or the rounding residue of that cancellation, normalised -- a row without meaning.  The result is finite in every
// case (tests/test_gpu_rowops.py pins exactly this), and the other blocks of the launch are not affected.  The
// solver's iterates never get there.
template <int LD, int D>
__device__ __forceinline__ void polar_rows(double (&a)[D][LD]) {
  {  // pre-pass only: the sweeps below are the same instructions for every block
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int c = 0; c < LD; ++c) amax = fmax(amax, fabs(a[i][c]));
    const int e = rescale_exponent(amax);
    if (e != 0) {
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int c = 0; c < LD; ++c) a[i][c] = ldexp(a[i][c], e);
    }
  }
  double J[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) J[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        const double alpha = dot_row<LD>(a[p], a[p]);
        const double beta = dot_row<LD>(a[q], a[q]);
        const double gamma = dot_row<LD>(a[p], a[q]);
        const double denom = sqrt(alpha * beta);
        if (gamma != 0.0 && denom > 0.0) {
          off = fmax(off, fabs(gamma) / denom);
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
          for (int c = 0; c < LD; ++c) {
            const double x = a[p][c], y = a[q][c];
            a[p][c] = cs * x - sn * y;
            a[q][c] = sn * x + cs * y;
          }
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const double x = J[p][c], y = J[q][c];
            J[p][c] = cs * x - sn * y;
            J[q][c] = sn * x + cs * y;
          }
        }
      }
    if (off < 1e-15) break;
  }
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const double nrm = sqrt(dot_row<LD>(a[i], a[i]));
    const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
#pragma unroll
    for (int c = 0; c < LD; ++c) a[i][c] *= inv;
  }
  double o[D][LD];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int c = 0; c < LD; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(J[k][i], a[k][c], s);
      o[i][c] = s;
    }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int c = 0; c < LD; ++c) a[i][c] = o[i][c];
}

// out = projectToManifold(A + alpha V)  (V == nullptr -> projectToManifold(A)):
// Problem::projectToManifold :905-934 and Problem::retract :936-938.
template <int LD, int D>
__global__ __launch_bounds__(256) void k_project_manifold(const RowArgs R, const double *__restrict__ A,
                                                          const double *__restrict__ V, double alpha,
                                                          double *__restrict__ out) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(R, u);
  if (un.kind == 0) {
    double a[D][LD];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      load_row<LD>(A + (un.row + i) * LD, a[i]);
      if (V) {
        double v[LD];
        load_row<LD>(V + (un.row + i) * LD, v);
#pragma unroll
        for (int c = 0; c < LD; ++c) a[i][c] = fma(alpha, v[c], a[i][c]);
      }
    }
    polar_rows<LD, D>(a);
#pragma unroll
    for (int i = 0; i < D; ++i) store_row<LD>(out + (un.row + i) * LD, a[i]);
  } else if (un.kind == 1 || un.kind == 2) {
    double a[LD];
    load_row<LD>(A + un.row * LD, a);
    if (V) {
      double v[LD];
      load_row<LD>(V + un.row * LD, v);
#pragma unroll
      for (int c = 0; c < LD; ++c) a[c] = fma(alpha, v[c], a[c]);
    }
    if (un.kind == 1) {
      double amax = 0.0;
#pragma unroll
      for (int c = 0; c < LD; ++c) amax = fmax(amax, fabs(a[c]));
      const int e = rescale_exponent(amax);  // 0 for an ordinary row (and for a zero row, which stays zero)
      if (e != 0) {
#pragma unroll
        for (int c = 0; c < LD; ++c) a[c] = ldexp(a[c], e);
      }
      const double nrm = sqrt(dot_row<LD>(a, a));
      if (nrm > 0.0) {
        const double inv = 1.0 / nrm;
#pragma unroll
        for (int c = 0; c < LD; ++c) a[c] *= inv;
      }
    }
    store_row<LD>(out + un.row * LD, a);
  }
}

// ---------------------------------------------------------------------------
// flat vector kernels over the local shard (contiguous doubles)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_axpby1(int64_t n, double a, const double *__restrict__ x, double b,
                                                double *__restrict__ y) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const double yv = (b != 0.0) ? y[i] : 0.0;
    y[i] = fma(a, x[i], b * yv);
  }
}

__global__ __launch_bounds__(256) void k_axpby(int64_t n2, double a, const double2 *__restrict__ x,
                                               double b, double2 *__restrict__ y) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const double2 xv = x[i];
    double2 yv = make_double2(0.0, 0.0);
    if (b != 0.0) yv = y[i];
    y[i] = make_double2(fma(a, xv.x, b * yv.x), fma(a, xv.y, b * yv.y));
  }
}

// y1 += a1 x1 and y2 += a2 x2 in one pass (the two updates of an STPCG iteration, s += alpha p and
// r += alpha Hp): one launch floor instead of two
__global__ __launch_bounds__(256) void k_axpy2(int64_t n, double a1, const double *__restrict__ x1,
                                               double *__restrict__ y1, double a2,
                                               const double *__restrict__ x2, double *__restrict__ y2) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    y1[i] = fma(a1, x1[i], y1[i]);
    y2[i] = fma(a2, x2[i], y2[i]);
  }
}

// the two vector updates of a device-resident STPCG iteration; coefficients come from the device state
__global__ __launch_bounds__(256) void k_stpcg_update(int64_t n, const StpcgState *__restrict__ S,
                                                      const double *__restrict__ p, const double *__restrict__ Hp,
                                                      double *__restrict__ s, double *__restrict__ r) {
  const double cs = S->coef_s, cr = S->coef_r;
  if (cs == 0.0 && cr == 0.0) return;  // solve already finished: enqueued ahead of the host's check
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    s[i] = fma(cs, p[i], s[i]);
    r[i] = fma(cr, Hp[i], r[i]);
  }
}

__global__ __launch_bounds__(256) void k_stpcg_direction(int64_t n, const StpcgState *__restrict__ S,
                                                         const double *__restrict__ v, double *__restrict__ p) {
  const double cv = S->coef_v, cb = S->coef_beta;
  if (cv == 0.0 && cb == 1.0) return;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256)
    p[i] = fma(cv, v[i], cb * p[i]);
}

// x[row of API variable i][col] = a number in (-1, 1) that depends on (seed, i, col) only (splitmix64 of the triple) -- what an
// upload of a host-drawn N x k block would leave, whatever the partition: the start block of an eigensolver run, made
// where it is used (450 k x 4 doubles from the host were 3 ms to draw and 6 ms to upload)
__global__ __launch_bounds__(256) void k_fill_random(int64_t N, int ld, int k, unsigned long long seed,
                                                     const int32_t *__restrict__ api2int, double *__restrict__ x) {
  const int64_t n = N * ld;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < n; t += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t i = t / ld;
    const int col = static_cast<int>(t - i * ld);
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (static_cast<unsigned long long>(i) * 32ull + static_cast<unsigned long long>(col) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);  // [0, 1)
    x[static_cast<size_t>(api2int[i]) * ld + col] = col < k ? 2.0 * u - 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_scale_rows(int64_t rows, int ld, const double *__restrict__ scale,
                                                    const double *__restrict__ x, double *__restrict__ y) {
  const int64_t n = rows * ld;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256)
    y[i] = scale[i / ld] * x[i];
}

#endif  // CORA_TU & 2
// Tail of the inner-product kernels: every block publishes its partial sums write-through, takes a
// ticket, and the last block to arrive adds all partials in block order (deterministic) and writes the
// results to D.out -- pinned host memory, so the caller only has to wait for the stream.  Same
// inter-workgroup hand-off as the long rows of k_spmm.
__device__ __forceinline__ void dots_finish(const DotArgs &D, const double (&acc)[4], double *sm, double kappa = 0.0) {
  __shared__ int s_last;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < D.count) {
      const double t = block_sum_256(acc[j], sm);
      if (threadIdx.x == 0)
        __hip_atomic_store(D.partial + static_cast<size_t>(j) * gridDim.x + blockIdx.x, t, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(D.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (old == gridDim.x - 1);
    if (s_last) __hip_atomic_store(D.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  for (int j = 0; j < D.count; ++j) {
    double s = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += 256)
      s += __hip_atomic_load(D.partial + static_cast<size_t>(j) * gridDim.x + b, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    const double t = block_sum_256(s, sm);
    if (threadIdx.x == 0) D.out[j] = t;
    if (threadIdx.x == 0) sm[4 + j] = t;
  }
  if (threadIdx.x == 0 && D.mode == DOTS_STPCG_KAPPA) stpcg_after_kappa(*D.st, sm[4]);
  if (threadIdx.x == 0 && D.mode == DOTS_STPCG_RR) stpcg_after_rr(*D.st, sm[4]);
  if (threadIdx.x == 0 && D.mode == DOTS_STPCG_KAPPA_RR) {  // k_kappa_residual: every block used the same kappa
    stpcg_after_kappa(*D.st, kappa);
    stpcg_after_rr(*D.st, sm[4]);
  }
  if (threadIdx.x == 0 && D.mode == DOTS_STPCG_RV) {
    stpcg_after_rv(*D.st, sm[4]);
    *D.st_host = *D.st;  // pinned mirror for the host's (infrequent) look
  }
  if (threadIdx.x == 0 && D.mode == DOTS_STPCG_BETA) {
    stpcg_after_rr(*D.st, sm[4]);
    stpcg_after_rv(*D.st, sm[5]);
    *D.st_host = *D.st;
  }
  if (threadIdx.x == 0 && D.seq_out) {  // results first, then the sequence number the host spins on
    unsigned long long seq = D.seq;
    if (D.seq_counter) *D.seq_counter = seq = *D.seq_counter + 1;
    __threadfence_system();
    __hip_atomic_store(D.seq_out, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#if CORA_TU & 2
// r += coef_r Hp with <r, r> of the result in the same pass (the scalar step that follows it runs in the last block)
__global__ __launch_bounds__(256) void k_stpcg_residual(DotArgs D, const double2 *__restrict__ Hp, double2 *__restrict__ r) {
  __shared__ double sm[8];
  const double cr = D.st->coef_r;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < D.n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    double2 rv = r[i];
    if (cr != 0.0) {
      const double2 h = Hp[i];
      rv.x = fma(cr, h.x, rv.x);
      rv.y = fma(cr, h.y, rv.y);
      r[i] = rv;
    }
    acc[0] = fma(rv.x, rv.x, fma(rv.y, rv.y, acc[0]));
  }
  dots_finish(D, acc, sm);
}

// start of a solve: s = 0, r = g, p = -Pg
__global__ __launch_bounds__(256) void k_stpcg_init(int64_t n, const double *__restrict__ g, const double *__restrict__ Pg,
                                                    double *__restrict__ s, double *__restrict__ r, double *__restrict__ p) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    s[i] = 0.0;
    r[i] = g[i];
    p[i] = -Pg[i];
  }
}

// Partitioned handles: the inner products are summed over the ranks between the pass that forms them and the scalar
// step (an all-reduce of the device values on the handle's stream), so the step is a launch of its own: one thread.
//   what = 0: vals[0] = kappa;   what = 1: vals[0] = <r, r>, vals[1] = <r, v>, then the pinned mirror and its sequence number
__global__ void k_stpcg_scalar_step(int what, const double *__restrict__ vals, StpcgState *st, StpcgState *st_host,
                                    unsigned long long *seq_out, unsigned long long seq) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (what == 0) {
    stpcg_after_kappa(*st, vals[0]);
    return;
  }
  stpcg_after_rr(*st, vals[0]);
  stpcg_after_rv(*st, vals[1]);
  *st_host = *st;
  if (seq_out) {
    __threadfence_system();
    __hip_atomic_store(seq_out, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// kappa = <p, Hp> from the per-block partials of an EPI_HVP_K product, then r += coef_r Hp with <r, r> in the same
// launch: EVERY block adds the partials (same order, same bits; they sit in L2) and runs the scalar step on a private
// copy of the state to get its coefficient; the state itself is advanced once, by the last block to finish -- by then
// every block has read it.
__global__ __launch_bounds__(256) void k_kappa_residual(DotArgs D, const double *__restrict__ kpartial, int nk,
                                                        const double2 *__restrict__ Hp, double2 *__restrict__ r) {
  __shared__ double sm[8];
  __shared__ double s_kappa;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int b = threadIdx.x;
  for (; b + 768 < nk; b += 1024) {
    s0 += kpartial[b];
    s1 += kpartial[b + 256];
    s2 += kpartial[b + 512];
    s3 += kpartial[b + 768];
  }
  for (; b < nk; b += 256) s0 += kpartial[b];
  const double t = block_sum_256((s0 + s1) + (s2 + s3), sm);
  if (threadIdx.x == 0) s_kappa = t;
  __syncthreads();
  const double kappa = s_kappa;
  StpcgState L = *D.st;
  stpcg_after_kappa(L, kappa);
  const double cr = L.coef_r;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < D.n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    double2 rv = r[i];
    if (cr != 0.0) {
      const double2 h = Hp[i];
      rv.x = fma(cr, h.x, rv.x);
      rv.y = fma(cr, h.y, rv.y);
      r[i] = rv;
    }
    acc[0] = fma(rv.x, rv.x, fma(rv.y, rv.y, acc[0]));
  }
  dots_finish(D, acc, sm, kappa);
}

// The same pass for the iterations whose reductions are finished by the tail block of a later launch (RvTail::n_kappa,
// RvTail::n_rr: the one-explicit-inverse form): no ticket and no last block -- a block leaves its share of <r, r> in its
// slot and is done, the state is not touched here.  Its first elements are requested BEFORE the partials are added, so
// the launch is one round trip to memory and a block reduction, not three dependent ones.
__global__ __launch_bounds__(256) void k_kappa_residual_slots(const StpcgState *__restrict__ st, const double *__restrict__ kpartial,
                                                              int nk, int64_t n2, const double2 *__restrict__ Hp,
                                                              double2 *__restrict__ r, double *__restrict__ rr_slot) {
  __shared__ double sm[8];
  __shared__ double ksm[4];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  double2 rv = make_double2(0.0, 0.0), h = make_double2(0.0, 0.0);
  if (i < n2) {
    rv = r[i];
    h = Hp[i];
  }
  const double kappa = kappa_sum_256(kpartial, nk, ksm);
  const double cr = stpcg_coef_r_after_kappa(st, kappa);
  double acc = 0.0;
  for (; i < n2; i += stride) {
    if (cr != 0.0) {
      rv.x = fma(cr, h.x, rv.x);
      rv.y = fma(cr, h.y, rv.y);
      r[i] = rv;
    }
    acc = fma(rv.x, rv.x, fma(rv.y, rv.y, acc));
    if (i + stride < n2) {
      rv = r[i + stride];
      h = Hp[i + stride];
    }
  }
  const double t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) rr_slot[blockIdx.x] = t;
}

// s += coef_s p (the step of THIS iteration), then p = coef_v v + coef_beta p
__global__ __launch_bounds__(256) void k_stpcg_step_direction(int64_t n2, const StpcgState *__restrict__ S,
                                                              const double2 *__restrict__ v, double2 *__restrict__ p,
                                                              double2 *__restrict__ s) {
  const double cs = S->coef_s, cv = S->coef_v, cb = S->coef_beta;
  if (cs == 0.0 && cv == 0.0 && cb == 1.0) return;  // solve already finished: enqueued ahead of the host's check
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const double2 pv = p[i], vv = v[i];
    double2 sv = s[i];
    sv.x = fma(cs, pv.x, sv.x);
    sv.y = fma(cs, pv.y, sv.y);
    s[i] = sv;
    p[i] = make_double2(fma(cv, vv.x, cb * pv.x), fma(cv, vv.y, cb * pv.y));
  }
}

// v = Proj_Y(x) by row unit with <r, v> in the same pass (the preconditioned residual of an STPCG iteration: the
// scalar step that follows <r, v> runs in the last block)
template <int LD, int D>
__global__ __launch_bounds__(256) void k_tangent_project_dot(const RowArgs R, DotArgs Dt, const double *__restrict__ Y,
                                                             const double *V, const double *__restrict__ scale,
                                                             const double *__restrict__ r, double *out) {
  __shared__ double sm[8];
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(R, u);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (un.kind == 0) {
    double y[D][LD], v[D][LD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(Y + (un.row + a) * LD, y[a]);
      load_row<LD>(V + (un.row + a) * LD, v[a]);
      if (scale) {
        const double sc = scale[un.row + a - R.base];
#pragma unroll
        for (int c = 0; c < LD; ++c) v[a][c] *= sc;
      }
    }
    stiefel_project_thread<LD, D>(y, v);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(r + (un.row + a) * LD, y[a]);  // y is dead: reuse its registers for the residual rows
      acc[0] += dot_row<LD>(y[a], v[a]);
      store_row<LD>(out + (un.row + a) * LD, v[a]);
    }
  } else if (un.kind == 1 || un.kind == 2) {
    double y[LD], v[LD];
    load_row<LD>(V + un.row * LD, v);
    if (scale) {
      const double sc = scale[un.row - R.base];
#pragma unroll
      for (int c = 0; c < LD; ++c) v[c] *= sc;
    }
    if (un.kind == 1) {
      load_row<LD>(Y + un.row * LD, y);
      const double ip = dot_row<LD>(y, v);
#pragma unroll
      for (int c = 0; c < LD; ++c) v[c] = fma(-ip, y[c], v[c]);
    }
    load_row<LD>(r + un.row * LD, y);
    acc[0] = dot_row<LD>(y, v);
    store_row<LD>(out + un.row * LD, v);
  }
  dots_finish(Dt, acc, sm);
}

// v = Proj_Y(x) by row unit, consumed at once: s += coef_s p, p = coef_v v + coef_beta p (v is not stored).  The last
// pass of an STPCG iteration whose <r, v> is already known (explicit-inverse plans: <r, v> = |W r|^2 from the first
// product of the solve), so the projection needs no reduction and the step / direction pass rides on it.
template <int LD, int D>
__global__ __launch_bounds__(256) void k_tangent_project_update(const RowArgs R, const StpcgState *__restrict__ S,
                                                                const double *__restrict__ Y, const double *__restrict__ X,
                                                                double *__restrict__ p, double *__restrict__ s) {
  const double cs = S->coef_s, cv = S->coef_v, cb = S->coef_beta;
  if (cs == 0.0 && cv == 0.0 && cb == 1.0) return;  // solve already finished: enqueued ahead of the host's check
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const Unit un = unit_of(R, u);
  auto update = [&](size_t row, const double (&v)[LD]) {
    double pv[LD], sv[LD];
    load_row<LD>(p + row * LD, pv);
    load_row<LD>(s + row * LD, sv);
#pragma unroll
    for (int j = 0; j < LD; ++j) {
      sv[j] = fma(cs, pv[j], sv[j]);
      pv[j] = fma(cv, v[j], cb * pv[j]);
    }
    store_row<LD>(s + row * LD, sv);
    store_row<LD>(p + row * LD, pv);
  };
  if (un.kind == 0) {
    double y[D][LD], v[D][LD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(Y + (un.row + a) * LD, y[a]);
      load_row<LD>(X + (un.row + a) * LD, v[a]);
    }
    stiefel_project_thread<LD, D>(y, v);
#pragma unroll
    for (int a = 0; a < D; ++a) update(un.row + a, v[a]);
  } else if (un.kind == 1 || un.kind == 2) {
    double y[LD], v[LD];
    load_row<LD>(X + un.row * LD, v);
    if (un.kind == 1) {
      load_row<LD>(Y + un.row * LD, y);
      const double ip = dot_row<LD>(y, v);
#pragma unroll
      for (int c = 0; c < LD; ++c) v[c] = fma(-ip, y[c], v[c]);
    }
    update(un.row, v);
  }
}

// scalar variant for odd lengths / 8-byte aligned shards
__global__ __launch_bounds__(256) void k_dots1(DotArgs D) {
  __shared__ double sm[8];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < D.n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < D.count) acc[j] = fma(D.a[j][i], D.b[j][i], acc[j]);
  }
  dots_finish(D, acc, sm);
}

// up to 4 inner products in one pass; partial[j * gridDim.x + block]
__global__ __launch_bounds__(256) void k_dots(DotArgs D) {
  __shared__ double sm[8];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < D.n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < D.count) {
        const double2 a = reinterpret_cast<const double2 *>(D.a[j])[i];
        const double2 b = reinterpret_cast<const double2 *>(D.b[j])[i];
        acc[j] = fma(a.x, b.x, fma(a.y, b.y, acc[j]));
      }
  }
  dots_finish(D, acc, sm);
}

// <r, r> and <r, v> in one pass that reads r once (the second reduction of an STPCG iteration)
__global__ __launch_bounds__(256) void k_dots_rr_rv(DotArgs D) {
  __shared__ double sm[8];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const double2 *r = reinterpret_cast<const double2 *>(D.a[0]);
  const double2 *v = reinterpret_cast<const double2 *>(D.b[1]);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < D.n2;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const double2 a = r[i], b = v[i];
    acc[0] = fma(a.x, a.x, fma(a.y, a.y, acc[0]));
    acc[1] = fma(a.x, b.x, fma(a.y, b.y, acc[1]));
  }
  dots_finish(D, acc, sm);
}

// out[j] = sum_b partial[j * nblocks + b]   (one 256-thread block, fixed order)
__global__ __launch_bounds__(256) void k_reduce_partials(const double *__restrict__ partial, int nblocks,
                                                         int count, double *__restrict__ out) {
  __shared__ double sm[4];
  for (int j = 0; j < count; ++j) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[static_cast<size_t>(j) * nblocks + b];
    const double t = block_sum_256(s, sm);
    if (threadIdx.x == 0) out[j] = t;
  }
}

// Row moves of the multi-GPU exchange: mode 0 pack (out[k] = x[rows[k]]), 1 scatter (x[rows[k]] = in[k]),
// 2 copy (dst[rows[k]] = src[rows[k]]); one thread per double.
__global__ __launch_bounds__(256) void k_move_rows(int mode, int64_t n, int ld, const int32_t *__restrict__ rows,
                                                   const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t tot = n * ld;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot;
       t += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t k = t / ld, j = t - k * ld;
    const int64_t at = static_cast<int64_t>(rows[k]) * ld + j;
    if (mode == 0) dst[t] = src[at];
    else if (mode == 1) dst[at] = src[t];
    else dst[at] = src[at];
  }
}

// The exchange of a partitioned handle's product, both ends (capi.hip, cora_native_comm::exchange_product):
//   pack  : dst = [ the n exported rows of src | ztail zeros ] -- the zeros are the slots of the distributed long rows'
//           partial sums, which the chunk launch that follows fills where this rank has a share
//   unpack: the gathered buffers of all ranks, `stride` doubles each = [ e_max rows | n_long slots ]: rows go to
//           X[recv_idx], and the owner of long row j adds slot j of every rank IN RANK ORDER (the same bits whatever the
//           transport) into its row of the result; with kappa != nullptr every rank writes the row's kappa slot.
__global__ __launch_bounds__(256) void k_exchange_pack(int64_t n, int ld, const int32_t *__restrict__ rows, int64_t ztail,
                                                       const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t tot = n * ld;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot + ztail;
       t += static_cast<int64_t>(gridDim.x) * 256) {
    if (t >= tot) {
      dst[t] = 0.0;
      continue;
    }
    const int64_t k = t / ld, j = t - k * ld;
    dst[t] = src[static_cast<int64_t>(rows[k]) * ld + j];
  }
}
// Packed all-gather of one contiguous piece of every shard (the translation rows of the implicit formulation's solve):
// recv holds `maxn` rows per rank; rank r's piece is meta[2 r + 1] rows that belong at row  r * shard_rows + meta[2 r]  of X.
__global__ __launch_bounds__(256) void k_scatter_shard_rows(int world, int rank, int64_t maxn, int ld, int64_t shard_rows,
                                                            const int64_t *__restrict__ meta, const double *__restrict__ recv,
                                                            double *__restrict__ X) {
  const int64_t per = maxn * ld, tot = per * world;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot; t += static_cast<int64_t>(gridDim.x) * 256) {
    const int r = static_cast<int>(t / per);
    const int64_t k = t - r * per;
    if (r == rank || k >= meta[2 * r + 1] * ld) continue;
    X[(r * shard_rows + meta[2 * r]) * ld + k] = recv[t];
  }
}
__global__ __launch_bounds__(256) void k_exchange_unpack(int world, int64_t e_max, int n_long, int ld, int64_t stride, int scatter_blocks,
                                                         const int32_t *__restrict__ recv_idx, const double *__restrict__ recv,
                                                         double *__restrict__ X, int rank, const int32_t *__restrict__ long_rows,
                                                         const int32_t *__restrict__ long_owner, double *__restrict__ out,
                                                         double *__restrict__ kappa) {
  if (static_cast<int>(blockIdx.x) < scatter_blocks) {
    const int64_t per = e_max * ld, tot = per * world;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot; t += static_cast<int64_t>(scatter_blocks) * 256) {
      const int64_t r = t / per, w = t - r * per, k = t / ld, j = t - k * ld;
      X[static_cast<int64_t>(recv_idx[k]) * ld + j] = recv[r * stride + w];
    }
    return;
  }
  const int j = static_cast<int>(blockIdx.x) - scatter_blocks, lane = threadIdx.x;
  if (j >= n_long || lane >= 64) return;
  double v = 0.0, k = 0.0;
  if (lane < ld)
    for (int r = 0; r < world; ++r) v += recv[r * stride + (e_max + j) * ld + lane];
  if (long_owner[j] == rank && lane < ld) {
    const size_t at = static_cast<size_t>(long_rows[j]) * ld + lane;
    out[at] = v;
    if (kappa) k = v * X[at];   // (a landmark's own row of X is this rank's: the scatter above does not write it)
  }
  if (kappa) {
    k = wave_sum(k);
    if (lane == 0) kappa[j] = k;
  }
}

// Distributed long rows of a partitioned handle, after their partial sums have been added over the ranks: the owner of
// long row j copies slot j to its row of the result; with kappa != nullptr EVERY rank writes the row's kappa slot
// (<X[row], out[row]> on the owner, 0 elsewhere -- every slot of a launch is written).  One wavefront per row.
__global__ __launch_bounds__(64) void k_long_finish(int n_long, int ld, int rank, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ owner, const double *__restrict__ slots,
                                                    const double *__restrict__ X, double *__restrict__ out,
                                                    double *__restrict__ kappa) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= n_long) return;
  const bool mine = owner[j] == rank;
  double k = 0.0;
  if (mine && lane < ld) {
    const size_t at = static_cast<size_t>(rows[j]) * ld + lane;
    const double v = slots[static_cast<size_t>(j) * ld + lane];
    out[at] = v;
    if (kappa) k = v * X[at];
  }
  if (kappa) {
    k = wave_sum(k);
    if (lane == 0) kappa[j] = k;
  }
}

// NaN guard of Problem::precondition (:898-901): flag != 0 if any NaN.
__global__ __launch_bounds__(256) void k_has_nan(int64_t n, const double *__restrict__ x, int *flag) {
  int bad = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256)
    bad |= (x[i] != x[i]);
  if (bad) atomicOr(flag, 1);
}

// host column-major (N x k, leading dimension N) -> resident layout
__global__ __launch_bounds__(256) void k_upload(int64_t N, int k, int ld, const double *__restrict__ src,
                                                const int32_t *__restrict__ api2int,
                                                double *__restrict__ dst) {
  const int64_t tot = N * k;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot;
       t += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t c = t / N, i = t - c * N;
    dst[static_cast<size_t>(api2int[i]) * ld + c] = src[t];
  }
}

__global__ __launch_bounds__(256) void k_download(int64_t N, int k, int ld, const double *__restrict__ src,
                                                  const int32_t *__restrict__ api2int,
                                                  double *__restrict__ dst) {
  const int64_t tot = N * k;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < tot;
       t += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t c = t / N, i = t - c * N;
    dst[t] = src[static_cast<size_t>(api2int[i]) * ld + c];
  }
}

struct GramBatch {  // up to 16 products A_e^T B_e of one launch (k_gram_batch)
  const double *A[16], *B[16];
  double *partial[16];
  int lda[16], ka[16], ldb[16], kb[16];
};
// ---------------------------------------------------------------------------
// Tall-skinny block kernels for the eigensolver (LOBPCG Rayleigh-Ritz):
//   Gram:    G = A^T B            (A: rows x ka, B: rows x kb; ka, kb <= 24)
//   combine: Out = sum_i X_i C_i  (X_i: rows x k_i, C_i: k_i x kout, small, in `coef`)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void gram_block(int64_t row0, int64_t rows, const double *__restrict__ A, int lda,
                                           int ka, const double *__restrict__ B, int ldb, int kb,
                                           double *__restrict__ partial) {
  // G = A^T B over the local rows is a GEMM with a long inner dimension (the rows) and a tiny output (ka x kb <= 24 x 24):
  // v_mfma_f64_16x16x4_f64 with the rows as k.  A wavefront walks its share of the rows four at a time; lane l feeds
  // A[row + l / 16][l % 16 (+ 16 per tile)] and B likewise -- one 8-byte load each, a wavefront covers four whole rows --
  // and keeps a 16 x 16 accumulator tile (4 doubles per lane) for each of the <= 2 x 2 tiles.  The four wavefronts of a
  // block are added through LDS in wave order, blocks by k_gram_reduce in block order: deterministic.
  typedef double f64x4 __attribute__((ext_vector_type(4)));
  __shared__ double red[4][2][2][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int TA = (ka + 15) >> 4, TB = (kb + 15) >> 4;  // <= 2 each (kMaxLD = 24)
  f64x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * 4;
  const int64_t per = ((rows + nwaves - 1) / nwaves + 3) & ~static_cast<int64_t>(3);
  const int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  const int64_t r_begin = min(rows, w * per), r_end = min(rows, r_begin + per);
  const int m = lane & 15, kq = lane >> 4;
  constexpr int kUnroll = 8;
  for (int64_t r = r_begin; r < r_end; r += 4 * kUnroll) {
    double av[kUnroll][2], bv[kUnroll][2];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t row = r + 4 * u + kq;
      const bool ok = row < r_end;
      const size_t ra = static_cast<size_t>(row0 + (ok ? row : r_begin)) * lda, rb = static_cast<size_t>(row0 + (ok ? row : r_begin)) * ldb;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ca = m + 16 * t, cb = m + 16 * t;
        av[u][t] = (t < TA && ok && ca < ka) ? A[ra + ca] : 0.0;
        bv[u][t] = (t < TB && ok && cb < kb) ? B[rb + cb] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
          if (x < TA && y < TB) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][x], bv[u][y], acc[x][y], 0, 0, 0);
  }
  // C/D layout of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int g = 0; g < 4; ++g) red[wave][x][y][g * 64 + lane] = acc[x][y][g];
  __syncthreads();
  for (int x = 0; x < TA; ++x)
    for (int y = 0; y < TB; ++y) {
      const int t = threadIdx.x, g = t >> 6, l = t & 63;
      const int i = 16 * x + (l >> 4) + 4 * g, j = 16 * y + (l & 15);
      if (i < ka && j < kb) {
        const double sum = ((red[0][x][y][t] + red[1][x][y][t]) + red[2][x][y][t]) + red[3][x][y][t];
        partial[static_cast<size_t>(i * kb + j) * gridDim.x + blockIdx.x] = sum;
      }
    }
}
__global__ __launch_bounds__(256) void k_gram(int64_t row0, int64_t rows, const double *__restrict__ A, int lda,
                                              int ka, const double *__restrict__ B, int ldb, int kb,
                                              double *__restrict__ partial) {
  gram_block(row0, rows, A, lda, ka, B, ldb, kb, partial);
}
// Up to 16 Gram products in ONE launch (blockIdx.y = product; blockIdx.x / gridDim.x as in k_gram: the same partial sums,
// the same bits): the twelve blocks of a Rayleigh-Ritz step were 24 launches of a few microseconds each.
__global__ __launch_bounds__(256) void k_gram_batch(int64_t row0, int64_t rows, const GramBatch G) {
  const int e = blockIdx.y;
  gram_block(row0, rows, G.A[e], G.lda[e], G.ka[e], G.B[e], G.ldb[e], G.kb[e], G.partial[e]);
}

// out[el] = sum over blocks of partial[el][block]: one block per element, fixed order
__global__ __launch_bounds__(256) void k_gram_reduce(const double *__restrict__ partial, int nblocks, int nel,
                                                     double *__restrict__ out) {
  __shared__ double sm[4];
  const int el = blockIdx.x;
  if (el >= nel) return;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[static_cast<size_t>(el) * nblocks + b];
  const double t = block_sum_256(s, sm);
  if (threadIdx.x == 0) out[el] = t;
}

struct CombineCoef {  // coefficient matrices passed by value (k_combine_karg)
  static constexpr int kMax = 400;
  double v[kMax];
};
struct CombineArgs {
  const double *x[4];
  int kx[4], ldx[4], coff[4];  // coff: offset of C_i in coef (row-major k_i x kout)
  int nblocks, kout, ldo;
};

template <bool KARG>
__device__ __forceinline__ void combine_block(int64_t row0, int64_t rows, const CombineArgs &A,
                                              const double *__restrict__ coef, const CombineCoef *K, int ncoef,
                                              double *__restrict__ out) {
  // Out = sum_b X_b C_b, 16 rows per wavefront and step, on v_mfma_f64_16x16x4_f64: the rows are the M dimension
  // (lane l feeds X[row + l % 16][4 s + l / 16]), the coefficient matrices the B operand (from LDS, zero padded), the
  // <= 2 column tiles of the output sit in 4 doubles per lane each: D[row = (l >> 4) + 4 reg][col = l & 15], so one
  // store instruction writes four whole consecutive rows.
  typedef double f64x4 __attribute__((ext_vector_type(4)));
  extern __shared__ double sc[];
  for (int t = threadIdx.x; t < ncoef; t += 256) sc[t] = KARG ? K->v[t] : coef[t];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int m = lane & 15, kq = lane >> 4;
  const int TO = (A.kout + 15) >> 4;  // column tiles of the output (<= 2)
  const int64_t groups = (rows + 15) >> 4, nw = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t gidx = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); gidx < groups; gidx += nw) {
    const int64_t r = gidx << 4;
    const bool rok = r + m < rows;
    f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
    for (int b = 0; b < A.nblocks; ++b) {
      const double *__restrict__ xr = A.x[b] + static_cast<size_t>(row0 + (rok ? r + m : r)) * A.ldx[b];
      const double *__restrict__ C = sc + A.coff[b];
      const int kx = A.kx[b];
      double xv[6];
#pragma unroll
      for (int st = 0; st < 6; ++st) {
        const int col = 4 * st + kq;
        xv[st] = (4 * st < kx && rok && col < kx) ? xr[col] : 0.0;
      }
#pragma unroll
      for (int st = 0; st < 6; ++st)
        if (4 * st < kx) {  // wave-uniform
          const int col = 4 * st + kq;
#pragma unroll
          for (int y = 0; y < 2; ++y)
            if (y < TO) {
              const int j = 16 * y + m;
              const double cv = (col < kx && j < A.kout) ? C[col * A.kout + j] : 0.0;
              acc[y] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[st], cv, acc[y], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int y = 0; y < 2; ++y)
      if (y < TO) {
        const int j = 16 * y + m;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t row = r + kq + 4 * g;
          if (row < rows && j < A.ldo) out[static_cast<size_t>(row0 + row) * A.ldo + j] = j < A.kout ? acc[y][g] : 0.0;
        }
      }
    if (A.ldo > 16 * TO) {  // padding columns beyond the last tile (row stride 20 / 24 with kout <= 16)
      for (int j = 16 * TO + m; j < A.ldo; j += 16)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t row = r + kq + 4 * g;
          if (row < rows) out[static_cast<size_t>(row0 + row) * A.ldo + j] = 0.0;
        }
    }
  }
}
__global__ __launch_bounds__(256) void k_combine(int64_t row0, int64_t rows, CombineArgs A,
                                                 const double *__restrict__ coef, int ncoef,
                                                 double *__restrict__ out) {
  combine_block<false>(row0, rows, A, coef, nullptr, ncoef, out);
}
// The coefficient matrices in the kernel's own arguments (up to CombineCoef::kMax doubles: every Rayleigh-Ritz step of the
// eigensolver): no copy to the device and no wait for it in front of the launch.
__global__ __launch_bounds__(256) void k_combine_karg(int64_t row0, int64_t rows, CombineArgs A, const CombineCoef K, int ncoef,
                                                      double *__restrict__ out) {
  combine_block<true>(row0, rows, A, nullptr, &K, ncoef, out);
}

#endif  // CORA_TU & 2
