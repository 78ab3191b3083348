// Part of kernels.hip (included there, in this order, inside namespace cora).  host-side launch wrappers (kernels.h), per translation unit and row-stride group.
// Which instantiation a runtime d, row stride, piece width, switch or mode selects is decided by the helpers of dispatch.h.
// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static inline int grid_for(int64_t n, int per_block = 256, int cap = 2048) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return static_cast<int>(g);
}

// e = run(LD) for a stride of the row-stride group G (kLdGroups, dispatch.h) of a family (SpMM, staged solves); refused outside.
// Each group's launcher is defined in the translation unit that instantiates the group's kernels (CORA_LDG bit G).
template <int G, class Run>
static hipError_t in_ld_group(int ld, Run run) {
  hipError_t e = hipErrorInvalidValue;
  for_ld<kLdGroups[G].first, kLdGroups[G].last>(ld, [&](auto LD) { e = run(LD); });
  return e;
}

#if CORA_TU & 1
template <int LD, int D>
static hipError_t launch_spmm_ld(const SpmmArgs &A_in, int epi, hipStream_t st) {
  SpmmArgs A = A_in;
  if (LD <= kPoseFirstMaxLD && A.slices_pose_first) A.slices = A.slices_pose_first;
  A.win_on = A.n_slices >= g_win_min_slices ? 1 : 0;
  A.stagger_ticks = spmm_stagger_ticks_for(A, LD, epi);
  A.n_real_chunks = A.n_chunks;
  A.n_chunks = (A.n_chunks + 7) & ~7;
  A.n_slice_blocks = A.n_slices;
  const int grid = A.n_chunks + 8 * ((A.n_slices + 7) / 8);
  A.kappa_long_base = grid;  // = launch_spmm_blocks(A_in): the long rows' own slots follow the per-block ones
  if (A.n_real_chunks + A.n_slices == 0) return hipSuccess;
  switch (epi) {
    case EPI_NONE: hipLaunchKernelGGL((k_spmm<LD, D, EPI_NONE>), dim3(grid), dim3(64), 0, st, A); break;
    case EPI_S: hipLaunchKernelGGL((k_spmm<LD, D, EPI_S>), dim3(grid), dim3(64), 0, st, A); break;
    case EPI_HVP_K:
      if (!A.kappa_partial) return hipErrorInvalidValue;
      hipLaunchKernelGGL((k_spmm<LD, D, EPI_HVP_K>), dim3(grid), dim3(64), 0, st, A);
      break;
    default: hipLaunchKernelGGL((k_spmm<LD, D, EPI_HVP>), dim3(grid), dim3(64), 0, st, A); break;
  }
  return hipGetLastError();
}

// one launcher per row-stride group, each in the translation unit that instantiates the group's kernels
template <int G>
static hipError_t spmm_group(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) {
  return in_ld_group<G>(ld, [&](auto LD) { return for_d(d, [&](auto D) { return launch_spmm_ld<LD(), D()>(A, epi, st); }); });
}
using SpmmGroupFn = hipError_t(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st);
SpmmGroupFn launch_spmm_g0, launch_spmm_g1, launch_spmm_g2, launch_spmm_g3, launch_spmm_g4, launch_spmm_g5;
#if CORA_LDG & 1
// slices from which the pose slices read X through their LDS windows (kWinMinSlices; CORA_SPMM_WINDOW_MIN_SLICES or
// cora_debug_spmm_window_min_slices: the tests run the window form of every row stride on small problems)
int g_win_min_slices = static_cast<int>(env_int(Env::SpmmWindowMinSlices));
// delay of the pose slices' second cohort (kernels.h, spmm_stagger_ticks_for; CORA_SPMM_STAGGER_TICKS or
// cora_debug_spmm_stagger_ticks), and the tests' switch that applies it whatever the size and the row stride
int g_spmm_stagger_ticks = spmm_stagger_clamp(env_int(Env::SpmmStaggerTicks));
int g_spmm_stagger_force = 0;
hipError_t launch_spmm_g0(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<0>(A, ld, d, epi, st); }
hipError_t launch_spmm(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) {
  SpmmGroupFn *const group[kNumLdGroups] = {launch_spmm_g0, launch_spmm_g1, launch_spmm_g2, launch_spmm_g3, launch_spmm_g4, launch_spmm_g5};
  const int g = ld_group_of(ld);
  return g < kNumLdGroups ? group[g](A, ld, d, epi, st) : hipErrorInvalidValue;
}
#endif
#if CORA_LDG & 2
hipError_t launch_spmm_g1(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<1>(A, ld, d, epi, st); }
#endif
#if CORA_LDG & 4
hipError_t launch_spmm_g2(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<2>(A, ld, d, epi, st); }
#endif
#if CORA_LDG & 8
hipError_t launch_spmm_g3(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<3>(A, ld, d, epi, st); }
#endif
#if CORA_LDG & 16
hipError_t launch_spmm_g4(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<4>(A, ld, d, epi, st); }
#endif
#if CORA_LDG & 32
hipError_t launch_spmm_g5(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st) { return spmm_group<5>(A, ld, d, epi, st); }
#endif
#endif  // CORA_TU & 1

#if CORA_TU & 2

// the grid of a row-unit kernel: 256 units (poses, range rows, translation rows) per block
static inline int row_unit_blocks(const RowArgs &R) {
  const int64_t units = static_cast<int64_t>(R.nl_poses) + R.nl_ranges + R.nl_trans;
  return static_cast<int>((units + 255) / 256);
}
// launch(LD, D) of a row-unit kernel instantiated for the strides LO..HI; a stride outside is refused
template <int LO, int HI, class Launch>
static hipError_t launch_row_units(const RowArgs &R, int ld, Launch launch) {
  const bool known = for_ld<LO, HI>(ld, [&](auto LD) { for_d(R.d, [&](auto D) { launch(LD, D); }); });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_point_finish(const RowArgs &R, int ld, const double *Y, const double *G,
                               double *rgrad, double *lam_st, double *lam_ob, const double *own_sym, double *S,
                               double *partial, int *nblocks, hipStream_t st) {
  const int grid = row_unit_blocks(R);
  *nblocks = grid;
  if (grid == 0) return hipSuccess;
  return launch_row_units<2, kMaxLD>(R, ld, [&](auto LD, auto D) {
    hipLaunchKernelGGL((k_point_finish<LD(), D()>), dim3(grid), dim3(256), 0, st, R, Y, G, rgrad, lam_st, lam_ob, own_sym, S, partial);
  });
}

hipError_t launch_tangent_project(const RowArgs &R, int ld, const double *Y, const double *V,
                                  const double *scale, double *out, hipStream_t st) {
  const int grid = row_unit_blocks(R);
  if (grid == 0) return hipSuccess;
  return launch_row_units<2, kMaxLD>(R, ld, [&](auto LD, auto D) {
    hipLaunchKernelGGL((k_tangent_project<LD(), D()>), dim3(grid), dim3(256), 0, st, R, Y, V, scale, out);
  });
}

hipError_t launch_project_manifold(const RowArgs &R, int ld, const double *A, const double *V,
                                   double alpha, double *out, hipStream_t st) {
  const int grid = row_unit_blocks(R);
  if (grid == 0) return hipSuccess;
  return launch_row_units<2, kMaxLD>(R, ld, [&](auto LD, auto D) {
    hipLaunchKernelGGL((k_project_manifold<LD(), D()>), dim3(grid), dim3(256), 0, st, R, A, V, alpha, out);
  });
}

// n doubles as n / 2 double2: an even count and every pointer 16-byte aligned
template <class... P>
static inline bool vec2_ok(int64_t n, const P *...p) {
  return n % 2 == 0 && ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}

hipError_t launch_axpby(int64_t n, double a, const double *x, double b, double *y, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (vec2_ok(n, x, y))
    hipLaunchKernelGGL(k_axpby, dim3(grid_for(n / 2)), dim3(256), 0, st, n / 2, a,
                       reinterpret_cast<const double2 *>(x), b, reinterpret_cast<double2 *>(y));
  else
    hipLaunchKernelGGL(k_axpby1, dim3(grid_for(n)), dim3(256), 0, st, n, a, x, b, y);
  return hipGetLastError();
}

hipError_t launch_axpy2(int64_t n, double a1, const double *x1, double *y1, double a2, const double *x2,
                        double *y2, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_axpy2, dim3(grid_for(n)), dim3(256), 0, st, n, a1, x1, y1, a2, x2, y2);
  return hipGetLastError();
}

hipError_t launch_stpcg_update(int64_t n, const StpcgState *S, const double *p, const double *Hp, double *s,
                               double *r, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stpcg_update, dim3(grid_for(n)), dim3(256), 0, st, n, S, p, Hp, s, r);
  return hipGetLastError();
}

hipError_t launch_stpcg_direction(int64_t n, const StpcgState *S, const double *v, double *p, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stpcg_direction, dim3(grid_for(n)), dim3(256), 0, st, n, S, v, p);
  return hipGetLastError();
}

// D: mode / st / st_host / partial / ticket / seq fields set by the caller; n doubles, even, 16-byte aligned
hipError_t launch_kappa_residual(const DotArgs &D_in, const double *kpartial, int nk, int64_t n, const double *Hp, double *r,
                                 hipStream_t st) {
  if (n <= 0 || !vec2_ok(n, Hp, r)) return hipErrorInvalidValue;
  DotArgs D = D_in;
  D.count = 1;
  D.n2 = n / 2;
  D.mode = DOTS_STPCG_KAPPA_RR;
  hipLaunchKernelGGL(k_kappa_residual, dim3(grid_for(n / 2, 256, 256)), dim3(256), 0, st, D, kpartial, nk,
                     reinterpret_cast<const double2 *>(Hp), reinterpret_cast<double2 *>(r));
  return hipGetLastError();
}
int kappa_residual_slots_blocks(int64_t n) { return grid_for(n / 2, 256, 256); }
// rr_slot: kappa_residual_slots_blocks(n) doubles, one per block of the launch (added by an RvTail block)
hipError_t launch_kappa_residual_slots(const StpcgState *S, const double *kpartial, int nk, int64_t n, const double *Hp, double *r,
                                       double *rr_slot, hipStream_t st) {
  if (n <= 0 || !vec2_ok(n, Hp, r)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_kappa_residual_slots, dim3(kappa_residual_slots_blocks(n)), dim3(256), 0, st, S, kpartial, nk, n / 2,
                     reinterpret_cast<const double2 *>(Hp), reinterpret_cast<double2 *>(r), rr_slot);
  return hipGetLastError();
}
// D: mode / st / st_host / partial / ticket / seq fields set by the caller; n doubles, even, 16-byte aligned
hipError_t launch_stpcg_residual(const DotArgs &D_in, int64_t n, const double *Hp, double *r, hipStream_t st) {
  if (n <= 0 || !vec2_ok(n, Hp, r)) return hipErrorInvalidValue;
  DotArgs D = D_in;
  D.count = 1;
  D.n2 = n / 2;
  hipLaunchKernelGGL(k_stpcg_residual, dim3(grid_for(n / 2, 256, 256)), dim3(256), 0, st, D, reinterpret_cast<const double2 *>(Hp),
                     reinterpret_cast<double2 *>(r));
  return hipGetLastError();
}

hipError_t launch_stpcg_scalar_step(int what, const double *vals, StpcgState *state, StpcgState *state_host,
                                    unsigned long long *seq_out, unsigned long long seq, hipStream_t st) {
  hipLaunchKernelGGL(k_stpcg_scalar_step, dim3(1), dim3(64), 0, st, what, vals, state, state_host, seq_out, seq);
  return hipGetLastError();
}
hipError_t launch_stpcg_init(int64_t n, const double *g, const double *Pg, double *s, double *r, double *p, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stpcg_init, dim3(grid_for(n)), dim3(256), 0, st, n, g, Pg, s, r, p);
  return hipGetLastError();
}
hipError_t launch_stpcg_step_direction(int64_t n, const StpcgState *S, const double *v, double *p, double *s,
                                       hipStream_t st) {
  if (n <= 0 || !vec2_ok(n, v, p, s)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stpcg_step_direction, dim3(grid_for(n / 2)), dim3(256), 0, st, n / 2, S,
                     reinterpret_cast<const double2 *>(v), reinterpret_cast<double2 *>(p), reinterpret_cast<double2 *>(s));
  return hipGetLastError();
}

hipError_t launch_tangent_project_update(const RowArgs &R, const StpcgState *S, int ld, const double *Y, const double *X,
                                         double *p, double *s, hipStream_t st) {
  const int grid = row_unit_blocks(R);
  if (grid == 0) return hipErrorInvalidValue;
  return launch_row_units<2, 12>(R, ld, [&](auto LD, auto D) {  // (the fused iteration's strides)
    hipLaunchKernelGGL((k_tangent_project_update<LD(), D()>), dim3(grid), dim3(256), 0, st, R, S, Y, X, p, s);
  });
}

// out = Proj_Y(V) and <r, out>; the partial array of D needs one slot per 256 row units
hipError_t launch_tangent_project_dot(const RowArgs &R, const DotArgs &D_in, int ld, const double *Y, const double *V,
                                      const double *scale, const double *r, double *out, hipStream_t st) {
  const int grid = row_unit_blocks(R);
  if (grid == 0) return hipErrorInvalidValue;
  DotArgs Dot = D_in;
  Dot.count = 1;
  return launch_row_units<2, 12>(R, ld, [&](auto LD, auto D) {  // (the fused iteration's strides)
    hipLaunchKernelGGL((k_tangent_project_dot<LD(), D()>), dim3(grid), dim3(256), 0, st, R, Dot, Y, V, scale, r, out);
  });
}

hipError_t launch_scale_rows(int64_t rows, int ld, const double *scale, const double *x, double *y,
                             hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scale_rows, dim3(grid_for(rows * ld)), dim3(256), 0, st, rows, ld, scale, x, y);
  return hipGetLastError();
}

// D.n2 holds the number of DOUBLES; the vectorised kernel is used when everything is 16-byte aligned
hipError_t launch_dots(const DotArgs &D_in, int *nblocks, hipStream_t st) {
  DotArgs D = D_in;
  bool vec = (D.n2 % 2 == 0);
  for (int j = 0; j < D.count; ++j)
    vec = vec && reinterpret_cast<uintptr_t>(D.a[j]) % 16 == 0 && reinterpret_cast<uintptr_t>(D.b[j]) % 16 == 0;
  if (vec) D.n2 /= 2;
  const int grid = grid_for(D.n2, 256, 256);  // one block per CU: 128 / 256 / 512 / 1024 blocks measured 24.0 / 16.8 / 19.0 / 24.7 us per inner product
  *nblocks = grid;
  if (vec && D.count == 2 && D.a[0] == D.b[0] && D.a[1] == D.a[0])
    hipLaunchKernelGGL(k_dots_rr_rv, dim3(grid), dim3(256), 0, st, D);
  else if (vec) hipLaunchKernelGGL(k_dots, dim3(grid), dim3(256), 0, st, D);
  else hipLaunchKernelGGL(k_dots1, dim3(grid), dim3(256), 0, st, D);
  return hipGetLastError();
}

hipError_t launch_reduce_partials(const double *partial, int nblocks, int count, double *out,
                                  hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, partial, nblocks, count, out);
  return hipGetLastError();
}

hipError_t launch_move_rows(int mode, int64_t n, int ld, const int32_t *rows, const double *src, double *dst,
                            hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_move_rows, dim3(grid_for(n * ld)), dim3(256), 0, st, mode, n, ld, rows, src, dst);
  return hipGetLastError();
}

hipError_t launch_exchange_pack(int64_t n, int ld, const int32_t *rows, int64_t ztail, const double *src, double *dst, hipStream_t st) {
  if (n * ld + ztail <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_exchange_pack, dim3(grid_for(n * ld + ztail)), dim3(256), 0, st, n, ld, rows, ztail, src, dst);
  return hipGetLastError();
}
hipError_t launch_scatter_shard_rows(int world, int rank, int64_t maxn, int ld, int64_t shard_rows, const int64_t *meta,
                                     const double *recv, double *X, hipStream_t st) {
  if (maxn * ld * world <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scatter_shard_rows, dim3(grid_for(maxn * ld * world)), dim3(256), 0, st, world, rank, maxn, ld, shard_rows, meta, recv, X);
  return hipGetLastError();
}
hipError_t launch_exchange_unpack(int world, int64_t e_max, int n_long, int ld, const int32_t *recv_idx, const double *recv, double *X,
                                  int rank, const int32_t *long_rows, const int32_t *long_owner, double *out, double *kappa,
                                  hipStream_t st) {
  const int sb = grid_for(static_cast<int64_t>(world) * e_max * ld);
  hipLaunchKernelGGL(k_exchange_unpack, dim3(sb + n_long), dim3(256), 0, st, world, e_max, n_long, ld,
                     (e_max + n_long) * static_cast<int64_t>(ld), sb, recv_idx, recv, X, rank, long_rows, long_owner, out, kappa);
  return hipGetLastError();
}

hipError_t launch_long_finish(int n_long, int ld, int rank, const int32_t *rows, const int32_t *owner, const double *slots,
                              const double *X, double *out, double *kappa, hipStream_t st) {
  if (n_long <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_long_finish, dim3(n_long), dim3(64), 0, st, n_long, ld, rank, rows, owner, slots, X, out, kappa);
  return hipGetLastError();
}

hipError_t launch_has_nan(int64_t n, const double *x, int *flag, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_has_nan, dim3(grid_for(n)), dim3(256), 0, st, n, x, flag);
  return hipGetLastError();
}

hipError_t launch_upload(int64_t N, int k, int ld, const double *src, const int32_t *api2int,
                         double *dst, hipStream_t st) {
  if (N * k <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_upload, dim3(grid_for(N * k)), dim3(256), 0, st, N, k, ld, src, api2int, dst);
  return hipGetLastError();
}

hipError_t launch_download(int64_t N, int k, int ld, const double *src, const int32_t *api2int,
                           double *dst, hipStream_t st) {
  if (N * k <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_download, dim3(grid_for(N * k)), dim3(256), 0, st, N, k, ld, src, api2int, dst);
  return hipGetLastError();
}

// per-measurement residuals (kernels/residuals.inc): 16-byte pieces of a row where the stride is even, 8-byte otherwise
hipError_t launch_edge_residuals(const ResidualArgs &A, hipStream_t st) {
  if (A.n <= 0) return hipSuccess;
  if ((A.d != 2 && A.d != 3) || A.k < 1 || A.k > A.ld) return hipErrorInvalidValue;
  const dim3 grid(residual_blocks(A.n)), block(256);
  for_d(A.d, [&](auto D) { for_width(A.ld, [&](auto W) { hipLaunchKernelGGL((k_edge_residuals<D(), W()>), grid, block, 0, st, A); }); });
  return hipGetLastError();
}

hipError_t launch_range_residuals(const ResidualArgs &A, hipStream_t st) {
  if (A.n <= 0) return hipSuccess;
  if (A.k < 1 || A.k > A.ld) return hipErrorInvalidValue;
  const dim3 grid(residual_blocks(A.n)), block(256);
  for_width(A.ld, [&](auto W) { hipLaunchKernelGGL((k_range_residuals<W()>), grid, block, 0, st, A); });
  return hipGetLastError();
}

// the GNC weight step (kernels/gnc.inc): the residual kernels' grid and piece width
hipError_t launch_gnc_edges(const GncArgs &A, hipStream_t st) {
  const ResidualArgs &R = A.R;
  if (R.n <= 0) return hipSuccess;
  if ((R.d != 2 && R.d != 3) || R.k < 1 || R.k > R.ld) return hipErrorInvalidValue;
  const dim3 grid(residual_blocks(R.n)), block(256);
  for_d(R.d, [&](auto D) { for_width(R.ld, [&](auto W) { hipLaunchKernelGGL((k_gnc_edges<D(), W()>), grid, block, 0, st, A); }); });
  return hipGetLastError();
}

hipError_t launch_gnc_ranges(const GncArgs &A, hipStream_t st) {
  const ResidualArgs &R = A.R;
  if (R.n <= 0) return hipSuccess;
  if (R.k < 1 || R.k > R.ld) return hipErrorInvalidValue;
  const dim3 grid(residual_blocks(R.n)), block(256);
  for_width(R.ld, [&](auto W) { hipLaunchKernelGGL((k_gnc_ranges<W()>), grid, block, 0, st, A); });
  return hipGetLastError();
}

hipError_t launch_reduce_max_partials(const double *partial, int nblocks, int count, double *out, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_max_partials, dim3(1), dim3(256), 0, st, partial, nblocks, count, out);
  return hipGetLastError();
}

// the trajectory comparison (kernels/compare.inc): grids sized by the count, piece widths by the parity of the two strides
static bool compare_args_ok(const CompareArgs &A) {
  return (A.d == 2 || A.d == 3) && A.k >= 1 && A.k <= A.ldx && A.kr >= 1 && A.kr <= A.ldr && A.k <= kMaxLD && A.kr <= A.k &&
         A.n >= 0 && A.nt >= A.n && A.nr >= 0;
}
// f(WX, WR): the piece widths of the strides of X and of the reference
template <class Args, class F>
static void for_widths(const Args &A, F f) {
  for_width(A.ldx, [&](auto WX) { for_width(A.ldr, [&](auto WR) { f(WX, WR); }); });
}
hipError_t launch_compare_sums(const CompareArgs &A, hipStream_t st) {
  if (!compare_args_ok(A) || A.n < 1) return hipErrorInvalidValue;
  const dim3 grid(compare_blocks(A.n)), block(256);
  for_widths(A, [&](auto WX, auto WR) { hipLaunchKernelGGL((k_compare_sums<WX(), WR()>), grid, block, 0, st, A); });
  return hipGetLastError();
}
hipError_t launch_compare_centre(const CompareArgs &A, hipStream_t st) {
  if (!compare_args_ok(A) || A.n < 1) return hipErrorInvalidValue;
  const dim3 grid(compare_blocks(A.n)), block(256);
  for_widths(A, [&](auto WX, auto WR) { hipLaunchKernelGGL((k_compare_centre<WX(), WR()>), grid, block, 0, st, A); });
  return hipGetLastError();
}
hipError_t launch_compare_errors(const CompareArgs &A, hipStream_t st) {
  if (!compare_args_ok(A) || A.nt < 1) return hipErrorInvalidValue;
  const dim3 grid(compare_blocks(static_cast<int64_t>(A.nt) + (A.aligned ? A.nr : 0))), block(256);
  for_d(A.d, [&](auto D) { for_width(A.ldr, [&](auto WR) { hipLaunchKernelGGL((k_compare_errors<D(), WR()>), grid, block, 0, st, A); }); });
  return hipGetLastError();
}

// the relative pose error (kernels/rpe.inc): grid sized by the count, piece widths by the parity of the two strides
hipError_t launch_rpe(const RpeArgs &A, hipStream_t st) {
  if ((A.d != 2 && A.d != 3) || A.k < 1 || A.k > A.ldx || A.kr < 1 || A.kr > A.ldr || A.ldx > kMaxLD || A.ldr > kMaxLD || A.m < 1 ||
      A.m > kRpeMaxPairs)
    return hipErrorInvalidValue;
  const dim3 grid(rpe_blocks(A.m)), block(256);
  for_d(A.d, [&](auto D) { for_widths(A, [&](auto WX, auto WR) { hipLaunchKernelGGL((k_rpe<D(), WX(), WR()>), grid, block, 0, st, A); }); });
  return hipGetLastError();
}
hipError_t launch_rpe_finish(const double *partial, int nblocks, int64_t m, double *stats, hipStream_t st) {
  const size_t nb = static_cast<size_t>(nblocks);
  hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, partial, nblocks, 2, stats);
  hipLaunchKernelGGL(k_reduce_max_partials, dim3(1), dim3(256), 0, st, partial + 2 * nb, nblocks, 2, stats + 2);
  hipLaunchKernelGGL(k_rpe_argmax, dim3(1), dim3(256), 0, st, partial + 2 * nb, partial + 4 * nb, nblocks, stats + 2,
                     static_cast<double>(m), stats + 4);
  return hipGetLastError();
}

// the rounding to SE(d) (kernels/round.inc): the count pass by wavefronts of poses with its one-wavefront finish, the apply
// pass by blocks of 256 units
static bool round_args_ok(const RoundArgs &A) {
  return (A.R.d == 2 || A.R.d == 3) && A.k >= A.R.d && A.k <= A.ldy && A.ldy <= kMaxLD && A.R.nl_poses >= 0 && A.R.nl_ranges >= 0 &&
         A.R.nl_trans >= 0;
}
hipError_t launch_round_count(const RoundArgs &A, hipStream_t st) {
  if (!round_args_ok(A)) return hipErrorInvalidValue;
  const int nb = round_count_blocks(A.R.nl_poses);
  if (nb > 0)
    for_d(A.R.d, [&](auto D) { hipLaunchKernelGGL(k_round_count<D()>, dim3(nb), dim3(kRoundCountBlock), 0, st, A); });
  hipLaunchKernelGGL(k_round_finish, dim3(1), dim3(64), 0, st, A.partial, nb, A.R.nl_poses, A.words);
  return hipGetLastError();
}
hipError_t launch_round_apply(const RoundArgs &A, hipStream_t st) {
  if (!round_args_ok(A)) return hipErrorInvalidValue;
  const int grid = row_unit_blocks(A.R);
  if (grid == 0) return hipSuccess;
  for_d(A.R.d, [&](auto D) { hipLaunchKernelGGL(k_round_apply<D()>, dim3(grid), dim3(256), 0, st, A); });
  return hipGetLastError();
}
// the odometry initialisation (kernels/odom.inc): the scan's three launches; the fill; the range rows with the sum of their counts
hipError_t launch_odom_scan(const OdomArgs &A, hipStream_t st) {
  if (A.P <= 0) return hipSuccess;
  if ((A.d != 2 && A.d != 3) || A.ntiles != odom_tiles(A.P) || !A.pos_edge || !A.pos_chain || !A.pos_rot || !A.pos_trn || !A.starts ||
      !A.totals || !A.carry || !A.out || !A.flag || (A.n_edges > 0 && !A.edge_data))
    return hipErrorInvalidValue;
  const dim3 grid(A.ntiles), block(kOdomTile);
  for_d(A.d, [&](auto D) {
    hipLaunchKernelGGL(k_odom_totals<D()>, grid, block, 0, st, A);
    hipLaunchKernelGGL(k_odom_middle<D()>, dim3(1), dim3(kOdomSweep), 0, st, A);
    hipLaunchKernelGGL(k_odom_scan<D()>, grid, block, 0, st, A);
  });
  return hipGetLastError();
}
hipError_t launch_odom_fill(const OdomFillArgs &A, hipStream_t st) {
  const int64_t units = A.n_free + A.n_lm;
  if (units <= 0) return hipSuccess;
  if ((A.d != 2 && A.d != 3) || !A.out || (A.n_free > 0 && (!A.free_rot || !A.free_trn)) || (A.n_lm > 0 && !A.lm_row))
    return hipErrorInvalidValue;
  const int64_t grid = (units + 255) / 256;
  if (grid >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  for_d(A.d, [&](auto D) { hipLaunchKernelGGL(k_odom_fill<D()>, dim3(grid), dim3(256), 0, st, A); });
  return hipGetLastError();
}
hipError_t launch_odom_ranges(const OdomFillArgs &A, hipStream_t st) {
  if ((A.d != 2 && A.d != 3) || !A.partial || !A.words || A.n_ranges < 0) return hipErrorInvalidValue;
  const int nb = odom_range_blocks(A.n_ranges);
  if (nb > 0) {
    if (!A.out || !A.range_rows || !A.deg || !A.flag) return hipErrorInvalidValue;
    for_d(A.d, [&](auto D) { hipLaunchKernelGGL(k_odom_ranges<D()>, dim3(nb), dim3(kWave), 0, st, A); });
  }
  hipLaunchKernelGGL(k_round_finish, dim3(1), dim3(64), 0, st, A.partial, nb, 0, A.words);  // words[0] = the sum
  return hipGetLastError();
}
// the multilateration (kernels/multilat.inc): the pass over the chunks and the fold per landmark of one stage, plain or with
// the masked passes of the robust form (whose Gauss-Newton fold is the plain one).  (The stage stands outside d: the linear
// kernels of both d are instantiated before the Gauss-Newton ones, and keep their places in the code object.)
template <bool ROBUST>
static hipError_t multilat_pass_fold(const MlKernelArgs<ROBUST> &K, hipStream_t st) {
  const MlArgs &A = ml_plain(K);
  const dim3 chunks(static_cast<unsigned>(A.n_chunks)), lms(static_cast<unsigned>(A.n_lm));
  if (A.stage == 0)
    for_d(A.d, [&](auto D) {
      if (A.n_chunks > 0) hipLaunchKernelGGL((k_ml_pass_linear<D(), ROBUST>), chunks, dim3(kMlChunk), 0, st, K);
      hipLaunchKernelGGL((k_ml_fold_linear<D(), ROBUST>), lms, dim3(kWave), 0, st, A);
    });
  else
    for_d(A.d, [&](auto D) {
      if (A.n_chunks > 0) hipLaunchKernelGGL((k_ml_pass_gn<D(), ROBUST>), chunks, dim3(kMlChunk), 0, st, K);
      hipLaunchKernelGGL(k_ml_fold_gn<D()>, lms, dim3(kWave), 0, st, A);
    });
  return hipGetLastError();
}
hipError_t launch_multilat_stage(const MlArgs &A, hipStream_t st) {
  if (A.n_lm <= 0) return hipSuccess;
  if ((A.d != 2 && A.d != 3) || A.stage < 0 || A.stage > kMlMaxSteps + 1 || (A.last && A.stage == 0) || A.n_chunks < 0 ||
      A.n_chunks >= (int64_t(1) << 31) || A.n_lm >= (int64_t(1) << 31) || !A.lm_chunk0 || !A.lm_row || !A.lm_origin || !A.lm_init ||
      !A.state || !A.istate || !A.x || !A.flag ||
      (A.n_chunks > 0 && (!A.chunk_lm || !A.chunk_begin || !A.chunk_len || !A.ent_row || !A.ent_m || !A.range_data || !A.partial)))
    return hipErrorInvalidValue;
  return multilat_pass_fold<false>(A, st);
}
// the outlier-robust multilateration: the consensus vote (one workgroup per chunk of all lists, then one wavefront per list),
// and a stage with the masked passes (every list has chunks: multilat_robust_args_ok)
static bool multilat_robust_args_ok(const MlRobustArgs &R) {
  const MlArgs &A = R.A;
  return (A.d == 2 || A.d == 3) && A.n_lm > 0 && A.n_chunks > 0 && A.n_chunks < (int64_t(1) << 31) && A.n_lm < (int64_t(1) << 31) &&
         A.n_ranges > 0 && A.chunk_lm && A.chunk_begin && A.chunk_len && A.ent_row && A.ent_m && A.lm_chunk0 && A.lm_row && A.lm_origin &&
         A.lm_init && A.range_data && A.partial && A.state && A.istate && A.x && A.flag && R.barc2 > 0.0 && R.min_consensus >= 1 && R.votes &&
         R.cstate && R.cint && R.inlier;
}
hipError_t launch_multilat_vote_elect(const MlRobustArgs &R, hipStream_t st) {
  if (!multilat_robust_args_ok(R)) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(R.A.n_chunks)), lms(static_cast<unsigned>(R.A.n_lm));
  for_d(R.A.d, [&](auto D) {
    hipLaunchKernelGGL(k_ml_vote<D()>, chunks, dim3(kMlChunk), 0, st, R);
    hipLaunchKernelGGL(k_ml_elect<D()>, lms, dim3(kWave), 0, st, R);
  });
  return hipGetLastError();
}
hipError_t launch_multilat_robust_stage(const MlRobustArgs &R, hipStream_t st) {
  const MlArgs &A = R.A;
  if (!multilat_robust_args_ok(R) || A.stage < 0 || A.stage > kMlMaxSteps + 1 || (A.last && A.stage == 0)) return hipErrorInvalidValue;
  return multilat_pass_fold<true>(R, st);
}
// the chain placement (kernels/placement.inc): every launch serves the one stage A describes
static bool place_args_ok(const PlArgs &A) {
  return (A.d == 2 || A.d == 3) && A.n_chunks > 0 && A.chunk0 >= 0 && A.pstride >= A.n_chunks && A.origin_q >= 0 && A.origin_a >= 0 &&
         A.pos0 >= 0 && A.n_pos > 0 && A.n_ranges > 0 && A.chunk_begin && A.chunk_len && A.ent_q && A.ent_a && A.ent_m && A.pos_rot &&
         A.pos_trn && A.range_data && A.partial && A.state && A.istate && A.x && A.flag;
}
hipError_t launch_place_linear(const PlArgs &A, hipStream_t st) {
  if (!place_args_ok(A)) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(A.n_chunks));
  for_d(A.d, [&](auto D) {
    hipLaunchKernelGGL(k_pl_pass_linear<D()>, chunks, dim3(kPlChunk), 0, st, A);
    hipLaunchKernelGGL(k_pl_fold_linear<D()>, dim3(1), dim3(kWave), 0, st, A);
  });
  return hipGetLastError();
}
hipError_t launch_place_gn(const PlArgs &A, hipStream_t st) {
  if (!place_args_ok(A) || A.step < 0 || A.step > kPlMaxSteps + 1) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(A.n_chunks));
  for_d(A.d, [&](auto D) {
    hipLaunchKernelGGL(k_pl_pass_gn<D()>, chunks, dim3(kPlChunk), 0, st, A);
    hipLaunchKernelGGL(k_pl_fold_gn<D()>, dim3(1), dim3(kWave), 0, st, A);
  });
  return hipGetLastError();
}
hipError_t launch_place_apply(const PlArgs &A, hipStream_t st) {
  if (!place_args_ok(A)) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((A.n_pos + 255) / 256));
  for_d(A.d, [&](auto D) { hipLaunchKernelGGL(k_pl_apply<D()>, grid, dim3(256), 0, st, A); });
  return hipGetLastError();
}
// the placement from sightings (kernels/sighting.inc): every launch serves all lists of the one stage A describes
static bool sighting_args_ok(const SgArgs &A) {
  return (A.d == 2 || A.d == 3) && A.n_chunks > 0 && A.chunk0 >= 0 && A.n_lists > 0 && A.list0 >= 0 && A.n_edges > 0 &&
         A.pstride >= static_cast<int64_t>(A.chunk0) + A.n_chunks && A.chunk_begin && A.chunk_len && A.chunk_list && A.list_chunk0 && A.list_row &&
         A.ent_rot && A.ent_trn && A.ent_lm && A.ent_e && A.edge_data && A.partial && A.state && A.istate && A.x && A.flag;
}
static bool sighting_args_ok(const SgRobustArgs &R) {
  return sighting_args_ok(R.A) && R.barc2 > 0.0 && R.min_chain_consensus >= 1 && R.min_landmark_consensus >= 1 && R.votes && R.hyp &&
         R.hstride > 0 && R.cstate && R.cint && R.inlier_chain && R.inlier_landmark;
}
template <bool ROBUST>
static hipError_t sighting_pass_fold(const SgKernelArgs<ROBUST> &K, hipStream_t st) {
  const SgArgs &A = sg_plain(K);
  if (!sighting_args_ok(K) || A.mode < 0 || A.mode > 3) return hipErrorInvalidValue;
  for_d(A.d, [&](auto D) {
    for_mode<4>(A.mode, [&](auto MODE) {
      hipLaunchKernelGGL((k_sg_pass<D(), MODE(), ROBUST>), dim3(static_cast<unsigned>(A.n_chunks)), dim3(kSgChunk), 0, st, K);
      hipLaunchKernelGGL((k_sg_fold<D(), MODE(), ROBUST>), dim3(static_cast<unsigned>(A.n_lists)), dim3(kWave), 0, st, K);
    });
  });
  return hipGetLastError();
}
hipError_t launch_sighting_pass_fold(const SgArgs &A, hipStream_t st) { return sighting_pass_fold<false>(A, st); }
hipError_t launch_sighting_robust_pass_fold(const SgRobustArgs &R, hipStream_t st) { return sighting_pass_fold<true>(R, st); }
// the consensus vote of the robust placement: (chain lists: one thread per entry for the hypotheses,) one workgroup per chunk,
// then one wavefront per list
hipError_t launch_sighting_vote_elect(const SgRobustArgs &R, int kind, hipStream_t st) {
  if (!sighting_args_ok(R) || kind < 0 || kind > 1) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(R.A.n_chunks)), lists(static_cast<unsigned>(R.A.n_lists));
  for_d(R.A.d, [&](auto D) {
    for_mode<2>(kind, [&](auto KIND) {
      if constexpr (KIND() == 1) hipLaunchKernelGGL(k_sg_hyp<D()>, chunks, dim3(kSgChunk), 0, st, R);
      hipLaunchKernelGGL((k_sg_vote<D(), KIND()>), chunks, dim3(kSgChunk), 0, st, R);
      hipLaunchKernelGGL((k_sg_elect<D(), KIND()>), lists, dim3(kWave), 0, st, R);
    });
  });
  return hipGetLastError();
}
// the rigid motion of the stage's chains: k_sg_apply reads only these fields, of SgArgs or of ClArgs (whose lists' state has
// the sighting placement's layout)
template <class Args>
static hipError_t chain_apply(const Args &A, hipStream_t st) {
  if (A.n_apply <= 0 || A.apply0 < 0 || !A.apply_pos || !A.apply_list || !A.pos_rot || !A.pos_trn) return hipErrorInvalidValue;
  const SgApplyArgs G{A.d, A.apply0, A.n_apply, A.apply_pos, A.apply_list, A.pos_rot, A.pos_trn, A.state, A.istate, A.x};
  const dim3 grid(static_cast<unsigned>((A.n_apply + 255) / 256));
  for_d(A.d, [&](auto D) { hipLaunchKernelGGL(k_sg_apply<D()>, grid, dim3(256), 0, st, G); });
  return hipGetLastError();
}
hipError_t launch_sighting_apply(const SgArgs &A, hipStream_t st) { return sighting_args_ok(A) ? chain_apply(A, st) : hipErrorInvalidValue; }
// the placement from closures (kernels/closure.inc): every launch serves all lists of the one stage A describes
static bool closure_args_ok(const ClArgs &A) {
  return (A.d == 2 || A.d == 3) && A.n_chunks > 0 && A.chunk0 >= 0 && A.n_lists > 0 && A.list0 >= 0 && A.n_edges > 0 &&
         A.pstride >= static_cast<int64_t>(A.chunk0) + A.n_chunks && A.chunk_begin && A.chunk_len && A.chunk_list && A.list_chunk0 && A.ent_e &&
         A.ent_dir && A.edge_rows && A.edge_data && A.partial && A.state && A.istate && A.x && A.flag;
}
static bool closure_args_ok(const ClRobustArgs &R) {
  return closure_args_ok(R.A) && R.barc2 > 0.0 && R.min_consensus >= 1 && R.votes && R.cstate && R.cint && R.inlier;
}
template <bool ROBUST>
static hipError_t closure_pass_fold(const ClKernelArgs<ROBUST> &K, hipStream_t st) {
  const ClArgs &A = cl_plain(K);
  if (!closure_args_ok(K) || A.mode < 0 || A.mode > 1) return hipErrorInvalidValue;
  for_d(A.d, [&](auto D) {
    for_mode<2>(A.mode, [&](auto MODE) {
      hipLaunchKernelGGL((k_cl_pass<D(), MODE(), ROBUST>), dim3(static_cast<unsigned>(A.n_chunks)), dim3(kClChunk), 0, st, K);
      hipLaunchKernelGGL((k_cl_fold<D(), MODE(), ROBUST>), dim3(static_cast<unsigned>(A.n_lists)), dim3(kWave), 0, st, K);
    });
  });
  return hipGetLastError();
}
hipError_t launch_closure_pass_fold(const ClArgs &A, hipStream_t st) { return closure_pass_fold<false>(A, st); }
hipError_t launch_closure_robust_pass_fold(const ClRobustArgs &R, hipStream_t st) { return closure_pass_fold<true>(R, st); }
hipError_t launch_closure_apply(const ClArgs &A, hipStream_t st) { return closure_args_ok(A) ? chain_apply(A, st) : hipErrorInvalidValue; }
// the consensus vote of the robust placement: one workgroup per chunk, then one wavefront per list
hipError_t launch_closure_vote_elect(const ClRobustArgs &R, hipStream_t st) {
  if (!closure_args_ok(R)) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(R.A.n_chunks)), lists(static_cast<unsigned>(R.A.n_lists));
  for_d(R.A.d, [&](auto D) {
    hipLaunchKernelGGL(k_cl_vote<D()>, chunks, dim3(kClChunk), 0, st, R);
    hipLaunchKernelGGL(k_cl_elect<D()>, lists, dim3(kWave), 0, st, R);
  });
  return hipGetLastError();
}
hipError_t launch_round_amax(int64_t n, const double *y, double *partial, int nblocks, int *flag, hipStream_t st) {
  if (n < 1 || nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_round_amax, dim3(nblocks), dim3(256), 0, st, n, y, partial, flag);
  return hipGetLastError();
}
hipError_t launch_round_scale(int64_t n, const double *y, int e, double *out, hipStream_t st) {
  if (n < 1) return hipSuccess;
  hipLaunchKernelGGL(k_round_scale, dim3(grid_for(n)), dim3(256), 0, st, n, y, e, out);
  return hipGetLastError();
}

// in-place update of Q's values (kernels/update_values.inc): two slots per thread
hipError_t launch_values_check(int64_t nnz, const double *vals, int64_t n_pairs, const int32_t *mirror, int *flag,
                               hipStream_t st) {
  if (nnz <= 0 && n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_values_check, dim3(grid_for(std::max(nnz, n_pairs))), dim3(256), 0, st, nnz, vals, n_pairs, mirror, flag);
  return hipGetLastError();
}

hipError_t launch_values_gather(int64_t n, const int32_t *src, const double *vals, double *dst, bool reciprocal,
                                hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const dim3 grid(grid_for((n + 1) / 2)), block(256);
  for_bool(reciprocal, [&](auto RECIPROCAL) { hipLaunchKernelGGL((k_values_gather<RECIPROCAL()>), grid, block, 0, st, n, src, vals, dst); });
  return hipGetLastError();
}

hipError_t launch_values_gather_sym(int64_t n, const int32_t *src, const double *vals, double *dst0, double *dst1,
                                    hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_values_gather_sym, dim3(grid_for((n + 1) / 2)), dim3(256), 0, st, n, src, vals, dst0, dst1);
  return hipGetLastError();
}

// assembly of Q(w) (kernels/assemble.inc)
hipError_t launch_weights_check(int64_t n, const double *w, int *flag, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_weights_check, dim3(grid_for(n)), dim3(256), 0, st, n, w, flag);
  return hipGetLastError();
}

hipError_t launch_assemble(const AssembleArgs &A, const double *w, double *vals, hipStream_t st) {
  if (A.nnz <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_assemble_short, dim3(grid_for((A.nnz + 1) / 2)), dim3(256), 0, st, A.nnz, A.tptr, A.tweight, A.tcoef, w, vals);
  if (A.n_long > 0)  // (after the short pass on the same stream: it leaves 0.0 in the long entries)
    hipLaunchKernelGGL(k_assemble_long, dim3(grid_for(A.n_long, 256 / kWave)), dim3(256), 0, st, A.n_long, A.long_entries, A.tptr,
                       A.tweight, A.tcoef, w, vals);
  return hipGetLastError();
}

hipError_t launch_scale_precisions(int64_t n, const double *base, const double *w, double *dst, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scale_precisions, dim3(grid_for(n)), dim3(256), 0, st, n, base, w, dst);
  return hipGetLastError();
}

#endif  // CORA_TU & 2
#if CORA_TU & 4

template <int LD>
static hipError_t rowop_ld(const RowOpDev &op, const double *src0, const double *src, double *dst, hipStream_t st,
                           const RvTail *tail) {
  const int grid = ((op.n8 + 31) >> 5) + ((op.n64 + 3) >> 2) + ((op.nchunks + 3) >> 2) + ((tail && tail->st) ? 1 : 0);
  RvTail T{};
  if (tail) T = *tail;
  if (grid > 0) hipLaunchKernelGGL((k_rowop<LD>), dim3(grid), dim3(256), 0, st, op, src0, src, dst, T);
  return hipGetLastError();
}

template <int LD>
static hipError_t blockop_ld(const BlockOpDev &B, bool backward, const double *src, double *dst, hipStream_t st) {
  const int grid = (B.nblocks + 3) >> 2;
  if (grid <= 0) return hipSuccess;
  for_bool(backward, [&](auto BACKWARD) { hipLaunchKernelGGL((k_blockop<LD, BACKWARD()>), dim3(grid), dim3(256), 0, st, B, src, dst); });
  return hipGetLastError();
}

template <int LD>
static hipError_t subblock_ld(const SubOpDev &S, bool backward, const double *src, double *work, double *dst, hipStream_t st,
                              const SubFuse *F = nullptr) {
  const int grid = launch_subblock_blocks(S);
  if (grid <= 0) return hipSuccess;
  const size_t lds = ((static_cast<size_t>(S.max_rows) * SubTile<LD>::kStride * 8 + 15) & ~static_cast<size_t>(15)) + static_cast<size_t>(S.max_lev + 2) * 16;
  if (S.max_level_lanes > kSubThreads || S.max_npl > kSubNpl || lds > 160 * 1024) return hipErrorInvalidValue;
  // (wide rows: the tile of a 435-row block is 56 KB at 16 columns, 84 KB at 24 -- above the 64 KB a kernel gets without asking)
  auto allow_lds = [&](const void *fn) {
    return lds > 64 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) : hipSuccess;
  };
  const dim3 g(grid), t(kSubThreads);
  if (F) {
    // the fused sweeps exist where cora_stpcg_dev dispatches them (row stride x d <= 24: above, the fused backward sweep
    // spills -- 172 to 380 bytes of scratch per lane at row strides 10-12 with d = 3 -- and was never launched)
    // the sweep's third template argument: 1 forward, d backward
    if (!backward) {
      if constexpr (LD <= 12) hipLaunchKernelGGL((k_subblock<LD, false, 1>), g, t, lds, st, S, src, work, dst, *F);
      else return hipErrorInvalidValue;
      return hipGetLastError();
    }
    if (F->d != 2 && F->d != 3) return hipErrorInvalidValue;
    return for_d(F->d, [&](auto D) {
      if constexpr (LD * D() <= 24) {
        hipLaunchKernelGGL((k_subblock<LD, true, D()>), g, t, lds, st, S, src, work, dst, *F);
        return hipGetLastError();
      } else {
        return hipErrorInvalidValue;
      }
    });
  }
  const SubFuse none{};
  return for_bool(backward, [&](auto BACKWARD) {
    if (const hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_subblock<LD, BACKWARD(), 0>)); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_subblock<LD, BACKWARD(), 0>), g, t, lds, st, S, src, work, dst, none);
    return hipGetLastError();
  });
}

// one set of launchers per row-stride group, each in the translation unit that instantiates the group's kernels
struct TriCall {  // what a staged-solve launch needs, whichever kernel it is
  int kind;       // 0 blockop, 1 rowop, 2 subblock, 3 subblock fused
  int ld;
  bool backward;
  const BlockOpDev *B;
  const RowOpDev *R;
  const SubOpDev *S;
  const SubFuse *F;
  const double *a, *b;  // blockop: src, -;  rowop: src0, src;  subblock: rhs_or_y, -
  double *work, *dst;
  const RvTail *tail = nullptr;
};
template <int G>
static hipError_t tri_group(const TriCall &c, hipStream_t st) {
  return in_ld_group<G>(c.ld, [&](auto LD) {
    if (c.kind == 0) return blockop_ld<LD()>(*c.B, c.backward, c.a, c.dst, st);
    if (c.kind == 1) return rowop_ld<LD()>(*c.R, c.a, c.b, c.dst, st, c.tail);
    if (c.kind == 2) return subblock_ld<LD()>(*c.S, c.backward, c.a, c.work, c.dst, st);
    return subblock_ld<LD()>(*c.S, c.backward, c.a, c.work, c.dst, st, c.F);
  });
}
using TriGroupFn = hipError_t(const TriCall &c, hipStream_t st);
TriGroupFn launch_tri_g0, launch_tri_g1, launch_tri_g2, launch_tri_g3, launch_tri_g4, launch_tri_g5;
#if CORA_LDG & 2
hipError_t launch_tri_g1(const TriCall &c, hipStream_t st) { return tri_group<1>(c, st); }
#endif
#if CORA_LDG & 4
hipError_t launch_tri_g2(const TriCall &c, hipStream_t st) { return tri_group<2>(c, st); }
#endif
#if CORA_LDG & 8
hipError_t launch_tri_g3(const TriCall &c, hipStream_t st) { return tri_group<3>(c, st); }
#endif
#if CORA_LDG & 16
hipError_t launch_tri_g4(const TriCall &c, hipStream_t st) { return tri_group<4>(c, st); }
#endif
#if CORA_LDG & 32
hipError_t launch_tri_g5(const TriCall &c, hipStream_t st) { return tri_group<5>(c, st); }
#endif
#if CORA_LDG & 1
hipError_t launch_tri_g0(const TriCall &c, hipStream_t st) { return tri_group<0>(c, st); }
static hipError_t launch_tri(const TriCall &c, hipStream_t st) {
  TriGroupFn *const group[kNumLdGroups] = {launch_tri_g0, launch_tri_g1, launch_tri_g2, launch_tri_g3, launch_tri_g4, launch_tri_g5};
  const int g = ld_group_of(c.ld);
  return g < kNumLdGroups ? group[g](c, st) : hipErrorInvalidValue;
}
hipError_t launch_blockop(const BlockOpDev &B, int ld, bool backward, const double *src, double *dst, hipStream_t st) {
  return launch_tri(TriCall{0, ld, backward, &B, nullptr, nullptr, nullptr, src, nullptr, nullptr, dst}, st);
}
hipError_t launch_rowop(const RowOpDev &op, int ld, const double *src0, const double *src, double *dst,
                        hipStream_t st, const RvTail *tail) {
  return launch_tri(TriCall{1, ld, false, nullptr, &op, nullptr, nullptr, src0, src, nullptr, dst, tail}, st);
}
hipError_t launch_subblock_fused(const SubOpDev &S, int ld, bool backward, const SubFuse &F, double *work, double *out,
                                 hipStream_t st) {
  // forward: the right-hand side is F.r, y -> out;  backward: y is read from `out`, v -> out
  return launch_tri(TriCall{3, ld, backward, nullptr, nullptr, &S, &F, backward ? out : F.r, nullptr, work, out}, st);
}
hipError_t launch_subblock(const SubOpDev &S, int ld, bool backward, const double *rhs_or_y, double *work, double *out,
                           hipStream_t st) {
  return launch_tri(TriCall{2, ld, backward, nullptr, nullptr, &S, nullptr, rhs_or_y, nullptr, work, out}, st);
}
hipError_t launch_kappa_finish(const double *partial, int n, StpcgState *state, hipStream_t st) {
  hipLaunchKernelGGL(k_kappa_finish, dim3(1), dim3(256), 0, st, partial, n, state);
  return hipGetLastError();
}
hipError_t launch_zero_row(double *x, size_t row, int ld, hipStream_t st) {
  hipLaunchKernelGGL(k_zero_row, dim3(1), dim3(64), 0, st, x, row, ld);
  return hipGetLastError();
}
#endif  // CORA_LDG & 1

#endif  // CORA_TU & 4
#if CORA_TU & 2

hipError_t launch_fill_random(int64_t N, int k, unsigned long long seed, const int32_t *api2int, double *x, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  const int ld = ld_for(k);
  hipLaunchKernelGGL(k_fill_random, dim3(grid_for(N * ld)), dim3(256), 0, st, N, ld, k, seed, api2int, x);
  return hipGetLastError();
}

hipError_t launch_gram(int64_t row0, int64_t rows, const double *A, int ka, const double *B, int kb,
                       double *partial, int nblocks, double *out, hipStream_t st) {
  hipLaunchKernelGGL(k_gram, dim3(nblocks), dim3(256), 0, st, row0, rows, A, ld_for(ka), ka, B, ld_for(kb), kb, partial);
  const int nel = ka * kb;
  hipLaunchKernelGGL(k_gram_reduce, dim3(nel), dim3(256), 0, st, partial, nblocks, nel, out);
  return hipGetLastError();
}

// n products in one launch + one reduction over all their elements: partial = n consecutive pieces (ka_e kb_e nblocks
// doubles each), out = the n results one after the other (row-major ka_e x kb_e) -- may be pinned host memory
hipError_t launch_gram_batch(int64_t row0, int64_t rows, int n, const double *const *A, const int *ka, const double *const *B,
                             const int *kb, double *partial, int nblocks, double *out, hipStream_t st) {
  if (n < 1 || n > 16) return hipErrorInvalidValue;
  GramBatch G{};
  int nel_all = 0;
  for (int e = 0; e < n; ++e) {
    G.A[e] = A[e];
    G.B[e] = B[e];
    G.lda[e] = ld_for(ka[e]);
    G.ka[e] = ka[e];
    G.ldb[e] = ld_for(kb[e]);
    G.kb[e] = kb[e];
    G.partial[e] = partial + static_cast<size_t>(nel_all) * nblocks;
    nel_all += ka[e] * kb[e];
  }
  hipLaunchKernelGGL(k_gram_batch, dim3(nblocks, n), dim3(256), 0, st, row0, rows, G);
  hipLaunchKernelGGL(k_gram_reduce, dim3(nel_all), dim3(256), 0, st, partial, nblocks, nel_all, out);
  return hipGetLastError();
}

// coef_host != nullptr and ncoef <= CombineCoef::kMax: the coefficients travel in the kernel's arguments (coef unused)
hipError_t launch_combine(int64_t row0, int64_t rows, int nblocks, const double *const *x, const int *kx,
                          const int *coff, const double *coef, int ncoef, int kout, double *out, hipStream_t st,
                          const double *coef_host) {
  CombineArgs A;
  for (int b = 0; b < 4; ++b) { A.x[b] = nullptr; A.kx[b] = 0; A.ldx[b] = 0; A.coff[b] = 0; }
  for (int b = 0; b < nblocks; ++b) { A.x[b] = x[b]; A.kx[b] = kx[b]; A.ldx[b] = ld_for(kx[b]); A.coff[b] = coff[b]; }
  A.nblocks = nblocks;
  A.kout = kout;
  A.ldo = ld_for(kout);
  const int grid = static_cast<int>(std::min<int64_t>((rows + 63) / 64, 2048));  // 4 wavefronts x 16 rows per block and step
  if (coef_host && ncoef <= CombineCoef::kMax) {
    CombineCoef K;
    for (int t = 0; t < ncoef; ++t) K.v[t] = coef_host[t];
    hipLaunchKernelGGL(k_combine_karg, dim3(std::max(grid, 1)), dim3(256), ncoef * sizeof(double), st, row0, rows, A, K, ncoef, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_combine, dim3(std::max(grid, 1)), dim3(256), ncoef * sizeof(double), st, row0, rows, A, coef,
                     ncoef, out);
  return hipGetLastError();
}

#endif  // CORA_TU & 2
// the chain placement's batched form (kernels/placement.inc, BATCHED): every launch serves all stages of the one level B
// describes.  A translation unit of its own: the plain and the batched kernels call the same functions of kernels.h, and the
// compiler inlines and unrolls a function with one caller in a unit differently from one with two -- side by side the
// plain kernels would no longer be the ones profiles/chain_placement.md measured.
#if CORA_TU & 8
static bool place_args_ok(const PlBatchArgs &B) { return pl_batch_args_ok(B); }
hipError_t launch_place_linear(const PlBatchArgs &B, hipStream_t st) {
  if (!place_args_ok(B)) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(B.A.n_chunks)), stages(static_cast<unsigned>(B.n_stages));
  for_d(B.A.d, [&](auto D) {
    hipLaunchKernelGGL((k_pl_pass_linear<D(), true>), chunks, dim3(kPlChunk), 0, st, B);
    hipLaunchKernelGGL((k_pl_fold_linear<D(), true>), stages, dim3(kWave), 0, st, B);
  });
  return hipGetLastError();
}
hipError_t launch_place_gn(const PlBatchArgs &B, hipStream_t st) {
  if (!place_args_ok(B) || B.A.step < 0 || B.A.step > kPlMaxSteps + 1) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(B.A.n_chunks)), stages(static_cast<unsigned>(B.n_stages));
  for_d(B.A.d, [&](auto D) {
    hipLaunchKernelGGL((k_pl_pass_gn<D(), true>), chunks, dim3(kPlChunk), 0, st, B);
    hipLaunchKernelGGL((k_pl_fold_gn<D(), true>), stages, dim3(kWave), 0, st, B);
  });
  return hipGetLastError();
}
hipError_t launch_place_apply(const PlBatchArgs &B, hipStream_t st) {
  if (!place_args_ok(B)) return hipErrorInvalidValue;
  for_d(B.A.d, [&](auto D) { hipLaunchKernelGGL((k_pl_apply<D(), true>), dim3(static_cast<unsigned>(B.n_tiles)), dim3(256), 0, st, B); });
  return hipGetLastError();
}
#endif  // CORA_TU & 8
// the chain placement's outlier-robust form (kernels/placement.inc, MASK): the consensus vote of the one level R describes, and
// the batched launches over the inliers.  A translation unit of its own, for the reason above: the plain and the batched
// kernels stay the code objects they were.
#if CORA_TU & 16
static bool place_args_ok(const PlRobustArgs &R) {
  const PlArgs &A = R.B.A;
  return pl_batch_args_ok(R.B) && R.barc2 > 0.0 && R.min_consensus >= 1 && R.ent0 >= 0 && R.n_ent >= A.n_chunks && R.hstride >= static_cast<int64_t>(R.ent0) + R.n_ent &&
         R.hyp && R.votes && R.cstate && R.cint && R.inlier;
}
hipError_t launch_place_vote_elect(const PlRobustArgs &R, hipStream_t st) {
  if (!place_args_ok(R)) return hipErrorInvalidValue;
  const dim3 hyps(static_cast<unsigned>((R.n_ent + 256 / kWave - 1) / (256 / kWave))), chunks(static_cast<unsigned>(R.B.A.n_chunks)),
      stages(static_cast<unsigned>(R.B.n_stages));
  for_d(R.B.A.d, [&](auto D) {
    hipLaunchKernelGGL(k_pl_hyp<D()>, hyps, dim3(256), 0, st, R);
    hipLaunchKernelGGL(k_pl_vote<D()>, chunks, dim3(kPlChunk), 0, st, R);
    hipLaunchKernelGGL(k_pl_elect<D()>, stages, dim3(kWave), 0, st, R);
  });
  return hipGetLastError();
}
hipError_t launch_place_linear(const PlRobustArgs &R, hipStream_t st) {
  if (!place_args_ok(R)) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(R.B.A.n_chunks)), stages(static_cast<unsigned>(R.B.n_stages));
  for_d(R.B.A.d, [&](auto D) {
    hipLaunchKernelGGL((k_pl_pass_linear<D(), true, true>), chunks, dim3(kPlChunk), 0, st, R);
    hipLaunchKernelGGL((k_pl_fold_linear<D(), true, true>), stages, dim3(kWave), 0, st, R);
  });
  return hipGetLastError();
}
hipError_t launch_place_gn(const PlRobustArgs &R, hipStream_t st) {
  if (!place_args_ok(R) || R.B.A.step < 0 || R.B.A.step > kPlMaxSteps + 1) return hipErrorInvalidValue;
  const dim3 chunks(static_cast<unsigned>(R.B.A.n_chunks)), stages(static_cast<unsigned>(R.B.n_stages));
  for_d(R.B.A.d, [&](auto D) {
    hipLaunchKernelGGL((k_pl_pass_gn<D(), true, true>), chunks, dim3(kPlChunk), 0, st, R);
    hipLaunchKernelGGL((k_pl_fold_gn<D(), true, true>), stages, dim3(kWave), 0, st, R);
  });
  return hipGetLastError();
}
hipError_t launch_place_apply(const PlRobustArgs &R, hipStream_t st) {
  if (!place_args_ok(R)) return hipErrorInvalidValue;
  for_d(R.B.A.d, [&](auto D) { hipLaunchKernelGGL((k_pl_apply<D(), true, true>), dim3(static_cast<unsigned>(R.B.n_tiles)), dim3(256), 0, st, R); });
  return hipGetLastError();
}
#endif  // CORA_TU & 16
