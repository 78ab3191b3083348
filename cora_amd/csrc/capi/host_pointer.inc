// Part of capi.hip (one translation unit; included there, in this order).  host-pointer operator API (one entry per reference method) and host-side debug hooks.
// ------------------------------------------------- host-pointer operator API

#define CHECK_LD(c, ld)                                                                  \
  do {                                                                                   \
    if ((ld) < (c)->F.L.N) return fail((c), CORA_ERR_SHAPE, "leading dimension smaller than N"); \
  } while (0)

int cora_data_matrix_product(cora_ctx *c, const double *X, int ldx, int k, double *out, int ldo) {
  NEED_DEVICE(c);
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  double *dX, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, ld_for(k), &dX))) return rc;
  if ((rc = get_scratch(c, 1, ld_for(k), &dO))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, ld_for(k)), c->stream));
  if ((rc = cora_spmm_dev(c, dX, k, dO))) return rc;
  return download_impl(c, dO, k, out, ldo);
}

int cora_evaluate_objective(cora_ctx *c, const double *Y, int ldy, double *f) {
  if (!f) return fail(c, CORA_ERR_ARG, "null pointer");
  int rc = cora_set_point(c, Y, ldy);
  if (rc) return rc;
  *f = c->f;
  return CORA_OK;
}

int cora_euclidean_gradient(cora_ctx *c, const double *Y, int ldy, double *out, int ldo) {
  int rc = cora_set_point(c, Y, ldy);
  if (rc) return rc;
  return download_impl(c, c->d_G, c->p, out, ldo);
}

int cora_riemannian_gradient(cora_ctx *c, const double *Y, int ldy, double *out, int ldo) {
  int rc = cora_set_point(c, Y, ldy);
  if (rc) return rc;
  return download_impl(c, c->d_rgrad, c->p, out, ldo);
}

int cora_tangent_space_projection(cora_ctx *c, const double *Y, int ldy, const double *V, int ldv,
                                  double *out, int ldo) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  double *dV, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, c->ld, &dV))) return rc;
  if ((rc = get_scratch(c, 1, c->ld, &dO))) return rc;
  if ((rc = upload_impl(c, Y, ldy, c->p, c->d_Y))) return rc;
  c->have_point = false;  // Y replaced without refreshing the cached gradient
  c->trial_x = nullptr;
  if ((rc = upload_impl(c, V, ldv, c->p, dV))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, c->ld), c->stream));
  HIP_TRY(c, launch_tangent_project(row_args(c), c->ld, c->d_Y, dV, nullptr, dO, c->stream));
  return download_impl(c, dO, c->p, out, ldo);
}

int cora_riemannian_hessian_vector_product(cora_ctx *c, const double *Y, int ldy, const double *G, int ldg,
                                           const double *dotY, int ldd, double *out, int ldo) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  double *dX, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, c->ld, &dX))) return rc;
  if ((rc = get_scratch(c, 1, c->ld, &dO))) return rc;
  // honour the reference signature: Lambda is built from the nablaF_Y passed in
  if ((rc = upload_impl(c, Y, ldy, c->p, c->d_Y))) return rc;
  if ((rc = upload_impl(c, G, ldg, c->p, c->d_G))) return rc;
  if ((rc = point_finish(c))) return rc;
  if ((rc = upload_impl(c, dotY, ldd, c->p, dX))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, c->ld), c->stream));
  if ((rc = cora_hvp_dev(c, dX, dO))) return rc;
  return download_impl(c, dO, c->p, out, ldo);
}

int cora_project_to_manifold(cora_ctx *c, const double *A, int lda, double *out, int ldo) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  double *dA, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, c->ld, &dA))) return rc;
  if ((rc = get_scratch(c, 1, c->ld, &dO))) return rc;
  if ((rc = upload_impl(c, A, lda, c->p, dA))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, c->ld), c->stream));
  HIP_TRY(c, launch_project_manifold(row_args(c), c->ld, dA, nullptr, 0.0, dO, c->stream));
  return download_impl(c, dO, c->p, out, ldo);
}

int cora_retract(cora_ctx *c, const double *Y, int ldy, const double *V, int ldv, double *out, int ldo) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  double *dY, *dV, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, c->ld, &dY))) return rc;
  if ((rc = get_scratch(c, 1, c->ld, &dV))) return rc;
  if ((rc = get_scratch(c, 2, c->ld, &dO))) return rc;
  if ((rc = upload_impl(c, Y, ldy, c->p, dY))) return rc;
  if ((rc = upload_impl(c, V, ldv, c->p, dV))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, c->ld), c->stream));
  HIP_TRY(c, launch_project_manifold(row_args(c), c->ld, dY, dV, 1.0, dO, c->stream));
  return download_impl(c, dO, c->p, out, ldo);
}

int cora_precondition(cora_ctx *c, const double *V, int ldv, double *out, int ldo) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (c->precond == CORA_PRECOND_NONE)
    return fail(c, CORA_ERR_NOT_READY, "preconditioner not set up (cora_precond_setup)");
  double *dV, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, c->ld, &dV))) return rc;
  if ((rc = get_scratch(c, 1, c->ld, &dO))) return rc;
  const size_t off = static_cast<size_t>(c->F.L.base) * c->ld;
  if (c->precond == CORA_PRECOND_JACOBI) {
    if ((rc = upload_impl(c, V, ldv, c->p, dV))) return rc;
    HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, c->ld), c->stream));
    HIP_TRY(c, launch_scale_rows(c->F.L.local_rows, c->ld, c->d_diag_inv, dV + off, dO + off, c->stream));
  } else {
    if ((rc = upload_impl(c, V, ldv, c->p, dV))) return rc;
    if ((rc = chol_solve(c, c->ld, dV, dO))) return rc;
  }
  // NaN guard, src/CORA_problem.cpp:898-901
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  HIP_TRY(c, launch_has_nan(c->F.L.local_rows * c->ld, dO + off, c->d_flag, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_flag) return fail(c, CORA_ERR_NAN, "NaNs in preconditioned vector");
  return download_impl(c, dO, c->p, out, ldo);
}

int cora_compute_lambda_blocks(cora_ctx *c, const double *Y, int ldy, double *stiefel, double *oblique) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  int rc = cora_set_point(c, Y, ldy);
  if (rc) return rc;
  const Layout &L = c->F.L;
  if (L.world != 1) {
    // Partitioned handle: every rank holds the blocks of its own poses and range rows.  They travel as a resident
    // vector with d columns -- row (pose, a) carries row a of the pose's block, a range row its multiplier in column 0
    // -- through the collective download (one all-gather of the shards); every rank gets all of them.
    const int k = L.d, ld = ld_for(k);
    if (ld != L.d) return fail(c, CORA_ERR_ARG, "unexpected row stride");
    double *vec;
    if ((rc = get_scratch(c, 2, ld, &vec))) return rc;
    HIP_TRY(c, hipMemsetAsync(vec, 0, vec_bytes(c, ld), c->stream));
    if (L.nl_poses > 0)  // [pose][d * d] IS rows (pose, a) x d columns at row stride d
      HIP_TRY(c, hipMemcpyAsync(vec + static_cast<size_t>(L.rot_base) * ld, c->d_lam_st,
                                static_cast<size_t>(L.nl_poses) * L.d * L.d * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (L.nl_ranges > 0)
      HIP_TRY(c, hipMemcpy2DAsync(vec + static_cast<size_t>(L.rng_base) * ld, ld * sizeof(double), c->d_lam_ob, sizeof(double),
                                  sizeof(double), static_cast<size_t>(L.nl_ranges), hipMemcpyDeviceToDevice, c->stream));
    std::vector<double> M(static_cast<size_t>(L.N) * k);
    if ((rc = download_impl(c, vec, k, M.data(), static_cast<int>(L.N)))) return rc;
    if (stiefel)
      for (int64_t i = 0; i < L.n; ++i)
        for (int a = 0; a < L.d; ++a)
          for (int b = 0; b < L.d; ++b)
            stiefel[(i * L.d + b) * L.d + a] = M[static_cast<size_t>(i * L.d + a) + static_cast<size_t>(L.N) * b];
    if (oblique)
      for (int64_t j = 0; j < L.r; ++j) oblique[j] = M[static_cast<size_t>(L.d) * L.n + j];
    return CORA_OK;
  }
  // a symmetric d x d block is the same row- or column-major, so the device
  // array [pose][d*d] already is the d x (d n) column-major matrix
  if (L.n > 0 && stiefel)
    HIP_TRY(c, hipMemcpyAsync(stiefel, c->d_lam_st, static_cast<size_t>(L.n) * L.d * L.d * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
  std::vector<double> ob(static_cast<size_t>(std::max(L.r, 1)));
  if (L.r > 0 && oblique)
    HIP_TRY(c, hipMemcpyAsync(ob.data(), c->d_lam_ob, static_cast<size_t>(L.r) * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the device keeps range rows in its internal (pose-sorted) order
  if (L.r > 0 && oblique)
    for (int k = 0; k < L.r; ++k)
      oblique[k] = ob[static_cast<size_t>(c->F.api2int[static_cast<size_t>(L.d) * L.n + k] - L.rng_base)];
  return CORA_OK;
}

int cora_certificate_product(cora_ctx *c, const double *X, int ldx, int k, double *out, int ldo) {
  NEED_DEVICE(c);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  double *dX, *dO;
  int rc;
  if ((rc = get_scratch(c, 0, ld_for(k), &dX))) return rc;
  if ((rc = get_scratch(c, 1, ld_for(k), &dO))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  HIP_TRY(c, hipMemsetAsync(dO, 0, vec_bytes(c, ld_for(k)), c->stream));
  if ((rc = cora_certificate_product_dev(c, dX, k, dO))) return rc;
  return download_impl(c, dO, k, out, ldo);
}

int cora_inner_product(cora_ctx *c, const double *A, int lda, const double *B, int ldb, int k, double *out) {
  NEED_DEVICE(c);
  double *dA, *dB;
  int rc;
  if ((rc = get_scratch(c, 0, ld_for(k), &dA))) return rc;
  if ((rc = get_scratch(c, 1, ld_for(k), &dB))) return rc;
  if ((rc = upload_impl(c, A, lda, k, dA))) return rc;
  if ((rc = upload_impl(c, B, ldb, k, dB))) return rc;
  return cora_dot_dev(c, dA, dB, k, out);
}

int cora_debug_format_spmm_host(const cora_ctx *c, const double *X, int ldx, int k, double *out, int ldo) {
  if (!c || !X || !out || k <= 0 || k > kMaxLD) return CORA_ERR_ARG;
  if (c->host_values_stale)
    return fail(const_cast<cora_ctx *>(c), CORA_ERR_NOT_READY,
                "the host copy of the format holds the values from before cora_update_values_dev: update with host values first");
  const HostFormat &F = c->F;
  const int ld = ld_for(k);
  const int64_t N = F.L.N;
  std::vector<double> xi(static_cast<size_t>(F.L.rows) * ld, 0.0), oi(static_cast<size_t>(F.L.rows) * ld, 0.0);
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i)
      xi[static_cast<size_t>(F.api2int[i]) * ld + cc] = X[static_cast<size_t>(cc) * ldx + i];
  format_spmm_host(F, xi.data(), ld, oi.data());
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i)
      out[static_cast<size_t>(cc) * ldo + i] = oi[static_cast<size_t>(F.api2int[i]) * ld + cc];
  return CORA_OK;
}

int cora_debug_format_digest(const cora_ctx *c, uint64_t out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  format_digest(c->F, out);
  return CORA_OK;
}

int cora_debug_long_image(const cora_ctx *c, int piece, int64_t sizes[5], int32_t *chunks, int32_t *chunk_order, double *lval,
                          int32_t *lcol, int32_t *perm, int8_t *home, int8_t *home_pose_first) {
  if (!c || !sizes) return CORA_ERR_ARG;
  if (c->host_values_stale)
    return fail(const_cast<cora_ctx *>(c), CORA_ERR_NOT_READY,
                "the host copy of the format holds the values from before cora_update_values_dev: update with host values first");
  const LongImage I = build_long_image(c->F, piece > 0 ? piece : kLongPiece);
  sizes[0] = static_cast<int64_t>(I.chunks.size());
  sizes[1] = static_cast<int64_t>(I.chunk_order.size());
  sizes[2] = static_cast<int64_t>(I.lval.size());
  sizes[3] = c->F.L.rows;
  sizes[4] = I.placed ? 1 : 0;
  if (chunks) std::memcpy(chunks, I.chunks.data(), I.chunks.size() * sizeof(LongChunk));
  if (chunk_order) std::copy(I.chunk_order.begin(), I.chunk_order.end(), chunk_order);
  if (lval) std::copy(I.lval.begin(), I.lval.end(), lval);
  if (lcol) std::copy(I.lcol.begin(), I.lcol.end(), lcol);
  if (perm) std::copy(I.perm.begin(), I.perm.end(), perm);
  std::vector<int8_t> h;
  if (home) {
    long_row_homes(c->F, c->F.slices, h);
    std::copy(h.begin(), h.end(), home);
  }
  if (home_pose_first) {
    long_row_homes(c->F, c->F.slices_pose_first.empty() ? c->F.slices : c->F.slices_pose_first, h);
    std::copy(h.begin(), h.end(), home_pose_first);
  }
  return CORA_OK;
}

int cora_debug_value_map_digest(cora_ctx *c, uint64_t out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  if (!c->vmap.built) return fail(c, CORA_ERR_NOT_READY, "no source map yet: call cora_values_map_build or cora_update_values first");
  value_map_digest(c->vmap, out);
  return CORA_OK;
}

int cora_debug_factor_solve_host(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, int k,
                                 const double *B, double *X, int64_t stats[4]) {
  if (m <= 0 || !Lp || !Li || !Lx || !B || !X || k <= 0) return CORA_ERR_ARG;
  try {
    std::vector<int32_t> row_of(static_cast<size_t>(m));
    for (int i = 0; i < m; ++i) row_of[i] = i;
    TriPlan P;
    build_tri_plan(m, Lp, Li, Lx, row_of, m, P, nullptr, m + 1);  // row m plays the pinned variable
    std::vector<double> rhs(static_cast<size_t>(m) + 1), out(static_cast<size_t>(m) + 1);
    for (int cc = 0; cc < k; ++cc) {
      std::copy(B + static_cast<size_t>(cc) * m, B + static_cast<size_t>(cc + 1) * m, rhs.begin());
      rhs[m] = 1.0;
      std::fill(out.begin(), out.end(), 7.0);
      tri_plan_solve_host(P, m + 1, rhs.data(), out.data());
      if (out[m] != 0.0) return fail(nullptr, CORA_ERR_ARG, "the pinned row was not zeroed");
      std::copy(out.begin(), out.begin() + m, X + static_cast<size_t>(cc) * m);
    }
    if (stats) {
      stats[0] = static_cast<int64_t>(P.stages.size());
      stats[1] = P.nnzW;
      stats[2] = P.nnzL;
      stats[3] = P.stages.empty() ? 0 : (P.stages[0].dense ? static_cast<int64_t>(P.stages[0].blocks_op.nrows.size())
                                                        : (P.stages[0].sub ? static_cast<int64_t>(P.stages[0].sub_op.nrows.size()) : 0));
    }
  } catch (const std::exception &e) {
    return fail(nullptr, CORA_ERR_ARG, e.what());
  }
  return CORA_OK;
}

int cora_debug_factor_plan_host(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, int aux_ok, int64_t out[24]) {
  if (m <= 0 || !Lp || !Li || !Lx || !out) return CORA_ERR_ARG;
  try {
    std::vector<int32_t> row_of(static_cast<size_t>(m));
    for (int i = 0; i < m; ++i) row_of[i] = i;
    TriPlan P;
    build_tri_plan(m, Lp, Li, Lx, row_of, -1, P, nullptr, aux_ok ? m : -1);
    tri_plan_shape(P, out);
  } catch (const std::exception &e) {
    return fail(nullptr, CORA_ERR_ARG, e.what());
  }
  return CORA_OK;
}

int cora_debug_factor_plan_digest(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, const int32_t *group, int aux_ok,
                                  uint64_t out[2]) {
  if (m <= 0 || !Lp || !Li || !Lx || !out) return CORA_ERR_ARG;
  try {
    std::vector<int32_t> row_of(static_cast<size_t>(m));
    for (int i = 0; i < m; ++i) row_of[i] = i;
    std::vector<int32_t> g;
    if (group) g.assign(group, group + m);
    TriPlan P;
    build_tri_plan(m, Lp, Li, Lx, row_of, -1, P, group ? &g : nullptr, aux_ok ? m : -1);
    tri_plan_digest(P, out);
  } catch (const std::exception &e) {
    return fail(nullptr, CORA_ERR_ARG, e.what());
  }
  return CORA_OK;
}

int cora_debug_factor_image(int m, const int32_t *Lp, const int32_t *Li, const double *Lx, const int32_t *row_of,
                            const int32_t *group, int aux_ok, int64_t rows, int32_t zero_row, int d, int64_t rot0, int64_t rot1,
                            uint64_t digest[2], int64_t shape[24]) {
  if (m <= 0 || !Lp || !Li || !Lx || !digest || !shape) return CORA_ERR_ARG;
  if (rows <= 0) rows = m;
  if (rows < m || rows > INT32_MAX || zero_row >= rows || rot0 < 0 || rot1 < rot0 || rot1 > rows ||
      (rot1 > rot0 && (d <= 0 || (rot1 - rot0) % d != 0)))
    return fail(nullptr, CORA_ERR_ARG, "cora_debug_factor_image: layout outside the vector");
  try {
    std::vector<int32_t> map(static_cast<size_t>(m));
    for (int i = 0; i < m; ++i) {
      map[i] = row_of ? row_of[i] : i;
      if (map[i] < 0 || map[i] >= rows) return fail(nullptr, CORA_ERR_ARG, "cora_debug_factor_image: row map outside the vector");
    }
    std::vector<int32_t> g;
    if (group) g.assign(group, group + m);
    TriPlan P;
    TriImage I;
    PhaseTimer tick(false, "", 0, 0);
    build_tri_plan(m, Lp, Li, Lx, map, zero_row, P, group ? &g : nullptr, aux_ok ? static_cast<int32_t>(rows) : -1);
    build_tri_image(P, ImageLayout{d, rot0, rot1, rows, group != nullptr}, I, tick);
    tri_image_digest(P, I, digest);
    tri_image_shape(P, I, shape);
  } catch (const std::exception &e) {
    return fail(nullptr, CORA_ERR_ARG, e.what());
  }
  return CORA_OK;
}
