// Part of capi.hip (one translation unit; included there, in this order).  the measurement table of a handle (cora_set_measurements) and the per-measurement residuals: device pass, host-pointer form, host execution of the translated table.
// ------------------------------------------------- per-measurement residuals

int cora_set_measurements(cora_ctx *c, int64_t n_edges, const int32_t *edge_rows, const double *edge_data, int64_t n_ranges,
                          const int32_t *range_rows, const double *range_data) {
  if (!c) return CORA_ERR_ARG;
  const Layout &L = c->F.L;
  if (L.world > 1) return fail(c, CORA_ERR_ARG, "measurement tables are not supported on partitioned handles");
  if (n_edges < 0 || n_ranges < 0) return fail(c, CORA_ERR_ARG, "negative measurement count");
  if ((n_edges > 0 && (!edge_rows || !edge_data)) || (n_ranges > 0 && (!range_rows || !range_data)))
    return fail(c, CORA_ERR_ARG, "null pointer");
  const int d = L.d;
  const int64_t dn = static_cast<int64_t>(d) * L.n, r0 = dn, t0 = dn + L.r, N = L.N;
  const int nf = d * d + d + 2;
  const std::vector<int32_t> &a2i = c->F.api2int;
  auto at = [](const char *what, int64_t e) { return std::string(what) + " of measurement " + std::to_string(e); };
  // first internal row of the pose whose rotation block starts at API row `row`; its d rows must be consecutive there too
  auto rot_row = [&](int32_t row, int32_t *out) {
    if (row < 0 || row >= dn || row % d != 0) return false;
    *out = a2i[static_cast<size_t>(row)];
    for (int j = 1; j < d; ++j)
      if (a2i[static_cast<size_t>(row) + j] != *out + j) return false;
    return true;
  };
  MeasurementTable T;
  T.n_edges = n_edges;
  T.n_ranges = n_ranges;
  T.edge_rows.resize(static_cast<size_t>(4 * n_edges));
  T.edge_data.resize(static_cast<size_t>(nf) * n_edges);
  T.range_rows.resize(static_cast<size_t>(3 * n_ranges));
  T.range_data.resize(static_cast<size_t>(2 * n_ranges));
  T.api_edge_rows.assign(edge_rows, edge_rows + 4 * n_edges);
  T.api_range_rows.assign(range_rows, range_rows + 3 * n_ranges);
  for (int64_t e = 0; e < n_edges; ++e) {
    const int32_t *row = edge_rows + 4 * e;
    int32_t ra = 0, rb = -1;
    if (!rot_row(row[0], &ra))
      return fail(c, CORA_ERR_ARG, at("first rotation row", e) + " must be a multiple of d below d * n whose d rows are consecutive in the internal order");
    if (row[1] != -1 && !rot_row(row[1], &rb))
      return fail(c, CORA_ERR_ARG, at("second rotation row", e) + " must be -1 or a multiple of d below d * n whose d rows are consecutive in the internal order");
    for (int j = 2; j < 4; ++j)
      if (row[j] < t0 || row[j] >= N) return fail(c, CORA_ERR_ARG, at("translation row", e) + " must lie in [d * n + r, N)");
    T.edge_rows[static_cast<size_t>(e)] = ra;
    T.edge_rows[static_cast<size_t>(n_edges + e)] = rb;
    T.edge_rows[static_cast<size_t>(2 * n_edges + e)] = a2i[static_cast<size_t>(row[2])];
    T.edge_rows[static_cast<size_t>(3 * n_edges + e)] = a2i[static_cast<size_t>(row[3])];
    for (int f = 0; f < nf; ++f) {
      const double v = edge_data[static_cast<size_t>(e) * nf + f];
      if (!std::isfinite(v)) return fail(c, CORA_ERR_ARG, at("non-finite data", e));
      T.edge_data[static_cast<size_t>(f) * n_edges + e] = v;
    }
  }
  for (int64_t m = 0; m < n_ranges; ++m) {
    const int32_t *row = range_rows + 3 * m;
    if (row[0] < r0 || row[0] >= t0) return fail(c, CORA_ERR_ARG, at("range row", m) + " must lie in [d * n, d * n + r)");
    for (int j = 1; j < 3; ++j)
      if (row[j] < t0 || row[j] >= N) return fail(c, CORA_ERR_ARG, at("translation row of range", m) + " must lie in [d * n + r, N)");
    for (int j = 0; j < 3; ++j) T.range_rows[static_cast<size_t>(j * n_ranges + m)] = a2i[static_cast<size_t>(row[j])];
    for (int f = 0; f < 2; ++f) {
      const double v = range_data[2 * m + f];
      if (!std::isfinite(v)) return fail(c, CORA_ERR_ARG, at("non-finite data of range", m));
      T.range_data[static_cast<size_t>(f * n_ranges + m)] = v;
    }
  }
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_measurements(c);
    c->meas = std::move(T);
    MeasurementTable &M = c->meas;  // (set stays false until every array is up: a failed upload leaves no table)
    HIP_TRY(c, to_device(&M.d_edge_rows, M.edge_rows));
    HIP_TRY(c, to_device(&M.d_edge_data, M.edge_data));
    HIP_TRY(c, to_device(&M.d_range_rows, M.range_rows));
    HIP_TRY(c, to_device(&M.d_range_data, M.range_data));
    HIP_TRY(c, alloc_device(&M.d_out, static_cast<size_t>(2 * n_edges + n_ranges + 3) * sizeof(double)));
    M.set = true;
  } else {
    c->tmap = TermMap();  // (a term map belongs to the table it was built from)
    c->odom = OdomTables();  // (so do the chain tables)
    c->ml = MlTables();      // (and the multilateration's lists)
    c->pl = PlTables();      // (and the chain placement's stages)
    c->sg = SgTables();      // (and the sighting placement's lists)
    c->cl = ClTables();      // (and the closure placement's lists)
    c->meas = std::move(T);
    c->meas.set = true;
  }
  return CORA_OK;
}

int cora_measurement_counts(const cora_ctx *c, int64_t out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->meas.set ? c->meas.n_edges : 0;
  out[1] = c->meas.set ? c->meas.n_ranges : 0;
  return CORA_OK;
}

int cora_measurement_residuals_dev(cora_ctx *c, const double *dX, int k, double *edge_rot, double *edge_trans,
                                   double *range_res, double sums[3]) {
  if (!c) return CORA_ERR_ARG;
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  NEED_DEVICE(c);
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  if (!dX) return fail(c, CORA_ERR_ARG, "null pointer");
  const MeasurementTable &M = c->meas;
  const int64_t ne = M.n_edges, nr = M.n_ranges;
  const int be = residual_blocks(ne), br = residual_blocks(nr);
  int rc = ensure_red(c, static_cast<size_t>(std::max(2 * be + br, 1)));
  if (rc) return rc;
  double *d_rot = M.d_out, *d_trn = M.d_out + ne, *d_rng = M.d_out + 2 * ne, *d_sums = M.d_out + 2 * ne + nr;
  HIP_TRY(c, hipMemsetAsync(d_sums, 0, 3 * sizeof(double), c->stream));  // (a kind without measurements has no launch)
  ResidualArgs A;
  A.d = c->F.L.d;
  A.ld = ld_for(k);
  A.k = k;
  A.X = dX;
  if (ne > 0) {
    A.n = ne;
    A.rows = M.d_edge_rows;
    A.data = M.d_edge_data;
    A.out0 = d_rot;
    A.out1 = d_trn;
    A.partial = c->d_red;
    HIP_TRY(c, launch_edge_residuals(A, c->stream));
    HIP_TRY(c, launch_reduce_partials(c->d_red, be, 2, d_sums, c->stream));
  }
  if (nr > 0) {
    A.n = nr;
    A.rows = M.d_range_rows;
    A.data = M.d_range_data;
    A.out0 = d_rng;
    A.out1 = nullptr;
    A.partial = c->d_red + 2 * be;
    HIP_TRY(c, launch_range_residuals(A, c->stream));
    HIP_TRY(c, launch_reduce_partials(c->d_red + 2 * be, br, 1, d_sums + 2, c->stream));
  }
  if (edge_rot && ne > 0) HIP_TRY(c, hipMemcpyAsync(edge_rot, d_rot, ne * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (edge_trans && ne > 0) HIP_TRY(c, hipMemcpyAsync(edge_trans, d_trn, ne * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (range_res && nr > 0) HIP_TRY(c, hipMemcpyAsync(range_res, d_rng, nr * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (sums) HIP_TRY(c, hipMemcpyAsync(sums, d_sums, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CORA_OK;
}

int cora_measurement_residuals(cora_ctx *c, const double *X, int ldx, int k, double *edge_rot, double *edge_trans,
                               double *range_res, double sums[3]) {
  if (!c) return CORA_ERR_ARG;
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  NEED_DEVICE(c);
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  double *dX;
  int rc;
  if ((rc = get_scratch(c, 0, ld_for(k), &dX))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  return cora_measurement_residuals_dev(c, dX, k, edge_rot, edge_trans, range_res, sums);
}

int cora_debug_measurement_residuals_host(cora_ctx *c, const double *X, int ldx, int k, double *edge_rot,
                                          double *edge_trans, double *range_res, double sums[3]) {
  if (!c) return CORA_ERR_ARG;
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (c->meas.host_stale)
    return fail(c, CORA_ERR_NOT_READY, "the host copy of the measurement table is stale (cora_assemble_values_dev rescaled the device's only)");
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  if (!X) return fail(c, CORA_ERR_ARG, "null pointer");
  const HostFormat &F = c->F;
  const int64_t N = F.L.N;
  if (ldx < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int ld = ld_for(k), d = F.L.d;
  std::vector<double> xi(static_cast<size_t>(F.L.rows) * ld, 0.0);  // X as a resident vector: internal row order, row-major
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i) xi[static_cast<size_t>(F.api2int[i]) * ld + cc] = X[static_cast<size_t>(cc) * ldx + i];
  auto x = [&](int32_t row, int col) { return xi[static_cast<size_t>(row) * ld + col]; };
  const MeasurementTable &M = c->meas;
  const int64_t ne = M.n_edges, nr = M.n_ranges;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = 0; e < ne; ++e) {
    const int32_t ra = M.edge_rows[e], rb = M.edge_rows[ne + e], ta = M.edge_rows[2 * ne + e], tb = M.edge_rows[3 * ne + e];
    auto field = [&](int f) { return M.edge_data[static_cast<size_t>(f) * ne + e]; };
    double rot = 0.0, trn = 0.0;
    for (int col = 0; col < k; ++col) {
      double diff = x(tb, col) - x(ta, col);
      for (int a = 0; a < d; ++a) diff -= field(d * d + a) * x(ra + a, col);
      trn += diff * diff;
      if (rb < 0) continue;
      for (int b = 0; b < d; ++b) {
        double q = x(rb + b, col);
        for (int a = 0; a < d; ++a) q -= field(a * d + b) * x(ra + a, col);
        rot += q * q;
      }
    }
    rot = rb < 0 ? 0.0 : field(d * d + d) * rot;
    trn *= field(d * d + d + 1);
    if (edge_rot) edge_rot[e] = rot;
    if (edge_trans) edge_trans[e] = trn;
    s[0] += rot;
    s[1] += trn;
  }
  for (int64_t m = 0; m < nr; ++m) {
    const int32_t rr = M.range_rows[m], ta = M.range_rows[nr + m], tb = M.range_rows[2 * nr + m];
    double res = 0.0;
    for (int col = 0; col < k; ++col) {
      const double diff = x(tb, col) - x(ta, col) + M.range_data[m] * x(rr, col);
      res += diff * diff;
    }
    res *= M.range_data[nr + m];
    if (range_res) range_res[m] = res;
    s[2] += res;
  }
  if (sums) std::copy(s, s + 3, sums);
  return CORA_OK;
}
