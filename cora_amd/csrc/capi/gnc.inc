// Part of capi.hip (one translation unit; included there, in this order).  the weight step of a robust-cost (GNC) loop: unweighted residuals -> ratios -> weights and their statistics; device-pointer form, host-pointer form, host mirror.  Reads the table's structure and the term map's base precisions; writes nothing of the handle.

namespace {

// what the three forms check alike (everything but the device and the pointers)
int gnc_check(cora_ctx *c, int k, int cost, double mu) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the GNC weight step is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (!c->tmap.built) return fail(c, CORA_ERR_NOT_READY, "no term map yet: call cora_assembly_build first");
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  if (cost != CORA_GNC_NONE && cost != CORA_GNC_TLS && cost != CORA_GNC_GM) return fail(c, CORA_ERR_ARG, "unknown GNC cost");
  if (cost != CORA_GNC_NONE && !(std::isfinite(mu) && mu > 0.0)) return fail(c, CORA_ERR_ARG, "mu must be finite and > 0");
  return CORA_OK;
}

int gnc_flag_error(cora_ctx *c, int flag) {
  if (flag & 2) return fail(c, CORA_ERR_ARG, "a threshold is NaN or <= 0");
  if (flag & 1) return fail(c, CORA_ERR_NAN, "a residual is not finite");
  return CORA_OK;
}

// the device's order of the 12 statistics ({sum w r^2, n_mid, n_out} of rot, trans, range | max rho of rot, trans, range)
// to stats[3][4] = {sum_wr2, max_rho, n_mid, n_out}
void gnc_stats_out(const double *dev, double *stats) {
  for (int s = 0; s < 3; ++s) {
    stats[4 * s + 0] = dev[3 * s + 0];
    stats[4 * s + 1] = dev[9 + s];
    stats[4 * s + 2] = dev[3 * s + 1];
    stats[4 * s + 3] = dev[3 * s + 2];
  }
}

}  // namespace

int cora_gnc_weights_dev(cora_ctx *c, const double *dX, int k, const double *d_barc2, int cost, int couple_edges, double mu,
                         double *d_w_out, double *d_r2_out, double stats[12]) {
  if (!c) return CORA_ERR_ARG;
  int rc = gnc_check(c, k, cost, mu);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!dX || !d_barc2 || !d_w_out) return fail(c, CORA_ERR_ARG, "null pointer");
  const MeasurementTable &M = c->meas;
  const int64_t ne = M.n_edges, nr = M.n_ranges;
  const int be = residual_blocks(ne), br = residual_blocks(nr);
  // d_red: the edges' partials [8][be] | the ranges' [4][br] | the 12 statistics in the device's order
  const size_t off_rng = static_cast<size_t>(8) * be, off_stats = off_rng + static_cast<size_t>(4) * br;
  if ((rc = ensure_red(c, off_stats + 12))) return rc;
  double *d_stats = c->d_red + off_stats;
  HIP_TRY(c, hipMemsetAsync(d_stats, 0, 12 * sizeof(double), c->stream));  // (a kind without measurements has no launch)
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  GncArgs A;
  A.R.d = c->F.L.d;
  A.R.ld = ld_for(k);
  A.R.k = k;
  A.R.X = dX;
  A.cost = cost;
  A.couple = couple_edges != 0;
  A.mu = mu;
  A.flag = c->d_flag;
  if (ne > 0) {
    A.R.n = ne;
    A.R.rows = M.d_edge_rows;
    A.R.data = M.d_edge_data;
    A.base = c->d_tbase;
    A.barc2 = d_barc2;
    A.w = d_w_out;
    A.r2 = d_r2_out;
    A.partial = c->d_red;
    HIP_TRY(c, launch_gnc_edges(A, c->stream));
    HIP_TRY(c, launch_reduce_partials(c->d_red, be, 6, d_stats, c->stream));
    HIP_TRY(c, launch_reduce_max_partials(c->d_red + static_cast<size_t>(6) * be, be, 2, d_stats + 9, c->stream));
  }
  if (nr > 0) {
    A.R.n = nr;
    A.R.rows = M.d_range_rows;
    A.R.data = M.d_range_data;
    A.base = c->d_tbase + 2 * ne;
    A.barc2 = d_barc2 + 2 * ne;
    A.w = d_w_out + 2 * ne;
    A.r2 = d_r2_out ? d_r2_out + 2 * ne : nullptr;
    A.partial = c->d_red + off_rng;
    HIP_TRY(c, launch_gnc_ranges(A, c->stream));
    HIP_TRY(c, launch_reduce_partials(c->d_red + off_rng, br, 3, d_stats + 6, c->stream));
    HIP_TRY(c, launch_reduce_max_partials(c->d_red + off_rng + static_cast<size_t>(3) * br, br, 1, d_stats + 11, c->stream));
  }
  double dev[12];
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (stats) HIP_TRY(c, hipMemcpyAsync(dev, d_stats, sizeof(dev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((rc = gnc_flag_error(c, *c->h_flag))) return rc;
  if (stats) gnc_stats_out(dev, stats);
  return CORA_OK;
}

int cora_gnc_weights(cora_ctx *c, const double *X, int ldx, int k, const double *barc2, int cost, int couple_edges, double mu,
                     double *w_out, double *r2_out, double stats[12]) {
  if (!c) return CORA_ERR_ARG;
  int rc = gnc_check(c, k, cost, mu);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!X || !barc2 || !w_out) return fail(c, CORA_ERR_ARG, "null pointer");
  const size_t nw = static_cast<size_t>(c->tmap.n_weights);
  if (!c->d_gnc) HIP_TRY(c, alloc_device(&c->d_gnc, std::max<size_t>(3 * nw, 1) * sizeof(double)));
  double *d_barc2 = c->d_gnc, *d_w = c->d_gnc + nw, *d_r2 = c->d_gnc + 2 * nw;
  double *dX;
  if ((rc = get_scratch(c, 0, ld_for(k), &dX))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  if (nw > 0) HIP_TRY(c, hipMemcpyAsync(d_barc2, barc2, nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = cora_gnc_weights_dev(c, dX, k, d_barc2, cost, couple_edges, mu, d_w, r2_out ? d_r2 : nullptr, stats))) return rc;
  if (nw > 0) HIP_TRY(c, hipMemcpyAsync(w_out, d_w, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (nw > 0 && r2_out) HIP_TRY(c, hipMemcpyAsync(r2_out, d_r2, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CORA_OK;
}

// The device's sequence on the host, operation for operation, so that the mirror gives the device's bits: a measurement's
// columns go in pieces of W = 2 (even row stride) or 1 to 8 lanes, lane g takes pieces g, g + 8, ..., every step is the
// kernels' fma, and the lanes are added as the butterfly over the distances 4, 2, 1 adds them.  The precisions are the
// term map's base ones; the table's rows, R, t and r never change, so a stale host copy of kappa, tau and omega does not
// matter: they are not read.  Then gnc_ratio / gnc_weight (kernels.h); the statistics are summed in measurement order.
int cora_debug_gnc_weights_host(cora_ctx *c, const double *X, int ldx, int k, const double *barc2, int cost, int couple_edges,
                                double mu, double *w_out, double *r2_out, double stats[12]) {
  if (!c) return CORA_ERR_ARG;
  const int rc = gnc_check(c, k, cost, mu);
  if (rc) return rc;
  if (!X || !barc2 || !w_out) return fail(c, CORA_ERR_ARG, "null pointer");
  const HostFormat &F = c->F;
  const int64_t N = F.L.N;
  if (ldx < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int ld = ld_for(k), d = F.L.d;
  std::vector<double> xi(static_cast<size_t>(F.L.rows) * ld, 0.0);  // X as a resident vector: internal row order, row-major
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i) xi[static_cast<size_t>(F.api2int[i]) * ld + cc] = X[static_cast<size_t>(cc) * ldx + i];
  auto x = [&](int32_t row, int col) { return xi[static_cast<size_t>(row) * ld + col]; };
  const MeasurementTable &M = c->meas;
  const std::vector<double> &base = c->tmap.base;
  const int64_t ne = M.n_edges, nr = M.n_ranges;
  const int W = ld % 2 == 0 ? 2 : 1, pieces = (k + W - 1) / W;
  auto butterfly = [](const double (&v)[kResidualLanes]) { return ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7])); };
  double st[3][4] = {};
  int bad = 0;
  auto tally = [&](int seg, double w, double ratio) {
    if (w > 0.0 && w < 1.0) st[seg][2] += 1.0;
    if (w < 0.5) st[seg][3] += 1.0;
    st[seg][1] = std::fmax(st[seg][1], ratio);
  };
  for (int64_t e = 0; e < ne; ++e) {
    const int32_t ra = M.edge_rows[e], rb = M.edge_rows[ne + e], ta = M.edge_rows[2 * ne + e], tb = M.edge_rows[3 * ne + e];
    auto field = [&](int f) { return M.edge_data[static_cast<size_t>(f) * ne + e]; };
    double lr[kResidualLanes] = {}, lt[kResidualLanes] = {};
    for (int v = 0; v < pieces; ++v) {
      double &rot_l = lr[v % kResidualLanes], &trn_l = lt[v % kResidualLanes];
      const int c0 = v * W, c1 = std::min(c0 + W, k);
      for (int col = c0; col < c1; ++col) {
        double diff = x(tb, col) - x(ta, col);
        for (int a = 0; a < d; ++a) diff = std::fma(-field(d * d + a), x(ra + a, col), diff);
        trn_l = std::fma(diff, diff, trn_l);
      }
      if (rb < 0) continue;
      for (int b = 0; b < d; ++b)
        for (int col = c0; col < c1; ++col) {
          double q = x(rb + b, col);
          for (int a = 0; a < d; ++a) q = std::fma(-field(a * d + b), x(ra + a, col), q);
          rot_l = std::fma(q, q, rot_l);
        }
    }
    double rot = butterfly(lr), trn = butterfly(lt);
    rot = rb < 0 ? 0.0 : base[static_cast<size_t>(e)] * rot;
    trn = base[static_cast<size_t>(ne + e)] * trn;
    double w_rot, w_trn;
    if (couple_edges) {
      const double ratio = gnc_ratio(gnc_coupled_r2(rot, trn), barc2[ne + e], bad);
      w_rot = w_trn = gnc_weight(cost, mu, ratio);
      tally(1, w_trn, ratio);
    } else {
      const double ratio_rot = gnc_ratio(rot, barc2[e], bad), ratio_trn = gnc_ratio(trn, barc2[ne + e], bad);
      w_rot = gnc_weight(cost, mu, ratio_rot);
      w_trn = gnc_weight(cost, mu, ratio_trn);
      tally(0, w_rot, ratio_rot);
      tally(1, w_trn, ratio_trn);
    }
    st[0][0] += w_rot * rot;
    st[1][0] += w_trn * trn;
    w_out[e] = w_rot;
    w_out[ne + e] = w_trn;
    if (r2_out) {
      r2_out[e] = rot;
      r2_out[ne + e] = trn;
    }
  }
  for (int64_t m = 0; m < nr; ++m) {
    const int32_t rr = M.range_rows[m], ta = M.range_rows[nr + m], tb = M.range_rows[2 * nr + m];
    double ls[kResidualLanes] = {};
    for (int v = 0; v < pieces; ++v)
      for (int col = v * W; col < std::min(v * W + W, k); ++col) {
        const double diff = std::fma(M.range_data[m], x(rr, col), x(tb, col) - x(ta, col));
        ls[v % kResidualLanes] = std::fma(diff, diff, ls[v % kResidualLanes]);
      }
    const double res = base[static_cast<size_t>(2 * ne + m)] * butterfly(ls);
    const double ratio = gnc_ratio(res, barc2[2 * ne + m], bad);
    const double w = gnc_weight(cost, mu, ratio);
    tally(2, w, ratio);
    st[2][0] += w * res;
    w_out[2 * ne + m] = w;
    if (r2_out) r2_out[2 * ne + m] = res;
  }
  if (const int err = gnc_flag_error(c, bad)) return err;
  if (stats) std::copy(&st[0][0], &st[0][0] + 12, stats);
  return CORA_OK;
}
