// Part of capi.hip (one translation unit; included there, in this order).  relative pose error of an estimate against a reference over a table of pose pairs kept on the handle: the table, device-pointer form, host-pointer form, host mirror.  Reads the pose table of the comparison; writes nothing the handle computes with.

namespace {

// what the three forms check alike (everything but the device and the pointers)
int rpe_check(cora_ctx *c, int k, int kr) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the relative pose error is not supported on partitioned handles");
  if (k <= 0 || k > kMaxLD || kr <= 0 || kr > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column counts must lie in [1, 24]");
  if (!c->pairs.set) return fail(c, CORA_ERR_NOT_READY, "no pair table (cora_set_pose_pairs)");
  return CORA_OK;
}

// The d^2 + d sums of one pair for one vector as lane 0 of the pair's group holds them after the butterfly (k_rpe,
// kernels/rpe.inc): V is a resident vector on the host (internal rows, row-major, stride ld); lane g takes the pieces
// g, g + 8, ... of W columns (W = 2 at an even stride), one fma per term in column order; the lanes are added as
// ((l0 + l4) + (l2 + l6)) + ((l1 + l5) + (l3 + l7)), which is what the distances 4, 2, 1 leave in lane 0.
void rpe_host_sums(const double *V, int ld, int k, int d, int32_t ri, int32_t ti, int32_t rj, int32_t tj, double *s) {
  const int W = ld % 2 == 0 ? 2 : 1, ns = d * d + d, pieces = (k + W - 1) / W;
  double lane[kResidualLanes][12];
  auto at = [&](int32_t row, int col) { return col < k ? V[static_cast<size_t>(row) * ld + col] : 0.0; };  // (res_load: columns from k on are 0)
  for (int g = 0; g < kResidualLanes; ++g) {
    double *sg = lane[g];
    std::fill(sg, sg + ns, 0.0);
    for (int v = g; v < pieces; v += kResidualLanes)
      for (int col = v * W; col < v * W + W; ++col) {
        const double dx = at(tj, col) - at(ti, col);
        for (int a = 0; a < d; ++a) {
          const double via = at(ri + a, col);
          for (int b = 0; b < d; ++b) sg[a * d + b] = std::fma(via, at(rj + b, col), sg[a * d + b]);
          sg[d * d + a] = std::fma(via, dx, sg[d * d + a]);
        }
      }
  }
  for (int q = 0; q < ns; ++q) {
    const double a0 = lane[0][q] + lane[4][q], a1 = lane[1][q] + lane[5][q], a2 = lane[2][q] + lane[6][q], a3 = lane[3][q] + lane[7][q];
    const double b0 = a0 + a2, b1 = a1 + a3;
    s[q] = b0 + b1;
  }
}

}  // namespace

int cora_set_pose_pairs(cora_ctx *c, int64_t m, const int32_t *pairs) {
  if (!c) return CORA_ERR_ARG;
  const Layout &L = c->F.L;
  if (L.world > 1) return fail(c, CORA_ERR_ARG, "pair tables are not supported on partitioned handles");
  if (m < 0) return fail(c, CORA_ERR_ARG, "negative pair count");
  if (m > kRpeMaxPairs) return fail(c, CORA_ERR_ARG, "more than 2^30 pairs");
  if (m > 0 && !pairs) return fail(c, CORA_ERR_ARG, "null pointer");
  PosePairTable T;
  if (m > 0) {
    if (const int rc = compare_pose_table(c)) return rc;
    const int32_t *rot = c->cmp_rows.data(), *trn = rot + L.n;
    T.m = m;
    T.api.assign(pairs, pairs + 2 * m);
    T.rows.resize(static_cast<size_t>(4 * m));
    for (int64_t p = 0; p < m; ++p) {
      const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
      if (i < 0 || i >= L.n || j < 0 || j >= L.n)
        return fail(c, CORA_ERR_ARG, "pair " + std::to_string(p) + " = (" + std::to_string(i) + ", " + std::to_string(j) +
                                         "): pose indices must lie in [0, " + std::to_string(L.n) + ")");
      T.rows[static_cast<size_t>(p)] = rot[i];
      T.rows[static_cast<size_t>(m + p)] = trn[i];
      T.rows[static_cast<size_t>(2 * m + p)] = rot[j];
      T.rows[static_cast<size_t>(3 * m + p)] = trn[j];
    }
  }
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_tables(c->pairs);
    if (m == 0) return CORA_OK;
    c->pairs = std::move(T);
    PosePairTable &P = c->pairs;  // (set stays false until every array is up: a failed upload leaves no table)
    HIP_TRY(c, to_device(&P.d_rows, P.rows));
    HIP_TRY(c, alloc_device(&P.d_err, static_cast<size_t>(2 * m + 5) * sizeof(double)));
    P.set = true;
  } else {
    c->pairs = std::move(T);
    c->pairs.set = m > 0;
  }
  return CORA_OK;
}

int cora_pose_pairs_count(const cora_ctx *c, int64_t *m) {
  if (!c || !m) return CORA_ERR_ARG;
  *m = c->pairs.set ? c->pairs.m : 0;
  return CORA_OK;
}

int cora_pose_pairs_equal(const cora_ctx *c, int64_t m, const int32_t *pairs, int *equal) {
  if (!c || !equal || m < 0 || (m > 0 && !pairs)) return CORA_ERR_ARG;
  const PosePairTable &P = c->pairs;
  *equal = (P.set ? P.m : 0) == m && (m == 0 || std::equal(pairs, pairs + 2 * m, P.api.begin())) ? 1 : 0;
  return CORA_OK;
}

int cora_rpe_dev(cora_ctx *c, const double *dX, int k, const double *dRef, int kr, double *trans_err, double *rot_err, double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = rpe_check(c, k, kr);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!dX || !dRef || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const PosePairTable &P = c->pairs;
  const int64_t m = P.m;
  const int nb = rpe_blocks(m);
  if ((rc = ensure_red(c, static_cast<size_t>(5) * nb))) return rc;
  double *d_et = P.d_err, *d_er = d_et + m, *d_stats = d_er + m;
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  RpeArgs A;
  A.m = m;
  A.d = c->F.L.d;
  A.k = k;
  A.ldx = ld_for(k);
  A.kr = kr;
  A.ldr = ld_for(kr);
  A.X = dX;
  A.Ref = dRef;
  A.rows = P.d_rows;
  A.et = d_et;
  A.er = d_er;
  A.partial = c->d_red;
  A.flag = c->d_flag;
  HIP_TRY(c, launch_rpe(A, c->stream));
  HIP_TRY(c, launch_rpe_finish(c->d_red, nb, m, d_stats, c->stream));
  double st[5];
  HIP_TRY(c, hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (trans_err) HIP_TRY(c, hipMemcpyAsync(trans_err, d_et, static_cast<size_t>(m) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (rot_err) HIP_TRY(c, hipMemcpyAsync(rot_err, d_er, static_cast<size_t>(m) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_flag || !std::isfinite(st[0]) || !std::isfinite(st[1])) return fail(c, CORA_ERR_NAN, "a relative pose error or a sum of their squares is not finite");
  out[0] = static_cast<double>(m);
  out[1] = st[0];
  out[2] = st[2];
  out[3] = st[1];
  out[4] = st[3];
  out[5] = st[4];
  return CORA_OK;
}

int cora_rpe(cora_ctx *c, const double *X, int ldx, int k, const double *Ref, int ldref, int kr, double *trans_err, double *rot_err,
             double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = rpe_check(c, k, kr);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!X || !Ref || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  double *dX, *dRef;
  if ((rc = compare_vec(c, 2, ld_for(k), &dX)) || (rc = compare_vec(c, 3, ld_for(kr), &dRef))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the two uploads share one staging buffer)
  if ((rc = upload_impl(c, Ref, ldref, kr, dRef))) return rc;
  rc = cora_rpe_dev(c, dX, k, dRef, kr, trans_err, rot_err, out);
  // the two vectors of this form are not kept: a caller that evaluates often stays resident and uses cora_rpe_dev
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 2, 4, 0);
  return rc;
}

// The same operations on the host through the translated table.  A pair's two errors have the device's bits: the lane
// pieces, the fma order and the butterfly of k_rpe are mirrored (rpe_host_sums).  The two sums of squares are added in
// PAIR order, not in the device's block order: they agree with the device's within m eps times the sum, not bit for bit;
// the maxima and the first maximum are exact functions of the per-pair values and agree exactly.
int cora_debug_rpe_host(cora_ctx *c, const double *X, int ldx, int k, const double *Ref, int ldref, int kr, double *trans_err,
                        double *rot_err, double *out) {
  if (!c) return CORA_ERR_ARG;
  const int rc = rpe_check(c, k, kr);
  if (rc) return rc;
  if (!X || !Ref || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const HostFormat &F = c->F;
  const int64_t N = F.L.N;
  if (ldx < N || ldref < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = F.L.d, ldxi = ld_for(k), ldri = ld_for(kr), ns = d * d + d;
  // X and Ref as resident vectors: internal row order, row-major
  std::vector<double> xi(static_cast<size_t>(F.L.rows) * ldxi, 0.0), gi(static_cast<size_t>(F.L.rows) * ldri, 0.0);
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i) xi[static_cast<size_t>(F.api2int[i]) * ldxi + cc] = X[static_cast<size_t>(cc) * ldx + i];
  for (int cc = 0; cc < kr; ++cc)
    for (int64_t i = 0; i < N; ++i) gi[static_cast<size_t>(F.api2int[i]) * ldri + cc] = Ref[static_cast<size_t>(cc) * ldref + i];
  const PosePairTable &P = c->pairs;
  const int64_t m = P.m;
  double st[4] = {0.0, 0.0, 0.0, 0.0}, first = 0.0;
  bool bad = false;
  for (int64_t p = 0; p < m; ++p) {
    const int32_t ri = P.rows[p], ti = P.rows[m + p], rj = P.rows[2 * m + p], tj = P.rows[3 * m + p];
    double et = 0.0, er = 0.0;
    if (ri != rj) {
      double sx[12], sr[12], r2 = 0.0, t2 = 0.0;
      rpe_host_sums(xi.data(), ldxi, k, d, ri, ti, rj, tj, sx);
      rpe_host_sums(gi.data(), ldri, kr, d, ri, ti, rj, tj, sr);
      for (int q = 0; q < d * d; ++q) {
        const double diff = sx[q] - sr[q];
        r2 = std::fma(diff, diff, r2);
      }
      for (int q = d * d; q < ns; ++q) {
        const double diff = sx[q] - sr[q];
        t2 = std::fma(diff, diff, t2);
      }
      et = std::sqrt(t2);
      er = std::sqrt(r2);
    }
    bad = bad || !std::isfinite(et) || !std::isfinite(er);
    if (trans_err) trans_err[p] = et;
    if (rot_err) rot_err[p] = er;
    const double et2 = et * et, er2 = er * er;
    st[0] += et2;
    st[1] += er2;
    if (et > st[2]) {
      st[2] = et;
      first = static_cast<double>(p);
    }
    st[3] = std::fmax(st[3], er);
  }
  if (bad || !std::isfinite(st[0]) || !std::isfinite(st[1])) return fail(c, CORA_ERR_NAN, "a relative pose error or a sum of their squares is not finite");
  out[0] = static_cast<double>(m);
  out[1] = st[0];
  out[2] = st[2];
  out[3] = st[1];
  out[4] = st[3];
  out[5] = first;
  return CORA_OK;
}
