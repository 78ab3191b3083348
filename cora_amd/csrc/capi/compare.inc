// Part of capi.hip (one translation unit; included there, in this order).  comparison of an estimate with a reference (normally ground truth) after an orthogonal alignment on the selected poses' positions: device-pointer form, host-pointer form, host form.  Reads the row maps; writes nothing of the handle.

namespace {

constexpr int kCompareHead = 8;  // m, sum et^2, max et, sum er^2, max er, selected landmarks, sum el^2, max el

// what the three forms check alike (everything but the device and the pointers)
int compare_check(cora_ctx *c, int k, int kr, int flags) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the trajectory comparison is not supported on partitioned handles");
  if (k <= 0 || k > kMaxLD || kr <= 0 || kr > k) return fail(c, CORA_ERR_SHAPE, "column counts must satisfy 1 <= kr <= k <= 24");
  if (flags & ~CORA_COMPARE_PROPER) return fail(c, CORA_ERR_ARG, "unknown flag");
  if ((flags & CORA_COMPARE_PROPER) && k != kr) return fail(c, CORA_ERR_ARG, "CORA_COMPARE_PROPER needs k == kr");
  return CORA_OK;
}

// number of selected poses and landmarks; sel (nt bytes, 0 / 1) filled from `select` (NULL: all ones)
void compare_selection(const Layout &L, const unsigned char *select, std::vector<unsigned char> &sel, int64_t &m, int64_t &ml) {
  sel.resize(static_cast<size_t>(L.nt));
  m = ml = 0;
  for (int i = 0; i < L.nt; ++i) {
    sel[static_cast<size_t>(i)] = select ? (select[i] != 0) : 1;
    (i < L.n ? m : ml) += sel[static_cast<size_t>(i)];
  }
}

bool all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// The one-sided Jacobi both compare_align and the rounding's basis (capi/round.inc) run: H (k x kr row-major, k >= kr,
// finite) is divided by its largest |entry| (returned) and its columns are rotated until every pair is orthogonal to
// working precision; U: the rotated columns (k x kr row-major), V: the accumulated rotations (kr x kr row-major), so that
// H / scale = U V^T with the columns of U orthogonal.
double compare_jacobi(int k, int kr, const double *H, std::vector<double> &U, std::vector<double> &V) {
  U.assign(H, H + static_cast<size_t>(k) * kr);
  V.assign(static_cast<size_t>(kr) * kr, 0.0);
  for (int j = 0; j < kr; ++j) V[static_cast<size_t>(j) * kr + j] = 1.0;
  double scale = 0.0;
  for (double v : U) scale = std::max(scale, std::fabs(v));
  if (scale > 0.0)
    for (double &v : U) v /= scale;
  const double eps = 2.220446049250313e-16;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p + 1 < kr; ++p)
      for (int q = p + 1; q < kr; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < k; ++i) {
          const double up = U[static_cast<size_t>(i) * kr + p], uq = U[static_cast<size_t>(i) * kr + q];
          alpha += up * up;
          beta += uq * uq;
          gamma += up * uq;
        }
        if (gamma == 0.0 || std::fabs(gamma) <= 0.25 * eps * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < k; ++i) {
          double &up = U[static_cast<size_t>(i) * kr + p], &uq = U[static_cast<size_t>(i) * kr + q];
          const double a = up, b = uq;
          up = cs * a - sn * b;
          uq = sn * a + cs * b;
        }
        for (int i = 0; i < kr; ++i) {
          double &vp = V[static_cast<size_t>(i) * kr + p], &vq = V[static_cast<size_t>(i) * kr + q];
          const double a = vp, b = vq;
          vp = cs * a - sn * b;
          vq = sn * a + cs * b;
        }
      }
    if (!rotated) break;
  }
  return scale;
}

// A = U D V^T of the thin SVD H = U Sigma V^T (H: k x kr row-major, k >= kr, finite), D = I or, with `proper` (k == kr),
// diag(1, .., 1, det(U V^T)); sigma: the kr singular values, descending; A: k x kr row-major.  One-sided Jacobi on the
// columns of H (rotations until every pair is orthogonal to working precision), which also leaves the columns that
// belong to tiny singular values orthogonal to the others to working precision; a column that is exactly null (one pose:
// H = 0) is replaced by the unit vector with the largest remainder against the columns already there, so A^T A = I
// whatever the rank.
void compare_align(int k, int kr, const double *H, bool proper, double *A, double *sigma) {
  std::vector<double> U, V;
  const double scale = compare_jacobi(k, kr, H, U, V);
  std::vector<double> norm(static_cast<size_t>(kr));
  std::vector<int> order(static_cast<size_t>(kr));
  for (int j = 0; j < kr; ++j) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += U[static_cast<size_t>(i) * kr + j] * U[static_cast<size_t>(i) * kr + j];
    norm[static_cast<size_t>(j)] = std::sqrt(s);
    order[static_cast<size_t>(j)] = j;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return norm[static_cast<size_t>(a)] > norm[static_cast<size_t>(b)]; });
  // Us, Vs: the columns in descending order of the singular value, U's normalised (null ones completed)
  std::vector<double> Us(static_cast<size_t>(k) * kr, 0.0), Vs(static_cast<size_t>(kr) * kr, 0.0);
  for (int j = 0; j < kr; ++j) {
    const int src = order[static_cast<size_t>(j)];
    const double nj = norm[static_cast<size_t>(src)];
    sigma[j] = nj * scale;
    for (int i = 0; i < kr; ++i) Vs[static_cast<size_t>(i) * kr + j] = V[static_cast<size_t>(i) * kr + src];
    if (nj > 1e-150) {
      for (int i = 0; i < k; ++i) Us[static_cast<size_t>(i) * kr + j] = U[static_cast<size_t>(i) * kr + src] / nj;
      continue;
    }
    sigma[j] = 0.0;
    std::vector<double> best(static_cast<size_t>(k), 0.0), v(static_cast<size_t>(k));
    double best_norm = -1.0;
    for (int unit = 0; unit < k; ++unit) {
      std::fill(v.begin(), v.end(), 0.0);
      v[static_cast<size_t>(unit)] = 1.0;
      for (int pass = 0; pass < 2; ++pass)  // (twice: the second pass removes what rounding left of the first)
        for (int done = 0; done < j; ++done) {
          double dot = 0.0;
          for (int i = 0; i < k; ++i) dot += Us[static_cast<size_t>(i) * kr + done] * v[static_cast<size_t>(i)];
          for (int i = 0; i < k; ++i) v[static_cast<size_t>(i)] -= dot * Us[static_cast<size_t>(i) * kr + done];
        }
      double s = 0.0;
      for (double x : v) s += x * x;
      if (s > best_norm) {
        best_norm = s;
        best = v;
      }
    }
    const double bn = std::sqrt(best_norm);
    for (int i = 0; i < k; ++i) Us[static_cast<size_t>(i) * kr + j] = best[static_cast<size_t>(i)] / bn;
  }
  auto form = [&](double last) {
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < kr; ++b) {
        double s = 0.0;
        for (int j = 0; j < kr; ++j)
          s += Us[static_cast<size_t>(a) * kr + j] * (j == kr - 1 ? last : 1.0) * Vs[static_cast<size_t>(b) * kr + j];
        A[static_cast<size_t>(a) * kr + b] = s;
      }
  };
  form(1.0);
  if (!proper) return;
  // sign of det(U V^T): elimination with partial pivoting on a copy (k == kr)
  std::vector<double> M(A, A + static_cast<size_t>(k) * k);
  double sign = 1.0;
  for (int col = 0; col < k; ++col) {
    int piv = col;
    for (int i = col + 1; i < k; ++i)
      if (std::fabs(M[static_cast<size_t>(i) * k + col]) > std::fabs(M[static_cast<size_t>(piv) * k + col])) piv = i;
    if (piv != col) {
      for (int j = 0; j < k; ++j) std::swap(M[static_cast<size_t>(piv) * k + j], M[static_cast<size_t>(col) * k + j]);
      sign = -sign;
    }
    const double pv = M[static_cast<size_t>(col) * k + col];
    if (pv < 0.0) sign = -sign;
    if (pv == 0.0) break;  // (cannot happen for an orthogonal matrix)
    for (int i = col + 1; i < k; ++i) {
      const double f = M[static_cast<size_t>(i) * k + col] / pv;
      for (int j = col; j < k; ++j) M[static_cast<size_t>(i) * k + j] -= f * M[static_cast<size_t>(col) * k + j];
    }
  }
  if (sign < 0.0) form(-1.0);
}

// out[kCompareHead ..]: sigma | mean of x | mean of g | A column-major
void compare_tail_out(int k, int kr, const double *sigma, const double *xbar, const double *gbar, const double *A, double *out) {
  double *o = out + kCompareHead;
  o = std::copy(sigma, sigma + kr, o);
  o = std::copy(xbar, xbar + k, o);
  o = std::copy(gbar, gbar + kr, o);
  for (int b = 0; b < kr; ++b)
    for (int a = 0; a < k; ++a) *o++ = A[static_cast<size_t>(a) * kr + b];
}

// the pose table (host copy), built at the first call; shared with the pair table of capi/rpe.inc
int compare_pose_table(cora_ctx *c) {
  const Layout &L = c->F.L;
  const int d = L.d;
  if (c->cmp_rows.empty()) {
    const std::vector<int32_t> &a2i = c->F.api2int;
    const int64_t dn = static_cast<int64_t>(d) * L.n, t0 = dn + L.r;
    std::vector<int32_t> rows(static_cast<size_t>(L.n) + L.nt + L.r + 1);
    for (int i = 0; i < L.n; ++i) {
      const int32_t first = a2i[static_cast<size_t>(d) * i];
      for (int j = 1; j < d; ++j)
        if (a2i[static_cast<size_t>(d) * i + j] != first + j)
          return fail(c, CORA_ERR_ARG, "the rotation rows of pose " + std::to_string(i) + " are not consecutive in the internal order");
      rows[static_cast<size_t>(i)] = first;
    }
    for (int i = 0; i < L.nt; ++i) rows[static_cast<size_t>(L.n) + i] = a2i[static_cast<size_t>(t0 + i)];
    for (int i = 0; i < L.r; ++i) rows[static_cast<size_t>(L.n) + L.nt + i] = a2i[static_cast<size_t>(dn + i)];
    for (size_t i = 0; i + 1 < rows.size(); ++i)
      if (rows[i] < 0 || rows[i] >= L.rows) return fail(c, CORA_ERR_ARG, "row map out of range");
    c->cmp_rows = std::move(rows);
  }
  return CORA_OK;
}

// the pose table and the buffers of the device forms, built at the first call
int compare_prepare(cora_ctx *c) {
  const Layout &L = c->F.L;
  if (const int rc = compare_pose_table(c)) return rc;
  if (!c->d_cmp_rows) HIP_TRY(c, to_device(&c->d_cmp_rows, c->cmp_rows));
  if (!c->d_cmp_sel) HIP_TRY(c, alloc_device(&c->d_cmp_sel, std::max<size_t>(L.nt, 1)));
  if (!c->d_cmp)
    HIP_TRY(c, alloc_device(&c->d_cmp, (static_cast<size_t>(L.n) + L.nt + 2 * kMaxLD + 6 + kMaxLD * kMaxLD) * sizeof(double)));
  return need_gram(c);
}

int compare_vec(cora_ctx *c, int slot, int ld, double **out) {
  HIP_TRY(c, c->cmp_vec[slot].ensure(vec_bytes(c, ld)));
  *out = c->cmp_vec[slot];
  return CORA_OK;
}

// frees the pass's vectors [from, to) that are larger than min_bytes (the stream must be idle)
void compare_release(cora_ctx *c, int from, int to, size_t min_bytes) {
  for (int slot = from; slot < to; ++slot) c->cmp_vec[slot].release_above(min_bytes);
}
constexpr size_t kCompareKeepBytes = static_cast<size_t>(256) << 20;  // centred vectors above this are not kept between calls

bool overlaps(const double *a, size_t a_bytes, const double *b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

int cora_compare_dev(cora_ctx *c, const double *dX, int k, const double *dRef, int kr, const unsigned char *select, int flags,
                     double *pose_trans_err, double *pose_rot_err, double *landmark_err, double *dAligned, double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = compare_check(c, k, kr, flags);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!dX || !dRef || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const Layout &L = c->F.L;
  const int ldx = ld_for(k), ldr = ld_for(kr);
  if (dAligned && (overlaps(dAligned, vec_bytes(c, ldr), dX, vec_bytes(c, ldx)) || overlaps(dAligned, vec_bytes(c, ldr), dRef, vec_bytes(c, ldr))))
    return fail(c, CORA_ERR_ARG, "the aligned vector must not alias the estimate or the reference");
  int64_t m = 0, ml = 0;
  compare_selection(L, select, c->cmp_sel_host, m, ml);
  if (m == 0) return fail(c, CORA_ERR_ARG, "no pose selected");
  if ((rc = compare_prepare(c))) return rc;
  const int n = L.n, nt = L.nt, nl = nt - n;
  const int b_pose = compare_blocks(n), b_err = compare_blocks(static_cast<int64_t>(nt) + (dAligned ? L.r : 0));
  const int gram_blocks = 256, nel = k * kr;
  if ((rc = ensure_red(c, std::max<size_t>({static_cast<size_t>(k + kr) * b_pose, static_cast<size_t>(nel) * gram_blocks + nel,
                                            static_cast<size_t>(6) * b_err}))))
    return rc;
  double *Xc, *Gc;
  if ((rc = compare_vec(c, 0, ldx, &Xc)) || (rc = compare_vec(c, 1, ldr, &Gc))) return rc;
  double *d_et = c->d_cmp, *d_er = d_et + n, *d_el = d_er + n, *d_sums = d_el + nl, *d_stats = d_sums + 2 * kMaxLD, *d_A = d_stats + 6;
  HIP_TRY(c, hipMemcpyAsync(c->d_cmp_sel, c->cmp_sel_host.data(), static_cast<size_t>(nt), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(Xc, 0, vec_bytes(c, ldx), c->stream));
  HIP_TRY(c, hipMemsetAsync(Gc, 0, vec_bytes(c, ldr), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  CompareArgs A;
  A.d = L.d;
  A.n = n;
  A.nt = nt;
  A.nr = L.r;
  A.k = k;
  A.ldx = ldx;
  A.kr = kr;
  A.ldr = ldr;
  A.X = dX;
  A.Ref = dRef;
  A.rot_row = c->d_cmp_rows;
  A.trn_row = c->d_cmp_rows + n;
  A.rng_row = c->d_cmp_rows + n + nt;
  A.sel = c->d_cmp_sel;
  A.m = static_cast<double>(m);
  A.sums = d_sums;
  A.A = d_A;
  A.Xc = Xc;
  A.Gc = Gc;
  A.et = d_et;
  A.er = d_er;
  A.el = d_el;
  A.aligned = dAligned;
  A.partial = c->d_red;
  A.flag = c->d_flag;
  // steps 1 and 2: column sums, centred rows, H = Xc^T Gc (row-major k x kr, straight into pinned memory)
  HIP_TRY(c, launch_compare_sums(A, c->stream));
  HIP_TRY(c, launch_reduce_partials(c->d_red, b_pose, k + kr, d_sums, c->stream));
  HIP_TRY(c, launch_compare_centre(A, c->stream));
  HIP_TRY(c, launch_gram(L.base, L.local_rows, Xc, k, Gc, kr, c->d_red, gram_blocks, c->h_gram, c->stream));
  double sums[2 * kMaxLD], Amat[kMaxLD * kMaxLD], sigma[kMaxLD], xbar[kMaxLD], gbar[kMaxLD];
  HIP_TRY(c, hipMemcpyAsync(sums, d_sums, static_cast<size_t>(k + kr) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int a = 0; a < k; ++a) xbar[a] = sums[a] / A.m;
  for (int b = 0; b < kr; ++b) gbar[b] = sums[k + b] / A.m;
  if (!all_finite(xbar, static_cast<size_t>(k)) || !all_finite(gbar, static_cast<size_t>(kr))) return fail(c, CORA_ERR_NAN, "a mean position is not finite");
  if (!all_finite(c->h_gram, static_cast<size_t>(nel))) return fail(c, CORA_ERR_NAN, "the cross-covariance H is not finite");
  c->cmp_H.assign(c->h_gram, c->h_gram + nel);
  c->cmp_H_k = k;
  c->cmp_H_kr = kr;
  compare_align(k, kr, c->h_gram, (flags & CORA_COMPARE_PROPER) != 0, Amat, sigma);
  // step 3: errors, statistics, the aligned vector
  HIP_TRY(c, hipMemcpyAsync(d_A, Amat, static_cast<size_t>(nel) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (dAligned) {
    wrote(c, dAligned);
    HIP_TRY(c, hipMemsetAsync(dAligned, 0, vec_bytes(c, ldr), c->stream));
  }
  HIP_TRY(c, launch_compare_errors(A, c->stream));
  HIP_TRY(c, launch_reduce_partials(c->d_red, b_err, 3, d_stats, c->stream));
  HIP_TRY(c, launch_reduce_max_partials(c->d_red + static_cast<size_t>(3) * b_err, b_err, 3, d_stats + 3, c->stream));
  double st[6];
  HIP_TRY(c, hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (pose_trans_err) HIP_TRY(c, hipMemcpyAsync(pose_trans_err, d_et, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (pose_rot_err) HIP_TRY(c, hipMemcpyAsync(pose_rot_err, d_er, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (landmark_err && nl > 0) HIP_TRY(c, hipMemcpyAsync(landmark_err, d_el, static_cast<size_t>(nl) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  compare_release(c, 0, 2, kCompareKeepBytes);  // (synchronised above)
  if (*c->h_flag) return fail(c, CORA_ERR_NAN, "an error is not finite");
  out[0] = static_cast<double>(m);
  out[1] = st[0];
  out[2] = st[3];
  out[3] = st[1];
  out[4] = st[4];
  out[5] = static_cast<double>(ml);
  out[6] = st[2];
  out[7] = st[5];
  compare_tail_out(k, kr, sigma, xbar, gbar, Amat, out);
  return CORA_OK;
}

int cora_compare(cora_ctx *c, const double *X, int ldx, int k, const double *Ref, int ldref, int kr, const unsigned char *select,
                 int flags, double *pose_trans_err, double *pose_rot_err, double *landmark_err, double *Aligned, int ldal, double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = compare_check(c, k, kr, flags);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!X || !Ref || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  double *dX, *dRef, *dAl = nullptr;
  if ((rc = compare_vec(c, 2, ld_for(k), &dX)) || (rc = compare_vec(c, 3, ld_for(kr), &dRef))) return rc;
  if (Aligned && (rc = compare_vec(c, 4, ld_for(kr), &dAl))) return rc;
  if ((rc = upload_impl(c, X, ldx, k, dX))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the two uploads share one staging buffer)
  if ((rc = upload_impl(c, Ref, ldref, kr, dRef))) return rc;
  rc = cora_compare_dev(c, dX, k, dRef, kr, select, flags, pose_trans_err, pose_rot_err, landmark_err, dAl, out);
  if (rc == CORA_OK && Aligned) rc = download_impl(c, dAl, kr, Aligned, ldal);
  // the three vectors of this form are not kept: a caller that compares often stays resident and uses cora_compare_dev
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 2, 5, 0);
  return rc;
}

// The same operations on the host, in the plain order of the definitions (cora_hip.h): sequential sums over the poses in
// API order, H from centred rows, the alignment of compare_align, a column's sum over a = 0 .. k - 1 with one fma per
// term.  The lane order of the device's sums is NOT mirrored: the outputs agree with the device's within the rounding
// bounds of the definitions, not bit for bit.
int cora_debug_compare_host(cora_ctx *c, const double *X, int ldx, int k, const double *Ref, int ldref, int kr,
                            const unsigned char *select, int flags, double *pose_trans_err, double *pose_rot_err, double *landmark_err,
                            double *Aligned, int ldal, double *out) {
  if (!c) return CORA_ERR_ARG;
  const int rc = compare_check(c, k, kr, flags);
  if (rc) return rc;
  if (!X || !Ref || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const Layout &L = c->F.L;
  const int64_t N = L.N;
  if (ldx < N || ldref < N || (Aligned && ldal < N)) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  if (Aligned && (overlaps(Aligned, static_cast<size_t>(ldal) * kr * sizeof(double), X, static_cast<size_t>(ldx) * k * sizeof(double)) ||
                  overlaps(Aligned, static_cast<size_t>(ldal) * kr * sizeof(double), Ref, static_cast<size_t>(ldref) * kr * sizeof(double))))
    return fail(c, CORA_ERR_ARG, "the aligned matrix must not alias the estimate or the reference");
  std::vector<unsigned char> sel;
  int64_t m = 0, ml = 0;
  compare_selection(L, select, sel, m, ml);
  if (m == 0) return fail(c, CORA_ERR_ARG, "no pose selected");
  const int d = L.d, n = L.n, nt = L.nt;
  const int64_t dn = static_cast<int64_t>(d) * n, t0 = dn + L.r;
  auto x = [&](int64_t row, int col) { return X[static_cast<size_t>(col) * ldx + row]; };
  auto g = [&](int64_t row, int col) { return Ref[static_cast<size_t>(col) * ldref + row]; };
  double xbar[kMaxLD] = {}, gbar[kMaxLD] = {}, H[kMaxLD * kMaxLD] = {}, Amat[kMaxLD * kMaxLD], sigma[kMaxLD];
  for (int i = 0; i < n; ++i) {
    if (!sel[static_cast<size_t>(i)]) continue;
    for (int a = 0; a < k; ++a) xbar[a] += x(t0 + i, a);
    for (int b = 0; b < kr; ++b) gbar[b] += g(t0 + i, b);
  }
  for (int a = 0; a < k; ++a) xbar[a] /= static_cast<double>(m);
  for (int b = 0; b < kr; ++b) gbar[b] /= static_cast<double>(m);
  if (!all_finite(xbar, static_cast<size_t>(k)) || !all_finite(gbar, static_cast<size_t>(kr))) return fail(c, CORA_ERR_NAN, "a mean position is not finite");
  for (int i = 0; i < n; ++i) {
    if (!sel[static_cast<size_t>(i)]) continue;
    for (int a = 0; a < k; ++a) {
      const double xa = x(t0 + i, a) - xbar[a];
      for (int b = 0; b < kr; ++b) H[a * kr + b] = std::fma(xa, g(t0 + i, b) - gbar[b], H[a * kr + b]);
    }
  }
  if (!all_finite(H, static_cast<size_t>(k) * kr)) return fail(c, CORA_ERR_NAN, "the cross-covariance H is not finite");
  c->cmp_H.assign(H, H + static_cast<size_t>(k) * kr);
  c->cmp_H_k = k;
  c->cmp_H_kr = kr;
  compare_align(k, kr, H, (flags & CORA_COMPARE_PROPER) != 0, Amat, sigma);
  // one row through A: squared error against the row of Ref, the aligned row
  auto row_pass = [&](int64_t row, bool centred, bool want_err) {
    double sq = 0.0;
    for (int b = 0; b < kr; ++b) {
      double acc = 0.0;
      for (int a = 0; a < k; ++a) acc = std::fma(centred ? x(row, a) - xbar[a] : x(row, a), Amat[a * kr + b], acc);
      if (want_err) {
        const double diff = centred ? acc - (g(row, b) - gbar[b]) : acc - g(row, b);
        sq = std::fma(diff, diff, sq);
      }
      if (Aligned) Aligned[static_cast<size_t>(b) * ldal + row] = centred ? acc + gbar[b] : acc;
    }
    return sq;
  };
  double st[6] = {};
  bool bad = false;
  for (int i = 0; i < nt; ++i) {
    const bool on = sel[static_cast<size_t>(i)] != 0;
    double et = 0.0, er = 0.0;
    if (on || Aligned) {
      et = std::sqrt(row_pass(t0 + i, true, on));
      if (i < n) {
        double rot = 0.0;
        for (int cc = 0; cc < d; ++cc) rot += row_pass(static_cast<int64_t>(d) * i + cc, false, on);
        er = std::sqrt(rot);
      }
    }
    bad = bad || !std::isfinite(et) || !std::isfinite(er);
    if (i < n) {
      if (pose_trans_err) pose_trans_err[i] = et;
      if (pose_rot_err) pose_rot_err[i] = er;
      st[0] += et * et;
      st[1] += er * er;
      st[3] = std::fmax(st[3], et);
      st[4] = std::fmax(st[4], er);
    } else {
      if (landmark_err) landmark_err[i - n] = et;
      st[2] += et * et;
      st[5] = std::fmax(st[5], et);
    }
  }
  if (Aligned)
    for (int i = 0; i < L.r; ++i) (void)row_pass(dn + i, false, false);
  if (bad) return fail(c, CORA_ERR_NAN, "an error is not finite");
  out[0] = static_cast<double>(m);
  out[1] = st[0];
  out[2] = st[3];
  out[3] = st[1];
  out[4] = st[4];
  out[5] = static_cast<double>(ml);
  out[6] = st[2];
  out[7] = st[5];
  compare_tail_out(k, kr, sigma, xbar, gbar, Amat, out);
  return CORA_OK;
}

int cora_debug_compare_H(const cora_ctx *c, int k, int kr, double *H) {
  if (!c || !H || c->cmp_H_k != k || c->cmp_H_kr != kr || k <= 0) return CORA_ERR_ARG;
  for (int b = 0; b < kr; ++b)
    for (int a = 0; a < k; ++a) H[static_cast<size_t>(b) * k + a] = c->cmp_H[static_cast<size_t>(a) * kr + b];
  return CORA_OK;
}
