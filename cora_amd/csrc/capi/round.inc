// Part of capi.hip (one translation unit; included there, in this order).  rounding of a relaxed point (k columns) to SE(d): device-pointer form, host-pointer form, host mirror.  Reads the row maps; writes nothing the handle computes with.

namespace {

// what the three forms check alike (everything but the device and the pointers)
int round_check(cora_ctx *c, int k) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the rounding is not supported on partitioned handles");
  if (k < c->F.L.d || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "the column count must lie in [d, 24]");
  return CORA_OK;
}

// Eigen-decomposition of the symmetric positive semi-definite k x k matrix G (row-major; its symmetric part is taken) by
// the one-sided Jacobi of the comparison (compare_jacobi): G / scale = U V^T with orthogonal columns of U, and for a
// symmetric positive semi-definite G the columns of V are its eigenvectors, the column norms of U its eigenvalues.
// sigma: sqrt(eigenvalue), descending, all k; vd: the eigenvectors of the d largest, column-major k x d -- orthogonalised
// against the ones before them (twice: the accumulated rotations leave V orthogonal to a few eps times the number of
// rotations only), normalised, and signed so that the entry of largest magnitude (the first on a tie) is positive.
void round_basis(int k, int d, const double *G, double *vd, double *sigma) {
  const size_t K = static_cast<size_t>(k);
  std::vector<double> S(K * K), U, V;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) S[i * K + j] = 0.5 * (G[i * K + j] + G[j * K + i]);
  const double scale = compare_jacobi(k, k, S.data(), U, V);
  std::vector<double> lambda(K);
  std::vector<int> order(K);
  for (int j = 0; j < k; ++j) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += U[i * K + j] * U[i * K + j];
    lambda[static_cast<size_t>(j)] = std::sqrt(s);
    order[static_cast<size_t>(j)] = j;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lambda[static_cast<size_t>(a)] > lambda[static_cast<size_t>(b)]; });
  for (int j = 0; j < k; ++j) {
    const size_t src = static_cast<size_t>(order[static_cast<size_t>(j)]);
    sigma[j] = std::sqrt(lambda[src] * scale);
    if (j >= d) continue;
    double *col = vd + static_cast<size_t>(j) * K;
    for (int i = 0; i < k; ++i) col[i] = V[i * K + src];
    for (int pass = 0; pass < 2; ++pass)
      for (int done = 0; done < j; ++done) {
        const double *prev = vd + static_cast<size_t>(done) * K;
        double dot = 0.0;
        for (int i = 0; i < k; ++i) dot += prev[i] * col[i];
        for (int i = 0; i < k; ++i) col[i] -= dot * prev[i];
      }
    double nrm = 0.0;
    for (int i = 0; i < k; ++i) nrm += col[i] * col[i];
    nrm = std::sqrt(nrm);
    int big = 0;
    for (int i = 1; i < k; ++i)
      if (std::fabs(col[i]) > std::fabs(col[big])) big = i;
    const double sign = (col[big] < 0.0 ? -1.0 : 1.0) / nrm;
    for (int i = 0; i < k; ++i) col[i] *= sign;
  }
}

// The power of two of the rare path for an input whose largest |entry| is amax (finite, > 0): it brings amax to [1/2, 1),
// but stays within +-1000 so that the basis times it (entries up to 1) stays a normal number -- what is left of a
// subnormal or a near-overflow input after that is well inside the range the units rescale themselves.
int round_input_exponent(double amax) {
  int e = 0;
  (void)std::frexp(amax, &e);
  return std::max(-1000, std::min(1000, -e));
}

// whether a Gram matrix (k x k) is one the basis can be taken from as it stands: finite, and not so small that the
// squares it is made of have left the range.  Otherwise the rare path forms it from a scaled copy of the input.
bool round_gram_usable(int k, const double *G) {
  double top = 0.0;
  for (int a = 0; a < k; ++a) top = std::max(top, G[static_cast<size_t>(a) * k + a]);
  return all_finite(G, static_cast<size_t>(k) * k) && !(top < 0x1p-500);
}

void round_fill_out(int k, int d, int count, int flip, const double *sigma, int e, const double *vd, double *out) {
  out[0] = static_cast<double>(count);
  out[1] = static_cast<double>(flip);
  for (int a = 0; a < k; ++a) out[2 + a] = std::ldexp(sigma[a], -e);
  std::copy(vd, vd + static_cast<size_t>(k) * d, out + 2 + k);
}

// the units of the host mirror: xi a resident vector on the host (internal rows, stride ldy), oi the rounded one (stride D)
extern "C++" {  // (a template: this file is included inside extern "C")
template <int D>
bool round_host_units(const Layout &L, const double *xi, int ldy, int k, const double *vd, const double *vd_dir, double *oi,
                      int *count_out, int *flip_out) {
  int count = 0;
  for (int u = 0; u < L.nl_poses; ++u) {
    const double *row = xi + (static_cast<size_t>(L.rot_base) + static_cast<size_t>(u) * D) * ldy;
    double m[D][D];
    for (int i = 0; i < D; ++i) round_product<D>(row + static_cast<size_t>(i) * ldy, k, vd_dir, m[i]);
    if (round_det_positive<D>(m)) ++count;
  }
  const bool flip = count < L.n / 2;
  bool finite = true;
  for (int u = 0; u < L.nl_poses; ++u) {
    const size_t row = static_cast<size_t>(L.rot_base) + static_cast<size_t>(u) * D;
    double m[D][D];
    finite = round_pose<D>(xi + row * ldy, ldy, k, vd_dir, flip, m) && finite;
    std::copy(&m[0][0], &m[0][0] + D * D, oi + row * D);
  }
  for (int u = 0; u < L.nl_ranges + L.nl_trans; ++u) {
    const bool range = u < L.nl_ranges;
    const size_t row = range ? static_cast<size_t>(L.rng_base) + u : static_cast<size_t>(L.trn_base) + (u - L.nl_ranges);
    double m[D];
    finite = round_row<D>(range, xi + row * ldy, k, range ? vd_dir : vd, flip, m) && finite;
    std::copy(m, m + D, oi + row * D);
  }
  *count_out = count;
  *flip_out = flip ? 1 : 0;
  return finite;
}
}  // extern "C++"

}  // namespace

int cora_round_dev(cora_ctx *c, const double *dY, int k, double *dOut, double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = round_check(c, k);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!dY || !dOut || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const Layout &L = c->F.L;
  const int d = L.d, ldy = ld_for(k), ldo = ld_for(d);
  if (overlaps(dOut, vec_bytes(c, ldo), dY, vec_bytes(c, ldy))) return fail(c, CORA_ERR_ARG, "the rounded vector must not alias the input");
  const int gram_blocks = 256, nel = k * k, nb = round_count_blocks(L.nl_poses);
  if ((rc = ensure_red(c, std::max<size_t>(static_cast<size_t>(nel) * gram_blocks + nel, static_cast<size_t>(nb) / 2 + 4)))) return rc;
  if ((rc = need_gram(c))) return rc;
  // step 1: G = Y^T Y (row-major k x k, straight into pinned memory), the basis on the host
  HIP_TRY(c, launch_gram(L.base, L.local_rows, dY, k, dY, k, c->d_red, gram_blocks, c->h_gram, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int e = 0;
  if (!round_gram_usable(k, c->h_gram)) {
    // the rare path: a non-finite entry is refused; an input whose squares leave the range is scaled by a power of two
    // (exact) into a vector of the pass's own for the Gram matrix alone -- the units read the input itself
    const int64_t len = static_cast<int64_t>(L.rows) * ldy;
    double amax = 0.0;
    HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
    HIP_TRY(c, launch_round_amax(len, dY, c->d_red, gram_blocks, c->d_flag, c->stream));
    HIP_TRY(c, launch_reduce_max_partials(c->d_red, gram_blocks, 1, c->d_red + gram_blocks, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&amax, c->d_red + gram_blocks, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (*c->h_flag || !std::isfinite(amax)) return fail(c, CORA_ERR_NAN, "the input of the rounding is not finite");
    if (amax > 0.0) {
      e = round_input_exponent(amax);
      double *tmp;
      if ((rc = compare_vec(c, 0, ldy, &tmp))) return rc;
      HIP_TRY(c, launch_round_scale(len, dY, e, tmp, c->stream));
      HIP_TRY(c, launch_gram(L.base, L.local_rows, tmp, k, tmp, k, c->d_red, gram_blocks, c->h_gram, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      compare_release(c, 0, 1, 0);  // (synchronised above; nothing of the call stays on the handle)
      if (!all_finite(c->h_gram, static_cast<size_t>(nel))) return fail(c, CORA_ERR_NAN, "the Gram matrix of the input is not finite");
    }
  }
  double sigma[kMaxLD];
  RoundArgs A;
  round_basis(k, d, c->h_gram, A.vd, sigma);
  for (int i = 0; i < k * d; ++i) A.vd_dir[i] = std::ldexp(A.vd[i], e);
  // steps 2 and 3: count, finish, apply -- one after the other on the stream, the flip read from the device
  A.R = row_args(c);
  A.k = k;
  A.ldy = ldy;
  A.Y = dY;
  A.out = dOut;
  A.partial = reinterpret_cast<int *>(c->d_red.p);
  A.words = A.partial + nb;
  A.flag = c->d_flag;
  wrote(c, dOut);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  HIP_TRY(c, hipMemsetAsync(dOut, 0, vec_bytes(c, ldo), c->stream));
  HIP_TRY(c, launch_round_count(A, c->stream));
  HIP_TRY(c, launch_round_apply(A, c->stream));
  int words[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(words, A.words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_flag) return fail(c, CORA_ERR_NAN, "a product of the rounding is not finite");
  round_fill_out(k, d, words[0], words[1], sigma, e, A.vd, out);
  return CORA_OK;
}

int cora_round(cora_ctx *c, const double *Y, int ldy, int k, double *Out, int ldo, double *out) {
  if (!c) return CORA_ERR_ARG;
  int rc = round_check(c, k);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!Y || !Out || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  if (ldo < c->F.L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = c->F.L.d;
  double *dY, *dOut;
  if ((rc = compare_vec(c, 2, ld_for(k), &dY)) || (rc = compare_vec(c, 3, ld_for(d), &dOut))) return rc;
  if ((rc = upload_impl(c, Y, ldy, k, dY))) return rc;
  rc = cora_round_dev(c, dY, k, dOut, out);
  if (rc == CORA_OK) rc = download_impl(c, dOut, d, Out, ldo);
  // the two vectors of this form are not kept: a caller that rounds often stays resident and uses cora_round_dev
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 2, 4, 0);
  return rc;
}

// The same operations on the host: the Gram matrix by plain sums over the rows in API order (one fma per term), the basis
// by round_basis -- or the caller's, so that a device result can be reproduced with the device's own basis --, then every
// unit through round_pose / round_row and their parts (kernels.h), the functions the kernels call: given the same basis, every output
// row, the count and the flip have the device's bits.  The singular values always come from this form's own Gram matrix.
int cora_debug_round_host(cora_ctx *c, const double *Y, int ldy, int k, const double *basis, double *Out, int ldo, double *out) {
  if (!c) return CORA_ERR_ARG;
  const int rc = round_check(c, k);
  if (rc) return rc;
  if (!Y || !Out || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const HostFormat &F = c->F;
  const Layout &L = F.L;
  const int64_t N = L.N;
  if (ldy < N || ldo < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = L.d, ldi = ld_for(k);
  std::vector<double> xi(static_cast<size_t>(L.rows) * ldi, 0.0), oi(static_cast<size_t>(L.rows) * d, 0.0);
  double amax = 0.0;
  for (int cc = 0; cc < k; ++cc)
    for (int64_t i = 0; i < N; ++i) {
      const double v = Y[static_cast<size_t>(cc) * ldy + i];
      if (!std::isfinite(v)) return fail(c, CORA_ERR_NAN, "the input of the rounding is not finite");
      amax = std::max(amax, std::fabs(v));
      xi[static_cast<size_t>(F.api2int[i]) * ldi + cc] = v;
    }
  double G[kMaxLD * kMaxLD];
  auto gram = [&](int e) {
    std::fill(G, G + k * k, 0.0);
    for (int64_t i = 0; i < N; ++i)
      for (int a = 0; a < k; ++a) {
        const double ya = std::ldexp(Y[static_cast<size_t>(a) * ldy + i], e);
        for (int b = 0; b < k; ++b) G[a * k + b] = std::fma(ya, std::ldexp(Y[static_cast<size_t>(b) * ldy + i], e), G[a * k + b]);
      }
  };
  gram(0);
  int e = 0;
  if (!round_gram_usable(k, G) && amax > 0.0) {
    e = round_input_exponent(amax);
    gram(e);
  }
  double sigma[kMaxLD], vd[kMaxLD * 3], own[kMaxLD * 3], vd_dir[kMaxLD * 3];
  round_basis(k, d, G, own, sigma);
  std::copy(basis ? basis : own, (basis ? basis : own) + k * d, vd);
  for (int i = 0; i < k * d; ++i) vd_dir[i] = std::ldexp(vd[i], e);
  int count = 0, flip = 0;
  const bool finite = for_d(d, [&](auto D) { return round_host_units<D()>(L, xi.data(), ldi, k, vd, vd_dir, oi.data(), &count, &flip); });
  if (!finite) return fail(c, CORA_ERR_NAN, "a product of the rounding is not finite");
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < N; ++i) Out[static_cast<size_t>(cc) * ldo + i] = oi[static_cast<size_t>(F.api2int[i]) * d + cc];
  round_fill_out(k, d, count, flip, sigma, e, vd, out);
  return CORA_OK;
}
