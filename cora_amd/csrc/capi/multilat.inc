// Part of capi.hip (one translation unit; included there, in this order).  landmark initialisation from ranges (multilateration over the range table of the measurement table): list and chunk tables, device-pointer form, host-pointer form, host mirror.  Reads the measurement table and the row maps; writes nothing the handle computes with.

namespace {

int ml_check(cora_ctx *c) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the multilateration is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  return CORA_OK;
}

// groups the usable ranges of the measurement table per landmark and cuts the lists into chunks (host part of T only)
int ml_build(cora_ctx *c, const unsigned char *pose_ok, const unsigned char *landmark_on, MlTables &T) {
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  if (const int rc = compare_pose_table(c)) return rc;
  const int32_t *trn_of = c->cmp_rows.data() + L.n;
  const int64_t nr = M.n_ranges, nl = L.nt - L.n;
  std::vector<int32_t> which(static_cast<size_t>(L.rows), -1);  // internal row -> translation index
  for (int i = 0; i < L.nt; ++i) which[static_cast<size_t>(trn_of[i])] = i;
  std::vector<std::vector<int32_t>> rows(static_cast<size_t>(nl)), meas(static_cast<size_t>(nl));
  int64_t entries = 0;
  for (int64_t m = 0; m < nr; ++m) {
    const int32_t ta = M.range_rows[static_cast<size_t>(nr + m)], tb = M.range_rows[static_cast<size_t>(2 * nr + m)];
    const int32_t ia = which[static_cast<size_t>(ta)], ib = which[static_cast<size_t>(tb)];
    if (ia < 0 || ib < 0) return fail(c, CORA_ERR_ARG, "range measurement " + std::to_string(m) + " names a row that is no translation row");
    if ((ia >= L.n) == (ib >= L.n)) {  // pose - pose, landmark - landmark
      ++T.skipped;
      continue;
    }
    ++T.usable;
    const int32_t l = (ia >= L.n ? ia : ib) - L.n, pose = ia >= L.n ? ib : ia;
    if ((landmark_on && !landmark_on[l]) || (pose_ok && !pose_ok[pose])) continue;
    rows[static_cast<size_t>(l)].push_back(ia >= L.n ? tb : ta);
    meas[static_cast<size_t>(l)].push_back(static_cast<int32_t>(m));
    ++entries;
  }
  if (nr >= (int64_t(1) << 31) || entries + nl * kMlChunk >= (int64_t(1) << 31))
    return fail(c, CORA_ERR_ARG, "the range lists have more entries than a 32-bit index holds");
  T.lm_chunk0.assign(1, 0);
  for (int64_t l = 0; l < nl; ++l) {
    const std::vector<int32_t> &list = rows[static_cast<size_t>(l)];
    const int64_t len = static_cast<int64_t>(list.size()), begin = static_cast<int64_t>(T.ent_row.size());
    const bool on = !landmark_on || landmark_on[l];
    T.lm_row.push_back(trn_of[L.n + l]);
    T.lm_origin.push_back(len > 0 ? list[0] : -1);
    T.lm_init.push_back(!on || len == 0 ? 3 : len < L.d + 1 ? 1 : 0);
    T.n_with_list += len > 0 ? 1 : 0;
    T.ent_row.insert(T.ent_row.end(), list.begin(), list.end());
    T.ent_m.insert(T.ent_m.end(), meas[static_cast<size_t>(l)].begin(), meas[static_cast<size_t>(l)].end());
    for (int64_t at = 0; at < len; at += kMlChunk) {
      T.chunk_lm.push_back(static_cast<int32_t>(l));
      T.chunk_begin.push_back(static_cast<int32_t>(begin + at));
      T.chunk_len.push_back(static_cast<int32_t>(std::min<int64_t>(kMlChunk, len - at)));
    }
    T.lm_chunk0.push_back(static_cast<int32_t>(T.chunk_lm.size()));
  }
  // (a range row two measurements name would be written by two threads of the range-row step)
  std::vector<unsigned char> written(static_cast<size_t>(L.rows), 0);
  for (int64_t m = 0; m < nr; ++m) {
    unsigned char &w = written[static_cast<size_t>(M.range_rows[static_cast<size_t>(m)])];
    if (w) return fail(c, CORA_ERR_ARG, "range measurement " + std::to_string(m) + " names a range row an earlier one names");
    w = 1;
  }
  T.built = true;
  return CORA_OK;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int ml_upload(cora_ctx *c, MlTables &T) {
  std::vector<int32_t> idx;
  for (const std::vector<int32_t> *v : {&T.chunk_lm, &T.chunk_begin, &T.chunk_len, &T.ent_row, &T.ent_m, &T.lm_chunk0, &T.lm_row, &T.lm_origin})
    idx.insert(idx.end(), v->begin(), v->end());
  HIP_TRY(c, to_device(&T.d_idx, idx));
  HIP_TRY(c, to_device(&T.d_init, T.lm_init));
  const int d = c->F.L.d;
  const size_t nl = std::max<size_t>(T.lm_row.size(), 1), nc = std::max<size_t>(T.chunk_lm.size(), 1);
  HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&T.d_partial), static_cast<size_t>(kMlSums(d)) * nc * sizeof(double)));
  HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&T.d_state), static_cast<size_t>(kMlState(d)) * nl * sizeof(double)));
  HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&T.d_istate), static_cast<size_t>(kMlInts) * nl * sizeof(int32_t)));
  HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&T.d_deg), std::max<size_t>(static_cast<size_t>(c->meas.n_ranges), 1)));
  // the range-row step writes the direction of (second row) - (first row): with a and b exchanged it writes the
  // direction of x_t(a) - x_t(b), the one at which the residual |x_t(b) - x_t(a) + r x_rho|^2 is (|x_t(b) - x_t(a)| - r)^2
  const size_t nr = static_cast<size_t>(c->meas.n_ranges);
  std::vector<int32_t> rows(c->meas.range_rows);
  std::swap_ranges(rows.begin() + static_cast<std::ptrdiff_t>(nr), rows.begin() + static_cast<std::ptrdiff_t>(2 * nr), rows.begin() + static_cast<std::ptrdiff_t>(2 * nr));
  HIP_TRY(c, to_device(&T.d_range_rows, rows));
  return CORA_OK;
}

void ml_release(MlTables &T) {  // a table that never reached the handle
  for (void *p : {static_cast<void *>(T.d_idx), static_cast<void *>(T.d_init), static_cast<void *>(T.d_partial), static_cast<void *>(T.d_state),
                  static_cast<void *>(T.d_istate), static_cast<void *>(T.d_deg), static_cast<void *>(T.d_range_rows)})
    if (p) (void)hipFree(p);
}

int ml_args_check(cora_ctx *c, const double *X, int gn_steps, const int64_t *out) {
  if (!c->ml.built) return fail(c, CORA_ERR_NOT_READY, "no multilateration tables (cora_set_multilateration)");
  if (gn_steps < 0 || gn_steps > kMlMaxSteps) return fail(c, CORA_ERR_ARG, "gn_steps must be in [0, 16]");
  if (!X || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  return CORA_OK;
}

// what a call returns, from the landmarks' state ([nl][kMlState(d)], [nl][kMlInts])
void ml_results(const cora_ctx *c, const std::vector<double> &state, const std::vector<int32_t> &ist, int64_t n_deg, int64_t out[4],
                unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen) {
  const int d = c->F.L.d;
  const size_t nl = c->ml.lm_row.size();
  int64_t solved = 0, steps = 0;
  for (size_t l = 0; l < nl; ++l) {
    const int32_t *li = ist.data() + l * kMlInts;
    const double *st = state.data() + l * kMlState(d);
    solved += li[0] == 0 ? 1 : 0;
    steps += li[2];
    if (status) status[l] = static_cast<unsigned char>(li[0]);
    if (cost_linear) cost_linear[l] = li[0] == 0 ? st[2 * d + 1] : 0.0;
    if (cost_final) cost_final[l] = li[0] == 0 ? st[2 * d] : 0.0;
    if (chosen) chosen[l] = li[0] == 0 ? li[1] : -1;
  }
  out[0] = solved;
  out[1] = static_cast<int64_t>(nl) - solved;
  out[2] = n_deg;
  out[3] = steps;
}

extern "C++" {  // (templates: this file is included inside extern "C")
// the butterfly of a wavefront as the tree it is: v[0] = ((v0 + v1) + (v2 + v3)) + ..
inline double ml_host_wave_sum(double *v) {
  for (int off = 1; off < kWave; off <<= 1)
    for (int i = 0; i < kWave; i += 2 * off) v[i] = v[i] + v[i + off];
  return v[0];
}
// the whole multilateration on the host, in the kernels' order: oi a d-column resident vector; state and ist as on the device
template <int D>
bool ml_host_run(const cora_ctx *c, int gn_steps, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg,
                 int64_t *n_deg) {
  const MlTables &T = c->ml;
  const MeasurementTable &M = c->meas;
  const int64_t nr = M.n_ranges;
  const size_t nl = T.lm_row.size(), nc = T.chunk_lm.size();
  bool finite = true;
  std::vector<double> partial(static_cast<size_t>(kMlSums(D)) * std::max<size_t>(nc, 1), 0.0);
  for (int stage = 0; stage <= gn_steps + 1; ++stage) {
    const int ns = stage == 0 ? kMlSums(D) : kMlGnSums(D), last = stage == gn_steps + 1 ? 1 : 0;
    for (size_t ch = 0; ch < nc; ++ch) {
      const size_t l = static_cast<size_t>(T.chunk_lm[ch]);
      if ((stage == 0 ? static_cast<int>(T.lm_init[l]) : ist[l * kMlInts]) != 0) continue;
      double wave[kMlChunk / kWave][kMlSums(D)];
      for (int w = 0; w < kMlChunk / kWave; ++w) {
        double term[kWave][kMlSums(D)];
        for (int lane = 0; lane < kWave; ++lane) {
          const int i = w * kWave + lane;
          for (int s = 0; s < ns; ++s) term[lane][s] = 0.0;
          if (i >= T.chunk_len[ch]) continue;
          const size_t e = static_cast<size_t>(T.chunk_begin[ch]) + i, m = static_cast<size_t>(T.ent_m[e]);
          const double *t0 = oi + static_cast<size_t>(T.lm_origin[l]) * D, *ti = oi + static_cast<size_t>(T.ent_row[e]) * D;
          const double r = M.range_data[m], om = M.range_data[static_cast<size_t>(nr) + m];
          if (stage == 0) ml_linear_terms<D>(t0, ti, r, om, term[lane]);
          else ml_gn_terms<D>(state.data() + l * kMlState(D), t0, ti, r, om, term[lane]);
        }
        for (int s = 0; s < ns; ++s) {
          double v[kWave];
          for (int lane = 0; lane < kWave; ++lane) v[lane] = term[lane][s];
          wave[w][s] = ml_host_wave_sum(v);
        }
      }
      for (int s = 0; s < ns; ++s) {
        double v = wave[0][s];
        for (int w = 1; w < kMlChunk / kWave; ++w) v = v + wave[w][s];
        partial[static_cast<size_t>(s) * nc + ch] = v;
      }
    }
    for (size_t l = 0; l < nl; ++l) {
      int32_t *li = ist.data() + l * kMlInts;
      double *st = state.data() + l * kMlState(D);
      const int init = T.lm_init[l];
      double S[kMlSums(D)] = {};
      if (stage == 0 ? init != 0 : li[0] != 0) {
        if (stage == 0) ml_fold<D>(0, 0, S, st, li, init);
        continue;
      }
      for (int s = 0; s < ns; ++s) {
        double v[kWave];
        for (int lane = 0; lane < kWave; ++lane) {
          v[lane] = 0.0;
          for (int64_t ch = static_cast<int64_t>(T.lm_chunk0[l]) + lane; ch < T.lm_chunk0[l + 1]; ch += kWave)
            v[lane] = v[lane] + partial[static_cast<size_t>(s) * nc + static_cast<size_t>(ch)];
        }
        S[s] = ml_host_wave_sum(v);
      }
      finite = ml_fold<D>(stage, last, S, st, li, init) && finite;
      if (last && li[0] == 0) {
        const double *t0 = oi + static_cast<size_t>(T.lm_origin[l]) * D;
        for (int cc = 0; cc < D; ++cc) oi[static_cast<size_t>(T.lm_row[l]) * D + cc] = t0[cc] + st[D + cc];
      }
    }
  }
  int64_t count = 0;
  for (int64_t m = 0; m < nr; ++m) {
    const size_t rr = static_cast<size_t>(M.range_rows[static_cast<size_t>(m)]), ta = static_cast<size_t>(M.range_rows[static_cast<size_t>(nr + m)]),
                 tb = static_cast<size_t>(M.range_rows[static_cast<size_t>(2 * nr + m)]);
    double row[D];
    const bool degenerate = odom_range_row<D>(oi + tb * D, oi + ta * D, row);  // (towards a: see ml_upload)
    std::copy(row, row + D, oi + rr * D);
    if (deg) deg[m] = degenerate ? 1 : 0;
    count += degenerate ? 1 : 0;
    finite = odom_finite(row, D) && finite;
  }
  *n_deg = count;
  return finite;
}
}  // extern "C++"

}  // namespace

int cora_set_multilateration(cora_ctx *c, const unsigned char *pose_ok, const unsigned char *landmark_on) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  MlTables T;
  if ((rc = ml_build(c, pose_ok, landmark_on, T))) return rc;
  if (c->has_device) {
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, CORA_ERR_HIP, "hipSetDevice failed");
    if ((rc = ml_upload(c, T))) {
      ml_release(T);
      return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_ml(c);
  }
  c->ml = std::move(T);
  return CORA_OK;
}

int cora_multilateration_counts(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->ml.n_with_list;
  out[1] = c->ml.usable;
  out[2] = c->ml.skipped;
  out[3] = static_cast<int64_t>(c->ml.chunk_lm.size());
  return CORA_OK;
}

int cora_multilaterate_dev(cora_ctx *c, double *dX, int gn_steps, int64_t out[4], unsigned char *status, double *cost_linear,
                           double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, dX, gn_steps, out))) return rc;
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  MlTables &T = c->ml;
  const int d = L.d, nb = odom_range_blocks(M.n_ranges);
  const size_t nl = T.lm_row.size(), nc = T.chunk_lm.size(), ne = T.ent_row.size();
  if ((rc = ensure_red(c, static_cast<size_t>(nb) / 2 + 4))) return rc;
  MlArgs A;
  A.d = d;
  A.n_lm = static_cast<int64_t>(nl);
  A.n_chunks = static_cast<int64_t>(nc);
  A.n_entries = static_cast<int64_t>(ne);
  A.n_ranges = M.n_ranges;
  A.chunk_lm = T.d_idx;
  A.chunk_begin = A.chunk_lm + nc;
  A.chunk_len = A.chunk_begin + nc;
  A.ent_row = A.chunk_len + nc;
  A.ent_m = A.ent_row + ne;
  A.lm_chunk0 = A.ent_m + ne;
  A.lm_row = A.lm_chunk0 + nl + 1;
  A.lm_origin = A.lm_row + nl;
  A.lm_init = T.d_init;
  A.range_data = M.d_range_data;
  A.partial = T.d_partial;
  A.state = T.d_state;
  A.istate = T.d_istate;
  A.x = dX;
  A.flag = c->d_flag;
  OdomFillArgs Fl;  // the range-row step of the odometry initialisation, its rules unchanged, over the exchanged table
  Fl.d = d;
  Fl.n_ranges = M.n_ranges;
  Fl.range_rows = T.d_range_rows;
  Fl.deg = T.d_deg;
  Fl.partial = reinterpret_cast<int *>(c->d_red);
  Fl.words = Fl.partial + nb;
  Fl.flag = c->d_flag;
  Fl.out = dX;
  wrote(c, dX);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  for (int stage = 0; stage <= gn_steps + 1; ++stage) {
    A.stage = stage;
    A.last = stage == gn_steps + 1 ? 1 : 0;
    HIP_TRY(c, launch_multilat_stage(A, c->stream));
  }
  HIP_TRY(c, launch_odom_ranges(Fl, c->stream));  // (after the landmarks' rows)
  int words[2] = {0, 0};
  std::vector<double> state(nl * kMlState(d));
  std::vector<int32_t> ist(nl * kMlInts);
  HIP_TRY(c, hipMemcpyAsync(words, Fl.words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (nl > 0) {
    HIP_TRY(c, hipMemcpyAsync(state.data(), T.d_state, state.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ist.data(), T.d_istate, ist.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  if (degenerate && M.n_ranges > 0)
    HIP_TRY(c, hipMemcpyAsync(degenerate, T.d_deg, static_cast<size_t>(M.n_ranges), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_flag) return fail(c, CORA_ERR_NAN, "a sum of the multilateration is not finite");
  ml_results(c, state, ist, words[0], out, status, cost_linear, cost_final, chosen);
  return CORA_OK;
}

int cora_multilaterate(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status, double *cost_linear,
                       double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, X, gn_steps, out))) return rc;
  if (ldx < c->F.L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = c->F.L.d;
  double *dX;
  if ((rc = compare_vec(c, 3, ld_for(d), &dX))) return rc;
  rc = upload_impl(c, X, ldx, d, dX);
  if (rc == CORA_OK) rc = cora_multilaterate_dev(c, dX, gn_steps, out, status, cost_linear, cost_final, chosen, degenerate);
  if (rc == CORA_OK) rc = download_impl(c, dX, d, X, ldx);
  // the vector of this form is not kept: a caller that stays resident uses cora_multilaterate_dev
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 3, 4, 0);
  return rc;
}

// The same on the host through the translated tables, every sum in the kernels' bracket order and every term and solve
// through the functions of kernels.h the kernels call: the output has the device's bits.  Works on a plan-only handle.
int cora_debug_multilaterate_host(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status,
                                  double *cost_linear, double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  if ((rc = ml_args_check(c, X, gn_steps, out))) return rc;
  const HostFormat &F = c->F;
  const Layout &L = F.L;
  if (ldx < L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = L.d;
  const size_t nl = c->ml.lm_row.size();
  std::vector<double> oi(static_cast<size_t>(L.rows) * d, 0.0), state(nl * kMlState(d), 0.0);
  std::vector<int32_t> ist(nl * kMlInts, 0);
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < L.N; ++i) oi[static_cast<size_t>(F.api2int[i]) * d + cc] = X[static_cast<size_t>(cc) * ldx + i];
  int64_t n_deg = 0;
  const bool finite = d == 2 ? ml_host_run<2>(c, gn_steps, oi.data(), state, ist, degenerate, &n_deg)
                             : ml_host_run<3>(c, gn_steps, oi.data(), state, ist, degenerate, &n_deg);
  if (!finite) return fail(c, CORA_ERR_NAN, "a sum of the multilateration is not finite");
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < L.N; ++i) X[static_cast<size_t>(cc) * ldx + i] = oi[static_cast<size_t>(F.api2int[i]) * d + cc];
  ml_results(c, state, ist, n_deg, out, status, cost_linear, cost_final, chosen);
  return CORA_OK;
}
