// Part of capi.hip (one translation unit; included there, in this order).  landmark initialisation from ranges (multilateration over the range table of the measurement table): list and chunk tables, device-pointer form, host-pointer form, host mirror; the outlier-robust forms (a consensus vote over samples of d + 1 ranges in front of the fit: MlConsensus, MlHostVote) share every one of them.  Reads the measurement table and the row maps; writes nothing the handle computes with.  What it shares with the other initialisers -- the range-row step, the host-pointer and host-mirror wrappers, installing tables, chunk cutting, the mirror's sums -- is in capi/init_common.inc.

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
    cut_chunks(begin, len, T.chunk_begin, T.chunk_len, &T.chunk_lm, static_cast<int32_t>(l));
    T.lm_chunk0.push_back(static_cast<int32_t>(T.chunk_lm.size()));
  }
  if (const int rc = range_rows_unique(c)) return rc;
  T.built = true;
  return CORA_OK;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int ml_upload(cora_ctx *c, MlTables &T) {
  HIP_TRY(c, upload_joined(&T.d_idx, {&T.chunk_lm, &T.chunk_begin, &T.chunk_len, &T.ent_row, &T.ent_m, &T.lm_chunk0, &T.lm_row, &T.lm_origin}));
  HIP_TRY(c, to_device(&T.d_init, T.lm_init));
  const int d = c->F.L.d;
  const size_t nl = std::max<size_t>(T.lm_row.size(), 1), nc = std::max<size_t>(T.chunk_lm.size(), 1);
  HIP_TRY(c, alloc_device(&T.d_partial, static_cast<size_t>(kMlSums(d)) * nc * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_state, static_cast<size_t>(kMlState(d)) * nl * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_istate, static_cast<size_t>(kMlInts) * nl * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_votes, std::max<size_t>(T.ent_row.size(), 1) * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_cstate, static_cast<size_t>(kMlCState(d)) * nl * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_cint, static_cast<size_t>(kMlCInts) * nl * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_inlier, std::max<size_t>(static_cast<size_t>(c->meas.n_ranges), 1)));
  return CORA_OK;
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

// the consensus setting and the outputs of a robust call (cora_multilaterate_robust_dev)
struct MlConsensus {
  double barc2;
  int min_consensus;
  int32_t *elected, *consensus, *list_len;
  unsigned char *inlier;
};
const char *ml_not_finite(const MlConsensus *rb) {  // the refusal of a call whose flag word is set
  return rb ? "a sum or a hypothesis of the multilateration is not finite" : "a sum of the multilateration is not finite";
}
int ml_consensus_check(cora_ctx *c, double barc2, int min_consensus) {
  if (!(barc2 > 0.0) || !std::isfinite(barc2)) return fail(c, CORA_ERR_ARG, "barc2 must be finite and positive");
  if (min_consensus < 1) return fail(c, CORA_ERR_ARG, "min_consensus must be at least 1");
  return CORA_OK;
}
// the length of landmark l's list
int32_t ml_list_len(const MlTables &T, size_t l) {
  const size_t c0 = static_cast<size_t>(T.lm_chunk0[l]), c1 = static_cast<size_t>(T.lm_chunk0[l + 1]);
  return c1 > c0 ? T.chunk_begin[c1 - 1] + T.chunk_len[c1 - 1] - T.chunk_begin[c0] : 0;
}
// what a robust call returns beyond the plain call's: cint [nl][kMlCInts] (read where lm_init == 0), inl [n_ranges] (2 where a
// range is in no list that is voted on)
void ml_robust_results(const cora_ctx *c, const std::vector<int32_t> &ist, const std::vector<int32_t> &cint, const std::vector<unsigned char> &inl,
                       const MlConsensus &rb, int64_t out[6]) {
  const MlTables &T = c->ml;
  const size_t nl = T.lm_row.size(), nr = static_cast<size_t>(c->meas.n_ranges);
  out[4] = out[5] = 0;
  for (size_t l = 0; l < nl; ++l) {
    const bool voted = T.lm_init[l] == 0;
    if (ist[l * kMlInts] == 5) ++out[4];
    if (rb.elected) rb.elected[l] = voted ? cint[l * kMlCInts] : -1;
    if (rb.consensus) rb.consensus[l] = voted ? cint[l * kMlCInts + 1] : 0;
    if (rb.list_len) rb.list_len[l] = ml_list_len(T, l);
  }
  for (size_t m = 0; m < nr; ++m) out[5] += inl[m] == 0 ? 1 : 0;
  if (rb.inlier) std::copy(inl.begin(), inl.begin() + static_cast<std::ptrdiff_t>(nr), rb.inlier);
}

extern "C++" {  // (templates: this file is included inside extern "C")
// the consensus vote of a robust call on the host: the setting and the lists' elected hypotheses, as on the device
struct MlHostVote {
  double barc2;
  int min_consensus;
  std::vector<double> cstate;      // [nl][kMlCState(d)]
  std::vector<int32_t> cint;       // [nl][kMlCInts]
  std::vector<unsigned char> inl;  // [n_ranges]
};
// the hypothesis of entry h of landmark l's list (begin, len), as k_ml_vote and k_ml_elect gather it
template <int D>
bool ml_host_hypothesis(const cora_ctx *c, const double *oi, size_t l, size_t begin, int32_t len, int32_t h, double *y) {
  const MlTables &T = c->ml;
  const MeasurementTable &M = c->meas;
  double ts[(D + 1) * D], rs[D + 1], ws[D + 1];
  for (int k = 0; k <= D; ++k) {
    const size_t e = begin + static_cast<size_t>(ml_sample<D>(h, k, len)), m = static_cast<size_t>(T.ent_m[e]);
    std::copy_n(oi + static_cast<size_t>(T.ent_row[e]) * D, D, ts + k * D);
    rs[k] = M.range_data[m];
    ws[k] = M.range_data[static_cast<size_t>(M.n_ranges) + m];
  }
  return ml_hypothesis<D>(oi + static_cast<size_t>(T.lm_origin[l]) * D, ts, rs, ws, y);
}
// vote and election over all lists (k_ml_vote, k_ml_elect): the votes are integers, so the order of the scoring is free
template <int D>
bool ml_host_vote_elect(const cora_ctx *c, const double *oi, MlHostVote &hv, std::vector<int32_t> &ist) {
  const MlTables &T = c->ml;
  const MeasurementTable &M = c->meas;
  bool finite = true;
  for (size_t l = 0; l < T.lm_row.size(); ++l) {
    if (T.lm_init[l] != 0) continue;
    const size_t begin = static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.lm_chunk0[l])]);
    const int32_t len = ml_list_len(T, l);
    const double *t0 = oi + static_cast<size_t>(T.lm_origin[l]) * D;
    std::vector<double> ent(static_cast<size_t>(len) * (D + 2));  // u | r | omega
    for (int32_t j = 0; j < len; ++j) {
      const size_t e = begin + static_cast<size_t>(j), m = static_cast<size_t>(T.ent_m[e]);
      double *f = ent.data() + static_cast<size_t>(j) * (D + 2);
      for (int cc = 0; cc < D; ++cc) f[cc] = oi[static_cast<size_t>(T.ent_row[e]) * D + cc] - t0[cc];
      f[D] = M.range_data[m];
      f[D + 1] = M.range_data[static_cast<size_t>(M.n_ranges) + m];
    }
    int32_t bv = -1, be = len;
    for (int32_t h = 0; h < len; ++h) {
      double y[D];
      int32_t vote = 0;
      if (ml_host_hypothesis<D>(c, oi, l, begin, len, h, y)) {
        for (int32_t j = 0; j < len; ++j) {
          const double *f = ent.data() + static_cast<size_t>(j) * (D + 2);
          vote += cl_agrees(ml_cost_at<D>(y, f, f[D], f[D + 1]), hv.barc2) ? 1 : 0;
        }
      }
      if (cl_better(vote, h, bv, be)) {
        bv = vote;
        be = h;
      }
    }
    double *y = hv.cstate.data() + l * kMlCState(D);
    ml_host_hypothesis<D>(c, oi, l, begin, len, be, y);
    hv.cint[l * kMlCInts] = be;
    hv.cint[l * kMlCInts + 1] = bv;
    ist[l * kMlInts] = bv < hv.min_consensus ? 5 : 0;
    finite = odom_finite(y, D) && finite;
  }
  return finite;
}
// the whole multilateration on the host, in the kernels' order: oi a d-column resident vector; state and ist as on the device
template <int D>
bool ml_host_run(const cora_ctx *c, int gn_steps, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg,
                 int64_t *n_deg, MlHostVote *hv = nullptr) {  // hv: over the inliers of the elected hypotheses (an entry outside adds +0.0 terms)
  const MlTables &T = c->ml;
  const MeasurementTable &M = c->meas;
  const int64_t nr = M.n_ranges;
  const size_t nl = T.lm_row.size(), nc = T.chunk_lm.size();
  bool finite = true;
  std::vector<double> partial(static_cast<size_t>(kMlSums(D)) * std::max<size_t>(nc, 1), 0.0);
  for (int stage = 0; stage <= gn_steps + 1; ++stage) {
    const int last = stage == gn_steps + 1 ? 1 : 0;
    for (size_t ch = 0; ch < nc; ++ch) {
      const size_t l = static_cast<size_t>(T.chunk_lm[ch]);
      if ((stage == 0 ? static_cast<int>(T.lm_init[l]) : ist[l * kMlInts]) != 0) continue;
      auto terms = [&](int i, double *t) {
        const size_t e = static_cast<size_t>(T.chunk_begin[ch]) + i, m = static_cast<size_t>(T.ent_m[e]);
        const double *t0 = oi + static_cast<size_t>(T.lm_origin[l]) * D, *ti = oi + static_cast<size_t>(T.ent_row[e]) * D;
        const double r = M.range_data[m], om = M.range_data[static_cast<size_t>(nr) + m];
        if (hv) {
          double u[D];
          for (int cc = 0; cc < D; ++cc) u[cc] = ti[cc] - t0[cc];
          const bool in = hv->cint[l * kMlCInts + 1] > 0 && cl_agrees(ml_cost_at<D>(hv->cstate.data() + l * kMlCState(D), u, r, om), hv->barc2);
          if (stage == 0) hv->inl[m] = in ? 1 : 0;
          if (!in) return;
        }
        if (stage == 0) ml_linear_terms<D>(t0, ti, r, om, t);
        else ml_gn_terms<D>(state.data() + l * kMlState(D), t0, ti, r, om, t);
      };
      if (stage == 0 && hv && ist[l * kMlInts] == 5) {  // (the bytes alone: the fold reads no sum of this list)
        double none[kMlSums(D)];
        for (int i = 0; i < T.chunk_len[ch]; ++i) terms(i, none);
        continue;
      }
      if (stage == 0) host_chunk_sums<kMlSums(D)>(T.chunk_len[ch], terms, partial.data(), nc, ch);
      else host_chunk_sums<kMlGnSums(D)>(T.chunk_len[ch], terms, partial.data(), nc, ch);
    }
    for (size_t l = 0; l < nl; ++l) {
      int32_t *li = ist.data() + l * kMlInts;
      double *st = state.data() + l * kMlState(D);
      const int init = hv && stage == 0 && T.lm_init[l] == 0 && li[0] == 5 ? 5 : static_cast<int>(T.lm_init[l]);
      double S[kMlSums(D)] = {};
      if (stage == 0 ? init != 0 : li[0] != 0) {
        if (stage == 0) ml_fold<D>(0, 0, S, st, li, init);
        continue;
      }
      const size_t c0 = static_cast<size_t>(T.lm_chunk0[l]), c1 = static_cast<size_t>(T.lm_chunk0[l + 1]);
      if (stage == 0) host_list_sums<kMlSums(D)>(partial.data(), nc, c0, c1, S);
      else host_list_sums<kMlGnSums(D)>(partial.data(), nc, c0, c1, S);
      finite = ml_fold<D>(stage, last, S, st, li, init) && finite;
      if (last && li[0] == 0) {
        const double *t0 = oi + static_cast<size_t>(T.lm_origin[l]) * D;
        for (int cc = 0; cc < D; ++cc) oi[static_cast<size_t>(T.lm_row[l]) * D + cc] = t0[cc] + st[D + cc];
      }
    }
  }
  return host_range_rows<D>(M, true, oi, deg, n_deg) && finite;
}
// the robust multilateration on the host, in the kernels' order: vote, election, then the stages over the inliers
template <int D>
bool ml_host_run_robust(const cora_ctx *c, int gn_steps, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg,
                        int64_t *n_deg, MlHostVote &hv) {
  const bool finite = ml_host_vote_elect<D>(c, oi, hv, ist);
  return ml_host_run<D>(c, gn_steps, oi, state, ist, deg, n_deg, &hv) && finite;
}
}  // extern "C++"

}  // namespace

int cora_set_multilateration(cora_ctx *c, const unsigned char *pose_ok, const unsigned char *landmark_on) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  return install_tables(c, c->ml, [&](MlTables &T) { return ml_build(c, pose_ok, landmark_on, T); }, [&](MlTables &T) { return ml_upload(c, T); });
}

int cora_multilateration_counts(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->ml.n_with_list;
  out[1] = c->ml.usable;
  out[2] = c->ml.skipped;
  out[3] = static_cast<int64_t>(c->ml.chunk_lm.size());
  return CORA_OK;
}

namespace {
// the device-pointer forms: rb null, the plain multilateration (2 (gn_steps + 2) launches); else the consensus vote in front of
// the masked passes (2 more)
int ml_dev(cora_ctx *c, double *dX, int gn_steps, const MlConsensus *rb, int64_t *out, unsigned char *status, double *cost_linear,
           double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  int rc;
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  MlTables &T = c->ml;
  const int d = L.d;
  const size_t nl = T.lm_row.size(), nc = T.chunk_lm.size(), ne = T.ent_row.size(), nr = static_cast<size_t>(M.n_ranges);
  const bool vote = rb && nc > 0;  // (no entry: no list to vote on, the plain launches serve the call)
  MlRobustArgs R;
  MlArgs &A = R.A;
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
  wrote(c, dX);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  if (rb) {
    R.barc2 = rb->barc2;
    R.min_consensus = rb->min_consensus;
    R.votes = T.d_votes;
    R.cstate = T.d_cstate;
    R.cint = T.d_cint;
    R.inlier = T.d_inlier;
    if (nr > 0) HIP_TRY(c, hipMemsetAsync(T.d_inlier, 2, nr, c->stream));  // (a range of no list that is voted on)
  }
  if (vote) HIP_TRY(c, launch_multilat_vote_elect(R, c->stream));
  for (int stage = 0; stage <= gn_steps + 1; ++stage) {
    A.stage = stage;
    A.last = stage == gn_steps + 1 ? 1 : 0;
    HIP_TRY(c, vote ? launch_multilat_robust_stage(R, c->stream) : launch_multilat_stage(A, c->stream));
  }
  std::vector<double> state(nl * kMlState(d));
  std::vector<int32_t> ist(nl * kMlInts), cint(rb ? nl * kMlCInts : 0, 0);
  std::vector<unsigned char> inl(rb ? nr : 0);
  int64_t n_deg = 0;
  if ((rc = range_rows_step(c, dX, true, degenerate, ml_not_finite(rb), &n_deg, [&]() -> int {  // (after the landmarks' rows)
         if (const int e = read_back_state(c, state, T.d_state, ist, T.d_istate)) return e;
         if (vote) HIP_TRY(c, hipMemcpyAsync(cint.data(), T.d_cint, cint.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
         if (rb && nr > 0) HIP_TRY(c, hipMemcpyAsync(inl.data(), T.d_inlier, nr, hipMemcpyDeviceToHost, c->stream));
         return CORA_OK;
       })))
    return rc;
  ml_results(c, state, ist, n_deg, out, status, cost_linear, cost_final, chosen);
  if (rb) ml_robust_results(c, ist, cint, inl, *rb, out);
  return CORA_OK;
}
// the host mirrors (with_host_x)
int ml_mirror(cora_ctx *c, double *X, int ldx, int gn_steps, const MlConsensus *rb, int64_t *out, unsigned char *status, double *cost_linear,
              double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  const int d = c->F.L.d;
  const size_t nl = c->ml.lm_row.size();
  std::vector<double> state(nl * kMlState(d), 0.0);
  std::vector<int32_t> ist(nl * kMlInts, 0);
  MlHostVote hv;
  if (rb) {
    hv.barc2 = rb->barc2;
    hv.min_consensus = rb->min_consensus;
    hv.cstate.assign(nl * kMlCState(d), 0.0);
    hv.cint.assign(nl * kMlCInts, 0);
    hv.inl.assign(static_cast<size_t>(c->meas.n_ranges), 2);
  }
  int64_t n_deg = 0;
  const int rc = with_host_x(c, X, ldx, ml_not_finite(rb), [&](auto D, double *oi) {
    return rb ? ml_host_run_robust<D()>(c, gn_steps, oi, state, ist, degenerate, &n_deg, hv)
              : ml_host_run<D()>(c, gn_steps, oi, state, ist, degenerate, &n_deg);
  });
  if (rc) return rc;
  ml_results(c, state, ist, n_deg, out, status, cost_linear, cost_final, chosen);
  if (rb) ml_robust_results(c, ist, hv.cint, hv.inl, *rb, out);
  return CORA_OK;
}
}  // namespace

int cora_multilaterate_dev(cora_ctx *c, double *dX, int gn_steps, int64_t out[4], unsigned char *status, double *cost_linear,
                           double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, dX, gn_steps, out))) return rc;
  return ml_dev(c, dX, gn_steps, nullptr, out, status, cost_linear, cost_final, chosen, degenerate);
}

int cora_multilaterate_robust_dev(cora_ctx *c, double *dX, int gn_steps, double barc2, int min_consensus, int64_t out[6], unsigned char *status,
                                  double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected, int32_t *consensus,
                                  int32_t *list_len, unsigned char *inlier, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, dX, gn_steps, out)) || (rc = ml_consensus_check(c, barc2, min_consensus))) return rc;
  const MlConsensus rb{barc2, min_consensus, elected, consensus, list_len, inlier};
  return ml_dev(c, dX, gn_steps, &rb, out, status, cost_linear, cost_final, chosen, degenerate);
}

int cora_multilaterate(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status, double *cost_linear,
                       double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, X, gn_steps, out))) return rc;
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return cora_multilaterate_dev(c, dX, gn_steps, out, status, cost_linear, cost_final, chosen, degenerate);
  });
}

int cora_multilaterate_robust(cora_ctx *c, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[6],
                              unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected,
                              int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = ml_args_check(c, X, gn_steps, out)) || (rc = ml_consensus_check(c, barc2, min_consensus))) return rc;
  const MlConsensus rb{barc2, min_consensus, elected, consensus, list_len, inlier};
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return ml_dev(c, dX, gn_steps, &rb, out, status, cost_linear, cost_final, chosen, degenerate);
  });
}

int cora_debug_multilaterate_host(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[4], unsigned char *status,
                                  double *cost_linear, double *cost_final, int32_t *chosen, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  if ((rc = ml_args_check(c, X, gn_steps, out))) return rc;
  return ml_mirror(c, X, ldx, gn_steps, nullptr, out, status, cost_linear, cost_final, chosen, degenerate);
}

int cora_debug_multilaterate_robust_host(cora_ctx *c, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[6],
                                         unsigned char *status, double *cost_linear, double *cost_final, int32_t *chosen, int32_t *elected,
                                         int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = ml_check(c);
  if (rc) return rc;
  if ((rc = ml_args_check(c, X, gn_steps, out)) || (rc = ml_consensus_check(c, barc2, min_consensus))) return rc;
  const MlConsensus rb{barc2, min_consensus, elected, consensus, list_len, inlier};
  return ml_mirror(c, X, ldx, gn_steps, &rb, out, status, cost_linear, cost_final, chosen, degenerate);
}
