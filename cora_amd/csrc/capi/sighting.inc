// Part of capi.hip (one translation unit; included there, in this order).  placement from pose-landmark sightings (landmarks by the weighted mean of what placed poses predict, chains by the weighted rigid alignment onto placed landmarks): order of the stages and list tables, device-pointer form, host-pointer form, host mirror, each plain and with the consensus vote in front of every fit (cora_place_by_sightings_robust_dev).  Reads the measurement table, the chain tables and the row maps; writes nothing the handle computes with.  What it shares with the other initialisers -- the range-row step, the host-pointer and host-mirror wrappers, installing tables, chunk cutting, the mirror's sums -- is in capi/init_common.inc.

namespace {

int sg_check(cora_ctx *c) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the sighting placement is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (!c->odom.built) return fail(c, CORA_ERR_NOT_READY, "no chain tables (cora_set_odometry_chains)");
  return CORA_OK;
}

// the order of the stages and their lists, from structure alone (host part of T only)
int sg_build(cora_ctx *c, const unsigned char *chain_fixed, const unsigned char *landmark_fixed, int min_sightings, SgTables &T) {
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  const OdomTables &O = c->odom;
  const int d = L.d;
  const int64_t ne = M.n_edges, nch = O.n_chains, nl = static_cast<int64_t>(O.lm_row.size());
  if (min_sightings < d) return fail(c, CORA_ERR_ARG, "min_sightings must be at least d");
  if (ne >= (int64_t(1) << 31)) return fail(c, CORA_ERR_ARG, "the edge table has more entries than a 32-bit index holds");
  std::vector<unsigned char> placed, lm_placed(static_cast<size_t>(nl), 0);
  if (const int rc = seed_fixed_chains(c, chain_fixed, placed)) return rc;
  if (landmark_fixed)
    for (int64_t l = 0; l < nl; ++l) lm_placed[static_cast<size_t>(l)] = landmark_fixed[l] ? 1 : 0;
  const std::vector<unsigned char> lm_fixed = lm_placed;
  const ChainMaps maps = chain_maps(c);
  const std::vector<int32_t> &chain_of = maps.chain_of;
  const std::vector<std::vector<int32_t>> &chain_pos = maps.chain_pos;
  std::vector<int32_t> lm_of(static_cast<size_t>(L.rows), -1);
  for (int64_t l = 0; l < nl; ++l) lm_of[static_cast<size_t>(O.lm_row[static_cast<size_t>(l)])] = static_cast<int32_t>(l);
  // the sightings in table order: edge, chain, landmark   (edge_rows: [ra | rb | ta | tb][edge])
  std::vector<int32_t> s_e, s_ch, s_lm;
  for (int64_t e = 0; e < ne; ++e) {
    if (M.edge_rows[static_cast<size_t>(ne + e)] >= 0) continue;  // a pose-pose edge
    const int32_t ch = chain_of[static_cast<size_t>(M.edge_rows[static_cast<size_t>(2 * ne + e)])];
    const int32_t lm = lm_of[static_cast<size_t>(M.edge_rows[static_cast<size_t>(3 * ne + e)])];
    if (ch < 0 || lm < 0) {
      ++T.skipped;
      continue;
    }
    s_e.push_back(static_cast<int32_t>(e));
    s_ch.push_back(ch);
    s_lm.push_back(lm);
  }
  const size_t nsg = s_e.size();
  T.min_sightings = min_sightings;
  T.stage_list0.assign(1, 0);
  T.stage_apply0.assign(1, 0);
  T.list_chunk0.assign(1, 0);
  auto add_list = [&](int32_t item, int32_t row, const std::vector<size_t> &members) {
    const size_t begin = T.ent_e.size();
    for (const size_t u : members) {
      const int32_t e = s_e[u];
      T.ent_rot.push_back(M.edge_rows[static_cast<size_t>(e)]);
      T.ent_trn.push_back(M.edge_rows[static_cast<size_t>(2 * ne + e)]);
      T.ent_lm.push_back(M.edge_rows[static_cast<size_t>(3 * ne + e)]);
      T.ent_e.push_back(e);
    }
    cut_chunks(static_cast<int64_t>(begin), static_cast<int64_t>(members.size()), T.chunk_begin, T.chunk_len, &T.chunk_list,
               static_cast<int32_t>(T.list_item.size()));
    T.list_item.push_back(item);
    T.list_row.push_back(row);
    T.list_chunk0.push_back(static_cast<int32_t>(T.chunk_begin.size()));
  };
  auto end_stage = [&](int kind) {
    T.stage_kind.push_back(kind);
    T.stage_list0.push_back(static_cast<int32_t>(T.list_item.size()));
    T.stage_apply0.push_back(static_cast<int32_t>(T.apply_pos.size()));
  };
  // a landmark's list: its sightings from placed chains, in table order
  auto landmark_stage = [&](int kind, const std::vector<unsigned char> &want) {
    std::vector<std::vector<size_t>> members(static_cast<size_t>(nl));
    for (size_t u = 0; u < nsg; ++u)
      if (want[static_cast<size_t>(s_lm[u])] && placed[static_cast<size_t>(s_ch[u])]) members[static_cast<size_t>(s_lm[u])].push_back(u);
    std::vector<int32_t> taken;
    for (int64_t l = 0; l < nl; ++l)
      if (!members[static_cast<size_t>(l)].empty()) {
        if (kind == 2) T.lm_list[static_cast<size_t>(l)] = static_cast<int32_t>(T.list_item.size());
        add_list(static_cast<int32_t>(l), O.lm_row[static_cast<size_t>(l)], members[static_cast<size_t>(l)]);
        taken.push_back(static_cast<int32_t>(l));
      }
    if (!taken.empty()) end_stage(kind);
    return taken;
  };
  T.chain_list.assign(static_cast<size_t>(nch), -1);
  T.lm_list.assign(static_cast<size_t>(nl), -1);
  if (nsg > 0)
    for (;;) {
      std::vector<unsigned char> want(static_cast<size_t>(nl), 0);
      for (int64_t l = 0; l < nl; ++l) want[static_cast<size_t>(l)] = lm_placed[static_cast<size_t>(l)] ? 0 : 1;
      const std::vector<int32_t> lms = landmark_stage(0, want);
      for (const int32_t l : lms) lm_placed[static_cast<size_t>(l)] = 1;
      // EVERY unplaced chain with min_sightings sightings of placed landmarks, d of them distinct, in ONE stage
      std::vector<std::vector<size_t>> members(static_cast<size_t>(nch));
      for (size_t u = 0; u < nsg; ++u)
        if (!placed[static_cast<size_t>(s_ch[u])] && lm_placed[static_cast<size_t>(s_lm[u])]) members[static_cast<size_t>(s_ch[u])].push_back(u);
      std::vector<int32_t> chains;
      for (int64_t ch = 0; ch < nch; ++ch) {
        const std::vector<size_t> &mb = members[static_cast<size_t>(ch)];
        if (static_cast<int64_t>(mb.size()) < min_sightings) continue;
        std::vector<int32_t> seen;
        for (const size_t u : mb) seen.push_back(s_lm[u]);
        std::sort(seen.begin(), seen.end());
        if (std::unique(seen.begin(), seen.end()) - seen.begin() < d) continue;
        T.chain_list[static_cast<size_t>(ch)] = static_cast<int32_t>(T.list_item.size());
        for (const int32_t pos : chain_pos[static_cast<size_t>(ch)]) {
          T.apply_pos.push_back(pos);
          T.apply_list.push_back(static_cast<int32_t>(T.list_item.size()));
        }
        add_list(static_cast<int32_t>(ch), -1, mb);
        chains.push_back(static_cast<int32_t>(ch));
      }
      if (!chains.empty()) end_stage(1);
      for (const int32_t ch : chains) placed[static_cast<size_t>(ch)] = 1;
      if (lms.empty() && chains.empty()) break;
    }
  {  // the REFIT: every landmark that is not fixed, from ALL its sightings by placed chains
    std::vector<unsigned char> want(static_cast<size_t>(nl), 0);
    for (int64_t l = 0; l < nl; ++l) want[static_cast<size_t>(l)] = lm_fixed[static_cast<size_t>(l)] ? 0 : 1;
    (void)landmark_stage(2, want);
  }
  std::vector<unsigned char> sees(static_cast<size_t>(nch), 0);
  for (size_t u = 0; u < nsg; ++u) sees[static_cast<size_t>(s_ch[u])] = 1;
  T.chain_init.assign(static_cast<size_t>(nch), 0);
  for (int64_t ch = 0; ch < nch; ++ch) {
    const size_t i = static_cast<size_t>(ch);
    T.chain_init[i] = T.chain_list[i] >= 0 ? 0 : (placed[i] ? 4 : (sees[i] ? 1 : 3));
  }
  T.lm_init.assign(static_cast<size_t>(nl), 0);
  for (int64_t l = 0; l < nl; ++l) {
    const size_t i = static_cast<size_t>(l);
    T.lm_init[i] = lm_fixed[i] ? 3 : (T.lm_list[i] >= 0 ? 0 : 1);
  }
  if (T.ent_e.size() >= (size_t(1) << 31)) return fail(c, CORA_ERR_ARG, "the lists have more entries than a 32-bit index holds");
  if (const int rc = range_rows_unique(c)) return rc;
  T.built = true;
  return CORA_OK;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int sg_upload(cora_ctx *c, SgTables &T) {
  HIP_TRY(c, upload_joined(&T.d_idx, {&T.chunk_begin, &T.chunk_len, &T.chunk_list, &T.list_chunk0, &T.list_row, &T.ent_rot, &T.ent_trn, &T.ent_lm,
                                      &T.ent_e, &T.apply_pos, &T.apply_list}));
  const int d = c->F.L.d;
  const size_t nlist = std::max<size_t>(T.list_item.size(), 1), nc = std::max<size_t>(T.chunk_begin.size(), 1);
  HIP_TRY(c, alloc_device(&T.d_partial, static_cast<size_t>(kSgMaxSums(d)) * nc * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_state, static_cast<size_t>(kSgState(d)) * nlist * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_istate, static_cast<size_t>(kSgInts) * nlist * sizeof(int32_t)));
  // the consensus vote's scratch
  const size_t nent = std::max<size_t>(T.ent_e.size(), 1);
  HIP_TRY(c, alloc_device(&T.d_votes, nent * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_hyp, static_cast<size_t>(kSgCState(d)) * nent * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_cstate, static_cast<size_t>(kSgCState(d)) * nlist * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_cint, static_cast<size_t>(kSgCInts) * nlist * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_inlier, 2 * std::max<size_t>(static_cast<size_t>(c->meas.n_edges), 1)));
  return CORA_OK;
}

int sg_args_check(cora_ctx *c, const double *X, const int64_t *out) {
  if (!c->sg.built) return fail(c, CORA_ERR_NOT_READY, "no sighting tables (cora_set_sighting_placement)");
  if (!X || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  return CORA_OK;
}

// what a call returns, from the lists' state ([lists][kSgState(d)], [lists][kSgInts])
void sg_results(const cora_ctx *c, const std::vector<double> &state, const std::vector<int32_t> &ist, int64_t n_deg, int64_t out[6],
                unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms, unsigned char *lm_status,
                double *lm_cost) {
  const int d = c->F.L.d, G = kSgG(d), NS = kSgState(d);
  const SgTables &T = c->sg;
  const size_t nch = T.chain_init.size(), nl = T.lm_init.size();
  for (int i = 0; i < 6; ++i) out[i] = 0;
  for (size_t ch = 0; ch < nch; ++ch) {
    const int32_t list = T.chain_list[ch];
    const int32_t *li = list >= 0 ? ist.data() + static_cast<size_t>(list) * kSgInts : nullptr;
    const double *st = list >= 0 ? state.data() + static_cast<size_t>(list) * NS : nullptr;
    const int s = li ? li[0] : T.chain_init[ch];
    out[0] += s == 0 ? 1 : 0;
    out[1] += s == 1 || s == 2 || s == 3 ? 1 : 0;
    if (status) status[ch] = static_cast<unsigned char>(s);
    if (cost_start) cost_start[ch] = st ? st[G + d] : 0.0;
    if (cost_final) cost_final[ch] = st ? st[G + d + 1] : 0.0;
    if (chosen) chosen[ch] = li ? li[1] : -1;
    if (transforms && li && li[1] > 0) std::copy(st, st + G, transforms + ch * G);
    else if (transforms) identity_transform(d, transforms + ch * G);
  }
  for (size_t l = 0; l < nl; ++l) {
    const int32_t list = T.lm_list[l];
    const int s = list >= 0 ? ist[static_cast<size_t>(list) * kSgInts] : T.lm_init[l];
    out[2] += s == 0 ? 1 : 0;
    out[3] += s == 1 || s == 2 ? 1 : 0;
    if (lm_status) lm_status[l] = static_cast<unsigned char>(s);
    if (lm_cost) lm_cost[l] = list >= 0 ? state[static_cast<size_t>(list) * NS + d + 1] : 0.0;
  }
  out[4] = n_deg;
  out[5] = static_cast<int64_t>(T.stage_kind.size());
}

extern "C++" {  // (templates: this file is included inside extern "C")
template <int D>
double sg_host_entry(const cora_ctx *c, const double *oi, size_t e, double *p, const double **l) {
  const SgTables &T = c->sg;
  const MeasurementTable &M = c->meas;
  const size_t ne = static_cast<size_t>(M.n_edges), m = static_cast<size_t>(T.ent_e[e]);
  double t[D];
  for (int cc = 0; cc < D; ++cc) t[cc] = M.edge_data[static_cast<size_t>(D * D + cc) * ne + m];
  sg_predict<D>(oi + static_cast<size_t>(T.ent_rot[e]) * D, oi + static_cast<size_t>(T.ent_trn[e]) * D, t, p);
  *l = oi + static_cast<size_t>(T.ent_lm[e]) * D;
  return M.edge_data[static_cast<size_t>(D * D + D + 1) * ne + m];
}
// the consensus vote of a robust call on the host: the setting and the lists' elected hypotheses, as on the device
struct SgHostVote {
  double barc2;
  int min_chain_consensus, min_landmark_consensus;
  std::vector<double> cstate;      // [lists][kSgCState(d)]
  std::vector<int32_t> cint;       // [lists][kSgCInts]
  std::vector<unsigned char> inl;  // [2][n_edges]: chain lists | landmark lists
};
// the first entry and the length of a list
void sg_host_span(const SgTables &T, size_t list, size_t *begin, size_t *len) {
  const size_t last = static_cast<size_t>(T.list_chunk0[list + 1]) - 1;
  *begin = static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]);
  *len = static_cast<size_t>(T.chunk_begin[last] + T.chunk_len[last]) - *begin;
}
// vote and election over one stage (k_sg_hyp, k_sg_vote, k_sg_elect): the votes are integers, so the order of the scoring is free
template <int D>
bool sg_host_vote_elect(const cora_ctx *c, size_t s, const double *oi, SgHostVote &hv, std::vector<int32_t> &ist) {
  constexpr int CS = kSgCState(D);
  const SgTables &T = c->sg;
  const bool chain = T.stage_kind[s] == 1;
  const int GS = chain ? CS : D;
  bool finite = true;
  for (size_t list = static_cast<size_t>(T.stage_list0[s]); list < static_cast<size_t>(T.stage_list0[s + 1]); ++list) {
    size_t begin, len;
    sg_host_span(T, list, &begin, &len);
    std::vector<double> pp(len * D), ll(len * D), tau(len);
    double p0[D];
    const double *l0;
    (void)sg_host_entry<D>(c, oi, begin, p0, &l0);
    for (size_t j = 0; j < len; ++j) {
      double p[D];
      const double *l;
      tau[j] = sg_host_entry<D>(c, oi, begin + j, p, &l);
      for (int cc = 0; cc < D; ++cc) {
        pp[j * D + cc] = p[cc] - p0[cc];
        ll[j * D + cc] = l[cc] - l0[cc];
      }
    }
    int32_t bv = -1, be = static_cast<int32_t>(len);
    double best[CS] = {};
    for (size_t h = 0; h < len; ++h) {
      double g[CS] = {};
      bool valid = true;
      if (chain) {
        valid = sg_hypothesis<D>(static_cast<int32_t>(h), static_cast<int32_t>(len), p0, l0,
                                 [&](int32_t j, double *p, const double **l) { return sg_host_entry<D>(c, oi, begin + static_cast<size_t>(j), p, l); }, g);
      } else {
        for (int cc = 0; cc < D; ++cc) g[cc] = pp[h * D + cc];
      }
      int32_t vote = 0;
      if (valid)
        for (size_t j = 0; j < len; ++j) {
          const double r = chain ? sg_cost_rel<D>(g, pp.data() + j * D, ll.data() + j * D, tau[j]) : sg_lm_cost<D>(pp.data() + j * D, g, tau[j]);
          vote += cl_agrees(r, hv.barc2) ? 1 : 0;
        }
      if (cl_better(vote, static_cast<int32_t>(h), bv, be)) {
        bv = vote;
        be = static_cast<int32_t>(h);
        std::copy(g, g + CS, best);
      }
    }
    std::copy(best, best + CS, hv.cstate.data() + list * CS);
    hv.cint[list * kSgCInts] = be;
    hv.cint[list * kSgCInts + 1] = bv;
    ist[list * kSgInts] = bv < (chain ? hv.min_chain_consensus : hv.min_landmark_consensus) ? 5 : 0;
    ist[list * kSgInts + 1] = 0;
    finite = odom_finite(best, GS) && finite;
  }
  return finite;
}
// pass and fold of one mode over one stage, in the kernels' order; hv: over the inliers of the elected hypotheses only (an
// entry outside adds +0.0 terms), the folds with status 5 passed through
template <int D, int MODE>
bool sg_host_pass_fold(const cora_ctx *c, size_t s, double *oi, std::vector<double> &partial, std::vector<double> &state, std::vector<int32_t> &ist,
                       SgHostVote *hv = nullptr) {
  constexpr int NS = MODE == 0 ? kSgLmSums(D) : (MODE == 1 ? kSgChainSums(D) : (MODE == 2 ? kSgCostSums : 1));
  const SgTables &T = c->sg;
  const size_t nc = std::max<size_t>(T.chunk_begin.size(), 1), ne = static_cast<size_t>(c->meas.n_edges);
  const size_t l0 = static_cast<size_t>(T.stage_list0[s]), l1 = static_cast<size_t>(T.stage_list0[s + 1]);
  bool finite = true;
  for (size_t ch = static_cast<size_t>(T.list_chunk0[l0]); ch < static_cast<size_t>(T.list_chunk0[l1]); ++ch) {
    const size_t list = static_cast<size_t>(T.chunk_list[ch]);
    double p0[D];
    const double *lm0;
    (void)sg_host_entry<D>(c, oi, static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]), p0, &lm0);
    host_chunk_sums<NS>(T.chunk_len[ch], [&](int i, double *t) {
      double p[D];
      const double *lm;
      const size_t e = static_cast<size_t>(T.chunk_begin[ch]) + i;
      const double tau = sg_host_entry<D>(c, oi, e, p, &lm);
      if (hv) {
        const double *h = hv->cstate.data() + list * kSgCState(D);
        double pp[D], ll[D];
        for (int cc = 0; cc < D; ++cc) {
          pp[cc] = p[cc] - p0[cc];
          ll[cc] = lm[cc] - lm0[cc];
        }
        const bool in = cl_agrees(MODE == 0 || MODE == 3 ? sg_lm_cost<D>(pp, h, tau) : sg_cost_rel<D>(h, pp, ll, tau), hv->barc2);
        if constexpr (MODE == 0) hv->inl[ne + static_cast<size_t>(T.ent_e[e])] = in ? 1 : 0;
        if constexpr (MODE == 1) hv->inl[static_cast<size_t>(T.ent_e[e])] = in ? 1 : 0;
        if (!in) return;
      }
      if constexpr (MODE == 0) sg_lm_terms<D>(p0, p, tau, t);
      else if constexpr (MODE == 1) sg_chain_terms<D>(p0, lm0, p, lm, tau, t);
      else if constexpr (MODE == 2) sg_cost_terms<D>(state.data() + list * kSgState(D), p0, lm0, p, lm, tau, t);
      else t[0] = sg_lm_cost<D>(p, lm, tau);
    }, partial.data(), nc, ch);
  }
  for (size_t list = l0; list < l1; ++list) {
    double S[NS];
    host_list_sums<NS>(partial.data(), nc, static_cast<size_t>(T.list_chunk0[list]), static_cast<size_t>(T.list_chunk0[list + 1]), S);
    double p0[D];
    const double *lm0;
    (void)sg_host_entry<D>(c, oi, static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]), p0, &lm0);
    const int32_t row = T.list_row[list];
    double *st = state.data() + list * kSgState(D), *xr = row >= 0 ? oi + static_cast<size_t>(row) * D : nullptr;
    int32_t *li = ist.data() + list * kSgInts;
    finite = (hv ? sg_fold_robust<D, MODE>(S, st, li, p0, lm0, xr) : sg_fold<D, MODE>(S, st, li, p0, lm0, xr)) && finite;
  }
  return finite;
}
// the whole placement on the host, in the kernels' order: oi a d-column resident vector; state and ist as on the device
template <int D>
bool sg_host_run(const cora_ctx *c, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg, int64_t *n_deg,
                 SgHostVote *hv = nullptr) {
  const SgTables &T = c->sg;
  const MeasurementTable &M = c->meas;
  bool finite = true;
  std::vector<double> partial(static_cast<size_t>(kSgMaxSums(D)) * std::max<size_t>(T.chunk_begin.size(), 1), 0.0);
  for (size_t s = 0; s < T.stage_kind.size(); ++s) {
    if (hv) finite = sg_host_vote_elect<D>(c, s, oi, *hv, ist) && finite;
    if (T.stage_kind[s] != 1) {
      finite = sg_host_pass_fold<D, 0>(c, s, oi, partial, state, ist, hv) && finite;
      if (T.stage_kind[s] == 2) finite = sg_host_pass_fold<D, 3>(c, s, oi, partial, state, ist, hv) && finite;
      continue;
    }
    finite = sg_host_pass_fold<D, 1>(c, s, oi, partial, state, ist, hv) && finite;
    finite = sg_host_pass_fold<D, 2>(c, s, oi, partial, state, ist, hv) && finite;
    host_apply_stage<D>(c->odom, T, s, state, ist, oi);
  }
  return host_range_rows<D>(M, true, oi, deg, n_deg) && finite;
}
}  // extern "C++"

}  // namespace

int cora_set_sighting_placement(cora_ctx *c, const unsigned char *chain_fixed, const unsigned char *landmark_fixed, int min_sightings) {
  if (!c) return CORA_ERR_ARG;
  int rc = sg_check(c);
  if (rc) return rc;
  return install_tables(c, c->sg, [&](SgTables &T) { return sg_build(c, chain_fixed, landmark_fixed, min_sightings, T); },
                        [&](SgTables &T) { return sg_upload(c, T); });
}

int cora_sighting_placement_counts(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = static_cast<int64_t>(c->sg.stage_kind.size());
  out[1] = static_cast<int64_t>(c->sg.ent_e.size());
  out[2] = static_cast<int64_t>(c->sg.chunk_begin.size());
  out[3] = c->sg.skipped;
  return CORA_OK;
}

int cora_sighting_placement_order(const cora_ctx *c, int32_t *stage_kind, int32_t *stage_ptr, int32_t *items) {
  if (!c || !stage_kind || !stage_ptr || !items) return CORA_ERR_ARG;
  const SgTables &T = c->sg;
  std::copy(T.stage_kind.begin(), T.stage_kind.end(), stage_kind);
  std::copy(T.stage_list0.begin(), T.stage_list0.end(), stage_ptr);
  if (T.stage_list0.empty()) stage_ptr[0] = 0;
  std::copy(T.list_item.begin(), T.list_item.end(), items);
  return CORA_OK;
}

namespace {
// the consensus setting and the outputs of a robust call (cora_place_by_sightings_robust_dev)
struct SgConsensus {
  double barc2;
  int min_chain_consensus, min_landmark_consensus;
  int32_t *chain_consensus, *chain_list_len, *landmark_consensus, *landmark_list_len;
  unsigned char *inlier_chain, *inlier_landmark;
};
// the plain call's outputs
struct SgOutputs {
  int64_t *out;
  unsigned char *status;
  double *cost_start, *cost_final;
  int32_t *chosen;
  double *transforms;
  unsigned char *landmark_status;
  double *landmark_cost;
  unsigned char *degenerate;
};
const char *sg_not_finite(const SgConsensus *rb) {  // the refusal of a call whose flag word is set
  return rb ? "a sum or an elected hypothesis of the sighting placement is not finite" : "a sum of the sighting placement is not finite";
}
int sg_consensus_check(cora_ctx *c, double barc2, int min_chain_consensus, int min_landmark_consensus) {
  if (!(barc2 > 0.0) || !std::isfinite(barc2)) return fail(c, CORA_ERR_ARG, "barc2 must be finite and positive");
  if (min_chain_consensus < 1 || min_landmark_consensus < 1) return fail(c, CORA_ERR_ARG, "a minimum consensus must be at least 1");
  return CORA_OK;
}
// what a robust call returns beyond the plain call's: cint [lists][kSgCInts], inl [2][n_edges] (2 where an edge is in no list)
void sg_robust_results(const cora_ctx *c, const std::vector<int32_t> &ist, const std::vector<int32_t> &cint, const std::vector<unsigned char> &inl,
                       const SgConsensus &rb, int64_t out[10]) {
  const SgTables &T = c->sg;
  const size_t nch = T.chain_init.size(), nl = T.lm_init.size(), ne = static_cast<size_t>(c->meas.n_edges);
  auto per_item = [&](const std::vector<int32_t> &list_of, size_t n, int32_t *consensus, int32_t *list_len, int64_t *none) {
    *none = 0;
    for (size_t i = 0; i < n; ++i) {
      const int32_t list = list_of[i];
      size_t begin = 0, len = 0;
      if (list >= 0) sg_host_span(T, static_cast<size_t>(list), &begin, &len);
      if (list >= 0 && ist[static_cast<size_t>(list) * kSgInts] == 5) ++*none;
      if (consensus) consensus[i] = list >= 0 ? cint[static_cast<size_t>(list) * kSgCInts + 1] : 0;
      if (list_len) list_len[i] = static_cast<int32_t>(len);
    }
  };
  per_item(T.chain_list, nch, rb.chain_consensus, rb.chain_list_len, &out[6]);
  per_item(T.lm_list, nl, rb.landmark_consensus, rb.landmark_list_len, &out[7]);
  out[8] = out[9] = 0;
  for (size_t e = 0; e < ne; ++e) {
    out[8] += inl[e] == 0 ? 1 : 0;
    out[9] += inl[ne + e] == 0 ? 1 : 0;
  }
  if (rb.inlier_chain) std::copy(inl.begin(), inl.begin() + static_cast<std::ptrdiff_t>(ne), rb.inlier_chain);
  if (rb.inlier_landmark) std::copy(inl.begin() + static_cast<std::ptrdiff_t>(ne), inl.begin() + static_cast<std::ptrdiff_t>(2 * ne), rb.inlier_landmark);
}
// the device-pointer forms: rb null, the plain placement; else the consensus vote in front of the masked passes
int sg_place_dev(cora_ctx *c, double *dX, const SgConsensus *rb, const SgOutputs &o) {
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  SgTables &T = c->sg;
  const OdomTables &O = c->odom;
  const int d = L.d;
  const size_t ns = T.stage_kind.size(), nc = T.chunk_begin.size(), ne = T.ent_e.size(), nlist = T.list_item.size(), na = T.apply_pos.size();
  const size_t nedges = static_cast<size_t>(M.n_edges);
  SgRobustArgs R;
  SgArgs &A = R.A;
  A.d = d;
  A.n_edges = M.n_edges;
  A.pstride = static_cast<int64_t>(std::max<size_t>(nc, 1));
  A.chunk_begin = T.d_idx;
  A.chunk_len = A.chunk_begin + nc;
  A.chunk_list = A.chunk_len + nc;
  A.list_chunk0 = A.chunk_list + nc;
  A.list_row = A.list_chunk0 + nlist + 1;
  A.ent_rot = A.list_row + nlist;
  A.ent_trn = A.ent_rot + ne;
  A.ent_lm = A.ent_trn + ne;
  A.ent_e = A.ent_lm + ne;
  A.apply_pos = A.ent_e + ne;
  A.apply_list = A.apply_pos + na;
  A.pos_rot = O.d_idx + 2 * O.P;
  A.pos_trn = O.d_idx + 3 * O.P;
  A.edge_data = M.d_edge_data;
  A.partial = T.d_partial;
  A.state = T.d_state;
  A.istate = T.d_istate;
  A.x = dX;
  A.flag = c->d_flag;
  if (rb) {
    R.barc2 = rb->barc2;
    R.min_chain_consensus = rb->min_chain_consensus;
    R.min_landmark_consensus = rb->min_landmark_consensus;
    R.votes = T.d_votes;
    R.hyp = T.d_hyp;
    R.hstride = static_cast<int64_t>(std::max<size_t>(ne, 1));
    R.cstate = T.d_cstate;
    R.cint = T.d_cint;
    R.inlier_chain = T.d_inlier;
    R.inlier_landmark = T.d_inlier + std::max<size_t>(nedges, 1);
  }
  auto pass_fold = [&](int mode) {
    A.mode = mode;
    return rb ? launch_sighting_robust_pass_fold(R, c->stream) : launch_sighting_pass_fold(A, c->stream);
  };
  wrote(c, dX);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  if (rb) HIP_TRY(c, hipMemsetAsync(T.d_inlier, 2, 2 * std::max<size_t>(nedges, 1), c->stream));  // (an edge of no list)
  for (size_t s = 0; s < ns; ++s) {  // dependent: a stage reads the rows the stages before it wrote
    stage_args(T, s, A);
    if (rb) HIP_TRY(c, launch_sighting_vote_elect(R, T.stage_kind[s] == 1 ? 1 : 0, c->stream));
    if (T.stage_kind[s] != 1) {
      HIP_TRY(c, pass_fold(0));
      if (T.stage_kind[s] == 2) HIP_TRY(c, pass_fold(3));
      continue;
    }
    HIP_TRY(c, pass_fold(1));
    HIP_TRY(c, pass_fold(2));
    HIP_TRY(c, launch_sighting_apply(A, c->stream));
  }
  std::vector<double> state(nlist * kSgState(d));
  std::vector<int32_t> ist(nlist * kSgInts), cint(rb ? nlist * kSgCInts : 0);
  std::vector<unsigned char> inl(rb ? 2 * nedges : 0);
  int64_t n_deg = 0;
  const int rc = range_rows_step(c, dX, true, o.degenerate, sg_not_finite(rb), &n_deg, [&]() -> int {  // (after the chains' and the landmarks' rows)
    if (const int e = read_back_state(c, state, T.d_state, ist, T.d_istate)) return e;
    if (rb && nlist > 0) HIP_TRY(c, hipMemcpyAsync(cint.data(), T.d_cint, cint.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (rb && nedges > 0) {
      HIP_TRY(c, hipMemcpyAsync(inl.data(), R.inlier_chain, nedges, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(inl.data() + nedges, R.inlier_landmark, nedges, hipMemcpyDeviceToHost, c->stream));
    }
    return CORA_OK;
  });
  if (rc) return rc;
  sg_results(c, state, ist, n_deg, o.out, o.status, o.cost_start, o.cost_final, o.chosen, o.transforms, o.landmark_status, o.landmark_cost);
  if (rb) sg_robust_results(c, ist, cint, inl, *rb, o.out);
  return CORA_OK;
}
// the host mirrors (with_host_x), every hypothesis too through the function of kernels.h the kernels call
int sg_place_mirror(cora_ctx *c, double *X, int ldx, const SgConsensus *rb, const SgOutputs &o) {
  const int d = c->F.L.d;
  const size_t nlist = c->sg.list_item.size();
  std::vector<double> state(nlist * kSgState(d), 0.0);
  std::vector<int32_t> ist(nlist * kSgInts, 0);
  SgHostVote hv;
  if (rb) {
    hv.barc2 = rb->barc2;
    hv.min_chain_consensus = rb->min_chain_consensus;
    hv.min_landmark_consensus = rb->min_landmark_consensus;
    hv.cstate.assign(nlist * kSgCState(d), 0.0);
    hv.cint.assign(nlist * kSgCInts, 0);
    hv.inl.assign(2 * static_cast<size_t>(c->meas.n_edges), 2);
  }
  int64_t n_deg = 0;
  const int rc = with_host_x(c, X, ldx, sg_not_finite(rb), [&](auto D, double *oi) {
    return sg_host_run<D()>(c, oi, state, ist, o.degenerate, &n_deg, rb ? &hv : nullptr);
  });
  if (rc) return rc;
  sg_results(c, state, ist, n_deg, o.out, o.status, o.cost_start, o.cost_final, o.chosen, o.transforms, o.landmark_status, o.landmark_cost);
  if (rb) sg_robust_results(c, ist, hv.cint, hv.inl, *rb, o.out);
  return CORA_OK;
}
// what every form checks first: form 0 device-pointer | 1 host-pointer | 2 mirror
int sg_enter(cora_ctx *c, int form, const double *X, const int64_t *out, const SgConsensus *rb) {
  if (!c) return CORA_ERR_ARG;
  int rc = sg_check(c);
  if (rc) return rc;
  if (form != 2) NEED_DEVICE(c);
  if ((rc = sg_args_check(c, X, out))) return rc;
  return rb ? sg_consensus_check(c, rb->barc2, rb->min_chain_consensus, rb->min_landmark_consensus) : CORA_OK;
}
}  // namespace

int cora_place_by_sightings_dev(cora_ctx *c, double *dX, int64_t out[6], unsigned char *status, double *cost_start, double *cost_final,
                                int32_t *chosen, double *transforms, unsigned char *landmark_status, double *landmark_cost,
                                unsigned char *degenerate) {
  if (const int rc = sg_enter(c, 0, dX, out, nullptr)) return rc;
  return sg_place_dev(c, dX, nullptr, SgOutputs{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate});
}

int cora_place_by_sightings(cora_ctx *c, double *X, int ldx, int64_t out[6], unsigned char *status, double *cost_start, double *cost_final,
                            int32_t *chosen, double *transforms, unsigned char *landmark_status, double *landmark_cost,
                            unsigned char *degenerate) {
  if (const int rc = sg_enter(c, 1, X, out, nullptr)) return rc;
  const SgOutputs o{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate};
  return with_uploaded_x(c, X, ldx, [&](double *dX) { return sg_place_dev(c, dX, nullptr, o); });
}

// the host mirror (with_host_x)
int cora_debug_place_by_sightings_host(cora_ctx *c, double *X, int ldx, int64_t out[6], unsigned char *status, double *cost_start,
                                       double *cost_final, int32_t *chosen, double *transforms, unsigned char *landmark_status,
                                       double *landmark_cost, unsigned char *degenerate) {
  if (const int rc = sg_enter(c, 2, X, out, nullptr)) return rc;
  return sg_place_mirror(c, X, ldx, nullptr, SgOutputs{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate});
}

int cora_place_by_sightings_robust_dev(cora_ctx *c, double *dX, double barc2, int min_chain_consensus, int min_landmark_consensus, int64_t out[10],
                                       unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms,
                                       unsigned char *landmark_status, double *landmark_cost, unsigned char *degenerate, int32_t *chain_consensus,
                                       int32_t *chain_list_len, int32_t *landmark_consensus, int32_t *landmark_list_len,
                                       unsigned char *inlier_chain, unsigned char *inlier_landmark) {
  const SgConsensus rb{barc2, min_chain_consensus, min_landmark_consensus, chain_consensus, chain_list_len, landmark_consensus, landmark_list_len,
                       inlier_chain, inlier_landmark};
  if (const int rc = sg_enter(c, 0, dX, out, &rb)) return rc;
  return sg_place_dev(c, dX, &rb, SgOutputs{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate});
}

int cora_place_by_sightings_robust(cora_ctx *c, double *X, int ldx, double barc2, int min_chain_consensus, int min_landmark_consensus, int64_t out[10],
                                   unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms,
                                   unsigned char *landmark_status, double *landmark_cost, unsigned char *degenerate, int32_t *chain_consensus,
                                   int32_t *chain_list_len, int32_t *landmark_consensus, int32_t *landmark_list_len, unsigned char *inlier_chain,
                                   unsigned char *inlier_landmark) {
  const SgConsensus rb{barc2, min_chain_consensus, min_landmark_consensus, chain_consensus, chain_list_len, landmark_consensus, landmark_list_len,
                       inlier_chain, inlier_landmark};
  if (const int rc = sg_enter(c, 1, X, out, &rb)) return rc;
  const SgOutputs o{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate};
  return with_uploaded_x(c, X, ldx, [&](double *dX) { return sg_place_dev(c, dX, &rb, o); });
}

int cora_debug_place_by_sightings_robust_host(cora_ctx *c, double *X, int ldx, double barc2, int min_chain_consensus, int min_landmark_consensus,
                                              int64_t out[10], unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen,
                                              double *transforms, unsigned char *landmark_status, double *landmark_cost, unsigned char *degenerate,
                                              int32_t *chain_consensus, int32_t *chain_list_len, int32_t *landmark_consensus,
                                              int32_t *landmark_list_len, unsigned char *inlier_chain, unsigned char *inlier_landmark) {
  const SgConsensus rb{barc2, min_chain_consensus, min_landmark_consensus, chain_consensus, chain_list_len, landmark_consensus, landmark_list_len,
                       inlier_chain, inlier_landmark};
  if (const int rc = sg_enter(c, 2, X, out, &rb)) return rc;
  return sg_place_mirror(c, X, ldx, &rb, SgOutputs{out, status, cost_start, cost_final, chosen, transforms, landmark_status, landmark_cost, degenerate});
}
