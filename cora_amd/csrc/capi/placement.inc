// Part of capi.hip (one translation unit; included there, in this order).  chain placement from inter-robot ranges (a rigid motion per odometry chain from the pose-pose ranges between chains): order of the stages and entry tables, device-pointer form, host-pointer form, host mirror; the outlier-robust forms (a consensus vote over samples of kPlTerms(d) ranges in front of the batched fit: PlConsensus, PlHostVote) share every one of them.  Reads the measurement table, the chain tables and the row maps; writes nothing the handle computes with.  What it shares with the other initialisers -- the range-row step, the host-pointer and host-mirror wrappers, installing tables, chunk cutting, the mirror's sums -- is in capi/init_common.inc.

namespace {

int pl_check(cora_ctx *c) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the chain placement is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (!c->odom.built) return fail(c, CORA_ERR_NOT_READY, "no chain tables (cora_set_odometry_chains)");
  return CORA_OK;
}

// the order of the stages and their entry lists, from structure alone (host part of T only).  order CORA_PL_ORDER_GREEDY:
// one chain at a time, the one with the most entries against the chains placed so far; a stage is a level of its own.
// CORA_PL_ORDER_LEVELS: level k holds, in ascending chain index, every chain not yet placed with at least min_ranges
// entries against the chains of levels < k, and a stage's list only those entries -- a range to a chain of the same level
// is left out, which is what makes the stages of a level independent.
int pl_build(cora_ctx *c, const unsigned char *chain_fixed, int min_ranges, int order, PlTables &T) {
  if (order != CORA_PL_ORDER_GREEDY && order != CORA_PL_ORDER_LEVELS) return fail(c, CORA_ERR_ARG, "order must be CORA_PL_ORDER_GREEDY or CORA_PL_ORDER_LEVELS");
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  const OdomTables &O = c->odom;
  const int64_t nr = M.n_ranges, nch = O.n_chains;
  if (min_ranges < kPlUnknowns(L.d) + 1)
    return fail(c, CORA_ERR_ARG, "min_ranges must be at least " + std::to_string(kPlUnknowns(L.d) + 1) + ", the unknowns of the linear stage + 1");
  std::vector<unsigned char> placed;
  if (const int rc = seed_fixed_chains(c, chain_fixed, placed)) return rc;
  const ChainMaps maps = chain_maps(c);
  const std::vector<int32_t> &chain_of = maps.chain_of;
  // the ranges between two chains; cnt[c][c'] entries of c against c'
  std::vector<int32_t> use_m, use_ca, use_cb;
  std::vector<int64_t> cnt(static_cast<size_t>(nch * nch), 0);
  for (int64_t m = 0; m < nr; ++m) {
    const int32_t ca = chain_of[static_cast<size_t>(M.range_rows[static_cast<size_t>(nr + m)])];
    const int32_t cb = chain_of[static_cast<size_t>(M.range_rows[static_cast<size_t>(2 * nr + m)])];
    if (ca < 0 || cb < 0 || ca == cb) {
      ++T.skipped;
      continue;
    }
    use_m.push_back(static_cast<int32_t>(m));
    use_ca.push_back(ca);
    use_cb.push_back(cb);
    ++cnt[static_cast<size_t>(ca * nch + cb)];
    ++cnt[static_cast<size_t>(cb * nch + ca)];
  }
  if (nr >= (int64_t(1) << 31)) return fail(c, CORA_ERR_ARG, "the range table has more entries than a 32-bit index holds");
  T.min_ranges = min_ranges;
  T.chain_init.assign(static_cast<size_t>(nch), 0);
  for (int64_t ch = 0; ch < nch; ++ch) T.chain_init[static_cast<size_t>(ch)] = placed[static_cast<size_t>(ch)] ? 4 : 0;
  T.stage_chunk0.assign(1, 0);
  std::vector<int64_t> against(static_cast<size_t>(nch), 0);  // entries against placed chains
  for (int64_t ch = 0; ch < nch; ++ch)
    for (int64_t o = 0; o < nch; ++o)
      if (placed[static_cast<size_t>(o)]) against[static_cast<size_t>(ch)] += cnt[static_cast<size_t>(ch * nch + o)];
  T.order = order;
  T.level_stage0.assign(1, 0);
  T.level_tile0.assign(1, 0);
  // the stage of chain `take`: its entries against the chains placed at this moment, in table order
  auto add_stage = [&](int64_t take) {
    const size_t begin = T.ent_m.size();
    for (size_t u = 0; u < use_m.size(); ++u) {
      const int32_t m = use_m[u];
      const bool a_mine = use_ca[u] == take, b_mine = use_cb[u] == take;
      if (!(a_mine && placed[static_cast<size_t>(use_cb[u])]) && !(b_mine && placed[static_cast<size_t>(use_ca[u])])) continue;
      const int32_t ta = M.range_rows[static_cast<size_t>(nr + m)], tb = M.range_rows[static_cast<size_t>(2 * nr + m)];
      T.ent_q.push_back(a_mine ? ta : tb);
      T.ent_a.push_back(a_mine ? tb : ta);
      T.ent_m.push_back(m);
    }
    const int64_t len = static_cast<int64_t>(T.ent_m.size() - begin);
    const int32_t stage = static_cast<int32_t>(T.stage_chain.size()), npos = static_cast<int32_t>(maps.chain_pos[static_cast<size_t>(take)].size());
    cut_chunks(static_cast<int64_t>(begin), len, T.chunk_begin, T.chunk_len, &T.chunk_stage, stage);
    T.stage_chain.push_back(static_cast<int32_t>(take));
    T.stage_origin_q.push_back(T.ent_q[begin]);
    T.stage_origin_a.push_back(T.ent_a[begin]);
    T.stage_pos0.push_back(maps.chain_pos[static_cast<size_t>(take)].front());
    T.stage_npos.push_back(npos);
    T.stage_chunk0.push_back(static_cast<int32_t>(T.chunk_begin.size()));
    T.max_chunks = std::max<int64_t>(T.max_chunks, (len + kPlChunk - 1) / kPlChunk);
    for (int32_t off = 0; off < npos; off += 256) {
      T.tile_stage.push_back(stage);
      T.tile_off.push_back(off);
    }
  };
  auto now_placed = [&](int64_t take) {
    placed[static_cast<size_t>(take)] = 1;
    for (int64_t ch = 0; ch < nch; ++ch) against[static_cast<size_t>(ch)] += cnt[static_cast<size_t>(ch * nch + take)];
  };
  auto end_level = [&] {
    T.max_level_chunks = std::max<int64_t>(T.max_level_chunks, static_cast<int64_t>(T.chunk_begin.size()) - T.stage_chunk0[static_cast<size_t>(T.level_stage0.back())]);
    T.level_stage0.push_back(static_cast<int32_t>(T.stage_chain.size()));
    T.level_tile0.push_back(static_cast<int32_t>(T.tile_stage.size()));
  };
  while (order == CORA_PL_ORDER_GREEDY) {
    int64_t take = -1, most = -1;
    for (int64_t ch = 0; ch < nch; ++ch)
      if (!placed[static_cast<size_t>(ch)] && against[static_cast<size_t>(ch)] > most) {  // (ties: the lowest index)
        most = against[static_cast<size_t>(ch)];
        take = ch;
      }
    if (take < 0 || most < min_ranges) break;
    add_stage(take);
    now_placed(take);
    end_level();
  }
  while (order == CORA_PL_ORDER_LEVELS) {
    std::vector<int64_t> level;
    for (int64_t ch = 0; ch < nch; ++ch)
      if (!placed[static_cast<size_t>(ch)] && against[static_cast<size_t>(ch)] >= min_ranges) level.push_back(ch);
    if (level.empty()) break;
    for (const int64_t take : level) add_stage(take);  // (all against the chains of the levels before)
    for (const int64_t take : level) now_placed(take);
    end_level();
  }
  for (int64_t ch = 0; ch < nch; ++ch) {
    if (placed[static_cast<size_t>(ch)]) continue;
    int64_t n = 0;
    for (int64_t o = 0; o < nch; ++o) n += cnt[static_cast<size_t>(ch * nch + o)];
    T.chain_init[static_cast<size_t>(ch)] = n > 0 ? 1 : 3;
  }
  if (const int rc = range_rows_unique(c)) return rc;
  T.built = true;
  return CORA_OK;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int pl_upload(cora_ctx *c, PlTables &T) {
  HIP_TRY(c, upload_joined(&T.d_idx, {&T.chunk_begin, &T.chunk_len, &T.ent_q, &T.ent_a, &T.ent_m, &T.chunk_stage, &T.stage_chunk0, &T.stage_origin_q,
                                      &T.stage_origin_a, &T.stage_pos0, &T.stage_npos, &T.tile_stage, &T.tile_off}));
  const int d = c->F.L.d;
  const size_t ns = std::max<size_t>(T.stage_chain.size(), 1), nc = static_cast<size_t>(std::max<int64_t>(T.max_level_chunks, 1));  // (>= max_chunks)
  HIP_TRY(c, alloc_device(&T.d_partial, static_cast<size_t>(kPlSums(d)) * nc * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_state, static_cast<size_t>(kPlState(d)) * ns * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_istate, static_cast<size_t>(kPlInts) * ns * sizeof(int32_t)));
  return CORA_OK;
}

int pl_args_check(cora_ctx *c, const double *X, int gn_steps, const int64_t *out) {
  if (!c->pl.built) return fail(c, CORA_ERR_NOT_READY, "no placement tables (cora_set_chain_placement)");
  if (gn_steps < 0 || gn_steps > kPlMaxSteps) return fail(c, CORA_ERR_ARG, "gn_steps must be in [0, 16]");
  if (!X || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  return CORA_OK;
}

// the fields of the kernels' arguments that hold for every stage of a call on dX (pstride, and the stage's or level's own
// fields, are the caller's)
PlArgs pl_table_args(const cora_ctx *c, double *dX) {
  const PlTables &T = c->pl;
  const OdomTables &O = c->odom;
  const size_t nc = T.chunk_begin.size(), ne = T.ent_m.size();
  PlArgs A;
  A.d = c->F.L.d;
  A.n_ranges = c->meas.n_ranges;
  A.chunk_begin = T.d_idx;
  A.chunk_len = A.chunk_begin + nc;
  A.ent_q = A.chunk_len + nc;
  A.ent_a = A.ent_q + ne;
  A.ent_m = A.ent_a + ne;
  A.pos_rot = O.d_idx + 2 * O.P;
  A.pos_trn = O.d_idx + 3 * O.P;
  A.range_data = c->meas.d_range_data;
  A.partial = T.d_partial;
  A.x = dX;
  A.flag = c->d_flag;
  return A;
}

// what a call returns, from the stages' state ([stages][kPlState(d)], [stages][kPlInts])
void pl_results(const cora_ctx *c, const std::vector<double> &state, const std::vector<int32_t> &ist, int64_t n_deg, int64_t out[5],
                unsigned char *status, double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen, double *transforms) {
  const int d = c->F.L.d, G = kPlG(d);
  const PlTables &T = c->pl;
  const size_t nch = T.chain_init.size(), ns = T.stage_chain.size();
  int64_t not_placed = 0, steps = 0;
  for (size_t ch = 0; ch < nch; ++ch) {
    not_placed += T.chain_init[ch] == 1 || T.chain_init[ch] == 3 ? 1 : 0;
    if (status) status[ch] = T.chain_init[ch];
    if (cost_start) cost_start[ch] = 0.0;
    if (cost_linear) cost_linear[ch] = 0.0;
    if (cost_final) cost_final[ch] = 0.0;
    if (chosen) chosen[ch] = -1;
    if (transforms) identity_transform(d, transforms + ch * G);
  }
  for (size_t s = 0; s < ns; ++s) {
    const size_t ch = static_cast<size_t>(T.stage_chain[s]);
    const int32_t *li = ist.data() + s * kPlInts;
    const double *st = state.data() + s * kPlState(d);
    steps += li[2];
    if (status) status[ch] = static_cast<unsigned char>(li[0]);
    if (cost_start) cost_start[ch] = st[3 * G + 1];
    if (cost_linear) cost_linear[ch] = st[3 * G + 2];
    if (cost_final) cost_final[ch] = st[3 * G];
    if (chosen) chosen[ch] = li[1];
    if (transforms) std::copy(st + 2 * G, st + 3 * G, transforms + ch * G);
  }
  out[0] = static_cast<int64_t>(ns);
  out[1] = not_placed;
  out[2] = steps;
  out[3] = n_deg;
  out[4] = static_cast<int64_t>(ns);
}

// the consensus setting and the outputs of a robust call (cora_place_chains_robust_dev)
struct PlConsensus {
  double barc2;
  int min_consensus;
  int32_t *elected, *consensus, *list_len;
  unsigned char *inlier;
};
const char *pl_not_finite(const PlConsensus *rb) {  // the refusal of a call whose flag word is set
  return rb ? "a sum or a hypothesis of the chain placement is not finite" : "a sum of the chain placement is not finite";
}
int pl_consensus_check(cora_ctx *c, double barc2, int min_consensus) {
  if (!(barc2 > 0.0) || !std::isfinite(barc2)) return fail(c, CORA_ERR_ARG, "barc2 must be finite and positive");
  if (min_consensus < 1) return fail(c, CORA_ERR_ARG, "min_consensus must be at least 1");
  return CORA_OK;
}
// the first entry and the length of stage s's list
void pl_list_span(const PlTables &T, size_t s, size_t *begin, int32_t *len) {
  const size_t c0 = static_cast<size_t>(T.stage_chunk0[s]), c1 = static_cast<size_t>(T.stage_chunk0[s + 1]);
  *begin = static_cast<size_t>(T.chunk_begin[c0]);
  *len = T.chunk_begin[c1 - 1] + T.chunk_len[c1 - 1] - T.chunk_begin[c0];
}
// what a robust call returns beyond the batched call's: cint [stages][kPlCInts], inl [n_ranges] (2 where a range is in no
// stage list); a stage without consensus counts as not placed (out[1]) and not as placed (out[0])
void pl_robust_results(const cora_ctx *c, const std::vector<int32_t> &ist, const std::vector<int32_t> &cint, const std::vector<unsigned char> &inl,
                       const PlConsensus &rb, int64_t out[8]) {
  const PlTables &T = c->pl;
  const size_t nch = T.chain_init.size(), ns = T.stage_chain.size(), nr = static_cast<size_t>(c->meas.n_ranges);
  out[5] = static_cast<int64_t>(T.level_stage0.size()) - 1;
  out[6] = out[7] = 0;
  for (size_t ch = 0; ch < nch; ++ch) {
    if (rb.elected) rb.elected[ch] = -1;
    if (rb.consensus) rb.consensus[ch] = 0;
    if (rb.list_len) rb.list_len[ch] = 0;
  }
  for (size_t s = 0; s < ns; ++s) {
    const size_t ch = static_cast<size_t>(T.stage_chain[s]);
    size_t begin;
    int32_t len;
    pl_list_span(T, s, &begin, &len);
    if (ist[s * kPlInts] == 5) {  // (no consensus: not placed, though a stage)
      ++out[6];
      ++out[1];
      --out[0];
    }
    if (rb.elected) rb.elected[ch] = cint[s * kPlCInts];
    if (rb.consensus) rb.consensus[ch] = cint[s * kPlCInts + 1];
    if (rb.list_len) rb.list_len[ch] = len;
  }
  for (size_t m = 0; m < nr; ++m) out[7] += inl[m] == 0 ? 1 : 0;
  if (rb.inlier) std::copy(inl.begin(), inl.begin() + static_cast<std::ptrdiff_t>(nr), rb.inlier);
}

extern "C++" {  // (templates: this file is included inside extern "C")
// the consensus vote of a robust call on the host: the setting and the stages' elected hypotheses, as on the device
struct PlHostVote {
  double barc2;
  int min_consensus;
  std::vector<double> cstate;      // [stages][kPlCState(d)]
  std::vector<int32_t> cint;       // [stages][kPlCInts]
  std::vector<unsigned char> inl;  // [n_ranges]
};
// the hypothesis of entry h of stage s's list (begin, len), as k_pl_hyp takes it; work: kPlUnknowns(D) (kPlUnknowns(D) + 1)
template <int D>
bool pl_host_hypothesis(const cora_ctx *c, const double *oi, size_t s, size_t begin, int32_t len, int32_t h, double *work, double *g) {
  constexpr int NT = kPlTerms(D), NP = kPlSums(D);
  const PlTables &T = c->pl;
  const MeasurementTable &M = c->meas;
  const double *q0 = oi + static_cast<size_t>(T.stage_origin_q[s]) * D, *a0 = oi + static_cast<size_t>(T.stage_origin_a[s]) * D;
  double term[NT * NT], wt[NT], S[NP];
  auto entry = [&](int k, const double **q, const double **a, double *r, double *om) {
    const size_t e = begin + static_cast<size_t>(pl_sample<D>(h, k, len)), m = static_cast<size_t>(T.ent_m[e]);
    *q = oi + static_cast<size_t>(T.ent_q[e]) * D;
    *a = oi + static_cast<size_t>(T.ent_a[e]) * D;
    *r = M.range_data[m];
    *om = M.range_data[static_cast<size_t>(M.n_ranges) + m];
  };
  for (int k = 0; k < NT; ++k) {
    const double *q, *a;
    double r;
    entry(k, &q, &a, &r, &wt[k]);
    pl_linear_terms<D>(q0, a0, q, a, r, term + k * NT);
  }
  for (int p = 0; p < NP; ++p) {
    int i, j;
    pl_pair(NT, p, &i, &j);
    S[p] = pl_pair_sum(term, wt, NT, NT, i, j);
  }
  return pl_hypothesis<D>(S, work, q0, a0, entry, g);
}
// whether entry e of stage s is an inlier of the stage's elected hypothesis (pl_inlier, kernels/placement.inc)
template <int D>
bool pl_host_inlier(const cora_ctx *c, const double *oi, const PlHostVote &hv, size_t s, size_t e) {
  const PlTables &T = c->pl;
  const MeasurementTable &M = c->meas;
  const size_t m = static_cast<size_t>(T.ent_m[e]);
  double qq[D], aa[D];
  for (int k = 0; k < D; ++k) {
    qq[k] = oi[static_cast<size_t>(T.ent_q[e]) * D + k] - oi[static_cast<size_t>(T.stage_origin_q[s]) * D + k];
    aa[k] = oi[static_cast<size_t>(T.ent_a[e]) * D + k] - oi[static_cast<size_t>(T.stage_origin_a[s]) * D + k];
  }
  return hv.cint[s * kPlCInts + 1] > 0 &&
         cl_agrees(pl_cost_at<D>(hv.cstate.data() + s * kPlCState(D), qq, aa, M.range_data[m], M.range_data[static_cast<size_t>(M.n_ranges) + m]), hv.barc2);
}
// hypotheses, vote and election of stage s (k_pl_hyp, k_pl_vote, k_pl_elect): the votes are integers, so the order of the
// scoring is free
template <int D>
bool pl_host_vote_elect(const cora_ctx *c, const double *oi, size_t s, PlHostVote &hv, int32_t *li) {
  constexpr int G = kPlG(D), N = kPlUnknowns(D);
  const PlTables &T = c->pl;
  const MeasurementTable &M = c->meas;
  size_t begin;
  int32_t len;
  pl_list_span(T, s, &begin, &len);
  const double *q0 = oi + static_cast<size_t>(T.stage_origin_q[s]) * D, *a0 = oi + static_cast<size_t>(T.stage_origin_a[s]) * D;
  std::vector<double> ent(static_cast<size_t>(len) * (2 * D + 2)), work(N * (N + 1));  // q' | a' | r | omega
  for (int32_t j = 0; j < len; ++j) {
    const size_t e = begin + static_cast<size_t>(j), m = static_cast<size_t>(T.ent_m[e]);
    double *f = ent.data() + static_cast<size_t>(j) * (2 * D + 2);
    for (int k = 0; k < D; ++k) {
      f[k] = oi[static_cast<size_t>(T.ent_q[e]) * D + k] - q0[k];
      f[D + k] = oi[static_cast<size_t>(T.ent_a[e]) * D + k] - a0[k];
    }
    f[2 * D] = M.range_data[m];
    f[2 * D + 1] = M.range_data[static_cast<size_t>(M.n_ranges) + m];
  }
  int32_t bv = -1, be = len;
  double *best = hv.cstate.data() + s * kPlCState(D);
  for (int32_t h = 0; h < len; ++h) {
    double g[G];
    int32_t vote = 0;
    if (pl_host_hypothesis<D>(c, oi, s, begin, len, h, work.data(), g)) {
      for (int32_t j = 0; j < len; ++j) {
        const double *f = ent.data() + static_cast<size_t>(j) * (2 * D + 2);
        vote += cl_agrees(pl_cost_at<D>(g, f, f + D, f[2 * D], f[2 * D + 1]), hv.barc2) ? 1 : 0;
      }
    }
    if (cl_better(vote, h, bv, be)) {
      bv = vote;
      be = h;
      std::copy(g, g + G, best);
    }
  }
  hv.cint[s * kPlCInts] = be;
  hv.cint[s * kPlCInts + 1] = bv;
  li[0] = bv < hv.min_consensus ? 5 : 0;
  li[1] = -1;
  return odom_finite(best, G);
}
// the whole placement on the host, in the kernels' order: oi a d-column resident vector; state and ist as on the device
template <int D>
bool pl_host_run(const cora_ctx *c, int gn_steps, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg,
                 int64_t *n_deg, PlHostVote *hv = nullptr) {  // hv: over the inliers of the elected hypotheses (an entry outside adds +0.0 terms)
  constexpr int NT = kPlTerms(D), NP = kPlSums(D), NS = kPlGnSums(D), N = kPlUnknowns(D), G = kPlG(D);
  const PlTables &T = c->pl;
  const OdomTables &O = c->odom;
  const MeasurementTable &M = c->meas;
  const int64_t nr = M.n_ranges;
  const size_t ns = T.stage_chain.size(), stride = static_cast<size_t>(std::max<int64_t>(T.max_chunks, 1));
  bool finite = true;
  std::vector<double> partial(static_cast<size_t>(NP) * stride, 0.0), term(static_cast<size_t>(kPlChunk) * NT), wt(kPlChunk), work(N * (N + 1));
  std::vector<unsigned char> in(kPlChunk, 1);
  for (size_t s = 0; s < ns; ++s) {
    const size_t c0 = static_cast<size_t>(T.stage_chunk0[s]), nc = static_cast<size_t>(T.stage_chunk0[s + 1]) - c0;
    const double *q0 = oi + static_cast<size_t>(T.stage_origin_q[s]) * D, *a0 = oi + static_cast<size_t>(T.stage_origin_a[s]) * D;
    double *st = state.data() + s * kPlState(D);
    int32_t *li = ist.data() + s * kPlInts;
    if (hv) finite = pl_host_vote_elect<D>(c, oi, s, *hv, li) && finite;
    for (size_t ch = 0; ch < nc; ++ch) {
      const int len = T.chunk_len[c0 + ch];
      for (int i = 0; i < len; ++i) {
        const size_t e = static_cast<size_t>(T.chunk_begin[c0 + ch]) + i, m = static_cast<size_t>(T.ent_m[e]);
        pl_linear_terms<D>(q0, a0, oi + static_cast<size_t>(T.ent_q[e]) * D, oi + static_cast<size_t>(T.ent_a[e]) * D, M.range_data[m],
                           term.data() + static_cast<size_t>(i) * NT);
        wt[static_cast<size_t>(i)] = M.range_data[static_cast<size_t>(nr) + m];
        if (hv) hv->inl[m] = in[static_cast<size_t>(i)] = pl_host_inlier<D>(c, oi, *hv, s, e) ? 1 : 0;
      }
      for (int p = 0; p < NP; ++p) {
        int i, j;
        pl_pair(NT, p, &i, &j);
        partial[static_cast<size_t>(p) * stride + ch] = hv ? pl_pair_sum_masked(term.data(), wt.data(), in.data(), len, NT, i, j) : pl_pair_sum(term.data(), wt.data(), len, NT, i, j);
      }
    }
    double S[NP];
    host_list_sums<NP>(partial.data(), stride, 0, nc, S);
    finite = (hv ? pl_fold_linear_robust<D>(S, work.data(), st, li, q0, a0) : pl_fold_linear<D>(S, work.data(), st, li, q0, a0)) && finite;
    for (int step = 0; step <= gn_steps + 1; ++step) {
      const double *g = st + (step == 0 ? G : 0);
      for (size_t ch = 0; ch < nc; ++ch)
        host_chunk_sums<NS>(T.chunk_len[c0 + ch], [&](int i, double *t) {
          const size_t e = static_cast<size_t>(T.chunk_begin[c0 + ch]) + i, m = static_cast<size_t>(T.ent_m[e]);
          if (hv && !pl_host_inlier<D>(c, oi, *hv, s, e)) return;
          pl_gn_terms<D>(g, st[3 * G + 4], q0, a0, oi + static_cast<size_t>(T.ent_q[e]) * D, oi + static_cast<size_t>(T.ent_a[e]) * D,
                         M.range_data[m], M.range_data[static_cast<size_t>(nr) + m], t);
        }, partial.data(), stride, ch);
      double Sg[NS];
      host_list_sums<NS>(partial.data(), stride, 0, nc, Sg);
      const int last = step == gn_steps + 1 ? 1 : 0;
      finite = (hv ? pl_fold_gn_robust<D>(step, last, Sg, st, li, q0, a0) : pl_fold_gn<D>(step, last, Sg, st, li, q0, a0)) && finite;
    }
    if (li[1] > 0 && li[0] != 5)
      for (int64_t i = 0; i < T.stage_npos[s]; ++i) {
        const size_t pos = static_cast<size_t>(T.stage_pos0[s] + i);
        pl_apply<D>(st + 2 * G, oi + static_cast<size_t>(O.pos_rot[pos]) * D, oi + static_cast<size_t>(O.pos_trn[pos]) * D);
      }
  }
  return host_range_rows<D>(M, true, oi, deg, n_deg) && finite;
}
}  // extern "C++"

}  // namespace

int cora_set_chain_placement(cora_ctx *c, const unsigned char *chain_fixed, int min_ranges) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  return install_tables(c, c->pl, [&](PlTables &T) { return pl_build(c, chain_fixed, min_ranges, CORA_PL_ORDER_GREEDY, T); }, [&](PlTables &T) { return pl_upload(c, T); });
}

int cora_set_chain_placement_order(cora_ctx *c, const unsigned char *chain_fixed, int min_ranges, int order) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  return install_tables(c, c->pl, [&](PlTables &T) { return pl_build(c, chain_fixed, min_ranges, order, T); }, [&](PlTables &T) { return pl_upload(c, T); });
}

int cora_chain_placement_counts(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = static_cast<int64_t>(c->pl.stage_chain.size());
  out[1] = static_cast<int64_t>(c->pl.ent_m.size());
  out[2] = static_cast<int64_t>(c->pl.chunk_begin.size());
  out[3] = c->pl.skipped;
  return CORA_OK;
}

int cora_chain_placement_order(const cora_ctx *c, int32_t *stage_chain) {
  if (!c || !stage_chain) return CORA_ERR_ARG;
  std::copy(c->pl.stage_chain.begin(), c->pl.stage_chain.end(), stage_chain);
  return CORA_OK;
}

namespace {
// both device-pointer forms: stage after stage (17 launches per stage at 5 steps), or level after level with every launch
// serving all stages of the level (the same number per level); then the range rows and the results
int pl_place_dev(cora_ctx *c, double *dX, int gn_steps, bool batched, const PlConsensus *rb, int64_t *out, unsigned char *status, double *cost_start,
                 double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  int rc = pl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = pl_args_check(c, dX, gn_steps, out))) return rc;
  PlTables &T = c->pl;
  const int d = c->F.L.d;
  const size_t ns = T.stage_chain.size(), nl = T.level_stage0.size() - 1, nr = static_cast<size_t>(c->meas.n_ranges);
  if (rb) {
    // The vote's scratch, at the first robust call on these tables and not in the set call's upload as the other robust forms
    // have it: the plain and batched calls then hold what they held before.  Each pointer on its own: a call that failed
    // half-way leaves what it got to the tables, and the next call allocates the rest.
    const size_t ne = std::max<size_t>(T.ent_m.size(), 1), nst = std::max<size_t>(ns, 1);
    if (!T.d_votes) HIP_TRY(c, alloc_device(&T.d_votes, ne * sizeof(int32_t)));
    if (!T.d_hyp) HIP_TRY(c, alloc_device(&T.d_hyp, static_cast<size_t>(kPlG(d)) * ne * sizeof(double)));
    if (!T.d_cstate) HIP_TRY(c, alloc_device(&T.d_cstate, static_cast<size_t>(kPlCState(d)) * nst * sizeof(double)));
    if (!T.d_cint) HIP_TRY(c, alloc_device(&T.d_cint, static_cast<size_t>(kPlCInts) * nst * sizeof(int32_t)));
    if (!T.d_inlier) HIP_TRY(c, alloc_device(&T.d_inlier, std::max<size_t>(nr, 1)));
  }
  PlArgs A = pl_table_args(c, dX);
  wrote(c, dX);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  if (rb && nr > 0) HIP_TRY(c, hipMemsetAsync(T.d_inlier, 2, nr, c->stream));  // (a range of no stage list)
  // linear stage, evaluations 0 .. gn_steps + 1, apply: of one stage (PlArgs) or of one level (PlBatchArgs)
  auto launches = [&](auto &K, PlArgs &S) -> int {
    S.step = 0;
    S.last = 0;
    HIP_TRY(c, launch_place_linear(K, c->stream));
    for (int step = 0; step <= gn_steps + 1; ++step) {
      S.step = step;
      S.last = step == gn_steps + 1 ? 1 : 0;
      HIP_TRY(c, launch_place_gn(K, c->stream));
    }
    HIP_TRY(c, launch_place_apply(K, c->stream));
    return static_cast<int>(CORA_OK);
  };
  if (!batched) {
    A.pstride = std::max<int64_t>(T.max_chunks, 1);
    for (size_t s = 0; s < ns; ++s) {  // dependent: a stage reads the rows the stages before it wrote
      A.chunk0 = T.stage_chunk0[s];
      A.n_chunks = T.stage_chunk0[s + 1] - T.stage_chunk0[s];
      A.origin_q = T.stage_origin_q[s];
      A.origin_a = T.stage_origin_a[s];
      A.pos0 = T.stage_pos0[s];
      A.n_pos = T.stage_npos[s];
      A.state = T.d_state + s * kPlState(d);
      A.istate = T.d_istate + s * kPlInts;
      if ((rc = launches(A, A))) return rc;
    }
  } else {
    PlBatchArgs B;
    A.pstride = std::max<int64_t>(T.max_level_chunks, 1);
    A.state = T.d_state;
    A.istate = T.d_istate;
    B.A = A;
    B.chunk_stage = A.ent_m + T.ent_m.size();
    B.stage_chunk0 = B.chunk_stage + T.chunk_begin.size();
    B.stage_origin_q = B.stage_chunk0 + ns + 1;
    B.stage_origin_a = B.stage_origin_q + ns;
    B.stage_pos0 = B.stage_origin_a + ns;
    B.stage_npos = B.stage_pos0 + ns;
    B.tile_stage = B.stage_npos + ns;
    B.tile_off = B.tile_stage + T.tile_stage.size();
    for (size_t l = 0; l < nl; ++l) {  // dependent: a level reads the rows the levels before it wrote
      const size_t s0 = static_cast<size_t>(T.level_stage0[l]), s1 = static_cast<size_t>(T.level_stage0[l + 1]);
      B.stage0 = static_cast<int32_t>(s0);
      B.n_stages = static_cast<int32_t>(s1 - s0);
      B.A.chunk0 = T.stage_chunk0[s0];
      B.A.n_chunks = T.stage_chunk0[s1] - T.stage_chunk0[s0];
      B.tile0 = T.level_tile0[l];
      B.n_tiles = T.level_tile0[l + 1] - T.level_tile0[l];
      if (!rb) {
        if ((rc = launches(B, B.A))) return rc;
        continue;
      }
      // the consensus vote in front of the masked launches: hypotheses, vote, election of the level's stages
      PlRobustArgs R;
      R.B = B;
      R.barc2 = rb->barc2;
      R.min_consensus = rb->min_consensus;
      R.ent0 = T.chunk_begin[static_cast<size_t>(T.stage_chunk0[s0])];
      R.n_ent = T.chunk_begin[static_cast<size_t>(T.stage_chunk0[s1]) - 1] + T.chunk_len[static_cast<size_t>(T.stage_chunk0[s1]) - 1] - R.ent0;
      R.hstride = static_cast<int64_t>(T.ent_m.size());
      R.hyp = T.d_hyp;
      R.votes = T.d_votes;
      R.cstate = T.d_cstate;
      R.cint = T.d_cint;
      R.inlier = T.d_inlier;
      HIP_TRY(c, launch_place_vote_elect(R, c->stream));
      if ((rc = launches(R, R.B.A))) return rc;
    }
  }
  std::vector<double> state(ns * kPlState(d));
  std::vector<int32_t> ist(ns * kPlInts), cint(rb ? ns * kPlCInts : 0, 0);
  std::vector<unsigned char> inl(rb ? nr : 0);
  int64_t n_deg = 0;
  if ((rc = range_rows_step(c, dX, true, degenerate, pl_not_finite(rb), &n_deg, [&]() -> int {  // (after the chains' rows)
         if (const int e = read_back_state(c, state, T.d_state, ist, T.d_istate)) return e;
         if (rb && ns > 0) HIP_TRY(c, hipMemcpyAsync(cint.data(), T.d_cint, cint.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
         if (rb && nr > 0) HIP_TRY(c, hipMemcpyAsync(inl.data(), T.d_inlier, nr, hipMemcpyDeviceToHost, c->stream));
         return CORA_OK;
       })))
    return rc;
  pl_results(c, state, ist, n_deg, out, status, cost_start, cost_linear, cost_final, chosen, transforms);
  if (batched) out[5] = static_cast<int64_t>(nl);
  if (rb) pl_robust_results(c, ist, cint, inl, *rb, out);
  return CORA_OK;
}
}  // namespace

int cora_chain_placement_levels(const cora_ctx *c, int32_t *stage_level) {
  if (!c || !stage_level) return CORA_ERR_ARG;
  const std::vector<int32_t> &l0 = c->pl.level_stage0;
  for (size_t l = 0; l + 1 < l0.size(); ++l) std::fill(stage_level + l0[l], stage_level + l0[l + 1], static_cast<int32_t>(l + 1));  // (level 0: the fixed chains)
  return CORA_OK;
}

int cora_place_chains_dev(cora_ctx *c, double *dX, int gn_steps, int64_t out[5], unsigned char *status, double *cost_start,
                          double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  return pl_place_dev(c, dX, gn_steps, false, nullptr, out, status, cost_start, cost_linear, cost_final, chosen, transforms, degenerate);
}

int cora_place_chains_batched_dev(cora_ctx *c, double *dX, int gn_steps, int64_t out[6], unsigned char *status, double *cost_start,
                                  double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  return pl_place_dev(c, dX, gn_steps, true, nullptr, out, status, cost_start, cost_linear, cost_final, chosen, transforms, degenerate);
}

int cora_place_chains_batched(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[6], unsigned char *status, double *cost_start,
                              double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = pl_args_check(c, X, gn_steps, out))) return rc;
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return cora_place_chains_batched_dev(c, dX, gn_steps, out, status, cost_start, cost_linear, cost_final, chosen, transforms, degenerate);
  });
}

int cora_place_chains(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[5], unsigned char *status, double *cost_start,
                      double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = pl_args_check(c, X, gn_steps, out))) return rc;
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return cora_place_chains_dev(c, dX, gn_steps, out, status, cost_start, cost_linear, cost_final, chosen, transforms, degenerate);
  });
}

// the host mirror (with_host_x)
int cora_debug_place_chains_host(cora_ctx *c, double *X, int ldx, int gn_steps, int64_t out[5], unsigned char *status, double *cost_start,
                                 double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  if ((rc = pl_args_check(c, X, gn_steps, out))) return rc;
  const size_t ns = c->pl.stage_chain.size();
  std::vector<double> state(ns * kPlState(c->F.L.d), 0.0);
  std::vector<int32_t> ist(ns * kPlInts, 0);
  int64_t n_deg = 0;
  if ((rc = with_host_x(c, X, ldx, "a sum of the chain placement is not finite",
                        [&](auto D, double *oi) { return pl_host_run<D()>(c, gn_steps, oi, state, ist, degenerate, &n_deg); })))
    return rc;
  pl_results(c, state, ist, n_deg, out, status, cost_start, cost_linear, cost_final, chosen, transforms);
  return CORA_OK;
}

// the outlier-robust forms: the consensus vote in front of the batched fit (kernels.h, PlRobustArgs)
int cora_place_chains_robust_dev(cora_ctx *c, double *dX, int gn_steps, double barc2, int min_consensus, int64_t out[8], unsigned char *status,
                                 double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, int32_t *elected,
                                 int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = pl_args_check(c, dX, gn_steps, out)) || (rc = pl_consensus_check(c, barc2, min_consensus))) return rc;
  const PlConsensus rb{barc2, min_consensus, elected, consensus, list_len, inlier};
  return pl_place_dev(c, dX, gn_steps, true, &rb, out, status, cost_start, cost_linear, cost_final, chosen, transforms, degenerate);
}

int cora_place_chains_robust(cora_ctx *c, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[8], unsigned char *status,
                             double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen, double *transforms, int32_t *elected,
                             int32_t *consensus, int32_t *list_len, unsigned char *inlier, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = pl_args_check(c, X, gn_steps, out)) || (rc = pl_consensus_check(c, barc2, min_consensus))) return rc;
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return cora_place_chains_robust_dev(c, dX, gn_steps, barc2, min_consensus, out, status, cost_start, cost_linear, cost_final, chosen, transforms,
                                        elected, consensus, list_len, inlier, degenerate);
  });
}

// the host mirror (with_host_x)
int cora_debug_place_chains_robust_host(cora_ctx *c, double *X, int ldx, int gn_steps, double barc2, int min_consensus, int64_t out[8],
                                        unsigned char *status, double *cost_start, double *cost_linear, double *cost_final, int32_t *chosen,
                                        double *transforms, int32_t *elected, int32_t *consensus, int32_t *list_len, unsigned char *inlier,
                                        unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = pl_check(c);
  if (rc) return rc;
  if ((rc = pl_args_check(c, X, gn_steps, out)) || (rc = pl_consensus_check(c, barc2, min_consensus))) return rc;
  const int d = c->F.L.d;
  const size_t ns = c->pl.stage_chain.size();
  const PlConsensus rb{barc2, min_consensus, elected, consensus, list_len, inlier};
  std::vector<double> state(ns * kPlState(d), 0.0);
  std::vector<int32_t> ist(ns * kPlInts, 0);
  PlHostVote hv{barc2, min_consensus, std::vector<double>(ns * kPlCState(d), 0.0), std::vector<int32_t>(ns * kPlCInts, 0),
                std::vector<unsigned char>(static_cast<size_t>(c->meas.n_ranges), 2)};
  int64_t n_deg = 0;
  if ((rc = with_host_x(c, X, ldx, pl_not_finite(&rb),
                        [&](auto D, double *oi) { return pl_host_run<D()>(c, gn_steps, oi, state, ist, degenerate, &n_deg, &hv); })))
    return rc;
  pl_results(c, state, ist, n_deg, out, status, cost_start, cost_linear, cost_final, chosen, transforms);
  pl_robust_results(c, ist, hv.cint, hv.inl, rb, out);
  return CORA_OK;
}
