// Part of capi.hip (one translation unit; included there, in this order).  placement of odometry chains from inter-chain relative-pose edges (closures; the weighted rigid alignment of a chain onto chains placed before it, rotation and translation residuals together): order of the stages and list tables, device-pointer form, host-pointer form, host mirror, each plain and with the consensus vote in front of the fit (cora_place_by_closures_robust_dev).  Reads the measurement table and the chain tables; writes nothing the handle computes with.  What it shares with the other initialisers -- the range-row step, the host-pointer and host-mirror wrappers, installing tables, chunk cutting, the mirror's sums -- is in capi/init_common.inc.

namespace {

int cl_check(cora_ctx *c) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the closure placement is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (!c->odom.built) return fail(c, CORA_ERR_NOT_READY, "no chain tables (cora_set_odometry_chains)");
  return CORA_OK;
}

// the order of the stages and their lists, from structure alone (host part of T only)
int cl_build(cora_ctx *c, const unsigned char *chain_fixed, int min_closures, ClTables &T) {
  const MeasurementTable &M = c->meas;
  const OdomTables &O = c->odom;
  const int64_t ne = M.n_edges, nch = O.n_chains;
  if (min_closures < 1) return fail(c, CORA_ERR_ARG, "min_closures must be at least 1");
  if (ne >= (int64_t(1) << 31)) return fail(c, CORA_ERR_ARG, "the edge table has more entries than a 32-bit index holds");
  std::vector<unsigned char> placed;
  if (const int rc = seed_fixed_chains(c, chain_fixed, placed)) return rc;
  const std::vector<unsigned char> fixed = placed;
  const ChainMaps maps = chain_maps(c);
  const std::vector<int32_t> &chain_of = maps.chain_of;
  const std::vector<std::vector<int32_t>> &chain_pos = maps.chain_pos;
  std::vector<unsigned char> chain_edge(static_cast<size_t>(ne), 0);
  for (const int32_t e : O.pos_edge)
    if (e >= 0) chain_edge[static_cast<size_t>(e)] = 1;
  // the closures in table order: edge, chain of a, chain of b   (edge_rows: [ra | rb | ta | tb][edge])
  std::vector<int32_t> c_e, c_a, c_b;
  for (int64_t e = 0; e < ne; ++e) {
    if (M.edge_rows[static_cast<size_t>(ne + e)] < 0 || chain_edge[static_cast<size_t>(e)]) continue;  // a sighting, an edge of a chain
    const int32_t ca = chain_of[static_cast<size_t>(M.edge_rows[static_cast<size_t>(2 * ne + e)])];
    const int32_t cb = chain_of[static_cast<size_t>(M.edge_rows[static_cast<size_t>(3 * ne + e)])];
    if (ca < 0 || cb < 0 || ca == cb) {
      ++T.skipped;
      continue;
    }
    c_e.push_back(static_cast<int32_t>(e));
    c_a.push_back(ca);
    c_b.push_back(cb);
  }
  const size_t ncl = c_e.size();
  T.min_closures = min_closures;
  T.stage_list0.assign(1, 0);
  T.stage_apply0.assign(1, 0);
  T.list_chunk0.assign(1, 0);
  T.chain_list.assign(static_cast<size_t>(nch), -1);
  for (;;) {
    // EVERY unplaced chain with min_closures closures against chains placed before this stage, in ONE stage
    std::vector<std::vector<size_t>> members(static_cast<size_t>(nch));
    for (size_t u = 0; u < ncl; ++u) {
      const size_t a = static_cast<size_t>(c_a[u]), b = static_cast<size_t>(c_b[u]);
      if (placed[a] && !placed[b]) members[b].push_back(u);
      else if (placed[b] && !placed[a]) members[a].push_back(u);
    }
    std::vector<int32_t> chains;
    for (int64_t ch = 0; ch < nch; ++ch) {
      const std::vector<size_t> &mb = members[static_cast<size_t>(ch)];
      if (mb.empty() || static_cast<int64_t>(mb.size()) < min_closures) continue;
      const int32_t list = static_cast<int32_t>(T.list_item.size());
      T.chain_list[static_cast<size_t>(ch)] = list;
      for (const int32_t pos : chain_pos[static_cast<size_t>(ch)]) {
        T.apply_pos.push_back(pos);
        T.apply_list.push_back(list);
      }
      const size_t begin = T.ent_e.size();
      for (const size_t u : mb) {
        T.ent_e.push_back(c_e[u]);
        T.ent_dir.push_back(c_a[u] == ch ? 1 : 0);
      }
      cut_chunks(static_cast<int64_t>(begin), static_cast<int64_t>(mb.size()), T.chunk_begin, T.chunk_len, &T.chunk_list, list);
      T.list_item.push_back(static_cast<int32_t>(ch));
      T.list_chunk0.push_back(static_cast<int32_t>(T.chunk_begin.size()));
      chains.push_back(static_cast<int32_t>(ch));
    }
    if (chains.empty()) break;
    T.stage_list0.push_back(static_cast<int32_t>(T.list_item.size()));
    T.stage_apply0.push_back(static_cast<int32_t>(T.apply_pos.size()));
    for (const int32_t ch : chains) placed[static_cast<size_t>(ch)] = 1;
  }
  T.unused = static_cast<int64_t>(ncl) - static_cast<int64_t>(T.ent_e.size());
  std::vector<unsigned char> has(static_cast<size_t>(nch), 0);
  for (size_t u = 0; u < ncl; ++u) has[static_cast<size_t>(c_a[u])] = has[static_cast<size_t>(c_b[u])] = 1;
  T.chain_init.assign(static_cast<size_t>(nch), 0);
  for (int64_t ch = 0; ch < nch; ++ch) {
    const size_t i = static_cast<size_t>(ch);
    T.chain_init[i] = fixed[i] ? 4 : (T.chain_list[i] >= 0 ? 0 : (has[i] ? 1 : 3));
  }
  if (T.ent_e.size() >= (size_t(1) << 31)) return fail(c, CORA_ERR_ARG, "the lists have more entries than a 32-bit index holds");
  if (const int rc = range_rows_unique(c)) return rc;
  T.built = true;
  return CORA_OK;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int cl_upload(cora_ctx *c, ClTables &T) {
  HIP_TRY(c, upload_joined(&T.d_idx, {&T.chunk_begin, &T.chunk_len, &T.chunk_list, &T.list_chunk0, &T.ent_e, &T.ent_dir, &T.apply_pos, &T.apply_list}));
  const int d = c->F.L.d;
  const size_t nlist = std::max<size_t>(T.list_item.size(), 1), nc = std::max<size_t>(T.chunk_begin.size(), 1);
  HIP_TRY(c, alloc_device(&T.d_partial, static_cast<size_t>(kClSums(d)) * nc * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_state, static_cast<size_t>(kSgState(d)) * nlist * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_istate, static_cast<size_t>(kSgInts) * nlist * sizeof(int32_t)));
  // the consensus vote's scratch
  HIP_TRY(c, alloc_device(&T.d_votes, std::max<size_t>(T.ent_e.size(), 1) * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_cstate, static_cast<size_t>(kClCState(d)) * nlist * sizeof(double)));
  HIP_TRY(c, alloc_device(&T.d_cint, static_cast<size_t>(kClCInts) * nlist * sizeof(int32_t)));
  HIP_TRY(c, alloc_device(&T.d_inlier, std::max<size_t>(static_cast<size_t>(c->meas.n_edges), 1)));
  return CORA_OK;
}

int cl_args_check(cora_ctx *c, const double *X, const int64_t *out) {
  if (!c->cl.built) return fail(c, CORA_ERR_NOT_READY, "no closure tables (cora_set_closure_placement)");
  if (!X || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  return CORA_OK;
}

// the kernels' arguments of a call on the resident vector dX: the tables' device side
void cl_fill_args(cora_ctx *c, double *dX, ClArgs &A) {
  const MeasurementTable &M = c->meas;
  ClTables &T = c->cl;
  const OdomTables &O = c->odom;
  const size_t nc = T.chunk_begin.size(), ne = T.ent_e.size(), nlist = T.list_item.size(), na = T.apply_pos.size();
  A.d = c->F.L.d;
  A.n_edges = M.n_edges;
  A.pstride = static_cast<int64_t>(std::max<size_t>(nc, 1));
  A.chunk_begin = T.d_idx;
  A.chunk_len = A.chunk_begin + nc;
  A.chunk_list = A.chunk_len + nc;
  A.list_chunk0 = A.chunk_list + nc;
  A.ent_e = A.list_chunk0 + nlist + 1;
  A.ent_dir = A.ent_e + ne;
  A.apply_pos = A.ent_dir + ne;
  A.apply_list = A.apply_pos + na;
  A.pos_rot = O.d_idx + 2 * O.P;
  A.pos_trn = O.d_idx + 3 * O.P;
  A.edge_rows = M.d_edge_rows;
  A.edge_data = M.d_edge_data;
  A.partial = T.d_partial;
  A.state = T.d_state;
  A.istate = T.d_istate;
  A.x = dX;
  A.flag = c->d_flag;
}

// what a call returns, from the lists' state ([lists][kSgState(d)], [lists][kSgInts])
void cl_results(const cora_ctx *c, const std::vector<double> &state, const std::vector<int32_t> &ist, int64_t n_deg, int64_t out[5],
                unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms) {
  const int d = c->F.L.d, G = kSgG(d), NS = kSgState(d);
  const ClTables &T = c->cl;
  const size_t nch = T.chain_init.size();
  for (int i = 0; i < 5; ++i) out[i] = 0;
  for (size_t ch = 0; ch < nch; ++ch) {
    const int32_t list = T.chain_list[ch];
    const int32_t *li = list >= 0 ? ist.data() + static_cast<size_t>(list) * kSgInts : nullptr;
    const double *st = list >= 0 ? state.data() + static_cast<size_t>(list) * NS : nullptr;
    const int s = li ? li[0] : T.chain_init[ch];
    out[0] += s == 0 ? 1 : 0;
    out[1] += s == 1 || s == 2 || s == 3 ? 1 : 0;
    out[4] += s == 2 ? 1 : 0;
    if (status) status[ch] = static_cast<unsigned char>(s);
    if (cost_start) cost_start[ch] = st ? st[G + d] : 0.0;
    if (cost_final) cost_final[ch] = st ? st[G + d + 1] : 0.0;
    if (chosen) chosen[ch] = li ? li[1] : -1;
    if (transforms && li && li[1] > 0) std::copy(st, st + G, transforms + ch * G);
    else if (transforms) identity_transform(d, transforms + ch * G);
  }
  out[2] = n_deg;
  out[3] = static_cast<int64_t>(T.stage_list0.size()) - 1;
}

extern "C++" {  // (templates: this file is included inside extern "C")
template <int D>
void cl_host_entry(const cora_ctx *c, const double *oi, size_t e, double *P, double *q, double *l, double *res, double *kt) {
  constexpr int NF = D * D + D + 2;
  const ClTables &T = c->cl;
  const MeasurementTable &M = c->meas;
  const size_t ne = static_cast<size_t>(M.n_edges), m = static_cast<size_t>(T.ent_e[e]);
  double f[NF];
  for (int i = 0; i < NF; ++i) f[i] = M.edge_data[static_cast<size_t>(i) * ne + m];
  cl_entry<D>(oi + static_cast<size_t>(M.edge_rows[m]) * D, oi + static_cast<size_t>(M.edge_rows[2 * ne + m]) * D,
              oi + static_cast<size_t>(M.edge_rows[ne + m]) * D, oi + static_cast<size_t>(M.edge_rows[3 * ne + m]) * D, f, T.ent_dir[e], P, q, l, res);
  kt[0] = f[D * D + D];
  kt[1] = f[D * D + D + 1];
}
// the consensus vote of a robust call on the host: the setting and the lists' elected hypotheses, as on the device
struct ClHostVote {
  double barc2;
  int min_consensus;
  std::vector<double> cstate;      // [lists][kClCState(d)]
  std::vector<int32_t> cint;       // [lists][kClCInts]
  std::vector<unsigned char> inl;  // [n_edges]
};
// vote and election over one stage (k_cl_vote, k_cl_elect): the votes are integers, so the order of the scoring is free
template <int D>
bool cl_host_vote_elect(const cora_ctx *c, size_t s, const double *oi, ClHostVote &hv, std::vector<int32_t> &ist) {
  constexpr int GS = kClCState(D), NE = D * D + 2 * D + 2;
  const ClTables &T = c->cl;
  bool finite = true;
  for (size_t list = static_cast<size_t>(T.stage_list0[s]); list < static_cast<size_t>(T.stage_list0[s + 1]); ++list) {
    const size_t last = static_cast<size_t>(T.list_chunk0[list + 1]) - 1, begin = static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]);
    const size_t len = static_cast<size_t>(T.chunk_begin[last] + T.chunk_len[last]) - begin;
    std::vector<double> ent(len * NE);  // P | q | l | kappa | tau
    for (size_t j = 0; j < len; ++j) {
      double *f = ent.data() + j * NE, res;
      cl_host_entry<D>(c, oi, begin + j, f, f + D * D, f + D * D + D, &res, f + D * D + 2 * D);
    }
    const double *q0 = ent.data() + D * D, *l0 = q0 + D;
    int32_t bv = -1, be = static_cast<int32_t>(len);
    for (size_t h = 0; h < len; ++h) {
      const double *fh = ent.data() + h * NE;
      double g[GS];
      cl_hypothesis<D>(q0, l0, fh, fh + D * D, fh + D * D + D, g);
      int32_t vote = 0;
      if (fh[D * D + 2 * D] > 0.0) {
        finite = odom_finite(g, GS) && finite;
        for (size_t j = 0; j < len; ++j) {
          const double *f = ent.data() + j * NE;
          vote += cl_agrees(cl_cost_at<D>(g, q0, l0, f, f + D * D, f + D * D + D, f[D * D + 2 * D], f[D * D + 2 * D + 1]), hv.barc2) ? 1 : 0;
        }
      }
      if (cl_better(vote, static_cast<int32_t>(h), bv, be)) {
        bv = vote;
        be = static_cast<int32_t>(h);
      }
    }
    const double *fh = ent.data() + static_cast<size_t>(be) * NE;
    double *g = hv.cstate.data() + list * GS;
    cl_hypothesis<D>(q0, l0, fh, fh + D * D, fh + D * D + D, g);
    hv.cint[list * kClCInts] = be;
    hv.cint[list * kClCInts + 1] = bv;
    ist[list * kSgInts] = bv < hv.min_consensus ? 5 : 0;
    ist[list * kSgInts + 1] = 0;
    finite = odom_finite(g, GS) && finite;
  }
  return finite;
}
// pass and fold of one mode over one stage, in the kernels' order; hv: over the inliers of the elected hypotheses only (an
// entry outside adds +0.0 terms), the folds with status 5 passed through
template <int D, int MODE>
bool cl_host_pass_fold(const cora_ctx *c, size_t s, const double *oi, std::vector<double> &partial, std::vector<double> &state, std::vector<int32_t> &ist,
                       ClHostVote *hv = nullptr) {
  constexpr int NS = MODE == 0 ? kClSums(D) : kClCostSums;
  const ClTables &T = c->cl;
  const size_t nc = std::max<size_t>(T.chunk_begin.size(), 1);
  const size_t l0 = static_cast<size_t>(T.stage_list0[s]), l1 = static_cast<size_t>(T.stage_list0[s + 1]);
  bool finite = true;
  double P0[D * D], q0[D], lm0[D], res0, kt0[2];
  for (size_t ch = static_cast<size_t>(T.list_chunk0[l0]); ch < static_cast<size_t>(T.list_chunk0[l1]); ++ch) {
    const size_t list = static_cast<size_t>(T.chunk_list[ch]);
    cl_host_entry<D>(c, oi, static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]), P0, q0, lm0, &res0, kt0);
    host_chunk_sums<NS>(T.chunk_len[ch], [&](int i, double *t) {
      double P[D * D], q[D], l[D], res, kt[2];
      cl_host_entry<D>(c, oi, static_cast<size_t>(T.chunk_begin[ch]) + i, P, q, l, &res, kt);
      if (hv) {
        const bool in = cl_agrees(cl_cost_at<D>(hv->cstate.data() + list * kClCState(D), q0, lm0, P, q, l, kt[0], kt[1]), hv->barc2);
        if constexpr (MODE == 0) hv->inl[static_cast<size_t>(T.ent_e[static_cast<size_t>(T.chunk_begin[ch]) + i])] = in ? 1 : 0;
        if (!in) return;
      }
      if constexpr (MODE == 0) {
        cl_terms<D>(q0, lm0, P, q, l, kt[0], kt[1], t);
      } else {
        t[0] = res;
        t[1] = cl_cost_at<D>(state.data() + list * kSgState(D), q0, lm0, P, q, l, kt[0], kt[1]);
      }
    }, partial.data(), nc, ch);
  }
  for (size_t list = l0; list < l1; ++list) {
    double S[NS];
    host_list_sums<NS>(partial.data(), nc, static_cast<size_t>(T.list_chunk0[list]), static_cast<size_t>(T.list_chunk0[list + 1]), S);
    cl_host_entry<D>(c, oi, static_cast<size_t>(T.chunk_begin[static_cast<size_t>(T.list_chunk0[list])]), P0, q0, lm0, &res0, kt0);
    finite = (hv ? cl_fold_robust<D, MODE>(S, state.data() + list * kSgState(D), ist.data() + list * kSgInts, q0, lm0)
                 : cl_fold<D, MODE>(S, state.data() + list * kSgState(D), ist.data() + list * kSgInts, q0, lm0)) &&
             finite;
  }
  return finite;
}
// the whole placement on the host, in the kernels' order: oi a d-column resident vector; state and ist as on the device
template <int D>
bool cl_host_run(const cora_ctx *c, double *oi, std::vector<double> &state, std::vector<int32_t> &ist, unsigned char *deg, int64_t *n_deg,
                 ClHostVote *hv = nullptr) {
  const ClTables &T = c->cl;
  const MeasurementTable &M = c->meas;
  bool finite = true;
  std::vector<double> partial(static_cast<size_t>(kClSums(D)) * std::max<size_t>(T.chunk_begin.size(), 1), 0.0);
  for (size_t s = 0; s + 1 < T.stage_list0.size(); ++s) {
    if (hv) finite = cl_host_vote_elect<D>(c, s, oi, *hv, ist) && finite;
    finite = cl_host_pass_fold<D, 0>(c, s, oi, partial, state, ist, hv) && finite;
    finite = cl_host_pass_fold<D, 1>(c, s, oi, partial, state, ist, hv) && finite;
    host_apply_stage<D>(c->odom, T, s, state, ist, oi);
  }
  return host_range_rows<D>(M, true, oi, deg, n_deg) && finite;
}
}  // extern "C++"

}  // namespace

int cora_set_closure_placement(cora_ctx *c, const unsigned char *chain_fixed, int min_closures) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  return install_tables(c, c->cl, [&](ClTables &T) { return cl_build(c, chain_fixed, min_closures, T); }, [&](ClTables &T) { return cl_upload(c, T); });
}

int cora_closure_placement_counts(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->cl.stage_list0.empty() ? 0 : static_cast<int64_t>(c->cl.stage_list0.size()) - 1;
  out[1] = static_cast<int64_t>(c->cl.ent_e.size());
  out[2] = static_cast<int64_t>(c->cl.chunk_begin.size());
  out[3] = c->cl.skipped + c->cl.unused;
  return CORA_OK;
}

int cora_closure_placement_order(const cora_ctx *c, int32_t *stage_ptr, int32_t *items) {
  if (!c || !stage_ptr || !items) return CORA_ERR_ARG;
  const ClTables &T = c->cl;
  std::copy(T.stage_list0.begin(), T.stage_list0.end(), stage_ptr);
  if (T.stage_list0.empty()) stage_ptr[0] = 0;
  std::copy(T.list_item.begin(), T.list_item.end(), items);
  return CORA_OK;
}

namespace {
// the consensus setting and the outputs of a robust call (cora_place_by_closures_robust_dev)
struct ClConsensus {
  double barc2;
  int min_consensus;
  int32_t *consensus, *list_len;
  unsigned char *inlier;
};
const char *cl_not_finite(const ClConsensus *rb) {  // the refusal of a call whose flag word is set
  return rb ? "a sum or a hypothesis of the closure placement is not finite" : "a sum of the closure placement is not finite";
}
int cl_consensus_check(cora_ctx *c, double barc2, int min_consensus) {
  if (!(barc2 > 0.0) || !std::isfinite(barc2)) return fail(c, CORA_ERR_ARG, "barc2 must be finite and positive");
  if (min_consensus < 1) return fail(c, CORA_ERR_ARG, "min_consensus must be at least 1");
  return CORA_OK;
}
// what a robust call returns beyond the plain call's: cint [lists][kClCInts], inl [n_edges] (2 where an edge is in no list)
void cl_robust_results(const cora_ctx *c, const std::vector<int32_t> &ist, const std::vector<int32_t> &cint, const std::vector<unsigned char> &inl,
                       const ClConsensus &rb, int64_t out[7]) {
  const ClTables &T = c->cl;
  const size_t nch = T.chain_init.size(), ne = static_cast<size_t>(c->meas.n_edges);
  out[5] = out[6] = 0;
  for (size_t ch = 0; ch < nch; ++ch) {
    const int32_t list = T.chain_list[ch];
    if (list >= 0 && ist[static_cast<size_t>(list) * kSgInts] == 5) ++out[5];
    if (rb.consensus) rb.consensus[ch] = list >= 0 ? cint[static_cast<size_t>(list) * kClCInts + 1] : 0;
    if (rb.list_len) {
      const size_t first = list >= 0 ? static_cast<size_t>(T.list_chunk0[static_cast<size_t>(list)]) : 0;
      const size_t last = list >= 0 ? static_cast<size_t>(T.list_chunk0[static_cast<size_t>(list) + 1]) - 1 : 0;
      rb.list_len[ch] = list >= 0 ? T.chunk_begin[last] + T.chunk_len[last] - T.chunk_begin[first] : 0;
    }
  }
  for (size_t e = 0; e < ne; ++e) out[6] += inl[e] == 0 ? 1 : 0;
  if (rb.inlier) std::copy(inl.begin(), inl.begin() + static_cast<std::ptrdiff_t>(ne), rb.inlier);
}
// the device-pointer forms: rb null, the plain placement (5 launches per stage); else the consensus vote in front of the
// masked passes (7 launches per stage)
int cl_place_dev(cora_ctx *c, double *dX, const ClConsensus *rb, int64_t *out, unsigned char *status, double *cost_start, double *cost_final,
                 int32_t *chosen, double *transforms, unsigned char *degenerate) {
  const MeasurementTable &M = c->meas;
  ClTables &T = c->cl;
  const int d = c->F.L.d;
  const size_t ns = T.stage_list0.size() - 1, nlist = T.list_item.size(), ne = static_cast<size_t>(M.n_edges);
  ClRobustArgs R;
  ClArgs &A = R.A;
  cl_fill_args(c, dX, A);
  if (rb) {
    R.barc2 = rb->barc2;
    R.min_consensus = rb->min_consensus;
    R.votes = T.d_votes;
    R.cstate = T.d_cstate;
    R.cint = T.d_cint;
    R.inlier = T.d_inlier;
  }
  wrote(c, dX);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  if (rb && ne > 0) HIP_TRY(c, hipMemsetAsync(T.d_inlier, 2, ne, c->stream));  // (an edge of no list)
  for (size_t s = 0; s < ns; ++s) {  // dependent: a stage reads the rows the stages before it wrote
    stage_args(T, s, A);
    if (rb) HIP_TRY(c, launch_closure_vote_elect(R, c->stream));
    A.mode = 0;
    HIP_TRY(c, rb ? launch_closure_robust_pass_fold(R, c->stream) : launch_closure_pass_fold(A, c->stream));
    A.mode = 1;
    HIP_TRY(c, rb ? launch_closure_robust_pass_fold(R, c->stream) : launch_closure_pass_fold(A, c->stream));
    HIP_TRY(c, launch_closure_apply(A, c->stream));
  }
  std::vector<double> state(nlist * kSgState(d));
  std::vector<int32_t> ist(nlist * kSgInts), cint(rb ? nlist * kClCInts : 0);
  std::vector<unsigned char> inl(rb ? ne : 0);
  int64_t n_deg = 0;
  const int rc = range_rows_step(c, dX, true, degenerate, cl_not_finite(rb), &n_deg, [&]() -> int {  // (after the chains' rows)
    if (const int e = read_back_state(c, state, T.d_state, ist, T.d_istate)) return e;
    if (rb && nlist > 0) HIP_TRY(c, hipMemcpyAsync(cint.data(), T.d_cint, cint.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (rb && ne > 0) HIP_TRY(c, hipMemcpyAsync(inl.data(), T.d_inlier, ne, hipMemcpyDeviceToHost, c->stream));
    return CORA_OK;
  });
  if (rc) return rc;
  cl_results(c, state, ist, n_deg, out, status, cost_start, cost_final, chosen, transforms);
  if (rb) cl_robust_results(c, ist, cint, inl, *rb, out);
  return CORA_OK;
}
}  // namespace

int cora_place_by_closures_dev(cora_ctx *c, double *dX, int64_t out[5], unsigned char *status, double *cost_start, double *cost_final,
                               int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = cl_args_check(c, dX, out))) return rc;
  return cl_place_dev(c, dX, nullptr, out, status, cost_start, cost_final, chosen, transforms, degenerate);
}

int cora_place_by_closures_robust_dev(cora_ctx *c, double *dX, double barc2, int min_consensus, int64_t out[7], unsigned char *status,
                                      double *cost_start, double *cost_final, int32_t *chosen, double *transforms, int32_t *consensus,
                                      int32_t *list_len, unsigned char *inlier) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = cl_args_check(c, dX, out)) || (rc = cl_consensus_check(c, barc2, min_consensus))) return rc;
  const ClConsensus rb{barc2, min_consensus, consensus, list_len, inlier};
  return cl_place_dev(c, dX, &rb, out, status, cost_start, cost_final, chosen, transforms, nullptr);
}

namespace {
// the host-pointer forms (with_uploaded_x)
int cl_place_host_ptr(cora_ctx *c, double *X, int ldx, const ClConsensus *rb, int64_t *out, unsigned char *status, double *cost_start,
                      double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  return with_uploaded_x(c, X, ldx, [&](double *dX) {
    return cl_place_dev(c, dX, rb, out, status, cost_start, cost_final, chosen, transforms, degenerate);
  });
}
// the host mirrors (with_host_x), every hypothesis too through the function of kernels.h the kernels call
int cl_place_mirror(cora_ctx *c, double *X, int ldx, const ClConsensus *rb, int64_t *out, unsigned char *status, double *cost_start,
                    double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  const int d = c->F.L.d;
  const size_t nlist = c->cl.list_item.size();
  std::vector<double> state(nlist * kSgState(d), 0.0);
  std::vector<int32_t> ist(nlist * kSgInts, 0);
  ClHostVote hv;
  if (rb) {
    hv.barc2 = rb->barc2;
    hv.min_consensus = rb->min_consensus;
    hv.cstate.assign(nlist * kClCState(d), 0.0);
    hv.cint.assign(nlist * kClCInts, 0);
    hv.inl.assign(static_cast<size_t>(c->meas.n_edges), 2);
  }
  int64_t n_deg = 0;
  const int rc = with_host_x(c, X, ldx, cl_not_finite(rb), [&](auto D, double *oi) {
    return cl_host_run<D()>(c, oi, state, ist, degenerate, &n_deg, rb ? &hv : nullptr);
  });
  if (rc) return rc;
  cl_results(c, state, ist, n_deg, out, status, cost_start, cost_final, chosen, transforms);
  if (rb) cl_robust_results(c, ist, hv.cint, hv.inl, *rb, out);
  return CORA_OK;
}
}  // namespace

int cora_place_by_closures(cora_ctx *c, double *X, int ldx, int64_t out[5], unsigned char *status, double *cost_start, double *cost_final,
                           int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = cl_args_check(c, X, out))) return rc;
  return cl_place_host_ptr(c, X, ldx, nullptr, out, status, cost_start, cost_final, chosen, transforms, degenerate);
}

int cora_place_by_closures_robust(cora_ctx *c, double *X, int ldx, double barc2, int min_consensus, int64_t out[7], unsigned char *status,
                                  double *cost_start, double *cost_final, int32_t *chosen, double *transforms, int32_t *consensus,
                                  int32_t *list_len, unsigned char *inlier) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if ((rc = cl_args_check(c, X, out)) || (rc = cl_consensus_check(c, barc2, min_consensus))) return rc;
  const ClConsensus rb{barc2, min_consensus, consensus, list_len, inlier};
  return cl_place_host_ptr(c, X, ldx, &rb, out, status, cost_start, cost_final, chosen, transforms, nullptr);
}

int cora_debug_place_by_closures_host(cora_ctx *c, double *X, int ldx, int64_t out[5], unsigned char *status, double *cost_start,
                                      double *cost_final, int32_t *chosen, double *transforms, unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  if ((rc = cl_args_check(c, X, out))) return rc;
  return cl_place_mirror(c, X, ldx, nullptr, out, status, cost_start, cost_final, chosen, transforms, degenerate);
}

int cora_debug_place_by_closures_robust_host(cora_ctx *c, double *X, int ldx, double barc2, int min_consensus, int64_t out[7],
                                             unsigned char *status, double *cost_start, double *cost_final, int32_t *chosen, double *transforms,
                                             int32_t *consensus, int32_t *list_len, unsigned char *inlier) {
  if (!c) return CORA_ERR_ARG;
  int rc = cl_check(c);
  if (rc) return rc;
  if ((rc = cl_args_check(c, X, out)) || (rc = cl_consensus_check(c, barc2, min_consensus))) return rc;
  const ClConsensus rb{barc2, min_consensus, consensus, list_len, inlier};
  return cl_place_mirror(c, X, ldx, &rb, out, status, cost_start, cost_final, chosen, transforms, nullptr);
}
