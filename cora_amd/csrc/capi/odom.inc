// Part of capi.hip (one translation unit; included there, in this order).  odometry initialisation (a segmented scan of SE(d) over the chains of the measurement table): chain tables, device-pointer form, host-pointer form, host mirror.  Reads the measurement table and the row maps; writes nothing the handle computes with.  What it shares with the other initialisers -- the range-row step, the host-pointer and host-mirror wrappers, installing tables, chunk cutting, the mirror's sums -- is in capi/init_common.inc.

namespace {

int odom_check(cora_ctx *c) {
  if (c->F.L.world > 1) return fail(c, CORA_ERR_ARG, "the odometry initialisation is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  return CORA_OK;
}

// validates the chains against the measurement table and translates them to position tables (host part of T only)
int odom_build(cora_ctx *c, int64_t n_chains, const int64_t *chain_ptr, const int32_t *chain_edges, OdomTables &T) {
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  const int64_t ne = M.n_edges;
  if (const int rc = compare_pose_table(c)) return rc;
  const int32_t *rot_of = c->cmp_rows.data(), *trn_of = rot_of + L.n;
  auto chain = [](int64_t ch) { return "chain " + std::to_string(ch); };
  if (n_chains > 0 && chain_ptr[0] != 0) return fail(c, CORA_ERR_ARG, "chain_ptr[0] must be 0");
  for (int64_t ch = 0; ch < n_chains; ++ch)
    if (chain_ptr[ch + 1] <= chain_ptr[ch]) return fail(c, CORA_ERR_ARG, chain(ch) + " is empty (chain_ptr must increase)");
  const int64_t total = n_chains > 0 ? chain_ptr[n_chains] : 0;
  if (total + n_chains > L.n) return fail(c, CORA_ERR_ARG, "the chains have more positions than the problem has poses: a pose would be written twice");
  T.n_chains = n_chains;
  T.P = total + n_chains;
  for (std::vector<int32_t> *v : {&T.pos_edge, &T.pos_chain, &T.pos_rot, &T.pos_trn}) v->assign(static_cast<size_t>(T.P), 0);
  std::vector<unsigned char> written(static_cast<size_t>(L.rows), 0);
  auto write = [&](int64_t pos, int32_t edge, int64_t ch, int32_t rot, int32_t trn) {
    T.pos_edge[static_cast<size_t>(pos)] = edge;
    T.pos_chain[static_cast<size_t>(pos)] = static_cast<int32_t>(ch);
    T.pos_rot[static_cast<size_t>(pos)] = rot;
    T.pos_trn[static_cast<size_t>(pos)] = trn;
    const bool twice = written[static_cast<size_t>(rot)] || written[static_cast<size_t>(trn)];
    written[static_cast<size_t>(rot)] = written[static_cast<size_t>(trn)] = 1;
    return !twice;
  };
  int64_t pos = 0;
  for (int64_t ch = 0; ch < n_chains; ++ch)
    for (int64_t k = chain_ptr[ch]; k < chain_ptr[ch + 1]; ++k) {
      const int64_t e = chain_edges[k];
      const std::string at = "edge " + std::to_string(e) + " (entry " + std::to_string(k - chain_ptr[ch]) + " of " + chain(ch) + ")";
      if (e < 0 || e >= ne) return fail(c, CORA_ERR_ARG, at + " lies outside the table of " + std::to_string(ne) + " edges");
      const int32_t ra = M.edge_rows[static_cast<size_t>(e)], rb = M.edge_rows[static_cast<size_t>(ne + e)];
      const int32_t ta = M.edge_rows[static_cast<size_t>(2 * ne + e)], tb = M.edge_rows[static_cast<size_t>(3 * ne + e)];
      if (rb < 0) return fail(c, CORA_ERR_ARG, at + " has no rotation part");
      if (k == chain_ptr[ch]) {
        if (!write(pos++, -1, ch, ra, ta)) return fail(c, CORA_ERR_ARG, "the head of " + chain(ch) + " is a pose another position writes");
      } else if (T.pos_rot[static_cast<size_t>(pos - 1)] != ra || T.pos_trn[static_cast<size_t>(pos - 1)] != ta) {
        return fail(c, CORA_ERR_ARG, at + " does not start at the pose the edge before it ends at");
      }
      if (!write(pos++, static_cast<int32_t>(e), ch, rb, tb)) return fail(c, CORA_ERR_ARG, at + " ends at a pose another position writes");
    }
  // what no position writes: the free poses; the landmarks' rows
  for (int i = 0; i < L.n; ++i) {
    const bool w_rot = written[static_cast<size_t>(rot_of[i])] != 0, w_trn = written[static_cast<size_t>(trn_of[i])] != 0;
    if (w_rot != w_trn) return fail(c, CORA_ERR_ARG, "an edge of the chains pairs the rotation rows of pose " + std::to_string(i) + " with another pose's translation row");
    if (w_rot) continue;
    T.free_rot.push_back(rot_of[i]);
    T.free_trn.push_back(trn_of[i]);
  }
  T.lm_row.assign(trn_of + L.n, trn_of + L.nt);
  if (const int rc = range_rows_unique(c)) return rc;
  T.built = true;
  return CORA_OK;
}

size_t odom_stage_doubles(const cora_ctx *c, const OdomTables &T) {
  return static_cast<size_t>(T.n_chains + (c->F.L.nt - c->F.L.n)) * c->F.L.d;
}

// the device side of freshly built tables (T's device pointers are null); on failure T owns what was allocated
int odom_upload(cora_ctx *c, OdomTables &T) {
  HIP_TRY(c, upload_joined(&T.d_idx, {&T.pos_edge, &T.pos_chain, &T.pos_rot, &T.pos_trn, &T.free_rot, &T.free_trn, &T.lm_row}));
  const size_t work = 2 * static_cast<size_t>(kOdomFields(c->F.L.d)) * std::max(odom_tiles(T.P), 1);
  HIP_TRY(c, alloc_device(&T.d_work, work * sizeof(double)));
  const size_t stage = std::max<size_t>(odom_stage_doubles(c, T), 1) * sizeof(double);
  HIP_TRY(c, alloc_device(&T.d_stage, stage));
  HIP_TRY(c, alloc_pinned(&T.h_stage, stage));
  return CORA_OK;
}

// builds, uploads and installs; a failure leaves the handle's tables as they were
int odom_install(cora_ctx *c, int64_t n_chains, const int64_t *chain_ptr, const int32_t *chain_edges) {
  const int rc = install_tables(c, c->odom, [&](OdomTables &T) { return odom_build(c, n_chains, chain_ptr, chain_edges, T); },
                                [&](OdomTables &T) { return odom_upload(c, T); });
  if (rc) return rc;
  free_tables(c->pl);  // (the chain placement's stages name the positions of the chains they were built from)
  free_tables(c->sg);  // (so do the sighting placement's lists)
  free_tables(c->cl);  // (and the closure placement's)
  return CORA_OK;
}

int odom_inputs_check(cora_ctx *c, const double *starts, const double *landmarks) {
  const OdomTables &T = c->odom;
  const size_t ns = static_cast<size_t>(T.n_chains) * c->F.L.d, nl = static_cast<size_t>(c->F.L.nt - c->F.L.n) * c->F.L.d;
  if (ns > 0 && !starts) return fail(c, CORA_ERR_ARG, "null pointer");
  if (!all_finite(starts, ns)) return fail(c, CORA_ERR_ARG, "a start of a chain is not finite");
  if (landmarks && !all_finite(landmarks, nl)) return fail(c, CORA_ERR_ARG, "a landmark is not finite");
  return CORA_OK;
}

extern "C++" {  // (templates: this file is included inside extern "C")
template <int D>
void odom_host_wave_scan(OdomEl<D> *el) {  // kWave elements; descending, so that el[i - off] is still the step's input
  for (int off = 1; off < kWave; off <<= 1)
    for (int i = kWave - 1; i >= off; --i) odom_compose<D>(el[i - off], el[i]);
}
template <int D>
void odom_host_tile_scan(OdomEl<D> *el) {  // kOdomTile elements
  constexpr int NW = kOdomTile / kWave;
  OdomEl<D> tot[NW];
  for (int w = 0; w < NW; ++w) {
    odom_host_wave_scan<D>(el + w * kWave);
    tot[w] = el[w * kWave + kWave - 1];
  }
  for (int w = 1; w < NW; ++w) {
    OdomEl<D> acc = tot[0];
    for (int j = 1; j < w; ++j) {
      OdomEl<D> nxt = tot[j];
      odom_compose<D>(acc, nxt);
      acc = nxt;
    }
    for (int l = 0; l < kWave; ++l) odom_compose<D>(acc, el[w * kWave + l]);
  }
}
// the whole initialisation on the host, in the kernels' order: oi a d-column resident vector (zeroed), deg [n_ranges]
template <int D>
bool odom_host_run(const cora_ctx *c, const double *starts, const double *landmarks, double *oi, unsigned char *deg, int64_t *n_deg) {
  const OdomTables &T = c->odom;
  const MeasurementTable &M = c->meas;
  const int64_t P = T.P, ne = M.n_edges;
  const int ntiles = odom_tiles(P);
  bool finite = true;
  std::vector<OdomEl<D>> el(static_cast<size_t>(ntiles) * kOdomTile), carry(static_cast<size_t>(ntiles));
  for (size_t pos = 0; pos < el.size(); ++pos) {
    OdomEl<D> &e = el[pos];
    odom_head<D>(e);
    if (static_cast<int64_t>(pos) >= P) continue;
    const int32_t ed = T.pos_edge[pos];
    if (ed < 0) {
      for (int cc = 0; cc < D; ++cc) e.v[D * D + cc] = starts[static_cast<size_t>(T.pos_chain[pos]) * D + cc];
    } else {
      for (int f = 0; f < D * D + D; ++f) e.v[f] = M.edge_data[static_cast<size_t>(f) * ne + ed];
      e.flag = 0;
    }
  }
  for (int t = 0; t < ntiles; ++t) odom_host_tile_scan<D>(el.data() + static_cast<size_t>(t) * kOdomTile);
  OdomEl<D> before;
  odom_head<D>(before);
  for (int base = 0; base < ntiles; base += kOdomSweep) {
    OdomEl<D> e[kOdomSweep];
    for (int l = 0; l < kOdomSweep; ++l) {
      odom_head<D>(e[l]);
      if (base + l < ntiles) e[l] = el[static_cast<size_t>(base + l) * kOdomTile + kOdomTile - 1];
    }
    odom_host_wave_scan<D>(e);
    for (int l = 0; l < kOdomSweep; ++l) {
      if (base > 0) odom_compose<D>(before, e[l]);
      if (base + l < ntiles) carry[static_cast<size_t>(base + l)] = e[l];
    }
    before = e[kOdomSweep - 1];
  }
  for (int64_t pos = 0; pos < P; ++pos) {
    OdomEl<D> &e = el[static_cast<size_t>(pos)];
    if (pos >= kOdomTile) odom_compose<D>(carry[static_cast<size_t>(pos / kOdomTile - 1)], e);
    double *rot = oi + static_cast<size_t>(T.pos_rot[static_cast<size_t>(pos)]) * D, *trn = oi + static_cast<size_t>(T.pos_trn[static_cast<size_t>(pos)]) * D;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) rot[a * D + b] = e.v[b * D + a];
    for (int cc = 0; cc < D; ++cc) trn[cc] = e.v[D * D + cc];
    finite = odom_finite(e.v, D * D + D) && finite;
  }
  for (size_t u = 0; u < T.free_rot.size(); ++u) {
    double *rot = oi + static_cast<size_t>(T.free_rot[u]) * D, *trn = oi + static_cast<size_t>(T.free_trn[u]) * D;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) rot[a * D + b] = a == b ? 1.0 : 0.0;
    for (int cc = 0; cc < D; ++cc) trn[cc] = 0.0;
  }
  for (size_t l = 0; l < T.lm_row.size(); ++l)
    for (int cc = 0; cc < D; ++cc) oi[static_cast<size_t>(T.lm_row[l]) * D + cc] = landmarks ? landmarks[l * D + cc] : 0.0;
  return host_range_rows<D>(M, false, oi, deg, n_deg) && finite;
}
}  // extern "C++"

}  // namespace

int cora_set_odometry_chains(cora_ctx *c, int64_t n_chains, const int64_t *chain_ptr, const int32_t *chain_edges) {
  if (!c) return CORA_ERR_ARG;
  if (const int rc = odom_check(c)) return rc;
  if (n_chains < 0) return fail(c, CORA_ERR_ARG, "negative chain count");
  if (n_chains > 0 && (!chain_ptr || !chain_edges)) return fail(c, CORA_ERR_ARG, "null pointer");
  return odom_install(c, n_chains, chain_ptr, chain_edges);
}

int cora_odometry_chains_count(const cora_ctx *c, int64_t out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->odom.n_chains;
  out[1] = c->odom.P;
  return CORA_OK;
}

int cora_odometry_scan_shape(const cora_ctx *c, int64_t out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = kOdomTile;
  out[1] = kOdomSweep;
  return CORA_OK;
}

int cora_odometry_init_dev(cora_ctx *c, const double *starts, const double *landmarks, double *dOut, int64_t out[2],
                           unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = odom_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!dOut || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  if (!c->odom.built && (rc = odom_install(c, 0, nullptr, nullptr))) return rc;  // (no chains: every pose is free)
  if ((rc = odom_inputs_check(c, starts, landmarks))) return rc;
  const Layout &L = c->F.L;
  const MeasurementTable &M = c->meas;
  OdomTables &T = c->odom;
  const int d = L.d;
  const size_t ns = static_cast<size_t>(T.n_chains) * d, nl = static_cast<size_t>(L.nt - L.n) * d;
  if (ns) std::copy(starts, starts + ns, T.h_stage);
  if (landmarks && nl) std::copy(landmarks, landmarks + nl, T.h_stage + ns);
  if (ns + (landmarks ? nl : 0) > 0)
    HIP_TRY(c, hipMemcpyAsync(T.d_stage, T.h_stage, (ns + (landmarks ? nl : 0)) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  OdomArgs A;
  A.d = d;
  A.P = T.P;
  A.ntiles = odom_tiles(T.P);
  A.n_edges = M.n_edges;
  A.pos_edge = T.d_idx;
  A.pos_chain = A.pos_edge + T.P;
  A.pos_rot = A.pos_chain + T.P;
  A.pos_trn = A.pos_rot + T.P;
  A.edge_data = M.d_edge_data;
  A.starts = T.d_stage;
  A.totals = T.d_work;
  A.carry = T.d_work + static_cast<size_t>(kOdomFields(d)) * std::max(A.ntiles, 1);
  A.out = dOut;
  A.flag = c->d_flag;
  OdomFillArgs Fl;
  Fl.d = d;
  Fl.n_free = static_cast<int64_t>(T.free_rot.size());
  Fl.n_lm = static_cast<int64_t>(T.lm_row.size());
  Fl.free_rot = A.pos_trn + T.P;
  Fl.free_trn = Fl.free_rot + Fl.n_free;
  Fl.lm_row = Fl.free_trn + Fl.n_free;
  Fl.lm = landmarks ? T.d_stage + ns : nullptr;
  Fl.out = dOut;
  wrote(c, dOut);
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  HIP_TRY(c, hipMemsetAsync(dOut, 0, vec_bytes(c, ld_for(d)), c->stream));
  HIP_TRY(c, launch_odom_fill(Fl, c->stream));
  HIP_TRY(c, launch_odom_scan(A, c->stream));
  // (after both: it reads the translation rows they wrote)
  if ((rc = range_rows_step(c, dOut, false, degenerate, "a product of the odometry initialisation is not finite", &out[1], []() -> int { return CORA_OK; })))
    return rc;
  out[0] = T.P;
  return CORA_OK;
}

int cora_odometry_init(cora_ctx *c, const double *starts, const double *landmarks, double *Out, int ldo, int64_t out[2],
                       unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = odom_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (!Out || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  if (ldo < c->F.L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = c->F.L.d;
  double *dOut;
  if ((rc = compare_vec(c, 3, ld_for(d), &dOut))) return rc;
  rc = cora_odometry_init_dev(c, starts, landmarks, dOut, out, degenerate);
  if (rc == CORA_OK) rc = download_impl(c, dOut, d, Out, ldo);
  // the vector of this form is not kept: a caller that stays resident uses cora_odometry_init_dev
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 3, 4, 0);
  return rc;
}

int cora_odometry_set_range_rows_dev(cora_ctx *c, int64_t m, const int32_t *range_idx, const double *dirs, double *dOut) {
  if (!c) return CORA_ERR_ARG;
  int rc = odom_check(c);
  if (rc) return rc;
  NEED_DEVICE(c);
  if (m < 0) return fail(c, CORA_ERR_ARG, "negative count");
  if (m == 0) return CORA_OK;
  if (!range_idx || !dirs || !dOut) return fail(c, CORA_ERR_ARG, "null pointer");
  const MeasurementTable &M = c->meas;
  const int d = c->F.L.d;
  std::vector<int32_t> rows(static_cast<size_t>(m));
  std::vector<double> unit(static_cast<size_t>(m) * d);
  const double zero[3] = {0.0, 0.0, 0.0};
  for (int64_t i = 0; i < m; ++i) {
    if (range_idx[i] < 0 || range_idx[i] >= M.n_ranges) return fail(c, CORA_ERR_ARG, "range measurement " + std::to_string(range_idx[i]) + " lies outside the table");
    rows[static_cast<size_t>(i)] = M.range_rows[static_cast<size_t>(range_idx[i])];
    const double *dir = dirs + static_cast<size_t>(i) * d;
    double *u = unit.data() + static_cast<size_t>(i) * d;
    if (!all_finite(dir, static_cast<size_t>(d))) return fail(c, CORA_ERR_ARG, "direction " + std::to_string(i) + " is not finite");
    const bool degenerate = for_d(d, [&](auto D) { return odom_range_row<D()>(zero, dir, u); });
    if (degenerate || !all_finite(u, static_cast<size_t>(d))) return fail(c, CORA_ERR_ARG, "direction " + std::to_string(i) + " has no usable length");
  }
  // the rare path: the scatter of the exchange (k_move_rows) moves the rows; its two arrays live for this call only
  int32_t *d_rows = nullptr;
  double *d_unit = nullptr;
  hipError_t e = to_device(&d_rows, rows);
  if (e == hipSuccess) e = to_device(&d_unit, unit);
  wrote(c, dOut);
  if (e == hipSuccess) e = launch_move_rows(1, m, ld_for(d), d_rows, d_unit, dOut, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  free_device(d_rows, d_unit);
  HIP_TRY(c, e);
  return CORA_OK;
}

// The same on the host through the translated tables, every composition in the kernels' bracket order through
// odom_compose (kernels.h): the output has the device's bits.  Works on a plan-only handle.
int cora_debug_odometry_init_host(cora_ctx *c, const double *starts, const double *landmarks, double *Out, int ldo, int64_t out[2],
                                  unsigned char *degenerate) {
  if (!c) return CORA_ERR_ARG;
  int rc = odom_check(c);
  if (rc) return rc;
  if (!Out || !out) return fail(c, CORA_ERR_ARG, "null pointer");
  const HostFormat &F = c->F;
  const Layout &L = F.L;
  if (ldo < L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  if (!c->odom.built && (rc = odom_install(c, 0, nullptr, nullptr))) return rc;
  if ((rc = odom_inputs_check(c, starts, landmarks))) return rc;
  const int d = L.d;
  std::vector<double> oi(static_cast<size_t>(L.rows) * d, 0.0);
  int64_t n_deg = 0;
  const bool finite = for_d(d, [&](auto D) { return odom_host_run<D()>(c, starts, landmarks, oi.data(), degenerate, &n_deg); });
  if (!finite) return fail(c, CORA_ERR_NAN, "a product of the odometry initialisation is not finite");
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < L.N; ++i) Out[static_cast<size_t>(cc) * ldo + i] = oi[static_cast<size_t>(F.api2int[i]) * d + cc];
  out[0] = c->odom.P;
  out[1] = n_deg;
  return CORA_OK;
}
