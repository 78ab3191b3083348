// Part of capi.hip (one translation unit; included there, in this order).  what the initialisers that follow share (odometry, multilateration, chain placement, placement from sightings and from closures): the range-row step their calls end in, the host-pointer and the host-mirror form of a call, installing tables on the handle, the pieces of their table builders, and the mirror's chunk and list sums in the kernels' bracket order (chunk_sums and list_sums, kernels/common.inc).  Each feature keeps only what is its own: the ordering rule of its builder, its terms, its folds, its results.

namespace {
extern "C++" {  // (templates and C++ types: this file is included inside extern "C")

// ---- the range-row step -------------------------------------------------------------------------------------------------
// The step of the odometry initialisation (launch_odom_ranges), its rules unchanged: range row m = the direction of (second
// row) - (first row) of the table it runs over.  The odometry initialisation runs it over the measurement table (the direction
// of x_t(b) - x_t(a)); the four placements over the table with a and b EXCHANGED: the direction of x_t(a) - x_t(b), the one at
// which the residual |x_t(b) - x_t(a) + r x_rho|^2 is (|x_t(b) - x_t(a)| - r)^2.

// (a range row two measurements name would be written by two threads of the step)
int range_rows_unique(cora_ctx *c) {
  const MeasurementTable &M = c->meas;
  std::vector<unsigned char> written(static_cast<size_t>(c->F.L.rows), 0);
  for (int64_t m = 0; m < M.n_ranges; ++m) {
    unsigned char &w = written[static_cast<size_t>(M.range_rows[static_cast<size_t>(m)])];
    if (w) return fail(c, CORA_ERR_ARG, "range measurement " + std::to_string(m) + " names a range row an earlier one names");
    w = 1;
  }
  return CORA_OK;
}

// The end of every device-pointer form, after the launches that wrote the translation rows of dX: the step, the read-back of
// its count into *n_deg, of the flag word, of what read_back enqueues (the feature's own state) and of the bytes (degenerate
// non-null), the wait, and the refusal of a call whose flag word is set.  The handle's arrays of the step are made at the
// first call (to_device never makes an empty buffer: n_ranges == 0 is served too, without a launch over the ranges).
template <class ReadBack>
int range_rows_step(cora_ctx *c, double *dX, bool exchanged, unsigned char *degenerate, const char *not_finite, int64_t *n_deg,
                    ReadBack read_back) {
  const MeasurementTable &M = c->meas;
  RangeRowStep &S = c->range_step;
  const size_t nr = static_cast<size_t>(M.n_ranges);
  const int nb = odom_range_blocks(M.n_ranges);
  if (const int rc = ensure_red(c, static_cast<size_t>(nb) / 2 + 4)) return rc;
  if (!S.d_deg) HIP_TRY(c, alloc_device(&S.d_deg, std::max<size_t>(nr, 1)));
  if (exchanged && !S.d_exchanged) {
    std::vector<int32_t> rows(M.range_rows);
    std::swap_ranges(rows.begin() + static_cast<std::ptrdiff_t>(nr), rows.begin() + static_cast<std::ptrdiff_t>(2 * nr), rows.begin() + static_cast<std::ptrdiff_t>(2 * nr));
    HIP_TRY(c, to_device(&S.d_exchanged, rows));
  }
  OdomFillArgs Fl;
  Fl.d = c->F.L.d;
  Fl.n_ranges = M.n_ranges;
  Fl.range_rows = exchanged ? S.d_exchanged : M.d_range_rows;
  Fl.deg = S.d_deg;
  Fl.partial = reinterpret_cast<int *>(c->d_red.p);
  Fl.words = Fl.partial + nb;
  Fl.flag = c->d_flag;
  Fl.out = dX;
  HIP_TRY(c, launch_odom_ranges(Fl, c->stream));
  int words[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(words, Fl.words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (const int rc = read_back()) return rc;
  if (degenerate && nr > 0) HIP_TRY(c, hipMemcpyAsync(degenerate, S.d_deg, nr, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_flag) return fail(c, CORA_ERR_NAN, not_finite);
  *n_deg = words[0];
  return CORA_OK;
}

// the read-back of a feature's state arrays ([items][..] doubles and ints), for range_rows_step
int read_back_state(cora_ctx *c, std::vector<double> &state, const double *d_state, std::vector<int32_t> &ist, const int32_t *d_istate) {
  if (state.empty()) return CORA_OK;
  HIP_TRY(c, hipMemcpyAsync(state.data(), d_state, state.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(ist.data(), d_istate, ist.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  return CORA_OK;
}

// the step on the host, in the kernel's order: oi a d-column resident vector; false where a row is not finite
template <int D>
bool host_range_rows(const MeasurementTable &M, bool exchanged, double *oi, unsigned char *deg, int64_t *n_deg) {
  const int64_t nr = M.n_ranges;
  bool finite = true;
  int64_t count = 0;
  for (int64_t m = 0; m < nr; ++m) {
    const size_t rr = static_cast<size_t>(M.range_rows[static_cast<size_t>(m)]), ta = static_cast<size_t>(M.range_rows[static_cast<size_t>(nr + m)]),
                 tb = static_cast<size_t>(M.range_rows[static_cast<size_t>(2 * nr + m)]);
    double row[D];
    const bool degenerate = exchanged ? odom_range_row<D>(oi + tb * D, oi + ta * D, row) : odom_range_row<D>(oi + ta * D, oi + tb * D, row);
    std::copy(row, row + D, oi + rr * D);
    if (deg) deg[m] = degenerate ? 1 : 0;
    count += degenerate ? 1 : 0;
    finite = odom_finite(row, D) && finite;
  }
  *n_deg = count;
  return finite;
}

// ---- the forms of a call ---------------------------------------------------------------------------------------------------
// The host-pointer form: upload of X (N x d, ldx) into a vector of the call, dev_form(dX), download.  The vector is not kept: a
// caller that stays resident uses the device-pointer form.
template <class DevForm>
int with_uploaded_x(cora_ctx *c, double *X, int ldx, DevForm dev_form) {
  if (ldx < c->F.L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = c->F.L.d;
  double *dX;
  int rc;
  if ((rc = compare_vec(c, 3, ld_for(d), &dX))) return rc;
  rc = upload_impl(c, X, ldx, d, dX);
  if (rc == CORA_OK) rc = dev_form(dX);
  if (rc == CORA_OK) rc = download_impl(c, dX, d, X, ldx);
  (void)hipStreamSynchronize(c->stream);
  compare_release(c, 3, 4, 0);
  return rc;
}

// The host mirror: X gathered into a d-column vector in the internal order, host_run(D as an integral_constant, oi) -- the
// feature's host_run<2> or host_run<3>, false where a value is not finite -- and the vector scattered back.  Through the
// translated tables, every sum in the kernels' bracket order and every term and solve through the functions of kernels.h the
// kernels call: the output has the device's bits.  Works on a plan-only handle.
template <class HostRun>
int with_host_x(cora_ctx *c, double *X, int ldx, const char *not_finite, HostRun host_run) {
  const HostFormat &F = c->F;
  const Layout &L = F.L;
  if (ldx < L.N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  const int d = L.d;
  std::vector<double> oi(static_cast<size_t>(L.rows) * d, 0.0);
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < L.N; ++i) oi[static_cast<size_t>(F.api2int[i]) * d + cc] = X[static_cast<size_t>(cc) * ldx + i];
  const bool finite = for_d(d, [&](auto D) { return host_run(D, oi.data()); });
  if (!finite) return fail(c, CORA_ERR_NAN, not_finite);
  for (int cc = 0; cc < d; ++cc)
    for (int64_t i = 0; i < L.N; ++i) X[static_cast<size_t>(cc) * ldx + i] = oi[static_cast<size_t>(F.api2int[i]) * d + cc];
  return CORA_OK;
}

// ---- tables ---------------------------------------------------------------------------------------------------------------
// build(T) makes the host part of fresh tables, upload(T) their device side (T's device pointers are null; on failure T owns
// what was allocated); then they take the place of the handle's.  A failure leaves the handle's tables as they were.
template <class T, class Build, class Upload>
int install_tables(cora_ctx *c, T &installed, Build build, Upload upload) {
  T fresh;
  int rc = build(fresh);
  if (rc) return rc;
  if (c->has_device) {
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, CORA_ERR_HIP, "hipSetDevice failed");
    if ((rc = upload(fresh))) {
      fresh.release();
      return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    installed.release();
  }
  installed = std::move(fresh);
  return CORA_OK;
}

// the stage s of the tables T in the kernels' arguments (SgArgs, ClArgs): its lists, their chunks, its positions
template <class Tables, class Args>
void stage_args(const Tables &T, size_t s, Args &A) {
  A.list0 = T.stage_list0[s];
  A.n_lists = T.stage_list0[s + 1] - A.list0;
  A.chunk0 = T.list_chunk0[static_cast<size_t>(A.list0)];
  A.n_chunks = T.list_chunk0[static_cast<size_t>(T.stage_list0[s + 1])] - A.chunk0;
  A.apply0 = T.stage_apply0[s];
  A.n_apply = T.stage_apply0[s + 1] - A.apply0;
}

// k_sg_apply on the host: the positions of stage s of the tables T under their lists' motions, where chosen > 0
template <int D, class Tables>
void host_apply_stage(const OdomTables &O, const Tables &T, size_t s, const std::vector<double> &state, const std::vector<int32_t> &ist, double *oi) {
  for (int32_t i = T.stage_apply0[s]; i < T.stage_apply0[s + 1]; ++i) {
    const size_t list = static_cast<size_t>(T.apply_list[static_cast<size_t>(i)]), pos = static_cast<size_t>(T.apply_pos[static_cast<size_t>(i)]);
    if (ist[list * kSgInts + 1] <= 0) continue;
    pl_apply<D>(state.data() + list * kSgState(D), oi + static_cast<size_t>(O.pos_rot[pos]) * D, oi + static_cast<size_t>(O.pos_trn[pos]) * D);
  }
}

// ---- the mirror's sums ------------------------------------------------------------------------------------------------------
// the butterfly of a wavefront as the tree it is: v[0] = ((v0 + v1) + (v2 + v3)) + ..
inline double host_wave_sum(double *v) {
  for (int off = 1; off < kWave; off <<= 1)
    for (int i = 0; i < kWave; i += 2 * off) v[i] = v[i] + v[i + off];
  return v[0];
}
// chunk_sums (kernels/common.inc) of one chunk of len entries: terms(i, t) writes the NS terms of entry i into t, which holds
// +0.0 -- what the lanes beyond len, and an entry that writes nothing, add; the sums go to partial[k * stride + chunk]
template <int NS, class Terms>
void host_chunk_sums(int len, Terms terms, double *partial, size_t stride, size_t chunk) {
  double wave[kSumChunk / kWave][NS];
  for (int w = 0; w < kSumChunk / kWave; ++w) {
    double term[kWave][NS];
    for (int lane = 0; lane < kWave; ++lane) {
      const int i = w * kWave + lane;
      for (int k = 0; k < NS; ++k) term[lane][k] = 0.0;
      if (i < len) terms(i, term[lane]);
    }
    for (int k = 0; k < NS; ++k) {
      double v[kWave];
      for (int lane = 0; lane < kWave; ++lane) v[lane] = term[lane][k];
      wave[w][k] = host_wave_sum(v);
    }
  }
  for (int k = 0; k < NS; ++k) {
    double v = wave[0][k];
    for (int w = 1; w < kSumChunk / kWave; ++w) v = v + wave[w][k];
    partial[static_cast<size_t>(k) * stride + chunk] = v;
  }
}
// list_sums (kernels/common.inc) of the chunks [c0, c1): lane j takes 0.0 + chunk (c0 + j) + chunk (c0 + j + 64) + .., then the butterfly
template <int NS>
void host_list_sums(const double *partial, size_t stride, size_t c0, size_t c1, double *S) {
  for (int k = 0; k < NS; ++k) {
    double v[kWave];
    for (int lane = 0; lane < kWave; ++lane) {
      v[lane] = 0.0;
      for (size_t ch = c0 + static_cast<size_t>(lane); ch < c1; ch += kWave) v[lane] = v[lane] + partial[static_cast<size_t>(k) * stride + ch];
    }
    S[k] = host_wave_sum(v);
  }
}

// the concatenation of the parts as ONE device array (never an empty buffer: to_device)
hipError_t upload_joined(int32_t **d, std::initializer_list<const std::vector<int32_t> *> parts) {
  std::vector<int32_t> idx;
  for (const std::vector<int32_t> *v : parts) idx.insert(idx.end(), v->begin(), v->end());
  return to_device(d, idx);
}

// placed[ch] = 1 for the chains a placement starts from: those of the mask chain_fixed, chain 0 without one
int seed_fixed_chains(cora_ctx *c, const unsigned char *chain_fixed, std::vector<unsigned char> &placed) {
  const int64_t nch = c->odom.n_chains;
  placed.assign(static_cast<size_t>(nch), 0);
  if (chain_fixed) {
    bool any = false;
    for (int64_t ch = 0; ch < nch; ++ch) any = (placed[static_cast<size_t>(ch)] = chain_fixed[ch] ? 1 : 0) || any;
    if (!any) return fail(c, CORA_ERR_ARG, "chain_fixed fixes no chain");
  } else if (nch > 0) {
    placed[0] = 1;
  } else {
    return fail(c, CORA_ERR_ARG, "no chain to fix: the chain tables hold no chain");
  }
  return CORA_OK;
}

// the chain tables read the other way: the chain of a translation row (-1: of no chain), the positions of a chain (ascending
// and consecutive: a chain's positions follow each other in the tables)
struct ChainMaps {
  std::vector<int32_t> chain_of;                // [rows]
  std::vector<std::vector<int32_t>> chain_pos;  // [chains]
};
ChainMaps chain_maps(const cora_ctx *c) {
  const OdomTables &O = c->odom;
  ChainMaps m{std::vector<int32_t>(static_cast<size_t>(c->F.L.rows), -1), std::vector<std::vector<int32_t>>(static_cast<size_t>(O.n_chains))};
  for (int64_t pos = 0; pos < O.P; ++pos) {
    const int32_t ch = O.pos_chain[static_cast<size_t>(pos)];
    m.chain_of[static_cast<size_t>(O.pos_trn[static_cast<size_t>(pos)])] = ch;
    m.chain_pos[static_cast<size_t>(ch)].push_back(static_cast<int32_t>(pos));
  }
  return m;
}

// the list of len entries from entry `begin` cut into chunks of kSumChunk entries, appended to the chunk tables; chunk_owner
// (where a feature keeps one) gets `owner` per chunk
void cut_chunks(int64_t begin, int64_t len, std::vector<int32_t> &chunk_begin, std::vector<int32_t> &chunk_len, std::vector<int32_t> *chunk_owner,
                int32_t owner) {
  for (int64_t at = 0; at < len; at += kSumChunk) {
    chunk_begin.push_back(static_cast<int32_t>(begin + at));
    chunk_len.push_back(static_cast<int32_t>(std::min<int64_t>(kSumChunk, len - at)));
    if (chunk_owner) chunk_owner->push_back(owner);
  }
}

// the transform of a chain that did not move: R = I row-major, then t = 0
void identity_transform(int d, double *g) {
  for (int i = 0; i < d * d + d; ++i) g[i] = i < d * d && i / d == i % d ? 1.0 : 0.0;
}

}  // extern "C++"
}  // namespace
