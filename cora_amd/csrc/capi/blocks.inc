// Part of capi.hip (one translation unit; included there, in this order).  row moves of the exchange, STPCG measurement hooks, block algebra of LOBPCG (Gram products, combinations), timers.
int cora_pack_rows_dev(cora_ctx *c, const double *dX, int ld, const int32_t *d_rows, int64_t n, double *dPacked) {
  NEED_DEVICE(c);
  wrote(c, dPacked);
  if (!dX || !d_rows || !dPacked || ld <= 0 || n < 0) return fail(c, CORA_ERR_ARG, "bad arguments");
  HIP_TRY(c, launch_move_rows(0, n, ld, d_rows, dX, dPacked, c->stream));
  return CORA_OK;
}

int cora_scatter_rows_dev(cora_ctx *c, const double *dPacked, int ld, const int32_t *d_rows, int64_t n, double *dX) {
  NEED_DEVICE(c);
  wrote(c, dX);
  if (!dX || !d_rows || !dPacked || ld <= 0 || n < 0) return fail(c, CORA_ERR_ARG, "bad arguments");
  HIP_TRY(c, launch_move_rows(1, n, ld, d_rows, dPacked, dX, c->stream));
  return CORA_OK;
}

int cora_copy_rows_dev(cora_ctx *c, const double *dSrc, int ld, const int32_t *d_rows, int64_t n, double *dDst) {
  NEED_DEVICE(c);
  wrote(c, dDst);
  if (!dSrc || !d_rows || !dDst || ld <= 0 || n < 0) return fail(c, CORA_ERR_ARG, "bad arguments");
  HIP_TRY(c, launch_move_rows(2, n, ld, d_rows, dSrc, dDst, c->stream));
  return CORA_OK;
}

int cora_copy_shard_dev(cora_ctx *c, const double *dSrc, int ld, int shard, double *dDst) {
  NEED_DEVICE(c);
  wrote(c, dDst);
  if (!dSrc || !dDst || ld <= 0 || shard < 0 || shard >= c->F.L.world) return fail(c, CORA_ERR_ARG, "bad arguments");
  const size_t off = static_cast<size_t>(shard) * c->F.L.shard_rows * ld;
  HIP_TRY(c, hipMemcpyAsync(dDst + off, dSrc + off, static_cast<size_t>(c->F.L.shard_rows) * ld * sizeof(double),
                            hipMemcpyDeviceToDevice, c->stream));
  return CORA_OK;
}

int cora_debug_profile_stpcg(cora_ctx *c, int on) {
  NEED_DEVICE(c);
  c->prof_stpcg = on < 0 ? 0 : (on > 2 ? 2 : on);
  if (on && c->prof_events.empty()) {
    c->prof_events.resize(kProfMarks * 256, nullptr);
    for (hipEvent_t &e : c->prof_events) HIP_TRY(c, hipEventCreate(&e));
  }
  return CORA_OK;
}

int cora_debug_stpcg_phase_us(cora_ctx *c, double us[8]) {
  if (!c || !us) return CORA_ERR_ARG;
  for (int k = 0; k < 7; ++k) us[k] = c->prof_phase_us[k];
  us[7] = c->prof_kappa_folded ? 1.0 : 0.0;
  return CORA_OK;
}

int cora_debug_stpcg_path(const cora_ctx *c) { return c ? c->stpcg_path : -1; }

int cora_debug_stpcg_graph(const cora_ctx *c, long out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->stpcg_graph_captures;
  out[1] = c->stpcg_graph_replays;
  return CORA_OK;
}

int cora_debug_stpcg_hvp_us(cora_ctx *c, double *mean_us, int *count) {
  if (!c || !mean_us || !count) return CORA_ERR_ARG;
  *mean_us = c->prof_hvp_us;
  *count = c->prof_hvp_count;
  return CORA_OK;
}

int cora_dot_dev(cora_ctx *c, const double *dA, const double *dB, int k, double *out) {
  NEED_DEVICE(c);
  if (k <= 0 || k > kMaxLD || !dA || !dB || !out) return fail(c, CORA_ERR_ARG, "bad arguments");
  const int ld = ld_for(k);
  DotArgs D;
  const size_t off = static_cast<size_t>(c->F.L.base) * ld;
  for (int j = 0; j < 4; ++j) { D.a[j] = nullptr; D.b[j] = nullptr; }
  D.a[0] = dA + off;
  D.b[0] = dB + off;
  D.count = 1;
  D.n2 = c->F.L.local_rows * ld;
  int rc = ensure_red(c, 4 * 512);
  if (rc) return rc;
  D.partial = c->d_red;
  D.ticket = c->d_ticket;
  D.out = c->h_scalars;
  D.seq_out = reinterpret_cast<unsigned long long *>(c->h_scalars + 7);
  D.seq = ++c->dot_seq;
  D.mode = DOTS_PLAIN;
  D.st = D.st_host = nullptr;
  int nblocks = 0;
  HIP_TRY(c, launch_dots(D, &nblocks, c->stream));
  if ((rc = wait_dots(c, D.seq))) return rc;
  *out = c->h_scalars[0];
  return comm_allreduce(c, out, 1);
}

int cora_gram_dev(cora_ctx *c, const double *dA, int ka, const double *dB, int kb, double *G) {
  NEED_DEVICE(c);
  if (!dA || !dB || !G || ka <= 0 || kb <= 0 || ka > kMaxLD || kb > kMaxLD) return fail(c, CORA_ERR_ARG, "bad arguments");
  const int nblocks = 256, nel = ka * kb;
  int rc = ensure_red(c, static_cast<size_t>(nel) * nblocks + nel);
  if (rc) return rc;
  if ((rc = need_gram(c))) return rc;
  // (the reduction writes the results to pinned host memory itself: no copy, one wait)
  HIP_TRY(c, launch_gram(c->F.L.base, c->F.L.local_rows, dA, ka, dB, kb, c->d_red, nblocks, c->h_gram, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double *tmp = c->h_gram;
  for (int a = 0; a < ka; ++a)  // device result is row-major ka x kb
    for (int b = 0; b < kb; ++b) G[static_cast<size_t>(b) * ka + a] = tmp[static_cast<size_t>(a) * kb + b];
  return comm_allreduce(c, G, nel);
}

int cora_gram_batch_dev(cora_ctx *c, int n, const double *const *dA, const int *ka, const double *const *dB,
                        const int *kb, double *const *G) {
  NEED_DEVICE(c);
  if (n < 1 || n > 16 || !dA || !ka || !dB || !kb || !G) return fail(c, CORA_ERR_ARG, "bad arguments");
  const int nblocks = 256;
  size_t need = 0, nel_all = 0;
  for (int e = 0; e < n; ++e) {
    if (!dA[e] || !dB[e] || !G[e] || ka[e] <= 0 || kb[e] <= 0 || ka[e] > kMaxLD || kb[e] > kMaxLD)
      return fail(c, CORA_ERR_ARG, "bad block");
    const size_t nel = static_cast<size_t>(ka[e]) * kb[e];
    need += nel * nblocks;
    nel_all += nel;
  }
  // every product is the block of cora_gram_dev's kernel on its own piece of the reduction buffer: the numbers are those
  // of n separate calls -- in TWO launches (all products | all reductions, which write the results to pinned host memory)
  // and one wait, where a Rayleigh-Ritz step's twelve products were 24 launches, a copy and a wait
  int rc = ensure_red(c, need);
  if (rc) return rc;
  if ((rc = need_gram(c))) return rc;
  HIP_TRY(c, launch_gram_batch(c->F.L.base, c->F.L.local_rows, n, dA, ka, dB, kb, c->d_red, nblocks, c->h_gram, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double *tmp = c->h_gram;
  size_t off = 0;
  for (int e = 0; e < n; ++e) {
    for (int a = 0; a < ka[e]; ++a)  // device result is row-major ka x kb
      for (int b = 0; b < kb[e]; ++b) G[e][static_cast<size_t>(b) * ka[e] + a] = tmp[off + static_cast<size_t>(a) * kb[e] + b];
    rc = comm_allreduce(c, G[e], ka[e] * kb[e]);
    if (rc) return rc;
    off += static_cast<size_t>(ka[e]) * kb[e];
  }
  return CORA_OK;
}

int cora_combine_dev(cora_ctx *c, int n, const double *const *dX, const int *k, const double *const *C, int kout,
                     double *dOut) {
  NEED_DEVICE(c);
  wrote(c, dOut);
  if (n < 1 || n > 4 || !dX || !k || !C || !dOut || kout <= 0 || kout > kMaxLD) return fail(c, CORA_ERR_ARG, "bad arguments");
  std::vector<double> coef;
  int coff[4] = {0, 0, 0, 0};
  for (int b = 0; b < n; ++b) {
    if (k[b] <= 0 || k[b] > kMaxLD || !dX[b] || !C[b]) return fail(c, CORA_ERR_ARG, "bad block");
    if (dX[b] == dOut) return fail(c, CORA_ERR_ARG, "output aliases an input block");
    coff[b] = static_cast<int>(coef.size());
    for (int i = 0; i < k[b]; ++i)
      for (int j = 0; j < kout; ++j) coef.push_back(C[b][static_cast<size_t>(j) * k[b] + i]);  // row-major on device
  }
  if (coef.size() <= static_cast<size_t>(kCombineKargMax)) {  // the coefficients ride in the kernel's arguments: nothing to wait for
    HIP_TRY(c, launch_combine(c->F.L.base, c->F.L.local_rows, n, dX, k, coff, nullptr, static_cast<int>(coef.size()), kout, dOut,
                              c->stream, coef.data()));
    return CORA_OK;
  }
  int rc = ensure_red(c, coef.size() + 8);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_red, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // coef is a stack-lifetime host buffer
  HIP_TRY(c, launch_combine(c->F.L.base, c->F.L.local_rows, n, dX, k, coff, c->d_red, static_cast<int>(coef.size()),
                            kout, dOut, c->stream));
  return CORA_OK;
}

int cora_timer_start(cora_ctx *c) {
  NEED_DEVICE(c);
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  return CORA_OK;
}

int cora_timer_stop_ms(cora_ctx *c, float *ms) {
  NEED_DEVICE(c);
  if (!ms) return fail(c, CORA_ERR_ARG, "null pointer");
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  HIP_TRY(c, hipEventSynchronize(c->ev1));
  HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return CORA_OK;
}

int cora_sync(cora_ctx *c) {
  NEED_DEVICE(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CORA_OK;
}
