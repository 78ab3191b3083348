// Part of capi.hip (one translation unit; included there, in this order).  handle: creation of (partitioned) handles from the reference's CSR, destruction, rank state, row maps and statistics.

const char *cora_last_error(const cora_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int cora_ld_for(int k) { return ld_for(k); }

int cora_ctx_create_part(int device, int d, int n_poses, int n_ranges, int n_trans, const int32_t *rowptr,
                         const int32_t *colidx, const double *vals, int rank, int world, cora_ctx **out) {
  return cora_ctx_create_part_opts(device, d, n_poses, n_ranges, n_trans, rowptr, colidx, vals, rank, world, 0u, out);
}

int cora_ctx_create_part_opts(int device, int d, int n_poses, int n_ranges, int n_trans, const int32_t *rowptr,
                              const int32_t *colidx, const double *vals, int rank, int world, unsigned flags,
                              cora_ctx **out) {
  if (!out) return fail(nullptr, CORA_ERR_ARG, "out is null");
  *out = nullptr;
  if (!rowptr) return fail(nullptr, CORA_ERR_ARG, "null CSR pointer");
  {  // an empty Q (variables without a single measurement) has no index / value arrays to point at
    const int64_t N = static_cast<int64_t>(d) * n_poses + n_ranges + n_trans;
    static const int32_t no_col = 0;
    static const double no_val = 0.0;
    if (N > 0 && rowptr[N] == 0) {
      if (!colidx) colidx = &no_col;
      if (!vals) vals = &no_val;
    }
  }
  if (!colidx || !vals) return fail(nullptr, CORA_ERR_ARG, "null CSR pointer");
  cora_ctx *c = new (std::nothrow) cora_ctx();
  if (!c) return fail(nullptr, CORA_ERR_NOMEM, "out of host memory");
  try {
    build_format(d, n_poses, n_ranges, n_trans, rowptr, colidx, vals, rank, world, c->F,
                 (flags & CORA_PART_WHOLE_LONG_ROWS) == 0);
  } catch (const std::exception &e) {
    const std::string msg = e.what();
    delete c;
    return fail(nullptr, CORA_ERR_SHAPE, msg);
  }
  c->device = device;
  c->dist_long = (flags & CORA_PART_WHOLE_LONG_ROWS) == 0;
  if (device < 0) {  // plan-only handle: format inspection / host tests
    *out = c;
    return CORA_OK;
  }
#define CREATE_TRY(expr)                                                        \
  do {                                                                          \
    hipError_t e__ = (expr);                                                    \
    if (e__ != hipSuccess) {                                                    \
      const std::string m = std::string(#expr) + ": " + hipGetErrorString(e__); \
      cora_ctx_destroy(c);                                                      \
      return fail(nullptr, CORA_ERR_HIP, m);                                    \
    }                                                                           \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  c->has_device = true;
  CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  const HostFormat &F = c->F;
  CREATE_TRY(to_device(&c->d_slices, F.slices));
  if (!F.slices_pose_first.empty()) CREATE_TRY(to_device(&c->d_slices_pf, F.slices_pose_first));
  CREATE_TRY(to_device(&c->d_head_val, F.head_val));
  if (F.L.world > 1) {
    // a slice is "boundary" when one of its stored columns is a row outside this rank's shard (padding entries carry
    // local columns; what a chain slice does not store belongs to local poses by construction: format_build.cpp puts
    // the couplings of a shard's first pose to the shard before into the general slots and the tail)
    std::vector<SliceDesc> in, bd;
    const int64_t lo = F.L.base, hi = F.L.base + F.L.shard_rows;
    std::vector<int32_t> cols;
    for (const SliceDesc &sd : F.slices) {
      bool remote = false;
      cols.clear();
      slice_columns(F, sd, cols);  // (the implied columns of a chain slice are local rows)
      if (sd.type & kSliceChainFlag) {
        // a chain slice's tail holds its poses' range measurements -- landmark rows, mostly another rank's.  Only the
        // general slots decide where the slice runs; a slice that could run ahead of the exchange but for its tail is
        // split: everything except the remote pairs of the tails with the interior slices, the remote pairs (added to
        // the translation rows) with the boundary slices.
        const size_t ngen = static_cast<size_t>(sd.width) * kWave;
        for (size_t q = 0; q < ngen && !remote; ++q) remote = cols[q] < lo || cols[q] >= hi;
        bool remote_tail = false;
        for (size_t q = ngen; q < cols.size() && !remote_tail; ++q) remote_tail = cols[q] < lo || cols[q] >= hi;
        if (!remote && remote_tail) {
          SliceDesc a = sd, b = sd;
          a.nrows |= kSliceSkipRemoteTail;
          b.nrows |= kSliceRemoteTailOnly;
          in.push_back(a);
          bd.push_back(b);
          continue;
        }
        (remote ? bd : in).push_back(sd);
        continue;
      }
      for (size_t q = 0; q < cols.size() && !remote; ++q) remote = cols[q] < lo || cols[q] >= hi;
      (remote ? bd : in).push_back(sd);
    }
    c->n_slices_int = static_cast<int>(in.size());
    c->n_slices_bnd = static_cast<int>(bd.size());
    CREATE_TRY(to_device(&c->d_slices_int, in));
    CREATE_TRY(to_device(&c->d_slices_bnd, bd));
    {
      // highest priority: the exchange's small kernels take the wavefront slots the product frees first, instead of
      // queueing behind a launch that fills the GPU
      int least = 0, greatest = 0;
      CREATE_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
      CREATE_TRY(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, greatest));
    }
    CREATE_TRY(hipEventCreateWithFlags(&c->ev_operand, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&c->ev_exchanged, hipEventDisableTiming));
  }
  if (!F.long_rows.empty()) {
    CREATE_TRY(to_device(&c->d_long_rows, F.long_rows));
    CREATE_TRY(to_device(&c->d_long_owner, F.long_owner));
    CREATE_TRY(alloc_device(&c->d_long_out, F.long_rows.size() * kMaxLD * sizeof(double)));
  }
  CREATE_TRY(to_device(&c->d_sval, F.sval));
  CREATE_TRY(to_device(&c->d_scol, F.scol));
  CREATE_TRY(to_device(&c->d_perm, F.perm));
  // the long rows: the image (pieces per XCD), not the format's chunks; its values and columns are not kept on the host
  c->LI = build_long_image(F);
  CREATE_TRY(to_device(&c->d_chunks, c->LI.chunks));
  CREATE_TRY(to_device(&c->d_chunk_order, c->LI.chunk_order));
  CREATE_TRY(to_device(&c->d_lval, c->LI.lval));
  CREATE_TRY(to_device(&c->d_lcol, c->LI.lcol));
  std::vector<double>().swap(c->LI.lval);
  std::vector<int32_t>().swap(c->LI.lcol);
  CREATE_TRY(to_device(&c->d_api2int, F.api2int));
  {
    std::vector<double> dinv(F.diag.size());
    for (size_t i = 0; i < dinv.size(); ++i) dinv[i] = 1.0 / F.diag[i];
    CREATE_TRY(to_device(&c->d_diag_inv, dinv));
  }
  CREATE_TRY(alloc_device(&c->d_partials, std::max<size_t>(c->LI.chunks.size(), 1) * kMaxLD * sizeof(double)));
  CREATE_TRY(alloc_device(&c->d_tickets, std::max<size_t>(F.n_long_rows, 1) * sizeof(unsigned)));
  CREATE_TRY(hipMemset(c->d_tickets, 0, std::max<size_t>(F.n_long_rows, 1) * sizeof(unsigned)));
  // (+ 2 doubles: the pose slices' cooperative epilogue reads the blocks in pairs of doubles, kernels.hip)
  CREATE_TRY(alloc_device(&c->d_lam_st, (static_cast<size_t>(F.L.nl_poses) * d * d + 2) * sizeof(double)));
  CREATE_TRY(hipMemset(c->d_lam_st, 0, (static_cast<size_t>(F.L.nl_poses) * d * d + 2) * sizeof(double)));
  // S starts as sym(Q_PP) (Lambda = 0, what d_lam_st holds until the first point): a product before it means what it did
  CREATE_TRY(to_device(&c->d_own_sym, F.own_sym));
  CREATE_TRY(to_device(&c->d_S, F.own_sym));
  CREATE_TRY(alloc_device(&c->d_lam_ob, std::max<size_t>(F.L.nl_ranges, 1) * sizeof(double)));
  CREATE_TRY(alloc_device(&c->d_scalars, 8 * sizeof(double)));
  CREATE_TRY(alloc_device(&c->d_ticket, 4 * sizeof(unsigned)));  // [0] inner products, [1] kappa (k_spmm)
  CREATE_TRY(alloc_device(&c->d_stpcg, sizeof(StpcgState)));
  CREATE_TRY(alloc_device(&c->d_seq_counter, sizeof(unsigned long long)));
  CREATE_TRY(hipMemset(c->d_seq_counter, 0, sizeof(unsigned long long)));
  CREATE_TRY(alloc_pinned(&c->h_stpcg, 2 * sizeof(StpcgState)));
  CREATE_TRY(hipMemset(c->d_ticket, 0, 4 * sizeof(unsigned)));
  CREATE_TRY(alloc_pinned(&c->h_scalars, 8 * sizeof(double)));
  std::memset(c->h_scalars, 0, 8 * sizeof(double));
  CREATE_TRY(alloc_device(&c->d_flag, sizeof(int)));
  CREATE_TRY(alloc_pinned(&c->h_flag, sizeof(int)));
  CREATE_TRY(hipEventCreate(&c->ev0));
  CREATE_TRY(hipEventCreate(&c->ev1));
#undef CREATE_TRY
  *out = c;
  return CORA_OK;
}

int cora_ctx_create(int device, int d, int n_poses, int n_ranges, int n_trans, const int32_t *rowptr,
                    const int32_t *colidx, const double *vals, cora_ctx **out) {
  return cora_ctx_create_part(device, d, n_poses, n_ranges, n_trans, rowptr, colidx, vals, 0, 1, out);
}

void cora_ctx_destroy(cora_ctx *c) {
  if (!c) return;
  if (c->has_device) {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    native_comm_destroy(c->native_comm);
    c->native_comm = nullptr;
    if (c->p2p_pending) cora::p2p_destroy(c->p2p_pending);
    c->p2p_pending = nullptr;
    if (c->stpcg_graph) (void)hipGraphExecDestroy(c->stpcg_graph);
    c->release_format();
    c->release_factors();
    c->release_rank_state();
    c->release_solver_buffers();
    c->release_value_map();
    free_measurements(c);  // (the table, the tables built from it, the assembly and GNC buffers)
    c->release_compare();
    c->pairs.release();
    c->release_vectors();
    c->release_events();
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

int64_t cora_debug_live_allocations(void) { return g_live_allocations.load(); }

int cora_set_rank(cora_ctx *c, int p) {
  if (!c) return CORA_ERR_ARG;
  if (p < c->F.L.d || p > kMaxLD)
    return fail(c, CORA_ERR_SHAPE, "relaxation rank must satisfy d <= p <= 24");
  if (p == c->p) return CORA_OK;
  c->p = p;
  c->ld = ld_for(p);
  c->have_point = false;
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_rank_state(c);
    for (double **q : {&c->d_Y, &c->d_G, &c->d_rgrad}) {
      HIP_TRY(c, alloc_device(q, vec_bytes(c, c->ld)));
      HIP_TRY(c, hipMemsetAsync(*q, 0, vec_bytes(c, c->ld), c->stream));
    }
  }
  return CORA_OK;
}

int cora_get_rank(const cora_ctx *c) { return c ? c->p : 0; }

int cora_set_stream(cora_ctx *c, void *hip_stream) {
  NEED_DEVICE(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  c->stream = static_cast<hipStream_t>(hip_stream);
  c->own_stream = false;
  return CORA_OK;
}

int cora_ld(const cora_ctx *c) { return c ? c->ld : 0; }
int64_t cora_rows(const cora_ctx *c) { return c ? c->F.L.rows : 0; }
int64_t cora_shard_rows(const cora_ctx *c) { return c ? c->F.L.shard_rows : 0; }
int64_t cora_shard_begin(const cora_ctx *c) { return c ? c->F.L.base : 0; }
int64_t cora_nnz(const cora_ctx *c) { return c ? c->F.nnz_global : 0; }
int64_t cora_dim(const cora_ctx *c) { return c ? c->F.L.N : 0; }

int cora_row_map(const cora_ctx *c, int32_t *api_to_internal) {
  if (!c || !api_to_internal) return CORA_ERR_ARG;
  std::memcpy(api_to_internal, c->F.api2int.data(), c->F.api2int.size() * sizeof(int32_t));
  return CORA_OK;
}

int cora_remote_rows(const cora_ctx *c, int32_t *rows, int64_t *count) {
  if (!c || !count) return CORA_ERR_ARG;
  const Layout &L = c->F.L;
  const int64_t lo = L.base, hi = L.base + L.shard_rows;
  std::vector<char> seen(static_cast<size_t>(L.rows), 0);
  {
    std::vector<int32_t> cols;  // (scol also holds the chain slices' tail descriptors: only real columns count)
    for (const SliceDesc &sd : c->F.slices) slice_columns(c->F, sd, cols);
    for (int32_t col : cols) seen[col] = 1;  // padded slots repeat a real column of their lane
  }
  for (int32_t col : c->F.lcol) seen[col] = 1;
  int64_t n = 0;
  for (int64_t r = 0; r < L.rows; ++r)
    if (seen[r] && (r < lo || r >= hi)) {
      if (rows) rows[n] = static_cast<int32_t>(r);
      ++n;
    }
  *count = n;
  return CORA_OK;
}

int cora_long_rows(const cora_ctx *c, int32_t *api_rows, int64_t *count) {
  if (!c || !count) return CORA_ERR_ARG;
  const int64_t n = static_cast<int64_t>(c->F.long_rows.size());
  if (api_rows)
    for (int64_t j = 0; j < n; ++j) api_rows[j] = c->F.int2api[c->F.long_rows[static_cast<size_t>(j)]];
  *count = n;
  return CORA_OK;
}

int cora_precond_stats(const cora_ctx *c, int64_t s[4]) {
  if (!c || !s) return CORA_ERR_ARG;
  const auto &f = c->precond_f;
  s[0] = f.ready ? f.shape[kShapeStages] : 0;
  s[1] = f.ready ? f.shape[kShapeNnzW] : 0;
  s[2] = f.ready ? f.shape[kShapeNnzL] : 0;
  s[3] = f.ready ? f.shape[kShapeTopRows] : 0;
  return CORA_OK;
}

// entries the solve plan of the preconditioner stores (bench.py's algorithmic bytes of the last stage; padding of the
// substitution blocks): [0] last stage, forward product | [1] last stage, backward product | [2], [3] entry slots of the
// substitution blocks' forward / backward sweep (null padding included) | [4] substitution blocks | [5] aux rows
int cora_precond_entries(const cora_ctx *c, int64_t s[6]) {
  if (!c || !s) return CORA_ERR_ARG;
  for (int k = 0; k < 6; ++k) s[k] = c->precond_f.ready ? c->precond_f.entries[k] : 0;
  return CORA_OK;
}

int cora_format_stats(const cora_ctx *c, int64_t s[8]) {
  if (!c || !s) return CORA_ERR_ARG;
  s[0] = static_cast<int64_t>(c->F.slices.size());
  s[1] = c->F.padded_nnz;
  s[2] = c->F.long_nnz;
  s[3] = c->F.n_long_rows;
  s[4] = static_cast<int64_t>(c->F.chunks.size());
  s[5] = c->F.L.local_rows;
  s[6] = c->F.nnz_local;
  s[7] = c->F.max_width;
  return CORA_OK;
}

// Test hook (include/cora_hip.h): counted from the host copy of the format, the way k_spmm decodes it.
int cora_debug_format_shape(const cora_ctx *c, int64_t out[11]) {
  if (!c || !out) return CORA_ERR_ARG;
  const HostFormat &F = c->F;
  for (int k = 0; k < 11; ++k) out[k] = 0;
  for (const SliceDesc &sd : F.slices) {
    if ((sd.type & kSliceTypeMask) != kSliceStiefel) continue;
    if (!(sd.type & kSliceChainFlag)) { ++out[1]; continue; }
    ++out[0];
    const int64_t T = static_cast<int64_t>(static_cast<uint32_t>(sd.type) >> kSliceTailShift);
    out[2] = std::max<int64_t>(out[2], sd.width);
    out[3] = std::max(out[3], T);
    out[4] = std::max<int64_t>(out[4], (sd.type >> kSliceTailMaxShift) & kSliceTailMaxMask);
    if (T > kWave) ++out[5];
    for (int lane = 0; lane < (sd.nrows & kSliceRowsMask); ++lane) {
      const uint32_t info = static_cast<uint32_t>(F.scol[static_cast<size_t>(sd.coff) + lane]);
      const uint32_t start = info & 0xffffu, count = (info >> 16) & 0x7fu;
      out[6] += static_cast<int64_t>(count) - static_cast<int64_t>((info >> 24) & 0x7fu);
      if (count > 0 && start / kWave != (start + count - 1) / kWave) ++out[10];
    }
  }
  const int64_t first_trans = static_cast<int64_t>(F.L.d) * F.L.n + F.L.r;
  for (size_t ci = 0; ci < F.chunks.size(); ci += static_cast<size_t>(std::max(F.chunks[ci].nchunks, 1))) {
    const LongChunk &ch = F.chunks[ci];
    const int64_t api = F.int2api[static_cast<size_t>(ch.row)];
    ++out[api >= first_trans && api < first_trans + F.L.n ? 7 : 8];
    out[9] = std::max<int64_t>(out[9], ch.nchunks);
  }
  return CORA_OK;
}

int cora_format_bytes(const cora_ctx *c, int64_t b[4]) {
  if (!c || !b) return CORA_ERR_ARG;
  const HostFormat &F = c->F;
  b[0] = static_cast<int64_t>((F.sval.size() + F.lval.size()) * sizeof(double));
  b[1] = static_cast<int64_t>((F.scol.size() + F.lcol.size()) * sizeof(int32_t));
  b[2] = static_cast<int64_t>(F.slices.size() * sizeof(SliceDesc) + F.chunks.size() * sizeof(LongChunk) +
                              (F.perm.size() + F.chunk_order.size()) * sizeof(int32_t) + F.head_val.size() * sizeof(double));
  b[3] = b[0] + b[1] + b[2];
  return CORA_OK;
}
