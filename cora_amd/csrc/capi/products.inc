// Part of capi.hip (one translation unit; included there, in this order).  products: the implicit formulation's lift, the exchange of a partitioned product and its overlap, distributed long rows.
static int implicit_lift(cora_ctx *c, const double *dX, int ld, double *w0, double *w1) {
  const Layout &L = c->F.L;
  const bool sharded = L.world != 1;
  const size_t toff = static_cast<size_t>(L.trn_base) * ld;
  const size_t tbytes = static_cast<size_t>(L.nl_trans) * ld * sizeof(double);
  HIP_TRY(c, hipMemcpyAsync(w0, dX, vec_bytes(c, ld), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(w0 + toff, 0, tbytes, c->stream));
  SpmmArgs A = spmm_args(c, w0, w1);
  int rc;
  if (sharded) {
    if ((rc = exchange_and_product(c, A, ld, EPI_NONE))) return rc;               // (the exported translations are zero)
  } else {
    HIP_TRY(c, launch_spmm(A, ld, L.d, EPI_NONE, c->stream));                      // w1[trans] = B^T X
  }
  const int64_t last = pinned_translation_row(c);                                  // pinned translation (the API's last row)
  const bool mine = last >= L.base && last < L.base + L.shard_rows;
  if (mine) HIP_TRY(c, launch_zero_row(w1, static_cast<size_t>(last), ld, c->stream));
  if (sharded) {  // every rank: all translation rows of B^T X (the solve is replicated)
    if (c->native_comm && c->comm_user == c->native_comm && !cora::env_flag(cora::Env::ImplicitWholeGather)) {
      // the library's own communication gathers the translation rows alone, packed: 2 / 9 of a shard's rows at d = 3
      if (native_allgather_rows(c->native_comm, w1, ld, L.trn_base - L.base, L.nl_trans))
        return fail(c, CORA_ERR_HIP, "all-gather step failed: " + native_error(c->native_comm));
    } else if ((rc = comm_allgather(c, w1, ld))) {
      return rc;
    }
  }
  double *w2;
  if ((rc = get_scratch(c, 8, ld, &w2))) return rc;
  if ((rc = factor_solve(c, c->implicit_f, ld, w1, w2))) return rc;                // w2[trans] = M^-1 B^T X
  HIP_TRY(c, launch_axpby(static_cast<int64_t>(L.nl_trans) * ld, -1.0, w2 + toff, 0.0, w0 + toff, c->stream));
  if (mine) HIP_TRY(c, launch_zero_row(w0, static_cast<size_t>(last), ld, c->stream));  // w0 = [X; t; 0]
  return CORA_OK;
}

static int implicit_product(cora_ctx *c, const double *dX, int ld, int epi, double *dOut) {
  if (!c->implicit_f.ready)
    return fail(c, CORA_ERR_NOT_READY, "implicit formulation needs cora_implicit_set_cholesky");
  double *w0, *w1;
  int rc;
  if ((rc = get_scratch(c, 3, ld, &w0))) return rc;
  if ((rc = get_scratch(c, 4, ld, &w1))) return rc;
  if ((rc = implicit_lift(c, dX, ld, w0, w1))) return rc;
  SpmmArgs A = spmm_args(c, w0, dOut);
  if (c->F.L.world != 1) {
    if ((rc = exchange_and_product(c, A, ld, epi))) return rc;
  } else {
    HIP_TRY(c, launch_spmm(A, ld, c->F.L.d, epi, c->stream));
  }
  const Layout &L = c->F.L;
  HIP_TRY(c, hipMemsetAsync(dOut + static_cast<size_t>(L.trn_base) * ld, 0,
                            static_cast<size_t>(L.nl_trans) * ld * sizeof(double), c->stream));
  return CORA_OK;
}

// one product in the active formulation
static int apply_product(cora_ctx *c, const double *dX, int ld, int epi, double *dOut) {
  if (c->implicit) return implicit_product(c, dX, ld, epi, dOut);
  return exchange_and_product(c, spmm_args(c, dX, dOut), ld, epi);
}

// true when products of this handle run as two launches around the exchange (exchange_and_product)
static bool product_overlaps_exchange(const cora_ctx *c) {
  const bool off = cora::env_flag(cora::Env::NoExchangeOverlap);
  // The split costs a second launch and two cross-stream dependencies (a few microseconds); it pays when the interior
  // slices run longer than that.  Measured with the in-process transport, 8 partitions of the 10^5-pose graph on one
  // GPU (500 slices per rank, a 3 us product): 290-350 us per step serial, 460 us split -- so the default takes the
  // split from kOverlapMinSlices interior slices on (about 10 us of product; 10^6 poses on 8 GPUs: 5 000 per rank).
  const int64_t min_slices = cora::env_int(cora::Env::ExchangeOverlapMinSlices);
  const bool wanted = c->overlap_exchange == 2 || (c->overlap_exchange == 1 && c->n_slices_int >= min_slices);
  return c->F.L.world > 1 && wanted && !off && c->native_comm && c->comm_user == c->native_comm &&
         c->comm_exchange != nullptr && c->n_slices_int > 0 && c->n_slices_bnd > 0 &&
         (c->F.chunks.empty() || !c->F.long_rows.empty());  // (whole long rows read columns of every shard)
}

// true when a product of this handle is ONE collective: the library's own communication and distributed long rows -- the
// chunks of the long rows run first (they read columns of this shard only), their partial sums travel with the exported
// rows of the operand, and every owner adds them up in rank order.  (Injected callbacks: exchange, product, all-reduce
// of the slots, as before.)
static bool product_one_collective(const cora_ctx *c) {
  return c->F.L.world > 1 && !c->local_products && c->native_comm && c->comm_user == c->native_comm && c->comm_exchange != nullptr &&
         !c->F.long_rows.empty();
}

// number of kappa slots an EPI_HVP_K product of this handle writes (launch_product / exchange_and_product)
static int product_kappa_slots(const cora_ctx *c, const SpmmArgs &A) {
  if (product_one_collective(c)) {  // chunk launch | one slot per long row | slice launch (or interior | boundary)
    SpmmArgs Ac = A, A1 = A, A2 = A;
    Ac.n_slices = 0;
    A1.n_chunks = A2.n_chunks = 0;
    if (!product_overlaps_exchange(c)) return launch_spmm_blocks(Ac) + A.n_long_rows + launch_spmm_blocks(A1);
    A1.n_slices = c->n_slices_int;
    A2.n_slices = c->n_slices_bnd;
    return launch_spmm_blocks(Ac) + A.n_long_rows + launch_spmm_blocks(A1) + launch_spmm_blocks(A2);
  }
  if (!product_overlaps_exchange(c)) return launch_spmm_kappa_slots(A);
  SpmmArgs A1 = A, A2 = A;
  A1.n_slices = c->n_slices_int;
  A2.n_slices = c->n_slices_bnd;
  A2.n_chunks = 0;
  return launch_spmm_blocks(A1) + A.n_long_rows + launch_spmm_blocks(A2);
}

// Exchange of the operand's remote rows + the product.
//   * the library's own communication: pack (+ zeroed slots) -> the long rows' chunks -> ONE all-gather of rows and slots
//     -> unpack (rows into X, slots summed into the owners' rows) -> the slices.  With the overlap on, gather and unpack
//     run on comm_stream while the interior slices -- which read rows of this rank's shard only -- run on the handle's
//     stream, and the boundary slices follow when the exchange has landed.
//   * injected callbacks (cora_set_comm): exchange, product, all-reduce of the long rows' slots, in that order.
static int exchange_and_product(cora_ctx *c, SpmmArgs A, int ld, int epi) {
  if (c->local_products) return launch_product(c, A, ld, epi, /*finish=*/false);  // timing hook: no collective step at all
  if (!product_one_collective(c)) {
    if (!product_overlaps_exchange(c)) {
      const int rc = comm_exchange(c, A.X, ld);
      if (rc) return rc;
      return launch_product(c, A, ld, epi);
    }
    // (overlap without distributed long rows: whole long rows are excluded by product_overlaps_exchange, so this is a
    // handle with no long rows at all)
    HIP_TRY(c, hipEventRecord(c->ev_operand, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->comm_stream, c->ev_operand, 0));
    SpmmArgs A1 = A;
    A1.slices = c->d_slices_int;
    A1.slices_pose_first = nullptr;
    A1.n_slices = c->n_slices_int;
    int rc = launch_product(c, A1, ld, epi, /*finish=*/false);
    if (rc) return rc;
    if (native_exchange_on(c->native_comm, const_cast<double *>(A.X), ld, c->comm_stream))
      return fail(c, CORA_ERR_HIP, "exchange step failed: " + native_error(c->native_comm));
    HIP_TRY(c, hipEventRecord(c->ev_exchanged, c->comm_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_exchanged, 0));
    SpmmArgs A2 = A;
    A2.slices = c->d_slices_bnd;
    A2.slices_pose_first = nullptr;
    A2.n_slices = c->n_slices_bnd;
    A2.n_chunks = 0;
    A2.n_long_rows = 0;
    if (A.kappa_partial) A2.kappa_partial = A.kappa_partial + launch_spmm_blocks(A1) + A.n_long_rows;
    HIP_TRY(c, launch_spmm(A2, ld, c->F.L.d, epi, c->stream));
    return CORA_OK;
  }
  cora_native_comm *nc = c->native_comm;
  const bool kap = epi == EPI_HVP_K && A.kappa_partial;
  double *slots = nullptr;
  auto mark = [&](int i) {  // (measurement hook: five phases, six events)
    if (c->phase_timing && static_cast<size_t>(i) < c->phase_events.size()) (void)hipEventRecord(c->phase_events[i], c->stream);
  };
  mark(0);
  if (native_product_pack(nc, A.X, ld, c->stream, &slots)) return fail(c, CORA_ERR_HIP, "exchange step failed: " + native_error(nc));
  mark(1);
  SpmmArgs Ac = A;  // the long rows' chunks: partial sums over this rank's columns -> the slots that travel
  Ac.n_slices = 0;
  Ac.slices_pose_first = nullptr;
  Ac.long_out = slots;
  HIP_TRY(c, launch_spmm(Ac, ld, c->F.L.d, epi, c->stream));
  mark(2);
  const int kc = launch_spmm_blocks(Ac);
  double *klong = kap ? A.kappa_partial + kc : nullptr;
  SpmmArgs A1 = A;
  A1.n_chunks = 0;
  A1.n_long_rows = 0;
  if (kap) A1.kappa_partial = A.kappa_partial + kc + A.n_long_rows;
  if (!product_overlaps_exchange(c)) {
    if (native_product_gather(nc, const_cast<double *>(A.X), ld, c->stream, A.out, klong, c->phase_timing ? c->phase_events[3] : nullptr))
      return fail(c, CORA_ERR_HIP, "exchange step failed: " + native_error(nc));
    mark(4);
    HIP_TRY(c, launch_spmm(A1, ld, c->F.L.d, epi, c->stream));
    mark(5);
    return CORA_OK;
  }
  HIP_TRY(c, hipEventRecord(c->ev_operand, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->comm_stream, c->ev_operand, 0));
  if (native_product_gather(nc, const_cast<double *>(A.X), ld, c->comm_stream, A.out, klong))
    return fail(c, CORA_ERR_HIP, "exchange step failed: " + native_error(nc));
  HIP_TRY(c, hipEventRecord(c->ev_exchanged, c->comm_stream));
  SpmmArgs A2 = A1;
  A1.slices = c->d_slices_int;
  A1.slices_pose_first = nullptr;
  A1.n_slices = c->n_slices_int;
  HIP_TRY(c, launch_spmm(A1, ld, c->F.L.d, epi, c->stream));   // interior slices: no row of another rank is read
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_exchanged, 0));
  A2.slices = c->d_slices_bnd;
  A2.slices_pose_first = nullptr;
  A2.n_slices = c->n_slices_bnd;
  if (kap) A2.kappa_partial = A1.kappa_partial + launch_spmm_blocks(A1);
  HIP_TRY(c, launch_spmm(A2, ld, c->F.L.d, epi, c->stream));
  return CORA_OK;
}

// A product of a partitioned handle WITHOUT the library's own communication ends with its DISTRIBUTED long rows
// (format_build.cpp): the slots of partial sums are added over the ranks through the injected all-reduce and the owner
// copies its rows to the result; the rows' shares of kappa follow (EPI_HVP_K).
static int launch_product(cora_ctx *c, SpmmArgs A, int ld, int epi, bool finish) {
  const int nl = static_cast<int>(c->F.long_rows.size());
  const bool dist = c->F.L.world > 1 && nl > 0;
  if (dist) {
    A.long_out = c->d_long_out;
    HIP_TRY(c, hipMemsetAsync(c->d_long_out, 0, static_cast<size_t>(nl) * ld * sizeof(double), c->stream));
  }
  HIP_TRY(c, launch_spmm(A, ld, c->F.L.d, epi, c->stream));
  return finish ? finish_long_rows(c, A, ld, epi) : CORA_OK;
}

// (A: the arguments of the launch that ran the long-row chunks -- its block count places the rows' kappa slots)
static int finish_long_rows(cora_ctx *c, const SpmmArgs &A, int ld, int epi) {
  const int nl = static_cast<int>(c->F.long_rows.size());
  const bool dist = c->F.L.world > 1 && nl > 0;
  if (!dist) return CORA_OK;
  const int n = nl * ld;
  if (c->native_comm && c->comm_user == c->native_comm) {
    if (native_allreduce_dev(c->native_comm, c->d_long_out, n))
      return fail(c, CORA_ERR_HIP, "all-reduce step failed: " + native_error(c->native_comm));
  } else if (c->comm_allreduce) {
    std::vector<double> h(static_cast<size_t>(n));
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_long_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int at = 0; at < n; at += 512) {  // "a few doubles" per call: the callbacks' contract
      const int rc = comm_allreduce(c, h.data() + at, std::min(512, n - at));
      if (rc) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_long_out, h.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    // nobody can add the slots up: the landmark rows of the result would silently be PARTIAL sums (round-3 advice).
    // A handle that is to run without communication keeps whole long rows: cora_ctx_create_part_opts(...,
    // CORA_PART_WHOLE_LONG_ROWS).
    return fail(c, CORA_ERR_NOT_READY,
                "partitioned handle with distributed long rows and no communication: install cora_set_comm / cora_comm_create_*, "
                "or create the handle with CORA_PART_WHOLE_LONG_ROWS");
  }
  const int kbase = launch_spmm_blocks(A);
  HIP_TRY(c, launch_long_finish(nl, ld, c->F.L.rank, c->d_long_rows, c->d_long_owner, c->d_long_out, A.X, A.out,
                                (epi == EPI_HVP_K && A.kappa_partial) ? A.kappa_partial + kbase : nullptr, c->stream));
  return CORA_OK;
}
