// Part of capi.hip (one translation unit; included there, in this order).  the device-resident Steihaug-Toint PCG (all forms of the iteration) and the injected communication.
// can cora_stpcg_dev run on this handle?  One GPU: always.  Partitioned: with the library's own communication (the
// reductions stay on the device), the explicit formulation, a row-local preconditioner and 16-byte aligned shards.
// The answer is the same on every rank (the two loops make different collective calls): nothing in it depends on the
// rank's own rows.  The flat vector passes of a partitioned handle run over the PADDED shard (shard_rows is a multiple
// of 8, so the range is even and 64-byte aligned whatever the row stride); padding rows are zero in every resident
// vector -- allocations are zeroed and no kernel writes them -- and add nothing to an update or an inner product.
static bool stpcg_device_ok(const cora_ctx *c) {
  if (c->F.L.world == 1) return true;
  // the library's own communication must be the ACTIVE transport (after cora_comm_native_enable(0) or a later
  // cora_set_comm the reductions would go one way and the operand's exchange another -- round-3 advice).  The answer must
  // not depend on anything rank-local: the Cholesky case is decided by the preconditioner's KIND (a missing factor fails
  // loudly in the solve, on every rank alike).
  return c->native_comm && c->comm_user == c->native_comm && c->comm_exchange != nullptr && !c->implicit && c->ld <= 12;
}

// Steihaug-Toint truncated PCG for  min <g,s> + 1/2 <s,Hs>,  ||s||_M <= Delta, entirely on the device
// (the inner solver of Optimization::Riemannian::TNT, called from src/CORA.cpp:139-140).  The scalar
// recurrences live in a StpcgState that the inner-product kernels update themselves, so the host only
// enqueues iterations -- a few at a time -- and looks at the state's pinned mirror between batches.
// dPg != nullptr: the caller already holds P g and the inner products <g, g>, <g, P g> (TNT computes them for its
// stopping tests): the solve starts without a preconditioner apply and without a reduction of its own.
static int stpcg_run(cora_ctx *c, const double *dGrad, const double *dPg, double gg, double gPg, double Delta,
                     double kappa_fgr, double theta, int max_iters, double *dS, double *dR, double *dV, double *dP,
                     double *dHp, int *iters, double *step_M_norm) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  if (!dGrad || !dS || !dR || !dV || !dP || !dHp || !iters || !step_M_norm || max_iters < 0)
    return fail(c, CORA_ERR_ARG, "bad arguments");
  for (const double *w : {dS, dR, dV, dP, dHp}) wrote(c, w);
  // Partitioned handle: the same fused iteration, every rank on its own rows, with the library's own communication
  // (cora_comm_create_*): the operand's remote rows are exchanged before the product, and the three inner products are
  // summed over the ranks ON THE DEVICE -- kappa after the product, <r, r> and <r, v> together after the projection --
  // by an all-reduce on the handle's stream, followed by a one-thread launch for the scalar step.  The host enqueues
  // and looks at the pinned mirror between batches, exactly as on one GPU.
  const bool sharded = c->F.L.world != 1;
  if (sharded && !stpcg_device_ok(c))
    return fail(c, CORA_ERR_ARG, "the device-resident STPCG on a partitioned handle needs cora_comm_create_* and the explicit formulation");
  int rc;
  double rr_rv[2];
  if (dPg) {  // s = 0, r = g, p = -P g in one pass
    const size_t off0 = static_cast<size_t>(c->F.L.base) * c->ld;
    HIP_TRY(c, launch_stpcg_init(c->F.L.local_rows * c->ld, dGrad + off0, dPg + off0, dS + off0, dR + off0, dP + off0,
                                 c->stream));
    rr_rv[0] = gg;
    rr_rv[1] = gPg;
  } else {  // s = 0, r = g, v = P r, p = -v
    if ((rc = cora_axpby_dev(c, 0.0, dGrad, 0.0, dS))) return rc;
    if ((rc = cora_axpby_dev(c, 1.0, dGrad, 0.0, dR))) return rc;
    if ((rc = cora_precondition_projected_dev(c, dR, dV))) return rc;
    if ((rc = cora_axpby_dev(c, -1.0, dV, 0.0, dP))) return rc;
    const double *A[2] = {dR, dR};
    const double *B[2] = {dR, dV};
    if ((rc = cora_dots_dev(c, 2, A, B, rr_rv))) return rc;
  }
  const double r0 = std::sqrt(rr_rv[0]);
  if (c->stpcg_pending_seq) {  // the last solve's neutral iteration writes the mirror too: it must be behind us before
    if ((rc = wait_dots(c, c->stpcg_pending_seq))) return rc;  // the mirror is reset (long finished by now: no wait)
    c->stpcg_pending_seq = 0;
  }
  StpcgState &H = c->h_stpcg[1];  // staging copy for the upload; h_stpcg[0] is the mirror the kernels write
  H = StpcgState();
  H.r_v = rr_rv[1];
  H.p_M2 = rr_rv[1];
  H.Delta2 = Delta * Delta;
  H.target = r0 * std::min(kappa_fgr, std::pow(r0, theta));
  H.coef_beta = 1.0;
  H.max_iters = max_iters;
  c->h_stpcg[0] = H;
  HIP_TRY(c, hipMemcpyAsync(c->d_stpcg, &H, sizeof(StpcgState), hipMemcpyHostToDevice, c->stream));
  const int64_t n = (sharded ? c->F.L.shard_rows : c->F.L.local_rows) * c->ld;  // sharded: the padded shard (stpcg_device_ok)
  DotArgs D;
  for (int j = 0; j < 4; ++j) D.a[j] = D.b[j] = nullptr;
  D.n2 = n;
  D.count = 1;
  D.mode = DOTS_PLAIN;
  D.seq_out = nullptr;
  D.seq = 0;
  if ((rc = ensure_red(c, 4 * 512))) return rc;
  D.partial = c->d_red;
  D.ticket = c->d_ticket;
  D.out = c->d_scalars;
  D.st = c->d_stpcg;
  D.st_host = &c->h_stpcg[0];
  // How far the host runs ahead of the state it has seen.  One GPU: ONE iteration on small problems (`depth`, below: the
  // host waits for iteration k - 1 before it enqueues k + 1, so the GPU never waits for the host and exactly one
  // iteration is enqueued past the stopping point, neutralised by the state), none on large ones (the reductions' block
  // runs in the launch BEFORE the backward sweep, which covers the host's reaction).  Partitioned handles and graph replay:
  // `batch` iterations between two looks, everything waited for (every rank must enqueue the same collective calls, so
  // the decision may only depend on a state that no iteration in flight can have advanced).
  // (the three switches of the host loop are read per solve: tests/test_gpu_solver.py runs one problem under each form)
  const int batch_env = static_cast<int>(cora::env_int(cora::Env::StpcgBatch));
  const int batch = batch_env > 0 ? batch_env : (n > 1000000 ? 1 : 4);
  int enqueued = 0;
  // Fused iteration (explicit formulation, one shard, row strides up to 12): six passes instead of nine --
  //   Hp = H p | kappa = <p, Hp> | r += alpha Hp with <r, r> | Cholesky solve | v = Proj_Y(x) with <r, v> |
  //   s += alpha p, p = -v + beta p
  // The scalar steps run in the last block of the pass that finishes the inner product they need.
  const bool chol = c->precond == CORA_PRECOND_BLOCK_CHOLESKY || c->precond == CORA_PRECOND_REGULARIZED_CHOLESKY;
  const size_t off = static_cast<size_t>(c->F.L.base) * c->ld;
  const bool fused = sharded || (!c->implicit && c->ld <= 12 && n % 2 == 0 && (off * sizeof(double)) % 16 == 0 &&
                                 !cora::env_flag(cora::Env::NoFuse));
  // Sweep-fused iteration (the above, with a two-stage Cholesky solve plan): five passes and a scalar step --
  //   Hp = H p with the partials of kappa | kappa | forward sweep on r += alpha Hp with <r, r> | last stage (2 products) |
  //   backward sweep with v = Proj_Y(x) and <r, v> | s += alpha p, p = -v + beta p
  bool sweep_fused = false, inverse_fused = false;
  SubFuse FF, FB;
  double *kappa_partial = nullptr;
  int kappa_blocks = 0;
  RvTail tail{}, sq{};
  if (fused) {
    const RowArgs R = row_args(c);
    const int64_t units = static_cast<int64_t>(R.nl_poses) + R.nl_ranges + R.nl_trans;
    size_t need = std::max<size_t>(4 * 512, static_cast<size_t>((units + 255) / 256) + 8);
    const cora_ctx::DevFactor &f = c->precond_f;
    sweep_fused = !c->implicit && chol && f.ready && f.fuse_ok && !f.stages.empty() && f.stages[0].is_sub && c->ld * c->F.L.d <= 24 && c->ld <= 11 &&
                  !cora::env_flag(cora::Env::NoSweepFuse);  // (row stride x d > 24: the fused backward sweep spills)
    // slots of the sweep-fused reductions: <r, r> per block of the forward sweep's launch, |y|^2 per solve block,
    // |row|^2 per row of the last stage's forward product
    size_t rr_slots = 0, yy_slots = 0, sq_slots = 0;
    if (sweep_fused) {
      rr_slots = static_cast<size_t>(launch_subblock_blocks(f.stages[0].sub)) + 8;
      yy_slots = static_cast<size_t>(f.stages[0].sub.nblocks) + 8;
      const RowOpDev &fb = f.stages[1].fwd_b;
      sq_slots = static_cast<size_t>(rowop_rowsq_slots(fb)) + 8;
    }
    // one explicit inverse W = L^-1 and nothing else (two products per solve), no pinned-row stage in between
    inverse_fused = !sharded && !sweep_fused && chol && f.ready && f.stages.size() == 1 && !f.stages[0].dense && !f.stages[0].is_sub &&
                    !f.stages[0].has_fwd_a && !f.stages[0].has_bwd_a && !cora::env_flag(cora::Env::NoInverseFuse);
    const bool residual_slots = !cora::env_flag(cora::Env::NoResidualSlots);
    if (inverse_fused) {
      const RowOpDev &fb = f.stages[0].fwd_b;
      sq_slots = static_cast<size_t>(rowop_rowsq_slots(fb)) + 8;
      if (residual_slots) rr_slots = static_cast<size_t>(kappa_residual_slots_blocks(n)) + 8;
    }
    kappa_blocks = product_kappa_slots(c, spmm_args(c, dP, dHp));
    if ((rc = ensure_red(c, need + static_cast<size_t>(kappa_blocks) + rr_slots + yy_slots + sq_slots))) return rc;
    D.partial = c->d_red;
    kappa_partial = c->d_red + need;
    if (inverse_fused) {
      double *rr_partial = kappa_partial + kappa_blocks, *rowsq = rr_partial + rr_slots;
      sq.rowsq_out = rowsq;
      // kappa and <r, r> are finished by the tail block too (k_kappa_residual_slots): the residual pass has no ticket and
      // no last block, and the iteration's three scalar steps run in one place.  (CORA_NO_RESIDUAL_SLOTS: the residual
      // pass finishes both itself, n_rr = n_kappa = 0 -- the form measured against in profiles/r05_kernel_evolution.md)
      tail.rr_partial = rr_partial;
      tail.n_rr = residual_slots ? kappa_residual_slots_blocks(n) : 0;
      if (residual_slots) {
        tail.kappa_partial = kappa_partial;
        tail.n_kappa = kappa_blocks;
      }
      tail.yy_partial = rowsq;
      tail.n_yy = 0;
      tail.rowsq = rowsq;
      tail.n_rowsq = static_cast<int>(sq_slots) - 8;
      tail.st = c->d_stpcg;
      tail.st_host = &c->h_stpcg[0];
      tail.seq_out = reinterpret_cast<unsigned long long *>(c->h_scalars + 7);
    }
    if (sweep_fused) {
      const Layout &L = c->F.L;
      double *rr_partial = kappa_partial + kappa_blocks, *yy_partial = rr_partial + rr_slots, *rowsq = yy_partial + yy_slots;
      FF.dot = D;
      FF.Hp = dHp;
      FF.r = dR;
      FF.d = L.d;
      FF.rot_base = L.rot_base;
      FF.rng_base = L.rng_base;
      FF.trn_base = L.trn_base;
      FF.rr_partial = rr_partial;
      FF.yy_partial = yy_partial;
      FB = FF;
      FB.Y = c->d_Y;
      FB.p = dP;
      FB.s = dS;
      // the two reductions of the iteration are finished by an extra block of the last stage's SECOND product:
      // <r, r> from the forward sweep's slots, <r, v> = |L^-1 r|^2 from its |y|^2 slots + the squared norms of the rows
      // of t_1, which the last stage's FIRST product leaves (sq)
      sq.rowsq_out = rowsq;
      tail.rr_partial = rr_partial;
      tail.n_rr = launch_subblock_blocks(f.stages[0].sub);
      tail.yy_partial = yy_partial;
      tail.n_yy = f.stages[0].sub.nblocks;
      tail.rowsq = rowsq;
      tail.n_rowsq = static_cast<int>(sq_slots) - 8;
      tail.st = c->d_stpcg;
      tail.st_host = &c->h_stpcg[0];
      tail.seq_out = reinterpret_cast<unsigned long long *>(c->h_scalars + 7);
      // kappa without a launch of its own (one GPU, mid-size problems): every block of the forward sweep adds the
      // product's partials and runs the scalar step privately, the tail block of the last stage advances the state.
      // Measured: with a few hundred partials (the reference's data sets: 288) an iteration loses the 4.5 us launch and
      // the sweep does not notice (plaza1 69.0 -> 66.6 us per product end to end, tiers 88.5 -> 84.8, mrclam6 109 -> 104.5);
      // with the 2 470 partials of 10^5 poses every block's sum costs the sweep the 5.2 us the launch took (1 060 blocks
      // reading the same 20 KB through eight L2s): there, and above, the launch stays.
      // (round 5: a solve block adds the partials BEHIND the loads of its right-hand sides -- kernels.hip, late_kappa --, which
      // moved the break-even up: at 10^5 poses the iteration goes from 111.8 to 110.6 us without the launch; 10^6 poses, 24 k
      // partials, keep it)
      if (!sharded && kappa_blocks <= cora::env_int(cora::Env::KappaFoldMax) && !cora::env_flag(cora::Env::NoKappaFold)) {
        FF.kappa_partial = tail.kappa_partial = kappa_partial;
        FF.n_kappa = tail.n_kappa = kappa_blocks;
      }
    }
  }
  c->stpcg_path = sweep_fused ? 2 : inverse_fused ? 3 : fused ? 1 : 0;
  c->prof_kappa_folded = sweep_fused && FF.n_kappa > 0;
  // hipGraph replay of whole batches (one GPU, the fused forms): OPT-IN, CORA_STPCG_GRAPH=1.  Measured on this part, replaying the batches does not bring the launches of an iteration
  // closer together -- a dependent kernel of 5 us and more already has its successor's packet waiting, what is left
  // between them is the dependency itself -- and a six-launch graph per iteration costs the host more than six launches:
  // iteration at 10^5 poses 116 -> 122 us, the reference's data sets unchanged.  tools/launch_lab.hip shows the gain only
  // for kernels shorter than the launch rate, 3.5 -> 2.1 us each.  Kept: same bits, tested, one switch.
  const bool graphs_on = cora::env_flag(cora::Env::StpcgGraph);  // (read per solve: tests flip it)
  const bool use_graph = graphs_on && fused && !sharded && !c->prof_stpcg && max_iters >= batch;
  std::vector<uintptr_t> key;
  if (use_graph) {
    double *t = nullptr, *t2 = nullptr;
    if (sweep_fused && (rc = get_scratch(c, 6, c->ld, &t, c->precond_f.aux_rows))) return rc;  // (allocations happen here,
    if ((sweep_fused || inverse_fused) && (rc = get_scratch(c, 7, c->ld, &t2))) return rc;      // not under capture)
    if (chol && !sweep_fused && !inverse_fused) {  // the general solve allocates its own scratch on first use: one warm call
      if ((rc = chol_solve(c, c->ld, dR, dV))) return rc;
    }
    auto U = [](const void *q) { return reinterpret_cast<uintptr_t>(q); };
    key = {static_cast<uintptr_t>(c->stpcg_path), static_cast<uintptr_t>(c->ld), static_cast<uintptr_t>(batch), static_cast<uintptr_t>(n),
           U(dS), U(dR), U(dV), U(dP), U(dHp), U(c->d_red), static_cast<uintptr_t>(kappa_blocks), U(c->d_Y), U(c->d_lam_st), U(c->d_S), U(t), U(t2),
           static_cast<uintptr_t>(c->precond), static_cast<uintptr_t>(c->precond_f.generation), U(c->stream),
           static_cast<uintptr_t>(c->F.slices.size())};
    for (int i = 0; i < kScratchSlots; ++i) key.push_back(U(c->scratch[i]));  // (whatever a solve in the batch borrows)
    // the device's sequence counter = the host's count (launches of this solve take their numbers from it)
    unsigned long long *stage = reinterpret_cast<unsigned long long *>(c->h_scalars + 6);
    *stage = c->dot_seq;
    HIP_TRY(c, hipMemcpyAsync(c->d_seq_counter, stage, sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    D.seq_counter = c->d_seq_counter;
    tail.seq_counter = c->d_seq_counter;
    FF.dot.seq_counter = FB.dot.seq_counter = c->d_seq_counter;
  }
  const int depth_env = static_cast<int>(cora::env_int(cora::Env::StpcgDepth));
  const bool pipelined = !sharded && !use_graph && batch_env <= 0;
  const int depth = depth_env >= 0 ? depth_env : (batch == 1 ? 0 : 1);
  // Small problems, the default: the host runs ahead by the next iteration's PRODUCT only.  The reductions' block of
  // iteration k runs in its second-to-last launch (or finishes it: the unfused forms); behind it the GPU still has the
  // last launch of k and the product of k + 1, which is what the host needs to see the state and enqueue the rest of
  // k + 1 -- the GPU does not wait for the host, and past the stopping point there is one product (its results are never
  // read), not one whole neutral iteration.  CORA_STPCG_DEPTH=1 is the whole-iteration form.
  const int ahead_env = static_cast<int>(cora::env_int(cora::Env::StpcgAhead));  // (lab)
  const bool product_ahead = pipelined && !c->prof_stpcg && (ahead_env >= 0 ? ahead_env != 0 : (depth == 1 && depth_env < 0));
  bool have_product = false;
  std::deque<unsigned long long> in_flight;
  while (c->h_stpcg[0].status == 0 && enqueued < max_iters) {
    unsigned long long seq = 0;
    const bool whole = use_graph && max_iters - enqueued >= batch;
    if (whole && c->stpcg_graph && key == c->stpcg_graph_key) {  // replay: `batch` iterations in one call
      HIP_TRY(c, hipGraphLaunch(c->stpcg_graph, c->stream));
      enqueued += batch;
      seq = (c->dot_seq += static_cast<unsigned long long>(batch));
      ++c->stpcg_graph_replays;
      if ((rc = wait_dots(c, seq))) return rc;
      continue;
    }
    const bool capture = whole;
    if (capture) {
      if (c->stpcg_graph) (void)hipGraphExecDestroy(c->stpcg_graph);
      c->stpcg_graph = nullptr;
      c->stpcg_graph_key.clear();
      HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    }
    auto end_capture = [&](bool ok) -> int {  // closes the capture (always) and, when the batch was recorded whole, runs it
      if (!capture) return CORA_OK;
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(c->stream, &g);
      if (e != hipSuccess || !g) return fail(c, CORA_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
      if (!ok) { (void)hipGraphDestroy(g); return CORA_OK; }
      const hipError_t ei = hipGraphInstantiate(&c->stpcg_graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (ei != hipSuccess) { c->stpcg_graph = nullptr; return fail(c, CORA_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
      c->stpcg_graph_key = key;
      ++c->stpcg_graph_captures;
      HIP_TRY(c, hipGraphLaunch(c->stpcg_graph, c->stream));
      return CORA_OK;
    };
    // (the launches of one iteration; under capture an error must still close the capture: the caller does)
    // part: 0 the whole iteration | 1 its product alone (Hp = H p, with the partials of kappa) | 2 everything after the product
    auto one_iteration = [&](int part = 0) -> int {
      // measurement hook (cora_debug_profile_stpcg): mark 0 before the product, 1 after it; mode 2 also after every
      // other launch of the sweep-fused form -- 2 kappa | 3 forward sweep | 4, 5 the last stage's two products | 6
      // backward sweep (a mark is an event on the handle's stream: it does not reorder anything)
      const bool prof = c->prof_stpcg && kProfMarks * (static_cast<size_t>(enqueued) + 1) <= c->prof_events.size();
      auto mark = [&](int i) {
        // (mode 1: the product's two marks and the two marks in a row that measure what a mark costs)
        if (prof && (i <= 1 || i >= 6 || c->prof_stpcg >= 2)) (void)hipEventRecord(c->prof_events[kProfMarks * enqueued + i], c->stream);
      };
      mark(0);
      if (fused) {
        // Hp = H p with the partials of kappa | kappa, alpha, r += alpha Hp with <r, r> | preconditioner | ...
        if (part != 2) {
          SpmmArgs A = spmm_args(c, dP, dHp);
          A.kappa_partial = kappa_partial;
          if ((rc = exchange_and_product(c, A, c->ld, EPI_HVP_K))) return rc;  // (one rank: the product alone)
        }
        if (part == 1) return CORA_OK;
        mark(1);
        if (sharded) {
          // kappa: local partials (fixed order) -> sum over the ranks -> scalar step;  then r += alpha Hp with <r, r>
          // and v = Proj_Y(D^-1 r) with <r, v>, both left on the device, one all-reduce for the two, scalar step
          double *ds = native_scalars(c->native_comm);
          HIP_TRY(c, launch_reduce_partials(kappa_partial, kappa_blocks, 1, ds, c->stream));
          if (native_allreduce_dev(c->native_comm, ds, 1)) return fail(c, CORA_ERR_HIP, "all-reduce step failed: " + native_error(c->native_comm));
          HIP_TRY(c, launch_stpcg_scalar_step(0, ds, c->d_stpcg, nullptr, nullptr, 0, c->stream));
          if (sweep_fused) {
            // the sweep-fused form on this rank's block-Jacobi factor: forward sweep (r += alpha Hp, slots of <r, r> and
            // |y|^2) | last stage, whose tail block leaves this rank's <r, r> and <r, v> = |L_k^-1 r_k|^2 | ONE all-reduce
            // for the two | scalar step | backward sweep (v = Proj_Y(x), s += alpha p, p = -v + beta p).  Three vector
            // passes fewer than the form below, the same two all-reduces per iteration.
            cora_ctx::DevFactor &f = c->precond_f;
            double *t, *t2;
            if ((rc = get_scratch(c, 6, c->ld, &t, f.aux_rows))) return rc;
            if ((rc = get_scratch(c, 7, c->ld, &t2))) return rc;
            const cora_ctx::DevStage &S0 = f.stages[0], &S1 = f.stages[1];
            HIP_TRY(c, launch_subblock_fused(S0.sub, c->ld, false, FF, t, dV, c->stream));
            if (S1.aux_sum) HIP_TRY(c, launch_rowop(S1.fwd_a, c->ld, t, t, t, c->stream));
            HIP_TRY(c, launch_rowop(S1.fwd_b, c->ld, nullptr, t, t2, c->stream, &sq));
            tail.sums_out = ds + 2;
            HIP_TRY(c, launch_rowop(S1.bwd_b, c->ld, nullptr, t2, t, c->stream, &tail));
            if (native_allreduce_dev(c->native_comm, ds + 2, 2)) return fail(c, CORA_ERR_HIP, "all-reduce step failed: " + native_error(c->native_comm));
            seq = ++c->dot_seq;
            HIP_TRY(c, launch_stpcg_scalar_step(1, ds + 2, c->d_stpcg, &c->h_stpcg[0],
                                                reinterpret_cast<unsigned long long *>(c->h_scalars + 7), seq, c->stream));
            HIP_TRY(c, launch_subblock_fused(S0.sub, c->ld, true, FB, t, dV, c->stream));
            return CORA_OK;
          }
          DotArgs Ds = D;
          Ds.mode = DOTS_PLAIN;
          Ds.count = 1;
          Ds.seq_out = nullptr;
          Ds.seq = 0;
          Ds.out = ds + 2;
          HIP_TRY(c, launch_stpcg_residual(Ds, n, dHp + off, dR + off, c->stream));
          Ds.out = ds + 3;
          const double *xs = dR;  // what is projected: r (none), D^-1 r (Jacobi, scaled in the pass), or the rank's own
          if (chol) {             // Cholesky solve of its diagonal block (block Jacobi over the ranks)
            if ((rc = chol_solve(c, c->ld, dR, dV))) return rc;
            xs = dV;
          }
          HIP_TRY(c, launch_tangent_project_dot(row_args(c), Ds, c->ld, c->d_Y, xs, c->precond == CORA_PRECOND_JACOBI ? c->d_diag_inv : nullptr,
                                                dR, dV, c->stream));
          if (native_allreduce_dev(c->native_comm, ds + 2, 2)) return fail(c, CORA_ERR_HIP, "all-reduce step failed: " + native_error(c->native_comm));
          seq = ++c->dot_seq;
          HIP_TRY(c, launch_stpcg_scalar_step(1, ds + 2, c->d_stpcg, &c->h_stpcg[0],
                                              reinterpret_cast<unsigned long long *>(c->h_scalars + 7), seq, c->stream));
          HIP_TRY(c, launch_stpcg_step_direction(n, c->d_stpcg, dV + off, dP + off, dS + off, c->stream));
          return CORA_OK;
        }
        if (sweep_fused) {
          if (FF.n_kappa == 0) HIP_TRY(c, launch_kappa_finish(kappa_partial, kappa_blocks, c->d_stpcg, c->stream));
          mark(2);
          // Hp = H p | kappa | forward sweep: r += alpha Hp, <r, r>, |y|^2 | last stage, <r, v> in its second product |
          // backward sweep: v = Proj_Y(x), s += alpha p, p = -v + beta p   -- six launches
          cora_ctx::DevFactor &f = c->precond_f;
          double *t, *t2;
          if ((rc = get_scratch(c, 6, c->ld, &t, f.aux_rows))) return rc;
          if ((rc = get_scratch(c, 7, c->ld, &t2))) return rc;
          const cora_ctx::DevStage &S0 = f.stages[0], &S1 = f.stages[1];
          HIP_TRY(c, launch_subblock_fused(S0.sub, c->ld, false, FF, t, dV, c->stream));
          mark(3);
          if (S1.aux_sum) HIP_TRY(c, launch_rowop(S1.fwd_a, c->ld, t, t, t, c->stream));
          HIP_TRY(c, launch_rowop(S1.fwd_b, c->ld, nullptr, t, t2, c->stream, &sq));
          mark(4);
          tail.seq = seq = ++c->dot_seq;
          HIP_TRY(c, launch_rowop(S1.bwd_b, c->ld, nullptr, t2, t, c->stream, &tail));
          mark(5);
          HIP_TRY(c, launch_subblock_fused(S0.sub, c->ld, true, FB, t, dV, c->stream));
          mark(6);
          mark(7);  // (two marks with nothing between them: what a mark itself costs the stream)
          return CORA_OK;
        }
        // kappa, the scalar step and r += alpha Hp with <r, r> in ONE launch (every block adds the partials: the plans
        // that come here are small, and a launch is what costs them)
        if (inverse_fused && tail.n_rr > 0)
          HIP_TRY(c, launch_kappa_residual_slots(c->d_stpcg, kappa_partial, kappa_blocks, n, dHp + off, dR + off,
                                                 const_cast<double *>(tail.rr_partial), c->stream));
        else
          HIP_TRY(c, launch_kappa_residual(D, kappa_partial, kappa_blocks, n, dHp + off, dR + off, c->stream));
        if (inverse_fused) {
          // one explicit inverse (every data set of the reference): v = Proj_Y(W^T W r) and <r, v> = |W r|^2 -- the first
          // product leaves the squared norms of its rows, an extra block of the second adds them and runs the scalar step,
          // and the projection consumes v at once (s += alpha p, p = -v + beta p): five launches per iteration
          cora_ctx::DevFactor &f = c->precond_f;
          double *t2;
          if ((rc = get_scratch(c, 7, c->ld, &t2))) return rc;
          const cora_ctx::DevStage &S = f.stages[0];
          HIP_TRY(c, launch_rowop(S.fwd_b, c->ld, nullptr, dR, t2, c->stream, &sq));
          tail.seq = seq = ++c->dot_seq;
          HIP_TRY(c, launch_rowop(S.bwd_b, c->ld, nullptr, t2, dV, c->stream, &tail));
          HIP_TRY(c, launch_tangent_project_update(row_args(c), c->d_stpcg, c->ld, c->d_Y, dV, dP, dS, c->stream));
          return CORA_OK;
        }
        const double *x = dR, *scale = nullptr;
        if (chol) {
          if ((rc = chol_solve(c, c->ld, dR, dV))) return rc;
          x = dV;
        } else if (c->precond == CORA_PRECOND_JACOBI) {
          scale = c->d_diag_inv;
        }
        D.mode = DOTS_STPCG_RV;
        D.count = 1;
        D.seq_out = reinterpret_cast<unsigned long long *>(c->h_scalars + 7);
        D.seq = seq = ++c->dot_seq;
        HIP_TRY(c, launch_tangent_project_dot(row_args(c), D, c->ld, c->d_Y, x, scale, dR, dV, c->stream));
        HIP_TRY(c, launch_stpcg_step_direction(n, c->d_stpcg, dV + off, dP + off, dS + off, c->stream));
        D.seq_out = nullptr;
        D.seq = 0;
        return CORA_OK;
      }
      if (part != 2 && (rc = apply_product(c, dP, c->ld, EPI_HVP, dHp))) return rc;
      if (part == 1) return CORA_OK;
      mark(1);
      int nblocks = 0;
      D.count = 1;
      D.a[0] = dP;
      D.b[0] = dHp;
      D.mode = DOTS_STPCG_KAPPA;
      D.seq_out = nullptr;
      D.seq = 0;
      HIP_TRY(c, launch_dots(D, &nblocks, c->stream));
      HIP_TRY(c, launch_stpcg_update(n, c->d_stpcg, dP, dHp, dS, dR, c->stream));
      if ((rc = cora_precondition_projected_dev(c, dR, dV))) return rc;
      D.count = 2;
      D.a[0] = dR;
      D.b[0] = dR;
      D.a[1] = dR;
      D.b[1] = dV;
      D.mode = DOTS_STPCG_BETA;
      D.seq_out = reinterpret_cast<unsigned long long *>(c->h_scalars + 7);
      D.seq = seq = ++c->dot_seq;
      HIP_TRY(c, launch_dots(D, &nblocks, c->stream));
      HIP_TRY(c, launch_stpcg_direction(n, c->d_stpcg, dV, dP, c->stream));
      return CORA_OK;
    };
    if (product_ahead) {
      if (!have_product && (rc = one_iteration(1))) return rc;
      if ((rc = one_iteration(2))) return rc;
      ++enqueued;
      have_product = enqueued < max_iters;
      if (have_product && (rc = one_iteration(1))) return rc;
      if ((rc = wait_dots(c, seq))) return rc;
      std::atomic_thread_fence(std::memory_order_acquire);
      continue;
    }
    if (pipelined) {
      if ((rc = one_iteration())) return rc;
      ++enqueued;
      in_flight.push_back(seq);
      if (static_cast<int>(in_flight.size()) > depth) {
        if ((rc = wait_dots(c, in_flight.front()))) return rc;
        in_flight.pop_front();
        std::atomic_thread_fence(std::memory_order_acquire);
      }
      continue;
    }
    for (int b = 0; b < batch && enqueued < max_iters; ++b, ++enqueued) {
      if ((rc = one_iteration())) {
        (void)end_capture(false);
        return rc;
      }
    }
    if ((rc = end_capture(true))) return rc;
    if ((rc = wait_dots(c, seq))) return rc;
  }
  if (c->h_stpcg[0].status == 0 || c->prof_stpcg) {  // the iteration limit ended the loop: what is in flight decides
    while (!in_flight.empty()) {
      if ((rc = wait_dots(c, in_flight.front()))) return rc;
      in_flight.pop_front();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  if (c->h_stpcg[0].status != 0 && !c->prof_stpcg) {
    // Whole-iteration-ahead forms (CORA_STPCG_DEPTH >= 1 / CORA_STPCG_AHEAD=0: lab switches): the host has only waited for
    // iteration k - 1, so the status it has just seen may come from iteration k, whose tail block can still be writing
    // the mirror -- a plain struct store over PCIe: it is waited for before the mirror is copied (round-5 advice: a torn
    // iters / step_M_norm).  The default product-ahead form has only a product in flight, which writes nothing here.
    if (pipelined && !product_ahead) {
      while (!in_flight.empty()) {
        if ((rc = wait_dots(c, in_flight.front()))) return rc;
        in_flight.pop_front();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    // the mirror was written by the iteration that set the status (and only rewritten with the same iteration count,
    // step norm and status by a neutral one after it): final, nothing to wait for.  What is still in flight is
    // neutral and ordered before anything enqueued after this call; the next solve makes sure of it before it resets the mirror.
    H = c->h_stpcg[0];
    c->stpcg_pending_seq = in_flight.empty() ? 0 : in_flight.back();
  } else {
    // an iteration that starts at the limit only records the status: flush it so that the mirror is final
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(&H, c->d_stpcg, sizeof(StpcgState), hipMemcpyDeviceToHost));
  }
  if (c->prof_stpcg) {  // iterations that really ran (enqueued-ahead ones after the stop are neutral but timed)
    const bool phases = c->prof_stpcg >= 2 && c->stpcg_path == 2 && !sharded;
    for (int k = 0; k < 7; ++k) c->prof_phase_us[k] = -1.0;
    const bool tail_marks = c->stpcg_path == 2 && !sharded;  // (marks 6 and 7 exist on the sweep-fused form)
    for (int k = 0; k < 7; ++k) {
      if (!(k == 0 || phases || (k == 6 && tail_marks))) continue;
      double tot = 0.0;
      int cnt = 0;
      for (int i = 0; i < H.iters && kProfMarks * (static_cast<size_t>(i) + 1) <= c->prof_events.size(); ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->prof_events[kProfMarks * i + k], c->prof_events[kProfMarks * i + k + 1]) == hipSuccess) {
          tot += ms * 1e3;
          ++cnt;
        }
      }
      c->prof_phase_us[k] = cnt ? tot / cnt : -1.0;
      if (k == 0) {
        c->prof_hvp_us = cnt ? tot / cnt : 0.0;
        c->prof_hvp_count = cnt;
      }
    }
  }
  *iters = H.iters;
  *step_M_norm = H.step_M_norm;
  return CORA_OK;
}

int cora_stpcg_dev(cora_ctx *c, const double *dGrad, double Delta, double kappa_fgr, double theta, int max_iters,
                   double *dS, double *dR, double *dV, double *dP, double *dHp, int *iters, double *step_M_norm) {
  return stpcg_run(c, dGrad, nullptr, 0.0, 0.0, Delta, kappa_fgr, theta, max_iters, dS, dR, dV, dP, dHp, iters, step_M_norm);
}

int cora_stpcg_warm_dev(cora_ctx *c, const double *dGrad, const double *dPg, double g_g, double g_Pg, double Delta,
                        double kappa_fgr, double theta, int max_iters, double *dS, double *dR, double *dV, double *dP,
                        double *dHp, int *iters, double *step_M_norm) {
  if (!c || !dPg || dPg == dS || dPg == dR || dPg == dV || dPg == dP || dPg == dHp) return fail(c, CORA_ERR_ARG, "bad arguments");
  return stpcg_run(c, dGrad, dPg, g_g, g_Pg, Delta, kappa_fgr, theta, max_iters, dS, dR, dV, dP, dHp, iters, step_M_norm);
}

int cora_set_comm(cora_ctx *c, cora_exchange_fn exchange, cora_allreduce_fn allreduce, cora_allgather_fn allgather,
                  void *user) {
  if (!c) return CORA_ERR_ARG;
  c->comm_exchange = exchange;
  c->comm_allreduce = allreduce;
  c->comm_allgather = allgather;
  c->comm_user = user;
  return CORA_OK;
}

int cora_stpcg_device_ok(const cora_ctx *c) { return (c && c->has_device && c->p > 0 && stpcg_device_ok(c)) ? 1 : 0; }

int cora_require_comm(cora_ctx *c, int on) {
  if (!c) return CORA_ERR_ARG;
  c->comm_required = on != 0;
  return CORA_OK;
}

int cora_rank(const cora_ctx *c) { return c ? c->F.L.rank : 0; }
int cora_world(const cora_ctx *c) { return c ? c->F.L.world : 0; }
