// Part of capi.hip (one translation unit; included there, in this order).  preconditioner: Jacobi / Cholesky set-up, installation of a host factor as a device solve plan, the staged solve.
int cora_precond_setup(cora_ctx *c, int kind) {
  if (!c) return CORA_ERR_ARG;
  if (kind == CORA_PRECOND_NONE || kind == CORA_PRECOND_JACOBI) {
    if (kind == CORA_PRECOND_JACOBI && c->host_values_stale) {
      // (cora_update_values_dev: the diagonal the device holds is newer than F.diag -- a zero shows as an infinite reciprocal)
      HIP_TRY(c, hipSetDevice(c->device));
      std::vector<double> dinv(c->F.diag.size());
      HIP_TRY(c, hipMemcpy(dinv.data(), c->d_diag_inv, dinv.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (double v : dinv)
        if (!std::isfinite(v)) return fail(c, CORA_ERR_NAN, "zero on the diagonal of Q: Jacobi preconditioner undefined");
    } else if (kind == CORA_PRECOND_JACOBI) {
      for (double v : c->F.diag)
        if (!(v != 0.0)) return fail(c, CORA_ERR_NAN, "zero on the diagonal of Q: Jacobi preconditioner undefined");
    }
    c->precond = kind;
    return CORA_OK;
  }
  if (kind == CORA_PRECOND_BLOCK_CHOLESKY || kind == CORA_PRECOND_REGULARIZED_CHOLESKY) {
    if (!c->precond_f.ready)
      return fail(c, CORA_ERR_NOT_READY,
                  "Cholesky preconditioners need a factor installed with cora_precond_set_cholesky");
    c->precond = kind;
    return CORA_OK;
  }
  return fail(c, CORA_ERR_ARG, "unknown preconditioner kind");
}

// cora_precond_entries: counted from the plan as built (before the image appends the over-read tails to its arrays)
static void plan_entries(const TriPlan &plan, int64_t e[6]) {
  std::fill(e, e + 6, int64_t{0});
  if (plan.stages.empty()) return;
  const TriStage &top = plan.stages.back();
  e[0] = static_cast<int64_t>(top.fwd_b.val.size());
  e[1] = static_cast<int64_t>(top.bwd_b.val.size());
  if (!plan.stages[0].sub) return;
  const SubBlockOpHost &o = plan.stages[0].sub_op;
  e[2] = static_cast<int64_t>(o.f_val.size());
  e[3] = static_cast<int64_t>(o.b_val.size());
  e[4] = static_cast<int64_t>(o.nrows.size());
  e[5] = o.n_aux;
}

// Installs a host factor as a device solve plan: the plan (build_tri_plan), its device image (build_tri_image), both
// uploaded through the factor's arena (walk_tri_image).  row_of[i] = internal row of permuted variable i.
static int install_factor(cora_ctx *c, cora_ctx::DevFactor &f, int m, const int32_t *Lp, const int32_t *Li,
                          const double *Lx, const std::vector<int32_t> &row_of, int32_t zero_row,
                          const std::vector<int32_t> *group = nullptr) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  cora::PhaseTimer tick(cora::env_flag(cora::Env::TriTiming), "  [install]", 26, 3);
  f.arena.rewind();
  f.stages.clear();
  f.ready = false;
  f.aux_rows = 0;
  f.fuse_ok = false;
  const Layout &L = c->F.L;
  TriPlan plan;
  TriImage image;
  try {
    build_tri_plan(m, Lp, Li, Lx, row_of, zero_row, plan, group, static_cast<int32_t>(L.rows));
    tick("plan (host)");
    plan_entries(plan, f.entries);
    build_tri_image(plan, ImageLayout{L.d, L.rot_base, L.rot_base + static_cast<int64_t>(L.d) * L.nl_poses, L.rows, group != nullptr},
                    image, tick);
  } catch (const std::exception &e) {
    return fail(c, CORA_ERR_ARG, e.what());
  }
  tri_image_shape(plan, image, f.shape);
  walk_tri_image(f.arena, plan, image, f.stages);
  HIP_TRY(c, f.arena.error);
  for (size_t k = 0; k < f.stages.size(); ++k) {
    const StageImage &I = image.stages[k];
    cora_ctx::DevStage &D = f.stages[k];
    D.has_fwd_a = I.has_fwd_a, D.has_bwd_a = I.has_bwd_a, D.dense = I.dense, D.is_sub = I.is_sub, D.aux_sum = I.aux_sum;
  }
  f.aux_rows = image.aux_rows;
  f.fuse_ok = image.fuse_ok;
  tick("upload");
  if (!plan.stages.empty() && plan.stages[0].sub) {
    // the substitution arrays are not needed any more: 130 MB of vectors, 16 ms to hand back at 10^5 poses and 0.1 s at
    // 10^6 -- on a thread of its own (joined before the next factor is installed and when the handle goes), started AFTER
    // the last stage's uploads: a thread that unmaps 130 MB holds the address space's lock, and the next copy from
    // pageable memory waited 12 ms for it (measured: a 2.3 MB copy, 0.0122 s)
    auto dead = std::make_shared<SubBlockOpHost>(std::move(plan.stages[0].sub_op));
    if (c->deferred_free.valid()) c->deferred_free.get();
    c->deferred_free = std::async(std::launch::async, [dead = std::move(dead)]() mutable { dead.reset(); });
  }
  image = TriImage();  // (the rest of the host copy goes here, inside the install's reported time)
  plan = TriPlan();
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  tick("host copy dropped");
  f.ready = true;
  ++f.generation;
  f.shape[kShapeGeneration] = static_cast<int64_t>(f.generation);
  return CORA_OK;
}

int cora_debug_factor_shape(const cora_ctx *c, int which, int64_t out[24]) {
  if (!c || !out || which < 0 || which > 2) return CORA_ERR_ARG;
  const cora_ctx::DevFactor &f = which == 0 ? c->precond_f : (which == 1 ? c->implicit_f : c->aux_f);
  if (!f.ready) return fail(const_cast<cora_ctx *>(c), CORA_ERR_NOT_READY, "no factor installed");
  static_assert(kShapeFields == 24, "include/cora_hip.h documents 24 fields");
  std::copy(f.shape, f.shape + kShapeFields, out);
  return CORA_OK;
}

// out[rows of the factor] = (P^T L L^T P)^-1 rhs[rows of the factor]; rows outside the factor are not
// written.  rhs and out must be different resident vectors.  A fixed sequence of 4K-2 sparse products
// (trisolve.h): forward stages ascending, backward stages descending.
// project != nullptr (two-stage plans that allow it): the solution leaves the backward sweep projected to the tangent
// space of the current point (SubFuse with p == nullptr) and *project is set; otherwise the caller projects.
static int factor_solve(cora_ctx *c, cora_ctx::DevFactor &f, int ld, const double *rhs, double *out, bool *project = nullptr) {
  if (project) *project = false;
  if (rhs == out) return fail(c, CORA_ERR_ARG, "factor_solve: output aliases the right-hand side");
  const int K = static_cast<int>(f.stages.size());
  if (K == 0) return CORA_OK;
  double *t, *t2;
  int rc;
  if ((rc = get_scratch(c, 6, ld, &t, f.aux_rows))) return rc;
  if ((rc = get_scratch(c, 7, ld, &t2))) return rc;
  if (f.stages[0].is_sub) {  // two-stage plan: substitution blocks around one explicit inverse (trisolve.h)
    const cora_ctx::DevStage &S0 = f.stages[0], &S1 = f.stages[1];
    HIP_TRY(c, launch_subblock(S0.sub, ld, false, rhs, t, out, c->stream));  // y_0 -> out, couplings + rhs_1 -> t
    if (S1.aux_sum) HIP_TRY(c, launch_rowop(S1.fwd_a, ld, t, t, t, c->stream));  // t_1 += its aux rows (in place: a row is read and written by its own lanes only)
    HIP_TRY(c, launch_rowop(S1.fwd_b, ld, nullptr, t, t2, c->stream));       // y_1 = W_1 t_1 (with the aux sums folded in otherwise)
    HIP_TRY(c, launch_rowop(S1.bwd_b, ld, nullptr, t2, t, c->stream));       // x_1 = W_1^T y_1 -> t
    if (project && f.fuse_ok && ld * c->F.L.d <= 24 && ld <= 12 && c->have_point) {
      const Layout &L = c->F.L;
      SubFuse FB;
      FB.dot.st = c->d_stpcg;  // (coefficients unused in this mode)
      FB.Y = c->d_Y;
      FB.d = L.d;
      FB.rot_base = L.rot_base;
      FB.rng_base = L.rng_base;
      FB.trn_base = L.trn_base;
      HIP_TRY(c, launch_subblock_fused(S0.sub, ld, true, FB, t, out, c->stream));  // Proj_Y(x) -> out
      *project = true;
      return CORA_OK;
    }
    HIP_TRY(c, launch_subblock(S0.sub, ld, true, out, t, out, c->stream));   // x_0, and x_1 -> out
    return CORA_OK;
  }
  for (int k = 0; k < K; ++k) {  // L y = rhs
    const cora_ctx::DevStage &S = f.stages[k];
    if (S.dense) {  // stage 0, never the last one
      HIP_TRY(c, launch_blockop(S.blocks, ld, false, rhs, out, c->stream));
      continue;
    }
    const double *tk = rhs;
    if (S.has_fwd_a) {
      HIP_TRY(c, launch_rowop(S.fwd_a, ld, rhs, out, t, c->stream));   // t_k = rhs_k - L[k,<k] y_<k
      tk = t;
    }
    HIP_TRY(c, launch_rowop(S.fwd_b, ld, nullptr, tk, k == K - 1 ? t2 : out, c->stream));  // y_k = W_k t_k
  }
  for (int k = K - 1; k >= 0; --k) {  // L^T x = y
    const cora_ctx::DevStage &S = f.stages[k];
    if (S.dense) {
      HIP_TRY(c, launch_blockop(S.blocks, ld, true, out, out, c->stream));
      continue;
    }
    const double *tk = t2;  // last stage: y_K-1 was left in t2
    if (S.has_bwd_a) {
      HIP_TRY(c, launch_rowop(S.bwd_a, ld, out, out, t, c->stream));   // t_k = y_k - L[>k,k]^T x_>k
      tk = t;
    }
    HIP_TRY(c, launch_rowop(S.bwd_b, ld, nullptr, tk, out, c->stream));  // x_k = W_k^T t_k
  }
  return CORA_OK;
}

int cora_precond_set_cholesky(cora_ctx *c, int m, const int32_t *Lp, const int32_t *Li, const double *Lx,
                              const int32_t *perm) {
  NEED_DEVICE(c);
  const int64_t N = c->F.L.N;
  const Layout &Lo = c->F.L;
  // Partitioned handle: the factor is the one of THIS RANK'S rows -- the diagonal block of (Q + lambda I) on the rows
  // of its shard, all of them or all but one (the pinned variable, if it lives here): block Jacobi over the ranks.
  const bool sharded = Lo.world != 1;
  const int64_t owned = sharded ? Lo.local_rows : N;
  if (!Lp || !Li || !Lx || !perm || (m != owned && m != owned - 1))
    return fail(c, CORA_ERR_ARG, sharded ? "factor must cover the rank's own rows (all, or all but the pinned one)"
                                         : "factor must have N or N-1 rows");
  std::vector<int32_t> row_of(static_cast<size_t>(m));
  std::vector<char> seen(static_cast<size_t>(N), 0);
  for (int i = 0; i < m; ++i) {
    if (perm[i] < 0 || perm[i] >= N || seen[perm[i]]) return fail(c, CORA_ERR_ARG, "perm is not a permutation");
    seen[perm[i]] = 1;
    row_of[i] = c->F.api2int[perm[i]];
    if (sharded && (row_of[i] < Lo.base || row_of[i] >= Lo.base + Lo.shard_rows))
      return fail(c, CORA_ERR_ARG, "the factor of a partitioned handle may only hold rows of its own shard");
  }
  int32_t zero_row = -1;  // blockCholeskySolve: last row zeroed, src/CORA_preconditioners.cpp:78-79
  if (m == owned - 1)
    for (int64_t i = 0; i < N; ++i) {
      const int32_t ir = c->F.api2int[i];
      if (!seen[i] && (!sharded || (ir >= Lo.base && ir < Lo.base + Lo.shard_rows))) zero_row = ir;
    }
  // the d rotation rows of a pose stay in one block of the solve plan (row-unit work can then be fused into it)
  std::vector<int32_t> group(static_cast<size_t>(m), -1);
  const int64_t dn = static_cast<int64_t>(c->F.L.d) * c->F.L.n;
  for (int i = 0; i < m; ++i)
    if (perm[i] < dn) group[i] = perm[i] / c->F.L.d;
  return install_factor(c, c->precond_f, m, Lp, Li, Lx, row_of, zero_row, &group);
}

// dOut = [ (Q + lambda I)[0:m]^-1 V[0:m] ; 0 ]
static int chol_solve(cora_ctx *c, int ld, const double *dV, double *dOut) {
  return factor_solve(c, c->precond_f, ld, dV, dOut);  // the pinned row is zeroed by the plan itself
}

// ---- translation-implicit formulation (src/CORA_problem.cpp:714-753) ------------------------
// Q_impl Y = Qmain Y - B M^-1 B^T Y with M = Q33[0:nt-1] = top rows of Q [Y; t; 0] for
// t = -M^-1 (B^T Y), and B^T Y = translation rows of Q [Y; 0].  Two explicit products and
// one triangular solve on the translation block; vectors keep N rows, translation rows of the
// input are ignored and translation rows of the output are zero.
// Partitioned handle: the two products are the partitioned products (one exchange of the operand each); the translation
// solve in between is a recurrence over the whole chain, so it is REPLICATED -- the right-hand side's rows are gathered
// (whole shards in place: one collective) and every rank runs the same solve plan on the same numbers, then keeps its
// own translations (and already holds the remote ones the second product reads).  Exact: the operator is the single
// handle's, whatever the partition.
static int64_t pinned_translation_row(const cora_ctx *c) { return c->F.api2int[static_cast<size_t>(c->F.L.N) - 1]; }
