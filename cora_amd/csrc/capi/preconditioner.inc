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

// Builds the level schedule of a factor and uploads it.  row_of[i] = internal row of permuted variable i.
static int install_factor(cora_ctx *c, cora_ctx::DevFactor &f, int m, const int32_t *Lp, const int32_t *Li,
                          const double *Lx, const std::vector<int32_t> &row_of, int32_t zero_row,
                          const std::vector<int32_t> *group = nullptr) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  cora::PhaseTimer tick(cora::env_flag(cora::Env::TriTiming), "  [install]", 26, 3);
  f.chunk_at = 0;
  f.chunk_used = 0;
  f.stages.clear();
  f.ready = false;
  f.aux_rows = 0;
  f.fuse_ok = false;
  try {
    build_tri_plan(m, Lp, Li, Lx, row_of, zero_row, f.plan, group, static_cast<int32_t>(c->F.L.rows));
  } catch (const std::exception &e) {
    return fail(c, CORA_ERR_ARG, e.what());
  }
  tick("plan (host)");
  tri_plan_shape(f.plan, f.shape);
  auto up = [&](auto **dst, const auto &vec) -> hipError_t {
    using T = typename std::remove_reference<decltype(vec)>::type::value_type;
    const size_t bytes = (std::max<size_t>(vec.size(), 1) * sizeof(T) + 255) & ~static_cast<size_t>(255);
    while (f.chunk_at < f.allocs.size() && f.chunk_used + bytes > f.chunk_bytes[f.chunk_at]) {
      ++f.chunk_at;
      f.chunk_used = 0;
    }
    if (f.chunk_at == f.allocs.size()) {
      const size_t cb = std::max<size_t>(bytes, static_cast<size_t>(64) << 20);
      void *q = nullptr;
      const hipError_t e = hipMalloc(&q, cb);
      if (e != hipSuccess) return e;
      f.allocs.push_back(q);
      f.chunk_bytes.push_back(cb);
      f.chunk_used = 0;
    }
    T *p = reinterpret_cast<T *>(static_cast<char *>(f.allocs[f.chunk_at]) + f.chunk_used);
    f.chunk_used += bytes;
    *dst = p;
    if (vec.empty()) return hipSuccess;
    return hipMemcpy(p, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice);  // (vec may be a temporary)
  };
  auto up_op = [&](RowOpDev &D, RowOpHost &H) -> hipError_t {
    hipError_t e;
    D.n8 = H.n8;
    D.n64 = H.n64;
    D.nlong = static_cast<int>(H.long_out.size());
    D.nchunks = static_cast<int>(H.chunk_begin.size());
    if ((e = up(&D.out_row, H.out_row)) != hipSuccess) return e;
    if ((e = up(&D.begin, H.begin)) != hipSuccess) return e;
    if ((e = up(&D.end, H.end)) != hipSuccess) return e;
    if ((e = up(&D.long_out, H.long_out)) != hipSuccess) return e;
    if ((e = up(&D.long_chunk_ptr, H.long_chunk_ptr)) != hipSuccess) return e;
    if ((e = up(&D.chunk_begin, H.chunk_begin)) != hipSuccess) return e;
    if ((e = up(&D.chunk_end, H.chunk_end)) != hipSuccess) return e;
    if ((e = up(&D.col, H.col)) != hipSuccess) return e;
    if ((e = up(&D.val, H.val)) != hipSuccess) return e;
    std::vector<int32_t> chunk_row(static_cast<size_t>(D.nchunks), 0);
    for (int r = 0; r < D.nlong; ++r)
      for (int32_t ch = H.long_chunk_ptr[r]; ch < H.long_chunk_ptr[r + 1]; ++ch) chunk_row[ch] = r;
    if ((e = up(&D.chunk_row, chunk_row)) != hipSuccess) return e;
    const std::vector<unsigned> tick(static_cast<size_t>(std::max(D.nlong, 1)), 0u);
    const unsigned *tp = nullptr;
    if ((e = up(&tp, tick)) != hipSuccess) return e;
    D.tickets = const_cast<unsigned *>(tp);
    const std::vector<double> part(static_cast<size_t>(std::max(D.nchunks, 1)) * kMaxLD, 0.0);
    const double *pp = nullptr;
    if ((e = up(&pp, part)) != hipSuccess) return e;
    D.partial = const_cast<double *>(pp);
    H = RowOpHost();  // the host copy is not needed any more
    return hipSuccess;
  };
  const size_t K = f.plan.stages.size();
  f.stages.resize(K);
  std::shared_ptr<SubBlockOpHost> dead_sub;
  for (int64_t &e : f.entries) e = 0;
  if (K > 0) {
    const TriStage &top = f.plan.stages.back();
    f.entries[0] = static_cast<int64_t>(top.fwd_b.val.size());
    f.entries[1] = static_cast<int64_t>(top.bwd_b.val.size());
    if (f.plan.stages[0].sub) {
      const SubBlockOpHost &o = f.plan.stages[0].sub_op;
      f.entries[2] = static_cast<int64_t>(o.f_val.size());
      f.entries[3] = static_cast<int64_t>(o.b_val.size());
      f.entries[4] = static_cast<int64_t>(o.nrows.size());
      f.entries[5] = o.n_aux;
    }
  }
  for (size_t k = 0; k < K; ++k) {
    TriStage &S = f.plan.stages[k];
    cora_ctx::DevStage &D = f.stages[k];
    D.has_fwd_a = k > 0;
    D.has_bwd_a = k + 1 < K;
    D.dense = S.dense;
    if (S.sub) {
      SubBlockOpHost &H = S.sub_op;
      D.is_sub = true;
      std::vector<SubDesc> desc(H.nrows.size());
      for (size_t b = 0; b < desc.size(); ++b) {
        SubDesc &d = desc[b];
        d.row_begin = H.row_begin[b];
        d.nrows = H.nrows[b];
        d.f_ent_begin = H.f_ent_begin[b];
        d.f_nent = H.f_nent[b];
        d.b_ent_begin = H.b_ent_begin[b];
        d.b_nent = H.b_nent[b];
        d.f_lev_begin = H.f_lev_begin[b];
        d.f_nlev = (H.f_lev_begin[b + 1] - H.f_lev_begin[b]) / 4 - 1;  // barrier levels: one header per wavefront (4) each, + the closing one
        d.b_lev_begin = H.b_lev_begin[b];
        d.b_nlev = (H.b_lev_begin[b + 1] - H.b_lev_begin[b]) / 4 - 1;
        d.tgt_begin = H.tgt_begin[b];
        d.ntgt = H.tgt_begin[b + 1] - H.tgt_begin[b];
      }
      SubOpDev &Q = D.sub;
      Q.nblocks = static_cast<int>(desc.size());
      Q.ntop = static_cast<int>(f.plan.top_rows.size());
      Q.max_rows = H.max_rows;
      Q.max_ent = H.max_ent;
      Q.max_lev = H.max_lev;
      Q.max_level_lanes = H.max_level_lanes;
      Q.max_npl = H.max_npl;
      Q.aux_base = f.plan.aux_base;
      HIP_TRY(c, up(&Q.fwd.rows, H.rows));
      H.f_hdr.resize(H.f_hdr.size() + 8, 0);  // the kernel reads one header ahead
      H.f_idx.resize(H.f_idx.size() + 8, 0);  // ... and an entry past a block without entries
      H.f_val.resize(H.f_val.size() + 8, 0.0);
      H.b_idx.resize(H.b_idx.size() + 8, 0);
      H.b_val.resize(H.b_val.size() + 8, 0.0);
      H.b_hdr.resize(H.b_hdr.size() + 8, 0);
      HIP_TRY(c, up(&Q.fwd.hdr, H.f_hdr));
      HIP_TRY(c, up(&Q.fwd.idx, H.f_idx));
      HIP_TRY(c, up(&Q.fwd.val, H.f_val));
      HIP_TRY(c, up(&Q.bwd.rows, H.b_rows));
      HIP_TRY(c, up(&Q.bwd.hdr, H.b_hdr));
      HIP_TRY(c, up(&Q.bwd.idx, H.b_idx));
      HIP_TRY(c, up(&Q.bwd.val, H.b_val));
      HIP_TRY(c, up(&Q.tgt_row, H.tgt_row));
      HIP_TRY(c, up(&Q.tgt_slot, H.tgt_slot));
      HIP_TRY(c, up(&Q.c_ptr, H.c_ptr));
      HIP_TRY(c, up(&Q.c_idx, H.c_idx));
      HIP_TRY(c, up(&Q.c_val, H.c_val));
      HIP_TRY(c, up(&Q.top_rows, f.plan.top_rows));
      f.aux_rows = H.n_aux;
      tick("  sub: desc + arrays");
      {
        // memory-order I/O lists of both sweeps: {internal row, tile position} of every block row, sorted by row
        auto io_of = [&](const std::vector<int32_t> &rows) {
          std::vector<int2> io(rows.size() + 1);  // (+ 1: a block without rows still forms an address)
          const size_t nblk = desc.size();
          const unsigned nth = nblk < 64 ? 1u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
          auto part = [&](unsigned t) {  // blocks are independent: a range of them per thread
            std::vector<int32_t> ord;
            for (size_t b = nblk * t / nth; b < nblk * (t + 1) / nth; ++b) {
              const int32_t r0 = desc[b].row_begin, nb = desc[b].nrows;
              ord.resize(static_cast<size_t>(nb));
              for (int k = 0; k < nb; ++k) ord[k] = k;
              std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return rows[r0 + x] < rows[r0 + y]; });
              for (int k = 0; k < nb; ++k) io[static_cast<size_t>(r0) + k] = make_int2(rows[r0 + ord[k]], ord[k]);
            }
          };
          cora::parallel_parts(nth, part);
          io.back() = make_int2(0, 0);
          return io;
        };
        // (the rows of a block in memory order are the same set for both sweeps: the runs are found once, from the
        // forward list; only the tile positions differ)
        {
          const std::vector<int2> iof = io_of(H.rows), iob = io_of(H.b_rows);
          bool runs_ok = !cora::env_flag(cora::Env::SubIoLists);  // (lab switch: the 8-byte index lists)
          std::vector<uint16_t> tpf(iof.size() + 8, 0), tpb(iob.size() + 8, 0);
          for (size_t b = 0; b < desc.size(); ++b) {
            SubDesc &d = desc[b];
            const int32_t r0 = d.row_begin, nb = d.nrows;
            int nr = 0;
            for (int q = 0; q < kSubMaxRuns; ++q) { d.run_off[q] = 0; d.run_end[q] = INT32_MAX; }
            for (int k = 0; k < nb; ++k) {
              const int2 a = iof[static_cast<size_t>(r0) + k], bb = iob[static_cast<size_t>(r0) + k];
              if (a.x != bb.x || a.y > 0xffff || bb.y > 0xffff) runs_ok = false;
              tpf[static_cast<size_t>(r0) + k] = static_cast<uint16_t>(a.y);
              tpb[static_cast<size_t>(r0) + k] = static_cast<uint16_t>(bb.y);
              if (k == 0 || a.x != iof[static_cast<size_t>(r0) + k - 1].x + 1) {  // a new run starts at k
                if (nr > 0 && nr <= kSubMaxRuns) d.run_end[nr - 1] = k;
                if (nr < kSubMaxRuns) d.run_off[nr] = a.x - k;
                ++nr;
              }
            }
            if (nr > kSubMaxRuns) runs_ok = false;
          }
          Q.io_runs = runs_ok ? 1 : 0;
          f.shape[kShapeIoRuns] = Q.io_runs;
          HIP_TRY(c, up(&Q.fwd.io, iof));
          HIP_TRY(c, up(&Q.bwd.io, iob));
          HIP_TRY(c, up(&Q.fwd.tpos, tpf));
          HIP_TRY(c, up(&Q.bwd.tpos, tpb));
        }
        tick("  sub: io lists");
        // fused projection in the backward sweep: the first rotation row of a pose finds the others right behind it
        // in the tile, and a pose of the last stage has all its rows there.  Row units of a block: {tile position, row}
        const Layout &L = c->F.L;
        const int64_t rot0 = L.rot_base, rot1 = L.rot_base + static_cast<int64_t>(L.d) * L.nl_poses;
        bool ok = group != nullptr;  // (a shard's rows are rotations | ranges | translations in this order too: the same tests on the row index)
        std::vector<int2> units;
        for (size_t b = 0; b < desc.size(); ++b) {
          const int32_t *rows = H.b_rows.data() + desc[b].row_begin;
          const int nb = desc[b].nrows;
          int64_t leaders = 0, rot_rows = 0;
          desc[b].unit_begin = static_cast<int32_t>(units.size());
          for (int k = 0; k < nb; ++k) {
            if (rows[k] < rot0 || rows[k] >= rot1) {
              units.push_back(make_int2(k, rows[k]));
              continue;
            }
            ++rot_rows;
            if ((rows[k] - rot0) % L.d != 0) continue;
            ++leaders;
            units.push_back(make_int2(k, rows[k]));
            for (int a = 1; a < L.d && ok; ++a) ok = k + a < nb && rows[k + a] == rows[k] + a;
          }
          desc[b].nunits = static_cast<int32_t>(units.size()) - desc[b].unit_begin;
          ok = ok && rot_rows == leaders * L.d;
        }
        units.push_back(make_int2(0, 0));
        HIP_TRY(c, up(&Q.b_unit, units));
        if (ok) {
          std::vector<char> in_top(static_cast<size_t>(L.rows), 0);
          for (int32_t r : f.plan.top_rows) in_top[r] = 1;
          for (int32_t r : f.plan.top_rows)
            if (r >= rot0 && r < rot1) {
              const int64_t lead = r - (r - rot0) % L.d;
              for (int a = 0; a < L.d && ok; ++a) ok = in_top[lead + a] != 0;
            }
        }
        f.fuse_ok = ok;
        if (tick.on()) std::fprintf(stderr, "  [tri plan] sweep fusion possible: %d\n", int(ok));
      }
      HIP_TRY(c, up(&Q.desc, desc));
      tick("  sub: units");
      // the host copy is not needed any more: 130 MB of vectors, 16 ms to hand back at 10^5 poses and 0.1 s at 10^6 -- on
      // a thread of its own (joined before the next factor is installed and when the handle goes), started AFTER the
      // last stage's uploads: a thread that unmaps 130 MB holds the address space's lock, and the next copy from pageable
      // memory waited 12 ms for it (measured: a 2.3 MB copy, 0.0122 s)
      dead_sub = std::make_shared<SubBlockOpHost>(std::move(H));
      H = SubBlockOpHost();
      continue;
    }
    if (k == 1 && f.stages[0].is_sub) {  // the last stage of a two-stage plan: only its two explicit-inverse products
      D.aux_sum = !S.fwd_a.empty();      // (+ the sum of the aux rows as a product of its own on large plans)
      if (D.aux_sum) HIP_TRY(c, up_op(D.fwd_a, S.fwd_a));
      HIP_TRY(c, up_op(D.fwd_b, S.fwd_b));
      tick("  top: forward product");
      HIP_TRY(c, up_op(D.bwd_b, S.bwd_b));
      tick("  top: backward product");
      continue;
    }
    if (D.has_fwd_a) HIP_TRY(c, up_op(D.fwd_a, S.fwd_a));
    if (S.dense) {
      BlockOpHost &H = S.blocks_op;
      D.blocks.nblocks = static_cast<int>(H.nrows.size());
      {
        // per-row records, padded per block to a multiple of eight (empty masks) + one spare round at the end; the
        // value arrays get 64 * 65 zero entries: the kernel's prefetch of the next round reads past a block's end
        std::vector<BlockDesc> desc(H.nrows.size());
        std::vector<BlockLane> bc, br;
        for (size_t b = 0; b < desc.size(); ++b) {
          desc[b] = BlockDesc{H.row_begin[b], H.nrows[b], static_cast<int32_t>(bc.size()), 0, H.w_off[b], 0};
          for (int l = 0; l < H.nrows[b]; ++l) {
            const size_t i = static_cast<size_t>(H.row_begin[b]) + l;
            bc.push_back(BlockLane{H.mask_col[i], H.off_col[i], H.rows[i]});
            br.push_back(BlockLane{H.mask_row[i], H.off_row[i], H.rows[i]});
          }
          while (bc.size() % 8) {
            bc.push_back(BlockLane{0, 0, 0});
            br.push_back(BlockLane{0, 0, 0});
          }
        }
        bc.resize(bc.size() + 24, BlockLane{0, 0, 0});
        br.resize(br.size() + 24, BlockLane{0, 0, 0});
        H.w_by_col.resize(H.w_by_col.size() + 64 * 65, 0.0);
        H.w_by_row.resize(H.w_by_row.size() + 64 * 65, 0.0);
        HIP_TRY(c, up(&D.blocks.desc, desc));
        HIP_TRY(c, up(&D.blocks.by_col, bc));
        HIP_TRY(c, up(&D.blocks.by_row, br));
      }
      HIP_TRY(c, up(&D.blocks.w_by_col, H.w_by_col));
      HIP_TRY(c, up(&D.blocks.w_by_row, H.w_by_row));
      HIP_TRY(c, up(&D.blocks.ext_ptr, H.ext_ptr));
      HIP_TRY(c, up(&D.blocks.ext_col, H.ext_col));
      HIP_TRY(c, up(&D.blocks.ext_val, H.ext_val));
      H = BlockOpHost();
      continue;
    }
    HIP_TRY(c, up_op(D.fwd_b, S.fwd_b));
    if (D.has_bwd_a) HIP_TRY(c, up_op(D.bwd_a, S.bwd_a));
    HIP_TRY(c, up_op(D.bwd_b, S.bwd_b));
  }
  if (dead_sub) {
    if (c->deferred_free.valid()) c->deferred_free.get();
    c->deferred_free = std::async(std::launch::async, [dead = std::move(dead_sub)]() mutable { dead.reset(); });
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  tick("upload");
  f.ready = true;
  ++f.generation;
  f.shape[kShapeFuseOk] = f.fuse_ok ? 1 : 0;
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
