// Part of capi.hip (one translation unit; included there, in this order).  values: in-place update of Q's values on a live handle -- the source map (ValueMap, cora_internal.h), the host-pointer and the device-pointer update, what an update invalidates.

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the map on the device: sources of sval | lval | head_val | diag | own_sym (two per slot), every part from a multiple
// of four entries on (the gather kernels read the sources in pairs and, for own_sym, in fours)
int upload_value_map(cora_ctx *c) {
  const ValueMap &M = c->vmap;
  const std::vector<int32_t> *parts[5] = {&M.sval, &M.lval, &M.head_val, &M.diag, &M.own_sym};
  size_t at = 0;
  for (int i = 0; i < 5; ++i) {
    c->vmap_off[i] = at;
    at += (parts[i]->size() + 3) & ~size_t{3};
  }
  std::vector<int32_t> all(std::max<size_t>(at, 4), kNoSource);
  for (int i = 0; i < 5; ++i) std::copy(parts[i]->begin(), parts[i]->end(), all.begin() + static_cast<std::ptrdiff_t>(c->vmap_off[i]));
  // d_lval holds the image's order of the long rows' entries (long_image.h): slot i of it is slot perm[i] of the format
  for (size_t i = 0; i < M.lval.size(); ++i) all[c->vmap_off[1] + i] = M.lval[static_cast<size_t>(c->LI.perm[i])];
  c->release_value_map();
  HIP_TRY(c, to_device(&c->d_vmap_src, all));
  HIP_TRY(c, to_device(&c->d_vmap_mirror, M.mirror));
  HIP_TRY(c, alloc_device(&c->d_vmap_vals, std::max<size_t>(static_cast<size_t>(M.nnz), 1) * sizeof(double)));
  return CORA_OK;
}

int build_value_map_impl(cora_ctx *c, const int32_t *rowptr, const int32_t *colidx) {
  static const int32_t no_col = 0;
  if (!colidx && c->F.L.N > 0 && rowptr[c->F.L.N] == 0) colidx = &no_col;  // (an empty Q, as at creation)
  if (!colidx) return fail(c, CORA_ERR_ARG, "null CSR pointer");
  ValueMap M;
  try {
    build_value_map(c->F, rowptr, colidx, c->dist_long, M);
  } catch (const std::exception &e) {
    return fail(c, CORA_ERR_ARG, e.what());
  }
  c->vmap = std::move(M);
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = upload_value_map(c);
    if (rc) {
      c->vmap = ValueMap();
      return rc;
    }
  }
  return CORA_OK;
}

// What depended on Q's values goes back to the state of a fresh handle: no point, no kept trial product, no
// preconditioner, no implicit factor, the explicit formulation.  Vectors, scratch, the communicator, the aux factor
// and the measurement table stay.
void values_changed(cora_ctx *c) {
  c->have_point = false;
  c->trial_x = nullptr;
  c->precond = CORA_PRECOND_NONE;
  c->precond_f.ready = false;
  c->implicit_f.ready = false;
  c->implicit = false;
}

// check kernel, flag, gather passes (d_vals: nnz doubles in CSR order).  Nothing is written unless the check passes.
int update_values_device(cora_ctx *c, const double *d_vals) {
  const ValueMap &M = c->vmap;
  const HostFormat &F = c->F;
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  HIP_TRY(c, launch_values_check(M.nnz, d_vals, static_cast<int64_t>(M.mirror.size() / 2), c->d_vmap_mirror, c->d_flag, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also: every product that reads the old values has finished)
  if (*c->h_flag & 1) return fail(c, CORA_ERR_ARG, "a value is not finite");
  if (*c->h_flag & 2)
    return fail(c, CORA_ERR_ARG, "the values break the symmetry the chain layout of the handle relies on (Q(i, j) and Q(j, i) "
                                 "of a pose's couplings to itself and to its neighbour must be equal)");
  const int32_t *src = c->d_vmap_src;
  HIP_TRY(c, launch_values_gather(static_cast<int64_t>(F.sval.size()), src + c->vmap_off[0], d_vals, c->d_sval, false, c->stream));
  HIP_TRY(c, launch_values_gather(static_cast<int64_t>(F.lval.size()), src + c->vmap_off[1], d_vals, c->d_lval, false, c->stream));
  HIP_TRY(c, launch_values_gather(static_cast<int64_t>(F.head_val.size()), src + c->vmap_off[2], d_vals, c->d_head_val, false, c->stream));
  HIP_TRY(c, launch_values_gather(static_cast<int64_t>(F.diag.size()), src + c->vmap_off[3], d_vals, c->d_diag_inv, true, c->stream));
  HIP_TRY(c, launch_values_gather_sym(static_cast<int64_t>(F.own_sym.size()), src + c->vmap_off[4], d_vals, c->d_own_sym, c->d_S, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_lam_st, 0, (static_cast<size_t>(F.L.nl_poses) * F.L.d * F.L.d + 2) * sizeof(double), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CORA_OK;
}

}  // namespace

int cora_values_map_build(cora_ctx *c, const int32_t *rowptr, const int32_t *colidx) {
  if (!c) return CORA_ERR_ARG;
  if (!rowptr) return fail(c, CORA_ERR_ARG, "null CSR pointer");
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = build_value_map_impl(c, rowptr, colidx);
  c->values_ms[0] = ms_since(t0);
  return rc;
}

int cora_update_values(cora_ctx *c, const int32_t *rowptr, const int32_t *colidx, const double *vals) {
  if (!c) return CORA_ERR_ARG;
  if (!rowptr) return fail(c, CORA_ERR_ARG, "null CSR pointer");
  const int64_t N = c->F.L.N;
  {
    static const int32_t no_col = 0;
    static const double no_val = 0.0;
    if (N > 0 && rowptr[N] == 0) {
      if (!colidx) colidx = &no_col;
      if (!vals) vals = &no_val;
    }
  }
  if (!colidx || !vals) return fail(c, CORA_ERR_ARG, "null CSR pointer");
  auto t0 = std::chrono::steady_clock::now();
  c->values_ms[0] = 0.0;
  if (!c->vmap.built) {
    const int rc = build_value_map_impl(c, rowptr, colidx);
    c->values_ms[0] = ms_since(t0);
    if (rc) return rc;
  } else {
    if (rowptr[0] != 0 || rowptr[N] != c->vmap.nnz)
      return fail(c, CORA_ERR_ARG, "the number of nonzeros differs from the handle's matrix");
    for (int64_t i = 0; i < N; ++i)
      if (rowptr[i + 1] < rowptr[i]) return fail(c, CORA_ERR_ARG, "rowptr not monotone");
    if (pattern_hash(N, rowptr, colidx) != c->vmap.pattern_hash)
      return fail(c, CORA_ERR_ARG, "the sparsity pattern differs from the one the handle was created with");
  }
  t0 = std::chrono::steady_clock::now();
  if (const char *why = value_map_check_host(c->vmap, vals)) return fail(c, CORA_ERR_ARG, why);
  c->values_ms[1] = ms_since(t0);
  c->values_ms[2] = c->values_ms[3] = 0.0;
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    t0 = std::chrono::steady_clock::now();
    if (c->vmap.nnz > 0) {
      HIP_TRY(c, hipMemcpyAsync(c->d_vmap_vals, vals, static_cast<size_t>(c->vmap.nnz) * sizeof(double), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->values_ms[2] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    const int rc = update_values_device(c, c->d_vmap_vals);
    c->values_ms[3] = ms_since(t0);
    if (rc) return rc;
  }
  t0 = std::chrono::steady_clock::now();
  value_map_apply_host(c->vmap, vals, c->F);
  c->host_values_stale = false;
  c->values_ms[4] = ms_since(t0);
  values_changed(c);
  return CORA_OK;
}

int cora_update_values_dev(cora_ctx *c, const double *d_vals) {
  NEED_DEVICE(c);
  if (!c->vmap.built) return fail(c, CORA_ERR_NOT_READY, "no source map yet: call cora_values_map_build or cora_update_values first");
  if (!d_vals && c->vmap.nnz > 0) return fail(c, CORA_ERR_ARG, "null pointer");
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = update_values_device(c, d_vals);
  c->values_ms[0] = c->values_ms[1] = c->values_ms[2] = c->values_ms[4] = 0.0;
  c->values_ms[3] = ms_since(t0);
  if (rc) return rc;
  c->host_values_stale = true;
  values_changed(c);
  return CORA_OK;
}

int cora_update_values_times(const cora_ctx *c, double ms[5]) {
  if (!c || !ms) return CORA_ERR_ARG;
  std::copy(c->values_ms, c->values_ms + 5, ms);
  return CORA_OK;
}
