// Part of capi.hip (one translation unit; included there, in this order).  assembly: Q(w) from per-measurement weights on a live handle -- the term map (TermMap, cora_internal.h), the host-pointer and the device-pointer assembly, the host mirror, what an assembly changes.

namespace {

int upload_term_map(cora_ctx *c) {
  const TermMap &M = c->tmap;
  HIP_TRY(c, to_device(&c->d_tptr, M.tptr));
  HIP_TRY(c, to_device(&c->d_tweight, M.tweight));
  HIP_TRY(c, to_device(&c->d_tcoef, M.tcoef));
  HIP_TRY(c, to_device(&c->d_tlong, M.long_entries));
  HIP_TRY(c, to_device(&c->d_tbase, M.base));
  HIP_TRY(c, alloc_device(&c->d_asm_w, std::max<size_t>(static_cast<size_t>(M.n_weights), 1) * sizeof(double)));
  for (hipEvent_t &e : c->asm_ev)
    if (!e) HIP_TRY(c, hipEventCreate(&e));
  return CORA_OK;
}

const char *weights_bad_host(const TermMap &M, const double *w) {
  for (int64_t i = 0; i < M.n_weights; ++i)
    if (!(std::isfinite(w[i]) && w[i] >= 0.0)) return "a weight is negative or not finite";
  return nullptr;
}

// kappa, tau and omega of the host table = base * w (the device's k_scale_precisions computes the same products)
void scale_host_table(cora_ctx *c, const double *w) {
  MeasurementTable &T = c->meas;
  const TermMap &M = c->tmap;
  const int d = c->F.L.d;
  const int64_t ne = T.n_edges, nr = T.n_ranges;
  double *kt = T.edge_data.data() + static_cast<size_t>(d * d + d) * ne;  // [kappa | tau], contiguous
  for (int64_t i = 0; i < 2 * ne; ++i) kt[i] = M.base[static_cast<size_t>(i)] * w[i];
  for (int64_t m = 0; m < nr; ++m) T.range_data[static_cast<size_t>(nr + m)] = M.base[static_cast<size_t>(2 * ne + m)] * w[2 * ne + m];
}

// weight check, flag | assembly into the staging buffer | update_values_device (check and gather passes) | rescale of the
// device table.  Nothing of the handle is written unless both checks pass.
int assemble_device(cora_ctx *c, const double *d_w) {
  const TermMap &M = c->tmap;
  MeasurementTable &T = c->meas;
  auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
  HIP_TRY(c, launch_weights_check(M.n_weights, d_w, c->d_flag, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->asm_ms[1] = ms_since(t0);
  if (*c->h_flag) return fail(c, CORA_ERR_ARG, "a weight is negative or not finite");
  AssembleArgs A;
  A.nnz = M.nnz;
  A.n_long = static_cast<int>(M.long_entries.size());
  A.tptr = c->d_tptr;
  A.tweight = c->d_tweight;
  A.tcoef = c->d_tcoef;
  A.long_entries = c->d_tlong;
  HIP_TRY(c, hipEventRecord(c->asm_ev[0], c->stream));
  HIP_TRY(c, launch_assemble(A, d_w, c->d_vmap_vals, c->stream));
  HIP_TRY(c, hipEventRecord(c->asm_ev[1], c->stream));
  t0 = std::chrono::steady_clock::now();
  const int rc = update_values_device(c, c->d_vmap_vals);  // (synchronises)
  c->asm_ms[3] = ms_since(t0);
  float ms = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&ms, c->asm_ev[0], c->asm_ev[1]));
  c->asm_ms[2] = ms;
  if (rc) return rc;
  const int d = c->F.L.d;
  const int64_t ne = T.n_edges, nr = T.n_ranges;
  HIP_TRY(c, launch_scale_precisions(2 * ne, c->d_tbase, d_w, T.d_edge_data + static_cast<size_t>(d * d + d) * ne, c->stream));
  HIP_TRY(c, launch_scale_precisions(nr, c->d_tbase + 2 * ne, d_w + 2 * ne, T.d_range_data + nr, c->stream));
  return CORA_OK;
}

}  // namespace

int cora_assembly_build(cora_ctx *c, const int32_t *rowptr, const int32_t *colidx) {
  if (!c) return CORA_ERR_ARG;
  const Layout &L = c->F.L;
  if (L.world > 1) return fail(c, CORA_ERR_ARG, "the assembly of Q(w) is not supported on partitioned handles");
  if (!c->meas.set) return fail(c, CORA_ERR_NOT_READY, "no measurement table (cora_set_measurements)");
  if (!rowptr || (!colidx && rowptr[L.N] > 0)) return fail(c, CORA_ERR_ARG, "null CSR pointer");
  const auto t0 = std::chrono::steady_clock::now();
  if (!c->vmap.built) {
    const int rc = build_value_map_impl(c, rowptr, colidx);
    if (rc) return rc;
  } else {
    if (rowptr[0] != 0 || rowptr[L.N] != c->vmap.nnz)
      return fail(c, CORA_ERR_ARG, "the number of nonzeros differs from the handle's matrix");
    for (int64_t i = 0; i < L.N; ++i)
      if (rowptr[i + 1] < rowptr[i]) return fail(c, CORA_ERR_ARG, "rowptr not monotone");
    if (pattern_hash(L.N, rowptr, colidx) != c->vmap.pattern_hash)
      return fail(c, CORA_ERR_ARG, "the sparsity pattern differs from the one the handle was created with");
  }
  MeasurementTable &T = c->meas;
  if (c->has_device) HIP_TRY(c, hipSetDevice(c->device));
  if (T.host_stale) {  // the base precisions are the ones the table holds NOW: on the device
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!T.edge_data.empty()) HIP_TRY(c, hipMemcpy(T.edge_data.data(), T.d_edge_data, T.edge_data.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!T.range_data.empty()) HIP_TRY(c, hipMemcpy(T.range_data.data(), T.d_range_data, T.range_data.size() * sizeof(double), hipMemcpyDeviceToHost));
    T.host_stale = false;
  }
  TermMap M;
  try {
    build_term_map(L.d, L.N, rowptr, colidx, T.n_edges, T.api_edge_rows.data(), T.edge_data.data(), T.n_ranges,
                   T.api_range_rows.data(), T.range_data.data(), M);
  } catch (const std::exception &e) {
    return fail(c, CORA_ERR_ARG, e.what());
  }
  if (c->has_device) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_assembly(c);
    c->tmap = std::move(M);
    const int rc = upload_term_map(c);
    if (rc) {
      const std::string why = c->err;
      free_assembly(c);
      return fail(c, rc, why);
    }
  } else {
    c->tmap = std::move(M);
  }
  c->asm_ms[0] = ms_since(t0);
  return CORA_OK;
}

int cora_assembly_info(const cora_ctx *c, int64_t out[4]) {
  if (!c || !out) return CORA_ERR_ARG;
  if (!c->tmap.built) return CORA_ERR_NOT_READY;
  out[0] = c->tmap.n_weights;
  out[1] = c->tmap.n_terms;
  out[2] = static_cast<int64_t>(c->tmap.long_entries.size());
  out[3] = c->tmap.max_terms;
  return CORA_OK;
}

int cora_debug_assemble_values_host(cora_ctx *c, const double *w, double *vals_out) {
  if (!c) return CORA_ERR_ARG;
  if (!c->tmap.built) return fail(c, CORA_ERR_NOT_READY, "no term map yet: call cora_assembly_build first");
  if ((!w && c->tmap.n_weights > 0) || (!vals_out && c->tmap.nnz > 0)) return fail(c, CORA_ERR_ARG, "null pointer");
  if (const char *why = weights_bad_host(c->tmap, w)) return fail(c, CORA_ERR_ARG, why);
  term_map_apply_host(c->tmap, w, vals_out);
  return CORA_OK;
}

int cora_assemble_values(cora_ctx *c, const double *w, double *vals_out) {
  if (!c) return CORA_ERR_ARG;
  const TermMap &M = c->tmap;
  if (!M.built) return fail(c, CORA_ERR_NOT_READY, "no term map yet: call cora_assembly_build first");
  if (!w && M.n_weights > 0) return fail(c, CORA_ERR_ARG, "null pointer");
  if (const char *why = weights_bad_host(M, w)) return fail(c, CORA_ERR_ARG, why);
  std::vector<double> tmp;
  double *vals = vals_out;
  if (!vals) {
    tmp.resize(std::max<size_t>(static_cast<size_t>(M.nnz), 1));
    vals = tmp.data();
  }
  c->asm_ms[1] = c->asm_ms[2] = c->asm_ms[3] = 0.0;
  auto t0 = std::chrono::steady_clock::now();
  if (c->has_device) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (M.n_weights > 0) HIP_TRY(c, hipMemcpyAsync(c->d_asm_w, w, static_cast<size_t>(M.n_weights) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int rc = assemble_device(c, c->d_asm_w);
    if (rc) return rc;
    t0 = std::chrono::steady_clock::now();
    if (M.nnz > 0) HIP_TRY(c, hipMemcpyAsync(vals, c->d_vmap_vals, static_cast<size_t>(M.nnz) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    term_map_apply_host(M, w, vals);
    c->asm_ms[2] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (const char *why = value_map_check_host(c->vmap, vals)) return fail(c, CORA_ERR_ARG, why);
  }
  value_map_apply_host(c->vmap, vals, c->F);  // the host copy of the format holds the assembled bits
  c->host_values_stale = false;
  scale_host_table(c, w);
  c->meas.host_stale = false;
  c->asm_ms[4] = ms_since(t0);
  values_changed(c);
  return CORA_OK;
}

int cora_assemble_values_dev(cora_ctx *c, const double *d_w, double *d_vals_out) {
  NEED_DEVICE(c);
  const TermMap &M = c->tmap;
  if (!M.built) return fail(c, CORA_ERR_NOT_READY, "no term map yet: call cora_assembly_build first");
  if (!d_w && M.n_weights > 0) return fail(c, CORA_ERR_ARG, "null pointer");
  const int rc = assemble_device(c, d_w);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  if (d_vals_out && M.nnz > 0)
    HIP_TRY(c, hipMemcpyAsync(d_vals_out, c->d_vmap_vals, static_cast<size_t>(M.nnz) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->asm_ms[4] = ms_since(t0);
  c->host_values_stale = true;
  c->meas.host_stale = true;
  values_changed(c);
  return CORA_OK;
}

int cora_assemble_times(const cora_ctx *c, double ms[5]) {
  if (!c || !ms) return CORA_ERR_ARG;
  std::copy(c->asm_ms, c->asm_ms + 5, ms);
  return CORA_OK;
}
