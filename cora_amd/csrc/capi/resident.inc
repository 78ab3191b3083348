// Part of capi.hip (one translation unit; included there, in this order).  resident API: device vectors, the current point, the trust-region trial / accept pair, products and projections.
// ------------------------------------------------------------ resident API

// Resident vectors come from a small per-handle pool: TNT, the saddle escape and LOBPCG allocate and release 4-10
// vectors per call, three to six calls per staircase level, and every allocation and every free is a device-wide
// synchronisation (a failed certification at 10^5 poses spent more time in them than in its eigensolver iterations).
// A released vector is kept (up to kPoolMax of them) and handed to the next request of the same size, zeroed on the
// handle's stream like a fresh one; everything returns to the driver with the handle.
int cora_dev_alloc(cora_ctx *c, int k, double **dptr) {
  NEED_DEVICE(c);
  if (!dptr || k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_ARG, "bad arguments");
  const size_t bytes = vec_bytes(c, ld_for(k));
  *dptr = nullptr;
  for (size_t i = 0; i < c->pool.size(); ++i)
    if (c->pool[i].second == bytes) {
      *dptr = c->pool[i].first;
      c->pool.erase(c->pool.begin() + static_cast<std::ptrdiff_t>(i));
      break;
    }
  if (!*dptr) HIP_TRY(c, alloc_device(dptr, bytes));
  wrote(c, *dptr);  // the allocator may return an address that was freed while a trial product of it was kept
  HIP_TRY(c, hipMemsetAsync(*dptr, 0, bytes, c->stream));
  for (auto &p : c->user_allocs)
    if (!p.first) {
      p = {*dptr, bytes};
      return CORA_OK;
    }
  c->user_allocs.push_back({*dptr, bytes});
  return CORA_OK;
}

int cora_dev_free(cora_ctx *c, double *dptr) {
  NEED_DEVICE(c);
  wrote(c, dptr);
  constexpr size_t kPoolMax = 16;
  for (auto &p : c->user_allocs)
    if (p.first == dptr && dptr) {
      if (c->pool.size() < kPoolMax) {
        c->pool.push_back(p);  // work already enqueued on the handle's stream is ordered before any reuse
      } else {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        free_device(dptr);
      }
      p = {nullptr, 0};
      return CORA_OK;
    }
  return fail(c, CORA_ERR_ARG, "pointer was not allocated by cora_dev_alloc");
}

int cora_upload(cora_ctx *c, const double *host, int ld, int k, double *dptr) {
  NEED_DEVICE(c);
  wrote(c, dptr);
  int rc = upload_impl(c, host, ld, k, dptr);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // host buffer may be pageable
  return CORA_OK;
}

int cora_download(cora_ctx *c, const double *dptr, int k, double *host, int ld) {
  NEED_DEVICE(c);
  return download_impl(c, dptr, k, host, ld);
}

int cora_set_point_dev(cora_ctx *c, const double *dY) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!dY) return fail(c, CORA_ERR_ARG, "null pointer");
  return set_point_dev_impl(c, dY);
}

int cora_set_point(cora_ctx *c, const double *Y, int ldy) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  int rc = upload_impl(c, Y, ldy, c->p, c->d_Y);
  if (rc) return rc;
  return set_point_dev_impl(c, c->d_Y);
}

int cora_objective_dev(cora_ctx *c, const double *dY, double *f) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!dY || !f) return fail(c, CORA_ERR_ARG, "null pointer");
  double *dG;
  int rc = get_scratch(c, 5, c->ld, &dG);
  if (rc) return rc;
  if ((rc = apply_product(c, dY, c->ld, EPI_NONE, dG))) return rc;
  double v = 0.0;
  const double *a[1] = {dY};
  const double *b[1] = {dG};
  rc = cora_dots_dev(c, 1, a, b, &v);
  if (rc) return rc;
  *f = 0.5 * v;
  return CORA_OK;
}

// One trust-region trial step in ONE wait (Optimization::Riemannian::TNT's outer iteration between two inner solves, as
// called from src/CORA.cpp:139-140): H s for the model decrease, the retraction, Q X of the trial point for its cost, and
// the four inner products in one reduction.  The same kernels, in the same order per vector, as cora_hvp_dev +
// cora_dots_dev + cora_retract_dev + cora_objective_dev: the values are the same bits, two waits and a launch fewer.
int cora_tnt_trial_dev(cora_ctx *c, const double *dS, double *dHs, double *dXprop, double out[4]) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  if (!dS || !dHs || !dXprop || !out || dHs == dS || dXprop == dS || dXprop == dHs) return fail(c, CORA_ERR_ARG, "bad arguments");
  c->trial_x = nullptr;
  int rc;
  if (!c->d_G_trial) {
    HIP_TRY(c, alloc_device(&c->d_G_trial, vec_bytes(c, c->ld)));
    HIP_TRY(c, hipMemsetAsync(c->d_G_trial, 0, vec_bytes(c, c->ld), c->stream));
  }
  if ((rc = apply_product(c, dS, c->ld, EPI_HVP, dHs))) return rc;
  HIP_TRY(c, launch_project_manifold(row_args(c), c->ld, c->d_Y, dS, 1.0, dXprop, c->stream));
  if ((rc = apply_product(c, dXprop, c->ld, EPI_NONE, c->d_G_trial))) return rc;
  const double *A[4] = {c->d_rgrad, dS, dS, dXprop};
  const double *B[4] = {dS, dHs, dS, c->d_G_trial};
  if ((rc = cora_dots_dev(c, 4, A, B, out))) return rc;
  out[3] *= 0.5;
  c->trial_x = dXprop;
  return CORA_OK;
}

// The accepted trial point becomes the current point, and the preconditioned gradient with the norms TNT's stopping
// tests need comes back in the same wait: out = f, <g, g>, <P g, P g>, <g, P g>.  After cora_tnt_trial_dev of the same
// vector (one GPU) the product Q X is not formed again.  Otherwise: cora_set_point_dev + cora_precondition_projected_dev
// + cora_dots_dev, call by call.
int cora_tnt_accept_dev(cora_ctx *c, const double *dX, double *dPg, double out[4]) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!dX || !dPg || !out || dX == dPg) return fail(c, CORA_ERR_ARG, "bad arguments");
  int rc;
  const bool fast = c->F.L.world == 1 && c->trial_x == dX && c->d_G_trial && !cora::env_flag(cora::Env::NoTntFuse);
  if (fast) {
    c->trial_x = nullptr;
    if (dX != c->d_Y) HIP_TRY(c, hipMemcpyAsync(c->d_Y, dX, vec_bytes(c, c->ld), hipMemcpyDeviceToDevice, c->stream));
    std::swap(c->d_G, c->d_G_trial);
    if ((rc = point_finish(c, false))) return rc;
  } else if ((rc = set_point_dev_impl(c, dX))) {
    return rc;
  }
  if ((rc = cora_precondition_projected_dev(c, c->d_rgrad, dPg))) return rc;
  const double *A[3] = {c->d_rgrad, dPg, c->d_rgrad};
  const double *B[3] = {c->d_rgrad, dPg, dPg};
  if ((rc = cora_dots_dev(c, 3, A, B, out + 1))) return rc;
  if (fast) c->f = c->h_scalars[4];
  out[0] = c->f;
  return CORA_OK;
}

int cora_point_cost(cora_ctx *c, double *f) {
  if (!c || !f) return CORA_ERR_ARG;
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  *f = c->f;
  return CORA_OK;
}

const double *cora_point_Y_dev(const cora_ctx *c) { return (c && c->have_point) ? c->d_Y : nullptr; }
const double *cora_point_egrad_dev(const cora_ctx *c) { return (c && c->have_point) ? c->d_G : nullptr; }
const double *cora_point_rgrad_dev(const cora_ctx *c) { return (c && c->have_point) ? c->d_rgrad : nullptr; }

int cora_spmm_dev(cora_ctx *c, const double *dX, int k, double *dOut) {
  NEED_DEVICE(c);
  wrote(c, dOut);
  if (!dX || !dOut || k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_ARG, "bad arguments");
  return apply_product(c, dX, ld_for(k), EPI_NONE, dOut);
}

int cora_hvp_dev(cora_ctx *c, const double *dX, double *dOut) {
  NEED_DEVICE(c);
  wrote(c, dOut);
  NEED_RANK(c);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  if (!dX || !dOut) return fail(c, CORA_ERR_ARG, "null pointer");
  return apply_product(c, dX, c->ld, EPI_HVP, dOut);
}

int cora_certificate_product_dev(cora_ctx *c, const double *dX, int k, double *dOut) {
  NEED_DEVICE(c);
  wrote(c, dOut);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  if (!dX || !dOut || k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_ARG, "bad arguments");
  return exchange_and_product(c, spmm_args(c, dX, dOut), ld_for(k), EPI_S);
}

int cora_tangent_space_projection_dev(cora_ctx *c, const double *dV, double *dOut) {
  NEED_DEVICE(c);
  wrote(c, dOut);
  NEED_RANK(c);
  if (!c->have_point) return fail(c, CORA_ERR_NOT_READY, "no current point (cora_set_point)");
  HIP_TRY(c, launch_tangent_project(row_args(c), c->ld, c->d_Y, dV, nullptr, dOut, c->stream));
  return CORA_OK;
}
