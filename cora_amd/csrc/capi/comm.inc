// Part of capi.hip (one translation unit; included there, in this order).  native communication of a partitioned handle: RCCL, in-process and device-side (p2p) transports.

// ---------------------------------------------------------------------------------------------------------
// Native communication of a partitioned handle (SURVEY 8e; the collective steps of include/cora_hip.h,
// cora_set_comm, provided by the library itself instead of injected callbacks).  Two transports behind one plan:
//   RCCL  -- one process per GPU: ncclAllGather / ncclAllReduce on the handle's stream (librccl.so is opened at run
//            time, so single-GPU users carry no dependency); the id is created on rank 0 (cora_rccl_unique_id) and
//            handed to the other ranks by whatever launched them (torch.distributed in bench.py, MPI, a file);
//   local -- every rank a thread of ONE process with its own handle (and stream) on one or several visible devices:
//            device-to-device copies between the ranks' buffers behind a host barrier.  This is how the sharded
//            solver is tested on a one-GPU box, and it runs the same planning, pack and scatter code as RCCL.
// The exchange moves only the rows somebody reads: pack (k_move_rows) -> ONE all-gather of the packed rows ->
// scatter.  Every rank pads its export list to the longest one with its own first row.
// ---------------------------------------------------------------------------------------------------------

struct cora_local_group {
  int world = 0;
  std::mutex m;
  std::condition_variable cv;
  int waiting = 0;
  uint64_t generation = 0;
  bool broken = false;
  std::vector<const void *> ptrs;          // what every rank published for the current step
  std::vector<std::vector<double>> vals;   // host all-reduce operands
  // returns false if the group was broken (a rank failed): nobody waits for ever
  bool barrier() {
    std::unique_lock<std::mutex> lk(m);
    if (broken) return false;
    const uint64_t gen = generation;
    if (++waiting == world) {
      waiting = 0;
      ++generation;
      cv.notify_all();
      return true;
    }
    if (!cv.wait_for(lk, std::chrono::seconds(600), [&] { return generation != gen || broken; })) broken = true;
    if (broken) cv.notify_all();
    return !broken;
  }
};

namespace {

struct RcclApi {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;     // (optional: what the communicator itself reports)
  ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
};

const RcclApi *rccl_api(std::string *err) {
  static RcclApi api;
  static std::once_flag once;
  static std::string load_error;
  std::call_once(once, [] {
    for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
    }
    if (!api.lib) {
      load_error = std::string("cannot open librccl.so: ") + dlerror();
      return;
    }
    auto sym = [&](const char *n) {
      void *q = dlsym(api.lib, n);
      if (!q && load_error.empty()) load_error = std::string("librccl.so lacks ") + n;
      return q;
    };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(sym("ncclAllReduce"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.lib, "ncclCommCount"));
    api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(dlsym(api.lib, "ncclCommUserRank"));
  });
  if (!load_error.empty()) {
    if (err) *err = load_error;
    return nullptr;
  }
  return &api;
}

}  // namespace

struct cora_native_comm {
  cora_ctx *c = nullptr;
  int rank = 0, world = 1;
  cora_local_group *g = nullptr;  // local transport
  const RcclApi *api = nullptr;   // RCCL transport
  ncclComm_t nccl = nullptr;
  cora::P2PState *p2p = nullptr;  // device-side transport over peer-mapped mailboxes (p2p.h): no RCCL, no host on the data path
  long n_p2p_gather = 0, n_p2p_reduce = 0;
  // exchange plan
  int e_max = 0;
  int64_t exchanged_rows = 0;       // rows received per exchange (world * e_max)
  int32_t *d_export = nullptr;      // [e_max] rows of this rank's shard that some other rank reads (padded)
  int32_t *d_recv_idx = nullptr;    // [world * e_max] where the gathered rows go, rank by rank
  struct Buf { double *send = nullptr, *recv = nullptr; };
  std::map<int, Buf> buf;           // per row stride
  double *d_scal = nullptr, *h_scal = nullptr;  // 1024 doubles each (device / pinned): all-reduce staging
  std::string err;
  long n_allgather = 0, n_allreduce = 0;  // collectives issued on the data path (cora_comm_counters)
  int n_long() const { return static_cast<int>(c->F.long_rows.size()); }

  int fail_(const std::string &m) {
    err = m;
    if (c) c->err = m;
    if (g) {  // release the other ranks
      std::lock_guard<std::mutex> lk(g->m);
      g->broken = true;
      g->cv.notify_all();
    }
    return 1;
  }
  int hip(hipError_t e, const char *what) { return e == hipSuccess ? 0 : fail_(std::string(what) + ": " + hipGetErrorString(e)); }
  int nc(ncclResult_t r, const char *what) {
    return r == ncclSuccess ? 0 : fail_(std::string(what) + ": " + (api && api->GetErrorString ? api->GetErrorString(r) : "RCCL error"));
  }

  // all-gather of `bytes` bytes per rank between DEVICE buffers, ordered on the handle's stream
  int allgather_dev(const void *send, void *recv, size_t bytes, hipStream_t st = nullptr) {
    if (!st) st = c->stream;
    if (p2p) {  // one kernel: push into the peers' mailboxes, wait for theirs, copy out (counted apart: not a library collective)
      ++n_p2p_gather;
      return cora::p2p_allgather(p2p, send, recv, bytes, st, &err) ? fail_(err) : 0;
    }
    ++n_allgather;
    if (nccl) return nc(api->AllGather(send, recv, bytes, ncclChar, nccl, st), "ncclAllGather");
    if (hip(hipStreamSynchronize(st), "hipStreamSynchronize")) return 1;
    g->ptrs[rank] = send;
    if (!g->barrier()) return fail_("local group broken");
    for (int r = 0; r < world; ++r)
      if (hip(hipMemcpyAsync(static_cast<char *>(recv) + static_cast<size_t>(r) * bytes, g->ptrs[r], bytes,
                             hipMemcpyDeviceToDevice, st), "hipMemcpyAsync")) return 1;
    if (hip(hipStreamSynchronize(st), "hipStreamSynchronize")) return 1;
    if (!g->barrier()) return fail_("local group broken");  // nobody reuses its send buffer before everyone has copied
    return 0;
  }
  // sum of n device doubles over the ranks, in place, ordered on the handle's stream (the same bits on every rank)
  int allreduce_dev(double *d, int n) {
    if (p2p) {
      ++n_p2p_reduce;
      return cora::p2p_allreduce(p2p, d, n, c->stream, &err) ? fail_(err) : 0;
    }
    if (nccl) {
      ++n_allreduce;
      return nc(api->AllReduce(d, d, static_cast<size_t>(n), ncclDouble, ncclSum, nccl, c->stream), "ncclAllReduce");
    }
    std::vector<double> h(static_cast<size_t>(n));
    if (hip(hipMemcpyAsync(h.data(), d, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync")) return 1;
    if (hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return 1;
    if (allreduce_host(h.data(), n)) return 1;
    if (hip(hipMemcpyAsync(d, h.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync")) return 1;
    return hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  }
  int allreduce_host(double *vals, int n) {
    if (!p2p) ++n_allreduce;
    if (nccl || p2p) {
      if (n > 1016) return fail_("all-reduce of more than 1016 doubles");
      std::memcpy(h_scal, vals, sizeof(double) * n);
      if (hip(hipMemcpyAsync(d_scal, h_scal, sizeof(double) * n, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync")) return 1;
      if (p2p) {
        if (allreduce_dev(d_scal, n)) return 1;
      } else if (nc(api->AllReduce(d_scal, d_scal, static_cast<size_t>(n), ncclDouble, ncclSum, nccl, c->stream), "ncclAllReduce")) return 1;
      if (hip(hipMemcpyAsync(h_scal, d_scal, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync")) return 1;
      if (hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return 1;
      std::memcpy(vals, h_scal, sizeof(double) * n);
      return 0;
    }
    g->vals[rank].assign(vals, vals + n);
    if (!g->barrier()) return fail_("local group broken");
    std::vector<double> tot(static_cast<size_t>(n), 0.0);
    for (int r = 0; r < world; ++r)  // rank order: the same bits on every rank
      for (int i = 0; i < n; ++i) tot[i] += g->vals[r][i];
    if (!g->barrier()) return fail_("local group broken");
    std::copy(tot.begin(), tot.end(), vals);
    return 0;
  }
  // all-gather of host data (planning): `bytes` per rank
  int allgather_host(const void *send, void *recv, size_t bytes) {
    void *ds = nullptr, *dr = nullptr;
    if (hip(hipMalloc(&ds, std::max<size_t>(bytes, 8)), "hipMalloc") || hip(hipMalloc(&dr, std::max<size_t>(bytes, 8) * world), "hipMalloc")) return 1;
    int rc = hip(hipMemcpy(ds, send, bytes, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) rc = allgather_dev(ds, dr, bytes);
    if (!rc) rc = hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    if (!rc) rc = hip(hipMemcpy(recv, dr, bytes * world, hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(ds);
    (void)hipFree(dr);
    return rc;
  }

  int plan() {
    const Layout &L = c->F.L;
    int64_t n_need = 0;
    cora_remote_rows(c, nullptr, &n_need);
    std::vector<int32_t> need(static_cast<size_t>(std::max<int64_t>(n_need, 1)));
    cora_remote_rows(c, need.data(), &n_need);
    // every rank learns every need-list (padded to the longest with -1)
    std::vector<int64_t> counts(static_cast<size_t>(world));
    if (allgather_host(&n_need, counts.data(), sizeof(int64_t))) return 1;
    const int64_t n_max = std::max<int64_t>(1, *std::max_element(counts.begin(), counts.end()));
    std::vector<int32_t> padded(static_cast<size_t>(n_max), -1), lists(static_cast<size_t>(n_max) * world);
    std::copy(need.begin(), need.begin() + n_need, padded.begin());
    if (allgather_host(padded.data(), lists.data(), sizeof(int32_t) * n_max)) return 1;
    // rows of rank r's shard that any OTHER rank reads, ascending
    std::vector<std::vector<int32_t>> exports(static_cast<size_t>(world));
    {
      std::vector<char> wanted(static_cast<size_t>(L.rows), 0);
      for (int r = 0; r < world; ++r)
        for (int64_t k = 0; k < counts[r]; ++k) wanted[lists[static_cast<size_t>(r) * n_max + k]] = 1;  // a rank never lists its own rows
      for (int r = 0; r < world; ++r)
        for (int64_t row = L.shard_rows * r; row < L.shard_rows * (r + 1); ++row)
          if (wanted[row]) exports[r].push_back(static_cast<int32_t>(row));
    }
    size_t em = 1;
    for (const auto &e : exports) em = std::max(em, e.size());
    e_max = static_cast<int>(em);
    exchanged_rows = static_cast<int64_t>(world) * e_max;
    std::vector<int32_t> recv_idx;
    for (int r = 0; r < world; ++r) {
      std::vector<int32_t> e = exports[r];
      e.resize(em, static_cast<int32_t>(L.shard_rows * r));  // padding: the shard's first row, sent with its own value
      recv_idx.insert(recv_idx.end(), e.begin(), e.end());
      if (r == rank) {
        if (hip(hipMalloc(reinterpret_cast<void **>(&d_export), sizeof(int32_t) * em), "hipMalloc")) return 1;
        if (hip(hipMemcpy(d_export, e.data(), sizeof(int32_t) * em, hipMemcpyHostToDevice), "hipMemcpy")) return 1;
      }
    }
    if (hip(hipMalloc(reinterpret_cast<void **>(&d_recv_idx), sizeof(int32_t) * recv_idx.size()), "hipMalloc")) return 1;
    return hip(hipMemcpy(d_recv_idx, recv_idx.data(), sizeof(int32_t) * recv_idx.size(), hipMemcpyHostToDevice), "hipMemcpy");
  }

  int buffers(int ld, Buf **out) {
    Buf &b = buf[ld];
    if (!b.send) {  // per rank: e_max rows + one slot per distributed long row
      const size_t per = sizeof(double) * (static_cast<size_t>(e_max) + n_long()) * ld;
      if (hip(hipMalloc(reinterpret_cast<void **>(&b.send), per), "hipMalloc")) return 1;
      if (hip(hipMalloc(reinterpret_cast<void **>(&b.recv), per * world), "hipMalloc")) return 1;
      // (the slots of long rows that have no chunk on this rank are never written: they must read as zero -- the pack kernel
      // zeroes them per product, the device-side transport's pack-free path relies on this once)
      if (hip(hipMemsetAsync(b.send, 0, per, c->stream), "hipMemsetAsync")) return 1;
    }
    *out = &b;
    return 0;
  }

  // pack -> all-gather -> scatter, ordered on `st` (default: the handle's stream)
  int exchange(double *dX, int ld, hipStream_t st = nullptr) {
    if (!st) st = c->stream;
    if (hip(hipSetDevice(c->device), "hipSetDevice")) return 1;
    Buf *b;
    if (buffers(ld, &b)) return 1;
    if (hip(launch_move_rows(0, e_max, ld, d_export, dX, b->send, st), "pack")) return 1;
    if (allgather_dev(b->send, b->recv, sizeof(double) * e_max * ld, st)) return 1;
    return hip(launch_move_rows(1, static_cast<int64_t>(world) * e_max, ld, d_recv_idx, b->recv, dX, st), "scatter");
  }
  // device-side transport: the exchange kernel reads the exported rows from X itself, so a product needs no pack launch
  bool pack_free(int ld) const { return p2p && cora::p2p_exchange_unpack_fits(p2p, e_max, n_long(), ld); }
  int product_pack(const double *dX, int ld, hipStream_t st, double **slots) {
    if (hip(hipSetDevice(c->device), "hipSetDevice")) return 1;
    Buf *b;
    if (buffers(ld, &b)) return 1;
    *slots = b->send + static_cast<size_t>(e_max) * ld;
    if (pack_free(ld)) return 0;  // (slots written by this rank's chunks are overwritten per product, the others stay zero)
    return hip(launch_exchange_pack(e_max, ld, d_export, static_cast<int64_t>(n_long()) * ld, dX, b->send, st), "pack");
  }
  int product_gather(double *dX, int ld, hipStream_t st, double *out, double *kappa, hipEvent_t after_collective = nullptr) {
    Buf *b;
    if (buffers(ld, &b)) return 1;
    if (p2p && cora::p2p_exchange_unpack_fits(p2p, e_max, n_long(), ld)) {  // hand-over, wait and unpack in ONE kernel, from the mailbox
      ++n_p2p_gather;
      if (after_collective) (void)hipEventRecord(after_collective, st);
      return cora::p2p_exchange_unpack(p2p, b->send + static_cast<size_t>(e_max) * ld, d_export, e_max, n_long(), ld, d_recv_idx, dX,
                                       c->d_long_rows, c->d_long_owner, out, kappa, st, &err)
                 ? fail_(err) : 0;
    }
    if (allgather_dev(b->send, b->recv, sizeof(double) * (static_cast<size_t>(e_max) + n_long()) * ld, st)) return 1;
    if (after_collective) (void)hipEventRecord(after_collective, st);
    return hip(launch_exchange_unpack(world, e_max, n_long(), ld, d_recv_idx, b->recv, dX, rank, c->d_long_rows, c->d_long_owner,
                                      out, kappa, st), "unpack");
  }
  int allgather(double *dX, int ld) {  // whole shards, in place
    ++n_allgather;
    rows_gathered += static_cast<long long>(c->F.L.shard_rows) * world;
    if (hip(hipSetDevice(c->device), "hipSetDevice")) return 1;
    const Layout &L = c->F.L;
    const size_t n = static_cast<size_t>(L.shard_rows) * ld;
    if (p2p) {
      --n_allgather;
      return allgather_dev(dX + n * rank, dX, n * sizeof(double));  // in place: a rank's own piece is delivered onto itself
    }
    if (nccl) return nc(api->AllGather(dX + n * rank, dX, n, ncclDouble, nccl, c->stream), "ncclAllGather");
    if (hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return 1;
    g->ptrs[rank] = dX;
    if (!g->barrier()) return fail_("local group broken");
    for (int r = 0; r < world; ++r)
      if (r != rank && hip(hipMemcpyAsync(dX + n * r, static_cast<const double *>(g->ptrs[r]) + n * r, n * sizeof(double),
                                          hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync")) return 1;
    if (hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return 1;
    return g->barrier() ? 0 : fail_("local group broken");
  }
  // All-gather of ONE contiguous piece of every shard -- rows [row0, row0 + nrows) of the caller's own shard, every rank
  // its own piece (different offsets and lengths) -- into X in place: what the replicated translation solve of the
  // implicit formulation needs (the translation rows: 2 / 9 of a shard's rows at d = 3) instead of whole shards.
  // The pieces travel packed: own piece -> send buffer, one all-gather of the longest piece's size, one scatter kernel.
  struct PackedRows {
    int64_t row0 = -1, nrows = -1, maxn = 0;
    std::vector<int64_t> meta;   // {row0, nrows} of every rank
    int64_t *d_meta = nullptr;
    std::map<int, Buf> buf;      // per row stride
  } packed;
  long long rows_gathered = 0;   // rows received by all-gathers of resident vectors so far (whole shards or packed pieces)
  int allgather_rows(double *dX, int ld, int64_t row0, int64_t nrows) {
    if (hip(hipSetDevice(c->device), "hipSetDevice")) return 1;
    const Layout &L = c->F.L;
    if (packed.row0 != row0 || packed.nrows != nrows) {  // first call (the piece of a handle does not change): learn every rank's
      const int64_t mine[2] = {row0, nrows};
      packed.meta.assign(static_cast<size_t>(2 * world), 0);
      if (allgather_host(mine, packed.meta.data(), sizeof(mine))) return 1;
      if (!p2p) --n_allgather;  // (planning, not the data path)
      packed.maxn = 0;
      for (int r = 0; r < world; ++r) packed.maxn = std::max(packed.maxn, packed.meta[static_cast<size_t>(2 * r + 1)]);
      if (!packed.d_meta && hip(hipMalloc(&packed.d_meta, sizeof(int64_t) * 2 * world), "hipMalloc")) return 1;
      if (hip(hipMemcpy(packed.d_meta, packed.meta.data(), sizeof(int64_t) * 2 * world, hipMemcpyHostToDevice), "hipMemcpy")) return 1;
      for (auto &kv : packed.buf) {
        if (kv.second.send) (void)hipFree(kv.second.send);
        if (kv.second.recv) (void)hipFree(kv.second.recv);
      }
      packed.buf.clear();
      packed.row0 = row0;
      packed.nrows = nrows;
    }
    const size_t per = static_cast<size_t>(packed.maxn) * ld;
    rows_gathered += packed.maxn * world;
    if (per == 0) return 0;
    // (one path for both transports: the in-process one runs the same staging, collective and scatter kernel as RCCL)
    Buf &B = packed.buf[ld];
    if (!B.send) {
      if (hip(hipMalloc(&B.send, per * sizeof(double)), "hipMalloc") || hip(hipMalloc(&B.recv, per * world * sizeof(double)), "hipMalloc")) return 1;
      if (hip(hipMemsetAsync(B.send, 0, per * sizeof(double), c->stream), "hipMemsetAsync")) return 1;
    }
    if (nrows > 0 && hip(hipMemcpyAsync(B.send, dX + static_cast<size_t>(rank * L.shard_rows + row0) * ld, static_cast<size_t>(nrows) * ld * sizeof(double),
                                        hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync")) return 1;
    if (allgather_dev(B.send, B.recv, per * sizeof(double))) return 1;
    return hip(launch_scatter_shard_rows(world, rank, packed.maxn, ld, L.shard_rows, packed.d_meta, B.recv, dX, c->stream), "scatter");
  }
  ~cora_native_comm() {
    if (c && c->has_device) (void)hipSetDevice(c->device);
    for (auto &kv : packed.buf) {
      if (kv.second.send) (void)hipFree(kv.second.send);
      if (kv.second.recv) (void)hipFree(kv.second.recv);
    }
    if (packed.d_meta) (void)hipFree(packed.d_meta);
    for (auto &kv : buf) {
      if (kv.second.send) (void)hipFree(kv.second.send);
      if (kv.second.recv) (void)hipFree(kv.second.recv);
    }
    if (d_export) (void)hipFree(d_export);
    if (d_recv_idx) (void)hipFree(d_recv_idx);
    if (d_scal) (void)hipFree(d_scal);
    if (h_scal) (void)hipHostFree(h_scal);
    if (nccl && api) (void)api->CommDestroy(nccl);
    if (p2p) cora::p2p_destroy(p2p);
  }
};

static void native_comm_destroy(cora_native_comm *nc) { delete nc; }
static double *native_scalars(cora_native_comm *nc) { return nc->d_scal + 1016; }  // behind the host all-reduce's staging
static int native_allreduce_dev(cora_native_comm *nc, double *d, int n) { return nc->allreduce_dev(d, n); }
static int native_exchange_on(cora_native_comm *nc, double *dX, int ld, hipStream_t st) { return nc->exchange(dX, ld, st); }
static int native_product_pack(cora_native_comm *nc, const double *dX, int ld, hipStream_t st, double **slots) { return nc->product_pack(dX, ld, st, slots); }
static int native_product_gather(cora_native_comm *nc, double *dX, int ld, hipStream_t st, double *out, double *kappa,
                                 hipEvent_t after_collective) {
  return nc->product_gather(dX, ld, st, out, kappa, after_collective);
}
static const std::string &native_error(const cora_native_comm *nc) { return nc->err; }
static int native_allgather_rows(cora_native_comm *nc, double *dX, int ld, int64_t row0, int64_t nrows) { return nc->allgather_rows(dX, ld, row0, nrows); }

namespace {
int native_exchange_cb(void *u, double *dX, int ld) { return static_cast<cora_native_comm *>(u)->exchange(dX, ld); }
int native_allreduce_cb(void *u, double *vals, int n) { return static_cast<cora_native_comm *>(u)->allreduce_host(vals, n); }
int native_allgather_cb(void *u, double *dX, int ld) { return static_cast<cora_native_comm *>(u)->allgather(dX, ld); }

int native_finish(cora_ctx *c, cora_native_comm *nc) {
  if (nc->hip(hipMalloc(reinterpret_cast<void **>(&nc->d_scal), 1024 * sizeof(double)), "hipMalloc") ||
      nc->hip(hipHostMalloc(reinterpret_cast<void **>(&nc->h_scal), 1024 * sizeof(double)), "hipHostMalloc") || nc->plan()) {
    const std::string m = nc->err;
    delete nc;
    return fail(c, CORA_ERR_HIP, "native communication: " + m);
  }
  delete c->native_comm;
  c->native_comm = nc;
  c->comm_exchange = native_exchange_cb;
  c->comm_allreduce = native_allreduce_cb;
  c->comm_allgather = native_allgather_cb;
  c->comm_user = nc;
  return CORA_OK;
}
}  // namespace

extern "C" {

int cora_rccl_unique_id(void *id128) {
  if (!id128) return CORA_ERR_ARG;
  std::string err;
  const RcclApi *api = rccl_api(&err);
  if (!api) return fail(nullptr, CORA_ERR_HIP, err);
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return fail(nullptr, CORA_ERR_HIP, "ncclGetUniqueId failed");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id128, &id, sizeof(id));
  return CORA_OK;
}

int cora_comm_create_rccl(cora_ctx *c, const void *id128) {
  NEED_DEVICE(c);
  if (!id128) return fail(c, CORA_ERR_ARG, "bad arguments");
  std::string err;
  const RcclApi *api = rccl_api(&err);
  if (!api) return fail(c, CORA_ERR_HIP, err);
  auto *nc = new cora_native_comm;
  nc->c = c;
  nc->rank = c->F.L.rank;
  nc->world = c->F.L.world;
  nc->api = api;
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  const ncclResult_t r = api->CommInitRank(&nc->nccl, nc->world, id, nc->rank);
  if (r != ncclSuccess) {
    const std::string m = std::string("ncclCommInitRank: ") + api->GetErrorString(r);
    nc->nccl = nullptr;
    delete nc;
    return fail(c, CORA_ERR_HIP, m);
  }
  // the communicator must be what the partition assumes: world ranks, this rank's number (a launcher that hands the
  // id to the wrong set of processes would otherwise gather shards in the wrong order, silently)
  if (api->CommCount && api->CommUserRank) {
    int cnt = -1, ur = -1;
    if (api->CommCount(nc->nccl, &cnt) != ncclSuccess || api->CommUserRank(nc->nccl, &ur) != ncclSuccess || cnt != nc->world || ur != nc->rank) {
      const std::string m = "RCCL communicator reports " + std::to_string(cnt) + " ranks / rank " + std::to_string(ur) +
                            ", the handle was partitioned for " + std::to_string(nc->world) + " / " + std::to_string(nc->rank);
      delete nc;
      return fail(c, CORA_ERR_ARG, m);
    }
  }
  return native_finish(c, nc);
}

int cora_comm_rccl_ranks(const cora_ctx *c, int out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = out[1] = -1;
  const cora_native_comm *nc = c->native_comm;
  if (!nc || !nc->nccl || !nc->api || !nc->api->CommCount || !nc->api->CommUserRank) return CORA_OK;
  if (nc->api->CommCount(nc->nccl, &out[0]) != ncclSuccess || nc->api->CommUserRank(nc->nccl, &out[1]) != ncclSuccess) out[0] = out[1] = -1;
  return CORA_OK;
}

cora_local_group *cora_local_group_create(int world) {
  if (world < 1) return nullptr;
  auto *g = new cora_local_group;
  g->world = world;
  g->ptrs.assign(static_cast<size_t>(world), nullptr);
  g->vals.resize(static_cast<size_t>(world));
  return g;
}
void cora_local_group_destroy(cora_local_group *g) { delete g; }
void cora_local_group_abort(cora_local_group *g) {  // a rank gave up: nobody keeps waiting for it
  if (!g) return;
  std::lock_guard<std::mutex> lk(g->m);
  g->broken = true;
  g->cv.notify_all();
}

int cora_comm_create_local(cora_ctx *c, cora_local_group *g) {
  NEED_DEVICE(c);
  if (!g || g->world != c->F.L.world) return fail(c, CORA_ERR_ARG, "the group's size is not the handle's world size");
  auto *nc = new cora_native_comm;
  nc->c = c;
  nc->rank = c->F.L.rank;
  nc->world = c->F.L.world;
  nc->g = g;
  return native_finish(c, nc);
}

// Device-side transport (p2p.h).  Two steps, because the peers' mailboxes must exist before anybody can map them:
//   cora_comm_p2p_handle  -> this rank's mailbox and its 128-byte export blob;
//   (the launcher gathers the blobs of all ranks in rank order: torch.distributed, MPI, a file -- like the RCCL id)
//   cora_comm_create_p2p  -> maps the peers and plans the exchange (the planning all-gathers already run on the mailboxes).
int cora_comm_p2p_handle(cora_ctx *c, void *blob128) {
  NEED_DEVICE(c);
  if (!blob128) return fail(c, CORA_ERR_ARG, "bad arguments");
  if (c->p2p_pending) {
    cora::p2p_destroy(c->p2p_pending);
    c->p2p_pending = nullptr;
  }
  std::string err;
  if (cora::p2p_create(c->device, c->F.L.rank, c->F.L.world, &c->p2p_pending, blob128, &err)) return fail(c, CORA_ERR_HIP, err);
  return CORA_OK;
}

int cora_comm_create_p2p(cora_ctx *c, const void *blobs) {
  NEED_DEVICE(c);
  if (!blobs) return fail(c, CORA_ERR_ARG, "bad arguments");
  if (!c->p2p_pending) return fail(c, CORA_ERR_NOT_READY, "cora_comm_p2p_handle was not called on this handle");
  std::string err;
  if (cora::p2p_connect(c->p2p_pending, blobs, &err)) return fail(c, CORA_ERR_HIP, err);
  auto *nc = new cora_native_comm;
  nc->c = c;
  nc->rank = c->F.L.rank;
  nc->world = c->F.L.world;
  nc->p2p = c->p2p_pending;
  c->p2p_pending = nullptr;
  return native_finish(c, nc);
}

int cora_comm_p2p_status(const cora_ctx *c, long out[6]) {
  if (!c || !out) return CORA_ERR_ARG;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  out[3] = -1;
  const cora_native_comm *nc = c->native_comm;
  if (!nc || !nc->p2p) return CORA_OK;
  cora::p2p_status(nc->p2p, out);
  out[4] = nc->n_p2p_gather;
  out[5] = nc->n_p2p_reduce;
  return CORA_OK;
}

int cora_comm_native_enable(cora_ctx *c, int on) {
  if (!c || !c->native_comm) return fail(c, CORA_ERR_NOT_READY, "no native communication on this handle");
  c->comm_exchange = on ? native_exchange_cb : nullptr;
  c->comm_allreduce = on ? native_allreduce_cb : nullptr;
  c->comm_allgather = on ? native_allgather_cb : nullptr;
  c->comm_user = on ? c->native_comm : nullptr;
  return CORA_OK;
}

int cora_debug_spmm_window_min_slices(int min_slices) {
  const int old = g_win_min_slices;
  if (min_slices >= 0) g_win_min_slices = min_slices;
  return old;
}

int cora_debug_spmm_stagger_ticks(int ticks) {
  const int old = g_spmm_stagger_ticks;
  if (ticks >= 0) g_spmm_stagger_ticks = spmm_stagger_clamp(ticks);
  return old;
}

int cora_debug_spmm_stagger_force(int on) {
  const int old = g_spmm_stagger_force;
  if (on >= 0) g_spmm_stagger_force = std::min(on, 2);
  return old;
}

int cora_debug_local_products(cora_ctx *c, int on) {
  if (!c) return CORA_ERR_ARG;
  c->local_products = on != 0;
  return CORA_OK;
}

int cora_debug_product_phases(cora_ctx *c, const double *dX, double *dOut, int epi, int reps, double us[5]) {
  NEED_DEVICE(c);
  NEED_RANK(c);
  if (!dX || !dOut || !us || reps < 1 || epi < EPI_NONE || epi > EPI_HVP) return fail(c, CORA_ERR_ARG, "bad arguments");
  // The call is collective (reps + 3 all-gathers), so whether it runs must not depend on anything rank-local (round-4
  // advice): product_one_collective() is the same on every rank (world, transport, the common list of long rows), the
  // interior / boundary overlap is not (it counts THIS rank's slices) -- the serial order is forced for the duration of
  // the call instead of being required.
  if (!product_one_collective(c))
    return fail(c, CORA_ERR_NOT_READY, "phase timing needs the library's own communication and distributed long rows");
  while (c->phase_events.size() < 6) {
    hipEvent_t e;
    HIP_TRY(c, hipEventCreate(&e));
    c->phase_events.push_back(e);
  }
  for (int k = 0; k < 5; ++k) us[k] = 0.0;
  const int overlap_saved = c->overlap_exchange;
  c->overlap_exchange = 0;
  int rc = CORA_OK;
  for (int it = 0; it < reps + 3 && !rc; ++it) {   // (three warm-up rounds)
    c->phase_timing = true;
    rc = apply_product(c, dX, c->ld, epi, dOut);
    c->phase_timing = false;
    if (rc) break;
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, CORA_ERR_HIP, "hipStreamSynchronize"); break; }
    if (it < 3) continue;
    for (int k = 0; k < 5 && !rc; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->phase_events[k], c->phase_events[k + 1]) != hipSuccess) rc = fail(c, CORA_ERR_HIP, "hipEventElapsedTime");
      us[k] += ms * 1e3 / reps;
    }
  }
  c->overlap_exchange = overlap_saved;
  return rc;
}

long long cora_comm_gathered_rows(const cora_ctx *c) { return (c && c->native_comm) ? c->native_comm->rows_gathered : 0; }

int cora_comm_counters(const cora_ctx *c, long out[2]) {
  if (!c || !out) return CORA_ERR_ARG;
  out[0] = c->native_comm ? c->native_comm->n_allgather : 0;
  out[1] = c->native_comm ? c->native_comm->n_allreduce : 0;
  return CORA_OK;
}

int cora_comm_overlap_enable(cora_ctx *c, int on) {
  if (!c) return CORA_ERR_ARG;
  if (on < 0 || on > 2) return fail(c, CORA_ERR_ARG, "overlap mode must be 0, 1 or 2");
  c->overlap_exchange = on;
  return CORA_OK;
}

int cora_comm_overlap_active(const cora_ctx *c) { return c && product_overlaps_exchange(c) ? 1 : 0; }

int64_t cora_comm_exchanged_rows(const cora_ctx *c) { return (c && c->native_comm) ? c->native_comm->exchanged_rows : 0; }

}  // extern "C"
