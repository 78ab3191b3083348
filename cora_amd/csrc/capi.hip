// C-ABI layer of libcora_hip.so (see include/cora_hip.h).  Owns the handle,
// device memory and stream; every compute entry point ends in a HIP kernel of
// kernels.hip -- there is no CPU fallback.
//
// ONE translation unit in eighteen pieces (round 6: the file had grown to 3 400 lines).  This file holds the handle (cora_ctx), the
// error / device macros and the helpers every part uses; the entry points live in capi/*.inc, included at the end in this order:
//   handle.inc          creation of (partitioned) handles, destruction, rank state, row maps, statistics
//   resident.inc        device vectors, the current point, the trust-region trial / accept pair, products, projections
//   preconditioner.inc  Jacobi / Cholesky set-up, a host factor installed as a device solve plan, the staged solve
//   products.inc        implicit formulation, exchange of a partitioned product and its overlap, distributed long rows
//   solver_ops.inc      auxiliary factors, formulation switch, retraction, vector updates, inner products
//   stpcg.inc           the device-resident Steihaug-Toint PCG (every form of the iteration), injected communication
//   blocks.inc          row moves, STPCG measurement hooks, LOBPCG's block algebra, timers
//   host_pointer.inc    the host-pointer operator API (one entry per reference method), host-side debug hooks
//   measurements.inc    the measurement table of a handle and the per-measurement residuals
//   values.inc          in-place update of Q's values: source map, host-pointer and device-pointer update
//   assembly.inc        Q(w) from per-measurement weights: term map, host-pointer, device-pointer and host-mirror assembly
//   gnc.inc             the weight step of a robust-cost (GNC) loop: device-pointer, host-pointer and host-mirror form
//   compare.inc         trajectory comparison after an orthogonal alignment: device-pointer, host-pointer and host form
//   rpe.inc             relative pose error over a pair table of the handle: table, device-pointer, host-pointer and host-mirror form
//   round.inc           rounding of a relaxed point to SE(d): device-pointer, host-pointer and host-mirror form
//   init_common.inc     what the five initialisers below share: the range-row step, the three forms of a call, installing and building tables, the mirror's sums
//   odom.inc            odometry initialisation: chain tables, device-pointer, host-pointer and host-mirror form
//   multilat.inc        landmark initialisation from ranges: list tables, device-pointer, host-pointer and host-mirror form
//   placement.inc       chain placement from inter-robot ranges: stage tables, device-pointer, host-pointer and host-mirror form
//   sighting.inc        placement from pose-landmark sightings: stage and list tables, device-pointer, host-pointer and host-mirror form
//   closure.inc         placement from inter-chain relative-pose edges: stage and list tables, device-pointer, host-pointer and host-mirror form, plain and with the consensus vote
//   comm.inc            native communication: RCCL, in-process and device-side (p2p.h) transports
#include <hip/hip_runtime.h>
// RCCL's types and the few enumerators used, declared here (NCCL's public ABI: they have not changed since 2.0): the
// entry points are resolved with dlsym at run time (native communication, end of file), so neither the build nor a
// single-GPU user needs RCCL's headers or library.
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclChar = 0, ncclDouble = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
}
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <future>
#include <condition_variable>
#include <map>
#include <mutex>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <deque>
#include <atomic>
#include <vector>

#include "../../include/cora_hip.h"
#include "config.h"
#include "cora_internal.h"
#include "dispatch.h"
#include "kernels.h"
#include "long_image.h"
#include "p2p.h"
#include "parallel.h"
#include "trisolve_image.h"

using namespace cora;

namespace {
thread_local std::string g_create_error;
constexpr int kScratchSlots = 9;
}  // namespace

constexpr size_t kProfMarks = 8;  // events per profiled STPCG iteration (cora_debug_profile_stpcg)
struct cora_native_comm;
static void native_comm_destroy(cora_native_comm *nc);
static double *native_scalars(cora_native_comm *nc);                       // 8 device doubles of the sharded STPCG
static int native_allreduce_dev(cora_native_comm *nc, double *d, int n);   // sum over the ranks, in place, on the stream
static int native_exchange_on(cora_native_comm *nc, double *dX, int ld, hipStream_t st);  // the exchange, ordered on st
// the exchange of a PRODUCT, in two halves around the launch of the distributed long rows' chunks: pack the exported rows
// (+ zeroed slots for the long rows' partial sums, returned in *slots) | all-gather of rows and slots in ONE collective,
// rows scattered into dX, slots summed in rank order into the owners' rows of `out` (+ their kappa slots)
static int native_product_pack(cora_native_comm *nc, const double *dX, int ld, hipStream_t st, double **slots);
static int native_product_gather(cora_native_comm *nc, double *dX, int ld, hipStream_t st, double *out, double *kappa,
                                 hipEvent_t after_collective = nullptr);
static const std::string &native_error(const cora_native_comm *nc);
static int native_allgather_rows(cora_native_comm *nc, double *dX, int ld, int64_t row0, int64_t nrows);  // one piece of every shard, packed
// The ONE place that talks to the allocator (capi/comm.inc's transports keep their own state).  alloc_* pass the runtime's answer
// to the caller's HIP_TRY / CREATE_TRY and write no byte; free_* free what is named and null the pointers (the device must be
// current).  The rule of the whole handle: every resource has ONE owner -- a table struct, a DevBuf, a DevArena or a group of
// cora_ctx's fields -- whose release(), written under the declarations, is the ONE list of its pointers; destruction names none.
static std::atomic<int64_t> g_live_allocations{0};  // device and pinned blocks these helpers hold (cora_debug_live_allocations)
template <class T>
static hipError_t alloc_device(T **p, size_t bytes) {
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
  if (e == hipSuccess && *p) ++g_live_allocations;
  return e;
}
template <class T>
static hipError_t alloc_pinned(T **p, size_t bytes) {
  const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(p), bytes);
  if (e == hipSuccess && *p) ++g_live_allocations;
  return e;
}
template <class... P>
static void free_device(P *&...p) {
  ((p ? ((void)hipFree(p), (void)--g_live_allocations) : void(), p = nullptr), ...);
}
template <class... P>
static void free_pinned(P *&...p) {
  ((p ? ((void)hipHostFree(p), (void)--g_live_allocations) : void(), p = nullptr), ...);
}
template <class... E>
static void free_events(E &...e) {
  ((e ? (void)hipEventDestroy(e) : void(), e = nullptr), ...);
}
// A grow-only device buffer: the pointer and the bytes it has.  ensure frees the old block BEFORE it allocates the larger one
// (the peak is one block, not two), never shrinks, never zeroes, and leaves {nullptr, 0} behind where the allocation fails.
// No destructor: a handle is destroyed with its device made current first, so release() is explicit like the tables'.
struct DevBuf {
  double *p = nullptr;
  size_t bytes = 0;
  operator double *() const { return p; }
  hipError_t ensure(size_t need) {
    if (bytes >= need) return hipSuccess;
    release();
    const hipError_t e = alloc_device(&p, need);
    if (e == hipSuccess) bytes = need;
    return e;
  }
  void release() {
    free_device(p);
    bytes = 0;
  }
  void release_above(size_t min_bytes) {
    if (bytes > min_bytes) release();
  }
};
// The measurement table of cora_set_measurements (capi/measurements.inc), rows already translated to the internal order,
// structure-of-arrays [field][measurement] on the host and on the device (ResidualArgs, kernels.h)
struct MeasurementTable {
  bool set = false;
  int64_t n_edges = 0, n_ranges = 0;
  std::vector<int32_t> edge_rows, range_rows;  // [4][n_edges], [3][n_ranges]
  std::vector<int32_t> api_edge_rows, api_range_rows;  // [n_edges][4], [n_ranges][3] as given (API rows): the term map of Q(w) is over the CSR
  bool host_stale = false;  // cora_assemble_values_dev rescaled the device's kappa, tau and omega only
  std::vector<double> edge_data, range_data;   // [d*d + d + 2][n_edges], [2][n_ranges]
  int32_t *d_edge_rows = nullptr, *d_range_rows = nullptr;
  double *d_edge_data = nullptr, *d_range_data = nullptr;
  double *d_out = nullptr;  // [n_edges] rotation | [n_edges] translation | [n_ranges] range | 3 sums
  void release() { free_device(d_edge_rows, d_range_rows, d_edge_data, d_range_data, d_out); }
};
// The pair table of cora_set_pose_pairs (capi/rpe.inc): the pairs as given (API pose indices) and translated to internal
// rows, structure-of-arrays [first rotation row of i | translation row of i | first rotation row of j | translation row
// of j][pair] (RpeArgs, kernels.h), and the device's error arrays
struct PosePairTable {
  bool set = false;
  int64_t m = 0;
  std::vector<int32_t> api;   // [m][2]
  std::vector<int32_t> rows;  // [4][m]
  int32_t *d_rows = nullptr;
  double *d_err = nullptr;  // [m] translation | [m] rotation | 5 statistics
  void release() { free_device(d_rows, d_err); }
};
// The chain tables of cora_set_odometry_chains (capi/odom.inc): one entry per chain position (a chain's head, then its
// edges), rows already internal (OdomArgs, kernels.h); the poses in no chain and the landmarks' rows (OdomFillArgs); the
// device copies, the scan's tile totals and carries, the staging of the starts and the landmarks
struct OdomTables {
  bool built = false;  // (false: built at the next initialisation as "no chains", every pose free)
  int64_t n_chains = 0, P = 0;
  std::vector<int32_t> pos_edge, pos_chain, pos_rot, pos_trn;  // [P]
  std::vector<int32_t> free_rot, free_trn, lm_row;
  int32_t *d_idx = nullptr;      // pos_edge | pos_chain | pos_rot | pos_trn | free_rot | free_trn | lm_row
  double *d_work = nullptr;      // totals | carry, kOdomFields(d) x tiles each
  double *d_stage = nullptr;     // starts [n_chains][d] | landmarks [nt - n][d]
  double *h_stage = nullptr;     // the same, pinned
  void release() { free_device(d_idx, d_work, d_stage); free_pinned(h_stage); }
};
// What the initialisers below share.  Every call of theirs ends in the range-row step (range_rows_step, capi/init_common.inc),
// which owns its device arrays on the handle (RangeRowStep below), built at first need and freed with the measurement table.
// Each table struct names its device pointers once, in release(): a table that never reached the handle is released, the
// handle's is freed (free_tables: release, then back to the default state).
struct RangeRowStep {
  int32_t *d_exchanged = nullptr;  // [3][n_ranges] internal rows: range | b | a (the measurement table's with a and b exchanged)
  unsigned char *d_deg = nullptr;  // one byte per range measurement
  void release() { free_device(d_exchanged, d_deg); }
};
// The tables of cora_set_multilateration (capi/multilat.inc): the usable ranges of the measurement table grouped per
// landmark in table order (after the masks), cut into chunks of kMlChunk entries, rows already internal (MlArgs,
// kernels.h); the device copies, the chunks' partial sums, the landmarks' state
struct MlTables {
  bool built = false;
  int64_t n_with_list = 0, usable = 0, skipped = 0;
  std::vector<int32_t> chunk_lm, chunk_begin, chunk_len;  // [chunks]
  std::vector<int32_t> ent_row, ent_m;                    // [entries]
  std::vector<int32_t> lm_chunk0, lm_row, lm_origin;      // [nl + 1], [nl], [nl]
  std::vector<unsigned char> lm_init;                     // [nl]
  int32_t *d_idx = nullptr;  // chunk_lm | chunk_begin | chunk_len | ent_row | ent_m | lm_chunk0 | lm_row | lm_origin
  unsigned char *d_init = nullptr;
  double *d_partial = nullptr;   // [kMlSums(d)][chunks]
  double *d_state = nullptr;     // [nl][kMlState(d)]
  int32_t *d_istate = nullptr;   // [nl][kMlInts]
  // the consensus vote's (cora_multilaterate_robust_dev): scratch of a call, like d_partial
  int32_t *d_votes = nullptr;         // [entries]
  double *d_cstate = nullptr;         // [nl][kMlCState(d)]
  int32_t *d_cint = nullptr;          // [nl][kMlCInts]
  unsigned char *d_inlier = nullptr;  // [n_ranges]
  void release() { free_device(d_idx, d_init, d_partial, d_state, d_istate, d_votes, d_cstate, d_cint, d_inlier); }
};
// The tables of cora_set_chain_placement (capi/placement.inc): the order of the stages, decided from structure alone; per
// stage the chain, its positions in the chain tables, the first entry's rows and the stage's chunks; the entry lists (row
// of the chain's position, row of the anchor, range measurement) in table order, cut into chunks of kPlChunk entries, rows
// already internal (PlArgs, kernels.h); the device copies, the chunks' partial sums, the stages' state
struct PlTables {
  bool built = false;
  int min_ranges = 0;
  int64_t skipped = 0, max_chunks = 0;
  std::vector<int32_t> stage_chain, stage_chunk0;             // [stages], [stages + 1]
  std::vector<int32_t> stage_origin_q, stage_origin_a, stage_pos0, stage_npos;  // [stages]
  std::vector<int32_t> chunk_begin, chunk_len;                // [chunks]
  std::vector<int32_t> ent_q, ent_a, ent_m;                   // [entries]
  std::vector<unsigned char> chain_init;                      // [chains]: 0 a stage | 1 too few entries | 3 no entry | 4 fixed
  // the levels (cora_place_chains_batched_dev): stages whose lists name only chains of earlier levels, so independent of
  // each other; the greedy order stores every stage as a level of its own
  int order = 0;                                              // CORA_PL_ORDER_GREEDY | CORA_PL_ORDER_LEVELS
  int64_t max_level_chunks = 0;
  std::vector<int32_t> level_stage0, level_tile0;             // [levels + 1]: into the stages, into the apply tiles
  std::vector<int32_t> chunk_stage;                           // [chunks]
  std::vector<int32_t> tile_stage, tile_off;                  // [tiles]: 256 positions of one chain, from tile_off within it
  int32_t *d_idx = nullptr;      // chunk_begin | chunk_len | ent_q | ent_a | ent_m | chunk_stage | stage_chunk0 | stage_origin_q | stage_origin_a | stage_pos0 | stage_npos | tile_stage | tile_off
  double *d_partial = nullptr;   // [kPlSums(d)][max_level_chunks] (>= max_chunks)
  double *d_state = nullptr;     // [stages][kPlState(d)]
  int32_t *d_istate = nullptr;   // [stages][kPlInts]
  // the consensus vote's (cora_place_chains_robust_dev): scratch of a call, like d_partial; made at the first robust call
  int32_t *d_votes = nullptr;         // [entries]
  double *d_hyp = nullptr;            // [kPlG(d)][entries]
  double *d_cstate = nullptr;         // [stages][kPlCState(d)]
  int32_t *d_cint = nullptr;          // [stages][kPlCInts]
  unsigned char *d_inlier = nullptr;  // [n_ranges]
  void release() { free_device(d_idx, d_partial, d_state, d_istate, d_votes, d_hyp, d_cstate, d_cint, d_inlier); }
};
// The tables of cora_set_sighting_placement (capi/sighting.inc): the order of the stages, decided from structure alone; per
// stage its kind and its lists; per list the landmark or chain and its chunks; the entries (first rotation row and
// translation row of the pose, row of the landmark, edge) in table order, cut into chunks of kSgChunk entries, rows already
// internal; the positions of every C-stage's chains (SgArgs, kernels.h); the device copies, the chunks' partial sums, the
// lists' state
struct SgTables {
  bool built = false;
  int min_sightings = 0;
  int64_t skipped = 0;
  std::vector<int32_t> stage_kind, stage_list0, stage_apply0;  // [stages] 0 L | 1 C | 2 REFIT, [stages + 1], [stages + 1]
  std::vector<int32_t> list_item, list_chunk0, list_row;       // [lists] landmark or chain, [lists + 1], [lists]
  std::vector<int32_t> chunk_begin, chunk_len, chunk_list;     // [chunks]
  std::vector<int32_t> ent_rot, ent_trn, ent_lm, ent_e;        // [entries]
  std::vector<int32_t> apply_pos, apply_list;                  // [positions of all C-stages]
  std::vector<unsigned char> chain_init, lm_init;  // [chains] 0 taken | 1 never taken | 3 no sighting | 4 fixed; [landmarks] 0 in the REFIT | 1 | 3 fixed
  std::vector<int32_t> chain_list, lm_list;        // [chains], [landmarks]: the C-stage list of the chain, the REFIT list of the landmark (-1: none)
  int32_t *d_idx = nullptr;      // chunk_begin | chunk_len | chunk_list | list_chunk0 | list_row | ent_rot | ent_trn | ent_lm | ent_e | apply_pos | apply_list
  double *d_partial = nullptr;   // [kSgMaxSums(d)][chunks]
  double *d_state = nullptr;     // [lists][kSgState(d)]
  int32_t *d_istate = nullptr;   // [lists][kSgInts]
  // the consensus vote's (cora_place_by_sightings_robust_dev): scratch of a call, like d_partial
  int32_t *d_votes = nullptr;         // [entries]
  double *d_hyp = nullptr;            // [kSgCState(d)][entries]
  double *d_cstate = nullptr;         // [lists][kSgCState(d)]
  int32_t *d_cint = nullptr;          // [lists][kSgCInts]
  unsigned char *d_inlier = nullptr;  // [2][n_edges]: chain lists | landmark lists
  void release() { free_device(d_idx, d_partial, d_state, d_istate, d_votes, d_hyp, d_cstate, d_cint, d_inlier); }
};
// The tables of cora_set_closure_placement (capi/closure.inc): the order of the stages, decided from structure alone; per
// stage its lists; per list the chain and its chunks; the entries (edge, direction) in table order, cut into chunks of
// kClChunk entries; the positions of every stage's chains (ClArgs, kernels.h); the device copies, the chunks' partial sums,
// the lists' state, the consensus vote's scratch
struct ClTables {
  bool built = false;
  int min_closures = 0;
  int64_t skipped = 0, unused = 0;  // non-chain relative-pose edges that are no closure; closures in no list
  std::vector<int32_t> stage_list0, stage_apply0;              // [stages + 1]
  std::vector<int32_t> list_item, list_chunk0;                 // [lists] chain, [lists + 1]
  std::vector<int32_t> chunk_begin, chunk_len, chunk_list;     // [chunks]
  std::vector<int32_t> ent_e, ent_dir;                         // [entries]
  std::vector<int32_t> apply_pos, apply_list;                  // [positions of all stages]
  std::vector<unsigned char> chain_init;  // [chains] 0 taken | 1 never taken | 3 no inter-chain closure | 4 fixed
  std::vector<int32_t> chain_list;        // [chains]: the list of the chain (-1: none)
  int32_t *d_idx = nullptr;      // chunk_begin | chunk_len | chunk_list | list_chunk0 | ent_e | ent_dir | apply_pos | apply_list
  double *d_partial = nullptr;   // [kClSums(d)][chunks]
  double *d_state = nullptr;     // [lists][kSgState(d)]
  int32_t *d_istate = nullptr;   // [lists][kSgInts]
  // the consensus vote's (cora_place_by_closures_robust_dev): scratch of a call, like d_partial
  int32_t *d_votes = nullptr;       // [entries]
  double *d_cstate = nullptr;       // [lists][kClCState(d)]
  int32_t *d_cint = nullptr;        // [lists][kClCInts]
  unsigned char *d_inlier = nullptr;  // [n_edges]
  void release() { free_device(d_idx, d_partial, d_state, d_istate, d_votes, d_cstate, d_cint, d_inlier); }
};
struct cora_ctx {
  HostFormat F;
  LongImage LI;  // what the long rows' device arrays hold (long_image.h); derived from F at creation, device handles only
  MeasurementTable meas;
  PosePairTable pairs;
  OdomTables odom;
  RangeRowStep range_step;
  MlTables ml;
  PlTables pl;
  SgTables sg;
  ClTables cl;
  cora_native_comm *native_comm = nullptr;  // owned: the library's own communication (cora_comm_create_*)
  cora::P2PState *p2p_pending = nullptr;    // a mailbox exported by cora_comm_p2p_handle, not yet connected
  int device = -1;
  bool has_device = false;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int p = 0, ld = 0;

  SliceDesc *d_slices = nullptr;
  SliceDesc *d_slices_pf = nullptr;  // HostFormat::slices_pose_first (empty: nullptr)
  // partitioned handles: the slices that read only rows of this rank's own shard ("interior") and the ones that read a
  // row another rank owns ("boundary"), both in chain order.  With the library's own communication the interior slices
  // run while the exchange of the operand is still under way on comm_stream (exchange_and_product)
  SliceDesc *d_slices_int = nullptr, *d_slices_bnd = nullptr;
  int n_slices_int = 0, n_slices_bnd = 0;
  hipStream_t comm_stream = nullptr;
  int overlap_exchange = 1;  // cora_comm_overlap_enable: 0 never, 1 when the interior part is worth a launch of its own, 2 always
  double *d_sval = nullptr;
  double *d_head_val = nullptr;  // HostFormat::head_val
  int32_t *d_scol = nullptr;
  int32_t *d_perm = nullptr;
  LongChunk *d_chunks = nullptr;
  int32_t *d_chunk_order = nullptr;
  double *d_lval = nullptr;
  int32_t *d_lcol = nullptr;
  double *d_partials = nullptr;
  unsigned *d_tickets = nullptr;
  int32_t *d_api2int = nullptr;
  double *d_diag_inv = nullptr;  // 1/diag(Q), local rows
  double *d_lam_st = nullptr, *d_lam_ob = nullptr;
  // [pose slice][kSymEl(d)][64] (HostFormat::own_sym): sym(Q_PP) as uploaded, and S_P = sym(Q_PP) - Lambda_P of the
  // current point, which the pose slices' epilogues read instead of their own block and Lambda (k_point_finish writes it)
  double *d_own_sym = nullptr, *d_S = nullptr;
  // partitioned handles: distributed long rows (HostFormat::long_rows): partial-sum slots, rows, owners
  double *d_long_out = nullptr;
  int32_t *d_long_rows = nullptr, *d_long_owner = nullptr;
  void release_format() {
    free_device(d_slices, d_slices_pf, d_slices_int, d_slices_bnd, d_sval, d_head_val, d_scol, d_perm, d_chunks, d_chunk_order,
                d_lval, d_lcol, d_partials, d_tickets, d_api2int, d_diag_inv, d_lam_st, d_lam_ob, d_own_sym, d_S, d_long_out,
                d_long_rows, d_long_owner);
  }

  // sparse Cholesky factors resident on the device (level-scheduled triangular solves):
  // the preconditioner's (Q + lambda I)[0:m] and, for the translation-implicit formulation,
  // the translation Laplacian Q33[0:nt-1]
  using DevStage = cora::DevStage;
  // The device sink of walk_tri_image.  A factor's arrays live in a few large device chunks handed out front to back (60
  // arrays per factor: one allocation and one free each cost more than the copies); a re-installed factor writes over the
  // chunks of the one before (rewind).  After a failed call `error` is set and put does nothing more.
  struct DevArena {
    std::vector<void *> allocs;
    std::vector<size_t> chunk_bytes;
    size_t chunk_at = 0, chunk_used = 0;
    hipError_t error = hipSuccess;
    void release() {
      for (void *&p : allocs) free_device(p);
      *this = DevArena();
    }
    void rewind() {
      chunk_at = 0;
      chunk_used = 0;
      error = hipSuccess;
    }
    void scalar(int64_t) {}
    template <class T>
    const T *put(const std::vector<T> &vec) {
      if (error != hipSuccess) return nullptr;
      const size_t bytes = (std::max<size_t>(vec.size(), 1) * sizeof(T) + 255) & ~static_cast<size_t>(255);
      while (chunk_at < allocs.size() && chunk_used + bytes > chunk_bytes[chunk_at]) {
        ++chunk_at;
        chunk_used = 0;
      }
      if (chunk_at == allocs.size()) {
        const size_t cb = std::max<size_t>(bytes, static_cast<size_t>(64) << 20);
        void *q = nullptr;
        if ((error = alloc_device(&q, cb)) != hipSuccess) return nullptr;
        allocs.push_back(q);
        chunk_bytes.push_back(cb);
        chunk_used = 0;
      }
      T *p = reinterpret_cast<T *>(static_cast<char *>(allocs[chunk_at]) + chunk_used);
      chunk_used += bytes;
      if (!vec.empty()) error = hipMemcpy(p, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice);  // (vec may be a temporary)
      return p;
    }
  };
  struct DevFactor {
    std::vector<DevStage> stages;
    DevArena arena;
    int aux_rows = 0;  // two-stage plans: rows appended to the work vector
    bool fuse_ok = false;  // substitution blocks whose tiles hold every pose's rotation rows at consecutive positions:
                           // the STPCG passes can be fused into the sweeps (SubFuse, kernels.h)
    bool ready = false;
    int64_t entries[6] = {0, 0, 0, 0, 0, 0};  // cora_precond_entries (counted at install, from the host plan)
    int64_t shape[kShapeFields] = {0};        // cora_debug_factor_shape, cora_precond_stats (the same)
    unsigned long long generation = 0;  // counts installs: a captured STPCG graph carries the plan's arrays and sizes
  };
  DevFactor precond_f, implicit_f, aux_f;  // aux_f: the caller's own factor (cora_aux_set_cholesky)
  void release_factors() {
    for (DevFactor *f : {&precond_f, &implicit_f, &aux_f}) f->arena.release();
  }
  bool implicit = false;  // Formulation::Implicit active

  bool have_point = false;
  double *d_Y = nullptr, *d_G = nullptr, *d_rgrad = nullptr;
  // cora_tnt_trial_dev leaves Q X of its trial point here; cora_tnt_accept_dev of the same point takes it as the new
  // point's Euclidean gradient (the two buffers change places) instead of forming the product again
  double *d_G_trial = nullptr;
  void release_rank_state() { free_device(d_Y, d_G, d_rgrad, d_G_trial); }
  const double *trial_x = nullptr;  // the trial point d_G_trial belongs to (nullptr: none)
  unsigned long long stpcg_pending_seq = 0;  // a neutral iteration of the last inner solve may still be in flight (stpcg_run)
  double f = 0.0;
  int precond = CORA_PRECOND_NONE;

  std::future<void> deferred_free;  // a solve plan's host arrays being freed (install_factor)
  unsigned long long dot_seq = 0;  // h_scalars[7] carries the sequence number of the last finished reduction
  DevBuf scratch[kScratchSlots];
  DevBuf d_stage;
  DevBuf d_red;  // reduction partials
  // two pinned buffers of kPinChunk bytes and their events: big downloads are pipelined through them (DMA into one
  // while the host copies the other out) instead of hipMemcpy's own staging of pageable memory
  char *h_pin[2] = {nullptr, nullptr};
  hipEvent_t ev_pin[2] = {nullptr, nullptr};
  double *d_scalars = nullptr;  // 8 doubles
  StpcgState *d_stpcg = nullptr, *h_stpcg = nullptr;  // device-resident STPCG scalars and their pinned mirror
  unsigned *d_ticket = nullptr;  // last-block ticket of the inner-product kernels (zero between launches)
  unsigned long long *d_seq_counter = nullptr;  // the device's copy of dot_seq (kernels.h, DotArgs::seq_counter)
  double *h_scalars = nullptr;  // pinned, 8 doubles
  double *h_gram = nullptr;     // pinned, 16 x 24 x 24 doubles: where the Gram products' reduction writes its results (need_gram)
  int *d_flag = nullptr;
  int *h_flag = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void release_solver_buffers() {
    for (DevBuf &b : scratch) b.release();
    d_stage.release();
    d_red.release();
    free_device(d_scalars, d_stpcg, d_ticket, d_seq_counter, d_flag);
    free_pinned(h_pin[0], h_pin[1], h_stpcg, h_scalars, h_gram, h_flag);
    free_events(ev_pin[0], ev_pin[1], ev0, ev1);
  }
  // the other events: of the exchange's overlap (partitioned handles), around the assembly kernels (capi/assembly.inc), at the
  // phase boundaries of the one-collective product in serial order (cora_debug_product_phases), and kProfMarks per profiled
  // STPCG iteration (cora_debug_profile_stpcg: event pairs around the Hessian-vector product of every device-resident iteration)
  hipEvent_t ev_operand = nullptr, ev_exchanged = nullptr;
  hipEvent_t asm_ev[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> phase_events;
  std::vector<hipEvent_t> prof_events;
  void release_events() {
    free_events(ev_operand, ev_exchanged, asm_ev[0], asm_ev[1]);
    for (std::vector<hipEvent_t> *v : {&phase_events, &prof_events}) {
      for (hipEvent_t &e : *v) free_events(e);
      v->clear();
    }
  }
  // injected communication of a partitioned handle (cora_set_comm)
  cora_exchange_fn comm_exchange = nullptr;
  cora_allreduce_fn comm_allreduce = nullptr;
  cora_allgather_fn comm_allgather = nullptr;
  void *comm_user = nullptr;
  bool comm_required = false;  // cora_require_comm: a collective step without communication is an error, not a no-op
  bool local_products = false;  // cora_debug_local_products: products skip every collective step (kernel timing only)
  bool phase_timing = false;  // cora_debug_product_phases
  int prof_stpcg = 0;  // 0 off | 1 events around the product of every STPCG iteration | 2 around every launch of it
  double prof_hvp_us = 0.0;
  int prof_hvp_count = 0;
  double prof_phase_us[7] = {0, 0, 0, 0, 0, 0, 0};  // mean time between marks k and k + 1 (-1: not recorded); [6]: two marks in a row
  bool prof_kappa_folded = false;  // the profiled iterations had no kappa launch (SubFuse::n_kappa)
  int stpcg_path = 0;  // iteration form of the last cora_stpcg_dev: 0 unfused, 1 fused vector passes, 2 sweep-fused (two-stage plan), 3 inverse-fused (one-inverse plan)
  // A batch of device-resident STPCG iterations as a hipGraph: the launches of an iteration have the same arguments
  // every time (the scalars live in device memory, the sequence number the host waits for is a device counter), so a
  // batch is captured once and replayed -- replayed launches follow each other 1.3 us closer than launches enqueued
  // one by one (tools/launch_lab.hip) and cost the host one call instead of twenty.  Kept while its key -- every
  // pointer and size the captured launches carry -- stays the same, i.e. normally for a whole TNT call and beyond.
  hipGraphExec_t stpcg_graph = nullptr;
  std::vector<uintptr_t> stpcg_graph_key;
  long stpcg_graph_replays = 0, stpcg_graph_captures = 0;
  // in-place update of Q's values (capi/values.inc): the source map, built at the first update, its device copy
  // (sources of the five arrays at vmap_off, mirror pairs, a staging buffer for host values) and what it needs to know
  ValueMap vmap;
  int32_t *d_vmap_src = nullptr, *d_vmap_mirror = nullptr;
  double *d_vmap_vals = nullptr;
  void release_value_map() { free_device(d_vmap_src, d_vmap_mirror, d_vmap_vals); }
  size_t vmap_off[5] = {0, 0, 0, 0, 0};
  bool dist_long = true;            // the handle was created with distributed long rows (no CORA_PART_WHOLE_LONG_ROWS)
  bool host_values_stale = false;   // cora_update_values_dev moved the device's values only: F's value arrays are old
  double values_ms[5] = {0, 0, 0, 0, 0};  // cora_update_values_times
  // assembly of Q(w) from per-measurement weights (capi/assembly.inc): the term map, its device copy, a device weight
  // vector for the host-pointer form, events around the assembly kernels (asm_ev above) and the times of the last call
  TermMap tmap;
  int32_t *d_tptr = nullptr, *d_tweight = nullptr, *d_tlong = nullptr;
  double *d_tcoef = nullptr, *d_tbase = nullptr, *d_asm_w = nullptr;
  double asm_ms[5] = {0, 0, 0, 0, 0};  // cora_assemble_times
  double *d_gnc = nullptr;  // cora_gnc_weights (capi/gnc.inc): thresholds | weights | residuals of the host-pointer form, 3 n_weights
  void release_assembly() { free_device(d_tptr, d_tweight, d_tlong, d_tcoef, d_tbase, d_asm_w, d_gnc); }
  // trajectory comparison (capi/compare.inc): the pose table (internal rows: first rotation row of every pose | translation
  // row of every pose, then landmark | range rows), built at the first call, its device copy, the selection bytes, one
  // block of doubles (pose translation errors | pose rotation errors | landmark errors | 48 column sums | 6 statistics |
  // A) and the vectors of the pass (centred X, centred Ref; X, Ref, aligned of the host-pointer form) -- its own, so that a
  // call moves none of the handle's scratch vectors
  std::vector<int32_t> cmp_rows;
  std::vector<unsigned char> cmp_sel_host;
  std::vector<double> cmp_H;  // H of the last comparison, k x kr row-major (test hook cora_debug_compare_H)
  int cmp_H_k = 0, cmp_H_kr = 0;
  int32_t *d_cmp_rows = nullptr;
  unsigned char *d_cmp_sel = nullptr;
  double *d_cmp = nullptr;
  DevBuf cmp_vec[5];
  void release_compare() {
    free_device(d_cmp_rows, d_cmp_sel, d_cmp);
    for (DevBuf &v : cmp_vec) v.release();
  }
  std::vector<std::pair<double *, size_t>> user_allocs;  // live vectors of cora_dev_alloc (pointer, bytes)
  std::vector<std::pair<double *, size_t>> pool;         // released ones, kept for the next request of the same size
  void release_vectors() {
    for (auto *v : {&user_allocs, &pool}) {
      for (auto &p : *v) free_device(p.first);
      v->clear();
    }
  }
  std::string err;
};

struct cora_ctx;
static int apply_product(cora_ctx *c, const double *dX, int ld, int epi, double *dOut);  // formulation-aware
static int launch_product(cora_ctx *c, SpmmArgs A, int ld, int epi, bool finish = true);  // one SpMM launch (+ the distributed long rows)
static int finish_long_rows(cora_ctx *c, const SpmmArgs &A, int ld, int epi);
static int exchange_and_product(cora_ctx *c, SpmmArgs A, int ld, int epi);  // exchange of the operand's remote rows + the product
static int product_kappa_slots(const cora_ctx *c, const SpmmArgs &A);

namespace {

int fail(cora_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  else g_create_error = msg;
  return code;
}

#define HIP_TRY(c, expr)                                                              \
  do {                                                                                \
    hipError_t e__ = (expr);                                                          \
    if (e__ != hipSuccess)                                                            \
      return fail((c), CORA_ERR_HIP,                                                  \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                \
  } while (0)

#define NEED_DEVICE(c)                                                                \
  do {                                                                                \
    if (!(c)) return CORA_ERR_ARG;                                                    \
    if (!(c)->has_device)                                                             \
      return fail((c), CORA_ERR_HIP, "no HIP device bound to this handle (plan-only)"); \
    HIP_TRY((c), hipSetDevice((c)->device));                                          \
  } while (0)

#define NEED_RANK(c)                                                                  \
  do {                                                                                \
    if ((c)->p <= 0) return fail((c), CORA_ERR_NOT_READY, "cora_set_rank not called"); \
  } while (0)

// A kept trial product (cora_tnt_trial_dev) belongs to the CONTENTS of a vector, not to its address: every entry point that
// can write a caller's vector, or hand its address out again, says so here (round-5 advice: an accept after such a write
// silently took a stale Euclidean gradient).
inline void wrote(cora_ctx *c, const void *p) {
  if (c && p && p == c->trial_x) c->trial_x = nullptr;
}

template <typename T>
hipError_t to_device(T **dptr, const std::vector<T> &v) {
  const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  hipError_t e = alloc_device(dptr, bytes);
  if (e != hipSuccess) return e;
  if (!v.empty()) e = hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

size_t vec_bytes(const cora_ctx *c, int ld) {
  return static_cast<size_t>(c->F.L.rows) * ld * sizeof(double);
}

int get_scratch(cora_ctx *c, int slot, int ld, double **out, int64_t extra_rows = 0) {
  const size_t need = vec_bytes(c, ld) + static_cast<size_t>(extra_rows) * ld * sizeof(double);
  HIP_TRY(c, c->scratch[slot].ensure(need));
  *out = c->scratch[slot];
  return CORA_OK;
}

// the pinned block the Gram products' reduction writes its results to, made at first need
int need_gram(cora_ctx *c) {
  if (!c->h_gram) HIP_TRY(c, alloc_pinned(&c->h_gram, 16 * kMaxLD * kMaxLD * sizeof(double)));
  return CORA_OK;
}

// collective steps of a partitioned handle; no-ops on a single-GPU one
// (a partitioned handle WITHOUT communication keeps the round-1 contract: the caller keeps the rows the products
// read current and adds up the per-rank partial results itself)
int comm_missing(cora_ctx *c) {
  if (!c->comm_required) return CORA_OK;
  return fail(c, CORA_ERR_NOT_READY,
              "partitioned handle without communication: install it with cora_set_comm or cora_comm_create_* (again after "
              "every rebuild of the handle, e.g. Problem::updateProblemData or a second setPartition)");
}
int comm_exchange(cora_ctx *c, const double *dX, int ld) {
  if (c->F.L.world == 1) return CORA_OK;
  if (!c->comm_exchange) return comm_missing(c);
  if (c->comm_exchange(c->comm_user, const_cast<double *>(dX), ld)) return fail(c, CORA_ERR_HIP, "exchange step failed");
  return CORA_OK;
}
int comm_allreduce(cora_ctx *c, double *vals, int n) {
  if (c->F.L.world == 1) return CORA_OK;
  if (!c->comm_allreduce) return comm_missing(c);
  if (c->comm_allreduce(c->comm_user, vals, n)) return fail(c, CORA_ERR_HIP, "all-reduce step failed");
  return CORA_OK;
}
int comm_allgather(cora_ctx *c, const double *dX, int ld) {
  if (c->F.L.world == 1) return CORA_OK;
  if (!c->comm_allgather) return comm_missing(c);
  if (c->comm_allgather(c->comm_user, const_cast<double *>(dX), ld)) return fail(c, CORA_ERR_HIP, "all-gather step failed");
  return CORA_OK;
}

RowArgs row_args(const cora_ctx *c) {
  const Layout &L = c->F.L;
  RowArgs R;
  R.d = L.d;
  R.nl_poses = L.nl_poses;
  R.nl_ranges = L.nl_ranges;
  R.nl_trans = L.nl_trans;
  R.rot_base = static_cast<size_t>(L.rot_base);
  R.rng_base = static_cast<size_t>(L.rng_base);
  R.trn_base = static_cast<size_t>(L.trn_base);
  R.base = static_cast<size_t>(L.base);
  return R;
}

SpmmArgs spmm_args(const cora_ctx *c, const double *X, double *out) {
  SpmmArgs A;
  A.slices = c->d_slices;
  A.slices_pose_first = c->d_slices_pf;
  A.n_slices = static_cast<int>(c->F.slices.size());
  A.n_chunks = static_cast<int>(c->LI.chunk_order.size());  // launch positions of the image: its pieces and the padding of the XCDs' lists
  A.sval = c->d_sval;
  A.head_val = c->d_head_val;
  A.scol = c->d_scol;
  A.perm = c->d_perm;
  A.chunks = c->d_chunks;
  A.chunk_order = c->d_chunk_order;
  A.lval = c->d_lval;
  A.lcol = c->d_lcol;
  A.partials = c->d_partials;
  A.tickets = c->d_tickets;
  A.n_long_rows = c->F.n_long_rows;
  A.X = X;
  A.out = out;
  A.Y = c->d_Y;
  A.lam_st = c->d_lam_st;
  A.lam_ob = c->d_lam_ob;
  A.S = c->d_S;
  const Layout &L = c->F.L;
  A.win_rot_lo = static_cast<int32_t>(L.rot_base);
  A.win_rot_hi = static_cast<int32_t>(L.rot_base + static_cast<int64_t>(L.nl_poses) * L.d);
  A.win_trn_lo = static_cast<int32_t>(L.trn_base);
  A.win_trn_hi = static_cast<int32_t>(L.trn_base + L.nl_trans);
  A.n_local_poses = L.nl_poses;
  return A;
}

int ensure_red(cora_ctx *c, size_t doubles) {
  HIP_TRY(c, c->d_red.ensure(doubles * sizeof(double)));
  return CORA_OK;
}

// host col-major (N x k, ld) -> resident vector (rows x ld_for(k)), zero padded
int upload_impl(cora_ctx *c, const double *host, int ldh, int k, double *dptr) {
  const int64_t N = c->F.L.N;
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  if (ldh < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  if (!host || !dptr) return fail(c, CORA_ERR_ARG, "null pointer");
  const int ld = ld_for(k);
  const size_t need = static_cast<size_t>(N) * k * sizeof(double);
  HIP_TRY(c, c->d_stage.ensure(need));
  HIP_TRY(c, hipMemcpy2DAsync(c->d_stage, N * sizeof(double), host, static_cast<size_t>(ldh) * sizeof(double),
                              N * sizeof(double), k, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(dptr, 0, vec_bytes(c, ld), c->stream));
  HIP_TRY(c, launch_upload(N, k, ld, c->d_stage, c->d_api2int, dptr, c->stream));
  return CORA_OK;
}

int download_impl(cora_ctx *c, const double *dptr, int k, double *host, int ldh) {
  const int64_t N = c->F.L.N;
  if (k <= 0 || k > kMaxLD) return fail(c, CORA_ERR_SHAPE, "column count must be in [1, 24]");
  if (ldh < N) return fail(c, CORA_ERR_SHAPE, "leading dimension smaller than N");
  if (!host || !dptr) return fail(c, CORA_ERR_ARG, "null pointer");
  const int ld = ld_for(k);
  const size_t need = static_cast<size_t>(N) * k * sizeof(double);
  HIP_TRY(c, c->d_stage.ensure(need));
  {
    const int rc = comm_allgather(c, dptr, ld);
    if (rc) return rc;
  }
  HIP_TRY(c, launch_download(N, k, ld, dptr, c->d_api2int, c->d_stage, c->stream));
  constexpr size_t kPinChunk = size_t(8) << 20;
  if (ldh == N && need >= 4 * kPinChunk) {
    // One flat block of `need` bytes.  hipMemcpy into pageable memory stages through the runtime's own bounce buffer
    // (measured 4.4 GB/s: 0.1 s for the 430 MB Ritz block of a 10^6-pose certification); here the DMA engine fills one
    // pinned chunk while host threads copy the previous one out.
    for (int i = 0; i < 2; ++i) {
      if (!c->h_pin[i]) HIP_TRY(c, alloc_pinned(&c->h_pin[i], kPinChunk));
      if (!c->ev_pin[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_pin[i], hipEventDisableTiming));
    }
    const char *src = reinterpret_cast<const char *>(c->d_stage.p);
    char *dst = reinterpret_cast<char *>(host);
    const size_t nchunks = (need + kPinChunk - 1) / kPinChunk;
    auto bytes_of = [&](size_t ch) { return std::min(kPinChunk, need - ch * kPinChunk); };
    auto start = [&](size_t ch) -> hipError_t {
      const hipError_t e = hipMemcpyAsync(c->h_pin[ch & 1], src + ch * kPinChunk, bytes_of(ch), hipMemcpyDeviceToHost, c->stream);
      return e != hipSuccess ? e : hipEventRecord(c->ev_pin[ch & 1], c->stream);
    };
    HIP_TRY(c, start(0));
    const unsigned nth = std::min(4u, std::max(1u, std::thread::hardware_concurrency()));
    for (size_t ch = 0; ch < nchunks; ++ch) {
      HIP_TRY(c, hipEventSynchronize(c->ev_pin[ch & 1]));
      if (ch + 1 < nchunks) HIP_TRY(c, start(ch + 1));  // (the other buffer: its host copy finished in the round before)
      const size_t nb = bytes_of(ch);
      const char *from = c->h_pin[ch & 1];
      char *to = dst + ch * kPinChunk;
      cora::parallel_parts(nth, [&](unsigned t) {
        const size_t a = nb * t / nth, b = nb * (t + 1) / nth;
        std::memcpy(to + a, from + a, b - a);
      });
    }
    return CORA_OK;
  }
  HIP_TRY(c, hipMemcpy2DAsync(host, static_cast<size_t>(ldh) * sizeof(double), c->d_stage, N * sizeof(double),
                              N * sizeof(double), k, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CORA_OK;
}

// Lambda, grad and f from (Y, G) already resident in d_Y / d_G.
// wait == false (one GPU): nothing is waited for -- f arrives in h_scalars[4] (pinned) before whatever the caller enqueues
// next on the stream finishes, and the caller stores it in c->f after its own wait.
int point_finish(cora_ctx *c, bool wait = true) {
  const RowArgs R = row_args(c);
  const int64_t units = static_cast<int64_t>(R.nl_poses) + R.nl_ranges + R.nl_trans;
  const int nb = static_cast<int>((units + 255) / 256);
  int rc = ensure_red(c, static_cast<size_t>(std::max(nb, 1)) * 4);
  if (rc) return rc;
  int nblocks = 0;
  HIP_TRY(c, launch_point_finish(R, c->ld, c->d_Y, c->d_G, c->d_rgrad, c->d_lam_st, c->d_lam_ob, c->d_own_sym, c->d_S, c->d_red,
                                 &nblocks, c->stream));
  if (!wait) {
    c->h_scalars[4] = 0.0;
    if (nblocks > 0) HIP_TRY(c, launch_reduce_partials(c->d_red, nblocks, 1, c->h_scalars + 4, c->stream));
    c->have_point = true;
    return CORA_OK;
  }
  if (nblocks > 0) {
    HIP_TRY(c, launch_reduce_partials(c->d_red, nblocks, 1, c->h_scalars, c->stream));  // pinned host memory
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->f = c->h_scalars[0];
  } else {
    c->f = 0.0;
  }
  if ((rc = comm_allreduce(c, &c->f, 1))) return rc;
  c->have_point = true;
  return CORA_OK;
}

// Wait for the inner-product kernel that was just launched: its last block writes the results and then
// the sequence number into pinned memory, which the host polls -- a few microseconds less than a stream
// synchronisation, twice per STPCG iteration.  Falls back to the stream if the number never arrives.
int wait_dots(cora_ctx *c, unsigned long long seq) {
  volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(c->h_scalars + 7);
  for (long spin = 0; spin < 20000000L; ++spin)
    if (*flag >= seq) return CORA_OK;  // (numbers only grow on a handle; a later reduction may already have finished)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return *flag >= seq ? CORA_OK : fail(c, CORA_ERR_HIP, "inner-product kernel did not complete");
}

int set_point_dev_impl(cora_ctx *c, const double *dY) {
  c->trial_x = nullptr;
  if (dY != c->d_Y)
    HIP_TRY(c, hipMemcpyAsync(c->d_Y, dY, vec_bytes(c, c->ld), hipMemcpyDeviceToDevice, c->stream));
  const int rc = apply_product(c, c->d_Y, c->ld, EPI_NONE, c->d_G);
  if (rc) return rc;
  return point_finish(c);
}

void free_assembly(cora_ctx *c) {  // (the device must be current where there is one)
  c->release_assembly();
  c->tmap = TermMap();
}

template <class T>
void free_tables(T &t) {  // (the device must be current where there is one)
  t.release();
  t = T();
}

void free_measurements(cora_ctx *c) {  // (the device must be current)
  free_assembly(c);            // (the term map belongs to the table)
  free_tables(c->odom);        // (so do the chain tables: their positions name its edges)
  free_tables(c->range_step);  // (and the exchanged range rows)
  free_tables(c->ml);          // (and the multilateration's lists: their entries name its ranges)
  free_tables(c->pl);          // (and the chain placement's stages)
  free_tables(c->sg);          // (and the sighting placement's lists: their entries name its edges)
  free_tables(c->cl);          // (and the closure placement's lists: their entries name its edges)
  free_tables(c->meas);
}

void free_rank_state(cora_ctx *c) {
  c->release_rank_state();
  c->trial_x = nullptr;
  c->have_point = false;
}

}  // namespace

extern "C" {
#include "capi/handle.inc"
#include "capi/resident.inc"
#include "capi/preconditioner.inc"
#include "capi/products.inc"
#include "capi/solver_ops.inc"
#include "capi/stpcg.inc"
#include "capi/blocks.inc"
#include "capi/host_pointer.inc"
#include "capi/measurements.inc"
#include "capi/values.inc"
#include "capi/assembly.inc"
#include "capi/gnc.inc"
#include "capi/compare.inc"
#include "capi/rpe.inc"
#include "capi/round.inc"
#include "capi/init_common.inc"
#include "capi/odom.inc"
#include "capi/multilat.inc"
#include "capi/placement.inc"
#include "capi/sighting.inc"
#include "capi/closure.inc"

}  // extern "C"

#include "capi/comm.inc"
