// The DEVICE IMAGE of a solve plan: everything the kernels of the staged Cholesky solve read that the plan (trisolve.h)
// does not hold -- the descriptors of the substitution blocks, their memory-order I/O lists, tile positions, run tables
// and row units, the packed lanes of dense blocks, the chunk rows of the row products -- and the two decisions taken on
// the way: io_runs (how k_subblock forms its global addresses) and fuse_ok (whether the sweeps can take the projection
// and the STPCG passes).  Derived on the host, without a device: build_tri_image.  What is uploaded is plan + image, and
// walk_tri_image is the one list of it: it hands every array to a sink, in upload order, and keeps the pointer the sink
// returns -- the device arena of an install (capi.hip), or a digest that covers exactly what an install uploads.
#pragma once

#include <hip/hip_vector_types.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "config.h"
#include "kernels.h"
#include "trisolve.h"

namespace cora {

// What the image needs to know of the vectors the solve runs on.
struct ImageLayout {
  int d = 0;                   // rotation rows of a pose
  int64_t rot0 = 0, rot1 = 0;  // internal rows [rot0, rot1) are rotation rows, pose by pose
  int64_t rows = 0;            // rows of a vector
  bool grouped = false;        // the plan was built with a group vector (build_tri_plan: a pose's rotation rows share a block)
};

struct RowOpImage {
  bool live = false;               // the product is launched by factor_solve (and uploaded)
  std::vector<int32_t> chunk_row;  // RowOpDev::chunk_row
  size_t tickets = 0, partial = 0; // elements of the zeroed RowOpDev::tickets / partial
};
struct SubImage {
  std::vector<SubDesc> desc;
  std::vector<int2> io_f, io_b;         // SubSweep::io of the forward / backward sweep
  std::vector<uint16_t> tpos_f, tpos_b; // SubSweep::tpos
  std::vector<int2> b_unit;             // SubOpDev::b_unit
};
struct BlockImage {
  std::vector<BlockDesc> desc;
  std::vector<BlockLane> by_col, by_row;
};
struct StageImage {
  bool has_fwd_a = false, has_bwd_a = false, dense = false, is_sub = false, aux_sum = false;  // the flags of a device stage
  RowOpImage fwd_a, fwd_b, bwd_a, bwd_b;
  SubImage sub;
  BlockImage blocks;
};
// Owns the derived arrays only; everything else is read from the plan it was built from (no second copy of the plan's
// arrays: the substitution arrays are 130 MB at 10^5 poses).
struct TriImage {
  std::vector<StageImage> stages;
  int io_runs = -1;      // substitution plans: 1 run tables, 0 index lists (SubOpDev::io_runs); -1: no substitution stage
  bool fuse_ok = false;  // substitution blocks whose tiles hold every pose's rotation rows at consecutive positions
  int aux_rows = 0;      // two-stage plans: rows appended to the work vector
};

// Derives the image of `plan`.  The plan's own arrays stay where they are, but the tails the kernels' prefetches read
// past their ends are appended to them in place (so a plan is given to this function once).  tick: the phases' times
// (CORA_TRI_TIMING).  CORA_SUB_IO_LISTS is read here, per call.
void build_tri_image(TriPlan &plan, const ImageLayout &layout, TriImage &image, PhaseTimer &tick);

// The device's view of one stage: the argument blocks of its launches (filled by walk_tri_image) and the flags
// factor_solve chooses them by (StageImage's).
struct DevStage {
  RowOpDev fwd_a{}, fwd_b{}, bwd_a{}, bwd_b{};
  BlockOpDev blocks{};
  SubOpDev sub{};
  bool has_fwd_a = false, has_bwd_a = false, dense = false, is_sub = false, aux_sum = false;
};

// Visits every array of plan + image in upload order.  Sink: `const T *put(const std::vector<T> &)` takes an array and
// returns where the kernels will find it; `void scalar(int64_t)` is told every scalar member of the argument blocks.
template <class Sink>
void walk_row_op(Sink &s, const RowOpHost &H, const RowOpImage &I, RowOpDev &D) {
  D.n8 = H.n8;
  D.n64 = H.n64;
  D.nlong = static_cast<int>(H.long_out.size());
  D.nchunks = static_cast<int>(H.chunk_begin.size());
  for (int v : {D.n8, D.n64, D.nlong, D.nchunks}) s.scalar(v);
  D.out_row = s.put(H.out_row);
  D.begin = s.put(H.begin);
  D.end = s.put(H.end);
  D.long_out = s.put(H.long_out);
  D.long_chunk_ptr = s.put(H.long_chunk_ptr);
  D.chunk_begin = s.put(H.chunk_begin);
  D.chunk_end = s.put(H.chunk_end);
  D.col = s.put(H.col);
  D.val = s.put(H.val);
  D.chunk_row = s.put(I.chunk_row);
  D.tickets = const_cast<unsigned *>(s.put(std::vector<unsigned>(I.tickets, 0u)));
  D.partial = const_cast<double *>(s.put(std::vector<double>(I.partial, 0.0)));
}

template <class Sink>
void walk_sub_op(Sink &s, const TriPlan &plan, const SubBlockOpHost &H, const SubImage &I, int io_runs, SubOpDev &Q) {
  Q.nblocks = static_cast<int>(I.desc.size());
  Q.ntop = static_cast<int>(plan.top_rows.size());
  Q.max_rows = H.max_rows;
  Q.max_ent = H.max_ent;
  Q.max_lev = H.max_lev;
  Q.max_level_lanes = H.max_level_lanes;
  Q.max_npl = H.max_npl;
  Q.aux_base = plan.aux_base;
  Q.io_runs = io_runs;
  for (int v : {Q.nblocks, Q.ntop, Q.max_rows, Q.max_ent, Q.max_lev, Q.max_level_lanes, Q.max_npl, Q.aux_base}) s.scalar(v);  // (io_runs: with the decisions, at the end)
  Q.fwd.rows = s.put(H.rows);
  Q.fwd.hdr = s.put(H.f_hdr);
  Q.fwd.idx = s.put(H.f_idx);
  Q.fwd.val = s.put(H.f_val);
  Q.bwd.rows = s.put(H.b_rows);
  Q.bwd.hdr = s.put(H.b_hdr);
  Q.bwd.idx = s.put(H.b_idx);
  Q.bwd.val = s.put(H.b_val);
  Q.tgt_row = s.put(H.tgt_row);
  Q.tgt_slot = s.put(H.tgt_slot);
  Q.c_ptr = s.put(H.c_ptr);
  Q.c_idx = s.put(H.c_idx);
  Q.c_val = s.put(H.c_val);
  Q.top_rows = s.put(plan.top_rows);
  Q.fwd.io = s.put(I.io_f);
  Q.bwd.io = s.put(I.io_b);
  Q.fwd.tpos = s.put(I.tpos_f);
  Q.bwd.tpos = s.put(I.tpos_b);
  Q.b_unit = s.put(I.b_unit);
  Q.desc = s.put(I.desc);
}

template <class Sink>
void walk_block_op(Sink &s, const BlockOpHost &H, const BlockImage &I, BlockOpDev &B) {
  B.nblocks = static_cast<int>(H.nrows.size());
  s.scalar(B.nblocks);
  B.desc = s.put(I.desc);
  B.by_col = s.put(I.by_col);
  B.by_row = s.put(I.by_row);
  B.w_by_col = s.put(H.w_by_col);
  B.w_by_row = s.put(H.w_by_row);
  B.ext_ptr = s.put(H.ext_ptr);
  B.ext_col = s.put(H.ext_col);
  B.ext_val = s.put(H.ext_val);
}

template <class Sink>
void walk_tri_image(Sink &s, const TriPlan &plan, const TriImage &image, std::vector<DevStage> &dev) {
  dev.assign(plan.stages.size(), DevStage());
  for (size_t k = 0; k < plan.stages.size(); ++k) {
    const TriStage &S = plan.stages[k];
    const StageImage &I = image.stages[k];
    DevStage &D = dev[k];
    if (I.is_sub) {
      walk_sub_op(s, plan, S.sub_op, I.sub, image.io_runs, D.sub);
      continue;
    }
    if (I.fwd_a.live) walk_row_op(s, S.fwd_a, I.fwd_a, D.fwd_a);
    if (I.dense) {
      walk_block_op(s, S.blocks_op, I.blocks, D.blocks);
      continue;
    }
    if (I.fwd_b.live) walk_row_op(s, S.fwd_b, I.fwd_b, D.fwd_b);
    if (I.bwd_a.live) walk_row_op(s, S.bwd_a, I.bwd_a, D.bwd_a);
    if (I.bwd_b.live) walk_row_op(s, S.bwd_b, I.bwd_b, D.bwd_b);
  }
  for (int v : {image.io_runs, int(image.fuse_ok), image.aux_rows}) s.scalar(v);
}

// The digest sink: FNV-1a as tri_plan_digest's -- per array its element size and length, then its bytes; integers and
// indices into h[0], doubles into h[1]; scalars into h[0].  It returns null pointers.
struct ImageDigest {
  uint64_t h[2] = {0xcbf29ce484222325ull, 0xcbf29ce484222325ull};
  void bytes(int which, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) h[which] = (h[which] ^ b[i]) * 0x100000001b3ull;
  }
  void scalar(int64_t v) { bytes(0, &v, sizeof v); }
  template <class T>
  const T *put(const std::vector<T> &v) {
    const int which = std::is_floating_point<T>::value ? 1 : 0;
    const uint64_t head[2] = {sizeof(T), v.size()};
    bytes(which, head, sizeof head);
    bytes(which, v.data(), v.size() * sizeof(T));
    return nullptr;
  }
};

// Test hook (cora_debug_factor_image): the digest of everything an install of plan + image uploads, and the shape of the
// plan with the fields the image decides (kShapeIoRuns, kShapeFuseOk) filled in.
void tri_image_digest(const TriPlan &plan, const TriImage &image, uint64_t out[2]);
void tri_image_shape(const TriPlan &plan, const TriImage &image, int64_t out[kShapeFields]);

}  // namespace cora
