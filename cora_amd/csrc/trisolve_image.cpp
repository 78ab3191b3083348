// The device image of a solve plan, derived on the host (trisolve_image.h).  No HIP runtime call in this file.
#include "trisolve_image.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <thread>

#include "parallel.h"

namespace cora {
namespace {

// ---- block descriptors
std::vector<SubDesc> sub_descriptors(const SubBlockOpHost &H) {
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
  return desc;
}

// ---- over-read tails, appended to the plan's own arrays
void sub_tails(SubBlockOpHost &H) {
  H.f_hdr.resize(H.f_hdr.size() + 8, 0);  // the kernel reads one header ahead
  H.f_idx.resize(H.f_idx.size() + 8, 0);  // ... and an entry past a block without entries
  H.f_val.resize(H.f_val.size() + 8, 0.0);
  H.b_idx.resize(H.b_idx.size() + 8, 0);
  H.b_val.resize(H.b_val.size() + 8, 0.0);
  H.b_hdr.resize(H.b_hdr.size() + 8, 0);
}

// ---- I/O lists
// memory-order I/O list of one sweep: {internal row, tile position} of every block row, sorted by row
std::vector<int2> io_list(const std::vector<int32_t> &rows, const std::vector<SubDesc> &desc) {
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
  parallel_parts(nth, part);
  io.back() = make_int2(0, 0);
  return io;
}

// ---- run tables and io_runs
// (the rows of a block in memory order are the same set for both sweeps: the runs are found once, from the forward
// list; only the tile positions differ)
bool run_tables(SubImage &I) {
  bool runs_ok = !env_flag(Env::SubIoLists);  // (lab switch: the 8-byte index lists)
  const std::vector<int2> &iof = I.io_f, &iob = I.io_b;
  I.tpos_f.assign(iof.size() + 8, 0);
  I.tpos_b.assign(iob.size() + 8, 0);
  for (SubDesc &d : I.desc) {
    const int32_t r0 = d.row_begin, nb = d.nrows;
    int nr = 0;
    for (int q = 0; q < kSubMaxRuns; ++q) { d.run_off[q] = 0; d.run_end[q] = INT32_MAX; }
    for (int k = 0; k < nb; ++k) {
      const int2 a = iof[static_cast<size_t>(r0) + k], bb = iob[static_cast<size_t>(r0) + k];
      if (a.x != bb.x || a.y > 0xffff || bb.y > 0xffff) runs_ok = false;
      I.tpos_f[static_cast<size_t>(r0) + k] = static_cast<uint16_t>(a.y);
      I.tpos_b[static_cast<size_t>(r0) + k] = static_cast<uint16_t>(bb.y);
      if (k == 0 || a.x != iof[static_cast<size_t>(r0) + k - 1].x + 1) {  // a new run starts at k
        if (nr > 0 && nr <= kSubMaxRuns) d.run_end[nr - 1] = k;
        if (nr < kSubMaxRuns) d.run_off[nr] = a.x - k;
        ++nr;
      }
    }
    if (nr > kSubMaxRuns) runs_ok = false;
  }
  return runs_ok;
}

// ---- row units and fuse_ok
// fused projection in the backward sweep: the first rotation row of a pose finds the others right behind it in the
// tile, and a pose of the last stage has all its rows there.  Row units of a block: {tile position, row}
bool row_units(const SubBlockOpHost &H, const std::vector<int32_t> &top_rows, const ImageLayout &L, SubImage &I) {
  const int64_t rot0 = L.rot0, rot1 = L.rot1;
  bool ok = L.grouped;  // (a shard's rows are rotations | ranges | translations in this order too: the same tests on the row index)
  std::vector<int2> &units = I.b_unit;
  for (SubDesc &d : I.desc) {
    const int32_t *rows = H.b_rows.data() + d.row_begin;
    const int nb = d.nrows;
    int64_t leaders = 0, rot_rows = 0;
    d.unit_begin = static_cast<int32_t>(units.size());
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
    d.nunits = static_cast<int32_t>(units.size()) - d.unit_begin;
    ok = ok && rot_rows == leaders * L.d;
  }
  units.push_back(make_int2(0, 0));
  if (ok) {
    std::vector<char> in_top(static_cast<size_t>(L.rows), 0);
    for (int32_t r : top_rows) in_top[r] = 1;
    for (int32_t r : top_rows)
      if (r >= rot0 && r < rot1) {
        const int64_t lead = r - (r - rot0) % L.d;
        for (int a = 0; a < L.d && ok; ++a) ok = in_top[lead + a] != 0;
      }
  }
  return ok;
}

// ---- dense-block packing
// per-row records, padded per block to a multiple of eight (empty masks) + one spare round at the end; the value arrays
// get 64 * 65 zero entries: the kernel's prefetch of the next round reads past a block's end
void pack_blocks(BlockOpHost &H, BlockImage &I) {
  std::vector<BlockLane> &bc = I.by_col, &br = I.by_row;
  I.desc.resize(H.nrows.size());
  for (size_t b = 0; b < I.desc.size(); ++b) {
    I.desc[b] = BlockDesc{H.row_begin[b], H.nrows[b], static_cast<int32_t>(bc.size()), 0, H.w_off[b], 0};
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
}

// ---- chunk rows
// long-row ordinal of every chunk of a row product; sizes of its zeroed tickets and partial sums
void chunk_rows(const RowOpHost &H, RowOpImage &I) {
  const int nlong = static_cast<int>(H.long_out.size()), nchunks = static_cast<int>(H.chunk_begin.size());
  I.live = true;
  I.chunk_row.assign(static_cast<size_t>(nchunks), 0);
  for (int r = 0; r < nlong; ++r)
    for (int32_t ch = H.long_chunk_ptr[r]; ch < H.long_chunk_ptr[r + 1]; ++ch) I.chunk_row[ch] = r;
  I.tickets = static_cast<size_t>(std::max(nlong, 1));
  I.partial = static_cast<size_t>(std::max(nchunks, 1)) * kMaxLD;
}

void sub_stage(TriPlan &plan, const ImageLayout &layout, TriImage &image, PhaseTimer &tick) {
  SubBlockOpHost &H = plan.stages[0].sub_op;
  SubImage &I = image.stages[0].sub;
  I.desc = sub_descriptors(H);
  sub_tails(H);
  image.aux_rows = H.n_aux;
  tick("  sub: descriptors");
  I.io_f = io_list(H.rows, I.desc);
  I.io_b = io_list(H.b_rows, I.desc);
  image.io_runs = run_tables(I) ? 1 : 0;
  tick("  sub: io lists, runs");
  image.fuse_ok = row_units(H, plan.top_rows, layout, I);
  if (tick.on()) std::fprintf(stderr, "  [tri plan] sweep fusion possible: %d\n", int(image.fuse_ok));
  tick("  sub: units");
}

}  // namespace

void build_tri_image(TriPlan &plan, const ImageLayout &layout, TriImage &image, PhaseTimer &tick) {
  const size_t K = plan.stages.size();
  image = TriImage();
  image.stages.resize(K);
  for (size_t k = 0; k < K; ++k) {
    TriStage &S = plan.stages[k];
    StageImage &I = image.stages[k];
    I.has_fwd_a = k > 0;
    I.has_bwd_a = k + 1 < K;
    I.dense = S.dense;
    I.is_sub = S.sub;
    if (S.sub) {
      sub_stage(plan, layout, image, tick);
      continue;
    }
    if (k == 1 && image.stages[0].is_sub) {  // the last stage of a two-stage plan: only its two explicit-inverse products
      I.aux_sum = !S.fwd_a.empty();          // (+ the sum of the aux rows as a product of its own on large plans)
      if (I.aux_sum) chunk_rows(S.fwd_a, I.fwd_a);
      chunk_rows(S.fwd_b, I.fwd_b);
      chunk_rows(S.bwd_b, I.bwd_b);
      tick("  top: chunk rows");
      continue;
    }
    if (I.has_fwd_a) chunk_rows(S.fwd_a, I.fwd_a);
    if (S.dense) {
      pack_blocks(S.blocks_op, I.blocks);
      continue;
    }
    chunk_rows(S.fwd_b, I.fwd_b);
    if (I.has_bwd_a) chunk_rows(S.bwd_a, I.bwd_a);
    chunk_rows(S.bwd_b, I.bwd_b);
  }
}

void tri_image_digest(const TriPlan &plan, const TriImage &image, uint64_t out[2]) {
  ImageDigest dig;
  std::vector<DevStage> dev;
  walk_tri_image(dig, plan, image, dev);
  out[0] = dig.h[0];
  out[1] = dig.h[1];
}

void tri_image_shape(const TriPlan &plan, const TriImage &image, int64_t out[kShapeFields]) {
  tri_plan_shape(plan, out);  // (counts arrays by their sizes: none of them has a tail)
  out[kShapeIoRuns] = image.io_runs;
  out[kShapeFuseOk] = image.fuse_ok ? 1 : 0;
}

}  // namespace cora
