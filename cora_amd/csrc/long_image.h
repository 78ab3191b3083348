// The DEVICE IMAGE of the long rows: what the chunk blocks of k_spmm read (chunk descriptors, launch order, values and
// columns) derived from the format on the host when a handle is created, apart from the format itself -- HostFormat, its
// digest and the value map stay as build_format leaves them.
//
// Why an image of its own.  The format keeps a long row in CSR order and cuts it every kLongChunk entries.  For a
// landmark row that is the range columns in measurement order, then the translation columns: the gathers of one chunk are
// spread over the territory of all eight L2s, while the slices that stream the same rows of X through their LDS windows
// run on XCD floor(8 x position along the chain).  The L2s of different XCDs share nothing, so nearly every line a chunk
// gathered crossed the fabric a second time.  The image sorts a row's entries by the XCD that already reads the column
// ("home") and runs every piece on that XCD.
#pragma once

#include <cstdint>
#include <vector>

#include "cora_internal.h"

namespace cora {

constexpr int kXcds = 8;  // k_spmm deals chunk and slice blocks out by blockIdx % 8
// entries per piece of a long row (one wavefront each); see profiles/long_rows_xcd.md for the sizes measured
#ifndef CORA_LONG_PIECE
#define CORA_LONG_PIECE 1024
#endif
constexpr int kLongPiece = CORA_LONG_PIECE;

struct LongImage {
  // placed: pieces sorted and dealt out per XCD (below).  false: the format's own chunks, order and arrays, perm the
  // identity -- partitioned handles, whose long rows keep the format's cut.
  bool placed = false;
  // Pieces, row by row in the format's order of rows; a row's pieces are consecutive, in ascending (home, column), and
  // carry the row's slot, `first` = the row's first piece, `nchunks` = its pieces: the last arriver adds partials
  // first .. first + nchunks - 1 in that order.  [k0, k1) index lval / lcol of the IMAGE.
  std::vector<LongChunk> chunks;
  // Launch order, 8 x cper entries: XCD x runs the pieces at [x cper, (x + 1) cper) -- those whose home is x, by first
  // column --, every list padded to the longest with -1 (the block does nothing).  Not placed: the format's chunk_order.
  std::vector<int32_t> chunk_order;
  std::vector<double> lval;
  std::vector<int32_t> lcol;
  std::vector<int32_t> perm;  // lval[i] = F.lval[perm[i]], lcol[i] = F.lcol[perm[i]]
};

// home[internal row] = the XCD whose eighth of `order` (F.slices or F.slices_pose_first; per_xcd = ceil(n_slices / 8) as
// in k_spmm) holds the slice that owns the row: the pose slice for the rotation rows of its poses and, in the chain
// layout, their translation rows; the range slice for a range row; the perm slice for a translation row no chain slice
// took.  -1: no slice owns the row (long rows, rows of other ranks, padding).
void long_row_homes(const HostFormat &F, const std::vector<SliceDesc> &order, std::vector<int8_t> &home);

// The image of F's long rows.  One GPU (world == 1): every row's entries stable-sorted by (home, column), cut at every
// change of home and into equal parts (whole wavefront rounds) of at most `piece` entries; an entry without a home goes
// with the row's lowest home (its first piece, or the parts that piece is cut into).  Partitioned handles: the format's chunks as they are.
LongImage build_long_image(const HostFormat &F, int piece = kLongPiece);

}  // namespace cora
