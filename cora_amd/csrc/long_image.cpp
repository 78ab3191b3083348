// The device image of the long rows (long_image.h): homes of the rows of X, then sort, cut and place.  Host only.
#include "long_image.h"

#include <algorithm>
#include <numeric>

namespace cora {

void long_row_homes(const HostFormat &F, const std::vector<SliceDesc> &order, std::vector<int8_t> &home) {
  const Layout &L = F.L;
  home.assign(static_cast<size_t>(L.rows), int8_t{-1});
  const size_t per_xcd = (order.size() + kXcds - 1) / kXcds;
  for (size_t s = 0; s < order.size(); ++s) {
    const SliceDesc &sd = order[s];
    const int8_t x = static_cast<int8_t>(s / per_xcd);
    const int nrows = sd.nrows & kSliceRowsMask;
    const int type = sd.type & kSliceTypeMask;
    for (int lane = 0; lane < nrows; ++lane) {
      if (type == kSliceStiefel) {
        const bool chain = (sd.type & kSliceChainFlag) != 0;
        const int64_t P = static_cast<int64_t>(sd.aux0) + lane;
        const int64_t rot = chain ? L.rot_base + P * L.d : static_cast<int64_t>(sd.row0) + static_cast<int64_t>(lane) * L.d;
        for (int a = 0; a < L.d; ++a) home[static_cast<size_t>(rot + a)] = x;
        if (chain) home[static_cast<size_t>(L.trn_base + P)] = x;
      } else if (type == kSliceEuclidPerm) {
        home[static_cast<size_t>(F.perm[static_cast<size_t>(sd.row0) + lane])] = x;
      } else {
        home[static_cast<size_t>(sd.row0) + lane] = x;
      }
    }
  }
}

LongImage build_long_image(const HostFormat &F, int piece) {
  LongImage I;
  if (F.L.world > 1 || F.chunks.empty()) {
    I.chunks = F.chunks;
    I.chunk_order = F.chunk_order;
    I.lval = F.lval;
    I.lcol = F.lcol;
    I.perm.resize(F.lval.size());
    std::iota(I.perm.begin(), I.perm.end(), 0);
    return I;
  }
  I.placed = true;
  piece = std::max(piece, kWave);
  std::vector<int8_t> home;
  long_row_homes(F, F.slices, home);
  I.perm.reserve(F.lval.size());
  std::vector<int32_t> idx;
  std::vector<int8_t> h;  // home of every entry of the row under work, by position - k_begin
  std::vector<int8_t> piece_home;
  for (size_t ci = 0; ci < F.chunks.size(); ci += static_cast<size_t>(std::max(F.chunks[ci].nchunks, 1))) {
    const LongChunk &c0 = F.chunks[ci];
    const int32_t k_begin = c0.k0, k_end = F.chunks[ci + static_cast<size_t>(std::max(c0.nchunks, 1)) - 1].k1;
    const int32_t len = k_end - k_begin;
    h.resize(static_cast<size_t>(len));
    int8_t lowest = kXcds;
    for (int32_t k = 0; k < len; ++k) {
      h[k] = home[static_cast<size_t>(F.lcol[k_begin + k])];
      if (h[k] >= 0) lowest = std::min(lowest, h[k]);
    }
    if (lowest == kXcds) lowest = 0;
    for (int32_t k = 0; k < len; ++k)
      if (h[k] < 0) h[k] = lowest;  // the row's own diagonal, landmark rows: with the row's first run, in column order
    idx.resize(static_cast<size_t>(len));
    std::iota(idx.begin(), idx.end(), k_begin);
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {
      const int8_t ha = h[a - k_begin], hb = h[b - k_begin];
      return ha != hb ? ha < hb : F.lcol[a] < F.lcol[b];
    });
    const int32_t first = static_cast<int32_t>(I.chunks.size());
    const int32_t base = static_cast<int32_t>(I.perm.size());
    for (int32_t b = 0; b < len;) {
      int32_t e = b;
      const int8_t hb = h[idx[b] - k_begin];
      while (e < len && h[idx[e] - k_begin] == hb) ++e;
      // equal parts rather than full pieces and a remainder: the longest wavefront of the run is as short as it can be
      const int32_t run = e - b, parts = (run + piece - 1) / piece;
      const int32_t part = std::min(piece, ((run + parts - 1) / parts + kWave - 1) / kWave * kWave);
      for (int32_t p = b; p < e; p += part) {
        LongChunk ch{};
        ch.row = c0.row;
        ch.k0 = base + p;
        ch.k1 = base + std::min(e, p + part);
        ch.first = first;
        ch.slot = c0.slot;
        I.chunks.push_back(ch);
        piece_home.push_back(hb);
      }
      b = e;
    }
    const int32_t n_pieces = static_cast<int32_t>(I.chunks.size()) - first;
    for (int32_t p = 0; p < n_pieces; ++p) I.chunks[static_cast<size_t>(first + p)].nchunks = n_pieces;
    I.perm.insert(I.perm.end(), idx.begin(), idx.end());
  }
  I.lval.resize(I.perm.size());
  I.lcol.resize(I.perm.size());
  for (size_t i = 0; i < I.perm.size(); ++i) {
    I.lval[i] = F.lval[static_cast<size_t>(I.perm[i])];
    I.lcol[i] = F.lcol[static_cast<size_t>(I.perm[i])];
  }
  // launch order: every XCD its own pieces, by first column (pieces of different rows that read the same rows of X run
  // together), all lists as long as the longest
  std::vector<int32_t> list[kXcds];
  for (size_t p = 0; p < I.chunks.size(); ++p) list[piece_home[p]].push_back(static_cast<int32_t>(p));
  size_t cper = 0;
  for (auto &l : list) {
    std::stable_sort(l.begin(), l.end(), [&I](int32_t a, int32_t b) { return I.lcol[I.chunks[a].k0] < I.lcol[I.chunks[b].k0]; });
    cper = std::max(cper, l.size());
  }
  I.chunk_order.assign(cper * kXcds, -1);
  for (int x = 0; x < kXcds; ++x) std::copy(list[x].begin(), list[x].end(), I.chunk_order.begin() + static_cast<std::ptrdiff_t>(x * cper));
  return I;
}

}  // namespace cora
