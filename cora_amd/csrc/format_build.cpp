// Host-side construction of the device format of the data matrix Q:
//   (1) row partition across ranks (pose-aligned, nnz-balanced),
//   (2) internal row order (rank-major; per rank: rotations | ranges | translations),
//   (3) sliced-ELL storage, one 64-row slice per wavefront, slot-major so every
//       wavefront load is coalesced, plus a separate path for the few very long
//       (landmark) rows.
// Input is the reference's `Problem::data_matrix_` (Eigen row-major CSR,
// src/CORA_problem.cpp:625-712) with the variable layout of
// include/CORA/CORA_problem.h:151-157.
//
// build_format is a list of phases over one build context (struct Build): check_input, assign_owners, number_rows,
// pose_slices (build_pose_slice per slice, on a few threads: gather_rows of the rotation rows and of the translation
// row, sort_lane, chain_identities_hold, split_tails, write_chain_slice | write_plain_slice; then place_pose_slices),
// range_slices, distributed_long_rows, translation_slices (both through append_long_row), order_chunks, order_slices.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <thread>

#include "config.h"
#include "cora_internal.h"
#include "parallel.h"

namespace cora {

namespace {

struct RowRef { int32_t api_row, int_row, len; };

// What the phases of build_format share: the inputs, and what more than one phase needs of the phases before it.
struct Build {
  const int d, n, r, nt, l;  // l = nt - n landmarks
  const int64_t dn, tb, N;   // d * n | first translation row dn + r | rows of Q
  const int32_t *const rowptr, *const col;
  const double *const val;
  const int rank, world;
  const bool dist_long;  // long rows distributed over the ranks (world > 1)
  ProvenanceBuild *const prov;
  HostFormat &F;
  std::vector<int> pose_owner, range_pose, range_lm, range_owner, lm_owner;  // assign_owners
  std::vector<double> local_range_pose;  // number_rows: local pose index each local range row hangs off (work ordering key)
  std::vector<char> trn_owned;           // pose_slices: local translation rows that a chain slice took with it
  std::vector<double> slice_key;  // position of each slice of F.slices along the pose chain (work ordering)
  int32_t rowlen(int64_t i) const { return rowptr[i + 1] - rowptr[i]; }
};

void emit_slice(const Build &B, const std::vector<RowRef> &rows, size_t begin, size_t end, int32_t type, int32_t row0,
                int32_t aux0) {
  HostFormat &F = B.F;
  SliceDesc s{};
  s.row0 = row0;
  s.nrows = static_cast<int32_t>(end - begin);
  s.type = type;
  s.aux0 = aux0;
  int width = 0;
  for (size_t i = begin; i < end; ++i) width = std::max(width, rows[i].len);
  s.width = width;
  s.off = static_cast<int64_t>(F.sval.size());
  s.coff = static_cast<int32_t>(F.scol.size());
  F.max_width = std::max(F.max_width, width);
  const size_t base = F.sval.size(), cbase = F.scol.size();
  F.sval.resize(base + static_cast<size_t>(width) * kWave, 0.0);
  F.scol.resize(cbase + static_cast<size_t>(width) * kWave, 0);
  for (int lane = 0; lane < kWave; ++lane) {
    // padding lanes replicate the last active row's columns with zero values
    const size_t src = begin + std::min<size_t>(lane, end - begin - 1);
    const RowRef &rr = rows[src];
    const bool active = lane < s.nrows;
    const int32_t p0 = B.rowptr[rr.api_row];
    int32_t fill = rr.len > 0 ? F.api2int[B.col[p0]] : rr.int_row;
    for (int k = 0; k < width; ++k) {
      const size_t dst = base + static_cast<size_t>(k) * kWave + lane;
      const size_t cdst = cbase + static_cast<size_t>(k) * kWave + lane;
      if (k < rr.len) {
        F.scol[cdst] = F.api2int[B.col[p0 + k]];
        F.sval[dst] = active ? B.val[p0 + k] : 0.0;
        fill = F.scol[cdst];
      } else {
        F.scol[cdst] = fill;  // padded slot: re-reads a row already in cache
        F.sval[dst] = 0.0;
      }
    }
  }
  F.padded_nnz += static_cast<int64_t>(width) * kWave;
  F.slices.push_back(s);
}

// A local row by its internal number; its length goes to nnz_acc (F.nnz_local, or a thread's own count that is added
// up later) and its diagonal entries to F.diag, summed in CSR order.
RowRef local_row(const Build &B, int64_t int_row, int64_t &nnz_acc) {
  const int32_t api = B.F.int2api[int_row];
  const RowRef rr{api, static_cast<int32_t>(int_row), B.rowlen(api)};
  nnz_acc += rr.len;
  for (int32_t q = B.rowptr[api]; q < B.rowptr[api + 1]; ++q)
    if (B.col[q] == api) B.F.diag[int_row - B.F.L.base] += B.val[q];
  return rr;
}

// ---- the phases of build_format, in order ----------------------------------------------------------------------------
// sizes, CSR monotone, columns in range
void check_input(const Build &B) {
  const int64_t N = B.N;
  if (B.d != 2 && B.d != 3) throw std::runtime_error("cora: dimension d must be 2 or 3");
  if (B.n < 0 || B.r < 0 || B.nt < B.n) throw std::runtime_error("cora: invalid problem sizes");
  if (B.world < 1 || B.rank < 0 || B.rank >= B.world) throw std::runtime_error("cora: invalid rank/world");
  if (N <= 0) throw std::runtime_error("cora: empty problem");
  if (N > 2000000000LL) throw std::runtime_error("cora: problem too large for int32 rows");
  if (B.rowptr[0] != 0) throw std::runtime_error("cora: rowptr[0] must be 0 (call makeCompressed())");
  Layout &L = B.F.L;
  L.d = B.d; L.n = B.n; L.r = B.r; L.nt = B.nt; L.N = N; L.rank = B.rank; L.world = B.world;
  B.F.nnz_global = B.rowptr[N];
  for (int64_t i = 0; i < N; ++i) {
    if (B.rowptr[i + 1] < B.rowptr[i]) throw std::runtime_error("cora: rowptr not monotone");
    for (int32_t q = B.rowptr[i]; q < B.rowptr[i + 1]; ++q)
      if (B.col[q] < 0 || B.col[q] >= N) throw std::runtime_error("cora: column index out of range");
  }
}

// owner of every pose / range row / landmark
void assign_owners(Build &B) {
  const int d = B.d, n = B.n, r = B.r, l = B.l, world = B.world;
  const int64_t dn = B.dn, tb = B.tb;
  const int32_t *rowptr = B.rowptr, *col = B.col;
  std::vector<int> &pose_owner = B.pose_owner, &range_pose = B.range_pose, &range_lm = B.range_lm,
                   &range_owner = B.range_owner, &lm_owner = B.lm_owner;
  pose_owner.assign(n, 0); range_pose.assign(r, -1); range_lm.assign(r, -1); range_owner.assign(r, 0); lm_owner.assign(l, 0);
  // a range row belongs with the first pose translation it touches (Q23 holds
  // its two endpoints, src/CORA_problem.cpp:660-663)
  for (int k = 0; k < r; ++k) {
    const int64_t row = dn + k;
    for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
      const int64_t c = col[q];
      if (c >= tb) {
        const int64_t t = c - tb;
        if (t < n) { if (range_pose[k] < 0) range_pose[k] = static_cast<int>(t); }
        else if (range_lm[k] < 0) range_lm[k] = static_cast<int>(t - n);
      }
    }
  }
  if (world == 1) return;
  for (int j = 0; j < l; ++j) lm_owner[j] = j % world;
  for (int k = 0; k < r; ++k)
    if (range_pose[k] < 0) range_owner[k] = range_lm[k] >= 0 ? lm_owner[range_lm[k]] : 0;
  // the nnz-balanced pose partition: w = what a pose brings with it, lw = what a rank holds whatever its poses
  std::vector<int64_t> w(n, 0), lw(world, 0);
  for (int i = 0; i < n; ++i) {
    for (int a = 0; a < d; ++a) w[i] += B.rowlen(static_cast<int64_t>(i) * d + a);
    w[i] += B.rowlen(tb + i);
  }
  for (int k = 0; k < r; ++k) {
    if (range_pose[k] >= 0) w[range_pose[k]] += B.rowlen(dn + k);
    else lw[range_owner[k]] += B.rowlen(dn + k);
  }
  for (int j = 0; j < l; ++j) {
    const int64_t len = B.rowlen(tb + n + j);
    if (len > kLongRow && B.dist_long) {  // a distributed long row (below): every rank works on the columns it owns
      for (int gg = 0; gg < world; ++gg) lw[gg] += len / world;
    } else {
      lw[lm_owner[j]] += len;
    }
  }
  const int64_t total = std::accumulate(w.begin(), w.end(), int64_t{0}) +
                        std::accumulate(lw.begin(), lw.end(), int64_t{0});
  int g = 0;
  int64_t acc = lw[0];
  const double target = static_cast<double>(total) / world;
  for (int i = 0; i < n; ++i) {
    // move on when this rank is full, keeping enough poses for the ranks left
    if (g < world - 1 && acc + w[i] / 2 > target) {
      ++g;
      acc = lw[g];
    }
    pose_owner[i] = g;
    acc += w[i];
  }
  for (int k = 0; k < r; ++k)
    if (range_pose[k] >= 0) range_owner[k] = pose_owner[range_pose[k]];
}

// internal numbering: Layout, api2int / int2api, the order of the range rows
void number_rows(Build &B) {
  const int d = B.d, n = B.n, r = B.r, l = B.l, rank = B.rank, world = B.world;
  const int64_t dn = B.dn, N = B.N;
  HostFormat &F = B.F;
  Layout &L = F.L;
  std::vector<int64_t> np(world, 0), nr(world, 0), nlm(world, 0);  // poses, range rows and landmarks of every rank
  for (int i = 0; i < n; ++i) np[B.pose_owner[i]]++;
  for (int k = 0; k < r; ++k) nr[B.range_owner[k]]++;
  for (int j = 0; j < l; ++j) nlm[B.lm_owner[j]]++;
  int64_t shard = 0;
  for (int g = 0; g < world; ++g)
    shard = std::max(shard, d * np[g] + nr[g] + np[g] + nlm[g]);
  if (world > 1) shard = (shard + 7) & ~int64_t{7};
  L.shard_rows = shard;
  L.rows = shard * world;
  if (L.rows > 2000000000LL) throw std::runtime_error("cora: too many internal rows");
  L.base = shard * rank;
  L.nl_poses = static_cast<int>(np[rank]);
  L.nl_ranges = static_cast<int>(nr[rank]);
  L.nl_trans = static_cast<int>(np[rank] + nlm[rank]);
  L.rot_base = L.base;
  L.rng_base = L.rot_base + static_cast<int64_t>(d) * L.nl_poses;
  L.trn_base = L.rng_base + L.nl_ranges;
  L.local_rows = static_cast<int64_t>(d) * L.nl_poses + L.nl_ranges + L.nl_trans;

  F.api2int.assign(N, -1);
  F.int2api.assign(L.rows, -1);
  std::vector<int64_t> cp(world, 0), cr(world, 0), ct(world, 0);
  for (int i = 0; i < n; ++i) {
    const int g = B.pose_owner[i];
    const int64_t b = shard * g;
    for (int a = 0; a < d; ++a)
      F.api2int[static_cast<int64_t>(i) * d + a] = static_cast<int32_t>(b + d * cp[g] + a);
    // pose translation
    F.api2int[dn + r + i] = static_cast<int32_t>(b + d * np[g] + nr[g] + cp[g]);
    cp[g]++;
  }
  // range rows follow the order of the pose they hang off, so that the Q23 /
  // Q32 blocks are banded in the internal order whatever the measurement order
  std::vector<int32_t> rorder(r);
  std::iota(rorder.begin(), rorder.end(), 0);
  std::stable_sort(rorder.begin(), rorder.end(), [&B, n](int32_t a, int32_t b) {
    const int pa = B.range_pose[a] < 0 ? n : B.range_pose[a], pb = B.range_pose[b] < 0 ? n : B.range_pose[b];
    return pa < pb;
  });
  for (int32_t k : rorder) {
    const int g = B.range_owner[k];
    F.api2int[dn + k] = static_cast<int32_t>(shard * g + d * np[g] + cr[g]++);
  }
  for (int j = 0; j < l; ++j) {
    const int g = B.lm_owner[j];
    F.api2int[dn + r + n + j] =
        static_cast<int32_t>(shard * g + d * np[g] + nr[g] + np[g] + ct[g]++);
  }
  for (int64_t i = 0; i < N; ++i) F.int2api[F.api2int[i]] = static_cast<int32_t>(i);

  B.local_range_pose.assign(static_cast<size_t>(std::max(L.nl_ranges, 1)), 0.0);
  for (int k = 0; k < r; ++k) {
    if (B.range_owner[k] != rank) continue;
    const int64_t li = F.api2int[dn + k] - L.rng_base;
    double key = L.nl_poses;  // ranges between landmarks go last
    if (B.range_pose[k] >= 0 && B.pose_owner[B.range_pose[k]] == rank)
      key = static_cast<double>((F.api2int[static_cast<int64_t>(B.range_pose[k]) * d] - L.rot_base) / d);
    B.local_range_pose[li] = key;
  }
}

// Pose slices: lane = pose.  The d rotation rows of a pose share (almost)
// the same column pattern -- Q11 is made of dense d x d blocks and Q13 of
// d x 1 columns (src/CORA_problem.cpp:297-377, 639-652) -- so the union
// pattern is stored once with d values per column: one 4-byte index and one
// X-row gather serve d nonzeros.
//
// Chain layout (kSliceChainFlag, cora_internal.h).  Along a pose chain every pose has the same columns -- its own
// rotation block, the next and the previous pose's, the translations t_P and t_{P+1} -- so they carry no index; Q is
// symmetric, so the previous pose's block, the rotation part of the pose's translation row (Q31 = Q13^T) and the
// sub-diagonal of Q33 are what a neighbouring slot already holds; and the lane takes the pose's translation row with
// it: what is left of that row (its range measurements) is a short compact tail.  26 values + a 4-byte tail
// descriptor per pose at d = 3 instead of 33 values + 11 indices in the pose slice and ~11 values + 11 gathered rows
// of X in a translation-row slice of its own.  Every identity the layout relies on is checked bit for bit here; a
// slice that fails one keeps the plain layout (all columns explicit) and its translation rows go to the row slices.
struct Cols { std::vector<int32_t> c; std::vector<double> v; };  // distinct columns, nv values per column: v[k * nv + a]
struct Ent { int32_t col, a, seq; double v; };  // one nonzero: internal column, row of the pose, position in the CSR
struct ChainSlots {
  double s0[4], s1[4], nxt[9], own[9], hq[3], ht, prev[9];
  double trot[3];  // Q(t_P, rot(P)_c): not stored, checked against s0
};
struct ChainLane : ChainSlots {
  int nlocal = 0;  // pairs of the tail whose columns are rows of this shard (they come first)
  std::vector<int32_t> gc, tc;
  std::vector<double> gv, tv;
};
// a thread's scratch: kept from slice to slice so that the loop allocates nothing once it is warm
struct Scratch {
  std::vector<Cols> pc, tr;  // per lane: the union pattern of the rotation rows (d values per column), the translation row
  std::vector<ChainLane> cl;
  std::vector<Ent> ent;
  std::vector<int32_t> lc, rc;
  std::vector<double> lv, rv;
};
// The slices are independent of each other: a few threads build them, each slice into buffers of its own, and
// they are put together in order afterwards (the same format whatever the thread count).
struct SliceOut {
  SliceDesc sd{};
  std::vector<double> v;
  std::vector<int32_t> c;
  std::vector<int32_t> mirror;  // provenance mode: the pairs of sources the identity checks would have compared
  int64_t padded = 0, nnz = 0;
  int maxw = 0;
};

// Sorts entries by (column, CSR position) and sums equal columns in that order: `out` gets the distinct columns with nv
// values each, entry e in value e.a.  add0: every value is a sum from +0.0 (the rotation rows' union pattern, where a
// column a row lacks is a zero; kSourceAdd0 tells the update); otherwise the first entry of a value is copied as it is.
void sum_by_column(std::vector<Ent> &ent, int nv, bool add0, Cols &out) {
  std::sort(ent.begin(), ent.end(),
            [](const Ent &x, const Ent &y) { return x.col != y.col ? x.col < y.col : x.seq < y.seq; });
  out.c.clear(); out.v.clear();
  for (const Ent &e : ent) {
    const bool first = out.c.empty() || out.c.back() != e.col;
    if (first) {
      out.c.push_back(e.col);
      out.v.resize(out.v.size() + nv, 0.0);
    }
    double &v = out.v[(out.c.size() - 1) * nv + e.a];
    v = first && !add0 ? e.v : v + e.v;
  }
}

// The nv internal rows from int_row on, by internal column: the union pattern of a pose's d rotation rows (add0), or
// its translation row (nv = 1).
void gather_rows(const Build &B, int64_t int_row, int nv, bool add0, std::vector<Ent> &ent, Cols &out) {
  ent.clear();
  for (int a = 0; a < nv; ++a) {
    const int32_t api = B.F.int2api[int_row + a];
    for (int32_t t = B.rowptr[api]; t < B.rowptr[api + 1]; ++t)
      ent.push_back({B.F.api2int[B.col[t]], a, static_cast<int32_t>(ent.size()), B.val[t]});
  }
  sum_by_column(ent, nv, add0, out);
}

// The columns of local pose P (R: its rotation rows, T: its translation row) into the chain's fixed slots, what the
// lane before holds (prev, hq, ht, trot: checked, not stored), the general slots (gc, gv) and the tail (tc, tv).
void sort_lane(const Layout &L, int d, int P, const Cols &R, const Cols &T, ChainLane &C) {
  static_cast<ChainSlots &>(C) = ChainSlots{};
  C.nlocal = 0;
  C.gc.clear(); C.gv.clear(); C.tc.clear(); C.tv.clear();
  const int64_t me = L.rot_base + static_cast<int64_t>(P) * d, tme = L.trn_base + P;
  const bool has_next = P + 1 < L.nl_poses, has_prev = P > 0;
  for (size_t k = 0; k < R.c.size(); ++k) {
    const int64_t c = R.c[k];
    const double *v = &R.v[k * d];
    if (c == tme) { for (int a = 0; a < d; ++a) C.s0[a] = v[a]; }
    else if (has_next && c == tme + 1) { for (int a = 0; a < d; ++a) C.s1[a] = v[a]; }
    else if (has_next && c >= me + d && c < me + 2 * d) { for (int a = 0; a < d; ++a) C.nxt[(c - me - d) * d + a] = v[a]; }
    else if (c >= me && c < me + d) { for (int a = 0; a < d; ++a) C.own[(c - me) * d + a] = v[a]; }
    else if (has_prev && c >= me - d && c < me) { for (int a = 0; a < d; ++a) C.prev[(c - me + d) * d + a] = v[a]; }
    else { C.gc.push_back(static_cast<int32_t>(c)); for (int a = 0; a < d; ++a) C.gv.push_back(v[a]); }
  }
  for (size_t k = 0; k < T.c.size(); ++k) {
    const int64_t c = T.c[k];
    const double v = T.v[k];
    if (c == tme) C.s0[d] = v;
    else if (has_next && c == tme + 1) C.s1[d] = v;
    else if (c >= me && c < me + d) C.trot[c - me] = v;
    else if (has_prev && c >= me - d && c < me) C.hq[c - me + d] = v;
    else if (has_prev && c == tme - 1) C.ht = v;
    else { C.tc.push_back(static_cast<int32_t>(c)); C.tv.push_back(v); }
  }
}

// The identities of the chain layout inside one slice: what a lane does not store equals, bit for bit, what the same
// lane or the lane before it stores.  Provenance mode (ProvenanceBuild, cora_internal.h): the values are 1 + their CSR
// position, a pair that differs is recorded in O.mirror (0: no entry there) and every identity counts as holding -- the
// slice follows the handle's own layout.
bool chain_identities_hold(const std::vector<ChainLane> &cl, int cnt, int d, bool prov, SliceOut &O) {
  auto differ = [prov, &O](double x, double y) {
    if (prov && x != y) O.mirror.insert(O.mirror.end(), {static_cast<int32_t>(x) - 1, static_cast<int32_t>(y) - 1});
    return !prov && x != y;
  };
  bool ok = true;
  for (int q = 0; q < cnt; ++q)
    for (int c = 0; c < d; ++c)
      if (differ(cl[q].trot[c], cl[q].s0[c])) ok = false;  // Q31 = Q13^T on the pose's own block
  for (int q = 1; q < cnt && ok; ++q) {  // what lane q takes from lane q - 1
    const ChainLane &C = cl[q], &B = cl[q - 1];
    for (int a = 0; a < d; ++a)
      for (int c = 0; c < d; ++c)
        if (differ(C.prev[c * d + a], B.nxt[a * d + c])) ok = false;  // Q(rot(P)_a, rot(P-1)_c) = Q(rot(P-1)_c, rot(P)_a)
    for (int c = 0; c < d; ++c)
      if (differ(C.hq[c], B.s1[c])) ok = false;                      // Q(t_P, rot(P-1)_c) = Q(rot(P-1)_c, t_P)
    if (differ(C.ht, B.s1[d])) ok = false;                           // Q(t_P, t_{P-1}) = Q(t_{P-1}, t_P)
  }
  return ok;
}

// Every lane's tail as PAIRS of entries (cora_internal.h), columns of this shard first, rows of other ranks after them
// (each group padded to whole pairs with a zero): a partitioned handle can run the local part before the exchange of
// the operand has landed.  False: a tail does not fit the descriptors (the slice keeps the plain layout).
bool split_tails(const Layout &L, int cnt, Scratch &W) {
  std::vector<int32_t> &lc = W.lc, &rc = W.rc;
  std::vector<double> &lv = W.lv, &rv = W.rv;
  size_t T = 0;
  for (int q = 0; q < cnt; ++q) {
    ChainLane &C = W.cl[q];
    lc.clear(); rc.clear(); lv.clear(); rv.clear();
    for (size_t k = 0; k < C.tc.size(); ++k) {
      const bool local = C.tc[k] >= L.base && C.tc[k] < L.base + L.shard_rows;
      (local ? lc : rc).push_back(C.tc[k]);
      (local ? lv : rv).push_back(C.tv[k]);
    }
    if (lc.size() & 1) { lc.push_back(lc.back()); lv.push_back(0.0); }
    if (rc.size() & 1) { rc.push_back(rc.back()); rv.push_back(0.0); }
    C.nlocal = static_cast<int>(lc.size() / 2);
    C.tc.assign(lc.begin(), lc.end()); C.tc.insert(C.tc.end(), rc.begin(), rc.end());
    C.tv.assign(lv.begin(), lv.end()); C.tv.insert(C.tv.end(), rv.begin(), rv.end());
    if (C.tc.size() / 2 > static_cast<size_t>(kSliceTailMaxMask)) return false;
    T += C.tc.size() / 2;
  }
  return T <= 0xffffu;
}

// The chain slice of local poses p0 .. p0 + cnt - 1 into O; its head values, sym(Q_PP) and trn_owned marks into the
// slice's own entries of F.head_val, F.own_sym and B.trn_owned.
void write_chain_slice(Build &B, int p0, int cnt, const std::vector<ChainLane> &cl, SliceOut &O) {
  HostFormat &F = B.F;
  const Layout &L = F.L;
  const int d = B.d, FV = kChainFixed(d), HV = kChainHead(d), SE = kSymEl(d);
  int gw = 0;
  size_t T = 0, mc = 0;
  for (int q = 0; q < cnt; ++q) {
    gw = std::max(gw, static_cast<int>(cl[q].gc.size()));
    mc = std::max(mc, cl[q].tc.size() / 2);
    T += cl[q].tc.size() / 2;
  }
  double *hv = &F.head_val[static_cast<size_t>(p0 / kWave) * HV];
  for (int a = 0; a < d; ++a)
    for (int c = 0; c < d; ++c) hv[a * d + c] = cl[0].prev[c * d + a];
  for (int c = 0; c < d; ++c) hv[d * d + c] = cl[0].hq[c];
  hv[d * d + d] = cl[0].ht;
  O.sd.width = gw;
  O.sd.type = kSliceStiefel | kSliceChainFlag | static_cast<int32_t>(mc << kSliceTailMaxShift) |
              static_cast<int32_t>(static_cast<uint32_t>(T) << kSliceTailShift);
  O.maxw = gw + 2 + 2 * d;
  O.v.assign((static_cast<size_t>(FV) + static_cast<size_t>(gw) * d) * kWave + 2 * T, 0.0);
  O.c.assign((1 + static_cast<size_t>(gw)) * kWave + 2 * T, 0);
  double *tv = O.v.data() + (static_cast<size_t>(FV) + static_cast<size_t>(gw) * d) * kWave;
  int32_t *tc = O.c.data() + (1 + static_cast<size_t>(gw)) * kWave;
  size_t te = 0;
  for (int lane = 0; lane < kWave; ++lane) {
    const bool active = lane < cnt;
    const ChainLane &C = cl[std::min(lane, cnt - 1)];
    auto put = [&](int slot, double v) { O.v[static_cast<size_t>(slot) * kWave + lane] = active ? v : 0.0; };
    for (int a = 0; a <= d; ++a) { put(a, C.s0[a]); put(d + 1 + a, C.s1[a]); }
    for (int k = 0; k < d * d; ++k) { put(2 * (d + 1) + k, C.nxt[k]); put(2 * (d + 1) + d * d + k, C.own[k]); }
    if (active) {  // sym(Q_PP) for the epilogues that fold Lambda into the own block (HostFormat::own_sym)
      double *os = &F.own_sym[static_cast<size_t>(p0 / kWave) * SE * kWave + lane];
      for (int a = 0; a < d; ++a)
        for (int c = a; c < d; ++c) os[static_cast<size_t>(kSymSlot(a, c, d)) * kWave] = 0.5 * (C.own[c * d + a] + C.own[a * d + c]);
    }
    // general slots; padded slots repeat a column of the lane (or the lane's own first row) with zero values
    int32_t fill = static_cast<int32_t>(L.rot_base + static_cast<int64_t>(std::min(p0 + lane, L.nl_poses - 1)) * d);
    for (int k = 0; k < gw; ++k) {
      const bool have = k < static_cast<int>(C.gc.size());
      if (have) fill = C.gc[k];
      O.c[(1 + static_cast<size_t>(k)) * kWave + lane] = fill;
      for (int a = 0; a < d; ++a) put(FV + k * d + a, have ? C.gv[static_cast<size_t>(k) * d + a] : 0.0);
    }
    uint32_t info = static_cast<uint32_t>(te);
    if (active) {
      info |= static_cast<uint32_t>(C.tc.size() / 2) << 16 | static_cast<uint32_t>(C.nlocal) << 24;
      for (size_t k = 0; k + 1 < C.tc.size(); k += 2) {
        tc[2 * te] = C.tc[k]; tv[2 * te] = C.tv[k];
        tc[2 * te + 1] = C.tc[k + 1]; tv[2 * te + 1] = C.tv[k + 1];
        ++te;
      }
      B.trn_owned[static_cast<size_t>(p0 + lane)] = 1;
    }
    O.c[lane] = static_cast<int32_t>(info);
  }
  O.padded += (static_cast<int64_t>(FV) + static_cast<int64_t>(gw) * d) * kWave + 2 * static_cast<int64_t>(T);
}

// the plain slice: every column of the union patterns explicit, `width` slots per lane
void write_plain_slice(int d, int cnt, const std::vector<Cols> &pc, int width, SliceOut &O) {
  O.sd.width = width;
  O.sd.type = kSliceStiefel;
  O.maxw = width;
  O.v.assign(static_cast<size_t>(width) * d * kWave, 0.0);
  O.c.assign(static_cast<size_t>(width) * kWave, 0);
  for (int lane = 0; lane < kWave; ++lane) {
    const Cols &P = pc[std::min(lane, cnt - 1)];
    const bool active = lane < cnt;
    int32_t fill = P.c.empty() ? O.sd.row0 : P.c[0];
    for (int k = 0; k < width; ++k) {
      const bool have = k < static_cast<int>(P.c.size());
      if (have) fill = P.c[k];
      O.c[static_cast<size_t>(k) * kWave + lane] = fill;
      for (int a = 0; a < d; ++a)
        O.v[(static_cast<size_t>(k) * d + a) * kWave + lane] =
            (have && active) ? P.v[static_cast<size_t>(k) * d + a] : 0.0;
    }
  }
  O.padded += static_cast<int64_t>(width) * d * kWave;
}

// The pose slice of local poses p0 .. p0 + 63.  Several threads run this, one slice each at a time.  WHAT A THREAD MAY
// WRITE: its own SliceOut and Scratch, the F.diag rows of its slice's poses (local_row), and its slice's entries of
// F.head_val, F.own_sym and B.trn_owned.  Nothing else: every other member of B and F is read only here.
void build_pose_slice(Build &B, bool chain_layout, int p0, SliceOut &O, Scratch &W) {
  const Layout &L = B.F.L;
  const int d = B.d, cnt = std::min(kWave, L.nl_poses - p0);
  int width = 0;
  for (int q = 0; q < cnt; ++q) {
    const int64_t row = L.rot_base + static_cast<int64_t>(p0 + q) * d;
    for (int a = 0; a < d; ++a) local_row(B, row + a, O.nnz);
    gather_rows(B, row, d, true, W.ent, W.pc[q]);
    width = std::max(width, static_cast<int>(W.pc[q].c.size()));
  }
  // chain layout: gather what every lane stores and check what it does not store
  bool chain = chain_layout;
  if (chain) {
    if (W.cl.size() < static_cast<size_t>(cnt)) W.cl.resize(static_cast<size_t>(cnt));
    for (int q = 0; q < cnt; ++q) {
      const int64_t trow = L.trn_base + p0 + q;
      if (B.rowlen(B.F.int2api[trow]) > kLongRow) chain = false;  // a long row stays on the chunked path
      gather_rows(B, trow, 1, false, W.ent, W.tr[q]);
      sort_lane(L, d, p0 + q, W.pc[q], W.tr[q], W.cl[q]);
    }
    if (chain) chain = chain_identities_hold(W.cl, cnt, d, B.prov != nullptr, O);
    if (chain) chain = split_tails(L, cnt, W);
    if (B.prov && !B.prov->chain[static_cast<size_t>(p0 / kWave)]) chain = false;
  }
  if (!chain) O.mirror.clear();
  O.sd = SliceDesc{};  // (off, coff: placed when the slices are put together)
  O.sd.row0 = static_cast<int32_t>(L.rot_base + static_cast<int64_t>(p0) * d);
  O.sd.nrows = cnt;
  O.sd.aux0 = p0;
  if (chain) write_chain_slice(B, p0, cnt, W.cl, O);
  else write_plain_slice(d, cnt, W.pc, width, O);
}

// the finished pose slices into F, in order (single-threaded)
void place_pose_slices(Build &B, std::vector<SliceOut> &outs) {
  HostFormat &F = B.F;
  size_t nv = F.sval.size(), nc = F.scol.size();
  for (const SliceOut &O : outs) { nv += O.v.size(); nc += O.c.size(); }
  F.sval.reserve(nv);
  F.scol.reserve(nc);
  for (SliceOut &O : outs) {
    O.sd.off = static_cast<int64_t>(F.sval.size());
    O.sd.coff = static_cast<int32_t>(F.scol.size());
    F.sval.insert(F.sval.end(), O.v.begin(), O.v.end());
    F.scol.insert(F.scol.end(), O.c.begin(), O.c.end());
    F.padded_nnz += O.padded;
    F.nnz_local += O.nnz;
    F.max_width = std::max(F.max_width, O.maxw);
    B.slice_key.push_back(O.sd.aux0);
    F.slices.push_back(O.sd);
    if (B.prov) B.prov->mirror.insert(B.prov->mirror.end(), O.mirror.begin(), O.mirror.end());
    std::vector<double>().swap(O.v);
    std::vector<int32_t>().swap(O.c);
  }
}

void pose_slices(Build &B, PhaseTimer &tick) {
  HostFormat &F = B.F;
  const Layout &L = F.L;
  F.diag.assign(static_cast<size_t>(std::max<int64_t>(L.local_rows, 1)), 0.0);
  B.trn_owned.assign(static_cast<size_t>(std::max(L.nl_trans, 1)), 0);
  const int lanes = std::min(kWave, std::max(L.nl_poses, 1));
  const int n_pose_slices = (L.nl_poses + kWave - 1) / kWave;
  std::vector<SliceOut> outs(static_cast<size_t>(n_pose_slices));
  F.head_val.assign(static_cast<size_t>(n_pose_slices) * kChainHead(B.d), 0.0);
  F.own_sym.assign(static_cast<size_t>(n_pose_slices) * kSymEl(B.d) * kWave, 0.0);
  // CORA_CHAIN_SLICES=0: the plain layout with every column explicit (measurement switch)
  const bool chain_layout = env_flag(Env::ChainSlices);
  unsigned nth = n_pose_slices < 64 ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  if (env_set(Env::FormatThreads)) nth = static_cast<unsigned>(env_int(Env::FormatThreads));
  parallel_parts(nth, [&B, &outs, chain_layout, lanes, n_pose_slices, nth](unsigned t) {
    Scratch W;
    W.pc.resize(static_cast<size_t>(lanes));
    W.tr.resize(static_cast<size_t>(lanes));
    const int s_begin = static_cast<int>(static_cast<int64_t>(n_pose_slices) * t / nth);
    const int s_end = static_cast<int>(static_cast<int64_t>(n_pose_slices) * (t + 1) / nth);
    for (int sl = s_begin; sl < s_end; ++sl) build_pose_slice(B, chain_layout, sl * kWave, outs[static_cast<size_t>(sl)], W);
  });
  tick("pose slices: built");
  place_pose_slices(B, outs);
}

// range (oblique) slices
void range_slices(Build &B) {
  HostFormat &F = B.F;
  const Layout &L = F.L;
  std::vector<RowRef> rows;
  rows.reserve(L.nl_ranges);
  for (int64_t i = 0; i < L.nl_ranges; ++i) rows.push_back(local_row(B, L.rng_base + i, F.nnz_local));
  for (int64_t k0 = 0; k0 < L.nl_ranges; k0 += kWave) {
    const int64_t cnt = std::min<int64_t>(kWave, L.nl_ranges - k0);
    emit_slice(B, rows, k0, k0 + cnt, kSliceOblique, static_cast<int32_t>(L.rng_base + k0), static_cast<int32_t>(k0));
    B.slice_key.push_back(B.local_range_pose[k0] + 0.25);
  }
}

// Long row number F.n_long_rows: the entries of API row `api` whose columns rank `keep` owns (keep < 0: all of them) go
// to lval / lcol in CSR order and are cut into chunks of kLongChunk.  Returns how many were kept (0: no chunk).
int append_long_row(const Build &B, int32_t api, int32_t int_row, int keep) {
  HostFormat &F = B.F;
  const int32_t p0 = B.rowptr[api];
  const int32_t k_begin = static_cast<int32_t>(F.lval.size());
  for (int k = 0; k < B.rowlen(api); ++k) {
    const int32_t ic = F.api2int[B.col[p0 + k]];
    if (keep >= 0 && ic / F.L.shard_rows != keep) continue;
    F.lval.push_back(B.val[p0 + k]);
    F.lcol.push_back(ic);
  }
  const int mylen = static_cast<int>(F.lval.size()) - k_begin;
  const int nch = (mylen + kLongChunk - 1) / kLongChunk;
  const int32_t first = static_cast<int32_t>(F.chunks.size());
  for (int c = 0; c < nch; ++c) {
    LongChunk ch{};
    ch.row = int_row;
    ch.k0 = k_begin + c * kLongChunk;
    ch.k1 = k_begin + std::min(mylen, (c + 1) * kLongChunk);
    ch.nchunks = nch;
    ch.first = first;
    ch.slot = F.n_long_rows;
    F.chunks.push_back(ch);
  }
  F.n_long_rows++;
  F.long_nnz += mylen;
  return mylen;
}

// Partitioned handles: DISTRIBUTED long rows.  The columns of a landmark row span every rank (the translation
// and range rows of all the poses that saw the landmark), so its owner used to ask for ~10^4 remote rows of X per
// landmark (18 % of the vector at 8 ranks on the 10^5-pose graph).  Instead every rank multiplies the part of every
// long row that falls on the columns it owns -- the same list of long rows, in API order, on every rank -- into
// slot j of a small buffer (SpmmArgs::long_out), the buffers are summed over the ranks after the product and the
// owner copies its rows out (capi.hip, finish_long_rows): the exchange shrinks to the chain halo plus the
// landmarks' own rows of X.
void distributed_long_rows(Build &B) {
  HostFormat &F = B.F;
  if (!B.dist_long) return;
  for (int64_t api = B.tb; api < B.N; ++api) {
    if (B.rowlen(api) <= kLongRow) continue;
    const int32_t int_row = F.api2int[api];
    // (a rank may hold nothing of the row: no chunk.  The owner's local_row() counts the whole row: taken back there)
    F.nnz_local += append_long_row(B, static_cast<int32_t>(api), int_row, B.rank);
    F.long_rows.push_back(int_row);
    F.long_owner.push_back(static_cast<int>(int_row / F.L.shard_rows));
  }
}

// The local translation rows no chain slice took: long rows whole on the chunked path (unless distributed above), the
// rest sorted by length inside windows of kSigma rows (keeps column locality) and sliced.
void translation_slices(Build &B) {
  HostFormat &F = B.F;
  const Layout &L = F.L;
  std::vector<RowRef> rows;
  rows.reserve(L.nl_trans);
  for (int64_t i = 0; i < L.nl_trans; ++i) {
    RowRef rr = local_row(B, L.trn_base + i, F.nnz_local);
    if (rr.len > kLongRow && B.dist_long) {  // distributed above (local_row() has taken its diagonal)
      F.nnz_local -= rr.len;
      continue;
    }
    if (i < L.nl_poses && B.trn_owned[static_cast<size_t>(i)]) continue;  // the pose's chain slice has it
    if (rr.len > kLongRow) append_long_row(B, rr.api_row, rr.int_row, -1);
    else rows.push_back(rr);
  }
  static_assert(kSigma % kWave == 0, "whole slices per sorting window");
  const size_t sigma = kSigma;
  std::vector<double> window_key;
  for (size_t w0 = 0; w0 < rows.size(); w0 += sigma) {
    const size_t w1 = std::min(rows.size(), w0 + sigma);
    window_key.push_back(static_cast<double>(rows[w0].int_row - L.trn_base));
    std::stable_sort(rows.begin() + w0, rows.begin() + w1,
                     [](const RowRef &a, const RowRef &b) { return a.len > b.len; });
  }
  for (size_t k0 = 0; k0 < rows.size(); k0 += kWave) {
    const size_t cnt = std::min<size_t>(kWave, rows.size() - k0);
    B.slice_key.push_back(window_key[k0 / sigma] + 0.5 + 1e-3 * static_cast<double>((k0 % sigma) / kWave));
    const int32_t poff = static_cast<int32_t>(F.perm.size());
    for (int lane = 0; lane < kWave; ++lane)
      F.perm.push_back(rows[k0 + std::min<size_t>(lane, cnt - 1)].int_row);
    emit_slice(B, rows, k0, k0 + cnt, kSliceEuclidPerm, poff, 0);
  }
}

// long-row chunks: launch order by the region of X they read
void order_chunks(HostFormat &F) {
  F.chunk_order.resize(F.chunks.size());
  std::iota(F.chunk_order.begin(), F.chunk_order.end(), 0);
  std::stable_sort(F.chunk_order.begin(), F.chunk_order.end(), [&F](int32_t a, int32_t b) {
    const int32_t ca = F.chunks[a].k1 > F.chunks[a].k0 ? F.lcol[F.chunks[a].k0] : 0;
    const int32_t cb = F.chunks[b].k1 > F.chunks[b].k0 ? F.lcol[F.chunks[b].k0] : 0;
    return ca < cb;
  });
}

// Slices: walk the pose chain, so that the pose / range / translation slices that gather the same rows of X run close
// together in time (and, with the kernel's per-XCD block chunking, on the same L2).
void order_slices(HostFormat &F, const std::vector<double> &slice_key) {
  std::vector<size_t> order(F.slices.size());
  std::iota(order.begin(), order.end(), size_t{0});
  std::stable_sort(order.begin(), order.end(),
                   [&slice_key](size_t a, size_t b) { return slice_key[a] < slice_key[b]; });
  std::vector<SliceDesc> sorted;
  sorted.reserve(F.slices.size());
  for (size_t i : order) sorted.push_back(F.slices[i]);
  F.slices.swap(sorted);
  // Second order of the same list for small row strides: inside each XCD's contiguous eighth (k_spmm: per_xcd =
  // ceil(n_slices / 8)) the pose slices go first -- their wavefronts live longest (X window + d x LD accumulators
  // + the Hvp epilogue), and launched last they were the tail of the kernel.  The eighth still covers the same
  // poses, so its rows of X stay in that XCD's L2.  Measured at 10^5 poses (profiles/r02_rank_sweep.md): Hvp
  // 2-4 % faster up to a row stride of 6, 3-9 % SLOWER from 10 on, hence kPoseFirstMaxLD.  CORA_SLICE_LJF=0
  // switches it off (measurement switch).
  if (!env_flag(Env::SliceLjf)) return;
  F.slices_pose_first = F.slices;
  const size_t per = (F.slices.size() + 7) / 8;
  for (size_t x = 0; x < 8; ++x) {
    const size_t b = std::min(x * per, F.slices.size()), e = std::min(b + per, F.slices.size());
    std::stable_partition(F.slices_pose_first.begin() + b, F.slices_pose_first.begin() + e,
                          [](const SliceDesc &sd) { return (sd.type & kSliceTypeMask) == kSliceStiefel; });
  }
}

}  // namespace

void build_format(int d, int n, int r, int nt, const int32_t *rowptr,
                  const int32_t *col, const double *val, int rank, int world,
                  HostFormat &F, bool distribute_long_rows, ProvenanceBuild *prov) {
  PhaseTimer tick(env_flag(Env::FormatTiming), "  [format]", 28, 4);
  F = HostFormat();  // every member is built below
  const int64_t dn = static_cast<int64_t>(d) * n;
  Build B{d, n, r, nt, nt - n, dn, dn + r, dn + r + nt, rowptr, col, val, rank, world, distribute_long_rows && world > 1, prov, F};
  check_input(B);
  tick("checks");
  assign_owners(B);
  number_rows(B);
  tick("owners + numbering");
  pose_slices(B, tick);  // (its own line "pose slices: built" when the threads are done)
  tick("pose slices");
  range_slices(B);
  tick("range slices");
  distributed_long_rows(B);
  translation_slices(B);
  tick("translation + long rows");
  order_chunks(F);
  order_slices(F, B.slice_key);
  tick("work order");
}

void slice_columns(const HostFormat &F, const SliceDesc &sd, std::vector<int32_t> &out) {
  const int32_t *cb = F.scol.data() + sd.coff;
  if (sd.type & kSliceChainFlag) {
    const size_t T = static_cast<uint32_t>(sd.type) >> kSliceTailShift;
    out.insert(out.end(), cb + kWave, cb + (1 + static_cast<size_t>(sd.width)) * kWave + 2 * T);
  } else {
    out.insert(out.end(), cb, cb + static_cast<size_t>(sd.width) * kWave);
  }
}

void format_spmm_host(const HostFormat &F, const double *X, int ld, double *out) {
  const int d = F.L.d;
  const Layout &L = F.L;
  std::vector<double> acc(static_cast<size_t>(ld) * 4);
  auto axpy = [&](double *y, double v, int64_t row) {
    const double *xr = X + static_cast<size_t>(row) * ld;
    for (int c = 0; c < ld; ++c) y[c] += v * xr[c];
  };
  for (const SliceDesc &s : F.slices) {
    for (int lane = 0; lane < s.nrows; ++lane) {
      std::fill(acc.begin(), acc.end(), 0.0);
      if ((s.type & kSliceTypeMask) == kSliceStiefel && (s.type & kSliceChainFlag)) {
        // the chain layout exactly as the kernel reads it (cora_internal.h): implied columns, the lane before, the tail
        const int FV = kChainFixed(d), HV = kChainHead(d);
        const double *vb = F.sval.data() + s.off;
        const int32_t *cb = F.scol.data() + s.coff;
        const double *tv = vb + (static_cast<size_t>(FV) + static_cast<size_t>(s.width) * d) * kWave;
        const int32_t *tc = cb + (1 + static_cast<size_t>(s.width)) * kWave;
        auto V = [&](int slot, int ln) { return vb[static_cast<size_t>(slot) * kWave + ln]; };
        const int P = s.aux0 + lane, np = L.nl_poses;
        const int64_t own_row = L.rot_base + static_cast<int64_t>(P) * d;
        const int64_t nxt_row = L.rot_base + static_cast<int64_t>(std::min(P + 1, np - 1)) * d;
        const int64_t prv_row = L.rot_base + static_cast<int64_t>(std::max(P - 1, 0)) * d;
        const int64_t t_own = L.trn_base + P, t_nxt = L.trn_base + std::min(P + 1, np - 1), t_prv = L.trn_base + std::max(P - 1, 0);
        double *acct = &acc[static_cast<size_t>(d) * ld];
        for (int a = 0; a <= d; ++a) {
          axpy(&acc[static_cast<size_t>(a) * ld], V(a, lane), t_own);
          axpy(&acc[static_cast<size_t>(a) * ld], V(d + 1 + a, lane), t_nxt);
        }
        if (P > 0) {
          const double *hv = &F.head_val[static_cast<size_t>(s.aux0 / kWave) * HV];
          axpy(acct, lane > 0 ? V(d + 1 + d, lane - 1) : hv[d * d + d], t_prv);
          for (int c = 0; c < d; ++c) {
            for (int a = 0; a < d; ++a)
              axpy(&acc[static_cast<size_t>(a) * ld], lane > 0 ? V(2 * (d + 1) + a * d + c, lane - 1) : hv[a * d + c], prv_row + c);
            axpy(acct, lane > 0 ? V(d + 1 + c, lane - 1) : hv[d * d + c], prv_row + c);
          }
        }
        for (int c = 0; c < d; ++c) {
          for (int a = 0; a < d; ++a) {
            axpy(&acc[static_cast<size_t>(a) * ld], V(2 * (d + 1) + c * d + a, lane), nxt_row + c);
            axpy(&acc[static_cast<size_t>(a) * ld], V(2 * (d + 1) + d * d + c * d + a, lane), own_row + c);
          }
          axpy(acct, V(c, lane), own_row + c);
        }
        for (int k = 0; k < s.width; ++k)
          for (int a = 0; a < d; ++a)
            axpy(&acc[static_cast<size_t>(a) * ld], V(FV + k * d + a, lane), cb[(1 + static_cast<size_t>(k)) * kWave + lane]);
        const uint32_t info = static_cast<uint32_t>(cb[lane]);
        for (uint32_t e = info & 0xffffu; e < (info & 0xffffu) + ((info >> 16) & 0x7fu); ++e) {  // pairs of entries
          axpy(acct, tv[2 * e], tc[2 * e]);
          axpy(acct, tv[2 * e + 1], tc[2 * e + 1]);
        }
        for (int a = 0; a < d; ++a)
          for (int c = 0; c < ld; ++c) out[static_cast<size_t>(own_row + a) * ld + c] = acc[a * ld + c];
        for (int c = 0; c < ld; ++c) out[static_cast<size_t>(t_own) * ld + c] = acct[c];
        continue;
      }
      if ((s.type & kSliceTypeMask) == kSliceStiefel) {
        for (int k = 0; k < s.width; ++k) {
          const double *xr = X + static_cast<size_t>(F.scol[s.coff + static_cast<size_t>(k) * kWave + lane]) * ld;
          for (int a = 0; a < d; ++a) {
            const double v = F.sval[s.off + (static_cast<size_t>(k) * d + a) * kWave + lane];
            for (int c = 0; c < ld; ++c) acc[a * ld + c] += v * xr[c];
          }
        }
        for (int a = 0; a < d; ++a)
          for (int c = 0; c < ld; ++c)
            out[(static_cast<size_t>(s.row0) + static_cast<size_t>(lane) * d + a) * ld + c] = acc[a * ld + c];
        continue;
      }
      for (int k = 0; k < s.width; ++k) {
        const double v = F.sval[s.off + static_cast<size_t>(k) * kWave + lane];
        const double *xr = X + static_cast<size_t>(F.scol[s.coff + static_cast<size_t>(k) * kWave + lane]) * ld;
        for (int c = 0; c < ld; ++c) acc[c] += v * xr[c];
      }
      const int64_t row = (s.type == kSliceEuclidPerm) ? F.perm[s.row0 + lane] : s.row0 + lane;
      for (int c = 0; c < ld; ++c) out[static_cast<size_t>(row) * ld + c] = acc[c];
    }
  }
  size_t ci = 0;
  while (ci < F.chunks.size()) {
    const LongChunk &c0 = F.chunks[ci];
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int c = 0; c < c0.nchunks; ++c) {
      const LongChunk &ch = F.chunks[ci + c];
      for (int32_t k = ch.k0; k < ch.k1; ++k) {
        const double *xr = X + static_cast<size_t>(F.lcol[k]) * ld;
        for (int j = 0; j < ld; ++j) acc[j] += F.lval[k] * xr[j];
      }
    }
    for (int j = 0; j < ld; ++j) out[static_cast<size_t>(c0.row) * ld + j] = acc[j];
    ci += c0.nchunks;
  }
}

// ---- in-place update of the values (cora_update_values): where every stored value comes from -------------------------

uint64_t pattern_hash(int64_t N, const int32_t *rowptr, const int32_t *col) {
  // FNV-1a over 64-bit words: the dimensions, the row pointers, the column indices
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
  mix(static_cast<uint64_t>(N));
  for (int64_t i = 0; i <= N; ++i) mix(static_cast<uint32_t>(rowptr[i]));
  const int64_t nnz = rowptr[N];
  for (int64_t q = 0; q < nnz; ++q) mix(static_cast<uint32_t>(col[q]));
  return h;
}

void build_value_map(const HostFormat &F, const int32_t *rowptr, const int32_t *col, bool distribute_long_rows, ValueMap &M) {
  const Layout &L = F.L;
  const int d = L.d;
  const int64_t N = L.N;
  M = ValueMap();
  if (rowptr[0] != 0) throw std::runtime_error("cora: rowptr[0] must be 0");
  for (int64_t i = 0; i < N; ++i)
    if (rowptr[i + 1] < rowptr[i]) throw std::runtime_error("cora: rowptr not monotone");
  if (rowptr[N] != F.nnz_global) throw std::runtime_error("cora: the number of nonzeros differs from the handle's matrix");
  const int64_t nnz = rowptr[N];
  {  // a slot that is the sum of several entries has no single source
    std::vector<int32_t> rc;
    for (int64_t i = 0; i < N; ++i) {
      rc.assign(col + rowptr[i], col + rowptr[i + 1]);
      std::sort(rc.begin(), rc.end());
      if (std::adjacent_find(rc.begin(), rc.end()) != rc.end())
        throw std::runtime_error("cora: a row repeats a column index: such a matrix cannot be updated in place (merge the "
                                 "duplicates, or create a new handle)");
    }
  }
  ProvenanceBuild prov;
  prov.chain.assign(static_cast<size_t>((L.nl_poses + kWave - 1) / kWave), 0);
  for (const SliceDesc &sd : F.slices)
    if ((sd.type & kSliceTypeMask) == kSliceStiefel && (sd.type & kSliceChainFlag)) prov.chain[static_cast<size_t>(sd.aux0 / kWave)] = 1;
  std::vector<double> pos(static_cast<size_t>(std::max<int64_t>(nnz, 1)));
  for (int64_t q = 0; q < nnz; ++q) pos[static_cast<size_t>(q)] = static_cast<double>(q + 1);
  HostFormat G;
  build_format(d, L.n, L.r, L.nt, rowptr, col, pos.data(), L.rank, L.world, G, distribute_long_rows, &prov);
  auto same_pod = [](const auto &a, const auto &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
  };
  if (G.L.rows != L.rows || G.L.base != L.base || G.L.local_rows != L.local_rows || !same_pod(G.api2int, F.api2int) ||
      !same_pod(G.slices, F.slices) || !same_pod(G.slices_pose_first, F.slices_pose_first) || !same_pod(G.scol, F.scol) ||
      !same_pod(G.perm, F.perm) || !same_pod(G.chunks, F.chunks) || !same_pod(G.chunk_order, F.chunk_order) ||
      !same_pod(G.lcol, F.lcol) || !same_pod(G.long_rows, F.long_rows) || G.sval.size() != F.sval.size() ||
      G.lval.size() != F.lval.size() || G.head_val.size() != F.head_val.size() || G.own_sym.size() != F.own_sym.size() ||
      G.diag.size() != F.diag.size())
    throw std::runtime_error("cora: the sparsity pattern differs from the one the handle was created with");
  auto source = [](double v) { return v == 0.0 ? kNoSource : static_cast<int32_t>(v) - 1; };
  auto add0 = [](int32_t s) { return s == kNoSource ? s : (s | kSourceAdd0); };
  M.sval.resize(G.sval.size());
  for (size_t i = 0; i < G.sval.size(); ++i) M.sval[i] = source(G.sval[i]);
  M.lval.resize(G.lval.size());
  for (size_t i = 0; i < G.lval.size(); ++i) M.lval[i] = source(G.lval[i]);
  M.diag.resize(G.diag.size());
  for (size_t i = 0; i < G.diag.size(); ++i) M.diag[i] = add0(source(G.diag[i]));
  const int HV = kChainHead(d), FV = kChainFixed(d), SE = kSymEl(d);
  M.head_val.resize(G.head_val.size());
  for (size_t i = 0; i < G.head_val.size(); ++i) {
    const int32_t s = source(G.head_val[i]);
    M.head_val[i] = static_cast<int>(i % HV) < d * d ? add0(s) : s;  // the rotation rows' entries are sums from +0.0
  }
  M.own_sym.assign(2 * G.own_sym.size(), kNoSource);
  // which slots of the pose slices hold entries of the rotation rows (added to +0.0 by build_slice); sym(Q_PP) of a
  // chain slice's lane from the sources of its own block
  for (const SliceDesc &sd : G.slices) {
    if ((sd.type & kSliceTypeMask) != kSliceStiefel) continue;
    int32_t *sv = M.sval.data() + sd.off;
    if (!(sd.type & kSliceChainFlag)) {
      for (size_t i = 0; i < static_cast<size_t>(sd.width) * d * kWave; ++i) sv[i] = add0(sv[i]);
      continue;
    }
    for (int slot = 0; slot < FV + sd.width * d; ++slot) {
      if (slot == d || slot == 2 * d + 1) continue;  // s0[d], s1[d]: entries of the translation row, copied as they are
      for (int lane = 0; lane < kWave; ++lane) sv[static_cast<size_t>(slot) * kWave + lane] = add0(sv[static_cast<size_t>(slot) * kWave + lane]);
    }
    int32_t *os = M.own_sym.data() + 2 * static_cast<size_t>(sd.aux0 / kWave) * SE * kWave;
    const int own0 = 2 * (d + 1) + d * d;
    for (int lane = 0; lane < sd.nrows; ++lane)
      for (int a = 0; a < d; ++a)
        for (int c = a; c < d; ++c) {
          const size_t o = static_cast<size_t>(kSymSlot(a, c, d)) * kWave + lane;
          os[2 * o] = sv[static_cast<size_t>(own0 + c * d + a) * kWave + lane];
          os[2 * o + 1] = sv[static_cast<size_t>(own0 + a * d + c) * kWave + lane];
        }
  }
  M.mirror.swap(prov.mirror);
  M.nnz = nnz;
  M.pattern_hash = pattern_hash(N, rowptr, col);
  M.built = true;
}

// ---- digests (test hooks): FNV-1a over 64-bit words, every array preceded by its length ------------------------------

namespace {
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void word(uint64_t v) { h = (h ^ v) * 0x100000001b3ull; }
  void num(int64_t v) { word(static_cast<uint64_t>(v)); }
  void ints(const std::vector<int32_t> &v) {
    num(static_cast<int64_t>(v.size()));
    for (int32_t x : v) num(x);
  }
  void bits(const std::vector<double> &v) {
    num(static_cast<int64_t>(v.size()));
    for (double x : v) {
      uint64_t b;
      std::memcpy(&b, &x, sizeof b);
      word(b);
    }
  }
  void slices(const std::vector<SliceDesc> &v) {
    num(static_cast<int64_t>(v.size()));
    for (const SliceDesc &s : v) num(s.row0), num(s.nrows), num(s.width), num(s.type), num(s.off), num(s.coff), num(s.aux0);
  }
};
}  // namespace

// Every member of HostFormat, in declaration order (the scalars of the struct first): out[0] the integers, out[1] the
// bits of the doubles.
void format_digest(const HostFormat &F, uint64_t out[2]) {
  Fnv I, D;
  const Layout &L = F.L;
  I.num(L.d), I.num(L.n), I.num(L.r), I.num(L.nt), I.num(L.N), I.num(L.rank), I.num(L.world), I.num(L.shard_rows);
  I.num(L.rows), I.num(L.base), I.num(L.nl_poses), I.num(L.nl_ranges), I.num(L.nl_trans), I.num(L.rot_base);
  I.num(L.rng_base), I.num(L.trn_base), I.num(L.local_rows);
  I.num(F.n_long_rows), I.num(F.nnz_global), I.num(F.nnz_local), I.num(F.padded_nnz), I.num(F.long_nnz), I.num(F.max_width);
  I.ints(F.api2int), I.ints(F.int2api), I.slices(F.slices), I.slices(F.slices_pose_first), I.ints(F.scol), I.ints(F.perm);
  I.num(static_cast<int64_t>(F.chunks.size()));
  for (const LongChunk &c : F.chunks) I.num(c.row), I.num(c.k0), I.num(c.k1), I.num(c.nchunks), I.num(c.first), I.num(c.slot);
  I.ints(F.chunk_order), I.ints(F.lcol), I.ints(F.long_rows), I.ints(F.long_owner);
  D.bits(F.sval), D.bits(F.lval), D.bits(F.head_val), D.bits(F.own_sym), D.bits(F.diag);
  out[0] = I.h;
  out[1] = D.h;
}

// out[0]: the sources of the five value arrays; out[1]: the mirror pairs (what the provenance mode of build_format
// recorded where the handle's builder compared).
void value_map_digest(const ValueMap &M, uint64_t out[2]) {
  Fnv S, P;
  S.num(M.nnz), S.word(M.pattern_hash);
  S.ints(M.sval), S.ints(M.lval), S.ints(M.head_val), S.ints(M.diag), S.ints(M.own_sym);
  P.ints(M.mirror);
  out[0] = S.h;
  out[1] = P.h;
}

namespace {
inline double mapped(const double *val, int32_t s) {
  if (s == kNoSource) return 0.0;
  const double v = val[s & INT32_MAX];
  return s < 0 ? 0.0 + v : v;
}
}  // namespace

const char *value_map_check_host(const ValueMap &M, const double *val) {
  for (int64_t q = 0; q < M.nnz; ++q)
    if (!std::isfinite(val[q])) return "a value is not finite";
  for (size_t j = 0; j + 1 < M.mirror.size(); j += 2) {
    const double a = M.mirror[j] == kNoSource ? 0.0 : val[M.mirror[j]];
    const double b = M.mirror[j + 1] == kNoSource ? 0.0 : val[M.mirror[j + 1]];
    if (a != b)
      return "the values break the symmetry the chain layout of the handle relies on (Q(i, j) and Q(j, i) of a pose's "
             "couplings to itself and to its neighbour must be equal)";
  }
  return nullptr;
}

void value_map_apply_host(const ValueMap &M, const double *val, HostFormat &F) {
  for (size_t i = 0; i < M.sval.size(); ++i) F.sval[i] = mapped(val, M.sval[i]);
  for (size_t i = 0; i < M.lval.size(); ++i) F.lval[i] = mapped(val, M.lval[i]);
  for (size_t i = 0; i < M.head_val.size(); ++i) F.head_val[i] = mapped(val, M.head_val[i]);
  for (size_t i = 0; i < M.diag.size(); ++i) F.diag[i] = mapped(val, M.diag[i]);
  for (size_t i = 0; i < F.own_sym.size(); ++i) F.own_sym[i] = 0.5 * (mapped(val, M.own_sym[2 * i]) + mapped(val, M.own_sym[2 * i + 1]));
}

}  // namespace cora
