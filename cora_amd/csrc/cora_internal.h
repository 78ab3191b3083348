// Internal declarations shared by the format builder (host C++), the kernels
// (HIP) and the C-ABI layer.  Not installed; the public interface is
// include/cora_hip.h.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace cora {

constexpr int kWave = 64;         // CDNA4 wavefront
constexpr int kLongRow = 96;      // translation rows longer than this -> long path
constexpr int kLongChunk = 1024;  // nnz per long-row chunk (one wavefront each)
constexpr int kSigma = 256;       // sorting window (rows) for translation slices
constexpr int kMaxLD = 24;

// Row stride (doubles) used for a k-column resident vector: the number of columns itself, whatever k (<= kMaxLD).  Odd
// strides cost 8-byte instead of 16-byte row accesses but save the padding traffic (Hvp at p = 5 measured 24.45 ->
// 23.28 us against a stride of 6); rounds 1-2 padded 13..24 columns to 16 / 20 / 24 -- the certificate block of rank
// p >= 11 has max(10, p + 2) >= 13 columns (src/CORA_problem.cpp:1062-1063) and paid up to 23 % of padding.
inline int ld_for(int k) { return k < 2 ? 2 : k; }

enum SliceType : int32_t {
  kSliceStiefel = 0,   // lane = one pose (its d rotation rows); d x 1 column blocks
  kSliceOblique = 1,   // lane = one unit-sphere row
  kSliceEuclid = 2,    // lane = one translation row, identity row order
  kSliceEuclidPerm = 3 // lane = one translation row, rows given by perm[]
};
constexpr int32_t kSliceTypeMask = 0xff;
// Flag on a pose slice: the CHAIN layout.  The lane owns its pose's d rotation rows AND the pose's translation row, the
// columns every pose of a chain has are implied by the lane (no index stored), and everything Q's symmetry gives is
// stored once:
//   fixed slots (values only, [..][lane], in this order; P = the lane's local pose, t_P its translation row):
//     s0[a], a <= d : column t_P      -- Q(rot(P)_a, t_P) for a < d,  Q(t_P, t_P) for a = d
//     s1[a], a <= d : column t_{P+1}  -- Q(rot(P)_a, t_{P+1}),        Q(t_P, t_{P+1})       (zeros without a next local pose)
//     nxt[c][a]     : column rot(P+1)_c, rows rot(P)_a               (zeros without a next local pose)
//     own[c][a]     : column rot(P)_c,   rows rot(P)_a   -- read by EPI_NONE only: the epilogues that subtract Lambda
//                     (EPI_S, EPI_HVP, EPI_HVP_K) take the block S_P = sym(own) - Lambda_P instead (HostFormat::own_sym)
//   taken from elsewhere (checked bit for bit when the format is built; a slice that fails keeps the plain layout and
//   its translation rows go to row slices):
//     Q(t_P, rot(P)_c)      = s0[c] of the same lane
//     Q(rot(P)_a, rot(P-1)_c) = nxt[a][c], Q(t_P, rot(P-1)_c) = s1[c], Q(t_P, t_{P-1}) = s1[d] of the lane BEFORE
//                             (lane 0: HostFormat::head_val, kChainHead(d) doubles per pose slice)
//   general slots (index + d values, SliceDesc::width of them): every other column of the rotation rows
//   tail (PAIRS of {index, value}, compact, sorted by lane; lane's range of pairs in tinfo = start | count << 16):
//     every other column of the translation row -- its range measurements (two entries each: the range row and the
//     landmark's translation), loop closures, a predecessor on another shard; an odd count is padded with a zero
// Value stream from SliceDesc::off: fixed (kChainFixed(d) x 64) | general (width x d x 64) | tail (T x 2);  index stream
// from SliceDesc::coff: tinfo (64) | general (width x 64) | tail (T x 2);  T = SliceDesc::type >> kSliceTailShift pairs.
constexpr int32_t kSliceChainFlag = 0x100;
// tinfo = start | count << 16 | nlocal << 24 (pairs; count, nlocal <= 127): the first nlocal pairs of a lane's tail have
// columns of the handle's own shard, the rest are rows another rank owns (partitioned handles sort them so).
// SliceDesc::nrows carries two launch-time flags above the lane count (capi.hip builds the lists of a partitioned
// handle's overlapped product with them): kSliceSkipRemoteTail -- the slice runs before the exchange has landed and
// leaves out the remote pairs of its tails; kSliceRemoteTailOnly -- the rest: out[t] += the remote pairs, nothing else.
constexpr int32_t kSliceRowsMask = 0x7f;
constexpr int32_t kSliceSkipRemoteTail = 0x100;
constexpr int32_t kSliceRemoteTailOnly = 0x200;
constexpr int kSliceTailShift = 16;
constexpr int kSliceTailMaxShift = 9;   // SliceDesc::type bits 9..15: the longest tail (in pairs) of a lane of the slice
constexpr int32_t kSliceTailMaxMask = 0x7f;
constexpr int kChainFixed(int d) { return 2 * (d + 1) + 2 * d * d; }   // doubles per lane in the fixed slots
constexpr int kChainHead(int d) { return d * d + d + 1; }              // doubles per slice in head_val
// A symmetric d x d block stored as its upper triangle: d(d+1)/2 doubles, entry (a, c) with a <= c in slot kSymSlot
// (d = 3: 00 01 02 11 12 22).  Per pose slice [slot][64], indexed by the local pose P as (P / 64, slot, P % 64).
constexpr int kSymEl(int d) { return d * (d + 1) / 2; }
constexpr int kSymSlot(int a, int c, int d) {
  return a <= c ? a * d - a * (a - 1) / 2 + c - a : c * d - c * (c - 1) / 2 + a - c;
}

// One wavefront's work, stored slot-major ([k][lane]) so that every load is a
// fully coalesced 512 B (values) / 256 B (columns).
//  - row slices (types 1-3): lane = row, slot k = one nonzero:
//        col  = scol[coff + k*64 + lane],  val = sval[off + k*64 + lane]
//  - pose slices (type 0): lane = pose, slot k = one column of the union pattern
//    of the pose's d rows, carrying d values (a d x 1 block; zero where a row
//    does not have the column):
//        col  = scol[coff + k*64 + lane],  val_a = sval[off + (k*d + a)*64 + lane]
struct SliceDesc {
  int32_t row0;    // first internal row (or offset into perm[] for kSliceEuclidPerm)
  int32_t nrows;   // active lanes
  int32_t width;   // slots per lane
  int32_t type;    // SliceType
  int64_t off;     // element offset into sval
  int32_t coff;    // element offset into scol
  int32_t aux0;    // Stiefel: first LOCAL pose index; Oblique: first LOCAL range index
};
static_assert(sizeof(SliceDesc) == 32, "SliceDesc must be 32 bytes");

// A chunk of one long row, processed by one 256-thread workgroup.
struct LongChunk {
  int32_t row;       // internal row
  int32_t k0, k1;    // nonzero range in lval / lcol
  int32_t nchunks;   // chunks of this row
  int32_t first;     // index of this row's first chunk (partials slot base)
  int32_t slot;      // long-row ordinal (ticket counter index)
  int32_t pad0, pad1;
};
static_assert(sizeof(LongChunk) == 32, "LongChunk must be 32 bytes");

// Region of the internal row order owned by this handle.
struct Layout {
  int d = 0, n = 0, r = 0, nt = 0;  // global problem dims (nt = n + l)
  int64_t N = 0;                    // n*d + r + nt
  int rank = 0, world = 1;
  int64_t shard_rows = 0;           // padded rows per rank
  int64_t rows = 0;                 // world * shard_rows
  // local (owned) counts and internal bases
  int64_t base = 0;                 // rank * shard_rows
  int nl_poses = 0, nl_ranges = 0, nl_trans = 0;
  int64_t rot_base = 0, rng_base = 0, trn_base = 0;  // internal row of first local rot/range/trans row
  int64_t local_rows = 0;
};

// (A new member of HostFormat or Layout has to enter format_digest, format_build.cpp: the digest is what pins the format.)
struct HostFormat {
  Layout L;
  std::vector<int32_t> api2int;   // N: internal row of API row
  std::vector<int32_t> int2api;   // rows: API row of internal row (-1 = padding)
  std::vector<SliceDesc> slices;
  std::vector<SliceDesc> slices_pose_first;  // same slices, pose slices first inside each eighth (small row strides)
  // [pose slice][kChainHead(d)]: what lane 0 of a chain slice takes from the pose before it --
  // [a * d + c] = Q(rot(P)_a, rot(P-1)_c), [d * d + c] = Q(t_P, rot(P-1)_c), [d * d + d] = Q(t_P, t_{P-1})
  std::vector<double> head_val;
  // [pose slice][kSymEl(d)][64]: sym(Q_PP) = (own + own^T) / 2 of every lane of a chain slice (kSymSlot order; zeros in
  // plain slices and past the slice's poses).  The handle's S array starts as a copy and k_point_finish writes
  // S_P = sym(Q_PP) - Lambda_P from it at every point (own is not bit-symmetric: the two halves differ by up to an ulp).
  std::vector<double> own_sym;
  std::vector<double> sval;
  std::vector<int32_t> scol;
  std::vector<int32_t> perm;      // internal rows for kSliceEuclidPerm slices
  std::vector<LongChunk> chunks;
  std::vector<int32_t> chunk_order;  // launch order of the chunks: by first column, so that chunks of
                                     // different long rows that read the same region of X run together
  std::vector<double> lval;
  std::vector<int32_t> lcol;
  int n_long_rows = 0;
  // partitioned handles: the long rows are DISTRIBUTED (format_build.cpp) -- the same list on every rank: internal row
  // and owner rank of long row j (LongChunk::slot = j); empty on one GPU
  std::vector<int32_t> long_rows, long_owner;
  std::vector<double> diag;       // diag(Q) for LOCAL rows, indexed by (internal row - base)
  int64_t nnz_global = 0, nnz_local = 0, padded_nnz = 0, long_nnz = 0;
  int max_width = 0;
};

// Provenance mode of build_format (build_value_map): `val` holds 1 + the CSR position of every entry, so every slot of
// the format names its source; the equalities a chain slice is checked for are recorded in `mirror` instead of tested,
// and pose slice j takes the chain layout only where chain[j] says the handle's own slice did.
struct ProvenanceBuild {
  std::vector<char> chain;
  std::vector<int32_t> mirror;
};

// Builds the partition + sliced format.  Throws std::runtime_error on invalid input.
// distribute_long_rows (world > 1 only): see HostFormat::long_rows.
void build_format(int d, int n, int r, int nt, const int32_t *rowptr,
                  const int32_t *col, const double *val, int rank, int world,
                  HostFormat &out, bool distribute_long_rows = true, ProvenanceBuild *prov = nullptr);

// Where every stored value of a HostFormat comes from in the CSR the format was built from (cora_update_values: the
// sparsity pattern of Q stays, only numbers move).  A source is a CSR position, or kNoSource for a slot that holds no
// entry (padding; a column one of a pose's rows does not have).  kSourceAdd0 marks the slots build_format fills by
// ADDING the entry to +0.0 (the rotation rows' union pattern, the diagonal): the update adds too, so that a -0.0 in the
// CSR ends as the same +0.0.  Rows with a repeated column index have no map (their slots are sums of several entries):
// build_value_map refuses them, creation keeps accepting them.
constexpr int32_t kNoSource = -1;
constexpr int32_t kSourceAdd0 = INT32_MIN;  // flag bit; position = src & INT32_MAX
struct ValueMap {
  bool built = false;
  uint64_t pattern_hash = 0;   // of (rowptr, colidx): checked on every later update
  int64_t nnz = 0;
  std::vector<int32_t> sval, lval, head_val, diag;  // one source per slot of the array of the same name
  std::vector<int32_t> own_sym;  // two sources per slot ([2 * slot], [2 * slot + 1]): the slot is half their sum
  // The equalities the chain layout relies on (format_build.cpp: trot/s0, prev/nxt, hq/s1, ht/s1[d]) as pairs of
  // sources: the values at [2 * j] and [2 * j + 1] must compare equal (kNoSource: zero) or the update is refused.
  std::vector<int32_t> mirror;
};
uint64_t pattern_hash(int64_t N, const int32_t *rowptr, const int32_t *col);
// Recomputes the format's structure from (rowptr, col), compares it with F's own (slices, columns, chunks, row maps) and
// records the sources.  Throws std::runtime_error (pattern differs, repeated column in a row, invalid CSR).
void build_value_map(const HostFormat &F, const int32_t *rowptr, const int32_t *col, bool distribute_long_rows, ValueMap &M);
// Why `val` cannot replace the values (non-finite entry, broken mirror equality), or nullptr.
const char *value_map_check_host(const ValueMap &M, const double *val);
// F's five value arrays from `val` through the map: the bits build_format would have produced.
void value_map_apply_host(const ValueMap &M, const double *val, HostFormat &F);

// Q(w) as a fixed sum of per-measurement terms (cora_assembly_build / cora_assemble_values, capi/assembly.inc).  Q is
// linear in the measurement weights: CSR entry q is the sum over t in [tptr[q], tptr[q + 1]) of tcoef[t] * w[tweight[t]],
// w = [rot of every edge | trans of every edge | range] (the layout of the residuals).  A coefficient carries the
// precision (kappa, tau, omega) the table held when the map was built; `base` keeps those 2 * n_edges + n_ranges numbers.
// ORDER of an entry's terms: ascending weight index, and for one weight index the enumeration order of the measurement
//   rotation of edge e (second rotation row >= 0):  (ra+k, ra+k) k < d;  (rb+k, rb+k) k < d;  then for a < d, c < d:
//       (ra+a, rb+c);  then for a < d, c < d: (rb+c, ra+a)                        -- kappa on the diagonals, -kappa R[a,c]
//   translation of edge e:  rows u = (ra .. ra+d-1, ta, tb), v = (-t, -1, +1): (u_i, u_j) for i, then j   -- tau (v_i v_j)
//   range m:                rows u = (q, ta, tb),            v = (r, -1, +1):  (u_i, u_j) for i, then j   -- omega (v_i v_j)
// (v_i v_j is formed first, so the coefficients of (i, j) and (j, i) have the same bits and Q(w) is bitwise symmetric.)
// SUM of an entry, on the device and in the host mirror alike, acc = fma(coef, w, acc) from +0.0:
//   at most kLongEntry terms: in map order, one accumulator;
//   more ("long" entries, listed in long_entries): 64 accumulators, number l takes terms l, l + 64, ... in order; then
//   acc[l] += acc[l + off] for l < off, off = 32, 16, 8, 4, 2, 1; the entry is acc[0].
// An entry no term reaches is +0.0.
// kLongEntry = 2 waves of terms: up to there a lane's serial loop is shorter than the launch of a wavefront per entry
// would be; beyond it (a landmark's diagonal collects a term per measurement: thousands) one lane would hold its wave up.
constexpr int kLongEntry = 2 * kWave;
struct TermMap {
  bool built = false;
  int64_t nnz = 0, n_edges = 0, n_ranges = 0, n_weights = 0, n_terms = 0, max_terms = 0;
  std::vector<int32_t> tptr;          // nnz + 1
  std::vector<int32_t> tweight;       // n_terms
  std::vector<double> tcoef;          // n_terms
  std::vector<int32_t> long_entries;  // CSR positions with more than kLongEntry terms, ascending
  std::vector<double> base;           // n_weights: kappa of every edge | tau of every edge | omega of every range
};
// The table in API rows as cora_set_measurements takes it, except edge_data / range_data, which are field-major
// ([field][measurement], the handle's copy).  Throws std::runtime_error: a row with a repeated column, a term with a
// nonzero coefficient outside the pattern (names the measurement), 2^31 terms or more.
void build_term_map(int d, int64_t N, const int32_t *rowptr, const int32_t *col, int64_t n_edges, const int32_t *edge_rows,
                    const double *edge_data, int64_t n_ranges, const int32_t *range_rows, const double *range_data,
                    TermMap &M);
// The map executed on the host in the device's order (see above): vals[nnz].
void term_map_apply_host(const TermMap &M, const double *w, double *vals);

// Every column index a slice stores (general slots and tail of a chain slice; all slots of the others); the implied
// columns of a chain slice are rows of the local shard.
void slice_columns(const HostFormat &F, const SliceDesc &sd, std::vector<int32_t> &out);

// Host execution of the FORMAT (test hook, see cora_debug_format_spmm_host).
void format_spmm_host(const HostFormat &F, const double *X_int, int ld,
                      double *out_int);

// Digests (test hooks, cora_debug_format_digest / cora_debug_value_map_digest): FNV-1a over 64-bit words, every array
// preceded by its length.  format_digest: out[0] every integer of the format (Layout, counters, row maps, slice and chunk
// descriptors, indices, work orders), out[1] the bits of every double.  value_map_digest: out[0] the sources, out[1] the
// mirror pairs.  Equal digests: the kernels see the same format.
void format_digest(const HostFormat &F, uint64_t out[2]);
void value_map_digest(const ValueMap &M, uint64_t out[2]);

}  // namespace cora
