// Part of kernels.hip (included there, in this order, inside namespace cora).  the sliced SpMM with fused epilogues (k_spmm: chain slices, row slices, long-row chunks) -- CORA_TU & 1.
// ---------------------------------------------------------------------------
// Sliced SpMM with fused epilogues.
//   EPI_NONE : out = Q X                       (Problem::dataMatrixProduct, :742-746)
//   EPI_S    : out = Q X - Lambda X            (certificate operator, :1162-1166)
//   EPI_HVP  : out = Proj_Y(Q X - Lambda X)    (Riemannian Hvp, :822-867)
// A chain slice's epilogues take the pose's own block and Lambda_P as ONE symmetric block, S_P = sym(Q_PP) - Lambda_P
// (SpmmArgs::S, written by k_point_finish): 6 doubles per pose at d = 3 instead of 9 own slots + 9 of Lambda, and no
// Lambda term after the slots.  EPI_NONE reads the own slots, so Q X keeps its bits.
// One wavefront per slice, lane = row, LD accumulators per lane in registers.
// Blocks [0, n_chunks) handle chunks of the long (landmark) rows instead.
// ---------------------------------------------------------------------------
// One wavefront per chunk of a long (landmark) row.
// EPI_HVP_K: the wavefront that finishes the row leaves <X[row], out[row]> in the ROW's own slot of kappa_partial
// (behind the per-block slots).  Which chunk arrives last differs from launch to launch: a term that travelled with the
// finishing block's partial would move between slots and change the rounding of their fixed-order sum -- the one source
// of run-to-run differences the solver had (tools/determinism_probe.py: 10^5 poses, where a landmark row has 40 chunks).
template <int LD, bool KAPPA>
__device__ __forceinline__ void long_chunk_wave(const SpmmArgs &A, int ci) {
  const LongChunk ch = A.chunks[ci];
  const int lane = threadIdx.x;
  double acc[LD];
#pragma unroll
  for (int j = 0; j < LD; ++j) acc[j] = 0.0;
#pragma unroll 4
  for (int k = ch.k0 + lane; k < ch.k1; k += kWave) {
    const double v = stream_load(A.lval + k);
    double x[LD];
    load_row<LD>(A.X + static_cast<size_t>(stream_load(A.lcol + k)) * LD, x);
#pragma unroll
    for (int j = 0; j < LD; ++j) acc[j] = fma(v, x[j], acc[j]);
  }
  double tot = 0.0;  // lane j < LD ends up with column j
#pragma unroll
  for (int j = 0; j < LD; ++j) {
    const double v = wave_sum(acc[j]);
    const double v0 = __shfl(v, 0, 64);
    if (lane == j) tot = v0;
  }
  // partitioned handles: the row is distributed -- this rank's part of it goes to slot ch.slot of long_out, to be summed
  // over the ranks (the row's share of kappa follows the sum: k_long_finish)
  double *orow = A.long_out ? A.long_out + static_cast<size_t>(ch.slot) * LD : A.out + static_cast<size_t>(ch.row) * LD;
  auto publish_kappa = [&](double row_j) {  // row_j: out[row][lane] in the lanes below LD
    if constexpr (KAPPA) {
      if (A.long_out) return;  // wave-uniform
      const double t = wave_sum(lane < LD ? row_j * A.X[static_cast<size_t>(ch.row) * LD + lane] : 0.0);
      if (lane == 0) A.kappa_partial[A.kappa_long_base + ch.slot] = t;
    }
  };
  if (ch.nchunks == 1) {
    if (lane < LD) orow[lane] = tot;
    publish_kappa(tot);
    return;
  }
  // several chunks: publish the partial WRITE-THROUGH (sc1 stores, so no L2
  // release fence is needed), drain, take a ticket; the last arriver re-reads
  // all partials with sc1 loads (which bypass its L1) and sums them in chunk
  // order (compensated, below), so the result is deterministic.  gfx950 inter-workgroup hand-off
  // recipe R1 (cdna_hip_programming.md, Guideline 16).
  if (lane < LD)
    __hip_atomic_store(A.partials + static_cast<size_t>(ci) * kMaxLD + lane, tot, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int last = 0;
  if (lane == 0) {
    const unsigned old = __hip_atomic_fetch_add(A.tickets + ch.slot, 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
    last = (old == static_cast<unsigned>(ch.nchunks - 1));
    if (last) __hip_atomic_store(A.tickets + ch.slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  last = __shfl(last, 0, 64);
  if (!last) return;  // wave-uniform
  double s = 0.0;
  if (lane < LD) {
    const double *P = A.partials + static_cast<size_t>(ch.first) * kMaxLD + lane;
    // The image cuts a row into more pieces than the format has chunks (a short row: one chunk, up to eight pieces), and
    // every partial added plainly is one more rounding of the row's sum.  So the partials are added with compensation
    // (Neumaier, in a fixed order): the row is the exact sum of its partials rounded once, to second order in the unit
    // roundoff, however many there are.
    // Eight loads in flight at a time; a batch the row does not fill takes +0.0 for what is missing.
    double comp = 0.0;
    for (int c = 0; c < ch.nchunks; c += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        t[u] = c + u < ch.nchunks ? __hip_atomic_load(P + static_cast<size_t>(c + u) * kMaxLD, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT)
                                  : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double n = s + t[u];
        comp += fabs(s) >= fabs(t[u]) ? (s - n) + t[u] : (t[u] - n) + s;
        s = n;
      }
    }
    s += comp;
    orow[lane] = s;
  }
  publish_kappa(s);
}

// V_i - sym(Y_i V_i^T) Y_i for one pose held entirely by this thread
// (StiefelProduct::projectToTangentSpace, include/CORA/StiefelProduct.h:79-81).
template <int LD, int D>
__device__ __forceinline__ void stiefel_project_thread(const double (&y)[D][LD],
                                                       double (&v)[D][LD]) {
  double m[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) m[a][b] = dot_row<LD>(y[a], v[b]);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const double s = 0.5 * (m[a][b] + m[b][a]);
#pragma unroll
      for (int c = 0; c < LD; ++c) v[a][c] = fma(-s, y[b][c], v[a][c]);
    }
}

// Pose slice: lane = pose, d x LD accumulators, one X-row read per d nonzeros.
//
// X window (row strides up to kWinMaxLD): along the pose chain the columns of a pose slice are the rotation rows of
// its own poses and their chain neighbours and the translation rows of the same poses -- two CONTIGUOUS pieces of X
// ((64 + 2) d and 64 + 2 rows).  The wavefront copies them to LDS with coalesced loads (4 cache lines per instruction)
// and the lanes read their rows from there; a per-lane gather of a 40-byte row costs one L1 tag look-up per lane and
// instruction (3 x 64 per slot), and the L1's look-up rate -- not bytes -- was what bounded the kernel (PMC:
// TCP_TOTAL_CACHE_ACCESSES 10.8 M per product at 10^5 poses, the L1s busy for the whole kernel).  Columns outside
// the windows (loop closures, rows of another shard) take the global gather as before; results are bit-identical.
#ifndef CORA_SPMM_WINDOW
#define CORA_SPMM_WINDOW 1
#endif
#ifndef CORA_WIN_MAX_LD
#define CORA_WIN_MAX_LD 24
#endif
// rotation window at every row stride: 198 x LD doubles (19 KB at 12, 25 KB at 16, 38 KB at 24: four to six wavefronts per
// CU still keep their loads in flight).  Round 2 stopped at 12 and the strides above fell off a cliff: (Q - Lambda) X
// with 16 columns 68.5 -> 51.6 us, 20 columns 70.5 -> 55.0 us, Hvp at p = 16 76.9 -> 60.6 us (profiles/r03_rank_sweep.md).
// (Measured and not kept: an odd LDS row stride against bank conflicts at even strides -- the index arithmetic cost more
// than the conflicts: Hvp at p = 10 32.8 -> 38.3 us, p = 16 unchanged.)
constexpr int kWinMaxLD = CORA_SPMM_WINDOW ? CORA_WIN_MAX_LD : 0;
#ifndef CORA_WIN_TRN_MAX_LD
#define CORA_WIN_TRN_MAX_LD 8
#endif
constexpr int kWinTrnMaxLD = CORA_WIN_TRN_MAX_LD;      // + the translation window while 8 wavefronts per CU fit the LDS
#ifndef CORA_POSE_COOP_EPI
#define CORA_POSE_COOP_EPI 1
#endif
#ifndef CORA_ROW_UNROLL
#define CORA_ROW_UNROLL 4  // gathers in flight per lane of a row slice (translation / range rows)
#endif
#ifndef CORA_COOP_PREFETCH_LATE
#define CORA_COOP_PREFETCH_LATE 1
#endif
#ifndef CORA_POSE_FUSE_T_MAX
#define CORA_POSE_FUSE_T_MAX 20  // (d + 1) x row stride up to which the translation row is accumulated with the rotation rows
#endif
#ifndef CORA_POSE_EARLY_MAX
#define CORA_POSE_EARLY_MAX 20  // (d + 1) x row stride up to which a chain slice requests all its fixed slots up front
#endif
#ifndef CORA_POSE_COOP_MAX_LD
// cooperative Hvp epilogue up to this row stride: above it the prefetched Y rows and Lambda blocks (d LD + d d doubles per
// lane) push the kernel into AGPR spills at one wave per SIMD -- without them p = 11 / 12 / 16 / 24: 39.6 / 40.6 / 60.1 /
// 98.7 -> 38.7 / 38.9 / 57.0 / 89.9 us (two waves per SIMD), while p = 10 lost in round 3 (32.5 -> 33.7).  Round 6: with the
// cooperative form k_spmm<10, 3, *> spilled (92-116 B of scratch per lane at two waves per SIMD: the round-5 review's
// "config 5's kernel spills"); without it 242-248 registers, no scratch, and faster on today's kernel -- certificate operator
// at 10 columns 26.25 -> 25.73 us, PMC traffic 1.36x -> 1.19x the format's compulsory bytes (writes 1.25x -> 1.00x), Hvp at
// p = 10 29.4 -> 28.75 us (profiles/r06_kernel_evolution.md): the limit is 9.
#define CORA_POSE_COOP_MAX_LD 9
#endif
#ifndef CORA_POSE_COOP_MAX_DLD
#define CORA_POSE_COOP_MAX_DLD 18  // d x row stride up to which the Hvp epilogue's operands travel through LDS (above: per lane)
#endif
#ifndef CORA_POSE_UNROLL_WIN
#define CORA_POSE_UNROLL_WIN 2  // slots per trip of the window loop (round 3, with 3 waves per SIMD: 1 / 2 / 3 / 6 / 11 slots
#endif                          // -> Hvp 21.4 / 21.5 / 21.8 / 23.0 / 30.0 us, rotated 29.2 / 29.2 / 29.3 / 32.0 / 41.0 us)
#ifdef CORA_SPMM_TIMES
// measurement build: wall-clock stamps of a pose slice's phases (tools/spmm_timeline.py)
constexpr unsigned kSpmmTimesMax = 65536;
constexpr int kSpmmPhases = 6;
__device__ unsigned long long g_spmm_phase[kSpmmPhases * kSpmmTimesMax];
#define CORA_PHASE(i) do { if (threadIdx.x == 0 && blockIdx.x < kSpmmTimesMax) g_spmm_phase[kSpmmPhases * blockIdx.x + (i)] = wall_clock64(); } while (0)
#else
#define CORA_PHASE(i) do { } while (0)
#endif
// A chain slice's second launch on a partitioned handle (kSliceRemoteTailOnly): the pairs of its tails that read rows of
// other ranks, added to the translation rows the first launch -- ahead of the exchange -- has written.
template <int LD, int D, int EPI>
__device__ __forceinline__ double remote_tail_only(const SpmmArgs &A, const SliceDesc &sd, int lane) {
  const int T = static_cast<int>(static_cast<unsigned>(sd.type) >> kSliceTailShift);
  const int mc = (sd.type >> kSliceTailMaxShift) & kSliceTailMaxMask;
  const double *__restrict__ tail_v = A.sval + sd.off + (static_cast<size_t>(kChainFixed(D)) + static_cast<size_t>(sd.width) * D) * kWave;
  const int32_t *__restrict__ tail_c = A.scol + sd.coff + (1 + static_cast<size_t>(sd.width)) * kWave;
  const int32_t tinfo = A.scol[sd.coff + lane];
  const int tstart = tinfo & 0xffff, tnloc = (tinfo >> 24) & 0x7f, tcnt = (tinfo >> 16) & 0x7f;
  double acct[LD];
#pragma unroll
  for (int j = 0; j < LD; ++j) acct[j] = 0.0;
  for (int r0 = 0; r0 < T; r0 += kWave) {
    const int e = r0 + lane;
    int2 c2 = make_int2(sd.row0, sd.row0);
    double2 v2 = make_double2(0.0, 0.0);
    if (e < T) {
      c2 = *reinterpret_cast<const int2 *>(tail_c + 2 * e);
      v2 = *reinterpret_cast<const double2 *>(tail_v + 2 * e);
    }
    double x[LD], x1[LD], pr[LD];
    load_row<LD>(A.X + static_cast<size_t>(c2.x) * LD, x);
    load_row<LD>(A.X + static_cast<size_t>(c2.y) * LD, x1);
#pragma unroll
    for (int j = 0; j < LD; ++j) pr[j] = fma(v2.x, x[j], v2.y * x1[j]);
    for (int i = 0; i < mc; ++i) {  // wave-uniform
      const int e2 = tstart + i - r0;
      const bool mine = i >= tnloc && i < tcnt && e2 >= 0 && e2 < kWave;
#pragma unroll
      for (int j = 0; j < LD; ++j) {
        const double t = __shfl(pr[j], e2 & (kWave - 1), kWave);
        acct[j] += mine ? t : 0.0;
      }
    }
  }
  const int nrows = sd.nrows & kSliceRowsMask;
  if (lane >= nrows || tcnt == tnloc) return 0.0;
  double *o = A.out + static_cast<size_t>(A.win_trn_lo + sd.aux0 + lane) * LD;
  double cur[LD];
  load_row<LD>(o, cur);
#pragma unroll
  for (int j = 0; j < LD; ++j) cur[j] += acct[j];
  store_row<LD>(o, cur);
  if (EPI == EPI_HVP_K) {  // <X, out> is linear in out: this launch's share is <X[t], what it added>
    double x[LD];
    load_row<LD>(A.X + static_cast<size_t>(A.win_trn_lo + sd.aux0 + lane) * LD, x);
    return dot_row<LD>(x, acct);
  }
  return 0.0;
}

template <int LD, int D, int EPI, bool WIN>
__device__ __forceinline__ double pose_slice(const SpmmArgs &A, const SliceDesc &sd_in, int lane) {
  const int sflags = sd_in.nrows & ~kSliceRowsMask;  // launch-time flags of a partitioned handle's overlapped product
  SliceDesc sd = sd_in;
  sd.nrows &= kSliceRowsMask;
  const double *__restrict__ vp = A.sval + sd.off + lane;
  const int32_t *__restrict__ cp = A.scol + sd.coff + lane;
  const double *__restrict__ X = A.X;
  constexpr bool kWinLD = LD <= kWinMaxLD;
  // launch-time switch (SpmmArgs::win_on, launch_spmm): below kWinMinSlices wavefronts every wavefront is resident at
  // once and its chain of dependent latencies sets the time -- the window copy and the LDS hand-overs of the
  // cooperative epilogue are extra stages there (10^4 poses: Hvp 5.9 -> 7.1 us with them)
  // (WIN is a template parameter, the two forms are separate code: behind a run-time test every row of X was "LDS read
  // or gather", the consumers sank below the last of them and twelve rows stayed live at once)
  constexpr bool kWin = kWinLD && WIN;
  constexpr int kRotRows = (kWave + 2) * D, kTrnRows = LD <= kWinTrnMaxLD ? kWave + 2 : 0;
  // cooperative Hvp epilogue (CORA_POSE_COOP_EPI): the slice's rows of Y and its rows of the result are contiguous too --
  // requested with coalesced loads BEFORE the slot loop, handed to the lanes through the window's LDS after it, and the
  // result rows leave through LDS as 512-byte runs instead of 16-byte pieces of 64 lines
  constexpr bool kCoopT = kWinLD && CORA_POSE_COOP_EPI && EPI >= EPI_HVP && D * LD <= CORA_POSE_COOP_MAX_DLD;
  constexpr bool kCoop = kCoopT && WIN;
  constexpr int kYEl = kWave * D * LD;
  constexpr int kWinEl = (kRotRows + kTrnRows) * LD;
  // (the cooperative epilogue hands Y rows in, result rows + the slice's translation rows out)
  constexpr int kCoopEl = kYEl + kWave * LD;
  // staged stores (window form, row strides up to CORA_POSE_COOP_MAX_LD, every epilogue): result rows + translation rows
  constexpr bool kStaged = kWin && LD <= CORA_POSE_COOP_MAX_LD;
  constexpr int kStagedEl = kStaged ? kYEl + kWave * LD : 0;
  constexpr int kNeedEl = (kCoopT && kCoopEl > kStagedEl) ? kCoopEl : kStagedEl;
  constexpr int kSmemEl = !kWinLD ? 1 : (kNeedEl > kWinEl ? kNeedEl : kWinEl);
  __shared__ __attribute__((aligned(16))) double win[kSmemEl];
  constexpr int kYIt = (D * LD + 1) / 2;  // (pairs of doubles per lane and access)
  double ystage[kCoopT ? 2 * kYIt : 1];
  // Chain layout (kSliceChainFlag, cora_internal.h): the lane owns the pose's translation row as well, the chain's columns
  // are implied, and what Q's symmetry gives comes from the lane before (lane 0: the slice's head block).
  const bool chain = (sd.type & kSliceChainFlag) != 0;  // wave-uniform
  // narrow rows: the values a lane hands to the lane after it stay in registers and move with a lane shift; wide rows
  // (registers are what they are short of) re-read the previous lane's values from the stream the wavefront has just
  // loaded (L1 / L2 hits)
  constexpr bool kNxtRegs = LD <= 5 || (LD <= 8 && EPI < 2);
  constexpr int kFV = kChainFixed(D);
  // the epilogues that subtract Lambda read S_P (SpmmArgs::S) for the own block: the own slots -- the last d x d fixed
  // slots, whole 512-byte lines of the stream -- are not read at all
  constexpr bool kFold = EPI != EPI_NONE;
  constexpr int kFVRead = kFold ? 2 * (D + 1) + D * D : kFV;
  constexpr int kSE = kSymEl(D);
  // Everything that does not depend on the windows is requested HERE, ahead of the windows' own loads: all wavefronts of
  // a launch are resident at once, so a launch lasts as long as a wavefront's chain of dependent memory latencies -- the
  // fixed slots' values, the tail's first 64 entries and (below) the epilogue's operands arrive with the window rows.
  const int tailT = chain ? static_cast<int>(static_cast<unsigned>(sd.type) >> kSliceTailShift) : 0;  // wave-uniform
  const double *__restrict__ tail_v = A.sval + sd.off + (static_cast<size_t>(kFV) + static_cast<size_t>(sd.width) * D) * kWave;  // [pair][2]
  const int32_t *__restrict__ tail_c = A.scol + sd.coff + (1 + static_cast<size_t>(sd.width)) * kWave;
  // the lane's range of the tail (pairs): start | count << 16; pair `lane` of the tail: two columns, two values
  int32_t tinfo = 0, tc0 = sd.row0, tc1 = sd.row0;
  double tv0 = 0.0, tv1 = 0.0;
  // (kEarly: narrow rows only -- from d + 1 accumulator rows of 7 doubles on the values and the tail's rows would not
  // fit the 256 registers of two wavefronts per SIMD beside the accumulators; wide rows load every group of fixed
  // slots where it is used and gather the tail's rows in the tail)
  constexpr bool kEarly = (D + 1) * LD <= CORA_POSE_EARLY_MAX;
  // kFuseT: the translation row accumulates beside the rotation rows (one read of every row of X for d + 1 rows of Q).
  // Wide rows cannot hold d + 1 accumulator rows: there the translation row goes first, on its own -- its slots' values,
  // nine rows of X from the windows, the tail -- and is stored before the rotation rows start.
  constexpr bool kFuseT = (D + 1) * LD <= CORA_POSE_FUSE_T_MAX;
  double fx[kEarly ? kFVRead : 1], sx[kEarly && kFold ? kSE : 1];
  auto fixed = [&](int i) { if constexpr (kEarly) return fx[i]; else return stream_load(vp + static_cast<size_t>(i) * kWave); };
  // entry k of S_P (chain slices start at a multiple of 64 poses; the address is formed where it is used)
  auto s_load = [&](int k) { return stream_load(A.S + static_cast<size_t>(sd.aux0) * kSE + static_cast<size_t>(k) * kWave + lane); };
  auto sym = [&](int k) { if constexpr (kEarly && kFold) return sx[k]; else return s_load(k); };
  double headv = 0.0;  // lane h < kChainHead(D): entry h of the slice's head block
  if (chain) {
    if (lane < kChainHead(D)) headv = A.head_val[static_cast<size_t>(sd.aux0 / kWave) * kChainHead(D) + lane];
    tinfo = stream_load(cp);
    if (lane < tailT) {
      const int2 c2 = *reinterpret_cast<const int2 *>(tail_c + 2 * lane);
      const double2 v2 = *reinterpret_cast<const double2 *>(tail_v + 2 * lane);
      tc0 = c2.x; tc1 = c2.y;
      tv0 = v2.x; tv1 = v2.y;
    }
    if constexpr (kEarly) {
#pragma unroll
      for (int i = 0; i < kFVRead; ++i) fx[i] = stream_load(vp + static_cast<size_t>(i) * kWave);
      if constexpr (kFold) {
#pragma unroll
        for (int k = 0; k < kSE; ++k) sx[k] = s_load(k);
      }
    }
  }
  // the cooperative epilogue's operand: the slice's rows of Y, requested with coalesced loads -- plain slices with the
  // window's rows; chain slices right AFTER the windows have landed: bytes needed last travel while the fixed slots and
  // the tail are computed instead of holding up their operands
  // (all wavefronts of a launch start together and share the memory system: what is requested first lands first)
  auto coop_prefetch = [&] {
    if constexpr (kCoopT) {
      const double *__restrict__ Yp = A.Y + static_cast<size_t>(sd.row0) * LD;
#pragma unroll
      // ONE predicate per access (an odd count reads one double past the slice's rows: Y has the range rows behind
      // its rotation rows).  The two-way form -- a pair, else a single
      // double into the same registers -- made the compiler wait for EVERY outstanding load before each pair (a
      // write-after-write hazard on the staging registers): thirteen loads, one after the other.
      for (int i = 0; i < kYIt; ++i) {
        const int e = 2 * (i * kWave + lane), n = sd.nrows * D * LD;
        Pair8 v{0.0, 0.0};
        if (e < n) v = *reinterpret_cast<const Pair8 *>(Yp + e);
        ystage[2 * i] = v.x;
        ystage[2 * i + 1] = v.y;
      }
    }
  };
  if (kCoop && !(chain && CORA_COOP_PREFETCH_LATE)) coop_prefetch();
  int w0 = 0, nrot = 0, t0 = 0, ntr = 0;
  if constexpr (kWinLD) if (kWin) {
    w0 = max(sd.row0 - D, A.win_rot_lo);
    nrot = max(min(sd.row0 + (kWave + 1) * D, A.win_rot_hi) - w0, 0);
    t0 = max(A.win_trn_lo + sd.aux0 - 1, A.win_trn_lo);
    ntr = kTrnRows ? max(min(A.win_trn_lo + sd.aux0 + kWave + 1, A.win_trn_hi) - t0, 0) : 0;
    const double *__restrict__ srot = X + static_cast<size_t>(w0) * LD;
    const double *__restrict__ strn = X + static_cast<size_t>(t0) * LD;
    // LDS-DMA (global_load_lds_dwordx4): 16 bytes per lane straight into the window -- wave-uniform LDS base + lane x 16,
    // per-lane source address --, no staging registers (44 at a row stride of 5: what kept the Hvp from holding its
    // other operands in flight) and no LDS-store pass.  Lanes past the end of the window's rows are masked off: LDS
    // there keeps whatever it held, and nothing reads it (chain columns are clamped to local rows, the general slots
    // test the window's range, lanes past the slice's poses are never stored).  An odd element count leaves one double
    // to an ordinary load.  __syncthreads() below carries the vmcnt(0).
    {
      typedef __attribute__((address_space(1))) const void *gptr_t;
      typedef __attribute__((address_space(3))) void *lptr_t;
      constexpr int kRotEl = kRotRows * LD, kTrnEl = kTrnRows * LD;
      constexpr int kRotIt = (kRotEl + 2 * kWave - 1) / (2 * kWave), kTrnIt = (kTrnEl + 2 * kWave - 1) / (2 * kWave);
      const int nre = nrot * LD, nte = ntr * LD;
#pragma unroll
      for (int i = 0; i < kRotIt; ++i) {
        const int e = 2 * (i * kWave + lane);
        if (e + 1 < nre)
          __builtin_amdgcn_global_load_lds((gptr_t)(srot + e), (lptr_t)(win + 2 * i * kWave), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < kTrnIt; ++i) {
        const int e = 2 * (i * kWave + lane);
        if (e + 1 < nte)
          __builtin_amdgcn_global_load_lds((gptr_t)(strn + e), (lptr_t)(win + kRotEl + 2 * i * kWave), 16, 0, 0);
      }
      if ((nre & 1) && lane == 0) win[nre - 1] = srot[nre - 1];
      if ((nte & 1) && lane == 1) win[kRotEl + nte - 1] = strn[nte - 1];
    }
    __syncthreads();
  }
  CORA_PHASE(0);  // the windows (and everything requested with them) have landed
#ifdef CORA_SPMM_TIMES
  if (threadIdx.x == 0 && blockIdx.x < kSpmmTimesMax)  // where the wavefront runs: HW_ID (reg 4) | XCC_ID (reg 20) << 32
    g_spmm_phase[kSpmmPhases * blockIdx.x + 5] = static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((31 << 11) | 4)) |
                                                 (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((31 << 11) | 20)) << 32);
#endif
  // the tail's first round: pair `lane` gathers its two rows of X now (the indices have arrived with the window's rows;
  // lanes past the tail read a valid row and multiply it by zero)
  double tg[kEarly ? LD : 1], tg1[kEarly ? LD : 1];
  if constexpr (kEarly) if (chain && tailT > 0) {
    load_row<LD>(X + static_cast<size_t>(tc0) * LD, tg);
    load_row<LD>(X + static_cast<size_t>(tc1) * LD, tg1);
  }
  if (kCoop && chain && CORA_COOP_PREFETCH_LATE) coop_prefetch();
  double acc[D][LD], acct[LD];  // the pose's d rotation rows; its translation row (chain slices)
#pragma unroll
  for (int j = 0; j < LD; ++j) {
    acct[j] = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) acc[a][j] = 0.0;
  }
  // rows of X: a local rotation / translation row from the windows when they are on, from memory otherwise
  auto x_rot = [&](int row, double (&x)[LD]) {
    if (kWinLD && kWin) {
#pragma unroll
      for (int j = 0; j < LD; ++j) x[j] = win[(row - w0) * LD + j];
    } else {
      load_row<LD>(X + static_cast<size_t>(row) * LD, x);
    }
  };
  auto x_trn = [&](int row, double (&x)[LD]) {
    if (kWinLD && kTrnRows > 0 && kWin) {
#pragma unroll
      for (int j = 0; j < LD; ++j) x[j] = win[(kRotRows + row - t0) * LD + j];
    } else {
      load_row<LD>(X + static_cast<size_t>(row) * LD, x);
    }
  };
  // one slot: column index, d values, the row of X (from the windows when they are on), d x LD products
  auto slot_apply = [&](const int32_t c, const double (&v)[D]) {
    double x[LD];
    if (kWinLD && kWin) {
      const unsigned rr = static_cast<unsigned>(c - w0), rt = static_cast<unsigned>(c - t0);
      const bool in_rot = rr < static_cast<unsigned>(nrot), in_trn = rt < static_cast<unsigned>(ntr);
      const int l = in_rot ? static_cast<int>(rr) : (in_trn ? kRotRows + static_cast<int>(rt) : 0);
#pragma unroll
      for (int j = 0; j < LD; ++j) x[j] = win[l * LD + j];
      if (!(in_rot || in_trn)) load_row<LD>(X + static_cast<size_t>(c) * LD, x);
    } else {
      load_row<LD>(X + static_cast<size_t>(c) * LD, x);
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int j = 0; j < LD; ++j) acc[a][j] = fma(v[a], x[j], acc[a][j]);
  };
  // The tail of the translation row (range measurements, loop closures): T entries of the slice, sorted by lane, gathered
  // by the whole wavefront -- lane e takes entry e -- and handed to their owners with lane permutes in entry order (a
  // fixed order of summation); the owner's loop runs to the longest tail of the slice (kSliceTailMaxShift).
  double kap_t = 0.0;
  int t_own = 0;
  auto translation_tail = [&] {
    const int T = tailT;
    const int mc = (sd.type >> kSliceTailMaxShift) & kSliceTailMaxMask;
    if (T > 0) {
      const int tstart = tinfo & 0xffff, tnloc = (tinfo >> 24) & 0x7f;
      // (pairs [0, nlocal) read rows of this shard, the rest rows of other ranks: a launch ahead of the exchange leaves
      // the rest to a later launch of the same slice that adds only them)
      const int tcnt = (sflags & kSliceSkipRemoteTail) ? tnloc : ((tinfo >> 16) & 0x7f);
      // (the remote pairs are summed on their own and added last: the same operations in the same order as the two
      // launches of a split slice, so the overlapped product of a partitioned handle has the serial one's bits)
      double accr[LD];
#pragma unroll
      for (int j = 0; j < LD; ++j) accr[j] = 0.0;
      for (int r0 = 0; r0 < T; r0 += kWave) {
        double pr[LD];
        if (kEarly && r0 == 0) {
#pragma unroll
          for (int j = 0; j < LD; ++j) pr[j] = fma(tv0, tg[kEarly ? j : 0], tv1 * tg1[kEarly ? j : 0]);
        } else if (r0 == 0) {
          double x[LD], x1[LD];
          load_row<LD>(X + static_cast<size_t>(tc0) * LD, x);
          load_row<LD>(X + static_cast<size_t>(tc1) * LD, x1);
#pragma unroll
          for (int j = 0; j < LD; ++j) pr[j] = fma(tv0, x[j], tv1 * x1[j]);
        } else {  // more than 64 pairs (128 entries) in one slice: rare
          const int e = r0 + lane;
          int2 c2 = make_int2(sd.row0, sd.row0);
          double2 v2 = make_double2(0.0, 0.0);
          if (e < T) {
            c2 = *reinterpret_cast<const int2 *>(tail_c + 2 * e);
            v2 = *reinterpret_cast<const double2 *>(tail_v + 2 * e);
          }
          double x[LD], x1[LD];
          load_row<LD>(X + static_cast<size_t>(c2.x) * LD, x);
          load_row<LD>(X + static_cast<size_t>(c2.y) * LD, x1);
#pragma unroll
          for (int j = 0; j < LD; ++j) pr[j] = fma(v2.x, x[j], v2.y * x1[j]);
        }
        for (int i = 0; i < mc; ++i) {  // wave-uniform
          const int e2 = tstart + i - r0;
          const bool mine = i < tcnt && e2 >= 0 && e2 < kWave, rem = i >= tnloc;
#pragma unroll
          for (int j = 0; j < LD; ++j) {
            const double t = __shfl(pr[j], e2 & (kWave - 1), kWave);
            acct[j] += (mine && !rem) ? t : 0.0;
            accr[j] += (mine && rem) ? t : 0.0;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < LD; ++j) acct[j] += accr[j];
    }
    if (EPI == EPI_HVP_K && lane < sd.nrows) {  // the translation row is final (no epilogue touches it): its share of <X, out>
      double x[LD];
      x_trn(t_own, x);
      kap_t = dot_row<LD>(x, acct);
    }
  };
  const double *__restrict__ vpg = vp;    // the general slots: index + d values
  const int32_t *__restrict__ cpg = cp;
  if (chain) {
    vpg = vp + static_cast<size_t>(kFV) * kWave;
    cpg = cp + kWave;
    // implied columns: rows of the lane's pose, the pose after and the pose before (clamped to the local poses where
    // there is none: the values there are zeros)
    const int np = A.n_local_poses, P = sd.aux0 + lane, Pc = min(P, np - 1);
    const int own_row = A.win_rot_lo + Pc * D, nxt_row = A.win_rot_lo + min(Pc + 1, np - 1) * D,
              prv_row = A.win_rot_lo + max(Pc - 1, 0) * D;
    const int t_nxt = A.win_trn_lo + min(Pc + 1, np - 1), t_prv = A.win_trn_lo + max(Pc - 1, 0);
    t_own = A.win_trn_lo + Pc;
    // value `slot` of the lane before (lane 0: entry h of the head block, which lane h loaded with the fixed slots and
    // hands over through a scalar register; no pose before: 0)
    // (a DPP wave shift: lane 0 keeps the "old" operand, which is the head entry.  The head block of a shard's first
    // pose is zeros -- format_build.cpp -- and every other lane has a pose before it, so there is nothing to mask.)
    auto before = [&](double mine, int slot, int h) {
      const int hlo = __builtin_amdgcn_readlane(__double2loint(headv), h), hhi = __builtin_amdgcn_readlane(__double2hiint(headv), h);
      if constexpr (kNxtRegs) {
        return __hiloint2double(__builtin_amdgcn_update_dpp(hhi, __double2hiint(mine), 0x138, 0xf, 0xf, false),
                                __builtin_amdgcn_update_dpp(hlo, __double2loint(mine), 0x138, 0xf, 0xf, false));
      } else {
        const double t = lane > 0 ? stream_load(vp + static_cast<size_t>(slot) * kWave - 1) : 0.0;
        return lane == 0 ? __hiloint2double(hhi, hlo) : t;
      }
    };
    // (wide rows: the groups of fixed slots are kept apart -- the scheduler otherwise hoists every group's loads to the top
    // of the block and the register file cannot hold them beside the accumulators)
    auto phase_fence = [] { if constexpr (!kEarly) __builtin_amdgcn_sched_barrier(0); };
    // (a) columns t_P and t_{P+1}: d + 1 values each (the rotation rows and the translation row)
    double s0[D + 1], s1[D + 1];
#pragma unroll
    for (int a = 0; a <= D; ++a) {
      s0[a] = fixed(a);
      s1[a] = fixed(D + 1 + a);
    }
    // (b) what the translation row takes from the lane before: Q(t_P, rot(P-1)_c) = its s1[c], Q(t_P, t_{P-1}) = its s1[d]
    double ps1[D + 1];
#pragma unroll
    for (int c = 0; c <= D; ++c) ps1[c] = before(s1[c], D + 1 + c, D * D + c);
    if constexpr (!kFuseT) {
      // wide rows: the whole translation row now -- Q33's three entries, the rotation columns of the pose and of the pose
      // before (Q31 = Q13^T), the tail -- stored at once; its accumulator row is free again for the rotation rows
      double x[LD];
      x_trn(t_own, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) acct[j] = s0[D] * x[j];
      x_trn(t_nxt, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) acct[j] = fma(s1[D], x[j], acct[j]);
      x_trn(t_prv, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) acct[j] = fma(ps1[D], x[j], acct[j]);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        x_rot(prv_row + c, x);
#pragma unroll
        for (int j = 0; j < LD; ++j) acct[j] = fma(ps1[c], x[j], acct[j]);
        x_rot(own_row + c, x);
#pragma unroll
        for (int j = 0; j < LD; ++j) acct[j] = fma(s0[c], x[j], acct[j]);
      }
      translation_tail();
      if (lane < sd.nrows) store_row<LD>(A.out + static_cast<size_t>(t_own) * LD, acct);
      phase_fence();
    }
    {
      double x[LD];
      x_trn(t_own, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) {
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a][j] = fma(s0[a], x[j], acc[a][j]);
        if constexpr (kFuseT) acct[j] = fma(s0[D], x[j], acct[j]);
      }
      x_trn(t_nxt, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) {
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a][j] = fma(s1[a], x[j], acc[a][j]);
        if constexpr (kFuseT) acct[j] = fma(s1[D], x[j], acct[j]);
      }
    }
    if constexpr (kFuseT) {
      double x[LD];
      x_trn(t_prv, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) acct[j] = fma(ps1[D], x[j], acct[j]);
    }
    // (c) the next pose's block, (d) the previous pose's block = the transposed next block of the lane before
    phase_fence();
    double nxt[D][D];  // [c][a] = Q(rot(P)_a, rot(P+1)_c)
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int a = 0; a < D; ++a) nxt[c][a] = fixed(2 * (D + 1) + c * D + a);
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double x[LD];
      x_rot(nxt_row + c, x);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int j = 0; j < LD; ++j) acc[a][j] = fma(nxt[c][a], x[j], acc[a][j]);
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double x[LD];
      x_rot(prv_row + c, x);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const double pv = before(nxt[a][c], 2 * (D + 1) + a * D + c, a * D + c);  // Q(rot(P)_a, rot(P-1)_c)
#pragma unroll
        for (int j = 0; j < LD; ++j) acc[a][j] = fma(pv, x[j], acc[a][j]);
      }
      if constexpr (kFuseT) {
#pragma unroll
        for (int j = 0; j < LD; ++j) acct[j] = fma(ps1[c], x[j], acct[j]);
      }
    }
    // (e) the pose's own block -- S_P = sym(Q_PP) - Lambda_P when an epilogue subtracts Lambda; the translation row's
    // share of these columns is Q(t_P, rot(P)_c) = s0[c]
    phase_fence();
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double v[D], x[LD];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if constexpr (kFold) v[a] = sym(kSymSlot(a, c, D));
        else v[a] = fixed(2 * (D + 1) + D * D + c * D + a);
      }
      x_rot(own_row + c, x);
#pragma unroll
      for (int j = 0; j < LD; ++j) {
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a][j] = fma(v[a], x[j], acc[a][j]);
        if constexpr (kFuseT) acct[j] = fma(s0[c], x[j], acct[j]);
      }
    }
  }
  CORA_PHASE(1);  // fixed slots done
  auto slot = [&](int k) {
    double v[D];
    const int32_t c = stream_load(cpg + static_cast<size_t>(k) * kWave);
#pragma unroll
    for (int a = 0; a < D; ++a) v[a] = stream_load(vpg + (static_cast<size_t>(k) * D + a) * kWave);
    slot_apply(c, v);
  };
  // slots in flight per lane: CORA_POSE_UNROLL_WIN with the windows; without, 3 up to a row stride of 6, 2 above
  // (register pressure: p = 10 Hvp 40.1 -> 39.4 us)
  if (kWin) {
#pragma unroll CORA_POSE_UNROLL_WIN
    for (int k = 0; k < sd.width; ++k) slot(k);
  } else {
    constexpr int kSlotsInFlight = LD <= 6 ? CORA_POSE_UNROLL : 2;
#pragma unroll kSlotsInFlight
    for (int k = 0; k < sd.width; ++k) slot(k);
  }
  CORA_PHASE(2);  // general slots done
  if (kFuseT && chain) translation_tail();
  CORA_PHASE(3);  // tail done
  // the slice's result rows leave through LDS: rotation rows and translation rows are runs of consecutive rows, stored as
  // full 512-byte pieces instead of 16-byte pieces of 64 different lines
  auto staged_store = [&] {
    __syncthreads();
    CORA_PHASE(4);  // projected
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int j = 0; j < LD; ++j) win[(lane * D + a) * LD + j] = acc[a][j];
    if (kFuseT && chain) {
#pragma unroll
      for (int j = 0; j < LD; ++j) win[kYEl + lane * LD + j] = acct[j];
    }
    __syncthreads();
    double *__restrict__ op = A.out + static_cast<size_t>(sd.row0) * LD;
#pragma unroll
    for (int i = 0; i < kYIt; ++i) {
      const int e = 2 * (i * kWave + lane), n = sd.nrows * D * LD;
      if (e + 1 < n) {
        Pair8 v{win[e], win[e + 1]};
        *reinterpret_cast<Pair8 *>(op + e) = v;
      } else if (e < n) {
        op[e] = win[e];
      }
    }
    if (kFuseT && chain) {  // the slice's translation rows: consecutive rows as well
      double *__restrict__ ot = A.out + static_cast<size_t>(A.win_trn_lo + sd.aux0) * LD;
      constexpr int kTIt = (LD + 1) / 2;
#pragma unroll
      for (int i = 0; i < kTIt; ++i) {
        const int e = 2 * (i * kWave + lane), n = sd.nrows * LD;
        if (e + 1 < n) {
          Pair8 v{win[kYEl + e], win[kYEl + e + 1]};
          *reinterpret_cast<Pair8 *>(ot + e) = v;
        } else if (e < n) {
          ot[e] = win[kYEl + e];
        }
      }
    }
  };
  if constexpr (kCoopT) if (kCoop) {
    // the pose's own rows of X (inside the rotation window; lanes past nrows read rows they ignore): <X, out> needs them,
    // and so does a plain slice, which subtracts Lambda_P X_P here (a chain slice has it in S_P)
    auto x_own = [&](int b, double (&x)[LD]) {
      const int l = sd.row0 + lane * D + b - w0;
#pragma unroll
      for (int j = 0; j < LD; ++j) x[j] = win[l * LD + j];
    };
    constexpr bool kKap = EPI == EPI_HVP_K;
    double xo[kKap ? D : 1][LD];
    if constexpr (kKap) {
#pragma unroll
      for (int b = 0; b < D; ++b) x_own(b, xo[b]);
    }
    if (!chain) {
      const double *__restrict__ Lp = A.lam_st + static_cast<size_t>(sd.aux0 + min(lane, sd.nrows - 1)) * (D * D);
#pragma unroll
      for (int b = 0; b < D; ++b) {
        double x[LD];
        if constexpr (kKap) {
#pragma unroll
          for (int j = 0; j < LD; ++j) x[j] = xo[kKap ? b : 0][j];
        } else {
          x_own(b, x);
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double lam = Lp[a * D + b];
#pragma unroll
          for (int j = 0; j < LD; ++j) acc[a][j] = fma(-lam, x[j], acc[a][j]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kYIt; ++i) {
      const int e = 2 * (i * kWave + lane);
      if (e < kYEl) win[e] = ystage[2 * i];
      if (e + 1 < kYEl) win[e + 1] = ystage[2 * i + 1];
    }
    __syncthreads();
    double y[D][LD];
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
      for (int j = 0; j < LD; ++j) y[b][j] = win[(lane * D + b) * LD + j];
    stiefel_project_thread<LD, D>(y, acc);
    double kap = 0.0;
    if (kKap && lane < sd.nrows) {
#pragma unroll
      for (int a = 0; a < D; ++a) kap += dot_row<LD>(xo[kKap ? a : 0], acc[a]);
    }
    staged_store();
    return kap + kap_t;
  }
  const bool active = lane < sd.nrows;
  if (!kStaged && !active) return 0.0;
  if (!kStaged && kFuseT && chain) store_row<LD>(A.out + static_cast<size_t>(t_own) * LD, acct);
  const size_t prow = static_cast<size_t>(sd.row0) + static_cast<size_t>(lane) * D;
  constexpr bool kKeepX = EPI == EPI_HVP_K && D * LD <= 18;  // the pose's own rows of X stay in registers for <X, out>
  double xs[kKeepX ? D : 1][LD];
  if (EPI != EPI_NONE && active) {
    auto x_own = [&](int b, double (&x)[LD]) {
      if (kWinLD && kWin) {  // the pose's own rows are inside the rotation window
        const int l = sd.row0 + lane * D + b - w0;
#pragma unroll
        for (int j = 0; j < LD; ++j) x[j] = win[l * LD + j];
      } else {
        load_row<LD>(X + (prow + b) * LD, x);
      }
    };
    if (!chain) {  // plain slices: - Lambda_P X_P (a chain slice has it in S_P)
      const double *Lp = A.lam_st + static_cast<size_t>(sd.aux0 + lane) * (D * D);
#pragma unroll
      for (int b = 0; b < D; ++b) {
        double x[LD];
        x_own(b, x);
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double lam = Lp[a * D + b];
#pragma unroll
          for (int j = 0; j < LD; ++j) acc[a][j] = fma(-lam, x[j], acc[a][j]);
        }
        if (kKeepX) {
#pragma unroll
          for (int j = 0; j < LD; ++j) xs[kKeepX ? b : 0][j] = x[j];
        }
      }
    } else if (kKeepX) {
#pragma unroll
      for (int b = 0; b < D; ++b) x_own(b, xs[kKeepX ? b : 0]);
    }
    if (EPI >= EPI_HVP) {
      double y[D][LD];
#pragma unroll
      for (int b = 0; b < D; ++b) load_row<LD>(A.Y + (prow + b) * LD, y[b]);
      stiefel_project_thread<LD, D>(y, acc);
    }
  }
  double kap = 0.0;
  if constexpr (kStaged) {
    staged_store();
    if (!active) return 0.0;
  } else {
#pragma unroll
    for (int a = 0; a < D; ++a) store_row<LD>(A.out + (prow + a) * LD, acc[a]);
  }
  if (EPI == EPI_HVP_K) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
      if (kKeepX) {
        kap += dot_row<LD>(xs[kKeepX ? a : 0], acc[a]);
      } else {
        double x[LD];
        load_row<LD>(X + (prow + a) * LD, x);
        kap += dot_row<LD>(x, acc[a]);
      }
    }
  }
  return kap + kap_t;
}

// The gate of a staggered launch (SpmmArgs::stagger_ticks): the wavefront sleeps until `ticks` of the 100 MHz wall clock
// have passed since it got here.  It reads no memory and waits for nobody -- a clock and a trip count bound it: should
// the clock stand still, kStaggerMaxTrips sleeps of 128 cycles (about 0.2 ms) end it.
constexpr int kStaggerMaxTrips = 4096;
__device__ __forceinline__ void stagger_wait(int ticks) {
  const unsigned long long t_entry = wall_clock64();
  for (int i = 0; i < kStaggerMaxTrips && wall_clock64() - t_entry < static_cast<unsigned long long>(ticks); ++i)
    __builtin_amdgcn_s_sleep(2);
}

// One wavefront, one slice (lane = row, or lane = pose for the rotation rows).  Returns the lane's share of
// <X, out> over the rows it wrote (EPI_HVP_K; 0 otherwise).
template <int LD, int D, int EPI>
__device__ __forceinline__ double slice_wave(const SpmmArgs &A, const SliceDesc sd, int lane) {
  if ((sd.type & kSliceTypeMask) == kSliceStiefel) {
    if (sd.nrows & kSliceRemoteTailOnly) return remote_tail_only<LD, D, EPI>(A, sd, lane);
    // A pose slice that finds itself in an odd wave slot of its SIMD (HW_ID 3:0) -- the second of the two wavefronts
    // the SIMD holds -- starts late, so that its loads travel while the first one computes (launch_spmm sets
    // stagger_ticks for window-form launches only; wave-uniform; a negative value is the tests': every pose slice waits).
    // The cohort by residency measured better than every second slice of the list (profiles/hvp_stagger.md).  The gate
    // stands in front of the unchanged choice of the form: with the forms reordered around it the register counts of
    // most instances of the narrow strides moved.
    if (A.stagger_ticks != 0) {
      if (A.stagger_ticks < 0 || (__builtin_amdgcn_s_getreg((3 << 11) | 4) & 1)) stagger_wait(abs(A.stagger_ticks));
    }
    return A.win_on ? pose_slice<LD, D, EPI, true>(A, sd, lane) : pose_slice<LD, D, EPI, false>(A, sd, lane);
  }
  const double *__restrict__ vp = A.sval + sd.off + lane;
  const int32_t *__restrict__ cp = A.scol + sd.coff + lane;
  const double *__restrict__ X = A.X;

  // the epilogue's operands do not depend on the slots: requested first, so that they travel with the slots' own loads
  // (a wavefront of a row slice is a chain of dependent latencies: index -> row of X -> epilogue operands was one more)
  const bool active = lane < sd.nrows;
  const bool oblique = sd.type == kSliceOblique;
  const size_t row = !active ? static_cast<size_t>(A.win_rot_lo)
                             : (sd.type == kSliceEuclidPerm ? static_cast<size_t>(A.perm[sd.row0 + lane]) : static_cast<size_t>(sd.row0) + lane);
  double lam = 0.0, xo[LD], yo[LD];
  if (EPI != EPI_NONE && (oblique || EPI == EPI_HVP_K)) load_row<LD>(X + row * LD, xo);
  if (EPI != EPI_NONE && oblique) {
    if (active) lam = A.lam_ob[sd.aux0 + lane];
    if (EPI >= EPI_HVP) load_row<LD>(A.Y + row * LD, yo);
  }

  double acc[LD];
#pragma unroll
  for (int j = 0; j < LD; ++j) acc[j] = 0.0;

#pragma unroll CORA_ROW_UNROLL
  for (int k = 0; k < sd.width; ++k) {
    const double v = stream_load(vp + static_cast<size_t>(k) * kWave);
    const int32_t c = stream_load(cp + static_cast<size_t>(k) * kWave);
    double x[LD];
    load_row<LD>(X + static_cast<size_t>(c) * LD, x);
#pragma unroll
    for (int j = 0; j < LD; ++j) acc[j] = fma(v, x[j], acc[j]);
  }

  if (!active) return 0.0;
  double kap = 0.0;
  if (oblique && EPI != EPI_NONE) {
#pragma unroll
    for (int j = 0; j < LD; ++j) acc[j] = fma(-lam, xo[j], acc[j]);
    if (EPI >= EPI_HVP) {
      const double ip = dot_row<LD>(yo, acc);
#pragma unroll
      for (int j = 0; j < LD; ++j) acc[j] = fma(-ip, yo[j], acc[j]);
    }
  }
  store_row<LD>(A.out + row * LD, acc);
  if (EPI == EPI_HVP_K) kap = dot_row<LD>(xo, acc);
  return kap;
}

#if CORA_TU & 1
#ifdef CORA_SPMM_TIMES
__device__ unsigned long long g_spmm_times[3 * kSpmmTimesMax];
#endif
#ifndef CORA_SPMM_WAVES_PER_EU
#define CORA_SPMM_WAVES_PER_EU 3
#endif
#ifndef CORA_SPMM_MIN_WAVES_PER_EU
#define CORA_SPMM_MIN_WAVES_PER_EU 2  // (up to a row stride of CORA_SPMM_MIN2_MAX_LD; above, the accumulators alone need more)
#endif
#ifndef CORA_SPMM_MIN2_MAX_LD
#define CORA_SPMM_MIN2_MAX_LD 10
#endif
// The kernel is latency bound unless each wave keeps many loads in flight, so
// let the register allocator spend registers instead of squeezing for full occupancy (round 1: 8 waves per SIMD at
// 64 registers 31.3 us, 2 waves 20.4 us on the 10^5-pose graph).  With the X window the balance moved: what the memory
// side sustains is requests in flight per CU, and three lighter wavefronts per SIMD (<= 168 registers, two slots per
// trip) beat two heavier ones: Hvp 22.2 -> 21.4 us, HBM-resident 30.9 -> 29.2 us, inside the STPCG loop 27.8 -> 25.2 us;
// four per SIMD are no better (profiles/r03_kernel_evolution.md).
template <int LD, int D, int EPI>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LD <= CORA_SPMM_MIN2_MAX_LD ? CORA_SPMM_MIN_WAVES_PER_EU : 1, CORA_SPMM_WAVES_PER_EU)))
void k_spmm(const SpmmArgs A) {
  // one wavefront per block: the dispatcher balances the (uneven) slices.
  // EPI_HVP_K: the wavefront also leaves sum <X[row], out[row]> over the rows it finished in
  // kappa_partial[blockIdx.x] (every block writes its slot; k_kappa_finish adds them in slot order).
  constexpr bool KAPPA = EPI == EPI_HVP_K;
  const int lane = threadIdx.x;
  double kap = 0.0;
#ifdef CORA_SPMM_TIMES
  const unsigned long long dbg_t0 = wall_clock64();
  unsigned long long dbg_meta = 0xFFull << 32;
#endif
  if (static_cast<int>(blockIdx.x) < A.n_chunks) {
    // chunk blocks, also one contiguous range of the launch order per XCD: the pieces whose columns that XCD's slices read
    const int tc = static_cast<int>(blockIdx.x);
    const int cper = A.n_chunks >> 3;  // n_chunks is a multiple of 8
    const int pos = (tc & 7) * cper + (tc >> 3);
    // (a negative entry pads an XCD's list of pieces to the longest: long_image.h)
    const int ci = pos < A.n_real_chunks ? A.chunk_order[pos] : -1;
    if (ci >= 0) long_chunk_wave<LD, KAPPA>(A, ci);
  } else {
    // Slice blocks: XCD x (= blockIdx % 8, observed dispatch order; speed only)
    // walks its own contiguous eighth of the slice list, so neighbouring slices
    // share one L2.  n_chunks is padded to a multiple of 8 by the launcher.
    const int t = static_cast<int>(blockIdx.x) - A.n_chunks;
    const int per_xcd = (A.n_slices + 7) >> 3;
    const int s = (t & 7) * per_xcd + (t >> 3);
    if ((t >> 3) < per_xcd && s < A.n_slices) kap = slice_wave<LD, D, EPI>(A, A.slices[s], lane);
#ifdef CORA_SPMM_TIMES
    if ((t >> 3) < per_xcd && s < A.n_slices)
      dbg_meta = (static_cast<unsigned long long>(A.slices[s].type) << 32) | static_cast<unsigned>(A.slices[s].width);
#endif
  }
  if (KAPPA) {
    kap = wave_sum(kap);
    if (lane == 0) A.kappa_partial[blockIdx.x] = kap;
  }
#ifdef CORA_SPMM_TIMES
  // measurement build only (tools/spmm_timeline.py): start / end of every wavefront on the 100 MHz wall clock
  if (lane == 0 && blockIdx.x < kSpmmTimesMax) {
    g_spmm_times[3 * blockIdx.x] = dbg_t0;
    g_spmm_times[3 * blockIdx.x + 1] = wall_clock64();
    g_spmm_times[3 * blockIdx.x + 2] = dbg_meta;
  }
#endif
}

#endif  // CORA_TU & 1
