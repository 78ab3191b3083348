// Part of kernels.hip (included there, in this order, inside namespace cora).  the staged Cholesky solve: k_rowop, k_blockop, k_subblock and what they share -- CORA_TU & 4.
#if CORA_TU & 4
// ---------------------------------------------------------------------------
// Staged sparse Cholesky solves (trisolve.h): every step is one dependency-free
// sparse product  dst[out_row] = src0[out_row] + sum_k val_k * src[col_k]  over the
// rows of a stage.  Block ranges of one launch: 8-lane rows, wavefront rows, chunks
// of the long (landmark) rows, whose partial sums the last chunk to finish adds up (ticket).
// Reference: CHOLMOD solve behind src/CORA_preconditioners.cpp:46-83.
// ---------------------------------------------------------------------------
// acc += sum_k val[k] * src[col[k]] over k = k0, k0 + stride, ... < k1.  Batches of eight PREDICATED entries (no
// remainder loop): the index / value loads of a batch are in flight together, then its eight row gathers -- two
// dependent round trips per batch, where a remainder loop pays two per entry.  Rows of the staged solves are short
// (<= 8 entries per lane in the 8-lane and chunk classes), so this is what bounds the kernel.
template <int LD>
__device__ __forceinline__ void rowop_entries(const int32_t *__restrict__ col, const double *__restrict__ val,
                                              const double *__restrict__ src, int k0, int k1, int stride,
                                              double (&acc)[LD]) {
  for (int kb = k0; kb < k1; kb += 8 * stride) {
    int32_t c[8];
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb + u * stride;
      const bool ok = k < k1;
      const int kk = ok ? k : kb;
      c[u] = col[kk];
      const double vv = val[kk];
      v[u] = ok ? vv : 0.0;
    }
#pragma unroll
    for (int h = 0; h < 8; h += 4) {
      double xx[4][LD];
#pragma unroll
      for (int u = 0; u < 4; ++u) load_row<LD>(src + static_cast<size_t>(c[h + u]) * LD, xx[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < LD; ++j) acc[j] = fma(v[h + u], xx[u][j], acc[j]);
    }
  }
}

// The two reductions of a sweep-fused STPCG iteration (RvTail, kernels.h) in ONE block, fixed order: <r, r> from the
// forward sweep's slots, then <r, v> = |L^-1 r|^2 from its |y|^2 slots and the squared norms of the last stage's rows.
__device__ __forceinline__ double lane_sum_slots_256(const double *__restrict__ x, int n) {  // a lane's share (no barrier)
  double s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = 0.0;
  for (int b0 = threadIdx.x; b0 < n; b0 += 256 * 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = b0 + 256 * u;
      t[u] = x[i < n ? i : n - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += (b0 + 256 * u < n) ? t[u] : 0.0;
  }
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}
__device__ __forceinline__ void rv_tail_block(const RvTail &T) {
  __shared__ double sm[12];
  StpcgState L = {};
  if (threadIdx.x == 0 && !T.sums_out) L = *T.st;  // in flight while the slots are added up
  // the three sets of slots are loaded together (one round trip, not three), then reduced one after the other
  const double l_rr = lane_sum_slots_256(T.rr_partial, T.n_rr);
  const double l_yy = lane_sum_slots_256(T.yy_partial, T.n_yy);
  const double l_tt = lane_sum_slots_256(T.rowsq, T.n_rowsq);
  __shared__ double ksm[4];
  const double kappa = T.n_kappa > 0 ? kappa_sum_256(T.kappa_partial, T.n_kappa, ksm) : 0.0;  // (wave-uniform branch)
  const double rr = block_sum_256(l_rr, sm);
  const double yy = block_sum_256(l_yy, sm + 4);
  const double tt = block_sum_256(l_tt, sm + 8);
  if (threadIdx.x == 0) {
    if (T.sums_out) {  // partitioned: this rank's share of the two inner products
      T.sums_out[0] = rr;
      T.sums_out[1] = yy + tt;
      return;
    }
    if (T.n_kappa > 0) stpcg_after_kappa(L, kappa);  // the iteration's first scalar step, which no launch of its own ran
    if (T.n_rr > 0) stpcg_after_rr(L, rr);  // (n_rr == 0: <r, r> was finished by the residual pass)
    stpcg_after_rv(L, yy + tt);
    *T.st = L;
    *T.st_host = L;  // pinned mirror for the host's (infrequent) look
    if (T.seq_out) {
      unsigned long long seq = T.seq;
      if (T.seq_counter) *T.seq_counter = seq = *T.seq_counter + 1;
      __threadfence_system();
      __hip_atomic_store(T.seq_out, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <int LD>
__global__ __launch_bounds__(256) void k_rowop(RowOpDev op, const double *__restrict__ src0,
                                               const double *__restrict__ src, double *__restrict__ dst, const RvTail tail) {
  const int nb8 = (op.n8 + 31) >> 5, nb64 = (op.n64 + 3) >> 2;
  if (tail.st && blockIdx.x == gridDim.x - 1) {  // the extra block of a launch with a tail
    rv_tail_block(tail);
    return;
  }
  // Blocks are dispatched in index order and the chunks of the long rows are the longest chain of the launch (entries,
  // gathers, partial, ticket, the row's partials again): they take the first indices.  b below is the index in the order
  // 8-lane rows | wavefront rows | chunks that the rest of the kernel (and the slots of the row squares) uses.
  int b = static_cast<int>(blockIdx.x);
  {
    const int nbch = (op.nchunks + 3) >> 2;
    b = b < nbch ? nb8 + nb64 + b : b - nbch;
  }
  // optional: the squared norms of the product's rows, ONE SLOT PER WAVEFRONT (the eight rows of a wavefront of the 8-lane
  // class added in a fixed order; a row of the wavefront class; a long row) -- slot = 4 block + wavefront | 4 nb8 + row of
  // its class | 4 nb8 + n64 + long row.  (A slot per row -- 14 k of them on plaza2, 9 k at 10^5 poses -- made the block that
  // adds them up the longest chain of the NEXT launch: 7 dependent rounds of loads where the rows of that launch need
  // three.  A slot per block needed a barrier here: first product 13.8 -> 15.0 us at 10^5 poses.)
  double *__restrict__ rowsq = tail.st ? nullptr : tail.rowsq_out;
  double acc[LD];
#pragma unroll
  for (int j = 0; j < LD; ++j) acc[j] = 0.0;
  if (b < nb8) {  // 32 rows per block, 8 lanes each
    const int r = (b << 5) + (static_cast<int>(threadIdx.x) >> 3), g = threadIdx.x & 7;
    const bool ok = r < op.n8;
    int orow = 0;
    if (ok) {
      orow = op.out_row[r];
      if (src0 && g == 0) load_row<LD>(src0 + static_cast<size_t>(orow) * LD, acc);
      rowop_entries<LD>(op.col, op.val, src, op.begin[r] + g, op.end[r], 8, acc);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1)
#pragma unroll
      for (int j = 0; j < LD; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
    double sq = 0.0;
    if (ok && g == 0) {
      store_row<LD>(dst + static_cast<size_t>(orow) * LD, acc);
      if (rowsq) sq = dot_row<LD>(acc, acc);
    }
#ifdef CORA_ROWSQ_PER_ROW
    if (rowsq && ok && g == 0) rowsq[r] = sq;
#else
    if (rowsq) {  // (block-uniform)
      const double t = wave_sum(sq);
      if ((threadIdx.x & 63) == 0) rowsq[(b << 2) + (static_cast<int>(threadIdx.x) >> 6)] = t;
    }
#endif
  } else if (b < nb8 + nb64) {  // one wavefront per row
    const int r = op.n8 + ((b - nb8) << 2) + (static_cast<int>(threadIdx.x) >> 6), g = threadIdx.x & 63;
    if (r >= op.n8 + op.n64) return;  // (wave-uniform)
    const int orow = op.out_row[r];
    if (src0 && g == 0) load_row<LD>(src0 + static_cast<size_t>(orow) * LD, acc);
    rowop_entries<LD>(op.col, op.val, src, op.begin[r] + g, op.end[r], 64, acc);
#pragma unroll
    for (int j = 0; j < LD; ++j) acc[j] = wave_sum(acc[j]);
    if (g == 0) {
      store_row<LD>(dst + static_cast<size_t>(orow) * LD, acc);
#ifdef CORA_ROWSQ_PER_ROW
      if (rowsq) rowsq[r] = dot_row<LD>(acc, acc);
#else
      if (rowsq) rowsq[(nb8 << 2) + (r - op.n8)] = dot_row<LD>(acc, acc);
#endif
    }
  } else {  // one wavefront per chunk of a long row
    const int ch = ((b - nb8 - nb64) << 2) + (static_cast<int>(threadIdx.x) >> 6), g = threadIdx.x & 63;
    if (ch >= op.nchunks) return;
    // (what the hand-off below needs is requested with the chunk's bounds, not after its entries: three dependent round
    // trips fewer at the end of the longest chain of the launch)
    const int r = op.chunk_row[ch];
    const int c0 = op.long_chunk_ptr[r], c1 = op.long_chunk_ptr[r + 1];
    const size_t long_orow = static_cast<size_t>(op.long_out[r]);
    rowop_entries<LD>(op.col, op.val, src, op.chunk_begin[ch] + g, op.chunk_end[ch], 64, acc);
    double tot = 0.0;  // lane j < LD ends up with column j
#pragma unroll
    for (int j = 0; j < LD; ++j) {
      const double v = __shfl(wave_sum(acc[j]), 0, 64);
      if (g == j) tot = v;
    }
    // publish the partial write-through, take a ticket of the row; the last chunk to arrive adds the row's
    // partials in chunk order (deterministic) -- the hand-off of k_spmm's long rows
    if (g < LD)
      __hip_atomic_store(op.partial + static_cast<size_t>(ch) * kMaxLD + g, tot, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int last = 0;
    if (g == 0) {
      const unsigned old = __hip_atomic_fetch_add(op.tickets + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = (old == static_cast<unsigned>(c1 - c0 - 1));
      if (last) __hip_atomic_store(op.tickets + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = __shfl(last, 0, 64);
    if (last) {  // wave-uniform: lane g adds chunks g, g + 64, ... (loads all in flight), then a fixed shuffle tree
      const double *P = op.partial + static_cast<size_t>(c0) * kMaxLD;
      const int nc = c1 - c0;
      double part[LD];
#pragma unroll
      for (int j = 0; j < LD; ++j) part[j] = 0.0;
      for (int c = g; c < nc; c += 64)
#pragma unroll
        for (int j = 0; j < LD; ++j)
          part[j] += __hip_atomic_load(P + static_cast<size_t>(c) * kMaxLD + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int j = 0; j < LD; ++j) part[j] = wave_sum(part[j]);
      if (g == 0) {
        const size_t orow = long_orow;
        if (src0) {
          double b0[LD];
          load_row<LD>(src0 + orow * LD, b0);
#pragma unroll
          for (int j = 0; j < LD; ++j) part[j] += b0[j];
        }
        store_row<LD>(dst + orow * LD, part);
#ifdef CORA_ROWSQ_PER_ROW
        if (rowsq) rowsq[op.n8 + op.n64 + r] = dot_row<LD>(part, part);
#else
        if (rowsq) rowsq[(nb8 << 2) + op.n64 + r] = dot_row<LD>(part, part);
#endif
      }
    }
  }
}

// LDS hand-off between the lanes of one wavefront (no workgroup barrier: the waves of a block work on
// different blocks of the factor and run different trip counts)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v where the lane's bit of the wave-uniform mask m is set, 0 elsewhere: the mask is used as the select
// condition directly (two v_cndmask), no per-lane bit test
__device__ __forceinline__ double select_by_lane_mask(double v, uint64_t m) {
  unsigned lo = static_cast<unsigned>(__double2loint(v)), hi = static_cast<unsigned>(__double2hiint(v));
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(lo) : "v"(lo), "s"(m));
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(hi) : "v"(hi), "s"(m));
  return __hiloint2double(static_cast<int>(hi), static_cast<int>(lo));
}

// Stage 0 in block form (trisolve.h): one wavefront per block, lane = row of the block.
//   forward : dst[rows] = W src[rows]
//   backward: t = src[rows] - L[later, rows]^T src[later rows];  dst[rows] = W^T t   (src may be dst:
//             a block reads its own rows before it writes them and nobody else reads them)
// The kernel is bound by VALU issue, not by bandwidth (8 waves / SIMD, ~60 columns each), so the loop over
// the columns q of W keeps everything wave-uniform on the scalar side: mask and offset of column q come
// from one scalar load, the lane's entry is base + popcount(mask below the lane).
template <int LD, bool BWD>
__global__ __launch_bounds__(256) void k_blockop(BlockOpDev B, const double *src, double *dst) {
  __shared__ double tl[4][64][LD];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * 4 + wv);
  if (b >= B.nblocks) return;  // wave-uniform; the waves of a workgroup never synchronise with each other
  const BlockDesc bd = B.desc[b];
  const int nb = bd.nrows, rb = bd.row_begin;
  const BlockLane *__restrict__ meta = (BWD ? B.by_row : B.by_col) + bd.meta_begin;
  const bool mine = lane < nb;
  const size_t row = mine ? static_cast<size_t>(meta[lane].row) : 0;
  {
    double t[LD];
#pragma unroll
    for (int j = 0; j < LD; ++j) t[j] = 0.0;
    if (mine) load_row<LD>(src + row * LD, t);
    if constexpr (BWD) {
    // coupling to the later stages: the lanes stride over ALL entries of the block (independent gathers),
    // park the products in LDS, and every row then adds up its own segment in entry order
    const int e0 = B.ext_ptr[rb], e1 = B.ext_ptr[rb + nb];
    const int my0 = mine ? B.ext_ptr[rb + lane] : 0, my1 = mine ? B.ext_ptr[rb + lane + 1] : 0;
    for (int base = e0; base < e1; base += 64) {
      const int k = base + lane;
      double p[LD];
#pragma unroll
      for (int j = 0; j < LD; ++j) p[j] = 0.0;
      if (k < e1) {
        const double v = B.ext_val[k];
        load_row<LD>(src + static_cast<size_t>(B.ext_col[k]) * LD, p);
#pragma unroll
        for (int j = 0; j < LD; ++j) p[j] *= v;
      }
#pragma unroll
      for (int j = 0; j < LD; ++j) tl[wv][lane][j] = p[j];
      wave_lds_sync();
      const int lo = my0 > base ? my0 : base, hi = my1 < base + 64 ? my1 : base + 64;
      for (int q = lo; q < hi; ++q)
#pragma unroll
        for (int j = 0; j < LD; ++j) t[j] += tl[wv][q - base][j];
      wave_lds_sync();
    }
    }
#pragma unroll
    for (int j = 0; j < LD; ++j) tl[wv][lane][j] = t[j];
    wave_lds_sync();
  }
  double acc[LD];
#pragma unroll
  for (int j = 0; j < LD; ++j) acc[j] = 0.0;
  const char *__restrict__ W = reinterpret_cast<const char *>((BWD ? B.w_by_row : B.w_by_col) + bd.w_off);
  // Eight columns per round.  Wave-uniform part: two wide scalar loads bring the round's eight 16-byte records
  // {mask, off, row} (every block's records are padded to a multiple of eight with empty masks).  Lanes outside a
  // column's mask read some nearby entry (the value arrays are padded) and drop it.  The next round's records and
  // entries are requested before this round's products are formed, so a wave always has a round in flight.
  typedef int i32x16 __attribute__((ext_vector_type(16), aligned(16)));
  auto issue = [&](const i32x16 &ra, const i32x16 &rc, double(&w)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned mlo = static_cast<unsigned>(u < 4 ? ra[4 * u] : rc[4 * (u - 4)]);
      const unsigned mhi = static_cast<unsigned>(u < 4 ? ra[4 * u + 1] : rc[4 * (u - 4) + 1]);
      const unsigned off = static_cast<unsigned>(u < 4 ? ra[4 * u + 2] : rc[4 * (u - 4) + 2]);
      const unsigned rank = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
      // scalar base + 32-bit byte offset: one VALU op for the address
      w[u] = *reinterpret_cast<const double *>(W + ((rank << 3) + (off << 3)));
    }
  };
  // (the right-hand side rows t_q through the scalar cache instead of the LDS tile: measured 37 us against 25)
  auto products = [&](const i32x16 &ra, const i32x16 &rc, const double(&w)[8], int q0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned mlo = static_cast<unsigned>(u < 4 ? ra[4 * u] : rc[4 * (u - 4)]);
      const unsigned mhi = static_cast<unsigned>(u < 4 ? ra[4 * u + 1] : rc[4 * (u - 4) + 1]);
      const double wu = select_by_lane_mask(w[u], static_cast<uint64_t>(mhi) << 32 | mlo);
      const int q = (q0 + u) & 63;
#pragma unroll
      for (int j = 0; j < LD; ++j) acc[j] = fma(wu, tl[wv][q][j], acc[j]);
    }
  };
  // two rounds per trip (A / B register sets) so that the prefetched round needs no copies
  i32x16 ra = *reinterpret_cast<const i32x16 *>(meta), rc = *reinterpret_cast<const i32x16 *>(meta + 4);
  double wa[8], wb[8];
  issue(ra, rc, wa);
  for (int q0 = 0; q0 < nb; q0 += 16) {
    const i32x16 sa = *reinterpret_cast<const i32x16 *>(meta + q0 + 8), sc = *reinterpret_cast<const i32x16 *>(meta + q0 + 12);
    issue(sa, sc, wb);  // past the block's end on its last round: the arrays are padded, the result is unused
    products(ra, rc, wa, q0);
    if (q0 + 8 >= nb) break;
    ra = *reinterpret_cast<const i32x16 *>(meta + q0 + 16);
    rc = *reinterpret_cast<const i32x16 *>(meta + q0 + 20);
    issue(ra, rc, wa);
    products(sa, sc, wb, q0 + 8);
  }
  if (mine) store_row<LD>(dst + row * LD, acc);
}


// ---------------------------------------------------------------------------
// Stage 0 as workgroup blocks solved by substitution (trisolve.h, SubBlockOpHost).  One workgroup of kSubThreads
// per block; only the block's right-hand sides sit in LDS (the tile T, rows x LD).  The block's part of L is
// STREAMED: the coefficients of a level are stored [entry slot u][lane] (coalesced), its local row indices
// [lane][4 or 8]; every lane fetches its <= kSubNpl entries of level l + 1 into registers while level l is
// computed (two register sets, ping-pong), so the HBM latency of the stream
// hides behind the LDS work of the level before, and four workgroups per CU -- the whole of a 10^5-pose problem
// resident at once -- keep the memory side busy without phases.  (The first version copied the block's entries into
// LDS before the first level: 75 KB per block, two blocks per CU, every block of a round streaming at the same
// time and computing at the same time: 20 us of row I/O + 8 us of stream + 17 us of levels, added up.)
//
// A level: lane (row, part) forms  sum_e val_e T[idx_e]  over its entries for ALL columns (columns in chunks of
// <= 6 accumulators), the g lanes of a row are summed with DPP, THEN (barrier) the rows of the level are written,
// then (barrier) the next level starts: the rows of a supernode read each other's right-hand sides.  Everything
// wave-uniform (level headers) stays on the scalar unit; wavefronts without a row only see the two barriers.
// ---------------------------------------------------------------------------
constexpr int kSubThreads = 256;  // >= rows x lanes per row of a level (plan: kLevelLanes)
constexpr int kSubNpl = 8;        // >= entries per lane of a level (plan: kLaneEntries)

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sum over aligned groups of g lanes (g a power of two, wave-uniform); every lane of the group gets the total.
// Neighbours first: quad permutes, then the half-row / row mirrors, then shuffles across rows of 16.
__device__ __forceinline__ double group_sum(double x, int g) {
  if (g >= 2) x += dpp_f64<0xB1>(x);    // quad_perm [1,0,3,2]
  if (g >= 4) x += dpp_f64<0x4E>(x);    // quad_perm [2,3,0,1]
  if (g >= 8) x += dpp_f64<0x141>(x);   // row_half_mirror
  if (g >= 16) x += dpp_f64<0x140>(x);  // row_mirror
  if (g >= 32) x += __shfl_xor(x, 16, 64);
  if (g >= 64) x += __shfl_xor(x, 32, 64);
  return x;
}

#ifndef CORA_SUB_NT
#define CORA_SUB_NT 1
#endif
// The factor is read once per sweep: its loads are non-temporal (CORA_SUB_NT = 1), so that 130 MB of L per STPCG
// iteration do not push Q and the vectors out of the 256 MB Infinity Cache.  Measured at 10^5 poses, p = 5: the
// product inside the loop 31.8 -> 24.9 us (its back-to-back rate), the iteration 166 -> 153 us.
template <typename T>
__device__ __forceinline__ T factor_load(const T *p) {
#if CORA_SUB_NT == 1
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

// the same for N values at once: one jump on log2(g), then every step exchanges all N values (independent DPP chains
// that overlap) instead of N x log2(g) conditional steps
template <int N>
__device__ __forceinline__ void group_sum_all(double (&x)[N], int gs) {
  auto steps = [&](auto gs_c) {
    constexpr int GS = decltype(gs_c)::value;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (GS >= 1) x[j] += dpp_f64<0xB1>(x[j]);
      if (GS >= 2) x[j] += dpp_f64<0x4E>(x[j]);
      if (GS >= 3) x[j] += dpp_f64<0x141>(x[j]);
      if (GS >= 4) x[j] += dpp_f64<0x140>(x[j]);
      if (GS >= 5) x[j] += __shfl_xor(x[j], 16, 64);
      if (GS >= 6) x[j] += __shfl_xor(x[j], 32, 64);
    }
  };
  switch (gs) {
    case 0: break;
    case 1: steps(std::integral_constant<int, 1>()); break;
    case 2: steps(std::integral_constant<int, 2>()); break;
    case 3: steps(std::integral_constant<int, 3>()); break;
    case 4: steps(std::integral_constant<int, 4>()); break;
    case 5: steps(std::integral_constant<int, 5>()); break;
    default: steps(std::integral_constant<int, 6>()); break;
  }
}

struct SubRegs {  // a lane's entries of one level: coefficients and (two per dword) local row indices
  double v[kSubNpl];
  uint32_t i[kSubNpl / 2];
  int32_t row;  // forward sweeps that store a level's rows as they are solved (kDirect): the internal row of the lane's row
};
// Pins a register set: the compiler waits HERE for whatever load still writes it (before the next level's loads are
// issued), and treats the values as opaque afterwards.
__device__ __forceinline__ void sub_touch(SubRegs &R) {
#pragma unroll
  for (int u = 0; u < kSubNpl; ++u) asm volatile("" : "+v"(R.v[u]));
#pragma unroll
  for (int u = 0; u < kSubNpl / 2; ++u) asm volatile("" : "+v"(R.i[u]));
  asm volatile("" : "+v"(R.row));
}

// v = Proj_Y(x) for the row unit that starts at `row` (a pose's d rotation rows: only its first row does the work;
// a range row; a translation row); sink(row, v) receives every row of the result.  row_of_x(a) -> the a-th row of x.
// (Rows of the last stage in the fused backward sweep.)
template <int LD, int D, typename RowOfX, typename Sink>
__device__ __forceinline__ void project_unit(const SubFuse &F, size_t row, RowOfX row_of_x, Sink sink) {
  if (row < static_cast<size_t>(F.rng_base)) {
    if ((row - static_cast<size_t>(F.rot_base)) % D != 0) return;
    double y[D][LD], v[D][LD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      load_row<LD>(F.Y + (row + a) * LD, y[a]);
      row_of_x(a, v[a]);
    }
    stiefel_project_thread<LD, D>(y, v);
#pragma unroll
    for (int a = 0; a < D; ++a) sink(row + a, v[a]);
    return;
  }
  double y[LD], v[LD];
  row_of_x(0, v);
  if (row < static_cast<size_t>(F.trn_base)) {
    load_row<LD>(F.Y + row * LD, y);
    const double ip = dot_row<LD>(y, v);
#pragma unroll
    for (int c = 0; c < LD; ++c) v[c] = fma(-ip, y[c], v[c]);
  }
  sink(row, v);
}

#ifndef CORA_SUB_MIN_BLOCKS
#define CORA_SUB_MIN_BLOCKS 4
#endif
#ifndef CORA_SUB_FWD_DIRECT
#define CORA_SUB_FWD_DIRECT 0  // 1: forward sweeps send a level's rows to memory when the level is solved (40-byte pieces from the
                               // lanes that hold them) instead of an epilogue of their own.  Built and measured in round 5, not kept:
                               // forward sweep at 10^5 poses 32.8 -> 35.4 us (with the folded kappa 35.8 -> 37.9) -- the level loop
                               // streams the factor at 4.8 TB/s while it runs at the LDS's bandwidth and has no room for 435 more
                               // stores and a row index per lane and level; the burst after the last level is the cheaper way
#endif
#ifndef CORA_SUB_LATE_FETCH
#define CORA_SUB_LATE_FETCH 1  // fused forward sweep: the first level's entries are requested behind the prologue's loads
#endif
#ifdef CORA_SUB_TIMES
// measurement build: wall-clock stamps of a substitution block's phases, forward and backward sweep apart
// (tools/sub_timeline.py): 0 start | 1 right-hand sides in the tile | 2 levels done | 3 end | 4 clocks spent waiting for
// a level's entries (wave 0) | 5 levels | 6.. shader-clock cycles of wave 0 inside the level loop, summed over the levels:
// 6 wait for the entries | 7 request of the next level's + header | 8 tile reads and products | 9 sums over a row's lanes |
// 10 first barrier | 11 rows into the tile | 12 second barrier | 13 unused
constexpr unsigned kSubTimesMax = 8192;
constexpr int kSubPhases = 14;
__device__ unsigned long long g_sub_phase[2 * kSubPhases * kSubTimesMax];
#define CORA_SUB_STAMP(i, v) do { if (threadIdx.x == 0 && blockIdx.x < kSubTimesMax) g_sub_phase[(BWD ? kSubPhases * kSubTimesMax : 0) + kSubPhases * blockIdx.x + (i)] = (v); } while (0)
#else
#define CORA_SUB_STAMP(i, v) do { } while (0)
#endif
// FD: 0 plain solve; 1 (forward) residual update fused into the prologue; 2 / 3 (backward) tangent projection for
// d = FD fused into the epilogue -- see SubFuse (kernels.h).
//
// Rows move between memory and the tile ELEMENT BY ELEMENT in memory order (SubSweep::io): a block is a few runs of
// consecutive rows, so a wavefront's load is 512 contiguous bytes whatever the row stride, and all loads of a phase
// are issued before the first one is consumed -- a phase costs two dependent latencies (index, value), not two per
// row.  (A lane per row: 40-byte pieces, 5 x the line requests; with the fused passes written that way the forward
// sweep took 50 us instead of 33.)
#ifndef CORA_SUB_PAD_TILE
#define CORA_SUB_PAD_TILE 1  // odd row strides: rows of the LDS tile padded to an even number of doubles (16-byte aligned rows)
#endif
// Row stride of a substitution block's tile in LDS, in doubles.  With an odd row stride (p = 5: the headline) a row of the
// tile was 8-byte aligned, so every tile read of the level loop was LD ds_read_b64 per entry; with the rows padded to an even
// stride they are 16-byte aligned and an entry costs LD / 2 ds_read_b128 + one b64 (p = 5: 3 LDS instructions instead of 5,
// the level loop's largest phase -- "tile reads and products", profiles/r05_kernel_evolution.md step 15).  Memory keeps
// its stride: only the tile's addressing changes.
template <int LD>
struct SubTile {
  static constexpr int kStride = (CORA_SUB_PAD_TILE && (LD % 2 == 1) && LD >= 3) ? LD + 1 : LD;
};
template <int LD, bool BWD, int FD>
__global__ __launch_bounds__(kSubThreads, CORA_SUB_MIN_BLOCKS) void k_subblock(SubOpDev S, const double *src, double *work, double *dst,
                                                              const SubFuse F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double dot_sm[8];
  double *T = reinterpret_cast<double *>(smem);
  const int tid = threadIdx.x;
  const int b = static_cast<int>(blockIdx.x);
  double dacc[4] = {0.0, 0.0, 0.0, 0.0};
  double cr = 0.0;
  // kappa folded into this launch (SubFuse::n_kappa): every block adds the product's partials itself and runs the scalar
  // step on a private copy of the state (the state is not written).  A solve block does that INSIDE its prologue, behind
  // the loads of its right-hand sides (kLateKappa below): the partials -- the same 20 KB for every block at 10^5 poses,
  // L2 hits -- travel with the block's 35 KB of r and Hp instead of ahead of them.
  auto folded_kappa = [&]() -> double {
    const double kappa = kappa_sum_256(F.kappa_partial, F.n_kappa, dot_sm);
    const double c = stpcg_coef_r_after_kappa(F.dot.st, kappa);
    __syncthreads();  // (dot_sm is used again below)
    return c;
  };
  const bool late_kappa = FD == 1 && F.n_kappa > 0 && b < S.nblocks;  // (block-uniform)
  if (FD == 1 && !late_kappa) cr = F.n_kappa > 0 ? folded_kappa() : F.dot.st->coef_r;
  // fused backward sweep: the step and the direction are updated on the way out (the scalars are final: the launch
  // before this one finished <r, v>)
  const double cs = (FD >= 2) ? F.dot.st->coef_s : 0.0, cv = (FD >= 2) ? F.dot.st->coef_v : 0.0,
               cb = (FD >= 2) ? F.dot.st->coef_beta : 1.0;
  // F.p == nullptr: the projected solution itself is the result (v -> dst: the stand-alone preconditioner apply)
  const bool store_v = FD >= 2 && F.p == nullptr;
  const bool upd = FD >= 2 && (store_v || !(cs == 0.0 && cv == 0.0 && cb == 1.0));  // false: solve already finished (enqueued ahead)
  if (b >= S.nblocks) {  // rows of the last stage: forward rhs -> work, backward work -> x
    const int t = (b - S.nblocks) * kSubThreads + tid;
    if (t < S.ntop) {
      const size_t row = static_cast<size_t>(S.top_rows[t]);
      if (FD == 0) {
        double x[LD];
        load_row<LD>((BWD ? work : src) + row * LD, x);
        store_row<LD>((BWD ? dst : work) + row * LD, x);
      } else if (FD == 1) {  // r += coef_r Hp, <r, r>
        double x[LD];
        load_row<LD>(F.r + row * LD, x);
        if (cr != 0.0) {
          double h[LD];
          load_row<LD>(F.Hp + row * LD, h);
#pragma unroll
          for (int j = 0; j < LD; ++j) x[j] = fma(cr, h[j], x[j]);
          store_row<LD>(F.r + row * LD, x);
        }
        dacc[0] = dot_row<LD>(x, x);
        store_row<LD>(work + row * LD, x);
      } else if (upd) {
        constexpr int D = FD >= 2 ? FD : 2;
        project_unit<LD, D>(F, row, [&](int a, double (&x)[LD]) { load_row<LD>(work + (row + a) * LD, x); },
                            [&](size_t rw, const double (&v)[LD]) {
                              if (store_v) {
                                store_row<LD>(dst + rw * LD, v);
                                return;
                              }
                              double pv[LD], sv[LD];
                              load_row<LD>(F.p + rw * LD, pv);
                              load_row<LD>(F.s + rw * LD, sv);
#pragma unroll
                              for (int j = 0; j < LD; ++j) {
                                sv[j] = fma(cs, pv[j], sv[j]);
                                pv[j] = fma(cv, v[j], cb * pv[j]);
                              }
                              store_row<LD>(F.s + rw * LD, sv);
                              store_row<LD>(F.p + rw * LD, pv);
                            });
      }
    }
    if (FD == 1) {  // <r, r> over these rows: a slot of its own (RvTail adds the slots up, no ticket)
      const double rr = block_sum_256(dacc[0], dot_sm);
      if (tid == 0) F.rr_partial[b] = rr;
    }
    return;
  }
  CORA_SUB_STAMP(0, wall_clock64());
  [[maybe_unused]] unsigned long long dbg_wait = 0;
  const SubSweep &Q = BWD ? S.bwd : S.fwd;
  const SubDesc bd = S.desc[b];
  const int nb = bd.nrows, rb = bd.row_begin;
  const int nlev = BWD ? bd.b_nlev : bd.f_nlev;
  const double *__restrict__ gv = Q.val + (BWD ? bd.b_ent_begin : bd.f_ent_begin);
  const uint16_t *__restrict__ gi = Q.idx;
  const int4 *__restrict__ gh = reinterpret_cast<const int4 *>(Q.hdr) + (BWD ? bd.b_lev_begin : bd.f_lev_begin);
  const int wave_base = __builtin_amdgcn_readfirstlane(tid);
  // level headers {first row, g | npl << 8 | rows << 12, first coefficient, first index}: staged in LDS behind the tile
  // (the loop below orders its loads with scheduling barriers, after which the compiler no longer reads global memory
  // through the scalar cache) and handed from level to level in scalar registers
  // A barrier level is kSubWaves headers, one per WAVEFRONT of the workgroup: {first row, lanes per row | entries per
  // lane << 8 | rows << 12, first coefficient, first index} of the rows that wavefront solves in the level (its own
  // width: short rows do not pay for the level's longest); nlev levels + a closing one.
  constexpr int kSubWaves = kSubThreads / 64;
  const int wv = wave_base >> 6;
  constexpr int LT = SubTile<LD>::kStride;  // row stride of the tile (doubles)
  int4 *hl = reinterpret_cast<int4 *>(smem + ((static_cast<size_t>(S.max_rows) * LT * 8 + 15) & ~static_cast<size_t>(15)));
  for (int i = tid; i < (nlev + 1) * kSubWaves; i += kSubThreads) hl[i] = gh[i];
  auto header = [&](int l) {
    const int4 h = hl[(l < nlev ? l : nlev) * kSubWaves + wv];  // the closing level has no rows
    return make_int4(__builtin_amdgcn_readfirstlane(h.x), __builtin_amdgcn_readfirstlane(h.y),
                     __builtin_amdgcn_readfirstlane(h.z), __builtin_amdgcn_readfirstlane(h.w));
  };
  const int wl = tid & 63;  // lane of the wavefront: a level's lanes are counted per wavefront
  // Forward sweeps store a level's rows the moment the level is solved (they are final): 40-byte pieces from the lanes
  // that hold them, in flight while the next levels run (a barrier waits for LDS only), instead of a burst of its own
  // after the last level with every block of the launch in the same phase.  |y|^2 is summed by the same lanes.
  constexpr bool kDirect = CORA_SUB_FWD_DIRECT && !BWD;
  const int32_t *__restrict__ grows = Q.rows + rb;  // internal row of every tile row (level order)

  // (Measured and dropped: entries of TWO levels ahead in a third register set.  The compiler only keeps loads in flight
  // across a first use when their number is branch-free, i.e. nine loads per lane and level whatever the level's width:
  // sweeps 45 -> 57 us fused, 33 -> 41 us plain -- the issue rate costs more than the latency hidden.)
  // entries of a level -> registers: one load for the lane's indices, one per coefficient slot.  Wavefronts
  // without a row of the level and slots past its width load nothing (the load unit's instruction rate is what
  // bounds a level once the latency is hidden: 16 unconditional loads per lane and level were 1.7 us per level).
  auto fetch = [&](const int4 h, SubRegs &R) {
    const int g = h.y & 0xff, npl = (h.y >> 8) & 0xf, nlane = (h.y >> 12) * g;
    if (nlane == 0) return;  // (wave-uniform: the header is the wavefront's own)
    const int lane = wl < nlane ? wl : nlane - 1;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    if (npl > 4) {
      const u32x4 q = factor_load(reinterpret_cast<const u32x4 *>(gi + h.w + lane * 8));
      R.i[0] = q.x, R.i[1] = q.y, R.i[2] = q.z, R.i[3] = q.w;
    } else {
      const u32x2 q = factor_load(reinterpret_cast<const u32x2 *>(gi + h.w + lane * 4));
      R.i[0] = q.x, R.i[1] = q.y;
    }
    const double *__restrict__ pv = gv + h.z + lane;
#pragma unroll
    for (int u = 0; u < kSubNpl; ++u)
      if (u < npl) R.v[u] = factor_load(pv + u * nlane);
    if constexpr (kDirect) R.row = grows[h.x + (lane >> (31 - __builtin_clz(g)))];  // (g: a power of two)
  };
  SubRegs RA, RB;
#pragma unroll
  for (int u = 0; u < kSubNpl; ++u) RA.v[u] = RB.v[u] = 0;
#pragma unroll
  for (int u = 0; u < kSubNpl / 2; ++u) RA.i[u] = RB.i[u] = 0;
  RA.row = RB.row = 0;
  // The first level's entries are requested before the prologue, so that they travel with the right-hand sides -- except
  // in the fused forward sweep (two value streams in flight): there the twenty registers of the set did not fit beside
  // the prologue's, the compiler WAITED for the entries in order to spill three of them (56 bytes of scratch per lane,
  // written and read back by 267 k lanes: 25 MB per launch in the counters) and only then issued the prologue's first
  // load.  The header is requested up front, the entries right behind the prologue's last load.
  constexpr bool kLateFetch = CORA_SUB_LATE_FETCH && FD == 1;
  // (a SCALAR load: the header is the wavefront's own, the plan's arrays are written by the host before any launch, and
  // held in vector registers across the prologue it was the next thing to be waited for and spilled)
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(4))) const v4i_t *const_v4i_ptr;
  const v4i_t h_first_v = *reinterpret_cast<const_v4i_ptr>(reinterpret_cast<uintptr_t>(gh + wv));  // before anything is ordered
  const int4 h_first = make_int4(h_first_v.x, h_first_v.y, h_first_v.z, h_first_v.w);
  auto fetch_first = [&] {
    fetch(make_int4(__builtin_amdgcn_readfirstlane(h_first.x), __builtin_amdgcn_readfirstlane(h_first.y),
                    __builtin_amdgcn_readfirstlane(h_first.z), __builtin_amdgcn_readfirstlane(h_first.w)), RA);
  };
  if (!kLateFetch) fetch_first();

  // element e of the block = column e % LD of its (e / LD)-th row in memory order.  Per pass a lane resolves kIoBatch
  // elements (all index loads in flight together; a block has <= 512 rows: ONE pass up to a row stride of 6) and moves
  // them in two halves (registers: the sweep must keep >= 5 workgroups per CU, or the 10^5-pose plan's 1 042 blocks
  // no longer run at once)
  const int2 *__restrict__ io = Q.io + rb;
  const int ne = nb * LD;
  // (fused forward, two value streams: one pass of 2 LD elements per lane up to a row stride of 5 -- 45 us at 10^5 poses against
  // 52 us in two passes of 6 --, two passes of LD above, where one pass spills)
  constexpr int kIoBatch = (FD == 1 && LD > 5) ? (LD <= 8 ? LD : 8) : (2 * LD <= 12 ? 2 * LD : 12);
  constexpr int kIoSub = (kIoBatch + 1) / 2;
  // offsets of a lane's kIoBatch elements in the vectors (g) and in the tile (t: below 2^16 -- 512 rows x 24 columns --, two
  // per register: the fused forward sweep at a row stride of 5 was five registers short of holding them unpacked)
  struct IoAt {
    int g[kIoBatch];
    uint32_t tp[(kIoBatch + 1) / 2];
    __device__ __forceinline__ int t(int u) const { return static_cast<int>((u & 1) ? tp[u >> 1] >> 16 : tp[u >> 1] & 0xffffu); }
    __device__ __forceinline__ void set_t(int u, int v) {
      if (u & 1) tp[u >> 1] |= static_cast<uint32_t>(v) << 16; else tp[u >> 1] = static_cast<uint32_t>(v);
    }
  };
  // (io_runs: the row of an element from the block's run table -- eight scalars of its descriptor --, so that the loads
  // of a phase do not wait for an index list; the tile position from a 16-bit list, requested at the same time)
  const uint16_t *__restrict__ tpos = Q.tpos + rb;
  const bool io_runs = S.io_runs != 0;
  auto io_index = [&](int e0, IoAt &at) {
#pragma unroll
    for (int u = 0; u < kIoBatch; ++u) {
      const int e = e0 + u * kSubThreads;
      const int ee = e < ne ? e : ne - 1;
      const int k = ee / LD, col = ee - k * LD;
      if (io_runs) {
        const int off = k < bd.run_end[0] ? bd.run_off[0] : (k < bd.run_end[1] ? bd.run_off[1] : (k < bd.run_end[2] ? bd.run_off[2] : bd.run_off[3]));
        at.g[u] = (k + off) * LD + col;
        at.set_t(u, static_cast<int>(tpos[k]) * LT + col);
      } else {
        const int2 rp = io[k];
        at.g[u] = rp.x * LD + col;
        at.set_t(u, rp.y * LT + col);
      }
    }
  };

  // ---- prologue: right-hand sides -> T (fused forward: r += coef_r Hp on the way, <r, r>); backward: behind them the
  // later stage's solution (it sits in `work`) at the rows coupled to the block, which the block's entries address as
  // rows nb + k
  {
    const int ntg = BWD ? bd.ntgt : 0;
    int tgt_row = -1;
    if (BWD && tid < ntg) tgt_row = S.tgt_row[bd.tgt_begin + tid];
    // (the trip count is block-uniform -- lanes past the block's elements re-read its last one and store nothing --:
    // the folded kappa below has barriers)
    for (int base = 0; base < ne; base += kIoBatch * kSubThreads) {
      const int e0 = base + tid;
      IoAt at;
      io_index(e0, at);
#pragma unroll
      for (int half = 0; half < kIoBatch; half += kIoSub) {
        double x[kIoSub], h[FD == 1 ? kIoSub : 1];
#pragma unroll
        for (int u = 0; u < kIoSub; ++u) {
          if (half + u >= kIoBatch) continue;
          x[u] = (FD == 1 ? F.r : src)[at.g[half + u]];
          if (FD == 1) h[FD == 1 ? u : 0] = F.Hp[at.g[half + u]];
        }
        if (FD == 1 && half == 0 && base == 0 && late_kappa) cr = folded_kappa();  // behind the first loads of the block
#pragma unroll
        for (int u = 0; u < kIoSub; ++u) {
          if (half + u >= kIoBatch) continue;
          const bool ok = e0 + (half + u) * kSubThreads < ne;
          if (FD == 1) {
            if (cr != 0.0) {
              x[u] = fma(cr, h[FD == 1 ? u : 0], x[u]);
              if (ok) F.r[at.g[half + u]] = x[u];
            }
            if (ok) dacc[0] = fma(x[u], x[u], dacc[0]);
          }
          if (ok) T[at.t(half + u)] = x[u];
        }
      }
    }
    if (kLateFetch) fetch_first();
    if (BWD) {
      for (int t = tid; t < ntg; t += kSubThreads) {
        if (t != tid) tgt_row = S.tgt_row[bd.tgt_begin + t];
        double x[LD];
        load_row<LD>(work + static_cast<size_t>(tgt_row) * LD, x);
#pragma unroll
        for (int j = 0; j < LD; ++j) T[(nb + t) * LT + j] = x[j];
      }
    }
  }
  __syncthreads();
  CORA_SUB_STAMP(1, wall_clock64());

  // ---- the triangular solve, level by level
  constexpr int CW = LD <= 6 ? LD : (LD % 6 == 0 ? 6 : (LD % 5 == 0 ? 5 : 4));  // accumulators per column chunk
#ifdef CORA_SUB_TIMES
  unsigned long long dbg_cyc[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned long long dbg_c = 0;
#define DBG_CYC(i) do { const unsigned long long c__ = __builtin_readcyclecounter(); dbg_cyc[i] += c__ - dbg_c; dbg_c = c__; } while (0)
#else
#define DBG_CYC(i) do { } while (0)
#endif
  auto level = [&](int l, const int4 h, const int4 hn, SubRegs &R, SubRegs &Rnext) {
#ifdef CORA_SUB_TIMES
    const unsigned long long dbg_w0 = wall_clock64();
    dbg_c = __builtin_readcyclecounter();
#endif
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the level's entries have arrived ...
#ifdef CORA_SUB_TIMES
    dbg_wait += wall_clock64() - dbg_w0;
#endif
    DBG_CYC(0);
    __builtin_amdgcn_sched_barrier(0);
    fetch(hn, Rnext);  // ... the next level's are on their way while this one is computed
    __builtin_amdgcn_sched_barrier(0);
    const int4 hnn = header(l + 2);
    DBG_CYC(1);
    const int r0 = h.x, g = h.y & 0xff, npl = (h.y >> 8) & 0xf;
    const int gs = 31 - __builtin_clz(g), nlane = (h.y >> 12) << gs;
    const bool active = nlane > 0;  // wavefront-uniform: the others go straight to the barriers
    double res[LD];
    if (active) {
      // One jump on the (wave-uniform) number of entries per lane and one on the lanes per row, then straight-line code:
      // with a branch per entry / per reduction step the tile reads of an entry were issued only after the previous
      // entry's, and the columns of a DPP sum one after the other.
#pragma unroll
      for (int c0 = 0; c0 < LD; c0 += CW) {
        double s[CW];
#pragma unroll
        for (int j = 0; j < CW; ++j) s[j] = 0.0;
        auto accumulate = [&](auto npl_c) {
          constexpr int NPL = decltype(npl_c)::value;
#pragma unroll
          for (int u = 0; u < NPL; ++u) {
            const uint32_t li = (u & 1) ? R.i[u >> 1] >> 16 : R.i[u >> 1] & 0xffffu;
            const double *__restrict__ t = static_cast<const double *>(__builtin_assume_aligned(smem + __umul24(li, LT * 8), LT % 2 == 0 ? 16 : 8)) + c0;
#pragma unroll
            for (int j = 0; j < CW; ++j)
              if (c0 + j < LD) s[j] = fma(static_cast<double>(R.v[u]), t[j], s[j]);
          }
        };
        switch (npl) {
          case 1: accumulate(std::integral_constant<int, 1>()); break;
          case 2: accumulate(std::integral_constant<int, 2>()); break;
          case 3: accumulate(std::integral_constant<int, 3>()); break;
          case 4: accumulate(std::integral_constant<int, 4>()); break;
          case 5: accumulate(std::integral_constant<int, 5>()); break;
          case 6: accumulate(std::integral_constant<int, 6>()); break;
          case 7: accumulate(std::integral_constant<int, 7>()); break;
          default: accumulate(std::integral_constant<int, 8>()); break;
        }
        DBG_CYC(2);
        group_sum_all<CW>(s, gs);
        DBG_CYC(3);
#pragma unroll
        for (int j = 0; j < CW; ++j)
          if (c0 + j < LD) res[c0 + j] = s[j];
      }
    }
    __syncthreads();  // every row of the level has read the tile ...
    DBG_CYC(4);
    if (active && wl < nlane && (wl & (g - 1)) == 0) {
      double *__restrict__ o = static_cast<double *>(__builtin_assume_aligned(smem + __mul24(r0 + (wl >> gs), LT * 8), LT % 2 == 0 ? 16 : 8));
#pragma unroll
      for (int j = 0; j < LD; ++j) o[j] = res[j];
      if constexpr (kDirect) {
        store_row<LD>(dst + static_cast<size_t>(R.row) * LD, res);
        if (FD == 1) dacc[1] += dot_row<LD>(res, res);
      }
    }
    DBG_CYC(5);
    __syncthreads();  // ... before any of them is written
    DBG_CYC(6);
    return hnn;
  };
  {
    int4 h0 = header(0), h1 = header(1);
    for (int l = 0; l < nlev; l += 2) {
      const int4 h2 = level(l, h0, h1, RA, RB);
      if (l + 1 >= nlev) break;
      const int4 h3 = level(l + 1, h1, h2, RB, RA);
      h0 = h2;
      h1 = h3;
    }
  }

  CORA_SUB_STAMP(2, wall_clock64());
  CORA_SUB_STAMP(4, dbg_wait);
  CORA_SUB_STAMP(5, static_cast<unsigned long long>(nlev));
#ifdef CORA_SUB_TIMES
  for (int q = 0; q < 7; ++q) CORA_SUB_STAMP(6 + q, dbg_cyc[q]);
#endif
#ifdef CORA_SUB_TIMES
  struct SubEnd {  // (the result paths return from several places)
    unsigned bwd;
    __device__ ~SubEnd() {
      if (threadIdx.x == 0 && blockIdx.x < kSubTimesMax) g_sub_phase[(bwd ? kSubPhases * kSubTimesMax : 0) + kSubPhases * blockIdx.x + 3] = wall_clock64();
    }
  } dbg_end{BWD ? 1u : 0u};
#endif
  // ---- results
  if (FD >= 2) {
    // v = Proj_Y(x) in the tile, a lane per row unit (a pose's rotation rows sit at consecutive positions) ...
    constexpr int D = FD >= 2 ? FD : 2;
    const int2 *__restrict__ un = S.b_unit + bd.unit_begin;
    for (int u = tid; u < bd.nunits; u += kSubThreads) {
      const int2 pr = un[u];  // {tile position, internal row}
      const size_t row = static_cast<size_t>(pr.y);
      double *__restrict__ tv = T + pr.x * LT;
      if (row < static_cast<size_t>(F.rng_base)) {
        double y[D][LD], v[D][LD];
#pragma unroll
        for (int a = 0; a < D; ++a) load_row<LD>(F.Y + (row + a) * LD, y[a]);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int j = 0; j < LD; ++j) v[a][j] = tv[a * LT + j];
        stiefel_project_thread<LD, D>(y, v);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int j = 0; j < LD; ++j) tv[a * LT + j] = v[a][j];
      } else if (row < static_cast<size_t>(F.trn_base)) {
        double y[LD], v[LD];
        load_row<LD>(F.Y + row * LD, y);
#pragma unroll
        for (int j = 0; j < LD; ++j) v[j] = tv[j];
        const double ip = dot_row<LD>(y, v);
#pragma unroll
        for (int j = 0; j < LD; ++j) tv[j] = fma(-ip, y[j], v[j]);
      }
    }
    __syncthreads();
  }
  // ... and the tile -> dst in memory order.  Fused backward: the tile holds v; nothing is stored but the updated step
  // and direction, s += coef_s p and p = coef_v v + coef_beta p, element by element in the same order.  Fused forward:
  // with |y|^2 of the block's rows (SubFuse::yy_partial).
  if (FD >= 2) {
    if (!upd) return;
    if (store_v) {
      for (int e0 = tid; e0 < ne; e0 += kIoBatch * kSubThreads) {
        IoAt at;
        io_index(e0, at);
#pragma unroll
        for (int u = 0; u < kIoBatch; ++u)
          if (e0 + u * kSubThreads < ne) dst[at.g[u]] = T[at.t(u)];
      }
      return;
    }
    for (int e0 = tid; e0 < ne; e0 += kIoBatch * kSubThreads) {
      IoAt at;
      io_index(e0, at);
#pragma unroll
      for (int half = 0; half < kIoBatch; half += kIoSub) {
        double pv[kIoSub], sv[kIoSub];
#pragma unroll
        for (int u = 0; u < kIoSub; ++u)
          if (half + u < kIoBatch) {
            pv[u] = F.p[at.g[half + u]];
            sv[u] = F.s[at.g[half + u]];
          }
#pragma unroll
        for (int u = 0; u < kIoSub; ++u)
          if (half + u < kIoBatch && e0 + (half + u) * kSubThreads < ne) {
            const double v = T[at.t(half + u)];
            F.s[at.g[half + u]] = fma(cs, pv[u], sv[u]);
            F.p[at.g[half + u]] = fma(cv, v, cb * pv[u]);
          }
      }
    }
    return;
  }
  if constexpr (!kDirect) {
    for (int e0 = tid; e0 < ne; e0 += kIoBatch * kSubThreads) {
      IoAt at;
      io_index(e0, at);
#pragma unroll
      for (int u = 0; u < kIoBatch; ++u)
        if (e0 + u * kSubThreads < ne) {
          const double v = T[at.t(u)];
          dst[at.g[u]] = v;
          if (FD == 1) dacc[1] = fma(v, v, dacc[1]);
        }
    }
  }
  if (FD == 1) {  // <r, r> and |y|^2 over the block's rows (RvTail adds the slots of all blocks in fixed order)
    const double rr = block_sum_256(dacc[0], dot_sm);
    const double yy = block_sum_256(dacc[1], dot_sm + 4);
    if (tid == 0) {
      F.rr_partial[b] = rr;
      F.yy_partial[b] = yy;
    }
  }
  if (!BWD) {  // couplings to the last stage: aux row of target g = -sum_v L_gv y_v, 16 lanes per target
    const int ntgt = bd.ntgt;
    for (int base = 0; base < (ntgt << 4); base += kSubThreads) {
      const int id = base + tid, tq = id >> 4, part = id & 15;
      const bool live = tq < ntgt;
      const int tg = bd.tgt_begin + (live ? tq : 0);
      const int c0 = S.c_ptr[tg] + part, c1 = live ? S.c_ptr[tg + 1] : 0;
      double sum[LD];
#pragma unroll
      for (int j = 0; j < LD; ++j) sum[j] = 0.0;
      for (int kb = c0; kb < c1; kb += 4 * 16) {
        int ci[4];
        double cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = kb + u * 16;
          const bool ok = k < c1;
          const int kk = ok ? k : kb;
          ci[u] = S.c_idx[kk];
          const double v = S.c_val[kk];
          cv[u] = ok ? v : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double *__restrict__ t = T + ci[u] * LT;
#pragma unroll
          for (int j = 0; j < LD; ++j) sum[j] = fma(cv[u], t[j], sum[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < LD; ++j) sum[j] = group_sum(sum[j], 16);
      if (live && part == 0) store_row<LD>(work + (static_cast<size_t>(S.aux_base) + S.tgt_slot[tg]) * LD, sum);
    }
  }
}

#if CORA_LDG & 1
// kappa = <p, Hp> from the partials of an EPI_HVP_K product (one block, fixed order), then the scalar step.
// (Measured and not kept, round 3: the same sum in the product's own last block behind a ticket -- one counter for the
// 4 016 blocks serialises 4 016 returning atomics on one address, 63 us; a two-level ticket, 64 blocks per counter, costs
// every wavefront a drain of its stores and an atomic round trip before it frees its slot: 29.8 us against 24.4 + 4.7.)
__global__ __launch_bounds__(256) void k_kappa_finish(const double *__restrict__ partial, int n, StpcgState *st) {
  __shared__ double sm[4];
  StpcgState L = {};
  if (threadIdx.x == 0) L = *st;  // in flight while the partials are added up
  const double t = kappa_sum_256(partial, n, sm);
  if (threadIdx.x == 0) {
    stpcg_after_kappa(L, t);
    *st = L;
  }
}

__global__ void k_zero_row(double *x, size_t row, int ld) {
  if (static_cast<int>(threadIdx.x) < ld) x[row * ld + threadIdx.x] = 0.0;
}
#endif  // CORA_LDG & 1

#endif  // CORA_TU & 4
