// Kernel argument blocks and launcher declarations (host-visible).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "cora_internal.h"
#include "trisolve.h"

namespace cora {

// EPI_HVP_K: EPI_HVP that also leaves per-block partial sums of <X, out> in SpmmArgs::kappa_partial (the curvature
// kappa = <p, Hp> of an STPCG iteration without a pass of its own)
enum Epilogue : int { EPI_NONE = 0, EPI_S = 1, EPI_HVP = 2, EPI_HVP_K = 3 };

struct StpcgState;
struct SpmmArgs {
  const SliceDesc *slices;
  int n_slices;
  int n_chunks;        // set by the caller: launch positions of the long rows' pieces (entries of chunk_order)
  int n_real_chunks;   // filled by launch_spmm
  int n_slice_blocks;  // filled by launch_spmm
  const double *sval;
  const double *head_val;  // [pose slice][kChainHead(d)]: what lane 0 of a chain slice takes from the pose before it
  const int32_t *scol;
  const int32_t *perm;
  const LongChunk *chunks;
  const int32_t *chunk_order;  // [n_chunks] piece at every launch position, -1: none (long_image.h)
  const double *lval;
  const int32_t *lcol;
  double *partials;    // [pieces][kMaxLD]
  unsigned *tickets;   // [n_long_rows], zero between launches
  const double *X;     // rows x LD
  double *out;         // rows x LD (only local rows are written)
  const double *Y;     // current point (epilogues)
  const double *lam_st;  // [local pose][d*d]
  const double *lam_ob;  // [local range]
  // [pose slice][kSymEl(d)][64]: S_P = sym(Q_PP) - Lambda_P (cora_internal.h, HostFormat::own_sym) -- what the chain
  // slices of EPI_S / EPI_HVP / EPI_HVP_K read for the pose's own block; plain slices keep own slots + lam_st
  const double *S = nullptr;
  // EPI_HVP_K: [launch_spmm_kappa_slots()] one partial sum of <X, out> per block, then one per long row (written by
  // whichever chunk finishes the row -- a fixed slot whatever the arrival order)
  double *kappa_partial = nullptr;
  // partitioned handles: [n_long_rows][ld] partial sums of the DISTRIBUTED long rows (zeroed before the launch, summed
  // over the ranks after it: capi.hip, finish_long_rows); nullptr: long rows are whole and written to `out`
  double *long_out = nullptr;
  int n_long_rows = 0;      // set by the caller (HostFormat::n_long_rows)
  int kappa_long_base = 0;  // filled by launch_spmm

  // internal row ranges [lo, hi) of the LOCAL rotation and translation rows of X: the pose slices clip their LDS
  // windows of X to them (kernels.hip, pose_slice); empty ranges switch the windows off, never the result
  int32_t win_rot_lo = 0, win_rot_hi = 0, win_trn_lo = 0, win_trn_hi = 0;
  // the same slices with the pose slices first inside each XCD's eighth of the list (HostFormat::slices_pose_first);
  // launch_spmm takes this order up to a row stride of kPoseFirstMaxLD (measured: better below, worse above)
  const SliceDesc *slices_pose_first = nullptr;
  int32_t n_local_poses = 0;  // poses of the shard (chain slices clamp their implied columns to them)
  int32_t win_on = 0;  // set by launch_spmm: X window + cooperative epilogue of the pose slices (n_slices >= kWinMinSlices)
  // set by launch_spmm (spmm_stagger_ticks_for): a pose slice in an odd wave slot of its SIMD -- the second of the two the
  // SIMD holds -- issues its first load this many ticks of the 100 MHz wall clock after it reaches the gate, so that its
  // loads travel while the first one computes (window form only).  0: nobody waits; negative (tests): every pose slice
  // waits that long.  Results do not depend on it.
  int32_t stagger_ticks = 0;
};
extern int g_win_min_slices;  // launch_spmm: window form from this many slices on (kernels.hip)
// The stagger of the pose slices (SpmmArgs::stagger_ticks; profiles/hvp_stagger.md).  The delay is CORA_SPMM_STAGGER_TICKS,
// at most kStaggerMaxTicks (20 us), and applies where it was measured to win: window-form launches with an epilogue, at
// a row stride of 5 (strides 3, 4, 6 and 8 lose or draw), with kStaggerMinPoseSlices (one per SIMD of the part: from
// there on SIMDs hold two of them) to kStaggerMaxPoseSlices pose slices (the wavefront slots of the part: one round --
// 2 10^5 poses and more lose at 300 ticks).  g_spmm_stagger_force (cora_debug_spmm_stagger_force) = 1 drops the
// conditions on size, stride and epilogue, = 2 also makes every pose slice wait (small launches leave the odd wave
// slots empty).
extern int g_spmm_stagger_ticks, g_spmm_stagger_force;
constexpr int kStaggerMaxTicks = 2000;
constexpr int kStaggerMinPoseSlices = 1024, kStaggerMaxPoseSlices = 2048;
constexpr int kStaggerMinLD = 5, kStaggerMaxLD = 5;
inline int spmm_stagger_clamp(int64_t ticks) { return static_cast<int>(std::min<int64_t>(std::max<int64_t>(ticks, 0), kStaggerMaxTicks)); }
inline int spmm_stagger_ticks_for(const SpmmArgs &A, int ld, int epi) {
  if (!A.win_on || g_spmm_stagger_ticks <= 0) return 0;
  const int pose_slices = (A.n_local_poses + kWave - 1) / kWave;
  const bool measured = epi != EPI_NONE && ld >= kStaggerMinLD && ld <= kStaggerMaxLD && pose_slices >= kStaggerMinPoseSlices &&
                        pose_slices <= kStaggerMaxPoseSlices;
  if (!measured && !g_spmm_stagger_force) return 0;
  return g_spmm_stagger_force == 2 ? -spmm_stagger_clamp(g_spmm_stagger_ticks) : spmm_stagger_clamp(g_spmm_stagger_ticks);
}
constexpr int kPoseFirstMaxLD = 6;
constexpr int kWinMinSlices = 2048;  // = the wavefronts resident at once (256 CUs x 8)
// number of blocks (= kappa partials) of a launch with these arguments
inline int launch_spmm_blocks(const SpmmArgs &A) { return ((A.n_chunks + 7) & ~7) + 8 * ((A.n_slices + 7) / 8); }
// number of kappa partials an EPI_HVP_K launch with these arguments writes (every slot, every launch)
inline int launch_spmm_kappa_slots(const SpmmArgs &A) { return launch_spmm_blocks(A) + A.n_long_rows; }

struct RowArgs {
  int d;
  int nl_poses, nl_ranges, nl_trans;
  size_t rot_base, rng_base, trn_base, base;
};

// Scalars of one Steihaug-Toint PCG solve, resident on the device so that an iteration needs no host
// round trip: the inner-product kernels update them in their last block, the vector kernels read their
// coefficients from here.  status: 0 running, 1 residual target met, 2 stopped on the trust-region
// boundary (or negative curvature), 3 iteration limit.  Once status != 0 all coefficients are neutral, so
// iterations the host has already enqueued do not change s, r or p.
struct StpcgState {
  double r_v, sigma_M2, s_Mp, p_M2;  // recurrences of the M-norms (Conn, Gould & Toint, Alg. 7.5.1)
  double Delta2, target;
  double alpha, coef_s, coef_r, coef_v, coef_beta;
  double kappa, rr, step_M_norm;
  int iters, status, max_iters, pad;
};
enum { DOTS_PLAIN = 0, DOTS_STPCG_KAPPA = 1, DOTS_STPCG_BETA = 2, DOTS_STPCG_RR = 3, DOTS_STPCG_RV = 4, DOTS_STPCG_KAPPA_RR = 5 };

struct DotArgs {
  const double *a[4];
  const double *b[4];
  int count;
  int64_t n2;        // number of doubles (launch_dots halves it for the double2 kernel)
  double *partial;   // [count][gridDim.x]
  unsigned *ticket;  // zero between launches; the last block to finish reduces the partials
  double *out;       // [count] results, written by that block (may be pinned host memory)
  unsigned long long *seq_out;  // optional (pinned): set to `seq` after the results are visible to the host
  unsigned long long seq;
  int mode;                     // DOTS_*: what the last block does with the results
  StpcgState *st, *st_host;     // device state and its pinned mirror (DOTS_STPCG_*)
  // non-null: the sequence number is ++(*seq_counter) (device memory) instead of `seq` -- launches replayed from a
  // hipGraph carry no per-launch argument; the host keeps the counter equal to its own count (capi.hip, stpcg_run)
  unsigned long long *seq_counter = nullptr;
};

struct RowOpDev {  // device copy of a RowOpHost (trisolve.h)
  const int32_t *out_row, *begin, *end;
  int n8, n64;
  const int32_t *long_out, *long_chunk_ptr, *chunk_begin, *chunk_end;
  int nlong, nchunks;
  const int32_t *col;
  const double *val;
  const int32_t *chunk_row;  // long-row ordinal of every chunk
  double *partial;     // [nchunks][kMaxLD]
  unsigned *tickets;   // [nlong], zero between launches
};
// Device copy of a BlockOpHost (trisolve.h), packed so that everything wave-uniform is one scalar load:
// a 16-byte descriptor per block and a 16-byte record per block row (its internal row for the lane that
// owns it; the lane mask and offset of column / row q of W for the wave's loop over q).
struct BlockDesc { int32_t row_begin, nrows, meta_begin, pad; int64_t w_off; int64_t pad2; };  // 32 bytes
struct BlockLane { uint64_t mask; int32_t off; int32_t row; };
struct BlockOpDev {
  const BlockDesc *desc;
  const BlockLane *by_col, *by_row;     // [desc.meta_begin + q]: column q of W (forward) / row q of W (backward)
  const double *w_by_col, *w_by_row;
  const int32_t *ext_ptr, *ext_col;
  const double *ext_val;
  int nblocks;
};
// Device copy of a SubBlockOpHost (trisolve.h): stage 0 as workgroup blocks solved by substitution in LDS.
struct SubDesc {  // 88 bytes per block
  int32_t row_begin, nrows;
  int32_t f_ent_begin, f_nent, b_ent_begin, b_nent;
  int32_t f_lev_begin, f_nlev, b_lev_begin, b_nlev;
  int32_t tgt_begin, ntgt;
  int32_t unit_begin, nunits;  // backward, fused projection: the block's row units in SubOpDev::b_unit
  // The block's rows in MEMORY order are a few runs of consecutive rows (a chain block: its poses' rotation rows, their
  // range rows, their translation rows): the k-th row in memory order is  k + run_off[r]  for the first r with
  // k < run_end[r] (unused runs end at INT32_MAX).  With SubOpDev::io_runs the sweeps form their global addresses from
  // these eight scalars -- the loads of a phase no longer wait for an index list -- and take the tile position of a row
  // from a 16-bit list (SubSweep::tpos).
  int32_t run_off[4], run_end[4];
};
constexpr int kSubMaxRuns = 4;
struct SubSweep {  // one direction of the solve; rows are numbered by level within the block
  const int32_t *rows;      // [row_begin + k]: internal row
  const int32_t *hdr;       // [4 * (lev_begin + l)]: {first row, lanes per row g | entries per lane npl << 8, first coefficient (block-relative), first index (absolute)} of level l
  const uint16_t *idx;      // local row a block entry multiplies: per level [lane = row * g + part][4 or 8]
  // val: per level [slot u < npl][lane]
  const double *val;        // coefficient
  // [row_begin + k]: {internal row, tile position} of the block's k-th row in MEMORY order: the tile is filled and
  // written back element by element in that order (a block is a few runs of consecutive rows: coalesced)
  const int2 *io;
  const uint16_t *tpos;  // [row_begin + k]: the tile position alone (SubOpDev::io_runs)
};
struct SubOpDev {
  const SubDesc *desc;
  SubSweep fwd, bwd;
  const int32_t *tgt_row;        // backward: rows of the last stage coupled to the block, staged behind the block's rows in the tile
  const int32_t *tgt_slot, *c_ptr;  // forward: aux rows written for the last stage
  const uint16_t *c_idx;
  const double *c_val;
  const int32_t *top_rows;  // rows of the last stage + the pinned row
  const int2 *b_unit;       // backward, fused projection: {tile position, internal row} of every row unit of a block (a pose's
                            // first rotation row -- the others follow it in the tile --, a range row, a translation row)
  int nblocks, ntop, max_rows, max_ent, max_lev, aux_base;
  int max_level_lanes, max_npl;  // widest level (rows x lanes per row) and most entries per lane of the plan
  int io_runs;  // 1: every block has at most kSubMaxRuns runs of consecutive rows (SubDesc::run_off / run_end are valid)
};
// STPCG passes fused into the two sweeps (cora_stpcg_dev; one shard, explicit formulation):
//   forward : the right-hand side IS the residual and is updated on the way in:  r += coef_r Hp; every row of the vector
//             is a block row or a row of the last stage; every block leaves <r, r> and |y|^2 over its rows in slots
//   backward: the solution is projected on the way out, v = Proj_Y(x), and the step and the direction are updated in the
//             same epilogue (s += coef_s p, p = coef_v v + coef_beta p); needs the d rotation rows of a pose at
//             consecutive tile positions (checked when the factor is installed)
// Between the sweeps, an extra block of the last stage's second product (RvTail) adds the slots and the squared norms of
// the rows of t_1 in fixed order and runs the scalar steps that follow <r, r> and <r, v>: no ticket, no atomics.
struct RvTail {
  const double *rr_partial;  // [n_rr]  <r, r> slots of the forward sweep (one per block of its launch)
  int n_rr;
  const double *yy_partial;  // [n_yy]  |y|^2 slots of the forward sweep's solve blocks
  int n_yy;
  const double *rowsq;       // [n_rowsq] squared norms of the rows of t_1, a slot per wavefront (the last stage's first product leaves them)
  int n_rowsq;
  StpcgState *st, *st_host;  // st == nullptr: no tail block in this launch ...
  double *rowsq_out;         // ... but, if set, the product leaves the squared norms of its rows in rowsq_out[rowop_rowsq_slots]
  unsigned long long *seq_out;  // pinned: set to seq after the mirror is visible to the host
  unsigned long long seq;
  unsigned long long *seq_counter;  // non-null: seq = ++(*seq_counter), see DotArgs
  // n_kappa > 0: the iteration's kappa step has not run yet (SubFuse::n_kappa): the block adds the partials and runs it
  // before the two steps of its own
  const double *kappa_partial;
  int n_kappa;
  // non-null (partitioned handle): the block leaves THIS RANK'S sums -- sums_out[0] = <r, r>, sums_out[1] = <r, v> -- and
  // touches neither the state nor the mirror: the sums are added over the ranks first (one all-reduce), then
  // k_stpcg_scalar_step runs the scalar step
  double *sums_out;
};
struct SubFuse {
  DotArgs dot;                 // only dot.st (the coefficients of the state) is used
  const double *Hp = nullptr;  // forward
  double *r = nullptr;         // forward: the right-hand side (updated in place)
  // forward: slot b of rr_partial receives <r, r> over the rows of block b of the launch (solve blocks, then the blocks
  // that carry the rows of the last stage); slot b of yy_partial |y|^2 over the rows of solve block b (y = L^-1 r).  With
  // |t_1|^2 of the last stage they make <r, v> = <r, Proj_Y(L^-T L^-1 r)> = |L^-1 r|^2 (r is a tangent vector and
  // Proj_Y is an orthogonal projector), so beta is known BEFORE the backward sweep (RvTail, k_rowop) and the direction
  // update rides on its epilogue.
  double *rr_partial = nullptr, *yy_partial = nullptr;
  const double *Y = nullptr;   // backward: the current point
  double *p = nullptr, *s = nullptr;  // backward: s += coef_s p, then p = coef_v v + coef_beta p  (v = Proj_Y(x), not stored)
  int d = 0;
  int64_t rot_base = 0, rng_base = 0, trn_base = 0;  // internal rows: rotations | ranges | translations
  // forward, n_kappa > 0: kappa = <p, Hp> has NOT been finished by a launch of its own -- every block adds the product's
  // n_kappa partial sums itself (same order, same bits: kappa_sum_256) and runs the scalar step on a private copy of the
  // state to get coef_r; the state itself is advanced later, by the tail block of the last stage (RvTail::n_kappa), which
  // adds the same partials the same way.  One launch per iteration less; worth it while blocks x partials is small.
  const double *kappa_partial = nullptr;
  int n_kappa = 0;
};
inline int launch_subblock_blocks(const SubOpDev &S) { return S.nblocks + (S.ntop + 255) / 256; }
hipError_t launch_subblock_fused(const SubOpDev &S, int ld, bool backward, const SubFuse &F, double *work, double *out,
                                 hipStream_t st);

// forward : y[block rows] = L_bb^-1 rhs[block rows] -> y;  work[aux rows] = couplings to the last stage;  work[top rows] = rhs[top rows]
// backward: x[block rows] = L_bb^-T (y[block rows] - L[top, rows]^T work[top rows]) -> x (may be y);  x[top rows] = work[top rows]
hipError_t launch_subblock(const SubOpDev &S, int ld, bool backward, const double *rhs_or_y, double *work, double *out,
                           hipStream_t st);

// forward: dst[rows] = W src[rows];  backward: dst[rows] = W^T (src[rows] - L[later, rows]^T src[later])
hipError_t launch_blockop(const BlockOpDev &B, int ld, bool backward, const double *src, double *dst, hipStream_t st);
// dst[out_row] = (src0 ? src0[out_row] : 0) + sum_k val_k * src[col_k] for every row of the product
// kappa = sum of the n partials of an EPI_HVP_K product (fixed order), then the scalar step that follows it
hipError_t launch_kappa_finish(const double *partial, int n, StpcgState *state, hipStream_t st);
// tail: optional RvTail (see SubFuse) -- per-row squared norms out, or one extra block that runs the reductions
// slots a product leaves its rows' squared norms in (RvTail::rowsq_out): one per wavefront of the 8-lane class, one per row of the other two
#ifdef CORA_ROWSQ_PER_ROW  // (lab: a slot per row, the form before)
inline int rowop_rowsq_slots(const RowOpDev &op) { return op.n8 + op.n64 + op.nlong; }
#else
inline int rowop_rowsq_slots(const RowOpDev &op) { return 4 * ((op.n8 + 31) >> 5) + op.n64 + op.nlong; }
#endif
hipError_t launch_rowop(const RowOpDev &op, int ld, const double *src0, const double *src, double *dst,
                        hipStream_t st, const RvTail *tail = nullptr);
hipError_t launch_gram(int64_t row0, int64_t rows, const double *A, int ka, const double *B, int kb,
                       double *partial, int nblocks, double *out, hipStream_t st);
hipError_t launch_fill_random(int64_t N, int k, unsigned long long seed, const int32_t *api2int, double *x, hipStream_t st);
hipError_t launch_gram_batch(int64_t row0, int64_t rows, int n, const double *const *A, const int *ka, const double *const *B,
                             const int *kb, double *partial, int nblocks, double *out, hipStream_t st);
constexpr int kCombineKargMax = 400;  // coefficients that travel in the kernel's arguments (CombineCoef::kMax)
hipError_t launch_combine(int64_t row0, int64_t rows, int nblocks, const double *const *x, const int *kx,
                          const int *coff, const double *coef, int ncoef, int kout, double *out, hipStream_t st,
                          const double *coef_host = nullptr);
hipError_t launch_zero_row(double *x, size_t row, int ld, hipStream_t st);

hipError_t launch_spmm(const SpmmArgs &A, int ld, int d, int epi, hipStream_t st);
hipError_t launch_point_finish(const RowArgs &R, int ld, const double *Y, const double *G,
                               double *rgrad, double *lam_st, double *lam_ob, const double *own_sym, double *S,
                               double *partial, int *nblocks, hipStream_t st);
hipError_t launch_tangent_project(const RowArgs &R, int ld, const double *Y, const double *V,
                                  const double *scale, double *out, hipStream_t st);
hipError_t launch_project_manifold(const RowArgs &R, int ld, const double *A, const double *V,
                                   double alpha, double *out, hipStream_t st);
hipError_t launch_axpby(int64_t n, double a, const double *x, double b, double *y, hipStream_t st);
hipError_t launch_axpy2(int64_t n, double a1, const double *x1, double *y1, double a2, const double *x2,
                        double *y2, hipStream_t st);
// s += coef_s p, r += coef_r Hp  /  p = coef_v v + coef_beta p  with the coefficients of the device state
hipError_t launch_stpcg_update(int64_t n, const StpcgState *S, const double *p, const double *Hp, double *s,
                               double *r, hipStream_t st);
hipError_t launch_stpcg_direction(int64_t n, const StpcgState *S, const double *v, double *p, hipStream_t st);
// the fused passes of the device-resident STPCG iteration (cora_stpcg_dev):
//   r += coef_r Hp with <r, r> (DOTS_STPCG_RR)  |  out = Proj_Y(V) with <r, out> (DOTS_STPCG_RV)  |
//   s += coef_s p, then p = coef_v v + coef_beta p
hipError_t launch_stpcg_residual(const DotArgs &D, int64_t n, const double *Hp, double *r, hipStream_t st);
// v = Proj_Y(X) consumed at once by  s += coef_s p, p = coef_v v + coef_beta p  (row strides up to 12)
hipError_t launch_tangent_project_update(const RowArgs &R, const StpcgState *S, int ld, const double *Y, const double *X,
                                         double *p, double *s, hipStream_t st);
// kappa from the nk partials of an EPI_HVP_K product, the scalar step, then r += coef_r Hp with <r, r> -- ONE launch:
// every block adds the partials itself (same order, same bits).  For the small plans, where a launch is what costs.
hipError_t launch_kappa_residual(const DotArgs &D, const double *kpartial, int nk, int64_t n, const double *Hp, double *r,
                                 hipStream_t st);
// The same pass without the scalar step: a block leaves its share of <r, r> in rr_slot[block] (kappa_residual_slots_blocks(n)
// slots) and the state is advanced by the tail block of a later launch (RvTail::n_kappa, RvTail::n_rr) -- no ticket here.
int kappa_residual_slots_blocks(int64_t n);
hipError_t launch_kappa_residual_slots(const StpcgState *S, const double *kpartial, int nk, int64_t n, const double *Hp, double *r,
                                       double *rr_slot, hipStream_t st);
hipError_t launch_tangent_project_dot(const RowArgs &R, const DotArgs &D, int ld, const double *Y, const double *V,
                                      const double *scale, const double *r, double *out, hipStream_t st);
// the scalar step of a partitioned handle's iteration, after the all-reduce of its inner products (k_stpcg_scalar_step)
hipError_t launch_stpcg_scalar_step(int what, const double *vals, StpcgState *state, StpcgState *state_host,
                                    unsigned long long *seq_out, unsigned long long seq, hipStream_t st);
// s = 0, r = g, p = -Pg (start of a solve whose preconditioned gradient is known)
hipError_t launch_stpcg_init(int64_t n, const double *g, const double *Pg, double *s, double *r, double *p, hipStream_t st);
hipError_t launch_stpcg_step_direction(int64_t n, const StpcgState *S, const double *v, double *p, double *s,
                                       hipStream_t st);
hipError_t launch_scale_rows(int64_t rows, int ld, const double *scale, const double *x, double *y,
                             hipStream_t st);
hipError_t launch_dots(const DotArgs &D, int *nblocks, hipStream_t st);
hipError_t launch_reduce_partials(const double *partial, int nblocks, int count, double *out,
                                  hipStream_t st);
// distributed long rows after the sum over the ranks: owner copies slot j -> out[rows[j]]; kappa != nullptr: kappa[j] = the
// row's share of <X, out> (0 on the other ranks)
hipError_t launch_long_finish(int n_long, int ld, int rank, const int32_t *rows, const int32_t *owner, const double *slots,
                              const double *X, double *out, double *kappa, hipStream_t st);
// the two ends of a partitioned product's exchange (kernels.hip, k_exchange_pack / k_exchange_unpack)
hipError_t launch_scatter_shard_rows(int world, int rank, int64_t maxn, int ld, int64_t shard_rows, const int64_t *meta,
                                     const double *recv, double *X, hipStream_t st);
hipError_t launch_exchange_pack(int64_t n, int ld, const int32_t *rows, int64_t ztail, const double *src, double *dst, hipStream_t st);
hipError_t launch_exchange_unpack(int world, int64_t e_max, int n_long, int ld, const int32_t *recv_idx, const double *recv, double *X,
                                  int rank, const int32_t *long_rows, const int32_t *long_owner, double *out, double *kappa,
                                  hipStream_t st);
hipError_t launch_has_nan(int64_t n, const double *x, int *flag, hipStream_t st);
// mode 0: dst[k] = src[rows[k]];  1: dst[rows[k]] = src[k];  2: dst[rows[k]] = src[rows[k]]  (rows of ld doubles)
hipError_t launch_move_rows(int mode, int64_t n, int ld, const int32_t *rows, const double *src, double *dst,
                            hipStream_t st);
hipError_t launch_upload(int64_t N, int k, int ld, const double *src, const int32_t *api2int,
                         double *dst, hipStream_t st);
hipError_t launch_download(int64_t N, int k, int ld, const double *src, const int32_t *api2int,
                           double *dst, hipStream_t st);

// Per-measurement residuals (kernels/residuals.inc; include/cora_hip.h, cora_set_measurements).  The table is
// structure-of-arrays, [field][measurement], rows are INTERNAL rows of X:
//   edges : rows [4][n] = first rotation row of a, of b (-1: no rotation part), translation row of a, of b
//           data [d*d + d + 2][n] = R row-major, t, kappa, tau;  out0 = rotation, out1 = translation residual
//   ranges: rows [3][n] = range row, translation row of a, of b;  data [2][n] = r, omega;  out0 = residual
// partial: [2][blocks] (edges) / [1][blocks] (ranges) block sums of the outputs, a fixed slot per block
// (launch_reduce_partials adds them up).  k = columns of X read (ld >= k; the padding column of k = 1 is not trusted).
struct ResidualArgs {
  int64_t n = 0;
  int d = 0, ld = 0, k = 0;
  const int32_t *rows = nullptr;
  const double *data = nullptr;
  const double *X = nullptr;
  double *out0 = nullptr, *out1 = nullptr;
  double *partial = nullptr;
};
constexpr int kResidualLanes = 8;  // lanes that share one measurement (they stride over the columns of X)
inline int residual_blocks(int64_t n) {  // blocks of a launch over n measurements (= partial sums per output)
  const int64_t per_block = 256 / kResidualLanes;
  return static_cast<int>(std::min<int64_t>((n + per_block - 1) / per_block, 2048));
}
hipError_t launch_edge_residuals(const ResidualArgs &A, hipStream_t st);   // n == 0: no launch
hipError_t launch_range_residuals(const ResidualArgs &A, hipStream_t st);  // n == 0: no launch

// The weight step of a robust-cost (GNC) loop (kernels/gnc.inc; include/cora_hip.h, cora_gnc_weights_dev).  One launch per
// kind of measurement: R is the table of that kind as the residual kernels take it (out0, out1 and partial unused),
//   edges : base = [kappa | tau], barc2, w, r2 = [rot | trans], each 2 n doubles;  partial [8][blocks]
//   ranges: base = omega,         barc2, w, r2 = n doubles;                          partial [4][blocks]
// partial: per segment (edges: rot, trans) three sums -- sum of w r^2, count of 0 < w < 1, count of w < 0.5 -- then one
// row of maxima of rho per segment.  r2 may be nullptr.  flag |= 1: an r^2 that is not finite, |= 2: a threshold that
// is NaN or <= 0.
constexpr int kGncNone = 0, kGncTls = 1, kGncGm = 2;
struct GncArgs {
  ResidualArgs R;
  const double *base = nullptr, *barc2 = nullptr;
  double *w = nullptr, *r2 = nullptr, *partial = nullptr;
  int *flag = nullptr;
  int cost = kGncNone, couple = 0;
  double mu = 1.0;
};
// The arithmetic of one slot, shared by the kernels and the host mirror (cora_debug_gnc_weights_host): every operation
// is a single correctly rounded fp64 one, in this order, never contracted.
// rho = r2 / barc2 (0 for a trusted slot: barc2 = +inf);  bad |= 1: r2 not finite, |= 2: barc2 NaN or <= 0
__host__ __device__ inline double gnc_ratio(double r2, double barc2, int &bad) {
  if (!(fabs(r2) <= 1.79769313486231570815e308)) bad |= 1;
  if (!(barc2 > 0.0)) bad |= 2;
  return barc2 > 1.79769313486231570815e308 ? 0.0 : r2 / barc2;
}
// a coupled edge is one measurement: one addition, rot first
__host__ __device__ inline double gnc_coupled_r2(double rot, double trn) {
#pragma clang fp contract(off)
  return rot + trn;
}
// TLS: 1 up to rho = mu / (mu + 1), 0 from (mu + 1) / mu on, sqrt(mu (mu + 1) / rho) - mu between;  GM: (mu / (rho + mu))^2.
// The middle band of TLS lies in (0, 1); rounding can leave it an ulp outside, so it is clamped (a weight below zero
// would be refused by the assembly).
__host__ __device__ inline double gnc_weight(int cost, double mu, double rho) {
#pragma clang fp contract(off)
  if (cost == kGncTls) {
    const double m1 = mu + 1.0;
    if (rho <= mu / m1) return 1.0;
    if (rho >= m1 / mu) return 0.0;
    const double q = mu * m1 / rho;
    const double w = sqrt(q) - mu;
    return w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w);
  }
  if (cost == kGncGm) {
    const double t = mu / (rho + mu);
    return t * t;
  }
  return 1.0;
}
hipError_t launch_gnc_edges(const GncArgs &A, hipStream_t st);   // n == 0: no launch
hipError_t launch_gnc_ranges(const GncArgs &A, hipStream_t st);  // n == 0: no launch
// out[j] = max over b of partial[j * nblocks + b] (values >= 0), one block, fixed order
hipError_t launch_reduce_max_partials(const double *partial, int nblocks, int count, double *out, hipStream_t st);

// Comparison of a resident estimate X (k columns) with a resident reference Ref (kr <= k columns) after an orthogonal
// alignment on the selected poses' positions (kernels/compare.inc; include/cora_hip.h, cora_compare_dev).  An entity
// -- pose i < n, landmark n <= i < nt, range row -- belongs to a group of kResidualLanes lanes; the pose table holds
// INTERNAL rows: rot_row[n] (first rotation row; the d rows are consecutive), trn_row[nt] (poses, then landmarks),
// rng_row[nr].  sel: nt bytes, API order.  Three steps:
//   sums   : partial[k + kr][blocks] = column sums of X | Ref over the selected poses' translation rows
//   centre : Xc, Gc (zeroed by the caller) get x_i - mean, g_i - mean in the selected poses' translation rows; the caller
//            forms H = Xc^T Gc with launch_gram: the other rows add exact zeros.  mean_c = sums[c] / m, formed by every
//            lane that needs it (one division, the same bits everywhere)
//   errors : et, er [n], el [nt - n] (0.0 where not selected), aligned (may be nullptr: all rows, kr columns),
//            partial[6][blocks] = sum et^2, sum er^2, sum el^2 | max et, max er, max el.  A: [k][kr] row-major.
//            flag |= 1 where an error is not finite.
// Every grid is sized by the count (32 entities per block, no grid-stride loop).
struct CompareArgs {
  int d = 0, n = 0, nt = 0, nr = 0;
  int k = 0, ldx = 0, kr = 0, ldr = 0;
  const double *X = nullptr, *Ref = nullptr;
  const int32_t *rot_row = nullptr, *trn_row = nullptr, *rng_row = nullptr;
  const unsigned char *sel = nullptr;
  double m = 0.0;               // number of selected poses
  const double *sums = nullptr; // [k + kr]
  const double *A = nullptr;
  double *Xc = nullptr, *Gc = nullptr;
  double *et = nullptr, *er = nullptr, *el = nullptr, *aligned = nullptr;
  double *partial = nullptr;
  int *flag = nullptr;
};
inline int compare_blocks(int64_t entities) { return static_cast<int>((entities + 256 / kResidualLanes - 1) / (256 / kResidualLanes)); }
hipError_t launch_compare_sums(const CompareArgs &A, hipStream_t st);    // compare_blocks(n) blocks
hipError_t launch_compare_centre(const CompareArgs &A, hipStream_t st);  // compare_blocks(n) blocks
hipError_t launch_compare_errors(const CompareArgs &A, hipStream_t st);  // compare_blocks(nt + (aligned ? nr : 0)) blocks

// Relative pose error of a resident estimate X (k columns) against a resident reference Ref (kr columns, independent of
// k) over m pairs of poses (kernels/rpe.inc; include/cora_hip.h, cora_rpe_dev).  rows: [4][m] INTERNAL rows -- first
// rotation row of i | translation row of i | first rotation row of j | translation row of j (a pose's d rotation rows
// are consecutive).  et, er: m doubles each.  partial[5][rpe_blocks(m)]: sum et^2, sum er^2 | max et, max er | m - (first
// pair of the block that attains the block's max et).  flag |= 1 where an error is not finite.
struct RpeArgs {
  int64_t m = 0;
  int d = 0, k = 0, ldx = 0, kr = 0, ldr = 0;
  const double *X = nullptr, *Ref = nullptr;
  const int32_t *rows = nullptr;
  double *et = nullptr, *er = nullptr;
  double *partial = nullptr;
  int *flag = nullptr;
};
constexpr int64_t kRpeMaxPairs = static_cast<int64_t>(1) << 30;  // (32 pairs per block: the grid stays far below 2^31)
inline int rpe_blocks(int64_t m) { return compare_blocks(m); }
hipError_t launch_rpe(const RpeArgs &A, hipStream_t st);  // rpe_blocks(m) blocks; m == 0: invalid
// stats[5] = sum et^2, sum er^2, max et, max er, first pair that attains max et, from the partials of launch_rpe
hipError_t launch_rpe_finish(const double *partial, int nblocks, int64_t m, double *stats, hipStream_t st);

// Scale guard of the normalisations of rows.inc and of the rounding below.  The polar factor of a block and the direction
// of a row do not change when the input is multiplied by a positive number, but their formulas square the entries:
// sqrt(alpha * beta) is a product of two squared row norms (0 below |A| ~ 1e-77, inf above 1e77) and dot_row(a, a) leaves
// the range at 1e+-154.  Returns the exponent e for which ldexp(x, e) -- exact -- brings a block whose largest |entry| is
// amax to [1/2, 1), and 0 (leave the block alone: the arithmetic of an ordinary block is untouched) when amax already
// lies in [2^-250, 2^250], where a product of two squared norms of <= 24 entries stays finite, or is 0, inf or NaN.
__host__ __device__ inline int rescale_exponent(double amax) {
  if ((amax >= 0x1p-250 && amax <= 0x1p250) || !(amax > 0.0) || !(amax < HUGE_VAL)) return 0;
  int e;
  (void)frexp(amax, &e);
  return -e;
}

// Rounding of a resident vector Y (k columns, d <= k <= 24) to SE(d): out = d columns at stride ld_for(d)
// (kernels/round.inc; include/cora_hip.h, cora_round_dev).  One thread per unit of RowArgs (pose block, range row,
// translation row).  vd: the basis, column-major k x d, for the translation rows; vd_dir: the same basis times the power
// of two that brings an extreme-scale Y into range (equal to vd otherwise), for the pose blocks and the range rows, whose
// results do not depend on a positive scale.  Three launches without a host step between them:
//   count  : partial[round_count_blocks] = number of pose blocks of the block with det(Y_i Vd) > 0 (fixed slots)
//   finish : words[0] = their sum, words[1] = 1 when the sum < n / 2 (integer division): the last column is negated
//   apply  : every unit's rows of out; reads words[1]; flag |= 1 where a product is not finite
struct RoundArgs {
  RowArgs R;
  int k = 0, ldy = 0;
  const double *Y = nullptr;
  double *out = nullptr;
  int *partial = nullptr, *words = nullptr, *flag = nullptr;
  double vd[kMaxLD * 3], vd_dir[kMaxLD * 3];
};
constexpr int kRoundCountBlock = 64;  // poses per block of the count pass: one wavefront, its partial is a ballot
inline int round_count_blocks(int64_t poses) { return static_cast<int>((poses + kRoundCountBlock - 1) / kRoundCountBlock); }
hipError_t launch_round_count(const RoundArgs &A, hipStream_t st);  // + the finish; no poses: words = {0, 0}
hipError_t launch_round_apply(const RoundArgs &A, hipStream_t st);
// the rare path of an input whose Gram matrix leaves the range: partial[blocks] = max |y| (finish: launch_reduce_max_partials),
// flag |= 1 where an entry is not finite;  out = ldexp(y, e)
hipError_t launch_round_amax(int64_t n, const double *y, double *partial, int nblocks, int *flag, hipStream_t st);
hipError_t launch_round_scale(int64_t n, const double *y, int e, double *out, hipStream_t st);

// The arithmetic of one unit (round_pose, round_row and their parts), shared by the kernels and the host mirror
// (cora_debug_round_host): every operation is a
// single correctly rounded fp64 one in the order written, never contracted; a fused one is an explicit fma.
// m[b] = sum over a = 0 .. k - 1 of row[a] vd[b k + a], one fma per term from +0.0, b < D
template <int D>
__host__ __device__ inline void round_product(const double *row, int k, const double *vd, double *m) {
#pragma clang fp contract(off)
#pragma unroll
  for (int b = 0; b < D; ++b) m[b] = 0.0;
  for (int a = 0; a < k; ++a) {
    const double y = row[a];
#pragma unroll
    for (int b = 0; b < D; ++b) m[b] = fma(y, vd[b * k + a], m[b]);
  }
}
// ldexp by rescale_exponent of the largest |entry| (exact; nothing for an ordinary block)
template <int N>
__host__ __device__ inline void round_rescale(double *m) {
  double amax = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) amax = fmax(amax, fabs(m[i]));
  const int e = rescale_exponent(amax);
  if (e != 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = ldexp(m[i], e);
  }
}
template <int D>
__host__ __device__ inline double round_det(const double (&m)[D][D]) {
#pragma clang fp contract(off)
  if constexpr (D == 2) {
    return fma(m[0][0], m[1][1], -(m[0][1] * m[1][0]));
  } else {
    const double c0 = fma(m[1][1], m[2][2], -(m[1][2] * m[2][1]));
    const double c1 = fma(m[1][2], m[2][0], -(m[1][0] * m[2][2]));
    const double c2 = fma(m[1][0], m[2][1], -(m[1][1] * m[2][0]));
    return fma(m[0][0], c0, fma(m[0][1], c1, m[0][2] * c2));
  }
}
// whether det(M) > 0, on the rescaled block (the sign does not depend on a positive scale; the determinant of an
// extreme-scale block would leave the range)
template <int D>
__host__ __device__ inline bool round_det_positive(double (&m)[D][D]) {
  round_rescale<D * D>(&m[0][0]);
  return round_det<D>(m) > 0.0;
}
template <int D>
__host__ __device__ inline void round_cross(const double *a, const double *b, double *c) {
#pragma clang fp contract(off)
  static_assert(D == 3, "cross products complete frames at d = 3");
  c[0] = fma(a[1], b[2], -(a[2] * b[1]));
  c[1] = fma(a[2], b[0], -(a[0] * b[2]));
  c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}
// The rotation R in SO(D) that maximises tr(R^T M), in place; M finite.  One-sided (Hestenes) Jacobi on the rows as in
// polar_rows (rows.inc): rotations J, a product of proper rotations, leave J M = diag(n) Q with orthogonal rows n_i q_i;
// polar(M) = J^T Q and det(polar) = det(Q).  With all rows there and det(Q) < 0 the row of smallest norm is negated: the
// correction sits on the smallest singular value.  A row whose squared norm is below 2^-960 after the rescaling -- below
// 2^-355 of the largest entry at the least, where eps times the condition number is beyond every bound -- counts as
// missing, takes part in no rotation and is completed: the perpendicular at D = 2, cross products at D = 3 (one row left:
// the frame built from the axis it is furthest from), so that det = +1; no row left: J is the identity, and so is R.
template <int D>
__host__ __device__ inline void round_rotation(double (&a)[D][D]) {
#pragma clang fp contract(off)
  constexpr double kTiny = 0x1p-960;
  round_rescale<D * D>(&a[0][0]);
  double J[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) J[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          alpha = fma(a[p][c], a[p][c], alpha);
          beta = fma(a[q][c], a[q][c], beta);
          gamma = fma(a[p][c], a[q][c], gamma);
        }
        if (gamma != 0.0 && alpha >= kTiny && beta >= kTiny) {
          const double denom = sqrt(alpha * beta);
          off = fmax(off, fabs(gamma) / denom);
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
          const double cs = 1.0 / sqrt(fma(t, t, 1.0)), sn = cs * t;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const double x = a[p][c], y = a[q][c];
            a[p][c] = fma(cs, x, -(sn * y));
            a[q][c] = fma(sn, x, cs * y);
          }
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const double x = J[p][c], y = J[q][c];
            J[p][c] = fma(cs, x, -(sn * y));
            J[q][c] = fma(sn, x, cs * y);
          }
        }
      }
    if (off < 1e-15) break;
  }
  double nrm2[D];
  double least = 0.0;
  int present = 0, smallest = 0;  // (the first of equal norms)
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) s = fma(a[i][c], a[i][c], s);
    nrm2[i] = s;
    if (i == 0 || s < least) {
      least = s;
      smallest = i;
    }
    if (s >= kTiny) {
      ++present;
      const double nrm = sqrt(s);
#pragma unroll
      for (int c = 0; c < D; ++c) a[i][c] = a[i][c] / nrm;
    } else {
#pragma unroll
      for (int c = 0; c < D; ++c) a[i][c] = 0.0;
    }
  }
  if (present == D) {
    if (round_det<D>(a) < 0.0) {
#pragma unroll
      for (int i = 0; i < D; ++i)
        if (i == smallest) {
#pragma unroll
          for (int c = 0; c < D; ++c) a[i][c] = -a[i][c];
        }
    }
  } else if (present == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) a[i][i] = 1.0;
  } else if constexpr (D == 2) {
    if (nrm2[0] >= kTiny) {  // det [x y; -y x] = 1
      a[1][0] = -a[0][1];
      a[1][1] = a[0][0];
    } else {
      a[0][0] = a[1][1];
      a[0][1] = -a[1][0];
    }
  } else {
    if (present == 1) {
      // the row that is there, u, at place p; the axis e it is furthest from; v = (u x e) / |u x e|, then w = u x v:
      // (u, v, w) at the places (p, p + 1, p + 2) mod 3, an even permutation
      const int p = nrm2[0] >= kTiny ? 0 : (nrm2[1] >= kTiny ? 1 : 2);
      double u[3], e[3] = {0.0, 0.0, 0.0}, v[3], w[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i == p) {
#pragma unroll
          for (int c = 0; c < 3; ++c) u[c] = a[i][c];
        }
      const int ax = (fabs(u[0]) <= fabs(u[1]) && fabs(u[0]) <= fabs(u[2])) ? 0 : (fabs(u[1]) <= fabs(u[2]) ? 1 : 2);
#pragma unroll
      for (int c = 0; c < 3; ++c) e[c] = c == ax ? 1.0 : 0.0;
      round_cross<3>(u, e, v);
      const double nv = sqrt(fma(v[0], v[0], fma(v[1], v[1], v[2] * v[2])));
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = v[c] / nv;
      round_cross<3>(u, v, w);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (i == (p + 1) % 3) a[i][c] = v[c];
          if (i == (p + 2) % 3) a[i][c] = w[c];
        }
    } else {
      // two rows there: the third is the cross product of the other two in cyclic order (det = +1), normalised (the two
      // are orthogonal to working precision only)
      const int z = nrm2[0] < kTiny ? 0 : (nrm2[1] < kTiny ? 1 : 2);
      double x[3], y[3], w[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (i == (z + 1) % 3) x[c] = a[i][c];
          if (i == (z + 2) % 3) y[c] = a[i][c];
        }
      round_cross<3>(x, y, w);
      const double nw = sqrt(fma(w[0], w[0], fma(w[1], w[1], w[2] * w[2])));
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i == z) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a[i][c] = w[c] / nw;
        }
    }
  }
  double o[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < D; ++j) s = fma(J[j][i], a[j][c], s);
      o[i][c] = s;
    }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int c = 0; c < D; ++c) a[i][c] = o[i][c];
}
// a range row: the direction of m (D entries), a zero row stays zero
template <int D>
__host__ __device__ inline void round_direction(double *m) {
#pragma clang fp contract(off)
  round_rescale<D>(m);
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) s = fma(m[c], m[c], s);
  const double nrm = sqrt(s);
  if (nrm > 0.0) {
#pragma unroll
    for (int c = 0; c < D; ++c) m[c] = m[c] / nrm;
  }
}
// One unit.  round_pose: the D rows of a pose block (row, row + ldy, ..) through vd_dir, the flip, then round_rotation;
// round_row: a range row (through vd_dir, then its direction) or a translation row (through vd).  Both return whether every
// product was finite; a unit that is not keeps its products.
template <int D>
__host__ __device__ inline bool round_pose(const double *row, int ldy, int k, const double *vd_dir, bool flip, double (&m)[D][D]) {
  bool finite = true;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    round_product<D>(row + static_cast<size_t>(i) * ldy, k, vd_dir, m[i]);
    if (flip) m[i][D - 1] = -m[i][D - 1];
#pragma unroll
    for (int c = 0; c < D; ++c) finite = finite && fabs(m[i][c]) <= 1.79769313486231570815e308;
  }
  if (finite) round_rotation<D>(m);
  return finite;
}
template <int D>
__host__ __device__ inline bool round_row(bool range, const double *row, int k, const double *vd, bool flip, double (&m)[D]) {
  bool finite = true;
  round_product<D>(row, k, vd, m);
  if (flip) m[D - 1] = -m[D - 1];
#pragma unroll
  for (int c = 0; c < D; ++c) finite = finite && fabs(m[c]) <= 1.79769313486231570815e308;
  if (range && finite) round_direction<D>(m);
  return finite;
}

// Odometry initialisation: a segmented inclusive scan of SE(d) over the chain positions (kernels/odom.inc;
// include/cora_hip.h, cora_odometry_init_dev).  Chain c contributes its head and then its edges as consecutive positions;
// the element at a head is (flag = 1, I, start of the chain), at an edge (0, R_e, t_e) from the measurement table's
// edge_data ([field][measurement]); a right operand whose flag is set wins.  Three launches, no workgroup waits for another:
//   totals : totals[tile] = the product of the tile's kOdomTile positions           (one workgroup of kOdomTile threads per tile)
//   middle : carry[tile] = totals[0] o .. o totals[tile], kOdomSweep tiles per sweep (ONE wavefront; the last lane's value
//            is carried into the next sweep)
//   scan   : every position's product, with carry[tile - 1] from the left; the rows of the pose the position writes
// Elements travel as kOdomFields(d) doubles, structure-of-arrays [field][tile]: the flag (0.0 / 1.0), R row-major, t.
// BRACKET ORDER, a function of (P, kOdomTile, kOdomSweep) alone and the same in the host mirror (capi/odom.inc):
//   wavefront: Kogge-Stone, offsets 1, 2, .., 32 -- lane l >= off takes (lane l - off) o (lane l), all lanes at once;
//   tile: wave w > 0 folds the totals of waves 0 .. w - 1 from the left, (..(W_0 o W_1) o ..) o W_{w-1}, then that o (lane);
//   sweeps of the middle pass and the carry into a tile: (what came before) o (the wavefront's / the tile's result).
// Positions past P are heads of nothing (flag = 1, I, 0) and write nothing.
constexpr int kOdomTile = 256;
constexpr int kOdomSweep = 64;
constexpr int kOdomFields(int d) { return 1 + d * d + d; }
template <int D>
struct OdomEl {
  double v[D * D + D];  // R row-major, then t
  int flag;
};
struct OdomArgs {
  int d = 0, ntiles = 0;
  int64_t P = 0, n_edges = 0;
  const int32_t *pos_edge = nullptr, *pos_chain = nullptr;  // [P]: edge index (-1 at a head), chain index (at a head)
  const int32_t *pos_rot = nullptr, *pos_trn = nullptr;     // [P]: first INTERNAL rotation row, translation row of the pose written
  const double *edge_data = nullptr;                        // the measurement table's, [d*d + d + 2][n_edges]
  const double *starts = nullptr;                           // [chains][d]
  double *totals = nullptr, *carry = nullptr;               // [kOdomFields(d)][ntiles] each
  double *out = nullptr;                                    // d columns at stride ld_for(d) = d
  int *flag = nullptr;                                      // |= 1 where a product is not finite
};
// the other rows of the start: identity blocks and zero translations of the n_free poses in no chain, the landmarks' rows
// from lm ([n_lm][d] on the device; nullptr: zeros), then -- launch_odom_ranges, after everything above -- range row m =
// the direction of x_t(b) - x_t(a) through range_rows ([3][n_ranges] internal rows: range | a | b), deg[m] = 1 and a
// zero row where it has none (odom_range_row), partial[odom_range_blocks] = the blocks' counts of those, words[0] their sum
struct OdomFillArgs {
  int d = 0;
  int64_t n_free = 0, n_lm = 0, n_ranges = 0;
  const int32_t *free_rot = nullptr, *free_trn = nullptr, *lm_row = nullptr, *range_rows = nullptr;
  const double *lm = nullptr;
  unsigned char *deg = nullptr;
  int *partial = nullptr, *words = nullptr, *flag = nullptr;
  double *out = nullptr;
};
inline int odom_tiles(int64_t P) { return static_cast<int>((P + kOdomTile - 1) / kOdomTile); }
inline int odom_range_blocks(int64_t n_ranges) { return static_cast<int>((n_ranges + kWave - 1) / kWave); }
hipError_t launch_odom_scan(const OdomArgs &A, hipStream_t st);      // the three launches; P == 0: none
hipError_t launch_odom_fill(const OdomFillArgs &A, hipStream_t st);  // free poses and landmarks; none of either: no launch
hipError_t launch_odom_ranges(const OdomFillArgs &A, hipStream_t st);  // + the sum of the counts; no ranges: words[0] = 0
// The arithmetic, shared by the kernels and the host mirror (cora_debug_odometry_init_host): single correctly rounded
// fp64 operations in the order written, never contracted; one fma per term.
// b = a o b:  a right operand with its flag set wins; else R = R_a R_b (every entry from +0.0, k ascending),
// t = t_a + R_a t_b (from t_a, k ascending), flag = flag_a
template <int D>
__host__ __device__ inline void odom_compose(const OdomEl<D> &a, OdomEl<D> &b) {
#pragma clang fp contract(off)
  if (b.flag) return;
  double r[D * D + D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(a.v[i * D + k], b.v[k * D + j], s);
      r[i * D + j] = s;
    }
    double s = a.v[D * D + i];
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(a.v[i * D + k], b.v[D * D + k], s);
    r[D * D + i] = s;
  }
#pragma unroll
  for (int i = 0; i < D * D + D; ++i) b.v[i] = r[i];
  b.flag = a.flag;
}
template <int D>
__host__ __device__ inline void odom_head(OdomEl<D> &e) {  // (1, I, 0)
#pragma unroll
  for (int i = 0; i < D * D + D; ++i) e.v[i] = (i < D * D && i / D == i % D) ? 1.0 : 0.0;
  e.flag = 1;
}
__host__ __device__ inline bool odom_finite(const double *v, int n) {
  bool finite = true;
  for (int i = 0; i < n; ++i) finite = finite && fabs(v[i]) <= 1.79769313486231570815e308;
  return finite;
}
// row = (tb - ta) / |tb - ta|; returns true, and a zero row, where the norm is below 1e-5 (a degenerate row)
template <int D>
__host__ __device__ inline bool odom_range_row(const double *ta, const double *tb, double *row) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    row[c] = tb[c] - ta[c];
    s = fma(row[c], row[c], s);
  }
  const double nrm = sqrt(s);
  if (nrm < 1e-5) {
#pragma unroll
    for (int c = 0; c < D; ++c) row[c] = 0.0;
    return true;
  }
#pragma unroll
  for (int c = 0; c < D; ++c) row[c] = row[c] / nrm;
  return false;
}

// Landmark initialisation from ranges: multilateration (kernels/multilat.inc; include/cora_hip.h, cora_multilaterate_dev).
// The usable ranges of the measurement table (one endpoint a landmark, the other a pose) are grouped per landmark into
// lists in table order and cut into chunks of kMlChunk entries, none across two lists.  Every stage is two launches:
//   pass : one workgroup of kMlChunk threads per chunk, one entry per thread: the entry's terms (ml_linear_terms,
//          ml_gn_terms), summed over the chunk into partial[sum][chunk]
//   fold : ONE wavefront per landmark sums its chunks' partials and runs ml_fold on the sums
// stage 0 is the linear solve, stage j >= 1 evaluates visited point j - 1 (cost, and H, g of the Gauss-Newton step to
// point j); the last stage evaluates only and writes the row: 2 (gn_steps + 2) launches.
// BRACKET ORDER, a function of the list length and kMlChunk alone and the same in the host mirror (capi/multilat.inc):
//   wavefront: a butterfly over lane exchanges, offsets 1, 2, .., 32 -- every lane takes (lane) + (lane ^ off): the
//              balanced tree ((l0 + l1) + (l2 + l3)) + ..; lanes without an entry hold +0.0;
//   chunk: the four wavefronts from the left, ((W_0 + W_1) + W_2) + W_3;
//   landmark: lane j of the fold takes 0.0 + chunk j + chunk (j + 64) + .. of the list from the left, then the butterfly.
// Every term is made of single correctly rounded fp64 operations in the order written, never contracted.
constexpr int kMlChunk = 256;
constexpr int kMlMaxSteps = 16;
constexpr double kMlMinPivot = 1e-8;     // of the scaled (d + 1) x (d + 1) normal matrix of the linear stage
constexpr double kMlGnMinPivot = 1e-12;  // of H / sum(omega)
constexpr int kMlSums(int d) { return 2 + 2 * d + d * (d + 1) / 2; }   // sum w | w u | w u u^T (upper) | w b | w b u
constexpr int kMlGnSums(int d) { return d * (d + 1) / 2 + d + 1; }    // sum w J J^T (upper) | w J e | w e^2
constexpr int kMlState(int d) { return 2 * d + 3; }                   // y | least-cost y | its cost | linear cost | sum w
constexpr int kMlInts = 4;                                            // status | chosen | steps taken | still stepping
struct MlArgs {
  int d = 0, stage = 0, last = 0;
  int64_t n_lm = 0, n_chunks = 0, n_entries = 0, n_ranges = 0;
  const int32_t *chunk_lm = nullptr, *chunk_begin = nullptr, *chunk_len = nullptr;  // [n_chunks]
  const int32_t *ent_row = nullptr, *ent_m = nullptr;  // [n_entries]: INTERNAL row of the anchor, range measurement
  const int32_t *lm_chunk0 = nullptr;                  // [n_lm + 1]: first chunk of a list
  const int32_t *lm_row = nullptr, *lm_origin = nullptr;  // [n_lm]: INTERNAL row of the landmark, of its first anchor (-1: none)
  const unsigned char *lm_init = nullptr;              // [n_lm]: 0 to be solved | 1 too few entries | 3 masked or empty
  const double *range_data = nullptr;                  // the measurement table's, [2][n_ranges]: r | omega
  double *partial = nullptr;                           // [kMlSums(d)][n_chunks]
  double *state = nullptr;                             // [n_lm][kMlState(d)], positions relative to the origin
  int32_t *istate = nullptr;                           // [n_lm][kMlInts]
  double *x = nullptr;                                 // d columns at stride ld_for(d) = d
  int *flag = nullptr;                                 // |= 1 where a sum is not finite
};
hipError_t launch_multilat_stage(const MlArgs &A, hipStream_t st);  // pass and fold of A.stage; no landmark: no launch
// terms of one entry of the linear stage: u = t_i - t_0, b = r^2 - |u|^2
template <int D>
__host__ __device__ inline void ml_linear_terms(const double *t0, const double *ti, double r, double w, double *s) {
#pragma clang fp contract(off)
  double u[D], wu[D], n2 = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    u[c] = ti[c] - t0[c];
    n2 = fma(u[c], u[c], n2);
    wu[c] = w * u[c];
  }
  const double wb = w * fma(r, r, -n2);
  int k = 0;
  s[k++] = w;
#pragma unroll
  for (int c = 0; c < D; ++c) s[k++] = wu[c];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) s[k++] = wu[a] * u[b];
  s[k++] = wb;
#pragma unroll
  for (int c = 0; c < D; ++c) s[k++] = wb * u[c];
}
// terms of one entry at the point t_0 + y: D = y - u, J = D / |D| (0 where |D| == 0), e = |D| - r
template <int D>
__host__ __device__ inline void ml_gn_terms(const double *y, const double *t0, const double *ti, double r, double w, double *s) {
#pragma clang fp contract(off)
  double dv[D], J[D], wJ[D], n2 = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    dv[c] = y[c] - (ti[c] - t0[c]);
    n2 = fma(dv[c], dv[c], n2);
  }
  const double nrm = sqrt(n2), e = nrm - r;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    J[c] = nrm == 0.0 ? 0.0 : dv[c] / nrm;
    wJ[c] = w * J[c];
  }
  int k = 0;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) s[k++] = wJ[a] * J[b];
#pragma unroll
  for (int c = 0; c < D; ++c) s[k++] = wJ[c] * e;
  s[k++] = (w * e) * e;
}
// Cholesky without pivoting of the symmetric M (n x n row-major, upper part read) and the solve of M z = q in place in
// q; returns false, with q undefined, at the first pivot <= min_pivot (or not a number)
template <int N>
__host__ __device__ inline bool ml_cholesky_solve(const double *M, double *q, double min_pivot) {
#pragma clang fp contract(off)
  double G[N * N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double p = M[j * N + j];
#pragma unroll
    for (int k = 0; k < j; ++k) p = fma(-G[j * N + k], G[j * N + k], p);
    if (!(p > min_pivot)) return false;
    const double g = sqrt(p);
    G[j * N + j] = g;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = M[j * N + i];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-G[i * N + k], G[j * N + k], v);
      G[i * N + j] = v / g;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = q[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-G[i * N + k], q[k], v);
    q[i] = v / G[i * N + i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = q[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) v = fma(-G[k * N + i], q[k], v);
    q[i] = v / G[i * N + i];
  }
  return true;
}
// The linear stage of a landmark from its sums S: the normal equations of |x|^2 - 2 u^T x = b in (x, s), lengths scaled
// by the ONE scale L = sqrt(sum w |u|^2 / sum w), divided by sum w.  Returns the status (0 solved, 2 degenerate), y = L x'.
template <int D>
__host__ __device__ inline int ml_linear_solve(const double *S, double *y) {
#pragma clang fp contract(off)
  constexpr int N = D + 1, UU = 1 + D, B = UU + D * (D + 1) / 2;
  const double sw = S[0];
  if (!(sw > 0.0)) return 2;
  double tr = 0.0;
  {
    int k = UU;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      tr = tr + S[k];
      k += D - a;
    }
  }
  const double L = sqrt(tr / sw);
  if (!(L > 0.0)) return 2;
  const double Lsw = L * sw, Ltr = L * tr;
  double M[N * N], q[N];
  int k = UU;
#pragma unroll
  for (int a = 0; a < D; ++a) {
#pragma unroll
    for (int b = a; b < D; ++b) M[a * N + b] = M[b * N + a] = (4.0 * S[k++]) / tr;
    M[a * N + D] = M[D * N + a] = (-2.0 * S[1 + a]) / Lsw;
    q[a] = (-2.0 * S[B + 1 + a]) / Ltr;
  }
  M[D * N + D] = 1.0;
  q[D] = S[B] / tr;
  if (!ml_cholesky_solve<N>(M, q, kMlMinPivot)) return 2;
#pragma unroll
  for (int c = 0; c < D; ++c) y[c] = L * q[c];
  return odom_finite(y, D) ? 0 : 2;
}
// y <- y - H^-1 g with H = sum w J J^T / sum w, g = sum w J e / sum w; false, and y kept, at a pivot <= kMlGnMinPivot
// or a step that is not finite
template <int D>
__host__ __device__ inline bool ml_gn_step(const double *S, double sw, double *y) {
#pragma clang fp contract(off)
  double H[D * D], g[D], yn[D];
  int k = 0;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) H[a * D + b] = H[b * D + a] = S[k++] / sw;
#pragma unroll
  for (int c = 0; c < D; ++c) g[c] = S[k++] / sw;
  if (!ml_cholesky_solve<D>(H, g, kMlGnMinPivot)) return false;
#pragma unroll
  for (int c = 0; c < D; ++c) yn[c] = y[c] - g[c];
  if (!odom_finite(yn, D)) return false;
#pragma unroll
  for (int c = 0; c < D; ++c) y[c] = yn[c];
  return true;
}
// What the fold does with the sums S of a landmark at a stage (st: kMlState(D) doubles, ist: kMlInts integers, init: the
// status known from the list alone).  Returns false where a sum is not finite (the landmark is then given up: status 2).
template <int D>
__host__ __device__ inline bool ml_fold(int stage, int last, const double *S, double *st, int32_t *ist, int init) {
  double *y = st, *best = st + D, &cbest = st[2 * D], &clin = st[2 * D + 1], &sw = st[2 * D + 2];
  if (stage == 0) {
    for (int i = 0; i < kMlState(D); ++i) st[i] = 0.0;
    ist[0] = init;
    ist[1] = -1;
    ist[2] = ist[3] = 0;
    if (init != 0) return true;
    if (!odom_finite(S, kMlSums(D))) {
      ist[0] = 2;
      return false;
    }
    ist[0] = ml_linear_solve<D>(S, y);
    if (ist[0] != 0) {
      for (int c = 0; c < D; ++c) y[c] = 0.0;
      return true;
    }
    for (int c = 0; c < D; ++c) best[c] = y[c];
    sw = S[0];
    ist[3] = 1;
    return true;
  }
  if (ist[0] != 0) return true;
  if (!odom_finite(S, kMlGnSums(D))) {
    ist[3] = 0;
    return false;
  }
  const double cost = S[kMlGnSums(D) - 1];
  if (stage == 1) {
    clin = cbest = cost;
    ist[1] = 0;
  } else if (cost < cbest) {
    cbest = cost;
    for (int c = 0; c < D; ++c) best[c] = y[c];
    ist[1] = stage - 1;
  }
  if (!last && ist[3]) {
    if (ml_gn_step<D>(S, sw, y)) ist[2] += 1;
    else ist[3] = 0;
  }
  return true;
}

// Outlier-robust multilateration: a consensus vote over minimal hypotheses (kernels/multilat.inc; include/cora_hip.h,
// cora_multilaterate_robust_dev).  Tables, lists, chunks, origin and masks are the plain multilateration's.  Per
// list of a landmark with lm_init == 0, of length L >= d + 1, entries e = 0 .. L - 1 in table order, u_j = t_j - t_0:
//   sample of entry h : entries (h + k s) mod L, k = 0 .. d, s = max(1, L / (d + 1)) (ml_sample) -- distinct as d s < L, spread
//                       over the list, a function of (h, L, d) alone;
//   hypothesis y_h    : the sample's ml_linear_terms added from the left in the order k = 0 .. d from +0.0, then
//                       ml_linear_solve (ml_hypothesis); valid where the solve returns 0, else y = 0, vote 0, no flag;
//   score             : r(h, j) = (omega_j e) e, e = |y_h - u_j| - r_j (ml_cost_at: the last term of ml_gn_terms);
//   vote(h)           : #{j : r(h, j) <= barc2} over EVERY entry j, the sample's own included (cl_agrees: a NaN is no vote) --
//                       a valid hypothesis has about d + 1 votes of its own, a consensus means something above d + 1 only;
//   election          : the largest vote, among equal votes the lowest entry (cl_better); consensus = its vote; consensus <
//                       min_consensus: status 5, the landmark keeps its row; no valid hypothesis: entry 0, consensus 0;
//   I = {j : r(h*, j) <= barc2} (empty at consensus 0); the plain stages run over I alone: AN ENTRY OUTSIDE I ADDS +0.0 FOR
//                       EACH OF ITS TERMS, as a lane beyond the chunk's end does, so the bracket order of a sum is the plain one's.
// 2 + 2 (gn_steps + 2) launches: vote, elect, then the plain stages with the masked passes.  One election, one refit.
constexpr int kMlCState(int d) { return d; }  // of the elected hypothesis: y
constexpr int kMlCInts = 2;                   // elected entry (index in its list) | consensus
struct MlRobustArgs {
  MlArgs A;
  double barc2 = 0.0;
  int min_consensus = 0;
  int32_t *votes = nullptr;         // [n_entries]
  double *cstate = nullptr;         // [n_lm][kMlCState(d)]
  int32_t *cint = nullptr;          // [n_lm][kMlCInts], written where lm_init == 0
  unsigned char *inlier = nullptr;  // [n_ranges]: written where a range is an entry of a list with lm_init == 0, 1 in I | 0 outside
};
hipError_t launch_multilat_vote_elect(const MlRobustArgs &R, hipStream_t st);    // k_ml_vote and k_ml_elect over all lists
hipError_t launch_multilat_robust_stage(const MlRobustArgs &R, hipStream_t st);  // masked pass and fold of R.A.stage
// entry k of the sample of entry h of a list of len entries (h < len, 0 <= k <= D, len >= D + 1)
template <int D>
__host__ __device__ inline int32_t ml_sample(int32_t h, int k, int32_t len) {
  const int32_t s = len / (D + 1) > 1 ? len / (D + 1) : 1;
  const int32_t e = h + k * s;  // (< 2 len)
  return e >= len ? e - len : e;
}
// The point the D + 1 ranges of a sample determine: t: the sample's anchors [D + 1][D], r, w: their ranges and precisions.
// Returns whether the hypothesis is valid; y = 0 where it is not.
template <int D>
__host__ __device__ inline bool ml_hypothesis(const double *t0, const double *t, const double *r, const double *w, double *y) {
#pragma clang fp contract(off)
  constexpr int NS = kMlSums(D);
  double S[NS], term[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) S[i] = 0.0;
#pragma unroll
  for (int k = 0; k <= D; ++k) {
    ml_linear_terms<D>(t0, t + k * D, r[k], w[k], term);
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = S[i] + term[i];
  }
  if (ml_linear_solve<D>(S, y) == 0) return true;
#pragma unroll
  for (int c = 0; c < D; ++c) y[c] = 0.0;
  return false;
}
// the weighted squared range residual of an entry (u = t_j - t_0) at the point t_0 + y, without the 1/2
template <int D>
__host__ __device__ inline double ml_cost_at(const double *y, const double *u, double r, double w) {
#pragma clang fp contract(off)
  double n2 = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const double dv = y[c] - u[c];
    n2 = fma(dv, dv, n2);
  }
  const double e = sqrt(n2) - r;
  return (w * e) * e;
}

// Chain placement from inter-robot ranges (kernels/placement.inc; include/cora_hip.h, cora_place_chains_dev): the
// multilateration with a rigid body in place of a point.  The host orders the chains into STAGES (capi/placement.inc); a
// stage finds g = (R, t) in SE(d) that moves one chain onto the chains placed before it, from the stage's entry list (row
// of the chain's position q, row of the anchor a, range measurement), cut into chunks of kPlChunk entries.  The stages are
// dependent, so every launch below serves ONE stage; per stage, with s = gn_steps:
//   linear        : pass (one workgroup per chunk) and fold (ONE wavefront) of the linear stage in the squared ranges
//   step 0 .. s+1 : pass and fold of a Gauss-Newton evaluation: step 0 at the identity (visited point 0), step 1 at the
//                   linear stage's point (visited point 1), step k at the point after k - 1 Gauss-Newton steps; every
//                   step but the last also takes the next Gauss-Newton step
//   apply         : one thread per position of the chain
// 2 (s + 3) + 1 launches.  Coordinates are taken relative to the first entry: q' = q - q_0, a' = a - a_0, and the
// translation the stages carry is t' = R q_0 + t - a_0, so that |R q + t - a| = |R q' + t' - a'|; the identity is
// (I, q_0 - a_0).  No transcendental function: the rotation update is the Cayley map, then round_rotation.
// BRACKET ORDER, a function of the list length and kPlChunk alone and the same in the host mirror (capi/placement.inc):
//   linear pass: the entry's kPlTerms(d) terms and its weight are staged in LDS; thread p < kPlSums(d) owns the pair (i, j)
//                of pl_pair and sums (w_e c_i(e)) c_j(e) over the chunk's entries from the left, from +0.0 (pl_pair_sum);
//   Gauss-Newton pass: as the multilateration's -- butterfly per wavefront, lanes without an entry hold +0.0, the four
//                wavefronts from the left;
//   fold: lane j takes 0.0 + chunk j + chunk (j + 64) + .. of the stage from the left, then the butterfly.
// Every term is made of single correctly rounded fp64 operations in the order written, never contracted.
constexpr int kPlChunk = 256;
constexpr int kPlMaxSteps = 16;
constexpr double kPlMinPivot = 1e-8;     // of the scaled normal matrix of the linear stage, divided by sum(omega)
constexpr double kPlGnMinPivot = 1e-12;  // of H / sum(omega), rotations in units of the length scale
constexpr int kPlUnknowns(int d) { return d == 2 ? 7 : 16; }  // s | v = R^T t | M (d = 2: c, s; d = 3: 9 entries) | t
constexpr int kPlTerms(int d) { return kPlUnknowns(d) + 1; }  // the coefficients, then the right-hand side
constexpr int kPlSums(int d) { return kPlTerms(d) * (kPlTerms(d) + 1) / 2; }  // sum w c_i c_j, i <= j: 36, 153
constexpr int kPlDof(int d) { return d * (d + 1) / 2; }                      // rotation, then translation
constexpr int kPlGnSums(int d) { return kPlDof(d) * (kPlDof(d) + 1) / 2 + kPlDof(d) + 1; }  // w J J^T (upper) | w J e | w e^2: 10, 28
constexpr int kPlG(int d) { return d * d + d; }                              // R row-major | translation
// current (R, t') | least-cost (R, t') | written (R, t) | least cost | cost at the identity | cost at the linear point | sum w | L
constexpr int kPlState(int d) { return 3 * kPlG(d) + 5; }
constexpr int kPlInts = 4;  // status | chosen | steps taken | still stepping
struct PlArgs {
  int d = 0, step = 0, last = 0;
  int32_t chunk0 = 0, n_chunks = 0;                    // the stage's chunks in the chunk table
  int32_t origin_q = 0, origin_a = 0;                  // INTERNAL rows of the first entry's position and anchor
  int32_t pos0 = 0, n_pos = 0;                         // the chain's positions in the chain tables
  int64_t n_ranges = 0, pstride = 0;
  const int32_t *chunk_begin = nullptr, *chunk_len = nullptr;            // [chunks of all stages]
  const int32_t *ent_q = nullptr, *ent_a = nullptr, *ent_m = nullptr;    // [entries]: INTERNAL rows, range measurement
  const int32_t *pos_rot = nullptr, *pos_trn = nullptr;                  // the chain tables' (OdomArgs)
  const double *range_data = nullptr;                  // the measurement table's, [2][n_ranges]: r | omega
  double *partial = nullptr;                           // [kPlSums(d)][pstride], pstride >= the most chunks of a stage
  double *state = nullptr;                             // kPlState(d) doubles of THIS stage
  int32_t *istate = nullptr;                           // kPlInts integers of THIS stage
  double *x = nullptr;                                 // d columns at stride ld_for(d) = d
  int *flag = nullptr;                                 // |= 1 where a sum is not finite
};
hipError_t launch_place_linear(const PlArgs &A, hipStream_t st);  // pass and fold of the linear stage
hipError_t launch_place_gn(const PlArgs &A, hipStream_t st);      // pass and fold of evaluation A.step
hipError_t launch_place_apply(const PlArgs &A, hipStream_t st);
// The batched form (cora_place_chains_batched_dev): the host groups the stages into LEVELS (capi/placement.inc; a level's
// stages read only rows that earlier levels wrote, so they are independent) and every launch serves ALL stages of one level:
// the passes one workgroup per chunk of the level, the folds one wavefront per stage, the apply one workgroup per tile of
// 256 positions of one chain -- 2 (s + 3) + 1 launches per level.  The kernels are the plain ones' bodies (template axis
// BATCHED, kernels/placement.inc); terms, chunk sums and the fold's bracket order over a stage's own chunks are the plain
// call's, so the bits are.  In A: chunk0 / n_chunks the LEVEL's chunks, partial [kPlSums(d)][pstride] indexed by the chunk's
// place in its level (pstride >= the most chunks of a level), state / istate the arrays of ALL stages; origin_q, origin_a,
// pos0, n_pos unused.
struct PlBatchArgs {
  PlArgs A;
  int32_t stage0 = 0, n_stages = 0;                    // the level's stages
  int32_t tile0 = 0, n_tiles = 0;                      // the level's apply tiles
  const int32_t *chunk_stage = nullptr;                // [chunks of all stages]
  const int32_t *stage_chunk0 = nullptr;               // [stages + 1]
  const int32_t *stage_origin_q = nullptr, *stage_origin_a = nullptr;  // [stages]: INTERNAL rows of the first entry
  const int32_t *stage_pos0 = nullptr, *stage_npos = nullptr;          // [stages]: the chain's positions in the chain tables
  const int32_t *tile_stage = nullptr, *tile_off = nullptr;            // [tiles]: stage, first position of the tile within the chain
};
// what every batched launch asks of its arguments (the robust form's too: PlRobustArgs below)
inline bool pl_batch_args_ok(const PlBatchArgs &B) {
  const PlArgs &A = B.A;
  return (A.d == 2 || A.d == 3) && A.n_chunks > 0 && A.chunk0 >= 0 && A.pstride >= A.n_chunks && B.n_stages > 0 && B.stage0 >= 0 &&
         B.n_stages <= A.n_chunks && B.n_tiles >= B.n_stages && B.tile0 >= 0 && A.n_ranges > 0 && A.chunk_begin && A.chunk_len && A.ent_q &&
         A.ent_a && A.ent_m && A.pos_rot && A.pos_trn && A.range_data && A.partial && A.state && A.istate && A.x && A.flag && B.chunk_stage &&
         B.stage_chunk0 && B.stage_origin_q && B.stage_origin_a && B.stage_pos0 && B.stage_npos && B.tile_stage && B.tile_off;
}
hipError_t launch_place_linear(const PlBatchArgs &B, hipStream_t st);
hipError_t launch_place_gn(const PlBatchArgs &B, hipStream_t st);  // evaluation B.A.step
hipError_t launch_place_apply(const PlBatchArgs &B, hipStream_t st);
// pair p of the upper triangle in row-major order: (0,0), (0,1), .., (0,nt-1), (1,1), ..
__host__ __device__ inline void pl_pair(int nt, int p, int *i, int *j) {
  int r = 0;
  while (p >= nt - r) {
    p -= nt - r;
    ++r;
  }
  *i = r;
  *j = r + p;
}
__host__ __device__ inline int pl_pair_index(int nt, int i, int j) { return i * nt - i * (i - 1) / 2 + (j - i); }  // i <= j
// the power of the length scale a term carries: 1 | q | a q | a | right-hand side
template <int D>
__host__ __device__ inline int pl_degree(int i) {
  constexpr int MM = D == 2 ? 2 : 9;
  return i == 0 ? 0 : i <= D ? 1 : i <= D + MM ? 2 : i <= D + MM + D ? 1 : 2;
}
// terms of one entry of the linear stage: |q'|^2 + |a'|^2 + s + 2 q'.v - 2 a'^T M q' - 2 a'.t = r^2
template <int D>
__host__ __device__ inline void pl_linear_terms(const double *q0, const double *a0, const double *q, const double *a, double r, double *c) {
#pragma clang fp contract(off)
  double qq[D], aa[D], n2 = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    qq[k] = q[k] - q0[k];
    aa[k] = a[k] - a0[k];
  }
#pragma unroll
  for (int k = 0; k < D; ++k) n2 = fma(qq[k], qq[k], n2);
#pragma unroll
  for (int k = 0; k < D; ++k) n2 = fma(aa[k], aa[k], n2);
  int at = 0;
  c[at++] = 1.0;
#pragma unroll
  for (int k = 0; k < D; ++k) c[at++] = 2.0 * qq[k];
  if constexpr (D == 2) {
    c[at++] = -2.0 * fma(aa[0], qq[0], aa[1] * qq[1]);     // cos:  a . q
    c[at++] = -2.0 * fma(aa[1], qq[0], -(aa[0] * qq[1]));  // sin:  a_y q_x - a_x q_y
  } else {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) c[at++] = -2.0 * (aa[i] * qq[j]);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) c[at++] = -2.0 * aa[k];
  c[at++] = fma(r, r, -n2);
}
// sum over the chunk's entries, from the left, of (w_e c_i(e)) c_j(e); term: [len][nt]
__host__ __device__ inline double pl_pair_sum(const double *term, const double *wt, int len, int nt, int i, int j) {
#pragma clang fp contract(off)
  double v = 0.0;
  for (int e = 0; e < len; ++e) v = v + (wt[e] * term[e * nt + i]) * term[e * nt + j];
  return v;
}
// Cholesky without pivoting in place in M (n x n row-major: the upper part is read, the factor is left in the lower part
// and on the diagonal) and the solve of M z = q in place; false at the first pivot <= min_pivot (or not a number).  Loops,
// no local array: the fold runs it on LDS.
__host__ __device__ inline bool pl_cholesky_solve(int n, double *M, double *q, double min_pivot) {
#pragma clang fp contract(off)
  for (int j = 0; j < n; ++j) {
    double p = M[j * n + j];
    for (int k = 0; k < j; ++k) p = fma(-M[j * n + k], M[j * n + k], p);
    if (!(p > min_pivot)) return false;
    const double g = sqrt(p);
    M[j * n + j] = g;
    for (int i = j + 1; i < n; ++i) {
      double v = M[j * n + i];
      for (int k = 0; k < j; ++k) v = fma(-M[i * n + k], M[j * n + k], v);
      M[i * n + j] = v / g;
    }
  }
  for (int i = 0; i < n; ++i) {
    double v = q[i];
    for (int k = 0; k < i; ++k) v = fma(-M[i * n + k], q[k], v);
    q[i] = v / M[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = q[i];
    for (int k = i + 1; k < n; ++k) v = fma(-M[k * n + i], q[k], v);
    q[i] = v / M[i * n + i];
  }
  return true;
}
__host__ __device__ inline double pl_power(double L, int k) {
#pragma clang fp contract(off)
  double v = 1.0;
  for (int i = 0; i < k; ++i) v = v * L;
  return v;
}
// The linear stage from the sums S (kPlSums(D)): lengths scaled by the ONE scale L = sqrt(sum w (|q'|^2 + |a'|^2) /
// (2 sum w)), the normal equations divided by sum w; work: kPlUnknowns(D) (kPlUnknowns(D) + 1) doubles.  Returns the
// status (0 solved, 2 refused) and g = (R, t'); *scale = L (1 where it has none), *sum_w = S[0].
template <int D>
__host__ __device__ inline int pl_linear_solve(const double *S, double *work, double *g, double *scale, double *sum_w) {
#pragma clang fp contract(off)
  constexpr int N = kPlUnknowns(D), NT = kPlTerms(D), MM = D == 2 ? 2 : 9;
  const double sw = S[0];
  *scale = 1.0;
  *sum_w = sw;
  if (!(sw > 0.0)) return 2;
  double tr = 0.0;
  for (int k = 0; k < D; ++k) tr = tr + S[pl_pair_index(NT, 1 + k, 1 + k)];
  for (int k = 0; k < D; ++k) tr = tr + S[pl_pair_index(NT, 1 + D + MM + k, 1 + D + MM + k)];
  const double L = sqrt(tr / (8.0 * sw));
  if (!(L > 0.0) || !(L <= 1.79769313486231570815e308)) return 2;
  *scale = L;
  double *M = work, *z = work + N * N;
  for (int i = 0; i < N; ++i) {
    for (int j = i; j < N; ++j) {
      const double v = S[pl_pair_index(NT, i, j)] / (sw * pl_power(L, pl_degree<D>(i) + pl_degree<D>(j)));
      M[i * N + j] = v;
      M[j * N + i] = v;
    }
    z[i] = S[pl_pair_index(NT, i, N)] / (sw * pl_power(L, pl_degree<D>(i) + 2));
  }
  if (!pl_cholesky_solve(N, M, z, kPlMinPivot)) return 2;
  if constexpr (D == 2) {
    const double c = z[3], s = z[4], nrm = sqrt(fma(c, c, s * s));
    if (!(nrm > 0.0) || !(nrm <= 1.79769313486231570815e308)) return 2;
    g[0] = c / nrm;
    g[1] = -(s / nrm);
    g[2] = s / nrm;
    g[3] = c / nrm;
  } else {
    double R[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) R[i][j] = z[1 + D + i * D + j];
    if (!odom_finite(&R[0][0], D * D)) return 2;
    round_rotation<D>(R);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) g[i * D + j] = R[i][j];
  }
#pragma unroll
  for (int k = 0; k < D; ++k) g[D * D + k] = L * z[1 + D + MM + k];
  return odom_finite(g, kPlG(D)) ? 0 : 2;
}
// the identity in the stage's coordinates: (I, q_0 - a_0)
template <int D>
__host__ __device__ inline void pl_identity(const double *q0, const double *a0, double *g) {
#pragma unroll
  for (int i = 0; i < D * D; ++i) g[i] = i / D == i % D ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) g[D * D + k] = q0[k] - a0[k];
}
// What the linear fold does with the sums: every field of the stage's state, the status, the current point (the linear
// stage's, or the identity where it is refused), the least-cost point = the identity.  False where a sum is not finite.
template <int D>
__host__ __device__ inline bool pl_fold_linear(const double *S, double *work, double *st, int32_t *ist, const double *q0, const double *a0) {
  constexpr int G = kPlG(D);
  for (int i = 0; i < kPlState(D); ++i) st[i] = 0.0;
  pl_identity<D>(q0, a0, st + G);
  ist[0] = 0;
  ist[1] = -1;
  ist[2] = 0;
  ist[3] = 1;
  st[3 * G + 4] = 1.0;
  const bool finite = odom_finite(S, kPlSums(D));
  ist[0] = finite ? pl_linear_solve<D>(S, work, st, st + 3 * G + 4, st + 3 * G + 3) : 2;
  if (ist[0] != 0) pl_identity<D>(q0, a0, st);
  return finite;
}
// terms of one entry at g = (R, t'): u = R q', p = u + t' - a', n = p / |p| (0 where |p| == 0), e = |p| - r;
// J = ((u x n) / L | n): the rotation in units of the length scale L
template <int D>
__host__ __device__ inline void pl_gn_terms(const double *g, double L, const double *q0, const double *a0, const double *q, const double *a,
                                            double r, double w, double *s) {
#pragma clang fp contract(off)
  constexpr int F = kPlDof(D);
  double qq[D], u[D], p[D], n[D], J[F], wJ[F], n2 = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) qq[k] = q[k] - q0[k];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) v = fma(g[i * D + k], qq[k], v);
    u[i] = v;
    p[i] = (v + g[D * D + i]) - (a[i] - a0[i]);
    n2 = fma(p[i], p[i], n2);
  }
  const double nrm = sqrt(n2), e = nrm - r;
#pragma unroll
  for (int k = 0; k < D; ++k) n[k] = nrm == 0.0 ? 0.0 : p[k] / nrm;
  if constexpr (D == 2) {
    J[0] = fma(u[0], n[1], -(u[1] * n[0])) / L;
  } else {
    J[0] = fma(u[1], n[2], -(u[2] * n[1])) / L;
    J[1] = fma(u[2], n[0], -(u[0] * n[2])) / L;
    J[2] = fma(u[0], n[1], -(u[1] * n[0])) / L;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) J[F - D + k] = n[k];
#pragma unroll
  for (int k = 0; k < F; ++k) wJ[k] = w * J[k];
  int at = 0;
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = i; j < F; ++j) s[at++] = wJ[i] * J[j];
#pragma unroll
  for (int k = 0; k < F; ++k) s[at++] = wJ[k] * e;
  s[at++] = (w * e) * e;
}
// g <- the Gauss-Newton step from g: delta = -H^-1 grad with H = sum w J J^T / sum w; R <- round_rotation(C R) with C the
// Cayley map of the rotation step b = delta_rot / (2 L) (d = 3: ((1 - b.b) I + 2 b b^T + 2 [b]x) / (1 + b.b)), t' <- t' +
// delta_t.  False, and g kept, at a pivot <= kPlGnMinPivot or a step that is not finite.
template <int D>
__host__ __device__ inline bool pl_gn_step(const double *S, double sw, double L, double *g) {
#pragma clang fp contract(off)
  constexpr int F = kPlDof(D);
  double H[F * F], dl[F], gn[kPlG(D)];
  int at = 0;
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = i; j < F; ++j) H[i * F + j] = H[j * F + i] = S[at++] / sw;
#pragma unroll
  for (int k = 0; k < F; ++k) dl[k] = S[at++] / sw;
  if (!ml_cholesky_solve<F>(H, dl, kPlGnMinPivot)) return false;
  double C[D][D], R[D][D];
  if constexpr (D == 2) {
    const double b = -dl[0] / (2.0 * L), den = fma(b, b, 1.0);
    const double cs = fma(-b, b, 1.0) / den, sn = (2.0 * b) / den;
    C[0][0] = cs;
    C[0][1] = -sn;
    C[1][0] = sn;
    C[1][1] = cs;
  } else {
    double b[3], bb = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b[k] = -dl[k] / (2.0 * L);
      bb = fma(b[k], b[k], bb);
    }
    const double den = 1.0 + bb, dg = 1.0 - bb;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // [b]x: (0,1) -b2, (0,2) b1, (1,2) -b0 and the opposite signs below the diagonal
        const double cr = i == j ? 0.0 : ((j - i + 3) % 3 == 1 ? -b[(6 - i - j) % 3] : b[(6 - i - j) % 3]);
        C[i][j] = (fma(2.0 * b[i], b[j], i == j ? dg : 0.0) + 2.0 * cr) / den;
      }
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) v = fma(C[i][k], g[k * D + j], v);
      R[i][j] = v;
    }
  if (!odom_finite(&R[0][0], D * D)) return false;
  round_rotation<D>(R);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) gn[i * D + j] = R[i][j];
#pragma unroll
  for (int k = 0; k < D; ++k) gn[D * D + k] = g[D * D + k] - dl[F - D + k];
  if (!odom_finite(gn, kPlG(D))) return false;
#pragma unroll
  for (int i = 0; i < kPlG(D); ++i) g[i] = gn[i];
  return true;
}
// What the fold of evaluation `step` does with the sums S (kPlGnSums(D)); at the last one also the transform as written:
// the identity exactly where point 0 has the least cost, else (R, t' + a_0 - R q_0).  False where a sum is not finite
// (the stage then stops stepping).
template <int D>
__host__ __device__ inline bool pl_fold_gn(int step, int last, const double *S, double *st, int32_t *ist, const double *q0, const double *a0) {
#pragma clang fp contract(off)
  constexpr int G = kPlG(D);
  double *cur = st, *best = st + G, *out = st + 2 * G, &cbest = st[3 * G], &cstart = st[3 * G + 1], &clin = st[3 * G + 2];
  const double sw = st[3 * G + 3], L = st[3 * G + 4];
  bool finite = odom_finite(S, kPlGnSums(D));
  if (!finite) {
    ist[3] = 0;
  } else {
    const double cost = S[kPlGnSums(D) - 1];
    if (step == 0) {
      cstart = cbest = clin = cost;
      ist[1] = 0;
    } else {
      if (step == 1) clin = cost;
      if (cost < cbest) {
        cbest = cost;
        for (int i = 0; i < G; ++i) best[i] = cur[i];
        ist[1] = step;
      }
      if (!last && ist[3]) {
        if (pl_gn_step<D>(S, sw, L, cur)) ist[2] += 1;
        else ist[3] = 0;
      }
    }
  }
  if (last) {
    for (int i = 0; i < G; ++i) out[i] = i < D * D && i / D == i % D ? 1.0 : 0.0;
    if (ist[1] > 0) {
      for (int i = 0; i < D * D; ++i) out[i] = best[i];
      for (int c = 0; c < D; ++c) {
        double v = best[D * D + c] + a0[c];
        for (int k = 0; k < D; ++k) v = fma(-best[c * D + k], q0[k], v);
        out[D * D + c] = v;
      }
    }
  }
  return finite;
}
// one position of the chain under g = (R, t): t_i <- R t_i + t (from t, k ascending), the stored block (R_i^T, row a =
// column a of R_i) <- R_i^T R^T (every entry from +0.0, k ascending)
template <int D>
__host__ __device__ inline void pl_apply(const double *g, double *rot, double *trn) {
#pragma clang fp contract(off)
  double nr[D * D], nt[D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) v = fma(rot[a * D + k], g[b * D + k], v);
      nr[a * D + b] = v;
    }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    double v = g[D * D + c];
#pragma unroll
    for (int k = 0; k < D; ++k) v = fma(g[c * D + k], trn[k], v);
    nt[c] = v;
  }
#pragma unroll
  for (int i = 0; i < D * D; ++i) rot[i] = nr[i];
#pragma unroll
  for (int c = 0; c < D; ++c) trn[c] = nt[c];
}

// Outlier-robust chain placement: a consensus vote over hypotheses from samples of m = kPlTerms(d) ranges in front of the
// batched fit (kernels/placement.inc, MASK; include/cora_hip.h, cora_place_chains_robust_dev).  Tables, order,
// lists, chunks and origin are the batched call's; every launch serves ALL stages of one level.  Per stage list of length
// L >= m (the least min_ranges), entries e = 0 .. L - 1 in table order, q' = q - q_0, a' = a - a_0:
//   sample of entry h : entries (h + k s) mod L, k = 0 .. m - 1, s = max(1, L / m) (pl_sample) -- distinct as (m - 1) s < L, a
//                       function of (h, L, d) alone;
//   hypothesis g_h    : the sample's pl_linear_terms and weights, the pair products added from the left in the order k (pl_pair_sum
//                       over the m staged entries), pl_linear_solve -- valid where it returns 0, else g = the identity (pl_identity),
//                       vote 0, no flag; then kPlHypSteps Gauss-Newton steps ON THE SAMPLE'S OWN m ENTRIES (pl_hyp_polish: pl_gn_terms
//                       added from the left in the order k from +0.0, pl_gn_step with the sample's L and sum w); a refused step keeps
//                       the point and ends the stepping, the hypothesis stays valid;
//   score             : r(h, j) = (w_j e) e, e = |R_h q'_j + t'_h - a'_j| - r_j (pl_cost_at: the last term of pl_gn_terms);
//   vote(h)           : #{j : r(h, j) <= barc2} over EVERY entry j, the sample's own included (cl_agrees: a NaN is no vote) -- a
//                       consensus means something above m only;
//   election          : the largest vote, among equal votes the lowest entry (cl_better); consensus = its vote; consensus <
//                       min_consensus: status 5, the chain keeps its rows; no valid hypothesis: entry 0, consensus 0;
//   I = {j : r(h*, j) <= barc2} (empty at consensus 0); the batched stages run over I alone: AN ENTRY OUTSIDE I ADDS +0.0 FOR
//                       EACH OF ITS TERMS (pl_pair_sum_masked; a Gauss-Newton lane that holds +0.0), so the bracket order of a
//                       sum is the plain one's and a list without outliers has the batched call's bits.
// Per level 3 + 2 (gn_steps + 3) + 1 launches: hypotheses, vote, election, then the batched call's.  One election, one refit.
constexpr int kPlHypSteps = 3;
constexpr int kPlCState(int d) { return kPlG(d); }  // of the elected hypothesis: (R, t')
constexpr int kPlCInts = 2;                         // elected entry (index in its list) | consensus
struct PlRobustArgs {
  PlBatchArgs B;
  double barc2 = 0.0;
  int min_consensus = 0;
  int32_t ent0 = 0, n_ent = 0;      // the level's entries (those of its chunks, consecutive)
  int64_t hstride = 0;
  double *hyp = nullptr;            // [kPlG(d)][hstride], by entry
  int32_t *votes = nullptr;         // [entries]
  double *cstate = nullptr;         // [stages][kPlCState(d)]
  int32_t *cint = nullptr;          // [stages][kPlCInts]
  unsigned char *inlier = nullptr;  // [n_ranges]: written where a range is an entry of a stage list, 1 in I | 0 outside
};
hipError_t launch_place_vote_elect(const PlRobustArgs &R, hipStream_t st);  // k_pl_hyp, k_pl_vote, k_pl_elect of the level
hipError_t launch_place_linear(const PlRobustArgs &R, hipStream_t st);      // the masked forms of the batched launches
hipError_t launch_place_gn(const PlRobustArgs &R, hipStream_t st);
hipError_t launch_place_apply(const PlRobustArgs &R, hipStream_t st);
// entry k of the sample of entry h of a list of len entries (h < len, 0 <= k < kPlTerms(D), len >= kPlTerms(D))
template <int D>
__host__ __device__ inline int32_t pl_sample(int32_t h, int k, int32_t len) {
  const int32_t s = len / kPlTerms(D) > 1 ? len / kPlTerms(D) : 1;
  const int32_t e = h + k * s;  // (< 2 len)
  return e >= len ? e - len : e;
}
// pl_pair_sum over the entries with in[e] != 0: an entry outside adds +0.0
__host__ __device__ inline double pl_pair_sum_masked(const double *term, const double *wt, const unsigned char *in, int len, int nt, int i, int j) {
#pragma clang fp contract(off)
  double v = 0.0;
  for (int e = 0; e < len; ++e) v = v + (in[e] ? (wt[e] * term[e * nt + i]) * term[e * nt + j] : 0.0);
  return v;
}
// the weighted squared range residual of an entry (qq = q', aa = a') at g = (R, t'), without the 1/2: the last term of pl_gn_terms
template <int D>
__host__ __device__ inline double pl_cost_at(const double *g, const double *qq, const double *aa, double r, double w) {
#pragma clang fp contract(off)
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) v = fma(g[i * D + k], qq[k], v);
    const double p = (v + g[D * D + i]) - aa[i];
    n2 = fma(p, p, n2);
  }
  const double e = sqrt(n2) - r;
  return (w * e) * e;
}
// The polish of a valid hypothesis: kPlHypSteps Gauss-Newton steps from g on the sample's own entries.  entry(k, &q, &a, &r,
// &w) gives entry k of the sample: the rows of its position and anchor, its range and precision.
template <int D, class Entry>
__host__ __device__ inline void pl_hyp_polish(double sw, double L, const double *q0, const double *a0, Entry entry, double *g) {
#pragma clang fp contract(off)
  constexpr int NS = kPlGnSums(D);
  for (int step = 0; step < kPlHypSteps; ++step) {
    double S[NS], t[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = 0.0;
    for (int k = 0; k < kPlTerms(D); ++k) {
      const double *q, *a;
      double r, w;
      entry(k, &q, &a, &r, &w);
      pl_gn_terms<D>(g, L, q0, a0, q, a, r, w, t);
#pragma unroll
      for (int i = 0; i < NS; ++i) S[i] = S[i] + t[i];
    }
    if (!pl_gn_step<D>(S, sw, L, g)) return;
  }
}
// The hypothesis from the pair sums S of its sample (kPlSums(D)): the linear solve, then the polish.  Returns whether it is
// valid; g = the identity where it is not.  work: kPlUnknowns(D) (kPlUnknowns(D) + 1) doubles.
template <int D, class Entry>
__host__ __device__ inline bool pl_hypothesis(const double *S, double *work, const double *q0, const double *a0, Entry entry, double *g) {
  double L, sw;
  if (pl_linear_solve<D>(S, work, g, &L, &sw) != 0) {
    pl_identity<D>(q0, a0, g);
    return false;
  }
  pl_hyp_polish<D>(sw, L, q0, a0, entry, g);
  return true;
}
// What the folds of a masked stage do: a stage the election left at status 5 keeps the identity, takes no step and writes the
// identity; every other stage is the plain fold's.
template <int D>
__host__ __device__ inline bool pl_fold_linear_robust(const double *S, double *work, double *st, int32_t *ist, const double *q0, const double *a0) {
  if (ist[0] != 5) return pl_fold_linear<D>(S, work, st, ist, q0, a0);
  constexpr int G = kPlG(D);
  for (int i = 0; i < kPlState(D); ++i) st[i] = 0.0;
  pl_identity<D>(q0, a0, st);
  pl_identity<D>(q0, a0, st + G);
  st[3 * G + 4] = 1.0;
  ist[1] = -1;
  ist[2] = 0;
  ist[3] = 0;
  return true;
}
template <int D>
__host__ __device__ inline bool pl_fold_gn_robust(int step, int last, const double *S, double *st, int32_t *ist, const double *q0, const double *a0) {
  if (ist[0] != 5) return pl_fold_gn<D>(step, last, S, st, ist, q0, a0);
  if (last)
    for (int i = 0; i < kPlG(D); ++i) st[2 * kPlG(D) + i] = i < D * D && i / D == i % D ? 1.0 : 0.0;
  return true;
}

// Placement from pose-landmark sightings (kernels/sighting.inc; include/cora_hip.h, cora_place_by_sightings_dev).  A
// sighting is an edge without a second rotation from a position of an odometry chain to a landmark: its prediction is
// p = x_t(a) + sum_c t_c X_a[c, :].  The host orders the work into STAGES (capi/sighting.inc) of three kinds: an L-stage
// sets landmarks to the weighted mean of their predictions, a C-stage moves chains by the weighted rigid alignment of their
// predictions onto the landmarks, the REFIT sets the landmarks again.  A stage holds LISTS (one per landmark or chain) of
// entries (first rotation row and translation row of the pose, row of the landmark, edge), cut into chunks of kSgChunk
// entries, none across two lists; ALL lists of a stage share its launches:
//   L-stage, REFIT : pass (mode 0: sum tau | tau (p - p_0)) and fold (one wavefront per list; writes the landmark's row)
//   C-stage        : pass and fold of the alignment's sums (mode 1), pass and fold of the two costs (mode 2), apply
//   after the REFIT: pass and fold of the landmarks' cost (mode 3)
// Coordinates are relative to the list's first entry: p' = p - p_0, l' = x_t(l) - l_0.
// BRACKET ORDER, a function of the list length and kSgChunk alone and the same in the host mirror (capi/sighting.inc):
// as the multilateration's -- butterfly per wavefront, lanes without an entry hold +0.0, the four wavefronts of a chunk from
// the left; fold: lane j takes 0.0 + chunk j + chunk (j + 64) + .. of the list from the left, then the butterfly.
// Every term is made of single correctly rounded fp64 operations in the order written, never contracted.
constexpr int kSgChunk = 256;
constexpr double kSgMinSpread = 1e-6;  // the refusal rule of sg_chain_solve, in units of length
constexpr int kSgLmSums(int d) { return 1 + d; }                   // sum tau | tau (p - p_0)
constexpr int kSgChainSums(int d) { return 3 + 2 * d + d * d; }    // tau | tau p' | tau l' | tau l' p'^T (row-major) | tau |p'|^2 | tau |l'|^2
constexpr int kSgCostSums = 2;                                     // at the identity | at g
constexpr int kSgMaxSums(int d) { return kSgChainSums(d); }
constexpr int kSgG(int d) { return d * d + d; }                    // R row-major | translation
// a chain's list: R | t | t' = R p_0 + t - l_0 | cost_start | cost_final;  a landmark's: x | sum tau | cost
constexpr int kSgState(int d) { return kSgG(d) + d + 2; }
constexpr int kSgInts = 2;  // status | chosen
struct SgArgs {
  int d = 0, mode = 0;
  int32_t chunk0 = 0, n_chunks = 0;   // the stage's chunks in the chunk table
  int32_t list0 = 0, n_lists = 0;     // the stage's lists in the list table
  int32_t apply0 = 0, n_apply = 0;    // the positions of the stage's chains in the apply table
  int64_t n_edges = 0, pstride = 0;
  const int32_t *chunk_begin = nullptr, *chunk_len = nullptr, *chunk_list = nullptr;  // [chunks of all stages]
  const int32_t *list_chunk0 = nullptr, *list_row = nullptr;  // [lists + 1], [lists]: the landmark's INTERNAL row (a chain's list: -1)
  const int32_t *ent_rot = nullptr, *ent_trn = nullptr, *ent_lm = nullptr, *ent_e = nullptr;  // [entries]: INTERNAL rows, edge
  const int32_t *apply_pos = nullptr, *apply_list = nullptr;  // [positions of all C-stages]: chain-table position, its list
  const int32_t *pos_rot = nullptr, *pos_trn = nullptr;       // the chain tables' (OdomArgs)
  const double *edge_data = nullptr;   // the measurement table's, [d*d + d + 2][n_edges]
  double *partial = nullptr;           // [kSgMaxSums(d)][pstride], pstride = the chunks of all stages
  double *state = nullptr;             // [lists][kSgState(d)]
  int32_t *istate = nullptr;           // [lists][kSgInts]
  double *x = nullptr;                 // d columns at stride ld_for(d) = d
  int *flag = nullptr;                 // |= 1 where a sum is not finite
};
hipError_t launch_sighting_pass_fold(const SgArgs &A, hipStream_t st);  // pass and fold of A.mode over the stage A describes
hipError_t launch_sighting_apply(const SgArgs &A, hipStream_t st);
// p = x_t(a) + sum_c t_c X_a[c, :]  (from x_t(a), c ascending, one fma per term)
template <int D>
__host__ __device__ inline void sg_predict(const double *rot, const double *trn, const double *t, double *p) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double v = trn[k];
#pragma unroll
    for (int c = 0; c < D; ++c) v = fma(t[c], rot[c * D + k], v);
    p[k] = v;
  }
}
template <int D>
__host__ __device__ inline void sg_lm_terms(const double *p0, const double *p, double tau, double *s) {
#pragma clang fp contract(off)
  s[0] = tau;
#pragma unroll
  for (int c = 0; c < D; ++c) s[1 + c] = tau * (p[c] - p0[c]);
}
// x = p_0 + (sum tau (p - p_0)) / sum tau; status 0, or 2 (x untouched) where sum tau <= 0 (or is not a number)
template <int D>
__host__ __device__ inline int sg_lm_solve(const double *S, const double *p0, double *x) {
#pragma clang fp contract(off)
  if (!(S[0] > 0.0)) return 2;
#pragma unroll
  for (int c = 0; c < D; ++c) x[c] = p0[c] + S[1 + c] / S[0];
  return 0;
}
// tau |x_t(l) - p|^2, the table's own translation residual of the edge (from +0.0, c ascending)
template <int D>
__host__ __device__ inline double sg_lm_cost(const double *p, const double *l, double tau) {
#pragma clang fp contract(off)
  double q = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const double r = l[c] - p[c];
    q = fma(r, r, q);
  }
  return tau * q;
}
template <int D>
__host__ __device__ inline void sg_chain_terms(const double *p0, const double *l0, const double *p, const double *l, double tau, double *s) {
#pragma clang fp contract(off)
  double pp[D], ll[D], np = 0.0, nl = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    pp[c] = p[c] - p0[c];
    ll[c] = l[c] - l0[c];
    np = fma(pp[c], pp[c], np);
    nl = fma(ll[c], ll[c], nl);
  }
  s[0] = tau;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    s[1 + c] = tau * pp[c];
    s[1 + D + c] = tau * ll[c];
  }
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) s[1 + 2 * D + a * D + b] = (tau * ll[a]) * pp[b];
  s[1 + 2 * D + D * D] = tau * np;
  s[2 + 2 * D + D * D] = tau * nl;
}
// The weighted rigid alignment from the sums: H = sum tau l' p'^T - (sum tau l')(sum tau p')^T / sum tau, R =
// round_rotation(H), t' = lbar - R pbar with the relative centroids, t = t' + l_0 - R p_0.  g: R | t | t'.
// REFUSED (status 2, g = the identity with t' = p_0 - l_0), a function of the sums alone, with W = sum tau,
// s_p = sum tau |p'|^2 - |sum tau p'|^2 / W and s_l likewise (the two centred spreads), k = kSgMinSpread:
//   W <= 0, s_p <= 0 or s_l <= 0 (no spread), or
//   d = 2:  |H|_F^2 <= k^2 s_p s_l                   (H = 0: no direction at all)
//   d = 3:  |cof(H)|_F^2 <= k^4 (s_p s_l)^2          (the sum of the squared 2 x 2 minors: rank below 2)
// (every comparison written so that a NaN refuses).  With singular values s_1 >= s_2 >= s_3 of H these read
// s_1^2 + s_2^2 <= k^2 s_p s_l and s_1^2 s_2^2 + s_1^2 s_3^2 + s_2^2 s_3^2 <= k^4 (s_p s_l)^2.
template <int D>
__host__ __device__ inline int sg_chain_solve(const double *S, const double *p0, const double *l0, double *g) {
#pragma clang fp contract(off)
  constexpr int G = kSgG(D);
  const double *Sp = S + 1, *Sl = S + 1 + D, *Slp = S + 1 + 2 * D;
  const double W = S[0];
#pragma unroll
  for (int i = 0; i < D * D; ++i) g[i] = i / D == i % D ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    g[D * D + c] = 0.0;
    g[G + c] = p0[c] - l0[c];
  }
  if (!(W > 0.0)) return 2;
  double H[D][D], np = 0.0, nl = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    np = fma(Sp[c], Sp[c], np);
    nl = fma(Sl[c], Sl[c], nl);
  }
  const double sp = S[1 + 2 * D + D * D] - np / W, sl = S[2 + 2 * D + D * D] - nl / W;
  if (!(sp > 0.0) || !(sl > 0.0)) return 2;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) H[a][b] = Slp[a * D + b] - (Sl[a] * Sp[b]) / W;
  const double scale = sp * sl, k2 = kSgMinSpread * kSgMinSpread;
  if constexpr (D == 2) {
    const double f = fma(H[1][1], H[1][1], fma(H[1][0], H[1][0], fma(H[0][1], H[0][1], H[0][0] * H[0][0])));
    if (!(f > k2 * scale)) return 2;
  } else {
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        const double m = fma(H[a1][b1], H[a2][b2], -(H[a1][b2] * H[a2][b1]));
        q = fma(m, m, q);
      }
    if (!(q > (k2 * scale) * (k2 * scale))) return 2;
  }
  round_rotation<D>(H);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) g[a * D + b] = H[a][b];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double rp = 0.0, r0 = 0.0;  // R pbar, R p_0 (from +0.0, k ascending)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      rp = fma(H[a][k], Sp[k] / W, rp);
      r0 = fma(H[a][k], p0[k], r0);
    }
    const double tr = Sl[a] / W - rp;
    g[G + a] = tr;
    g[D * D + a] = (tr + l0[a]) - r0;
  }
  return 0;
}
// the cost of one entry at g from its relative coordinates p' = p - p_0, l' = l - l_0: tau |R p' + t' - l'|^2
template <int D>
__host__ __device__ inline double sg_cost_rel(const double *g, const double *pp, const double *ll, double tau) {
#pragma clang fp contract(off)
  constexpr int G = kSgG(D);
  double q = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double v = g[G + a];
#pragma unroll
    for (int k = 0; k < D; ++k) v = fma(g[a * D + k], pp[k], v);
    const double r = v - ll[a];
    q = fma(r, r, q);
  }
  return tau * q;
}
// the two costs of one entry: at the identity, tau |x_t(l) - p|^2 as the table has it; at g, sg_cost_rel at p' and l'
template <int D>
__host__ __device__ inline void sg_cost_terms(const double *g, const double *p0, const double *l0, const double *p, const double *l, double tau,
                                              double *s) {
#pragma clang fp contract(off)
  s[0] = sg_lm_cost<D>(p, l, tau);
  double pp[D], ll[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    pp[c] = p[c] - p0[c];
    ll[c] = l[c] - l0[c];
  }
  s[1] = sg_cost_rel<D>(g, pp, ll, tau);
}
// what lane 0 of a list's fold does with the list's sums S in mode MODE; row: the landmark's row of x (modes 0 and 3);
// p0, l0: the first entry's prediction and landmark.  False where a sum is not finite.
template <int D, int MODE>
__host__ __device__ inline bool sg_fold(const double *S, double *st, int32_t *ist, const double *p0, const double *l0, double *row) {
  constexpr int G = kSgG(D);
  constexpr int ns = MODE == 0 ? kSgLmSums(D) : (MODE == 1 ? kSgChainSums(D) : (MODE == 2 ? kSgCostSums : 1));
  bool finite = odom_finite(S, ns);
  if constexpr (MODE == 0) {
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = row[c];
    ist[0] = finite ? sg_lm_solve<D>(S, p0, x) : 2;
    ist[1] = ist[0] == 0 ? 1 : 0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      st[c] = x[c];
      if (ist[0] == 0) row[c] = x[c];
    }
    st[D] = S[0];
    st[D + 1] = 0.0;
  } else if constexpr (MODE == 1) {
    double g[G + D];
    ist[0] = sg_chain_solve<D>(S, p0, l0, g);  // (sums that are not finite: the call fails, whatever g is)
    ist[1] = 0;
#pragma unroll
    for (int i = 0; i < G + D; ++i) st[i] = g[i];
    finite = finite && odom_finite(g, G + D);
  } else if constexpr (MODE == 2) {
    ist[1] = ist[0] == 0 && S[1] < S[0] ? 1 : 0;
    st[G + D] = S[0];
    st[G + D + 1] = ist[1] ? S[1] : S[0];  // the cost of what is applied
  } else {
    st[D + 1] = S[0];
  }
  return finite;
}

// Placement from inter-chain relative-pose edges (kernels/closure.inc; include/cora_hip.h, cora_place_by_closures_dev).  A
// CLOSURE is an edge with a second rotation that is no edge of an odometry chain and whose two poses are positions of two
// different chains.  Against a placed chain its two residuals are functions of the motion g = (G, s) of the other chain:
// kappa |G - P|_F^2 + tau |G q + s - l|^2, with (dir 0: a placed, b moves) P = X_a^T R X_b, q = x_t(b), l = x_t(a) + R_a t
// and (dir 1: a moves, b placed) P = X_b^T R^T X_a, q = x_t(a) + R_a t, l = x_t(b): the two P are transposes of each other.
// The host orders the chains into STAGES (capi/closure.inc); a stage holds one LIST per chain taken in it (its closures
// against chains placed before the stage, in table order: edge and dir), cut into chunks of kClChunk entries, none across
// two lists; ALL lists of a stage share its five launches:
//   pass and fold of the sums (mode 0; the fold solves, cl_solve), pass and fold of the two costs (mode 1), apply.
// The lists' state has the layout of the sighting placement's chain lists (kSgState, kSgInts), so the apply is k_sg_apply.
// Coordinates are relative to the list's first entry: q' = q - q_0, l' = l - l_0.  BRACKET ORDER and arithmetic: as the
// sighting placement's (above), the same in the host mirror (capi/closure.inc).
constexpr int kClChunk = 256;
// the chunk of the four placement initialisers: their passes end in one chunk sum (kernels/common.inc), their table builders cut
// lists with one function and their mirrors sum with one (capi/init_common.inc)
constexpr int kSumChunk = 256;
static_assert(kMlChunk == kSumChunk && kPlChunk == kSumChunk && kSgChunk == kSumChunk && kClChunk == kSumChunk, "one chunk size");
constexpr double kClMinRank = 1e-6;  // the refusal rule of cl_solve, relative to the bound S of |H|_F
// tau | tau q' | tau l' | tau l' q'^T (row-major) | tau |q'|^2 | tau |l'|^2 (sg_chain_terms' layout) | kappa | kappa P (row-major)
constexpr int kClSums(int d) { return 4 + 2 * d + 2 * d * d; }
constexpr int kClCostSums = 2;  // at the identity (the table's own rot + trans residuals) | at g
struct ClArgs {
  int d = 0, mode = 0;
  int32_t chunk0 = 0, n_chunks = 0;   // the stage's chunks in the chunk table
  int32_t list0 = 0, n_lists = 0;     // the stage's lists in the list table
  int32_t apply0 = 0, n_apply = 0;    // the positions of the stage's chains in the apply table
  int64_t n_edges = 0, pstride = 0;
  const int32_t *chunk_begin = nullptr, *chunk_len = nullptr, *chunk_list = nullptr;  // [chunks of all stages]
  const int32_t *list_chunk0 = nullptr;                      // [lists + 1]
  const int32_t *ent_e = nullptr, *ent_dir = nullptr;        // [entries]: edge, 0 a placed and b moves | 1 a moves and b placed
  const int32_t *apply_pos = nullptr, *apply_list = nullptr;  // [positions of all stages]: chain-table position, its list
  const int32_t *pos_rot = nullptr, *pos_trn = nullptr;       // the chain tables' (OdomArgs)
  const int32_t *edge_rows = nullptr;  // the measurement table's, [ra | rb | ta | tb][n_edges], INTERNAL rows
  const double *edge_data = nullptr;   // the measurement table's, [d*d + d + 2][n_edges]
  double *partial = nullptr;           // [kClSums(d)][pstride], pstride = the chunks of all stages
  double *state = nullptr;             // [lists][kSgState(d)]: G | s | s' | cost_start | cost_final
  int32_t *istate = nullptr;           // [lists][kSgInts]: status | chosen
  double *x = nullptr;                 // d columns at stride ld_for(d) = d
  int *flag = nullptr;                 // |= 1 where a sum is not finite
};
hipError_t launch_closure_pass_fold(const ClArgs &A, hipStream_t st);  // pass and fold of A.mode over the stage A describes
hipError_t launch_closure_apply(const ClArgs &A, hipStream_t st);     // k_sg_apply over the stage's positions
// One entry from the rows as they stand: Y = R^T X_a (Y[b][k] from +0.0, a ascending), P (dir 0: P[i][j] = sum_b Y[b][i]
// X_b[b][j] from +0.0, b ascending; dir 1: its transpose), q and l, the table's own residuals res = kappa |X_b - Y|_F^2 +
// tau |x_t(b) - (x_t(a) + R_a t)|^2 (each from +0.0, row-major resp. c ascending).  f: the edge's fields R | t | kappa | tau.
template <int D>
__host__ __device__ inline void cl_entry(const double *xa, const double *ta, const double *xb, const double *tb, const double *f, int dir,
                                         double *P, double *q, double *l, double *res) {
#pragma clang fp contract(off)
  double Y[D * D], pa[D];
#pragma unroll
  for (int b = 0; b < D; ++b)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) v = fma(f[a * D + b], xa[a * D + k], v);
      Y[b * D + k] = v;
    }
  double rot = 0.0;
#pragma unroll
  for (int i = 0; i < D * D; ++i) {
    const double r = xb[i] - Y[i];
    rot = fma(r, r, rot);
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double v = 0.0;
#pragma unroll
      for (int b = 0; b < D; ++b) v = fma(Y[b * D + i], xb[b * D + j], v);
      P[dir ? j * D + i : i * D + j] = v;
    }
  sg_predict<D>(xa, ta, f + D * D, pa);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    q[c] = dir ? pa[c] : tb[c];
    l[c] = dir ? tb[c] : pa[c];
  }
  res[0] = f[D * D + D] * rot + sg_lm_cost<D>(pa, tb, f[D * D + D + 1]);
}
// the entry's terms of the sums (kClSums): sg_chain_terms' with p = q, then kappa and kappa P
template <int D>
__host__ __device__ inline void cl_terms(const double *q0, const double *l0, const double *P, const double *q, const double *l, double kappa,
                                         double tau, double *s) {
#pragma clang fp contract(off)
  sg_chain_terms<D>(q0, l0, q, l, tau, s);
  s[3 + 2 * D + D * D] = kappa;
#pragma unroll
  for (int i = 0; i < D * D; ++i) s[4 + 2 * D + D * D + i] = kappa * P[i];
}
// The minimiser of the list's closure cost from its sums, with W = sum tau, K = sum kappa: H = sum kappa P + [W > 0: sum tau
// l' q'^T - (sum tau l')(sum tau q')^T / W], G = round_rotation(H), s' = [W > 0: (sum tau l') / W - G (sum tau q') / W, else
// 0], s = s' + l_0 - G q_0.  g: G | s | s'.
// REFUSED (status 2, g = the identity with s' = q_0 - l_0), a function of the sums alone, with the centred spreads s_q = sum
// tau |q'|^2 - |sum tau q'|^2 / W and s_l likewise (0 where W <= 0), S = K sqrt(d) + sqrt(max(s_q, 0) max(s_l, 0)) (an upper
// bound of |H|_F) and k = kClMinRank:
//   K <= 0 and W <= 0;  K <= 0 and (s_q <= 0 or s_l <= 0);
//   d = 2:  |H|_F^2 <= k^2 S^2;      d = 3:  |cof(H)|_F^2 <= k^4 S^4
// (every comparison written so that a NaN refuses).
template <int D>
__host__ __device__ inline int cl_solve(const double *S, const double *q0, const double *l0, double *g) {
#pragma clang fp contract(off)
  constexpr int G = kSgG(D);
  const double *Sq = S + 1, *Sl = S + 1 + D, *Slq = S + 1 + 2 * D, *SP = S + 4 + 2 * D + D * D;
  const double W = S[0], K = S[3 + 2 * D + D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) g[i] = i / D == i % D ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    g[D * D + c] = 0.0;
    g[G + c] = q0[c] - l0[c];
  }
  const bool hasW = W > 0.0, hasK = K > 0.0;
  if (!hasW && !hasK) return 2;
  double sq = 0.0, sl = 0.0;
  if (hasW) {
    double nq = 0.0, nl = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      nq = fma(Sq[c], Sq[c], nq);
      nl = fma(Sl[c], Sl[c], nl);
    }
    sq = S[1 + 2 * D + D * D] - nq / W;
    sl = S[2 + 2 * D + D * D] - nl / W;
  }
  if (!hasK && (!(sq > 0.0) || !(sl > 0.0))) return 2;
  double H[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) H[a][b] = hasW ? SP[a * D + b] + (Slq[a * D + b] - (Sl[a] * Sq[b]) / W) : SP[a * D + b];
  const double root_d = D == 2 ? 1.4142135623730951 : 1.7320508075688772;  // sqrt(d), correctly rounded
  const double bound = (hasK ? K * root_d : 0.0) + sqrt((sq > 0.0 ? sq : 0.0) * (sl > 0.0 ? sl : 0.0));
  const double k2 = kClMinRank * kClMinRank, b2 = bound * bound;
  if constexpr (D == 2) {
    const double f = fma(H[1][1], H[1][1], fma(H[1][0], H[1][0], fma(H[0][1], H[0][1], H[0][0] * H[0][0])));
    if (!(f > k2 * b2)) return 2;
  } else {
    double m2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2i = (b + 2) % 3;
        const double m = fma(H[a1][b1], H[a2][b2i], -(H[a1][b2i] * H[a2][b1]));
        m2 = fma(m, m, m2);
      }
    if (!(m2 > (k2 * b2) * (k2 * b2))) return 2;
  }
  round_rotation<D>(H);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) g[a * D + b] = H[a][b];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double rq = 0.0, r0 = 0.0;  // G qbar, G q_0 (from +0.0, k ascending)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (hasW) rq = fma(H[a][k], Sq[k] / W, rq);
      r0 = fma(H[a][k], q0[k], r0);
    }
    const double tr = hasW ? Sl[a] / W - rq : 0.0;
    g[G + a] = tr;
    g[D * D + a] = (tr + l0[a]) - r0;
  }
  return 0;
}
// the cost of one entry at g from its relative coordinates q' = q - q_0, l' = l - l_0: kappa |G - P|_F^2 (from +0.0,
// row-major) + tau |G q' + s' - l'|^2
template <int D>
__host__ __device__ inline double cl_cost_rel(const double *g, const double *P, const double *qq, const double *ll, double kappa, double tau) {
#pragma clang fp contract(off)
  constexpr int G = kSgG(D);
  double rot = 0.0, trn = 0.0;
#pragma unroll
  for (int i = 0; i < D * D; ++i) {
    const double r = g[i] - P[i];
    rot = fma(r, r, rot);
  }
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double v = g[G + a];
#pragma unroll
    for (int k = 0; k < D; ++k) v = fma(g[a * D + k], qq[k], v);
    const double r = v - ll[a];
    trn = fma(r, r, trn);
  }
  return kappa * rot + tau * trn;
}
// the cost of one entry at g: cl_cost_rel at q' = q - q_0, l' = l - l_0 (the same operations in the same order)
template <int D>
__host__ __device__ inline double cl_cost_at(const double *g, const double *q0, const double *l0, const double *P, const double *q, const double *l,
                                             double kappa, double tau) {
#pragma clang fp contract(off)
  double qq[D], ll[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    qq[c] = q[c] - q0[c];
    ll[c] = l[c] - l0[c];
  }
  return cl_cost_rel<D>(g, P, qq, ll, kappa, tau);
}
// what lane 0 of a list's fold does with the list's sums S in mode MODE (0 solve, 1 costs); q0, l0: the first entry's.
// False where a sum is not finite.
template <int D, int MODE>
__host__ __device__ inline bool cl_fold(const double *S, double *st, int32_t *ist, const double *q0, const double *l0) {
  constexpr int G = kSgG(D);
  bool finite = odom_finite(S, MODE == 0 ? kClSums(D) : kClCostSums);
  if constexpr (MODE == 0) {
    double g[G + D];
    ist[0] = cl_solve<D>(S, q0, l0, g);  // (sums that are not finite: the call fails, whatever g is)
    ist[1] = 0;
#pragma unroll
    for (int i = 0; i < G + D; ++i) st[i] = g[i];
    finite = finite && odom_finite(g, G + D);
  } else {
    ist[1] = ist[0] == 0 && S[1] < S[0] ? 1 : 0;
    st[G + D] = S[0];
    st[G + D + 1] = ist[1] ? S[1] : S[0];  // the cost of what is applied
  }
  return finite;
}

// Outlier-robust placement from closures: a consensus vote over minimal hypotheses (kernels/closure.inc; include/cora_hip.h,
// cora_place_by_closures_robust_dev).  Tables, stages, lists and chunks are the plain placement's.  Every entry h
// of a list with kappa_h > 0 proposes the motion g_h its one edge determines (cl_hypothesis); every entry j is scored under
// every proposal, r(h, j) = cl_cost_at(g_h, .., entry j); vote(h) = #{j : r(h, j) <= barc2} (cl_agrees: a NaN is no vote; an
// invalid h has vote 0).  Elected: the largest vote, among equal votes the lowest entry (cl_better); consensus = its vote;
// consensus < min_consensus: status 5, the chain keeps its rows.  I = {j : r(h*, j) <= barc2}; the sums and the two costs of
// the plain placement run over I alone: AN ENTRY OUTSIDE I ADDS +0.0 FOR EACH OF ITS TERMS, exactly as a lane beyond the
// chunk's end does, so the bracket order of a sum is the plain placement's.  Seven launches per stage:
//   vote, elect, pass and fold of the sums over I, pass and fold of the two costs over I, apply.
constexpr int kClCState(int d) { return kSgG(d) + d; }  // of the elected hypothesis: G | s | s'
constexpr int kClCInts = 2;                             // elected entry (index in its list) | consensus
struct ClRobustArgs {
  ClArgs A;
  double barc2 = 0.0;
  int min_consensus = 0;
  int32_t *votes = nullptr;         // [entries]
  double *cstate = nullptr;         // [lists][kClCState(d)]
  int32_t *cint = nullptr;          // [lists][kClCInts]
  unsigned char *inlier = nullptr;  // [n_edges]: written where an edge is an entry, 1 in I | 0 outside
};
hipError_t launch_closure_vote_elect(const ClRobustArgs &R, hipStream_t st);      // k_cl_vote and k_cl_elect over the stage
hipError_t launch_closure_robust_pass_fold(const ClRobustArgs &R, hipStream_t st);  // masked pass and fold of R.A.mode
// The motion entry h proposes: G = P as cl_entry produced it, s'[a] = (l[a] - l_0[a]) - sum_k G[a][k] (q[k] - q_0[k]) (the sum
// from +0.0, k ascending), s = (s' + l_0) - G q_0 as cl_solve writes it.  g: G | s | s'.
template <int D>
__host__ __device__ inline void cl_hypothesis(const double *q0, const double *l0, const double *P, const double *q, const double *l, double *g) {
#pragma clang fp contract(off)
  constexpr int G = kSgG(D);
  double qq[D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) g[i] = P[i];
#pragma unroll
  for (int c = 0; c < D; ++c) qq[c] = q[c] - q0[c];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double rq = 0.0, r0 = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      rq = fma(P[a * D + k], qq[k], rq);
      r0 = fma(P[a * D + k], q0[k], r0);
    }
    const double tr = (l[a] - l0[a]) - rq;
    g[G + a] = tr;
    g[D * D + a] = (tr + l0[a]) - r0;
  }
}
__host__ __device__ inline bool cl_agrees(double r, double barc2) { return r <= barc2; }  // (a NaN is no vote)
// the election's order: (vote, entry) beats (v, e)
__host__ __device__ inline bool cl_better(int32_t vote, int32_t entry, int32_t v, int32_t e) { return vote > v || (vote == v && entry < e); }
// cl_fold with status 5 passed through: a list without consensus has the identity (as a refused one) and is never chosen
template <int D, int MODE>
__host__ __device__ inline bool cl_fold_robust(const double *S, double *st, int32_t *ist, const double *q0, const double *l0) {
  constexpr int G = kSgG(D);
  if (ist[0] != 5) return cl_fold<D, MODE>(S, st, ist, q0, l0);
  const bool finite = odom_finite(S, MODE == 0 ? kClSums(D) : kClCostSums);
  if constexpr (MODE == 0) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) st[i] = i / D == i % D ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      st[D * D + c] = 0.0;
      st[G + c] = q0[c] - l0[c];
    }
    ist[1] = 0;
  } else {
    ist[1] = 0;
    st[G + D] = S[0];
    st[G + D + 1] = S[0];
  }
  return finite;
}

// Outlier-robust placement from sightings: a consensus vote in front of every closed-form fit (kernels/sighting.inc;
// include/cora_hip.h, cora_place_by_sightings_robust_dev).  Tables, stages, lists, chunks and the origin (the list's
// first entry, inlier or not) are the plain placement's.
//   landmark list: entry h proposes y_h = p'_h; r(h, j) = sg_lm_cost(p'_j, y_h, tau_j) = tau_j |y_h - p'_j|^2.
//   chain list of L entries: entry h proposes the plain chain solve of its SAMPLE, the d entries (h + k s) mod L, k = 0 .. d - 1,
//     s = max(1, L / d) (sg_sample_entry; distinct, since L >= d), their sg_chain_terms added from the left to +0.0
//     (sg_hypothesis); VALID where the solve is not refused and g is finite; r(h, j) = sg_cost_rel(g_h, p'_j, l'_j, tau_j).
// vote(h) = #{j : r(h, j) <= barc2} (cl_agrees: a NaN is no vote; an invalid h has vote 0 and sets no flag).  Elected: the
// largest vote, among equal votes the lowest entry (cl_better); consensus = its vote; a list without a valid hypothesis elects
// entry 0 with consensus 0.  consensus below the minimum of the list's kind: status 5, the rows are not touched.  I = {j :
// r(h*, j) <= barc2}; the plain sums and costs run over I alone: AN ENTRY OUTSIDE I ADDS +0.0 FOR EACH OF ITS TERMS, exactly as
// a lane beyond the chunk's end does, so the bracket order of a sum is the plain placement's and a list without an outlier has
// the plain call's bits.  Launches per stage:
//   L-stage 4: vote, elect, masked pass and fold (mode 0);  REFIT 6: these and the masked pass and fold of the cost (mode 3);
//   C-stage 8: hypotheses, vote, elect, masked pass and fold of the sums (mode 1) and of the two costs (mode 2), apply.
// The chain hypotheses are computed in a launch of their own into a workspace (hyp) the vote reads: the one-sided Jacobi of
// the solve does not share registers with the vote's inner loop.
constexpr int kSgCState(int d) { return kSgG(d) + d; }  // of the elected hypothesis: chain R | t | t'; landmark y (the first d)
constexpr int kSgCInts = 2;                             // elected entry (index in its list) | consensus
struct SgRobustArgs {
  SgArgs A;
  double barc2 = 0.0;
  int min_chain_consensus = 0, min_landmark_consensus = 0;
  int32_t *votes = nullptr;         // [entries]; between k_sg_hyp and k_sg_vote of a C-stage: 0 valid | -1 invalid
  double *hyp = nullptr;            // [kSgCState(d)][hstride]: the chain hypothesis of every entry
  int64_t hstride = 0;              // the entries of all lists
  double *cstate = nullptr;         // [lists][kSgCState(d)]
  int32_t *cint = nullptr;          // [lists][kSgCInts]
  unsigned char *inlier_chain = nullptr;     // [n_edges]: written where an edge is an entry of a C-stage list, 1 in I | 0 outside
  unsigned char *inlier_landmark = nullptr;  // [n_edges]: the same for the landmark lists (the REFIT's pass writes last)
};
hipError_t launch_sighting_vote_elect(const SgRobustArgs &R, int kind, hipStream_t st);  // kind 0 landmark lists | 1 chain lists (with k_sg_hyp)
hipError_t launch_sighting_robust_pass_fold(const SgRobustArgs &R, hipStream_t st);       // masked pass and fold of R.A.mode
// entry k of the sample of entry h in a list of len entries
__host__ __device__ inline int32_t sg_sample_entry(int32_t h, int32_t len, int d, int k) {
  const int64_t s = len / d > 1 ? len / d : 1;
  return static_cast<int32_t>((static_cast<int64_t>(h) + k * s) % len);
}
// The motion entry h of a list of len entries proposes.  entry(j, p, &l) gives prediction, landmark row and tau of entry j of
// the list; p0, l0: the first entry's.  g: R | t | t'.  True where the hypothesis is valid.
template <int D, class Entry>
__host__ __device__ inline bool sg_hypothesis(int32_t h, int32_t len, const double *p0, const double *l0, Entry entry, double *g) {
#pragma clang fp contract(off)
  constexpr int NS = kSgChainSums(D);
  double S[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) S[i] = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double p[D], t[NS];
    const double *l;
    const double tau = entry(sg_sample_entry(h, len, D, k), p, &l);
    sg_chain_terms<D>(p0, l0, p, l, tau, t);
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = S[i] + t[i];
  }
  return sg_chain_solve<D>(S, p0, l0, g) == 0 && odom_finite(g, kSgCState(D));
}
// sg_fold with status 5 passed through: a list without consensus writes no row, has the identity and is never chosen
template <int D, int MODE>
__host__ __device__ inline bool sg_fold_robust(const double *S, double *st, int32_t *ist, const double *p0, const double *l0, double *row) {
  constexpr int G = kSgG(D);
  constexpr int ns = MODE == 0 ? kSgLmSums(D) : (MODE == 1 ? kSgChainSums(D) : (MODE == 2 ? kSgCostSums : 1));
  if (ist[0] != 5) return sg_fold<D, MODE>(S, st, ist, p0, l0, row);
  const bool finite = odom_finite(S, ns);
  ist[1] = 0;
  if constexpr (MODE == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) st[c] = row[c];
    st[D] = S[0];
    st[D + 1] = 0.0;
  } else if constexpr (MODE == 1) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) st[i] = i / D == i % D ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      st[D * D + c] = 0.0;
      st[G + c] = p0[c] - l0[c];
    }
  } else if constexpr (MODE == 2) {
    st[G + D] = S[0];
    st[G + D + 1] = S[0];
  } else {
    st[D + 1] = S[0];
  }
  return finite;
}

// In-place update of Q's values (kernels/update_values.inc).  src: the sources of ValueMap (cora_internal.h), vals: the
// new CSR values on the device.
// check: flag |= 1 where a value is not finite, |= 2 where a mirror pair (mirror[2j], mirror[2j + 1]) differs.
hipError_t launch_values_check(int64_t nnz, const double *vals, int64_t n_pairs, const int32_t *mirror, int *flag,
                               hipStream_t st);
// dst[i] = vals[src[i]] (0 without a source);  reciprocal: dst[i] = 1 / that
hipError_t launch_values_gather(int64_t n, const int32_t *src, const double *vals, double *dst, bool reciprocal,
                                hipStream_t st);
// dst0[i] = dst1[i] = 0.5 * (vals[src[2i]] + vals[src[2i + 1]])
hipError_t launch_values_gather_sym(int64_t n, const int32_t *src, const double *vals, double *dst0, double *dst1,
                                    hipStream_t st);

// Assembly of Q(w) from per-measurement weights (kernels/assemble.inc): the device copy of a TermMap (cora_internal.h).
struct AssembleArgs {
  int64_t nnz = 0;
  int n_long = 0;
  const int32_t *tptr = nullptr, *tweight = nullptr, *long_entries = nullptr;
  const double *tcoef = nullptr;
};
// flag |= 1 where a weight is negative or not finite
hipError_t launch_weights_check(int64_t n, const double *w, int *flag, hipStream_t st);
// vals[q] = sum of tcoef[t] * w[tweight[t]] over the terms of entry q (order: TermMap); vals: 16-byte aligned
hipError_t launch_assemble(const AssembleArgs &A, const double *w, double *vals, hipStream_t st);
// dst[i] = base[i] * w[i]
hipError_t launch_scale_precisions(int64_t n, const double *base, const double *w, double *dst, hipStream_t st);

}  // namespace cora
