// HIP kernels for the CORA hot path on gfx950 (CDNA4, wave64).
//
// All resident vectors are row-major  rows x LD  doubles with LD = the number of columns (2..24, no padding
// columns), so one row is LD*8 contiguous bytes and a d x LD pose block is contiguous as well.  fp64 throughout (the
// reference's `typedef double Scalar`, include/CORA/CORA_types.h:43).  No MFMA in the products: the path is
// HBM/L2-bound (0.49 flop/B at p = 5); the fp64 matrix cores serve the Gram / combine kernels of LOBPCG only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "config.h"
#include "cora_internal.h"
#include "dispatch.h"
#include "kernels.h"

// The file is compiled several times in parallel (cora_amd/build.py): CORA_TU selects the kernel families of a
// translation unit (1 SpMM, 2 row-unit / vector / block kernels, 4 staged triangular solves, 8 the chain placement's batched kernels, 16 its outlier-robust kernels), CORA_LDG the row strides
// it instantiates of the two big families (1: LD 2-5, 2: 6-9, 4: 10-12, 8: 13-16, 16: 17-20, 32: 21-24).  Default: all.
#ifndef CORA_TU
#define CORA_TU 31
#endif
#ifndef CORA_LDG
#define CORA_LDG 63
#endif

// ONE source in sixteen pieces (round 6: the file had grown to 3 700 lines); this file holds the switches of the translation units
// and, at the end, the measurement builds' read-back hooks.  Inside namespace cora, in this order:
//   kernels/common.inc   row loads / stores, wave reductions, the chunk and list sums of the placement initialisers, the STPCG state's scalar steps
//   kernels/spmm.inc     the sliced SpMM with fused epilogues (chain slices, row slices, long-row chunks)        CORA_TU & 1
//   kernels/rows.inc     row-unit, vector, reduction, exchange and LOBPCG block kernels                           CORA_TU & 2
//   kernels/residuals.inc  per-measurement residuals: one gather pass over the measurement table                   CORA_TU & 2
//   kernels/gnc.inc      the GNC weight step: unweighted residuals, weights and statistics in one pass                CORA_TU & 2
//   kernels/compare.inc  trajectory comparison: column sums, centred rows, errors and the aligned vector               CORA_TU & 2
//   kernels/rpe.inc      relative pose error over the handle's pair table: errors, sums, maxima, first maximum       CORA_TU & 2
//   kernels/round.inc    rounding of a resident vector to SE(d): count, finish, per-unit pass                       CORA_TU & 2
//   kernels/odom.inc     odometry initialisation: segmented scan of SE(d) over the chain positions, fill of the other rows  CORA_TU & 2
//   kernels/multilat.inc  landmark initialisation from ranges: pass over the chunks of the range lists, fold and solve per landmark  CORA_TU & 2
//   kernels/placement.inc  chain placement from inter-robot ranges: linear and Gauss-Newton pass and fold per stage, the rigid motion of a chain  CORA_TU & 2; the same for all stages of a level  CORA_TU & 8; the hypotheses, consensus vote, election and masked passes of the robust form  CORA_TU & 16
//   kernels/sighting.inc  placement from pose-landmark sightings: pass and fold over all lists of a stage, the rigid motion of a stage's chains; the hypotheses, consensus vote, election and masked passes of the robust form  CORA_TU & 2
//   kernels/closure.inc  placement from inter-chain relative-pose edges: pass and fold over all lists of a stage (sums and solve, costs); the consensus vote, election and masked passes of the robust form  CORA_TU & 2
//   kernels/update_values.inc  in-place update of Q's values: check of the new values, gather passes                CORA_TU & 2
//   kernels/assemble.inc  Q(w) from per-measurement weights through the term map: check, short and long entries     CORA_TU & 2
//   kernels/tri.inc      the staged Cholesky solve: k_rowop, k_blockop, k_subblock                                 CORA_TU & 4
//   kernels/launch.inc   host-side launch wrappers (kernels.h), per translation unit and row-stride group; every choice of an instantiation goes through dispatch.h
namespace cora {
#include "kernels/common.inc"
#include "kernels/spmm.inc"
#include "kernels/rows.inc"
#include "kernels/residuals.inc"
#include "kernels/gnc.inc"
#include "kernels/compare.inc"
#include "kernels/rpe.inc"
#include "kernels/round.inc"
#include "kernels/odom.inc"
#include "kernels/multilat.inc"
#include "kernels/placement.inc"
#include "kernels/sighting.inc"
#include "kernels/closure.inc"
#include "kernels/update_values.inc"
#include "kernels/assemble.inc"
#include "kernels/tri.inc"
#include "kernels/launch.inc"
}  // namespace cora

#if defined(CORA_SUB_TIMES) && (CORA_TU & 4) && (CORA_LDG & 1)
// measurement build only (-DCORA_SUB_TIMES, tools/sub_timeline.py): the block timestamps of the last forward and backward sweep
extern "C" int cora_debug_sub_phases(unsigned long long *out, int n_blocks) {
  if (n_blocks < 0 || static_cast<unsigned>(n_blocks) > cora::kSubTimesMax) return -1;
  for (int w = 0; w < 2; ++w)
    if (hipMemcpyFromSymbol(out + static_cast<size_t>(w) * cora::kSubPhases * n_blocks, HIP_SYMBOL(cora::g_sub_phase),
                            sizeof(unsigned long long) * cora::kSubPhases * n_blocks,
                            sizeof(unsigned long long) * w * cora::kSubPhases * cora::kSubTimesMax) != hipSuccess) return -2;
  return 0;
}
#endif
#if defined(CORA_SPMM_TIMES) && (CORA_TU & 1) && (CORA_LDG & 1)
// measurement build only (-DCORA_SPMM_TIMES, tools/spmm_timeline.py): the wavefront timestamps of the last k_spmm launch
extern "C" int cora_debug_spmm_times(unsigned long long *out, int n_blocks) {
  if (n_blocks < 0 || static_cast<unsigned>(n_blocks) > cora::kSpmmTimesMax) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(cora::g_spmm_times), sizeof(unsigned long long) * 3 * n_blocks) == hipSuccess ? 0 : -2;
}
extern "C" int cora_debug_spmm_phases(unsigned long long *out, int n_blocks) {
  if (n_blocks < 0 || static_cast<unsigned>(n_blocks) > cora::kSpmmTimesMax) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(cora::g_spmm_phase), sizeof(unsigned long long) * cora::kSpmmPhases * n_blocks) == hipSuccess ? 0 : -2;
}
#endif
