// Every environment variable the library reads, in one table (config.cpp is the only reader).  Call sites name a variable
// by its enum, so a misspelt name does not compile; include/cora_hip.h documents the same names for users, and
// tests/test_config_cpu.py keeps the two lists equal.
//
// Kinds: a FLAG is on when the variable is set to a non-empty value that does not start with '0' (unset: the default);
// an INT is parsed as a decimal integer and a REAL as a floating-point number, each clamped to [lo, hi] when set (an
// unset variable gives the default, which may lie outside the range: 0 = "the site decides" where the description says so).
// Lifetimes: ONCE entries are read at their first use and keep that value for the life of the process (thread-safe);
// CALL entries are read every time a call asks for them (tests flip them between calls).
#pragma once

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace cora {

// X(id, name, kind, default, lo, hi, lifetime, description)
#define CORA_ENV_TABLE(X)                                                                                                    \
  /* forms of the STPCG iteration */                                                                                         \
  X(NoFuse, "CORA_NO_FUSE", Flag, 0, 0, 1, Call, "one pass per operation instead of the fused vector passes")               \
  X(NoSweepFuse, "CORA_NO_SWEEP_FUSE", Flag, 0, 0, 1, Call, "vector passes not folded into the Cholesky sweeps")             \
  X(NoInverseFuse, "CORA_NO_INVERSE_FUSE", Flag, 0, 0, 1, Call, "... nor into the products of a one-inverse plan")          \
  X(NoResidualSlots, "CORA_NO_RESIDUAL_SLOTS", Flag, 0, 0, 1, Once, "one-inverse iteration: <r, r> by ticket")               \
  X(NoKappaFold, "CORA_NO_KAPPA_FOLD", Flag, 0, 0, 1, Call, "kappa = <p, Hp> always gets a launch of its own")               \
  X(KappaFoldMax, "CORA_KAPPA_FOLD_MAX", Int, 4096, INT32_MIN, INT32_MAX, Once, "... above this many partials")              \
  X(NoTntFuse, "CORA_NO_TNT_FUSE", Flag, 0, 0, 1, Call, "cora_tnt_accept_dev forms Q X again")                               \
  /* host loop of cora_stpcg_dev */                                                                                          \
  X(StpcgDepth, "CORA_STPCG_DEPTH", Int, -1, INT32_MIN, INT32_MAX, Call, "iterations the host runs ahead (-1: by size)")     \
  X(StpcgAhead, "CORA_STPCG_AHEAD", Int, -1, INT32_MIN, INT32_MAX, Call, "product-ahead form off | on (-1: by depth)")       \
  X(StpcgBatch, "CORA_STPCG_BATCH", Int, 0, INT32_MIN, INT32_MAX, Call, "iterations enqueued per look (0: by size)")         \
  X(StpcgGraph, "CORA_STPCG_GRAPH", Flag, 0, 0, 1, Call, "hipGraph replay of batches")                                       \
  /* partitioned handles */                                                                                                  \
  X(NoExchangeOverlap, "CORA_NO_EXCHANGE_OVERLAP", Flag, 0, 0, 1, Once, "interior slices never beside the exchange")        \
  X(ExchangeOverlapMinSlices, "CORA_EXCHANGE_OVERLAP_MIN_SLICES", Int, 2048, INT32_MIN, INT32_MAX, Once,                     \
    "... from this many interior slices per rank")                                                                           \
  X(ImplicitWholeGather, "CORA_IMPLICIT_WHOLE_GATHER", Flag, 0, 0, 1, Call, "implicit form gathers whole shards")            \
  X(P2pTimeoutS, "CORA_P2P_TIMEOUT_S", Real, 60, 0.001, HUGE_VAL, Call, "seconds a device-side collective waits")               \
  /* format of Q and the product's launch */                                                                                 \
  X(ChainSlices, "CORA_CHAIN_SLICES", Flag, 1, 0, 1, Once, "pose slices in the chain layout")                                \
  X(SliceLjf, "CORA_SLICE_LJF", Flag, 1, 0, 1, Call, "pose slices first inside an XCD's range")                              \
  X(SpmmWindowMinSlices, "CORA_SPMM_WINDOW_MIN_SLICES", Int, 2048, INT32_MIN, INT32_MAX, Once,                               \
    "LDS-window form of k_spmm from this many slices")                                                                       \
  X(SpmmStaggerTicks, "CORA_SPMM_STAGGER_TICKS", Int, 300, 0, 2000, Once,                                                    \
    "10 ns ticks a SIMD's second pose slice of k_spmm starts late (0: off)")                                                 \
  X(FormatThreads, "CORA_FORMAT_THREADS", Int, 0, 1, INT32_MAX, Call, "format builder threads (0: by size)")                 \
  X(FormatTiming, "CORA_FORMAT_TIMING", Flag, 0, 0, 1, Call, "format builder phase times on stderr")                         \
  /* solve plan of a Cholesky factor (trisolve_build.cpp) */                                                                 \
  X(TriSub, "CORA_TRI_SUB", Int, 1, INT32_MIN, INT32_MAX, Call, "0: explicit stages instead of substitution blocks")         \
  X(TriSnCap, "CORA_TRI_SN_CAP", Int, 0, 1, 32, Call, "rows per supernode (0: 4 or 8 by tree height)")                       \
  X(TriUnfoldMin, "CORA_TRI_UNFOLD_MIN", Int, 2000000, INT64_MIN, INT64_MAX, Call, "aux sums folded below this")             \
  X(TriThreads, "CORA_TRI_THREADS", Int, 0, 1, INT32_MAX, Call, "plan builder threads (0: by size)")                         \
  X(TriCheckEtree, "CORA_TRI_CHECK_ETREE", Flag, 0, 0, 1, Call, "elimination tree computed both ways and compared")          \
  X(TriTiming, "CORA_TRI_TIMING", Flag, 0, 0, 1, Call, "set-up phase times on stderr")                                       \
  X(SubIoLists, "CORA_SUB_IO_LISTS", Flag, 0, 0, 1, Call, "sweep row I/O from index lists instead of run tables")            \
  X(TriTopInv, "CORA_TRI_TOP_INV", Int, 2500000, 0, INT64_MAX, Once, "entries of a last-stage inverse always taken")         \
  X(TriShortRow, "CORA_TRI_SHORT_ROW", Int, 64, 8, 1 << 30, Once, "row entries: up to this, 8 lanes per row")                \
  X(TriWaveRow, "CORA_TRI_WAVE_ROW", Int, 1024, 64, 1 << 30, Once, "... up to this, a wavefront per row")                    \
  X(TriChunk, "CORA_TRI_CHUNK", Int, 512, 64, 1 << 30, Once, "entries per chunk of a longer row")                            \
  X(TriSubRows, "CORA_TRI_SUB_ROWS", Int, 512, 32, 2048, Once, "rows of a substitution block")                               \
  X(TriSubEnt, "CORA_TRI_SUB_ENT", Int, 5000, 100, 1 << 30, Once, "entries of L per substitution block")                     \
  X(TriLaneEntries, "CORA_TRI_LANE_ENTRIES", Int, 8, 1, 8, Once, "entries one lane of a level walks")                        \
  X(TriLevelLanes, "CORA_TRI_LEVEL_LANES", Int, 256, 64, 256, Once, "rows x lanes per row of one level")                     \
  X(TriSplitMinRows, "CORA_TRI_SPLIT_MIN_ROWS", Int, 1 << 20, 1, 1 << 30, Once, "level chunks closed early from here")       \
  /* host factorisation and ordering */                                                                                      \
  X(CholThreads, "CORA_CHOL_THREADS", Int, 0, 1, INT32_MAX, Call, "numeric factorisation threads (0: by size)")              \
  X(SymbolicThreads, "CORA_SYMBOLIC_THREADS", Int, 0, 1, INT32_MAX, Call, "symbolic analysis threads (0: by size)")          \
  X(CholNoSymbolicCache, "CORA_CHOL_NO_SYMBOLIC_CACHE", Flag, 0, 0, 1, Call, "symbolic analysis never reused")               \
  X(CholNoTrailingGroup, "CORA_CHOL_NO_TRAILING_GROUP", Flag, 0, 0, 1, Call, "trailing rows one at a time")                  \
  X(NdLeaf, "CORA_ND_LEAF", Int, 0, 1, INT32_MAX, Call, "poses per dissection leaf (0: 2 preconditioner, 8 translations)")   \
  X(RegCholeskyMaxCond, "CORA_REG_CHOLESKY_MAX_COND", Real, 1e6, -HUGE_VAL, HUGE_VAL, Call, "kappa_max, regularised precond.")    \
  /* solveCORA */                                                                                                            \
  X(NoCertPrepare, "CORA_NO_CERT_PREPARE", Flag, 0, 0, 1, Call, "certification not prepared beside the first solve")        \
  X(NoCertSpeculation, "CORA_NO_CERT_SPECULATION", Flag, 0, 0, 1, Call, "eigensolver not started beside the PSD test")      \
  X(NoPivotSeed, "CORA_NO_PIVOT_SEED", Flag, 0, 0, 1, Call, "fast_verification keeps the reference's plain order")          \
  X(TraceBits, "CORA_TRACE_BITS", Flag, 0, 0, 1, Once, "bits of every staircase stage on stdout")

enum class Env : int {
#define CORA_ENV_ID(id, ...) id,
  CORA_ENV_TABLE(CORA_ENV_ID)
#undef CORA_ENV_ID
};

bool env_flag(Env e);
int64_t env_int(Env e);
double env_real(Env e);
bool env_set(Env e);  // the variable is set (for a ONCE entry: was set when first read)

// Phase times on stderr, one line per phase: "<tag> <phase, padded to width> <seconds> s".
class PhaseTimer {
 public:
  PhaseTimer(bool on, const char *tag, int width, int precision)
      : on_(on), tag_(tag), width_(width), precision_(precision), prev_(std::chrono::steady_clock::now()) {}
  void operator()(const char *phase) {
    if (!on_) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "%s %-*s %.*f s\n", tag_, width_, phase, precision_, std::chrono::duration<double>(now - prev_).count());
    prev_ = now;
  }
  bool on() const { return on_; }

 private:
  bool on_;
  const char *tag_;
  int width_, precision_;
  std::chrono::steady_clock::time_point prev_;
};

}  // namespace cora
