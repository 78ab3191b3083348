// Runtime value -> template argument, once per axis.  Each helper hands the value of a call (d, a row stride, the piece width
// of a stride, a switch, a mode) to a generic functor as a std::integral_constant, so a launcher names its kernel ONCE,
//   for_d(A.d, [&](auto D) { for_width(A.ld, [&](auto W) { hipLaunchKernelGGL((k_edge_residuals<D(), W()>), ..); }); });
// and which instantiation a value selects is decided here and nowhere else.  Host-only and HIP-free; the whole mapping is
// checked at compile time at the end of the file.
#pragma once

#include <type_traits>

namespace cora {

template <int V>
using int_c = std::integral_constant<int, V>;

// d = 2 | 3 (checked by the caller); returns what f returns
template <class F>
constexpr auto for_d(int d, F &&f) {
  return d == 2 ? f(int_c<2>()) : f(int_c<3>());
}
// a switch of a kernel (backward, reciprocal) as std::true_type | std::false_type; returns what f returns
template <class F>
constexpr auto for_bool(bool b, F &&f) {
  return b ? f(std::true_type()) : f(std::false_type());
}
// the piece width of a row stride: 2 (16-byte pieces of a row) where the stride is even, 1 (8-byte) where it is odd
template <class F>
constexpr auto for_width(int ld, F &&f) {
  return ld % 2 == 0 ? f(int_c<2>()) : f(int_c<1>());
}
// an int in [LO, HI]: f(int_c<v>) and true; outside, no call and false.  (LO's own call stands before the rest, so that the
// compiler instantiates in ascending order, as for a typed-out list: the kernels keep their places in the code object)
template <int LO, int HI, class F>
constexpr bool for_int_in(int v, F &&f) {
  if constexpr (LO > HI) {
    return false;
  } else {
    if (v == LO) {
      f(int_c<LO>());
      return true;
    }
    return for_int_in<LO + 1, HI>(v, f);
  }
}
// a row stride in [LO, HI]: false, and no call, where ld is outside
template <int LO, int HI, class F>
constexpr bool for_ld(int ld, F &&f) {
  return for_int_in<LO, HI>(ld, f);
}
// a mode in [0, MODES) (checked by the caller)
template <int MODES, class F>
constexpr void for_mode(int mode, F &&f) {
  for_int_in<0, MODES - 1>(mode, f);
}

// The row-stride groups of the two big kernel families (SpMM, staged solves): group g is instantiated by the translation
// unit with bit g of CORA_LDG (kernels.hip).  ld_group_of: the group of a stride, kNumLdGroups where no group holds it.
struct LdGroup {
  int first, last;
};
constexpr LdGroup kLdGroups[] = {{2, 5}, {6, 9}, {10, 12}, {13, 16}, {17, 20}, {21, 24}};
constexpr int kNumLdGroups = sizeof(kLdGroups) / sizeof(kLdGroups[0]);
constexpr int ld_group_of(int ld) {
  int g = 0;
  while (g < kNumLdGroups && (ld < kLdGroups[g].first || ld > kLdGroups[g].last)) ++g;
  return g;
}

// ---- the self-test: every build checks the whole mapping before anything is launched ------------------------------------------
namespace dispatch_selftest {
// a stride ld in [LO, HI] with d and the width of ld: one call, with the runtime values as constants; a stride outside calls
// nothing and reports false
template <int LO, int HI>
constexpr bool strides_ok() {
  for (int ld = 0; ld <= 30; ++ld)
    for (int d = 2; d <= 3; ++d) {
      int calls = 0, got_ld = -1, got_d = -1, w = -1;
      const bool hit = for_ld<LO, HI>(ld, [&](auto LD) {
        for_d(d, [&](auto D) { for_width(ld, [&](auto W) { ++calls, got_ld = LD(), got_d = D(), w = W(); }); });
      });
      const bool inside = ld >= LO && ld <= HI;
      if (hit != inside || calls != (inside ? 1 : 0)) return false;
      if (inside && (got_ld != ld || got_d != d || w != (ld & 1 ? 1 : 2))) return false;
    }
  return true;
}
constexpr bool width_pairs_ok() {  // the widths of two strides, in the order given
  for (int ldx = 0; ldx <= 30; ++ldx)
    for (int ldr = 0; ldr <= 30; ++ldr) {
      int calls = 0, wx = -1, wr = -1;
      for_width(ldx, [&](auto WX) { for_width(ldr, [&](auto WR) { ++calls, wx = WX(), wr = WR(); }); });
      if (calls != 1 || wx != (ldx & 1 ? 1 : 2) || wr != (ldr & 1 ? 1 : 2)) return false;
    }
  return true;
}
template <int G = 0>
constexpr bool groups_ok() {  // the groups tile 2..24 in order, each dispatches its own strides, ld_group_of finds them
  if constexpr (G == kNumLdGroups) {
    return kLdGroups[G - 1].last == 24 && ld_group_of(1) == kNumLdGroups && ld_group_of(25) == kNumLdGroups;
  } else {
    constexpr LdGroup g = kLdGroups[G];
    if (g.first != (G == 0 ? 2 : kLdGroups[G == 0 ? 0 : G - 1].last + 1) || g.last < g.first) return false;
    for (int ld = g.first; ld <= g.last; ++ld)
      if (ld_group_of(ld) != G) return false;
    return strides_ok<g.first, g.last>() && groups_ok<G + 1>();
  }
}
template <int MODES>
constexpr bool modes_ok() {  // d, a mode and a switch
  for (int d = 2; d <= 3; ++d)
    for (int mode = 0; mode < MODES; ++mode)
      for (int b = 0; b <= 1; ++b) {
        int calls = 0, got_d = -1, got_mode = -1, got_b = -1;
        for_d(d, [&](auto D) {
          for_mode<MODES>(mode, [&](auto MODE) { for_bool(b != 0, [&](auto B) { ++calls, got_d = D(), got_mode = MODE(), got_b = B() ? 1 : 0; }); });
        });
        if (calls != 1 || got_d != d || got_mode != mode || got_b != b) return false;
      }
  return true;
}
static_assert(strides_ok<2, 24>() && width_pairs_ok(), "row strides 2..24 (row-unit kernels), d, piece widths");
static_assert(strides_ok<2, 12>(), "row strides 2..12 (the STPCG projections)");
static_assert(groups_ok(), "the row-stride groups");
static_assert(modes_ok<2>() && modes_ok<4>(), "d, mode and switch");
static_assert(for_d(3, [](auto D) { return D() + 1; }) == 4 && for_width(5, [](auto W) { return W() + 1; }) == 2, "what f returns");
}  // namespace dispatch_selftest

}  // namespace cora
