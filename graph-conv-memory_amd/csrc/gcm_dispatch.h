// From runtime shapes to a kernel instantiation: the one mechanism every launcher in csrc/ uses.
//
//     return gcm_pick([&](auto nt, auto nct) { return launch(k_step<nt(), nct()>, ...); },
//                     OneOf<1, 2, 3, 4>{NT}, OneOf<1, 2>{NCT});
//
// f is called at most once, with the std::integral_constant of each runtime value, and its int result is returned;
// when a value is none of its Vs nothing is called and GCM_EUNSUPPORTED comes back.  Exactly the product of the Vs is
// instantiated: a table that is no full product is several picks, or an `if constexpr` in f around what does not
// exist.  A bucketed choice (F <= 16 -> 16, ...) computes the bucket in plain code first.  Plain host C++.
#pragma once
#include <type_traits>

#include "gcm_hip.h"

template <int... Vs>
struct OneOf {   // a runtime value and the compile-time values it may take
  int v;
};
using Flag = OneOf<0, 1>;   // a bool: Flag{p != nullptr}, used as k<bool(c())>
template <int V>
constexpr std::integral_constant<int, V> gcm_c{};   // a constant where f is called by hand: f(gcm_c<32>, ...)

template <typename F>
int gcm_pick(F f) {
  return f();
}
template <typename F, int... Vs, typename... Rest>
int gcm_pick(F f, OneOf<Vs...> d, Rest... rest) {
  int rc = GCM_EUNSUPPORTED;
  (void)((d.v == Vs
              ? (rc = gcm_pick([&](auto... c) { return f(std::integral_constant<int, Vs>{}, c...); }, rest...), true)
              : false) ||
         ...);
  return rc;
}
