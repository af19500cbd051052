// Run-time choices as compile-time constants: a launcher writes its kernel's argument list once, inside a generic lambda, and
// a dispatcher hands the lambda the variant as std::integral_constant arguments (decltype(arg)::value in the template list).
#pragma once
#include <type_traits>

namespace pl {

template <int V>
using Int = std::integral_constant<int, V>;

// f(flag): a run-time yes / no as a compile-time constant
template <typename F>
inline void with_flag(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace pl
