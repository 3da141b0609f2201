// pea_dispatch.h -- run-time facts to template arguments, shared by the launchers (pea_k_*.hip).  Each with_* helper calls a generic
// lambda with a tag whose TYPE carries the fact (std::true_type, Tag<__half>, std::integral_constant<int, 32>, ..); the lambda reads
// it back as tag.value / typename decltype(tag)::type and uses `if constexpr` where a combination must not be instantiated.
#pragma once
#include <type_traits>

#include "pea_host.h"

namespace pea {

template <typename T>
struct Tag { using type = T; };
template <int N>
using Int = std::integral_constant<int, N>;

// Launch KERNEL with `lds` bytes of dynamic LDS.  false: the LDS limit could not be raised (allow_lds left the pending error set, the
// next hip_rc() reports it) and nothing was launched.
template <auto KERNEL, typename... ARGS>
inline bool launch(dim3 grid, dim3 blk, size_t lds, hipStream_t s, const ARGS&... args) {
  if (allow_lds<KERNEL>(lds)) return false;
  hipLaunchKernelGGL(KERNEL, grid, blk, lds, s, args...);
  return true;
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
inline auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// f(Tag<T>{}), T the embedding's storage type (validate() admits PEA_F32, PEA_F16 and PEA_BF16 only)
template <typename F>
inline auto with_storage(int dtype, F&& f) {
  if (dtype == PEA_F16) return f(Tag<__half>{});
  if (dtype == PEA_BF16) return f(Tag<__bf16>{});
  return f(Tag<float>{});
}

// f(Int<D>{}) for D among DS; false when it is not
template <int... DS, typename F>
inline bool with_width(int D, F&& f) {
  bool r = false;
  (void)((D == DS && ((r = f(Int<DS>{})), true)) || ...);
  return r;
}

// f(Tag<MT>{}, LACT): the mask's element type (float with PEA_FLAG_MASK_F32) and PEA_FLAG_LOSS_ACT as std::true_type / std::false_type
template <typename F>
inline auto with_mask_form(bool mf32, bool lact, F&& f) {
  return with_bool(lact, [&](auto la) { return mf32 ? f(Tag<float>{}, la) : f(Tag<uint8_t>{}, la); });
}

// f(Tag<MT>{}, LACT, BCE): with_mask_form and PEA_FLAG_LOSS_BCE; the criterion exists on the activated map only (pea_desc_validate), so
// BCE without LACT is never instantiated
template <typename F>
inline auto with_loss_form(bool mf32, bool lact, bool bce, F&& f) {
  return with_mask_form(mf32, lact, [&](auto mt, auto la) {
    if constexpr (la.value) return bce ? f(mt, la, std::true_type{}) : f(mt, la, std::false_type{});
    else return f(mt, la, std::false_type{});
  });
}

}  // namespace pea
