// pea_quad.h -- a lane's QUAD of four consecutive elements, shared by the streaming kernels that walk a flat pixel range (pea_k_metrics.hip,
// pea_k_fgmask.hip, pea_k_disc.hip, pea_k_segscore.hip, through pea_stream.h): one wide access (dwordx4 for f32 / i32, dwordx2 for 16-bit
// storage, one dword for u8) where the address is aligned to four elements and the quad is whole, four scalar accesses otherwise.  Which of
// the two is taken changes no bit of any value.
#pragma once
#include "pea_common.h"

namespace pea {

constexpr int kQuad = 4;  // consecutive pixels per lane and step

typedef float quad_t __attribute__((ext_vector_type(4)));
typedef int iquad_t __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float widen(unsigned short u) {
  if constexpr (std::is_same<T, __half>::value) return __half2float(__ushort_as_half(u));
  else return (float)__builtin_bit_cast(__bf16, u);
}
// round to nearest even, NaN kept (pea_common.h st())
template <typename T>
__device__ __forceinline__ unsigned short narrow(float v) {
  if constexpr (std::is_same<T, __half>::value) return __half_as_ushort(__float2half(v));
  else return __builtin_bit_cast(unsigned short, (__bf16)v);
}

// four consecutive values from p, the first nv of them valid, widened to f32: one dwordx4 / dwordx2 where the quad is whole and aligned
template <typename T>
__device__ __forceinline__ void ld_quad(const T* __restrict__ p, int nv, float (&o)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & (kQuad * sizeof(T) - 1)) == 0) {
    if constexpr (std::is_same<T, float>::value) {
      const quad_t v = *(const quad_t*)p;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
      const uint2 v = *(const uint2*)p;
      o[0] = widen<T>((unsigned short)(v.x & 0xffffu)); o[1] = widen<T>((unsigned short)(v.x >> 16));
      o[2] = widen<T>((unsigned short)(v.y & 0xffffu)); o[3] = widen<T>((unsigned short)(v.y >> 16));
    }
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e) o[e] = e < nv ? ld<T>(p, e) : 0.f;
  }
}
// the same for a u8 mask (one dword)
__device__ __forceinline__ void ld_quad(const uint8_t* __restrict__ p, int nv, float (&o)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & 3) == 0) {
    const uint32_t v = *(const uint32_t*)p;
    o[0] = (float)(v & 0xffu); o[1] = (float)((v >> 8) & 0xffu); o[2] = (float)((v >> 16) & 0xffu); o[3] = (float)(v >> 24);
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e) o[e] = e < nv ? (float)p[e] : 0.f;
  }
}
// the same for int32 labels (one dwordx4); the caller names the value of the lanes past nv
__device__ __forceinline__ void ld_iquad(const int32_t* __restrict__ p, int nv, int fill, int (&o)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & 15) == 0) {
    const iquad_t v = *(const iquad_t*)p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e) o[e] = e < nv ? p[e] : fill;
  }
}
template <typename T>
__device__ __forceinline__ void st_quad(T* __restrict__ p, int nv, const float (&v)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & (kQuad * sizeof(T) - 1)) == 0) {
    if constexpr (std::is_same<T, float>::value) {
      quad_t q;
      q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
      *(quad_t*)p = q;
    } else {
      uint2 q;
      q.x = (unsigned)narrow<T>(v[0]) | ((unsigned)narrow<T>(v[1]) << 16);
      q.y = (unsigned)narrow<T>(v[2]) | ((unsigned)narrow<T>(v[3]) << 16);
      *(uint2*)p = q;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e)
      if (e < nv) st(p, e, v[e]);
  }
}

}  // namespace pea
