// pea_gather.h -- the one-lane-per-pixel ("gather") arithmetic, stated once.
//
// The direct kernels (pea_direct.h), the batched tensor form (pea_k_multi.hip) and the batched labels-in form
// (pea_k_multi_labels.hip) all evaluate a pixel the same way: its own D channels in registers, every neighbour vector read from
// global memory with its sum of squares accumulated while the channels stream in,
//   a = dot * 1 / max(|e(p)|, eps) * 1 / max(|e(q)|, eps),
//   de = dloss * (G - ehat <ehat, G>) / n(p)        (G / eps where |e(p)| < eps: the clamp branch of F.normalize).
// The contracts between these families are contracts on BITS (the batched launches carry the single calls' affs and g, and their
// de in f32 and bf16 -- an f16 de lies within one f16 ulp: the two store policies of project_store --; role B of the labels-in form
// reproduces what role A of the neighbour computes), so the order of the fused multiply-adds exists here: the bodies compose these
// blocks (k_bwd_direct restates gather_pair, see there).  The loss term of a pair is loss_term of pea_epilogue.h, shared with the
// LDS-staged families.  What differs between the families on purpose stays in the kernels: which lanes hold a loss partial and how
// they meet, the tile walk, the REPLICATE pre-image loop and the runtime-D paths.
//
// Every block is a __forceinline__ template of the storage type T (float / __half / __bf16 through ld() / st()), the width D and a
// geometry GEO: anything with S, Z, Y, X, K, eps, off[i][3] (and border for the runtime neighbour) -- KParams and multi::MGeom.
#pragma once
#include "pea_epilogue.h"

namespace pea {

// p -> (z, y, x)
template <typename GEO>
__device__ __forceinline__ void split_voxel(const GEO& G, int p, int& z, int& y, int& x) {
  const int yx = G.Y * G.X;
  z = p / yx;
  const int r = p - z * yx;
  y = r / G.X;
  x = r - y * G.X;
}

// neighbour of (z, y, x) displaced by o: flat index, or -1 (CROP_ZERO, outside).  BORDER: PEA_BORDER_CIRCULAR / PEA_BORDER_CROP_ZERO
// known at compile time, or kBorderRuntime: G.border decides (the only form that serves REPLICATE)
constexpr int kBorderRuntime = -1;
template <int BORDER = kBorderRuntime, typename GEO>
__device__ __forceinline__ int neighbour(const GEO& G, int z, int y, int x, int oz, int oy, int ox) {
  static_assert(BORDER == kBorderRuntime || BORDER == PEA_BORDER_CIRCULAR || BORDER == PEA_BORDER_CROP_ZERO, "REPLICATE: runtime form only");
  int border = BORDER;
  if constexpr (BORDER == kBorderRuntime) border = G.border;
  int zz = z + oz, yy = y + oy, xx = x + ox;
  if (border == PEA_BORDER_CIRCULAR) {  // the host guarantees |o| < dim
    zz += (zz < 0) ? G.Z : 0; zz -= (zz >= G.Z) ? G.Z : 0;
    yy += (yy < 0) ? G.Y : 0; yy -= (yy >= G.Y) ? G.Y : 0;
    xx += (xx < 0) ? G.X : 0; xx -= (xx >= G.X) ? G.X : 0;
  } else if (border == PEA_BORDER_REPLICATE) {  // index clamped into the volume: every pair exists
    zz = min(max(zz, 0), G.Z - 1);
    yy = min(max(yy, 0), G.Y - 1);
    xx = min(max(xx, 0), G.X - 1);
  } else if ((unsigned)zz >= (unsigned)G.Z || (unsigned)yy >= (unsigned)G.Y || (unsigned)xx >= (unsigned)G.X) {
    return -1;
  }
  return (zz * G.Y + yy) * G.X + xx;
}

// v = the D channels of pixel p of `base` ([D, S]); returns their sum of squares, accumulated in channel order
template <int D, typename T>
__device__ __forceinline__ float load_vec(const T* base, size_t S, int p, float (&v)[D]) {
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    v[c] = ld(base, c * S + p);
    ss = fmaf(v[c], v[c], ss);
  }
  return ss;
}

// <own, v> in channel order
template <int D>
__device__ __forceinline__ float dot_vec(const float (&own)[D], const float (&v)[D]) {
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) dot = fmaf(own[c], v[c], dot);
  return dot;
}

// the forward's streaming form: the cosine of `own` (1 / norm: inv_own) and pixel q of `base`, no copy of q's vector kept
template <int D, typename T>
__device__ __forceinline__ float cosine_streamed(const float (&own)[D], float inv_own, const T* base, size_t S, int q, float eps) {
  float dot = 0.f, sq = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float v = ld(base, c * S + q);
    dot = fmaf(own[c], v, dot);
    sq = fmaf(v, v, sq);
  }
  return dot * inv_own * inv_norm(sq, eps);
}

// G += coef * v
template <int D>
__device__ __forceinline__ void accumulate(float (&G)[D], float coef, const float (&v)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) G[c] = fmaf(coef, v[c], G[c]);
}

// one (offset, role) pair of the backward: G += g * nhat(q), q the neighbour in `nb`.  g is the loss term's gradient, read by the
// caller at the FIRST operand's pixel: the own pixel for role A, q for role B.  (k_bwd_direct states these lines itself: see there.)
template <int D, typename T>
__device__ __forceinline__ void gather_pair(float (&G)[D], const T* nb, size_t S, int q, float g, float eps) {
  float v[D];
  const float sq = load_vec(nb, S, q, v);
  accumulate(G, g * inv_norm(sq, eps), v);
}

// st() of a value that exists as f32 BEFORE it is rounded to the storage type (the contract of include/pea.h: de16 = round(de32)).
// Left alone the compiler folds the last multiply and the f16 conversion into one v_fma_mixlo_f16: a single rounding of the exact
// product, one f16 ulp away from the rounded f32 result in a few of 100 000 values.  Only __half has such an instruction: the
// f32 and the bf16 stores (a plain v_cvt_pk_bf16_f32 of the finished product) are left to the compiler.
template <typename T>
__device__ __forceinline__ void st_rounded(T* p, size_t i, float v) {
  if constexpr (std::is_same<T, __half>::value) asm volatile("" : "+v"(v));
  st(p, i, v);
}

// dx(p) = dl * (G - xhat <xhat, G>) / n(p), G / eps where n(p) = nrm < eps; xc = x(p), inv_p = 1 / max(nrm, eps).
// ROUNDED is the store policy: st_rounded() (the batched kernels) or st() (k_bwd_direct, whose f16 store the compiler may fuse with the
// last multiply).  The two differ in a few f16 values and each is its family's current behaviour: they are NOT to be unified.
template <bool ROUNDED, int D, typename T>
__device__ __forceinline__ void project_store(T* db, size_t S, int p, const float (&xc)[D], const float (&G)[D], float nrm, float inv_p,
                                              float eps, float dl) {
  float proj = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) proj = fmaf(xc[c] * inv_p, G[c], proj);
  if (nrm < eps) proj = 0.f;  // clamp_min branch of F.normalize: d ehat / d e = I / eps
  const float sc = dl * inv_p;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float v = (G[c] - xc[c] * inv_p * proj) * sc;
    if constexpr (ROUNDED) st_rounded(db, c * S + p, v);  // 16-bit: rounded once, NaN kept
    else st(db, c * S + p, v);
  }
}

// class-balance weights of a channel with `count` target-1 voxels of S: f = clip(count / S, 0.05, 0.99), the minority class gets
// max(f, 1 - f) / min(f, 1 - f), the majority and a single-valued channel 1.  Evaluated in f64 like numpy, rounded to f32 once.
struct ClassWeights {
  float pos, neg;  // weight of the target-1 voxels, of the target-0 voxels
};
__device__ __forceinline__ ClassWeights class_balance(unsigned count, int S) {
  float wpos = 1.f, wneg = 1.f;
  if (count != 0 && count != (unsigned)S) {
    double f = (double)count / (double)S;
    f = fmin(fmax(f, 5e-2), 0.99);
    if (f > 0.5) wneg = (float)(f / (1.0 - f));
    else wpos = (float)((1.0 - f) / f);
  }
  return ClassWeights{wpos, wneg};
}

}  // namespace pea
