// pea_common.h -- kernel parameters and device helpers common to every kernel family.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pea.h"

namespace pea {

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kXcd = 8;

struct KParams {
  int B, D, Z, Y, X, K;
  int S;  // Z*Y*X (fits int32: checked on the host)
  int border;
  unsigned flags;
  float eps;
  int chunks;          // workgroups per batch item = ceil(S / kBlock)
  int tiles;           // B * chunks
  int tiles_per_xcd;   // ceil(tiles / 8)
  int off[PEA_MAX_K][3];
  float lam[PEA_MAX_K];
  float inv_n[PEA_MAX_K];   // 1 / N_i
  float gscale[PEA_MAX_K];  // 2 * lambda_i / N_i
  long long tbs, wbs, mbs;  // batch strides (elements) of target / weight / mask
  int ksplit;               // offset channels >= ksplit are addressed through a second buffer resource based ksplit planes further:
                            // K (no split) unless the [K, Z, Y, X] block of a batch item reaches 2 GiB (the raw-buffer range check
                            // counts the scalar plane offset: pea_hip.hip plan_tiles); only k_fwd_tiled / k_bwd_tiled honour it
};

template <typename T>
__device__ __forceinline__ float ld(const T* p, size_t i);
template <>
__device__ __forceinline__ float ld<float>(const float* p, size_t i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<__half>(const __half* p, size_t i) { return __half2float(p[i]); }
template <>
__device__ __forceinline__ float ld<__bf16>(const __bf16* p, size_t i) { return (float)p[i]; }  // a 16-bit shift

__device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(__half* p, size_t i, float v) { p[i] = __float2half(v); }
// a plain cast: v_cvt_pk_bf16_f32, round to nearest even with NaN kept (the integer-rounding trick turns some NaNs into 0 / inf)
__device__ __forceinline__ void st(__bf16* p, size_t i, float v) { p[i] = (__bf16)v; }

// the storage types of the embedding (PEA_F32 / PEA_F16 / PEA_BF16)
template <typename T>
constexpr bool is_emb_t = std::is_same<T, float>::value || std::is_same<T, __half>::value || std::is_same<T, __bf16>::value;

// XCD-aware remap: hardware deals consecutive workgroup ids round-robin over the 8 XCDs, so
// id % 8 labels the XCD group.  Give group g the contiguous logical tiles [g*tpx, (g+1)*tpx).
__device__ __forceinline__ int logical_tile(const KParams& P) {
  const int bid = blockIdx.x;
  return (bid % kXcd) * P.tiles_per_xcd + bid / kXcd;
}

// REPLICATE, role B: the coordinates c' along one axis (extent n) with clamp(c' + o) == c, as [lo, hi] (empty: lo > hi).
// Interior c has the one pre-image c - o; a border coordinate collects every c' that the clamp folds onto it.
__device__ __forceinline__ void clamp_preimage(int c, int o, int n, int& lo, int& hi) {
  lo = hi = c - o;
  if (o < 0 && c == 0) { lo = 0; hi = min(-o, n - 1); }
  else if (o > 0 && c == n - 1) { lo = max(n - 1 - o, 0); hi = n - 1; }
  else if (lo < 0 || lo > n - 1) { lo = 1; hi = 0; }
}

// activation of the affs output (include/pea.h PEA_FLAG_*): flags are wave-uniform, the common case (0) is one scalar branch
constexpr unsigned kActMask = PEA_FLAG_RELU_AFFS | PEA_FLAG_ONE_MINUS | PEA_FLAG_HALF_SHIFT | PEA_FLAG_CLAMP01;
// relu and clamp as SELECTS, not fmaxf / fminf: C's fmaxf(NaN, 0) is 0, F.relu and torch.clamp keep NaN -- and a NaN affinity is the only
// sign of a non-finite embedding that a caller gets (include/pea.h, "Non-finite embeddings").  Every comparison with NaN is false, so
// NaN falls through; every other value compares equal to what fmaxf / fminf gave (-0.0 stays -0.0, as in torch).
__device__ __forceinline__ float relu_keep_nan(float a) { return a < 0.f ? 0.f : a; }
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float act_affs(float a, unsigned af) {
  if (af == 0) return a;
  if (af & PEA_FLAG_HALF_SHIFT) a = (a + 1.0f) * 0.5f;
  if (af & PEA_FLAG_RELU_AFFS) a = relu_keep_nan(a);
  if (af & PEA_FLAG_CLAMP01) a = clamp_keep_nan(a, 0.f, 1.0f);
  if (af & PEA_FLAG_ONE_MINUS) a = 1.0f - a;
  return a;
}

// PEA_FLAG_LOSS_ACT (the LACT instantiations of the training forwards): the loss is taken on u = act_affs(a, af), af = HALF_SHIFT and /
// or CLAMP01 (pea_desc_validate admits nothing else).  The flags are wave-uniform, so the activation is four scalars and no branch:
//   v = a * sc + of,  u = v < lo ? lo : v > hi ? hi : v   (sc, of) = (1/2, 1/2) for the half shift, (lo, hi) = (0, 1) for the clamp, else infinite
// -- the same bits act_affs stores ((a + 1) / 2 and a / 2 + 1/2 round alike: halving is exact) -- and the slope du / da is sc where the
// clamp left v alone (u == v: torch.clamp's backward is INCLUSIVE at both edges), 0 where it did not.  The forward folds the slope
// into g (act_g), so the backward kernels do not know about activations.  `gz` is g where u != v because v is NaN: 0 with the clamp,
// NaN without it (the half shift alone has no branch: g = 2 w m r s / N is NaN like r).  How the epilogues use these -- the order of
// operations, what they keep across their stores, the NaN policy -- is stated with the loss term in pea_epilogue.h.
struct ActK {
  float sc, of, lo, hi, gz;
};
__device__ __forceinline__ ActK act_consts(unsigned af) {
  ActK k;
  k.sc = (af & PEA_FLAG_HALF_SHIFT) ? 0.5f : 1.0f;
  k.of = (af & PEA_FLAG_HALF_SHIFT) ? 0.5f : 0.f;
  k.lo = (af & PEA_FLAG_CLAMP01) ? 0.f : -__builtin_inff();
  k.hi = (af & PEA_FLAG_CLAMP01) ? 1.0f : __builtin_inff();
  k.gz = (af & PEA_FLAG_CLAMP01) ? 0.f : __builtin_nanf("");
  return k;
}
__device__ __forceinline__ float act_v(float a, const ActK& k) { return fmaf(a, k.sc, k.of); }
__device__ __forceinline__ float act_u(float v, const ActK& k) { return clamp_keep_nan(v, k.lo, k.hi); }
// g of a term whose raw-cosine form is gs_sc * wr * m, gs_sc = gscale * ActK::sc (exact: sc is a power of two)
__device__ __forceinline__ float act_g(float u, float v, float gs_sc, float wr, float m, const ActK& k) { return u == v ? gs_sc * wr * m : k.gz; }

// PEA_FLAG_LOSS_BCE (the BCE instantiations of the LACT forwards: k_fwd_direct, k_fwd_xdma): the criterion on x = u m, y = t m is the
// weighted binary cross-entropy of F.binary_cross_entropy -- both logs clamped at -100 (a select: NaN stays NaN), log1p for the second --
// and the returned factor is torch's own BCE backward, w (x - y) / max(x (1 - x), 1e-12); loss_term (pea_epilogue.h) hands it to act_g
// as `wr` with gs_sc = lambda / N * ActK::sc (no factor 2).  Explicit fmaf (no contraction left to the context), IEEE division, logf /
// log1pf (not the fast intrinsics): the direct and the cross kernel give the same bits of g and contrib for the same a.
// m = 0: x = y = 0, contrib = -w (0 * -100 + 1 * log1p(-0)) = 0 and the factor is 0 / 1e-12 = 0.  x = 0, y = 1: contrib = 100 w exactly.
__device__ __forceinline__ float bce_log(float l) { return l < -100.0f ? -100.0f : l; }
__device__ __forceinline__ float bce_term(float x, float y, float w, float& contrib) {
  const float lx = bce_log(logf(x)), l1 = bce_log(log1pf(-x));
  contrib = -w * fmaf(y, lx, (1.0f - y) * l1);
  return (x - y) / fmaxf(x * (1.0f - x), 1e-12f) * w;
}

__device__ __forceinline__ float inv_norm(float ss, float eps) { return 1.0f / fmaxf(sqrtf(ss), eps); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

}  // namespace pea
