// pea_head16.h -- the embedding head (pea_head.h) on 16-bit features: x and dx in f16 / bf16, e and de in the same type or in f32,
// W / bias / dW / db always f32 (include/pea_head16.h).  Reference: the same OutConv / conv3dBlock lines as pea_head.h, run under
// torch.autocast or on a .half() / .bfloat16() feature map.
//
// Same structure as pea_head.h -- planar streaming, W through the scalar cache, kHeadCB channels at a time, dx a launch of its own,
// dW on v_mfma_f32_16x16x4_f32 through the per-wave LDS tiles, per-workgroup partials and k_head_finalize (unchanged) -- with what
// 2-byte elements change:
//   * row width.  One pixel per lane would make every wave access a 128-byte row.  The PACKED form (V = 2) gives a lane two
//     x-adjacent pixels: one dword per lane and channel, the 256-byte rows of the f32 kernels at half the pixels' bytes.  It needs
//     every plane base + p to be 4-byte aligned (8 for an f32 e / de, moved as dwordx2): S even and the tensor bases aligned.  With
//     S odd the planes of odd channels sit 2 bytes off, so the host picks the ELEMENT form (V = 1, one ushort per lane) for those
//     calls and for skewed pointers; the answer is the same, only the speed differs.
//   * working form.  The loaded rows stay packed in registers (C dwords for 2C pixels-times-channels); a value is widened once, when
//     its channel is consumed (f16: v_cvt_f32_f16 on the selected half, bf16: a shift / a mask), and feeds D (forward) or kN (dx)
//     f32 accumulators per pixel.  Every product and sum is f32 with the f32 W; a 16-bit result is rounded once, to nearest even.
//   * dW.  The packed rows are handed to the MFMA tiles one half at a time (which pixel lands in which k slot is free as long as
//     de and x agree), so the tile code and its LDS footprint are those of pea_head.h.  16-bit values are exact in f32, the products
//     and sums are the f32 kernel's.  The wide heads (C > kHeadCB, coarse scales) load x 16 channels at a time inside the tile loop
//     and keep the element form.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "pea_host.h"
#include "pea_head.h"

namespace pea {

// the (C, D) pairs of PEA_HEAD_CASES (pea_k_head.hip): every head of the reference's models
#define PEA_HEAD16_CASES(X) \
  X(28, 16) X(32, 16) X(36, 16) X(48, 16) X(64, 16) X(80, 16) X(128, 16) X(256, 16) X(32, 32) X(64, 32) X(128, 32) X(256, 32)

// what pea_k_head16.hip calls; one translation unit per 16-bit type defines its pair (pea_k_head16_f16.hip, pea_k_head16_bf16.hip).
// Arguments are validated by the caller; PEA_OK, PEA_E_UNSUPPORTED (more chunks than one grid holds) or a HIP error.
int head16_fwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s);
int head16_fwd_bf16(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s);
int head16_bwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW,
                   float* db, float* partials, hipStream_t s);
int head16_bwd_bf16(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW,
                    float* db, float* partials, hipStream_t s);

typedef float hv2 __attribute__((ext_vector_type(2)));

// V x-adjacent elements of T as ONE load / store: f32 dword / dwordx2, 16-bit ushort / dword (the bit patterns, widened on use)
template <typename T, int V>
struct HeadRow {
  static constexpr bool kF32 = std::is_same<T, float>::value;
  static_assert(kF32 || std::is_same<T, __half>::value || std::is_same<T, __bf16>::value, "f32, f16 or bf16");
  static_assert(V == 1 || V == 2, "one pixel per lane or two");
  using raw = typename std::conditional<kF32, typename std::conditional<V == 1, float, hv2>::type,
                                        typename std::conditional<V == 1, unsigned short, unsigned>::type>::type;

  template <bool NT>
  static __device__ __forceinline__ raw load(const T* p) {
    const raw* q = reinterpret_cast<const raw*>(p);
    return NT ? __builtin_nontemporal_load(q) : *q;
  }
  // element h (0 .. V - 1) as f32
  static __device__ __forceinline__ float get(raw r, int h) {
    if constexpr (kF32) {
      if constexpr (V == 1) return r;
      else return h ? r.y : r.x;
    } else {
      const unsigned u = r;
      if constexpr (std::is_same<T, __bf16>::value) {
        return __uint_as_float(V == 2 ? ((u >> (16 * h)) << 16) : (u << 16));  // h known: a shift or a mask
      } else {
        const unsigned short b = (unsigned short)(V == 2 ? (u >> (16 * h)) : u);
        return (float)__builtin_bit_cast(_Float16, b);
      }
    }
  }
  static __device__ __forceinline__ unsigned narrow(float v) {  // round to nearest even, once
    if constexpr (std::is_same<T, __bf16>::value) {
      return __builtin_bit_cast(unsigned short, (__bf16)v);
    } else {
      // the f32 sum is a value of its own: without this the compiler folds the last FMA and the conversion into v_fma_mixlo_f16,
      // which rounds the unrounded sum -- and the f16 embedding would no longer be the f32 embedding of the same call, rounded
      asm volatile("" : "+v"(v));
      return __builtin_bit_cast(unsigned short, (_Float16)v);
    }
  }
  template <bool NT>
  static __device__ __forceinline__ void store(T* p, const float (&v)[V]) {
    raw r;
    if constexpr (kF32) {
      if constexpr (V == 1) r = v[0];
      else r = hv2{v[0], v[1]};
    } else {
      if constexpr (V == 1) r = (unsigned short)narrow(v[0]);
      else r = narrow(v[0]) | (narrow(v[1]) << 16);
    }
    raw* q = reinterpret_cast<raw*>(p);
    if (NT) __builtin_nontemporal_store(r, q);
    else *q = r;
  }
};

// e[b,d,p] = bias[d] + sum_c W[d,c] x[b,c,p]: kHeadCB packed rows requested up front, D x V accumulators, each value widened once
template <int C, int D, typename TX, typename TE, int V>
__global__ __launch_bounds__(kHeadBlock) void k_head16_fwd(const TX* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ bias, TE* __restrict__ e, long long S,
                                                           int chunks_per_b) {
  using RX = HeadRow<TX, V>;
  const int b = blockIdx.x / chunks_per_b;
  const long long p = ((long long)(blockIdx.x - b * chunks_per_b) * kHeadBlock + threadIdx.x) * V;
  if (p >= S) return;  // V = 2: S is even, so p + 1 < S as well
  const TX* xb = x + (size_t)b * C * S + p;
  TE* eb = e + (size_t)b * D * S + p;
  const bool has_bias = bias != nullptr;
  float a[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float bv = has_bias ? bias[d] : 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) a[d][v] = bv;
  }
  for (int c0 = 0; c0 < C; c0 += kHeadCB) {  // one pass for C <= kHeadCB
    constexpr int kN = C < kHeadCB ? C : kHeadCB;
    typename RX::raw xv[kN];
#pragma unroll
    for (int c = 0; c < kN; ++c)
      if (c0 + c < C) xv[c] = RX::template load<true>(xb + (size_t)(c0 + c) * S);
#pragma unroll
    for (int c = 0; c < kN; ++c) {
      if (c0 + c < C) {
        float xf[V];
#pragma unroll
        for (int v = 0; v < V; ++v) xf[v] = RX::get(xv[c], v);
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const float w = W[d * C + c0 + c];
#pragma unroll
          for (int v = 0; v < V; ++v) a[d][v] = fmaf(w, xf[v], a[d][v]);
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) HeadRow<TE, V>::template store<false>(eb + (size_t)d * S, a[d]);  // the affinity kernels read it next
}

// dx[b,c,p] = sum_d W[d,c] de[b,d,p], rounded once into TX.  A launch of its own for the reason k_head_dx gives.
template <int C, int D, typename TX, typename TE, int V>
__global__ __launch_bounds__(kHeadBlock) void k_head16_dx(const float* __restrict__ W, const TE* __restrict__ de, TX* __restrict__ dx,
                                                          long long S, int chunks_per_b) {
  using RE = HeadRow<TE, V>;
  const int b = blockIdx.x / chunks_per_b;
  const long long p = ((long long)(blockIdx.x - b * chunks_per_b) * kHeadBlock + threadIdx.x) * V;
  if (p >= S) return;
  const TE* deb = de + (size_t)b * D * S + p;
  TX* dxb = dx + (size_t)b * C * S + p;
  float dv[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const typename RE::raw r = RE::template load<false>(deb + (size_t)d * S);  // read again by k_head16_dw
#pragma unroll
    for (int v = 0; v < V; ++v) dv[d][v] = RE::get(r, v);
  }
  constexpr int kCB = kHeadCB / V;  // accumulators held at a time: kHeadCB registers in either form
  for (int c0 = 0; c0 < C; c0 += kCB) {
    constexpr int kN = C < kCB ? C : kCB;
    float dxv[kN][V];
#pragma unroll
    for (int c = 0; c < kN; ++c)
#pragma unroll
      for (int v = 0; v < V; ++v) dxv[c][v] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int c = 0; c < kN; ++c)
        if (c0 + c < C) {
          const float w = W[d * C + c0 + c];
#pragma unroll
          for (int v = 0; v < V; ++v) dxv[c][v] = fmaf(w, dv[d][v], dxv[c][v]);
        }
#pragma unroll
    for (int c = 0; c < kN; ++c)
      if (c0 + c < C) HeadRow<TX, V>::template store<true>(dxb + (size_t)(c0 + c) * S, dxv[c]);
  }
}

// partials[wg][D*C + D] as k_head_dw writes them (same tiles, same reduction, same residency).  A chunk is 256 * V pixels; the
// packed rows go through the tiles one half at a time.
// workgroups per CU that the registers allow: those of k_head_dw, except that two f32 de pixels per lane (D dwordx2 rows next to the
// C packed x rows) leave room for four only up to C = 32
constexpr int head16_dw_resident(int C, int D, bool e_f32, int V) {
  return (C <= 48 && D == 16 && !(e_f32 && V == 2 && C > 32)) ? 4 : (C <= 128 ? 2 : 1);
}

template <int C, int D, typename TX, typename TE, int V>
__global__ __launch_bounds__(kHeadBlock, head16_dw_resident(C, D, std::is_same<TE, float>::value, V)) void k_head16_dw(
    const TX* __restrict__ x, const TE* __restrict__ de, float* __restrict__ partials, long long S, int chunks_per_b, int nchunks) {
  static_assert(D % 16 == 0, "the dW tiles are 16 x 16");
  constexpr bool kAll = C <= kHeadCB;  // every row of the chunk requested up front (else 16 channels at a time)
  static_assert(kAll || V == 1, "the channel-chunked heads load x inside the tile loop: element form only");
  using RX = HeadRow<TX, V>;
  using RE = HeadRow<TE, V>;
  constexpr int DT = D / 16, CC = (C + 15) / 16, NW = kHeadBlock / 64;
  constexpr int kTileA = D * kHeadRow, kTileB = 16 * kHeadRow;
  constexpr int kRed = D * CC * 16;
  constexpr int kLds = (NW * (kTileA + kTileB) > NW * kRed + NW * D) ? NW * (kTileA + kTileB) : NW * kRed + NW * D;
  __shared__ float lds[kLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tA = lds + wave * (kTileA + kTileB);
  float* tB = tA + kTileA;
  const int mi = lane & 15, mk = lane >> 4;

  hv4 acc[DT][CC];
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int j = 0; j < CC; ++j) acc[i][j] = hv4{0.f, 0.f, 0.f, 0.f};
  float dbv[D];
#pragma unroll
  for (int d = 0; d < D; ++d) dbv[d] = 0.f;

  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {  // uniform trip count per workgroup
    const int b = chunk / chunks_per_b;
    const long long p = ((long long)(chunk - b * chunks_per_b) * kHeadBlock + threadIdx.x) * V;
    const bool live = p < S;  // V = 2: S is even, both pixels or neither
    const size_t pc = live ? (size_t)p : 0;  // clamped address, value masked below
    const TE* deb = de + (size_t)b * D * S + pc;
    const TX* xb = x + (size_t)b * C * S + pc;
    typename RE::raw dv[D];
    typename RX::raw xv[kAll ? C : 16];
#pragma unroll
    for (int d = 0; d < D; ++d) dv[d] = RE::template load<true>(deb + (size_t)d * S);
    if (kAll) {
#pragma unroll
      for (int c = 0; c < C; ++c) xv[c] = RX::template load<true>(xb + (size_t)c * S);
    }
    // not unrolled: the halves take their turn through the same registers (unrolled, both halves were widened up front and the
    // C <= 48 instantiations no longer fitted the 128 registers of four workgroups per CU)
#pragma unroll 1
    for (int h = 0; h < V; ++h) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const float v = live ? RE::get(dv[d], h) : 0.f;
        dbv[d] += v;
        tA[d * kHeadRow + lane] = v;
      }
      __builtin_amdgcn_wave_barrier();
      float av[DT][16];
#pragma unroll
      for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int s = 0; s < 16; ++s) av[i][s] = tA[(16 * i + mi) * kHeadRow + 4 * s + mk];
#pragma unroll
      for (int j = 0; j < CC; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 16 * j + r;
          if (!kAll) {
            if (c < C) xv[r] = RX::template load<true>(xb + (size_t)c * S);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 16 * j + r;
          tB[r * kHeadRow + lane] = (c < C && live) ? RX::get(xv[kAll ? (c < C ? c : 0) : r], h) : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float bv = tB[mi * kHeadRow + 4 * s + mk];
#pragma unroll
          for (int i = 0; i < DT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][s], bv, acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();  // the next writes of tB (and of tA, for the last j) come after these reads
      }
    }
  }

  // ---- workgroup partial: sum the waves' tiles in wave order (as k_head_dw)
  __syncthreads();
  float* red = lds;               // [NW][kRed]
  float* redb = lds + NW * kRed;  // [NW][D]
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int j = 0; j < CC; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * kRed + (16 * i + 4 * mk + r) * (16 * CC) + 16 * j + mi] = acc[i][j][r];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float s = wave_sum63(dbv[d]);
    if (lane == 63) redb[wave * D + d] = s;
  }
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * (D * C + D);
  for (int t = threadIdx.x; t < D * C; t += kHeadBlock) {
    const int d = t / C, c = t - d * C;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w * kRed + d * (16 * CC) + c];
    out[t] = s;
  }
  if (threadIdx.x < D) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += redb[w * D + threadIdx.x];
    out[D * C + threadIdx.x] = s;
  }
}

// ---- launchers, instantiated once per 16-bit type ---------------------------------------------------------------------------------
template <typename TX, typename TE, int V>
void head16_launch_fwd(int C, int D, dim3 grid, hipStream_t s, const void* x, const float* W, const float* bias, void* e, size_t S, int chunks) {
#define PEA_HEAD16_F(c, d)                                                                                                          \
  if (C == c && D == d)                                                                                                             \
    hipLaunchKernelGGL((k_head16_fwd<c, d, TX, TE, V>), grid, dim3(kHeadBlock), 0, s, (const TX*)x, W, bias, (TE*)e, (long long)S, chunks);
  PEA_HEAD16_CASES(PEA_HEAD16_F)
#undef PEA_HEAD16_F
}

template <typename TX, typename TE, int V>
void head16_launch_dx(int C, int D, dim3 grid, hipStream_t s, const float* W, const void* de, void* dx, size_t S, int chunks) {
#define PEA_HEAD16_X(c, d)                                                                                                          \
  if (C == c && D == d)                                                                                                             \
    hipLaunchKernelGGL((k_head16_dx<c, d, TX, TE, V>), grid, dim3(kHeadBlock), 0, s, W, (const TE*)de, (TX*)dx, (long long)S, chunks);
  PEA_HEAD16_CASES(PEA_HEAD16_X)
#undef PEA_HEAD16_X
}

template <typename TX, typename TE, int V>
void head16_launch_dw(int C, int D, int nwg, hipStream_t s, const void* x, const void* de, float* partials, size_t S, int chunks, int nchunks) {
#define PEA_HEAD16_B(c, d)                                                                                                           \
  if (C == c && D == d) {                                                                                                            \
    if constexpr (V == 1 || c <= kHeadCB)                                                                                            \
      hipLaunchKernelGGL((k_head16_dw<c, d, TX, TE, V>), dim3((unsigned)nwg), dim3(kHeadBlock), 0, s, (const TX*)x, (const TE*)de,  \
                         partials, (long long)S, chunks, nchunks);                                                                   \
  }
  PEA_HEAD16_CASES(PEA_HEAD16_B)
#undef PEA_HEAD16_B
}

// chunks of 256 * V pixels per batch item; false if B of them do not fit one grid
inline bool head16_chunks(int B, size_t S, int V, size_t* chunks) {
  *chunks = (S + (size_t)kHeadBlock * V - 1) / ((size_t)kHeadBlock * V);
  return *chunks * (size_t)B <= 0x7fffffffULL;
}

template <typename TX>
int head16_fwd(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s) {
  // the packed form: every plane base + p on a dword (an f32 e: on two)
  const int V = (S % 2 == 0 && !misaligned(x, 4) && !misaligned(e, e_f32 ? 8 : 4)) ? 2 : 1;
  size_t chunks;
  if (!head16_chunks(B, S, V, &chunks)) return PEA_E_UNSUPPORTED;
  const dim3 grid((unsigned)(chunks * B));
  if (e_f32) (V == 2 ? head16_launch_fwd<TX, float, 2> : head16_launch_fwd<TX, float, 1>)(C, D, grid, s, x, W, bias, e, S, (int)chunks);
  else (V == 2 ? head16_launch_fwd<TX, TX, 2> : head16_launch_fwd<TX, TX, 1>)(C, D, grid, s, x, W, bias, e, S, (int)chunks);
  return hip_rc();
}

template <typename TX>
int head16_bwd(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW, float* db,
               float* partials, hipStream_t s) {
  const bool even = S % 2 == 0 && !misaligned(de, e_f32 ? 8 : 4);
  const int Vx = (even && !misaligned(dx, 4)) ? 2 : 1;
  // dW: chosen from x and de alone, so the sums do not depend on whether dx is asked for
  const int Vw = (even && !misaligned(x, 4) && C <= kHeadCB) ? 2 : 1;
  size_t chunks_x, chunks_w;
  if (!head16_chunks(B, S, Vx, &chunks_x) || !head16_chunks(B, S, Vw, &chunks_w)) return PEA_E_UNSUPPORTED;
  if (dx) {
    const dim3 grid((unsigned)(chunks_x * B));
    if (e_f32) (Vx == 2 ? head16_launch_dx<TX, float, 2> : head16_launch_dx<TX, float, 1>)(C, D, grid, s, W, de, dx, S, (int)chunks_x);
    else (Vx == 2 ? head16_launch_dx<TX, TX, 2> : head16_launch_dx<TX, TX, 1>)(C, D, grid, s, W, de, dx, S, (int)chunks_x);
  }
  const int nchunks = (int)(chunks_w * B);
  // a multiple of the CU count that the instantiation keeps resident, no partial round (as pea_head_bwd)
  const int per_cu = (head16_dw_resident(C, D, e_f32, Vw) == 4 ? 4 : 2) * device_cus();
  const int nwg = nchunks < per_cu ? (nchunks < kHeadMaxWg ? nchunks : kHeadMaxWg) : (per_cu < kHeadMaxWg ? per_cu : kHeadMaxWg);
  if (e_f32) (Vw == 2 ? head16_launch_dw<TX, float, 2> : head16_launch_dw<TX, float, 1>)(C, D, nwg, s, x, de, partials, S, (int)chunks_w, nchunks);
  else (Vw == 2 ? head16_launch_dw<TX, TX, 2> : head16_launch_dw<TX, TX, 1>)(C, D, nwg, s, x, de, partials, S, (int)chunks_w, nchunks);
  const int rc = hip_rc();
  if (rc) return rc;
  const int n = D * C + D;
  hipLaunchKernelGGL(k_head_finalize, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, partials, nwg, D * C, n, dW, db);
  return hip_rc();
}

}  // namespace pea
