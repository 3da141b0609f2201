// pea_head.h -- the per-pixel embedding head: the 1x1 (1x1x1) convolution that turns the decoder's C feature channels
// into the D-dimensional embedding, e[b,d,p] = bias[d] + sum_c W[d,c] * x[b,c,p], and its backward, on f32 features
// (include/pea.h) and on f16 / bf16 features (include/pea_head16.h: x and dx in the 16-bit type, e and de in the same type or
// in f32, W / bias / dW / db always f32).
// Reference: OutConv, scripts_cvppp/model/unet2d_residual.py:67-74 (outconv_emb :307, applied :346; same class in
// scripts_bbbc039v1/model/unet2d_residual.py:67,235); 3D: conv3dBlock(.., [(1,1,1)]) out_put*,
// scripts_ac3ac4/model/model_superhuman.py:437-441, applied :486-490; the same lines under torch.autocast or on a .half() /
// .bfloat16() feature map.  The step immediately before the path.
// Included by pea_k_head.hip (f32) and pea_k_head16{,_f16,_bf16}.hip (one translation unit per 16-bit type).
//
// Every kernel streams: one lane per pixel, planar [B,C,S] / [B,D,S] tensors, every access a coalesced 256-byte row of
// one channel.  They are HBM-bound (f32: forward 4(C+D) bytes per pixel, backward 4(2C+D)); the arithmetic (2CD flops per
// pixel forward, 4CD backward) is a fraction of the memory time.  W is read through the scalar cache (uniform addresses,
// compile-time offsets), so the forward and dx are plain v_fmac with an SGPR operand.  dW = sum_p de[:,p] x[:,p]^T is
// the one contraction over PIXELS here and goes to the matrix cores: v_mfma_f32_16x16x4_f32 (exact f32, k-ordered fma
// chain) with A = de[16 d x 4 px], B = x[4 px x 16 c]; the pixel-per-lane registers are turned into that operand
// layout through a per-wave LDS tile (row stride 68 floats: both the pixel-major write and the (l%16, l/16) read are
// bank-conflict free).  Deterministic: lane-private / wave-private accumulators, per-workgroup partial sums, fixed-order
// final reduction.
//
// The backward kernels (k_head_dx, k_head_dw) are written once for every storage type: HeadRow<T, V> is the one place that knows
// how V x-adjacent elements of T are loaded, widened and stored.  f32 features always run V = 1.  What 2-byte elements change:
//   * row width.  One pixel per lane would make every wave access a 128-byte row.  The PACKED form (V = 2) gives a lane two
//     x-adjacent pixels: one dword per lane and channel, the 256-byte rows of the f32 kernels at half the pixels' bytes.  It needs
//     every plane base + p to be 4-byte aligned (8 for an f32 e / de, moved as dwordx2): S even and the tensor bases aligned.  With
//     S odd the planes of odd channels sit 2 bytes off, so the host picks the ELEMENT form (V = 1, one ushort per lane) for those
//     calls and for skewed pointers; the answer is the same, only the speed differs.
//   * working form.  The loaded rows stay packed in registers (C dwords for 2C pixels-times-channels); a value is widened once, when
//     its channel is consumed (f16: v_cvt_f32_f16 on the selected half, bf16: a shift / a mask), and feeds D (forward) or kN (dx)
//     f32 accumulators per pixel.  Every product and sum is f32 with the f32 W; a 16-bit result is rounded once, to nearest even.
//   * dW.  The packed rows are handed to the MFMA tiles one half at a time (which pixel lands in which k slot is free as long as
//     de and x agree), so the tile code and its LDS footprint do not depend on the form.  16-bit values are exact in f32, the
//     products and sums are those of f32 features.  The wide heads (C > kHeadCB, coarse scales) load x 16 channels at a time inside
//     the tile loop and keep the element form.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "pea_host.h"
#include "pea_epilogue.h"  // wave_sum63

namespace pea {

typedef float hv4 __attribute__((ext_vector_type(4)));
typedef float hv2 __attribute__((ext_vector_type(2)));
constexpr int kHeadBlock = 256;    // 4 waves
constexpr int kHeadMaxWg = 1024;   // backward: workgroups (= partial sums of dW / db)
constexpr int kHeadRow = 68;       // LDS row stride (floats) of a [channel][64 px] tile
constexpr int kHeadCB = 64;        // input channels held in registers at a time (the wide low-resolution heads are chunked)

// (C, D) pairs of the reference's heads: ResUNet 32 / 64 / 128 / 256 -> 16 (CVPPP) or 32 (BBBC039V1),
// superhuman 3D U-Net 28 / 36 / 48 / 64 / 80 -> 16.  Every storage type serves the same pairs.
#define PEA_HEAD_CASES(X) \
  X(28, 16) X(32, 16) X(36, 16) X(48, 16) X(64, 16) X(80, 16) X(128, 16) X(256, 16) X(32, 32) X(64, 32) X(128, 32) X(256, 32)

inline bool head_supported(int C, int D) {
#define PEA_HEAD_Q(c, d) if (C == c && D == d) return true;
  PEA_HEAD_CASES(PEA_HEAD_Q)
#undef PEA_HEAD_Q
  return false;
}

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

// ---- the forward: two kernels, on purpose --------------------------------------------------------------------------------------
// Both add in the same order per accumulator (bias first, then c ascending), so on the same values they give the same bits.  They
// differ in the loop nest.  k_head_fwd (f32 x) is d-outer: one running accumulator over the loaded rows.  k_head16_fwd is c-outer
// with D x V live accumulators, so that each 16-bit value is widened once.  k_head16_fwd<C, D, float, float, 1> is a valid f32
// forward, but its D accumulators live next to the loaded rows.  VGPRs / waves per SIMD, k_head_fwd<C, D> against it (compiled for
// gfx950, no scratch in either): 32->16 50 / 8 against 61 / 8, 32->32 47 / 7 against 88 / 5, 64->32 71 / 7 against 120 / 4,
// 80->16 86 / 5 against 166 / 3, 128->32 122 / 4 against 184 / 2, 256->32 122 / 4 against 152 / 3.
// Serving f32 features from the c-outer form is a question about the forward's registers, not a restatement: the two stay apart.
template <int C, int D>
__global__ __launch_bounds__(kHeadBlock) void k_head_fwd(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ e, long long S,
                                                         int chunks_per_b) {
  const int b = blockIdx.x / chunks_per_b;
  const long long p = (long long)(blockIdx.x - b * chunks_per_b) * kHeadBlock + threadIdx.x;
  if (p >= S) return;
  const float* xb = x + (size_t)b * C * S + p;
  float* eb = e + (size_t)b * D * S + p;
  const bool has_bias = bias != nullptr;
  if (C <= kHeadCB) {
    float xv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = __builtin_nontemporal_load(xb + (size_t)c * S);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float a = has_bias ? bias[d] : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) a = fmaf(W[d * C + c], xv[c], a);
      eb[(size_t)d * S] = a;  // the affinity kernels read it next: keep it in the caches
    }
  } else {  // wide heads (C = 80 / 128 / 256 at the coarse scales): D accumulators, kHeadCB channels at a time
    float a[D];
#pragma unroll
    for (int d = 0; d < D; ++d) a[d] = has_bias ? bias[d] : 0.f;
    for (int c0 = 0; c0 < C; c0 += kHeadCB) {
      constexpr int kN = kHeadCB;
      float xv[kN];
#pragma unroll
      for (int c = 0; c < kN; ++c) xv[c] = (c0 + c < C) ? __builtin_nontemporal_load(xb + (size_t)(c0 + c) * S) : 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int c = 0; c < kN; ++c)
          if (c0 + c < C) a[d] = fmaf(W[d * C + c0 + c], xv[c], a[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) eb[(size_t)d * S] = a[d];
  }
}

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

// ---- the backward: one dx and one dw kernel for every storage type ----------------------------------------------------------------
// dx[b,c,p] = sum_d W[d,c] de[b,d,p], rounded once into TX: a streaming kernel of its own (like the forward: loads, 2CD flops,
// stores, exit).  Fused with the dW kernel below it ran 1.6x slower than the two together: vmcnt retires in order, so the next
// pixels' loads of a looping workgroup wait for the acknowledgements of the dx stores before them.
template <int C, int D, typename TX, typename TE, int V>
__global__ __launch_bounds__(kHeadBlock) void k_head_dx(const float* __restrict__ W, const TE* __restrict__ de, TX* __restrict__ dx,
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
    const typename RE::raw r = RE::template load<false>(deb + (size_t)d * S);  // read again by k_head_dw: no non-temporal hint
#pragma unroll
    for (int v = 0; v < V; ++v) dv[d][v] = RE::get(r, v);
  }
  constexpr int kCB = kHeadCB / V;  // accumulators held at a time: kHeadCB registers in either form
  for (int c0 = 0; c0 < C; c0 += kCB) {  // one pass for C <= kCB
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

// workgroups of k_head_dw per CU that the registers allow: four for C <= 48, D = 16, except that two f32 de pixels per lane (D
// dwordx2 rows next to the C packed x rows) leave room for four only up to C = 32
constexpr int head_dw_resident(int C, int D, bool e_f32, int V) {
  return (C <= 48 && D == 16 && !(e_f32 && V == 2 && C > 32)) ? 4 : (C <= 128 ? 2 : 1);
}

// partials[wg][D*C + D] = this workgroup's share of dW[d,c] = sum_{b,p} de[b,d,p] x[b,c,p] and db[d] = sum_{b,p} de[b,d,p].
// Loads only.  What it needs is rows in flight (HBM latency under load is several times the ~1 us a wave spends on 256
// pixels): D + C rows per wave, head_dw_resident workgroups per CU.  Prefetching the next 256 pixels instead (twice the
// registers, half the waves) was slower: 114 vs 9x us.  A chunk is 256 * V pixels; the packed rows go through the tiles one half
// at a time.
template <int C, int D, typename TX, typename TE, int V>
__global__ __launch_bounds__(kHeadBlock, head_dw_resident(C, D, std::is_same<TE, float>::value, V)) void k_head_dw(
    const TX* __restrict__ x, const TE* __restrict__ de, float* __restrict__ partials, long long S, int chunks_per_b, int nchunks) {
  static_assert(D % 16 == 0, "the dW tiles are 16 x 16");
  constexpr bool kAll = C <= kHeadCB;  // every row of the chunk requested up front (else 16 channels at a time)
  static_assert(kAll || V == 1, "the channel-chunked heads load x inside the tile loop: element form only");
  using RX = HeadRow<TX, V>;
  using RE = HeadRow<TE, V>;
  constexpr int DT = D / 16, CC = (C + 15) / 16, NW = kHeadBlock / 64;
  constexpr int kTileA = D * kHeadRow, kTileB = 16 * kHeadRow;
  constexpr int kRed = D * CC * 16;  // one wave's dW tile set, [d][16*CC]
  // per wave: A tile (de, [D][68]) + B tile (16 channels of x, [16][68]); reused as [NW][kRed] for the final reduction
  constexpr int kLds = (NW * (kTileA + kTileB) > NW * kRed + NW * D) ? NW * (kTileA + kTileB) : NW * kRed + NW * D;
  __shared__ float lds[kLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tA = lds + wave * (kTileA + kTileB);
  float* tB = tA + kTileA;
  const int mi = lane & 15, mk = lane >> 4;  // MFMA operand coordinates of this lane: row / column mi, k index mk

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
    const size_t pc = live ? (size_t)p : 0;  // clamped address, value masked below: no branches around the loads
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
      // A operands of the 16 k-steps (4 pixels each), kept for every channel chunk
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

  // ---- workgroup partial: sum the waves' tiles in wave order
  __syncthreads();
  float* red = lds;               // [NW][kRed]
  float* redb = lds + NW * kRed;  // [NW][D]
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int j = 0; j < CC; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C/D layout: row = 4 * (lane >> 4) + r, column = lane & 15
        red[wave * kRed + (16 * i + 4 * mk + r) * (16 * CC) + 16 * j + mi] = acc[i][j][r];
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

// dW[d,c], db[d] = sum over the workgroup partials in a fixed order.  One workgroup per 16 outputs: thread (o, g) adds
// the partials of workgroups g, g + 16, g + 32, ... (64-byte coalesced reads, nwg / 16 loads per thread instead of nwg:
// a thread per output walking all 1024 partials took 75 us, longer than the kernel that produced them), then the 16
// group sums are added in group order.
static __global__ __launch_bounds__(256) void k_head_finalize(const float* __restrict__ partials, int nwg, int dc, int n,
                                                       float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int t = blockIdx.x * 16 + o;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four independent chains: loads in flight, still a fixed order
  if (t < n) {
    int w = g;
    for (; w + 48 < nwg; w += 64) {
      s0 += partials[(size_t)w * n + t];
      s1 += partials[(size_t)(w + 16) * n + t];
      s2 += partials[(size_t)(w + 32) * n + t];
      s3 += partials[(size_t)(w + 48) * n + t];
    }
    for (; w < nwg; w += 16) s0 += partials[(size_t)w * n + t];
  }
  red[g][o] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (threadIdx.x < 16 && t < n) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][o];
    if (t < dc) dW[t] = s;
    else if (db) db[t - dc] = s;
  }
}

// ---- launchers, instantiated once per feature type (TX = float: pea_k_head.hip) -----------------------------------------------------
// f32 features have the element form only
template <typename TX, int V>
constexpr bool kHeadForm = V == 1 || !std::is_same<TX, float>::value;

template <typename TX, typename TE, int V>
void head16_launch_fwd(int C, int D, dim3 grid, hipStream_t s, const void* x, const float* W, const float* bias, void* e, size_t S, int chunks) {
#define PEA_HEAD_F(c, d)                                                                                                            \
  if (C == c && D == d)                                                                                                             \
    hipLaunchKernelGGL((k_head16_fwd<c, d, TX, TE, V>), grid, dim3(kHeadBlock), 0, s, (const TX*)x, W, bias, (TE*)e, (long long)S, chunks);
  PEA_HEAD_CASES(PEA_HEAD_F)
#undef PEA_HEAD_F
}

template <typename TX, typename TE, int V>
void head_launch_dx(int C, int D, dim3 grid, hipStream_t s, const float* W, const void* de, void* dx, size_t S, int chunks) {
#define PEA_HEAD_X(c, d)                                                                                                            \
  if (C == c && D == d) {                                                                                                           \
    if constexpr (kHeadForm<TX, V>)                                                                                                 \
      hipLaunchKernelGGL((k_head_dx<c, d, TX, TE, V>), grid, dim3(kHeadBlock), 0, s, W, (const TE*)de, (TX*)dx, (long long)S, chunks); \
  }
  PEA_HEAD_CASES(PEA_HEAD_X)
#undef PEA_HEAD_X
}

template <typename TX, typename TE, int V>
void head_launch_dw(int C, int D, int nwg, hipStream_t s, const void* x, const void* de, float* partials, size_t S, int chunks, int nchunks) {
#define PEA_HEAD_B(c, d)                                                                                                            \
  if (C == c && D == d) {                                                                                                           \
    if constexpr (kHeadForm<TX, V> && (V == 1 || c <= kHeadCB))                                                                     \
      hipLaunchKernelGGL((k_head_dw<c, d, TX, TE, V>), dim3((unsigned)nwg), dim3(kHeadBlock), 0, s, (const TX*)x, (const TE*)de,    \
                         partials, (long long)S, chunks, nchunks);                                                                   \
  }
  PEA_HEAD_CASES(PEA_HEAD_B)
#undef PEA_HEAD_B
}

// chunks of 256 * V pixels per batch item; false if B of them do not fit one grid
inline bool head_chunks(int B, size_t S, int V, size_t* chunks) {
  *chunks = (S + (size_t)kHeadBlock * V - 1) / ((size_t)kHeadBlock * V);
  return *chunks * (size_t)B <= 0x7fffffffULL;
}

template <typename TX>
int head16_fwd(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s) {
  // the packed form: every plane base + p on a dword (an f32 e: on two)
  const int V = (S % 2 == 0 && !misaligned(x, 4) && !misaligned(e, e_f32 ? 8 : 4)) ? 2 : 1;
  size_t chunks;
  if (!head_chunks(B, S, V, &chunks)) return PEA_E_UNSUPPORTED;
  const dim3 grid((unsigned)(chunks * B));
  if (e_f32) (V == 2 ? head16_launch_fwd<TX, float, 2> : head16_launch_fwd<TX, float, 1>)(C, D, grid, s, x, W, bias, e, S, (int)chunks);
  else (V == 2 ? head16_launch_fwd<TX, TX, 2> : head16_launch_fwd<TX, TX, 1>)(C, D, grid, s, x, W, bias, e, S, (int)chunks);
  return hip_rc();
}

// the backward of every entry point (arguments validated by the caller; TX = float comes with e_f32 = true)
template <typename TX>
int head_bwd(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW, float* db,
             float* partials, hipStream_t s) {
  const bool even = kHeadForm<TX, 2> && S % 2 == 0 && !misaligned(de, e_f32 ? 8 : 4);
  const int Vx = (even && !misaligned(dx, 4)) ? 2 : 1;
  // dW: chosen from x and de alone, so the sums do not depend on whether dx is asked for
  const int Vw = (even && !misaligned(x, 4) && C <= kHeadCB) ? 2 : 1;
  size_t chunks_x, chunks_w;
  if (!head_chunks(B, S, Vx, &chunks_x) || !head_chunks(B, S, Vw, &chunks_w)) return PEA_E_UNSUPPORTED;
  if (dx) {
    const dim3 grid((unsigned)(chunks_x * B));
    if (e_f32) (Vx == 2 ? head_launch_dx<TX, float, 2> : head_launch_dx<TX, float, 1>)(C, D, grid, s, W, de, dx, S, (int)chunks_x);
    else (Vx == 2 ? head_launch_dx<TX, TX, 2> : head_launch_dx<TX, TX, 1>)(C, D, grid, s, W, de, dx, S, (int)chunks_x);
  }
  const int nchunks = (int)(chunks_w * B);
  // dW: a multiple of the CU count that the instantiation keeps resident, no partial round
  const int per_cu = (head_dw_resident(C, D, e_f32, Vw) == 4 ? 4 : 2) * device_cus();
  const int nwg = nchunks < per_cu ? (nchunks < kHeadMaxWg ? nchunks : kHeadMaxWg) : (per_cu < kHeadMaxWg ? per_cu : kHeadMaxWg);
  if (e_f32) (Vw == 2 ? head_launch_dw<TX, float, 2> : head_launch_dw<TX, float, 1>)(C, D, nwg, s, x, de, partials, S, (int)chunks_w, nchunks);
  else (Vw == 2 ? head_launch_dw<TX, TX, 2> : head_launch_dw<TX, TX, 1>)(C, D, nwg, s, x, de, partials, S, (int)chunks_w, nchunks);
  const int rc = hip_rc();
  if (rc) return rc;
  const int n = D * C + D;
  hipLaunchKernelGGL(k_head_finalize, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, partials, nwg, D * C, n, dW, db);
  return hip_rc();
}

// what pea_k_head16.hip calls; one translation unit per 16-bit type defines its pair (pea_k_head16_f16.hip, pea_k_head16_bf16.hip).
// Arguments are validated by the caller; PEA_OK, PEA_E_UNSUPPORTED (more chunks than one grid holds) or a HIP error.
int head16_fwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s);
int head16_fwd_bf16(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s);
int head16_bwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW,
                   float* db, float* partials, hipStream_t s);
int head16_bwd_bf16(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW,
                    float* db, float* partials, hipStream_t s);

}  // namespace pea
