// pea_xdma_pf.h -- the cross backward with the projection known FIRST (round 3).
//
//   d e(p) = dl / n(p) * ( G(p) - ehat(p) <ehat(p), G(p)> ),     G(p) = sum over (offset, role) pairs of c_k ehat(q_k)
//
// k_bwd_xdma (pea_xdma.h) learns <ehat, G> only after the last channel chunk, so it keeps G (D registers) -- and for D > 16 has no
// registers left for ehat and reads the own pixel AGAIN from global memory at the end: at D = 64 that is a second pass over e
// (605 MB at the bench shape; e does not fit the Infinity Cache), 64 one-dword loads and 64 one-dword stores per lane in the tail.
// The ablation that found it (profiles/microbench/stamp_bwd.hip): with BOTH the gather and the chunk DMA compiled out the D = 64
// backward still takes 282 of 430 us.
//
// But  <ehat(p), ehat(q_k)>  is the affinity of the pair -- a_i(p) for role A, a_i(p - o_i) for role B -- which the forward wrote:
//
//   <ehat(p), G(p)> = sum_i [ g_i(p) a_i(p) + g_i(p - o_i) a_i(p - o_i) ]
//
// needs no embedding channel at all: 2K more loads next to the 2K g loads of the prologue (same addresses, the affs tensor).
// With the projection in hand a chunk FINISHES its two channels: (acc - ehat_c proj) * dl / n is stored right away.  No G array, no
// kept ehat, no second read of e; ~70 VGPRs instead of 104-126, so stencils whose cross fits 7 KB planes (reach <= 11: BBBC039V1,
// the K = 8 table of configs[4], the deep-supervision scales) run THREE workgroups per CU; every width takes 10 pairs per axis.
// Needs the RAW cosine map (no activation flag on the forward's affs output): pea_affinity_bwd_ex2(.., affs, ..).
// Self loss, in-plane stencils (no z offsets), f32 storage here; f16 storage: k_bwd_xdma_h<.., PF> (pea_xdma_h16.h).
#pragma once
#include "pea_xdma.h"

namespace pea {

// RB: buffers of the ring (3: two chunks in flight beside the one being gathered; more where the planes are small -- a store has
// to be acknowledged RB - 1 chunk periods after it was issued, or the next hand-off waits for it).  The hand-offs (pea_stage.h) leave
// the DMA of up to RB - 2 chunks in flight: a ladder over the counts this wave can have issued for them.
template <int D_T, int TH, int TW, int PSU, bool CROP, int WPE, int RB = 3>
__global__ __launch_bounds__(TH* TW, WPE) void k_bwd_xdma_pf(const KParams P, const XParams C, const float* __restrict__ xt,
                                                              const float* __restrict__ invp, const float* __restrict__ gin,
                                                              const float* __restrict__ affs, const float* __restrict__ dloss,
                                                              float* __restrict__ dx) {
  constexpr int NT = TH * TW, PS = PSU * 256, NP = D_T / 2, XP = kXP, IP = 2 * (RB - 1);  // IP: the plane the 1 / norm plane sits in first
  static_assert(TW == 32 && D_T % 2 == 0 && RB >= 3 && NP >= RB, "lane mapping / channel pairs / ring");
  extern __shared__ f4 lds4[];
  char* lds = (char*)lds4;
  int tile, b, z, y0, x0;
  if (!xdma_tile<TH, TW>(C, P, tile, b, z, y0, x0)) return;
  const size_t S = (size_t)P.S;
  const unsigned YX = (unsigned)(P.Y * P.X);
  const rsrc_t xB = mkbuf(xt + (size_t)b * D_T * S), dB = mkbuf(dx + (size_t)b * D_T * S);
  const rsrc_t gB = mkbuf(gin + (size_t)b * P.K * S), iB = mkbuf(invp + (size_t)b * S), aB = mkbuf(affs + (size_t)b * P.K * S);
  const unsigned ecs = (unsigned)P.S * 4u, ezo = (unsigned)z * YX * 4u;
  const float dl = dloss ? dloss[0] : 1.f;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31;
  const int py = y0 + ly, px = x0 + lx;
  const bool live = py < P.Y && px < P.X;
  const unsigned po4 = (unsigned)(py * P.X + px) * 4u;
  const unsigned pe = live ? po4 : kOOB;

  // ---- the (up to) two quads this lane moves per plane
  const CrossStage<> ST = cross_stage<TH, TW, CROP>(P, C, y0, x0, wave, lane);
  const int npc = ST.npc;
  cross_dma(ST, iB, lds, IP * PS, ezo);
  cross_dma(ST, xB, lds, 0, ezo);
  cross_dma(ST, xB, lds, PS, ezo + ecs);

  // ---- g and the affinity of every pair (role A at p, role B at p - o): the coefficients, and the projection
  const unsigned pg = live ? po4 : 0xC0000000u;
  float cx[XP], cy[XP];
  int ax[XP], ay[XP];
  float proj = 0.f;
  const int vown = cross_slots<TW>(C, ly, lx, ax, ay);
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    const int go = C.xgo[k];
    const int t = px + go;
    const bool out = (unsigned)t >= (unsigned)P.X;
    const int fix = go > 0 ? -P.X : P.X;
    const unsigned o = CROP ? (out ? kOOB : pg + (unsigned)(go * 4)) : pg + (unsigned)((out ? go + fix : go) * 4);
    const unsigned so = ezo + (unsigned)C.xgi[k] * ecs;
    cx[k] = bl32(gB, k < C.npx ? o : kOOB, so);
    proj = fmaf(cx[k], bl32(aB, k < C.npx ? o : kOOB, so), proj);
  }
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    const int go = C.ygo[k];
    const int t = py + go;
    const bool out = (unsigned)t >= (unsigned)P.Y;
    const int fix = go > 0 ? -P.Y : P.Y;
    const unsigned o = CROP ? (out ? kOOB : pg + (unsigned)(go * P.X * 4)) : pg + (unsigned)((out ? go + fix : go) * P.X * 4);
    const unsigned so = ezo + (unsigned)C.ygi[k] * ecs;
    cy[k] = bl32(gB, k < C.npy ? o : kOOB, so);
    proj = fmaf(cy[k], bl32(aB, k < C.npy ? o : kOOB, so), proj);
  }
#pragma unroll
  for (int c = 1; c <= RB - 2; ++c) {  // chunks 1 .. RB - 2 into their buffers (the last buffer holds the 1 / norm plane for now)
    cross_dma(ST, xB, lds, 2 * c * PS, ezo + (unsigned)(2 * c) * ecs);
    cross_dma(ST, xB, lds, (2 * c + 1) * PS, ezo + (unsigned)(2 * c + 1) * ecs);
  }
  // inv, chunk 0, g and affs have landed (the DMA instructions of chunks 1 .. RB - 2 may still fly)
  loads_barrier_upto<4 * (RB - 2), 2>((RB - 2) * npc);

  const float invo = *(const float*)(lds + IP * PS + vown);
  const float inv_own = fabsf(invo);
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    cx[k] *= fabsf(*(const float*)(lds + IP * PS + ax[k]));
    cy[k] *= fabsf(*(const float*)(lds + IP * PS + ay[k]));
    asm volatile("" : "+v"(cx[k]), "+v"(cy[k]));
  }
  if (invo < 0.f) proj = 0.f;  // clamp branch of F.normalize: d ehat / d e = I / eps
  asm volatile("" : "+v"(proj));
  lds_barrier();  // the inv plane is dead: the last buffer may be filled
  cross_dma(ST, xB, lds, IP * PS, ezo + (unsigned)(2 * (RB - 1)) * ecs);
  cross_dma(ST, xB, lds, (IP + 1) * PS, ezo + (unsigned)(2 * (RB - 1) + 1) * ecs);
  const float sc = dl * inv_own;

#pragma unroll
  for (int ps = 0; ps < NP; ++ps) {
    const int bo = (ps % RB) * 2 * PS;
    f2 o;
    o.x = *(const float*)(lds + bo + vown);
    o.y = *(const float*)(lds + bo + PS + vown);
    f2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < XP; ++k) {
      f2 v;
      v.x = *(const float*)(lds + bo + ax[k]);
      v.y = *(const float*)(lds + bo + PS + ax[k]);
      acc = __builtin_elementwise_fma((f2){cx[k], cx[k]}, v, acc);
      if (k % 5 == 4) asm volatile("" ::: "memory");  // bound the ds_read hoisting
    }
#pragma unroll
    for (int k = 0; k < XP; ++k) {
      f2 v;
      v.x = *(const float*)(lds + bo + ay[k]);
      v.y = *(const float*)(lds + bo + PS + ay[k]);
      acc = __builtin_elementwise_fma((f2){cy[k], cy[k]}, v, acc);
      if (k % 5 == 4) asm volatile("" ::: "memory");
    }
    // this chunk's two channels are final: (G - ehat <ehat, G>) dl / n
    const float pq = proj * inv_own;
    float vx = (acc.x - o.x * pq) * sc, vy = (acc.y - o.y * pq) * sc;
    asm volatile("" : "+v"(vx), "+v"(vy));  // (stored behind the hand-off: there the stores have a chunk's time to retire)
    if (ps + 1 < NP) {
      // chunk ps + 1 has landed; younger than it: the DMA of chunks ps + 2 .. ps + RB - 1 (those that exist) and the stores of the
      // last min(ps + 1, RB - 1) chunks, which are not counted (pea_stage.h); everyone is done with buffer ps % RB
      const int nd = (ps + RB - 1 < NP ? ps + RB - 1 : NP - 1) - (ps + 1);
      loads_barrier_upto<4 * (RB - 2), 2>(nd * npc, npc == 0);
      if (ps + RB < NP) {
        cross_dma(ST, xB, lds, bo, ezo + (unsigned)(2 * (ps + RB)) * ecs);
        cross_dma(ST, xB, lds, bo + PS, ezo + (unsigned)(2 * (ps + RB) + 1) * ecs);
      }
    }
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vx), dB, pe, ezo + (unsigned)(2 * ps) * ecs, kAuxNT);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vy), dB, pe, ezo + (unsigned)(2 * ps + 1) * ecs, kAuxNT);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The cross loss with a DETACHED second operand (ema_embedding_loss, scripts_cvppp/loss/loss_embedding_mse.py:79-95 behind
// convert_consistency_flip's detach) at D > 16: role A only,
//     G(p) = sum_i g_i(p) ehat_other(p + o_i),     <ehat(p), G(p)> = sum_i g_i(p) a_i(p)      (every pair, exactly)
// so the projection-first form needs nothing but the K values of g and of the raw map at the own pixel.  xt / invp are the SECOND
// operand and its 1 / norm plane (staged: the one-sided cross of plan_xdma mode 2); the own pixel -- needed raw, two channels per
// chunk, to finish them -- is staged as the own TILE (no halo: 2 KB per channel, the first two waves move it) beside each chunk;
// own_inv: the own operand's signed 1 / norm plane.  No accumulate form (the caller adds two buffers).
// ------------------------------------------------------------------------------------------------------------------
template <int D_T, int TH, int TW, int PSU, bool CROP, int WPE, int RB = 3>
__global__ __launch_bounds__(TH* TW, WPE) void k_bwd_xdma_pfo(const KParams P, const XParams C, const float* __restrict__ xt,
                                                               const float* __restrict__ invp, const float* __restrict__ own,
                                                               const float* __restrict__ own_inv, const float* __restrict__ gin,
                                                               const float* __restrict__ affs, const float* __restrict__ dloss,
                                                               float* __restrict__ dx) {
  constexpr int NT = TH * TW, PS = PSU * 256, NP = D_T / 2, XP = kXP, IP = 2 * (RB - 1), OWNB = 2 * RB * PS;
  static_assert(TW == 32 && D_T % 2 == 0 && RB >= 3 && NP >= RB && NT == 512, "lane mapping / channel pairs / ring");
  extern __shared__ f4 lds4[];
  char* lds = (char*)lds4;
  int tile, b, z, y0, x0;
  if (!xdma_tile<TH, TW>(C, P, tile, b, z, y0, x0)) return;
  const size_t S = (size_t)P.S;
  const unsigned YX = (unsigned)(P.Y * P.X);
  const rsrc_t xB = mkbuf(xt + (size_t)b * D_T * S), dB = mkbuf(dx + (size_t)b * D_T * S), oB = mkbuf(own + (size_t)b * D_T * S);
  const rsrc_t gB = mkbuf(gin + (size_t)b * P.K * S), iB = mkbuf(invp + (size_t)b * S), aB = mkbuf(affs + (size_t)b * P.K * S);
  const rsrc_t oiB = mkbuf(own_inv + (size_t)b * S);
  const unsigned ecs = (unsigned)P.S * 4u, ezo = (unsigned)z * YX * 4u;
  const float dl = dloss ? dloss[0] : 1.f;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31;
  const int py = y0 + ly, px = x0 + lx;
  const bool live = py < P.Y && px < P.X;
  const unsigned pe = live ? (unsigned)(py * P.X + px) * 4u : kOOB;

  const CrossStage<> ST = cross_stage<TH, TW, CROP>(P, C, y0, x0, wave, lane);
  const bool ownw = wave < NT / 256;  // uniform: the waves that move the own tile (quads 0 .. 127)
  unsigned ownvo = kOOB;
  {
    const int q = (int)threadIdx.x, qy = y0 + (q >> 3), qx = x0 + 4 * (q & 7);
    ownvo = (q < NT / 4 && qy < P.Y && qx < P.X) ? (unsigned)(qy * P.X + qx) * 4u : kOOB;
  }
  const int npc = ST.npc + (ownw ? 2 : 0);
// chunk c: the second operand's cross into ring buffer c % RB, the own tile into its 4 KB slot
#define PEA_PFCHUNK(c)                                                                                                            \
  {                                                                                                                              \
    cross_dma(ST, xB, lds, (2 * ((c) % RB)) * PS, ezo + (unsigned)(2 * (c)) * ecs);                                              \
    cross_dma(ST, xB, lds, (2 * ((c) % RB) + 1) * PS, ezo + (unsigned)(2 * (c) + 1) * ecs);                                      \
    if (ownw) {                                                                                                                  \
      cross_dma1(oB, lds + OWNB + (2 * ((c) % RB)) * 2048 + wave * 1024, ownvo, ezo + (unsigned)(2 * (c)) * ecs);                \
      cross_dma1(oB, lds + OWNB + (2 * ((c) % RB) + 1) * 2048 + wave * 1024, ownvo, ezo + (unsigned)(2 * (c) + 1) * ecs);        \
    }                                                                                                                            \
  }
  // the second operand's 1 / norm plane sits in the LAST buffer's first plane until the coefficients are done; chunk 0 .. RB - 2
  cross_dma(ST, iB, lds, IP * PS, ezo);
  PEA_PFCHUNK(0)

  // ---- g and the raw affinity at the own pixel: the coefficients, and the projection
  float cx[XP], cy[XP];
  int ax[XP], ay[XP];
  float proj = 0.f;
  cross_slots<TW>(C, ly, lx, ax, ay);
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    const unsigned so = ezo + (unsigned)C.xgi[k] * ecs;
    cx[k] = bl32(gB, k < C.npx ? pe : kOOB, so);
    proj = fmaf(cx[k], bl32(aB, k < C.npx ? pe : kOOB, so), proj);
  }
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    const unsigned so = ezo + (unsigned)C.ygi[k] * ecs;
    cy[k] = bl32(gB, k < C.npy ? pe : kOOB, so);
    proj = fmaf(cy[k], bl32(aB, k < C.npy ? pe : kOOB, so), proj);
  }
  const float invo = bl32(oiB, pe, ezo);
#pragma unroll
  for (int c = 1; c <= RB - 2; ++c) PEA_PFCHUNK(c)
  loads_barrier_upto<6 * (RB - 2), 2>((RB - 2) * npc);  // inv, chunk 0, g, affs and the own 1 / norm have landed (chunks 1 .. RB - 2 may still fly)

  const float inv_own = fabsf(invo);
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    cx[k] *= fabsf(*(const float*)(lds + IP * PS + ax[k]));
    cy[k] *= fabsf(*(const float*)(lds + IP * PS + ay[k]));
    asm volatile("" : "+v"(cx[k]), "+v"(cy[k]));
  }
  if (invo < 0.f) proj = 0.f;  // clamp branch of F.normalize
  asm volatile("" : "+v"(proj));
  lds_barrier();  // the inv plane is dead: the last buffer may be filled
  PEA_PFCHUNK(RB - 1)
  const float sc = dl * inv_own;
  const float pq = proj * inv_own;

#pragma unroll
  for (int ps = 0; ps < NP; ++ps) {
    const int bo = (ps % RB) * 2 * PS;
    f2 o;  // the own pixel, raw
    o.x = *(const float*)(lds + OWNB + (2 * (ps % RB)) * 2048 + (int)threadIdx.x * 4);
    o.y = *(const float*)(lds + OWNB + (2 * (ps % RB) + 1) * 2048 + (int)threadIdx.x * 4);
    f2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < XP; ++k) {
      f2 v;
      v.x = *(const float*)(lds + bo + ax[k]);
      v.y = *(const float*)(lds + bo + PS + ax[k]);
      acc = __builtin_elementwise_fma((f2){cx[k], cx[k]}, v, acc);
      if (k % 5 == 4) asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int k = 0; k < XP; ++k) {
      f2 v;
      v.x = *(const float*)(lds + bo + ay[k]);
      v.y = *(const float*)(lds + bo + PS + ay[k]);
      acc = __builtin_elementwise_fma((f2){cy[k], cy[k]}, v, acc);
      if (k % 5 == 4) asm volatile("" ::: "memory");
    }
    float vx = __builtin_fmaf(-o.x, pq, acc.x) * sc, vy = __builtin_fmaf(-o.y, pq, acc.y) * sc;
    asm volatile("" : "+v"(vx), "+v"(vy));
    if (ps + 1 < NP) {
      const int nd = (ps + RB - 1 < NP ? ps + RB - 1 : NP - 1) - (ps + 1);  // chunks requested behind the one that has to have landed
      loads_barrier_upto<6 * (RB - 2), 2>(nd * npc, npc == 0);
      if (ps + RB < NP) PEA_PFCHUNK(ps + RB)
    }
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vx), dB, pe, ezo + (unsigned)(2 * ps) * ecs, kAuxNT);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vy), dB, pe, ezo + (unsigned)(2 * ps + 1) * ecs, kAuxNT);
  }
#undef PEA_PFCHUNK
}

}  // namespace pea
