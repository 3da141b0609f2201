// pea_stage.h -- what every LDS-staged ("cross", "march", "box") kernel rests on, stated once: which pixels of the cross a lane
// moves per plane (cross_stage), where a neighbour sits in the staged plane (cross_slots), the LDS-DMA instructions of one plane
// (cross_dma) and the hand-off between the DMA and the gather (loads_barrier and its siblings).  Included by pea_xdma.h.
//
// The region of a tile (pea_xdma.h has the picture): VF, rows of TW pixels, then the strip rows of SW pixels; a plane holds it as
// QA quads (4 x-adjacent pixels, 16 bytes), QV of them in VF.  Blocks of 64 quads go round the waves: wave w moves block w and
// block NW + w (NW = TH * TW / 64 waves), one dwordx4 LDS-DMA instruction each -- 1 KiB per wave instruction, block s at byte
// s * 1024 of the plane.
#pragma once
#include <utility>

#include "pea_tiled.h"

namespace pea {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// ------------------------------------------------------------------------------------------------------------------
// staging geometry
// ------------------------------------------------------------------------------------------------------------------
// region quad q (UNIT = 4 pixels) or oct q (UNIT = 8: the 16-bit planes) -> the byte offset of its first pixel in an image plane of
// BYTES-byte elements, kOOB where the border rule has no pixel (CROP) or q lies beyond the region; act: q lies inside the region
template <int TW, bool CROP, int UNIT, int BYTES, typename CP>
__device__ __forceinline__ unsigned cross_item(const KParams& P, const CP& C, int y0, int x0, int q, bool& act) {
  constexpr int SH = UNIT == 8 ? 1 : 0;  // an oct is two quads
  int gy, gx;
  if (q < (C.QV >> SH)) {
    gy = y0 - C.hy0 + (int)((unsigned)q / (TW / UNIT));
    gx = x0 + UNIT * (int)((unsigned)q % (TW / UNIT));
  } else {
    const int k = q - (C.QV >> SH);
    const int sh = (C.SW == 64 ? 4 : 3) - SH;  // items per strip row
    const int cc = UNIT * (k & ((1 << sh) - 1));
    gy = y0 + (k >> sh);
    gx = cc < C.split ? x0 + TW + cc : x0 - C.SW + cc;
  }
  act = q < (C.QA >> SH);
  bool oky, okx;
  gy = wrap1<CROP>(gy, P.Y, oky);
  gx = wrap1<CROP>(gx, P.X, okx);
  return (act && oky && okx) ? (unsigned)(gy * P.X + gx) * (unsigned)BYTES : kOOB;
}

// The (up to) two quads a lane moves per f32 plane.  vo: byte offset of the quad in the image plane; act: the lane's quad lies in
// the region (a lane beyond it must write nothing: its 16 bytes would land in the next plane); wbase / w1: where the wave's two
// blocks go inside an LDS plane; npc: the DMA instructions this wave issues per plane PAIR (a chunk) -- a block without a live
// lane is skipped --, which is what the hand-off has to count.
// UNCOND (the 3D instantiations and the march): every wave issues BOTH slots for every plane, unconditionally -- a wave without a
// second block repeats its first one (same bytes to the same place), the tail lanes of the last block write zeros into the plane's
// padding (plan_xdma sizes it in whole blocks).  npc is then a compile-time 4, which is what lets the compiler wait for loads of
// its own with vmcnt(4) instead of vmcnt(0): with a DMA inside an `if` it has to assume that none was issued.
template <bool UNCOND = false>
struct CrossStage {
  unsigned vo[2];
  bool act[2];
  int wbase, w1, npc;
};
template <int TH, int TW, bool CROP, bool UNCOND = false, typename CP>
__device__ __forceinline__ CrossStage<UNCOND> cross_stage(const KParams& P, const CP& C, int y0, int x0, int wave, int lane) {
  constexpr int NW = TH * TW / 64;
  CrossStage<UNCOND> g;
#pragma unroll
  for (int s = 0; s < 2; ++s) g.vo[s] = cross_item<TW, CROP, 4, 4>(P, C, y0, x0, (s * NW + wave) * 64 + lane, g.act[s]);
  g.wbase = wave * 1024;
  g.w1 = g.wbase + NW * 1024;
  if (UNCOND) {
    const bool two = __builtin_amdgcn_readfirstlane((NW + wave) * 64 < C.QA);
    if (!two) { g.vo[1] = g.vo[0]; g.w1 = g.wbase; }
    g.npc = 4;
  } else {
    g.npc = 2 * ((__builtin_amdgcn_ballot_w64(g.act[0]) != 0) + (__builtin_amdgcn_ballot_w64(g.act[1]) != 0));
  }
  return g;
}

// The one oct a lane moves per 16-bit plane (8 pixels = 16 bytes; X % 8 == 0: inside or outside as a whole): half the bytes, one
// block per wave and plane.  vo in bytes of a 16-bit plane; npc as above (2 or 0).
struct CrossStage8 {
  unsigned vo;
  bool act;
  int wbase, npc;
};
template <int TH, int TW, bool CROP, typename CP>
__device__ __forceinline__ CrossStage8 cross_stage8(const KParams& P, const CP& C, int y0, int x0, int wave, int lane) {
  CrossStage8 g;
  g.vo = cross_item<TW, CROP, 8, 2>(P, C, y0, x0, wave * 64 + lane, g.act);
  g.wbase = wave * 1024;
  g.npc = 2 * (__builtin_amdgcn_ballot_w64(g.act) != 0);
  return g;
}

// ------------------------------------------------------------------------------------------------------------------
// the LDS slot of the in-plane neighbours: byte offsets inside a staged f32 plane
// ------------------------------------------------------------------------------------------------------------------
// a neighbour column c = lx + d outside the tile sits in the strip at coordinate (c & mask): the bank it would have inside the tile
template <int TW>
__device__ __forceinline__ int cross_slot_x(int vown, int hrow, int lx, int d, int mask) {
  const int c = lx + d;
  return (unsigned)c < (unsigned)TW ? vown + d * 4 : hrow + (c & mask) * 4;
}
// backward: the (offset, role) pairs along x and along y.  Returns vown, the lane's own pixel.
template <int TW, int XP, typename CP>
__device__ __forceinline__ int cross_slots(const CP& C, int ly, int lx, int (&ax)[XP], int (&ay)[XP]) {
  const int vown = ((C.hy0 + ly) * TW + lx) * 4;
  const int hrow = (C.QV * 4 + ly * C.SW) * 4;
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    ax[k] = cross_slot_x<TW>(vown, hrow, lx, C.xd[k], C.xm[k]);
    ay[k] = vown + C.yd[k] * TW * 4;
  }
  return vown;
}
// forward: the offsets in their own order (unused offsets: d = 0, the own slot)
template <int TW, int NXP, typename CP>
__device__ __forceinline__ int cross_slots(const CP& C, int ly, int lx, int (&an)[NXP]) {
  const int vown = ((C.hy0 + ly) * TW + lx) * 4;
  const int hrow = (C.QV * 4 + ly * C.SW) * 4;
#pragma unroll
  for (int k = 0; k < NXP; ++k) {
    const int d = C.fd[k];
    an[k] = C.fax[k] ? cross_slot_x<TW>(vown, hrow, lx, d, C.fm[k]) : vown + d * TW * 4;
  }
  return vown;
}

// ------------------------------------------------------------------------------------------------------------------
// the DMA issue
// ------------------------------------------------------------------------------------------------------------------
// one dwordx4 LDS-DMA instruction of this wave: 64 lanes x 16 bytes from (rsrc, per-lane vo, scalar so) to dst .. dst + 1 KiB.
// A kernel's loads beside the cross (the own tile, an oct plane) go through it and into the kernel's own count.
__device__ __forceinline__ void cross_dma1(const rsrc_t rsrc, char* dst, unsigned vo, unsigned so) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)dst, 16, vo, so, 0, 0);
}
// one plane of the cross, from plane offset `so` to byte `plane_byte` of the LDS
template <bool UNCOND>
__device__ __forceinline__ void cross_dma(const CrossStage<UNCOND>& g, const rsrc_t rsrc, char* lds, int plane_byte, unsigned so) {
  if (UNCOND || g.act[0]) cross_dma1(rsrc, lds + plane_byte + g.wbase, g.vo[0], so);
  if (UNCOND || g.act[1]) cross_dma1(rsrc, lds + plane_byte + g.w1, g.vo[1], so);
}
__device__ __forceinline__ void cross_dma(const CrossStage8& g, const rsrc_t rsrc, char* lds, int plane_byte, unsigned so) {
  if (g.act) cross_dma1(rsrc, lds + plane_byte + g.wbase, g.vo, so);
}

// ------------------------------------------------------------------------------------------------------------------
// the hand-off:  s_waitcnt vmcnt(N) lgkmcnt(0);  s_barrier
// ------------------------------------------------------------------------------------------------------------------
// "What this wave requested up to N loads ago has landed, and every wave is done with the buffer behind the barrier."
//  * N counts LOADS only: the load instructions (DMA and plain) this wave issued AFTER the one that has to have landed.  Loads
//    retire in order among themselves, so "at most N outstanding" means the older ones are complete.  Stores sit on the same
//    counter but may retire before an older load (LLVM's waitcnt pass treats a gfx9 vmcnt with loads and stores pending as out of
//    order for the same reason): counted in -- "only these may still fly" -- they let a wait pass with part of the awaited chunk
//    in flight whenever stores had retired early.  In the march backward that made the gradient differ between identical launches
//    at 17 k of 403 M values.  With loads only, outstanding stores make a wait a little longer,
//    never shorter.  For the same reason a smaller N than the exact one is always sound: it only waits for more.
//  * N is a literal: the immediate of s_waitcnt is part of the instruction.  A count that is known only at run time (how many of
//    its two blocks a wave moves) goes through a ladder over the values it can take (loads_barrier_among).
template <int N>
__device__ __forceinline__ void loads_barrier() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a six-bit field");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
// without the barrier: a wave that waits for loads into its own registers, or drains its look-ahead before it ends
template <int N>
__device__ __forceinline__ void loads_landed() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a six-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int... Ns>
constexpr bool descending() {
  const int v[] = {Ns..., 0};
  for (unsigned i = 0; i + 1 < sizeof(v) / sizeof(v[0]); ++i)
    if (v[i] <= v[i + 1]) return false;
  return true;
}
// run-time n (wave-uniform) over the listed steps Ns, descending: the largest step <= n, else 0.
// idle: this wave issues no DMA at all (the region has fewer blocks than the workgroup has waves), so it has no load to wait for --
// vmcnt(0) would make it drain its own STORES at every chunk and hold everybody's barrier: it takes the barrier alone.
template <int... Ns>
__device__ __forceinline__ void loads_barrier_among(int n, bool idle = false) {
  static_assert(descending<Ns...>(), "steps: positive, largest first");
  if (idle) lds_barrier();
  else if (!((n >= Ns && (loads_barrier<Ns>(), true)) || ...)) loads_barrier<0>();
}
// the same over the steps MAX, MAX - STEP, .., STEP: a ring of RB buffers leaves up to RB - 2 chunks of STEP-wise counted loads in flight
template <int MAX, int STEP, int... Is>
__device__ __forceinline__ void loads_barrier_upto_(int n, bool idle, std::integer_sequence<int, Is...>) {
  loads_barrier_among<(MAX - STEP * Is)...>(n, idle);
}
template <int MAX, int STEP>
__device__ __forceinline__ void loads_barrier_upto(int n, bool idle = false) {
  static_assert(MAX > 0 && MAX % STEP == 0, "whole steps");
  loads_barrier_upto_<MAX, STEP>(n, idle, std::make_integer_sequence<int, MAX / STEP>{});
}
template <int... Ns>
__device__ __forceinline__ void loads_landed_among(int n) {
  static_assert(descending<Ns...>(), "steps: positive, largest first");
  if (!((n >= Ns && (loads_landed<Ns>(), true)) || ...)) loads_landed<0>();
}

}  // namespace pea
