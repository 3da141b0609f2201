// pea_segtable.h -- the contingency table of two label images, stated once for pea_k_segscore.hip (include/pea_segscore.h) and
// pea_k_instscore.hip (include/pea_instscore.h): the streaming pass over the pixels that builds the joint histogram n_ij, the slot
// helpers of its open-addressing tables, and the wave-side integer and fixed-point sums into per-image words.  Both files keep their
// own workspace layout behind the two words that the pass itself writes (I_BAD, I_OVF of an image's kSegImgWords words).
//
// The pass over pixels is the segmented reduction of pea_k_disc.hip with a 64-bit key: a WAVE owns 256 consecutive pixels of one image,
// a lane one quad of four, and the wave PEELS its pairs -- it takes the key of the first lane that still has an open pixel, every lane
// closes its pixels of that key, the count is a butterfly of popcounts -- so neighbouring pixels, which mostly share their pair, cost
// one table update per (wave, distinct pair), not one per pixel.  The r-th peeled pair is kept by lane r, and the lanes then claim
// their slots side by side (one round of probes for the wave's pairs instead of a dependent chain per pair); a wave with more than 64
// pairs flushes and goes on.  There is no workgroup-side LDS table in front of the global one: at the shapes of the drivers a wave
// meets two to six pairs, so the four waves of a workgroup would save a handful of atomics per kilobyte of labels read.
//
// The tables.  Slot = hash(key) mod capacity, linear probing; the stored key is key + 1, so a zero word is an empty slot and the
// prepared workspace is all zero.  A slot is claimed with ONE compare-and-swap of the key word (empty -> key); whoever finds the key
// there, by that swap or by the load before it, adds to the slot's count words with integer atomics.  No lane ever waits for another
// lane: a probe that meets a foreign key moves on, and EVERY probe sequence ends after `capacity` slots, so a full table drops the
// pair (counted in n_overflow) and the kernel ends.  Lookups in later launches are plain loads behind the kernel boundary.
// Slot placement depends on arrival order; nothing that is summed in floating point runs over slots.
#pragma once
#include "pea_stream.h"

#pragma clang fp contract(off)

namespace pea {
namespace {

constexpr int kSegImgWords = 32;                // u64 words per image; the pass over pixels writes the first two
constexpr int kPairWords = 2;                   // per pair slot: key + 1, n_ij
constexpr u64 kMaxCapacity = 1ull << 31;
constexpr double kFx = 4294967296.0;            // 2^32: the fixed-point sums carry 32 fractional bits
enum { I_BAD = 0, I_OVF = 1 };                  // labels that are no ids; pixels of pairs that found no slot

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the slot of `key1` (a stored key: never 0) in a table of `cap` slots of W words, claiming an empty one; -1 after cap probes
template <int W>
__device__ __forceinline__ long long slot_claim(u64* __restrict__ tab, u64 cap, u64 key1) {
  u64 s = mix64(key1) & (cap - 1);
  for (u64 i = 0; i < cap; ++i) {
    u64* kp = tab + s * W;
    u64 cur = PEA_LD_AGENT(kp);
    if (cur == 0) {
      u64 expect = 0;
      if (__hip_atomic_compare_exchange_strong(kp, &expect, key1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return (long long)s;
      cur = expect;  // another lane took the slot: for the same key, or this probe moves on
    }
    if (cur == key1) return (long long)s;
    s = (s + 1) & (cap - 1);
  }
  return -1;
}
// the slot of `key1` in a table that an EARLIER launch filled; -1: not there
template <int W>
__device__ __forceinline__ long long slot_find(const u64* __restrict__ tab, u64 cap, u64 key1) {
  u64 s = mix64(key1) & (cap - 1);
  for (u64 i = 0; i < cap; ++i) {
    const u64 cur = tab[s * W];
    if (cur == key1) return (long long)s;
    if (cur == 0) return -1;
    s = (s + 1) & (cap - 1);
  }
  return -1;
}

// a lane's wave total / wave maximum into a per-image word (all 64 lanes call)
__device__ __forceinline__ void wave_add(u64* p, u64 v, int lane) {
  v = wave_sum(v);
  if (lane == 0 && v) PEA_ATOM_ADD(p, v);
}
__device__ __forceinline__ void wave_max_into(u64* p, u64 v, int lane) {
  v = wave_max(v);
  if (lane == 0 && v) PEA_ATOM_MAX(p, v);
}
// v >= 0, finite, below 2^63 -> fixed point with 32 fractional bits, truncated: lo = the fraction's digits, hi = the whole part
__device__ __forceinline__ void fx_split(double v, u64& lo, u64& hi) {
  hi = (u64)v;
  lo = (u64)((v - (double)hi) * kFx);
}
__device__ __forceinline__ void wave_add_fx(u64* p, double v, int lane) {
  u64 lo, hi;
  fx_split(v, lo, hi);
  wave_add(p, lo, lane);
  wave_add(p + 1, hi, lane);
}
// the two words of a fixed-point sum -> its value
__device__ __forceinline__ double fx_value(const u64* p) {
  const u64 hi = p[1] + (p[0] >> 32), lo = p[0] & 0xffffffffull;
  return (double)hi + (double)lo / kFx;
}

// ---- the joint histogram -----------------------------------------------------------------------------------------------------------------
// pred / gt: image 0 of the launch; img / pairs: the words and the table of image 0 of the launch (pea_seg_table launches one image).
// A negative label is no id (I_BAD, its pixel is skipped); kBounded: neither is a label above `hi`.
template <bool kBounded>
__global__ __launch_bounds__(kBlock) void k_seg_pairs(const size_t S, const unsigned chunks, const u64 cap, const int32_t* __restrict__ pred,
                                                      const int32_t* __restrict__ gt, u64* __restrict__ img, u64* __restrict__ pairs, const int hi) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(at.chunk, S, &w0)) return;
  const size_t i0 = w0 + (size_t)lane * kQuad;
  const int nv = quad_nv(i0, S);
  int lp[kQuad], lg[kQuad];
  ld_iquad(pred + b * S + (nv ? i0 : 0), nv, -1, lp);
  ld_iquad(gt + b * S + (nv ? i0 : 0), nv, -1, lg);
  u64 key[kQuad];
  unsigned open = 0;
  u64 bad = 0;
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    key[i] = 0;
    if (i < nv) {
      const bool okp = kBounded ? (unsigned)lp[i] <= (unsigned)hi : lp[i] >= 0, okg = kBounded ? (unsigned)lg[i] <= (unsigned)hi : lg[i] >= 0;
      bad += (u64)!okp + (u64)!okg;
      if (okp && okg) {
        key[i] = (((u64)(unsigned)lp[i] << 32) | (u64)(unsigned)lg[i]) + 1;
        open |= 1u << i;
      }
    }
  }
  u64* __restrict__ tab = pairs + b * cap * kPairWords;
  u64 mykey = 0, mycnt = 0, dropped = 0;
  const auto flush = [&]() {  // every lane that holds a peeled pair claims its slot and adds its count
    if (mykey) {
      const long long s = slot_claim<kPairWords>(tab, cap, mykey);
      if (s >= 0) PEA_ATOM_ADD(tab + s * kPairWords + 1, mycnt);
      else dropped += mycnt;
    }
    mykey = 0;
  };
  int r = 0;
  u64 cur;
  unsigned mm;
  while (peel(key, open, cur, mm)) {
    const u64 cnt = wave_sum((u64)__popc(mm));
    if (lane == r) { mykey = cur; mycnt = cnt; }
    if (++r == 64) { flush(); r = 0; }
  }
  flush();
  u64* w = img + b * kSegImgWords;
  wave_add(w + I_BAD, bad, lane);
  wave_add(w + I_OVF, dropped, lane);
}

// the 64 consecutive slots of a wave of a launch over B * cap slots lie in one image (capacity is a multiple of 64): -> false past
// the last image
__device__ __forceinline__ bool slot_of_lane(u64 cap, int B, size_t* b, size_t* s) {
  const size_t gs = (size_t)blockIdx.x * kBlock + threadIdx.x;
  *b = gs / cap;
  *s = gs - *b * cap;
  return *b < (size_t)B;
}

// workgroups of the pass over `images` images' S pixels and of a pass over their slots; false: a grid exceeds 2^31 - 1
inline bool seg_grids(uint64_t S, uint64_t capacity, uint64_t images, unsigned* chunks, unsigned* pixel_groups, unsigned* slot_groups) {
  const uint64_t sg = images * (capacity / kBlock + (capacity % kBlock ? 1 : 0));
  if (!stream_grid(S, images, kQuadRun, chunks, pixel_groups) || sg > 0x7fffffffULL) return false;
  *slot_groups = (unsigned)((images * capacity + kBlock - 1) / kBlock);
  return true;
}

}  // namespace
}  // namespace pea
