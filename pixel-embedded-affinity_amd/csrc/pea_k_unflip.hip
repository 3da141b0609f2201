// pea_k_unflip.hip -- the per-sample un-flip of the EMA embedding (include/pea_flip.h): what convert_consistency_flip does between the
// second backbone forward and the EMA cross loss (scripts_cvppp/data/data_consistency.py:19-45, scripts_ac3ac4/utils/
// consistency_aug.py:58-77, 217-228) as ONE launch that reads every element once and writes it once, the rules read on the device.
//
// A workgroup of 256 threads (four waves) serves a 64 x 64 tile of one OUTPUT plane (b, c, z); the grid is one-dimensional over
// planes x tiles, x tiles fastest.  The workgroup's facts -- its plane, its tile and its sample's rule bits -- depend on blockIdx
// alone: the rules are read once, from an address the whole wave shares, and every branch on them is uniform.  Pure data movement:
// the element travels as an integer of its size (uint32_t / uint16_t), so NaN payloads and -0 arrive as they left.
//
//   no transpose   row by row.  Wave w takes rows w, w + 4, ..; lane l writes column x0 + l and reads column x' = x0 + l or
//                  X-1 - (x0 + l): descending across the wave when rx is set, the same 64 consecutive elements (the same cache
//                  lines) either way.  All sixteen loads of a lane are issued before its first store.
//   transpose      (Y == X) out[y][x] = src[x'][y']: the source tile is loaded coalesced along the SOURCE's x -- lane l holds
//                  y = y0 + l, the wave's row index j is the output column x0 + j -- into the LDS tile s_t[j][l], and after a barrier
//                  read as s_t[l][i] by the lane that writes column x0 + l of output row y0 + i, coalesced along the output's x.
//                  The tile is [64][65] dwords (16 640 bytes: nine workgroups per CU by LDS, eight by waves); 16-bit elements are
//                  widened to a dword container, so both storage widths take the same path.
//                  Banks (ds_write_b32 and ds_read_b32: bank = (a / 4) % 32, conflicts within a 32-lane half only): the write's
//                  dword address is 65 j + l with j wave-uniform, 32 consecutive dwords per half, 32 distinct banks: conflict-free.
//                  The read's is 65 l + i with i wave-uniform: 65 = 2 * 32 + 1, so the bank is (l + i) % 32, distinct for the 32
//                  lanes of a half: conflict-free.  (At a row stride of 64 the read would be a 32-way conflict.)  The same for the
//                  widened 16-bit elements: 0 conflicts.
//   rt with Y != X the sample's whole output is filled with NaN (pea_flip.h); uniform per workgroup like the other two.
// The LDS tile is a static allocation of the kernel, so the workgroups of the other two paths hold their 16 640 bytes unused: the
// paths are chosen on the device, per sample, and one launch serves them all.  It costs no occupancy (eight workgroups per CU by
// waves, nine by LDS).  `rules` may not overlap dst (pea_flip.h: the caller's responsibility), hence __restrict__ on all three.
#include "../../include/pea_flip.h"
#include "pea_dispatch.h"

using namespace pea;

namespace {

constexpr int kTile = 64;                     // the tile's edge = the wave's width
constexpr int kRows = kTile / (kBlock / 64);  // rows of the tile per wave: 16
static_assert(kBlock == 256, "four waves share a 64 x 64 tile");

// rule i of the table: set = nonzero (pea_flip.h)
__device__ __forceinline__ bool rule_set(const void* __restrict__ rules, int rdt, size_t i) {
  if (rdt == PEA_RULES_U8) return ((const uint8_t*)rules)[i] != 0;
  if (rdt == PEA_RULES_I32) return ((const int32_t*)rules)[i] != 0;
  if (rdt == PEA_RULES_I64) return ((const long long*)rules)[i] != 0;
  return ((const float*)rules)[i] != 0.f;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_unflip(const T* __restrict__ src, T* __restrict__ dst, const void* __restrict__ rules,
                                                   int rdt, int nrules, int C, int Z, int Y, int X, unsigned ty, unsigned tx, T nan) {
  __shared__ uint32_t s_t[kTile][kTile + 1];
  // blockIdx -> (b, c, z, tile row, tile column): everything here is uniform over the workgroup
  unsigned t = blockIdx.x;
  const unsigned txi = t % tx; t /= tx;
  const unsigned tyi = t % ty; t /= ty;
  const unsigned z = t % (unsigned)Z; t /= (unsigned)Z;
  const unsigned c = t % (unsigned)C;
  const size_t b = t / (unsigned)C;
  const size_t r0 = b * (size_t)nrules;
  const bool rz = nrules == 4 && rule_set(rules, rdt, r0);
  const bool rx = rule_set(rules, rdt, r0 + (size_t)(nrules - 3));
  const bool ry = rule_set(rules, rdt, r0 + (size_t)(nrules - 2));
  const bool rt = rule_set(rules, rdt, r0 + (size_t)(nrules - 1));

  const size_t plane = (size_t)Y * (size_t)X, sX = (size_t)X, sY = (size_t)Y;
  const size_t bc = b * (size_t)C + c;
  const T* __restrict__ sp = src + (bc * (size_t)Z + (rz ? (size_t)Z - 1 - z : (size_t)z)) * plane;
  T* __restrict__ dp = dst + (bc * (size_t)Z + z) * plane;
  const size_t y0 = (size_t)tyi * kTile, x0 = (size_t)txi * kTile;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t x = x0 + lane;  // the output column this lane writes

  if (!rt) {
    const size_t xs = rx ? sX - 1 - x : x;
    T v[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const size_t y = y0 + wave + 4 * k;
      v[k] = (y < sY && x < sX) ? sp[(ry ? sY - 1 - y : y) * sX + xs] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const size_t y = y0 + wave + 4 * k;
      if (y < sY && x < sX) dp[y * sX + x] = v[k];
    }
    return;
  }
  if (Y != X) {  // a transpose of a non-square plane: the whole sample is NaN
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const size_t y = y0 + wave + 4 * k;
      if (y < sY && x < sX) dp[y * sX + x] = nan;
    }
    return;
  }
  {  // out[y][x] = src[x'][y'], Y == X
    const size_t yl = y0 + lane;                 // the output row whose source element this lane loads: source column y'
    const size_t xsrc = ry ? sY - 1 - yl : yl;
    T v[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const size_t xj = x0 + wave + 4 * k;       // the output column = source row x'
      v[k] = (xj < sX && yl < sY) ? sp[(rx ? sX - 1 - xj : xj) * sX + xsrc] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k) s_t[wave + 4 * k][lane] = (uint32_t)v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int i = wave + 4 * k;
      const size_t y = y0 + i;
      if (y < sY && x < sX) dp[y * sX + x] = (T)s_t[lane][i];
    }
  }
}

}  // namespace

extern "C" int pea_consistency_unflip(int B, int C, int Z, int Y, int X, int dtype, const void* src, void* dst, const void* rules,
                                      int rules_dtype, int nrules, void* stream) {
  if (B < 1 || C < 1 || Z < 1 || Y < 1 || X < 1) return PEA_E_DESC;
  if (dtype != PEA_F32 && dtype != PEA_F16 && dtype != PEA_BF16) return PEA_E_DESC;
  if (rules_dtype < PEA_RULES_U8 || rules_dtype > PEA_RULES_F32 || (nrules != 3 && nrules != 4)) return PEA_E_DESC;
  if (!src || !dst || !rules) return PEA_E_NULL;
  const size_t es = dtype_bytes(dtype);
  const size_t rs = rules_dtype == PEA_RULES_U8 ? 1 : rules_dtype == PEA_RULES_I64 ? 8 : 4;
  if (misaligned(src, es) || misaligned(dst, es) || misaligned(rules, rs)) return PEA_E_ALIGN;
  uint64_t bytes = es;
  for (int v : {B, C, Z, Y, X}) bytes = mul_sat(bytes, (uint64_t)v);
  const uint64_t s0 = (uint64_t)(uintptr_t)src, d0 = (uint64_t)(uintptr_t)dst;
  if (s0 < add_sat(d0, bytes) && d0 < add_sat(s0, bytes)) return PEA_E_DESC;
  const uint64_t ty = ((uint64_t)Y + kTile - 1) / kTile, tx = ((uint64_t)X + kTile - 1) / kTile;
  uint64_t tiles = mul_sat(ty, tx);
  for (int v : {B, C, Z}) tiles = mul_sat(tiles, (uint64_t)v);
  if (tiles > 0x7fffffffULL) return PEA_E_UNSUPPORTED;

  const dim3 grid((unsigned)tiles), blk(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PEA_F32)
    hipLaunchKernelGGL(k_unflip<uint32_t>, grid, blk, 0, s, (const uint32_t*)src, (uint32_t*)dst, rules, rules_dtype, nrules, C, Z, Y,
                       X, (unsigned)ty, (unsigned)tx, (uint32_t)0x7fc00000u);
  else
    hipLaunchKernelGGL(k_unflip<uint16_t>, grid, blk, 0, s, (const uint16_t*)src, (uint16_t*)dst, rules, rules_dtype, nrules, C, Z, Y,
                       X, (unsigned)ty, (unsigned)tx, (uint16_t)(dtype == PEA_F16 ? 0x7e00u : 0x7fc0u));
  return hip_rc();
}
