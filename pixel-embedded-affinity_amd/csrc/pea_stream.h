// pea_stream.h -- what a streaming kernel over a flat pixel range is made of, stated once for pea_k_metrics.hip, pea_k_fgmask.hip,
// pea_k_disc.hip and pea_k_segscore.hip, which keep their arithmetic and their launch sequences.  No product stands here: the files
// switch contraction off after their includes, and a product next to a sum would be compiled under another rule than its caller.
//   lane run   a workgroup owns kLaneRun = 4096 consecutive elements of one plane, a lane kSteps quads: element (step * 256 + lane) * 4
//              + e of the run, so a step of a wave is 1 KiB of an f32 tensor (lane_run)
//   quad run   a workgroup owns kQuadRun = 1024 elements, a lane ONE quad (quad_start); seen by waves, a WAVE owns kWaveRun = 256
//              consecutive elements and keeps them in registers (wave_start: the same element-to-lane assignment)
// and what the label kernels (pea_k_cc.hip, pea_k_ws.hip, pea_k_rag.hip, pea_k_instscore.hip, pea_k_segscore.hip) share beyond the walks:
//   scans      wave_scan_incl, block_scan_excl over int, u32 or u64: the workgroup's exclusive prefix
//   atomics    PEA_LD_AGENT / PEA_ST_AGENT / PEA_ATOM_MAX (relaxed, agent scope; PEA_ATOM_ADD: pea_loss.h), f32_ord / ord_f32
//   host       the table workspace, stream_grid, or_prepare_again, and LaunchChain: a launch entry as a straight list of launches
//              (the layout of a workspace: pea_carve.h through pea_host.h)
#pragma once
#include "pea_host.h"
#include "pea_quad.h"

namespace pea {

constexpr int kSteps = 4;                             // steps per lane of a lane run
constexpr int kLaneRun = kBlock * kQuad * kSteps;     // elements of one plane per workgroup of a lane run
constexpr int kWaveRun = 64 * kQuad;                  // elements of one plane per wave: one quad per lane
constexpr int kQuadRun = kBlock * kQuad;              // .. per workgroup where a lane takes one quad
static_assert(kQuadRun == kWaveRun * (kBlock / 64), "a workgroup's quad run is its four wave runs");
static_assert(kLaneRun < (1 << 24), "a workgroup's count is an exact f32 integer");

// the valid elements of the quad at i0 of a range of n (0 past the end)
__device__ __forceinline__ int quad_nv(size_t i0, size_t n) { return i0 >= n ? 0 : (n - i0 >= (size_t)kQuad ? kQuad : (int)(n - i0)); }

// ---- walks --------------------------------------------------------------------------------------------------------------------------
// blockIdx -> (plane, chunk of the plane's range): uniform over the workgroup
struct BlockAt { unsigned chunk, plane; };
__device__ __forceinline__ BlockAt block_at(unsigned chunks) { return {blockIdx.x % chunks, blockIdx.x / chunks}; }

// the lane run of chunk `chunk` of a range of n elements: body(i0, nv) for each of the lane's quads that begins inside the range
template <typename F>
__device__ __forceinline__ void lane_run(unsigned chunk, size_t n, F&& body) {
  const size_t run0 = (size_t)chunk * kLaneRun;
#pragma unroll 1
  for (int j = 0; j < kSteps; ++j) {
    const size_t i0 = run0 + ((size_t)j * kBlock + threadIdx.x) * kQuad;
    if (i0 >= n) break;
    body(i0, quad_nv(i0, n));
  }
}
// the lane's one quad of chunk `chunk` of a quad run (the caller leaves where it lies past the range)
__device__ __forceinline__ size_t quad_start(unsigned chunk) { return (size_t)chunk * kQuadRun + (size_t)threadIdx.x * kQuad; }
// the wave's first element (lane l's quad begins at *w0 + l * kQuad); false: past the range, the WHOLE wave leaves (it meets no other)
__device__ __forceinline__ bool wave_start(unsigned chunk, size_t S, size_t* w0) {
  *w0 = (size_t)chunk * kQuadRun + (size_t)(threadIdx.x >> 6) * kWaveRun;
  return *w0 < S;
}

// The quad cursor of a cropped walk: the lane's first element of a dense [outer][EY][EX] range is decoded once (two divisions), the
// next three are reached by stepping x -> y -> outer (z of a volume, the image of a batch of crops).
struct CropCursor {
  size_t o;
  unsigned y, x;
  __device__ __forceinline__ CropCursor(size_t i0, unsigned EY, unsigned EX) {
    const size_t plane = (size_t)EY * EX;
    o = i0 / plane;
    const size_t r = i0 - o * plane;
    y = (unsigned)(r / EX), x = (unsigned)(r - (size_t)y * EX);
  }
  __device__ __forceinline__ void step(unsigned EY, unsigned EX) {
    if (++x == EX) {
      x = 0;
      if (++y == EY) { y = 0; ++o; }
    }
  }
};

// ---- wave reductions: __shfl_xor butterflies, offsets 32, 16, .., 1 (a fixed order) ------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {  // float, int, u64
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int N>
__device__ __forceinline__ void wave_sums(float (&v)[N]) {  // N butterflies side by side, each in the order of wave_sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] += __shfl_xor(v[u], o, 64);
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// ---- relaxed agent-scope accesses of words that other workgroups write meanwhile (PEA_ATOM_ADD: pea_loss.h) ----------------------------
#define PEA_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PEA_ST_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PEA_ATOM_MAX(p, v) (void)__hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// the order-preserving unsigned image of an f32 and back
__device__ __forceinline__ unsigned f32_ord(float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_f32(unsigned o) { return __builtin_bit_cast(float, (o >> 31) ? (o ^ 0x80000000u) : ~o); }

// ---- scans: T is int, u32 or u64 ----------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// the exclusive prefix of v over the workgroup's lanes and the workgroup's total (the whole workgroup calls it: two barriers; four
// words of LDS per element type)
template <typename T>
__device__ __forceinline__ T block_scan_excl(T v, T* total) {
  static_assert(kBlock / 64 == 4, "written for four waves");
  __shared__ T s_wave[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_scan_incl(v, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  T before = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) before += w < wave ? s_wave[w] : 0;
  *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  __syncthreads();
  return before + incl - v;
}
// The end of a streaming reduction of N sums per lane: a wave reduces each with wave_sum, the four waves meet in LDS and lane 0 of the
// workgroup hands sum k, ((p0 + p1) + p2) + p3 of the waves' partials, to f(k, v).  The whole workgroup calls it (a barrier).
template <int N, typename F>
__device__ __forceinline__ void block_sums(float (&q)[N], const F& f) {
  static_assert(kBlock / 64 == 4, "the fixed order is written for four waves");
  __shared__ float s_part[N][kBlock / 64];
#pragma unroll
  for (int k = 0; k < N; ++k) q[k] = wave_sum(q[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_part[k][wave] = q[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) f(k, ((s_part[k][0] + s_part[k][1]) + s_part[k][2]) + s_part[k][3]);
  }
}

// ---- the peel -----------------------------------------------------------------------------------------------------------------------------
// The next key among a wave's pixels that are still `open` (bit i: pixel i of the lane's quad; false: none left): the key of the lowest
// open pixel of the first lane that has one.  mm: the lane's open pixels of that key, which are closed.  A 32-bit key comes back uniform.
template <typename K>
__device__ __forceinline__ bool peel(const K (&key)[kQuad], unsigned& open, K& cur, unsigned& mm) {
  const unsigned long long any = __ballot(open != 0);
  if (!any) return false;
  K cand = 0;
#pragma unroll
  for (int i = kQuad - 1; i >= 0; --i)
    if ((open >> i) & 1u) cand = key[i];
  if constexpr (sizeof(K) == 4) cur = __builtin_amdgcn_readfirstlane(__shfl(cand, __ffsll(any) - 1, 64));
  else cur = __shfl(cand, __ffsll(any) - 1, 64);
  mm = 0;
#pragma unroll
  for (int i = 0; i < kQuad; ++i)
    if (((open >> i) & 1u) && key[i] == cur) mm |= 1u << i;
  open &= ~mm;
  return true;
}

// ---- the table workspace: u64 words, all zero but for the magic word in front -----------------------------------------------------------------
constexpr int kTableHdrWords = 8;  // [0] magic; the rest of the header is the family's

template <unsigned MAGIC>
__global__ __launch_bounds__(kBlock) void k_table_init(u64* __restrict__ w, size_t words) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (size_t)gridDim.x * kBlock) w[i] = i == 0 ? (u64)MAGIC : 0ull;
}
template <unsigned MAGIC>
inline void launch_table_init(void* ws, size_t bytes, hipStream_t s) {
  const size_t words = bytes / 8;
  const size_t g = (words + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_table_init<MAGIC>, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(kBlock), 0, s, (u64*)ws, words);
}
// the body of a pea_*_workspace_init entry
template <unsigned MAGIC>
inline int table_workspace_init(void* workspace, size_t bytes, void* stream) {
  if (!workspace) return PEA_E_NULL;
  if (misaligned(workspace, 8)) return PEA_E_ALIGN;
  if (bytes < 8 * kTableHdrWords || bytes % 8) return PEA_E_WORKSPACE;
  launch_table_init<MAGIC>(workspace, bytes, (hipStream_t)stream);
  return hip_rc();
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// workgroups of a streaming launch, one per `run` elements of each of `planes` ranges of n; false: more than 2^31 - 1 (n and planes
// may be saturated products)
inline bool stream_grid(uint64_t n, uint64_t planes, int run, unsigned* chunks, unsigned* groups) {
  const uint64_t c = n / run + (n % run ? 1 : 0);
  const uint64_t g = mul_sat(planes, c);
  if (g > 0x7fffffffULL) return false;
  *chunks = (unsigned)c; *groups = (unsigned)g;
  return true;
}
// A launch entry's list of launches: chain(kernel, grid, block, args..) launches on the stream unless an earlier launch failed; rc is
// the first failure (hip_rc) or PEA_OK.  The arguments convert to the kernel's parameter types as in a plain call.
struct LaunchChain {
  hipStream_t s;
  int rc = PEA_OK;
  explicit LaunchChain(void* stream) : s((hipStream_t)stream) {}
  template <typename... P, typename... A>
  void operator()(void (*kernel)(P...), dim3 grid, dim3 block, const A&... args) {
    if (rc) return;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<P>(args)...);
    rc = hip_rc();
  }
};
// the end of a launch sequence on a prepared block: where a launch failed, partials may be queued without what zeroes them, so the
// block is prepared again (the contract of its init entry) and the error of that launch, if any, is swallowed.  -> rc
template <typename F>
inline int or_prepare_again(int rc, F&& prepare) {
  if (rc) { prepare(); (void)hipGetLastError(); }
  return rc;
}

}  // namespace pea
