// pea_k_fgmask.hip -- the foreground-mask term of the BBBC039V1 step (include/pea_fgmask.h): the class-balanced two-class
// cross-entropy of scripts_bbbc039v1/loss/loss.py:187-194 on the binary_seg logits as ONE streaming reduction launch and one small
// finish, its gradient as ONE streaming launch, and the validation mask of scripts_bbbc039v1/main.py:406-410.
//
// The walk is the lane run of pea_stream.h, as in pea_k_metrics.hip.  A workgroup of 256 lanes owns a RUN of kRun = 4096 consecutive pixels of one image; a lane
// takes four steps of four x-adjacent pixels (pixel (step * 256 + lane) * 4 + e of the run), so a step of a wave is 1 KiB of each f32
// logit plane and of i32 labels.  A lane's quad is one wide access (dwordx4 for f32 / i32, dwordx2 for 16-bit logits, one dword for u8
// labels) where its address is aligned to four elements and the quad is whole, four scalar accesses otherwise; the two logit planes
// are Y * X elements apart, so each plane decides for itself.  The pixel-to-lane assignment and the order of the additions do not
// depend on it: every element-aligned pointer and every Y * X give the same bits.
//
// Arithmetic (pea_fgmask.h): f32, every step rounded on its own -- contraction is switched off for this file --, accurate expf /
// log1pf, IEEE division.  A lane sums its sixteen terms in order, a wave reduces with __shfl_xor (a butterfly: a fixed order), the
// four waves meet in LDS and lane 0 adds the four partials into the integer accumulators of csrc/pea_loss.h: ONE state, index 0 S0,
// 1 S1, 2 n0, 3 n1, slot = workgroup number.  The counts of a workgroup are f32 integers <= 4096, exact, and the accumulators add them
// as integers.  The finish (one wave: 16 slots x 4 indices) reads the state, writes loss and stats and zeroes what it read.
//
// Cost: forward 12 B / pixel, backward 20 B / pixel with f32 logits and i32 labels (5 + 9 with 16-bit logits and u8 labels); at the BBBC
// training shape (8 x 256 x 256) that is 17 MB a step, so both launches are launch-bound.  Measured there (DESIGN.md section 8,
// profiles/fgmask_ab.json): forward 10 us, finish 4 us, backward 6 us in a kernel trace; nothing was tuned.
#include "../../include/pea_fgmask.h"
#include "pea_dispatch.h"
#include "pea_stream.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

constexpr int kSums = 4;                        // S0, S1, n0, n1: indices of the one loss state
static_assert(kSums <= PEA_MAX_K, "the four sums are indices of one state");
static_assert(kSums * kLossSlots == 64, "the finish is one wave");
constexpr unsigned kKnownFlags = PEA_FG_SKIP_EMPTY_CLASS;

// a quad of labels (pea_quad.h has the logits' ld_quad / st_quad): y = [label > 0] (i32: one dwordx4, u8: one dword)
__device__ __forceinline__ void ld_fg(const int32_t* __restrict__ p, int nv, bool (&y)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & 15) == 0) {
    const iquad_t v = *(const iquad_t*)p;
    y[0] = v.x > 0; y[1] = v.y > 0; y[2] = v.z > 0; y[3] = v.w > 0;
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e) y[e] = e < nv && p[e] > 0;
  }
}
__device__ __forceinline__ void ld_fg(const uint8_t* __restrict__ p, int nv, bool (&y)[kQuad]) {
  if (nv == kQuad && ((uintptr_t)p & 3) == 0) {
    const uint32_t v = *(const uint32_t*)p;
    y[0] = (v & 0xffu) != 0; y[1] = (v & 0xff00u) != 0; y[2] = (v & 0xff0000u) != 0; y[3] = (v >> 24) != 0;
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e) y[e] = e < nv && p[e] != 0;
  }
}
// z = y ? l0 - l1 : l1 - l0: the logit of the WRONG class minus the logit of the right one
__device__ __forceinline__ float wrong_minus_right(float l0, float l1, bool y) { return y ? l0 - l1 : l1 - l0; }

// ---- forward: the four sums -----------------------------------------------------------------------------------------------------
template <typename T, typename LT>
__global__ __launch_bounds__(kBlock) void k_fg_fwd(const size_t S, const unsigned chunks, const T* __restrict__ logits,
                                                   const LT* __restrict__ labels, LossState* __restrict__ st) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const T* __restrict__ p0 = logits + b * 2 * S;
  const T* __restrict__ p1 = p0 + S;
  const LT* __restrict__ lp = labels + b * S;

  float s0 = 0.f, s1 = 0.f, c0 = 0.f, c1 = 0.f;
  const size_t run0 = (size_t)at.chunk * kLaneRun;
#pragma unroll 1
  for (int j = 0; j < kSteps; ++j) {  // (lane_run written out: see profiles/README.md, Stream refactor)
    const size_t i0 = run0 + ((size_t)j * kBlock + threadIdx.x) * kQuad;
    if (i0 >= S) break;
    const int nv = S - i0 >= (size_t)kQuad ? kQuad : (int)(S - i0);
    float l0[kQuad], l1[kQuad];
    bool y[kQuad];
    ld_quad(p0 + i0, nv, l0);
    ld_quad(p1 + i0, nv, l1);
    ld_fg(lp + i0, nv, y);
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      if (e < nv) {
        const float z = wrong_minus_right(l0[e], l1[e], y[e]);
        const float t = log1pf(expf(-fabsf(z)));
        const float nll = (z > 0.f ? z : 0.f) + t;  // a select, not fmaxf: a NaN z stays NaN through t
        s0 += y[e] ? 0.f : nll;
        s1 += y[e] ? nll : 0.f;
        c0 += y[e] ? 0.f : 1.0f;
        c1 += y[e] ? 1.0f : 0.f;
      }
    }
  }

  float q[kSums] = {s0, s1, c0, c1};
  block_sums(q, [&](int k, float v) { loss_accumulate(st, (int)blockIdx.x, k, v); });
}

// The finish, one wave: lane = 16 * k + slot reads index k of the state (as k_loss_finish), writes loss and stats and puts the state
// back to zero.
__global__ __launch_bounds__(64) void k_fg_finish(LossState* __restrict__ st, float* __restrict__ loss, double* __restrict__ stats,
                                                  int skip_empty) {
  __shared__ double s_v[kSums];
  const int lane = threadIdx.x, s = lane & (kLossSlots - 1), k = lane >> 4;
  const bool good = st->magic == kLossMagic;
  const double v = loss_row_collect(st, k, s, true);
  if (s == 0) s_v[k] = v;
  __syncthreads();
  if (lane == 0) {
    const double qnan = __builtin_nan("");
    const double n0 = s_v[2], n1 = s_v[3];
    // an absent class: 0 / 0 = NaN (the reference), or 0 with PEA_FG_SKIP_EMPTY_CLASS
    const double t0 = (skip_empty && n0 == 0.0) ? 0.0 : s_v[0] / n0;
    const double t1 = (skip_empty && n1 == 0.0) ? 0.0 : s_v[1] / n1;
    const double l = 0.5 * (t0 + t1);
    stats[0] = good ? l : qnan;
    stats[1] = good ? t0 : qnan;
    stats[2] = good ? t1 : qnan;
    stats[3] = good ? n0 : qnan;
    stats[4] = good ? n1 : qnan;
    loss[0] = good ? (float)l : __builtin_nanf("");
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename LT>
__global__ __launch_bounds__(kBlock) void k_fg_bwd(const size_t S, const unsigned chunks, const int skip_empty, const T* __restrict__ logits,
                                                   const LT* __restrict__ labels, const double* __restrict__ stats,
                                                   const float* __restrict__ dloss, T* __restrict__ dlogits) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const T* __restrict__ p0 = logits + b * 2 * S;
  const T* __restrict__ p1 = p0 + S;
  const LT* __restrict__ lp = labels + b * S;
  T* __restrict__ g0 = dlogits + b * 2 * S;
  T* __restrict__ g1 = g0 + S;

  // c_y = dloss / (2 n_y), divided in f64 and rounded once (uniform over the grid).  An absent class without PEA_FG_SKIP_EMPTY_CLASS:
  // the reference's class weights are (n1, n0), so the weight of the only class present is 0 and every element is 0 / 0
  const double n0 = stats[3], n1 = stats[4];
  const double dl = dloss ? (double)dloss[0] : 1.0;
  const bool all_nan = !skip_empty && (n0 == 0.0 || n1 == 0.0);
  const float cn0 = all_nan ? __builtin_nanf("") : (float)(dl / (2.0 * n0));
  const float cn1 = all_nan ? __builtin_nanf("") : (float)(dl / (2.0 * n1));

  const size_t run0 = (size_t)at.chunk * kLaneRun;
#pragma unroll 1
  for (int j = 0; j < kSteps; ++j) {  // (lane_run written out, as in k_fg_fwd)
    const size_t i0 = run0 + ((size_t)j * kBlock + threadIdx.x) * kQuad;
    if (i0 >= S) break;
    const int nv = S - i0 >= (size_t)kQuad ? kQuad : (int)(S - i0);
    float l0[kQuad], l1[kQuad], d0[kQuad], d1[kQuad];
    bool y[kQuad];
    ld_quad(p0 + i0, nv, l0);
    ld_quad(p1 + i0, nv, l1);
    ld_fg(lp + i0, nv, y);
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      const float z = wrong_minus_right(l0[e], l1[e], y[e]);
      const float s = __fdiv_rn(1.0f, 1.0f + expf(-z));  // softmax of the wrong class
      const float q = s * (y[e] ? cn1 : cn0);
      d1[e] = y[e] ? -q : q;
      d0[e] = y[e] ? q : -q;
    }
    st_quad(g0 + i0, nv, d0);
    st_quad(g1 + i0, nv, d1);
  }
}

// ---- the validation mask ------------------------------------------------------------------------------------------------------------
struct CropParams {
  size_t S;          // Y * X
  int X, oy, ox;     // row length of the logits, origin of the crop
  unsigned OY, OX;   // the crop
  size_t n;          // B * OY * OX
};

// a lane owns four consecutive elements of the (dense) output; the logits are gathered row by row behind the crop
template <typename T>
__global__ __launch_bounds__(kBlock) void k_fg_argmax(const CropParams P, const T* __restrict__ logits, uint8_t* __restrict__ out) {
  const size_t i0 = quad_start(blockIdx.x);
  if (i0 >= P.n) return;
  const int nv = quad_nv(i0, P.n);
  CropCursor at(i0, P.OY, P.OX);  // (image, y, x) of the output
  unsigned m[kQuad];
#pragma unroll
  for (int e = 0; e < kQuad; ++e) {
    m[e] = 0;
    if (e < nv) {
      const size_t o = at.o * 2 * P.S + (size_t)(at.y + (unsigned)P.oy) * P.X + (at.x + (unsigned)P.ox);
      const float l0 = ld<T>(logits, o), l1 = ld<T>(logits, o + P.S);
      m[e] = l1 > l0 ? 1u : 0u;  // a tie or a NaN: 0
    }
    at.step(P.OY, P.OX);
  }
  uint8_t* __restrict__ op = out + i0;
  if (nv == kQuad && ((uintptr_t)op & 3) == 0) {
    *(uint32_t*)op = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e)
      if (e < nv) op[e] = (uint8_t)m[e];
  }
}

// workgroups of a loss launch (one per lane run of an image); false: more than 2^31 - 1
inline bool loss_grid(const PeaFgDesc* d, uint64_t* S, unsigned* chunks, unsigned* groups) {
  *S = (uint64_t)d->Y * (uint64_t)d->X;
  return stream_grid(*S, (uint64_t)d->B, kLaneRun, chunks, groups);
}

// f(Tag<T>{}, Tag<LT>{}): the logits' storage type and the labels' element type
template <typename F>
inline void with_fg_types(const PeaFgDesc* d, F&& f) {
  with_storage(d->logits_dtype, [&](auto t) {
    if (d->labels_type == PEA_FG_LABELS_U8) f(t, Tag<uint8_t>{});
    else f(t, Tag<int32_t>{});
  });
}

}  // namespace

extern "C" int pea_fgmask_validate(const PeaFgDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->Y < 1 || d->X < 1) return PEA_E_DESC;
  if (d->logits_dtype != PEA_F32 && d->logits_dtype != PEA_F16 && d->logits_dtype != PEA_BF16) return PEA_E_DESC;
  if (d->labels_type != PEA_FG_LABELS_I32 && d->labels_type != PEA_FG_LABELS_U8) return PEA_E_DESC;
  if (d->flags & ~kKnownFlags) return PEA_E_DESC;
  const int32_t ext[2] = {d->Y, d->X};
  for (int a = 0; a < 2; ++a)
    if (d->origin[a] < 0 || d->out_dims[a] < 0 || (int64_t)d->origin[a] + d->out_dims[a] > (int64_t)ext[a]) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" size_t pea_fgmask_workspace_bytes(void) { return sizeof(LossState); }

extern "C" int pea_fgmask_loss_fwd(const PeaFgDesc* d, const void* logits, const void* labels, float* loss, double* stats,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_fgmask_validate(d);
  if (vrc) return vrc;
  if (!logits || !labels || !loss || !stats) return PEA_E_NULL;
  const bool li32 = d->labels_type == PEA_FG_LABELS_I32;
  if (misaligned(logits, dtype_bytes(d->logits_dtype)) || (li32 && misaligned(labels, 4)) || misaligned(loss, 4) ||
      misaligned(stats, 8) || misaligned(workspace, 8))
    return PEA_E_ALIGN;
  if (!workspace || workspace_bytes < pea_fgmask_workspace_bytes()) return PEA_E_WORKSPACE;
  uint64_t S;
  unsigned chunks, groups;
  if (!loss_grid(d, &S, &chunks, &groups)) return PEA_E_UNSUPPORTED;

  LaunchChain chain(stream);
  LossState* st = (LossState*)workspace;
  with_fg_types(d, [&](auto t, auto lt) {
    using T = typename decltype(t)::type;
    using LT = typename decltype(lt)::type;
    chain(k_fg_fwd<T, LT>, groups, kBlock, S, chunks, (const T*)logits, (const LT*)labels, st);
  });
  chain(k_fg_finish, 1, 64, st, loss, stats, (d->flags & PEA_FG_SKIP_EMPTY_CLASS) ? 1 : 0);
  return or_prepare_again(chain.rc, [&] { launch_loss_state_init(st, 1, chain.s); });
}

extern "C" int pea_fgmask_loss_bwd(const PeaFgDesc* d, const void* logits, const void* labels, const double* stats, const float* dloss,
                                   void* dlogits, void* stream) {
  const int vrc = pea_fgmask_validate(d);
  if (vrc) return vrc;
  if (!logits || !labels || !stats || !dlogits) return PEA_E_NULL;
  const bool li32 = d->labels_type == PEA_FG_LABELS_I32;
  const size_t eb = dtype_bytes(d->logits_dtype);
  if (misaligned(logits, eb) || misaligned(dlogits, eb) || (li32 && misaligned(labels, 4)) || misaligned(dloss, 4) || misaligned(stats, 8))
    return PEA_E_ALIGN;
  uint64_t S;
  unsigned chunks, groups;
  if (!loss_grid(d, &S, &chunks, &groups)) return PEA_E_UNSUPPORTED;

  LaunchChain chain(stream);
  const int skip = (d->flags & PEA_FG_SKIP_EMPTY_CLASS) ? 1 : 0;
  with_fg_types(d, [&](auto t, auto lt) {
    using T = typename decltype(t)::type;
    using LT = typename decltype(lt)::type;
    chain(k_fg_bwd<T, LT>, groups, kBlock, S, chunks, skip, (const T*)logits, (const LT*)labels, stats, dloss, (T*)dlogits);
  });
  return chain.rc;
}

extern "C" int pea_fgmask_argmax(const PeaFgDesc* d, const void* logits, uint8_t* mask_out, void* stream) {
  const int vrc = pea_fgmask_validate(d);
  if (vrc) return vrc;
  if (d->out_dims[0] < 1 || d->out_dims[1] < 1) return PEA_E_DESC;
  if (!logits || !mask_out) return PEA_E_NULL;
  if (misaligned(logits, dtype_bytes(d->logits_dtype))) return PEA_E_ALIGN;
  CropParams P;
  P.S = (size_t)d->Y * (size_t)d->X;
  P.X = d->X; P.oy = d->origin[0]; P.ox = d->origin[1];
  P.OY = (unsigned)d->out_dims[0]; P.OX = (unsigned)d->out_dims[1];
  const uint64_t n = mul_sat(mul_sat((uint64_t)d->B, (uint64_t)P.OY), (uint64_t)P.OX);
  unsigned chunks, groups;  // one quad run per workgroup over all images' output
  if (!stream_grid(n, 1, kQuadRun, &chunks, &groups)) return PEA_E_UNSUPPORTED;
  P.n = (size_t)n;
  LaunchChain chain(stream);
  with_storage(d->logits_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    chain(k_fg_argmax<T>, groups, kBlock, P, (const T*)logits, mask_out);
  });
  return chain.rc;
}
