// pea_epilogue.h -- the end of every training forward, stated once: the loss term of one pair, its quad form, the wave partial and
// the workgroup's tail into the LossState.  (The finish that follows in a launch of its own is loss_row_collect, pea_loss.h.)
//
// The term.  For a pair (p, p + o) with the value v that the loss sees, target t, weight w and mask m:
//   u  = v                                  (LACT: u = act_u(v), v = act_v(a) taken by the CALLER -- it also stores u as affs)
//   r  = u * m - t * m
//   wr = exists ? w * r : 0
//   g  = gs * wr * m                        (LACT: act_g(u, v, gs * sc, wr, m): the slope of the activation folded in)
//   share of the loss = wr * r              (the quad form: acc = fmaf(wr, r, acc), j = 0 .. 3 in order)
// BCE (on the activated map only) puts bce_term's (contrib, factor) in the place of (wr * r, wr): x = u m, y = t m, both outputs
// zeroed where the pair does not exist, gs = lambda / N without the squared residual's factor 2, and the quad adds acc += contrib.
// This is a contract on BITS between the families (tests/test_gpu_alignment.py, test_gpu_loss_reduction.py, test_gpu_nonfinite.py):
//   * the order of operations is the one above, left to right; the quad's accumulation is an EXPLICIT fmaf, the scalar share a
//     product, and every includer compiles with the default contraction (the streaming kernels that switch it off do not come here).
//     r itself is left to that contraction: with a mask of 0 / 1 every form of u m - t m gives the same bits, with any other mask the
//     compiler's choice per kernel (one fma, or two products and a subtraction) shows.  profiles/README.md, "Epilogue refactor", holds
//     the check that every kernel kept the choice it had: the multiset of its floating-point instructions.  One site did not keep it
//     behind the call and states the quad itself: k_fwd_tiled_v (pea_tiled.h), which decides its border at run time.
//   * relu and clamp are SELECTS (clamp_keep_nan), never fmaxf / fminf: a NaN v stays NaN in u and the loss is NaN; u == v is then
//     false and g is ActK::gz -- 0 with the clamp (torch.clamp's backward at a NaN input), NaN without it.
//   * `exists` zeroes wr (and with it g and the share); it never multiplies a by 0: 0 * e(p) is NaN for a non-finite own pixel.
//     The caller passes a = 0 for a pair that does not exist where its staging has not already made it so.
//   * the epilogues keep v, not u, across their stores: u is two instructions away from v, and keeping both spilled in the 64-VGPR
//     forwards.  So the term takes v and clamps it itself, and a caller that stores affs clamps its own copy.
//
// Geometry is the family's business: WHICH pairs exist (the axis-aligned test of the cross, march and 16-bit kernels, the general
// (oy, ox, oz) test of k_fwd_tiled_v, rowok && x-test of the box kernel, `valid` / `exists` of the one-lane-per-pixel forms) reaches
// this header as a bool, or as four of them for the quad.  Nothing here knows which family calls it.  The labels-in branch of
// k_fwd_xdma derives t, m and w from the two labels itself and calls the term with them.  The three PEA_LAB_* macros and the two tails
// of pea_fused_labels.h state the same lines themselves: with the calls in their place the kernels' instruction order moved and the
// two-launch labels step measured above the parent's interval (profiles/README.md, "Epilogue refactor").
//
// The tail.  Lane 63 of each wave writes wave_sum63(acc) into a workgroup array s_part; after the family's barrier the lanes it picks
// (threadIdx.x < K of wave 0, lane_k, two waves with two states in the pair kernel) call part_accumulate: the row's slices summed in
// index order, one loss_accumulate.  The two layouts of s_part are two pairs of strides: [k * NSL + slice] is (NSL, 1), [wave * K + k]
// is (1, K).  The z-march reads the previous plane's partials under the next plane's barrier with part_sum and carries the sum.
#pragma once
#include "pea_loss.h"

namespace pea {

typedef float f4 __attribute__((ext_vector_type(4)));

// the four masks of a quad of x-adjacent pixels: one dword of four bytes (MT = uint8_t), or one dwordx4 (MT = float, PEA_FLAG_MASK_F32)
template <typename MT>
using mq_t = typename std::conditional<std::is_same<MT, float>::value, f4, unsigned>::type;
template <typename MT>
__device__ __forceinline__ float mq_get(const mq_t<MT>& q, int j) {
  if constexpr (std::is_same<MT, float>::value) return q[j];
  else return (float)((q >> (8 * j)) & 0xffu);
}

// ACC: `s` is a running sum and takes the share by fmaf (the quad); else `s` becomes the share.  Returns g = d loss / d a.
template <bool LACT, bool BCE, bool ACC>
__device__ __forceinline__ float loss_term_as(float v, float t, float w, float m, bool exists, float gs, const ActK& k, float& s) {
  static_assert(!BCE || LACT, "binary cross-entropy (PEA_FLAG_LOSS_BCE, bce_term) is taken on the activated map");
  const float u = LACT ? act_u(v, k) : v;
  if constexpr (BCE) {
    float l, bt = bce_term(u * m, t * m, w, l);
    bt = exists ? bt : 0.f;
    l = exists ? l : 0.f;
    s = ACC ? s + l : l;
    return act_g(u, v, gs * k.sc, bt, m, k);
  } else {
    const float r = u * m - t * m;
    const float wr = exists ? w * r : 0.f;
    s = ACC ? fmaf(wr, r, s) : wr * r;
    return LACT ? act_g(u, v, gs * k.sc, wr, m, k) : gs * wr * m;
  }
}

// the scalar term: the pair's share of the loss into `contrib`, returns g
template <bool LACT, bool BCE = false>
__device__ __forceinline__ float loss_term(float v, float t, float w, float m, bool exists, float gs, const ActK& k, float& contrib) {
  return loss_term_as<LACT, BCE, false>(v, t, w, m, exists, gs, k, contrib);
}
// on the raw cosine a
__device__ __forceinline__ float loss_term(float a, float t, float w, float m, bool exists, float gs, float& contrib) {
  return loss_term_as<false, false, false>(a, t, w, m, exists, gs, ActK{}, contrib);
}
// ... as one element of a quad whose t, w and m the caller derives itself (the labels-in cross kernel): acc = fmaf(wr, r, acc)
__device__ __forceinline__ float loss_term_acc(float a, float t, float w, float m, bool exists, float gs, float& acc) {
  return loss_term_as<false, false, true>(a, t, w, m, exists, gs, ActK{}, acc);
}

// the quad form: four x-adjacent pairs of one offset, exists[j] says which of them there are.  Returns g4, the quad's share in acc.
template <typename MT, bool LACT, bool BCE = false>
__device__ __forceinline__ f4 loss_quad(const f4& v4, const f4& t4, const f4& w4, const mq_t<MT>& m4, const bool (&exists)[4], float gs,
                                        const ActK& k, float& acc) {
  f4 g4;
  acc = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) g4[j] = loss_term_as<LACT, BCE, true>(v4[j], t4[j], w4[j], mq_get<MT>(m4, j), exists[j], gs, k, acc);
  return g4;
}
template <typename MT>
__device__ __forceinline__ f4 loss_quad(const f4& a4, const f4& t4, const f4& w4, const mq_t<MT>& m4, const bool (&exists)[4], float gs,
                                        float& acc) {
  return loss_quad<MT, false, false>(a4, t4, w4, m4, exists, gs, ActK{}, acc);
}

// sum over the 64 lanes, result valid in lane 63: 6 DPP adds (no LDS traffic)
__device__ __forceinline__ float wave_sum63(float v) {
#define PEA_DPP_ADD(ctrl, rmask) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false))
  PEA_DPP_ADD(0x111, 0xf);  // row_shr:1
  PEA_DPP_ADD(0x112, 0xf);  // row_shr:2
  PEA_DPP_ADD(0x114, 0xf);  // row_shr:4
  PEA_DPP_ADD(0x118, 0xf);  // row_shr:8   -> lane 15 of each row = row total
  PEA_DPP_ADD(0x142, 0xa);  // row_bcast:15 into rows 1,3
  PEA_DPP_ADD(0x143, 0xc);  // row_bcast:31 into rows 2,3 -> lane 63 = wave total
#undef PEA_DPP_ADD
  return v;
}

// v + the N slices of row k of s_part in index order; slice s of row k lies at s_part[k * ks + s * ss]
template <int N>
__device__ __forceinline__ float part_sum(const float* s_part, int k, int ks, int ss, float v = 0.f) {
#pragma unroll
  for (int s = 0; s < N; ++s) v += s_part[k * ks + s * ss];
  return v;
}
// the tail of one lane: offset k's partial of this workgroup into the loss state
template <int N>
__device__ __forceinline__ void part_accumulate(LossState* __restrict__ st, int tile, int k, const float* s_part, int ks, int ss, float v = 0.f) {
  loss_accumulate(st, tile, k, part_sum<N>(s_part, k, ks, ss, v));
}

}  // namespace pea
