// pea_k_xdma_h.hip -- launchers of the LDS-DMA cross kernels for 16-bit storage, f16 and bf16 (pea_xdma_h16.h).  One translation unit of libpea_hip.so
// (pea_host.h); split from pea_k_xdma.hip for compile time (the f32 projection-first backward: pea_k_xdma_pf.hip).
#include "pea_k_xdma_plan.h"
#include "pea_xdma_h16.h"
#include "pea_xdma_pf.h"

namespace pea {

namespace {

// bf16 storage runs one form per kernel, the one f16 runs by default: the 16-bit working buffer (PEA_H16_HW >= 1) wherever f16 has
// it -- forward, projection-first backward, the cross loss -- and the f32 working buffer in the plain backward.  PEA_H16_HW and the
// producer / consumer backward (PEA_H16_HW=2, pea_xdma_hq.h) select among the f16 kernels only.  (Projection-first backward in bf16,
// B=8 x 64 x 544^2, forward + backward: 0.431 ms with the bf16 working buffer -- shift / and unpack in front of the FMAs -- against
// 0.470 ms with the f32 one; the bf16 step is 1.04x the f16 step without the producer / consumer kernel: profiles/bf16_ab.json.)
template <typename T>
constexpr bool kBf16 = std::is_same<T, __bf16>::value;

// ---- 16-bit storage (pea_xdma_h16.h): 2D self loss / inference, X % 8 == 0 ------------------------------------------------
template <typename T, int D_T, bool TRAIN>
bool fwd_self_h(const KParams& P, const FwdArgs& A, hipStream_t s) {
  const T* e = (const T*)A.e;
  if (P.X % 8 || P.Z != 1 || misaligned(e, 16) || misaligned(A.t, 16) || misaligned(A.w, 16) || misaligned(A.affs, 16) ||
      misaligned(A.gout, 16) || misaligned(A.m, 4) || misaligned(A.inv_out, 4))
    return false;
  if (TRAIN && ((P.tbs | P.wbs | P.mbs) & 3)) return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0 || P.K > kXP) return false;
  const size_t lds = (size_t)5 * kXdmaPSUF * 256;  // two f32 working planes + six half-size ring planes
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  // an f32 mask (training): the 16-bit working buffer's kernel with dwordx4 mask quads, one slot count (kXP); a plane that is not
  // 16-byte aligned, or PEA_H16_HW=0, takes the next family
  const bool mf = TRAIN && A.mf32;
  if (mf && (misaligned(A.m, 16) || !(kBf16<T> || env().h16_hw))) return false;
  // the loss on the activated map (PEA_FLAG_LOSS_ACT): likewise the 16-bit working buffer's kernel with one slot count, either mask type
  const bool la = TRAIN && A.lact;
  if (la && !(kBf16<T> || env().h16_hw)) return false;
  const bool crop = P.border != PEA_BORDER_CIRCULAR;
  if (kBf16<T> || env().h16_hw) {  // half-precision working buffer, v_dot2 gather: 48 VGPRs and 30 KB -- four workgroups per CU (five: 173 against 168 us)
    const size_t ldsh = (size_t)4 * kXdmaPSUF * 256;
    return with_bool(crop, [&](auto crop) {
      return with_mask_form(mf, la, [&](auto mt, auto lact) {
        using MT = typename decltype(mt)::type;
        if constexpr (std::is_same<MT, uint8_t>::value && !lact.value) {
          // (D = 64 with at most eight offsets -- BASELINE configs[4] -- walks eight slots instead of ten)
          return with_bool(D_T == 64 && X.C.nf <= 8, [&](auto few) {
            constexpr int NXP = few.value && D_T == 64 ? 8 : kXP;
            return launch<k_fwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, TRAIN, 8, true, NXP, false, T>>(
                grid, blk, ldsh, s, P, X.C, e, A.t, A.w, A.m, A.affs, A.gout, A.st, A.inv_out, (const T*)nullptr, (float*)nullptr);
          });
        } else if constexpr (TRAIN) {
          // (LOSS_ACT with an f32 mask and a cropped border takes 65 VGPRs: three workgroups per CU instead of a spill at four)
          constexpr int WPE = (lact.value && crop.value && std::is_same<MT, float>::value) ? 6 : 8;
          return launch<k_fwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, true, WPE, true, kXP, false, T, MT, lact.value>>(
              grid, blk, ldsh, s, P, X.C, e, A.t, A.w, (const MT*)(const void*)A.m, A.affs, A.gout, A.st, A.inv_out, (const T*)nullptr,
              (float*)nullptr);
        } else {
          return false;
        }
      });
    });
  }
  if constexpr (!kBf16<T>)
    return with_bool(crop, [&](auto crop) {
      return launch<k_fwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, TRAIN, 6>>(
          grid, blk, lds, s, P, X.C, e, A.t, A.w, A.m, A.affs, A.gout, A.st, A.inv_out, (const __half*)nullptr, (float*)nullptr);
    });
  return true;
}

template <typename T, int D_T>
bool bwd_self_h(const KParams& P, const T* x, const float* inv, const float* g, const float* affs, const float* dl, T* dx,
                hipStream_t s) {
  if (P.X % 8 || P.Z != 1 || misaligned(x, 16) || misaligned(inv, 16) || misaligned(g, 4) || misaligned(dx, 2) || misaligned(affs, 4))
    return false;
  XPlan X;
  const dim3 blk(kXdmaTH * kXdmaTW);
  const bool crop = P.border != PEA_BORDER_CIRCULAR;
  if constexpr (D_T > 16) {  // the projection first (pea_xdma_pf.h); at D = 16 it loses and is not instantiated
   if (affs && env().bwd_pf && !(P.flags & kActMask)) {
    const bool small = plan(P, kXdmaPSUHS, 0, &X);
    if ((small || plan(P, kXdmaPSUH, 0, &X)) && X.C.npz == 0 && X.C.npx <= kXP && X.C.npy <= kXP) {
      const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd));
      // (D = 64 with at most eight pairs per axis -- BASELINE configs[4]: offsets[:8] = four shifts per axis, two roles each -- walks
      //  eight pairs per axis instead of ten: an unused pair costs its LDS read and its two FMAs all the same)
      constexpr int XPS = D_T == 64 ? 8 : kXP;
      const bool few = D_T == 64 && X.C.npx <= 8 && X.C.npy <= 8;
      // (87 VGPRs: the conversion's temporaries keep it above the 80 a third workgroup would need; small planes all the same --
      //  less LDS per workgroup never hurts the other kernels sharing the CU in a multi-stream section)
      auto go = [&](auto psu) {
        const size_t lds = (size_t)5 * psu.value * 256;
        return with_bool(crop, [&](auto crop) {
          if (kBf16<T> || env().h16_hw)
            return with_bool(few, [&](auto few) {
              return launch<k_bwd_xdma_h<D_T, kXdmaTH, kXdmaTW, psu.value, crop.value, (few.value ? XPS : kXP), true, 4, true, false, T>>(
                  grid, blk, lds, s, P, X.C, x, inv, g, affs, dl, dx, (const T*)nullptr, (const float*)nullptr);
            });
          if constexpr (!kBf16<T>)
            return launch<k_bwd_xdma_h<D_T, kXdmaTH, kXdmaTW, psu.value, crop.value, kXP, true, 4>>(
                grid, blk, lds, s, P, X.C, x, inv, g, affs, dl, dx, (const T*)nullptr, (const float*)nullptr);
          else return true;
        });
      };
      return small ? go(Int<kXdmaPSUHS>{}) : go(Int<kXdmaPSUH>{});
    }
   }
  }
  if (!plan(P, kXdmaPSUH, 0, &X) || X.C.npz > 0) return false;
  constexpr int XP = D_T > 32 ? 8 : kXP;
  if (X.C.npx > XP || X.C.npy > XP) return false;
  const size_t lds = (size_t)5 * kXdmaPSUH * 256;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd));
  return with_bool(crop, [&](auto crop) {
    return launch<k_bwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUH, crop.value, XP, false, 4, false, false, T>>(
        grid, blk, lds, s, P, X.C, x, inv, g, (const float*)nullptr, dl, dx, (const T*)nullptr, (const float*)nullptr);
  });
}

// ---- 16-bit storage, the cross loss with a detached second operand (k_fwd_xdma_h<.., OTHER>, k_bwd_xdma_h<.., PF, HW, OTHER>): 2D, X % 8 == 0
template <typename T, int D_T>
bool fwd_other_h(const KParams& P, const FwdArgs& A, hipStream_t s) {
  const T *e = (const T*)A.e, *eo = (const T*)A.eo;
  if (P.X % 8 || P.Z != 1 || misaligned(e, 16) || misaligned(eo, 16) || misaligned(A.t, 16) || misaligned(A.w, 16) || misaligned(A.affs, 16) ||
      misaligned(A.gout, 16) || misaligned(A.m, 4) || misaligned(A.inv_out, 4) || ((P.tbs | P.wbs | P.mbs) & 3))
    return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0 || P.K > kXP) return false;
  const size_t lds = (size_t)4 * kXdmaPSUF * 256 + 6 * 1024;  // working plane + ring + the own tiles
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  float* inv_other = A.inv_out + (size_t)P.B * P.S;
  if (A.mf32 && misaligned(A.m, 16)) return false;  // an f32 mask: dwordx4 mask quads
  return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
    return with_mask_form(A.mf32, A.lact, [&](auto mt, auto lact) {
      using MT = typename decltype(mt)::type;
      // an f32 mask; PEA_FLAG_LOSS_ACT: the loss on the activated map -- one slot count (kXP); else D = 64 with at most eight offsets walks eight
      constexpr bool kPlain = std::is_same<MT, uint8_t>::value && !lact.value;
      return with_bool(kPlain && D_T == 64 && X.C.nf <= 8, [&](auto few) {
        constexpr int NXP = kPlain && few.value && D_T == 64 ? 8 : kXP;
        return launch<k_fwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, true, 6, true, NXP, true, T, MT, lact.value>>(
            grid, blk, lds, s, P, X.C, eo, A.t, A.w, (const MT*)(const void*)A.m, A.affs, A.gout, A.st, A.inv_out, e, inv_other);
      });
    });
  });
}

template <typename T, int D_T>
bool bwd_other_h(const KParams& P, const T* e, const T* eo, const float* inv2, const float* g, const float* affs, const float* dl,
                 T* de, hipStream_t s) {
  if (P.X % 8 || P.Z != 1 || misaligned(e, 16) || misaligned(eo, 16) || misaligned(inv2, 16) || ((size_t)P.B * P.S) % 4 ||
      misaligned(g, 4) || misaligned(affs, 4) || misaligned(de, 2))
    return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 2, &X) || X.C.npz > 0 || X.C.npx > kXP || X.C.npy > kXP) return false;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  const size_t lds = (size_t)5 * kXdmaPSUF * 256 + 6 * 1024;
  const float* inv_other = inv2 + (size_t)P.B * P.S;
  constexpr int XPS = D_T == 64 ? 8 : kXP;
  const bool few = D_T == 64 && X.C.npx <= 8 && X.C.npy <= 8;
  return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
    return with_bool(few, [&](auto few) {
      return launch<k_bwd_xdma_h<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, (few.value ? XPS : kXP), true, 4, true, true, T>>(
          grid, blk, lds, s, P, X.C, eo, inv_other, g, affs, dl, de, e, inv2);
    });
  });
}

}  // namespace

bool xdma_h_fwd_other(const KParams& P, const FwdArgs& A, hipStream_t s) {
  if (A.dtype != PEA_BF16 && !env().h16_hw) return false;
  if (A.bce) return false;  // no PEA_FLAG_LOSS_BCE form in the 16-bit cross forwards: the direct kernels take it
  return with_bool(A.dtype == PEA_BF16, [&](auto bf) {
    using T = std::conditional_t<bf.value, __bf16, __half>;
    return with_width<16, 32, 64>(P.D, [&](auto d) { return fwd_other_h<T, d.value>(P, A, s); });
  });
}

bool xdma_h_bwd_other(const KParams& P, int dtype, const void* e, const void* e_other, const float* inv2, const float* g, const float* affs,
                      const float* dl, void* de, hipStream_t s) {
  if (!env().bwd_pf || !affs || (P.flags & kActMask)) return false;
  if (dtype != PEA_BF16 && !env().h16_hw) return false;
  return with_bool(dtype == PEA_BF16, [&](auto bf) {
    using T = std::conditional_t<bf.value, __bf16, __half>;
    return with_width<16, 32, 64>(
        P.D, [&](auto d) { return bwd_other_h<T, d.value>(P, (const T*)e, (const T*)e_other, inv2, g, affs, dl, (T*)de, s); });
  });
}

// entry points used by pea_k_xdma.hip's dispatchers
bool xdma_h_fwd_self(const KParams& P, const FwdArgs& A, hipStream_t s) {
  if (A.train && A.bce) return false;  // no PEA_FLAG_LOSS_BCE form in the 16-bit cross forwards: the direct kernels take it
  return with_bool(A.dtype == PEA_BF16, [&](auto bf) {
    using T = std::conditional_t<bf.value, __bf16, __half>;
    return with_width<16, 32, 64>(P.D, [&](auto d) {
      return with_bool(A.train, [&](auto train) { return fwd_self_h<T, d.value, train.value>(P, A, s); });
    });
  });
}

bool xdma_bwd_self_h(const KParams& P, int dtype, const void* x, const float* inv, const float* g, const float* affs, const float* dl,
                     void* dx, hipStream_t s) {
  if (!inv || !env().bwd_xdma || env().force_direct) return false;
  if (dtype != PEA_BF16 && env().h16_hw == 2 && env().bwd_pf && xdma_hq_bwd_self(P, x, inv, g, affs, dl, dx, s)) return true;  // pea_k_xdma_hq.hip
  return with_bool(dtype == PEA_BF16, [&](auto bf) {
    using T = std::conditional_t<bf.value, __bf16, __half>;
    return with_width<16, 32, 64>(P.D, [&](auto d) { return bwd_self_h<T, d.value>(P, (const T*)x, inv, g, affs, dl, (T*)dx, s); });
  });
}

}  // namespace pea
