// pea_k_xdma.hip -- launchers of the LDS-DMA cross kernels (pea_xdma.h): plan, pick the instantiation, launch.
// One translation unit of libpea_hip.so (pea_host.h).
#include "pea_k_xdma_plan.h"
#include "pea_xdma_dual.h"

namespace pea {

namespace {

template <int D_T, bool TRAIN>
bool fwd_self(const KParams& P, const FwdArgs& A, hipStream_t s) {
  const float *e = (const float*)A.e, *t = A.t, *w = A.w;
  if (misaligned(e, 16) || misaligned(t, 16) || misaligned(w, 16) || misaligned(A.affs, 16) || misaligned(A.gout, 16) ||
      misaligned(A.m, 4) || misaligned(A.inv_out, 4))
    return false;
  if (TRAIN && ((P.tbs | P.wbs | P.mbs) & 3)) return false;
  XPlan X;
  bool z3 = false, wg3 = false;
  // (binary cross-entropy with an f32 mask does not fit the 80 VGPRs of three workgroups per CU -- 5 to 8 registers spilled -- and is
  //  not instantiated there: two workgroups per CU, 118 / 120 VGPRs)
  const bool bce_mf = TRAIN && A.lact && A.bce && A.mf32;
  if (env().fwd_wg3 && !bce_mf && plan(P, kXdmaPSUF, 1, &X) && X.C.nfz == 0) {
    wg3 = true;
  } else if (!plan(P, kXdmaPSU, 1, &X) || X.C.nfz > 0) {
    if (D_T != 16 || !plan(P, kXdmaPSU3F, 1, &X) || X.C.nfz == 0) return false;
    z3 = true;
  }
  if (!z3 && P.K > kXP) return false;
  if (z3 && P.K > kXP + 2) return false;
  // an f32 mask (2D training only): the quads' masks are dwordx4 loads -- a plane that is not 16-byte aligned takes the next family
  const bool mf = TRAIN && A.mf32;
  if (mf && (z3 || misaligned(A.m, 16))) return false;
  // the loss on the activated map (PEA_FLAG_LOSS_ACT): training only; 2D with either mask type; 3D (z3) its binary cross-entropy form with
  // a u8 mask or none.
  // (the squared-residual z3 form is not instantiated: at 2 x 16 x 18 x 160 x 160, norm5, it ran 64.8 us against the 79.0 us of k_fwd_tiled
  //  that takes the call instead, but the eager step only went from 175.7 to 172.9 us with spreads of 4.9 + 9.0 us -- not the gain
  //  beyond the spreads a new form is held to; the BCE form replaces k_fwd_direct, 113.7 against 102.7 us per launch but 201.2
  //  against 210.0 us per step, spreads 0.9 + 0.8 -- the direct kernel also needs a k_inv_norm launch of 12.7 us: profiles/act3d_ab.json,
  //  EXPERIMENTS.md)
  const bool la = TRAIN && A.lact;
  if (la && z3 && !A.bce) return false;
  const XParams& C = X.C;
  const dim3 grid((unsigned)(C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  // the f32-mask forms are built for 2D training only (TRAIN, ZF = 0), the LOSS_ACT forms for 2D training and, BCE with the u8 mask,
  // for z3: every other call with them was declined above
  auto go = [&](auto psu, auto zf, auto wpe) {
    return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
      return with_loss_form(mf, la, la && A.bce, [&](auto mt, auto lact, auto bce) {
        using MT = typename decltype(mt)::type;
        constexpr bool kSpills = bce.value && wpe.value == 6 && std::is_same<MT, float>::value;  // (bce_mf above: never asked for)
        if constexpr (((std::is_same<MT, uint8_t>::value && (!lact.value || (TRAIN && bce.value))) || (TRAIN && zf.value == 0)) && !kSpills)
          return launch<k_fwd_xdma<D_T, kXdmaTH, kXdmaTW, psu.value, crop.value, TRAIN, zf.value, false, wpe.value, false, MT, lact.value, bce.value>>(
              grid, blk, X.lds, s, P, C, e, t, w, (const MT*)(const void*)A.m, A.affs, A.gout, A.st, A.inv_out, (const float*)nullptr,
              (float*)nullptr, LabArgs{});
        else return false;
      });
    });
  };
  if constexpr (D_T == 16) {
    if (z3) return go(Int<kXdmaPSU3F>{}, Int<kXZ / 2>{}, Int<4>{});
  }
  if (wg3) return go(Int<kXdmaPSUF>{}, Int<0>{}, Int<6>{});
  return go(Int<kXdmaPSU>{}, Int<0>{}, Int<4>{});
}

template <int D_T>
bool bwd_self(const KParams& P, const float* x, const float* inv, const float* g, const float* dl, float* dx, hipStream_t s) {
  if (misaligned(x, 16) || misaligned(inv, 16) || misaligned(g, 4) || misaligned(dx, 4)) return false;
  XPlan X;
  bool z3 = false;
  if (!plan(P, kXdmaPSU, 0, &X)) {
    if (D_T != 16 || !plan(P, kXdmaPSU3, 0, &X) || X.C.npz == 0) return false;
    z3 = true;
  } else if (X.C.npz > 0) {
    if (D_T != 16 || !plan(P, kXdmaPSU3, 0, &X)) return false;
    z3 = true;
  }
  const XParams& C = X.C;
  constexpr int XP = D_T > 32 ? 8 : kXP;  // pairs per axis the instantiation keeps in registers
  if (C.npx > (z3 ? 8 : XP) || C.npy > (z3 ? 8 : XP)) return false;
  const dim3 grid((unsigned)(C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  auto go = [&](auto xp, auto psu, auto zp) {
    return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
      return launch<k_bwd_xdma<D_T, kXdmaTH, kXdmaTW, psu.value, crop.value, xp.value, kAuxNT, zp.value>>(grid, blk, X.lds, s, P, C, x, inv, g,
                                                                                                       dl, dx, OtherArgs{}, DualArgs{});
    });
  };
  if constexpr (D_T == 16) {
    if (z3) return go(Int<8>{}, Int<kXdmaPSU3>{}, Int<kXZ>{});
  }
  return go(Int<XP>{}, Int<kXdmaPSU>{}, Int<0>{});
}

}  // namespace

// the LDS-DMA forward of the self loss (f32 storage, D in {16, 32, 64}, axis-aligned stencil, K <= kXP; 3D norm1 / norm5 at D = 16).
// (Inference keeps k_fwd_tiled: 60 us against 68 us at B=8 x 544^2 -- without the epilogue streams the one-sided box of the
//  tiled kernel moves fewer bytes than six ring planes do.)
bool xdma_fwd_self(const KParams& P, const FwdArgs& A, hipStream_t s) {
  if (!env().fwd_xdma || env().force_direct || A.eo != A.e) return false;
  if (A.dtype == PEA_F16 || A.dtype == PEA_BF16) {  // 16-bit storage: pea_xdma_h16.h
    return xdma_h_fwd_self(P, A, s);  // pea_k_xdma_h.hip
  }
  return with_width<16, 32, 64>(P.D, [&](auto d) {
    return with_bool(A.train, [&](auto train) { return fwd_self<d.value, train.value>(P, A, s); });
  });
}

// the full-resolution pair of the 2D training loops as one forward launch (pea_xdma_dual.h): 2D, D = 16, f32, axis-aligned stencil
bool xdma_fwd_dual_supported(const KParams& P, int dtype) {
  if (!env().fwd_dual || !env().fwd_xdma || env().force_direct || dtype != PEA_F32 || P.D != 16 || P.Z != 1 || P.K > kXP) return false;
  XPlan X;
  return plan(P, kXdmaPSUF, 1, &X) && X.C.nfz == 0;
}

bool xdma_fwd_dual(const KParams& P, const KParams& P2, const FwdArgs& A, const FwdArgs& A2, hipStream_t s) {
  if (!xdma_fwd_dual_supported(P, A.dtype) || !A.gout || !A2.gout || !A.inv_out || !A2.inv_out) return false;
  const float *e = (const float*)A.e, *e2 = (const float*)A2.eo;
  if (misaligned(e, 16) || misaligned(e2, 16) || misaligned(A.t, 16) || misaligned(A.w, 16) || misaligned(A.affs, 16) ||
      misaligned(A.gout, 16) || misaligned(A2.gout, 16) || misaligned(A.m, 4) || misaligned(A.inv_out, 4) || misaligned(A2.inv_out, 4))
    return false;
  if ((P.tbs | P.wbs | P.mbs) & 3) return false;
  if (A.mf32 && misaligned(A.m, 16)) return false;  // (the f32 mask's quads are dwordx4 loads)
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0) return false;
  DualFwdArgs DA = {};
  DA.e2 = e2; DA.gout2 = A2.gout; DA.inv_other_out = A2.inv_out; DA.st2 = A2.st;
  for (int i = 0; i < kXK; ++i) DA.gs2[i] = i < P2.K ? P2.gscale[i] : 0.f;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  // (NB = 4: the ring of two four-plane buffers handed over in halves; the whole-buffer hand-off -- NB = 2, +2.6 % -- and the ring of
  //  three at one workgroup per CU -- NB = 3, +21 % -- were switches until round 6 and are no longer compiled: EXPERIMENTS.md)
  constexpr int NB = 4;
  const size_t lds = (size_t)2 * 4 * kXdmaPSUF * 256;
  return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
    return with_bool(A.mf32, [&](auto mf) {
      using MT = std::conditional_t<mf.value, float, uint8_t>;
      return launch<k_fwd_xdma_dual<kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, NB, MT>>(grid, blk, lds, s, P, X.C, e, A.t, A.w,
                                                                                      (const MT*)(const void*)A.m, A.affs, A.gout, A.st,
                                                                                      A.inv_out, DA);
    });
  });
}

// the cross loss with a second operand: D = 16, f32, axis-aligned stencil; 2D images (either border) and 3D volumes whose stencil
// steps along z (ema_embedding_loss_norm5 / norm1, scripts_ac3ac4/loss/loss_embedding_mse.py:30-51, 237-289: CROP_ZERO; the z
// neighbours are the second operand's, gathered per chunk like the self loss' tile-per-plane kernels do).  e_other staged, own pixel
// from e, both 1 / norm planes written (inv_out[0 .. B*S) own, inv_out[B*S .. 2*B*S) second operand)
// D = 32 / 64 (2D): the own pixel comes from own TILES staged beside each chunk (k_fwd_xdma OWNL); one-sided cross in 7.5 KB planes
template <int D_T>
static bool fwd_other_wide(const KParams& P, const FwdArgs& A, hipStream_t s) {
  const float *e = (const float*)A.e, *e_other = (const float*)A.eo;
  if (misaligned(e, 16)) return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0 || P.K > kXP || P.Z != 1) return false;
  const size_t lds = X.lds + (size_t)6 * 2048;  // + the own tiles: three buffers x two channels x 2 KB
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
    // lact: the loss on the activated map (PEA_FLAG_LOSS_ACT); bce: its binary cross-entropy form (PEA_FLAG_LOSS_BCE)
    return with_loss_form(A.mf32, A.lact, A.bce, [&](auto mt, auto lact, auto bce) {
      using MT = typename decltype(mt)::type;
      return launch<k_fwd_xdma<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, true, 0, true, 4, false, MT, lact.value, bce.value>>(
          grid, blk, lds, s, P, X.C, e_other, A.t, A.w, (const MT*)(const void*)A.m, A.affs, A.gout, A.st, A.inv_out, e,
          A.inv_out + (size_t)P.B * P.S, LabArgs{});
    });
  });
}

bool xdma_fwd_other(const KParams& P, const FwdArgs& A, hipStream_t s) {
  if (!env().fwd_xdma || env().force_direct || !A.train || !A.inv_out) return false;
  if (A.dtype == PEA_F16 || A.dtype == PEA_BF16) return xdma_h_fwd_other(P, A, s);  // pea_k_xdma_h.hip
  if (A.dtype != PEA_F32) return false;
  if (P.D != 16 && P.D != 32 && P.D != 64) return false;
  const float *e = (const float*)A.e, *e_other = (const float*)A.eo;
  if (misaligned(e, 4) || misaligned(e_other, 16) || misaligned(A.t, 16) || misaligned(A.w, 16) || misaligned(A.affs, 16) ||
      misaligned(A.gout, 16) || misaligned(A.m, 4) || misaligned(A.inv_out, 4))
    return false;
  if ((P.tbs | P.wbs | P.mbs) & 3) return false;
  if (A.mf32 && misaligned(A.m, 16)) return false;  // (the f32 mask's quads are dwordx4 loads)
  if (P.D != 16) return with_width<32, 64>(P.D, [&](auto d) { return fwd_other_wide<d.value>(P, A, s); });
  XPlan X;
  // (three workgroups per CU do not fit here: the own pixel's 16 registers on top of the accumulators spill at 80 VGPRs)
  bool z3 = false;
  if (!plan(P, kXdmaPSU, 1, &X) || X.C.nfz > 0) {
    if (!plan(P, kXdmaPSU3F, 1, &X) || X.C.nfz == 0) return false;
    z3 = true;
  }
  if (P.K > (z3 ? kXP + 2 : kXP)) return false;
  // the f32-mask forms are 2D.  So are the PEA_FLAG_LOSS_ACT forms of the second operand: the z3 squared-residual one was built and
  // measured (ema_embedding_loss_norm2 at 2 x 16 x 18 x 160 x 160: 52.6 us per launch, 162.5 us per eager step against 152.5 us with
  // PEA_FWD_XDMA=0, spreads 9.9 + 6.6 us -- no gain, profiles/act3d_ab.json, EXPERIMENTS.md) and is not instantiated; its BCE sibling
  // was never measured
  if (z3 && (A.mf32 || A.lact)) return false;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  // the f32-mask and the loss on the activated map (PEA_FLAG_LOSS_ACT) are 2D forms (ZF = 0): z3 with them was declined above
  auto go = [&](auto psu, auto zf) {
    return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
      return with_loss_form(A.mf32, A.lact, A.bce, [&](auto mt, auto lact, auto bce) {
        using MT = typename decltype(mt)::type;
        if constexpr ((std::is_same<MT, uint8_t>::value && !lact.value) || zf.value == 0)
          return launch<k_fwd_xdma<16, kXdmaTH, kXdmaTW, psu.value, crop.value, true, zf.value, true, 4, false, MT, lact.value, bce.value>>(
              grid, blk, X.lds, s, P, X.C, e_other, A.t, A.w, (const MT*)(const void*)A.m, A.affs, A.gout, A.st, A.inv_out, e,
              A.inv_out + (size_t)P.B * P.S, LabArgs{});
        else return false;
      });
    });
  };
  return z3 ? go(Int<kXdmaPSU3F>{}, Int<kXZ / 2>{}) : go(Int<kXdmaPSU>{}, Int<0>{});
}

// the labels-in forward (k_fwd_xdma<.., LAB>): self loss, 2D, f32, axis-aligned stencil, K <= kXP; g_out and inv_out are required
// (the backward that follows is xdma_bwd_self).  true = launched.
template <int D_T>
static bool fwd_labels(const KParams& P, const FwdArgs& A, const LabArgs& LA, hipStream_t s) {
  const float* e = (const float*)A.e;
  if (misaligned(e, 16) || misaligned(A.affs, 16) || misaligned(A.gout, 16) || misaligned(A.inv_out, 4) || misaligned(LA.labels, 16))
    return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0 || P.K > kXP || P.Z != 1) return false;
  const size_t lds = X.lds + (size_t)kXdmaPSUF * 256;  // + the label plane
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
    return launch<k_fwd_xdma<D_T, kXdmaTH, kXdmaTW, kXdmaPSUF, crop.value, true, 0, false, 6, true>>(
        grid, blk, lds, s, P, X.C, e, (const float*)nullptr, (const float*)nullptr, (const uint8_t*)nullptr, A.affs, A.gout, A.st, A.inv_out,
        (const float*)nullptr, (float*)nullptr, LA);
  });
}

// would xdma_fwd_labels + xdma_bwd_self take this descriptor (16-byte aligned tensors assumed)?
bool xdma_labels_supported(const KParams& P, int dtype) {
  if (!env().fwd_xdma || !env().bwd_xdma || env().force_direct || dtype != PEA_F32 || (P.D != 16 && P.D != 32) || P.Z != 1) return false;
  XPlan X;
  if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0 || P.K > kXP) return false;
  return plan(P, kXdmaPSU, 0, &X) && X.C.npz == 0 && X.C.npx <= kXP && X.C.npy <= kXP;
}

bool xdma_fwd_labels(const KParams& P, const FwdArgs& A, const int32_t* labels, const float* wtab, unsigned lflags, hipStream_t s) {
  if (!env().fwd_xdma || !env().bwd_xdma || env().force_direct || A.dtype != PEA_F32 || !A.gout || !A.inv_out) return false;
  const LabArgs LA = {labels, wtab, lflags};
  return with_width<16, 32>(P.D, [&](auto d) { return fwd_labels<d.value>(P, A, LA, s); });
}

// the cross backward (self loss, f32 storage, axis-aligned stencil): needs the 1 / norm plane; with the raw affinity map too
// (affs: what the forward wrote with no activation flag) the projection-first kernel runs
bool xdma_bwd_self(const KParams& P, const float* x, const float* inv, const float* g, const float* affs, const float* dl, float* dx,
                   hipStream_t s) {
  if (!inv || !env().bwd_xdma || env().force_direct) return false;
  // (D = 16 keeps k_bwd_xdma: with G in 16 registers and the own pixel kept there is no second read to save, and the stores
  //  inside the chunk loop cost more than they give: 137 against 94-107 us at the bench shape)
  if (affs && env().bwd_pf && !(P.flags & kActMask) && P.D > 16) {
    bool done = false;
    done = xdma_pf_bwd_self(P, x, inv, g, affs, dl, dx, s);  // pea_k_xdma_pf.hip
    if (done) return true;
  }
  return with_width<16, 32, 64>(P.D, [&](auto d) { return bwd_self<d.value>(P, x, inv, g, dl, dx, s); });
}

// backward, role A only (the second operand is detached): de (+)= dloss * d loss / d e.  2D (either border) and 3D volumes with z steps
bool xdma_bwd_other(const KParams& P, const float* e, const float* e_other, const float* inv2, const float* g, const float* affs,
                    const float* dl, float* de, bool accumulate, hipStream_t s) {
  if (!inv2 || !env().bwd_xdma || env().force_direct) return false;
  if (P.D == 32 || P.D == 64) {  // projection first: needs the forward's raw map; no accumulate form
    if (!affs || accumulate || (P.flags & kActMask) || !env().bwd_pf || P.Z != 1) return false;
    return xdma_pf_bwd_other(P, e, e_other, inv2, g, affs, dl, de, s);
  }
  if (P.D != 16) return false;
  if (misaligned(e_other, 16) || misaligned(inv2, 16) || ((size_t)P.B * P.S) % 4) return false;
  XPlan X;
  bool z3 = false;
  if (!plan(P, kXdmaPSU, 2, &X) || X.C.npz > 0) {
    if (!plan(P, kXdmaPSU3, 2, &X) || X.C.npz == 0) return false;
    z3 = true;
  }
  if (X.C.npx > (z3 ? 8 : kXP) || X.C.npy > (z3 ? 8 : kXP)) return false;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  OtherArgs O;
  O.own = e; O.own_inv = inv2; O.accumulate = accumulate ? 1 : 0;
  auto go = [&](auto xp, auto psu, auto zp) {
    return with_bool(P.border != PEA_BORDER_CIRCULAR, [&](auto crop) {
      return launch<k_bwd_xdma<16, kXdmaTH, kXdmaTW, psu.value, crop.value, xp.value, kAuxNT, zp.value, true>>(
          grid, blk, X.lds, s, P, X.C, e_other, inv2 + (size_t)P.B * P.S, g, dl, de, O, DualArgs{});
    });
  };
  return z3 ? go(Int<8>{}, Int<kXdmaPSU3>{}, Int<kXZ / 2>{}) : go(Int<kXP>{}, Int<kXdmaPSU>{}, Int<0>{});
}

// the pair's backward in one launch (k_bwd_xdma<.., DUAL>): 2D, D = 16, f32, circular border
bool xdma_bwd_dual(const KParams& P, const float* e, const float* ema, const float* inv, const float* inv_other, const float* g,
                   const float* g_cross, const float* dl, const float* dl_cross, float* de, hipStream_t s) {
  if (!inv || !inv_other || !env().bwd_xdma || env().force_direct || P.D != 16 || P.border != PEA_BORDER_CIRCULAR) return false;
  if (misaligned(e, 16) || misaligned(ema, 16) || misaligned(inv, 16) || misaligned(inv_other, 16)) return false;
  XPlan X, X2;
  if (!plan(P, kXdmaPSU, 0, &X) || X.C.npz > 0 || X.C.npx > kXP || X.C.npy > kXP) return false;
  if (!plan(P, kXdmaPSU, 2, &X2)) return false;
  DualArgs Q;
  Q.C2 = X2.C;
  Q.ema = ema; Q.inv_other = inv_other; Q.g_cross = g_cross; Q.dloss_cross = dl_cross;
  const dim3 grid((unsigned)(X.C.tiles_per_xcd * kXcd)), blk(kXdmaTH * kXdmaTW);
  return launch<k_bwd_xdma<16, kXdmaTH, kXdmaTW, kXdmaPSU, false, kXP, kAuxNT, 0, false, true>>(grid, blk, X.lds, s, P, X.C, e, inv, g, dl, de,
                                                                                              OtherArgs{}, Q);
}

void launch_inv_norm(const KParams& P, int dtype, const void* e, float* inv, hipStream_t s) {
  const dim3 grid((unsigned)(P.tiles_per_xcd * kXcd)), blk(kBlock);
  with_storage(dtype, [&](auto st) {
    using T = typename decltype(st)::type;
    hipLaunchKernelGGL(k_inv_norm<T>, grid, blk, 0, s, P, (const T*)e, inv);
  });
}

// pea_cross_supported: would the cross kernels take this descriptor?  mode 0: forward, 1: backward (self loss),
// 2: the cross loss with a detached second operand (forward + role-A backward)
int xdma_cross_supported(const KParams& P, int dtype, int mode) {
  if ((P.D != 16 && P.D != 32 && P.D != 64) || env().force_direct) return 0;
  if (!(mode ? env().bwd_xdma : env().fwd_xdma)) return 0;
  XPlan X;
  if (dtype == PEA_F16 || dtype == PEA_BF16) {  // pea_xdma_h16.h: 2D self loss (bf16: pea_k_xdma_h.hip builds the same scope)
    if (P.X % 8 || P.Z != 1) return 0;
    if (mode == 2 || mode == 4) {  // the cross loss with a detached second operand: forward + projection-first role-A backward
      if ((dtype == PEA_F16 && !env().h16_hw) || !env().bwd_pf || !env().fwd_xdma || (P.flags & kActMask) || P.K > kXP) return 0;
      if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0) return 0;
      return (plan(P, kXdmaPSUF, 2, &X) && X.C.npz == 0 && X.C.npx <= kXP && X.C.npy <= kXP) ? 1 : 0;
    }
    if (mode == 0) return (plan(P, kXdmaPSUF, 1, &X) && X.C.nfz == 0 && P.K <= kXP) ? 1 : 0;
    if (!plan(P, kXdmaPSUH, 0, &X) || X.C.npz > 0) return 0;
    const int xp = P.D > 32 ? 8 : kXP;
    return (X.C.npx <= xp && X.C.npy <= xp) ? 1 : 0;
  }
  if (dtype != PEA_F32) return 0;
  if (mode == 2 || mode == 4) {  // 4: does the backward of the cross loss with a detached second operand READ the raw map?
    if (!env().fwd_xdma) return 0;
    if (P.D == 32 || P.D == 64) {
      if (!env().bwd_pf || (P.flags & kActMask) || P.Z != 1 || P.K > kXP) return 0;
      if (!plan(P, kXdmaPSUF, 1, &X) || X.C.nfz > 0) return 0;
      return (plan(P, kXdmaPSUF, 2, &X) && X.C.npz == 0 && X.C.npx <= kXP && X.C.npy <= kXP) ? 1 : 0;
    }
    if (P.D != 16 || mode == 4) return 0;
    if (plan(P, kXdmaPSU, 1, &X) && X.C.nfz == 0)
      return (P.K <= kXP && plan(P, kXdmaPSU, 2, &X) && X.C.npx <= kXP && X.C.npy <= kXP) ? 1 : 0;
    // 3D volumes whose stencil steps along z (ema_embedding_loss_norm5 / norm1): the tile-per-plane instantiations
    if (!plan(P, kXdmaPSU3F, 1, &X) || X.C.nfz == 0 || P.K > kXP + 2) return 0;
    return (plan(P, kXdmaPSU3, 2, &X) && X.C.npz > 0 && X.C.npx <= 8 && X.C.npy <= 8) ? 1 : 0;
  }
  const int pm = mode == 0 ? 1 : 0;
  if (!plan(P, kXdmaPSU3, pm, &X)) return 0;
  const bool z3 = X.C.npz > 0 || X.C.nfz > 0;
  if (z3) return (P.D == 16 && X.C.npx <= 8 && X.C.npy <= 8 && P.K <= kXP + 2 && (mode || plan(P, kXdmaPSU3F, 1, &X))) ? 1 : 0;
  if (!plan(P, kXdmaPSU, pm, &X)) return 0;
  if (!mode && P.K > kXP) return 0;
  return (mode && P.D > 32 && (X.C.npx > 8 || X.C.npy > 8)) ? 0 : 1;
}

}  // namespace pea
