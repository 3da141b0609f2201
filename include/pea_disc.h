/*
 * pea_disc.h -- C ABI of the discriminative (pull / push) instance loss on the raw embedding, forward and backward (new entry points
 * of libpea_hip.so; include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea.h and pea_fgmask.h: every data
 * pointer is a DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a
 * hipStream_t (NULL = the default stream), and every refusal returns before anything is launched.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_ac3ac4/loss/loss_discriminative.py:6-60      discriminative_loss(embedding, seg_gt, background, delta_v, delta_d, alpha,
 *                                                        beta, gama), the 3D copy
 *   scripts_cvppp/loss/loss_discriminative.py            the 2D copy that keeps label 0 (= background=True)
 *   scripts_bbbc039v1/loss/loss_discriminative.py        the 2D copy that drops label 0 (= background=False)
 *
 * There, per image: torch.unique (a sort and a device -> host round trip), a Python loop over the ids, and per id a mask, a gather, a
 * mean, a norm, a relu and a mean.  Here: three streaming launches over e and two small per-cluster launches for the forward, one
 * streaming launch for the backward, no host synchronisation.
 *
 * Semantics.  e [B, D, S] (S = Z Y X pixels per image; spatial structure plays no part), labels int32 [B, S].  Per image b:
 *
 *   ids   = the distinct labels of the image, without 0 unless PEA_DISC_BACKGROUND; C_b their number, n_c the pixel count of id c
 *   mu_c  = (1 / n_c) sum_{p in c} e_p
 *   h_p   = max(|e_p - mu_c| - delta_v, 0),   u_p = (e_p - mu_c) / |e_p - mu_c|  (the zero vector where the norm is 0)
 *   var_b = (1 / C_b) sum_c (1 / n_c) sum_{p in c} h_p^2
 *   dist_b = sum_{c != c'} max(2 delta_d - |mu_c - mu_c'|, 0)^2 / (C_b (C_b - 1)) / 2   for C_b > 1, else 0 (ordered pairs)
 *   reg_b = (1 / C_b) sum_c |mu_c|
 *   loss  = (alpha sum_b var_b + beta sum_b dist_b + gamma sum_b reg_b) / B;  an image with C_b = 0 contributes 0
 *   de_p  = dloss [ k_c h_p u_p + G_c / n_c ],   k_c = 2 alpha / (B C_b n_c),   G_c = d loss / d mu_c =
 *             - k_c sum_{q in c} h_q u_q                                                        (var)
 *             - beta 2 / (B C_b (C_b - 1)) sum_{c' != c} max(2 delta_d - |mu_c - mu_c'|, 0) (mu_c - mu_c') / |mu_c - mu_c'|
 *                                                              (dist; a pair at distance exactly 0 contributes 0, as in torch)
 *             + gamma / (B C_b) mu_c / |mu_c|                                   (reg; 0 where mu_c = 0)
 *   A pixel of no counted id (label 0 without PEA_DISC_BACKGROUND, or a label outside [0, num_ids)) gets exactly 0.
 *
 * Arithmetic and its order (f32 with every step rounded on its own -- no fused multiply-add --, IEEE division and sqrtf, unless f64
 * is named).  16-bit embeddings are widened first (exact), so they give the bits of the f32 call on the widened values.
 *
 *   sums      a wave owns 256 consecutive pixels of one image, lane l the pixels 4 l + i (i = 0..3).  For each id of the
 *             wave and each channel a lane adds its pixels of that id in ascending order, the 64 lanes are added by a butterfly
 *             (xor 32, 16, .., 1), and the wave's f32 partial is added as a 128-bit fixed-point number (the integer accumulators of
 *             pea.h: exact for 2^-41 <= |v| < 2^60) into the row of (image, id).  Integer addition: any arrival order, any grid.
 *   mu_c      = (float)(sum / (double)n_c): the exact sum, divided in f64, rounded once
 *   |x|       per pixel: sqrtf(((x_0^2 + x_1^2) + x_2^2) + ..), channels in ascending order; per cluster (|mu_c|, |mu_c - mu_c'|): the
 *             squares added by a butterfly over the channels (xor D'/2, .., 1; D' = D rounded up to a power of two, the rest 0)
 *   reg_b     = (sum_c (double)|mu_c|) / C_b in f64;  its gradient (gamma / (B C_b) in f64, rounded) * (mu_c / |mu_c|)
 *   dist_b    t = 2 delta_d - |mu_c - mu_c'| (f32), hinge = t < 0 ? 0 : t, the squares hinge * hinge summed in f64, divided by
 *             (double)C_b (C_b - 1) and by 2;  its gradient: (-2 beta / (B C_b (C_b - 1)) in f64, rounded) * sum_{c'} (hinge /
 *             dist) (mu_c - mu_c'), c' in ascending order of id within a fixed partition
 *   h_p       x = |e_p - mu_c| - delta_v, h = x < 0 ? 0 : x (a select: NaN stays NaN)
 *   var_b     a wave's partial sum_{p of c in the wave} h_p h_p (lane order and butterfly as above) times w_c =
 *             (float)(1 / ((double)C_b n_c)) goes through an accumulator of the same kind per image
 *   sum h u   s_p = h_p / |e_p - mu_c| (0 where the norm is 0); a wave's partial of s_p (e_p - mu_c) per channel, accumulated as above
 *   G_c / n_c = ((-k_c * sum) + (dist part + reg part)) / (float)n_c,  k_c = (float)(2 alpha / ((double)B C_b n_c))
 *   de_p      = dloss * (k_c * (s_p * (e_p - mu_c)) + G_c / n_c), rounded once to nearest even for 16-bit de (NaN stays NaN)
 *   loss      = (alpha sum_b var_b + beta sum_b dist_b + gamma sum_b reg_b) / B in f64, images in ascending order
 *
 * Every sum that crosses waves is an integer sum or is taken by one workgroup in a fixed order, so two runs, an eager and a captured
 * run, and calls on differently aligned pointers give the same bits.
 *
 * Non-finite embeddings follow the accumulators' rule (pea.h): a NaN or +-inf pixel of image b makes var_b, possibly dist_b / reg_b,
 * and the loss NaN; de is NaN at that pixel (and at the other pixels of its cluster, whose mean is not finite).  The terms and de of
 * every OTHER image have the bits of the finite run, and the workspace is clean afterwards.
 *
 * Labels outside [0, num_ids) are counted in stats[4] and otherwise skipped: nothing is read or written outside the tables, loss and
 * stats[0..3] are NaN, the per-image entries are those of the remaining pixels, and pea_disc_loss_bwd writes 0 at such a pixel.
 */
#ifndef PEA_DISC_H_
#define PEA_DISC_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_DISC_MAX_IDS 4096
#define PEA_DISC_MAX_D 64
#define PEA_DISC_BACKGROUND 1u /* label 0 is an instance like any other (the CVPPP copy); without it label 0 is not counted */
#define PEA_DISC_NEED_GRAD 2u  /* the forward also takes the sums of h_p u_p and finishes ctx for pea_disc_loss_bwd */
#define PEA_DISC_STATS 5       /* loss, var, dist, reg, n_bad; then 4 per image: var_b, dist_b, reg_b, C_b */

typedef struct PeaDiscDesc {
  int32_t B, D;
  int64_t S;
  int32_t num_ids; /* labels are table indices: 0 <= id < num_ids <= PEA_DISC_MAX_IDS */
  int32_t dtype;   /* PEA_F32 / PEA_F16 / PEA_BF16: e and de */
  uint32_t flags;  /* PEA_DISC_BACKGROUND, PEA_DISC_NEED_GRAD */
  float delta_v, delta_d, alpha, beta, gamma;
} PeaDiscDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: B, D or S < 1; num_ids outside
 * 1..PEA_DISC_MAX_IDS; an unknown dtype; unknown flag bits; a negative or non-finite delta_v or delta_d; or PEA_E_UNSUPPORTED for
 * D > PEA_DISC_MAX_D (checked last). */
int pea_disc_validate(const PeaDiscDesc *d);

/* Host-only: bytes of the transient accumulator tables (a multiple of 8): a header of 8 words, an accumulator of 4 words per image and
 * one row of 2 + 3 D words per (image, id).  0 for a descriptor that does not validate; SIZE_MAX where the count does not fit (no
 * descriptor that validates reaches it: B < 2^31, num_ids <= 4096, D <= 64). */
size_t pea_disc_workspace_bytes(const PeaDiscDesc *d);

/* Prepare `bytes` bytes at `workspace` (8-byte aligned, bytes >= 64 and a multiple of 8) once per allocation: all zero but for a
 * magic word.  Every pea_disc_loss_fwd leaves the block like that for the next call on the same stream; a block that was never
 * prepared gives NaN in loss and in every entry of stats.  PEA_E_NULL / PEA_E_ALIGN / PEA_E_WORKSPACE (bytes < 64 or not a multiple
 * of 8). */
int pea_disc_workspace_init(void *workspace, size_t bytes, void *stream);

/* Host-only: bytes of what the forward leaves for the backward (a multiple of 8): per image C_b, dist_b and reg_b; per (image, id)
 * n_c, the compacted id list, k_c and w_c; per (image, id, channel) mu_c and the finished G_c / n_c; every array padded to 8 bytes.
 * 0 for a descriptor that does not validate; SIZE_MAX where the count does not fit (as above: never reached).  The forward writes
 * every byte of it.  It stays valid until the caller overwrites it. */
size_t pea_disc_context_bytes(const PeaDiscDesc *d);

/* e [B, D, S] of dtype; labels int32 [B, S]; loss f32 [1]; stats f64 [PEA_DISC_STATS + 4 B] = { loss, var, dist, reg, n_bad, then per
 * image var_b, dist_b, reg_b, C_b }: var, dist and reg are batch means without alpha / beta / gamma, loss[0] == (float)stats[0].
 * n_bad != 0: loss and stats[0..3] are NaN.
 * ctx is needed by EVERY call: the means travel through it from the second launch to the third.  Without PEA_DISC_NEED_GRAD the sums
 * of h_p u_p are skipped and the G_c / n_c of ctx lack their var part: such a ctx must not be handed to pea_disc_loss_bwd.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_disc_validate refuses
 *   PEA_E_NULL         e, labels, loss, stats or ctx is NULL
 *   PEA_E_ALIGN        e not aligned to its element, labels or loss not 4-byte, stats, ctx or workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_disc_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  S > 2^31 - 1, or more than 2^31 - 1 workgroups (one per 1024 pixels of an image)
 * Any element-aligned pointer and any S is served with the same bits (the alignment contract of pea.h): alignment to four elements
 * only selects wide loads. */
int pea_disc_loss_fwd(const PeaDiscDesc *d, const void *e, const int32_t *labels, float *loss, double *stats, void *ctx,
                      void *workspace, size_t workspace_bytes, void *stream);

/* de [B, D, S] of dtype = dloss[0] * d loss / d e from the ctx of a PEA_DISC_NEED_GRAD forward on the same e and labels (the flag is
 * not looked at here); dloss is a DEVICE f32 scalar, NULL = 1.  Every element of de is written, the exact zeros of uncounted pixels
 * included.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_disc_validate refuses
 *   PEA_E_NULL         e, labels, ctx or de is NULL
 *   PEA_E_ALIGN        e or de not aligned to its element, labels or dloss not 4-byte, ctx not 8-byte aligned
 *   PEA_E_UNSUPPORTED  S > 2^31 - 1, or more than 2^31 - 1 workgroups (one per 1024 pixels of an image) */
int pea_disc_loss_bwd(const PeaDiscDesc *d, const void *e, const int32_t *labels, const void *ctx, const float *dloss, void *de,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_DISC_H_ */
