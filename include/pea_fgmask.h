/*
 * pea_fgmask.h -- C ABI of the foreground-mask term of the BBBC039V1 step: the class-balanced two-class cross-entropy on the
 * `binary_seg` logits, forward and backward, and the validation mask (new entry points of libpea_hip.so; include/pea.h is unchanged
 * and PEA_ABI_VERSION stays 2).  Same conventions as pea.h and pea_metrics.h: every data pointer is a DEVICE pointer owned by the
 * caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and
 * every refusal returns before anything is launched.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_bbbc039v1/main.py:289      loss_mask = mask_weight(1000) * BCE_loss_func(pred_mask, torch.gt(target_ins[:, 0], 0),
 *                                                                                    weight_rate=[10, 1])
 *   scripts_bbbc039v1/loss/loss.py:187-194
 *       weight = torch.FloatTensor([torch.sum(target == 1).item(), torch.sum(target == 0).item()]).cuda()
 *       loss   = nn.CrossEntropyLoss(weight=weight)(output, target.squeeze(1).long())
 *   scripts_bbbc039v1/main.py:385, scripts_cvppp/inference.py:190     the same call in both validation loops
 *   scripts_bbbc039v1/main.py:406-410  softmax -> argmax -> .cpu() -> uint8 -> [92:-92, 4:-4]: the validation mask
 *   model/unet2d_residual.py:309-314, 348                             pred_mask: the two-channel output of the binary_seg head
 *
 * There: two .item() calls -- two device -> host round trips per step, which also keep the step out of a captured graph -- before
 * the class weights exist, then the comparison, two reductions, log_softmax, nll_loss and their autograd nodes.  Here: ONE
 * streaming launch that reads every logit and label once plus one small finish; ONE streaming launch for the gradient.  The sums go
 * through the integer accumulators of the training forward (pea_workspace_init, pea.h), so every number is bit-reproducible.
 *
 * Semantics.  Per pixel p of image b:  y = [label > 0],  d = l1 - l0  (l_c = logits[b, c, p]),  z = y ? -d : d,
 *
 *   nll = -log softmax(l)[y] = softplus(z) = (z > 0 ? z : 0) + log1pf(expf(-|z|))
 *   n0 = #(y == 0), n1 = #(y == 1);  S0, S1 = the sums of nll over each class
 *   class weights w[0] = n1, w[1] = n0 (loss.py:189; `weight_rate` is ignored there)
 *   loss = sum(w_y nll) / sum(w_y) = S0 / (2 n0) + S1 / (2 n1) = 0.5 (S0 / n0 + S1 / n1)
 *   gradient: s = 1 / (1 + expf(-z)),  q = (y ? -s : s) c_y  with  c_y = dloss / (2 n_y)      ( = (softmax(l)[1] - y) c_y )
 *             dlogits[b, 1, p] = q,  dlogits[b, 0, p] = -q
 *
 * Every step up to nll and q is f32, rounded on its own (no fused multiply-add), with the accurate expf / log1pf and IEEE division;
 * 16-bit logits are widened first (exact), so they give the bits of the f32 call on the widened values.  A workgroup sums its terms in
 * f32 in a fixed order and adds the partial into the state of its quantity; the counts are exact.  The finish divides in f64.
 *
 * An absent class (n0 == 0 or n1 == 0) is 0 / 0 in the reference: the loss is NaN and so is EVERY element of the gradient (the
 * weight of the only class present is the count of the absent one, 0).  That is the default here too.  With
 * PEA_FG_SKIP_EMPTY_CLASS the term of an absent class is 0 and the class that is present keeps its c_y.
 *
 * Non-finite logits follow the accumulators' rule (pea.h): a NaN term makes its class's mean and the loss NaN; dlogits is NaN at
 * that pixel only, every other element has the bits of the finite run, and the states are clean for the next call.
 *
 * pea_fgmask_argmax writes [l1 > l0] (a tie or a NaN gives 0).  That is the reference's argmax(softmax(l)) -- argmax takes the first
 * maximum -- except where the f32 softmax rounds two DISTINCT logits to equal probabilities (|d| below about 2^-24 relative):
 * the reference then answers 0 and this call answers [l1 > l0].
 */
#ifndef PEA_FGMASK_H_
#define PEA_FGMASK_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_FG_LABELS_I32 0          /* labels hold int32, signed: foreground <=> label > 0 (an instance image as it comes) */
#define PEA_FG_LABELS_U8 1           /* labels hold uint8 (also torch.bool): foreground <=> label != 0 */
#define PEA_FG_SKIP_EMPTY_CLASS 1u   /* the term of an absent class is 0 instead of NaN */
#define PEA_FG_STATS 5               /* loss, S0 / n0, S1 / n1, n0, n1 */

typedef struct PeaFgDesc {
  int32_t B, Y, X;                /* logits [B, 2, Y, X] dense, labels [B, Y, X] dense */
  int32_t logits_dtype;           /* PEA_F32 / PEA_F16 / PEA_BF16: logits and dlogits */
  int32_t labels_type;            /* PEA_FG_LABELS_I32 / PEA_FG_LABELS_U8 */
  uint32_t flags;                 /* PEA_FG_SKIP_EMPTY_CLASS */
  int32_t origin[2], out_dims[2]; /* pea_fgmask_argmax only: the crop (y, x); origin + out_dims <= (Y, X) */
} PeaFgDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: B, Y or X < 1; an unknown logits_dtype or
 * labels_type; unknown flag bits; a negative origin or out_dims, or a crop that leaves (Y, X).  out_dims of (0, 0) pass: the loss
 * calls do not look at the crop. */
int pea_fgmask_validate(const PeaFgDesc *d);

/* Host-only: the workspace of pea_fgmask_loss_fwd, ONE loss state (S0, S1, n0, n1 are four of its indices) = pea_workspace_bytes().
 * Prepare it once with pea_workspace_init; the finish puts the state back to zero, so the block serves any later pea_* call on
 * the stream. */
size_t pea_fgmask_workspace_bytes(void);

/* logits [B, 2, Y, X] of logits_dtype; labels [B, Y, X] of labels_type; loss f32 [1]; stats f64 [PEA_FG_STATS] =
 * { loss, S0 / n0, S1 / n1, n0, n1 } and loss[0] = (float)stats[0].  A state that was never initialised gives NaN in all of them.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_fgmask_validate refuses
 *   PEA_E_NULL         logits, labels, loss or stats is NULL
 *   PEA_E_ALIGN        logits or int32 labels not aligned to their element, loss not 4-byte, stats or workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_fgmask_workspace_bytes()
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 4096 pixels of an image)
 * Any element-aligned pointer and any Y * X is served with the same bits (the alignment contract of pea.h): alignment to four
 * elements only selects wide loads. */
int pea_fgmask_loss_fwd(const PeaFgDesc *d, const void *logits, const void *labels, float *loss, double *stats, void *workspace,
                        size_t workspace_bytes, void *stream);

/* dlogits [B, 2, Y, X] of logits_dtype = dloss[0] * d loss / d logits; dloss is a DEVICE f32 scalar, NULL = 1.  Of stats only
 * stats[3] and stats[4] (the counts) are read.  16-bit values are rounded once to nearest even, NaN stays NaN.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_fgmask_validate refuses
 *   PEA_E_NULL         logits, labels, stats or dlogits is NULL
 *   PEA_E_ALIGN        logits, dlogits or int32 labels not aligned to their element, dloss not 4-byte, stats not 8-byte aligned
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 4096 pixels of an image) */
int pea_fgmask_loss_bwd(const PeaFgDesc *d, const void *logits, const void *labels, const double *stats, const float *dloss,
                        void *dlogits, void *stream);

/* mask_out u8 [B, out_dims[0], out_dims[1]] = [l1 > l0] at (origin + p): the validation mask, cropped on the device.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_fgmask_validate refuses, or an out_dims < 1
 *   PEA_E_NULL         logits or mask_out is NULL
 *   PEA_E_ALIGN        logits not aligned to its element
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 1024 pixels of the output) */
int pea_fgmask_argmax(const PeaFgDesc *d, const void *logits, uint8_t *mask_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_FGMASK_H_ */
