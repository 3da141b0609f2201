/*
 * pea_multi_labels.h -- C ABI of the batched self losses evaluated straight from LABEL IMAGES (new entry points of libpea_hip.so;
 * include/pea.h, pea_multi.h, pea_infer.h and pea_flip.h are unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea.h and
 * pea_multi.h: every data pointer is a DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised,
 * `void *stream` is a hipStream_t (NULL = the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity): the four deep-supervision self losses of a training
 * step (scripts_cvppp/main.py:284-287, scripts_ac3ac4/main.py:227-230) TOGETHER WITH the data they are fed with -- the
 * nearest-downsampled label images and what the providers derive from them,
 *
 *   scripts_cvppp/data/data_provider.py:200-225               cv2.resize(label, fx = 1/2 .. 1/16, INTER_NEAREST), gen_affs_ours,
 *                                                             weight_binary_ratio per channel
 *   scripts_ac3ac4/data/data_provider_labeled_deep.py:225-256 the same per slice, seg_to_aff
 *
 * Up to four losses become one count launch (the class-balance tables), one fused forward + backward launch and one loss finish.
 * Each entry samples either a label image of its own (label_step = {1,1,1}) or a larger one with an integer step: where the size of
 * the full-resolution image is a multiple of the scale's, OpenCV's nearest rule (src = floor(dst / f)) IS the plain stride, so the
 * four scales read the one label image the GPU already holds.
 *
 * Semantics.  Per entry the results are exactly those of pea_affinity_fwd_bwd_labels (include/pea.h) for a self loss
 * (e_other == NULL) on the label image L'[b][z][y][x] = labels[b][z * sz][y * sy][x * sx]: target / mask / weight as the comment
 * above pea_label_weights says (flags: PEA_TGT_PADDING, PEA_TGT_BOTH_FOREGROUND, PEA_TGT_MASK_INSIDE), N_i the normaliser of
 * pea.h, the loss through the integer accumulators of the state block, de in gather form without atomics: loss, map and gradient
 * are bit-reproducible from run to run.  Where `wtab` is NULL the class-balance table is computed by the call from integer counts
 * of t_i != 0 per (image, channel) over all S voxels of the scale (a neighbour outside the image counts as PEA_TGT_PADDING says)
 * with the f64 formula of pea_label_weights -- the same bits that call writes for the materialised image L'.
 *
 * The fused set.  pea_multi_labels_supported(entries, n, flags) == 1 exactly when
 *   - 1 <= n <= PEA_MULTI_MAX_N and every descriptor passes pea_desc_validate,
 *   - dtype is PEA_F32, PEA_F16 or PEA_BF16 and THE SAME for all n entries (as in pea_multi.h: mixed tables are outside the set),
 *     D is 16 or 32, K <= PEA_MULTI_MAX_K, the border is PEA_BORDER_CIRCULAR or PEA_BORDER_CROP_ZERO,
 *     neither PEA_FLAG_LOSS_ACT nor PEA_FLAG_MASK_F32 is set,
 *   - flags holds nothing but PEA_TGT_PADDING, PEA_TGT_BOTH_FOREGROUND, PEA_TGT_MASK_INSIDE,
 *   - every label_step >= 1 and (dims[a] - 1) * label_step[a] + 1 <= label_dims[a] on every axis (no sampled index leaves the image),
 *   - B * LZ * LY * LX and S * max(D, K) fit int32, every offset component fits int16,
 *   - the tiles (256 voxels) of all entries fit one grid.
 * For any other table the call returns PEA_E_UNSUPPORTED and the caller makes the n single calls on materialised label images.
 *
 * 16-bit storage: as in pea_multi.h.  e is read and de is written in the descriptor's dtype (element alignment: 2 bytes, any S);
 * the arithmetic in between is that of the f32 table, so affs and loss_out carry the bits of the f32 call on the upcast embedding
 * and de is that call's de rounded once to nearest even (NaN stays NaN).  labels, wtab, affs, loss_out and dloss keep their types.
 */
#ifndef PEA_MULTI_LABELS_H_
#define PEA_MULTI_LABELS_H_

#include "pea_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PeaMultiLabels { /* one self loss evaluated from labels */
  const PeaDesc *desc;          /* geometry of THIS scale, D, K, offsets, lambda, norm, eps, border, activation bits of affs */
  const void *e;                /* [B, D, Z, Y, X] in desc->dtype (f32 / f16 / bf16) */
  const int32_t *labels;        /* [B, LZ, LY, LX] int32, dense */
  int32_t label_dims[3];        /* LZ, LY, LX */
  int32_t label_step[3];        /* label of voxel (z,y,x) of this scale = labels[b][z*sz][y*sy][x*sx]; {1,1,1}: an image of its own */
  const float *wtab;            /* [B, K, 2] as pea_label_weights writes it, or NULL: computed by this call */
  float *affs;                  /* [B, K, Z, Y, X], nullable */
  float *loss_out;              /* [1 + K] */
  const float *dloss;           /* device scalar or NULL = 1 */
  void *de;                     /* [B, D, Z, Y, X] in desc->dtype, like e */
} PeaMultiLabels;

/* host-only: 1 when the table is in the fused set (above), else 0 (also for NULL entries or a NULL / invalid descriptor).  No
 * pointer but `desc` is looked at.  No GPU needed. */
int pea_multi_labels_supported(const PeaMultiLabels *entries, int n, unsigned flags);

/* host-only: bytes of `scratch` for the table: the integer counts, one uint32 per (entry, image, channel) = 4 * sum_j B_j K_j
 * (0 for a table the call would refuse). */
size_t pea_multi_labels_scratch_bytes(const PeaMultiLabels *entries, int n);

/* n self losses, forward and backward.  `entries` is a HOST array, read during the call only.  `workspace` holds n loss states back
 * to back, as for pea_affinity_fwd_multi: entry i adds into state i, every state is left zero for the next call.  `scratch`
 * (4-byte aligned, pea_multi_labels_scratch_bytes; contents undefined before and after) is zeroed by the call itself; it is only
 * looked at when at least one entry has wtab == NULL -- if every entry brings a table no count launch is made and scratch may be NULL.
 * Returns n < 1 or n > PEA_MULTI_MAX_N: PEA_E_DESC; PEA_E_NULL for missing entries; then per entry, in table order, the
 * descriptor's own code (PEA_E_NULL where it is missing; PEA_E_DESC also for PEA_FLAG_MASK_F32, as the labels-in calls of pea.h),
 * PEA_E_NULL (e, labels, loss_out or de missing), PEA_E_ALIGN (element alignment: 4 bytes, 2 for e / de of a 16-bit entry);
 * then PEA_E_ALIGN for `workspace` (8 bytes) or `scratch` (4); PEA_E_WORKSPACE for a missing or short workspace or scratch;
 * PEA_E_UNSUPPORTED where pea_multi_labels_supported is 0.
 * Two entries whose output buffers (affs, loss_out, de) overlap are the CALLER'S error, as in pea_multi.h. */
int pea_affinity_fwd_bwd_labels_multi(const PeaMultiLabels *entries, int n, unsigned flags, void *workspace, size_t workspace_bytes,
                                      void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_MULTI_LABELS_H_ */
