/*
 * pea_cc.h -- C ABI of connected-component labelling on the device: label, size filter, mask (new entry points of libpea_hip.so;
 * include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_fgmask.h and pea_instscore.h: every data pointer
 * is a DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t
 * (NULL = the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_bbbc039v1/utils/postprocessing.py:43-48   remove_samll_object: skimage.morphology.label(mask), remove_small_objects(
 *                                                     min_size=25), binarise -- between the argmax mask and seg_mutex in the
 *                                                     validation loop (scripts_bbbc039v1/main.py:406-414, inference.py:185-195)
 *   scripts_bbbc039v1/utils/merge_small.py:106        vigra.analysis.labelVolumeWithBackground: a segmentation split into its pieces
 *   scripts_bbbc039v1/convert_mask2ins.py:33          skimage.morphology.label
 *
 * Semantics.  Two pixels p, q of ONE image are joined iff they are neighbours under `connectivity`, in[p] != 0 and in[p] == in[q].
 * Background is 0; nothing wraps and the images of a batch never touch.  On a mask that gives the foreground components; on an int32
 * label image it splits every id into its connected pieces (skimage.morphology.label on a multi-valued image, vigra's
 * labelVolumeWithBackground); a negative id is an ordinary non-zero value.
 *
 * Numbering.  A component is KEPT iff it has at least min_size pixels (0 and 1 keep every component).  The kept components of an
 * image get the ids 1 .. n_kept in raster order of their FIRST pixel, the smallest flat index (z * Y + y) * X + x among a component's
 * pixels.  For min_size <= 1 that is the numbering of scipy.ndimage.label and of skimage.morphology.label.
 *
 * Outputs.  labels_out[p] = the id, 0 for background and for dropped components; mask_out[p] = [labels_out[p] != 0] -- with a 2D
 * mask, connectivity 2 and min_size 25 the reference's remove_samll_object; counts[b] = { components found, components kept }.  At
 * least one of labels_out / mask_out is given; `in` overlaps no output.  Every number is an exact integer: a root is a minimum and a
 * size is an integer sum, so the result does not depend on the order in which workgroups arrive and two runs give the same bits.
 *
 * The workspace is scratch, not state: it needs no preparation, every word that is read was written by the same call, its contents
 * afterwards are unspecified, and the same block serves any later call that it is large enough for.
 *
 * Termination (csrc/pea_k_cc.hip).  The launches are: tile pass, border merge, compress and count, three for the scan (block
 * totals, one workgroup per image over the totals, apply) and the write.  A parent is only ever replaced by a strictly smaller index
 * of the same component, so every find and every union ends; the tile pass ends on a workgroup-wide vote over labels that only fall;
 * no workgroup waits for another one -- launch boundaries are the only ordering between workgroups.
 */
#ifndef PEA_CC_H_
#define PEA_CC_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_CC_IN_U8 0  /* in holds uint8 (also torch.bool) */
#define PEA_CC_IN_I32 1 /* in holds int32 */

typedef struct PeaCcDesc {
  int32_t ndim;          /* 2 or 3 */
  int32_t B, dims[3];    /* in [B, Z, Y, X] dense; ndim == 2: dims[0] == 1 */
  int32_t in_type;       /* PEA_CC_IN_U8 (uint8 / bool) or PEA_CC_IN_I32 */
  int32_t connectivity;  /* skimage's meaning: 1 .. ndim.  2D: 1 = 4-, 2 = 8-neighbourhood; 3D: 1 = 6, 2 = 18, 3 = 26 */
  int32_t min_size;      /* >= 0: components with fewer pixels are dropped (0 and 1 drop nothing) */
  uint32_t flags;        /* none yet; unknown bits are PEA_E_DESC */
} PeaCcDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: ndim not 2 or 3; B or a dim < 1; ndim == 2
 * with dims[0] != 1; connectivity outside 1 .. ndim; a negative min_size; an unknown in_type; any flag bit. */
int pea_cc_validate(const PeaCcDesc *d);

/* Host-only: the bytes of workspace that pea_cc_label needs (two int32 words per pixel and two per 1024 pixels of an image, a
 * multiple of 8); 0 for a descriptor that does not validate; SIZE_MAX where the count does not fit. */
size_t pea_cc_workspace_bytes(const PeaCcDesc *d);

/* in [B, S] of in_type (S = Z * Y * X); labels_out int32 [B, S] or NULL; mask_out uint8 [B, S] or NULL; counts int32 [B, 2].
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_cc_validate refuses
 *   PEA_E_NULL         in or counts is NULL, or labels_out and mask_out are both NULL
 *   PEA_E_ALIGN        an int32 `in`, labels_out, counts or the workspace is not 4-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_cc_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  Z * Y * X >= 2^31, or more than 2^31 - 1 workgroups (one per 32 x 32 tile of a plane; one per 1024 pixels
 *                      of an image)
 * Any element-aligned pointer and any extent is served, with the same result. */
int pea_cc_label(const PeaCcDesc *d, const void *in, int32_t *labels_out, uint8_t *mask_out, int32_t *counts, void *workspace,
                 size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_CC_H_ */
