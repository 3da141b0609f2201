/*
 * pea_instscore.h -- C ABI of the instance scores of the BBBC039V1 validation loop: the aggregated Jaccard index, the panoptic quality
 * and the pixel F1, from ONE contingency table per image (new entry points of libpea_hip.so; include/pea.h and include/pea_segscore.h
 * are unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_segscore.h: every data pointer is a DEVICE pointer owned by
 * the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and
 * every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_bbbc039v1/main.py:425-429, inference.py:201-205   agg_jc_index, pixel_f1, remap_label and get_fast_pq(match_iou=0.5) of
 *                                                             utils/metrics_bbbc.py: one full-image mask per instance, two or three
 *                                                             full-image passes per (gt instance, pred id) pair
 *
 * All three scores are functions of the joint histogram n_ij = #{pixels with pred = i and gt = j}, which the streaming pass of
 * pea_seg_scores builds.  Here: that pass, one launch over the table's slots (marginals, pixel counts, row lengths), one scan per image
 * (the table as a CSR by gt id, the sorted list of present gt ids), one launch over the slots (the PQ pairs; the scatter into the
 * rows), the AJI walk (one wave per image), and one launch that writes the columns and puts the workspace back.
 *
 * Semantics.  pred, gt int32 [B, S] with ids in [0, max_id]; background is label 0 (NOT the lowest label, which the Dice scores of
 * pea_segscore.h use).  Per image, a_i = sum_j n_ij, b_j = sum_i n_ij.
 *
 *   AJI (agg_jc_index(gt, pred)).  C = U = 0, used = {}.  For each present gt id j = 1, 2, .. in increasing order (present: b_j > 0,
 *   a gt id that overlaps only pred 0 included): among the pred ids i >= 1 that are not used and have n_ij > 0, the winner is the one
 *   with the greatest iou = n_ij / (b_j + a_i - n_ij) (one f64 division, compared as f64), ties to the lowest id; inter = n_ij,
 *   union = b_j + a_i - n_ij.  If there is none, the winner is pred id 1 whether or not it occurs in pred: inter = 0, union = b_j + a_1
 *   if id 1 is not used (a_1 = 0 when absent), b_j if it is.  C += inter, U += union, the winner is used, aji_match[j] = winner.
 *   After the walk U += sum of a_i over the present pred ids i >= 1 that were never used.  aji = C / U, one f64 division; 0 / 0 = NaN.
 *   Two inputs that the reference does not define are defined here: a gt id ABSENT between 1 and the maximum is skipped (the
 *   reference divides 0 by 0 there and its result depends on how argmax orders NaNs), and a pred without any id > 0 gives aji = 0,
 *   or NaN when gt has none either (the reference raises).
 *
 *   PQ (get_fast_pq, match_iou >= 0.5).  Over the pairs i >= 1, j >= 1 with n_ij > 0: iou = n_ij / (a_i + b_j - n_ij); a pair counts
 *   where iou > match_iou (f64).  tp = their number, sum_iou = the sum of their iou, fp = n_pred_ids - tp, fn = n_gt_ids - tp,
 *   dq = tp / (tp + 0.5 fp + 0.5 fn), sq = sum_iou / (tp + 1e-6), pq = dq * sq; IEEE divisions: an image without instances on either
 *   side gives dq = pq = NaN and sq = 0.  pq_match[j] = the pred id paired with gt id j or 0 (for match_iou >= 0.5 the pairing is
 *   unique).  remap_label plays no part: the score does not depend on the numbering, and pq_match speaks in the caller's ids.
 *
 *   Pixel F1 (pixel_f1).  pix_tp / pix_fp / pix_fn count (pred > 0, gt > 0); pixel_f1 = 2 tp / (2 tp + fp + fn), 0 where that
 *   denominator is 0 (sklearn's answer).
 *
 * A negative label or one above max_id is counted in n_bad and its pixel is skipped; a pair without a free slot is counted (its
 * pixels) in n_overflow.  Either makes every other column of THAT image NaN and zeroes its rows of the match tables; the other images
 * keep the bits of a clean call.
 *
 * Arithmetic.  All counts are exact u64 integers, the quotients single f64 divisions, maxima are taken on the f64 bit patterns with
 * the id as tie-break, and sum_iou is a fixed-point integer sum with 32 fractional bits, each term truncated.  Every column is
 * bit-reproducible across runs, capacities that do not overflow, pointer alignments, and eager against captured execution.  aji, dq,
 * pixel_f1 and the integer columns equal exact arithmetic rounded once; sq and pq are within 2^-32 per term of it.
 */
#ifndef PEA_INSTSCORE_H_
#define PEA_INSTSCORE_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_INST_MIN_CAPACITY 64
#define PEA_INST_MAX_ID 65535
#define PEA_INST_COLS 18
/* the columns of out [B][PEA_INST_COLS] */
#define PEA_INST_N_OVERFLOW 0
#define PEA_INST_N_BAD 1
#define PEA_INST_AJI 2
#define PEA_INST_AJI_INTER 3 /* C and U of the walk */
#define PEA_INST_AJI_UNION 4
#define PEA_INST_DQ 5
#define PEA_INST_SQ 6
#define PEA_INST_PQ 7
#define PEA_INST_TP 8
#define PEA_INST_FP 9
#define PEA_INST_FN 10
#define PEA_INST_SUM_IOU 11
#define PEA_INST_PIXEL_F1 12
#define PEA_INST_PIX_TP 13
#define PEA_INST_PIX_FP 14
#define PEA_INST_PIX_FN 15
#define PEA_INST_N_PRED_IDS 16 /* distinct ids > 0 of pred, of gt */
#define PEA_INST_N_GT_IDS 17

typedef struct PeaInstDesc {
  int32_t B;
  int64_t S;
  int64_t capacity; /* slots per image of the pair table: a power of two >= 64, as PeaSegDesc */
  int32_t max_id;   /* ids of pred and gt lie in [0, max_id]; 1 <= max_id <= 65535 */
  double match_iou; /* PQ pairing threshold; >= 0.5 (below it the reference runs Munkres: PEA_E_UNSUPPORTED) */
  uint32_t flags;   /* none defined: must be 0 */
} PeaInstDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: B or S < 1; a capacity below
 * PEA_INST_MIN_CAPACITY, above 2^31 or no power of two; max_id < 1 or > PEA_INST_MAX_ID; a match_iou that is NaN, negative or above
 * 1; any flag bit; or PEA_E_UNSUPPORTED for match_iou < 0.5 (the Munkres branch) or S > 2^31 - 1 (checked last). */
int pea_inst_validate(const PeaInstDesc *d);

/* Host-only: bytes of the workspace (a multiple of 8): a header of 8 words, 32 words per image, 6 words per (image, slot), 2 words per
 * (image, present gt id) with room for min(max_id + 1, capacity) of them, and three int32 per (image, id), padded to 8 bytes together.
 * Strictly increasing in B, capacity and max_id; S plays no part.  0 for a descriptor that does not validate; SIZE_MAX where the
 * count does not fit. */
size_t pea_inst_workspace_bytes(const PeaInstDesc *d);

/* Prepare `bytes` bytes at `ws` (8-byte aligned, bytes >= 64 and a multiple of 8) once per allocation: all zero but for a magic word.
 * Every pea_inst_scores leaves the block like that for the next call on the same stream, whatever its descriptor; a block that was
 * never prepared gives NaN in every column and zero match tables.  PEA_E_NULL / PEA_E_ALIGN / PEA_E_WORKSPACE. */
int pea_inst_workspace_init(void *ws, size_t bytes, void *stream);

/* pred, gt int32 [B, S]; out f64 [B][PEA_INST_COLS]; aji_match, pq_match int32 [B][max_id + 1], either may be NULL.  Every element
 * of what is given is written.  Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_inst_validate refuses
 *   PEA_E_NULL         pred, gt or out is NULL
 *   PEA_E_ALIGN        pred, gt, aji_match or pq_match not 4-byte, out or ws not 8-byte aligned
 *   PEA_E_WORKSPACE    ws is NULL or shorter than pea_inst_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 1024 pixels of an image, one per 256 slots)
 * Any element-aligned pointer and any S is served with the same bits: alignment to four elements only selects wide loads.  Every
 * loop is bounded (probes by capacity, the walk by the present gt ids, a row by its length): a full table drops pairs (n_overflow),
 * it never stalls a kernel. */
int pea_inst_scores(const PeaInstDesc *d, const int32_t *pred, const int32_t *gt, double *out, int32_t *aji_match, int32_t *pq_match,
                    void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_INSTSCORE_H_ */
