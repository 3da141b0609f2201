/*
 * pea_segscore.h -- C ABI of the segmentation scores of the validation loops, from ONE contingency table per image (new entry points
 * of libpea_hip.so; include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_disc.h and pea_metrics.h: every
 * data pointer is a DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a
 * hipStream_t (NULL = the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_cvppp/main.py:413-417 (scripts_bbbc039v1/main.py likewise)   SymmetricBestDice, AbsDiffFGLabels (utils/evaluate.py: a Python
 *                                                                        double loop over label pairs, full-image numpy passes per pair),
 *                                                                        skimage's adapted_rand_error and variation_of_information
 *   scripts_ac3ac4/main.py:322-327, inference.py:199-244                 VOI and ARAND per validation volume, waterz and LMC
 *
 * Every one of these scores is a function of the joint histogram n_ij = #{pixels with pred = i and gt = j} of the two label images.
 * Here: one streaming launch over the pixels builds that table, three launches over table SLOTS take the marginals, the best Dice per
 * segment and the sums, one small launch writes the columns.  No host synchronisation: the call can be captured in a graph.
 *
 * Semantics.  pred, gt int32 [B, S] (S pixels per image; spatial structure plays no part).  Per image, with a_i = sum_j n_ij (the
 * pixels of pred id i), b_j = sum_i n_ij, minP / maxP / minG / maxG the lowest and highest label of pred / gt:
 *
 *   best_dice      BestDice(pred, gt) of utils/evaluate.py:21-59: background is the LOWEST label of each image (not 0);
 *                    sum_{i present, i > minP}  max_{j present, j > minG}  2 n_ij / (a_i + b_j)   /   (maxP - minP)
 *                  (absent integers between min and max count as 0, as the reference's range() loop does); 0 when maxP == minP
 *   best_dice_rev  BestDice(gt, pred): the same with the roles exchanged
 *   sbd            min(best_dice, best_dice_rev)                                                 (SymmetricBestDice)
 *   diff_fg        (maxP - minP) - (maxG - minG)                                                 (DiffFGLabels; |.| is AbsDiffFGLabels)
 *   fgbg_dice      2 #{pred != minP and gt != minG} / (#{pred != minP} + #{gt != minG}), 0 where the denominator is 0   (FGBGDice)
 *
 * The following use only the pixels with gt != 0 (skimage's ignore_labels=(0,) on image_true, the only form the drivers use); N' is
 * their number, a'_i = sum_{j != 0} n_ij, and every sum over j leaves j = 0 out:
 *
 *   voi_split      H(pred | gt) = (sum_j b_j log2 b_j - sum_ij n_ij log2 n_ij) / N'      in bits
 *   voi_merge      H(gt | pred) = (sum_i a'_i log2 a'_i - sum_ij n_ij log2 n_ij) / N'
 *   are            1 - P2 / (0.5 A2 + 0.5 B2),  P2 = sum_ij n_ij^2 - N',  A2 = sum_i a'_i^2 - N',  B2 = sum_j b_j^2 - N'
 *   are_precision  P2 / A2  (over the pred segments)
 *   are_recall     P2 / B2  (over the gt segments)
 *   N' = 0 (gt is all 0): voi_split = voi_merge = 0 and are, are_precision, are_recall follow 0 / 0: NaN.  A2 = 0 or B2 = 0 with
 *   N' > 0 (every counted pixel a segment of its own) follows IEEE division likewise.
 *
 * Negative labels are not ids: each negative value of pred or gt is counted in n_bad and its pixel is skipped.  A pair that finds no
 * free slot in the table is counted (its pixels) in n_overflow and dropped.  If n_bad or n_overflow of an image is non-zero, every
 * other column of THAT image is NaN; the other images keep the bits of a clean call.
 *
 * Arithmetic.  Counts, squares and the marginals are exact integer sums (u64; S <= 2^31 - 1).  A term n log2 n (f64 log2) and a best
 * Dice (the f64 quotient 2 n_ij / (a_i + b_j), its maximum taken on the bit patterns, which order like the values) enter their sum
 * as fixed-point integers with 32 fractional bits, truncated: integer addition, any arrival order.  The quotients of the finish are
 * IEEE f64 divisions of those integers.  Slot placement depends on arrival order, but no floating-point sum runs over slots, so two
 * runs, an eager and a captured run, calls on differently aligned pointers and calls with different capacities that do not overflow
 * give the same bits in every column.  Against exact arithmetic: the Dice columns and the VOI columns are within 2^-31 (one
 * truncation of 2^-32 per term, at most as many terms as the divisor counts), the are* columns within a few ulp.
 * Integer columns above 2^53 are rounded to f64 on output.
 */
#ifndef PEA_SEGSCORE_H_
#define PEA_SEGSCORE_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_SEG_MIN_CAPACITY 64
#define PEA_SEG_COLS 19
/* the columns of out [B][PEA_SEG_COLS] */
#define PEA_SEG_N_OVERFLOW 0
#define PEA_SEG_N_BAD 1
#define PEA_SEG_BEST_DICE 2
#define PEA_SEG_BEST_DICE_REV 3
#define PEA_SEG_SBD 4
#define PEA_SEG_DIFF_FG 5
#define PEA_SEG_FGBG_DICE 6
#define PEA_SEG_VOI_SPLIT 7
#define PEA_SEG_VOI_MERGE 8
#define PEA_SEG_ARE 9
#define PEA_SEG_ARE_PRECISION 10
#define PEA_SEG_ARE_RECALL 11
#define PEA_SEG_SUM_NIJ2 12 /* sum_ij n_ij^2, sum_i a'_i^2, sum_j b_j^2 and N' over the pixels with gt != 0 */
#define PEA_SEG_SUM_AI2 13
#define PEA_SEG_SUM_BJ2 14
#define PEA_SEG_N_PRIME 15
#define PEA_SEG_N_PRED_IDS 16 /* distinct ids of pred, of gt, and distinct (pred, gt) pairs of the whole image */
#define PEA_SEG_N_GT_IDS 17
#define PEA_SEG_N_PAIRS 18

typedef struct PeaSegDesc {
  int32_t B;
  int64_t S;
  int64_t capacity; /* slots per image of the pair table (and of the two marginal tables): a power of two >= 64 */
  uint32_t flags;   /* none defined: must be 0 */
} PeaSegDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: B or S < 1; a capacity below
 * PEA_SEG_MIN_CAPACITY, above 2^31 or no power of two; any flag bit; or PEA_E_UNSUPPORTED for S > 2^31 - 1 (checked last). */
int pea_seg_validate(const PeaSegDesc *d);

/* Host-only: bytes of the tables (a multiple of 8): a header of 8 words, 32 words per image and 10 words per (image, slot).  Strictly
 * increasing in capacity and in B; S plays no part.  0 for a descriptor that does not validate; SIZE_MAX where the count does not
 * fit. */
size_t pea_seg_workspace_bytes(const PeaSegDesc *d);

/* Prepare `bytes` bytes at `workspace` (8-byte aligned, bytes >= 64 and a multiple of 8) once per allocation: all zero but for a
 * magic word.  Every pea_seg_scores / pea_seg_table leaves the block like that for the next call on the same stream, whatever its
 * descriptor; a block that was never prepared gives NaN in every column.  PEA_E_NULL / PEA_E_ALIGN / PEA_E_WORKSPACE (bytes < 64 or
 * not a multiple of 8). */
int pea_seg_workspace_init(void *workspace, size_t bytes, void *stream);

/* pred, gt int32 [B, S]; out f64 [B][PEA_SEG_COLS], every element written.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_seg_validate refuses
 *   PEA_E_NULL         pred, gt or out is NULL
 *   PEA_E_ALIGN        pred or gt not 4-byte, out or workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_seg_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 1024 pixels of an image, one per 256 slots)
 * Any element-aligned pointer and any S is served with the same bits: alignment to four elements only selects wide loads.  Every
 * probe sequence ends after `capacity` slots: a full table drops pairs (n_overflow), it never stalls a kernel. */
int pea_seg_scores(const PeaSegDesc *d, const int32_t *pred, const int32_t *gt, double *out, void *workspace, size_t workspace_bytes,
                   void *stream);

/* The non-empty (pred id, gt id, count) triples of image b (0 <= b < d->B) in no particular order: the first min(n, max_triples) of
 * them go to pred_ids / gt_ids int32 [max_triples] and counts int64 [max_triples], and n_out[0] (int64, DEVICE) = n, the number of
 * distinct pairs that found a slot; n_out[1] = the pixels dropped for want of a slot, n_out[2] = the negative labels.  Nothing comes
 * back to the host.  The workspace is the one of pea_seg_scores (only the part of one image is used).
 * Returns in this order: PEA_E_NULL (d); what pea_seg_validate refuses; PEA_E_DESC (b outside 0 .. B - 1, max_triples < 1);
 * PEA_E_NULL (pred, gt, pred_ids, gt_ids, counts, n_out); PEA_E_ALIGN (pred, gt, pred_ids, gt_ids not 4-byte; counts, n_out or
 * workspace not 8-byte aligned); PEA_E_WORKSPACE; PEA_E_UNSUPPORTED (the grid). */
int pea_seg_table(const PeaSegDesc *d, const int32_t *pred, const int32_t *gt, int32_t b, int32_t *pred_ids, int32_t *gt_ids,
                  int64_t *counts, int64_t *n_out, int64_t max_triples, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_SEGSCORE_H_ */
