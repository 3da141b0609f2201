/*
 * pea_metrics.h -- C ABI of the validation pixel metrics on the affinity map: MSE, BCE and the F1 counts in one data launch (new entry
 * points of libpea_hip.so; include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is
 * a DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL =
 * the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity): what the drivers' validation loops do with the map,
 *
 *   scripts_cvppp/main.py:395-399 (the same lines in scripts_bbbc039v1/main.py)     2D: pred = F.relu(pred),
 *       valid_mse(pred * affs_mask, target * affs_mask), valid_bce(torch.clamp(pred, 0, 1) * affs_mask, target * affs_mask)
 *   scripts_cvppp/loss/loss.py:126-140                                               MSELoss / BCELoss = nn.MSELoss() / nn.BCELoss()
 *   scripts_ac3ac4/data/provider_valid.py:337-349                                    get_results: divide by the weight map, crop
 *   scripts_ac3ac4/main.py:304-351, scripts_ac3ac4/inference.py:253-269              3D: out_affs[:3], then in numpy on the host
 *       np.sum(np.square(out - gt)) / np.size(gt), np.clip(out, 1e-6, 0.999999), the BCE sum, the threshold at 0.5 and sklearn's
 *       f1_score(1 - gt, 1 - out)
 *
 * There: about ten elementwise torch launches and two reductions per 2D validation image, a copy of the stitched volume to the host
 * and five numpy passes per 3D validation.  Here: ONE streaming launch that reads every element once, plus one small finish launch;
 * the sums go through the integer loss accumulators of the training forward (pea_workspace_init, pea.h), so every number is
 * bit-reproducible and nothing waits for the host.
 *
 * Semantics.  The sums run over every evaluated element (b, c < C, p in the region); x = pred[b, c, origin + p]:
 *
 *   v  = x ;  PEA_MET_DIVIDE: v = x / weight_map[origin + p]  (IEEE division, the bits of pea_stitch_finalize)
 *             PEA_MET_RELU:   v = v < 0 ? 0 : v               (NaN kept, the bits of pea_fill_border_relu)
 *   m  = mask[b, c, p] (1 where mask == NULL) ;  a = v * m ;  t' = target[b, c, p] * m
 *   u  = (v < clip_lo ? clip_lo : v > clip_hi ? clip_hi : v) * m          (a NaN v stays NaN)
 *   mse term = (a - t')^2
 *   bce term = -( t' * max(log(u), -100) + (1 - t') * max(log(1 - u), -100) )     (nn.BCELoss; the floor is inert for the numpy clip)
 *   ground-truth boundary <=> t' < 1   (1 - gt.astype(uint8) for gt in [0, 1]) ;  predicted boundary <=> u <= 0.5  (false for NaN)
 *   tp, fp, fn count the elements that are (boundary, predicted), (not boundary, predicted), (boundary, not predicted)
 *
 * Every step up to the terms is f32, each rounded on its own (no fused multiply-add), the logarithm is the accurate logf; a
 * workgroup sums its terms in f32 in a fixed order and adds the partial into the state of its quantity.  The counts are exact.
 *
 *   out [1 + C][PEA_METRICS_COLS] f64:  row 1 + c = { sum_c / N, sum_c / N, tp_c, fp_c, fn_c },  N = B * Z * Y * X
 *                                       row 0     = { (sum over c of sum_c) / (C * N) twice -- summed in f64 in channel order --,
 *                                                     the total counts }
 *
 * F1 = 2 tp / (2 tp + fp + fn) is left to the caller (0 where the denominator is 0: sklearn's zero_division default).
 * Non-finite inputs follow the accumulators' rule (pea.h): a NaN or +-inf term makes mse / bce of that channel and of row 0 NaN /
 * +-inf; every other channel is bit-identical to the finite run.  A state block that was never initialised gives NaN in every column.
 *
 * PEA_MET_STORE writes v back to EVERY element of pred -- all CP channels, the whole [PZ, PY, PX] volume, not only the region --,
 * each element read and written by the same lane: with DIVIDE the bits of pea_stitch_finalize, with RELU alone those of
 * pea_fill_border_relu(shift 0, relu 1).  Without it nothing but `out` and the workspace is written.
 */
#ifndef PEA_METRICS_H_
#define PEA_METRICS_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_METRICS_COLS 5   /* mse, bce, tp, fp, fn */
#define PEA_MET_RELU 1u      /* v = max(v, 0), NaN kept                       (F.relu(pred), main.py:395) */
#define PEA_MET_DIVIDE 2u    /* v = pred / weight_map  (IEEE division)        (provider_valid.py:339)     */
#define PEA_MET_STORE 4u     /* write v back into pred, ALL CP channels, whole pred volume */
#define PEA_MET_MASK_F32 8u  /* mask holds f32, else u8 */

typedef struct PeaMetricsDesc {
  int32_t B, C, CP;       /* batch; channels evaluated = the first C of pred's CP channels; 1 <= C <= CP, C <= PEA_MAX_K */
  int32_t dims[3];        /* Z, Y, X of the evaluated region = of target / mask (2D: Z = 1) */
  int32_t pred_dims[3];   /* PZ, PY, PX of pred (and of weight_map) */
  int32_t origin[3];      /* the region starts here inside pred's volume (valid_padding); origin + dims <= pred_dims */
  uint32_t flags;         /* PEA_MET_* */
  float clip_lo, clip_hi; /* BCE clip: (0, 1) = torch.clamp of main.py:397; (1e-6f, 0.999999f) = np.clip of main.py:345 */
} PeaMetricsDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: any size < 1; C > CP or C > PEA_MAX_K; a
 * negative origin or a region that leaves pred_dims; unknown flag bits; STORE with neither RELU nor DIVIDE; DIVIDE with B != 1;
 * clip_lo > clip_hi, or either clip bound NaN. */
int pea_metrics_validate(const PeaMetricsDesc *d);

/* Host-only: the workspace of pea_affs_metrics, five loss states (mse, bce, tp, fp, fn) back to back = 5 * pea_workspace_bytes().
 * Prepare it once with pea_workspace_init; the finish puts every state back to zero, so the block serves any later pea_* call on
 * the stream (each takes the states it needs from the front). */
size_t pea_metrics_workspace_bytes(void);

/* pred [B, CP, PZ, PY, PX] f32 (written only with STORE); weight_map [PZ, PY, PX] f32, required with DIVIDE and ignored otherwise;
 * target [B, C, Z, Y, X] f32 dense; mask like target, u8 or f32 (PEA_MET_MASK_F32), NULL = all ones; out f64 [1 + C][5].
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_metrics_validate refuses
 *   PEA_E_NULL         pred, target or out is NULL, or weight_map is NULL with DIVIDE
 *   PEA_E_ALIGN        pred, weight_map, target or an f32 mask not 4-byte aligned; out or workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_metrics_workspace_bytes()
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups (one per 4096 elements of a channel)
 * Any element-aligned pointer is served with the same bits (the alignment contract of pea.h): 16-byte alignment only selects
 * dwordx4 loads and stores. */
int pea_affs_metrics(const PeaMetricsDesc *d, float *pred, const float *weight_map, const float *target, const void *mask,
                     double *out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_METRICS_H_ */
