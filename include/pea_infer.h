/*
 * pea_infer.h -- C ABI of the fused 3D window inference (new entry points of libpea_hip.so; include/pea.h is unchanged and
 * PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE pointer owned by the caller, nothing is
 * allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream).
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity), per predicted window of the 3D inference loop:
 *
 *   pea_affinity_infer_stitch <- scripts_ac3ac4/inference.py:152-158        embedding_loss_norm1 / _norm5 (the map only)
 *                                scripts_ac3ac4/loss/loss_embedding_mse.py:54-67, 212-234  inf_embedding_loss_norm1 / _norm5
 *                                scripts_ac3ac4/inference.py:160-164        border fill of channels 0..2, F.relu
 *                                scripts_ac3ac4/inference.py:166            valid_provider.add_vol(pred.cpu().numpy())
 *                                scripts_ac3ac4/data/provider_valid.py:320-331  add_vol: out_affs += pred * weight, weight_map += weight
 *
 * i.e. pea_affinity_infer + pea_fill_border_relu + pea_stitch_add of pea.h in ONE launch: the [K, oz, oy, ox] map of the window is
 * never written (4D + 4 + 8K + 8 bytes per voxel instead of 4D + 4K, 8K and 12K + 12).
 */
#ifndef PEA_INFER_H_
#define PEA_INFER_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host-only: 1 if pea_affinity_infer_stitch fuses this descriptor / fill_shift, else 0 (also 0 for an invalid descriptor).
 * Fused: PEA_BORDER_CROP_ZERO, D = 16 or 32, any storage dtype, any K and offsets, fill_shift 0 or 1, no PEA_FLAG_LOSS_ACT. */
int pea_infer_stitch_supported(const PeaDesc *desc, int fill_shift);

/* One window e [1, D, oz, oy, ox] (desc->dims = (oz, oy, ox), desc->B == 1, desc->K = channels of out_affs; no second operand)
 * placed at (z0, y0, x0) of the volume out_affs [K, Z, Y, X] / weight_map [Z, Y, X], blend weights weight_vol [oz, oy, ox] (f32).
 * For every window voxel p and channel i < K:
 *   q = p, and where fill_shift > 0, i < 3 and p[axis i] < fill_shift: q[axis i] += fill_shift     (inference.py:160-163, window
 *                                                                                                    coordinates, at the source)
 *   a = < ehat(q), ehat(q + o_i) >,  0 where q + o_i leaves the window                               (pea_affinity_infer)
 *   u = act(a)  by desc->flags as pea_affinity_infer applies them; PEA_FLAG_RELU_AFFS = F.relu       (inference.py:164)
 *   out_affs[i, p + (z0, y0, x0)] += u * weight_vol[p];   weight_map[p + (z0, y0, x0)] += weight_vol[p]   (provider_valid.py:326-331)
 * Product and sum are rounded separately (no FMA), as pea_stitch_add does.  One lane owns a voxel's stores: plain stores, no
 * atomics, deterministic.  Overlapping windows must be issued as separate calls on one stream (they read-modify-write the same
 * voxels); pea_stitch_finalize divides as before.
 * Returns, before anything is launched: PEA_E_DESC for an invalid descriptor, B != 1, a window that does not lie inside the
 * volume, fill_shift < 0, or fill_shift > 0 with 2 * fill_shift above a window dimension that a filled channel uses (K >= 3: any
 * dimension, the rule of pea_fill_border_relu); PEA_E_NULL / PEA_E_ALIGN as elsewhere; PEA_E_UNSUPPORTED wherever
 * pea_infer_stitch_supported is 0 (the caller then makes the three calls of pea.h). */
int pea_affinity_infer_stitch(const PeaDesc *desc, const void *e, int fill_shift, const float *weight_vol,
                              float *out_affs, float *weight_map, int Z, int Y, int X, int z0, int y0, int x0,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_INFER_H_ */
