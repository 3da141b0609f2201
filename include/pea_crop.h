/*
 * pea_crop.h -- C ABI of the reference's 3D border rule on an ACTIVATED affinity map (a new entry point of libpea_hip.so;
 * include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE pointer owned
 * by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream),
 * and every refusal returns before anything is launched.
 *
 * What it is for.  Under PEA_BORDER_CROP_ZERO a pair whose neighbour p + o_i leaves the volume does not exist: the kernels give it
 * the raw value a = 0 and store act(0) in `affs` -- 0.5 under PEA_FLAG_HALF_SHIFT (tests/test_gpu_act_loss.py pins that).  The
 * reference's 3D modules on the activated map (weih527/Pixel-Embedded-Affinity, scripts_ac3ac4/loss/embedding2affs_3d.py,
 * embedding2affs_3d_l2.py, loss_embedding_mse.py:70-140) build their map as torch.zeros_like(target) and write the cropped slices
 * into it, or zero the first `shift` slices after the activation (embedding_single_offset :89-96): there a non-existent pair holds
 * 0, whatever the activation.  This call restores that: it stores +0.0f at every affs[b, k, p] whose pair does not exist and
 * touches NO other element.  (Under a clamp-only activation act(0) = 0 already and the call is not needed.)
 *
 * One launch that reads nothing.  The set of non-existent pairs of offset k is the union, over the non-zero components of o_k,
 * of one slab: the |o_k[a]| slices at the low end of axis a (o_k[a] < 0) or at its high end (o_k[a] > 0).  The grid covers
 * those slabs only -- at most 3 K of them, listed in the kernel's arguments -- never the interior; where the slabs of a diagonal
 * offset overlap, an element is written twice with the same bits.
 */
#ifndef PEA_CROP_H_
#define PEA_CROP_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

/* affs: [B, K, Z, Y, X] f32, dense.  Of `desc` only B, K, dims, offsets and border are read (the rest is validated as everywhere).
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         desc is NULL
 *   (the code of pea_desc_validate(desc))
 *   PEA_E_DESC         desc->border is not PEA_BORDER_CROP_ZERO (under the other borders every pair exists)
 *   PEA_E_NULL         affs is NULL
 *   PEA_E_ALIGN        affs is not 4-byte aligned
 *   PEA_E_UNSUPPORTED  the slabs need more than 2^31 - 1 workgroups (one per 256 elements of a slab)
 * Any element-aligned pointer is served (the alignment contract of pea.h).  A stencil without a non-zero component launches nothing
 * and returns PEA_OK. */
int pea_affs_crop_zero(const PeaDesc *desc, float *affs, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_CROP_H_ */
