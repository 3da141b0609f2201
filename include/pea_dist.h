/*
 * pea_dist.h -- C ABI of the DISTANCE-form affinities of a raw, un-normalised embedding, forward and vjp (new entry points of
 * libpea_hip.so; include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE
 * pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the
 * default stream), and every refusal returns before anything is launched.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity), the transform that turns the embedding of a model trained
 * with the discriminative loss (pea_disc.h) into an affinity map:
 *
 *   scripts_{cvppp,bbbc039v1,ac3ac4}/utils/emb2affs.py:63-75   embeddings_to_affinities(embeddings, offsets, delta): torch, batched,
 *                                                              differentiable; border by shift_tensor :6-56 (replication padding)
 *   scripts_ac3ac4/utils/embeddings_ours.py:47-98              embeddings_to_affinities(embeddings, offsets, delta_v, delta_d, invert):
 *                                                              numpy, one volume, scipy.ndimage.shift(order=0), a dead zone
 *   scripts_ac3ac4/utils/embeddings.py:78-114                  the same without the dead zone
 *
 * Semantics.  e [B, D, Z, Y, X] (2D: Z = 1), affs [B, K, Z, Y, X] f32.  For voxel p and offset o_i the neighbour is q = p + o_i:
 *
 *   d   = || e(p) - e(q) ||_2
 *   h   = d <= delta_v ? 0 : d                            (the dead zone of embeddings_ours.py; delta_v = 0: none)
 *   u   = (2 delta_d - h) / (2 delta_d)
 *   a_i = max(u, 0)^2,   with PEA_DIST_INVERT  1 - a_i    (what the mutex watershed is handed)
 *
 * Border.  PEA_BORDER_REPLICATE: the index of q is clamped into the volume (emb2affs.py).  PEA_DIST_BORDER_ZERO_VECTOR: outside the
 * volume e(q) is the zero vector, so a = f(||e(p)||) (embeddings_ours.py) -- NOT the "a = 0" of PEA_BORDER_CROP_ZERO.  Under either
 * rule every pair is defined, also for an offset that reaches beyond an extent; offsets of any size are valid.  Circular borders
 * have no reference and are refused.
 *
 * The derivative is torch's for the emb2affs.py form: da / dd = -u / delta_d where u > 0 and d > delta_v, else 0 (inside the dead zone
 * the map is constant); the direction is (e(p) - e(q)) / d, and 0 where d == 0 (the backward of torch.norm) -- under REPLICATE every
 * pair that the clamp folds onto p itself is such a pair.  PEA_DIST_INVERT flips the sign.  The vjp
 *
 *   de(p) = dscale * sum_i [ c_i(p) (e(p) - e(p + o_i))  +  sum_{p' : p' + o_i = p} c_i(p') (e(p) - e(p')) ],
 *   c_i(p) = g_i(p) * (da / dd) / d
 *
 * takes an ARBITRARY upstream g (the vjp contract of pea.h: the caller need not have run the forward; d is recomputed).
 *
 * Arithmetic (f32; 16-bit embeddings are widened first, which is exact): the sum of squares of e(p) - e(q) by fused multiply-add in
 * ascending channel order, sqrtf, IEEE division; de is computed in f32 and rounded once to the storage type (nearest even, NaN kept).
 * One lane owns each stored element and nothing is accumulated across lanes: two runs, an eager and a captured run, and calls on
 * differently aligned pointers give the same bits.  No workspace, no atomics.
 *
 * Non-finite values (the policy of pea.h: a NaN affinity is the sign a caller gets).  max(u, 0) is a select that keeps NaN.  A sum of
 * squares that is not finite -- a NaN or +-inf channel in e(p) or e(q), or an overflow -- makes a_i NaN (plain IEEE arithmetic would
 * turn d = inf into a = 0 and hide it): a non-finite embedding vector makes exactly the affinities of the pairs that touch it NaN, and
 * every other element has the bits of the finite run.
 */
#ifndef PEA_DIST_H_
#define PEA_DIST_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_DIST_MAX_D 64
#define PEA_DIST_BORDER_ZERO_VECTOR 3 /* a value of PeaDistDesc.border beside PEA_BORDER_REPLICATE: e(q) = 0 outside the volume */
#define PEA_DIST_INVERT 1u            /* affs = 1 - a; the vjp changes sign */

typedef struct PeaDistDesc {
  int32_t B, D;    /* D in 1..PEA_DIST_MAX_D */
  int32_t dims[3]; /* Z, Y, X; 2D: Z = 1 */
  int32_t K;       /* 1..PEA_MAX_K */
  int32_t offsets[PEA_MAX_K][3];
  int32_t dtype;  /* PEA_F32 / PEA_F16 / PEA_BF16: e and de */
  int32_t border; /* PEA_BORDER_REPLICATE or PEA_DIST_BORDER_ZERO_VECTOR */
  uint32_t flags; /* PEA_DIST_INVERT */
  float delta_v, delta_d;
} PeaDistDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (desc == NULL), or PEA_E_DESC for: B, D, K or a dimension < 1; D >
 * PEA_DIST_MAX_D; K > PEA_MAX_K; an unknown dtype; a border other than the two above (PEA_BORDER_CIRCULAR and PEA_BORDER_CROP_ZERO
 * included); unknown flag bits; delta_d not finite or <= 0; delta_v negative or not finite. */
int pea_dist_validate(const PeaDistDesc *desc);

/* e [B, D, Z, Y, X] of dtype, dense -> affs [B, K, Z, Y, X] f32, dense; every element of affs is written.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         desc is NULL
 *   PEA_E_DESC         what pea_dist_validate refuses
 *   PEA_E_NULL         e or affs is NULL
 *   PEA_E_ALIGN        e not aligned to its element, affs not 4-byte aligned
 *   PEA_E_UNSUPPORTED  Z Y X > 2^31 - 1, or more than 2^31 - 8 workgroups (one per 256 voxels of an image)
 * Any element-aligned pointer is served with the same bits (the alignment contract of pea.h). */
int pea_dist_affinity(const PeaDistDesc *desc, const void *e, float *affs, void *stream);

/* de [B, D, Z, Y, X] of dtype = dscale[0] * sum(g * d affs / d e) for g [B, K, Z, Y, X] f32; dscale is a DEVICE f32 scalar, NULL = 1.
 * Every element of de is written.
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         desc is NULL
 *   PEA_E_DESC         what pea_dist_validate refuses
 *   PEA_E_NULL         e, g or de is NULL
 *   PEA_E_ALIGN        e or de not aligned to its element, g or dscale not 4-byte aligned
 *   PEA_E_UNSUPPORTED  as above */
int pea_dist_affinity_vjp(const PeaDistDesc *desc, const void *e, const float *g, const float *dscale, void *de, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_DIST_H_ */
