/*
 * pea_multi.h -- C ABI of the batched self losses (new entry points of libpea_hip.so; include/pea.h is unchanged and
 * PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE pointer owned by the caller, nothing is
 * allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and every refusal
 * returns before anything is launched.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity): the four deep-supervision self losses every training
 * step evaluates beside the full-resolution pair,
 *
 *   scripts_cvppp/main.py:284-287, scripts_bbbc039v1/main.py:279-282   embedding_loss on emd1..emd4 with offsets[:8], [:6], [:4], [:2]
 *   scripts_cvppp/inference.py:185-188                                  the same calls in the validation loop
 *   scripts_ac3ac4/main.py:227-230                                      four embedding_loss_norm1 calls
 *
 * n calls of pea_affinity_fwd (each followed by its loss finish) and n calls of pea_affinity_bwd become THREE launches: one forward
 * over every tile of every entry, one loss finish with a workgroup per entry, one backward.  The images are small (578 tiles of 256
 * pixels at 272^2 down to 8 at 34^2, B = 2): one after the other they cost their launch latencies.
 *
 * Per entry the semantics are exactly those of pea_affinity_fwd / pea_affinity_bwd for a self loss (e_other == NULL): `affs` is
 * written with the descriptor's activation bits, g_out = lambda_i * 2 w m (a m - t m) / N_i (0 where the neighbour is cropped
 * away), loss_out = { loss, L_0 .. L_{K-1} } through the integer accumulators of the state block (exact, bit-reproducible), de in
 * gather form without atomics.  The entries of a table may differ in every field of their descriptors.
 *
 * The fused set.  pea_multi_supported(descs, n) == 1 exactly when
 *   - 1 <= n <= PEA_MULTI_MAX_N and every descriptor passes pea_desc_validate (so |offset| < the dimension it steps along),
 *   - dtype is PEA_F32, PEA_F16 or PEA_BF16 and THE SAME for all n entries (a table of f32 and 16-bit entries, or of f16 and bf16
 *     ones, is outside the set: the launch is instantiated per storage type), D is 16 or 32, K <= PEA_MULTI_MAX_K,
 *   - the border is PEA_BORDER_CIRCULAR or PEA_BORDER_CROP_ZERO, PEA_FLAG_LOSS_ACT is not set,
 *   - S * max(D, K) per batch item (S = Z * Y * X) fits int32, as for the kernels of pea.h,
 *   - every offset component fits int16 (the table of the launch stores them so; no image of a deep-supervision scale is 32768 wide).
 * For any other table the two calls return PEA_E_UNSUPPORTED and the caller makes the n single calls.
 *
 * 16-bit storage (what the embedding heads emit under autocast: include/pea_head16.h).  e is read and de is written in the
 * descriptor's dtype, one element per lane: e and de want the alignment of ONE element (2 bytes) and nothing of S, as pea.h
 * states for every entry point.  Everything between the load and the store is the f32 arithmetic of the f32 table, in the same
 * order: affs, g_out and loss_out carry the bits the f32 call gives on the upcast embedding, and de is that call's de rounded
 * once to nearest even (NaN stays NaN).  target, weight, mask, affs, g_out, loss_out, dloss and the loss states stay f32.
 */
#ifndef PEA_MULTI_H_
#define PEA_MULTI_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_MULTI_MAX_N 4  /* the reference has four deep-supervision heads */
#define PEA_MULTI_MAX_K 12 /* offsets[:8] in 2D, norm1 = 3 / norm5 = 12 in 3D */

typedef struct PeaMultiFwd { /* one self loss: the arguments of pea_affinity_fwd for it */
  const PeaDesc *desc;
  const void *e;        /* [B, D, Z, Y, X] in desc->dtype (f32 / f16 / bf16) */
  const float *target;  /* [B, K, Z, Y, X], batch stride desc->target_bstride */
  const float *weight;  /* likewise, desc->weight_bstride */
  const uint8_t *mask;  /* NULL, u8, or f32 with PEA_FLAG_MASK_F32 (passed as for pea_affinity_fwd); desc->mask_bstride */
  float *affs;          /* [B, K, Z, Y, X], nullable: the training loop throws the small maps away */
  float *g_out;         /* [B, K, Z, Y, X], required */
  float *loss_out;      /* [1 + K] */
} PeaMultiFwd;

typedef struct PeaMultiBwd { /* the arguments of pea_affinity_bwd for it */
  const PeaDesc *desc;
  const void *e;       /* [B, D, Z, Y, X] in desc->dtype (f32 / f16 / bf16) */
  const float *g;      /* [B, K, Z, Y, X]: what the forward wrote to g_out, or any upstream gradient d criterion / d affs */
  const float *dloss;  /* device scalar or NULL = 1 */
  void *de;            /* [B, D, Z, Y, X] in desc->dtype, like e */
} PeaMultiBwd;

/* host-only: 1 when the table is in the fused set (above), else 0 (also for a NULL or invalid descriptor).  No GPU needed. */
int pea_multi_supported(const PeaDesc *const *descs, int n);

/* The forward of n self losses.  `entries` is a HOST array, read during the call only.  `workspace` holds n loss states back to
 * back, pea_workspace_bytes(desc) each (workspace_bytes >= n times that), prepared by pea_workspace_init -- what
 * pea_affinity_fwd_bwd_labels_dual does with two; entry i adds into state i, and every state is left zero for the next call (of
 * any entry point of pea.h, on the same stream).
 * Returns n < 1 or n > PEA_MULTI_MAX_N: PEA_E_DESC; then per entry, in table order, what pea_affinity_fwd returns for it
 * (PEA_E_NULL: entries, desc, e, target, weight, g_out or loss_out missing; the descriptor's own code; PEA_E_ALIGN);
 * PEA_E_WORKSPACE; PEA_E_UNSUPPORTED where pea_multi_supported is 0.
 * Two entries whose output buffers (affs, g_out, loss_out; de below) overlap are the CALLER'S error: one launch writes them all
 * and nothing orders the writers. */
int pea_affinity_fwd_multi(const PeaMultiFwd *entries, int n, void *workspace, size_t workspace_bytes, void *stream);

/* The backward of the same n self losses in one launch: de_j = dloss_j * sum_i g_i d a_i / d e_j.  Return codes as above
 * (PEA_E_NULL: entries, desc, e, g or de missing). */
int pea_affinity_bwd_multi(const PeaMultiBwd *entries, int n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_MULTI_H_ */
