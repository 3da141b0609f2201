/*
 * pea_flip.h -- C ABI of the per-sample un-flip of the EMA embedding (a new entry point of libpea_hip.so; include/pea.h is unchanged
 * and PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE pointer owned by the caller, nothing is
 * allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and every refusal
 * returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity): the inverse of the EMA branch's random flips, taken
 * between the second backbone forward and the EMA cross loss of every training step (if_ema_flip: True in the shipped yamls),
 *
 *   scripts_cvppp/data/data_consistency.py:19-31, 34-45     simple_augment_reverse_torch, convert_consistency_flip (2D, three rules)
 *   scripts_bbbc039v1/data/data_consistency.py:34-46, 49-60 the same pair
 *   scripts_ac3ac4/utils/consistency_aug.py:58-77, 217-228  simple_augment_reverse_torch, convert_consistency_flip (3D, FOUR rules)
 *   scripts_cvppp/main.py:275, scripts_bbbc039v1/main.py:271, scripts_ac3ac4/main.py:214   the call sites
 *
 * There: a clone of the whole tensor, a copy of `rules` to the host (a synchronisation in the middle of the step), up to three
 * flip / permute views per sample and a torch.stack.  Here: ONE launch for the batch that reads every element once and writes it
 * once, with the rules read on the device -- so a step that contains it can be captured into a HIP graph and replayed with the
 * rules of the next batch.
 *
 * Semantics, per sample b and for every channel c (rules[b] read as nrules consecutive elements of `rules`):
 *
 *   nrules == 3, rules[b] = (rx, ry, rt):      z' = z                   (2D; on a volume the three rules apply to every z slice)
 *   nrules == 4, rules[b] = (rz, rx, ry, rt):  z' = rz ? Z-1-z : z      (the AC3/AC4 order: z-flip FIRST)
 *       y' = ry ? Y-1-y : y ;   x' = rx ? X-1-x : x
 *       dst[b,c,z,y,x] = rt ? src[b,c,z',x',y'] : src[b,c,z',y',x']
 *
 * A rule is SET when its value is nonzero (f32: compares unequal to 0, so -0 is clear and a NaN is set).  The reference casts with
 * astype(np.uint8) and its Filp_EMA draws 0 / 1, for which the two agree; what any other value (256, 0.5, -1 ..) should mean is
 * the caller's business.
 * The transpose needs Y == X, and the host cannot see the rules.  A sample whose rt is set while Y != X therefore gets its WHOLE
 * output [C, Z, Y, X] filled with NaN (f32 0x7fc00000, f16 0x7e00, bf16 0x7fc0) -- never a silently wrong number, as for the
 * uninitialised state block of pea.h; nothing outside that sample's output is touched and the other samples are served.
 * The result is a bit-exact copy: no arithmetic anywhere, NaN payloads, -0 and infinities are preserved; dst has the dtype of src.
 */
#ifndef PEA_FLIP_H_
#define PEA_FLIP_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element type of `rules` */
#define PEA_RULES_U8 0  /* also torch.bool */
#define PEA_RULES_I32 1
#define PEA_RULES_I64 2
#define PEA_RULES_F32 3

/* src, dst: [B, C, Z, Y, X] dense, dtype PEA_F32 / PEA_F16 / PEA_BF16 (2D: Z = 1); rules: DEVICE [B, nrules] dense, nrules 3 or 4.
 * Returns, before anything is launched and in this order:
 *   PEA_E_DESC         B, C, Z, Y or X < 1; unknown dtype or rules_dtype; nrules not 3 or 4
 *   PEA_E_NULL         src, dst or rules is NULL
 *   PEA_E_ALIGN        src / dst not aligned to the element size, or rules not aligned to ITS element size
 *   PEA_E_DESC         the byte ranges of src and dst overlap (a flip or transpose cannot be done in place)
 *   PEA_E_UNSUPPORTED  B * C * Z * ceil(Y / 64) * ceil(X / 64) tiles do not fit one grid (2^31 - 1)
 * Any element-aligned pointer is served (the alignment contract of pea.h).
 * `rules` is only read and must not overlap dst: that is the CALLER'S responsibility (it is not checked; the kernel reads a sample's
 * rules while other workgroups already write dst). */
int pea_consistency_unflip(int B, int C, int Z, int Y, int X, int dtype, const void *src, void *dst,
                           const void *rules, int rules_dtype, int nrules, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_FLIP_H_ */
