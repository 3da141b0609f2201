/*
 * pea_head16.h -- C ABI of the embedding head on 16-bit features (new entry points of libpea_hip.so; include/pea.h is unchanged and
 * PEA_ABI_VERSION stays 2).  Same conventions as pea.h: every data pointer is a DEVICE pointer owned by the caller, nothing is
 * allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and every refusal
 * returns before anything is launched.  Dtype codes are PEA_F32 / PEA_F16 / PEA_BF16 of pea.h.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity), as pea_head_fwd / pea_head_bwd of pea.h do for f32:
 *
 *   scripts_cvppp/model/unet2d_residual.py:67-74       OutConv = nn.Conv2d(C, D, 1) (outconv_emb :307, applied :346)
 *   scripts_bbbc039v1/model/unet2d_residual.py:67,235  the same class
 *   scripts_ac3ac4/model/basic.py:114-127              conv3dBlock([C], [D], [(1, 1, 1)]), the out_put* heads of
 *   scripts_ac3ac4/model/model_superhuman.py:437-441   (applied :486-490)
 *
 * when the feature map x is f16 or bf16 -- the backbone under torch.autocast, or 16-bit embedding storage for the f16 / bf16 loss
 * kernels (pea_affinity_fwd_ex / pea_affinity_bwd_ex2 with desc.dtype = PEA_F16 / PEA_BF16).  The head is bound by HBM traffic, and
 * 2-byte elements halve it: 2(C+D) bytes per pixel forward and 2(2C+D) backward against 4(C+D) / 4(2C+D).
 *
 *     e[b,d,p] = bias[d] + sum_c W[d,c] x[b,c,p]      x x_dtype [B,C,S] , W f32 [D,C] , bias f32 [D] or NULL , e e_dtype [B,D,S]
 *     dx[b,c,p] = sum_d W[d,c] de[b,d,p]              de e_dtype [B,D,S] , dx x_dtype [B,C,S] (nullable)
 *     dW[d,c] = sum_{b,p} de[b,d,p] x[b,c,p] ,  db[d] = sum_{b,p} de[b,d,p]          f32 [D,C] , f32 [D] (nullable)
 *
 * with S = H*W or Z*Y*X contiguous pixels per channel plane.  W and bias are the f32 MASTER parameters and are used unrounded;
 * every product and every sum is f32; a 16-bit e / dx is rounded ONCE, to nearest even, when it is stored.  dW and db are f32 sums
 * over pixels (16-bit values are exact in f32) through per-workgroup partials in `workspace` -- pea_head_workspace_bytes(C, D) of
 * pea.h, the same size as for the f32 head -- with a fixed-order final reduction: bit-reproducible from run to run, and the same
 * whether or not dx / db are requested.
 *
 * Supported: x_dtype PEA_F16 or PEA_BF16; e_dtype the SAME 16-bit type or PEA_F32 (four type pairs); (C, D) the pairs of the f32
 * head, (28|32|36|48|64|80|128|256, 16) and (32|64|128|256, 32).
 * Refused with PEA_E_UNSUPPORTED (pea_head_supported_t: 0):
 *   (PEA_F32, PEA_F32)            stays with pea_head_fwd / pea_head_bwd of pea.h
 *   (PEA_F32, 16-bit)             not built: an f32 feature map with a 16-bit embedding
 *   (PEA_F16, PEA_BF16) and back  mixed 16-bit types
 *   any other (C, D)
 *
 * Alignment: ELEMENT alignment only (the contract of pea.h) -- 2 bytes for a 16-bit tensor, 4 for W, bias, dW, db, workspace and
 * an f32 e / de.  Any element-aligned pointer and any S >= 1, odd included, is served; the kernels move two pixels per lane as one
 * dword where S is even and the tensors are 4-byte aligned (8 for an f32 e / de) and one element per lane otherwise, so only the
 * speed differs.
 */
#ifndef PEA_HEAD16_H_
#define PEA_HEAD16_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only (no GPU needed): 1 if the two calls below serve (C, D, x_dtype, e_dtype), else 0. */
int pea_head_supported_t(int C, int D, int x_dtype, int e_dtype);

/* Both calls return, before anything is launched and in this order:
 *   PEA_E_DESC         B, C, D or S < 1; a dtype code outside 0..2
 *   PEA_E_NULL         x, W or e (forward) / x, W, de or dW (backward) is NULL
 *   PEA_E_ALIGN        a pointer not aligned to its element size (above)
 *   PEA_E_UNSUPPORTED  pea_head_supported_t is 0
 *   PEA_E_WORKSPACE    (backward) workspace NULL or shorter than pea_head_workspace_bytes(C, D)
 * and PEA_E_UNSUPPORTED if the pixel chunks of the batch do not fit one grid (B * ceil(S / 256) > 2^31 - 1). */
int pea_head_fwd_t(int B, int C, int D, size_t S, const void *x, int x_dtype, const float *W, const float *bias, void *e,
                   int e_dtype, void *stream);
int pea_head_bwd_t(int B, int C, int D, size_t S, const void *x, int x_dtype, const float *W, const void *de, int e_dtype,
                   void *dx, float *dW, float *db, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_HEAD16_H_ */
