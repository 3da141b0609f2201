// pea_k_head16.hip -- entry points of the embedding head on 16-bit features (include/pea_head16.h): validation and the choice of
// the storage type.  The kernels (pea_head.h) live in pea_k_head16_f16.hip / pea_k_head16_bf16.hip.
// One translation unit of libpea_hip.so (pea_host.h).
#include "pea_head.h"

#include "../../include/pea_head16.h"

using namespace pea;

static bool dtype_known(int t) { return t == PEA_F32 || t == PEA_F16 || t == PEA_BF16; }

extern "C" {

int pea_head_supported_t(int C, int D, int x_dtype, int e_dtype) {
  if (x_dtype != PEA_F16 && x_dtype != PEA_BF16) return 0;      // f32 features: pea_head_fwd / pea_head_bwd
  if (e_dtype != x_dtype && e_dtype != PEA_F32) return 0;       // mixed f16 / bf16
  return head_supported(C, D) ? 1 : 0;
}

int pea_head_fwd_t(int B, int C, int D, size_t S, const void* x, int x_dtype, const float* W, const float* bias, void* e, int e_dtype,
                   void* stream) {
  if (B < 1 || C < 1 || D < 1 || S < 1 || !dtype_known(x_dtype) || !dtype_known(e_dtype)) return PEA_E_DESC;
  if (!x || !W || !e) return PEA_E_NULL;
  if (misaligned(x, dtype_bytes(x_dtype)) || misaligned(W, 4) || misaligned(bias, 4) || misaligned(e, dtype_bytes(e_dtype)))
    return PEA_E_ALIGN;
  if (!pea_head_supported_t(C, D, x_dtype, e_dtype)) return PEA_E_UNSUPPORTED;
  const bool e_f32 = e_dtype == PEA_F32;
  return (x_dtype == PEA_F16 ? head16_fwd_f16 : head16_fwd_bf16)(B, C, D, S, x, W, bias, e, e_f32, (hipStream_t)stream);
}

int pea_head_bwd_t(int B, int C, int D, size_t S, const void* x, int x_dtype, const float* W, const void* de, int e_dtype, void* dx,
                   float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || C < 1 || D < 1 || S < 1 || !dtype_known(x_dtype) || !dtype_known(e_dtype)) return PEA_E_DESC;
  if (!x || !W || !de || !dW) return PEA_E_NULL;
  if (misaligned(x, dtype_bytes(x_dtype)) || misaligned(W, 4) || misaligned(de, dtype_bytes(e_dtype)) ||
      misaligned(dx, dtype_bytes(x_dtype)) || misaligned(dW, 4) || misaligned(db, 4) || misaligned(workspace, 4))
    return PEA_E_ALIGN;
  if (!pea_head_supported_t(C, D, x_dtype, e_dtype)) return PEA_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < pea_head_workspace_bytes(C, D)) return PEA_E_WORKSPACE;
  const bool e_f32 = e_dtype == PEA_F32;
  return (x_dtype == PEA_F16 ? head16_bwd_f16 : head16_bwd_bf16)(B, C, D, S, x, W, de, e_f32, dx, dW, db, (float*)workspace,
                                                                 (hipStream_t)stream);
}

}  // extern "C"
