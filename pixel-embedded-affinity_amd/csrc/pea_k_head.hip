// pea_k_head.hip -- entry points of the embedding head on f32 features (pea_head.h: the 1x1 convolution in front of the path and its
// backward).  One translation unit of libpea_hip.so (pea_host.h).
#include "pea_host.h"
#include "pea_head.h"

using namespace pea;

extern "C" {

size_t pea_head_workspace_bytes(int C, int D) {
  if (C < 1 || D < 1) return 0;
  return (size_t)kHeadMaxWg * ((size_t)D * C + D) * sizeof(float);
}

int pea_head_fwd(int B, int C, int D, size_t S, const float* x, const float* W, const float* bias, float* e, void* stream) {
  if (B < 1 || C < 1 || D < 1 || S < 1) return PEA_E_DESC;
  if (!x || !W || !e) return PEA_E_NULL;
  if (misaligned(x, 4) || misaligned(W, 4) || misaligned(bias, 4) || misaligned(e, 4)) return PEA_E_ALIGN;
  if (!head_supported(C, D)) return PEA_E_UNSUPPORTED;
  size_t chunks;
  if (!head_chunks(B, S, 1, &chunks)) return PEA_E_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(chunks * B)), blk(kHeadBlock);
#define PEA_HEAD_F(c, d) \
  if (C == c && D == d) hipLaunchKernelGGL((k_head_fwd<c, d>), grid, blk, 0, s, x, W, bias, e, (long long)S, (int)chunks);
  PEA_HEAD_CASES(PEA_HEAD_F)
#undef PEA_HEAD_F
  return hip_rc();
}

int pea_head_bwd(int B, int C, int D, size_t S, const float* x, const float* W, const float* de, float* dx, float* dW, float* db,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || C < 1 || D < 1 || S < 1) return PEA_E_DESC;
  if (!x || !W || !de || !dW) return PEA_E_NULL;
  if (misaligned(x, 4) || misaligned(W, 4) || misaligned(de, 4) || misaligned(dx, 4) || misaligned(dW, 4) || misaligned(db, 4) ||
      misaligned(workspace, 4))
    return PEA_E_ALIGN;
  if (!head_supported(C, D)) return PEA_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < pea_head_workspace_bytes(C, D)) return PEA_E_WORKSPACE;
  return head_bwd<float>(B, C, D, S, x, W, de, true, dx, dW, db, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
