// pea_k_head16_f16.hip -- the kernels of the embedding head (pea_head.h) for f16 features.
// One translation unit of libpea_hip.so per 16-bit type: the two compile side by side.
#include "pea_head.h"

namespace pea {

int head16_fwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const float* bias, void* e, bool e_f32, hipStream_t s) {
  return head16_fwd<__half>(B, C, D, S, x, W, bias, e, e_f32, s);
}

int head16_bwd_f16(int B, int C, int D, size_t S, const void* x, const float* W, const void* de, bool e_f32, void* dx, float* dW,
                   float* db, float* partials, hipStream_t s) {
  return head_bwd<__half>(B, C, D, S, x, W, de, e_f32, dx, dW, db, partials, s);
}

}  // namespace pea
