// pea_k_crop.hip -- the reference's 3D border rule on an activated affinity map (include/pea_crop.h): +0.0f at every affs[b, k, p]
// whose pair does not exist under PEA_BORDER_CROP_ZERO, nothing else touched.  One translation unit of libpea_hip.so; one kernel.
//
// The non-existent pairs of offset k are the union of one slab per non-zero component of o_k: |o_k[a]| slices at the low end of axis
// a (o < 0) or at its high end (o > 0).  The host lists the slabs (at most 3 K = 96) with the first workgroup of each in the kernel's
// arguments; the grid is one-dimensional over the slabs' workgroups, 256 consecutive slab elements each, and reads no memory: a
// workgroup finds its slab by a uniform walk over the list (scalar registers), a lane decodes its element of the slab -- (b, then the
// slab's own z, y, x extents, x fastest) -- and stores one dword.  A slab along z or y is whole rows of X, so a wave writes 256
// consecutive bytes; a slab along x writes |o| elements per row.  Every index is inside the tensor by construction: the slab's
// origin plus extent is at most the dimension (|o| < dim: pea_desc_validate), and elements past the slab's count are not stored.
#include "../../include/pea_crop.h"
#include "pea_dispatch.h"

using namespace pea;

namespace {

constexpr int kMaxSlabs = 3 * PEA_MAX_K;

struct CropSlab {
  int k, axis, lo, n;  // channel; axis of the slab (0 z, 1 y, 2 x); its first slice and its thickness along that axis
  unsigned blk0;       // first workgroup of the slab
};
struct CropArgs {
  int nslab;
  CropSlab s[kMaxSlabs];
};

__global__ __launch_bounds__(kBlock) void k_affs_crop_zero(float* __restrict__ affs, int B, int K, int Z, int Y, int X, const CropArgs A) {
  // the slab of this workgroup: the last one that starts at or before it (uniform)
  int si = 0;
  for (int i = 1; i < A.nslab; ++i)
    if (A.s[i].blk0 <= blockIdx.x) si = i;
  const int k = A.s[si].k, ax = A.s[si].axis, lo = A.s[si].lo, n = A.s[si].n;
  const uint64_t e0 = ax == 0 ? (uint64_t)n : (uint64_t)Z, e1 = ax == 1 ? (uint64_t)n : (uint64_t)Y, e2 = ax == 2 ? (uint64_t)n : (uint64_t)X;
  const uint64_t per = e0 * e1 * e2;
  const uint64_t i = (uint64_t)(blockIdx.x - A.s[si].blk0) * kBlock + threadIdx.x;
  if (i >= per * (uint64_t)B) return;
  const uint64_t b = i / per, r = i - b * per;
  const uint64_t z = r / (e1 * e2) + (ax == 0 ? (uint64_t)lo : 0), y = (r / e2) % e1 + (ax == 1 ? (uint64_t)lo : 0),
                 x = r % e2 + (ax == 2 ? (uint64_t)lo : 0);
  affs[(((b * (uint64_t)K + (uint64_t)k) * (uint64_t)Z + z) * (uint64_t)Y + y) * (uint64_t)X + x] = 0.f;
}

}  // namespace

extern "C" int pea_affs_crop_zero(const PeaDesc* desc, float* affs, void* stream) {
  if (!desc) return PEA_E_NULL;
  const int v = pea_desc_validate(desc);
  if (v != PEA_OK) return v;
  if (desc->border != PEA_BORDER_CROP_ZERO) return PEA_E_DESC;
  if (!affs) return PEA_E_NULL;
  if (misaligned(affs, 4)) return PEA_E_ALIGN;
  CropArgs A = {};
  uint64_t blocks = 0;
  for (int k = 0; k < desc->K; ++k)
    for (int a = 0; a < 3; ++a) {
      const int o = desc->offsets[k][a];
      if (o == 0) continue;
      const int n = o < 0 ? -o : o;  // < dims[a] (pea_desc_validate)
      uint64_t cnt = (uint64_t)desc->B * (uint64_t)n;
      for (int c = 0; c < 3; ++c)
        if (c != a) cnt *= (uint64_t)desc->dims[c];
      if (blocks > 0x7fffffffULL) return PEA_E_UNSUPPORTED;
      A.s[A.nslab] = {k, a, o < 0 ? 0 : desc->dims[a] - n, n, (unsigned)blocks};
      ++A.nslab;
      blocks += (cnt + kBlock - 1) / kBlock;  // cnt <= B * S < 2^62
    }
  if (blocks > 0x7fffffffULL) return PEA_E_UNSUPPORTED;
  if (A.nslab == 0) return PEA_OK;
  hipLaunchKernelGGL(k_affs_crop_zero, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, affs, desc->B, desc->K, desc->dims[0],
                     desc->dims[1], desc->dims[2], A);
  return hip_rc();
}
