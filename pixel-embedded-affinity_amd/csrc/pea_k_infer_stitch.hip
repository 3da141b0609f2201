// pea_k_infer_stitch.hip -- the 3D inference window in ONE launch (include/pea_infer.h): embedding -> affinities -> border fill ->
// activation -> blend into the stitched volume.  Replaces, per window, pea_affinity_infer + pea_fill_border_relu + pea_stitch_add
// (scripts_ac3ac4/inference.py:152-166, scripts_ac3ac4/data/provider_valid.py:320-331): the [K, oz, oy, ox] map of the window is never
// written and read back twice.
//
// Gather form (the style of k_fwd_direct, pea_direct.h): one lane owns FOUR x-adjacent voxels, keeps their D channels in registers and
// reads every neighbour vector from global memory -- 16-byte (f32) / 8-byte (16-bit) loads where the window's rows are aligned and the
// offset keeps the quad aligned (dx % 4 == 0: the z and y offsets of norm1 / norm5), single elements otherwise (x offsets, ox % 4 != 0,
// an unaligned tensor); the window (29 MB at 16 x 18 x 160 x 160) is served by L2 / the Infinity Cache.  The same arithmetic as the
// existing forwards: channels summed in order with fmaf, a = dot * (1 / max(|e(p)|, eps)) * (1 / max(|e(q)|, eps)).
// The border fill is evaluated at its SOURCE: channel i < 3 of a voxel whose coordinate along axis i is below fill_shift takes the
// affinity of the voxel fill_shift further along that axis (copy and relu commute); those few voxels (three faces of the window) take
// a per-voxel gather.  The blend rounds product and sum separately (no FMA), as k_stitch_add does; one lane owns a voxel's stores.
#include "../../include/pea_infer.h"
#include "pea_dispatch.h"

using namespace pea;

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct ISParams {
  int oz, oy, ox, K;        // the window
  int Z, Y, X, z0, y0, x0;  // the volume and the window's place in it
  int S;                    // oz * oy * ox
  int xq, quads;            // quads per window row = ceil(ox / 4); oz * oy * xq
  int tiles, tiles_per_xcd; // workgroups of kBlock quads; ceil(tiles / 8)
  int fill;                 // fill_shift
  int vin, vout;            // quads of e / weight_vol, of out_affs / weight_map are aligned: vector loads and stores
  unsigned act;             // activation bits of desc->flags
  float eps;
  int off[PEA_MAX_K][3];
};

// four consecutive elements base[i .. i + 3] as f32; VEC: one aligned load, else the elements j in [lo, hi) one by one (others 0)
template <bool VEC, typename T>
__device__ __forceinline__ void ld_quad(const T* __restrict__ base, long long i, int lo, int hi, float (&v)[4]) {
  if constexpr (VEC) {
    if constexpr (std::is_same<T, float>::value) {
      const f4 r = *(const f4*)(base + i);
      v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
      const uint2 r = *(const uint2*)(base + i);
      if constexpr (std::is_same<T, __half>::value) {
        v[0] = __half2float(__ushort_as_half((unsigned short)(r.x & 0xffffu)));
        v[1] = __half2float(__ushort_as_half((unsigned short)(r.x >> 16)));
        v[2] = __half2float(__ushort_as_half((unsigned short)(r.y & 0xffffu)));
        v[3] = __half2float(__ushort_as_half((unsigned short)(r.y >> 16)));
      } else {  // bf16: the upper half of an f32
        v[0] = __uint_as_float(r.x << 16);
        v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16);
        v[3] = __uint_as_float(r.y & 0xffff0000u);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (j >= lo && j < hi) ? ld(base, (size_t)(i + j)) : 0.f;
  }
}

// a_i at the single voxel (z, y, x): the border fill's source voxels (channels not unrolled: a rare path that must stay small)
template <typename T, int D>
__device__ __forceinline__ float affinity_at(const ISParams& P, const T* __restrict__ e, int i, int z, int y, int x) {
  const int zz = z + P.off[i][0], yy = y + P.off[i][1], xx = x + P.off[i][2];
  if ((unsigned)zz >= (unsigned)P.oz || (unsigned)yy >= (unsigned)P.oy || (unsigned)xx >= (unsigned)P.ox) return 0.f;
  const size_t S = (size_t)P.S, p = ((size_t)z * P.oy + y) * P.ox + x, q = ((size_t)zz * P.oy + yy) * P.ox + xx;
  float ss = 0.f, dot = 0.f, sq = 0.f;
#pragma unroll 4
  for (int c = 0; c < D; ++c) {
    const float u = ld(e, c * S + p), v = ld(e, c * S + q);
    ss = fmaf(u, u, ss);
    dot = fmaf(u, v, dot);
    sq = fmaf(v, v, sq);
  }
  return dot * inv_norm(ss, P.eps) * inv_norm(sq, P.eps);
}

// dot[j] = <own(j), e(q + j)>, sq[j] = |e(q + j)|^2 over the D channels for the quad at q
template <bool VEC, typename T, int D>
__device__ __forceinline__ void gather_quad(const T* __restrict__ e, long long S, long long q, int lo, int hi, const float (&ec)[D][4],
                                            float (&dot)[4], float (&sq)[4]) {
#pragma unroll
  for (int c = 0; c < D; ++c) {
    float v[4];
    ld_quad<VEC>(e, c * S + q, lo, hi, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dot[j] = fmaf(ec[c][j], v[j], dot[j]);
      sq[j] = fmaf(v[j], v[j], sq[j]);
    }
    if (c % 8 == 7) __builtin_amdgcn_sched_barrier(0);  // at most eight channels' loads in flight: registers
  }
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_infer_stitch(const ISParams P, const T* __restrict__ e, const float* __restrict__ wv,
                                                         float* __restrict__ out, float* __restrict__ wmap) {
  // XCD-aware walk as logical_tile(): each XCD takes a contiguous range of the window (a few z planes)
  const int tile = ((int)blockIdx.x % kXcd) * P.tiles_per_xcd + (int)blockIdx.x / kXcd;
  if (tile >= P.tiles) return;
  const int t = tile * kBlock + (int)threadIdx.x;
  if (t >= P.quads) return;
  const int row = t / P.xq;  // z * oy + y
  const int x4 = (t - row * P.xq) * 4;
  const int z = row / P.oy, y = row - z * P.oy;
  const int nv = min(4, P.ox - x4);  // live voxels of a ragged last quad
  const long long S = P.S, p = (long long)row * P.ox + x4;
  const bool vin = P.vin != 0, vout = P.vout != 0;

  float ec[D][4], w[4], inv_p[4];
  if (vin) {
#pragma unroll
    for (int c = 0; c < D; ++c) ld_quad<true>(e, c * S + p, 0, 4, ec[c]);
    ld_quad<true>(wv, p, 0, 4, w);
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) ld_quad<false>(e, c * S + p, 0, nv, ec[c]);
    ld_quad<false>(wv, p, 0, nv, w);
  }
  {
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) ss[j] = fmaf(ec[c][j], ec[c][j], ss[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) inv_p[j] = inv_norm(ss[j], P.eps);
  }

  const size_t SV = (size_t)P.Z * P.Y * P.X;
  const size_t o = ((size_t)(P.z0 + z) * P.Y + (P.y0 + y)) * P.X + (P.x0 + x4);

  for (int i = 0; i < P.K; ++i) {
    const int dz = P.off[i][0], dy = P.off[i][1], dx = P.off[i][2];
    const int zz = z + dz, yy = y + dy;
    // voxels j of the quad whose neighbour lies inside the window row: 0 <= x4 + j + dx < ox
    const int lo = max(0, -(x4 + dx)), hi = min(nv, P.ox - x4 - dx);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)zz < (unsigned)P.oz && (unsigned)yy < (unsigned)P.oy && hi > lo) {
      const long long q = ((long long)zz * P.oy + yy) * P.ox + (x4 + dx);
      float dot[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
      if (vin && (dx & 3) == 0) gather_quad<true, T, D>(e, S, q, lo, hi, ec, dot, sq);  // aligned like the own quad, and whole (ox % 4 == 0)
      else gather_quad<false, T, D>(e, S, q, lo, hi, ec, dot, sq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j >= lo && j < hi) a[j] = dot[j] * inv_p[j] * inv_norm(sq[j], P.eps);
    }
    if (P.fill > 0 && i < 3) {  // inference.py:160-163 at the source: pred[.., :s] = pred[.., s:2s] along axis i of channel i
      const int c0 = i == 0 ? z : i == 1 ? y : x4;  // the quad's (first) coordinate along axis i
      if (c0 < P.fill) {
        const int fz = i == 0 ? P.fill : 0, fy = i == 1 ? P.fill : 0, fx = i == 2 ? P.fill : 0;
#pragma unroll 1
        for (int j = 0; j < nv; ++j) {
          if (i == 2 && x4 + j >= P.fill) break;
          const float f = affinity_at<T, D>(P, e, i, z + fz, y + fy, x4 + j + fx);
          a[0] = j == 0 ? f : a[0]; a[1] = j == 1 ? f : a[1]; a[2] = j == 2 ? f : a[2]; a[3] = j == 3 ? f : a[3];
        }
      }
    }
    float prod[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      prod[j] = act_affs(a[j], P.act) * w[j];
      asm volatile("" : "+v"(prod[j]));  // keep the product a rounded f32: hipcc would contract a * b + c into one FMA
    }
    float* oc = out + (size_t)i * SV + o;
    if (vout) {
      f4 cur = *(const f4*)oc;
      cur.x = cur.x + prod[0]; cur.y = cur.y + prod[1]; cur.z = cur.z + prod[2]; cur.w = cur.w + prod[3];
      *(f4*)oc = cur;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) oc[j] = oc[j] + prod[j];
    }
  }
  if (vout) {
    f4 cur = *(const f4*)(wmap + o);
    cur.x = cur.x + w[0]; cur.y = cur.y + w[1]; cur.z = cur.z + w[2]; cur.w = cur.w + w[3];
    *(f4*)(wmap + o) = cur;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) wmap[o + j] = wmap[o + j] + w[j];
  }
}

bool fuses(const PeaDesc* d, int fill_shift) {
  return d->border == PEA_BORDER_CROP_ZERO && (d->D == 16 || d->D == 32) && (fill_shift == 0 || fill_shift == 1) &&
         !(d->flags & PEA_FLAG_LOSS_ACT);
}

}  // namespace

extern "C" {

int pea_infer_stitch_supported(const PeaDesc* desc, int fill_shift) {
  return pea_desc_validate(desc) == PEA_OK && fuses(desc, fill_shift) ? 1 : 0;
}

int pea_affinity_infer_stitch(const PeaDesc* desc, const void* e, int fill_shift, const float* weight_vol, float* out_affs,
                              float* weight_map, int Z, int Y, int X, int z0, int y0, int x0, void* stream) {
  const int rc = pea_desc_validate(desc);
  if (rc) return rc;
  if (desc->B != 1) return PEA_E_DESC;
  const int oz = desc->dims[0], oy = desc->dims[1], ox = desc->dims[2];
  if (Z < 1 || Y < 1 || X < 1 || z0 < 0 || y0 < 0 || x0 < 0 || oz > Z - z0 || oy > Y - y0 || ox > X - x0) return PEA_E_DESC;
  if (fill_shift < 0) return PEA_E_DESC;
  // the fill of channel i < 3 reads [fill_shift, 2 * fill_shift) along axis i (K >= 3: every axis, the rule of pea_fill_border_relu)
  for (int a = 0; a < 3 && a < desc->K; ++a)
    if (fill_shift > 0 && 2LL * fill_shift > desc->dims[a]) return PEA_E_DESC;
  if (!e || !weight_vol || !out_affs || !weight_map) return PEA_E_NULL;
  if (misaligned(e, dtype_bytes(desc->dtype)) || misaligned(weight_vol, 4) || misaligned(out_affs, 4) || misaligned(weight_map, 4))
    return PEA_E_ALIGN;
  if (!fuses(desc, fill_shift)) return PEA_E_UNSUPPORTED;

  ISParams P;
  memset(&P, 0, sizeof(P));
  P.oz = oz; P.oy = oy; P.ox = ox; P.K = desc->K;
  P.Z = Z; P.Y = Y; P.X = X; P.z0 = z0; P.y0 = y0; P.x0 = x0;
  P.S = oz * oy * ox;  // fits: pea_desc_validate
  P.xq = (ox + 3) / 4;
  P.quads = oz * oy * P.xq;
  P.tiles = (P.quads + kBlock - 1) / kBlock;
  P.tiles_per_xcd = (P.tiles + kXcd - 1) / kXcd;
  P.fill = fill_shift;
  P.act = desc->flags & kActMask;
  P.eps = desc->eps;
  for (int i = 0; i < desc->K; ++i)
    for (int a = 0; a < 3; ++a) P.off[i][a] = desc->offsets[i][a];
  // rows of the window / of the volume start on a quad boundary: S and Z * Y * X are then multiples of 4 as well
  P.vin = ox % 4 == 0 && !misaligned(e, 4 * dtype_bytes(desc->dtype)) && !misaligned(weight_vol, 16);
  P.vout = ox % 4 == 0 && X % 4 == 0 && x0 % 4 == 0 && !misaligned(out_affs, 16) && !misaligned(weight_map, 16);

  const dim3 grid((unsigned)(P.tiles_per_xcd * kXcd)), blk(kBlock);
  hipStream_t s = (hipStream_t)stream;
  with_storage(desc->dtype, [&](auto st) {
    using T = typename decltype(st)::type;
    return with_width<16, 32>(desc->D, [&](auto dw) {
      return launch<k_infer_stitch<T, decltype(dw)::value>>(grid, blk, 0, s, P, (const T*)e, weight_vol, out_affs, weight_map);
    });
  });
  return hip_rc();
}

}  // extern "C"
