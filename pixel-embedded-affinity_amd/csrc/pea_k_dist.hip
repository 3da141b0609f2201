// pea_k_dist.hip -- distance-form affinities of the raw embedding (include/pea_dist.h): a = max((2 delta_d - h) / (2 delta_d), 0)^2 with
// h = d outside the dead zone d <= delta_v, d = |e(p) - e(p + o)|, forward and vjp.  One translation unit of libpea_hip.so.
//
// The gather form of pea_gather.h: one lane per voxel, consecutive lanes along x, so every channel plane of the [D, S] layout is read
// coalesced and every one of the K output planes is stored coalesced.  The own D channels sit in registers; a neighbour vector
// streams in channel by channel.  Nothing is exchanged between lanes and one lane owns each store: no LDS, no atomics, no workspace.
// The 1-D grid is remapped so that each XCD walks a contiguous span of voxels (dist_tile).
//
//   forward   per offset: ss = sum_c (own[c] - v_c)^2 by fmaf in channel order, d = sqrtf(ss), the dead zone, u, the select, the
//             square, the optional inversion, one store.  Under the zero-vector border a pair that leaves the volume reads nothing: its
//             ss is the own vector's sum of squares (own[c] - 0 = own[c]: the same chain, taken once).
//   vjp       gather, no scatter: G[D] in registers.  For offset i, role A is the pair (p, p + o_i) with g_i(p); role B walks the
//             pre-image of p -- the p' with p' + o_i = p: p - o_i if it lies inside under the zero-vector border, the box of
//             clamp_preimage along each axis under REPLICATE -- with g_i(p').  d is symmetric in its two vectors and the direction
//             changes sign with the role, so both add  c * (own - other),  c = g * slope(d) / d  (0 in the dead zone, where u <= 0
//             and where d == 0).  de = dscale * G, rounded once.
//
// Widths.  D = 16 and D = 32 have instantiations of their own.  Every other D in 1..64 runs the form of the next padded width W
// (8 / 16 / 32 / 64) with the channel loop predicated on c < D (D is uniform: scalar branches), the channels past D held as zeros, so
// the register arrays stay statically indexed and nothing goes to scratch.
#include "../../include/pea_dist.h"
#include "pea_dispatch.h"
#include "pea_gather.h"

using namespace pea;

namespace {

// geometry in the shape split_voxel() and neighbour<kBorderRuntime>() read.  border: PEA_BORDER_REPLICATE, or PEA_BORDER_CROP_ZERO for
// the zero-vector rule (neighbour() then answers -1 outside the volume, which is all the kernels ask of it)
struct DistGeom {
  int B, D, Z, Y, X, K;
  int S, chunks;          // chunks: workgroups per image = ceil(S / kBlock)
  int tiles, tiles_per_xcd;  // B * chunks; ceil(tiles / 8): the grid is 8 * tiles_per_xcd
  int border;
  int invert;
  float delta_v, delta_d, two_dd;  // two_dd = 2 delta_d (exact)
  int off[PEA_MAX_K][3];
};

// XCD-aware remap, as logical_tile() of pea_common.h: the hardware deals consecutive workgroup ids round-robin over the 8 XCDs, so XCD g
// walks the contiguous tiles [g * tiles_per_xcd, (g + 1) * tiles_per_xcd) and the neighbour vectors it re-reads stay in its own L2
__device__ __forceinline__ int dist_tile(const DistGeom& G) {
  const int bid = blockIdx.x;
  return (bid % kXcd) * G.tiles_per_xcd + bid / kXcd;
}

template <int W, bool PRED, typename T>
__device__ __forceinline__ void load_own(const DistGeom& G, const T* eb, size_t S, int p, float (&own)[W]) {
#pragma unroll
  for (int c = 0; c < W; ++c) own[c] = (!PRED || c < G.D) ? ld(eb, c * S + p) : 0.f;
}

// u of a distance: the dead zone, then (2 delta_d - h) / (2 delta_d)
__device__ __forceinline__ float dist_u(const DistGeom& G, float d) {
  const float h = d <= G.delta_v ? 0.f : d;
  return (G.two_dd - h) / G.two_dd;
}

template <typename T, int W, bool PRED>
__global__ __launch_bounds__(kBlock) void k_dist_fwd(const DistGeom G, const T* __restrict__ e, float* __restrict__ affs) {
  const int tile = dist_tile(G);
  if (tile >= G.tiles) return;
  const int b = tile / G.chunks;
  const int p = (tile - b * G.chunks) * kBlock + threadIdx.x;
  if (p >= G.S) return;
  const size_t S = (size_t)G.S;
  const T* eb = e + (size_t)b * G.D * S;
  float* ab = affs + (size_t)b * G.K * S;
  int z, y, x;
  split_voxel(G, p, z, y, x);

  float own[W];
  load_own<W, PRED>(G, eb, S, p, own);
  float own_ss = 0.f;  // the pair with the zero vector
#pragma unroll
  for (int c = 0; c < W; ++c) own_ss = fmaf(own[c], own[c], own_ss);

  for (int i = 0; i < G.K; ++i) {
    const int q = neighbour(G, z, y, x, G.off[i][0], G.off[i][1], G.off[i][2]);
    float ss = own_ss;
    if (q >= 0) {
      ss = 0.f;
#pragma unroll
      for (int c = 0; c < W; ++c) {
        if (!PRED || c < G.D) {
          const float t = own[c] - ld(eb, c * S + q);
          ss = fmaf(t, t, ss);
        }
      }
    }
    const float u = relu_keep_nan(dist_u(G, sqrtf(ss)));
    float a = fmaf(ss, 0.f, u * u);  // ss not finite: NaN (include/pea_dist.h); else + 0, which changes no bit of u * u >= 0
    if (G.invert) a = 1.0f - a;
    ab[(size_t)i * S + p] = a;
  }
}

// one pair of the vjp: Gr += c * (own - e(q)), c = gv * slope(d) / d; q < 0: the zero vector
template <int W, bool PRED, typename T>
__device__ __forceinline__ void dist_pair(const DistGeom& G, const T* eb, size_t S, int q, float gv, const float (&own)[W], float (&Gr)[W]) {
  float t[W], ss = 0.f;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    t[c] = own[c];
    if (q >= 0 && (!PRED || c < G.D)) t[c] = own[c] - ld(eb, c * S + q);
    ss = fmaf(t[c], t[c], ss);
  }
  const float d = sqrtf(ss);
  const float u = dist_u(G, d);
  // da / dd = -u / delta_d on the slope; d > delta_v >= 0 there, so the division by d is taken where d > 0 only
  const float coef = (u > 0.f && d > G.delta_v) ? gv * (-u / G.delta_d) / d : 0.f;
#pragma unroll
  for (int c = 0; c < W; ++c) Gr[c] = fmaf(coef, t[c], Gr[c]);
}

template <typename T, int W, bool PRED>
__global__ __launch_bounds__(kBlock) void k_dist_vjp(const DistGeom G, const T* __restrict__ e, const float* __restrict__ gin,
                                                     const float* __restrict__ dscale, T* __restrict__ de) {
  const int tile = dist_tile(G);
  if (tile >= G.tiles) return;
  const int b = tile / G.chunks;
  const int p = (tile - b * G.chunks) * kBlock + threadIdx.x;
  if (p >= G.S) return;
  const size_t S = (size_t)G.S;
  const T* eb = e + (size_t)b * G.D * S;
  const float* gb = gin + (size_t)b * G.K * S;
  T* db = de + (size_t)b * G.D * S;
  // the inverted map's vjp is the negated one, bit for bit (signed zeros included): the sign rides on the scale
  const float dl = G.invert ? -(dscale ? dscale[0] : 1.f) : (dscale ? dscale[0] : 1.f);
  int z, y, x;
  split_voxel(G, p, z, y, x);

  float own[W], Gr[W] = {};
  load_own<W, PRED>(G, eb, S, p, own);

  for (int i = 0; i < G.K; ++i) {
    const int oz = G.off[i][0], oy = G.off[i][1], ox = G.off[i][2];
    // role A: the pair of p itself
    dist_pair<W, PRED>(G, eb, S, neighbour(G, z, y, x, oz, oy, ox), gb[(size_t)i * S + p], own, Gr);
    // role B: every p' whose neighbour is p
    int z0, z1, y0, y1, x0, x1;
    if (G.border == PEA_BORDER_REPLICATE) {
      clamp_preimage(z, oz, G.Z, z0, z1);
      clamp_preimage(y, oy, G.Y, y0, y1);
      clamp_preimage(x, ox, G.X, x0, x1);
    } else {
      z0 = z1 = z - oz; y0 = y1 = y - oy; x0 = x1 = x - ox;
      if ((unsigned)z0 >= (unsigned)G.Z || (unsigned)y0 >= (unsigned)G.Y || (unsigned)x0 >= (unsigned)G.X) z1 = z0 - 1;  // empty
    }
    for (int zz = z0; zz <= z1; ++zz)
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
          const int q = (zz * G.Y + yy) * G.X + xx;
          dist_pair<W, PRED>(G, eb, S, q, gb[(size_t)i * S + q], own, Gr);
        }
  }
#pragma unroll
  for (int c = 0; c < W; ++c)
    if (!PRED || c < G.D) st_rounded(db, c * S + p, dl * Gr[c]);
}

// f(Int<W>{}, PRED): the instantiation of a width (file comment)
template <typename F>
inline void with_dist_width(int D, F&& f) {
  if (D == 16) f(Int<16>{}, std::false_type{});
  else if (D == 32) f(Int<32>{}, std::false_type{});
  else if (D <= 8) f(Int<8>{}, std::true_type{});
  else if (D <= 16) f(Int<16>{}, std::true_type{});
  else if (D <= 32) f(Int<32>{}, std::true_type{});
  else f(Int<64>{}, std::true_type{});
}

int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// descriptor -> geometry; PEA_E_UNSUPPORTED where the volume or the grid leaves the 32-bit range
int make_geom(const PeaDistDesc* d, DistGeom* G) {
  const int64_t zy = (int64_t)d->dims[0] * d->dims[1];
  if (zy > 0x7fffffffLL || zy * d->dims[2] > 0x7fffffffLL) return PEA_E_UNSUPPORTED;
  const int64_t S = zy * d->dims[2];
  const int64_t chunks = (S + kBlock - 1) / kBlock;
  if (chunks * d->B > 0x7fffffffLL - (kXcd - 1)) return PEA_E_UNSUPPORTED;  // the grid is rounded up to a multiple of 8
  G->B = d->B; G->D = d->D; G->Z = d->dims[0]; G->Y = d->dims[1]; G->X = d->dims[2]; G->K = d->K;
  G->S = (int)S; G->chunks = (int)chunks;
  G->tiles = (int)(chunks * d->B); G->tiles_per_xcd = (G->tiles + kXcd - 1) / kXcd;
  G->border = d->border == PEA_BORDER_REPLICATE ? PEA_BORDER_REPLICATE : PEA_BORDER_CROP_ZERO;
  G->invert = (d->flags & PEA_DIST_INVERT) ? 1 : 0;
  G->delta_v = d->delta_v; G->delta_d = d->delta_d; G->two_dd = 2.0f * d->delta_d;
  for (int i = 0; i < PEA_MAX_K; ++i)
    for (int a = 0; a < 3; ++a)
      // an offset of the extent n or more acts like n under either border (the clamp folds onto the last slice; the zero-vector rule
      // leaves the volume from every voxel), and p + o then stays inside int
      G->off[i][a] = i < d->K ? clampi(d->offsets[i][a], -d->dims[a], d->dims[a]) : 0;
  return PEA_OK;
}

}  // namespace

extern "C" int pea_dist_validate(const PeaDistDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->D < 1 || d->D > PEA_DIST_MAX_D || d->K < 1 || d->K > PEA_MAX_K) return PEA_E_DESC;
  for (int a = 0; a < 3; ++a)
    if (d->dims[a] < 1) return PEA_E_DESC;
  if (d->dtype != PEA_F32 && d->dtype != PEA_F16 && d->dtype != PEA_BF16) return PEA_E_DESC;
  if (d->border != PEA_BORDER_REPLICATE && d->border != PEA_DIST_BORDER_ZERO_VECTOR) return PEA_E_DESC;
  if (d->flags & ~PEA_DIST_INVERT) return PEA_E_DESC;
  if (!__builtin_isfinite(d->delta_d) || !(d->delta_d > 0.f)) return PEA_E_DESC;
  if (!__builtin_isfinite(d->delta_v) || d->delta_v < 0.f) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" int pea_dist_affinity(const PeaDistDesc* d, const void* e, float* affs, void* stream) {
  const int v = pea_dist_validate(d);
  if (v != PEA_OK) return v;
  if (!e || !affs) return PEA_E_NULL;
  if (misaligned(e, dtype_bytes(d->dtype)) || misaligned(affs, 4)) return PEA_E_ALIGN;
  DistGeom G;
  const int r = make_geom(d, &G);
  if (r != PEA_OK) return r;
  const dim3 grid((unsigned)G.tiles_per_xcd * kXcd);
  with_storage(d->dtype, [&](auto st) {
    using T = typename decltype(st)::type;
    with_dist_width(d->D, [&](auto w, auto pred) {
      launch<k_dist_fwd<T, w.value, pred.value>>(grid, dim3(kBlock), 0, (hipStream_t)stream, G, (const T*)e, affs);
    });
  });
  return hip_rc();
}

extern "C" int pea_dist_affinity_vjp(const PeaDistDesc* d, const void* e, const float* g, const float* dscale, void* de, void* stream) {
  const int v = pea_dist_validate(d);
  if (v != PEA_OK) return v;
  if (!e || !g || !de) return PEA_E_NULL;
  const size_t eb = dtype_bytes(d->dtype);
  if (misaligned(e, eb) || misaligned(de, eb) || misaligned(g, 4) || (dscale && misaligned(dscale, 4))) return PEA_E_ALIGN;
  DistGeom G;
  const int r = make_geom(d, &G);
  if (r != PEA_OK) return r;
  const dim3 grid((unsigned)G.tiles_per_xcd * kXcd);
  with_storage(d->dtype, [&](auto st) {
    using T = typename decltype(st)::type;
    with_dist_width(d->D, [&](auto w, auto pred) {
      launch<k_dist_vjp<T, w.value, pred.value>>(grid, dim3(kBlock), 0, (hipStream_t)stream, G, (const T*)e, g, dscale, (T*)de);
    });
  });
  return hip_rc();
}
