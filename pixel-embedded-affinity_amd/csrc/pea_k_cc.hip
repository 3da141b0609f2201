// pea_k_cc.hip -- connected-component labelling on the device (include/pea_cc.h): label, size filter, mask.  What
// scripts_bbbc039v1/utils/postprocessing.py:43-48 (remove_samll_object), utils/merge_small.py:106 (labelVolumeWithBackground) and
// convert_mask2ins.py:33 (skimage.morphology.label) do on the host.
//
// Two pixels are joined iff they are neighbours under `connectivity` (an offset in {-1, 0, 1}^3 with |dz| + |dy| + |dx| <= connectivity),
// their value is not 0 and it is the same.  The forest lives in the workspace: parent[b][p] is a flat index of image b that is <= p and
// lies in p's component (-1 for background); the root of a component is its smallest flat index, which is the numbering rule of the header.
//
// Seven launches, none per component, and launch boundaries are the only ordering between workgroups:
//   1 k_cc_tile      a workgroup labels one 32 x 32 tile of one plane in LDS by label equivalence: every pixel starts with its own local
//                    index, takes the minimum over its joined neighbours inside the tile, follows that label's own label down (pointer
//                    jumping) and lowers its label and its old label's with atomicMin; the loop ends when a workgroup-wide vote says that
//                    nothing fell.  Labels only fall and are bounded below, so the vote comes.  Local and flat order agree inside a tile, so
//                    the local root is the tile's smallest flat index of the component: parent[p] = its flat index, size[p] = 0.
//                    3D: the z step is one more border of the 2D tile (8 KiB of LDS per workgroup whatever Z is,
//                    and the volumes of the drivers are a few planes of large extent).
//   2 k_cc_merge     every pixel unions itself with its joined neighbours of SMALLER flat index that lie in another tile (each
//                    unordered pair once): find both roots, atomicMin the larger root's parent down to the smaller, go on from what the
//                    atomic returned.  max(a, b) falls strictly with every round, so a union ends; a find only ever steps to a strictly
//                    smaller index, so it ends whatever it reads.  A union is a chain of dependent L2 accesses, so pairs that other
//                    pairs imply are left out (a diagonal beside a straight neighbour; all of a run along x but its first pair).
//   3 k_cc_compress  every pixel finds its root and writes it back; a wave peels its equal roots (pea_stream.h) and adds one count per
//                    (wave, root) to size[root] -- a blob that fills a tile costs 16 atomics on its root, not 1024.
//   4 k_cc_totals    per 1024 pixels of an image: how many roots, how many kept ones (parent[i] == i, size[i] >= min_size)
//   5 k_cc_scan      one workgroup per image: exclusive prefix of the kept totals (block_scan_excl, pea_stream.h), in place; counts[b]
//   6 k_cc_apply     size[root] = the root's new id = prefix of its block + its rank in the block + 1, 0 for a dropped one.  A root is its
//                    component's first pixel, so the scan in flat order IS the raster-order numbering.
//   7 k_cc_write     labels_out[p] = size[parent[p]], mask_out[p] = that != 0
// Every value is an integer; roots are minima and sizes integer sums, so no result depends on the order in which workgroups arrive.
// Host: cc_layout carves the three blocks (pea_carve.h), cc_grids decides what pea_cc_label takes (pea::cc_grids_fit for pea_k_ws.hip).
#include "../../include/pea_cc.h"
#include "pea_stream.h"

using namespace pea;

namespace {

constexpr int kTile = 32;                   // a tile is kTile x kTile pixels of one plane
constexpr int kTilePix = kTile * kTile;
constexpr int kTileSteps = kTilePix / kBlock;  // pixels per lane: local index step * 256 + lane, so a wave reads two rows of the tile
constexpr int kNoLabel = 0x7fffffff;        // the LDS label of a background pixel
static_assert(kTilePix == kBlock * kTileSteps && kBlock % kTile == 0, "a workgroup's step is whole rows of the tile");

struct CcParams {
  size_t S;            // Z * Y * X
  int Z, Y, X;
  unsigned ty, tx;     // tiles of a plane
  unsigned chunks;     // runs of kQuadRun pixels of an image
  int conn;            // 1 .. 3
  int min_size;
};

// blockIdx -> the tile: image, plane, first row and column
struct TileAt { size_t b; int z, y0, x0; };
__device__ __forceinline__ TileAt tile_at(const CcParams& P) {
  unsigned t = blockIdx.x;
  const unsigned txi = t % P.tx; t /= P.tx;
  const unsigned tyi = t % P.ty; t /= P.ty;
  const unsigned z = t % (unsigned)P.Z;
  return {(size_t)(t / (unsigned)P.Z), (int)z, (int)(tyi * kTile), (int)(txi * kTile)};
}

// ---- 1. the tile pass -----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_cc_tile(const CcParams P, const T* __restrict__ in, int* __restrict__ parent, int* __restrict__ size) {
  __shared__ int s_val[kTilePix];
  __shared__ int s_lab[kTilePix];
  const TileAt at = tile_at(P);
  const T* __restrict__ ip = in + at.b * P.S;
  const int lx = threadIdx.x & (kTile - 1), ly0 = threadIdx.x / kTile;
  const bool diag = P.conn >= 2;  // inside a plane: the 4- or the 8-neighbourhood
  int val[kTileSteps];
#pragma unroll
  for (int j = 0; j < kTileSteps; ++j) {
    const int ly = j * (kBlock / kTile) + ly0, l = ly * kTile + lx;
    const int gy = at.y0 + ly, gx = at.x0 + lx;
    int v = 0;
    if (gy < P.Y && gx < P.X) v = (int)ip[((size_t)at.z * P.Y + gy) * P.X + gx];
    val[j] = v;
    s_val[l] = v;
    s_lab[l] = v ? l : kNoLabel;
  }
  __syncthreads();

  // Labels only fall (atomicMin) and a label is always a local index of the pixel's own component, so a round in which nothing fell
  // comes after at most kTilePix * kTilePix rounds; in practice pointer jumping ends a serpentine in a few tens.
  for (;;) {
    int fell = 0;
#pragma unroll
    for (int j = 0; j < kTileSteps; ++j) {
      const int v = val[j];
      if (!v) continue;
      const int ly = j * (kBlock / kTile) + ly0, l = ly * kTile + lx;
      const int cur = s_lab[l];
      int m = cur;
      const auto look = [&](int ny, int nx) {
        if ((unsigned)ny < (unsigned)kTile && (unsigned)nx < (unsigned)kTile) {
          const int n = ny * kTile + nx;
          if (s_val[n] == v) {
            const int t = s_lab[n];
            m = t < m ? t : m;
          }
        }
      };
      look(ly - 1, lx); look(ly, lx - 1); look(ly, lx + 1); look(ly + 1, lx);
      if (diag) { look(ly - 1, lx - 1); look(ly - 1, lx + 1); look(ly + 1, lx - 1); look(ly + 1, lx + 1); }
      for (int r = s_lab[m]; r < m; r = s_lab[m]) m = r;  // strictly down: ends
      if (m < cur) {
        if (atomicMin(&s_lab[l], m) > m) fell = 1;
        if (atomicMin(&s_lab[cur], m) > m) fell = 1;     // the old label's pixel learns of it too
      }
    }
    if (!__syncthreads_or(fell)) break;
  }

  int* __restrict__ pp = parent + at.b * P.S;
  int* __restrict__ sp = size + at.b * P.S;
#pragma unroll
  for (int j = 0; j < kTileSteps; ++j) {
    const int ly = j * (kBlock / kTile) + ly0, l = ly * kTile + lx;
    const int gy = at.y0 + ly, gx = at.x0 + lx;
    if (gy < P.Y && gx < P.X) {
      const size_t plane0 = (size_t)at.z * P.Y;
      const size_t p = (plane0 + gy) * P.X + gx;
      int root = -1;
      if (val[j]) {
        const int r = s_lab[l];
        root = (int)((plane0 + at.y0 + r / kTile) * P.X + at.x0 + (r & (kTile - 1)));
      }
      pp[p] = root;
      sp[p] = 0;
    }
  }
}

// ---- 2. the border merge ----------------------------------------------------------------------------------------------------------------
// the root of x: a step goes to a strictly smaller index or the walk is over, so it ends whatever the words hold
__device__ __forceinline__ int cc_find(int* par, int x) {
  for (;;) {
    const int p = PEA_LD_AGENT(par + x);
    if (p >= x || p < 0) return x;
    x = p;
  }
}
// a and b are one component.  A parent that the atomic replaces was a link a -> old of the same component, which the next round
// restores as a union of old and b; max(a, b) falls strictly from round to round.
__device__ __forceinline__ void cc_union(int* par, int a, int b) {
  for (;;) {
    a = cc_find(par, a);
    b = cc_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;  // a was a root and now hangs below b
    a = old;               // a hung below old < a already
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_cc_merge(const CcParams P, const T* __restrict__ in, int* __restrict__ parent) {
  const TileAt at = tile_at(P);
  const T* __restrict__ ip = in + at.b * P.S;
  int* par = parent + at.b * P.S;
  const int lx = threadIdx.x & (kTile - 1), ly0 = threadIdx.x / kTile;
  const int gx = at.x0 + lx;
  if (gx >= P.X) return;
#pragma unroll 1
  for (int j = 0; j < kTileSteps; ++j) {
    const int ly = j * (kBlock / kTile) + ly0, gy = at.y0 + ly;
    if (gy >= P.Y) break;
    // a neighbour of smaller flat index in another tile: in the plane below, the row above from the tile's first row, the column
    // to the left from its first column, the diagonal to the upper right from its last column
    if (!(at.z > 0 || ly == 0 || lx == 0 || lx == kTile - 1)) continue;
    const size_t p = ((size_t)at.z * P.Y + gy) * P.X + gx;
    const T v = ip[p];
    if (!v) continue;
#pragma unroll 1
    for (int dz = -1; dz <= 0; ++dz) {
      if (at.z + dz < 0) continue;
#pragma unroll 1
      for (int dy = -1; dy <= (dz ? 1 : 0); ++dy) {
        const int ny = gy + dy;
        if ((unsigned)ny >= (unsigned)P.Y) continue;
        const int lastx = (dz || dy < 0) ? 1 : -1;
#pragma unroll 1
        for (int dx = -1; dx <= lastx; ++dx) {
          const int nx = gx + dx;
          if ((unsigned)nx >= (unsigned)P.X) continue;
          if (-dz + (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx) > P.conn) continue;
          if (!dz && ny / kTile == gy / kTile && nx / kTile == gx / kTile) continue;  // the tile pass joined them
          const size_t q = ((size_t)(at.z + dz) * P.Y + ny) * P.X + nx;
          if (ip[q] != v) continue;
          // Pairs that other pairs imply are left out; what is left joins the same components (by induction: straight pairs along
          // x, then diagonals).  A diagonal of the plane is implied where the pixel above p or the pixel beside p has the value: it
          // is a straight neighbour of both.  A pair is implied by the same pair one pixel to the left where that one crosses
          // tiles too and p - 1, q - 1 lie in the tiles of p, q and have the value: only the first pair of a run makes the union.
          if (!dz && dy && dx && (ip[q - dx] == v || ip[p + dx] == v)) continue;
          if (lx > 0 && (nx & (kTile - 1)) != 0 && (dz || ny / kTile != gy / kTile) && ip[p - 1] == v && ip[q - 1] == v) continue;
          cc_union(par, (int)p, (int)q);
        }
      }
    }
  }
}

// ---- 3. compress and count ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cc_compress(const CcParams P, int* __restrict__ parent, int* __restrict__ size) {
  const BlockAt at = block_at(P.chunks);
  int* par = parent + (size_t)at.plane * P.S;
  int* sz = size + (size_t)at.plane * P.S;
  const int lane = threadIdx.x & 63;
  const size_t i0 = quad_start(at.chunk);
  const int nv = quad_nv(i0, P.S);
  int key[kQuad];
  unsigned open = 0;
#pragma unroll
  for (int e = 0; e < kQuad; ++e) {
    key[e] = 0;
    if (e < nv) {
      const int first = PEA_LD_AGENT(par + i0 + e);
      if (first >= 0) {
        const int r = cc_find(par, first);
        if (r != first) PEA_ST_AGENT(par + i0 + e, r);  // (whoever walks through this word meets the old ancestor or the root)
        key[e] = r + 1;
        open |= 1u << e;
      }
    }
  }
  // the r-th root that the wave peels is kept by lane r; the lanes then add side by side
  int mykey = 0, mycnt = 0, r = 0, cur;
  unsigned mm;
  const auto flush = [&]() {
    if (mykey) PEA_ATOM_ADD(sz + (mykey - 1), mycnt);
    mykey = 0;
  };
  while (peel(key, open, cur, mm)) {
    const int cnt = wave_sum((int)__popc(mm));
    if (lane == r) { mykey = cur; mycnt = cnt; }
    if (++r == 64) { flush(); r = 0; }
  }
  flush();
}

// ---- 4 - 6. the scan ----------------------------------------------------------------------------------------------------------------------
// the lane's quad: bit e of *root: pixel i0 + e is a root; bit e of *kept: a root of at least min_size pixels
__device__ __forceinline__ void quad_roots(const CcParams& P, const int* __restrict__ par, const int* __restrict__ sz, size_t i0, int nv,
                                           unsigned* root, unsigned* kept) {
  int p[kQuad], s[kQuad];
  ld_iquad(par + (nv ? i0 : 0), nv, -1, p);
  ld_iquad(sz + (nv ? i0 : 0), nv, 0, s);
  *root = *kept = 0;
#pragma unroll
  for (int e = 0; e < kQuad; ++e) {
    const bool is_root = e < nv && p[e] == (int)(i0 + e);
    if (is_root) *root |= 1u << e;
    if (is_root && s[e] >= P.min_size) *kept |= 1u << e;
  }
}

__global__ __launch_bounds__(kBlock) void k_cc_totals(const CcParams P, const int* __restrict__ parent, const int* __restrict__ size,
                                                      int* __restrict__ tot) {
  __shared__ int s_part[2][kBlock / 64];
  const BlockAt at = block_at(P.chunks);
  const size_t i0 = quad_start(at.chunk);
  unsigned root, kept;
  quad_roots(P, parent + (size_t)at.plane * P.S, size + (size_t)at.plane * P.S, i0, quad_nv(i0, P.S), &root, &kept);
  const int nr = wave_sum((int)__popc(root)), nk = wave_sum((int)__popc(kept));
  if ((threadIdx.x & 63) == 0) { s_part[0][threadIdx.x >> 6] = nr; s_part[1][threadIdx.x >> 6] = nk; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int* s = s_part[threadIdx.x];
    tot[((size_t)at.plane * P.chunks + at.chunk) * 2 + threadIdx.x] = s[0] + s[1] + s[2] + s[3];
  }
}

// one workgroup per image walks its totals 256 at a time with a carry: tot[..][1] becomes the exclusive prefix of the kept totals
__global__ __launch_bounds__(kBlock) void k_cc_scan(const CcParams P, int* __restrict__ tot, int32_t* __restrict__ counts) {
  int* t = tot + (size_t)blockIdx.x * P.chunks * 2;
  int found = 0, carry = 0;
#pragma unroll 1
  for (unsigned base = 0; base < P.chunks; base += kBlock) {  // (uniform: every lane meets every barrier)
    const unsigned c = base + threadIdx.x;
    const bool in = c < P.chunks;
    const int k = in ? t[(size_t)c * 2 + 1] : 0;
    found += in ? t[(size_t)c * 2] : 0;
    int total;
    const int ex = block_scan_excl(k, &total);
    if (in) t[(size_t)c * 2 + 1] = carry + ex;
    carry += total;
  }
  int total;
  (void)block_scan_excl(found, &total);
  if (threadIdx.x == 0) {
    counts[(size_t)blockIdx.x * 2] = total;
    counts[(size_t)blockIdx.x * 2 + 1] = carry;
  }
}

__global__ __launch_bounds__(kBlock) void k_cc_apply(const CcParams P, const int* __restrict__ parent, int* __restrict__ size,
                                                     const int* __restrict__ tot) {
  const BlockAt at = block_at(P.chunks);
  const size_t i0 = quad_start(at.chunk);
  const int nv = quad_nv(i0, P.S);
  int* sz = size + (size_t)at.plane * P.S;
  unsigned root, kept;
  quad_roots(P, parent + (size_t)at.plane * P.S, sz, i0, nv, &root, &kept);
  int total;
  int id = tot[((size_t)at.plane * P.chunks + at.chunk) * 2 + 1] + block_scan_excl((int)__popc(kept), &total);
#pragma unroll
  for (int e = 0; e < kQuad; ++e) {
    if ((kept >> e) & 1u) sz[i0 + e] = ++id;
    else if ((root >> e) & 1u) sz[i0 + e] = 0;
  }
}

// ---- 7. the write ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cc_write(const CcParams P, const int* __restrict__ parent, const int* __restrict__ size,
                                                     int32_t* __restrict__ labels_out, uint8_t* __restrict__ mask_out) {
  const BlockAt at = block_at(P.chunks);
  const size_t i0 = quad_start(at.chunk);
  const int nv = quad_nv(i0, P.S);
  if (!nv) return;
  const size_t img = (size_t)at.plane * P.S;
  int p[kQuad], id[kQuad];
  ld_iquad(parent + img + i0, nv, -1, p);
#pragma unroll
  for (int e = 0; e < kQuad; ++e) id[e] = p[e] >= 0 ? size[img + p[e]] : 0;
  if (labels_out) {
    int32_t* __restrict__ op = labels_out + img + i0;
    if (nv == kQuad && ((uintptr_t)op & 15) == 0) {
      iquad_t q;
      q.x = id[0]; q.y = id[1]; q.z = id[2]; q.w = id[3];
      *(iquad_t*)op = q;
    } else {
#pragma unroll
      for (int e = 0; e < kQuad; ++e)
        if (e < nv) op[e] = id[e];
    }
  }
  if (mask_out) {
    uint8_t* __restrict__ op = mask_out + img + i0;
    if (nv == kQuad && ((uintptr_t)op & 3) == 0) {
      *(uint32_t*)op = (id[0] ? 1u : 0u) | (id[1] ? 1u << 8 : 0u) | (id[2] ? 1u << 16 : 0u) | (id[3] ? 1u << 24 : 0u);
    } else {
#pragma unroll
      for (int e = 0; e < kQuad; ++e)
        if (e < nv) op[e] = id[e] ? 1 : 0;
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t cc_pixels(const PeaCcDesc* d) { return mul_sat(mul_sat((uint64_t)d->dims[0], (uint64_t)d->dims[1]), (uint64_t)d->dims[2]); }
inline uint64_t cc_chunks(uint64_t S) { return S / kQuadRun + (S % kQuadRun ? 1 : 0); }

// parent and size, int32 [B, S] each, then the scan's totals, int32 [B, chunks, 2]: three blocks without padding
struct CcWs { int *parent, *size, *tot; };
inline size_t cc_layout(const PeaCcDesc* d, void* base, CcWs* w) {
  const uint64_t S = cc_pixels(d), BS = mul_sat((uint64_t)d->B, S);
  Carver c(base);
  w->parent = c.take<int>(BS, 4);
  w->size = c.take<int>(BS, 4);
  w->tot = c.take<int>(mul_sat(mul_sat((uint64_t)d->B, cc_chunks(S)), 2), 4);
  return c.bytes();
}

// S < 2^31, a grid of one workgroup per tile and one per kQuadRun pixels of an image: P's geometry and the two grids
inline bool cc_grids(const PeaCcDesc* d, CcParams* P, unsigned* tiles, unsigned* groups) {
  const uint64_t S = cc_pixels(d);
  if (S >= (1ull << 31)) return false;
  P->S = (size_t)S;
  P->Z = d->dims[0]; P->Y = d->dims[1]; P->X = d->dims[2];
  P->ty = (unsigned)((d->dims[1] + kTile - 1) / kTile);
  P->tx = (unsigned)((d->dims[2] + kTile - 1) / kTile);
  const uint64_t t = mul_sat(mul_sat((uint64_t)d->B, (uint64_t)d->dims[0]), (uint64_t)P->ty * P->tx);
  if (t > 0x7fffffffULL || !stream_grid(S, (uint64_t)d->B, kQuadRun, &P->chunks, groups)) return false;
  *tiles = (unsigned)t;
  return true;
}

}  // namespace

bool pea::cc_grids_fit(const PeaCcDesc* d) {
  CcParams P;
  unsigned tiles, groups;
  return cc_grids(d, &P, &tiles, &groups);
}

extern "C" int pea_cc_validate(const PeaCcDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->ndim != 2 && d->ndim != 3) return PEA_E_DESC;
  if (d->B < 1 || d->dims[0] < 1 || d->dims[1] < 1 || d->dims[2] < 1) return PEA_E_DESC;
  if (d->ndim == 2 && d->dims[0] != 1) return PEA_E_DESC;
  if (d->connectivity < 1 || d->connectivity > d->ndim) return PEA_E_DESC;
  if (d->min_size < 0) return PEA_E_DESC;
  if (d->in_type != PEA_CC_IN_U8 && d->in_type != PEA_CC_IN_I32) return PEA_E_DESC;
  if (d->flags) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" size_t pea_cc_workspace_bytes(const PeaCcDesc* d) {
  CcWs w;
  return pea_cc_validate(d) ? 0 : cc_layout(d, nullptr, &w);
}

extern "C" int pea_cc_label(const PeaCcDesc* d, const void* in, int32_t* labels_out, uint8_t* mask_out, int32_t* counts, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const int vrc = pea_cc_validate(d);
  if (vrc) return vrc;
  if (!in || !counts || (!labels_out && !mask_out)) return PEA_E_NULL;
  if ((d->in_type == PEA_CC_IN_I32 && misaligned(in, 4)) || misaligned(labels_out, 4) || misaligned(counts, 4) || misaligned(workspace, 4))
    return PEA_E_ALIGN;
  CcWs w;
  if (!workspace || workspace_bytes < cc_layout(d, workspace, &w)) return PEA_E_WORKSPACE;
  CcParams P;
  unsigned tiles, groups;
  if (!cc_grids(d, &P, &tiles, &groups)) return PEA_E_UNSUPPORTED;
  P.conn = d->connectivity;
  P.min_size = d->min_size;

  LaunchChain chain(stream);
  const bool u8 = d->in_type == PEA_CC_IN_U8;
  if (u8) chain(k_cc_tile<uint8_t>, tiles, kBlock, P, (const uint8_t*)in, w.parent, w.size);
  else chain(k_cc_tile<int32_t>, tiles, kBlock, P, (const int32_t*)in, w.parent, w.size);
  if (u8) chain(k_cc_merge<uint8_t>, tiles, kBlock, P, (const uint8_t*)in, w.parent);
  else chain(k_cc_merge<int32_t>, tiles, kBlock, P, (const int32_t*)in, w.parent);
  chain(k_cc_compress, groups, kBlock, P, w.parent, w.size);
  chain(k_cc_totals, groups, kBlock, P, w.parent, w.size, w.tot);
  chain(k_cc_scan, d->B, kBlock, P, w.tot, counts);
  chain(k_cc_apply, groups, kBlock, P, w.parent, w.size, w.tot);
  chain(k_cc_write, groups, kBlock, P, w.parent, w.size, labels_out, mask_out);
  return chain.rc;
}
