// pea_k_ws.hip -- the watershed fragments on the device (include/pea_ws.h): distance transform, seeds, flood.  What the reference's
// utils/lmc.py and scripts_ac3ac4/utils/fragment.py do per z-plane on the host with elf's distance_transform_watershed and
// mahotas.cwatershed.  All data are N independent planes [N, Y, X]; S = Y * X < 2^30; a workgroup of the per-pixel kernels owns 256
// consecutive pixels of one plane, so consecutive lanes take consecutive x.  Every access is one element wide: any element-aligned
// pointer is served with the same result.
//
// pea_ws_seeds
//   k_ws_rowdist   a wave per row: g(y, x) = the distance along x to the nearest boundary pixel of the row, by a max-scan of the last
//                  boundary index from the left and a min-scan of the next one from the right, 64 pixels a step with a carry
//   k_ws_coldist   dt2(y, x) = min over y' of (y - y')^2 + g(y', x)^2: a lane walks outwards from y and stops once dy^2 reaches the best
//                  so far; the plane's integer extrema by atomicMin / atomicMax
//   k_ws_pre       dt = sqrtf(dt2) and the height map before smoothing
//   k_ws_gauss_x / k_ws_gauss_y   the separable Gaussian through LDS with an r halo, mirrored border
//   k_ws_key       the order-preserving image of dts as an int32 image, which pea_cc_label (pea_k_cc.hip: its union-find is reused whole,
//                  through its entry point) splits into plateaus under maxima_connectivity
//   k_ws_disq      one flag per plateau, set by any pixel that sees a higher neighbour;  k_ws_mask  the pixels of the plateaus without
//   pea_cc_label   on that mask under seed_connectivity: the seeds, 1 .. n in raster order of their first pixel
// pea_ws_flood (Boruvka; the header states the definition and why it ends)
//   k_ws_finit     root[p] = par[p] = p, slot[p] = none, seed[p] = the seed id or 0
//   per round:  k_ws_pick  per pixel of an unlabelled tree the smallest key over its neighbours in other trees, one 64-bit atomicMin
//               into the slot of the tree's root;  k_ws_hook  per unlabelled root with a slot: par[root] = the root at the other end
//               of the edge, unless the two picked the same edge and this one is the smaller; roots are read from root[], the snapshot
//               of the last compress, and only parents of roots are written;  k_ws_compress  every pixel follows par[] from its old
//               root by path halving (a chain can be as long as a plane) and writes root[p]; the slots are cleared
//   k_ws_tally .. k_ws_write   sizes per seed id, the size filter (then a second flood), the rank of the kept ids, the offsets of the
//               planes, the labels (k_ws_rank and k_ws_offsets on block_scan_excl of pea_stream.h)
// Host: seeds_layout and flood_layout carve the two workspaces (pea_carve.h); pea_cc_label's grid acceptance is pea::cc_grids_fit.
#include "../../include/pea_ws.h"
#include "../../include/pea_cc.h"
#include "pea_stream.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace pea;

namespace {

typedef unsigned long long u64t;
constexpr u64t kNoSlot = ~0ull;
constexpr int kNoDist = 0x7fffffff;  // g of a row without a boundary pixel
constexpr int kPlaneWords = 64;      // int32 words per plane of the flood: a flag per round, then the counters
constexpr int kMaxRounds = 32;       // ceil(log2(S)) + 1 <= 31 for S < 2^30
enum { W_FOUND = 40, W_KEPT, W_ZEROS, W_OFFSET, W_NKEPT };
constexpr int kGaussTileX = 64, kGaussTileY = 32;

struct WsParams {
  int N, Y, X;
  int S;            // Y * X
  unsigned chunks;  // runs of 256 pixels of a plane
  int big;          // Y * Y + X * X
  float threshold, alpha;
  int conn;         // the connectivity of the kernel at hand
  int min_size;
  unsigned flags;
};
struct GaussW { float w[PEA_WS_MAX_RADIUS + 1]; int r; };

// blockIdx -> (plane, pixel of the plane); false: past the plane
__device__ __forceinline__ bool pixel_at(const WsParams& P, int* n, int* p) {
  *n = (int)(blockIdx.x / P.chunks);
  *p = (int)((blockIdx.x % P.chunks) * kBlock + threadIdx.x);
  return *p < P.S;
}

// ---- the distance transform ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ws_rowdist(const WsParams P, const float* __restrict__ in, int* __restrict__ g,
                                                       int* __restrict__ ext) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= (long long)P.N * P.Y) return;  // (the whole wave: it meets no other)
  if (lane == 0 && row % P.Y == 0) {        // the plane's extrema of dt2, for k_ws_coldist
    ext[(row / P.Y) * 2] = 0x7fffffff;
    ext[(row / P.Y) * 2 + 1] = 0;
  }
  const float* __restrict__ ip = in + row * P.X;
  int* __restrict__ gp = g + row * P.X;
  int carry = -1;
#pragma unroll 1
  for (int base = 0; base < P.X; base += 64) {  // the last boundary index at or before x
    const int x = base + lane;
    int v = (x < P.X && ip[x] > P.threshold) ? x : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v = t > v ? t : v;
    }
    v = carry > v ? carry : v;
    if (x < P.X) gp[x] = v;
    carry = __shfl(v, 63, 64);
  }
  carry = kNoDist;
#pragma unroll 1
  for (int base = (P.X - 1) / 64 * 64; base >= 0; base -= 64) {  // the next boundary index at or after x
    const int x = base + lane;
    int v = (x < P.X && ip[x] > P.threshold) ? x : kNoDist;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(v, o, 64);
      if (lane + o < 64) v = t < v ? t : v;
    }
    v = carry < v ? carry : v;
    if (x < P.X) {
      const int last = gp[x];
      const int dl = last >= 0 ? x - last : kNoDist, dr = v != kNoDist ? v - x : kNoDist;
      gp[x] = dl < dr ? dl : dr;
    }
    carry = __shfl(v, 0, 64);
  }
}

__global__ __launch_bounds__(kBlock) void k_ws_coldist(const WsParams P, const int* __restrict__ g, int* __restrict__ dt2,
                                                       int* __restrict__ ext) {
  int n, p;
  const bool in = pixel_at(P, &n, &p);
  int best = P.big;
  if (in) {
    const int y = p / P.X;
    const int* __restrict__ col = g + (size_t)n * P.S + (p - y * P.X);
    const int g0 = col[(size_t)y * P.X];
    if (g0 != kNoDist) best = g0 * g0;
#pragma unroll 1
    for (int d = 1; d < P.Y; ++d) {  // d * d <= Y * Y and g * g <= X * X: the sums fit an int32 (the launcher checked big)
      const int dd = d * d;
      if (dd >= best) break;
      const bool up = y - d >= 0, down = y + d < P.Y;
      if (!up && !down) break;
      if (up) {
        const int gv = col[(size_t)(y - d) * P.X];
        if (gv != kNoDist) { const int c = dd + gv * gv; best = c < best ? c : best; }
      }
      if (down) {
        const int gv = col[(size_t)(y + d) * P.X];
        if (gv != kNoDist) { const int c = dd + gv * gv; best = c < best ? c : best; }
      }
    }
    dt2[(size_t)n * P.S + p] = best;
  }
  // the extrema of the plane (a wave may straddle nothing: a workgroup lies in one plane)
  int lo = in ? best : 0x7fffffff, hi = in ? best : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0 && lo != 0x7fffffff) {
    atomicMin(ext + (size_t)n * 2, lo);
    atomicMax(ext + (size_t)n * 2 + 1, hi);
  }
}

// dt (where wanted) and the height map before smoothing (where wanted)
__global__ __launch_bounds__(kBlock) void k_ws_pre(const WsParams P, const float* __restrict__ boundary, const int* __restrict__ dt2,
                                                   const int* __restrict__ ext, float* __restrict__ dt_out, float* __restrict__ pre_out) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  const size_t i = (size_t)n * P.S + p;
  const float dt = sqrtf((float)dt2[i]);
  if (dt_out) dt_out[i] = dt;
  if (pre_out) {
    const float dmin = sqrtf((float)ext[(size_t)n * 2]), dmax = sqrtf((float)ext[(size_t)n * 2 + 1]);
    const float q = dmax == dmin ? 0.0f : (dt - dmin) / (dmax - dmin);
    pre_out[i] = P.alpha * boundary[i] + (1.0f - P.alpha) * (1.0f - q);
  }
}

__global__ __launch_bounds__(kBlock) void k_ws_copy(const WsParams P, const float* __restrict__ in, float* __restrict__ out) {
  int n, p;
  if (pixel_at(P, &n, &p)) out[(size_t)n * P.S + p] = in[(size_t)n * P.S + p];
}

// ---- the Gaussian -----------------------------------------------------------------------------------------------------------------------
// i mirrored into 0 .. n - 1 without repeating the edge (r < n: one reflection is enough)
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(kBlock) void k_ws_gauss_x(const WsParams P, const GaussW G, unsigned cx, const float* __restrict__ in,
                                                       float* __restrict__ out) {
  __shared__ float s[kBlock + 2 * PEA_WS_MAX_RADIUS];
  const size_t row = blockIdx.x / cx;  // of N * Y
  const int x0 = (int)(blockIdx.x % cx) * kBlock;
  const float* __restrict__ ip = in + row * P.X;
  for (int i = threadIdx.x; i < kBlock + 2 * G.r; i += kBlock) {
    const int gx = x0 - G.r + i;
    s[i] = gx <= P.X - 1 + G.r ? ip[mirror(gx, P.X)] : 0.0f;  // (past the last halo: not read below)
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= P.X) return;
  float acc = 0.0f;
  for (int k = -G.r; k <= G.r; ++k) acc += G.w[k < 0 ? -k : k] * s[(int)threadIdx.x + G.r + k];
  out[row * P.X + x] = acc;
}

__global__ __launch_bounds__(kBlock) void k_ws_gauss_y(const WsParams P, const GaussW G, unsigned ty, unsigned tx, const float* __restrict__ in,
                                                       float* __restrict__ out) {
  __shared__ float s[kGaussTileY + 2 * PEA_WS_MAX_RADIUS][kGaussTileX];
  unsigned t = blockIdx.x;
  const int x0 = (int)(t % tx) * kGaussTileX; t /= tx;
  const int y0 = (int)(t % ty) * kGaussTileY;
  const size_t n = t / ty;
  const int lx = threadIdx.x & (kGaussTileX - 1), ly0 = threadIdx.x / kGaussTileX;
  const int x = x0 + lx;
  const float* __restrict__ ip = in + n * P.S;
  for (int i = ly0; i < kGaussTileY + 2 * G.r; i += kBlock / kGaussTileX) {
    const int gy = y0 - G.r + i;
    s[i][lx] = (x < P.X && gy <= P.Y - 1 + G.r) ? ip[(size_t)mirror(gy, P.Y) * P.X + x] : 0.0f;
  }
  __syncthreads();
  if (x >= P.X) return;
  for (int j = ly0; j < kGaussTileY; j += kBlock / kGaussTileX) {
    const int y = y0 + j;
    if (y >= P.Y) break;
    float acc = 0.0f;
    for (int k = -G.r; k <= G.r; ++k) acc += G.w[k < 0 ? -k : k] * s[j + G.r + k][lx];
    out[n * P.S + (size_t)y * P.X + x] = acc;
  }
}

// ---- plateau maxima -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ws_key(const WsParams P, const float* __restrict__ dts, int* __restrict__ key, int* __restrict__ flag) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  key[(size_t)n * P.S + p] = (int)f32_ord(dts[(size_t)n * P.S + p] + 0.0f);  // (-0.0 + 0.0 = +0.0: one plateau with +0.0)
  flag[(size_t)n * ((size_t)P.S + 1) + p + 1] = 0;                           // plateau ids are 1 .. S
}

__global__ __launch_bounds__(kBlock) void k_ws_disq(const WsParams P, const int* __restrict__ key, const int* __restrict__ plab,
                                                    int* __restrict__ flag) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  const int* __restrict__ kp = key + (size_t)n * P.S;
  const int y = p / P.X, x = p - y * P.X;
  const unsigned mine = (unsigned)kp[p];
  bool higher = false;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      if ((!dy && !dx) || (dy && dx && P.conn < 2)) continue;
      const int ny = y + dy, nx = x + dx;
      if ((unsigned)ny >= (unsigned)P.Y || (unsigned)nx >= (unsigned)P.X) continue;
      higher |= (unsigned)kp[ny * P.X + nx] > mine;
    }
  if (higher) {
    const int id = plab[(size_t)n * P.S + p];
    if (id > 0) flag[(size_t)n * ((size_t)P.S + 1) + id] = 1;  // (every writer writes 1)
  }
}

__global__ __launch_bounds__(kBlock) void k_ws_mask(const WsParams P, const int* __restrict__ plab, const int* __restrict__ flag,
                                                    uint8_t* __restrict__ mask) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  const int id = plab[(size_t)n * P.S + p];
  mask[(size_t)n * P.S + p] = (id > 0 && !flag[(size_t)n * ((size_t)P.S + 1) + id]) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_ws_seed_counts(int N, const int* __restrict__ cc_counts, int32_t* __restrict__ counts) {
  const int n = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (n < N) counts[n] = cc_counts[(size_t)n * 2 + 1];
}

// ---- the flood ------------------------------------------------------------------------------------------------------------------------------
struct Flood {
  int* root;   // [N][S] the root of p's tree at the last compress
  int* par;    // [N][S] meaningful for roots: itself, or the root it was hooked onto
  int* seed;   // [N][S] the seed id of p in 1 .. S, or 0
  u64t* slot;  // [N][S] of a root: the smallest key of an outgoing edge this round
  int* cnt;    // [N][S + 1] per seed id: pixels, later the new id
  int* pl;     // [N][kPlaneWords]
};

// first: the seeds of the caller are read and the counters of the planes cleared; else the forest alone starts over
__global__ __launch_bounds__(kBlock) void k_ws_finit(const WsParams P, const Flood F, const int32_t* __restrict__ seeds, int first) {
  int n, p;
  if (threadIdx.x < kPlaneWords && blockIdx.x % P.chunks == 0) {
    const int w = threadIdx.x;
    if (first || w < W_FOUND) F.pl[(size_t)(blockIdx.x / P.chunks) * kPlaneWords + w] = 0;
  }
  if (!pixel_at(P, &n, &p)) return;
  const size_t i = (size_t)n * P.S + p;
  F.root[i] = p;
  F.par[i] = p;
  F.slot[i] = kNoSlot;
  if (first) {
    const int s = seeds[i];
    F.seed[i] = (s >= 1 && s <= P.S) ? s : 0;
    F.cnt[(size_t)n * ((size_t)P.S + 1) + p + 1] = 0;
  }
}

// has round k of plane n anything to do?  Round k - 1 hooked nothing: the forest is final
__device__ __forceinline__ bool round_open(const Flood& F, int n, int k) { return k == 0 || F.pl[(size_t)n * kPlaneWords + k - 1] != 0; }

__global__ __launch_bounds__(kBlock) void k_ws_pick(const WsParams P, const Flood F, const float* __restrict__ hmap, int k) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  if (!round_open(F, n, k)) return;
  const size_t base = (size_t)n * P.S;
  const int* __restrict__ root = F.root + base;
  const float* __restrict__ h = hmap + base;
  const int r = root[p];
  if (F.seed[base + r]) return;  // a labelled tree never picks
  const int y = p / P.X, x = p - y * P.X;
  const unsigned hp = f32_ord(h[p]);
  u64t best = kNoSlot;
  const auto look = [&](int q, unsigned edge) {
    if (root[q] == r) return;
    const unsigned hq = f32_ord(h[q]);
    const u64t key = ((u64t)(hq > hp ? hq : hp) << 32) | edge;
    best = key < best ? key : best;
  };
  if (x + 1 < P.X) look(p + 1, 2u * (unsigned)p);
  if (x > 0) look(p - 1, 2u * (unsigned)(p - 1));
  if (y + 1 < P.Y) look(p + P.X, 2u * (unsigned)p + 1u);
  if (y > 0) look(p - P.X, 2u * (unsigned)(p - P.X) + 1u);
  if (best != kNoSlot) atomicMin(F.slot + base + r, best);
}

__global__ __launch_bounds__(kBlock) void k_ws_hook(const WsParams P, const Flood F, int k) {
  int n, r;
  if (!pixel_at(P, &n, &r)) return;
  if (!round_open(F, n, k)) return;
  const size_t base = (size_t)n * P.S;
  if (F.root[base + r] != r || F.seed[base + r]) return;
  const u64t key = F.slot[base + r];
  if (key == kNoSlot) return;
  const unsigned e = (unsigned)key;
  const int p = (int)(e >> 1), q = p + ((e & 1u) ? P.X : 1);
  const int a = F.root[base + p], b = F.root[base + q];
  const int o = a == r ? b : a;
  if (!F.seed[base + o] && F.slot[base + o] == key && r < o) return;  // the two picked the same edge: the smaller root stays
  F.par[base + r] = o;
  F.pl[(size_t)n * kPlaneWords + k] = 1;  // (every writer writes 1)
}

__global__ __launch_bounds__(kBlock) void k_ws_compress(const WsParams P, const Flood F, int k) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  if (!F.pl[(size_t)n * kPlaneWords + k]) return;  // nothing was hooked: root[] stands, and no later round reads a slot
  const size_t base = (size_t)n * P.S;
  int* par = F.par + base;
  // Path halving from the old root.  par[] of a true root is itself and is not written here; every other word that is written gets an
  // ancestor of its node, whoever writes it, so a walk only ever moves up a forest and ends at the root.
  int x = F.root[base + p];
  for (;;) {
    const int px = PEA_LD_AGENT(par + x);
    if (px == x) break;
    const int gp = PEA_LD_AGENT(par + px);
    if (gp == px) { x = px; break; }
    PEA_ST_AGENT(par + x, gp);
    x = gp;
  }
  F.root[base + p] = x;
  F.slot[base + p] = kNoSlot;
}

// pixels per seed id
__global__ __launch_bounds__(kBlock) void k_ws_tally(const WsParams P, const Flood F) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  const size_t base = (size_t)n * P.S;
  const int id = F.seed[base + F.root[base + p]];
  if (id) atomicAdd(F.cnt + (size_t)n * ((size_t)P.S + 1) + id, 1);
}

// over the ids: how many were found, how many have at least min_size pixels
__global__ __launch_bounds__(kBlock) void k_ws_found(const WsParams P, const Flood F) {
  int n, p;
  const bool in = pixel_at(P, &n, &p);
  const int c = in ? F.cnt[(size_t)n * ((size_t)P.S + 1) + p + 1] : 0;
  const int nf = wave_sum(c > 0 ? 1 : 0), nk = wave_sum((c > 0 && c >= P.min_size) ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && nf) {
    atomicAdd(F.pl + (size_t)n * kPlaneWords + W_FOUND, nf);
    if (nk) atomicAdd(F.pl + (size_t)n * kPlaneWords + W_KEPT, nk);
  }
}

// the size filter: the seeds of the fragments below min_size go, unless none would remain in the plane
__global__ __launch_bounds__(kBlock) void k_ws_filter(const WsParams P, const Flood F) {
  int n, p;
  if (!pixel_at(P, &n, &p)) return;
  if (!F.pl[(size_t)n * kPlaneWords + W_KEPT]) return;
  const size_t i = (size_t)n * P.S + p;
  const int s = F.seed[i];
  if (s && F.cnt[(size_t)n * ((size_t)P.S + 1) + s] < P.min_size) F.seed[i] = 0;
}

// one workgroup per plane walks the ids 256 at a time with a carry: cnt[id] becomes the new id of a kept id (its rank in ascending
// order of id), 0 of any other; counts[n]
__global__ __launch_bounds__(kBlock) void k_ws_rank(const WsParams P, const Flood F, int32_t* __restrict__ counts) {
  const int n = blockIdx.x;
  int* cnt = F.cnt + (size_t)n * ((size_t)P.S + 1);
  const int* pl = F.pl + (size_t)n * kPlaneWords;
  const bool all = P.min_size <= 1 || pl[W_KEPT] == 0;  // (read before the barrier below; W_NKEPT is another word)
  int carry = 0;
#pragma unroll 1
  for (int base = 1; base <= P.S; base += kBlock) {  // (uniform: every lane meets every barrier)
    const int id = base + (int)threadIdx.x;
    const int c = id <= P.S ? cnt[id] : 0;
    const int keep = (c > 0 && (all || c >= P.min_size)) ? 1 : 0;
    int total;
    const int ex = block_scan_excl(keep, &total);
    if (id <= P.S) cnt[id] = keep ? carry + ex + 1 : 0;
    carry += total;
  }
  if (threadIdx.x == 0) {
    counts[(size_t)n * 2] = pl[W_FOUND];
    counts[(size_t)n * 2 + 1] = carry;
    F.pl[(size_t)n * kPlaneWords + W_NKEPT] = carry;
  }
}

// one workgroup: the exclusive prefix of the kept counts over the planes (0 everywhere without PEA_WS_STACK_IDS)
__global__ __launch_bounds__(kBlock) void k_ws_offsets(const WsParams P, const Flood F) {
  int carry = 0;
#pragma unroll 1
  for (int base = 0; base < P.N; base += kBlock) {
    const int n = base + (int)threadIdx.x;
    const int v = n < P.N ? F.pl[(size_t)n * kPlaneWords + W_NKEPT] : 0;
    int total;
    const int ex = block_scan_excl(v, &total);
    if (n < P.N) F.pl[(size_t)n * kPlaneWords + W_OFFSET] = (P.flags & PEA_WS_STACK_IDS) ? carry + ex : 0;
    carry += total;
  }
}

__global__ __launch_bounds__(kBlock) void k_ws_write(const WsParams P, const Flood F, int32_t* __restrict__ labels) {
  int n, p;
  const bool in = pixel_at(P, &n, &p);
  int id = 0;
  if (in) {
    const size_t base = (size_t)n * P.S;
    const int s = F.seed[base + F.root[base + p]];
    id = s ? F.cnt[(size_t)n * ((size_t)P.S + 1) + s] : 0;
    labels[base + p] = id ? id + F.pl[(size_t)n * kPlaneWords + W_OFFSET] : 0;
  }
  const int nz = wave_sum((in && !id) ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && nz) atomicAdd(F.pl + (size_t)n * kPlaneWords + W_ZEROS, nz);
}

__global__ __launch_bounds__(kBlock) void k_ws_stats(int N, const Flood F, int32_t* __restrict__ stats) {
  const int n = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (n >= N) return;
  const int* pl = F.pl + (size_t)n * kPlaneWords;
  int rounds = 0;
  for (int k = 0; k < kMaxRounds; ++k) rounds += pl[k] ? 1 : 0;
  stats[(size_t)n * 2] = rounds;
  stats[(size_t)n * 2 + 1] = pl[W_ZEROS];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t ws_pixels(const PeaWsDesc* d) { return mul_sat((uint64_t)d->Y, (uint64_t)d->X); }
// (int)(3 sigma + 0.5), decided in floating point first: a radius past the served one comes back as PEA_WS_MAX_RADIUS + 1, so no sigma
// however large (validate admits any finite one) reaches a conversion that does not fit an int
inline int gauss_radius(float sigma) {
  const double v = 3.0 * (double)sigma + 0.5;
  return v >= (double)(PEA_WS_MAX_RADIUS + 1) ? PEA_WS_MAX_RADIUS + 1 : (int)v;
}

inline void cc_desc(const PeaWsDesc* d, int in_type, int conn, PeaCcDesc* c) {
  memset(c, 0, sizeof(*c));
  c->ndim = 2; c->B = d->N;
  c->dims[0] = 1; c->dims[1] = d->Y; c->dims[2] = d->X;
  c->in_type = in_type; c->connectivity = conn; c->min_size = 0; c->flags = 0;
}

// the blocks of the seeds' workspace in order, each a multiple of 8 bytes: six images of 4 bytes a pixel (g then the keys; dt2; dt; the
// Gaussian's row pass; the height map before smoothing then the plateau ids; dts), a flag per plateau id, the mask, per plane the
// extrema of dt2 and the counts of pea_cc_label, the workspace of pea_cc_label
struct SeedsWs {
  int *a, *dt2;
  float *dtf, *tmp, *pre, *dts;
  int* flag;
  uint8_t* mask;
  int *ext, *ccc;
  char* cc;
  size_t cc_bytes;
};
inline size_t seeds_layout(const PeaWsDesc* d, void* base, SeedsWs* w) {
  const uint64_t N = (uint64_t)d->N, per = mul_sat(N, ws_pixels(d));
  PeaCcDesc c;
  cc_desc(d, PEA_CC_IN_I32, 1, &c);
  w->cc_bytes = pea_cc_workspace_bytes(&c);  // (the same for either element type and connectivity)
  Carver k(base);
  w->a = k.take<int>(per); w->dt2 = k.take<int>(per);
  w->dtf = k.take<float>(per); w->tmp = k.take<float>(per); w->pre = k.take<float>(per); w->dts = k.take<float>(per);
  w->flag = k.take<int>(mul_sat(N, add_sat(ws_pixels(d), 1)));
  w->mask = k.take<uint8_t>(per);
  w->ext = k.take<int>(2 * N); w->ccc = k.take<int>(2 * N);
  w->cc = k.take<char>(w->cc_bytes, 1);
  return k.bytes();
}

// the flood's blocks: root, par and seed (4 bytes a pixel each), the slots (8), a counter per seed id, 64 words per plane
inline size_t flood_layout(const PeaWsDesc* d, void* base, Flood* F) {
  const uint64_t N = (uint64_t)d->N, per = mul_sat(N, ws_pixels(d));
  Carver k(base);
  F->root = k.take<int>(per); F->par = k.take<int>(per); F->seed = k.take<int>(per);
  F->slot = k.take<u64t>(per);
  F->cnt = k.take<int>(mul_sat(N, add_sat(ws_pixels(d), 1)));
  F->pl = k.take<int>(kPlaneWords * N);
  return k.bytes();
}

// S < 2^30 and a grid of one workgroup per 256 pixels of a plane
inline bool ws_grid(const PeaWsDesc* d, WsParams* P, unsigned* groups) {
  const uint64_t S = ws_pixels(d);
  if (S >= (1ull << 30)) return false;
  if (!stream_grid(S, (uint64_t)d->N, kBlock, &P->chunks, groups)) return false;
  P->N = d->N; P->Y = d->Y; P->X = d->X; P->S = (int)S;
  P->big = 0;
  P->threshold = d->threshold; P->alpha = d->alpha;
  P->conn = 1; P->min_size = d->min_size; P->flags = d->flags;
  return true;
}

inline GaussW gauss_weights(float sigma) {
  GaussW G;
  memset(&G, 0, sizeof(G));
  G.r = gauss_radius(sigma);
  double w[PEA_WS_MAX_RADIUS + 1], sum = 0.0;
  for (int i = 0; i <= G.r && i <= PEA_WS_MAX_RADIUS; ++i) {
    w[i] = exp(-0.5 * (double)i * (double)i / ((double)sigma * (double)sigma));
    sum += i ? 2.0 * w[i] : w[i];
  }
  for (int i = 0; i <= G.r && i <= PEA_WS_MAX_RADIUS; ++i) G.w[i] = (float)(w[i] / sum);
  return G;
}

// out = G(sigma) * in through tmp (in != out, in != tmp; tmp != out)
inline void launch_gauss(LaunchChain& chain, const WsParams& P, float sigma, const float* in, float* tmp, float* out) {
  const GaussW G = gauss_weights(sigma);
  const unsigned cx = (unsigned)((P.X + kBlock - 1) / kBlock);
  const unsigned ty = (unsigned)((P.Y + kGaussTileY - 1) / kGaussTileY), tx = (unsigned)((P.X + kGaussTileX - 1) / kGaussTileX);
  chain(k_ws_gauss_x, (unsigned)((uint64_t)P.N * P.Y * cx), kBlock, P, G, cx, in, tmp);
  chain(k_ws_gauss_y, (unsigned)((uint64_t)P.N * ty * tx), kBlock, P, G, ty, tx, tmp, out);
}
// is a Gaussian of this sigma served on the planes, and do its grids fit?
inline bool gauss_ok(const PeaWsDesc* d, float sigma) {
  const int r = gauss_radius(sigma);
  if (sigma == 0.0f) return true;
  if (r > PEA_WS_MAX_RADIUS || r >= d->Y || r >= d->X) return false;
  const uint64_t cx = ((uint64_t)d->X + kBlock - 1) / kBlock;
  const uint64_t ty = ((uint64_t)d->Y + kGaussTileY - 1) / kGaussTileY, tx = ((uint64_t)d->X + kGaussTileX - 1) / kGaussTileX;
  return mul_sat(mul_sat((uint64_t)d->N, (uint64_t)d->Y), cx) <= 0x7fffffffULL && mul_sat((uint64_t)d->N, ty * tx) <= 0x7fffffffULL;
}

}  // namespace

extern "C" int pea_ws_validate(const PeaWsDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->N < 1 || d->Y < 1 || d->X < 1) return PEA_E_DESC;
  if (!isfinite(d->threshold) || !isfinite(d->sigma_seeds) || !isfinite(d->sigma_weights) || !isfinite(d->alpha)) return PEA_E_DESC;
  if (d->sigma_seeds < 0.0f || d->sigma_weights < 0.0f || d->alpha < 0.0f || d->alpha > 1.0f) return PEA_E_DESC;
  if (d->maxima_connectivity != 1 && d->maxima_connectivity != 2) return PEA_E_DESC;
  if (d->seed_connectivity != 1 && d->seed_connectivity != 2) return PEA_E_DESC;
  if (d->min_size < 0) return PEA_E_DESC;
  if (d->flags & ~(PEA_WS_STACK_IDS | PEA_WS_FIELD)) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" size_t pea_ws_seeds_workspace_bytes(const PeaWsDesc* d) {
  SeedsWs w;
  return pea_ws_validate(d) ? 0 : seeds_layout(d, nullptr, &w);
}

extern "C" size_t pea_ws_flood_workspace_bytes(const PeaWsDesc* d) {
  Flood F;
  return pea_ws_validate(d) ? 0 : flood_layout(d, nullptr, &F);
}

extern "C" int pea_ws_seeds(const PeaWsDesc* d, const float* boundary, int32_t* dt2, float* dts, float* hmap, int32_t* seeds, int32_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_ws_validate(d);
  if (vrc) return vrc;
  const bool field = (d->flags & PEA_WS_FIELD) != 0;
  if (!boundary || !seeds || !counts || (field && (dt2 || hmap))) return PEA_E_NULL;
  if (misaligned(boundary, 4) || misaligned(dt2, 4) || misaligned(dts, 4) || misaligned(hmap, 4) || misaligned(seeds, 4) ||
      misaligned(counts, 4) || misaligned(workspace, 8))
    return PEA_E_ALIGN;
  SeedsWs W;
  if (!workspace || workspace_bytes < seeds_layout(d, workspace, &W)) return PEA_E_WORKSPACE;
  WsParams P;
  unsigned groups;
  if (!ws_grid(d, &P, &groups)) return PEA_E_UNSUPPORTED;
  const uint64_t big = (uint64_t)d->Y * d->Y + (uint64_t)d->X * d->X;
  if (big >= (1ull << 31)) return PEA_E_UNSUPPORTED;
  P.big = (int)big;
  if (!gauss_ok(d, d->sigma_seeds) || (hmap && !gauss_ok(d, d->sigma_weights))) return PEA_E_UNSUPPORTED;
  PeaCcDesc c;
  cc_desc(d, PEA_CC_IN_I32, d->maxima_connectivity, &c);
  const uint64_t rows = ((uint64_t)d->N * d->Y + kBlock / 64 - 1) / (kBlock / 64);
  if (!cc_grids_fit(&c) || rows > 0x7fffffffULL) return PEA_E_UNSUPPORTED;  // (every refusal comes before the first launch)

  LaunchChain chain(stream);
  int* dt2p = dt2 ? dt2 : W.dt2;
  float* dtsp = dts ? dts : W.dts;
  if (field) {
    if (d->sigma_seeds == 0.0f) chain(k_ws_copy, groups, kBlock, P, boundary, dtsp);
    else launch_gauss(chain, P, d->sigma_seeds, boundary, W.tmp, dtsp);
  } else {
    chain(k_ws_rowdist, (unsigned)rows, kBlock, P, boundary, W.a, W.ext);
    chain(k_ws_coldist, groups, kBlock, P, W.a, dt2p, W.ext);
    const bool smooth_s = d->sigma_seeds != 0.0f, smooth_w = d->sigma_weights != 0.0f;
    chain(k_ws_pre, groups, kBlock, P, boundary, dt2p, W.ext, smooth_s ? W.dtf : dtsp, hmap ? (smooth_w ? W.pre : hmap) : nullptr);
    if (smooth_s) launch_gauss(chain, P, d->sigma_seeds, W.dtf, W.tmp, dtsp);
    if (hmap && smooth_w) launch_gauss(chain, P, d->sigma_weights, W.pre, W.tmp, hmap);
  }
  // plateaus of dts, the maxima among them, the components of their mask
  int* plab = (int*)W.pre;
  chain(k_ws_key, groups, kBlock, P, dtsp, W.a, W.flag);
  if (!chain.rc) chain.rc = pea_cc_label(&c, W.a, plab, nullptr, W.ccc, W.cc, W.cc_bytes, stream);
  P.conn = d->maxima_connectivity;
  chain(k_ws_disq, groups, kBlock, P, W.a, plab, W.flag);
  chain(k_ws_mask, groups, kBlock, P, plab, W.flag, W.mask);
  cc_desc(d, PEA_CC_IN_U8, d->seed_connectivity, &c);
  if (!chain.rc) chain.rc = pea_cc_label(&c, W.mask, seeds, nullptr, W.ccc, W.cc, W.cc_bytes, stream);
  chain(k_ws_seed_counts, (unsigned)((d->N + kBlock - 1) / kBlock), kBlock, d->N, W.ccc, counts);
  return chain.rc;
}

extern "C" int pea_ws_flood(const PeaWsDesc* d, const float* hmap, const int32_t* seeds, int32_t* labels, int32_t* counts, int32_t* stats,
                            void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_ws_validate(d);
  if (vrc) return vrc;
  if (!hmap || !seeds || !labels || !counts || !stats) return PEA_E_NULL;
  if (misaligned(hmap, 4) || misaligned(seeds, 4) || misaligned(labels, 4) || misaligned(counts, 4) || misaligned(stats, 4) ||
      misaligned(workspace, 8))
    return PEA_E_ALIGN;
  Flood F;
  if (!workspace || workspace_bytes < flood_layout(d, workspace, &F)) return PEA_E_WORKSPACE;
  WsParams P;
  unsigned groups;
  if (!ws_grid(d, &P, &groups)) return PEA_E_UNSUPPORTED;
  // stacked ids are int32 sums of the kept counts, which a seed on every pixel makes N * Y * X
  if ((d->flags & PEA_WS_STACK_IDS) && mul_sat((uint64_t)d->N, (uint64_t)P.S) >= (1ull << 31)) return PEA_E_UNSUPPORTED;

  int rounds = 1;  // ceil(log2(S)) + 1
  while ((1ll << (rounds - 1)) < (long long)P.S) ++rounds;
  LaunchChain chain(stream);
  const auto flood = [&](int first) {
    chain(k_ws_finit, groups, kBlock, P, F, seeds, first);
    for (int k = 0; k < rounds && !chain.rc; ++k) {
      chain(k_ws_pick, groups, kBlock, P, F, hmap, k);
      chain(k_ws_hook, groups, kBlock, P, F, k);
      chain(k_ws_compress, groups, kBlock, P, F, k);
    }
  };
  flood(1);
  chain(k_ws_tally, groups, kBlock, P, F);
  chain(k_ws_found, groups, kBlock, P, F);
  if (d->min_size > 1) {
    chain(k_ws_filter, groups, kBlock, P, F);
    flood(0);
  }
  chain(k_ws_rank, d->N, kBlock, P, F, counts);
  chain(k_ws_offsets, 1, kBlock, P, F);
  chain(k_ws_write, groups, kBlock, P, F, labels);
  chain(k_ws_stats, (unsigned)((d->N + kBlock - 1) / kBlock), kBlock, d->N, F, stats);
  return chain.rc;
}
