// pea_k_mws.hip -- the mutex watershed on the device (include/pea_mws.h, which states the definition, the round rule and why it is
// exact).  What the reference's utils/seg_mutex.py does on the host with elf's mutex_watershed.  All data are B independent images of
// S = Z * Y * X pixels and K channels; a workgroup of the edge kernels owns 256 consecutive pixels of ONE channel of one image, so
// consecutive lanes take consecutive x, the channel's offset is uniform, and the far end of lane i's edge is pixel p + delta[k].  A
// workgroup of the pixel kernels owns 256 consecutive pixels of one image.  In the rounds a repulsive channel is walked on its stride
// lattice only (lattice_at): its other slots never hold an edge.  Every access is one element wide: any element-aligned
// pointer is served with the same result.  An edge's key is recomputed from x wherever it is wanted (one load and two subtractions)
// instead of being kept at 8 bytes an edge; what is kept per edge is its state byte.
//
// set-up     k_mws_init_pix    root[p] = par[p] = p, has_con = 0, best = 0, the image's words and its exclusion table cleared
//            k_mws_init_edges  the state byte of every edge slot: undecided where the edge exists, dead where it is missing (counted by
//                              cause and channel)
// per round  k_mws_best        prune (same root, or the root pair is in the table), then best[root] of both ends by a 64-bit atomic max;
//                              a survivor sets the round's ALIVE flag: a round that finds none sets the image's DONE word through k_mws_compress,
//                              and every launch of a later round returns at once
//            k_mws_attr        the attractive decisions: reads best, has_con; writes the edge's state and par[] of the promoting roots
//            k_mws_rep         the repulsive decisions: writes the edge's state and has_con of both roots; in a round without a merge
//                              the new pairs go straight into the table (a pair is promoted by at most one edge and the prune has
//                              shown that it is not there yet)
//            k_mws_compress    best cleared; after a merge: every pixel follows par[] from its old root by path halving and writes
//                              root[p], has_con is carried to the new roots, the table is cleared; one lane per image closes the
//                              round's flags
//            k_mws_reinsert    after a merge: the active exclusions enter the cleared table under their new roots; an active edge
//                              whose pair is already there dies (which of two survives depends on arrival, their number does not)
//            A round never reads what it writes inside one launch, except par[] in the compress (relaxed agent-scope accesses of a
//            forest that only shortens) and the table's slots in claims (one compare-and-swap each).
// labelling  k_mws_count  the undecided edges and the active exclusions, per channel (a round counts nothing: it leaves flags);
//            k_mws_first .. k_mws_write  the smallest pixel of every cluster (atomicMin), a flag on it, the flags' prefix over the
//            image (totals per 256 pixels, one workgroup per image scans them, block_scan_excl): the raster-order numbering
// Host: mws_layout carves the workspace (pea_carve.h).
#include "../../include/pea_mws.h"
#include "pea_stream.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

enum : uint8_t { E_UNDECIDED = 0, E_DEAD = 1, E_MERGED = 2, E_ACTIVE = 3 };
// u64 words per image: 16 of the image, then 8 counters per channel.  Counts are taken where they cost nothing per round -- at the set-up
// and in the labelling, a workgroup's sum into the words of ITS channel, so that the adds spread over K addresses -- and a round leaves
// flags only (plain stores of 1).  The flags come in pairs, used by the parity of the round's index in its call: round k sets [k & 1]
// and clears [(k + 1) & 1].
constexpr int kChanWords = 8;
constexpr int kImgWords = 16 + PEA_MWS_MAX_K * kChanWords;
enum { F_ALIVE = 0, F_MERGED = 2, F_DECIDED = 4, W_DONE = 6, W_ROUNDS, W_VALID };
enum { C_OUT = 0, C_MASK, C_STRIDE, C_NAN, C_UNDEC, C_ACTIVE };
constexpr u64 kMinCapacity = 64;

struct MwsParams {
  int B, Z, Y, X, K, nA;
  unsigned S;       // Z * Y * X < 2^31
  unsigned chunks;  // runs of 256 pixels of an image
  int input;
  int off[PEA_MWS_MAX_K][3];
  int delta[PEA_MWS_MAX_K];  // (dz * Y + dy) * X + dx
  int stride[3];
  unsigned lat[3];      // points of the stride lattice along z, y, x: ceil(extent / stride)
  unsigned lchunks;     // runs of 256 lattice points of an image
  unsigned attr_groups; // workgroups of the attractive channels' walk: B * nA * chunks
  u64 cap;  // slots of an image's table: a power of two
};

struct Mws {
  int* root;       // [B][S] the root of p's cluster at the last compress
  int* par;        // [B][S] meaningful for roots: itself, or the root it was hooked onto
  int* first;      // [B][S] labelling: of a root, the smallest pixel of its cluster
  int* rank;       // [B][S] labelling: of a first pixel, the cluster's id
  int* tot;        // [B][chunks] labelling: first pixels per 256 pixels, then their exclusive prefix
  u64* best;       // [B][S] of a root: the largest key of an undecided edge at the cluster this round; 0 between rounds
  u64* tab;        // [B][cap] (smaller root << 32 | larger root) + 1 of an active exclusion; 0 = empty
  u64* img;        // [B][kImgWords]
  uint8_t* hascon; // [B][S] of a root: the cluster is an end of an active exclusion
  uint8_t* state;  // [B][K][S]
};

// blockIdx -> (image, pixel); false: past the image
__device__ __forceinline__ bool pixel_at(const MwsParams& P, size_t* b, unsigned* p) {
  *b = blockIdx.x / P.chunks;
  *p = (blockIdx.x % P.chunks) * kBlock + threadIdx.x;
  return *p < P.S;
}
// blockIdx -> (image, channel k0 .. k0 + nk - 1, pixel): the channel is uniform over the workgroup
__device__ __forceinline__ bool edge_at(const MwsParams& P, int k0, int nk, size_t* b, int* k, unsigned* p) {
  unsigned t = blockIdx.x;
  *p = (t % P.chunks) * kBlock + threadIdx.x;
  t /= P.chunks;
  *k = k0 + (int)(t % (unsigned)nk);
  *b = t / (unsigned)nk;
  return *p < P.S;
}

// The repulsive channels' walk: an edge of theirs exists on the stride lattice only, so after the set-up a workgroup owns 256
// consecutive LATTICE points of one channel of one image (blk: its index among such workgroups): 1 / (sz * sy * sx) of the slots.
__device__ __forceinline__ bool lattice_at(const MwsParams& P, unsigned blk, size_t* b, int* k, unsigned* p) {
  const unsigned l = (blk % P.lchunks) * kBlock + threadIdx.x;
  blk /= P.lchunks;
  const unsigned nr = (unsigned)(P.K - P.nA);
  *k = P.nA + (int)(blk % nr);
  *b = blk / nr;
  const unsigned xl = l % P.lat[2], t = l / P.lat[2], yl = t % P.lat[1], zl = t / P.lat[1];
  *p = ((zl * (unsigned)P.stride[0]) * (unsigned)P.Y + yl * (unsigned)P.stride[1]) * (unsigned)P.X + xl * (unsigned)P.stride[2];
  return zl < P.lat[0];
}
// every channel's walk in one grid: the attractive channels' workgroups first, then the repulsive channels' lattice workgroups
__device__ __forceinline__ bool round_edge_at(const MwsParams& P, size_t* b, int* k, unsigned* p) {
  return blockIdx.x < P.attr_groups ? edge_at(P, 0, P.nA, b, k, p) : lattice_at(P, blockIdx.x - P.attr_groups, b, k, p);
}

// the weight of an edge of channel k from its element of x (include/pea_mws.h: exactly these roundings)
__device__ __forceinline__ float edge_weight(int input, bool attractive, float v) {
  if (input == PEA_MWS_IN_AFFS) {
    const float c = 1.0f - v;
    return attractive ? 1.0f - c : c;
  }
  if (input == PEA_MWS_IN_ELF) return attractive ? 1.0f - v : v;
  return v;
}
__device__ __forceinline__ u64 edge_key(const MwsParams& P, const float* __restrict__ x, size_t b, int k, unsigned p) {
  const float w = edge_weight(P.input, k < P.nA, x[(b * P.K + k) * (size_t)P.S + p]);
  return ((u64)f32_ord(w) << 32) | (u64)(0xFFFFFFFFu - ((unsigned)k * P.S + p));
}
__device__ __forceinline__ u64 pair_key1(int a, int b) {
  const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
  return (((u64)lo << 32) | (u64)hi) + 1;
}
__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
// is key1 in a table that EARLIER launches filled?  At most cap probes.
__device__ __forceinline__ bool tab_has(const u64* __restrict__ tab, u64 cap, u64 key1) {
  u64 s = mix64(key1) & (cap - 1);
  for (u64 i = 0; i < cap; ++i) {
    const u64 cur = tab[s];
    if (cur == key1) return true;
    if (cur == 0) return false;
    s = (s + 1) & (cap - 1);
  }
  return false;
}
// key1 enters the table: 1 = this lane claimed a slot, 0 = it is there already, -1 = no slot after cap probes (cannot happen: the
// capacity is twice the edges that can be active).  A slot only ever goes from empty to a key inside a launch and every lane of a key
// walks the same sequence, so all of them end on one slot.
__device__ __forceinline__ int tab_claim(u64* __restrict__ tab, u64 cap, u64 key1) {
  u64 s = mix64(key1) & (cap - 1);
  for (u64 i = 0; i < cap; ++i) {
    u64 cur = PEA_LD_AGENT(tab + s);
    if (cur == 0) {
      u64 expect = 0;
      if (__hip_atomic_compare_exchange_strong(tab + s, &expect, key1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 1;
      cur = expect;
    }
    if (cur == key1) return 0;
    s = (s + 1) & (cap - 1);
  }
  return -1;
}
// the workgroup's sums of four 0 / 1 counts per lane (16 bits each of one u64: a sum is at most 256) into four words, NULL = none: one
// atomic per workgroup and word that has anything (integer sums: the order of arrival does not show).  The whole workgroup calls it.
__device__ __forceinline__ void block_count4(u64* w0, u64* w1, u64* w2, u64* w3, bool c0, bool c1, bool c2, bool c3) {
  u64 total;
  (void)block_scan_excl((u64)c0 | ((u64)c1 << 16) | ((u64)c2 << 32) | ((u64)c3 << 48), &total);
  if (threadIdx.x == 0) {
    u64* const w[4] = {w0, w1, w2, w3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 t = (total >> (16 * i)) & 0xffffu;
      if (w[i] && t) PEA_ATOM_ADD(w[i], t);
    }
  }
}
// a flag of the image: one lane per wave that has a reason stores 1 (every writer writes 1)
__device__ __forceinline__ void wave_flag(u64* w, bool mine) {
  if (__ballot(mine) && (threadIdx.x & 63) == 0) *w = 1;
}

// ---- set-up ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_mws_init_pix(const MwsParams P, const Mws M) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  if (blockIdx.x % P.chunks == 0)
    for (int i = threadIdx.x; i < kImgWords; i += kBlock) M.img[b * kImgWords + i] = 0;
  u64* tab = M.tab + b * P.cap;
  for (u64 i = (u64)(blockIdx.x % P.chunks) * kBlock + threadIdx.x; i < P.cap; i += (u64)P.chunks * kBlock) tab[i] = 0;
  if (!in) return;
  const size_t i = b * P.S + p;
  M.root[i] = (int)p;
  M.par[i] = (int)p;
  M.best[i] = 0;
  M.hascon[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_mws_init_edges(const MwsParams P, const Mws M, const float* __restrict__ x,
                                                           const uint8_t* __restrict__ mask) {
  size_t b;
  int k;
  unsigned p;
  const bool in = edge_at(P, 0, P.K, &b, &k, &p);
  int cause = -1;  // -1: past the image; 0: the edge exists; else 1 + the counter of its cause
  if (in) {
    const unsigned YX = (unsigned)P.Y * (unsigned)P.X;
    const int z = (int)(p / YX);
    const unsigned r = p - (unsigned)z * YX;
    const int y = (int)(r / (unsigned)P.X), xx = (int)(r - (unsigned)y * (unsigned)P.X);
    const int qz = z + P.off[k][0], qy = y + P.off[k][1], qx = xx + P.off[k][2];
    cause = 0;
    if ((unsigned)qz >= (unsigned)P.Z || (unsigned)qy >= (unsigned)P.Y || (unsigned)qx >= (unsigned)P.X) cause = 1 + C_OUT;
    else if (mask && (!mask[b * P.S + p] || !mask[b * P.S + (unsigned)((int)p + P.delta[k])])) cause = 1 + C_MASK;
    else if (k >= P.nA && (z % P.stride[0] || y % P.stride[1] || xx % P.stride[2])) cause = 1 + C_STRIDE;
    else {
      const float w = edge_weight(P.input, k < P.nA, x[(b * P.K + k) * (size_t)P.S + p]);
      if (w != w) cause = 1 + C_NAN;
    }
    M.state[(b * P.K + k) * (size_t)P.S + p] = cause ? E_DEAD : E_UNDECIDED;
  }
  u64* ch = M.img + b * kImgWords + 16 + k * kChanWords;  // (b and k are uniform over the workgroup)
  block_count4(ch + C_OUT, ch + C_MASK, ch + C_STRIDE, ch + C_NAN, cause == 1 + C_OUT, cause == 1 + C_MASK, cause == 1 + C_STRIDE, cause == 1 + C_NAN);
}

// a resumed call with a round: the flags of its first round start at 0 (the last round of the call before cleared the other pair)
__global__ __launch_bounds__(kBlock) void k_mws_begin(int B, const Mws M) {
  const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (b >= B) return;
  u64* img = M.img + (size_t)b * kImgWords;
  img[F_ALIVE] = 0; img[F_MERGED] = 0; img[F_DECIDED] = 0;
}

// ---- a round ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_mws_best(const MwsParams P, const Mws M, const float* __restrict__ x, int par) {
  size_t b;
  int k;
  unsigned p;
  const bool in = round_edge_at(P, &b, &k, &p);
  u64* img = M.img + b * kImgWords;
  if (img[W_DONE]) return;
  bool alive = false;
  if (in) {
    uint8_t* st = M.state + (b * P.K + k) * (size_t)P.S + p;
    if (*st == E_UNDECIDED) {
      const int* __restrict__ root = M.root + b * P.S;
      const int ra = root[p], rb = root[(unsigned)((int)p + P.delta[k])];
      if (ra == rb || (P.nA < P.K && tab_has(M.tab + b * P.cap, P.cap, pair_key1(ra, rb)))) *st = E_DEAD;
      else {
        const u64 key = edge_key(P, x, b, k, p);
        u64* best = M.best + b * P.S;
        // (a stale smaller value only costs an atomic that changes nothing: best only grows inside the launch)
        if (PEA_LD_AGENT(best + ra) < key) PEA_ATOM_MAX(best + ra, key);
        if (PEA_LD_AGENT(best + rb) < key) PEA_ATOM_MAX(best + rb, key);
        alive = true;
      }
    }
  }
  wave_flag(img + F_ALIVE + par, alive);
}

__global__ __launch_bounds__(kBlock) void k_mws_attr(const MwsParams P, const Mws M, const float* __restrict__ x, int par) {
  size_t b;
  int k;
  unsigned p;
  const bool in = edge_at(P, 0, P.nA, &b, &k, &p);
  u64* img = M.img + b * kImgWords;
  if (img[W_DONE] || !img[F_ALIVE + par]) return;
  bool merged = false;
  if (in) {
    uint8_t* st = M.state + (b * P.K + k) * (size_t)P.S + p;
    if (*st == E_UNDECIDED) {
      const int* __restrict__ root = M.root + b * P.S;
      const int ra = root[p], rb = root[(unsigned)((int)p + P.delta[k])];
      const u64 key = edge_key(P, x, b, k, p);
      const bool ba = M.best[b * P.S + ra] == key, bb = M.best[b * P.S + rb] == key;
      const bool pa = ba && (bb || !M.hascon[b * P.S + ra]), pb = bb && (ba || !M.hascon[b * P.S + rb]);
      if (pa || pb) {
        *st = E_MERGED;
        merged = true;
        int* parent = M.par + b * P.S;  // par[r] has one writer: the lane of the one edge that is best[r]
        if (pa && pb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
        else if (pa) parent[ra] = rb;
        else parent[rb] = ra;
      }
    }
  }
  if (__ballot(merged) && (threadIdx.x & 63) == 0) { img[F_MERGED + par] = 1; img[F_DECIDED + par] = 1; }
}

__global__ __launch_bounds__(kBlock) void k_mws_rep(const MwsParams P, const Mws M, const float* __restrict__ x, int par) {
  size_t b;
  int k;
  unsigned p;
  const bool in = lattice_at(P, blockIdx.x, &b, &k, &p);
  u64* img = M.img + b * kImgWords;
  if (img[W_DONE] || !img[F_ALIVE + par]) return;
  bool excl = false;
  if (in) {
    uint8_t* st = M.state + (b * P.K + k) * (size_t)P.S + p;
    if (*st == E_UNDECIDED) {
      const int* __restrict__ root = M.root + b * P.S;
      const int ra = root[p], rb = root[(unsigned)((int)p + P.delta[k])];
      const u64 key = edge_key(P, x, b, k, p);
      if (M.best[b * P.S + ra] == key || M.best[b * P.S + rb] == key) {
        *st = E_ACTIVE;
        excl = true;
        M.hascon[b * P.S + ra] = 1;  // (every writer writes 1)
        M.hascon[b * P.S + rb] = 1;
        if (!img[F_MERGED + par]) (void)tab_claim(M.tab + b * P.cap, P.cap, pair_key1(ra, rb));  // (else k_mws_reinsert rebuilds the table)
      }
    }
  }
  wave_flag(img + F_DECIDED + par, excl);
}

__global__ __launch_bounds__(kBlock) void k_mws_compress(const MwsParams P, const Mws M, int par) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  u64* img = M.img + b * kImgWords;
  if (img[W_DONE]) return;  // (set below only in a round with nothing alive, where every lane leaves on the next line as well)
  const u64 alive = img[F_ALIVE + par], nmerge = img[F_MERGED + par];
  if (blockIdx.x % P.chunks == 0 && threadIdx.x == 0) {  // the round's books; the flags of the next round start at 0
    if (!alive) img[W_DONE] = 1;
    if (img[F_DECIDED + par]) img[W_ROUNDS] += 1;
    img[F_ALIVE + (par ^ 1)] = 0; img[F_MERGED + (par ^ 1)] = 0; img[F_DECIDED + (par ^ 1)] = 0;
  }
  if (!alive) return;  // best[] was not touched
  if (nmerge) {
    u64* tab = M.tab + b * P.cap;
    for (u64 i = (u64)(blockIdx.x % P.chunks) * kBlock + threadIdx.x; i < P.cap; i += (u64)P.chunks * kBlock) tab[i] = 0;
  }
  if (!in) return;
  const size_t base = b * P.S;
  M.best[base + p] = 0;
  if (!nmerge) return;  // root[] stands
  int* parent = M.par + base;
  // Path halving from the old root.  par[] of a true root is itself and is not written here; every other word that is written gets an
  // ancestor of its node, whoever writes it, so a walk only ever moves up a forest and ends at the root.
  const int x0 = M.root[base + p];
  int x = x0;
  for (;;) {
    const int px = PEA_LD_AGENT(parent + x);
    if (px == x) break;
    const int gp = PEA_LD_AGENT(parent + px);
    if (gp == px) { x = px; break; }
    PEA_ST_AGENT(parent + x, gp);
    x = gp;
  }
  M.root[base + p] = x;
  // has_con of a root that was hooked goes to its new root (every writer writes 1; the words that are read here belong to roots that
  // are none any more, the words that are written to roots that still are)
  if (x0 == (int)p && x != x0 && M.hascon[base + p]) M.hascon[base + x] = 1;
}

__global__ __launch_bounds__(kBlock) void k_mws_reinsert(const MwsParams P, const Mws M, int par) {
  size_t b;
  int k;
  unsigned p;
  const bool in = lattice_at(P, blockIdx.x, &b, &k, &p);
  u64* img = M.img + b * kImgWords;
  // (W_DONE may have been set by this round's compress: then nothing was alive and nothing merged)
  if (!img[F_MERGED + par]) return;
  if (in) {
    uint8_t* st = M.state + (b * P.K + k) * (size_t)P.S + p;
    if (*st == E_ACTIVE) {
      const int* __restrict__ root = M.root + b * P.S;
      const int ra = root[p], rb = root[(unsigned)((int)p + P.delta[k])];
      if (tab_claim(M.tab + b * P.cap, P.cap, pair_key1(ra, rb)) != 1) *st = E_DEAD;
    }
  }
}

// ---- the labelling ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_mws_first_init(const MwsParams P, const Mws M) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  if (blockIdx.x % P.chunks == 0) {  // the counters that the labelling takes start at 0
    u64* img = M.img + b * kImgWords;
    if (threadIdx.x == 0) img[W_VALID] = 0;
    if (threadIdx.x < PEA_MWS_MAX_K) { img[16 + threadIdx.x * kChanWords + C_UNDEC] = 0; img[16 + threadIdx.x * kChanWords + C_ACTIVE] = 0; }
  }
  if (in) M.first[b * P.S + p] = 0x7fffffff;
}
// the edges that are undecided and the active exclusions, per channel
__global__ __launch_bounds__(kBlock) void k_mws_count(const MwsParams P, const Mws M) {
  size_t b;
  int k;
  unsigned p;
  const bool in = edge_at(P, 0, P.K, &b, &k, &p);
  const int st = in ? M.state[(b * P.K + k) * (size_t)P.S + p] : E_DEAD;
  u64* ch = M.img + b * kImgWords + 16 + k * kChanWords;
  block_count4(ch + C_UNDEC, ch + C_ACTIVE, nullptr, nullptr, st == E_UNDECIDED, st == E_ACTIVE, false, false);
}
__global__ __launch_bounds__(kBlock) void k_mws_first(const MwsParams P, const Mws M, const uint8_t* __restrict__ mask) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  const int r = (in && (!mask || mask[b * P.S + p])) ? M.root[b * P.S + p] : -1;
  // of a run of lanes in one cluster the first lane holds the smallest pixel: it alone asks (clusters are mostly runs along x, and
  // thousands of lanes on one root's word are what this launch would otherwise wait for)
  const int left = __shfl_up(r, 1, 64);
  if (r < 0 || ((threadIdx.x & 63) && left == r)) return;
  int* f = M.first + b * P.S + r;
  if (PEA_LD_AGENT(f) > (int)p) atomicMin(f, (int)p);
}
__device__ __forceinline__ bool is_first(const MwsParams& P, const Mws& M, const uint8_t* __restrict__ mask, size_t b, unsigned p) {
  if (mask && !mask[b * P.S + p]) return false;
  return M.first[b * P.S + M.root[b * P.S + p]] == (int)p;
}
__global__ __launch_bounds__(kBlock) void k_mws_totals(const MwsParams P, const Mws M, const uint8_t* __restrict__ mask) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  const int valid = (in && (!mask || mask[b * P.S + p])) ? 1 : 0;
  int total;  // (two counts of at most 256 side by side)
  (void)block_scan_excl(((in && is_first(P, M, mask, b, p)) ? 1 : 0) | (valid << 16), &total);
  if (threadIdx.x == 0) {
    M.tot[blockIdx.x] = total & 0xffff;  // [b][chunk]
    if (total >> 16) PEA_ATOM_ADD(M.img + b * kImgWords + W_VALID, (u64)(total >> 16));
  }
}
// one workgroup per image walks its totals 256 at a time with a carry: tot becomes the exclusive prefix; counts[b]
__global__ __launch_bounds__(kBlock) void k_mws_scan(const MwsParams P, const Mws M, int32_t* __restrict__ counts) {
  int* tot = M.tot + (size_t)blockIdx.x * P.chunks;
  int carry = 0;
#pragma unroll 1
  for (unsigned base = 0; base < P.chunks; base += kBlock) {  // (uniform: every lane meets every barrier)
    const unsigned c = base + threadIdx.x;
    const int v = c < P.chunks ? tot[c] : 0;
    int total;
    const int ex = block_scan_excl(v, &total);
    if (c < P.chunks) tot[c] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}
__global__ __launch_bounds__(kBlock) void k_mws_rank(const MwsParams P, const Mws M, const uint8_t* __restrict__ mask) {
  size_t b;
  unsigned p;
  const bool in = pixel_at(P, &b, &p);
  const int f = (in && is_first(P, M, mask, b, p)) ? 1 : 0;
  int total;
  const int ex = block_scan_excl(f, &total);
  if (f) M.rank[b * P.S + p] = M.tot[blockIdx.x] + ex + 1;
}
__global__ __launch_bounds__(kBlock) void k_mws_write(const MwsParams P, const Mws M, const uint8_t* __restrict__ mask, int32_t* __restrict__ labels) {
  size_t b;
  unsigned p;
  if (!pixel_at(P, &b, &p)) return;
  const size_t i = b * P.S + p;
  labels[i] = (mask && !mask[i]) ? 0 : M.rank[b * P.S + M.first[b * P.S + M.root[i]]];
}
// a merge takes one cluster away, so the merges are the valid pixels less the clusters
__global__ __launch_bounds__(kBlock) void k_mws_stats(int B, const Mws M, const int32_t* __restrict__ counts, int32_t* __restrict__ stats) {
  const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (b >= B) return;
  const u64* img = M.img + (size_t)b * kImgWords;
  u64 sum[kChanWords] = {};
  for (int k = 0; k < PEA_MWS_MAX_K; ++k)
    for (int c = 0; c < kChanWords; ++c) sum[c] += img[16 + k * kChanWords + c];
  const u64 v[PEA_MWS_STATS] = {img[W_ROUNDS], sum[C_UNDEC], img[W_VALID] - (u64)counts[b], sum[C_ACTIVE], sum[C_STRIDE], sum[C_MASK], sum[C_NAN], sum[C_OUT]};
  for (int c = 0; c < PEA_MWS_STATS; ++c) stats[(size_t)b * PEA_MWS_STATS + c] = v[c] > 0x7fffffffull ? 0x7fffffff : (int32_t)v[c];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t mws_pixels(const PeaMwsDesc* d) { return mul_sat(mul_sat((uint64_t)d->Z, (uint64_t)d->Y), (uint64_t)d->X); }
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b ? 1 : 0); }
// slots of an image's table: a power of two, at least twice the repulsive edge slots that the strides admit (an active exclusion is a
// repulsive edge on the stride lattice), so a claim always finds room; UINT64_MAX where that does not fit
inline uint64_t mws_capacity(const PeaMwsDesc* d) {
  const uint64_t lattice = mul_sat(mul_sat(ceil_div(d->Z, d->strides[0]), ceil_div(d->Y, d->strides[1])), ceil_div(d->X, d->strides[2]));
  const uint64_t want = mul_sat(2 * (uint64_t)(d->K - d->n_attractive), lattice);
  if (want > (1ull << 62)) return UINT64_MAX;
  uint64_t cap = kMinCapacity;
  while (cap < want) cap <<= 1;
  return cap;
}
// the blocks in order, each a multiple of 8 bytes: root, par, first, rank (4 bytes a pixel), the totals of the scan (4 per 256 pixels),
// best (8 a pixel), the tables, 272 words per image, has_con (1 a pixel), the state bytes (K a pixel)
inline size_t mws_layout(const PeaMwsDesc* d, void* base, Mws* M) {
  const uint64_t B = (uint64_t)d->B, S = mws_pixels(d), per = mul_sat(B, S);
  Carver k(base);
  M->root = k.take<int>(per); M->par = k.take<int>(per); M->first = k.take<int>(per); M->rank = k.take<int>(per);
  M->tot = k.take<int>(mul_sat(B, ceil_div(S, kBlock)));
  M->best = k.take<u64>(per);
  M->tab = k.take<u64>(mul_sat(B, mws_capacity(d)));
  M->img = k.take<u64>(kImgWords * B);
  M->hascon = k.take<uint8_t>(per);
  M->state = k.take<uint8_t>(mul_sat(per, (uint64_t)d->K));
  return k.bytes();
}

}  // namespace

extern "C" int pea_mws_validate(const PeaMwsDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->flags & ~PEA_MWS_RESUME) return PEA_E_DESC;
  if (d->B < 1 || d->Z < 1 || d->Y < 1 || d->X < 1 || d->K < 1) return PEA_E_DESC;
  if (d->K > PEA_MWS_MAX_K) return PEA_E_DESC;
  if (d->n_attractive < 1 || d->n_attractive > d->K) return PEA_E_DESC;
  if (d->strides[0] < 1 || d->strides[1] < 1 || d->strides[2] < 1) return PEA_E_DESC;
  if (d->input != PEA_MWS_IN_AFFS && d->input != PEA_MWS_IN_ELF && d->input != PEA_MWS_IN_WEIGHTS) return PEA_E_DESC;
  if (d->rounds < 0 || d->rounds > PEA_MWS_MAX_ROUNDS) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" size_t pea_mws_workspace_bytes(const PeaMwsDesc* d) {
  Mws M;
  return pea_mws_validate(d) ? 0 : mws_layout(d, nullptr, &M);
}

extern "C" int pea_mws_segment(const PeaMwsDesc* d, const float* x, const uint8_t* mask, int32_t* labels, int32_t* counts, int32_t* stats,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_mws_validate(d);
  if (vrc) return vrc;
  if (!x || !labels || !counts || !stats) return PEA_E_NULL;
  const uint64_t S = mws_pixels(d);
  if (S >= (1ull << 31) || mul_sat(S, (uint64_t)d->K) >= (1ull << 32)) return PEA_E_UNSUPPORTED;
  MwsParams P;
  unsigned pix_groups, edge_groups;
  if (!stream_grid(S, (uint64_t)d->B, kBlock, &P.chunks, &pix_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid(S, (uint64_t)d->B * d->K, kBlock, &P.chunks, &edge_groups)) return PEA_E_UNSUPPORTED;
  if (misaligned(x, 4) || misaligned(labels, 4) || misaligned(counts, 4) || misaligned(stats, 4) || misaligned(workspace, 8)) return PEA_E_ALIGN;
  Mws M;
  if (!workspace || workspace_bytes < mws_layout(d, workspace, &M)) return PEA_E_WORKSPACE;

  P.B = d->B; P.Z = d->Z; P.Y = d->Y; P.X = d->X; P.K = d->K; P.nA = d->n_attractive;
  P.S = (unsigned)S;
  P.input = d->input;
  memset(P.off, 0, sizeof(P.off));
  memset(P.delta, 0, sizeof(P.delta));
  for (int k = 0; k < d->K; ++k) {
    // an offset that leaves the image on its own makes a channel without edges; its delta is never added (clamped so the product fits).
    // A step is copied clamped to [-extent, extent] of its axis: one at or past the extent is outside for every pixel either way, and
    // coordinate + step then fits an int in k_mws_init_edges whatever the caller wrote (2^31 - 1, -2^31).
    long long delta = 0;
    bool far = false;
    for (int a = 0; a < 3; ++a) {
      const int ext = a == 0 ? d->Z : (a == 1 ? d->Y : d->X);
      const int step = d->offsets[k][a];
      P.off[k][a] = step > ext ? ext : (step < -ext ? -ext : step);
      if (step >= ext || step <= -ext) far = true;
    }
    if (!far) delta = ((long long)d->offsets[k][0] * d->Y + d->offsets[k][1]) * d->X + d->offsets[k][2];
    P.delta[k] = (int)delta;
  }
  for (int a = 0; a < 3; ++a) P.stride[a] = d->strides[a];
  P.cap = mws_capacity(d);
  const uint64_t ext[3] = {(uint64_t)d->Z, (uint64_t)d->Y, (uint64_t)d->X};
  for (int a = 0; a < 3; ++a) P.lat[a] = (unsigned)ceil_div(ext[a], (uint64_t)d->strides[a]);
  P.lchunks = (unsigned)ceil_div((uint64_t)P.lat[0] * P.lat[1] * P.lat[2], kBlock);  // (at most S: fits)
  const unsigned attr_groups = P.attr_groups = (unsigned)((uint64_t)d->B * d->n_attractive * P.chunks);
  const unsigned rep_groups = (unsigned)((uint64_t)d->B * (d->K - d->n_attractive) * P.lchunks);  // (attr + rep <= edge_groups)
  const unsigned img_groups = (unsigned)((d->B + kBlock - 1) / kBlock);

  LaunchChain chain(stream);
  if (!(d->flags & PEA_MWS_RESUME)) {
    chain(k_mws_init_pix, pix_groups, kBlock, P, M);
    chain(k_mws_init_edges, edge_groups, kBlock, P, M, x, mask);
  } else if (d->rounds) {
    chain(k_mws_begin, img_groups, kBlock, d->B, M);
  }
  for (int k = 0; k < d->rounds && !chain.rc; ++k) {
    const int par = k & 1;
    chain(k_mws_best, attr_groups + rep_groups, kBlock, P, M, x, par);
    chain(k_mws_attr, attr_groups, kBlock, P, M, x, par);
    if (rep_groups) chain(k_mws_rep, rep_groups, kBlock, P, M, x, par);
    chain(k_mws_compress, pix_groups, kBlock, P, M, par);
    if (rep_groups) chain(k_mws_reinsert, rep_groups, kBlock, P, M, par);
  }
  chain(k_mws_first_init, pix_groups, kBlock, P, M);
  chain(k_mws_count, edge_groups, kBlock, P, M);
  chain(k_mws_first, pix_groups, kBlock, P, M, mask);
  chain(k_mws_totals, pix_groups, kBlock, P, M, mask);
  chain(k_mws_scan, (unsigned)d->B, kBlock, P, M, counts);
  chain(k_mws_rank, pix_groups, kBlock, P, M, mask);
  chain(k_mws_write, pix_groups, kBlock, P, M, mask, labels);
  chain(k_mws_stats, img_groups, kBlock, d->B, M, counts, stats);
  return chain.rc;
}
