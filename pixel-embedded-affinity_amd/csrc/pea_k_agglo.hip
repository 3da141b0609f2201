// pea_k_agglo.hip -- the hierarchical agglomeration of a fragment graph on the device (include/pea_agglo.h, which states the
// definition, the round rule and why it yields the sequential procedure's partition).  What the reference does on the host with
// waterz.agglomerate between the region adjacency graph and the projection.  All data are B independent images of N = max_id + 1 ids
// and two tables of `cap` slots of four words: (smaller root << 32 | larger root) + 1, and the payload -- MEAN: the low word, the high
// word and the count of the fixed-point sum; MIN: 0xFFFFFFFF - ord(score); MAX: ord(score), both combined by an integer max.  A
// workgroup of the slot kernels owns 256 consecutive slots of one image, of the id kernels 256 consecutive ids, of the row kernel 256
// consecutive input rows.  Every access is one element wide: any element-aligned pointer is served with the same result.
//
// set-up     k_agglo_init     root[i] = i, best = all ones, both tables and the image's words cleared, the record written
//            k_agglo_insert   the input rows into table 0 (rows that are no edge or refused for their value are counted)
// resumed    k_agglo_check    one lane holds the descriptor against the record and leaves the verdict in the header: every later launch of
//                             a refused call returns at once, the output launches write -1
//            k_agglo_begin    the round flags and the finished word of every image start at 0
// per round  k_agglo_best     best[A], best[B] of every live edge by a 64-bit atomic min; an edge below the threshold sets the round's
//                             ALIVE flag: a round that finds none sets the image's DONE word (k_agglo_flip), and every launch of a later
//                             round returns at once
//            k_agglo_merge    a live edge that is best[] of both its ends and below the threshold: root[larger] = smaller
//            k_agglo_compress best reset; after a merge an id whose root was hooked takes the new root (one hop: the merges are a
//                             matching) and the other table is cleared
//            k_agglo_rekey    after a merge: the live edges enter the other table under their new roots, parallel edges combine
//            k_agglo_flip     one lane per image closes the round's books: rounds, DONE, which table is current, the next round's flags
//            A round never reads what it writes inside one launch, except the table's slots in claims (one compare-and-swap each) and
//            best[] (min only).
// outputs    k_agglo_count    the live edges and those below the threshold
//            k_agglo_totals .. k_agglo_write   a flag on every root that is present, the flags' prefix over the ids (totals per 256 ids,
//            one workgroup per image scans them): the numbering in ascending root id; root and labels
//            k_agglo_stats
// Host: agglo_layout carves the workspace (pea_carve.h).
#include "../../include/pea_agglo.h"
#include "pea_segtable.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

constexpr int kSlotWords = 4;  // key + 1, payload 0 .. 2
constexpr int kImgWords = 16;
constexpr int kHdrWords = 8;
constexpr u64 kMagic = 0x50454141474c4f31ull;  // "PEAAGLO1"
constexpr u64 kMinCapacity = 64;
constexpr u64 kNone = ~0ull;
constexpr double kMaxAbs = 32768.0;          // 2^15
constexpr long long kMaxWeight = 1ll << 31;
enum { H_MAGIC = 0, H_B, H_MAX_ID, H_MAX_EDGES, H_LINKAGE, H_THRESHOLD, H_REFUSED };
// the flags come in pairs, used by the parity of the round's index in its call: round k sets [k & 1], k_agglo_flip clears [(k + 1) & 1]
enum { F_ALIVE = 0, F_MERGED = 2, W_DONE = 4, W_CUR, W_ROUNDS, W_MERGES, W_NO_EDGE, W_BAD_VALUE, W_LIVE, W_MERGEABLE, W_CLUSTERS };

struct AggloParams {
  int B, linkage;
  unsigned N;         // max_id + 1 <= 2^31 - 1
  unsigned ichunks;   // runs of 256 ids of an image
  unsigned schunks;   // runs of 256 slots of a table
  unsigned rchunks;   // runs of 256 rows of an image
  u64 cap;            // slots of a table: a power of two
  u64 max_edges;
  long long nstride;
  float thr;
  int ignore_zero;
};

struct Agglo {
  u64* hdr;   // [kHdrWords]
  u64* img;   // [B][kImgWords]
  u64* tab;   // [B][2][cap][kSlotWords]
  u64* best;  // [B][N] of a root: the smallest key of a live edge at the cluster this round; all ones between rounds
  int* root;  // [B][N]
  int* rank;  // [B][N] outputs: of a numbered root, its number
  int* tot;   // [B][ichunks] outputs: numbered roots per 256 ids, then their exclusive prefix
};

__device__ __forceinline__ u64* table_of(const AggloParams& P, const Agglo& M, size_t b, u64 which) {
  return M.tab + ((b * 2 + which) * P.cap) * kSlotWords;
}
// blockIdx -> (image, element of a range of n in runs of `chunks`); false: past the range
__device__ __forceinline__ bool at(unsigned chunks, u64 n, size_t* b, u64* i) {
  *b = blockIdx.x / chunks;
  *i = (u64)(blockIdx.x % chunks) * kBlock + threadIdx.x;
  return *i < n;
}
// a flag of the image: one lane per wave that has a reason stores 1 (every writer writes 1)
__device__ __forceinline__ void wave_flag(u64* w, bool mine) {
  if (__ballot(mine) && (threadIdx.x & 63) == 0) *w = 1;
}
__device__ __forceinline__ void wave_count(u64* w, bool mine) {
  const u64 n = (u64)__popcll(__ballot(mine));
  if (n && (threadIdx.x & 63) == 0) PEA_ATOM_ADD(w, n);
}
__device__ __forceinline__ u64 pair_key1(unsigned a, unsigned b) { return (((u64)a << 32) | (u64)b) + 1; }  // a < b
// the two words of a fixed-point sum -> its value, rounded to f64 once (pea_k_rag.hip fx_signed)
__device__ __forceinline__ double fx_signed(u64 lo, u64 hi) {
  const long long whole = (long long)hi + (long long)(lo >> 32);
  return (double)whole + (double)(lo & 0xffffffffull) / kFx;
}
// the score of a live slot (include/pea_agglo.h)
__device__ __forceinline__ float slot_score(int linkage, const u64* __restrict__ w) {
  if (linkage == PEA_AGGLO_MEAN) {
    const u64 cnt = w[3];
    return cnt ? (float)(fx_signed(w[1], w[2]) / (double)cnt) : __builtin_inff();
  }
  const unsigned o = (unsigned)w[1];
  return ord_f32(linkage == PEA_AGGLO_MIN ? 0xFFFFFFFFu - o : o);
}
__device__ __forceinline__ u64 score_word(int linkage, float score) {
  const unsigned o = f32_ord(score);
  return (u64)(linkage == PEA_AGGLO_MIN ? 0xFFFFFFFFu - o : o);
}

// The wave's edges (key1 != 0: this lane has one, payload p0 .. p2) enter `tab`, one update per (wave, key): the wave peels its keys,
// the lanes of a key combine their payloads by butterflies, the r-th key is kept by lane r, and the lanes then claim their slots side
// by side.  All 64 lanes call.  A claim cannot fail: the table has twice the slots of the edges that can be live.
__device__ __forceinline__ void wave_insert(int linkage, u64* __restrict__ tab, u64 cap, u64 key1, u64 p0, u64 p1, u64 p2) {
  const int lane = threadIdx.x & 63;
  const u64 key[kQuad] = {key1, 0, 0, 0};
  unsigned open = key1 ? 1u : 0u;
  u64 mykey = 0, m0 = 0, m1 = 0, m2 = 0;
  int r = 0;
  u64 cur;
  unsigned mm;
  while (peel(key, open, cur, mm)) {
    u64 s0, s1 = 0, s2 = 0;
    if (linkage == PEA_AGGLO_MEAN) {
      s0 = wave_sum(mm ? p0 : 0ull);
      s1 = wave_sum(mm ? p1 : 0ull);
      s2 = wave_sum(mm ? p2 : 0ull);
    } else {
      s0 = wave_max(mm ? p0 : 0ull);
    }
    if (lane == r) { mykey = cur; m0 = s0; m1 = s1; m2 = s2; }
    ++r;  // (one key per lane: at most 64 keys)
  }
  if (mykey) {
    const long long s = slot_claim<kSlotWords>(tab, cap, mykey);
    if (s >= 0) {
      u64* w = tab + (u64)s * kSlotWords;
      if (linkage == PEA_AGGLO_MEAN) {
        if (m0) PEA_ATOM_ADD(w + 1, m0);
        if (m1) PEA_ATOM_ADD(w + 2, m1);
        if (m2) PEA_ATOM_ADD(w + 3, m2);
      } else {
        PEA_ATOM_MAX(w + 1, m0);
      }
    }
  }
}

// ---- set-up ---------------------------------------------------------------------------------------------------------------------------
// grid: per image the runs of 256 of max(N, 2 * cap)
__global__ __launch_bounds__(kBlock) void k_agglo_init(const AggloParams P, const Agglo M, unsigned chunks) {
  const size_t b = blockIdx.x / chunks;
  const u64 i = (u64)(blockIdx.x % chunks) * kBlock + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    M.hdr[H_MAGIC] = kMagic; M.hdr[H_B] = (u64)P.B; M.hdr[H_MAX_ID] = (u64)P.N - 1; M.hdr[H_MAX_EDGES] = P.max_edges;
    M.hdr[H_LINKAGE] = (u64)P.linkage | ((u64)P.ignore_zero << 8); M.hdr[H_THRESHOLD] = (u64)f32_ord(P.thr); M.hdr[H_REFUSED] = 0;
    M.hdr[7] = 0;
  }
  if (blockIdx.x % chunks == 0 && threadIdx.x < kImgWords) M.img[b * kImgWords + threadIdx.x] = 0;
  if (i < 2 * P.cap) {
    u64* w = table_of(P, M, b, 0) + i * kSlotWords;  // (the two tables lie side by side)
    w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0;
  }
  if (i < P.N) {
    M.root[b * P.N + i] = (int)i;
    M.best[b * P.N + i] = kNone;
  }
}

__global__ __launch_bounds__(kBlock) void k_agglo_insert(const AggloParams P, const Agglo M, const PeaAggloBuffers io) {
  size_t b;
  u64 r;
  bool in = at(P.rchunks, P.max_edges, &b, &r);
  const long long ne = io.n_edges[(long long)b * P.nstride];
  in = in && (long long)r < ne;
  u64 key1 = 0, p0 = 0, p1 = 0, p2 = 0;
  bool no_edge = false, bad = false;
  if (in) {
    const size_t e = b * P.max_edges + r;
    const int u = io.uv[2 * e], v = io.uv[2 * e + 1];
    if (u >= v || u < 0 || (unsigned)v >= P.N || (P.ignore_zero && u == 0)) no_edge = true;
    else {
      const double val = io.value[e];
      if (!(__builtin_fabs(val) <= kMaxAbs)) bad = true;
      else if (P.linkage == PEA_AGGLO_MEAN) {
        const long long wt = io.weight[e];
        if (wt < 0 || wt > kMaxWeight) bad = true;
        else {
          const double p = val * (double)wt;
          const double whole = __builtin_floor(p);
          p0 = (u64)((p - whole) * kFx);
          p1 = (u64)(long long)whole;
          p2 = (u64)wt;
        }
      } else {
        p0 = score_word(P.linkage, (float)val);
      }
      if (!bad) key1 = pair_key1((unsigned)u, (unsigned)v);
    }
  }
  wave_insert(P.linkage, table_of(P, M, b, 0), P.cap, key1, p0, p1, p2);
  u64* img = M.img + b * kImgWords;
  wave_count(img + W_NO_EDGE, no_edge);
  wave_count(img + W_BAD_VALUE, bad);
}

// a resumed call against the record of the set-up; the threshold of the record rises to this call's
__global__ void k_agglo_check(const AggloParams P, const Agglo M) {
  if (blockIdx.x || threadIdx.x) return;
  const bool ok = M.hdr[H_MAGIC] == kMagic && M.hdr[H_B] == (u64)P.B && M.hdr[H_MAX_ID] == (u64)P.N - 1 && M.hdr[H_MAX_EDGES] == P.max_edges &&
                  M.hdr[H_LINKAGE] == ((u64)P.linkage | ((u64)P.ignore_zero << 8)) && M.hdr[H_THRESHOLD] <= (u64)f32_ord(P.thr);
  M.hdr[H_REFUSED] = ok ? 0 : 1;
  if (ok) M.hdr[H_THRESHOLD] = (u64)f32_ord(P.thr);
}
__global__ __launch_bounds__(kBlock) void k_agglo_begin(int B, const Agglo M) {
  const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (b >= B || M.hdr[H_REFUSED]) return;
  u64* img = M.img + (size_t)b * kImgWords;
  img[F_ALIVE] = 0; img[F_ALIVE + 1] = 0; img[F_MERGED] = 0; img[F_MERGED + 1] = 0; img[W_DONE] = 0;
}

// ---- a round ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_agglo_best(const AggloParams P, const Agglo M, int par) {
  size_t b;
  u64 s;
  const bool in = at(P.schunks, P.cap, &b, &s);
  u64* img = M.img + b * kImgWords;
  if (M.hdr[H_REFUSED] || img[W_DONE]) return;
  bool alive = false;
  if (in) {
    const u64* w = table_of(P, M, b, img[W_CUR]) + s * kSlotWords;
    const u64 key1 = w[0];
    if (key1) {
      const unsigned A = (unsigned)((key1 - 1) >> 32), Bq = (unsigned)(key1 - 1);
      const float score = slot_score(P.linkage, w);
      const u64 hi = (u64)f32_ord(score) << 32;
      u64* best = M.best + b * P.N;
      // (a stale larger value only costs an atomic that changes nothing: best only falls inside the launch)
      if (PEA_LD_AGENT(best + A) > (hi | Bq)) (void)__hip_atomic_fetch_min(best + A, hi | Bq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (PEA_LD_AGENT(best + Bq) > (hi | A)) (void)__hip_atomic_fetch_min(best + Bq, hi | A, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      alive = score < P.thr;
    }
  }
  wave_flag(img + F_ALIVE + par, alive);
}

__global__ __launch_bounds__(kBlock) void k_agglo_merge(const AggloParams P, const Agglo M, int par) {
  size_t b;
  u64 s;
  const bool in = at(P.schunks, P.cap, &b, &s);
  u64* img = M.img + b * kImgWords;
  if (M.hdr[H_REFUSED] || img[W_DONE] || !img[F_ALIVE + par]) return;
  bool merged = false;
  if (in) {
    const u64* w = table_of(P, M, b, img[W_CUR]) + s * kSlotWords;
    const u64 key1 = w[0];
    if (key1) {
      const unsigned A = (unsigned)((key1 - 1) >> 32), Bq = (unsigned)(key1 - 1);
      const float score = slot_score(P.linkage, w);
      const u64 hi = (u64)f32_ord(score) << 32;
      if (score < P.thr && M.best[b * P.N + A] == (hi | Bq) && M.best[b * P.N + Bq] == (hi | A)) {
        M.root[b * P.N + Bq] = (int)A;  // one writer: a cluster has one best
        merged = true;
      }
    }
  }
  wave_flag(img + F_MERGED + par, merged);
  wave_count(img + W_MERGES, merged);
}

// grid: per image the runs of 256 of max(N, cap)
__global__ __launch_bounds__(kBlock) void k_agglo_compress(const AggloParams P, const Agglo M, unsigned chunks, int par) {
  const size_t b = blockIdx.x / chunks;
  const u64 i = (u64)(blockIdx.x % chunks) * kBlock + threadIdx.x;
  const u64* img = M.img + b * kImgWords;
  if (M.hdr[H_REFUSED] || img[W_DONE] || !img[F_ALIVE + par]) return;  // (nothing alive: the image is finished; k_agglo_reset puts best[] back)
  const bool merged = img[F_MERGED + par] != 0;
  if (merged && i < P.cap) {
    u64* w = table_of(P, M, b, img[W_CUR] ^ 1) + i * kSlotWords;
    w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0;
  }
  if (i >= P.N) return;
  M.best[b * P.N + i] = kNone;
  if (!merged) return;
  // One hop.  A word that is read here as a root's (root[r], r a root when the round began) is written by k_agglo_merge alone; the words
  // written here belong to ids that were no roots.
  int* root = M.root + b * P.N;
  const int r = root[i];
  if (r != (int)i) {
    const int rr = root[r];
    if (rr != r) root[i] = rr;
  }
}

__global__ __launch_bounds__(kBlock) void k_agglo_rekey(const AggloParams P, const Agglo M, int par) {
  size_t b;
  u64 s;
  const bool in = at(P.schunks, P.cap, &b, &s);
  const u64* img = M.img + b * kImgWords;
  if (M.hdr[H_REFUSED] || img[W_DONE] || !img[F_MERGED + par]) return;
  u64 key1 = 0, p0 = 0, p1 = 0, p2 = 0;
  if (in) {
    const u64* w = table_of(P, M, b, img[W_CUR]) + s * kSlotWords;
    if (w[0]) {
      const int* __restrict__ root = M.root + b * P.N;
      const unsigned a = (unsigned)root[(unsigned)((w[0] - 1) >> 32)], c = (unsigned)root[(unsigned)(w[0] - 1)];
      if (a != c) {
        key1 = pair_key1(a < c ? a : c, a < c ? c : a);
        p0 = w[1]; p1 = w[2]; p2 = w[3];
      }
    }
  }
  wave_insert(P.linkage, table_of(P, M, b, img[W_CUR] ^ 1), P.cap, key1, p0, p1, p2);
}

__global__ __launch_bounds__(kBlock) void k_agglo_flip(int B, const Agglo M, int par) {
  const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (b >= B || M.hdr[H_REFUSED]) return;
  u64* img = M.img + (size_t)b * kImgWords;
  if (img[W_DONE]) return;
  if (!img[F_ALIVE + par]) img[W_DONE] = 1;  // (k_agglo_best lowered best[] for the live edges at or above the threshold: k_agglo_reset)
  if (img[F_MERGED + par]) { img[W_ROUNDS] += 1; img[W_CUR] ^= 1; }
  img[F_ALIVE + (par ^ 1)] = 0; img[F_MERGED + (par ^ 1)] = 0;
}

// ---- the outputs ------------------------------------------------------------------------------------------------------------------------
// the counters that the outputs take start at 0; best[] back to all ones (a round that found nothing below the threshold left it
// lowered, and a resumed call with a higher threshold reads it)
__global__ __launch_bounds__(kBlock) void k_agglo_reset(const AggloParams P, const Agglo M) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  if (M.hdr[H_REFUSED]) return;
  if (blockIdx.x % P.ichunks == 0 && threadIdx.x == 0) {
    u64* img = M.img + b * kImgWords;
    img[W_LIVE] = 0; img[W_MERGEABLE] = 0;
  }
  if (in) M.best[b * P.N + i] = kNone;
}
__global__ __launch_bounds__(kBlock) void k_agglo_count(const AggloParams P, const Agglo M) {
  size_t b;
  u64 s;
  const bool in = at(P.schunks, P.cap, &b, &s);
  if (M.hdr[H_REFUSED]) return;
  u64* img = M.img + b * kImgWords;
  bool live = false, below = false;
  if (in) {
    const u64* w = table_of(P, M, b, img[W_CUR]) + s * kSlotWords;
    if (w[0]) {
      live = true;
      below = slot_score(P.linkage, w) < P.thr;
    }
  }
  wave_count(img + W_LIVE, live);
  wave_count(img + W_MERGEABLE, below);
}
__device__ __forceinline__ bool present(const AggloParams& P, const int64_t* __restrict__ node_size, size_t b, u64 i) {
  if (P.ignore_zero && i == 0) return false;
  return !node_size || node_size[b * P.N + i] > 0;
}
__global__ __launch_bounds__(kBlock) void k_agglo_totals(const AggloParams P, const Agglo M, const int64_t* __restrict__ node_size) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  if (M.hdr[H_REFUSED]) return;
  const int f = (in && M.root[b * P.N + i] == (int)i && present(P, node_size, b, i)) ? 1 : 0;
  int total;
  (void)block_scan_excl(f, &total);
  if (threadIdx.x == 0) M.tot[blockIdx.x] = total;  // [b][chunk]
}
// one workgroup per image walks its totals 256 at a time with a carry: tot becomes the exclusive prefix
__global__ __launch_bounds__(kBlock) void k_agglo_scan(const AggloParams P, const Agglo M) {
  if (M.hdr[H_REFUSED]) return;
  int* tot = M.tot + (size_t)blockIdx.x * P.ichunks;
  int carry = 0;
#pragma unroll 1
  for (unsigned base = 0; base < P.ichunks; base += kBlock) {  // (uniform: every lane meets every barrier)
    const unsigned c = base + threadIdx.x;
    const int v = c < P.ichunks ? tot[c] : 0;
    int total;
    const int ex = block_scan_excl(v, &total);
    if (c < P.ichunks) tot[c] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) M.img[(size_t)blockIdx.x * kImgWords + W_CLUSTERS] = (u64)carry;
}
__global__ __launch_bounds__(kBlock) void k_agglo_rank(const AggloParams P, const Agglo M, const int64_t* __restrict__ node_size) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  if (M.hdr[H_REFUSED]) return;
  const int f = (in && M.root[b * P.N + i] == (int)i && present(P, node_size, b, i)) ? 1 : 0;
  int total;
  const int ex = block_scan_excl(f, &total);
  if (in) M.rank[b * P.N + i] = f ? M.tot[blockIdx.x] + ex + 1 : 0;
}
__global__ __launch_bounds__(kBlock) void k_agglo_write(const AggloParams P, const Agglo M, const PeaAggloBuffers io) {
  size_t b;
  u64 i;
  if (!at(P.ichunks, P.N, &b, &i)) return;
  const size_t o = b * P.N + i;
  if (M.hdr[H_REFUSED]) {
    io.root[o] = -1;
    if (io.labels) io.labels[o] = -1;
    return;
  }
  const int r = M.root[o];
  io.root[o] = r;
  if (io.labels) io.labels[o] = present(P, io.node_size, b, i) ? M.rank[b * P.N + (unsigned)r] : 0;
}
__global__ __launch_bounds__(kBlock) void k_agglo_stats(int B, const Agglo M, const PeaAggloBuffers io) {
  const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (b >= B) return;
  int64_t* st = io.stats + (size_t)b * PEA_AGGLO_STATS;
  if (M.hdr[H_REFUSED]) {
    for (int c = 0; c < PEA_AGGLO_STATS; ++c) st[c] = -1;
    if (io.counts) io.counts[b] = -1;
    return;
  }
  const u64* img = M.img + (size_t)b * kImgWords;
  st[PEA_AGGLO_ROUNDS] = (int64_t)img[W_ROUNDS];
  st[PEA_AGGLO_LIVE] = (int64_t)img[W_LIVE];
  st[PEA_AGGLO_MERGEABLE] = (int64_t)img[W_MERGEABLE];
  st[PEA_AGGLO_MERGES] = (int64_t)img[W_MERGES];
  st[PEA_AGGLO_CLUSTERS] = (int64_t)img[W_CLUSTERS];
  st[PEA_AGGLO_NO_EDGE] = (int64_t)img[W_NO_EDGE];
  st[PEA_AGGLO_BAD_VALUE] = (int64_t)img[W_BAD_VALUE];
  st[7] = 0;
  if (io.counts) io.counts[b] = (int32_t)img[W_CLUSTERS];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b ? 1 : 0); }
// slots of a table: the power of two >= max(64, 2 * max_edges): a claim always finds room
inline uint64_t agglo_capacity(const PeaAggloDesc* d) {
  uint64_t cap = kMinCapacity;
  while (cap < 2 * (uint64_t)d->max_edges) cap <<= 1;
  return cap;
}
// the blocks in order, each a multiple of 8 bytes: the header, 16 words per image, the two tables, best (8 bytes an id), root, rank (4
// an id), the totals of the scan (4 per 256 ids)
inline size_t agglo_layout(const PeaAggloDesc* d, void* base, Agglo* M) {
  const uint64_t B = (uint64_t)d->B, N = (uint64_t)d->max_id + 1, per = mul_sat(B, N);
  Carver k(base);
  M->hdr = k.take<u64>(kHdrWords);
  M->img = k.take<u64>(kImgWords * B);
  M->tab = k.take<u64>(mul_sat(mul_sat(B, 2 * kSlotWords), agglo_capacity(d)));
  M->best = k.take<u64>(per);
  M->root = k.take<int>(per);
  M->rank = k.take<int>(per);
  M->tot = k.take<int>(mul_sat(B, ceil_div(N, kBlock)));
  return k.bytes();
}

}  // namespace

extern "C" int pea_agglo_validate(const PeaAggloDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->flags & ~(PEA_AGGLO_RESUME | PEA_AGGLO_IGNORE_ZERO)) return PEA_E_DESC;
  if (d->B < 1) return PEA_E_DESC;
  if (d->max_id < 0 || d->max_id > 0x7ffffffe) return PEA_E_DESC;
  if (d->max_edges < 1 || d->max_edges > PEA_AGGLO_MAX_EDGES) return PEA_E_DESC;
  if (d->n_edges_stride < 0) return PEA_E_DESC;
  if (d->linkage != PEA_AGGLO_MEAN && d->linkage != PEA_AGGLO_MIN && d->linkage != PEA_AGGLO_MAX) return PEA_E_DESC;
  if (d->threshold != d->threshold) return PEA_E_DESC;
  if (d->rounds < 0 || d->rounds > PEA_AGGLO_MAX_ROUNDS) return PEA_E_DESC;
  return PEA_OK;
}

extern "C" size_t pea_agglo_workspace_bytes(const PeaAggloDesc* d) {
  Agglo M;
  return pea_agglo_validate(d) ? 0 : agglo_layout(d, nullptr, &M);
}

extern "C" int pea_agglo_merge(const PeaAggloDesc* d, const PeaAggloBuffers* io, void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_agglo_validate(d);
  if (vrc) return vrc;
  if (!io || !io->uv || !io->n_edges || !io->value || !io->root || !io->stats) return PEA_E_NULL;
  if (d->linkage == PEA_AGGLO_MEAN && !io->weight) return PEA_E_NULL;
  if (!io->labels != !io->counts) return PEA_E_NULL;
  AggloParams P;
  const uint64_t N = (uint64_t)d->max_id + 1;
  P.cap = agglo_capacity(d);
  unsigned id_groups, slot_groups, row_groups, wide_groups, wide_chunks, init_groups, init_chunks;
  if (!stream_grid(N, (uint64_t)d->B, kBlock, &P.ichunks, &id_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid(P.cap, (uint64_t)d->B, kBlock, &P.schunks, &slot_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid((uint64_t)d->max_edges, (uint64_t)d->B, kBlock, &P.rchunks, &row_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid(N > P.cap ? N : P.cap, (uint64_t)d->B, kBlock, &wide_chunks, &wide_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid(N > 2 * P.cap ? N : 2 * P.cap, (uint64_t)d->B, kBlock, &init_chunks, &init_groups)) return PEA_E_UNSUPPORTED;
  if (misaligned(io->uv, 4) || misaligned(io->root, 4) || misaligned(io->labels, 4) || misaligned(io->counts, 4) || misaligned(io->n_edges, 8) ||
      misaligned(io->value, 8) || misaligned(io->weight, 8) || misaligned(io->node_size, 8) || misaligned(io->stats, 8) || misaligned(workspace, 8))
    return PEA_E_ALIGN;
  Agglo M;
  if (!workspace || workspace_bytes < agglo_layout(d, workspace, &M)) return PEA_E_WORKSPACE;

  P.B = d->B; P.linkage = d->linkage; P.N = (unsigned)N;
  P.max_edges = (u64)d->max_edges; P.nstride = (long long)d->n_edges_stride;
  P.thr = d->threshold; P.ignore_zero = (d->flags & PEA_AGGLO_IGNORE_ZERO) ? 1 : 0;
  const unsigned img_groups = (unsigned)((d->B + kBlock - 1) / kBlock);

  LaunchChain chain(stream);
  if (!(d->flags & PEA_AGGLO_RESUME)) {
    chain(k_agglo_init, init_groups, kBlock, P, M, init_chunks);
    chain(k_agglo_insert, row_groups, kBlock, P, M, *io);
  } else {
    chain(k_agglo_check, 1, 64, P, M);
    chain(k_agglo_begin, img_groups, kBlock, d->B, M);
  }
  for (int k = 0; k < d->rounds && !chain.rc; ++k) {
    const int par = k & 1;
    chain(k_agglo_best, slot_groups, kBlock, P, M, par);
    chain(k_agglo_merge, slot_groups, kBlock, P, M, par);
    chain(k_agglo_compress, wide_groups, kBlock, P, M, wide_chunks, par);
    chain(k_agglo_rekey, slot_groups, kBlock, P, M, par);
    chain(k_agglo_flip, img_groups, kBlock, d->B, M, par);
  }
  chain(k_agglo_reset, id_groups, kBlock, P, M);
  chain(k_agglo_count, slot_groups, kBlock, P, M);
  chain(k_agglo_totals, id_groups, kBlock, P, M, io->node_size);
  chain(k_agglo_scan, (unsigned)d->B, kBlock, P, M);
  chain(k_agglo_rank, id_groups, kBlock, P, M, io->node_size);
  chain(k_agglo_write, id_groups, kBlock, P, M, *io);
  chain(k_agglo_stats, img_groups, kBlock, d->B, M, *io);
  return chain.rc;
}
