// pea_k_merge.hip -- the small-segment merges and the renumbering on the device (include/pea_merge.h, which states the definition and
// the tie rule).  What the reference does on the host with merge_small_object / merge_func / relabel between seg_mutex and the scores.
// All data are B independent images of S = Y * X pixels and N = max_id + 1 ids.  The image is never rewritten: alias[i] is the id that
// the pixels of i carry now (a chain that ends in a root, alias[r] == r), and cnt / sr / sc of a root are the pixel count, row sum and
// column sum of everything that carries it.  Every access is one element wide or checks its alignment: any element-aligned pointer is
// served with the same result.
//
// moments    k_merge_init      cnt = sr = sc = 0, alias[i] = i, the image's words cleared
//            k_merge_moments   one streaming pass: a wave owns 256 consecutive pixels, peels its ids (pea_stream.h) and sends one integer
//                              atomic per (wave, id) and moment; pixels whose id is outside [0, max_id] are counted
// walk       k_merge_walk      ONE WORKGROUP PER IMAGE.  Per pass: a ballot over the ids' sizes at the start of the pass leaves the
//                              candidates (0 < size <= threshold) as a bit per id; the words of 64 ids are walked 256 at a time and
//                              the candidates served in ascending order.  Per candidate: the
//                              centroid from the root's moments, the lanes stride over the crop, each resolves its pixel's alias by a
//                              find bounded by N and counts into an LDS open-addressing table (key ~id, claimed by one compare-and-swap);
//                              three 64-bit maxima over the slots of count << 32 | ~id give the top entry, the best that is not 0 and the
//                              best that is neither 0 nor the candidate; lane 0 commits the merge; a barrier.  Between passes all aliases
//                              are compressed in parallel.  The workgroup's waves hand alias and the moments to each other through
//                              relaxed agent-scope accesses (served by the L2, never by the CU's L1) with every store drained before
//                              the barrier that publishes it.  No workgroup waits for another.
// finish     k_merge_totals    root[i] = find(i); a flag on every id above 0 that has pixels; totals per 256 ids
//            k_merge_scan      one workgroup per image: the exclusive prefix of the totals; counts[b]
//            k_merge_rank      rank[i] = the flag's prefix + 1 (0 without the flag): ascending id order
//            k_merge_map       PEA_MERGE_RELABEL only: root[i] = rank[root[i]]
//            k_merge_project   one streaming pass: out[p] = root[seg[p]], ids outside [0, max_id] written through
// Host: merge_layout carves the workspace (pea_carve.h).
#include "../../include/pea_merge.h"
#include "pea_stream.h"

using namespace pea;

namespace {

constexpr int kImgWords = 8;
constexpr int kLook = 4;      // loads that a lane of the walk keeps in flight where it streams over the ids
constexpr int kSlots = 4096;  // >= 2 * PEA_MERGE_MAX_WINDOW^2: a claim always finds room
static_assert(2 * PEA_MERGE_MAX_WINDOW * PEA_MERGE_MAX_WINDOW <= kSlots, "the crop's id table holds every pixel of the largest window twice over");
enum { W_BAD = 0 };

struct MergeParams {
  int B, Y, X;
  unsigned N;        // max_id + 1 <= 2^31 - 1
  size_t S;          // Y * X < 2^31
  unsigned pchunks;  // runs of 1024 pixels of an image
  unsigned ichunks;  // runs of 256 ids of an image
  unsigned wchunks;  // words of 64 ids of an image
  int n_passes, relabel;
  int thr[PEA_MERGE_MAX_PASSES], win[PEA_MERGE_MAX_PASSES];
};

struct MergeWs {
  u64* img;           // [B][kImgWords]
  u64 *cnt, *sr, *sc; // [B][N] of a root: pixels, row sum, column sum of what carries it now; 0 of an id that was merged away
  int* alias;         // [B][N]
  u64* bits;          // [B][wchunks] the walk: the candidates of the pass, a bit per id
  int* root;          // [B][N] the finish: the id that an id's pixels carry at the end, then the output map
  int* rank;          // [B][N] of an id above 0 with pixels: its number
  int* tot;           // [B][ichunks] numbered ids per 256 ids, then their exclusive prefix
};

// blockIdx -> (image, element of a range of n in runs of `chunks`); false: past the range
__device__ __forceinline__ bool at(unsigned chunks, u64 n, size_t* b, u64* i) {
  *b = blockIdx.x / chunks;
  *i = (u64)(blockIdx.x % chunks) * kBlock + threadIdx.x;
  return *i < n;
}

// the id that the pixels of v carry now; *hops: the links followed.  alias only ever moves toward its root, so the loop ends at a root
// whatever another lane compresses meanwhile; N bounds it regardless of the workspace's contents.
__device__ __forceinline__ int find_root(int* __restrict__ alias, int v, unsigned N, int* hops) {
  int h = 0;
  for (unsigned k = 0; k < N; ++k) {
    const int a = PEA_LD_AGENT(alias + v);
    if (a == v || (unsigned)a >= N) break;
    v = a;
    ++h;
  }
  *hops = h;
  return v;
}

// ---- moments ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_merge_init(const MergeParams P, const MergeWs M) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  if (blockIdx.x % P.ichunks == 0 && threadIdx.x < kImgWords) M.img[b * kImgWords + threadIdx.x] = 0;
  if (!in) return;
  const size_t o = b * P.N + i;
  M.cnt[o] = 0; M.sr[o] = 0; M.sc[o] = 0;
  M.alias[o] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_merge_moments(const MergeParams P, const MergeWs M, const int32_t* __restrict__ seg) {
  const BlockAt where = block_at(P.pchunks);
  const size_t b = where.plane;
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(where.chunk, P.S, &w0)) return;
  const size_t i0 = w0 + (size_t)lane * kQuad;
  const int nv = quad_nv(i0, P.S);
  int v[kQuad];
  ld_iquad(seg + b * P.S + (nv ? i0 : 0), nv, -1, v);
  unsigned key[kQuad], row[kQuad], col[kQuad];
  unsigned open = 0;
  u64 bad = 0;
  unsigned y = nv ? (unsigned)(i0 / (unsigned)P.X) : 0, x = nv ? (unsigned)(i0 - (size_t)y * (unsigned)P.X) : 0;
#pragma unroll
  for (int e = 0; e < kQuad; ++e) {
    key[e] = (unsigned)v[e]; row[e] = y; col[e] = x;
    if (e < nv) {
      if ((unsigned)v[e] < P.N) open |= 1u << e;
      else ++bad;
    }
    if (++x == (unsigned)P.X) { x = 0; ++y; }
  }
  u64* cnt = M.cnt + b * P.N;
  u64* sr = M.sr + b * P.N;
  u64* sc = M.sc + b * P.N;
  unsigned myid = 0;
  u64 myn = 0, myr = 0, myc = 0;
  const auto flush = [&]() {  // every lane that holds a peeled id adds its three moments
    if (myn) {
      PEA_ATOM_ADD(cnt + myid, myn);
      if (myr) PEA_ATOM_ADD(sr + myid, myr);
      if (myc) PEA_ATOM_ADD(sc + myid, myc);
    }
    myn = 0;
  };
  int r = 0;
  unsigned cur, mm;
  while (peel(key, open, cur, mm)) {
    u64 n = 0, rs = 0, cs = 0;
#pragma unroll
    for (int e = 0; e < kQuad; ++e)
      if ((mm >> e) & 1u) { ++n; rs += row[e]; cs += col[e]; }
    n = wave_sum(n); rs = wave_sum(rs); cs = wave_sum(cs);
    if (lane == r) { myid = cur; myn = n; myr = rs; myc = cs; }
    if (++r == 64) { flush(); r = 0; }
  }
  flush();
  bad = wave_sum(bad);
  if (lane == 0 && bad) PEA_ATOM_ADD(M.img + b * kImgWords + W_BAD, bad);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// every store of this wave has left for the L2 before the barrier lets another wave read it
__device__ __forceinline__ void wg_publish() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_merge_walk(const MergeParams P, const MergeWs M, const int32_t* __restrict__ seg, int64_t* __restrict__ stats) {
  __shared__ unsigned s_key[kSlots], s_cnt[kSlots];  // ~id (0: empty) and its pixels in the crop
  __shared__ u64 s_word[2][kBlock];  // the step's 256 candidate words, and which of them are not 0
  __shared__ u64 s_ball[2][kBlock / 64];
  __shared__ u64 s_red[kBlock / 64][4];
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned N = P.N;
  u64* cnt = M.cnt + b * N;
  u64* sr = M.sr + b * N;
  u64* sc = M.sc + b * N;
  int* alias = M.alias + b * N;
  u64* bits = M.bits + b * P.wchunks;
  const unsigned nwords = P.wchunks;
  const int32_t* __restrict__ img = seg + b * P.S;
  u64 looked = 0, merges = 0, negative = 0, few = 0;  // uniform over the workgroup
  int chain = 0;                                      // the lane's own

#pragma unroll 1
  for (int p = 0; p < P.n_passes; ++p) {
    const int thr = P.thr[p], win = P.win[p], half = win / 2;
    unsigned cap = 64;
    while (cap < 2u * (unsigned)(win * win)) cap <<= 1;
    // the candidates of the pass, judged by the sizes at its start: a bit per id (kLook loads in flight per lane)
#pragma unroll 1
    for (unsigned base = 0; base < N; base += kLook * kBlock) {  // (uniform: every lane meets every ballot)
      u64 n[kLook];
#pragma unroll
      for (int k = 0; k < kLook; ++k) {
        const unsigned i = base + (unsigned)k * kBlock + tid;
        n[k] = i < N ? PEA_LD_AGENT(cnt + i) : 0;
      }
#pragma unroll
      for (int k = 0; k < kLook; ++k) {
        const unsigned first = base + (unsigned)k * kBlock + (unsigned)wave * 64;  // the wave's 64 ids are one word
        const u64 ballot = __ballot(n[k] > 0 && n[k] <= (u64)thr);
        if (lane == 0 && first < N) PEA_ST_AGENT(bits + first / 64, ballot);
      }
    }
    wg_publish();
    unsigned par = 0;
#pragma unroll 1
    for (unsigned wb = 0; wb < nwords; wb += kBlock, par ^= 1) {  // 256 words = 16384 ids a step (uniform: every lane meets every barrier)
      const unsigned mine = wb + tid;
      const u64 word = mine < nwords ? PEA_LD_AGENT(bits + mine) : 0;
      s_word[par][tid] = word;
      const u64 ballot = __ballot(word != 0);
      if (lane == 0) s_ball[par][wave] = ballot;
      __syncthreads();
#pragma unroll 1
      for (int w = 0; w < kBlock / 64; ++w) {
        u64 words = s_ball[par][w];
#pragma unroll 1
        while (words) {
          const unsigned at_word = (unsigned)w * 64 + (unsigned)(__ffsll((unsigned long long)words) - 1);
          words &= words - 1;
          u64 todo = s_word[par][at_word];
#pragma unroll 1
          while (todo) {
            const unsigned i = (wb + at_word) * 64 + (unsigned)(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1;
            // -- the candidate i: every lane walks the same path up to the crop
            const u64 n = PEA_LD_AGENT(cnt + i);
            if (!n) continue;  // (cannot happen: pixels leave an id only when it is served)
            ++looked;
            const u64 rs = PEA_LD_AGENT(sr + i), cs = PEA_LD_AGENT(sc + i);
            const int r0 = (int)(rs / n) - half, c0 = (int)(cs / n) - half;
            if (r0 < 0 || c0 < 0) { ++negative; continue; }
            const int r1 = r0 + win < P.Y ? r0 + win : P.Y, c1 = c0 + win < P.X ? c0 + win : P.X;
            const int cw = c1 - c0, area = (r1 - r0) * cw;
            for (unsigned s = tid; s < cap; s += kBlock) { s_key[s] = 0; s_cnt[s] = 0; }
            __syncthreads();
            for (int q = tid; q < area; q += kBlock) {
              const int rr = r0 + q / cw, cc = c0 + q % cw;
              const int v = img[(size_t)rr * (unsigned)P.X + (unsigned)cc];
              if ((unsigned)v >= N) continue;
              int hops;
              const unsigned root = (unsigned)find_root(alias, v, N, &hops);
              chain = hops > chain ? hops : chain;
              const unsigned key = ~root;
              unsigned s = ((root * 0x9E3779B1u) >> 20) & (cap - 1);
              for (unsigned k = 0; k < cap; ++k) {  // (the table has twice the slots of the crop's pixels: a claim finds room)
                const unsigned old = atomicCAS(&s_key[s], 0u, key);
                if (old == 0u || old == key) { atomicAdd(&s_cnt[s], 1u); break; }
                s = (s + 1) & (cap - 1);
              }
            }
            __syncthreads();
            u64 m0 = 0, m1 = 0, m2 = 0, distinct = 0;  // the best entry; .. that is not id 0; .. that is neither 0 nor i
            for (unsigned s = tid; s < cap; s += kBlock) {
              const unsigned key = s_key[s];
              if (!key) continue;
              const u64 e = ((u64)s_cnt[s] << 32) | key;  // more pixels first, then the larger ~id: the smaller id
              ++distinct;
              m0 = e > m0 ? e : m0;
              if (key != ~0u) {
                m1 = e > m1 ? e : m1;
                if (key != ~i) m2 = e > m2 ? e : m2;
              }
            }
            m0 = wave_max(m0); m1 = wave_max(m1); m2 = wave_max(m2); distinct = wave_sum(distinct);
            if (lane == 0) { s_red[wave][0] = m0; s_red[wave][1] = m1; s_red[wave][2] = m2; s_red[wave][3] = distinct; }
            __syncthreads();
            m0 = 0; m1 = 0; m2 = 0; distinct = 0;
#pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) {
              m0 = s_red[k][0] > m0 ? s_red[k][0] : m0;
              m1 = s_red[k][1] > m1 ? s_red[k][1] : m1;
              m2 = s_red[k][2] > m2 ? s_red[k][2] : m2;
              distinct += s_red[k][3];
            }
            if (distinct <= 2) { ++few; continue; }
            const unsigned id0 = ~(unsigned)m0, id1 = ~(unsigned)m1, id2 = ~(unsigned)m2;
            const unsigned target = id0 != 0 ? id0 : (id1 == i ? id2 : id1);  // (three or more ids, one of them 0: m1 and m2 exist)
            if (target != i && target < N) {
              ++merges;
              if (tid == 0) {
                PEA_ST_AGENT(alias + i, (int)target);
                PEA_ST_AGENT(cnt + target, PEA_LD_AGENT(cnt + target) + n);
                PEA_ST_AGENT(sr + target, PEA_LD_AGENT(sr + target) + rs);
                PEA_ST_AGENT(sc + target, PEA_LD_AGENT(sc + target) + cs);
                PEA_ST_AGENT(cnt + i, 0ull); PEA_ST_AGENT(sr + i, 0ull); PEA_ST_AGENT(sc + i, 0ull);
              }
              wg_publish();
            }
          }
        }
      }
    }
    if (p + 1 < P.n_passes) {  // every chain becomes one link (the roots do not move meanwhile); the finish resolves the last pass's
      wg_publish();
#pragma unroll 1
      for (unsigned base = 0; base < N; base += kLook * kBlock) {
        int a[kLook];
#pragma unroll
        for (int k = 0; k < kLook; ++k) {
          const unsigned i = base + (unsigned)k * kBlock + tid;
          a[k] = i < N ? PEA_LD_AGENT(alias + i) : (int)i;
        }
#pragma unroll
        for (int k = 0; k < kLook; ++k) {
          const unsigned i = base + (unsigned)k * kBlock + tid;
          if (i >= N || a[k] == (int)i || (unsigned)a[k] >= N) continue;
          int hops;
          const int r = find_root(alias, a[k], N, &hops);
          if (hops) PEA_ST_AGENT(alias + i, r);
        }
      }
      wg_publish();
    }
  }
  chain = wave_max(chain);
  __syncthreads();
  if (lane == 0) s_red[wave][0] = (u64)chain;
  __syncthreads();
  if (tid == 0) {
    u64 longest = 0;
    for (int k = 0; k < kBlock / 64; ++k) longest = s_red[k][0] > longest ? s_red[k][0] : longest;
    int64_t* st = stats + b * PEA_MERGE_STATS;
    st[PEA_MERGE_CANDIDATES] = (int64_t)looked;
    st[PEA_MERGE_MERGES] = (int64_t)merges;
    st[PEA_MERGE_NEGATIVE] = (int64_t)negative;
    st[PEA_MERGE_FEW] = (int64_t)few;
    st[PEA_MERGE_OUT_OF_RANGE] = (int64_t)M.img[b * kImgWords + W_BAD];
    st[PEA_MERGE_CHAIN] = (int64_t)longest;
    st[6] = 0; st[7] = 0;
  }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int numbered(const MergeParams& P, const MergeWs& M, bool in, size_t b, u64 i) {
  return (in && i > 0 && M.cnt[b * P.N + i] > 0) ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void k_merge_totals(const MergeParams P, const MergeWs M) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  if (in) {
    int hops;
    M.root[b * P.N + i] = find_root(M.alias + b * P.N, (int)i, P.N, &hops);
  }
  int total;
  (void)block_scan_excl(numbered(P, M, in, b, i), &total);
  if (threadIdx.x == 0) M.tot[blockIdx.x] = total;  // [b][chunk]
}
// one workgroup per image walks its totals 256 at a time with a carry: tot becomes the exclusive prefix
__global__ __launch_bounds__(kBlock) void k_merge_scan(const MergeParams P, const MergeWs M, int32_t* __restrict__ counts) {
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
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}
__global__ __launch_bounds__(kBlock) void k_merge_rank(const MergeParams P, const MergeWs M) {
  size_t b;
  u64 i;
  const bool in = at(P.ichunks, P.N, &b, &i);
  const int f = numbered(P, M, in, b, i);
  int total;
  const int ex = block_scan_excl(f, &total);
  if (in) M.rank[b * P.N + i] = f ? M.tot[blockIdx.x] + ex + 1 : 0;
}
__global__ __launch_bounds__(kBlock) void k_merge_map(const MergeParams P, const MergeWs M) {
  size_t b;
  u64 i;
  if (!at(P.ichunks, P.N, &b, &i)) return;
  const size_t o = b * P.N + i;
  M.root[o] = M.rank[b * P.N + (unsigned)M.root[o]];
}
// seg and out may be the same block: a lane writes only what it has read
__global__ __launch_bounds__(kBlock) void k_merge_project(const MergeParams P, const int* __restrict__ map, const int32_t* seg, int32_t* out) {
  const BlockAt where = block_at(P.pchunks);
  const size_t i0 = quad_start(where.chunk);
  const int nv = quad_nv(i0, P.S);
  if (!nv) return;
  const size_t o = (size_t)where.plane * P.S + i0;
  int v[kQuad];
  ld_iquad(seg + o, nv, 0, v);
  const int* __restrict__ m = map + (size_t)where.plane * P.N;
#pragma unroll
  for (int e = 0; e < kQuad; ++e)
    if (e < nv && (unsigned)v[e] < P.N) v[e] = m[(unsigned)v[e]];
  int32_t* op = out + o;
  if (nv == kQuad && ((uintptr_t)op & 15) == 0) {
    iquad_t q;
    q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    *(iquad_t*)op = q;
  } else {
#pragma unroll
    for (int e = 0; e < kQuad; ++e)
      if (e < nv) op[e] = v[e];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b ? 1 : 0); }
// the blocks in order, each a multiple of 8 bytes: 8 words per image, the three moments (8 bytes an id each), alias (4 an id), the
// candidate bits (8 per 64 ids), root, rank (4 an id each), the totals of the scan (4 per 256 ids)
inline size_t merge_layout(const PeaMergeDesc* d, void* base, MergeWs* M) {
  const uint64_t B = (uint64_t)d->B, N = (uint64_t)d->max_id + 1, per = mul_sat(B, N);
  Carver k(base);
  M->img = k.take<u64>(kImgWords * B);
  M->cnt = k.take<u64>(per);
  M->sr = k.take<u64>(per);
  M->sc = k.take<u64>(per);
  M->alias = k.take<int>(per);
  M->bits = k.take<u64>(mul_sat(B, ceil_div(N, 64)));
  M->root = k.take<int>(per);
  M->rank = k.take<int>(per);
  M->tot = k.take<int>(mul_sat(B, ceil_div(N, kBlock)));
  return k.bytes();
}

}  // namespace

extern "C" int pea_merge_validate(const PeaMergeDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->flags & ~PEA_MERGE_RELABEL) return PEA_E_DESC;
  if (d->B < 1 || d->Y < 1 || d->X < 1) return PEA_E_DESC;
  if (d->max_id < 0 || d->max_id > 0x7ffffffe) return PEA_E_DESC;
  if (d->n_passes < 1 || d->n_passes > PEA_MERGE_MAX_PASSES) return PEA_E_DESC;
  for (int p = 0; p < d->n_passes; ++p)
    if (d->threshold[p] < 0 || d->window[p] < 1 || d->window[p] > PEA_MERGE_MAX_WINDOW) return PEA_E_DESC;
  for (int p = 0; p < d->n_passes; ++p)
    if (d->window[p] > d->Y || d->window[p] > d->X) return PEA_E_UNSUPPORTED;
  return PEA_OK;
}

extern "C" size_t pea_merge_workspace_bytes(const PeaMergeDesc* d) {
  MergeWs M;
  return pea_merge_validate(d) ? 0 : merge_layout(d, nullptr, &M);
}

extern "C" int pea_merge_small(const PeaMergeDesc* d, const int32_t* seg, int32_t* out, int32_t* counts, int64_t* stats, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const int vrc = pea_merge_validate(d);
  if (vrc) return vrc;
  if (!seg || !out || !counts || !stats) return PEA_E_NULL;
  if (misaligned(seg, 4) || misaligned(out, 4) || misaligned(counts, 4) || misaligned(stats, 8) || misaligned(workspace, 8)) return PEA_E_ALIGN;
  MergeWs M;
  if (!workspace || workspace_bytes < merge_layout(d, workspace, &M)) return PEA_E_WORKSPACE;
  MergeParams P;
  const uint64_t S = mul_sat((uint64_t)d->Y, (uint64_t)d->X), N = (uint64_t)d->max_id + 1;
  if (S >= (1ull << 31)) return PEA_E_UNSUPPORTED;
  unsigned pixel_groups, id_groups;
  if (!stream_grid(S, (uint64_t)d->B, kQuadRun, &P.pchunks, &pixel_groups)) return PEA_E_UNSUPPORTED;
  if (!stream_grid(N, (uint64_t)d->B, kBlock, &P.ichunks, &id_groups)) return PEA_E_UNSUPPORTED;
  if (out != seg) {
    const uint64_t bytes = mul_sat(mul_sat((uint64_t)d->B, S), 4);
    const uintptr_t a = (uintptr_t)seg, o = (uintptr_t)out;
    if ((a < o ? o - a : a - o) < bytes) return PEA_E_UNSUPPORTED;
  }
  P.wchunks = (unsigned)ceil_div(N, 64);
  P.B = d->B; P.Y = d->Y; P.X = d->X; P.N = (unsigned)N; P.S = (size_t)S;
  P.n_passes = d->n_passes; P.relabel = (d->flags & PEA_MERGE_RELABEL) ? 1 : 0;
  for (int p = 0; p < PEA_MERGE_MAX_PASSES; ++p) {
    P.thr[p] = p < d->n_passes ? d->threshold[p] : 0;
    P.win[p] = p < d->n_passes ? d->window[p] : 1;
  }

  LaunchChain chain(stream);
  chain(k_merge_init, id_groups, kBlock, P, M);
  chain(k_merge_moments, pixel_groups, kBlock, P, M, seg);
  chain(k_merge_walk, (unsigned)d->B, kBlock, P, M, seg, stats);
  chain(k_merge_totals, id_groups, kBlock, P, M);
  chain(k_merge_scan, (unsigned)d->B, kBlock, P, M, counts);
  chain(k_merge_rank, id_groups, kBlock, P, M);
  if (P.relabel) chain(k_merge_map, id_groups, kBlock, P, M);
  chain(k_merge_project, pixel_groups, kBlock, P, M.root, seg, out);
  return chain.rc;
}
