// pea_k_rag.hip -- the region adjacency graph of a fragment image or volume with per-edge statistics of an affinity map and of a
// boundary map (include/pea_rag.h): what elf's compute_rag, compute_affinity_features and compute_boundary_mean_and_length hand to the
// multicut solver in the reference's utils/lmc.py, and project_node_labels_to_pixels after it.  The header states the semantics and
// the arithmetic; this comment says how the launches are laid out.  The table, its probes and the peel are those of pea_segtable.h
// with another key: the pair of ids at the two ends of a voxel edge, (min << 32 | max) + 1, and eight words per slot.
//
//   k_rag_clear    the output rows and node_size go to zero
//   k_rag_edges    the streaming walk of k_seg_pairs over the voxels: a lane holds a quad of ids and reads the forward neighbours along
//                  x, y and z (guarded against the row, plane and image end); per axis the wave peels its keys -- an interior wave has
//                  none and leaves at the first ballot -- and lane r keeps the r-th peeled key with its pair count and the fixed-point
//                  boundary sum; the lanes then claim their slots side by side.  The same walk counts the voxels per id.
//   k_rag_samples  the same walk over (k, voxel): the key of (fragments[p], fragments[p + o_k]) is peeled with count, sum, min and max
//                  and LOOKED UP (slot_find, behind the kernel boundary): a miss is a pair that does not touch.  min and max are
//                  integer maxima of the order-preserving image of the f32 (min: of its complement), so a zero word is "none yet"
//   k_rag_degree   over the slots: edges by u into a dense array; the number of edges
//   k_rag_scan     a workgroup per image: the exclusive scan of the degrees (eight ids a lane, block_scan_excl of pea_stream.h over the
//                  lanes, a carry from step to step), the row starts
//   k_rag_scatter  over the slots: (slot, v) of every edge into its row, in arrival order
//   k_rag_rows     a LANE PER EDGE, so a row is served by as many lanes as it has entries (a hub of thousands of neighbours is spread
//                  over its own waves, whose lanes read the same row-mate at the same time): the rank of v among the row-mates, the
//                  means, the write, and the slot goes back to zero
//   k_rag_stats    the stats, a lane per image; the per-image words, the rows and the per-id counters go back to zero, so the whole
//                  block is zero again behind the magic word and serves a call with ANY descriptor
// Every loop is bounded: probes by the capacity, the rank by the row length, the walks by the image extent.
#include "../../include/pea_rag.h"
#include "pea_segtable.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

typedef unsigned int u32;
constexpr unsigned kRagMagic = 0x50454152u;  // "PEAR"
constexpr int kHdrWords = kTableHdrWords;
constexpr int kImgWords = kSegImgWords;
constexpr int kSlotWords = 8;  // key + 1, size, bsum (lo, hi), count, sum (lo, hi), ~ord(min) | ord(max) << 32
enum { W_KEY = 0, W_SIZE, W_BLO, W_BHI, W_CNT, W_SLO, W_SHI, W_MNMX };
enum { I_NOID = I_BAD, I_PDROP = I_OVF, I_NEDGE, I_EDROP, I_NTOUCH, I_SKIP, I_END };
static_assert(I_END <= kImgWords, "the per-image words");
constexpr int kScanPer = 8;            // ids per lane and step of the scan
constexpr float kMaxAbs = 32768.f;     // 2^15: a larger term is skipped

struct Rag {
  u64* hdr;
  u64* img;    // [B][kImgWords]
  u64* slots;  // [B][cap][kSlotWords]
  u32* order;  // [B][cap] slot of the edge at a row position (arrival order within a row)
  u32* rowv;   // [B][cap] its v
  u32* deg;    // [B][M]   edges with this u
  u32* start;  // [B][M]   row start
  u32* cur;    // [B][M]   cursor of the scatter
  u64 cap, max_edges;
  size_t S;
  u32 M, X, Y, Z;
  int B, K;
  unsigned flags;
};

struct RagOffs { int o[PEA_RAG_MAX_K][3]; };

// u64 words (header, per image, slots), then the u32 arrays as ONE block padded to a word
inline size_t rag_layout(const PeaRagDesc* d, void* base, Rag* t) {
  const uint64_t B = (uint64_t)d->B, cap = (uint64_t)d->capacity, M = (uint64_t)d->max_id + 1;
  Carver c(base);
  t->hdr = c.take<u64>(kHdrWords);
  t->img = c.take<u64>(kImgWords * B);
  t->slots = c.take<u64>(mul_sat(mul_sat(B, cap), kSlotWords));
  Carver tail(c.take<u32>(mul_sat(B, 2 * cap + 3 * M)));
  t->order = tail.take<u32>(B * cap, 4);
  t->rowv = tail.take<u32>(B * cap, 4);
  t->deg = tail.take<u32>(B * M, 4);
  t->start = tail.take<u32>(B * M, 4);
  t->cur = tail.take<u32>(B * M, 4);
  t->cap = cap; t->max_edges = (u64)d->max_edges;
  t->X = (u32)d->dims[2]; t->Y = (u32)d->dims[1]; t->Z = (u32)d->dims[0];
  t->S = (size_t)d->dims[0] * d->dims[1] * d->dims[2];
  t->M = (u32)M; t->B = d->B; t->K = d->K; t->flags = d->flags;
  return c.bytes();
}

__device__ __forceinline__ bool prepared(const Rag& T) { return *(const unsigned*)T.hdr == kRagMagic; }
__device__ __forceinline__ bool takes_part(const Rag& T, int id) {
  return (unsigned)id < T.M && !((T.flags & PEA_RAG_IGNORE_ZERO) && id == 0);
}
__device__ __forceinline__ u64 pair_key(int a, int b) {
  const u64 lo = (u64)(unsigned)(a < b ? a : b), hi = (u64)(unsigned)(a < b ? b : a);
  return ((lo << 32) | hi) + 1;
}
// one f32 term into a lane's fixed-point partial (floored, 32 fractional bits: lo the low 32 bits, hi the signed whole part); false:
// not finite or above 2^15 in magnitude, nothing added
__device__ __forceinline__ bool fx_term(float x, u64& lo, u64& hi) {
  if (!(__builtin_fabsf(x) <= kMaxAbs)) return false;
  const long long f = (long long)__builtin_floor((double)x * kFx);  // (exact: a power of two times an f32 of at most 2^15)
  lo += (u64)f & 0xffffffffull;
  hi += (u64)(f >> 32);
  return true;
}
// the two words of such a sum -> its value, rounded to f64 once
__device__ __forceinline__ double fx_signed(u64 lo, u64 hi) {
  const long long whole = (long long)hi + (long long)(lo >> 32);
  return (double)whole + (double)(lo & 0xffffffffull) / kFx;
}

// ---- 1: clear ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_clear(const Rag T, const PeaRagBuffers io, const size_t per) {
  const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t b = g / per, i = g - b * per;
  if (b >= (size_t)T.B) return;
  if (i < T.max_edges) {
    const size_t r = b * T.max_edges + i;
    io.uv[2 * r] = 0; io.uv[2 * r + 1] = 0;
    if (io.size) io.size[r] = 0;
    if (io.count) io.count[r] = 0;
    if (io.mean) io.mean[r] = 0.0;
    if (io.bmean) io.bmean[r] = 0.0;
    if (io.min) io.min[r] = 0.f;
    if (io.max) io.max[r] = 0.f;
  }
  if (i < T.M) {
    const size_t r = b * T.M + i;
    if (io.node_size) io.node_size[r] = 0;
  }
}

// ---- 2: the edge pass --------------------------------------------------------------------------------------------------------------------
// the quad at image element j0 (any alignment), the elements past the image as `fill`
__device__ __forceinline__ void nbr_ids(const int32_t* __restrict__ img, size_t j0, size_t S, int (&o)[kQuad]) {
  const int nv = quad_nv(j0, S);
  ld_iquad(img + (nv ? j0 : 0), nv, -1, o);
}
__device__ __forceinline__ void nbr_vals(const float* __restrict__ img, size_t j0, size_t S, float (&o)[kQuad]) {
  const int nv = quad_nv(j0, S);
  ld_quad<float>(img + (nv ? j0 : 0), nv, o);
}

template <bool kBnd>
__global__ __launch_bounds__(kBlock) void k_rag_edges(const Rag T, const unsigned chunks, const int32_t* __restrict__ frag,
                                                      const float* __restrict__ bnd, long long* __restrict__ node_size) {
  if (!prepared(T)) return;
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane, S = T.S;
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(at.chunk, S, &w0)) return;
  const size_t i0 = w0 + (size_t)lane * kQuad;
  const int nv = quad_nv(i0, S);
  const int32_t* __restrict__ fimg = frag + b * S;
  const float* __restrict__ bimg = kBnd ? bnd + b * S : nullptr;
  int f[kQuad];
  float bq[kQuad] = {0.f, 0.f, 0.f, 0.f};
  nbr_ids(fimg, i0, S, f);
  if constexpr (kBnd) nbr_vals(bimg, i0, S, bq);
  // where each of the lane's voxels lies: the guards of the three forward steps
  bool gx[kQuad], gy[kQuad], gz[kQuad];
  {
    CropCursor c(nv ? i0 : 0, T.Y, T.X);
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      const bool in = e < nv;
      gx[e] = in && c.x + 1 < T.X;
      gy[e] = in && c.y + 1 < T.Y;
      gz[e] = in && c.o + 1 < (size_t)T.Z;
      c.step(T.Y, T.X);
    }
  }
  u64 noid = 0;
  u64* __restrict__ tab = T.slots + b * T.cap * kSlotWords;
  u64 mykey = 0, mycnt = 0, mylo = 0, myhi = 0, dropped = 0, skipped = 0;
  const auto flush = [&]() {
    if (mykey) {
      const long long s = slot_claim<kSlotWords>(tab, T.cap, mykey);
      if (s >= 0) {
        u64* w = tab + s * kSlotWords;
        PEA_ATOM_ADD(w + W_SIZE, mycnt);
        if (kBnd) {
          if (mylo) PEA_ATOM_ADD(w + W_BLO, mylo);
          if (myhi) PEA_ATOM_ADD(w + W_BHI, myhi);
        }
      } else dropped += mycnt;
    }
    mykey = 0;
  };
  int r = 0;
  // one axis: the neighbour ids n (and boundary values nb) of the lane's quad under the guards g
  const auto axis = [&](const int (&n)[kQuad], const float (&nb)[kQuad], const bool (&g)[kQuad]) {
    u64 key[kQuad];
    unsigned open = 0;
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      key[e] = 0;
      if (g[e] && f[e] != n[e] && takes_part(T, f[e]) && takes_part(T, n[e])) {
        key[e] = pair_key(f[e], n[e]);
        open |= 1u << e;
      }
    }
    u64 cur;
    unsigned mm;
    while (peel(key, open, cur, mm)) {
      u64 lo = 0, hi = 0;
      if constexpr (kBnd) {
#pragma unroll
        for (int e = 0; e < kQuad; ++e)
          if ((mm >> e) & 1u) {
            skipped += (u64)!fx_term(bq[e], lo, hi);
            skipped += (u64)!fx_term(nb[e], lo, hi);
          }
        lo = wave_sum(lo);
        hi = wave_sum(hi);
      }
      const u64 cnt = wave_sum((u64)__popc(mm));
      if (lane == r) { mykey = cur; mycnt = cnt; mylo = lo; myhi = hi; }
      if (++r == 64) { flush(); r = 0; }
    }
  };
  int n[kQuad];
  float nb[kQuad] = {0.f, 0.f, 0.f, 0.f};
  // x: the next element (the guard keeps a row's last voxel from the next row's first)
  n[0] = f[1]; n[1] = f[2]; n[2] = f[3];
  n[3] = i0 + kQuad < S ? fimg[i0 + kQuad] : -1;
  if constexpr (kBnd) {
    nb[0] = bq[1]; nb[1] = bq[2]; nb[2] = bq[3];
    nb[3] = i0 + kQuad < S ? bimg[i0 + kQuad] : 0.f;
  }
  axis(n, nb, gx);
  if (T.Y > 1) {  // (uniform)
    nbr_ids(fimg, i0 + T.X, S, n);
    if constexpr (kBnd) nbr_vals(bimg, i0 + T.X, S, nb);
    axis(n, nb, gy);
  }
  if (T.Z > 1) {
    const size_t plane = (size_t)T.X * T.Y;
    nbr_ids(fimg, i0 + plane, S, n);
    if constexpr (kBnd) nbr_vals(bimg, i0 + plane, S, nb);
    axis(n, nb, gz);
  }
  flush();
  // the voxels per id, and the voxels with none
  {
    int key[kQuad];
    unsigned open = 0;
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      key[e] = f[e];
      if (e < nv) {
        if ((unsigned)f[e] < T.M) open |= 1u << e;
        else ++noid;
      }
    }
    if (node_size) {
      int cur;
      unsigned mm;
      while (peel(key, open, cur, mm)) {
        const u64 cnt = wave_sum((u64)__popc(mm));
        if (lane == 0) PEA_ATOM_ADD((u64*)node_size + b * T.M + (unsigned)cur, cnt);
      }
    }
  }
  u64* w = T.img + b * kImgWords;
  wave_add(w + I_NOID, noid, lane);
  wave_add(w + I_PDROP, dropped, lane);
  wave_add(w + I_SKIP, skipped, lane);
}

// ---- 3: the sample pass -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_samples(const Rag T, const RagOffs O, const unsigned chunks, const int32_t* __restrict__ frag,
                                                        const float* __restrict__ affs) {
  if (!prepared(T)) return;
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane / (unsigned)T.K, S = T.S;
  const int k = (int)(at.plane % (unsigned)T.K);
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(at.chunk, S, &w0)) return;
  const size_t i0 = w0 + (size_t)lane * kQuad;
  const int nv = quad_nv(i0, S);
  const int32_t* __restrict__ fimg = frag + b * S;
  int f[kQuad];
  float a[kQuad];
  nbr_ids(fimg, i0, S, f);
  nbr_vals(affs + (b * (size_t)T.K + k) * S, i0, S, a);
  const int dz = O.o[k][0], dy = O.o[k][1], dx = O.o[k][2];
  const long long step = ((long long)dz * T.Y + dy) * (long long)T.X + dx;
  u64 key[kQuad];
  unsigned open = 0;
  {
    CropCursor c(nv ? i0 : 0, T.Y, T.X);
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      key[e] = 0;
      const long long qz = (long long)c.o + dz, qy = (long long)c.y + dy, qx = (long long)c.x + dx;
      if (e < nv && qz >= 0 && qz < (long long)T.Z && qy >= 0 && qy < (long long)T.Y && qx >= 0 && qx < (long long)T.X) {
        const int v = fimg[(long long)(i0 + e) + step];  // inside the image: every coordinate was checked
        if (f[e] != v && takes_part(T, f[e]) && takes_part(T, v)) {
          key[e] = pair_key(f[e], v);
          open |= 1u << e;
        }
      }
      if (T.flags & PEA_RAG_ONE_MINUS) a[e] = 1.0f - a[e];
      c.step(T.Y, T.X);
    }
  }
  const u64* __restrict__ tab = T.slots + b * T.cap * kSlotWords;
  u64 mykey = 0, myall = 0, myok = 0, mylo = 0, myhi = 0, ntouch = 0, skipped = 0;
  u32 mymn = 0, mymx = 0;
  const auto flush = [&]() {
    if (mykey) {
      const long long s = slot_find<kSlotWords>(tab, T.cap, mykey);
      if (s < 0) ntouch += myall;
      else {
        skipped += myall - myok;
        if (myok) {
          u64* w = T.slots + (b * T.cap + (u64)s) * kSlotWords;
          PEA_ATOM_ADD(w + W_CNT, myok);
          if (mylo) PEA_ATOM_ADD(w + W_SLO, mylo);
          if (myhi) PEA_ATOM_ADD(w + W_SHI, myhi);
          u32* mm = (u32*)(w + W_MNMX);
          PEA_ATOM_MAX(mm, mymn);
          PEA_ATOM_MAX(mm + 1, mymx);
        }
      }
    }
    mykey = 0;
  };
  int r = 0;
  u64 cur;
  unsigned mm;
  while (peel(key, open, cur, mm)) {
    u64 lo = 0, hi = 0, ok = 0;
    u32 mn = 0, mx = 0;
#pragma unroll
    for (int e = 0; e < kQuad; ++e)
      if (((mm >> e) & 1u) && fx_term(a[e], lo, hi)) {
        ++ok;
        const u32 o = f32_ord(a[e]);
        mn = ~o > mn ? ~o : mn;
        mx = o > mx ? o : mx;
      }
    const u64 all = wave_sum((u64)__popc(mm));
    ok = wave_sum(ok);
    lo = wave_sum(lo);
    hi = wave_sum(hi);
    mn = wave_max(mn);
    mx = wave_max(mx);
    if (lane == r) { mykey = cur; myall = all; myok = ok; mylo = lo; myhi = hi; mymn = mn; mymx = mx; }
    if (++r == 64) { flush(); r = 0; }
  }
  flush();
  u64* w = T.img + b * kImgWords;
  wave_add(w + I_NTOUCH, ntouch, lane);
  wave_add(w + I_SKIP, skipped, lane);
}

// ---- 4: edges by u --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_degree(const Rag T) {
  size_t b, s;
  if (!slot_of_lane(T.cap, T.B, &b, &s)) return;
  if (!prepared(T)) return;
  const int lane = threadIdx.x & 63;
  const u64 key = T.slots[(b * T.cap + s) * kSlotWords + W_KEY];
  u64 one = 0;
  if (key) {
    const u64 u = (key - 1) >> 32;
    if (u < T.M) {
      PEA_ATOM_ADD(T.deg + b * T.M + u, 1u);
      one = 1;
    }
  }
  wave_add(T.img + b * kImgWords + I_NEDGE, one, lane);
}

// ---- 5: the row starts ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_scan(const Rag T) {
  if (!prepared(T)) return;
  const size_t b = blockIdx.x;
  const u32* deg = T.deg + b * T.M;
  u32* start = T.start + b * T.M;
  u32 carry = 0;
  for (u32 base = 0; base < T.M; base += kBlock * kScanPer) {  // (uniform: the barriers are met by all)
    const u32 j0 = base + threadIdx.x * kScanPer;
    u32 len[kScanPer], mine = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      len[e] = j0 + e < T.M ? deg[j0 + e] : 0u;
      mine += len[e];
    }
    u32 total;
    u32 run = carry + block_scan_excl(mine, &total);
    carry += total;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      if (j0 + e < T.M) start[j0 + e] = run;
      run += len[e];
    }
  }
}

// ---- 6: every edge into its row -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_scatter(const Rag T) {
  size_t b, s;
  if (!slot_of_lane(T.cap, T.B, &b, &s)) return;
  if (!prepared(T)) return;
  const u64 key = T.slots[(b * T.cap + s) * kSlotWords + W_KEY];
  if (!key) return;
  const u64 u = (key - 1) >> 32, v = (key - 1) & 0xffffffffull;
  if (u >= T.M) return;
  const u64 pos = (u64)T.start[b * T.M + u] + __hip_atomic_fetch_add(T.cur + b * T.M + u, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (pos < T.cap) {
    T.order[b * T.cap + pos] = (u32)s;
    T.rowv[b * T.cap + pos] = (u32)v;
  }
}

// ---- 7: rank within the row, the write ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_rows(const Rag T, const PeaRagBuffers io) {
  size_t b, pos;
  if (!slot_of_lane(T.cap, T.B, &b, &pos)) return;
  if (!prepared(T)) return;
  const int lane = threadIdx.x & 63;
  u64* img = T.img + b * kImgWords;
  const u64 n_edges = img[I_NEDGE] < T.cap ? img[I_NEDGE] : T.cap;
  u64 beyond = 0;
  if (pos < n_edges) {
    const u64 s = T.order[b * T.cap + pos];
    if (s < T.cap) {
      u64* w = T.slots + (b * T.cap + s) * kSlotWords;
      const u64 key = w[W_KEY];
      const u64 u = (key - 1) >> 32, v = (key - 1) & 0xffffffffull;
      if (key && u < T.M) {
        const u64 r0 = T.start[b * T.M + u];
        u64 len = T.deg[b * T.M + u];
        if (r0 + len > T.cap) len = r0 < T.cap ? T.cap - r0 : 0;
        const u32* __restrict__ row = T.rowv + b * T.cap + r0;
        u64 rank = 0;
        for (u64 j = 0; j < len; ++j) rank += (u64)(row[j] < (u32)v);
        const u64 e = r0 + rank;
        if (e < T.max_edges) {
          const size_t o = b * T.max_edges + e;
          const u64 size = w[W_SIZE], cnt = w[W_CNT];
          io.uv[2 * o] = (int32_t)u;
          io.uv[2 * o + 1] = (int32_t)v;
          if (io.size) io.size[o] = (int64_t)size;
          if (io.count) io.count[o] = (int64_t)cnt;
          if (io.mean) io.mean[o] = cnt ? fx_signed(w[W_SLO], w[W_SHI]) / (double)cnt : 0.0;
          if (io.bmean) io.bmean[o] = size ? fx_signed(w[W_BLO], w[W_BHI]) / (double)(2 * size) : 0.0;
          const u32 mn = ~(u32)(w[W_MNMX] & 0xffffffffull), mx = (u32)(w[W_MNMX] >> 32);
          if (io.min) io.min[o] = cnt ? ord_f32(mn) : 0.f;
          if (io.max) io.max[o] = cnt ? ord_f32(mx) : 0.f;
        } else beyond = 1;
      }
#pragma unroll
      for (int i = 0; i < kSlotWords; ++i) w[i] = 0;
    }
  }
  wave_add(img + I_EDROP, beyond, lane);
}

// ---- 8: the stats ------------------------------------------------------------------------------------------------------------------------------------
// A later call may come with another descriptor, whose tables lie where this call's rows and counters lay: they go back to zero too.
__global__ __launch_bounds__(kBlock) void k_rag_stats(const Rag T, long long* __restrict__ stats, const size_t per) {
  const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t b = g / per, i = g - b * per;
  if (b >= (size_t)T.B) return;
  long long* o = stats + b * PEA_RAG_STATS;
  if (!prepared(T)) {
    if (i < PEA_RAG_STATS) o[i] = -1;
    return;
  }
  if (i < T.cap) {
    u32 *po = T.order + b * T.cap + i, *pv = T.rowv + b * T.cap + i;
    if (*po) *po = 0;
    if (*pv) *pv = 0;
  }
  if (i < T.M) {
    u32 *pd = T.deg + b * T.M + i, *ps = T.start + b * T.M + i, *pc = T.cur + b * T.M + i;
    if (*pd) *pd = 0;
    if (*ps) *ps = 0;
    if (*pc) *pc = 0;
  }
  if (i) return;
  u64* w = T.img + b * kImgWords;
  o[PEA_RAG_N_EDGES] = (long long)w[I_NEDGE];
  o[PEA_RAG_N_EDGES_DROPPED] = (long long)w[I_EDROP];
  o[PEA_RAG_N_PAIRS_DROPPED] = (long long)w[I_PDROP];
  o[PEA_RAG_N_NO_ID] = (long long)w[I_NOID];
  o[PEA_RAG_N_NOT_TOUCHING] = (long long)w[I_NTOUCH];
  o[PEA_RAG_N_SKIPPED] = (long long)w[I_SKIP];
  o[6] = 0; o[7] = 0;
  for (int i = 0; i < I_END; ++i) w[i] = 0;
}

// ---- the projection ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rag_project(const size_t n, const int32_t* __restrict__ frag, const int32_t* __restrict__ labels,
                                                        const u32 n_labels, int32_t* __restrict__ seg, u64* __restrict__ n_bad) {
  u64 bad = 0;
  lane_run(blockIdx.x, n, [&](size_t i0, int nv) {
    int f[kQuad], o[kQuad];
    ld_iquad(frag + i0, nv, -1, f);
#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      const bool ok = (u32)f[e] < n_labels;
      o[e] = ok ? labels[(u32)f[e]] : 0;
      bad += (u64)(e < nv && !ok);
    }
    if (nv == kQuad && ((uintptr_t)(seg + i0) & 15) == 0) {
      iquad_t q;
      q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
      *(iquad_t*)(seg + i0) = q;
    } else {
#pragma unroll
      for (int e = 0; e < kQuad; ++e)
        if (e < nv) seg[i0 + e] = o[e];
    }
  });
  if (n_bad) wave_add(n_bad, bad, threadIdx.x & 63);
}

}  // namespace

extern "C" int pea_rag_validate(const PeaRagDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->flags & ~(PEA_RAG_ONE_MINUS | PEA_RAG_IGNORE_ZERO)) return PEA_E_DESC;
  if (d->K < 0 || d->K > PEA_RAG_MAX_K) return PEA_E_DESC;
  if (d->ndim != 2 && d->ndim != 3) return PEA_E_DESC;
  if (d->B < 1 || d->dims[0] < 1 || d->dims[1] < 1 || d->dims[2] < 1) return PEA_E_DESC;
  if (d->ndim == 2) {
    if (d->dims[0] != 1) return PEA_E_DESC;
    for (int k = 0; k < d->K; ++k)
      if (d->offsets[k][0] != 0) return PEA_E_DESC;
  }
  if (d->max_id < 0) return PEA_E_DESC;
  if (d->capacity < PEA_RAG_MIN_CAPACITY || (uint64_t)d->capacity > kMaxCapacity || (d->capacity & (d->capacity - 1))) return PEA_E_DESC;
  if (d->max_edges < 1) return PEA_E_DESC;
  if (mul_sat(mul_sat((uint64_t)d->dims[0], (uint64_t)d->dims[1]), (uint64_t)d->dims[2]) >= (1ull << 31)) return PEA_E_UNSUPPORTED;
  return PEA_OK;
}

extern "C" size_t pea_rag_workspace_bytes(const PeaRagDesc* d) {
  Rag T;
  return pea_rag_validate(d) ? 0 : rag_layout(d, nullptr, &T);
}

extern "C" int pea_rag_workspace_init(void* ws, size_t bytes, void* stream) { return table_workspace_init<kRagMagic>(ws, bytes, stream); }

extern "C" int pea_rag_build(const PeaRagDesc* d, const PeaRagBuffers* io, void* ws, size_t ws_bytes, void* stream) {
  const int vrc = pea_rag_validate(d);
  if (vrc) return vrc;
  if (!io || !io->fragments || !io->uv || !io->stats) return PEA_E_NULL;
  if (misaligned(io->fragments, 4) || misaligned(io->affs, 4) || misaligned(io->boundary, 4) || misaligned(io->uv, 4) || misaligned(io->min, 4) ||
      misaligned(io->max, 4) || misaligned(io->size, 8) || misaligned(io->count, 8) || misaligned(io->mean, 8) || misaligned(io->bmean, 8) ||
      misaligned(io->node_size, 8) || misaligned(io->stats, 8) || misaligned(ws, 8))
    return PEA_E_ALIGN;
  Rag T;
  const size_t need = rag_layout(d, ws, &T);
  if (!ws || need == SIZE_MAX || ws_bytes < need) return PEA_E_WORKSPACE;
  const bool sampled = io->affs && d->K > 0;
  unsigned chunks, pgroups, sgroups, kchunks, kgroups = 0, cgroups;
  if (!pea::seg_grids((uint64_t)T.S, (uint64_t)d->capacity, (uint64_t)d->B, &chunks, &pgroups, &sgroups)) return PEA_E_UNSUPPORTED;
  if (sampled && !stream_grid((uint64_t)T.S, mul_sat((uint64_t)d->B, (uint64_t)d->K), kQuadRun, &kchunks, &kgroups)) return PEA_E_UNSUPPORTED;
  const uint64_t per = (uint64_t)d->max_edges > (uint64_t)T.M ? (uint64_t)d->max_edges : (uint64_t)T.M;
  const uint64_t cg = mul_sat((uint64_t)d->B, per) / kBlock + 1;
  if (mul_sat((uint64_t)d->B, per) == UINT64_MAX || cg > 0x7fffffffULL) return PEA_E_UNSUPPORTED;
  cgroups = (unsigned)cg;
  const uint64_t tper = (uint64_t)d->capacity > (uint64_t)T.M ? (uint64_t)d->capacity : (uint64_t)T.M;
  const uint64_t tg = mul_sat((uint64_t)d->B, tper) / kBlock + 1;
  if (mul_sat((uint64_t)d->B, tper) == UINT64_MAX || tg > 0x7fffffffULL) return PEA_E_UNSUPPORTED;

  RagOffs O;
  memcpy(O.o, d->offsets, sizeof(O.o));
  const PeaRagBuffers A = *io;
  LaunchChain chain(stream);
  chain(k_rag_clear, cgroups, kBlock, T, A, per);
  if (A.boundary) chain(k_rag_edges<true>, pgroups, kBlock, T, chunks, A.fragments, A.boundary, (long long*)A.node_size);
  else chain(k_rag_edges<false>, pgroups, kBlock, T, chunks, A.fragments, A.boundary, (long long*)A.node_size);
  if (sampled) chain(k_rag_samples, kgroups, kBlock, T, O, kchunks, A.fragments, A.affs);
  chain(k_rag_degree, sgroups, kBlock, T);
  chain(k_rag_scan, d->B, kBlock, T);
  chain(k_rag_scatter, sgroups, kBlock, T);
  chain(k_rag_rows, sgroups, kBlock, T, A);
  chain(k_rag_stats, (unsigned)tg, kBlock, T, (long long*)A.stats, tper);
  return or_prepare_again(chain.rc, [&] { launch_table_init<kRagMagic>(ws, need, chain.s); });
}

extern "C" int pea_rag_project(int64_t n, const int32_t* fragments, const int32_t* node_labels, int64_t n_labels, int32_t* seg, int64_t* n_bad,
                               void* stream) {
  if (n < 1 || n_labels < 1) return PEA_E_DESC;
  if (!fragments || !node_labels || !seg) return PEA_E_NULL;
  if (misaligned(fragments, 4) || misaligned(node_labels, 4) || misaligned(seg, 4) || misaligned(n_bad, 8)) return PEA_E_ALIGN;
  unsigned chunks, groups;
  if (!stream_grid((uint64_t)n, 1, kLaneRun, &chunks, &groups)) return PEA_E_UNSUPPORTED;
  const u32 nl = n_labels > 0x80000000LL ? 0x80000000u : (u32)n_labels;  // (an int32 id is below 2^31)
  LaunchChain chain(stream);
  chain(k_rag_project, groups, kBlock, n, fragments, node_labels, nl, seg, (u64*)n_bad);
  return chain.rc;
}
