// pea_multi_common.h -- what the batched launches share (pea_k_multi.hip: the tensor form, include/pea_multi.h;
// pea_k_multi_labels.hip: the labels-in form, include/pea_multi_labels.h): the per-entry geometry of the launch table, the walk from
// a workgroup to (entry, tile), the uniform branch over an entry's D / border, the loss finish with a workgroup per entry, and the
// host side that fills them (fused set -- any of the three storage types, one per table --, tile order, tile placement).
//
// The table of a launch travels BY VALUE in the kernel arguments: no device-side table and no copy from host memory on the stream,
// so the calls can be captured into a HIP graph.  A workgroup serves one tile (256 consecutive pixels of one batch item) of one entry
// and finds the entry from the prefix of tile counts; the host puts the entry with the most tiles first.  The tiles are walked
// XCD-aware like logical_tile() walks one image: every XCD takes a contiguous range of the concatenated tile list, so the rows a
// tile's neighbours live in are mostly rows its own XCD loads anyway.
#pragma once
#include <algorithm>

#include "../../include/pea_multi.h"
#include "pea_dispatch.h"
#include "pea_gather.h"

namespace pea {
namespace multi {

constexpr int kMaxN = PEA_MULTI_MAX_N, kMaxK = PEA_MULTI_MAX_K;

struct MGeom {  // what the bodies read of an entry's descriptor
  int S, Z, Y, X, K, D, border;
  int chunks;  // workgroups per batch item = ceil(S / kBlock)
  int tile0;   // the entry's first tile in the launch's tile order
  float eps;
  int16_t off[kMaxK][3];
};
struct MFinEntry {
  LossState* st;
  float* loss_out;
  int K, pad;
  float inv_n[kMaxK], lam[kMaxK];
};
template <typename ENT>
struct MTable {
  int n, tiles, tiles_per_xcd, pad;
  ENT en[kMaxN];
};
struct MFinTable {
  MFinEntry en[kMaxN];
};
static_assert(sizeof(MFinTable) <= 4096 - 64, "the tables must fit the kernel-argument segment");

// the launch's tile of this workgroup (XCD-aware, as logical_tile) and the entry it belongs to; false: past the last tile
template <typename ENT>
__device__ __forceinline__ bool find_entry(const MTable<ENT>& T, int& idx, int& tile) {
  const int t = ((int)blockIdx.x % kXcd) * T.tiles_per_xcd + (int)blockIdx.x / kXcd;
  if (t >= T.tiles) return false;
  idx = 0;
  for (int i = 1; i < T.n; ++i)
    if (t >= T.en[i].g.tile0) idx = i;
  tile = t - T.en[idx].g.tile0;
  return true;
}

// f(Int<v>{}) for the value a workgroup's entry has: SEL >= 0 when the whole table agrees on it, else a uniform branch over A, B(, C)
template <int SEL, int A, int B, int C = B, typename F>
__device__ __forceinline__ void with_value(int v, F&& f) {
  if constexpr (SEL >= 0) f(Int<SEL>{});
  else if (v == A) f(Int<A>{});
  else if (C == B || v == B) f(Int<B>{});
  else f(Int<C>{});
}

// k_loss_finish (pea_loss.h) with one workgroup per entry
static __global__ __launch_bounds__(64 * ((kMaxK + 3) / 4)) void k_loss_finish_multi(const MFinTable T) {
  const MFinEntry& E = T.en[blockIdx.x];
  loss_finish<kMaxK>(E.st, E.loss_out, E.K, E.inv_n, E.lam);
}

inline void launch_loss_finish_multi(const MFinTable& F, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_loss_finish_multi, dim3((unsigned)n), dim3(64 * ((kMaxK + 3) / 4)), 0, s, F);
}

// ------------------------------------------------------------------------------------------------
// host: the fused set, descriptor -> table entry
// ------------------------------------------------------------------------------------------------
inline bool fuses(const PeaDesc* d) {  // (any of the three storage types: pea_desc_validate admits no other)
  if ((d->D != 16 && d->D != 32) || d->K > kMaxK) return false;
  if (d->border != PEA_BORDER_CIRCULAR && d->border != PEA_BORDER_CROP_ZERO) return false;
  if (d->flags & PEA_FLAG_LOSS_ACT) return false;
  const long long S = (long long)d->dims[0] * d->dims[1] * d->dims[2];
  if (S * std::max(d->D, d->K) > 0x7fffffffLL) return false;
  for (int i = 0; i < d->K; ++i)
    for (int a = 0; a < 3; ++a)
      if (d->offsets[i][a] < -32768 || d->offsets[i][a] > 32767) return false;
  return true;
}

inline MGeom make_geom(const PeaDesc* d) {
  MGeom g;
  memset(&g, 0, sizeof(g));
  g.Z = d->dims[0]; g.Y = d->dims[1]; g.X = d->dims[2]; g.K = d->K; g.D = d->D;
  g.S = g.Z * g.Y * g.X;
  g.border = d->border; g.eps = d->eps;
  g.chunks = (g.S + kBlock - 1) / kBlock;
  for (int i = 0; i < d->K; ++i)
    for (int a = 0; a < 3; ++a) g.off[i][a] = (int16_t)d->offsets[i][a];
  return g;
}

// the loss finish's entry i
inline void fill_finish(MFinEntry& Fe, const PeaDesc* d, LossState* st, float* loss_out) {
  Fe.st = st; Fe.loss_out = loss_out; Fe.K = d->K;
  for (int k = 0; k < d->K; ++k) {
    Fe.inv_n[k] = (float)(1.0 / normaliser(d, k));
    Fe.lam[k] = d->lambda[k];
  }
}

// entry order of the launch: most tiles first (stable), so the tail of every XCD's range is the small images
inline void tile_order(const PeaDesc* const* descs, int n, int* order) {
  long long tiles[kMaxN];
  for (int i = 0; i < n; ++i) {
    const long long S = (long long)descs[i]->dims[0] * descs[i]->dims[1] * descs[i]->dims[2];
    tiles[i] = (S + kBlock - 1) / kBlock * descs[i]->B;
    order[i] = i;
  }
  std::stable_sort(order, order + n, [&](int a, int b) { return tiles[a] > tiles[b]; });
}

// the whole table: every descriptor valid and in the fused set, ONE storage type for all entries (the kernels are instantiated
// per storage type and chosen on the host: a table of f32 and 16-bit entries, or of f16 and bf16 ones, stays outside), and the
// tiles of all entries fit one grid
inline bool table_fuses(const PeaDesc* const* descs, int n) {
  if (n < 1 || n > kMaxN || !descs) return false;
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    if (!descs[i] || pea_desc_validate(descs[i]) != PEA_OK || !fuses(descs[i])) return false;
    if (descs[i]->dtype != descs[0]->dtype) return false;
    const long long S = (long long)descs[i]->dims[0] * descs[i]->dims[1] * descs[i]->dims[2];
    tiles += (S + kBlock - 1) / kBlock * descs[i]->B;  // (each term < 2^31: pea_desc_validate)
  }
  return tiles <= 0x7fffff00LL;
}

// tile0 of every entry (entries already in launch order, g.chunks set; B[i]: their batch sizes), the totals -> the grid
template <typename ENT>
inline dim3 place_tiles(MTable<ENT>& T, const int* B) {
  int t0 = 0;
  for (int i = 0; i < T.n; ++i) {
    T.en[i].g.tile0 = t0;
    t0 += B[i] * T.en[i].g.chunks;
  }
  T.tiles = t0;
  T.tiles_per_xcd = (t0 + kXcd - 1) / kXcd;
  return dim3((unsigned)(T.tiles_per_xcd * kXcd));
}

// the value all n entries share, or -1
template <typename GET>
inline int common(int n, GET&& get) {
  const int v = get(0);
  for (int i = 1; i < n; ++i)
    if (get(i) != v) return -1;
  return v;
}

}  // namespace multi
}  // namespace pea
