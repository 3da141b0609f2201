// pea_k_segscore.hip -- the segmentation scores of the validation loops from one contingency table per image (include/pea_segscore.h):
// SymmetricBestDice / AbsDiffFGLabels / FGBGDice of utils/evaluate.py and skimage's adapted_rand_error / variation_of_information, which
// the reference computes with a Python double loop over label pairs and one scipy sparse table per score.  The header states the
// semantics and the arithmetic; this comment says how the launches are laid out.
//
//   k_seg_pairs      streaming over the pixels: the joint histogram n_ij into a per-image open-addressing table keyed by (pred, gt)
//   k_seg_marginals  over the pair slots: a_i, a'_i and b_j into two tables of the same kind keyed by id; min / max label, N',
//                    sum n_ij^2, sum n_ij log2 n_ij, the number of pairs
//   k_seg_dice       over the slots of all three tables: per pair 2 n_ij / (a_i + b_j), its maximum per row and per column (an integer
//                    max on the f64 bits); per row / column the squares, the n log2 n terms, the foreground counts, the id counts
//   k_seg_best       over the row / column slots: the sums of the best Dice values; every slot goes back to zero
//   k_seg_finish     a lane per image: the columns; the per-image words go back to zero
//
// The pass over pixels, the slot helpers of the tables and the wave-side sums are those of pea_segtable.h, which says how they work.
#include "../../include/pea_segscore.h"
#include "pea_segtable.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

constexpr unsigned kSegMagic = 0x50454153u;     // "PEAS"
constexpr int kHdrWords = kTableHdrWords;       // u64 words: [0] magic
constexpr int kImgWords = kSegImgWords;         // per image, below
constexpr int kMargWords = 4;                   // per row slot: id + 1, a_i, a'_i, best Dice bits; per column slot: id + 1, b_j, best Dice bits, -

// the per-image words.  The four extrema are kept as (label + 1) and (2^31 - label) under an integer max, so that zero means "none yet"
enum {
  I_MAXP = I_OVF + 1, I_MINP, I_MAXG, I_MING, I_N2, I_NP, I_PAIRS, I_NPRED, I_NGT, I_A2, I_B2, I_FGP, I_FGG, I_FGB,
  I_NLN = 16,  // fixed point, two words each (fraction digits, whole part): sum n_ij log2 n_ij
  I_ALA = 18,  // sum a'_i log2 a'_i
  I_BLB = 20,  // sum b_j log2 b_j
  I_BDR = 22,  // sum of the rows' best Dice
  I_BDC = 24,  // sum of the columns' best Dice
};
static_assert(I_BDC + 2 <= kImgWords, "the per-image words");

struct Tables {
  u64* hdr;
  u64* img;    // [B][kImgWords]
  u64* pairs;  // [B][cap][kPairWords]
  u64* rows;   // [B][cap][kMargWords]
  u64* cols;   // [B][cap][kMargWords]
  u64 cap;
  int B;
};

inline size_t tables_layout(const PeaSegDesc* d, void* base, Tables* t) {
  const uint64_t B = (uint64_t)d->B, cap = (uint64_t)d->capacity;
  Carver c(base);
  t->hdr = c.take<u64>(kHdrWords);
  t->img = c.take<u64>(kImgWords * B);
  t->pairs = c.take<u64>(mul_sat(B * cap, kPairWords));
  t->rows = c.take<u64>(mul_sat(B * cap, kMargWords));
  t->cols = c.take<u64>(mul_sat(B * cap, kMargWords));
  t->cap = cap;
  t->B = d->B;
  return c.bytes();
}

__device__ __forceinline__ double nlog2n(u64 n) { return n > 1 ? (double)n * log2((double)n) : 0.0; }
// the difference p - q of two fixed-point sums, taken on the integers
__device__ __forceinline__ double fx_diff(const u64* p, const u64* q) {
  const long long hp = (long long)(p[1] + (p[0] >> 32)), hq = (long long)(q[1] + (q[0] >> 32));
  const long long lp = (long long)(p[0] & 0xffffffffull), lq = (long long)(q[0] & 0xffffffffull);
  return (double)(hp - hq) + (double)(lp - lq) / kFx;
}
__device__ __forceinline__ long long label_min(u64 w) { return w ? (long long)0x80000000ll - (long long)w : 0; }
__device__ __forceinline__ long long label_max(u64 w) { return w ? (long long)w - 1 : 0; }

// ---- 1: the joint histogram: k_seg_pairs of pea_segtable.h -------------------------------------------------------------------------------------

__device__ __forceinline__ bool slot_of_lane(const Tables& T, size_t* b, size_t* s) { return pea::slot_of_lane(T.cap, T.B, b, s); }

// ---- 2: marginals, extrema and the sums over pairs -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_marginals(const Tables T) {
  size_t b, s;
  if (!slot_of_lane(T, &b, &s)) return;
  const int lane = threadIdx.x & 63;
  const u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
  const u64 key = ps[0], n = ps[1];
  u64 one = 0, n2 = 0, np = 0, lo = 0, hi = 0, mxp = 0, mnp = 0, mxg = 0, mng = 0, ovf = 0;
  if (key) {
    const u64 p = (key - 1) >> 32, g = (key - 1) & 0xffffffffull;
    one = 1;
    mxp = p + 1; mnp = 0x80000000ull - p;
    mxg = g + 1; mng = 0x80000000ull - g;
    u64* rows = T.rows + b * T.cap * kMargWords;
    u64* cols = T.cols + b * T.cap * kMargWords;
    const long long rs = slot_claim<kMargWords>(rows, T.cap, p + 1);
    const long long cs = slot_claim<kMargWords>(cols, T.cap, g + 1);
    if (rs >= 0) {
      PEA_ATOM_ADD(rows + rs * kMargWords + 1, n);
      if (g != 0) PEA_ATOM_ADD(rows + rs * kMargWords + 2, n);
    }
    if (cs >= 0) PEA_ATOM_ADD(cols + cs * kMargWords + 1, n);
    if (rs < 0 || cs < 0) ovf = n;  // (cannot happen: there are no more ids than pairs)
    if (g != 0) {
      n2 = n * n;
      np = n;
      fx_split(nlog2n(n), lo, hi);
    }
  }
  u64* w = T.img + b * kImgWords;
  wave_add(w + I_PAIRS, one, lane);
  wave_add(w + I_N2, n2, lane);
  wave_add(w + I_NP, np, lane);
  wave_add(w + I_NLN, lo, lane);
  wave_add(w + I_NLN + 1, hi, lane);
  wave_add(w + I_OVF, ovf, lane);
  wave_max_into(w + I_MAXP, mxp, lane);
  wave_max_into(w + I_MINP, mnp, lane);
  wave_max_into(w + I_MAXG, mxg, lane);
  wave_max_into(w + I_MING, mng, lane);
}

// ---- 3: the Dice of every pair, the sums over rows and columns ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_dice(const Tables T) {
  size_t b, s;
  if (!slot_of_lane(T, &b, &s)) return;
  const int lane = threadIdx.x & 63;
  u64* w = T.img + b * kImgWords;
  const u64 minP = (u64)label_min(w[I_MINP]), minG = (u64)label_min(w[I_MING]);
  u64* rows = T.rows + b * T.cap * kMargWords;
  u64* cols = T.cols + b * T.cap * kMargWords;
  u64 fgb = 0;
  {
    const u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
    const u64 key = ps[0], n = ps[1];
    if (key) {
      const u64 p = (key - 1) >> 32, g = (key - 1) & 0xffffffffull;
      if (p > minP && g > minG) {
        fgb = n;
        const long long rs = slot_find<kMargWords>(rows, T.cap, p + 1);
        const long long cs = slot_find<kMargWords>(cols, T.cap, g + 1);
        if (rs >= 0 && cs >= 0) {
          const u64 a = rows[rs * kMargWords + 1], bj = cols[cs * kMargWords + 1];
          const double dice = 2.0 * (double)n / (double)(a + bj);
          const u64 bits = __builtin_bit_cast(u64, dice);  // positive: the bit patterns order like the values
          PEA_ATOM_MAX(rows + rs * kMargWords + 3, bits);
          PEA_ATOM_MAX(cols + cs * kMargWords + 2, bits);
        }
      }
    }
  }
  u64 npred = 0, a2 = 0, fgp = 0, alo = 0, ahi = 0;
  {
    const u64* rw = rows + s * kMargWords;
    const u64 key = rw[0];
    if (key) {
      const u64 a = rw[1], ap = rw[2];
      npred = 1;
      a2 = ap * ap;
      fx_split(nlog2n(ap), alo, ahi);
      if (key - 1 != minP) fgp = a;
    }
  }
  u64 ngt = 0, b2 = 0, fgg = 0, blo = 0, bhi = 0;
  {
    const u64* cw = cols + s * kMargWords;
    const u64 key = cw[0];
    if (key) {
      const u64 bj = cw[1];
      ngt = 1;
      if (key - 1 != 0) {
        b2 = bj * bj;
        fx_split(nlog2n(bj), blo, bhi);
      }
      if (key - 1 != minG) fgg = bj;
    }
  }
  wave_add(w + I_FGB, fgb, lane);
  wave_add(w + I_NPRED, npred, lane);
  wave_add(w + I_A2, a2, lane);
  wave_add(w + I_FGP, fgp, lane);
  wave_add(w + I_ALA, alo, lane);
  wave_add(w + I_ALA + 1, ahi, lane);
  wave_add(w + I_NGT, ngt, lane);
  wave_add(w + I_B2, b2, lane);
  wave_add(w + I_FGG, fgg, lane);
  wave_add(w + I_BLB, blo, lane);
  wave_add(w + I_BLB + 1, bhi, lane);
}

// ---- 4: the sums of the best Dice values; the slots go back to zero -------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_best(const Tables T) {
  size_t b, s;
  if (!slot_of_lane(T, &b, &s)) return;
  const int lane = threadIdx.x & 63;
  u64* w = T.img + b * kImgWords;
  const u64 minP = (u64)label_min(w[I_MINP]), minG = (u64)label_min(w[I_MING]);
  u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
  u64* rw = T.rows + (b * T.cap + s) * kMargWords;
  u64* cw = T.cols + (b * T.cap + s) * kMargWords;
  double dr = 0.0, dc = 0.0;
  if (rw[0] && rw[0] - 1 > minP) dr = __builtin_bit_cast(double, rw[3]);
  if (cw[0] && cw[0] - 1 > minG) dc = __builtin_bit_cast(double, cw[2]);
  if (ps[0]) { ps[0] = 0; ps[1] = 0; }
  if (rw[0]) { rw[0] = 0; rw[1] = 0; rw[2] = 0; rw[3] = 0; }
  if (cw[0]) { cw[0] = 0; cw[1] = 0; cw[2] = 0; }
  wave_add_fx(w + I_BDR, dr, lane);
  wave_add_fx(w + I_BDC, dc, lane);
}

// ---- 5: the columns -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_seg_finish(const Tables T, double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= T.B) return;
  const bool good = *(const unsigned*)T.hdr == kSegMagic;
  u64* w = T.img + (size_t)b * kImgWords;
  u64 v[kImgWords];
  for (int i = 0; i < kImgWords; ++i) {
    v[i] = w[i];
    w[i] = 0;
  }
  double* o = out + (size_t)b * PEA_SEG_COLS;
  const double qnan = __builtin_nan("");
  if (!good) {
    for (int i = 0; i < PEA_SEG_COLS; ++i) o[i] = qnan;
    return;
  }
  o[PEA_SEG_N_OVERFLOW] = (double)v[I_OVF];
  o[PEA_SEG_N_BAD] = (double)v[I_BAD];
  if (v[I_OVF] || v[I_BAD]) {
    for (int i = 2; i < PEA_SEG_COLS; ++i) o[i] = qnan;
    return;
  }
  const long long spanP = label_max(v[I_MAXP]) - label_min(v[I_MINP]), spanG = label_max(v[I_MAXG]) - label_min(v[I_MING]);
  const double bd = spanP > 0 ? fx_value(v + I_BDR) / (double)spanP : 0.0;
  const double bdr = spanG > 0 ? fx_value(v + I_BDC) / (double)spanG : 0.0;
  o[PEA_SEG_BEST_DICE] = bd;
  o[PEA_SEG_BEST_DICE_REV] = bdr;
  o[PEA_SEG_SBD] = bd < bdr ? bd : bdr;
  o[PEA_SEG_DIFF_FG] = (double)(spanP - spanG);
  const u64 fgden = v[I_FGP] + v[I_FGG];
  o[PEA_SEG_FGBG_DICE] = fgden ? 2.0 * (double)v[I_FGB] / (double)fgden : 0.0;
  const u64 np = v[I_NP];
  double split = 0.0, merge = 0.0;
  if (np) {  // a conditional entropy is never negative: a difference that truncation made negative is 0
    const double ds = fx_diff(v + I_BLB, v + I_NLN), dm = fx_diff(v + I_ALA, v + I_NLN);
    split = (ds > 0.0 ? ds : 0.0) / (double)np;
    merge = (dm > 0.0 ? dm : 0.0) / (double)np;
  }
  o[PEA_SEG_VOI_SPLIT] = split;
  o[PEA_SEG_VOI_MERGE] = merge;
  const double P2 = (double)(v[I_N2] - np), A2 = (double)(v[I_A2] - np), B2 = (double)(v[I_B2] - np);
  o[PEA_SEG_ARE] = 1.0 - P2 / (0.5 * A2 + 0.5 * B2);
  o[PEA_SEG_ARE_PRECISION] = P2 / A2;
  o[PEA_SEG_ARE_RECALL] = P2 / B2;
  o[PEA_SEG_SUM_NIJ2] = (double)v[I_N2];
  o[PEA_SEG_SUM_AI2] = (double)v[I_A2];
  o[PEA_SEG_SUM_BJ2] = (double)v[I_B2];
  o[PEA_SEG_N_PRIME] = (double)np;
  o[PEA_SEG_N_PRED_IDS] = (double)v[I_NPRED];
  o[PEA_SEG_N_GT_IDS] = (double)v[I_NGT];
  o[PEA_SEG_N_PAIRS] = (double)v[I_PAIRS];
}

// ---- pea_seg_table: the triples of one image (its table is image 0 of the workspace) -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_compact(const u64 cap, u64* __restrict__ img, u64* __restrict__ pairs, int32_t* __restrict__ pred_ids,
                                                        int32_t* __restrict__ gt_ids, int64_t* __restrict__ counts, const u64 max_triples) {
  const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= cap) return;
  u64* ps = pairs + s * kPairWords;
  const u64 key = ps[0], n = ps[1];
  if (!key) return;
  ps[0] = 0;
  ps[1] = 0;
  const u64 at = __hip_atomic_fetch_add(img + I_PAIRS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (at < max_triples) {
    pred_ids[at] = (int32_t)((key - 1) >> 32);
    gt_ids[at] = (int32_t)((key - 1) & 0xffffffffull);
    counts[at] = (int64_t)n;
  }
}
__global__ __launch_bounds__(64) void k_seg_table_finish(const u64* __restrict__ hdr, u64* __restrict__ img, int64_t* __restrict__ n_out) {
  if (threadIdx.x != 0) return;
  const bool good = *(const unsigned*)hdr == kSegMagic;
  n_out[0] = good ? (int64_t)img[I_PAIRS] : -1;
  n_out[1] = good ? (int64_t)img[I_OVF] : -1;
  n_out[2] = good ? (int64_t)img[I_BAD] : -1;
  img[I_PAIRS] = 0;
  img[I_OVF] = 0;
  img[I_BAD] = 0;
}

inline bool seg_grids(const PeaSegDesc* d, uint64_t images, unsigned* chunks, unsigned* pixel_groups, unsigned* slot_groups) {
  return pea::seg_grids((uint64_t)d->S, (uint64_t)d->capacity, images, chunks, pixel_groups, slot_groups);
}

}  // namespace

extern "C" int pea_seg_validate(const PeaSegDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->S < 1) return PEA_E_DESC;
  if (d->capacity < PEA_SEG_MIN_CAPACITY || (uint64_t)d->capacity > kMaxCapacity || (d->capacity & (d->capacity - 1))) return PEA_E_DESC;
  if (d->flags) return PEA_E_DESC;
  if (d->S > 0x7fffffffLL) return PEA_E_UNSUPPORTED;
  return PEA_OK;
}

extern "C" size_t pea_seg_workspace_bytes(const PeaSegDesc* d) {
  Tables T;
  return pea_seg_validate(d) ? 0 : tables_layout(d, nullptr, &T);
}

extern "C" int pea_seg_workspace_init(void* workspace, size_t bytes, void* stream) {
  return table_workspace_init<kSegMagic>(workspace, bytes, stream);
}

extern "C" int pea_seg_scores(const PeaSegDesc* d, const int32_t* pred, const int32_t* gt, double* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const int vrc = pea_seg_validate(d);
  if (vrc) return vrc;
  if (!pred || !gt || !out) return PEA_E_NULL;
  if (misaligned(pred, 4) || misaligned(gt, 4) || misaligned(out, 8) || misaligned(workspace, 8)) return PEA_E_ALIGN;
  Tables T;
  const size_t need = tables_layout(d, workspace, &T);
  if (!workspace || workspace_bytes < need) return PEA_E_WORKSPACE;
  unsigned chunks, pgroups, sgroups;
  if (!seg_grids(d, (uint64_t)d->B, &chunks, &pgroups, &sgroups)) return PEA_E_UNSUPPORTED;

  LaunchChain chain(stream);
  chain(k_seg_pairs<false>, pgroups, kBlock, d->S, chunks, T.cap, pred, gt, T.img, T.pairs, 0);
  chain(k_seg_marginals, sgroups, kBlock, T);
  chain(k_seg_dice, sgroups, kBlock, T);
  chain(k_seg_best, sgroups, kBlock, T);
  chain(k_seg_finish, (unsigned)((d->B + 63) / 64), 64, T, out);
  return or_prepare_again(chain.rc, [&] { launch_table_init<kSegMagic>(workspace, need, chain.s); });
}

extern "C" int pea_seg_table(const PeaSegDesc* d, const int32_t* pred, const int32_t* gt, int32_t b, int32_t* pred_ids, int32_t* gt_ids,
                             int64_t* counts, int64_t* n_out, int64_t max_triples, void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_seg_validate(d);
  if (vrc) return vrc;
  if (b < 0 || b >= d->B || max_triples < 1) return PEA_E_DESC;
  if (!pred || !gt || !pred_ids || !gt_ids || !counts || !n_out) return PEA_E_NULL;
  if (misaligned(pred, 4) || misaligned(gt, 4) || misaligned(pred_ids, 4) || misaligned(gt_ids, 4) || misaligned(counts, 8) ||
      misaligned(n_out, 8) || misaligned(workspace, 8))
    return PEA_E_ALIGN;
  Tables T;
  const size_t need = tables_layout(d, workspace, &T);
  if (!workspace || workspace_bytes < need) return PEA_E_WORKSPACE;
  unsigned chunks, pgroups, sgroups;
  if (!seg_grids(d, 1, &chunks, &pgroups, &sgroups)) return PEA_E_UNSUPPORTED;

  const size_t off = (size_t)b * (size_t)d->S;
  LaunchChain chain(stream);
  chain(k_seg_pairs<false>, pgroups, kBlock, d->S, chunks, T.cap, pred + off, gt + off, T.img, T.pairs, 0);
  chain(k_seg_compact, sgroups, kBlock, T.cap, T.img, T.pairs, pred_ids, gt_ids, counts, max_triples);
  chain(k_seg_table_finish, 1, 64, T.hdr, T.img, n_out);
  return or_prepare_again(chain.rc, [&] { launch_table_init<kSegMagic>(workspace, need, chain.s); });
}
