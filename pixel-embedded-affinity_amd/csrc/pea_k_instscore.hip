// pea_k_instscore.hip -- the instance scores of the BBBC039V1 validation loop from one contingency table per image
// (include/pea_instscore.h): agg_jc_index, get_fast_pq(match_iou >= 0.5) and pixel_f1 of the reference's utils/metrics_bbbc.py, which
// builds one full-image mask per instance and makes two or three full-image passes per (gt instance, pred id) pair.  The header states
// the semantics and the arithmetic; this comment says how the launches are laid out.
//
//   k_seg_pairs<true>  (pea_segtable.h) streaming over the pixels: the joint histogram n_ij; a label outside [0, max_id] is no id
//   k_inst_marginals   over the pair slots: a_i and b_j into DENSE arrays [max_id + 1] (the ids are bounded: no hash lookup later), the
//                      pixel counts, the number of entries of every gt row; the match tables are zeroed
//   k_inst_scan        a workgroup per image: an exclusive scan of the row lengths (the table as a CSR by gt id) and of the present
//                      flags (b_j > 0: the sorted list of present gt ids, one record (j, row start, row length, b_j) each) as ONE u64
//                      scan of the packed pair (block_scan_excl of pea_stream.h, eight ids a lane); n_pred_ids
//   k_inst_pairs       over the pair slots: iou of every pair, the PQ pairs (tp, the fixed-point sum_iou, pq_match) and the scatter of
//                      (pred id, n_ij, a_i, iou bits) into the rows; the order within a row is arrival order, nothing depends on it
//   k_inst_walk        ONE WAVE per image: the greedy AJI matching, a dependent chain of one step per present gt id
//   k_inst_finish      over the slots: every word of the workspace goes back to zero; one lane per image writes the columns
//
// The walk.  The used set is a bitset of max_id + 1 bits in LDS.  The wave reads the records of 64 present gt ids at once (one load
// for 64 steps) and hands them round with v_readlane; rows follow each other in the entry array in the order of the walk, and the head
// of the next row (its first 64 entries, which do not depend on this step) is loaded before this step's arithmetic, so a step does not
// wait for a round trip to memory.  The iou of an entry is the quotient that k_inst_pairs took (it does not depend on the used set), so
// no division stands in the chain from step to step either: that chain is the bitset alone.  Each lane keeps its best (iou bits,
// lowest id) among the entries that are not used; a row of up to kSeqRow entries is then searched lane by lane with v_readlane (a
// butterfly of __shfl goes through the LDS crossbar six times), a longer one by the butterfly.  The owning lane hands over n_ij and
// a_i, lane 0 sets the bit, and lane r keeps the winner of step r for one store of aji_match per 64 steps.  The pred ids that were
// never used are not searched for: their pixels are (all pixels of pred ids > 0) - (the a_i of the ids that were used), both known.
// Every loop is bounded: probes by the capacity, the walk by the number of present ids, a row by its length.
#include "../../include/pea_instscore.h"
#include "pea_segtable.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

typedef unsigned int u32;
constexpr unsigned kInstMagic = 0x50454149u;  // "PEAI"
constexpr int kHdrWords = kTableHdrWords;     // u64 words: [0] magic
constexpr int kImgWords = kSegImgWords;
constexpr int kEntWords = 4;                  // per row entry: n_ij << 32 | pred id, a_i, the bits of iou = n_ij / (a_i + b_j - n_ij), -
constexpr int kSeqRow = 8;                    // rows of up to this many entries are searched lane by lane, longer ones by a butterfly
constexpr int kRecWords = 2;                  // per present gt id: row start << 32 | row length << 16 | j, b_j
constexpr int kScanPer = 8;                   // ids per lane and step of the scan
constexpr int kUsedWords = (PEA_INST_MAX_ID + 1) / 32;

enum { I_TP = I_OVF + 1, I_SIOU /* two words */, I_PTP = I_SIOU + 2, I_PFP, I_PFN, I_NPRED, I_NPRES, I_C, I_U, I_END };
static_assert(I_END <= kImgWords, "the per-image words");

struct Inst {
  u64* hdr;
  u64* img;    // [B][kImgWords]
  u64* pairs;  // [B][cap][kPairWords]
  u64* ents;   // [B][cap][kEntWords]: the rows of the CSR, one after the other
  u64* recs;   // [B][R][kRecWords], R = min(M, cap): no more present gt ids than ids, nor than pairs
  u32* a;      // [B][M]  a_i  (the three u32 arrays end the block, which is padded to a u64 word)
  u32* bc;     // [B][M]  b_j
  u32* cur;    // [B][M]  row length, then row start, then the cursor of the scatter
  u64 cap, R;
  u32 M;       // max_id + 1
  int B;
};

inline size_t inst_layout(const PeaInstDesc* d, void* base, Inst* t) {
  const uint64_t B = (uint64_t)d->B, cap = (uint64_t)d->capacity, M = (uint64_t)d->max_id + 1;
  const uint64_t R = M < cap ? M : cap;
  Carver c(base);
  t->hdr = c.take<u64>(kHdrWords);
  t->img = c.take<u64>(kImgWords * B);
  t->pairs = c.take<u64>(mul_sat(B * cap, kPairWords));
  t->ents = c.take<u64>(mul_sat(B * cap, kEntWords));
  t->recs = c.take<u64>(B * R * kRecWords);
  Carver tail(c.take<u32>(3 * B * M));
  t->a = tail.take<u32>(B * M, 4);
  t->bc = tail.take<u32>(B * M, 4);
  t->cur = tail.take<u32>(B * M, 4);
  t->cap = cap; t->R = R; t->M = (u32)M; t->B = d->B;
  return c.bytes();
}

__device__ __forceinline__ bool prepared(const Inst& T) { return *(const unsigned*)T.hdr == kInstMagic; }

// ---- 2: marginals, pixel counts, row lengths ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_inst_marginals(const Inst T, int32_t* __restrict__ aji_match, int32_t* __restrict__ pq_match) {
  size_t b, s;
  if (!slot_of_lane(T.cap, T.B, &b, &s)) return;
  const int lane = threadIdx.x & 63;
  for (size_t j = s; j < T.M; j += T.cap) {
    if (aji_match) aji_match[b * T.M + j] = 0;
    if (pq_match) pq_match[b * T.M + j] = 0;
  }
  if (!prepared(T)) return;
  const u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
  const u64 key = ps[0], n = ps[1];
  u64 ptp = 0, pfp = 0, pfn = 0;
  if (key) {
    const u64 p = (key - 1) >> 32, g = (key - 1) & 0xffffffffull;
    if (p < T.M && g < T.M) {
      PEA_ATOM_ADD(T.a + b * T.M + p, (u32)n);
      PEA_ATOM_ADD(T.bc + b * T.M + g, (u32)n);
      if (p && g) {
        PEA_ATOM_ADD(T.cur + b * T.M + g, 1u);
        ptp = n;
      } else if (p) pfp = n;
      else if (g) pfn = n;
    }
  }
  u64* w = T.img + b * kImgWords;
  wave_add(w + I_PTP, ptp, lane);
  wave_add(w + I_PFP, pfp, lane);
  wave_add(w + I_PFN, pfn, lane);
}

// ---- 3: the CSR by gt id and the list of present gt ids ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_inst_scan(const Inst T) {
  if (!prepared(T)) return;
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const u32* a = T.a + b * T.M;
  const u32* bc = T.bc + b * T.M;
  u32* cur = T.cur + b * T.M;
  u64* recs = T.recs + b * T.R * kRecWords;
  u64 carry = 0;  // entries so far << 32 | present ids so far
  u64 npred = 0;
  for (u32 base = 0; base < T.M; base += kBlock * kScanPer) {
    const u32 j0 = base + threadIdx.x * kScanPer;
    u32 len[kScanPer], bj[kScanPer];
    u64 mine = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      const u32 j = j0 + e;
      const bool ok = j >= 1 && j < T.M;
      len[e] = ok ? cur[j] : 0u;
      bj[e] = ok ? bc[j] : 0u;
      npred += (u64)(ok && a[j] != 0);
      mine += ((u64)len[e] << 32) | (u64)(bj[e] != 0);
    }
    u64 total;
    u64 run = carry + block_scan_excl(mine, &total);
    carry += total;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      if (bj[e]) {
        const u64 k = run & 0xffffffffull, start = run >> 32;
        if (k < T.R) {
          recs[k * kRecWords] = (start << 32) | ((u64)len[e] << 16) | (u64)(j0 + e);
          recs[k * kRecWords + 1] = bj[e];
        }
        cur[j0 + e] = (u32)start;
      }
      run += ((u64)len[e] << 32) | (u64)(bj[e] != 0);
    }
  }
  u64* w = T.img + b * kImgWords;
  if (threadIdx.x == 0) w[I_NPRES] = carry & 0xffffffffull;
  wave_add(w + I_NPRED, npred, lane);
}

// ---- 4: the PQ pairs; the scatter into the rows ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_inst_pairs(const Inst T, const double match_iou, int32_t* __restrict__ pq_match) {
  size_t b, s;
  if (!slot_of_lane(T.cap, T.B, &b, &s)) return;
  if (!prepared(T)) return;
  const int lane = threadIdx.x & 63;
  u64* w = T.img + b * kImgWords;
  const bool clean = !(w[I_BAD] | w[I_OVF]);
  const u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
  const u64 key = ps[0], n = ps[1];
  u64 tp = 0, lo = 0, hi = 0;
  if (key) {
    const u64 p = (key - 1) >> 32, g = (key - 1) & 0xffffffffull;
    if (p && g && p < T.M && g < T.M) {
      const u64 ai = T.a[b * T.M + p], bj = T.bc[b * T.M + g];
      const double iou = (double)n / (double)(ai + bj - n);
      if (iou > match_iou) {
        tp = 1;
        fx_split(iou, lo, hi);
        if (pq_match && clean) pq_match[b * T.M + g] = (int32_t)p;
      }
      const u64 at = __hip_atomic_fetch_add(T.cur + b * T.M + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (at < T.cap) {
        u64* e = T.ents + (b * T.cap + at) * kEntWords;
        e[0] = (n << 32) | p;
        e[1] = ai;
        e[2] = __builtin_bit_cast(u64, iou);  // (positive: the bit patterns order like the values)
      }
    }
  }
  wave_add(w + I_TP, tp, lane);
  wave_add(w + I_SIOU, lo, lane);
  wave_add(w + I_SIOU + 1, hi, lane);
}

// ---- 5: the AJI walk, one wave per image ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_inst_walk(const Inst T, int32_t* __restrict__ aji_match) {
  // read and written with wavefront-scope atomics in program order: a wave's LDS accesses are served in the order it issues them, so
  // lane 0's update of a step is seen by every lane's reads of the next one without a barrier
  __shared__ u32 s_used[kUsedWords];
  const auto is_used = [&](u32 p) -> bool { return (__hip_atomic_load(&s_used[p >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) >> (p & 31)) & 1u; };
  if (!prepared(T)) return;
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x;
  u64* w = T.img + b * kImgWords;
  if (w[I_BAD] | w[I_OVF]) return;
  for (u32 i = lane; i < (T.M + 31) / 32; i += 64) s_used[i] = 0;
  __syncthreads();
  const u64 npres = w[I_NPRES] < T.R ? w[I_NPRES] : T.R;
  const u64 a1 = T.a[b * T.M + 1];  // (max_id >= 1)
  const u64* recs = T.recs + b * T.R * kRecWords;
  const u64* ents = T.ents + b * T.cap * kEntWords;
  u64 C = 0, U = 0, used_px = 0;
  // entry `lane` of the row of record `rec` (zeros past its end): the first 64 entries of a row, one load per lane
  const auto row_head = [&](u64 rec, u64& e0, u64& ai, u64& v) {
    const u64 at = (rec >> 32) + (u64)lane;
    const bool in = (u32)lane < (u32)((rec >> 16) & 0xffffu) && at < T.cap;
    e0 = in ? ents[at * kEntWords] : 0;
    ai = in ? ents[at * kEntWords + 1] : 0;
    v = in ? ents[at * kEntWords + 2] : 0;
  };
  const auto lane64 = [](u64 v, int l) -> u64 {  // v of lane l (uniform): two v_readlane, no trip through the LDS crossbar
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, l);
  };
  for (u64 k0 = 0; k0 < npres; k0 += 64) {
    const bool have = k0 + lane < npres;
    const u64 r0 = have ? recs[(k0 + lane) * kRecWords] : 0, r1 = have ? recs[(k0 + lane) * kRecWords + 1] : 0;
    const int steps = npres - k0 < 64 ? (int)(npres - k0) : 64;
    u32 mine = 0;
    u64 ne0, nai, nv;
    row_head(lane64(r0, 0), ne0, nai, nv);
    for (int r = 0; r < steps; ++r) {
      const u64 rec = lane64(r0, r), bj = lane64(r1, r);
      const u32 len = (u32)((rec >> 16) & 0xffffu);
      const u64 start = rec >> 32;
      const u64 he0 = ne0, hai = nai, hv = nv;
      if (r + 1 < steps) row_head(lane64(r0, r + 1), ne0, nai, nv);  // the next row's head is in flight during this step
      u64 bits = 0, mn = 0, ma = 0;  // the lane's best candidate; bits == 0: none (an iou of n_ij > 0 pixels is above 0)
      u32 id = 0;
      const auto consider = [&](u64 e0, u64 ai, u64 v) {
        const u32 p = (u32)(e0 & 0xffffffffull);
        if (e0 && p < T.M && !is_used(p) && (v > bits || (v == bits && p < id))) { bits = v; id = p; mn = e0 >> 32; ma = ai; }
      };
      consider(he0, hai, hv);
      u64 wbits = 0;
      u32 wid = 0;
      int owner = 0;
      if (len <= (u32)kSeqRow) {  // (uniform) a nucleus overlaps a handful of predictions: lane e holds entry e
        for (int e = 0; e < (int)len; ++e) {
          const u64 v = lane64(bits, e);
          const u32 p = (u32)__builtin_amdgcn_readlane((int)id, e);
          if (v > wbits || (v == wbits && v != 0 && p < wid)) { wbits = v; wid = p; owner = e; }
        }
      } else {
        for (u32 e = 64 + lane; e < len && start + e < T.cap; e += 64)  // a row longer than the wave
          consider(ents[(start + e) * kEntWords], ents[(start + e) * kEntWords + 1], ents[(start + e) * kEntWords + 2]);
        wbits = bits;
        wid = id;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const u64 ob = __shfl_xor(wbits, o, 64);
          const u32 oi = __shfl_xor(wid, o, 64);
          if (ob > wbits || (ob == wbits && oi < wid)) { wbits = ob; wid = oi; }
        }
        owner = __ffsll(__ballot(bits != 0 && id == wid)) - 1;
        owner = __builtin_amdgcn_readfirstlane(owner < 0 ? 0 : owner);
      }
      u32 winner = 1;
      u64 inter = 0, uni;
      if (wbits) {  // (uniform)
        const u64 aw = lane64(ma, owner);
        inter = lane64(mn, owner);
        winner = wid;
        uni = bj + aw - inter;
        used_px += aw;
      } else {
        const bool taken = is_used(1);
        uni = bj + (taken ? 0 : a1);
        used_px += taken ? 0 : a1;
      }
      C += inter;
      U += uni;
      if (lane == r) mine = winner;
      if (lane == 0) (void)__hip_atomic_fetch_or(&s_used[winner >> 5], 1u << (winner & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (no instruction: the compiler keeps the order)
    }
    const u32 j = (u32)(r0 & 0xffffu);  // lane r kept the winner of step r: one store for the 64 steps
    if (aji_match && have && j < T.M) aji_match[b * T.M + j] = (int32_t)mine;
  }
  if (lane == 0) {
    w[I_C] = C;
    w[I_U] = U + (w[I_PTP] + w[I_PFP] - used_px);  // + the pixels of the pred ids > 0 that were never used
  }
}

// ---- 6: the columns; every word goes back to zero ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void inst_columns(const Inst& T, size_t b, double* __restrict__ out) {
  u64* w = T.img + b * kImgWords;
  u64 v[I_END];
  for (int i = 0; i < I_END; ++i) {
    v[i] = w[i];
    w[i] = 0;
  }
  double* o = out + b * PEA_INST_COLS;
  const double qnan = __builtin_nan("");
  o[PEA_INST_N_OVERFLOW] = (double)v[I_OVF];
  o[PEA_INST_N_BAD] = (double)v[I_BAD];
  if (v[I_OVF] || v[I_BAD]) {
    for (int i = 2; i < PEA_INST_COLS; ++i) o[i] = qnan;
    return;
  }
  o[PEA_INST_AJI] = (double)v[I_C] / (double)v[I_U];
  o[PEA_INST_AJI_INTER] = (double)v[I_C];
  o[PEA_INST_AJI_UNION] = (double)v[I_U];
  const double tp = (double)v[I_TP], fp = (double)(v[I_NPRED] - v[I_TP]), fn = (double)(v[I_NPRES] - v[I_TP]);
  const double sum_iou = fx_value(v + I_SIOU);
  const double dq = tp / (tp + 0.5 * fp + 0.5 * fn), sq = sum_iou / (tp + 1.0e-6);
  o[PEA_INST_DQ] = dq;
  o[PEA_INST_SQ] = sq;
  o[PEA_INST_PQ] = dq * sq;
  o[PEA_INST_TP] = tp;
  o[PEA_INST_FP] = fp;
  o[PEA_INST_FN] = fn;
  o[PEA_INST_SUM_IOU] = sum_iou;
  const u64 den = 2 * v[I_PTP] + v[I_PFP] + v[I_PFN];
  o[PEA_INST_PIXEL_F1] = den ? (double)(2 * v[I_PTP]) / (double)den : 0.0;
  o[PEA_INST_PIX_TP] = (double)v[I_PTP];
  o[PEA_INST_PIX_FP] = (double)v[I_PFP];
  o[PEA_INST_PIX_FN] = (double)v[I_PFN];
  o[PEA_INST_N_PRED_IDS] = (double)v[I_NPRED];
  o[PEA_INST_N_GT_IDS] = (double)v[I_NPRES];
}

__global__ __launch_bounds__(kBlock) void k_inst_finish(const Inst T, double* __restrict__ out) {
  size_t b, s;
  if (!slot_of_lane(T.cap, T.B, &b, &s)) return;
  if (!prepared(T)) {
    if (s < PEA_INST_COLS) out[b * PEA_INST_COLS + s] = __builtin_nan("");
    return;
  }
  u64* ps = T.pairs + (b * T.cap + s) * kPairWords;
  u64* es = T.ents + (b * T.cap + s) * kEntWords;
  if (ps[0]) { ps[0] = 0; ps[1] = 0; }
  if (es[0]) { es[0] = 0; es[1] = 0; es[2] = 0; }
  for (size_t k = s; k < T.R; k += T.cap) {
    u64* r = T.recs + (b * T.R + k) * kRecWords;
    if (r[1]) { r[0] = 0; r[1] = 0; }
  }
  for (size_t j = s; j < T.M; j += T.cap) {
    u32 *pa = T.a + b * T.M + j, *pb = T.bc + b * T.M + j, *pc = T.cur + b * T.M + j;
    if (*pa) *pa = 0;
    if (*pb) *pb = 0;
    if (*pc) *pc = 0;
  }
  if (s == 0) inst_columns(T, b, out);
}

}  // namespace

extern "C" int pea_inst_validate(const PeaInstDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->S < 1) return PEA_E_DESC;
  if (d->capacity < PEA_INST_MIN_CAPACITY || (uint64_t)d->capacity > kMaxCapacity || (d->capacity & (d->capacity - 1))) return PEA_E_DESC;
  if (d->max_id < 1 || d->max_id > PEA_INST_MAX_ID) return PEA_E_DESC;
  if (!(d->match_iou >= 0.0 && d->match_iou <= 1.0)) return PEA_E_DESC;
  if (d->flags) return PEA_E_DESC;
  if (d->match_iou < 0.5) return PEA_E_UNSUPPORTED;
  if (d->S > 0x7fffffffLL) return PEA_E_UNSUPPORTED;
  return PEA_OK;
}

extern "C" size_t pea_inst_workspace_bytes(const PeaInstDesc* d) {
  Inst T;
  return pea_inst_validate(d) ? 0 : inst_layout(d, nullptr, &T);
}

extern "C" int pea_inst_workspace_init(void* ws, size_t bytes, void* stream) { return table_workspace_init<kInstMagic>(ws, bytes, stream); }

extern "C" int pea_inst_scores(const PeaInstDesc* d, const int32_t* pred, const int32_t* gt, double* out, int32_t* aji_match, int32_t* pq_match,
                               void* ws, size_t ws_bytes, void* stream) {
  const int vrc = pea_inst_validate(d);
  if (vrc) return vrc;
  if (!pred || !gt || !out) return PEA_E_NULL;
  if (misaligned(pred, 4) || misaligned(gt, 4) || misaligned(aji_match, 4) || misaligned(pq_match, 4) || misaligned(out, 8) || misaligned(ws, 8))
    return PEA_E_ALIGN;
  Inst T;
  const size_t need = inst_layout(d, ws, &T);
  if (!ws || ws_bytes < need) return PEA_E_WORKSPACE;
  unsigned chunks, pgroups, sgroups;
  if (!pea::seg_grids((uint64_t)d->S, (uint64_t)d->capacity, (uint64_t)d->B, &chunks, &pgroups, &sgroups)) return PEA_E_UNSUPPORTED;

  LaunchChain chain(stream);
  chain(k_seg_pairs<true>, pgroups, kBlock, d->S, chunks, T.cap, pred, gt, T.img, T.pairs, d->max_id);
  chain(k_inst_marginals, sgroups, kBlock, T, aji_match, pq_match);
  chain(k_inst_scan, d->B, kBlock, T);
  chain(k_inst_pairs, sgroups, kBlock, T, d->match_iou, pq_match);
  chain(k_inst_walk, d->B, 64, T, aji_match);
  chain(k_inst_finish, sgroups, kBlock, T, out);
  return or_prepare_again(chain.rc, [&] { launch_table_init<kInstMagic>(ws, need, chain.s); });
}
