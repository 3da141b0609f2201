// pea_k_disc.hip -- the discriminative (pull / push) instance loss on the raw embedding (include/pea_disc.h): the per-image torch.unique,
// the Python loop over the ids and the dozen launches per id of scripts_*/loss/loss_discriminative.py as three streaming launches and
// two small per-cluster launches for the forward and one streaming launch for the backward.  The header states the semantics and the
// order of every operation; this comment says how the launches are laid out.
//
//   k_disc_sums      streaming: per (image, id) the sum of e per channel and the pixel count, and the number of out-of-range labels
//   k_disc_clusters  one workgroup per image: compacts the present ids in ascending order, mu_c, n_c, C_b, k_c, w_c, the pair term, the
//                    norm term and their parts of G_c; puts the rows it read back to zero
//   k_disc_pull      streaming, mu at hand (cache-resident): h_p, the per-image sum of w_c h_p^2, with NEED_GRAD the sums of h_p u_p
//   k_disc_finish    one workgroup: completes G_c / n_c, writes loss and stats, puts what it read back to zero
//   k_disc_bwd       streaming: de
//
// The segmented reduction (k_disc_sums, k_disc_pull).  A WAVE owns 256 consecutive pixels of one image, a lane one quad of four
// x-adjacent pixels (pixel 4 lane + i), whose labels it keeps in registers.  Channels are taken four at a time: every lane loads its
// quad of the four planes once (1 KiB per wave and plane, wide where aligned), then the wave PEELS its ids over the registers: it
// takes the id of the first lane that still has an open pixel, every lane marks its pixels of that id and closes them, a lane adds
// its marked values in ascending order, the 64 lanes are added by xor butterflies (a fixed order; four side by side), and lanes
// 0 .. 3 convert the four totals to fixed-point digits and add them into the row of (image, id) with integer atomics
// (csrc/pea_loss.h: digits_accumulate).  Memory is touched once per channel whatever the number of ids; an id costs a round of
// shuffles.  A wave of 256 distinct ids takes 256 rounds and is served all the same.  (Built and measured first: ids outside, channels
// inside, only the marked lanes loading -- a row of a 256-wide image crosses six instances, and every round waited for memory:
// 169 us and 222 us for the two passes at the BBBC shape.)
// There is no workgroup-side cache of "the ids of my run": a wave's partial goes straight to the global table, at most one add per (id
// in the wave's run, channel, digit).  A cache that combines the four waves in f32 would round where the integer table does not, so
// the result would depend on whether an id fitted into the cache; adding the wave partials as integers has no such case.  At the
// BBBC crop shape that is 2048 waves x 1 - 2 ids x 16 channels x 2 - 3 digits, some 120 k atomics over 15 k addresses.
//
// Measured on an MI355X at 8 x 16 x 256 x 256 with about 40 ids per image (profiles/disc_ab.json), kernel trace:
// sums 34 us, clusters 26 us, pull 85 us, finish 16 us, backward 25 us.  The backward runs near the memory system's rate; the two
// reducing passes are bound by latency (four dependent rounds of loads per wave, then shuffles and atomics per id), the two
// per-cluster launches by their chain of dependent steps in one workgroup.
#include "../../include/pea_disc.h"
#include "pea_dispatch.h"
#include "pea_stream.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

constexpr int kCh = 4;                                // channels in flight per lane: independent loads and butterflies
constexpr int kClBlock = 1024;                        // lanes of the two per-cluster launches
constexpr int kClWaves = kClBlock / 64;
constexpr unsigned kDiscMagic = 0x50454144u;          // "PEAD"
constexpr unsigned kKnownFlags = PEA_DISC_BACKGROUND | PEA_DISC_NEED_GRAD;
constexpr int kHdrWords = kTableHdrWords;             // u64 words: [0] magic, [1] n_bad
constexpr int kImgWords = 4;                          // per image: three digit words of sum w_c h_p^2, flags
constexpr int kRowHead = 2;                           // per (image, id): [0] count, [1] flags, then three digit words per channel
static_assert(PEA_DISC_MAX_IDS % kClBlock == 0 && PEA_DISC_MAX_D == 64, "the compaction's chunks; one lane per channel");

// the workspace: header, per-image accumulators, rows
struct Tables {
  u64* hdr;
  u64* img;
  u64* rows;
  int R;  // words per row
};
// what the forward leaves for the backward (pea_disc_context_bytes)
struct Ctx {
  double* img;  // [B][2] dist_b, reg_b
  int* cb;      // [B] C_b
  int* n;       // [B][N] n_c (0: not counted)
  int* ids;     // [B][N] the counted ids of the image in ascending order, then zeros
  float* kc;    // [B][N] 2 alpha / (B C_b n_c)
  float* w;     // [B][N] 1 / (C_b n_c)
  float* mu;    // [B][N][D]
  float* gn;    // [B][N][D] G_c / n_c
};
struct DiscK {
  int B, D, N, bg, grad;
  float dv, dd2, alpha, beta, gamma;  // dd2 = 2 delta_d
};

inline size_t tables_layout(const PeaDiscDesc* d, void* base, Tables* t) {
  const uint64_t B = (uint64_t)d->B, R = kRowHead + 3 * (uint64_t)d->D;
  Carver c(base);
  t->hdr = c.take<u64>(kHdrWords);
  t->img = c.take<u64>(kImgWords * B);
  t->rows = c.take<u64>(mul_sat(B * (uint64_t)d->num_ids, R));
  t->R = (int)R;
  return c.bytes();
}
inline size_t ctx_layout(const PeaDiscDesc* d, void* base, Ctx* x) {
  const uint64_t B = (uint64_t)d->B, BN = B * (uint64_t)d->num_ids, BND = mul_sat(BN, (uint64_t)d->D);
  Carver c(base);
  x->img = c.take<double>(2 * B);
  x->cb = c.take<int>(B);
  x->n = c.take<int>(BN);
  x->ids = c.take<int>(BN);
  x->kc = c.take<float>(BN);
  x->w = c.take<float>(BN);
  x->mu = c.take<float>(BND);
  x->gn = c.take<float>(BND);
  return c.bytes();
}

// wave_sum(float) of pea_stream.h written out for k_disc_pull, which came out 0.8 % slower behind the template (profiles/README.md)
__device__ __forceinline__ float bfly(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- a wave's pixels (the peel of their ids: pea_stream.h) ------------------------------------------------------------------------------
struct WaveRun {
  size_t i0;        // the lane's first pixel
  int nv;           // its valid pixels (0 .. 4)
  int lab[kQuad];   // their labels (-1 past the end)
  unsigned act;     // bit i: pixel i is valid and counted
  int bad;          // the lane's out-of-range labels
};

__device__ __forceinline__ void wave_labels(WaveRun& W, const int32_t* __restrict__ lp, size_t w0, size_t S, int N, int bg, int lane) {
  W.i0 = w0 + (size_t)lane * kQuad;
  W.nv = quad_nv(W.i0, S);
  W.act = 0;
  W.bad = 0;
  int l[kQuad] = {-1, -1, -1, -1};
  if (W.nv == kQuad && ((uintptr_t)(lp + W.i0) & 15) == 0) {
    const iquad_t v = *(const iquad_t*)(lp + W.i0);
    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < kQuad; ++i)
      if (i < W.nv) l[i] = lp[W.i0 + i];
  }
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    W.lab[i] = l[i];
    if (i < W.nv) {
      if ((unsigned)l[i] >= (unsigned)N) ++W.bad;
      else if (l[i] != 0 || bg) W.act |= 1u << i;
    }
  }
}

// kCh channel planes of the lane's quad, d0 first; past the last channel the last one again (loaded, never used)
template <typename T>
__device__ __forceinline__ void ld_group(const WaveRun& W, const T* __restrict__ eb, int d0, int D, size_t S, float (&v)[kCh][kQuad]) {
#pragma unroll
  for (int u = 0; u < kCh; ++u) {
    const int d = d0 + u < D ? d0 + u : D - 1;
    ld_quad(eb + (size_t)d * S + W.i0, W.nv, v[u]);
  }
}

// For every id of the wave: the lane's marked values of each of the kCh channels added in ascending pixel order, the lanes by
// butterflies, and lanes 0 .. kCh - 1 add the totals of channels d0 .. into the id's row.  first(row, mm): once per id, before the adds.
template <typename F>
__device__ __forceinline__ void reduce_group(const WaveRun& W, const float (&t)[kCh][kQuad], int d0, int D, u64* rows, size_t bN, int R,
                                             int lane, F&& first) {
  unsigned open = W.act, mm;
  int cur;
  while (peel(W.lab, open, cur, mm)) {
    u64* row = rows + (bN + (size_t)cur) * R;
    first(row, mm);
    float s[kCh];
#pragma unroll
    for (int u = 0; u < kCh; ++u) {
      s[u] = 0.f;
#pragma unroll
      for (int i = 0; i < kQuad; ++i)
        if ((mm >> i) & 1u) s[u] += t[u][i];
    }
    wave_sums(s);
    float mine = 0.f;
#pragma unroll
    for (int u = 0; u < kCh; ++u)
      if (lane == u) mine = s[u];
    if (lane < kCh && d0 + lane < D) digits_accumulate(row + kRowHead + 3 * (d0 + lane), (unsigned*)(row + 1), mine);
  }
}

// ---- forward 1: sums and counts -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_disc_sums(const size_t S, const unsigned chunks, const DiscK K, const T* __restrict__ e,
                                                      const int32_t* __restrict__ labels, const Tables Tb) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(at.chunk, S, &w0)) return;
  WaveRun W;
  wave_labels(W, labels + b * S, w0, S, K.N, K.bg, lane);
  const T* __restrict__ eb = e + b * K.D * S;
#pragma unroll 1
  for (int d0 = 0; d0 < K.D; d0 += kCh) {
    float v[kCh][kQuad];
    ld_group(W, eb, d0, K.D, S, v);
    reduce_group(W, v, d0, K.D, Tb.rows, b * K.N, Tb.R, lane, [&](u64* row, unsigned mm) {
      if (d0 == 0) {  // the pixel count, once
        const int cnt = wave_sum((int)__popc(mm));
        if (lane == 0) PEA_ATOM_ADD(row, (u64)cnt);
      }
    });
  }
  const int bad = wave_sum(W.bad);
  if (lane == 0 && bad) PEA_ATOM_ADD(Tb.hdr + 1, (u64)bad);
}

// ---- forward 2: the clusters of one image ---------------------------------------------------------------------------------------------
// f64 sum over the workgroup in a fixed order: the waves' lane 0 values, wave 0 first (every lane of a wave holds the wave's value)
__device__ __forceinline__ double block_sum_of_waves(double v, double* s_red, int lane, int wave) {
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kClWaves; ++w) t += s_red[w];
  return t;
}

__global__ __launch_bounds__(kClBlock) void k_disc_clusters(const DiscK K, const Tables Tb, const Ctx C) {
  __shared__ int s_ids[PEA_DISC_MAX_IDS];
  __shared__ int s_wtot[kClWaves];
  __shared__ double s_red[kClWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t b = blockIdx.x, bN = b * K.N;
  const int per = (K.N + kClBlock - 1) / kClBlock;

  // the present ids in ascending order: lane t looks at ids [t per, (t + 1) per)
  int mine = 0;
  for (int i = 0; i < per; ++i) {
    const int id = t * per + i;
    if (id < K.N && Tb.rows[(bN + id) * Tb.R] != 0 && (id != 0 || K.bg)) ++mine;
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_wtot[wave] = incl;
  __syncthreads();
  int pos = incl - mine, Cb = 0;
  for (int w = 0; w < kClWaves; ++w) {
    if (w < wave) pos += s_wtot[w];
    Cb += s_wtot[w];
  }
  for (int i = 0; i < per; ++i) {
    const int id = t * per + i;
    if (id >= K.N) break;
    u64* row = Tb.rows + (bN + id) * Tb.R;
    const u64 cnt = row[0];
    const bool on = cnt != 0 && (id != 0 || K.bg);
    const int n = on ? (int)cnt : 0;
    if (on) {
      s_ids[pos] = id;
      C.ids[bN + pos] = id;
      ++pos;
    }
    C.n[bN + id] = n;
    C.kc[bN + id] = on ? (float)(2.0 * (double)K.alpha / ((double)K.B * (double)Cb * (double)n)) : 0.f;
    C.w[bN + id] = on ? (float)(1.0 / ((double)Cb * (double)n)) : 0.f;
  }
  for (int i = Cb + t; i < K.N; i += kClBlock) C.ids[bN + i] = 0;
  __syncthreads();

  // mu_c = (float)(sum / n_c); the digits go back to zero
  for (int idx = t; idx < K.N * K.D; idx += kClBlock) {
    const int id = idx / K.D, d = idx - id * K.D;
    const int n = C.n[bN + id];
    float m = 0.f;
    if (n > 0) {
      u64* row = Tb.rows + (bN + id) * Tb.R;
      u64* a = row + kRowHead + 3 * d;
      const double sum = loss_value(a[0], a[1], a[2], *(const unsigned*)(row + 1));
      a[0] = 0; a[1] = 0; a[2] = 0;
      m = (float)(sum / (double)n);
    }
    C.mu[(bN + id) * K.D + d] = m;
    C.gn[(bN + id) * K.D + d] = 0.f;
  }
  __syncthreads();
  for (int i = t; i < Cb; i += kClBlock) {
    u64* row = Tb.rows + (bN + s_ids[i]) * Tb.R;
    row[0] = 0;
    row[1] = 0;
  }

  // a wave per cluster c; its lanes are 64 / Dp groups of Dp channels (Dp: D rounded up to a power of two), group g walks the other
  // clusters c' = g, g + 64 / Dp, ..
  int Dp = 1;
  while (Dp < K.D) Dp <<= 1;
  const int G = 64 / Dp, g = lane / Dp, dl = lane - g * Dp;
  const bool chan = dl < K.D;
  const float creg = Cb ? (float)((double)K.gamma / ((double)K.B * (double)Cb)) : 0.f;
  const float cdist = Cb > 1 ? (float)(-2.0 * (double)K.beta / ((double)K.B * (double)Cb * (double)(Cb - 1))) : 0.f;
  double reg_acc = 0.0, pair_acc = 0.0;
  for (int ci = wave; ci < Cb; ci += kClWaves) {
    const int id = s_ids[ci];
    const float mc = chan ? C.mu[(bN + id) * K.D + dl] : 0.f;
    float ss = mc * mc;
    for (int o = Dp >> 1; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float nr = sqrtf(ss);
    reg_acc += (double)nr;
    const float greg = nr == 0.f ? 0.f : creg * __fdiv_rn(mc, nr);
    float gd = 0.f;
    double hs = 0.0;
    if (Cb > 1) {
      for (int c0 = 0; c0 < Cb; c0 += G) {
        const int c2 = c0 + g;
        const bool valid = c2 < Cb && c2 != ci;
        const int id2 = s_ids[c2 < Cb ? c2 : Cb - 1];
        const float m2 = chan ? C.mu[(bN + id2) * K.D + dl] : 0.f;
        const float df = mc - m2;
        float q = df * df;
        for (int o = Dp >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float dist = sqrtf(q);
        const float x = K.dd2 - dist;
        const float hinge = x < 0.f ? 0.f : x;
        if (valid) {
          hs += (double)(hinge * hinge);
          gd += dist == 0.f ? 0.f : __fdiv_rn(hinge, dist) * df;
        }
      }
      for (int o = Dp; o < 64; o <<= 1) {
        gd += __shfl_xor(gd, o, 64);
        hs += __shfl_xor(hs, o, 64);
      }
    }
    pair_acc += hs;
    if (g == 0 && chan) C.gn[(bN + id) * K.D + dl] = cdist * gd + greg;
  }
  const double reg_sum = block_sum_of_waves(reg_acc, s_red, lane, wave);
  const double pair_sum = block_sum_of_waves(pair_acc, s_red, lane, wave);
  if (t == 0) {
    C.cb[b] = Cb;
    C.img[2 * b + 0] = Cb > 1 ? pair_sum / ((double)Cb * (double)(Cb - 1)) / 2.0 : 0.0;
    C.img[2 * b + 1] = Cb ? reg_sum / (double)Cb : 0.0;
  }
}

// ---- forward 3: the pull term ---------------------------------------------------------------------------------------------------------
template <typename T, bool GRAD>
__global__ __launch_bounds__(kBlock) void k_disc_pull(const size_t S, const unsigned chunks, const DiscK K, const T* __restrict__ e,
                                                      const int32_t* __restrict__ labels, const Tables Tb, const Ctx C) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const int lane = threadIdx.x & 63;
  size_t w0;
  if (!wave_start(at.chunk, S, &w0)) return;
  WaveRun W;
  wave_labels(W, labels + b * S, w0, S, K.N, K.bg, lane);
  const T* __restrict__ eb = e + b * K.D * S;
  const size_t bN = b * K.N;

  // |e_p - mu_c|: every lane gathers the means of its own pixels' ids (a few KB per image: cache-resident)
  const float* mp[kQuad];
  float ss[kQuad];
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    mp[i] = C.mu + (bN + (size_t)(((W.act >> i) & 1u) ? W.lab[i] : 0)) * K.D;
    ss[i] = 0.f;
  }
#pragma unroll 1
  for (int d0 = 0; d0 < K.D; d0 += kCh) {
    float v[kCh][kQuad];
    ld_group(W, eb, d0, K.D, S, v);
#pragma unroll
    for (int u = 0; u < kCh; ++u) {
      if (d0 + u < K.D) {
#pragma unroll
        for (int i = 0; i < kQuad; ++i) {
          const float df = v[u][i] - mp[i][d0 + u];
          ss[i] += df * df;
        }
      }
    }
  }
  float sc[kQuad], h2[kQuad];
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    const float nr = sqrtf(ss[i]);
    const float x = nr - K.dv;
    const float h = x < 0.f ? 0.f : x;
    sc[i] = nr == 0.f ? 0.f : __fdiv_rn(h, nr);
    h2[i] = h * h;
  }
  {  // var_b: per id the wave's sum of h^2, weighted, into the image's accumulator
    unsigned open = W.act, mm;
    int cur;
    while (peel(W.lab, open, cur, mm)) {
      float hh = 0.f;
#pragma unroll
      for (int i = 0; i < kQuad; ++i)
        if ((mm >> i) & 1u) hh += h2[i];
      hh = bfly(hh);
      if (lane == 0) digits_accumulate(Tb.img + kImgWords * b, (unsigned*)(Tb.img + kImgWords * b + 3), hh * C.w[bN + cur]);
    }
  }
  if constexpr (GRAD) {
#pragma unroll 1
    for (int d0 = 0; d0 < K.D; d0 += kCh) {
      float v[kCh][kQuad];
      ld_group(W, eb, d0, K.D, S, v);
#pragma unroll
      for (int u = 0; u < kCh; ++u) {
        const int d = d0 + u < K.D ? d0 + u : K.D - 1;
#pragma unroll
        for (int i = 0; i < kQuad; ++i) v[u][i] = sc[i] * (v[u][i] - mp[i][d]);
      }
      reduce_group(W, v, d0, K.D, Tb.rows, bN, Tb.R, lane, [](u64*, unsigned) {});
    }
  }
}

// ---- forward 4: the finish --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kClBlock) void k_disc_finish(const DiscK K, const Tables Tb, const Ctx C, float* __restrict__ loss,
                                                          double* __restrict__ stats) {
  const int t = threadIdx.x;
  const bool good = *(const unsigned*)Tb.hdr == kDiscMagic;
  const double qnan = __builtin_nan("");
  if (K.grad) {
    for (int b = 0; b < K.B; ++b) {
      const size_t bN = (size_t)b * K.N;
      const int Cb = C.cb[b];
      for (int idx = t; idx < Cb * K.D; idx += kClBlock) {
        const int ci = idx / K.D, d = idx - ci * K.D;
        const size_t bc = bN + C.ids[bN + ci];
        u64* row = Tb.rows + bc * Tb.R;
        u64* a = row + kRowHead + 3 * d;
        const float sum = (float)loss_value(a[0], a[1], a[2], *(const unsigned*)(row + 1));
        a[0] = 0; a[1] = 0; a[2] = 0;
        float* gp = C.gn + bc * K.D + d;
        *gp = __fdiv_rn((-C.kc[bc] * sum) + *gp, (float)C.n[bc]);
      }
    }
    __syncthreads();
    for (int b = 0; b < K.B; ++b) {
      const size_t bN = (size_t)b * K.N;
      const int Cb = C.cb[b];
      for (int ci = t; ci < Cb; ci += kClBlock) Tb.rows[(bN + C.ids[bN + ci]) * Tb.R + 1] = 0;
    }
  }
  for (int b = t; b < K.B; b += kClBlock) {
    u64* a = Tb.img + (size_t)kImgWords * b;
    const double var = loss_value(a[0], a[1], a[2], (unsigned)a[3]);
    a[0] = 0; a[1] = 0; a[2] = 0; a[3] = 0;
    double* o = stats + PEA_DISC_STATS + 4 * (size_t)b;
    o[0] = good ? var : qnan;
    o[1] = good ? C.img[2 * b + 0] : qnan;
    o[2] = good ? C.img[2 * b + 1] : qnan;
    o[3] = good ? (double)C.cb[b] : qnan;
  }
  __syncthreads();
  if (t == 0) {
    const u64 nbad = Tb.hdr[1];
    Tb.hdr[1] = 0;
    double v = 0.0, ds = 0.0, r = 0.0;
    for (int b = 0; b < K.B; ++b) {
      const double* o = stats + PEA_DISC_STATS + 4 * (size_t)b;
      v += o[0]; ds += o[1]; r += o[2];
    }
    const double B = (double)K.B;
    const bool ok = good && nbad == 0;
    const double l = ((double)K.alpha * v + (double)K.beta * ds + (double)K.gamma * r) / B;
    stats[0] = ok ? l : qnan;
    stats[1] = ok ? v / B : qnan;
    stats[2] = ok ? ds / B : qnan;
    stats[3] = ok ? r / B : qnan;
    stats[4] = good ? (double)nbad : qnan;
    loss[0] = ok ? (float)l : __builtin_nanf("");
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_disc_bwd(const size_t S, const unsigned chunks, const DiscK K, const T* __restrict__ e,
                                                     const int32_t* __restrict__ labels, const Ctx C, const float* __restrict__ dloss,
                                                     T* __restrict__ de) {
  const BlockAt at = block_at(chunks);
  const size_t b = at.plane;
  const size_t i0 = quad_start(at.chunk);
  if (i0 >= S) return;
  const int nv = quad_nv(i0, S);
  const int32_t* __restrict__ lp = labels + b * S + i0;
  const float dl = dloss ? dloss[0] : 1.0f;

  size_t bc[kQuad];
  bool on[kQuad];
  float ss[kQuad], sc[kQuad], kc[kQuad];
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    const int l = i < nv ? lp[i] : -1;
    const bool in = (unsigned)l < (unsigned)K.N;
    bc[i] = b * K.N + (size_t)(in ? l : 0);
    on[i] = in && C.n[bc[i]] > 0;
    ss[i] = 0.f;
  }
#pragma unroll 1
  for (int d = 0; d < K.D; ++d) {
    float v[kQuad];
    ld_quad(e + (b * K.D + d) * S + i0, nv, v);
#pragma unroll
    for (int i = 0; i < kQuad; ++i) {
      const float df = v[i] - (on[i] ? C.mu[bc[i] * K.D + d] : 0.f);
      ss[i] += df * df;
    }
  }
#pragma unroll
  for (int i = 0; i < kQuad; ++i) {
    const float nr = sqrtf(ss[i]);
    const float x = nr - K.dv;
    const float h = x < 0.f ? 0.f : x;
    sc[i] = nr == 0.f ? 0.f : __fdiv_rn(h, nr);
    kc[i] = on[i] ? C.kc[bc[i]] : 0.f;
  }
#pragma unroll 1
  for (int d = 0; d < K.D; ++d) {
    float v[kQuad], o[kQuad];
    ld_quad(e + (b * K.D + d) * S + i0, nv, v);
#pragma unroll
    for (int i = 0; i < kQuad; ++i) {
      o[i] = 0.f;
      if (on[i]) {
        const size_t k = bc[i] * K.D + d;
        o[i] = dl * (kc[i] * (sc[i] * (v[i] - C.mu[k])) + C.gn[k]);
      }
    }
    st_quad(de + (b * K.D + d) * S + i0, nv, o);
  }
}

// workgroups of a streaming launch over the images' pixels; false: S or the grid exceeds 2^31 - 1
inline bool disc_grid(const PeaDiscDesc* d, unsigned* chunks, unsigned* groups) {
  return d->S <= 0x7fffffffLL && stream_grid((uint64_t)d->S, (uint64_t)d->B, kQuadRun, chunks, groups);
}

inline DiscK disc_params(const PeaDiscDesc* d) {
  DiscK K;
  K.B = d->B; K.D = d->D; K.N = d->num_ids;
  K.bg = (d->flags & PEA_DISC_BACKGROUND) ? 1 : 0;
  K.grad = (d->flags & PEA_DISC_NEED_GRAD) ? 1 : 0;
  K.dv = d->delta_v; K.dd2 = 2.0f * d->delta_d;
  K.alpha = d->alpha; K.beta = d->beta; K.gamma = d->gamma;
  return K;
}

inline bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

}  // namespace

extern "C" int pea_disc_validate(const PeaDiscDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->D < 1 || d->S < 1) return PEA_E_DESC;
  if (d->num_ids < 1 || d->num_ids > PEA_DISC_MAX_IDS) return PEA_E_DESC;
  if (d->dtype != PEA_F32 && d->dtype != PEA_F16 && d->dtype != PEA_BF16) return PEA_E_DESC;
  if (d->flags & ~kKnownFlags) return PEA_E_DESC;
  if (!finite_nonneg(d->delta_v) || !finite_nonneg(d->delta_d)) return PEA_E_DESC;
  if (d->D > PEA_DISC_MAX_D) return PEA_E_UNSUPPORTED;
  return PEA_OK;
}

extern "C" size_t pea_disc_workspace_bytes(const PeaDiscDesc* d) {
  Tables t;
  return pea_disc_validate(d) ? 0 : tables_layout(d, nullptr, &t);
}

extern "C" size_t pea_disc_context_bytes(const PeaDiscDesc* d) {
  Ctx c;
  return pea_disc_validate(d) ? 0 : ctx_layout(d, nullptr, &c);
}

extern "C" int pea_disc_workspace_init(void* workspace, size_t bytes, void* stream) {
  return table_workspace_init<kDiscMagic>(workspace, bytes, stream);
}

extern "C" int pea_disc_loss_fwd(const PeaDiscDesc* d, const void* e, const int32_t* labels, float* loss, double* stats, void* ctx,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_disc_validate(d);
  if (vrc) return vrc;
  if (!e || !labels || !loss || !stats || !ctx) return PEA_E_NULL;
  if (misaligned(e, dtype_bytes(d->dtype)) || misaligned(labels, 4) || misaligned(loss, 4) || misaligned(stats, 8) || misaligned(ctx, 8) ||
      misaligned(workspace, 8))
    return PEA_E_ALIGN;
  Tables Tb;
  const size_t need = tables_layout(d, workspace, &Tb);
  if (!workspace || workspace_bytes < need) return PEA_E_WORKSPACE;
  unsigned chunks, groups;
  if (!disc_grid(d, &chunks, &groups)) return PEA_E_UNSUPPORTED;

  const DiscK K = disc_params(d);
  Ctx C;
  ctx_layout(d, ctx, &C);
  LaunchChain chain(stream);
  with_storage(d->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    chain(k_disc_sums<T>, groups, kBlock, d->S, chunks, K, (const T*)e, labels, Tb);
    chain(k_disc_clusters, d->B, kClBlock, K, Tb, C);
    if (K.grad) chain(k_disc_pull<T, true>, groups, kBlock, d->S, chunks, K, (const T*)e, labels, Tb, C);
    else chain(k_disc_pull<T, false>, groups, kBlock, d->S, chunks, K, (const T*)e, labels, Tb, C);
    chain(k_disc_finish, 1, kClBlock, K, Tb, C, loss, stats);
  });
  return or_prepare_again(chain.rc, [&] { launch_table_init<kDiscMagic>(workspace, need, chain.s); });
}

extern "C" int pea_disc_loss_bwd(const PeaDiscDesc* d, const void* e, const int32_t* labels, const void* ctx, const float* dloss, void* de,
                                 void* stream) {
  const int vrc = pea_disc_validate(d);
  if (vrc) return vrc;
  if (!e || !labels || !ctx || !de) return PEA_E_NULL;
  const size_t eb = dtype_bytes(d->dtype);
  if (misaligned(e, eb) || misaligned(de, eb) || misaligned(labels, 4) || misaligned(dloss, 4) || misaligned(ctx, 8)) return PEA_E_ALIGN;
  unsigned chunks, groups;
  if (!disc_grid(d, &chunks, &groups)) return PEA_E_UNSUPPORTED;
  const DiscK K = disc_params(d);
  Ctx C;
  ctx_layout(d, const_cast<void*>(ctx), &C);
  LaunchChain chain(stream);
  with_storage(d->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    chain(k_disc_bwd<T>, groups, kBlock, d->S, chunks, K, (const T*)e, labels, C, dloss, (T*)de);
  });
  return chain.rc;
}
