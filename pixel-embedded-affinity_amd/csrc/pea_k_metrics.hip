// pea_k_metrics.hip -- the validation pixel metrics on the affinity map (include/pea_metrics.h): MSE, BCE and the F1 counts of
// scripts_cvppp/main.py:395-399 and scripts_ac3ac4/main.py:339-351 as ONE streaming reduction launch and one small finish.
//
// A workgroup of 256 lanes owns a RUN of kRun = 4096 consecutive elements of one (b, c) plane of the WALKED tensor; a lane takes four
// steps of four consecutive elements (element (step * 256 + lane) * 4 + e of the run), so a step of a wave is 1 KiB of each tensor.
//   without STORE  the walk is the evaluated region, i.e. target / mask in their own (dense) order; pred and the weight map are read
//                  at origin + p -- x-rows that are not contiguous in pred when there is a crop
//   with STORE     the walk is ALL of pred (every one of the CP channels, the whole [PZ, PY, PX] volume): every element is read,
//                  finished (divide / relu) and written back by the same lane; target / mask are read, and the sums taken, only where
//                  c < C and the voxel lies inside the region.  Channels c >= C are plain divide / relu passes.
// Where the region IS pred's volume (no crop: the 2D callers) both sides are contiguous.  The contiguous side of a lane's quad is one
// dwordx4 (one dword for a u8 mask) where its address is 16-byte (4-byte) aligned and the quad is whole, four scalar accesses
// otherwise -- the element-to-lane assignment and the order of the additions do not depend on it, so every element-aligned pointer
// gives the same bits.  The other side of a cropped walk is gathered element by element (the quad's first voxel is decoded with two
// divisions, the next three by stepping x, y, z).
//
// Arithmetic (pea_metrics.h): every step up to the terms is f32 and rounded on its own -- contraction is switched off for this file
// -- with the accurate logf.  A lane sums its sixteen terms in order, a wave reduces with __shfl_xor (a butterfly: a fixed order), the
// four waves meet in LDS and lane 0 adds the at most five partials into the integer accumulators of csrc/pea_loss.h: state q (0 mse,
// 1 bce, 2 tp, 3 fp, 4 fn), index c, slot = workgroup number.  The counts of a workgroup are f32 integers <= 4096, exact, and the
// accumulators add them as integers.  Sixteen non-negative terms per lane and eight levels of the tree keep the f32 partial within
// about 2^-20 of the exact sum.
// The finish (one workgroup, five waves: one per state) reads the 16 slots of every channel, writes out[1 + C][5] and zeroes what it
// read, so the block serves any later pea_* call on the stream.
//
// Expected cost (from instruction rates, not measured): 8 1/4 bytes per evaluated element read (pred, target, u8 mask; + 4 written
// with STORE), two logf per element: bandwidth-bound.
#include "../../include/pea_metrics.h"
#include "pea_dispatch.h"
#include "pea_stream.h"

#pragma clang fp contract(off)

using namespace pea;

namespace {

constexpr int kStates = 5;                      // mse, bce, tp, fp, fn
static_assert(kStates == PEA_METRICS_COLS, "one state per column");
constexpr unsigned kKnownFlags = PEA_MET_RELU | PEA_MET_DIVIDE | PEA_MET_STORE | PEA_MET_MASK_F32;

struct MetParams {
  int C, CP, CW;        // channels evaluated, channels of pred, channels walked (STORE: CP, else C)
  int Z, Y, X;          // the region = target / mask
  int PZ, PY, PX;       // pred / weight map
  int oz, oy, ox;
  unsigned chunks;      // workgroups per walked plane
  int dense;            // the region is pred's whole volume
  int relu;
  float lo, hi;
};

template <typename MT, bool DIVIDE, bool STORE>
__global__ __launch_bounds__(kBlock) void k_metrics(const MetParams P, float* __restrict__ pred, const float* __restrict__ wmap,
                                                    const float* __restrict__ target, const MT* __restrict__ mask,
                                                    LossState* __restrict__ st) {
  // blockIdx -> (b, c, chunk): uniform over the workgroup
  const BlockAt at = block_at(P.chunks);
  const unsigned c = at.plane % (unsigned)P.CW;
  const size_t b = at.plane / (unsigned)P.CW;
  const bool eval = !STORE || (int)c < P.C;  // channels c >= C of a STORE walk are finished and stored, not evaluated
  const size_t RS = (size_t)P.Z * P.Y * P.X, PS = (size_t)P.PZ * P.PY * P.PX;
  const size_t n = STORE ? PS : RS;  // elements of the walked plane
  float* __restrict__ pp = pred + (b * (size_t)P.CP + c) * PS;
  const size_t tplane = eval ? (b * (size_t)P.C + c) * RS : 0;
  const float* __restrict__ tp = target + tplane;
  const MT* __restrict__ mp = mask ? mask + tplane : nullptr;
  // the walk's extents along y and x (the region's, or with STORE pred's)
  const unsigned WY = STORE ? P.PY : P.Y, WX = STORE ? P.PX : P.X;

  float s_mse = 0.f, s_bce = 0.f, s_tp = 0.f, s_fp = 0.f, s_fn = 0.f;
  lane_run(at.chunk, n, [&](size_t i0, int nv) {
    float x[kQuad], w[kQuad], t[kQuad], m[kQuad];
    bool in[kQuad];
#pragma unroll
    for (int e = 0; e < kQuad; ++e) { x[e] = 0.f; w[e] = 1.0f; t[e] = 0.f; m[e] = 1.0f; in[e] = e < nv; }

    if (STORE || P.dense) {  // the walk's side of a STORE walk; without a crop pred, weight map, target and mask share the index
      ld_quad(pp + i0, nv, x);
      if (DIVIDE) ld_quad(wmap + i0, nv, w);
    }
    if (!STORE || (P.dense && eval)) {
      ld_quad(tp + i0, nv, t);
      if (mp) ld_quad(mp + i0, nv, m);
    }
    if (!P.dense && eval) {  // the other side of a cropped walk: the quad's first voxel in the walk's coordinates, then step by step
      CropCursor vox(i0, WY, WX);
#pragma unroll
      for (int e = 0; e < kQuad; ++e) {
        if (e < nv) {
          const unsigned z = (unsigned)vox.o, y = vox.y, xx = vox.x;
          if (STORE) {  // pred's voxel -> the region's, where it lies inside
            const unsigned rz = z - (unsigned)P.oz, ry = y - (unsigned)P.oy, rx = xx - (unsigned)P.ox;
            in[e] = rz < (unsigned)P.Z && ry < (unsigned)P.Y && rx < (unsigned)P.X;
            if (in[e]) {
              const size_t o = ((size_t)rz * P.Y + ry) * P.X + rx;
              t[e] = tp[o];
              if (mp) m[e] = (float)mp[o];
            }
          } else {      // the region's voxel -> pred's
            const size_t o = ((size_t)(z + (unsigned)P.oz) * P.PY + (y + (unsigned)P.oy)) * P.PX + (xx + (unsigned)P.ox);
            x[e] = pp[o];
            if (DIVIDE) w[e] = wmap[o];
          }
        }
        vox.step(WY, WX);
      }
    }

#pragma unroll
    for (int e = 0; e < kQuad; ++e) {
      float v = x[e];
      if (DIVIDE) v = __fdiv_rn(v, w[e]);
      if (P.relu) v = relu_keep_nan(v);
      x[e] = v;
      if (eval && in[e]) {
        const float a = v * m[e], tq = t[e] * m[e];
        const float u = clamp_keep_nan(v, P.lo, P.hi) * m[e];
        const float d = a - tq;
        const float sq = d * d;
        s_mse += sq;
        const float omu = 1.0f - u, omt = 1.0f - tq;
        const float p1 = tq * bce_log(logf(u)), p2 = omt * bce_log(logf(omu));  // nn.BCELoss's floor, a select: NaN stays NaN
        const float term = -(p1 + p2);
        s_bce += term;
        const bool gb = tq < 1.0f, pb = u <= 0.5f;
        s_tp += (gb && pb) ? 1.0f : 0.f;
        s_fp += (!gb && pb) ? 1.0f : 0.f;
        s_fn += (gb && !pb) ? 1.0f : 0.f;
      }
    }
    if (STORE) st_quad(pp + i0, nv, x);
  });
  if (!eval) return;  // (uniform: the whole workgroup leaves before the barrier)

  float q[kStates] = {s_mse, s_bce, s_tp, s_fp, s_fn};
  block_sums(q, [&](int k, float v) { loss_accumulate(st + k, (int)blockIdx.x, (int)c, v); });
}

// The finish: wave q reads state q, four channels per pass (lane = 16 * j + slot, as k_loss_finish), writes the table and puts the
// states back to zero.  n = B * Z * Y * X.
__global__ __launch_bounds__(64 * kStates) void k_metrics_finish(LossState* __restrict__ st, double* __restrict__ out, int C, double n) {
  __shared__ double s_v[kStates][PEA_MAX_K];
  __shared__ int s_bad;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, s = lane & (kLossSlots - 1), j = lane >> 4;
  LossState* __restrict__ S = st + q;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  if (lane == 0 && S->magic != kLossMagic) s_bad = 1;  // a state that was never initialised (pea_workspace_init): say so
  for (int k0 = 0; k0 < C; k0 += 4) {
    const int k = k0 + j;
    const bool on = k < C;
    const double v = loss_row_collect(S, k, s, on);
    if (on && s == 0) s_v[q][k] = v;
  }
  __syncthreads();
  const bool bad = s_bad != 0;
  const double qnan = __builtin_nan("");
  for (int i = threadIdx.x; i < kStates * C; i += 64 * kStates) {
    const int k = i / kStates, col = i - k * kStates;
    const double v = col < 2 ? s_v[col][k] / n : s_v[col][k];
    out[(size_t)(1 + k) * kStates + col] = bad ? qnan : v;
  }
  if (threadIdx.x < kStates) {
    const int col = threadIdx.x;
    double tot = 0.0;
    for (int k = 0; k < C; ++k) tot += s_v[col][k];
    out[col] = bad ? qnan : (col < 2 ? tot / ((double)C * n) : tot);
  }
}

}  // namespace

extern "C" int pea_metrics_validate(const PeaMetricsDesc* d) {
  if (!d) return PEA_E_NULL;
  if (d->B < 1 || d->C < 1 || d->CP < 1) return PEA_E_DESC;
  for (int a = 0; a < 3; ++a)
    if (d->dims[a] < 1 || d->pred_dims[a] < 1) return PEA_E_DESC;
  if (d->C > d->CP || d->C > PEA_MAX_K) return PEA_E_DESC;
  for (int a = 0; a < 3; ++a)
    if (d->origin[a] < 0 || (int64_t)d->origin[a] + d->dims[a] > (int64_t)d->pred_dims[a]) return PEA_E_DESC;
  if (d->flags & ~kKnownFlags) return PEA_E_DESC;
  if ((d->flags & PEA_MET_STORE) && !(d->flags & (PEA_MET_RELU | PEA_MET_DIVIDE))) return PEA_E_DESC;
  if ((d->flags & PEA_MET_DIVIDE) && d->B != 1) return PEA_E_DESC;
  if (!(d->clip_lo <= d->clip_hi)) return PEA_E_DESC;  // (false for a NaN bound too)
  return PEA_OK;
}

extern "C" size_t pea_metrics_workspace_bytes(void) { return kStates * sizeof(LossState); }

extern "C" int pea_affs_metrics(const PeaMetricsDesc* d, float* pred, const float* weight_map, const float* target, const void* mask,
                                double* out, void* workspace, size_t workspace_bytes, void* stream) {
  const int vrc = pea_metrics_validate(d);
  if (vrc) return vrc;
  const bool divide = d->flags & PEA_MET_DIVIDE, store = d->flags & PEA_MET_STORE, mf32 = mask && (d->flags & PEA_MET_MASK_F32);
  if (!pred || !target || !out || (divide && !weight_map)) return PEA_E_NULL;
  if (misaligned(pred, 4) || (divide && misaligned(weight_map, 4)) || misaligned(target, 4) || (mf32 && misaligned(mask, 4)) ||
      misaligned(out, 8) || misaligned(workspace, 8))
    return PEA_E_ALIGN;
  if (!workspace || workspace_bytes < pea_metrics_workspace_bytes()) return PEA_E_WORKSPACE;

  MetParams P;
  P.C = d->C; P.CP = d->CP; P.CW = store ? d->CP : d->C;
  P.Z = d->dims[0]; P.Y = d->dims[1]; P.X = d->dims[2];
  P.PZ = d->pred_dims[0]; P.PY = d->pred_dims[1]; P.PX = d->pred_dims[2];
  P.oz = d->origin[0]; P.oy = d->origin[1]; P.ox = d->origin[2];
  P.dense = P.Z == P.PZ && P.Y == P.PY && P.X == P.PX;
  P.relu = (d->flags & PEA_MET_RELU) ? 1 : 0;
  P.lo = d->clip_lo; P.hi = d->clip_hi;
  const uint64_t RS = mul_sat(mul_sat((uint64_t)P.Z, (uint64_t)P.Y), (uint64_t)P.X);
  const uint64_t PS = mul_sat(mul_sat((uint64_t)P.PZ, (uint64_t)P.PY), (uint64_t)P.PX);
  unsigned groups;
  if (!stream_grid(store ? PS : RS, mul_sat((uint64_t)d->B, (uint64_t)P.CW), kLaneRun, &P.chunks, &groups)) return PEA_E_UNSUPPORTED;

  LaunchChain chain(stream);
  LossState* st = (LossState*)workspace;
  with_bool(mf32, [&](auto mf) {
    using MT = std::conditional_t<decltype(mf)::value, float, uint8_t>;
    with_bool(divide, [&](auto dv) {
      with_bool(store, [&](auto sv) {
        chain(k_metrics<MT, decltype(dv)::value, decltype(sv)::value>, groups, kBlock, P, pred, weight_map, target, (const MT*)mask, st);
      });
    });
  });
  chain(k_metrics_finish, 1, 64 * kStates, st, out, P.C, (double)d->B * (double)RS);
  return or_prepare_again(chain.rc, [&] { launch_loss_state_init(st, kStates, chain.s); });
}
