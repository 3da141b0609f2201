// pea_k_multi.hip -- up to four self losses per launch (include/pea_multi.h): the deep-supervision scales of the training loops
// (scripts_cvppp/main.py:284-287: embedding_loss on emd1..emd4 at 1/2 .. 1/16 resolution; scripts_ac3ac4/main.py:227-230: four
// embedding_loss_norm1 calls) as one forward, one loss finish and one backward instead of three launches per scale.
//
// The table of the launch -- per entry its pointers and the few descriptor fields the bodies read, offsets as int16 -- travels BY
// VALUE in the kernel arguments (KParams is ~900 bytes: four of them do not fit the 4 KB segment): no device-side table and no copy
// from host memory on the stream, so the calls can be captured into a HIP graph.  A workgroup serves one tile (256 consecutive
// pixels of one batch item) of one entry and finds the entry from the prefix of tile counts; the host puts the entry with the most
// tiles first.  The tiles are then walked XCD-aware like logical_tile() walks one image: every XCD takes a contiguous range of the
// concatenated tile list, so the rows a tile's neighbours live in are mostly rows its own XCD loads anyway.
//
// Gather-from-global form: the bodies compose the blocks of pea_gather.h, the same ones k_fwd_direct / k_bwd_direct (pea_direct.h)
// are made of, so affs and g carry the single direct calls' bits, and so does de in f32 and bf16 (an f16 de lies within one f16 ulp:
// st_rounded here, st there); only the loss partials are summed in an order of their own (below).  The largest table of the
// reference (B = 8 x 16 x 272^2 and below, f32) is 38 MB of embeddings: L2 / Infinity Cache resident.
// The body is a template of D (16 / 32), the mask type (none / u8 / f32) and the border; a table whose entries agree on the three
// (the four scales of one training loop do) takes the kernel instantiated for them, any other the kernel that branches per
// workgroup (the branch is uniform: a workgroup has one entry).
// Storage type T (float / __half / __bf16: what the embedding heads emit under autocast) is a template parameter too: e is loaded
// through ld() and de stored through st() (one rounding to nearest even per stored 16-bit value, NaN kept; st_rounded keeps the
// f32 result apart from the conversion), one element per lane, so nothing but the element's own alignment is asked of e / de / S.
// Everything in between is f32 in the f32 order: affs, g and the loss carry the f32 kernel's bits on the upcast embedding.  All
// entries of a table share T (table_fuses), so T never takes the per-workgroup branch: with_storage picks it on the host.
// ALL common-D / mask / border specialisations are instantiated for the 16-bit types as well (3 x (13 + 5) kernels): the four
// scales of a 16-bit training step agree on the three like the f32 ones and should not pay the branching kernel's registers
// (86 against 50 VGPRs in the forward at D = 16).  Cost: this file compiles in 26 s instead of 8 s, pea_k_multi_labels.hip in
// 11 s instead of 6 s; neither is the library's longest translation unit, a full parallel build took 189 s before and 180 s after.
// Loss partials: per offset a wave reduction and a fixed-order sum of the four waves, then loss_accumulate() into the entry's own
// state block (integer adds: order-independent, exact); k_loss_finish_multi is k_loss_finish (pea_loss.h) with a workgroup per entry.
#include "pea_multi_common.h"

using namespace pea;
using namespace pea::multi;

namespace {

enum { kMaskNone = 0, kMaskU8 = 1, kMaskF32 = 2 };

struct MFwdEntry {
  MGeom g;
  int mtype;     // kMask*
  unsigned act;  // activation bits of the affs output
  float gscale[kMaxK];      // 2 * lambda_i / N_i
  long long tbs, wbs, mbs;  // batch strides (elements) of target / weight / mask
  const void* e;  // [B, D, S] in the table's storage type
  const float* t;
  const float* w;
  const void* m;
  float* affs;
  float* gout;
  LossState* st;
};
struct MBwdEntry {
  MGeom g;
  const void* e;  // [B, D, S] in the table's storage type, and so is de
  const float* gin;
  const float* dloss;
  void* de;
};
static_assert(sizeof(MTable<MFwdEntry>) <= 4096 - 64, "the forward's table must fit the kernel-argument segment");
static_assert(sizeof(MTable<MBwdEntry>) <= 4096 - 64, "the tables must fit the kernel-argument segment");

// ------------------------------------------------------------------------------------------------
// forward: affs (nullable), g = d loss / d affs, the tile's loss partials
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int MT, int BORDER>
__device__ __forceinline__ void fwd_body(const MFwdEntry& E, int tile, float (*s_part)[kBlock / 64]) {
  const MGeom& G = E.g;
  const int b = tile / G.chunks;
  const int p = (tile - b * G.chunks) * kBlock + (int)threadIdx.x;
  const bool live = p < G.S;
  const size_t S = (size_t)G.S;
  const T* eb = (const T*)E.e + (size_t)b * D * S;
  const size_t kb = (size_t)b * G.K * S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  int x = 0, y = 0, z = 0;
  float ec[D];
  float inv_p = 0.f;
  if (live) {
    split_voxel(G, p, z, y, x);
    inv_p = inv_norm(load_vec(eb, S, p, ec), G.eps);
  }

  for (int i = 0; i < G.K; ++i) {
    float contrib = 0.f;
    if (live) {
      const int q = neighbour<BORDER>(G, z, y, x, G.off[i][0], G.off[i][1], G.off[i][2]);
      const float a = q >= 0 ? cosine_streamed(ec, inv_p, eb, S, q, G.eps) : 0.f;
      const size_t in = (size_t)i * S + p;
      if (E.affs) E.affs[kb + in] = act_affs(a, E.act);
      float g = 0.f;
      if (q >= 0) {
        float m = 1.f;
        if constexpr (MT == kMaskU8) m = (float)((const uint8_t*)E.m)[(size_t)b * E.mbs + in];
        if constexpr (MT == kMaskF32) m = ((const float*)E.m)[(size_t)b * E.mbs + in];
        g = loss_term(a, E.t[(size_t)b * E.tbs + in], E.w[(size_t)b * E.wbs + in], m, true, E.gscale[i], contrib);
      }
      E.gout[kb + in] = g;
    }
    const float v = wave_sum(contrib);
    if (lane == 0) s_part[i][wave] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < G.K) {
    const float* r = s_part[threadIdx.x];
    loss_accumulate(E.st, tile, (int)threadIdx.x, (r[0] + r[1]) + (r[2] + r[3]));
  }
}

// DS / MS / BS: the table's common D / mask type / border, or -1: read from the workgroup's entry
template <typename T, int DS, int MS, int BS>
__global__ __launch_bounds__(kBlock) void k_fwd_multi(const MTable<MFwdEntry> Tb) {
  __shared__ float s_part[kMaxK][kBlock / 64];
  int idx, tile;
  if (!find_entry(Tb, idx, tile)) return;  // the whole workgroup together
  const MFwdEntry& E = Tb.en[idx];
  with_value<DS, 16, 32>(E.g.D, [&](auto d) {
    with_value<MS, kMaskNone, kMaskU8, kMaskF32>(E.mtype, [&](auto m) {
      with_value<BS, PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(E.g.border, [&](auto bd) {
        fwd_body<T, decltype(d)::value, decltype(m)::value, decltype(bd)::value>(E, tile, s_part);
      });
    });
  });
}

// ------------------------------------------------------------------------------------------------
// backward, gather form: G(p) = sum_i g_i(p) nhat(p + o_i) + g_i(p - o_i) nhat(p - o_i),
//   de(p) = dloss * (G - ehat <ehat, G>) / n(p)        (G / eps when |e(p)| < eps)
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int BORDER>
__device__ __forceinline__ void bwd_body(const MBwdEntry& E, int tile) {
  const MGeom& Gm = E.g;
  const int b = tile / Gm.chunks;
  const int p = (tile - b * Gm.chunks) * kBlock + (int)threadIdx.x;
  if (p >= Gm.S) return;
  const size_t S = (size_t)Gm.S;
  const T* xb = (const T*)E.e + (size_t)b * D * S;
  const float* gb = E.gin + (size_t)b * Gm.K * S;
  const float dl = E.dloss ? E.dloss[0] : 1.f;

  int z, y, x;
  split_voxel(Gm, p, z, y, x);

  float xc[D], G[D] = {};
  const float nrm = sqrtf(load_vec(xb, S, p, xc));
  const float inv_p = 1.0f / fmaxf(nrm, Gm.eps);

  for (int i = 0; i < Gm.K; ++i) {
    const int oz = Gm.off[i][0], oy = Gm.off[i][1], ox = Gm.off[i][2];
#pragma unroll
    for (int role = 0; role < 2; ++role) {
      const int sg = role == 0 ? 1 : -1;
      const int q = neighbour<BORDER>(Gm, z, y, x, sg * oz, sg * oy, sg * ox);
      if (q < 0) continue;
      // the loss term lives at the first operand's pixel: p for role A, the neighbour for role B
      gather_pair(G, xb, S, q, gb[(size_t)i * S + (role == 0 ? p : q)], Gm.eps);
    }
  }
  project_store<true>((T*)E.de + (size_t)b * D * S, S, p, xc, G, nrm, inv_p, Gm.eps, dl);
}

template <typename T, int DS, int BS>
__global__ __launch_bounds__(kBlock) void k_bwd_multi(const MTable<MBwdEntry> Tb) {
  int idx, tile;
  if (!find_entry(Tb, idx, tile)) return;
  const MBwdEntry& E = Tb.en[idx];
  with_value<DS, 16, 32>(E.g.D, [&](auto d) {
    with_value<BS, PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(E.g.border, [&](auto bd) {
      bwd_body<T, decltype(d)::value, decltype(bd)::value>(E, tile);
    });
  });
}

}  // namespace

extern "C" {

int pea_multi_supported(const PeaDesc* const* descs, int n) { return table_fuses(descs, n) ? 1 : 0; }

int pea_affinity_fwd_multi(const PeaMultiFwd* entries, int n, void* workspace, size_t workspace_bytes, void* stream) {
  if (n < 1 || n > kMaxN) return PEA_E_DESC;
  if (!entries) return PEA_E_NULL;
  const PeaDesc* descs[kMaxN];
  for (int i = 0; i < n; ++i) {
    const PeaMultiFwd& A = entries[i];
    const int rc = pea_desc_validate(A.desc);  // (PEA_E_NULL for a missing descriptor)
    if (rc) return rc;
    if (!A.e || !A.target || !A.weight || !A.g_out || !A.loss_out) return PEA_E_NULL;
    if (misaligned(A.e, dtype_bytes(A.desc->dtype)) || misaligned(A.affs, 4) || misaligned(A.g_out, 4) || misaligned(A.target, 4) ||
        misaligned(A.weight, 4) || misaligned(A.loss_out, 4) || ((A.desc->flags & PEA_FLAG_MASK_F32) && misaligned(A.mask, 4)))
      return PEA_E_ALIGN;
    descs[i] = A.desc;
  }
  if (misaligned(workspace, 8)) return PEA_E_ALIGN;
  if (!workspace || workspace_bytes / sizeof(LossState) < (size_t)n) return PEA_E_WORKSPACE;
  if (!table_fuses(descs, n)) return PEA_E_UNSUPPORTED;

  int order[kMaxN], B[kMaxN];
  tile_order(descs, n, order);
  MTable<MFwdEntry> T;
  MFinTable F;
  memset(&T, 0, sizeof(T));
  memset(&F, 0, sizeof(F));
  T.n = n;
  LossState* states = (LossState*)workspace;
  for (int j = 0; j < n; ++j) {
    const int i = order[j];  // entry i of the caller is entry j of the launch; its loss state stays state i
    const PeaMultiFwd& A = entries[i];
    const PeaDesc* d = A.desc;
    MFwdEntry& E = T.en[j];
    E.g = make_geom(d);
    B[j] = d->B;
    E.mtype = !A.mask ? kMaskNone : (d->flags & PEA_FLAG_MASK_F32) ? kMaskF32 : kMaskU8;
    E.act = d->flags & kActMask;
    const long long dense = (long long)d->K * E.g.S;
    E.tbs = d->target_bstride ? d->target_bstride : dense;
    E.wbs = d->weight_bstride ? d->weight_bstride : dense;
    E.mbs = d->mask_bstride ? d->mask_bstride : dense;
    E.e = A.e; E.t = A.target; E.w = A.weight; E.m = A.mask; E.affs = A.affs; E.gout = A.g_out;
    E.st = states + i;
    fill_finish(F.en[i], d, states + i, A.loss_out);
    for (int k = 0; k < d->K; ++k) E.gscale[k] = (float)(2.0 * (double)d->lambda[k] / normaliser(d, k));
  }
  const dim3 grid = place_tiles(T, B), blk(kBlock);
  hipStream_t s = (hipStream_t)stream;
  const int cd = common(n, [&](int j) { return T.en[j].g.D; }), cm = common(n, [&](int j) { return T.en[j].mtype; }),
            cb = common(n, [&](int j) { return T.en[j].g.border; });
  with_storage(descs[0]->dtype, [&](auto tg) {  // (table_fuses: one storage type for the whole table)
    using ST = typename decltype(tg)::type;
    if (cd >= 0 && cm >= 0 && cb >= 0) {
      return with_width<16, 32>(cd, [&](auto dw) {
        return with_width<kMaskNone, kMaskU8, kMaskF32>(cm, [&](auto mt) {
          return with_width<PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(cb, [&](auto bd) {
            return launch<k_fwd_multi<ST, decltype(dw)::value, decltype(mt)::value, decltype(bd)::value>>(grid, blk, 0, s, T);
          });
        });
      });
    }
    return launch<k_fwd_multi<ST, -1, -1, -1>>(grid, blk, 0, s, T);
  });
  int rc = hip_rc();
  if (!rc) {
    launch_loss_finish_multi(F, n, s);
    rc = hip_rc();
  }
  if (rc) {  // (run_fwd of pea_abi.hip: the states must be zero between calls, and only the finish puts them back)
    launch_loss_state_init(states, n, s);
    (void)hipGetLastError();
  }
  return rc;
}

int pea_affinity_bwd_multi(const PeaMultiBwd* entries, int n, void* stream) {
  if (n < 1 || n > kMaxN) return PEA_E_DESC;
  if (!entries) return PEA_E_NULL;
  const PeaDesc* descs[kMaxN];
  for (int i = 0; i < n; ++i) {
    const PeaMultiBwd& A = entries[i];
    const int rc = pea_desc_validate(A.desc);
    if (rc) return rc;
    if (!A.e || !A.g || !A.de) return PEA_E_NULL;
    const size_t es = dtype_bytes(A.desc->dtype);
    if (misaligned(A.e, es) || misaligned(A.de, es) || misaligned(A.g, 4) || misaligned(A.dloss, 4)) return PEA_E_ALIGN;
    descs[i] = A.desc;
  }
  if (!table_fuses(descs, n)) return PEA_E_UNSUPPORTED;

  int order[kMaxN], B[kMaxN];
  tile_order(descs, n, order);
  MTable<MBwdEntry> T;
  memset(&T, 0, sizeof(T));
  T.n = n;
  for (int j = 0; j < n; ++j) {
    const PeaMultiBwd& A = entries[order[j]];
    MBwdEntry& E = T.en[j];
    E.g = make_geom(A.desc);
    B[j] = A.desc->B;
    E.e = A.e; E.gin = A.g; E.dloss = A.dloss; E.de = A.de;
  }
  const dim3 grid = place_tiles(T, B), blk(kBlock);
  hipStream_t s = (hipStream_t)stream;
  const int cd = common(n, [&](int j) { return T.en[j].g.D; }), cb = common(n, [&](int j) { return T.en[j].g.border; });
  with_storage(descs[0]->dtype, [&](auto tg) {
    using ST = typename decltype(tg)::type;
    if (cd >= 0 && cb >= 0) {
      return with_width<16, 32>(cd, [&](auto dw) {
        return with_width<PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(cb, [&](auto bd) {
          return launch<k_bwd_multi<ST, decltype(dw)::value, decltype(bd)::value>>(grid, blk, 0, s, T);
        });
      });
    }
    return launch<k_bwd_multi<ST, -1, -1>>(grid, blk, 0, s, T);
  });
  return hip_rc();
}

}  // extern "C"
