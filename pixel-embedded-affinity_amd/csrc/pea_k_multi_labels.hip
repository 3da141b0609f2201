// pea_k_multi_labels.hip -- up to four self losses per launch evaluated straight from LABEL IMAGES (include/pea_multi_labels.h): the
// deep-supervision scales of the training loops (scripts_cvppp/main.py:284-287, scripts_ac3ac4/main.py:227-230) without target /
// weight / mask tensors and without the nearest-downsampled label images the providers make for them
// (scripts_cvppp/data/data_provider.py:200-203): every entry samples a label image with an integer step.
//
// Launches of a call: a memset node over the counts, k_count_multi (only where an entry brings no class-balance table),
// k_fwd_bwd_labels_multi, k_loss_finish_multi.  Table by value, tile walk, entry order and the loss finish are those of
// pea_k_multi.hip (pea_multi_common.h).
//
// k_count_multi: a workgroup counts t_i != 0 per channel over its 256 voxels -- ballot per wave, LDS, then one u32 atomic per
// (workgroup, channel) into scratch[entry][b][i].  Integer sums: the result does not depend on the order of arrival.
//
// k_fwd_bwd_labels_multi: gather-from-global form, composed of the blocks of pea_gather.h that k_fwd_multi / k_bwd_multi are made
// of (so affs and de carry their bits on the same targets): one lane per voxel p, its D channels and its label in registers.  The backward of p needs g_i(p - o_i), which depends on cos(e(p - o_i), e(p)), two labels and two
// table entries -- all of which the backward's gather reads anyway -- so no g map makes a round trip through memory.  Per offset
//   role A: q = p + o_i, a = cos(e(p), e(q)), t / m / w from L'(p), L'(q): affs, the loss partial, G += g_A ehat(q)
//   role B: q = p - o_i, the loss term lives at q: a (evaluated in q's operand order: the same bits role A of q computes), t / m / w
//           for the pair (q, p); its mask is [p - o_i did not leave the image]: G += g_B ehat(q)
// then de = dloss (G - ehat <ehat, G>) / n(p), G / eps where |e(p)| < eps.  The class-balance table of the workgroup's image is put
// into LDS by the prologue: copied from the caller's wtab, or evaluated from the counts with class_balance() (pea_gather.h), which
// k_weight_table (pea_fused_labels.h) calls too -- the same bits pea_label_weights writes.
// Label reads with a step are uncoalesced (a wave's 64 labels of one row span 64 * sx * 4 bytes); the label images are 1.2 MB per
// sample (544^2 int32) and L2-resident, every one of their cache lines is used by some scale, so they are not staged through LDS.
// The body is a template of the storage type T (float / __half / __bf16: ld() / st_rounded() around the unchanged f32 arithmetic,
// one element per lane, one storage type per table chosen on the host -- as pea_k_multi.hip says, which also states the build cost
// of instantiating every specialisation for the 16-bit types: 3 x 5 kernels here), of D and of the border; the three target flags
// are uniform scalars of the launch (they live in SGPRs: templating on them as well would multiply the instantiations by eight
// without freeing a vector register).  A table whose entries disagree on D or the border takes <-1, -1>, which branches per
// workgroup (uniform: a workgroup has one entry).
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage); no form spills to scratch (ScratchSize 0,
// no SGPR / VGPR spill), LDS 288 bytes (loss partials + the image's table), 48 bytes in the count kernel:
//   k_fwd_bwd_labels_multi<float, 16, CIRCULAR> 84 VGPRs   <16, CROP_ZERO> 84   <32, CIRCULAR> 131   <32, CROP_ZERO> 131   <-1, -1> 130
//   <__half, ..> 84 / 81 / 131 / 131 / 130   <__bf16, ..> 83 / 79 / 131 / 129 / 130
//   k_count_multi 11 VGPRs
#include "../../include/pea_multi_labels.h"
#include "pea_multi_common.h"

using namespace pea;
using namespace pea::multi;

namespace {

constexpr unsigned kTgtBits = PEA_TGT_PADDING | PEA_TGT_BOTH_FOREGROUND | PEA_TGT_MASK_INSIDE;

struct LabGeom {  // how an entry samples its label image
  int bs;         // batch stride (elements) = LZ * LY * LX
  int zs, ys, xs; // element strides of one step along z, y, x of THIS scale = sz * LY * LX, sy * LX, sx
};
struct MLabEntry {
  MGeom g;
  LabGeom l;
  unsigned act;          // activation bits of the affs output
  int pad;
  float gscale[kMaxK];   // 2 * lambda_i / N_i
  const void* e;         // [B, D, S] in the table's storage type, and so is de
  const int32_t* lab;
  const float* wtab;     // the caller's table, or NULL: evaluated from cnt
  unsigned* cnt;         // [B, K] counts of this entry in the scratch (written by k_count_multi), or NULL
  float* affs;
  const float* dloss;
  void* de;
  LossState* st;
};
struct MCntEntry {
  MGeom g;
  LabGeom l;
  const int32_t* lab;
  unsigned* cnt;
};
static_assert(sizeof(MTable<MLabEntry>) + 16 <= 4096 - 64, "the table must fit the kernel-argument segment");
static_assert(sizeof(MTable<MCntEntry>) + 16 <= 4096 - 64, "the table must fit the kernel-argument segment");

// target of the pair (own label, neighbour label): `inside` = the neighbour lies inside the image (un-wrapped)
__device__ __forceinline__ bool target_of(int lown, int lnb, bool inside, bool pad, bool fg) {
  const bool eq = (lown == lnb) & (!fg | ((lown > 0) & (lnb > 0)));
  return inside ? eq : pad;
}

// ------------------------------------------------------------------------------------------------
// counts of t_i != 0 per (entry, image, channel)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_count_multi(const MTable<MCntEntry> T, const unsigned lflags) {
  __shared__ unsigned s_cnt[kMaxK];
  int idx, tile;
  if (!find_entry(T, idx, tile)) return;  // the whole workgroup together
  const MCntEntry& E = T.en[idx];
  const MGeom& G = E.g;
  if ((int)threadIdx.x < kMaxK) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int b = tile / G.chunks;
  const int p = (tile - b * G.chunks) * kBlock + (int)threadIdx.x;
  const bool live = p < G.S;
  const bool pad = lflags & PEA_TGT_PADDING, fg = lflags & PEA_TGT_BOTH_FOREGROUND;
  const int32_t* lb = E.lab + (size_t)b * E.l.bs;
  int x = 0, y = 0, z = 0, lown = 0;
  if (live) {
    split_voxel(G, p, z, y, x);
    lown = lb[z * E.l.zs + y * E.l.ys + x * E.l.xs];
  }
  for (int i = 0; i < G.K; ++i) {
    bool t = false;
    if (live) {
      const int zz = z + G.off[i][0], yy = y + G.off[i][1], xx = x + G.off[i][2];
      const bool in = (unsigned)zz < (unsigned)G.Z && (unsigned)yy < (unsigned)G.Y && (unsigned)xx < (unsigned)G.X;
      const int lnb = in ? lb[zz * E.l.zs + yy * E.l.ys + xx * E.l.xs] : 0;
      t = target_of(lown, lnb, in, pad, fg);
    }
    const unsigned c = (unsigned)__popcll(__ballot(t));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[i], c);
  }
  __syncthreads();
  if ((int)threadIdx.x < G.K && s_cnt[threadIdx.x]) atomicAdd(&E.cnt[b * G.K + (int)threadIdx.x], s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// forward + backward
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int BORDER>
__device__ __forceinline__ void lab_body(const MLabEntry& E, int tile, unsigned lflags, float (*s_part)[kBlock / 64], float (*s_w)[2]) {
  const MGeom& Gm = E.g;
  const int b = tile / Gm.chunks;
  const int p = (tile - b * Gm.chunks) * kBlock + (int)threadIdx.x;
  const bool live = p < Gm.S;
  const size_t S = (size_t)Gm.S;
  const T* xb = (const T*)E.e + (size_t)b * D * S;
  const int32_t* lb = E.lab + (size_t)b * E.l.bs;
  float* ab = E.affs ? E.affs + (size_t)b * Gm.K * S : nullptr;
  const bool pad = lflags & PEA_TGT_PADDING, fg = lflags & PEA_TGT_BOTH_FOREGROUND, msk = lflags & PEA_TGT_MASK_INSIDE;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  // the class-balance table of this image: {weight of target-1 voxels, weight of target-0 voxels} per channel
  if ((int)threadIdx.x < Gm.K) {
    const int i = threadIdx.x;
    ClassWeights cw;
    if (E.wtab) {
      cw.pos = E.wtab[2 * ((size_t)b * Gm.K + i)];
      cw.neg = E.wtab[2 * ((size_t)b * Gm.K + i) + 1];
    } else {
      cw = class_balance(E.cnt[b * Gm.K + i], Gm.S);
    }
    s_w[i][0] = cw.pos;
    s_w[i][1] = cw.neg;
  }

  int x = 0, y = 0, z = 0, lown = 0;
  float xc[D], G[D] = {};
  float nrm = 0.f, inv_p = 0.f;
  if (live) {
    split_voxel(Gm, p, z, y, x);
    lown = lb[z * E.l.zs + y * E.l.ys + x * E.l.xs];
    nrm = sqrtf(load_vec(xb, S, p, xc));
    inv_p = 1.0f / fmaxf(nrm, Gm.eps);  // inv_norm(ss, eps)
  }
  __syncthreads();  // s_w

  for (int i = 0; i < Gm.K; ++i) {
    const int oz = Gm.off[i][0], oy = Gm.off[i][1], ox = Gm.off[i][2];
    const float wpos = s_w[i][0], wneg = s_w[i][1], gs = E.gscale[i];
    float contrib = 0.f;
    if (live) {
#pragma unroll
      for (int role = 0; role < 2; ++role) {
        const int sg = role == 0 ? 1 : -1;
        const int uz = z + sg * oz, uy = y + sg * oy, ux = x + sg * ox;
        // un-wrapped: a neighbour outside the image has no label, whatever the border does with the embedding
        const bool in = (unsigned)uz < (unsigned)Gm.Z && (unsigned)uy < (unsigned)Gm.Y && (unsigned)ux < (unsigned)Gm.X;
        const int q = neighbour<BORDER>(Gm, z, y, x, sg * oz, sg * oy, sg * ox);  // -1: the pair is cropped away
        const int lnb = in ? lb[uz * E.l.zs + uy * E.l.ys + ux * E.l.xs] : 0;
        const float t = target_of(lown, lnb, in, pad, fg) ? 1.f : 0.f;
        const float m = (msk && !in) ? 0.f : 1.f;
        const float w = t != 0.f ? wpos : wneg;
        float a = 0.f;
        if (q >= 0) {
          float v[D];
          const float inv_q = inv_norm(load_vec(xb, S, q, v), Gm.eps);
          // (role B: the term lives at q, whose forward multiplies e(q)[c] * e(p)[c] -- the product commutes, the sum's order is c)
          const float dot = dot_vec(xc, v);
          a = role == 0 ? dot * inv_p * inv_q : dot * inv_q * inv_p;  // the first operand's 1 / norm first, as cosine_streamed
          float term;  // the term's share of the loss: counted where it lives, at role A's pixel
          const float g = loss_term(a, t, w, m, true, gs, term);
          if (role == 0) contrib = term;
          accumulate(G, g * inv_q, v);
        }
        if (role == 0 && ab) ab[(size_t)i * S + p] = act_affs(a, E.act);
      }
    }
    const float v = wave_sum(contrib);
    if (lane == 0) s_part[i][wave] = v;
  }

  if (live) {
    const float dl = E.dloss ? E.dloss[0] : 1.f;
    project_store<true>((T*)E.de + (size_t)b * D * S, S, p, xc, G, nrm, inv_p, Gm.eps, dl);
  }
  __syncthreads();
  if ((int)threadIdx.x < Gm.K) {
    const float* r = s_part[threadIdx.x];
    loss_accumulate(E.st, tile, (int)threadIdx.x, (r[0] + r[1]) + (r[2] + r[3]));
  }
}

// DS / BS: the table's common D / border, or -1: read from the workgroup's entry
template <typename T, int DS, int BS>
__global__ __launch_bounds__(kBlock) void k_fwd_bwd_labels_multi(const MTable<MLabEntry> Tb, const unsigned lflags) {
  __shared__ float s_part[kMaxK][kBlock / 64];
  __shared__ float s_w[kMaxK][2];
  int idx, tile;
  if (!find_entry(Tb, idx, tile)) return;  // the whole workgroup together
  const MLabEntry& E = Tb.en[idx];
  with_value<DS, 16, 32>(E.g.D, [&](auto d) {
    with_value<BS, PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(E.g.border, [&](auto bd) {
      lab_body<T, decltype(d)::value, decltype(bd)::value>(E, tile, lflags, s_part, s_w);
    });
  });
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
bool labels_fuse(const PeaMultiLabels& A) {  // the label geometry of one entry (its descriptor is valid)
  const PeaDesc* d = A.desc;
  long long vol = d->B;
  for (int a = 0; a < 3; ++a) {
    if (A.label_step[a] < 1 || A.label_dims[a] < 1) return false;
    if ((long long)(d->dims[a] - 1) * A.label_step[a] + 1 > (long long)A.label_dims[a]) return false;
    vol *= A.label_dims[a];
    if (vol > 0x7fffffffLL) return false;
  }
  return true;
}

bool table_fuses_labels(const PeaMultiLabels* entries, int n, unsigned flags) {
  if (n < 1 || n > kMaxN || !entries || (flags & ~kTgtBits)) return false;
  const PeaDesc* descs[kMaxN];
  for (int i = 0; i < n; ++i) descs[i] = entries[i].desc;
  if (!table_fuses(descs, n)) return false;
  for (int i = 0; i < n; ++i)
    if ((descs[i]->flags & PEA_FLAG_MASK_F32) || !labels_fuse(entries[i])) return false;
  return true;
}

LabGeom make_lab_geom(const PeaMultiLabels& A) {
  LabGeom l;
  const int LY = A.label_dims[1], LX = A.label_dims[2];
  l.bs = A.label_dims[0] * LY * LX;
  l.zs = A.label_step[0] * LY * LX;
  l.ys = A.label_step[1] * LX;
  l.xs = A.label_step[2];
  return l;
}

}  // namespace

extern "C" {

int pea_multi_labels_supported(const PeaMultiLabels* entries, int n, unsigned flags) {
  return table_fuses_labels(entries, n, flags) ? 1 : 0;
}

size_t pea_multi_labels_scratch_bytes(const PeaMultiLabels* entries, int n) {
  if (n < 1 || n > kMaxN || !entries) return 0;
  size_t c = 0;
  for (int i = 0; i < n; ++i) {
    if (!entries[i].desc || pea_desc_validate(entries[i].desc) != PEA_OK) return 0;
    c += (size_t)entries[i].desc->B * entries[i].desc->K;
  }
  return c * sizeof(unsigned);
}

int pea_affinity_fwd_bwd_labels_multi(const PeaMultiLabels* entries, int n, unsigned flags, void* workspace, size_t workspace_bytes,
                                      void* scratch, size_t scratch_bytes, void* stream) {
  if (n < 1 || n > kMaxN) return PEA_E_DESC;
  if (!entries) return PEA_E_NULL;
  const PeaDesc* descs[kMaxN];
  bool counting = false;
  size_t cnt0[kMaxN + 1];  // entry i's first count
  cnt0[0] = 0;
  for (int i = 0; i < n; ++i) {
    const PeaMultiLabels& A = entries[i];
    const int rc = pea_desc_validate(A.desc);  // (PEA_E_NULL for a missing descriptor)
    if (rc) return rc;
    if (A.desc->flags & PEA_FLAG_MASK_F32) return PEA_E_DESC;  // the labels-in calls derive their own masks (include/pea.h)
    if (!A.e || !A.labels || !A.loss_out || !A.de) return PEA_E_NULL;
    const size_t es = dtype_bytes(A.desc->dtype);
    if (misaligned(A.e, es) || misaligned(A.de, es) || misaligned(A.labels, 4) || misaligned(A.wtab, 4) || misaligned(A.affs, 4) ||
        misaligned(A.loss_out, 4) || misaligned(A.dloss, 4))
      return PEA_E_ALIGN;
    descs[i] = A.desc;
    counting |= !A.wtab;
    cnt0[i + 1] = cnt0[i] + (size_t)A.desc->B * A.desc->K;
  }
  if (misaligned(workspace, 8) || misaligned(scratch, 4)) return PEA_E_ALIGN;
  if (!workspace || workspace_bytes / sizeof(LossState) < (size_t)n) return PEA_E_WORKSPACE;
  if (counting && (!scratch || scratch_bytes / sizeof(unsigned) < cnt0[n])) return PEA_E_WORKSPACE;
  if (!table_fuses_labels(entries, n, flags)) return PEA_E_UNSUPPORTED;

  int order[kMaxN], B[kMaxN], Bc[kMaxN];
  tile_order(descs, n, order);
  MTable<MLabEntry> T;
  MTable<MCntEntry> C;
  MFinTable F;
  memset(&T, 0, sizeof(T));
  memset(&C, 0, sizeof(C));
  memset(&F, 0, sizeof(F));
  T.n = n;
  LossState* states = (LossState*)workspace;
  for (int j = 0; j < n; ++j) {
    const int i = order[j];  // entry i of the caller is entry j of the launch; its loss state stays state i
    const PeaMultiLabels& A = entries[i];
    const PeaDesc* d = A.desc;
    MLabEntry& E = T.en[j];
    E.g = make_geom(d);
    E.l = make_lab_geom(A);
    B[j] = d->B;
    E.act = d->flags & kActMask;
    E.e = A.e; E.lab = A.labels; E.wtab = A.wtab; E.affs = A.affs; E.dloss = A.dloss; E.de = A.de;
    E.cnt = A.wtab ? nullptr : (unsigned*)scratch + cnt0[i];
    E.st = states + i;
    for (int k = 0; k < d->K; ++k) E.gscale[k] = (float)(2.0 * (double)d->lambda[k] / normaliser(d, k));
    fill_finish(F.en[i], d, states + i, A.loss_out);
    if (!A.wtab) {  // (the launch order is kept: most tiles first)
      MCntEntry& Ce = C.en[C.n];
      Ce.g = E.g; Ce.l = E.l; Ce.lab = A.labels; Ce.cnt = E.cnt;
      Bc[C.n++] = d->B;
    }
  }
  const dim3 blk(kBlock);
  hipStream_t s = (hipStream_t)stream;
  int rc = 0;
  if (counting) {
    const hipError_t me = hipMemsetAsync(scratch, 0, cnt0[n] * sizeof(unsigned), s);
    if (me != hipSuccess) {
      (void)hipGetLastError();
      return (int)me;
    }
    const dim3 cgrid = place_tiles(C, Bc);
    hipLaunchKernelGGL(k_count_multi, cgrid, blk, 0, s, C, flags);
    rc = hip_rc();
    if (rc) return rc;  // (no loss state was touched)
  }
  const dim3 grid = place_tiles(T, B);
  const int cd = common(n, [&](int j) { return T.en[j].g.D; }), cb = common(n, [&](int j) { return T.en[j].g.border; });
  with_storage(descs[0]->dtype, [&](auto tg) {  // (table_fuses: one storage type for the whole table)
    using ST = typename decltype(tg)::type;
    if (cd >= 0 && cb >= 0) {
      return with_width<16, 32>(cd, [&](auto dw) {
        return with_width<PEA_BORDER_CIRCULAR, PEA_BORDER_CROP_ZERO>(cb, [&](auto bd) {
          return launch<k_fwd_bwd_labels_multi<ST, decltype(dw)::value, decltype(bd)::value>>(grid, blk, 0, s, T, flags);
        });
      });
    }
    return launch<k_fwd_bwd_labels_multi<ST, -1, -1>>(grid, blk, 0, s, T, flags);
  });
  rc = hip_rc();
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

}  // extern "C"
