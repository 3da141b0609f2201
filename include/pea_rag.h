/*
 * pea_rag.h -- C ABI of the region adjacency graph of a fragment image or volume, with per-edge statistics of an affinity map and of a
 * boundary map (new entry points of libpea_hip.so; include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as
 * pea_cc.h and pea_segscore.h: every data pointer is a DEVICE pointer owned by the caller, nothing is allocated, the host is never
 * synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity), scripts_ac3ac4/utils/lmc.py (mc_baseline, multicut_multi;
 * the 2D scripts import the same file), between the fragments and the Kernighan-Lin solver and after it:
 *
 *   rag        = feats.compute_rag(fragments)                                   the sorted unique pairs of touching fragments
 *   costs      = feats.compute_affinity_features(rag, 1 - affs, offsets)[:, 0]   the mean of (1 - a) over each pair's boundary
 *   edge_sizes = feats.compute_boundary_mean_and_length(rag, boundary)[:, 1]     the boundary length of each pair
 *   seg        = feats.project_node_labels_to_pixels(rag, node_labels)           seg[p] = node_labels[fragments[p]]
 *
 * Semantics, per image b of a batch; ndim is 2 or 3 and a 2D image is Z = 1; S = Z * Y * X; nothing wraps and the images of a batch
 * never touch.
 *
 *   fragments  int32 [B, S], ids in [0, max_id].  Any other value is no id: its voxel takes part in nothing and is counted
 *              (PEA_RAG_N_NO_ID).  With PEA_RAG_IGNORE_ZERO id 0 is background: it takes part in no edge and is not counted.
 *   edges      {u, v} with u < v is an edge iff some voxel of u and some voxel of v are direct neighbours, one step along one axis.
 *              size(u, v) is the number of such voxel pairs.
 *   boundary   optional f32 [B, S]: every one of those voxel pairs (p, q) adds boundary[p] + boundary[q] to bsum(u, v); the
 *              boundary mean is bsum / (2 size).  A term that is not finite or has |x| > 2^15 adds nothing and is counted with the
 *              skipped samples.
 *   affs       optional f32 [B, K, S] with K <= 32 offsets of any reach.  For every k and every p with q = p + offsets[k] inside
 *              the image, u = fragments[p], v = fragments[q]: where both are ids that take part, u != v and {u, v} is an edge,
 *              the sample x = affs[b, k, p] goes into count, sum, min, max of that edge.  With PEA_RAG_ONE_MINUS the sample is
 *              x = 1.0f - affs[b, k, p], rounded once in f32.  A pair of fragments that do not touch is skipped and counted
 *              (PEA_RAG_N_NOT_TOUCHING: what the long-range channels need); then a sample that is not finite or has |x| > 2^15 is
 *              skipped and counted (PEA_RAG_N_SKIPPED).
 *   sums       fixed point with 32 fractional bits, floored, in two words: the low 32 bits of each term are added into one u64, the
 *              signed whole part into another, so 2^31 terms of either sign cannot overflow and the sum does not depend on the
 *              order of arrival.  mean = sum / count (the sum rounded to f64 once, one f64 division; 0 where count is 0) and the
 *              boundary mean lie within 2^-32 of the exact mean of the f32 terms plus 2^-52 |value|.  min and max are the exact f32
 *              values (0 where count is 0); size and count are exact integers.
 *   order      the edges of an image come out sorted by (u, v), and the edge id is the rank, as np.unique(pairs, axis=0) orders
 *              them: the uv list that multicut(n_nodes, uvs, costs) of the reference's utils/mc_baselines.py takes.
 *
 * Outputs.  uv int32 [B, max_edges, 2]; size, count int64 [B, max_edges]; mean, bmean f64 [B, max_edges]; min, max f32
 * [B, max_edges]; node_size int64 [B, max_id + 1], the voxels per id (id 0 also under PEA_RAG_IGNORE_ZERO); stats int64
 * [B, PEA_RAG_STATS].  Rows past the edge count are zero.  uv and stats are required, every other output may be NULL.  No output
 * overlaps an input or another output.  Two runs, an eager and a captured run, calls on differently aligned pointers and calls with
 * different capacities that do not overflow give the same bits everywhere.
 *
 * The launches (csrc/pea_k_rag.hip): clear, the edge pass over the voxels, the sample pass over (k, voxel), degree by u over the
 * table's slots, one scan per image, the scatter into rows, the rank within a row and the write, the stats: eight, none per edge.
 * Every loop is bounded by `capacity`, a row length or an image extent; no workgroup waits for another one, launch boundaries are
 * the only ordering between workgroups; a full table drops voxel pairs, counts them and the call ends.
 */
#ifndef PEA_RAG_H_
#define PEA_RAG_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_RAG_ONE_MINUS 1u   /* the affinity sample is 1.0f - affs */
#define PEA_RAG_IGNORE_ZERO 2u /* id 0 is background and takes part in nothing */
#define PEA_RAG_MAX_K 32
#define PEA_RAG_MIN_CAPACITY 64
#define PEA_RAG_STATS 8
/* the columns of stats [B][PEA_RAG_STATS] */
#define PEA_RAG_N_EDGES 0        /* edges found (that found a slot) */
#define PEA_RAG_N_EDGES_DROPPED 1 /* edges beyond max_edges, not written */
#define PEA_RAG_N_PAIRS_DROPPED 2 /* voxel pairs dropped by a full table */
#define PEA_RAG_N_NO_ID 3        /* voxels with no id */
#define PEA_RAG_N_NOT_TOUCHING 4 /* samples on pairs of fragments that do not touch */
#define PEA_RAG_N_SKIPPED 5      /* samples and boundary terms skipped as non-finite or too large */
/* 6, 7: reserved, written as 0 (-1 in every column: the workspace was never prepared) */

typedef struct PeaRagDesc {
  int32_t ndim;                       /* 2 or 3 */
  int32_t B, dims[3];                 /* fragments [B, Z, Y, X] dense; ndim == 2: dims[0] == 1 */
  int32_t K;                          /* offsets of the affinity map, 0 .. 32 */
  int32_t offsets[PEA_RAG_MAX_K][3];  /* (dz, dy, dx) of channel k: q = p + offsets[k]; ndim == 2: dz == 0 */
  int32_t max_id;                     /* >= 0: ids are 0 .. max_id */
  int64_t capacity;                   /* table slots per image: a power of two, 64 .. 2^31 */
  int64_t max_edges;                  /* >= 1: rows per image of the edge outputs */
  uint32_t flags;                     /* PEA_RAG_ONE_MINUS | PEA_RAG_IGNORE_ZERO; unknown bits are PEA_E_DESC */
} PeaRagDesc;

typedef struct PeaRagBuffers {
  const int32_t *fragments; /* [B, S] */
  const float *affs;        /* [B, K, S] or NULL */
  const float *boundary;    /* [B, S] or NULL */
  int32_t *uv;              /* [B, max_edges, 2] */
  int64_t *size;            /* [B, max_edges] or NULL */
  int64_t *count;           /* [B, max_edges] or NULL */
  double *mean;             /* [B, max_edges] or NULL */
  double *bmean;            /* [B, max_edges] or NULL */
  float *min;               /* [B, max_edges] or NULL */
  float *max;               /* [B, max_edges] or NULL */
  int64_t *node_size;       /* [B, max_id + 1] or NULL */
  int64_t *stats;           /* [B, PEA_RAG_STATS] */
} PeaRagBuffers;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for, in this order: any unknown flag bit; K
 * outside 0 .. 32; ndim not 2 or 3; B or a dim < 1; ndim == 2 with dims[0] != 1 or an offset with dz != 0; max_id < 0; a capacity
 * that is no power of two, below PEA_RAG_MIN_CAPACITY or above 2^31; max_edges < 1; or PEA_E_UNSUPPORTED for Z * Y * X >= 2^31
 * (checked last). */
int pea_rag_validate(const PeaRagDesc *d);

/* Host-only: the bytes of workspace of pea_rag_build (a multiple of 8): a header, 32 words per image, 64 bytes and two int32 per
 * (image, slot), three int32 per (image, id).  0 for a descriptor that does not validate; SIZE_MAX where the count does not fit. */
size_t pea_rag_workspace_bytes(const PeaRagDesc *d);

/* Prepare `bytes` bytes at `workspace` (8-byte aligned, bytes >= 64 and a multiple of 8) once per allocation: all zero but for a
 * magic word.  Every pea_rag_build leaves the tables like that for the next call on the same stream, whatever its descriptor; on a
 * block that was never prepared every column of stats is -1 and the edge outputs are zero.  PEA_E_NULL / PEA_E_ALIGN /
 * PEA_E_WORKSPACE (bytes < 64 or not a multiple of 8). */
int pea_rag_workspace_init(void *workspace, size_t bytes, void *stream);

/* Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_rag_validate refuses
 *   PEA_E_NULL         io, io->fragments, io->uv or io->stats is NULL
 *   PEA_E_ALIGN        fragments, affs, boundary, uv, min or max not 4-byte aligned; size, count, mean, bmean, node_size, stats or
 *                      the workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_rag_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups in a launch (one per 1024 voxels of an image and channel; one per 256 slots,
 *                      output rows or ids of an image)
 * Never synchronises, allocates nothing.  Any element-aligned pointer and any extent is served with the same bits. */
int pea_rag_build(const PeaRagDesc *d, const PeaRagBuffers *io, void *workspace, size_t workspace_bytes, void *stream);

/* seg[p] = node_labels[fragments[p]] for n voxels, int32 in and out, one streaming launch (project_node_labels_to_pixels without
 * torch's int64 index copy).  A voxel whose fragment id lies outside 0 .. n_labels - 1 gives 0 and ADDS one to n_bad[0] (int64,
 * DEVICE, may be NULL; the caller zeroes it).  seg may be fragments itself.
 * Returns in this order: PEA_E_DESC (n < 1 or n_labels < 1); PEA_E_NULL (fragments, node_labels, seg); PEA_E_ALIGN (an int32 pointer
 * not 4-byte, n_bad not 8-byte aligned); PEA_E_UNSUPPORTED (more than 2^31 - 1 workgroups, one per 4096 voxels). */
int pea_rag_project(int64_t n, const int32_t *fragments, const int32_t *node_labels, int64_t n_labels, int32_t *seg, int64_t *n_bad,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_RAG_H_ */
