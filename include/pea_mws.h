/*
 * pea_mws.h -- C ABI of the mutex watershed on the device (new entry points of libpea_hip.so; include/pea.h is unchanged and
 * PEA_ABI_VERSION stays 2).  Same conventions as pea_ws.h: every data pointer is a DEVICE pointer owned by the caller, nothing is
 * allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and every refusal returns
 * before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   scripts_cvppp/utils/seg_mutex.py, scripts_bbbc039v1/utils/seg_mutex.py     seg_mutex(affs, offsets, strides, mask) =
 *                                                                              elf's mutex_watershed(1 - affs, offsets, strides, mask=mask)
 *   scripts_ac3ac4/inference.py -mutex                                         mutex_watershed(1 - affs, 12 offsets, strides [1, 10, 10])
 *
 * Data.  B independent images.  x is f32 [B, K, Z, Y, X] dense (Z = 1 for 2D), S = Z * Y * X.  offsets[k] = (dz, dy, dx), K <= 32.  The
 * channels before n_attractive (1 .. K; elf passes ndim) attract, the rest repel.  strides[3] >= 1.  mask is uint8 [B, Z, Y, X] or
 * NULL: non-zero means valid.
 *
 * Edges.  Edge (k, p) joins pixel p (a flat index of its image) and q = p + offsets[k].  It EXISTS iff, asked in this order,
 *   1 q lies inside the image                                                  (else counted in PEA_MWS_MISSING_OUTSIDE)
 *   2 both ends are valid under mask                                           (else PEA_MWS_MISSING_MASK)
 *   3 for a repulsive channel every coordinate of p is a multiple of its stride (elf's strides with randomize_strides = False;
 *     else PEA_MWS_MISSING_STRIDE)
 *   4 its weight is not a NaN                                                  (else PEA_MWS_MISSING_NAN)
 * and a missing edge is counted once, under the first question it fails.  The edge id is k * S + p; K * S < 2^32.
 *
 * Weights, from x in f32 arithmetic with exactly these roundings (fl = one f32 rounding), so the order is the one that the reference's
 * chain produces:
 *   input                 attractive weight      repulsive weight
 *   PEA_MWS_IN_AFFS       fl(1 - fl(1 - a))      fl(1 - a)          x is what seg_mutex(affs, ..) is given: the reference hands 1 - affs to
 *                                                                   elf, which inverts the first ndim channels back
 *   PEA_MWS_IN_ELF        fl(1 - c)              c                  x is elf's own first argument c = 1 - affs
 *   PEA_MWS_IN_WEIGHTS    x                      x
 *
 * Order.  key = (ord(w) << 32) | (0xFFFFFFFF - edge id), ord the order-preserving uint32 image of an f32 of pea_ws.h (-0.0 sorts below
 * +0.0).  A LARGER key comes first.  Keys are distinct, so this is a strict total order: the higher weight first, equal weights by the
 * lower edge id.  The tie rule is this library's, not elf's: affogato sorts the edges with an order that is unspecified among equal
 * weights, so where weights tie (quantised or constant maps) the partition can differ from elf's by the ties only.
 *
 * Result.  The partition that this sequential procedure yields, visiting the existing edges in key order with a union-find:
 *   an edge whose ends are already in one cluster is skipped;
 *   a repulsive edge between clusters A and B makes (A, B) mutually exclusive for good;
 *   an attractive edge between A and B merges them unless (A, B) is exclusive;
 *   exclusions are inherited by the merged cluster.
 *
 * Outputs.
 *   labels  int32 [B, Z, Y, X]: the clusters numbered 1 .. n per image in raster order of their first pixel (the numbering of
 *           pea_cc_label); invalid pixels are 0
 *   counts  int32 [B] = n
 *   stats   int32 [B, PEA_MWS_STATS], the columns PEA_MWS_<NAME> below (a count above 2^31 - 1 is stored as 2^31 - 1)
 *
 * How it runs (csrc/pea_k_mws.hip).  The procedure is not sequential by construction: a ROUND decides a set of edges at once with the
 * same result.  State: a byte per edge (undecided, dead, merged, active exclusion), per pixel the root of its cluster (fully compressed
 * between rounds), per root has_con (the cluster is an end of an active exclusion), and an open-addressing table of the active
 * exclusions keyed by (smaller root, larger root).  Every decision of a round reads the state as it was when the round began:
 *   prune    an undecided edge dies when both ends share a root or its root pair is in the table (it could never merge, and as an
 *            exclusion it would add nothing, whenever it would have been reached)
 *   best     best[root] = the largest key among the surviving undecided edges with an end in the cluster (64-bit atomic max)
 *   decide   an edge that is `best` for a cluster A, B the cluster at its other end: repulsive -> it becomes the active exclusion
 *            (A, B); attractive and A without exclusions -> merge; attractive and best for B too -> merge (the prune has shown that
 *            (A, B) is not exclusive); anything else waits
 *   hook     a cluster that promoted a merge points at the other root; where both promoted the same edge the smaller root stays
 *   compress by pointer jumping; has_con is carried to the new roots; the table is rebuilt on the new roots from the active edges,
 *            and an active edge whose pair is already there dies
 * Why it is exact: deciding an edge e now instead of at its turn changes nothing provided no undecided edge of larger key touches the
 * cluster A that promotes it -- every edge in between is not incident to A, so its same-cluster test does not involve A; a repulsive
 * e = (A, .) cannot be asked for by an edge in between (that takes an attractive edge at A); an attractive e of a cluster A without
 * exclusions brings none into the cluster it joins, so every lookup in between answers as before; a mutual best has nothing in between
 * on either side.  Inside a round take the promoted edges by descending key: one of higher key touches its own cluster and its target,
 * and the target cannot be A (the edge would be incident to A and exceed best[A]).  Promoted merges have strictly increasing keys along
 * a chain, so the hooks form a forest plus mutual pairs, as in pea_ws_flood.  Progress: while an undecided edge survives the prune, the
 * largest one is a mutual best, so such a round decides at least one edge; the number of rounds depends on the data and is not
 * logarithmic (tens to a few hundred on the drivers' maps).
 * Termination: table probes are bounded by the capacity (sized from the repulsive edge slots that the strides admit: it cannot fill),
 * a find walks a path that only ever shortens, no workgroup waits for another one.
 *
 * Rounds.  pea_mws_segment enqueues the set-up, exactly d->rounds rounds and the labelling.  A word per image lets the launches of a
 * round with nothing left return at once.  If the rounds run out, labels is the partition reached so far -- every cluster is a subset of
 * a final one -- and stats[.][PEA_MWS_UNDECIDED] > 0.  With PEA_MWS_RESUME the set-up is skipped and the rounds continue from the
 * workspace as the previous call on the same descriptor, x and mask left it, so a caller adds rounds until the stats say complete.
 * Without PEA_MWS_RESUME the workspace is scratch: it needs no preparation.
 * A NaN in x is a missing edge; +-inf weights are ordinary weights.  labels, counts and stats are integers that the definition fixes:
 * two runs give the same bits.
 */
#ifndef PEA_MWS_H_
#define PEA_MWS_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_MWS_MAX_K 32
#define PEA_MWS_MAX_ROUNDS 65536 /* rounds of one call */
#define PEA_MWS_RESUME 1u        /* skip the set-up: continue from the workspace of the previous call */

#define PEA_MWS_IN_AFFS 0    /* x = affs, what seg_mutex is given */
#define PEA_MWS_IN_ELF 1     /* x = 1 - affs, elf's first argument */
#define PEA_MWS_IN_WEIGHTS 2 /* x = the weights themselves */

#define PEA_MWS_STATS 8
#define PEA_MWS_ROUNDS 0          /* rounds in which an edge was decided (merged or made an exclusion), over all calls since the set-up */
#define PEA_MWS_UNDECIDED 1       /* edges still undecided: 0 = complete */
#define PEA_MWS_MERGES 2          /* edges decided as merges */
#define PEA_MWS_EXCLUSIONS 3      /* active exclusions (distinct cluster pairs) at the end */
#define PEA_MWS_MISSING_STRIDE 4  /* edges missing by cause, each under the first question it fails */
#define PEA_MWS_MISSING_MASK 5
#define PEA_MWS_MISSING_NAN 6
#define PEA_MWS_MISSING_OUTSIDE 7

typedef struct PeaMwsDesc {
  int32_t B, Z, Y, X, K;                 /* x is [B, K, Z, Y, X] dense, each >= 1, K <= PEA_MWS_MAX_K */
  int32_t n_attractive;                  /* 1 .. K */
  int32_t offsets[PEA_MWS_MAX_K][3];     /* (dz, dy, dx) of channel k */
  int32_t strides[3];                    /* >= 1 */
  int32_t input;                         /* PEA_MWS_IN_* */
  int32_t rounds;                        /* 0 .. PEA_MWS_MAX_ROUNDS */
  uint32_t flags;                        /* PEA_MWS_RESUME; unknown bits are PEA_E_DESC */
} PeaMwsDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for, in this order: an unknown flag; B, Z, Y, X or
 * K < 1; K > PEA_MWS_MAX_K; n_attractive outside 1 .. K; a stride < 1; an unknown input; rounds outside 0 .. PEA_MWS_MAX_ROUNDS. */
int pea_mws_validate(const PeaMwsDesc *d);

/* Host-only: the bytes of workspace that the call needs (a multiple of 8, monotone in every extent); 0 for a descriptor that does not
 * validate; SIZE_MAX where the count does not fit. */
size_t pea_mws_workspace_bytes(const PeaMwsDesc *d);

/* x f32 [B, K, Z, Y, X]; mask uint8 [B, Z, Y, X] or NULL; labels int32 [B, Z, Y, X]; counts int32 [B]; stats int32 [B, PEA_MWS_STATS].
 * No two of them overlap.  Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_mws_validate refuses
 *   PEA_E_NULL         x, labels, counts or stats is NULL
 *   PEA_E_UNSUPPORTED  K * S >= 2^32 or S >= 2^31 (edge ids are uint32, roots int32); more than 2^31 - 1 workgroups (one per 256
 *                      pixels of a channel)
 *   PEA_E_ALIGN        x, labels, counts or stats is not 4-byte aligned, or the workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_mws_workspace_bytes(d)
 * Any element-aligned pointer and any extent is served, with the same result. */
int pea_mws_segment(const PeaMwsDesc *d, const float *x, const uint8_t *mask, int32_t *labels, int32_t *counts, int32_t *stats,
                    void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_MWS_H_ */
