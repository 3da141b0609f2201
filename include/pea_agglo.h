/*
 * pea_agglo.h -- C ABI of the hierarchical agglomeration of a fragment graph on the device (new entry points of libpea_hip.so;
 * include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_rag.h and pea_mws.h: every data pointer is a
 * DEVICE pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL =
 * the default stream), and every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity): the merge loop of waterz,
 *
 *   scripts_ac3ac4/main.py:316-324, scripts_ac3ac4/inference.py:211-220 (-waterz)   waterz.agglomerate(affs, [t], fragments=..,
 *   scripts_cvppp/utils/seg_waterz.py, scripts_bbbc039v1/utils/seg_waterz.py         scoring_function=.., discretize_queue=256)
 *
 * between the region adjacency graph (pea_rag_build) and the projection back to voxels (pea_rag_project).
 *
 * Input, per image b of B independent images: a weighted graph exactly as pea_rag_build writes it.
 *   uv       int32 [B, max_edges, 2]
 *   n_edges  int64, read ON THE DEVICE at n_edges[b * n_edges_stride]: the rows 0 .. min(n_edges, max_edges) - 1 of image b are looked
 *            at (a negative count is 0); `stats + PEA_RAG_N_EDGES` of pea_rag_build with a stride of PEA_RAG_STATS fits as it is
 *   value    f64 [B, max_edges]: a COST (the Python layer builds the graph with PEA_RAG_ONE_MINUS)
 *   weight   int64 [B, max_edges]: the samples behind `value`; read under PEA_AGGLO_MEAN only (may be NULL otherwise)
 * A row is NO EDGE, takes part in nothing and is counted in stats[PEA_AGGLO_NO_EDGE], if u >= v, or an end lies outside
 * [0, max_id], or, under PEA_AGGLO_IGNORE_ZERO, an end is 0.  Asked after that: a row whose value is not finite or exceeds 2^15 in
 * magnitude, or, under PEA_AGGLO_MEAN, whose weight lies outside [0, 2^31], is refused for its value and counted in
 * stats[PEA_AGGLO_BAD_VALUE].  Duplicate (u, v) rows are combined like any two parallel edges.
 *
 * Linkage (d->linkage) and the payload of an edge.  Every payload is combined in integer arithmetic, so the order of arrival does not
 * show anywhere.
 *   PEA_AGGLO_MEAN  payload (sum, count).  count = weight.  sum starts as p = value * (double)weight, ONE f64 rounding, converted once
 *                   to the two-word fixed point with 32 fractional bits of pea_rag.h: whole = floor(p) as a signed integer (|p| <=
 *                   2^46), frac = the integer part of (p - whole) * 2^32 (both steps exact in f64: the conversion floors p to a
 *                   multiple of 2^-32); the low word holds frac, the high word whole.  Combining adds low words, high words and
 *                   counts as integers.  An edge of count 0 has score +inf: it never merges on its own and adds nothing when combined.
 *                   The high words are added in 64 bits: the sum is right while the |whole| parts of the rows that combine into ONE
 *                   edge stay below 2^63 in total -- always for |value| <= 1, a cost (2^30 rows of weight <= 2^31 reach 2^61), and for
 *                   values at the limit 2^15 with weights at the limit 2^31 up to 2^17 rows an edge; beyond that the sum wraps.
 *   PEA_AGGLO_MIN   payload (float)value, combined by min: single linkage on the cost
 *   PEA_AGGLO_MAX   payload (float)value, combined by max: complete linkage on the cost
 * Score, an f32.  MEAN: (float)(f64(sum) / (double)count), f64(sum) = (double)(high + (low >> 32)) + (double)(low & 0xffffffff) / 2^32,
 * the sum rounded to f64 once and divided once in f64, as pea_rag.h makes its mean.  MIN / MAX: the payload.
 * All three linkages are REDUCIBLE: score(A u B, C) >= min(score(A, C), score(B, C)) -- a weighted mean lies between its parts (and the
 * roundings above are monotone), min and max of the parts trivially so.
 * A pair merges only while its score is STRICTLY BELOW d->threshold (f32 comparison): waterz stops at the first score >= threshold.
 *
 * Result: defined by the ROUND RULE.  State: root[i], the smallest fragment id of i's cluster, and the live edges, which sit between
 * distinct roots with combined payloads.  A round reads the state as it was when the round began:
 *   1 best   for every live edge (A, B): key = (ord(score) << 32) | other root, ord the order-preserving uint32 image of an f32 of
 *            pea_ws.h, into best[A] and best[B] by a 64-bit atomic min: a cluster's best neighbour has the lowest score, then the
 *            lowest root id
 *   2 merge  every pair that is each other's best and whose score is below the threshold merges: the larger root points at the
 *            smaller.  A cluster has one best, so such pairs form a matching: no chains, no compression beyond one hop
 *   3 re-key every live edge is keyed on the new roots: an edge inside one cluster dies, parallel edges combine their payloads
 * The live edges are kept in an open-addressing table keyed by the root pair (the probe of csrc/pea_segtable.h, a wave peels its keys
 * so that one wave sends one update per key); a round that merged reads one table and fills the other.  Nothing in the definition
 * depends on a slot's position.  A table has at least 2 * max_edges slots and edges only ever become fewer: it cannot fill.
 *
 * Progress.  While a live edge is below the threshold, the live edge that is smallest under (score, u, v) is a mutual best: another
 * edge at u or at v has a larger score, or the same score and then a larger other end (a smaller one would make that edge the
 * smaller of the two).  So a round that can merge does merge, and the number of rounds is at most the number of merges.
 *
 * Relation to the sequential procedure "pop the live edge of lowest score, merge if below the threshold, rescore" -- waterz without
 * queue discretisation.  Where no two live edges ever share a score the round rule yields its partition exactly.  Let (A, B) be mutual
 * bests.  Until A or B merges, every edge (A, C) keeps a score above score(A, B): it changes only when C merges with some D, and then
 * score(A, C u D) >= min(score(A, C), score(A, D)) > score(A, B) by reducibility; likewise at B.  So the first merge of the sequential
 * procedure that involves A or B is (A, B) itself, at the same score, and it happens iff that score is below the threshold.  Merging
 * (A, B) earlier than its turn changes no score that an earlier pop looks at: pops before it involve neither A nor B, and the
 * edges from A u B to a third cluster carry the same combined payload whenever they are formed (integer sums, min, max: commutative
 * and associative).  The mutual bests of a round are disjoint, so the argument holds for all of them at once, and by induction over the
 * rounds both procedures perform the same set of merges.
 *
 * Ties.  Where scores tie, the round rule IS the definition.  The tie rule is this library's, not waterz's: waterz's
 * discretize_queue=256 puts the scores into 256 bins and leaves the order inside a bin to its queue.
 *
 * Rounds.  pea_agglo_merge enqueues the set-up, exactly d->rounds rounds (0 .. PEA_AGGLO_MAX_ROUNDS) and the outputs.  A word per image
 * lets the launches of a finished image return at once.  If the rounds run out, root is the partition reached so far -- a refinement of
 * the final one -- and stats[.][PEA_AGGLO_MERGEABLE] > 0.  The number of rounds depends on the data: a chain with rising scores takes one
 * round per merge.  With PEA_AGGLO_RESUME the set-up is skipped and the rounds continue from the workspace as the previous call left it
 * (the input rows are not read again).  On a resumed call the threshold may be HIGHER than before: the merges below a threshold are a
 * prefix of those below a higher one, which is how the several thresholds of waterz.agglomerate(affs, thresholds, ..) are served from
 * one run.  The set-up leaves a record (B, max_id, max_edges, linkage, PEA_AGGLO_IGNORE_ZERO, threshold) in the workspace and a resumed
 * call is checked against it: a lower threshold, another linkage or other extents are refused.  The record lies in device memory and
 * the host is never synchronised, so THIS refusal is made on the device: the call changes nothing in the workspace but its verdict word
 * (which the next call's check writes again) and writes -1 into
 * every element of root, labels, counts and stats (what a host-side PEA_E_DESC would say; a workspace that no set-up ever wrote is
 * refused in the same way).  Without PEA_AGGLO_RESUME the workspace is scratch that needs no preparation.
 *
 * Outputs.
 *   root    int32 [B, max_id + 1]: waterz's convention (the reference calls relabel next).  An id in no edge is its own root.
 *   labels  optional int32 [B, max_id + 1] with counts int32 [B] (both or neither): the clusters numbered 1 .. n in ascending root id,
 *           the array that pea_rag_project takes.  An id is PRESENT if node_size[b][id] > 0 (node_size: optional int64 [B, max_id + 1]
 *           from pea_rag_build; without it every id is present) and it is not 0 under PEA_AGGLO_IGNORE_ZERO.  The clusters whose root
 *           is present are numbered; labels[i] is the number of i's cluster if i is present and its cluster is numbered, else 0.
 *   stats   int64 [B, PEA_AGGLO_STATS], the columns below.
 * Everything is an integer that the definition fixes: eager and captured runs, differently aligned pointers and larger workspaces
 * give the same bits.
 *
 * The kernels (csrc/pea_k_agglo.hip): every loop is bounded by a capacity or an extent, no workgroup waits for another one, launch
 * boundaries are the only ordering between workgroups, there are no float atomics.
 *
 * Not served: waterz's HistogramQuantileAffinity scoring (scripts_ac3ac4/main.py:317).  It needs a 256-bin histogram per edge from a
 * sample pass of its own and waterz's bin rule.  A quantile is reducible too, so these rounds will carry it with another payload.
 * Merge history and merge_small_segments are not served either.
 */
#ifndef PEA_AGGLO_H_
#define PEA_AGGLO_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_AGGLO_RESUME 1u      /* skip the set-up: continue from the workspace of the previous call */
#define PEA_AGGLO_IGNORE_ZERO 2u /* id 0 is background: a row with an end 0 is no edge, labels[0] = 0 */
#define PEA_AGGLO_MEAN 0
#define PEA_AGGLO_MIN 1
#define PEA_AGGLO_MAX 2
#define PEA_AGGLO_MAX_ROUNDS 65536     /* rounds of one call */
#define PEA_AGGLO_MAX_EDGES 1073741824 /* 2^30 rows per image */

#define PEA_AGGLO_STATS 8
#define PEA_AGGLO_ROUNDS 0    /* rounds that merged, over all calls since the set-up */
#define PEA_AGGLO_LIVE 1      /* edges live at the end */
#define PEA_AGGLO_MERGEABLE 2 /* live edges still below the threshold: 0 = complete */
#define PEA_AGGLO_MERGES 3    /* merges, over all calls since the set-up */
#define PEA_AGGLO_CLUSTERS 4  /* numbered clusters: what counts holds */
#define PEA_AGGLO_NO_EDGE 5   /* rows that were no edge */
#define PEA_AGGLO_BAD_VALUE 6 /* rows refused for their value (or weight) */
/* 7: reserved, written as 0 */

typedef struct PeaAggloDesc {
  int32_t B;              /* >= 1 */
  int32_t max_id;         /* 0 .. 2^31 - 2: ids are 0 .. max_id */
  int64_t max_edges;      /* 1 .. PEA_AGGLO_MAX_EDGES: rows per image of uv, value, weight */
  int64_t n_edges_stride; /* >= 0: elements between the edge counts of consecutive images */
  int32_t linkage;        /* PEA_AGGLO_MEAN, PEA_AGGLO_MIN, PEA_AGGLO_MAX */
  int32_t rounds;         /* 0 .. PEA_AGGLO_MAX_ROUNDS */
  float threshold;        /* not a NaN */
  uint32_t flags;         /* PEA_AGGLO_RESUME | PEA_AGGLO_IGNORE_ZERO; unknown bits are PEA_E_DESC */
} PeaAggloDesc;

typedef struct PeaAggloBuffers {
  const int32_t *uv;        /* [B, max_edges, 2] */
  const int64_t *n_edges;   /* [b * n_edges_stride] */
  const double *value;      /* [B, max_edges] */
  const int64_t *weight;    /* [B, max_edges]; NULL allowed unless PEA_AGGLO_MEAN */
  const int64_t *node_size; /* [B, max_id + 1] or NULL */
  int32_t *root;            /* [B, max_id + 1] */
  int32_t *labels;          /* [B, max_id + 1] or NULL */
  int32_t *counts;          /* [B]; NULL iff labels is NULL */
  int64_t *stats;           /* [B, PEA_AGGLO_STATS] */
} PeaAggloBuffers;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for, in this order: an unknown flag; B < 1; max_id
 * outside 0 .. 2^31 - 2; max_edges outside 1 .. PEA_AGGLO_MAX_EDGES; n_edges_stride < 0; an unknown linkage; a NaN threshold; rounds
 * outside 0 .. PEA_AGGLO_MAX_ROUNDS. */
int pea_agglo_validate(const PeaAggloDesc *d);

/* Host-only: the bytes of workspace that the call needs (a multiple of 8, monotone in B, max_id and max_edges; it depends on nothing
 * else): a header, 16 words per image, two tables of 32 bytes a slot with the power of two >= max(64, 2 * max_edges) slots each, 16 bytes
 * per id and 4 per 256 ids.  0 for a descriptor that does not validate; SIZE_MAX where the count does not fit. */
size_t pea_agglo_workspace_bytes(const PeaAggloDesc *d);

/* No two buffers overlap.  Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_agglo_validate refuses
 *   PEA_E_NULL         io, io->uv, io->n_edges, io->value, io->root or io->stats is NULL; io->weight is NULL under PEA_AGGLO_MEAN;
 *                      exactly one of io->labels and io->counts is NULL
 *   PEA_E_UNSUPPORTED  more than 2^31 - 1 workgroups in a launch (one per 256 slots, rows or ids of an image)
 *   PEA_E_ALIGN        uv, root, labels or counts not 4-byte aligned; n_edges, value, weight, node_size, stats or the workspace not
 *                      8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_agglo_workspace_bytes(d)
 * A resumed call that does not go with the record in the workspace is refused on the device (above).  Any element-aligned pointer and
 * any extent is served, with the same result. */
int pea_agglo_merge(const PeaAggloDesc *d, const PeaAggloBuffers *io, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_AGGLO_H_ */
