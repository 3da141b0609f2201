/*
 * pea_merge.h -- C ABI of the small-segment merges and the renumbering on the device (new entry points of libpea_hip.so; include/pea.h
 * is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_cc.h and pea_agglo.h: every data pointer is a DEVICE pointer owned
 * by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the default stream), and
 * every refusal returns before anything is launched.
 *
 * What the call replaces in the reference (weih527/Pixel-Embedded-Affinity), between seg_mutex and the scores of the validation loops
 * (scripts_cvppp/main.py:406-416, scripts_bbbc039v1/main.py:403-431) and in both inference.py files:
 *
 *   scripts_cvppp/utils/postprocessing.py:8-40        merge_small_object, merge_func   passes (5, 5), (20, 11), (50, 11), (300, 21)
 *   scripts_bbbc039v1/utils/postprocessing.py:9-41    merge_small_object, merge_func   passes (5, 5), (25, 11), (50, 11), (100, 21)
 *   scripts_cvppp/utils/seg_waterz.py:5-19            relabel (the same in scripts_bbbc039v1)
 *
 * The definition.  One pass (threshold, window) over an image seg [Y, X], int32, ids in [0, max_id]:
 *
 *   1. size0[i] is the number of pixels of id i at the START of the pass (the reference takes np.unique(.., return_counts=True) once,
 *      before its loop).  The sizes are stale during the pass: an id that has received merges is still judged by size0.
 *   2. For i = 0, 1, .., max_id in ascending order, the ids with 0 < size0[i] <= threshold are candidates.  Id 0 is a candidate like any
 *      other: the reference does not exempt the background.  (Pixels only ever move when their own id is served, and an id is served
 *      once per pass, so a candidate still has pixels at its turn.)
 *   3. The candidate's window: r = floor(sum of rows / n), c = floor(sum of columns / n) over the pixels that carry i NOW, including the
 *      pixels merged into i earlier in this pass; r0 = r - window / 2, c0 = c - window / 2 (integer halves).  If r0 < 0 or c0 < 0
 *      NOTHING HAPPENS: Python's negative slice start gives an empty crop when window <= min(Y, X), which is required here.  The crop is
 *      rows r0 .. min(r0 + window, Y) - 1 and the columns likewise, read through the merges made so far.
 *   4. Count the distinct current ids in the crop.  With 2 or fewer nothing happens.  Otherwise they are ranked by count descending,
 *      THEN ID ASCENDING -- np.argsort(-counts, kind="stable") on np.unique's ascending ids.  If rank 0 is id 0, the target is rank 1, or
 *      rank 2 where rank 1 is i itself; otherwise the target is rank 0.
 *   5. If the target is not i, every pixel of i takes the target's id.
 *
 * The tie rule is this library's.  The reference ranks with np.argsort(-counts), whose default sort is not stable and, from numpy 1.25
 * on, differs between CPUs (the AVX-512 / AVX2 argsort); the order of equal counts is the ONLY freedom it has, and here it is fixed.  An
 * image on which no pass meets a tie that matters gives the reference's result exactly (tests/golden/gmerge_*.npz hold such images, made
 * with the reference's own functions).
 *
 * PEA_MERGE_RELABEL renumbers afterwards: the ids above 0 that still have pixels become 1 .. n in ascending id order, 0 stays 0 -- the
 * reference's relabel.  counts[b] = n in either case.  The reference casts to uint16 before merge_func, so its ids wrap at 65536; the
 * ids here are int32 and do not wrap.  merge_func2 of scripts_cvppp/inference.py (window 101, called nowhere) is not served: a window is
 * at most PEA_MERGE_MAX_WINDOW = 45, which keeps the crop's id table in LDS (2025 pixels, 4096 slots of 8 bytes, 32 KiB).
 *
 * How it runs (csrc/pea_k_merge.hip).  A merge is seg[seg == i] = target, so the image is never rewritten: an alias per id carries every
 * merge, and per-id pixel count, row sum and column sum are integers that add under a merge, so the centroid is exact.  One streaming
 * pass takes the moments; ONE WORKGROUP PER IMAGE walks the candidates in order (the images of a batch side by side), each candidate a
 * crop of at most window^2 pixels counted into an LDS table; a streaming pass writes out[p] = map[root(seg[p])].  Every number is an
 * integer that the definition fixes: eager and captured runs, any element-aligned pointers and a larger workspace give the same bits.
 * Every loop is bounded by an extent or max_id + 1, and no workgroup waits for another one.
 *
 * A pixel whose id lies outside [0, max_id] is written through unchanged, is never a candidate, counts for nothing in a crop or a
 * centroid, and is counted in stats: the result is the definition's only where that count is 0.
 *
 * The workspace is scratch, not state: it needs no preparation, every word that is read was written by the same call, and the same
 * block serves any later call that it is large enough for.
 */
#ifndef PEA_MERGE_H_
#define PEA_MERGE_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_MERGE_RELABEL 1u    /* renumber the ids above 0 that are left as 1 .. n in ascending id order */
#define PEA_MERGE_MAX_PASSES 8
#define PEA_MERGE_MAX_WINDOW 45

#define PEA_MERGE_STATS 8
#define PEA_MERGE_CANDIDATES 0   /* candidates looked at, over all passes */
#define PEA_MERGE_MERGES 1       /* candidates that took another id */
#define PEA_MERGE_NEGATIVE 2     /* candidates skipped for a negative window start */
#define PEA_MERGE_FEW 3          /* candidates whose crop held 2 or fewer distinct ids */
#define PEA_MERGE_OUT_OF_RANGE 4 /* pixels with an id outside [0, max_id] */
#define PEA_MERGE_CHAIN 5        /* the longest alias chain met while a crop was read (hops from a pixel's id to its current id) */
/* 6, 7: reserved, written as 0 */

typedef struct PeaMergeDesc {
  int32_t B, Y, X;                         /* seg [B, Y, X] dense, each >= 1 */
  int32_t max_id;                          /* 0 .. 2^31 - 2: ids are 0 .. max_id */
  int32_t n_passes;                        /* 1 .. PEA_MERGE_MAX_PASSES */
  int32_t threshold[PEA_MERGE_MAX_PASSES]; /* >= 0; entries from n_passes on are ignored */
  int32_t window[PEA_MERGE_MAX_PASSES];    /* 1 .. PEA_MERGE_MAX_WINDOW and <= min(Y, X); entries from n_passes on are ignored */
  uint32_t flags;                          /* PEA_MERGE_RELABEL; unknown bits are PEA_E_DESC */
} PeaMergeDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for, in this order: an unknown flag; B, Y or X < 1;
 * max_id outside 0 .. 2^31 - 2; n_passes outside 1 .. 8; a negative threshold or a window outside 1 .. 45 among the first n_passes; or,
 * after all of these, PEA_E_UNSUPPORTED for a window above min(Y, X). */
int pea_merge_validate(const PeaMergeDesc *d);

/* Host-only: the bytes of workspace that pea_merge_small needs (a multiple of 8, monotone in B and max_id; it depends on nothing else):
 * 64 bytes per image, 36 bytes per id (three int64 moments, alias, root, rank), 8 per 64 ids (the candidates of a pass, a bit each)
 * and 4 per 256 ids.  0 for a descriptor that does not validate; SIZE_MAX where the count does not fit. */
size_t pea_merge_workspace_bytes(const PeaMergeDesc *d);

/* seg int32 [B, Y * X]; out int32, the same shape: exactly seg (in place) or disjoint from it; counts int32 [B]: the ids above 0 that
 * are left; stats int64 [B, PEA_MERGE_STATS].  Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC / PEA_E_UNSUPPORTED   what pea_merge_validate refuses
 *   PEA_E_NULL         seg, out, counts or stats is NULL
 *   PEA_E_ALIGN        seg, out or counts not 4-byte aligned; stats or the workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_merge_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  Y * X >= 2^31; more than 2^31 - 1 workgroups in a launch (one per 1024 pixels or 256 ids of an image); out
 *                      overlaps seg without being seg
 * Any element-aligned pointer and any extent is served, with the same result. */
int pea_merge_small(const PeaMergeDesc *d, const int32_t *seg, int32_t *out, int32_t *counts, int64_t *stats, void *workspace,
                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_MERGE_H_ */
