/*
 * pea_ws.h -- C ABI of the watershed fragments on the device: distance transform, seeds, flood (new entry points of libpea_hip.so;
 * include/pea.h is unchanged and PEA_ABI_VERSION stays 2).  Same conventions as pea_cc.h and pea_rag.h: every data pointer is a DEVICE
 * pointer owned by the caller, nothing is allocated, the host is never synchronised, `void *stream` is a hipStream_t (NULL = the
 * default stream), and every refusal returns before anything is launched.
 *
 * What the calls replace in the reference (weih527/Pixel-Embedded-Affinity):
 *
 *   utils/lmc.py mc_baseline / multicut_multi          elf.segmentation.watershed.distance_transform_watershed(boundary_input[z],
 *   scripts_ac3ac4/utils/fragment.py elf_watershed      threshold=.25, sigma_seeds=2.) per z-plane, ids stacked with `wsz += offset`
 *   scripts_ac3ac4/utils/fragment.py watershed          mahotas.cwatershed from grid / minima / distance-maxima seeds
 *
 * All data are a batch of N independent planes [N, Y, X]; a volume is N = B * Z, as the reference works per plane.  Planes never
 * touch.  One descriptor serves both calls; each call reads its own fields and every field must be valid for both.
 *
 * pea_ws_seeds: boundary map -> distance transform, height map, seeds
 *   dt2[p]   the exact squared Euclidean distance, in pixels, from p to the nearest pixel of its plane with boundary > threshold: 0 on
 *            those pixels, Y * Y + X * X everywhere in a plane that has none.  An integer: exact.
 *   dt       sqrtf((float)dt2)
 *   G(s)     a separable Gaussian in f32 of radius r = (int)(3 s + 0.5) (vigra's window ratio), weights exp(-i * i / (2 s * s))
 *            normalised to sum 1, computed on the host in f64 and rounded once; the border is mirrored without repeating the edge
 *            pixel (scipy mode='mirror'); s == 0 skips the filter.  Along x first, then along y.
 *   dts      G(sigma_seeds) * dt
 *   hmap     G(sigma_weights) * (alpha * boundary + (1 - alpha) * (1 - (dt - dmin) / (dmax - dmin))), dmin / dmax the plane's extrema of
 *            dt taken as sqrtf of the integer extrema of dt2; the quotient is 0 where they are equal
 *   seeds    A plateau is a maximal set of pixels of equal dts value (-0.0 counts as +0.0), connected under maxima_connectivity (1: the
 *            4-, 2: the 8-neighbourhood, vigra's localMaxima).  A plateau is a maximum iff every neighbour of every one of its pixels
 *            that lies outside it is strictly lower; the image border is allowed (allowAtBorder = True, allowPlateaus = True).  The
 *            pixels of all maxima form a mask, and `seeds` numbers the components of that mask under seed_connectivity 1 .. n in raster
 *            order of their first pixel -- the numbering of pea_cc_label, whose kernels do both labellings.  counts[n] = n.
 *   With PEA_WS_FIELD `boundary` is not a boundary map but the field whose maxima are wanted: threshold, the distance transform and
 *   the height map are skipped, dts = G(sigma_seeds) * boundary, and dt2 and hmap must be NULL.  (fragment.py's 'minima' seeds are the
 *   maxima of -boundary, its 'maxima_distance' seeds those of dt, both with sigma_seeds == 0.)
 *   A NaN in `boundary` is refused by nobody: the results are unspecified, but every loop still ends (a NaN is never above the
 *   threshold; the plateau labelling works on bit patterns).
 *
 * pea_ws_flood: height map + seeds -> fragments
 *   Every 4-neighbour pair (p, q = p + 1) or (p, q = p + X) of a plane is an edge with the key (max(ord(h[p]), ord(h[q])), 2 p + dir):
 *   ord is the order-preserving uint32 image of an f32 (-0.0 sorts below +0.0; a NaN sorts by its bits), dir is 0 for the x edge and 1
 *   for the y edge, p is the flat index y * X + x.  Keys are distinct, so they are a strict total order.  The result is the minimum
 *   spanning forest relative to the seeds under that order: Kruskal over the edges by key, where an edge is skipped iff both ends are
 *   already in one tree or both trees hold a seeded pixel; a pixel takes the seed id of its tree.  This is the watershed cut: every
 *   pixel is joined to its seed by a path whose highest point is as low as that of any path to any seed.  The definition fixes every
 *   tie, so the label image is unique and does not depend on the order in which workgroups arrive.  The tie rule is this library's,
 *   not vigra's or mahotas' (whose floods break ties by queue order): on plateaus a fragment boundary can differ from theirs.
 *   seeds    int32, 0 = none.  A seed id lies in 1 .. Y * X (the ids of pea_ws_seeds do); any other value is read as 0.  Pixels of one
 *            id need not touch.
 *   min_size elf's size_filter followed by a second flood: with min_size > 1 the seeds whose fragment has fewer than min_size pixels
 *            are removed and the flood runs again from the remaining seeds.  A plane in which none would remain keeps its first flood.
 *   labels   the kept fragments renumbered 1 .. n per plane in ascending order of seed id; with PEA_WS_STACK_IDS plane n is offset by
 *            the kept counts of the planes before it (the reference's `wsz += offset`).  0 where no seed is reached: only in a plane
 *            without seeds.
 *   counts   int32 [N, 2] = { fragments found by the first flood, fragments kept }
 *   stats    int32 [N, 2] = { rounds of the last flood in which a tree was hooked, pixels left 0 }
 *
 * The workspace of either call is scratch, not state: it needs no preparation, every word that is read was written by the same call,
 * and its contents afterwards are unspecified.
 *
 * Termination (csrc/pea_k_ws.hip).  The flood is Boruvka's algorithm: every pixel starts as its own tree, a seeded pixel is a labelled
 * tree, and labelled trees never pick an edge.  A round is three launches (pick the smallest outgoing edge per unlabelled tree with a
 * 64-bit atomicMin; hook every such root onto the root at the other end, the smaller root staying where two picked the same edge;
 * compress by path halving).  Picks of distinct keys form a forest, so every find ends; a round at least halves the number of
 * unlabelled trees that have an outgoing edge, so the host enqueues exactly ceil(log2(Y * X)) + 1 rounds and a flag per (plane, round)
 * lets the launches of finished rounds return at once.  No workgroup waits for another one.  The column pass of the distance transform
 * walks outwards from a pixel and stops once dy * dy reaches the best so far: bounded by Y.
 */
#ifndef PEA_WS_H_
#define PEA_WS_H_

#include "pea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_WS_STACK_IDS 1u /* pea_ws_flood: plane n's ids are offset by the kept counts of the planes before it */
#define PEA_WS_FIELD 2u     /* pea_ws_seeds: `boundary` is the field whose plateau maxima are the seeds */
#define PEA_WS_MAX_RADIUS 32 /* the largest Gaussian radius (int)(3 sigma + 0.5) that is served */

typedef struct PeaWsDesc {
  int32_t N, Y, X;              /* planes [N, Y, X] dense, each >= 1 */
  float threshold;              /* seeds: boundary > threshold is a boundary pixel (finite) */
  float sigma_seeds;            /* seeds: >= 0, finite; 0 = no filter */
  float sigma_weights;          /* seeds: >= 0, finite; 0 = no filter */
  float alpha;                  /* seeds: in [0, 1] */
  int32_t maxima_connectivity;  /* seeds: 1 | 2 (2: vigra's 8-neighbourhood localMaxima) */
  int32_t seed_connectivity;    /* seeds: 1 | 2 */
  int32_t min_size;             /* flood: >= 0 (0 and 1 filter nothing) */
  uint32_t flags;               /* PEA_WS_*; unknown bits are PEA_E_DESC */
} PeaWsDesc;

/* Host-only check of a descriptor: PEA_OK, or PEA_E_NULL (d == NULL), or PEA_E_DESC for: N, Y or X < 1; a threshold, sigma or alpha
 * that is not finite; a negative sigma; alpha outside [0, 1]; a connectivity that is not 1 or 2; a negative min_size; an unknown flag. */
int pea_ws_validate(const PeaWsDesc *d);

/* Host-only: the bytes of workspace that the call needs (a multiple of 8); 0 for a descriptor that does not validate; SIZE_MAX where
 * the count does not fit. */
size_t pea_ws_seeds_workspace_bytes(const PeaWsDesc *d);
size_t pea_ws_flood_workspace_bytes(const PeaWsDesc *d);

/* boundary f32 [N, Y, X]; dt2 int32, dts f32, hmap f32 of that shape, each or NULL; seeds int32 of that shape; counts int32 [N].
 * Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_ws_validate refuses
 *   PEA_E_NULL         boundary, seeds or counts is NULL; with PEA_WS_FIELD: dt2 or hmap is given
 *   PEA_E_ALIGN        a data pointer is not 4-byte aligned, or the workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_ws_seeds_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  Y * X >= 2^30; Y * Y + X * X >= 2^31 (dt2 is an int32); a Gaussian radius that is used is > PEA_WS_MAX_RADIUS
 *                      or >= min(Y, X), for any finite sigma however large; more than 2^31 - 1 workgroups (one per 256 pixels of a plane; one per 32 x 32 tile)
 * Any element-aligned pointer and any extent is served, with the same result. */
int pea_ws_seeds(const PeaWsDesc *d, const float *boundary, int32_t *dt2, float *dts, float *hmap, int32_t *seeds, int32_t *counts,
                 void *workspace, size_t workspace_bytes, void *stream);

/* hmap f32 [N, Y, X]; seeds int32 [N, Y, X]; labels int32 [N, Y, X]; counts int32 [N, 2]; stats int32 [N, 2].  seeds may be labels
 * (in place); no other pair overlaps.  Returns, before anything is launched and in this order:
 *   PEA_E_NULL         d is NULL
 *   PEA_E_DESC         what pea_ws_validate refuses
 *   PEA_E_NULL         hmap, seeds, labels, counts or stats is NULL
 *   PEA_E_ALIGN        a data pointer is not 4-byte aligned, or the workspace not 8-byte aligned
 *   PEA_E_WORKSPACE    workspace is NULL or shorter than pea_ws_flood_workspace_bytes(d)
 *   PEA_E_UNSUPPORTED  Y * X >= 2^30 (the edge index 2 p + 1 must fit 31 bits); more than 2^31 - 1 workgroups (one per 256 pixels);
 *                      with PEA_WS_STACK_IDS: N * Y * X >= 2^31 (a stacked id is an int32 sum of kept counts, at most one per pixel) */
int pea_ws_flood(const PeaWsDesc *d, const float *hmap, const int32_t *seeds, int32_t *labels, int32_t *counts, int32_t *stats,
                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_WS_H_ */
