"""The watershed fragments on the device (include/pea_ws.h: pea_ws_seeds, pea_ws_flood) -- what the reference does per z-plane on the
host before its multicut,

  utils/lmc.py mc_baseline / multicut_multi, scripts_ac3ac4/utils/fragment.py elf_watershed
      elf.segmentation.watershed.distance_transform_watershed(boundary_input[z], threshold=.25, sigma_seeds=2.), `wsz += offset`
  scripts_ac3ac4/utils/fragment.py watershed          mahotas.cwatershed from grid / minima / distance-maxima seeds

as launches of csrc/pea_k_ws.hip: an exact squared Euclidean distance transform, two separable Gaussians, plateau maxima through the
union-find of pea_cc_label, and a flood that is the minimum spanning forest relative to the seeds (Boruvka rounds).  No host
synchronisation, so the calls can be captured with pea.graphed.  The flood's tie rule is this library's, not vigra's: on plateaus a
fragment boundary can differ from elf's by the tie only.  Device tensors only; distance_transform_watershed alone also
takes numpy arrays, through the device.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _no_init, _on_device, _ptr, _require_gpu, _stream, stream_workspace

_INT32_MAX = 2 ** 31 - 1


class WatershedSeeds(object):
    """seeds   int32 [N, Y, X]: the plateau maxima of dts, numbered 1 .. n per plane in raster order of their first pixel, 0 elsewhere
    hmap    float32 [N, Y, X]: G(sigma_weights) * (alpha * boundary + (1 - alpha) * (1 - normalised dt)), or None
    dt2     int32 [N, Y, X]: the exact squared Euclidean distance to the nearest pixel with boundary > threshold, or None
    dts     float32 [N, Y, X]: G(sigma_seeds) * sqrt(dt2) (of plateau_maxima: G(sigma) * field)
    counts  int32 [N]: seeds per plane
    All are device tensors of the input's shape ([Y, X] in: no N); nothing is copied to the host."""

    def __init__(self, seeds, hmap, dt2, dts, counts):
        self.seeds, self.hmap, self.dt2, self.dts, self.counts = seeds, hmap, dt2, dts, counts

    def __repr__(self):
        return "WatershedSeeds(shape=%s)" % (tuple(self.seeds.shape),)


class Watershed(object):
    """labels  int32 [N, Y, X]: the kept fragments 1 .. n per plane in ascending order of seed id (stack_ids: offset by the kept counts
            of the planes before), 0 only in a plane without seeds
    counts  int32 [N, 2] = (fragments found by the first flood, fragments kept)
    stats   int32 [N, 2] = (rounds of the last flood that hooked a tree, pixels left 0)"""

    def __init__(self, labels, counts, stats):
        self.labels, self.counts, self.stats = labels, counts, stats

    def __repr__(self):
        return "Watershed(shape=%s)" % (tuple(self.labels.shape),)


def gauss_radius(sigma):
    """(int)(3 sigma + 0.5) of the float32 sigma: vigra's window ratio, scipy's truncate=3.0"""
    return int(3.0 * float(np.float32(sigma)) + 0.5)


def _planes(x, name, dtype_ok, gpu=True):
    """-> (dense [N, Y, X] tensor, had_batch): shape, dtype and ranges first, then the device"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if x.dim() not in (2, 3):
        raise ValueError("%s must be [Y, X] or [N, Y, X], got %s" % (name, tuple(x.shape)))
    if x.dtype not in dtype_ok:
        raise TypeError("%s must be %s, got %s" % (name, " or ".join(str(d).replace("torch.", "") for d in dtype_ok), x.dtype))
    if min(x.shape) < 1:
        raise ValueError("%s has an empty dimension: %s" % (name, tuple(x.shape)))
    if int(x.shape[-1]) * int(x.shape[-2]) >= 2 ** 30:
        raise ValueError("a plane of %d x %d pixels: the watershed serves fewer than 2^30 per plane" % (int(x.shape[-2]), int(x.shape[-1])))
    if gpu:
        _require_gpu(x, name)
    batched = x.dim() == 3
    x = x.detach()
    if not batched:
        x = x[None]
    return (x if x.is_contiguous() else x.contiguous()), batched


def _sigma(sigma, name, shape):
    s = float(sigma)
    if not (s >= 0.0 and s < float("inf")):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, sigma))
    r = gauss_radius(s)
    if s and (r > _lib.WS_MAX_RADIUS or r >= min(int(shape[-1]), int(shape[-2]))):
        raise ValueError("%s = %r is a Gaussian of radius %d: the kernels serve a radius up to %d that is smaller than both extents of "
                         "the plane %s" % (name, sigma, r, _lib.WS_MAX_RADIUS, tuple(shape[-2:])))
    return s


def _conn(c, name):
    if c not in (1, 2):
        raise ValueError("%s must be 1 (the 4-neighbourhood) or 2 (the 8-neighbourhood), got %r" % (name, c))
    return int(c)


def _desc(x, threshold=0.0, sigma_seeds=0.0, sigma_weights=0.0, alpha=0.0, maxima_connectivity=2, seed_connectivity=1, min_size=0, flags=0):
    d = _lib.PeaWsDesc()
    d.N, d.Y, d.X = (int(v) for v in x.shape)
    d.threshold, d.sigma_seeds, d.sigma_weights, d.alpha = threshold, sigma_seeds, sigma_weights, alpha
    d.maxima_connectivity, d.seed_connectivity, d.min_size, d.flags = maxima_connectivity, seed_connectivity, min_size, flags
    return d


def _seeds(x, d, want_dt2, want_hmap):
    """pea_ws_seeds on a dense device tensor [N, Y, X] -> (seeds, hmap, dt2, dts, counts)"""
    L = _lib.lib()
    dev = x.device
    with _on_device(dev):
        seeds = torch.empty(x.shape, dtype=torch.int32, device=dev)
        dts = torch.empty(x.shape, dtype=torch.float32, device=dev)
        dt2 = torch.empty(x.shape, dtype=torch.int32, device=dev) if want_dt2 else None
        hmap = torch.empty(x.shape, dtype=torch.float32, device=dev) if want_hmap else None
        counts = torch.empty((d.N,), dtype=torch.int32, device=dev)
        nb = int(L.pea_ws_seeds_workspace_bytes(ctypes.byref(d)))
        work = stream_workspace("ws_seeds", dev, nb, _no_init, "pea_ws_seeds' workspace")
        _lib.check(L.pea_ws_seeds(ctypes.byref(d), _ptr(x), _ptr(dt2), _ptr(dts), _ptr(hmap), _ptr(seeds), _ptr(counts), _ptr(work), nb,
                                  _stream()), "pea_ws_seeds")
    return seeds, hmap, dt2, dts, counts


def _squeeze(batched, *ts):
    return ts if batched else tuple(None if t is None else t[0] for t in ts)


def watershed_seeds(boundary, threshold, sigma_seeds=2., sigma_weights=2., alpha=.9, maxima_connectivity=2, seed_connectivity=1):
    """The first half of elf's distance_transform_watershed on a batch of planes -> WatershedSeeds (seeds, hmap, dt2, dts, counts).

    boundary   float32 [N, Y, X] or [Y, X] on the GPU (a view that is not dense is copied); planes never touch
    threshold  boundary > threshold is a boundary pixel; dt2 is the exact squared Euclidean distance to the nearest one
    sigma_*    Gaussians of radius (int)(3 sigma + 0.5), mirrored border; 0 skips the filter
    alpha      the height map blends alpha * boundary with (1 - alpha) * the inverted, normalised distance
    maxima_connectivity  2: a plateau and its neighbours are taken in the 8-neighbourhood (vigra's localMaxima), 1: in the 4-
    seed_connectivity    the neighbourhood in which the pixels of the maxima are joined into seeds (1: the 4-)"""
    thr = float(threshold)
    if thr != thr or thr in (float("inf"), float("-inf")):
        raise ValueError("threshold must be finite, got %r" % (threshold,))
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError("alpha must lie in [0, 1], got %r" % (alpha,))
    mc, sc = _conn(maxima_connectivity, "maxima_connectivity"), _conn(seed_connectivity, "seed_connectivity")
    if isinstance(boundary, torch.Tensor) and boundary.dim() in (2, 3) and min(boundary.shape) >= 1:
        ss, sw = _sigma(sigma_seeds, "sigma_seeds", boundary.shape), _sigma(sigma_weights, "sigma_weights", boundary.shape)
        if int(boundary.shape[-1]) ** 2 + int(boundary.shape[-2]) ** 2 > _INT32_MAX:
            raise ValueError("a plane of %s pixels: the squared distance must fit an int32" % (tuple(boundary.shape[-2:]),))
    x, batched = _planes(boundary, "boundary", (torch.float32,))
    d = _desc(x, thr, ss, sw, a, mc, sc)
    return WatershedSeeds(*_squeeze(batched, *_seeds(x, d, True, True)))


def plateau_maxima(field, sigma=0., maxima_connectivity=2, seed_connectivity=1):
    """The plateau maxima of G(sigma) * field as seeds -> WatershedSeeds with .seeds, .dts and .counts (hmap and dt2 are None): the
    last stage of watershed_seeds on a field of the caller (pea_ws_seeds with PEA_WS_FIELD).  fragment.py's 'minima' seeds are
    plateau_maxima(-boundary), its 'maxima_distance' seeds those of the distance transform."""
    mc, sc = _conn(maxima_connectivity, "maxima_connectivity"), _conn(seed_connectivity, "seed_connectivity")
    if isinstance(field, torch.Tensor) and field.dim() in (2, 3) and min(field.shape) >= 1:
        s = _sigma(sigma, "sigma", field.shape)
    x, batched = _planes(field, "field", (torch.float32,))
    d = _desc(x, 0.0, s, 0.0, 0.0, mc, sc, 0, _lib.WS_FIELD)
    return WatershedSeeds(*_squeeze(batched, *_seeds(x, d, False, False)))


def seeded_watershed(hmap, seeds, min_size=0, stack_ids=False):
    """The seeded watershed of a batch of planes -> Watershed (labels, counts, stats).

    hmap      float32 [N, Y, X] or [Y, X] on the GPU
    seeds     int32 of that shape: 0 = none, ids in 1 .. Y * X (any other value is read as 0); pixels of one id need not touch
    min_size  elf's size_filter and a second flood: with min_size > 1, seeds whose fragment has fewer pixels are removed and the flood
              runs again from the rest; a plane in which none would remain keeps its first flood
    stack_ids plane n's ids are offset by the kept counts of the planes before it (the reference's `wsz += offset`)

    The result is the minimum spanning forest relative to the seeds over the 4-neighbour edges ordered by (max of the two heights, edge
    index): every pixel is joined to its seed by a path whose highest point is as low as any path to any seed, and every tie is fixed
    by the definition, so two runs give the same bits."""
    ms = int(min_size)
    if not 0 <= ms <= _INT32_MAX:
        raise ValueError("min_size must lie in 0 .. 2^31 - 1, got %r" % (min_size,))
    if isinstance(hmap, torch.Tensor) and isinstance(seeds, torch.Tensor) and tuple(hmap.shape) != tuple(seeds.shape):
        raise ValueError("hmap %s and seeds %s differ in shape" % (tuple(hmap.shape), tuple(seeds.shape)))
    h, batched = _planes(hmap, "hmap", (torch.float32,), gpu=False)
    s, _ = _planes(seeds, "seeds", (torch.int32,), gpu=False)
    _require_gpu(h, "hmap")
    _require_gpu(s, "seeds")
    d = _desc(h, min_size=ms, flags=_lib.WS_STACK_IDS if stack_ids else 0)
    L = _lib.lib()
    dev = h.device
    with _on_device(dev):
        labels = torch.empty(h.shape, dtype=torch.int32, device=dev)
        counts = torch.empty((d.N, 2), dtype=torch.int32, device=dev)
        stats = torch.empty((d.N, 2), dtype=torch.int32, device=dev)
        nb = int(L.pea_ws_flood_workspace_bytes(ctypes.byref(d)))
        work = stream_workspace("ws_flood", dev, nb, _no_init, "pea_ws_flood's workspace")
        _lib.check(L.pea_ws_flood(ctypes.byref(d), _ptr(h), _ptr(s), _ptr(labels), _ptr(counts), _ptr(stats), _ptr(work), nb, _stream()),
                   "pea_ws_flood")
    return Watershed(*_squeeze(batched, labels, counts, stats))


def distance_transform_watershed(boundary, threshold, sigma_seeds, sigma_weights=2., min_size=100, alpha=.9, pixel_pitch=None,
                                 apply_nonmax_suppression=False, mask=None):
    """elf.segmentation.watershed.distance_transform_watershed under its name, argument order and defaults -> (labels, max_id).

    boundary  [Y, X], or [Z, Y, X] which is processed plane by plane with stacked ids (the reference's loop with `wsz += offset`).  A
              tensor on the GPU gives (int32 tensor, 0-dim int64 tensor), both on the device and without a host synchronisation; a numpy
              array goes through the device and gives (int32 array, int).
    pixel_pitch, apply_nonmax_suppression and mask are not served: anything but their defaults raises NotImplementedError."""
    if pixel_pitch is not None or apply_nonmax_suppression or mask is not None:
        raise NotImplementedError("pixel_pitch, apply_nonmax_suppression and mask of elf's distance_transform_watershed are not served "
                                  "on the device: leave them at their defaults")
    as_numpy = isinstance(boundary, np.ndarray)
    if as_numpy:
        if boundary.ndim not in (2, 3):
            raise ValueError("boundary must be [Y, X] or [Z, Y, X], got %s" % (tuple(boundary.shape),))
        if not np.issubdtype(boundary.dtype, np.floating):
            raise TypeError("boundary must hold floats, got %s" % boundary.dtype)
        b = torch.from_numpy(np.ascontiguousarray(boundary, dtype=np.float32))
        _sigma(sigma_seeds, "sigma_seeds", b.shape), _sigma(sigma_weights, "sigma_weights", b.shape)
        if not torch.cuda.is_available():
            raise RuntimeError("distance_transform_watershed runs on an MI355X only (no CPU fallback), and no GPU is visible")
        b = b.cuda()
    else:
        b = boundary
        if isinstance(b, torch.Tensor) and b.is_floating_point() and b.dtype != torch.float32:
            b = b.to(torch.float32)
    s = watershed_seeds(b, threshold, sigma_seeds, sigma_weights, alpha)
    w = seeded_watershed(s.hmap, s.seeds, min_size=min_size, stack_ids=True)
    max_id = w.counts[..., 1].sum(dtype=torch.int64)
    if as_numpy:
        return w.labels.cpu().numpy(), int(max_id)
    return w.labels, max_id
