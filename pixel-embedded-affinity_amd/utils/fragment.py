"""The reference's scripts_ac3ac4/utils/fragment.py under its own names, on the device (harness/ws.py, include/pea_ws.h): the
fragments of an affinity volume affs [3, Z, Y, X] plane by plane, with stacked ids.

  elf_watershed(affs)             distance_transform_watershed(np.maximum((1 - affs)[1], (1 - affs)[2])[z], threshold=.25,
                                  sigma_seeds=2.) per plane, `wsz += offset`
  watershed(affs, seed_method)    the flood of 1 - 0.5 * (affs[1] + affs[2]) from 'grid', 'minima' or 'maxima_distance' seeds
  relabel(seg), remove_small(seg, thres)   as tensor ops

A tensor on the GPU gives an int32 tensor on the GPU; a numpy array goes through the device and gives a numpy array (uint64, the
reference's dtype).  The flood is the watershed cut of include/pea_ws.h: its tie rule is this library's, not mahotas' or vigra's.  The
ids of a plane are 1 .. n in ascending order of its seeds, stacked over the planes; the reference's 'minima' and 'maxima_distance' leave
one id unused per plane (seeds += next_id), which is not reproduced.  randomlabel is not carried: it draws from numpy's global
generator.
"""
import numpy as np
import torch

from ..harness.ws import distance_transform_watershed, plateau_maxima, seeded_watershed, watershed_seeds

__all__ = ["elf_watershed", "watershed", "get_seeds", "relabel", "remove_small"]

SEED_METHODS = ("grid", "minima", "maxima_distance")


def _affs(affs):
    """-> (float32 tensor [C >= 3, Z, Y, X] on the GPU, came as numpy): arguments first, then the device"""
    if not isinstance(affs, (np.ndarray, torch.Tensor)):
        raise TypeError("affs must be a numpy array or a torch.Tensor, got %s" % type(affs).__name__)
    if len(affs.shape) != 4 or int(affs.shape[0]) < 3:
        raise ValueError("affs must be [C >= 3, Z, Y, X] (the in-plane channels are 1 and 2), got %s" % (tuple(affs.shape),))
    as_numpy = isinstance(affs, np.ndarray)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("the fragments are made on an MI355X only (no CPU fallback), and no GPU is visible")
        affs = torch.from_numpy(np.ascontiguousarray(affs[:3], dtype=np.float32)).cuda()
    elif not affs.is_cuda:
        raise RuntimeError("affs is on %s: the fragments are made on an MI355X only (no CPU fallback)" % affs.device)
    return affs.detach().to(torch.float32), as_numpy


def _out(labels, as_numpy):
    return labels.cpu().numpy().astype(np.uint64) if as_numpy else labels


def elf_watershed(affs):
    """the reference's elf_watershed: boundary = max(1 - affs[1], 1 - affs[2]), threshold .25, sigma_seeds 2 (elf's defaults for the
    rest: sigma_weights 2, min_size 100, alpha .9), ids stacked plane by plane"""
    a, as_numpy = _affs(affs)
    boundary = torch.maximum(1 - a[1], 1 - a[2])
    return _out(distance_transform_watershed(boundary, .25, 2.)[0], as_numpy)


def get_seeds(boundary, method="grid", seed_distance=10):
    """seeds int32 of a batch of planes [N, Y, X] on the GPU, numbered from 1 in every plane -> (seeds, counts int32 [N]).
    'grid': every seed_distance-th pixel of every seed_distance-th row, written by one index assignment; 'minima': the plateau minima of
    the boundary map; 'maxima_distance': the plateau maxima of the distance to the nearest pixel with boundary >= 0.5.  (mahotas' regmin /
    regmax and label work in the 4-neighbourhood.)"""
    if method not in SEED_METHODS:
        raise ValueError("seed_method must be one of %s, got %r" % (", ".join(repr(m) for m in SEED_METHODS), method))
    if method == "grid":
        N, Y, X = (int(v) for v in boundary.shape)
        ny, nx = (Y + seed_distance - 1) // seed_distance, (X + seed_distance - 1) // seed_distance
        seeds = torch.zeros((N, Y, X), dtype=torch.int32, device=boundary.device)
        seeds[:, ::seed_distance, ::seed_distance] = torch.arange(1, ny * nx + 1, dtype=torch.int32, device=boundary.device).reshape(ny, nx)
        return seeds, torch.full((N,), ny * nx, dtype=torch.int32, device=boundary.device)
    if method == "minima":
        s = plateau_maxima(-boundary, 0., maxima_connectivity=1, seed_connectivity=1)
        return s.seeds, s.counts
    below_half = float(np.nextafter(np.float32(0.5), np.float32(0)))  # boundary > this <=> boundary >= 0.5
    s = watershed_seeds(boundary, below_half, 0., 0., 1., maxima_connectivity=1, seed_connectivity=1)
    return s.seeds, s.counts


def watershed(affs, seed_method, seed_distance=10):
    """the reference's watershed(affs, seed_method): the flood of 1 - 0.5 * (affs[1] + affs[2]) per plane from the seeds of get_seeds"""
    if seed_method not in SEED_METHODS:
        raise ValueError("seed_method must be one of %s, got %r" % (", ".join(repr(m) for m in SEED_METHODS), seed_method))
    a, as_numpy = _affs(affs)
    affs_xy = (1.0 - 0.5 * (a[1] + a[2])).contiguous()
    seeds, _ = get_seeds(affs_xy, seed_method, seed_distance)
    return _out(seeded_watershed(affs_xy, seeds, min_size=0, stack_ids=True).labels, as_numpy)


def relabel(seg):
    """the ids of seg > 0 renumbered 1 .. n in ascending order, 0 kept (a tensor op: torch.unique synchronises)"""
    if not isinstance(seg, torch.Tensor):
        raise TypeError("seg must be a torch.Tensor")
    uid = torch.unique(seg)
    uid = uid[uid > 0]
    if uid.numel() == 0:
        return seg
    new = torch.searchsorted(uid, seg.contiguous()).to(seg.dtype) + 1
    return torch.where(seg > 0, new, torch.zeros_like(seg))


def remove_small(seg, thres=100):
    """the ids of seg with fewer than thres pixels set to 0 (a tensor op: torch.unique synchronises)"""
    if not isinstance(seg, torch.Tensor):
        raise TypeError("seg must be a torch.Tensor")
    uid, inv, cnt = torch.unique(seg, return_inverse=True, return_counts=True)
    return torch.where((cnt < thres)[inv], torch.zeros_like(seg), seg)
