"""The reference's utils/seg_waterz.py (scripts_cvppp/, scripts_bbbc039v1/) under its own names, and waterz's agglomerate under its
name for the call sites of scripts_ac3ac4/main.py and inference.py, on the device (harness/agglo.py, include/pea_agglo.h):

    def seg_waterz(affs, mask=None):
        fragments = gen_fragment(affs)                      # maxima_distance seeds, flood of 1 - min(affs[0], affs[1])
        fragments[mask == 0] = 0
        sf = 'OneMinus<EdgeStatisticValue<RegionGraphType, MeanAffinityProvider<RegionGraphType, ScoreValue>>>'
        segmentation = list(waterz.agglomerate(affs_expend, [0.50], fragments=fragments, scoring_function=sf, discretize_queue=256))[0]
        return segmentation, fragments

A tensor on the GPU gives int32 tensors on the GPU; a numpy array is uploaded, segmented on the device and comes back as numpy
(uint64, the reference's dtype).  The fragments are the package's maxima_distance watershed (utils/fragment.py: plateau maxima in the
4-neighbourhood, the watershed cut of include/pea_ws.h), not mahotas'.  The merge order among EQUAL scores is this library's round
rule: waterz's discretize_queue=256 puts the scores into 256 bins and leaves the order inside a bin to its queue, so discretize_queue
is accepted and not reproduced.  The cost of an edge is the mean of fl(1 - a) over its samples, which differs from waterz's
1 - mean(a) by rounding, at most 2^-24.  Segment ids are 1 .. n in ascending order of the clusters' smallest fragment id (what the
reference's relabel makes of waterz's ids).
"""
import re

import numpy as np
import torch

from ..harness.agglo import agglomerate as _agglomerate
from ..harness.ws import seeded_watershed
from . import fragment as _fragment

__all__ = ["seg_waterz", "relabel", "agglomerate", "gen_fragment", "scoring_linkage"]

MEAN_SF = "OneMinus<EdgeStatisticValue<RegionGraphType, MeanAffinityProvider<RegionGraphType, ScoreValue>>>"
# the scoring functions that are served, spaces removed -> the linkage ON THE COST 1 - a: the smallest affinity is the largest cost
_SCORING = {
    "OneMinus<EdgeStatisticValue<RegionGraphType,MeanAffinityProvider<RegionGraphType,ScoreValue>>>": "mean",
    "OneMinus<MeanAffinity<RegionGraphType,ScoreValue>>": "mean",
    "OneMinus<MinAffinity<RegionGraphType,ScoreValue>>": "max",
    "OneMinus<MaxAffinity<RegionGraphType,ScoreValue>>": "min",
    "OneMinus<EdgeStatisticValue<RegionGraphType,MinAffinityProvider<RegionGraphType,ScoreValue>>>": "max",
    "OneMinus<EdgeStatisticValue<RegionGraphType,MaxAffinityProvider<RegionGraphType,ScoreValue>>>": "min",
}


def scoring_linkage(scoring_function):
    """a waterz scoring-function string -> the linkage of pea.agglomerate; NotImplementedError that names it for any other"""
    key = re.sub(r"\s+", "", str(scoring_function))
    if key not in _SCORING:
        raise NotImplementedError("scoring_function %r is not served on the device (the mean-, min- and max-affinity forms are; "
                                  "HistogramQuantileAffinity needs a histogram per edge: include/pea_agglo.h)" % (scoring_function,))
    return _SCORING[key]


def relabel(seg):
    """the reference's relabel: the ids > 0 renumbered 1 .. n in ascending order, 0 kept; numpy or tensor"""
    if isinstance(seg, torch.Tensor):
        return _fragment.relabel(seg)
    seg = np.asarray(seg)
    ids, rank = np.unique(seg, return_inverse=True)  # rank: the position of every element's id among the sorted ids
    rank = rank.reshape(seg.shape)
    if ids.size and ids[0] <= 0:  # ids <= 0 stay as they are and take no number: the positive ids start at 1 behind them
        kept = int((ids <= 0).sum())
        return np.where(seg > 0, rank - kept + 1, seg).astype(seg.dtype)
    return (rank + 1).astype(seg.dtype)


def gen_fragment(affs):
    """the reference's gen_fragment on the device: affs float32 [2, H, W] on the GPU -> int32 [H, W], the flood of
    1 - min(affs[0], affs[1]) from the maxima_distance seeds"""
    boundary = (1.0 - torch.minimum(affs[0], affs[1]))[None].contiguous()
    seeds, _ = _fragment.get_seeds(boundary, "maxima_distance")
    return seeded_watershed(boundary, seeds, min_size=0, stack_ids=True).labels[0]


def seg_waterz(affs, mask=None):
    """the reference's seg_waterz: affs [2, H, W] (offsets (-1, 0), (0, -1)), mask [H, W] or None -> (segmentation, fragments)"""
    if not isinstance(affs, (np.ndarray, torch.Tensor)):
        raise TypeError("affs must be a numpy array or a torch.Tensor, got %s" % type(affs).__name__)
    if len(affs.shape) != 3 or int(affs.shape[0]) != 2:
        raise ValueError("affs must be [2, H, W], got %s" % (tuple(affs.shape),))
    if mask is not None and tuple(mask.shape) != tuple(affs.shape[1:]):
        raise ValueError("mask %s does not go with affs %s" % (tuple(mask.shape), tuple(affs.shape)))
    as_numpy = isinstance(affs, np.ndarray)
    if as_numpy:
        if not np.issubdtype(affs.dtype, np.floating):
            raise TypeError("the affinities must hold floats, got %s" % affs.dtype)
        if not torch.cuda.is_available():
            raise RuntimeError("seg_waterz runs on an MI355X only (no CPU fallback), and no GPU is visible")
        a = torch.from_numpy(np.ascontiguousarray(affs, dtype=np.float32)).cuda()
    else:
        if not affs.is_cuda:
            raise RuntimeError("affs is on %s: seg_waterz runs on an MI355X only (no CPU fallback)" % affs.device)
        a = affs.detach().to(torch.float32)
    fragments = gen_fragment(a)
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)) if isinstance(mask, np.ndarray) else (mask != 0)
        fragments = torch.where(m.to(a.device), fragments, torch.zeros_like(fragments))
    segmentation = next(_agglomerate(a, [0.50], fragments=fragments, linkage="mean"))
    if as_numpy:
        return segmentation.cpu().numpy().astype(np.uint64), fragments.cpu().numpy().astype(np.uint64)
    return segmentation, fragments


def agglomerate(affs, thresholds, fragments=None, scoring_function="OneMinus<MeanAffinity<RegionGraphType, ScoreValue>>", discretize_queue=0):
    """waterz.agglomerate under its name: affs [3, Z, Y, X], ascending thresholds -> a generator of one segmentation per threshold.
    fragments=None makes them on the device (the distance-transform watershed of utils/lmc.py, plane by plane); discretize_queue is
    accepted and not reproduced (the module's docstring).  A numpy affs gives uint64 numpy arrays, waterz's dtype."""
    linkage = scoring_linkage(scoring_function)
    gen = _agglomerate(affs, thresholds, fragments="watershed" if fragments is None else fragments, linkage=linkage)
    if isinstance(affs, np.ndarray):
        return (seg.astype(np.uint64) for seg in gen)
    return gen
