"""The reference's merge_small_object / merge_func (scripts_cvppp/utils/postprocessing.py, scripts_bbbc039v1/utils/postprocessing.py) and
relabel (utils/seg_waterz.py) under their own names and signatures, on the device (harness/merge.py, include/pea_merge.h):

    pred_seg = seg_mutex(output_affs, offsets=offsets, strides=list(cfg.DATA.strides), mask=pred_mask).astype(np.uint16)
    pred_seg = merge_func(pred_seg)                      # four passes of merge_small_object
    pred_seg = relabel(pred_seg)

The two loops differ only in the passes: merge_func is CVPPP's, merge_func_bbbc is BBBC039V1's.  [Y, X] (the reference's call) or
[B, Y, X].  An int32 tensor on the GPU gives an int32 tensor on the GPU and nothing is copied to the host; a numpy array is uploaded,
merged on the device and comes back as numpy with its dtype kept.  Where the reference ranks equal counts in a window by whatever its
unstable np.argsort makes of them, the order here is count descending, then id ascending (include/pea_merge.h); and the ids are int32
on the device, so nothing wraps at 65536 as the reference's uint16 cast does.  Unlike the reference's functions these do not change
their argument.
"""
import numpy as np
import torch

from ..harness.merge import BBBC_MERGE_PASSES, CVPPP_MERGE_PASSES, merge_small_objects

__all__ = ["merge_small_object", "merge_func", "merge_func_bbbc", "relabel", "CVPPP_MERGE_PASSES", "BBBC_MERGE_PASSES"]


def _to_device(seg):
    """a numpy label image -> an int32 device tensor"""
    a = np.ascontiguousarray(seg)
    if a.dtype.kind not in "iu":
        raise TypeError("seg must hold integers, got %s" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 2):
        raise ValueError("seg holds ids outside 0 .. 2^31 - 2")
    if not torch.cuda.is_available():
        raise RuntimeError("the merges run on an MI355X only (no CPU fallback), and no GPU is visible")
    return torch.from_numpy(a.astype(np.int32)).cuda()


def _run(seg, passes, relabel):
    as_numpy = isinstance(seg, np.ndarray)
    if not as_numpy and not isinstance(seg, torch.Tensor):
        raise TypeError("seg must be a numpy array or a torch.Tensor, got %s" % type(seg).__name__)
    if len(seg.shape) not in (2, 3):
        raise ValueError("seg must be [Y, X] or [B, Y, X], got %s" % (tuple(seg.shape),))
    out = merge_small_objects(_to_device(seg) if as_numpy else seg, passes=passes, relabel=relabel).labels
    return out.cpu().numpy().astype(seg.dtype) if as_numpy else out


def merge_small_object(seg, threshold=5, window=5):
    """one pass: every id of at most `threshold` pixels takes the id that is most frequent in the window around its centroid"""
    return _run(seg, ((threshold, window),), False)


def merge_func(seg, step=4):
    """the four passes of the CVPPP loop (`step` is unused there as well)"""
    return _run(seg, CVPPP_MERGE_PASSES, False)


def merge_func_bbbc(seg, step=4):
    """the four passes of the BBBC039V1 loop"""
    return _run(seg, BBBC_MERGE_PASSES, False)


def relabel(seg):
    """the ids above 0 renumbered 1 .. n in ascending order, 0 kept: a threshold of 0 makes no id a candidate, so the one pass merges
    nothing and only the numbering runs"""
    return _run(seg, ((0, 1),), True)
