"""The small-segment merges and the renumbering on the device (include/pea_merge.h: pea_merge_small) -- what the reference's validation
and inference loops do on the host between seg_mutex and the scores,

  scripts_cvppp/utils/postprocessing.py, scripts_bbbc039v1/utils/postprocessing.py   merge_small_object, merge_func
  scripts_cvppp/utils/seg_waterz.py                                                   relabel

as launches of csrc/pea_k_merge.hip: the per-id moments in one streaming pass, one workgroup per image that walks the small ids in
ascending order through an alias table, the numbering and one streaming projection.  With an integer max_id nothing is read back and
the call can be captured with pea.graphed.  The order among EQUAL counts in a window is this library's (count descending, then id
ascending: a stable argsort); the reference's np.argsort leaves it to the sort.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _no_init, _on_device, _ptr, _require_gpu, _stream, stream_workspace

# (threshold, window) of the four passes of the reference's merge_func
CVPPP_MERGE_PASSES = ((5, 5), (20, 11), (50, 11), (300, 21))   # scripts_cvppp/utils/postprocessing.py:35-40
BBBC_MERGE_PASSES = ((5, 5), (25, 11), (50, 11), (100, 21))    # scripts_bbbc039v1/utils/postprocessing.py:36-41
_INT32_MAX = 2 ** 31 - 1


class MergedSegments(object):
    """labels  int32, the shape of the input: every small segment under the id it was merged into (renumbered 1 .. n with relabel=True)
    counts  int32 [B] (0-dim for one image): the ids above 0 that are left
    stats   int64 [B, 8] ([8] for one image): the columns _lib.MERGE_STAT_COLUMNS; stats[..., 4] > 0 says that ids lay outside
            [0, max_id] and were written through
    All three are device tensors; nothing is copied to the host."""

    def __init__(self, labels, counts, stats):
        self.labels, self.counts, self.stats = labels, counts, stats

    def __repr__(self):
        return "MergedSegments(shape=%s)" % (tuple(self.labels.shape),)

    def stat(self, name):
        return self.stats[..., _lib.MERGE_STAT_COLUMNS.index(name)]


def _arguments(seg, passes, relabel, max_id):
    """everything that can be said without a device -> (descriptor without max_id, batched)"""
    if not isinstance(seg, torch.Tensor):
        raise TypeError("seg must be a torch.Tensor")
    if seg.dim() not in (2, 3):
        raise ValueError("seg must be [Y, X] or [B, Y, X], got %s" % (tuple(seg.shape),))
    if seg.dtype != torch.int32:
        raise TypeError("seg must be int32, got %s: convert a label image once with .to(torch.int32)" % seg.dtype)
    if min(seg.shape) < 1:
        raise ValueError("seg has an empty dimension: %s" % (tuple(seg.shape),))
    batched = seg.dim() == 3
    Y, X = int(seg.shape[-2]), int(seg.shape[-1])
    if Y * X > _INT32_MAX:
        raise ValueError("an image of %d pixels: pea_merge_small serves fewer than 2^31 per image" % (Y * X))
    passes = [tuple(p) for p in passes]
    if not 1 <= len(passes) <= _lib.MERGE_MAX_PASSES or any(len(p) != 2 for p in passes):
        raise ValueError("passes must be 1 .. %d pairs (threshold, window), got %r" % (_lib.MERGE_MAX_PASSES, passes))
    d = _lib.PeaMergeDesc()
    d.B, d.Y, d.X, d.n_passes = (int(seg.shape[0]) if batched else 1), Y, X, len(passes)
    for k, (t, w) in enumerate(passes):
        t, w = int(t), int(w)
        if not 0 <= t <= _INT32_MAX:
            raise ValueError("a threshold must lie in 0 .. 2^31 - 1, got %r" % (t,))
        if not 1 <= w <= _lib.MERGE_MAX_WINDOW:
            raise ValueError("a window must lie in 1 .. %d (the crop's id table is held in LDS), got %r" % (_lib.MERGE_MAX_WINDOW, w))
        if w > min(Y, X):
            raise ValueError("a window of %d on an image of %d x %d: the window may not exceed the image" % (w, Y, X))
        d.threshold[k], d.window[k] = t, w
    d.flags = _lib.MERGE_RELABEL if relabel else 0
    if max_id is not None and not 0 <= int(max_id) <= _INT32_MAX - 1:
        raise ValueError("max_id must be None or lie in 0 .. 2^31 - 2, got %r" % (max_id,))
    return d, batched


def merge_small_objects(seg, passes=CVPPP_MERGE_PASSES, relabel=False, max_id=None):
    """The reference's merge_func (and relabel) on a batch of label images -> MergedSegments (labels, counts, stats), all on the device.

    seg      int32 [Y, X] or [B, Y, X] on the GPU (a view that is not dense is copied), ids in [0, max_id]
    passes   1 .. 8 pairs (threshold, window): one merge_small_object each, in order (CVPPP_MERGE_PASSES, BBBC_MERGE_PASSES)
    relabel  True: the ids above 0 that are left are renumbered 1 .. n in ascending id order, the reference's relabel
    max_id   None: seg.max() is read back (one synchronisation); an integer: nothing is read back and the call can be captured --
             ids above it are written through and counted in stats[..., 4]"""
    d, batched = _arguments(seg, passes, relabel, max_id)
    _require_gpu(seg, "seg")
    x = seg.detach()
    x = x if x.is_contiguous() else x.contiguous()
    if max_id is None:
        max_id = int(x.max())  # the one synchronisation
        if max_id < 0:
            max_id = 0
        if max_id > _INT32_MAX - 1:
            raise ValueError("seg holds the id 2^31 - 1: ids up to 2^31 - 2 are served")
    d.max_id = int(max_id)
    L = _lib.lib()
    dev = x.device
    with _on_device(dev):
        labels = torch.empty(x.shape, dtype=torch.int32, device=dev)
        counts = torch.empty((d.B,), dtype=torch.int32, device=dev)
        stats = torch.empty((d.B, _lib.MERGE_STATS), dtype=torch.int64, device=dev)
        nb = int(L.pea_merge_workspace_bytes(ctypes.byref(d)))
        work = stream_workspace("merge", dev, nb, _no_init, "pea_merge_small's workspace")
        _lib.check(L.pea_merge_small(ctypes.byref(d), _ptr(x), _ptr(labels), _ptr(counts), _ptr(stats), _ptr(work), nb, _stream()), "pea_merge_small")
    if not batched:
        counts, stats = counts[0], stats[0]
    return MergedSegments(labels, counts, stats)
