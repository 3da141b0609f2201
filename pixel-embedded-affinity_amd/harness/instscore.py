"""The instance scores of the BBBC039V1 validation loop on the device (include/pea_instscore.h: pea_inst_scores): what the reference's
driver computes per validation image,

  scripts_bbbc039v1/main.py:425-429, inference.py:201-205   agg_jc_index, pixel_f1, remap_label and get_fast_pq(match_iou=0.5) of
                                                            utils/metrics_bbbc.py

from ONE contingency table of the predicted against the ground-truth label image: the streaming pass of segmentation_scores, two
launches over the table's slots, one scan per image, the AJI walk (one wave per image) and a finish.  No host synchronisation for a
device tensor of up to 32 bits with max_id given or left at its device default (the call can be captured with pea.graphed); every
column is bit-reproducible.  utils/metrics_bbbc.py carries the reference's names and signatures.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _on_device, _ptr, _stream, stream_workspace
from .segscore import _ScoreTable, _args, default_capacity

_HOST_ID_FLOOR = 1  # max_id of an image without any id


def _workspace(dev, nb):
    """the workspace of pea_inst_scores for the CURRENT stream of `dev` (every call leaves it all zero but for the magic word: ready
    for ANY descriptor that fits)"""
    return stream_workspace("inst", dev, nb, _lib.lib().pea_inst_workspace_init, "pea_inst_workspace_init")


def _host_max(x):
    """the largest id of a numpy array or CPU tensor, None for a device tensor"""
    if isinstance(x, np.ndarray):
        return int(x.max()) if x.size else 0
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        return int(x.max()) if x.numel() else 0
    return None


def default_max_id(pred, gt):
    """max_id when the caller names none: the maximum over both images where both are on the host (numpy arrays, CPU tensors: the
    normal case, the segmentation comes from elf), at least 1 and at most 65535 (a larger id is then counted in n_bad); 65535 as soon
    as one is a device tensor, so that no synchronisation is added"""
    mp, mg = _host_max(pred), _host_max(gt)
    if mp is None or mg is None:
        return _lib.INST_MAX_ID
    return min(_lib.INST_MAX_ID, max(_HOST_ID_FLOOR, mp, mg))


def _check_match_iou(match_iou):
    m = float(match_iou)
    if not 0.0 <= m <= 1.0:
        raise ValueError("match_iou must lie in [0, 1], got %r" % (match_iou,))
    if m < 0.5:
        raise NotImplementedError("match_iou = %r < 0.5 is the Munkres branch of get_fast_pq (linear_sum_assignment on the host), which "
                                  "is not served: only match_iou >= 0.5, where the pairing is unique" % (match_iou,))
    return m


def _launch(P, G, capacity, max_id, match_iou):
    d = _lib.PeaInstDesc()
    d.B, d.S, d.capacity, d.max_id, d.match_iou, d.flags = int(P.shape[0]), int(P.shape[1]), int(capacity), int(max_id), float(match_iou), 0
    L = _lib.lib()
    rc = L.pea_inst_validate(ctypes.byref(d))
    if rc:
        raise ValueError("invalid instance-score descriptor (%s): B=%d, S=%d, capacity=%d (a power of two >= %d), max_id=%d (1 .. %d), "
                         "match_iou=%r" % (L.pea_strerror(rc).decode(), d.B, d.S, d.capacity, _lib.INST_MIN_CAPACITY, d.max_id,
                                           _lib.INST_MAX_ID, d.match_iou))
    dev = P.device
    with _on_device(dev):
        out = torch.empty((d.B, _lib.INST_COLS), dtype=torch.float64, device=dev)
        match = torch.empty((2, d.B, d.max_id + 1), dtype=torch.int32, device=dev)
        nb = int(L.pea_inst_workspace_bytes(ctypes.byref(d)))
        work = _workspace(dev, nb)
        _lib.check(L.pea_inst_scores(ctypes.byref(d), _ptr(P), _ptr(G), _ptr(out), _ptr(match[0]), _ptr(match[1]), _ptr(work), nb, _stream()),
                   "pea_inst_scores")
    return out, match


class InstanceScores(_ScoreTable):
    """The device table [B, 18] (float64; columns _lib.INST_COLUMNS) of one instance_scores call and its two match tables.  Nothing is
    copied to the host until a value is asked for.  The properties give a Python number for a single image and a list over the batch
    otherwise: .aji / .dq / .sq / .pq / .pixel_f1 / .tp / .fp / .fn / .n_bad / .n_overflow; .table is the device tensor,
    .aji_match(b) the pred id that every gt id of image b took in the AJI walk, .pq_pairs(b) the pairing lists of get_fast_pq.

    If the first read finds n_overflow != 0 (the table was too small for the image's pairs), the call is repeated ONCE with four times
    the capacity; if that overflows too, RuntimeError."""

    COLUMNS = _lib.INST_COLUMNS

    def __init__(self, table, match, pred, gt, capacity, max_id, match_iou):
        self.table, self.match, self.capacity, self.max_id, self.match_iou = table, match, int(capacity), int(max_id), float(match_iou)
        self._pred, self._gt = pred, gt
        self._host = None
        self._host_match = None

    def _relaunch(self, capacity):
        self.table, self.match = _launch(self._pred, self._gt, capacity, self.max_id, self.match_iou)

    aji = property(lambda self: self._col("aji"))
    dq = property(lambda self: self._col("dq"))
    sq = property(lambda self: self._col("sq"))
    pq = property(lambda self: self._col("pq"))
    pixel_f1 = property(lambda self: self._col("pixel_f1"))
    tp = property(lambda self: self._col("tp", int))
    fp = property(lambda self: self._col("fp", int))
    fn = property(lambda self: self._col("fn", int))
    n_overflow = property(lambda self: self._col("n_overflow", int))
    n_bad = property(lambda self: self._col("n_bad", int))

    def _matches(self, b):
        B = int(self._pred.shape[0])
        if not 0 <= int(b) < B:
            raise IndexError("image %r of a batch of %d" % (b, B))
        self._rows()  # (settles the capacity)
        if self._host_match is None:
            self._host_match = self.match.detach().cpu().numpy()
        return self._host_match[:, int(b)]

    def aji_match(self, b=0):
        """-> int32 [max_id + 1]: entry j is the pred id that gt id j took in the AJI walk, 0 for j = 0 and for absent j"""
        return self._matches(b)[0].copy()

    def pq_pairs(self, b=0):
        """-> paired_true, paired_pred, unpaired_true, unpaired_pred of get_fast_pq, in the caller's ids: the gt ids that have a pred
        with iou > match_iou in increasing order and those preds beside them (int64 arrays), then the lists of the remaining gt and
        pred ids > 0 (one more pass over image b: the ids come from its contingency table)"""
        pq = self._matches(b)[1]
        paired_true = np.nonzero(pq)[0].astype(np.int64)
        paired_pred = pq[paired_true].astype(np.int64)
        pred_ids, gt_ids = self._ids(b)
        taken_t, taken_p = set(paired_true.tolist()), set(paired_pred.tolist())
        return (paired_true, paired_pred, [j for j in gt_ids if j not in taken_t], [i for i in pred_ids if i not in taken_p])

    def _ids(self, b):
        """the ids > 0 of pred and of gt of image b, sorted (one copy of the two label rows)"""
        p, g = np.unique(self._pred[int(b)].cpu().numpy()), np.unique(self._gt[int(b)].cpu().numpy())
        return [int(v) for v in p if v > 0], [int(v) for v in g if v > 0]

    def __repr__(self):
        return "InstanceScores(aji=%s, pq=%s, pixel_f1=%s)" % (self.aji, self.pq, self.pixel_f1)


def instance_scores(pred, gt, *, max_id=None, capacity=None, batched=None, match_iou=0.5):
    """AJI, DQ / SQ / PQ and pixel F1 of a predicted against a ground-truth instance image -> InstanceScores.

    pred, gt   label images of one shape, ids in [0, max_id], background 0: a device tensor is used as it is, a numpy array or CPU
               tensor is uploaded.  Dtypes as segmentation_scores takes them (labels_int32).  A negative id or one above max_id is
               counted in n_bad and makes that image's scores NaN.
    max_id     the largest id of either image, 1 .. 65535; None: default_max_id (the maximum on the host for numpy arrays and CPU
               tensors, 65535 for device tensors: no synchronisation)
    batched    as segmentation_scores: None batches where there are more than two dimensions
    capacity   slots per image of the pair table, a power of two >= 64; None: default_capacity(S)
    match_iou  the pairing threshold of PQ, >= 0.5 (below it the reference runs Munkres: NotImplementedError)"""
    m = _check_match_iou(match_iou)
    if batched is None:
        batched = len(getattr(pred, "shape", ())) > 2
    mid = None if max_id is None else int(max_id)
    if mid is not None and not 1 <= mid <= _lib.INST_MAX_ID:
        raise ValueError("max_id must lie in 1 .. %d, got %r" % (_lib.INST_MAX_ID, max_id))
    P, G = _args(pred, gt, bool(batched))
    if mid is None:
        mid = default_max_id(pred, gt)
    cap = default_capacity(P.shape[1]) if capacity is None else int(capacity)
    out, match = _launch(P, G, cap, mid, m)
    return InstanceScores(out, match, P, G, cap, mid, m)
