"""The reference's utils/metrics_bbbc.py (scripts_bbbc039v1/: the instance scores of the nuclei validation loop) under its own names
and signatures, computed on the device from one contingency table (harness/instscore.py, include/pea_instscore.h) instead of one
full-image mask per instance and several full-image numpy passes per (gt instance, pred id) pair.

Every function takes numpy arrays or tensors (on any device) of integer ids, background 0, and returns Python numbers.  Two inputs that
the reference does not define are defined in the header: a gt id absent between 1 and the maximum is skipped by agg_jc_index, and a
pred without any id > 0 gives 0 (NaN when gt has none either).  get_fast_pq does not need consecutive ids: its lists speak in the
caller's ids, and remap_label is kept for callers that relabel anyway.  BestDice and FGBGDice are those of utils/evaluate.py.
"""
import numpy as np

from ..harness.instscore import instance_scores
from ..harness.segscore import labels_int32
from .evaluate import BestDice, FGBGDice  # noqa: F401  (the reference's file carries them too)


def _scores(gt, pred, match_iou=0.5):
    return instance_scores(pred, gt, batched=False, match_iou=match_iou)


def agg_jc_index(gt_ins, pred):
    """the aggregated Jaccard index of pred against gt_ins: every gt instance, in id order, takes the best-IoU prediction that no
    earlier instance took (pred id 1 where none overlaps); sum of intersections over sum of unions plus the unused predictions"""
    return _scores(gt_ins, pred).aji


def pixel_f1(gt_ins, pred_ins):
    """F1 of the foreground masks (id > 0); 0 where neither image has foreground"""
    return _scores(gt_ins, pred_ins).pixel_f1


def get_fast_pq(true, pred, match_iou=0.5):
    """-> [dq, sq, pq], [paired_true, paired_pred, unpaired_true, unpaired_pred]: a gt and a pred instance pair up where their
    IoU > match_iou (unique for match_iou >= 0.5; below it the reference runs Munkres, which is not served: NotImplementedError)"""
    s = _scores(true, pred, match_iou)
    return [s.dq, s.sq, s.pq], list(s.pq_pairs(0))


def remap_label(pred, by_size=False):
    """ids renamed to 1 .. n (0 stays): in increasing order of the old id, or by_size with the larger instance first (ties keep the
    id order).  A host relabel in numpy -> int32 array of pred's shape; a pred without ids comes back as it is."""
    a = labels_int32(pred, "pred").cpu().numpy() if not isinstance(pred, np.ndarray) else pred
    ids, inverse, counts = np.unique(a, return_inverse=True, return_counts=True)
    fg = ids != 0
    if not fg.any():
        return pred
    order = np.nonzero(fg)[0]
    if by_size:
        order = order[np.argsort(-counts[order], kind="stable")]
    new = np.zeros(len(ids), np.int32)
    new[order] = np.arange(1, len(order) + 1, dtype=np.int32)
    return new[inverse].reshape(a.shape)
