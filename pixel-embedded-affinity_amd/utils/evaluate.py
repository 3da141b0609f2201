"""The reference's utils/evaluate.py (scripts_cvppp/, scripts_bbbc039v1/: the CVPPP leaf-segmentation scores) under its own names and
signatures, computed on the device from one contingency table (harness/segscore.py, include/pea_segscore.h) instead of a Python
double loop over label pairs with several full-image numpy passes per pair.

Every function takes numpy arrays or tensors (on any device) of integer ids and returns a Python number; the shape-mismatch returns
of the reference (-1 for DiffFGLabels, 0 elsewhere) are kept.  Background is the LOWEST label of each image, as in the reference.
Negative ids are not served: the scores of an image that holds one are NaN (SegmentationScores.n_bad counts them).
"""
import numpy as np

from ..harness.segscore import segmentation_scores


def _same_shape(inLabel, gtLabel):
    return tuple(inLabel.shape) == tuple(gtLabel.shape)


def _scores(inLabel, gtLabel):
    return segmentation_scores(inLabel, gtLabel, batched=False)


def DiffFGLabels(inLabel, gtLabel):
    """difference of the number of foreground labels, (max - min) of inLabel minus (max - min) of gtLabel; -1 on a shape mismatch"""
    if not _same_shape(inLabel, gtLabel):
        return -1
    return _scores(inLabel, gtLabel).diff_fg


def BestDice(inLabel, gtLabel):
    """for every label of inLabel but its lowest the best Dice among the labels of gtLabel but its lowest, summed and divided by
    max - min of inLabel; 0 on a shape mismatch or when inLabel holds one label"""
    if not _same_shape(inLabel, gtLabel):
        return 0
    return _scores(inLabel, gtLabel).best_dice


def FGBGDice(inLabel, gtLabel):
    """Dice of the foreground masks (label != the image's lowest); 0 on a shape mismatch"""
    if not _same_shape(inLabel, gtLabel):
        return 0
    return _scores(inLabel, gtLabel).fgbg_dice


def Dice(inLabel, gtLabel, i, j):
    """Dice of label i of inLabel against label j of gtLabel: 2 n_ij / (a_i + b_j), 0 where neither label is present or on a shape
    mismatch"""
    if not _same_shape(inLabel, gtLabel):
        return 0
    p, g, c = _scores(inLabel, gtLabel).contingency(0)
    size = int(c[p == i].sum()) + int(c[g == j].sum())
    overlap = int(c[(p == i) & (g == j)].sum())
    return 2.0 * overlap / size if size > 1e-8 else 0


def AbsDiffFGLabels(inLabel, gtLabel):
    """|DiffFGLabels|"""
    return int(np.abs(DiffFGLabels(inLabel, gtLabel)))


def SymmetricBestDice(inLabel, gtLabel):
    """min(BestDice(inLabel, gtLabel), BestDice(gtLabel, inLabel)), both from one table"""
    if not _same_shape(inLabel, gtLabel):
        return 0
    return _scores(inLabel, gtLabel).sbd
