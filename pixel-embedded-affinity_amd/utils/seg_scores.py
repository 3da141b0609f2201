"""skimage.metrics.adapted_rand_error and variation_of_information as the reference's drivers call them (scripts_*/main.py,
inference.py: `adapted_rand_ref(gt, seg, ignore_labels=(0))[0]`, `voi_ref(gt, seg, ignore_labels=(0))`), computed on the device from
one contingency table (harness/segscore.py); the formulas are stated in include/pea_segscore.h.

The first argument is the ground truth (image_true / image0), whose label 0 is ignored.  ignore_labels=(0,) -- also written 0
or (0), the one form the drivers use -- and ignore_labels=() are served; anything else raises ValueError.
"""
import numpy as np

from ..harness.segscore import labels_int32, segmentation_scores


def _ignores_zero(ignore_labels):
    ig = (ignore_labels,) if np.isscalar(ignore_labels) else tuple(ignore_labels)
    if ig not in ((), (0,)):
        raise ValueError("only ignore_labels=(0,) and () are supported, got %r" % (ignore_labels,))
    return ig == (0,)


def _scores(image_true, image_test, ignore_labels):
    zero = _ignores_zero(ignore_labels)
    if tuple(image_true.shape) != tuple(image_test.shape):
        raise ValueError("the label images differ in shape: %s and %s" % (tuple(image_true.shape), tuple(image_test.shape)))
    if not zero:  # nothing ignored: the scores do not depend on the ids' names, so every id of image_true moves up by one (as int64,
        image_true = labels_int32(image_true, "image_true").long() + 1  # so that the range check of the call sees 2^31 - 1 + 1)
    return segmentation_scores(image_test, image_true, batched=False)


def adapted_rand_error(image_true, image_test, ignore_labels=(0,)):
    """-> (are, precision, recall) as Python floats.  are = 1 - P2 / (0.5 A2 + 0.5 B2); precision = P2 / A2 over the segments of
    image_test, recall = P2 / B2 over the segments of image_true.  An image_true that is all 0 gives NaN (0 / 0)."""
    s = _scores(image_true, image_test, ignore_labels)
    return s.are, s.are_precision, s.are_recall


def variation_of_information(image0, image1, ignore_labels=(0,)):
    """-> array([H(image1 | image0), H(image0 | image1)]) in bits: with image0 the ground truth, (split, merge)"""
    s = _scores(image0, image1, ignore_labels)
    return np.array([s.voi_split, s.voi_merge])
