"""The reference's utils/postprocessing.py (scripts_bbbc039v1/) under its own names, as far as it runs on the device.

remove_samll_object (the reference's spelling: scripts_bbbc039v1/utils/postprocessing.py:43-48) is skimage.morphology.label(mask) --
full connectivity --, remove_small_objects(min_size) -- components of FEWER than min_size pixels go -- and a binarisation.  Here it is
one pea_cc_label call with mask_out only (harness/cc.py, include/pea_cc.h): the mask that pea.foreground_mask left on the device stays
there.

merge_small_object and merge_func of the same file are NOT in this module; they live in utils/merge_objects.py, with relabel of the
validation loop.  Each merge rewrites the image that the next one reads, in id order (a small segment takes the id that is most
frequent in a window around its centroid, and the segments after it see the result), so the merges are sequential by definition; they
run on the device all the same, one workgroup per image walking the small ids in order through an alias table (include/pea_merge.h).
seg_mutex runs on the device as well (utils/seg_mutex.py, include/pea_mws.h).
"""
import numpy as np
import torch

from ..harness.cc import remove_small_components


def _mask_to_device(mask):
    """a numpy mask -> a device tensor of a dtype that pea_cc_label reads (bool and uint8 as they are, other integers as int32)"""
    a = np.ascontiguousarray(mask)
    if a.dtype == np.bool_ or a.dtype == np.uint8 or a.dtype == np.int32:
        pass
    elif a.dtype.kind in "iu":
        if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
            raise ValueError("mask holds values outside int32")
        a = a.astype(np.int32)
    else:
        raise TypeError("mask must hold bool or integers, got %s" % a.dtype)
    return torch.from_numpy(a).cuda()


def remove_samll_object(mask, min_size=25):
    """The mask without its connected components (full connectivity) of fewer than min_size pixels, as 0 / 1.

    mask  [H, W] (the reference's call), [B, H, W] or [B, Z, H, W].  A GPU tensor (bool / uint8 / int32) gives a uint8 GPU tensor and
          nothing is copied to the host; a numpy array is uploaded, filtered on the device and comes back as a uint8 numpy array.
    Pixels of different non-zero values are different objects, as in skimage.morphology.label."""
    as_numpy = isinstance(mask, np.ndarray)
    t = _mask_to_device(mask) if as_numpy else mask
    if not isinstance(t, torch.Tensor):
        raise TypeError("mask must be a numpy array or a torch.Tensor")
    single = t.dim() == 2
    out = remove_small_components(t[None] if single else t, min_size)
    out = out[0] if single else out
    return out.cpu().numpy() if as_numpy else out
