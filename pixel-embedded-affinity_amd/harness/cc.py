"""Connected-component labelling on the device (include/pea_cc.h: pea_cc_label): label, size filter, mask -- what the reference does on
the host between the argmax mask and the scorers,

  scripts_bbbc039v1/utils/postprocessing.py:43-48   remove_samll_object: skimage.morphology.label, remove_small_objects(min_size=25)
  scripts_bbbc039v1/utils/merge_small.py:106        vigra.analysis.labelVolumeWithBackground
  scripts_bbbc039v1/convert_mask2ins.py:33          skimage.morphology.label

as seven launches of csrc/pea_k_cc.hip, none per component: a tile pass in LDS, a lock-free union across the tile borders, compress and
count, a three-step scan and the write.  No host synchronisation, so the call can be captured with pea.graphed; every number is an exact
integer and does not depend on the order in which workgroups arrive.  Device tensors only.  utils/postprocessing.py carries the reference's
own name for the mask form, remove_samll_object.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _no_init, _on_device, _ptr, _require_gpu, _stream, stream_workspace

_IN_CODE = {torch.bool: _lib.CC_IN_U8, torch.uint8: _lib.CC_IN_U8, torch.int32: _lib.CC_IN_I32}
_INT32_MAX = 2 ** 31 - 1


class ConnectedComponents(object):
    """labels  int32, the shape of the input: 1 .. n_kept in raster order of each component's first pixel, 0 for background and for
               components of fewer than min_size pixels (None where only the mask was asked for)
    counts  int32 [B, 2] = (components found, components kept) per image
    mask    uint8, the shape of the input: labels != 0, or None
    All three are device tensors; nothing is copied to the host."""

    def __init__(self, labels, counts, mask):
        self.labels, self.counts, self.mask = labels, counts, mask

    def __repr__(self):
        return "ConnectedComponents(shape=%s)" % (tuple((self.labels if self.labels is not None else self.mask).shape),)


def _cc_args(x, connectivity, min_size, gpu=True):
    """-> (dense tensor, PEA_CC_IN_*, ndim, connectivity, min_size): shape, dtype and ranges first, then the device"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (3, 4):
        raise ValueError("x must be [B, H, W] or [B, Z, H, W], got %s" % (tuple(x.shape),))
    if x.dtype not in _IN_CODE:
        raise TypeError("x must be bool, uint8 or int32, got %s: convert a label image once with .to(torch.int32)" % x.dtype)
    if min(x.shape) < 1:
        raise ValueError("x has an empty dimension: %s" % (tuple(x.shape),))
    ndim = x.dim() - 1
    conn = ndim if connectivity is None else int(connectivity)
    if not 1 <= conn <= ndim:
        raise ValueError("connectivity must lie in 1 .. %d for a %dD image (skimage's meaning; None = %d, full), got %r" % (ndim, ndim, ndim, connectivity))
    ms = int(min_size)
    if not 0 <= ms <= _INT32_MAX:
        raise ValueError("min_size must lie in 0 .. 2^31 - 1, got %r" % (min_size,))
    pixels = 1
    for v in x.shape[1:]:
        pixels *= int(v)
    if pixels > _INT32_MAX:
        raise ValueError("an image of %d pixels: pea_cc_label serves fewer than 2^31 per image" % pixels)
    if gpu:
        _require_gpu(x, "x")
    code = _IN_CODE[x.dtype]
    x = x.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    return x, code, ndim, conn, ms


def _label(x, code, ndim, conn, ms, want_labels, want_mask):
    """pea_cc_label on a dense device tensor -> (labels or None, counts, mask or None)"""
    d = _lib.PeaCcDesc()
    d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = ndim, int(x.shape[0]), code, conn, ms, 0
    d.dims[:] = [1 if ndim == 2 else int(x.shape[1]), int(x.shape[-2]), int(x.shape[-1])]
    L = _lib.lib()
    dev = x.device
    with _on_device(dev):
        labels = torch.empty(x.shape, dtype=torch.int32, device=dev) if want_labels else None
        mask = torch.empty(x.shape, dtype=torch.uint8, device=dev) if want_mask else None
        counts = torch.empty((d.B, 2), dtype=torch.int32, device=dev)
        nb = int(L.pea_cc_workspace_bytes(ctypes.byref(d)))
        work = stream_workspace("cc", dev, nb, _no_init, "pea_cc_label's workspace")
        _lib.check(L.pea_cc_label(ctypes.byref(d), _ptr(x), _ptr(labels), _ptr(mask), _ptr(counts), _ptr(work), nb, _stream()), "pea_cc_label")
    return labels, counts, mask


def connected_components(x, connectivity=None, min_size=0, mask=False):
    """The connected components of a batch of masks or label images -> ConnectedComponents (labels, counts, mask).

    x             [B, H, W] or [B, Z, H, W] on the GPU, bool / uint8 / int32; a view that is not dense is copied.  Two neighbouring
                  pixels are joined iff their value is not 0 and is the same: on a mask the foreground components, on an int32 label
                  image every id split into its connected pieces (negative ids are ordinary values).  Images of a batch never touch.
    connectivity  skimage's meaning, 1 .. ndim: 2D 1 = 4-, 2 = 8-neighbourhood; 3D 1 = 6, 2 = 18, 3 = 26.  None = full (skimage's default)
    min_size      components of fewer pixels are dropped (0 and 1 drop nothing): skimage's remove_small_objects
    mask          True: also the uint8 mask labels != 0

    The kept components of an image are numbered 1 .. n_kept in raster order of their first pixel; for min_size <= 1 that is the numbering
    of scipy.ndimage.label and skimage.morphology.label.  Per-component sizes are not returned: torch.bincount(labels.flatten()) of one
    image gives them."""
    xc, code, ndim, conn, ms = _cc_args(x, connectivity, min_size)
    labels, counts, m = _label(xc, code, ndim, conn, ms, True, bool(mask))
    return ConnectedComponents(labels, counts, m)


def remove_small_components(mask, min_size, connectivity=None):
    """uint8, the shape of `mask` ([B, H, W] or [B, Z, H, W] on the GPU): the pixels of the components of at least min_size pixels
    (pea_cc_label with mask_out only)"""
    xc, code, ndim, conn, ms = _cc_args(mask, connectivity, min_size)
    return _label(xc, code, ndim, conn, ms, False, True)[2]
