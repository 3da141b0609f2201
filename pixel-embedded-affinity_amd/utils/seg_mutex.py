"""The reference's utils/seg_mutex.py (scripts_cvppp/, scripts_bbbc039v1/) under its own name, and elf's mutex_watershed under its
name for the call site of scripts_ac3ac4/inference.py, both on the device (harness/mws.py, include/pea_mws.h):

    def seg_mutex(affs, offsets=[[-1,0],[0,-1]], strides=[1,1], randomize_strides=False, mask=None):
        return mutex_watershed(1.0 - affs, offsets, strides, randomize_strides=randomize_strides, mask=mask)

A tensor on the GPU gives an int32 tensor on the GPU (one synchronisation per batch of rounds, nothing else visits the host); a numpy
array is uploaded, segmented on the device and comes back as a uint64 numpy array, elf's dtype.  Ids are 1 .. n in raster order of the
clusters' first pixels and 0 where mask is 0 (elf numbers from 1 in the same way after its relabelling).  Among EQUAL weights the
order is by edge id, which elf leaves unspecified: on maps with ties the partition can differ from elf's by the ties only.
randomize_strides=True draws the repulsive edges at random and is not served.
"""
import numpy as np
import torch

from ..harness.mws import mutex_watershed as _mutex_watershed

__all__ = ["seg_mutex", "mutex_watershed"]


def _run(x, offsets, strides, randomize_strides, mask, input):
    if randomize_strides:
        raise NotImplementedError("randomize_strides=True (repulsive edges drawn at random) is not served on the device")
    as_numpy = isinstance(x, np.ndarray)
    if as_numpy:
        if not np.issubdtype(x.dtype, np.floating):
            raise TypeError("the affinities must hold floats, got %s" % x.dtype)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        if len(offsets) and t.dim() != len(offsets[0]) + 1:
            raise ValueError("affs must be [K, Y, X] or [K, Z, Y, X] for its offsets, got %s" % (tuple(t.shape),))
        if not torch.cuda.is_available():
            raise RuntimeError("the mutex watershed runs on an MI355X only (no CPU fallback), and no GPU is visible")
        t, m = t.cuda(), (None if m is None else m.cuda())
    else:
        t, m = x, mask
        if isinstance(t, torch.Tensor) and t.is_floating_point() and t.dtype != torch.float32:
            t = t.to(torch.float32)
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(np.ascontiguousarray(m != 0))
            m = m.to(t.device) if isinstance(t, torch.Tensor) else m
    labels = _mutex_watershed(t, offsets, strides, m, input=input).labels
    return labels.cpu().numpy().astype(np.uint64) if as_numpy else labels


def seg_mutex(affs, offsets=[[-1, 0], [0, -1]], strides=[1, 1], randomize_strides=False, mask=None):
    """the reference's seg_mutex: the mutex watershed of the affinity map affs [K, Y, X] (or [K, Z, Y, X]); the first ndim channels
    attract, the others repel on the stride lattice"""
    return _run(affs, offsets, strides, randomize_strides, mask, "affs")


def mutex_watershed(affs, offsets, strides, randomize_strides=False, mask=None):
    """elf.segmentation.mutex_watershed.mutex_watershed under its name and argument order: `affs` is what elf is handed, 1 - affinities
    (the AC3/AC4 call site passes `1 - affs`), which elf inverts back on the first ndim channels"""
    return _run(affs, offsets, strides, randomize_strides, mask, "elf")
