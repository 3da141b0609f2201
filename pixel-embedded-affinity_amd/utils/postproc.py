"""Caller-side epilogues on the affinity map that the reference applies right after the loss call.

  * fill_border_relu_  scripts_ac3ac4/main.py:233-237, 296-300 and scripts_ac3ac4/inference.py:160-164
                       (first slice(s) of channel c along axis c copied from the next ones, then F.relu)
  * relu_              scripts_cvppp/main.py:312,395; scripts_cvppp/inference.py:193  (F.relu(pred))
Both run in place through pea_fill_border_relu (one launch, no temporaries); device tensors only.
  * affs_crop_zero_    the border of the reference's 3D forms on the activated map (scripts_ac3ac4/loss/embedding2affs_3d.py:31-34,
                       89-96: the map starts as zeros / the first slices are set to 0): 0 on the pairs that do not exist, in place
                       through pea_affs_crop_zero (include/pea_crop.h: one launch over the border slabs)
"""
import ctypes

import torch

from .. import _lib


def fill_border_relu_(pred, shift=1, relu=True):
    """in place on pred [B,K,Z,Y,X] (f32, contiguous, on the GPU); returns pred"""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError("fill_border_relu_ runs on an MI355X tensor only (no CPU fallback)")
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        raise ValueError("pred must be a contiguous float32 tensor")
    if pred.dim() == 4:
        B, K, Z, Y, X = pred.shape[0], pred.shape[1], 1, pred.shape[2], pred.shape[3]
        if shift:
            raise ValueError("border fill is the 3D callers' epilogue: pass shift=0 for [B,K,H,W]")
    elif pred.dim() == 5:
        B, K, Z, Y, X = pred.shape
    else:
        raise ValueError("pred must be [B,K,H,W] or [B,K,Z,Y,X], got %s" % (tuple(pred.shape),))
    with torch.cuda.device(pred.device):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().pea_fill_border_relu(ctypes.c_void_p(pred.data_ptr()), B, K, Z, Y, X, int(shift),
                                                   1 if relu else 0, st), "pea_fill_border_relu")
    # the kernel writes through data_ptr(): tell autograd, so that a map saved for a backward (the raw cosines of the
    # projection-first backward, affinity_op.FusedAffinityMSE) raises "modified by an inplace operation" instead of miscomputing
    torch.autograd.graph.increment_version(pred)
    return pred


def crop_desc(shape, offsets):
    """the PeaDesc pea_affs_crop_zero reads for a map of `shape` [B,K,Z,Y,X] (or [B,K,H,W]) and K offsets (dz, dy, dx) or (dy, dx):
    B, K, dims, offsets and the CROP_ZERO border; every other field a valid default.  Host only."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (4, 5):
        raise ValueError("affs must be [B,K,H,W] or [B,K,Z,Y,X], got %s" % (shape,))
    if len(offsets) != shape[1]:
        raise ValueError("%d offsets for %d channels" % (len(offsets), shape[1]))
    d = _lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = _lib.PEA_ABI_VERSION, len(shape) - 2, shape[0], 1, shape[1]
    d.dims[:] = [1] * (5 - len(shape)) + list(shape[2:])
    d.border, d.dtype, d.norm, d.flags, d.eps = _lib.BORDER_CROP_ZERO, _lib.F32, _lib.NORM_CROPPED, 0, 1e-12
    for i, o in enumerate(offsets):
        d.offsets[i][:] = [0] * (3 - len(o)) + [int(v) for v in o]
        d.lam[i] = 1.0
    return d


_CROP_DESC = {}


def affs_crop_zero_(affs, offsets):
    """in place on affs [B,K,Z,Y,X] or [B,K,H,W] (f32, contiguous, on the GPU): +0.0 at every element whose pair (p, p + offsets[k])
    does not exist under the cropped border, nothing else touched; returns affs.  One launch over the border slabs
    (include/pea_crop.h) -- what the reference's 3D forms on the activated map hold there, where the kernels store act(0)."""
    if not isinstance(affs, torch.Tensor) or not affs.is_cuda:
        raise RuntimeError("affs_crop_zero_ runs on an MI355X tensor only (no CPU fallback)")
    if affs.dtype != torch.float32 or not affs.is_contiguous():
        raise ValueError("affs must be a contiguous float32 tensor")
    key = (tuple(affs.shape), tuple(tuple(int(v) for v in o) for o in offsets))
    d = _CROP_DESC.get(key)
    if d is None:
        if len(_CROP_DESC) > 64:
            _CROP_DESC.clear()
        d = _CROP_DESC[key] = crop_desc(affs.shape, offsets)
    with torch.cuda.device(affs.device):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().pea_affs_crop_zero(ctypes.byref(d), ctypes.c_void_p(affs.data_ptr()), st), "pea_affs_crop_zero")
    torch.autograd.graph.increment_version(affs)  # (as fill_border_relu_)
    return affs


def relu_(pred):
    """F.relu(pred) in place"""
    return fill_border_relu_(pred, shift=0, relu=True)
