"""The mutex watershed on the device (include/pea_mws.h: pea_mws_segment) -- what the reference's validation and inference loops do on
the host with elf,

  scripts_cvppp/utils/seg_mutex.py, scripts_bbbc039v1/utils/seg_mutex.py   mutex_watershed(1.0 - affs, offsets, strides, mask=mask)
  scripts_ac3ac4/inference.py -mutex                                        the same on a volume with 12 offsets, strides [1, 10, 10]

as launches of csrc/pea_k_mws.hip.  The result is the partition of the sequential procedure over the edges ordered by (weight, edge id);
the kernels reach it in rounds that each decide many edges at once (the header says why that is exact).  The number of rounds depends
on the data, so with rounds=None the call enqueues a batch of rounds, reads how many edges are undecided (one synchronisation per
batch) and resumes with a doubling batch until none is; with an explicit `rounds` nothing is read back, the call can be captured with
pea.graphed, and completeness is left in stats.  The tie rule among equal weights is this library's, not elf's.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _no_init, _on_device, _ptr, _require_gpu, _stream, stream_workspace

FIRST_BATCH = 32  # rounds of the first batch with rounds=None


class MutexWatershed(object):
    """labels  int32, the spatial shape of x: clusters 1 .. n per image in raster order of their first pixel, 0 where mask is 0
    counts  int32 [B] (0-dim for one image): n
    stats   int32 [B, 8] ([8] for one image): the columns _lib.MWS_STAT_COLUMNS; stats[..., 1] == 0 says the partition is complete"""

    def __init__(self, labels, counts, stats):
        self.labels, self.counts, self.stats = labels, counts, stats

    def __repr__(self):
        return "MutexWatershed(shape=%s)" % (tuple(self.labels.shape),)

    def stat(self, name):
        return self.stats[..., _lib.MWS_STAT_COLUMNS.index(name)]


def _arguments(x, offsets, strides, mask, input, n_attractive, rounds):
    """everything that can be said without a device -> (x5 dense [B, K, Z, Y, X] view, mask or None, descriptor, batched, ndim)"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    offsets = [[int(v) for v in o] for o in offsets]
    if not offsets or len(offsets) > _lib.MWS_MAX_K:
        raise ValueError("1 .. %d offsets are served, got %d" % (_lib.MWS_MAX_K, len(offsets)))
    ndim = len(offsets[0])
    if ndim not in (2, 3) or any(len(o) != ndim for o in offsets):
        raise ValueError("offsets must all have 2 or all have 3 steps, got %r" % (offsets,))
    if x.dim() not in (ndim + 1, ndim + 2):
        dims = "Y, X" if ndim == 2 else "Z, Y, X"
        raise ValueError("x must be [K, %s] or [B, K, %s] for offsets of %d steps, got %s" % (dims, dims, ndim, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise TypeError("x must be float32, got %s" % x.dtype)
    batched = x.dim() == ndim + 2
    if min(x.shape) < 1:
        raise ValueError("x has an empty dimension: %s" % (tuple(x.shape),))
    xb = x.detach() if batched else x.detach()[None]
    if ndim == 2:
        xb = xb[:, :, None]
    B, K, Z, Y, X = (int(v) for v in xb.shape)
    if K != len(offsets):
        raise ValueError("x has %d channels and %d offsets were given" % (K, len(offsets)))
    if K * Z * Y * X >= 2 ** 32 or Z * Y * X >= 2 ** 31:
        raise ValueError("an image of %d channels of %d pixels: edge ids must fit 32 bits" % (K, Z * Y * X))
    na = ndim if n_attractive is None else int(n_attractive)
    if not 1 <= na <= K:
        raise ValueError("n_attractive must lie in 1 .. K = %d, got %r" % (K, n_attractive))
    st = [1] * ndim if strides is None else [int(s) for s in strides]
    if len(st) != ndim or min(st) < 1:
        raise ValueError("strides must be %d integers >= 1, got %r" % (ndim, strides))
    if input not in _lib.MWS_INPUTS:
        raise ValueError("input must be one of %s, got %r" % (sorted(_lib.MWS_INPUTS), input))
    if rounds is not None and not 0 <= int(rounds) <= _lib.MWS_MAX_ROUNDS:
        raise ValueError("rounds must be None or lie in 0 .. %d, got %r" % (_lib.MWS_MAX_ROUNDS, rounds))
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError("mask must be a torch.Tensor")
        if mask.dtype not in (torch.uint8, torch.bool):
            raise TypeError("mask must be uint8 or bool, got %s" % mask.dtype)
        want = tuple(x.shape[:1] if batched else ()) + tuple(x.shape[-ndim:])
        if tuple(mask.shape) != want:
            raise ValueError("mask must have the shape %s of x without its channels, got %s" % (want, tuple(mask.shape)))
    d = _lib.PeaMwsDesc()
    d.B, d.Z, d.Y, d.X, d.K, d.n_attractive = B, Z, Y, X, K, na
    for k, o in enumerate(offsets):
        d.offsets[k][:] = [0] * (3 - ndim) + o
    d.strides[:] = [1] * (3 - ndim) + st
    d.input, d.rounds, d.flags = _lib.MWS_INPUTS[input], 0, 0
    return xb, d, batched, ndim


def mutex_watershed(x, offsets, strides=None, mask=None, input="affs", n_attractive=None, rounds=None):
    """The mutex watershed of a batch of images -> MutexWatershed (labels, counts, stats), all on the device.

    x         float32 [K, Y, X] / [K, Z, Y, X] or with a batch in front, on the GPU (a view that is not dense is copied)
    offsets   K offsets of 2 or 3 steps; channel k joins pixel p and p + offsets[k]
    strides   repulsive edges exist only at pixels whose every coordinate is a multiple of its stride (elf's strides)
    mask      uint8 or bool, the shape of x without its channels: 0 = invalid (label 0, no edges); pea.foreground_mask's output fits
    input     "affs": x is the affinity map that seg_mutex is given; "elf": x is 1 - affs, elf's first argument; "weights": x holds
              the edge weights themselves
    n_attractive  the channels before it attract, the rest repel (default: the number of dimensions, as elf)
    rounds    None: run to completion (a synchronisation per batch of rounds); an integer: enqueue exactly that many rounds and
              return without reading anything back -- stats[..., 1] > 0 then says that the partition is not final yet (it is a
              refinement of the final one)"""
    xb, d, batched, ndim = _arguments(x, offsets, strides, mask, input, n_attractive, rounds)
    _require_gpu(xb, "x")
    if mask is not None:
        _require_gpu(mask, "mask")
        mask = mask.detach()
        mask = mask if mask.is_contiguous() else mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    xb = xb if xb.is_contiguous() else xb.contiguous()
    L = _lib.lib()
    dev = xb.device
    spatial = (d.B, d.Z, d.Y, d.X)
    with _on_device(dev):
        labels = torch.empty(spatial, dtype=torch.int32, device=dev)
        counts = torch.empty((d.B,), dtype=torch.int32, device=dev)
        stats = torch.empty((d.B, _lib.MWS_STATS), dtype=torch.int32, device=dev)
        nb = int(L.pea_mws_workspace_bytes(ctypes.byref(d)))
        work = stream_workspace("mws", dev, nb, _no_init, "pea_mws_segment's workspace")

        def call():
            _lib.check(L.pea_mws_segment(ctypes.byref(d), _ptr(xb), _ptr(mask), _ptr(labels), _ptr(counts), _ptr(stats), _ptr(work), nb,
                                         _stream()), "pea_mws_segment")

        if rounds is not None:
            d.rounds = int(rounds)
            call()
        else:
            cap = d.K * d.Z * d.Y * d.X  # a round that finds an edge decides one: more rounds than edges cannot be needed
            batch, done = FIRST_BATCH, 0
            while True:
                d.rounds = min(batch, _lib.MWS_MAX_ROUNDS)
                call()
                done += d.rounds
                if int(stats[:, 1].max()) == 0:  # the one synchronisation of the batch
                    break
                if done > cap:
                    raise _lib.PeaLibraryError("the mutex watershed is not complete after %d rounds on %d edge slots" % (done, cap))
                d.flags = _lib.MWS_RESUME
                batch *= 2
    labels = labels if ndim == 3 else labels[:, 0]
    if not batched:
        labels, counts, stats = labels[0], counts[0], stats[0]
    return MutexWatershed(labels, counts, stats)
