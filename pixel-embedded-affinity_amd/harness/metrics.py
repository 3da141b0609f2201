"""The validation pixel metrics on the affinity map, on the device (include/pea_metrics.h: pea_affs_metrics): what the reference's
drivers log in their validation loops,

  2D  scripts_cvppp/main.py:395-399 (scripts_bbbc039v1/main.py likewise): pred = F.relu(pred), valid_mse(pred * affs_mask, target *
      affs_mask), valid_bce(torch.clamp(pred, 0, 1) * affs_mask, target * affs_mask)  (MSELoss / BCELoss, loss/loss.py:126-140)
  3D  scripts_ac3ac4/main.py:339-351 (inference.py:253-269): whole_mse, np.clip(out, 1e-6, 0.999999), whole_bce, the threshold at
      0.5 and sklearn's f1_score(1 - gt, 1 - out) -- in numpy on the host there

as ONE streaming launch plus a small finish: no host synchronisation (the call can be captured with pea.graphed), bit-reproducible
sums (the integer accumulators of the training forward).  Device tensors only.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _on_device, _ptr, _stream, stream_workspace


class AffinityMetrics(object):
    """The device table [1 + C, 5] (float64; columns mse, bce, tp, fp, fn; row 0 the whole map, row 1 + c channel c) of one
    affinity_metrics call.  Nothing is copied to the host until a value is asked for: .mse / .bce / .tp / .fp / .fn / .f1 are the
    whole map's, .per_channel a dict of per-channel lists.  F1 = 2 tp / (2 tp + fp + fn), 0.0 where the denominator is 0
    (sklearn's zero_division default)."""
    COLUMNS = ("mse", "bce", "tp", "fp", "fn")

    def __init__(self, table):
        self.table = table
        self._host = None

    def _rows(self):
        if self._host is None:
            self._host = self.table.detach().cpu().numpy()
        return self._host

    @staticmethod
    def _f1(tp, fp, fn):
        den = 2 * tp + fp + fn
        return 2.0 * tp / den if den else 0.0

    mse = property(lambda self: float(self._rows()[0, 0]))
    bce = property(lambda self: float(self._rows()[0, 1]))
    tp = property(lambda self: int(self._rows()[0, 2]))
    fp = property(lambda self: int(self._rows()[0, 3]))
    fn = property(lambda self: int(self._rows()[0, 4]))
    f1 = property(lambda self: self._f1(self.tp, self.fp, self.fn))

    @property
    def per_channel(self):
        r = self._rows()[1:]
        d = {"mse": [float(v) for v in r[:, 0]], "bce": [float(v) for v in r[:, 1]]}
        for j, name in ((2, "tp"), (3, "fp"), (4, "fn")):
            d[name] = [int(v) for v in r[:, j]]
        d["f1"] = [self._f1(t, p, n) for t, p, n in zip(d["tp"], d["fp"], d["fn"])]
        return d

    def __repr__(self):
        return "AffinityMetrics(mse=%.6g, bce=%.6g, f1=%.6g)" % (self.mse, self.bce, self.f1)


def affinity_metrics(pred, target, mask=None, *, relu=False, store=False, clip=(0.0, 1.0), weight_map=None, origin=(0, 0, 0),
                     channels=None):
    """MSE, BCE and the F1 counts of an affinity map against its target -> AffinityMetrics.

    pred    [B, CP, H, W] or [B, CP, Z, Y, X], float32, contiguous, on the GPU
    target  [B, C, ...] float32 with C = channels (default: target's own), the region origin .. origin + target's extent of pred
    mask    like target: uint8 / bool or float32, taken as it comes; None = all ones
    relu    pred = F.relu(pred) first (main.py:395); weight_map [PZ, PY, PX] (or [1, ...]): pred / weight_map first (get_results;
            B must be 1); store=True writes that finished value back into ALL of pred (every channel, the whole volume)
    clip    the BCE clip: (0, 1) is torch.clamp of main.py:397, (1e-6, 0.999999) np.clip of scripts_ac3ac4/main.py:345; the bounds are
            rounded to float32 (numpy.float32 values pass unchanged)"""
    for t, name in ((pred, "pred"), (target, "target"), (mask, "mask"), (weight_map, "weight_map")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if not t.is_cuda:
            raise RuntimeError("%s is on %s: affinity_metrics runs on an MI355X only (no CPU fallback)" % (name, t.device))
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() not in (4, 5):
        raise ValueError("pred must be a contiguous float32 [B,CP,H,W] or [B,CP,Z,Y,X] tensor")
    if target.dim() != pred.dim() or target.shape[0] != pred.shape[0]:
        raise ValueError("target %s does not fit pred %s" % (tuple(target.shape), tuple(pred.shape)))
    C = int(target.shape[1] if channels is None else channels)
    if target.shape[1] != C:
        raise ValueError("target has %d channels, expected %d" % (target.shape[1], C))
    target = target.detach()
    if target.dtype != torch.float32:
        target = target.float()
    target = target.contiguous()
    flags = 0
    if mask is not None:
        if tuple(mask.shape) != tuple(target.shape):
            raise ValueError("mask %s does not fit target %s" % (tuple(mask.shape), tuple(target.shape)))
        mask = mask.detach()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        elif mask.is_floating_point():
            mask = mask if mask.dtype == torch.float32 else mask.float()
            flags |= _lib.MET_MASK_F32
        elif mask.dtype != torch.uint8:
            mask = mask.to(torch.uint8)
        mask = mask.contiguous()
    if weight_map is not None:
        weight_map = weight_map.detach()
        if weight_map.dtype != torch.float32 or not weight_map.is_contiguous() or weight_map.numel() != int(np.prod(pred.shape[2:])):
            raise ValueError("weight_map must be a contiguous float32 tensor of pred's volume")
        flags |= _lib.MET_DIVIDE
    if relu:
        flags |= _lib.MET_RELU
    if store:
        flags |= _lib.MET_STORE
    d = _lib.PeaMetricsDesc()
    d.B, d.C, d.CP = int(pred.shape[0]), C, int(pred.shape[1])
    d.dims[:] = [1] * (5 - target.dim()) + [int(v) for v in target.shape[2:]]
    d.pred_dims[:] = [1] * (5 - pred.dim()) + [int(v) for v in pred.shape[2:]]
    org = [int(v) for v in origin]
    d.origin[:] = [0] * (3 - len(org)) + org
    d.flags = flags
    d.clip_lo, d.clip_hi = float(np.float32(clip[0])), float(np.float32(clip[1]))
    L = _lib.lib()
    rc = L.pea_metrics_validate(ctypes.byref(d))
    if rc:
        raise ValueError("invalid metrics descriptor (%s): pred %s, target %s, origin %s, relu=%s, store=%s, clip=%s"
                         % (L.pea_strerror(rc).decode(), tuple(pred.shape), tuple(target.shape), tuple(org), relu, store, tuple(clip)))
    dev = pred.device
    with _on_device(dev):
        out = torch.empty((1 + C, _lib.METRICS_COLS), dtype=torch.float64, device=dev)
        nb = int(L.pea_metrics_workspace_bytes())  # five loss states
        work = stream_workspace("metrics", dev, nb, L.pea_workspace_init, "pea_workspace_init")
        _lib.check(L.pea_affs_metrics(ctypes.byref(d), _ptr(pred), _ptr(weight_map), _ptr(target), _ptr(mask), _ptr(out), _ptr(work), nb,
                                      _stream()), "pea_affs_metrics")
    if store:
        # the kernel writes through data_ptr(): tell autograd (as fill_border_relu_ does)
        torch.autograd.graph.increment_version(pred)
    return AffinityMetrics(out)
