"""The foreground-mask term of the BBBC039V1 step and the validation mask, on the device (include/pea_fgmask.h):

  scripts_bbbc039v1/main.py:289      loss_mask = mask_weight * BCE_loss_func(pred_mask, torch.gt(target_ins[:, 0], 0), weight_rate=[10, 1])
  scripts_bbbc039v1/loss/loss.py:187-194   two .item() calls for the class weights, then nn.CrossEntropyLoss(weight=weight)
  scripts_bbbc039v1/main.py:406-410  softmax -> argmax -> .cpu() -> uint8 -> [92:-92, 4:-4]

as one streaming launch plus a small finish for the loss, one streaming launch for its gradient and one for the mask: no host
synchronisation, so the calls can be captured with pea.graphed; bit-reproducible sums (the integer accumulators of the training
forward).  Device tensors only.  loss/loss.py carries the reference's own name for it, BCE_loss_func.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _DTYPE_CODE, _on_device, _ptr, _require_gpu, _stream, stream_workspace
from .cc import remove_small_components


def _logits_arg(logits, gpu=True):
    """shape and dtype first, then the device (gpu=False: left to the caller): what is wrong with a call can be said without a GPU"""
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch.Tensor")
    if logits.dim() != 4 or logits.shape[1] != 2:
        raise ValueError("the mask logits must be [B, 2, H, W] (the two-channel output of the binary_seg head), got %s" % (tuple(logits.shape),))
    if logits.dtype not in _DTYPE_CODE:
        raise TypeError("the mask logits must be float32, float16 or bfloat16, got %s" % logits.dtype)
    if gpu:
        _require_gpu(logits, "logits")
    return logits if logits.is_contiguous() else logits.contiguous()


_LABEL_CODE = {torch.bool: _lib.FG_LABELS_U8, torch.uint8: _lib.FG_LABELS_U8, torch.int32: _lib.FG_LABELS_I32}


def _labels_arg(labels, logits, name, gpu=True):
    """-> (tensor, PEA_FG_LABELS_*): bool and uint8 are read as they are (a view, no conversion), int32 likewise; nothing else is taken.
    A label view that is not dense (a slice of a packed tensor, an expanded image) is copied.  gpu=False: as in _logits_arg"""
    if not isinstance(labels, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    B, _, H, W = logits.shape
    if tuple(labels.shape) == (B, 1, H, W):
        labels = labels[:, 0]
    if tuple(labels.shape) != (B, H, W):
        raise ValueError("%s has shape %s, expected %s or %s" % (name, tuple(labels.shape), (B, H, W), (B, 1, H, W)))
    if labels.dtype not in _LABEL_CODE:
        raise ValueError("%s must be bool, uint8 or int32 (foreground <=> value > 0), got %s: pass torch.gt(%s, 0), or convert the "
                         "label image once with .to(torch.int32)" % (name, labels.dtype, name))
    if gpu:
        _require_gpu(labels, name)
    if labels.device != logits.device:
        raise RuntimeError("%s is on %s, the logits on %s" % (name, labels.device, logits.device))
    labels = labels.detach()
    code = _LABEL_CODE[labels.dtype]
    if not labels.is_contiguous():
        labels = labels.contiguous()
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8)
    return labels, code


def _desc(logits, code, flags=0):
    d = _lib.PeaFgDesc()
    d.B, d.Y, d.X = int(logits.shape[0]), int(logits.shape[2]), int(logits.shape[3])
    d.logits_dtype, d.labels_type, d.flags = _DTYPE_CODE[logits.dtype], code, flags
    return d


class ForegroundMaskCE(torch.autograd.Function):
    """loss, stats = f(logits, labels, skip_empty): pea_fgmask_loss_fwd and, in backward, pea_fgmask_loss_bwd.  loss is a float32
    scalar, stats float64 [5] = (loss, S0 / n0, S1 / n1, n0, n1); dlogits has the logits' dtype."""

    @staticmethod
    def forward(ctx, logits, labels, skip_empty):
        ctx.set_materialize_grads(False)
        lg = _logits_arg(logits, gpu=False)
        if isinstance(labels, torch.Tensor) and labels.is_cuda:
            _require_gpu(lg, "logits")
        lab, code = _labels_arg(labels, lg, "labels")
        d = _desc(lg, code, _lib.FG_SKIP_EMPTY_CLASS if skip_empty else 0)
        L = _lib.lib()
        dev = lg.device
        with _on_device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            stats = torch.empty(_lib.FG_STATS, dtype=torch.float64, device=dev)
            nb = int(L.pea_fgmask_workspace_bytes())  # one loss state
            work = stream_workspace("fgmask", dev, nb, L.pea_workspace_init, "pea_workspace_init")
            _lib.check(L.pea_fgmask_loss_fwd(ctypes.byref(d), _ptr(lg.detach()), _ptr(lab), _ptr(loss), _ptr(stats), _ptr(work), nb, _stream()),
                       "pea_fgmask_loss_fwd")
        ctx.desc = d
        ctx.save_for_backward(lg, lab, stats)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        if dloss is None or not ctx.needs_input_grad[0]:
            return None, None, None
        lg, lab, stats = ctx.saved_tensors
        with _on_device(lg.device):
            dl = dloss.to(device=lg.device, dtype=torch.float32).contiguous()
            dlogits = torch.empty_like(lg)
            _lib.check(_lib.lib().pea_fgmask_loss_bwd(ctypes.byref(ctx.desc), _ptr(lg), _ptr(lab), _ptr(stats), _ptr(dl), _ptr(dlogits),
                                                      _stream()), "pea_fgmask_loss_bwd")
        return dlogits, None, None


def foreground_mask_loss(logits, labels, skip_empty=False):
    """The class-balanced two-class cross-entropy of the reference's BCE_loss_func -> (loss, stats).

    logits  [B, 2, H, W] float32 / float16 / bfloat16 on the GPU: the binary_seg head's output
    labels  [B, H, W] (or [B, 1, H, W]): bool / uint8 (the reference's torch.gt(target_ins[:, 0], 0), read as it is) or the int32
            instance image the labels-in path already takes -- foreground <=> label > 0
    loss    float32 scalar, differentiable in logits; stats float64 [5] = (loss, mean nll of the background, of the foreground, n0, n1)
    An image batch without foreground or without background gives NaN and an all-NaN gradient, as the reference does (0 / 0);
    skip_empty=True counts the absent class as 0 instead."""
    return ForegroundMaskCE.apply(logits, labels, bool(skip_empty))


def foreground_mask(logits, crop=((0, 0), (0, 0)), min_size=0):
    """uint8 [B, H', W'] = [l1 > l0] on logits[..., top:H - bottom, left:W - right], crop = ((top, bottom), (left, right)): the
    reference's argmax(softmax(pred_mask), dim=1) and its [92:-92, 4:-4] (scripts_bbbc039v1/main.py:406-410) in one launch, left on the
    device.  A tie or a NaN gives 0.  min_size > 0: the mask then loses its connected components (8-neighbourhood) of fewer than
    min_size pixels -- remove_samll_object of main.py:411, pea_cc_label with mask_out only (harness/cc.py); 0 adds no launch."""
    ms = int(min_size)
    if ms < 0:
        raise ValueError("min_size must be >= 0, got %r" % (min_size,))
    lg = _logits_arg(logits).detach()
    (top, bottom), (left, right) = crop
    H, W = int(lg.shape[2]), int(lg.shape[3])
    d = _desc(lg, _lib.FG_LABELS_U8)
    d.origin[:] = [int(top), int(left)]
    d.out_dims[:] = [H - int(top) - int(bottom), W - int(left) - int(right)]
    if min(top, bottom, left, right) < 0 or d.out_dims[0] < 1 or d.out_dims[1] < 1:
        raise ValueError("crop %s leaves nothing of a %d x %d image" % (crop, H, W))
    with _on_device(lg.device):
        out = torch.empty((lg.shape[0], d.out_dims[0], d.out_dims[1]), dtype=torch.uint8, device=lg.device)
        _lib.check(_lib.lib().pea_fgmask_argmax(ctypes.byref(d), _ptr(lg), _ptr(out), _stream()), "pea_fgmask_argmax")
    if ms > 0:
        out = remove_small_components(out, ms)
    return out
