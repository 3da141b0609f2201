"""The discriminative (pull / push) instance loss on the raw embedding, on the device (include/pea_disc.h):

  scripts_ac3ac4/loss/loss_discriminative.py:6-60   per image torch.unique (a sort and a host round trip), a Python loop over the ids,
  scripts_cvppp/, scripts_bbbc039v1/ (2D copies)    per id a mask, a gather, a mean, a norm, a relu and a mean

as three streaming launches and two small per-cluster launches for the forward and one streaming launch for the backward.  With
num_ids given there is no host synchronisation, so the calls can be captured with pea.graphed; every sum is bit-reproducible (integer
accumulators per (image, id)).  Device tensors only.  loss/loss_discriminative.py carries the reference's own name and signature.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _DTYPE_CODE, _labels_int32, _on_device, _ptr, _require_gpu, _stream, stream_workspace


def _args(embedding, seg_gt, num_ids, gpu=True):
    """-> (embedding [B, D, *spatial] contiguous, labels int32 [B, S] contiguous, num_ids): shapes and dtypes first, then the device, so
    that what is wrong with a call can be said without a GPU.  Any layout torch can express is taken (a crop, a strided or expanded
    label view, channels_last): what the kernels read is a dense copy of the same values.  gpu=False leaves the device checks out
    (the normalisation alone, on any tensor)"""
    if not isinstance(embedding, torch.Tensor) or not isinstance(seg_gt, torch.Tensor):
        raise TypeError("embedding and seg_gt must be torch.Tensors")
    if embedding.dim() < 3:
        raise ValueError("embedding must be [B, D, *spatial], got %s" % (tuple(embedding.shape),))
    if embedding.dtype not in _DTYPE_CODE:
        raise TypeError("embedding must be float32, float16 or bfloat16, got %s" % embedding.dtype)
    B, D, spatial = int(embedding.shape[0]), int(embedding.shape[1]), tuple(embedding.shape[2:])
    if D > _lib.DISC_MAX_D:
        raise ValueError("embeddings of more than %d channels are not supported, got %d" % (_lib.DISC_MAX_D, D))
    if tuple(seg_gt.shape) == (B, 1) + spatial:
        seg_gt = seg_gt[:, 0]
    if tuple(seg_gt.shape) != (B,) + spatial:
        raise ValueError("seg_gt has shape %s, expected %s or %s" % (tuple(seg_gt.shape), (B,) + spatial, (B, 1) + spatial))
    if seg_gt.dtype.is_floating_point or seg_gt.dtype.is_complex or seg_gt.dtype == torch.bool:
        raise ValueError("seg_gt must hold integer ids, got %s" % seg_gt.dtype)
    if embedding.numel() == 0:
        raise ValueError("embedding is empty: %s" % (tuple(embedding.shape),))
    if num_ids is not None and not 1 <= int(num_ids) <= _lib.DISC_MAX_IDS:
        raise ValueError("num_ids must be in 1 .. %d, got %r" % (_lib.DISC_MAX_IDS, num_ids))
    if gpu:
        _require_gpu(embedding, "embedding")
        _require_gpu(seg_gt, "seg_gt")
    if seg_gt.device != embedding.device:
        raise RuntimeError("seg_gt is on %s, the embedding on %s" % (seg_gt.device, embedding.device))
    seg_gt = seg_gt.detach()
    if num_ids is None:  # the exact drop-in: ONE host synchronisation for the label range
        lo, hi = (int(v) for v in torch.aminmax(seg_gt))
        if lo < 0 or hi >= _lib.DISC_MAX_IDS:
            raise ValueError("label ids must lie in [0, %d), got %d .. %d: relabel the segmentation first" % (_lib.DISC_MAX_IDS, lo, hi))
        num_ids = hi + 1
    lab = _labels_int32(seg_gt).reshape(B, -1)
    return (embedding if embedding.is_contiguous() else embedding.contiguous()), lab, int(num_ids)


def _desc(e, lab, num_ids, background, need_grad, delta_v, delta_d, alpha, beta, gama):
    d = _lib.PeaDiscDesc()
    d.B, d.D, d.S, d.num_ids = int(e.shape[0]), int(e.shape[1]), int(lab.shape[1]), num_ids
    d.dtype = _DTYPE_CODE[e.dtype]
    d.flags = (_lib.DISC_BACKGROUND if background else 0) | (_lib.DISC_NEED_GRAD if need_grad else 0)
    d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = float(delta_v), float(delta_d), float(alpha), float(beta), float(gama)
    return d


class DiscriminativeLoss(torch.autograd.Function):
    """loss, stats = f(embedding, seg_gt, background, delta_v, delta_d, alpha, beta, gama, num_ids): pea_disc_loss_fwd and, in backward,
    pea_disc_loss_bwd.  loss is a float32 scalar, stats float64 [5 + 4 B] = (loss, var, dist, reg, n_bad, then var_b, dist_b, reg_b, C_b
    per image); the gradient has the embedding's dtype."""

    @staticmethod
    def forward(ctx, embedding, seg_gt, background, delta_v, delta_d, alpha, beta, gama, num_ids):
        ctx.set_materialize_grads(False)
        e, lab, num_ids = _args(embedding, seg_gt, num_ids)
        need_grad = bool(ctx.needs_input_grad[0])
        d = _desc(e, lab, num_ids, background, need_grad, delta_v, delta_d, alpha, beta, gama)
        L = _lib.lib()
        _lib.check(L.pea_disc_validate(ctypes.byref(d)), "pea_disc_validate")
        dev = e.device
        with _on_device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            stats = torch.empty(_lib.DISC_STATS + 4 * d.B, dtype=torch.float64, device=dev)
            saved = torch.empty(int(L.pea_disc_context_bytes(ctypes.byref(d))) // 8, dtype=torch.float64, device=dev)
            nb = int(L.pea_disc_workspace_bytes(ctypes.byref(d)))
            # (every call leaves the tables all zero but for the magic word: ready for ANY descriptor that fits)
            work = stream_workspace("disc", dev, nb, L.pea_disc_workspace_init, "pea_disc_workspace_init")
            _lib.check(L.pea_disc_loss_fwd(ctypes.byref(d), _ptr(e.detach()), _ptr(lab), _ptr(loss), _ptr(stats), _ptr(saved), _ptr(work), nb,
                                           _stream()), "pea_disc_loss_fwd")
        ctx.desc = d
        ctx.shape = embedding.shape
        if need_grad:
            ctx.save_for_backward(e, lab, saved)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        none = (None,) * 9
        if dloss is None or not ctx.needs_input_grad[0]:
            return none
        e, lab, saved = ctx.saved_tensors
        with _on_device(e.device):
            dl = dloss.to(device=e.device, dtype=torch.float32).contiguous()
            de = torch.empty_like(e)
            _lib.check(_lib.lib().pea_disc_loss_bwd(ctypes.byref(ctx.desc), _ptr(e), _ptr(lab), _ptr(saved), _ptr(dl), _ptr(de), _stream()),
                       "pea_disc_loss_bwd")
        return (de.view(ctx.shape),) + none[1:]


def discriminative_loss_stats(embedding, seg_gt, background=False, delta_v=0.5, delta_d=1.5, alpha=1, beta=1, gama=0.001, num_ids=None):
    """The reference's discriminative_loss -> (loss, stats).

    embedding  [B, D, *spatial] float32 / float16 / bfloat16 on the GPU, D <= 64
    seg_gt     [B, *spatial] or [B, 1, *spatial], any integer dtype; ids in [0, 4096).  background=False drops id 0 (the BBBC and 3D
               default), True keeps it as an instance (the CVPPP copy)
    num_ids    None: the label range is read once on the host (one synchronisation) and a ValueError names an id outside [0, 4096).
               A number: every id must be < num_ids, nothing is synchronised and the call can be captured with pea.graphed; stats[4]
               then counts the labels outside [0, num_ids), and if there are any the loss is NaN
    loss       float32 scalar, differentiable in embedding; stats float64 [5 + 4 B] = (loss, var, dist, reg, n_bad, then var_b, dist_b,
               reg_b, C_b per image), var / dist / reg the batch means without alpha / beta / gama"""
    return DiscriminativeLoss.apply(embedding, seg_gt, bool(background), delta_v, delta_d, alpha, beta, gama, num_ids)
