"""Shared dispatch of the 2D losses taken on the ACTIVATED affinity map (loss_embedding.py, loss_embedding_exp.py,
loss_embedding_norm.py): u = clamp((a + 1) / 2, 0, 1) or clamp(a, 0, 1) instead of the raw cosine a.

With this package's criteria (loss/loss.py: WeightedMSE, MSELoss, BCELoss, WeightedBCE -- the four `loss_func` choices of the
reference's drivers) the call is one fused forward launch -- the descriptor carries PEA_FLAG_LOSS_ACT next to the activation bits
(include/pea.h), the kernels' epilogue takes the criterion on u and folds du / da into g -- and one backward launch, the same
backward kernels as the raw-cosine loss.  FusedAffinityMSE carries either criterion: the squared residual, or with
PEA_FLAG_LOSS_BCE the binary cross-entropy (the backward only ever sees g).  Any other criterion gets
`criterion(u * mask, target * mask, weightmap)` per offset on a differentiable map: the raw map through AffinityMap (which has the
vjp), the activation with torch ops.
"""
import torch

from .. import _lib
from ..affinity_op import AffinityMap, AffinitySpec, FusedAffinityMSE, affinity_infer

HALF_CLAMP = _lib.FLAG_HALF_SHIFT | _lib.FLAG_CLAMP01  # clamp((a + 1) / 2, 0, 1)
CLAMP = _lib.FLAG_CLAMP01                              # clamp(a, 0, 1)


def _spec(offsets, lam, eps, act, norm=_lib.NORM_BX):
    return AffinitySpec(2, offsets, lam, _lib.BORDER_CIRCULAR, norm, eps, False, act)


_ONES = {}


def ones_weight(target):
    """the weight map of an unweighted criterion (and of weightmap=None): ones of the target's shape, one tensor per (device, shape).
    The C entry points require `weight`; the kernels read it like any other."""
    key = (target.device, tuple(target.shape))
    w = _ONES.get(key)
    if w is None:
        if len(_ONES) >= 16:
            _ONES.clear()
        w = _ONES[key] = torch.ones(target.shape, dtype=torch.float32, device=target.device)
    return w


def criterion_kind(criterion):
    """'wmse' / 'mse' / 'wbce' / 'bce' for this package's criteria (loss/loss.py), None for any other callable"""
    if getattr(criterion, 'pea_fused', False):
        return 'wmse'
    kind = getattr(criterion, 'pea_criterion', None)
    return kind if kind in ('mse', 'wbce', 'bce') else None


def activate(affs, act):
    """the activation bits of `act` with torch ops (differentiable; torch.clamp's backward is inclusive at both edges, as the kernels')"""
    if act & _lib.FLAG_HALF_SHIFT:
        affs = (affs + 1) / 2
    if act & _lib.FLAG_CLAMP01:
        affs = torch.clamp(affs, 0.0, 1.0)
    return affs


def _foreign_criterion(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, lam, eps, act):
    affs = activate(AffinityMap.apply(embedding, ema_embedding, _spec(offsets, None, eps, 0)), act)
    mask = mask.float()
    loss = torch.zeros((), dtype=affs.dtype, device=affs.device)
    for i in range(len(offsets)):
        loss = loss + criterion(affs[:, i] * mask[:, i], target[:, i] * mask[:, i], weightmap[:, i]) * lam[i]
    return loss, affs.detach()


def activated_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight, eps, act):
    """-> (loss, affs): affs is the activated map, un-masked.  affs0_weight scales the first two offsets, in the self loss too
    (unlike loss_embedding_mse.embedding_loss, which accepts it and never applies it)."""
    lam = [float(affs0_weight) if i < 2 else 1.0 for i in range(len(offsets))]
    kind = criterion_kind(criterion)
    if kind == 'wmse':
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, mask,
                                               _spec(offsets, lam, eps, act | _lib.FLAG_LOSS_ACT))
        return loss, affs
    if kind is not None:
        # torch's criteria take the mean over [B,H,W] (PEA_NORM_FULL); the unweighted ones, and weightmap=None, get a ones weight.
        # Binary cross-entropy needs the clamp (its argument in [0, 1]): every module of this file has it
        flags = act | _lib.FLAG_LOSS_ACT | (_lib.FLAG_LOSS_BCE if kind in ('wbce', 'bce') else 0)
        if kind != 'wbce' or weightmap is None:
            weightmap = ones_weight(target)
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, mask,
                                               _spec(offsets, lam, eps, flags, _lib.NORM_FULL))
        return loss, affs
    return _foreign_criterion(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, lam, eps, act)


def activated_affs(embedding, offsets, eps, act):
    return affinity_infer(embedding, None, _spec(offsets, None, eps, act))
