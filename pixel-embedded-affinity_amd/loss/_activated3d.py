"""Shared dispatch of the 3D losses taken on the ACTIVATED affinity map (embedding2affs_3d.py, embedding2affs_3d_l2.py and the norm2
pair of loss_embedding_mse_3d.py): u = clamp((a + 1) / 2, 0, 1), clamp(a, 0, 1) or (a + 1) / 2 instead of the raw cosine a, on the
cropped pairs of an axis-aligned 3D stencil (channel i compares p with p - shifts[i] along axis i % 3 of (z, y, x)).

Two shapes of criterion call exist in the reference and both are one fused forward launch here (PEA_FLAG_LOSS_ACT, include/pea.h):
  * per channel, on the cropped slice (`cropped_loss`): PEA_NORM_CROPPED -- WeightedMSE's normaliser, and torch's mean, over
    [B,1,Z',Y',X'];
  * ONE call over the whole [B,K,Z,Y,X] map with the border terms masked out (`whole_loss`): PEA_NORM_FULL.  A cropped-away pair has
    no term in the kernels, which is what `target * mask`, `weightmap * mask` and affs = 0 there amount to (for the unweighted
    criteria too: (0 - 0)^2 = 0 and BCE(0, 0) = 0).  WeightedMSE divides by B*Z*Y*X (pred.size()[2:], loss/loss.py:113-116): lambda 1;
    torch's means divide by B*K*Z*Y*X: lambda 1 / K.
The criteria are routed as _activated.activated_loss routes them: WeightedMSE, MSELoss, BCELoss and WeightedBCE of loss/loss.py run
fused (the unweighted ones on a ones weight; binary cross-entropy only where the activation has the clamp); any other criterion is
called on a differentiable map -- the raw map through AffinityMap, activation and border with torch ops.

The stored map: the reference builds it from zeros, so a pair that does not exist holds 0 where the kernels store act(0) -- 0.5
under the half shift.  pea_affs_crop_zero (include/pea_crop.h, one launch over the border slabs) restores the reference's value;
under the clamp alone act(0) = 0 and nothing is launched.
"""
import torch

from .. import _lib
from ..affinity_op import AffinityMap, AffinitySpec, FusedAffinityMSE, affinity_infer
from ..utils.affinity_ours import axis_offsets_3d
from ..utils.postproc import affs_crop_zero_, fill_border_relu_
from ._activated import HALF_CLAMP, activate, criterion_kind, ones_weight

HALF = _lib.FLAG_HALF_SHIFT  # (a + 1) / 2 without a clamp: the L2 forms, 1 - |ehat_p - ehat_q|^2 / 4


def spec3d(shifts, lam, eps, act, norm=_lib.NORM_CROPPED):
    return AffinitySpec(3, axis_offsets_3d(shifts), lam, _lib.BORDER_CROP_ZERO, norm, eps, False, act)


def _fused_flags(kind, act):
    """descriptor flags of the fused criterion, or None where it has no fused form (a foreign criterion; BCE without the clamp)"""
    if kind in ('wmse', 'mse'):
        return act | _lib.FLAG_LOSS_ACT
    if kind in ('wbce', 'bce') and (act & _lib.FLAG_CLAMP01):
        return act | _lib.FLAG_LOSS_ACT | _lib.FLAG_LOSS_BCE
    return None


def _border_(affs, shifts, act, fill_shift=0):
    """the reference's border on the stored map, in place: the first `fill_shift` slices of channel c along axis c copied from the
    next ones (fill=True of the norm1 / norm2 forms), else 0 on the pairs that do not exist"""
    if fill_shift:
        return fill_border_relu_(affs, shift=fill_shift, relu=False)
    if act & _lib.FLAG_HALF_SHIFT:  # act(0) = 0.5; under the clamp alone the kernels stored 0 already
        affs_crop_zero_(affs, axis_offsets_3d(shifts))
    return affs


def cropped_loss(embedding, ema_embedding, target, weightmap, criterion, shifts, affs0_weight, first, act, eps=1e-12, fill_shift=0):
    """sum_i lambda_i criterion(u_i on its cropped slice, ..) -> (loss, affs [B,K,Z,Y,X]); lambda = affs0_weight on channels < first"""
    lam = [float(affs0_weight) if i < first else 1.0 for i in range(len(shifts))]
    kind = criterion_kind(criterion)
    flags = _fused_flags(kind, act)
    if flags is not None:
        if kind not in ('wmse', 'wbce') or weightmap is None:
            weightmap = ones_weight(target)
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, None, spec3d(shifts, lam, eps, flags))
        return loss, _border_(affs, shifts, act, fill_shift)
    u = activate(AffinityMap.apply(embedding, ema_embedding, spec3d(shifts, None, eps, 0)), act)
    loss = 0
    for i, s in enumerate(shifts):
        ax = 2 + i % 3
        n = u.shape[ax] - s
        li = criterion(u[:, i:i + 1].narrow(ax, s, n), target[:, i:i + 1].narrow(ax, s, n), weightmap[:, i:i + 1].narrow(ax, s, n))
        loss = loss + li * lam[i]
    return loss, _border_(u.detach().clone(), shifts, act, fill_shift)


def whole_loss(embedding, target, weightmap, criterion, shifts, act, eps=1e-12):
    """criterion(u with 0 on the border, target * mask, weightmap * mask), ONE call over [B,K,Z,Y,X] -> (loss, affs)"""
    K = len(shifts)
    kind = criterion_kind(criterion)
    flags = _fused_flags(kind, act)
    if flags is not None:
        lam = [1.0 if kind == 'wmse' else 1.0 / K] * K
        if kind not in ('wmse', 'wbce') or weightmap is None:
            weightmap = ones_weight(target)
        loss, affs, _ = FusedAffinityMSE.apply(embedding, None, target, weightmap, None, spec3d(shifts, lam, eps, flags, _lib.NORM_FULL))
        return loss, _border_(affs, shifts, act)
    exists = torch.ones_like(target)
    for i, s in enumerate(shifts):
        exists[:, i].narrow(1 + i % 3, 0, s).zero_()
    u = activate(AffinityMap.apply(embedding, None, spec3d(shifts, None, eps, 0)), act) * exists
    return criterion(u, target * exists, weightmap * exists), u.detach()


def single_offset(embedding, order, shift, eps):
    """-> [B,Z,Y,X]: clamp((<ehat(p), ehat(p - shift along axis `order`)> + 1) / 2, 0, 1), 0 on the first `shift` slices"""
    if order not in (0, 1, 2):
        raise NotImplementedError
    o = [0, 0, 0]
    o[order] = -int(shift)
    affs = affinity_infer(embedding, None, AffinitySpec(3, [o], None, _lib.BORDER_CROP_ZERO, _lib.NORM_CROPPED, eps, False, HALF_CLAMP))
    return affs_crop_zero_(affs, [o])[:, 0]
