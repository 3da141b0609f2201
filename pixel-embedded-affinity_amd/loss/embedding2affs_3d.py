"""3D losses on the ACTIVATED affinity map: drop-in for the reference's scripts_ac3ac4/loss/embedding2affs_3d.py -- the same names
and signatures, every loss returns (loss, affs).  With the criteria of loss/loss.py each is one fused forward launch
(PEA_FLAG_LOSS_ACT, with BCELoss / WeightedBCE also PEA_FLAG_LOSS_BCE), one loss finish, one backward launch and, under the half
shift, one launch over the border slabs (loss/_activated3d.py says how the criteria are routed and why the border needs a call).

Semantics kept from the reference (file:line there):
  * norm1 (:7-40), norm5 (:220-245): u = clamp((cos + 1) / 2, 0, 1); the criterion per channel on the cropped slice; affs0_weight on
    channel 0 (norm1) / channels 0..2 (norm5).  norm1 with fill=True stores the next `shift` slices in the first ones (:36-39), every
    other border is 0.  norm5 ignores `shift` and `fill`: the literal table [1,1,1,2,3,3,3,9,9,4,27,27] (:227)
  * norm1_relu (:42-71), norm5_relu (:274-299): u = clamp(relu(cos), 0, 1) = clamp(cos, 0, 1); `fill` is unused
  * norm2 (:126-147), norm3 (:149-169): ONE criterion call over [B,3,Z,Y,X] with the border terms masked out; affs0_weight and fill
    are unused.  norm3 is norm2 through nn.CosineSimilarity(eps=1e-6): the norms are clamped at 1e-6 instead of 1e-12
  * norm4 (:171-192): the 12-channel table through ONE criterion call, but only channels 0..2 have their border masked (:183-188): on
    channels 3..11 the border terms stay in the loss, a gradient-free constant sum w t^2 (affs is 0 there) that no kernel has a term
    for.  It runs COMPOSED: the raw map through AffinityMap (one forward and one backward launch), activation, border and criterion
    with torch ops
  * embedding_single_offset (:73-97), embedding_single_offset_cos (:99-123): one channel [B,Z,Y,X], 0 on the first `shift` slices.
    The reference's first form takes an embedding that its caller has normalised and sums the products; here both normalise (the
    cosine, eps 1e-12 / 1e-6), which is the same number on unit vectors
"""
import torch

from ..affinity_op import AffinityMap
from ..utils.affinity_ours import NORM5_SHIFTS
from ._activated import CLAMP, HALF_CLAMP, activate
from ._activated3d import cropped_loss, single_offset, spec3d, whole_loss


def embedding_loss_norm1(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, [shift] * 3, affs0_weight, 1, HALF_CLAMP,
                        fill_shift=shift if fill else 0)


def embedding_loss_norm1_relu(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, [shift] * 3, affs0_weight, 1, CLAMP)


def embedding_single_offset(embedding, order, shift=1):
    return single_offset(embedding, order, shift, 1e-12)


def embedding_single_offset_cos(embedding, order, shift=1, dis=None):
    """`dis` is accepted for the signature; the cosine is nn.CosineSimilarity(dim=1, eps=1e-6)'s, the reference's default"""
    return single_offset(embedding, order, shift, 1e-6)


def embedding_loss_norm2(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return whole_loss(embedding, target, weightmap, criterion, [shift] * 3, HALF_CLAMP)


def embedding_loss_norm3(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return whole_loss(embedding, target, weightmap, criterion, [shift] * 3, HALF_CLAMP, eps=1e-6)


def embedding_loss_norm4(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """composed (module docstring): the border terms of channels 3..11 stay in the loss"""
    exists = torch.ones_like(target)
    for i, s in enumerate(NORM5_SHIFTS):
        exists[:, i].narrow(1 + i % 3, 0, s).zero_()
    masked = torch.ones_like(target)
    for i in range(3):
        masked[:, i].narrow(1 + i, 0, 1).zero_()
    affs = activate(AffinityMap.apply(embedding, None, spec3d(NORM5_SHIFTS, None, 1e-12, 0)), HALF_CLAMP) * exists
    return criterion(affs, target * masked, weightmap * masked), affs.detach()


def embedding_loss_norm5(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, NORM5_SHIFTS, affs0_weight, 3, HALF_CLAMP)


def embedding_loss_norm5_relu(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, NORM5_SHIFTS, affs0_weight, 3, CLAMP)
