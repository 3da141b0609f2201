"""3D losses on the L2 affinity: drop-in for the reference's scripts_ac3ac4/loss/embedding2affs_3d_l2.py -- the same names and
signatures, every function returns (loss, affs).

The reference's affinity is 1 - |ehat_p - ehat_q|^2 / 4 with ehat = F.normalize(e), NOT clamped (:10-12, 46-48, 94-95).  For unit
vectors that is (1 + cos) / 2: the half shift without the clamp (PEA_FLAG_HALF_SHIFT | PEA_FLAG_LOSS_ACT), which is what runs here.
The caveat of include/pea.h holds: at a voxel with |e| < eps (1e-12) F.normalize yields a non-unit vector and the two forms differ
there; the library computes the cosine form.

  * l21 (:6-32), l25 (:108-130): the criterion per channel on the cropped slice; affs0_weight on channel 0 (l21) / channels 0..2
    (l25); the border of the stored map is 0.  l25 ignores `shift`: the literal table [1,1,1,2,3,3,3,9,9,4,27,27] (:112)
  * l22 (:60-77): ONE criterion call over [B,3,Z,Y,X] with the border terms masked out; affs0_weight is unused
`fill` is unused everywhere, as in the reference.  WeightedMSE and MSELoss run fused; the map is not clamped, so BCELoss /
WeightedBCE (whose argument must lie in [0, 1]) and any other criterion are called on the differentiable map (loss/_activated3d.py).
"""
from ..utils.affinity_ours import NORM5_SHIFTS
from ._activated3d import HALF, cropped_loss, whole_loss


def embedding_loss_l21(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, [shift] * 3, affs0_weight, 1, HALF)


def embedding_loss_l22(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return whole_loss(embedding, target, weightmap, criterion, [shift] * 3, HALF)


def embedding_loss_l25(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    return cropped_loss(embedding, None, target, weightmap, criterion, NORM5_SHIFTS, affs0_weight, 3, HALF)
