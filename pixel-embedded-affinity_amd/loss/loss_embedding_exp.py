"""Drop-in for the reference's scripts_cvppp/loss/loss_embedding_exp.py (the same file under scripts_bbbc039v1/loss/): same function
names, argument order, defaults and return values.  The loss is taken on u = clamp(cos, 0, 1) with nn.CosineSimilarity's norm
clamp (eps = 1e-6); `affs0_weight` scales the first two offsets; -> (loss, affs) with affs = u, un-masked.  The reference module
has no EMA variant.  One fused forward launch and one backward launch with this package's criteria -- WeightedMSE, MSELoss, BCELoss, WeightedBCE (loss/_activated.py)."""
from ._activated import CLAMP, activated_affs, activated_loss

_EPS = 1e-6


def embedding_loss(embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1):
    """-> (loss, affs [B,K,H,W]) -- reference :16-31"""
    return activated_loss(embedding, None, target, weightmap, mask, criterion, offsets, affs0_weight, _EPS, CLAMP)


def embedding2affs(embedding, offsets):
    """-> affs [B,K,H,W] -- reference :40-47"""
    return activated_affs(embedding, offsets, _EPS, CLAMP)
