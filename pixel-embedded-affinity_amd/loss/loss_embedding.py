"""Drop-in for the reference's scripts_cvppp/loss/loss_embedding.py (the same file under scripts_bbbc039v1/loss/): same function
names, argument order, defaults and return values.  The loss is taken on u = clamp((cos + 1) / 2, 0, 1) with
nn.CosineSimilarity's norm clamp (eps = 1e-6); `affs0_weight` scales the first two offsets; -> (loss, affs) with affs = u,
un-masked.  One fused forward launch and one backward launch with this package's criteria -- WeightedMSE, MSELoss, BCELoss, WeightedBCE (loss/_activated.py)."""
from ._activated import HALF_CLAMP, activated_affs, activated_loss

_EPS = 1e-6


def embedding_loss(embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1):
    """-> (loss, affs [B,K,H,W]) -- reference :16-31"""
    return activated_loss(embedding, None, target, weightmap, mask, criterion, offsets, affs0_weight, _EPS, HALF_CLAMP)


def embedding2affs(embedding, offsets):
    """-> affs [B,K,H,W] -- reference :40-47"""
    return activated_affs(embedding, offsets, _EPS, HALF_CLAMP)


def ema_embedding_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1):
    """-> (loss, affs) with a_i(p) = cos(e(p), ema(p + o_i)) -- reference :58-73.  Gradients flow into `ema_embedding` only if it
    requires grad."""
    return activated_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight, _EPS, HALF_CLAMP)
