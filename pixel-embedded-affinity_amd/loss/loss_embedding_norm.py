"""Drop-in for the reference's scripts_cvppp/loss/loss_embedding_norm.py (the same file under scripts_bbbc039v1/loss/): same function
names, argument order, defaults and return values.  The embeddings go through F.normalize (eps = 1e-12); the loss is taken on
u = clamp((dot + 1) / 2, 0, 1) (mode='cos') or u = clamp(1 - |ehat_s - ehat|^2 / 4, 0, 1) (any other mode).  For unit vectors the
two are the same number, and both modes run the same kernels here; they differ only at a pixel with |e| < 1e-12, where
F.normalize yields a non-unit vector (include/pea.h, PEA_FLAG_LOSS_ACT).  `affs0_weight` scales the first two offsets;
-> (loss, affs) with affs = u, un-masked.  One fused forward launch and one backward launch with this package's criteria -- WeightedMSE, MSELoss, BCELoss, WeightedBCE
(loss/_activated.py)."""
from ._activated import HALF_CLAMP, activated_affs, activated_loss

_EPS = 1e-12


def embedding_loss(embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1, mode='cos'):
    """-> (loss, affs [B,K,H,W]) -- reference :21-36"""
    return activated_loss(embedding, None, target, weightmap, mask, criterion, offsets, affs0_weight, _EPS, HALF_CLAMP)


def embedding2affs(embedding, offsets, mode='cos'):
    """-> affs [B,K,H,W] -- reference :50-58"""
    return activated_affs(embedding, offsets, _EPS, HALF_CLAMP)


def ema_embedding_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1, mode='cos'):
    """-> (loss, affs) with a_i(p) = <ehat(p), ehat_ema(p + o_i)> -- reference :74-90.  Gradients flow into `ema_embedding` only if
    it requires grad."""
    return activated_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight, _EPS, HALF_CLAMP)
