"""The criteria of the reference's training drivers, with its signatures (loss/loss.py:106-152 in all three script trees; chosen by
`loss_func` at scripts_cvppp/main.py:182-189): WeightedMSE, MSELoss, BCELoss, WeightedBCE.

When an instance of WeightedMSE is handed to embedding_loss & co. as `criterion`, the whole
normalise -> K-offset dot -> mask -> weighted MSE chain runs fused in the HIP kernels and this
module's forward is never called.  Called directly (on any pred/target/weight) it evaluates the
same formula with torch ops, including the reference's normaliser
`prod(pred.size()[2:]) * pred.size(0)` -- for a [B,H,W] prediction that is B*W, not B*H*W.

The other three say which criterion they are through `pea_criterion`; the single-loss functions that have a fused form for it
(loss/_activated.py; "mse" also in loss_embedding_mse.py and loss_embedding_mse_3d.py) then run fused as well, and everything else calls
the module.  They do NOT carry `pea_fused`: the loss sections, head_embedding_loss and the multi / labels paths key on that attribute
and fuse WeightedMSE only.

BCE_loss_func (loss/loss.py:187-194 of scripts_bbbc039v1) is the foreground-mask loss on the binary_seg logits: a function, as there.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


class WeightedMSE(nn.Module):
    """Weighted mean-squared error."""

    pea_fused = True  # tells the affinity ops they may take the fused path
    pea_criterion = "wmse"

    def __init__(self):
        super().__init__()

    @staticmethod
    def norm_term(pred):
        n = pred.size(0)
        for s in pred.size()[2:]:
            n *= s
        return float(n)

    def forward(self, pred, target, weight=None):
        sq = (pred - target) ** 2
        if weight is not None:
            sq = weight * sq
        return torch.sum(sq) / self.norm_term(pred)


class MSELoss(nn.Module):
    """nn.MSELoss with the criteria's call signature; `weight` is accepted and ignored (loss/loss.py:126-132)."""

    pea_criterion = "mse"

    def __init__(self):
        super().__init__()
        self.criterion = nn.MSELoss()

    def forward(self, pred, target, weight=None):
        return self.criterion(pred, target)


class BCELoss(nn.Module):
    """nn.BCELoss with the criteria's call signature; `weight` is accepted and ignored (loss/loss.py:134-140)."""

    pea_criterion = "bce"

    def __init__(self):
        super().__init__()
        self.criterion = nn.BCELoss()

    def forward(self, pred, target, weight=None):
        return self.criterion(pred, target)


class WeightedBCE(nn.Module):
    """Weighted binary cross-entropy (loss/loss.py:142-152)."""

    pea_criterion = "wbce"

    def __init__(self, size_average=True, reduce=True):
        super().__init__()
        self.size_average = size_average
        self.reduce = reduce

    def forward(self, pred, target, weight=None):
        return F.binary_cross_entropy(pred, target, weight)


def BCE_loss_func(output, target, weight_rate=[1, 1]):
    """The foreground-mask loss of the BBBC039V1 step with the reference's name and signature (scripts_bbbc039v1/loss/loss.py:187-194;
    called at scripts_bbbc039v1/main.py:289 and :385): nn.CrossEntropyLoss on the two-channel mask logits with the class weights
    (count of foreground, count of background) -- there after two .item() round trips, here one forward and one backward launch with
    no host synchronisation (include/pea_fgmask.h), one autograd node.

    output  [B, 2, H, W] float32 / float16 / bfloat16 on the GPU
    target  [B, H, W] or [B, 1, H, W]: bool or uint8 (read as it is) or int32, foreground <=> value > 0 -- for the reference's 0 / 1
            targets the same classes; any other dtype raises ValueError
    `weight_rate` is accepted and ignored, as in the reference.  A batch without foreground or without background gives NaN, as
    there; pea.foreground_mask_loss(..., skip_empty=True) is the form that does not."""
    from ..harness.fgmask import foreground_mask_loss
    return foreground_mask_loss(output, target)[0]
