"""discriminative_loss of the reference (scripts_ac3ac4/loss/loss_discriminative.py:6-60; the 2D copies of scripts_cvppp and
scripts_bbbc039v1 are its background=True and background=False) with its signature, its spelling `gama` and one more keyword.

There: torch.unique per image, a Python loop over the ids, a dozen launches per id.  Here: include/pea_disc.h through
harness/disc.py -- six launches for forward and backward whatever the number of instances.
"""
from ..harness.disc import discriminative_loss_stats


def discriminative_loss(embedding, seg_gt, background=False, delta_v=0.5, delta_d=1.5, alpha=1, beta=1, gama=0.001, num_ids=None):
    """-> the loss (float32 scalar, differentiable in embedding).  embedding [B, D, *spatial] float32 / float16 / bfloat16 on the GPU;
    seg_gt [B, *spatial] or [B, 1, *spatial] of any integer dtype, ids in [0, 4096).
    num_ids=None reads the label range once on the host (one synchronisation: the exact drop-in, ValueError for an id outside
    [0, 4096)); a number promises ids < num_ids, synchronises nothing and lets pea.graphed capture the call (a label outside the range
    then makes the loss NaN; pea.discriminative_loss_stats reports how many there were)."""
    return discriminative_loss_stats(embedding, seg_gt, background, delta_v, delta_d, alpha, beta, gama, num_ids)[0]
