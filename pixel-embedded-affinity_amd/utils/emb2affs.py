"""scripts_{cvppp,bbbc039v1,ac3ac4}/utils/emb2affs.py with the reference's names and signatures, on the device.

  embeddings_to_affinities(embeddings, offsets, delta=1.5)   :63-75   one launch (include/pea_dist.h) instead of K padded copies, K
                                                                      subtractions, K norms and a cat; differentiable (a second
                                                                      launch for the vjp)
  invert_offsets(offsets)                                    :59-60
  segmentation_to_affinities(segmentation, offsets)          :78-95   composed in torch: the library's target generation
                                                                      (utils/targets.py) crops at the border, this form clamps

The border is shift_tensor's (:6-56): replication padding, i.e. the neighbour index p + o is clamped into the volume.
"""
import torch

from ..harness.dist import distance_affinities


def invert_offsets(offsets):
    return [[-off for off in offset] for offset in offsets]


def embeddings_to_affinities(embeddings, offsets, delta=1.5):
    """ Transform embeddings to affinities: max((2 delta - |e(p) - e(p + o)|) / (2 delta), 0)^2.
    embeddings [B, D, H, W] or [B, D, Z, Y, X] on the GPU (float32 / float16 / bfloat16) -> float32 [B, K, *spatial]."""
    return distance_affinities(embeddings, offsets, delta_v=0.0, delta_d=delta, border="replicate", invert=False)


def segmentation_to_affinities(segmentation, offsets):
    """ Transform segmentation to affinities: 1 where p and the (clamped) neighbour p + o hold the same id, else 0.
    segmentation [B, 1, H, W] or [B, 1, Z, Y, X] -> float32 [B, K, *spatial]."""
    assert segmentation.shape[1] == 1
    ndim = segmentation.dim() - 2
    assert ndim in (2, 3)
    seg = segmentation.float()
    shifted = []
    for off in offsets:
        assert len(off) == ndim
        s = seg
        for ax, o in enumerate(off):
            n = seg.shape[2 + ax]
            idx = torch.clamp(torch.arange(n, device=seg.device) + int(o), 0, n - 1)
            s = s.index_select(2 + ax, idx)
        shifted.append(s)
    return (segmentation - torch.cat(shifted, dim=1)).eq_(0.)
