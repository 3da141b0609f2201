"""scripts_ac3ac4/utils/embeddings_ours.py:47-98 (and utils/embeddings.py:78-114, its copy without the dead zone: delta_v = 0) with
the reference's name and signature: one launch on the device (include/pea_dist.h) instead of one scipy.ndimage.shift of the whole
volume per offset.  The border is that shift's (order=0, constant 0): outside the volume the neighbour is the zero vector.
"""
import numpy as np
import torch

from ..harness.dist import distance_affinities


def embeddings_to_affinities(embeddings,
                             offsets=[[-1, 0, 0], [0, -1, 0], [0, 0, -1]],
                             delta_v=0.5,
                             delta_d=1.5,
                             invert=False):
    """ Convert embeddings to affinities: a = max((2 delta_d - dis) / (2 delta_d), 0)^2 with dis = |e(p) - e(p + o)| set to 0
    where it is <= delta_v; invert: 1 - a.

    embeddings  one volume [D, *spatial] (2 or 3 spatial dimensions): a device tensor (float32 / float16 / bfloat16) gives a device
                tensor [K, *spatial] float32; a numpy array is taken to the current device as float32 and a numpy float32 array comes
                back, as the reference returns it"""
    as_numpy = isinstance(embeddings, np.ndarray)
    e = embeddings
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("embeddings_to_affinities runs on an MI355X only (no CPU fallback)")
        e = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).cuda()
    elif not isinstance(e, torch.Tensor):
        raise TypeError("embeddings must be a torch.Tensor or a numpy array")
    ndim = e.dim() - 1
    if not all(len(off) == ndim for off in offsets):
        raise ValueError("Incosistent dimension of offsets and embeddings")
    affs = distance_affinities(e[None], offsets, delta_v=delta_v, delta_d=delta_d, border="zero", invert=invert)[0]
    return affs.cpu().numpy() if as_numpy else affs
