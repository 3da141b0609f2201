"""Distance-form affinities of a raw, un-normalised embedding on the device (include/pea_dist.h):

  scripts_{cvppp,bbbc039v1,ac3ac4}/utils/emb2affs.py:63-75   K padded copies of the embedding, K subtractions, K norms and a cat
  scripts_ac3ac4/utils/embeddings_ours.py:47-98              per offset a scipy.ndimage.shift of the whole volume on the host

as one launch (pea_dist_affinity) and, under autograd, one more for the vjp (pea_dist_affinity_vjp).  No workspace, no host
synchronisation: the calls can be captured with pea.graphed, and two runs give the same bits.  Device tensors only.
utils/emb2affs.py and utils/embeddings_ours.py carry the reference's own names and signatures.
"""
import ctypes

import torch

from .. import _lib
from ..affinity_op import _DTYPE_CODE, _on_device, _ptr, _require_gpu, _stream

BORDERS = {"replicate": _lib.BORDER_REPLICATE, "zero": _lib.DIST_BORDER_ZERO_VECTOR}


def _offsets3(offsets, ndim):
    """-> a tuple of (oz, oy, ox) integer triples (2D: oz = 0)"""
    offs = [tuple(int(v) for v in o) for o in offsets]
    if not 1 <= len(offs) <= _lib.PEA_MAX_K:
        raise ValueError("between 1 and %d offsets are supported, got %d" % (_lib.PEA_MAX_K, len(offs)))
    if not all(len(o) == ndim for o in offs):
        raise ValueError("Incosistent dimension of offsets and embeddings")  # (the reference's own words, embeddings_ours.py:79)
    lim = 2 ** 31 - 1
    return tuple((0,) * (3 - ndim) + tuple(max(-lim, min(lim, v)) for v in o) for o in offs)


def _args(e, offsets, delta_v, delta_d, border, gpu=True):
    """-> (e [B, D, *spatial] contiguous, the offsets as triples): shapes, dtypes and parameters first, then the device, so that what
    is wrong with a call can be said without a GPU.  Any layout torch can express is taken (a crop, an expanded batch,
    channels_last): what the kernels read is a dense copy of the same values."""
    if not isinstance(e, torch.Tensor):
        raise TypeError("embeddings must be a torch.Tensor")
    if e.dim() not in (4, 5):
        raise ValueError("embeddings must be [B, D, H, W] or [B, D, Z, Y, X], got %s" % (tuple(e.shape),))
    if e.dtype not in _DTYPE_CODE:
        raise TypeError("embeddings must be float32, float16 or bfloat16, got %s" % e.dtype)
    if e.numel() == 0:
        raise ValueError("embeddings is empty: %s" % (tuple(e.shape),))
    if e.shape[1] > _lib.DIST_MAX_D:
        raise ValueError("embeddings of more than %d channels are not supported, got %d" % (_lib.DIST_MAX_D, e.shape[1]))
    if border not in BORDERS:
        raise ValueError("border must be 'replicate' or 'zero', got %r" % (border,))
    dv, dd = float(delta_v), float(delta_d)
    if not (dd > 0 and dd != float("inf")) or not (0 <= dv < float("inf")):
        raise ValueError("delta_d must be finite and > 0 and delta_v finite and >= 0, got delta_v=%r delta_d=%r" % (delta_v, delta_d))
    offs = _offsets3(offsets, e.dim() - 2)
    if gpu:
        _require_gpu(e, "embeddings")
    return (e if e.is_contiguous() else e.contiguous()), offs


def _desc(e, offs, delta_v, delta_d, border, invert):
    d = _lib.PeaDistDesc()
    d.B, d.D, d.K = int(e.shape[0]), int(e.shape[1]), len(offs)
    sp = [int(v) for v in e.shape[2:]]
    d.dims[:] = [1] * (3 - len(sp)) + sp
    for i, o in enumerate(offs):
        d.offsets[i][:] = o
    d.dtype, d.border, d.flags = _DTYPE_CODE[e.dtype], BORDERS[border], (_lib.DIST_INVERT if invert else 0)
    d.delta_v, d.delta_d = float(delta_v), float(delta_d)
    return d


class DistanceAffinities(torch.autograd.Function):
    """affs = f(e, offsets, delta_v, delta_d, border, invert): pea_dist_affinity and, in backward, pea_dist_affinity_vjp.  affs is
    float32 [B, K, *spatial]; the gradient has the embedding's dtype."""

    @staticmethod
    def forward(ctx, e, offsets, delta_v, delta_d, border, invert):
        e_c, offs = _args(e, offsets, delta_v, delta_d, border)
        d = _desc(e_c, offs, delta_v, delta_d, border, invert)
        e_c = e_c.detach()
        with _on_device(e_c.device):
            affs = torch.empty((e_c.shape[0], d.K) + tuple(e_c.shape[2:]), dtype=torch.float32, device=e_c.device)
            _lib.check(_lib.lib().pea_dist_affinity(ctypes.byref(d), _ptr(e_c), _ptr(affs), _stream()), "pea_dist_affinity")
        ctx.desc = d
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(e_c)
        return affs

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        (e_c,) = ctx.saved_tensors
        with _on_device(e_c.device):
            gc = g.to(device=e_c.device, dtype=torch.float32).contiguous()
            de = torch.empty_like(e_c)
            _lib.check(_lib.lib().pea_dist_affinity_vjp(ctypes.byref(ctx.desc), _ptr(e_c), _ptr(gc), None, _ptr(de), _stream()),
                       "pea_dist_affinity_vjp")
        return (de,) + (None,) * 5


def distance_affinities(e, offsets, delta_v=0.0, delta_d=1.5, border="replicate", invert=False):
    """a_i(p) = max((2 delta_d - h) / (2 delta_d), 0)^2, h = d outside the dead zone d <= delta_v, d = |e(p) - e(p + o_i)| on the RAW e.

    e        [B, D, H, W] or [B, D, Z, Y, X], float32 / float16 / bfloat16 on the GPU, D <= 64; differentiable
    offsets  K <= 32 offsets of the spatial rank; any size (a reach beyond an extent is defined under either border)
    border   "replicate": the neighbour index is clamped into the volume (emb2affs.py); "zero": outside the volume the neighbour is
             the zero vector (embeddings_ours.py: scipy.ndimage.shift)
    invert   1 - a (what the mutex watershed is handed)
    -> float32 [B, K, *spatial]"""
    return DistanceAffinities.apply(e, offsets, delta_v, delta_d, border, bool(invert))
