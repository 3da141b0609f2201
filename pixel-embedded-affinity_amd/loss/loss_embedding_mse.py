"""2D embedding -> affinity losses: drop-in for the reference's scripts_cvppp/loss/loss_embedding_mse.py
(byte-identical copy in scripts_bbbc039v1/loss/): same function names, argument order, defaults and
return values; the body is one fused HIP forward launch and one backward launch instead of a Python
loop of K torch.roll / mul / sum / criterion / .item() steps.

Semantics kept from the reference (file:line there):
  * circular wrap of the stencil (torch.roll, :8,:50,:69); wrapped values are returned un-masked in `affs` (:46)
  * `affs0_weight` is accepted but NOT applied by embedding_loss (:26-39); ema_embedding_loss applies it
    to the first two offsets (:90-93)
  * mode != 'ours' selects nn.CosineSimilarity(dim=1, eps=1e-6) on the un-normalised embedding (:11-13,:19-20),
    i.e. the same cosine with the norm clamp at 1e-6 instead of F.normalize's 1e-12
  * the criterion is a parameter: with this package's WeightedMSE the loss is fused into the kernel
    (normaliser B*W, loss.py:113-115); any other callable gets `criterion(affs*mask, target*mask, weightmap)`
    per offset on a differentiable affinity map, exactly like the reference
  * `all_loss` is a list of K floats; here it is filled lazily from a device tensor (no K host syncs)
  * `mask` is the 0 / 1 map gen_affs_ours produces, or any real-valued map: the reference multiplies by mask.float() (:21).  The
    fused path reads a float32 mask as it is (fractional values are honoured; other floating dtypes are converted once with .float())
    and a bool / uint8 mask as one byte per pixel
"""
import torch

from .. import _lib
from ..affinity_op import (AffinityMap, activation_flags, AffinitySpec, FusedAffinityMSE, LabelsAffinityMSE, LabelsStepUnsupported, LossList,
                           MultiAffinityMSE, MultiLabelsAffinityMSE, MultiLabelsUnsupported, MultiUnsupported, affinity_infer, label_sources,
                           materialise_labels)
from ._activated import ones_weight


def _eps(mode):
    return 1e-12 if mode == 'ours' else 1e-6


def _spec(offsets, lam, mode, relu=False, act=0, norm=_lib.NORM_BX):
    return AffinitySpec(2, offsets, lam, _lib.BORDER_CIRCULAR, norm, _eps(mode), relu, act)


def _fused(criterion):
    return getattr(criterion, 'pea_fused', False)


def _plain_mse(criterion):
    """this package's MSELoss (nn.MSELoss, the weight map ignored): the fused squared residual with a ones weight and torch's mean
    over [B,H,W] (PEA_NORM_FULL).  Single losses only: the multi / labels paths key on pea_fused"""
    return not _fused(criterion) and getattr(criterion, 'pea_criterion', None) == 'mse'


def _foreign_criterion(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, lam, mode):
    affs = AffinityMap.apply(embedding, ema_embedding, _spec(offsets, None, mode))
    mask = mask.float()
    loss = torch.zeros((), dtype=affs.dtype, device=affs.device)
    parts = []
    for i in range(len(offsets)):
        li = criterion(affs[:, i] * mask[:, i], target[:, i] * mask[:, i], weightmap[:, i])
        loss = loss + li * lam[i]
        parts.append(li.detach())
    return loss, affs.detach(), torch.stack(parts)


def embedding_loss(embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1, mode='ours'):
    """-> (loss, affs [B,K,H,W], all_loss list[K]) -- reference :18-47"""
    lam = [1.0] * len(offsets)  # the reference computes affs0_weight_factor but never applies it
    if _fused(criterion):
        loss, affs, parts = FusedAffinityMSE.apply(embedding, None, target, weightmap, mask, _spec(offsets, lam, mode))
    elif _plain_mse(criterion):
        loss, affs, parts = FusedAffinityMSE.apply(embedding, None, target, ones_weight(target), mask,
                                                   _spec(offsets, lam, mode, norm=_lib.NORM_FULL))
    else:
        loss, affs, parts = _foreign_criterion(embedding, None, target, weightmap, mask, criterion, offsets, lam, mode)
    return loss, affs, LossList(parts)


def embedding_loss_multi(embeddings, targets, weightmaps, masks, criterion, offsets_list, affs0_weight=1, mode='ours', need_affs=False):
    """[embedding_loss(embeddings[j], targets[j], weightmaps[j], masks[j], criterion, offsets_list[j], affs0_weight, mode) for j]
    -> a list of (loss, affs, all_loss) -- the four deep-supervision calls of scripts_cvppp/main.py:284-287 (and of the validation
    loop, inference.py:185-188) -- as ONE forward, one loss finish and one backward launch where the fused criterion is used and
    the table is in the fused set of include/pea_multi.h (up to four losses; float32, float16 or bfloat16 embeddings, all of ONE dtype;
    D = 16 / 32, at most 12 offsets: 16-bit embeddings get their gradients in their own dtype, rounded once from the f32 result).
    A 16-bit table of more than affinity_op.MULTI16_MAX_TILES tiles of 256 pixels runs the single calls: measured with bf16 at the
    CVPPP shapes, the one launch wins at B = 2 (772 tiles) and loses 8 % of the section at B = 8 (3088 tiles, profiles/multi16_ab.json);
    anything else, and any other criterion, takes the single calls.  need_affs=False (what those callers want: they throw the small
    maps away): affs is None and, on the fused path, never written."""
    n = len(embeddings)
    if not (len(targets) == len(weightmaps) == len(masks) == len(offsets_list) == n):
        raise ValueError("one target, weightmap, mask and offset list per embedding")
    if _fused(criterion):
        specs = [_spec(offs, [1.0] * len(offs), mode) for offs in offsets_list]
        try:
            out = MultiAffinityMSE.apply(specs, list(zip(targets, weightmaps, masks)), bool(need_affs), *embeddings)
            return [(out[j], out[n + j] if need_affs else None, LossList(out[2 * n + j])) for j in range(n)]
        except MultiUnsupported:
            pass
    out = [embedding_loss(e, t, w, m, criterion, offs, affs0_weight=affs0_weight, mode=mode)
           for e, t, w, m, offs in zip(embeddings, targets, weightmaps, masks, offsets_list)]
    return [(l, a if need_affs else None, parts) for l, a, parts in out]


def embedding2affs(embedding, offsets, mode='ours', activation=None):
    """-> affs [B,K,H,W] -- reference :58-66.  activation (beyond the reference's signature): the statement the caller applies
    to the map next, fused into its store -- 'relu' (F.relu(pred), inference.py:193), 'mutex' (1 - relu(a): the map
    elf.mutex_watershed is handed, utils/seg_mutex.py:4-5), 'half' ((a + 1) / 2 = the L2 affinity 1 - d^2 / 4 of unit vectors),
    'half_clamp' (clamp((a + 1) / 2, 0, 1): the embedding2affs of scripts_cvppp/loss/loss_embedding.py:33-46, with mode='cos')."""
    return affinity_infer(embedding, None, _spec(offsets, None, mode, act=activation_flags(activation)))


def ema_embedding_loss(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, affs0_weight=1, mode='ours'):
    """-> (loss, affs) with a_i(p) = <ehat(p), ehat_ema(p+o_i)> -- reference :79-95.
    Gradients flow into `ema_embedding` only if it requires grad (the shipped configs detach it,
    scripts_cvppp/data/data_consistency.py:36)."""
    lam = [float(affs0_weight) if i < 2 else 1.0 for i in range(len(offsets))]
    if _fused(criterion):
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, mask, _spec(offsets, lam, mode))
    elif _plain_mse(criterion):
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, ones_weight(target), mask,
                                               _spec(offsets, lam, mode, norm=_lib.NORM_FULL))
    else:
        loss, affs, _ = _foreign_criterion(embedding, ema_embedding, target, weightmap, mask, criterion, offsets, lam, mode)
    return loss, affs


# ---- the same losses straight from the label image (no target / weightmap / mask tensors) ----
_FLAGS_2D = _lib.TGT_PADDING | _lib.TGT_MASK_INSIDE  # gen_affs_ours(ignore=False, padding=True) + its mask, the shipped provider


def _from_labels(embedding, ema_embedding, labels, criterion, offsets, lam, mode, need_affs=True):
    if not _fused(criterion):
        raise NotImplementedError("the labels-in step fuses WeightedMSE; for another criterion use gen_targets + embedding_loss")
    try:
        return LabelsAffinityMSE.apply(embedding, ema_embedding, labels, _spec(offsets, lam, mode), _FLAGS_2D, need_affs)
    except LabelsStepUnsupported:  # e.g. the coarsest deep-supervision scales: targets on the GPU, then the tensor path
        from ..utils.targets import gen_targets
        t, m, w = gen_targets(labels, offsets, padding=True)
        return FusedAffinityMSE.apply(embedding, ema_embedding, t, w, m, _spec(offsets, lam, mode))


def embedding_loss_from_labels(embedding, labels, criterion, offsets, affs0_weight=1, mode='ours', need_affs=True):
    """embedding_loss(embedding, *gen_targets(labels, offsets, padding=True), criterion, offsets) without the three
    [B,K,H,W] tensors: -> (loss, affs, all_loss).  labels: int tensor [B,H,W] on the GPU.  need_affs=False skips the
    affinity-map output (an empty tensor is returned) for the calls whose map the training loop throws away."""
    loss, affs, parts = _from_labels(embedding, None, labels, criterion, offsets, [1.0] * len(offsets), mode, need_affs)
    return loss, affs, LossList(parts)


def ema_embedding_loss_from_labels(embedding, ema_embedding, labels, criterion, offsets, affs0_weight=1, mode='ours', need_affs=True):
    """ema_embedding_loss from the label image (the EMA operand must be detached, as the shipped configs have it)"""
    if ema_embedding.requires_grad:
        raise NotImplementedError("a second operand that needs its own gradient takes gen_targets + ema_embedding_loss")
    lam = [float(affs0_weight) if i < 2 else 1.0 for i in range(len(offsets))]
    loss, affs, _ = _from_labels(embedding, ema_embedding, labels, criterion, offsets, lam, mode, need_affs)
    return loss, affs


def embedding_loss_from_labels_multi(embeddings, labels, criterion, offsets_list, label_steps=None, need_affs=False, weight_tables=None,
                                     affs0_weight=1, mode='ours'):
    """[embedding_loss_from_labels(embeddings[j], labels of scale j, criterion, offsets_list[j], need_affs=need_affs) for j] -> a list of
    (loss, affs, all_loss) -- the four deep-supervision losses of scripts_cvppp/main.py:284-287 straight from label images -- as ONE
    library call (include/pea_multi_labels.h: a count launch, one fused forward + backward launch, one loss finish).
    labels: a list with one label tensor [B,h,w] per embedding, or ONE tensor [B,H,W] that every embedding samples with a step --
    label_steps[j] (an int or (sy, sx)); None: H / h and W / w, which must divide exactly (ValueError otherwise).  Such a strided view
    is what the reference's loader makes with cv2.resize(label, fx=1/2 .. 1/16, INTER_NEAREST), data_provider.py:200-203.
    weight_tables: per embedding None or the [B,K,2] table of pea_label_weights for its (materialised) label image.
    float32, float16 and bfloat16 embeddings are fused alike as long as all n share ONE dtype, at every size (this form was measured
    no slower than the single calls at B = 8 and faster at B = 2).  A 16-bit gradient is rounded when the call stores it and once
    more when backward() rescales it by a grad_output that is no power of two: within one ulp of the f32 product.  A table outside
    the fused set (embeddings of different dtypes, D other than 16 / 32, more than four losses or twelve offsets) and any
    foreign criterion run the single calls on materialised label images -- embedding_loss_from_labels, or, for a foreign criterion
    (which that call refuses), gen_targets + embedding_loss -- same results."""
    n = len(embeddings)
    if len(offsets_list) != n or (weight_tables is not None and len(weight_tables) != n):
        raise ValueError("one offset list (and weight table) per embedding")
    sources = label_sources(embeddings, 2, labels, label_steps)
    if _fused(criterion):
        specs = [_spec(offs, [1.0] * len(offs), mode) for offs in offsets_list]
        try:
            out = MultiLabelsAffinityMSE.apply(specs, sources, _FLAGS_2D, bool(need_affs), weight_tables, *embeddings)
            return [(out[j], out[n + j], LossList(out[2 * n + j])) for j in range(n)]
        except MultiLabelsUnsupported:
            pass
        return [embedding_loss_from_labels(e, materialise_labels(lab, e, 2, step), criterion, offs, affs0_weight=affs0_weight, mode=mode,
                                           need_affs=need_affs)
                for e, (lab, step), offs in zip(embeddings, sources, offsets_list)]
    from ..utils.targets import gen_targets
    out = []
    for e, (lab, step), offs in zip(embeddings, sources, offsets_list):
        t, m, w = gen_targets(materialise_labels(lab, e, 2, step), offs, padding=True)
        out.append(embedding_loss(e, t, w, m, criterion, offs, affs0_weight=affs0_weight, mode=mode))
    return out
