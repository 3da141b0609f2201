"""3D embedding -> affinity losses: drop-in for the reference's scripts_ac3ac4/loss/loss_embedding_mse.py
(norm1, norm5 and their ema_/inf_ variants -- the ones the shipped ac3ac4.yaml selects, embedding_mode 5
plus norm1 for the four deep-supervision heads, scripts_ac3ac4/main.py:219-230 -- and norm2 / ema_norm2, :70-140, whose loss is
taken on the activated map).

Semantics kept from the reference (file:line there):
  * channel i compares p with p - shift along axis i % 3 of (z,y,x) on the CROPPED extent (:11-18,:143-151);
    the first `shift` slices of that axis stay 0 in `affs` (:22-25,:175-190); no mask tensor
  * WeightedMSE normaliser = B * cropped volume of that channel (pred is [B,1,Z',Y',X'], loss.py:113-115)
  * affs0_weight multiplies loss0 only in norm1 (:20) and channels 0..2 in norm5 (:181-184)
  * norm5's shift table is the literal [1,1,1,2,3,3,3,9,9,4,27,27] (:176); its `shift`/`fill` arguments are unused
  * ema_*: the EMA embedding is the shifted-from operand (:35,:241)
"""

from .. import _lib
from ..affinity_op import (AffinityMap, AffinitySpec, FusedAffinityMSE, LabelsAffinityMSE, LabelsStepUnsupported, MultiAffinityMSE,
                           MultiLabelsAffinityMSE, MultiLabelsUnsupported, MultiUnsupported, affinity_infer, label_sources,
                           materialise_labels)
from ..utils.affinity_ours import NORM5_SHIFTS, axis_offsets_3d
from ._activated import HALF_CLAMP, ones_weight
from ._activated3d import cropped_loss


def _spec(shifts, affs0_weight, first):
    lam = [float(affs0_weight) if i < first else 1.0 for i in range(len(shifts))]
    return AffinitySpec(3, axis_offsets_3d(shifts), lam, _lib.BORDER_CROP_ZERO, _lib.NORM_CROPPED, 1e-12)


def _foreign(embedding, ema_embedding, target, weightmap, criterion, shifts, spec):
    affs = AffinityMap.apply(embedding, ema_embedding, spec)
    loss = 0
    for i, s in enumerate(shifts):
        ax = 2 + i % 3
        n = affs.shape[ax] - s
        li = criterion(affs[:, i:i + 1].narrow(ax, s, n), target[:, i:i + 1].narrow(ax, s, n),
                       weightmap[:, i:i + 1].narrow(ax, s, n))
        loss = loss + li * spec.lam[i]
    return loss, affs.detach()


def _run(embedding, ema_embedding, target, weightmap, criterion, shifts, affs0_weight, first):
    spec = _spec(shifts, affs0_weight, first)
    if getattr(criterion, 'pea_fused', False):
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, None, spec)
        return loss, affs
    if getattr(criterion, 'pea_criterion', None) == 'mse':
        # this package's MSELoss: nn.MSELoss's mean over the cropped slice is WeightedMSE's normaliser there; the weight map is ignored
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, ones_weight(target), None, spec)
        return loss, affs
    return _foreign(embedding, ema_embedding, target, weightmap, criterion, shifts, spec)


def embedding_loss_norm1(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """-> (loss, affs [B,3,Z,Y,X]) -- reference :7-27"""
    return _run(embedding, None, target, weightmap, criterion, [shift] * 3, affs0_weight, 1)


def embedding_loss_norm1_multi(embeddings, targets, weightmaps, criterion, affs0_weight=1, shift=1, need_affs=True):
    """[embedding_loss_norm1(embeddings[j], targets[j], weightmaps[j], criterion, affs0_weight, shift) for j] -> a list of
    (loss, affs) -- the four deep-supervision calls of scripts_ac3ac4/main.py:227-230 -- as ONE forward, one loss finish and one
    backward launch with the fused criterion (include/pea_multi.h: up to four losses; float32, float16 or bfloat16 embeddings, all of
    ONE dtype; D = 16 / 32); anything else takes the single calls.  shift: one value, or one per embedding.  need_affs=False: affs
    is None (never written on the fused path).  16-bit tables too large for the batched launch to pay run call by call as well
    (affinity_op.multi16_pays)."""
    n = len(embeddings)
    if not (len(targets) == len(weightmaps) == n):
        raise ValueError("one target and weightmap per embedding")
    shifts = list(shift) if isinstance(shift, (list, tuple)) else [shift] * n
    if getattr(criterion, 'pea_fused', False):
        specs = [_spec([s] * 3, affs0_weight, 1) for s in shifts]
        try:
            out = MultiAffinityMSE.apply(specs, [(t, w, None) for t, w in zip(targets, weightmaps)], bool(need_affs), *embeddings)
            return [(out[j], out[n + j] if need_affs else None) for j in range(n)]
        except MultiUnsupported:
            pass
    out = [embedding_loss_norm1(e, t, w, criterion, affs0_weight=affs0_weight, shift=s)
           for e, t, w, s in zip(embeddings, targets, weightmaps, shifts)]
    return [(l, a if need_affs else None) for l, a in out]


def ema_embedding_loss_norm1(embedding, ema_embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """reference :30-51"""
    return _run(embedding, ema_embedding, target, weightmap, criterion, [shift] * 3, affs0_weight, 1)


def inf_embedding_loss_norm1(embedding, shift=1):
    """-> affs [B,3,Z,Y,X] -- reference :54-67"""
    return affinity_infer(embedding, None, _spec([shift] * 3, 1, 1))


def embedding_loss_norm2(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """-> (loss, affs [B,3,Z,Y,X]) -- reference :70-103: norm1 with the loss on u = clamp((cos + 1) / 2, 0, 1) (PEA_FLAG_LOSS_ACT: one
    fused forward launch with WeightedMSE, MSELoss, BCELoss or WeightedBCE, loss/_activated3d.py); fill=True stores the next `shift`
    slices in the first ones (:99-102), otherwise they hold 0"""
    return cropped_loss(embedding, None, target, weightmap, criterion, [shift] * 3, affs0_weight, 1, HALF_CLAMP,
                        fill_shift=shift if fill else 0)


def ema_embedding_loss_norm2(embedding, ema_embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """reference :106-140: the EMA embedding is the shifted-from operand"""
    return cropped_loss(embedding, ema_embedding, target, weightmap, criterion, [shift] * 3, affs0_weight, 1, HALF_CLAMP,
                        fill_shift=shift if fill else 0)


def embedding_loss_norm5(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """-> (loss, affs [B,12,Z,Y,X]) -- reference :169-194"""
    return _run(embedding, None, target, weightmap, criterion, NORM5_SHIFTS, affs0_weight, 3)


def ema_embedding_loss_norm5(embedding, ema_embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """reference :263-289"""
    return _run(embedding, ema_embedding, target, weightmap, criterion, NORM5_SHIFTS, affs0_weight, 3)


def inf_embedding_loss_norm5(embedding):
    """-> affs [B,12,Z,Y,X] -- reference :212-234"""
    return affinity_infer(embedding, None, _spec(NORM5_SHIFTS, 1, 3))


# ---- norm6: generic offsets with a replicate border (reference :346-366; not selected by any shipped yaml) ----
def _spec6(offsets):
    return AffinitySpec(3, offsets, None, _lib.BORDER_REPLICATE, _lib.NORM_FULL, 1e-12)


def _run6(embedding, ema_embedding, target, weightmap, criterion, offsets):
    spec = _spec6(offsets)
    if getattr(criterion, 'pea_fused', False):
        # ONE criterion call over the [B,K,Z,Y,X] map: WeightedMSE's normaliser is B*Z*Y*X (loss.py:113-115)
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, target, weightmap, None, spec)
        return loss, affs
    affs = AffinityMap.apply(embedding, ema_embedding, spec)
    return criterion(affs, target, weightmap), affs


def embedding_loss_norm6(embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """-> (loss, affs [B,K,Z,Y,X]); `shift` is the LIST of 3D offsets (the reference's naming, :348); a_i(p) =
    <ehat(p), ehat(clamp(p + o_i))> (shift_tensor with replication padding, :294-344)"""
    return _run6(embedding, None, target, weightmap, criterion, shift)


def ema_embedding_loss_norm6(embedding, ema_embedding, target, weightmap, criterion, affs0_weight=1, shift=1, fill=True):
    """reference :356-366: the EMA embedding is the shifted operand"""
    return _run6(embedding, ema_embedding, target, weightmap, criterion, shift)


# ---- the same losses straight from the segmentation (no target / weightmap tensors) ----
# targets as the 12-channel provider builds them: seg_to_aff(lb, nhood, pad='') (scripts_ac3ac4/data/data_affinity.py:53-102,
# data_provider_labeled_deep.py:253-256): 1 iff both voxels carry the same label > 0, 0 in the border slices; weights =
# weight_binary_ratio per channel over the whole volume.  The cropped-away border pairs carry no loss either way.
_FLAGS_3D = _lib.TGT_BOTH_FOREGROUND


def _run_labels(embedding, ema_embedding, labels, criterion, shifts, affs0_weight, first):
    if not getattr(criterion, 'pea_fused', False):
        raise NotImplementedError("the labels-in step fuses WeightedMSE; for another criterion use gen_targets + the tensor API")
    if ema_embedding is not None and ema_embedding.requires_grad:
        raise NotImplementedError("a second operand that needs its own gradient takes the tensor API")
    spec = _spec(shifts, affs0_weight, first)
    try:
        loss, affs, _ = LabelsAffinityMSE.apply(embedding, ema_embedding, labels, spec, _FLAGS_3D)
    except LabelsStepUnsupported:
        from ..utils.targets import gen_targets
        t, _, w = gen_targets(labels, axis_offsets_3d(shifts), padding=False, both_foreground=True, want_mask=False)
        loss, affs, _ = FusedAffinityMSE.apply(embedding, ema_embedding, t, w, None, spec)
    return loss, affs


def embedding_loss_norm1_from_labels(embedding, labels, criterion, affs0_weight=1, shift=1):
    return _run_labels(embedding, None, labels, criterion, [shift] * 3, affs0_weight, 1)


def embedding_loss_norm1_from_labels_multi(embeddings, labels, criterion, label_steps=None, affs0_weight=1, shift=1, need_affs=True,
                                           weight_tables=None):
    """[embedding_loss_norm1_from_labels(embeddings[j], segmentation of scale j, criterion, affs0_weight, shift) for j] -> a list of
    (loss, affs) -- the four deep-supervision losses of scripts_ac3ac4/main.py:227-230 straight from the segmentation -- as ONE
    library call (include/pea_multi_labels.h).  labels: one tensor [B,z,y,x] per embedding, or ONE tensor [B,Z,Y,X] every embedding
    samples with a step -- label_steps[j]: an int (in-plane, z keeps 1: the reference downsamples slice by slice,
    data_provider_labeled_deep.py:225-232) or (sz, sy, sx); None: label size / embedding size, which must divide exactly.
    shift: one value, or one per embedding.  need_affs=False: the maps are not written (empty tensors come back).  float32, float16
    and bfloat16 embeddings are fused alike as long as all share ONE dtype; anything outside the fused set (mixed dtypes, D other than
    16 / 32) runs the single calls on materialised label images."""
    n = len(embeddings)
    shifts = list(shift) if isinstance(shift, (list, tuple)) else [shift] * n
    if len(shifts) != n or (weight_tables is not None and len(weight_tables) != n):
        raise ValueError("one shift (and weight table) per embedding")
    sources = label_sources(embeddings, 3, labels, label_steps)
    if not getattr(criterion, 'pea_fused', False):
        raise NotImplementedError("the labels-in step fuses WeightedMSE; for another criterion use gen_targets + the tensor API")
    specs = [_spec([s] * 3, affs0_weight, 1) for s in shifts]
    try:
        out = MultiLabelsAffinityMSE.apply(specs, sources, _FLAGS_3D, bool(need_affs), weight_tables, *embeddings)
        return [(out[j], out[n + j]) for j in range(n)]
    except MultiLabelsUnsupported:
        pass
    return [embedding_loss_norm1_from_labels(e, materialise_labels(lab, e, 3, step), criterion, affs0_weight=affs0_weight, shift=s)
            for e, (lab, step), s in zip(embeddings, sources, shifts)]


def embedding_loss_norm5_from_labels(embedding, labels, criterion, affs0_weight=1):
    return _run_labels(embedding, None, labels, criterion, NORM5_SHIFTS, affs0_weight, 3)


def ema_embedding_loss_norm5_from_labels(embedding, ema_embedding, labels, criterion, affs0_weight=1):
    return _run_labels(embedding, ema_embedding, labels, criterion, NORM5_SHIFTS, affs0_weight, 3)
