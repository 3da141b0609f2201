"""One CVPPP training step, the way one rank of a multi-GPU job runs it (BASELINE.json "train imgs/sec").

What the reference does per iteration (scripts_cvppp/main.py:230-319, shipped cvppp.yaml):
    model(inputs) -> five embeddings + mask logits; model(ema_inputs) -> the EMA embedding (sharing_weights: the same net,
    train mode) -> convert_consistency_flip (per-sample un-flip, DETACHED: scripts_cvppp/data/data_consistency.py:34-45) ->
    five self losses + the EMA cross loss (:284-293) -> ct_weight (0.0) * MSE(embedding, ema_embedding) (:296) ->
    loss.backward() -> relu(pred) -> Adam(lr 1e-4, betas (0.9, 0.999), eps 0.01, weight_decay 1e-6, amsgrad) .step() (:492-493)
under nn.DataParallel with the loss on cuda:0 over the gathered batch (:117-125, :266-293).

Here: one process per GPU.  The backbone (model/unet2d_residual.py, plain PyTorch-ROCm, its heads on pea_head_*) is wrapped by
the caller in DistributedDataParallel (backend "nccl" = RCCL over xGMI): its bucketed gradient all-reduce overlaps the
backward and averages over ranks, which with the LOCAL normaliser 1/(b*W) of each rank's loss reproduces the reference's
1/(B*W) exactly (utils/shard.py).  The loss section is this package's labels-in section (harness/loss_section.py): targets,
masks and class-balance weights are evaluated from the int32 label pyramid inside the kernels, so the per-step host->device
traffic is the images and five label maps instead of ~40 MB of target / weight / mask tensors per image.
The second forward runs under no_grad: its output is detached by convert_consistency_flip, so the graph the reference
builds for it is never used (BatchNorm statistics update the same way)."""
import numpy as np
import torch
import torch.nn.functional as F

from ..loss.loss import WeightedMSE
from ..affinity_op import UNFLIP_DTYPES, check_unflip_shapes, unflip
from ..utils.affinity_ours import multi_offset
from .disc import discriminative_loss_stats
from .fgmask import foreground_mask_loss
from .loss_section import cvppp_loss_section, cvppp_loss_section_from_labels


def _torch_unflip(out, r):
    """the reference's composition on views (simple_augment_reverse_torch: transpose, y-flip, x-flip[, z-flip]) and one torch.stack;
    r: host uint8 [B, 3] = (x-flip, y-flip, xy-transpose) or [B, 4] = (z-flip, x-flip, y-flip, xy-transpose)"""
    o = r.shape[1] - 3  # the AC3/AC4 table puts the z-flip FIRST (scripts_ac3ac4/utils/consistency_aug.py:58-77)
    parts = []
    for b in range(out.shape[0]):
        t = out[b]
        if r[b][o + 2]:
            t = t.transpose(-1, -2)
        if r[b][o + 1]:
            t = t.flip(-2)
        if r[b][o]:
            t = t.flip(-1)
        if o and r[b][0]:
            t = t.flip(-3)
        parts.append(t)
    return torch.stack(parts, dim=0)  # (a transposed view cannot be written back over its own storage)


def convert_consistency_flip(ema_embedding, rules):
    """per-sample inverse of the EMA branch's flips, drawn by the data provider: rules[b] = (x-flip, y-flip, xy-transpose) for a
    [B,C,H,W] tensor (on a [B,C,Z,H,W] tensor: applied to every z slice), or rules[b] = (z-flip, x-flip, y-flip, xy-transpose) for a
    [B,C,Z,H,W] tensor (scripts_ac3ac4/utils/consistency_aug.py:217-228).  Returns a DETACHED tensor, as the reference's
    convert_consistency_flip does (data_consistency.py:36).
    A tensor on a ROCm device takes pea_consistency_unflip (affinity_op.unflip): one launch, the rules read on the device, no host
    synchronisation -- rules that live on the host (list, array, CPU tensor) are uploaded asynchronously through a pinned block of
    torch's caching host allocator (a NEW block is a hipHostMalloc, which can stall the device: the upload is free of that only once
    the allocator's cache is warm, i.e. after the first steps; a loop that wants no such hazard at all hands over device rules);
    under graph capture they must already be a device tensor, which a replay then reads afresh.  A CPU tensor, and a device tensor
    of a dtype the kernel does not move (anything but float32 / float16 / bfloat16), takes the torch composition."""
    if rules is None:
        return ema_embedding.detach().clone()
    if ema_embedding.is_cuda and ema_embedding.dtype in UNFLIP_DTYPES:
        if not (torch.is_tensor(rules) and rules.is_cuda):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("convert_consistency_flip under graph capture needs rules that are a device tensor (a static input)")
            r = rules.detach() if torch.is_tensor(rules) else torch.as_tensor(np.asarray(rules))
            check_unflip_shapes(ema_embedding.shape, r.shape)
            rules = r.contiguous().pin_memory().to(ema_embedding.device, non_blocking=True)
        return unflip(ema_embedding, rules)
    # cast the way the reference does (rules.data.cpu().numpy().astype(np.uint8), :37)
    r = (rules.detach().cpu().numpy() if torch.is_tensor(rules) else np.asarray(rules)).astype(np.uint8)
    check_unflip_shapes(ema_embedding.shape, r.shape)
    return _torch_unflip(ema_embedding.detach(), r)


def label_pyramid(labels):
    """the four nearest-neighbour downsampled label maps the data provider builds on the host with
    cv2.resize(label, (0, 0), fx=fy=1/2 .. 1/16, interpolation=cv2.INTER_NEAREST) (scripts_cvppp/data/data_provider.py:199-208), on the
    device: cv2's nearest rule is src = floor(dst / fx) = 2^j * dst with an output extent of cvRound(n * fx) (round half to even),
    i.e. a strided slice trimmed to that extent (for the provider's 544 x 544 crops the slice itself)"""
    out = []
    for j in range(1, 5):
        f = 2 ** j
        ny, nx = round(labels.shape[-2] / f), round(labels.shape[-1] / f)  # Python's round() is round-half-to-even, like cvRound
        out.append(labels[..., ::f, ::f][..., :ny, :nx].contiguous())
    return out


def make_optimizer(model, base_lr=1e-4):
    return torch.optim.Adam(model.parameters(), lr=base_lr, betas=(0.9, 0.999), eps=0.01, weight_decay=1e-6, amsgrad=True)


class CvpppTrainStep(object):
    """step(inputs, ema_inputs, labels[, rules]) -> loss: forward x2, loss section, backward (DDP all-reduce inside), Adam step.
    `model` is the (DDP-wrapped) ResidualUNet2D_deep; labels int32 [b,H,W] on the model's device.
    mask_weight: None -- the mask logits of the binary_seg head are dropped (the CVPPP step) -- or a number (bbbc039v1.yaml: 1000.0):
    the BBBC039V1 step, which adds mask_weight * BCE_loss_func(pred_mask, labels > 0) (scripts_bbbc039v1/main.py:289) as
    foreground_mask_loss on the same int32 label image, without a host synchronisation; mask_skip_empty is its skip_empty (a crop
    without foreground or without background: 0 for the absent class instead of the reference's NaN).
    disc_weight: None -- the step as it is -- or a number: adds disc_weight * discriminative_loss(embedding, labels,
    background=disc_background, num_ids=disc_num_ids) on the full-resolution embedding (include/pea_disc.h); give disc_num_ids (every
    id < disc_num_ids) to keep the step free of host synchronisations."""

    def __init__(self, model, optimizer=None, shifts=(1, 3, 5, 9, 27), neighbor=4, deep_weight=1, self_emb=1.0, cross_emb=1.0,
                 ct_weight=0.0, affs0_weight=1, disc_weight=None, disc_num_ids=None, disc_background=False, mask_weight=None,
                 mask_skip_empty=False):
        self.model = model
        self.optimizer = optimizer if optimizer is not None else make_optimizer(model)
        self.offsets = multi_offset(list(shifts), neighbor)
        self.nb_half = neighbor // 2
        self.criterion = WeightedMSE()
        self.cfg = dict(deep_weight=deep_weight, self_emb=self_emb, cross_emb=cross_emb, affs0_weight=affs0_weight)
        self.ct_weight = ct_weight
        self.mask_weight = None if mask_weight is None else float(mask_weight)
        self.mask_skip_empty = bool(mask_skip_empty)
        self.disc_weight = None if disc_weight is None else float(disc_weight)
        self.disc_num_ids = disc_num_ids
        self.disc_background = bool(disc_background)
        self.pred = None

    def step(self, inputs, ema_inputs, labels, rules=None):
        self.model.train()
        self.optimizer.zero_grad(set_to_none=True)
        emd4, emd3, emd2, emd1, embedding, mask_logits = self.model(inputs)
        with torch.no_grad():
            ema_embedding = self.model(ema_inputs)[4]
        ema_embedding = convert_consistency_flip(ema_embedding, rules)
        loss, pred, _parts = cvppp_loss_section_from_labels(embedding, [emd1, emd2, emd3, emd4], ema_embedding, labels,
                                                            label_pyramid(labels), self.criterion, self.offsets, self.nb_half,
                                                            relu_pred=True, **self.cfg)
        loss = loss + self.ct_weight * F.mse_loss(embedding, ema_embedding)  # main.py:296 (weight 0.0 in the shipped yaml)
        if self.mask_weight is not None:  # scripts_bbbc039v1/main.py:289
            loss = loss + self.mask_weight * foreground_mask_loss(mask_logits, labels, self.mask_skip_empty)[0]
        if self.disc_weight is not None:
            loss = loss + self.disc_weight * discriminative_loss_stats(embedding, labels, self.disc_background, num_ids=self.disc_num_ids)[0]
        loss.backward()
        self.optimizer.step()
        self.pred = pred
        return loss.detach()
