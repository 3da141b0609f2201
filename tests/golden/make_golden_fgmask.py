#!/usr/bin/env python3
"""Generate tests/golden/gfg_*.npz: the foreground-mask loss of the BBBC039V1 step and the validation mask, from the reference's own
code on small seeded inputs (include/pea_fgmask.h says what they are).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_fgmask.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_bbbc039v1/loss/loss.py      BCE_loss_func (:187-194), called as scripts_bbbc039v1/main.py:289 calls it:
                                        BCE_loss_func(pred_mask, torch.gt(target_ins[:, 0], 0), weight_rate=[10, 1])
The function moves its class weights with .cuda(), the only thing that stops it on a CPU: torch.Tensor.cuda is patched to the
identity in THIS process only.

gfg_b2_37x53      B = 2, Y * X odd; blocky int32 labels, about 30 % foreground, negative and large ids among them
gfg_b3_64x80      B = 3, 5120 pixels per image
gfg_allbg         no foreground at all: the reference's loss and every element of its gradient are NaN
  each: logits [B, 2, Y, X] float32, labels [B, Y, X] int32, loss / dlogits = the reference's float32 loss and its autograd gradient,
        loss64 / dlogits64 = nn.CrossEntropyLoss with the same weights in float64, params = the parameter names of BCE_loss_func
gfg_valid_200x24  logits [1, 2, 200, 24] with a few exact ties and NaNs inside the crop, crop = ((92, 92), (4, 4)), mask [16, 16] uint8 =
                  scripts_bbbc039v1/main.py:406-410 run as written (softmax, argmax, squeeze, uint8, [92:-92, 4:-4]).  The generator
                  asserts argmax(softmax) == (l1 > l0) on EVERY pixel of the fixture, so the reference alone satisfies the rule the
                  header states.

Arrays and names only.
"""
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))


def load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blocky_labels(rng, B, Y, X, fg=0.3, block=5):
    """instance-like label images: blocks of one id; about `fg` of the blocks positive (small and large ids), the rest 0 or negative"""
    by, bx = (Y + block - 1) // block, (X + block - 1) // block
    pos = rng.random((B, by, bx)) < fg
    ids = np.where(rng.random((B, by, bx)) < 0.2, 2 ** 31 - 1 - rng.integers(0, 5, (B, by, bx)), rng.integers(1, 40, (B, by, bx)))
    neg = np.where(rng.random((B, by, bx)) < 0.25, -rng.integers(1, 2 ** 31, (B, by, bx)), 0)
    coarse = np.where(pos, ids, neg).astype(np.int64)
    lab = np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :Y, :X]
    return np.ascontiguousarray(lab.astype(np.int32))


def make_loss(loss_mod, name, seed, B, Y, X, fg=0.3):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, 2, Y, X)) * 2.0).astype(np.float32)
    labels = blocky_labels(rng, B, Y, X, fg)
    if fg == 0.0:
        assert (labels <= 0).all() and (labels < 0).any()
    else:
        frac = float((labels > 0).mean())
        assert 0.15 < frac < 0.45 and (labels < 0).any() and (labels > 2 ** 30).any(), frac
    target_ins = torch.from_numpy(labels)[:, None]                       # [B, 1, Y, X], as the provider hands it over
    # the reference, as main.py:289 calls it
    pred_mask = torch.from_numpy(logits).clone().requires_grad_(True)
    loss = loss_mod.BCE_loss_func(pred_mask, torch.gt(target_ins[:, 0], 0), weight_rate=[10, 1])
    loss.backward()
    # the same criterion in float64
    t = torch.gt(target_ins[:, 0], 0)
    w64 = torch.tensor([float(torch.sum(t == 1)), float(torch.sum(t == 0))], dtype=torch.float64)
    p64 = torch.from_numpy(logits).double().requires_grad_(True)
    loss64 = nn.CrossEntropyLoss(weight=w64)(p64, t.long())
    loss64.backward()
    params = np.array(list(inspect.signature(loss_mod.BCE_loss_func).parameters))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, logits=logits, labels=labels, loss=np.float32(loss.item()), dlogits=pred_mask.grad.numpy(),
                        loss64=np.float64(loss64.item()), dlogits64=p64.grad.numpy(), params=params)
    print("wrote", path, os.path.getsize(path), "bytes; loss %.9g (float64 %.17g), n1 = %d of %d" %
          (loss.item(), loss64.item(), int(t.sum()), t.numel()))


def make_valid():
    rng = np.random.default_rng(44)
    top, left = 92, 4
    logits = (rng.standard_normal((1, 2, 200, 24)) * 2.0).astype(np.float32)
    for y, x in ((0, 0), (3, 7), (15, 15), (8, 1)):       # exact ties inside the crop
        logits[0, 1, top + y, left + x] = logits[0, 0, top + y, left + x]
    logits[0, 0, top + 1, left + 2] = np.nan             # NaN in either channel, in both
    logits[0, 1, top + 5, left + 9] = np.nan
    logits[0, :, top + 12, left + 3] = np.nan
    logits[0, 1, 10, 10] = logits[0, 0, 10, 10]          # .. and outside it
    logits[0, 1, 199, 23] = np.nan
    # main.py:406-410
    pred_mask = torch.from_numpy(logits)
    pred_mask = F.softmax(pred_mask, dim=1)
    pred_mask = torch.argmax(pred_mask, dim=1).squeeze(0)
    pred_mask_b = pred_mask.data.cpu().numpy()
    pred_mask_b = pred_mask_b.astype(np.uint8)
    full = pred_mask_b.copy()
    pred_mask_b = pred_mask_b[92:-92, 4:-4]
    with np.errstate(invalid="ignore"):
        rule = (logits[0, 1] > logits[0, 0]).astype(np.uint8)
    assert np.array_equal(full, rule), "argmax(softmax) != (l1 > l0) somewhere: choose another seed"
    assert pred_mask_b.shape == (16, 16) and 0 < pred_mask_b.sum() < 256
    path = os.path.join(OUT, "gfg_valid_200x24.npz")
    np.savez_compressed(path, logits=logits, crop=np.array([[92, 92], [4, 4]], dtype=np.int32), mask=np.ascontiguousarray(pred_mask_b))
    print("wrote", path, os.path.getsize(path), "bytes; %d of 256 foreground" % int(pred_mask_b.sum()))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    torch.Tensor.cuda = lambda self, *a, **k: self       # (module docstring) this process only
    loss_mod = load(ref, "ref_loss_bbbc", "scripts_bbbc039v1/loss/loss.py")
    make_loss(loss_mod, "gfg_b2_37x53", 41, 2, 37, 53)
    make_loss(loss_mod, "gfg_b3_64x80", 42, 3, 64, 80)
    make_loss(loss_mod, "gfg_allbg", 43, 2, 12, 20, fg=0.0)
    make_valid()


if __name__ == "__main__":
    main()
