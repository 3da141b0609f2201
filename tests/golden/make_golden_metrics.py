#!/usr/bin/env python3
"""Generate tests/golden/gmetrics_2d.npz and gmetrics_3d.npz: the validation pixel metrics of the reference's drivers on small seeded
inputs (include/pea_metrics.h says what they are).

Run on the development machine only (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity, and sklearn; the GPU box
has neither):
    python tests/golden/make_golden_metrics.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_cvppp/loss/loss.py      MSELoss (:126-132) and BCELoss (:134-140), the valid_mse / valid_bce of scripts_cvppp/main.py

gmetrics_2d  pred [1, 4, 24, 40] float32 in (-0.3, 1.3), binary target and binary mask (uint8); expected = scripts_cvppp/main.py:395-397
             run as written: pred = F.relu(pred), valid_mse(pred * affs_mask, target * affs_mask),
             valid_bce(torch.clamp(pred, 0, 1) * affs_mask, target * affs_mask) with affs_mask = mask.float() (:387)
gmetrics_3d  the stitcher's accumulators out_affs [12, 6, 20, 24] (stored as float16: every value is exactly a float16, the tests
             widen them to float32) and weight_map [6, 20, 24] in (0.5, 2), gt_affs [3, 4, 14, 16] (uint8), valid_padding (1, 3, 4);
             expected = scripts_ac3ac4/data/provider_valid.py:337-349 (divide, crop) and scripts_ac3ac4/main.py:308, 344-351 restated
             in numpy statement for statement, F1 from sklearn's f1_score

Both fixtures hold arrays only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))


def load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_2d(ref):
    loss = load(ref, "ref_loss_cvppp", "scripts_cvppp/loss/loss.py")
    valid_mse, valid_bce = loss.MSELoss(), loss.BCELoss()
    rng = np.random.default_rng(20)
    pred = rng.uniform(-0.3, 1.3, (1, 4, 24, 40)).astype(np.float32)
    target = (rng.random(pred.shape) < 0.6).astype(np.uint8)
    mask = (rng.random(pred.shape) < 0.8).astype(np.uint8)
    p, t, affs_mask = torch.from_numpy(pred), torch.from_numpy(target).float(), torch.from_numpy(mask).float()
    p = F.relu(p)
    temp_mse = valid_mse(p * affs_mask, t * affs_mask)
    temp_bce = valid_bce(torch.clamp(p, 0.0, 1.0) * affs_mask, t * affs_mask)
    path = os.path.join(OUT, "gmetrics_2d.npz")
    np.savez_compressed(path, pred=pred, target=target, mask=mask, relu=np.ascontiguousarray(p.numpy()),
                        mse=np.float64(temp_mse.item()), bce=np.float64(temp_bce.item()))
    print("wrote", path, os.path.getsize(path), "bytes; mse %.9g bce %.9g" % (temp_mse.item(), temp_bce.item()))


def make_3d():
    from sklearn.metrics import f1_score
    rng = np.random.default_rng(21)
    C, Z, Y, X = 12, 6, 20, 24
    pad = (1, 3, 4)
    weight_map = rng.uniform(0.5, 2.0, (1, Z, Y, X)).astype(np.float32)
    acc16 = (rng.uniform(-0.1, 1.1, (C, Z, Y, X)).astype(np.float32) * weight_map).astype(np.float16)
    out_affs = acc16.astype(np.float32)
    gt = (rng.random((3, Z - 2 * pad[0], Y - 2 * pad[1], X - 2 * pad[2])) < 0.7).astype(np.uint8)
    # provider_valid.py:337-349
    out_affs = out_affs / weight_map
    out_affs = out_affs[:, pad[0]:-pad[0], pad[1]:-pad[1], pad[2]:-pad[2]]
    results = np.ascontiguousarray(out_affs)
    # main.py:308, 344-351
    gt_affs = gt.astype(np.float32)
    out_affs = out_affs[:3]
    whole_mse = np.sum(np.square(out_affs - gt_affs)) / np.size(gt_affs)
    out_affs = np.clip(out_affs, 0.000001, 0.999999)
    bce = -(gt_affs * np.log(out_affs) + (1 - gt_affs) * np.log(1 - out_affs))
    whole_bce = np.sum(bce) / np.size(gt_affs)
    out_affs[out_affs <= 0.5] = 0
    out_affs[out_affs > 0.5] = 1
    a, b = 1 - gt_affs.astype(np.uint8).flatten(), 1 - out_affs.astype(np.uint8).flatten()
    whole_f1 = f1_score(a, b)
    counts = np.array([np.sum((a == 1) & (b == 1)), np.sum((a == 0) & (b == 1)), np.sum((a == 1) & (b == 0))], np.int64)
    path = os.path.join(OUT, "gmetrics_3d.npz")
    np.savez_compressed(path, acc_f16=acc16, weight_map=weight_map, gt=gt, padding=np.array(pad, np.int32), results=results[:3],
                        mse=np.float64(whole_mse), bce=np.float64(whole_bce), f1=np.float64(whole_f1), counts=counts)
    print("wrote", path, os.path.getsize(path), "bytes; mse %.9g bce %.9g f1 %.9g counts %s" % (whole_mse, whole_bce, whole_f1, counts))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    make_2d(sys.argv[1])
    make_3d()
