#!/usr/bin/env python3
"""The segmentation scores of the validation loops (SBD, FG/BG Dice, VOI, ARAND) three ways, timed in ONE process:

  hip          pea.segmentation_scores on device label images (include/pea_segscore.h: one pass over the pixels, three over the
               table's slots, a finish), the [B, 19] table left on the device
  hip_upload   the same from numpy label images (the segmentation comes from elf / waterz on the host): upload, call, and the
               table read back
  torch        the same scores from a torch composition on the device: per image torch.unique(keys, return_counts=True) on the
               combined 64-bit keys, the marginals by unique + scatter_add, the best Dice by scatter_reduce(amax), VOI and ARAND
               from the counts; the columns stacked on the device
  host         tests/segscore_reference.py (numpy, np.unique on combined keys) on the host arrays

on three shapes: one 544 x 544 image with about 20 ids (CVPPP), eight 256 x 256 crops (BBBC), and 24 images of 1024 x 1024 with
several thousand ids each.

Every call is timed by a host clock around work that ends in a device synchronise (torch.unique synchronises by itself; the host
variant has no device work).  After warm-up the variants alternate batch by batch; a batch times `--reps` calls (the host variant
one); min, median and max of the batches in microseconds per call.  Recorded, not gated.

  python profiles/segscore_ab.py [--batches 7] [--reps 10] [--warmup 3] [--out profiles/segscore_ab.json] [--only LEG]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from segscore_reference import COL, seg_reference  # noqa: E402

SHOWN = ("sbd", "fgbg_dice", "voi_split", "voi_merge", "are")


def torch_scores_image(p, g):
    """one image's columns (sbd, fgbg_dice, voi_split, voi_merge, are) from torch ops on the device"""
    keys, n = torch.unique((p.long() << 32) | g.long(), return_counts=True)
    kp, kg = keys >> 32, keys & 0xffffffff
    up, ip = torch.unique(kp, return_inverse=True)
    ug, ig = torch.unique(kg, return_inverse=True)
    a = torch.zeros(up.numel(), dtype=torch.int64, device=p.device).scatter_add_(0, ip, n)
    b = torch.zeros(ug.numel(), dtype=torch.int64, device=p.device).scatter_add_(0, ig, n)
    min_p, max_p, min_g, max_g = up[0], up[-1], ug[0], ug[-1]
    fg = (kp > min_p) & (kg > min_g)
    dice = torch.where(fg, 2.0 * n.double() / (a[ip] + b[ig]).double(), torch.zeros((), dtype=torch.float64, device=p.device))
    best_p = torch.zeros(up.numel(), dtype=torch.float64, device=p.device).scatter_reduce_(0, ip, dice, "amax")
    best_g = torch.zeros(ug.numel(), dtype=torch.float64, device=p.device).scatter_reduce_(0, ig, dice, "amax")
    bd = torch.where(max_p > min_p, best_p.sum() / (max_p - min_p).clamp(min=1), torch.zeros((), dtype=torch.float64, device=p.device))
    bdr = torch.where(max_g > min_g, best_g.sum() / (max_g - min_g).clamp(min=1), torch.zeros((), dtype=torch.float64, device=p.device))
    fg_p, fg_g = a[1:].sum(), b[1:].sum()
    fgbg = 2.0 * (n * fg).sum().double() / (fg_p + fg_g).clamp(min=1).double()
    keep = kg != 0
    nk = (n * keep).double()
    ap = torch.zeros(up.numel(), dtype=torch.float64, device=p.device).scatter_add_(0, ip, nk)
    bp = torch.where(ug != 0, b, torch.zeros_like(b)).double()
    n_prime = nk.sum()
    xlogx = lambda v: (v * torch.log2(v.clamp(min=1.0))).sum()
    split, merge = (xlogx(bp) - xlogx(nk)) / n_prime, (xlogx(ap) - xlogx(nk)) / n_prime
    P2, A2, B2 = (nk * nk).sum() - n_prime, (ap * ap).sum() - n_prime, (bp * bp).sum() - n_prime
    return torch.stack([torch.minimum(bd, bdr), fgbg, split, merge, 1.0 - P2 / (0.5 * A2 + 0.5 * B2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segscore_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")

    def leg(B, Y, X, cells, n_ids):
        pred = synth.synth_labels(B, (1, Y, X), 901, cell=cells[0], n=n_ids[0])[:, 0].astype(np.int32)
        gt = synth.synth_labels(B, (1, Y, X), 902, cell=cells[1], n=n_ids[1])[:, 0].astype(np.int32)
        P, G = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)

        def step(variant):
            if variant == "hip":
                return pkg.segmentation_scores(P, G).table
            if variant == "hip_upload":
                return pkg.segmentation_scores(pred, gt).table.cpu()
            if variant == "torch":
                return torch.stack([torch_scores_image(P[b].reshape(-1), G[b].reshape(-1)) for b in range(B)])
            return seg_reference(pred, gt)
        return step, pred, gt

    legs = {"cvppp_1x544x544": lambda: leg(1, 544, 544, (96, 80), (20, 18)),
            "bbbc_8x256x256": lambda: leg(8, 256, 256, (24, 20), (60, 50)),
            "large_24x1024x1024": lambda: leg(24, 1024, 1024, (16, 12), (4000, 3000))}
    if a.only and a.only not in legs:
        raise SystemExit("unknown leg %r (one of %s)" % (a.only, ", ".join(legs)))
    variants = ["hip", "hip_upload", "torch", "host"]
    rows = {}
    for name, mk in legs.items():
        if a.only and a.only != name:
            continue
        step, pred, gt = mk()
        ref = seg_reference(pred, gt)
        hip, tor = step("hip").cpu().numpy(), step("torch").cpu().numpy()
        values = {"n_pairs_per_image": [int(v) for v in ref[:, COL["n_pairs"]]], "n_pred_ids_per_image": [int(v) for v in ref[:, COL["n_pred_ids"]]],
                  "capacity": pkg.segmentation_scores(pred, gt).capacity, "n_overflow": [int(v) for v in hip[:, 0]],
                  "max_abs_hip_minus_host": {c: float(np.abs(hip[:, COL[c]] - ref[:, COL[c]]).max()) for c in SHOWN},
                  "max_abs_torch_minus_host": {c: float(np.abs(tor[:, i] - ref[:, COL[c]]).max()) for i, c in enumerate(SHOWN)}}
        reps = {v: (1 if v == "host" else a.reps) for v in variants}
        for v in variants:
            for _ in range(1 if v == "host" else a.warmup):
                step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            for v in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[v]):
                    step(v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / reps[v])
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        h = row["hip"]["median_us"]
        row.update(shape=list(pred.shape), torch_over_hip=row["torch"]["median_us"] / h, host_over_hip_upload=row["host"]["median_us"] / row["hip_upload"]["median_us"],
                   label_bytes=int(pred.nbytes + gt.nbytes), hip_GBps_on_label_bytes=(pred.nbytes + gt.nbytes) / h * 1e-3, values=values)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step
        torch.cuda.empty_cache()
    out = {"kernel_form": "a wave peels the (pred, gt) pairs of 256 consecutive pixels, one table update per (wave, pair); open addressing on 64-bit "
                          "keys, bounded probes; integer and fixed-point sums (csrc/pea_k_segscore.hip)",
           "timing": "host clock around calls that end in a device synchronise; medians over alternating batches",
           "batches": a.batches, "reps_per_batch": a.reps, "host_reps_per_batch": 1, "warmup": a.warmup, "us_per_call": rows,
           "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
