#!/usr/bin/env python3
"""The validation pixel metrics as the reference's drivers compute them, restated with torch ops on the device, against
pea_affs_metrics (include/pea_metrics.h, csrc/pea_k_metrics.hip: one streaming launch and a small finish), timed in ONE process
through the Python API:

  cvppp_1x10x544     relu_ + the composition of scripts_cvppp/main.py:396-397 -- MSELoss(pred * mask, target * mask),
                     BCELoss(clamp(pred, 0, 1) * mask, target * mask) -- against affinity_metrics(relu=True, store=True) on
                     1 x 10 x 544^2 with a float mask (affs_mask = batch['mask'].float(), main.py:387)
  ac3ac4_12x58x1120  VolumeStitcher.get_results + scripts_ac3ac4/main.py:344-351 restated with torch ops on the device (the
                     reference does these in numpy on the host, after a copy of the volume) against VolumeStitcher.finish, on the
                     12-channel stitched volume of the AC3 / AC4 validation (50 x 1024^2 padded by valid_padding (4, 48, 48)), three
                     channels compared with gt_affs [3, 50, 1024, 1024]

Neither side synchronises the host.  After warm-up the two variants of a leg alternate batch by batch; a batch times `--reps` calls,
each between two HIP events of its own (the stitched volume is restored from a pristine copy before every call of the 3D leg,
outside the timed span: both variants divide it in place); min, median and max of the batches in microseconds per call.
`hip_faster_beyond_spread`: the HIP median below the torch median by more than the batch-to-batch spread (max - min) of either.
GB/s: the bytes the fused pass has to move (pred read and written, target and mask read, the weight map once per channel) over the
median.

  python profiles/metrics_ab.py [--batches 7] [--reps 10] [--warmup 3] [--out profiles/metrics_ab.json] [--only LEG]

Run each leg under a time limit of its own (`timeout 300 python profiles/metrics_ab.py --only LEG`) when looking for trouble."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(31)

    def leg_2d():
        shape = (1, 10, 544, 544)
        pred0 = torch.rand(shape, generator=gen, device=dev) * 1.6 - 0.3
        target = (torch.rand(shape, generator=gen, device=dev) < 0.6).float()
        mask = (torch.rand(shape, generator=gen, device=dev) < 0.8).float()
        pred = pred0.clone()
        mse_fn, bce_fn = torch.nn.MSELoss(), torch.nn.BCELoss()

        def restore():
            pred.copy_(pred0)

        def step(variant):
            if variant == "hip":
                m = pkg.affinity_metrics(pred, target, mask, relu=True, store=True)
                return m.table[0, 0], m.table[0, 1]
            p = pkg.relu_(pred)
            return mse_fn(p * mask, target * mask), bce_fn(torch.clamp(p, 0.0, 1.0) * mask, target * mask)

        def agree():
            restore()
            t = [float(v) for v in step("torch")]
            restore()
            h = [float(v) for v in step("hip")]
            return {"torch_mse_bce": t, "hip_mse_bce": h}
        n = pred.numel()
        return step, restore, agree, n * (4 + 4 + 4 + 4), list(shape)

    def leg_3d():
        vol, pad, win = (58, 1120, 1120), (4, 48, 48), (18, 160, 160)
        st = pkg.VolumeStitcher(12, vol, win, dev)
        wm0 = torch.rand((1,) + vol, generator=gen, device=dev) * 1.5 + 0.5
        acc0 = (torch.rand((12,) + vol, generator=gen, device=dev) * 1.2 - 0.1) * wm0
        gt = (torch.rand((3, vol[0] - 2 * pad[0], vol[1] - 2 * pad[1], vol[2] - 2 * pad[2]), generator=gen, device=dev) < 0.7).float()
        st.weight_map.copy_(wm0)

        def restore():
            st.out_affs.copy_(acc0)

        def step(variant):
            if variant == "hip":
                _, m = st.finish(pad, gt)
                return m.table[0, 0], m.table[0, 1], m.table[0, 2], m.table[0, 3], m.table[0, 4]
            out_affs = st.get_results(pad)[:3]
            whole_mse = torch.sum(torch.square(out_affs - gt)) / gt.numel()
            out_affs = torch.clamp(out_affs, 0.000001, 0.999999)
            bce = -(gt * torch.log(out_affs) + (1 - gt) * torch.log(1 - out_affs))
            whole_bce = torch.sum(bce) / gt.numel()
            pb, gb = out_affs <= 0.5, gt < 1  # 1 - out.astype(uint8), 1 - gt.astype(uint8) after the threshold at 0.5
            return whole_mse, whole_bce, (gb & pb).sum(), (~gb & pb).sum(), (gb & ~pb).sum()

        def agree():
            restore()
            t = [float(v) for v in step("torch")]
            restore()
            h = [float(v) for v in step("hip")]
            return {"torch_mse_bce_tp_fp_fn": t, "hip_mse_bce_tp_fp_fn": h}
        nvol = int(np.prod(vol))
        return step, restore, agree, 12 * nvol * (4 + 4 + 4) + gt.numel() * 4, [12] + list(vol)

    legs = {"cvppp_1x10x544": leg_2d, "ac3ac4_12x58x1120": leg_3d}
    if a.only and a.only not in legs:
        raise SystemExit("unknown leg %r (one of %s)" % (a.only, ", ".join(legs)))
    variants = ["torch", "hip"]
    rows = {}
    for name, mk in legs.items():
        if a.only and a.only != name:
            continue
        step, restore, agree, moved, shape = mk()
        values = agree()
        for v in variants:
            for _ in range(a.warmup):
                restore()
                step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            for v in variants:
                pairs = []
                for _ in range(a.reps):
                    restore()
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    step(v)
                    s1.record()
                    pairs.append((s0, s1))
                torch.cuda.synchronize()
                times[v].append(sum(s0.elapsed_time(s1) for s0, s1 in pairs) * 1e3 / a.reps)
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        t, h = row["torch"], row["hip"]
        gain = t["median_us"] - h["median_us"]
        spread = max(t["max_us"] - t["min_us"], h["max_us"] - h["min_us"])
        h["GBps_on_fused_bytes"] = moved / h["median_us"] * 1e-3
        row.update(shape=shape, fused_bytes=moved, median_gain_us=gain, largest_spread_us=spread, torch_over_hip=t["median_us"] / h["median_us"],
                   hip_faster_beyond_spread=bool(gain > spread), hip_slower_beyond_spread=bool(-gain > spread), values=values)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step, restore, agree
        torch.cuda.empty_cache()
    out = {"kernel_form": "256 lanes x 4 steps x 4 consecutive elements per workgroup, dwordx4 where aligned, integer loss accumulators (csrc/pea_k_metrics.hip)",
           "torch": "relu_ + MSELoss / BCELoss compositions (2D); get_results + the numpy statements of main.py:344-351 as torch ops on the device (3D)",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
