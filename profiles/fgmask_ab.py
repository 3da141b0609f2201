#!/usr/bin/env python3
"""The foreground-mask loss of the BBBC039V1 step, forward + backward, three ways in ONE process:

  reference  the reference's op sequence (scripts_bbbc039v1/loss/loss.py:187-194) restated with torch ops on the device: two
             .item() round trips for the class weights, nn.CrossEntropyLoss(weight=..), autograd
  eager      BCE_loss_func of this package + pea.backward (include/pea_fgmask.h: one forward launch, a finish, one backward launch)
  graphed    the same step captured with pea.graphed and replayed

on the BBBC training shape (8 x 2 x 256 x 256) and the validation shape (1 x 2 x 704 x 704), int32 labels (compared with 0 on the
device in the reference variant, as main.py:289 does).

After warm-up the variants alternate batch by batch; a batch is `--reps` steps between two readings of the host clock, the second
one after a device synchronise (the reference variant synchronises inside every step by itself: that is what is being measured);
the median of the batches with the fastest and the slowest, in microseconds per step.  Acceptance (recorded, not tuned for): the
median of `eager` is not above the median of `reference` at the training shape.

  python profiles/fgmask_ab.py [--batches 7] [--reps 50] [--warmup 10] [--out profiles/fgmask_ab.json]

Kernel times are a run of their own:  rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/fgmask_ab.py --batches 1 --out ''"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgmask_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(77)
    rows = {}
    for name, (B, H, W) in (("train_8x2x256x256", (8, 256, 256)), ("valid_1x2x704x704", (1, 704, 704))):
        logits = (torch.randn((B, 2, H, W), generator=gen, device=dev) * 2.0).requires_grad_(True)
        labels = (torch.rand((B, H, W), generator=gen, device=dev) < 0.3).to(torch.int32) * 17

        def reference():
            logits.grad = None
            target = torch.gt(labels, 0)
            weight = torch.tensor([torch.sum(target == 1).item(), torch.sum(target == 0).item()], dtype=torch.float32).to(dev)
            loss = torch.nn.CrossEntropyLoss(weight=weight)(logits, target.long())
            loss.backward()
            return loss, logits.grad

        def eager(lg=logits, lb=labels):
            lg.grad = None
            loss = pkg.BCE_loss_func(lg, lb)
            pkg.backward(loss)
            return loss, lg.grad

        graph = pkg.graphed(eager, logits, labels)
        variants = {"reference": reference, "eager": eager, "graphed": graph.replay}
        vals = {}
        for v, fn in variants.items():
            for _ in range(a.warmup):
                out = fn()
            torch.cuda.synchronize()
            vals[v] = {"loss": float(out[0]), "grad_abs_max": float(out[1].abs().max())}
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            for v, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / a.reps)
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        ref = row["reference"]
        row.update(shape=[B, 2, H, W], values=vals, reference_spread_us=ref["max_us"] - ref["min_us"],
                   eager_not_above_reference=bool(row["eager"]["median_us"] <= ref["median_us"]),
                   reference_over_eager=ref["median_us"] / row["eager"]["median_us"],
                   reference_over_graphed=ref["median_us"] / row["graphed"]["median_us"])
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del graph
    out = {"kernel_form": "256 lanes x 4 steps x 4 x-adjacent pixels per workgroup, wide loads where aligned, integer loss accumulators (csrc/pea_k_fgmask.hip)",
           "reference": "two .item(), nn.CrossEntropyLoss(weight), autograd: the op sequence of scripts_bbbc039v1/loss/loss.py:187-194 on the device",
           "clock": "host clock around `reps` steps ending in a device synchronise", "batches": a.batches, "reps_per_batch": a.reps,
           "warmup": a.warmup, "us_per_step": rows, "device": torch.cuda.get_device_name(0)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
