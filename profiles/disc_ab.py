#!/usr/bin/env python3
"""The discriminative instance loss, forward + backward, four ways in ONE process:

  reference  the reference's op sequence (scripts_ac3ac4/loss/loss_discriminative.py:6-60) restated with torch ops on the device: per
             image torch.unique (a host round trip), a Python loop over the ids, per id a mask, a gather, a mean, a norm, a relu and a
             mean; autograd
  dropin     pea.discriminative_loss(e, labels) + backward: the label range is read on the host once (one synchronisation)
  eager      pea.discriminative_loss(e, labels, num_ids=N) + pea.backward (include/pea_disc.h: four forward launches, one backward
             launch, no synchronisation)
  graphed    the same step captured with pea.graphed and replayed

on the BBBC crop shape (8 x 16 x 256 x 256, about 40 ids per image), one CVPPP image (1 x 16 x 544 x 544) and an AC3/AC4 batch
(2 x 16 x 18 x 160 x 160, about 60 ids), int32 labels made of blocks.

After warm-up the variants alternate batch by batch; a batch is `--reps` steps (`--ref-reps` for the reference, whose step is
thousands of launches) between two readings of the host clock, the second one after a device synchronise; the median of the batches
with the fastest and the slowest, in microseconds per step.  Acceptance (recorded, not tuned for): at each shape the median of
`eager` is below the median of `reference`.

  python profiles/disc_ab.py [--batches 7] [--reps 30] [--ref-reps 3] [--warmup 5] [--out profiles/disc_ab.json]

Kernel times are a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/disc_ab.py --batches 1 --no-reference --only bbbc_8x16x256x256 --out ''"""
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


def block_labels(gen, dev, B, spatial, cell, keep=0.8):
    """int32 [B, *spatial]: cells of `cell` pixels per axis, each its own id (1 ..) or, for about 1 - keep of them, 0"""
    grid = [(s + c - 1) // c for s, c in zip(spatial, cell)]
    n = 1
    for g in grid:
        n *= g
    ids = torch.arange(1, n + 1, device=dev, dtype=torch.int32).reshape(grid).expand(B, *grid).clone()
    ids[torch.rand(ids.shape, generator=gen, device=dev) > keep] = 0
    for ax, c in enumerate(cell):
        ids = ids.repeat_interleave(c, dim=1 + ax)
    return ids[(slice(None),) + tuple(slice(0, s) for s in spatial)].contiguous(), n + 1


def reference_loss(e, labels, delta_v=0.5, delta_d=1.5, alpha=1.0, beta=1.0, gama=0.001):
    """the reference's op sequence (background=False) on device tensors"""
    B, D = e.shape[:2]
    x, lab = e.reshape(B, D, -1), labels.reshape(B, -1)
    var = dist = reg = e.new_zeros(())
    for b in range(B):
        ids = torch.unique(lab[b])
        ids = ids[ids != 0]
        C = len(ids)
        if C == 0:
            continue
        means = []
        for c in ids:
            xc = x[b][:, lab[b] == c]
            m = torch.mean(xc, dim=1)
            means.append(m)
            var = var + torch.mean(torch.relu(torch.norm(xc - m.reshape(D, 1), dim=0) - delta_v) ** 2) / C
        M = torch.stack(means)
        if C > 1:
            pd = torch.norm(M.reshape(-1, 1, D) - M.reshape(1, -1, D), dim=2) + torch.eye(C, dtype=M.dtype, device=M.device) * (2 * delta_d)
            dist = dist + torch.sum(torch.relu(2 * delta_d - pd) ** 2) / (C * (C - 1)) / 2
        reg = reg + torch.mean(torch.norm(M, dim=1))
    return (alpha * var + beta * dist + gama * reg) / B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(79)
    rows = {}
    shapes = (("bbbc_8x16x256x256", 8, (256, 256), (40, 40)), ("cvppp_1x16x544x544", 1, (544, 544), (80, 80)),
              ("ac3ac4_2x16x18x160x160", 2, (18, 160, 160), (9, 28, 28)))
    for name, B, spatial, cell in shapes:
        if a.only and name != a.only:
            continue
        e = torch.randn((B, 16) + spatial, generator=gen, device=dev).requires_grad_(True)
        labels, num_ids = block_labels(gen, dev, B, spatial, cell)
        per_image = [int(torch.unique(labels[b]).numel()) - int((labels[b] == 0).any()) for b in range(B)]

        def reference():
            e.grad = None
            loss = reference_loss(e, labels)
            loss.backward()
            return loss, e.grad

        def dropin():
            e.grad = None
            loss = pkg.discriminative_loss(e, labels)
            loss.backward()
            return loss, e.grad

        def eager(x=e, lb=labels):
            x.grad = None
            loss = pkg.discriminative_loss(x, lb, num_ids=num_ids)
            pkg.backward(loss)
            return loss, x.grad

        graph = pkg.graphed(eager, e, labels)
        variants = {"reference": reference, "dropin": dropin, "eager": eager, "graphed": graph.replay}
        reps = {"reference": a.ref_reps, "dropin": a.reps, "eager": a.reps, "graphed": a.reps}
        if a.no_reference:
            del variants["reference"]
        vals = {}
        for v, fn in variants.items():
            for _ in range(min(a.warmup, 2) if v == "reference" else a.warmup):
                out = fn()
            torch.cuda.synchronize()
            vals[v] = {"loss": float(out[0].detach()), "grad_abs_max": float(out[1].abs().max())}
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            for v, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[v]):
                    fn()
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / reps[v])
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        row.update(shape=[B, 16] + list(spatial), num_ids=num_ids, ids_per_image=per_image, values=vals,
                   bytes_three_reads_one_write=4 * 4 * B * 16 * int(labels[0].numel()))
        if "reference" in row:
            ref = row["reference"]
            row.update(reference_spread_us=ref["max_us"] - ref["min_us"],
                       eager_below_reference=bool(row["eager"]["median_us"] < ref["median_us"]),
                       reference_over_eager=ref["median_us"] / row["eager"]["median_us"],
                       reference_over_graphed=ref["median_us"] / row["graphed"]["median_us"])
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del graph
    out = {"kernel_form": "a wave owns 1024 consecutive pixels and peels its ids; integer accumulators per (image, id, channel) "
                          "(csrc/pea_k_disc.hip)",
           "reference": "torch.unique per image, a Python loop over the ids, mask / gather / mean / norm / relu / mean per id, autograd: the op "
                        "sequence of scripts_ac3ac4/loss/loss_discriminative.py:6-60 on the device",
           "clock": "host clock around `reps` steps ending in a device synchronise", "batches": a.batches, "reps_per_batch": a.reps,
           "reference_reps_per_batch": a.ref_reps, "warmup": a.warmup, "us_per_step": rows, "device": torch.cuda.get_device_name(0)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
