#!/usr/bin/env python3
"""convert_consistency_flip as it was (a clone, a copy of the rules to the host, up to three flip / transpose views per sample, one
torch.stack: the private copy below) against pea_consistency_unflip (include/pea_flip.h, csrc/pea_k_unflip.hip: one launch, the rules
read on the device), timed in ONE process through the Python API at the shapes of the training loops:

  cvppp_B8    8 x 16 x 544^2 f32, random (x-flip, y-flip, xy-transpose) rules
  cvppp_B2    2 x 16 x 544^2 f32
  ac3ac4_B2   2 x 16 x 18 x 160^2 f32, random (z-flip, x-flip, y-flip, xy-transpose) rules; the torch side is the four-rule composition
              (the function as it was has no such form)

each eager (the call issued from Python as a user would, host gaps and the old function's host synchronisation included) and, the
HIP call, replayed from a HIP graph (pea.graphed) together with the EMA cross loss it feeds (ema_embedding_loss / _norm5); the same
graph without the un-flip is timed beside it, the difference being what the call costs inside a captured step.  The old function
cannot be captured (it reads the rules on the host).

After warm-up the variants of a leg alternate batch by batch; a batch times `--reps` calls between two HIP events; min, median and max
of the batches in microseconds per call.  A fresh set of rules is drawn for every batch (the same for both variants).
`hip_faster_beyond_spread`: the HIP median below the torch median by more than the batch-to-batch spread (max - min) of either.
Reading the flag: the torch function launches one copy per set rule, so with a fresh draw per batch its max - min holds the draws as
well as the noise.  In the recorded run (unflip_ab.json) that alone keeps the flag false at ac3ac4_B2: torch 91.6 / 115.3 / 188.2 us
(min / median / max) against HIP 21.3 / 22.6 / 23.0 us -- the gain of 92.7 us is below torch's own spread of 96.5 us although the
slowest HIP batch is four times faster than the fastest torch batch.
GB/s: 2 x tensor bytes (every element read once, written once) over the median; `fraction_of_copy_rate`: of the 4.7-5.3 TB/s DESIGN.md
section 5 quotes for copy-like kernels (the range's lower and upper end).

  python profiles/unflip_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/unflip_ab.json] [--only LEG]"""
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

COPY_RATE_TBS = (4.7, 5.3)


def torch_convert_consistency_flip(ema_embedding, rules):
    """harness/train_step.convert_consistency_flip before pea_consistency_unflip (four rules: the reference's 3D order, z-flip first)"""
    out = ema_embedding.detach().clone()
    r = rules.detach().cpu().numpy().astype(np.uint8)
    o = r.shape[1] - 3
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
    return torch.stack(parts, dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unflip_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(29)
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)

    def rand(*shape):
        return torch.randn(shape, generator=gen, device=dev)

    def binary(*shape):
        return (torch.rand(shape, generator=gen, device=dev) < 0.6).float()

    def leg(shape, nrules):
        ema, e = rand(*shape), rand(*shape)
        rules = torch.zeros((shape[0], nrules), dtype=torch.float32, device=dev)
        if len(shape) == 4:
            K = len(offsets)
            kshape = (shape[0], K) + shape[2:]
            T, W, M = binary(*kshape), torch.rand(kshape, generator=gen, device=dev) + 0.5, binary(*kshape).to(torch.uint8)
            loss_fn = lambda un: pkg.ema_embedding_loss(e, un, T, W, M, crit, offsets)[0]
        else:
            kshape = (shape[0], 12) + shape[2:]
            T, W = binary(*kshape), torch.rand(kshape, generator=gen, device=dev) + 0.5
            loss_fn = lambda un: pkg.ema_embedding_loss_norm5(e, un, T, W, crit)[0]
        graphs = {}

        def step(variant):
            if variant == "torch":
                return torch_convert_consistency_flip(ema, rules)
            if variant == "hip":
                return pkg.convert_consistency_flip(ema, rules)
            if variant not in graphs:  # "graphed_hip_and_loss" / "graphed_loss_alone"
                with_unflip = variant == "graphed_hip_and_loss"
                graphs[variant] = pkg.graphed(lambda ema, rules: loss_fn(pkg.convert_consistency_flip(ema, rules) if with_unflip else ema), ema, rules)
            return graphs[variant].replay()

        def redraw():
            rules.copy_((torch.rand(rules.shape, generator=gen, device=dev) < 0.5).float())
        return step, redraw, 2 * ema.numel() * ema.element_size()

    legs = {"cvppp_B8": ((8, 16, 544, 544), 3), "cvppp_B2": ((2, 16, 544, 544), 3), "ac3ac4_B2": ((2, 16, 18, 160, 160), 4)}
    if a.only and a.only not in legs:
        raise SystemExit("unknown leg %r (one of %s)" % (a.only, ", ".join(legs)))
    variants = ["torch", "hip", "graphed_hip_and_loss", "graphed_loss_alone"]
    rows = {}
    for name, (shape, nrules) in legs.items():
        if a.only and a.only != name:
            continue
        step, redraw, moved = leg(shape, nrules)
        redraw()
        assert torch.equal(step("torch"), step("hip"))
        for v in variants:
            for _ in range(a.warmup):
                step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            redraw()
            for v in variants:
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.reps):
                    step(v)
                s1.record()
                torch.cuda.synchronize()
                times[v].append(s0.elapsed_time(s1) * 1e3 / a.reps)
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        for v in ("torch", "hip"):
            row[v]["GBps_on_2x_tensor_bytes"] = moved / row[v]["median_us"] * 1e-3
        t, h = row["torch"], row["hip"]
        gain = t["median_us"] - h["median_us"]
        spread = max(t["max_us"] - t["min_us"], h["max_us"] - h["min_us"])
        in_graph = row["graphed_hip_and_loss"]["median_us"] - row["graphed_loss_alone"]["median_us"]
        row.update(shape=list(shape), bytes_read_plus_written=moved, median_gain_us=gain, largest_spread_us=spread,
                   torch_over_hip=t["median_us"] / h["median_us"], hip_faster_beyond_spread=bool(gain > spread),
                   hip_slower_beyond_spread=bool(-gain > spread),
                   hip_fraction_of_copy_rate=[h["GBps_on_2x_tensor_bytes"] / (r * 1e3) for r in reversed(COPY_RATE_TBS)],
                   unflip_inside_graph_us=in_graph, unflip_inside_graph_GBps=moved / in_graph * 1e-3 if in_graph > 0 else None)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step, redraw
        torch.cuda.empty_cache()
    out = {"kernel_form": "64 x 64 tiles, dword / 16-bit loads and stores, the transpose through a [64][65]-dword LDS tile (csrc/pea_k_unflip.hip)",
           "torch": "clone + rules to the host + up to three flip / transpose views per sample + torch.stack",
           "copy_rate_TBps_DESIGN_5": list(COPY_RATE_TBS), "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup,
           "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
