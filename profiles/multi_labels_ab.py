#!/usr/bin/env python3
"""The labels-in loss sections with the deep-supervision scales served per scale from four nearest-downsampled label images
(batched=False with explicit label_downs: what the sections did before include/pea_multi_labels.h -- per scale two launches for the
class-balance table, a labels-in step and its loss finish, the tensor path for scales smaller than a tile) against ONE
pea_affinity_fwd_bwd_labels_multi call for the four scales sampling the full-resolution label image (batched=True,
label_downs=None: a memset node, a count launch, one fused forward + backward launch, one loss finish), timed in ONE process through
the Python API:

  cvppp_B8[_graphed]   cvppp_loss_section_from_labels, 8 x 16 x 544^2, K = 10, scales 272^2 .. 34^2
  cvppp_B2[_graphed]   the same at B = 2
  ac3ac4[_graphed]     ac3ac4_loss_section_from_labels, 2 x 16 x 18 x 160^2, norm5, heads 80^2 .. 10^2 (norm1)

each eager (the calls issued from Python as a user would, host gaps included) and replayed from a HIP graph (pea.graphed).  After
warm-up the two variants of a leg alternate batch by batch; a batch times `--reps` steps between two HIP events; min, median and max
of the batches in microseconds per step.  `faster_beyond_spread`: the batched median below the other by more than the batch-to-batch
spread (max - min) of either variant.

  python profiles/multi_labels_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/multi_labels_ab.json] [--only LEG]

--only LEG[:0|:1] runs one leg (one variant) alone."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_labels_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(29)
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half = 2

    def rand(*shape):
        return torch.randn(shape, generator=gen, device=dev)

    def cvppp(B, graphed):
        H = 544
        leaves = [rand(B, 16, H, H).requires_grad_(True)] + [rand(B, 16, H >> (j + 1), H >> (j + 1)).requires_grad_(True) for j in range(4)]
        labels = torch.from_numpy(synth.synth_labels(B, (1, H, H), 31, cell=48)[:, 0]).to(dev)
        downs = [labels[:, ::2 << j, ::2 << j].contiguous() for j in range(4)]  # what the loader's nearest resize hands over
        bufs = leaves + [rand(B, 16, H, H), labels] + downs

        def section(batched, *b):
            for x in b[:5]:
                x.grad = None
            loss, pred, _ = pkg.cvppp_loss_section_from_labels(b[0], list(b[1:5]), b[5], b[6], None if batched else list(b[7:11]), crit,
                                                               offsets, nb_half, batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, bufs, graphed)

    def ac3ac4(graphed):
        B, Z, Y = 2, 18, 160
        leaves = [rand(B, 16, Z, Y, Y).requires_grad_(True)] + [rand(B, 16, Z, Y >> j, Y >> j).requires_grad_(True) for j in (4, 3, 2, 1)]
        seg = torch.from_numpy(synth.synth_labels(B, (Z, Y, Y), 37, cell=20)).to(dev)
        downs = [seg[:, :, ::1 << j, ::1 << j].contiguous() for j in (1, 2, 3, 4)]  # seg of down1 .. down4
        bufs = leaves + [rand(B, 16, Z, Y, Y), seg] + downs

        def section(batched, *b):
            for x in b[:5]:
                x.grad = None
            loss, pred = pkg.ac3ac4_loss_section_from_labels(b[0], list(b[1:5]), b[5], b[6], None if batched else list(b[7:11]), crit,
                                                             embedding_mode=5, batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, bufs, graphed)

    legs = {}
    for g in (False, True):
        sfx = "_graphed" if g else ""
        legs["cvppp_B8" + sfx] = lambda g=g: cvppp(8, g)
        legs["cvppp_B2" + sfx] = lambda g=g: cvppp(2, g)
        legs["ac3ac4" + sfx] = lambda g=g: ac3ac4(g)
    only, _, variant = (a.only or "").partition(":")
    if only and only not in legs:
        raise SystemExit("unknown leg %r (one of %s)" % (only, ", ".join(legs)))
    variants = [bool(int(variant))] if variant else [False, True]
    rows = {}
    for name, make in legs.items():
        if only and only != name:
            continue
        step = make()
        for b in variants:
            for _ in range(a.warmup):
                step(b)
        torch.cuda.synchronize()
        times = {b: [] for b in variants}
        for _ in range(a.batches):
            for b in variants:
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.reps):
                    step(b)
                s1.record()
                torch.cuda.synchronize()
                times[b].append(s0.elapsed_time(s1) * 1e3 / a.reps)
        row = {("batched" if b else "unbatched"): {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v)} for b, v in times.items()}
        if len(row) == 2:
            u, m = row["unbatched"], row["batched"]
            gain = u["median_us"] - m["median_us"]
            spread = max(u["max_us"] - u["min_us"], m["max_us"] - m["min_us"])
            row.update(median_gain_us=gain, largest_spread_us=spread, unbatched_over_batched=u["median_us"] / m["median_us"],
                       faster_beyond_spread=bool(gain > spread), slower_beyond_spread=bool(-gain > spread))
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step
        torch.cuda.empty_cache()
    out = {"kernel_form": "gather from global memory, one lane per voxel, labels sampled with a step (csrc/pea_k_multi_labels.hip); "
                          "no LDS-staged form was built",
           "variants": {"unbatched": "batched=False, explicit label_downs (per-scale launches)",
                        "batched": "batched=True, label_downs=None (one pea_affinity_fwd_bwd_labels_multi call)"},
           "shapes": {"cvppp": "B x 16 x 544^2, K = 10; scales 272^2 / 136^2 / 68^2 / 34^2, K = 8 / 6 / 4 / 2",
                      "ac3ac4": "2 x 16 x 18 x 160^2, norm5; heads 18 x 80^2 / 40^2 / 20^2 / 10^2, norm1"},
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_step": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


def _maybe_graphed(pkg, section, bufs, graphed):
    """step(batched): the section eagerly, or the replay of its HIP graph (one capture per variant, made on first use)"""
    if not graphed:
        return lambda batched: section(batched, *bufs)
    graphs = {}

    def step(batched):
        if batched not in graphs:
            graphs[batched] = pkg.graphed(lambda *b: section(batched, *b), *bufs)
        graphs[batched].replay()
    return step


if __name__ == "__main__":
    main()
