#!/usr/bin/env python3
"""The deep-supervision self losses one launch per scale (batched=False: three launches per scale, what every section runs by default)
against one launch for the four scales each way (batched=True: include/pea_multi.h, csrc/pea_k_multi.hip), timed in ONE process
through the Python API:

  small2d_B2 / small2d_B8   the four small scales alone, forward + backward, at the CVPPP shapes (B x 16 x 272^2 .. 34^2, K = 8 / 6 /
                            4 / 2, packed float `downN` thirds): four embedding_loss calls against one embedding_loss_multi call
  small3d                   the same at the AC3 / AC4 crop's deep scales (2 x 16 x 18 x 80^2 .. 10^2, norm1): four
                            embedding_loss_norm1 calls against one embedding_loss_norm1_multi call
  cvppp_section[_graphed]   cvppp_loss_section (one node; the small scales on the side stream), B x 16 x 544^2, K = 10
  cvppp_composed[_graphed]  cvppp_loss_section_composed (call by call: what INTEGRATION.md section 2 gives)
  ac3ac4_section[_graphed]  ac3ac4_loss_section, 2 x 16 x 18 x 160^2, norm5

each eager (the calls issued from Python as a user would, host gaps included) and, the sections, replayed from a HIP graph
(pea.graphed).  After warm-up the two variants of a leg alternate batch by batch; a batch times `--reps` steps between two HIP events;
min, median and max of the batches in microseconds per step.  `batched_faster_beyond_spread`: the batched median below the other by
more than the batch-to-batch spread (max - min) of either variant.

  python profiles/multi_scale_ab.py [--batches 7] [--reps 20] [--warmup 3] [--section-batch 2] [--out profiles/multi_scale_ab.json] [--only LEG]

--only LEG[:0|:1] runs one leg (one variant) alone: rocprofv3 --kernel-trace --stats -- python profiles/multi_scale_ab.py --only small2d_B2:1"""
import argparse
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
    ap.add_argument("--section-batch", type=int, default=2)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_scale_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(23)
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half = 2

    def rand(*shape):
        return torch.randn(shape, generator=gen, device=dev)

    def binary(*shape):
        return (torch.rand(shape, generator=gen, device=dev) < 0.6).float()

    def downs_2d(B, H):
        """down1..down4: packed (target | weight | mask) float thirds, as the reference's provider builds them"""
        out = []
        for j in range(4):
            k, h = nb_half * (4 - j), H >> (j + 1)
            out.append(torch.cat([binary(B, k, h, h), torch.rand((B, k, h, h), generator=gen, device=dev) + 0.5, binary(B, k, h, h)], dim=1))
        return out

    def small2d(B):
        H = 544
        emds = [rand(B, 16, H >> (j + 1), H >> (j + 1)).requires_grad_(True) for j in range(4)]
        downs = downs_2d(B, H)
        ks = [nb_half * (4 - j) for j in range(4)]
        T, W, M = ([d[:, i * k:(i + 1) * k] for d, k in zip(downs, ks)] for i in range(3))
        offs = [offsets[:k] for k in ks]

        def step(batched):
            for x in emds:
                x.grad = None
            if batched:
                out = pkg.embedding_loss_multi(emds, T, W, M, crit, offs)
            else:
                out = [pkg.embedding_loss(e, t, w, m, crit, o) for e, t, w, m, o in zip(emds, T, W, M, offs)]
            pkg.backward(out[0][0] + out[1][0] + out[2][0] + out[3][0])
        return step

    def small3d():
        B, Z, Y = 2, 18, 160
        emds = [rand(B, 16, Z, Y >> j, Y >> j).requires_grad_(True) for j in (4, 3, 2, 1)]
        T = [binary(B, 3, Z, Y >> j, Y >> j) for j in (4, 3, 2, 1)]
        W = [torch.rand((B, 3, Z, Y >> j, Y >> j), generator=gen, device=dev) + 0.5 for j in (4, 3, 2, 1)]

        def step(batched):
            for x in emds:
                x.grad = None
            if batched:
                out = pkg.embedding_loss_norm1_multi(emds, T, W, crit, need_affs=False)
            else:
                out = [pkg.embedding_loss_norm1(e, t, w, crit) for e, t, w in zip(emds, T, W)]
            pkg.backward(out[0][0] + out[1][0] + out[2][0] + out[3][0])
        return step

    def cvppp(fn, graphed):
        B, H = a.section_batch, 544
        K = len(offsets)
        leaves = [rand(B, 16, H, H).requires_grad_(True)] + [rand(B, 16, H >> (j + 1), H >> (j + 1)).requires_grad_(True) for j in range(4)]
        rest = [rand(B, 16, H, H), binary(B, K, H, H), torch.rand((B, K, H, H), generator=gen, device=dev) + 0.5,
                binary(B, K, H, H).to(torch.uint8)] + downs_2d(B, H)

        def section(batched, *bufs):
            for x in bufs[:5]:
                x.grad = None
            loss, pred, _ = fn(bufs[0], list(bufs[1:5]), bufs[5], bufs[6], bufs[7], bufs[8], list(bufs[9:13]), crit, offsets, nb_half,
                               batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, leaves + rest, graphed)

    def ac3ac4(graphed):
        B, Z, Y = 2, 18, 160
        leaves = [rand(B, 16, Z, Y, Y).requires_grad_(True)] + [rand(B, 16, Z, Y >> j, Y >> j).requires_grad_(True) for j in (4, 3, 2, 1)]
        rest = [rand(B, 16, Z, Y, Y), binary(B, 12, Z, Y, Y), torch.rand((B, 12, Z, Y, Y), generator=gen, device=dev) + 0.5]
        rest += [torch.cat([binary(B, 3, Z, Y >> j, Y >> j), torch.rand((B, 3, Z, Y >> j, Y >> j), generator=gen, device=dev) + 0.5], dim=1)
                 for j in (1, 2, 3, 4)]

        def section(batched, *bufs):
            for x in bufs[:5]:
                x.grad = None
            loss, pred = pkg.ac3ac4_loss_section(bufs[0], list(bufs[1:5]), bufs[5], bufs[6], bufs[7], list(bufs[8:12]), crit, embedding_mode=5,
                                                 batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, leaves + rest, graphed)

    legs = {"small2d_B2": lambda: small2d(2), "small2d_B8": lambda: small2d(8), "small3d": small3d}
    for g in (False, True):
        sfx = "_graphed" if g else ""
        legs["cvppp_section" + sfx] = lambda g=g: cvppp(pkg.cvppp_loss_section, g)
        legs["cvppp_composed" + sfx] = lambda g=g: cvppp(pkg.cvppp_loss_section_composed, g)
        legs["ac3ac4_section" + sfx] = lambda g=g: ac3ac4(g)
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
                       batched_faster_beyond_spread=bool(gain > spread), batched_slower_beyond_spread=bool(-gain > spread))
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step
        torch.cuda.empty_cache()
    out = {"kernel_form": "gather from global memory, one lane per pixel (csrc/pea_k_multi.hip); no LDS-staged form was built",
           "shapes": {"small2d": "B x 16 x 272^2 / 136^2 / 68^2 / 34^2, K = 8 / 6 / 4 / 2, float masks", "small3d": "2 x 16 x 18 x 80^2 / 40^2 / 20^2 / 10^2, norm1",
                      "cvppp": "%d x 16 x 544^2, K = 10" % a.section_batch, "ac3ac4": "2 x 16 x 18 x 160^2, norm5"},
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
