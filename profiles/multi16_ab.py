#!/usr/bin/env python3
"""The CVPPP six-loss section on 16-bit embeddings (what OutConv / EmbeddingHead emit under torch.autocast) with the four
deep-supervision scales one call at a time (batched=False) against one launch for the four each way (batched=True: include/pea_multi.h
and include/pea_multi_labels.h on f16 / bf16 storage), timed in ONE process through the Python API:

  cvppp_tensor[_graphed]   cvppp_loss_section, B x 16 x 544^2, K = 10, scales 272^2 .. 34^2 with packed float `downN` thirds
  cvppp_labels[_graphed]   cvppp_loss_section_from_labels on the same shapes (batched: label_downs=None, the scales sample the
                           full-resolution label image; unbatched: four nearest-downsampled label images)
  small2d                  the four small scales alone: four embedding_loss calls against one embedding_loss_multi call

each eager (the calls issued from Python as a user would, host gaps included) and, the sections, replayed from a HIP graph
(pea.graphed).  After warm-up the two variants of a leg alternate batch by batch; a batch times `--reps` steps between two HIP events;
min, median and max of the batches in microseconds per step.  `faster_beyond_spread`: the batched median below the other by more than
the batch-to-batch spread (max - min) of either variant.

On a checkout whose batched launches are f32-only, batched=True falls back (MultiUnsupported) and both columns are the call-by-call
path: `--root DIR` times the package of another checkout of the project (the parent commit, built in DIR) with this script, and
`--run NAME` files the result under that name in --out beside the runs already there.

  python profiles/multi16_ab.py [--dtype bf16] [--batch 8] [--batches 7] [--reps 100] [--warmup 3] [--run change] [--root DIR]
                                [--out profiles/multi16_ab.json] [--only LEG[:0|:1]]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)  # 100 steps of ~0.5 ms: 20 made windows of 10 ms, and legs that said nothing
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--run", default="change")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multi16_ab.json"))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    assert os.path.dirname(os.path.abspath(ge.__file__)) == root, ge.__file__
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(41)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half, B, H = 2, a.batch, 544
    K = len(offsets)

    def emb(*shape):
        return torch.randn(shape, generator=gen, device=dev).to(dt)

    def binary(*shape):
        return (torch.rand(shape, generator=gen, device=dev) < 0.6).float()

    def weight(*shape):
        return torch.rand(shape, generator=gen, device=dev) + 0.5

    def downs_2d():
        """down1..down4: packed (target | weight | mask) float thirds, as the reference's provider builds them"""
        out = []
        for j in range(4):
            k, h = nb_half * (4 - j), H >> (j + 1)
            out.append(torch.cat([binary(B, k, h, h), weight(B, k, h, h), binary(B, k, h, h)], dim=1))
        return out

    def leaves():
        return [emb(B, 16, H, H).requires_grad_(True)] + [emb(B, 16, H >> (j + 1), H >> (j + 1)).requires_grad_(True) for j in range(4)]

    def tensor_form(graphed):
        rest = [emb(B, 16, H, H), binary(B, K, H, H), weight(B, K, H, H), binary(B, K, H, H).to(torch.uint8)] + downs_2d()

        def section(batched, *b):
            for x in b[:5]:
                x.grad = None
            loss, pred, _ = pkg.cvppp_loss_section(b[0], list(b[1:5]), b[5], b[6], b[7], b[8], list(b[9:13]), crit, offsets, nb_half,
                                                   batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, leaves() + rest, graphed)

    def labels_form(graphed):
        labels = torch.from_numpy(synth.synth_labels(B, (1, H, H), 43, cell=48)[:, 0]).to(dev)
        downs = [labels[:, ::2 << j, ::2 << j].contiguous() for j in range(4)]  # what the loader's nearest resize hands over
        bufs = leaves() + [emb(B, 16, H, H), labels] + downs

        def section(batched, *b):
            for x in b[:5]:
                x.grad = None
            loss, pred, _ = pkg.cvppp_loss_section_from_labels(b[0], list(b[1:5]), b[5], b[6], None if batched else list(b[7:11]), crit,
                                                               offsets, nb_half, batched=batched)
            pkg.backward(loss)
            return loss, pred
        return _maybe_graphed(pkg, section, bufs, graphed)

    def small2d():
        emds = leaves()[1:]
        downs = downs_2d()
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

    legs = {}
    for g in (False, True):
        sfx = "_graphed" if g else ""
        legs["cvppp_tensor" + sfx] = lambda g=g: tensor_form(g)
        legs["cvppp_labels" + sfx] = lambda g=g: labels_form(g)
    legs["small2d"] = small2d
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
        row = {("batched" if b else "unbatched"): {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v)}
               for b, v in times.items()}
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
    run = {"dtype": a.dtype, "shapes": "%d x 16 x 544^2, K = 10; scales 272^2 / 136^2 / 68^2 / 34^2, K = 8 / 6 / 4 / 2" % B,
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_step": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = json.load(open(a.out)) if os.path.exists(a.out) else {}
        out.setdefault("variants", {"unbatched": "batched=False (per-scale launches)",
                                    "batched": "batched=True (one launch for the four scales each way; the per-scale launches "
                                               "where the library fuses f32 tables only, and for a 16-bit tensor-form table "
                                               "above affinity_op.MULTI16_MAX_TILES)"})
        out.setdefault("runs", {})[a.run] = run
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({a.run: run}, indent=1))


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
