#!/usr/bin/env python3
"""loss_embedding.embedding_loss with WeightedBCE (`loss_func: WeightedBCELoss`), forward plus backward, at B = 8, D = 16, 544^2, K = 10,
timed in ONE process through the Python API, three variants alternating batch by batch:

  fused_wbce     one forward launch with PEA_FLAG_LOSS_ACT | PEA_FLAG_LOSS_BCE, one loss finish, one backward launch
  composed_wbce  the path every criterion but WeightedMSE took before: one AffinityMap launch for the raw map, K chains of torch ops
                 (activate, mask, F.binary_cross_entropy) under autograd, the map's vjp (loss/_activated.py _foreign_criterion)
  fused_wmse     the same module with WeightedMSE (PEA_FLAG_LOSS_ACT): the same kernels with the squared residual in the epilogue --
                 the same bytes moved, so the difference to fused_wbce is what two logf-class calls per term cost

A batch times `--reps` steps, each between two HIP events of its own, and the forward call alone between two more; min, median and
max over the batches, microseconds per step.  Nothing synchronises the host inside a batch.

  python profiles/bce_ab.py [--batches 7] [--reps 10] [--warmup 3] [--out profiles/bce_ab.json]
  python profiles/bce_ab.py --only fused_wbce --steps 20            the run for rocprofv3 --kernel-trace --stats (a run of its own)
  python profiles/bce_ab.py --merge-trace DIR --steps 20            add the launch counts per step of that trace to the JSON
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

VARIANTS = ["fused_wbce", "composed_wbce", "fused_wmse"]
WARM_TRACE = 3  # steps the --only run makes before its --steps (all of them are in the trace)


def merge_trace(a):
    """kernel_stats.csv of `rocprofv3 --kernel-trace --stats -- python profiles/bce_ab.py --only fused_wbce --steps N` -> launches per step"""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    steps = a.steps + WARM_TRACE
    rows = []
    for r in csv.DictReader(open(paths[0])):
        rows.append({"kernel": r["Name"][:160], "calls": int(r["Calls"]), "calls_per_step": int(r["Calls"]) / steps,
                     "average_us": float(r["AverageNs"]) * 1e-3})
    rows.sort(key=lambda r: -r["calls"])
    per_step = [r for r in rows if r["calls"] >= steps]
    doc = json.load(open(a.out))
    doc["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python profiles/bce_ab.py --only fused_wbce --steps %d" % a.steps,
                           "steps_in_trace": steps, "kernels_launched_every_step": per_step,
                           "other_kernels": [r for r in rows if r["calls"] < steps],
                           "launches_per_step": sum(r["calls"] for r in per_step) / steps}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bce_ab.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    pkg = ge.load_package()
    import importlib
    act = importlib.import_module(ge.PKG_NAME + ".loss._activated")
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    B, D, H, W = 8, 16, 544, 544
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], neighbor=4)
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, 2024)
    E = torch.from_numpy(e).to(dev).requires_grad_(True)
    T, Wt, M = torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(m).to(dev)
    wbce, wmse = pkg.WeightedBCE(), pkg.WeightedMSE()
    lam = [1.0] * len(offsets)

    def forward(variant):
        if variant == "fused_wbce":
            return pkg.loss_embedding.embedding_loss(E, T, Wt, M, wbce, offsets)
        if variant == "fused_wmse":
            return pkg.loss_embedding.embedding_loss(E, T, Wt, M, wmse, offsets)
        return act._foreign_criterion(E, None, T, Wt, M, wbce, offsets, lam, 1e-6, act.HALF_CLAMP)

    def step(variant, events=None):
        E.grad = None
        if events:
            events[0].record()
        loss, _ = forward(variant)
        if events:
            events[1].record()
        loss.backward()
        if events:
            events[2].record()
        return loss

    if a.only:  # the profiler's run: nothing but steps of one variant
        for _ in range(WARM_TRACE + a.steps):
            step(a.only)
        torch.cuda.synchronize()
        print("ran %d steps of %s" % (WARM_TRACE + a.steps, a.only))
        return

    values = {}
    for v in VARIANTS:
        for _ in range(a.warmup):
            loss = step(v)
        torch.cuda.synchronize()
        values[v] = {"loss": float(loss), "grad_abs_max": float(E.grad.abs().max())}
    g_f = None
    step("fused_wbce"); g_f = E.grad.clone()
    step("composed_wbce")
    values["fused_vs_composed_grad_rel_max"] = float((g_f - E.grad).abs().max() / E.grad.abs().max())
    torch.cuda.synchronize()

    times = {v: {"step": [], "forward": []} for v in VARIANTS}
    for _ in range(a.batches):
        for v in VARIANTS:
            evs = []
            for _ in range(a.reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                step(v, ev)
                evs.append(ev)
            torch.cuda.synchronize()
            times[v]["step"].append(sum(x[0].elapsed_time(x[2]) for x in evs) * 1e3 / a.reps)
            times[v]["forward"].append(sum(x[0].elapsed_time(x[1]) for x in evs) * 1e3 / a.reps)
    rows = {v: {k: {"min_us": min(ts), "median_us": statistics.median(ts), "max_us": max(ts)} for k, ts in tv.items()}
            for v, tv in times.items()}
    med = lambda v, k: rows[v][k]["median_us"]
    spread = lambda v, k: rows[v][k]["max_us"] - rows[v][k]["min_us"]
    gain = med("composed_wbce", "step") - med("fused_wbce", "step")
    out = {"shape": [B, D, H, W], "K": len(offsets), "module": "loss_embedding.embedding_loss, forward + backward",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_step": rows,
           "composed_over_fused_step": med("composed_wbce", "step") / med("fused_wbce", "step"),
           "fused_faster_than_composed_beyond_spread": bool(gain > max(spread("composed_wbce", "step"), spread("fused_wbce", "step"))),
           "fused_wbce_over_fused_wmse_forward": med("fused_wbce", "forward") / med("fused_wmse", "forward"),
           "fused_wbce_over_fused_wmse_step": med("fused_wbce", "step") / med("fused_wmse", "step"),
           "forward_note": "the forward span is the Python call of embedding_loss between two events: the forward kernel, the loss "
                           "finish and the host time between them where the queue runs dry",
           "values": values, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
