#!/usr/bin/env python3
"""The 3D losses on the activated affinity map at the reference's training shape, 2 x 16 x 18 x 160 x 160, forward plus backward through
the Python API, timed in ONE process with three variants alternating batch by batch:

  A  default switches: the forward is the tile-per-plane cross kernel's PEA_FLAG_LOSS_ACT form where one is dispatched
     (k_fwd_xdma<16, .., ZF, .., LACT, BCE>)
  B  PEA_FWD_XDMA=0 (set_switch): the forwards the library ran for these descriptors before (k_fwd_tiled<.., LACT>, k_fwd_direct)
  C  A captured in a HIP graph (pea.graphed) and replayed

for three calls:

  norm5_wmse      embedding2affs_3d.embedding_loss_norm5 with WeightedMSE
  norm5_wbce      embedding2affs_3d.embedding_loss_norm5 with WeightedBCE
  ema_norm2_wmse  loss_embedding_mse_3d.ema_embedding_loss_norm2 with WeightedMSE (detached second operand)

A batch is `--reps` steps between two HIP events, and every step's forward call between two more; median, fastest and slowest batch
per variant, microseconds per step.  Nothing synchronises the host inside a batch.  The condition per call: A's median lies below B's
by more than the two spreads (slowest - fastest) together.  For the second-operand call PEA_FWD_XDMA=0 also takes the role-A cross
BACKWARD away (pea_cross_supported mode 2 asks for both), which the library before this form did not do: B's step is then not that
library's step, so the call is judged on the forward span (`judged_on`); the step medians are recorded beside it (`step_gain_us`).

The committed profiles/act3d_ab.json was taken with the squared-residual forms (self and second operand) still dispatched: it is the
measurement that switched them off again (EXPERIMENTS.md); on the library as it stands A and B of the two
WeightedMSE calls differ only in what PEA_FWD_XDMA=0 does to them.

  python profiles/act3d_ab.py [--batches 7] [--reps 30] [--warmup 5] [--out profiles/act3d_ab.json]
  python profiles/act3d_ab.py --only A --steps 20          the run for rocprofv3 --kernel-trace --stats (a run of its own per variant)
  python profiles/act3d_ab.py --merge-trace A=DIR --steps 20   add that trace's kernels (calls per step, average us) to the JSON
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SHAPE = (2, 16, 18, 160, 160)
CALLS = ["norm5_wmse", "norm5_wbce", "ema_norm2_wmse"]
VARIANTS = ["A", "B", "C"]
WARM_TRACE = 3  # steps per call the --only run makes before its --steps (all of them are in the trace)


def merge_trace(a):
    variant, d = a.merge_trace.split("=", 1)
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (d, len(paths)))
    steps = a.steps + WARM_TRACE
    rows = [{"kernel": r["Name"][:200], "calls": int(r["Calls"]), "calls_per_step_of_a_call": int(r["Calls"]) / steps,
             "average_us": float(r["AverageNs"]) * 1e-3} for r in csv.DictReader(open(paths[0]))]
    rows.sort(key=lambda r: -r["average_us"] * r["calls"])
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[variant] = {
        "command": "rocprofv3 --kernel-trace --stats -- python profiles/act3d_ab.py --only %s --steps %d" % (variant, a.steps),
        "steps_per_call_in_trace": steps, "calls_traced": CALLS, "kernels": rows}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"][variant], indent=1)[:6000])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--merge-trace")
    ap.add_argument("--shape", type=int, nargs=5, default=list(SHAPE))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act3d_ab.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "act3d_ab.py measures on an MI355X"
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    B, D, Z, Y, X = a.shape
    rng = np.random.default_rng(2025)

    def rand(*shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)

    E = rand(B, D, Z, Y, X).requires_grad_(True)
    EMA = (E.detach() + 0.5 * rand(B, D, Z, Y, X))
    T12 = (torch.from_numpy(rng.random((B, 12, Z, Y, X)).astype(np.float32)).to(dev) < 0.6).float()
    W12 = 0.5 + 1.5 * torch.from_numpy(rng.random((B, 12, Z, Y, X)).astype(np.float32)).to(dev)
    T3, W3 = T12[:, :3].contiguous(), W12[:, :3].contiguous()
    wmse, wbce = pkg.WeightedMSE(), pkg.WeightedBCE()
    set_switch = pkg._lib.set_switch

    def forward(call):
        if call == "norm5_wmse":
            return pkg.embedding2affs_3d.embedding_loss_norm5(E, T12, W12, wmse, affs0_weight=1.0)
        if call == "norm5_wbce":
            return pkg.embedding2affs_3d.embedding_loss_norm5(E, T12, W12, wbce, affs0_weight=1.0)
        return pkg.ema_embedding_loss_norm2(E, EMA, T3, W3, wmse, affs0_weight=1.0, shift=1, fill=True)

    def step(call, events=None):
        E.grad = None
        if events:
            events[0].record()
        loss, affs = forward(call)
        if events:
            events[1].record()
        pkg.backward(loss)
        # detached: a loss kept by the caller keeps its autograd graph -- and E's AccumulateGrad node, bound to the stream of THIS step --
        # alive, and a later capture on another stream (pea.graphed) would meet a node of the default stream
        return loss.detach(), affs, E.grad

    def switches(variant):
        set_switch("PEA_FWD_XDMA", "0" if variant == "B" else None)

    if a.only:  # the profiler's run: nothing but steps of one variant
        switches(a.only)
        if a.only == "C":
            graphs = {c: pkg.graphed(lambda _e, c=c: step(c), E) for c in CALLS}
        for c in CALLS:
            for _ in range(WARM_TRACE + a.steps):
                graphs[c].replay() if a.only == "C" else step(c)
        torch.cuda.synchronize()
        switches("A")
        print("ran %d steps per call of variant %s" % (WARM_TRACE + a.steps, a.only))
        return

    # warm-up and values: every variant of every call; A, B and C compute the same step
    values, graphs = {}, {}
    for c in CALLS:
        values[c] = {}
        for v in ("A", "B"):
            switches(v)
            for _ in range(a.warmup):
                loss, affs, grad = step(c)
            torch.cuda.synchronize()
            values[c][v] = {"loss": float(loss), "grad_abs_max": float(grad.abs().max())}
            if v == "A":
                ga, aa = grad.clone(), affs.clone()
            else:
                values[c]["B_vs_A_grad_rel_max"] = float((grad - ga).abs().max() / ga.abs().max())
                values[c]["B_vs_A_affs_abs_max"] = float((affs - aa).abs().max())
        switches("A")
        graphs[c] = pkg.graphed(lambda _e, c=c: step(c), E, warmup=a.warmup)
        loss, affs, grad = graphs[c].replay()
        torch.cuda.synchronize()
        values[c]["C"] = {"loss": float(loss), "grad_abs_max": float(grad.abs().max())}
        values[c]["C_bit_identical_to_A"] = bool(torch.equal(grad, ga) and torch.equal(affs, aa))

    times = {c: {v: {"step": [], "forward": []} for v in VARIANTS} for c in CALLS}
    for _ in range(a.batches):
        for c in CALLS:
            for v in VARIANTS:
                switches(v)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                evs = []
                t0.record()
                for _ in range(a.reps):
                    if v == "C":
                        graphs[c].replay()
                    else:
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                        step(c, ev)
                        evs.append(ev)
                t1.record()
                torch.cuda.synchronize()
                times[c][v]["step"].append(t0.elapsed_time(t1) * 1e3 / a.reps)
                if evs:
                    times[c][v]["forward"].append(sum(x[0].elapsed_time(x[1]) for x in evs) * 1e3 / a.reps)
    switches("A")

    def row(ts):
        return {"min_us": min(ts), "median_us": statistics.median(ts), "max_us": max(ts), "spread_us": max(ts) - min(ts)} if ts else None

    rows = {c: {v: {k: row(ts) for k, ts in tv.items()} for v, tv in cv.items()} for c, cv in times.items()}
    verdict = {}
    for c in CALLS:
        span = "forward" if c.startswith("ema_") else "step"
        ra, rb = rows[c]["A"][span], rows[c]["B"][span]
        verdict[c] = {"judged_on": span, "gain_us": rb["median_us"] - ra["median_us"], "spreads_together_us": ra["spread_us"] + rb["spread_us"],
                      "A_below_B_by_more_than_the_spreads": bool(rb["median_us"] - ra["median_us"] > ra["spread_us"] + rb["spread_us"]),
                      "step_gain_us": rows[c]["B"]["step"]["median_us"] - rows[c]["A"]["step"]["median_us"],
                      "graphed_over_eager_step": rows[c]["C"]["step"]["median_us"] / rows[c]["A"]["step"]["median_us"]}
    out = {"shape": [B, D, Z, Y, X], "calls": CALLS, "variants": {"A": "default switches", "B": "PEA_FWD_XDMA=0", "C": "A graphed"},
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_step": rows, "condition": verdict,
           "forward_note": "the forward span is the Python call of the loss function between two events: the forward kernel, the loss "
                           "finish, the border launch and the host time between them where the queue runs dry",
           "values": values, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
