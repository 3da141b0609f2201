#!/usr/bin/env python3
"""The watershed fragments (include/pea_ws.h: pea_ws_seeds, pea_ws_flood), timed in ONE process against what a caller of mc_baseline
had to do before them with a boundary map that is on the device:

  ws          pea.distance_transform_watershed(boundary, .25, 2.) on a device tensor (elf's defaults: sigma_weights 2, min_size 100,
              alpha .9; ids stacked over the planes): the launches of csrc/pea_k_ws.hip and the two labellings of csrc/pea_k_cc.hip;
              everything stays on the device
  ws_graphed  the same call captured with pea.graphed and replayed
  host        device -> host copy of the boundary map, the numpy / scipy restatement of the same chain (tests/ws_reference.py:
              scipy.ndimage.distance_transform_edt and gaussian_filter, plateau maxima by scipy.ndimage.label, Kruskal in Python), the
              fragments copied back.  Neither elf nor vigra is installed here, so the restatement stands in for them: its flood is a
              Python loop over the sorted edges, where vigra's is compiled code -- the host figure says what THIS machine's caller
              pays, not what elf would.  On the largest shape the host chain runs on --host-planes planes only and is scaled to all.

on three shapes of synthetic membranes (utils/synth.py synth_membranes: Voronoi cell walls with two-pixel gaps and a little noise):
1 x 520 x 696, 18 x 160 x 160 and 100 x 1024 x 1024 (four distinct planes, repeated).

Every call is timed by a host clock around work that ends in a device synchronise.  After warm-up the device variants alternate batch
by batch; a batch times `--reps` calls; min, median and max of the batches in microseconds per call.  The host chain is timed
--host-reps times.  Recorded, not gated.  The launches' shares of the device time come from a kernel trace, a run of its own:

  python profiles/ws_ab.py [--batches 5] [--reps 5] [--warmup 2] [--out profiles/ws_ab.json] [--only LEG] [--no-host]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/ws_ab.py --trace LEG --steps 10
  python profiles/ws_ab.py --merge-trace DIR --trace LEG --steps 10     (adds the kernels' average times to the json)"""
import argparse
import csv
import glob
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
import ws_reference as R  # noqa: E402

THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, MIN_SIZE, ALPHA = .25, 2., 2., 100, .9
LEGS = {"bbbc_1x520x696": dict(shape=(1, 520, 696), cells=150, distinct=1),
        "ac3_18x160x160": dict(shape=(18, 160, 160), cells=20, distinct=18),
        "ac3_100x1024x1024": dict(shape=(100, 1024, 1024), cells=400, distinct=4)}


def make_boundary(synth, name):
    kw = LEGS[name]
    N, Y, X = kw["shape"]
    b, _ = synth.synth_membranes(kw["distinct"], Y, X, kw["cells"], seed=71, gap=2, gaps_per_plane=max(6, kw["cells"] // 4), noise=0.1)
    return np.ascontiguousarray(np.tile(b, (N // kw["distinct"], 1, 1)))


def host_chain(b):
    """[n, Y, X] float32 on the host -> the fragments, int32, ids stacked"""
    return R.chain_reference(b, THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, MIN_SIZE, ALPHA)


def make_leg(pkg, B):
    graph = []

    def step(variant):
        if variant == "ws":
            return pkg.distance_transform_watershed(B, THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, MIN_SIZE, ALPHA)[0]
        if not graph:
            graph.append(pkg.graphed(lambda B: pkg.distance_transform_watershed(B, THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, MIN_SIZE, ALPHA), B))
        return graph[0].replay()[0]
    return step


WARM_TRACE = 2  # calls the --trace run makes before its --steps (all of them are in the trace)


def trace_run(a):
    """what the kernel trace sees: WARM_TRACE + --steps eager calls of one leg"""
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    step = make_leg(pkg, torch.from_numpy(make_boundary(synth, a.trace)).to("cuda:0"))
    for _ in range(WARM_TRACE + a.steps):
        step("ws")
    torch.cuda.synchronize()


def merge_trace(a):
    """kernel_stats.csv of the traced run -> the kernels' times per call, into the json.  A kernel of the flood runs once per round and
    flood, so its row is its total over a call: launches per call and microseconds per call."""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = []
    for r in csv.DictReader(open(paths[0])):
        if "k_ws_" in r["Name"] or "k_cc_" in r["Name"]:
            rows.append({"kernel": r["Name"][:100], "launches_per_call": int(r["Calls"]) / float(calls),
                         "us_per_call": float(r["AverageNs"]) * int(r["Calls"]) * 1e-3 / calls, "average_us": float(r["AverageNs"]) * 1e-3})
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/ws_ab.py --trace %s --steps %d" % (a.trace, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(rows, key=lambda r: -r["us_per_call"]),
        "device_us_per_call": sum(r["us_per_call"] for r in rows)}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"][a.trace], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-planes", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only")
    ap.add_argument("--trace")
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ws_ab.json"))
    a = ap.parse_args()
    for name in (a.only, a.trace):
        if name and name not in LEGS:
            raise SystemExit("unknown leg %r (one of %s)" % (name, ", ".join(LEGS)))
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "ws_ab.py measures on an MI355X: there is no CPU fallback"
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    variants = ["ws", "ws_graphed"]
    rows = {}
    for name, kw in LEGS.items():
        if a.only and a.only != name:
            continue
        b = make_boundary(synth, name)
        assert b.shape == kw["shape"]
        B = torch.from_numpy(b).to(dev)
        step = make_leg(pkg, B)
        s = pkg.watershed_seeds(B, THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, ALPHA)
        w = pkg.seeded_watershed(s.hmap, s.seeds, min_size=MIN_SIZE, stack_ids=True)
        rounds = w.stats[:, 0].cpu().numpy()
        N, Y, X = b.shape
        values = {"threshold": THRESHOLD, "sigma_seeds": SIGMA_SEEDS, "sigma_weights": SIGMA_WEIGHTS, "min_size": MIN_SIZE, "alpha": ALPHA,
                  "boundary_share": float((b > THRESHOLD).mean()), "distinct_planes": kw["distinct"],
                  "seeds_per_plane_median": float(np.median(s.counts.cpu().numpy())),
                  "fragments_found": int(w.counts[:, 0].sum()), "fragments_kept": int(w.counts[:, 1].sum()),
                  "rounds_enqueued_per_flood": int(np.ceil(np.log2(Y * X))) + 1,
                  "rounds_used_last_flood_per_plane": {"min": int(rounds.min()), "median": float(np.median(rounds)), "max": int(rounds.max())},
                  "pixels_left_0": int(w.stats[:, 1].sum())}
        del s, w
        for v in variants:
            for _ in range(a.warmup):
                step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.batches):
            for v in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    step(v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / a.reps)
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        if not a.no_host:
            planes = N if N * Y * X <= 18 * 160 * 160 * 2 else min(N, a.host_planes)
            t = []
            for _ in range(a.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = B[:planes].cpu().numpy()
                frag = torch.from_numpy(host_chain(host)).to(dev)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e6 * (N / float(planes)))
            dev_frag = pkg.distance_transform_watershed(B[:planes].contiguous(), THRESHOLD, SIGMA_SEEDS, SIGMA_WEIGHTS, MIN_SIZE, ALPHA)[0]
            row["host"] = {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t), "planes_run": planes,
                           "scaled_by": N / float(planes), "reps": a.host_reps}
            # the restatement smooths in float64 and the device in float32, so a plateau of dts can come out differently and a seed more or
            # fewer shifts every later id of the stacked numbering: this share says little beyond 1.0; recorded, not asserted (the GPU
            # tests compare stage by stage on the device's own intermediates, bit for bit)
            values["share_of_pixels_equal_host_chain"] = float((dev_frag == frag).float().mean())
            row["host_over_ws"] = row["host"]["median_us"] / row["ws"]["median_us"]
            row["host_over_ws_graphed"] = row["host"]["median_us"] / row["ws_graphed"]["median_us"]
        row.update(shape=list(b.shape), values=values)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step, B
        torch.cuda.empty_cache()
    out = {"kernel_form": "row scan and column walk for the exact squared distance, two separable Gaussians through LDS, plateau maxima on "
                          "the union-find of pea_cc_label, Boruvka rounds of pick (64-bit atomicMin per tree) / hook / compress for the "
                          "flood, run twice where min_size > 1 (csrc/pea_k_ws.hip)",
           "host_path": "device -> host copy, tests/ws_reference.py (scipy.ndimage distance_transform_edt, gaussian_filter, label; Kruskal "
                        "in Python), host -> device copy of the fragments.  Neither elf nor vigra is installed on the measuring machine: "
                        "the restatement stands in for elf's distance_transform_watershed and is slower than compiled vigra would be",
           "timing": "host clock around calls that end in a device synchronise; medians over alternating batches",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
