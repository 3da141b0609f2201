#!/usr/bin/env python3
"""The small-segment merges on the device (include/pea_merge.h: pea_merge_small), timed in ONE process against what the validation
loops do today with a label image that is on the device:

  merge        pea.merge_small_objects(labels, passes, relabel=True, max_id=Y * X): nothing read back (the resident chain's call; the id
               space is the bound that is known without looking at the data, one id per pixel)
  merge_tight  the same with max_id = the largest id that occurs (known here; max_id=None would read it back)
  merge_graphed  the first captured with pea.graphed and replayed
  host         device -> host copy of the labels, the reference's op sequence restated in numpy (tests/merge_reference.py chain(): np.unique
               per pass and per crop, seg[seg == i] = target over the whole image per merge) and its relabel, the copy back

  cvppp_1x544x544   CVPPP passes (5, 5), (20, 11), (50, 11), (300, 21)
  bbbc_1x520x696    BBBC039V1 passes (5, 5), (25, 11), (50, 11), (100, 21)
  bbbc_8x256x256    the same passes

The inputs are mutex-watershed outputs of the synthetic cell maps of profiles/mws_ab.py, of the trained-like kind ("cells") and of the
noisy kind.  Recorded per leg: candidates and merges per pass (the passes run one call each for this, and their chain equals the fused
call), the device time of the call by device events, of the same call with every threshold 0 (moments, the walk's scans over the ids,
the finish: no candidate) and their difference per candidate.  Medians; recorded, not gated.

  python profiles/merge_ab.py [--batches 5] [--reps 5] [--warmup 2] [--out profiles/merge_ab.json] [--only LEG] [--no-host]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/merge_ab.py --trace LEG/KIND --steps 10
  python profiles/merge_ab.py --merge-trace DIR --trace LEG/KIND --steps 10    (adds the kernels' times per call to the json)"""
import argparse
import csv
import ctypes
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as ge  # noqa: E402
import merge_reference as R  # noqa: E402
import mws_ab  # noqa: E402

WARM_TRACE = 2


def legs(pkg):
    bbbc = pkg.multi_offset([1, 3, 5, 9, 11], 4)
    return {"cvppp_1x544x544": dict(B=1, dims=(1, 544, 544), offsets=pkg.multi_offset([1, 3, 5, 9, 27], 4), strides=[5, 5], cells=40, passes=R.CVPPP_MERGE_PASSES),
            "bbbc_1x520x696": dict(B=1, dims=(1, 520, 696), offsets=bbbc, strides=[10, 10], cells=80, passes=R.BBBC_MERGE_PASSES),
            "bbbc_8x256x256": dict(B=8, dims=(1, 256, 256), offsets=bbbc, strides=[10, 10], cells=60, passes=R.BBBC_MERGE_PASSES)}


def labels_of(pkg, synth, kw, kind, dev):
    """the mutex watershed of the leg's synthetic map: int32 [B, Y, X] on the device"""
    x = torch.from_numpy(mws_ab.make_affs(synth, kw, kind)).to(dev)
    return pkg.mutex_watershed(x[:, :, 0], kw["offsets"], kw["strides"]).labels.contiguous()


def device_times(pkg, labels, passes, max_id, reps):
    """device events around C ABI calls -> microseconds: the call, and the same call with every threshold 0"""
    L = pkg._lib.lib()
    d = pkg._lib.PeaMergeDesc()
    d.B, d.Y, d.X = labels.shape
    d.max_id, d.n_passes, d.flags = max_id, len(passes), pkg._lib.MERGE_RELABEL
    for k, (t, w) in enumerate(passes):
        d.threshold[k], d.window[k] = t, w
    nb = L.pea_merge_workspace_bytes(ctypes.byref(d))
    assert nb > 0
    dev = labels.device
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    out = torch.empty_like(labels)
    counts = torch.empty(d.B, dtype=torch.int32, device=dev)
    stats = torch.empty((d.B, 8), dtype=torch.int64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def timed(zero):
        for k, (t, w) in enumerate(passes):
            d.threshold[k], d.window[k] = (0 if zero else t), w
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pkg._lib.check(L.pea_merge_small(ctypes.byref(d), vp(labels), vp(out), vp(counts), vp(stats), vp(ws), nb, None), "pea_merge_small")
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts[1:])

    full, zero = timed(False), timed(True)
    return {"call_us": full, "no_candidate_us": zero, "workspace_bytes": int(nb)}


def trace_run(a):
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    name, kind = a.trace.split("/")
    kw = legs(pkg)[name]
    labels = labels_of(pkg, synth, kw, kind, torch.device("cuda:0"))
    S = int(labels.shape[-2] * labels.shape[-1])
    for _ in range(WARM_TRACE + a.steps):
        pkg.merge_small_objects(labels, kw["passes"], relabel=True, max_id=S)
    torch.cuda.synchronize()


def merge_trace(a):
    """kernel_stats.csv of the traced run -> the kernels' times per call, into the json"""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = []
    for r in csv.DictReader(open(paths[0])):
        if "k_merge_" in r["Name"]:
            rows.append({"kernel": r["Name"][:60], "launches_per_call": int(r["Calls"]) / float(calls),
                         "us_per_call": float(r["AverageNs"]) * int(r["Calls"]) * 1e-3 / calls})
    part = lambda names: sum(r["us_per_call"] for r in rows if any(n in r["kernel"] for n in names))
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/merge_ab.py --trace %s --steps %d" % (a.trace, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(rows, key=lambda r: -r["us_per_call"]),
        "moments_us": part(("k_merge_init", "k_merge_moments")), "walk_us": part(("k_merge_walk",)),
        "finish_us": part(("k_merge_totals", "k_merge_scan", "k_merge_rank", "k_merge_map", "k_merge_project"))}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"][a.trace], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only")
    ap.add_argument("--trace")
    ap.add_argument("--merge-trace")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_ab.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "merge_ab.py measures on an MI355X: there is no CPU fallback"
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    rows = {}
    for name, kw, kind in [(n, k, kind) for n, k in legs(pkg).items() for kind in ("cells", "noisy")]:
        if a.only and a.only != name:
            continue
        labels = labels_of(pkg, synth, kw, kind, dev)
        passes = kw["passes"]
        S = int(labels.shape[-2] * labels.shape[-1])
        top = int(labels.max())
        fused = pkg.merge_small_objects(labels, passes, relabel=True, max_id=S)
        tight = pkg.merge_small_objects(labels, passes, relabel=True, max_id=top)
        assert torch.equal(fused.labels, tight.labels) and torch.equal(fused.stats, tight.stats) and int(fused.stat("out_of_range").max()) == 0
        per_pass, cur = [], labels
        for p in passes:  # one call per pass: its own counters; the chain of the calls is the fused call
            one = pkg.merge_small_objects(cur, (p,), max_id=S)
            per_pass.append({"threshold": p[0], "window": p[1], "candidates": one.stat("candidates").tolist(), "merges": one.stat("merges").tolist(),
                             "negative": one.stat("negative").tolist(), "few": one.stat("few").tolist()})
            cur = one.labels
        assert torch.equal(pkg.merge_small_objects(cur, ((0, 1),), relabel=True, max_id=S).labels, fused.labels)
        graph = pkg.graphed(lambda x: pkg.merge_small_objects(x, passes, relabel=True, max_id=S).labels, labels)
        assert torch.equal(graph.replay(), fused.labels)
        steps = {"merge": lambda: pkg.merge_small_objects(labels, passes, relabel=True, max_id=S),
                 "merge_tight": lambda: pkg.merge_small_objects(labels, passes, relabel=True, max_id=top), "merge_graphed": graph.replay}
        for f in steps.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {v: [] for v in steps}
        for _ in range(a.batches):
            for v, f in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    f()
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / a.reps)
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        cands = int(fused.stat("candidates").sum())
        for key, mid in (("device", S), ("device_tight", top)):
            dt = device_times(pkg, labels, passes, mid, a.reps)
            dt["us_per_candidate"] = (dt["call_us"] - dt["no_candidate_us"]) / max(1, cands)
            row[key] = dt
        row["values"] = {"ids_in": top, "max_id": S, "ids_left_per_image": fused.counts.tolist(), "candidates": cands, "merges": int(fused.stat("merges").sum()),
                         "longest_chain": int(fused.stat("chain").max()), "per_pass": per_pass}
        if not a.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = labels.cpu().numpy()
            ref = np.stack([R.relabel(R.chain(h, passes))[0] for h in host]).astype(np.int32)
            back = torch.from_numpy(ref).to(dev)
            torch.cuda.synchronize()
            row["host"] = {"us": (time.perf_counter() - t0) * 1e6, "reps": 1}
            row["values"]["labels_equal_host"] = bool(torch.equal(back, fused.labels))
            row["host_over_merge"] = row["host"]["us"] / row["merge"]["median_us"]
        row["shape"] = list(labels.shape)
        rows[name + "/" + kind] = row
        print(name, kind, json.dumps(row), flush=True)
        del graph
        torch.cuda.empty_cache()
    out = {"kernel_form": "moments by a peeled streaming pass with integer atomics; one workgroup per image walks the ids in chunks of 256, a "
                          "ballot picks the candidates, each a crop counted into an LDS table and three 64-bit maxima; a three-step scan and one "
                          "streaming projection (csrc/pea_k_merge.hip)",
           "host_path": "device -> host copy, tests/merge_reference.py chain() and relabel() (the reference's op sequence in numpy with a stable "
                        "argsort), host -> device copy of the labels",
           "timing": "host clock around calls that end in a device synchronise, medians over alternating batches; device: device events "
                     "around C ABI calls, medians; no_candidate_us: the same call with every threshold 0",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
