#!/usr/bin/env python3
"""The mutex watershed on the device (include/pea_mws.h: pea_mws_segment), timed in ONE process on the three drivers' shapes against
what a caller of seg_mutex had to do before it with an affinity map that is on the device:

  mws         pea.mutex_watershed(affs, offsets, strides, rounds=R) on a device tensor, R = the rounds that the data needs (found once
              with rounds=None): the launches of csrc/pea_k_mws.hip, nothing read back
  mws_auto    the same with rounds=None: batches of 32, 64, .. rounds with one synchronisation each
  mws_graphed the fixed-round call captured with pea.graphed and replayed
  host        device -> host copy of the map, the sequential definition restated in Python (tests/mws_reference.py: the edges sorted by
              key, a union-find, a set of excluded roots per root), the labels copied back.  elf is not installed here, so this is NOT
              elf's time: affogato's loop is compiled code, this one is interpreted.  It says what THIS machine's caller pays.

  cvppp_1x544x544    the 10 offsets of multi_offset([1, 3, 5, 9, 27], 4), strides [5, 5]     (scripts_cvppp/config/cvppp.yaml)
  bbbc_8x256x256     the 10 offsets of multi_offset([1, 3, 5, 9, 11], 4), strides [10, 10]    (scripts_bbbc039v1/config/bbbc039v1.yaml)
  ac3_18x160x160     the 12 norm5 offsets, strides [1, 10, 10], three attractive          (scripts_ac3ac4/inference.py -mutex)

The maps are affinities of Voronoi cells (utils/synth.py synth_membranes) with noise, in two kinds: "cells" = 0.8 * same + 0.1 + 0.1 *
uniform (a trained network's map) and "noisy" = 0.4 * same + 0.6 * uniform (many clusters, many exclusions, a long tail).  The split of
the device time comes from the C ABI with device events: a call with 0 rounds less a resumed call with 0 rounds on the same state (the
set-up), a resumed call with 0 rounds after a complete one (the labelling of the final partition), calls with R / 2 and R rounds (the
rounds, and the time per round in the second half: the tail).  Medians; recorded, not gated.

  python profiles/mws_ab.py [--batches 5] [--reps 5] [--warmup 2] [--out profiles/mws_ab.json] [--only LEG] [--no-host]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/mws_ab.py --trace LEG/KIND --rounds R --steps 10
  python profiles/mws_ab.py --merge-trace DIR --trace LEG/KIND --rounds R --steps 10    (adds the kernels' times per call to the json)"""
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
import __graft_entry__ as ge  # noqa: E402
import mws_reference as R  # noqa: E402

NORM5 = [1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]


def legs(pkg):
    norm5 = [[-s if a == i % 3 else 0 for a in range(3)] for i, s in enumerate(NORM5)]
    return {"cvppp_1x544x544": dict(B=1, dims=(1, 544, 544), offsets=pkg.multi_offset([1, 3, 5, 9, 27], 4), strides=[5, 5], cells=40),
            "bbbc_8x256x256": dict(B=8, dims=(1, 256, 256), offsets=pkg.multi_offset([1, 3, 5, 9, 11], 4), strides=[10, 10], cells=60),
            "ac3_18x160x160": dict(B=1, dims=(18, 160, 160), offsets=norm5, strides=[1, 10, 10], cells=25)}


def make_affs(synth, kw, kind, seed=91):
    """float32 [B, K, Z, Y, X]: every plane has its own Voronoi cells (a volume's planes are cut from one drifting set of sites: the
    cells of plane z are those of plane 0 shifted by z pixels, so that z edges mostly join one cell)"""
    B, (Z, Y, X) = kw["B"], kw["dims"]
    rng = np.random.default_rng(seed)
    _, cells = synth.synth_membranes(B, Y + Z, X + Z, kw["cells"], seed=seed)
    lab = np.stack([np.stack([cells[b, z:z + Y, z:z + X] for z in range(Z)]) for b in range(B)])
    offs = [[0] * (3 - len(o)) + list(o) for o in kw["offsets"]]
    x = np.zeros((B, len(offs), Z, Y, X), np.float32)
    for k, (dz, dy, dx) in enumerate(offs):
        src = lab[:, max(0, -dz):Z - max(0, dz), max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)]
        dst = lab[:, max(0, dz):Z - max(0, -dz), max(0, dy):Y - max(0, -dy), max(0, dx):X - max(0, -dx)]
        x[:, k, max(0, -dz):Z - max(0, dz), max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)] = src == dst
    if kind == "noisy":
        return (0.4 * x + 0.6 * rng.random(x.shape)).astype(np.float32)
    return (0.8 * x + 0.1 + 0.1 * rng.random(x.shape)).astype(np.float32)


def device_split(pkg, X5, kw, rounds, reps):
    """device events around C ABI calls -> microseconds: set-up, labelling, all rounds, a round of the second half"""
    L = pkg._lib.lib()
    d = pkg._lib.PeaMwsDesc()
    d.B, d.K, d.Z, d.Y, d.X = X5.shape
    nd = len(kw["offsets"][0])
    d.n_attractive, d.input = nd, 0
    for k, o in enumerate(kw["offsets"]):
        d.offsets[k][:] = [0] * (3 - nd) + list(o)
    d.strides[:] = [1] * (3 - nd) + list(kw["strides"])
    nb = L.pea_mws_workspace_bytes(ctypes.byref(d))
    dev = X5.device
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    labels = torch.empty((d.B, d.Z, d.Y, d.X), dtype=torch.int32, device=dev)
    counts = torch.empty(d.B, dtype=torch.int32, device=dev)
    stats = torch.empty((d.B, 8), dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(r, flags):
        d.rounds, d.flags = r, flags
        pkg._lib.check(L.pea_mws_segment(ctypes.byref(d), vp(X5), None, vp(labels), vp(counts), vp(stats), vp(ws), nb, None), "pea_mws_segment")

    def timed(r, flags, before=None):
        """the median device time of call(r, flags), each one after call(before, 0) where given: the state that a resumed call finds"""
        t = []
        for _ in range(reps + 1):
            if before is not None:
                call(before, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(r, flags)
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
        return statistics.median(t[1:])

    # the labelling costs what the partition makes it cost (few large clusters: many lanes on one word), so each is timed on its own state
    setup = timed(0, 0) - timed(0, 1, before=0)
    labelling = timed(0, 1, before=rounds)
    th, tr = timed(rounds // 2, 0), timed(rounds, 0)
    half = th - setup - timed(0, 1, before=rounds // 2)
    all_rounds = tr - setup - labelling
    return {"setup_us": setup, "labelling_us": labelling, "rounds_us": all_rounds, "call_us": tr, "rounds": rounds, "launches": 2 + 5 * rounds + 8,
            "us_per_round_first_half": half / max(1, rounds // 2), "us_per_round_second_half": (all_rounds - half) / max(1, rounds - rounds // 2),
            "workspace_bytes": int(nb)}


WARM_TRACE = 2  # calls the --trace run makes before its --steps (all of them are in the trace)


def trace_run(a):
    """what the kernel trace sees: WARM_TRACE + --steps eager calls of one leg with --rounds rounds"""
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    name, kind = a.trace.split("/")
    kw = legs(pkg)[name]
    X5 = torch.from_numpy(make_affs(synth, kw, kind)).to("cuda:0")
    X = X5[:, :, 0] if len(kw["offsets"][0]) == 2 else X5
    for _ in range(WARM_TRACE + a.steps):
        out = pkg.mutex_watershed(X, kw["offsets"], kw["strides"], rounds=a.rounds)
    torch.cuda.synchronize()
    assert int(out.stat("undecided").max()) == 0, "--rounds %d do not complete %s" % (a.rounds, a.trace)


def merge_trace(a):
    """kernel_stats.csv of the traced run -> the kernels' times per call, into the json (a kernel of a round runs once per round, so its
    row is its total over a call: launches per call, microseconds per call and its average)"""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = []
    for r in csv.DictReader(open(paths[0])):
        if "k_mws_" in r["Name"]:
            rows.append({"kernel": r["Name"][:60], "launches_per_call": int(r["Calls"]) / float(calls),
                         "us_per_call": float(r["AverageNs"]) * int(r["Calls"]) * 1e-3 / calls, "average_us": float(r["AverageNs"]) * 1e-3})
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/mws_ab.py --trace %s --rounds %d --steps %d"
                   % (a.trace, a.rounds, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(rows, key=lambda r: -r["us_per_call"]),
        "device_us_per_call": sum(r["us_per_call"] for r in rows)}
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
    ap.add_argument("--rounds", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mws_ab.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "mws_ab.py measures on an MI355X: there is no CPU fallback"
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    rows = {}
    for name, kw, kind in [(n, k, kind) for n, k in legs(pkg).items() for kind in ("cells", "noisy")]:
        if a.only and a.only != name:
            continue
        x = make_affs(synth, kw, kind)
        two_d = len(kw["offsets"][0]) == 2
        X5 = torch.from_numpy(x).to(dev)
        X = X5[:, :, 0] if two_d else X5
        auto = pkg.mutex_watershed(X, kw["offsets"], kw["strides"])
        used = auto.stat("rounds").cpu().numpy()
        rounds = int(used.max()) + 1  # (+ 1: the round that finds nothing left and says so)
        fixed = pkg.mutex_watershed(X, kw["offsets"], kw["strides"], rounds=rounds)
        assert int(fixed.stat("undecided").max()) == 0 and torch.equal(fixed.labels, auto.labels)
        graph = pkg.graphed(lambda X: pkg.mutex_watershed(X, kw["offsets"], kw["strides"], rounds=rounds).labels, X)
        assert torch.equal(graph.replay(), auto.labels)
        steps = {"mws": lambda: pkg.mutex_watershed(X, kw["offsets"], kw["strides"], rounds=rounds),
                 "mws_auto": lambda: pkg.mutex_watershed(X, kw["offsets"], kw["strides"]), "mws_graphed": graph.replay}
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
        row["device_split"] = device_split(pkg, X5, kw, rounds, a.reps)
        st = auto.stats.cpu().numpy()
        row["values"] = {"offsets": len(kw["offsets"]), "strides": kw["strides"], "rounds_used_per_image": used.tolist(), "rounds_enqueued": rounds,
                         "clusters_per_image": auto.counts.cpu().numpy().tolist(), "merges": st[:, 2].tolist(), "exclusions_at_end": st[:, 3].tolist(),
                         "edges": (int(np.prod(x.shape[1:])) - st[:, 4:].sum(1)).tolist()}
        if not a.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = X5.cpu().numpy()
            offs = [[0] * (3 - len(o)) + list(o) for o in kw["offsets"]]
            ref = R.segment(host, offs, len(kw["offsets"][0]), [1] * (3 - len(kw["strides"])) + list(kw["strides"]))[0]
            back = torch.from_numpy(ref).to(dev)
            torch.cuda.synchronize()
            row["host"] = {"us": (time.perf_counter() - t0) * 1e6, "reps": 1}
            row["values"]["labels_equal_host"] = bool(torch.equal(back.reshape(auto.labels.shape), auto.labels))
            row["host_over_mws"] = row["host"]["us"] / row["mws"]["median_us"]
        row["shape"] = list(x.shape)
        rows[name + "/" + kind] = row
        print(name, kind, json.dumps(row), flush=True)
        del graph, X, X5
        torch.cuda.empty_cache()
    out = {"kernel_form": "a lane per edge slot (256 consecutive pixels of an attractive channel or 256 consecutive points of a repulsive channel's stride lattice per workgroup), a state byte per edge, keys recomputed "
                          "from x, five launches a round (best / attractive / repulsive / compress / reinsert), the exclusion table rebuilt "
                          "after every round that merged; no compaction of the surviving edges (csrc/pea_k_mws.hip)",
           "host_path": "device -> host copy, tests/mws_reference.py sequential() (a Python loop over the sorted edges), host -> device copy of "
                        "the labels.  elf is not installed on the measuring machine: this is not elf's time",
           "timing": "host clock around calls that end in a device synchronise, medians over alternating batches; device_split: device "
                     "events around C ABI calls, medians",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
