#!/usr/bin/env python3
"""The region adjacency graph with affinity and boundary statistics (include/pea_rag.h: pea_rag_build), timed in ONE process against two
baselines that are stated here and are no part of the package:

  rag          pea.region_adjacency(fragments, affs, offsets, boundary, one_minus=True, max_id=, capacity=, max_edges=) on device tensors:
               the eight launches of csrc/pea_k_rag.hip; the tables stay on the device
  rag_graphed  `rag` captured with pea.graphed and replayed (not at the full volume: the capture would hold a second set of tables)
  torch        (a) the same table from a torch composition on the device: pair codes of the three axes, torch.unique(return_inverse),
               index_add_ of sizes and boundary sums, searchsorted + index_add_ / scatter_reduce_ of count, sum, min, max per channel
  host         (b) the numpy restatement tests/rag_reference.py on the host, including the copy of the affinity map, the boundary map
               and the fragments to the host

on three shapes: one 520 x 696 image with about 150 cells over an over-segmentation into 12 x 12 blocks (2 in-plane offsets and a
long-range pair), 2 x 18 x 160 x 160 (balls over stacked 10 x 10 blocks, the three local offsets), and one 100 x 1024 x 1024 volume of
stacked 2D fragments (jittered 32 x 32 blocks) with the three local offsets, made on the device from a seed.

Every call is timed by a host clock around work that ends in a device synchronise.  After warm-up the variants alternate batch by batch;
min, median and max of the batches in microseconds per call.  Recorded, not gated.  The launches' shares of the device time come from a
kernel trace, a run of its own:

  python profiles/rag_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/rag_ab.json] [--only LEG]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/rag_ab.py --trace LEG --steps 20
  python profiles/rag_ab.py --merge-trace DIR --trace LEG --steps 20     (adds the kernels' average times to the json)"""
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
from rag_reference import mean_bound, rag_reference  # noqa: E402

LOCAL3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
LEGS = {"cells_1x520x696": dict(shape=(1, 520, 696), offsets=[[0, -1, 0], [0, 0, -1], [0, -9, 0], [0, 0, -9]], capacity=1 << 14, reps=1.0),
        "vol_2x18x160x160": dict(shape=(2, 18, 160, 160), offsets=LOCAL3, capacity=1 << 16, reps=1.0),
        "vol_1x100x1024x1024": dict(shape=(1, 100, 1024, 1024), offsets=LOCAL3, capacity=1 << 21, reps=0.1)}


def relabel(*keys):
    """consecutive ids 0 .. n - 1 of the distinct key tuples"""
    code = np.zeros(keys[0].shape, np.int64)
    for k in keys:
        code = code * (int(k.max()) + 1) + k
    return np.unique(code, return_inverse=True)[1].reshape(keys[0].shape).astype(np.int32)


def make_inputs(synth, name, dev):
    """-> (fragments int32 [B, Z, Y, X], affs f32 [B, K, Z, Y, X], boundary f32 [B, Z, Y, X]) on the device"""
    B, Z, Y, X = (1,) + LEGS[name]["shape"] if len(LEGS[name]["shape"]) == 3 else LEGS[name]["shape"]
    K = len(LEGS[name]["offsets"])
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    if name == "cells_1x520x696":
        cells = synth.synth_nuclei(1, Y, X, 150, 14, 39).astype(np.int64)[:, None]
        yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
        frag = relabel(cells, np.broadcast_to(yy // 12, cells.shape), np.broadcast_to(xx // 12, cells.shape))
        F = torch.from_numpy(frag).to(dev)
    elif name == "vol_2x18x160x160":
        rng = np.random.default_rng(43)
        zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
        vols = []
        for b in range(B):
            ball = np.zeros((Z, Y, X), np.int64)
            for i, (cz, cy, cx, r) in enumerate(zip(rng.integers(0, Z, 60), rng.integers(0, Y, 60), rng.integers(0, X, 60), rng.integers(5, 10, 60))):
                ball[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
            vols.append(relabel(ball, zz, yy // 10, xx // 10))
        F = torch.from_numpy(np.stack(vols)).to(dev)
    else:  # stacked 2D fragments: jittered 32 x 32 blocks, every plane its own ids
        z = torch.arange(Z, device=dev).view(Z, 1, 1)
        y = torch.arange(Y, device=dev).view(1, Y, 1)
        x = torch.arange(X, device=dev).view(1, 1, X)
        by = (y + 5 * (z % 7)) // 32
        bx = (x + 3 * (by % 5) + 11 * (z % 3)) // 32
        nby, nbx = int(by.max()) + 1, int(bx.max()) + 1
        F = ((z * nby + by) * nbx + bx).to(torch.int32)[None].contiguous()
    A = torch.rand((B, K, Z, Y, X), generator=g, device=dev)
    Bd = torch.maximum(1 - A[:, 1], 1 - A[:, 2]) if K >= 3 else torch.maximum(1 - A[:, 0], 1 - A[:, 1])
    return F, A, Bd.contiguous()


def torch_table(F, A, offsets, Bd):
    """baseline (a), one image [Z, Y, X]: -> (uv int64 [n, 2], size, bsum f64, count, sum f64, min, max) on the device"""
    M = int(F.max()) + 1
    f = F.to(torch.int64)
    codes, bterm = [], []
    for axis in range(3):
        if f.shape[axis] < 2:
            continue
        p, q = f.narrow(axis, 0, f.shape[axis] - 1), f.narrow(axis, 1, f.shape[axis] - 1)
        m = p != q
        codes.append((torch.minimum(p, q) * M + torch.maximum(p, q))[m])
        bterm.append((Bd.narrow(axis, 0, f.shape[axis] - 1)[m].double() + Bd.narrow(axis, 1, f.shape[axis] - 1)[m].double()))
    codes = torch.cat(codes)
    edges, inv = torch.unique(codes, return_inverse=True)
    n = edges.numel()
    size = torch.zeros(n, dtype=torch.int64, device=F.device).index_add_(0, inv, torch.ones_like(inv))
    bsum = torch.zeros(n, dtype=torch.float64, device=F.device).index_add_(0, inv, torch.cat(bterm))
    count = torch.zeros(n, dtype=torch.int64, device=F.device)
    ssum = torch.zeros(n, dtype=torch.float64, device=F.device)
    mn = torch.full((n,), float("inf"), device=F.device)
    mx = torch.full((n,), float("-inf"), device=F.device)
    for k, off in enumerate(offsets):
        ps, qs = f, f
        a = A[k]
        for axis, o in enumerate(off):
            L = f.shape[axis]
            if abs(o) >= L:
                ps = None
                break
            ps, a = ps.narrow(axis, max(0, -o), L - abs(o)), a.narrow(axis, max(0, -o), L - abs(o))
            qs = qs.narrow(axis, max(0, o), L - abs(o))
        if ps is None:
            continue
        m = ps != qs
        c = (torch.minimum(ps, qs) * M + torch.maximum(ps, qs))[m]
        x = 1 - a[m]
        i = torch.searchsorted(edges, c).clamp_(max=n - 1)
        hit = edges[i] == c
        i, x = i[hit], x[hit]
        count.index_add_(0, i, torch.ones_like(i))
        ssum.index_add_(0, i, x.double())
        mn.scatter_reduce_(0, i, x, "amin")
        mx.scatter_reduce_(0, i, x, "amax")
    return torch.stack([edges // M, edges % M], 1), size, bsum, count, ssum, mn, mx


def make_leg(pkg, name, F, A, Bd):
    kw = LEGS[name]
    three = len(kw["shape"]) == 3
    offs_py = [o[1:] for o in kw["offsets"]] if three else kw["offsets"]
    Fp, Ap, Bp = (F[:, 0], A[:, :, 0], Bd[:, 0]) if three else (F, A, Bd)
    M = int(F.max())
    graph = []

    def rag(Fp, Ap, Bp):
        return pkg.region_adjacency(Fp, Ap, offs_py, Bp, one_minus=True, max_id=M, capacity=kw["capacity"], max_edges=kw["capacity"] // 2, batched=True)

    def step(variant):
        if variant == "rag":
            return rag(Fp, Ap, Bp)
        if variant == "rag_graphed":
            if not graph:
                graph.append(pkg.graphed(lambda f, a, b: tuple(v for v in rag(f, a, b).tensors.values()), Fp, Ap, Bp))
            return graph[0].replay()
        if variant == "torch":
            return [torch_table(F[b], A[b], kw["offsets"], Bd[b]) for b in range(F.shape[0])]
        f, a, bd = F.cpu().numpy(), A.cpu().numpy(), Bd.cpu().numpy()
        return [rag_reference(f[b], a[b], kw["offsets"], bd[b], max_id=M, one_minus=True) for b in range(f.shape[0])]
    return step


WARM_TRACE = 2


def trace_run(a):
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    step = make_leg(pkg, a.trace, *make_inputs(synth, a.trace, dev))
    for _ in range(WARM_TRACE + a.steps):
        step("rag")
    torch.cuda.synchronize()


def merge_trace(a):
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = [{"kernel": r["Name"][:100], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) * 1e-3} for r in csv.DictReader(open(paths[0]))]
    per_call = [r for r in rows if r["calls"] == calls and "k_rag_" in r["kernel"]]
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/rag_ab.py --trace %s --steps %d" % (a.trace, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(per_call, key=lambda r: -r["average_us"]),
        "device_us_per_call": sum(r["average_us"] for r in per_call)}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"][a.trace], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only")
    ap.add_argument("--trace")
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rag_ab.json"))
    a = ap.parse_args()
    for name in (a.only, a.trace):
        if name and name not in LEGS:
            raise SystemExit("unknown leg %r (one of %s)" % (name, ", ".join(LEGS)))
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "rag_ab.py measures on an MI355X: there is no CPU fallback"
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    rows = json.load(open(a.out)).get("us_per_call", {}) if a.only and os.path.exists(a.out) else {}
    for name, kw in LEGS.items():
        if a.only and a.only != name:
            continue
        full = name == "vol_1x100x1024x1024"
        F, A, Bd = make_inputs(synth, name, dev)
        step = make_leg(pkg, name, F, A, Bd)
        variants = ["rag", "torch", "host"] if full else ["rag", "rag_graphed", "torch", "host"]
        reps = {v: max(1, int(a.reps * kw["reps"])) for v in variants}
        reps["host"] = 1 if full else max(1, a.reps // 10)
        reps["torch"] = max(1, reps["torch"] // 4)
        batches = {v: a.batches for v in variants}
        if full:
            batches["host"] = 0  # timed once, by the call whose result is compared above
        # the three tables agree (the reference on the first image only where it takes long)
        rag = step("rag")
        tt_ = step("torch")
        n = rag.n_edges
        values = {"edges_per_image": n, "stats": rag.stats, "n_nodes": rag.n_nodes,
                  "uv_equal_torch": all(bool(np.array_equal(rag.uv[b], tt_[b][0].cpu().numpy())) for b in range(len(n))),
                  "sizes_equal_torch": all(bool(np.array_equal(rag.sizes[b], tt_[b][1].cpu().numpy())) for b in range(len(n))),
                  "counts_equal_torch": all(bool(np.array_equal(rag.counts[b], tt_[b][3].cpu().numpy())) for b in range(len(n))),
                  "min_max_equal_torch": all(bool(np.array_equal(rag.min[b], tt_[b][5].cpu().numpy()) and np.array_equal(rag.max[b], tt_[b][6].cpu().numpy()))
                                             for b in range(len(n)))}
        del tt_
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = step("host")
        host_once = (time.perf_counter() - t0) * 1e6
        values["equal_host_reference"] = all(
            bool(np.array_equal(rag.uv[b], host[b]["uv"]) and np.array_equal(rag.sizes[b], host[b]["size"]) and np.array_equal(rag.counts[b], host[b]["count"])
                 and np.array_equal(rag.min[b], host[b]["min"]) and np.array_equal(rag.max[b], host[b]["max"])
                 and (np.abs(rag.mean[b] - host[b]["mean"]) <= mean_bound(host[b]["mean"]) + 1e-12).all()) for b in range(len(n)))
        del host, rag
        for v in variants:
            if not (full and v == "host"):
                for _ in range(1 if full else a.warmup):
                    step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        if full:
            times["host"].append(host_once)
        for i in range(a.batches):
            for v in variants:
                if i >= batches[v]:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[v]):
                    step(v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / reps[v])
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t), "batches": len(t), "reps": reps[v]} for v, t in times.items()}
        row.update(shape=list(F.shape), offsets=kw["offsets"], capacity=kw["capacity"], torch_over_rag=row["torch"]["median_us"] / row["rag"]["median_us"],
                   host_over_rag=row["host"]["median_us"] / row["rag"]["median_us"], values=values)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step, F, A, Bd
        torch.cuda.empty_cache()
    out = {"kernel_form": "clear, the edge pass (wave peel of pair keys into an open-addressing table), the sample pass (peel, lookup, integer "
                          "atomics), degree by u, one scan per image, scatter, rank within the row and write, stats: eight launches, none "
                          "per edge (csrc/pea_k_rag.hip)",
           "baselines": {"torch": "pair codes, torch.unique(return_inverse), index_add_, searchsorted, scatter_reduce_ on the device (this script)",
                         "host": "device -> host copies of fragments, affinity map and boundary map, tests/rag_reference.py in numpy"},
           "timing": "host clock around calls that end in a device synchronise; medians over alternating batches (the json names batches and reps "
                     "per variant; the numpy reference at the full volume is timed once)",
           "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "kernel_trace" in old:
            out["kernel_trace"] = old["kernel_trace"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
