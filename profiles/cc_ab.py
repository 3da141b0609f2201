#!/usr/bin/env python3
"""Connected components with a size filter (include/pea_cc.h: pea_cc_label), timed in ONE process against what the validation loop does
today with a mask that is on the device:

  cc          pea.connected_components(x, connectivity, min_size, mask=True) on a device tensor: the seven launches of
              csrc/pea_k_cc.hip; labels, counts and mask stay on the device
  cc_mask     pea.remove_small_components (pea_cc_label with mask_out only: what pea.foreground_mask(min_size=...) and
              remove_samll_object run)
  cc_graphed  `cc` captured with pea.graphed and replayed
  host        device -> host copy of the mask, scipy.ndimage.label + numpy.bincount + threshold on the host, the filtered mask copied
              back to the device (scipy stands in for skimage; where scipy is missing, the numpy restatement tests/cc_reference.py
              runs in its place and the json says so)

on three shapes: one 520 x 696 mask with about 150 nuclei and 200 specks (connectivity 2, min_size 25: remove_samll_object's call), eight
256 x 256 masks with about 40 nuclei each (the same call), and one 18 x 160 x 160 volume of balls at connectivity 1.

Every call is timed by a host clock around work that ends in a device synchronise.  After warm-up the variants alternate batch by batch;
a batch times `--reps` calls; min, median and max of the batches in microseconds per call.  Recorded, not gated.  The launches' shares of
the device time come from a kernel trace, a run of its own:

  python profiles/cc_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/cc_ab.json] [--only LEG]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/cc_ab.py --trace LEG --steps 50
  python profiles/cc_ab.py --merge-trace DIR --trace LEG --steps 50     (adds the kernels' average times to the json)"""
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
from cc_reference import NEIGHBOURS, cc_reference_batch  # noqa: E402

try:
    from scipy import ndimage as ndi
    HOST_PATH = "scipy.ndimage.label + numpy.bincount + threshold"
except ImportError:
    ndi = None
    HOST_PATH = "tests/cc_reference.py (numpy / Python flood fill: scipy is not installed here)"


def balls(seed, Z, Y, X, n, radius):
    """a uint8 volume of n balls of about `radius` voxels"""
    rng = np.random.default_rng(seed)
    out = np.zeros((Z, Y, X), np.uint8)
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    for cz, cy, cx, r in zip(rng.integers(0, Z, n), rng.integers(0, Y, n), rng.integers(0, X, n), rng.integers(radius - 2, radius + 3, n)):
        out[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return out


def host_filter(mask, connectivity, min_size):
    """one image on the host -> the mask of its components of at least min_size pixels"""
    if ndi is None:
        return (cc_reference_batch(mask[None], connectivity, min_size)[0][0] != 0).astype(np.uint8)
    lab, _ = ndi.label(mask, structure=ndi.generate_binary_structure(mask.ndim, connectivity))
    keep = np.bincount(lab.ravel()) >= min_size
    keep[0] = False
    return keep[lab].astype(np.uint8)


LEGS = {"bbbc_1x520x696": dict(shape=(1, 520, 696), connectivity=2, min_size=25),
        "bbbc_8x256x256": dict(shape=(8, 256, 256), connectivity=2, min_size=25),
        "vol_1x18x160x160": dict(shape=(1, 18, 160, 160), connectivity=1, min_size=25)}


def make_mask(synth, name):
    if name == "bbbc_1x520x696":
        return (synth.synth_nuclei(1, 520, 696, 150, 14, 39, specks=200) > 0).astype(np.uint8)
    if name == "bbbc_8x256x256":
        return (synth.synth_nuclei(8, 256, 256, 40, 12, 41, specks=40) > 0).astype(np.uint8)
    return balls(43, 18, 160, 160, 60, 7)[None]


def make_leg(pkg, dev, mask, connectivity, min_size):
    X = torch.from_numpy(mask).to(dev)
    graph = []

    def step(variant):
        if variant == "cc":
            return pkg.connected_components(X, connectivity=connectivity, min_size=min_size, mask=True).mask
        if variant == "cc_mask":
            return pkg.remove_small_components(X, min_size, connectivity)
        if variant == "cc_graphed":
            if not graph:
                graph.append(pkg.graphed(lambda X: (pkg.connected_components(X, connectivity=connectivity, min_size=min_size, mask=True).mask,), X))
            return graph[0].replay()[0]
        host = X.cpu().numpy()
        return torch.from_numpy(np.stack([host_filter(m, connectivity, min_size) for m in host])).to(dev)
    return step


WARM_TRACE = 3  # calls the --trace run makes before its --steps (all of them are in the trace)


def trace_run(a):
    """what the kernel trace sees: WARM_TRACE + --steps eager calls of one leg"""
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    kw = LEGS[a.trace]
    step = make_leg(pkg, torch.device("cuda:0"), make_mask(synth, a.trace), kw["connectivity"], kw["min_size"])
    for _ in range(WARM_TRACE + a.steps):
        step("cc")
    torch.cuda.synchronize()


def merge_trace(a):
    """kernel_stats.csv of the traced run -> the kernels' average times, into the json"""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = [{"kernel": r["Name"][:100], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) * 1e-3} for r in csv.DictReader(open(paths[0]))]
    per_call = [r for r in rows if r["calls"] == calls and "k_cc_" in r["kernel"]]
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/cc_ab.py --trace %s --steps %d" % (a.trace, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(per_call, key=lambda r: -r["average_us"]),
        "device_us_per_call": sum(r["average_us"] for r in per_call)}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc["kernel_trace"][a.trace], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only")
    ap.add_argument("--trace")
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cc_ab.json"))
    a = ap.parse_args()
    for name in (a.only, a.trace):
        if name and name not in LEGS:
            raise SystemExit("unknown leg %r (one of %s)" % (name, ", ".join(LEGS)))
    if a.merge_trace:
        return merge_trace(a)
    assert torch.cuda.is_available(), "cc_ab.py measures on an MI355X: there is no CPU fallback"
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    variants = ["cc", "cc_mask", "cc_graphed", "host"]
    rows = {}
    for name, kw in LEGS.items():
        if a.only and a.only != name:
            continue
        mask = make_mask(synth, name)
        assert mask.shape == kw["shape"]
        c, ms = kw["connectivity"], kw["min_size"]
        assert (mask.ndim - 1, c) in NEIGHBOURS
        step = make_leg(pkg, dev, mask, c, ms)
        cc = pkg.connected_components(torch.from_numpy(mask).to(dev), connectivity=c, min_size=ms, mask=True)
        ref_labels, ref_counts = cc_reference_batch(mask, c, ms)
        host_mask = step("host").cpu().numpy()
        values = {"connectivity": c, "min_size": ms, "foreground_share": float(mask.mean()),
                  "components_found_per_image": cc.counts[:, 0].tolist(), "components_kept_per_image": cc.counts[:, 1].tolist(),
                  "labels_equal_restatement": bool(np.array_equal(cc.labels.cpu().numpy(), ref_labels)),
                  "counts_equal_restatement": bool(np.array_equal(cc.counts.cpu().numpy(), ref_counts)),
                  "mask_equal_host_path": bool(np.array_equal(cc.mask.cpu().numpy(), host_mask))}
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
        row.update(shape=list(mask.shape), host_over_cc=row["host"]["median_us"] / row["cc"]["median_us"],
                   host_over_cc_graphed=row["host"]["median_us"] / row["cc_graphed"]["median_us"], values=values)
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step
        torch.cuda.empty_cache()
    out = {"kernel_form": "32 x 32 tiles of one plane labelled in LDS by label equivalence, a lock-free union across the tile borders "
                          "(the z step is one more border), compress and count with a wave peel, a three-step scan, the write: seven "
                          "launches, none per component (csrc/pea_k_cc.hip)",
           "host_path": "device -> host copy, " + HOST_PATH + ", host -> device copy of the filtered mask",
           "timing": "host clock around calls that end in a device synchronise; medians over alternating batches",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
