#!/usr/bin/env python3
"""The instance scores of the BBBC039V1 validation loop (AJI, DQ / SQ / PQ, pixel F1), timed in ONE process:

  inst          pea.instance_scores on device label images with max_id given (include/pea_instscore.h: the streaming pass, two passes
                over the table's slots, a scan, the AJI walk, a finish); the [B, 18] table and the match tables stay on the device
  inst_default  the same with max_id left at its device default, 65535 (the dense arrays and the match tables are 64 K ids long)
  inst_graphed  `inst` captured with pea.graphed and replayed
  inst_upload   the same from numpy label images (the segmentation comes from elf on the host): upload, call, the table read back
  seg           pea.segmentation_scores at the same shape: it runs the same streaming pass, so its time is the floor below which only
                the added passes and the walk remain
  host          the reference's op sequence restated in numpy below (host_*): one full-image mask per gt instance and a full-image
                comparison per (gt instance, pred id) for the AJI, one mask per id and a loop over overlapping pairs for PQ

on two shapes: one 520 x 696 image with about 150 nuclei on each side, and eight 256 x 256 crops with about 40.

Every call is timed by a host clock around work that ends in a device synchronise (the host variant has no device work).  After
warm-up the variants alternate batch by batch; a batch times `--reps` calls (the host variant one); min, median and max of the batches
in microseconds per call.  Recorded, not gated.  The walk's share of the device time comes from a kernel trace, a run of its own:

  python profiles/instscore_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/instscore_ab.json] [--only LEG]
  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/instscore_ab.py --trace LEG --steps 50
  python profiles/instscore_ab.py --merge-trace DIR --trace LEG --steps 50     (adds the kernels' average times to the json)"""
import argparse
import csv
import glob
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
from instscore_reference import COL, inst_reference  # noqa: E402

SHOWN = ("aji", "dq", "sq", "pq", "pixel_f1")
WARM_TRACE = 3  # calls the --trace run makes before its --steps (all of them are in the trace)


def nuclei(seed, B, Y, X, n, radius, jitter=0, drop=0):
    """B images of about n discs of about `radius` pixels, later ones over earlier ones, ids 1 .. in drawing order; jitter / drop: the
    same discs moved by up to `jitter` pixels with `drop` of them left out (a prediction of the image with jitter = drop = 0)"""
    out = np.zeros((B, Y, X), np.int32)
    yy, xx = np.mgrid[0:Y, 0:X]
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        cy, cx, r = rng.integers(0, Y, n), rng.integers(0, X, n), rng.integers(radius - 3, radius + 4, n)
        move = np.random.default_rng(seed + 1000 + b)
        dy, dx = move.integers(-jitter, jitter + 1, n), move.integers(-jitter, jitter + 1, n)
        keep = move.permutation(n)[drop:]
        for new, k in enumerate(sorted(keep.tolist())):
            y0, y1 = max(0, cy[k] + dy[k] - r[k]), min(Y, cy[k] + dy[k] + r[k] + 1)
            x0, x1 = max(0, cx[k] + dx[k] - r[k]), min(X, cx[k] + dx[k] + r[k] + 1)
            disc = (yy[y0:y1, x0:x1] - cy[k] - dy[k]) ** 2 + (xx[y0:y1, x0:x1] - cx[k] - dx[k]) ** 2 <= r[k] ** 2
            out[b, y0:y1, x0:x1][disc] = new + 1
        ids, inverse = np.unique(out[b], return_inverse=True)  # a disc that later ones cover leaves no gap in the ids
        out[b] = (np.arange(len(ids)) if ids[0] == 0 else np.arange(1, len(ids) + 1))[inverse].reshape(Y, X)
    return out


# ---- the reference's op sequence on the host ------------------------------------------------------------------------------------------------
def host_aji(gt, pred):
    n_pred = int(pred.max())
    used = np.zeros(n_pred + 1, bool)
    c = u = 0
    for j in range(1, int(gt.max()) + 1):
        m = gt == j
        inter, union = np.zeros(n_pred, np.int64), np.zeros(n_pred, np.int64)
        for i in range(1, n_pred + 1):
            if used[i]:
                union[i - 1] = np.count_nonzero(m)
            else:
                p = pred == i
                inter[i - 1] = np.count_nonzero(m & p)
                union[i - 1] = np.count_nonzero(m) + np.count_nonzero(p) - inter[i - 1]
        hit = int(np.argmax(inter / union))
        c, u = c + inter[hit], u + union[hit]
        used[hit + 1] = True
    u += sum(int(np.sum(pred == i)) for i in np.unique(pred) if i > 0 and not used[i])
    return c / u


def host_pq(gt, pred, match_iou=0.5):
    t_ids, p_ids = np.unique(gt)[1:], np.unique(pred)[1:]
    t_masks = {int(t): (gt == t).astype(np.uint8) for t in t_ids}
    p_masks = {int(p): (pred == p).astype(np.uint8) for p in p_ids}
    ious = []
    for t, tm in t_masks.items():
        for p in np.unique(pred[tm > 0]):
            if p:
                inter = int((tm * p_masks[int(p)]).sum())
                iou = inter / (int((tm + p_masks[int(p)]).sum()) - inter)
                if iou > match_iou:
                    ious.append(iou)
    tp = len(ious)
    dq = tp / (tp + 0.5 * (len(p_ids) - tp) + 0.5 * (len(t_ids) - tp))
    sq = float(np.sum(ious)) / (tp + 1.0e-6)
    return dq, sq, dq * sq


def host_f1(gt, pred):
    tp, fp, fn = np.count_nonzero((pred > 0) & (gt > 0)), np.count_nonzero((pred > 0) & (gt == 0)), np.count_nonzero((pred == 0) & (gt > 0))
    return 2.0 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0


def host_scores(pred, gt):
    return np.array([[host_aji(g, p)] + list(host_pq(g, p)) + [host_f1(g, p)] for p, g in zip(pred, gt)])


LEGS = {"bbbc_1x520x696": dict(B=1, Y=520, X=696, n=150, radius=14), "bbbc_8x256x256": dict(B=8, Y=256, X=256, n=40, radius=12)}


def make_leg(pkg, dev, B, Y, X, n, radius):
    gt = nuclei(700, B, Y, X, n, radius)
    pred = nuclei(700, B, Y, X, n, radius, jitter=3, drop=max(1, n // 20))
    max_id = int(max(pred.max(), gt.max()))
    P, G = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    graph = []

    def step(variant):
        if variant == "inst":
            return pkg.instance_scores(P, G, max_id=max_id).table
        if variant == "inst_default":
            return pkg.instance_scores(P, G).table
        if variant == "inst_graphed":
            if not graph:
                graph.append(pkg.graphed(lambda P, G: (pkg.instance_scores(P, G, max_id=max_id).table,), P, G))
            return graph[0].replay()[0]
        if variant == "inst_upload":
            return pkg.instance_scores(pred, gt).table.cpu()
        if variant == "seg":
            return pkg.segmentation_scores(P, G).table
        return host_scores(pred, gt)
    return step, pred, gt, max_id


def trace_run(a):
    """what the kernel trace sees: WARM_TRACE + --steps eager calls of one leg"""
    pkg = ge.load_package()
    step = make_leg(pkg, torch.device("cuda:0"), **LEGS[a.trace])[0]
    for _ in range(WARM_TRACE + a.steps):
        step("inst")
    torch.cuda.synchronize()


def merge_trace(a):
    """kernel_stats.csv of the traced run -> the kernels' average times and the walk's share, into the json"""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_stats.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_stats.csv under %s, found %d" % (a.merge_trace, len(paths)))
    calls = a.steps + WARM_TRACE
    rows = [{"kernel": r["Name"][:120], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) * 1e-3} for r in csv.DictReader(open(paths[0]))]
    per_call = [r for r in rows if r["calls"] == calls and ("k_inst" in r["kernel"] or "k_seg_pairs" in r["kernel"])]
    total = sum(r["average_us"] for r in per_call)
    walk = sum(r["average_us"] for r in per_call if "k_inst_walk" in r["kernel"])
    doc = json.load(open(a.out))
    doc.setdefault("kernel_trace", {})[a.trace] = {
        "command": "rocprofv3 --kernel-trace --stats -- python profiles/instscore_ab.py --trace %s --steps %d" % (a.trace, a.steps),
        "calls_in_trace": calls, "kernels_of_a_call": sorted(per_call, key=lambda r: -r["average_us"]), "device_us_per_call": total,
        "walk_us_per_call": walk, "walk_share_of_device_time": walk / total if total else None}
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
    ap.add_argument("--no-host", action="store_true", help="leave the host variant out (it takes tens of seconds per call at 520 x 696)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instscore_ab.json"))
    a = ap.parse_args()
    for name in (a.only, a.trace):
        if name and name not in LEGS:
            raise SystemExit("unknown leg %r (one of %s)" % (name, ", ".join(LEGS)))
    if a.merge_trace:
        return merge_trace(a)
    if a.trace:
        return trace_run(a)
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    variants = ["inst", "inst_default", "inst_graphed", "inst_upload", "seg"] + ([] if a.no_host else ["host"])
    rows = {}
    for name, kw in LEGS.items():
        if a.only and a.only != name:
            continue
        step, pred, gt, max_id = make_leg(pkg, dev, **kw)
        ref = inst_reference(pred.reshape(kw["B"], -1), gt.reshape(kw["B"], -1), max_id)[0]
        hip = step("inst").cpu().numpy()
        values = {"n_pred_ids_per_image": [int(v) for v in ref[:, COL["n_pred_ids"]]], "n_gt_ids_per_image": [int(v) for v in ref[:, COL["n_gt_ids"]]],
                  "max_id": max_id, "capacity": pkg.instance_scores(pred, gt).capacity, "n_overflow": [int(v) for v in hip[:, 0]],
                  "aji": [float(v) for v in hip[:, COL["aji"]]], "pq": [float(v) for v in hip[:, COL["pq"]]],
                  "max_abs_hip_minus_restatement": {c: float(np.abs(hip[:, COL[c]] - ref[:, COL[c]]).max()) for c in SHOWN}}
        if not a.no_host:
            t0 = time.perf_counter()
            host = host_scores(pred, gt)  # (also the host variant's warm-up)
            values["host_first_call_s"] = time.perf_counter() - t0
            values["max_abs_hip_minus_host"] = {c: float(np.abs(hip[:, COL[c]] - host[:, i]).max()) for i, c in enumerate(SHOWN)}
        reps = {v: (1 if v == "host" else a.reps) for v in variants}
        for v in variants:
            for _ in range(0 if v == "host" else a.warmup):
                step(v)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for k in range(a.batches):
            for v in variants:
                if v == "host" and k >= 3:  # three batches of the host variant: it is five orders of magnitude away
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[v]):
                    step(v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / reps[v])
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for v, t in times.items()}
        row.update(shape=list(pred.shape), inst_minus_seg_us=row["inst"]["median_us"] - row["seg"]["median_us"],
                   graphed_minus_seg_us=row["inst_graphed"]["median_us"] - row["seg"]["median_us"], values=values)
        if not a.no_host:
            row["host_over_inst_upload"] = row["host"]["median_us"] / row["inst_upload"]["median_us"]
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del step
        torch.cuda.empty_cache()
    out = {"kernel_form": "the streaming pass of the segmentation scores (pea_segtable.h), dense marginals by id, a CSR of the table by gt id "
                          "from one scan per image, the AJI walk on one wave per image with the used set in LDS (csrc/pea_k_instscore.hip)",
           "timing": "host clock around calls that end in a device synchronise; medians over alternating batches",
           "batches": a.batches, "reps_per_batch": a.reps, "host_reps_per_batch": 1, "host_batches": min(3, a.batches), "warmup": a.warmup,
           "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
