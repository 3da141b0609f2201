#!/usr/bin/env python3
"""3D window inference into the stitcher, timed in ONE process through the Python API (VolumeStitcher.add_embedding):
      composed   affinity_infer + fill_border_relu_ + add_vol        (three launches per window: pea_affinity_infer,
                                                                      pea_fill_border_relu, pea_stitch_add)
      fused      pea_affinity_infer_stitch                           (one launch per window, csrc/pea_k_infer_stitch.hip)
each for f32 storage (composed, fused) and f16 storage (composed_f16, fused_f16).  The walk: 27 windows of 1 x 16 x 18 x 160 x 160
(an embedding each) over a 38 x 320 x 320 volume, stride 10 / 80 / 80, norm5, fill_shift 1, relu on.  The legs alternate batch by
batch; each batch times one walk between two HIP events after warm-up; min, median and max per window, in microseconds.  What is
timed is the stream from the first launch to the last, host gaps included (the calls are issued from Python as a user would).
`verdict`: fused's median below composed's by more than the batch-to-batch spread (max - min) of either leg.

  python profiles/infer_stitch_ab.py [--batches 9] [--warmup 2] [--out profiles/infer_stitch_ab.json] [--only LEG]

--only LEG runs one leg alone: rocprofv3 --kernel-trace --stats -- python profiles/infer_stitch_ab.py --only fused"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

D, WIN, VOL, STRIDE = 16, (18, 160, 160), (38, 320, 320), (10, 80, 80)
POS = [(z, y, x) for z in range(0, VOL[0] - WIN[0] + 1, STRIDE[0]) for y in range(0, VOL[1] - WIN[1] + 1, STRIDE[1])
       for x in range(0, VOL[2] - WIN[2] + 1, STRIDE[2])]
BYTES_PER_VOXEL_FUSED = 4 * D + 4 + 8 * 12 + 8   # e, blend weight, out_affs and weight_map read-modify-written
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_stitch_ab.json"))
    a = ap.parse_args()
    assert len(POS) == 27
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    emb = torch.randn((len(POS), D) + WIN, generator=gen, device=dev, dtype=torch.float32)
    emb_h = emb.half()

    def leg(e, fused):
        st = pkg.VolumeStitcher(12, VOL, WIN, dev)

        def walk():
            for b, pos in enumerate(POS):
                st.add_embedding(e[b:b + 1], pos, embedding_mode=5, shift=1, relu=True, fused=fused)
        return walk

    legs = {"composed": lambda: leg(emb, False), "fused": lambda: leg(emb, True),
            "composed_f16": lambda: leg(emb_h, False), "fused_f16": lambda: leg(emb_h, True)}
    runs = {k: mk() for k, mk in legs.items() if not a.only or a.only == k}
    if not runs:
        raise SystemExit("unknown leg %r (one of %s)" % (a.only, ", ".join(legs)))
    for f in runs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.batches):
        for k, f in runs.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            f()
            s1.record()
            torch.cuda.synchronize()
            times[k].append(s0.elapsed_time(s1) * 1e3 / len(POS))
    res = {k: {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v)} for k, v in times.items()}
    voxels = WIN[0] * WIN[1] * WIN[2]
    out = {"shape": "27 windows of 1 x %d x %d x %d x %d over %d x %d x %d, stride %d / %d / %d, norm5, fill_shift 1, relu" %
           ((D,) + WIN + VOL + STRIDE), "batches": a.batches, "warmup": a.warmup, "us_per_window": res,
           "device": torch.cuda.get_device_name(0)}
    for c, f in (("composed", "fused"), ("composed_f16", "fused_f16")):
        if c in res and f in res:
            gain = res[c]["median_us"] - res[f]["median_us"]
            spread = max(res[c]["max_us"] - res[c]["min_us"], res[f]["max_us"] - res[f]["min_us"])
            out[f + "_verdict"] = {"median_gain_us": gain, "largest_spread_us": spread, "composed_over_fused": res[c]["median_us"] / res[f]["median_us"],
                                   "fused_faster_beyond_spread": bool(gain > spread)}
    if "fused" in res:
        floor_us = BYTES_PER_VOXEL_FUSED * voxels / HBM_PEAK * 1e6
        out["fused_floor_us_at_172B_per_voxel_8TBps"] = floor_us
        out["fused_fraction_of_floor"] = floor_us / res["fused"]["median_us"]
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
