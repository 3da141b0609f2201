#!/usr/bin/env python3
"""f32 / f16 / bf16 embedding storage, A/B in ONE process: embedding_loss forward + backward through the Python API, the three dtypes
alternating batch by batch so that clock and thermal drift land on all three alike.  Shapes: BASELINE configs[4] (B=8 x 64 x 544^2,
offsets[:8]) and the headline shape (B=8 x 16 x 544^2, K=10).  Each batch times STEPS steps between two HIP events after warm-up;
min and median over the batches are per step, in ms.

  python profiles/bf16_ab.py [--batches 9] [--steps 10] [--out profiles/bf16_ab.json] [--only bf16]

--only DTYPE runs that dtype alone (for a kernel-trace run: rocprofv3 --kernel-trace --stats -- python profiles/bf16_ab.py --only bf16)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(DTYPES))
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = ge.load_package()
    import importlib
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    shapes = {"configs4_B8x64x544sq_K8": (8, 64, 544, 544, cv[:8]), "headline_B8x16x544sq_K10": (8, 16, 544, 544, cv)}
    dts = [a.only] if a.only else list(DTYPES)
    crit = pkg.WeightedMSE()
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "steps_per_batch": a.steps, "unit": "ms per step", "shapes": {}}
    for sname, (B, D, H, W, offs) in shapes.items():
        e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offs, 7)
        T, Wt, M = (torch.from_numpy(x).to(dev) for x in (t, w, m))
        E = {k: torch.from_numpy(e).to(dev).to(DTYPES[k]).requires_grad_(True) for k in dts}
        del e

        def step(k):
            x = E[k]
            x.grad = None
            loss, _, _ = pkg.embedding_loss(x, T, Wt, M, crit, offs)
            loss.backward()

        for k in dts:
            for _ in range(a.warmup):
                step(k)
        torch.cuda.synchronize()
        times = {k: [] for k in dts}
        for _ in range(a.batches):
            for k in dts:
                s, f = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.steps):
                    step(k)
                f.record()
                f.synchronize()
                times[k].append(s.elapsed_time(f) / a.steps)
        r = {k: {"min": min(v), "median": statistics.median(v), "all": [round(x, 4) for x in v]} for k, v in times.items()}
        if "bf16" in r and "f16" in r:
            r["bf16_over_f16_min"] = r["bf16"]["min"] / r["f16"]["min"]
            r["bf16_over_f16_median"] = r["bf16"]["median"] / r["f16"]["median"]
        res["shapes"][sname] = r
        print(sname, json.dumps({k: (v if not isinstance(v, dict) else {"min": round(v["min"], 4), "median": round(v["median"], 4)})
                                 for k, v in r.items()}), flush=True)
        del E, T, Wt, M
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
