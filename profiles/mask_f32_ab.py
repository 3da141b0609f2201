#!/usr/bin/env python3
"""Float32 loss masks (PEA_FLAG_MASK_F32), timed in ONE process through the Python API:
  * the CVPPP loss section (scripts_cvppp/main.py:284-310, B=8 x 16 x 544^2, nb_half = 2) fed with packed float downN tensors whose
    mask thirds are channel slices -- cvppp_loss_section (one autograd node) and cvppp_loss_section_composed (call by call), eager and
    graphed (pea.graphed), forward + backward;
  * the headline forward + backward (embedding_loss, B=8 x 16 x 544^2, K=10) with a u8 mask against an f32 mask of the same values.
The legs alternate batch by batch.  Each batch times STEPS steps between two HIP events after warm-up; min and median per step, in ms.

  python profiles/mask_f32_ab.py [--batches 7] [--steps 10] [--out FILE] [--only LEG]

Runs on any tree of the package (the parent commit converts float masks to u8 inside the section: that is the "before").
--only LEG runs one leg alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python profiles/mask_f32_ab.py --only one_node)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half, B, D, H, W = 2, 8, 16, 544, 544
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, 11)
    E, T, Wt, M8 = cu(e), cu(t), cu(w), cu(m)
    Mf = M8.float()
    ema = cu(synth.synth_embedding((B, D, H, W), 12))
    emds, downs = [], []
    for j in range(4):
        k = nb_half * (4 - j)
        ej, tj, wj, mj = synth.synth_inputs_2d(B, D, H >> (j + 1), W >> (j + 1), offsets[:k], 13 + j)
        emds.append(cu(ej))
        downs.append(cu(np.concatenate([tj, wj, mj.astype(np.float32)], axis=1)))
    crit = pkg.WeightedMSE()

    def section(fn):
        def step(E, *rest):
            x = E.detach().requires_grad_(True)
            xs = [r.detach().requires_grad_(True) for r in rest]
            loss, pred, _ = fn(x, xs, ema, T, Wt, Mf, downs, crit, offsets, nb_half)
            return torch.autograd.grad(loss, [x] + xs)
        return step

    def headline(M):
        def step(E):
            x = E.detach().requires_grad_(True)
            loss, affs, _ = pkg.embedding_loss(x, T, Wt, M, crit, offsets)
            return torch.autograd.grad(loss, [x])
        return step

    legs = {"one_node": (section(pkg.cvppp_loss_section), [E] + emds), "composed": (section(pkg.cvppp_loss_section_composed), [E] + emds),
            "headline_u8": (headline(M8), [E]), "headline_f32": (headline(Mf), [E])}
    runs = {}
    for name, (fn, args) in legs.items():
        if a.only and a.only not in name:
            continue
        runs[name + "_eager"] = (lambda fn=fn, args=args: fn(*args))
        if name in ("one_node", "composed"):
            g = pkg.graphed(fn, *args)
            runs[name + "_graphed"] = g.replay
    for f in runs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.batches):
        for k, f in runs.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.steps):
                f()
            s1.record()
            torch.cuda.synchronize()
            times[k].append(s0.elapsed_time(s1) / a.steps)
    res = {k: {"min_ms": min(v), "median_ms": statistics.median(v)} for k, v in times.items()}
    out = {"shape": "B=%d x %d x %d^2, K=10, nb_half=%d" % (B, D, H, nb_half), "batches": a.batches, "steps": a.steps, "ms_per_step": res,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
