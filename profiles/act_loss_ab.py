#!/usr/bin/env python3
"""The loss on the ACTIVATED affinity map (PEA_FLAG_LOSS_ACT), timed in ONE process through the Python API, forward + backward:
  * headline legs, B=8 x 16 x 544^2, K=10, u8 mask:
      mse              loss_embedding_mse.embedding_loss             (the raw-cosine loss: what the library fused before)
      act_fused        loss_embedding.embedding_loss                 (clamp((cos + 1) / 2, 0, 1), fused: one forward + one backward launch)
      act_exp_fused    loss_embedding_exp.embedding_loss             (clamp(cos, 0, 1), fused)
      act_ema_fused    loss_embedding.ema_embedding_loss             (detached second operand, fused)
      act_foreign      the same loss as act_fused through a criterion the library does not fuse: AffinityMap + K rounds of torch
                       elementwise ops and reductions (what a user had before this flag existed)
  * family legs (for a kernel trace; smaller shapes): xdma_d32, xdma_h_d32_bf16, xdma_h_d32_bf16_crop_f32mask / _u8mask (CROP_ZERO
    border: with an f32 mask the 16-bit forward runs at three workgroups per CU, with a u8 mask at four), tiled_d16 (diagonal
    stencil), and -- with --only
    alone, since its switch holds for the process -- direct_d16 (PEA_FORCE_DIRECT=1).
The legs alternate batch by batch.  Each batch times STEPS steps between two HIP events after warm-up; min and median per step, in ms.

  python profiles/act_loss_ab.py [--batches 7] [--steps 10] [--out FILE] [--only LEG]

--only LEG runs one leg alone: rocprofv3 --kernel-trace --stats -- python profiles/act_loss_ab.py --only xdma_d32"""
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
    cross = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    diag = pkg.multi_offset([1, 3, 9], 8)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    crit = pkg.WeightedMSE()

    def foreign(pred, target, weight):  # WeightedMSE's arithmetic without the `pea_fused` attribute
        return torch.sum(weight * (pred - target) ** 2) / (pred.shape[0] * pred.shape[-1])

    def inputs(B, D, H, W, offsets, dtype=torch.float32, seed=11):
        e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, seed)
        return cu(e).to(dtype), cu(t), cu(w), cu(m), cu(synth.synth_embedding((B, D, H, W), seed + 1)).to(dtype)

    def leg(fn, offsets, ins, criterion=crit, ema=False):
        E, T, Wt, M, other = ins

        def step():
            x = E.detach().requires_grad_(True)
            args = (x, other) if ema else (x,)
            return torch.autograd.grad(fn(*args, T, Wt, M, criterion, offsets)[0], [x])
        return step

    def direct_leg():  # (the switch holds for the whole process: this leg runs with --only alone)
        pkg._lib.set_switch("PEA_FORCE_DIRECT", "1")
        return leg(pkg.loss_embedding.embedding_loss, cross, inputs(4, 16, 256, 256, cross))

    def crop_leg(fmask=True):  # 16-bit storage, CROP_ZERO border, f32 mask: the one LOSS_ACT form at three workgroups per CU
        E, T, Wt, M, _ = inputs(4, 32, 256, 256, cross, torch.bfloat16)
        M = M.float() if fmask else M
        spec = pkg.AffinitySpec(2, cross, None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED, 1e-6, False,
                                pkg._lib.FLAG_HALF_SHIFT | pkg._lib.FLAG_CLAMP01 | pkg._lib.FLAG_LOSS_ACT)

        def step():
            x = E.detach().requires_grad_(True)
            return torch.autograd.grad(pkg.FusedAffinityMSE.apply(x, None, T, Wt, M, spec)[0], [x])
        return step

    head = inputs(8, 16, 544, 544, cross)
    legs = {
        "mse": lambda: leg(pkg.embedding_loss, cross, head),
        "act_fused": lambda: leg(pkg.loss_embedding.embedding_loss, cross, head),
        "act_exp_fused": lambda: leg(pkg.loss_embedding_exp.embedding_loss, cross, head),
        "act_ema_fused": lambda: leg(pkg.loss_embedding.ema_embedding_loss, cross, head, ema=True),
        "act_foreign": lambda: leg(pkg.loss_embedding.embedding_loss, cross, head, criterion=foreign),
        "xdma_d32": lambda: leg(pkg.loss_embedding.embedding_loss, cross, inputs(4, 32, 256, 256, cross)),
        "xdma_h_d32_bf16": lambda: leg(pkg.loss_embedding.embedding_loss, cross, inputs(4, 32, 256, 256, cross, torch.bfloat16)),
        "tiled_d16": lambda: leg(pkg.loss_embedding_exp.embedding_loss, diag, inputs(4, 16, 256, 256, diag)),
        "xdma_h_d32_bf16_crop_f32mask": crop_leg,                     # (65 VGPRs: three workgroups per CU)
        "xdma_h_d32_bf16_crop_u8mask": lambda: crop_leg(False),       # (the same call with a u8 mask: four workgroups per CU)
        "direct_d16": direct_leg,
    }
    runs = {k: mk() for k, mk in legs.items() if a.only == k or (not a.only and k != "direct_d16")}
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
    out = {"headline_shape": "B=8 x 16 x 544^2, K=10", "family_shape": "B=4 x D x 256^2", "batches": a.batches, "steps": a.steps,
           "ms_per_step": res, "device": torch.cuda.get_device_name(0)}
    if "mse" in res and "act_fused" in res:
        out["act_fused_over_mse"] = res["act_fused"]["median_ms"] / res["mse"]["median_ms"]
    if "act_foreign" in res and "act_fused" in res:
        out["act_foreign_over_act_fused"] = res["act_foreign"]["median_ms"] / res["act_fused"]["median_ms"]
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
