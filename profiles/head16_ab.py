#!/usr/bin/env python3
"""The embedding head on 16-bit features (include/pea_head16.h, csrc/pea_head.h) against the f32 head and against torch's convolution
under autocast, timed in ONE process at the shapes of the reference's heads:

  cvppp_B8     8 x 32 -> 16 x 544^2        (OutConv, CVPPP)
  bbbc_B8      8 x 32 -> 32 x 704^2        (OutConv, BBBC039V1)
  ac3ac4_B2    2 x 28 -> 16 x 18 x 160^2   (conv3dBlock 1x1x1, AC3/AC4)

forward and backward separately, for
  f32          pea_head_fwd / pea_head_bwd on f32 features (what the package did so far)
  hip_f16      pea_head_fwd_t / pea_head_bwd_t, x and e in f16, W / bias / dW / db f32
  hip_bf16     the same in bf16
  torch_f16    F.conv2d / F.conv3d inside torch.autocast(dtype=f16) on the same f16 features with the f32 parameters (the cast of the
               weight included: it is what a user's step pays); backward = torch.autograd.grad of (x, weight, bias)
  torch_bf16   the same in bf16

The HIP calls go through the C ABI (workspace allocated once), so a batch holds kernel time and launch gaps only.  After warm-up the
variants alternate batch by batch; a batch times `--reps` calls between two HIP events; min, median and max of the batches in
microseconds per call.  GB/s on the algorithmic bytes: 2(C+D) / 2(2C+D) bytes per pixel for the 16-bit variants, 4(C+D) / 4(2C+D) for f32.
`hip_faster_beyond_spread`: the HIP median below torch's by more than the batch-to-batch spread (max - min) of either -- the routing
rule of model/head.py: a (C, D, type) for which this is false in either direction stays on torch's convolution.

  python profiles/head16_ab.py [--batches 7] [--reps 20] [--warmup 3] [--out profiles/head16_ab.json] [--only LEG]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LEGS = {"cvppp_B8": (8, 32, 16, (544, 544)), "bbbc_B8": (8, 32, 32, (704, 704)), "ac3ac4_B2": (2, 28, 16, (18, 160, 160))}
VARIANTS = ["f32", "hip_f16", "hip_bf16", "torch_f16", "torch_bf16"]
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head16_ab.json"))
    a = ap.parse_args()
    if a.only and a.only not in LEGS:
        raise SystemExit("unknown leg %r (one of %s)" % (a.only, ", ".join(LEGS)))
    pkg = ge.load_package()
    L = pkg._lib.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(31)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = {torch.float16: pkg._lib.F16, torch.bfloat16: pkg._lib.BF16}

    def leg(B, C, D, sp):
        S = 1
        for v in sp:
            S *= v
        x32 = torch.randn((B, C) + sp, generator=gen, device=dev)
        de32 = torch.randn((B, D) + sp, generator=gen, device=dev)
        W = torch.randn((D, C), generator=gen, device=dev) * 0.2
        bias = torch.randn(D, generator=gen, device=dev)
        wsb = L.pea_head_workspace_bytes(C, D)
        work = torch.empty(wsb // 4, device=dev)
        dW, db = torch.empty_like(W), torch.empty_like(bias)
        conv = F.conv3d if len(sp) == 3 else F.conv2d
        wconv = W.reshape((D, C) + (1,) * len(sp)).clone().requires_grad_(True)
        bconv = bias.clone().requires_grad_(True)
        steps = {}
        e32, dx32 = torch.empty_like(de32), torch.empty_like(x32)
        steps["f32"] = (lambda: pkg._lib.check(L.pea_head_fwd(B, C, D, S, p(x32), p(W), p(bias), p(e32), st), "fwd"),
                        lambda: pkg._lib.check(L.pea_head_bwd(B, C, D, S, p(x32), p(W), p(de32), p(dx32), p(dW), p(db), p(work), wsb, st), "bwd"))
        keep = []
        for name, dt in DT.items():
            x, de = x32.to(dt), de32.to(dt)
            e, dx = torch.empty_like(de), torch.empty_like(x)
            c = code[dt]
            steps["hip_" + name] = (
                lambda x=x, e=e, c=c: pkg._lib.check(L.pea_head_fwd_t(B, C, D, S, p(x), c, p(W), p(bias), p(e), c, st), "fwd_t"),
                lambda x=x, de=de, dx=dx, c=c: pkg._lib.check(L.pea_head_bwd_t(B, C, D, S, p(x), c, p(W), p(de), c, p(dx), p(dW), p(db), p(work),
                                                                                 wsb, st), "bwd_t"))
            xg = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=dt):
                eg = conv(xg, wconv, bconv)
            assert eg.dtype == dt

            def tfwd(x=x, dt=dt):
                with torch.autocast("cuda", dtype=dt), torch.no_grad():
                    return conv(x, wconv, bconv)

            steps["torch_" + name] = (tfwd, lambda eg=eg, xg=xg, de=de: torch.autograd.grad(eg, (xg, wconv, bconv), de, retain_graph=True))
            keep.append((x, de, e, dx, xg, eg))
            # the two agree (a loose look: torch rounds the weight to the 16-bit type first)
            steps["hip_" + name][0]()
            ref = tfwd()
            assert float((e.float() - ref.float()).abs().max()) <= 0.05 * float(ref.float().abs().max())
        return steps, S, keep

    rows = {}
    for name, (B, C, D, sp) in LEGS.items():
        if a.only and a.only != name:
            continue
        steps, S, keep = leg(B, C, D, sp)
        row = {"shape": [B, C, D] + list(sp)}
        for k, direction in enumerate(("forward", "backward")):
            for v in VARIANTS:
                for _ in range(a.warmup):
                    steps[v][k]()
            torch.cuda.synchronize()
            times = {v: [] for v in VARIANTS}
            for _ in range(a.batches):
                for v in VARIANTS:
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    for _ in range(a.reps):
                        steps[v][k]()
                    s1.record()
                    torch.cuda.synchronize()
                    times[v].append(s0.elapsed_time(s1) * 1e3 / a.reps)
            res = {}
            for v, t in times.items():
                per_px = (C + D) if k == 0 else (2 * C + D)
                nbytes = (4 if v == "f32" else 2) * per_px * B * S
                med = statistics.median(t)
                res[v] = {"min_us": min(t), "median_us": med, "max_us": max(t), "algorithmic_bytes": nbytes, "GBps": nbytes / med * 1e-3}
            for n in DT:
                h, t = res["hip_" + n], res["torch_" + n]
                gain = t["median_us"] - h["median_us"]
                spread = max(t["max_us"] - t["min_us"], h["max_us"] - h["min_us"])
                res["hip_%s_vs_torch" % n] = {"median_gain_us": gain, "largest_spread_us": spread, "torch_over_hip": t["median_us"] / h["median_us"],
                                             "hip_faster_beyond_spread": bool(gain > spread), "f32_over_hip": res["f32"]["median_us"] / h["median_us"]}
            row[direction] = res
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del steps, keep
        torch.cuda.empty_cache()
    out = {"kernel_form": "two x-adjacent pixels per lane as one dword (S even, 4-byte aligned tensors), rows kept packed in registers, "
                          "dW on v_mfma_f32_16x16x4_f32 after widening (csrc/pea_head.h)",
           "torch": "F.conv2d / F.conv3d under torch.autocast on the 16-bit features with f32 parameters; backward = autograd.grad(x, weight, bias)",
           "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
