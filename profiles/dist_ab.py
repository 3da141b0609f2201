#!/usr/bin/env python3
"""Distance-form affinities of a raw embedding (include/pea_dist.h), forward and forward + vjp, two ways in ONE process:

  reference  the reference's op sequence (scripts_ac3ac4/utils/emb2affs.py:6-75) restated with torch ops on the device: per offset a
             replication pad and a slice, a cat of the K shifted copies, one subtraction, a norm over the channels, the affine map, a
             clamp and a square; autograd for the gradient
  pea        pea.emb2affs.embeddings_to_affinities (one launch, csrc/pea_k_dist.hip) and, for the gradient, its vjp launch

on the CVPPP batch (8 x 16 x 544 x 544, the 10 offsets of multi_offset([1, 3, 5, 9, 27], neighbor=4)) and the AC3/AC4 batch
(2 x 16 x 18 x 160 x 160, the 12 offsets of norm5), in f32 and bf16 storage.

After warm-up the legs alternate batch by batch; a batch is `--reps` steps between two readings of the host clock, the second one after
a device synchronise; the median of the batches with the fastest and the slowest, in microseconds per step.  No ratio is fixed in
advance: the medians are recorded as they come.

  python profiles/dist_ab.py [--batches 7] [--reps 10] [--warmup 3] [--out profiles/dist_ab.json]

Kernel times are a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/dist_ab.py --batches 1 --no-reference --out ''"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NORM5 = (1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27)


def shifted(t, off):
    """t at p + off with the index clamped into the volume: the pad and the slice of shift_tensor(t, -off)"""
    pad, sl = [], [slice(None), slice(None)]
    for o in reversed(off):
        pad.extend([max(0, -o), max(0, o)])
    for o, n in zip(off, t.shape[2:]):
        sl.append(slice(o, o + n) if o > 0 else slice(0, n))
    return torch.nn.functional.pad(t, pad, mode="replicate")[tuple(sl)]


def reference_affinities(e, offsets, delta=1.5):
    sh = torch.cat([shifted(e, off).unsqueeze(1) for off in offsets], dim=1)
    affs = (2 * delta - torch.norm(e.unsqueeze(1) - sh, dim=2)) / (2 * delta)
    return torch.clamp(affs, min=0) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_ab.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(83)
    offs3 = [[-s if i % 3 == ax else 0 for ax in range(3)] for i, s in enumerate(NORM5)]
    shapes = (("cvppp_8x16x544x544", (8, 16, 544, 544), [list(o) for o in pkg.multi_offset([1, 3, 5, 9, 27], neighbor=4)]),
              ("ac3ac4_2x16x18x160x160", (2, 16, 18, 160, 160), offs3))
    rows = {}
    for name, shape, offs in shapes:
        if a.only and name != a.only:
            continue
        for dt in (torch.float32, torch.bfloat16):
            e = (0.4 * torch.randn(shape, generator=gen, device=dev)).to(dt).requires_grad_(True)
            up = torch.randn((shape[0], len(offs)) + shape[2:], generator=gen, device=dev)

            def fwd_of(fn):
                def run():
                    with torch.no_grad():
                        return fn(e, offs)
                return run

            def step_of(fn):
                def run():
                    e.grad = None
                    out = fn(e, offs)
                    out.backward(up.to(out.dtype))
                    return e.grad
                return run

            legs = {"fwd_reference": fwd_of(reference_affinities), "fwd_pea": fwd_of(pkg.emb2affs.embeddings_to_affinities),
                    "step_reference": step_of(reference_affinities), "step_pea": step_of(pkg.emb2affs.embeddings_to_affinities)}
            if a.no_reference:
                legs = {k: v for k, v in legs.items() if k.endswith("pea")}
            vals = {}
            for k, fn in legs.items():
                for _ in range(a.warmup):
                    out = fn()
                torch.cuda.synchronize()
                vals[k] = float(out.float().abs().mean())
            times = {k: [] for k in legs}
            for _ in range(a.batches):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e6 / a.reps)
            row = {k: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t)} for k, t in times.items()}
            S = 1
            for v in shape[2:]:
                S *= v
            row.update(shape=list(shape), K=len(offs), dtype=str(dt).replace("torch.", ""), mean_abs=vals,
                       bytes_e_read_affs_written=shape[0] * S * (shape[1] * e.element_size() + 4 * len(offs)))
            if not a.no_reference:
                row.update(reference_over_pea_fwd=row["fwd_reference"]["median_us"] / row["fwd_pea"]["median_us"],
                           reference_over_pea_step=row["step_reference"]["median_us"] / row["step_pea"]["median_us"])
            rows["%s_%s" % (name, row["dtype"])] = row
            print(name, json.dumps(row), flush=True)
            del e, up, legs
            torch.cuda.empty_cache()
    out = {"kernel_form": "gather: one lane per voxel, own channels in registers, neighbour vectors streamed (csrc/pea_k_dist.hip)",
           "reference": "replication pad + slice per offset, cat, subtraction, norm, affine map, clamp, square; autograd: the op sequence of "
                        "scripts_ac3ac4/utils/emb2affs.py:6-75 on the device",
           "clock": "host clock around `reps` steps ending in a device synchronise", "batches": a.batches, "reps_per_batch": a.reps,
           "warmup": a.warmup, "us_per_step": rows, "device": torch.cuda.get_device_name(0)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
